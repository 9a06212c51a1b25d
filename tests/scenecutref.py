"""The scene-cut detector and the encoder's key-frame policy of include/h264mi.h restated in numpy:
the reference of the GPU tests, with no import from the library. Exact integers, so every comparison with the device is
equality of bytes and words.

A frame is a flat uint8 array of a tight w x h I420 picture (only its luma is read); params is
(level, share, min_gap, max_gap, compensate).
  thumbnail(frame, w, h)                    -> th x tw uint8, vectorised;  thumbnail_loops: the same as plain loops
  block_stats(tc, tp, params)               -> (per-block sad, dsum, changed), vectorised
  frame_stats(tc, tp, params)               -> the frame's eight words;    frame_stats_loops: the same as plain loops
  is_cut(params, stats)                     -> the cut test
  policy_sequence(frames, w, h, params, forced=set()) -> per frame (key, reason, dist), with the stream's first frame at
                                               index 0 and a host force_idr in front of every frame in `forced`
  policy_states(...)                        -> the same walk, per frame the sixteen words of h264mi_enc_scenecut_state"""
import numpy as np

DEFAULT = (64, 128, 4, 0, 1)


def frame_bytes(w, h):
    return w * h + 2 * (w // 2) * (h // 2)


def thumb_size(w, h):
    return (w + 3) // 4, (h + 3) // 4


def params_ok(params):
    level, share, min_gap, max_gap, comp = params
    return 0 <= level <= 1020 and 0 <= share <= 256 and 0 <= min_gap <= 65535 and 0 <= max_gap <= 65535 and comp in (0, 1)


def thumbnail(frame, w, h):
    assert w % 2 == 0 and h % 2 == 0 and frame.size >= w * h
    tw, th = thumb_size(w, h)
    Y = np.zeros((4 * th, 4 * tw), np.int64)
    Y[:h, :w] = np.asarray(frame[:w * h]).reshape(h, w)
    s = Y.reshape(th, 4, tw, 4).sum(axis=(1, 3))
    cw = np.minimum(4, w - 4 * np.arange(tw))
    ch = np.minimum(4, h - 4 * np.arange(th))
    npix = ch[:, None] * cw[None, :]
    return ((s + npix // 2) // npix).astype(np.uint8)


def thumbnail_loops(frame, w, h):
    tw, th = thumb_size(w, h)
    T = np.zeros((th, tw), np.uint8)
    for cy in range(th):
        for cx in range(tw):
            s = n = 0
            for y in range(4 * cy, min(4 * cy + 4, h)):
                for x in range(4 * cx, min(4 * cx + 4, w)):
                    s += int(frame[y * w + x])
                    n += 1
            T[cy][cx] = (s + n // 2) // n
    return T


def _blocks(a):
    """a (th x tw, int64) summed over blocks of 8 x 8 cells"""
    th, tw = a.shape
    nbx, nby = (tw + 7) // 8, (th + 7) // 8
    p = np.zeros((8 * nby, 8 * nbx), np.int64)
    p[:th, :tw] = a
    return p.reshape(nby, 8, nbx, 8).sum(axis=(1, 3))


def block_stats(tc, tp, params):
    level, _, _, _, comp = params
    th, tw = tc.shape
    c, p = tc.astype(np.int64), tp.astype(np.int64)
    sad = _blocks(np.abs(c - p))
    dsum = np.abs(_blocks(c) - _blocks(p))
    bw = np.minimum(8, tw - 8 * np.arange((tw + 7) // 8))
    bh = np.minimum(8, th - 8 * np.arange((th + 7) // 8))
    m = sad - dsum if comp else sad
    return sad, dsum, 4 * m > level * (bh[:, None] * bw[None, :])


def frame_stats(tc, tp, params):
    sad, _, changed = block_stats(tc, tp, params)
    return [int(changed.sum()), int(changed.size), int(sad.sum()), int(tc.astype(np.int64).sum()), int(tp.astype(np.int64).sum()), 0, 0, 0]


def frame_stats_loops(tc, tp, params):
    level, _, _, _, comp = params
    th, tw = tc.shape
    st = [0] * 8
    for by in range((th + 7) // 8):
        for bx in range((tw + 7) // 8):
            sad = sc = sp = ncell = 0
            for y in range(8 * by, min(8 * by + 8, th)):
                for x in range(8 * bx, min(8 * bx + 8, tw)):
                    c, p = int(tc[y][x]), int(tp[y][x])
                    sad += abs(c - p)
                    sc += c
                    sp += p
                    ncell += 1
            dsum = abs(sc - sp)
            assert dsum <= sad
            m = sad - dsum if comp else sad
            st[0] += int(4 * m > level * ncell)
            st[1] += 1
            st[2] += sad
            st[3] += sc
            st[4] += sp
    return st


def is_cut(params, stats):
    return params[1] > 0 and 256 * stats[0] > params[1] * stats[1]


def policy_states(frames, w, h, params, forced=frozenset(), first=True):
    """the policy turned on in front of frames[0]. first: frames[0] is the stream's first frame (an IDR anyway). Per
    frame the sixteen words: the eight statistics words, cut, key, reason, dist, keys by cut, by period, other, frames"""
    _, share, min_gap, max_gap, _ = params
    prev = None
    dist = by_cut = by_period = by_other = 0
    out = []
    for t, f in enumerate(frames):
        stats = [0] * 8
        has = False
        if share > 0:
            tc = thumbnail(f, w, h)
            if prev is not None:
                stats = frame_stats(tc, prev, params)
                has = True
            prev = tc
        other = (first and t == 0) or t in forced
        period = max_gap > 0 and dist + 1 >= max_gap
        cut = share > 0 and has and is_cut(params, stats) and dist + 1 >= min_gap
        key = other or period or cut
        reason = 3 if other else 2 if period else 1 if cut else 0
        dist = 0 if key else dist + 1
        by_cut += reason == 1
        by_period += reason == 2
        by_other += reason == 3
        out.append(stats + [int(cut), int(key), reason, dist, by_cut, by_period, by_other, t + 1])
    return out


def policy_sequence(frames, w, h, params, forced=frozenset(), first=True):
    return [(bool(s[9]), s[10], s[11]) for s in policy_states(frames, w, h, params, forced, first)]
