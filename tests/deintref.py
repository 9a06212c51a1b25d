"""The deinterlacer of include/h264mi.h restated in numpy from the header's text: the reference of the
CPU and GPU tests. Exact integers, so every comparison with the library is equality of bytes.

A frame is a flat uint8 array of a tight w x h I420 picture; params is (parity, spatial, temporal, comb_level).
  deint_frame(cur, prev, w, h, params)     -> (out, stats); prev may be None (then the result is spatial only)
  deint_sequence(frames, w, h, params)     -> the outputs of one stream: frame 0 without a previous frame, frame t
                                              against the unfiltered frame t - 1
  interlace(frames_2x, w, h, parity)       -> a double-rate progressive clip woven into half as many interlaced frames
stats is [missing luma samples, combed luma samples, sum |O - v| over luma, over both chroma planes], modulo 2^32."""
import numpy as np


def frame_bytes(w, h):
    return w * h + 2 * (w // 2) * (h // 2)


def params_ok(params):
    parity, spatial, temporal, comb = params
    return parity in (0, 1) and spatial in (0, 1) and temporal in (0, 1) and 0 <= comb <= 255


def planes(frame, w, h):
    """views of Y (h x w), Cb, Cr (h/2 x w/2)"""
    y, c = w * h, (w // 2) * (h // 2)
    return frame[:y].reshape(h, w), frame[y:y + c].reshape(h // 2, w // 2), frame[y + c:y + 2 * c].reshape(h // 2, w // 2)


def _plane(C, P, params):
    """one plane: C, P (or None) int32 arrays ph x pw. (O uint8, missing samples, combed samples, sum |O - v|)"""
    parity, spatial, temporal, comb = params
    ph, pw = C.shape
    O = C.copy()
    missing = combed = total = 0
    if ph == 1 and parity == 1:  # no kept line
        return O.astype(np.uint8), 0, 0, 0
    x = np.arange(pw)
    cx = lambda i: np.clip(i, 0, pw - 1)
    for y in range(ph):
        if y % 2 == parity:
            continue
        has_up, has_dn = y - 1 >= 0, y + 1 < ph
        v = C[y]
        if has_up and has_dn:
            up, dn = C[y - 1], C[y + 1]
            if spatial == 0:
                s = (up + dn + 1) >> 1
            else:
                best = None
                for d in (0, -1, 1):
                    score = sum(np.abs(up[cx(x + j + d)] - dn[cx(x + j - d)]) for j in (-1, 0, 1))
                    cand = (up[cx(x + d)] + dn[cx(x - d)] + 1) >> 1
                    if best is None:
                        best, s = score, cand
                    else:
                        take = score < best  # a tie stays with the earlier d
                        s = np.where(take, cand, s)
                        best = np.where(take, score, best)
            du, dd = v - up, v - dn
            same = ((du > 0) & (dd > 0)) | ((du < 0) & (dd < 0))
            combed += int((same & (np.minimum(np.abs(du), np.abs(dd)) > comb)).sum())
        else:
            s = C[y - 1] if has_up else C[y + 1]
        if temporal == 1 and P is not None:
            k = y ^ 1
            if k >= ph:
                k = y
            m = np.maximum(np.abs(C[y] - P[y]), np.abs(C[k] - P[k]))
            s = np.minimum(np.maximum(s, v - m), v + m)
        missing += pw
        total += int(np.abs(s - v).sum())
        O[y] = s
    assert O.min() >= 0 and O.max() <= 255
    return O.astype(np.uint8), missing, combed, total


def deint_frame(cur, prev, w, h, params):
    assert params_ok(params) and w % 2 == 0 and h % 2 == 0 and cur.size == frame_bytes(w, h)
    assert prev is None or prev.size == cur.size
    C = [pl.astype(np.int32) for pl in planes(np.asarray(cur), w, h)]
    P = [pl.astype(np.int32) for pl in planes(np.asarray(prev), w, h)] if prev is not None else [None] * 3
    res = [_plane(C[i], P[i], params) for i in range(3)]
    out = np.concatenate([r[0].ravel() for r in res])
    M = 1 << 32
    return out, [res[0][1] % M, res[0][2] % M, res[0][3] % M, (res[1][3] + res[2][3]) % M]


def deint_sequence(frames, w, h, params):
    """frames: a sequence of frames of one stream. (outputs, stats): frame 0 without a previous frame"""
    outs, stats = [], []
    for t, f in enumerate(frames):
        o, st = deint_frame(np.asarray(f), np.asarray(frames[t - 1]) if t else None, w, h, params)
        outs.append(o)
        stats.append(st)
    return outs, stats


def interlace(frames_2x, w, h, parity):
    """frames_2x: 2 T progressive frames at twice the frame rate. Interlaced frame t: in every plane the lines
    y % 2 == parity from frame 2 t (the kept field's instant), the other lines from frame 2 t + 1"""
    out = []
    for t in range(len(frames_2x) // 2):
        a, b = np.asarray(frames_2x[2 * t]), np.asarray(frames_2x[2 * t + 1])
        f = np.array(b, dtype=np.uint8, copy=True)
        for fa, ff in zip(planes(a, w, h), planes(f, w, h)):
            ff[parity::2] = fa[parity::2]
        out.append(f)
    return out
