"""The temporal denoiser of include/h264mi.h restated in numpy: the reference of the GPU tests. Exact
integers, so every comparison with the device is equality of bytes.

A frame is a flat uint8 array of a tight w x h I420 picture; params is (strength_y, strength_c, reach, motion).
  denoise_frame(cur, prev, w, h, params)        -> (out, stats), vectorised
  denoise_frame_loops(cur, prev, w, h, params)  -> the same, as plain loops straight from the definition
  denoise_sequence(frames, w, h, params)        -> the recursion: frame 0 as it is, frame t against output t - 1
stats is [moving blocks, blocks, sum of m over luma, sum of m over both chroma planes]."""
import numpy as np


def frame_bytes(w, h):
    return w * h + 2 * (w // 2) * (h // 2)


def params_ok(params):
    ky, kc, t, mo = params
    return 0 <= ky <= 224 and 0 <= kc <= 224 and 1 <= t <= 32 and 0 <= mo <= 1020


def planes(frame, w, h):
    """views of Y (h x w), Cb, Cr (h/2 x w/2)"""
    y, c = w * h, (w // 2) * (h // 2)
    return frame[:y].reshape(h, w), frame[y:y + c].reshape(h // 2, w // 2), frame[y + c:y + 2 * c].reshape(h // 2, w // 2)


def sample_m(K, T, a):
    """m of the sample rule for one difference a >= 0"""
    if a >= T:
        return 0
    k = (K * (T - a)) // T
    return (a * k + 128) >> 8


def _filter_plane(c, p, K, T, moving):
    """c, p: int32 planes; moving: bool per sample. (out uint8, sum of m)"""
    d = c - p
    a = np.abs(d)
    k = (K * np.maximum(T - a, 0)) // T
    m = np.where((a < T) & ~moving, (a * k + 128) >> 8, 0)
    return (c - np.sign(d) * m).astype(np.uint8), int(m.sum())


def denoise_frame(cur, prev, w, h, params):
    assert params_ok(params) and w % 2 == 0 and h % 2 == 0 and cur.size == prev.size == frame_bytes(w, h)
    ky, kc, T, motion = params
    C = [pl.astype(np.int32) for pl in planes(cur, w, h)]
    P = [pl.astype(np.int32) for pl in planes(prev, w, h)]
    nbx, nby = (w + 7) // 8, (h + 7) // 8
    ad = np.zeros((nby * 8, nbx * 8), np.int64)
    ad[:h, :w] = np.abs(C[0] - P[0])
    sad = ad.reshape(nby, 8, nbx, 8).sum(axis=(1, 3))
    bw = np.minimum(8, w - 8 * np.arange(nbx))
    bh = np.minimum(8, h - 8 * np.arange(nby))
    moving = 4 * sad > motion * (bh[:, None] * bw[None, :])
    mov_y = np.repeat(np.repeat(moving, 8, axis=0), 8, axis=1)[:h, :w]
    mov_c = np.repeat(np.repeat(moving, 4, axis=0), 4, axis=1)[:h // 2, :w // 2]
    oy, sy = _filter_plane(C[0], P[0], ky, T, mov_y)
    ou, su = _filter_plane(C[1], P[1], kc, T, mov_c)
    ov, sv = _filter_plane(C[2], P[2], kc, T, mov_c)
    out = np.concatenate([oy.ravel(), ou.ravel(), ov.ravel()])
    return out, [int(moving.sum()), nbx * nby, sy, su + sv]


def denoise_frame_loops(cur, prev, w, h, params):
    assert params_ok(params) and w % 2 == 0 and h % 2 == 0 and cur.size == prev.size == frame_bytes(w, h)
    ky, kc, T, motion = params
    out = np.empty_like(cur)
    C, P, O = planes(cur, w, h), planes(prev, w, h), planes(out, w, h)
    stats = [0, 0, 0, 0]
    for by in range((h + 7) // 8):
        for bx in range((w + 7) // 8):
            bw, bh = min(8, w - 8 * bx), min(8, h - 8 * by)
            sad = 0
            for y in range(8 * by, 8 * by + bh):
                for x in range(8 * bx, 8 * bx + bw):
                    sad += abs(int(C[0][y][x]) - int(P[0][y][x]))
            moving = 4 * sad > motion * bw * bh
            stats[0] += int(moving)
            stats[1] += 1
            for pl in range(3):
                K = ky if pl == 0 else kc
                x0, y0, rw, rh = (8 * bx, 8 * by, bw, bh) if pl == 0 else (4 * bx, 4 * by, bw // 2, bh // 2)
                for y in range(y0, y0 + rh):
                    for x in range(x0, x0 + rw):
                        c = int(C[pl][y][x])
                        d = c - int(P[pl][y][x])
                        m = 0 if moving else sample_m(K, T, abs(d))
                        stats[2 if pl == 0 else 3] += m
                        O[pl][y][x] = c - m if d > 0 else c + m
    return out, stats


def denoise_sequence(frames, w, h, params):
    """frames: a sequence of frames of one stream. The filtered frames (frame 0 unchanged) and the stats of frames 1.."""
    outs, stats = [np.array(frames[0], dtype=np.uint8, copy=True)], []
    for f in frames[1:]:
        o, st = denoise_frame(np.asarray(f), outs[-1], w, h, params)
        outs.append(o)
        stats.append(st)
    return outs, stats
