"""The reference for h264mi_quality (include/h264mi.h): a numpy restatement of the definition, written from the
definition and not from the kernel. Integer sums in int64 by sliding windows, num and den in int64, one float64
division, np.rint(x * 2**32) to int64.

A plane is a 2-D uint8 array; a frame is tight I420 bytes (w * h luma, then two (w/2) x (h/2) chroma planes)."""
import numpy as np

C1, C2 = 416, 235963
ONE = 1 << 32


def window_sums(x):
    """sum of x over every 8x8 window at stride 4 (x: 2-D int64): shape (windows down, windows across)"""
    v = np.lib.stride_tricks.sliding_window_view(x, (8, 8))[::4, ::4]
    return v.sum(axis=(2, 3), dtype=np.int64)


def window_counts(pw, ph):
    """windows across, down of a pw x ph plane: x = 0, 4, .. <= pw - 8"""
    return (pw - 8) // 4 + 1, (ph - 8) // 4 + 1


def plane_windows(a, b):
    """per-window llrint(ssim_window * 2^32) of two planes, as an int64 array (windows down, windows across)"""
    a = a.astype(np.int64)
    b = b.astype(np.int64)
    s1, s2 = window_sums(a), window_sums(b)
    ss = window_sums(a * a) + window_sums(b * b)
    s12 = window_sums(a * b)
    vars_ = 64 * ss - s1 * s1 - s2 * s2
    covar = 64 * s12 - s1 * s2
    num = (2 * s1 * s2 + C1) * (2 * covar + C2)
    den = (s1 * s1 + s2 * s2 + C1) * (vars_ + C2)
    ssim = num.astype(np.float64) / den.astype(np.float64)
    return np.rint(ssim * float(ONE)).astype(np.int64)


def plane_quality(a, b):
    """(sse, ssim_fix, windows) of two planes, Python ints"""
    d = a.astype(np.int64) - b.astype(np.int64)
    fix = plane_windows(a, b)
    return int((d * d).sum()), int(fix.sum()), int(fix.size)


def planes(frame, w, h):
    """the Y, Cb, Cr planes of a tight I420 frame"""
    f = np.asarray(frame, np.uint8).ravel()
    cw, ch = w // 2, h // 2
    y = f[:w * h].reshape(h, w)
    u = f[w * h:w * h + cw * ch].reshape(ch, cw)
    v = f[w * h + cw * ch:w * h + 2 * cw * ch].reshape(ch, cw)
    return y, u, v


def frame_quality(a, b, w, h):
    """the record of a pair of tight I420 frames: {'sse': [3], 'ssim_fix': [3], 'windows': [2], 'coded': 1}"""
    q = [plane_quality(pa, pb) for pa, pb in zip(planes(a, w, h), planes(b, w, h))]
    assert q[1][2] == q[2][2]
    return {'sse': [p[0] for p in q], 'ssim_fix': [p[1] for p in q], 'windows': [q[0][2], q[1][2]], 'coded': 1}


ZERO = {'sse': [0, 0, 0], 'ssim_fix': [0, 0, 0], 'windows': [0, 0], 'coded': 0}
