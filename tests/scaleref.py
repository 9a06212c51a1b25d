"""The reference for h264mi_i420_scale_dev (include/h264mi.h): a numpy restatement of the definition, written from the
definition and not from the kernel. Area-average downscaling, every plane on its own: the weight matrices of both
axes, Wy @ plane @ Wx.T in int64, then the rounding division.

A plane is a 2-D uint8 array; a frame is tight I420 bytes (w * h luma, then two (w/2) x (h/2) chroma planes)."""
import functools

import numpy as np


@functools.lru_cache(maxsize=None)
def weights(p, q):
    """W[o, i] = max(0, min((i + 1) q, (o + 1) p) - max(i q, o p)): the weight of source sample i (of p) in output
    sample o (of q <= p), int64, shape (q, p). Rows sum to p, columns to q."""
    assert 1 <= q <= p
    i = np.arange(p, dtype=np.int64)[None, :]
    o = np.arange(q, dtype=np.int64)[:, None]
    w = np.maximum(0, np.minimum((i + 1) * q, (o + 1) * p) - np.maximum(i * q, o * p))
    w.setflags(write=False)
    return w


def scale_plane(plane, qw, qh):
    """a (ph, pw) uint8 plane scaled to (qh, qw): (Wy @ plane @ Wx.T + (pw ph >> 1)) // (pw ph)"""
    ph, pw = plane.shape
    assert pw <= 4096 and ph <= 4096
    num = weights(ph, qh) @ plane.astype(np.int64) @ weights(pw, qw).T
    assert int(num.max()) + ((pw * ph) >> 1) < 1 << 32
    out = (num + ((pw * ph) >> 1)) // (pw * ph)
    assert 0 <= int(out.min()) and int(out.max()) <= 255
    return out.astype(np.uint8)


def planes(frame, w, h):
    """the Y, Cb, Cr planes of a tight I420 frame"""
    f = np.asarray(frame, np.uint8).ravel()
    cw, ch = w // 2, h // 2
    y = f[:w * h].reshape(h, w)
    u = f[w * h:w * h + cw * ch].reshape(ch, cw)
    v = f[w * h + cw * ch:w * h + 2 * cw * ch].reshape(ch, cw)
    return y, u, v


def frame_bytes(w, h):
    return w * h + 2 * (w // 2) * (h // 2)


def scale_frame(frame, sw, sh, dw, dh):
    """a tight sw x sh I420 frame scaled to dw x dh: the tight I420 bytes as a uint8 array"""
    assert sw % 2 == 0 and sh % 2 == 0 and dw % 2 == 0 and dh % 2 == 0 and 2 <= dw <= sw and 2 <= dh <= sh
    y, u, v = planes(frame, sw, sh)
    return np.concatenate([scale_plane(y, dw, dh).ravel(), scale_plane(u, dw // 2, dh // 2).ravel(),
                           scale_plane(v, dw // 2, dh // 2).ravel()])
