"""The colour specifications of include/h264mi.h (h264mi_colorspec) restated in numpy: the reference of
tests/test_gpu_cs.py and tests/test_cs_host.py. Exact integers in int32, written from the header's text: the table,
Y = clamp(((FY.p + 128) >> 8) + yo), chroma of the top-left pixel or of the sum of four, chroma repeated or
interpolated 9-3-3-1 with clamped neighbours, and sat(v) = min(max(v, 0), 65535) >> 8 on the way back."""
import collections

import numpy as np

BT601, BT709 = 0, 1
LIMITED, FULL = 0, 1
TOPLEFT, AVERAGE = 0, 1
REPEAT, BILINEAR = 0, 1

Spec = collections.namedtuple('Spec', 'matrix range chroma_down chroma_up', defaults=(0, 0, 0, 0))
DEFAULT = Spec()

# (matrix, range): FY, FU, FV, yo, IY, RV, GU, GV, BU
TABLE = {
    (BT601, LIMITED): ((66, 129, 25), (-38, -74, 112), (112, -94, -18), 16, 298, 409, 100, 208, 516),
    (BT601, FULL): ((77, 150, 29), (-43, -85, 128), (128, -107, -21), 0, 256, 359, 88, 183, 454),
    (BT709, LIMITED): ((47, 157, 16), (-26, -86, 112), (112, -102, -10), 16, 298, 459, 55, 136, 541),
    (BT709, FULL): ((54, 183, 19), (-29, -99, 128), (128, -116, -12), 0, 256, 403, 48, 120, 475),
}
TABLES = sorted(TABLE)
NAMES = {(BT601, LIMITED): '601-limited', (BT601, FULL): '601-full', (BT709, LIMITED): '709-limited', (BT709, FULL): '709-full'}


def spec_ok(spec):
    return spec is not None and all(v in (0, 1) for v in spec)


def frame_bytes(w, h):
    return w * h + 2 * (w // 2) * (h // 2)


def i420a_bytes(w, h):
    return 2 * w * h + 2 * (w // 2) * (h // 2)


def _dot(F, p):
    """F.p over the last axis of p (..., >= 3): int32"""
    return F[0] * p[..., 0] + F[1] * p[..., 1] + F[2] * p[..., 2]


def rgba_to_planes(rgba, w, h, spec):
    """one tight RGBA frame (w * h * 4 bytes) -> (Y h x w, Cb, Cr h/2 x w/2, A h x w), uint8"""
    FY, FU, FV, yo = TABLE[spec.matrix, spec.range][:4]
    p = np.asarray(rgba, np.uint8).reshape(h, w, 4).astype(np.int32)
    Y = np.clip(((_dot(FY, p) + 128) >> 8) + yo, 0, 255)
    if spec.chroma_down == AVERAGE:
        S = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
        Cb = np.clip(((_dot(FU, S) + 512) >> 10) + 128, 0, 255)
        Cr = np.clip(((_dot(FV, S) + 512) >> 10) + 128, 0, 255)
    else:
        p00 = p[0::2, 0::2]
        Cb = np.clip(((_dot(FU, p00) + 128) >> 8) + 128, 0, 255)
        Cr = np.clip(((_dot(FV, p00) + 128) >> 8) + 128, 0, 255)
    return Y.astype(np.uint8), Cb.astype(np.uint8), Cr.astype(np.uint8), p[..., 3].astype(np.uint8)


def rgba_to_i420(rgba, w, h, spec=DEFAULT):
    """one tight RGBA frame -> one tight I420 frame"""
    Y, Cb, Cr, _ = rgba_to_planes(rgba, w, h, spec)
    return np.concatenate([Y.ravel(), Cb.ravel(), Cr.ravel()])


def rgba_to_i420a(rgba, w, h, spec=DEFAULT):
    """one tight RGBA frame -> one I420A sprite: Y, Cb, Cr, then A = the fourth bytes"""
    Y, Cb, Cr, A = rgba_to_planes(rgba, w, h, spec)
    return np.concatenate([Y.ravel(), Cb.ravel(), Cr.ravel(), A.ravel()])


def upsample(C, mode):
    """a chroma plane ch x cw (uint8) -> the chroma of every luma position, 2ch x 2cw int32"""
    C = np.asarray(C).astype(np.int32)
    ch, cw = C.shape
    y, x = np.arange(2 * ch), np.arange(2 * cw)
    cy, cx = y >> 1, x >> 1
    if mode == REPEAT:
        return C[cy][:, cx]
    ny = np.clip(cy + np.where(y & 1, 1, -1), 0, ch - 1)
    nx = np.clip(cx + np.where(x & 1, 1, -1), 0, cw - 1)
    return (9 * C[cy][:, cx] + 3 * C[cy][:, nx] + 3 * C[ny][:, cx] + C[ny][:, nx] + 8) >> 4


def i420_to_rgba(i420, w, h, spec=DEFAULT):
    """one tight I420 frame -> one tight RGBA frame (w * h * 4 bytes), A = 255"""
    _, _, _, yo, IY, RV, GU, GV, BU = TABLE[spec.matrix, spec.range]
    b = np.asarray(i420, np.uint8)
    cw, ch = w // 2, h // 2
    Y = b[:w * h].reshape(h, w).astype(np.int32)
    cb = upsample(b[w * h:w * h + cw * ch].reshape(ch, cw), spec.chroma_up) - 128
    cr = upsample(b[w * h + cw * ch:w * h + 2 * cw * ch].reshape(ch, cw), spec.chroma_up) - 128
    c = IY * (Y - yo)

    def sat(v):
        return np.minimum(np.maximum(v, 0), 65535) >> 8
    out = np.empty((h, w, 4), np.uint8)
    out[..., 0] = sat(c + RV * cr + 128)
    out[..., 1] = sat(c - GU * cb - GV * cr + 128)
    out[..., 2] = sat(c + BU * cb + 128)
    out[..., 3] = 255
    return out.ravel()


def frames(fn, src, w, h, n, spec):
    """fn over n frames back to back"""
    src = np.asarray(src, np.uint8).reshape(n, -1)
    return np.concatenate([fn(src[f], w, h, spec) for f in range(n)])
