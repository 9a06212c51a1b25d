"""The reference for h264mi_i420_orient_dev (include/h264mi.h): a numpy restatement of the definition, written from the
header's table and not from the kernel. Every plane is turned by itself; samples are moved, never interpolated.

A plane is a 2-D uint8 array; a frame is tight I420 bytes (w * h luma, then two (w/2) x (h/2) chroma planes). The
algebra (compose, inverse) is not typed in: it is read off what the orientations do to a 2 x 3 plane of six different
values, which tells all eight apart."""
import numpy as np

IDENTITY, ROT90, ROT180, ROT270, MIRROR, FLIP, TRANSPOSE, TRANSVERSE = range(8)
ALL = tuple(range(8))
TRANSPOSING = (ROT90, ROT270, TRANSPOSE, TRANSVERSE)

# the right-hand column of the header's table
_TURN = {
    IDENTITY: lambda p: p,
    ROT90: lambda p: np.rot90(p, -1),
    ROT180: lambda p: np.rot90(p, 2),
    ROT270: lambda p: np.rot90(p, 1),
    MIRROR: lambda p: p[:, ::-1],
    FLIP: lambda p: p[::-1],
    TRANSPOSE: lambda p: p.T,
    TRANSVERSE: lambda p: np.rot90(p, 2).T,
}


def orient_plane(plane, orient):
    """a (ph, pw) plane turned by orient: (ph, pw), or (pw, ph) for a transposing orientation; a contiguous copy"""
    return np.ascontiguousarray(_TURN[orient](np.asarray(plane)))


def frame_bytes(w, h):
    return w * h + 2 * (w // 2) * (h // 2)


def planes(frame, w, h):
    """the Y, Cb, Cr planes of a tight I420 frame"""
    f = np.asarray(frame, np.uint8).ravel()
    cw, ch = w // 2, h // 2
    y = f[:w * h].reshape(h, w)
    u = f[w * h:w * h + cw * ch].reshape(ch, cw)
    v = f[w * h + cw * ch:w * h + 2 * cw * ch].reshape(ch, cw)
    return y, u, v


def size(orient, w, h):
    """(width, height) of a w x h frame turned by orient"""
    assert orient in ALL and w % 2 == 0 and h % 2 == 0 and w >= 2 and h >= 2
    return (h, w) if orient in TRANSPOSING else (w, h)


def orient_frame(frame, w, h, orient):
    """a tight w x h I420 frame turned by orient: the tight I420 bytes of the size(orient, w, h) frame as a uint8 array"""
    assert w % 2 == 0 and h % 2 == 0 and w >= 2 and h >= 2
    return np.concatenate([orient_plane(p, orient).ravel() for p in planes(frame, w, h)])


_INDEX = np.arange(6, dtype=np.uint8).reshape(2, 3)


def _which(plane):
    """the one orientation that takes the index plane to `plane`"""
    hits = [k for k in ALL if orient_plane(_INDEX, k).shape == plane.shape and np.array_equal(orient_plane(_INDEX, k), plane)]
    assert len(hits) == 1
    return hits[0]


# COMPOSE[a][b]: a, then b.  INVERSE[a]: what undoes a
COMPOSE = tuple(tuple(_which(orient_plane(orient_plane(_INDEX, a), b)) for b in ALL) for a in ALL)
INVERSE = tuple(next(b for b in ALL if COMPOSE[a][b] == IDENTITY) for a in ALL)


def compose(first, then):
    return COMPOSE[first][then]


def inverse(orient):
    return INVERSE[orient]
