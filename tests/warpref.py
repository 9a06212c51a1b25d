"""The reference for h264mi_i420_warp_dev and the h264mi_warp_mesh_* builders (include/h264mi.h): a numpy restatement
of the header's rule, written from the header and not from the kernel. Vectorised over a plane, 64-bit integers
throughout (numpy's >> and // floor, as the rule's shifts and divisions do).

A frame is tight I420 bytes; a mesh is a (mh, mw, 2) int32 array of (x, y) source luma positions in sixteenths. The
module also holds what the host test and the GPU test share: the shapes, the mesh set and the settings."""
import functools

import numpy as np

BILINEAR, BICUBIC = 0, 1
CLAMP, FILL = 0, 1
POINT_MAX = 1 << 18
RADIAL_MAX_CENTRE, RADIAL_MAX_K, RADIAL_MAX_R2, RADIAL_MAX_Q = 1 << 18, 1 << 20, 1 << 40, 1 << 24


def frame_bytes(w, h):
    return w * h + 2 * (w // 2) * (h // 2)


def mesh_size(dw, dh, g):
    G = 1 << g
    return ((dw + G - 1) >> g) + 1, ((dh + G - 1) >> g) + 1


def planes(frame, w, h):
    f = np.asarray(frame, np.uint8).ravel()
    cw, ch = w // 2, h // 2
    return f[:w * h].reshape(h, w), f[w * h:w * h + cw * ch].reshape(ch, cw), f[w * h + cw * ch:w * h + 2 * cw * ch].reshape(ch, cw)


def weights(f, cubic):
    """the four weights of the phases f (an int64 array), sum 8192: the header's table of h264mi_i420_upscale_dev"""
    if cubic:
        f2, f3 = f * f, f * f * f
        return [-f3 + 32 * f2 - 256 * f, 3 * f3 - 80 * f2 + 8192, -3 * f3 + 64 * f2 + 256 * f, f3 - 16 * f2]
    z = np.zeros_like(f)
    return [z, (16 - f) * 512, f * 512, z]


def positions(mesh, qw, qh, g, chroma):
    """(Lx, Ly): the source positions, in sixteenths of the plane's own samples, of the qw x qh samples of a plane"""
    m = np.clip(np.asarray(mesh, np.int64), -POINT_MAX, POINT_MAX)
    G, G2 = 1 << g, 2 << g
    u = (4 * np.arange(qw, dtype=np.int64) + 1 if chroma else 2 * np.arange(qw, dtype=np.int64))[None, :]
    v = (4 * np.arange(qh, dtype=np.int64) + 1 if chroma else 2 * np.arange(qh, dtype=np.int64))[:, None]
    cx, cy, fx, fy = u >> (g + 1), v >> (g + 1), u & (G2 - 1), v & (G2 - 1)
    out = []
    for k in (0, 1):
        A, B, C, D = m[cy, cx, k], m[cy, cx + 1, k], m[cy + 1, cx, k], m[cy + 1, cx + 1, k]
        P = (G2 - fx) * (G2 - fy) * A + fx * (G2 - fy) * B + (G2 - fx) * fy * C + fx * fy * D
        assert np.abs(P).max() <= 1 << 30
        out.append((P - 28 * G * G) // (8 * G * G) if chroma else (P + 2 * G * G) // (4 * G * G))
    return out[0], out[1]


def warp_plane(src, qw, qh, mesh, g, cubic, chroma, fill):
    """a (ph, pw) source plane sampled into a (qh, qw) plane; fill: None (CLAMP) or the plane's fill value"""
    S = np.asarray(src, np.int64)
    ph, pw = S.shape
    Lx, Ly = positions(mesh, qw, qh, g, chroma)
    ix, iy = Lx >> 4, Ly >> 4
    wx, wy = weights(Lx & 15, cubic), weights(Ly & 15, cubic)
    acc = np.zeros((qh, qw), np.int64)
    for t in range(4):
        row = np.clip(iy - 1 + t, 0, ph - 1)
        h = sum(wx[k] * S[row, np.clip(ix - 1 + k, 0, pw - 1)] for k in range(4))
        acc += wy[t] * ((h + 16) >> 5)
    assert np.abs(acc).max() < 1 << 31
    out = np.clip((acc + (1 << 20)) >> 21, 0, 255)
    if fill is not None:
        out = np.where((Lx < 0) | (Lx > 16 * (pw - 1)) | (Ly < 0) | (Ly > 16 * (ph - 1)), fill, out)
    return out.astype(np.uint8)


def warp_frame(frame, sw, sh, dw, dh, mesh, params):
    """params: (filter, edge, fill_y, fill_u, fill_v, grid_log2). The tight dw x dh I420 bytes"""
    filt, edge, fy, fu, fv, g = params
    assert np.asarray(mesh).shape == mesh_size(dw, dh, g)[::-1] + (2,)
    out = []
    for k, p in enumerate(planes(frame, sw, sh)):
        c = k != 0
        out.append(warp_plane(p, dw >> c, dh >> c, mesh, g, filt == BICUBIC, c, (fy, fu, fv)[k] if edge == FILL else None).ravel())
    return np.concatenate(out)


# ---------------------------------------------------------------- the builders


def _grid(dw, dh, g):
    mw, mh = mesh_size(dw, dh, g)
    return (np.arange(mw, dtype=object) << g)[None, :], (np.arange(mh, dtype=object) << g)[:, None]  # Python integers: no overflow


def _mesh(x, y, dw, dh, g):
    mw, mh = mesh_size(dw, dh, g)
    m = np.empty((mh, mw, 2), np.int32)
    m[..., 0] = np.clip(np.broadcast_to(x, (mh, mw)).astype(object), -POINT_MAX, POINT_MAX).astype(np.int64)
    m[..., 1] = np.clip(np.broadcast_to(y, (mh, mw)).astype(object), -POINT_MAX, POINT_MAX).astype(np.int64)
    return m


def mesh_affine(dw, dh, g, m):
    X, Y = _grid(dw, dh, g)
    m = [int(v) for v in m]
    return _mesh((m[0] * X + m[1] * Y + m[2] + (1 << 11)) >> 12, (m[3] * X + m[4] * Y + m[5] + (1 << 11)) >> 12, dw, dh, g)


def mesh_homography(dw, dh, g, h):
    """None where the library returns -1"""
    X, Y = _grid(dw, dh, g)
    h = [int(v) for v in h]
    den = h[6] * X + h[7] * Y + h[8]
    if (den <= 0).any():
        return None
    return _mesh((32 * (h[0] * X + h[1] * Y + h[2]) + den) // (2 * den), (32 * (h[3] * X + h[4] * Y + h[5]) + den) // (2 * den), dw, dh, g)


def mesh_radial(dw, dh, g, cx, cy, r2, k1, k2):
    """None where the library returns -1"""
    if abs(cx) > RADIAL_MAX_CENTRE or abs(cy) > RADIAL_MAX_CENTRE or not 1 <= r2 <= RADIAL_MAX_R2 or abs(k1) > RADIAL_MAX_K or abs(k2) > RADIAL_MAX_K:
        return None
    X, Y = _grid(dw, dh, g)
    dx, dy = 16 * X - int(cx), 16 * Y - int(cy)
    q = ((dx * dx + dy * dy) << 16) // int(r2)
    if (q > RADIAL_MAX_Q).any():
        return None
    s = 65536 + ((int(k1) * q) >> 16) + ((int(k2) * ((q * q) >> 16)) >> 16)
    return _mesh(int(cx) + ((dx * s + (1 << 15)) >> 16), int(cy) + ((dy * s + (1 << 15)) >> 16), dw, dh, g)


# the index maps of the eight orientations (include/h264mi.h's table) as affine maps, source position from destination
# position: (x, y) = (a ox + b oy + c, d ox + e oy + f), c and f in terms of the source's last column sw - 1 and row sh - 1
def orient_affine(orient, sw, sh):
    W, H = sw - 1, sh - 1
    return {0: (1, 0, 0, 0, 1, 0), 1: (0, 1, 0, -1, 0, H), 2: (-1, 0, W, 0, -1, H), 3: (0, -1, W, 1, 0, 0), 4: (-1, 0, W, 0, 1, 0),
            5: (1, 0, 0, 0, -1, H), 6: (0, 1, 0, 1, 0, 0), 7: (0, -1, W, -1, 0, H)}[orient]


def mesh_orient(orient, sw, sh, g):
    """the mesh, for the destination h264mi_orient_size gives, whose points are the orientation's index map"""
    dw, dh = (sh, sw) if orient in (1, 3, 6, 7) else (sw, sh)
    return mesh_affine(dw, dh, g, [65536 * v for v in orient_affine(orient, sw, sh)]), dw, dh


# ---------------------------------------------------------------- what the two test files share

# source -> destination, and whether both sit at odd addresses on the device
SHAPES = [((2, 2), (2, 2), 0), ((16, 16), (16, 16), 0), ((18, 34), (34, 18), 0), ((130, 66), (130, 66), 0), ((130, 66), (130, 66), 1),
          ((2, 2), (130, 66), 0), ((130, 66), (2, 2), 0), ((8192, 2), (2, 8192), 0), ((2, 8192), (8192, 2), 0)]
GRIDS = (3, 4, 5)
N = 3  # frames of a call


def shape_id(c):
    return f'{c[0][0]}x{c[0][1]}-to-{c[1][0]}x{c[1][1]}' + ('-odd-address' if c[2] else '')


def _q16(v):
    return int(round(v * 65536))


def _m_identity(sw, sh, dw, dh, g):
    return mesh_affine(dw, dh, g, [65536, 0, 0, 0, 65536, 0])


def _m_shift(sw, sh, dw, dh, g):  # 37/16 right, 23/16 up: odd sixteenths
    m = _m_identity(sw, sh, dw, dh, g)
    return m + np.array([37, -23], np.int32)


def _m_rotate(sw, sh, dw, dh, g):  # 7 degrees about the centres: the destination's centre reads the source's
    c, s = _q16(np.cos(np.radians(7))), _q16(np.sin(np.radians(7)))
    return mesh_affine(dw, dh, g, [c, -s, (65536 * (sw - 1) - c * (dw - 1) + s * (dh - 1)) // 2,
                                   s, c, (65536 * (sh - 1) - s * (dw - 1) - c * (dh - 1)) // 2])


def _m_keystone(sw, sh, dw, dh, g):  # the lower edge 1.25 times as wide as the upper one, leaning right
    return mesh_homography(dw, dh, g, [65536, 6554, 0, 0, 65536, 0, 0, max(1, 16384 // dh), 65536])


def _radial(dw, dh, g, k1, k2):  # centre and reference radius of the destination with its mesh's overhang
    G = 1 << g
    return mesh_radial(dw, dh, g, 8 * (dw - 1), 8 * (dh - 1), (8 * (dw + 2 * G)) ** 2 + (8 * (dh + 2 * G)) ** 2, k1, k2)


def _m_barrel(sw, sh, dw, dh, g):
    return _radial(dw, dh, g, _q16(0.2), _q16(0.05))


def _m_pincushion(sw, sh, dw, dh, g):
    return _radial(dw, dh, g, _q16(-0.15), _q16(-0.02))


def _m_zoom_in(sw, sh, dw, dh, g):  # 4x: small footprints
    return mesh_affine(dw, dh, g, [16384, 0, _q16(sw / 8), 0, 16384, _q16(sh / 8)])


def _m_zoom_out(sw, sh, dw, dh, g):  # 1/8: large footprints
    return mesh_affine(dw, dh, g, [8 * 65536, 0, -_q16(1.5), 0, 8 * 65536, _q16(0.25)])


def _m_random(sw, sh, dw, dh, g):
    mw, mh = mesh_size(dw, dh, g)
    rng = np.random.default_rng(1000 * g + dw + 7 * dh + 13 * sw)
    return np.stack([rng.integers(-64, 16 * sw + 64, (mh, mw)), rng.integers(-64, 16 * sh + 64, (mh, mw))], axis=-1).astype(np.int32)


def _m_coincide(sw, sh, dw, dh, g):
    mw, mh = mesh_size(dw, dh, g)
    return np.broadcast_to(np.array([16 * (sw // 2) + 5, 16 * (sh // 2) + 9], np.int32), (mh, mw, 2)).copy()


def _m_outside(sw, sh, dw, dh, g):  # left of and below the source, moving
    m = _m_identity(sw, sh, dw, dh, g)
    return np.stack([-5000 - m[..., 1], 16 * sh + 4000 + m[..., 0]], axis=-1).astype(np.int32)


def _m_extreme(sw, sh, dw, dh, g):  # 0x7fffffff and 0x80000000, which the kernel clamps
    mw, mh = mesh_size(dw, dh, g)
    k = np.add.outer(np.arange(mh), np.arange(mw))
    a, b = np.int32(0x7fffffff), np.int32(-0x80000000)
    return np.stack([np.where(k % 2 == 0, a, b), np.where(k % 3 == 0, b, a)], axis=-1).astype(np.int32)


MESHES = [('identity', _m_identity), ('shift', _m_shift), ('rotate7', _m_rotate), ('keystone', _m_keystone), ('barrel', _m_barrel),
          ('pincushion', _m_pincushion), ('zoom-in-4', _m_zoom_in), ('zoom-out-8', _m_zoom_out), ('random', _m_random),
          ('coincide', _m_coincide), ('outside', _m_outside), ('extreme', _m_extreme)]
SETTINGS = [(f, e) for f in (BILINEAR, BICUBIC) for e in (CLAMP, FILL)]
FILLS = (31, 77, 201)


@functools.lru_cache(maxsize=None)
def mesh(k, src, dst, g):
    """mesh k of the set for a case; shared, never written"""
    m = MESHES[k][1](src[0], src[1], dst[0], dst[1], g)
    assert m is not None and m.dtype == np.int32 and m.shape == mesh_size(dst[0], dst[1], g)[::-1] + (2,), MESHES[k][0]
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def frames(src, n=N):
    """n frames of different content, half noise and half a gradient so that positions show; shared, never written"""
    w, h = src
    rng = np.random.default_rng(4000 + w + 3 * h)
    f = rng.integers(0, 256, (n, frame_bytes(w, h)), dtype=np.uint8)
    ramp = ((np.add.outer(np.arange(h), 2 * np.arange(w)) * 3) & 255).astype(np.uint8).ravel()
    f[1, :w * h] = ramp
    f.setflags(write=False)
    return f


def params(filt, edge, g):
    return (filt, edge) + FILLS + (g,)


@functools.lru_cache(maxsize=None)
def reference(src, dst, g, k, filt, edge, f):
    """frame f of the case's sources under mesh k: computed once, shared, never written"""
    out = warp_frame(frames(src)[f], src[0], src[1], dst[0], dst[1], mesh(k, src, dst, g), params(filt, edge, g))
    out.setflags(write=False)
    return out
