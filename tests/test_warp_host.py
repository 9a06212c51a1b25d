"""CPU: the mesh warp's host side (include/h264mi.h) -- the names, the library's own loop restatement
h264mi_i420_warp_host and the three builders against tests/warpref.py on every case the GPU test runs, the consequences
the header states (identity, whole shifts, the eight orientations), the limits, and the audit that the shared mesh set
holds tiles of both classes of the kernel."""
import ctypes
import os
import re

import numpy as np
import pytest

import orientref
import warpref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_NAMES = ('h264mi_warp_ok', 'h264mi_warp_mesh_size', 'h264mi_warp_mesh_affine', 'h264mi_warp_mesh_homography', 'h264mi_warp_mesh_radial',
           'h264mi_warp_tile_class', 'h264mi_i420_warp_dev', 'h264mi_i420_warp_host', 'h264mi_enc_encode_warped')
PY_NAMES = ('Warp', 'WARP_CLAMP', 'WARP_FILL', 'warp_ok', 'warp_mesh_size', 'warp_mesh_affine', 'warp_mesh_homography', 'warp_mesh_radial',
            'warp_tile_class', 'i420_warp', 'i420_warp_host')


def test_names_are_declared_exported_and_bound(libpath):
    import h264mi
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'h264mi.h')).read(), flags=re.S)
    L = ctypes.CDLL(libpath)
    for n in C_NAMES:
        assert re.search(r'\b' + n + r'\s*\(', header), f'{n} is not declared in include/h264mi.h'
        assert hasattr(L, n), f'{n} is not exported'
        assert getattr(h264mi.lib(), n).argtypes is not None, f'{n} has no signature in h264mi.lib()'
    for n in ('H264MI_WARP_CLAMP', 'H264MI_WARP_FILL', 'h264mi_warp;'):
        assert n in header, n
    for n in PY_NAMES:
        assert hasattr(h264mi, n), f'h264mi.{n} is missing'
    assert hasattr(h264mi.BatchEncoder, 'encode_warped')
    assert ctypes.sizeof(h264mi.Warp) == 24 and (h264mi.WARP_CLAMP, h264mi.WARP_FILL) == (warpref.CLAMP, warpref.FILL)


def test_mesh_size(libpath):
    import h264mi
    for dw, dh in ((2, 2), (16, 16), (18, 34), (130, 66), (8192, 2), (1920, 1080)):
        for g in warpref.GRIDS:
            assert h264mi.warp_mesh_size(dw, dh, g) == warpref.mesh_size(dw, dh, g)
    assert h264mi.warp_mesh_size(8192, 8192, 3) == (1025, 1025) and h264mi.warp_mesh_size(2, 2, 5) == (2, 2)
    for dw, dh, g in ((0, 2, 3), (3, 2, 3), (8194, 2, 3), (2, 8194, 3), (2, -2, 3), (16, 16, 2), (16, 16, 6)):
        with pytest.raises(ValueError):
            h264mi.warp_mesh_size(dw, dh, g)
    mw = ctypes.c_int()
    assert h264mi.lib().h264mi_warp_mesh_size(16, 16, 3, None, ctypes.byref(mw)) == -1
    assert h264mi.lib().h264mi_warp_mesh_size(16, 16, 3, ctypes.byref(mw), None) == -1


@pytest.mark.parametrize('case', warpref.SHAPES[:4] + warpref.SHAPES[5:], ids=[warpref.shape_id(c) for c in warpref.SHAPES[:4] + warpref.SHAPES[5:]])
def test_reference_equals_the_library_host_restatement(libpath, case):
    """every mesh x pitch x filter x edge mode of the shared set, the three frames"""
    import h264mi
    src, dst, _ = case
    for g in warpref.GRIDS:
        for k, (name, _) in enumerate(warpref.MESHES):
            for filt, edge in warpref.SETTINGS:
                for f in range(warpref.N):
                    got = h264mi.i420_warp_host(warpref.frames(src)[f], src[0], src[1], dst[0], dst[1], warpref.mesh(k, src, dst, g),
                                                warpref.params(filt, edge, g))
                    want = warpref.reference(src, dst, g, k, filt, edge, f)
                    assert np.array_equal(got, want), f'{name} pitch {1 << g} filter {filt} edge {edge} frame {f}: {int((got != want).sum())} bytes'


AFFINE = ([65536, 0, 0, 0, 65536, 0], [65048, -7987, 123456, 7987, 65048, -654321], [-65536, 0, 65536 * 129, 0, -65536, 65536 * 65],
          [0x7fffffff, 0x7fffffff, 0x7fffffff, -0x80000000, -0x80000000, -0x80000000], [1, -1, 2047, -1, 1, -2049])
HOMOGRAPHY = ([65536, 0, 0, 0, 65536, 0, 0, 0, 65536], [65536, 6554, 0, 0, 65536, 0, 0, 31, 65536], [70000, -3000, 99999, 2500, 60000, -77777, 5, 3, 40000],
              [0x7fffffff, 0x7fffffff, 0x7fffffff, -0x80000000, -0x80000000, -0x80000000, 0, 0, 1],
              [-0x80000000, 0, 0, 0x7fffffff, 0, 0, 0x7fffffff, 0x7fffffff, 0x7fffffff])
SIZES = ((2, 2), (16, 16), (34, 18), (130, 66), (8192, 2), (2, 8192), (1920, 1080))


def test_builders_equal_the_reference(libpath):
    import h264mi
    for dw, dh in SIZES:
        for g in warpref.GRIDS:
            for m in AFFINE:
                assert np.array_equal(h264mi.warp_mesh_affine(dw, dh, g, m), warpref.mesh_affine(dw, dh, g, m)), (dw, dh, g, m)
            for h in HOMOGRAPHY:
                want = warpref.mesh_homography(dw, dh, g, h)
                assert want is not None
                assert np.array_equal(h264mi.warp_mesh_homography(dw, dh, g, h), want), (dw, dh, g, h)
            G = 1 << g
            r2 = (8 * (dw + 2 * G)) ** 2 + (8 * (dh + 2 * G)) ** 2
            for cx, cy, r2, k1, k2 in ((8 * (dw - 1), 8 * (dh - 1), r2, 13107, 3277), (8 * (dw - 1), 8 * (dh - 1), r2, -9830, -1311),
                                       (-(1 << 18), 1 << 18, 1 << 40, 1 << 20, -(1 << 20)), (1 << 18, -(1 << 18), 1 << 39, -(1 << 20), 1 << 20),
                                       (0, 0, 1 << 32, 1 << 20, 1 << 20)):
                want = warpref.mesh_radial(dw, dh, g, cx, cy, r2, k1, k2)
                assert want is not None, (dw, dh, g, cx, cy, r2)
                assert np.array_equal(h264mi.warp_mesh_radial(dw, dh, g, cx, cy, r2, k1, k2), want), (dw, dh, g, cx, cy, r2, k1, k2)
    for k, (name, _) in enumerate(warpref.MESHES):  # the set's own meshes stay inside the clamp, but for the last
        m = warpref.mesh(k, (130, 66), (130, 66), 4)
        assert name == 'extreme' or np.abs(m.astype(np.int64)).max() <= warpref.POINT_MAX


def test_identity_shifts_and_orientations_hold_exactly(libpath):
    import h264mi
    src = (130, 66)
    fr = warpref.frames(src)[0]
    y, u, v = warpref.planes(fr, 130, 66)
    for g in warpref.GRIDS:
        for filt in (warpref.BILINEAR, warpref.BICUBIC):
            clamp, fill = warpref.params(filt, warpref.CLAMP, g), warpref.params(filt, warpref.FILL, g)
            ident = warpref.mesh(0, src, src, g)
            for prm in (clamp, fill):
                assert np.array_equal(h264mi.i420_warp_host(fr, 130, 66, 130, 66, ident, prm), fr)
                assert np.array_equal(warpref.warp_frame(fr, 130, 66, 130, 66, ident, prm), fr)
            for sx, sy in ((2, 0), (0, -4), (-6, 10), (128, 64), (-130, 66)):  # whole even shifts: the frame moved, edges repeated or filled
                m = ident + np.array([16 * sx, 16 * sy], np.int32)
                for prm, filled in ((clamp, False), (fill, True)):
                    want = []
                    for p, c, fv in ((y, 0, warpref.FILLS[0]), (u, 1, warpref.FILLS[1]), (v, 1, warpref.FILLS[2])):
                        ph, pw = p.shape
                        yy, xx = np.arange(ph)[:, None] + (sy >> c), np.arange(pw)[None, :] + (sx >> c)
                        moved = p[np.clip(yy, 0, ph - 1), np.clip(xx, 0, pw - 1)]
                        if filled:
                            moved = np.where((yy < 0) | (yy > ph - 1) | (xx < 0) | (xx > pw - 1), fv, moved)
                        want.append(moved.astype(np.uint8).ravel())
                    want = np.concatenate(want)
                    assert np.array_equal(h264mi.i420_warp_host(fr, 130, 66, 130, 66, m, prm), want), (g, filt, sx, sy, filled)
                    assert np.array_equal(warpref.warp_frame(fr, 130, 66, 130, 66, m, prm), want), (g, filt, sx, sy, filled)
            for sw, sh in ((130, 66), (18, 34), (2, 2)):
                f2 = warpref.frames((sw, sh))[2]
                for orient in orientref.ALL:
                    m, dw, dh = warpref.mesh_orient(orient, sw, sh, g)
                    assert (dw, dh) == orientref.size(orient, sw, sh)
                    want = orientref.orient_frame(f2, sw, sh, orient)
                    for prm in (clamp, fill):
                        assert np.array_equal(h264mi.i420_warp_host(f2, sw, sh, dw, dh, m, prm), want), (g, filt, sw, sh, orient)
                        assert np.array_equal(warpref.warp_frame(f2, sw, sh, dw, dh, m, prm), want), (g, filt, sw, sh, orient)


def test_limits_are_refused_one_past_each(libpath):
    import h264mi
    L = h264mi.lib()
    assert h264mi.warp_ok(None) == -1
    for filt in (0, 1):
        for edge in (0, 1):
            for g in (3, 4, 5):
                assert h264mi.warp_ok((filt, edge, 0, 255, 128, g)) == 0
    for bad in ((-1, 0, 0, 0, 0, 3), (2, 0, 0, 0, 0, 3), (0, -1, 0, 0, 0, 3), (0, 2, 0, 0, 0, 3), (0, 0, -1, 0, 0, 3), (0, 0, 256, 0, 0, 3),
                (0, 0, 0, -1, 0, 3), (0, 0, 0, 256, 0, 3), (0, 0, 0, 0, -1, 3), (0, 0, 0, 0, 256, 3), (0, 0, 0, 0, 0, 2), (0, 0, 0, 0, 0, 6)):
        assert h264mi.warp_ok(bad) == -1, bad
    # the builders: null pointers, sides, pitch; a refusal writes nothing
    mesh = np.full((3, 3, 2), 0x5A5A5A5A, np.int32)
    pm = mesh.ctypes.data_as(ctypes.c_void_p)
    six, nine = (ctypes.c_int32 * 6)(65536, 0, 0, 0, 65536, 0), (ctypes.c_int32 * 9)(65536, 0, 0, 0, 65536, 0, 0, 0, 65536)
    assert L.h264mi_warp_mesh_affine(None, 16, 16, 3, six) == -1 and L.h264mi_warp_mesh_affine(pm, 16, 16, 3, None) == -1
    assert L.h264mi_warp_mesh_homography(None, 16, 16, 3, nine) == -1 and L.h264mi_warp_mesh_homography(pm, 16, 16, 3, None) == -1
    assert L.h264mi_warp_mesh_radial(None, 16, 16, 3, 0, 0, 1 << 20, 0, 0) == -1
    for dw, dh, g in ((0, 16, 3), (15, 16, 3), (8194, 16, 3), (16, 8194, 3), (16, 16, 2), (16, 16, 6)):
        assert L.h264mi_warp_mesh_affine(pm, dw, dh, g, six) == -1 and L.h264mi_warp_mesh_homography(pm, dw, dh, g, nine) == -1
        assert L.h264mi_warp_mesh_radial(pm, dw, dh, g, 0, 0, 1 << 20, 0, 0) == -1
    assert L.h264mi_warp_mesh_affine(pm, 16, 16, 3, six) == 9 and (mesh[..., 0] == 16 * 8 * np.arange(3)[None, :]).all()
    mesh[:] = 0x5A5A5A5A
    # the homography: a denominator that reaches 0 or below at one control point, the last one included
    for h in ([65536, 0, 0, 0, 65536, 0, 0, 0, 0], [65536, 0, 0, 0, 65536, 0, -1, 0, 16], [65536, 0, 0, 0, 65536, 0, 0, -1, 16],
              [65536, 0, 0, 0, 65536, 0, -1, -1, 32], [65536, 0, 0, 0, 65536, 0, 1, 1, -1]):
        assert L.h264mi_warp_mesh_homography(pm, 16, 16, 3, (ctypes.c_int32 * 9)(*h)) == -1, h
        assert warpref.mesh_homography(16, 16, 3, h) is None
    assert L.h264mi_warp_mesh_homography(pm, 16, 16, 3, (ctypes.c_int32 * 9)(65536, 0, 0, 0, 65536, 0, -1, -1, 33)) == 9
    mesh[:] = 0x5A5A5A5A
    # the radial builder: at each limit it is taken, one past it refused
    C, K, R2, Q = warpref.RADIAL_MAX_CENTRE, warpref.RADIAL_MAX_K, warpref.RADIAL_MAX_R2, warpref.RADIAL_MAX_Q
    for args, ok in (((C, -C, R2, K, -K), True), ((C + 1, 0, R2, 0, 0), False), ((-C - 1, 0, R2, 0, 0), False), ((0, C + 1, R2, 0, 0), False),
                     ((0, -C - 1, R2, 0, 0), False), ((0, 0, R2 + 1, 0, 0), False), ((0, 0, 0, 0, 0), False), ((0, 0, -1, 0, 0), False),
                     ((0, 0, R2, K + 1, 0), False), ((0, 0, R2, -K - 1, 0), False), ((0, 0, R2, 0, K + 1), False), ((0, 0, R2, 0, -K - 1), False)):
        mesh[:] = 0x5A5A5A5A
        r = L.h264mi_warp_mesh_radial(pm, 16, 16, 3, *args)
        assert r == (9 if ok else -1), args
        assert ok or (mesh == 0x5A5A5A5A).all(), args
        assert (warpref.mesh_radial(16, 16, 3, *args) is not None) == ok
    # q: the far corner of the 16x16 mesh is 16 * 16 sixteenths from the centre both ways, so q = 2 * 256^2 * 2^16 / r2
    r2_at = (2 * 256 * 256 << 16) // Q  # q == 2^24 exactly
    mesh[:] = 0x5A5A5A5A
    assert L.h264mi_warp_mesh_radial(pm, 16, 16, 3, 0, 0, r2_at, 1, 1) == 9
    mesh[:] = 0x5A5A5A5A
    assert L.h264mi_warp_mesh_radial(pm, 16, 16, 3, 0, 0, r2_at - 1, 1, 1) == -1 and (mesh == 0x5A5A5A5A).all()
    assert warpref.mesh_radial(16, 16, 3, 0, 0, r2_at, 1, 1) is not None and warpref.mesh_radial(16, 16, 3, 0, 0, r2_at - 1, 1, 1) is None
    # the host restatement refuses what the device call refuses of one frame
    src, dst = np.zeros(warpref.frame_bytes(16, 16), np.uint8), np.zeros(warpref.frame_bytes(16, 16) + 8, np.uint8)
    ps, pd = src.ctypes.data_as(ctypes.c_void_p), dst.ctypes.data_as(ctypes.c_void_p)
    good = h264mi.Warp(1, 0, 0, 0, 0, 3)
    mesh[:] = warpref.mesh(0, (16, 16), (16, 16), 3)
    fn = L.h264mi_i420_warp_host
    assert fn(pd, 16, 16, ps, 16, 16, pm, ctypes.byref(good)) == 0
    assert fn(None, 16, 16, ps, 16, 16, pm, ctypes.byref(good)) == -1 and fn(pd, 16, 16, None, 16, 16, pm, ctypes.byref(good)) == -1
    assert fn(pd, 16, 16, ps, 16, 16, None, ctypes.byref(good)) == -1 and fn(pd, 16, 16, ps, 16, 16, pm, None) == -1
    assert fn(pd, 16, 16, ps, 16, 16, pm, ctypes.byref(h264mi.Warp(1, 0, 0, 0, 0, 6))) == -1
    assert fn(pd, 18, 16, ps, 16, 15, pm, ctypes.byref(good)) == -1 and fn(pd, 8194, 16, ps, 16, 16, pm, ctypes.byref(good)) == -1
    assert fn(ps, 16, 16, ps, 16, 16, pm, ctypes.byref(good)) == -1 and fn(pm, 2, 2, ps, 16, 16, pm, ctypes.byref(good)) == -1
    assert fn(pd, 16, 16, ps, 16, 16, ctypes.c_void_p(mesh.ctypes.data + 2), ctypes.byref(good)) == -1


def test_the_shared_mesh_set_reaches_both_kernel_classes(libpath):
    """the kernel stages a tile's source footprint in LDS when it is small and samples global memory otherwise
    (h264mi_warp_tile_class, the helper the kernel itself decides with). Over the shapes, pitches and meshes the GPU test
    runs, both classes occur in every plane kind and at every pitch; the zoom out reaches the fallback, the zoom in,
    the identity and the rotation stay staged"""
    import h264mi
    seen = {}
    for src, dst, _ in warpref.SHAPES:
        for g in warpref.GRIDS:
            mw, mh = warpref.mesh_size(dst[0], dst[1], g)
            tiles = [(tx, ty) for ty in sorted({0, (mh - 2) // 2, mh - 2}) for tx in sorted({0, (mw - 2) // 2, mw - 2})]
            for k, (name, _) in enumerate(warpref.MESHES):
                for plane in range(3):
                    for tx, ty in tiles:
                        c = h264mi.warp_tile_class(warpref.mesh(k, src, dst, g), dst[0], dst[1], src[0], src[1], g, plane, tx, ty)
                        assert c in (0, 1)
                        seen.setdefault((name, g, plane != 0), set()).add(c)
    for g in warpref.GRIDS:
        for chroma in (False, True):
            classes = set().union(*(v for (name, gg, cc), v in seen.items() if gg == g and cc == chroma))
            assert classes == {0, 1}, f'pitch {1 << g}, chroma {chroma}: only {classes} reached'
            # a chroma tile at pitch 8 is 4 x 4 samples: shrunk by 8 its footprint is 36 x 36, which is staged
            assert chroma or 1 in seen[('zoom-out-8', g, chroma)], f'the zoom out never leaves the staged class at pitch {1 << g}'
            for name in ('identity', 'rotate7', 'zoom-in-4'):
                assert seen[(name, g, chroma)] == {0}, (name, g, chroma)
    with pytest.raises(ValueError):
        h264mi.warp_tile_class(warpref.mesh(0, (16, 16), (16, 16), 3), 16, 16, 16, 16, 3, 0, 2, 0)
    with pytest.raises(ValueError):
        h264mi.warp_tile_class(warpref.mesh(0, (16, 16), (16, 16), 3), 16, 16, 16, 16, 3, 3, 0, 0)
