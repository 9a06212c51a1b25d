"""CPU: the spatial filter and the privacy masks exist at every layer -- declared in include/h264mi.h, exported by the
library, bound in Python --, the vectorised reference of the GPU tests (tests/spatialref.py) equals the definitions written
as loops and the library's own host restatements, the identities of the rules hold exactly, the ok-functions refuse one
past every limit, and the content and parameter sets the GPU tests share reach every class of the rules (the class audit:
a class not reached is a failure)."""
import ctypes
import functools

import numpy as np
import pytest

import spatialref as ref
from test_capi_exports import declared_functions

NEW = ('h264mi_spatial_ok', 'h264mi_i420_spatial_dev', 'h264mi_i420_spatial_host', 'h264mi_privacy_ok', 'h264mi_i420_privacy_dev',
       'h264mi_i420_privacy_host', 'h264mi_enc_set_spatial', 'h264mi_enc_spatial', 'h264mi_enc_set_privacy', 'h264mi_enc_privacy')
N = 3
AMOUNTS = (-64, -17, 40, 255)
# (radius_y, radius_c, amount_y, amount_c, core): each radius with each amount and core 0 and 3, luma and chroma settings
# that differ; then a plane kind copied by r == 0 and by amount == 0
PARAMS = [(r, r % 3 + 1, a, AMOUNTS[(k + 1) % 4], core) for r in (1, 2, 3) for k, a in enumerate(AMOUNTS) for core in (0, 3)]
PARAMS += [(0, 2, 40, 40, 3), (2, 0, -64, 40, 0), (1, 1, 0, 40, 2), (3, 3, 255, 0, 0)]
# the kernel's tile is 256 samples by 32 rows of one plane (csrc/spatial.hip); a load unit is a dword
#   2x2: chroma 1x1, every tap clamps; 4x4 and 8x6: planes narrower than 2r + 1; 16x16; 36x18: luma rows of 36 bytes move as
#   dwords, chroma rows of 18 bytes as bytes; 130x66: every plane as bytes, three tile rows of luma, chroma 65x33 one row
#   past the tile; 8192x2 and 2x8192: the limit; 260x34: luma one dword past the tile across and one (even-sized) step
#   past it down; 520x66: chroma 260x33, one dword past the tile across and one row past it down
SHAPES = [(2, 2), (4, 4), (8, 6), (16, 16), (36, 18), (130, 66), (8192, 2), (2, 8192), (260, 34), (520, 66)]
SMALL = [(2, 2), (4, 4), (8, 6), (16, 16), (36, 18)]


@functools.lru_cache(maxsize=None)
def make_frames(w, h):
    """N frames of different content as an (N, frame bytes) array, shared and never written: 0 random samples; 1 a smooth
    ramp with noise of +-2, a 0/255 checker patch and a flat patch in every plane; 2 random samples with a checker of
    2 x 2 squares and a flat patch at other places"""
    rng = np.random.default_rng(1009 * w + h)
    nb = ref.frame_bytes(w, h)
    fr = np.empty((N, nb), np.uint8)
    fr[0] = rng.integers(0, 256, nb, dtype=np.uint8)
    fr[2] = rng.integers(0, 256, nb, dtype=np.uint8)
    for pl, plane in enumerate(ref.planes(fr[1], w, h)):
        ph, pw = plane.shape
        yy, xx = np.mgrid[0:ph, 0:pw]
        plane[:, :] = np.clip(40 + (3 * xx + 2 * yy + 30 * pl) % 180 + rng.integers(-2, 3, (ph, pw)), 0, 255)
    for f, (fy, fx, step) in ((1, (0, 0, 1)), (2, (1, 1, 2))):
        for plane in ref.planes(fr[f], w, h):
            ph, pw = plane.shape
            yy, xx = np.mgrid[0:ph, 0:pw]
            y0, x0 = (ph // 4) * fy, (pw // 4) * fx
            y1, x1 = min(ph, y0 + max(ph // 3, 1)), min(pw, x0 + min(max(pw // 3, 1), 40))
            plane[y0:y1, x0:x1] = (255 * (((yy // step) + (xx // step)) & 1))[y0:y1, x0:x1]
            y2, x2 = ph - max(ph // 3, 1), pw - min(max(pw // 3, 1), 40)
            plane[y2:, x2:] = 77
    fr.setflags(write=False)
    return fr


def privacy_lists(w, h):
    """the mask lists the GPU tests share, for N frames of w x h >= 130x66"""
    P, F = ref.PIXELATE, ref.FILL
    return {
        'block4-partial': [(0, 2, 4, 126, 58, P, 4, 0, 0, 0)],
        'block64-whole-frame': [(1, 0, 0, w, h, P, 64, 0, 0, 0)],
        'block4-whole-frame': [(2, 0, 0, w, h, P, 4, 0, 0, 0)],
        '2x2': [(1, 10, 20, 2, 2, P, 4, 0, 0, 0)],
        'mixed': [(0, 0, 0, 64, 32, P, 8, 0, 0, 0), (0, 64, 32, w - 64, h - 32, P, 32, 0, 0, 0), (1, 32, 16, 16, 16, P, 16, 0, 0, 0),
                  (2, 6, 2, 100, 50, F, 0, 17, 200, 90), (1, 100, 40, 30, 26, F, 0, 0, 255, 128), (1, 2, 40, 64, 6, P, 64, 1, 2, 3)],
    }


def test_header_declares_library_exports_python_binds(libpath):
    names = declared_functions()
    L = ctypes.CDLL(libpath)
    for n in NEW:
        assert n in names, n
        assert hasattr(L, n), n
    import h264mi
    B = h264mi.lib()
    assert [len(getattr(B, n).argtypes) for n in NEW] == [1, 7, 5, 5, 7, 6, 2, 2, 3, 1]
    for f in ('i420_spatial', 'spatial_ok', 'i420_privacy', 'privacy_ok'):
        assert callable(getattr(h264mi, f)), f
    for f in ('set_spatial', 'spatial', 'set_privacy', 'privacy'):
        assert callable(getattr(h264mi.BatchEncoder, f)), f
    assert ctypes.sizeof(h264mi.Spatial) == 20 and ctypes.sizeof(h264mi.Privacy) == 40
    assert [k for k, _ in h264mi.Spatial._fields_] == ['radius_y', 'radius_c', 'amount_y', 'amount_c', 'core']
    assert [k for k, _ in h264mi.Privacy._fields_] == ['frame', 'x', 'y', 'w', 'h', 'mode', 'block', 'fill_y', 'fill_cb', 'fill_cr']
    assert (h264mi.PRIVACY_PIXELATE, h264mi.PRIVACY_FILL) == (ref.PIXELATE, ref.FILL) == (0, 1)


@pytest.mark.parametrize('w,h', SMALL, ids=[f'{w}x{h}' for w, h in SMALL])
def test_vectorised_reference_equals_the_loops(w, h):
    fr = make_frames(w, h)
    for k, params in enumerate(PARAMS):
        f = fr[k % N]
        assert np.array_equal(ref.spatial_frame(f, w, h, params), ref.spatial_frame_loops(f, w, h, params)), params


def _lib_spatial(frame, w, h, params):
    import h264mi
    out = np.full(frame.size, 0x5A, np.uint8)
    src = np.ascontiguousarray(frame)
    assert h264mi.lib().h264mi_i420_spatial_host(out.ctypes.data, src.ctypes.data, w, h, ctypes.byref(h264mi.Spatial(*params))) == 0
    return out


@pytest.mark.parametrize('w,h', SMALL + [(130, 66)], ids=[f'{w}x{h}' for w, h in SMALL + [(130, 66)]])
def test_library_host_restatement_equals_the_reference(libpath, w, h):
    fr = make_frames(w, h)
    for k, params in enumerate(PARAMS):
        f = fr[k % N]
        assert np.array_equal(_lib_spatial(f, w, h, params), ref.spatial_frame(f, w, h, params)), params


def test_identities_and_the_pure_blur():
    for w, h in ((36, 18), (8, 6), (2, 2)):
        for f in make_frames(w, h):
            for r in (1, 2, 3):
                out = ref.spatial_frame(f, w, h, (r, r, -64, -64, 5))
                for o, s in zip(ref.planes(out, w, h), ref.planes(f, w, h)):
                    assert np.array_equal(o, ref.lowpass(s, r)), 'amount -64 is the low-pass itself'
                assert np.array_equal(ref.spatial_frame(f, w, h, (r, r, 0, 0, 0)), f), 'amount 0 copies'
                assert np.array_equal(ref.spatial_frame(f, w, h, (0, 0, 255, -64, 3)), f), 'radius 0 copies'
                mixed = ref.spatial_frame(f, w, h, (r, 0, 255, 255, 0))
                assert np.array_equal(mixed[w * h:], f[w * h:])
    assert ref.inert((0, 3, 40, 0, 1)) and ref.inert((2, 0, 0, 40, 1)) and not ref.inert((1, 0, 1, 0, 0))
    flat = np.full(ref.frame_bytes(16, 16), 200, np.uint8)
    for params in PARAMS:
        assert np.array_equal(ref.spatial_frame(flat, 16, 16, params), flat), 'a flat picture is a fixed point'


def test_separable_and_direct_sums_agree():
    for w, h in SMALL + [(130, 66)]:
        for f in make_frames(w, h):
            for plane in ref.planes(f, w, h):
                for r in (1, 2, 3):
                    assert np.array_equal(ref.lowpass(plane, r), ref.lowpass_direct(plane, r))
    for r, wt in ref.WEIGHTS.items():
        assert len(wt) == 2 * r + 1 and sum(wt) == 4 ** r and 255 * sum(wt) < 65536


def test_the_sample_rule():
    assert ref.sample(100, 90, 64, 0) == 110 and ref.sample(100, 90, -64, 0) == 90
    assert ref.sample(100, 97, 255, 3) == 100 and ref.sample(100, 96, 255, 3) == 100 + ((255 * 4 + 32) >> 6)
    assert ref.sample(100, 97, -17, 3) == 100 + ((-17 * 3 + 32) >> 6) == 99, 'the core does not gate a negative amount; the shift floors'
    assert ref.sample(250, 0, 255, 0) == 255 and ref.sample(5, 255, 255, 0) == 0
    for c in range(0, 256, 5):
        for l in range(0, 256, 3):
            assert ref.sample(c, l, -64, 0) == l


def test_privacy_reference_equals_the_loops_and_the_library(libpath):
    import h264mi
    w, h = 130, 66
    fr = make_frames(w, h)
    for name, masks in privacy_lists(w, h).items():
        want = ref.privacy_frames(fr, w, h, masks)
        if name != 'block4-whole-frame':
            assert np.array_equal(want, ref.privacy_frames_loops(fr, w, h, masks)), name
        got = np.array(fr, copy=True)
        arr = h264mi._privacy_array(masks)
        assert h264mi.lib().h264mi_i420_privacy_host(got.ctypes.data, w, h, N, arr, len(arr)) == 0
        assert np.array_equal(got, want), name
        assert not np.array_equal(want, fr)
        assert np.array_equal(ref.privacy_frames(want, w, h, masks), want), 'pixelate and fill are idempotent'
        untouched = np.ones((N, ref.frame_bytes(w, h)), bool)
        for f, x, y, mw, mh, *_ in masks:
            for pl, plane in enumerate(ref.planes(untouched[f], w, h)):
                s = 1 if pl else 0
                plane[y >> s:(y + mh) >> s, x >> s:(x + mw) >> s] = False
        assert np.array_equal(want[untouched], fr[untouched]), 'samples outside the rectangles'
    filled = ref.privacy_frames(fr, w, h, [(2, 6, 2, 100, 50, ref.FILL, 0, 17, 200, 90)])
    Y, U, V = ref.planes(filled[2], w, h)
    assert (Y[2:52, 6:106] == 17).all() and (U[1:26, 3:53] == 200).all() and (V[1:26, 3:53] == 90).all()


GOOD = (1, 2, 40, -17, 3)
BAD_PARAMS = [(-1, 1, 40, 40, 0), (4, 1, 40, 40, 0), (1, -1, 40, 40, 0), (1, 4, 40, 40, 0), (1, 1, -65, 40, 0), (1, 1, 256, 40, 0),
              (1, 1, 40, -65, 0), (1, 1, 40, 256, 0), (1, 1, 40, 40, -1), (1, 1, 40, 40, 256)]
LIMIT_PARAMS = [(0, 0, -64, -64, 0), (3, 3, 255, 255, 255), (0, 3, 255, -64, 255), (3, 0, -64, 255, 0)]
# (w, h, n) that h264mi_i420_spatial_dev must refuse; the pointers are never dereferenced
BAD_SHAPES = [(32, 32, 0), (32, 32, -1), (31, 32, 1), (32, 31, 1), (0, 32, 1), (32, 0, 1), (-2, 32, 1), (8194, 32, 1), (32, 8194, 1)]
P, F = ref.PIXELATE, ref.FILL
# for 2 frames of 32x16
GOOD_MASKS = [[(0, 0, 0, 32, 16, P, 4, 0, 0, 0)], [(1, 30, 14, 2, 2, P, 64, 0, 0, 0)], [(0, 0, 0, 2, 2, F, 0, 0, 0, 0)],
              [(1, 2, 2, 4, 4, F, 99, 255, 255, 255)], [(0, 0, 0, 16, 16, P, 8, 999, -1, 999)],
              [(0, 0, 0, 16, 16, P, 8, 0, 0, 0), (0, 16, 0, 16, 16, P, 16, 0, 0, 0), (1, 0, 0, 16, 16, P, 32, 0, 0, 0)],
              [(0, 0, 0, 16, 8, P, 8, 0, 0, 0), (0, 0, 8, 16, 8, F, 0, 1, 2, 3)]]
BAD_MASKS = [[(2, 0, 0, 4, 4, P, 4, 0, 0, 0)], [(-1, 0, 0, 4, 4, P, 4, 0, 0, 0)], [(0, 1, 0, 4, 4, P, 4, 0, 0, 0)], [(0, 0, 1, 4, 4, P, 4, 0, 0, 0)],
             [(0, 0, 0, 3, 4, P, 4, 0, 0, 0)], [(0, 0, 0, 4, 3, P, 4, 0, 0, 0)], [(0, 0, 0, 0, 4, P, 4, 0, 0, 0)], [(0, 0, 0, 4, 0, P, 4, 0, 0, 0)],
             [(0, -2, 0, 4, 4, P, 4, 0, 0, 0)], [(0, 0, -2, 4, 4, P, 4, 0, 0, 0)], [(0, 30, 0, 4, 4, P, 4, 0, 0, 0)], [(0, 0, 14, 4, 4, P, 4, 0, 0, 0)],
             [(0, 0, 0, 34, 4, P, 4, 0, 0, 0)], [(0, 0, 0, 4, 18, P, 4, 0, 0, 0)], [(0, 32, 0, 2, 2, P, 4, 0, 0, 0)],
             [(0, 2147483646, 0, 4, 4, P, 4, 0, 0, 0)], [(0, 0, 0, 2147483646, 4, P, 4, 0, 0, 0)],
             [(0, 0, 0, 4, 4, P, 0, 0, 0, 0)], [(0, 0, 0, 4, 4, P, 2, 0, 0, 0)], [(0, 0, 0, 4, 4, P, 6, 0, 0, 0)], [(0, 0, 0, 4, 4, P, 128, 0, 0, 0)],
             [(0, 0, 0, 4, 4, 2, 4, 0, 0, 0)], [(0, 0, 0, 4, 4, -1, 4, 0, 0, 0)],
             [(0, 0, 0, 4, 4, F, 0, 256, 0, 0)], [(0, 0, 0, 4, 4, F, 0, 0, -1, 0)], [(0, 0, 0, 4, 4, F, 0, 0, 0, 256)],
             [(0, 0, 0, 16, 16, P, 8, 0, 0, 0), (0, 14, 14, 4, 4, P, 8, 0, 0, 0)], [(1, 0, 0, 4, 4, F, 0, 1, 1, 1), (1, 0, 0, 4, 4, F, 0, 1, 1, 1)]]


def test_ok_functions_at_the_limits(libpath):
    import h264mi
    B = h264mi.lib()
    for p in LIMIT_PARAMS + PARAMS:
        assert h264mi.spatial_ok(p) == 0 and ref.params_ok(p), p
    for p in BAD_PARAMS:
        assert h264mi.spatial_ok(p) == -1 and not ref.params_ok(p), p
        assert B.h264mi_spatial_ok(ctypes.byref(h264mi.Spatial(*p))) == -1
    assert h264mi.spatial_ok(None) == -1 and B.h264mi_spatial_ok(None) == -1
    for masks in GOOD_MASKS:
        assert h264mi.privacy_ok(masks, 32, 16, 2) == 0 and ref.masks_ok(masks, 32, 16, 2), masks
    for masks in BAD_MASKS:
        assert h264mi.privacy_ok(masks, 32, 16, 2) == -1 and not ref.masks_ok(masks, 32, 16, 2), masks
    one = GOOD_MASKS[0]
    assert h264mi.privacy_ok(one, 32, 16, 1) == 0 and h264mi.privacy_ok(one, 32, 16, 0) == -1
    for w, h in ((31, 16), (32, 15), (0, 16), (8194, 16), (32, 8194)):
        assert h264mi.privacy_ok(one, w, h, 2) == -1, (w, h)
    assert h264mi.privacy_ok([], 32, 16, 2) == -1 and h264mi.privacy_ok(None, 32, 16, 2) == -1
    arr = h264mi._privacy_array(one)
    assert B.h264mi_privacy_ok(arr, 0, 32, 16, 2) == -1 and B.h264mi_privacy_ok(arr, -1, 32, 16, 2) == -1 and B.h264mi_privacy_ok(None, 1, 32, 16, 2) == -1
    # the longest list and one more: 4096 disjoint 2x2 rectangles of one 8192x2 frame
    many = [(0, 2 * k, 0, 2, 2, F, 0, 1, 2, 3) for k in range(ref.MAX_LIST + 1)]
    assert h264mi.privacy_ok(many[:ref.MAX_LIST], 8192, 2, 1) == 0 and h264mi.privacy_ok(many, 8194 - 2, 2, 1) == -1
    # the encoder's entry points on a null encoder
    assert B.h264mi_enc_set_spatial(None, ctypes.byref(h264mi.Spatial(*GOOD))) == -1 and B.h264mi_enc_spatial(None, None) == -1
    assert B.h264mi_enc_set_privacy(None, arr, 1) == -1 and B.h264mi_enc_privacy(None) == -1


def test_dev_calls_refuse_bad_arguments_without_a_device(libpath):
    import h264mi
    B = h264mi.lib()
    vp = ctypes.c_void_p
    good = ctypes.byref(h264mi.Spatial(*GOOD))
    n, fb = 3, ref.frame_bytes(32, 16)
    D, S = 0x10000000, 0x20000000

    def call(dst=D, src=S, w=32, h=16, nn=n, p=good):
        return B.h264mi_i420_spatial_dev(vp(dst) if dst else None, vp(src) if src else None, w, h, nn, p, None)

    assert call(dst=0) == -1 and call(src=0) == -1 and call(p=None) == -1
    for w, h, nn in BAD_SHAPES:
        assert call(w=w, h=h, nn=nn) == -1, (w, h, nn)
    for p in BAD_PARAMS:
        assert call(p=ctypes.byref(h264mi.Spatial(*p))) == -1, p
    for off in (0, 1, n * fb - 1, -1, -(n * fb - 1)):  # in place, and partial overlaps from above and below
        assert call(dst=S + off) == -1, off
    arr = h264mi._privacy_array(GOOD_MASKS[0])
    assert B.h264mi_i420_privacy_dev(None, 32, 16, 2, arr, 1, None) == -1
    for masks in BAD_MASKS:
        a = h264mi._privacy_array(masks)
        assert B.h264mi_i420_privacy_dev(vp(D), 32, 16, 2, a, len(a), None) == -1, masks
    assert B.h264mi_i420_privacy_dev(vp(D), 32, 16, 2, arr, 0, None) == -1 and B.h264mi_i420_privacy_dev(vp(D), 32, 16, 2, None, 1, None) == -1


def test_class_audit_of_the_shared_content():
    """every class of the two rules is reached by the reference alone on the content and parameters the GPU tests use"""
    total = dict.fromkeys(('keep', 'filtered', 'clip0', 'clip255', 'negative'), 0)
    radius = {(kind, r): 0 for kind in 'yc' for r in (1, 2, 3)}
    edges = dict.fromkeys(('left', 'right', 'top', 'bottom', 'corner', 'narrower-than-the-stencil'), 0)
    for w, h in SHAPES:
        fr = make_frames(w, h)
        for params in PARAMS:
            ry, rc, ay, ac, _ = params
            per_shape = dict.fromkeys(total, 0)
            for f in fr:
                for k, v in ref.spatial_classes(f, w, h, params).items():
                    per_shape[k] += v
                    total[k] += v
            for kind, r, amount, (pw, ph) in (('y', ry, ay, (w, h)), ('c', rc, ac, (w // 2, h // 2))):
                if r == 0 or amount == 0:
                    continue
                radius[(kind, r)] += N * pw * ph
                edges['left'] += min(r, pw) * ph
                edges['right'] += min(r, pw) * ph
                edges['top'] += min(r, ph) * pw
                edges['bottom'] += min(r, ph) * pw
                edges['corner'] += 4 * min(r, pw) * min(r, ph)
                edges['narrower-than-the-stencil'] += int(pw < 2 * r + 1 or ph < 2 * r + 1)
            if min(w, h) >= 16 and ay > 0 and ac > 0 and ry and rc:
                assert per_shape['keep'] > 0 and per_shape['filtered'] > 0, (w, h, params, per_shape)
        if min(w, h) >= 16:  # each of these shapes reaches both clips on its own
            sharp = [ref.spatial_classes(f, w, h, (1, 1, 255, 255, 0)) for f in fr]
            assert sum(s['clip0'] for s in sharp) > 0 and sum(s['clip255'] for s in sharp) > 0, (w, h)
    for name, table in (('rule', total), ('radius', radius), ('edges', edges)):
        missed = [k for k, v in table.items() if v == 0]
        assert not missed, f'{name}: classes not reached: {missed}'
    cells = dict.fromkeys(('whole', 'right', 'bottom', 'both', 'one_cell', 'fill'), 0)
    for masks in privacy_lists(130, 66).values():
        for k, v in ref.privacy_classes(masks).items():
            cells[k] += v
    missed = [k for k, v in cells.items() if v == 0]
    assert not missed, f'privacy: classes not reached: {missed}'
    blocks = {m[6] for masks in privacy_lists(130, 66).values() for m in masks if m[5] == ref.PIXELATE}
    assert blocks == set(ref.BLOCKS)
