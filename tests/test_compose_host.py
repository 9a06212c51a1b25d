"""CPU: the I420 compositor exists at every layer -- declared in include/h264mi.h, exported by the library, bound in
Python --, h264mi_mosaic_cells equals its plain-integer restatement, tests/composeref.py (the reference of the GPU
tests) has the properties the definition promises, and the device calls refuse bad arguments before touching a device."""
import ctypes

import numpy as np
import pytest

import composeref
import scaleref
from test_capi_exports import declared_functions

NEW = {'h264mi_i420_compose_dev': 11, 'h264mi_i420_fill_dev': 8, 'h264mi_mosaic_cells': 7, 'h264mi_enc_encode_composed': 10}
# (src_w, src_h, cw, ch)
SIZES = [(1920, 1080, 1920, 1080), (64, 36, 48, 48), (176, 144, 352, 288), (4096, 2160, 640, 360), (32, 32, 32, 32), (1280, 720, 854, 480),
         (16, 16, 160, 112), (36, 18, 50, 22)]


def test_header_declares_library_exports_python_binds(libpath):
    names = declared_functions()
    L = ctypes.CDLL(libpath)
    import h264mi
    B = h264mi.lib()
    for n, nargs in NEW.items():
        assert n in names, n
        assert hasattr(L, n), n
        assert getattr(B, n).argtypes is not None and len(getattr(B, n).argtypes) == nargs, n
    assert ctypes.sizeof(h264mi.Cell) == 40
    assert [k for k, _ in h264mi.Cell._fields_] == list(composeref.FIELDS)
    assert callable(h264mi.i420_compose) and callable(h264mi.i420_fill) and callable(h264mi.mosaic_cells)
    assert callable(h264mi.BatchEncoder.encode_composed)


@pytest.mark.parametrize('src_w,src_h,cw,ch', SIZES, ids=[f'{a}x{b}-on-{c}x{d}' for a, b, c, d in SIZES])
def test_mosaic_cells_equals_the_restatement(libpath, src_w, src_h, cw, ch):
    import h264mi
    fn = h264mi.lib().h264mi_mosaic_cells
    for n in range(1, 18):
        want = composeref.mosaic_cells(n, src_w, src_h, cw, ch)
        out = (h264mi.Cell * n)()
        if want is None:
            assert fn(out, n, n, src_w, src_h, cw, ch) == -1, n
            with pytest.raises(ValueError):
                h264mi.mosaic_cells(n, src_w, src_h, cw, ch)
            continue
        assert fn(out, n, n, src_w, src_h, cw, ch) == n, n
        assert [composeref.as_tuple(c) for c in out] == [tuple(c) for c in want], n
        assert [composeref.as_tuple(c) for c in h264mi.mosaic_cells(n, src_w, src_h, cw, ch)] == [tuple(c) for c in want]
        for c in want:  # inside the canvas, even, never enlarged, no two sharing a sample
            assert all(v % 2 == 0 for v in c[2:]) and 0 <= c.dx and c.dx + c.dw <= cw and 0 <= c.dy and c.dy + c.dh <= ch
            assert 2 <= c.dw <= src_w and 2 <= c.dh <= src_h
        for i, a in enumerate(want):
            for b in want[:i]:
                assert not (a.dx < b.dx + b.dw and b.dx < a.dx + a.dw and a.dy < b.dy + b.dh and b.dy < a.dy + a.dh)


def test_mosaic_examples_by_hand(libpath):
    import h264mi
    cells = h264mi.mosaic_cells(16, 1920, 1080, 1920, 1080)
    assert [composeref.as_tuple(c) for c in cells] == [(k, 0, 0, 0, 1920, 1080, 480 * (k % 4), 270 * (k // 4), 480, 270) for k in range(16)]
    (c,) = h264mi.mosaic_cells(1, 64, 36, 48, 48)
    assert composeref.as_tuple(c) == (0, 0, 0, 0, 64, 36, 0, 10, 48, 26)
    cells = h264mi.mosaic_cells(4, 176, 144, 352, 288)  # slots of the source's size: capped there, not enlarged
    assert [composeref.as_tuple(c) for c in cells] == [(k, 0, 0, 0, 176, 144, 176 * (k % 2), 144 * (k // 2), 176, 144) for k in range(4)]
    (c,) = h264mi.mosaic_cells(1, 176, 144, 352, 288)  # one source in a larger slot: its own size, centred
    assert composeref.as_tuple(c) == (0, 0, 0, 0, 176, 144, 88, 72, 176, 144)


def test_mosaic_refusals(libpath):
    import h264mi
    fn = h264mi.lib().h264mi_mosaic_cells
    out = (h264mi.Cell * 16)()
    assert fn(out, 16, 16, 1920, 1080, 1920, 1080) == 16
    assert fn(None, 16, 16, 1920, 1080, 1920, 1080) == -1
    assert fn(out, 15, 16, 1920, 1080, 1920, 1080) == -1  # cap < n
    assert fn(out, 16, 0, 1920, 1080, 1920, 1080) == -1 and fn(out, 16, -1, 1920, 1080, 1920, 1080) == -1
    for bad in ((1919, 1080, 1920, 1080), (1920, 1079, 1920, 1080), (1920, 1080, 1921, 1080), (1920, 1080, 1920, 1081),
                (0, 1080, 1920, 1080), (1920, 0, 1920, 1080), (1920, 1080, 0, 1080), (1920, 1080, 1920, -2)):
        assert fn(out, 16, 4, *bad) == -1, bad
    assert fn(out, 16, 16, 1920, 1080, 6, 6) == -1  # four columns of a 6-wide canvas: slots of 0 or 2, a cell below 2
    assert composeref.mosaic_cells(16, 1920, 1080, 6, 6) is None
    with pytest.raises(ValueError):
        h264mi.mosaic_cells(0, 64, 36, 48, 48)


def _frames(w, h, n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, scaleref.frame_bytes(w, h)), dtype=np.uint8)


def test_reference_one_whole_frame_cell_is_the_scaler():
    for sw, sh, dw, dh in ((48, 36, 32, 24), (36, 18, 20, 10), (38, 22, 38, 10)):
        src, canvas = _frames(sw, sh, 2, 21), _frames(dw, dh, 1, 22)
        out = composeref.compose(canvas, dw, dh, src, sw, sh, [composeref.C(1, 0, 0, 0, sw, sh, 0, 0, dw, dh)])
        assert np.array_equal(out[0], scaleref.scale_frame(src[1], sw, sh, dw, dh))


def test_reference_identity_cell_copies_and_the_rest_is_unchanged():
    sw, sh, cw, ch = 64, 48, 40, 24
    src, canvas = _frames(sw, sh, 1, 23), _frames(cw, ch, 2, 24)
    cell = composeref.C(0, 1, 6, 10, 20, 12, 14, 8, 20, 12)
    out = composeref.compose(canvas, cw, ch, src, sw, sh, [cell])
    assert np.array_equal(out[0], canvas[0]), 'a canvas without a cell'
    touched = np.zeros_like(canvas[1])
    for p, (o, s, t) in enumerate(zip(scaleref.planes(out[1], cw, ch), scaleref.planes(src[0], sw, sh), scaleref.planes(touched, cw, ch))):
        k = 1 if p else 0
        rect = (slice(8 >> k, (8 + 12) >> k), slice(14 >> k, (14 + 20) >> k))
        assert np.array_equal(o[rect], s[10 >> k:(10 + 12) >> k, 6 >> k:(6 + 20) >> k]), f'plane {p}: the crop, copied'
        t[rect] = True
    assert touched.sum() == 20 * 12 * 3 // 2
    assert np.array_equal(out[1][touched == 0], canvas[1][touched == 0]), 'bytes outside the rectangle'
    assert not np.shares_memory(out, canvas)


def test_reference_scaled_crop_by_hand():
    """a 2:1 cell: every sample the rounded mean of four of the crop, per plane, at the rectangle's (halved) origin"""
    sw, sh, cw, ch = 64, 48, 40, 24
    src, canvas = _frames(sw, sh, 1, 25), _frames(cw, ch, 1, 26)
    out = composeref.compose(canvas, cw, ch, src, sw, sh, [composeref.C(0, 0, 2, 6, 36, 20, 6, 4, 18, 10)])
    y, u, _ = scaleref.planes(out[0], cw, ch)
    sy, su, _ = (p.astype(np.int32) for p in scaleref.planes(src[0], sw, sh))
    a = sy[6:26, 2:38]
    assert np.array_equal(y[4:14, 6:24], (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2)
    assert np.array_equal(u[2:7, 3:12], scaleref.scale_plane(su[3:13, 1:19].astype(np.uint8), 9, 5))


def test_reference_fill():
    f = composeref.fill(6, 4, 2, 16, 128, 129)
    assert f.shape == (2, 36) and (f[:, :24] == 16).all() and (f[:, 24:30] == 128).all() and (f[:, 30:] == 129).all()


def _cells(*tuples):
    import h264mi
    return (h264mi.Cell * len(tuples))(*[h264mi.Cell(*t) for t in tuples])


OK_CELL = (0, 0, 0, 0, 32, 32, 0, 0, 16, 16)
# (cw, ch, ncanvas, src_w, src_h, nsrc, cells) that h264mi_i420_compose_dev must refuse; the pointers are never dereferenced
BAD = [(32, 32, 0, 32, 32, 1, [OK_CELL]), (32, 32, -1, 32, 32, 1, [OK_CELL]), (32, 32, 1, 32, 32, 0, [OK_CELL]),  # counts
       (32, 32, 1, 32, 32, 1, []),
       (31, 32, 1, 32, 32, 1, [OK_CELL]), (32, 31, 1, 32, 32, 1, [OK_CELL]), (32, 32, 1, 33, 32, 1, [OK_CELL]),  # odd sizes
       (32, 32, 1, 32, 33, 1, [OK_CELL]),
       (32, 32, 1, 4098, 32, 1, [OK_CELL]), (32, 32, 1, 32, 4098, 1, [OK_CELL]),                                   # sides too large
       (8194, 32, 1, 32, 32, 1, [OK_CELL]), (32, 8194, 1, 32, 32, 1, [OK_CELL]),
       (32, 32, 1, 32, 32, 1, [(1, 0, 0, 0, 32, 32, 0, 0, 16, 16)]), (32, 32, 1, 32, 32, 1, [(-1, 0, 0, 0, 32, 32, 0, 0, 16, 16)]),  # src
       (32, 32, 1, 32, 32, 1, [(0, 1, 0, 0, 32, 32, 0, 0, 16, 16)]), (32, 32, 1, 32, 32, 1, [(0, -1, 0, 0, 32, 32, 0, 0, 16, 16)]),  # canvas
       (32, 32, 1, 32, 32, 1, [(0, 0, 2, 0, 32, 32, 0, 0, 16, 16)]), (32, 32, 1, 32, 32, 1, [(0, 0, 0, 2, 32, 32, 0, 0, 16, 16)]),   # crop
       (32, 32, 1, 32, 32, 1, [(0, 0, -2, 0, 16, 16, 0, 0, 16, 16)]), (32, 32, 1, 32, 32, 1, [(0, 0, 0, -2, 16, 16, 0, 0, 16, 16)]),
       (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, 34, 32, 0, 0, 16, 16)]), (32, 32, 1, 32, 32, 1, [(0, 0, 2147483646, 0, 4, 4, 0, 0, 4, 4)]),
       (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, 32, 32, 18, 0, 16, 16)]), (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, 32, 32, 0, 18, 16, 16)]),  # rectangle
       (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, 32, 32, -2, 0, 16, 16)]), (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, 32, 32, 0, -2, 16, 16)]),
       (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, 32, 32, 2147483646, 0, 4, 4)]),
       (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, 0, 0, 18, 16)]), (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, 0, 0, 16, 18)]),   # enlarging
       (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, 0, 0, 0, 16)]), (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, 0, 0, 16, 0)]),     # below 2
       (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, 0, 0, -2, 16)]),
       (32, 32, 1, 32, 32, 1, [OK_CELL, (0, 0, 0, 0, 32, 32, 14, 14, 16, 16)]),                                    # two cells sharing a sample
       (32, 32, 1, 32, 32, 1, [OK_CELL, (0, 0, 0, 0, 32, 32, 16, 0, 16, 16), (0, 0, 0, 0, 4, 4, 4, 4, 2, 2)]),
       (32, 32, 2, 32, 32, 1, [(0, 1, 0, 0, 32, 32, 0, 0, 16, 16), OK_CELL, (0, 1, 0, 0, 32, 32, 0, 14, 16, 16)])]
BAD += [(32, 32, 1, 32, 32, 1, [tuple(v + (1 if i == k else 0) for i, v in enumerate((0, 0, 2, 2, 16, 16, 4, 4, 8, 8)))]) for k in range(2, 10)]  # an odd field


def test_compose_dev_refuses_bad_arguments_without_a_device(libpath):
    import h264mi
    fn = h264mi.lib().h264mi_i420_compose_dev
    d, s = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x20000000)
    one = _cells(OK_CELL)
    assert fn(None, 32, 32, 1, s, 32, 32, 1, one, 1, None) == -1
    assert fn(d, 32, 32, 1, None, 32, 32, 1, one, 1, None) == -1
    assert fn(d, 32, 32, 1, s, 32, 32, 1, None, 1, None) == -1
    for cw, ch, ncanvas, sw, sh, nsrc, cells in BAD:
        arr = _cells(*cells) if cells else one
        assert fn(d, cw, ch, ncanvas, s, sw, sh, nsrc, arr, len(cells), None) == -1, (cw, ch, ncanvas, sw, sh, nsrc, cells)
    many = _cells(*[(0, 0, 0, 0, 2, 2, 2 * (k % 64), 2 * (k // 64), 2, 2) for k in range(4097)])  # disjoint cells, one too many
    assert fn(d, 128, 256, 1, s, 32, 32, 1, many, 4097, None) == -1
    # overlapping byte ranges: one 32x32 frame is 1536 bytes
    base = 0x10000000
    for off in (0, 1, 1535, -1, -1535):
        assert fn(ctypes.c_void_p(base + off), 32, 32, 1, ctypes.c_void_p(base), 32, 32, 1, one, 1, None) == -1, off
    assert fn(ctypes.c_void_p(base + 3 * 1536 - 1), 32, 32, 1, ctypes.c_void_p(base), 32, 32, 3, one, 1, None) == -1  # nsrc frames count
    assert fn(ctypes.c_void_p(base - 2 * 1536 + 1), 32, 32, 2, ctypes.c_void_p(base), 32, 32, 1, one, 1, None) == -1  # ncanvas canvases count


def test_fill_dev_refuses_bad_arguments_without_a_device(libpath):
    import h264mi
    fn = h264mi.lib().h264mi_i420_fill_dev
    d = ctypes.c_void_p(0x10000000)
    assert fn(None, 32, 32, 1, 16, 128, 128, None) == -1
    for w, h, n, y, cb, cr in ((32, 32, 0, 16, 128, 128), (32, 32, -1, 16, 128, 128), (31, 32, 1, 16, 128, 128), (32, 31, 1, 16, 128, 128),
                               (0, 32, 1, 16, 128, 128), (32, 0, 1, 16, 128, 128), (-2, 32, 1, 16, 128, 128), (32, -2, 1, 16, 128, 128),
                               (32, 32, 1, 256, 128, 128), (32, 32, 1, 16, 256, 128), (32, 32, 1, 16, 128, 256),
                               (32, 32, 1, -1, 128, 128), (32, 32, 1, 16, -1, 128), (32, 32, 1, 16, 128, -1)):
        assert fn(d, w, h, n, y, cb, cr, None) == -1, (w, h, n, y, cb, cr)


def test_encode_composed_refuses_a_null_encoder(libpath):
    import h264mi
    one = _cells(OK_CELL)
    assert h264mi.lib().h264mi_enc_encode_composed(None, ctypes.c_void_p(0x20000000), 32, 32, 1, one, 1, 16, 128, 128) == -1
