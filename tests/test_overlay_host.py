"""CPU: the overlay blend exists at every layer -- declared in include/h264mi.h, exported by the library, bound in
Python --, tests/overlayref.py (the reference of the GPU tests) has the properties the definition promises, and the
device calls refuse bad arguments before touching a device."""
import ctypes

import numpy as np
import pytest

import overlayref
import scaleref
from overlayref import O
from test_capi_exports import declared_functions

NEW = {'h264mi_rgba_to_i420a_dev': 6, 'h264mi_i420_overlay_dev': 11, 'h264mi_enc_set_overlays': 7, 'h264mi_enc_overlays': 1}


def test_header_declares_library_exports_python_binds(libpath):
    names = declared_functions()
    L = ctypes.CDLL(libpath)
    import h264mi
    B = h264mi.lib()
    for n, nargs in NEW.items():
        assert n in names, n
        assert hasattr(L, n), n
        assert getattr(B, n).argtypes is not None and len(getattr(B, n).argtypes) == nargs, n
    assert ctypes.sizeof(h264mi.Overlay) == 40
    assert [k for k, _ in h264mi.Overlay._fields_] == list(overlayref.FIELDS)
    assert [k for k, _ in h264mi.Overlay._fields_] == ['sprite', 'canvas', 'sx', 'sy', 'w', 'h', 'dx', 'dy', 'opacity', 'reserved']
    assert all(t is ctypes.c_int32 for _, t in h264mi.Overlay._fields_)
    assert h264mi.i420a_bytes(38, 22) == 2 * 38 * 22 + 2 * 19 * 11 == overlayref.sprite_bytes(38, 22)
    assert callable(h264mi.i420_overlay) and callable(h264mi.rgba_to_i420a)
    for m in ('set_overlays', 'clear_overlays', 'overlays'):
        assert callable(getattr(h264mi.BatchEncoder, m)), m


# ---------------------------------------------------------------- the reference's properties

def test_division_identity_over_every_numerator():
    """t = x + 128; (t + (t >> 8)) >> 8 == (x + 127) // 255 for every numerator a blend can reach, 0..255 * 255"""
    x = np.arange(255 * 255 + 1, dtype=np.int64)
    assert x.size == 65026
    t = x + 128
    assert np.array_equal((t + (t >> 8)) >> 8, (x + 127) // 255)
    assert np.array_equal(overlayref.div255(x), (x + 127) // 255)


def test_effective_alpha_range():
    A = np.arange(256)
    for op in range(257):
        a = overlayref.effective_alpha(A, op)
        assert 0 <= a.min() and a.max() <= 255
    assert (overlayref.effective_alpha(A, 256) == A).all() and (overlayref.effective_alpha(A, 0) == 0).all()
    assert overlayref.effective_alpha(255, 256) == 255


def test_blend_lies_between_canvas_and_sprite_for_every_triple():
    d, s, a = np.meshgrid(np.arange(256), np.arange(256), np.arange(256), indexing='ij', sparse=True)
    out = overlayref.blend_samples(d, s, a)
    assert (out >= np.minimum(d, s)).all() and (out <= np.maximum(d, s)).all()
    assert (out[:, :, 0] == d[:, :, 0]).all(), 'a == 0 keeps the canvas'
    assert (out[:, :, 255] == s[:, :, 0]).all(), 'a == 255 copies the sprite'


def _frames(w, h, n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, scaleref.frame_bytes(w, h)), dtype=np.uint8)


def _sprites(w, h, n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, overlayref.sprite_bytes(w, h)), dtype=np.uint8)


def _with_alpha(sprites, w, h, value):
    out = sprites.copy()
    out[:, scaleref.frame_bytes(w, h):] = value
    return out


def test_reference_opacity_0_and_alpha_0_are_identities():
    cw, ch, ow, oh = 40, 24, 38, 22
    canvas, spr = _frames(cw, ch, 2, 31), _sprites(ow, oh, 2, 32)
    ov = [O(1, 0, 6, 2, 26, 18, 10, 4, 0), O(0, 1, 0, 0, 38, 22, 2, 2, 0)]
    assert np.array_equal(overlayref.blend(canvas, cw, ch, spr, ow, oh, ov), canvas)
    ov = [p._replace(opacity=256) for p in ov]
    assert np.array_equal(overlayref.blend(canvas, cw, ch, _with_alpha(spr, ow, oh, 0), ow, oh, ov), canvas)
    assert not np.array_equal(overlayref.blend(canvas, cw, ch, spr, ow, oh, ov), canvas)


def test_reference_opaque_is_a_copy_of_the_crop_and_the_rest_is_unchanged():
    cw, ch, ow, oh = 40, 24, 38, 22
    canvas, spr = _frames(cw, ch, 2, 33), _with_alpha(_sprites(ow, oh, 1, 34), ow, oh, 255)
    sx, sy, w, h, dx, dy = 6, 2, 26, 18, 10, 4
    out = overlayref.blend(canvas, cw, ch, spr, ow, oh, [O(0, 1, sx, sy, w, h, dx, dy, 256)])
    assert np.array_equal(out[0], canvas[0]), 'a canvas without a placement'
    touched = np.zeros_like(canvas[1])
    for p, (o, s, t) in enumerate(zip(scaleref.planes(out[1], cw, ch), overlayref.sprite_planes(spr[0], ow, oh)[:3], scaleref.planes(touched, cw, ch))):
        k = 1 if p else 0
        rect = (slice(dy >> k, (dy + h) >> k), slice(dx >> k, (dx + w) >> k))
        assert np.array_equal(o[rect], s[sy >> k:(sy + h) >> k, sx >> k:(sx + w) >> k]), f'plane {p}: the crop, copied'
        t[rect] = 1
    assert touched.sum() == w * h * 3 // 2
    assert np.array_equal(out[1][touched == 0], canvas[1][touched == 0]), 'bytes outside the rectangle'
    assert not np.shares_memory(out, canvas)


def test_reference_by_hand():
    """one 2x2 placement: four luma samples and one of each chroma, computed here with Python integers"""
    canvas = np.array([[10, 200, 30, 255, 100, 7]], np.uint8)            # 2x2: Y0..3, Cb, Cr
    spr = overlayref.make_sprite([[250, 0], [90, 255]], [[200]], [[1]], [[255, 128], [1, 0]])[None]
    out = overlayref.blend(canvas, 2, 2, spr, 2, 2, [O(0, 0, 0, 0, 2, 2, 0, 0, 200)])[0]
    al = [(A * 200 + 128) >> 8 for A in (255, 128, 1, 0)]
    assert al == [199, 100, 1, 0]
    want = [(d * (255 - a) + s * a + 127) // 255 for d, s, a in zip((10, 200, 30, 255), (250, 0, 90, 255), al)]
    ac = (sum(al) + 2) >> 2
    assert ac == 75
    want += [(100 * (255 - ac) + 200 * ac + 127) // 255, (7 * (255 - ac) + 1 * ac + 127) // 255]
    assert out.tolist() == want


def test_reference_order_matters_where_placements_overlap_and_only_there():
    cw, ch, ow, oh = 32, 32, 16, 16
    canvas, spr = _frames(cw, ch, 1, 35), _sprites(ow, oh, 2, 36)
    a, b = O(0, 0, 0, 0, 16, 16, 4, 4, 200), O(1, 0, 0, 0, 16, 16, 12, 12, 256)
    ab, ba = overlayref.blend(canvas, cw, ch, spr, ow, oh, [a, b]), overlayref.blend(canvas, cw, ch, spr, ow, oh, [b, a])
    assert not np.array_equal(ab, ba), 'two overlapping placements, reversed'
    diff = scaleref.planes(ab[0] != ba[0], cw, ch)[0]
    assert diff[12:20, 12:20].any() and not diff[:12].any() and not diff[20:].any() and not diff[:, :12].any() and not diff[:, 20:].any()
    c = O(1, 0, 0, 0, 16, 12, 4, 20, 77)  # below a: rows 20..31
    assert np.array_equal(overlayref.blend(canvas, cw, ch, spr, ow, oh, [a, c]), overlayref.blend(canvas, cw, ch, spr, ow, oh, [c, a])), \
        'two disjoint placements commute'
    one_by_one = overlayref.blend(overlayref.blend(canvas, cw, ch, spr, ow, oh, [a]), cw, ch, spr, ow, oh, [b])
    assert np.array_equal(ab, one_by_one), 'a list is its placements one after another'


def test_reference_rgba_to_i420a_by_hand():
    rgba = np.array([[255, 0, 0, 9], [0, 255, 0, 100], [0, 0, 255, 255], [255, 255, 255, 0]], np.uint8)  # 2x2
    s = overlayref.rgba_to_i420a(rgba, 2, 2)
    assert s.tolist() == [82, 144, 41, 235, 90, 240, 9, 100, 255, 0]


# ---------------------------------------------------------------- refusals, no device

def _ovs(*tuples):
    import h264mi
    return (h264mi.Overlay * len(tuples))(*[h264mi.Overlay(*t) for t in tuples])


OK = (0, 0, 0, 0, 16, 16, 0, 0, 256, 0)
# (cw, ch, ncanvas, ow, oh, nsprites, placements) that h264mi_i420_overlay_dev must refuse; the pointers are never dereferenced
BAD = [(32, 32, 0, 32, 32, 1, [OK]), (32, 32, -1, 32, 32, 1, [OK]), (32, 32, 1, 32, 32, 0, [OK]), (32, 32, 1, 32, 32, -1, [OK]),  # counts
       (32, 32, 1, 32, 32, 1, []),
       (31, 32, 1, 32, 32, 1, [OK]), (32, 31, 1, 32, 32, 1, [OK]), (32, 32, 1, 33, 32, 1, [OK]), (32, 32, 1, 32, 33, 1, [OK]),     # odd sizes
       (0, 32, 1, 32, 32, 1, [OK]), (32, 0, 1, 32, 32, 1, [OK]), (32, 32, 1, 0, 32, 1, [OK]), (32, 32, 1, 32, -2, 1, [OK]),        # below 2
       (8194, 32, 1, 32, 32, 1, [OK]), (32, 8194, 1, 32, 32, 1, [OK]), (32, 32, 1, 8194, 32, 1, [OK]), (32, 32, 1, 32, 8194, 1, [OK]),  # above 8192
       (32, 32, 1, 32, 32, 1, [(1, 0, 0, 0, 16, 16, 0, 0, 256, 0)]), (32, 32, 1, 32, 32, 1, [(-1, 0, 0, 0, 16, 16, 0, 0, 256, 0)]),  # sprite
       (32, 32, 1, 32, 32, 1, [(0, 1, 0, 0, 16, 16, 0, 0, 256, 0)]), (32, 32, 1, 32, 32, 1, [(0, -1, 0, 0, 16, 16, 0, 0, 256, 0)]),  # canvas
       (32, 32, 1, 32, 32, 1, [(0, 0, 18, 0, 16, 16, 0, 0, 256, 0)]), (32, 32, 1, 32, 32, 1, [(0, 0, 0, 18, 16, 16, 0, 0, 256, 0)]),  # crop
       (32, 32, 1, 32, 32, 1, [(0, 0, -2, 0, 16, 16, 0, 0, 256, 0)]), (32, 32, 1, 32, 32, 1, [(0, 0, 0, -2, 16, 16, 0, 0, 256, 0)]),
       (32, 32, 1, 32, 32, 1, [(0, 0, 2147483646, 0, 4, 4, 0, 0, 256, 0)]), (64, 64, 1, 32, 32, 1, [(0, 0, 0, 0, 34, 16, 0, 0, 256, 0)]),
       (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, 0, 16, 0, 0, 256, 0)]), (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 0, 0, 0, 256, 0)]),     # w, h below 2
       (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, -2, 16, 0, 0, 256, 0)]),
       (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, 18, 0, 256, 0)]), (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, 0, 18, 256, 0)]),  # rectangle
       (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, -2, 0, 256, 0)]), (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, 0, -2, 256, 0)]),
       (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, 4, 4, 2147483646, 0, 256, 0)]), (16, 16, 1, 32, 32, 1, [(0, 0, 0, 0, 18, 16, 0, 0, 256, 0)]),
       (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, 0, 0, 257, 0)]), (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, 0, 0, -1, 0)]),     # opacity
       (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, 0, 0, 256, 1)]), (32, 32, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, 0, 0, 256, -1)]),   # reserved
       (32, 32, 1, 32, 32, 1, [OK, OK, (0, 0, 0, 0, 16, 16, 0, 0, 300, 0)])]                                                        # the last of three
BAD += [(32, 32, 1, 32, 32, 1, [tuple(v + (1 if i == k else 0) for i, v in enumerate((0, 0, 2, 2, 8, 8, 4, 4, 256, 0)))]) for k in range(2, 8)]  # an odd field


def test_overlay_dev_refuses_bad_arguments_without_a_device(libpath):
    import h264mi
    fn = h264mi.lib().h264mi_i420_overlay_dev
    d, s = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x20000000)
    one = _ovs(OK)
    assert fn(None, 32, 32, 1, s, 32, 32, 1, one, 1, None) == -1
    assert fn(d, 32, 32, 1, None, 32, 32, 1, one, 1, None) == -1
    assert fn(d, 32, 32, 1, s, 32, 32, 1, None, 1, None) == -1
    assert fn(d, 32, 32, 1, s, 32, 32, 1, one, 0, None) == -1 and fn(d, 32, 32, 1, s, 32, 32, 1, one, -1, None) == -1
    for cw, ch, ncanvas, ow, oh, nspr, ovs in BAD:
        arr = _ovs(*ovs) if ovs else one
        assert fn(d, cw, ch, ncanvas, s, ow, oh, nspr, arr, len(ovs), None) == -1, (cw, ch, ncanvas, ow, oh, nspr, ovs)
    many = _ovs(*[(0, 0, 0, 0, 2, 2, 2 * (k % 64), 2 * (k // 64), 256, 0) for k in range(4097)])  # one too many
    assert fn(d, 128, 256, 1, s, 32, 32, 1, many, 4097, None) == -1
    # overlapping byte ranges: a 32x32 canvas is 1536 bytes, a 32x32 sprite 2560
    base = 0x10000000
    for off in (0, 1, 2559, -1, -1535):
        assert fn(ctypes.c_void_p(base + off), 32, 32, 1, ctypes.c_void_p(base), 32, 32, 1, one, 1, None) == -1, off
    assert fn(ctypes.c_void_p(base + 3 * 2560 - 1), 32, 32, 1, ctypes.c_void_p(base), 32, 32, 3, one, 1, None) == -1  # nsprites sprites count
    assert fn(ctypes.c_void_p(base - 2 * 1536 + 1), 32, 32, 2, ctypes.c_void_p(base), 32, 32, 1, one, 1, None) == -1  # ncanvas canvases count


def test_rgba_to_i420a_dev_refuses_bad_arguments_without_a_device(libpath):
    import h264mi
    fn = h264mi.lib().h264mi_rgba_to_i420a_dev
    d, s = ctypes.c_void_p(0x10000001), ctypes.c_void_p(0x20000000)
    assert fn(None, s, 32, 32, 1, None) == -1 and fn(d, None, 32, 32, 1, None) == -1
    for off in (1, 2, 3):  # the source is 4-byte aligned
        assert fn(d, ctypes.c_void_p(0x20000000 + off), 32, 32, 1, None) == -1
    for w, h, n in ((31, 32, 1), (32, 31, 1), (0, 32, 1), (32, 0, 1), (-2, 32, 1), (32, 32, 0), (32, 32, -1), (8194, 32, 1), (32, 8194, 1)):
        assert fn(d, s, w, h, n, None) == -1, (w, h, n)


def test_encoder_entry_points_refuse_a_null_encoder(libpath):
    import h264mi
    L = h264mi.lib()
    one = _ovs(OK)
    assert L.h264mi_enc_set_overlays(None, ctypes.c_void_p(0x20000000), 32, 32, 1, one, 1) == -1
    assert L.h264mi_enc_set_overlays(None, None, 0, 0, 0, None, 0) == -1
    assert L.h264mi_enc_overlays(None) == -1


class _FakeTensor:
    """what the Python wrappers look at before they call the library: a device uint8 tensor that is never read"""
    is_cuda = True

    def __init__(self, n, ptr):
        import torch
        self.dtype, self._n, self._p = torch.uint8, n, ptr

    def is_contiguous(self):
        return True

    def numel(self):
        return self._n

    def data_ptr(self):
        return self._p


class _NoStream:
    cuda_stream = 0


def test_python_wrappers_raise_value_error(libpath):
    import h264mi
    canvas, spr = _FakeTensor(1 << 40, 0x10000000), _FakeTensor(1 << 40, 0x20000000)
    for cw, ch, ncanvas, ow, oh, nspr, ovs in BAD:
        with pytest.raises(ValueError):
            h264mi.i420_overlay(canvas, cw, ch, ncanvas, spr, ow, oh, nspr, [h264mi.Overlay(*t) for t in ovs], stream=_NoStream())
    with pytest.raises(ValueError):  # the canvas inside the sprites
        h264mi.i420_overlay(_FakeTensor(1536, 0x20000000 + 100), 32, 32, 1, spr, 32, 32, 1, [h264mi.Overlay(*OK)], stream=_NoStream())
    for w, h, n in ((31, 32, 1), (32, 31, 1), (32, 32, 0)):
        with pytest.raises(ValueError):
            h264mi.rgba_to_i420a(spr, canvas, w, h, n, stream=_NoStream())
