"""CPU: the colour specifications exist at every layer -- declared in include/h264mi.h, exported by the library, bound
in Python --, tests/csref.py (the reference of the GPU tests) has the properties a colour conversion must have, its
default equals the restatements the existing RGBA tests use, h264mi_colorspec_ok agrees with it, and every device call
refuses bad arguments before touching a device."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import csref
import overlayref
from test_capi_exports import declared_functions

NEW = ('h264mi_colorspec_ok', 'h264mi_rgba_to_i420_cs_dev', 'h264mi_i420_to_rgba_cs_dev', 'h264mi_rgba_to_i420a_cs_dev',
       'h264mi_enc_set_colorspec', 'h264mi_enc_colorspec', 'h264mi_dec_set_output_colorspec', 'h264mi_dec_output_colorspec')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_SPECS = [csref.Spec(*f) for f in itertools.product((0, 1), repeat=4)]


def _c(spec):
    import h264mi
    return h264mi.ColorSpec(*spec)


def test_header_declares_library_exports_python_binds(libpath):
    names = declared_functions()
    L = ctypes.CDLL(libpath)
    for n in NEW:
        assert n in names, n
        assert hasattr(L, n), n
    import h264mi
    B = h264mi.lib()
    assert [len(getattr(B, n).argtypes) for n in NEW] == [1, 7, 7, 7, 2, 2, 2, 2]
    assert ctypes.sizeof(h264mi.ColorSpec) == 16
    assert [k for k, _ in h264mi.ColorSpec._fields_] == list(csref.Spec._fields)
    assert callable(h264mi.colorspec_ok)
    import inspect
    for f in (h264mi.rgba_to_i420, h264mi.i420_to_rgba, h264mi.rgba_to_i420a):
        assert inspect.signature(f).parameters['spec'].default is None, f
    assert callable(h264mi.BatchEncoder.set_colorspec) and callable(h264mi.BatchEncoder.colorspec)
    assert callable(h264mi.BatchDecoder.set_output_colorspec) and callable(h264mi.BatchDecoder.output_colorspec)


def test_constants_agree_across_header_python_and_reference():
    import h264mi
    src = open(os.path.join(ROOT, 'include', 'h264mi.h')).read()
    for name, ref in (('MATRIX_BT601', csref.BT601), ('MATRIX_BT709', csref.BT709), ('RANGE_LIMITED', csref.LIMITED),
                      ('RANGE_FULL', csref.FULL), ('CHROMA_DOWN_TOPLEFT', csref.TOPLEFT), ('CHROMA_DOWN_AVERAGE', csref.AVERAGE),
                      ('CHROMA_UP_REPEAT', csref.REPEAT), ('CHROMA_UP_BILINEAR', csref.BILINEAR)):
        m = re.search(r'^#define H264MI_%s (\d+)' % name, src, flags=re.M)
        assert m and int(m.group(1)) == ref == getattr(h264mi, name), name
    # the header's table, row by row, is the reference's
    rows = re.findall(r'^\s+(601|709) (limited|full)\s+((?:-?\d+\s+){14}-?\d+)\s*$', src, flags=re.M)
    assert len(rows) == 4
    for mat, rng, nums in rows:
        v = [int(x) for x in nums.split()]
        key = (csref.BT709 if mat == '709' else csref.BT601, csref.FULL if rng == 'full' else csref.LIMITED)
        assert (tuple(v[0:3]), tuple(v[3:6]), tuple(v[6:9]), *v[9:]) == csref.TABLE[key], (mat, rng)
    # ... and the table the kernels get (csrc/picture_host.h), in matrix * 2 + range order
    host = open(os.path.join(ROOT, 'openh264-wasm_amd', 'csrc', 'picture_host.h')).read()
    rows = re.findall(r'^\s+\{\{(-?\d+), (-?\d+), (-?\d+)\}, \{(-?\d+), (-?\d+), (-?\d+)\}, \{(-?\d+), (-?\d+), (-?\d+)\}, ([-\d, ]+)\},', host, flags=re.M)
    assert len(rows) == 4
    for k, r in enumerate(rows):
        v = [int(x) for x in r[:9]] + [int(x) for x in r[9].split(',')]
        assert (tuple(v[0:3]), tuple(v[3:6]), tuple(v[6:9]), *v[9:]) == csref.TABLE[k >> 1, k & 1], k


def test_table_rows_sum_as_they_must():
    for (m, r), (FY, FU, FV, yo, IY, *_rest) in csref.TABLE.items():
        assert sum(FU) == 0 and sum(FV) == 0
        assert sum(FY) == (256 if r == csref.FULL else 220)
        assert (yo, IY) == ((0, 256) if r == csref.FULL else (16, 298))


def _corner_frames(w=16, h=16, seed=7100):
    """random RGBA with the cube's corners in front"""
    a = np.random.default_rng(seed).integers(0, 256, (w * h, 4), dtype=np.uint8)
    for c in range(min(8, w * h)):
        a[c, :3] = [255 * (c & 1), 255 * ((c >> 1) & 1), 255 * ((c >> 2) & 1)]
    return a.ravel()


def test_default_spec_equals_the_existing_restatements(oracle):
    """the CPU oracle's conversions (the reference of tests/test_gpu_rgba.py) and overlayref.rgba_to_i420a"""
    for w, h, seed in ((2, 2, 1), (16, 16, 2), (36, 18, 3)):
        rgba = _corner_frames(w, h, 7100 + seed)
        assert np.array_equal(csref.rgba_to_i420(rgba, w, h), oracle.rgba_to_i420(rgba, w, h))
        assert np.array_equal(csref.rgba_to_i420a(rgba, w, h), overlayref.rgba_to_i420a(rgba, w, h))
        yuv = np.random.default_rng(7200 + seed).integers(0, 256, csref.frame_bytes(w, h), dtype=np.uint8)
        assert np.array_equal(csref.i420_to_rgba(yuv, w, h), oracle.i420_to_rgba(yuv, w, h))
        # chroma_up does not reach the way in, chroma_down not the way out
        assert np.array_equal(csref.rgba_to_i420(rgba, w, h, csref.Spec(0, 0, 0, 1)), oracle.rgba_to_i420(rgba, w, h))
        assert np.array_equal(csref.i420_to_rgba(yuv, w, h, csref.Spec(0, 0, 1, 0)), oracle.i420_to_rgba(yuv, w, h))


def _constant(rgb, w=4, h=4):
    return np.tile(np.array([*rgb, 255], np.uint8), w * h)


@pytest.mark.parametrize('key', csref.TABLES, ids=[csref.NAMES[k] for k in csref.TABLES])
def test_grey_black_and_white(key):
    lo, hi = (0, 255) if key[1] == csref.FULL else (16, 235)
    for down in (csref.TOPLEFT, csref.AVERAGE):
        spec = csref.Spec(*key, down, 0)
        for g in range(256):
            out = csref.rgba_to_i420(_constant((g, g, g), 2, 2), 2, 2, spec)
            assert out[4] == 128 and out[5] == 128, (key, down, g)
        assert csref.rgba_to_i420(_constant((0, 0, 0), 2, 2), 2, 2, spec)[0] == lo
        assert csref.rgba_to_i420(_constant((255, 255, 255), 2, 2), 2, 2, spec)[0] == hi


@pytest.mark.parametrize('key', csref.TABLES, ids=[csref.NAMES[k] for k in csref.TABLES])
def test_constant_colour_round_trip_error(key):
    """a constant-colour frame to I420 and back differs by at most 3 per component (limited range) or 2 (full): the
    bounds of the tables over all 2^24 colours; sampled here on a lattice of step 17 (0, 17, .. 255: the corners included)
    plus a seeded random thousand. A constant frame has the same chroma in every mode"""
    bound = 2 if key[1] == csref.FULL else 3
    lat = np.arange(0, 256, 17)
    cols = np.array(list(itertools.product(lat, lat, lat)), np.uint8)
    cols = np.concatenate([cols, np.random.default_rng(7300).integers(0, 256, (1000, 3), dtype=np.uint8)])
    n = len(cols)
    # one 2 x 2n frame: every 2x2 block a constant colour; REPEAT keeps the blocks apart
    rgba = np.empty((2, 2 * n, 4), np.uint8)
    rgba[..., :3] = np.repeat(cols, 2, axis=0)[None]
    rgba[..., 3] = 255
    worst = 0
    for down in (csref.TOPLEFT, csref.AVERAGE):
        spec = csref.Spec(*key, down, csref.REPEAT)
        back = csref.i420_to_rgba(csref.rgba_to_i420(rgba.ravel(), 2 * n, 2, spec), 2 * n, 2, spec).reshape(2, 2 * n, 4)
        assert (back[..., 3] == 255).all()
        worst = max(worst, int(np.abs(back[..., :3].astype(np.int32) - rgba[..., :3].astype(np.int32)).max()))
    assert worst <= bound, (key, worst)
    # and with BILINEAR on a truly constant frame
    for rgb in ((255, 0, 0), (0, 255, 0), (0, 0, 255), (12, 200, 77)):
        spec = csref.Spec(*key, csref.AVERAGE, csref.BILINEAR)
        back = csref.i420_to_rgba(csref.rgba_to_i420(_constant(rgb, 6, 4), 6, 4, spec), 6, 4, spec).reshape(-1, 4)
        assert np.abs(back[:, :3].astype(np.int32) - np.array(rgb)).max() <= bound and (back == back[0]).all()


def test_bilinear_of_a_constant_plane_is_constant_and_weights_are_9_3_3_1():
    for v in (0, 1, 127, 128, 254, 255):
        for ch, cw in ((1, 1), (1, 5), (4, 1), (3, 4)):
            assert (csref.upsample(np.full((ch, cw), v, np.uint8), csref.BILINEAR) == v).all()
    C = np.array([[0, 16], [32, 48]], np.uint8)
    up = csref.upsample(C, csref.BILINEAR)
    assert up.shape == (4, 4)
    assert up[1][1] == (9 * 0 + 3 * 16 + 3 * 32 + 48 + 8) >> 4 and up[2][2] == (9 * 48 + 3 * 32 + 3 * 16 + 0 + 8) >> 4
    assert up[0][0] == 0 and up[3][3] == 48, 'every neighbour of a corner clamps to the corner'
    assert up[0][1] == (12 * 0 + 4 * 16 + 8) >> 4, 'the row above the first clamps to the first'
    assert np.array_equal(csref.upsample(C, csref.REPEAT), np.repeat(np.repeat(C, 2, 0), 2, 1))


def test_full_range_chroma_of_256_clamps_to_255():
    for key in ((csref.BT601, csref.FULL), (csref.BT709, csref.FULL)):
        out = csref.rgba_to_i420(_constant((0, 0, 255), 2, 2), 2, 2, csref.Spec(*key, 0, 0))
        assert out[4] == 255, 'Cb of pure blue: ((128 * 255 + 128) >> 8) + 128 = 256'
        out = csref.rgba_to_i420(_constant((255, 0, 0), 2, 2), 2, 2, csref.Spec(*key, 1, 0))
        assert out[5] == 255, 'Cr of pure red, averaged'


def test_colorspec_ok_accepts_the_16_and_refuses_the_rest(libpath):
    import h264mi
    B = h264mi.lib()
    assert len(ALL_SPECS) == 16
    for s in ALL_SPECS:
        assert h264mi.colorspec_ok(_c(s)) == 0 and csref.spec_ok(s)
    for k in range(4):
        for bad in (-1, 2, (1 << 31) - 1, -(1 << 31)):
            f = [0, 1, 1, 0]
            f[k] = bad
            assert h264mi.colorspec_ok(_c(f)) == -1, f
            assert not csref.spec_ok(csref.Spec(*f))
    assert B.h264mi_colorspec_ok(None) == -1 and h264mi.colorspec_ok(None) == -1


def test_device_calls_refuse_bad_arguments_without_a_device(libpath):
    import h264mi
    B = h264mi.lib()
    w, h = 32, 16
    fb, ab, rb = csref.frame_bytes(w, h), csref.i420a_bytes(w, h), w * h * 4
    a, b = 0x10000000, 0x20000000  # never dereferenced: every call below is refused first
    pa, pb = ctypes.c_void_p(a), ctypes.c_void_p(b)
    good = ctypes.byref(_c((1, 1, 1, 1)))
    # (the call, its RGBA argument first?, bytes a frame of the other side)
    calls = ((B.h264mi_rgba_to_i420_cs_dev, False, fb), (B.h264mi_i420_to_rgba_cs_dev, True, fb), (B.h264mi_rgba_to_i420a_cs_dev, False, ab))
    for fn, rgba_first, ob in calls:
        assert fn(None, pb, w, h, 1, good, None) == -1 and fn(pa, None, w, h, 1, good, None) == -1
        assert fn(pa, pb, w, h, 1, None, None) == -1
        for n in (0, -1):
            assert fn(pa, pb, w, h, n, good, None) == -1
        for bw, bh in ((31, 16), (32, 15), (0, 16), (32, 0), (-2, 16), (8194, 16), (32, 8194)):
            assert fn(pa, pb, bw, bh, 1, good, None) == -1, (bw, bh)
        for k in range(4):
            for bad in (-1, 2):
                f = [0, 0, 0, 0]
                f[k] = bad
                assert fn(pa, pb, w, h, 1, ctypes.byref(_c(f)), None) == -1, f
        for mis in (1, 2, 3):  # the RGBA side must be 4-byte aligned; the other side may sit anywhere
            args = (ctypes.c_void_p(a + mis), pb) if rgba_first else (pa, ctypes.c_void_p(b + mis))
            assert fn(*args, w, h, 1, good, None) == -1, mis
        # overlapping byte ranges, n frames on each side: first = the call's first argument at a, the other at a + off
        for n in (1, 3):
            first_b, second_b = (n * rb, n * ob) if rgba_first else (n * ob, n * rb)
            for off in (0, 4 * ((first_b - 1) // 4), -4 * ((second_b - 1) // 4)):
                assert fn(pa, ctypes.c_void_p(a + off), w, h, n, good, None) == -1, (n, off)
    spec = _c((1, 0, 1, 0))
    assert B.h264mi_enc_set_colorspec(None, ctypes.byref(spec)) == -1 and B.h264mi_enc_set_colorspec(None, None) == -1
    assert B.h264mi_enc_colorspec(None, ctypes.byref(spec)) == -1
    assert B.h264mi_dec_set_output_colorspec(None, ctypes.byref(spec)) == -1 and B.h264mi_dec_set_output_colorspec(None, None) == -1
    assert B.h264mi_dec_output_colorspec(None, ctypes.byref(spec)) == -1
    assert (spec.matrix, spec.range, spec.chroma_down, spec.chroma_up) == (1, 0, 1, 0), 'a refused call writes nothing'
