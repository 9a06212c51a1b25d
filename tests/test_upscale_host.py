"""CPU: the I420 upscaler exists at every layer -- declared in include/h264mi.h, exported by the library, bound in
Python --, h264mi_speaker_cells equals its plain-integer restatement, tests/upscaleref.py (the reference of the GPU
tests) has the properties the definition promises, and the device calls refuse bad arguments before touching a device."""
import ctypes

import numpy as np
import pytest

import composeref
import scaleref
import upscaleref
from test_capi_exports import declared_functions
from test_compose_host import SIZES

NEW = {'h264mi_i420_upscale_dev': 9, 'h264mi_i420_compose_any_dev': 12, 'h264mi_speaker_cells': 8, 'h264mi_enc_encode_composed_any': 11}


def test_header_declares_library_exports_python_binds(libpath):
    names = declared_functions()
    L = ctypes.CDLL(libpath)
    import h264mi
    B = h264mi.lib()
    for n, nargs in NEW.items():
        assert n in names, n
        assert hasattr(L, n), n
        assert getattr(B, n).argtypes is not None and len(getattr(B, n).argtypes) == nargs, n
    assert (h264mi.FILTER_BILINEAR, h264mi.FILTER_BICUBIC) == (0, 1) == (upscaleref.BILINEAR, upscaleref.BICUBIC)
    assert callable(h264mi.i420_upscale) and callable(h264mi.i420_compose_any) and callable(h264mi.speaker_cells)
    assert callable(h264mi.BatchEncoder.encode_composed_any)


def _mixed(c, src_w, src_h):
    return (c.dw > src_w and c.dh < src_h) or (c.dw < src_w and c.dh > src_h)


@pytest.mark.parametrize('src_w,src_h,cw,ch', SIZES, ids=[f'{a}x{b}-on-{c}x{d}' for a, b, c, d in SIZES])
def test_speaker_cells_equals_the_restatement(libpath, src_w, src_h, cw, ch):
    import h264mi
    fn = h264mi.lib().h264mi_speaker_cells
    for n in range(1, 18):
        for speaker in range(n):
            want = upscaleref.speaker_cells(n, speaker, src_w, src_h, cw, ch)
            out = (h264mi.Cell * n)()
            if want is None:
                assert fn(out, n, n, speaker, src_w, src_h, cw, ch) == -1, (n, speaker)
                continue
            assert fn(out, n, n, speaker, src_w, src_h, cw, ch) == n, (n, speaker)
            assert [composeref.as_tuple(c) for c in out] == [tuple(c) for c in want], (n, speaker)
            for k, c in enumerate(want):  # source k's cell: inside the canvas, even, the whole source, never mixed
                assert c.src == k and c.canvas == 0 and (c.sx, c.sy, c.sw, c.sh) == (0, 0, src_w, src_h)
                assert all(v % 2 == 0 for v in c[2:]) and 0 <= c.dx and c.dx + c.dw <= cw and 0 <= c.dy and c.dy + c.dh <= ch
                assert c.dw >= 2 and c.dh >= 2 and upscaleref.kind(c) is not None and not _mixed(c, src_w, src_h)
            for i, a in enumerate(want):
                for b in want[:i]:
                    assert not (a.dx < b.dx + b.dw and b.dx < a.dx + a.dw and a.dy < b.dy + b.dh and b.dy < a.dy + a.dh)
        if upscaleref.speaker_cells(n, 0, src_w, src_h, cw, ch) is None:
            with pytest.raises(ValueError):
                h264mi.speaker_cells(n, 0, src_w, src_h, cw, ch)
        else:
            assert [composeref.as_tuple(c) for c in h264mi.speaker_cells(n, n - 1, src_w, src_h, cw, ch)] == \
                   [tuple(c) for c in upscaleref.speaker_cells(n, n - 1, src_w, src_h, cw, ch)]


def test_speaker_rule_never_mixes_axes():
    """dw > src_w implies dh >= src_h and dw < src_w implies dh < src_h, over shapes from 1:8 to 8:1 and canvases both
    smaller and larger than the source"""
    sides = (2, 6, 16, 18, 34, 36, 50, 64, 144, 176, 360, 640, 720, 1080, 1280, 1920, 4096)
    canv = (8, 16, 22, 48, 50, 112, 288, 360, 720, 1080, 1280, 2160, 8192)
    seen = set()
    for src_w in sides:
        for src_h in sides:
            for cw in canv:
                for ch in canv:
                    for n in (1, 2, 3, 9):
                        cells = upscaleref.speaker_cells(n, n // 2, src_w, src_h, cw, ch)
                        for c in cells or ():
                            assert not (c.dw > src_w and c.dh < src_h), (c, cw, ch)
                            assert not (c.dw < src_w and c.dh >= src_h), (c, cw, ch)
                            seen.add(upscaleref.kind(c))
    assert seen == {0, 1}


def test_speaker_examples_by_hand(libpath):
    import h264mi
    t = lambda cells: [composeref.as_tuple(c) for c in cells]
    # strip 2 * (720 // 8) = 180: the speaker's slot 1280x540 holds 960x540 at x = 160; two strip slots of 640x180 hold 320x180
    assert t(h264mi.speaker_cells(3, 1, 640, 360, 1280, 720)) == [(0, 0, 0, 0, 640, 360, 160, 540, 320, 180),
                                                                   (1, 0, 0, 0, 640, 360, 160, 0, 960, 540),
                                                                   (2, 0, 0, 0, 640, 360, 800, 540, 320, 180)]
    # one source: the whole canvas, enlarged 2x
    assert t(h264mi.speaker_cells(1, 0, 640, 360, 1280, 720)) == [(0, 0, 0, 0, 640, 360, 0, 0, 1280, 720)]
    # 4:3 on 16:9, one source: pillar-boxed, 960x720 centred
    assert t(h264mi.speaker_cells(1, 0, 640, 480, 1280, 720)) == [(0, 0, 0, 0, 640, 480, 160, 0, 960, 720)]
    # 3 sources of 32x24 on 64x48: strip 12, speaker slot 64x36 holds 48x36 at x = 8; strip slots 32x12 hold 16x12 at +8
    assert t(h264mi.speaker_cells(3, 0, 32, 24, 64, 48)) == [(0, 0, 0, 0, 32, 24, 8, 0, 48, 36), (1, 0, 0, 0, 32, 24, 8, 36, 16, 12),
                                                              (2, 0, 0, 0, 32, 24, 40, 36, 16, 12)]
    # 9 sources: eight strip slots of 160x180, pictures 160x90 centred 44 rows down (2 * ((180 - 90) // 4))
    cells = t(h264mi.speaker_cells(9, 0, 640, 360, 1280, 720))
    assert cells[0] == (0, 0, 0, 0, 640, 360, 160, 0, 960, 540)
    assert cells[1:] == [(k, 0, 0, 0, 640, 360, 160 * (k - 1), 540 + 44, 160, 90) for k in range(1, 9)]


def test_speaker_refusals(libpath):
    import h264mi
    fn = h264mi.lib().h264mi_speaker_cells
    out = (h264mi.Cell * 16)()
    assert fn(out, 16, 9, 0, 640, 360, 1280, 720) == 9
    assert fn(None, 16, 9, 0, 640, 360, 1280, 720) == -1
    assert fn(out, 8, 9, 0, 640, 360, 1280, 720) == -1  # cap < n
    assert fn(out, 16, 0, 0, 640, 360, 1280, 720) == -1 and fn(out, 16, -1, 0, 640, 360, 1280, 720) == -1
    assert fn(out, 16, 9, 9, 640, 360, 1280, 720) == -1 and fn(out, 16, 9, -1, 640, 360, 1280, 720) == -1  # speaker
    assert fn(out, 16, 1, 1, 640, 360, 1280, 720) == -1
    assert fn(out, 16, 4097, 0, 640, 360, 1280, 720) == -1
    for bad in ((639, 360, 1280, 720), (640, 359, 1280, 720), (640, 360, 1281, 720), (640, 360, 1280, 721), (0, 360, 1280, 720),
                (640, 0, 1280, 720), (640, 360, 0, 720), (640, 360, 1280, -2), (4098, 360, 1280, 720), (640, 4098, 1280, 720),
                (640, 360, 8194, 720), (640, 360, 1280, 8194)):
        assert fn(out, 16, 4, 0, *bad) == -1, bad
    assert fn(out, 16, 2, 0, 64, 36, 48, 6) == -1  # ch // 8 == 0: no strip, a cell below 2
    assert upscaleref.speaker_cells(2, 0, 64, 36, 48, 6) is None
    with pytest.raises(ValueError):
        h264mi.speaker_cells(0, 0, 64, 36, 48, 48)


# ---- the reference's properties

def _frames(w, h, n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, scaleref.frame_bytes(w, h)), dtype=np.uint8)


@pytest.mark.parametrize('filt', (0, 1))
def test_reference_weights_sum_to_8192_in_every_phase(filt):
    w = upscaleref.weights(np.arange(16), filt)
    assert w.shape == (16, 4) and (w.sum(axis=1) == 8192).all()
    assert w[0].tolist() == [0, 8192, 0, 0]
    if filt == upscaleref.BICUBIC:  # Catmull-Rom at one half: -1/16, 9/16, 9/16, -1/16
        assert w[8].tolist() == [-512, 4608, 4608, -512]
        assert [upscaleref.weights(f, filt)[::-1].tolist() for f in range(1, 16)] == [w[16 - f].tolist() for f in range(1, 16)]  # symmetric
    else:
        assert w[4].tolist() == [0, 6144, 2048, 0]


def test_reference_phase_is_a_floor_division():
    """P for negative N equals Python's floor (C truncation would give one more)"""
    for p, q in ((2, 128), (16, 32), (18, 25), (9, 11), (360, 720), (4096, 8192), (2, 8192), (4096, 4098)):
        P = upscaleref.phases(p, q)
        want = [(16 * ((2 * o + 1) * p - q) + q) // (2 * q) for o in range(q)]
        assert P.tolist() == want
        assert P[0] == (16 * (p - q) + q) // (2 * q) and P[0] >= -8 and (P >> 4).min() >= -1 and (P >> 4).max() <= p - 1
        assert (np.diff(P) <= 16).all()  # i advances by at most one from an output sample to the next
    P = upscaleref.phases(16, 32)  # N = -16: (16 * -16 + 32) // 64 = -4 (truncation: -3); i = -1, f = 12
    assert P[0] == -4 and P[0] >> 4 == -1 and P[0] & 15 == 12 and int(-224 / 64) == -3
    assert upscaleref.phases(7, 7).tolist() == [16 * o for o in range(7)]  # p == q: f = 0, i = o


@pytest.mark.parametrize('filt', (0, 1))
def test_reference_identity_at_equal_sizes(filt):
    for w, h in ((2, 2), (36, 18), (64, 48)):
        f = _frames(w, h, 1, 31)[0]
        assert np.array_equal(upscaleref.up_frame(f, w, h, w, h, filt), f)
    crop = _frames(34, 18, 1, 32)[0][:34 * 18].reshape(18, 34)
    out = upscaleref.up_plane(crop, 36, 18, filt)  # one axis equal: every column is filtered vertically with f = 0
    assert out.shape == (18, 36) and np.array_equal(out[:, 0], crop[:, 0]) and np.array_equal(out[:, -1], crop[:, -1])


@pytest.mark.parametrize('filt', (0, 1))
def test_reference_keeps_constants(filt):
    for v in (0, 1, 16, 127, 128, 254, 255):
        out = upscaleref.up_plane(np.full((5, 7), v, np.uint8), 19, 12, filt)
        assert out.shape == (12, 19) and (out == v).all(), v


def test_reference_bicubic_checkerboard_overshoots_before_the_clamp():
    yy, xx = np.mgrid[0:8, 0:8]
    board = (((xx // 2 + yy // 2) & 1) * 255).astype(np.uint8)  # 2x2 squares of 0 and 255
    raw = upscaleref.up_plane(board, 24, 24, upscaleref.BICUBIC, clamp=False)
    assert raw.min() < 0 and raw.max() > 255, (raw.min(), raw.max())
    out = upscaleref.up_plane(board, 24, 24, upscaleref.BICUBIC)
    assert out.dtype == np.uint8 and np.array_equal(out, np.clip(raw, 0, 255))
    lin = upscaleref.up_plane(board, 24, 24, upscaleref.BILINEAR, clamp=False)
    assert lin.min() >= 0 and lin.max() <= 255  # bilinear weights are non-negative: no overshoot


def test_reference_bilinear_by_hand():
    """2 -> 4 samples: phases -4, 4, 12, 20 -> (i, f) = (-1, 12), (0, 4), (0, 12), (1, 4); clamped taps"""
    crop = np.array([[0, 160]], np.uint8)
    out = upscaleref.up_plane(crop, 4, 1, upscaleref.BILINEAR)
    assert out.tolist() == [[0, 40, 120, 160]]


def test_reference_compose_any_pastes_both_kinds_and_nothing_else():
    sw, sh, cw, ch = 32, 24, 64, 48
    src, canvas = _frames(sw, sh, 2, 33), _frames(cw, ch, 2, 34)
    big = composeref.C(1, 0, 4, 2, 16, 12, 8, 4, 40, 30)      # enlarging, a crop strictly inside the source
    small = composeref.C(0, 0, 0, 0, 32, 24, 48, 36, 16, 12)  # shrinking
    same = composeref.C(0, 1, 2, 2, 8, 8, 10, 10, 8, 8)       # equal sizes: compose's copy
    out = upscaleref.compose_any(canvas, cw, ch, src, sw, sh, [big, small, same], upscaleref.BICUBIC)
    only_small = composeref.compose(canvas, cw, ch, src, sw, sh, [small, same])
    touched = np.zeros(scaleref.frame_bytes(cw, ch), np.uint8)
    for p, (o, s, t) in enumerate(zip(scaleref.planes(out[0], cw, ch), scaleref.planes(src[1], sw, sh), scaleref.planes(touched, cw, ch))):
        k = 1 if p else 0
        rect = (slice(4 >> k, (4 + 30) >> k), slice(8 >> k, (8 + 40) >> k))
        assert np.array_equal(o[rect], upscaleref.up_plane(s[2 >> k:(2 + 12) >> k, 4 >> k:(4 + 16) >> k], 40 >> k, 30 >> k, upscaleref.BICUBIC))
        t[rect] = 1
    assert touched.sum() == 40 * 30 * 3 // 2 and np.array_equal(out[0][touched == 0], only_small[0][touched == 0]) and np.array_equal(out[1], only_small[1])
    with pytest.raises(AssertionError):
        upscaleref.compose_any(canvas, cw, ch, src, sw, sh, [composeref.C(0, 0, 0, 0, 16, 12, 0, 0, 18, 10)], 1)  # mixed


# ---- refusals, before a device is touched: the pointers are never dereferenced

def test_upscale_dev_refuses_bad_arguments_without_a_device(libpath):
    import h264mi
    fn = h264mi.lib().h264mi_i420_upscale_dev
    d, s = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x20000000)
    assert fn(None, 64, 48, s, 32, 24, 1, 1, None) == -1
    assert fn(d, 64, 48, None, 32, 24, 1, 1, None) == -1
    for dw, dh, sw, sh, n, filt in ((64, 48, 32, 24, 0, 1), (64, 48, 32, 24, -1, 1),                          # n
                                    (63, 48, 32, 24, 1, 1), (64, 47, 32, 24, 1, 1), (64, 48, 31, 24, 1, 1), (64, 48, 32, 23, 1, 1),  # odd
                                    (30, 48, 32, 24, 1, 1), (64, 22, 32, 24, 1, 1),                            # shrinking an axis
                                    (64, 48, 0, 24, 1, 1), (64, 48, 32, 0, 1, 1), (64, 48, -2, 24, 1, 1),      # source out of range
                                    (8192, 48, 4098, 24, 1, 1), (64, 8192, 32, 4098, 1, 1),
                                    (8194, 48, 32, 24, 1, 1), (64, 8194, 32, 24, 1, 1),                        # destination out of range
                                    (64, 48, 32, 24, 1, 2), (64, 48, 32, 24, 1, -1)):                          # unknown filter
        assert fn(d, dw, dh, s, sw, sh, n, filt, None) == -1, (dw, dh, sw, sh, n, filt)
    # overlapping byte ranges: a 32x24 frame is 1152 bytes, a 64x48 frame 4608
    base = 0x10000000
    for off in (0, 1, 1151, -1, -4607):
        assert fn(ctypes.c_void_p(base + off), 64, 48, ctypes.c_void_p(base), 32, 24, 1, 0, None) == -1, off
    assert fn(ctypes.c_void_p(base + 3 * 1152 - 1), 64, 48, ctypes.c_void_p(base), 32, 24, 3, 0, None) == -1  # n frames count
    assert fn(ctypes.c_void_p(base - 3 * 4608 + 1), 64, 48, ctypes.c_void_p(base), 32, 24, 3, 0, None) == -1


def _cells(*tuples):
    import h264mi
    return (h264mi.Cell * len(tuples))(*[h264mi.Cell(*t) for t in tuples])


UP_CELL = (0, 0, 0, 0, 16, 16, 0, 0, 32, 32)
DOWN_CELL = (0, 0, 0, 0, 32, 32, 32, 32, 16, 16)
# (cw, ch, ncanvas, src_w, src_h, nsrc, cells, filter) that h264mi_i420_compose_any_dev must refuse
BAD = [(64, 64, 0, 32, 32, 1, [UP_CELL], 1), (64, 64, 1, 32, 32, 0, [UP_CELL], 1), (64, 64, 1, 32, 32, 1, [], 1),          # counts
       (63, 64, 1, 32, 32, 1, [UP_CELL], 1), (64, 63, 1, 32, 32, 1, [UP_CELL], 1), (64, 64, 1, 33, 32, 1, [UP_CELL], 1),     # odd sizes
       (64, 64, 1, 32, 33, 1, [UP_CELL], 1),
       (64, 64, 1, 4098, 32, 1, [UP_CELL], 1), (64, 64, 1, 32, 4098, 1, [UP_CELL], 1),                                        # sides too large
       (8194, 64, 1, 32, 32, 1, [UP_CELL], 1), (64, 8194, 1, 32, 32, 1, [UP_CELL], 1),
       (64, 64, 1, 32, 32, 1, [UP_CELL], 2), (64, 64, 1, 32, 32, 1, [UP_CELL], -1), (64, 64, 1, 32, 32, 1, [DOWN_CELL], 2),   # unknown filter
       (64, 64, 1, 32, 32, 1, [(1, 0, 0, 0, 16, 16, 0, 0, 32, 32)], 1), (64, 64, 1, 32, 32, 1, [(0, 1, 0, 0, 16, 16, 0, 0, 32, 32)], 1),  # src, canvas
       (64, 64, 1, 32, 32, 1, [(-1, 0, 0, 0, 16, 16, 0, 0, 32, 32)], 1), (64, 64, 1, 32, 32, 1, [(0, -1, 0, 0, 16, 16, 0, 0, 32, 32)], 1),
       (64, 64, 1, 32, 32, 1, [(0, 0, 18, 0, 16, 16, 0, 0, 32, 32)], 1), (64, 64, 1, 32, 32, 1, [(0, 0, 0, 18, 16, 16, 0, 0, 32, 32)], 1),   # crop
       (64, 64, 1, 32, 32, 1, [(0, 0, -2, 0, 16, 16, 0, 0, 32, 32)], 1), (64, 64, 1, 32, 32, 1, [(0, 0, 2147483646, 0, 4, 4, 0, 0, 8, 8)], 1),
       (64, 64, 1, 32, 32, 1, [(0, 0, 0, 0, 0, 16, 0, 0, 32, 32)], 1), (64, 64, 1, 32, 32, 1, [(0, 0, 0, 0, 16, -2, 0, 0, 32, 32)], 1),
       (64, 64, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, 34, 0, 32, 32)], 1), (64, 64, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, 0, 34, 32, 32)], 1),   # rectangle
       (64, 64, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, -2, 0, 32, 32)], 1), (64, 64, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, 2147483646, 0, 32, 32)], 1),
       (64, 64, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, 0, 0, 66, 32)], 1), (64, 64, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, 0, 0, 32, 2147483646)], 1),
       (64, 64, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, 0, 0, 0, 32)], 1), (64, 64, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, 0, 0, 32, -2)], 1),       # below 2
       (64, 64, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, 0, 0, 18, 14)], 1), (64, 64, 1, 32, 32, 1, [(0, 0, 0, 0, 16, 16, 0, 0, 14, 18)], 0),      # mixed
       (64, 64, 1, 32, 32, 1, [UP_CELL, DOWN_CELL, (0, 0, 0, 0, 16, 16, 0, 32, 32, 8)], 1),
       (64, 64, 1, 32, 32, 1, [UP_CELL, (0, 0, 0, 0, 32, 32, 30, 30, 16, 16)], 1),                                                            # cells of two kinds sharing a sample
       (64, 64, 1, 32, 32, 1, [(0, 0, 0, 0, 32, 32, 30, 30, 16, 16), UP_CELL], 1),
       (64, 64, 1, 32, 32, 1, [UP_CELL, (0, 0, 0, 0, 16, 16, 30, 30, 34, 34)], 1),                                                            # two enlarging
       (64, 64, 2, 32, 32, 1, [(0, 1, 0, 0, 16, 16, 0, 0, 32, 32), UP_CELL, (0, 1, 0, 0, 32, 32, 0, 30, 16, 16)], 1)]
BAD += [(64, 64, 1, 32, 32, 1, [tuple(v + (1 if i == k else 0) for i, v in enumerate((0, 0, 2, 2, 8, 8, 4, 4, 16, 16)))], 1) for k in range(2, 10)]  # an odd field


def test_compose_any_dev_refuses_bad_arguments_without_a_device(libpath):
    import h264mi
    fn = h264mi.lib().h264mi_i420_compose_any_dev
    d, s = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x20000000)
    one = _cells(UP_CELL)
    assert fn(None, 64, 64, 1, s, 32, 32, 1, one, 1, 1, None) == -1
    assert fn(d, 64, 64, 1, None, 32, 32, 1, one, 1, 1, None) == -1
    assert fn(d, 64, 64, 1, s, 32, 32, 1, None, 1, 1, None) == -1
    for cw, ch, ncanvas, sw, sh, nsrc, cells, filt in BAD:
        arr = _cells(*cells) if cells else one
        assert fn(d, cw, ch, ncanvas, s, sw, sh, nsrc, arr, len(cells), filt, None) == -1, (cw, ch, ncanvas, sw, sh, nsrc, cells, filt)
    many = _cells(*[(0, 0, 0, 0, 2, 2, 4 * (k % 64), 4 * (k // 64), 4, 4) for k in range(4097)])  # disjoint enlarging cells, one too many
    assert fn(d, 256, 512, 1, s, 32, 32, 1, many, 4097, 1, None) == -1
    # overlapping byte ranges: a 32x32 frame is 1536 bytes, a 64x64 canvas 6144
    base = 0x10000000
    for off in (0, 1, 1535, -1, -6143):
        assert fn(ctypes.c_void_p(base + off), 64, 64, 1, ctypes.c_void_p(base), 32, 32, 1, one, 1, 1, None) == -1, off
    assert fn(ctypes.c_void_p(base + 3 * 1536 - 1), 64, 64, 1, ctypes.c_void_p(base), 32, 32, 3, one, 1, 1, None) == -1
    assert fn(ctypes.c_void_p(base - 2 * 6144 + 1), 64, 64, 2, ctypes.c_void_p(base), 32, 32, 1, one, 1, 1, None) == -1


def test_compose_dev_still_refuses_an_enlarging_cell(libpath):
    import h264mi
    d, s = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x20000000)
    assert h264mi.lib().h264mi_i420_compose_dev(d, 64, 64, 1, s, 32, 32, 1, _cells(UP_CELL), 1, None) == -1
    assert h264mi.lib().h264mi_i420_scale_dev(d, 64, 64, s, 32, 32, 1, None) == -1


def test_encode_composed_any_refuses_a_null_encoder(libpath):
    import h264mi
    one = _cells(UP_CELL)
    assert h264mi.lib().h264mi_enc_encode_composed_any(None, ctypes.c_void_p(0x20000000), 32, 32, 1, one, 1, 1, 16, 128, 128) == -1
