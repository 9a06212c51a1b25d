"""CPU: the deeper and wider pixel layouts (ids 16..24) exist at every layer, the library's tight layouts, spans, layout
rule (the unit rule included) and h264mi_pixopt_ok equal tests/pixdeepref.py on directed and seeded random layouts, ids
5..15 and 25 stay refused, and the reference's own algebra holds: I420 -> format -> I420 is the identity under every
depth rule."""
import ctypes
import os
import re

import numpy as np
import pytest

import pixdeepref as R
import pixref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX, INT64_MAX = (1 << 31) - 1, (1 << 63) - 1
SIZES = ((2, 2), (6, 2), (16, 16), (36, 18), (50, 2), (8192, 2))
IDS = [R.NAMES[p] for p in R.ALL]


def _c(L):
    import h264mi
    return h264mi.PixLayout(L.pix, L.pitch, L.offset, L.frame_stride)


def test_constants_symbols_and_bindings(libpath):
    import h264mi
    src = open(os.path.join(ROOT, 'include', 'h264mi.h')).read()
    for pix in R.ALL:
        m = re.search(r'^#define H264MI_PIX_%s (\d+)' % R.NAMES[pix], src, flags=re.M)
        assert m and int(m.group(1)) == pix == getattr(h264mi, 'PIX_' + R.NAMES[pix])
    for k, name in enumerate(('ROUND', 'DITHER', 'TRUNC')):
        m = re.search(r'^#define H264MI_DEPTH_%s (\d+)' % name, src, flags=re.M)
        assert m and int(m.group(1)) == k == getattr(h264mi, 'DEPTH_' + name) == getattr(R, name)
    B = h264mi.lib()
    for n, nargs in (('h264mi_pix_unit', 1), ('h264mi_pixopt_ok', 1), ('h264mi_pix_to_i420_opt_dev', 8), ('h264mi_enc_set_pixopt', 2),
                     ('h264mi_enc_pixopt', 2)):
        assert len(getattr(B, n).argtypes) == nargs, n
    assert ctypes.sizeof(h264mi.PixOpt) == 16
    assert callable(h264mi.BatchEncoder.set_pixopt) and callable(h264mi.BatchEncoder.pixopt)
    for pix in list(range(-1, 26)) + [INT32_MAX]:
        assert h264mi.pix_unit(pix) == R.unit(pix), pix
    assert [h264mi.pix_unit(p) for p in (0, 4, 16, 19, 20, 23, 24, 5, 15, 25)] == [1, 1, 1, 1, 2, 2, 4, -1, -1, -1]


@pytest.mark.parametrize('pix', R.ALL, ids=IDS)
def test_tight_layouts_and_spans_equal_the_reference(libpath, pix):
    import h264mi
    for w, h in SIZES:
        got, want = h264mi.pix_layout_tight(pix, w, h), R.tight(pix, w, h)
        assert (got.pix, list(got.pitch), list(got.offset), got.frame_stride) == (want.pix, want.pitch, want.offset, want.frame_stride), (w, h)
        assert h264mi.pix_span(got, w, h) == R.span(want, w, h)
        assert h264mi.pix_layout_ok(got, w, h) == 0 and R.layout_ok(want, w, h)
        if pix == R.V210:
            assert got.pitch[0] == 128 * ((w + 47) // 48) and got.frame_stride == h * got.pitch[0]
            assert R.span(want, w, h) == (h - 1) * got.pitch[0] + 16 * ((w + 5) // 6)
        else:
            bits = {R.I422: 16, R.I444: 24, R.NV16: 16, R.Y800: 8, R.P010: 24, R.I010: 24, R.P210: 32, R.I210: 32}[pix]
            assert want.frame_stride == R.span(want, w, h) == w * h * bits // 8


def _agree(L, w, h):
    import h264mi
    c = _c(L)
    assert h264mi.pix_span(c, w, h) == R.span(L, w, h), (L, w, h)
    assert h264mi.pix_layout_ok(c, w, h) == (0 if R.layout_ok(L, w, h) else -1), (L, w, h)
    return R.layout_ok(L, w, h)


def _directed():
    """(layout, w, h, expected) with the one rule each breaks"""
    w, h = 36, 18
    out = []
    for pix in R.ALL:
        u = R.unit(pix)
        np_ = len(R.planes(pix, w, h))
        rb0 = R.planes(pix, w, h)[0][0]
        t = R.tight(pix, w, h)
        out.append((t, w, h, True))
        a = R.tight(pix, w, h); a.pitch[0] = rb0 - u  # a pitch one unit below the row bytes
        out.append((a, w, h, False))
        a = R.tight(pix, w, h); a.frame_stride = R.span(a, w, h) - u  # a frame_stride one unit below the span
        out.append((a, w, h, False))
        a = R.tight(pix, w, h); a.frame_stride += 8
        out.append((a, w, h, True))
        if np_ > 1:
            a = R.tight(pix, w, h); a.offset[1] -= u  # planes that overlap by one unit
            out.append((a, w, h, False))
            a = R.tight(pix, w, h); a.offset[0] = a.frame_stride; a.frame_stride += 4 * w * h  # another order, touching
            out.append((a, w, h, True))
        if np_ < 3:
            a = R.tight(pix, w, h); a.pitch[2] = 4  # a nonzero unused entry
            out.append((a, w, h, False))
            a = R.tight(pix, w, h); a.offset[2] = 4
            out.append((a, w, h, False))
        a = R.tight(pix, w, h); a.offset[0] = -4  # a negative offset
        out.append((a, w, h, False))
        out.append((t, w + 1, h, False))  # an odd w
        out.append((t, w, h + 1, False))
        out.append((R.tight(pix, 8192, 16), 8194, 16, False))
        out.append((R.tight(pix, 16, 16), 0, 16, False))
        a = R.tight(pix, w, h); a.pitch[0] = 65536; a.offset = [o + 70000 * h if 0 < k < np_ else o for k, o in enumerate(a.offset)]
        a.frame_stride = a.offset[np_ - 1] + 70000 * h  # the largest pitch
        out.append((a, w, h, True))
        a = R.tight(pix, w, h); a.pitch[0] = 65536 + 4; a.frame_stride = INT64_MAX - 3
        out.append((a, w, h, False))
        a = R.tight(pix, w, h); a.frame_stride = INT64_MAX - 3  # a multiple of 4
        out.append((a, w, h, True))
        a = R.tight(pix, w, h); a.offset[np_ - 1] = INT64_MAX - 3; a.frame_stride = INT64_MAX - 3  # the span leaves int64
        out.append((a, w, h, False))
        # the unit rule: a pitch, an offset and a frame_stride that are one byte (16-bit formats, V210) or two bytes (V210) off
        for d in ([1] if u == 2 else [1, 2] if u == 4 else []):
            a = R.tight(pix, w, h); a.pitch[0] += d; a.offset = [o + 128 * k if k < np_ else 0 for k, o in enumerate(a.offset)]; a.frame_stride += 4096
            out.append((a, w, h, False))
            a = R.tight(pix, w, h); a.offset[0] += d; a.offset = [o + 128 * k if k < np_ else 0 for k, o in enumerate(a.offset)]; a.frame_stride += 4096
            out.append((a, w, h, False))
            a = R.tight(pix, w, h); a.frame_stride += d
            out.append((a, w, h, False))
            a = R.tight(pix, w, h); a.pitch[0] += 4; a.offset = [o + 128 * k if k < np_ else 0 for k, o in enumerate(a.offset)]; a.frame_stride += 4096
            out.append((a, w, h, True))  # ... and the same moves by a whole unit are fine
        if u == 1:
            a = R.tight(pix, w, h); a.pitch[0] += 1; a.offset = [o + 63 * k if k < np_ else 0 for k, o in enumerate(a.offset)]; a.frame_stride += 4097
            out.append((a, w, h, True))  # no unit rule for the 8-bit formats
    for bad in list(range(5, 16)) + [25, -1, INT32_MAX]:  # no such format
        out.append((pixref.Layout(bad, [64], [0], 1 << 20), 16, 16, False))
    return out


def test_layout_ok_on_directed_layouts(libpath):
    seen = {True: 0, False: 0}
    for L, w, h, want in _directed():
        assert _agree(L, w, h) == want, (L, w, h)
        seen[want] += 1
    assert seen[True] > 30 and seen[False] > 100


def test_unassigned_ids_stay_refused(libpath):
    import h264mi
    B = h264mi.lib()
    out = h264mi.PixLayout(7, (7, 7, 7), (7, 7, 7), 7)
    for bad in list(range(5, 16)) + [25]:
        assert B.h264mi_pix_layout_tight(ctypes.byref(out), bad, 16, 16) == -1, bad
        with pytest.raises(ValueError):
            h264mi.pix_layout_tight(bad, 16, 16)
        L = h264mi.PixLayout(bad, (64, 0, 0), (0, 0, 0), 1 << 20)
        assert h264mi.pix_span(L, 16, 16) == -1 and h264mi.pix_layout_ok(L, 16, 16) == -1 and h264mi.pix_unit(bad) == -1
        assert R.planes(bad, 16, 16) is None and R.unit(bad) == -1
    assert (out.pix, list(out.pitch), list(out.offset), out.frame_stride) == (7, [7] * 3, [7] * 3, 7), 'a refused call writes nothing'


def test_layout_ok_on_random_layouts(libpath):
    """seeded: half the layouts start good (planes in a random order with random gaps and pitches, all in units) and get
    at most one field disturbed by a few bytes, the rest have every field random with the extremes mixed in"""
    rng = np.random.default_rng(7100)
    extremes = [0, 1, -1, 2, INT32_MAX, -INT32_MAX - 1, 65536, 65537, 65534]
    extremes64 = extremes + [INT64_MAX, -INT64_MAX - 1, INT64_MAX - 1, INT64_MAX - 3, 1 << 31, 1 << 32]
    good = 0
    for it in range(4000):
        pix = int(rng.integers(16, 25))
        w, h = 2 * int(rng.integers(1, 40)), 2 * int(rng.integers(1, 40))
        u = R.unit(pix)
        if it % 2 == 0:
            pl = R.planes(pix, w, h)
            pitch = [rb + u * int(rng.integers(0, 3)) * int(rng.integers(0, 20)) for rb, _ in pl]
            offset, at = [0] * len(pl), u * int(rng.integers(0, 3)) * int(rng.integers(0, 50))
            for p in rng.permutation(len(pl)):
                offset[p] = at
                at += (pl[p][1] - 1) * pitch[p] + pl[p][0] + u * int(rng.integers(0, 2)) * int(rng.integers(0, 25))
            L = pixref.Layout(pix, pitch, offset, at + u * int(rng.integers(0, 2)) * int(rng.integers(0, 25)))
            k = int(rng.integers(0, 14))  # disturb one field, or (k >= 8) none
            d = int(rng.integers(-9, 10))
            if k < 3:
                L.pitch[k] += d
            elif k < 6:
                L.offset[k - 3] += d
            elif k == 6:
                L.frame_stride += d
            elif k == 7:
                w += int(rng.integers(-1, 2))
        else:
            def f32():
                return int(rng.choice(extremes)) if rng.integers(0, 3) == 0 else int(rng.integers(-10, 3000))

            def f64():
                return int(extremes64[int(rng.integers(0, len(extremes64)))]) if rng.integers(0, 3) == 0 else int(rng.integers(-10, 100000))
            L = pixref.Layout(int(rng.integers(15, 26)), [f32() for _ in range(3)], [f64() for _ in range(3)], f64())
            if rng.integers(0, 4) == 0:
                w = int(rng.choice([0, -2, 8192, 8194, 3]))
        good += _agree(L, w, h)
    assert 800 < good < 3200, f'{good} good layouts of 4000: the sample shows little'


def test_pixopt_ok(libpath):
    import h264mi
    for depth in (0, 1, 2):
        assert h264mi.pixopt_ok(h264mi.PixOpt(depth)) == 0
    for depth in (3, -1, INT32_MAX):
        assert h264mi.pixopt_ok(h264mi.PixOpt(depth)) == -1
    for k in range(3):
        r = [0, 0, 0]
        r[k] = 1
        assert h264mi.pixopt_ok(h264mi.PixOpt(0, r)) == -1
        r[k] = -INT32_MAX - 1
        assert h264mi.pixopt_ok(h264mi.PixOpt(2, r)) == -1
    assert h264mi.pixopt_ok(None) == -1
    B = h264mi.lib()
    assert B.h264mi_enc_set_pixopt(None, None) == -1 and B.h264mi_enc_pixopt(None, ctypes.byref(h264mi.PixOpt())) == -1


def _gapped(pix, w, h):
    """a layout with pitch padding, gaps and the planes in reverse order, all in units"""
    pl = R.planes(pix, w, h)
    pitch = [rb + 12 for rb, _ in pl]
    offset, at = [0] * len(pl), 8
    for p in reversed(range(len(pl))):
        offset[p] = at
        at += pl[p][1] * pitch[p] + 4
    return pixref.Layout(pix, pitch, offset, at + 8)


@pytest.mark.parametrize('pix', R.ALL, ids=IDS)
def test_reference_i420_to_format_and_back_is_the_identity(pix):
    rng = np.random.default_rng(7200 + pix)
    for w, h in ((2, 2), (6, 2), (14, 6), (16, 4), (36, 18)):
        fr = rng.integers(0, 256, pixref.frame_bytes(w, h), dtype=np.uint8)
        fr[:3] = (255, 0, 254)
        for lay in (R.tight(pix, w, h), _gapped(pix, w, h)):
            assert R.layout_ok(lay, w, h)
            buf = np.full(R.span(lay, w, h) + 9, 0xA5, np.uint8)
            R.pack(fr, lay, w, h, buf)
            for depth in R.DEPTHS:
                back = R.unpack(buf, lay, w, h, depth)
                if pix == R.Y800:
                    assert np.array_equal(back[:w * h], fr[:w * h]) and (back[w * h:] == 128).all()
                else:
                    assert np.array_equal(back, fr), (w, h, depth)
            named = np.zeros(buf.size, bool)  # the bytes the layout names, and only those, were written
            for p, (rb, rows) in enumerate(R.planes(pix, w, h)):
                for y in range(rows):
                    named[lay.offset[p] + y * lay.pitch[p]:lay.offset[p] + y * lay.pitch[p] + rb] = True
            assert (buf[~named] == 0xA5).all()
            other = np.zeros(buf.size, np.uint8)
            R.pack(fr, lay, w, h, other)
            assert np.array_equal(other[named], buf[named]), 'a named byte was left unwritten'


def test_reference_v210_equals_the_words_written_as_loops():
    """one 8x2 frame: a whole group and a partial one of two pixels, against the header's four words spelled out"""
    w, h = 8, 2
    rng = np.random.default_rng(7300)
    buf = rng.integers(0, 256, 32 * h, dtype=np.uint8)  # every bit random, bits 31..30 and the unused fields too
    L = pixref.Layout(R.V210, [32], [0], 64)
    words = buf.view('<u4').reshape(h, 8).astype(np.int64)
    f = lambda wd, k: (int(wd) >> (10 * k)) & 1023
    Y = np.zeros((h, w), np.int64); Cb = np.zeros((h, w // 2), np.int64); Cr = np.zeros((h, w // 2), np.int64)
    for y in range(h):
        g0, g1 = words[y][:4], words[y][4:]
        Y[y][:6] = [f(g0[0], 1), f(g0[1], 0), f(g0[1], 2), f(g0[2], 1), f(g0[3], 0), f(g0[3], 2)]
        Cb[y][:3] = [f(g0[0], 0), f(g0[1], 1), f(g0[2], 2)]
        Cr[y][:3] = [f(g0[0], 2), f(g0[2], 0), f(g0[3], 1)]
        Y[y][6:8] = [f(g1[0], 1), f(g1[1], 0)]
        Cb[y][3], Cr[y][3] = f(g1[0], 0), f(g1[0], 2)
    for depth in R.DEPTHS:
        want = []
        for plane, ph, pw in ((Y, h, w), (((Cb[0] + Cb[1] + 1) >> 1)[None], 1, w // 2), (((Cr[0] + Cr[1] + 1) >> 1)[None], 1, w // 2)):
            for y in range(ph):
                for x in range(pw):
                    v = int(plane[y][x])
                    want.append(min(255, (v + 2) >> 2) if depth == R.ROUND else v >> 2 if depth == R.TRUNC else min(255, (v + R.D[y & 1][x & 1]) >> 2))
        assert list(R.unpack(buf, L, w, h, depth)) == want, depth
    back = R.pack(R.unpack(buf, L, w, h), L, w, h, np.full(64, 0xA5, np.uint8)).view('<u4').reshape(h, 8)
    assert (back >> 30 == 0).all() and (back[:, 4] >> 30 == 0).all()
    assert (back[:, 5] >> 10 == 0).all() and (back[:, 6:] == 0).all(), 'fields beyond w are written as zeros'


def test_device_calls_refuse_bad_arguments_without_a_device(libpath):
    import h264mi
    B = h264mi.lib()
    to_i420, to_pix, to_opt = B.h264mi_pix_to_i420_dev, B.h264mi_i420_to_pix_dev, B.h264mi_pix_to_i420_opt_dev
    w, h = 36, 18
    a, b = 0x10000000, 0x20000000
    pa, pb = ctypes.c_void_p(a), ctypes.c_void_p(b)
    for pix in R.ALL:
        t = h264mi.pix_layout_tight(pix, w, h)
        r = ctypes.byref(t)
        assert to_i420(None, pb, r, w, h, 1, None) == -1 and to_pix(None, r, pb, w, h, 1, None) == -1 and to_i420(pa, pb, r, w, h, 0, None) == -1
        for opt in (h264mi.PixOpt(3), h264mi.PixOpt(-1), h264mi.PixOpt(0, (0, 1, 0))):
            assert to_opt(pa, pb, r, ctypes.byref(opt), w, h, 1, None) == -1
        for off in range(1, R.unit(pix)):  # a layout-side base that is no multiple of the unit
            assert to_i420(pa, ctypes.c_void_p(b + off), r, w, h, 1, None) == -1 and to_pix(ctypes.c_void_p(b + off), r, pa, w, h, 1, None) == -1
        for L, lw, lh, ok in _directed():
            if not ok and L.pix == pix:
                assert to_i420(pa, pb, ctypes.byref(_c(L)), lw, lh, 1, None) == -1 and to_pix(pb, ctypes.byref(_c(L)), pa, lw, lh, 1, None) == -1
        fs, fb = t.frame_stride, pixref.frame_bytes(w, h)
        for off in (0, R.unit(pix), -(fs - R.unit(pix))):  # overlapping byte ranges
            assert to_i420(pa, ctypes.c_void_p(a + off), r, w, h, 1, None) == -1 and to_pix(ctypes.c_void_p(a + off), r, pa, w, h, 1, None) == -1
        assert to_i420(pa, ctypes.c_void_p(a + 4 * ((fb + 3) // 4) - 4), r, w, h, 1, None) == -1
    for bad in (5, 15, 25):
        L = h264mi.PixLayout(bad, (64, 0, 0), (0, 0, 0), 1 << 20)
        assert to_i420(pa, pb, ctypes.byref(L), 16, 16, 1, None) == -1 and to_pix(pa, ctypes.byref(L), pb, 16, 16, 1, None) == -1
