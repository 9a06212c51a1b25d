"""CPU: the pixel formats and pitched layouts exist at every layer -- declared in include/h264mi.h, exported by the
library, bound in Python --, the library's tight layouts, spans and layout rule equal those of tests/pixref.py (the
reference of the GPU tests) on directed and seeded random layouts, the reference's algebra holds, and every device call
refuses bad arguments before touching a device."""
import ctypes
import re
import os

import numpy as np
import pytest

import pixref
from test_capi_exports import declared_functions

NEW = ('h264mi_pix_layout_tight', 'h264mi_pix_span', 'h264mi_pix_layout_ok', 'h264mi_pix_to_i420_dev', 'h264mi_i420_to_pix_dev',
       'h264mi_enc_encode_pix', 'h264mi_dec_set_output_layout', 'h264mi_dec_output_layout')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX, INT64_MAX = (1 << 31) - 1, (1 << 63) - 1
SIZES = ((2, 2), (36, 18), (8192, 8192))


def _c(L):
    """a pixref.Layout as the library's struct"""
    import h264mi
    return h264mi.PixLayout(L.pix, L.pitch, L.offset, L.frame_stride)


def test_header_declares_library_exports_python_binds(libpath):
    names = declared_functions()
    L = ctypes.CDLL(libpath)
    for n in NEW:
        assert n in names, n
        assert hasattr(L, n), n
    import h264mi
    B = h264mi.lib()
    assert [len(getattr(B, n).argtypes) for n in NEW] == [4, 3, 3, 7, 7, 3, 2, 2]
    assert B.h264mi_pix_span.restype is ctypes.c_int64
    assert ctypes.sizeof(h264mi.PixLayout) == 48
    for f in ('pix_layout_tight', 'pix_span', 'pix_layout_ok', 'pix_to_i420', 'i420_to_pix'):
        assert callable(getattr(h264mi, f)), f
    assert callable(h264mi.BatchEncoder.encode_pix)
    assert callable(h264mi.BatchDecoder.set_output_layout) and callable(h264mi.BatchDecoder.output_layout)
    assert h264mi.BatchDecoder.OUTPUT_FORMATS == {'i420': 0, 'rgba': 1}


def test_constants_agree_across_header_python_and_reference():
    import h264mi
    src = open(os.path.join(ROOT, 'include', 'h264mi.h')).read()
    for k, name in enumerate(pixref.NAMES):
        m = re.search(r'^#define H264MI_PIX_%s (\d+)' % name, src, flags=re.M)
        assert m and int(m.group(1)) == k == getattr(h264mi, 'PIX_' + name) == getattr(pixref, name)
    m = re.search(r'^#define H264MI_FMT_LAYOUT (\d+)', src, flags=re.M)
    assert m and int(m.group(1)) == 2 == h264mi.FMT_LAYOUT
    assert pixref.MAX_SIDE == 8192 and pixref.MAX_PITCH == 65536


@pytest.mark.parametrize('pix', pixref.ALL, ids=pixref.NAMES)
def test_tight_layouts_and_spans_equal_the_reference(libpath, pix):
    import h264mi
    for w, h in SIZES:
        got, want = h264mi.pix_layout_tight(pix, w, h), pixref.tight(pix, w, h)
        assert (got.pix, list(got.pitch), list(got.offset), got.frame_stride) == (want.pix, want.pitch, want.offset, want.frame_stride)
        assert h264mi.pix_span(got, w, h) == pixref.span(want, w, h) == want.frame_stride
        assert h264mi.pix_layout_ok(got, w, h) == 0 and pixref.layout_ok(want, w, h)
        bits = {pixref.I420: 12, pixref.NV12: 12, pixref.NV21: 12, pixref.YUY2: 16, pixref.UYVY: 16}[pix]
        assert want.frame_stride == w * h * bits // 8
    t = h264mi.pix_layout_tight(pixref.I420, 36, 18)
    assert list(t.offset) == [0, 36 * 18, 36 * 18 + 18 * 9] and t.frame_stride == pixref.frame_bytes(36, 18), "the library's tight I420"
    out = h264mi.PixLayout(7, (7, 7, 7), (7, 7, 7), 7)
    B = h264mi.lib()
    for bad in ((-1, 16, 16), (5, 16, 16), (0, 15, 16), (0, 16, 0), (1, 8194, 16), (3, 16, -2)):
        assert B.h264mi_pix_layout_tight(ctypes.byref(out), *bad) == -1, bad
        with pytest.raises(ValueError):
            h264mi.pix_layout_tight(*bad)
    assert B.h264mi_pix_layout_tight(None, 0, 16, 16) == -1
    assert (out.pix, list(out.pitch), list(out.offset), out.frame_stride) == (7, [7] * 3, [7] * 3, 7), 'a refused call writes nothing'
    assert B.h264mi_pix_span(None, 16, 16) == -1 and B.h264mi_pix_layout_ok(None, 16, 16) == -1


def _agree(L, w, h):
    import h264mi
    c = _c(L)
    s = pixref.span(L, w, h)
    assert h264mi.pix_span(c, w, h) == s, (L, w, h)
    assert h264mi.pix_layout_ok(c, w, h) == (0 if pixref.layout_ok(L, w, h) else -1), (L, w, h)
    return pixref.layout_ok(L, w, h)


def _directed():
    """(layout, w, h, expected) with the one rule each breaks"""
    w, h = 36, 18
    out = []
    for pix in pixref.ALL:
        t = pixref.tight(pix, w, h)
        np_ = len(pixref.planes(pix, w, h))
        out.append((t, w, h, True))
        a = pixref.tight(pix, w, h); a.pitch[0] -= 1  # a pitch one below the row bytes
        out.append((a, w, h, False))
        a = pixref.tight(pix, w, h); a.frame_stride -= 1  # a frame_stride one below the span
        out.append((a, w, h, False))
        a = pixref.tight(pix, w, h); a.frame_stride += 7
        out.append((a, w, h, True))
        if np_ > 1:
            a = pixref.tight(pix, w, h); a.offset[1] -= 1  # planes that overlap by one byte
            out.append((a, w, h, False))
            a = pixref.tight(pix, w, h); a.offset[0] = a.frame_stride - 1; a.frame_stride += w * h  # plane 0 begins in the last byte of the last plane
            out.append((a, w, h, False))
            a = pixref.tight(pix, w, h); a.offset[0] = a.frame_stride; a.frame_stride += w * h  # the planes in another order, touching
            out.append((a, w, h, True))
        if np_ < 3:
            a = pixref.tight(pix, w, h); a.pitch[2] = 1  # a nonzero unused entry
            out.append((a, w, h, False))
            a = pixref.tight(pix, w, h); a.offset[2] = 1
            out.append((a, w, h, False))
        a = pixref.tight(pix, w, h); a.offset[0] = -1  # a negative offset
        out.append((a, w, h, False))
        out.append((t, w + 1, h, False))  # an odd w
        out.append((t, w, h + 1, False))
        out.append((pixref.tight(pix, 8192, 16), 8194, 16, False))  # a side of 8194
        out.append((pixref.tight(pix, 16, 8192), 16, 8194, False))
        out.append((pixref.tight(pix, 16, 16), 0, 16, False))
        a = pixref.tight(pix, w, h); a.pitch[0] = 65536; a.offset = [o + 70000 * h if 0 < k < np_ else o for k, o in enumerate(a.offset)]
        a.frame_stride = a.offset[np_ - 1] + 70000 * h  # the largest pitch
        out.append((a, w, h, True))
        a = pixref.tight(pix, w, h); a.pitch[0] = 65537; a.frame_stride = INT64_MAX
        out.append((a, w, h, False))
        # fields at the int32 and int64 limits
        a = pixref.tight(pix, w, h); a.pitch[0] = INT32_MAX; a.frame_stride = INT64_MAX
        out.append((a, w, h, False))
        a = pixref.tight(pix, w, h); a.pitch[0] = -INT32_MAX - 1
        out.append((a, w, h, False))
        a = pixref.tight(pix, w, h); a.frame_stride = INT64_MAX
        out.append((a, w, h, True))
        a = pixref.tight(pix, w, h); a.frame_stride = -INT64_MAX - 1
        out.append((a, w, h, False))
        a = pixref.tight(pix, w, h); a.offset[np_ - 1] = INT64_MAX; a.frame_stride = INT64_MAX  # the span leaves int64
        out.append((a, w, h, False))
        a = pixref.tight(pix, w, h); a.offset[np_ - 1] = INT64_MAX - a.pitch[np_ - 1] * pixref.planes(pix, w, h)[np_ - 1][1]; a.frame_stride = INT64_MAX
        out.append((a, w, h, True))  # ... and just fits it
        a = pixref.tight(pix, w, h); a.offset[0] = -INT64_MAX - 1
        out.append((a, w, h, False))
    out.append((pixref.Layout(5, [16], [0], 1 << 20), 16, 16, False))  # no such format
    out.append((pixref.Layout(-1, [16], [0], 1 << 20), 16, 16, False))
    out.append((pixref.Layout(INT32_MAX, [16], [0], 1 << 20), 16, 16, False))
    return out


def test_layout_ok_on_directed_layouts(libpath):
    for L, w, h, want in _directed():
        assert _agree(L, w, h) == want, (L, w, h)


def test_layout_ok_on_random_layouts(libpath):
    """seeded: half the layouts start good (planes placed in a random order with random gaps and pitches) and get at most
    one field disturbed, the rest have every field random with the extremes mixed in"""
    rng = np.random.default_rng(5100)
    extremes = [0, 1, -1, INT32_MAX, -INT32_MAX - 1, 65536, 65537]
    extremes64 = extremes + [INT64_MAX, -INT64_MAX - 1, INT64_MAX - 1, 1 << 31, 1 << 32]
    good = 0
    for it in range(4000):
        pix = int(rng.integers(0, 5))
        w, h = 2 * int(rng.integers(1, 40)), 2 * int(rng.integers(1, 40))
        if it % 2 == 0:
            pl = pixref.planes(pix, w, h)
            pitch = [rb + int(rng.integers(0, 3)) * int(rng.integers(0, 40)) for rb, _ in pl]
            offset, at = [0] * len(pl), int(rng.integers(0, 3)) * int(rng.integers(0, 100))
            for p in rng.permutation(len(pl)):
                offset[p] = at
                at += (pl[p][1] - 1) * pitch[p] + pl[p][0] + int(rng.integers(0, 2)) * int(rng.integers(0, 50))
            L = pixref.Layout(pix, pitch, offset, at + int(rng.integers(0, 2)) * int(rng.integers(0, 50)))
            k = int(rng.integers(0, 12))  # disturb one field, or (k >= 8) none
            d = int(rng.integers(-40, 41))
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
            L = pixref.Layout(int(rng.integers(-1, 6)), [f32() for _ in range(3)], [f64() for _ in range(3)], f64())
            if rng.integers(0, 4) == 0:
                w = int(rng.choice([0, -2, 8192, 8194, 3]))
        good += _agree(L, w, h)
    assert 800 < good < 3200, f'{good} good layouts of 4000: the sample shows little'


@pytest.mark.parametrize('pix', pixref.ALL, ids=pixref.NAMES)
def test_reference_i420_to_format_and_back_is_the_identity(pix):
    rng = np.random.default_rng(5200 + pix)
    for w, h in ((2, 2), (36, 18), (16, 6)):
        fr = rng.integers(0, 256, pixref.frame_bytes(w, h), dtype=np.uint8)
        t = pixref.tight(pix, w, h)
        L = pixref.Layout(pix, [p + 5 for p in t.pitch[:len(pixref.planes(pix, w, h))]], [0] * 3, 0)
        at = 3
        for p, (rb, rows) in enumerate(pixref.planes(pix, w, h)):
            L.offset[p] = at
            at += rows * L.pitch[p] + 2
        L.frame_stride = at
        for lay in (t, L):
            buf = np.full(pixref.span(lay, w, h) + 9, 0xA5, np.uint8)
            pixref.pack(fr, lay, w, h, buf)
            assert np.array_equal(pixref.unpack(buf, lay, w, h), fr)
            named = np.zeros(buf.size, bool)  # the bytes the layout names, and only those, were written
            for p, (rb, rows) in enumerate(pixref.planes(pix, w, h)):
                for y in range(rows):
                    named[lay.offset[p] + y * lay.pitch[p]:lay.offset[p] + y * lay.pitch[p] + rb] = True
            assert (buf[~named] == 0xA5).all()
            other = np.zeros(buf.size, np.uint8)
            pixref.pack(fr, lay, w, h, other)
            assert np.array_equal(other[named], buf[named])


@pytest.mark.parametrize('pix', (pixref.YUY2, pixref.UYVY), ids=('YUY2', 'UYVY'))
def test_reference_422_equals_the_formulas_written_as_loops(pix):
    w, h = 4, 4
    rng = np.random.default_rng(5300 + pix)
    buf = rng.integers(0, 256, 2 * w * h, dtype=np.uint8)
    buf[1] = 255; buf[1 + 2 * w] = 254  # a rounding case at the top of the range, in either format's chroma or luma
    rows = buf.reshape(h, 2 * w)
    yo = 0 if pix == pixref.YUY2 else 1
    Y = np.zeros((h, w), np.uint8)
    C = [np.zeros((h, w // 2), np.uint8), np.zeros((h, w // 2), np.uint8)]  # 4:2:2 Cb, Cr
    for y in range(h):
        for k in range(w // 2):
            Y[y][2 * k], Y[y][2 * k + 1] = rows[y][4 * k + yo], rows[y][4 * k + 2 + yo]
            C[0][y][k], C[1][y][k] = rows[y][4 * k + 1 - yo], rows[y][4 * k + 3 - yo]
    want = list(Y.ravel())
    for c in C:
        for y in range(h // 2):
            for x in range(w // 2):
                want.append((int(c[2 * y][x]) + int(c[2 * y + 1][x]) + 1) >> 1)
    got = pixref.unpack(buf, pixref.tight(pix, w, h), w, h)
    assert list(got) == want
    # back: C422[y][x] = C420[y >> 1][x]; the identity exactly when the chroma row pairs are equal
    back = pixref.pack(got, pixref.tight(pix, w, h), w, h, np.zeros(2 * w * h, np.uint8)).reshape(h, 2 * w)
    for y in range(h):
        for k in range(w // 2):
            assert back[y][4 * k + yo] == Y[y][2 * k] and back[y][4 * k + 2 + yo] == Y[y][2 * k + 1]
            assert back[y][4 * k + 1 - yo] == got[w * h + (y >> 1) * (w // 2) + k]
            assert back[y][4 * k + 3 - yo] == got[w * h + (w // 2) * (h // 2) + (y >> 1) * (w // 2) + k]
    assert not np.array_equal(back.ravel(), buf)
    rows[1::2] = rows[0::2]  # now every chroma row pair is equal (and the luma rows, which are moved anyway)
    again = pixref.pack(pixref.unpack(buf, pixref.tight(pix, w, h), w, h), pixref.tight(pix, w, h), w, h, np.zeros(2 * w * h, np.uint8))
    assert np.array_equal(again, buf)


def test_device_calls_refuse_bad_arguments_without_a_device(libpath):
    import h264mi
    B = h264mi.lib()
    to_i420, to_pix = B.h264mi_pix_to_i420_dev, B.h264mi_i420_to_pix_dev
    w, h = 32, 16
    fb = pixref.frame_bytes(w, h)
    a, b = 0x10000000, 0x20000000
    pa, pb = ctypes.c_void_p(a), ctypes.c_void_p(b)
    for pix in pixref.ALL:
        t = h264mi.pix_layout_tight(pix, w, h)
        r = ctypes.byref(t)
        assert to_i420(None, pb, r, w, h, 1, None) == -1 and to_i420(pa, None, r, w, h, 1, None) == -1
        assert to_i420(pa, pb, None, w, h, 1, None) == -1
        assert to_pix(None, r, pb, w, h, 1, None) == -1 and to_pix(pa, r, None, w, h, 1, None) == -1
        assert to_pix(pa, None, pb, w, h, 1, None) == -1
        for n in (0, -1):
            assert to_i420(pa, pb, r, w, h, n, None) == -1 and to_pix(pa, r, pb, w, h, n, None) == -1
        for bw, bh in ((31, 16), (32, 15), (0, 16), (8194, 16), (34, 16)):  # 34: the pitch falls below the row bytes
            assert to_i420(pa, pb, r, bw, bh, 1, None) == -1 and to_pix(pa, r, pb, bw, bh, 1, None) == -1, (bw, bh)
        for L, lw, lh, ok in _directed()[:12]:  # at the case's own size: the tight layout is refused for 37x18, not for 36x18
            if not ok and L.pix == pix:
                assert to_i420(pa, pb, ctypes.byref(_c(L)), lw, lh, 1, None) == -1
        # overlapping byte ranges: n * frame_stride on the layout's side, n tight frames on the other
        fs = t.frame_stride
        for n in (1, 3):
            for off in (0, 1, n * fb - 1, -(n * fs - 1)):  # the layout's side at a + off, the tight frames at a
                assert to_i420(pa, ctypes.c_void_p(a + off), r, w, h, n, None) == -1, (pix, n, off)
                assert to_pix(ctypes.c_void_p(a + off), r, pa, w, h, n, None) == -1, (pix, n, off)
        t.frame_stride = fs + 100  # the gap after the last frame counts: n * frame_stride
        assert to_pix(pa, ctypes.byref(t), ctypes.c_void_p(a + 3 * (fs + 100) - 1), w, h, 3, None) == -1
        t.frame_stride = INT64_MAX  # a range no address space holds
        assert to_pix(pa, ctypes.byref(t), pb, w, h, 3, None) == -1 and to_i420(pb, pa, ctypes.byref(t), w, h, 2, None) == -1
    t = h264mi.pix_layout_tight(pixref.NV12, w, h)
    assert B.h264mi_enc_encode_pix(None, pb, ctypes.byref(t)) == -1
    assert B.h264mi_dec_set_output_layout(None, ctypes.byref(t)) == -1 and B.h264mi_dec_set_output_layout(None, None) == -1
    assert B.h264mi_dec_output_layout(None, ctypes.byref(t)) == -1
