"""CPU: the quality surface (per-frame SSE / PSNR / SSIM) exists at every layer -- declared in include/h264mi.h,
exported by the library, bound and mirrored in Python --, the entry points refuse bad arguments before touching a
device, h264mi_psnr is what the header says, and tests/qualityref.py (the reference of the GPU tests) agrees with a
plain per-window loop written here."""
import ctypes
import math

import numpy as np

import qualityref
from test_capi_exports import declared_functions

NEW = ('h264mi_i420_quality_dev', 'h264mi_enc_set_quality', 'h264mi_enc_quality_enabled', 'h264mi_enc_quality',
       'h264mi_enc_quality_dev', 'h264mi_psnr')


def test_header_declares_library_exports_python_mirrors(libpath):
    names = declared_functions()
    L = ctypes.CDLL(libpath)
    for n in NEW:
        assert n in names, n
        assert hasattr(L, n), n
    import h264mi
    B = h264mi.lib()
    for n in NEW:
        assert getattr(B, n).argtypes is not None, n
    assert ctypes.sizeof(h264mi.Quality) == 64
    assert [f[0] for f in h264mi.Quality._fields_] == ['sse', 'ssim_fix', 'windows', 'coded', 'reserved']
    assert h264mi.Quality.ssim_fix.offset == 24 and h264mi.Quality.windows.offset == 48 and h264mi.Quality.coded.offset == 56
    for m in ('set_quality', 'quality', 'quality_ptr'):
        assert callable(getattr(h264mi.BatchEncoder, m)), m
    assert callable(h264mi.i420_quality) and callable(h264mi.psnr)


def test_quality_dev_refuses_bad_arguments_without_a_device(libpath):
    import h264mi
    L = h264mi.lib()
    o, a, b = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000)  # never dereferenced
    fn = L.h264mi_i420_quality_dev
    assert fn(None, a, b, 16, 16, 1, None) == -1
    assert fn(o, None, b, 16, 16, 1, None) == -1
    assert fn(o, a, None, 16, 16, 1, None) == -1
    assert fn(o, a, b, 16, 16, 0, None) == -1
    assert fn(o, a, b, 16, 16, -2, None) == -1
    assert fn(o, a, b, 17, 16, 1, None) == -1
    assert fn(o, a, b, 16, 17, 1, None) == -1
    assert fn(o, a, b, 14, 16, 1, None) == -1
    assert fn(o, a, b, 16, 14, 1, None) == -1
    assert fn(o, a, b, 0, 16, 1, None) == -1
    assert fn(o, a, b, 16, -16, 1, None) == -1


def test_null_encoder_forms(libpath):
    import h264mi
    L = h264mi.lib()
    q = h264mi.Quality()
    assert L.h264mi_enc_set_quality(None, 1) == -1
    assert L.h264mi_enc_set_quality(None, 0) == -1
    assert L.h264mi_enc_quality_enabled(None) == -1
    assert L.h264mi_enc_quality(None, 0, ctypes.byref(q)) == -1
    assert L.h264mi_enc_quality_dev(None) is None


def test_psnr(libpath):
    import h264mi
    for n in (1, 25344, 1920 * 1080, 1 << 40):
        assert h264mi.psnr(0, n) == 100.0
        assert h264mi.psnr(65025 * n, n) == 0.0
        want = 10 * math.log10(65025)
        got = h264mi.psnr(n, n)
        assert got == want or got in (np.nextafter(want, 0.0), np.nextafter(want, 100.0)), (n, got, want)
    assert h264mi.psnr(1000, 500) < h264mi.psnr(999, 500)


def _loop_windows(a, b):
    """the definition, window by window, in plain Python integers and floats"""
    ph, pw = a.shape
    out = []
    for y in range(0, ph - 8 + 1, 4):
        row = []
        for x in range(0, pw - 8 + 1, 4):
            s1 = s2 = ss = s12 = 0
            for j in range(8):
                for i in range(8):
                    p, q = int(a[y + j, x + i]), int(b[y + j, x + i])
                    s1 += p
                    s2 += q
                    ss += p * p + q * q
                    s12 += p * q
            vars_ = 64 * ss - s1 * s1 - s2 * s2
            covar = 64 * s12 - s1 * s2
            num = (2 * s1 * s2 + 416) * (2 * covar + 235963)
            den = (s1 * s1 + s2 * s2 + 416) * (vars_ + 235963)
            assert abs(num) < 2.9e17 and 0 < den < 2.9e17
            row.append(round(float(num) / float(den) * 4294967296.0))  # round(): to nearest, ties to even
        out.append(row)
    return np.array(out, np.int64)


def test_qualityref_equals_a_plain_loop():
    rng = np.random.default_rng(7)
    a = rng.integers(0, 256, (20, 24), dtype=np.uint8)
    for b in (np.clip(a.astype(int) + rng.integers(-9, 10, a.shape), 0, 255).astype(np.uint8),  # mild noise
              rng.integers(0, 256, a.shape, dtype=np.uint8),                                    # unrelated
              255 - a):                                                                          # negative covariance
        got = qualityref.plane_windows(a, b)
        assert got.shape == (4, 5)
        assert np.array_equal(got, _loop_windows(a, b))
    assert (qualityref.plane_windows(a, 255 - a) < 0).any()
    d = a.astype(np.int64) - (255 - a).astype(np.int64)
    assert qualityref.plane_quality(a, 255 - a)[0] == int((d * d).sum())


def test_identical_planes_are_exactly_one():
    rng = np.random.default_rng(8)
    for a in (rng.integers(0, 256, (20, 24), dtype=np.uint8), np.zeros((16, 16), np.uint8), np.full((9, 18), 255, np.uint8)):
        sse, fix, n = qualityref.plane_quality(a, a.copy())
        assert sse == 0 and fix == n << 32


def test_window_counts():
    rng = np.random.default_rng(9)
    for (w, h), lw, cw in (((16, 16), 9, 1), ((36, 18), 8 * 3, 3 * 1)):
        f = rng.integers(0, 256, w * h * 3 // 2, dtype=np.uint8)
        q = qualityref.frame_quality(f, f, w, h)
        assert q['windows'] == [lw, cw]
        ax, ay = qualityref.window_counts(w, h)
        cx, cy = qualityref.window_counts(w // 2, h // 2)
        assert (ax * ay, cx * cy) == (lw, cw)
