"""CPU: the I420 downscaler exists at every layer -- declared in include/h264mi.h, exported by the library, bound in
Python --, h264mi_i420_scale_dev refuses bad arguments before touching a device, and tests/scaleref.py (the reference
of the GPU tests) has the properties the definition promises: weight sums, identity, 2:1, constants."""
import ctypes

import numpy as np
import pytest

import scaleref
from test_capi_exports import declared_functions

NEW = ('h264mi_i420_scale_dev', 'h264mi_enc_encode_scaled')
PAIRS = [(16, 16), (18, 10), (36, 20), (48, 32), (256, 16), (1920, 1280), (1080, 360), (4096, 854), (9, 5), (8, 1), (4096, 2)]


def test_header_declares_library_exports_python_binds(libpath):
    names = declared_functions()
    L = ctypes.CDLL(libpath)
    for n in NEW:
        assert n in names, n
        assert hasattr(L, n), n
    import h264mi
    B = h264mi.lib()
    for n in NEW:
        assert getattr(B, n).argtypes is not None, n
    assert len(B.h264mi_i420_scale_dev.argtypes) == 8 and len(B.h264mi_enc_encode_scaled.argtypes) == 4
    assert callable(h264mi.i420_scale) and callable(h264mi.BatchEncoder.encode_scaled)


@pytest.mark.parametrize('p,q', PAIRS, ids=[f'{p}to{q}' for p, q in PAIRS])
def test_weight_sums_and_support(p, q):
    w = scaleref.weights(p, q)
    assert w.shape == (q, p) and w.dtype == np.int64 and int(w.min()) >= 0
    assert (w.sum(axis=1) == p).all(), 'the weights of one output sample sum to p'
    assert (w.sum(axis=0) == q).all(), 'the weights of one source sample sum to q'
    for o in (0, q // 2, q - 1):  # non-zero exactly on [o p / q, ceil((o + 1) p / q) - 1]
        nz = np.flatnonzero(w[o])
        assert nz[0] == o * p // q and nz[-1] == -(-(o + 1) * p // q) - 1 and len(nz) == nz[-1] - nz[0] + 1
    assert np.flatnonzero(w[q - 1])[-1] == p - 1
    assert max(int((row > 0).sum()) for row in w) <= -(-p // q) + 1


def test_identity_returns_the_bytes():
    rng = np.random.default_rng(11)
    for w, h in ((16, 16), (36, 18), (38, 22)):
        f = rng.integers(0, 256, scaleref.frame_bytes(w, h), dtype=np.uint8)
        assert np.array_equal(scaleref.scale_frame(f, w, h, w, h), f)


def test_two_to_one_is_the_rounded_mean_of_four():
    rng = np.random.default_rng(12)
    for w, h in ((32, 32), (36, 20)):
        f = rng.integers(0, 256, scaleref.frame_bytes(w, h), dtype=np.uint8)
        got = scaleref.planes(scaleref.scale_frame(f, w, h, w // 2, h // 2), w // 2, h // 2)
        for g, p in zip(got, scaleref.planes(f, w, h)):
            ph, pw = p.shape
            if pw % 2 or ph % 2:  # 36x20's chroma is 18x10 -> 9x5: still 2:1
                assert (pw, ph) == (18, 10)
            a = p.astype(np.int32)
            want = (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2
            assert np.array_equal(g, want.astype(np.uint8))


def test_a_constant_frame_stays_constant():
    for c in (0, 1, 127, 128, 254, 255):
        for (sw, sh, dw, dh) in ((36, 18, 20, 10), (48, 36, 32, 24), (256, 64, 16, 16), (38, 22, 38, 10)):
            f = np.full(scaleref.frame_bytes(sw, sh), c, np.uint8)
            out = scaleref.scale_frame(f, sw, sh, dw, dh)
            assert out.size == scaleref.frame_bytes(dw, dh) and (out == c).all()


def test_three_to_two_by_hand():
    """48 -> 32 columns: output 2k = (2 a + b) / 3 of source 3k, 3k + 1; output 2k + 1 = (b + 2 c) / 3 of 3k + 1, 3k + 2"""
    rng = np.random.default_rng(13)
    p = rng.integers(0, 256, (4, 48), dtype=np.uint8)
    got = scaleref.scale_plane(p, 32, 4)
    a = p.astype(np.int64)
    assert np.array_equal(got[:, 0::2], (2 * a[:, 0::3] + a[:, 1::3] + 1) // 3)  # (4 (2a + b) 32 + 96) // 192, exactly
    assert np.array_equal(got[:, 1::2], (a[:, 1::3] + 2 * a[:, 2::3] + 1) // 3)


# (dw, dh, sw, sh, n) that h264mi_i420_scale_dev must refuse; the pointers are never dereferenced
BAD = [(16, 16, 32, 32, 0), (16, 16, 32, 32, -1),                       # n <= 0
       (15, 16, 32, 32, 1), (16, 15, 32, 32, 1), (16, 16, 31, 32, 1), (16, 16, 32, 31, 1),  # an odd size
       (0, 16, 32, 32, 1), (16, 0, 32, 32, 1), (-2, 16, 32, 32, 1),    # dw, dh below 2
       (34, 16, 32, 32, 1), (16, 34, 32, 32, 1),                       # upscaling in either direction
       (16, 16, 4098, 32, 1), (16, 16, 32, 4098, 1), (4098, 16, 4098, 32, 1)]  # a source above 4096


def test_scale_dev_refuses_bad_arguments_without_a_device(libpath):
    import h264mi
    fn = h264mi.lib().h264mi_i420_scale_dev
    d, s = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x20000000)
    assert fn(None, 16, 16, s, 32, 32, 1, None) == -1
    assert fn(d, 16, 16, None, 32, 32, 1, None) == -1
    for dw, dh, sw, sh, n in BAD:
        assert fn(d, dw, dh, s, sw, sh, n, None) == -1, (dw, dh, sw, sh, n)
    # overlapping byte ranges: one 32x32 source frame is 1536 bytes, one 16x16 destination frame 384
    base = 0x10000000
    for doff in (0, 1, 1535, -1, -383):
        assert fn(ctypes.c_void_p(base + doff), 16, 16, ctypes.c_void_p(base), 32, 32, 1, None) == -1, doff
    assert fn(ctypes.c_void_p(base + 1536 * 3 - 1), 16, 16, ctypes.c_void_p(base), 32, 32, 3, None) == -1  # n frames count
    assert h264mi.lib().h264mi_enc_encode_scaled(None, s, 32, 32) == -1
