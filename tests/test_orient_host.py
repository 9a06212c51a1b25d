"""CPU: rotating and mirroring exists at every layer -- declared in include/h264mi.h, exported by the library, bound in
Python --, the library's size, compose and inverse equal those of tests/orientref.py (the reference of the GPU tests),
the reference equals the D[y][x] formulas of the header's table written as loops, the algebra holds on frames, and
h264mi_i420_orient_dev refuses bad arguments before touching a device."""
import ctypes

import numpy as np
import pytest

import orientref
from test_capi_exports import declared_functions

NEW = ('h264mi_orient_size', 'h264mi_orient_compose', 'h264mi_orient_inverse', 'h264mi_i420_orient_dev', 'h264mi_enc_encode_oriented')
NAMES = ('IDENTITY', 'ROT90', 'ROT180', 'ROT270', 'MIRROR', 'FLIP', 'TRANSPOSE', 'TRANSVERSE')

# the D[y][x] column of the header's table: (whether the destination is ph x pw, the source sample of D[y][x])
TABLE = {
    0: (False, lambda S, pw, ph, x, y: S[y][x]),
    1: (True, lambda S, pw, ph, x, y: S[ph - 1 - x][y]),
    2: (False, lambda S, pw, ph, x, y: S[ph - 1 - y][pw - 1 - x]),
    3: (True, lambda S, pw, ph, x, y: S[x][pw - 1 - y]),
    4: (False, lambda S, pw, ph, x, y: S[y][pw - 1 - x]),
    5: (False, lambda S, pw, ph, x, y: S[ph - 1 - y][x]),
    6: (True, lambda S, pw, ph, x, y: S[x][y]),
    7: (True, lambda S, pw, ph, x, y: S[ph - 1 - x][pw - 1 - y]),
}


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
    assert [len(getattr(B, n).argtypes) for n in NEW] == [5, 2, 1, 7, 3]
    assert callable(h264mi.i420_orient) and callable(h264mi.BatchEncoder.encode_oriented)
    assert callable(h264mi.orient_size) and callable(h264mi.orient_compose) and callable(h264mi.orient_inverse)
    for k, name in enumerate(NAMES):
        assert getattr(h264mi, 'ORIENT_' + name) == k == getattr(orientref, name)


@pytest.mark.parametrize('orient', orientref.ALL, ids=NAMES)
def test_reference_equals_the_formulas_of_the_table(orient):
    rng = np.random.default_rng(40 + orient)
    for pw, ph in ((3, 5), (4, 2)):
        S = rng.integers(0, 256, (ph, pw), dtype=np.uint8)
        turned, at = TABLE[orient]
        qw, qh = (ph, pw) if turned else (pw, ph)
        want = np.empty((qh, qw), np.uint8)
        for y in range(qh):
            for x in range(qw):
                want[y][x] = at(S, pw, ph, x, y)
        got = orientref.orient_plane(S, orient)
        assert got.shape == want.shape and np.array_equal(got, want)


def test_library_size_compose_inverse_equal_the_reference(libpath):
    import h264mi
    B = h264mi.lib()
    for a in orientref.ALL:
        for w, h in ((2, 2), (36, 18), (8192, 2)):
            assert h264mi.orient_size(a, w, h) == orientref.size(a, w, h)
        assert B.h264mi_orient_inverse(a) == orientref.inverse(a) == h264mi.orient_inverse(a)
        for b in orientref.ALL:
            assert B.h264mi_orient_compose(a, b) == orientref.compose(a, b) == h264mi.orient_compose(a, b), (a, b)
    dw, dh = ctypes.c_int(-7), ctypes.c_int(-7)
    for bad in (-1, 8):
        assert B.h264mi_orient_inverse(bad) == -1
        assert B.h264mi_orient_compose(bad, 0) == -1 and B.h264mi_orient_compose(0, bad) == -1
        assert B.h264mi_orient_size(bad, 16, 16, ctypes.byref(dw), ctypes.byref(dh)) == -1
        with pytest.raises(ValueError):
            h264mi.orient_inverse(bad)
        with pytest.raises(ValueError):
            h264mi.orient_compose(1, bad)
    for w, h in ((0, 16), (16, 0), (-2, 16), (15, 16), (16, 17), (8194, 16), (16, 8194)):
        assert B.h264mi_orient_size(1, w, h, ctypes.byref(dw), ctypes.byref(dh)) == -1, (w, h)
        with pytest.raises(ValueError):
            h264mi.orient_size(1, w, h)
    assert B.h264mi_orient_size(1, 16, 16, None, ctypes.byref(dh)) == -1 and B.h264mi_orient_size(1, 16, 16, ctypes.byref(dw), None) == -1
    assert (dw.value, dh.value) == (-7, -7), 'a refused call writes nothing'


def test_the_algebra_holds_on_frames():
    w, h = 36, 18
    f = np.random.default_rng(41).integers(0, 256, orientref.frame_bytes(w, h), dtype=np.uint8)
    assert sorted(orientref.INVERSE) == list(orientref.ALL)
    for a in orientref.ALL:
        aw, ah = orientref.size(a, w, h)
        fa = orientref.orient_frame(f, w, h, a)
        assert fa.size == f.size
        assert np.array_equal(orientref.orient_frame(fa, aw, ah, orientref.inverse(a)), f), a
        assert orientref.size(orientref.inverse(a), aw, ah) == (w, h)
        for b in orientref.ALL:
            c = orientref.compose(a, b)
            assert np.array_equal(orientref.orient_frame(fa, aw, ah, b), orientref.orient_frame(f, w, h, c)), (a, b)
            assert orientref.size(b, aw, ah) == orientref.size(c, w, h)
    assert np.array_equal(orientref.orient_frame(f, w, h, 0), f)
    assert orientref.compose(1, 1) == 2 and orientref.compose(1, 2) == 3 and orientref.inverse(1) == 3 and orientref.inverse(3) == 1


# (sw, sh, n, orient) that h264mi_i420_orient_dev must refuse; the pointers are never dereferenced
BAD = [(32, 32, 0, 1), (32, 32, -1, 1),                                        # n <= 0
       (31, 32, 1, 1), (32, 31, 1, 0), (33, 33, 1, 6),                         # an odd side
       (0, 32, 1, 1), (32, 0, 1, 2), (-2, 32, 1, 1), (32, -2, 1, 4),           # zero or negative
       (8194, 32, 1, 1), (32, 8194, 1, 0), (8194, 8194, 1, 7),                 # above 8192
       (32, 32, 1, -1), (32, 32, 1, 8)]                                        # no such orientation


def test_orient_dev_refuses_bad_arguments_without_a_device(libpath):
    import h264mi
    fn = h264mi.lib().h264mi_i420_orient_dev
    d, s = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x20000000)
    for orient in orientref.ALL:
        assert fn(None, s, 32, 32, 1, orient, None) == -1
        assert fn(d, None, 32, 32, 1, orient, None) == -1
    for sw, sh, n, orient in BAD:
        assert fn(d, s, sw, sh, n, orient, None) == -1, (sw, sh, n, orient)
    # overlapping byte ranges: a 32x16 frame is 768 bytes on both sides, the destination 16x32 after a quarter turn
    base, fb = 0x10000000, 768
    assert orientref.frame_bytes(32, 16) == fb == orientref.frame_bytes(*orientref.size(1, 32, 16))
    for orient in (0, 1, 4, 7):
        for doff in (0, 1, fb - 1, -1, -(fb - 1)):
            assert fn(ctypes.c_void_p(base + doff), ctypes.c_void_p(base), 32, 16, 1, orient, None) == -1, (orient, doff)
        for doff in (3 * fb - 1, -(3 * fb - 1)):  # the last byte of the third frame
            assert fn(ctypes.c_void_p(base + doff), ctypes.c_void_p(base), 32, 16, 3, orient, None) == -1, (orient, doff)
    assert h264mi.lib().h264mi_enc_encode_oriented(None, s, 1) == -1
