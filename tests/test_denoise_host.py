"""CPU: the temporal denoiser exists at every layer -- declared in include/h264mi.h, exported by the library, bound in
Python --, the vectorised reference of the GPU tests (tests/denoiseref.py) equals the definition written as loops, the
sample rule needs no clamp, the identity cases and the gate's threshold hold exactly, the recursion lowers the error of
a noisy constant picture, and h264mi_denoise_ok and h264mi_i420_denoise_dev refuse bad arguments before touching a
device."""
import ctypes

import numpy as np
import pytest

import denoiseref as ref
from test_capi_exports import declared_functions

NEW = ('h264mi_denoise_ok', 'h264mi_i420_denoise_dev', 'h264mi_enc_set_denoise', 'h264mi_enc_denoise')
PARAMS = [(224, 224, 32, 1020), (128, 64, 12, 24), (224, 0, 12, 24), (0, 0, 12, 24), (128, 128, 1, 24), (128, 128, 12, 0)]
SIZES = [(2, 2), (8, 8), (10, 6), (36, 18), (24, 16)]


def make_pair(w, h, seed, reach=12):
    """(cur, prev) of one frame: prev random, cur = prev plus noise in -5..5 clipped; every fourth block (counted row by
    row, from the second) fresh random samples in all planes; in the others one luma sample with a difference of at least reach"""
    rng = np.random.default_rng(seed)
    prev = rng.integers(0, 256, ref.frame_bytes(w, h), dtype=np.uint8)
    cur = np.clip(prev.astype(np.int32) + rng.integers(-5, 6, prev.size), 0, 255).astype(np.uint8)
    C, P = ref.planes(cur, w, h), ref.planes(prev, w, h)
    k = 0
    for by in range((h + 7) // 8):
        for bx in range((w + 7) // 8):
            bw, bh = min(8, w - 8 * bx), min(8, h - 8 * by)
            if k % 4 == 1:
                C[0][8 * by:8 * by + bh, 8 * bx:8 * bx + bw] = rng.integers(0, 256, (bh, bw), dtype=np.uint8)
                for pl in (1, 2):
                    C[pl][4 * by:4 * by + bh // 2, 4 * bx:4 * bx + bw // 2] = rng.integers(0, 256, (bh // 2, bw // 2), dtype=np.uint8)
            else:
                y, x = 8 * by + int(rng.integers(0, bh)), 8 * bx + int(rng.integers(0, bw))
                p = int(P[0][y][x])
                C[0][y][x] = p + reach + 3 if p + reach + 3 <= 255 else p - reach - 3
            k += 1
    return cur, prev


def test_header_declares_library_exports_python_binds(libpath):
    names = declared_functions()
    L = ctypes.CDLL(libpath)
    for n in NEW:
        assert n in names, n
        assert hasattr(L, n), n
    import h264mi
    B = h264mi.lib()
    assert [len(getattr(B, n).argtypes) for n in NEW] == [1, 10, 2, 2]
    assert callable(h264mi.i420_denoise) and callable(h264mi.denoise_ok)
    assert callable(h264mi.BatchEncoder.set_denoise) and callable(h264mi.BatchEncoder.denoise)
    assert ctypes.sizeof(h264mi.Denoise) == 16
    assert [k for k, _ in h264mi.Denoise._fields_] == ['strength_y', 'strength_c', 'reach', 'motion']


@pytest.mark.parametrize('params', PARAMS, ids=[str(p) for p in PARAMS])
def test_vectorised_reference_equals_the_loops(params):
    for w, h in SIZES:
        cur, prev = make_pair(w, h, 7 * w + h)
        a, sa = ref.denoise_frame(cur, prev, w, h, params)
        b, sb = ref.denoise_frame_loops(cur, prev, w, h, params)
        assert np.array_equal(a, b), (w, h)
        assert sa == sb, (w, h, sa, sb)
        assert sa[1] == ((w + 7) // 8) * ((h + 7) // 8)


def test_the_sample_rule_needs_no_clamp():
    """m <= a, and m == 0 when a >= T or K == 0, for every K, T and a: O lies between P and C"""
    a = np.arange(256)[None, None, :]
    K = np.arange(225)[:, None, None]
    T = np.arange(1, 33)[None, :, None]
    k = (K * np.maximum(T - a, 0)) // T
    m = np.where(a < T, (a * k + 128) >> 8, 0)
    assert (m <= a).all()
    assert (m[np.broadcast_to(a >= T, m.shape)] == 0).all() and (m[0] == 0).all()
    assert int(m.max()) <= 31
    for Kv, Tv, av in ((224, 32, 16), (224, 32, 31), (128, 12, 5), (1, 1, 0), (224, 1, 0), (224, 32, 255)):
        assert ref.sample_m(Kv, Tv, av) == int(m[Kv][Tv - 1][av])


def test_identity_cases():
    w, h = 36, 18
    cur, prev = make_pair(w, h, 5)
    for params in PARAMS:
        out, st = ref.denoise_frame(cur, cur, w, h, params)
        assert np.array_equal(out, cur) and st[0] == 0 and st[2] == st[3] == 0
    for params in ((0, 0, 12, 24), (0, 0, 32, 1020), (128, 128, 1, 24), (224, 224, 1, 1020)):
        out, st = ref.denoise_frame(cur, prev, w, h, params)
        assert np.array_equal(out, cur) and st[2] == st[3] == 0, params
    out, st = ref.denoise_frame(cur, prev, w, h, (224, 0, 12, 1020))
    assert np.array_equal(out[w * h:], cur[w * h:]) and not np.array_equal(out[:w * h], cur[:w * h]) and st[3] == 0 < st[2]
    # moving blocks are the current frame in all planes, static ones with strengths on are not
    params = (128, 64, 12, 24)
    out, st = ref.denoise_frame(cur, prev, w, h, params)
    assert 0 < st[0] < st[1]
    O, C, P = ref.planes(out, w, h), ref.planes(cur, w, h), ref.planes(prev, w, h)
    changed = 0
    for by in range((h + 7) // 8):
        for bx in range((w + 7) // 8):
            ys, xs = slice(8 * by, min(8 * by + 8, h)), slice(8 * bx, min(8 * bx + 8, w))
            cys, cxs = slice(4 * by, min(4 * by + 4, h // 2)), slice(4 * bx, min(4 * bx + 4, w // 2))
            sad = int(np.abs(C[0][ys, xs].astype(int) - P[0][ys, xs].astype(int)).sum())
            if 4 * sad > 24 * C[0][ys, xs].size:
                assert np.array_equal(O[0][ys, xs], C[0][ys, xs])
                assert np.array_equal(O[1][cys, cxs], C[1][cys, cxs]) and np.array_equal(O[2][cys, cxs], C[2][cys, cxs])
            else:
                changed += not np.array_equal(O[0][ys, xs], C[0][ys, xs])
    assert changed > 0


def _flat_pair(w, h, sad):
    """a frame pair whose only difference is `sad` levels on luma sample (0, 0)"""
    prev = np.full(ref.frame_bytes(w, h), 100, np.uint8)
    cur = prev.copy()
    cur[0] = 100 + sad
    return cur, prev


def test_the_gate_is_exact():
    for w, h, motion, sad, moving in ((8, 8, 6, 96, 0), (8, 8, 6, 97, 1), (2, 2, 5, 5, 0), (2, 2, 5, 6, 1)):
        cur, prev = _flat_pair(w, h, sad)
        for fn in (ref.denoise_frame, ref.denoise_frame_loops):
            out, st = fn(cur, prev, w, h, (224, 224, 4, motion))
            assert st[:2] == [moving, 1], (w, h, motion, sad)
            assert np.array_equal(out, cur)  # the one difference is above the reach, or the block is moving
    # the same threshold spread over the block: 96 samples' worth of 1 in a whole block, within the reach
    prev = np.full(ref.frame_bytes(8, 8), 100, np.uint8)
    for sad, moving in ((96, 0), (97, 1)):
        cur = prev.copy()
        cur[:64] += 1
        cur[:sad - 64] += 1
        out, st = ref.denoise_frame(cur, prev, 8, 8, (224, 224, 32, 6))
        assert st[0] == moving and (st[2] > 0) == (not moving)


def test_the_recursion_lowers_the_error_of_a_noisy_constant():
    w, h, nf = 24, 16, 8
    rng = np.random.default_rng(11)
    clean = np.full(ref.frame_bytes(w, h), 120, np.float64)
    frames = [np.clip(np.rint(clean + rng.normal(0, 3, clean.size)), 0, 255).astype(np.uint8) for _ in range(nf)]
    outs, stats = ref.denoise_sequence(frames, w, h, (128, 64, 12, 24))
    assert len(outs) == nf and len(stats) == nf - 1 and np.array_equal(outs[0], frames[0])
    mse_in = np.mean([np.mean((f - clean) ** 2) for f in frames])
    mse_out = np.mean([np.mean((o - clean) ** 2) for o in outs])
    assert mse_out < mse_in, (mse_in, mse_out)


GOOD = (128, 64, 12, 24)
BAD_PARAMS = [(-1, 64, 12, 24), (225, 64, 12, 24), (128, -1, 12, 24), (128, 225, 12, 24), (128, 64, 0, 24), (128, 64, 33, 24),
              (128, 64, 12, -1), (128, 64, 12, 1021)]
LIMIT_PARAMS = [(0, 0, 1, 0), (224, 224, 32, 1020), (0, 224, 1, 1020), (224, 0, 32, 0)]
# (w, h, n) that h264mi_i420_denoise_dev must refuse; the pointers are never dereferenced
BAD_SHAPES = [(32, 32, 0), (32, 32, -1), (31, 32, 1), (32, 31, 1), (0, 32, 1), (32, 0, 1), (-2, 32, 1), (8194, 32, 1), (32, 8194, 1)]


def test_denoise_ok_at_the_limits(libpath):
    import h264mi
    B = h264mi.lib()
    for p in LIMIT_PARAMS + PARAMS:
        assert h264mi.denoise_ok(p) == 0 and ref.params_ok(p), p
        assert B.h264mi_denoise_ok(ctypes.byref(h264mi.Denoise(*p))) == 0
    for p in BAD_PARAMS:
        assert h264mi.denoise_ok(p) == -1 and not ref.params_ok(p), p
    assert h264mi.denoise_ok(None) == -1 and B.h264mi_denoise_ok(None) == -1
    assert B.h264mi_enc_set_denoise(None, ctypes.byref(h264mi.Denoise(*GOOD))) == -1 and B.h264mi_enc_denoise(None, None) == -1


def test_denoise_dev_refuses_bad_arguments_without_a_device(libpath):
    import h264mi
    fn = h264mi.lib().h264mi_i420_denoise_dev
    good = ctypes.byref(h264mi.Denoise(*GOOD))
    vp = ctypes.c_void_p
    fb = ref.frame_bytes(32, 16)
    n = 3
    A, Bq, Cq, Dq, St = (0x10000000 + k * 0x100000 for k in range(5))  # dst, dst2, cur, prev, stats: far apart

    def call(dst=A, dst2=Bq, cur=Cq, prev=Dq, stats=St, w=32, h=16, nn=n, p=good):
        return fn(vp(dst) if dst else None, vp(dst2) if dst2 else None, vp(cur) if cur else None, vp(prev) if prev else None,
                  w, h, nn, p, vp(stats) if stats else None, None)

    assert call(dst=0) == -1 and call(cur=0) == -1 and call(prev=0) == -1 and call(p=None) == -1
    for w, h, nn in BAD_SHAPES:
        assert call(w=w, h=h, nn=nn) == -1, (w, h, nn)
    for p in BAD_PARAMS:
        assert call(p=ctypes.byref(h264mi.Denoise(*p))) == -1, p
    for off in (1, 2, 3):
        assert call(stats=St + off) == -1
    assert call(dst2=A) == -1, 'dst == dst2'
    # partial overlaps of every pair: one byte into the other's first byte, last byte, and from below
    for off in (1, n * fb - 1, -1, -(n * fb - 1)):
        assert call(dst=Cq + off) == -1 and call(dst=Dq + off) == -1 and call(dst=Bq + off) == -1
        assert call(dst2=Cq + off) == -1 and call(dst2=Dq + off) == -1
        assert call(cur=Dq + off) == -1
    for off in (0, 4, n * fb - 4, -4, -(16 * n - 4)):  # the statistics against each of the four
        assert call(stats=A + off) == -1 and call(stats=Bq + off) == -1 and call(stats=Cq + off) == -1 and call(stats=Dq + off) == -1
    assert call(dst=Cq, dst2=Cq) == -1 and call(dst=Dq, dst2=Dq) == -1
