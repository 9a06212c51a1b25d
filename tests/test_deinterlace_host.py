"""CPU: the deinterlacer exists at every layer -- declared in include/h264mi.h, exported by the library, bound in Python
--, the library's per-sample host restatement (h264mi_i420_deinterlace_host) equals tests/deintref.py, hand-computed
cases hold, a still clip is woven back bit for bit, a panning clip is better deinterlaced than left woven, the combed
count is a property of the source, and the checks refuse bad arguments before touching a device."""
import ctypes
import functools
import os

import numpy as np
import pytest

import deintref as ref
from test_capi_exports import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('h264mi_deinterlace_ok', 'h264mi_i420_deinterlace_dev', 'h264mi_i420_deinterlace_host', 'h264mi_enc_set_deinterlace',
       'h264mi_enc_deinterlace')
STRIP, ROWS = 256, 16  # csrc/deinterlace.hip: samples across a strip, rows of a row group
# 18x10: chroma rows of 9 bytes, 5 chroma rows; 258x18: one strip + 2; 528x34: two strips + 16; 2x18: a row group + 2 rows
SIZES = [(2, 2), (4, 2), (16, 16), (18, 10), (34, 6), (STRIP + 2, 18), (2 * STRIP + 16, 34), (2, ROWS + 2)]
PARAMS = [(parity, spatial, temporal, 8) for parity in (0, 1) for spatial in (0, 1) for temporal in (0, 1)]
CONTENTS = ('random', 'zeros', 'ones', 'ramp')


@functools.lru_cache(maxsize=None)
def make_pair(w, h, content, seed=0):
    """(cur, prev) of one frame, never written. random: prev random, cur = prev with every third run of 8 bytes fresh,
    every third equal and the others within +-6; ramp: x + y in both, one sample in 16 of cur moved, to force ties"""
    nb = ref.frame_bytes(w, h)
    rng = np.random.default_rng(1000 * seed + 7 * w + h)
    if content == 'zeros':
        cur, prev = np.zeros(nb, np.uint8), np.zeros(nb, np.uint8)
    elif content == 'ones':
        cur, prev = np.full(nb, 255, np.uint8), np.full(nb, 255, np.uint8)
    elif content == 'ramp':
        prev = np.empty(nb, np.uint8)
        for pl in ref.planes(prev, w, h):
            yy, xx = np.mgrid[0:pl.shape[0], 0:pl.shape[1]]
            pl[:] = (xx + yy + seed) % 256
        cur = prev.copy()
        cur[5::16] += 3
    else:
        prev = rng.integers(0, 256, nb, dtype=np.uint8)
        near = np.clip(prev.astype(np.int32) + rng.integers(-6, 7, nb), 0, 255).astype(np.uint8)
        fresh = rng.integers(0, 256, nb, dtype=np.uint8)
        kind = (np.arange(nb) // 8) % 3
        cur = np.where(kind == 0, fresh, np.where(kind == 1, prev, near)).astype(np.uint8)
    cur.setflags(write=False)
    prev.setflags(write=False)
    return cur, prev


def host(cur, prev, w, h, params, in_place=False, stats=True):
    """h264mi_i420_deinterlace_host on one frame: (out, stats or None)"""
    import h264mi
    L = h264mi.lib()
    c = np.array(cur, dtype=np.uint8, copy=True)
    out = c if in_place else np.full(c.size, 0x5A, np.uint8)
    st = np.full(4, 9, np.uint32)
    p = None if prev is None else np.ascontiguousarray(prev)
    r = L.h264mi_i420_deinterlace_host(out.ctypes.data_as(ctypes.c_void_p), c.ctypes.data_as(ctypes.c_void_p),
                                       p.ctypes.data_as(ctypes.c_void_p) if p is not None else None, w, h,
                                       ctypes.byref(h264mi.Deinterlace(*params)), st.ctypes.data_as(ctypes.c_void_p) if stats else None)
    assert r == 0
    return out, [int(v) for v in st] if stats else None


def test_header_declares_library_exports_python_binds(libpath):
    names = declared_functions()
    L = ctypes.CDLL(libpath)
    for n in NEW:
        assert n in names, n
        assert hasattr(L, n), n
    import h264mi
    B = h264mi.lib()
    assert [len(getattr(B, n).argtypes) for n in NEW] == [1, 10, 7, 2, 2]
    assert callable(h264mi.i420_deinterlace) and callable(h264mi.deinterlace_ok)
    assert callable(h264mi.BatchEncoder.set_deinterlace) and callable(h264mi.BatchEncoder.deinterlace)
    assert ctypes.sizeof(h264mi.Deinterlace) == 16
    assert [k for k, _ in h264mi.Deinterlace._fields_] == ['parity', 'spatial', 'temporal', 'comb_level']


@pytest.mark.parametrize('params', PARAMS, ids=[str(p) for p in PARAMS])
def test_library_host_restatement_equals_the_reference(libpath, params):
    for w, h in SIZES:
        for content in CONTENTS:
            cur, prev = make_pair(w, h, content)
            for pv in (prev, None):
                want, want_st = ref.deint_frame(cur, pv, w, h, params)
                got, got_st = host(cur, pv, w, h, params)
                assert np.array_equal(got, want), (w, h, content, pv is None)
                assert got_st == want_st, (w, h, content, got_st, want_st)
                inp, _ = host(cur, pv, w, h, params, in_place=True, stats=False)
                assert np.array_equal(inp, want), (w, h, content, 'in place')
                # kept lines are the source's, and nothing leaves the range between s and v: 0..255 without a clip
                for o, c in zip(ref.planes(want, w, h), ref.planes(cur, w, h)):
                    assert np.array_equal(o[params[0]::2], c[params[0]::2])
            assert want_st[0] == w * (h // 2)


def _luma_frame(rows):
    """a frame whose luma rows are given (chroma 128)"""
    Y = np.array(rows, np.uint8)
    h, w = Y.shape
    return np.concatenate([Y.ravel(), np.full(2 * (w // 2) * (h // 2), 128, np.uint8)]), w, h


def test_hand_computed_cases(libpath):
    # a tie between d = 0 and d = -1 at x = 3 of row 1 (parity 0): score_0 = 10 + 10 + 10, score_-1 = 0 + 20 + 10,
    # score_+1 = 30 + 0 + 20. The tie goes to d = 0: s = (30 + 40 + 1) >> 1 = 35 (d = -1 would give (0 + 20 + 1) >> 1 = 10)
    up, dn = [30, 40, 0, 30, 10, 20, 40, 10], [30, 0, 10, 40, 20, 20, 10, 0]
    f, w, h = _luma_frame([up, [7] * 8, dn, [9] * 8])
    for fn in (lambda p: ref.deint_frame(f, None, w, h, p)[0], lambda p: host(f, None, w, h, p)[0]):
        assert fn((0, 1, 0, 0))[w + 3] == 35
        assert fn((0, 0, 0, 0))[w + 3] == 35  # linear: the same two samples
    # a diagonal edge: up[x + 1 ..] equals dn[x - 1 ..] around x = 3. score_+1 = 0, score_0 = 200, score_-1 = 300:
    # s = (up[4] + dn[2] + 1) >> 1 = 100, where linear gives (0 + 100 + 1) >> 1 = 50
    up, dn = [0, 0, 0, 0, 100, 100, 100, 100], [0, 0, 100, 100, 100, 100, 100, 100]
    f, w, h = _luma_frame([up, [7] * 8, dn, [9] * 8])
    for fn in (lambda p: ref.deint_frame(f, None, w, h, p)[0], lambda p: host(f, None, w, h, p)[0]):
        assert fn((0, 1, 0, 0))[w + 3] == 100 and fn((0, 0, 0, 0))[w + 3] == 50
        # row 3 has one neighbour, row 2: a copy of it, whatever the mode
        assert list(fn((0, 1, 0, 0))[3 * w:4 * w]) == dn and list(fn((0, 0, 0, 0))[3 * w:4 * w]) == dn
        # parity 1: row 0 has one neighbour, row 1; row 2 lies between rows 1 and 3: (7 + 9 + 1) >> 1 = 8
        o = fn((1, 1, 0, 0))
        assert list(o[:w]) == [7] * 8 and list(o[2 * w:3 * w]) == [8] * 8 and list(o[w:2 * w]) == [7] * 8
    # temporal: v = 7 on row 1; P differs from C by 3 at (1, 3) and by 5 at (0, 4), nowhere else. m = 3 at x = 3 and 5
    # at x = 4: O = min(max(s, v - m), v + m) with s = 50 (linear): 10 and 12; every other sample of row 1 is woven: 7
    prev = f.copy()
    prev[w + 3] = 10
    prev[4] = 105
    for fn in (lambda p: ref.deint_frame(f, prev, w, h, p)[0], lambda p: host(f, prev, w, h, p)[0]):
        o = fn((0, 0, 1, 0))
        assert list(o[w:2 * w]) == [7, 7, 7, 10, 12, 7, 7, 7]
    # the one-row chroma plane (h = 2): it is kept (parity 0) or has no kept line (parity 1): unchanged either way
    rng = np.random.default_rng(3)
    f = rng.integers(0, 256, ref.frame_bytes(6, 2), dtype=np.uint8)
    for parity in (0, 1):
        for fn in (lambda p: ref.deint_frame(f, None, 6, 2, p), lambda p: host(f, None, 6, 2, p)):
            o, st = fn((parity, 1, 0, 0))
            assert np.array_equal(o[12:], f[12:]) and st[3] == 0 and st[0] == 6
            kept, miss = (0, 1) if parity == 0 else (1, 0)
            assert np.array_equal(o[6 * miss:6 * miss + 6], f[6 * kept:6 * kept + 6])


def _clip(w, h, T, step):
    """2 T progressive frames of a smooth textured scene that pans `step` samples a frame (0: a still)"""
    yy, xx = np.mgrid[0:h, 0:w]
    fr = []
    for t in range(2 * T):
        X = xx + step * t
        Y = 128 + 50 * np.sin(X / 5.0 + yy / 9.0) + 40 * np.sin(X / 2.3) * np.cos(yy / 6.0) + 25 * np.sin((X + yy) / 3.1)
        U = 128 + 40 * np.sin(X[::2, ::2] / 11.0 + yy[::2, ::2] / 7.0)
        V = 128 + 40 * np.cos(X[::2, ::2] / 8.0 - yy[::2, ::2] / 13.0)
        fr.append(np.concatenate([np.clip(np.rint(p), 0, 255).astype(np.uint8).ravel() for p in (Y, U, V)]))
    return fr


def test_a_still_clip_is_woven_back_bit_for_bit(libpath):
    w, h, T = 64, 48, 4
    g = _clip(w, h, T, 0)
    for parity in (0, 1):
        il = ref.interlace(g, w, h, parity)
        assert all(np.array_equal(f, g[0]) for f in il)
        for spatial in (0, 1):
            outs, stats = ref.deint_sequence(il, w, h, (parity, spatial, 1, 8))
            assert not np.array_equal(outs[0], g[0]), 'frame 0 has no previous frame: spatial only'
            for t in range(1, T):
                assert np.array_equal(outs[t], g[2 * t]), (parity, spatial, t)
                assert stats[t][2] == stats[t][3] == 0
                assert np.array_equal(host(il[t], il[t - 1], w, h, (parity, spatial, 1, 8))[0], g[2 * t])
            assert all(st[1] == 0 and st[0] == w * h // 2 for st in stats), 'a smooth progressive picture has no comb'


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else float(10 * np.log10(65025 / mse))


def test_a_panning_clip_is_better_deinterlaced_than_woven(libpath):
    """PSNR against the progressive frame of the kept field's instant, frames 1.., of the linear, the edge-directed and
    the adaptive output and of the untouched woven input. The one assertion: adaptive > woven. The clip is the first
    one tried (a smooth texture panning 2 samples a field); on it linear is best, since there is no sharp diagonal."""
    w, h, T, step = 64, 48, 6, 2
    g = _clip(w, h, T, step)
    lines = ['# Deinterlacer: PSNR against the progressive source (tests/test_deinterlace_host.py)', '',
             f'{w}x{h}, {T} interlaced frames woven from a double-rate pan of {step} samples a field; mean over frames 1..{T - 1}, all planes.', '',
             '| parity | linear | edge-directed | adaptive (edge, temporal) | woven input |', '|---|---|---|---|---|']
    for parity in (0, 1):
        il = ref.interlace(g, w, h, parity)
        res = {}
        for name, par in (('linear', (parity, 0, 0, 8)), ('edge', (parity, 1, 0, 8)), ('adaptive', (parity, 1, 1, 8))):
            outs, stats = ref.deint_sequence(il, w, h, par)
            res[name] = np.mean([_psnr(outs[t], g[2 * t]) for t in range(1, T)])
            assert np.array_equal(host(il[2], il[1], w, h, par)[0], outs[2])
        res['woven'] = np.mean([_psnr(il[t], g[2 * t]) for t in range(1, T)])
        lines.append(f"| {parity} | {res['linear']:.2f} | {res['edge']:.2f} | {res['adaptive']:.2f} | {res['woven']:.2f} |")
        print(parity, res)
        assert res['adaptive'] > res['woven'], res
        assert stats[2][1] > 0, 'a woven pan has combs'
    try:
        os.makedirs(os.path.join(ROOT, 'profiles', 'deinterlace'), exist_ok=True)
        with open(os.path.join(ROOT, 'profiles', 'deinterlace', 'quality.md'), 'w') as f:
            f.write('\n'.join(lines) + '\n')
    except OSError:
        pass  # a read-only tree: the record is the committed one


def test_the_combed_count_equals_a_hand_count(libpath):
    """8x8, even rows 100, odd rows 200, parity 0, comb_level 20: rows 1, 3, 5 lie between two kept lines 100 below
    them: 24 combed samples; row 7 has one neighbour: none. Then (3, 2) = 100 (v - up = 0): 23; (5, 5) = 121
    (min = 21 > 20) stays, (5, 6) = 120 (min = 20) goes: 22; (1, 0) = 50 (below both by 50): stays. Seen from parity 1
    rows 2, 4, 6 lie 100 below their neighbours but for the three changed samples' columns"""
    Y = np.empty((8, 8), np.uint8)
    Y[0::2], Y[1::2] = 100, 200
    f, w, h = _luma_frame(Y)
    fns = (lambda fr, p: ref.deint_frame(fr, None, w, h, p)[1], lambda fr, p: host(fr, None, w, h, p)[1])
    for fn in fns:
        assert fn(f, (0, 0, 0, 20))[:2] == [32, 24]
        assert fn(f, (0, 1, 1, 99))[:2] == [32, 24] and fn(f, (0, 0, 0, 100))[:2] == [32, 0]
    f = f.copy()
    f[3 * w + 2] = 100
    f[5 * w + 5] = 121
    f[5 * w + 6] = 120
    f[1 * w + 0] = 50
    for fn in fns:
        assert fn(f, (0, 0, 0, 20))[:2] == [32, 22]
        # parity 1: rows 2, 4, 6 (row 0 has one neighbour). (2, 2): up 200, dn 100 -> v - dn = 0: not combed;
        # (2, 0): up 50, dn 200: v = 100 above one, below the other: not; (4, 5), (6, 5): a neighbour 121, min 21: combed;
        # (4, 6), (6, 6): a neighbour 120, min 20: not; (4, 2): up 100: v - up = 0: not. 24 - 5 = 19
        assert fn(f, (1, 0, 0, 20))[:2] == [32, 19]


GOOD = (0, 1, 1, 8)
BAD_PARAMS = [(-1, 1, 1, 8), (2, 1, 1, 8), (0, -1, 1, 8), (0, 2, 1, 8), (0, 1, -1, 8), (0, 1, 2, 8), (0, 1, 1, -1), (0, 1, 1, 256)]
LIMIT_PARAMS = [(0, 0, 0, 0), (1, 1, 1, 255), (0, 1, 0, 255), (1, 0, 1, 0)]
# (w, h, n) that h264mi_i420_deinterlace_dev must refuse; the pointers are never dereferenced
BAD_SHAPES = [(32, 32, 0), (32, 32, -1), (31, 32, 1), (32, 31, 1), (0, 32, 1), (32, 0, 1), (-2, 32, 1), (8194, 32, 1), (32, 8194, 1)]


def test_deinterlace_ok_at_the_limits(libpath):
    import h264mi
    B = h264mi.lib()
    for p in LIMIT_PARAMS + PARAMS:
        assert h264mi.deinterlace_ok(p) == 0 and ref.params_ok(p), p
        assert B.h264mi_deinterlace_ok(ctypes.byref(h264mi.Deinterlace(*p))) == 0
    for p in BAD_PARAMS:
        assert h264mi.deinterlace_ok(p) == -1 and not ref.params_ok(p), p
    assert h264mi.deinterlace_ok(None) == -1 and B.h264mi_deinterlace_ok(None) == -1
    assert B.h264mi_enc_set_deinterlace(None, ctypes.byref(h264mi.Deinterlace(*GOOD))) == -1 and B.h264mi_enc_deinterlace(None, None) == -1
    buf = np.zeros(ref.frame_bytes(4, 4), np.uint8)
    vp = buf.ctypes.data_as(ctypes.c_void_p)
    good = ctypes.byref(h264mi.Deinterlace(*GOOD))
    fn = B.h264mi_i420_deinterlace_host
    assert fn(None, vp, None, 4, 4, good, None) == -1 and fn(vp, None, None, 4, 4, good, None) == -1 and fn(vp, vp, None, 4, 4, None, None) == -1
    assert fn(vp, vp, None, 3, 4, good, None) == -1 and fn(vp, vp, None, 4, 8194, good, None) == -1
    assert fn(vp, vp, None, 4, 4, ctypes.byref(h264mi.Deinterlace(2, 0, 0, 0)), None) == -1


def test_deinterlace_dev_refuses_bad_arguments_without_a_device(libpath):
    import h264mi
    fn = h264mi.lib().h264mi_i420_deinterlace_dev
    good = ctypes.byref(h264mi.Deinterlace(*GOOD))
    vp = ctypes.c_void_p
    fb = ref.frame_bytes(32, 16)
    n = 3
    A, Bq, Cq, Dq, St = (0x10000000 + k * 0x100000 for k in range(5))  # dst, prev_out, cur, prev, stats: far apart

    def call(dst=A, prev_out=Bq, cur=Cq, prev=Dq, stats=St, w=32, h=16, nn=n, p=good):
        return fn(vp(dst) if dst else None, vp(prev_out) if prev_out else None, vp(cur) if cur else None, vp(prev) if prev else None,
                  w, h, nn, p, vp(stats) if stats else None, None)

    assert call(dst=0) == -1 and call(cur=0) == -1 and call(p=None) == -1
    for w, h, nn in BAD_SHAPES:
        assert call(w=w, h=h, nn=nn) == -1, (w, h, nn)
    for p in BAD_PARAMS:
        assert call(p=ctypes.byref(h264mi.Deinterlace(*p))) == -1, p
    for off in (1, 2, 3):
        assert call(stats=St + off) == -1
    assert call(prev_out=A) == -1, 'dst == prev_out'
    assert call(dst=Dq) == -1, 'dst == prev'
    assert call(prev_out=Cq) == -1, 'prev_out == cur'
    # partial overlaps of a written range with any other: one byte into its first byte, its last byte, and from below
    for off in (1, n * fb - 1, -1, -(n * fb - 1)):
        assert call(dst=Cq + off) == -1 and call(dst=Dq + off) == -1 and call(dst=Bq + off) == -1
        assert call(prev_out=Cq + off) == -1 and call(prev_out=Dq + off) == -1
        # the read ranges may overlap -- a clip in one buffer -- only while neither is written
        assert call(dst=Cq, cur=Cq, prev=Cq + off) == -1 and call(prev_out=Dq, cur=Dq + off) == -1
    for off in (0, 4, n * fb - 4, -4, -(16 * n - 4)):  # the statistics against each of the four
        assert call(stats=A + off) == -1 and call(stats=Bq + off) == -1 and call(stats=Cq + off) == -1 and call(stats=Dq + off) == -1
