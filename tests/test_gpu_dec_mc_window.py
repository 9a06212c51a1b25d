"""GPU: the decoder's luma prediction from its one reference window (csrc/dec_recon.inc: mb_in_window, dec_luma_frac)
against tests/reconref.py + tests/dbkref.py, as tests/test_gpu_recon_reference.py does: byte equality of whole pictures
with pictures derived from syntax elements alone, after the host check that this chain equals the oracle's pictures
(Analysis.chain_bad is None) for these very streams.

The decoder keeps the integer reference plane G only; a row wave holds columns and rows [DWIN_LO, DWIN_HI) = [-24, 40)
of it around each macroblock in a 64-column LDS ring (chroma [DWINC_LO, DWINC_HI) = [-12, 20)), runs the six-tap
filters of 8.4.2.2.1 over that window where a vector is fractional, and sends a macroblock with a block whose reads
leave the window to the interpolation from the picture in HBM. What the streams here pin, made with tests/streamgen.py
(scripted mvd, planned with reconref's own predictor so that the *absolute* vectors are the intended ones -- asserted
on the host from reconref's derived vectors, not assumed):

* window boundary: 48x48 (3x3 macroblocks: first, middle and last column and row, so the window lies in the picture's
  padding), P_L0_16x16 everywhere with one vector per picture. For each direction and each fractional part (0,0),
  (2,0), (0,2), (2,2) and (3,2) -- the last reads j and h at x + 1 -- one picture at the last integer displacement the
  window admits and one a sample beyond it. in_window() below restates mb_in_window's rule from the constants read out
  of the kernel source; for a 16x16 partition it gives, per direction,
      component with a fractional part:  displacement in [-22, 21]  (the taps reach 2 before, 3 after: -24 .. 39)
      whole-sample component:            displacement in [-24, 23]  (far side: the chroma window binds, its bilinear
                                                                    form reads the sample after the block's last)
  and the test asserts those values, so a change of the constants or of the rule shows here first.
* mixed classes: P_8x8 of four 4x4 sub-blocks whose sixteen blocks take the sixteen fractional positions at once, in
  every rotation; macroblocks that need only b, only h, only j, b and h without j; macroblocks with sixteen different
  whole-sample vectors between them (the one-read path after the filter path, the ring having slid).
* ring wrap: 96x48 (6 macroblock columns over a 64-column ring), every macroblock with fractional vectors pointing left
  and right up to the admitted extremes -22 and 21.
* batch path: the same streams through BatchDecoder, two streams of different content per call, two pictures per call.

Most P pictures are non-reference pictures (nal_ref_idc 0): every one predicts from the textured IDR picture instead of
from a picture that twenty shifts by 24 samples have smeared flat. The last picture of each stream is a reference
picture predicted from, so the planes are rebuilt after a P picture too. streamgen emits every element needed."""
import functools
import os
import re

import numpy as np
import pytest

import dbkref
import reconref
from test_dbk_reference import _gen, planes_of
from test_gpu_decoder import gpu_decode
from test_recon_reference import Analysis, _nal_ref_idc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def window_constants():
    src = open(os.path.join(ROOT, 'openh264-wasm_amd', 'csrc', 'dec_recon.inc')).read()
    c = {k: int(v) for k, v in re.findall(r'\b(DWINC?_(?:LO|HI)) = (-?\d+)', src)}
    assert set(c) == {'DWIN_LO', 'DWIN_HI', 'DWINC_LO', 'DWINC_HI'}, c
    return c


def in_window(mvs):
    """mb_in_window of dec_recon.inc for the 16 block vectors (raster, quarter samples) of one macroblock"""
    c = window_constants()
    for b, (mx, my) in enumerate(mvs):
        for p, m in ((b & 3, mx), (b >> 2, my)):
            f = (m & 3) != 0
            lo, hi = 4 * p + (m >> 2) - (2 if f else 0), 4 * p + (m >> 2) + 3 + (3 if f else 0)   # luma reads lo .. hi
            clo, chi = 2 * p + (m >> 3), 2 * p + (m >> 3) + 2                                     # chroma reads clo .. chi
            if not (lo >= c['DWIN_LO'] and hi < c['DWIN_HI'] and clo >= c['DWINC_LO'] and chi < c['DWINC_HI']):
                return False
    return True


def extreme(sign, frac):
    """the largest displacement |d| in direction sign that the window admits for a 16x16 vector component 4 d + frac"""
    d = 0
    while in_window([(4 * (d + sign) + frac, 0)] * 16):
        d += sign
    return d


# ---------------------------------------------------------------------------------------------------------------
# planning: absolute vectors -> mvd, with reconref's predictor over the vectors planned so far (one slice)

P4 = [(8 * (q & 1) + xx, 8 * (q >> 1) + yy) for q in range(4) for yy in (0, 4) for xx in (0, 4)]   # 4x4 blocks, parse order


def plan(mbw, mbh, want):
    """want[addr] = [one vector] (P_L0_16x16) or [16 vectors, raster] (P_8x8, four 4x4 sub-blocks) -> SyntaxGen script"""
    pic = reconref._Picture(mbw, mbh)
    script = {}
    for addr in range(mbw * mbh):
        mvs = want[addr]
        gx, gy = 4 * (addr % mbw), 4 * (addr // mbw)
        parts = [(0, 0, 16, 16)] if len(mvs) == 1 else [(x, y, 4, 4) for x, y in P4]
        mvd = []
        for x, y, w, h in parts:
            mv = mvs[0] if len(mvs) == 1 else mvs[(y // 4) * 4 + x // 4]
            mvp, _ = reconref._mvp(pic, addr, x, y, w, h, None, 0)
            mvd.append((mv[0] - mvp[0], mv[1] - mvp[1]))
            g = (slice(gy + y // 4, gy + (y + h) // 4), slice(gx + x // 4, gx + (x + w) // 4))
            pic.mv[g], pic.ref[g], pic.derived[g] = mv, 0, True
        reconref._finish_mb(pic, addr, intra=False)
        script[addr] = dict(kind='p16', subs=None, mvd=mvd) if len(mvs) == 1 else dict(kind='p8x8', subs=[3] * 4, mvd=mvd)
    return script


FRACS = [(0, 0), (2, 0), (0, 2), (2, 2), (3, 2)]
DIRS = {'left': (0, -1), 'right': (0, 1), 'up': (1, -1), 'down': (1, 1)}   # axis, sign


def boundary_pictures(direction):
    """[(vector, expected in-window)] : per fractional part the picture at the window's last displacement and one beyond"""
    axis, sign = DIRS[direction]
    out = []
    for f in FRACS:
        at = extreme(sign, f[axis])
        for d, inside in ((at, True), (at + sign, False)):
            v = [f[0], f[1]]
            v[axis] += 4 * d
            out.append((tuple(v), inside))
    return out


def _boundary(direction, seed):
    def build(oracle):
        g = _gen(3, 3, seed, init_qp=28)
        units = [g.idr()]
        pics = boundary_pictures(direction)
        for k, (v, _) in enumerate(pics):
            last = k == len(pics) - 1
            units.append(g.p(script=plan(3, 3, {a: [v] for a in range(9)}), cbp_fixed=0 if k % 3 else None, ref_idc=2 if last else 0))
        units.append(g.p(script=plan(3, 3, {a: [(6, -5)] for a in range(9)})))   # predicted from the last P picture
        return units, (48, 48)
    return build


ALL16 = list(range(16))
ONLY_B, ONLY_H, ONLY_J, B_AND_H = [0, 1, 2, 3], [0, 4, 8, 12], [0, 10], [5, 7, 13, 15, 0]


def _mb(rng, positions, rot, dmax=3):
    """16 block vectors: block b at fractional position positions[(b + rot) % n] (yFrac * 4 + xFrac), small displacement"""
    out = []
    for b in range(16):
        p = positions[(b + rot) % len(positions)]
        out.append((4 * int(rng.integers(-dmax, dmax + 1)) + (p & 3), 4 * int(rng.integers(-dmax, dmax + 1)) + (p >> 2)))
    return out


def _mixed(seed):
    def build(oracle):
        g = _gen(3, 3, seed, init_qp=30)
        rng = np.random.default_rng(seed)
        whole = lambda: _mb(rng, [0], 0, dmax=5)
        pics = [
            # all sixteen positions in every macroblock but the whole-sample ones in the middle of rows 1 and 2
            [_mb(rng, ALL16, a) for a in range(4)] + [whole()] + [_mb(rng, ALL16, 5 + a) for a in range(2)] + [whole(), _mb(rng, ALL16, 11)],
            # one filter at a time, then pairs; a 16x16 whole-sample and a 16x16 j macroblock between
            [_mb(rng, ONLY_B, 0), _mb(rng, ONLY_H, 1), _mb(rng, ONLY_J, 0), _mb(rng, B_AND_H, 2), [(8, -12)], _mb(rng, ALL16, 3),
             [(4 * 2 + 2, 4 * -1 + 2)], whole(), _mb(rng, ONLY_J, 1)],
        ]
        units = [g.idr()]
        for k, p in enumerate(pics):
            units.append(g.p(script=plan(3, 3, dict(enumerate(p))), cbp_fixed=0 if k == 0 else None, ref_idc=0 if k == 0 else 2))
        units.append(g.p(script=plan(3, 3, {a: _mb(rng, ALL16, a) for a in range(9)})))
        return units, (48, 48)
    return build


def _wrap(seed):
    def build(oracle):
        g = _gen(6, 3, seed, init_qp=30)
        rng = np.random.default_rng(seed)
        lo, hi = extreme(-1, 1), extreme(1, 1)   # fractional components: -22, 21

        def mb(a):
            out = []
            for b in range(16):
                left = not (b + a) & 1
                d = (lo if b == (a % 16) else int(rng.integers(lo, lo + 8))) if left else (hi if b == ((a + 1) % 16) else int(rng.integers(hi - 7, hi + 1)))
                p = (3 * b + a) % 15 + 1   # never 0: every block fractional
                fx = (p & 3) or 2          # the horizontal component fractional too (the taps reach the window's columns)
                out.append((4 * d + fx, 4 * int(rng.integers(-2, 3)) + (p >> 2)))
            return out
        units = [g.idr()]
        for k in range(2):
            units.append(g.p(script=plan(6, 3, {a: mb(a + k) for a in range(18)}), cbp_fixed=None if k else 0))
        return units, (96, 48)
    return build


BUILD = {f'bound_{d}_48x48': _boundary(d, 170 + k) for k, d in enumerate(DIRS)}
BUILD.update({'mixed_48x48_a': _mixed(181), 'mixed_48x48_b': _mixed(182), 'wrap_96x48_a': _wrap(191), 'wrap_96x48_b': _wrap(192)})
BATCH_PAIRS = [('bound_left_48x48', 'bound_down_48x48'), ('bound_right_48x48', 'bound_up_48x48'), ('mixed_48x48_a', 'mixed_48x48_b'),
               ('wrap_96x48_a', 'wrap_96x48_b')]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(units, (w, h), the chain's picture per unit, per picture the 16 derived vectors of every macroblock), once"""
    a = Analysis(name, build=BUILD[name])
    assert a.chain_bad is None and a.stage_bad is None and a.record_bad is None, (name, a.chain_bad, a.stage_bad, a.record_bad)
    w, h = a.size
    vectors, prev = [], None
    for k, u in enumerate(a.units):
        res = reconref.reconstruct(a.syntax[k], a.geometry, prev)
        vectors.append([[(int(r[22 + 2 * b]), int(r[23 + 2 * b])) for b in range(16)] if int(r[0]) in (2, 3, 4, 5, 6) else None
                        for r in res.records])
        if _nal_ref_idc(u):
            prev = planes_of(a.chain[k][0], w, h)
    return a.units, a.size, [c[0] for c in a.chain], vectors


def _explain(name, k, got):
    units, (w, h), _, _ = reference(name)
    a = Analysis(name, build=BUILD[name])
    prev = None
    for j in range(k + 1):
        res = reconref.reconstruct(a.syntax[j], a.geometry, prev)
        out = dbkref.deblock(res.planes, res.records, explain=(j == k))
        if _nal_ref_idc(units[j]):
            prev = out.planes
    gp = planes_of(got, w, h)
    msg = dbkref.first_difference(out, gp, w, h)
    for pl, (r, g) in enumerate(zip(out.planes, gp)):
        ne = np.argwhere(r != np.asarray(g))
        if len(ne):
            return f'{msg} || {" | ".join(res.explain(pl, int(ne[0][1]), int(ne[0][0])))}'
    return msg


def _require_equal(name, k, ref, got, what):
    if not np.array_equal(ref, got):
        pytest.fail(f'{what}, picture {k}: ' + _explain(name, k, got))


# ---------------------------------------------------------------------------------------------------------------
# the streams hold what they are for (host side, from reconref's derived vectors)


def test_window_bounds_follow_the_kernel_constants():
    assert window_constants() == {'DWIN_LO': -24, 'DWIN_HI': 40, 'DWINC_LO': -12, 'DWINC_HI': 20}
    assert [extreme(-1, f) for f in (0, 1, 2, 3)] == [-24, -22, -22, -22]
    assert [extreme(1, f) for f in (0, 1, 2, 3)] == [23, 21, 21, 21]


@pytest.mark.parametrize('direction', list(DIRS))
def test_boundary_streams_hold_both_sides(direction):
    _, _, _, vectors = reference(f'bound_{direction}_48x48')
    for k, (v, inside) in enumerate(boundary_pictures(direction)):
        for mb in vectors[1 + k]:
            assert mb == [v] * 16, (k, v, mb)              # every macroblock, first and last column and row included
            assert in_window(mb) == inside, (k, v)


@pytest.mark.parametrize('name', ['mixed_48x48_a', 'mixed_48x48_b'])
def test_mixed_streams_hold_the_classes(name):
    _, _, _, vectors = reference(name)
    pos = lambda mb: {(my & 3) * 4 + (mx & 3) for mx, my in mb}
    for pic in vectors[1:]:
        assert all(mb is not None and in_window(mb) for mb in pic)
    p1, p2 = vectors[1], vectors[2]
    assert sum(pos(mb) == set(range(16)) for mb in p1) == 7 and pos(p1[4]) == pos(p1[7]) == {0}
    assert len(set(p1[4])) > 8                             # whole-sample vectors that differ from block to block
    assert pos(p1[3]) == pos(p1[5]) == set(range(16))      # the one-read path between two filter macroblocks of a row
    assert [pos(mb) for mb in p2[:4]] == [set(ONLY_B), set(ONLY_H), set(ONLY_J), set(B_AND_H)]


@pytest.mark.parametrize('name', ['wrap_96x48_a', 'wrap_96x48_b'])
def test_wrap_streams_point_both_ways_in_every_column(name):
    _, (w, _), _, vectors = reference(name)
    assert w // 16 >= 5
    lo, hi = extreme(-1, 1), extreme(1, 1)
    for pic in vectors[1:]:
        for mb in pic:
            assert in_window(mb) and all(mx & 3 for mx, _ in mb)
            d = [mx >> 2 for mx, _ in mb]
            assert min(d) == lo and max(d) == hi, d        # both admitted extremes in every macroblock


# ---------------------------------------------------------------------------------------------------------------
# the GPU


@pytest.mark.parametrize('name', list(BUILD))
def test_decoder_window_paths_vs_clauses(gpu_lib, name):
    units, (w, h), refs, _ = reference(name)
    L = gpu_lib
    assert L.init_decoder(12) == 0
    try:
        for k, u in enumerate(units):
            gw, gh, got = gpu_decode(L, 12, u, w, h)
            assert (gw, gh) == (w, h), f'{name} picture {k}: {gw}x{gh}'
            _require_equal(name, k, refs[k], got, f'{name} through decode_frame_yuv_i420')
    finally:
        L.deinit_decoder(12)


@pytest.mark.parametrize('names', BATCH_PAIRS, ids=['+'.join(p) for p in BATCH_PAIRS])
def test_batch_decoder_two_streams(gpu_lib, names):
    """two streams of different content in one batch, two pictures per call after the IDR: a stream index slipping in the
    window addressing would predict one stream from the other's plane"""
    import torch
    import h264mi
    refs = [reference(n) for n in names]
    (w, h) = refs[0][1]
    n = min(len(r[0]) for r in refs)
    assert refs[1][1] == (w, h) and n >= 3
    dec = h264mi.BatchDecoder(w, h, 2, max_frames=2)
    try:
        dev = [[torch.from_numpy(np.frombuffer(u, np.uint8).copy()).cuda() for u in r[0][:n]] for r in refs]
        calls = [[0]] + [list(range(k, min(k + 2, n))) for k in range(1, n, 2)]
        for call in calls:
            ptrs = [dev[s][k].data_ptr() for k in call for s in range(2)]          # nal_ptrs[f * S + s]
            sizes = [len(refs[s][0][k]) for k in call for s in range(2)]
            dec.decode_frames(ptrs, nal_sizes=sizes)
            rc, got = dec.status()
            assert rc == 0 and got == [1, 1], (call, rc, got)
            for s in range(2):
                pic = np.frombuffer(dec.picture_i420(s), np.uint8)
                _require_equal(names[s], call[-1], refs[s][2][call[-1]], pic, f'{names[s]} as stream {s} of a batch of two')
    finally:
        dec.close()
