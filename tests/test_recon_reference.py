"""CPU: reconstruction (intra prediction, motion vector prediction, interpolation, scaling and transform, the QP
chain) against an independent reference of clauses 8.3-8.5, tests/reconref.py, and an audit of which branches of
those clauses the suite's streams reach.

The oracle decoder (oracle/h264o_dec.c, h264o_common.c) and the product's kernels are restatements by one hand, so
"GPU picture == oracle picture" cannot see a shared misreading. Here the oracle hands over only what it *parsed*
(h264o_dec_syntax: syntax elements, nothing derived), reconref derives the vectors, modes, QPs and samples from the
standard's text, and
  * stage check: reconref(oracle syntax, oracle's previous output) == the oracle's picture before its loop filter,
    and the derived records == h264o_dec_records;
  * chain check: with dbkref (clause 8.7) behind it, whole pictures follow from syntax elements alone -- no sample
    passes through the oracle's reconstruction -- and equal the oracle's output pictures. This chain is what
    tests/test_gpu_recon_reference.py compares the GPU against;
  * parse round trip: the hook's syntax == what the stream generator wrote, which pins the oracle's CAVLC parse.

`python tests/test_recon_reference.py` prints the audit table of DESIGN.md (class by hits, per stream family)."""
import functools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, 'oracle', 'build', 'libh264_oracle.so')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'openh264-wasm_amd'))

import dbkref  # noqa: E402
import reconref  # noqa: E402
import test_dbk_reference as tdr  # noqa: E402
from test_dbk_reference import _gen, _oracle_table, planes_of  # noqa: E402

CSRC = os.path.join(ROOT, 'openh264-wasm_amd', 'csrc')


# ---------------------------------------------------------------------------------------------------------------
# tables


def test_tables_match_the_oracle(oracle):
    """the zig-zag, normAdjust v, Table 9-4 and the block order as typed in reconref.py == the oracle's copies"""
    assert _oracle_table(oracle, 'zigzag4', 16) == [4 * y + x for x, y in reconref.ZIGZAG_XY]
    assert _oracle_table(oracle, 'dequant_v', 18) == [v for row in reconref.V for v in row]
    assert _oracle_table(oracle, 'pos_class', 16) == [reconref._pos_class(k % 4, k // 4) for k in range(16)]
    assert _oracle_table(oracle, 'cbp_intra', 48) == [a for a, _ in reconref.CBP_TABLE]
    assert _oracle_table(oracle, 'cbp_inter', 48) == [b for _, b in reconref.CBP_TABLE]
    assert _oracle_table(oracle, 'blk2ras', 16) == [(y // 4) * 4 + x // 4 for x, y in reconref.BLK_XY]
    assert _oracle_table(oracle, 'chroma_qp', 52) == reconref.QPC


def test_table_structure():
    """what the tables guarantee by construction: the scan and Table 9-4 are permutations, v grows with qP % 6"""
    assert sorted(reconref.ZIGZAG_XY) == [(x, y) for x in range(4) for y in range(4)]
    assert sorted(a for a, _ in reconref.CBP_TABLE) == sorted(b for _, b in reconref.CBP_TABLE) == list(range(48))
    assert all(a < b for col in zip(*reconref.V) for a, b in zip(col, col[1:]))
    assert sorted(reconref.BLK_XY) == [(x, y) for x in range(0, 16, 4) for y in range(0, 16, 4)]


def _rows(src, name, width):
    """the initialiser of the array `name` in C source, rows padded with zeros to width as C does"""
    m = re.search(r'\b' + name + r'(?:\[\d+\])+\s*=\s*\{(.*?)\};', src, re.S)
    assert m, name
    body = re.sub(r'/\*.*?\*/|//[^\n]*', '', m.group(1), flags=re.S)
    rows = re.findall(r'\{([^{}]*)\}', body) or [body]
    out = []
    for r in rows:
        v = [int(x) for x in re.findall(r'\d+', r)]
        assert len(v) <= width, name
        out += v + [0] * (width - len(v))
    return out


def _csrc(fn):
    return open(os.path.join(CSRC, fn)).read()


def test_tables_match_the_kernel_source():
    """every copy of these tables the kernels hold, by name, == the typed table in the direction that copy holds: the
    zig-zag as scan -> raster (ZZ) and raster -> scan (INVZZ, XF_INVZZ), v (c_V), Table 8-15 (c_CHROMA_QP, QPC) and
    Table 9-4 codeNum -> pattern (both pairs of enc_bits.inc, CBP_INTRA / CBP_INTER of vlc_tables.inc)"""
    zig = [4 * y + x for x, y in reconref.ZIGZAG_XY]
    inv_zig = [zig.index(k) for k in range(16)]
    intra, inter = [a for a, _ in reconref.CBP_TABLE], [b for _, b in reconref.CBP_TABLE]
    dev, mb, bits, vlc = _csrc('h264mi_dev.h'), _csrc('enc_mb.inc'), _csrc('enc_bits.inc'), _csrc('vlc_tables.inc')
    assert _rows(dev, 'ZZ', 16) == zig
    assert _rows(mb, 'INVZZ', 16) == inv_zig
    assert _rows(dev, 'XF_INVZZ', 16) == inv_zig
    assert _rows(dev, 'c_V', 3) == [v for row in reconref.V for v in row]
    assert _rows(dev, 'c_CHROMA_QP', 52) == reconref.QPC
    assert _rows(vlc, 'QPC', 52) == reconref.QPC
    for src, ni, ne in ((bits, 'CBP_INTRA_FROM_CODE', 'CBP_INTER_FROM_CODE'), (bits, 'c_CBP_INTRA_FROM_CODE', 'c_CBP_INTER_FROM_CODE'),
                        (vlc, 'CBP_INTRA', 'CBP_INTER')):
        assert _rows(src, ni, 48) == intra, ni
        assert _rows(src, ne, 48) == inter, ne


# ---------------------------------------------------------------------------------------------------------------
# streams


def _long_vectors(mbw, mbh, seed, sid=3, br=400000, nf=4):
    """streamgen.p_frame on an IDR picture of the oracle encoder: P_L0_16x16 without residual and P_Skip runs, mvd up to
    +-96 quarter samples in several P pictures so that the predicted vectors accumulate far beyond +-16 samples"""
    def build(oracle):
        from h264mi.synth import SyntheticStream
        from streamgen import p_frame
        w, h = 16 * mbw, 16 * mbh
        idr = oracle.encoder(w, h, br).encode(np.ascontiguousarray(SyntheticStream(sid, w, h).frame(0)))
        rng = np.random.default_rng(seed)
        return [idr] + [p_frame(mbw, mbh, t, 2 * t, rng, max_mvd=96) for t in range(1, nf + 1)], (w, h)
    return build


LONG = {'long_48x48': _long_vectors(3, 3, 96, br=100000, nf=5), 'long_176x144': _long_vectors(11, 9, 97)}

# ---- directed streams. The audit found CASES + MULTI + the long-vector streams to reach every class already, so these
# close no gap of the list: they hold the cases by construction (scripted mvd, sub types and neighbourhoods, QP chains
# across slices) rather than by the luck of a seed, on the small pictures the GPU module runs.


def _mv_script(mbw, mbh, rng, sizes):
    """every macroblock inter, of the partition shapes in `sizes`, mvd drawn so that all 16 fractional positions occur"""
    s = {}
    for a in range(mbw * mbh):
        kind = sizes[a % len(sizes)]
        s[a] = dict(kind=kind[0], subs=kind[1], mvd=[(int(rng.integers(-9, 10)), int(rng.integers(-9, 10))) for _ in range(16)])
    return s


def _d_fractions(oracle):
    """48x48, P pictures whose macroblocks cycle through P_L0_16x16, 16x8, 8x16 and P_8x8 with each sub_mb_type alone:
    every (xFrac, yFrac) at every partition size, with and without residual"""
    g = _gen(3, 3, 61, init_qp=30)
    rng = np.random.default_rng(61)
    sizes = [('p16', None), ('p16x8', None), ('p8x16', None), ('p8x8', [0] * 4), ('p8x8', [1] * 4), ('p8x8', [2] * 4), ('p8x8', [3] * 4)]
    units = [g.idr()]
    for k in range(5):
        units.append(g.p(script=_mv_script(3, 3, rng, sizes[k:] + sizes[:k]), cbp_fixed=0 if k % 2 else None))
    return units, (48, 48)


def _d_predictors(oracle):
    """48x48 and slices: scripted neighbourhoods for 8.4.1.3 -- an inter macroblock among intra ones (exactly one
    neighbour with the reference), P_Skip beside zero-vector and non-zero-vector neighbours, 16x8 / 8x16 beside intra"""
    g = _gen(3, 3, 62, init_qp=28)
    P = lambda mvd: dict(kind='p16', subs=None, mvd=[mvd] * 16)
    I = dict(kind='i16')
    S = dict(kind='skip')
    X = lambda k: dict(kind=k, subs=None, mvd=[(5, -3), (-6, 2)] * 8)
    pics = [
        # only A inter / only B inter / only C inter around the centre, then directional misses beside intra
        {0: I, 1: I, 2: I, 3: P((4, 4)), 4: P((1, 1)), 5: I, 6: I, 7: I, 8: I},
        {0: I, 1: P((4, 4)), 2: I, 3: I, 4: P((1, 1)), 5: I, 6: I, 7: I, 8: I},
        {0: I, 1: I, 2: P((4, 4)), 3: I, 4: P((1, 1)), 5: X('p16x8'), 6: I, 7: X('p8x16'), 8: X('p16x8')},
        # P_Skip: zero by a zero-vector A, by a zero-vector B, predicted
        {0: P((0, 0)), 1: P((3, 2)), 2: P((3, 2)), 3: P((0, 0)), 4: S, 5: S, 6: P((2, 2)), 7: S, 8: S},
        {0: P((3, 1)), 1: P((0, 0)), 2: P((0, 0)), 3: P((3, 1)), 4: S, 5: S, 6: I, 7: X('p8x16'), 8: X('p8x16')},
        {0: P((3, 1)), 1: P((2, 5)), 2: P((7, 0)), 3: P((3, 1)), 4: S, 5: S, 6: S, 7: S, 8: S},
    ]
    return [g.idr()] + [g.p(script=s, cbp_fixed=0) for s in pics], (48, 48)


def _d_qp(oracle):
    """80x48, slices starting mid-row: mb_qp_delta after P_Skip runs, after I_PCM, after coded_block_pattern 0
    macroblocks and at a slice start; low and high QPs with chroma offsets that clip qPI"""
    out = []
    for seed, iqp, cqp in ((63, 3, -12), (64, 49, 12), (65, 9, 0)):
        g = _gen(5, 3, seed, init_qp=iqp, cqp=cqp)
        lay = [dict(first=0), dict(first=3, qp_delta=2), dict(first=7, qp_delta=-2), dict(first=11)]
        if out:
            g.idr_id = len(out)
        out += [g.idr(slices=lay), g.p(slices=lay, mix={'skip': 3, 'p16': 3, 'pcm': 1, 'i16': 2, 'p8x8': 1, 'i4': 2}), g.p(slices=lay)]
    return out, (80, 48)


def _d_intra_edges(mbw, mbh, seed):
    def build(oracle):
        g = _gen(mbw, mbh, seed, init_qp=22)
        lay = [dict(first=0)] + ([dict(first=mbw * mbh // 2)] if mbw * mbh > 2 else [])
        return [g.idr(slices=lay), g.p(mix={'i4': 3, 'i16': 2, 'p16': 1, 'pcm': 0.5}, slices=lay), g.idr(slices=lay)], (16 * mbw, 16 * mbh)
    return build


def _d_clip(oracle):
    """48x48 at QP 30: I_PCM macroblocks near 0 and near 255 beside inter and intra macroblocks with large levels --
    Clip1 of 8-354 saturates at both ends after either kind of prediction"""
    g = _gen(3, 3, 66, init_qp=30)
    rng = np.random.default_rng(66)
    g.mag_choice = [3, 5, 8]
    script = {a: dict(kind='pcm', samples=tdr._pcm(rng, 255 if a & 2 else 0, 3)) for a in (0, 2, 4, 6, 8)}
    units = [g.idr(script=script, mix={'i4': 1, 'i16': 1})]
    units += [g.p(mix={'p16': 2, 'p8x8': 1, 'i4': 1, 'i16': 1}, max_mvd=4) for _ in range(2)]
    return units, (48, 48)


RECON_DIRECTED = {
    'fractions_48x48': _d_fractions,
    'predictors_48x48': _d_predictors,
    'qp_80x48': _d_qp,
    'clip_48x48': _d_clip,
    'intra_16x16': _d_intra_edges(1, 1, 67),
    'intra_16x48': _d_intra_edges(1, 3, 68),
    'intra_48x16': _d_intra_edges(3, 1, 69),
}

# ---- encoder content with sub-sample motion. SyntheticStream moves by whole samples, so the encoder's vectors on it sit
# at the quarter positions its refinement drifts to and never at a half-sample position (xFrac or yFrac 2): b, h and j
# would enter no prediction themselves, j none at all. Here the window into the same textures moves by quarter samples
# (bilinear between the four integer neighbours), a different step before every P picture, so the motion search ends on
# the half-sample positions.
ENC_STREAM_IDS = (0, 1, 3)
ENC_MOTION = {0: [(2, 0), (0, 2), (2, 2)], 1: [(2, 1), (1, 2), (2, 3)], 3: [(3, 2), (-2, 0), (0, -2)]}   # quarter samples per P picture
ENC_CASES = [(48, 48, 60000), (80, 48, 100000), (176, 144, 300000)]
# what each encoder stream must hold at every size, one slice (measured with reconref's counters on the oracle encoder,
# whose one-slice streams the GPU encoder's equal): the luma positions with a half-sample component
ENC_REQUIRED = {0: [(2, 0), (0, 2), (2, 2)], 1: [(2, 1), (1, 2), (2, 3)], 3: [(3, 2), (2, 0), (0, 2)]}


def _window(tex, qx, qy, w, h):
    ix, fx, iy, fy = qx >> 2, qx & 3, qy >> 2, qy & 3
    a = tex[iy:iy + h + 1, ix:ix + w + 1].astype(np.int32)
    top = (4 - fx) * a[:-1, :-1] + fx * a[:-1, 1:]
    bot = (4 - fx) * a[1:, :-1] + fx * a[1:, 1:]
    return (((4 - fy) * top + fy * bot + 8) >> 4).astype(np.uint8)


def subsample_frames(sid, w, h):
    """the four I420 frames of encoder stream sid: SyntheticStream sid's textures through a window that starts at (4, 4)
    and moves by ENC_MOTION[sid] quarter luma samples before each P picture (chroma: half of the luma offset)"""
    from h264mi.synth import SyntheticStream
    g = SyntheticStream(sid, w, h)
    qx = qy = 16
    out = []
    for dx, dy in [(0, 0)] + ENC_MOTION[sid]:
        qx, qy = qx + dx, qy + dy
        out.append(np.concatenate([_window(g.ty, qx, qy, w, h).ravel(), _window(g.tu, qx >> 1, qy >> 1, w // 2, h // 2).ravel(),
                                   _window(g.tv, qx >> 1, qy >> 1, w // 2, h // 2).ravel()]))
    return out


def _oracle_encoded_subsample(w, h, br, sid):
    def build(oracle):
        oe = oracle.encoder(w, h, br)
        oe.set_frame_skip(False)
        return [oe.encode(f) for f in subsample_frames(sid, w, h)], (w, h)
    return build


STREAMS = dict(tdr.STREAMS)
for _w, _h, _br in ENC_CASES:
    for _sid in ENC_STREAM_IDS:
        STREAMS[f'oracle_enc_subsample_{_w}x{_h}_s{_sid}'] = ('encoder', _oracle_encoded_subsample(_w, _h, _br, _sid))
for name, b in LONG.items():
    STREAMS[name] = ('LONG', b)
for name, b in RECON_DIRECTED.items():
    STREAMS[f'recon_{name}'] = ('RECON', b)


def _nal_ref_idc(unit):
    """nal_ref_idc of the access unit's slices (7.3.1)"""
    for k in range(len(unit) - 4):
        if unit[k:k + 3] == b'\x00\x00\x01' and unit[k + 3] & 31 in (1, 5):
            return (unit[k + 3] >> 5) & 3
    raise AssertionError('no slice in the access unit')


class Analysis:
    """one stream, decoded once by the oracle with its capture on and rebuilt by reconref + dbkref"""

    def __init__(self, name, build=None):
        from _oracle import Oracle
        oracle = Oracle(SO)
        self.units, self.size = (build or STREAMS[name][1])(oracle)
        d = oracle.decoder()
        d.set_capture(True)
        self.counts = reconref.Counter()
        self.stage_bad = self.chain_bad = self.record_bad = None
        self.chain, self.syntax, self.geometry = [], [], None   # per picture: the chain's cropped I420; the syntax
        prev_oracle = prev_chain = None                         # the reference picture at coded size, by either route
        for k, u in enumerate(self.units):
            rc, pic, w, h = d.decode(u)
            assert rc == 1, f'{name} unit {k}: oracle decode rc {rc}'
            cw, ch = d.coded_size()
            geo = (cw // 16, ch // 16)
            syn, pre, rec = d.syntax(), d.prefilter(), d.records()
            self.syntax.append(syn)
            self.geometry = geo
            # ---- stage: the oracle's own previous picture as reference
            res = reconref.reconstruct(syn, geo, prev_oracle)
            self.counts.update(res.counts)
            if self.stage_bad is None:
                msg = reconref.first_difference(res, pre, cw, ch)
                if msg:
                    self.stage_bad = f'picture {k}: {msg}'
            if self.record_bad is None:
                cols = list(range(0, 54))
                ne = np.argwhere(res.records[:, cols] != rec[:, cols])
                if len(ne):
                    a, c = (int(v) for v in ne[0])
                    self.record_bad = (f'picture {k} MB {a} record int {c}: reference {int(res.records[a, c])}, oracle {int(rec[a, c])}; '
                                       + ' | '.join(res.explain(0, 16 * (a % geo[0]), 16 * (a // geo[0]))))
            # ---- chain: no sample from the oracle
            same_ref = prev_chain is prev_oracle or all(np.array_equal(x, y) for x, y in zip(prev_chain, prev_oracle))
            cres = res if same_ref else reconref.reconstruct(syn, geo, prev_chain)   # equal inputs: one computation serves both
            out = dbkref.deblock(cres.planes, cres.records)
            self.chain.append((out.i420(w, h), w, h))
            if self.chain_bad is None and not np.array_equal(out.i420(w, h), pic):
                msg = reconref.first_difference(cres, pre, cw, ch) or dbkref.first_difference(out, planes_of(pic, w, h), w, h)
                self.chain_bad = f'picture {k}: {msg}'
            if _nal_ref_idc(u):
                prev_chain = out.planes
                prev_oracle = dbkref.deblock(pre, rec).planes   # == the oracle's output at coded size (test_dbk_reference)


@functools.lru_cache(maxsize=None)
def analysed(name):
    return Analysis(name)


@pytest.mark.parametrize('name', list(STREAMS))
def test_stage_reference_equals_oracle(oracle, name):
    """reconref(the oracle's syntax, the oracle's previous picture) == h264o_dec_prefilter over the whole coded picture;
    the derived type, QPY, TotalCoeff, ref and vectors == h264o_dec_records"""
    a = analysed(name)
    assert a.stage_bad is None, f'{name}: oracle picture before the filter != clauses 8.3-8.5 reference: {a.stage_bad}'
    assert a.record_bad is None, f'{name}: {a.record_bad}'


@pytest.mark.parametrize('name', list(STREAMS))
def test_chain_equals_oracle(oracle, name):
    """pictures derived from syntax elements alone (reconref, dbkref, the result as the next reference) == the oracle's"""
    a = analysed(name)
    assert a.chain_bad is None, f'{name}: {a.chain_bad}'


def test_non_reference_picture_keeps_the_reference(oracle):
    """nal_ref_idc 0: the chain does not replace its reference (the picture after decodes as the oracle's)"""
    from streamgen import SyntaxGen
    g = SyntaxGen(SO, 5, 3, 8)
    a = Analysis('non-reference', build=lambda o: ([g.idr(), g.p(ref_idc=0), g.p()], (80, 48)))
    assert a.stage_bad is None and a.chain_bad is None and a.record_bad is None, (a.stage_bad, a.chain_bad, a.record_bad)


# ---------------------------------------------------------------------------------------------------------------
# parse round trip: the hook's syntax == what the generator wrote


def _expected_blocks(s, it_is_i16, cbp):
    """the residual blocks of one macroblock's hook syntax in parse order (7.3.5.3), as lists of levels"""
    out = []
    if it_is_i16:
        out.append([int(v) for v in s[80:96]])
    for b in range(16):
        if (cbp >> (b >> 2)) & 1:
            out.append([int(v) for v in s[96 + 16 * b:96 + 16 * b + (15 if it_is_i16 else 16)]])
    if cbp >> 4:
        out += [[int(v) for v in s[352 + 4 * k:356 + 4 * k]] for k in (0, 1)]
        if cbp >> 4 == 2:
            out += [[int(v) for v in s[360 + 64 * k + 16 * b:360 + 64 * k + 16 * b + 15]] for k in (0, 1) for b in range(4)]
    return out


def _check_mblog(syn, mblog, where):
    assert len(syn) == len(mblog)
    for a, (s, m) in enumerate(zip(syn, mblog)):
        at = f'{where} MB {a}'
        assert int(s[0]) == m['mb_type'], f'{at}: mb_type {int(s[0])} != written {m["mb_type"]}'
        assert (int(s[73]), int(s[74])) == (m['slice_qp'], m['first']), f'{at}: SliceQPY / first_mb_in_slice'
        if m['mb_type'] == -1:
            continue
        it = m['mb_type'] - (5 if int(s[1]) == 0 else 0)
        if int(s[1]) == 0 and m['mb_type'] < 5:
            n = len(m['mvd'])
            assert [int(v) for v in s[2:6]] == m['subs'], f'{at}: sub_mb_type'
            assert [(int(s[6 + 2 * k]), int(s[7 + 2 * k])) for k in range(n)] == m['mvd'], f'{at}: mvd_l0'
            assert not s[6 + 2 * n:38].any(), f'{at}: mvd beyond the last partition'
            i16 = False
        else:
            if it == 25:
                assert [int(v) for v in s[488:872]] == m['pcm'], f'{at}: pcm_sample'
                continue
            i16 = it != 0
            if not i16:
                assert [int(v) for v in s[38:54]] == m['prev'], f'{at}: prev_intra4x4_pred_mode_flag'
                assert [int(v) for v in s[54:70]] == m['rem'], f'{at}: rem_intra4x4_pred_mode'
            assert int(s[70]) == m['chroma_mode'], f'{at}: intra_chroma_pred_mode'
        cbp = m['cbp']
        if i16:
            assert cbp == ((((it - 1) // 4) % 3) << 4 | (15 if it >= 13 else 0)), f'{at}: the I_16x16 pattern in mb_type'
        else:
            assert int(s[71]) == cbp, f'{at}: coded_block_pattern {int(s[71])} != written {cbp}'
        assert int(s[72]) == m.get('dq', 0), f'{at}: mb_qp_delta {int(s[72])} != written {m.get("dq", 0)}'
        assert _expected_blocks(s, i16, cbp) == m.get('blocks', []), f'{at}: coefficient levels'


def _roundtrip_units():
    """(name, [(access unit, its mblog, 'gen')]) of SyntaxGen streams: cropped, chroma offsets, multi-slice"""
    from streamgen import SyntaxGen
    from test_syntax_streams import CASES, MULTI, SLICES
    out = []
    for case in (CASES[1], CASES[3]):
        mbw, mbh, cr, cb, cqp, iqp, seed = case
        g = SyntaxGen(SO, mbw, mbh, seed, crop_right=cr, crop_bottom=cb, cqp=cqp, init_qp=iqp)
        units = [(g.idr(), g.mblog, 'gen')]
        for kw in SLICES:
            units.append((g.p(**kw), g.mblog, 'gen'))
        out.append((f'syntax_{mbw}x{mbh}', units))
    g = SyntaxGen(SO, 11, 9, 21)
    units = [(g.idr(slices=MULTI[1]), g.mblog, 'gen')] + [(g.p(slices=MULTI[1]), g.mblog, 'gen') for _ in range(2)]
    out.append(('multi_1', units))
    return out


def test_parse_round_trip_syntaxgen(oracle):
    """mb_type, sub types, mvd, intra mode flags and rem values, chroma mode, cbp, mb_qp_delta, every level of every block
    and the PCM samples, as the oracle parsed them == as SyntaxGen wrote them"""
    for name, units in _roundtrip_units():
        d = oracle.decoder()
        d.set_capture(True)
        for k, (u, mblog, _) in enumerate(units):
            assert d.decode(u)[0] == 1, f'{name} unit {k}'
            _check_mblog(d.syntax(), mblog, f'{name} picture {k}')


def test_parse_round_trip_p_frame(oracle):
    """streamgen.p_frame: skip runs and mvd up to +-96 as written"""
    from h264mi.synth import SyntheticStream
    from streamgen import p_frame
    d = oracle.decoder()
    d.set_capture(True)
    assert d.decode(oracle.encoder(48, 48, 100000).encode(np.ascontiguousarray(SyntheticStream(3, 48, 48).frame(0))))[0] == 1
    rng = np.random.default_rng(11)
    for t in range(1, 4):
        log = []
        assert d.decode(p_frame(3, 3, t, 2 * t, rng, max_mvd=96, log=log))[0] == 1
        syn = d.syntax()
        assert len(log) == 9
        for a, m in enumerate(log):
            if m is None:
                assert int(syn[a, 0]) == -1, f'picture {t} MB {a}: written as skipped'
            else:
                assert (int(syn[a, 0]), int(syn[a, 6]), int(syn[a, 7]), int(syn[a, 71])) == (0, m[0], m[1], 0), f'picture {t} MB {a}'


# ---------------------------------------------------------------------------------------------------------------
# VLC tables: structure only (their values remain unpinned against an outside source)


def _codes(lens, codes):
    return [(int(n), int(c)) for n, c in zip(lens, codes) if n]


def _assert_prefix_free(pairs, what):
    words = [format(c, 'b').zfill(n) for n, c in pairs]
    assert all(len(w) == n for w, (n, _) in zip(words, pairs)), f'{what}: a code does not fit its length'
    assert len(set(words)) == len(words), f'{what}: a code word twice'
    srt = sorted(words)
    assert not any(b.startswith(a) for a, b in zip(srt, srt[1:])), f'{what}: not prefix-free'
    from fractions import Fraction
    assert sum(Fraction(1, 2 ** n) for n, _ in pairs) <= 1, f'{what}: Kraft sum above 1'


VLC = [('ct_len', 'ct_code', 4, 68, 'CT_LEN', 'CT_CODE'), ('ct_dc_len', 'ct_dc_code', 1, 20, 'CTDC_LEN', 'CTDC_CODE'),
       ('tz_len', 'tz_code', 15, 16, 'TZ_LEN', 'TZ_CODE'), ('tz_dc_len', 'tz_dc_code', 3, 4, 'TZDC_LEN', 'TZDC_CODE'),
       ('rb_len', 'rb_code', 7, 15, 'RB_LEN', 'RB_CODE')]


def test_vlc_tables_are_prefix_free(oracle):
    """coeff_token per nC class and for chroma DC, total_zeros per TotalCoeff (4x4 and chroma DC), run_before per
    zerosLeft: every table of oracle/h264o_tables.h is a prefix-free code with a Kraft sum of at most 1"""
    for ln, cn, rows, width, _, _ in VLC:
        L, C = _oracle_table(oracle, ln, rows * width), _oracle_table(oracle, cn, rows * width)
        for r in range(rows):
            pairs = _codes(L[r * width:(r + 1) * width], C[r * width:(r + 1) * width])
            assert pairs, (ln, r)
            _assert_prefix_free(pairs, f'{ln} row {r}')


def test_vlc_tables_match_the_kernel_source(oracle):
    """Both typed copies of the VLC tables in the kernels == the oracle's, by value: the (length, code) arrays from which
    csrc/vlc_tables.inc builds the decoder's lookup tables at compile time (a collision is a compile error), and the
    arrays inside build_cavlc_tabs() of csrc/enc_bits.inc, which the encoder packs as (length << 8) | code -- that packed
    image is derived here from the oracle's pairs and from the parsed arrays and compared"""
    enc = _csrc('enc_bits.inc')
    enc = enc[enc.index('build_cavlc_tabs()'):]
    for ln, cn, rows, width, kl, kc in VLC:
        L, C = _oracle_table(oracle, ln, rows * width), _oracle_table(oracle, cn, rows * width)
        packed = [(a << 8) | b for a, b in zip(_rows(enc, kl, width), _rows(enc, kc, width))]
        assert packed == [(a << 8) | b for a, b in zip(L, C)], f'enc_bits.inc {kl} / {kc}'
    src = _csrc('vlc_tables.inc')
    for ln, cn, rows, width, kl, kc in VLC:
        keep = 3 * width if kl == 'CT_LEN' else rows * width   # coeff_token for nC >= 8 is a fixed-length code: no table
        assert _rows(src, kl, width)[:keep] == _oracle_table(oracle, ln, rows * width)[:keep], kl
        assert _rows(src, kc, width)[:keep] == _oracle_table(oracle, cn, rows * width)[:keep], kc
    # that class in the derived form the kernels compute (Table 9-5, 8 <= nC: 6 bits, 0000 11 for no coefficient, else
    # TotalCoeff - 1 and TrailingOnes)
    L, C = _oracle_table(oracle, 'ct_len', 272)[204:], _oracle_table(oracle, 'ct_code', 272)[204:]
    for tc in range(17):
        for t1 in range(4):
            valid = t1 <= min(tc, 3)
            assert L[4 * tc + t1] == (6 if valid else 0), (tc, t1)
            if valid:
                assert C[4 * tc + t1] == (3 if tc == 0 else ((tc - 1) << 2 | t1)), (tc, t1)


# ---------------------------------------------------------------------------------------------------------------
# coverage

# Classes of reconref's list that cannot occur in the pictures the decoders accept, with the clause. Nothing else.
EXCLUDED = {
    ('tr_substituted', 'slice_edge'):
        'p[x, -1], x = 4..7, lies in another slice only when mbAddrC does while mbAddrB, which holds p[0..3, -1], does not '
        '(6.4.11.4: only luma4x4BlkIdx 5 reads mbAddrC). With one slice group (num_slice_groups_minus1 0; FMO is rejected) '
        'a slice is a run of consecutive addresses, and mbAddrC = mbAddrB + 1 (6.4.9), so an available mbAddrB '
        '(>= first_mb_in_slice) makes mbAddrC available unless it is outside the picture',
}

FAMILIES = ('CASES', 'MULTI', 'LONG', 'DIRECTED', 'RECON')


def family_counts(families):
    total = reconref.Counter()
    for name, (fam, _) in STREAMS.items():
        if fam in families:
            total.update(analysed(name).counts)
    return total


def test_every_recon_class_is_reached(oracle):
    """every class of clauses 8.3-8.5 that reconref counts is reached by CASES + MULTI + the p_frame streams + the
    directed streams -- the streams the GPU decoder tests run"""
    hit = family_counts(FAMILIES)
    missing = sorted((k for k in reconref.required_classes() if k not in EXCLUDED and hit[k] == 0), key=str)
    assert not missing, f'{len(missing)} classes never reached: {missing}'
    assert all(hit[k] == 0 for k in EXCLUDED), 'an excluded class occurred'


def test_encoder_streams_reach_the_half_sample_positions(oracle):
    """the inputs of the GPU module's encoder test, coded by the oracle encoder (one slice: the GPU encoder's bytes): every
    stream holds its ENC_REQUIRED positions at every size, together all seven positions with a half-sample component --
    b, h and j predicted from directly, and j in the averages f, i, k, q"""
    for w, h, _ in ENC_CASES:
        for sid in ENC_STREAM_IDS:
            c = analysed(f'oracle_enc_subsample_{w}x{h}_s{sid}').counts
            missing = [p for p in ENC_REQUIRED[sid] if c[('luma_frac', '16x16', p[0], p[1])] == 0]
            assert not missing, f'{w}x{h} stream {sid}: positions {missing} not reached'
    assert {p for v in ENC_REQUIRED.values() for p in v} == {(x, y) for x in range(4) for y in range(4) if 2 in (x, y)}


def audit_table():
    fams = ['CASES', 'MULTI', 'LONG', 'encoder', 'DIRECTED', 'RECON']
    per = {f: family_counts((f,)) for f in fams}
    rows = ['| class | ' + ' | '.join(fams) + ' |', '|---|' + '---:|' * len(fams)]
    for key in sorted(reconref.required_classes(), key=str):
        rows.append('| `' + ' '.join(str(k) for k in key) + '` | ' + ' | '.join(str(per[f][key]) for f in fams) + ' |')
    return '\n'.join(rows)


if __name__ == '__main__':
    print(audit_table())
