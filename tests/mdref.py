"""An independent statement of the encoder's P-macroblock decisions -- TEST INFRASTRUCTURE ONLY.

Written from DESIGN.md §3.3 (the I16x16 rule), §3.5, §3.6 (the row plan), §3.7 (the slice-edge list), §3.12 (the sentences
the rule needs and the earlier sections left out) and tests/golden/openh264_tables.json (`lambda`, `i16_avail_modes`,
`i16_mode_map`, `single_ctr_run`, `chroma_qp`, `quant_mf`, `quant_ff`): not from the oracle's encode_p_mb, not from
enc_mb_kernel.inc, not from the listings transcribed in tests/test_oracle_golden.py. What is independent already is reused:
the prediction at a quarter-sample vector, the MV predictor, the skip vector and the intra prediction (tests/reconref.py),
the transform and quantiser (tests/fwdref.py), the frame-level rate control's window (tests/rcref.py).

The check is teacher-forced per macroblock: the neighbours' types, vectors and unfiltered samples are those in the bytes,
and the reference states the one outcome the rules demand of this macroblock:

    skip_judge      P_Skip by the judge                  intra_after_skip     intra after a taken skip
    p16             P16x16 with its vector               intra_after_search   intra after the integer search
    skip_double     P_Skip by the double check

and compares it with the bytes. A Mismatch names the macroblock, both outcomes and every intermediate the rule went
through. For an Intra16x16 macroblock (I slices too) the prediction mode must be §3.3's first minimum; whether an intra
macroblock is Intra4x4 or Intra16x16 is not restated (counted in Checked.intra_kind_open).

Stream(w, h, bitrate) carries what a picture's decisions need from the pictures before it: the reference planes, the
last P picture's skip SADs, the last coded picture's row bits and a rcref.PyRc for the QP window.
"""
import json
import os

import numpy as np

import fwdref
import rcref
import reconref
from fwdref import I4, I16, P16, PSKIP

HERE = os.path.dirname(os.path.abspath(__file__))
_T = json.load(open(os.path.join(HERE, 'golden', 'openh264_tables.json')))['tables']


def _tab(name):
    v = _T[name]['values']
    return np.array(json.loads(v) if isinstance(v, str) else v, np.int64)


LAMBDA = _tab('lambda').ravel()
I16_AVAIL = _tab('i16_avail_modes').reshape(8, 5)
I16_MAP = _tab('i16_mode_map').ravel()
SINGLE_CTR = _tab('single_ctr_run').ravel()
CHROMA_QP = _tab('chroma_qp').ravel()
H4 = fwdref.H4

DIAMOND = ((0, -1), (-1, 0), (1, 0), (0, 1))
SUBPEL = ((0, -1), (0, 1), (-1, 0), (1, 0), (-1, -1), (1, -1), (-1, 1), (1, 1))
RASTER8 = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))
RANGE = 16
OUTCOMES = ('skip_judge', 'intra_after_skip', 'intra_after_search', 'p16', 'skip_double')
EDGE_ITEMS = ('mvp', 'cand', 'try', 'keep', 'predsad', 'i16')


class Rules:
    """the switches a mutation turns; the default is the text as stated"""

    def __init__(self, name='as stated', kind='', **kw):
        self.name, self.kind = name, kind
        # search
        self.drop_cand = None            # 'A' / 'B' / 'C'
        self.c_no_topleft = False
        self.cand_round = 'round'        # 'trunc': >> 2
        self.cand_clip = True
        self.last_min = False
        self.diamond = DIAMOND
        self.diamond_cap = 32
        self.diamond_nonstrict = False
        self.cross_thr = 1024
        self.cross_ge = False
        self.cross_v_first = False
        self.cross_from_start = False
        self.mvd_vs_zero = False
        self.lambda_qp_off = 0
        # refinement
        self.subpel = SUBPEL
        self.quarter_around_integer = False
        self.subpel_sad = False
        self.subpel_no_bits = False
        # judge and after
        self.try_no_topleft = False
        self.try_no_coloc = False
        self.t_no_chroma = False
        self.predsad_median_always = False
        self.luma_ctr_max = 5
        self.chroma_ctr_max = 6
        self.level_max = 1
        self.keep_no_topright = False
        self.intra_vs_subpel = False
        self.intra_le = False
        self.double_check = True
        # slice edge: the items of §3.7's list that read the row above across a slice edge
        self.cross_edge = frozenset()
        # row plan
        self.mean_rows_with_bits = False
        self.thr2_ge = self.thr125_ge = self.thr05_le = False
        self.row_no_clip = False
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


MUTATIONS = [
    Rules('candidate A dropped', 'search', drop_cand='A'),
    Rules('candidate B dropped', 'search', drop_cand='B'),
    Rules('candidate C dropped', 'search', drop_cand='C'),
    Rules('C not replaced by the top-left MB', 'search', c_no_topleft=True),
    Rules('candidates truncated (>> 2), not rounded', 'search', cand_round='trunc'),
    Rules('candidates not clipped to +-16', 'search', cand_clip=False),
    Rules('last minimum candidate instead of the first', 'search', last_min=True),
    Rules('diamond points in another order', 'search', diamond=((0, 1), (1, 0), (-1, 0), (0, -1))),
    Rules('diamond cap 31', 'search', diamond_cap=31),
    Rules('diamond cap 33', 'search', diamond_cap=33),
    Rules('diamond moves without strict improvement', 'search', diamond_nonstrict=True),
    Rules('cross search at >= 1024', 'search', cross_ge=True),
    Rules('cross search above 512', 'search', cross_thr=512),
    Rules('cross search above 2048', 'search', cross_thr=2048),
    Rules('vertical line before horizontal', 'search', cross_v_first=True),
    Rules('cross lines through the start point', 'search', cross_from_start=True),
    Rules('mvd bits against zero', 'search', mvd_vs_zero=True),
    Rules('lambda of QP + 1', 'search', lambda_qp_off=1),
    Rules('sub-pel neighbours in raster order', 'refinement', subpel=RASTER8),
    Rules('quarter step around the integer point', 'refinement', quarter_around_integer=True),
    Rules('SAD instead of SATD', 'refinement', subpel_sad=True),
    Rules('SATD without lambda x bits', 'refinement', subpel_no_bits=True),
    Rules('top-left neighbour ignored for the try', 'judge', try_no_topleft=True),
    Rules('co-located MB ignored', 'judge', try_no_coloc=True),
    Rules('T without chroma', 'judge', t_no_chroma=True),
    Rules('median where a single skipped neighbour\'s SAD is due', 'judge', predsad_median_always=True),
    Rules('luma cost limit 4', 'judge', luma_ctr_max=4),
    Rules('luma cost limit 6', 'judge', luma_ctr_max=6),
    Rules('chroma cost limit 5', 'judge', chroma_ctr_max=5),
    Rules('chroma cost limit 7', 'judge', chroma_ctr_max=7),
    Rules('level limit 2', 'judge', level_max=2),
    Rules('keep without the top-right MB', 'judge', keep_no_topright=True),
    Rules('intra compared against the sub-pel cost', 'judge', intra_vs_subpel=True),
    Rules('intra compared with <=', 'judge', intra_le=True),
    Rules('double check off', 'judge', double_check=False),
    Rules('slice edge: MV predictor reads the row above', 'slice', cross_edge=frozenset(['mvp'])),
    Rules('slice edge: start candidates read the row above', 'slice', cross_edge=frozenset(['cand'])),
    Rules('slice edge: judge tried by the row above', 'slice', cross_edge=frozenset(['try'])),
    Rules('slice edge: keep satisfied by the row above', 'slice', cross_edge=frozenset(['keep'])),
    Rules('slice edge: predicted SAD counts the row above', 'slice', cross_edge=frozenset(['predsad'])),
    Rules('slice edge: I16x16 uses the row above', 'slice', cross_edge=frozenset(['i16'])),
    Rules('row mean over rows with bits only', 'rowplan', mean_rows_with_bits=True),
    Rules('row +2 at >= 2x', 'rowplan', thr2_ge=True),
    Rules('row +1 at >= 1.25x', 'rowplan', thr125_ge=True),
    Rules('row -1 at <= 0.5x', 'rowplan', thr05_le=True),
    Rules('row QP not clipped to the window', 'rowplan', row_no_clip=True),
]


class Mismatch:
    def __init__(self, message, mb, what):
        self.message, self.mb, self.what = message, mb, what

    def __str__(self):
        return self.message


def se_bits(v):
    """the length of se(v) (9.1): codeNum = 2 |v| - (v > 0), 2 floor(log2(codeNum + 1)) + 1 bits"""
    k = 2 * abs(int(v)) - (1 if v > 0 else 0)
    return 2 * (k + 1).bit_length() - 1


def mvd_bits(mv, pred):
    return se_bits(mv[0] - pred[0]) + se_bits(mv[1] - pred[1])


def single_ctr(levels):
    """per non-zero level in scan order, SINGLE_CTR[the zeros below it back to the next non-zero level or the start]"""
    cost, run = 0, 0
    for v in levels:
        if v:
            cost += int(SINGLE_CTR[run])
            run = 0
        else:
            run += 1
    return cost


def satd16(d):
    """per 4x4 block (sum |H4 . D . H4^T| + 1) >> 1, summed over the sixteen blocks"""
    b = d.reshape(4, 4, 4, 4).transpose(0, 2, 1, 3)
    t = np.abs(H4 @ b @ H4.T).sum(axis=(2, 3))
    return int(((t + 1) >> 1).sum())


def row_delta(bits, mean, rules):
    if mean <= 0:
        return 0
    if (bits >= 2 * mean) if rules.thr2_ge else (bits > 2 * mean):
        return 2
    if (4 * bits >= 5 * mean) if rules.thr125_ge else (4 * bits > 5 * mean):
        return 1
    if (2 * bits <= mean) if rules.thr05_le else (2 * bits < mean):
        return -1
    return 0


def row_plan(rowbits, frame_qp, window, rules):
    """§3.6: the QP of every MB row of a P picture from the last coded picture's row bits"""
    mbh = len(rowbits)
    if rules.mean_rows_with_bits:
        n = sum(1 for b in rowbits if b > 0)
        mean = sum(rowbits) // n if n else 0
    else:
        mean = sum(rowbits) // mbh
    out = []
    for b in rowbits:
        q = frame_qp + row_delta(b, mean, rules)
        out.append(q if rules.row_no_clip else min(window[1], max(window[0], q)))
    return out


class Stream:
    """what one stream's decisions carry from picture to picture"""

    def __init__(self, w, h, br, skip=False, gom=False, nslices=1):
        self.w, self.h, self.gom, self.nslices = w, h, gom, nslices
        self.mbw, self.mbh = (w + 15) // 16, (h + 15) // 16
        self.rc = rcref.PyRc(w, h, br, skip_en=skip)
        self.ref = None            # dbkref's planes of the last coded picture
        self.sksad = None          # the last coded picture's skip SADs (-1: none), None after an IDR
        self.rowbits = [0] * self.mbh
        self.pstate = None         # parseref.State, set by the caller's chain

    def force_idr(self):
        self.rc.force_idr()


class Picture:
    """one coded picture, with everything its check needs and the caches no rule changes"""


def _i16_mode(syn_row):
    it = int(syn_row[0]) - (5 if int(syn_row[1]) == 0 else 0)
    return (it - 1) % 4


def picture(stream, src, parsed, res, label=''):
    """src: tight I420 source; parsed / res: parseref.Parsed and reconref.Result of the bytes. Call before the stream
    advances (advance())."""
    p = Picture()
    p.label, p.stream, p.parsed, p.res = label, stream, parsed, res
    mbw, mbh = parsed.geometry
    p.mbw, p.mbh, p.nmb = mbw, mbh, mbw * mbh
    p.src = fwdref.pad_source(src, stream.w, stream.h)
    syn = np.asarray(parsed.syntax, np.int64).reshape(p.nmb, -1)
    rec = np.asarray(res.records, np.int64)
    p.syn, p.typ, p.qp, p.first = syn, rec[:, 0].copy(), rec[:, 1].copy(), rec[:, 54].copy()
    p.mv = rec[:, 22:24].copy()
    p.is_p = bool((syn[:, 1] == 0).any())
    assert (syn[:, 1] == syn[0, 1]).all(), 'slices of different types in one picture'
    p.slice_qp = int(syn[0, 73])
    assert (syn[:, 73] == p.slice_qp).all(), 'the slices of one picture carry different slice QPs'
    p.cbp = np.where(p.typ == PSKIP, 0, np.where(p.typ == I16, -1, syn[:, 71]))
    p.carrier = (p.typ == I16) | ((p.typ != PSKIP) & (p.typ != I16) & (syn[:, 71] != 0))
    p.rowbits = [sum(b - a for a, b in (parsed.layer_span(m) for m in range(r * mbw, (r + 1) * mbw) if parsed.layer_span(m))) for r in range(mbh)]
    p.ref = stream.ref
    p.prev_sksad = stream.sksad
    p.prev_rowbits = list(stream.rowbits)
    p.window, p.model_qp = (stream.rc.min_qp, stream.rc.max_qp), stream.rc.qp
    p.hv = reconref._halves(np.asarray(p.ref[0])) if (p.is_p and p.ref is not None) else None
    p.sadmaps, p.satd_cache, p.pred_cache, p.i16_cache = {}, {}, {}, {}
    # the picture as the macroblocks in the bytes left it, for reconref's neighbour rules; `open` reads across slices
    p.pics = {}
    for crossing in (False, True):
        q = reconref._Picture(mbw, mbh)
        q.P = [np.asarray(a, np.int32) for a in res.planes]
        q.built = [np.ones(a.shape, bool) for a in q.P]
        q.mv = np.asarray(rec[:, 22:54], np.int32).reshape(mbh, mbw, 4, 4, 2).transpose(0, 2, 1, 3, 4).reshape(4 * mbh, 4 * mbw, 2)
        intra = np.isin(p.typ, (I4, I16))
        q.ref = np.repeat(np.repeat(np.where(intra, -1, 0).reshape(mbh, mbw), 4, 0), 4, 1).astype(np.int32)
        q.derived = np.ones((4 * mbh, 4 * mbw), bool)
        q.mbtype = p.typ.astype(np.int32)
        q.first = np.zeros(p.nmb, np.int32) if crossing else p.first.astype(np.int32)
        p.pics[crossing] = q
    # the skip SAD of every macroblock the bytes code as P_Skip: T at its vector (§3.5)
    p.sksad = np.full(p.nmb, -1, np.int64)
    if p.is_p:
        for mb in np.flatnonzero(p.typ == PSKIP):
            p.sksad[mb] = _T_at(p, int(mb), tuple(int(v) for v in p.mv[mb]))[0]
    return p


def slice_nal_bytes(unit):
    """the bytes of every slice NAL unit of an access unit, start codes included"""
    starts = [k for k in range(len(unit) - 4) if unit[k:k + 4] == b'\x00\x00\x00\x01']
    return sum(b - a for a, b in zip(starts, starts[1:] + [len(unit)]) if unit[a + 4] & 31 in (1, 5))


def advance(stream, p, ref_planes, nal, idr):
    """after a coded picture: carry its reference planes, skip SADs and row bits; the rate control's update"""
    stream.ref = ref_planes
    stream.sksad = p.sksad.copy() if p.is_p else None
    stream.rowbits = list(p.rowbits)
    coded = p.typ != PSKIP
    n = int(coded.sum())
    # §3.6 update: the average QP over the macroblocks with bits, rounded; the frame QP of an IDR or without any
    avg = (n * 50 + int(p.qp[coded].sum()) * 100) // (n * 100) if (p.is_p and n) else stream.rc.qp
    # §3.7: the frame's bits are the bytes of all its slice NAL units, the parameter sets excluded
    stream.rc.picture_update(stream.rc.cur_idr, slice_nal_bytes(nal), avg, stream.rc.cmplx)


# ------------------------------------------------------------------------------------------------- pieces of the rule
def _src_mb(p, mb):
    x, y = 16 * (mb % p.mbw), 16 * (mb // p.mbw)
    return p.src[0][y:y + 16, x:x + 16], p.src[1][y // 2:y // 2 + 8, x // 2:x // 2 + 8], p.src[2][y // 2:y // 2 + 8, x // 2:x // 2 + 8]


def _pred_at(p, mb, mv):
    """(luma 16x16, Cb 8x8, Cr 8x8) of macroblock mb predicted at quarter-sample vector mv: reconref's"""
    key = (mb, mv)
    if key not in p.pred_cache:
        x, y = 16 * (mb % p.mbw), 16 * (mb // p.mbw)
        p.pred_cache[key] = (reconref._luma_pred(p.hv, x, y, 16, 16, mv[0], mv[1]),
                             reconref._chroma_pred(np.asarray(p.ref[1]), x // 2, y // 2, 8, 8, mv[0], mv[1]),
                             reconref._chroma_pred(np.asarray(p.ref[2]), x // 2, y // 2, 8, 8, mv[0], mv[1]))
    return p.pred_cache[key]


def _T_at(p, mb, mv):
    """-> (T, luma SAD, chroma SADs) of the prediction at mv"""
    sy, su, sv = _src_mb(p, mb)
    py, pu, pv = _pred_at(p, mb, mv)
    l, c = int(np.abs(sy - py).sum()), int(np.abs(su - pu).sum() + np.abs(sv - pv).sum())
    return l + c, l, c


def _sadmap(p, mb):
    """the luma SAD at every integer vector -17..17 (the search stays inside -16..16; an unclipped candidate may not)"""
    if mb not in p.sadmaps:
        R = RANGE + 1
        x, y = 16 * (mb % p.mbw), 16 * (mb // p.mbw)
        win = reconref._fetch(p.hv, 'G', x - R + np.arange(16 + 2 * R), y - R + np.arange(16 + 2 * R))
        v = np.lib.stride_tricks.sliding_window_view(win, (16, 16))
        p.sadmaps[mb] = np.abs(v - _src_mb(p, mb)[0][None, None]).sum(axis=(2, 3))
    return p.sadmaps[mb]


def _sad_int(p, mb, ix, iy):
    if max(abs(ix), abs(iy)) <= RANGE + 1:
        return int(_sadmap(p, mb)[iy + RANGE + 1, ix + RANGE + 1])
    return _T_at(p, mb, (4 * ix, 4 * iy))[1]


def _satd_at(p, mb, mv, sad=False):
    key = (mb, mv, sad)
    if key not in p.satd_cache:
        d = _src_mb(p, mb)[0] - _pred_at(p, mb, mv)[0]
        p.satd_cache[key] = int(np.abs(d).sum()) if sad else satd16(d)
    return p.satd_cache[key]


def _avail(p, mb, dx, dy, crossing):
    """the neighbouring macroblock at (dx, dy), or None: outside the picture, or (7.4.3) in another slice"""
    x, y = mb % p.mbw + dx, mb // p.mbw + dy
    if not (0 <= x < p.mbw and 0 <= y < p.mbh):
        return None
    nb = y * p.mbw + x
    if nb < p.first[mb] and not crossing:
        return None
    return nb


def _levels_luma(p, mb, pred, qp):
    """the inter levels of the sixteen luma blocks, every position: [raster block, y, x]"""
    d = (_src_mb(p, mb)[0] - pred).reshape(4, 4, 4, 4).transpose(0, 2, 1, 3).reshape(16, 4, 4)
    col = (np.arange(16) & 7).reshape(4, 4)
    return fwdref.quant(fwdref.forward(d), fwdref.FF[qp][col], fwdref.MF[qp][col])


def _levels_chroma(p, mb, pred, qpc):
    """-> (DC levels [2, 2], levels of every position by the AC rule [4 blocks, y, x]) of one chroma plane"""
    src, prd = pred
    d = (src - prd).reshape(2, 4, 2, 4).transpose(0, 2, 1, 3).reshape(4, 4, 4)
    c = fwdref.forward(d)
    col = (np.arange(16) & 7).reshape(4, 4)
    ac = fwdref.quant(c, fwdref.FF[qpc][col], fwdref.MF[qpc][col])
    ff, mf = fwdref.dc_params(fwdref.FF[qpc][0], fwdref.MF[qpc][0])
    dc = fwdref.quant(fwdref.H2 @ c[:, 0, 0].reshape(2, 2) @ fwdref.H2.T, ff, mf)
    return dc, ac


def _scan(block):
    return [int(block.ravel()[k]) for k in fwdref.SCAN_POS]


def residual_test(p, mb, mv, qp, rules, st):
    """§3.5's residual test at the skip vector -> True when the residual admits the skip"""
    py, pu, pv = _pred_at(p, mb, mv)
    lv = _levels_luma(p, mb, py, qp)
    cost = 0
    for b in range(16):
        m = int(np.abs(lv[b]).max())
        if m > rules.level_max:
            st['residual'] = f'luma block {b}: level {m} above {rules.level_max}'
            return False
        if m:
            cost += single_ctr(_scan(lv[b]))
    st['luma_cost'] = cost
    if cost > rules.luma_ctr_max:
        st['residual'] = f'luma cost {cost} above {rules.luma_ctr_max}'
        return False
    qpc = int(CHROMA_QP[qp])
    src = _src_mb(p, mb)
    for k, prd in ((1, pu), (2, pv)):
        dc, ac = _levels_chroma(p, mb, (src[k], prd), qpc)
        if dc.any():
            st['residual'] = f'{"UV"[k - 1]}: non-zero DC level'
            return False
        cost = 0
        for b in range(4):
            m = int(np.abs(ac[b]).max())
            if m > rules.level_max:
                st['residual'] = f'{"UV"[k - 1]} block {b}: level {m} above {rules.level_max}'
                return False
            if m:
                cost += single_ctr(_scan(ac[b])[1:])
        st[f'{"uv"[k - 1]}_cost'] = cost
        if cost > rules.chroma_ctr_max:
            st['residual'] = f'{"UV"[k - 1]} cost {cost} above {rules.chroma_ctr_max}'
            return False
    st['residual'] = 'passes'
    return True


def no_levels(p, mb, mv, qp):
    """a P16x16 at mv quantised at qp has coded_block_pattern 0 (§3.4: the levels go to the pattern as they are)"""
    py, pu, pv = _pred_at(p, mb, mv)
    if _levels_luma(p, mb, py, qp).any():
        return False
    qpc = int(CHROMA_QP[qp])
    src = _src_mb(p, mb)
    for k, prd in ((1, pu), (2, pv)):
        dc, ac = _levels_chroma(p, mb, (src[k], prd), qpc)
        ac[:, 0, 0] = 0
        if dc.any() or ac.any():
            return False
    return True


def predicted_sad(p, mb, rules, crossing):
    """§3.5 PredictSadSkip over the skip SADs of the picture's skipped macroblocks"""
    def one(dx, dy):
        nb = _avail(p, mb, dx, dy, crossing)
        if nb is None:
            return None
        skipped = p.typ[nb] == PSKIP
        return (bool(skipped), int(p.sksad[nb]) if skipped else 0)
    A, B, C, D = one(-1, 0), one(0, -1), one(1, -1), one(-1, -1)
    # "without a top or top-left MB the left one's" stands inside this branch: slices hold whole MB rows, so a missing top MB
    # means the whole row above is missing, the top-right MB with it -- B missing implies C missing
    if C is None:
        C = D
        if B is None and D is None and A is not None:
            return A[1]
    flags = [n is not None and n[0] for n in (A, B, C)]
    sads = [n[1] if n is not None else 0 for n in (A, B, C)]
    if sum(flags) == 1 and not rules.predsad_median_always:
        return sads[flags.index(True)]
    return sorted(sads)[1]


def i16_decision(p, mb, qp, rules, crossing=False):
    """§3.3: -> (cost, syntax mode) of the first minimum over the modes the neighbours allow, in the table's order"""
    key = (mb, qp, crossing)
    if key in p.i16_cache:
        return p.i16_cache[key]
    left, top = _avail(p, mb, -1, 0, crossing) is not None, _avail(p, mb, 0, -1, crossing) is not None
    flags = int(left) | (int(top) << 1) | (int(left and top and _avail(p, mb, -1, -1, crossing) is not None) << 2)
    row = I16_AVAIL[flags & 7]
    nb = reconref._Nb(p.pics[crossing], 0, mb, 16 * (mb % p.mbw), 16 * (mb // p.mbw))
    lam = int(LAMBDA[qp])
    src = _src_mb(p, mb)[0]
    best = None
    for k in range(int(row[4])):
        mode = int(I16_MAP[int(row[k])])
        pred = reconref._pred_square(nb, 16, ['V', 'H', 'DC', 'plane'][mode], [], 'i16')
        c = int(np.abs(src - pred).sum()) + lam * (1, 3, 3, 5)[mode]
        if best is None or c < best[0]:
            best = (c, mode)
    p.i16_cache[key] = best
    return best


def decide(p, mb, qp, rules):
    """the outcome the rules demand of P macroblock mb at decision QP qp -> (outcome, vector or None, steps)"""
    st = {'qp': qp}
    edge = rules.cross_edge
    lam = int(LAMBDA[min(51, qp + rules.lambda_qp_off)])
    st['lambda'] = lam
    pic = p.pics['mvp' in edge]
    skmv = tuple(int(v) for v in reconref._skip_mv(pic, mb)[0])
    mvp = tuple(int(v) for v in reconref._mvp(pic, mb, 0, 0, 16, 16, None, 0)[0])
    st['skip_mv'], st['mvp'] = skmv, mvp
    mbx, mby = mb % p.mbw, mb // p.mbw
    # ---- the judge
    skipped = lambda nb: nb is not None and p.typ[nb] == PSKIP
    why = []
    for name, dx, dy in (('left', -1, 0), ('top', 0, -1), ('top-left', -1, -1), ('top-right', 1, -1)):
        if name == 'top-left' and rules.try_no_topleft:
            continue
        if skipped(_avail(p, mb, dx, dy, 'try' in edge)):
            why.append(name)
    coloc = p.prev_sksad is not None and p.prev_sksad[mb] >= 0
    if coloc and not rules.try_no_coloc:
        why.append('co-located')
    st['try'] = why or 'not tried'
    taken = None
    if why:
        sx, sy = (skmv[0] >> 2) + 16 * mbx, (skmv[1] >> 2) + 16 * mby
        if -29 <= sx <= ((16 * p.mbw) | 12) and -29 <= sy <= ((16 * p.mbh) | 12):
            T, l, c = _T_at(p, mb, skmv)
            if rules.t_no_chroma:
                T = l
            st['T'], st['skip_luma_sad'] = T, l
            ps = predicted_sad(p, mb, rules, 'predsad' in edge)
            st['predicted_sad'] = ps
            cs = int(p.prev_sksad[mb]) if (coloc and not rules.try_no_coloc) else None
            st['colocated_sad'] = cs
            if T == 0:
                taken = 'T is 0'
            elif T < ps:
                taken = 'T below the predicted SAD'
            elif cs is not None and T < cs:
                taken = 'T below the co-located SAD'
            elif residual_test(p, mb, skmv, qp, rules, st):
                taken = 'the residual test'
            st['taken'] = taken or 'not taken'
        else:
            st['taken'] = 'skip vector refused'
    if taken:
        crossing = 'keep' in edge
        nbs = [_avail(p, mb, -1, 0, crossing), _avail(p, mb, 0, -1, crossing), _avail(p, mb, 1, -1, crossing)]
        if rules.keep_no_topright:
            keep = skipped(nbs[0]) and skipped(nbs[1])
        else:
            keep = all(skipped(n) for n in nbs)
        st['keep'] = bool(keep)
        if not keep:
            ic = i16_decision(p, mb, qp, rules, 'i16' in edge)[0]
            st['i16_cost'] = ic
            if (ic <= st['skip_luma_sad']) if rules.intra_le else (ic < st['skip_luma_sad']):
                return 'intra_after_skip', None, st
        return 'skip_judge', skmv, st
    # ---- integer search
    bitpred = (0, 0) if rules.mvd_vs_zero else mvp
    cost = lambda ix, iy: _sad_int(p, mb, ix, iy) + lam * mvd_bits((4 * ix, 4 * iy), bitpred)
    rnd = (lambda v: v >> 2) if rules.cand_round == 'trunc' else (lambda v: (v + 2) >> 2)
    cands = [('mvp', (rnd(mvp[0]), rnd(mvp[1]))), ('zero', (0, 0))]
    crossing = 'cand' in edge
    nbC = _avail(p, mb, 1, -1, crossing)
    if mbx + 1 >= p.mbw and not rules.c_no_topleft:
        nbC = _avail(p, mb, -1, -1, crossing)
    for name, nb in (('A', _avail(p, mb, -1, 0, crossing)), ('B', _avail(p, mb, 0, -1, crossing)), ('C', nbC)):
        if nb is None or p.typ[nb] in (I4, I16) or rules.drop_cand == name:
            continue
        cands.append((name, (rnd(int(p.mv[nb, 0])), rnd(int(p.mv[nb, 1])))))
    best, bc, cc = None, None, []
    for name, (cx, cy) in cands:
        if rules.cand_clip:
            cx, cy = max(-RANGE, min(RANGE, cx)), max(-RANGE, min(RANGE, cy))
        c = cost(cx, cy)
        cc.append((name, (cx, cy), c))
        if bc is None or c < bc or (rules.last_min and c == bc):
            best, bc = (cx, cy), c
    st['candidates'] = cc
    start = best
    path = [best]
    for _ in range(rules.diamond_cap):
        nb, nc = None, None
        for dx, dy in rules.diamond:
            cx, cy = best[0] + dx, best[1] + dy
            if max(abs(cx), abs(cy)) > RANGE:
                continue
            c = cost(cx, cy)
            if nc is None or c < nc:
                nb, nc = (cx, cy), c
        if nc is not None and (nc <= bc if rules.diamond_nonstrict else nc < bc):
            best, bc = nb, nc
            path.append(best)
        else:
            break
    st['diamond_path'], st['diamond_cost'] = path, bc
    if (bc >= rules.cross_thr) if rules.cross_ge else (bc > rules.cross_thr):
        through = start if rules.cross_from_start else best
        hor = [(x, through[1]) for x in range(-RANGE, RANGE + 1)]
        ver = [(through[0], y) for y in range(-RANGE, RANGE + 1)]
        for cx, cy in (ver + hor) if rules.cross_v_first else (hor + ver):
            c = cost(cx, cy)
            if c < bc:
                best, bc = (cx, cy), c
        st['cross'] = best
    else:
        st['cross'] = 'off'
    st['integer'], st['integer_cost'] = best, bc
    # ---- refinement (after the intra test in the text; before it only for the mutation that compares its cost)
    def refine():
        sub = lambda mv: _satd_at(p, mb, mv, rules.subpel_sad) + (0 if rules.subpel_no_bits else lam * mvd_bits(mv, bitpred))
        mv = (4 * best[0], 4 * best[1])
        sc = sub(mv)
        costs = [(mv, sc)]
        for step in (2, 1):
            centre = (4 * best[0], 4 * best[1]) if (step == 1 and rules.quarter_around_integer) else mv
            for dx, dy in rules.subpel:
                cand = (centre[0] + step * dx, centre[1] + step * dy)
                c = sub(cand)
                costs.append((cand, c))
                if c < sc:
                    mv, sc = cand, c
        st['subpel_costs'], st['subpel_cost'] = costs, sc
        return mv, sc
    ic = i16_decision(p, mb, qp, rules, 'i16' in edge)[0]
    st['i16_cost'] = ic
    inter = bc
    if rules.intra_vs_subpel:
        mv, inter = refine()
    if (ic <= inter) if rules.intra_le else (ic < inter):
        return 'intra_after_search', None, st
    if not rules.intra_vs_subpel:
        mv, _ = refine()
    if rules.double_check and mv == skmv and no_levels(p, mb, mv, qp):
        return 'skip_double', mv, st
    return 'p16', mv, st


# ------------------------------------------------------------------------------------------------- the check
class Checked:
    def __init__(self):
        self.mbs = 0
        self.outcomes = {k: 0 for k in OUTCOMES}
        self.intra_kind_open = 0      # intra macroblocks of P slices: I4 / I16 not restated
        self.i16_modes = 0
        self.rows_planned = 0
        self.free_rows = 0


def _fmt_steps(st):
    return '; '.join(f'{k} {v}' for k, v in st.items())


def _found(p, mb):
    t = int(p.typ[mb])
    mv = tuple(int(v) for v in p.mv[mb])
    return {I4: 'intra (I4x4)', I16: f'intra (I16x16 mode {_i16_mode(p.syn[mb])})', P16: f'P16x16 at {mv} cbp {int(p.cbp[mb])}', PSKIP: f'P_Skip at {mv}'}[t]


def _agrees(p, mb, out, mv):
    t = int(p.typ[mb])
    if out in ('skip_judge', 'skip_double'):
        return t == PSKIP and tuple(int(v) for v in p.mv[mb]) == mv
    if out == 'p16':
        return t == P16 and tuple(int(v) for v in p.mv[mb]) == mv
    return t in (I4, I16)


def row_qps(p, rules):
    """the decision QP of every row, and for the text as stated the assertion that a row's carriers stand at it.
    -> (list of QPs or None per row where exact GOM leaves a carrier-less row open, Mismatch or None)"""
    if not p.is_p:
        return [p.slice_qp] * p.mbh, None
    if p.stream.gom:   # exact GOM is out of scope: the row's QP is the carriers', a row without one is open
        out = []
        for r in range(p.mbh):
            c = np.flatnonzero(p.carrier[r * p.mbw:(r + 1) * p.mbw])
            out.append(int(p.qp[r * p.mbw + c[0]]) if len(c) else None)
        return out, None
    plan = row_plan(p.prev_rowbits, p.slice_qp, p.window, rules)
    for r in range(p.mbh):
        c = np.flatnonzero(p.carrier[r * p.mbw:(r + 1) * p.mbw])
        if len(c) and int(p.qp[r * p.mbw + c[0]]) != plan[r]:
            mb = r * p.mbw + int(c[0])
            return plan, Mismatch(f'{p.label}: mdref ({rules.name}) != the bytes at macroblock {mb} (x {mb % p.mbw}, y {r}): the row plan gives MB row {r} QP {plan[r]} '
                                  f'(frame QP {p.slice_qp}, window {p.window}, last coded picture\'s row bits {p.prev_rowbits}), its first carrier of mb_qp_delta stands at '
                                  f'QP {int(p.qp[mb])} | code words: ' + ' | '.join(p.parsed.explain(mb)), mb, 'row_qp')
    return plan, None


def check(p, rules=None, counts=None):
    """None, or the first macroblock (address order) whose outcome in the bytes is not the one the rules demand"""
    rules = rules or Rules()
    counts = counts if counts is not None else Checked()
    if p.is_p and not p.stream.gom:
        assert p.slice_qp == p.model_qp, f'{p.label}: slice QP {p.slice_qp}, the frame-level model says {p.model_qp}'
    qps, mm = row_qps(p, rules)
    if mm is not None:
        return mm
    counts.rows_planned += p.mbh if p.is_p else 0
    for mb in range(p.nmb):
        t = int(p.typ[mb])
        head = f'{p.label}: mdref ({rules.name}) != the bytes at macroblock {mb} (x {mb % p.mbw}, y {mb // p.mbw})'
        tail = ' | code words: ' + ' | '.join(p.parsed.explain(mb))
        qrow = qps[mb // p.mbw]
        tries = [qrow] if qrow is not None else list(range(max(12, p.slice_qp - 3), min(42, p.slice_qp + 8) + 1))
        if qrow is None and mb % p.mbw == 0:
            counts.free_rows += 1
        counts.mbs += 1
        if p.is_p:
            for q in tries:
                out, mv, st = decide(p, mb, q, rules)
                if _agrees(p, mb, out, mv):
                    break
            else:
                return Mismatch(f'{head}: the rules demand {out}{"" if mv is None else " at " + str(mv)}, the bytes hold {_found(p, mb)} | steps: {_fmt_steps(st)}' + tail,
                                mb, ('outcome', out))
            counts.outcomes[out] += 1
            if t in (I4, I16):
                counts.intra_kind_open += 1
        if t == I16:
            for q in tries:
                cost, mode = i16_decision(p, mb, q, rules, 'i16' in rules.cross_edge)
                if mode == _i16_mode(p.syn[mb]):
                    break
            else:
                return Mismatch(f'{head}: Intra16x16 prediction mode {_i16_mode(p.syn[mb])} in the bytes, the first minimum of §3.3 is mode {mode} (cost {cost}, QP {q})' + tail,
                                mb, ('i16_mode', mode))
            counts.i16_modes += 1
    return None
