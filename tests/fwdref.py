"""An independent statement of the encoder's forward residual path -- TEST INFRASTRUCTURE ONLY.

Written from DESIGN.md §3.4 and tests/golden/openh264_tables.json (`quant_mf`, `quant_ff`) alone: not from the oracle's
fdct4 / quant4 / quant_dc4 nor from the kernel's xf_fwd / quant1 / quant_dc. NumPy int64 throughout, every transform a
matrix product over all blocks of a picture at once:

    4x4 forward transform    C = Cf . X . Cf^T          Cf = [[1,1,1,1],[2,1,-1,-2],[1,-1,-1,1],[1,-2,2,-1]]
    Intra16x16 luma DC       (H4 . D . H4^T + 1) >> 1   D the sixteen raw DCs as [block row, block column], >> arithmetic
    chroma DC                H2 . D . H2^T              H2 = [[1,1],[1,-1]], D the four raw DCs as [block row, block column]
    AC level                 sign(c) . (((|c| + FF[qp + 6 . intra][pos & 7]) . MF[qp][pos & 7]) >> 16), pos = 4 y + x
    DC level (both kinds)    the same with ff = int16(FF[row][0] << 1), mf = MF[qp][0] >> 1
    chroma                   at QPc of Table 8-15 (chroma_qp_index_offset is 0), typed below

The prediction is not restated here: it is what tests/reconref.py predicted for every sample when it rebuilt the picture
from the bytes (Result.pred), so Intra4x4 blocks are held against the prediction from their reconstructed neighbours.
The source is padded to the macroblock grid the way the encoder loads it: a row repeats its last sample, the last row
repeats.

frame(src, w, h, parsed, res) caches what a picture's check needs; check(fr, rules) states the levels the rules demand,
compares them and the coded_block_pattern they imply with the bytes and returns None or a Mismatch, whose message names
macroblock, plane, block, scan index, coefficient, QP, table row and column, level demanded and found and the macroblock's
code words. `rules` is a Rules(): the default is the path as §3.4 states it, MUTATIONS are single wrong readings of it.
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_T = json.load(open(os.path.join(HERE, 'golden', 'openh264_tables.json')))['tables']
MF = np.array(_T['quant_mf']['values'], np.int64).reshape(52, 8)
FF = np.array(_T['quant_ff']['values'], np.int64).reshape(58, 8)

CF = np.array([[1, 1, 1, 1], [2, 1, -1, -2], [1, -1, -1, 1], [1, -2, 2, -1]], np.int64)
H4 = np.array([[1, 1, 1, 1], [1, 1, -1, -1], [1, -1, -1, 1], [1, -1, 1, -1]], np.int64)
H2 = np.array([[1, 1], [1, -1]], np.int64)
# Table 8-15: QPc as a function of qPI
QPC = list(range(30)) + [29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39]
# Figure 8-8 / Table 8-13, frame scan: scan index -> raster position 4 y + x of the coefficient
SCAN_POS = np.array([0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15])
POS_SCAN = np.argsort(SCAN_POS)
# Figure 6-10: luma4x4BlkIdx -> raster index 4 (y / 4) + x / 4 of the block inside its macroblock
BLK_RASTER = np.array([0, 1, 4, 5, 2, 3, 6, 7, 8, 9, 12, 13, 10, 11, 14, 15])
# the quadrant (coded_block_pattern bit) of each raster block
BLK_QUAD = np.array([[(by // 2) * 2 + bx // 2 for bx in range(4)] for by in range(4)]).ravel()
# position class of a table column: 0 both coordinates even, 1 both odd, 2 otherwise (columns 8..15 repeat 0..7)
COL_CLASS = np.array([0, 2, 0, 2, 2, 1, 2, 1])
CLASS_COLS = {0: (0, 2), 1: (5, 7), 2: (1, 3, 4, 6)}
KINDS = ('luma AC', 'chroma AC', 'I16 luma DC', 'chroma DC')
LUMA_AC, CHROMA_AC, I16_DC, CHROMA_DC = range(4)
I4, I16, P16, PSKIP = 0, 1, 2, 3
TYPE_NAMES = {0: 'I4x4', 1: 'I16x16', 2: 'P16x16', 3: 'P_Skip'}


class Rules:
    """the switches a mutation turns; the default is the path as DESIGN.md §3.4 states it"""

    def __init__(self, name='as stated', **kw):
        self.name = name
        self.ff_delta = None          # (kind, FF row, position class, +-1): one cell of one kind's rounding table moved
        self.mf_swap = False          # MF column of position class 1 <-> class 2
        self.pos_is_scan = False      # table column from the scan index instead of the raster position
        self.intra_offset = (0, 6)    # FF row offset of (inter, intra) blocks
        self.floor_negative = False   # negative c: (-(|c| + FF) * MF) >> 16, rounding toward minus infinity
        self.dc_as_ac = False         # DC quantiser with the AC's ff and mf
        self.i16dc_round = 'shift'    # (x + 1) >> 1 | 'noround': x >> 1 | 'trunc': (x + 1) / 2 truncating
        self.swap_transforms = False  # Cf^T . X . Cf
        self.chroma_at_qpy = False
        self.chroma_dc_transposed = False
        self.pad = 'repeat'           # 'zero' | 'mirror'
        self.cbp_neighbour = False    # a luma CBP bit taken from the quadrant beside it
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


# the fixed list; tests/fwdaudit.py adds the two FF mutations of every selectable cell
MUTATIONS = [
    Rules('MF column swapped between position classes 1 and 2', mf_swap=True),
    Rules('pos & 7 replaced by the scan index', pos_is_scan=True),
    Rules('intra row offset 6 dropped', intra_offset=(0, 0)),
    Rules('intra row offset 6 applied to inter', intra_offset=(6, 6)),
    Rules('negative c rounded toward minus infinity (>> on the signed value)', floor_negative=True),
    Rules('DC quantiser with the AC\'s ff / mf', dc_as_ac=True),
    Rules('I16 DC (x + 1) >> 1 as x >> 1', i16dc_round='noround'),
    Rules('I16 DC (x + 1) >> 1 as truncating division', i16dc_round='trunc'),
    Rules('row and column transforms exchanged', swap_transforms=True),
    Rules('chroma quantised at QPY', chroma_at_qpy=True),
    Rules('chroma DC order transposed', chroma_dc_transposed=True),
    Rules('source padded by zero', pad='zero'),
    Rules('source padded by mirror', pad='mirror'),
    Rules('a CBP bit taken from the neighbouring quadrant', cbp_neighbour=True),
]


def pad_source(src, w, h, how='repeat'):
    """tight I420 of w x h -> (Y, U, V) int64 on the macroblock grid"""
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    src = np.asarray(src, np.uint8).ravel()
    assert src.size == w * h * 3 // 2
    cw, ch = w // 2, h // 2
    tight = [src[:w * h].reshape(h, w), src[w * h:w * h + cw * ch].reshape(ch, cw), src[w * h + cw * ch:].reshape(ch, cw)]
    out = []
    for k, a in enumerate(tight):
        H, W = (16 * mbh, 16 * mbw) if k == 0 else (8 * mbh, 8 * mbw)
        a = a.astype(np.int64)
        if how == 'repeat':       # a row repeats its last sample, the last row repeats
            ys, xs = np.minimum(np.arange(H), a.shape[0] - 1), np.minimum(np.arange(W), a.shape[1] - 1)
            p = a[ys][:, xs]
        elif how == 'mirror':
            ys, xs = np.arange(H), np.arange(W)
            ys = np.where(ys < a.shape[0], ys, 2 * a.shape[0] - 1 - ys)
            xs = np.where(xs < a.shape[1], xs, 2 * a.shape[1] - 1 - xs)
            p = a[ys][:, xs]
        else:
            p = np.zeros((H, W), np.int64)
            p[:a.shape[0], :a.shape[1]] = a
        out.append(p)
    return out


def _blocks(plane, mbw, mbh, n):
    """a plane on the macroblock grid -> [macroblock, n x n blocks in raster order, y, x]"""
    return plane.reshape(mbh, n, 4, mbw, n, 4).transpose(0, 3, 1, 4, 2, 5).reshape(mbw * mbh, n * n, 4, 4)


def forward(x, swap=False):
    """Cf . X . Cf^T over the last two axes ([..., y, x])"""
    return (CF.T @ x @ CF) if swap else (CF @ x @ CF.T)


def quant(c, ff, mf, floor_negative=False):
    """sign(c) . (((|c| + ff) . mf) >> 16)"""
    a = (np.abs(c) + ff) * mf
    if floor_negative:
        return np.where(c < 0, (-a) >> 16, a >> 16)
    return np.sign(c) * (a >> 16)


def dc_params(ff_row0, mf0):
    """both DC kinds: ff = int16(FF[row][0] << 1), mf = MF[qp][0] >> 1"""
    ff = (np.asarray(ff_row0, np.int64) << 1).astype(np.int16).astype(np.int64)
    return ff, np.asarray(mf0, np.int64) >> 1


class Frame:
    """what one picture's check needs, cached: the source, the prediction, the macroblocks' types, QPs and patterns and
    the levels the bytes carry, as arrays over the whole picture"""


def frame(src, w, h, parsed, res, label=''):
    """src: the tight I420 source at the coded-from size; parsed: parseref.Parsed; res: reconref.Result with .pred"""
    f = Frame()
    f.label, f.src, f.w, f.h, f.parsed = label, np.asarray(src, np.uint8).ravel().copy(), w, h, parsed
    mbw, mbh = parsed.geometry
    assert (mbw, mbh) == ((w + 15) // 16, (h + 15) // 16), 'the bytes are not of the source\'s geometry'
    nmb = mbw * mbh
    f.mbw, f.mbh, f.nmb = mbw, mbh, nmb
    f.pred = [np.asarray(p, np.int64) for p in res.pred]
    syn = np.asarray(parsed.syntax, np.int64).reshape(nmb, -1)
    rec = np.asarray(res.records, np.int64)
    f.typ, f.qp = rec[:, 0].copy(), rec[:, 1].copy()
    assert np.isin(f.typ, (I4, I16, P16, PSKIP)).all(), 'a macroblock type the encoder does not write'
    assert (rec[:, 58] == 0).all(), 'chroma_qp_index_offset is 0 in every PPS the encoder writes'
    f.mv = rec[:, 22:24].copy()
    f.skip_mv = dict(res.skip_mv)
    # coded_block_pattern: parsed for I4 / P16, from mb_type for I16 (Table 7-11), none for P_Skip
    it = np.where(syn[:, 1] == 0, syn[:, 0] - 5, syn[:, 0])
    i16cbp = np.where(it >= 13, 15, 0) | ((((it - 1) // 4) % 3) << 4)
    f.cbp = np.where(f.typ == I16, i16cbp, np.where(f.typ == PSKIP, 0, syn[:, 71]))
    # The QP a macroblock was quantised at (§3.6). One that carries mb_qp_delta says it; one that does not (Intra4x4 or
    # P16x16 with pattern 0) was quantised at its row's QP all the same, which the bytes show at the row's carriers: every
    # carrier of a row stands at the row's QP. In a row without a carrier the QP is not in the bytes (`free`).
    carrier = (f.typ == I16) | ((f.typ != PSKIP) & (f.cbp != 0))
    f.qe, f.free = f.qp.copy(), np.zeros(nmb, bool)
    f.slice_qp = syn[:, 73].copy()
    for r in range(mbh):
        row = slice(r * mbw, (r + 1) * mbw)
        c = np.flatnonzero(carrier[row])
        quiet = (f.typ[row] != PSKIP) & ~carrier[row]
        if len(c):
            assert (f.qp[row][c] == f.qp[row][c[0]]).all(), 'the carriers of one macroblock row stand at different QPs'
            f.qe[row] = np.where(quiet, f.qp[row][c[0]], f.qp[row])
        else:
            f.free[row] = quiet
    # the levels in the bytes, at their coefficient positions: luma [MB, raster block, 4 y + x]
    scan = syn[:, 96:352].reshape(nmb, 16, 16).copy()
    is16 = f.typ == I16
    scan[is16] = np.concatenate([np.zeros((int(is16.sum()), 16, 1), np.int64), scan[is16][:, :, :15]], axis=2)
    luma = np.zeros((nmb, 16, 16), np.int64)
    luma[:, BLK_RASTER[:, None], SCAN_POS[None, :]] = scan
    f.luma = luma.reshape(nmb, 16, 4, 4)
    dc = np.zeros((nmb, 16), np.int64)
    dc[:, SCAN_POS] = syn[:, 80:96]
    f.i16dc = dc.reshape(nmb, 4, 4)
    f.cdc = syn[:, 352:360].reshape(nmb, 2, 2, 2).copy()                 # [MB, plane, block row, block column]
    cac = np.zeros((nmb, 2, 4, 16), np.int64)
    cac[:, :, :, SCAN_POS[1:]] = syn[:, 360:488].reshape(nmb, 2, 4, 16)[:, :, :, :15]
    f.cac = cac.reshape(nmb, 2, 4, 4, 4)
    return f


class Mismatch:
    def __init__(self, message, mb, what):
        self.message, self.mb, self.what = message, mb, what

    def __str__(self):
        return self.message


def _tables(rules):
    """per kind the FF table, and the MF table, as the rules read them"""
    ff = [FF.copy() for _ in KINDS]
    if rules.ff_delta is not None:
        kind, row, cls, d = rules.ff_delta
        for c in CLASS_COLS[cls]:
            ff[kind][row, c] += d
    mf = MF.copy()
    if rules.mf_swap:
        mf[:, [5, 7]] = MF[:, [1, 1]]
        mf[:, [1, 3, 4, 6]] = MF[:, [5, 5, 5, 5]]
    return ff, mf


def transform(fr, rules):
    """-> the coefficients of every block: luma [MB, 16, 4, 4], chroma [MB, 2, 4, 4, 4]"""
    Y, U, V = pad_source(fr.src, fr.w, fr.h, rules.pad)
    cy = forward(_blocks(Y - fr.pred[0], fr.mbw, fr.mbh, 4), rules.swap_transforms)
    cc = np.stack([forward(_blocks(p - q, fr.mbw, fr.mbh, 2), rules.swap_transforms) for p, q in ((U, fr.pred[1]), (V, fr.pred[2]))], axis=1)
    return cy, cc


def demand(fr, rules, coef=None, qe=None):
    """the levels the rules demand of every macroblock, with what went into each: dict of arrays
    luma, i16dc, cdc, cac (levels), c_* (coefficients), and per kind qp / row / col"""
    cy, cc = coef if coef is not None else transform(fr, rules)
    ffs, mf = _tables(rules)
    nmb = fr.nmb
    intra = (fr.typ == I4) | (fr.typ == I16)
    off = np.where(intra, rules.intra_offset[1], rules.intra_offset[0])
    pos = np.arange(16)
    col = ((POS_SCAN[pos] if rules.pos_is_scan else pos) & 7).reshape(4, 4)
    qp = fr.qe if qe is None else qe
    qpc = qp if rules.chroma_at_qpy else np.array(QPC, np.int64)[qp]
    out = dict(qp=qp, qpc=qpc, intra=intra, col=col)
    # luma AC
    row = qp + off
    out['luma'] = quant(cy, ffs[LUMA_AC][row[:, None, None, None], col], mf[qp[:, None, None, None], col], rules.floor_negative)
    out['luma'][fr.typ == I16, :, 0, 0] = 0
    out['c_luma'], out['row'] = cy, row
    # I16 luma DC
    raw = cy[:, :, 0, 0].reshape(nmb, 4, 4)
    had = H4 @ raw @ H4.T
    if rules.i16dc_round == 'shift':
        had = (had + 1) >> 1
    elif rules.i16dc_round == 'noround':
        had = had >> 1
    else:
        had = np.sign(had + 1) * (np.abs(had + 1) // 2)
    if rules.dc_as_ac:
        ff, m = ffs[I16_DC][row, 0], mf[qp, 0]
    else:
        ff, m = dc_params(ffs[I16_DC][row, 0], mf[qp, 0])
    out['i16dc'] = quant(had, ff[:, None, None], m[:, None, None], rules.floor_negative)
    out['c_i16dc'], out['raw_i16dc'] = had, raw
    # chroma
    rowc = qpc + off
    out['cac'] = quant(cc, ffs[CHROMA_AC][rowc[:, None, None, None, None], col], mf[qpc[:, None, None, None, None], col], rules.floor_negative)
    out['cac'][:, :, :, 0, 0] = 0
    out['c_cac'], out['rowc'] = cc, rowc
    rawc = cc[:, :, :, 0, 0].reshape(nmb, 2, 2, 2)
    hc = H2 @ rawc @ H2.T
    if rules.chroma_dc_transposed:
        hc = np.swapaxes(hc, -1, -2)
    if rules.dc_as_ac:
        ff, m = ffs[CHROMA_DC][rowc, 0], mf[qpc, 0]
    else:
        ff, m = dc_params(ffs[CHROMA_DC][rowc, 0], mf[qpc, 0])
    out['cdc'] = quant(hc, ff[:, None, None, None], m[:, None, None, None], rules.floor_negative)
    out['c_cdc'], out['raw_cdc'] = hc, rawc
    # the coded_block_pattern the levels imply (§3.8: the quantiser's levels go to the CBP as they are)
    nzq = np.zeros((nmb, 4), bool)
    nzb = (out['luma'] != 0).any(axis=(2, 3))
    for q in range(4):
        nzq[:, q ^ 1 if rules.cbp_neighbour else q] = nzb[:, BLK_QUAD == q].any(axis=1)
    lum = (nzq * (1 << np.arange(4))).sum(axis=1)
    lum = np.where(fr.typ == I16, np.where(nzb.any(axis=1), 15, 0), lum)
    anyac, anydc = (out['cac'] != 0).any(axis=(1, 2, 3, 4)), (out['cdc'] != 0).any(axis=(1, 2, 3))
    out['cbp'] = lum | (np.where(anyac, 2, np.where(anydc, 1, 0)) << 4)
    return out


def structure(fr):
    """the rules that need no transform: the pattern in the bytes against the levels in the bytes, the double check,
    the vectors' range -> None or a Mismatch"""
    for mb in np.flatnonzero(fr.typ != PSKIP):
        mb = int(mb)
        t, cbp = int(fr.typ[mb]), int(fr.cbp[mb])
        nzb = (fr.luma[mb] != 0).any(axis=(1, 2))
        if t == I16:
            want = 15 if nzb.any() else 0
        else:
            want = sum(1 << q for q in range(4) if nzb[BLK_QUAD == q].any())
        anyac, anydc = bool((fr.cac[mb] != 0).any()), bool((fr.cdc[mb] != 0).any())
        want |= (2 if anyac else (1 if anydc else 0)) << 4
        if want != cbp:
            return Mismatch(f'{fr.label}: macroblock {mb} (x {mb % fr.mbw}, y {mb // fr.mbw}) {TYPE_NAMES[t]}: coded_block_pattern {cbp} in the bytes, '
                            f'but the levels in the bytes give {want} (a set bit without a level) | ' + ' | '.join(fr.parsed.explain(mb)), mb, 'cbp_bytes')
        if t == P16:
            mv = (int(fr.mv[mb, 0]), int(fr.mv[mb, 1]))
            if cbp == 0 and mv == tuple(fr.skip_mv[mb]):
                return Mismatch(f'{fr.label}: macroblock {mb} (x {mb % fr.mbw}, y {mb // fr.mbw}) is a P16x16 without residual at the skip vector {mv}: '
                                f'the double check makes it a P_Skip | ' + ' | '.join(fr.parsed.explain(mb)), mb, 'double_check')
            if max(abs(mv[0]), abs(mv[1])) > 67:   # 4 x (-16..16) + half step + quarter step
                return Mismatch(f'{fr.label}: macroblock {mb} vector {mv}: integer part outside -16..16', mb, 'mv_range')
    return None


def _first(mask):
    idx = np.argwhere(mask)
    return tuple(int(v) for v in idx[0]) if len(idx) else None


def check(fr, rules=None, coef=None, d=None):
    """None, or the first disagreement (macroblock order) between the levels and pattern the rules demand and the bytes"""
    rules = rules or Rules()
    d = d if d is not None else demand(fr, rules, coef)
    coded = fr.typ != PSKIP
    is16 = fr.typ == I16
    bad = np.zeros(fr.nmb, bool)
    ne = {'cbp': (d['cbp'] != fr.cbp) & coded,
          'i16dc': (d['i16dc'] != fr.i16dc) & is16[:, None, None],
          'luma': (d['luma'] != fr.luma) & coded[:, None, None, None],
          'cdc': (d['cdc'] != fr.cdc) & coded[:, None, None, None],
          'cac': (d['cac'] != fr.cac) & coded[:, None, None, None, None]}
    for k, m in ne.items():
        bad |= m.reshape(fr.nmb, -1).any(axis=1)
    if (bad & fr.free).any() and rules.name == 'as stated':
        # a row without a carrier: the levels must vanish at one QP the row plan or the GOM rule can give the row
        # (slice QP - 3 .. + 8 inside 12..42, §3.6); a mutation is not given this freedom twice, it is held to the others
        sq = int(fr.slice_qp[np.flatnonzero(bad & fr.free)[0]])
        for q in range(max(12, sq - 3), min(42, sq + 8) + 1):
            alt = demand(fr, rules, coef, np.where(fr.free, q, fr.qe))
            ok = fr.free & (alt['cbp'] == 0)
            bad &= ~ok
    if not bad.any():
        return None
    mb = int(np.flatnonzero(bad)[0])
    rowqp = f" (the row's; QPY in the bytes {int(fr.qp[mb])})" if fr.qe[mb] != fr.qp[mb] else ''
    head = (f'{fr.label}: fwdref ({rules.name}) != the bytes at macroblock {mb} (x {mb % fr.mbw}, y {mb // fr.mbw}) {TYPE_NAMES[int(fr.typ[mb])]} '
            f'QP {int(fr.qe[mb])}{rowqp} QPc {int(d["qpc"][mb])} cbp {int(fr.cbp[mb])}')
    tail = ' | code words: ' + ' | '.join(fr.parsed.explain(mb))
    col = d['col']

    def cell(kind, row, y, x, dc):
        c = 0 if dc else int(col[y, x])
        return f'table row {int(row)} ({"intra" if d["intra"][mb] else "inter"}), column {c} (position class {int(COL_CLASS[c])}), kind {KINDS[kind]}'

    if ne['i16dc'][mb].any():
        y, x = _first(ne['i16dc'][mb])
        return Mismatch(f'{head}: plane Y, Intra16x16 DC block, scan index {int(POS_SCAN[4 * y + x])} (position x {x}, y {y}), coefficient {int(d["c_i16dc"][mb, y, x])} '
                        f'(Hadamard of the raw DCs, (x + 1) >> 1), {cell(I16_DC, d["row"][mb], y, x, True)}: level demanded {int(d["i16dc"][mb, y, x])}, '
                        f'found {int(fr.i16dc[mb, y, x])}' + tail, mb, ('i16dc', y, x))
    if ne['luma'][mb].any():
        b, y, x = _first(ne['luma'][mb])
        return Mismatch(f'{head}: plane Y, block {b} (raster; x {4 * (b % 4)}, y {4 * (b // 4)}), scan index {int(POS_SCAN[4 * y + x])} (position x {x}, y {y}), '
                        f'coefficient {int(d["c_luma"][mb, b, y, x])}, {cell(LUMA_AC, d["row"][mb], y, x, False)}: level demanded {int(d["luma"][mb, b, y, x])}, '
                        f'found {int(fr.luma[mb, b, y, x])}' + tail, mb, ('luma', b, y, x))
    if ne['cdc'][mb].any():
        p, y, x = _first(ne['cdc'][mb])
        return Mismatch(f'{head}: plane {"UV"[p]}, chroma DC block, scan index {2 * y + x}, coefficient {int(d["c_cdc"][mb, p, y, x])} (2x2 transform of the raw DCs), '
                        f'{cell(CHROMA_DC, d["rowc"][mb], y, x, True)}: level demanded {int(d["cdc"][mb, p, y, x])}, found {int(fr.cdc[mb, p, y, x])}' + tail, mb, ('cdc', p, y, x))
    if ne['cac'][mb].any():
        p, b, y, x = _first(ne['cac'][mb])
        return Mismatch(f'{head}: plane {"UV"[p]}, block {b} (raster; x {4 * (b % 2)}, y {4 * (b // 2)}), scan index {int(POS_SCAN[4 * y + x])} (position x {x}, y {y}), '
                        f'coefficient {int(d["c_cac"][mb, p, b, y, x])}, {cell(CHROMA_AC, d["rowc"][mb], y, x, False)}: level demanded {int(d["cac"][mb, p, b, y, x])}, '
                        f'found {int(fr.cac[mb, p, b, y, x])}' + tail, mb, ('cac', p, b, y, x))
    return Mismatch(f'{head}: every level agrees, but the levels demand coded_block_pattern {int(d["cbp"][mb])}' + tail, mb, ('cbp',))


def check_frame(src, w, h, parsed, res, label=''):
    """the whole check of one picture -> (Frame, None or Mismatch)"""
    fr = frame(src, w, h, parsed, res, label)
    return fr, (structure(fr) or check(fr))
