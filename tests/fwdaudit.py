"""Cell audit of the encoder's forward residual path -- TEST INFRASTRUCTURE ONLY.

tests/fwdref.py states the path; this module says which cells of the quantiser's tables the content pins. A cell is
(kind, QP of the MF row, inter / intra, position class): one FF entry as one kind of block reads it. Content pins a cell
when it reads the cell's FF within one of a rounding boundary on both sides: some coefficient has |c| exactly at a
threshold (the smallest value giving level n >= 1) and some coefficient has |c| exactly one below a threshold, so that
fwdref with the cell's FF moved by -1 and by +1 each disagrees with the bytes. Counting reads decisions and makes none.

    python tests/fwdaudit.py sweep     the seeded sweep and the greedy cover that chose DIRECTED (CPU, oracle encoder)
"""
import functools
import itertools
from collections import Counter

import numpy as np

import dbkref
import encaudit
import fwdref
import parseref
import reconref
from fwdref import LUMA_AC, CHROMA_AC, I16_DC, CHROMA_DC, I4, I16, P16, PSKIP, FF, MF, QPC

KIND_LETTER = 'YCDE'     # luma AC, chroma AC, I16 luma DC, chroma DC


def cell_name(cell):
    kind, qp, intra, cls = cell
    return f'{KIND_LETTER[kind]}{qp}{"i" if intra else "p"}{cls}'


def cell_of(name):
    return (KIND_LETTER.index(name[0]), int(name[1:-2]), int(name[-2] == 'i'), int(name[-1]))


def all_cells():
    """the table: every QP 0..51 for luma, every value of Table 8-15 for chroma; AC kinds read the three position
    classes, DC kinds column 0 alone; the Intra16x16 DC exists for intra only"""
    qpcs = sorted(set(QPC))
    out = [(LUMA_AC, q, i, c) for q in range(52) for i in (0, 1) for c in range(3)]
    out += [(CHROMA_AC, q, i, c) for q in qpcs for i in (0, 1) for c in range(3)]
    out += [(I16_DC, q, 1, 0) for q in range(52)]
    out += [(CHROMA_DC, q, i, 0) for q in qpcs for i in (0, 1)]
    return out


# The QPs the encoder can select (§3.6). A P frame's QP is clipped to [last - 3, last + 5] inside [12, 42]; the row plan
# and the exact GOM rule clip every row's QP to that window again, so every inter block is quantised at 12..42. An IDR's
# QP is clipped to its bitrate column's range of rc_qp_range, together 22..40, and I slices keep the frame QP; an intra
# macroblock of a P slice is quantised at its row's QP, so intra blocks are quantised at 12..42 as well, 12..21 and
# 41..42 of them in P slices only. chroma_qp_index_offset is 0, so chroma is quantised at Table 8-15 of 12..42: 12..37.
LUMA_QPS = range(12, 43)
CHROMA_QPS = sorted({QPC[q] for q in LUMA_QPS})
_WHY_LUMA = ('no block is quantised at this QP: a P frame\'s QP and every row QP inside it are clipped to a window inside 12..42 '
             '(rc_* FRAME_DQP window, row plan and GOM rule clip to it), an IDR\'s QP to its rc_qp_range column, 22..40 together')
_WHY_CHROMA = 'chroma is quantised at Table 8-15 of the luma QP, and the luma QP lies in 12..42 (see the luma cells): QPc lies in 12..37'


def selectable():
    return [c for c in all_cells() if c[1] in (LUMA_QPS if c[0] in (LUMA_AC, I16_DC) else CHROMA_QPS)]


def excluded():
    sel = set(selectable())
    return {c: (_WHY_LUMA if c[0] in (LUMA_AC, I16_DC) else _WHY_CHROMA) for c in all_cells() if c not in sel}


# The int16 wrap of FF << 1 is never taken: the largest FF of column 0 is 299, doubled 598 (derived from the table below).
assert int(FF[:, 0].max()) << 1 < 32768

CLASSES = ('level_negative', 'level_positive', 'abs_level_1', 'abs_level_2_15', 'abs_level_ge16', 'i16dc_round_negative_odd',
           'raw_dc_plus_4080', 'raw_dc_minus_4080', 'hadamard_sum_extreme', 'qpc_ne_qpy', 'padded_columns_in_block', 'padded_rows_in_block',
           'cbp_clear_beside_set', 'ff_doubled_no_wrap')
CLASS_EXCLUDED = {'ff_doubled_wraps': 'FF << 1 as int16 wraps only above 16383; column 0 of quant_ff holds at most 299 (asserted on the table)'}


def _levels(a, ff, mf):
    return ((a + ff) * mf) >> 16


def count(fr, d=None):
    """one picture -> (pins: {cell: [at a threshold, one below a threshold]}, Counter of residual-path classes).
    Only coefficients whose quantisation QP the bytes show are counted (not P_Skip, not a row without a carrier)."""
    d = d or fwdref.demand(fr, fwdref.Rules())
    ok = (fr.typ != PSKIP) & ~fr.free
    is16 = ok & (fr.typ == I16)
    col = d['col']
    cls = fwdref.COL_CLASS[col]
    intra = d['intra'].astype(np.int64)
    notdc = np.ones((4, 4), bool)
    notdc[0, 0] = False
    groups = []
    # (kind, |c|, levels, QP, FF row, column, class, intra, mask), broadcast to the coefficients' shape
    sh = d['c_luma'].shape
    b4 = lambda v: np.broadcast_to(v[:, None, None, None], sh)
    groups.append((LUMA_AC, d['c_luma'], d['luma'], b4(d['qp']), b4(d['row']), np.broadcast_to(col, sh), np.broadcast_to(cls, sh), b4(intra),
                   b4(ok) & (np.broadcast_to(notdc, sh) | ~b4(fr.typ == I16)), None))
    sh = d['c_cac'].shape
    b5 = lambda v: np.broadcast_to(v[:, None, None, None, None], sh)
    groups.append((CHROMA_AC, d['c_cac'], d['cac'], b5(d['qpc']), b5(d['rowc']), np.broadcast_to(col, sh), np.broadcast_to(cls, sh), b5(intra),
                   b5(ok) & np.broadcast_to(notdc, sh), None))
    sh = d['c_i16dc'].shape
    b3 = lambda v: np.broadcast_to(v[:, None, None], sh)
    z = np.zeros(sh, np.int64)
    groups.append((I16_DC, d['c_i16dc'], d['i16dc'], b3(d['qp']), b3(d['row']), z, z, b3(intra), b3(is16), 'dc'))
    sh = d['c_cdc'].shape
    b4c = lambda v: np.broadcast_to(v[:, None, None, None], sh)
    z = np.zeros(sh, np.int64)
    groups.append((CHROMA_DC, d['c_cdc'], d['cdc'], b4c(d['qpc']), b4c(d['rowc']), z, z, b4c(intra), b4c(ok), 'dc'))
    pins, cl = {}, Counter()
    for kind, c, lv, qp, row, cc, kk, it, mask, dc in groups:
        m = mask.ravel()
        if not m.any():
            continue
        a, lv, qp, row, cc, kk, it = (np.asarray(v).ravel()[m] for v in (np.abs(c), lv, qp, row, cc, kk, it))
        ff, mf = FF[row, cc], MF[qp, cc]
        if dc:
            ff, mf = fwdref.dc_params(ff, mf)
        l0 = _levels(a, ff, mf)
        assert (l0 == np.abs(lv)).all()
        at = (a >= 1) & (l0 >= 1) & (_levels(a - 1, ff, mf) < l0)
        below = _levels(a + 1, ff, mf) > l0
        key = ((qp * 2 + it) * 3 + kk)
        for side, hit in ((0, at), (1, below)):
            for k in np.unique(key[hit]):
                k = int(k)
                pins.setdefault((kind, k // 6, (k // 3) % 2, k % 3), [False, False])[side] = True
        cl['level_negative'] += int((lv < 0).sum())
        cl['level_positive'] += int((lv > 0).sum())
        cl['abs_level_1'] += int((l0 == 1).sum())
        cl['abs_level_2_15'] += int(((l0 >= 2) & (l0 <= 15)).sum())
        cl['abs_level_ge16'] += int((l0 >= 16).sum())
        if dc:
            cl['ff_doubled_no_wrap'] += int(m.sum())
            cl['ff_doubled_wraps'] += int(((FF[row, cc] << 1) > 32767).sum())
    if is16.any():
        raw = d['raw_i16dc'][is16]
        had = fwdref.H4 @ raw @ fwdref.H4.T
        cl['i16dc_round_negative_odd'] += int(((had < 0) & (had % 2 == 1)).sum())
        cl['raw_dc_plus_4080'] += int((raw == 4080).sum())
        cl['raw_dc_minus_4080'] += int((raw == -4080).sum())
        cl['hadamard_sum_extreme'] += int((np.abs(had) == 16 * 4080).sum())
    cl['qpc_ne_qpy'] += int((ok & (d['qpc'] != d['qp'])).sum())
    mbx, mby = np.arange(fr.nmb) % fr.mbw, np.arange(fr.nmb) // fr.mbw
    if fr.w % 16:
        cl['padded_columns_in_block'] += int((ok & (mbx == fr.mbw - 1)).sum())
    if fr.h % 16:
        cl['padded_rows_in_block'] += int((ok & (mby == fr.mbh - 1)).sum())
    lum = fr.cbp & 15
    cl['cbp_clear_beside_set'] += int((ok & (fr.typ != I16) & (lum != 0) & (lum != 15)).sum())
    return pins, cl


def chain(clip, units, label=None):
    """the bytes of one clip, one access unit per frame -> per frame (Frame, None or fwdref.Mismatch, deblocked planes);
    parseref -> reconref (with the prediction) -> dbkref carries the reference from frame to frame"""
    state, prev, out = parseref.State(), None, []
    for t, au in enumerate(units):
        if not au:      # a frame the rate control skipped
            continue
        p = parseref.parse(au, state)
        res = reconref.reconstruct(p.syntax, p.geometry, prev)
        prev = dbkref.deblock(res.planes, res.records).planes
        fr, mm = fwdref.check_frame(clip.frames[t], clip.w, clip.h, p, res, f'{label or clip.name} frame {t}')
        out.append((fr, mm, prev))
    return out


def suite_inputs(oracle, limit=352 * 288):
    """what the GPU tests fed the encoder before this audit, up to 352x288 and 40 frames (the Python chain is too slow
    for more): encaudit.suite_clips' small clips and the directed inputs of §3.8, §3.9 and §3.10"""
    import rcaudit
    import writeaudit
    out = list(encaudit.suite_clips(oracle)[0]) + list(encaudit.directed_clips())
    out += [c for c in writeaudit.directed_clips() if c.w * c.h <= limit]
    out += [encaudit.Clip('rc_' + s.name, s.w, s.h, s.br, s.frames(), skip=s.skip, idr=s.idr) for s in rcaudit.directed_seqs() if s.w * s.h <= limit and len(s) <= 40]
    return [c for c in out if c.w * c.h <= limit]


def count_frames(frames):
    """chain()'s frames -> (cells pinned on both sides, pins, classes)"""
    pins, cl = {}, Counter()
    for fr, _, _ in frames:
        p, c = count(fr)
        for k, v in p.items():
            e = pins.setdefault(k, [False, False])
            e[0] |= v[0]
            e[1] |= v[1]
        cl.update(c)
    return {k for k, v in pins.items() if v[0] and v[1]}, pins, cl


def ff_mutations(cells):
    return [fwdref.Rules(f'FF of cell {cell_name(c)} {d:+d}', ff_delta=(c[0], c[1] + 6 * c[2], c[3], d)) for c in cells for d in (-1, 1)]


def catches(frames, rules):
    """the first frame of chain()'s frames on which the mutated rules disagree with the bytes -> Mismatch or None"""
    for fr, _, _ in frames:
        mm = fwdref.check(fr, rules)
        if mm:
            return mm
    return None


# ---------------------------------------------------------------- directed content
def gen(kind, w, h, n, seed, amp):
    """n frames of tight I420.
    noise    fresh uniform noise of amplitude amp around 128 in every frame (intra and inter macroblocks mixed)
    low      a static seeded texture with fresh noise of amplitude amp (levels of +-1 near the dead zone)
    cells    0 / 255 cells of amp x amp samples, fresh in every frame (extreme DCs)
    checker  a 0 / 255 checker of period amp that moves one sample a frame
    shift    the seeded texture of encaudit.planes seen at a quarter-sample offset growing by (seed % 7 + 1, seed % 5) a frame
    stripes  columns of random values, fresh in every frame, with noise of amplitude amp: vertical prediction wins in P slices
    """
    rng = np.random.default_rng(seed * 1000 + 17)
    cw, ch = w // 2, h // 2
    out = []
    W, H = (w + 15) & ~15, (h + 15) & ~15
    base = None
    for t in range(n):
        if kind == 'noise':
            p = [rng.integers(128 - amp, 128 + amp + 1, s) for s in ((h, w), (ch, cw), (ch, cw))]
        elif kind == 'low':
            if base is None:
                base = [np.kron(rng.integers(60, 200, ((s[0] + 3) // 4, (s[1] + 3) // 4)), np.ones((4, 4), np.int64))[:s[0], :s[1]] for s in ((h, w), (ch, cw), (ch, cw))]
            p = [b + (rng.integers(-amp, amp + 1, b.shape) if t else 0) for b in base]
        elif kind == 'cells':
            p = [np.kron(rng.integers(0, 2, ((s[0] + amp - 1) // amp, (s[1] + amp - 1) // amp)) * 255, np.ones((amp, amp), np.int64))[:s[0], :s[1]]
                 for s in ((h, w), (ch, cw), (ch, cw))]
        elif kind == 'checker':
            p = []
            for s in ((h, w), (ch, cw), (ch, cw)):
                yy, xx = np.mgrid[0:s[0], 0:s[1]]
                p.append((((xx + t) // amp + yy // amp) & 1) * 255)
        elif kind == 'shift':
            y, u, v = encaudit.planes(seed, W, H, (seed % 7 + 1) * t, (seed % 5) * t)
            p = [y[:h, :w].astype(np.int64) + rng.integers(-amp, amp + 1, (h, w)), u[:ch, :cw], v[:ch, :cw]]
        elif kind == 'stripes':
            p = [np.broadcast_to(rng.integers(20, 236, (1, s[1])), s) + rng.integers(-amp, amp + 1, s) for s in ((h, w), (ch, cw), (ch, cw))]
        else:
            raise ValueError(kind)
        out.append(encaudit.pack([np.clip(a, 0, 255) for a in p]))
    return out


def spec_clip(spec, targets=(), classes=()):
    """(kind, w, h, frames, seed, amp, bitrate, forced IDRs) -> encaudit.Clip; frame skipping off, so the QPs hold"""
    kind, w, h, n, seed, amp, br, idr = spec
    c = encaudit.Clip(f'{kind}_{w}x{h}_{n}f_s{seed}_a{amp}_{br}' + ('_idr' + '_'.join(map(str, idr)) if idr else ''), w, h, br, gen(kind, w, h, n, seed, amp), idr=idr,
                      targets=tuple(targets))
    c.classes = tuple(classes)
    return c


GEOMETRIES = [(16, 16), (16, 48), (48, 16), (48, 48), (80, 48), (18, 18), (50, 34)]

# DIRECTED and NOT_PINNED are written by `python tests/fwdaudit.py sweep` (the greedy cover) and pasted here.
# (kind, w, h, frames, seed, amp, bitrate, forced IDRs), the cells the clip is the first to pin on both sides, the classes
# and the fixed mutations it is the first to reach / catch
DIRECTED = [
    (('noise', 50, 34, 8, 998, 120, 6000000, ()),
     'C12i0 C12i1 C12i2 C12p0 C12p2 C13i0 C13i1 C13i2 C13p0 C13p2 C14i0 C14i1 C14i2 C14p0 C14p2 C16p2 C17i0 C17i1 C17i2 C19i0 C19i1 C19i2 C19p2 C21p0 C21p2 C22i0 C22i1 C22i2 C23i0 C23i1 C23i2 D12i0 D14i0 E12i0 E12p0 E13i0 E14i0 E17i0 E19i0 Y12i0 Y12i1 Y12i2 Y12p0 Y12p1 Y12p2 Y13i0 Y13i1 Y13i2 Y13p0 Y13p1 Y13p2 Y14i0 Y14i1 Y14i2 Y14p0 Y14p1 Y14p2 Y16i2 Y16p0 Y16p2 Y17i0 Y17i1 Y17i2 Y19i0 Y19i1 Y19i2 Y19p0 Y19p1 Y19p2 Y21p0 Y21p1 Y21p2 Y22i0 Y22i1 Y22i2 Y23i0 Y23i1 Y23i2 Y23p0',
     ["DC quantiser with the AC's ff / mf", 'I16 DC (x + 1) >> 1 as truncating division', 'I16 DC (x + 1) >> 1 as x >> 1', 'MF column swapped between position classes 1 and 2', 'a CBP bit taken from the neighbouring quadrant', 'abs_level_1', 'abs_level_2_15', 'abs_level_ge16', 'cbp_clear_beside_set', 'chroma DC order transposed', 'ff_doubled_no_wrap', 'i16dc_round_negative_odd', 'intra row offset 6 applied to inter', 'intra row offset 6 dropped', 'level_negative', 'level_positive', 'negative c rounded toward minus infinity (>> on the signed value)', 'padded_columns_in_block', 'padded_rows_in_block', 'pos & 7 replaced by the scan index', 'row and column transforms exchanged', 'source padded by mirror', 'source padded by zero']),
    (('stripes', 80, 48, 6, 795, 12, 200000, (4,)),
     'C24i0 C24i1 C24i2 C25i0 C25i2 C25p0 C25p2 C27i0 C27i1 C27i2 C28i0 C28i2 C28p0 C29i0 C29i2 C30p0 D24i0 D28i0 E24i0 E25i0 E29i0 Y24i0 Y24i1 Y24i2 Y25i0 Y25i1 Y25i2 Y25p0 Y25p1 Y25p2 Y27i0 Y27i1 Y27i2 Y28i0 Y28i1 Y28i2 Y28p0 Y28p2 Y29i0 Y29i2 Y29p0 Y29p2 Y30i0 Y30i1 Y30i2 Y31i2 Y31p0 Y31p1',
     ['chroma quantised at QPY', 'qpc_ne_qpy']),
    (('stripes', 50, 34, 8, 1119, 12, 20000000, (4,)),
     'C14p1 C16i0 C16i2 C17p0 C17p1 C17p2 C20i0 C20i2 C20p0 C20p1 C20p2 C21i2 C23p1 D13i0 D16i0 D19i0 D22i0 E16i0 E22i0 Y16i0 Y16i1 Y17p0 Y17p1 Y17p2 Y20i1 Y20i2 Y20p0 Y20p1 Y20p2 Y21i2 Y23p1 Y23p2',
     []),
    (('noise', 48, 48, 8, 506, 60, 600000, ()),
     'C31i0 C31i1 C31i2 C32i2 C33i0 C33i2 C34i0 C34i1 C34i2 C35i1 C35i2 D27i0 D35i0 Y32i0 Y32i1 Y32i2 Y34i0 Y34i1 Y34i2 Y35i0 Y35i1 Y35i2 Y36i0 Y36i1 Y36i2 Y39i0 Y39i2',
     []),
    (('noise', 50, 34, 8, 994, 120, 60000, ()),
     'C29i1 C29p0 C30i2 C32i0 C36i0 C36i2 C36p2 C37i0 C37i1 C37i2 Y29i1 Y31i0 Y31i1 Y31p2 Y37i1 Y37i2 Y37p0 Y40i0 Y40i2 Y42i0 Y42i2',
     []),
    (('stripes', 48, 48, 8, 629, 2, 20000000, ()),
     'C13p1 C15i0 C15i1 C15i2 C15p0 C15p2 C19p0 C21i0 C24p0 D15i0 E13p0 Y15i0 Y15i1 Y15i2 Y15p0 Y15p2 Y21i0 Y24p0 Y24p2',
     []),
    (('low', 80, 48, 6, 705, 4, 200000, (4,)),
     'C18p0 C18p1 C18p2 C21p1 C22p0 C22p2 E18p0 E21p0 Y18p0 Y18p1 Y18p2 Y22p0 Y22p1 Y22p2',
     []),
    (('stripes', 48, 48, 8, 635, 12, 200000, ()),
     'C23p0 C23p2 C27p0 C27p2 C30p2 E23p0 Y27p0 Y27p2 Y33i0 Y33i2 Y34p2',
     []),
    (('noise', 50, 34, 8, 985, 60, 200000, ()),
     'C26i0 C26i2 C30i0 C30i1 C32p2 D31i0 E32p0 Y26i0 Y26i2 Y37i0 Y40p0',
     []),
    (('noise', 80, 48, 6, 646, 6, 600000, ()),
     'C18i0 C18i1 C18i2 D17i0 D18i0 E18i0 Y18i0 Y18i1 Y18i2',
     []),
    (('shift', 80, 48, 6, 779, 3, 20000000, ()),
     'C12p1 C16p0 C16p1 C19p1 C22p1 E16p0 E20p0 E22p0 Y16p1',
     []),
    (('noise', 50, 34, 8, 995, 120, 200000, ()),
     'C28i1 C32i1 C36i1 D37i0 E28i0 Y37p2 Y40i1',
     []),
    (('noise', 80, 48, 6, 667, 60, 2000000, ()),
     'C20i1 C21i1 D20i0 E20i0 E21i0 Y20i0 Y21i1',
     []),
    (('noise', 50, 34, 8, 996, 120, 600000, (2, 5)),
     'C26p0 C26p2 C31p0 E31i0 Y26p0 Y32p0',
     []),
    (('stripes', 80, 48, 6, 781, 2, 2000, ()),
     'E37p0 Y36p0 Y41i0 Y41i2 Y42p2',
     []),
    (('noise', 80, 48, 6, 671, 120, 2000, ()),
     'D34i0 E32i0 E34i0 Y42i1',
     []),
    (('noise', 80, 48, 6, 676, 120, 600000, ()),
     'D30i0 D33i0 E27i0 Y33i1',
     []),
    (('stripes', 48, 16, 8, 474, 12, 60000, (2, 5)),
     'C25i1 C27p1 C29p2 Y30p2',
     []),
    (('noise', 50, 34, 8, 987, 60, 2000000, (4,)),
     'C16i1 E14p0 E19p0 E23i0',
     []),
    (('cells', 50, 34, 8, 1032, 4, 6000, (2, 5)),
     'Y35p0',
     ['hadamard_sum_extreme', 'raw_dc_minus_4080', 'raw_dc_plus_4080']),
    (('stripes', 50, 34, 8, 1113, 12, 20000, (4,)),
     'Y35p2 Y38i2 Y41p0 Y42p0',
     []),
    (('shift', 48, 48, 8, 605, 0, 200000, ()),
     'C15p1 E15p0 Y15p1',
     []),
    (('stripes', 50, 34, 8, 1114, 12, 60000, ()),
     'C29p1 C37p0 Y29p1',
     []),
    (('stripes', 48, 48, 8, 636, 12, 600000, (2, 5)),
     'C24p2 D23i0 Y24p1',
     []),
    (('stripes', 80, 48, 6, 784, 2, 60000, ()),
     'Y30p0 Y33p0 Y39p0',
     []),
    (('noise', 80, 48, 6, 674, 120, 60000, ()),
     'E30i0 E36i0',
     []),
    (('shift', 80, 48, 6, 764, 0, 60000, ()),
     'C28p2 C31p2',
     []),
    (('stripes', 80, 48, 6, 796, 12, 600000, ()),
     'Y27p1 Y32p2',
     []),
    (('noise', 50, 34, 8, 964, 6, 60000, ()),
     'Y26i1 Y26p2',
     []),
    (('noise', 50, 34, 8, 974, 20, 60000, ()),
     'D29i0 E30p0',
     []),
    (('stripes', 48, 48, 8, 622, 2, 6000, ()),
     'C35p2 Y36p2',
     []),
    (('noise', 80, 48, 6, 662, 60, 6000, ()),
     'D40i0 D42i0',
     []),
    (('shift', 80, 48, 6, 773, 3, 20000, ()),
     'C32p1 Y34p0',
     []),
    (('stripes', 80, 48, 6, 785, 2, 200000, ()),
     'C35i0 Y33p2',
     []),
    (('low', 48, 48, 8, 539, 2, 20000000, ()),
     'E17p0',
     []),
    (('stripes', 48, 48, 8, 626, 2, 600000, ()),
     'E15i0',
     []),
    (('noise', 80, 48, 6, 644, 6, 60000, ()),
     'D25i0',
     []),
    (('noise', 80, 48, 6, 656, 20, 600000, ()),
     'D32i0',
     []),
    (('noise', 80, 48, 6, 675, 120, 200000, (4,)),
     'E33i0',
     []),
    (('low', 80, 48, 6, 704, 4, 60000, ()),
     'E27p0',
     []),
    (('cells', 80, 48, 6, 712, 4, 6000, ()),
     'C37p2',
     []),
    (('cells', 80, 48, 6, 713, 4, 20000, ()),
     'E34p0',
     []),
    (('shift', 80, 48, 6, 765, 0, 200000, (4,)),
     'C24p1',
     []),
    (('stripes', 80, 48, 6, 794, 12, 60000, ()),
     'C33p2',
     []),
    (('shift', 50, 34, 8, 1094, 3, 60000, ()),
     'C34p2',
     []),
    (('stripes', 50, 34, 8, 1116, 12, 600000, (2, 5)),
     'C25p1',
     []),
    (('noise', 48, 16, 8, 352, 120, 6000, ()),
     'E37i0',
     []),
    (('cells', 48, 16, 8, 394, 4, 60000, ()),
     'E26p0',
     []),
    (('stripes', 48, 16, 8, 465, 2, 200000, (4,)),
     'E24p0',
     []),
    (('stripes', 48, 16, 8, 471, 12, 2000, (4,)),
     'C36p0',
     []),
    (('shift', 48, 48, 8, 604, 0, 60000, ()),
     'C28p1',
     []),
    (('shift', 48, 48, 8, 614, 3, 60000, ()),
     'C32p0',
     []),
    (('noise', 18, 18, 8, 819, 20, 20000000, (4,)),
     'D21i0',
     []),
    (('noise', 18, 18, 8, 821, 60, 2000, ()),
     'Y38i0',
     []),
    (('stripes', 18, 18, 8, 951, 12, 2000, (4,)),
     'Y38p2',
     []),
    (('noise', 50, 34, 8, 984, 60, 60000, (2, 5)),
     'C35p0',
     []),
    (('noise', 50, 34, 8, 992, 120, 6000, ()),
     'C33i1',
     []),
    # two clips without claims of their own: the one-macroblock picture and the one-macroblock-wide picture
    (('low', 16, 16, 8, 46, 1, 600000, ()), '', []),
    (('stripes', 16, 48, 8, 301, 2, 2000, ()), '', []),
]

# cells of the selectable set no candidate of the sweep pinned on both sides: name -> (reason, candidates tried)
_SPARSE = ('not pinned on both sides by any candidate of the sweep: at this QP one step of the class is hundreds of coefficient units wide and the clip\'s few blocks of the kind did not land a coefficient on both sides of a boundary', 1120)
NOT_PINNED = {
    'C26i1': _SPARSE,
    'C26p1': _SPARSE,
    'C30p1': _SPARSE,
    'C31p1': _SPARSE,
    'C33p0': _SPARSE,
    'C33p1': _SPARSE,
    'C34p0': _SPARSE,
    'C34p1': _SPARSE,
    'C35p1': _SPARSE,
    'C36p1': _SPARSE,
    'C37p1': _SPARSE,
    'D26i0': _SPARSE,
    'D36i0': _SPARSE,
    'D38i0': _SPARSE,
    'D39i0': _SPARSE,
    'D41i0': _SPARSE,
    'E25p0': _SPARSE,
    'E26i0': _SPARSE,
    'E28p0': _SPARSE,
    'E29p0': _SPARSE,
    'E31p0': _SPARSE,
    'E33p0': _SPARSE,
    'E35i0': _SPARSE,
    'E35p0': _SPARSE,
    'E36p0': _SPARSE,
    'Y26p1': _SPARSE,
    'Y28p1': _SPARSE,
    'Y30p1': _SPARSE,
    'Y32p1': _SPARSE,
    'Y33p1': _SPARSE,
    'Y34p1': _SPARSE,
    'Y35p1': _SPARSE,
    'Y36p1': _SPARSE,
    'Y37p1': _SPARSE,
    'Y38i1': _SPARSE,
    'Y38p0': _SPARSE,
    'Y38p1': _SPARSE,
    'Y39i1': _SPARSE,
    'Y39p1': _SPARSE,
    'Y39p2': _SPARSE,
    'Y40p1': _SPARSE,
    'Y40p2': _SPARSE,
    'Y41i1': _SPARSE,
    'Y41p1': _SPARSE,
    'Y41p2': _SPARSE,
    'Y42p1': _SPARSE,
}


@functools.lru_cache(maxsize=None)
def directed_clips():
    return tuple(spec_clip(spec, cells.split(), rest) for spec, cells, rest in DIRECTED)


def not_pinned_ok():
    """NOT_PINNED may not hold a whole residue qp % 6 nor a whole qp // 6 in 2..7, for either rounding row, for any kind
    -> the list of violations"""
    bad = []
    sel, npin = selectable(), {cell_of(n) for n in NOT_PINNED}
    for kind, intra in sorted({(c[0], c[2]) for c in sel}):
        mine = [c for c in sel if (c[0], c[2]) == (kind, intra)]
        for what, f, vals in (('qp % 6', lambda q: q % 6, range(6)), ('qp // 6', lambda q: q // 6, range(2, 8))):
            for v in vals:
                grp = [c for c in mine if f(c[1]) == v]
                if grp and all(c in npin for c in grp):
                    bad.append(f'{fwdref.KINDS[kind]} {"intra" if intra else "inter"}: every cell with {what} == {v} is in NOT_PINNED')
    return bad


# ---------------------------------------------------------------- the sweep
def candidates():
    brs = [2000, 6000, 20000, 60000, 200000, 600000, 2000000, 6000000, 20000000, 60000000]
    out = []
    for (w, h) in GEOMETRIES:
        for kind, amps in (('noise', (6, 20, 60, 120)), ('low', (1, 2, 4)), ('cells', (4, 8, 16)), ('checker', (1, 4)), ('shift', (0, 3)), ('stripes', (2, 12))):
            for amp, br in itertools.product(amps, brs):
                seed = len(out) + 1
                n = 8 if w * h <= 48 * 48 else 6
                idr = () if seed % 3 else ((4,) if seed % 2 else (2, 5))
                out.append((kind, w, h, n, seed, amp, br, idr))
    return out


def _sweep_one(spec):
    import os
    from _oracle import Oracle
    oracle = Oracle(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle', 'build', 'libh264_oracle.so'))
    clip = spec_clip(spec)
    _, fr = encaudit.run_clip(oracle, clip)
    frames = chain(clip, [nal for nal, _, _ in fr])
    bad = [str(mm) for _, mm, _ in frames if mm]
    both, pins, cl = count_frames(frames)
    caught = [m.name for m in fwdref.MUTATIONS if catches(frames, m)]
    qps = sorted({int(q) for f, _, _ in frames for q in f.qe[f.typ != PSKIP]})
    return spec, sorted(cell_name(c) for c in both), sorted(k for k in cl if cl[k]), caught, bad, qps


def sweep(procs=8, out=None):
    import multiprocessing
    import pprint
    cands = candidates()
    with multiprocessing.Pool(procs) as pool:
        results = pool.map(_sweep_one, cands, chunksize=4)
    for spec, _, _, _, bad, _ in results:
        assert not bad, (spec, bad[0])
    sel = {cell_name(c) for c in selectable()}
    need = set(sel) | set(CLASSES) | {m.name for m in fwdref.MUTATIONS}
    chosen, batches = [], set()
    while True:
        best, gain = None, 0
        for r in results:
            spec = r[0]
            got = (set(r[1]) | set(r[2]) | set(r[3])) & need
            g = len(got) + (0.5 if (spec[1], spec[2], spec[6], spec[3], spec[7]) in batches else 0)   # a clip that fits a batch already in the set
            if got and g > gain:
                best, gain = r, g
        if best is None:
            break
        spec = best[0]
        cells = sorted(set(best[1]) & need)
        rest = sorted((set(best[2]) | set(best[3])) & need)
        chosen.append((spec, cells, rest))
        need -= set(cells) | set(rest)
        batches.add((spec[1], spec[2], spec[6], spec[3], spec[7]))
    text = 'DIRECTED = [\n' + ''.join(f'    ({spec!r},\n     {" ".join(cells)!r},\n     {rest!r}),\n' for spec, cells, rest in chosen) + ']\n'
    text += f'# not pinned / not reached after {len(cands)} candidates:\n' + pprint.pformat(sorted(need), width=150) + '\n'
    if out:
        open(out, 'w').write(text)
    return chosen, need, len(cands)


if __name__ == '__main__':
    import sys
    if sys.argv[1:2] == ['sweep']:
        chosen, need, n = sweep(out=sys.argv[2] if len(sys.argv) > 2 else None)
        print(f'{n} candidates, {len(chosen)} clips chosen, left: {sorted(need)}')
