"""An independent reference of the H.264 deblocking filter (ITU-T H.264 clause 8.7) for frame pictures of the
Baseline profile -- TEST INFRASTRUCTURE, written from the standard's clauses and tables, not from the oracle's
filter_line / compute_bs / deblock_frame nor from the product's filt_reg / bs_of / deblock_row.

It is also built differently from both, so that a slip of transcription cannot carry over:
  * bS (8.7.2.1) is derived for the whole picture at once, on the grid of 4x4 luma blocks: one array of block
    pairs for all vertical edges and one for all horizontal edges;
  * the samples (8.7.2.3, 8.7.2.4) are filtered one edge of one macroblock at a time, all its lines together as
    arrays, by computing every candidate value and choosing with masks of the standard's conditions;
  * the tables are typed as Table 8-16 / 8-17 print them: alpha' and beta' by indexA / indexB, t'C0 as one row
    per bS.

deblock(planes, records) -> Result: the filtered planes, a Counter of branch events keyed (plane, direction,
class) and explain(plane, x, y), which names the edge lines that cover a sample and their classes. Input: the
picture before the filter at *coded* size and the oracle decoder's records (oracle/h264o_api.h
h264o_dec_records), i.e. everything clause 8.7 reads.
"""
from collections import Counter

import numpy as np

# Table 8-16: alpha' and beta' as a function of indexA / indexB (0..51)
ALPHA = [0] * 16 + [4, 4, 5, 6, 7, 8, 9, 10, 12, 13,
                    15, 17, 20, 22, 25, 28, 32, 36, 40, 45,
                    50, 56, 63, 71, 80, 90, 101, 113, 127, 144,
                    162, 182, 203, 226, 255, 255]
BETA = [0] * 16 + [2, 2, 2, 3, 3, 3, 3, 4, 4, 4,
                   6, 6, 7, 7, 8, 8, 9, 9, 10, 10,
                   11, 11, 12, 12, 13, 13, 14, 14, 15, 15,
                   16, 16, 17, 17, 18, 18]
# Table 8-17: t'C0 as a function of indexA, one row per bS = 1, 2, 3
TC0 = {
    1: [0] * 23 + [1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                   2, 2, 2, 2, 3, 3, 3, 4, 4, 4,
                   5, 6, 6, 7, 8, 9, 10, 11, 13],
    2: [0] * 21 + [1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                   2, 2, 2, 2, 3, 3, 3, 4, 4, 5,
                   5, 6, 7, 8, 8, 10, 11, 12, 13, 15, 17],
    3: [0] * 17 + [1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                   2, 2, 2, 2, 3, 3, 3, 4, 4, 4,
                   5, 6, 6, 7, 8, 9, 10, 11, 13, 14,
                   16, 18, 20, 23, 25],
}
# Table 8-15: QPC as a function of qPI (ChromaArrayType 1)
QPC = list(range(30)) + [29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39]
assert len(ALPHA) == len(BETA) == len(QPC) == 52 and all(len(r) == 52 for r in TC0.values())

INTRA_TYPES = (0, 1, 7)   # I_NxN, I_16x16, I_PCM in the records' mb type code
PCM = 7
REC_INTS = 60

# ---- branch classes. Every one is counted per filtered-edge line, per plane ('luma' / 'chroma') and direction
# ('v': vertical edges, 'h': horizontal edges).
CLASSES_BOTH = [
    # edge class x bS (8.7.2.1)
    'mbedge_bs0', 'mbedge_bs1', 'mbedge_bs2', 'mbedge_bs4', 'inner_bs0', 'inner_bs1', 'inner_bs2', 'inner_bs3',
    # bS 1 by the horizontal / the vertical vector component alone; a difference of exactly 3 (bS 0) and exactly 4 (bS 1)
    'bs1_by_mvx', 'bs1_by_mvy', 'mvdiff_eq3_bs0', 'mvdiff_eq4_bs1',
    # filterSamplesFlag (8-468) of lines with bS != 0
    'fsf_true', 'fsf_false_alpha_only', 'fsf_false_betap_only', 'fsf_false_betaq_only',
    # indexA / indexB (8-460, 8-461) clipped by the slice offsets; alpha switched on / off by FilterOffsetA
    'indexA_clip0', 'indexA_clip51', 'indexB_clip0', 'indexB_clip51', 'alpha_on_by_offset', 'alpha_off_by_offset',
    # QPs across a macroblock edge (8.7.2.2)
    'qp_differ', 'pcm_neighbour',
    # slices: an idc 1 macroblock's samples modified from the neighbouring idc 0 / 2 macroblock's side
    'idc1_modified_by_neighbour',
    # geometry
    'picture_edge', 'last_mb_row', 'last_mb_col', 'one_mb_wide', 'one_mb_high',
]
CLASSES_LUMA = [
    # bS < 4 (8.7.2.3)
    'lt4_ap0_aq0', 'lt4_ap1_aq0', 'lt4_ap0_aq1', 'lt4_ap1_aq1',
    'lt4_delta_clip_pos', 'lt4_delta_clip_neg', 'lt4_delta_noclip',
    'lt4_p1_clip_pos', 'lt4_p1_clip_neg', 'lt4_q1_clip_pos', 'lt4_q1_clip_neg',
    'lt4_clip1_at0', 'lt4_clip1_at255',
    # bS 4 (8.7.2.4)
    'bs4_p_strong', 'bs4_p_weak', 'bs4_q_strong', 'bs4_q_weak', 'bs4_small_false_ap_true', 'bs4_small_false_aq_true',
    # |p0 - q0| on either side of the (alpha >> 2) + 2 threshold of 8-483, with ap or aq < beta (the threshold decides)
    'bs4_small_last_true', 'bs4_small_first_false',
]
CLASSES_CHROMA = ['c_lt4_clip', 'c_lt4_noclip', 'c_bs4', 'cqp_offset_nonzero', 'cqp_offset_clipped']
# per direction only: the left edge is a vertical edge, the top edge a horizontal one (8.7, filterLeftMbEdgeFlag /
# filterTopMbEdgeFlag)
CLASSES_V = ['idc2_left_unfiltered']
CLASSES_H = ['idc2_top_unfiltered']


def required_classes():
    """every (plane, direction, class) the suite's streams must reach (tests/test_dbk_reference.py)"""
    req = set()
    for d in 'vh':
        for pl in ('luma', 'chroma'):
            req |= {(pl, d, c) for c in CLASSES_BOTH}
            req |= {(pl, d, c) for c in (CLASSES_V if d == 'v' else CLASSES_H)}
        req |= {('luma', d, c) for c in CLASSES_LUMA}
        req |= {('chroma', d, c) for c in CLASSES_CHROMA}
    return req


def _clip3(lo, hi, v):
    return np.minimum(np.maximum(v, lo), hi)


class Result:
    def __init__(self, planes, counts, calls, cover):
        self.planes, self.counts, self._calls, self._cover = planes, counts, calls, cover

    def i420(self, w=None, h=None):
        """tight I420 bytes of the window (0, 0)..(w, h) (default: the coded picture)"""
        Y, U, V = self.planes
        h = Y.shape[0] if h is None else h
        w = Y.shape[1] if w is None else w
        return np.concatenate([Y[:h, :w].ravel(), U[:h // 2, :w // 2].ravel(), V[:h // 2, :w // 2].ravel()])

    def explain(self, plane, x, y):
        """the edge lines whose p2..q2 (chroma: p1..q1) cover sample (x, y) of plane 0 / 1 / 2, in filtering order"""
        out = []
        for k in self._cover[plane][y][x]:
            c = self._calls[k]
            i = (y - c['y0']) if c['dir'] == 'v' else (x - c['x0'])
            names = [n for n, m in c['masks'].items() if m[i]]
            out.append(f"MB ({c['mbx']},{c['mby']}) {'vertical' if c['dir'] == 'v' else 'horizontal'} edge {c['edge']} "
                       f"line {i}: bS {int(c['bs'][i])}, qPp {c['qpp']} qPq {c['qpq']} indexA {c['ia']} indexB {c['ib']} "
                       f"alpha {c['alpha']} beta {c['beta']}, classes {names}")
        return out or ['no filtered edge line covers this sample (8.7: it must equal the unfiltered picture)']


def _bs_grid(rec, mbw, mbh):
    """8.7.2.1 on the grid of 4x4 luma blocks -> for dir 'v' / 'h': bS [4 mbh, 4 mbw] of the edge on the left / top
    side of every block (mixedModeEdgeFlag 0, frame macroblocks, P and I slices), and the reasons of the bS 0 / 1
    lines as boolean grids"""
    g = lambda a: a.reshape(mbh, mbw, 4, 4).transpose(0, 2, 1, 3).reshape(4 * mbh, 4 * mbw)
    typ = rec[:, 0]
    intra = g(np.repeat(np.isin(typ, INTRA_TYPES), 16))
    coef = g(rec[:, 2:18] != 0)
    # refIdx of the 8x8 quadrant of each block; one reference picture list of one picture: equal indices are the
    # same reference picture
    quad = np.array([(r >> 3) * 2 + ((r & 3) >> 1) for r in range(16)])
    ref = g(rec[:, 18:22][:, quad])
    mvx, mvy = g(rec[:, 22:54:2]), g(rec[:, 23:54:2])
    out = {}
    for d, ax in (('v', 1), ('h', 0)):
        prev = lambda a: np.roll(a, 1, axis=ax)   # the block on the p side (wraps at the picture edge: never used there)
        n = 4 * (mbw if ax == 1 else mbh)
        on_mb_edge = (np.arange(n) % 4 == 0)
        on_mb_edge = np.broadcast_to(on_mb_edge[None, :] if ax == 1 else on_mb_edge[:, None], intra.shape)
        any_intra = intra | prev(intra)
        any_coef = coef | prev(coef)
        dx, dy = np.abs(mvx - prev(mvx)), np.abs(mvy - prev(mvy))
        other_ref = ref != prev(ref)
        bs = np.zeros(intra.shape, np.int32)
        bs[other_ref | (dx >= 4) | (dy >= 4)] = 1
        bs[any_coef] = 2
        bs[any_intra & ~on_mb_edge] = 3
        bs[any_intra & on_mb_edge] = 4
        plain = ~any_intra & ~any_coef & ~other_ref      # the vectors alone decide between bS 0 and 1
        out[d] = dict(bs=bs, by_mvx=plain & (dx >= 4) & (dy < 4), by_mvy=plain & (dy >= 4) & (dx < 4),
                      eq3=plain & (np.maximum(dx, dy) == 3), eq4=plain & (np.maximum(dx, dy) == 4))
    return out


def _filter_lines(p, q, bs, alpha, beta, tc0, chroma, ev):
    """8.7.2.2-8.7.2.4 on the lines of one edge: p[k], q[k] = arrays of the samples p_k, q_k of every line (k < 4
    luma, k < 2 chroma), bs / tc0 per line. Returns the new (p, q); adds this edge's event masks to ev."""
    p0, p1, q0, q1 = p[0], p[1], q[0], q[1]
    c_a, c_p, c_q = np.abs(p0 - q0) < alpha, np.abs(p1 - p0) < beta, np.abs(q1 - q0) < beta
    live = bs > 0
    fsf = live & c_a & c_p & c_q                                          # filterSamplesFlag (8-468)
    ev['fsf_true'] = fsf
    ev['fsf_false_alpha_only'] = live & ~c_a & c_p & c_q
    ev['fsf_false_betap_only'] = live & c_a & ~c_p & c_q
    ev['fsf_false_betaq_only'] = live & c_a & c_p & ~c_q
    weak, strong = fsf & (bs < 4), fsf & (bs == 4)
    np_, nq = [a.copy() for a in p], [a.copy() for a in q]
    raw = (((q0 - p0) << 2) + (p1 - q1) + 4) >> 3                        # 8-475 before Clip3
    if chroma:
        tc = tc0 + 1                                                       # 8-474
        delta = _clip3(-tc, tc, raw)
        ev['c_lt4_clip'], ev['c_lt4_noclip'], ev['c_bs4'] = weak & (delta != raw), weak & (delta == raw), strong
        np_[0] = np.where(weak, np.clip(p0 + delta, 0, 255), np.where(strong, (2 * p1 + p0 + q1 + 2) >> 2, p0))   # 8-476, 8-485
        nq[0] = np.where(weak, np.clip(q0 - delta, 0, 255), np.where(strong, (2 * q1 + q0 + p1 + 2) >> 2, q0))   # 8-477, 8-492
        return np_, nq
    p2, p3, q2, q3 = p[2], p[3], q[2], q[3]
    ap, aq = np.abs(p2 - p0) < beta, np.abs(q2 - q0) < beta               # 8-471, 8-472 against beta
    # ---- bS < 4 (8.7.2.3)
    tc = tc0 + ap.astype(np.int32) + aq.astype(np.int32)                  # 8-473
    delta = _clip3(-tc, tc, raw)
    mid = (p0 + q0 + 1) >> 1
    rp, rq = (p2 + mid - (p1 << 1)) >> 1, (q2 + mid - (q1 << 1)) >> 1     # 8-479, 8-481 before Clip3
    for a in (0, 1):
        for b in (0, 1):
            ev[f'lt4_ap{a}_aq{b}'] = weak & (ap == bool(a)) & (aq == bool(b))
    ev['lt4_delta_clip_pos'], ev['lt4_delta_clip_neg'], ev['lt4_delta_noclip'] = weak & (raw > tc), weak & (raw < -tc), weak & (np.abs(raw) <= tc)
    ev['lt4_p1_clip_pos'], ev['lt4_p1_clip_neg'] = weak & ap & (rp > tc0), weak & ap & (rp < -tc0)
    ev['lt4_q1_clip_pos'], ev['lt4_q1_clip_neg'] = weak & aq & (rq > tc0), weak & aq & (rq < -tc0)
    ev['lt4_clip1_at0'] = weak & ((p0 + delta < 0) | (q0 - delta < 0))
    ev['lt4_clip1_at255'] = weak & ((p0 + delta > 255) | (q0 - delta > 255))
    w_p0, w_q0 = np.clip(p0 + delta, 0, 255), np.clip(q0 - delta, 0, 255)
    w_p1, w_q1 = p1 + _clip3(-tc0, tc0, rp), q1 + _clip3(-tc0, tc0, rq)
    # ---- bS 4 (8.7.2.4)
    small = np.abs(p0 - q0) < ((alpha >> 2) + 2)                          # 8-483's second condition
    sp, sq = strong & ap & small, strong & aq & small
    ev['bs4_p_strong'], ev['bs4_p_weak'], ev['bs4_q_strong'], ev['bs4_q_weak'] = sp, strong & ~sp, sq, strong & ~sq
    ev['bs4_small_false_ap_true'], ev['bs4_small_false_aq_true'] = strong & ap & ~small, strong & aq & ~small
    ev['bs4_small_last_true'] = strong & (ap | aq) & (np.abs(p0 - q0) == (alpha >> 2) + 1)
    ev['bs4_small_first_false'] = strong & (ap | aq) & (np.abs(p0 - q0) == (alpha >> 2) + 2)
    np_[0] = np.where(weak, w_p0, np.where(sp, (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3,
                                           np.where(strong, (2 * p1 + p0 + q1 + 2) >> 2, p0)))
    np_[1] = np.where(weak & ap, w_p1, np.where(sp, (p2 + p1 + p0 + q0 + 2) >> 2, p1))
    np_[2] = np.where(sp, (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3, p2)
    nq[0] = np.where(weak, w_q0, np.where(sq, (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3,
                                          np.where(strong, (2 * q1 + q0 + p1 + 2) >> 2, q0)))
    nq[1] = np.where(weak & aq, w_q1, np.where(sq, (p0 + q0 + q1 + q2 + 2) >> 2, q1))
    nq[2] = np.where(sq, (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3, q2)
    return np_, nq


def deblock(planes, records, explain=False):
    """planes: (Y, U, V) uint8 at coded size, before the filter; records: int32 [macroblocks, REC_INTS]; explain: keep
    what Result.explain needs (slow: for the one picture an assertion message is about)"""
    P = [np.array(a, dtype=np.int32) for a in planes]
    ch, cw = P[0].shape
    mbw, mbh = cw // 16, ch // 16
    rec = np.asarray(records, np.int32).reshape(mbw * mbh, REC_INTS)
    grid = _bs_grid(rec, mbw, mbh)
    counts, calls = Counter(), []
    cover = [[[[] for _ in range(a.shape[1])] for _ in range(a.shape[0])] for a in P] if explain else None
    cqp = int(rec[0, 58])
    for mby in range(mbh):
        for mbx in range(mbw):
            addr = mby * mbw + mbx
            me = rec[addr]
            idc, first, off_a, off_b = int(me[55]), int(me[54]), int(me[56]), int(me[57])
            for d in 'vh':
                # the macroblock across the left / top edge, and whether that edge is filtered (8.7: filterLeftMbEdgeFlag,
                # filterTopMbEdgeFlag; with slices in raster order a neighbour is in another slice exactly when its address
                # is below this slice's first macroblock)
                nb = (addr - 1 if mbx > 0 else None) if d == 'v' else (addr - mbw if mby > 0 else None)
                outer = nb is not None and idc != 1 and not (idc == 2 and nb < first)
                for pl, nlines in (('luma', 16), ('chroma', 8)):
                    if nb is None:
                        counts[(pl, d, 'picture_edge')] += nlines * (1 if pl == 'luma' else 2)
                    elif idc == 2 and nb < first:
                        counts[(pl, d, 'idc2_left_unfiltered' if d == 'v' else 'idc2_top_unfiltered')] += nlines * (1 if pl == 'luma' else 2)
                if idc == 1:
                    continue
                for e in range(4):
                    if e == 0 and not outer:
                        continue
                    other = rec[nb] if e == 0 else me
                    qy_p = 0 if other[0] == PCM else int(other[1])             # qPp, qPq: QPY, 0 for I_PCM (8.7.2.2)
                    qy_q = 0 if me[0] == PCM else int(me[1])
                    g = grid[d]
                    if d == 'v':
                        sel = (slice(4 * mby, 4 * mby + 4), 4 * mbx + e)
                    else:
                        sel = (4 * mby + e, slice(4 * mbx, 4 * mbx + 4))
                    bs4 = g['bs'][sel]
                    why = {k: g[k][sel] for k in ('by_mvx', 'by_mvy', 'eq3', 'eq4')}
                    for pl in ('luma', 'chroma'):
                        if pl == 'chroma' and e & 1:
                            continue   # chroma 4x4 block edges lie on luma edges 0 and 2 (4:2:0)
                        chroma = pl == 'chroma'
                        if chroma:
                            qp, qq = QPC[min(51, max(0, qy_p + cqp))], QPC[min(51, max(0, qy_q + cqp))]
                        else:
                            qp, qq = qy_p, qy_q
                        qpav = (qp + qq + 1) >> 1                               # 8-459
                        ia, ib = min(51, max(0, qpav + off_a)), min(51, max(0, qpav + off_b))   # 8-460, 8-461
                        alpha, beta = ALPHA[ia], BETA[ib]
                        rep = 2 if chroma else 4
                        bs = np.repeat(bs4, rep)
                        if chroma:
                            bs = np.concatenate([bs, bs])                      # Cb lines then Cr lines
                        tc0 = np.array([0 if b in (0, 4) else TC0[int(b)][ia] for b in bs], np.int32)
                        taps, step = (2, 8) if chroma else (4, 16)
                        pos = (e // 2) * 4 if chroma else 4 * e               # the edge's offset inside the macroblock
                        x0, y0 = mbx * step, mby * step
                        views = []
                        for A in (P[1:] if chroma else P[:1]):
                            if d == 'v':
                                blk = A[y0:y0 + step, x0 + pos - taps:x0 + pos + taps]          # [line, tap]
                            else:
                                blk = A[y0 + pos - taps:y0 + pos + taps, x0:x0 + step].T        # [line, tap]
                            views.append(blk)
                        cat = np.concatenate(views, axis=0)
                        p = [cat[:, taps - 1 - k].copy() for k in range(taps)]
                        q = [cat[:, taps + k].copy() for k in range(taps)]
                        ev = {}
                        np_, nq = _filter_lines(p, q, bs, alpha, beta, tc0, chroma, ev)
                        new = np.stack(np_[::-1] + nq, axis=1)
                        for k, A in enumerate(P[1:] if chroma else P[:1]):
                            part = new[k * step:(k + 1) * step]
                            if d == 'v':
                                A[y0:y0 + step, x0 + pos - taps:x0 + pos + taps] = part
                            else:
                                A[y0 + pos - taps:y0 + pos + taps, x0:x0 + step] = part.T
                        # ---- classes of the edge as a whole, on its lines with bS != 0 (fsf: on its filtered lines)
                        live, fsf = bs > 0, ev['fsf_true']
                        kind = 'mbedge' if e == 0 else 'inner'
                        for b in (0, 1, 2, 3, 4):
                            if b == (3 if kind == 'mbedge' else 4):
                                continue   # 8.7.2.1: bS 4 on macroblock edges only, bS 3 on internal edges only
                            ev[f'{kind}_bs{b}'] = bs == b
                        wl = {k: np.repeat(v, rep) for k, v in why.items()}
                        if chroma:
                            wl = {k: np.concatenate([v, v]) for k, v in wl.items()}
                        ev['bs1_by_mvx'], ev['bs1_by_mvy'] = (bs == 1) & wl['by_mvx'], (bs == 1) & wl['by_mvy']
                        ev['mvdiff_eq3_bs0'], ev['mvdiff_eq4_bs1'] = (bs == 0) & wl['eq3'], (bs == 1) & wl['eq4']
                        ev['indexA_clip0'], ev['indexA_clip51'] = live & (qpav + off_a < 0), live & (qpav + off_a > 51)
                        ev['indexB_clip0'], ev['indexB_clip51'] = live & (qpav + off_b < 0), live & (qpav + off_b > 51)
                        ev['alpha_on_by_offset'] = live & (ALPHA[qpav] == 0 and alpha != 0)
                        ev['alpha_off_by_offset'] = live & (ALPHA[qpav] != 0 and alpha == 0)
                        ev['qp_differ'] = live & (e == 0 and qp != qq)
                        ev['pcm_neighbour'] = live & (e == 0 and (other[0] == PCM) != (me[0] == PCM))
                        changed_p = np.zeros(len(bs), bool)
                        for k in range(taps):
                            changed_p |= np_[k] != p[k]
                        ev['idc1_modified_by_neighbour'] = changed_p & (e == 0 and int(other[55]) == 1)
                        ev['last_mb_row'], ev['last_mb_col'] = fsf & (mby == mbh - 1), fsf & (mbx == mbw - 1)
                        ev['one_mb_wide'], ev['one_mb_high'] = fsf & (mbw == 1), fsf & (mbh == 1)
                        if chroma:
                            ev['cqp_offset_nonzero'] = live & (cqp != 0)
                            ev['cqp_offset_clipped'] = live & (not (0 <= qy_p + cqp <= 51 and 0 <= qy_q + cqp <= 51))
                        for name, m in ev.items():
                            n = int(np.count_nonzero(m))
                            if n:
                                counts[(pl, d, name)] += n
                        if explain:
                            for k in range(2 if chroma else 1):
                                ci = len(calls)
                                calls.append(dict(mbx=mbx, mby=mby, dir=d, edge=e, x0=x0, y0=y0, qpp=qp, qpq=qq, ia=ia, ib=ib,
                                                  alpha=alpha, beta=beta, bs=bs[k * step:(k + 1) * step],
                                                  masks={nm: np.broadcast_to(m, bs.shape)[k * step:(k + 1) * step] for nm, m in ev.items()}))
                                cv = cover[1 + k if chroma else 0]
                                reach = 1 if chroma else 3
                                for i in range(step):
                                    for t in range(-reach, reach):
                                        if d == 'v':
                                            cv[y0 + i][x0 + pos + t].append(ci)
                                        else:
                                            cv[y0 + pos + t][x0 + i].append(ci)
    out = tuple(a.astype(np.uint8) for a in P)
    return Result(out, counts, calls, cover)


def first_difference(res, got_planes, w, h):
    """None, or a message naming the first sample (plane, x, y) inside the w x h window at which got_planes differ from
    the reference's planes, its macroblock, and the reference's edge lines and branch classes covering it"""
    for k, (a, b) in enumerate(zip(res.planes, got_planes)):
        hh, ww = (h, w) if k == 0 else (h // 2, w // 2)
        ne = np.argwhere(a[:hh, :ww] != np.asarray(b)[:hh, :ww])
        if len(ne):
            y, x = (int(v) for v in ne[0])
            s = 16 if k == 0 else 8
            return (f"{len(ne)} samples of plane {'YUV'[k]} differ from tests/dbkref.py (clause 8.7 reference); first at "
                    f"({'YUV'[k]}, x {x}, y {y}): got {int(np.asarray(b)[y, x])}, reference {int(a[y, x])}; MB ({x // s},{y // s}); "
                    + ' | '.join(res.explain(k, x, y)))
    return None
