"""An independent reference of H.264 reconstruction -- intra prediction (ITU-T H.264 clause 8.3), inter prediction
(8.4) and the transform decoding process (8.5) with the QP chain of 7.4.5 -- for Baseline frame pictures with one
reference picture. TEST INFRASTRUCTURE, written from the standard's clauses and tables, not from the oracle's
recon_mb / mvp_part / mc_luma / pred4x4 / dequant_block nor from the product's dec_recon.inc / enc_mb_kernel.inc /
enc_planes.inc.

It is also built differently from both, so that a slip of transcription cannot carry over:
  * neighbour availability is not computed per case. The picture under construction carries a "constructed" flag per
    sample and the motion field a "derived" flag per 4x4 block; a neighbour (6.4.11.4, 6.4.11.7, 6.4.12) is available
    when it lies in the picture, in a macroblock at or after the slice's first one, and its flag is set. The
    top-right rules of blocks 3 / 11, of the macroblock to the right and of a not yet decoded sub-macroblock all fall
    out of the flags;
  * intra prediction evaluates the p[x, y] formulas of 8.3.1.2.x / 8.3.3.x / 8.3.4.x literally, sample by sample,
    through one accessor p(x, y) of the neighbouring samples;
  * inter prediction computes the unrounded half-sample intermediates b1, h1 and j1 (8-241..8-246) of the whole
    reference picture once, on the picture extended by the filter's reach, and reads every block through clipped
    indices (8-229, 8-230) -- so a vector may point anywhere. The twelve quarter positions are a table of sample pairs
    as Table 8-12 / Figure 8-4 give them; chroma is formula 8-270;
  * the residual is computed for all blocks of a macroblock together: the two butterfly stages of 8.5.12.2 on arrays,
    LevelScale from the normAdjust matrix v as printed, the zig-zag as (x, y) pairs.

reconstruct(syntax, geometry, ref_planes) -> Result: the picture before the loop filter at coded size, the derived
records in the layout of h264o_dec_records (so dbkref.deblock(res.planes, res.records) runs on it), a Counter of
branch classes and explain(plane, x, y). syntax: the oracle decoder's parse (oracle/h264o_api.h h264o_dec_syntax):
syntax elements only, nothing derived.
"""
from collections import Counter

import numpy as np

from dbkref import QPC   # Table 8-15

SYN_INTS, REC_INTS = 872, 60

# Table 8-13, frame scan: zig-zag index -> (x, y) of the coefficient (Figure 8-8: the scan leaves c00 to the right)
ZIGZAG_XY = [(0, 0), (1, 0), (0, 1), (0, 2), (1, 1), (2, 0), (3, 0), (2, 1),
             (1, 2), (0, 3), (1, 3), (2, 2), (3, 1), (3, 2), (2, 3), (3, 3)]
# 8-315: normAdjust4x4 -- the matrix v, one row per qP % 6; column 0: both indices even, 1: both odd, 2: otherwise
V = [[10, 16, 13],
     [11, 18, 14],
     [13, 20, 16],
     [14, 23, 18],
     [16, 25, 20],
     [18, 29, 23]]
# Table 9-4, ChromaArrayType 1: codeNum -> coded_block_pattern for (Intra_4x4, Inter)
CBP_TABLE = [(47, 0), (31, 16), (15, 1), (0, 2), (23, 4), (27, 8), (29, 32), (30, 3), (7, 5), (11, 10), (13, 12), (14, 15),
             (39, 47), (43, 7), (45, 11), (46, 13), (16, 14), (3, 6), (5, 9), (10, 31), (12, 35), (19, 37), (21, 42), (26, 44),
             (28, 33), (35, 34), (37, 36), (42, 40), (44, 39), (1, 43), (2, 45), (4, 46), (8, 17), (17, 18), (18, 20), (20, 24),
             (24, 19), (6, 21), (9, 26), (22, 28), (25, 23), (32, 27), (33, 29), (34, 30), (36, 22), (40, 25), (38, 38), (41, 41)]
# 6.4.3 (Figure 6-10): luma4x4BlkIdx -> (x, y) of the block's upper-left sample
BLK_XY = [(4 * ((b & 1) + 2 * ((b >> 2) & 1)), 4 * (((b >> 1) & 1) + 2 * (b >> 3))) for b in range(16)]
# Table 8-12 / Figure 8-4: (xFrac, yFrac) -> the sample itself, or the two samples whose rounded mean it is. A sample is
# (array, dx, dy): G integer samples, b / h / j the half samples to the right of / below / diagonal from G[dx, dy]
QUARTER = {
    (0, 0): (('G', 0, 0),),
    (1, 0): (('G', 0, 0), ('b', 0, 0)),     # a
    (2, 0): (('b', 0, 0),),                 # b
    (3, 0): (('b', 0, 0), ('G', 1, 0)),     # c  (H)
    (0, 1): (('G', 0, 0), ('h', 0, 0)),     # d
    (1, 1): (('b', 0, 0), ('h', 0, 0)),     # e
    (2, 1): (('b', 0, 0), ('j', 0, 0)),     # f
    (3, 1): (('b', 0, 0), ('h', 1, 0)),     # g  (m)
    (0, 2): (('h', 0, 0),),                 # h
    (1, 2): (('h', 0, 0), ('j', 0, 0)),     # i
    (2, 2): (('j', 0, 0),),                 # j
    (3, 2): (('j', 0, 0), ('h', 1, 0)),     # k  (m)
    (0, 3): (('h', 0, 0), ('G', 0, 1)),     # n  (M)
    (1, 3): (('h', 0, 0), ('b', 0, 1)),     # p  (s)
    (2, 3): (('j', 0, 0), ('b', 0, 1)),     # q  (s)
    (3, 3): (('h', 1, 0), ('b', 0, 1)),     # r  (m, s)
}
TYPE_NAMES = {0: 'I_NxN', 1: 'I_16x16', 2: 'P_L0_16x16', 3: 'P_Skip', 4: 'P_L0_L0_16x8', 5: 'P_L0_L0_8x16', 6: 'P_8x8', 7: 'I_PCM'}
SIZES = ['16x16', '16x8', '8x16', '8x8', '8x4', '4x8', '4x4']
I4_NAMES = ['V', 'H', 'DC', 'DDL', 'DDR', 'VR', 'HD', 'VL', 'HU']


def required_classes():
    """every class the suite's streams must reach (tests/test_recon_reference.py)"""
    req = set()
    req |= {('luma_frac', s, xf, yf) for s in SIZES for xf in range(4) for yf in range(4)}
    req |= {('chroma_frac', bool(a), bool(b)) for a in (0, 1) for b in (0, 1)}
    req |= {('ref_geom', 'inside')} | {('ref_geom', side, c) for side in 'LRTB' for c in ('cross', 'outside', 'support_only')}
    req |= {('mv', 'gt16'), ('mv', 'gt32')}
    req |= {('mvp', c) for c in ('median3', 'c_from_d', 'c_and_d_unavailable', 'only_a', 'single_A', 'single_B', 'single_C', 'none',
                                 'c_in_undecoded_sub', 'nb_other_slice')}
    req |= {('mvp', f'dir_{hm}_{p}') for hm in ('hit', 'miss') for p in ('16x8_0', '16x8_1', '8x16_0', '8x16_1')}
    req |= {('skip', c) for c in ('zero_A_unavailable', 'zero_B_unavailable', 'zero_mvA', 'zero_mvB', 'predicted')}
    for fam in ('i4', 'i16', 'chroma'):
        req |= {(fam, m) for m in ('V', 'H', 'plane' if fam != 'i4' else 'HU')}
        if fam != 'chroma':
            req |= {(fam, 'DC', t, l) for t in (False, True) for l in (False, True)}
    req |= {('i4', m) for m in ('DDR', 'VR', 'HD')} | {('i4', m, tr) for m in ('DDL', 'VL') for tr in ('tr', 'tr_substituted')}
    req |= {('chroma_dc', pos, t, l) for pos in ('diag', 'right', 'below') for t in (False, True) for l in (False, True)}
    req |= {('tr_substituted', c) for c in ('block_position', 'later_mb', 'picture_edge', 'slice_edge')}
    req |= {('i4pred', c) for c in ('dc_by_unavailable', 'dc_by_inter', 'dc_by_i16_or_pcm', 'prev_flag_1', 'prev_flag_0',
                                    'rem_below', 'rem_at_or_above')}
    req |= {('levelscale', pl, m, c) for pl in ('Y', 'Cb', 'Cr') for m in range(6) for c in range(3)}
    req |= {('qp_div6', pl, c) for pl in ('Y', 'Cb', 'Cr') for c in ('0', '1', 'ge6')}
    req |= {('i16dc', 'lt36'), ('i16dc', 'ge36'), ('chroma_dc_qp', 'lt6'), ('chroma_dc_qp', 'ge6')}
    req |= {('block', 'dc_only'), ('block', 'empty_beside_coded')}
    req |= {('clip1', v, k) for v in ('at0', 'at255') for k in ('inter', 'intra')}
    req |= {('qp', c) for c in ('wrap_below0', 'wrap_above51', 'carry_skip', 'carry_pcm', 'carry_cbp0', 'slice_start',
                                'qpc_clip0', 'qpc_clip51')}
    return req


class Result:
    def __init__(self, planes, records, counts, units, pred=None, skip_mv=None):
        self.planes, self.records, self.counts, self._units = planes, records, counts, units
        self.skip_mv = skip_mv   # macroblock address of every P_L0_16x16 -> the vector a P_Skip would have had there (8.4.1.1)
        self.pred = pred   # the prediction sample of every position, three planes beside `planes` (I_PCM: the sample itself)

    def i420(self, w=None, h=None):
        Y, U, V_ = self.planes
        h = Y.shape[0] if h is None else h
        w = Y.shape[1] if w is None else w
        return np.concatenate([Y[:h, :w].ravel(), U[:h // 2, :w // 2].ravel(), V_[:h // 2, :w // 2].ravel()])

    def explain(self, plane, x, y):
        """the macroblock, its type, the partition or block covering sample (x, y) of plane 0 / 1 / 2 and its classes"""
        s = 1 if plane == 0 else 2
        lx, ly = x * s, y * s
        mbw = self.planes[0].shape[1] // 16
        addr = (ly // 16) * mbw + lx // 16
        rec = self.records[addr]
        out = [f'MB ({lx // 16},{ly // 16}) addr {addr} {TYPE_NAMES[int(rec[0])]} QPY {int(rec[1])}']
        for u in self._units[addr]:
            if u['plane'] in ('all', 'luma' if plane == 0 else 'chroma') and u['x'] <= lx % 16 < u['x'] + u['w'] and u['y'] <= ly % 16 < u['y'] + u['h']:
                out.append(f"{u['what']}; classes {u['classes']}")
        return out


class _Picture:
    """everything reconstruct() carries from macroblock to macroblock"""

    def __init__(self, mbw, mbh):
        self.mbw, self.mbh = mbw, mbh
        W, H = 16 * mbw, 16 * mbh
        self.P = [np.zeros((H, W), np.int32), np.zeros((H // 2, W // 2), np.int32), np.zeros((H // 2, W // 2), np.int32)]
        self.built = [np.zeros(a.shape, bool) for a in self.P]       # sample constructed in this picture
        self.pred = [np.full(a.shape, -1, np.int32) for a in self.P]  # the prediction each sample was built from
        self.mv = np.zeros((4 * mbh, 4 * mbw, 2), np.int32)          # motion field on the 4x4 grid
        self.ref = np.full((4 * mbh, 4 * mbw), -1, np.int32)         # refIdxL0, -1 intra
        self.derived = np.zeros((4 * mbh, 4 * mbw), bool)            # the block's prediction mode / vector is known
        self.i4 = np.full((4 * mbh, 4 * mbw), -1, np.int32)          # Intra4x4PredMode, -1: not an Intra_4x4 block
        self.mbtype = np.full(mbw * mbh, -1, np.int32)
        self.first = np.zeros(mbw * mbh, np.int32)                   # first_mb_in_slice of each macroblock's slice


def _mb_of_block(pic, gx, gy):
    return (gy // 4) * pic.mbw + gx // 4


def _halves(ref):
    """G and the unrounded b1, h1, j1 of one reference plane on the picture extended by 3 samples each way: beyond
    that every tap reads the same clamped sample, so an index clipped into the extension is exact (8-229, 8-230)"""
    H, W = ref.shape
    ys, xs = np.clip(np.arange(-5, H + 6), 0, H - 1), np.clip(np.arange(-5, W + 6), 0, W - 1)
    E = ref.astype(np.int64)[ys][:, xs]                        # E[y + 5, x + 5] = sample (x, y), clipped
    tap = lambda a, ax: (np.roll(a, 2, ax) - 5 * np.roll(a, 1, ax) + 20 * a + 20 * np.roll(a, -1, ax) - 5 * np.roll(a, -2, ax)
                         + np.roll(a, -3, ax))                 # E - 5F + 20G + 20H - 5I + J, at G
    b1, h1 = tap(E, 1), tap(E, 0)
    j1 = tap(b1, 0)                                            # 8-245 over the b1 column (cc, dd, h1.. of Figure 8-4)
    core = (slice(2, H + 8), slice(2, W + 8))                  # coordinates -3 .. size + 2 (np.roll's wrap stays outside)
    return dict(G=E[core], b1=b1[core], h1=h1[core], j1=j1[core], W=W, H=H)


def _fetch(hv, kind, xs, ys):
    """sample array `kind` at picture coordinates xs (columns) x ys (rows)"""
    xi = np.clip(xs, -3, hv['W'] + 2) + 3
    yi = np.clip(ys, -3, hv['H'] + 2) + 3
    if kind == 'G':
        return hv['G'][yi][:, xi]
    if kind == 'b':
        return np.clip((hv['b1'][yi][:, xi] + 16) >> 5, 0, 255)      # 8-247
    if kind == 'h':
        return np.clip((hv['h1'][yi][:, xi] + 16) >> 5, 0, 255)      # 8-248
    return np.clip((hv['j1'][yi][:, xi] + 512) >> 10, 0, 255)        # 8-249


def _luma_pred(hv, x0, y0, w, h, mvx, mvy):
    xs, ys = x0 + (mvx >> 2) + np.arange(w), y0 + (mvy >> 2) + np.arange(h)      # 8-225, 8-226
    parts = [_fetch(hv, k, xs + dx, ys + dy) for k, dx, dy in QUARTER[(mvx & 3, mvy & 3)]]
    return parts[0] if len(parts) == 1 else (parts[0] + parts[1] + 1) >> 1     # 8-250 .. 8-261


def _chroma_pred(ref, x0, y0, w, h, mvx, mvy):
    H, W = ref.shape
    xf, yf = mvx & 7, mvy & 7                                                    # 8-231, 8-232: eighth samples
    xs, ys = x0 + (mvx >> 3) + np.arange(w), y0 + (mvy >> 3) + np.arange(h)
    at = lambda yy, xx: ref.astype(np.int64)[np.clip(yy, 0, H - 1)][:, np.clip(xx, 0, W - 1)]
    A, B, C, D = at(ys, xs), at(ys, xs + 1), at(ys + 1, xs), at(ys + 1, xs + 1)
    return ((8 - xf) * (8 - yf) * A + xf * (8 - yf) * B + (8 - xf) * yf * C + xf * yf * D + 32) >> 6   # 8-270


def _geometry_classes(x0, y0, w, h, mvx, mvy, W, H):
    out = []
    xa, ya = x0 + (mvx >> 2), y0 + (mvy >> 2)
    sx = (2, 3) if mvx & 3 else (0, 0)      # the 6-tap support beyond the block, left / right
    sy = (2, 3) if mvy & 3 else (0, 0)
    inside = True
    for side, lo, hi, s_lo, s_hi, size in (('L', xa, xa + w - 1, sx[0], 0, W), ('R', xa, xa + w - 1, 0, sx[1], W),
                                           ('T', ya, ya + h - 1, sy[0], 0, H), ('B', ya, ya + h - 1, 0, sy[1], H)):
        if side in 'LT':
            if hi < 0:
                out.append(('ref_geom', side, 'outside'))
            elif lo < 0:
                out.append(('ref_geom', side, 'cross'))
            elif lo - s_lo < 0:
                out.append(('ref_geom', side, 'support_only'))
            else:
                continue
        else:
            if lo > size - 1:
                out.append(('ref_geom', side, 'outside'))
            elif hi > size - 1:
                out.append(('ref_geom', side, 'cross'))
            elif hi + s_hi > size - 1:
                out.append(('ref_geom', side, 'support_only'))
            else:
                continue
        inside = False
    if inside:
        out.append(('ref_geom', 'inside'))
    far = max(abs(mvx >> 2), abs(mvy >> 2))
    if far > 16:
        out.append(('mv', 'gt16'))
    if far > 32:
        out.append(('mv', 'gt32'))
    return out


# ---------------------------------------------------------------------------------------------------------------
# 8.4.1: motion vector prediction


def _nb_motion(pic, addr, gx, gy):
    """the neighbouring partition covering 4x4 block (gx, gy) of the picture grid, for macroblock addr -> (available,
    refIdx, mv, why unavailable). Available: inside the picture, in a macroblock of this slice that precedes or is
    this one, and already derived (6.4.11.7: a partition later in decoding order is not available)"""
    if not (0 <= gx < 4 * pic.mbw and gy >= 0):
        return False, -1, (0, 0), 'picture'
    nb = _mb_of_block(pic, gx, gy)
    if nb > addr:
        return False, -1, (0, 0), 'later'
    if nb < pic.first[addr]:
        return False, -1, (0, 0), 'slice'
    if not pic.derived[gy, gx]:
        return False, -1, (0, 0), 'later'
    return True, int(pic.ref[gy, gx]), (int(pic.mv[gy, gx, 0]), int(pic.mv[gy, gx, 1])), None


def _neighbours(pic, addr, x, y, w):
    """A, B, C (D substituted when C is unavailable) of the partition at luma (x, y) of width w in macroblock addr"""
    gx, gy = 4 * (addr % pic.mbw) + x // 4, 4 * (addr // pic.mbw) + y // 4
    A = _nb_motion(pic, addr, gx - 1, gy)
    B = _nb_motion(pic, addr, gx, gy - 1)
    C = _nb_motion(pic, addr, gx + w // 4, gy - 1)
    D = _nb_motion(pic, addr, gx - 1, gy - 1)
    cls = []
    if any(n[3] == 'slice' for n in (A, B, C, D)):
        cls.append(('mvp', 'nb_other_slice'))
    if not C[0]:
        if C[3] == 'later' and x + w < 16 and y > 0:      # C lies inside this macroblock, in a partition still to come
            cls.append(('mvp', 'c_in_undecoded_sub'))
        cls.append(('mvp', 'c_from_d' if D[0] else 'c_and_d_unavailable'))
        C = D
    return A, B, C, cls


def _median_pred(A, B, C, cls):
    """8.4.1.3.1 with the reference index of the current partition 0"""
    if not B[0] and not C[0] and A[0]:
        cls.append(('mvp', 'only_a'))
        B = C = A
    same = [n[0] and n[1] == 0 for n in (A, B, C)]
    if sum(same) == 1:
        k = same.index(True)
        if ('mvp', 'only_a') not in cls:
            cls.append(('mvp', 'single_' + 'ABC'[k]))
        return (A, B, C)[k][2]
    if sum(same) == 3 and ('mvp', 'only_a') not in cls:
        cls.append(('mvp', 'median3'))
    if sum(same) == 0:
        cls.append(('mvp', 'none'))
    med = lambda a, b, c: a + b + c - min(a, b, c) - max(a, b, c)
    return tuple(med(A[2][k], B[2][k], C[2][k]) for k in (0, 1))


def _mvp(pic, addr, x, y, w, h, shape, idx):
    """mvpL0 of a partition; shape '16x8' / '8x16' select the directional rule of 8.4.1.3"""
    A, B, C, cls = _neighbours(pic, addr, x, y, w)
    pick = None
    if shape == '16x8':
        pick = B if idx == 0 else A
    elif shape == '8x16':
        pick = A if idx == 0 else C
    if pick is not None:
        if pick[0] and pick[1] == 0:
            cls.append(('mvp', f'dir_hit_{shape}_{idx}'))
            return pick[2], cls
        cls.append(('mvp', f'dir_miss_{shape}_{idx}'))
    return _median_pred(A, B, C, cls), cls


def _skip_mv(pic, addr):
    """8.4.1.1"""
    A, B, C, cls = _neighbours(pic, addr, 0, 0, 16)
    if not A[0]:
        return (0, 0), [('skip', 'zero_A_unavailable')]
    if not B[0]:
        return (0, 0), [('skip', 'zero_B_unavailable')]
    if A[1] == 0 and A[2] == (0, 0):
        return (0, 0), [('skip', 'zero_mvA')]
    if B[1] == 0 and B[2] == (0, 0):
        return (0, 0), [('skip', 'zero_mvB')]
    return _median_pred(A, B, C, cls), cls + [('skip', 'predicted')]


# ---------------------------------------------------------------------------------------------------------------
# 8.3: intra prediction


class _Nb:
    """the neighbouring samples p[x, y] (x = -1 or y = -1) of a block at (X, Y) of a plane, for macroblock addr"""

    def __init__(self, pic, plane, addr, X, Y):
        self.pic, self.pl, self.addr, self.X, self.Y = pic, plane, addr, X, Y
        self.s = 16 if plane == 0 else 8

    def why(self, x, y):
        """None when p[x, y] is available, else the cause"""
        pic, ax, ay = self.pic, self.X + x, self.Y + y
        H, W = pic.P[self.pl].shape
        if not (0 <= ax < W and 0 <= ay < H):
            return 'picture_edge'
        nb = (ay // self.s) * pic.mbw + ax // self.s
        if nb > self.addr:
            return 'later_mb'
        if nb < pic.first[self.addr]:
            return 'slice_edge'
        if not pic.built[self.pl][ay, ax]:
            return 'block_position'
        return None

    def has(self, x, y):
        return self.why(x, y) is None

    def p(self, x, y):
        assert self.has(x, y), (x, y)
        return int(self.pic.P[self.pl][self.Y + y, self.X + x])


def _pred4x4(nb, mode, cls):
    T, L, D, R = nb.has(0, -1), nb.has(-1, 0), nb.has(-1, -1), nb.has(4, -1)
    if T and not R:   # 8.3.1.2: p[x, -1], x = 4..7, take the value of p[3, -1]
        sub = nb.p(3, -1)
        p = lambda x, y: sub if (y == -1 and x > 3) else nb.p(x, y)
    else:
        p = nb.p
    name = I4_NAMES[mode]
    if mode in (3, 7):
        cls.append(('i4', name, 'tr' if R else 'tr_substituted'))
        if not R:
            cls.append(('tr_substituted', nb.why(4, -1)))
    elif mode == 2:
        cls.append(('i4', 'DC', T, L))
    else:
        cls.append(('i4', name))
    out = np.zeros((4, 4), np.int32)
    for y in range(4):
        for x in range(4):
            if mode == 0:
                v = p(x, -1)
            elif mode == 1:
                v = p(-1, y)
            elif mode == 2:
                if T and L:
                    v = (sum(p(k, -1) for k in range(4)) + sum(p(-1, k) for k in range(4)) + 4) >> 3
                elif L:
                    v = (sum(p(-1, k) for k in range(4)) + 2) >> 2
                elif T:
                    v = (sum(p(k, -1) for k in range(4)) + 2) >> 2
                else:
                    v = 128
            elif mode == 3:
                v = (p(6, -1) + 3 * p(7, -1) + 2) >> 2 if x == 3 and y == 3 else (p(x + y, -1) + 2 * p(x + y + 1, -1) + p(x + y + 2, -1) + 2) >> 2
            elif mode == 4:
                if x > y:
                    v = (p(x - y - 2, -1) + 2 * p(x - y - 1, -1) + p(x - y, -1) + 2) >> 2
                elif x < y:
                    v = (p(-1, y - x - 2) + 2 * p(-1, y - x - 1) + p(-1, y - x) + 2) >> 2
                else:
                    v = (p(0, -1) + 2 * p(-1, -1) + p(-1, 0) + 2) >> 2
            elif mode == 5:
                z = 2 * x - y
                if z >= 0 and z % 2 == 0:
                    v = (p(x - (y >> 1) - 1, -1) + p(x - (y >> 1), -1) + 1) >> 1
                elif z >= 0:
                    v = (p(x - (y >> 1) - 2, -1) + 2 * p(x - (y >> 1) - 1, -1) + p(x - (y >> 1), -1) + 2) >> 2
                elif z == -1:
                    v = (p(-1, 0) + 2 * p(-1, -1) + p(0, -1) + 2) >> 2
                else:
                    v = (p(-1, y - 1) + 2 * p(-1, y - 2) + p(-1, y - 3) + 2) >> 2
            elif mode == 6:
                z = 2 * y - x
                if z >= 0 and z % 2 == 0:
                    v = (p(-1, y - (x >> 1) - 1) + p(-1, y - (x >> 1)) + 1) >> 1
                elif z >= 0:
                    v = (p(-1, y - (x >> 1) - 2) + 2 * p(-1, y - (x >> 1) - 1) + p(-1, y - (x >> 1)) + 2) >> 2
                elif z == -1:
                    v = (p(-1, 0) + 2 * p(-1, -1) + p(0, -1) + 2) >> 2
                else:
                    v = (p(x - 1, -1) + 2 * p(x - 2, -1) + p(x - 3, -1) + 2) >> 2
            elif mode == 7:
                if y % 2 == 0:
                    v = (p(x + (y >> 1), -1) + p(x + (y >> 1) + 1, -1) + 1) >> 1
                else:
                    v = (p(x + (y >> 1), -1) + 2 * p(x + (y >> 1) + 1, -1) + p(x + (y >> 1) + 2, -1) + 2) >> 2
            else:
                z = x + 2 * y
                if z > 5:
                    v = p(-1, 3)
                elif z == 5:
                    v = (p(-1, 2) + 3 * p(-1, 3) + 2) >> 2
                elif z % 2 == 0:
                    v = (p(-1, y + (x >> 1)) + p(-1, y + (x >> 1) + 1) + 1) >> 1
                else:
                    v = (p(-1, y + (x >> 1)) + 2 * p(-1, y + (x >> 1) + 1) + p(-1, y + (x >> 1) + 2) + 2) >> 2
            out[y, x] = v
    return out


def _pred_square(nb, n, kind, cls, fam):
    """Intra_16x16 (n 16, 8.3.3) and chroma (n 8, 8.3.4) prediction by kind 'V' / 'H' / 'DC' / 'plane'"""
    T, L = nb.has(0, -1), nb.has(-1, 0)
    p = nb.p
    out = np.zeros((n, n), np.int32)
    if kind == 'V':
        out[:] = np.array([p(x, -1) for x in range(n)])[None, :]
    elif kind == 'H':
        out[:] = np.array([p(-1, y) for y in range(n)])[:, None]
    elif kind == 'plane':
        half = n // 2
        Hh = sum((k + 1) * (p(half + k, -1) - p(half - 2 - k, -1)) for k in range(half))
        Vv = sum((k + 1) * (p(-1, half + k) - p(-1, half - 2 - k)) for k in range(half))
        a = 16 * (p(-1, n - 1) + p(n - 1, -1))
        mul = 5 if n == 16 else 34                                   # 8-141, 8-142 (xCF = yCF = 0 in 4:2:0)
        b, c = (mul * Hh + 32) >> 6, (mul * Vv + 32) >> 6
        for y in range(n):
            for x in range(n):
                out[y, x] = min(255, max(0, (a + b * (x - (half - 1)) + c * (y - (half - 1)) + 16) >> 5))
    elif n == 16:
        cls.append((fam, 'DC', T, L))
        st, sl = sum(p(k, -1) for k in range(16)) if T else 0, sum(p(-1, k) for k in range(16)) if L else 0
        out[:] = (st + sl + 16) >> 5 if T and L else ((sl + 8) >> 4 if L else ((st + 8) >> 4 if T else 128))
    else:
        for yO in (0, 4):      # 8.3.4.1-3: each chroma 4x4 block by its position
            for xO in (0, 4):
                st = sum(p(xO + k, -1) for k in range(4)) if T else 0
                sl = sum(p(-1, yO + k) for k in range(4)) if L else 0
                pos = 'diag' if xO == yO else ('right' if xO else 'below')
                cls.append(('chroma_dc', pos, T, L))
                if pos == 'diag':
                    v = (st + sl + 4) >> 3 if T and L else ((sl + 2) >> 2 if L else ((st + 2) >> 2 if T else 128))
                elif pos == 'right':
                    v = (st + 2) >> 2 if T else ((sl + 2) >> 2 if L else 128)
                else:
                    v = (sl + 2) >> 2 if L else ((st + 2) >> 2 if T else 128)
                out[yO:yO + 4, xO:xO + 4] = v
    if kind != 'DC':
        cls.append((fam, kind))
    return out


# ---------------------------------------------------------------------------------------------------------------
# 8.5: residual


def _level_scale(qp):
    """LevelScale(qP % 6, i, j) for a flat scaling matrix (8-313): 16 * normAdjust4x4, as [y, x]"""
    m = qp % 6
    return np.array([[16 * V[m][0 if (x % 2 == 0 and y % 2 == 0) else (1 if (x % 2 and y % 2) else 2)] for x in range(4)] for y in range(4)], np.int64)


def _pos_class(x, y):
    return 0 if (x % 2 == 0 and y % 2 == 0) else (1 if (x % 2 and y % 2) else 2)


def _unscan(levels):
    """8.5.6: a list of 16 levels in zig-zag order -> c as [y, x]"""
    c = np.zeros((4, 4), np.int64)
    for k, (x, y) in enumerate(ZIGZAG_XY):
        c[y, x] = levels[k]
    return c


def _scale(c, qp, keep_dc):
    """8.5.12.1: d from c ([..., y, x]); keep_dc: c[0, 0] is an already scaled DC and passes unchanged"""
    ls = _level_scale(qp)
    if qp >= 24:
        d = (c * ls) << (qp // 6 - 4)
    else:
        d = (c * ls + (1 << (3 - qp // 6))) >> (4 - qp // 6)
    if keep_dc:
        d[..., 0, 0] = c[..., 0, 0]
    return d


def _transform(d):
    """8.5.12.2: the residual r of d ([..., y, x]): each row, then each column, then (x + 32) >> 6"""
    def stage(a):          # the one-dimensional transform along the last axis
        e0, e1 = a[..., 0] + a[..., 2], a[..., 0] - a[..., 2]
        e2, e3 = (a[..., 1] >> 1) - a[..., 3], a[..., 1] + (a[..., 3] >> 1)
        return np.stack([e0 + e3, e1 + e2, e1 - e2, e0 - e3], axis=-1)
    g = stage(d)                                       # 8-338 .. 8-345 on rows
    hh = np.swapaxes(stage(np.swapaxes(g, -1, -2)), -1, -2)   # 8-346 .. 8-353 on columns
    return (hh + 32) >> 6


def _luma_dc(levels, qp):
    """8.5.10: the Intra_16x16 DC values dcY as [y, x] over the 4x4 blocks"""
    A = np.array([[1, 1, 1, 1], [1, 1, -1, -1], [1, -1, -1, 1], [1, -1, 1, -1]], np.int64)
    f = A @ _unscan(levels) @ A
    ls = 16 * V[qp % 6][0]
    if qp >= 36:
        return (f * ls) << (qp // 6 - 6)
    return (f * ls + (1 << (5 - qp // 6))) >> (6 - qp // 6)


def _chroma_dc(levels, qpc):
    """8.5.11: dcC as [y, x] over the four chroma blocks (chroma4x4BlkIdx in raster order)"""
    A = np.array([[1, 1], [1, -1]], np.int64)
    f = A @ np.array(levels, np.int64).reshape(2, 2) @ A
    return ((f * (16 * V[qpc % 6][0])) << (qpc // 6)) >> 5


# ---------------------------------------------------------------------------------------------------------------


def reconstruct(syntax, geometry, ref_planes=None):
    """syntax: int32 [macroblocks, SYN_INTS] (h264o_dec_syntax); geometry: (macroblocks wide, high); ref_planes: the
    reference picture (Y, U, V) at coded size, None for a picture without P macroblocks"""
    mbw, mbh = geometry
    syn = np.asarray(syntax, np.int64).reshape(mbw * mbh, SYN_INTS)
    pic = _Picture(mbw, mbh)
    pic.first[:] = syn[:, 74]
    W, H = 16 * mbw, 16 * mbh
    counts, units = Counter(), [[] for _ in range(mbw * mbh)]
    rec = np.zeros((mbw * mbh, REC_INTS), np.int32)
    hv = _halves(np.asarray(ref_planes[0])) if ref_planes is not None else None
    qpy = np.zeros(mbw * mbh, np.int32)
    skip_mv = {}
    carried = [None] * (mbw * mbh)   # why the macroblock's QPY is its predecessor's: 'skip' / 'pcm' / 'cbp0', else None

    def note(addr, plane, x, y, w, h, what, cls):
        for c in cls:
            counts[c] += 1
        units[addr].append(dict(plane=plane, x=x, y=y, w=w, h=h, what=what, classes=list(cls)))

    for addr in range(mbw * mbh):
        s = syn[addr]
        mbx, mby = addr % mbw, addr // mbw
        X, Y = 16 * mbx, 16 * mby
        gx, gy = 4 * mbx, 4 * mby
        mbt, is_p, cqp = int(s[0]), int(s[1]) == 0, int(s[75])
        first = int(s[74])
        # ---- mb_type (Tables 7-11, 7-13)
        if mbt == -1:
            typ = 3
        elif is_p and mbt < 5:
            typ = [2, 4, 5, 6, 6][mbt]
        else:
            it = mbt - 5 if is_p else mbt
            typ = 0 if it == 0 else (7 if it == 25 else 1)
        pic.mbtype[addr] = typ
        # ---- coded_block_pattern and the QP chain (7.4.5)
        if typ == 1:
            i16_mode, cbp = (it - 1) % 4, (((it - 1) // 4) % 3) << 4 | (15 if it >= 13 else 0)
        elif typ in (3, 7):
            cbp = 0
        else:
            cbp = CBP_TABLE[int(s[76])][0 if typ == 0 else 1]
            assert cbp == int(s[71]), 'Table 9-4 as typed here != the parsed coded_block_pattern'
        qcls = []
        pred_qp = int(s[73]) if addr == first else int(qpy[addr - 1])
        has_delta = typ == 1 or (typ not in (3, 7) and cbp != 0)
        dq = int(s[72]) if has_delta else 0
        raw = pred_qp + dq
        qpy[addr] = (raw + 52) % 52
        if raw < 0:
            qcls.append(('qp', 'wrap_below0'))
        if raw > 51:
            qcls.append(('qp', 'wrap_above51'))
        carried[addr] = None if has_delta else {3: 'skip', 7: 'pcm'}.get(typ, 'cbp0')
        if has_delta and dq != 0:
            if addr == first and first > 0:
                qcls.append(('qp', 'slice_start'))
            elif addr > first and carried[addr - 1]:
                qcls.append(('qp', 'carry_' + carried[addr - 1]))
        qp = int(qpy[addr])
        qpi = qp + cqp
        qpc = QPC[min(51, max(0, qpi))]
        if typ != 7 and (cbp >> 4):
            if qpi < 0:
                qcls.append(('qp', 'qpc_clip0'))
            if qpi > 51:
                qcls.append(('qp', 'qpc_clip51'))
        r = rec[addr]
        r[0], r[1], r[54], r[55], r[56], r[57], r[58] = typ, qp, first, s[77], s[78], s[79], cqp
        r[18:22] = -1 if typ in (0, 1, 7) else 0
        note(addr, 'all', 0, 0, 16, 16, f'QPY,PRED {pred_qp} mb_qp_delta {dq} QPC {qpc} coded_block_pattern {cbp}', qcls)

        if typ == 7:      # ---- I_PCM (8.3.5)
            pcm = s[488:872]
            pic.P[0][Y:Y + 16, X:X + 16] = pcm[:256].reshape(16, 16)
            pic.P[1][Y // 2:Y // 2 + 8, X // 2:X // 2 + 8] = pcm[256:320].reshape(8, 8)
            pic.P[2][Y // 2:Y // 2 + 8, X // 2:X // 2 + 8] = pcm[320:384].reshape(8, 8)
            for pl, sz in ((0, 16), (1, 8), (2, 8)):
                py, px = Y * sz // 16, X * sz // 16
                assert (pic.pred[pl][py:py + sz, px:px + sz] == -1).all()
                pic.pred[pl][py:py + sz, px:px + sz] = pic.P[pl][py:py + sz, px:px + sz]
            r[2:18] = 16
            _finish_mb(pic, addr, intra=True)
            continue

        # ---- residual (8.5): r of every luma block as [blkIdx, y, x], of every chroma block as [plane][blk, y, x]
        rcls = []
        luma_lv = s[96:352].reshape(16, 16)
        nz = np.zeros(16, np.int32)
        c = np.zeros((16, 4, 4), np.int64)
        for b in range(16):
            if not (cbp >> (b >> 2)) & 1:
                continue
            lv = list(luma_lv[b])
            c[b] = _unscan([0] + lv[:15]) if typ == 1 else _unscan(lv)
            nz[b] = np.count_nonzero(lv)
        if typ == 1:
            dcy = _luma_dc(list(s[80:96]), qp)
            rcls.append(('i16dc', 'ge36' if qp >= 36 else 'lt36'))
            for b in range(16):
                c[b, 0, 0] = dcy[BLK_XY[b][1] // 4, BLK_XY[b][0] // 4]
        res_y = _transform(_scale(c, qp, keep_dc=(typ == 1)))
        _count_blocks(rcls, 'Y', c, nz if typ != 1 else None, qp, typ == 1)
        res_c = []
        for k in (0, 1):
            cc = np.zeros((4, 4, 4), np.int64)
            if cbp >> 4:
                rcls.append(('chroma_dc_qp', 'ge6' if qpc >= 6 else 'lt6'))
                dcc = _chroma_dc(list(s[352 + 4 * k:356 + 4 * k]), qpc)
                for b in range(4):
                    if (cbp >> 4) == 2:
                        cc[b] = _unscan([0] + list(s[360 + 64 * k + 16 * b:360 + 64 * k + 16 * b + 15]))
                    cc[b, 0, 0] = dcc[b >> 1, b & 1]
            res_c.append(_transform(_scale(cc, qpc, keep_dc=True)))
            _count_blocks(rcls, 'Cb' if k == 0 else 'Cr', cc, None, qpc, True)
        for b in range(16):     # TotalCoeff of each luma block, raster order of the record
            r[2 + (BLK_XY[b][1] // 4) * 4 + BLK_XY[b][0] // 4] = nz[b]
        note(addr, 'all', 0, 0, 16, 16, 'residual', rcls)

        def put(plane, px, py, pred, res, kind):
            """u = Clip1(pred + r) (8-354) into the picture, the samples flagged constructed"""
            u = pred + res
            cls = []
            if (u < 0).any():
                cls.append(('clip1', 'at0', kind))
            if (u > 255).any():
                cls.append(('clip1', 'at255', kind))
            hh, ww = u.shape
            pic.P[plane][py:py + hh, px:px + ww] = np.clip(u, 0, 255)
            pic.built[plane][py:py + hh, px:px + ww] = True
            assert (pic.pred[plane][py:py + hh, px:px + ww] == -1).all(), 'a sample predicted twice'
            pic.pred[plane][py:py + hh, px:px + ww] = pred
            return cls

        if typ in (0, 1):     # ---- intra (8.3)
            if typ == 0:
                for b in range(16):
                    bx, by = BLK_XY[b]
                    cls = []
                    # 8.3.1.1
                    nA = _i4_neighbour_mode(pic, addr, gx + bx // 4 - 1, gy + by // 4)
                    nB = _i4_neighbour_mode(pic, addr, gx + bx // 4, gy + by // 4 - 1)
                    if nA[1] == 'unavailable' or nB[1] == 'unavailable':
                        predmode = 2
                        cls.append(('i4pred', 'dc_by_unavailable'))
                    else:
                        for n in (nA, nB):
                            if n[1] in ('inter', 'i16_or_pcm'):
                                cls.append(('i4pred', 'dc_by_' + n[1]))
                        predmode = min(nA[0], nB[0])
                    if int(s[38 + b]):
                        mode = predmode
                        cls.append(('i4pred', 'prev_flag_1'))
                    else:
                        rem = int(s[54 + b])
                        mode = rem if rem < predmode else rem + 1
                        cls += [('i4pred', 'prev_flag_0'), ('i4pred', 'rem_below' if rem < predmode else 'rem_at_or_above')]
                    pic.i4[gy + by // 4, gx + bx // 4] = mode
                    pic.derived[gy + by // 4, gx + bx // 4] = True
                    pred = _pred4x4(_Nb(pic, 0, addr, X + bx, Y + by), mode, cls)
                    cls += put(0, X + bx, Y + by, pred, res_y[b], 'intra')
                    note(addr, 'luma', bx, by, 4, 4, f'luma4x4BlkIdx {b}: predIntra4x4PredMode {predmode}, Intra4x4PredMode {mode} ({I4_NAMES[mode]})', cls)
            else:
                cls = []
                pred = _pred_square(_Nb(pic, 0, addr, X, Y), 16, ['V', 'H', 'DC', 'plane'][i16_mode], cls, 'i16')
                for b in range(16):
                    bx, by = BLK_XY[b]
                    cls += [k for k in put(0, X + bx, Y + by, pred[by:by + 4, bx:bx + 4], res_y[b], 'intra') if k not in cls]
                note(addr, 'luma', 0, 0, 16, 16, f'Intra16x16PredMode {i16_mode}', cls)
            cm = int(s[70])
            for k in (0, 1):
                cls = []
                pred = _pred_square(_Nb(pic, 1 + k, addr, X // 2, Y // 2), 8, ['DC', 'H', 'V', 'plane'][cm], cls, 'chroma')
                for b in range(4):
                    ox, oy = 4 * (b & 1), 4 * (b >> 1)
                    cls += [q for q in put(1 + k, X // 2 + ox, Y // 2 + oy, pred[oy:oy + 4, ox:ox + 4], res_c[k][b], 'intra') if q not in cls]
                note(addr, 'chroma', 0, 0, 16, 16, f"intra_chroma_pred_mode {cm} ({'Cb' if k == 0 else 'Cr'})", cls)
            _finish_mb(pic, addr, intra=True)
            continue

        # ---- inter (8.4): the partitions in decoding order, each (x, y, w, h, shape, index)
        assert ref_planes is not None, 'a P macroblock without a reference picture'
        if typ == 3:
            parts = [(0, 0, 16, 16, 'skip', 0)]
        elif typ == 2:
            parts = [(0, 0, 16, 16, None, 0)]
            skip_mv[addr] = tuple(_skip_mv(pic, addr)[0])
        elif typ == 4:
            parts = [(0, 0, 16, 8, '16x8', 0), (0, 8, 16, 8, '16x8', 1)]
        elif typ == 5:
            parts = [(0, 0, 8, 16, '8x16', 0), (8, 0, 8, 16, '8x16', 1)]
        else:
            parts = []
            for q in range(4):
                sw, sh = [(8, 8), (8, 4), (4, 8), (4, 4)][int(s[2 + q])]       # Table 7-17
                parts += [(8 * (q & 1) + xx, 8 * (q >> 1) + yy, sw, sh, None, 0) for yy in range(0, 8, sh) for xx in range(0, 8, sw)]
        pred_y = np.zeros((16, 16), np.int64)
        pred_c = [np.zeros((8, 8), np.int64), np.zeros((8, 8), np.int64)]
        for k, (x, y, w, h, shape, idx) in enumerate(parts):
            if shape == 'skip':
                mv, cls = _skip_mv(pic, addr)
                mvd = (0, 0)
            else:
                mvp, cls = _mvp(pic, addr, x, y, w, h, shape, idx)
                mvd = (int(s[6 + 2 * k]), int(s[7 + 2 * k]))
                mv = (mvp[0] + mvd[0], mvp[1] + mvd[1])                          # 8-174, 8-175
            pic.mv[gy + y // 4:gy + (y + h) // 4, gx + x // 4:gx + (x + w) // 4] = mv
            pic.ref[gy + y // 4:gy + (y + h) // 4, gx + x // 4:gx + (x + w) // 4] = 0
            pic.derived[gy + y // 4:gy + (y + h) // 4, gx + x // 4:gx + (x + w) // 4] = True
            pred_y[y:y + h, x:x + w] = _luma_pred(hv, X + x, Y + y, w, h, mv[0], mv[1])
            for c_ in (0, 1):
                pred_c[c_][y // 2:(y + h) // 2, x // 2:(x + w) // 2] = _chroma_pred(np.asarray(ref_planes[1 + c_]), (X + x) // 2, (Y + y) // 2,
                                                                                  w // 2, h // 2, mv[0], mv[1])
            cls = list(cls) + [('luma_frac', f'{w}x{h}', mv[0] & 3, mv[1] & 3), ('chroma_frac', bool(mv[0] & 7), bool(mv[1] & 7))]
            cls += _geometry_classes(X + x, Y + y, w, h, mv[0], mv[1], W, H)
            note(addr, 'all', x, y, w, h, f'partition {k} {w}x{h} at ({x},{y}): mvd {mvd} mv {mv} (xFrac {mv[0] & 3}, yFrac {mv[1] & 3})', cls)
        cls = []
        for b in range(16):
            bx, by = BLK_XY[b]
            cls += [q for q in put(0, X + bx, Y + by, pred_y[by:by + 4, bx:bx + 4], res_y[b], 'inter') if q not in cls]
        for k in (0, 1):
            for b in range(4):
                ox, oy = 4 * (b & 1), 4 * (b >> 1)
                cls += [q for q in put(1 + k, X // 2 + ox, Y // 2 + oy, pred_c[k][oy:oy + 4, ox:ox + 4], res_c[k][b], 'inter') if q not in cls]
        note(addr, 'all', 0, 0, 16, 16, 'inter sum', cls)
        _finish_mb(pic, addr, intra=False)

    rec[:, 22:54] = pic.mv.reshape(mbh, 4, mbw, 4, 2).transpose(0, 2, 1, 3, 4).reshape(mbw * mbh, 32)
    planes = tuple(a.astype(np.uint8) for a in pic.P)
    assert all((a >= 0).all() for a in pic.pred), 'a sample without a prediction'
    return Result(planes, rec, counts, units, tuple(a.astype(np.uint8) for a in pic.pred), skip_mv)


def _finish_mb(pic, addr, intra):
    mbx, mby = addr % pic.mbw, addr // pic.mbw
    for pl, s in ((0, 16), (1, 8), (2, 8)):
        pic.built[pl][s * mby:s * mby + s, s * mbx:s * mbx + s] = True
    g = (slice(4 * mby, 4 * mby + 4), slice(4 * mbx, 4 * mbx + 4))
    pic.derived[g] = True
    if intra:
        pic.ref[g] = -1
        pic.mv[g] = 0


def _i4_neighbour_mode(pic, addr, bx, by):
    """8.3.1.1 for the 4x4 block (bx, by) of the picture grid as neighbour of a block of macroblock addr ->
    (intraMxMPredModeN, why it is 2 by rule: 'unavailable' / 'inter' / 'i16_or_pcm' / None)"""
    if not (0 <= bx < 4 * pic.mbw and by >= 0):
        return 2, 'unavailable'
    nb = _mb_of_block(pic, bx, by)
    if nb < pic.first[addr] or nb > addr or not pic.derived[by, bx]:
        return 2, 'unavailable'
    t = int(pic.mbtype[nb])
    if t == 0:
        return int(pic.i4[by, bx]), None
    return 2, ('i16_or_pcm' if t in (1, 7) else 'inter')


def _count_blocks(cls, plane, c, nz, qp, has_dc):
    """classes of the scaled blocks c [blk, y, x] of one plane of one macroblock"""
    coded = [bool(np.any(c[b] != 0)) for b in range(len(c))]
    for b in range(len(c)):
        if not coded[b]:
            continue
        for y in range(4):
            for x in range(4):
                if c[b, y, x] != 0 and not (has_dc and x == 0 and y == 0):
                    k = ('levelscale', plane, qp % 6, _pos_class(x, y))
                    if k not in cls:
                        cls.append(k)
        if np.count_nonzero(c[b]) == 1 and c[b, 0, 0] != 0 and ('block', 'dc_only') not in cls:
            cls.append(('block', 'dc_only'))
    if any(coded) and not all(coded) and ('block', 'empty_beside_coded') not in cls:
        cls.append(('block', 'empty_beside_coded'))
    if any(coded):       # qP / 6 of the plane's qP (QP'Y, QP'C): the shift of 8.5.12.1 to the right, to the right by less, to the left
        k = ('qp_div6', plane, '0' if qp < 6 else ('1' if qp < 12 else ('ge6' if qp >= 36 else None)))
        if k[2] is not None and k not in cls:
            cls.append(k)


def first_difference(res, got_planes, w, h):
    """None, or a message naming the first sample inside the w x h window at which got_planes differ from res.planes"""
    for k, (a, b) in enumerate(zip(res.planes, got_planes)):
        hh, ww = (h, w) if k == 0 else (h // 2, w // 2)
        ne = np.argwhere(a[:hh, :ww] != np.asarray(b)[:hh, :ww])
        if len(ne):
            y, x = (int(v) for v in ne[0])
            return (f"{len(ne)} samples of plane {'YUV'[k]} differ from tests/reconref.py (clauses 8.3-8.5 reference); first at "
                    f"({'YUV'[k]}, x {x}, y {y}): got {int(np.asarray(b)[y, x])}, reference {int(a[y, x])}; " + ' | '.join(res.explain(k, x, y)))
    return None
