"""The frame-level rate control's independent model -- TEST INFRASTRUCTURE ONLY.

OpenH264's RC_BITRATE_MODE at the wrapper's parameters, one layer, restated in Python from the fixture
tests/golden/openh264_tables.json and DESIGN §3.6 alone -- not from the kernel (enc_bits.inc) nor from the oracle
(oracle/h264o_enc.c), which are siblings written by one hand:

  * PyRc: the state machine -- skip decision, post-skip bookkeeping, VGOP budget, target bits, IDR and picture QP with
    their windows, the picture update with the R-Q model, the buffer and the VBV skip flag. Every outcome of every
    decision is a class of RC_CLASSES, counted per instance in PyRc.counts; counting reads decisions and makes none.
    PyRc.MUTATIONS names single wrong variants of the model for the sensitivity test;
  * frame_complexity(): the preprocessing's per-GOM SAD / variance of the coded-size luma, in NumPy;
  * seq_params(): the table part -- bits per frame, bit bounds, skip buffer, skip QP, area class, bpp column, IDR QP
    range and the first IDR's QP.
"""
import collections
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OH = json.load(open(os.path.join(HERE, 'golden', 'openh264_tables.json')))
T, C = OH['tables'], OH['code_constants']


def cc(name):
    return C[name]['value']


def py_logf(x):
    """musl logf (h264.wasm func 483) from the fixture's table and polynomial, float32 in and out"""
    x = np.float32(x)
    ix = int(np.array([x], np.float32).view(np.uint32)[0])
    if ix == 0x3f800000:
        return np.float32(0.0)
    assert 0x00800000 <= ix < 0x7f800000  # normal positive inputs only (QStep / 100 >= 0.64)
    tab, poly = T['logf_table']['values'], T['logf_poly']['values']
    tmp = (ix - 0x3f330000) & 0xffffffff
    i = (tmp >> 19) & 15
    k = (tmp if tmp < 0x80000000 else tmp - (1 << 32)) >> 23
    iz = (ix - (tmp & 0xff800000)) & 0xffffffff
    z = np.float64(np.array([iz], np.uint32).view(np.float32)[0])
    f = np.float64
    r = z * f(tab[i][0]) + f(-1.0)
    r2 = r * r
    y = (f(poly[1]) * r2 + (f(poly[2]) * r + f(poly[3]))) * r2 + ((f(k) * f(poly[0]) + f(tab[i][1])) + r)
    return np.float32(y)


def py_qstep2qp(q):
    """RcConvertQStep2Qp (func 1226): 0 below the pinned minimum, else trunc(6 logf(q / 100f) / ln2 + 4 + 0.5); the
    int32 QStep is read as uint32 by the float conversion"""
    if q < cc('qstep_min'):
        return 0
    t = py_logf(np.float32(np.float32(q & 0xffffffff) / np.float32(100.0)))
    return int((np.float64(np.float32(t * np.float32(6.0))) / cc('qstep_conv_ln2') + cc('qstep_conv_offset'))
               + cc('qstep_conv_round'))


# ---------------------------------------------------------------- classes
_FAMILIES = [
    # the skip decision before a frame
    ('SKIP', 'BY_FLAG BY_BUFFER RUN_CAP NOT_FULL OFF OVERRIDDEN_BY_IDR BPF_ZERO FLAG_WHILE_OFF'),
    # post-skip bookkeeping
    ('POST', 'CLAMPED UNCLAMPED'),
    ('REFRESH', 'FIRST_IDR'),
    # the virtual GOP
    ('VGOP', 'AT_REFRESH BY_IDR_CARRY_NEG BY_IDR_CARRY_ZERO BY_COUNT_CARRY_NEG BY_COUNT_CARRY_ZERO CONTINUES'),
    # target bits
    ('TGT', 'FIRST_IDR LATER_IDR SHARE CLIP_LO CLIP_HI BITS_LEVEL2 NONPOS_SKIP_ON RW_BELOW_WEIGHT RW_ZERO'),
    # IDR QP
    ('IDRQP', 'TABLE TABLE_CLIPPED MODEL MODEL_CLIP_LO MODEL_CLIP_HI WIN_LO_IN WIN_LO_CLIPPED WIN_HI_IN WIN_HI_CLIPPED MB_RESCALE'),
    # picture QP
    ('PQP', 'FIRST FIRST_CLIPPED EXCEEDED EXCEEDED_CLIP_HI EXCEEDED_CLIP_LO MODEL MODEL_CLIP_LO MODEL_CLIP_HI '
            'WIN_LO_IN WIN_LO_AT12 WIN_LO_AT42 WIN_HI_IN WIN_HI_AT42 WIN_HI_AT12'),
    # the complexity ratio of a P frame and of a later IDR
    ('PRATIO', 'MEAN_ZERO CLIP_LO CLIP_HI INSIDE'),
    ('IRATIO', 'MEAN_ZERO CLIP_LO CLIP_HI INSIDE'),
    # the QStep model and its conversion
    ('QSTEP', 'TARGET_ZERO TO_QP_ZERO TO_QP_MID TO_QP_TOP'),
    # the picture update
    ('UPD', 'FIRST_P LATER_P FIRST_IDR LATER_IDR PFRAMES_SATURATED IDRS_SATURATED AVG_IDR AVG_P_FROM_MBS AVG_P_NO_MB '
            'SKIP_OFF FLAG_BUFFER_ONLY FLAG_OVERSPENT_ONLY FLAG_BOTH FLAG_NONE VGOP_LE6 VGOP_GT6 BPF_ZERO'),
    # the sequence parameters
    ('SEQ', 'NARROW WIDE AREA0 AREA1 AREA2 AREA3 COL0 COL1 COL2 COL3 COL4'),
    # the frame complexity
    ('FC', 'P_SAD I_VAR SUMSQ_WRAP SUMSQ_NOWRAP W_NOT16 H_NOT16 ALIGNED PARTIAL_LAST_GOM WHOLE_LAST_GOM GOMS_GT8 GOMS_LE8 NARROW WIDE'),
]
RC_CLASSES = [f'{fam}_{n}' for fam, names in _FAMILIES for n in names.split()]
assert len(RC_CLASSES) == len(set(RC_CLASSES))
_KNOWN = frozenset(RC_CLASSES)


def _geometry(w, h, narrow_at=31):
    """narrow_at: the width in MBs from which a picture is wide (31; the sensitivity test moves it)"""
    w16, h16 = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    mbw, mbh = w16 // 16, h16 // 16
    narrow = mbw < narrow_at
    rows = cc('gom_rows_narrow') if narrow else cc('gom_rows_wide')
    return w16, h16, mbw, mbh, narrow, rows


def seq_params(w, h, bitrate, counts=None, narrow_at=31):
    """the table part of the sequence's rate control (RcInitSequenceParameter, RcUpdateBitrateFps, RcCalculateIdrQp's
    table look-up) -> dict: bpf, min_bits, max_bits, buf_size, skip_qp, area (class 0..3), col (bpp column 0..4),
    idr_lo, idr_hi (the IDR QP range), init_qp (the first IDR's QP)"""
    w16, h16, mbw, mbh, narrow, rows = _geometry(w, h, narrow_at)
    vary, weight = cc('rc_vary_percentage'), T['rc_tl_weight']['values'][0][0]
    fps = np.float32(cc('default_max_frame_rate'))
    bpf = int((fps * np.float32(0.5) + np.float32(bitrate)) / fps)
    lo = 100 - ((cc('min_bits_base') - vary) >> 1)
    div = cc('bits_tl_divisor')
    bpp = bitrate / float(np.float32(np.float32(fps * np.float32(w16)) * np.float32(h16)))
    area = w16 * h16
    cls = 0 if area < cc('area_90p') else 1 if area < cc('area_180p') else 2 if area < cc('area_360p') else 3
    i = 1 - cc('default_fix_rc_overshoot')
    while i < 4 and not T['rc_bpp']['values'][cls][i] >= bpp:
        i += 1
    qmin, qmax = cc('camera_min_qp'), cc('camera_max_qp')
    hi_, lo_ = (min(max(v, qmin), qmax) for v in T['rc_qp_range']['values'][i])
    if counts is not None:
        counts.update(['SEQ_NARROW' if narrow else 'SEQ_WIDE', f'SEQ_AREA{cls}', f'SEQ_COL{i}'])
    return {'bpf': bpf, 'max_bits': (bpf * cc('max_bits_ratio') * weight + div // 2) // div,
            'min_bits': (bpf * lo * weight + div // 2) // div, 'buf_size': (cc('skip_buffer_ratio') * bitrate + 50) // 100,
            'skip_qp': cc('skip_qp_value_narrow') if narrow else cc('skip_qp_value_wide'), 'area': cls, 'col': i,
            'idr_lo': lo_, 'idr_hi': hi_, 'init_qp': T['rc_init_qp']['values'][cls][i]}


def luma_coded(frame, w, h):
    """the coded-size luma of a tight I420 frame: right and bottom edges repeated to whole macroblocks"""
    w16, h16 = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    y = np.asarray(frame, np.uint8).ravel()[:w * h].reshape(h, w)
    return np.pad(y, ((0, h16 - h), (0, w16 - w)), mode='edge')


def frame_complexity(cur, prev_coded_source, w, h, idr, counts=None, narrow_at=31):
    """the preprocessing's frame complexity: per GOM of whole MB rows -- one row below 31 MBs wide, two
    from 31 on, the last GOM what is left -- the luma SAD of the coded-size source against the last coded frame's
    source (P), or square sum - sum^2 / (MBs of the first row << 8) (IDR), each a uint32 that wraps, and so their sum.
    cur, prev_coded_source: tight I420 frames (or their luma) of w x h"""
    w16, h16, mbw, mbh, narrow, rows = _geometry(w, h, narrow_at)
    a = luma_coded(cur, w, h).astype(np.uint64)
    M = 1 << 32
    goms = -(-mbh // rows)
    total, wrapped = 0, False
    if not idr:
        b = luma_coded(prev_coded_source, w, h).astype(np.int64)
        d = np.abs(a.astype(np.int64) - b)
    for g in range(goms):
        y0, y1 = g * rows * 16, min((g + 1) * rows * 16, h16)
        if idr:
            blk = a[y0:y1]
            s, q = int(blk.sum()), int((blk * blk).sum())
            wrapped |= s * s >= M
            shift = cc('gom_var_sample_shift')
            v = ((q % M) - ((s % M) * (s % M) % M) // (mbw << shift)) % M
        else:
            v = int(d[y0:y1].sum()) % M
        total = (total + v) % M
    if counts is not None:
        k = ['FC_I_VAR' if idr else 'FC_P_SAD', 'FC_NARROW' if narrow else 'FC_WIDE', 'FC_GOMS_GT8' if goms > 8 else 'FC_GOMS_LE8',
             'FC_PARTIAL_LAST_GOM' if mbh % rows else 'FC_WHOLE_LAST_GOM']
        if idr:
            k.append('FC_SUMSQ_WRAP' if wrapped else 'FC_SUMSQ_NOWRAP')
        if w % 16:
            k.append('FC_W_NOT16')
        if h % 16:
            k.append('FC_H_NOT16')
        if w % 16 == 0 and h % 16 == 0:
            k.append('FC_ALIGNED')
        counts.update(k)
    return total


def slice_bytes(nal):
    """bytes of the slice NAL (the access unit minus its parameter-set NALs: another layer for the RC)"""
    starts = [k for k in range(len(nal) - 4) if nal[k:k + 4] == b'\x00\x00\x00\x01']
    for a, b in zip(starts, starts[1:] + [len(nal)]):
        if nal[a + 4] & 31 in (1, 5):
            return b - a
    raise AssertionError('no slice NAL')


class PyRc:
    """RC_BITRATE_MODE at the wrapper's parameters, one layer, from the fixture alone"""

    # single wrong variants of the model (tests/test_rc_audit.py::test_sensitivity): name -> what it changes
    MUTATIONS = {
        'run_cap_gt': 'the run cap compares with > instead of >=',
        'buffer_ge': 'the skip decision takes a buffer equal to its size',
        'post_skip_no_clamp': 'the fullness clamp at 0 after a skipped frame is dropped',
        'post_skip_no_return': 'a skipped frame does not return its bits to the VGOP',
        'vgop_carry_swapped': 'the VGOP carry keeps the surplus instead of the deficit (max for min)',
        'vgop_restart_at_7': 'the VGOP restarts one frame early',
        'floor_division': 'integer division floors instead of truncating',
        'no_rounding': 'WELS_DIV_ROUND64 without its rounding term',
        'later_idr_ratio_off_by_one': 'a later IDR targets 399 % of the frame bits',
        'target_lo_dropped': 'the target is not clipped to the lower bound',
        'target_hi_dropped': 'the target is not clipped to the upper bound',
        'bits_level_with_skip_on': 'BITS_EXCEEDED is raised with skipping on too',
        'exceeded_step_2': 'BITS_EXCEEDED adds 2 to the QP',
        'window_lower_2': 'the frame window reaches 2 below the last QP',
        'window_upper_6': 'the frame window reaches 6 above the last QP',
        'window_floor_13': 'the frame window is clipped at 13 below',
        'window_cap_41': 'the frame window is clipped at 41 above',
        'idr_window_2': 'the IDR window is +-2',
        'idr_range_swapped': 'the IDR QP is clipped with the bounds swapped',
        'ratio_lo_79': 'the complexity ratio is clipped at 79 below',
        'ratio_hi_121': 'the complexity ratio is clipped at 121 above',
        'decay_19': 'the models decay with 19 / 81',
        'first_p_keeps_model': 'the first P frame updates the model by the EMA',
        'pframes_unsaturated': 'the P frame count does not saturate',
        'idrs_unsaturated': 'the IDR count does not saturate',
        'vbv_le5': 'the VBV prediction stops one frame early',
        'vbv_diff_minus4': 'the VBV overspend is judged against -4',
        'fullness_unsigned_bpf': 'the buffer is not drained by the frame bits at the update',
        'skip_qp_ge': 'the VBV check takes an average QP equal to the skip QP',
        'ratio_mean_zero_unscaled': 'a zero mean gives the complexity instead of 100 x the complexity',
        'narrow_below_32': 'pictures of 31 MBs count as narrow: one-row GOMs and skip QP 24',
    }

    def __init__(self, w, h, br, skip_en=True, mutation=None):
        assert mutation is None or mutation in self.MUTATIONS, mutation
        self.mut = mutation
        self.counts = collections.Counter()
        vary = cc('rc_vary_percentage')
        self.w, self.h = w, h
        w16, h16 = (w + 15) // 16 * 16, (h + 15) // 16 * 16
        self.mbw, self.nmb = w16 // 16, (w16 // 16) * (h16 // 16)
        self.narrow_at = 32 if mutation == 'narrow_below_32' else 31
        self.seq = seq_params(w, h, br, self.counts, self.narrow_at)
        self.skip_qp = self.seq['skip_qp']
        self.w16, self.h16, self.br, self.vary, self.skip_en = w16, h16, br, vary, skip_en
        self.qmin, self.qmax = cc('camera_min_qp'), cc('camera_max_qp')
        if mutation == 'window_floor_13':
            self.qmin = 13
        if mutation == 'window_cap_41':
            self.qmax = 41
        self.weight = T['rc_tl_weight']['values'][0][0]
        self.gop_num = cc('vgop_gops')
        self.idr_num = 0
        self.skip_flag, self.continual, self.fullness = False, 0, 0
        for k in ('remaining', 'vgop_bits', 'remaining_weights', 'gop_index', 'coded_in_vgop', 'target', 'bpf',
                  'pframes', 'intra_mb_count', 'intra_cmplx', 'intra_mean', 'lin', 'mean', 'last_qscale', 'init_qp',
                  'qp', 'min_qp', 'max_qp', 'bits_level', 'avg_qp', 'buf_size', 'min_bits', 'max_bits', 'cmplx'):
            setattr(self, k, 0)
        # the frame driver (begin / end / fail): what a frame step knows beside the rate control's own state
        self.first, self.pending_idr, self.failed, self.last_skipped, self.cur_idr = True, False, False, False, False
        self.prev_source = None

    def hit(self, name):
        assert name in _KNOWN, name
        self.counts[name] += 1

    def cdiv(self, a, b):  # C integer division (truncates toward zero)
        if self.mut == 'floor_division':
            return a // b
        q = abs(a) // abs(b)
        return q if (a >= 0) == (b > 0) else -q

    def div_round(self, x, y):  # WELS_DIV_ROUND64
        if self.mut == 'no_rounding':
            return x if y == 0 else self.cdiv(x, y)
        return x if y == 0 else self.cdiv(x + self.cdiv(y, 2), y)

    def update_bitrate_fps(self):
        fps = np.float32(cc('default_max_frame_rate'))
        self.bpf = int((fps * np.float32(0.5) + np.float32(self.br)) / fps)
        lo = 100 - ((cc('min_bits_base') - self.vary) >> 1)
        div = cc('bits_tl_divisor')
        self.max_bits = (self.bpf * cc('max_bits_ratio') * self.weight + div // 2) // div
        self.min_bits = (self.bpf * lo * self.weight + div // 2) // div
        self.buf_size = (cc('skip_buffer_ratio') * self.br + 50) // 100

    def init_vgop(self, why='REFRESH'):
        t = self.remaining + (self.gop_index - self.gop_num) * self.cdiv(self.vgop_bits, self.gop_num)
        self.hit('VGOP_AT_REFRESH' if why == 'REFRESH' else f'VGOP_BY_{why}_CARRY_{"NEG" if t < 0 else "ZERO"}')
        carry = max(t, 0) if self.mut == 'vgop_carry_swapped' else min(t, 0)
        self.remaining = carry + (self.bpf << cc('vgop_bits_shift'))
        self.vgop_bits = self.remaining
        self.gop_index = self.coded_in_vgop = 0
        self.remaining_weights = self.gop_num * cc('weight_multiply')

    def judge_skip(self):
        if not self.skip_flag:
            if not self.skip_en:
                self.hit('SKIP_OFF')
                return False
            if self.bpf == 0:
                self.hit('SKIP_BPF_ZERO')
            pred = (self.div_round(self.fullness, self.bpf) + 1) >> 1
            full = self.fullness >= self.buf_size if self.mut == 'buffer_ge' else self.fullness > self.buf_size
            cap = pred > self.continual if self.mut == 'run_cap_gt' else pred >= self.continual
            self.skip_flag = cap and full
            if not self.skip_flag:
                self.hit('SKIP_RUN_CAP' if full else 'SKIP_NOT_FULL')
                return False
            self.hit('SKIP_BY_BUFFER')
        else:
            self.hit('SKIP_BY_FLAG' if self.skip_en else 'SKIP_FLAG_WHILE_OFF')
        self.skip_flag = False
        self.continual += 1
        return True

    def post_skip(self):
        self.hit('POST_CLAMPED' if self.fullness - self.bpf < 0 else 'POST_UNCLAMPED')
        self.fullness = self.fullness - self.bpf if self.mut == 'post_skip_no_clamp' else max(0, self.fullness - self.bpf)
        if self.mut != 'post_skip_no_return':
            self.remaining += self.bpf

    def ratio(self, fc, mean, fam='PRATIO'):
        if mean == 0:
            r = fc if self.mut == 'ratio_mean_zero_unscaled' else fc * 100
        else:
            r = self.div_round(fc * 100, mean)
        lo = 79 if self.mut == 'ratio_lo_79' else cc('cmplx_ratio_lo')
        hi = 121 if self.mut == 'ratio_hi_121' else cc('cmplx_ratio_hi')
        self.hit(f'{fam}_MEAN_ZERO' if mean == 0 else f'{fam}_CLIP_LO' if r < lo else f'{fam}_CLIP_HI' if r > hi else f'{fam}_INSIDE')
        return min(max(r, lo), hi)

    def qstep(self, cmplx, ratio):
        if self.target == 0:
            self.hit('QSTEP_TARGET_ZERO')
        v = cmplx * ratio if self.target == 0 else self.div_round(cmplx * ratio, self.target * 100)
        return ((v + (1 << 31)) % (1 << 32)) - (1 << 31)  # wrapped to int32

    def to_qp(self, qstep):
        q = py_qstep2qp(qstep)
        self.hit('QSTEP_TO_QP_ZERO' if q == 0 else 'QSTEP_TO_QP_TOP' if q >= 51 else 'QSTEP_TO_QP_MID')
        return q

    def picture_init(self, idr, fc):
        self.continual = 0
        self.cmplx = fc
        if idr and self.idr_num == 0:
            self.hit('REFRESH_FIRST_IDR')
            self.intra_cmplx = self.intra_mb_count = self.intra_mean = 0
            self.pframes = self.lin = self.mean = 0
            self.fullness = self.gop_index = self.vgop_bits = self.remaining = 0
            self.bpf = 0
            self.update_bitrate_fps()
            self.init_vgop()
        restart = self.gop_num - 1 if self.mut == 'vgop_restart_at_7' else self.gop_num
        if self.gop_index == restart or idr:
            self.init_vgop('IDR' if idr else 'COUNT')
        else:
            self.hit('VGOP_CONTINUES')
        self.gop_index += 1
        self.bits_level = 0
        if idr:
            later = 399 if self.mut == 'later_idr_ratio_off_by_one' else cc('default_idr_bitrate_ratio')
            self.hit('TGT_LATER_IDR' if self.idr_num else 'TGT_FIRST_IDR')
            self.target = later * self.bpf // 100 if self.idr_num else self.bpf << cc('first_idr_target_shift')
        else:
            rw, wt = self.remaining_weights, self.weight
            if rw < wt:
                self.hit('TGT_RW_BELOW_WEIGHT')
                tb = self.remaining
            elif rw == 0:
                self.hit('TGT_RW_ZERO')
                tb = self.remaining * wt
            else:
                tb = self.cdiv(self.cdiv(rw, 2) + self.remaining * wt, rw)
            if tb <= 0 and (not self.skip_en or self.mut == 'bits_level_with_skip_on'):
                self.bits_level = 2
                self.hit('TGT_BITS_LEVEL2')
            elif tb <= 0:
                self.hit('TGT_NONPOS_SKIP_ON')
            self.hit('TGT_CLIP_LO' if tb < self.min_bits else 'TGT_CLIP_HI' if tb > self.max_bits else 'TGT_SHARE')
            lo = tb if self.mut == 'target_lo_dropped' else self.min_bits
            hi = tb if self.mut == 'target_hi_dropped' else self.max_bits
            self.target = min(max(tb, lo), hi)
        self.remaining_weights -= self.weight
        if idr:
            sq = self.seq
            cls, i, lo_, hi_ = sq['area'], sq['col'], sq['idr_lo'], sq['idr_hi']
            if self.idr_num == 0:
                q = sq['init_qp']
                self.hit('IDRQP_TABLE' if lo_ <= q <= hi_ else 'IDRQP_TABLE_CLIPPED')
            else:
                if self.nmb != self.intra_mb_count:
                    self.hit('IDRQP_MB_RESCALE')
                    self.intra_cmplx = self.cdiv(self.intra_cmplx * self.nmb, self.intra_mb_count)
                q = self.to_qp(self.qstep(self.intra_cmplx, self.ratio(fc, self.intra_mean, 'IRATIO')))
                self.hit('IDRQP_MODEL_CLIP_LO' if q < lo_ else 'IDRQP_MODEL_CLIP_HI' if q > hi_ else 'IDRQP_MODEL')
            q = max(min(q, lo_), hi_) if self.mut == 'idr_range_swapped' else min(max(q, lo_), hi_)
            self.init_qp = q
            w_ = 2 if self.mut == 'idr_window_2' else cc('idr_frame_qp_window')
            self.hit('IDRQP_WIN_LO_CLIPPED' if q - w_ < lo_ else 'IDRQP_WIN_LO_IN')
            self.hit('IDRQP_WIN_HI_CLIPPED' if q + w_ > hi_ else 'IDRQP_WIN_HI_IN')
            self.min_qp, self.max_qp = min(max(q - w_, lo_), hi_), min(max(q + w_, lo_), hi_)
        else:
            dl = 2 if self.mut == 'window_lower_2' else cc('frame_delta_qp_lower')
            du = 6 if self.mut == 'window_upper_6' else cc('frame_delta_qp_upper')
            lo_u, hi_u = self.last_qscale - dl, self.last_qscale + du
            self.hit('PQP_WIN_LO_AT12' if lo_u < self.qmin else 'PQP_WIN_LO_AT42' if lo_u > self.qmax else 'PQP_WIN_LO_IN')
            self.hit('PQP_WIN_HI_AT12' if hi_u < self.qmin else 'PQP_WIN_HI_AT42' if hi_u > self.qmax else 'PQP_WIN_HI_IN')
            self.min_qp = min(max(lo_u, self.qmin), self.qmax)
            self.max_qp = min(max(hi_u, self.qmin), self.qmax)
            if self.pframes == 0:
                q, fam = self.init_qp, 'FIRST'
            elif self.bits_level == 2:
                q, fam = self.last_qscale + (2 if self.mut == 'exceeded_step_2' else cc('bits_exceeded_qp_step')), 'EXCEEDED'
            else:
                q, fam = self.to_qp(self.qstep(self.lin, self.ratio(fc, self.mean))), 'MODEL'
            if fam == 'FIRST':
                self.hit('PQP_FIRST' if self.min_qp <= q <= self.max_qp else 'PQP_FIRST_CLIPPED')
            else:
                self.hit(f'PQP_{fam}_CLIP_LO' if q < self.min_qp else f'PQP_{fam}_CLIP_HI' if q > self.max_qp else f'PQP_{fam}')
            q = min(max(q, self.min_qp), self.max_qp)
        self.qp = self.last_qscale = q

    def picture_update(self, idr, slice_bytes, avg, fc, coded_mbs=None):
        """coded_mbs (macroblocks with bits, where the caller knows them) only tells the AVG classes apart"""
        bits = slice_bytes * 8
        self.last_qscale = self.avg_qp = avg
        if coded_mbs is not None:
            self.hit('UPD_AVG_IDR' if idr else 'UPD_AVG_P_FROM_MBS' if coded_mbs else 'UPD_AVG_P_NO_MB')
            assert idr or coded_mbs or avg == self.qp, 'no macroblock coded: the average QP is the frame QP'
        qs = T['rc_qstep']['values'][avg]
        new, old = cc('cmplx_decay_new'), cc('cmplx_decay_old')
        if self.mut == 'decay_19':
            new, old = 19, 81
        if not idr:
            if self.pframes == 0 and self.mut != 'first_p_keeps_model':
                self.hit('UPD_FIRST_P')
                self.mean, self.lin = fc, bits * qs
            else:
                self.hit('UPD_LATER_P')
                self.mean = self.cdiv(fc * new + self.mean * old + 50, 100)
                self.lin = self.cdiv(self.lin * old + qs * bits * new + 50, 100)
            if self.pframes >= 254:
                self.hit('UPD_PFRAMES_SATURATED')
            self.pframes = (self.pframes if self.mut == 'pframes_unsaturated' else min(self.pframes, 254)) + 1
        else:
            ic = qs * bits
            if self.idr_num == 0:
                self.hit('UPD_FIRST_IDR')
                self.intra_mean, self.intra_cmplx = fc, ic
            else:
                self.hit('UPD_LATER_IDR')
                self.intra_cmplx = self.cdiv(ic * new + self.intra_cmplx * old + 50, 100)
                self.intra_mean = self.cdiv(fc * new + self.intra_mean * old + 50, 100)
            self.intra_mb_count = self.nmb
            if self.idr_num >= 254:
                self.hit('UPD_IDRS_SATURATED')
            self.idr_num = (self.idr_num if self.mut == 'idrs_unsaturated' else min(self.idr_num, 254)) + 1
        self.remaining -= bits
        if self.skip_en:
            self.fullness += bits if self.mut == 'fullness_unsigned_bpf' else bits - self.bpf
            last = 5 if self.mut == 'vbv_le5' else 6
            self.hit('UPD_VGOP_LE6' if self.coded_in_vgop <= 6 else 'UPD_VGOP_GT6')
            pred = sum(self.min_bits for _ in range(self.coded_in_vgop + 1, 8)) if self.coded_in_vgop <= last else 0
            if self.bpf == 0:
                self.hit('UPD_BPF_ZERO')
            diff = -4.0 if self.mut == 'vbv_diff_minus4' else cc('vbv_percent_diff')
            inc = (float(pred - self.remaining) * cc('vbv_percent')) / float(self.bpf << cc('vbv_vgop_shift')) + diff
            over_qp = avg >= self.skip_qp if self.mut == 'skip_qp_ge' else avg > self.skip_qp
            a, b = self.fullness > self.buf_size and over_qp, inc > self.vary
            self.hit('UPD_FLAG_BOTH' if a and b else 'UPD_FLAG_BUFFER_ONLY' if a else 'UPD_FLAG_OVERSPENT_ONLY' if b else 'UPD_FLAG_NONE')
            if a or b:
                self.skip_flag = True
        else:
            self.hit('UPD_SKIP_OFF')
        self.coded_in_vgop += 1

    # ------------------------------------------------------------ a frame step, as the encoder's begin / pack see it
    def force_idr(self):
        self.pending_idr = True

    def begin(self, frame):
        """the frame step's first half on a tight I420 frame: the skip decision, and for a coded frame the complexity
        (frame_complexity against the last coded frame's source) and the picture init. -> True when the frame is coded.
        A frame that failed (fail()) is followed by an IDR."""
        idr = self.first or self.pending_idr or self.failed
        self.failed = False
        chosen = self.judge_skip()
        if chosen and idr:
            self.hit('SKIP_OVERRIDDEN_BY_IDR')
        self.last_skipped = chosen and not idr
        if self.last_skipped:
            self.post_skip()
            return False
        self.first = self.pending_idr = False
        self.cur_idr = idr
        fc = frame_complexity(frame, self.prev_source, self.w, self.h, idr, self.counts, self.narrow_at)
        self.prev_source = np.array(frame, np.uint8).ravel()[:self.w * self.h].copy()
        self.picture_init(idr, fc)
        return True

    def end(self, nal, avg_qp, coded_mbs=None):
        """the second half of a coded frame: the picture update on the access unit's slice bytes and average QP"""
        self.picture_update(self.cur_idr, slice_bytes(nal), avg_qp, self.cmplx, coded_mbs)

    def fail(self):
        """the coded frame produced no output: the picture init stands -- VGOP index, weights, target, QP,
        window, the preprocessing's reference picture --, no update is made, and the next frame is an IDR"""
        self.failed = True

    def state(self):
        """the sixteen fields of h264mi_enc_rc_state / h264o_enc_rc_state"""
        i32 = lambda v: ((int(v) + (1 << 31)) % (1 << 32)) - (1 << 31)
        return {'skipped': int(self.last_skipped), 'qp': self.qp, 'avg_qp': self.avg_qp, 'target': self.target,
                'remaining': self.remaining, 'fullness': i32(self.fullness), 'continual': self.continual, 'cmplx': i32(self.cmplx),
                'min_qp': self.min_qp, 'max_qp': self.max_qp, 'bpf': self.bpf, 'pframes': self.pframes, 'idrs': self.idr_num,
                'skip_flag': int(self.skip_flag), 'remaining_weights': self.remaining_weights, 'coded_in_vgop': self.coded_in_vgop}
