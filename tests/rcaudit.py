"""Class audit of the frame-level rate control -- TEST INFRASTRUCTURE ONLY.

tests/rcref.py names every outcome of every decision of the frame-level rate control as a class (RC_CLASSES) and counts
them. This module holds what the CPU audit (tests/test_rc_audit.py) and the GPU tests (tests/test_gpu_rc_audit.py) share:

  - Seq: one directed sequence -- geometry, bitrate, skipping on or off, a content schedule and the frames at which an
    IDR is forced;
  - DIRECTED: the sequences, each with the classes it is the first to reach; LONG_RUNS: the two long static runs;
  - EXCLUDED / NOT_REACHED: the classes no sequence is asked to reach, with the derivation or the reason;
  - oracle_run() / replay(): the oracle over a sequence, and the model fed with the oracle's bytes and average QPs;
  - TABLE_CASES: the geometries and bitrates around every threshold of the sequence parameters;
  - suite_reach(): the classes the inputs of the GPU tests that were there before this audit take;
  - sweep(): the seeded sweep and greedy cover DIRECTED was chosen by (python tests/rcaudit.py).
"""
import functools
import os

import numpy as np

import rcref

# ---------------------------------------------------------------- sequences
# A schedule is a string, one letter per frame:
#   f flat 128          b bright flat (250)      d dark flat (4)        s the frame before, unchanged (static)
#   n fresh noise       l flat 128 with fresh noise of +-6              h fresh noise on the left half, flat right
#   p the frame before with its first luma sample raised by 40 (a SAD of 40)
# A bright picture of two or more macroblocks per row takes the IDR variance's sum^2 beyond 32 bits.
KINDS = 'fbdsnlhp'


class Seq:
    def __init__(self, w, h, br, skip, schedule, idr=(), seed=1, targets=()):
        self.w, self.h, self.br, self.skip, self.schedule, self.seed = w, h, br, bool(skip), schedule, seed
        self.idr, self.targets = frozenset(idr), tuple(targets)
        assert set(schedule) <= set(KINDS) and schedule[0] not in 'sp'
        self.name = f'{w}x{h}_{br}_{"skip" if skip else "noskip"}_{self.tag()}_s{seed}'
        self._t, self._f, self._rng = -1, None, None

    def tag(self):
        sch = self.schedule if len(self.schedule) <= 32 else f'{self.schedule[:4]}x{len(self.schedule)}'
        every = len(self.idr) > 8
        return sch + ('_idrall' if every else ''.join(f'_i{t}' for t in sorted(self.idr)))

    def __len__(self):
        return len(self.schedule)

    def frame(self, t):
        """frame t (tight I420); frames are generated in order from the seed, so frame t costs one pass from 0 the first time"""
        if t < self._t or self._f is None:
            self._t, self._f, self._rng = -1, None, np.random.default_rng(self.seed)
        w, h = self.w, self.h
        while self._t < t:
            self._t += 1
            k = self.schedule[self._t]
            if k == 's':
                continue
            if k == 'p':
                self._f = self._f.copy()
                self._f[0] = (int(self._f[0]) + 40) % 256
                continue
            y = np.full((h, w), 128, np.int64)
            if k == 'b':
                y[:] = 250
            elif k == 'd':
                y[:] = 4
            elif k == 'n':
                y = self._rng.integers(0, 256, (h, w))
            elif k == 'l':
                y = y + self._rng.integers(-6, 7, (h, w))
            elif k == 'h':
                y[:, :max(w // 2, 1)] = self._rng.integers(0, 256, (h, max(w // 2, 1)))
            c = np.full((h // 2) * (w // 2) * 2, 128, np.int64)
            if k in 'nh':
                c = self._rng.integers(96, 160, c.size)
            self._f = np.ascontiguousarray(np.concatenate([y.ravel(), c]).astype(np.uint8))
        return self._f

    def frames(self):
        return [self.frame(t) for t in range(len(self))]


def _oracle():
    from _oracle import Oracle
    return Oracle(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle', 'build', 'libh264_oracle.so'))


def coded_mbs(mbinfo):
    """macroblocks with bits in a record array whose first column is the type (3: P_Skip)"""
    return int((np.asarray(mbinfo)[:, 0] != 3).sum())


def oracle_run(oracle, seq, keep=None):
    """the oracle over a sequence -> per frame (NAL bytes, rc_state, macroblocks with bits); keep: the frames whose bytes
    are kept (a range; the others keep only their slice NAL's length, as a bytes-free stand-in)"""
    oe = oracle.encoder(seq.w, seq.h, seq.br)
    oe.set_frame_skip(seq.skip)
    out = []
    for t in range(len(seq)):
        if t in seq.idr:
            oe.force_idr()
        nal = oe.encode(seq.frame(t))
        n = coded_mbs(oe.mbinfo()) if nal else 0
        out.append((nal if keep is None or t in keep or not nal else rcref.slice_bytes(nal), oe.rc_state(), n))
    return out


@functools.lru_cache(maxsize=None)
def directed_runs():
    o = _oracle()
    return tuple(oracle_run(o, s) for s in directed_seqs())


def _end(model, nal, avg, n):
    if isinstance(nal, int):
        model.picture_update(model.cur_idr, nal, avg, model.cmplx, n)
    else:
        model.end(nal, avg, n)


def replay(seq, run, mutation=None, stop=None):
    """the model over a sequence, fed with the run's bytes and average QPs, its complexity from frame_complexity
    -> (model, None) or (model, (frame, field, model's value, run's value)) at the first disagreement in any of the
    sixteen fields"""
    m = rcref.PyRc(seq.w, seq.h, seq.br, seq.skip, mutation)
    for t, (nal, st, n) in enumerate(run[:stop]):
        if t in seq.idr:
            m.force_idr()
        coded = m.begin(seq.frame(t))
        if coded != bool(nal):
            return m, (t, 'coded', coded, bool(nal))
        if coded:
            try:
                _end(m, nal, st['avg_qp'], n)
            except AssertionError as e:
                return m, (t, 'avg_qp', str(e), st['avg_qp'])
        got = m.state()
        for k in got:
            if got[k] != st[k]:
                return m, (t, k, got[k], st[k])
    return m, None


# ---------------------------------------------------------------- the table sweep
def _rate_for(w16, h16, bpp, side):
    """the bitrates on each side of bpp = bitrate / (60 x w16 x h16) as float32 arithmetic rounds it: the largest
    bitrate whose bpp is still at or below the threshold (side 0), and the next one (side 1)"""
    px = float(np.float32(np.float32(np.float32(60.0) * np.float32(w16)) * np.float32(h16)))
    r = int(bpp * px)
    while r / px <= bpp:
        r += 1
    while (r - 1) / px > bpp:
        r -= 1
    return r - 1 + side


def table_cases():
    """(w, h, bitrate): per area class one geometry, at the bitrates on each side of every bpp column threshold of its
    class -- so every cell of the 4 x 5 table; the MB counts on each side of the three area thresholds that a legal
    geometry has (112 / 113, 450 / 451, 1800 / 1802 MBs); and 16x16 at 3840 bit/s, where bpp equals 0.25 exactly"""
    out = []
    geo = {0: (16, 16), 1: (176, 176), 2: (480, 256), 3: (544, 848)}
    for cls, (w, h) in geo.items():
        for thr in rcref.T['rc_bpp']['values'][cls]:
            for side in (0, 1):
                out.append((w, h, _rate_for(w, h, thr, side)))
    for w, h in ((256, 112), (1808, 16), (480, 240), (656, 176), (800, 576), (544, 848)):
        out.append((w, h, 300000))
    out.append((16, 16, 3840))
    return out


# ---------------------------------------------------------------- classes that no input reaches
_WEIGHTS = ('remaining_weights is set to 8 x 2000 by every VGOP restart and loses 2000 with every coded frame, whose picture init '
            'also raises gop_index by one; the restart comes when gop_index is 8 or at an IDR, before the weights are read. So they '
            'are read at 16000 - 2000 x gop_index with gop_index in 0..7: never below 2000, the weight, and never 0. A failed frame '
            'advances both in its picture init, so the relation holds across it.')
_TARGET = ('the target is 4 x bits per frame (IDR) or clipped to at least min_bits_tl = round(0.55 x bits per frame); bits per frame '
           'is (30 + bitrate) / 60, at least 1 from 30 bit/s on -- less than one macroblock\'s header --, so the target is never 0.')
_TABLE = ('the first IDR QP of every table cell lies inside its column\'s range: the fixture\'s rc_init_qp columns hold 34..36, 28..34, '
          '26..32, 24..30 and 22..28 against the ranges 28..40, 25..37, 24..36, 23..35 and 22..34.')
_FIRSTP = ('pframe_num is 0 only until the first P frame is coded (it is reset at the first IDR alone), so every frame coded before is '
           'an IDR, whose update leaves last_qscale = its QP = init_qp in 22..40: init_qp lies inside [init_qp - 3, init_qp + 5] and '
           'inside 12..42. After a failed IDR last_qscale is that IDR\'s QP as well (its picture init set both).')
_QPRANGE = ('last_qscale is a frame QP or an average of macroblock QPs, all inside a frame window, so it lies in 12..42: last - 3 is '
            'never above 42 and last + 5 never below 12; last + 3 is never below max(last - 3, 12).')
EXCLUDED = {
    'TGT_RW_BELOW_WEIGHT': _WEIGHTS, 'TGT_RW_ZERO': _WEIGHTS,
    'QSTEP_TARGET_ZERO': _TARGET,
    'IDRQP_TABLE_CLIPPED': _TABLE,
    'IDRQP_MB_RESCALE': ('intra_mb_count is set to the picture\'s MB count by every IDR update and is read only at a later IDR (idr_num > 0, '
                         'so at least one IDR update has run); the MB count of a stream never changes.'),
    'PQP_FIRST_CLIPPED': _FIRSTP,
    'PQP_EXCEEDED_CLIP_LO': _QPRANGE, 'PQP_WIN_LO_AT42': _QPRANGE, 'PQP_WIN_HI_AT12': _QPRANGE,
    'SKIP_FLAG_WHILE_OFF': ('the skip flag is set by the update\'s VBV check and by the skip decision\'s buffer test, both behind bEnableFrameSkip, '
                            'which a sequence fixes before its first frame.'),
    'UPD_BPF_ZERO': ('bits per frame is set at the first IDR\'s refresh, before any update, to (30 + bitrate) / 60 > 0; only the skip decision '
                     'of the very first frame reads it at 0 (SKIP_BPF_ZERO).'),
}

# Classes neither reached by a directed sequence nor excluded, with what was tried. Empty: every class is required or excluded.
NOT_REACHED = {}

# ---------------------------------------------------------------- the directed sequences
# (w, h, bitrate, skipping, schedule, frames forced to IDR, seed) and the classes the sequence is in the set for: those it
# is the first of this list to reach. Chosen by sweep() below: a greedy cover over seeded candidates at the geometries
# of the issue, run through the oracle and the model on the CPU.
DIRECTED = [
    ((18, 18, 77760, True, 'fsldddnbbbffffffhhhlllf', (6, 8), 368),
     'SKIP_BY_FLAG SKIP_NOT_FULL SKIP_BPF_ZERO POST_CLAMPED REFRESH_FIRST_IDR VGOP_AT_REFRESH VGOP_BY_IDR_CARRY_NEG VGOP_BY_IDR_CARRY_ZERO VGOP_BY_COUNT_CARRY_ZERO VGOP_CONTINUES TGT_FIRST_IDR TGT_LATER_IDR TGT_SHARE TGT_CLIP_LO TGT_CLIP_HI IDRQP_TABLE IDRQP_MODEL_CLIP_LO IDRQP_WIN_LO_CLIPPED IDRQP_WIN_HI_IN PQP_FIRST PQP_MODEL PQP_MODEL_CLIP_LO PQP_MODEL_CLIP_HI PQP_WIN_LO_IN PQP_WIN_LO_AT12 PQP_WIN_HI_IN PRATIO_MEAN_ZERO PRATIO_CLIP_LO PRATIO_CLIP_HI PRATIO_INSIDE IRATIO_CLIP_LO IRATIO_CLIP_HI QSTEP_TO_QP_ZERO QSTEP_TO_QP_MID UPD_FIRST_P UPD_LATER_P UPD_FIRST_IDR UPD_LATER_IDR UPD_AVG_IDR UPD_AVG_P_FROM_MBS UPD_AVG_P_NO_MB UPD_FLAG_OVERSPENT_ONLY UPD_FLAG_NONE UPD_VGOP_LE6 UPD_VGOP_GT6 SEQ_NARROW SEQ_AREA0 SEQ_COL4 FC_P_SAD FC_I_VAR FC_SUMSQ_WRAP FC_SUMSQ_NOWRAP FC_W_NOT16 FC_H_NOT16 FC_WHOLE_LAST_GOM FC_GOMS_LE8 FC_NARROW'),
    ((512, 48, 29491, False, 'hhhhhhhnsshhhhhhnddnnh', (8, 10, 13), 778),
     'SKIP_OFF VGOP_BY_COUNT_CARRY_NEG TGT_BITS_LEVEL2 IDRQP_MODEL_CLIP_HI IDRQP_WIN_LO_IN IDRQP_WIN_HI_CLIPPED PQP_EXCEEDED PQP_EXCEEDED_CLIP_HI PQP_WIN_HI_AT42 IRATIO_INSIDE QSTEP_TO_QP_TOP UPD_SKIP_OFF SEQ_WIDE SEQ_COL0 FC_ALIGNED FC_PARTIAL_LAST_GOM FC_WIDE'),
    ((176, 144, 6082, True, 'dddddhhhhfff', (1, 2, 7), 200),
     'SKIP_BY_BUFFER SKIP_OVERRIDDEN_BY_IDR POST_UNCLAMPED TGT_NONPOS_SKIP_ON IDRQP_MODEL IRATIO_MEAN_ZERO UPD_FLAG_BOTH FC_GOMS_GT8'),
    ((32, 16, 9216, True, 'bbbffffffbbdddfffffffnnn', (), 828),
     'SEQ_COL1'),
    ((16, 16, 2000, True, 'hhhfffssssnllll', (4, 12, 13), 310),
     'UPD_FLAG_BUFFER_ONLY'),
    ((50, 34, 122400, False, 'bbhhhhhhffffll', (), 648),
     'SEQ_COL2'),
    ((18, 18, 2000, False, 'llllllllllllllllllll', (8,), 91),
     ''),
    ((18, 18, 5832, True, 'nnnnssssssssssnnnnnn', (), 5),
     ''),
    ((50, 34, 408000, True, 'bbbbbblllllnffffl', (4, 5, 12), 370),
     ''),
    ((50, 34, 8160, True, 'ffllsssssshhhhhffffhhhhh', (2, 7, 20), 316),
     ''),
    ((16, 16, 13000, True, 'f', (), 1),
     'SEQ_COL3'),
    ((176, 176, 300000, True, 'f', (), 1),
     'SEQ_AREA1'),
    ((656, 176, 300000, True, 'f', (), 1),
     'SEQ_AREA2'),
    ((544, 848, 300000, True, 'f', (), 1),
     'SEQ_AREA3'),
    # a noise IDR over a tenth of a second of bits, then static frames: 16 and more skipped in a row until the run cap refuses one
    ((16, 16, 2000, True, 'n' * 40, (), 5),
     'SKIP_RUN_CAP'),
    # 31 MBs wide and three MB rows: two-row GOMs from 31 MBs on show in the IDR's and the P frames' complexity
    ((496, 48, 60000, True, 'nnhhs', (3,), 7),
     ''),
    # a static first P frame (mean 0), then one sample changed: the ratio is 100 x the complexity, clipped to 120
    ((16, 16, 4000, False, 'fspss', (), 1),
     ''),
    # noise fills the buffer, then flat forced IDRs whose QP falls to the range's bottom, 24 = the skip QP, over a full buffer
    ((16, 16, 8000, True, 'nnnnnnf' + 's' * 13, tuple(range(6, 20)), 5),
     ''),
]

# the two long static runs at 16x16, skipping off: (sequence, the windows compared frame by frame, classes claimed)
LONG_WINDOWS = {'p': (range(250, 261), range(32760, 32776)), 'idr': (range(250, 261),)}


@functools.lru_cache(maxsize=None)
def long_runs():
    p = Seq(16, 16, 30000, False, 'f' + 's' * 32999, targets=('UPD_PFRAMES_SATURATED',))
    i = Seq(16, 16, 30000, False, 'f' + 's' * 299, idr=range(300), targets=('UPD_IDRS_SATURATED',))
    return {'p': p, 'idr': i}


@functools.lru_cache(maxsize=None)
def directed_seqs():
    return tuple(Seq(*spec, targets=t.split()) for spec, t in DIRECTED)


def required():
    return [c for c in rcref.RC_CLASSES if c not in EXCLUDED and c not in NOT_REACHED]


# ---------------------------------------------------------------- the suite's reach before this audit
def clip_counts(oracle, clip):
    """the classes one encaudit.Clip takes: the oracle through the model, which must agree with it on every frame"""
    oe = clip.encoder(oracle)
    m = rcref.PyRc(clip.w, clip.h, clip.br, clip.skip)
    for t, f in enumerate(clip.frames):
        if t in clip.idr:
            oe.force_idr()
            m.force_idr()
        nal = oe.encode(f)
        coded = m.begin(f)
        assert coded == bool(nal), (clip.name, t)
        if coded:
            m.end(nal, oe.rc_state()['avg_qp'], coded_mbs(oe.mbinfo()))
        if not clip.gom:  # the exact GOM rule moves the QP inside a frame; the frame level is the same
            st = oe.rc_state()
            assert m.state() == st, (clip.name, t, m.state(), st)
    return m.counts


@functools.lru_cache(maxsize=None)
def suite_reach():
    """class -> (count, first input) over the inputs of the GPU encoder-vs-oracle tests that were there before this audit:
    encaudit.suite_clips (tests/test_gpu_encoder.py, test_content_extremes.py, test_gpu_configs.py) and the directed
    clips of §3.8 and §3.9"""
    import encaudit
    import writeaudit
    o = _oracle()
    small, large = encaudit.suite_clips(o)
    out = {}
    for clip in list(small) + list(large) + list(encaudit.directed_clips()) + list(writeaudit.directed_clips()):
        for k, n in clip_counts(o, clip).items():
            c, first = out.get(k, (0, clip.name))
            out[k] = (c + n, first)
    return out


# ---------------------------------------------------------------- the sweep DIRECTED was chosen by
GEOMETRIES = ((16, 16), (48, 48), (176, 144), (50, 34), (18, 18), (32, 16), (512, 48), (496, 48))
TABLE_GEOMETRIES = ((176, 176), (656, 176), (544, 848))  # one flat frame each: the area classes 1..3


def candidates(seed=2024, per_geometry=80):
    rng = np.random.default_rng(seed)
    fixed = ['f' + 's' * 19, 'n' * 20, 'f' + 's' * 6 + 'n' * 6 + 's' * 7, 'n' * 4 + 's' * 10 + 'n' * 6, 'b' + 'd' * 3 + 'b' * 3,
             'l' * 20, 'f' + 's' * 3 + 'l' * 8 + 'n' * 8, 'n' + 's' * 19, 'h' * 20]
    for w, h in GEOMETRIES:
        px = w * h
        rates = sorted({max(int(px * 60 * b), 2000) for b in (0.004, 0.02, 0.08, 0.3, 1.2, 4.0)})
        for k in range(per_geometry):
            if k < 2 * len(fixed):
                sch = fixed[k % len(fixed)]
            else:
                sch, n = '', int(rng.integers(10, 25))
                while len(sch) < n:
                    sch += str(rng.choice(list('fsnlhbd'))) * int(rng.integers(1, 7))
                sch = sch[:n]
                if sch[0] == 's':
                    sch = 'f' + sch[1:]
            idr = sorted(set(int(x) for x in rng.integers(1, len(sch), int(rng.integers(0, 4))))) if k % 3 else []
            yield Seq(w, h, int(rng.choice(rates)), k % 2 == 0, sch, idr, seed=int(rng.integers(1, 1000)))


def sweep():
    o = _oracle()
    need = set(required()) - set(t for s in long_runs().values() for t in s.targets)
    muts = set(rcref.PyRc.MUTATIONS) - {'pframes_unsaturated', 'idrs_unsaturated'}
    pool = []
    for s in candidates():
        run = oracle_run(o, s)
        m, bad = replay(s, run)
        assert bad is None, (s.name, bad)
        caught = {x for x in muts if replay(s, run, x)[1] is not None}
        pool.append((s, set(m.counts), caught))
    chosen = []
    while need or muts:
        best = max(pool, key=lambda p: (len(p[1] & need) * 4 + len(p[2] & muts), -len(p[0]) * p[0].w * p[0].h))
        gain, mg = best[1] & need, best[2] & muts
        if not gain and not mg:
            break
        chosen.append((best[0], gain))
        need -= gain
        muts -= mg
    for s, gain in chosen:
        spec = (s.w, s.h, s.br, s.skip, s.schedule, tuple(sorted(s.idr)), s.seed)
        print(f'    ({spec!r},\n     {" ".join(sorted(gain, key=rcref.RC_CLASSES.index))!r}),')
    print('not reached:', sorted(need), 'mutations not caught:', sorted(muts))


if __name__ == '__main__':
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'openh264-wasm_amd'))
    sweep()
