"""Decision-branch audit of the encoder -- TEST INFRASTRUCTURE ONLY.

The oracle encoder counts, per named class, every outcome of its forward decisions (oracle/h264o_enc.c
BRANCH_CLASSES) and keeps per macroblock the classes it took. This module holds what the CPU audit
(tests/test_enc_branch_audit.py) and the GPU tests (tests/test_gpu_enc_branches.py) share:

  - Clip: one encoder input (geometry, bitrate, frames, rate-control switches, forced IDRs);
  - suite_clips(): the inputs the GPU encoder-vs-oracle tests already feed;
  - directed_clips(): seeded content built to reach the classes those inputs miss, each with the classes it is there for;
  - EXCLUDED / NOT_REACHED: the classes no content is asked to reach, with the reason;
  - run_clip(): the oracle over one clip;
  - explain_mismatch(): the macroblock-level message of a GPU / oracle disagreement.
"""
import functools

import numpy as np

MB_TYPES = {0: 'I4x4', 1: 'I16x16', 2: 'P16x16', 3: 'P_Skip'}


class Clip:
    def __init__(self, name, w, h, br, frames, skip=False, gom=False, idr=(), targets=()):
        self.name, self.w, self.h, self.br, self.frames = name, w, h, br, frames
        self.skip, self.gom, self.idr, self.targets = skip, gom, frozenset(idr), tuple(targets)
        fs = w * h * 3 // 2
        assert all(f.dtype == np.uint8 and f.size == fs for f in frames), name

    def encoder(self, oracle):
        oe = oracle.encoder(self.w, self.h, self.br)
        oe.set_frame_skip(self.skip)
        oe.set_gom_exact(self.gom)
        return oe


def run_clip(oracle, clip, decode=False):
    """the oracle over one clip -> (per-class counts, per frame (nal, rc_state, recon or None));
    decode: the oracle decoder must reproduce the encoder's reconstruction on every coded frame"""
    oe = clip.encoder(oracle)
    od = oracle.decoder() if decode else None
    out = []
    for t, f in enumerate(clip.frames):
        if t in clip.idr:
            oe.force_idr()
        nal = oe.encode(f)
        rec = oe.recon() if nal else None
        if decode and nal:
            rc, pic, dw, dh = od.decode(nal)
            assert rc == 1 and (dw, dh) == (clip.w, clip.h), (clip.name, t, rc)
            assert np.array_equal(pic, rec), f'{clip.name}: oracle decoder != encoder reconstruction at frame {t}'
        out.append((nal, oe.rc_state(), rec))
    return oe.branch_counts(), out


# ---------------------------------------------------------------- the suite's inputs
def _synth(sid, w, h, n):
    from h264mi.synth import SyntheticStream
    g = SyntheticStream(sid, w, h)
    return [np.ascontiguousarray(g.frame(t)) for t in range(n)]


def suite_clips(oracle):
    """What tests/test_gpu_encoder.py, tests/test_content_extremes.py and tests/test_gpu_configs.py -- the GPU tests
    that hold encoder bytes to the oracle's -- feed: same content, geometry, bitrate, frame count and switches.
    Streams of one batch are separate clips. -> (small, large): large are the 720p / 1080p ones."""
    from golden.make_golden import CASES, case_inputs
    from test_content_extremes import CASES as EXTREMES, content_frames, W, H
    small, large = [], []
    for name, w, h, br, n, every, kind in CASES:
        idr = [t for t in range(1, n) if every and t % every == 0]
        (large if w >= 1280 else small).append(Clip(f'fixture_{name}', w, h, br, case_inputs(oracle, w, h, n, kind)[0], skip=True, idr=idr))
    for name, br, kind in EXTREMES:
        small.append(Clip(f'extreme_{name}', W, H, br, content_frames(kind), skip=True))
    for w, h in [(16, 16), (48, 16), (16, 48), (32, 32), (80, 48), (176, 144)]:  # test_intra_decision_geometries_vs_oracle
        rng = np.random.default_rng(w * 131 + h)
        fs = w * h * 3 // 2
        tex = _synth(9, w, h, 4)
        a, b = [], []
        for t in range(4):
            flat = np.full(fs, 90 + 7 * t, np.uint8)
            b.append(rng.integers(0, 256, fs, dtype=np.uint8))
            a.append(flat if t == 0 else tex[t])
        for br in (300000, 4000000):
            small.append(Clip(f'intra_geo_{w}x{h}_{br}_tex', w, h, br, a, idr=range(4)))
            small.append(Clip(f'intra_geo_{w}x{h}_{br}_noise', w, h, br, b, idr=range(4)))
    small.append(Clip('gom_cif_narrow', 352, 288, 500000, _synth(5, 352, 288, 6), gom=True))  # stream 0 of 4
    for s in range(1, 4):
        small.append(Clip(f'gom_cif_narrow_s{s}', 352, 288, 500000, _synth(5 + s, 352, 288, 6), gom=True))
    s0_60 = _synth(0, 1920, 1080, 60)
    large.append(Clip('1080p_20m_3f', 1920, 1080, 20000000, s0_60[:3], skip=True))
    large.append(Clip('1080p_8m_60f', 1920, 1080, 8000000, s0_60, skip=True))
    large.append(Clip('1080p_1m_60f', 1920, 1080, 1000000, s0_60, skip=True))
    large.append(Clip('1080p_rc_state_s0', 1920, 1080, 8000000, s0_60[:14], skip=True, idr=[9]))
    large.append(Clip('1080p_rc_state_s1', 1920, 1080, 8000000, _synth(1, 1920, 1080, 14), skip=True, idr=[9]))
    large.append(Clip('1080p_1m_skip_off', 1920, 1080, 1000000, s0_60[:6]))
    for br in (1000000, 8000000):
        large.append(Clip(f'720p_ionly_{br}', 1280, 720, br, _synth(0, 1280, 720, 30), skip=True, idr=range(30)))
    for s in range(16):  # test_p_slice_decisions_16_streams_vs_oracle (stream 0 is 1080p_1m_skip_off's first frames)
        if s:
            large.append(Clip(f'1080p_16streams_s{s}', 1920, 1080, 1000000, _synth(s, 1920, 1080, 3)))
    for s in range(2):  # test_exact_gom_rc_vs_oracle
        large.append(Clip(f'gom_1080p_8m_s{s}', 1920, 1080, 8000000, _synth(5 + s, 1920, 1080, 6), gom=True))
        large.append(Clip(f'gom_1080p_20m_skip_s{s}', 1920, 1080, 20000000, _synth(5 + s, 1920, 1080, 5), skip=True, gom=True))
        large.append(Clip(f'gom_720p_s{s}', 1280, 720, 2000000, _synth(5 + s, 1280, 720, 5), gom=True))
    return small, large


# ---------------------------------------------------------------- directed content
def _blur(a, k):
    """separable box blur of width k (edge samples repeated)"""
    if k <= 1:
        return a
    for ax in (0, 1):
        p = np.concatenate([np.repeat(a.take([0], ax), k // 2, ax), a, np.repeat(a.take([-1], ax), k - 1 - k // 2, ax)], ax)
        c = np.cumsum(np.concatenate([np.zeros_like(p.take([0], ax)), p], ax), ax)
        a = (c.take(range(k, p.shape[ax] + 1), ax) - c.take(range(0, p.shape[ax] + 1 - k), ax)) / k
    return a


MARGIN = 144  # samples of world around the picture: 8 frames of 17 samples per frame, and the blur


@functools.lru_cache(maxsize=None)
def _world(seed, w, h, scale, cell, lo, hi, blur):
    """a seeded texture at `scale` samples per picture sample: random cells of `cell` picture samples in lo..hi,
    box-blurred over `blur` picture samples"""
    rng = np.random.default_rng(seed)
    W, H = w + 2 * MARGIN, h + 2 * MARGIN
    base = rng.integers(lo, hi + 1, ((H + cell - 1) // cell, (W + cell - 1) // cell)).astype(np.float64)
    a = np.kron(base, np.ones((cell * scale, cell * scale)))[:H * scale, :W * scale]
    return _blur(a, blur * scale)


def _sample(world, scale, w, h, ox, oy):
    """the w x h picture whose sample (0, 0) lies ox, oy world samples right of / below the world's centre position"""
    x0, y0 = MARGIN * scale + ox, MARGIN * scale + oy
    blk = world[y0:y0 + h * scale, x0:x0 + w * scale]
    assert blk.shape == (h * scale, w * scale), (ox, oy)
    return np.clip(np.floor(blk.reshape(h, scale, w, scale).mean((1, 3)) + 0.5), 0, 255).astype(np.uint8)


def planes(seed, w, h, qx, qy, cell=4, lo=40, hi=215, blur=3):
    """(Y, U, V) of a textured world seen through a w x h window displaced by (qx, qy) quarter luma samples: luma
    sampled from a world at 4 samples per luma sample, chroma from worlds at 8 per chroma sample, so a vector of
    (qx, qy) quarter samples predicts the window exactly up to the sampling's rounding"""
    y = _sample(_world(seed, w, h, 4, cell, lo, hi, blur), 4, w, h, qx, qy)
    u = _sample(_world(seed + 1, w // 2, h // 2, 8, max(cell // 2, 1), 96, 160, max(blur // 2, 1)), 8, w // 2, h // 2, qx, qy)
    v = _sample(_world(seed + 2, w // 2, h // 2, 8, max(cell // 2, 1), 96, 160, max(blur // 2, 1)), 8, w // 2, h // 2, qx, qy)
    return y, u, v


def pack(p):
    return np.ascontiguousarray(np.concatenate([a.ravel() for a in p]).astype(np.uint8))


def paste(dst, src, x0, y0, x1, y1):
    """the luma rectangle [x0, x1) x [y0, y1) (even bounds) and its chroma of src over dst"""
    out = [a.copy() for a in dst]
    out[0][y0:y1, x0:x1] = src[0][y0:y1, x0:x1]
    for k in (1, 2):
        out[k][y0 // 2:y1 // 2, x0 // 2:x1 // 2] = src[k][y0 // 2:y1 // 2, x0 // 2:x1 // 2]
    return out


def gen(kind, w, h, n, seed, dx, dy, **kw):
    """n frames of directed content. dx, dy: displacement per frame in quarter luma samples.
    slide    the whole picture moves
    left / right / top / bottom   that half moves over a static picture (the judge's triggers, keep, row costs)
    block    a 32x32 block at the picture's centre moves, the rest is static
    noisy    static picture, every frame with fresh noise of amplitude `amp` (the residual test's criteria)
    chroma   static luma, chroma planes offset by `amp` x the frame number (chroma DC)
    flat     flat picture, the left part static, the right part 3 brighter every frame (VAA gate below, SAD 0)
    ramp     a diagonal luma ramp that moves 40 samples: the diamond walks to its cap
    """
    amp = kw.pop('amp', 0)
    rng = np.random.default_rng(seed + 77)
    out = []
    still = planes(seed, w, h, 0, 0, **kw)
    for t in range(n):
        mov = planes(seed, w, h, dx * t, dy * t, **kw)
        if kind == 'slide':
            p = mov
        elif kind in ('left', 'right', 'top', 'bottom'):
            hw, hh = (w // 32) * 16 or 16, (h // 32) * 16 or 16
            box = {'left': (0, 0, hw, h), 'right': (hw, 0, w, h), 'top': (0, 0, w, hh), 'bottom': (0, hh, w, h)}[kind]
            p = paste(still, mov, *box)
        elif kind == 'block':
            x0, y0 = max((w // 2 - 16) & ~15, 0), max((h // 2 - 16) & ~15, 0)
            p = paste(still, mov, x0, y0, min(x0 + 32, w), min(y0 + 32, h))
        elif kind == 'noisy':
            p = [np.clip(a.astype(np.int32) + (rng.integers(-amp, amp + 1, a.shape) if t else 0), 0, 255) for a in still]
        elif kind == 'chroma':
            p = [still[0], np.clip(still[1].astype(np.int32) + amp * t, 0, 255), np.clip(still[2].astype(np.int32) - amp * t, 0, 255)]
        elif kind == 'flat':
            y = np.full((h, w), 120)
            y[:, (w // 32) * 16 or 16:] = 60 + 3 * t  # w == 16: the whole picture stays flat and static
            p = [y, np.full((h // 2, w // 2), 128), np.full((h // 2, w // 2), 128)]
        elif kind == 'ramp':
            yy, xx = np.mgrid[0:h, 0:w]
            p = [np.clip(xx + yy + (40 if t % 2 else 0), 0, 255), np.full((h // 2, w // 2), 128), np.full((h // 2, w // 2), 128)]
        else:
            raise ValueError(kind)
        out.append(pack(p))
    return out


def spec_clip(spec, targets=()):
    """a Clip from its committed parameters: (kind, w, h, frames, seed, dx, dy, bitrate, rate-control mode, content keywords)"""
    kind, w, h, n, seed, dx, dy, br, mode, kw = spec
    name = f'{kind}_{w}x{h}_s{seed}_d{dx}_{dy}_{br}_{mode}' + ''.join(f'_{k}{v}' for k, v in sorted(kw.items()))
    return Clip(name, w, h, br, gen(kind, w, h, n, seed, dx, dy, **kw), skip=(mode == 'skip'), gom=(mode == 'gom'), targets=targets)


# ---------------------------------------------------------------- the mismatch message
def gpu_mbinfo(enc, s):
    """stream s's h264mi_enc_mbinfo as int32 [MBs, 6]: type, QP, cbp, first vector, TotalCoeff sum (128 bytes per MB,
    h264mi_types.h MbInfo)"""
    nmb = ((enc.w + 15) // 16) * ((enc.h + 15) // 16)
    raw = np.zeros(nmb * 128, np.uint8)
    assert enc._L.h264mi_enc_mbinfo(enc._e, s, raw.ctypes.data) == 0
    raw = raw.reshape(nmb, 128)
    mv = raw[:, 60:64].copy().view(np.int16).astype(np.int32)  # mv[0]: after type..pad1 (8), i4mode (16), ref (4), nnz (24), mvd (4), sub (4)
    out = np.concatenate([raw[:, 0:3].astype(np.int32), mv, raw[:, 28:52].astype(np.int32).sum(axis=1, keepdims=True)], axis=1)
    # the record as the kernel leaves it: an intra MB's vector and a skipped MB's cbp are not part of it, and bit 7 of
    # the QP byte marks an MB before its row's first mb_qp_delta, whose QPY is the QP the row was entered with
    # (7.4.5): the QP of the last MB before it without the mark, -1 (not compared) when there is none
    out[out[:, 0] < 2, 3:5] = 0
    out[out[:, 0] == 3, 2] = 0
    running = -1
    for r in out:
        if r[1] & 0x80:
            r[1] = running
        else:
            running = r[1]
    return out


def _fmt(r):
    return f'{MB_TYPES.get(int(r[0]), int(r[0]))} QP {int(r[1])} cbp {int(r[2])} mv ({int(r[3])}, {int(r[4])}) coefficients {int(r[5])}'


def records_differ(got_info, ref_info):
    """indices of the macroblocks whose {type, QP, cbp, first vector, TotalCoeff sum} differ; records of 6 columns in
    that order or the oracle's 8 (the sum last); a GPU QP of -1 is not compared"""
    g, r = (np.asarray(a)[:, [0, 1, 2, 3, 4, a.shape[1] - 1]] for a in (got_info, ref_info))
    ne = g != r
    ne[:, 1] &= g[:, 1] != -1
    return np.flatnonzero(ne.any(axis=1)), g, r


def explain_mismatch(label, names, mbw, got_info, ref_info, ref_branches, got_len=None, ref_len=None):
    """The message of a GPU / oracle disagreement: the first macroblock whose {type, QP, cbp, first vector, TotalCoeff
    sum} differ, both sides' values and the classes the oracle recorded for it. Records: [MBs, 6] in that order, or the
    oracle's [MBs, 8] (h264o_enc_mbinfo / h264o_dec_mbinfo). got_info may be None (no record could be read)."""
    head = f'{label}: GPU != oracle'
    if got_len is not None:
        head += f' ({got_len} B vs {ref_len} B)'
    if got_info is None:
        return head + '; no macroblock record of the GPU side could be read'
    if len(got_info) != len(ref_info):
        return head + f'; {len(got_info)} GPU macroblock records vs {len(ref_info)} oracle records'
    bad, g, r = records_differ(got_info, ref_info)
    if bad.size == 0:
        return head + '; every macroblock agrees in type, QP, cbp, first vector and coefficient count: the difference is in level values, intra modes or the packing'
    m = int(bad[0])
    cls = ', '.join(names[c] for c in ref_branches[m]) or 'none'
    return (f'{head}; first differing macroblock {m} (x {m % mbw}, y {m // mbw}) of {bad.size}: GPU {_fmt(g[m])} | oracle {_fmt(r[m])} | '
            f'oracle classes: {cls}')


class Explainer:
    """Keeps what the message needs beside an oracle encoder. For a batch encoder `gpu` is a callable returning its
    macroblock records; the C-ABI encoder exposes none, so there the GPU side's records are parsed from its bytes by an
    oracle decoder that has followed the (identical) frames before."""

    def __init__(self, oracle, oe, label, gpu=None):
        self.oracle, self.oe, self.label, self.gpu = oracle, oe, label, gpu
        self.names = oracle.branch_names()
        self.od = None if gpu else oracle.decoder()

    def check(self, t, got, ref):
        """assert got == ref with the macroblock-level message; call once per frame, in order"""
        if got == ref:
            if self.od is not None and ref:
                self.od.decode(ref)
            return
        raise AssertionError(self.message(t, got, ref))

    def message(self, t, got, ref):
        label = f'{self.label} frame {t}'
        if not ref or not got:
            return f'{label}: GPU {len(got)} B vs oracle {len(ref)} B: one side skipped or failed the frame'
        mbw = (self.oe.w + 15) // 16
        if self.gpu is not None:
            gi = self.gpu()
        else:
            rc, _, _, _ = self.od.decode(got)
            gi = None
            if rc == 1:
                gi = np.zeros(self.oe.mbinfo().size, np.int32)
                self.oracle.L.h264o_dec_mbinfo(self.od.d, gi.ctypes.data)
                gi = gi.reshape(-1, 8)
        return explain_mismatch(label, self.names, mbw, gi, self.oe.mbinfo(), self.oe.mb_branches(), len(got), len(ref))


# ---------------------------------------------------------------- classes and content
# Classes no content can reach, each with its derivation. The audit fails if any content ever reaches one.
_MV_BOUND = ('the judge refuses a skip vector with (mv >> 2) + 16 * MB position below -29 or above (16 * MBs) | 12. The skip '
             'vector is zero or a median of neighbours\' vectors, and every vector the search writes is 4 * integer + half step + '
             'quarter step with the integer inside -16..16: -67..67 quarter samples, so mv >> 2 lies in -17..16. With the MB position '
             'in 0..MBs - 1 the sum lies in -17..16 * MBs: never below -29, never above 16 * MBs <= (16 * MBs) | 12.')
EXCLUDED = {'J_MV_BELOW_XMIN': _MV_BOUND, 'J_MV_ABOVE_XMAX': _MV_BOUND, 'J_MV_BELOW_YMIN': _MV_BOUND, 'J_MV_ABOVE_YMAX': _MV_BOUND}

# Classes neither reached nor excluded, with the content that was tried (at most three; none of the judge, intra, sub-pel
# or residual families). Empty: the directed clips reach every class that is not excluded.
NOT_REACHED = {}

# (kind, w, h, frames, seed, dx, dy, bitrate, rate-control mode, content keywords) and the classes the clip is in the set
# for: those it is the first of this list to reach. Clips without classes of their own widen a batch: a second bitrate,
# a third stream. Together the clips reach every class that is not excluded, so the GPU tests see each one at a
# geometry of at most 176x144.
DIRECTED = [
    (('slide', 16, 16, 6, 4, 0, 0, 30000, 'off', {}),
     'J_TRY_COLOC J_NOT_TRIED J_NOT_TAKEN J_REJ_LUMA_CTR J_DOUBLE_CHECK IA_AFTER_SEARCH_LOST II_VAA_ABOVE II_I4 S_START_MVP S_DIA_0 S_CROSS_OFF SP_HALF_NONE SP_QUARTER_NONE R_QUANT_INTER R_QUANT_INTRA R_CHROMA_DC_INTER R_CHROMA_DC_INTRA R_P_Y0_SET R_P_Y1_SET R_P_Y2_SET R_P_Y3_SET R_P_Y0_CLEAR R_P_Y1_CLEAR R_P_Y2_CLEAR R_P_Y3_CLEAR R_I4_Y0_SET R_I4_Y1_SET R_I4_Y2_SET R_I4_Y3_SET R_CBPC_0_INTER R_CBPC_2_INTER R_CBPC_2_INTRA Q_ROW_ZERO Q_ROW_FIRST_MB_CARRIES Q_ROW_NO_CARRIER G_JUDGE_MBW1 G_JUDGE_MBH1 G_JUDGE_COL_FIRST G_JUDGE_COL_LAST G_JUDGE_ROW_FIRST G_DOUBLE_MBW1 G_DOUBLE_MBH1 G_DOUBLE_COL_FIRST G_DOUBLE_COL_LAST G_DOUBLE_ROW_FIRST G_SEARCH_MBW1 G_SEARCH_MBH1 G_SEARCH_COL_FIRST G_SEARCH_COL_LAST G_SEARCH_ROW_FIRST G_CODED_MBW1 G_CODED_MBH1 G_CODED_COL_FIRST G_CODED_COL_LAST G_CODED_ROW_FIRST'),
    (('slide', 16, 16, 6, 3, -50, 0, 30000, 'off', {}),
     'IA_AFTER_SEARCH_WON IP_VAA_ABOVE IP_I4 S_DIA_2_7 S_DIA_8_31 S_CROSS_STAYED S_CROSS_MOVED_H S_REF_OUT_LEFT S_REF_OUT_RIGHT S_REF_OUT_TOP S_REF_OUT_BOTTOM SP_HALF_DOWN SP_HALF_RIGHT SP_HALF_UP_LEFT SP_HALF_UP_RIGHT SP_QUARTER_UP SP_QUARTER_UP_LEFT SP_QUARTER_DOWN_RIGHT G_INTRA_MBW1 G_INTRA_MBH1 G_INTRA_COL_FIRST G_INTRA_COL_LAST G_INTRA_ROW_FIRST G_SUBPEL_MBW1 G_SUBPEL_MBH1 G_SUBPEL_COL_FIRST G_SUBPEL_COL_LAST G_SUBPEL_ROW_FIRST'),
    (('flat', 16, 16, 6, 1, 0, 0, 30000, 'off', {}),
     'J_TAKE_SAD_ZERO J_NOKEEP_PICTURE_EDGE IA_AFTER_SKIP_LOST II_VAA_BELOW II_I16 R_I16_LUMA_DC R_I16_AC_CLEAR R_CBPC_0_INTRA G_SKIP_MBW1 G_SKIP_MBH1 G_SKIP_COL_FIRST G_SKIP_COL_LAST G_SKIP_ROW_FIRST'),
    (('top', 16, 48, 6, 3, 1, 0, 30000, 'off', {}),
     'J_TRY_TOP J_TAKE_RESIDUAL SP_QUARTER_LEFT SP_QUARTER_RIGHT Q_ROW_PLUS2 Q_ROW_PLUS1 Q_ROW_MINUS1 Q_ROW_CLIP_MIN'),
    (('bottom', 16, 48, 6, 5, 51, 0, 30000, 'off', {'cell': 16, 'blur': 8}),
     'J_REJ_LUMA_LEVEL S_START_ZERO S_DIA_1 S_DIA_EDGE_YMIN S_CROSS_MOVED_V S_FINAL_YMIN SP_HALF_UP SP_HALF_LEFT SP_QUARTER_DOWN_LEFT R_I4_Y3_CLEAR'),
    (('slide', 48, 16, 6, 6, 0, 0, 30000, 'off', {}),
     'J_TRY_LEFT J_TAKE_BELOW_PRED_SAD R_CBPC_1_INTER'),
    (('left', 48, 16, 6, 3, 50, 0, 30000, 'off', {}),
     ''),
    (('ramp', 48, 48, 6, 1, 0, 0, 30000, 'off', {}),
     'II_I4_EARLY_STOP II_I4_LOST_OVERHEAD IP_I4_EARLY_STOP IP_I16 S_CAND_CLIPPED S_DIA_CAP S_DIA_EDGE_XMIN S_DIA_EDGE_XMAX S_DIA_EDGE_YMAX S_FINAL_XMIN S_FINAL_XMAX S_FINAL_YMAX SP_HALF_DOWN_RIGHT R_I4_Y0_CLEAR R_I4_Y1_CLEAR R_I4_Y2_CLEAR R_P16_CBP_ZERO_KEPT Q_ROW_LATER_MB_CARRIES'),
    (('slide', 48, 48, 6, 5, 50, 0, 30000, 'off', {'cell': 16, 'blur': 8}),
     'J_NOKEEP_LEFT IA_AFTER_SKIP_WON IP_I4_LOST_OVERHEAD S_START_B SP_HALF_DOWN_LEFT SP_QUARTER_DOWN R_I16_AC_SET R_CBPC_1_INTRA'),
    (('flat', 48, 48, 6, 1, 0, 0, 30000, 'off', {}),
     'J_TRY_TOPLEFT J_TRY_TOPRIGHT J_KEEP IP_VAA_BELOW'),
    (('right', 80, 48, 6, 4, 2, -67, 30000, 'off', {}),
     'J_NOKEEP_TOP J_NOKEEP_TOPRIGHT S_START_A S_START_C S_START_C_TOPLEFT SP_QUARTER_UP_RIGHT Q_ROW_CLIP_MAX'),
    (('flat', 80, 48, 6, 1, 0, 0, 30000, 'off', {}),
     ''),
    (('right', 80, 48, 6, 4, 2, -67, 3000000, 'off', {}),
     'J_TAKE_BELOW_COLOC_SAD'),
    (('noisy', 80, 48, 6, 3, 0, 0, 3000000, 'off', {'amp': 3}),
     ''),
    (('bottom', 176, 144, 8, 4, 50, 0, 1000000, 'gom', {}),
     'J_REJ_CHROMA_DC J_REJ_CHROMA_LEVEL J_REJ_CHROMA_CTR Q_GOM_PLUS2 Q_GOM_PLUS1 Q_GOM_ZERO Q_GOM_MINUS1 Q_GOM_CLIP_MAX Q_GOM_CLIP_MIN'),
    (('noisy', 176, 144, 8, 4, 0, 0, 1000000, 'gom', {'amp': 8}),
     ''),
]


@functools.lru_cache(maxsize=None)
def directed_clips():
    return tuple(spec_clip(spec, tuple(t.split())) for spec, t in DIRECTED)
