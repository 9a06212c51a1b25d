"""Content and bookkeeping for the P-macroblock decision reference (tests/mdref.py) -- TEST
INFRASTRUCTURE ONLY.

clips():       encaudit's and fwdaudit's directed clips, coded with one slice, and the slice-edge clips below.
chain():       access units of one stream -> the mdref.Picture of every coded frame (parseref -> reconref -> dbkref carried).
check_all():   the first Mismatch over a chain, or None.
catches():     the first macroblock where a mutated reference disagrees with the bytes.
CLAIMS:        mutation name -> the clip that is there to catch it (and, for the slice-edge kind, its slice count).
"""
import functools

import numpy as np

import dbkref
import encaudit
import fwdaudit
import mdref
import parseref
import reconref


def _slice_frames(kind, w, h, n, seed):
    """content for a picture of at least four MB rows under two slices: the left half moves and the right half is static
    across the slice edge (the row above the edge holds skipped MBs and MBs with vectors), and a flat band with a step in
    it lies over the edge (the I16x16 alternative comes out differently with and without the row above)"""
    mov = encaudit.gen('left', w, h, n, seed, 9 if kind == 'a' else -6, 5 if kind == 'a' else 3)
    out = []
    edge = 16 * (((h + 15) // 16) // 2)   # first_row(1) of two slices (§3.7)
    for t, f in enumerate(mov):
        y = f[:w * h].reshape(h, w).copy()
        x0 = w - 32 if kind == 'a' else w - 16
        band = y[edge - 16:edge + 16, x0:x0 + 16]
        band[:] = 100
        band[:16, :] = 100 + 12 * (t % 3)        # the row above the edge changes from frame to frame,
        band[16:, 8:] = 100 + 12 * ((t + 1) % 3)  # the row below holds a vertical step: V from above predicts it, DC does not
        g = f.copy()
        g[:w * h] = y.ravel()
        out.append(g)
    return out


# (name, content kind, w, h, bitrate, slices, frames, seed) -- the smallest pictures with both kinds of row under two slices
_SLICE_SPECS = [('edge_a', 'a', 48, 80, 200000, 2, 7, 11), ('edge_b', 'b', 48, 80, 200000, 2, 7, 12), ('edge_c', 'a', 80, 64, 200000, 2, 7, 13),
                ('edge_d', 'b', 80, 64, 200000, 2, 7, 14), ('edge_e', 'a', 48, 80, 2000000, 2, 7, 15), ('edge_f', 'b', 80, 64, 2000000, 2, 7, 16)]


@functools.lru_cache(maxsize=None)
def slice_clips():
    out = []
    for name, kind, w, h, br, ns, n, seed in _SLICE_SPECS:
        c = encaudit.Clip(f'{name}_{w}x{h}_{br}', w, h, br, _slice_frames(kind, w, h, n, seed))
        c.nslices = ns
        out.append(c)
    return tuple(out)


def _mb(p, mbx, mby, src):
    """macroblock (mbx, mby) of planes p <- the same macroblock of planes src (or a luma constant with chroma 128)"""
    ys, xs = slice(16 * mby, 16 * mby + 16), slice(16 * mbx, 16 * mbx + 16)
    cy, cx = slice(8 * mby, 8 * mby + 8), slice(8 * mbx, 8 * mbx + 8)
    if np.isscalar(src):
        p[0][ys, xs], p[1][cy, cx], p[2][cy, cx] = src, 128, 128
    else:
        p[0][ys, xs], p[1][cy, cx], p[2][cy, cx] = src[0][ys, xs], src[1][cy, cx], src[2][cy, cx]


def gen_tie(kind, seed, a, k):
    """two frames (IDR + P) built so that an exact tie of the rules occurs at macroblock Y of the P frame. The IDR is flat
    (value 100) wherever Y's search reads it, so every SAD there is the same number and the costs differ by bits alone.
    lastmin    48x32, Y = (1, 1): the left MB moves down half a sample (the one above it stays), the top MB stays (and turns
               12 brighter, so that Intra16x16's V does not predict Y), the right MB column moves down 1.5 samples: mvp
               (0, 2), and the candidates mvp -> (0, 1) and B -> (0, 0) cost SAD + 6 lambda each: the reference under both is
               the same rows (Y's IDR rows are all alike, the row below the picture repeats the last). The two rows above Y
               are k brighter in the IDR, so the half-sample position (0, 2) between the two, which costs 4 lambda less,
               predicts worse than either and the refinement leaves each start point where it is; Y carries noise of
               amplitude a
    cross      48x16, Y = (1, 0): noise whose absolute sum against 100 is exactly k, found again 16 samples to the right in
               the reference: the diamond stays at (0, 0) with SAD k, the cross search -- if it runs -- moves to (16, 0)
    level2     48x16, Y = (1, 0): one 4x4 block k brighter, nothing else: a single DC level in the residual test"""
    rng = np.random.default_rng(seed)
    w, h = (48, 32) if kind == 'lastmin' else (48, 16)
    flat = lambda: [np.full((h, w), 100, np.int64), np.full((h // 2, w // 2), 128, np.int64), np.full((h // 2, w // 2), 128, np.int64)]
    f0, f1 = flat(), flat()
    if kind == 'lastmin':
        tex = lambda seed_, qy: [np.asarray(q, np.int64) for q in encaudit.planes(seed_, w, h, 0, qy, lo=160, hi=220)]
        for mbx, qy in ((0, 2), (2, 6)):         # whole MB columns of texture, moving down by qy quarter samples
            for mby in (0, 1):
                _mb(f0, mbx, mby, tex(seed + mbx, 0))
                _mb(f1, mbx, mby, tex(seed + mbx, 0 if (mbx, mby) == (0, 0) else qy))   # (0, 0) stays: the top MB's mvp is zero
        f0[0][14:16, 16:32] = 100 + k            # the two rows above Y: what the half-sample taps between (0, 0) and (0, 1) read
        f1[0][0:16, 16:32] = f0[0][0:16, 16:32] + 12
        f1[0][16:32, 16:32] += rng.integers(-a, a + 1, (16, 16))
    elif kind == 'cross':
        n = rng.integers(-a, a + 1, (16, 16))
        flatn = n.ravel()
        i = 0
        while np.abs(flatn).sum() != k:      # one sample at a time towards the sum
            flatn[i % 256] += 1 if np.abs(flatn).sum() < k and flatn[i % 256] >= 0 else (-1 if np.abs(flatn).sum() < k else -np.sign(flatn[i % 256]))
            i += 1
        f0[0][:, 32:48] = 100 + n
        f1[0][:, 32:48] = 100 + n
        f1[0][:, 16:32] = 100 + n
    elif kind == 'level2':
        f1[0][4:8, 20:24] += k
    else:
        raise ValueError(kind)
    return [encaudit.pack([np.clip(q, 0, 255) for q in f]) for f in (f0, f1)]


def tie_clip(kind, seed, a, k, br, targets=()):
    c = encaudit.Clip(f'tie_{kind}_s{seed}_a{a}_k{k}_{br}', 48, 32 if kind == 'lastmin' else 16, br, gen_tie(kind, seed, a, k), targets=targets)
    return c


# found by a seeded sweep of 280 clips of encaudit.gen for the mutations no other clip catches
_EXTRA = [(('bottom', 48, 48, 6, 20, 47, -62, 100000, 'off', {'cell': 16, 'blur': 8}), ('diamond cap 31', 'diamond cap 33')),
          (('noisy', 16, 48, 6, 8, 24, -16, 300000, 'off', {'amp': 2}), ('row +1 at >= 1.25x',))]


# directed ties (gen_tie) and a two-row picture whose second row is skipped, so that the first row's bits are exactly twice
# the integer mean whenever they are even; parameters from a sweep over k, seed and bitrate
_TIES = [(('cross', 1, 8, 1022, 300000), ('cross search at >= 1024',)), (('level2', 1, 0, 4, 300000), ('level limit 2',)),
         (('lastmin', 1, 4, 60, 300000), ('last minimum candidate instead of the first',))]
_EXTRA.append((('top', 16, 32, 6, 5, 10, 3, 30000, 'off', {}), ('row +2 at >= 2x',)))


@functools.lru_cache(maxsize=None)
def extra_clips():
    return tuple(encaudit.spec_clip(spec, targets) for spec, targets in _EXTRA) + tuple(tie_clip(*spec, targets=t) for spec, t in _TIES)


@functools.lru_cache(maxsize=None)
def clips():
    """every directed clip once (fwdaudit's repeat none of encaudit's names)"""
    seen, out = set(), []
    for c in encaudit.directed_clips() + fwdaudit.directed_clips() + extra_clips() + slice_clips():
        if c.name not in seen:
            seen.add(c.name)
            out.append(c)
    return tuple(out)


def stream_of(clip, nslices=1):
    return mdref.Stream(clip.w, clip.h, clip.br, skip=clip.skip, gom=clip.gom, nslices=nslices)


def step(stream, clip, t, unit, label):
    """one frame step of a chain: `unit` is the access unit the encoder gave for frame t (empty: skipped).
    -> (mdref.Picture, parsed, res, deblocked planes) or None for a skipped frame"""
    if stream.pstate is None:
        stream.pstate = parseref.State()
    if t in clip.idr:
        stream.force_idr()
    coded = stream.rc.begin(clip.frames[t])
    assert coded == bool(unit), f'{label}: the frame-level model {"codes" if coded else "skips"} frame {t}, the encoder does not'
    if not unit:
        return None
    parsed = parseref.parse(unit, stream.pstate)
    res = reconref.reconstruct(parsed.syntax, parsed.geometry, stream.ref)
    planes = dbkref.deblock(res.planes, res.records).planes
    pic = mdref.picture(stream, clip.frames[t], parsed, res, label)
    mdref.advance(stream, pic, planes, unit, stream.rc.cur_idr)
    return pic, parsed, res, planes


def chain(clip, units, nslices=1, label=None):
    stream = stream_of(clip, nslices)
    out = []
    for t, u in enumerate(units):
        r = step(stream, clip, t, u, f'{label or clip.name}, frame {t}')
        if r is not None:
            out.append(r[0])
    return out


def oracle_units(oracle, clip):
    oe = clip.encoder(oracle)
    out = []
    for t, f in enumerate(clip.frames):
        if t in clip.idr:
            oe.force_idr()
        out.append(oe.encode(f))
    return out


def check_all(pictures, rules=None, counts=None):
    for p in pictures:
        mm = mdref.check(p, rules, counts)
        if mm is not None:
            return mm
    return None


def catches(pictures, rules):
    """the first macroblock where the mutated reference disagrees with the bytes, or None"""
    for p in pictures:
        p.i16_cache.clear()
    try:
        return check_all(pictures, rules)
    finally:
        for p in pictures:
            p.i16_cache.clear()


# mutation name -> (clip name, slices): the clip that is there to catch it, on the oracle's bytes (and the GPU's, equal to
# them) with one slice, on the GPU's bytes alone with more. From the sweeps recorded in DESIGN.md §3.12.
CLAIMS = {
    'candidate A dropped': ('cells_80x48_6f_s712_a4_6000', 1),
    'candidate B dropped': ('noise_18x18_8f_s819_a20_20000000_idr4', 1),
    'candidate C dropped': ('cells_80x48_6f_s712_a4_6000', 1),
    'C not replaced by the top-left MB': ('cells_80x48_6f_s712_a4_6000', 1),
    'candidates truncated (>> 2), not rounded': ('stripes_48x16_8f_s474_a12_60000_idr2_5', 1),
    'candidates not clipped to +-16': ('ramp_48x48_s1_d0_0_30000_off', 1),
    'diamond points in another order': ('noise_18x18_8f_s819_a20_20000000_idr4', 1),
    'diamond cap 31': ('bottom_48x48_s20_d47_-62_100000_off_blur8_cell16', 1),
    'diamond cap 33': ('bottom_48x48_s20_d47_-62_100000_off_blur8_cell16', 1),
    'diamond moves without strict improvement': ('ramp_48x48_s1_d0_0_30000_off', 1),
    'last minimum candidate instead of the first': ('tie_lastmin_s1_a4_k60_300000', 1),
    'cross search at >= 1024': ('tie_cross_s1_a8_k1022_300000', 1),
    'level limit 2': ('tie_level2_s1_a0_k4_300000', 1),
    'row +2 at >= 2x': ('top_16x32_s5_d10_3_30000_off', 1),
    'cross search above 512': ('noise_80x48_6f_s644_a6_60000', 1),
    'cross search above 2048': ('bottom_16x48_s5_d51_0_30000_off_blur8_cell16', 1),
    'vertical line before horizontal': ('cells_50x34_8f_s1032_a4_6000_idr2_5', 1),
    'cross lines through the start point': ('slide_16x16_s3_d-50_0_30000_off', 1),
    'mvd bits against zero': ('stripes_48x16_8f_s465_a2_200000_idr4', 1),
    'lambda of QP + 1': ('stripes_48x16_8f_s465_a2_200000_idr4', 1),
    'sub-pel neighbours in raster order': ('stripes_48x16_8f_s465_a2_200000_idr4', 1),
    'quarter step around the integer point': ('slide_16x16_s3_d-50_0_30000_off', 1),
    'SAD instead of SATD': ('slide_16x16_s3_d-50_0_30000_off', 1),
    'SATD without lambda x bits': ('stripes_48x16_8f_s465_a2_200000_idr4', 1),
    'top-left neighbour ignored for the try': ('noise_50x34_8f_s964_a6_60000', 1),
    'co-located MB ignored': ('slide_48x16_s6_d0_0_30000_off', 1),
    'T without chroma': ('slide_16x16_s4_d0_0_30000_off', 1),
    'median where a single skipped neighbour\'s SAD is due': ('noise_50x34_8f_s964_a6_60000', 1),
    'luma cost limit 4': ('shift_48x48_8f_s614_a3_60000', 1),
    'luma cost limit 6': ('low_48x48_8f_s539_a2_20000000', 1),
    'chroma cost limit 5': ('top_16x48_s3_d1_0_30000_off', 1),
    'chroma cost limit 7': ('bottom_176x144_s4_d50_0_1000000_gom', 1),
    'keep without the top-right MB': ('noise_80x48_6f_s644_a6_60000', 1),
    'intra compared against the sub-pel cost': ('slide_16x16_s3_d-50_0_30000_off', 1),
    'intra compared with <=': ('noise_80x48_6f_s644_a6_60000', 1),
    'double check off': ('flat_16x16_s1_d0_0_30000_off', 1),
    'row mean over rows with bits only': ('bottom_16x48_s5_d51_0_30000_off_blur8_cell16', 1),
    'row +1 at >= 1.25x': ('noisy_16x48_s8_d24_-16_300000_off_amp2', 1),
    'row -1 at <= 0.5x': ('ramp_48x48_s1_d0_0_30000_off', 1),
    'row QP not clipped to the window': ('stripes_16x48_8f_s301_a2_2000', 1),
    'slice edge: MV predictor reads the row above': ('right_80x48_s4_d2_-67_30000_off', 3),
    'slice edge: start candidates read the row above': ('right_80x48_s4_d2_-67_30000_off', 3),
    'slice edge: judge tried by the row above': ('edge_c_80x64_200000', 2),
    'slice edge: keep satisfied by the row above': ('noise_80x48_6f_s644_a6_60000', 3),
    'slice edge: predicted SAD counts the row above': ('edge_b_48x80_200000', 2),
    'slice edge: I16x16 uses the row above': ('edge_a_48x80_200000', 2),
}
