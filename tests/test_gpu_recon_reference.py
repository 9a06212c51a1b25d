"""GPU: reconstruction -- intra prediction, motion vector prediction, the six-tap / eighth-sample interpolation, scaling
and transform, the QP chain (csrc/dec_recon.inc; the encoder's enc_mb_kernel.inc and enc_planes.inc) -- against the
independent reference of clauses 8.3-8.5, tests/reconref.py, with tests/dbkref.py (8.7) behind it: the expected
pictures are derived from syntax elements alone (the chain check of tests/test_recon_reference.py), no sample of
them passes through the oracle's reconstruction, which is a sibling of the kernels. Every comparison is byte
equality; a failure names the first differing sample with reconref's explain (macroblock, type, partition, vector
and fractional position or intra mode, branch classes), or dbkref's when the picture before the filter agrees.

Decoder: every directed stream of test_recon_reference.RECON_DIRECTED, the p_frame long-vector streams at 48x48 and
176x144 (vectors beyond +-16 and +-32 samples, reference blocks wholly outside the picture) and one multi-slice
layout through the C-ABI; through BatchDecoder two P pictures per call at 1 and 4 slice waves, and two streams of
different content in one batch.

Encoder: BatchEncoder's reference planes after every frame == the chain over the oracle's *parse* of the GPU's own
NAL bytes. The inputs are test_recon_reference.subsample_frames: SyntheticStream 0, 1 and 3 through a window that moves
by quarter samples, because on SyntheticStream's whole-sample motion the encoder never ends on a half-sample position.
The oracle encoder's streams of the same inputs are the CPU streams `oracle_enc_subsample_<size>_s<id>` (family
`encoder` of the audit table in DESIGN.md; one slice, where the GPU encoder's bytes equal the oracle encoder's). They
hold, at every size, all seven luma positions with a half-sample component -- b, h, j and the averages f, i, k, q that
read j -- beside quarter positions, only 16x16 partitions, all four Intra_16x16 modes over the sizes, all nine
Intra_4x4 modes and chroma DC / H / V / plane; no 16x8 / 8x16 / sub-8x8 partition, no I_PCM, no vector beyond +-16
samples and no mb_qp_delta wrap: the encoder does not emit those. The test asserts the half-sample positions of
ENC_REQUIRED per stream at the end."""
import functools

import numpy as np
import pytest

import dbkref
import reconref
from test_dbk_reference import planes_of
from test_gpu_dbk_reference import _ref_planes
from test_gpu_decoder import gpu_decode
from test_recon_reference import (ENC_CASES, ENC_REQUIRED, ENC_STREAM_IDS, LONG, RECON_DIRECTED, _nal_ref_idc, analysed,
                                  subsample_frames)

pytestmark = pytest.mark.gpu

DECODER_STREAMS = [f'recon_{n}' for n in RECON_DIRECTED] + list(LONG) + ['multi_1']
MULTISLICE = 'recon_qp_80x48'


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(access units, (w, h), per picture the chain's cropped I420) of one stream, computed once on the host"""
    a = analysed(name)
    assert a.chain_bad is None and a.stage_bad is None, f'{name}: the host chain does not stand (tests/test_recon_reference.py)'
    return a.units, a.size, [c[0] for c in a.chain]


def _explain(name, k, got, w, h):
    """where picture k of the GPU leaves the chain: reconref's explanation, or dbkref's if the unfiltered picture agrees
    (the GPU's unfiltered picture is not observable: the filtered one is explained by both references)"""
    a = analysed(name)
    prev = None
    for j in range(k + 1):
        res = reconref.reconstruct(a.syntax[j], a.geometry, prev)
        out = dbkref.deblock(res.planes, res.records, explain=(j == k))
        if _nal_ref_idc(a.units[j]):
            prev = out.planes
    gp = planes_of(got, w, h)
    msg = dbkref.first_difference(out, gp, w, h)
    for pl, (x, y) in enumerate(_first_xy(out.planes, gp, w, h)):
        if x is not None:
            return f'{msg} || {" | ".join(res.explain(pl, x, y))}'
    return msg


def _first_xy(ref, got, w, h):
    for k, (a, b) in enumerate(zip(ref, got)):
        hh, ww = (h, w) if k == 0 else (h // 2, w // 2)
        ne = np.argwhere(a[:hh, :ww] != np.asarray(b)[:hh, :ww])
        yield (int(ne[0][1]), int(ne[0][0])) if len(ne) else (None, None)


def _require_equal(name, k, ref, got, w, h, what):
    if not np.array_equal(ref, got):
        pytest.fail(f'{what}, picture {k}: ' + _explain(name, k, got, w, h))


@pytest.mark.parametrize('name', DECODER_STREAMS)
def test_decoder_vs_clauses_8_3_to_8_5(gpu_lib, name):
    units, (w, h), refs = _reference(name)
    L = gpu_lib
    assert L.init_decoder(12) == 0
    try:
        for k, u in enumerate(units):
            gw, gh, got = gpu_decode(L, 12, u, w, h)
            assert (gw, gh) == (w, h), f'{name} picture {k}: {gw}x{gh}'
            _require_equal(name, k, refs[k], got, w, h, f'{name} through decode_frame_yuv_i420')
    finally:
        L.deinit_decoder(12)


@pytest.mark.parametrize('waves', [1, 4])
@pytest.mark.parametrize('name', [MULTISLICE, 'long_48x48'])
def test_batch_decoder_two_frames_per_call(gpu_lib, name, waves):
    """IDR alone, then two P pictures in one call, then one more; `waves` slice waves"""
    import torch
    import h264mi
    units, (w, h), refs = _reference(name)
    dec = h264mi.BatchDecoder(w, h, 1, max_frames=2)
    try:
        dec.set_slice_waves(waves)
        dev = [torch.from_numpy(np.frombuffer(u, np.uint8).copy()).cuda() for u in units]
        for call in ([0], [1, 2], [3]):
            dec.decode_frames([dev[k].data_ptr() for k in call], nal_sizes=[len(units[k]) for k in call])
            rc, got = dec.status()
            assert rc == 0 and got == [1], (call, rc, got)
            pic = np.frombuffer(dec.picture_i420(0), np.uint8)
            _require_equal(name, call[-1], refs[call[-1]], pic, w, h, f'{name} through BatchDecoder, {waves} slice waves')
    finally:
        dec.close()


def test_batch_decoder_two_streams_of_different_content(gpu_lib):
    """two 48x48 streams in one batch, two pictures per call: a stream index slipping in the reference-plane
    addressing would predict one stream from the other's picture"""
    import torch
    import h264mi
    names = ['long_48x48', 'recon_fractions_48x48']
    refs = [_reference(n) for n in names]
    (w, h) = refs[0][1]
    assert refs[1][1] == (w, h)
    dec = h264mi.BatchDecoder(w, h, 2, max_frames=2)
    try:
        dev = [[torch.from_numpy(np.frombuffer(u, np.uint8).copy()).cuda() for u in r[0]] for r in refs]
        for call in ([0], [1, 2], [3, 4]):
            ptrs = [dev[s][k].data_ptr() for k in call for s in range(2)]          # nal_ptrs[f * S + s]
            sizes = [len(refs[s][0][k]) for k in call for s in range(2)]
            dec.decode_frames(ptrs, nal_sizes=sizes)
            rc, got = dec.status()
            assert rc == 0 and got == [1, 1], (call, rc, got)
            for s in range(2):
                pic = np.frombuffer(dec.picture_i420(s), np.uint8)
                _require_equal(names[s], call[-1], refs[s][2][call[-1]], pic, w, h, f'{names[s]} as stream {s} of a batch of two')
    finally:
        dec.close()


@pytest.mark.parametrize('nslices', [1, 3])
@pytest.mark.parametrize('case', ENC_CASES, ids=[f'{c[0]}x{c[1]}' for c in ENC_CASES])
def test_encoder_reference_planes_vs_clauses_8_3_to_8_5(gpu_lib, oracle, case, nslices):
    """3 streams (sub-sample motion, see above), 4 frames, frame skipping off: after each frame the planes the next
    frame predicts from == dbkref(reconref(the oracle's parse of the GPU's own access unit, the chain's previous picture)) -- the encoder's
    half-sample planes, quarter-sample averaging, intra predictors and transform / quantiser reconstruction against
    the standard's text"""
    import torch
    import h264mi
    w, h, br = case
    S, nf = len(ENC_STREAM_IDS), 4
    frames = [subsample_frames(sid, w, h) for sid in ENC_STREAM_IDS]
    enc = h264mi.BatchEncoder(w, h, br, S)
    ods = [oracle.decoder() for _ in range(S)]
    for d in ods:
        d.set_capture(True)
    prev = [None] * S
    counts = [reconref.Counter() for _ in range(S)]
    try:
        enc.set_frame_skip(False)
        enc.set_slices(nslices)
        for t in range(nf):
            enc.encode(torch.from_numpy(np.stack([f[t] for f in frames])).cuda())
            nb = enc.nal_sizes()
            assert all(x > 0 for x in nb), (t, nb)
            for s in range(S):
                rc, _, ow, oh = ods[s].decode(enc.nal_bytes(s, nb[s]))
                assert rc == 1 and (ow, oh) == (w, h), f'frame {t} stream {s}: the oracle decoder gives rc {rc}, {ow}x{oh}'
                cw, ch = ods[s].coded_size()
                res = reconref.reconstruct(ods[s].syntax(), (cw // 16, ch // 16), prev[s])
                counts[s].update(res.counts)
                out = dbkref.deblock(res.planes, res.records)
                got = _ref_planes(enc, s, cw, ch)
                if not all(np.array_equal(a[:hh, :ww], b[:hh, :ww]) for a, b, (hh, ww) in
                           zip(out.planes, got, ((h, w), (h // 2, w // 2), (h // 2, w // 2)))):
                    xy = list(_first_xy(out.planes, got, w, h))
                    pl = next(k for k, (x, _) in enumerate(xy) if x is not None)
                    pytest.fail(f'{w}x{h}, {nslices} slices, frame {t}, stream {s} (SyntheticStream {ENC_STREAM_IDS[s]}): '
                                + dbkref.first_difference(dbkref.deblock(res.planes, res.records, explain=True), got, w, h)
                                + ' || ' + ' | '.join(res.explain(pl, *xy[pl])))
                prev[s] = out.planes
    finally:
        enc.close()
    # the content reaches what this test is for: every stream its half-sample positions (b, h, j themselves and the
    # averages that read j), and intra macroblocks (the IDR pictures)
    for s, sid in enumerate(ENC_STREAM_IDS):
        missing = [p for p in ENC_REQUIRED[sid] if counts[s][('luma_frac', '16x16', p[0], p[1])] == 0]
        assert not missing, f'stream {s} (SyntheticStream {sid}): luma positions {missing} not reached'
        assert sum(v for k, v in counts[s].items() if k[0] in ('i4', 'i16')) > 0
