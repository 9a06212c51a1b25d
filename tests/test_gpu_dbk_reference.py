"""GPU: the loop filter (csrc/deblock.inc deblock_row, as dec_recon.inc and enc_mb_kernel.inc instantiate it with
DbkSrcGranules) against the independent reference of clause 8.7, tests/dbkref.py -- not against the oracle's filter,
which is a sibling of the kernel's. Every comparison is byte equality on the cropped window; a failure names the first
differing sample, its macroblock, the edge lines of the reference that cover it and the branch classes of 8.7 those
lines took (dbkref.first_difference), i.e. the clause that broke.

Decoder path: the DIRECTED streams of tests/test_dbk_reference.py (16x16, 16x48, 48x16, 80x48, 176x144: one
macroblock, one column, one row -- no top hand-over, first == last row --, three or more macroblocks per row for the
two-macroblock-lag hand-over) and one multi-slice layout, through the C-ABI; the multi-slice directed stream through
BatchDecoder, two frames per call, 1 and 4 slice waves. Encoder path: BatchEncoder's reference planes after every frame
== dbkref over the oracle decoder's parse of the GPU's own NAL bytes, so the QPs are the stream's mb_qp_delta chain as
a decoder sees it, not the encoder's bookkeeping (records flagged 0x80, DbkSrcGranules::resolve_qp / row_entry_qp)."""
import functools

import numpy as np
import pytest

import dbkref
from test_dbk_reference import DIRECTED, MULTISLICE_DIRECTED, SO, STREAMS, explain_difference, planes_of, reference_pictures
from test_gpu_decoder import gpu_decode

pytestmark = pytest.mark.gpu

DECODER_STREAMS = [f'directed_{n}' for n in DIRECTED] + ['multi_1']


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(access units, (w, h), per picture the reference's cropped I420) of one stream, computed once"""
    from _oracle import Oracle
    oracle = Oracle(SO)
    units, size = STREAMS[name][1](oracle)
    return units, size, [res.i420(w, h) for res, _, w, h in reference_pictures(oracle, units)]


def _require_equal(oracle, units, k, ref, got, w, h, what):
    if not np.array_equal(ref, got):
        pytest.fail(f'{what}, picture {k}: ' + explain_difference(oracle, units, k, planes_of(got, w, h), w, h))


@pytest.mark.parametrize('name', DECODER_STREAMS)
def test_decoder_vs_clause_8_7(gpu_lib, oracle, name):
    units, (w, h), refs = _reference(name)
    L = gpu_lib
    assert L.init_decoder(11) == 0
    try:
        for k, u in enumerate(units):
            gw, gh, got = gpu_decode(L, 11, u, w, h)
            assert (gw, gh) == (w, h), f'{name} picture {k}: {gw}x{gh}'
            _require_equal(oracle, units, k, refs[k], got, w, h, f'{name} through decode_frame_yuv_i420')
    finally:
        L.deinit_decoder(11)


@pytest.mark.parametrize('waves', [1, 4])
def test_batch_decoder_two_frames_per_call(gpu_lib, oracle, waves):
    """the multi-slice directed stream: IDR alone, then two P pictures in one call, then one; `waves` slice waves"""
    import torch
    import h264mi
    name = f'directed_{MULTISLICE_DIRECTED}'
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
            _require_equal(oracle, units, call[-1], refs[call[-1]], pic, w, h, f'{name} through BatchDecoder, {waves} slice waves')
    finally:
        dec.close()


ENC_CASES = [(80, 48, 100000), (176, 144, 300000)]
ENC_STREAM_IDS = (0, 1, 3)   # SyntheticStream ids whose one-slice streams hold P_Skip runs beside coded macroblocks and
                             # macroblock edges between differing QPs at both sizes (measured with dbkref's counters)


def _ref_planes(enc, s, cw, ch):
    """the encoder's padded motion-search planes of stream s -> the (Y, U, V) interiors (luma plane G, Cb, Cr)"""
    import ctypes
    lps, lph, cps, cph = cw + 80, ch + 64, cw // 2 + 40, ch // 2 + 32
    buf = np.zeros(4 * lps * lph + 2 * cps * cph, np.uint8)
    assert enc._L.h264mi_enc_ref_planes(enc._e, s, ctypes.c_void_p(buf.ctypes.data)) == 0
    y = buf[:lps * lph].reshape(lph, lps)[32:32 + ch, 40:40 + cw]
    c = [buf[4 * lps * lph + k * cps * cph:4 * lps * lph + (k + 1) * cps * cph].reshape(cph, cps)[16:16 + ch // 2, 20:20 + cw // 2]
         for k in range(2)]
    return y, c[0], c[1]


@pytest.mark.parametrize('nslices', [1, 3])
@pytest.mark.parametrize('case', ENC_CASES, ids=[f'{c[0]}x{c[1]}' for c in ENC_CASES])
def test_encoder_reference_planes_vs_clause_8_7(gpu_lib, oracle, case, nslices):
    """3 streams, 4 frames, frame skipping off: after each frame the reference planes the next frame predicts from ==
    dbkref(the oracle decoder's picture before its filter, its records) of the GPU's own access unit"""
    import torch
    import h264mi
    from h264mi.synth import SyntheticStream
    w, h, br = case
    S, nf = len(ENC_STREAM_IDS), 4
    gens = [SyntheticStream(sid, w, h) for sid in ENC_STREAM_IDS]
    enc = h264mi.BatchEncoder(w, h, br, S)
    ods = [oracle.decoder() for _ in range(S)]
    for d in ods:
        d.set_capture(True)
    counts, skipped_mbs = dbkref.Counter(), 0
    try:
        enc.set_frame_skip(False)
        enc.set_slices(nslices)
        for t in range(nf):
            enc.encode(torch.from_numpy(np.stack([np.ascontiguousarray(g.frame(t)) for g in gens])).cuda())
            nb = enc.nal_sizes()
            assert all(x > 0 for x in nb), (t, nb)
            for s in range(S):
                rc, _, ow, oh = ods[s].decode(enc.nal_bytes(s, nb[s]))
                assert rc == 1 and (ow, oh) == (w, h), f'frame {t} stream {s}: the oracle decoder gives rc {rc}, {ow}x{oh}'
                pre, rec = ods[s].prefilter(), ods[s].records()
                cw, ch = ods[s].coded_size()
                res = dbkref.deblock(pre, rec)
                counts.update(res.counts)
                skipped_mbs += int(np.count_nonzero(rec[:, 0] == 3))
                got = _ref_planes(enc, s, cw, ch)
                if not all(np.array_equal(a[:hh, :ww], b[:hh, :ww]) for a, b, (hh, ww) in
                           zip(res.planes, got, ((h, w), (h // 2, w // 2), (h // 2, w // 2)))):
                    pytest.fail(f'{w}x{h}, {nslices} slices, frame {t}, stream {s} (SyntheticStream {ENC_STREAM_IDS[s]}): '
                                + dbkref.first_difference(dbkref.deblock(pre, rec, explain=True), got, w, h))
    finally:
        enc.close()
    if nslices == 1:  # the content reaches what this test is for (one slice: the oracle encoder's streams, measured on the CPU)
        assert skipped_mbs > 0 and counts[('luma', 'v', 'mbedge_bs0')] > 0 and counts[('luma', 'v', 'mbedge_bs2')] > 0
        assert counts[('luma', 'h', 'qp_differ')] > 0
