"""GPU: the parse kernels (csrc/dec_parse.inc, cavlc_blk.inc) and the encoder's bit writer (csrc/enc_bits.inc) against
the from-bytes chain of tests/test_parse_reference.py: tests/parseref.py (clauses 7.3, 9.1, 9.2) parses the bytes,
tests/reconref.py (8.3-8.5) and tests/dbkref.py (8.7) rebuild the pictures -- no oracle in between. Every comparison is
byte equality; a failure names the first differing sample, its macroblock and parseref's code words of that macroblock.

Decoder: every directed stream of test_parse_reference.PARSE_DIRECTED (the table sweeps written by parseref's own
writer, every mb_type and coded_block_pattern, emulation prevention bytes in pcm_sample and in a NAL's tail, a slice
longer than two LDS rings) through the C-ABI; the two-slice sweep and the ring stream through BatchDecoder, two pictures
per call, at 1 and 4 slice waves.

Encoder: the access units BatchEncoder emits for test_recon_reference.subsample_frames, sent through the chain, == the
encoder's own reference planes after every frame, with 1 and 3 slices."""
import functools

import numpy as np
import pytest

import dbkref
import parseref
import reconref
from test_dbk_reference import planes_of
from test_gpu_dbk_reference import _ref_planes
from test_gpu_decoder import gpu_decode
from test_parse_reference import MULTISLICE, PARSE_DIRECTED, RING, parsed
from test_recon_reference import ENC_CASES, ENC_STREAM_IDS, subsample_frames

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _reference(name):
    a = parsed(name)
    assert a.parse_bad is None and a.chain_bad is None, f'{name}: the host chain does not stand (tests/test_parse_reference.py)'
    return a.units, a.size, a.chain


def _first_difference(ref_planes, got_planes, w, h, mbw, explain):
    """'plane p sample (x, y): reference r, GPU g; MB a: <its code words>' of the first differing sample inside w x h"""
    for pl, (a, b) in enumerate(zip(ref_planes, got_planes)):
        hh, ww = (h, w) if pl == 0 else (h // 2, w // 2)
        ne = np.argwhere(np.asarray(a)[:hh, :ww] != np.asarray(b)[:hh, :ww])
        if len(ne):
            y, x = (int(v) for v in ne[0])
            s = 16 if pl == 0 else 8
            mb = (y // s) * mbw + x // s
            return (f'plane {pl} sample ({x}, {y}): reference {int(a[y, x])}, GPU {int(b[y, x])}; MB {mb} ({x // s}, {y // s}): '
                    + ' | '.join(explain(mb)))[:4000]
    return 'no difference inside the cropped picture'


def _require_equal(name, k, ref, got, w, h, what):
    if not np.array_equal(ref, got):
        p = parsed(name).parsed[k]
        pytest.fail(f'{what}, picture {k}: ' + _first_difference(planes_of(ref, w, h), planes_of(got, w, h), w, h, p.geometry[0], p.explain))


@pytest.mark.parametrize('name', list(PARSE_DIRECTED))
def test_decoder_vs_from_bytes_chain(gpu_lib, name):
    units, (w, h), refs = _reference(name)
    L = gpu_lib
    assert L.init_decoder(13) == 0
    try:
        for k, u in enumerate(units):
            gw, gh, got = gpu_decode(L, 13, u, w, h)
            assert (gw, gh) == (w, h), f'{name} picture {k}: {gw}x{gh}'
            _require_equal(name, k, refs[k], got, w, h, f'{name} through decode_frame_yuv_i420')
    finally:
        L.deinit_decoder(13)


@pytest.mark.parametrize('waves', [1, 4])
@pytest.mark.parametrize('name', [MULTISLICE, RING])
def test_batch_decoder_two_frames_per_call(gpu_lib, name, waves):
    """IDR alone, then two P pictures per call; `waves` slice waves"""
    import torch
    import h264mi
    units, (w, h), refs = _reference(name)
    dec = h264mi.BatchDecoder(w, h, 1, max_frames=2)
    try:
        dec.set_slice_waves(waves)
        dev = [torch.from_numpy(np.frombuffer(u, np.uint8).copy()).cuda() for u in units]
        calls = [[0]] + [[k, k + 1] for k in range(1, len(units) - 1, 2)]
        for call in calls:
            dec.decode_frames([dev[k].data_ptr() for k in call], nal_sizes=[len(units[k]) for k in call])
            rc, got = dec.status()
            assert rc == 0 and got == [1], (call, rc, got)
            pic = np.frombuffer(dec.picture_i420(0), np.uint8)
            _require_equal(name, call[-1], refs[call[-1]], pic, w, h, f'{name} through BatchDecoder, {waves} slice waves')
    finally:
        dec.close()


@pytest.mark.parametrize('nslices', [1, 3])
@pytest.mark.parametrize('case', ENC_CASES, ids=[f'{c[0]}x{c[1]}' for c in ENC_CASES])
def test_encoder_bytes_through_the_chain(gpu_lib, case, nslices):
    """3 streams, 4 frames, frame skipping off: dbkref(reconref(parseref(the encoder's own bytes), the chain's previous
    picture)) == the encoder's reference planes after every frame -- enc_bits.inc's writer judged without the oracle"""
    import torch
    import h264mi
    w, h, br = case
    S, nf = len(ENC_STREAM_IDS), 4
    frames = [subsample_frames(sid, w, h) for sid in ENC_STREAM_IDS]
    enc = h264mi.BatchEncoder(w, h, br, S)
    states = [parseref.State() for _ in range(S)]
    prev = [None] * S
    try:
        enc.set_frame_skip(False)
        enc.set_slices(nslices)
        for t in range(nf):
            enc.encode(torch.from_numpy(np.stack([f[t] for f in frames])).cuda())
            nb = enc.nal_sizes()
            assert all(x > 0 for x in nb), (t, nb)
            for s in range(S):
                p = parseref.parse(enc.nal_bytes(s, nb[s]), states[s])
                assert p.size == (w, h), f'frame {t} stream {s}: parsed size {p.size}'
                mbw, mbh = p.geometry
                res = reconref.reconstruct(p.syntax, p.geometry, prev[s])
                out = dbkref.deblock(res.planes, res.records)
                got = _ref_planes(enc, s, 16 * mbw, 16 * mbh)
                if not all(np.array_equal(a[:hh, :ww], np.asarray(b)[:hh, :ww]) for a, b, (hh, ww) in
                           zip(out.planes, got, ((h, w), (h // 2, w // 2), (h // 2, w // 2)))):
                    pytest.fail(f'{w}x{h}, {nslices} slices, frame {t}, stream {s} (SyntheticStream {ENC_STREAM_IDS[s]}): '
                                + _first_difference(out.planes, got, w, h, mbw, p.explain))
                prev[s] = out.planes
    finally:
        enc.close()
