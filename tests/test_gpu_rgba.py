"""GPU: RGBA frames in and out of the device-resident batch API -- the batched colour conversions alone
(h264mi_rgba_to_i420_dev / h264mi_i420_to_rgba_dev), BatchEncoder.encode_rgba, BatchDecoder's RGBA output and
the round trip. Integer formulas with a CPU oracle: every comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5


def _guarded(nbytes, shift=0):
    """a device buffer of nbytes behind `shift` bytes of misalignment, 64 guard bytes of 0xA5 on either side"""
    import torch
    whole = torch.full((GUARD + shift + nbytes + GUARD,), FILL, dtype=torch.uint8, device='cuda')
    return whole, whole[GUARD + shift:GUARD + shift + nbytes]


def _guards_intact(whole, shift, nbytes):
    h = whole.cpu().numpy()
    return bool(np.all(h[:GUARD + shift] == FILL) and np.all(h[GUARD + shift + nbytes:] == FILL))


def _rgba_input(w, h, n, seed):
    """uniform random bytes in every channel, alpha included; every frame starts with the 8 corners of the RGB cube"""
    a = np.random.default_rng(seed).integers(0, 256, (n, w * h, 4), dtype=np.uint8)
    k = min(8, w * h)
    for c in range(k):
        a[:, c, :3] = [255 * (c & 1), 255 * ((c >> 1) & 1), 255 * ((c >> 2) & 1)]
    return a.reshape(n, w * h * 4)


CONVERT_CASES = [
    (2, 2, 1, 0, 0),        # one 2x2 block, no vector path
    (16, 16, 2, 0, 0),      # vector path, frame stride
    (18, 16, 3, 0, 0),      # w % 8 != 0; w*h*3/2 per frame breaks 16-byte alignment of later frames
    (24, 18, 2, 0, 0),      # w % 8 == 0 with an I420 frame size (648) that is not a multiple of 16
    (200, 2, 1, 0, 0),      # a single row pair, part of one wave
    (520, 10, 2, 0, 0),     # more than one wave per row, plus a partial wave
    (1920, 1080, 3, 0, 0),  # the workload's geometry, once
    (16, 16, 2, 4, 2),      # bases shifted inside their allocations (RGBA by 4 bytes, I420 by 2): the 2-pixel path
    (18, 16, 3, 4, 2),
]


@pytest.mark.parametrize('w,h,n,srgba,si420', CONVERT_CASES, ids=[f'{c[0]}x{c[1]}-n{c[2]}' + ('-shifted' if c[3] else '') for c in CONVERT_CASES])
def test_batched_conversions_vs_oracle(gpu_lib, oracle, w, h, n, srgba, si420):
    import torch
    import h264mi
    fr, fi = w * h * 4, w * h * 3 // 2
    # RGBA -> I420
    rgba = _rgba_input(w, h, n, 100 + w + h + n)
    _, src = _guarded(n * fr, srgba)
    src.copy_(torch.from_numpy(rgba.ravel()))
    whole, dst = _guarded(n * fi, si420)
    h264mi.rgba_to_i420(dst, src, w, h, n)
    torch.cuda.synchronize()
    got = dst.cpu().numpy().reshape(n, fi)
    for f in range(n):
        assert np.array_equal(got[f], oracle.rgba_to_i420(rgba[f], w, h)), f'rgba->i420 frame {f}'
    assert _guards_intact(whole, si420, n * fi)
    # I420 -> RGBA: full-range YUV reaches both clamps of every channel
    yuv = np.random.default_rng(200 + w + h + n).integers(0, 256, (n, fi), dtype=np.uint8)
    _, src = _guarded(n * fi, si420)
    src.copy_(torch.from_numpy(yuv.ravel()))
    whole, dst = _guarded(n * fr, srgba)
    h264mi.i420_to_rgba(dst, src, w, h, n)
    torch.cuda.synchronize()
    got = dst.cpu().numpy().reshape(n, fr)
    for f in range(n):
        assert np.array_equal(got[f], oracle.i420_to_rgba(yuv[f], w, h)), f'i420->rgba frame {f}'
    assert _guards_intact(whole, srgba, n * fr)


def test_conversion_bad_arguments(gpu_lib):
    import torch
    L = gpu_lib
    a = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    b = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    pa, pb = ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr())
    for fn in (L.h264mi_rgba_to_i420_dev, L.h264mi_i420_to_rgba_dev):
        assert fn(pa, pb, 16, 16, 1, None) == 0
        assert fn(pa, pb, 15, 16, 1, None) == -1   # odd w
        assert fn(pa, pb, 16, 15, 1, None) == -1   # odd h
        assert fn(pa, pb, 16, 16, 0, None) == -1   # n = 0
        assert fn(pa, pb, 0, 16, 1, None) == -1
        assert fn(pa, pb, 16, -2, 1, None) == -1
        assert fn(None, pb, 16, 16, 1, None) == -1
        assert fn(pa, None, 16, 16, 1, None) == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------- encoder / decoder

NFRAMES = 3


def _crop_planes(buf, cw, ch, w, h):
    """tight w x h I420 from contiguous coded-size planes"""
    y = buf[:cw * ch].reshape(ch, cw)[:h, :w]
    u = buf[cw * ch:cw * ch * 5 // 4].reshape(ch // 2, cw // 2)[:h // 2, :w // 2]
    v = buf[cw * ch * 5 // 4:cw * ch * 3 // 2].reshape(ch // 2, cw // 2)[:h // 2, :w // 2]
    return np.concatenate([y.ravel(), u.ravel(), v.ravel()])


@functools.lru_cache(maxsize=None)
def _encoded(w, h, br, S):
    """S streams x NFRAMES frames through BatchEncoder.encode_rgba: the RGBA inputs (golden.make_golden.rgba_frame, a
    seed per stream and frame) and every stream's NAL bytes per frame. Computed once per geometry."""
    import torch
    import h264mi
    from golden.make_golden import rgba_frame
    rgba = [[rgba_frame(w, h, 50 * s + f).reshape(-1) for s in range(S)] for f in range(NFRAMES)]
    enc = h264mi.BatchEncoder(w, h, br, S)
    enc.set_frame_skip(False)
    assert enc.rgba_frame_bytes == w * h * 4 == h264mi.lib().h264mi_enc_rgba_frame_bytes(enc._e)
    nals = []
    for f in range(NFRAMES):
        frames = torch.from_numpy(np.concatenate(rgba[f])).cuda()  # held until nal_sizes() has synchronised
        enc.encode_rgba(frames)
        sizes = enc.nal_sizes()
        nals.append([enc.nal_bytes(s, sizes[s]) for s in range(S)])
    enc.close()
    return rgba, nals


@pytest.mark.parametrize('w,h,br,S', [(176, 144, 300000, 3), (208, 120, 500000, 2)], ids=['qcif-s3', 'crop-s2'])
def test_encode_rgba_vs_oracle_and_i420_path(gpu_lib, oracle, w, h, br, S):
    import torch
    import h264mi
    rgba, nals = _encoded(w, h, br, S)
    oes = [oracle.encoder(w, h, br) for _ in range(S)]
    for oe in oes:
        oe.set_frame_skip(False)
    enc2 = h264mi.BatchEncoder(w, h, br, S)
    enc2.set_frame_skip(False)
    for f in range(NFRAMES):
        i420 = [oracle.rgba_to_i420(rgba[f][s], w, h) for s in range(S)]
        enc2.encode(torch.from_numpy(np.concatenate(i420)).cuda())
        sizes = enc2.nal_sizes()
        for s in range(S):
            assert len(nals[f][s]) > 0
            assert nals[f][s] == oes[s].encode(i420[s]), f'frame {f} stream {s}: encode_rgba != oracle'
            assert nals[f][s] == enc2.nal_bytes(s, sizes[s]), f'frame {f} stream {s}: encode_rgba != encode(I420)'
    enc2.close()


def _nal_tensors(nals, skip=()):
    """device copies of nals[f][s], pointer and size lists indexed f * S + s; (f, s) in skip gets size 0"""
    import torch
    dev = [[torch.from_numpy(np.frombuffer(u, np.uint8).copy()).cuda() for u in fr] for fr in nals]
    ptrs = [d.data_ptr() for fr in dev for d in fr]
    sizes = [0 if (f, s) in skip else len(u) for f, fr in enumerate(nals) for s, u in enumerate(fr)]
    return dev, ptrs, sizes


def test_decoder_rgba_output(gpu_lib, oracle):
    import torch
    import h264mi
    w, h, br, S = 208, 120, 500000, 2
    _, nals = _encoded(w, h, br, S)
    pics = []  # the oracle decoder's picture per frame and stream
    ods = [oracle.decoder() for _ in range(S)]
    for f in range(NFRAMES):
        row = []
        for s in range(S):
            rc, pic, pw, ph = ods[s].decode(nals[f][s])
            assert rc == 1 and (pw, ph) == (w, h)
            row.append(pic)
        pics.append(row)
    fr, fi, m = w * h * 4, w * h * 3 // 2, NFRAMES * S
    dev, ptrs, sizes = _nal_tensors(nals)

    # all 3 frames in one call, RGBA out
    dec = h264mi.BatchDecoder(w, h, S, max_frames=NFRAMES)
    assert dec.output_format() == 'i420'
    dec.set_output_format('rgba')
    assert dec.output_format() == 'rgba'
    bufs = [_guarded(fr) for _ in range(m)]
    got = torch.full((m,), 7, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()  # the fills run on torch's stream, the decoder on its own
    dec.decode_frames(ptrs, nal_sizes=sizes, out_ptrs=[b[1].data_ptr() for b in bufs], got_ptrs=[got[i:i + 1].data_ptr() for i in range(m)])
    torch.cuda.synchronize()
    assert got.cpu().tolist() == [1] * m
    for f in range(NFRAMES):
        for s in range(S):
            whole, out = bufs[f * S + s]
            assert np.array_equal(out.cpu().numpy(), oracle.i420_to_rgba(pics[f][s], w, h)), f'frame {f} stream {s}'
            assert _guards_intact(whole, 0, fr)
    dec.close()

    # a fresh decoder; stream 1's frame 1 is an access unit of size 0: no picture, buffer untouched
    dec = h264mi.BatchDecoder(w, h, S, max_frames=NFRAMES)
    dec.set_output_format('rgba')
    _, _, sizes0 = _nal_tensors(nals, skip={(1, 1)})
    bufs = [_guarded(fr) for _ in range(m)]
    got = torch.full((m,), 7, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()  # the fills run on torch's stream, the decoder on its own
    dec.decode_frames(ptrs, nal_sizes=sizes0, out_ptrs=[b[1].data_ptr() for b in bufs], got_ptrs=[got[i:i + 1].data_ptr() for i in range(m)])
    torch.cuda.synchronize()
    g = got.cpu().tolist()
    assert g[1 * S + 1] == 0
    assert np.all(bufs[1 * S + 1][0].cpu().numpy() == FILL)
    for f in range(NFRAMES):  # stream 0 is unaffected
        assert g[f * S] == 1
        assert np.array_equal(bufs[f * S][1].cpu().numpy(), oracle.i420_to_rgba(pics[f][0], w, h)), f'frame {f} stream 0'

    # the same decoder back to I420 for the next call (the streams again from their IDR): the format is per call
    dec.set_output_format('i420')
    bufs = [_guarded(fi) for _ in range(m)]
    got = torch.full((m,), 7, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()  # the fills run on torch's stream, the decoder on its own
    dec.decode_frames(ptrs, nal_sizes=sizes, out_ptrs=[b[1].data_ptr() for b in bufs], got_ptrs=[got[i:i + 1].data_ptr() for i in range(m)])
    torch.cuda.synchronize()
    assert got.cpu().tolist() == [1] * m
    for f in range(NFRAMES):
        for s in range(S):
            whole, out = bufs[f * S + s]
            assert np.array_equal(out.cpu().numpy(), pics[f][s]), f'I420 frame {f} stream {s}'
            assert _guards_intact(whole, 0, fi)
    with pytest.raises(ValueError):
        dec.set_output_format('nv12')
    dec.close()
    del dev


def test_rgba_round_trip_device_pointers(gpu_lib, oracle):
    """encode_rgba -> decode_frames from the encoder's device NAL and size pointers -> RGBA, S = 8: equals the
    conversion of the encoder's own reconstruction, every stream, every frame"""
    import torch
    import h264mi
    from golden.make_golden import rgba_frame
    w, h, S, nf = 176, 144, 8, 2
    fr = w * h * 4
    st = torch.cuda.Stream()  # one stream for both: the decoder's inputs are ordered behind the encoder by the stream alone
    enc = h264mi.BatchEncoder(w, h, 300000, S, stream=st)
    enc.set_frame_skip(False)
    dec = h264mi.BatchDecoder(w, h, S, stream=st)
    dec.set_output_format('rgba')
    n = dec.cw * dec.ch * 3 // 2
    for f in range(nf):
        frames = torch.from_numpy(np.concatenate([rgba_frame(w, h, 300 + 10 * s + f).reshape(-1) for s in range(S)])).cuda()
        bufs = [_guarded(fr) for _ in range(S)]
        got = torch.zeros(S, dtype=torch.int32, device='cuda')
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            enc.encode_rgba(frames)
            dec.decode_frames(enc.nal_ptrs(), size_ptrs=enc.nal_size_ptrs(), out_ptrs=[b[1].data_ptr() for b in bufs],
                              got_ptrs=[got[s:s + 1].data_ptr() for s in range(S)])
        torch.cuda.synchronize()
        assert got.cpu().tolist() == [1] * S
        for s in range(S):
            rec = np.empty(n, np.uint8)
            h264mi._hip_memcpy_d2h(rec.ctypes.data, enc.recon_ptr(s), n)
            want = oracle.i420_to_rgba(_crop_planes(rec, dec.cw, dec.ch, w, h), w, h)
            assert np.array_equal(bufs[s][1].cpu().numpy(), want), f'frame {f} stream {s}'
            assert _guards_intact(bufs[s][0], 0, fr)
    enc.close()
    dec.close()
