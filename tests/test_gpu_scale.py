"""GPU: the I420 area-average downscaler -- the standalone call h264mi_i420_scale_dev and the encoder's scaled input
h264mi_enc_encode_scaled -- against tests/scaleref.py. The definition is exact integer arithmetic, so every
comparison is equality of bytes; every destination sits between 64 guard bytes that must stay as they were."""
import ctypes
import functools

import numpy as np
import pytest

import qualityref
import scaleref

pytestmark = pytest.mark.gpu

GUARD = 64


def _device(x, shift=0):
    """x's bytes on the device, `shift` bytes into a larger allocation"""
    import torch
    whole = torch.zeros(x.size + shift + 64, dtype=torch.uint8, device='cuda')
    view = whole[shift:shift + x.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(x).ravel()))
    return view


def _guarded(nbytes, shift=0):
    """(whole, view): a destination of nbytes between 64 bytes of 0xA5 on each side, `shift` bytes into its allocation"""
    import torch
    whole = torch.full((shift + nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    return whole, whole[shift + GUARD:shift + GUARD + nbytes]


def _guards_intact(whole, nbytes, shift=0):
    h = whole.cpu().numpy()
    return bool((h[:shift + GUARD] == 0xA5).all() and (h[shift + GUARD + nbytes:] == 0xA5).all())


def _scale(src, sw, sh, dw, dh, n, shift=0):
    """the standalone call on n frames (a (n, frame bytes) array): the n scaled frames as an array, guards checked"""
    import h264mi
    dfb = scaleref.frame_bytes(dw, dh)
    d_src = _device(src, shift)
    whole, dst = _guarded(n * dfb, shift)
    if shift:
        assert d_src.data_ptr() % 2 == 1 and dst.data_ptr() % 2 == 1
    h264mi.i420_scale(dst, d_src, sw, sh, dw, dh, n)
    out = dst.cpu().numpy().reshape(n, dfb)
    assert _guards_intact(whole, n * dfb, shift), 'bytes outside the destination frames were written'
    return out


def _frames(w, h, n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, scaleref.frame_bytes(w, h)), dtype=np.uint8)


# (sw, sh, dw, dh, shift): each the smallest shape that reaches its case
#   16x16 and 36x18 onto themselves: identity; 32x32 -> 16x16: 2:1; 48x36 -> 32x24: 3:2, two taps of unequal weight;
#   36x18 -> 20x10: chroma 18x9 -> 10x5, three taps, odd plane sizes, rows that are no multiple of 4 bytes;
#   38x22 -> 38x10 and -> 20x22: one direction only; 256x64 -> 16x16: 16 horizontal taps, 4 vertical;
#   16x16 -> 2x2: a 1x1 chroma plane; 1280x48 -> 852x32: several column strips per row, chroma 426 wide, two row
#   segments; the same with source and destination at odd addresses: the byte path; 4096x64 -> 854x16: the widest source
SHAPES = [(16, 16, 16, 16, 0), (36, 18, 36, 18, 0), (32, 32, 16, 16, 0), (48, 36, 32, 24, 0), (36, 18, 20, 10, 0),
          (38, 22, 38, 10, 0), (38, 22, 20, 22, 0), (256, 64, 16, 16, 0), (16, 16, 2, 2, 0), (1280, 48, 852, 32, 0),
          (1280, 48, 852, 32, 1), (4096, 64, 854, 16, 0)]


@pytest.mark.parametrize('sw,sh,dw,dh,shift', SHAPES,
                         ids=[f'{c[0]}x{c[1]}-to-{c[2]}x{c[3]}' + ('-odd-address' if c[4] else '') for c in SHAPES])
def test_standalone_vs_reference(gpu_lib, sw, sh, dw, dh, shift):
    n = 3
    src = _frames(sw, sh, n, 2000 + sw + sh + dw + dh)
    got = _scale(src, sw, sh, dw, dh, n, shift)
    for f in range(n):
        want = scaleref.scale_frame(src[f], sw, sh, dw, dh)
        assert np.array_equal(got[f], want), f'frame {f}: {int((got[f] != want).sum())} bytes differ'
    if (sw, sh) == (dw, dh):
        assert np.array_equal(got, src)


def test_accumulator_needs_all_32_bits(gpu_lib):
    """all-255 4096x4096 -> 16x16: the numerator reaches 255 * 2^24 + 2^23 = 4 286 578 688, above 2^31"""
    import torch
    import h264mi
    sw = sh = 4096
    dfb = scaleref.frame_bytes(16, 16)
    src = torch.full((scaleref.frame_bytes(sw, sh),), 255, dtype=torch.uint8, device='cuda')
    whole, dst = _guarded(dfb)
    h264mi.i420_scale(dst, src, sw, sh, 16, 16, 1)
    out = dst.cpu().numpy()
    assert 255 * sw * sh + (sw * sh >> 1) == 4286578688 > 1 << 31
    assert (out == 255).all()
    assert _guards_intact(whole, dfb)


def test_repeatability(gpu_lib):
    src = _frames(1280, 48, 3, 77)
    a = _scale(src, 1280, 48, 852, 32, 3)
    b = _scale(src, 1280, 48, 852, 32, 3)
    assert a.tobytes() == b.tobytes()


def test_standalone_bad_arguments(gpu_lib):
    import torch
    from test_scale_host import BAD
    fn = gpu_lib.h264mi_i420_scale_dev
    s = torch.zeros(3 * 1536, dtype=torch.uint8, device='cuda')
    whole, d = _guarded(3 * 384)
    ps, pd = ctypes.c_void_p(s.data_ptr()), ctypes.c_void_p(d.data_ptr())
    assert fn(pd, 16, 16, ps, 32, 32, 3, None) == 0
    assert fn(None, 16, 16, ps, 32, 32, 1, None) == -1 and fn(pd, 16, 16, None, 32, 32, 1, None) == -1
    for dw, dh, sw, sh, n in BAD:
        assert fn(pd, dw, dh, ps, sw, sh, n, None) == -1, (dw, dh, sw, sh, n)
    for off in (0, 1, 1535):  # the destination inside the source
        assert fn(ctypes.c_void_p(s.data_ptr() + off), 16, 16, ps, 32, 32, 1, None) == -1
    assert fn(ctypes.c_void_p(s.data_ptr() + 1536), 16, 16, ps, 32, 32, 3, None) == -1  # inside the second frame
    assert fn(ctypes.c_void_p(s.data_ptr() + 1536), 16, 16, ps, 32, 32, 1, None) == 0   # right behind the only one
    torch.cuda.synchronize()
    assert _guards_intact(whole, 3 * 384)


# ---------------------------------------------------------------- the encoder's scaled input


@functools.lru_cache(maxsize=None)
def _sources(w, h, S, nf):
    from h264mi.synth import SyntheticStream
    gs = [SyntheticStream(s, w, h) for s in range(S)]
    return [np.stack([np.ascontiguousarray(g.frame(t)).ravel() for g in gs]) for t in range(nf)]


@functools.lru_cache(maxsize=None)
def _scaled_sources(sw, sh, dw, dh, S, nf):
    return [np.stack([scaleref.scale_frame(f, sw, sh, dw, dh) for f in step]) for step in _sources(sw, sh, S, nf)]


def _crop_frame(buf, cw, ch, w, h):
    y = buf[:cw * ch].reshape(ch, cw)[:h, :w]
    u = buf[cw * ch:cw * ch * 5 // 4].reshape(ch // 2, cw // 2)[:h // 2, :w // 2]
    v = buf[cw * ch * 5 // 4:cw * ch * 3 // 2].reshape(ch // 2, cw // 2)[:h // 2, :w // 2]
    return np.concatenate([y.ravel(), u.ravel(), v.ravel()])


def _recon(enc, s):
    import h264mi
    cw, ch = (enc.w + 15) // 16 * 16, (enc.h + 15) // 16 * 16
    buf = np.empty(cw * ch * 3 // 2, np.uint8)
    h264mi._hip_memcpy_d2h(buf.ctypes.data, enc.recon_ptr(s), buf.size)
    return _crop_frame(buf, cw, ch, enc.w, enc.h)


def _run(w, h, br, S, steps, feed, quality=False):
    """one encoder over `steps` (a list of (S, frame bytes) arrays), fed by feed(enc, device frames): per step the NAL
    bytes, rc_state and, with quality on, the records and the reconstructions"""
    import torch
    import h264mi
    enc = h264mi.BatchEncoder(w, h, br, S)
    enc.set_frame_skip(False)
    enc.set_quality(quality)
    out = []
    for fr in steps:
        frames = torch.from_numpy(np.ascontiguousarray(fr).ravel()).cuda()  # held until nal_sizes() has synchronised
        feed(enc, frames)
        sizes = enc.nal_sizes()
        st = {'nal': [enc.nal_bytes(s, sizes[s]) for s in range(S)], 'rc': [enc.rc_state(s) for s in range(S)]}
        if quality:
            st['q'] = [enc.quality(s) for s in range(S)]
            st['recon'] = [_recon(enc, s) for s in range(S)]
        out.append(st)
    enc.close()
    return out


KEYS = ('sse', 'ssim_fix', 'windows', 'coded')


@pytest.mark.parametrize('sw,sh,dw,dh', [(352, 288, 176, 144), (144, 80, 72, 40)], ids=['qcif-from-cif', 'cropped-72x40-from-144x80'])
def test_encode_scaled_equals_encode_of_reference_frames(gpu_lib, sw, sh, dw, dh):
    S, nf, br = 2, 3, 300000
    src, ref = _sources(sw, sh, S, nf), _scaled_sources(sw, sh, dw, dh, S, nf)
    for quality in (False, True):
        got = _run(dw, dh, br, S, src, lambda e, f: e.encode_scaled(f, sw, sh), quality)
        want = _run(dw, dh, br, S, ref, lambda e, f: e.encode(f), quality)
        for t in range(nf):
            for s in range(S):
                assert len(got[t]['nal'][s]) > 0
                assert got[t]['nal'][s] == want[t]['nal'][s], f'frame {t} stream {s}: NAL bytes'
                assert got[t]['rc'][s] == want[t]['rc'][s], f'frame {t} stream {s}: rate-control state'
                if quality:
                    q = {k: got[t]['q'][s][k] for k in KEYS}
                    assert q == qualityref.frame_quality(ref[t][s], got[t]['recon'][s], dw, dh), f'frame {t} stream {s}: records'
                    assert q == {k: want[t]['q'][s][k] for k in KEYS}


def test_encode_scaled_identity(gpu_lib):
    w, h, S, nf = 176, 144, 2, 3
    src = _sources(w, h, S, nf)
    got = _run(w, h, 300000, S, src, lambda e, f: e.encode_scaled(f, w, h))
    want = _run(w, h, 300000, S, src, lambda e, f: e.encode(f))
    for t in range(nf):
        assert got[t]['nal'] == want[t]['nal'] and got[t]['rc'] == want[t]['rc'], f'frame {t}'


def test_encode_scaled_refusals_leave_the_encoder_untouched(gpu_lib):
    import torch
    w, h, S = 176, 144, 2
    src = _sources(w, h, S, 1)[0]
    fresh = _run(w, h, 300000, S, [src], lambda e, f: e.encode(f))[0]
    big = torch.zeros(S * scaleref.frame_bytes(352, 288), dtype=torch.uint8, device='cuda')

    def feed(enc, frames):
        fn = enc._L.h264mi_enc_encode_scaled
        p = ctypes.c_void_p(big.data_ptr())
        for sw, sh in ((174, 144), (176, 142), (160, 288), (352, 120),   # smaller than the encoder
                       (177, 144), (352, 145), (353, 289),               # odd
                       (4098, 144), (176, 4098), (8192, 8192)):          # above 4096 (refused before anything is read)
            assert fn(enc._e, p, sw, sh) == -1, (sw, sh)
        for sw, sh in ((174, 144), (177, 145)):  # through the Python method: ValueError
            with pytest.raises(ValueError):
                enc.encode_scaled(big, sw, sh)
        assert fn(enc._e, None, 352, 288) == -1
        inp = enc._L.h264mi_enc_input_buffer(enc._e)  # frames that overlap the encoder's input area
        assert fn(enc._e, ctypes.c_void_p(inp), 352, 288) == -1
        assert fn(enc._e, ctypes.c_void_p(inp + S * scaleref.frame_bytes(w, h) - 1), 352, 288) == -1
        enc.encode(frames)

    got = _run(w, h, 300000, S, [src], feed)[0]
    assert got['nal'] == fresh['nal'] and got['rc'] == fresh['rc']
