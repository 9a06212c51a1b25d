"""GPU: rotating and mirroring I420 frames -- the standalone call h264mi_i420_orient_dev and the encoder's oriented
input h264mi_enc_encode_oriented -- against tests/orientref.py. Samples are moved, never computed, so every comparison
is equality of bytes; every destination sits between 64 guard bytes that must stay as they were. The tile of the
transposing orientations is 64 x 64 samples (csrc/orient.hip), which the shapes below are chosen around."""
import ctypes
import functools

import numpy as np
import pytest

import orientref
import qualityref

pytestmark = pytest.mark.gpu

GUARD = 64
NAMES = ('identity', 'rot90', 'rot180', 'rot270', 'mirror', 'flip', 'transpose', 'transverse')


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


def _orient(src, sw, sh, n, orient, shift=0):
    """the standalone call on n frames (a (n, frame bytes) array): the n turned frames as an array, guards checked"""
    import h264mi
    fb = orientref.frame_bytes(sw, sh)
    d_src = _device(src, shift)
    whole, dst = _guarded(n * fb, shift)
    if shift:
        assert d_src.data_ptr() % 2 == 1 and dst.data_ptr() % 2 == 1
    h264mi.i420_orient(dst, d_src, sw, sh, n, orient)
    out = dst.cpu().numpy().reshape(n, fb)
    assert _guards_intact(whole, n * fb, shift), 'bytes outside the destination frames were written'
    return out


@functools.lru_cache(maxsize=None)
def _frames(w, h, n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, orientref.frame_bytes(w, h)), dtype=np.uint8)  # shared: never written


# (sw, sh, shift): each the smallest shape that reaches its case
#   2x2: 1x1 chroma; 16x16; 36x18: chroma 18x9, rows that are no multiple of 4 bytes, odd plane sides;
#   64x64: chroma exactly half a tile; 128x64: whole tiles only; 130x66 and 66x130: one dword / row past a tile edge each
#   way, chroma 65x33; 1280x48 and 48x1280: many tiles one way (five strips of the rows kernel), a partial one the other;
#   130x66 with source and destination at odd addresses: the byte path; 8192x2 and 2x8192: the limit
SHAPES = [(2, 2, 0), (16, 16, 0), (36, 18, 0), (64, 64, 0), (128, 64, 0), (130, 66, 0), (66, 130, 0), (1280, 48, 0), (48, 1280, 0),
          (130, 66, 1), (8192, 2, 0), (2, 8192, 0)]


@pytest.mark.parametrize('orient', orientref.ALL, ids=NAMES)
@pytest.mark.parametrize('sw,sh,shift', SHAPES, ids=[f'{c[0]}x{c[1]}' + ('-odd-address' if c[2] else '') for c in SHAPES])
def test_standalone_vs_reference(gpu_lib, sw, sh, shift, orient):
    n = 3
    src = _frames(sw, sh, n, 3000 + sw + 3 * sh)
    got = _orient(src, sw, sh, n, orient, shift)
    for f in range(n):
        want = orientref.orient_frame(src[f], sw, sh, orient)
        assert np.array_equal(got[f], want), f'frame {f}: {int((got[f] != want).sum())} bytes differ'
    if orient == orientref.IDENTITY:
        assert np.array_equal(got, src)


def test_repeatability(gpu_lib):
    src = _frames(130, 66, 3, 78)
    for orient in (orientref.ROT180, orientref.ROT90):
        a = _orient(src, 130, 66, 3, orient)
        b = _orient(src, 130, 66, 3, orient)
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize('orient', orientref.TRANSPOSING, ids=[NAMES[k] for k in orientref.TRANSPOSING])
def test_round_trip_on_the_device(gpu_lib, orient):
    """orient, then its inverse, both on the device: the source"""
    import h264mi
    sw, sh, n = 130, 66, 3
    src = _frames(sw, sh, n, 79)
    fb = orientref.frame_bytes(sw, sh)
    d_src = _device(src)
    whole_a, mid = _guarded(n * fb)
    whole_b, back = _guarded(n * fb)
    h264mi.i420_orient(mid, d_src, sw, sh, n, orient)
    mw, mh = h264mi.orient_size(orient, sw, sh)
    inv = h264mi.orient_inverse(orient)
    assert h264mi.orient_size(inv, mw, mh) == (sw, sh) and h264mi.orient_compose(orient, inv) == orientref.IDENTITY
    h264mi.i420_orient(back, mid, mw, mh, n, inv)
    assert np.array_equal(back.cpu().numpy().reshape(n, fb), src)
    assert _guards_intact(whole_a, n * fb) and _guards_intact(whole_b, n * fb)


def test_standalone_bad_arguments(gpu_lib):
    import torch
    from test_orient_host import BAD
    fn = gpu_lib.h264mi_i420_orient_dev
    fb = orientref.frame_bytes(32, 16)
    s = torch.zeros(3 * fb, dtype=torch.uint8, device='cuda')
    whole, d = _guarded(3 * fb)
    ps, pd = ctypes.c_void_p(s.data_ptr()), ctypes.c_void_p(d.data_ptr())
    assert fn(pd, ps, 32, 16, 3, 1, None) == 0
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == 0).all()
    d.fill_(0xA5)
    assert fn(None, ps, 32, 16, 1, 1, None) == -1 and fn(pd, None, 32, 16, 1, 1, None) == -1
    for sw, sh, n, orient in BAD:
        assert fn(pd, ps, sw, sh, n, orient, None) == -1, (sw, sh, n, orient)
    for off in (0, 1, fb - 1):  # the destination inside the source
        assert fn(ctypes.c_void_p(s.data_ptr() + off), ps, 32, 16, 1, 1, None) == -1
    assert fn(ctypes.c_void_p(s.data_ptr() + 3 * fb - 1), ps, 32, 16, 3, 4, None) == -1  # the last byte of the third frame
    torch.cuda.synchronize()
    assert _guards_intact(whole, 3 * fb) and (d.cpu().numpy() == 0xA5).all(), 'a refused call wrote'


# ---------------------------------------------------------------- the encoder's oriented input


@functools.lru_cache(maxsize=None)
def _sources(w, h, S, nf):
    from h264mi.synth import SyntheticStream
    gs = [SyntheticStream(s, w, h) for s in range(S)]
    return [np.stack([np.ascontiguousarray(g.frame(t)).ravel() for g in gs]) for t in range(nf)]


@functools.lru_cache(maxsize=None)
def _turned_sources(sw, sh, orient, S, nf):
    return [np.stack([orientref.orient_frame(f, sw, sh, orient) for f in step]) for step in _sources(sw, sh, S, nf)]


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


def _run(w, h, br, S, steps, feed, quality=False, prepare=None):
    """one encoder over `steps` (a list of (S, frame bytes) arrays), fed by feed(enc, device frames): per step the NAL
    bytes, rc_state and, with quality on, the records and the reconstructions"""
    import torch
    import h264mi
    enc = h264mi.BatchEncoder(w, h, br, S)
    enc.set_frame_skip(False)
    enc.set_quality(quality)
    if prepare:
        prepare(enc)
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

# (encoder width, height, orientation): 176x144 fed 144x176; 72x40 (coded 80x48, cropped) fed 40x72; 72x40 fed 72x40
ENC_CASES = [(176, 144, orientref.ROT90), (72, 40, orientref.ROT270), (72, 40, orientref.ROT180), (72, 40, orientref.MIRROR),
             (176, 144, orientref.TRANSVERSE)]


@pytest.mark.parametrize('w,h,orient', ENC_CASES, ids=[f'{w}x{h}-{NAMES[o]}' for w, h, o in ENC_CASES])
def test_encode_oriented_equals_encode_of_reference_frames(gpu_lib, w, h, orient):
    S, nf, br = 2, 3, 300000
    sw, sh = orientref.size(orientref.inverse(orient), w, h)
    assert orientref.size(orient, sw, sh) == (w, h)
    src, ref = _sources(sw, sh, S, nf), _turned_sources(sw, sh, orient, S, nf)
    for quality in (False, True):
        got = _run(w, h, br, S, src, lambda e, f: e.encode_oriented(f, orient), quality)
        want = _run(w, h, br, S, ref, lambda e, f: e.encode(f), quality)
        for t in range(nf):
            for s in range(S):
                assert len(got[t]['nal'][s]) > 0
                assert got[t]['nal'][s] == want[t]['nal'][s], f'frame {t} stream {s}: NAL bytes'
                assert got[t]['rc'][s] == want[t]['rc'][s], f'frame {t} stream {s}: rate-control state'
                if quality:
                    q = {k: got[t]['q'][s][k] for k in KEYS}
                    assert q == qualityref.frame_quality(ref[t][s], got[t]['recon'][s], w, h), f'frame {t} stream {s}: records'
                    assert q == {k: want[t]['q'][s][k] for k in KEYS}


def test_encode_oriented_identity(gpu_lib):
    w, h, S, nf = 176, 144, 2, 3
    src = _sources(w, h, S, nf)
    got = _run(w, h, 300000, S, src, lambda e, f: e.encode_oriented(f, orientref.IDENTITY))
    want = _run(w, h, 300000, S, src, lambda e, f: e.encode(f))
    for t in range(nf):
        assert got[t]['nal'] == want[t]['nal'] and got[t]['rc'] == want[t]['rc'], f'frame {t}'


def test_encode_oriented_blends_the_overlays_after_the_turn(gpu_lib):
    """one 16x16 sprite, one placement per stream's canvas 0: encode_oriented of the sources equals encode of the
    reference-turned frames on an encoder that holds the same list"""
    import torch
    import h264mi
    w, h, S, nf, orient = 176, 144, 2, 3, orientref.ROT90
    src, ref = _sources(h, w, S, nf), _turned_sources(h, w, orient, S, nf)
    rng = np.random.default_rng(80)
    sprite = torch.from_numpy(rng.integers(0, 256, h264mi.i420a_bytes(16, 16), dtype=np.uint8)).cuda()
    ov = [h264mi.Overlay(0, 0, 0, 0, 16, 16, 20, 8, 256, 0)]  # off the diagonal: it tells before and after the turn apart

    def prepare(enc):
        enc.set_overlays(sprite, 16, 16, 1, ov)
        assert enc.overlays() == 1

    got = _run(w, h, 300000, S, src, lambda e, f: e.encode_oriented(f, orient), prepare=prepare)
    want = _run(w, h, 300000, S, ref, lambda e, f: e.encode(f), prepare=prepare)
    plain = _run(w, h, 300000, S, ref, lambda e, f: e.encode(f))
    for t in range(nf):
        assert got[t]['nal'] == want[t]['nal'] and got[t]['rc'] == want[t]['rc'], f'frame {t}'
    assert got[0]['nal'][0] != plain[0]['nal'][0], 'the overlay changed nothing: the test shows nothing'


def test_encode_oriented_refusals_leave_the_encoder_untouched(gpu_lib):
    import torch
    w, h, S = 176, 144, 2
    src = _sources(w, h, S, 1)[0]
    fresh = _run(w, h, 300000, S, [src], lambda e, f: e.encode(f))[0]
    other = torch.zeros(S * orientref.frame_bytes(w, h), dtype=torch.uint8, device='cuda')

    def feed(enc, frames):
        fn = enc._L.h264mi_enc_encode_oriented
        p = ctypes.c_void_p(other.data_ptr())
        for bad in (-1, 8, 100):
            assert fn(enc._e, p, bad) == -1, bad
            with pytest.raises(ValueError):
                enc.encode_oriented(other, bad)
        for orient in (orientref.ROT90, orientref.MIRROR):
            assert fn(enc._e, None, orient) == -1
            inp = enc._L.h264mi_enc_input_buffer(enc._e)  # frames that overlap the encoder's input area
            assert fn(enc._e, ctypes.c_void_p(inp), orient) == -1
            assert fn(enc._e, ctypes.c_void_p(inp + S * orientref.frame_bytes(w, h) - 1), orient) == -1
            assert fn(enc._e, ctypes.c_void_p(inp - S * orientref.frame_bytes(w, h) + 1), orient) == -1
        enc.encode(frames)

    got = _run(w, h, 300000, S, [src], feed)[0]
    assert got['nal'] == fresh['nal'] and got['rc'] == fresh['rc']
