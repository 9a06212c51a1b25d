"""GPU: the spatial filter and the privacy masks -- the standalone calls h264mi_i420_spatial_dev and
h264mi_i420_privacy_dev and the encoder's stages h264mi_enc_set_spatial / h264mi_enc_set_privacy -- against
tests/spatialref.py. Exact integers, so every comparison is equality of bytes; every destination sits between 64 guard
bytes of 0xA5 that must stay as they were.

The filter's tile is 256 samples by 32 rows of one plane and its load unit a dword (csrc/spatial.hip); a plane moves as
dwords when its bases and its row length are multiples of 4, else as bytes. The shapes (test_spatial_host.SHAPES, N = 3
frames of different content each): 2x2 (chroma 1x1, every tap clamps), 4x4 and 8x6 (planes narrower than 2r + 1), 16x16,
36x18 (chroma rows of 18 bytes: the byte path), 130x66 (every plane on the byte path; the same at an odd address),
8192x2 and 2x8192 (the limit), 260x34 (luma: one dword past the 256-sample tile across, one even step past the 32-row
tile down) and 520x66 (chroma 260x33: one dword past the tile across and exactly one row past it down)."""
import ctypes
import functools

import numpy as np
import pytest

import denoiseref
import scaleref
import spatialref as ref
from test_spatial_host import BAD_MASKS, BAD_PARAMS, BAD_SHAPES, N, PARAMS, SHAPES, make_frames, privacy_lists

pytestmark = pytest.mark.gpu

GUARD = 64
CASES = [(w, h, 0) for w, h in SHAPES] + [(130, 66, 1)]
CASE_IDS = [f'{w}x{h}' + ('-odd-address' if s else '') for w, h, s in CASES]


@functools.lru_cache(maxsize=None)
def _reference(w, h, params):
    out = np.stack([ref.spatial_frame(f, w, h, params) for f in make_frames(w, h)])
    out.setflags(write=False)
    return out


def _guarded(data, shift=0):
    """(whole, view): data's bytes on the device between 64 bytes of 0xA5 on each side, `shift` bytes into the allocation"""
    import torch
    nbytes = data.size
    whole = torch.full((shift + nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    view = whole[shift + GUARD:shift + GUARD + nbytes]
    view.copy_(torch.from_numpy(np.array(data, dtype=np.uint8).ravel()))
    return whole, view


def _guards_intact(whole, nbytes, shift=0):
    h = whole.cpu().numpy()
    return bool((h[:shift + GUARD] == 0xA5).all() and (h[shift + GUARD + nbytes:] == 0xA5).all())


@pytest.mark.parametrize('w,h,shift', CASES, ids=CASE_IDS)
def test_spatial_vs_reference(gpu_lib, w, h, shift):
    import torch
    import h264mi
    src = make_frames(w, h)
    nb = src.size
    ws, d_src = _guarded(src, shift)
    wd, d_dst = _guarded(np.full(nb, 0x5A, np.uint8), shift)
    if shift:
        assert d_src.data_ptr() % 2 == 1 and d_dst.data_ptr() % 2 == 1
    for params in PARAMS:
        want = _reference(w, h, params)
        d_dst.fill_(0x5A)
        h264mi.i420_spatial(d_dst, d_src, w, h, N, params)
        torch.cuda.synchronize()
        got = d_dst.cpu().numpy().reshape(N, -1)
        for f in range(N):
            assert np.array_equal(got[f], want[f]), f'{params} frame {f}: {int((got[f] != want[f]).sum())} bytes differ'
        assert _guards_intact(wd, nb, shift) and _guards_intact(ws, nb, shift), f'{params}: bytes outside the frames were written'
    assert np.array_equal(d_src.cpu().numpy(), src.ravel()), 'the source frames were written'


def test_spatial_one_frame_and_repeatability(gpu_lib):
    import torch
    import h264mi
    w, h, params = 130, 66, (2, 1, 40, -17, 3)
    src = make_frames(w, h)
    _, d_src = _guarded(src)
    outs = []
    for _ in range(2):
        wd, d_dst = _guarded(np.full(src.size, 0x5A, np.uint8))
        h264mi.i420_spatial(d_dst, d_src, w, h, 1, params)
        torch.cuda.synchronize()
        outs.append(d_dst.cpu().numpy())
        assert _guards_intact(wd, src.size)
    fb = ref.frame_bytes(w, h)
    assert np.array_equal(outs[0][:fb], _reference(w, h, params)[0]) and (outs[0][fb:] == 0x5A).all(), 'n = 1 writes one frame'
    assert outs[0].tobytes() == outs[1].tobytes()


def test_spatial_refusals_write_nothing(gpu_lib):
    import torch
    import h264mi
    fn = gpu_lib.h264mi_i420_spatial_dev
    w, h, n = 32, 16, 3
    nb = n * ref.frame_bytes(w, h)
    wd, d = _guarded(np.full(nb, 0x5A, np.uint8))
    ws, s = _guarded(np.full(nb, 0x33, np.uint8))
    good = ctypes.byref(h264mi.Spatial(1, 1, 40, 40, 0))
    vp = ctypes.c_void_p
    D, S = d.data_ptr(), s.data_ptr()

    def call(dst=D, src=S, ww=w, hh=h, nn=n, par=good):
        return fn(vp(dst) if dst else None, vp(src) if src else None, ww, hh, nn, par, None)

    assert call(dst=0) == -1 and call(src=0) == -1 and call(par=None) == -1
    for ww, hh, nn in BAD_SHAPES:
        assert call(ww=ww, hh=hh, nn=nn) == -1, (ww, hh, nn)
    for bad in BAD_PARAMS:
        assert call(par=ctypes.byref(h264mi.Spatial(*bad))) == -1, bad
        with pytest.raises(ValueError):
            h264mi.i420_spatial(d, s, w, h, n, bad)
    for off in (0, 1, nb - 1, -1, -(nb - 1)):
        assert call(dst=S + off) == -1 and call(src=D + off) == -1, off
    torch.cuda.synchronize()
    assert _guards_intact(wd, nb) and (d.cpu().numpy() == 0x5A).all() and _guards_intact(ws, nb) and (s.cpu().numpy() == 0x33).all(), 'a refused call wrote'
    assert call() == 0
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == 0x33).all() and _guards_intact(wd, nb), 'a flat picture is a fixed point'


LISTS = sorted(privacy_lists(130, 66))


@pytest.mark.parametrize('shift', [0, 1], ids=['aligned', 'odd-address'])
@pytest.mark.parametrize('name', LISTS)
def test_privacy_vs_reference(gpu_lib, name, shift):
    import torch
    import h264mi
    w, h = 130, 66
    src = make_frames(w, h)
    masks = privacy_lists(w, h)[name]
    want = ref.privacy_frames(src, w, h, masks)
    whole, d = _guarded(src, shift)
    assert not shift or d.data_ptr() % 2 == 1
    h264mi.i420_privacy(d, w, h, N, masks)
    torch.cuda.synchronize()
    got = d.cpu().numpy().reshape(N, -1)
    assert np.array_equal(got, want), f'{int((got != want).sum())} bytes differ'
    assert _guards_intact(whole, src.size, shift)
    outside = np.ones_like(got, bool)
    for f, x, y, mw, mh, *_ in masks:
        for pl, plane in enumerate(ref.planes(outside[f], w, h)):
            s = 1 if pl else 0
            plane[y >> s:(y + mh) >> s, x >> s:(x + mw) >> s] = False
    assert outside.any() and np.array_equal(got[outside], src[outside]), 'samples outside the rectangles changed'
    h264mi.i420_privacy(d, w, h, N, masks)  # idempotent on the device too
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().reshape(N, -1), want)


def test_privacy_more_masks_than_one_launch_holds(gpu_lib):
    """130 masks of 8x8 on three frames: three launches of at most 64"""
    import torch
    import h264mi
    w, h = 130, 66
    src = make_frames(w, h)
    masks = [(k % N, 8 * (k % 16), 8 * (k // 16), 8, 8, ref.PIXELATE if k % 3 else ref.FILL, 4, k, 255 - k, 7) for k in range(130) if 8 * (k // 16) + 8 <= h]
    assert len(masks) > 64 and ref.masks_ok(masks, w, h, N)
    whole, d = _guarded(src)
    h264mi.i420_privacy(d, w, h, N, masks)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().reshape(N, -1), ref.privacy_frames(src, w, h, masks)) and _guards_intact(whole, src.size)


def test_privacy_refusals_write_nothing(gpu_lib):
    import torch
    import h264mi
    w, h, n = 32, 16, 2
    nb = n * ref.frame_bytes(w, h)
    whole, d = _guarded(np.full(nb, 0x5A, np.uint8))
    for masks in BAD_MASKS:  # the overlapping lists among them
        with pytest.raises(ValueError):
            h264mi.i420_privacy(d, w, h, n, masks)
    with pytest.raises(ValueError):
        h264mi.i420_privacy(d, w, h, n, [])
    with pytest.raises(ValueError):
        h264mi.i420_privacy(d, w - 1, h, n, [(0, 0, 0, 4, 4, ref.FILL, 0, 1, 2, 3)])
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == 0x5A).all() and _guards_intact(whole, nb), 'a refused call wrote'


# ---------------------------------------------------------------- the encoder's stages

SP = (1, 2, 40, -17, 2)
KEYS = ('sse', 'ssim_fix', 'windows', 'coded')
ENC_CASES = [(176, 144, 2), (72, 40, 1)]  # 72x40 is coded 80x48 and cropped
ENC_IDS = ['176x144-S2', '72x40-S1']
NF = 6


def _masks(w, h, S):
    """per stream a pixelated rectangle with partial cells over the moving square's path and a filled one"""
    out = []
    for s in range(S):
        out += [(s, 4, 4 + 4 * s, 42, 22, ref.PIXELATE, 8, 0, 0, 0), (s, w - 20, h - 12, 20, 12, ref.FILL, 0, 30 + s, 120, 140)]
    return out


@functools.lru_cache(maxsize=None)
def _scene(w, h, S, nf):
    """nf steps of S frames: a textured scene per stream plus seeded noise, a 16x16 square moving 8 samples a frame"""
    rng = np.random.default_rng(23 * w + h + S)
    steps = []
    yy, xx = np.mgrid[0:h, 0:w]
    for t in range(nf):
        fr = []
        for s in range(S):
            Y = (64 + (xx * 2 + yy * 3 + 40 * s) % 128 + 24 * ((xx // 4 + yy // 4) & 1)).astype(np.int32)
            U = (110 + 10 * s + 6 * ((xx[:h // 2, :w // 2] // 3) & 1)).astype(np.int32)
            V = np.full((h // 2, w // 2), 140 - 10 * s, np.int32)
            x0, y0 = 8 + 8 * t, 8 + 4 * s
            Y[y0:y0 + 16, x0:x0 + 16] = 230
            U[y0 // 2:y0 // 2 + 8, x0 // 2:x0 // 2 + 8] = 60
            f = np.concatenate([Y.ravel(), U.ravel(), V.ravel()])
            fr.append(np.clip(f + np.rint(rng.normal(0, 2, f.size)).astype(np.int32), 0, 255).astype(np.uint8))
        steps.append(np.stack(fr))
    return steps


def _staged(steps, w, h, params=SP, masks=None):
    """the steps as the two stages leave them: the filter, then the masks"""
    out = []
    for st in steps:
        fr = np.stack([ref.spatial_frame(f, w, h, params) for f in st]) if params else np.array(st)
        out.append(ref.privacy_frames(fr, w, h, masks) if masks else fr)
    return out


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


def _run(w, h, S, steps, feed=None, quality=False, prepare=None, before=None):
    """one encoder over `steps`, fed by feed(enc, device frames) (default: encode), before(enc, t) in front of step t:
    per step the NAL bytes, rc_state and, with quality on, the records and the reconstructions"""
    import torch
    import h264mi
    enc = h264mi.BatchEncoder(w, h, 300000, S)
    enc.set_frame_skip(False)
    enc.set_quality(quality)
    if prepare:
        prepare(enc)
    out = []
    for t, fr in enumerate(steps):
        if before:
            before(enc, t)
        frames = torch.from_numpy(np.ascontiguousarray(fr).ravel()).cuda()  # held until nal_sizes() has synchronised
        (feed or (lambda e, f: e.encode(f)))(enc, frames)
        sizes = enc.nal_sizes()
        st = {'nal': [enc.nal_bytes(s, sizes[s]) for s in range(S)], 'rc': [enc.rc_state(s) for s in range(S)]}
        assert all(len(b) > 0 for b in st['nal'])
        assert np.array_equal(frames.cpu().numpy(), np.ascontiguousarray(fr).ravel()), "the caller's frames were written"
        if quality:
            st['q'] = [enc.quality(s) for s in range(S)]
            st['recon'] = [_recon(enc, s) for s in range(S)]
        out.append(st)
    enc.close()
    return out


def _same(got, want, what=''):
    assert len(got) == len(want)
    for t in range(len(want)):
        assert got[t]['nal'] == want[t]['nal'], f'{what} frame {t}: NAL bytes'
        assert got[t]['rc'] == want[t]['rc'], f'{what} frame {t}: rate-control state'


def _on(w, h, S, spatial=True, privacy=True):
    def prepare(enc):
        if spatial:
            enc.set_spatial(SP)
            p = enc.spatial()
            assert p is not None and (p.radius_y, p.radius_c, p.amount_y, p.amount_c, p.core) == SP
        if privacy:
            enc.set_privacy(_masks(w, h, S))
            assert enc.privacy() == 2 * S
    return prepare


@pytest.mark.parametrize('w,h,S', ENC_CASES, ids=ENC_IDS)
def test_encoder_equals_encode_of_reference_frames(gpu_lib, w, h, S):
    import qualityref
    raw = _scene(w, h, S, NF)
    masks = _masks(w, h, S)
    staged = _staged(raw, w, h, SP, masks)
    assert not np.array_equal(staged[0], raw[0])
    for quality in (False, True):
        got = _run(w, h, S, raw, quality=quality, prepare=_on(w, h, S))
        want = _run(w, h, S, staged, quality=quality)
        _same(got, want)
        if quality:
            for t in range(NF):
                for s in range(S):
                    q = {k: got[t]['q'][s][k] for k in KEYS}
                    assert q == qualityref.frame_quality(staged[t][s], got[t]['recon'][s], w, h), f'frame {t} stream {s}: records compare what was coded'
                    assert q == {k: want[t]['q'][s][k] for k in KEYS}
    plain = _run(w, h, S, raw)
    assert got[0]['nal'] != plain[0]['nal'], 'the stages changed nothing: the test shows nothing'
    # each stage alone
    _same(_run(w, h, S, raw, prepare=_on(w, h, S, privacy=False)), _run(w, h, S, _staged(raw, w, h, SP, None)), 'filter alone')
    _same(_run(w, h, S, raw, prepare=_on(w, h, S, spatial=False)), _run(w, h, S, _staged(raw, w, h, None, masks)), 'masks alone')


@pytest.mark.parametrize('w,h,S', ENC_CASES, ids=ENC_IDS)
def test_encoder_through_the_scaled_entry_point(gpu_lib, w, h, S):
    """sharpen-after-downscale: encode_scaled from twice the size with the stages on"""
    big = _scene(2 * w, 2 * h, S, NF)
    small = [np.stack([scaleref.scale_frame(f, 2 * w, 2 * h, w, h) for f in st]) for st in big]
    got = _run(w, h, S, big, feed=lambda e, f: e.encode_scaled(f, 2 * w, 2 * h), prepare=_on(w, h, S))
    _same(got, _run(w, h, S, _staged(small, w, h, SP, _masks(w, h, S))))


def test_encoder_order_with_the_denoiser_and_a_sprite(gpu_lib):
    """denoise, filter, mask, blend: the denoiser's state never holds a sharpened or masked frame, the label lies over the mask"""
    import torch
    import h264mi
    w, h, S = 176, 144, 2
    DN = (128, 64, 12, 24)
    raw = _scene(w, h, S, NF)
    masks = _masks(w, h, S)
    sprite = torch.from_numpy(np.random.default_rng(93).integers(0, 256, h264mi.i420a_bytes(16, 16), dtype=np.uint8)).cuda()
    ov = [h264mi.Overlay(0, s, 0, 0, 16, 16, 40, 20, 256, 0) for s in range(S)]  # inside the pixelated rectangle

    def sprites(enc):
        enc.set_overlays(sprite, 16, 16, 1, ov)

    def everything(enc):
        sprites(enc)
        enc.set_denoise(DN)
        _on(w, h, S)(enc)

    per = [denoiseref.denoise_sequence([st[s] for st in raw], w, h, DN)[0] for s in range(S)]
    clean = [np.stack([per[s][t] for s in range(S)]) for t in range(NF)]
    assert not np.array_equal(clean[2], raw[2])
    got = _run(w, h, S, raw, prepare=everything)
    want = _run(w, h, S, _staged(clean, w, h, SP, masks), prepare=sprites)
    _same(got, want)
    assert got[2]['nal'] != _run(w, h, S, _staged(clean, w, h, SP, masks))[2]['nal'], 'the overlay changed nothing'


@pytest.mark.parametrize('w,h,S', ENC_CASES, ids=ENC_IDS)
def test_encoder_off_on_and_refused_settings(gpu_lib, w, h, S):
    """on for frames 0-1, both off for 2-3 (an inert setting and an empty list), other settings for 4-5; refused
    settings in between leave the ones in force"""
    import h264mi
    raw = _scene(w, h, S, NF)
    masks = _masks(w, h, S)
    SP2, masks2 = (3, 1, -64, 255, 0), [(S - 1, 0, 0, w, h, ref.PIXELATE, 64, 0, 0, 0)]

    def refuse(enc):
        for bad in BAD_PARAMS:
            with pytest.raises(ValueError):
                enc.set_spatial(bad)
            assert enc._L.h264mi_enc_set_spatial(enc._e, ctypes.byref(h264mi.Spatial(*bad))) == -1
        for bad in ([(S, 0, 0, 4, 4, ref.FILL, 0, 1, 2, 3)], [(0, 0, 0, w + 2, 4, ref.FILL, 0, 1, 2, 3)], masks + [masks[0]]):
            with pytest.raises(ValueError):
                enc.set_privacy(bad)

    def before(enc, t):
        if t == 0:
            refuse(enc)
            assert enc.spatial() is None and enc.privacy() == 0
            _on(w, h, S)(enc)
        if t == 2:
            enc.set_spatial((0, 2, 40, 0, 9))  # inert: off
            enc.set_privacy([])
            assert enc.spatial() is None and enc.privacy() == 0 and enc._L.h264mi_enc_spatial(enc._e, None) == 0
        if t == 3:
            enc.set_spatial(None)
            enc.set_privacy(None)
        if t == 4:
            enc.set_spatial(SP2)
            enc.set_privacy(masks2)
        before_refusal = (enc.spatial(), enc.privacy())
        refuse(enc)
        after = (enc.spatial(), enc.privacy())
        assert repr(before_refusal) == repr(after)

    want = _run(w, h, S, _staged(raw[:2], w, h, SP, masks) + raw[2:4] + _staged(raw[4:], w, h, SP2, masks2))
    _same(_run(w, h, S, raw, before=before), want)


def test_both_stages_off_is_the_plain_encoder(gpu_lib):
    w, h, S = 72, 40, 1
    raw = _scene(w, h, S, 3)

    def off(enc):
        enc.set_spatial(None)
        enc.set_spatial((2, 2, 0, 0, 0))
        enc.set_privacy([])
        assert enc.spatial() is None and enc.privacy() == 0

    _same(_run(w, h, S, raw, prepare=off), _run(w, h, S, raw))
