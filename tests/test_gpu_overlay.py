"""GPU: alpha-blended overlays -- h264mi_i420_overlay_dev, h264mi_rgba_to_i420a_dev and the encoder's overlay list
h264mi_enc_set_overlays -- against tests/overlayref.py. The definition is exact integer arithmetic, so every
comparison is equality of bytes. Every canvas is pre-filled with a seeded random pattern, so an untouched byte is
provable, and sits between 64 guard bytes of 0xA5 that must stay as they were."""
import ctypes
import functools

import numpy as np
import pytest

import overlayref
import qualityref
import scaleref
from overlayref import O
from test_gpu_compose import _cells, _composed_sources, _gallery
from test_gpu_scale import KEYS, _device, _guarded, _guards_intact, _run, _scaled_sources, _sources

pytestmark = pytest.mark.gpu

PER_LAUNCH = 64  # H264MI_OVERLAY_PER_LAUNCH (include/h264mi.h)


def _frames(w, h, n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, scaleref.frame_bytes(w, h)), dtype=np.uint8)


def _sprites(w, h, n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, overlayref.sprite_bytes(w, h)), dtype=np.uint8)


def _ovs(overlays):
    import h264mi
    return [h264mi.Overlay(*overlayref.as_tuple(p)) for p in overlays]


def _outside(cw, ch, ncanvas, overlays):
    """a (ncanvas, frame bytes) mask of the bytes no placement covers"""
    m = np.ones((ncanvas, scaleref.frame_bytes(cw, ch)), np.uint8)  # uint8: scaleref.planes gives views of it
    for p in overlays:
        for k, plane in enumerate(scaleref.planes(m[p.canvas], cw, ch)):
            s = 1 if k else 0
            plane[p.dy >> s:(p.dy + p.h) >> s, p.dx >> s:(p.dx + p.w) >> s] = 0
    return m != 0


def _overlay(pattern, cw, ch, sprites, ow, oh, overlays, cshift=0, sshift=0):
    """the standalone call: canvases pre-filled with `pattern` (an (ncanvas, frame bytes) array), `sprites` an
    (nsprites, sprite bytes) array, each `shift` bytes into its allocation; the canvases as an array, guards checked"""
    import torch
    import h264mi
    ncanvas, cfb = pattern.shape
    d_spr = _device(sprites, sshift)
    whole, dst = _guarded(ncanvas * cfb, cshift)
    dst.copy_(torch.from_numpy(np.ascontiguousarray(pattern).ravel()))
    assert d_spr.data_ptr() % 2 == sshift and dst.data_ptr() % 2 == cshift
    h264mi.i420_overlay(dst, cw, ch, ncanvas, d_spr, ow, oh, len(sprites), _ovs(overlays))
    out = dst.cpu().numpy().reshape(ncanvas, cfb)
    assert _guards_intact(whole, ncanvas * cfb, cshift), 'bytes outside the canvases were written'
    assert np.array_equal(d_spr.cpu().numpy().reshape(sprites.shape), sprites), 'the sprites were written'
    return out


def _check(pattern, cw, ch, sprites, ow, oh, overlays, cshift=0, sshift=0):
    got = _overlay(pattern, cw, ch, sprites, ow, oh, overlays, cshift, sshift)
    want = overlayref.blend(pattern, cw, ch, sprites, ow, oh, overlays)
    out = _outside(cw, ch, len(pattern), overlays)
    assert np.array_equal(got[out], pattern[out]), 'bytes outside the rectangles were changed'
    for c in range(len(pattern)):
        assert np.array_equal(got[c], want[c]), f'canvas {c}: {int((got[c] != want[c]).sum())} bytes differ'
    return got, want


def _with_alpha(sprites, w, h, value):
    out = sprites.copy()
    out[:, scaleref.frame_bytes(w, h):] = value
    return out


def test_opaque_whole_sprite_gives_the_sprites_i420_bytes(gpu_lib):
    spr = _with_alpha(_sprites(32, 32, 1, 4000), 32, 32, 255)
    got, _ = _check(_frames(32, 32, 1, 4001), 32, 32, spr, 32, 32, [O(0, 0, 0, 0, 32, 32, 0, 0, 256)])
    assert np.array_equal(got[0], spr[0][:scaleref.frame_bytes(32, 32)])


@pytest.mark.parametrize('cshift,sshift', [(0, 0), (1, 0), (0, 1), (1, 1)], ids=['aligned', 'odd-canvas', 'odd-sprites', 'both-odd'])
def test_odd_pitches_and_addresses(gpu_lib, cshift, sshift):
    """38x22 sprites (chroma pitch 19) on 50x26 canvases (chroma pitch 25): a row's alignment changes from row to row in
    every plane of both; two sprites and two canvases, so frames start at every residue too"""
    ovs = [O(1, 1, 6, 2, 26, 18, 10, 4, 256), O(0, 0, 6, 2, 26, 18, 10, 4, 181)]
    _check(_frames(50, 26, 2, 4010), 50, 26, _sprites(38, 22, 2, 4011), 38, 22, ovs, cshift, sshift)


E = (0, 1, 127, 128, 254, 255)


def test_extremes(gpu_lib):
    """every (alpha, sprite sample, canvas sample) of {0, 1, 127, 128, 254, 255}^3 in luma -- the sprite's 36 columns
    are the (alpha, sample) pairs, the canvas's 6 rows the canvas values --, chroma planes from the same set, at
    opacities 0, 1, 128, 255, 256: one placement of the one sprite on each of 5 canvases"""
    w, h = 36, 6
    a = np.repeat(np.array(E, np.uint8), 6)[None, :].repeat(h, 0)
    s = np.tile(np.array(E, np.uint8), 6)[None, :].repeat(h, 0)
    rng = np.random.default_rng(4020)
    spr = overlayref.make_sprite(s, rng.choice(E, (h // 2, w // 2)), rng.choice(E, (h // 2, w // 2)), a)[None]
    canvas = np.concatenate([np.repeat(np.array(E, np.uint8), w), rng.choice(E, 2 * (w // 2) * (h // 2)).astype(np.uint8)])
    pattern = np.tile(canvas, (5, 1))
    triples = {(int(a[r, c]), int(s[r, c]), int(scaleref.planes(canvas, w, h)[0][r, c])) for r in range(h) for c in range(w)}
    assert len(triples) == 216
    ovs = [O(0, k, 0, 0, w, h, 0, 0, op) for k, op in enumerate((0, 1, 128, 255, 256))]
    got, _ = _check(pattern, w, h, spr, w, h, ovs)
    assert np.array_equal(got[0], pattern[0]), 'opacity 0'


@pytest.mark.parametrize('cw', [176, 178, 182])
def test_several_strips_and_row_segments(gpu_lib, cw):
    """a 150x100 placement at dx = 14: three column strips (the last 22 wide), seven row segments (the last 4 rows);
    canvas widths 178 and 182 (chroma 89 and 91) make a row's store alignment vary"""
    _check(_frames(cw, 144, 1, 4030 + cw), cw, 144, _sprites(160, 120, 1, 4031), 160, 120, [O(0, 0, 4, 10, 150, 100, 14, 22, 256)])


def test_overlap_in_one_call(gpu_lib):
    """three mutually overlapping placements on one canvas and a fourth that touches none of them. Expected launch
    split, in list order: [a, d] (d is disjoint from a and joins its launch), then [b] (shares samples with a), then
    [c] (shares samples with b); reversed: [c, d], [b], [a]. Stream order is list order, so the last is on top"""
    cw, ch = 64, 48
    pattern, spr = _frames(cw, ch, 1, 4040), _sprites(32, 32, 3, 4041)
    a, b, c = O(0, 0, 0, 0, 32, 32, 2, 2, 256), O(1, 0, 0, 0, 32, 32, 12, 8, 150), O(2, 0, 2, 4, 30, 28, 20, 14, 256)
    d = O(1, 0, 10, 10, 8, 8, 54, 38, 99)
    _, fwd = _check(pattern, cw, ch, spr, 32, 32, [a, d, b, c])
    _, rev = _check(pattern, cw, ch, spr, 32, 32, [c, d, b, a])
    assert not np.array_equal(fwd, rev)
    y = scaleref.planes(fwd[0] != rev[0], cw, ch)[0]
    assert not y[38:46, 54:62].any(), 'the disjoint placement is the same either way'


def test_overlap_across_the_capacity_boundary(gpu_lib):
    """PER_LAUNCH disjoint 4x4 placements fill a launch; one more lies over the first and over the one before it.
    Expected split: [0 .. 63] (full), then [64] -- which must see both of them done"""
    cw = ch = 64
    slots = list(range(PER_LAUNCH))
    slots[1], slots[PER_LAUNCH - 1] = slots[PER_LAUNCH - 1], slots[1]  # the last of the launch sits beside the first
    ovs = [O(k % 2, 0, 2 * (k % 7), 2 * (k % 5), 4, 4, 4 * (s % 16), 4 * (s // 16), 256 - 3 * k) for k, s in enumerate(slots)]
    ovs.append(O(0, 0, 8, 8, 4, 4, 2, 0, 140))  # columns 2..5: two of placement 0's, two of placement 63's
    assert len(ovs) == PER_LAUNCH + 1 and (ovs[0].dx, ovs[0].dy, ovs[-2].dx, ovs[-2].dy) == (0, 0, 4, 0)
    _, want = _check(_frames(cw, ch, 1, 4050), cw, ch, _sprites(16, 16, 2, 4051), 16, 16, ovs)
    assert not np.array_equal(want, overlayref.blend(_frames(cw, ch, 1, 4050), cw, ch, _sprites(16, 16, 2, 4051), 16, 16, ovs[-1:] + ovs[:-1]))


def test_fan_out(gpu_lib):
    """one sprite to each of 5 canvases at different positions and opacities, and two sprites to one canvas"""
    ovs = [O(0, k, 2 * k, 0, 20, 12, 4 * k, 2 * k, 256 - 50 * k) for k in range(5)] + [O(1, 3, 0, 0, 24, 16, 22, 14, 200)]
    _check(_frames(48, 32, 5, 4060), 48, 32, _sprites(32, 16, 2, 4061), 32, 16, ovs)


@pytest.mark.parametrize('w,h,n', [(38, 22, 3), (32, 32, 1)], ids=['38x22x3', '32x32'])
def test_rgba_to_i420a(gpu_lib, w, h, n):
    import torch
    import h264mi
    rgba = np.random.default_rng(4070 + w).integers(0, 256, (n, h * w * 4), dtype=np.uint8)
    d_rgba = _device(rgba)
    sb, fb = overlayref.sprite_bytes(w, h), scaleref.frame_bytes(w, h)
    whole, dst = _guarded(n * sb)
    h264mi.rgba_to_i420a(dst, d_rgba, w, h, n)
    i420 = torch.zeros(n * fb, dtype=torch.uint8, device='cuda')
    h264mi.rgba_to_i420(i420, d_rgba, w, h, n)
    got, plain = dst.cpu().numpy().reshape(n, sb), i420.cpu().numpy().reshape(n, fb)
    assert _guards_intact(whole, n * sb)
    for f in range(n):
        assert np.array_equal(got[f][:fb], plain[f]), f'sprite {f}: Y, Cb, Cr are the conversion\'s'
        assert np.array_equal(got[f][fb:], rgba[f].reshape(h * w, 4)[:, 3]), f'sprite {f}: A is the fourth byte'
        assert np.array_equal(got[f], overlayref.rgba_to_i420a(rgba[f], w, h))
    # the result feeds the blend as it lies
    pattern = _frames(48, 40, 1, 4071)
    cfb = scaleref.frame_bytes(48, 40)
    cwhole, canvas = _guarded(cfb)
    canvas.copy_(torch.from_numpy(pattern.ravel()))
    ovs = [O(n - 1, 0, 2, 2, 28, 18, 6, 4, 230)]
    h264mi.i420_overlay(canvas, 48, 40, 1, dst, w, h, n, _ovs(ovs))
    assert np.array_equal(canvas.cpu().numpy(), overlayref.blend(pattern, 48, 40, got, w, h, ovs)[0])
    assert _guards_intact(cwhole, cfb)


def test_repeatability(gpu_lib):
    pattern, spr = _frames(178, 144, 1, 4080), _sprites(160, 120, 1, 4081)
    ovs = [O(0, 0, 4, 10, 150, 100, 14, 22, 201), O(0, 0, 0, 0, 64, 64, 100, 70, 256)]
    a = _overlay(pattern, 178, 144, spr, 160, 120, ovs)
    b = _overlay(pattern, 178, 144, spr, 160, 120, ovs)
    assert a.tobytes() == b.tobytes()


def test_standalone_bad_arguments(gpu_lib):
    import torch
    import h264mi
    from test_overlay_host import BAD, OK
    fn = gpu_lib.h264mi_i420_overlay_dev
    s = torch.zeros(3 * 2560, dtype=torch.uint8, device='cuda')
    pattern = _frames(32, 32, 2, 4090)
    whole, d = _guarded(2 * 1536)
    d.copy_(torch.from_numpy(pattern.ravel()))
    ps, pd = ctypes.c_void_p(s.data_ptr()), ctypes.c_void_p(d.data_ptr())
    one = (h264mi.Overlay * 1)(h264mi.Overlay(*OK))
    for cw, ch, ncanvas, ow, oh, nspr, ovs in BAD:
        arr = (h264mi.Overlay * len(ovs))(*[h264mi.Overlay(*t) for t in ovs]) if ovs else one
        assert fn(pd, cw, ch, ncanvas, ps, ow, oh, nspr, arr, len(ovs), None) == -1, (cw, ch, ncanvas, ow, oh, nspr, ovs)
    assert fn(None, 32, 32, 1, ps, 32, 32, 1, one, 1, None) == -1 and fn(pd, 32, 32, 1, None, 32, 32, 1, one, 1, None) == -1
    for off in (0, 1, 2559, 3 * 2560 - 1):  # the canvas inside the sprites
        assert fn(ctypes.c_void_p(s.data_ptr() + off), 32, 32, 1, ps, 32, 32, 3, one, 1, None) == -1
    with pytest.raises(ValueError):
        h264mi.i420_overlay(d, 32, 32, 2, s, 32, 32, 3, [h264mi.Overlay(*OK), h264mi.Overlay(0, 0, 0, 0, 16, 16, 0, 0, 257, 0)])
    with pytest.raises(ValueError):
        h264mi.i420_overlay(d, 32, 32, 2, s, 32, 32, 3, [])
    with pytest.raises(ValueError):
        h264mi.rgba_to_i420a(s, d, 31, 16, 1)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), pattern.ravel()), 'a refused call changed the canvas'
    assert _guards_intact(whole, 2 * 1536)
    assert fn(pd, 32, 32, 1, ps, 32, 32, 1, one, 1, None) == 0  # and a good call goes through: alpha 0, nothing changes
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), pattern.ravel())


# ---------------------------------------------------------------- the encoder's overlay list

W, H, BR, S, NF = 176, 144, 300000, 2, 3
LW, LH = 64, 32
# a semi-transparent logo on both streams and, on stream 1, a label that lies over part of the logo
LIST = [O(0, 0, 0, 0, 48, 32, 120, 8, 160), O(0, 1, 0, 0, 48, 32, 120, 8, 160), O(1, 1, 4, 2, 60, 20, 100, 30, 256)]
LAYOUT, BG = ((0, 1, 2), (2, 4, 3)), (40, 100, 200)


@functools.lru_cache(maxsize=None)
def _logo_sprites():
    rng = np.random.default_rng(4100)
    out = []
    for k in range(2):
        y = (np.add.outer(np.arange(LH), np.arange(LW)) * (3 + k) % 256).astype(np.uint8)
        a = rng.integers(0, 256, (LH, LW), dtype=np.uint8)
        a[:, :LW // 2] = 255 if k else 90
        out.append(overlayref.make_sprite(y, rng.integers(0, 256, (LH // 2, LW // 2)), rng.integers(0, 256, (LH // 2, LW // 2)), a))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def _rgba_sources():
    rng = np.random.default_rng(4101)
    base = rng.integers(0, 256, (S, H // 8, W // 8, 4), dtype=np.uint8).repeat(8, 1).repeat(8, 2)
    return [np.stack([np.roll(base[s], 2 * t, 1).ravel() for s in range(S)]) for t in range(NF)]


@functools.lru_cache(maxsize=None)
def _path(path):
    """(what the encoder is fed per step, the frames it should code per step: the path's input with LIST blended on)"""
    if path == 'encode':
        src = plain = _sources(W, H, S, NF)
    elif path == 'encode_rgba':
        src = _rgba_sources()
        plain = [np.stack([overlayref.rgba_to_i420a(f, W, H)[:scaleref.frame_bytes(W, H)] for f in step]) for step in src]
    elif path == 'encode_scaled':
        src, plain = _sources(352, 288, S, NF), _scaled_sources(352, 288, W, H, S, NF)
    else:
        src, plain = _sources(W, H, 5, NF), _composed_sources(LAYOUT, BG, NF)
    return src, [overlayref.blend(step, W, H, _logo_sprites(), LW, LH, LIST) for step in plain]


def _feeder(path, d_spr):
    cells = _cells(_gallery(LAYOUT))

    def feed(enc, frames):
        import torch
        if enc.overlays() == 0:
            enc.set_overlays(d_spr, LW, LH, 2, _ovs(LIST))
            assert enc.overlays() == len(LIST)
        if path == 'encode':
            before = frames.clone()
            enc.encode(frames)
            torch.cuda.synchronize()
            assert torch.equal(frames, before), 'encode() with overlays changed the caller\'s frames'
        elif path == 'encode_rgba':
            enc.encode_rgba(frames)
        elif path == 'encode_scaled':
            enc.encode_scaled(frames, 352, 288)
        else:
            enc.encode_composed(frames, W, H, 5, cells, bg=BG)
    return feed


@pytest.mark.parametrize('path', ['encode', 'encode_rgba', 'encode_scaled', 'encode_composed'])
def test_every_frame_step_equals_encode_of_reference_frames(gpu_lib, path):
    src, ref = _path(path)
    assert not np.array_equal(ref[0][1], ref[0][0])
    d_spr = _device(_logo_sprites())
    for quality in (False, True):
        got = _run(W, H, BR, S, src, _feeder(path, d_spr), quality)
        want = _run(W, H, BR, S, ref, lambda e, f: e.encode(f), quality)
        for t in range(NF):
            for s in range(S):
                assert len(got[t]['nal'][s]) > 0
                assert got[t]['nal'][s] == want[t]['nal'][s], f'frame {t} stream {s}: NAL bytes'
                assert got[t]['rc'][s] == want[t]['rc'][s], f'frame {t} stream {s}: rate-control state'
                if quality:
                    q = {k: got[t]['q'][s][k] for k in KEYS}
                    assert q == qualityref.frame_quality(ref[t][s], got[t]['recon'][s], W, H), f'frame {t} stream {s}: records'
                    assert q == {k: want[t]['q'][s][k] for k in KEYS}


def test_clear_and_refused_set_and_the_input_buffer(gpu_lib):
    """frame 0 with the list; a refused set_overlays, then frame 1 still with the list and fed from the input buffer
    itself; clear_overlays, then frame 2 plain: all three equal an encoder fed those frames through plain encode"""
    import torch
    import h264mi
    src, ref = _path('encode')
    fb = scaleref.frame_bytes(W, H)
    d_spr = _device(_logo_sprites())
    hip = h264mi._hiprt()
    hip.hipMemcpyAsync.restype = ctypes.c_int
    step = [0]

    def feed(enc, frames):
        t = step[0]
        step[0] += 1
        L, inp = enc._L, enc._L.h264mi_enc_input_buffer(enc._e)
        if t == 0:
            assert enc.overlays() == 0
            enc.set_overlays(d_spr, LW, LH, 2, _ovs(LIST))
            enc.encode(frames)
        elif t == 1:
            for bad in ([LIST[0]._replace(canvas=2)], [LIST[0]._replace(opacity=257)], [LIST[0]._replace(dx=121)], [LIST[0]._replace(w=66)]):
                with pytest.raises(ValueError):
                    enc.set_overlays(d_spr, LW, LH, 2, _ovs(bad))
            arr = (h264mi.Overlay * 1)(*_ovs(LIST[:1]))
            for ptr in (inp, inp + S * fb - 1, inp - 2 * overlayref.sprite_bytes(LW, LH) + 1):  # sprites inside the input area
                assert L.h264mi_enc_set_overlays(enc._e, ctypes.c_void_p(ptr), LW, LH, 2, arr, 1) == -1
            assert L.h264mi_enc_set_overlays(enc._e, None, LW, LH, 2, arr, 1) == -1
            assert enc.overlays() == len(LIST), 'a refused call replaced the list'
            for ptr in (inp + 1, inp - 1, inp + S * fb - 1, inp - S * fb + 1):  # frames partly inside the input area
                assert L.h264mi_enc_encode(enc._e, ctypes.c_void_p(ptr)) == -1
            torch.cuda.synchronize()
            # a device-to-device hipMemcpy does not wait for the device, and the encoder's own stream does not wait for the
            # null stream: the frames go into the input area on the encoder's stream, as its producers' work does
            assert hip.hipMemcpyAsync(ctypes.c_void_p(inp), ctypes.c_void_p(frames.data_ptr()), ctypes.c_size_t(S * fb), 3,
                                      ctypes.c_void_p(L.h264mi_enc_stream(enc._e))) == 0
            assert L.h264mi_enc_encode(enc._e, ctypes.c_void_p(inp)) == 0
        else:
            enc.clear_overlays()
            assert enc.overlays() == 0
            enc.encode(frames)

    got = _run(W, H, BR, S, src, feed)
    want = _run(W, H, BR, S, [ref[0], ref[1], src[2]], lambda e, f: e.encode(f))
    plain = _run(W, H, BR, S, [src[0]], lambda e, f: e.encode(f))
    assert got[0]['nal'] != plain[0]['nal'], 'the list changed nothing'
    for t in range(NF):
        assert got[t]['nal'] == want[t]['nal'] and got[t]['rc'] == want[t]['rc'], f'frame {t}'


def test_decode_compose_label_encode(gpu_lib):
    """two streams encoded for 2 frames, decoded with frames out, composed side by side into a third encoder's input
    and labelled there through its overlay list with sprites made by rgba_to_i420a; its NAL bytes decode on a fresh
    decoder"""
    import torch
    import h264mi
    from composeref import C, compose, fill
    nf, fb = 2, scaleref.frame_bytes(W, H)
    enc = h264mi.BatchEncoder(W, H, BR, S)
    enc.set_frame_skip(False)
    dec = h264mi.BatchDecoder(W, H, S)
    mix = h264mi.BatchEncoder(W, H, BR, 1)
    mix.set_frame_skip(False)
    view = h264mi.BatchDecoder(W, H, 1)
    rgba = np.zeros((2, 16, 64, 4), np.uint8)  # two labels: a colour bar each, opaque with a faded right end
    rgba[0, ..., 0], rgba[1, ..., 2] = 230, 230
    rgba[..., 3] = np.minimum(255, 8 * np.arange(64)[::-1])[None, None, :]
    d_spr = torch.zeros(2 * h264mi.i420a_bytes(64, 16), dtype=torch.uint8, device='cuda')
    h264mi.rgba_to_i420a(d_spr, _device(rgba), 64, 16, 2)
    torch.cuda.synchronize()  # made on the current stream, read on the encoder's own
    labels = [O(0, 0, 0, 0, 64, 16, 12, 92, 256), O(1, 0, 0, 0, 64, 16, 100, 92, 256)]
    mix.set_overlays(d_spr, 64, 16, 2, _ovs(labels))
    decoded = torch.zeros(S * fb, dtype=torch.uint8, device='cuda')
    got = torch.zeros(S, dtype=torch.int32, device='cuda')
    shown = torch.zeros(fb, dtype=torch.uint8, device='cuda')
    shown_got = torch.zeros(1, dtype=torch.int32, device='cuda')
    cells = [C(0, 0, 0, 0, W, H, 0, 36, 88, 72), C(1, 0, 0, 0, W, H, 88, 36, 88, 72)]
    bg = (16, 128, 128)
    for step in _sources(W, H, S, nf):
        frames = torch.from_numpy(np.ascontiguousarray(step).ravel()).cuda()
        enc.encode(frames)
        sizes = enc.nal_sizes()  # synchronises
        assert all(n > 0 for n in sizes)
        got.zero_()
        dec.decode_frames(enc.nal_ptrs(), nal_sizes=sizes, out_ptrs=[decoded[s * fb:].data_ptr() for s in range(S)],
                          got_ptrs=[got[s:s + 1].data_ptr() for s in range(S)])
        torch.cuda.synchronize()
        assert dec.status()[0] == 0 and got.cpu().tolist() == [1] * S
        mix.encode_composed(decoded, W, H, S, _cells(cells), bg=bg)
        msize = mix.nal_sizes()  # synchronises
        assert msize[0] > 0
        inp = np.empty(fb, np.uint8)
        h264mi._hip_memcpy_d2h(inp.ctypes.data, gpu_lib.h264mi_enc_input_buffer(mix._e), fb)
        want = compose(fill(W, H, 1, *bg), W, H, decoded.cpu().numpy().reshape(S, fb), W, H, cells)
        want = overlayref.blend(want, W, H, d_spr.cpu().numpy(), 64, 16, labels)
        assert np.array_equal(inp, want[0]), 'the composed and labelled input'
        shown_got.zero_()
        view.decode_frames([mix.nal_ptr(0)], nal_sizes=[msize[0]], out_ptrs=[shown.data_ptr()], got_ptrs=[shown_got.data_ptr()])
        torch.cuda.synchronize()
        assert view.status()[0] == 0 and shown_got.cpu().tolist() == [1]
    for x in (enc, dec, mix, view):
        x.close()
