"""GPU: the I420 upscaler -- h264mi_i420_upscale_dev, h264mi_i420_compose_any_dev and the encoder's composed input
h264mi_enc_encode_composed_any -- against tests/upscaleref.py. The definition is exact integer arithmetic, so every
comparison is equality of bytes. Every destination is pre-filled with a seeded random pattern, so an untouched byte is
provable, and sits between 64 guard bytes of 0xA5 that must stay as they were."""
import ctypes
import functools

import numpy as np
import pytest

import composeref
import overlayref
import qualityref
import scaleref
import upscaleref
from composeref import C
from overlayref import O
from test_gpu_compose import _cells
from test_gpu_overlay import _ovs
from test_gpu_scale import KEYS, _device, _guarded, _guards_intact, _recon, _run, _sources

pytestmark = pytest.mark.gpu

FILTERS = [upscaleref.BILINEAR, upscaleref.BICUBIC]
FILTER_IDS = ['bilinear', 'bicubic']
PER_LAUNCH = 64  # H264MI_UPSCALE_PER_LAUNCH (include/h264mi.h)


def _frames(w, h, n, seed, extreme=False):
    f = np.random.default_rng(seed).integers(0, 256, (n, scaleref.frame_bytes(w, h)), dtype=np.uint8)
    return np.where(f < 128, 0, 255).astype(np.uint8) if extreme else f  # 0/255: overshoot on every edge, the clamp at work


# (sw, sh, dw, dh): 2x2 onto itself: identity, 1x1 chroma; 2x2 -> 128x64: every tap clamped, two strips, two segments;
# 16x16 -> 32x32: 2x; 36x18 -> 50x22: odd chroma pitches 18 -> 25 and 9 -> 11; 34x18 -> 36x18: one axis equal;
# 64x36 -> 130x72: a rectangle just over two wave widths, three row segments
SHAPES = [(2, 2, 2, 2), (2, 2, 128, 64), (16, 16, 32, 32), (36, 18, 50, 22), (34, 18, 36, 18), (64, 36, 130, 72)]


@functools.lru_cache(maxsize=None)
def _whole_frames(sw, sh, dw, dh, filt, extreme):
    src = _frames(sw, sh, 3, 5000 + sw + sh + dw + dh, extreme)
    return src, np.stack([upscaleref.up_frame(f, sw, sh, dw, dh, filt) for f in src])


@pytest.mark.parametrize('extreme', [False, True], ids=['random', '0-255'])
@pytest.mark.parametrize('filt', FILTERS, ids=FILTER_IDS)
@pytest.mark.parametrize('sw,sh,dw,dh', SHAPES, ids=[f'{a}x{b}-to-{c}x{d}' for a, b, c, d in SHAPES])
def test_whole_frames_vs_reference(gpu_lib, sw, sh, dw, dh, filt, extreme):
    """n = 3 frames, source and destination one byte into their allocations"""
    import h264mi
    n, dfb = 3, scaleref.frame_bytes(dw, dh)
    src, want = _whole_frames(sw, sh, dw, dh, filt, extreme)
    d_src = _device(src, 1)
    whole, dst = _guarded(n * dfb, 1)
    assert d_src.data_ptr() % 2 == 1 and dst.data_ptr() % 2 == 1
    h264mi.i420_upscale(dst, d_src, sw, sh, dw, dh, n, filt)
    got = dst.cpu().numpy().reshape(n, dfb)
    assert _guards_intact(whole, n * dfb, 1), 'bytes outside the destination frames were written'
    for f in range(n):
        assert np.array_equal(got[f], want[f]), f'frame {f}: {int((got[f] != want[f]).sum())} bytes differ'
    if (sw, sh) == (dw, dh):
        assert np.array_equal(got, src)
    if extreme and filt == upscaleref.BICUBIC and dw >= 2 * sw and sw > 2:
        raw = upscaleref.up_plane(src[0][:sw * sh].reshape(sh, sw), dw, dh, filt, clamp=False)
        assert raw.min() < 0 and raw.max() > 255, 'the case was to exercise the clamp'


def _compose_any(pattern, cw, ch, src, sw, sh, cells, filt, shift=0):
    """the standalone call: canvases pre-filled with `pattern`, composed from `src`; the canvases as an array, guards
    checked"""
    import torch
    import h264mi
    ncanvas, cfb = pattern.shape
    d_src = _device(src, shift)
    whole, dst = _guarded(ncanvas * cfb, shift)
    dst.copy_(torch.from_numpy(np.ascontiguousarray(pattern).ravel()))
    h264mi.i420_compose_any(dst, cw, ch, ncanvas, d_src, sw, sh, len(src), _cells(cells), filt)
    out = dst.cpu().numpy().reshape(ncanvas, cfb)
    assert _guards_intact(whole, ncanvas * cfb, shift), 'bytes outside the canvases were written'
    return out


def _outside(cw, ch, ncanvas, cells):
    """a (ncanvas, frame bytes) mask of the bytes no cell covers"""
    m = np.ones((ncanvas, scaleref.frame_bytes(cw, ch)), np.uint8)
    for c in cells:
        for p, plane in enumerate(scaleref.planes(m[c.canvas], cw, ch)):
            k = 1 if p else 0
            plane[c.dy >> k:(c.dy + c.dh) >> k, c.dx >> k:(c.dx + c.dw) >> k] = 0
    return m != 0


@pytest.mark.parametrize('filt', FILTERS, ids=FILTER_IDS)
def test_taps_clamp_to_the_crop_not_to_the_frame(gpu_lib, filt):
    """a 64x48 source that is 255 everywhere but 0 in the crop (10, 6, 20, 12): enlarged to 50x30 at (6, 4) of a 64x48
    canvas (chroma 10x6 at (5, 3) -> 25x15 at (3, 2)), every sample of the rectangle must be 0 -- a tap outside the
    crop would bring in 255"""
    sw, sh, cw, ch = 64, 48, 64, 48
    src = np.full((1, scaleref.frame_bytes(sw, sh)), 255, np.uint8)
    for p, plane in enumerate(scaleref.planes(src[0], sw, sh)):
        k = 1 if p else 0
        plane[6 >> k:(6 + 12) >> k, 10 >> k:(10 + 20) >> k] = 0
    cells = [C(0, 0, 10, 6, 20, 12, 6, 4, 50, 30)]
    pattern = _frames(cw, ch, 1, 5101)
    for shift in (0, 1):
        got = _compose_any(pattern, cw, ch, src, sw, sh, cells, filt, shift)
        out = _outside(cw, ch, 1, cells)
        assert (got[~out] == 0).all(), 'a tap outside the crop was read'
        assert np.array_equal(got[out], pattern[out])
        assert np.array_equal(got, upscaleref.compose_any(pattern, cw, ch, src, sw, sh, cells, filt))


@functools.lru_cache(maxsize=None)
def _seventy():
    """70 cells over 3 canvases of 200x120 from 4 sources of 32x24: slot k of a 10 x 7 grid of 20x16 slots on canvas
    k % 3 holds a shrinking cell (the whole source to 16x12 or 12x8; three of them), an equal-size one (a 16x12 crop;
    two) or an enlarging one (crops of 8x6 .. 16x12 to 20x16, 18x14 or 20x12; 65, more than one launch holds), in
    shuffled order"""
    rng = np.random.default_rng(5200)
    cells = []
    for k in range(70):
        x, y, src, canvas = 20 * (k % 10), 16 * (k // 10), int(rng.integers(4)), k % 3
        if k in (0, 23, 46):
            cells.append(C(src, canvas, 0, 0, 32, 24, x + 2, y + 2, (16, 12)[k == 23], (12, 8)[k == 23]))
        elif k in (11, 57):
            cells.append(C(src, canvas, 2 * int(rng.integers(8)), 2 * int(rng.integers(6)), 16, 12, x, y + 4, 16, 12))
        else:
            sw, sh = ((8, 6), (10, 12), (16, 12), (14, 10))[int(rng.integers(4))]
            dw, dh = ((20, 16), (18, 14), (20, 12))[int(rng.integers(3))]
            cells.append(C(src, canvas, 2 * int(rng.integers((32 - sw) // 2 + 1)), 2 * int(rng.integers((24 - sh) // 2 + 1)), sw, sh, x, y, dw, dh))
    cells = [cells[i] for i in rng.permutation(70)]
    kinds = [upscaleref.kind(c) for c in cells]
    assert None not in kinds and kinds.count(1) == 65 > PER_LAUNCH and sum(c.dw == c.sw and c.dh == c.sh for c in cells) == 2
    assert {c.canvas for c in cells if upscaleref.kind(c) == 0} == {0, 1, 2}
    return cells


@pytest.mark.parametrize('filt', FILTERS, ids=FILTER_IDS)
def test_seventy_cells_of_every_kind_over_three_canvases(gpu_lib, filt):
    import torch
    import h264mi
    cw, ch, sw, sh = 200, 120, 32, 24
    cells = _seventy()
    src, pattern = _frames(sw, sh, 4, 5201), _frames(cw, ch, 3, 5202)
    got = _compose_any(pattern, cw, ch, src, sw, sh, cells, filt, shift=1)
    want = upscaleref.compose_any(pattern, cw, ch, src, sw, sh, cells, filt)
    for c in range(3):
        assert np.array_equal(got[c], want[c]), f'canvas {c}: {int((got[c] != want[c]).sum())} bytes differ'
    out = _outside(cw, ch, 3, cells)
    assert out.any() and np.array_equal(got[out], pattern[out]), 'canvas bytes outside the rectangles'
    # the shrinking cells alone: the bytes of i420_compose itself
    small = [c for c in cells if upscaleref.kind(c) == 0]
    only = _compose_any(pattern, cw, ch, src, sw, sh, small, filt)
    d_src = _device(src)
    whole, dst = _guarded(pattern.size)
    dst.copy_(torch.from_numpy(pattern.ravel()))
    h264mi.i420_compose(dst, cw, ch, 3, d_src, sw, sh, 4, _cells(small))
    assert np.array_equal(only.ravel(), dst.cpu().numpy()), 'shrinking cells: i420_compose\'s own bytes'
    inside = ~_outside(cw, ch, 3, small)
    assert np.array_equal(got[inside], only[inside])


def test_standalone_bad_arguments(gpu_lib):
    import torch
    import h264mi
    from test_upscale_host import BAD, UP_CELL
    fn = gpu_lib.h264mi_i420_compose_any_dev
    s = torch.zeros(3 * 1536, dtype=torch.uint8, device='cuda')
    whole, d = _guarded(2 * 6144)
    ps, pd = ctypes.c_void_p(s.data_ptr()), ctypes.c_void_p(d.data_ptr())
    one = (h264mi.Cell * 1)(h264mi.Cell(*UP_CELL))
    assert fn(pd, 64, 64, 1, ps, 32, 32, 1, one, 1, 1, None) == 0
    for cw, ch, ncanvas, sw, sh, nsrc, cells, filt in BAD:
        arr = (h264mi.Cell * len(cells))(*[h264mi.Cell(*t) for t in cells]) if cells else one
        assert fn(pd, cw, ch, ncanvas, ps, sw, sh, nsrc, arr, len(cells), filt, None) == -1, (cw, ch, ncanvas, sw, sh, nsrc, cells, filt)
    with pytest.raises(ValueError):  # through the Python functions: a mixed cell, a shrinking whole frame, an unknown filter
        h264mi.i420_compose_any(d, 64, 64, 1, s, 32, 32, 1, [h264mi.Cell(0, 0, 0, 0, 16, 16, 0, 0, 18, 14)])
    with pytest.raises(ValueError):
        h264mi.i420_upscale(d, s, 32, 32, 30, 32, 1)
    with pytest.raises(ValueError):
        h264mi.i420_upscale(d, s, 32, 32, 64, 64, 1, filter=2)
    torch.cuda.synchronize()
    h = whole.cpu().numpy()
    assert (h[64 + 6144:] == 0xA5).all() and (h[:64] == 0xA5).all(), 'only the first canvas was written'


# ---------------------------------------------------------------- the encoder's composed input

W, H, BR, S, NF = 64, 48, 300000, 2, 3
SW, SH, NSRC = 32, 24, 3
BG = (40, 100, 200)
LW, LH = 16, 8
LIST = [O(0, 0, 0, 0, 16, 8, 10, 2, 160), O(1, 1, 2, 2, 12, 6, 40, 38, 256)]  # over the speaker on stream 0, over a thumbnail on stream 1


def _layout():
    """stream 0 shows source 0 as the speaker, stream 1 source 2"""
    cells = []
    for s, speaker in enumerate((0, 2)):
        cells += [c._replace(canvas=s) for c in upscaleref.speaker_cells(NSRC, speaker, SW, SH, W, H)]
    return cells


@functools.lru_cache(maxsize=None)
def _logo_sprites():
    return np.random.default_rng(5300).integers(0, 256, (2, overlayref.sprite_bytes(LW, LH)), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _reference_steps(filt):
    cells = _layout()
    assert [upscaleref.kind(c) for c in cells] == [1, 0, 0, 0, 0, 1] and cells[0][6:] == (8, 0, 48, 36)
    base = composeref.fill(W, H, S, *BG)
    return [overlayref.blend(upscaleref.compose_any(base, W, H, step, SW, SH, cells, filt), W, H, _logo_sprites(), LW, LH, LIST)
            for step in _sources(SW, SH, NSRC, NF)]


def _feeder(d_spr, filt):
    cells = _cells(_layout())

    def feed(enc, frames):
        if enc.overlays() == 0:
            enc.set_overlays(d_spr, LW, LH, 2, _ovs(LIST))
        enc.encode_composed_any(frames, SW, SH, NSRC, cells, filter=filt, bg=BG)
    return feed


@pytest.mark.parametrize('filt', FILTERS, ids=FILTER_IDS)
def test_encode_composed_any_equals_encode_of_reference_frames(gpu_lib, filt):
    src, ref = _sources(SW, SH, NSRC, NF), _reference_steps(filt)
    d_spr = _device(_logo_sprites())
    for quality in (False, True):
        got = _run(W, H, BR, S, src, _feeder(d_spr, filt), quality)
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


def test_encode_composed_any_decodes_to_the_reconstruction_and_encode_composed_still_refuses(gpu_lib):
    import torch
    import h264mi
    fb = scaleref.frame_bytes(W, H)
    enc = h264mi.BatchEncoder(W, H, BR, S)
    enc.set_frame_skip(False)
    dec = h264mi.BatchDecoder(W, H, S)
    d_spr = _device(_logo_sprites())
    feed = _feeder(d_spr, upscaleref.BICUBIC)
    decoded = torch.zeros(S * fb, dtype=torch.uint8, device='cuda')
    got = torch.zeros(S, dtype=torch.int32, device='cuda')
    ref = _reference_steps(upscaleref.BICUBIC)
    for t, step in enumerate(_sources(SW, SH, NSRC, NF)):
        frames = torch.from_numpy(np.ascontiguousarray(step).ravel()).cuda()
        feed(enc, frames)
        sizes = enc.nal_sizes()  # synchronises
        assert all(n > 0 for n in sizes)
        inp = np.empty(S * fb, np.uint8)
        h264mi._hip_memcpy_d2h(inp.ctypes.data, gpu_lib.h264mi_enc_input_buffer(enc._e), S * fb)
        assert np.array_equal(inp.reshape(S, fb), ref[t]), f'frame {t}: the composed input'
        got.zero_()
        dec.decode_frames(enc.nal_ptrs(), nal_sizes=sizes, out_ptrs=[decoded[s * fb:].data_ptr() for s in range(S)],
                          got_ptrs=[got[s:s + 1].data_ptr() for s in range(S)])
        torch.cuda.synchronize()
        assert dec.status()[0] == 0 and got.cpu().tolist() == [1] * S
        pics = decoded.cpu().numpy().reshape(S, fb)
        for s in range(S):
            assert np.array_equal(pics[s], _recon(enc, s)), f'frame {t} stream {s}: decoded picture != the encoder\'s reconstruction'
    # the parent's entry keeps its size rule on the same encoder
    cells = _cells(_layout())
    with pytest.raises(ValueError):
        enc.encode_composed(frames, SW, SH, NSRC, cells, bg=BG)
    with pytest.raises(ValueError):  # and the new one refuses a mixed cell, an unknown filter and a bad background
        enc.encode_composed_any(frames, SW, SH, NSRC, [h264mi.Cell(0, 0, 0, 0, 32, 24, 0, 0, 34, 22)])
    with pytest.raises(ValueError):
        enc.encode_composed_any(frames, SW, SH, NSRC, cells, filter=2)
    with pytest.raises(ValueError):
        enc.encode_composed_any(frames, SW, SH, NSRC, cells, bg=(16, 128, 256))
    enc.encode_composed(frames, SW, SH, NSRC, [c for c in cells if upscaleref.kind(c) == 0], bg=BG)  # its own cells still pass
    assert all(n > 0 for n in enc.nal_sizes())
    enc.close()
    dec.close()
