"""GPU: the I420 compositor -- h264mi_i420_compose_dev, h264mi_i420_fill_dev and the encoder's composed input
h264mi_enc_encode_composed -- against tests/composeref.py. The definition is exact integer arithmetic, so every
comparison is equality of bytes. Every canvas is pre-filled with a seeded random pattern, so an untouched byte is
provable, and sits between 64 guard bytes of 0xA5 that must stay as they were."""
import ctypes
import functools

import numpy as np
import pytest

import composeref
import qualityref
import scaleref
from composeref import C
from test_gpu_scale import KEYS, _device, _guarded, _guards_intact, _run, _sources

pytestmark = pytest.mark.gpu


def _frames(w, h, n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, scaleref.frame_bytes(w, h)), dtype=np.uint8)


def _cells(cells):
    import h264mi
    return [h264mi.Cell(*composeref.as_tuple(c)) for c in cells]


def _compose(pattern, cw, ch, src, sw, sh, cells, shift=0, fill=None):
    """the standalone call: canvases pre-filled with `pattern` (an (ncanvas, frame bytes) array) -- and then, with fill
    = (y, cb, cr), by i420_fill --, composed from `src` (an (nsrc, frame bytes) array); the canvases as an array,
    guards checked"""
    import torch
    import h264mi
    ncanvas, cfb = pattern.shape
    d_src = _device(src, shift)
    whole, dst = _guarded(ncanvas * cfb, shift)
    dst.copy_(torch.from_numpy(np.ascontiguousarray(pattern).ravel()))
    if shift:
        assert d_src.data_ptr() % 2 == 1 and dst.data_ptr() % 2 == 1
    if fill is not None:
        h264mi.i420_fill(dst, cw, ch, ncanvas, *fill)
    h264mi.i420_compose(dst, cw, ch, ncanvas, d_src, sw, sh, len(src), _cells(cells))
    out = dst.cpu().numpy().reshape(ncanvas, cfb)
    assert _guards_intact(whole, ncanvas * cfb, shift), 'bytes outside the canvases were written'
    return out


def _check(cw, ch, ncanvas, sw, sh, nsrc, cells, seed, shift=0):
    src, pattern = _frames(sw, sh, nsrc, seed), _frames(cw, ch, ncanvas, seed + 1)
    got = _compose(pattern, cw, ch, src, sw, sh, cells, shift)
    want = composeref.compose(pattern, cw, ch, src, sw, sh, cells)
    for c in range(ncanvas):
        assert np.array_equal(got[c], want[c]), f'canvas {c}: {int((got[c] != want[c]).sum())} bytes differ'
    return src, pattern, got


def test_one_whole_frame_cell_equals_the_scaler(gpu_lib):
    import torch
    import h264mi
    src, _, got = _check(32, 24, 1, 48, 36, 2, [C(1, 0, 0, 0, 48, 36, 0, 0, 32, 24)], 3000)
    assert np.array_equal(got[0], scaleref.scale_frame(src[1], 48, 36, 32, 24))
    dst = torch.zeros(scaleref.frame_bytes(32, 24), dtype=torch.uint8, device='cuda')
    h264mi.i420_scale(dst, _device(src[1]), 48, 36, 32, 24, 1)
    assert np.array_equal(got[0], dst.cpu().numpy()), 'the scaler\'s bytes'


def test_crop_with_pitch_and_an_origin_that_is_no_multiple_of_4(gpu_lib):
    """source 64x48, crop (2, 2, 36, 18) -> rectangle (6, 4, 20, 10) of a 40x24 canvas: the source pitch is not the
    crop's width; chroma is 18x9 at (1, 1) -> 10x5 at (3, 2), odd offsets and sizes"""
    _check(40, 24, 1, 64, 48, 1, [C(0, 0, 2, 2, 36, 18, 6, 4, 20, 10)], 3010)


def test_gallery_2x2_through_mosaic_cells(gpu_lib):
    import h264mi
    cells = h264mi.mosaic_cells(4, 32, 32, 32, 32)
    assert [composeref.as_tuple(c) for c in cells] == [tuple(c) for c in composeref.mosaic_cells(4, 32, 32, 32, 32)]
    _, pattern, got = _check(32, 32, 1, 32, 32, 4, cells, 3020)
    assert not np.array_equal(got[0], pattern[0])


def test_empty_slot_keeps_the_pattern_or_the_background(gpu_lib):
    cells = composeref.mosaic_cells(3, 32, 32, 32, 32)
    src, pattern, got = _check(32, 32, 1, 32, 32, 3, cells, 3030)
    y = scaleref.planes(got[0], 32, 32)[0]
    assert np.array_equal(y[16:, 16:], scaleref.planes(pattern[0], 32, 32)[0][16:, 16:]), 'the empty slot holds the pattern'
    bg = (16, 128, 129)
    got = _compose(pattern, 32, 32, src, 32, 32, cells, fill=bg)
    want = composeref.compose(composeref.fill(32, 32, 1, *bg), 32, 32, src, 32, 32, cells)
    assert np.array_equal(got, want)
    for p, v in zip(scaleref.planes(got[0], 32, 32), bg):
        assert (p[p.shape[0] // 2:, p.shape[1] // 2:] == v).all(), 'the empty slot holds the background'


@pytest.mark.parametrize('w,h,n,shift', [(32, 32, 1, 0), (38, 22, 3, 0), (38, 22, 3, 1), (2, 2, 5, 1), (176, 144, 2, 0)],
                         ids=['32x32', '38x22x3', '38x22x3-odd-address', '2x2x5-odd-address', '176x144x2'])
def test_fill(gpu_lib, w, h, n, shift):
    import h264mi
    fb = scaleref.frame_bytes(w, h)
    whole, dst = _guarded(n * fb, shift)
    h264mi.i420_fill(dst, w, h, n, 35, 212, 7)
    assert np.array_equal(dst.cpu().numpy().reshape(n, fb), composeref.fill(w, h, n, 35, 212, 7))
    assert _guards_intact(whole, n * fb, shift)
    for bad in ((w - 1, h, n, 16, 128, 128), (w, h, 0, 16, 128, 128), (w, h, n, 256, 128, 128), (w, h, n, 16, -1, 128)):
        with pytest.raises(ValueError):
            h264mi.i420_fill(dst, *bad)


def test_letterbox(gpu_lib):
    import h264mi
    cells = h264mi.mosaic_cells(1, 64, 36, 48, 48)
    assert composeref.as_tuple(cells[0]) == (0, 0, 0, 0, 64, 36, 0, 10, 48, 26)
    _, pattern, got = _check(48, 48, 1, 64, 36, 1, cells, 3040)
    assert np.array_equal(got[0][:48 * 10], pattern[0][:48 * 10]), 'the bar above the picture'


WIDE = [C(0, 0, 0, 0, 1280, 48, 6, 4, 852, 32)]  # several strips; the canvas pitch 998 (chroma 499) is no multiple of 4


@pytest.mark.parametrize('shift', [0, 1], ids=['aligned', 'odd-address'])
def test_several_strips_and_row_varying_store_alignment(gpu_lib, shift):
    _check(998, 40, 1, 1280, 48, 1, WIDE, 3050, shift)


def test_more_cells_than_one_launch_holds(gpu_lib):
    """70 sources of 16x16 as identity cells on a 160x112 canvas, in shuffled cell order: two launches"""
    order = np.random.default_rng(5).permutation(70)
    cells = [C(int(k), 0, 0, 0, 16, 16, 16 * (int(k) % 10), 16 * (int(k) // 10), 16, 16) for k in order]
    src, _, got = _check(160, 112, 1, 16, 16, 70, cells, 3060)
    y = scaleref.planes(got[0], 160, 112)[0]
    for k in (0, 63, 64, 69):
        assert np.array_equal(y[16 * (k // 10):16 * (k // 10) + 16, 16 * (k % 10):16 * (k % 10) + 16], scaleref.planes(src[k], 16, 16)[0])


def test_several_canvases_and_fan_out(gpu_lib):
    """3 canvases of 64x48, 2 sources of 96x64: source 0 in a cell of every canvas with different crops, source 1 in
    two; the cells not sorted by canvas"""
    cells = [C(0, 2, 10, 6, 60, 40, 2, 4, 30, 20), C(1, 0, 0, 0, 96, 64, 32, 0, 32, 22), C(0, 0, 0, 0, 96, 64, 0, 24, 48, 24),
             C(1, 2, 32, 16, 64, 48, 32, 24, 32, 24), C(0, 1, 34, 22, 62, 42, 2, 6, 62, 42)]
    _, pattern, got = _check(64, 48, 3, 96, 64, 2, cells, 3070)
    assert np.array_equal(scaleref.planes(got[1], 64, 48)[0][:6], scaleref.planes(pattern[1], 64, 48)[0][:6])


def test_accumulator_needs_all_32_bits(gpu_lib):
    """an all-255 4096x4096 source cropped whole into a 16x16 rectangle of a 32x32 canvas: the numerator reaches
    255 * 2^24 + 2^23 = 4 286 578 688, above 2^31. The expectation is by hand: 255 in the rectangle, the pattern elsewhere"""
    import torch
    import h264mi
    sw = sh = 4096
    assert 255 * sw * sh + (sw * sh >> 1) == 4286578688 > 1 << 31
    pattern = _frames(32, 32, 1, 3081)
    cfb = scaleref.frame_bytes(32, 32)
    src = torch.full((scaleref.frame_bytes(sw, sh),), 255, dtype=torch.uint8, device='cuda')
    whole, dst = _guarded(cfb)
    dst.copy_(torch.from_numpy(pattern.ravel()))
    h264mi.i420_compose(dst, 32, 32, 1, src, sw, sh, 1, _cells([C(0, 0, 0, 0, sw, sh, 8, 10, 16, 16)]))
    want = pattern.copy()
    for p, plane in enumerate(scaleref.planes(want[0], 32, 32)):
        k = 1 if p else 0
        plane[10 >> k:(10 >> k) + (16 >> k), 8 >> k:(8 >> k) + (16 >> k)] = 255
    assert np.array_equal(dst.cpu().numpy(), want[0])
    assert _guards_intact(whole, cfb)


def test_repeatability(gpu_lib):
    src, pattern = _frames(1280, 48, 1, 3090), _frames(998, 40, 1, 3091)
    a = _compose(pattern, 998, 40, src, 1280, 48, WIDE)
    b = _compose(pattern, 998, 40, src, 1280, 48, WIDE)
    assert a.tobytes() == b.tobytes()


def test_standalone_bad_arguments(gpu_lib):
    import torch
    import h264mi
    from test_compose_host import BAD, OK_CELL
    fn = gpu_lib.h264mi_i420_compose_dev
    s = torch.zeros(3 * 1536, dtype=torch.uint8, device='cuda')
    whole, d = _guarded(2 * 1536)
    ps, pd = ctypes.c_void_p(s.data_ptr()), ctypes.c_void_p(d.data_ptr())
    one = (h264mi.Cell * 1)(h264mi.Cell(*OK_CELL))
    assert fn(pd, 32, 32, 1, ps, 32, 32, 1, one, 1, None) == 0
    for cw, ch, ncanvas, sw, sh, nsrc, cells in BAD:
        arr = (h264mi.Cell * len(cells))(*[h264mi.Cell(*t) for t in cells]) if cells else one
        assert fn(pd, cw, ch, ncanvas, ps, sw, sh, nsrc, arr, len(cells), None) == -1, (cw, ch, ncanvas, sw, sh, nsrc, cells)
    for off in (0, 1, 1535, 3 * 1536 - 1):  # the canvas inside the sources
        assert fn(ctypes.c_void_p(s.data_ptr() + off), 32, 32, 1, ps, 32, 32, 3, one, 1, None) == -1
    with pytest.raises(ValueError):  # through the Python function: two cells that share a sample
        h264mi.i420_compose(d, 32, 32, 1, s, 32, 32, 1, [h264mi.Cell(*OK_CELL), h264mi.Cell(0, 0, 0, 0, 32, 32, 14, 14, 16, 16)])
    with pytest.raises(ValueError):
        h264mi.i420_compose(d, 32, 32, 1, s, 32, 32, 1, [])
    torch.cuda.synchronize()
    assert _guards_intact(whole, 2 * 1536)


# ---------------------------------------------------------------- the encoder's composed input

W, H, BR = 176, 144, 300000


def _gallery(per_stream):
    """per_stream[s]: the sources of stream s's gallery, in slot order -> cells on canvas s"""
    cells = []
    for s, srcs in enumerate(per_stream):
        for c, k in zip(composeref.mosaic_cells(len(srcs), W, H, W, H), srcs):
            cells.append(c._replace(src=k, canvas=s))
    return cells


@functools.lru_cache(maxsize=None)
def _composed_sources(layout, bg, nf):
    """composeref's frames of every step: the background (or zeros, where the cells cover everything) composed from the
    5 synthetic sources"""
    cells = _gallery(layout)
    base = composeref.fill(W, H, len(layout), *bg) if bg is not None else np.zeros((len(layout), scaleref.frame_bytes(W, H)), np.uint8)
    return [composeref.compose(base, W, H, step, W, H, cells) for step in _sources(W, H, 5, nf)]


@pytest.mark.parametrize('layout,bg', [(((0, 1, 2, 3), (3, 4, 0, 2)), None), (((0, 1, 2), (2, 4, 3)), (40, 100, 200))],
                         ids=['2x2-of-four', 'three-and-a-background'])
def test_encode_composed_equals_encode_of_reference_frames(gpu_lib, layout, bg):
    S, nf = 2, 3
    src, ref = _sources(W, H, 5, nf), _composed_sources(layout, bg, nf)
    cells = _cells(_gallery(layout))
    if bg is None:  # four 88x72 cells cover the 176x144 picture: no uncovered sample
        assert sum(c.dw * c.dh for c in cells) == S * W * H
    else:
        for f in ref[0]:
            assert (scaleref.planes(f, W, H)[0][H // 2:, W // 2:] == bg[0]).all() and (scaleref.planes(f, W, H)[2][H // 4:, W // 4:] == bg[2]).all()
    for quality in (False, True):
        got = _run(W, H, BR, S, src, lambda e, f: e.encode_composed(f, W, H, 5, cells, bg=bg), quality)
        want = _run(W, H, BR, S, ref, lambda e, f: e.encode(f), quality)
        for t in range(nf):
            for s in range(S):
                assert len(got[t]['nal'][s]) > 0
                assert got[t]['nal'][s] == want[t]['nal'][s], f'frame {t} stream {s}: NAL bytes'
                assert got[t]['rc'][s] == want[t]['rc'][s], f'frame {t} stream {s}: rate-control state'
                if quality:
                    q = {k: got[t]['q'][s][k] for k in KEYS}
                    assert q == qualityref.frame_quality(ref[t][s], got[t]['recon'][s], W, H), f'frame {t} stream {s}: records'
                    assert q == {k: want[t]['q'][s][k] for k in KEYS}


def test_encode_composed_refusals_leave_the_encoder_untouched(gpu_lib):
    import torch
    import h264mi
    S = 2
    src = _sources(W, H, S, 1)[0]
    fresh = _run(W, H, BR, S, [src], lambda e, f: e.encode(f))[0]
    big = torch.zeros(5 * scaleref.frame_bytes(W, H), dtype=torch.uint8, device='cuda')
    good = _gallery(((0, 1, 2, 3), (3, 4, 0, 2)))

    def feed(enc, frames):
        fn = enc._L.h264mi_enc_encode_composed
        p = ctypes.c_void_p(big.data_ptr())

        def call(cells, ptr=p, bg=(16, 128, 128), nsrc=5):
            arr = (h264mi.Cell * len(cells))(*_cells(cells))
            return fn(enc._e, ptr, W, H, nsrc, arr, len(cells), *bg)

        assert call(good + [C(0, 1, 0, 0, W, H, 80, 60, 16, 16)]) == -1          # an overlapping pair of cells
        assert call([good[0]._replace(dx=good[0].dx + 1)]) == -1                 # an odd field
        assert call([good[0]._replace(sw=W - 1)]) == -1
        assert call(good, nsrc=3) == -1                                          # src out of range
        assert call([good[0]._replace(canvas=2)]) == -1                          # a canvas the encoder has not
        assert call(good, bg=(256, 128, 128)) == -1 and call(good, bg=(16, 128, 300)) == -1 and call(good, bg=(-1, 256, 0)) == -1
        assert call(good, ptr=None) == -1
        inp = enc._L.h264mi_enc_input_buffer(enc._e)                             # sources inside the input area
        assert call(good, ptr=ctypes.c_void_p(inp)) == -1
        assert call(good, ptr=ctypes.c_void_p(inp + S * scaleref.frame_bytes(W, H) - 1)) == -1
        assert call(good, ptr=ctypes.c_void_p(inp - 5 * scaleref.frame_bytes(W, H) + 1)) == -1
        with pytest.raises(ValueError):  # through the Python method
            enc.encode_composed(big, W, H, 5, _cells(good + [C(0, 1, 0, 0, W, H, 80, 60, 16, 16)]))
        with pytest.raises(ValueError):
            enc.encode_composed(big, W, H, 5, _cells(good), bg=(16, 128, 256))
        enc.encode(frames)

    got = _run(W, H, BR, S, [src], feed)[0]
    assert got['nal'] == fresh['nal'] and got['rc'] == fresh['rc']


def test_decode_compose_encode(gpu_lib):
    """two streams encoded for 2 frames, decoded with frames out into one back-to-back buffer, composed side by side
    into a third encoder's input; its NAL bytes decode on a fresh decoder"""
    import torch
    import h264mi
    S, nf, fb = 2, 2, scaleref.frame_bytes(W, H)
    enc = h264mi.BatchEncoder(W, H, BR, S)
    enc.set_frame_skip(False)
    dec = h264mi.BatchDecoder(W, H, S)
    mix = h264mi.BatchEncoder(W, H, BR, 1)
    mix.set_frame_skip(False)
    view = h264mi.BatchDecoder(W, H, 1)
    decoded = torch.zeros(S * fb, dtype=torch.uint8, device='cuda')  # stream 0's frame, then stream 1's
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
        want = composeref.compose(composeref.fill(W, H, 1, *bg), W, H, decoded.cpu().numpy().reshape(S, fb), W, H, cells)
        assert np.array_equal(inp, want[0]), 'the composed input'
        shown_got.zero_()
        view.decode_frames([mix.nal_ptr(0)], nal_sizes=[msize[0]], out_ptrs=[shown.data_ptr()], got_ptrs=[shown_got.data_ptr()])
        torch.cuda.synchronize()
        assert view.status()[0] == 0 and shown_got.cpu().tolist() == [1]
        pic = scaleref.planes(shown.cpu().numpy(), W, H)[0].astype(np.int32)
        assert np.abs(pic[:36].mean() - 16) < 8 and pic.shape == (H, W), 'a picture: the bar above the cells is near the background'
    for x in (enc, dec, mix, view):
        x.close()
