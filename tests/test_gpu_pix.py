"""GPU: pixel formats and pitched layouts -- the standalone calls h264mi_pix_to_i420_dev / h264mi_i420_to_pix_dev, the
encoder's input h264mi_enc_encode_pix and the decoder's output layout -- against tests/pixref.py. Every comparison is
equality of bytes. Every destination is filled with 0xA5 and sits between 64 guard bytes; after a pack the whole
allocation -- guards, pitch padding, the gaps between planes and frames -- must equal the reference's pack into an equally
filled buffer. A lane's piece is 16 bytes of the packed or interleaved side and a wave reaches 1024 of them
(csrc/pixfmt.hip), which the shapes below are chosen around."""
import ctypes
import functools

import numpy as np
import pytest

import pixref

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5
N = 3


def _lay(L):
    import h264mi
    return h264mi.PixLayout(L.pix, L.pitch, L.offset, L.frame_stride)


def _device(x, shift=0):
    """x's bytes on the device, `shift` bytes into a larger allocation"""
    import torch
    whole = torch.zeros(x.size + shift + 64, dtype=torch.uint8, device='cuda')
    view = whole[shift:shift + x.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(x).ravel()))
    return view


def _guarded(nbytes, shift=0):
    """(whole, view): a destination of nbytes of 0xA5 between 64 bytes of 0xA5 on each side, `shift` bytes into its allocation"""
    import torch
    whole = torch.full((shift + nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device='cuda')
    return whole, whole[shift + GUARD:shift + GUARD + nbytes]


def _align(x, a):
    return (x + a - 1) // a * a


def layout(kind, pix, w, h):
    """the four layouts of a shape: 'tight'; 'pitch13' (every pitch 13 above the row bytes: unaligned rows); 'surface'
    (pitches rounded up to 256, every next plane on row align16(rows) of the one before: a hardware surface, the wide
    path with padding); 'stride7' (tight planes, frame_stride = span + 7: every later frame at another alignment)"""
    pl = pixref.planes(pix, w, h)
    if kind == 'tight':
        return pixref.tight(pix, w, h)
    if kind == 'stride7':
        L = pixref.tight(pix, w, h)
        L.frame_stride += 7
        return L
    pitch, offset, at = [], [], 0
    for rb, rows in pl:
        p = rb + 13 if kind == 'pitch13' else _align(rb, 256)
        pitch.append(p)
        offset.append(at)
        at += p * (rows if kind == 'pitch13' else _align(rows, 16))
    L = pixref.Layout(pix, pitch, offset, 0)
    L.frame_stride = pixref.span(L, w, h) if kind == 'pitch13' else at
    return L


KINDS = ('tight', 'pitch13', 'surface', 'stride7')


@functools.lru_cache(maxsize=None)
def _frames(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (N, pixref.frame_bytes(w, h)), dtype=np.uint8)  # shared: never written


def _pack(src, L, w, h, shift=0):
    """the standalone pack of the N frames src: the whole destination allocation (guards included) as an array"""
    import h264mi
    nb = N * L.frame_stride
    d_src = _device(src, shift)
    whole, dst = _guarded(nb, shift)
    if shift:
        assert d_src.data_ptr() % 2 == 1 and dst.data_ptr() % 2 == 1
    h264mi.i420_to_pix(dst, _lay(L), d_src, w, h, N)
    return whole.cpu().numpy()


def _want_pack(src, L, w, h, shift=0):
    nb = N * L.frame_stride
    want = np.full(shift + nb + 2 * GUARD, FILL, np.uint8)
    pixref.pack_frames(src, L, w, h, want[shift + GUARD:shift + GUARD + nb])
    return want


def _unpack(buf, L, w, h, shift=0):
    """the standalone unpack of the N frames in buf: (the N tight frames, the whole allocation)"""
    import h264mi
    fb = pixref.frame_bytes(w, h)
    d_src = _device(buf, shift)
    whole, dst = _guarded(N * fb, shift)
    h264mi.pix_to_i420(dst, d_src, _lay(L), w, h, N)
    return dst.cpu().numpy().reshape(N, fb), whole.cpu().numpy()


# (w, h, shift): each the smallest shape that reaches its case
#   2x2: 1x1 chroma; 16x16; 36x18: chroma 18x9, rows that are no multiple of 4 or 16 bytes; 64x4 and 72x4: whole 16-byte
#   pieces only, and one piece that crosses the row's end; 1040x6: a row longer than a wave's 1024 bytes on the packed side
#   (an odd number of row pairs: a strip's unused waves); 130x66 with both buffers at odd addresses: the byte path, and
#   more than one strip; 8192x2 and 2x8192: the limits
SHAPES = [(2, 2, 0), (16, 16, 0), (36, 18, 0), (64, 4, 0), (72, 4, 0), (1040, 6, 0), (130, 66, 1), (8192, 2, 0), (2, 8192, 0)]
SHAPE_IDS = [f'{c[0]}x{c[1]}' + ('-odd-address' if c[2] else '') for c in SHAPES]


@pytest.mark.parametrize('pix', pixref.ALL, ids=pixref.NAMES)
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('w,h,shift', SHAPES, ids=SHAPE_IDS)
def test_pack_and_unpack_vs_reference(gpu_lib, w, h, shift, kind, pix):
    L = layout(kind, pix, w, h)
    assert pixref.layout_ok(L, w, h)
    # I420 -> the layout: the whole allocation, guards, padding and gaps included
    src = _frames(w, h, 6000 + w + 3 * h)
    got, want = _pack(src, L, w, h, shift), _want_pack(src, L, w, h, shift)
    assert np.array_equal(got, want), f'pack: {int((got != want).sum())} bytes differ, the first at {int(np.argmax(got != want))}'
    # the layout -> I420, from a buffer whose every byte is random (4:2:2 chroma rows differ: the average is computed)
    nb = N * L.frame_stride
    buf = np.random.default_rng(6100 + w + 3 * h + pix).integers(0, 256, nb, dtype=np.uint8)
    got, whole = _unpack(buf, L, w, h, shift)
    want = pixref.unpack_frames(buf, L, w, h, N)
    assert np.array_equal(got, want), f'unpack: {int((got != want).sum())} bytes differ'
    fb = N * pixref.frame_bytes(w, h)
    assert (whole[:shift + GUARD] == FILL).all() and (whole[shift + GUARD + fb:] == FILL).all(), 'bytes outside the frames were written'


@pytest.mark.parametrize('pix', pixref.ALL, ids=pixref.NAMES)
def test_round_trip_on_the_device_is_the_identity(gpu_lib, pix):
    w, h = 130, 66
    src = _frames(w, h, 6200)
    L = layout('pitch13', pix, w, h)
    packed = _pack(src, L, w, h)[GUARD:GUARD + N * L.frame_stride]
    back, _ = _unpack(packed, L, w, h)
    assert np.array_equal(back, src)


def test_repeatability(gpu_lib):
    w, h = 130, 66
    src = _frames(w, h, 6200)
    for pix in (pixref.NV12, pixref.YUY2):
        L = layout('surface', pix, w, h)
        a, b = _pack(src, L, w, h), _pack(src, L, w, h)
        assert a.tobytes() == b.tobytes()
        buf = np.random.default_rng(6300 + pix).integers(0, 256, N * L.frame_stride, dtype=np.uint8)
        assert _unpack(buf, L, w, h)[0].tobytes() == _unpack(buf, L, w, h)[0].tobytes()


def test_refusals_leave_the_destination_untouched(gpu_lib):
    import torch
    import h264mi
    w, h = 32, 16
    fb = pixref.frame_bytes(w, h)
    to_i420, to_pix = gpu_lib.h264mi_pix_to_i420_dev, gpu_lib.h264mi_i420_to_pix_dev
    for pix in pixref.ALL:
        good = layout('pitch13', pix, w, h)
        nb = N * good.frame_stride
        s = torch.zeros(max(nb, N * fb), dtype=torch.uint8, device='cuda')
        whole, d = _guarded(max(nb, N * fb))
        ps, pd = ctypes.c_void_p(s.data_ptr()), ctypes.c_void_p(d.data_ptr())
        bad = []
        a = layout('pitch13', pix, w, h); a.pitch[0] = pixref.planes(pix, w, h)[0][0] - 1
        bad.append(a)
        a = layout('pitch13', pix, w, h); a.frame_stride -= 1
        bad.append(a)
        a = layout('pitch13', pix, w, h); a.offset[0] = -1
        bad.append(a)
        a = layout('pitch13', pix, w, h); a.pix = 5
        bad.append(a)
        if len(pixref.planes(pix, w, h)) > 1:
            a = layout('tight', pix, w, h); a.offset[1] -= 1
            bad.append(a)
        else:
            a = layout('tight', pix, w, h); a.pitch[1] = 2 * w
            bad.append(a)
        for L in bad:
            assert not pixref.layout_ok(L, w, h)
            r = ctypes.byref(_lay(L))
            assert to_pix(pd, r, ps, w, h, N, None) == -1 and to_i420(pd, ps, r, w, h, N, None) == -1, L
            with pytest.raises(ValueError):
                h264mi.i420_to_pix(d, _lay(L), s, w, h, N)
        r = ctypes.byref(_lay(good))
        assert to_pix(pd, r, ps, 34, h, N, None) == -1 and to_pix(pd, r, ps, w, h, 0, None) == -1
        # overlaps: the layout's side inside the tight frames and the other way round, by one byte at either end
        for off in (0, 1, N * fb - 1, -(nb - 1)):
            assert to_pix(ctypes.c_void_p(d.data_ptr() + off), r, pd, w, h, N, None) == -1, off
            assert to_i420(pd, ctypes.c_void_p(d.data_ptr() + off), r, w, h, N, None) == -1, off
        torch.cuda.synchronize()
        assert (whole.cpu().numpy() == FILL).all(), 'a refused call wrote'
        assert to_pix(pd, r, ps, w, h, N, None) == 0  # and the good call does write
        torch.cuda.synchronize()
        assert (d[:w].cpu().numpy() == 0).all()


# ---------------------------------------------------------------- the encoder's input


@functools.lru_cache(maxsize=None)
def _sources(w, h, S, nf):
    from h264mi.synth import SyntheticStream
    gs = [SyntheticStream(s, w, h) for s in range(S)]
    return [np.stack([np.ascontiguousarray(g.frame(t)).ravel() for g in gs]) for t in range(nf)]


def _run(w, h, br, S, steps, feed, prepare=None):
    """one encoder over `steps` (a list of byte arrays, one per frame step), fed by feed(enc, device bytes): per step the
    NAL bytes, rc_state and last_qp of every stream"""
    import torch
    import h264mi
    enc = h264mi.BatchEncoder(w, h, br, S)
    enc.set_frame_skip(False)
    if prepare:
        prepare(enc)
    out = []
    for fr in steps:
        frames = torch.from_numpy(np.ascontiguousarray(fr).ravel()).cuda()  # held until nal_sizes() has synchronised
        feed(enc, frames)
        sizes = enc.nal_sizes()
        out.append({'nal': [enc.nal_bytes(s, sizes[s]) for s in range(S)], 'rc': [enc.rc_state(s) for s in range(S)],
                    'qp': [enc.last_qp(s) for s in range(S)]})
    enc.close()
    return out


@functools.lru_cache(maxsize=None)
def _plain(w, h, S, nf):
    """encode() of the synthetic sources themselves: the one reference run the NV12 and I420 cases share"""
    return _run(w, h, 300000, S, _sources(w, h, S, nf), lambda e, f: e.encode(f))


def _in_layout(step, L, w, h, S, perturb=None):
    """the S frames of a step packed by the reference into one buffer in layout L; perturb(buffer) may then change it"""
    buf = np.full(S * L.frame_stride, 0x3C, np.uint8)
    pixref.pack_frames(step, L, w, h, buf)
    if perturb:
        perturb(buf)
    return buf


ENC_SIZES = [(176, 144), (208, 120)]  # 208x120 is coded 208x128: the input area is the display size, the planes are cropped


@pytest.mark.parametrize('w,h', ENC_SIZES, ids=[f'{w}x{h}' for w, h in ENC_SIZES])
@pytest.mark.parametrize('case', ['nv12-pitched', 'yuy2', 'i420-tight'])
def test_encode_pix_equals_encode_of_reference_frames(gpu_lib, w, h, case):
    S, nf = 2, 3
    src = _sources(w, h, S, nf)
    if case == 'nv12-pitched':
        L = layout('surface', pixref.NV12, w, h)
        bufs = [_in_layout(st, L, w, h, S) for st in src]
    elif case == 'yuy2':
        L = layout('tight', pixref.YUY2, w, h)
        rng = np.random.default_rng(6400 + w)

        def perturb(buf):  # the odd rows' chroma moves by up to 3: the 4:2:0 chroma is then a computed average
            rows = buf.reshape(S * h, 2 * w)
            d = rng.integers(-3, 4, (S * h // 2, w))
            rows[1::2, 1::2] = np.clip(rows[1::2, 1::2].astype(np.int32) + d, 0, 255).astype(np.uint8)
        bufs = [_in_layout(st, L, w, h, S, perturb) for st in src]
    else:
        L = pixref.tight(pixref.I420, w, h)
        bufs = [np.ascontiguousarray(st).ravel() for st in src]
    ref = [pixref.unpack_frames(b, L, w, h, S) for b in bufs]
    if case == 'yuy2':
        assert not np.array_equal(ref[0], src[0]), 'the perturbation changed nothing: the average is not exercised'
        want = _run(w, h, 300000, S, ref, lambda e, f: e.encode(f))
    else:
        assert all(np.array_equal(r, s) for r, s in zip(ref, src))
        want = _plain(w, h, S, nf)  # with the tight I420 layout: encode() on the same frames
    got = _run(w, h, 300000, S, bufs, lambda e, f: e.encode_pix(f, _lay(L)))
    for t in range(nf):
        for s in range(S):
            assert len(got[t]['nal'][s]) > 0
            assert got[t]['nal'][s] == want[t]['nal'][s], f'frame {t} stream {s}: NAL bytes'
            assert got[t]['rc'][s] == want[t]['rc'][s], f'frame {t} stream {s}: rate-control state'
            assert got[t]['qp'][s] == want[t]['qp'][s], f'frame {t} stream {s}: last_qp'


def test_encode_pix_blends_the_overlays_after_the_conversion(gpu_lib):
    import torch
    import h264mi
    w, h, S, nf = 176, 144, 2, 3
    src = _sources(w, h, S, nf)
    L = layout('surface', pixref.NV12, w, h)
    bufs = [_in_layout(st, L, w, h, S) for st in src]
    sprite = torch.from_numpy(np.random.default_rng(6500).integers(0, 256, h264mi.i420a_bytes(16, 16), dtype=np.uint8)).cuda()
    ov = [h264mi.Overlay(0, 0, 0, 0, 16, 16, 20, 8, 256, 0)]

    def prepare(enc):
        enc.set_overlays(sprite, 16, 16, 1, ov)
        assert enc.overlays() == 1

    got = _run(w, h, 300000, S, bufs, lambda e, f: e.encode_pix(f, _lay(L)), prepare=prepare)
    want = _run(w, h, 300000, S, src, lambda e, f: e.encode(f), prepare=prepare)
    plain = _plain(w, h, S, nf)
    for t in range(nf):
        assert got[t]['nal'] == want[t]['nal'] and got[t]['rc'] == want[t]['rc'] and got[t]['qp'] == want[t]['qp'], f'frame {t}'
    assert got[0]['nal'][0] != plain[0]['nal'][0], 'the overlay changed nothing: the test shows nothing'


def test_encode_pix_refusals_leave_the_encoder_untouched(gpu_lib):
    import torch
    w, h, S = 176, 144, 2
    src = _sources(w, h, S, 1)[0]
    fresh = _plain(w, h, S, 3)[0]
    L = layout('surface', pixref.NV12, w, h)
    other = torch.zeros(S * L.frame_stride, dtype=torch.uint8, device='cuda')

    def feed(enc, frames):
        fn = enc._L.h264mi_enc_encode_pix
        p, r = ctypes.c_void_p(other.data_ptr()), ctypes.byref(_lay(L))
        assert fn(enc._e, None, r) == -1 and fn(enc._e, p, None) == -1
        for kind, ww, hh in (('tight', w - 2, h), ('tight', w, h - 2)):  # a layout that does not hold the encoder's size
            bad = layout(kind, pixref.NV12, ww, hh)
            assert fn(enc._e, p, ctypes.byref(_lay(bad))) == -1
        bad = layout('surface', pixref.NV12, w, h); bad.frame_stride = 0
        with pytest.raises(ValueError):
            enc.encode_pix(other, _lay(bad))
        inp = enc._L.h264mi_enc_input_buffer(enc._e)  # frames that overlap the encoder's input area
        fb = pixref.frame_bytes(w, h)
        for off in (0, S * fb - 1, -(S * L.frame_stride - 1)):
            assert fn(enc._e, ctypes.c_void_p(inp + off), r) == -1, off
        enc.encode(frames)

    got = _run(w, h, 300000, S, [src], feed)[0]
    assert got['nal'] == fresh['nal'] and got['rc'] == fresh['rc']


# ---------------------------------------------------------------- the decoder's output layout


def _decode(dec, ptrs, sizes, nbytes, m):
    """one decode_frames call into m fresh guarded buffers of nbytes: (the whole allocations as arrays, got)"""
    import torch
    bufs = [_guarded(nbytes) for _ in range(m)]
    got = torch.full((m,), 7, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()  # the fills run on torch's stream, the decoder on its own
    dec.decode_frames(ptrs, nal_sizes=sizes, out_ptrs=[b[1].data_ptr() for b in bufs], got_ptrs=[got[i:i + 1].data_ptr() for i in range(m)])
    torch.cuda.synchronize()
    return [b[0].cpu().numpy() for b in bufs], got.cpu().tolist()


def _want_out(pic, L, w, h):
    want = np.full(pixref.span(L, w, h) + 2 * GUARD, FILL, np.uint8)
    if pic is not None:
        pixref.pack(pic, L, w, h, want[GUARD:GUARD + pixref.span(L, w, h)])
    return want


@functools.lru_cache(maxsize=None)
def _oracle_pictures(oracle, w, h, br, S):
    from test_gpu_rgba import NFRAMES, _encoded
    _, nals = _encoded(w, h, br, S)
    ods = [oracle.decoder() for _ in range(S)]
    pics = []
    for f in range(NFRAMES):
        row = []
        for s in range(S):
            rc, pic, pw, ph = ods[s].decode(nals[f][s])
            assert rc == 1 and (pw, ph) == (w, h)
            row.append(pic)
        pics.append(row)
    return nals, pics


@pytest.mark.parametrize('case', ['nv12-pitched', 'yuy2'])
def test_decoder_output_layout(gpu_lib, oracle, case):
    """208x120 is cropped from the coded 208x128: the crop origin and the coded strides are in play"""
    import h264mi
    from test_gpu_rgba import NFRAMES, _nal_tensors
    w, h, br, S = 208, 120, 500000, 2
    nals, pics = _oracle_pictures(oracle, w, h, br, S)
    m = NFRAMES * S
    dev, ptrs, sizes = _nal_tensors(nals)
    L = layout('surface', pixref.NV12, w, h) if case == 'nv12-pitched' else layout('pitch13', pixref.YUY2, w, h)
    span = pixref.span(L, w, h)

    dec = h264mi.BatchDecoder(w, h, S, max_frames=NFRAMES)
    assert dec.output_format() == 'i420' and dec.output_layout() is None
    dec.set_output_format('rgba')
    dec.set_output_layout(_lay(L))
    assert dec.output_format() == 'layout'
    o = dec.output_layout()
    assert (o.pix, list(o.pitch), list(o.offset), o.frame_stride) == (L.pix, L.pitch, L.offset, L.frame_stride)
    for bad in (layout('tight', L.pix, w - 2, h), layout('tight', L.pix, w, h - 2)):  # not the decoder's size: nothing changes
        with pytest.raises(ValueError):
            dec.set_output_layout(_lay(bad))
    assert dec.output_format() == 'layout' and list(dec.output_layout().pitch) == L.pitch
    wholes, got = _decode(dec, ptrs, sizes, span, m)
    assert got == [1] * m
    for f in range(NFRAMES):
        for s in range(S):
            want = _want_out(pics[f][s], L, w, h)
            assert np.array_equal(wholes[f * S + s], want), f'frame {f} stream {s}: {int((wholes[f * S + s] != want).sum())} bytes differ'
    dec.close()

    # a fresh decoder; stream 1's frame 1 is an access unit of size 0: no picture, buffer untouched
    dec = h264mi.BatchDecoder(w, h, S, max_frames=NFRAMES)
    dec.set_output_layout(_lay(L))
    _, _, sizes0 = _nal_tensors(nals, skip={(1, 1)})
    wholes, got = _decode(dec, ptrs, sizes0, span, m)
    assert got[1 * S + 1] == 0 and (wholes[1 * S + 1] == FILL).all()
    for f in range(NFRAMES):  # stream 0 is unaffected
        assert got[f * S] == 1 and np.array_equal(wholes[f * S], _want_out(pics[f][0], L, w, h)), f'frame {f} stream 0'

    # the same decoder back to the format (the streams again from their IDR): the setting is per call, the last setter wins
    dec.set_output_format('i420')
    assert dec.output_format() == 'i420' and dec.output_layout() is None
    fi = pixref.frame_bytes(w, h)
    wholes, got = _decode(dec, ptrs, sizes, fi, m)
    assert got == [1] * m
    for f in range(NFRAMES):
        for s in range(S):
            assert np.array_equal(wholes[f * S + s][GUARD:GUARD + fi], pics[f][s]), f'I420 frame {f} stream {s}'
            assert (wholes[f * S + s][:GUARD] == FILL).all() and (wholes[f * S + s][GUARD + fi:] == FILL).all()
    dec.set_output_format('rgba')
    dec.set_output_layout(_lay(L))
    dec.set_output_layout(None)  # back to the format set last
    assert dec.output_format() == 'rgba' and dec.output_layout() is None
    with pytest.raises(ValueError):
        dec.set_output_format('nv12')
    assert dec.output_format() == 'rgba'
    dec.close()
    del dev
