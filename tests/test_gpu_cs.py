"""GPU: colour specifications at the RGBA edges -- the standalone calls h264mi_rgba_to_i420_cs_dev, h264mi_i420_to_rgba_cs_dev
and h264mi_rgba_to_i420a_cs_dev, the encoder's RGBA input under h264mi_enc_set_colorspec and the decoder's RGBA output under
h264mi_dec_set_output_colorspec -- against tests/csref.py. Every comparison is equality of bytes. Every destination is
filled with 0xA5 and sits between 64 guard bytes of 0xA5; the whole allocation is compared. A lane converts 8 pixels on
2 rows, a wave 512 pixels of a row pair, and the grid is at most 2048 blocks of 256 lanes over min(n, 256) frames
(csrc/colorspace.hip), which the shapes below are chosen around."""
import ctypes
import functools
import os

import numpy as np
import pytest

import csref

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5
N = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, 'oracle', 'build', 'libh264_oracle.so')


def _spec(s):
    import h264mi
    return h264mi.ColorSpec(*s)


def _device(x, shift=0):
    """x's bytes on the device, `shift` bytes into a 64-byte aligned place of a larger allocation"""
    import torch
    whole = torch.zeros(x.size + shift + 128, dtype=torch.uint8, device='cuda')
    view = whole[GUARD + shift:GUARD + shift + x.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(x).ravel()))
    return view


def _guarded(nbytes, shift=0):
    """(whole, view): a destination of nbytes of 0xA5 between 64 bytes of 0xA5 on each side, `shift` bytes into its allocation"""
    import torch
    whole = torch.full((shift + nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device='cuda')
    return whole, whole[shift + GUARD:shift + GUARD + nbytes]


def _want(body, shift=0):
    want = np.full(shift + body.size + 2 * GUARD, FILL, np.uint8)
    want[shift + GUARD:shift + GUARD + body.size] = body
    return want


def _stride_shape(n):
    """the smallest 8192-wide shape whose units exceed what the grid covers in one pass: blocks = 2048 // min(n, 256) of
    256 lanes over a frame's (w / 8) * (h / 2) units"""
    lanes = (2048 // min(n, 256)) * 256
    return 8192, 2 * (lanes // 1024 + 1)


# (w, h, RGBA shift, I420 shift): each the smallest shape that reaches its case
#   2x2: one chroma sample, every neighbour clamps; 2x16 and 16x2: one chroma column / row; 8x4: one vector unit; 24x6: an
#   interior unit between two others, 3 chroma rows; 36x18: w % 8 != 0, the byte path with a unit that crosses the row's
#   end; 520x4: a row longer than one wave's 512 pixels; 130x66 with every buffer at the smallest misalignment it allows
#   (I420 at an odd address, RGBA at 4 mod 16); a second pass of the stride loop; 8192x2 and 2x8192: the limits
SHAPES = [(2, 2, 0, 0), (2, 16, 0, 0), (16, 2, 0, 0), (8, 4, 0, 0), (24, 6, 0, 0), (36, 18, 0, 0), (520, 4, 0, 0), (130, 66, 4, 1),
          _stride_shape(N) + (0, 0), (8192, 2, 0, 0), (2, 8192, 0, 0)]
SHAPE_IDS = [f'{c[0]}x{c[1]}' + ('-misaligned' if c[2] else '') for c in SHAPES]
TABLE_IDS = [csref.NAMES[k] for k in csref.TABLES]


assert (SHAPES[8][0] // 8) * (SHAPES[8][1] // 2) > (2048 // N) * 256 >= (SHAPES[8][0] // 8) * (SHAPES[8][1] // 2 - 1), 'a second pass, barely'


@functools.lru_cache(maxsize=4)
def _inputs(w, h):
    """N RGBA frames (uniform random bytes, alpha included, the cube's corners in front) and N I420 frames (uniform random:
    full-range YUV reaches both clamps of every channel). Shared by the specs of a shape: never written"""
    rng = np.random.default_rng(7400 + 3 * w + h)
    rgba = rng.integers(0, 256, (N, w * h, 4), dtype=np.uint8)
    for c in range(min(8, w * h)):
        rgba[:, c, :3] = [255 * (c & 1), 255 * ((c >> 1) & 1), 255 * ((c >> 2) & 1)]
    yuv = rng.integers(0, 256, (N, csref.frame_bytes(w, h)), dtype=np.uint8)
    return rgba.reshape(N, w * h * 4), yuv


@pytest.mark.parametrize('mode', (0, 1), ids=('topleft-repeat', 'average-bilinear'))
@pytest.mark.parametrize('key', csref.TABLES, ids=TABLE_IDS)
@pytest.mark.parametrize('w,h,srgba,si420', SHAPES, ids=SHAPE_IDS)
def test_conversions_vs_reference(gpu_lib, w, h, srgba, si420, key, mode):
    import torch
    import h264mi
    spec = csref.Spec(*key, mode, mode)
    rgba, yuv = _inputs(w, h)
    fr, fi = w * h * 4, csref.frame_bytes(w, h)
    # RGBA -> I420
    src = _device(rgba, srgba)
    whole, dst = _guarded(N * fi, si420)
    if srgba:
        assert src.data_ptr() % 16 == 4 and dst.data_ptr() % 2 == 1
    h264mi.rgba_to_i420(dst, src, w, h, N, spec=_spec(spec))
    torch.cuda.synchronize()
    got, want = whole.cpu().numpy(), _want(csref.frames(csref.rgba_to_i420, rgba, w, h, N, spec), si420)
    assert np.array_equal(got, want), f'rgba->i420: {int((got != want).sum())} bytes differ'
    # I420 -> RGBA
    src = _device(yuv, si420)
    whole, dst = _guarded(N * fr, srgba)
    if srgba:
        assert dst.data_ptr() % 16 == 4 and src.data_ptr() % 2 == 1
    h264mi.i420_to_rgba(dst, src, w, h, N, spec=_spec(spec))
    torch.cuda.synchronize()
    got, want = whole.cpu().numpy(), _want(csref.frames(csref.i420_to_rgba, yuv, w, h, N, spec), srgba)
    assert np.array_equal(got, want), f'i420->rgba: {int((got != want).sum())} bytes differ'


@pytest.mark.parametrize('w,h,srgba,si420', [(36, 18, 0, 0), (24, 6, 0, 0), (130, 66, 4, 1)], ids=['36x18', '24x6', '130x66-misaligned'])
def test_default_spec_gives_the_old_calls_bytes(gpu_lib, w, h, srgba, si420):
    import torch
    import h264mi
    rgba, yuv = _inputs(w, h)
    fr, fi, fa = w * h * 4, csref.frame_bytes(w, h), csref.i420a_bytes(w, h)
    for fn, src_np, ssrc, nb, sdst in ((h264mi.rgba_to_i420, rgba, srgba, N * fi, si420), (h264mi.i420_to_rgba, yuv, si420, N * fr, srgba),
                                       (h264mi.rgba_to_i420a, rgba, srgba, N * fa, si420)):
        src = _device(src_np, ssrc)
        old, dold = _guarded(nb, sdst)
        new, dnew = _guarded(nb, sdst)
        fn(dold, src, w, h, N)
        fn(dnew, src, w, h, N, spec=_spec(csref.DEFAULT))
        torch.cuda.synchronize()
        assert np.array_equal(old.cpu().numpy(), new.cpu().numpy()), fn.__name__
        assert not (dold.cpu().numpy() == FILL).all()


@pytest.mark.parametrize('w,h', [(2, 2), (36, 18), (64, 4)], ids=['2x2', '36x18', '64x4'])
def test_sprites_vs_reference(gpu_lib, w, h):
    import torch
    import h264mi
    rgba, _ = _inputs(w, h)
    fa = csref.i420a_bytes(w, h)
    src = _device(rgba)
    for key in csref.TABLES:
        for down in (csref.TOPLEFT, csref.AVERAGE):
            spec = csref.Spec(*key, down, 0)
            whole, dst = _guarded(N * fa, 1)  # sprites sit at any alignment
            h264mi.rgba_to_i420a(dst, src, w, h, N, spec=_spec(spec))
            torch.cuda.synchronize()
            got, want = whole.cpu().numpy(), _want(csref.frames(csref.rgba_to_i420a, rgba, w, h, N, spec), 1)
            assert np.array_equal(got, want), (spec, int((got != want).sum()))
            out = dst.cpu().numpy().reshape(N, fa)
            assert np.array_equal(out[:, fa - w * h:], rgba.reshape(N, w * h, 4)[:, :, 3]), 'A is the fourth bytes'
            assert np.array_equal(out[:, :fa - w * h], csref.frames(csref.rgba_to_i420, rgba, w, h, N, spec).reshape(N, -1)), 'Y, Cb, Cr as rgba_to_i420_cs'


# ---------------------------------------------------------------- the encoder's RGBA input

EW, EH, ES, ENF, EBR = 40, 24, 2, 3, 200000  # coded 48x32: the input area is the display size


@functools.lru_cache(maxsize=None)
def _enc_rgba():
    from golden.make_golden import rgba_frame
    return [[rgba_frame(EW, EH, 700 + 10 * s + f).reshape(-1) for s in range(ES)] for f in range(ENF)]


def _encode(feed):
    """ENF frame steps of a fresh 2-stream encoder, feed(enc, f) enqueueing frame f: every stream's NAL bytes per frame"""
    import h264mi
    enc = h264mi.BatchEncoder(EW, EH, EBR, ES)
    enc.set_frame_skip(False)
    nals = []
    for f in range(ENF):
        keep = feed(enc, f)  # held until nal_sizes() has synchronised
        sizes = enc.nal_sizes()
        nals.append([enc.nal_bytes(s, sizes[s]) for s in range(ES)])
        del keep
    enc.close()
    return nals


@pytest.mark.parametrize('spec', [csref.Spec(1, 1, 1, 0), csref.Spec(1, 0, 0, 1), csref.Spec(0, 1, 1, 1)], ids=['709-full-average', '709-limited-topleft', '601-full-average'])
def test_encode_rgba_under_a_spec(gpu_lib, spec):
    """frames 0 and 1 under the spec (a refused setter in between), frame 2 after set_colorspec(None): the NAL bytes of
    encode() on csref's I420 of the same RGBA under the spec in force"""
    import torch
    import h264mi
    rgba = _enc_rgba()
    in_force = [spec, spec, csref.DEFAULT]

    def by_rgba(enc, f):
        if f == 0:
            assert tuple(getattr(enc.colorspec(), k) for k in csref.Spec._fields) == (0, 0, 0, 0)
            enc.set_colorspec(_spec(spec))
        if f == 1:
            for k in range(4):
                for bad in (-1, 2):
                    v = list(spec)
                    v[k] = bad
                    with pytest.raises(ValueError):
                        enc.set_colorspec(_spec(v))
            assert tuple(getattr(enc.colorspec(), k) for k in csref.Spec._fields) == tuple(spec), 'a refused setter changes nothing'
        if f == 2:
            enc.set_colorspec(None)
            assert tuple(getattr(enc.colorspec(), k) for k in csref.Spec._fields) == (0, 0, 0, 0)
        frames = torch.from_numpy(np.concatenate(rgba[f])).cuda()
        enc.encode_rgba(frames)
        return frames

    def by_i420(enc, f):
        frames = torch.from_numpy(np.concatenate([csref.rgba_to_i420(rgba[f][s], EW, EH, in_force[f]) for s in range(ES)])).cuda()
        enc.encode(frames)
        return frames

    got, want = _encode(by_rgba), _encode(by_i420)
    for f in range(ENF):
        for s in range(ES):
            assert len(got[f][s]) > 0
            assert got[f][s] == want[f][s], f'frame {f} stream {s}: NAL bytes'
    assert not np.array_equal(csref.rgba_to_i420(rgba[0][0], EW, EH, spec), csref.rgba_to_i420(rgba[0][0], EW, EH)), 'the spec changes nothing: the test shows nothing'


def test_encode_rgba_with_the_default_spec_is_todays(gpu_lib, oracle):
    """never set, set to all zeros, and set then cleared: the NAL bytes of the oracle encoder on the oracle's conversion"""
    import torch
    rgba = _enc_rgba()

    def plain(enc, f):
        frames = torch.from_numpy(np.concatenate(rgba[f])).cuda()
        enc.encode_rgba(frames)
        return frames

    def zeros(enc, f):
        enc.set_colorspec(_spec(csref.Spec(1, 1, 1, 1)))
        enc.set_colorspec(_spec(csref.DEFAULT) if f % 2 else None)
        return plain(enc, f)

    a, b = _encode(plain), _encode(zeros)
    oes = [oracle.encoder(EW, EH, EBR) for _ in range(ES)]
    for oe in oes:
        oe.set_frame_skip(False)
    for f in range(ENF):
        for s in range(ES):
            assert a[f][s] == b[f][s] == oes[s].encode(oracle.rgba_to_i420(rgba[f][s], EW, EH)), f'frame {f} stream {s}'


# ---------------------------------------------------------------- the decoder's RGBA output


@functools.lru_cache(maxsize=None)
def _streams(kind):
    """ENF access units of ES streams of 40x24 pictures coded as 48x32: 'encoder' (cropped right and bottom, the
    encoder's own streams) or 'crop-left-top' (streamgen's syntax with frame_crop_left_offset 1 and frame_crop_top_offset 1:
    the picture starts at luma (2, 2) of the coded one)"""
    if kind == 'encoder':
        import torch
        rgba = _enc_rgba()

        def plain(enc, f):
            frames = torch.from_numpy(np.concatenate(rgba[f])).cuda()
            enc.encode_rgba(frames)
            return frames
        return _encode(plain)
    from streamgen import FastBits, SyntaxGen, nal

    class CropGen(SyntaxGen):
        def sps(self):  # SyntaxGen.sps with all four frame_crop offsets
            w = FastBits()
            w.u(66, 8); w.u(0xC0, 8); w.u(40, 8); w.ue(0)
            w.ue(12)
            w.ue(0); w.ue(12)  # POC type 0, 16-bit lsb
            w.ue(1); w.u(0, 1)
            w.ue(self.mbw - 1); w.ue(self.mbh - 1)
            w.u(1, 1); w.u(1, 1)
            w.u(1, 1)
            w.ue(1); w.ue(3); w.ue(1); w.ue(3)  # left, right, top, bottom: 48 - 2 * 4 = 40, 32 - 2 * 4 = 24
            w.u(0, 1)
            return nal(3, 7, w.rbsp())
    gens = [CropGen(SO, 3, 2, 7600 + s) for s in range(ES)]
    units = [[g.idr() for g in gens]]
    for _ in range(ENF - 1):
        units.append([g.p() for g in gens])
    return units


def _decode(dec, ptrs, sizes, nbytes, m, after=None):
    """one decode_frames call into m fresh guarded buffers of nbytes: (the whole allocations as arrays, got). after():
    called between the enqueue and the synchronise"""
    import torch
    bufs = [_guarded(nbytes) for _ in range(m)]
    got = torch.full((m,), 7, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()  # the fills run on torch's stream, the decoder on its own
    dec.decode_frames(ptrs, nal_sizes=sizes, out_ptrs=[b[1].data_ptr() for b in bufs], got_ptrs=[got[i:i + 1].data_ptr() for i in range(m)])
    if after:
        after()
    torch.cuda.synchronize()
    return [b[0].cpu().numpy() for b in bufs], got.cpu().tolist()


def _cs_tuple(dec):
    return tuple(getattr(dec.output_colorspec(), k) for k in csref.Spec._fields)


@pytest.mark.parametrize('kind', ['encoder', 'crop-left-top'])
def test_decoder_rgba_output_under_a_spec(gpu_lib, oracle, kind):
    import h264mi
    from test_gpu_rgba import _nal_tensors
    w, h, S = EW, EH, ES
    nals = _streams(kind)
    m = ENF * S
    fr, fi = w * h * 4, csref.frame_bytes(w, h)
    dev, ptrs, sizes = _nal_tensors(nals)
    X, Z = csref.Spec(1, 1, 0, 1), csref.Spec(0, 0, 1, 1)  # 709 full BILINEAR; 601 limited BILINEAR

    # the cropped I420 pictures of the same call sequence
    dec = h264mi.BatchDecoder(w, h, S, max_frames=ENF)
    assert (dec.cw, dec.ch) == (48, 32)
    wholes, got = _decode(dec, ptrs, sizes, fi, m)
    assert got == [1] * m
    pics = [x[GUARD:GUARD + fi] for x in wholes]
    if kind == 'encoder':  # the oracle decoder agrees (the syntax streams have their own tests)
        ods = [oracle.decoder() for _ in range(S)]
        for f in range(ENF):
            for s in range(S):
                rc, pic, pw, ph = ods[s].decode(nals[f][s])
                assert rc == 1 and (pw, ph) == (w, h) and np.array_equal(pic, pics[f * S + s])
    assert _cs_tuple(dec) == (0, 0, 0, 0)
    dec.close()

    def want(spec, i):
        return _want(csref.i420_to_rgba(pics[i], w, h, spec))

    dec = h264mi.BatchDecoder(w, h, S, max_frames=ENF)
    dec.set_output_colorspec(_spec(X))  # kept while the format is I420, and across the change to RGBA
    assert _cs_tuple(dec) == tuple(X) and dec.output_format() == 'i420'
    dec.set_output_format('rgba')
    assert _cs_tuple(dec) == tuple(X)
    for k in range(4):
        for bad in (-1, 2):
            v = list(X)
            v[k] = bad
            with pytest.raises(ValueError):
                dec.set_output_colorspec(_spec(v))
    assert _cs_tuple(dec) == tuple(X), 'a refused setter changes nothing'
    # the call captures its setting: Z is set after the enqueue, before anything is synchronised
    wholes, got = _decode(dec, ptrs, sizes, fr, m, after=lambda: dec.set_output_colorspec(_spec(Z)))
    assert got == [1] * m
    for i in range(m):
        assert np.array_equal(wholes[i], want(X, i)), f'X: frame {i // S} stream {i % S}: {int((wholes[i] != want(X, i)).sum())} bytes differ'
    assert not np.array_equal(want(X, 0), want(csref.Spec(1, 1, 0, 0), 0)), 'BILINEAR changes nothing: the test shows nothing'
    # the next call (the streams again from their IDR) runs under Z; stream 1's frame 1 is an access unit of size 0
    _, _, sizes0 = _nal_tensors(nals, skip={(1, 1)})
    wholes, got = _decode(dec, ptrs, sizes0, fr, m)
    assert got[1 * S + 1] == 0 and (wholes[1 * S + 1] == FILL).all(), 'no picture: got 0, the buffer untouched'
    for f in range(ENF):  # stream 0 is unaffected
        assert got[f * S] == 1 and np.array_equal(wholes[f * S], want(Z, f * S)), f'Z: frame {f} stream 0'
    # I420 output does not look at the specification
    dec.set_output_format('i420')
    wholes, got = _decode(dec, ptrs, sizes, fi, m)
    assert got == [1] * m and all(np.array_equal(wholes[i], _want(pics[i])) for i in range(m))
    # NULL: the default again, by the kernel of before
    dec.set_output_format('rgba')
    assert _cs_tuple(dec) == tuple(Z)
    dec.set_output_colorspec(None)
    assert _cs_tuple(dec) == (0, 0, 0, 0)
    wholes, got = _decode(dec, ptrs, sizes, fr, m)
    assert got == [1] * m
    for i in range(m):
        assert np.array_equal(wholes[i], _want(oracle.i420_to_rgba(pics[i], w, h))), f'default: frame {i // S} stream {i % S}'
    dec.close()
    del dev


def test_decoder_output_equals_the_standalone_call_on_the_cropped_picture(gpu_lib):
    """REPEAT and BILINEAR of every table on the left-top cropped stream: the bytes of h264mi_i420_to_rgba_cs_dev on the
    cropped tight I420 picture -- interpolation clamps to the crop, never to the coded samples outside it"""
    import torch
    import h264mi
    from test_gpu_rgba import _nal_tensors
    w, h, S = EW, EH, ES
    nals = _streams('crop-left-top')
    m = ENF * S
    fr, fi = w * h * 4, csref.frame_bytes(w, h)
    dev, ptrs, sizes = _nal_tensors(nals)
    dec = h264mi.BatchDecoder(w, h, S, max_frames=ENF)
    wholes, got = _decode(dec, ptrs, sizes, fi, m)
    assert got == [1] * m
    pics = np.stack([x[GUARD:GUARD + fi] for x in wholes])
    d_pics = _device(pics)
    dec.set_output_format('rgba')
    for key in csref.TABLES:
        for up in (csref.REPEAT, csref.BILINEAR):
            spec = csref.Spec(*key, 0, up)
            if spec == csref.DEFAULT:
                continue
            dec.set_output_colorspec(_spec(spec))
            wholes, got = _decode(dec, ptrs, sizes, fr, m)
            _, alone = _guarded(m * fr)
            h264mi.i420_to_rgba(alone, d_pics, w, h, m, spec=_spec(spec))
            torch.cuda.synchronize()
            alone = alone.cpu().numpy().reshape(m, fr)
            for i in range(m):
                assert np.array_equal(wholes[i][GUARD:GUARD + fr], alone[i]), (spec, i)
                assert np.array_equal(alone[i], csref.i420_to_rgba(pics[i], w, h, spec)), (spec, i)
    dec.close()
    del dev
