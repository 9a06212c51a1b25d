"""GPU: the deeper and wider pixel layouts (ids 16..24: I422, I444, NV16, Y800, P010, I010, P210, I210, V210) -- the
standalone calls, the depth rules of h264mi_pixopt, the encoder's input and the decoder's output layout -- against
tests/pixdeepref.py. Every comparison is equality of bytes. Every destination is filled with 0xA5 and sits between 64
guard bytes; after a pack the whole allocation -- guards, pitch padding, the gaps between planes and frames -- must equal
the reference's pack into an equally filled buffer. A lane's piece is 16 bytes of the side with the most bytes per sample
(8 samples of a 16-bit row, a run of 8 groups = 48 pixels of V210) and a wave reaches 64 of them (csrc/pixdeep.hip),
which the shapes below are chosen around."""
import ctypes
import functools

import numpy as np
import pytest

import pixdeepref as R
import pixref
from test_gpu_pix import FILL, GUARD, _decode, _device, _guarded, _oracle_pictures, _plain, _run, _sources

pytestmark = pytest.mark.gpu

N = 3
IDS = [R.NAMES[p] for p in R.ALL]


def _lay(L):
    import h264mi
    return h264mi.PixLayout(L.pix, L.pitch, L.offset, L.frame_stride)


def _opt(depth):
    import h264mi
    return None if depth is None else h264mi.PixOpt(depth)


def _up(x, a):
    return (x + a - 1) // a * a


def layout(kind, pix, w, h):
    """'tight', or 'gapped': every pitch 13 bytes above the row bytes rounded up to the unit (rows at changing alignments),
    the planes in reverse order with a gap of 5 units before each and 3 units after the last"""
    if kind == 'tight':
        return R.tight(pix, w, h)
    u = R.unit(pix)
    pl = R.planes(pix, w, h)
    pitch = [_up(rb + 13, u) for rb, _ in pl]
    offset, at = [0] * len(pl), 0
    for p in reversed(range(len(pl))):
        at += 5 * u
        offset[p] = at
        at += pl[p][1] * pitch[p]
    return pixref.Layout(pix, pitch, offset, at + 3 * u)


@functools.lru_cache(maxsize=None)
def _frames(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (N, pixref.frame_bytes(w, h)), dtype=np.uint8)  # shared: never written


def _pack(src, L, w, h, shift=0, n=N):
    """the standalone pack of the n frames src: the whole destination allocation (guards included) as an array; the
    layout side sits `shift` bytes into its allocation, the I420 side at an odd address when shift is not a multiple of 16"""
    import h264mi
    nb = n * L.frame_stride
    d_src = _device(src, 1 if shift % 16 else 0)
    whole, dst = _guarded(nb, shift)
    assert dst.data_ptr() % 16 == shift % 16
    h264mi.i420_to_pix(dst, _lay(L), d_src, w, h, n)
    return whole.cpu().numpy()


def _want_pack(src, L, w, h, shift=0, n=N):
    nb = n * L.frame_stride
    want = np.full(shift + nb + 2 * GUARD, FILL, np.uint8)
    R.pack_frames(src, L, w, h, want[shift + GUARD:shift + GUARD + nb])
    return want


def _unpack(buf, L, w, h, depth=None, shift=0, n=N):
    """the standalone unpack of the n frames in buf under a depth rule (None: no opt): (the n tight frames, the whole allocation)"""
    import h264mi
    fb = pixref.frame_bytes(w, h)
    d_src = _device(buf, shift)
    assert d_src.data_ptr() % 16 == shift % 16
    whole, dst = _guarded(n * fb, 1 if shift % 16 else 0)
    h264mi.pix_to_i420(dst, d_src, _lay(L), w, h, n, opt=_opt(depth))
    return dst.cpu().numpy().reshape(n, fb), whole.cpu().numpy()


def _depths(pix):
    return (None, R.ROUND, R.DITHER, R.TRUNC) if pix in R.TEN_BIT else (None, R.DITHER)  # the option is ignored for 8 bits


# 2x2: the smallest; 6x2: one V210 group; 14x6, 16x4: w % 6 = 2 and 4, partial groups; 130x66: unaligned rows, more than
# one piece a lane and more than one strip, w % 16 != 0; 1040x4: rows longer than one wave pass of 16-bit samples (64 x 8)
SHAPES = [(2, 2), (6, 2), (14, 6), (16, 4), (130, 66), (1040, 4)]


@pytest.mark.parametrize('pix', R.ALL, ids=IDS)
@pytest.mark.parametrize('w,h', SHAPES, ids=[f'{w}x{h}' for w, h in SHAPES])
def test_pack_and_unpack_vs_reference(gpu_lib, w, h, pix):
    u = R.unit(pix)
    src = _frames(w, h, 8000 + w + 3 * h)
    for kind, shift in (('tight', 0), ('gapped', 0), ('tight', u), ('gapped', u), ('tight', 16), ('gapped', 16)):
        L = layout(kind, pix, w, h)
        assert R.layout_ok(L, w, h)
        got, want = _pack(src, L, w, h, shift), _want_pack(src, L, w, h, shift)
        assert np.array_equal(got, want), f'pack {kind} +{shift}: {int((got != want).sum())} bytes differ, the first at {int(np.argmax(got != want))}'
        # the layout -> I420 from a buffer whose every byte is random: averages are computed, uninformative bits are set
        nb = N * L.frame_stride
        buf = np.random.default_rng(8100 + w + 3 * h + pix).integers(0, 256, nb, dtype=np.uint8)
        for depth in _depths(pix) if shift == 0 else (R.DITHER,):
            got, whole = _unpack(buf, L, w, h, depth, shift)
            want = R.unpack_frames(buf, L, w, h, N, R.ROUND if depth is None else depth)
            assert np.array_equal(got, want), f'unpack {kind} +{shift} depth {depth}: {int((got != want).sum())} bytes differ'
            fb = N * pixref.frame_bytes(w, h)
            s = 1 if shift % 16 else 0
            assert (whole[:s + GUARD] == FILL).all() and (whole[s + GUARD + fb:] == FILL).all(), 'bytes outside the frames were written'


@pytest.mark.parametrize('pix', R.TEN_BIT, ids=[R.NAMES[p] for p in R.TEN_BIT])
def test_uninformative_bits_are_ignored(gpu_lib, pix):
    """random 16-bit words: the low six bits of P010/P210, the high six of I010/I210, bits 31..30 of V210 are set; the same
    frames with those bits cleared give the same I420"""
    w, h = 50, 6
    L = layout('tight', pix, w, h)
    buf = np.random.default_rng(8200 + pix).integers(0, 256, N * L.frame_stride, dtype=np.uint8)
    words = buf.view('<u4' if pix == R.V210 else '<u2')
    junk = 0xC0000000 if pix == R.V210 else 0x003F if pix in (R.P010, R.P210) else 0xFC00
    assert (words & junk).any()
    clean = (words & ~np.array(junk, words.dtype)).view(np.uint8)
    for depth in R.DEPTHS:
        got, _ = _unpack(buf, L, w, h, depth)
        assert np.array_equal(got, R.unpack_frames(buf, L, w, h, N, depth))
        assert np.array_equal(got, R.unpack_frames(clean, L, w, h, N, depth)), 'the reference read an uninformative bit'


def _ramp(pw, ph):
    """a pw x ph plane that holds every value 0..1023 at each of the four (x & 1, y & 1) positions"""
    y, x = np.mgrid[0:ph, 0:pw]
    v = ((y >> 1) * (pw // 2) + (x >> 1)) & 1023
    for px in (0, 1):
        for py in (0, 1):
            assert set(v[py::2, px::2].ravel()) == set(range(1024))
    return v.astype(np.int64)


@pytest.mark.parametrize('pix', R.TEN_BIT, ids=[R.NAMES[p] for p in R.TEN_BIT])
def test_depth_rules_on_a_ramp(gpu_lib, pix):
    """128x128: the 64x64 4:2:0 chroma planes, and every 64x64 quarter of luma, hold every 10-bit value at every dither
    position. 4:2:2 chroma rows 2y and 2y + 1 are equal, so their average is the ramp"""
    w = h = 128
    Y, C = _ramp(w, h), _ramp(w // 2, h // 2)
    Cb, Cr = C, 1023 - C
    L = R.tight(pix, w, h)
    buf = np.zeros(L.frame_stride, np.uint8)
    if pix == R.V210:
        R._v210_write(R._rows(buf, L, 0, *R.planes(pix, w, h)[0]), Y, np.repeat(Cb, 2, axis=0), np.repeat(Cr, 2, axis=0), w, h)
    else:
        sh = 6 if pix in (R.P010, R.P210) else 0
        if pix in (R.P210, R.I210):
            Cb, Cr = np.repeat(Cb, 2, axis=0), np.repeat(Cr, 2, axis=0)
        if pix in (R.P010, R.P210):
            il = np.zeros((Cb.shape[0], w), np.int64)
            il[:, 0::2], il[:, 1::2] = Cb, Cr
            planes = [Y, il]
        else:
            planes = [Y, Cb, Cr]
        buf = np.concatenate([(p << sh).astype('<u2').ravel() for p in planes]).view(np.uint8)
    assert buf.size == L.frame_stride
    ref = {d: R.unpack(buf, L, w, h, d) for d in R.DEPTHS}
    top = (Y >= 1021).ravel()
    assert top.any() and (ref[R.ROUND][:w * h][(Y >= 1022).ravel()] == 255).all() and ((Y[Y >= 1022] + 2) >> 2 == 256).all(), 'the clamp at 255 occurs'
    assert (ref[R.ROUND][:w * h][top] == 255).all() and (ref[R.DITHER][:w * h] == 255).any()
    assert (ref[R.ROUND][w * h:] == 255).any(), 'and in chroma'
    for a, b in ((R.ROUND, R.DITHER), (R.ROUND, R.TRUNC), (R.DITHER, R.TRUNC)):
        for lo, hi in ((0, w * h), (w * h, pixref.frame_bytes(w, h))):
            assert not np.array_equal(ref[a][lo:hi], ref[b][lo:hi]), 'two depth rules agree on the ramp: it shows nothing'
    for d in R.DEPTHS:
        got, _ = _unpack(buf, L, w, h, d, n=1)
        assert np.array_equal(got[0], ref[d]), f'depth {d}: {int((got[0] != ref[d]).sum())} bytes differ'
    got, _ = _unpack(buf, L, w, h, None, n=1)
    assert np.array_equal(got[0], ref[R.ROUND]), 'no option means ROUND'


def test_444_and_422_averages_hit_every_residue(gpu_lib):
    w, h = 34, 6
    rng = np.random.default_rng(8300)
    L = R.tight(R.I444, w, h)
    buf = rng.integers(0, 256, N * L.frame_stride, dtype=np.uint8)
    c = buf[:L.frame_stride][w * h:].reshape(2, h, w).astype(np.int64)
    sums = c[:, 0::2, 0::2] + c[:, 0::2, 1::2] + c[:, 1::2, 0::2] + c[:, 1::2, 1::2]
    assert set((sums % 4).ravel()) == {0, 1, 2, 3}
    pairs = c[:, :, 0::2] + c[:, :, 1::2]
    assert set((pairs % 2).ravel()) == {0, 1}, 'horizontal pair sums both odd and even'
    got, _ = _unpack(buf, L, w, h)
    assert np.array_equal(got, R.unpack_frames(buf, L, w, h, N))
    for pix in (R.I422, R.NV16, R.P210, R.I210, R.V210):
        L = R.tight(pix, w, h)
        buf = rng.integers(0, 256, N * L.frame_stride, dtype=np.uint8)
        _, Cb, Cr, sub = R._source(buf, L, w, h)
        assert sub == '422' and set(((Cb[0::2] + Cb[1::2]) % 2).ravel()) == {0, 1} == set(((Cr[0::2] + Cr[1::2]) % 2).ravel())
        for depth in (R.ROUND, R.TRUNC):
            got, _ = _unpack(buf, L, w, h, depth)
            assert np.array_equal(got, R.unpack_frames(buf, L, w, h, N, depth)), R.NAMES[pix]


@pytest.mark.parametrize('case', ['P010-8192x2', 'V210-8192x2', 'I444-pitch65536'])
def test_limits(gpu_lib, case):
    if case == 'I444-pitch65536':
        w, h, pix = 130, 4, R.I444
        L = pixref.Layout(pix, [65536] * 3, [0, 4 * 65536, 8 * 65536], 12 * 65536)
    else:
        w, h, pix = 8192, 2, R.P010 if case[0] == 'P' else R.V210
        L = R.tight(pix, w, h)
    assert R.layout_ok(L, w, h)
    src = _frames(w, h, 8400)[:2]
    got, want = _pack(src, L, w, h, n=2), _want_pack(src, L, w, h, n=2)
    assert np.array_equal(got, want)
    buf = np.random.default_rng(8401).integers(0, 256, 2 * L.frame_stride, dtype=np.uint8)
    got, _ = _unpack(buf, L, w, h, R.DITHER, n=2)
    assert np.array_equal(got, R.unpack_frames(buf, L, w, h, 2, R.DITHER))


@pytest.mark.parametrize('pix', R.ALL, ids=IDS)
def test_round_trip_on_the_device_is_the_identity(gpu_lib, pix):
    w, h = 130, 66
    src = _frames(w, h, 8500)
    L = layout('gapped', pix, w, h)
    packed = _pack(src, L, w, h)[GUARD:GUARD + N * L.frame_stride]
    for depth in R.DEPTHS:
        back, _ = _unpack(packed, L, w, h, depth)
        if pix == R.Y800:
            assert np.array_equal(back[:, :w * h], src[:, :w * h]) and (back[:, w * h:] == 128).all()
        else:
            assert np.array_equal(back, src), depth


def test_repeatability(gpu_lib):
    w, h = 130, 66
    src = _frames(w, h, 8500)
    for pix in (R.I444, R.P010, R.V210):
        L = layout('gapped', pix, w, h)
        assert _pack(src, L, w, h).tobytes() == _pack(src, L, w, h).tobytes()
        buf = np.random.default_rng(8600 + pix).integers(0, 256, N * L.frame_stride, dtype=np.uint8)
        assert _unpack(buf, L, w, h, R.DITHER)[0].tobytes() == _unpack(buf, L, w, h, R.DITHER)[0].tobytes()


def test_refusals_leave_the_destination_untouched(gpu_lib):
    import torch
    import h264mi
    w, h = 36, 18
    fb = pixref.frame_bytes(w, h)
    B = gpu_lib
    to_i420, to_pix, to_opt = B.h264mi_pix_to_i420_dev, B.h264mi_i420_to_pix_dev, B.h264mi_pix_to_i420_opt_dev
    for pix in (R.P010, R.I210, R.V210, R.I444):
        u = R.unit(pix)
        good = layout('gapped', pix, w, h)
        nb = max(N * good.frame_stride, N * fb) + 4096
        s = torch.zeros(nb, dtype=torch.uint8, device='cuda')
        whole, d = _guarded(nb)
        ps, pd = ctypes.c_void_p(s.data_ptr()), ctypes.c_void_p(d.data_ptr())
        r = ctypes.byref(_lay(good))
        for off in range(1, u):  # a misaligned base on the layout's side
            assert to_pix(ctypes.c_void_p(d.data_ptr() + off), r, ps, w, h, N, None) == -1, (pix, off)
            assert to_i420(pd, ctypes.c_void_p(s.data_ptr() + off), r, w, h, N, None) == -1, (pix, off)
        bad = []
        if u > 1:  # the unit rule: a pitch, an offset, a frame_stride
            a = layout('gapped', pix, w, h); a.pitch[0] += u // 2; a.frame_stride += 64 * u
            bad.append(a)
            a = layout('gapped', pix, w, h); a.offset[0] += u // 2
            bad.append(a)
            a = layout('gapped', pix, w, h); a.frame_stride += 1
            bad.append(a)
        for k in (5, 25):
            a = layout('gapped', pix, w, h); a.pix = k
            bad.append(a)
        for L in bad:
            assert not R.layout_ok(L, w, h) or L.pix in (5, 25)
            q = ctypes.byref(_lay(L))
            assert to_pix(pd, q, ps, w, h, N, None) == -1 and to_i420(pd, ps, q, w, h, N, None) == -1, L
            with pytest.raises(ValueError):
                h264mi.i420_to_pix(d, _lay(L), s, w, h, N)
        for opt in (h264mi.PixOpt(3), h264mi.PixOpt(-1), h264mi.PixOpt(1, (0, 0, 7))):  # a bad opt, for 8-bit formats too
            assert to_opt(pd, ps, r, ctypes.byref(opt), w, h, N, None) == -1
            with pytest.raises(ValueError):
                h264mi.pix_to_i420(d, s, _lay(good), w, h, N, opt=opt)
        # overlaps: the layout's side inside the tight frames and the other way round, by one unit at either end
        for off in (0, u, (N * fb - 1) // u * u, -(N * good.frame_stride - u)):
            assert to_pix(ctypes.c_void_p(d.data_ptr() + 2048 + off), r, ctypes.c_void_p(d.data_ptr() + 2048), w, h, N, None) == -1, off
            assert to_i420(ctypes.c_void_p(d.data_ptr() + 2048), ctypes.c_void_p(d.data_ptr() + 2048 + off), r, w, h, N, None) == -1, off
        torch.cuda.synchronize()
        assert (whole.cpu().numpy() == FILL).all(), 'a refused call wrote'
        assert to_pix(pd, r, ps, w, h, N, None) == 0  # and the good call does write
        torch.cuda.synchronize()
        assert (d.cpu().numpy() != FILL).any()


# ---------------------------------------------------------------- the encoder's input

ENC_SIZES = [(176, 144), (208, 120)]


def _enc_case(case, w, h, S, step, rng):
    """(layout, buffer, depth): the S frames of a step in the case's layout, with detail below 8 bits added"""
    if case == 'p010-pitched-dither':
        L = layout('gapped', R.P010, w, h)
        buf = R.pack_frames(step, L, w, h, np.full(S * L.frame_stride, 0x3C, np.uint8))
        buf[0::2] = rng.integers(0, 256, buf.size // 2, dtype=np.uint8)  # the low byte of every word: two bits of value, six of junk
        return L, buf, R.DITHER
    if case == 'v210-tight':
        L = R.tight(R.V210, w, h)
        buf = R.pack_frames(step, L, w, h, np.full(S * L.frame_stride, 0x3C, np.uint8))
        words = buf.view('<u4')
        words ^= rng.integers(0, 1 << 32, words.size, dtype=np.uint32) & np.uint32(0xC0300C03)  # two low bits a field, bits 31..30
        return L, buf, None
    L = R.tight(R.I444, w, h)
    buf = R.pack_frames(step, L, w, h, np.zeros(S * L.frame_stride, np.uint8))
    buf[:] = np.clip(buf.astype(np.int32) + rng.integers(-3, 4, buf.size), 0, 255).astype(np.uint8)  # the 2x2 means are computed
    return L, buf, None


@pytest.mark.parametrize('w,h', ENC_SIZES, ids=[f'{w}x{h}' for w, h in ENC_SIZES])
@pytest.mark.parametrize('case', ['p010-pitched-dither', 'v210-tight', 'i444'])
def test_encode_pix_equals_encode_of_reference_frames(gpu_lib, w, h, case):
    import h264mi
    S, nf = 2, 3
    src = _sources(w, h, S, nf)
    rng = np.random.default_rng(8700 + w)
    cases = [_enc_case(case, w, h, S, st, rng) for st in src]
    L, depth = cases[0][0], cases[0][2]
    bufs = [c[1] for c in cases]
    ref = [R.unpack_frames(b, L, w, h, S, R.ROUND if depth is None else depth) for b in bufs]
    assert not np.array_equal(ref[0], src[0]), 'the perturbation changed nothing'
    if depth is not None:
        assert not np.array_equal(ref[0], R.unpack_frames(bufs[0], L, w, h, S, R.ROUND)), 'the depth rule changes nothing here'

    def prepare(enc):
        assert enc.pixopt().depth == 0
        if depth is not None:
            enc.set_pixopt(h264mi.PixOpt(depth))
            assert enc.pixopt().depth == depth

    want = _run(w, h, 300000, S, ref, lambda e, f: e.encode(f))
    got = _run(w, h, 300000, S, bufs, lambda e, f: e.encode_pix(f, _lay(L)), prepare=prepare)
    for t in range(nf):
        for s in range(S):
            assert len(got[t]['nal'][s]) > 0
            assert got[t]['nal'][s] == want[t]['nal'][s], f'frame {t} stream {s}: NAL bytes'
            assert got[t]['rc'][s] == want[t]['rc'][s], f'frame {t} stream {s}: rate-control state'
            assert got[t]['qp'][s] == want[t]['qp'][s], f'frame {t} stream {s}: last_qp'


def test_set_pixopt_none_restores_and_a_refused_one_changes_nothing(gpu_lib):
    import h264mi
    w, h, S, nf = 176, 144, 2, 3
    src = _sources(w, h, S, nf)
    rng = np.random.default_rng(8800)
    cases = [_enc_case('p010-pitched-dither', w, h, S, st, rng) for st in src]
    L = cases[0][0]
    bufs = [c[1] for c in cases]

    def restore(enc):
        enc.set_pixopt(h264mi.PixOpt(R.TRUNC))
        enc.set_pixopt(None)
        assert enc.pixopt().depth == 0 and list(enc.pixopt().reserved) == [0, 0, 0]

    def refuse(enc):
        enc.set_pixopt(h264mi.PixOpt(R.TRUNC))
        for bad in (h264mi.PixOpt(3), h264mi.PixOpt(-1), h264mi.PixOpt(0, (1, 0, 0))):
            with pytest.raises(ValueError):
                enc.set_pixopt(bad)
        assert enc.pixopt().depth == R.TRUNC

    feed = lambda e, f: e.encode_pix(f, _lay(L))
    by_rule = {d: _run(w, h, 300000, S, [R.unpack_frames(b, L, w, h, S, d) for b in bufs], lambda e, f: e.encode(f)) for d in (R.ROUND, R.TRUNC)}
    assert by_rule[R.ROUND][0]['nal'] != by_rule[R.TRUNC][0]['nal'], 'the two rules code the same bytes: the test shows nothing'
    for prepare, d in ((restore, R.ROUND), (refuse, R.TRUNC)):
        got = _run(w, h, 300000, S, bufs, feed, prepare=prepare)
        for t in range(nf):
            assert got[t]['nal'] == by_rule[d][t]['nal'] and got[t]['rc'] == by_rule[d][t]['rc'] and got[t]['qp'] == by_rule[d][t]['qp'], (d, t)


def test_encode_pix_blends_the_overlays_after_the_conversion(gpu_lib):
    import torch
    import h264mi
    w, h, S, nf = 176, 144, 2, 3
    src = _sources(w, h, S, nf)
    L = layout('gapped', R.I210, w, h)
    bufs = [R.pack_frames(st, L, w, h, np.full(S * L.frame_stride, 0x3C, np.uint8)) for st in src]
    sprite = torch.from_numpy(np.random.default_rng(8900).integers(0, 256, h264mi.i420a_bytes(16, 16), dtype=np.uint8)).cuda()
    ov = [h264mi.Overlay(0, 0, 0, 0, 16, 16, 20, 8, 256, 0)]

    def prepare(enc):
        enc.set_overlays(sprite, 16, 16, 1, ov)

    got = _run(w, h, 300000, S, bufs, lambda e, f: e.encode_pix(f, _lay(L)), prepare=prepare)
    want = _run(w, h, 300000, S, src, lambda e, f: e.encode(f), prepare=prepare)
    plain = _plain(w, h, S, nf)
    for t in range(nf):
        assert got[t]['nal'] == want[t]['nal'] and got[t]['rc'] == want[t]['rc'] and got[t]['qp'] == want[t]['qp'], f'frame {t}'
    assert got[0]['nal'][0] != plain[0]['nal'][0], 'the overlay changed nothing: the test shows nothing'


# ---------------------------------------------------------------- the decoder's output layout


def _want_out(pic, L, w, h):
    want = np.full(R.span(L, w, h) + 2 * GUARD, FILL, np.uint8)
    R.pack(pic, L, w, h, want[GUARD:GUARD + R.span(L, w, h)])
    return want


@pytest.mark.parametrize('case', ['p010-pitched', 'i422'])
def test_decoder_output_layout(gpu_lib, oracle, case):
    """208x120 is cropped from the coded 208x128: the crop origin and the coded strides are in play"""
    import h264mi
    from test_gpu_rgba import NFRAMES, _nal_tensors
    w, h, br, S = 208, 120, 500000, 2
    nals, pics = _oracle_pictures(oracle, w, h, br, S)
    m = NFRAMES * S
    dev, ptrs, sizes = _nal_tensors(nals)
    L = layout('gapped', R.P010, w, h) if case == 'p010-pitched' else R.tight(R.I422, w, h)
    span = R.span(L, w, h)
    dec = h264mi.BatchDecoder(w, h, S, max_frames=NFRAMES)
    dec.set_output_layout(_lay(L))
    assert dec.output_format() == 'layout'
    bad = layout('gapped', R.P010, w, h)  # breaks the unit rule: refused, and the setting stays
    bad.pitch[1] += 1
    assert not R.layout_ok(bad, w, h)
    with pytest.raises(ValueError):
        dec.set_output_layout(_lay(bad))
    o = dec.output_layout()
    assert (o.pix, list(o.pitch), list(o.offset), o.frame_stride) == (L.pix, L.pitch, L.offset, L.frame_stride)
    wholes, got = _decode(dec, ptrs, sizes, span, m)
    assert got == [1] * m
    for f in range(NFRAMES):
        for s in range(S):
            want = _want_out(pics[f][s], L, w, h)
            assert np.array_equal(wholes[f * S + s], want), f'frame {f} stream {s}: {int((wholes[f * S + s] != want).sum())} bytes differ'
    dec.close()
    del dev
