"""GPU: the temporal denoiser -- the standalone call h264mi_i420_denoise_dev and the encoder's pre-filter
h264mi_enc_set_denoise -- against tests/denoiseref.py. Exact integers, so every comparison is equality of bytes; every
destination sits between 64 guard bytes of 0xA5 that must stay as they were. The kernel's strip is 256 luma samples by
8 rows (csrc/denoise.hip), which the shapes below are chosen around."""
import ctypes
import functools

import numpy as np
import pytest

import denoiseref as ref
import orientref
import qualityref
from test_denoise_host import BAD_PARAMS, BAD_SHAPES, PARAMS, make_pair

pytestmark = pytest.mark.gpu

GUARD = 64
N = 3

# (w, h, shift): each the smallest shape that reaches its case
#   2x2: one partial block, 1x1 chroma; 8x8: exactly one block; 10x6: partial blocks both ways, bw = 2; 16x16: 2x2 whole
#   blocks; 36x18: chroma 18x9, rows that are no multiple of 4 (the byte path for every plane: 36 is no multiple of 8);
#   130x66: one dword past the 128 chroma samples of a 256-sample strip's half, a second strip of one partial block,
#   chroma 65x33; the same at odd addresses: the byte path; 264x10: 8 samples wider than the 256-sample strip, whole 8-byte words, a partial block row; 8192x2 and
#   2x8192: the limit
SHAPES = [(2, 2, 0), (8, 8, 0), (10, 6, 0), (16, 16, 0), (36, 18, 0), (130, 66, 0), (130, 66, 1), (264, 10, 0), (8192, 2, 0), (2, 8192, 0)]
SHAPE_IDS = [f'{w}x{h}' + ('-odd-address' if s else '') for w, h, s in SHAPES]


@functools.lru_cache(maxsize=None)
def _content(w, h):
    """(cur, prev): N frame pairs of different content, as (N, frame bytes) arrays; shared, never written"""
    pairs = [make_pair(w, h, 1000 * f + 3 * w + h) for f in range(N)]
    cur, prev = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    cur.setflags(write=False)
    prev.setflags(write=False)
    return cur, prev


@functools.lru_cache(maxsize=None)
def _reference(w, h, params):
    cur, prev = _content(w, h)
    res = [ref.denoise_frame(cur[f], prev[f], w, h, params) for f in range(N)]
    out = np.stack([r[0] for r in res])
    out.setflags(write=False)
    return out, [r[1] for r in res]


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


def _denoise(cur, prev, w, h, params, shift=0, dst='new', dst2=None, stats=True):
    """the standalone call on N frames. dst, dst2: 'new' (a fresh guarded buffer of 0x5A), 'cur', 'prev' or None.
    Returns (dst bytes, dst2 bytes or None, stats rows or None); every buffer's guards are checked"""
    import torch
    import h264mi
    nb = cur.size
    wc, d_cur = _guarded(cur, shift)
    wp, d_prev = _guarded(prev, shift)
    fresh = np.full(nb, 0x5A, np.uint8)
    bufs = {'cur': (wc, d_cur), 'prev': (wp, d_prev)}
    wd, d_dst = bufs[dst] if dst != 'new' else _guarded(fresh, shift)
    wd2, d_dst2 = (None, None) if dst2 is None else bufs[dst2] if dst2 != 'new' else _guarded(fresh, shift)
    if shift:
        assert all(t.data_ptr() % 2 == 1 for t in (d_cur, d_prev, d_dst))
    d_stats = torch.full((4 * N,), 0x7FFFFFFF, dtype=torch.int32, device='cuda') if stats else None
    h264mi.i420_denoise(d_dst, d_cur, d_prev, w, h, N, params, dst2=d_dst2, stats=d_stats)
    torch.cuda.synchronize()
    out = d_dst.cpu().numpy().reshape(N, -1)
    out2 = d_dst2.cpu().numpy().reshape(N, -1) if d_dst2 is not None else None
    for whole in (wc, wp, wd) + ((wd2,) if wd2 is not None else ()):
        assert _guards_intact(whole, nb, shift), 'bytes outside the frames were written'
    if dst != 'cur' and dst2 != 'cur':
        assert np.array_equal(d_cur.cpu().numpy(), cur.ravel()), 'the current frames were written'
    if dst != 'prev' and dst2 != 'prev':
        assert np.array_equal(d_prev.cpu().numpy(), prev.ravel()), 'the previous frames were written'
    st = d_stats.cpu().numpy().astype(np.int64).reshape(N, 4).tolist() if stats else None
    return out, out2, st


@pytest.mark.parametrize('params', PARAMS, ids=[str(p) for p in PARAMS])
@pytest.mark.parametrize('w,h,shift', SHAPES, ids=SHAPE_IDS)
def test_standalone_vs_reference(gpu_lib, w, h, shift, params):
    cur, prev = _content(w, h)
    want, want_st = _reference(w, h, params)
    if ((w + 7) // 8) * ((h + 7) // 8) >= 2:  # the case is worth trusting: static and moving blocks in it
        mid, mid_st = _reference(w, h, (128, 64, 12, 24))
        assert all(0 < s[0] < s[1] for s in mid_st), mid_st
    got, got2, got_st = _denoise(cur, prev, w, h, params, shift, dst2='new')
    for f in range(N):
        assert np.array_equal(got[f], want[f]), f'frame {f}: {int((got[f] != want[f]).sum())} bytes differ'
        assert got_st[f] == want_st[f], f'frame {f}: statistics {got_st[f]} != {want_st[f]}'
    assert np.array_equal(got2, got), 'dst2 differs from dst'
    if params[0] == 0 and params[1] == 0 or params[2] == 1:
        assert np.array_equal(got, cur)


@pytest.mark.parametrize('w,h', [(36, 18), (130, 66)])
def test_without_statistics_and_repeatability(gpu_lib, w, h):
    cur, prev = _content(w, h)
    params = (128, 64, 12, 24)
    want, _ = _reference(w, h, params)
    a, _, st = _denoise(cur, prev, w, h, params, stats=False)
    b, _, _ = _denoise(cur, prev, w, h, params, stats=False)
    assert st is None and np.array_equal(a, want)
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize('dst,dst2', [('prev', None), ('cur', None), ('cur', 'prev'), ('prev', 'cur')], ids=['dst=prev', 'dst=cur', 'encoder-form', 'swapped'])
@pytest.mark.parametrize('w,h,shift', [(36, 18, 0), (130, 66, 0), (130, 66, 1), (264, 10, 0)], ids=['36x18', '130x66', '130x66-odd-address', '264x10'])
def test_aliased_destinations(gpu_lib, w, h, shift, dst, dst2):
    cur, prev = _content(w, h)
    for params in ((128, 64, 12, 24), (224, 224, 32, 1020)):
        want, want_st = _reference(w, h, params)
        got, got2, got_st = _denoise(cur, prev, w, h, params, shift, dst=dst, dst2=dst2)
        assert np.array_equal(got, want) and got_st == want_st
        assert got2 is None or np.array_equal(got2, want)


def test_recursion_on_the_device(gpu_lib):
    """five frames, each filtered against the previous output with dst == prev: denoise_sequence"""
    import torch
    import h264mi
    w, h, params = 130, 66, (128, 64, 12, 24)
    rng = np.random.default_rng(91)
    base = rng.integers(0, 256, ref.frame_bytes(w, h)).astype(np.int32)
    frames = [np.clip(base + rng.integers(-5, 6, base.size), 0, 255).astype(np.uint8) for _ in range(5)]
    want, _ = ref.denoise_sequence(frames, w, h, params)
    whole, state = _guarded(frames[0])
    for t in range(1, 5):
        cur = torch.from_numpy(frames[t]).cuda()
        h264mi.i420_denoise(state, cur, state, w, h, 1, params)
        assert np.array_equal(state.cpu().numpy(), want[t]), f'frame {t}'
    assert not np.array_equal(want[4], frames[4]) and _guards_intact(whole, frames[0].size)


def test_standalone_refusals_leave_the_destination_untouched(gpu_lib):
    import torch
    import h264mi
    fn = gpu_lib.h264mi_i420_denoise_dev
    w, h, n = 32, 16, 3
    nb = n * ref.frame_bytes(w, h)
    zeros = np.zeros(nb, np.uint8)
    wd, d = _guarded(np.full(nb, 0x5A, np.uint8))
    wd2, d2 = _guarded(np.full(nb, 0x5A, np.uint8))
    _, c = _guarded(zeros)
    _, p = _guarded(zeros)
    st = torch.zeros(4 * n + 4, dtype=torch.int32, device='cuda')
    good = ctypes.byref(h264mi.Denoise(128, 64, 12, 24))
    vp = ctypes.c_void_p
    D, D2, C, P, ST = d.data_ptr(), d2.data_ptr(), c.data_ptr(), p.data_ptr(), st.data_ptr()

    def call(dst=D, dst2=D2, cur=C, prev=P, stats=ST, ww=w, hh=h, nn=n, par=good):
        return fn(vp(dst) if dst else None, vp(dst2) if dst2 else None, vp(cur) if cur else None, vp(prev) if prev else None,
                  ww, hh, nn, par, vp(stats) if stats else None, None)

    assert call(dst=0) == -1 and call(cur=0) == -1 and call(prev=0) == -1 and call(par=None) == -1
    for ww, hh, nn in BAD_SHAPES:
        assert call(ww=ww, hh=hh, nn=nn) == -1, (ww, hh, nn)
    for bad in BAD_PARAMS:
        assert call(par=ctypes.byref(h264mi.Denoise(*bad))) == -1, bad
    assert call(stats=ST + 1) == -1 and call(stats=ST + 2) == -1
    assert call(dst2=D) == -1
    for off in (1, nb - 1, -1, -(nb - 1)):  # partial overlaps of every pair of frame buffers
        assert call(dst=C + off) == -1 and call(dst=P + off) == -1 and call(dst=D2 + off) == -1
        assert call(dst2=C + off) == -1 and call(dst2=P + off) == -1 and call(dst2=D + off) == -1
        assert call(cur=P + off) == -1 and call(prev=C + off) == -1
    for base in (D, D2, C, P):  # the statistics inside a frame buffer
        assert call(stats=base) == -1 and call(stats=base + nb - 4) == -1 and call(stats=base - 4) == -1
    torch.cuda.synchronize()
    for whole, view in ((wd, d), (wd2, d2)):
        assert _guards_intact(whole, nb) and (view.cpu().numpy() == 0x5A).all(), 'a refused call wrote'
    assert (st.cpu().numpy() == 0).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == 0).all() and (d2.cpu().numpy() == 0).all() and _guards_intact(wd, nb) and _guards_intact(wd2, nb)
    assert st.cpu().numpy()[:4 * n].reshape(n, 4).tolist() == [[0, 8, 0, 0]] * n


# ---------------------------------------------------------------- the encoder's pre-filter

DN = (128, 64, 12, 24)


@functools.lru_cache(maxsize=None)
def _scene(w, h, S, nf):
    """nf steps of S frames: a static smooth scene per stream plus seeded noise, a 16x16 square moving 8 samples a frame"""
    rng = np.random.default_rng(17 * w + h + S)
    steps = []
    yy, xx = np.mgrid[0:h, 0:w]
    for t in range(nf):
        fr = []
        for s in range(S):
            Y = (64 + (xx * 2 + yy * 3 + 40 * s) % 128).astype(np.int32)
            U = np.full((h // 2, w // 2), 110 + 10 * s, np.int32)
            V = np.full((h // 2, w // 2), 140 - 10 * s, np.int32)
            x0, y0 = 8 + 8 * t, 8 + 4 * s
            Y[y0:y0 + 16, x0:x0 + 16] = 230
            U[y0 // 2:y0 // 2 + 8, x0 // 2:x0 // 2 + 8] = 60
            f = np.concatenate([Y.ravel(), U.ravel(), V.ravel()])
            fr.append(np.clip(f + np.rint(rng.normal(0, 2, f.size)).astype(np.int32), 0, 255).astype(np.uint8))
        steps.append(np.stack(fr))
    return steps


def _filtered(steps, w, h, params=DN):
    """the steps as the pre-filter leaves them: each stream's recursion, started at the first step"""
    S = steps[0].shape[0]
    per = [ref.denoise_sequence([st[s] for st in steps], w, h, params)[0] for s in range(S)]
    return [np.stack([per[s][t] for s in range(S)]) for t in range(len(steps))]


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
    for t in range(len(want)):
        assert got[t]['nal'] == want[t]['nal'], f'{what} frame {t}: NAL bytes'
        assert got[t]['rc'] == want[t]['rc'], f'{what} frame {t}: rate-control state'


KEYS = ('sse', 'ssim_fix', 'windows', 'coded')
ENC_CASES = [(176, 144, 2), (72, 40, 1)]  # 72x40 is coded 80x48 and cropped
ENC_IDS = ['176x144-S2', '72x40-S1']


def _on(enc):
    enc.set_denoise(DN)
    d = enc.denoise()
    assert d is not None and (d.strength_y, d.strength_c, d.reach, d.motion) == DN


@pytest.mark.parametrize('w,h,S', ENC_CASES, ids=ENC_IDS)
def test_encoder_equals_encode_of_reference_frames(gpu_lib, w, h, S):
    raw = _scene(w, h, S, 4)
    clean = _filtered(raw, w, h)
    assert np.array_equal(clean[0], raw[0]) and not np.array_equal(clean[1], raw[1])
    for quality in (False, True):
        got = _run(w, h, S, raw, quality=quality, prepare=_on)
        want = _run(w, h, S, clean, quality=quality)
        _same(got, want)
        if quality:
            for t in range(4):
                for s in range(S):
                    q = {k: got[t]['q'][s][k] for k in KEYS}
                    assert q == qualityref.frame_quality(clean[t][s], got[t]['recon'][s], w, h), f'frame {t} stream {s}: records'
                    assert q == {k: want[t]['q'][s][k] for k in KEYS}
    plain = _run(w, h, S, raw)
    assert got[0]['nal'] == plain[0]['nal'], 'frame 0 is coded unfiltered'
    assert got[1]['nal'] != plain[1]['nal'], 'the filter changed nothing: the test shows nothing'


@pytest.mark.parametrize('w,h,S', ENC_CASES, ids=ENC_IDS)
def test_encoder_through_the_oriented_entry_point(gpu_lib, w, h, S):
    raw = _scene(w, h, S, 4)
    turned = [np.stack([orientref.orient_frame(f, w, h, orientref.ROT180) for f in st]) for st in raw]
    got = _run(w, h, S, turned, feed=lambda e, f: e.encode_oriented(f, orientref.ROT180), prepare=_on)
    _same(got, _run(w, h, S, _filtered(raw, w, h)))


def test_encoder_blends_the_overlays_after_the_filter(gpu_lib):
    """a 16x16 sprite on every stream: denoise, then overlay; the state never holds the sprite"""
    import torch
    import h264mi
    w, h, S = 176, 144, 2
    raw = _scene(w, h, S, 3)
    sprite = torch.from_numpy(np.random.default_rng(93).integers(0, 256, h264mi.i420a_bytes(16, 16), dtype=np.uint8)).cuda()
    ov = [h264mi.Overlay(0, s, 0, 0, 16, 16, 40, 64, 256, 0) for s in range(S)]

    def sprites(enc):
        enc.set_overlays(sprite, 16, 16, 1, ov)
        assert enc.overlays() == S

    def both(enc):
        sprites(enc)
        _on(enc)

    got = _run(w, h, S, raw, prepare=both)
    want = _run(w, h, S, _filtered(raw, w, h), prepare=sprites)
    _same(got, want)
    assert got[2]['nal'] != _run(w, h, S, _filtered(raw, w, h))[2]['nal'], 'the overlay changed nothing'


@pytest.mark.parametrize('w,h,S', ENC_CASES, ids=ENC_IDS)
def test_encoder_off_and_on_again(gpu_lib, w, h, S):
    """on for frames 0-1, off for 2, on again for 3-4: frame 2 raw, frame 3 unfiltered, frame 4 filtered against raw 3"""
    raw = _scene(w, h, S, 5)
    first = _filtered(raw[:2], w, h)
    again = _filtered(raw[3:], w, h)

    def before(enc, t):
        if t == 0 or t == 3:
            _on(enc)
        if t == 2:
            enc.set_denoise(None)
            assert enc.denoise() is None
            enc.force_idr()  # does not matter to the state; both sides get one

    def before_want(enc, t):
        if t == 2:
            enc.force_idr()

    want = _run(w, h, S, first + [raw[2]] + again, before=before_want)
    got = _run(w, h, S, raw, before=before)
    _same(got, want)
    assert not np.array_equal(again[1], raw[4])


def test_force_idr_keeps_the_state_and_zero_strengths_are_off(gpu_lib):
    w, h, S = 72, 40, 1
    raw = _scene(w, h, S, 4)

    def idr(enc, t):
        if t == 2:
            enc.force_idr()

    got = _run(w, h, S, raw, prepare=_on, before=idr)
    _same(got, _run(w, h, S, _filtered(raw, w, h), before=idr))

    def zero(enc):
        enc.set_denoise((0, 0, 12, 24))
        assert enc.denoise() is None

    _same(_run(w, h, S, raw, prepare=zero), _run(w, h, S, raw))


def test_set_denoise_refusals_leave_the_setting_in_force(gpu_lib):
    import h264mi
    w, h, S = 72, 40, 1
    raw = _scene(w, h, S, 3)

    def refuse(enc):
        for bad in BAD_PARAMS:
            with pytest.raises(ValueError):
                enc.set_denoise(bad)
            assert enc._L.h264mi_enc_set_denoise(enc._e, ctypes.byref(h264mi.Denoise(*bad))) == -1

    def before(enc, t):
        if t == 0:
            refuse(enc)
            assert enc.denoise() is None
            _on(enc)
        refuse(enc)
        d = enc.denoise()
        assert (d.strength_y, d.strength_c, d.reach, d.motion) == DN
        assert enc._L.h264mi_enc_denoise(enc._e, None) == 1

    _same(_run(w, h, S, raw, before=before), _run(w, h, S, _filtered(raw, w, h)))
