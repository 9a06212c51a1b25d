"""GPU: histograms, level tables and automatic levels -- the standalone calls h264mi_i420_hist_dev, h264mi_i420_lut_dev
and h264mi_i420_levels_dev and the encoder's stage h264mi_enc_set_levels -- against tests/levelsref.py. Exact integers,
so every comparison is equality of bytes or words; every destination sits between 64 guard bytes of 0xA5 that must stay
as they were.

The two streaming kernels know no rows: a plane of a tight frame is one run of bytes, laid on the grid of 16-byte units
of the address space. The tile is an item of 16384 bytes of that grid (256 threads x 4 units) and the load unit 16
bytes (csrc/levels.hip); a unit inside the plane moves as one 16-byte word at any address, the units a plane only
partly covers as bytes. The shapes (test_levels_host.SHAPES, N = 3 frames of different content each): 2x2 (chroma one
byte), 4x4, 16x16, 36x18 (chroma rows of 18 bytes: planes that start and end between units), 130x66 (no plane a multiple
of 16; the same at an odd address, where every plane starts between units), 8192x2 and 2x8192 (the limit), 8x2050 (luma
16400 bytes: one load unit past the tile -- these kernels have no second axis) and 16x4100 (chroma 16400 bytes)."""
import ctypes
import functools

import numpy as np
import pytest

import denoiseref
import levelsref as ref
import scaleref
import spatialref
from test_levels_host import BAD_PARAMS, BAD_SHAPES, INERT, N, NF, PARAMS, SHAPES, make_frames, make_sequence

pytestmark = pytest.mark.gpu

GUARD = 64
CASES = [(w, h, 0) for w, h in SHAPES] + [(130, 66, 1)]
CASE_IDS = [f'{w}x{h}' + ('-odd-address' if s else '') for w, h, s in CASES]
AUTO37 = (ref.AUTO, 655, 655, 0, 0, 16, 235, 256, 37, 80)
FIXED1 = (ref.FIXED, 0, 0, 30, 200, 16, 235, 64, 1, 96)


def _guarded(data, shift=0, dtype=np.uint8):
    """(whole, view): data's bytes on the device between 64 bytes of 0xA5 on each side, `shift` bytes into the allocation"""
    import torch
    raw = np.ascontiguousarray(np.asarray(data, dtype=dtype)).view(np.uint8).ravel()
    whole = torch.full((shift + raw.size + 2 * GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    view = whole[shift + GUARD:shift + GUARD + raw.size]
    view.copy_(torch.from_numpy(raw.copy()))
    return whole, view


def _guards_intact(whole, nbytes, shift=0):
    h = whole.cpu().numpy()
    return bool((h[:shift + GUARD] == 0xA5).all() and (h[shift + GUARD + nbytes:] == 0xA5).all())


def _words(view, dtype):
    return view.cpu().numpy().view(dtype)


@functools.lru_cache(maxsize=None)
def _hists(w, h):
    out = np.stack([ref.hist_frame(f, w, h) for f in make_frames(w, h)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _tables():
    """per-frame table sets: random, identity, reversed"""
    rng = np.random.default_rng(5)
    v = np.arange(256, dtype=np.uint8)
    t = np.stack([rng.integers(0, 256, 768, dtype=np.uint8), np.tile(v, 3), np.tile(v[::-1], 3)])
    t.setflags(write=False)
    return t


@pytest.mark.parametrize('w,h,shift', CASES, ids=CASE_IDS)
def test_hist_vs_reference(gpu_lib, w, h, shift):
    import torch
    import h264mi
    src = make_frames(w, h)
    ws, d_src = _guarded(src, shift)
    wh, d_hist = _guarded(np.full(N * 768, 0xFFFFFFFF, np.uint32), 0, np.uint32)  # the call zeroes it
    assert not shift or d_src.data_ptr() % 2 == 1
    h264mi.i420_hist(d_hist, d_src, w, h, N)
    torch.cuda.synchronize()
    got = _words(d_hist, np.uint32).reshape(N, 768)
    assert np.array_equal(got, _hists(w, h)), f'{int((got != _hists(w, h)).sum())} words differ'
    assert _guards_intact(wh, N * 3072) and _guards_intact(ws, src.size, shift)
    assert np.array_equal(d_src.cpu().numpy(), src.ravel()), 'the frames were written'


def test_hist_one_frame_and_repeatability(gpu_lib):
    import torch
    import h264mi
    w, h = 130, 66
    _, d_src = _guarded(make_frames(w, h))
    outs = []
    for _ in range(2):
        wh, d_hist = _guarded(np.full(N * 768, 0xFFFFFFFF, np.uint32), 0, np.uint32)
        h264mi.i420_hist(d_hist, d_src, w, h, 1)
        torch.cuda.synchronize()
        outs.append(_words(d_hist, np.uint32))
        assert _guards_intact(wh, N * 3072)
    assert np.array_equal(outs[0][:768], _hists(w, h)[0]) and (outs[0][768:] == 0xFFFFFFFF).all(), 'n = 1 writes one frame\'s words'
    assert outs[0].tobytes() == outs[1].tobytes()


def test_flat_frames(gpu_lib):
    """1024x256 flat, each frame another value, and one frame of two alternating values: 262144 samples in one bin"""
    import torch
    import h264mi
    w, h = 1024, 256
    fb = ref.frame_bytes(w, h)
    values = (0, 77, 255, 128)
    src = np.empty((len(values) + 1, fb), np.uint8)
    for k, v in enumerate(values):
        src[k] = v
    src[-1] = np.where(np.arange(fb) & 1, 200, 13)
    n = src.shape[0]
    _, d_src = _guarded(src)
    wh, d_hist = _guarded(np.full(n * 768, 0xFFFFFFFF, np.uint32), 0, np.uint32)
    h264mi.i420_hist(d_hist, d_src, w, h, n)
    torch.cuda.synchronize()
    got = _words(d_hist, np.uint32).reshape(n, 768)
    for k, v in enumerate(values):
        want = np.zeros(768, np.uint32)
        want[v], want[256 + v], want[512 + v] = w * h, w * h // 4, w * h // 4
        assert np.array_equal(got[k], want), f'flat {v}'
    assert got[0][0] == 262144
    assert np.array_equal(got[-1], ref.hist_frame(src[-1], w, h)) and np.count_nonzero(got[-1]) == 6
    assert _guards_intact(wh, n * 3072)
    # the same frames through per-frame tables and through AUTO levels, in place
    luts = np.random.default_rng(9).integers(0, 256, (n, 768), dtype=np.uint8)
    _, d_luts = _guarded(luts)
    wd, d = _guarded(src)
    h264mi.i420_lut(d, d, w, h, n, d_luts, per_frame=True)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().reshape(n, fb), np.stack([ref.lut_frame(src[k], w, h, luts[k]) for k in range(n)])) and _guards_intact(wd, src.size)
    work = torch.zeros(h264mi.levels_work_bytes(n), dtype=torch.uint8, device='cuda')
    wr, d_rec = _guarded(np.zeros(8 * n, np.int32), 0, np.int32)
    wd, d = _guarded(src)
    h264mi.i420_levels(d, d, w, h, n, PARAMS[2], work, record=d_rec)
    torch.cuda.synchronize()
    want = [ref.levels_frame(src[k], w, h, PARAMS[2]) for k in range(n)]
    assert np.array_equal(d.cpu().numpy().reshape(n, fb), np.stack([x[0] for x in want])) and _guards_intact(wd, src.size)
    assert _words(d_rec, np.int32).reshape(n, 8).tolist() == [x[2] for x in want] and _guards_intact(wr, 32 * n)


@pytest.mark.parametrize('w,h,shift', CASES + [(130, 66, 3)], ids=CASE_IDS + ['130x66-source-off-the-grid'])
def test_lut_vs_reference(gpu_lib, w, h, shift):
    """out of place and in place, one shared table set (each of random, identity, reversed) and per-frame sets. shift 3:
    the source 3 bytes into its allocation, the destination 0: the two sit differently on the unit grid"""
    import torch
    import h264mi
    src = make_frames(w, h)
    nb = src.size
    tabs = _tables()
    ws, d_src = _guarded(src, shift)
    dshift = 0 if shift == 3 else shift
    wd, d_dst = _guarded(np.full(nb, 0x5A, np.uint8), dshift)
    wt, d_tabs = _guarded(tabs, shift)
    cases = [(tabs[k], d_tabs[768 * k:768 * k + 768], False) for k in range(3)] + [(None, d_tabs, True)]
    for tab, d_tab, per_frame in cases:
        want = np.stack([ref.lut_frame(src[f], w, h, tabs[f] if per_frame else tab) for f in range(N)])
        d_dst.fill_(0x5A)
        h264mi.i420_lut(d_dst, d_src, w, h, N, d_tab, per_frame=per_frame)
        torch.cuda.synchronize()
        got = d_dst.cpu().numpy().reshape(N, -1)
        assert np.array_equal(got, want), f'out of place, per_frame={per_frame}: {int((got != want).sum())} bytes differ'
        assert _guards_intact(wd, nb, dshift) and _guards_intact(ws, nb, shift) and _guards_intact(wt, tabs.size, shift)
        assert np.array_equal(d_src.cpu().numpy(), src.ravel()), 'the source frames were written'
        wi, d_in = _guarded(src, shift)
        h264mi.i420_lut(d_in, d_in, w, h, N, d_tab, per_frame=per_frame)
        torch.cuda.synchronize()
        assert np.array_equal(d_in.cpu().numpy().reshape(N, -1), want), f'in place, per_frame={per_frame}'
        assert _guards_intact(wi, nb, shift)
    assert np.array_equal(d_tabs.cpu().numpy(), tabs.ravel())


@functools.lru_cache(maxsize=None)
def _levels_reference(w, h, params, with_state):
    """N frames as N streams: (frames, states, records); with_state: stream 0 has == 0, the others a given state"""
    fr, st, rec = [], [], []
    for k, f in enumerate(make_frames(w, h)):
        s_in = _state_in(k) if with_state else None
        o, s, r = ref.levels_frame(f, w, h, params, s_in)
        fr.append(o)
        st.append(s if (params[0] == ref.AUTO or s_in is None) else s_in)
        rec.append(r)
    return np.stack(fr), st, rec


def _state_in(k):
    return [[0, 123, 456, 789], [1, 20 << 8, 200 << 8, 0], [7, 9000, 9100, 5]][k]


@pytest.mark.parametrize('w,h,shift', CASES, ids=CASE_IDS)
def test_levels_vs_reference(gpu_lib, w, h, shift):
    """AUTO and FIXED, every shared parameter set: without state and record out of place, with both in place"""
    import torch
    import h264mi
    src = make_frames(w, h)
    nb = src.size
    ws, d_src = _guarded(src, shift)
    wd, d_dst = _guarded(np.full(nb, 0x5A, np.uint8), shift)
    ww, d_work = _guarded(np.full(h264mi.levels_work_bytes(N), 0xEE, np.uint8))
    for params in PARAMS:
        want, _, _ = _levels_reference(w, h, params, False)
        d_dst.fill_(0x5A)
        h264mi.i420_levels(d_dst, d_src, w, h, N, params, d_work)
        torch.cuda.synchronize()
        got = d_dst.cpu().numpy().reshape(N, -1)
        assert np.array_equal(got, want), f'{params}: {int((got != want).sum())} bytes differ'
        assert _guards_intact(wd, nb, shift) and _guards_intact(ws, nb, shift) and _guards_intact(ww, d_work.numel())
        want, st, rec = _levels_reference(w, h, params, True)
        wi, d_in = _guarded(src, shift)
        wst, d_state = _guarded(np.array([_state_in(k) for k in range(N)], np.int32), 0, np.int32)
        wr, d_rec = _guarded(np.full(8 * N, -7, np.int32), 0, np.int32)
        h264mi.i420_levels(d_in, d_in, w, h, N, params, d_work, state=d_state, record=d_rec)
        torch.cuda.synchronize()
        assert np.array_equal(d_in.cpu().numpy().reshape(N, -1), want), f'{params}: in place with a state'
        assert _words(d_state, np.int32).reshape(N, 4).tolist() == st, f'{params}: state words'
        assert _words(d_rec, np.int32).reshape(N, 8).tolist() == rec, f'{params}: record words'
        assert _guards_intact(wi, nb, shift) and _guards_intact(wst, 16 * N) and _guards_intact(wr, 32 * N) and _guards_intact(ww, d_work.numel())
    assert np.array_equal(d_src.cpu().numpy(), src.ravel()), 'the source frames were written'
    # the work area holds the last call's histograms (AUTO) and tables
    h264mi.i420_levels(d_dst, d_src, w, h, N, AUTO37, d_work)
    torch.cuda.synchronize()
    wk = d_work.cpu().numpy()
    assert np.array_equal(wk[:N * 3072].view(np.uint32).reshape(N, 768), np.stack([ref.hist_frame(f, w, h) for f in src]))
    assert np.array_equal(wk[N * 3072:].reshape(N, 768), np.stack([ref.levels_lut(ref.hist_frame(f, w, h)[:256], w, h, AUTO37)[0] for f in src]))


def test_levels_sequence_one_call_at_a_time(gpu_lib):
    """two streams, six frames whose brightness steps up and down, speed 37 and the stalling speed 255: frames, state
    words and records after every call"""
    import torch
    import h264mi
    w, h, S = 64, 48, 2
    for params in (AUTO37, PARAMS[5]):
        seqs = [make_sequence(w, h, s) for s in range(S)]
        per = [ref.levels_frames(seqs[s], w, h, params) for s in range(S)]
        wst, d_state = _guarded(np.zeros(4 * S, np.int32), 0, np.int32)
        wr, d_rec = _guarded(np.zeros(8 * S, np.int32), 0, np.int32)
        work = torch.zeros(h264mi.levels_work_bytes(S), dtype=torch.uint8, device='cuda')
        for t in range(NF):
            wd, d = _guarded(np.stack([seqs[s][t] for s in range(S)]))
            h264mi.i420_levels(d, d, w, h, S, params, work, state=d_state, record=d_rec)
            torch.cuda.synchronize()
            assert np.array_equal(d.cpu().numpy().reshape(S, -1), np.stack([per[s][0][t] for s in range(S)])), f'frame {t}'
            assert _words(d_state, np.int32).reshape(S, 4).tolist() == [per[s][3][t] for s in range(S)], f'frame {t}: state'
            assert _words(d_rec, np.int32).reshape(S, 8).tolist() == [per[s][2][t] for s in range(S)], f'frame {t}: record'
            assert _guards_intact(wd, d.numel()) and _guards_intact(wst, 16 * S) and _guards_intact(wr, 32 * S)
        assert per[0][2][1][2:4] != [per[0][2][1][0] << 8, per[0][2][1][1] << 8], 'the smoothed ends lag the measured ones'


def test_refusals_write_nothing(gpu_lib):
    import torch
    import h264mi
    w, h, n = 32, 16, 3
    nb = n * ref.frame_bytes(w, h)
    vp = ctypes.c_void_p
    bufs = {'dst': (nb, 0x5A), 'src': (nb, 0x33), 'hist': (n * 3072, 0x11), 'luts': (n * 768, 0x22), 'work': (n * 3840, 0x44),
            'state': (n * 16, 0x00), 'record': (n * 32, 0x66)}
    dev = {k: _guarded(np.full(sz, fill, np.uint8)) for k, (sz, fill) in bufs.items()}
    ptr = {k: v[1].data_ptr() for k, v in dev.items()}
    good = ctypes.byref(h264mi.Levels(*AUTO37))

    def arg(p):
        return vp(p) if p else None

    def hist(hist=ptr['hist'], frames=ptr['src'], ww=w, hh=h, nn=n):
        return gpu_lib.h264mi_i420_hist_dev(arg(hist), arg(frames), ww, hh, nn, None)

    def lut(dst=ptr['dst'], src=ptr['src'], ww=w, hh=h, nn=n, luts=ptr['luts'], per_frame=1):
        return gpu_lib.h264mi_i420_lut_dev(arg(dst), arg(src), ww, hh, nn, arg(luts), per_frame, None)

    def levels(dst=ptr['dst'], src=ptr['src'], ww=w, hh=h, nn=n, par=good, state=ptr['state'], record=ptr['record'], work=ptr['work']):
        return gpu_lib.h264mi_i420_levels_dev(arg(dst), arg(src), ww, hh, nn, par, arg(state), arg(record), arg(work), None)

    assert hist(hist=0) == -1 and hist(frames=0) == -1
    assert lut(dst=0) == -1 and lut(src=0) == -1 and lut(luts=0) == -1 and lut(per_frame=2) == -1 and lut(per_frame=-1) == -1
    assert levels(dst=0) == -1 and levels(src=0) == -1 and levels(par=None) == -1 and levels(work=0) == -1
    for ww, hh, nn in BAD_SHAPES:
        assert hist(ww=ww, hh=hh, nn=nn) == -1 and lut(ww=ww, hh=hh, nn=nn) == -1 and levels(ww=ww, hh=hh, nn=nn) == -1, (ww, hh, nn)
    for bad in BAD_PARAMS:
        assert levels(par=ctypes.byref(h264mi.Levels(*bad))) == -1, bad
    with pytest.raises(ValueError):
        h264mi.i420_levels(dev['dst'][1], dev['src'][1], w, h, n, BAD_PARAMS[3], dev['work'][1])
    # word buffers off a multiple of 4
    for off in (1, 2, 3):
        assert hist(hist=ptr['hist'] + off, nn=n - 1) == -1
        assert levels(state=ptr['state'] + off, nn=n - 1) == -1 and levels(record=ptr['record'] + off, nn=n - 1) == -1 and levels(work=ptr['work'] + off, nn=n - 1) == -1
    # overlaps: the histogram with the frames; dst and src in part; the tables with the destination; the levels' buffers
    for off in (0, 4, nb - 4, -(n * 3072 - 4)):
        assert hist(hist=ptr['src'] + off) == -1, off
    for off in (1, nb - 1, -1, -(nb - 1)):
        assert lut(dst=ptr['src'] + off) == -1 and lut(src=ptr['dst'] + off) == -1 and levels(dst=ptr['src'] + off) == -1, off
    for off in (0, nb - 1, -(n * 768 - 1)):
        assert lut(luts=ptr['dst'] + off) == -1, off
    for off in (0, nb - 1, -767):
        assert lut(luts=ptr['dst'] + off, per_frame=0) == -1, off
    for other in ('dst', 'src', 'state', 'record'):
        assert levels(work=ptr[other]) == -1, other
    assert levels(state=ptr['dst']) == -1 and levels(record=ptr['src'] + 4) == -1 and levels(state=ptr['record']) == -1
    assert levels(state=ptr['work'] + 3840 * n - 4) == -1 and levels(record=ptr['state'] + 12) == -1
    assert hist(ww=w, nn=0) == -1 and gpu_lib.h264mi_levels_work_bytes(0) == 0
    torch.cuda.synchronize()
    for k, (whole, view) in dev.items():
        assert _guards_intact(whole, bufs[k][0]) and (view.cpu().numpy() == bufs[k][1]).all(), f'a refused call wrote {k}'
    assert hist() == 0 and lut(dst=ptr['src']) == 0 and levels(dst=ptr['src'], state=0, record=0) == 0 and levels() == 0
    torch.cuda.synchronize()
    assert all(_guards_intact(whole, bufs[k][0]) for k, (whole, _) in dev.items())


# ---- the encoder's stage
ENC_CASES = [(64, 48, 2), (130, 66, 2)]  # 130x66 is coded 144x80 and cropped
ENC_IDS = ['64x48-S2', '130x66-S2']


def _scene(w, h, S):
    return [np.stack([make_sequence(w, h, s)[t] for s in range(S)]) for t in range(NF)]


def _levelled(steps, w, h, params, states=None):
    """the steps as the stage leaves them, the records of every step, and the states after the last"""
    S = steps[0].shape[0]
    states = list(states) if states is not None else [None] * S
    out, recs = [], []
    for st in steps:
        fr, rc = [], []
        for s in range(S):
            o, states[s], r = ref.levels_frame(st[s], w, h, params, states[s])
            fr.append(o)
            rc.append(r)
        out.append(np.stack(fr))
        recs.append(rc)
    return out, recs, states


def _run(w, h, S, steps, feed=None, prepare=None, before=None, after=None):
    """one encoder over `steps`, fed by feed(enc, device frames) (default: encode), before(enc, t) in front of step t,
    after(enc, t) behind it: per step the NAL bytes and rc_state"""
    import torch
    import h264mi
    enc = h264mi.BatchEncoder(w, h, 300000, S)
    enc.set_frame_skip(False)
    if prepare:
        prepare(enc)
    out = []
    for t, fr in enumerate(steps):
        if before:
            before(enc, t)
        frames = torch.from_numpy(np.ascontiguousarray(fr).ravel()).cuda()  # held until nal_sizes() has synchronised
        (feed or (lambda e, f: e.encode(f)))(enc, frames)
        sizes = enc.nal_sizes()
        out.append({'nal': [enc.nal_bytes(s, sizes[s]) for s in range(S)], 'rc': [enc.rc_state(s) for s in range(S)]})
        assert all(len(b) > 0 for b in out[-1]['nal'])
        assert np.array_equal(frames.cpu().numpy(), np.ascontiguousarray(fr).ravel()), "the caller's frames were written"
        if after:
            after(enc, t)
    enc.close()
    return out


def _same(got, want, what=''):
    assert len(got) == len(want)
    for t in range(len(want)):
        assert got[t]['nal'] == want[t]['nal'], f'{what} frame {t}: NAL bytes'
        assert got[t]['rc'] == want[t]['rc'], f'{what} frame {t}: rate-control state'


@pytest.mark.parametrize('w,h,S', ENC_CASES, ids=ENC_IDS)
def test_encoder_equals_encode_of_reference_frames(gpu_lib, w, h, S):
    import h264mi
    raw = _scene(w, h, S)
    plain = _run(w, h, S, raw)
    for params in (AUTO37, FIXED1):
        staged, recs, _ = _levelled(raw, w, h, params)
        assert not np.array_equal(staged[0], raw[0])

        def on(enc):
            assert enc.levels() is None
            enc.set_levels(params)
            p = enc.levels()
            assert p is not None and tuple(getattr(p, k) for k in ref.FIELDS) == params
            if params[0] == ref.FIXED:
                assert enc.levels_record() == [[0, 0, 0, 0, 30 << 8, 200 << 8, 0, 0]] * S, 'the setter wrote the record'
            else:
                assert enc.levels_record() == [[0] * 8] * S

        def after(enc, t):
            assert enc.levels_record() == recs[t], f'frame {t}: records'

        got = _run(w, h, S, raw, prepare=on, after=after)
        _same(got, _run(w, h, S, staged), str(params))
        assert got[0]['nal'] != plain[0]['nal'], 'the stage changed nothing: the test shows nothing'
    # an inert setting and NULL: the bytes of an encoder never touched

    def off(enc):
        enc.set_levels(INERT)
        assert enc.levels() is None
        enc.set_levels(None)
        assert enc.levels() is None and enc._L.h264mi_enc_levels(enc._e, None) == 0
        with pytest.raises(RuntimeError):
            enc.levels_record()

    _same(_run(w, h, S, raw, prepare=off), plain, 'off')


def test_encoder_order_with_the_denoiser_and_the_spatial_filter(gpu_lib):
    """denoise, levels, sharpen: the denoiser's state never holds a levelled frame, the sharpening works on the stretched picture"""
    w, h, S = 64, 48, 2
    DN, SP = (128, 64, 12, 24), (1, 2, 40, -17, 2)
    raw = _scene(w, h, S)
    rng = np.random.default_rng(77)
    raw = [np.clip(st.astype(np.int32) + rng.integers(-3, 4, st.shape), 0, 255).astype(np.uint8) for st in raw]  # something to denoise
    per = [denoiseref.denoise_sequence([st[s] for st in raw], w, h, DN)[0] for s in range(S)]
    clean = [np.stack([per[s][t] for s in range(S)]) for t in range(NF)]
    assert not np.array_equal(clean[2], raw[2])
    lev, recs, _ = _levelled(clean, w, h, AUTO37)
    want = [np.stack([spatialref.spatial_frame(f, w, h, SP) for f in st]) for st in lev]

    def everything(enc):
        enc.set_spatial(SP)
        enc.set_levels(AUTO37)
        enc.set_denoise(DN)

    got = _run(w, h, S, raw, prepare=everything, after=lambda enc, t: recs[t] == enc.levels_record() or pytest.fail(f'frame {t}: records'))
    _same(got, _run(w, h, S, want))
    # the other orders give other bytes
    wrong = [np.stack([spatialref.spatial_frame(f, w, h, SP) for f in st]) for st in clean]
    wrong, _, _ = _levelled(wrong, w, h, AUTO37)
    assert _run(w, h, S, wrong)[1]['nal'] != got[1]['nal']


@pytest.mark.parametrize('w,h,S', ENC_CASES[:1], ids=ENC_IDS[:1])
def test_encoder_off_on_and_changed_settings(gpu_lib, w, h, S):
    """AUTO37 for frames 0-1, other parameters for 2-3 (the state is kept), off for 4, on again for 5 (a first frame);
    refused settings in between leave the one in force; force_idr does not reset the state"""
    import h264mi
    raw = _scene(w, h, S)
    P2 = PARAMS[2]  # speed 37 again: the ends it starts from matter

    def refuse(enc):
        for bad in BAD_PARAMS:
            with pytest.raises(ValueError):
                enc.set_levels(bad)
            assert enc._L.h264mi_enc_set_levels(enc._e, ctypes.byref(h264mi.Levels(*bad))) == -1

    def before(enc, t):
        if t == 0:
            refuse(enc)
            assert enc.levels() is None
            enc.set_levels(AUTO37)
        if t == 1:
            for s in range(S):
                enc.force_idr(s)
        if t == 2:
            enc.set_levels(P2)
        if t == 4:
            enc.set_levels(INERT)
        if t == 5:
            enc.set_levels(AUTO37)
        was = repr(enc.levels())
        refuse(enc)
        assert repr(enc.levels()) == was

    a, _, st = _levelled(raw[:2], w, h, AUTO37)
    b, _, _ = _levelled(raw[2:4], w, h, P2, st)
    assert not np.array_equal(b[0], _levelled(raw[2:3], w, h, P2)[0][0]), 'the kept state shows'
    c, _, _ = _levelled(raw[5:], w, h, AUTO37)

    def idr(enc, t):
        if t == 1:
            for s in range(S):
                enc.force_idr(s)

    _same(_run(w, h, S, raw, before=before), _run(w, h, S, a + b + raw[4:5] + c, before=idr))


def test_encoder_through_the_scaled_entry_point(gpu_lib):
    w, h, S = 64, 48, 2
    big = _scene(2 * w, 2 * h, S)
    small = [np.stack([scaleref.scale_frame(f, 2 * w, 2 * h, w, h) for f in st]) for st in big]
    staged, recs, _ = _levelled(small, w, h, AUTO37)
    got = _run(w, h, S, big, feed=lambda e, f: e.encode_scaled(f, 2 * w, 2 * h), prepare=lambda enc: enc.set_levels(AUTO37),
               after=lambda enc, t: recs[t] == enc.levels_record() or pytest.fail(f'frame {t}: records'))
    _same(got, _run(w, h, S, staged))


def test_encoder_getters_and_null_handling(gpu_lib):
    import h264mi
    L = gpu_lib
    p = h264mi.Levels(*AUTO37)
    out = h264mi.Levels()
    rec = (ctypes.c_int32 * 16)()
    assert L.h264mi_enc_set_levels(None, ctypes.byref(p)) == -1 and L.h264mi_enc_levels(None, ctypes.byref(out)) == -1
    assert L.h264mi_enc_levels_record(None, rec, 2) == -1
    enc = h264mi.BatchEncoder(64, 48, 300000, 2)
    try:
        assert L.h264mi_enc_levels(enc._e, ctypes.byref(out)) == 0 and out.max_gain == 0, 'off: *out untouched'
        assert L.h264mi_enc_levels_record(enc._e, rec, 2) == -1, 'off'
        assert L.h264mi_enc_set_levels(enc._e, ctypes.byref(p)) == 0
        assert L.h264mi_enc_levels(enc._e, None) == 1 and L.h264mi_enc_levels(enc._e, ctypes.byref(out)) == 1
        assert tuple(getattr(out, k) for k in ref.FIELDS) == AUTO37
        assert L.h264mi_enc_levels_record(enc._e, None, 2) == -1 and L.h264mi_enc_levels_record(enc._e, rec, 1) == -1
        assert L.h264mi_enc_levels_record(enc._e, rec, 3) == -1 and L.h264mi_enc_levels_record(enc._e, rec, 2) == 0
        assert L.h264mi_enc_set_levels(enc._e, None) == 0 and L.h264mi_enc_levels(enc._e, None) == 0
    finally:
        enc.close()
