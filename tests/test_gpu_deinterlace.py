"""GPU: the deinterlacer -- the standalone call h264mi_i420_deinterlace_dev and the encoder's first pre-filter
h264mi_enc_set_deinterlace -- against tests/deintref.py. Exact integers, so every comparison is equality of bytes; every
buffer sits between 64 guard bytes of 0xA5 that must stay as they were. The kernel's item is a row group of 16 rows by
a strip of 256 samples of one plane (csrc/deinterlace.hip), which the shapes of test_deinterlace_host.SIZES are chosen
around; every buffer is also placed at an odd address, so that the byte path runs beside the word path on one content."""
import ctypes
import functools

import numpy as np
import pytest

import deintref as ref
import denoiseref
from test_deinterlace_host import BAD_PARAMS, BAD_SHAPES, CONTENTS, PARAMS, SIZES, _clip, make_pair

pytestmark = pytest.mark.gpu

GUARD = 64
N = 3


@functools.lru_cache(maxsize=None)
def _content(w, h, content):
    """(cur, prev): N frame pairs of different content, as (N, frame bytes) arrays; shared, never written"""
    pairs = [make_pair(w, h, content, f) for f in range(N)]
    cur, prev = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    cur.setflags(write=False)
    prev.setflags(write=False)
    return cur, prev


@functools.lru_cache(maxsize=None)
def _reference(w, h, content, params, with_prev):
    cur, prev = _content(w, h, content)
    res = [ref.deint_frame(cur[f], prev[f] if with_prev else None, w, h, params) for f in range(N)]
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


def _deint(cur, prev, w, h, params, n=N, shift=0, dst='new', prev_out=None, stats=True):
    """the standalone call on n frames. prev: an array or None; dst: 'new' (a fresh guarded buffer of 0x5A) or 'cur';
    prev_out: None, 'new' or 'prev'. Returns (dst bytes, prev_out bytes or None, stats rows or None); every buffer's
    guards are checked, and every buffer that is not a destination must hold what it held"""
    import torch
    import h264mi
    cur = np.ascontiguousarray(cur[:n])
    nb = cur.size
    wc, d_cur = _guarded(cur, shift)
    wp, d_prev = (None, None) if prev is None else _guarded(np.ascontiguousarray(prev[:n]), shift)
    fresh = np.full(nb, 0x5A, np.uint8)
    wd, d_dst = (wc, d_cur) if dst == 'cur' else _guarded(fresh, shift)
    wq, d_q = (None, None) if prev_out is None else (wp, d_prev) if prev_out == 'prev' else _guarded(fresh, shift)
    if shift:
        assert all(t.data_ptr() % 2 == 1 for t in (d_cur, d_dst))
    d_stats = torch.full((4 * n,), 0x7FFFFFFF, dtype=torch.int32, device='cuda') if stats else None
    h264mi.i420_deinterlace(d_dst, d_cur, w, h, n, params, prev=d_prev, prev_out=d_q, stats=d_stats)
    torch.cuda.synchronize()
    out = d_dst.cpu().numpy().reshape(n, -1)
    out2 = d_q.cpu().numpy().reshape(n, -1) if d_q is not None else None
    for whole in (wc, wp, wd, wq):
        assert whole is None or _guards_intact(whole, nb, shift), 'bytes outside the frames were written'
    if dst != 'cur':
        assert np.array_equal(d_cur.cpu().numpy(), cur.ravel()), 'the current frames were written'
    if prev is not None and prev_out != 'prev':
        assert np.array_equal(d_prev.cpu().numpy(), prev[:n].ravel()), 'the previous frames were written'
    st = (d_stats.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).reshape(n, 4).tolist() if stats else None
    return out, out2, st


def _check(got, got_st, want, want_st, n, what):
    for f in range(n):
        assert np.array_equal(got[f], want[f]), f'{what} frame {f}: {int((got[f] != want[f]).sum())} bytes differ, first at {int(np.argmax(got[f] != want[f]))}'
        assert got_st is None or got_st[f] == want_st[f], f'{what} frame {f}: statistics {got_st[f]} != {want_st[f]}'


@pytest.mark.parametrize('params', PARAMS, ids=[str(p) for p in PARAMS])
@pytest.mark.parametrize('w,h', SIZES, ids=[f'{w}x{h}' for w, h in SIZES])
def test_standalone_vs_reference(gpu_lib, w, h, params):
    """all eight parameter combinations, with and without P, four contents, at an even and an odd address, n = 3; and
    n = 1 on the random content"""
    for content in CONTENTS:
        cur, prev = _content(w, h, content)
        for with_prev in (True, False):
            want, want_st = _reference(w, h, content, params, with_prev)
            for shift in (0, 1):
                got, got2, got_st = _deint(cur, prev if with_prev else None, w, h, params, shift=shift, prev_out='new')
                _check(got, got_st, want, want_st, N, (content, with_prev, shift))
                assert np.array_equal(got2, cur), 'prev_out is not the unfiltered input'
    cur, prev = _content(w, h, 'random')
    want, want_st = _reference(w, h, 'random', params, True)
    got, _, got_st = _deint(cur, prev, w, h, params, n=1)
    _check(got, got_st, want, want_st, 1, 'n = 1')
    if params[2] == 1 and h > 2:
        assert not np.array_equal(want, _reference(w, h, 'random', params, False)[0]), 'P changes nothing: the case shows nothing'


ALIAS_SIZES = [(18, 10), (34, 6), (SIZES[5][0], 18), (SIZES[6][0], 34), (2, SIZES[7][1])]


@pytest.mark.parametrize('dst,prev_out', [('cur', None), ('new', 'prev'), ('cur', 'prev')], ids=['dst=cur', 'prev_out=prev', 'encoder-form'])
@pytest.mark.parametrize('w,h', ALIAS_SIZES, ids=[f'{w}x{h}' for w, h in ALIAS_SIZES])
def test_aliased_buffers(gpu_lib, w, h, dst, prev_out):
    for content in ('random', 'ramp'):
        cur, prev = _content(w, h, content)
        for params in ((0, 1, 1, 8), (1, 1, 1, 8), (1, 0, 1, 8), (0, 1, 0, 8)):
            want, want_st = _reference(w, h, content, params, True)
            for shift in (0, 1):
                got, got2, got_st = _deint(cur, prev, w, h, params, shift=shift, dst=dst, prev_out=prev_out)
                _check(got, got_st, want, want_st, N, (content, params, shift))
                assert got2 is None or np.array_equal(got2, cur)


@pytest.mark.parametrize('w,h', [(34, 6), (SIZES[5][0], 18)])
def test_a_clip_in_one_buffer_and_no_statistics(gpu_lib, w, h):
    """d_prev = d_cur - one frame: the read ranges overlap, neither is written; twice, for the same bytes"""
    import h264mi
    import torch
    frames = np.stack([make_pair(w, h, 'random', f)[0] for f in range(N + 1)])
    fb = ref.frame_bytes(w, h)
    whole, clip = _guarded(frames)
    params = (0, 1, 1, 8)
    want = np.stack([ref.deint_frame(frames[t], frames[t - 1], w, h, params)[0] for t in range(1, N + 1)])
    outs = []
    for _ in range(2):
        wd, dst = _guarded(np.full(N * fb, 0x5A, np.uint8))
        h264mi.i420_deinterlace(dst, clip[fb:], w, h, N, params, prev=clip[:N * fb])
        torch.cuda.synchronize()
        outs.append(dst.cpu().numpy())
        assert _guards_intact(wd, N * fb)
    assert np.array_equal(outs[0].reshape(N, -1), want) and outs[0].tobytes() == outs[1].tobytes()
    assert np.array_equal(clip.cpu().numpy(), frames.ravel()) and _guards_intact(whole, frames.size)


def test_standalone_refusals_leave_the_destinations_untouched(gpu_lib):
    import torch
    import h264mi
    fn = gpu_lib.h264mi_i420_deinterlace_dev
    w, h, n = 32, 16, 3
    nb = n * ref.frame_bytes(w, h)
    zeros = np.zeros(nb, np.uint8)
    wd, d = _guarded(np.full(nb, 0x5A, np.uint8))
    wq, q = _guarded(np.full(nb, 0x5A, np.uint8))
    _, c = _guarded(zeros)
    _, p = _guarded(zeros)
    st = torch.zeros(4 * n + 4, dtype=torch.int32, device='cuda')
    good = ctypes.byref(h264mi.Deinterlace(0, 1, 1, 8))
    vp = ctypes.c_void_p
    D, Q, C, P, ST = d.data_ptr(), q.data_ptr(), c.data_ptr(), p.data_ptr(), st.data_ptr()

    def call(dst=D, prev_out=Q, cur=C, prev=P, stats=ST, ww=w, hh=h, nn=n, par=good):
        return fn(vp(dst) if dst else None, vp(prev_out) if prev_out else None, vp(cur) if cur else None, vp(prev) if prev else None,
                  ww, hh, nn, par, vp(stats) if stats else None, None)

    assert call(dst=0) == -1 and call(cur=0) == -1 and call(par=None) == -1
    for ww, hh, nn in BAD_SHAPES:
        assert call(ww=ww, hh=hh, nn=nn) == -1, (ww, hh, nn)
    for bad in BAD_PARAMS:
        assert call(par=ctypes.byref(h264mi.Deinterlace(*bad))) == -1, bad
    assert call(stats=ST + 1) == -1 and call(stats=ST + 2) == -1
    assert call(prev_out=D) == -1 and call(dst=P) == -1 and call(prev_out=C) == -1
    for off in (1, nb - 1, -1, -(nb - 1)):  # partial overlaps of a written range with every other
        assert call(dst=C + off) == -1 and call(dst=P + off) == -1 and call(dst=Q + off) == -1
        assert call(prev_out=C + off) == -1 and call(prev_out=P + off) == -1 and call(prev_out=D + off) == -1
        assert call(dst=C, prev=C + off) == -1 and call(prev_out=P, cur=P + off) == -1
    for base in (D, Q, C, P):  # the statistics inside a frame buffer
        assert call(stats=base) == -1 and call(stats=base + nb - 4) == -1 and call(stats=base - 4) == -1
    torch.cuda.synchronize()
    for whole, view in ((wd, d), (wq, q)):
        assert _guards_intact(whole, nb) and (view.cpu().numpy() == 0x5A).all(), 'a refused call wrote'
    assert (st.cpu().numpy() == 0).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == 0).all() and (q.cpu().numpy() == 0).all() and _guards_intact(wd, nb) and _guards_intact(wq, nb)
    assert st.cpu().numpy()[:4 * n].reshape(n, 4).tolist() == [[w * h // 2, 0, 0, 0]] * n


# ---------------------------------------------------------------- the encoder's first pre-filter

W, H, S, NF = 48, 32, 3, 6
DI = (0, 1, 1, 8)


@functools.lru_cache(maxsize=None)
def _interlaced(parity=0):
    """NF steps of S interlaced frames: stream s a pan of s samples a field (test_deinterlace_host._clip; stream 0 is a
    still) under seeded noise of +-3, woven"""
    rng = np.random.default_rng(41)
    noisy = lambda f: np.clip(f.astype(np.int32) + rng.integers(-3, 4, f.size), 0, 255).astype(np.uint8)
    per = [ref.interlace([noisy(f) for f in _clip(W, H, NF, s)], W, H, parity) for s in range(S)]
    return [np.stack([per[s][t] for s in range(S)]) for t in range(NF)]


def _model(steps, params=DI, start=0):
    """the steps as the filter leaves them: each stream's sequence, started (spatial only) at step `start`"""
    per = [ref.deint_sequence([st[s] for st in steps[start:]], W, H, params)[0] for s in range(S)]
    return list(steps[:start]) + [np.stack([per[s][t] for s in range(S)]) for t in range(len(steps) - start)]


def _run(steps, feed=None, prepare=None, before=None):
    """one encoder over `steps`, fed by feed(enc, device frames, step) (default: encode), before(enc, t) in front of
    step t: per step the NAL bytes and the rate-control state of every stream"""
    import torch
    import h264mi
    enc = h264mi.BatchEncoder(W, H, 300000, S)
    enc.set_frame_skip(False)
    if prepare:
        prepare(enc)
    out = []
    for t, fr in enumerate(steps):
        if before:
            before(enc, t)
        host = np.ascontiguousarray(fr).ravel()
        frames = torch.from_numpy(host).cuda()  # held until nal_sizes() has synchronised
        if feed:
            feed(enc, frames, fr)
        else:
            enc.encode(frames)
        sizes = enc.nal_sizes()
        st = {'nal': [enc.nal_bytes(s, sizes[s]) for s in range(S)], 'rc': [enc.rc_state(s) for s in range(S)]}
        assert all(len(b) > 0 for b in st['nal'])
        assert np.array_equal(frames.cpu().numpy(), host), "the caller's frames were written"
        out.append(st)
    enc.close()
    return out


def _same(got, want, what=''):
    for t in range(len(want)):
        assert got[t]['nal'] == want[t]['nal'], f'{what} frame {t}: NAL bytes'
        assert got[t]['rc'] == want[t]['rc'], f'{what} frame {t}: rate-control state'


def _on(enc, params=DI):
    enc.set_deinterlace(params)
    d = enc.deinterlace()
    assert d is not None and (d.parity, d.spatial, d.temporal, d.comb_level) == tuple(params)


def test_encoder_equals_encode_of_reference_frames(gpu_lib):
    for parity in (0, 1):
        raw = _interlaced(parity)
        par = (parity, 1, 1, 8)
        clean = _model(raw, par)
        assert all(not np.array_equal(clean[t], raw[t]) for t in range(NF))
        got = _run(raw, prepare=lambda e: _on(e, par))
        _same(got, _run(clean), f'parity {parity}')
        plain = _run(raw)
        assert all(got[t]['nal'] != plain[t]['nal'] for t in range(NF)), 'the filter changed nothing: the test shows nothing'


def _nv12(frames):
    """S tight I420 frames as S tight NV12 frames"""
    out = []
    for f in frames:
        y, u, v = ref.planes(f, W, H)
        out.append(np.concatenate([y.ravel(), np.stack([u, v], axis=-1).ravel()]))
    return np.stack(out)


def test_encoder_through_encode_pix_nv12(gpu_lib):
    import torch
    import h264mi
    raw = _interlaced()
    layout = h264mi.pix_layout_tight(h264mi.PIX_NV12, W, H)

    def feed(enc, frames, fr):
        nv = torch.from_numpy(_nv12(fr).ravel()).cuda()
        enc.encode_pix(nv, layout)
        enc.nal_sizes()  # nv is held until the stream has finished with it

    _same(_run(raw, feed=feed, prepare=_on), _run(_model(raw)))


def test_encoder_runs_the_deinterlacer_in_front_of_denoiser_scenecut_and_overlays(gpu_lib):
    """the models chained in the encoder's order: deintref, then denoiseref's recursion on its frames; the key-frame
    policy and the overlay list are on in both encoders and see those frames"""
    import torch
    import h264mi
    DN, SC = (128, 64, 12, 24), (64, 128, 2, 4, 1)
    raw = _interlaced()
    deint = _model(raw)
    per = [denoiseref.denoise_sequence([st[s] for st in deint], W, H, DN)[0] for s in range(S)]
    clean = [np.stack([per[s][t] for s in range(S)]) for t in range(NF)]
    assert not np.array_equal(clean[2], deint[2])
    sprite = torch.from_numpy(np.random.default_rng(93).integers(0, 256, h264mi.i420a_bytes(16, 16), dtype=np.uint8)).cuda()
    ov = [h264mi.Overlay(0, s, 0, 0, 16, 16, 8, 8, 256, 0) for s in range(S)]

    def tail(enc):
        enc.set_scenecut(SC)
        enc.set_overlays(sprite, 16, 16, 1, ov)

    def all_on(enc):
        tail(enc)
        enc.set_denoise(DN)
        _on(enc)

    got = _run(raw, prepare=all_on)
    _same(got, _run(clean, prepare=tail))
    assert got[3]['nal'] != _run(deint, prepare=tail)[3]['nal'], 'the denoiser changed nothing'


def test_encoder_all_four_stages_off_and_on_again(gpu_lib):
    """all four stages on for frames 0-1, all off in front of frame 2, all on again in front of frame 4: frames 2-3 are
    the raw frames, coded as an encoder with nothing configured codes them behind the same frames 0-1, and from frame 4
    every stage starts anew -- the deinterlacer spatial only, the denoiser with a copy, the detector with thumbnails
    only. The reference encoder is fed the chained models' frames and has only the key-frame policy and the overlay
    list, switched at the same steps"""
    import torch
    import h264mi
    DN, SC = (128, 64, 12, 24), (64, 128, 2, 4, 1)
    raw = _interlaced()

    def chained(lo, hi):
        """steps lo..hi-1 as deintref and then denoiseref's recursion leave them, both started at step lo"""
        deint = _model(raw[:hi], start=lo)[lo:]
        per = [denoiseref.denoise_sequence([st[s] for st in deint], W, H, DN)[0] for s in range(S)]
        return [np.stack([per[s][t] for s in range(S)]) for t in range(hi - lo)]

    first, again, never_off = chained(0, 2), chained(4, NF), chained(0, NF)
    assert not np.array_equal(never_off[2], raw[2]) and not np.array_equal(never_off[3], raw[3]), 'off shows nothing'
    assert not np.array_equal(again[0], never_off[4]) and not np.array_equal(again[1], never_off[5]), 'the restart shows nothing'
    sprite = torch.from_numpy(np.random.default_rng(93).integers(0, 256, h264mi.i420a_bytes(16, 16), dtype=np.uint8)).cuda()
    ov = [h264mi.Overlay(0, s, 0, 0, 16, 16, 8, 8, 256, 0) for s in range(S)]

    def tail(enc):
        enc.set_scenecut(SC)
        enc.set_overlays(sprite, 16, 16, 1, ov)

    def all_on(enc):
        tail(enc)
        enc.set_denoise(DN)
        _on(enc)

    def tail_off(enc):
        enc.set_scenecut(None)
        enc.clear_overlays()
        assert enc.scenecut() is None and enc.overlays() == 0

    def all_off(enc):
        enc.set_deinterlace(None)
        enc.set_denoise(None)
        tail_off(enc)
        assert enc.deinterlace() is None and enc.denoise() is None

    def switched(on, off):
        def before(enc, t):
            if t in (0, 4):
                on(enc)
            if t == 2:
                off(enc)
        return before

    got = _run(raw, before=switched(all_on, all_off))
    _same(got, _run(first + raw[2:4] + again, before=switched(tail, tail_off)))
    assert got[2]['nal'] != _run(never_off[:3], prepare=tail)[2]['nal'], 'frame 2 is coded as if nothing had been turned off'


def test_encoder_off_and_on_again_restarts_spatial_only(gpu_lib):
    """on for frames 0-1, off for 2, on again for 3-5: frame 2 raw, frame 3 spatial only, frame 4 against raw 3"""
    raw = _interlaced()
    first, again = _model(raw[:2]), _model(raw, start=3)[3:]
    assert not np.array_equal(again[0], _model(raw)[3]), 'frame 3 with and without a previous frame are the same'

    def before(enc, t):
        if t == 0 or t == 3:
            _on(enc)
        if t == 2:
            enc.set_deinterlace(None)
            assert enc.deinterlace() is None

    _same(_run(raw, before=before), _run(first + [raw[2]] + again))


def test_encoder_refuses_the_resampling_entry_points_while_on(gpu_lib):
    """scaled, composed, composed_any and oriented return -1 and submit nothing: the accepted frames' bytes are those
    of a run without the refused calls; off again they are accepted"""
    import torch
    import h264mi
    raw = _interlaced()
    big = torch.zeros(S * ref.frame_bytes(2 * W, 2 * H), dtype=torch.uint8, device='cuda')
    same = torch.zeros(S * ref.frame_bytes(W, H), dtype=torch.uint8, device='cuda')
    cells = [h264mi.Cell(s, s, 0, 0, W, H, 0, 0, W, H) for s in range(S)]

    def refused(enc):
        L, e, vp = enc._L, enc._e, ctypes.c_void_p
        arr = (h264mi.Cell * S)(*cells)
        assert L.h264mi_enc_encode_scaled(e, vp(big.data_ptr()), 2 * W, 2 * H) == -1
        assert L.h264mi_enc_encode_composed(e, vp(same.data_ptr()), W, H, S, arr, S, 16, 128, 128) == -1
        assert L.h264mi_enc_encode_composed_any(e, vp(same.data_ptr()), W, H, S, arr, S, 1, 16, 128, 128) == -1
        assert L.h264mi_enc_encode_oriented(e, vp(same.data_ptr()), h264mi.ORIENT_ROT180) == -1
        with pytest.raises(ValueError):
            enc.encode_scaled(big, 2 * W, 2 * H)
        with pytest.raises(ValueError):
            enc.encode_oriented(same, h264mi.ORIENT_ROT180)

    def before(enc, t):
        if t in (0, 2, 5):
            refused(enc)

    _same(_run(raw, prepare=_on, before=before), _run(_model(raw)))
    enc = h264mi.BatchEncoder(W, H, 300000, S)
    _on(enc)
    enc.set_deinterlace(None)
    enc.encode_scaled(big, 2 * W, 2 * H)
    enc.encode_oriented(same, h264mi.ORIENT_ROT180)
    enc.encode_composed(same, W, H, S, cells)
    assert all(n > 0 for n in enc.nal_sizes())
    enc.close()


def test_set_deinterlace_refusals_leave_the_setting_in_force(gpu_lib):
    import h264mi
    raw = _interlaced()

    def refuse(enc):
        for bad in BAD_PARAMS:
            with pytest.raises(ValueError):
                enc.set_deinterlace(bad)
            assert enc._L.h264mi_enc_set_deinterlace(enc._e, ctypes.byref(h264mi.Deinterlace(*bad))) == -1

    def before(enc, t):
        if t == 0:
            refuse(enc)
            assert enc.deinterlace() is None
            _on(enc)
        refuse(enc)
        d = enc.deinterlace()
        assert (d.parity, d.spatial, d.temporal, d.comb_level) == DI
        assert enc._L.h264mi_enc_deinterlace(enc._e, None) == 1

    _same(_run(raw[:3], before=before), _run(_model(raw)[:3]))
