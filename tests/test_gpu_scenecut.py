"""GPU: the scene-cut detector -- the standalone call h264mi_i420_scenecut_dev -- against tests/scenecutref.py, and the
encoder's key-frame policy h264mi_enc_set_scenecut against the oracle with force_idr() called on exactly the frames the
reference's policy model names. Exact integers, so every comparison is equality of bytes and words; every output sits
between 64 guard bytes of 0xA5 that must stay as they were. The kernel's item is 32 luma rows by a strip of 512 samples
(csrc/scenecut.hip), which the shapes below are chosen around."""
import functools

import numpy as np
import pytest

import denoiseref
import scenecutref as ref
from test_scenecut_host import CH, CW, clip_frame, make_pair, pan_clip, switch_clip

pytestmark = pytest.mark.gpu

GUARD = 64

# (w, h, shift): each the smallest shape that reaches its case
#   2x2: one cell of 4 samples; 6x2: a cell 2 wide; 34x18: cells 2 wide and 2 high, a second block row and column, rows
#   that are no multiple of 16 (the byte path); 66x34 and 130x70: more blocks, a thumbnail row of 17 and 33 bytes; 64x32:
#   whole 16-byte words and whole thumbnail dwords, and the same at odd addresses (the byte path for the same bytes);
#   514x34: 2 samples past the 512-sample strip; 48x66: 2 rows past two rows of blocks; 8192x16 and 16x8192: the limits
SHAPES = [(2, 2, 0), (6, 2, 0), (34, 18, 0), (34, 18, 1), (66, 34, 0), (130, 70, 0), (130, 70, 1), (64, 32, 0), (64, 32, 1), (528, 64, 0),
          (514, 34, 0), (48, 66, 0), (8192, 16, 0), (16, 8192, 0)]
SHAPE_IDS = [f'{w}x{h}' + ('-odd-address' if s else '') for w, h, s in SHAPES]
PARAM_SETS = [(24, 128, 4, 0, 1), (64, 128, 4, 0, 0), (0, 1, 0, 0, 1), (1020, 256, 0, 9, 0)]


@functools.lru_cache(maxsize=None)
def _content(w, h, n):
    """(cur frames, prev thumbnails): n different frame pairs; shared, never written"""
    pairs = [make_pair(w, h, 1000 * f + 3 * w + h) for f in range(n)]
    cur = np.stack([p[0] for p in pairs])
    tp = np.stack([ref.thumbnail(p[1], w, h) for p in pairs])
    cur.setflags(write=False)
    tp.setflags(write=False)
    return cur, tp


def _guarded(data, shift=0):
    """(whole, view): data's bytes on the device between 64 bytes of 0xA5 on each side, `shift` bytes into the allocation"""
    import torch
    data = np.ascontiguousarray(data).view(np.uint8).ravel()
    whole = torch.full((shift + data.size + 2 * GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    view = whole[shift + GUARD:shift + GUARD + data.size]
    view.copy_(torch.from_numpy(data.copy()))
    return whole, view


def _guards_intact(whole, nbytes, shift=0):
    h = whole.cpu().numpy()
    return bool((h[:shift + GUARD] == 0xA5).all() and (h[shift + GUARD + nbytes:] == 0xA5).all())


def _scenecut(cur, tp, w, h, params, shift=0, out='new', stats=True, prev=True, tshift=None):
    """the standalone call on cur's n frames. out: 'new' (a fresh guarded buffer of 0x5A), 'prev' (in place) or None.
    shift moves the frames, tshift (default: shift) the thumbnails. Returns (thumbnails or None, stats rows or None);
    guards and the inputs are checked"""
    import torch
    import h264mi
    n = cur.shape[0]
    tshift = shift if tshift is None else tshift
    wc, d_cur = _guarded(cur, shift)
    wp, d_tp = _guarded(tp, tshift) if prev else (None, None)
    if out == 'new':
        wo, d_out = _guarded(np.full(tp.size, 0x5A, np.uint8), tshift)
    else:
        wo, d_out = (wp, d_tp) if out == 'prev' else (None, None)
    if shift:
        assert d_cur.data_ptr() % 2 == 1
    ws, d_st = _guarded(np.full(32 * n, 0x7F, np.uint8)) if stats else (None, None)
    h264mi.i420_scenecut(d_cur, w, h, n, params, thumb_out=d_out, thumb_prev=d_tp, stats=d_st)
    torch.cuda.synchronize()
    assert _guards_intact(wc, cur.size, shift) and np.array_equal(d_cur.cpu().numpy(), cur.ravel()), 'the frames were written'
    if wp is not None:
        assert _guards_intact(wp, tp.size, tshift), 'bytes outside the previous thumbnails were written'
        if out != 'prev':
            assert np.array_equal(d_tp.cpu().numpy(), tp.ravel()), 'the previous thumbnails were written'
    if wo is not None:
        assert _guards_intact(wo, tp.size, tshift), 'bytes outside the thumbnails were written'
    if ws is not None:
        assert _guards_intact(ws, 32 * n), 'bytes outside the statistics were written'
    got = d_out.cpu().numpy().reshape(tp.shape) if d_out is not None else None
    st = d_st.cpu().numpy().view(np.uint32).astype(np.int64).reshape(n, 8).tolist() if stats else None
    return got, st


def _want(cur, tp, w, h, params):
    tc = np.stack([ref.thumbnail(f, w, h) for f in cur])
    return tc, [ref.frame_stats(tc[f], tp[f], params) for f in range(cur.shape[0])]


@pytest.mark.parametrize('w,h,shift', SHAPES, ids=SHAPE_IDS)
def test_standalone_vs_reference(gpu_lib, w, h, shift):
    big = w * h > 100000
    for n in ((1,) if big else (1, 3)):
        cur, tp = _content(w, h, n)
        for params in (PARAM_SETS[:2] if big else PARAM_SETS):
            want_t, want_st = _want(cur, tp, w, h, params)
            got_t, got_st = _scenecut(cur, tp, w, h, params, shift)
            assert np.array_equal(got_t, want_t), f'n={n} {params}: {int((got_t != want_t).sum())} thumbnail bytes differ'
            assert got_st == want_st, f'n={n} {params}: statistics {got_st} != {want_st}'
    if ((w + 31) // 32) * ((h + 31) // 32) >= 4:  # the case is worth trusting: changed and unchanged blocks in it
        assert all(0 < s[0] < s[1] for s in _want(cur, tp, w, h, PARAM_SETS[0])[1])


@pytest.mark.parametrize('w,h,shift', [(34, 18, 0), (130, 70, 1), (64, 32, 0), (514, 34, 0)], ids=['34x18', '130x70-odd-address', '64x32', '514x34'])
def test_in_place_statistics_only_thumbnails_only(gpu_lib, w, h, shift):
    cur, tp = _content(w, h, 3)
    for params in PARAM_SETS[:2]:
        want_t, want_st = _want(cur, tp, w, h, params)
        got_t, got_st = _scenecut(cur, tp, w, h, params, shift, out='prev')  # d_thumb_out == d_thumb_prev
        assert np.array_equal(got_t, want_t) and got_st == want_st, 'in place'
        got_t, got_st = _scenecut(cur, tp, w, h, params, shift, out=None)
        assert got_t is None and got_st == want_st, 'statistics only'
        got_t, got_st = _scenecut(cur, tp, w, h, params, shift, stats=False, prev=False)
        assert np.array_equal(got_t, want_t) and got_st is None, 'thumbnails only'
        got_t, got_st = _scenecut(cur, tp, w, h, params, shift, stats=False)
        assert np.array_equal(got_t, want_t), 'previous thumbnails given, no statistics'
    a = _scenecut(cur, tp, w, h, PARAM_SETS[0], shift)
    b = _scenecut(cur, tp, w, h, PARAM_SETS[0], shift)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]


# frames and thumbnails at independent alignments: 64x32 has whole 16-byte words and whole thumbnail dwords, so (0, 1) is
# words of luma with bytes of thumbnail and (1, 0) the reverse; 30x18 and 14x6 have thumbnail rows of 8 and 4 bytes --
# dwords -- whose last cell is 2 samples wide, under luma rows that are no multiple of 16 (bytes)
@pytest.mark.parametrize('w,h', [(64, 32), (30, 18), (14, 6)])
@pytest.mark.parametrize('shift,tshift', [(0, 1), (1, 0), (0, 0)], ids=['thumbnails+1', 'frames+1', 'aligned'])
def test_frames_and_thumbnails_on_different_paths(gpu_lib, w, h, shift, tshift):
    cur, tp = _content(w, h, 3)
    for params in PARAM_SETS[:2]:
        want_t, want_st = _want(cur, tp, w, h, params)
        for out in ('new', 'prev'):
            got_t, got_st = _scenecut(cur, tp, w, h, params, shift, out=out, tshift=tshift)
            assert np.array_equal(got_t, want_t) and got_st == want_st, (params, out)
        got_t, _ = _scenecut(cur, tp, w, h, params, shift, stats=False, prev=False, tshift=tshift)
        assert np.array_equal(got_t, want_t)


def test_identical_uniform_step_and_the_share_boundary(gpu_lib):
    import h264mi
    w, h = 66, 34  # 3 x 2 blocks
    rng = np.random.default_rng(8)
    prev = rng.integers(20, 200, ref.frame_bytes(w, h), dtype=np.uint8)
    tp = ref.thumbnail(prev, w, h)[None]
    for comp in (0, 1):
        _, st = _scenecut(prev[None], tp, w, h, (0, 128, 0, 0, comp))
        assert st == [ref.frame_stats(tp[0], tp[0], (0, 128, 0, 0, comp))] and st[0][0] == 0 and st[0][2] == 0
        step = (prev + 7).astype(np.uint8)[None]
        got_t, st = _scenecut(step, tp, w, h, (27, 128, 0, 0, comp))
        assert np.array_equal(got_t, tp + 7) and st == [ref.frame_stats(tp[0] + 7, tp[0], (27, 128, 0, 0, comp))]
        assert st[0][0] == (0 if comp else 6) and st[0][2] == 7 * tp.size
    # exactly half of the blocks changed: no cut at share 128 (256 * 3 == 128 * 6), a cut one block above
    for nchanged, cut in ((3, 0), (4, 1)):
        cur = prev.copy()
        Y = cur[:w * h].reshape(h, w)
        for k in range(nchanged):
            bx, by = k % 3, k // 3
            ys, xs = slice(32 * by, min(32 * by + 32, h)), slice(32 * bx, min(32 * bx + 32, w))
            Y[ys, xs] = rng.integers(0, 256, Y[ys, xs].shape, dtype=np.uint8)
        half = (24, 128, 0, 0, 0)
        _, st = _scenecut(cur[None], tp, w, h, half)
        assert st == [ref.frame_stats(ref.thumbnail(cur, w, h), tp[0], half)] and st[0][:2] == [nchanged, 6]
        assert h264mi.scenecut_is_cut(half, st[0]) == cut and bool(ref.is_cut(half, st[0])) == bool(cut)


def test_standalone_refusals_leave_the_outputs_untouched(gpu_lib):
    import ctypes
    import torch
    import h264mi
    from test_scenecut_host import BAD_PARAMS, BAD_SHAPES
    fn = gpu_lib.h264mi_i420_scenecut_dev
    w, h, n = 32, 16, 3
    fb, tb = n * ref.frame_bytes(w, h), n * 8 * 4
    wo, d_out = _guarded(np.full(tb, 0x5A, np.uint8))
    ws, d_st = _guarded(np.full(32 * n, 0x5A, np.uint8))
    _, d_cur = _guarded(np.zeros(fb, np.uint8))
    _, d_tp = _guarded(np.zeros(tb, np.uint8))
    good = ctypes.byref(h264mi.Scenecut(*ref.DEFAULT))
    vp = ctypes.c_void_p
    ST, TO, CU, TP = d_st.data_ptr(), d_out.data_ptr(), d_cur.data_ptr(), d_tp.data_ptr()

    def call(stats=ST, tout=TO, cur=CU, tprev=TP, ww=w, hh=h, nn=n, p=good):
        return fn(vp(stats) if stats else None, vp(tout) if tout else None, vp(cur) if cur else None, vp(tprev) if tprev else None, ww, hh, nn, p, None)

    assert call(cur=0) == -1 and call(p=None) == -1 and call(stats=0, tout=0) == -1 and call(tprev=0) == -1
    for ww, hh, nn in BAD_SHAPES:
        assert call(ww=ww, hh=hh, nn=nn) == -1, (ww, hh, nn)
    for bad in BAD_PARAMS:
        assert call(p=ctypes.byref(h264mi.Scenecut(*bad))) == -1, bad
    assert call(stats=ST + 1) == -1 and call(stats=ST + 2) == -1
    for off in (1, tb - 1, -1, -(tb - 1)):
        assert call(tout=TP + off) == -1
    for off in (0, fb - 1, -(tb - 1)):
        assert call(tout=CU + off) == -1 and call(tprev=CU + off) == -1
    for base, nb in ((CU, fb), (TO, tb), (TP, tb)):
        assert call(stats=base) == -1 and call(stats=base + nb - 4) == -1 and call(stats=base - 4) == -1
    torch.cuda.synchronize()
    for whole, view, nb in ((wo, d_out, tb), (ws, d_st, 32 * n)):
        assert _guards_intact(whole, nb) and (view.cpu().numpy() == 0x5A).all(), 'a refused call wrote'
    assert call() == 0
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0).all() and _guards_intact(wo, tb) and _guards_intact(ws, 32 * n)
    assert d_st.cpu().numpy().view(np.uint32).reshape(n, 8).tolist() == [[0, 1, 0, 0, 0, 0, 0, 0]] * n


# ---------------------------------------------------------------- the encoder's policy

W, H, S, NF = CW, CH, 3, 14
POLICY = (64, 128, 3, 8, 1)
WORDS = ('cut', 'key', 'reason', 'dist', 'keys_by_cut', 'keys_by_period', 'keys_other', 'frames')


@functools.lru_cache(maxsize=None)
def _streams(switches=((), (5,), (3, 4))):
    """per stream its NF frames: the pan with noise, the scene replaced at the stream's indices"""
    return tuple(pan_clip(NF) if not sw else switch_clip(NF, tuple(sw)) for sw in switches)


def _model(streams, params, forced=frozenset(), first=True, start=0):
    """per stream, per frame from `start` on, the sixteen words"""
    return [ref.policy_states(list(fr[start:]), W, H, params, forced, first) for fr in streams]


def _state_words(enc, s):
    st = enc.scenecut_state(s)
    return st['stats'] + [st[k] for k in WORDS]


def _nal_types(b):
    """nal_unit_type of every NAL unit of an Annex-B string"""
    a = np.frombuffer(b, np.uint8)
    at = [i for i in range(len(a) - 3) if a[i] == 0 and a[i + 1] == 0 and a[i + 2] == 1]
    return [int(a[i + 3]) & 31 for i in at]


def _run(streams, bitrate=300000, skip=False, prepare=None, before=None, states=True):
    """one encoder over the streams' frames: per frame the streams' NAL bytes and, with the policy on, state words"""
    import torch
    import h264mi
    enc = h264mi.BatchEncoder(W, H, bitrate, len(streams))
    enc.set_frame_skip(skip)
    if prepare:
        prepare(enc)
    out = []
    for t in range(len(streams[0])):
        if before:
            before(enc, t)
        fr = np.ascontiguousarray(np.stack([st[t] for st in streams])).ravel()
        frames = torch.from_numpy(fr).cuda()  # held until nal_sizes() has synchronised
        enc.encode(frames)
        sizes = enc.nal_sizes()
        rec = {'nal': [enc.nal_bytes(s, sizes[s]) if sizes[s] > 0 else b'' for s in range(len(streams))]}
        if states and enc.scenecut() is not None:
            rec['words'] = [_state_words(enc, s) for s in range(len(streams))]
        assert np.array_equal(frames.cpu().numpy(), fr), "the caller's frames were written"
        out.append(rec)
    enc.close()
    return out


def _oracle_run(oracle, frames, keys, bitrate=300000, skip=False):
    """one stream through the oracle, force_idr() in front of every frame in `keys`: per frame the NAL bytes"""
    o = oracle.encoder(W, H, bitrate)
    o.set_frame_skip(skip)
    out = []
    for t, f in enumerate(frames):
        if t in keys:
            o.force_idr()
        out.append(o.encode(f))
    return out


def _on(enc, params=POLICY):
    enc.set_scenecut(params)
    d = enc.scenecut()
    assert d is not None and (d.level, d.share, d.min_gap, d.max_gap, d.compensate) == tuple(params)


def _check_against_oracle(oracle, got, streams, model, bitrate=300000, skip=False):
    for s, fr in enumerate(streams):
        keys = {t for t, wd in enumerate(model[s]) if wd[9]}
        want = _oracle_run(oracle, fr, keys, bitrate, skip)
        for t in range(len(fr)):
            assert got[t]['nal'][s] == want[t], f'stream {s} frame {t}: NAL bytes'
            assert got[t]['words'][s] == model[s][t], f'stream {s} frame {t}: state {got[t]["words"][s]} != {model[s][t]}'
            if want[t]:
                assert (5 in _nal_types(want[t])) == (t in keys), f'stream {s} frame {t}: nal_unit_type 5'
            else:
                assert t not in keys, 'a key frame was skipped'


def test_encoder_keys_equal_the_oracle_forced_at_the_models_frames(gpu_lib, oracle):
    streams = _streams()
    model = _model(streams, POLICY)
    keys = [[(t, wd[10]) for t, wd in enumerate(m) if wd[9]] for m in model]
    # first frame; the period; a cut at 5 and the period counted from it; a cut at 3, the one at 4 held back by min_gap
    assert keys == [[(0, 3), (8, 2)], [(0, 3), (5, 1), (13, 2)], [(0, 3), (3, 1), (11, 2)]]
    assert model[2][4][0] * 2 > model[2][4][1] and model[2][4][8] == 0
    got = _run(streams, prepare=_on)
    _check_against_oracle(oracle, got, streams, model)
    plain = _run(streams)
    assert got[8]['nal'][0] != plain[8]['nal'][0] and got[4]['nal'][0] == plain[4]['nal'][0]


def test_encoder_with_frame_skipping_never_skips_a_key_frame(gpu_lib, oracle):
    streams = _streams()
    model = _model(streams, POLICY)
    got = _run(streams, bitrate=24000, skip=True, prepare=_on)
    _check_against_oracle(oracle, got, streams, model, bitrate=24000, skip=True)
    assert any(not got[t]['nal'][s] for t in range(NF) for s in range(S)), 'no frame was skipped: the test shows nothing'


def test_encoder_host_force_idr_counts_as_other_and_resets_dist(gpu_lib, oracle):
    streams = _streams()
    model = _model(streams, POLICY, forced={6})
    assert [(t, wd[10]) for t, wd in enumerate(model[0]) if wd[9]] == [(0, 3), (6, 3)]  # the period would be at 14
    assert model[1][6][10] == 3 and model[1][6][11] == 0

    def before(enc, t):
        if t == 6:
            enc.force_idr(-1)

    got = _run(streams, prepare=_on, before=before)
    _check_against_oracle(oracle, got, streams, model)


def test_encoder_overlays_do_not_reach_the_detector(gpu_lib):
    import torch
    import h264mi
    streams = _streams()
    sprite = torch.from_numpy(np.full(h264mi.i420a_bytes(32, 32), 255, np.uint8)).cuda()  # white, opaque
    ov = [h264mi.Overlay(0, s, 0, 0, 32, 32, 32, 16, 256, 0) for s in range(S)]

    def both(enc):
        enc.set_overlays(sprite, 32, 32, 1, ov)
        _on(enc)

    got = _run(streams, prepare=both)
    want = _run(streams, prepare=_on)
    model = _model(streams, POLICY)
    for t in range(NF):
        assert got[t]['words'] == want[t]['words'] == [model[s][t] for s in range(S)], f'frame {t}'
    assert all(got[0]['nal'][s] != want[0]['nal'][s] for s in range(S)), 'the overlay changed nothing'


def test_encoder_detector_sees_the_denoised_frames(gpu_lib):
    DN = (224, 224, 16, 40)
    rng = np.random.default_rng(9)  # still scenes under noise of +-6 (a pan's blocks all move: nothing is filtered), one switch
    streams = tuple(tuple(clip_frame(1 + s + (s == 1 and t >= 5), 10, 10, 0, rng.integers(-6, 7, (H, W))) for t in range(NF)) for s in range(S))
    clean = tuple(tuple(denoiseref.denoise_sequence(list(fr), W, H, DN)[0]) for fr in streams)
    model, raw_model = _model(clean, POLICY), _model(streams, POLICY)
    assert any(model[s][t][:5] != raw_model[s][t][:5] for s in range(S) for t in range(NF)), 'the filter changes no statistics'

    def both(enc):
        enc.set_denoise(DN)
        _on(enc)

    got = _run(streams, prepare=both)
    for t in range(NF):
        assert got[t]['words'] == [model[s][t] for s in range(S)], f'frame {t}'


def test_encoder_on_off_on_and_new_parameters_keep_or_drop_the_state(gpu_lib):
    streams = _streams(((6,), (5,), (3, 4)))  # stream 0 switches at the frame the policy comes back on
    other = (64, 128, 0, 8, 1)

    def before(enc, t):
        if t == 0 or t == 6:
            _on(enc)
        if t == 2:
            _on(enc, other)  # other parameters: the state stays
        if t == 4:
            enc.set_scenecut(None)
            assert enc.scenecut() is None
            with pytest.raises(RuntimeError):
                enc.scenecut_state(0)

    got = _run(streams, before=before)
    first = _model(streams, POLICY)
    again = _model(streams, POLICY, first=False, start=6)
    for s in range(S):
        assert [got[t]['words'][s] for t in range(2)] == first[s][:2]
        assert 'words' not in got[4] and 'words' not in got[5]
        assert [got[t]['words'][s] for t in range(6, NF)] == again[s], f'stream {s}'
    assert got[6]['words'][0][8:12] == [0, 0, 0, 1], 'the first frame after turning the policy on is no cut'
    # frames 2 and 3 under min_gap 0: stream 2's switch at 3 is a cut at dist 3 either way, its words carry on from frame 1
    assert got[3]['words'][2][8:12] == [1, 1, 1, 0] and got[3]['words'][2][15] == 4


def test_encoder_share_to_zero_and_back_starts_the_thumbnails_afresh(gpu_lib):
    streams = _streams(((6,), (5,), (3, 4)))  # stream 0 switches at the frame the detector comes back

    def before(enc, t):
        if t == 0 or t == 6:
            _on(enc)
        if t == 3:
            _on(enc, (0, 0, 0, 8, 0))  # period only: the words stay, the thumbnails go

    got = _run(streams, before=before)
    first = _model(streams, POLICY)
    for s in range(S):
        assert [got[t]['words'][s] for t in range(3)] == first[s][:3]
        assert all(got[t]['words'][s][:9] == [0] * 9 for t in range(3, 7)), 'no statistics and no cut without a previous thumbnail'
        assert [got[t]['words'][s][15] for t in range(NF)] == list(range(1, NF + 1)), 'the words carried on'
    assert got[7]['words'][0][1] == 9 and got[7]['words'][0][8] == 0
    # stream 0: first frame, then nothing but the period, counted through both changes of the parameters
    assert [t for t in range(NF) if got[t]['words'][0][9]] == [0, 8]


def test_encoder_off_is_the_encoder_that_never_heard_of_the_policy(gpu_lib):
    streams = _streams()

    def off(enc):
        _on(enc)
        enc.set_scenecut((64, 0, 4, 0, 1))  # share 0 and max_gap 0: off
        assert enc.scenecut() is None
        enc.set_scenecut(None)
        for bad in ((64, 257, 4, 0, 1), (-1, 128, 4, 0, 1)):
            with pytest.raises(ValueError):
                enc.set_scenecut(bad)
        assert enc.scenecut() is None

    got, plain = _run(streams, prepare=off), _run(streams)
    assert [g['nal'] for g in got] == [p['nal'] for p in plain]


def test_encoder_period_only(gpu_lib, oracle):
    streams = _streams()
    params = (0, 0, 0, 4, 0)
    model = _model(streams, params)
    assert all([t for t, wd in enumerate(m) if wd[9]] == [0, 4, 8, 12] and all(wd[:9] == [0] * 9 for wd in m) for m in model)
    got = _run(streams, prepare=lambda enc: _on(enc, params))
    _check_against_oracle(oracle, got, streams, model)
