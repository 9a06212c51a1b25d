"""CPU: the scene-cut detector and the key-frame policy exist at every layer -- declared in include/h264mi.h, exported by
the library, bound in Python --, the vectorised reference of the GPU tests (tests/scenecutref.py) equals the definition
written as loops, the rule's properties hold exactly, the policy model follows the header, h264mi_scenecut_ok and
h264mi_i420_scenecut_dev refuse bad arguments before touching a device, and the documented default parameters name
exactly the content switches of three synthetic clips."""
import ctypes
import functools

import numpy as np
import pytest

import scenecutref as ref
from test_capi_exports import declared_functions

NEW = ('h264mi_scenecut_ok', 'h264mi_thumb_size', 'h264mi_scenecut_is_cut', 'h264mi_i420_scenecut_dev', 'h264mi_enc_set_scenecut',
       'h264mi_enc_scenecut', 'h264mi_enc_scenecut_state')
# (level, share, min_gap, max_gap, compensate)
PARAMS = [ref.DEFAULT, (64, 128, 4, 0, 0), (0, 1, 0, 0, 0), (0, 256, 0, 0, 1), (1020, 1, 0, 9, 1), (24, 64, 0, 0, 0)]
SIZES = [(2, 2), (6, 2), (34, 18), (66, 34), (130, 70)]


def make_pair(w, h, seed):
    """(cur, prev) of one frame: prev random luma; cur = prev plus noise in -5..5, with every other 32x32 block (counted row by
    row, from the second) fresh random samples and every third one a uniform step of +9"""
    rng = np.random.default_rng(seed)
    prev = rng.integers(0, 256, ref.frame_bytes(w, h), dtype=np.uint8)
    cur = np.clip(prev.astype(np.int32) + rng.integers(-5, 6, prev.size), 0, 255).astype(np.uint8)
    C, P = cur[:w * h].reshape(h, w), prev[:w * h].reshape(h, w)
    k = 0
    for by in range((h + 31) // 32):
        for bx in range((w + 31) // 32):
            ys, xs = slice(32 * by, min(32 * by + 32, h)), slice(32 * bx, min(32 * bx + 32, w))
            if k % 2 == 1:
                C[ys, xs] = rng.integers(0, 256, C[ys, xs].shape, dtype=np.uint8)
            elif k % 3 == 2:
                C[ys, xs] = np.clip(P[ys, xs].astype(np.int32) // 2 + 60 + 9, 0, 255)
                P[ys, xs] = P[ys, xs] // 2 + 60
            k += 1
    return cur, prev


def test_header_declares_library_exports_python_binds(libpath):
    names = declared_functions()
    L = ctypes.CDLL(libpath)
    for n in NEW:
        assert n in names, n
        assert hasattr(L, n), n
    import h264mi
    B = h264mi.lib()
    assert [len(getattr(B, n).argtypes) for n in NEW] == [1, 4, 2, 9, 2, 2, 3]
    for f in ('scenecut_ok', 'scenecut_is_cut', 'thumb_size', 'i420_scenecut'):
        assert callable(getattr(h264mi, f)), f
    for f in ('set_scenecut', 'scenecut', 'scenecut_state'):
        assert callable(getattr(h264mi.BatchEncoder, f)), f
    assert ctypes.sizeof(h264mi.Scenecut) == 20
    assert [k for k, _ in h264mi.Scenecut._fields_] == ['level', 'share', 'min_gap', 'max_gap', 'compensate']
    assert tuple(h264mi.SCENECUT_DEFAULT) == ref.DEFAULT


@pytest.mark.parametrize('params', PARAMS, ids=[str(p) for p in PARAMS])
def test_vectorised_reference_equals_the_loops(params):
    for w, h in SIZES:
        cur, prev = make_pair(w, h, 7 * w + h)
        tc, tp = ref.thumbnail(cur, w, h), ref.thumbnail(prev, w, h)
        assert tc.shape == ref.thumb_size(w, h)[::-1]
        assert np.array_equal(tc, ref.thumbnail_loops(cur, w, h)), (w, h)
        assert np.array_equal(tp, ref.thumbnail_loops(prev, w, h)), (w, h)
        a, b = ref.frame_stats(tc, tp, params), ref.frame_stats_loops(tc, tp, params)
        assert a == b, (w, h, a, b)
        assert a[1] == ((w + 31) // 32) * ((h + 31) // 32) and a[5:] == [0, 0, 0]


def test_thumbnail_rounds_and_edge_cells():
    f = np.zeros(ref.frame_bytes(6, 2), np.uint8)
    f[:12] = [1, 2, 3, 4, 9, 10, 1, 2, 3, 5, 9, 11]  # cells: 8 samples summing 21, 4 samples summing 39
    assert ref.thumbnail(f, 6, 2).tolist() == [[(21 + 4) // 8, (39 + 2) // 4]]
    assert ref.thumb_size(8192, 8192) == (2048, 2048) and ref.thumb_size(2, 2) == (1, 1) and ref.thumb_size(34, 18) == (9, 5)


def test_dsum_never_exceeds_sad():
    for w, h in SIZES:
        for seed in range(3):
            cur, prev = make_pair(w, h, 100 * seed + w)
            sad, dsum, _ = ref.block_stats(ref.thumbnail(cur, w, h), ref.thumbnail(prev, w, h), ref.DEFAULT)
            assert (dsum <= sad).all()


def test_uniform_step_and_identical_frames():
    w, h = 130, 70
    rng = np.random.default_rng(3)
    prev = rng.integers(20, 200, ref.frame_bytes(w, h), dtype=np.uint8)
    tp = ref.thumbnail(prev, w, h)
    for k in (1, 7, 40):
        cur = (prev + k).astype(np.uint8)
        tc = ref.thumbnail(cur, w, h)
        assert np.array_equal(tc, tp + k)
        for level in (0, 4 * k - 1, 4 * k):
            on = ref.frame_stats(tc, tp, (level, 128, 0, 0, 1))
            off = ref.frame_stats(tc, tp, (level, 128, 0, 0, 0))
            assert on[0] == 0 and on[2] == k * tp.size, (k, level)
            assert off[0] == (off[1] if 4 * k > level else 0), (k, level)
    for comp in (0, 1):
        st = ref.frame_stats(tp, tp, (0, 1, 0, 0, comp))
        assert st[0] == 0 and st[2] == 0 and st[3] == st[4] == int(tp.astype(np.int64).sum())


def test_the_gate_is_exact():
    tp = np.full((8, 8), 100, np.uint8)
    for m, changed in ((96, 0), (97, 1)):  # level 6 on 64 cells: 4 m > 384
        tc = tp.copy()
        tc.ravel()[:m - 64] += 2
        tc.ravel()[m - 64:] += 1
        for fn in (ref.frame_stats, ref.frame_stats_loops):
            assert fn(tc, tp, (6, 1, 0, 0, 0))[:3] == [changed, 1, m]
    # compensated: 24 cells up by 2, 24 down by 2, then one more pair by 1: dsum = 0, m = sad = 96, 98 (sad and dsum have
    # one parity, so m is even: 98 is the next value)
    for extra, changed in ((0, 0), (1, 1)):
        tc = tp.copy()
        tc.ravel()[:24] += 2
        tc.ravel()[24:48] -= 2
        tc.ravel()[48:48 + extra] += 1
        tc.ravel()[50:50 + extra] -= 1
        for fn in (ref.frame_stats, ref.frame_stats_loops):
            assert fn(tc, tp, (6, 1, 0, 0, 1))[:3] == [changed, 1, 96 + 2 * extra]
    # an edge block of one cell
    one = np.full((1, 1), 50, np.uint8)
    assert ref.frame_stats(one + 1, one, (4, 1, 0, 0, 0))[0] == 0 and ref.frame_stats(one + 1, one, (3, 1, 0, 0, 0))[0] == 1


def test_is_cut_is_exact(libpath):
    import h264mi
    for share, changed, blocks, cut in ((128, 4, 8, 0), (128, 5, 8, 1), (256, 9, 9, 0), (1, 0, 9, 0), (1, 1, 256, 0), (1, 1, 255, 1), (0, 9, 9, 0),
                                       (256, 65536, 65536, 0), (255, 65536, 65536, 1)):
        stats = [changed, blocks, 0, 0, 0, 0, 0, 0]
        p = (32, share, 0, 7 if share == 0 else 0, 1)
        assert bool(ref.is_cut(p, stats)) == bool(cut), (share, changed, blocks)
        assert h264mi.scenecut_is_cut(p, stats) == cut, (share, changed, blocks)
    assert h264mi.scenecut_is_cut((32, 257, 0, 0, 1), [0] * 8) == -1 and h264mi.scenecut_is_cut(None, [0] * 8) == -1
    assert h264mi.lib().h264mi_scenecut_is_cut(ctypes.byref(h264mi.Scenecut(*ref.DEFAULT)), None) == -1


# ---------------------------------------------------------------- the policy model

def _still(n, w=32, h=32):
    f = np.full(ref.frame_bytes(w, h), 90, np.uint8)
    return [f] * n


def _switching(at, n, w=32, h=32):
    """n frames whose luma alternates between two random pictures at every index in `at`"""
    rng = np.random.default_rng(1)
    a, b = (rng.integers(0, 256, ref.frame_bytes(w, h), dtype=np.uint8) for _ in range(2))
    out, cur = [], a
    for t in range(n):
        if t in at:
            cur = b if cur is a else a
        out.append(cur)
    return out


def test_policy_period_only():
    seq = ref.policy_sequence(_still(10), 32, 32, (0, 0, 0, 4, 0))
    assert [t for t, s in enumerate(seq) if s[0]] == [0, 4, 8]
    assert [s[1] for s in seq] == [3, 0, 0, 0, 2, 0, 0, 0, 2, 0]
    assert [s[2] for s in seq] == [0, 1, 2, 3, 0, 1, 2, 3, 0, 1]
    # switches are not looked at without a share
    assert ref.policy_sequence(_switching({2}, 6), 32, 32, (0, 0, 0, 4, 0)) == ref.policy_sequence(_still(6), 32, 32, (0, 0, 0, 4, 0))


def test_policy_min_gap_forced_and_priority():
    p = (32, 128, 3, 8, 1)
    seq = ref.policy_sequence(_switching({3, 4, 9}, 14), 32, 32, p)
    #                      0          3: cut (dist 3)   4: suppressed (dist 1 < 3)        9: cut    11 = 3 + 8: no, 9 reset it
    assert [t for t, s in enumerate(seq) if s[0]] == [0, 3, 9]
    assert seq[3] == (True, 1, 0) and seq[4] == (False, 0, 1) and seq[9] == (True, 1, 0) and seq[13] == (False, 0, 4)
    st = ref.policy_states(_switching({3, 4, 9}, 14), 32, 32, p)
    assert st[4][0] == st[4][1] == 1 and st[4][8] == 0, 'the suppressed cut is in the statistics, not in cut'
    assert st[13][12:] == [2, 0, 1, 14]
    # a forced frame resets dist: the period counts from it; forced beats period beats cut
    seq = ref.policy_sequence(_still(16), 32, 32, (32, 128, 0, 8, 1), forced={6})
    assert [(t, s[1]) for t, s in enumerate(seq) if s[0]] == [(0, 3), (6, 3), (14, 2)]
    seq = ref.policy_sequence(_switching({8}, 10), 32, 32, (32, 128, 0, 8, 1), forced={8})
    assert seq[8] == (True, 3, 0)
    seq = ref.policy_sequence(_switching({8}, 10), 32, 32, (32, 128, 0, 8, 1))
    assert seq[8] == (True, 2, 0), 'period before cut'
    seq = ref.policy_sequence(_switching({5}, 10), 32, 32, (32, 128, 0, 8, 1))
    assert seq[5] == (True, 1, 0) and seq[8] == (False, 0, 3)
    # turned on in the middle of a stream: the first frame is no key and only stores a thumbnail
    seq = ref.policy_states(_switching({0, 1}, 4), 32, 32, (32, 128, 0, 0, 1), first=False)
    assert seq[0][:12] == [0] * 8 + [0, 0, 0, 1] and seq[1][8:12] == [1, 1, 1, 0]


# ---------------------------------------------------------------- refusals, no device

BAD_PARAMS = [(-1, 128, 4, 0, 1), (1021, 128, 4, 0, 1), (32, -1, 4, 0, 1), (32, 257, 4, 0, 1), (32, 128, -1, 0, 1), (32, 128, 65536, 0, 1),
              (32, 128, 4, -1, 1), (32, 128, 4, 65536, 1), (32, 128, 4, 0, -1), (32, 128, 4, 0, 2)]
LIMIT_PARAMS = [(0, 0, 0, 0, 0), (1020, 256, 65535, 65535, 1)]
BAD_SHAPES = [(32, 32, 0), (32, 32, -1), (31, 32, 1), (32, 31, 1), (0, 32, 1), (32, 0, 1), (-2, 32, 1), (8194, 32, 1), (32, 8194, 1)]


def test_scenecut_ok_and_thumb_size_at_the_limits(libpath):
    import h264mi
    B = h264mi.lib()
    for p in LIMIT_PARAMS + PARAMS:
        assert h264mi.scenecut_ok(p) == 0 and ref.params_ok(p), p
    for p in BAD_PARAMS:
        assert h264mi.scenecut_ok(p) == -1 and not ref.params_ok(p), p
    assert h264mi.scenecut_ok(None) == -1 and B.h264mi_scenecut_ok(None) == -1
    good = ctypes.byref(h264mi.Scenecut(*ref.DEFAULT))
    assert B.h264mi_enc_set_scenecut(None, good) == -1 and B.h264mi_enc_scenecut(None, None) == -1
    assert B.h264mi_enc_scenecut_state(None, 0, (ctypes.c_uint32 * 16)()) == -1
    for w, h in SIZES + [(8192, 8192), (8190, 2)]:
        assert h264mi.thumb_size(w, h) == ref.thumb_size(w, h)
    tw = ctypes.c_int(-7)
    for w, h, _ in BAD_SHAPES[2:]:
        with pytest.raises(ValueError):
            h264mi.thumb_size(w, h)
    assert B.h264mi_thumb_size(32, 32, None, ctypes.byref(tw)) == -1 and B.h264mi_thumb_size(32, 32, ctypes.byref(tw), None) == -1 and tw.value == -7


def test_scenecut_dev_refuses_bad_arguments_without_a_device(libpath):
    import h264mi
    fn = h264mi.lib().h264mi_i420_scenecut_dev
    good = ctypes.byref(h264mi.Scenecut(*ref.DEFAULT))
    vp = ctypes.c_void_p
    w, h, n = 32, 16, 3
    fb, tb, sb = n * ref.frame_bytes(w, h), n * 8 * 4, 32 * n
    St, To, Cu, Tp = (0x10000000 + k * 0x100000 for k in range(4))  # far apart

    def call(stats=St, tout=To, cur=Cu, tprev=Tp, ww=w, hh=h, nn=n, p=good):
        return fn(vp(stats) if stats else None, vp(tout) if tout else None, vp(cur) if cur else None, vp(tprev) if tprev else None, ww, hh, nn, p, None)

    assert call(cur=0) == -1 and call(p=None) == -1 and call(stats=0, tout=0) == -1
    assert call(tprev=0) == -1, 'statistics without previous thumbnails'
    for ww, hh, nn in BAD_SHAPES:
        assert call(ww=ww, hh=hh, nn=nn) == -1, (ww, hh, nn)
    for p in BAD_PARAMS:
        assert call(p=ctypes.byref(h264mi.Scenecut(*p))) == -1, p
    for off in (1, 2, 3):
        assert call(stats=St + off) == -1
    # every pair of ranges: one byte into the other's first byte, its last byte, and from below
    for off in (1, tb - 1, -1, -(tb - 1)):
        assert call(tout=Tp + off) == -1, off
    for off in (0, 1, fb - 1, -1, -(tb - 1)):
        assert call(tout=Cu + off) == -1 and call(tprev=Cu + off) == -1, off
    for off in (0, 4, fb - 4, -4, -(sb - 4)):
        assert call(stats=Cu + off) == -1, off
    for off in (0, 4, tb - 4, -4, -(sb - 4)):
        assert call(stats=To + off) == -1 and call(stats=Tp + off) == -1, off


# ---------------------------------------------------------------- usefulness: three clips and the documented default

CW, CH = 96, 80


@functools.lru_cache(maxsize=None)
def clip_texture(seed, tw=CW + 64, th=CH + 64):
    """synth.py's counter-based hash, box-filtered 8 x 8 (wrap-around) and stretched by 4 about mid-grey: features of
    about eight samples, a standard deviation of about 37 levels"""
    idx = np.arange(tw * th, dtype=np.uint64)
    x = (((idx * np.uint64(0x9E3779B1)) ^ np.uint64(seed)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    raw = (x >> np.uint32(24)).astype(np.int64).reshape(th, tw)
    acc = np.zeros_like(raw)
    for dy in range(8):
        for dx in range(8):
            acc += np.roll(np.roll(raw, -dy, axis=0), -dx, axis=1)
    out = np.clip(128 + (acc - 8160) * 4 // 64, 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


def clip_frame(seed, ox, oy, add=0, noise=None, w=CW, h=CH):
    """the w x h window at (ox, oy) of scene `seed`, every luma sample moved by add and by noise; flat chroma per scene"""
    y = clip_texture(seed)[oy:oy + h, ox:ox + w].astype(np.int64) + add
    if noise is not None:
        y = y + noise
    c = (w // 2) * (h // 2)
    return np.concatenate([np.clip(y, 0, 255).astype(np.uint8).ravel(), np.full(c, 100 + 9 * (seed % 5), np.uint8), np.full(c, 150 - 7 * (seed % 5), np.uint8)])


@functools.lru_cache(maxsize=None)
def pan_clip(n=16):
    """a pan of 2 x 1 samples a frame over one scene, sensor noise of +-3"""
    rng = np.random.default_rng(5)
    return tuple(clip_frame(1, 2 * t, t, 0, rng.integers(-3, 4, (CH, CW))) for t in range(n))


@functools.lru_cache(maxsize=None)
def fade_clip(n=14):
    """a still scene that brightens by 4 levels a frame, sensor noise of +-1"""
    rng = np.random.default_rng(6)
    return tuple(clip_frame(2, 5, 7, 4 * t - 28, rng.integers(-1, 2, (CH, CW))) for t in range(n))


SWITCHES = (5, 11, 12)


@functools.lru_cache(maxsize=None)
def switch_clip(n=18, switches=SWITCHES):
    """the slow pan with noise, the scene replaced at every index in `switches`"""
    rng = np.random.default_rng(7)
    out, scene = [], 1
    for t in range(n):
        scene += t in switches
        out.append(clip_frame(scene, t, t // 2, 0, rng.integers(-3, 4, (CH, CW))))
    return tuple(out)


def _cuts(frames, params):
    return [t for t, s in enumerate(ref.policy_states(list(frames), CW, CH, params)) if s[8]]


def test_the_documented_default_names_exactly_the_switches():
    src = open(__import__('os').path.join(__import__('test_capi_exports').ROOT, 'include', 'h264mi.h')).read()
    level, share, min_gap, max_gap, comp = ref.DEFAULT
    assert f'{{level {level}, share {share}, min_gap {min_gap}, max_gap {max_gap}, compensate {comp}}}' in src, 'the header documents the default'
    assert _cuts(pan_clip(), ref.DEFAULT) == []
    assert _cuts(fade_clip(), ref.DEFAULT) == []
    # min_gap 4 holds the switch at 12 back, one frame after the one at 11
    assert _cuts(switch_clip(), ref.DEFAULT) == [5, 11]
    assert _cuts(switch_clip(), (level, share, 0, 0, comp)) == list(SWITCHES)
    # the inputs are worth the name: the fade does move every block without the compensation at a level the pan
    # stays under, and a switch changes more than half of the blocks
    assert _cuts(fade_clip(), (12, share, 0, 0, 0)) == list(range(1, len(fade_clip())))
    assert _cuts(fade_clip(), (12, share, 0, 0, 1)) == []
    st = ref.policy_states(list(switch_clip()), CW, CH, ref.DEFAULT)
    assert all(2 * st[t][0] > st[t][1] for t in SWITCHES) and all(2 * st[t][0] <= st[t][1] for t in range(1, 18) if t not in SWITCHES)
