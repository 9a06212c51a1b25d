"""CPU: histograms, level tables and automatic levels exist at every layer -- declared in include/h264mi.h, exported by
the library, bound in Python --, the vectorised reference of the GPU tests (tests/levelsref.py) equals the rules written
as loops and the library's three host restatements, the identities of the rules hold exactly, h264mi_levels_ok refuses
one past every limit, and the content and parameter sets the GPU tests share reach every class of the rules (the class
audit: a class not reached is a failure)."""
import ctypes
import functools

import numpy as np
import pytest

import levelsref as ref
from test_capi_exports import declared_functions

NEW = ('h264mi_levels_ok', 'h264mi_i420_hist_dev', 'h264mi_i420_lut_dev', 'h264mi_levels_work_bytes', 'h264mi_i420_levels_dev',
       'h264mi_i420_hist_host', 'h264mi_i420_lut_host', 'h264mi_levels_lut_host', 'h264mi_enc_set_levels', 'h264mi_enc_levels',
       'h264mi_enc_levels_record')
N = 3
A, F = ref.AUTO, ref.FIXED
# (mode, clip_lo, clip_hi, in_lo, in_hi, out_lo, out_hi, max_gain, speed, sat)
PARAMS = [
    (A, 0, 0, 0, 0, 0, 255, 1024, 256, 64),         # no clip, full range, the largest gain, no memory
    (A, 0, 0, 0, 0, 16, 235, 64, 256, 64),          # gain 1: the limit is active on everything narrower than 219 levels
    (A, 2048, 2048, 0, 0, 16, 235, 256, 37, 64),    # the flat frame's 0 and 255 samples meet these thresholds exactly
    (A, 4096, 4096, 0, 0, 0, 255, 1024, 37, 0),     # the largest clip: the flat frame's ends coincide; chroma all 128
    (A, 655, 655, 3, 2, 16, 235, 128, 1, 255),      # 1 %; in_* ignored in AUTO; the slowest ends; the largest saturation
    (A, 0, 4096, 0, 0, 0, 255, 64, 255, 80),        # min_span 65280: lo_e < 0 on dark content, hi_e > 65280 on bright; speed 255 stalls
    (A, 4096, 0, 0, 0, 0, 1, 1024, 256, 64),        # R = 1: min_span 16
    (A, 100, 100, 0, 0, 235, 255, 96, 200, 32),
    (F, 0, 0, 16, 235, 0, 255, 64, 1, 64),          # limited to full range
    (F, 0, 0, 0, 255, 16, 235, 64, 1, 64),          # full to limited
    (F, 4096, 4096, 100, 101, 0, 255, 1024, 256, 255),  # a threshold
    (F, 0, 0, 16, 235, 16, 235, 64, 1, 0),          # luma the identity, chroma all 128: not inert
    (F, 0, 0, 0, 254, 1, 255, 64, 1, 100),
]
INERT = (F, 9, 9, 16, 235, 16, 235, 777, 5, 64)
# h264mi_levels_ok refuses: one past every limit, out_lo == out_hi, FIXED with in_lo >= in_hi
GOOD = (A, 100, 100, 10, 20, 16, 235, 256, 37, 64)
BAD_PARAMS = [(2,) + GOOD[1:], (-1,) + GOOD[1:]]
for _k, (_lo, _hi) in enumerate(((0, 4096), (0, 4096), (0, 255), (0, 255), (0, 255), (0, 255), (64, 1024), (1, 256), (0, 255)), 1):
    for _v in (_lo - 1, _hi + 1):
        BAD_PARAMS.append(GOOD[:_k] + (_v,) + GOOD[_k + 1:])
BAD_PARAMS += [(A, 0, 0, 0, 0, 100, 100, 256, 37, 64), (A, 0, 0, 0, 0, 101, 100, 256, 37, 64), (F, 0, 0, 50, 50, 16, 235, 256, 37, 64),
               (F, 0, 0, 51, 50, 16, 235, 256, 37, 64)]
BAD_SHAPES = [(0, 16, 3), (31, 16, 3), (32, 15, 3), (8194, 16, 3), (32, 8194, 3), (-32, 16, 3), (32, 16, 0), (32, 16, -1)]
# the streaming kernels lay a plane, one run of bytes, on the grid of 16-byte units of the address space; an item is
# 16384 bytes of that grid (csrc/levels.hip). 2x2: chroma 1 byte; 4x4; 16x16; 36x18: chroma rows of 18 bytes, planes that
# start and end between units; 130x66: no plane a multiple of 16 (and the same at an odd address); 8192x2 and 2x8192: the
# limit; 8x2050: luma 16400 bytes, one unit past an item; 16x4100: chroma 16400 bytes
SHAPES = [(2, 2), (4, 4), (16, 16), (36, 18), (130, 66), (8192, 2), (2, 8192), (8, 2050), (16, 4100)]
SMALL = [(2, 2), (4, 4), (16, 16), (36, 18)]
SEQ_LEVELS = (30, 150, 150, 150, 150, 60)  # the sequence's brightness: up, held, down
NF = len(SEQ_LEVELS)


@functools.lru_cache(maxsize=None)
def make_frames(w, h):
    """N frames of different content as an (N, frame bytes) array, shared and never written: 0 random samples; 1 dark
    and narrow, values 20..60 (a ramp with noise); 2 flat 77 in every plane but npix >> 5 luma samples of 0 at the start
    and one more than that of 255 at the end -- clip 2048 meets the first count exactly and exceeds the second by one --,
    and one 0 and one 255 in a chroma plane of at least three samples"""
    rng = np.random.default_rng(7919 * w + h)
    nb, npix = ref.frame_bytes(w, h), w * h
    fr = np.empty((N, nb), np.uint8)
    fr[0] = rng.integers(0, 256, nb, dtype=np.uint8)
    fr[1] = np.clip(25 + (np.arange(nb) * 7 // 5) % 31 + rng.integers(-5, 6, nb), 20, 60)
    fr[2] = 77
    z = npix >> 5
    fr[2, :z] = 0
    fr[2, npix - (z + 1):npix] = 255
    for s in ref.plane_slices(w, h)[1:]:
        if s.stop - s.start >= 3:
            fr[2, s.start] = 0
            fr[2, s.stop - 1] = 255
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def make_sequence(w, h, stream=0):
    """NF frames of one stream: a fixed texture spanning 40 levels plus the step's brightness; the measured ends move by
    exactly the brightness step, so a slow end approaches a held target until the floor stalls it"""
    rng = np.random.default_rng(31 * w + h + 1000 * stream)
    nb = ref.frame_bytes(w, h)
    tex = (np.arange(nb) * (3 + stream)) % 33 + rng.integers(0, 8, nb)
    seq = np.stack([np.clip(tex + lv + 5 * stream, 0, 255).astype(np.uint8) for lv in SEQ_LEVELS])
    seq.setflags(write=False)
    return seq


def P(params):
    import h264mi
    return h264mi.Levels(*params)


def test_header_declares_library_exports_python_binds(libpath):
    names = declared_functions()
    L = ctypes.CDLL(libpath)
    for n in NEW:
        assert n in names, n
        assert hasattr(L, n), n
    import h264mi
    B = h264mi.lib()
    assert [len(getattr(B, n).argtypes) for n in NEW] == [1, 6, 8, 1, 10, 4, 5, 7, 2, 2, 3]
    for f in ('levels_ok', 'i420_hist', 'i420_lut', 'i420_levels', 'levels_work_bytes'):
        assert callable(getattr(h264mi, f)), f
    for f in ('set_levels', 'levels', 'levels_record'):
        assert callable(getattr(h264mi.BatchEncoder, f)), f
    assert ctypes.sizeof(h264mi.Levels) == 40
    assert tuple(k for k, _ in h264mi.Levels._fields_) == ref.FIELDS
    assert (h264mi.LEVELS_AUTO, h264mi.LEVELS_FIXED) == (ref.AUTO, ref.FIXED) == (0, 1)
    assert h264mi.levels_work_bytes(1) == 768 * 4 + 768 and h264mi.levels_work_bytes(7) == 7 * 3840 and h264mi.levels_work_bytes(7) % 4 == 0


def _lib_hist(frame, w, h):
    import h264mi
    out = np.full(768, 0xFFFFFFFF, np.uint32)
    src = np.ascontiguousarray(frame)
    assert h264mi.lib().h264mi_i420_hist_host(out.ctypes.data, src.ctypes.data, w, h) == 0
    return out


def _lib_lut(frame, w, h, lut):
    import h264mi
    out = np.full(frame.size, 0x5A, np.uint8)
    src, lut = np.ascontiguousarray(frame), np.ascontiguousarray(lut, np.uint8)
    assert h264mi.lib().h264mi_i420_lut_host(out.ctypes.data, src.ctypes.data, w, h, lut.ctypes.data) == 0
    return out


def _lib_levels_lut(hist_y, w, h, params, state, want_record=True):
    import h264mi
    lut = np.full(768, 0x5A, np.uint8)
    hy = np.ascontiguousarray(hist_y, np.uint32)
    st = np.array(state, np.int32) if state is not None else None
    rec = np.full(8, -7, np.int32)
    r = h264mi.lib().h264mi_levels_lut_host(lut.ctypes.data, hy.ctypes.data, w, h, ctypes.byref(P(params)), st.ctypes.data if st is not None else None,
                                           rec.ctypes.data if want_record else None)
    assert r == 0
    return lut, (st.tolist() if st is not None else None), rec.tolist()


@pytest.mark.parametrize('w,h', SMALL + [(130, 66)], ids=[f'{w}x{h}' for w, h in SMALL + [(130, 66)]])
def test_reference_equals_the_loops_and_the_library(libpath, w, h):
    rng = np.random.default_rng(w + h)
    for k, f in enumerate(list(make_frames(w, h)) + list(make_sequence(w, h))):
        hist = ref.hist_frame(f, w, h)
        assert hist.dtype == np.uint32 and hist.size == 768 and int(hist.sum()) == f.size
        assert np.array_equal(hist, ref.hist_frame_loops(f, w, h)) and np.array_equal(hist, _lib_hist(f, w, h))
        lut = rng.integers(0, 256, 768, dtype=np.uint8)
        out = ref.lut_frame(f, w, h, lut)
        assert np.array_equal(out, ref.lut_frame_loops(f, w, h, lut)) and np.array_equal(out, _lib_lut(f, w, h, lut))
    for params in PARAMS:
        for frames in (make_frames(w, h), make_sequence(w, h)):
            state = None
            for t, f in enumerate(frames):
                hy = ref.hist_frame(f, w, h)[:256]
                first = frames is not make_sequence(w, h)  # the N frames are N streams: every one a first frame
                s_in = None if first else (state if state is not None else [0, -5, 99999, 3])  # has == 0: the other words are ignored
                lut, s_out, rec = ref.levels_lut(hy, w, h, params, s_in)
                lut_l, s_l, rec_l = ref.levels_lut_loops(hy, w, h, params, s_in)
                assert np.array_equal(lut, lut_l) and s_out == s_l and rec == rec_l, (params, t)
                lut_c, s_c, rec_c = _lib_levels_lut(hy, w, h, params, s_in)
                assert np.array_equal(lut, lut_c) and rec == rec_c, (params, t)
                if params[0] == A:
                    assert s_in is None or s_c == s_out, (params, t)
                else:
                    assert s_c == s_in and s_out == s_in, 'FIXED leaves the state alone'
                assert np.array_equal(_lib_levels_lut(hy, w, h, params, None, want_record=False)[0], ref.levels_lut(hy, w, h, params, None)[0])
                state = s_out
    import h264mi
    assert h264mi.lib().h264mi_levels_lut_host(np.zeros(768, np.uint8).ctypes.data, None, w, h, ctypes.byref(P(PARAMS[8])), None, None) == 0, 'FIXED reads no histogram'


def test_identities():
    v = np.arange(256)
    for w, h in SMALL + [(130, 66)]:
        for f in make_frames(w, h):
            hy = ref.hist_frame(f, w, h)[:256]
            for params in PARAMS + [INERT]:
                lut, state, rec = ref.levels_lut(hy, w, h, params, [1, 3000, 40000, 0])
                for pl in range(3):
                    assert (np.diff(lut[256 * pl:256 * pl + 256].astype(int)) >= 0).all(), 'a table never decreases'
                assert lut[:256].min() >= params[5] and lut[:256].max() <= params[6]
                if params[0] == A:
                    assert rec[0] <= rec[1], 'lo_m <= hi_m'
                    assert rec[5] - rec[4] >= max(16, (params[6] - params[5]) * 16384 // params[7]), 'the span is at least min_span'
                    if params[8] == 256:
                        assert state == [1, rec[0] << 8, rec[1] << 8, 0], 'speed 256: the state is the measured ends'
                    assert rec[6] + rec[7] <= w * h
                    assert ref.levels_lut(hy, w, h, params, None)[2][2:4] == [rec[0] << 8, rec[1] << 8], 'a first frame'
                if params[9] == 0:
                    assert (lut[256:] == 128).all(), 'sat 0: chroma all 128'
                if params[9] == 64:
                    assert np.array_equal(lut[256:512], v) and np.array_equal(lut[512:], v), 'sat 64 leaves chroma'
    # FIXED with in == out and sat 64: the identity table between the ends (outside them luma is clamped to the ends)
    lut = ref.levels_lut(None, 16, 16, INERT)[0]
    assert np.array_equal(lut[16:236], v[16:236]) and (lut[:16] == 16).all() and (lut[236:256] == 235).all() and np.array_equal(lut[256:], np.tile(v, 2))
    assert np.array_equal(ref.levels_lut(None, 16, 16, (F, 0, 0, 0, 255, 0, 255, 64, 1, 64))[0], np.tile(v, 3))
    assert ref.inert(INERT) and not any(ref.inert(p) for p in PARAMS)
    # AUTO with clip 0 on a frame spanning exactly out_lo..out_hi and a permissive max_gain: the identity on luma
    for out_lo, out_hi in ((16, 235), (0, 255), (100, 101)):
        f = np.full(ref.frame_bytes(16, 16), 128, np.uint8)
        f[:256] = np.linspace(out_lo, out_hi, 256).round()
        lut = ref.levels_lut(ref.hist_frame(f, 16, 16)[:256], 16, 16, (A, 0, 0, 0, 0, out_lo, out_hi, 1024, 256, 64))[0]
        assert np.array_equal(lut[out_lo:out_hi + 1], v[out_lo:out_hi + 1]) and np.array_equal(ref.lut_frame(f, 16, 16, lut), f)


def test_levels_ok_refuses_one_past_every_limit(libpath):
    import h264mi
    assert len(BAD_PARAMS) == 2 + 18 + 4
    assert h264mi.lib().h264mi_levels_ok(None) == -1 and h264mi.levels_ok(None) == -1
    for p in PARAMS + [INERT, GOOD]:
        assert ref.params_ok(p) and h264mi.levels_ok(p) == 0, p
    for k, (lo, hi) in enumerate(((0, 4096), (0, 4096), (0, 255), (0, 255), (0, 255), (0, 255), (64, 1024), (1, 256), (0, 255)), 1):
        for v in (lo, hi):
            p = list(GOOD)
            p[k] = v
            if k == 5:
                p[6] = 255
            if k == 6:
                p[5] = 0
            if p[5] < p[6]:
                assert h264mi.levels_ok(p) == 0 and ref.params_ok(p), p
    for p in BAD_PARAMS:
        assert not ref.params_ok(p) and h264mi.levels_ok(p) == -1, p
    assert h264mi.levels_ok((A, 0, 0, 50, 50, 16, 235, 256, 37, 64)) == 0, 'AUTO ignores the order of in_lo and in_hi'
    hy = np.zeros(256, np.uint32)
    lut = np.zeros(768, np.uint8)
    fn = h264mi.lib().h264mi_levels_lut_host
    assert fn(lut.ctypes.data, hy.ctypes.data, 16, 16, ctypes.byref(P(BAD_PARAMS[0])), None, None) == -1
    assert fn(None, hy.ctypes.data, 16, 16, ctypes.byref(P(GOOD)), None, None) == -1 and fn(lut.ctypes.data, None, 16, 16, ctypes.byref(P(GOOD)), None, None) == -1
    assert fn(lut.ctypes.data, hy.ctypes.data, 15, 16, ctypes.byref(P(GOOD)), None, None) == -1 and fn(lut.ctypes.data, hy.ctypes.data, 16, 16, None, None, None) == -1
    assert h264mi.lib().h264mi_i420_hist_host(None, lut.ctypes.data, 2, 2) == -1 and h264mi.lib().h264mi_i420_lut_host(lut.ctypes.data, lut.ctypes.data, 2, 3, lut.ctypes.data) == -1


CLASSES = ('lo_m at bin 0', 'hi_m at bin 255', 'lo_m interior', 'hi_m interior', 'k_lo == 0', 'k_lo > 0', 'cum == k at a bin', 'cum == k + 1 at the end',
           'lo_m == hi_m', 'gain limit active', 'gain limit inactive', 'lo_e < 0', 'hi_e > 65280', 'entry from t <= 0', 'entry clipped at out_hi',
           'entry interior', 'first frame', 'later frame', 'end moves up', 'end moves down', 'end stalled by the floor', 'chroma clipped at 0',
           'chroma clipped at 255', 'chroma unclipped')


def classes_of(hist_y, w, h, p, state):
    """the classes one decision reaches, from the rule's own intermediate values"""
    got = set()
    mode, clip_lo, clip_hi, _, _, out_lo, out_hi, max_gain, speed, sat = p
    lut, new, rec = ref.levels_lut(hist_y, w, h, p, state)
    lo_m, hi_m, lo_s, hi_s, lo_e, hi_e = rec[:6]
    if mode == A:
        H = np.asarray(hist_y, np.int64)
        npix = w * h
        k_lo, k_hi = (clip_lo * npix) >> 16, (clip_hi * npix) >> 16
        up, down = np.cumsum(H), np.cumsum(H[::-1])[::-1]
        got.add('lo_m at bin 0' if lo_m == 0 else 'lo_m interior')
        got.add('hi_m at bin 255' if hi_m == 255 else 'hi_m interior')
        got.add('k_lo == 0' if k_lo == 0 else 'k_lo > 0')
        if (k_lo > 0 and (up[H > 0] == k_lo).any()) or (k_hi > 0 and (down[H > 0] == k_hi).any()):
            got.add('cum == k at a bin')
        if (k_lo > 0 and up[lo_m] == k_lo + 1) or (k_hi > 0 and down[hi_m] == k_hi + 1):
            got.add('cum == k + 1 at the end')
        if lo_m == hi_m:
            got.add('lo_m == hi_m')
        got.add('gain limit active' if (lo_e, hi_e) != (lo_s, hi_s) else 'gain limit inactive')
        if lo_e < 0:
            got.add('lo_e < 0')
        if hi_e > 65280:
            got.add('hi_e > 65280')
        if state is None or not state[0]:
            got.add('first frame')
        else:
            got.add('later frame')
            for m, s0, s1 in ((lo_m, state[1], lo_s), (hi_m, state[2], hi_s)):
                d = (m << 8) - s0
                if s1 > s0:
                    got.add('end moves up')
                if s1 < s0:
                    got.add('end moves down')
                    assert d < 0
                if d > 0 and s1 == s0:
                    got.add('end stalled by the floor')
                assert not (d < 0 and s1 == s0), 'a downward difference always moves'
    t = (np.arange(256) << 8) - lo_e
    span, R = hi_e - lo_e, out_hi - out_lo
    raw = out_lo + (np.maximum(t, 0) * R + span // 2) // span
    if (t <= 0).any():
        got.add('entry from t <= 0')
    if ((t > 0) & (raw > out_hi)).any():
        got.add('entry clipped at out_hi')
    if ((t > 0) & (raw <= out_hi)).any():
        got.add('entry interior')
    c = 128 + (((np.arange(256) - 128) * sat + 32) >> 6)
    got |= {n for n, hit in (('chroma clipped at 0', (c < 0).any()), ('chroma clipped at 255', (c > 255).any()), ('chroma unclipped', ((c >= 0) & (c <= 255)).any())) if hit}
    return got, new


def test_class_audit():
    """every class of the rules is reached by the shared shapes, frames, sequence and parameter sets"""
    assert len(PARAMS) >= 12
    assert {p[5:7] for p in PARAMS} >= {(0, 255), (16, 235)} and {p[7] for p in PARAMS} >= {64, 1024}
    assert {p[8] for p in PARAMS} >= {1, 37, 256} and {p[9] for p in PARAMS} >= {0, 64, 255}
    reached = set()
    for w, h in SMALL + [(130, 66), (64, 48)]:
        for params in PARAMS:
            for f in make_frames(w, h):
                reached |= classes_of(ref.hist_frame(f, w, h)[:256], w, h, params, None)[0]
            state = None
            for f in make_sequence(w, h):
                got, state = classes_of(ref.hist_frame(f, w, h)[:256], w, h, params, state)
                reached |= got
    missing = [c for c in CLASSES if c not in reached]
    assert not missing, f'classes not reached: {missing}'
    assert reached <= set(CLASSES)
