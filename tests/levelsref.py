"""Histograms, level tables and automatic levels of tight I420 frames as include/h264mi.h defines them (DESIGN.md
§5.19), restated in numpy -- what the GPU tests compare the device with -- and, beside each, as plain Python loops over
Python integers, which the host test compares with the vectorised form and with the library's own host restatements.

A parameter set is the ten integers of h264mi_levels: (mode, clip_lo, clip_hi, in_lo, in_hi, out_lo, out_hi, max_gain,
speed, sat). A state is None (a first frame) or [has, lo_s, hi_s, 0]; a record is [lo_m, hi_m, lo_s, hi_s, lo_e, hi_e,
below, above]. Python's >> and // on integers are floor operations, as the rule's arithmetic shifts are."""
import numpy as np

AUTO, FIXED = 0, 1
FIELDS = ('mode', 'clip_lo', 'clip_hi', 'in_lo', 'in_hi', 'out_lo', 'out_hi', 'max_gain', 'speed', 'sat')


def frame_bytes(w, h):
    return w * h + 2 * (w // 2) * (h // 2)


def plane_slices(w, h):
    y, c = w * h, (w // 2) * (h // 2)
    return (slice(0, y), slice(y, y + c), slice(y + c, y + 2 * c))


def params_ok(p):
    if p is None or len(p) != 10:
        return False
    mode, clip_lo, clip_hi, in_lo, in_hi, out_lo, out_hi, max_gain, speed, sat = p
    return (mode in (AUTO, FIXED) and 0 <= clip_lo <= 4096 and 0 <= clip_hi <= 4096 and all(0 <= v <= 255 for v in (in_lo, in_hi, out_lo, out_hi, sat))
            and out_lo < out_hi and (mode == AUTO or in_lo < in_hi) and 64 <= max_gain <= 1024 and 1 <= speed <= 256)


def inert(p):
    mode, _, _, in_lo, in_hi, out_lo, out_hi, _, _, sat = p
    return mode == FIXED and in_lo == out_lo and in_hi == out_hi and sat == 64


# ---- histogram
def hist_frame(frame, w, h):
    """768 uint32: 256 counts of Y, of Cb, of Cr"""
    return np.concatenate([np.bincount(frame[s], minlength=256) for s in plane_slices(w, h)]).astype(np.uint32)


def hist_frame_loops(frame, w, h):
    out = [0] * 768
    for pl, s in enumerate(plane_slices(w, h)):
        for v in frame[s].tolist():
            out[256 * pl + v] += 1
    return np.array(out, np.uint32)


# ---- LUT
def lut_frame(frame, w, h, lut768):
    lut768 = np.asarray(lut768, np.uint8)
    return np.concatenate([lut768[256 * pl:256 * pl + 256][frame[s]] for pl, s in enumerate(plane_slices(w, h))])


def lut_frame_loops(frame, w, h, lut768):
    out = np.empty_like(frame)
    for pl, s in enumerate(plane_slices(w, h)):
        for i in range(s.start, s.stop):
            out[i] = lut768[256 * pl + int(frame[i])]
    return out


# ---- the decision
def measured_ends(hist_y, w, h, clip_lo, clip_hi):
    npix = w * h
    k_lo, k_hi = (clip_lo * npix) >> 16, (clip_hi * npix) >> 16
    H = np.asarray(hist_y, np.int64)
    up, down = np.cumsum(H), np.cumsum(H[::-1])[::-1]
    return int(np.flatnonzero(up > k_lo)[0]), int(np.flatnonzero(down > k_hi)[-1])


def measured_ends_loops(hist_y, w, h, clip_lo, clip_hi):
    npix = w * h
    k_lo, k_hi = (clip_lo * npix) >> 16, (clip_hi * npix) >> 16
    H = [int(v) for v in hist_y]
    lo_m = next(v for v in range(256) if sum(H[:v + 1]) > k_lo)
    hi_m = next(v for v in range(255, -1, -1) if sum(H[v:]) > k_hi)
    return lo_m, hi_m


def _ends(hist_y, w, h, p, state, ends):
    """(lo_m, hi_m, lo_s, hi_s, lo_e, hi_e, new state)"""
    mode, clip_lo, clip_hi, in_lo, in_hi, out_lo, out_hi, max_gain, speed, sat = p
    if mode == FIXED:
        return 0, 0, 0, 0, in_lo << 8, in_hi << 8, state
    lo_m, hi_m = ends(hist_y, w, h, clip_lo, clip_hi)
    if state is None or not state[0]:
        lo_s, hi_s = lo_m << 8, hi_m << 8
    else:
        lo_s = state[1] + ((((lo_m << 8) - state[1]) * speed) >> 8)
        hi_s = state[2] + ((((hi_m << 8) - state[2]) * speed) >> 8)
    R = out_hi - out_lo
    min_span = max(16, (R * 64 * 256) // max_gain)
    if hi_s - lo_s < min_span:
        lo_e = (lo_s + hi_s - min_span) >> 1
        hi_e = lo_e + min_span
    else:
        lo_e, hi_e = lo_s, hi_s
    return lo_m, hi_m, lo_s, hi_s, lo_e, hi_e, [1, lo_s, hi_s, 0]


def levels_lut(hist_y, w, h, p, state=None):
    """(lut768, state, record) of one frame whose luma histogram is hist_y (ignored in FIXED mode)"""
    assert params_ok(p), p
    mode, _, _, _, _, out_lo, out_hi, _, _, sat = p
    lo_m, hi_m, lo_s, hi_s, lo_e, hi_e, state = _ends(hist_y, w, h, p, state, measured_ends)
    v = np.arange(256, dtype=np.int64)
    t, span, R = (v << 8) - lo_e, hi_e - lo_e, out_hi - out_lo
    y = np.where(t <= 0, out_lo, np.minimum(out_hi, out_lo + (np.maximum(t, 0) * R + span // 2) // span))
    c = np.clip(128 + (((v - 128) * sat + 32) >> 6), 0, 255)
    below = above = 0
    if mode == AUTO:
        H = np.asarray(hist_y, np.int64)
        below, above = int(H[(v << 8) < lo_e].sum()), int(H[(v << 8) > hi_e].sum())
    return np.concatenate([y, c, c]).astype(np.uint8), state, [lo_m, hi_m, lo_s, hi_s, lo_e, hi_e, below, above]


def levels_lut_loops(hist_y, w, h, p, state=None):
    mode, _, _, _, _, out_lo, out_hi, _, _, sat = p
    lo_m, hi_m, lo_s, hi_s, lo_e, hi_e, state = _ends(hist_y, w, h, p, state, measured_ends_loops)
    R, span = out_hi - out_lo, hi_e - lo_e
    lut = [0] * 768
    below = above = 0
    for v in range(256):
        t = (v << 8) - lo_e
        lut[v] = out_lo if t <= 0 else min(out_hi, out_lo + (t * R + span // 2) // span)
        lut[256 + v] = lut[512 + v] = min(255, max(0, 128 + (((v - 128) * sat + 32) >> 6)))
        if mode == AUTO:
            below += int(hist_y[v]) if (v << 8) < lo_e else 0
            above += int(hist_y[v]) if (v << 8) > hi_e else 0
    return np.array(lut, np.uint8), state, [lo_m, hi_m, lo_s, hi_s, lo_e, hi_e, below, above]


def levels_frame(frame, w, h, p, state=None):
    """(out frame, state, record) of one frame of one stream"""
    lut, state, rec = levels_lut(hist_frame(frame, w, h)[:256], w, h, p, state)
    return lut_frame(frame, w, h, lut), state, rec


def levels_frames(frames, w, h, p, state=None):
    """a sequence of one stream's frames: (list of out frames, final state, list of records, list of states after each)"""
    out, recs, states = [], [], []
    for f in frames:
        o, state, rec = levels_frame(f, w, h, p, state)
        out.append(o)
        recs.append(rec)
        states.append(list(state) if state is not None else None)
    return out, state, recs, states
