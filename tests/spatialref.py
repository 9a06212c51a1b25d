"""The spatial filter and the privacy masks of include/h264mi.h restated in numpy: the reference of the
GPU tests. Exact integers, so every comparison with the device is equality of bytes.

A frame is a flat uint8 array of a tight w x h I420 picture; params is (radius_y, radius_c, amount_y, amount_c, core); a
mask is (frame, x, y, w, h, mode, block, fill_y, fill_cb, fill_cr).
  lowpass(plane, r)                        -> L, separable (rows, then columns), int64
  lowpass_direct(plane, r)                 -> L from the direct 2-D sum
  spatial_frame(frame, w, h, params)       -> out, vectorised
  spatial_frame_loops(frame, w, h, params) -> the same, as plain loops straight from the definition
  privacy_frames(frames, w, h, masks)      -> a copy of the (n, frame bytes) array with the masks applied, vectorised
  privacy_frames_loops(...)                -> the same, as plain loops
  spatial_classes / privacy_classes        -> how often the content reaches each class of the rules (the class audit)"""
import numpy as np

WEIGHTS = {1: (1, 2, 1), 2: (1, 4, 6, 4, 1), 3: (1, 6, 15, 20, 15, 6, 1)}
PIXELATE, FILL = 0, 1
BLOCKS = (4, 8, 16, 32, 64)
MAX_LIST = 4096


def frame_bytes(w, h):
    return w * h + 2 * (w // 2) * (h // 2)


def params_ok(params):
    ry, rc, ay, ac, core = params
    return 0 <= ry <= 3 and 0 <= rc <= 3 and -64 <= ay <= 255 and -64 <= ac <= 255 and 0 <= core <= 255


def inert(params):
    ry, rc, ay, ac, _ = params
    return (ry == 0 or ay == 0) and (rc == 0 or ac == 0)


def planes(frame, w, h):
    """views of Y (h x w), Cb, Cr (h/2 x w/2)"""
    y, c = w * h, (w // 2) * (h // 2)
    return frame[:y].reshape(h, w), frame[y:y + c].reshape(h // 2, w // 2), frame[y + c:y + 2 * c].reshape(h // 2, w // 2)


def _pad(plane, r):
    return np.pad(plane.astype(np.int64), r, mode='edge')


def lowpass(plane, r):
    """the separable form: the un-rounded horizontal sums (at most 255 * 64), then the vertical sum, rounded once"""
    ph, pw = plane.shape
    wt = WEIGHTS[r]
    p = _pad(plane, r)
    hs = sum(wt[i] * p[:, i:i + pw] for i in range(2 * r + 1))
    assert int(hs.max()) <= 255 * 64
    s = sum(wt[j] * hs[j:j + ph, :] for j in range(2 * r + 1))
    assert int(s.max()) <= 255 * 4096
    return (s + (1 << (4 * r - 1))) >> (4 * r)


def lowpass_direct(plane, r):
    ph, pw = plane.shape
    wt = WEIGHTS[r]
    p = _pad(plane, r)
    s = np.zeros((ph, pw), np.int64)
    for j in range(2 * r + 1):
        for i in range(2 * r + 1):
            s += wt[j] * wt[i] * p[j:j + ph, i:i + pw]
    return (s + (1 << (4 * r - 1))) >> (4 * r)


def sample(c, l, amount, core):
    """the sample rule for one sample, plain integers"""
    d = c - l
    if amount > 0 and abs(d) <= core:
        return c
    return min(255, max(0, c + ((amount * d + 32) >> 6)))


def _filter_plane(plane, r, amount, core):
    if r == 0:
        return plane.copy()
    c = plane.astype(np.int64)
    d = c - lowpass(plane, r)
    o = np.clip(c + ((amount * d + 32) >> 6), 0, 255)
    if amount > 0:
        o = np.where(np.abs(d) <= core, c, o)
    return o.astype(np.uint8)


def spatial_frame(frame, w, h, params):
    assert params_ok(params) and w % 2 == 0 and h % 2 == 0 and frame.size == frame_bytes(w, h)
    ry, rc, ay, ac, core = params
    Y, U, V = planes(frame, w, h)
    return np.concatenate([_filter_plane(Y, ry, ay, core).ravel(), _filter_plane(U, rc, ac, core).ravel(), _filter_plane(V, rc, ac, core).ravel()])


def spatial_frame_loops(frame, w, h, params):
    assert params_ok(params) and w % 2 == 0 and h % 2 == 0 and frame.size == frame_bytes(w, h)
    ry, rc, ay, ac, core = params
    out = np.empty_like(frame)
    S, O = planes(frame, w, h), planes(out, w, h)
    for pl in range(3):
        r, amount = (ry, ay) if pl == 0 else (rc, ac)
        ph, pw = S[pl].shape
        for y in range(ph):
            for x in range(pw):
                c = int(S[pl][y][x])
                if r == 0:
                    O[pl][y][x] = c
                    continue
                wt = WEIGHTS[r]
                s = 0
                for j in range(-r, r + 1):
                    for i in range(-r, r + 1):
                        s += wt[j + r] * wt[i + r] * int(S[pl][min(max(y + j, 0), ph - 1)][min(max(x + i, 0), pw - 1)])
                O[pl][y][x] = sample(c, (s + (1 << (4 * r - 1))) >> (4 * r), amount, core)
    return out


def spatial_classes(frame, w, h, params):
    """counts of the samples of `frame` that reach each class of the filter under params"""
    ry, rc, ay, ac, core = params
    n = dict.fromkeys(('keep', 'filtered', 'clip0', 'clip255', 'negative'), 0)
    for pl, plane in enumerate(planes(frame, w, h)):
        r, amount = (ry, ay) if pl == 0 else (rc, ac)
        if r == 0:
            continue
        c = plane.astype(np.int64)
        d = c - lowpass(plane, r)
        keep = (np.abs(d) <= core) if amount > 0 else np.zeros_like(d, bool)
        raw = c + ((amount * d + 32) >> 6)
        n['keep'] += int(keep.sum())
        n['filtered'] += int((~keep & (raw != c)).sum())
        n['clip0'] += int((~keep & (raw < 0)).sum())
        n['clip255'] += int((~keep & (raw > 255)).sum())
        n['negative'] += int((~keep).sum()) if amount < 0 else 0
    return n


# ---------------------------------------------------------------- privacy masks

def mask_ok(m, w, h, nframes):
    f, x, y, mw, mh, mode, block, fy, fcb, fcr = m
    if not 0 <= f < nframes or (x | y | mw | mh) & 1:
        return False
    if x < 0 or y < 0 or mw < 2 or mh < 2 or x + mw > w or y + mh > h:
        return False
    if mode == PIXELATE:
        return block in BLOCKS
    if mode == FILL:
        return all(0 <= v <= 255 for v in (fy, fcb, fcr))
    return False


def masks_ok(masks, w, h, nframes):
    if not 1 <= len(masks) <= MAX_LIST or nframes < 1 or w % 2 or h % 2 or not (2 <= w <= 8192 and 2 <= h <= 8192):
        return False
    if not all(mask_ok(m, w, h, nframes) for m in masks):
        return False
    for k, a in enumerate(masks):
        for b in masks[:k]:
            if a[0] == b[0] and a[1] < b[1] + b[3] and b[1] < a[1] + a[3] and a[2] < b[2] + b[4] and b[2] < a[2] + a[4]:
                return False
    return True


def _pixelate(rect, B):
    """rect: a 2-D uint8 view, changed in place: B x B cells anchored at its corner, partial at the right and bottom"""
    rh, rw = rect.shape
    ny, nx = -(-rh // B), -(-rw // B)
    pad = np.zeros((ny * B, nx * B), np.int64)
    pad[:rh, :rw] = rect
    s = pad.reshape(ny, B, nx, B).sum(axis=(1, 3))
    n = np.minimum(B, rh - B * np.arange(ny))[:, None] * np.minimum(B, rw - B * np.arange(nx))[None, :]
    v = (s + n // 2) // n
    rect[:, :] = np.repeat(np.repeat(v, B, axis=0), B, axis=1)[:rh, :rw]


def privacy_frames(frames, w, h, masks):
    frames = np.array(frames, dtype=np.uint8, copy=True)
    assert masks_ok(list(masks), w, h, frames.shape[0]) and frames.shape[1] == frame_bytes(w, h)
    for f, x, y, mw, mh, mode, block, fy, fcb, fcr in masks:
        for pl, plane in enumerate(planes(frames[f], w, h)):
            s = 1 if pl else 0
            rect = plane[y >> s:(y + mh) >> s, x >> s:(x + mw) >> s]
            if mode == FILL:
                rect[:, :] = (fy, fcb, fcr)[pl]
            else:
                _pixelate(rect, block >> s)
    return frames


def privacy_frames_loops(frames, w, h, masks):
    frames = np.array(frames, dtype=np.uint8, copy=True)
    assert masks_ok(list(masks), w, h, frames.shape[0])
    for f, x, y, mw, mh, mode, block, fy, fcb, fcr in masks:
        P = planes(frames[f], w, h)
        for pl in range(3):
            s = 1 if pl else 0
            rx, ry, rw, rh = x >> s, y >> s, mw >> s, mh >> s
            if mode == FILL:
                for yy in range(rh):
                    for xx in range(rw):
                        P[pl][ry + yy][rx + xx] = (fy, fcb, fcr)[pl]
                continue
            B = block >> s
            for cy in range(0, rh, B):
                for cx in range(0, rw, B):
                    ch, cw = min(B, rh - cy), min(B, rw - cx)
                    tot = 0
                    for yy in range(ch):
                        for xx in range(cw):
                            tot += int(P[pl][ry + cy + yy][rx + cx + xx])
                    n = cw * ch
                    v = (tot + n // 2) // n
                    for yy in range(ch):
                        for xx in range(cw):
                            P[pl][ry + cy + yy][rx + cx + xx] = v
    return frames


def privacy_classes(masks):
    """counts over the luma cells of the PIXELATE masks: whole cells, cells partial to the right only, at the bottom only,
    both ways, and rectangles of exactly one whole cell"""
    n = dict.fromkeys(('whole', 'right', 'bottom', 'both', 'one_cell', 'fill'), 0)
    for _, _, _, mw, mh, mode, block, *_ in masks:
        if mode == FILL:
            n['fill'] += 1
            continue
        n['one_cell'] += int(mw == block and mh == block)
        for cy in range(0, mh, block):
            for cx in range(0, mw, block):
                pr, pb = mw - cx < block, mh - cy < block
                n['both' if pr and pb else 'right' if pr else 'bottom' if pb else 'whole'] += 1
    return n
