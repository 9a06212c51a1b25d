"""The reference for h264mi_i420_upscale_dev, h264mi_i420_compose_any_dev and h264mi_speaker_cells (include/h264mi.h),
written from the header text and not from the kernel: numpy int64, every bound of the definition asserted on every call.

Per axis, for a plane crop of p samples enlarged to q >= p, output index o reads
    N = (2 o + 1) p - q,  P = floor((16 N + q) / (2 q)),  i = P >> 4,  f = P & 15
and the taps i - 1, i, i + 1, i + 2, each clamped to 0 .. p - 1, under the weights of phase f (sum 8192). Horizontal
first, H = (h + 16) >> 5; then vertical, out = clamp((v + 2^20) >> 21, 0, 255).

Frames and canvases are (n, frame bytes) uint8 arrays of tight I420 frames; a cell is anything with composeref's ten
fields."""
import numpy as np

import composeref
import scaleref

BILINEAR, BICUBIC = 0, 1
I32 = 2 ** 31


def weights(f, filt):
    """the four weights (taps i - 1 .. i + 2) of phase f, f an int or an int64 array; shape (..., 4)"""
    f = np.asarray(f, np.int64)
    assert ((f >= 0) & (f <= 15)).all() and filt in (BILINEAR, BICUBIC)
    if filt == BICUBIC:
        w = [-f ** 3 + 32 * f ** 2 - 256 * f, 3 * f ** 3 - 80 * f ** 2 + 8192, -3 * f ** 3 + 64 * f ** 2 + 256 * f, f ** 3 - 16 * f ** 2]
    else:
        w = [0 * f, (16 - f) * 512, f * 512, 0 * f]
    w = np.stack(w, axis=-1)
    assert (w.sum(axis=-1) == 8192).all()
    assert (np.where(w > 0, w, 0).sum(axis=-1) <= 9216).all() and (np.where(w < 0, w, 0).sum(axis=-1) >= -1024).all()
    return w


def phases(p, q):
    """P of every output index 0 .. q - 1 (int64), by floor division"""
    assert 1 <= p <= q and p <= 4096 and q <= 8192
    o = np.arange(q, dtype=np.int64)
    num = 16 * ((2 * o + 1) * p - q) + q
    assert (np.abs(num) < I32).all()
    return num // (2 * q)  # numpy's // on integers is a floor division


def taps(p, q, filt):
    """(indices (q, 4) into the crop, clamped; weights (q, 4)) of one axis"""
    P = phases(p, q)
    i, f = P >> 4, P & 15
    idx = np.clip(i[:, None] + np.arange(-1, 3)[None, :], 0, p - 1)
    return idx, weights(f, filt)


def up_plane(crop, qw, qh, filt, clamp=True):
    """the crop (ph x pw, uint8) enlarged to qh x qw. With clamp=False the values before the final clamp (int64)."""
    crop = np.asarray(crop)
    assert crop.dtype == np.uint8 and crop.ndim == 2
    ph, pw = crop.shape
    xi, wx = taps(pw, qw, filt)
    yi, wy = taps(ph, qh, filt)
    c = crop.astype(np.int64)
    h = (c[:, xi] * wx[None, :, :]).sum(axis=2)  # (ph, qw)
    assert (np.abs(h) < 2 ** 22).all()
    H = (h + 16) >> 5
    assert H.min() >= -8160 and H.max() <= 73440
    v = (H[yi, :] * wy[:, :, None]).sum(axis=1)  # (qh, qw)
    assert (np.abs(v) <= 9216 * 73440 + 1024 * 8160).all() and 9216 * 73440 + 1024 * 8160 < I32
    out = (v + (1 << 20)) >> 21
    return np.clip(out, 0, 255).astype(np.uint8) if clamp else out


def up_frame(frame, sw, sh, dw, dh, filt):
    """one tight sw x sh I420 frame enlarged to a tight dw x dh frame, every plane on its own"""
    assert not (sw | sh | dw | dh) & 1 and 2 <= sw <= dw and 2 <= sh <= dh
    out = np.empty(scaleref.frame_bytes(dw, dh), np.uint8)
    for p, (s, d) in enumerate(zip(scaleref.planes(np.asarray(frame, np.uint8), sw, sh), scaleref.planes(out, dw, dh))):
        k = 1 if p else 0
        d[:] = up_plane(s, dw >> k, dh >> k, filt)
    return out


def kind(cell):
    """0 a shrinking cell (equal sizes included), 1 an enlarging cell, None a mixed one"""
    _, _, _, _, sw, sh, _, _, dw, dh = composeref.as_tuple(cell)
    if dw <= sw and dh <= sh:
        return 0
    if dw >= sw and dh >= sh:
        return 1
    return None


def compose_any(canvases, cw, ch, sources, src_w, src_h, cells, filt):
    """a copy of `canvases` with every shrinking cell as composeref.compose gives it and every enlarging cell's crop
    enlarged by up_plane into its rectangle, per plane; everything else keeps its value"""
    cells = list(cells)
    assert all(kind(c) is not None for c in cells)
    for i, a in enumerate(cells):
        for b in cells[:i]:
            assert not (a.canvas == b.canvas and a.dx < b.dx + b.dw and b.dx < a.dx + a.dw and a.dy < b.dy + b.dh and b.dy < a.dy + a.dh)
    out = composeref.compose(canvases, cw, ch, sources, src_w, src_h, [c for c in cells if kind(c) == 0])
    sources = np.asarray(sources, np.uint8).reshape(-1, scaleref.frame_bytes(src_w, src_h))
    for cell in cells:
        if kind(cell) != 1:
            continue
        src, canvas, sx, sy, sw, sh, dx, dy, dw, dh = composeref.as_tuple(cell)
        assert 0 <= src < len(sources) and 0 <= canvas < len(out)
        assert not (sx | sy | sw | sh | dx | dy | dw | dh) & 1
        assert 0 <= sx and sx + sw <= src_w and 0 <= sy and sy + sh <= src_h and sw >= 2 and sh >= 2
        assert 0 <= dx and dx + dw <= cw and 0 <= dy and dy + dh <= ch
        for p, (s, d) in enumerate(zip(scaleref.planes(sources[src], src_w, src_h), scaleref.planes(out[canvas], cw, ch))):
            k = 1 if p else 0  # chroma: the crop's and the rectangle's origin and size halved
            crop = s[sy >> k:(sy >> k) + (sh >> k), sx >> k:(sx >> k) + (sw >> k)]
            d[dy >> k:(dy >> k) + (dh >> k), dx >> k:(dx >> k) + (dw >> k)] = up_plane(crop, dw >> k, dh >> k, filt)
    return out


def speaker_cells(n, speaker, src_w, src_h, cw, ch):
    """the active-speaker layout: source `speaker` above a strip 2 * (ch // 8) high that holds the others in index
    order, each picture as large as its slot allows at the source's shape, centred. None where a cell comes out below 2."""
    assert n >= 1 and 0 <= speaker < n
    strip = 0 if n == 1 else 2 * (ch // 8)
    m, k, cells = n - 1, 0, []
    for s in range(n):
        if s == speaker:
            x0, x1, y0, y1 = 0, cw, 0, ch - strip
        else:
            x0, x1, y0, y1 = 2 * (k * cw // (2 * m)), 2 * ((k + 1) * cw // (2 * m)), ch - strip, ch
            k += 1
        dw = min(x1 - x0, 2 * ((y1 - y0) * src_w // (2 * src_h)))
        dh = min(y1 - y0, 2 * (dw * src_h // (2 * src_w)))
        if dw < 2 or dh < 2:
            return None
        cells.append(composeref.C(s, 0, 0, 0, src_w, src_h, x0 + 2 * ((x1 - x0 - dw) // 4), y0 + 2 * ((y1 - y0 - dh) // 4), dw, dh))
    return cells
