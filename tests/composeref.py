"""The reference for h264mi_i420_compose_dev, h264mi_i420_fill_dev and h264mi_mosaic_cells (include/h264mi.h), written
from the header text and not from the kernel. Composition is defined on top of the area average of scaleref.py: the
canvases are copied, and for every cell and every plane scaleref.scale_plane(crop, qw, qh) is pasted into the cell's
rectangle of the canvas plane. The gallery layout is restated in plain Python integers.

A cell is anything with the ten fields src, canvas, sx, sy, sw, sh, dx, dy, dw, dh (h264mi.Cell, or C below); frames
and canvases are (n, frame bytes) uint8 arrays of tight I420 frames."""
import collections

import numpy as np

import scaleref

FIELDS = ('src', 'canvas', 'sx', 'sy', 'sw', 'sh', 'dx', 'dy', 'dw', 'dh')
C = collections.namedtuple('C', FIELDS)


def as_tuple(cell):
    return tuple(int(getattr(cell, k)) for k in FIELDS)


def compose(canvases, cw, ch, sources, src_w, src_h, cells):
    """a copy of `canvases` (ncanvas tight cw x ch frames) with every cell's crop of its source frame (of `sources`,
    nsrc tight src_w x src_h frames) area-averaged into its rectangle; everything else keeps its value"""
    out = np.array(canvases, dtype=np.uint8, copy=True).reshape(-1, scaleref.frame_bytes(cw, ch))
    sources = np.asarray(sources, np.uint8).reshape(-1, scaleref.frame_bytes(src_w, src_h))
    for cell in cells:
        src, canvas, sx, sy, sw, sh, dx, dy, dw, dh = as_tuple(cell)
        assert 0 <= src < len(sources) and 0 <= canvas < len(out)
        assert not (sx | sy | sw | sh | dx | dy | dw | dh) & 1
        assert 0 <= sx and sx + sw <= src_w and 0 <= sy and sy + sh <= src_h
        assert 0 <= dx and dx + dw <= cw and 0 <= dy and dy + dh <= ch and 2 <= dw <= sw and 2 <= dh <= sh
        for p, (s, d) in enumerate(zip(scaleref.planes(sources[src], src_w, src_h), scaleref.planes(out[canvas], cw, ch))):
            k = 1 if p else 0  # chroma: the crop's and the rectangle's origin and size halved
            crop = s[sy >> k:(sy >> k) + (sh >> k), sx >> k:(sx >> k) + (sw >> k)]
            d[dy >> k:(dy >> k) + (dh >> k), dx >> k:(dx >> k) + (dw >> k)] = scaleref.scale_plane(crop, dw >> k, dh >> k)
    return out


def fill(w, h, n, y, cb, cr):
    """n tight w x h frames of the colour (y, cb, cr)"""
    c = (w // 2) * (h // 2)
    return np.tile(np.concatenate([np.full(w * h, y, np.uint8), np.full(c, cb, np.uint8), np.full(c, cr, np.uint8)]), (n, 1))


def mosaic_cells(n, src_w, src_h, cw, ch):
    """the gallery layout: n whole sources on canvas 0, the smallest square grid of slots that holds them, each picture
    as large as its slot allows at the source's shape, never enlarged, centred. None where a cell comes out below 2."""
    cols = 1
    while cols * cols < n:
        cols += 1
    rows = (n + cols - 1) // cols
    cells = []
    for k in range(n):
        col, row = k % cols, k // cols
        x0, x1 = 2 * (col * cw // (2 * cols)), 2 * ((col + 1) * cw // (2 * cols))
        y0, y1 = 2 * (row * ch // (2 * rows)), 2 * ((row + 1) * ch // (2 * rows))
        dw = min(src_w, x1 - x0, 2 * ((y1 - y0) * src_w // (2 * src_h)))
        dh = min(src_h, y1 - y0, 2 * (dw * src_h // (2 * src_w)))
        if dw < 2 or dh < 2:
            return None
        cells.append(C(k, 0, 0, 0, src_w, src_h, x0 + 2 * ((x1 - x0 - dw) // 4), y0 + 2 * ((y1 - y0 - dh) // 4), dw, dh))
    return cells
