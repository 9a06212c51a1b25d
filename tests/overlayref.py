"""The reference for h264mi_i420_overlay_dev and h264mi_rgba_to_i420a_dev (include/h264mi.h), written from the header
text and not from the kernel: plain non-negative integers in numpy, the placements applied one after another in list
order on a copy of the canvases.

    a   = (A * opacity + 128) >> 8                 the effective alpha of a luma position, 0..255
    out = (d * (255 - a) + s * a + 127) // 255     d the canvas sample, s the sprite's
    chroma: a = (a00 + a01 + a10 + a11 + 2) >> 2   over the effective alphas of the four luma positions it covers

A placement is anything with the ten fields sprite, canvas, sx, sy, w, h, dx, dy, opacity, reserved (h264mi.Overlay, or
O below); canvases are (n, frame bytes) uint8 arrays of tight I420 frames, sprites (n, sprite bytes) arrays of tight
I420A sprites (Y, Cb, Cr, then a full-resolution A plane)."""
import collections

import numpy as np

import scaleref

FIELDS = ('sprite', 'canvas', 'sx', 'sy', 'w', 'h', 'dx', 'dy', 'opacity', 'reserved')
O = collections.namedtuple('O', FIELDS, defaults=(256, 0))


def as_tuple(ov):
    return tuple(int(getattr(ov, k)) for k in FIELDS)


def sprite_bytes(w, h):
    return 2 * w * h + 2 * (w // 2) * (h // 2)


def sprite_planes(sprite, w, h):
    """the Y, Cb, Cr and A planes of a tight I420A sprite"""
    f = np.asarray(sprite, np.uint8).ravel()
    y, u, v = scaleref.planes(f[:scaleref.frame_bytes(w, h)], w, h)
    a = f[scaleref.frame_bytes(w, h):sprite_bytes(w, h)].reshape(h, w)
    return y, u, v, a


def make_sprite(y, u, v, a):
    """a tight I420A sprite from its four planes"""
    return np.concatenate([np.asarray(p, np.uint8).ravel() for p in (y, u, v, a)])


def div255(x):
    """(x + 127) // 255"""
    return (np.asarray(x, np.int64) + 127) // 255


def effective_alpha(A, opacity):
    return (np.asarray(A, np.int64) * opacity + 128) >> 8


def blend_samples(d, s, a):
    d, s, a = (np.asarray(x, np.int64) for x in (d, s, a))
    return div255(d * (255 - a) + s * a)


def chroma_alpha(a):
    """the (h/2, w/2) chroma alphas of an (h, w) array of effective luma alphas"""
    a = np.asarray(a, np.int64)
    return (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2


def blend(canvases, cw, ch, sprites, ow, oh, overlays):
    """a copy of `canvases` (ncanvas tight cw x ch frames) with every placement blended onto it, one after another in
    list order; everything outside the rectangles keeps its value"""
    out = np.array(canvases, dtype=np.uint8, copy=True).reshape(-1, scaleref.frame_bytes(cw, ch))
    sprites = np.asarray(sprites, np.uint8).reshape(-1, sprite_bytes(ow, oh))
    for ov in overlays:
        sprite, canvas, sx, sy, w, h, dx, dy, opacity, reserved = as_tuple(ov)
        assert 0 <= sprite < len(sprites) and 0 <= canvas < len(out) and reserved == 0 and 0 <= opacity <= 256
        assert not (sx | sy | w | h | dx | dy) & 1 and w >= 2 and h >= 2
        assert 0 <= sx and sx + w <= ow and 0 <= sy and sy + h <= oh
        assert 0 <= dx and dx + w <= cw and 0 <= dy and dy + h <= ch
        y, u, v, A = sprite_planes(sprites[sprite], ow, oh)
        dy_, du, dv = scaleref.planes(out[canvas], cw, ch)  # views of `out`
        a = effective_alpha(A[sy:sy + h, sx:sx + w], opacity)
        assert 0 <= int(a.min()) and int(a.max()) <= 255
        rect = dy_[dy:dy + h, dx:dx + w]
        rect[...] = blend_samples(rect, y[sy:sy + h, sx:sx + w], a).astype(np.uint8)
        ac = chroma_alpha(a)
        for s, d in ((u, du), (v, dv)):
            rect = d[dy // 2:(dy + h) // 2, dx // 2:(dx + w) // 2]
            rect[...] = blend_samples(rect, s[sy // 2:(sy + h) // 2, sx // 2:(sx + w) // 2], ac).astype(np.uint8)
    return out


def rgba_to_i420a(rgba, w, h):
    """a tight w x h RGBA8 frame to a tight I420A sprite: BT.601 limited range as the wrapper's rgba_to_yuv has it (u8
    wrap, chroma from the top-left pixel of each 2x2, alpha ignored), A the fourth byte"""
    p = np.asarray(rgba, np.uint8).reshape(h, w, 4).astype(np.int32)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (((66 * r + 129 * g + 25 * b + 128) >> 8) + 16) & 255
    r, g, b = r[0::2, 0::2], g[0::2, 0::2], b[0::2, 0::2]
    u = (((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128) & 255
    v = (((112 * r - 94 * g - 18 * b + 128) >> 8) + 128) & 255
    return make_sprite(y, u, v, p[..., 3])
