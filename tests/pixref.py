"""Reference of the pixel formats and pitched layouts (TEST INFRASTRUCTURE): a numpy restatement of the definition in
include/h264mi.h (h264mi_pix_layout), written from that text alone. A layout is a plain object with pix, pitch[3],
offset[3] and frame_stride (h264mi.PixLayout has the same attributes, and either kind is accepted everywhere here).
A frame on the I420 side is the tight w*h*3/2 byte array every other reference here uses."""
import numpy as np

I420, NV12, NV21, YUY2, UYVY = range(5)
ALL = (I420, NV12, NV21, YUY2, UYVY)
NAMES = ('I420', 'NV12', 'NV21', 'YUY2', 'UYVY')
MAX_SIDE, MAX_PITCH = 8192, 65536
INT64_MAX = (1 << 63) - 1


class Layout:
    def __init__(self, pix, pitch, offset, frame_stride):
        self.pix = pix
        self.pitch = list(pitch) + [0] * (3 - len(pitch))
        self.offset = list(offset) + [0] * (3 - len(offset))
        self.frame_stride = frame_stride

    def __repr__(self):
        return f'Layout({NAMES[self.pix] if 0 <= self.pix < 5 else self.pix}, pitch={self.pitch}, offset={self.offset}, fs={self.frame_stride})'


def frame_bytes(w, h):
    return w * h + 2 * (w // 2) * (h // 2)


def planes(pix, w, h):
    """[(row bytes, rows)] of the format's planes; None for an unknown format"""
    if pix == I420:
        return [(w, h), (w // 2, h // 2), (w // 2, h // 2)]
    if pix in (NV12, NV21):
        return [(w, h), (w, h // 2)]
    if pix in (YUY2, UYVY):
        return [(2 * w, h)]
    return None


def tight(pix, w, h):
    pl = planes(pix, w, h)
    offset, at = [], 0
    for rb, rows in pl:
        offset.append(at)
        at += rb * rows
    return Layout(pix, [rb for rb, _ in pl], offset, at)


def span(L, w, h):
    """the bytes from a frame's base to one past the last byte the layout names; -1 on a layout that breaks a rule other
    than the frame_stride one. Python integers: no overflow to think about"""
    if w < 2 or h < 2 or w > MAX_SIDE or h > MAX_SIDE or w % 2 or h % 2:
        return -1
    pl = planes(L.pix, w, h)
    if pl is None:
        return -1
    ranges = []
    for p in range(3):
        pitch, off = int(L.pitch[p]), int(L.offset[p])
        if p >= len(pl):
            if pitch != 0 or off != 0:
                return -1
            continue
        rb, rows = pl[p]
        if pitch < rb or pitch > MAX_PITCH or off < 0:
            return -1
        ranges.append((off, off + (rows - 1) * pitch + rb))
    for i, (a0, a1) in enumerate(ranges):
        for b0, b1 in ranges[:i]:
            if a0 < b1 and b0 < a1:
                return -1
    s = max(e for _, e in ranges)
    return s if s <= INT64_MAX else -1


def layout_ok(L, w, h):
    s = span(L, w, h)
    return s >= 0 and int(L.frame_stride) >= s


def _split(i420, w, h):
    i420 = np.asarray(i420, np.uint8).ravel()
    y = i420[:w * h].reshape(h, w)
    u = i420[w * h:w * h + (w // 2) * (h // 2)].reshape(h // 2, w // 2)
    v = i420[w * h + (w // 2) * (h // 2):frame_bytes(w, h)].reshape(h // 2, w // 2)
    return y, u, v


def _plane_view(buf, L, p, rb, rows):
    """rows x rb view of plane p of the frame that starts at buf[0]"""
    off, pitch = int(L.offset[p]), int(L.pitch[p])
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(rows, rb), strides=(pitch, 1))


def pack(i420, L, w, h, buf):
    """one tight I420 frame written in layout L into buf (a uint8 array that starts at the frame's base); only the bytes
    the layout names are written"""
    assert layout_ok(L, w, h) and buf.dtype == np.uint8 and buf.ndim == 1 and buf.size >= span(L, w, h)
    y, u, v = _split(i420, w, h)
    pl = planes(L.pix, w, h)
    views = [_plane_view(buf, L, p, rb, rows) for p, (rb, rows) in enumerate(pl)]
    if L.pix == I420:
        views[0][:], views[1][:], views[2][:] = y, u, v
    elif L.pix in (NV12, NV21):
        views[0][:] = y
        first, second = (u, v) if L.pix == NV12 else (v, u)
        views[1][:, 0::2] = first
        views[1][:, 1::2] = second
    else:
        yo = 0 if L.pix == YUY2 else 1  # where luma sits in a byte pair
        u2, v2 = np.repeat(u, 2, axis=0), np.repeat(v, 2, axis=0)  # C422[y][x] = C420[y >> 1][x]
        views[0][:, yo::2] = y
        views[0][:, 1 - yo::4] = u2
        views[0][:, 3 - yo::4] = v2
    return buf


def unpack(buf, L, w, h):
    """the tight I420 frame of the frame in layout L that starts at buf[0]"""
    assert layout_ok(L, w, h) and buf.size >= span(L, w, h)
    pl = planes(L.pix, w, h)
    views = [_plane_view(buf, L, p, rb, rows) for p, (rb, rows) in enumerate(pl)]
    if L.pix == I420:
        y, u, v = views
    elif L.pix in (NV12, NV21):
        y = views[0]
        first, second = views[1][:, 0::2], views[1][:, 1::2]
        u, v = (first, second) if L.pix == NV12 else (second, first)
    else:
        yo = 0 if L.pix == YUY2 else 1
        y = views[0][:, yo::2]
        u2 = views[0][:, 1 - yo::4].astype(np.uint16)
        v2 = views[0][:, 3 - yo::4].astype(np.uint16)
        u = ((u2[0::2] + u2[1::2] + 1) >> 1).astype(np.uint8)  # C420[y][x] = (C422[2y][x] + C422[2y+1][x] + 1) >> 1
        v = ((v2[0::2] + v2[1::2] + 1) >> 1).astype(np.uint8)
    return np.concatenate([np.ascontiguousarray(y).ravel(), np.ascontiguousarray(u).ravel(), np.ascontiguousarray(v).ravel()])


def pack_frames(frames, L, w, h, buf):
    """frames[f] into buf at f * frame_stride"""
    for f, fr in enumerate(frames):
        pack(fr, L, w, h, buf[f * int(L.frame_stride):])
    return buf


def unpack_frames(buf, L, w, h, n):
    return np.stack([unpack(buf[f * int(L.frame_stride):], L, w, h) for f in range(n)])


def total_bytes(L, w, h, n):
    """bytes that n frames in L take: the last frame ends at its span"""
    return (n - 1) * int(L.frame_stride) + span(L, w, h)
