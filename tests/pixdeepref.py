"""Reference of the deeper and wider pixel layouts, ids 16..24 (TEST INFRASTRUCTURE): a numpy restatement of their
definition in include/h264mi.h (the second table of h264mi_pix_layout, h264mi_pixopt), written from that text alone.
Layouts are pixref.Layout objects (h264mi.PixLayout has the same attributes); a frame on the I420 side is the tight
w*h*3/2 byte array of pixref. Samples are handled as Python-wide integers (int64 arrays), never as packed words."""
import numpy as np

import pixref
from pixref import Layout, frame_bytes, MAX_SIDE, MAX_PITCH, INT64_MAX

I422, I444, NV16, Y800, P010, I010, P210, I210, V210 = range(16, 25)
ALL = (I422, I444, NV16, Y800, P010, I010, P210, I210, V210)
NAMES = {I422: 'I422', I444: 'I444', NV16: 'NV16', Y800: 'Y800', P010: 'P010', I010: 'I010', P210: 'P210', I210: 'I210', V210: 'V210'}
TEN_BIT = (P010, I010, P210, I210, V210)
ROUND, DITHER, TRUNC = 0, 1, 2
DEPTHS = (ROUND, DITHER, TRUNC)
D = ((0, 2), (3, 1))


def unit(pix):
    """1, 2 or 4; -1 for an unknown format"""
    if pix in (0, 1, 2, 3, 4, I422, I444, NV16, Y800):
        return 1
    if pix in (P010, I010, P210, I210):
        return 2
    return 4 if pix == V210 else -1


def planes(pix, w, h):
    """[(row bytes, rows)]; None for an unknown format (ids 0..4 are pixref's)"""
    return {I422: [(w, h), (w // 2, h), (w // 2, h)],
            I444: [(w, h), (w, h), (w, h)],
            NV16: [(w, h), (w, h)],
            Y800: [(w, h)],
            P010: [(2 * w, h), (2 * w, h // 2)],
            I010: [(2 * w, h), (w, h // 2), (w, h // 2)],
            P210: [(2 * w, h), (2 * w, h)],
            I210: [(2 * w, h), (w, h), (w, h)],
            V210: [(16 * -(-w // 6), h)]}.get(pix)


def tight(pix, w, h):
    pl = planes(pix, w, h)
    if pix == V210:
        pitch = 128 * -(-w // 48)
        return Layout(pix, [pitch], [0], h * pitch)
    offset, at = [], 0
    for rb, rows in pl:
        offset.append(at)
        at += rb * rows
    return Layout(pix, [rb for rb, _ in pl], offset, at)


def span(L, w, h):
    """as pixref.span, with the unit rule for the used pitches and offsets"""
    if w < 2 or h < 2 or w > MAX_SIDE or h > MAX_SIDE or w % 2 or h % 2:
        return -1
    pl = planes(L.pix, w, h)
    if pl is None:
        return -1
    u = unit(L.pix)
    ranges = []
    for p in range(3):
        pitch, off = int(L.pitch[p]), int(L.offset[p])
        if p >= len(pl):
            if pitch != 0 or off != 0:
                return -1
            continue
        rb, rows = pl[p]
        if pitch < rb or pitch > MAX_PITCH or off < 0 or pitch % u or off % u:
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
    return s >= 0 and int(L.frame_stride) >= s and int(L.frame_stride) % unit(L.pix) == 0


def _rows(buf, L, p, rb, rows):
    """rows x rb byte view of plane p of the frame that starts at buf[0]"""
    off, pitch = int(L.offset[p]), int(L.pitch[p])
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(rows, rb), strides=(pitch, 1))


def _words(view):
    """16-bit LE words of a byte view, as int64"""
    return view[:, 0::2].astype(np.int64) | (view[:, 1::2].astype(np.int64) << 8)


def _put_words(view, words):
    view[:, 0::2] = (words & 255).astype(np.uint8)
    view[:, 1::2] = (words >> 8).astype(np.uint8)


# V210: field f of a group (bits 10 (f % 3) .. of word f // 3), in the order the header's four words list them
_V210_FIELDS = ('Cb0', 'Y0', 'Cr0', 'Y1', 'Cb1', 'Y2', 'Cr1', 'Y3', 'Cb2', 'Y4', 'Cr2', 'Y5')


def _v210_read(view, w, h):
    """(Y h x w, Cb h x w/2, Cr h x w/2) 10-bit values of a V210 plane; fields beyond w are ignored"""
    ng = view.shape[1] // 16
    wd = (view[:, 0::4].astype(np.int64) | (view[:, 1::4].astype(np.int64) << 8) | (view[:, 2::4].astype(np.int64) << 16)
          | (view[:, 3::4].astype(np.int64) << 24)).reshape(h, ng, 4)
    Y = np.zeros((h, 6 * ng), np.int64)
    Cb = np.zeros((h, 3 * ng), np.int64)
    Cr = np.zeros((h, 3 * ng), np.int64)
    for f, name in enumerate(_V210_FIELDS):
        val = (wd[:, :, f // 3] >> (10 * (f % 3))) & 1023
        k = int(name[-1])
        {'Y': Y, 'Cb': Cb, 'Cr': Cr}[name[:-1]][:, k::(6 if name[0] == 'Y' else 3)] = val
    return Y[:, :w], Cb[:, :w // 2], Cr[:, :w // 2]


def _v210_write(view, Y, Cb, Cr, w, h):
    ng = view.shape[1] // 16
    Yp = np.zeros((h, 6 * ng), np.int64); Yp[:, :w] = Y
    Cbp = np.zeros((h, 3 * ng), np.int64); Cbp[:, :w // 2] = Cb
    Crp = np.zeros((h, 3 * ng), np.int64); Crp[:, :w // 2] = Cr
    wd = np.zeros((h, ng, 4), np.int64)
    for f, name in enumerate(_V210_FIELDS):
        k = int(name[-1])
        src = {'Y': Yp, 'Cb': Cbp, 'Cr': Crp}[name[:-1]][:, k::(6 if name[0] == 'Y' else 3)]
        wd[:, :, f // 3] |= src << (10 * (f % 3))
    wd = wd.reshape(h, 4 * ng)
    for b in range(4):
        view[:, b::4] = ((wd >> (8 * b)) & 255).astype(np.uint8)


def _narrow(v, depth):
    """step 3: 10-bit values of an output plane to 8 bits; x, y are positions in that plane"""
    if depth == ROUND:
        return np.minimum(255, (v + 2) >> 2)
    if depth == TRUNC:
        return v >> 2
    assert depth == DITHER
    hh, ww = v.shape
    d = np.array(D, np.int64)[np.arange(hh)[:, None] & 1, np.arange(ww)[None, :] & 1]
    return np.minimum(255, (v + d) >> 2)


def _source(buf, L, w, h):
    """(Y, Cb, Cr, subsampling) at source depth, as int64 arrays"""
    pl = planes(L.pix, w, h)
    v = [_rows(buf, L, p, rb, rows) for p, (rb, rows) in enumerate(pl)]
    pix = L.pix
    if pix in (I422, I444):
        return v[0].astype(np.int64), v[1].astype(np.int64), v[2].astype(np.int64), '422' if pix == I422 else '444'
    if pix == NV16:
        return v[0].astype(np.int64), v[1][:, 0::2].astype(np.int64), v[1][:, 1::2].astype(np.int64), '422'
    if pix == Y800:
        return v[0].astype(np.int64), None, None, 'grey'
    if pix in (P010, P210):
        c = _words(v[1]) >> 6
        return _words(v[0]) >> 6, c[:, 0::2], c[:, 1::2], '420' if pix == P010 else '422'
    if pix in (I010, I210):
        return _words(v[0]) & 1023, _words(v[1]) & 1023, _words(v[2]) & 1023, '420' if pix == I010 else '422'
    assert pix == V210
    return _v210_read(v[0], w, h) + ('422',)


def unpack(buf, L, w, h, depth=ROUND):
    """the tight I420 frame of the frame in layout L that starts at buf[0], under depth rule `depth`"""
    assert layout_ok(L, w, h) and buf.size >= span(L, w, h)
    Y, Cb, Cr, sub = _source(buf, L, w, h)
    if sub == 'grey':
        Cb = Cr = np.full((h // 2, w // 2), 128, np.int64)
    elif sub == '422':
        Cb, Cr = (Cb[0::2] + Cb[1::2] + 1) >> 1, (Cr[0::2] + Cr[1::2] + 1) >> 1
    elif sub == '444':
        Cb = (Cb[0::2, 0::2] + Cb[0::2, 1::2] + Cb[1::2, 0::2] + Cb[1::2, 1::2] + 2) >> 2
        Cr = (Cr[0::2, 0::2] + Cr[0::2, 1::2] + Cr[1::2, 0::2] + Cr[1::2, 1::2] + 2) >> 2
    if L.pix in TEN_BIT:
        Y, Cb, Cr = _narrow(Y, depth), _narrow(Cb, depth), _narrow(Cr, depth)
    return np.concatenate([Y.ravel(), Cb.ravel(), Cr.ravel()]).astype(np.uint8)


def pack(i420, L, w, h, buf):
    """one tight I420 frame written in layout L into buf (a uint8 array that starts at the frame's base); only the bytes
    the layout names are written"""
    assert layout_ok(L, w, h) and buf.dtype == np.uint8 and buf.ndim == 1 and buf.size >= span(L, w, h)
    y, u, v = (a.astype(np.int64) for a in pixref._split(i420, w, h))
    pl = planes(L.pix, w, h)
    views = [_rows(buf, L, p, rb, rows) for p, (rb, rows) in enumerate(pl)]
    pix = L.pix
    u2, v2 = np.repeat(u, 2, axis=0), np.repeat(v, 2, axis=0)  # 4:2:2: C[y][x] = C420[y >> 1][x]
    if pix == I422:
        views[0][:], views[1][:], views[2][:] = y, u2, v2
    elif pix == I444:
        views[0][:] = y
        views[1][:], views[2][:] = np.repeat(u2, 2, axis=1), np.repeat(v2, 2, axis=1)  # C420[y >> 1][x >> 1]
    elif pix == NV16:
        views[0][:] = y
        views[1][:, 0::2], views[1][:, 1::2] = u2, v2
    elif pix == Y800:
        views[0][:] = y
    elif pix in (P010, P210):
        cu, cv = (u, v) if pix == P010 else (u2, v2)
        _put_words(views[0], (y << 2) << 6)
        c = np.zeros((cu.shape[0], w), np.int64)
        c[:, 0::2], c[:, 1::2] = (cu << 2) << 6, (cv << 2) << 6
        _put_words(views[1], c)
    elif pix in (I010, I210):
        cu, cv = (u, v) if pix == I010 else (u2, v2)
        _put_words(views[0], y << 2)
        _put_words(views[1], cu << 2)
        _put_words(views[2], cv << 2)
    else:
        _v210_write(views[0], y << 2, u2 << 2, v2 << 2, w, h)
    return buf


def pack_frames(frames, L, w, h, buf):
    """frames[f] into buf at f * frame_stride"""
    for f, fr in enumerate(frames):
        pack(fr, L, w, h, buf[f * int(L.frame_stride):])
    return buf


def unpack_frames(buf, L, w, h, n, depth=ROUND):
    return np.stack([unpack(buf[f * int(L.frame_stride):], L, w, h, depth) for f in range(n)])


def total_bytes(L, w, h, n):
    return (n - 1) * int(L.frame_stride) + span(L, w, h)
