"""GPU: the encoder's forward residual path (enc_mb_kernel.inc: xf_fwd, quant1, the DC quantisers, the CBP) held to
tests/fwdref.py on the GPU encoder's own bytes.

The clips of fwdaudit.directed_clips() of one geometry, bitrate, frame count and IDR plan are the streams of one batch.
Per frame and stream parseref -> reconref (with its prediction) -> fwdref must find no disagreement between the levels
and coded_block_pattern in the bytes and those the rules demand of source - prediction, and dbkref's planes must equal
h264mi_enc_ref_planes, carried from frame to frame. With one slice the bytes also equal the oracle encoder's, so a failure
says which side left the rule, and fwdaudit's count on the GPU's bytes must find the cells and classes the clip claims.
With three slices (two on two-row pictures, one on one-row pictures) the oracle encoder has no bytes: there only fwdref
and the decode chain speak."""
import ctypes

import numpy as np
import pytest

import dbkref
import encaudit
import fwdaudit
import fwdref
import parseref
import reconref
from test_gpu_dbk_reference import _ref_planes

pytestmark = pytest.mark.gpu


def _groups():
    out = {}
    for c in fwdaudit.directed_clips():
        out.setdefault((c.w, c.h, c.br, len(c.frames), tuple(sorted(c.idr))), []).append(c)
    return out


GROUPS = _groups()
IDS = [f'{w}x{h}_{br}_{n}f' + ('_idr' + '_'.join(map(str, idr)) if idr else '') for (w, h, br, n, idr) in GROUPS]


def _slices_for(clip, n):
    return min(n, (clip.h + 15) // 16)


def _drive(oracle, clips, nslices=1, gom=False, claims=True):
    import torch
    import h264mi
    c0 = clips[0]
    S, names, mbw = len(clips), oracle.branch_names(), (c0.w + 15) // 16
    n = _slices_for(c0, nslices)
    enc = h264mi.BatchEncoder(c0.w, c0.h, c0.br, S)
    frames = [[] for _ in clips]
    try:
        enc.set_frame_skip(False)
        if gom:
            enc.set_gom_exact(True)
        enc.set_slices(n)
        oes = [c.encoder(oracle) for c in clips]
        for oe in oes:
            oe.set_gom_exact(gom)
        states, prev = [parseref.State() for _ in clips], [None] * S
        for t in range(len(c0.frames)):
            if t in c0.idr:
                enc.force_idr()
            enc.encode(torch.from_numpy(np.stack([c.frames[t] for c in clips])).cuda())
            nb = enc.nal_sizes()
            for s, c in enumerate(clips):
                label = f'{c.name} (stream {s} of {S}), {n} slices{", exact GOM" if gom else ""}, frame {t}'
                assert nb[s] > 0, label
                got = enc.nal_bytes(s, nb[s])
                p = parseref.parse(got, states[s])
                res = reconref.reconstruct(p.syntax, p.geometry, prev[s])
                prev[s] = dbkref.deblock(res.planes, res.records).planes
                fr, mm = fwdref.check_frame(c.frames[t], c.w, c.h, p, res, label)
                ref = None
                if n == 1:
                    if t in c.idr:
                        oes[s].force_idr()
                    ref = oes[s].encode(c.frames[t])
                if mm is not None:
                    side = '' if ref is None else (' -- the bytes equal the oracle\'s: kernel and oracle left the rule together' if got == ref else
                                                   ' -- the bytes differ from the oracle\'s: the kernel left the rule')
                    raise AssertionError(str(mm) + side)
                if ref is not None and got != ref:
                    raise AssertionError(encaudit.explain_mismatch(label, names, mbw, encaudit.gpu_mbinfo(enc, s), oes[s].mbinfo(), oes[s].mb_branches(),
                                                                   len(got), len(ref)))
                mine = _ref_planes(enc, s, 16 * p.geometry[0], 16 * p.geometry[1])
                assert all(np.array_equal(np.asarray(a)[:hh, :ww], np.asarray(b)[:hh, :ww]) for a, b, (hh, ww) in
                           zip(prev[s], mine, ((c.h, c.w), (c.h // 2, c.w // 2), (c.h // 2, c.w // 2)))), \
                    f'{label}: parseref -> reconref -> dbkref differs from the encoder\'s reference planes'
                frames[s].append((fr, mm, prev[s]))
    finally:
        enc.close()
    if claims:
        for c, f in zip(clips, frames):   # the GPU's own bytes pin what the clip is there for
            both, _, cl = fwdaudit.count_frames(f)
            missed = [k for k in c.targets if fwdaudit.cell_of(k) not in both] + [k for k in c.classes if k in fwdaudit.CLASSES and not cl[k]]
            assert not missed, f'{c.name}: the GPU\'s bytes do not reach {missed}'
            for m in fwdref.MUTATIONS:
                if m.name in c.classes:
                    assert fwdaudit.catches(f, m) is not None, f'{c.name}: {m.name} is not caught on the GPU\'s bytes'
    return frames


@pytest.mark.parametrize('nslices', [1, 3])
@pytest.mark.parametrize('key', list(GROUPS), ids=IDS)
def test_directed_clips_levels_vs_fwdref(gpu_lib, oracle, key, nslices):
    clips = GROUPS[key]
    if nslices > 1 and _slices_for(clips[0], nslices) == 1:
        nslices = 1   # a one-row picture has one slice: the same check once more, as its own case
    _drive(oracle, clips, nslices, claims=(nslices == 1))


def test_48x48_batch_reversed_stream_order(gpu_lib, oracle):
    """the largest batch of 48x48 clips again with the streams in reverse order: a stream-index slip in the residual
    path shows"""
    key = max((k for k in GROUPS if k[:2] == (48, 48)), key=lambda k: len(GROUPS[k]))
    assert len(GROUPS[key]) >= 2
    _drive(oracle, GROUPS[key][::-1])


@pytest.mark.parametrize('geo', [(18, 18), (50, 34)], ids=lambda g: f'{g[0]}x{g[1]}')
def test_padded_source_reaches_the_blocks(gpu_lib, oracle, geo):
    """the clips whose source is padded to the macroblock grid, each alone: padded columns and rows stand in coded blocks,
    and fwdref with the padding by zero or by mirror disagrees with the GPU's bytes"""
    clips = [c for c in fwdaudit.directed_clips() if (c.w, c.h) == geo]
    assert clips
    c = clips[0]
    frames = _drive(oracle, [c], claims=False)[0]
    _, _, cl = fwdaudit.count_frames(frames)
    assert cl['padded_columns_in_block'] and cl['padded_rows_in_block'], c.name
    for how in ('zero', 'mirror'):
        assert fwdaudit.catches(frames, fwdref.Rules(f'source padded by {how}', pad=how)) is not None, (c.name, how)


def test_48x48_clips_with_exact_gom(gpu_lib, oracle):
    """QP changes inside a picture: the 48x48 clips of one batch with set_gom_exact; the oracle in the same mode"""
    key = max((k for k in GROUPS if k[:2] == (48, 48)), key=lambda k: len(GROUPS[k]))
    frames = _drive(oracle, GROUPS[key], gom=True, claims=False)
    assert any(len({int(q) for q in fr.qe[fr.typ != fwdref.PSKIP]}) > 1 for f in frames for fr, _, _ in f), 'no picture with more than one QP'


def test_clip_through_the_c_abi(gpu_lib, oracle):
    """one clip through init_encoder / encode_frame_yuv_i420 (frame skipping on, as the wrapper's encoder): bytes ==
    the oracle's and fwdref agrees on every coded frame"""
    clip = next(c for c in fwdaudit.directed_clips() if (c.w, c.h) == (80, 48) and c.br >= 2000000)
    L = gpu_lib
    assert L.init_encoder(clip.w, clip.h, clip.br) == 0
    oe = oracle.encoder(clip.w, clip.h, clip.br)
    ex = encaudit.Explainer(oracle, oe, clip.name + ' (C-ABI)')
    p = ctypes.POINTER(ctypes.c_ubyte)()
    sz = ctypes.c_int(0)
    units = []
    for t, f in enumerate(clip.frames):
        L.encode_frame_yuv_i420(f.ctypes.data, clip.w, clip.h, ctypes.byref(p), ctypes.byref(sz))
        got = ctypes.string_at(p, sz.value) if sz.value > 0 else b''
        ex.check(t, got, oe.encode(f))
        units.append(got)
    assert sum(len(u) > 0 for u in units) >= 2
    for _, mm, _ in fwdaudit.chain(clip, units, clip.name + ' (C-ABI)'):
        assert mm is None, str(mm)
