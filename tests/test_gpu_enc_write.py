"""GPU: the encoder's bit writer (csrc/enc_bits.inc) on the directed clips of tests/writeaudit.py.

The clips of one geometry, bitrate, frame count and IDR plan are the streams of one batch. With one slice every frame's
bytes equal the oracle encoder's (a mismatch names the first differing macroblock, encaudit.explain_mismatch). With three
slices (as many as the picture has MB rows, if fewer) the oracle encoder has nothing to compare with -- it codes one slice
per picture -- so the oracle decoder decodes the bytes and must give the encoder's own reconstruction, and for the
pictures of at most 80x48 the from-bytes chain (parseref -> reconref -> dbkref) must give the encoder's reference planes.
Both times
writeaudit.count runs on the GPU's own bytes and must find the classes the clip claims: `targets` with one slice,
`slice_targets` with three. The large and the extreme geometries go once through encode_frame_yuv_i420."""
import ctypes

import numpy as np
import pytest

import dbkref
import encaudit
import parseref
import reconref
import writeaudit
from test_gpu_dbk_reference import _ref_planes
from test_gpu_enc_branches import _recon

pytestmark = pytest.mark.gpu


def _groups():
    out = {}
    for c in writeaudit.directed_clips():
        out.setdefault((c.w, c.h, c.br, len(c.frames), tuple(sorted(c.idr))), []).append(c)
    return out


GROUPS = _groups()
IDS = [f'{w}x{h}_{br}_{n}f' + ('_idr' if idr else '') for (w, h, br, n, idr) in GROUPS]


@pytest.mark.parametrize('nslices', [1, 3])
@pytest.mark.parametrize('key', list(GROUPS), ids=IDS)
def test_directed_clips_bytes_and_classes(gpu_lib, oracle, key, nslices):
    import torch
    import h264mi
    clips = GROUPS[key]
    c0 = clips[0]
    S, names, mbw = len(clips), oracle.branch_names(), (c0.w + 15) // 16
    n = writeaudit.slices_for(c0, nslices)
    enc = h264mi.BatchEncoder(c0.w, c0.h, c0.br, S)
    try:
        enc.set_frame_skip(False)
        enc.set_slices(n)
        oes = [c.encoder(oracle) for c in clips]
        ods = [oracle.decoder() for _ in clips]
        units = [[] for _ in clips]
        chain = n > 1 and c0.w * c0.h <= 80 * 48   # the from-bytes chain, which knows neither encoder nor oracle decoder
        states, prev = [parseref.State() for _ in clips], [None] * S
        for t in range(len(c0.frames)):
            if t in c0.idr:
                enc.force_idr()
            enc.encode(torch.from_numpy(np.stack([c.frames[t] for c in clips])).cuda())
            nb = enc.nal_sizes()
            for s, c in enumerate(clips):
                label = f'{c.name} (stream {s} of {S}), {n} slices, frame {t}'
                assert nb[s] > 0, label
                got = enc.nal_bytes(s, nb[s])
                units[s].append(got)
                if n == 1:
                    if t in c.idr:
                        oes[s].force_idr()
                    ref = oes[s].encode(c.frames[t])
                    if got != ref:
                        raise AssertionError(encaudit.explain_mismatch(label, names, mbw, encaudit.gpu_mbinfo(enc, s), oes[s].mbinfo(),
                                                                       oes[s].mb_branches(), len(got), len(ref)))
                rc, pic, dw, dh = ods[s].decode(got)
                assert rc == 1 and (dw, dh) == (c.w, c.h), f'{label}: oracle decoder rc {rc}, {dw}x{dh}'
                if chain:
                    p = parseref.parse(got, states[s])
                    res = reconref.reconstruct(p.syntax, p.geometry, prev[s])
                    prev[s] = dbkref.deblock(res.planes, res.records).planes
                    mine = _ref_planes(enc, s, 16 * p.geometry[0], 16 * p.geometry[1])
                    assert all(np.array_equal(np.asarray(a)[:hh, :ww], np.asarray(b)[:hh, :ww]) for a, b, (hh, ww) in
                               zip(prev[s], mine, ((c.h, c.w), (c.h // 2, c.w // 2), (c.h // 2, c.w // 2)))), \
                        f'{label}: the from-bytes chain differs from the encoder\'s reference planes'
                rec = _recon(enc, s)
                assert np.array_equal(rec, pic), f'{label}: {int((rec != pic).sum())} samples of the oracle decoder\'s picture differ from the reconstruction'
    finally:
        enc.close()
    for c, u in zip(clips, units):   # the GPU's own bytes reach what the clip is there for
        got = writeaudit.count_clip(u)
        want = c.targets if n == 1 else c.slice_targets
        missed = [k for k in want if not got[k]]
        assert not missed, f'{c.name}, {n} slices: the GPU\'s bytes do not reach {missed}'
        if n > 1:
            print(f'\n{c.name}, {n} slices:', sorted((k for k in got if got[k] and writeaudit.is_slice_class(k)), key=str))


@pytest.mark.parametrize('geo', [(3072, 2160), (16, 4096), (8192, 16)], ids=lambda g: f'{g[0]}x{g[1]}')
def test_large_and_extreme_geometries_through_the_c_abi(gpu_lib, oracle, geo):
    clip = next(c for c in writeaudit.directed_clips() if (c.w, c.h) == geo)
    L = gpu_lib
    assert L.init_encoder(clip.w, clip.h, clip.br) == 0
    oe = oracle.encoder(clip.w, clip.h, clip.br)   # frame skipping on, as the wrapper's encoder
    ex = encaudit.Explainer(oracle, oe, clip.name + ' (C-ABI)')
    p = ctypes.POINTER(ctypes.c_ubyte)()
    sz = ctypes.c_int(0)
    coded = 0
    for t, f in enumerate(clip.frames):
        L.encode_frame_yuv_i420(f.ctypes.data, clip.w, clip.h, ctypes.byref(p), ctypes.byref(sz))
        got = ctypes.string_at(p, sz.value) if sz.value > 0 else b''
        ex.check(t, got, oe.encode(f))
        coded += len(got) > 0
    assert coded >= 1
