"""GPU: the encoder's P-macroblock decisions (enc_mb_kernel.inc: the judge, keep, the intra alternative, the search, the
refinement, the double check, the row QP) held to tests/mdref.py on the GPU encoder's own bytes.

The clips of mdaudit.clips() of one geometry, bitrate, frame count and IDR plan are the streams of one batch. Per frame
and stream parseref -> reconref -> dbkref -> mdref must find every macroblock's outcome in the bytes to be the one the
rules demand, and dbkref's planes must equal h264mi_enc_ref_planes. With one slice the bytes also equal the oracle
encoder's, so a failure says which side left the rule. With two and three slices the oracle encoder has no bytes: there
mdref is the only statement of what the encoder chooses beside a slice edge, and each slice-edge mutation must be caught
on these bytes by the clip that claims it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import encaudit
import mdaudit
import mdref
from test_gpu_dbk_reference import _ref_planes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_SLICE = {(16, 16), (16, 32), (16, 48), (48, 16), (48, 32), (48, 48), (80, 48), (18, 18), (50, 34)}


def _groups(clips):
    out = {}
    for c in clips:
        if not c.gom:
            out.setdefault((c.w, c.h, c.br, len(c.frames), tuple(sorted(c.idr))), []).append(c)
    return out


def _ids(groups):
    return [f'{w}x{h}_{br}_{n}f' + ('_idr' + '_'.join(map(str, idr)) if idr else '') for (w, h, br, n, idr) in groups]


SMALL = _groups(c for c in mdaudit.clips() if (c.w, c.h) in ONE_SLICE)
THREE = {k: v for k, v in SMALL.items() if k[:2] in ((48, 48), (80, 48))}
EDGE = _groups(mdaudit.slice_clips())


def _drive(oracle, clips, nslices=1):
    """-> per clip the mdref.Picture of every frame; every assertion of the module's docstring made on the way"""
    import torch
    import h264mi
    c0 = clips[0]
    S, names, mbw = len(clips), oracle.branch_names(), (c0.w + 15) // 16
    enc = h264mi.BatchEncoder(c0.w, c0.h, c0.br, S)
    pics = [[] for _ in clips]
    counts = [mdref.Checked() for _ in clips]
    try:
        enc.set_frame_skip(False)
        enc.set_slices(nslices)
        oes = [c.encoder(oracle) for c in clips]
        streams = [mdaudit.stream_of(c, nslices) for c in clips]
        for t in range(len(c0.frames)):
            if t in c0.idr:
                enc.force_idr()
            enc.encode(torch.from_numpy(np.stack([c.frames[t] for c in clips])).cuda())
            nb = enc.nal_sizes()
            for s, c in enumerate(clips):
                label = f'{c.name} (stream {s} of {S}), {nslices} slices, frame {t}'
                assert nb[s] > 0, label
                got = enc.nal_bytes(s, nb[s])
                pic, parsed, res, planes = mdaudit.step(streams[s], c, t, got, label)
                assert len({int(v) for v in pic.first}) == nslices, f'{label}: not {nslices} slices in the bytes'
                mm = mdref.check(pic, None, counts[s])
                ref = None
                if nslices == 1:
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
                mine = _ref_planes(enc, s, 16 * parsed.geometry[0], 16 * parsed.geometry[1])
                assert all(np.array_equal(np.asarray(a)[:hh, :ww], np.asarray(b)[:hh, :ww]) for a, b, (hh, ww) in
                           zip(planes, mine, ((c.h, c.w), (c.h // 2, c.w // 2), (c.h // 2, c.w // 2)))), \
                    f'{label}: parseref -> reconref -> dbkref differs from the encoder\'s reference planes'
                pics[s].append(pic)
    finally:
        enc.close()
    for c, k in zip(clips, counts):
        print(f'{c.name}, {nslices} slices: {k.mbs} macroblocks, outcomes {k.outcomes}, intra macroblocks whose I4 / I16 kind is not restated: {k.intra_kind_open}')
    return pics


def _claims(clips, pics, nslices, kinds):
    for m in mdref.MUTATIONS:
        who = mdaudit.CLAIMS.get(m.name)
        if m.kind in kinds and who is not None and who[1] == nslices:
            for c, f in zip(clips, pics):
                if c.name == who[0]:
                    mm = mdaudit.catches(f, m)
                    assert mm is not None, f'{c.name}, {nslices} slices: "{m.name}" is not caught on the GPU\'s bytes'
                    assert 'macroblock' in str(mm)


@pytest.mark.parametrize('key', list(SMALL), ids=_ids(SMALL))
def test_one_slice_decisions_vs_mdref_and_oracle(gpu_lib, oracle, key):
    _drive(oracle, SMALL[key])


@pytest.mark.parametrize('key', list(THREE), ids=_ids(THREE))
def test_three_slices_every_row_a_first_row(gpu_lib, oracle, key):
    clips = THREE[key]
    _claims(clips, _drive(oracle, clips, 3), 3, ('slice',))


@pytest.mark.parametrize('key', list(EDGE), ids=_ids(EDGE))
def test_two_slices_both_kinds_of_row(gpu_lib, oracle, key):
    clips = EDGE[key]
    _claims(clips, _drive(oracle, clips, 2), 2, ('slice',))


def test_every_slice_edge_mutation_is_claimed_on_gpu_bytes():
    """the table of DESIGN §3.12: every slice-edge mutation names a clip and a slice count above one that the tests above run"""
    run = {(c.name, 2) for v in EDGE.values() for c in v} | {(c.name, 3) for v in THREE.values() for c in v}
    for m in mdref.MUTATIONS:
        if m.kind == 'slice':
            assert mdaudit.CLAIMS.get(m.name) in run, m.name


def test_largest_two_slice_batch_reversed_stream_order(gpu_lib, oracle):
    key = max(EDGE, key=lambda k: (len(EDGE[k]), k[0] * k[1]))
    assert len(EDGE[key]) >= 2
    _drive(oracle, EDGE[key][::-1], 2)


_CABI = r'''
import ctypes, os, sys
import numpy as np
sys.path.insert(0, os.path.join(sys.argv[1], 'openh264-wasm_amd'))
sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))
import torch
import h264mi
import mdaudit
torch.cuda.set_device(0)
L = h264mi.lib()
clip = next(c for c in mdaudit.slice_clips() if c.name == sys.argv[2])
assert L.init_encoder(clip.w, clip.h, clip.br) == 0
with open(sys.argv[3], 'wb') as out:
    for f in clip.frames:
        p, sz = ctypes.POINTER(ctypes.c_ubyte)(), ctypes.c_int(0)
        L.encode_frame_yuv_i420(f.ctypes.data, clip.w, clip.h, ctypes.byref(p), ctypes.byref(sz))
        u = ctypes.string_at(p, sz.value) if sz.value > 0 else b''
        out.write(len(u).to_bytes(4, 'little') + u)
print('cabi ok')
'''


def test_clip_through_the_c_abi_with_two_slices(gpu_lib, tmp_path):
    """one clip through init_encoder / encode_frame_yuv_i420 with H264MI_ENC_SLICES=2 set in a fresh process (frame
    skipping on, as the wrapper's encoder): mdref agrees with every macroblock of every coded frame"""
    clip = next(c for c in mdaudit.slice_clips() if c.br >= 2000000)
    script, units = tmp_path / 'cabi_slices.py', tmp_path / 'units.bin'
    script.write_text(_CABI)
    r = subprocess.run([sys.executable, str(script), ROOT, clip.name, str(units)], env=dict(os.environ, H264MI_ENC_SLICES='2'),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'cabi ok' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    raw, got = units.read_bytes(), []
    while raw:
        n = int.from_bytes(raw[:4], 'little')
        got.append(raw[4:4 + n])
        raw = raw[4 + n:]
    assert len(got) == len(clip.frames) and sum(len(u) > 0 for u in got) >= 3
    clip_skip = encaudit.Clip(clip.name + ' (C-ABI)', clip.w, clip.h, clip.br, clip.frames, skip=True)
    pics = mdaudit.chain(clip_skip, got, 2)
    assert all(len({int(v) for v in p.first}) == 2 for p in pics)
    mm = mdaudit.check_all(pics)
    assert mm is None, str(mm)
