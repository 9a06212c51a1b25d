"""GPU: the encoder's decision branches against the oracle on directed content.

encaudit.DIRECTED holds seeded clips of 16x16 .. 176x144 that together reach every decision-branch class of the oracle
encoder that is not excluded (tests/test_enc_branch_audit.py holds them to that on the CPU). Here the GPU encoder codes
them: the clips of one geometry, bitrate and rate-control mode as the streams of one batch, frame by frame against the
oracle -- NAL bytes, the rate control's state, the deblocked reconstruction and the macroblock records {type, QP, cbp,
first vector, TotalCoeff sum} -- and once more with the streams in reverse order; one clip through the C-ABI. A
mismatch names the first differing macroblock, both sides' values and the branch classes the oracle took there.
Bit-exact, no tolerance."""
import ctypes

import numpy as np
import pytest

import encaudit

pytestmark = pytest.mark.gpu


def _groups():
    out = {}
    for c in encaudit.directed_clips():
        out.setdefault((c.w, c.h, c.br, len(c.frames), c.gom), []).append(c)
    return out


GROUPS = _groups()
IDS = [f'{w}x{h}_{br}_{"gom" if gom else "rows"}' for (w, h, br, n, gom) in GROUPS]


def _recon(enc, s):
    import h264mi
    w, h = enc.w, enc.h
    cw, ch = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    buf = np.empty(cw * ch * 3 // 2, np.uint8)
    h264mi._hip_memcpy_d2h(buf.ctypes.data, enc.recon_ptr(s), buf.size)
    y = buf[:cw * ch].reshape(ch, cw)[:h, :w]
    u = buf[cw * ch:cw * ch * 5 // 4].reshape(ch // 2, cw // 2)[:h // 2, :w // 2]
    v = buf[cw * ch * 5 // 4:].reshape(ch // 2, cw // 2)[:h // 2, :w // 2]
    return np.concatenate([y.ravel(), u.ravel(), v.ravel()])


def _drive(oracle, clips):
    import torch
    import h264mi
    c0 = clips[0]
    S, names, mbw = len(clips), oracle.branch_names(), (c0.w + 15) // 16
    enc = h264mi.BatchEncoder(c0.w, c0.h, c0.br, S)
    enc.set_frame_skip(False)
    enc.set_gom_exact(c0.gom)
    oes = [c.encoder(oracle) for c in clips]
    for t in range(len(c0.frames)):
        enc.encode(torch.from_numpy(np.stack([c.frames[t] for c in clips])).cuda())
        n = enc.nal_sizes()
        for s, c in enumerate(clips):
            ref = oes[s].encode(c.frames[t])
            got = enc.nal_bytes(s, n[s]) if n[s] else b''
            gi, oi = encaudit.gpu_mbinfo(enc, s), oes[s].mbinfo()
            label = f'{c.name} (stream {s} of {S}) frame {t}'
            if got != ref or encaudit.records_differ(gi, oi)[0].size:
                raise AssertionError(encaudit.explain_mismatch(label, names, mbw, gi, oi, oes[s].mb_branches(), len(got), len(ref)))
            assert len(ref) > 0, label
            assert enc.rc_state(s) == oes[s].rc_state(), label
            if c.gom and t > 0:
                assert enc.gom_state(s) == oes[s].gom_state(), label
            rec, want = _recon(enc, s), oes[s].recon()
            assert np.array_equal(rec, want), f'{label}: {int((rec != want).sum())} samples of the reconstruction differ, bytes equal'
    enc.close()
    return oes


@pytest.mark.parametrize('key', list(GROUPS), ids=IDS)
def test_directed_clips_batch_vs_oracle(gpu_lib, oracle, key):
    clips = GROUPS[key]
    oes = _drive(oracle, clips)
    names = oracle.branch_names()
    for c, oe in zip(clips, oes):  # the oracle beside the GPU took the classes the clip is there for
        counts = oe.branch_counts()
        assert all(counts[names.index(t)] > 0 for t in c.targets), c.name


def test_directed_clips_batch_reversed_stream_order(gpu_lib, oracle):
    """the three 48x48 clips again with the streams in reverse order: a stream-index slip shows"""
    clips = [c for k, g in GROUPS.items() if k[:2] == (48, 48) for c in g]
    assert len(clips) >= 3
    _drive(oracle, clips[::-1])


def test_directed_clip_through_the_c_abi(gpu_lib, oracle):
    """one clip through init_encoder / encode_frame_yuv_i420: the half-moving 80x48 picture"""
    clip = next(c for c in encaudit.directed_clips() if (c.w, c.h, c.br) == (80, 48, 3000000))
    L = gpu_lib
    assert L.init_encoder(clip.w, clip.h, clip.br) == 0
    oe = oracle.encoder(clip.w, clip.h, clip.br)  # frame skipping on, as the wrapper's encoder
    ex = encaudit.Explainer(oracle, oe, clip.name + ' (C-ABI)')
    p = ctypes.POINTER(ctypes.c_ubyte)()
    sz = ctypes.c_int(0)
    coded = 0
    for t, f in enumerate(clip.frames):
        L.encode_frame_yuv_i420(f.ctypes.data, clip.w, clip.h, ctypes.byref(p), ctypes.byref(sz))
        got = ctypes.string_at(p, sz.value) if sz.value > 0 else b''
        ex.check(t, got, oe.encode(f))
        coded += len(got) > 0
    assert coded >= 2
