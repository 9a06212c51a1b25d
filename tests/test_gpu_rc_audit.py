"""GPU: the frame-level rate control against the oracle and against the independent model.

rcaudit.DIRECTED holds seeded sequences of 16x16 .. 512x48 that together reach every class of the rate control's state
machine that is neither excluded nor listed as not reached (tests/test_rc_audit.py holds them to that on the CPU). Here
the GPU encoder codes them, the sequences of one geometry, bitrate and skip switch as the streams of one batch -- one
stream skips while another codes an IDR --, and after every frame step every stream is held to

  * the oracle's NAL bytes and rc_state, and
  * the model (tests/rcref.py) fed with the GPU's own bytes and average QP and with rcref.frame_complexity of the frames:
    a chain that uses no oracle.

Further: the frame complexity with the source at an address that is no multiple of 16, one sequence through the C-ABI,
the sequence parameters of every table cell, the two long runs across pframe_num / idr_num 254 and the frame_num wrap,
and the state a failed frame leaves. Bit-exact, no tolerance."""
import ctypes

import numpy as np
import pytest

import encaudit
import rcaudit
import rcref

pytestmark = pytest.mark.gpu


def _groups():
    out = {}
    for s in rcaudit.directed_seqs():
        out.setdefault((s.w, s.h, s.br, s.skip), []).append(s)
    return out


GROUPS = _groups()
IDS = [f'{w}x{h}_{br}_{"skip" if skip else "noskip"}' for (w, h, br, skip) in GROUPS]


def _coded(enc, s):
    return rcaudit.coded_mbs(encaudit.gpu_mbinfo(enc, s))


def _drive(oracle, seqs):
    import torch
    import h264mi
    s0 = seqs[0]
    S, n = len(seqs), max(len(s) for s in seqs)
    enc = h264mi.BatchEncoder(s0.w, s0.h, s0.br, S)
    enc.set_frame_skip(s0.skip)
    runs = [rcaudit.oracle_run(oracle, s) for s in seqs]
    models = [rcref.PyRc(s.w, s.h, s.br, s.skip) for s in seqs]
    for t in range(n):
        for i, s in enumerate(seqs):
            if t < len(s) and t in s.idr:
                enc.force_idr(i)
                models[i].force_idr()
        frames = [s.frame(min(t, len(s) - 1)) for s in seqs]  # a sequence that has ended repeats its last frame, unchecked
        enc.encode(torch.from_numpy(np.stack(frames)).cuda())
        sizes = enc.nal_sizes()
        for i, s in enumerate(seqs):
            if t >= len(s):
                continue
            label = f'{s.name} (stream {i} of {S}) frame {t}'
            ref, ost, _ = runs[i][t]
            got = enc.nal_bytes(i, sizes[i]) if sizes[i] else b''
            st = enc.rc_state(i)
            assert len(got) == len(ref) and got == ref, f'{label}: GPU {len(got)} B != oracle {len(ref)} B; state {st} vs {ost}'
            assert st == ost, label
            m = models[i]
            coded = m.begin(frames[i])
            assert coded == bool(got), label
            if coded:
                m.end(got, st['avg_qp'], _coded(enc, i))
            assert m.state() == st, f'{label}: model {m.state()} != GPU {st}'
    enc.close()
    return models


@pytest.mark.parametrize('key', list(GROUPS), ids=IDS)
def test_directed_sequences_batch_vs_oracle_and_model(gpu_lib, oracle, key):
    seqs = GROUPS[key]
    for s, m in zip(seqs, _drive(oracle, seqs)):  # the model on the GPU's own outputs took the classes the sequence is there for
        missed = [t for t in s.targets if not m.counts[t]]
        assert not missed, f'{s.name}: {missed}'
        assert not [k for k in m.counts if k in rcaudit.EXCLUDED], s.name


def _mixed(w, h, br, skip):
    """every directed sequence of one geometry coded at one bitrate: streams of one launch in different states"""
    return [rcaudit.Seq(s.w, s.h, br, skip, s.schedule, s.idr, s.seed) for s in rcaudit.directed_seqs() if (s.w, s.h) == (w, h)]


@pytest.mark.parametrize('w,h,br,skip', [(18, 18, 5832, True), (50, 34, 8160, True), (16, 16, 2000, True)], ids=['18x18', '50x34', '16x16'])
def test_mixed_states_in_one_launch(gpu_lib, oracle, w, h, br, skip):
    seqs = _mixed(w, h, br, skip)
    assert len(seqs) >= 2
    _drive(oracle, seqs)


def test_48x48_batch_and_reversed_stream_order(gpu_lib, oracle):
    """three sequences at 48x48 as one batch, and again with the streams in reverse order: a stream-index slip shows"""
    seqs = [rcaudit.Seq(48, 48, 20000, True, sch, idr, seed) for sch, idr, seed in
            (('nnnnssssssssnnnn', (), 3), ('fsssssnnnnssssss', (5, 6), 4), ('bddllllhhhhnnsss', (9,), 5))]
    _drive(oracle, seqs)
    _drive(oracle, seqs[::-1])


@pytest.mark.parametrize('w,h', [(50, 34), (18, 18), (48, 48), (512, 48), (496, 48), (176, 144)])
def test_complexity_with_the_source_off_16_byte_alignment(gpu_lib, w, h):
    """cmplx == rcref.frame_complexity with the frames at an odd device address (the scalar source path), over an IDR and
    two P frames, two streams; 176x144 has nine GOMs for eight workgroups, 512x48 and 496x48 (31 MBs, the first wide
    width) a last GOM of one MB row out of two"""
    import torch
    import h264mi
    seqs = [rcaudit.Seq(w, h, 60 * w * h, False, 'nnl', (), 11), rcaudit.Seq(w, h, 60 * w * h, False, 'bhn', (), 12)]
    enc = h264mi.BatchEncoder(w, h, 60 * w * h, 2)
    enc.set_frame_skip(False)
    fs = w * h * 3 // 2
    for off in (1, 0):
        for t in range(3):
            buf = torch.zeros(2 * fs + 16, dtype=torch.uint8)
            buf[off:off + 2 * fs] = torch.from_numpy(np.concatenate([s.frame(t) for s in seqs]))
            dev = buf.cuda()
            assert (dev.data_ptr() + off) % 16 == off
            if off == 0 and t == 0:
                enc.force_idr()
            enc.encode(dev[off:off + 2 * fs])
            assert all(n > 0 for n in enc.nal_sizes())
            for i, s in enumerate(seqs):
                prev = seqs[i].frame(t - 1 if t else 2)
                want = rcref.frame_complexity(s.frame(t), prev, w, h, t == 0)
                assert enc.rc_state(i)['cmplx'] == want, (w, h, off, t, i)
    enc.close()


def test_directed_sequence_through_the_c_abi(gpu_lib, oracle):
    """one skipping sequence with its forced IDRs (force_key_frame) through init_encoder / encode_frame_yuv_i420: sizes
    and bytes == the oracle's. The wrapper's ABI has no call that releases the encoder: init_encoder replaces the one
    before, so every test that uses it starts there, as this one does."""
    s = next(q for q in rcaudit.directed_seqs() if q.skip and q.idr and (q.w, q.h) == (18, 18))
    L = gpu_lib
    assert L.init_encoder(s.w, s.h, s.br) == 0
    run = rcaudit.oracle_run(oracle, s)
    p = ctypes.POINTER(ctypes.c_ubyte)()
    sz = ctypes.c_int(0)
    for t in range(len(s)):
        if t in s.idr:
            L.force_key_frame()
        f = s.frame(t)
        L.encode_frame_yuv_i420(f.ctypes.data, s.w, s.h, ctypes.byref(p), ctypes.byref(sz))
        got = ctypes.string_at(p, sz.value) if sz.value > 0 else b''
        assert got == run[t][0], f'{s.name} (C-ABI) frame {t}: GPU {len(got)} B vs oracle {len(run[t][0])} B'
    assert sum(1 for nal, _, _ in run if not nal) > 0 and sum(1 for nal, _, _ in run if nal) > 2
    assert all(run[t][0][4] & 31 == 7 for t in s.idr), 'the forced frames are IDR access units'


@pytest.mark.parametrize('area', [0, 1, 2, 3])
def test_table_sweep(gpu_lib, area):
    """one encoder per table cell and per side of each threshold, one flat IDR frame each: qp, min_qp, max_qp, bpf"""
    import torch
    import h264mi
    cases = [c for c in rcaudit.table_cases() if rcref.seq_params(*c)['area'] == area]
    assert len(cases) >= 8
    for w, h, br in cases:
        p = rcref.seq_params(w, h, br)
        enc = h264mi.BatchEncoder(w, h, br, 1)
        enc.encode(torch.full((w * h * 3 // 2,), 128, dtype=torch.uint8).cuda())
        assert enc.nal_sizes()[0] > 0
        st = enc.rc_state(0)
        q = p['init_qp']
        want = (q, max(q - 3, p['idr_lo']), min(q + 3, p['idr_hi']), p['bpf'])
        assert (st['qp'], st['min_qp'], st['max_qp'], st['bpf']) == want, (w, h, br, st, p)
        enc.close()


@pytest.mark.parametrize('which', ['p', 'idr'])
def test_long_runs(gpu_lib, oracle, which):
    """33 000 static P frames / 300 forced IDRs at 16x16: bytes and rc_state == the oracle's in the windows around
    pframe_num / idr_num 254 and the frame_num wrap; the steps between the windows are not waited for. The oracle
    decoder and decode_frame_yuv_i420 decode the stream across the wrap."""
    import torch
    import h264mi
    s = rcaudit.long_runs()[which]
    windows = rcaudit.LONG_WINDOWS[which]
    keep = {t for w in windows for t in w}
    last = max(keep)
    head = rcaudit.Seq(s.w, s.h, s.br, s.skip, s.schedule[:last + 1], [t for t in s.idr if t <= last])
    run = rcaudit.oracle_run(oracle, head)
    enc = h264mi.BatchEncoder(s.w, s.h, s.br, 1)
    enc.set_frame_skip(False)
    dev = torch.from_numpy(s.frame(0)).cuda()
    for t in range(last + 1):
        if t in s.idr:
            enc.force_idr(0)
        enc.encode(dev)
        if t in keep:
            n = enc.nal_sizes()[0]
            assert enc.nal_bytes(0, n) == run[t][0], (which, t)
            assert enc.rc_state(0) == run[t][1], (which, t, enc.rc_state(0), run[t][1])
    enc.close()
    if which != 'p':
        return
    od = oracle.decoder()
    flat = s.frame(0)
    for t in range(last + 1):
        rc, pic, dw, dh = od.decode(run[t][0])
        assert rc == 1 and np.array_equal(pic, flat), t
    # the GPU decoder: the IDR, then the access units on both sides of the wrap. Every P picture here is P_Skip over a flat
    # reference, so what is checked is that frame_num 32767 -> 0 is taken as the next picture and not as a loss
    L = gpu_lib
    assert L.init_decoder(0) == 0
    out = np.zeros(flat.size, np.uint8)
    gw, gh = ctypes.c_int(), ctypes.c_int()
    for t in [0] + list(range(32760, 32776)):
        nal = np.frombuffer(run[t][0], np.uint8).copy()
        out[:] = 0  # every picture is the same flat frame: what compares equal below was written by this call
        L.decode_frame_yuv_i420(0, nal.ctypes.data, len(nal), out.ctypes.data, ctypes.byref(gw), ctypes.byref(gh))
        if t == 0 or t > 32760:  # frame 32760 follows the IDR across a gap: only the pictures after it are held to the source
            assert (gw.value, gh.value) == (s.w, s.h) and np.array_equal(out, flat), t
    L.deinit_decoder(0)


def test_failed_frame_leaves_the_state_of_design_3_10(gpu_lib):
    """inject_error on a P frame: the begin kernel's picture init stands (VGOP index, weights, target, QP, window, the
    preprocessing's reference picture), the update is not made, the next frame is an IDR; rc_state == the model run that
    way on the failed frame and on the two frames after it"""
    import torch
    import h264mi
    s = rcaudit.Seq(48, 48, 100000, False, 'nnnnnn', (), 21)
    enc = h264mi.BatchEncoder(s.w, s.h, s.br, 1)
    enc.set_frame_skip(False)
    m = rcref.PyRc(s.w, s.h, s.br, False)
    for t in range(len(s)):
        if t == 3:
            enc.inject_error(0, 3)
        f = s.frame(t)
        enc.encode(torch.from_numpy(f).cuda())
        assert m.begin(f)
        if t == 3:
            out = (ctypes.c_int * 1)()
            assert enc._L.h264mi_enc_nal_bytes(enc._e, out) == -2 and out[0] == 0
            m.fail()
        else:
            n = enc.nal_sizes()[0]
            nal = enc.nal_bytes(0, n)
            assert (nal[4] & 31 == 7) == (t in (0, 4)), t  # an access unit that starts with an SPS: frame 0 and the frame after the failure
            m.end(nal, enc.rc_state(0)['avg_qp'], _coded(enc, 0))
        got, want = enc.rc_state(0), m.state()  # the failed frame's average QP is the frame's before: no update wrote it
        assert got == want, (t, got, want)
    assert m.counts['VGOP_BY_IDR_CARRY_NEG'] + m.counts['VGOP_BY_IDR_CARRY_ZERO'] == 2
    enc.close()
