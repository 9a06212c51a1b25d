"""CPU: OpenH264's frame-level rate control (RC_BITRATE_MODE at the wrapper's parameters) as the oracle restates it
from the reference's h264.wasm, against a second, independent restatement in Python that reads
every constant and table from tests/golden/openh264_tables.json (cut from the wasm bytes by tools/wasm_tables.py):

* RcConvertQStep2Qp with musl's logf (func 483): the oracle's C, this file's numpy float64 / float32 version, and
  the product's device thresholds (libh264mi h264mi_rc_qstep_to_qp, a host function -- no GPU needed) agree on
  every QStep up to 400000;
* the frame-level state machine -- the skip decision with its run cap (func 589 / 1258), post-skip bookkeeping
  (func 1254), the VGOP allocation and picture QP (func 1226), the R-Q model updates (funcs 1218 / 676) and the
  VBV skip check -- driven by the oracle encoder's per-frame slice sizes, average QPs and frame complexities on
  real content, at 1080p 1 / 8 Mbps with skipping on and off, must give the oracle's skip decisions, QPs, QP
  windows, target bits, remaining bits, buffer fullness and run counts frame by frame.
Parity with OpenH264 itself: the functions are restated from its compiled code (no OpenH264 output exists here)."""
import ctypes

import numpy as np
import pytest

from rcref import T, PyRc, py_logf, py_qstep2qp, slice_bytes  # the model lives in tests/rcref.py


def test_logf_restatement(oracle):
    """the oracle's logf == this file's restatement bit for bit, and both within an ULP of the true log"""
    rng = np.random.default_rng(3)
    xs = np.concatenate([np.float32(rng.uniform(0.5, 5e6, 3000)), np.float32([1.0, 0.64, 2.0, 100.0])])
    for x in xs:
        a = np.float32(oracle.L.h264o_logf(float(x)))
        assert a == py_logf(x), x
        assert abs(float(a) - np.log(float(x))) <= 2 * np.spacing(np.float32(abs(a)) + np.float32(1e-30)), x


def test_qstep2qp_three_ways(oracle, libpath):
    """oracle (musl-logf form) == Python restatement == the product's thresholds, every QStep 0..400000"""
    lib = ctypes.CDLL(libpath)
    f_o, f_g = oracle.L.h264o_rc_qstep2qp, lib.h264mi_rc_qstep_to_qp
    f_g.argtypes = [ctypes.c_int]
    qs = np.arange(0, 400000)
    o = np.array([f_o(int(q)) for q in qs])
    g = np.array([f_g(int(q)) for q in qs])
    assert np.array_equal(np.minimum(o, 52), g)
    for q in list(range(0, 2000, 7)) + [2016, 22807, 24163, 24164, 399999]:
        assert py_qstep2qp(q) == o[q], q
    # the QStep table round trips: QP k's QStep converts back to k
    assert [int(o[v]) for v in T['rc_qstep']['values'][1:]] == list(range(1, 52))


@pytest.mark.parametrize('br,skip,force', [(1000000, True, 0), (8000000, True, 0), (1000000, False, 0),
                                           (8000000, False, 0), (8000000, True, 7)],
                         ids=['1m_skip', '8m_skip', '1m_noskip', '8m_noskip', '8m_skip_idr7'])
def test_frame_rc_state_machine_vs_python(oracle, br, skip, force):
    """the oracle's rate control on real 1080p content, frame by frame, == the Python restatement fed with the
    oracle's per-frame slice sizes, average QPs and frame complexities"""
    from h264mi.synth import SyntheticStream
    w, h, n = 1920, 1080, 45 if skip else 24
    g = SyntheticStream(1, w, h)
    oe = oracle.encoder(w, h, br)
    oe.set_frame_skip(skip)
    py = PyRc(w, h, br, skip)
    coded_p = 0
    for t in range(n):
        idr = t == 0 or (force and t % force == 0)
        if force and t % force == 0 and t > 0:
            oe.force_idr()
        nal = oe.encode(np.ascontiguousarray(g.frame(t)))
        st = oe.rc_state()
        skipped = py.judge_skip() and not idr
        assert skipped == bool(st['skipped']) == (len(nal) == 0), (t, st)
        if skipped:
            py.post_skip()
        else:
            py.picture_init(idr, st['cmplx'])
            assert (py.qp, py.min_qp, py.max_qp, py.target) == (st['qp'], st['min_qp'], st['max_qp'], st['target']), (t, st)
            py.picture_update(idr, slice_bytes(nal), st['avg_qp'], st['cmplx'])
            coded_p += not idr
        got = {'remaining': py.remaining, 'fullness': py.fullness, 'continual': py.continual,
               'skip_flag': int(py.skip_flag), 'remaining_weights': py.remaining_weights, 'coded_in_vgop': py.coded_in_vgop}
        assert got == {k: st[k] for k in got}, (t, got, st)
    assert coded_p > 0


def test_run_cap_codes_p_frames_at_the_wrappers_operating_point(oracle):
    """1080p at the wrapper's 1 Mbps with skipping on: the IDR fills the buffer, and the cap on the run of skipped
    frames (predicted skips >= the run) forces a P frame through after 39 skips (round 5's rule skipped all)"""
    from h264mi.synth import SyntheticStream
    w, h = 1920, 1080
    g = SyntheticStream(0, w, h)
    oe = oracle.encoder(w, h, 1000000)
    sizes = [len(oe.encode(np.ascontiguousarray(g.frame(t)))) for t in range(44)]
    assert sizes[0] > 0 and all(s == 0 for s in sizes[1:40]) and sizes[40] > 0, sizes
