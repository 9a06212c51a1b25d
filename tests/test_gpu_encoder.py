"""GPU: encoder parity through the C-ABI (init_encoder / force_key_frame / encode_frame_yuv_i420 /
encode_frame): Annex-B bytes identical to the oracle's on the same seeded input, frame by frame;
and identical to the committed fixture digests."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import encaudit
from golden.make_golden import CASES, case_inputs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FX = {c['name']: c for c in json.load(open(os.path.join(HERE, 'golden', 'oracle_fixtures.json')))['cases']}


def gpu_encode(L, frame, w, h, rgba=None):
    p = ctypes.POINTER(ctypes.c_ubyte)()
    sz = ctypes.c_int(0)
    if rgba is not None:
        L.encode_frame(rgba.ctypes.data, w, h, ctypes.byref(p), ctypes.byref(sz))
    else:
        L.encode_frame_yuv_i420(frame.ctypes.data, w, h, ctypes.byref(p), ctypes.byref(sz))
    return ctypes.string_at(p, sz.value) if sz.value > 0 else b''


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_encoder_matches_oracle_and_fixture(gpu_lib, oracle, case):
    name, w, h, br, n, force_every, kind = case
    L = gpu_lib
    frames, rgbas = case_inputs(oracle, w, h, n, kind)
    assert L.init_encoder(w, h, br) == 0
    oe = oracle.encoder(w, h, br)
    ex = encaudit.Explainer(oracle, oe, name)  # a mismatch names the first differing macroblock
    for t in range(n):
        if force_every and t % force_every == 0 and t > 0:
            L.force_key_frame()
            oe.force_idr()
        got = gpu_encode(L, frames[t], w, h, rgbas[t] if rgbas is not None else None)
        ref = oe.encode(frames[t])
        ex.check(t, got, ref)
        if not ref:  # skipped by both rate controls
            assert FX[name]['nal_sha256'][t] is None
            continue
        assert hashlib.sha256(got).hexdigest() == FX[name]['nal_sha256'][t]


def test_encoder_1080p_ippp_fixture_free(gpu_lib, oracle):
    """config 3 slice: 1920x1080 IPPP, 3 frames at 20 Mbps, GPU bytes == oracle bytes: the IDR, frame 1 skipped
    (the VBV check after the IDR's overspend, RcVBufferCalculationSkip), frame 2 a coded P frame"""
    from h264mi.synth import SyntheticStream
    w, h = 1920, 1080
    L = gpu_lib
    assert L.init_encoder(w, h, 20000000) == 0
    oe = oracle.encoder(w, h, 20000000)
    g = SyntheticStream(0, w, h)
    for t in range(3):
        f = np.ascontiguousarray(g.frame(t))
        got = gpu_encode(L, f, w, h)
        assert (len(got) > 0) == (t != 1), t
        assert got == oe.encode(f), t


def test_encoder_rejects_bad_geometry(gpu_lib):
    L = gpu_lib
    assert L.init_encoder(176, 144, 300000) == 0
    f = np.zeros(176 * 144 * 3 // 2, np.uint8)
    p = ctypes.POINTER(ctypes.c_ubyte)()
    sz = ctypes.c_int(123)
    L.encode_frame_yuv_i420(f.ctypes.data, 352, 288, ctypes.byref(p), ctypes.byref(sz))  # wrong size
    assert sz.value == 0 and not p
    assert L.init_encoder(0, 144, 300000) == -1
