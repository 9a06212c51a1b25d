"""GPU: the encoder's slices (h264mi_enc_set_slices / H264MI_ENC_SLICES): every picture coded as n
slices of whole MB rows. One checker for every case, per coded frame of every stream: the access unit holds exactly
n slice NAL units in order whose first_mb_in_slice follow the partition rule; the oracle decoder decodes it to the
encoder's own reconstruction bit for bit (which catches a wrong neighbour, nC, predicted Intra4x4 mode, MV predictor,
skip run, QP delta or deblocked edge at a slice edge); and the GPU decoder, fed on the device with 4 slice waves,
gives the same picture."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from test_syntax_streams import _split_nals

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _unescape(nal):
    """RBSP of one NAL unit (start code and header byte dropped, emulation prevention bytes removed)"""
    out, z = bytearray(), 0
    for b in nal[5:]:
        if z >= 2 and b == 3:
            z = 0
            continue
        out.append(b)
        z = z + 1 if b == 0 else 0
    return bytes(out)


def _ue(rbsp, pos=0):
    """(value, next bit position) of the ue(v) at bit pos"""
    bit = lambda p: (rbsp[p >> 3] >> (7 - (p & 7))) & 1
    lz = 0
    while bit(pos + lz) == 0:
        lz += 1
    v = 0
    for k in range(lz + 1):
        v = (v << 1) | bit(pos + lz + k)
    return v - 1, pos + 2 * lz + 1


def _crop(buf, cw, ch, w, h):
    y = buf[:cw * ch].reshape(ch, cw)[:h, :w]
    u = buf[cw * ch:cw * ch * 5 // 4].reshape(ch // 2, cw // 2)[:h // 2, :w // 2]
    v = buf[cw * ch * 5 // 4:].reshape(ch // 2, cw // 2)[:h // 2, :w // 2]
    return np.concatenate([y.ravel(), u.ravel(), v.ravel()])


def _check_syntax(unit, n, mbw, mbh, idr):
    import h264mi
    nals = _split_nals(unit)
    types = [x[4] & 31 for x in nals]
    if idr:
        assert types[:2] == [7, 8], types
        nals, types = nals[2:], types[2:]
    assert types == [5 if idr else 1] * n, (types, n)
    firsts = [_ue(_unescape(x))[0] for x in nals]
    assert firsts == [h264mi.slice_first_row(mbh, n, k) * mbw for k in range(n)], firsts
    return nals


class Checker:
    """the encoder `enc` (S streams of w x h), one oracle decoder per stream and one GPU decoder with 4 slice waves"""

    def __init__(self, enc, oracle, w, h, S):
        import h264mi
        self.enc, self.w, self.h, self.S = enc, w, h, S
        self.mbw, self.mbh = (w + 15) // 16, (h + 15) // 16
        self.ods = [oracle.decoder() for _ in range(S)]
        self.dec = h264mi.BatchDecoder(w, h, S)
        self.dec.set_slice_waves(4)

    def check(self, units, n, idr):
        """units: the access units of the frame just encoded (one per stream; every one coded)"""
        from h264mi import _hip_memcpy_d2h
        cw, ch = self.mbw * 16, self.mbh * 16
        self.dec.decode_dev(self.enc.nal_ptrs(), self.enc.nal_size_ptrs())
        rc, got = self.dec.status()
        assert rc == 0 and got == [1] * self.S, (rc, got)
        for s, u in enumerate(units):
            _check_syntax(u, n, self.mbw, self.mbh, idr)
            rc, pic, ow, oh = self.ods[s].decode(u)
            assert rc == 1 and (ow, oh) == (self.w, self.h), f'stream {s}: oracle decode rc {rc} {ow}x{oh}'
            buf = np.empty(cw * ch * 3 // 2, np.uint8)
            _hip_memcpy_d2h(buf.ctypes.data, self.enc.recon_ptr(s), buf.size)
            rec = _crop(buf, cw, ch, self.w, self.h)
            assert np.array_equal(rec, pic), f'stream {s}: {int(np.count_nonzero(rec != pic))} samples of the oracle picture != the reconstruction'
            gpu = np.frombuffer(self.dec.picture_i420(s), np.uint8)
            assert np.array_equal(gpu, pic), f'stream {s}: GPU decoder picture != oracle picture'

    def close(self):
        self.dec.close()


def _run(oracle, w, h, br, S, nf, plan, sid=0):
    """encode nf frames of S synthetic streams, frame skipping off; plan(t, enc) -> the slice count in force for frame
    t (it may call set_slices / force_idr first). Every frame of every stream goes through the checker."""
    import torch
    import h264mi
    from h264mi.synth import SyntheticStream
    gs = [SyntheticStream(sid + s, w, h) for s in range(S)]
    enc = h264mi.BatchEncoder(w, h, br, S)
    enc.set_frame_skip(False)
    ck = Checker(enc, oracle, w, h, S)
    sizes = []
    for t in range(nf):
        n, idr = plan(t, enc)
        enc.encode(torch.from_numpy(np.stack([np.ascontiguousarray(g.frame(t)) for g in gs])).cuda())
        nb = enc.nal_sizes()
        assert all(x > 0 for x in nb), (t, nb)
        units = [enc.nal_bytes(s, nb[s]) for s in range(S)]
        ck.check(units, n, idr)
        sizes.append(nb)
    ck.close()
    enc.close()
    return sizes


def _fixed(n):
    def plan(t, enc):
        if t == 0:
            enc.set_slices(n)
            assert enc.slices() == n
        return n, t == 0
    return plan


@pytest.mark.parametrize('n', [2, 3, 9])
def test_small_shapes(gpu_lib, oracle, n):
    """176x144 (11 x 9 MBs), IDR + 5 P: 3 slices of 3 rows, 2 uneven slices (4 and 5 rows), and 9 one-row slices (no
    row ever has a neighbour above). 600 kbps: the P frames carry residual."""
    _run(oracle, 176, 144, 600000, 1, 6, _fixed(n))


def test_cropped_uneven(gpu_lib, oracle):
    """640x360 (40 x 23 MBs, the last row cropped), 4 slices of 5, 6, 6 and 6 rows, IDR + 3 P"""
    _run(oracle, 640, 360, 2000000, 1, 4, _fixed(4), sid=3)


def test_1080p_8_slices(gpu_lib, oracle):
    """1920x1080 (120 x 68 MBs), 8 slices of 8 or 9 rows -- the shape the drop-in decoder's 8 slice waves meet"""
    _run(oracle, 1920, 1080, 8000000, 1, 3, _fixed(8))


def test_16_streams(gpu_lib, oracle):
    """16 streams of 352x288, 4 slices, IDR + 5 P (per-XCD ticket queues, two streams per queue)"""
    _run(oracle, 352, 288, 1000000, 16, 6, _fixed(4))


def test_changing_slice_count(gpu_lib, oracle):
    """176x144, IDR + 7 P: 1 slice for frames 0-1, 3 from frame 2 (a P frame with a new partition over a single-slice
    reference), 1 again from frame 5, a forced IDR of 2 slices at frame 6"""
    def plan(t, enc):
        if t == 2:
            enc.set_slices(3)
        if t == 5:
            enc.set_slices(1)
        if t == 6:
            enc.force_idr()
            enc.set_slices(2)
        n = 1 if t < 2 else 3 if t < 5 else 1 if t < 6 else 2
        assert enc.slices() == n
        return n, t in (0, 6)
    _run(oracle, 176, 144, 600000, 1, 8, plan)


def test_one_slice_is_todays_encoder(gpu_lib, oracle):
    """after an explicit set_slices(1) the bytes are the oracle encoder's, frame skipping on, frame by frame"""
    import torch
    import h264mi
    from h264mi.synth import SyntheticStream
    w, h, br = 176, 144, 300000
    g = SyntheticStream(0, w, h)
    enc = h264mi.BatchEncoder(w, h, br, 1)
    enc.set_slices(1)
    oe = oracle.encoder(w, h, br)
    for t in range(4):
        f = np.ascontiguousarray(g.frame(t))
        enc.encode(torch.from_numpy(f).cuda())
        n = enc.nal_sizes()[0]
        ref = oe.encode(f)
        assert n == len(ref) and (n == 0 or enc.nal_bytes(0, n) == ref), f'frame {t}'
    enc.close()


def test_rate_control_counts_every_slice(gpu_lib, oracle):
    """352x288, 4 slices: the frame's bits are the bytes of all its slice NAL units -- remaining bits (rc_state field
    4) drop by 8 x (access unit - SPS - PPS) on the IDR and by 8 x the access unit on a P frame of the same VGOP"""
    import torch
    import h264mi
    from h264mi.synth import SyntheticStream
    w, h, br = 352, 288, 1000000
    g = SyntheticStream(2, w, h)
    enc = h264mi.BatchEncoder(w, h, br, 1)
    enc.set_frame_skip(False)
    enc.set_slices(4)
    # The starting value of the IDR's check is not read back: the first IDR's picture init (enc_begin_stream:
    # RcInitRefreshParameter zeroes the remaining bits, then rc_init_vgop / OpenH264's RcInitVGop sets them to
    # bits per frame << 3) runs inside the first encode, so no state before it exists to read; bits per frame is a
    # creation-time constant (rc_seq_init, RcUpdateBitrateFps) that the frame's update does not touch.
    drops, units = [], []
    for t in range(3):
        enc.encode(torch.from_numpy(np.ascontiguousarray(g.frame(t))).cuda())
        n = enc.nal_sizes()[0]
        assert n > 0
        units.append(enc.nal_bytes(0, n))
        drops.append(enc.rc_state(0))
    nals = _split_nals(units[0])
    psets = sum(len(x) for x in nals if x[4] & 31 in (7, 8))
    assert len([x for x in nals if x[4] & 31 == 5]) == 4
    assert (drops[0]['bpf'] << 3) - drops[0]['remaining'] == 8 * (len(units[0]) - psets)
    for t in (1, 2):
        assert len(_split_nals(units[t])) == 4
        assert drops[t - 1]['remaining'] - drops[t]['remaining'] == 8 * len(units[t]), t
    enc.close()


def test_failed_frame_then_idr(gpu_lib, oracle):
    """176x144, 3 slices: a P frame failed through the pack's overflow branch gives 0 NAL bytes, and the next frame is
    an IDR of 3 slices that passes the checker (the oracle decoder starts afresh at it)"""
    import torch
    import h264mi
    from h264mi.synth import SyntheticStream
    w, h = 176, 144
    g = SyntheticStream(1, w, h)
    enc = h264mi.BatchEncoder(w, h, 600000, 1)
    enc.set_frame_skip(False)
    enc.set_slices(3)
    ck = Checker(enc, oracle, w, h, 1)
    for t in range(4):
        if t == 2:
            enc.inject_error(0, 3)
        enc.encode(torch.from_numpy(np.ascontiguousarray(g.frame(t))).cuda())
        if t == 2:
            with pytest.raises(RuntimeError):
                enc.nal_sizes()
            out = (ctypes.c_int * 1)()
            assert enc._L.h264mi_enc_nal_bytes(enc._e, out) == -2 and out[0] == 0
            continue
        n = enc.nal_sizes()[0]
        assert n > 0
        ck.check([enc.nal_bytes(0, n)], 3, t in (0, 3))
    ck.close()
    enc.close()


def test_arguments(gpu_lib):
    import h264mi
    enc = h264mi.BatchEncoder(176, 144, 300000, 1)  # 9 MB rows
    assert enc.slices() == 1
    for bad in (0, 33, 10, -1):
        with pytest.raises(ValueError):
            enc.set_slices(bad)
        assert enc.slices() == 1
    enc.set_slices(9)
    assert enc.slices() == 9
    with pytest.raises(RuntimeError):  # exact GOM rate control is a single-slice mode
        enc.set_gom_exact(True)
    enc.set_slices(1)
    enc.set_gom_exact(True)
    with pytest.raises(ValueError):
        enc.set_slices(2)
    assert enc.slices() == 1
    enc.set_gom_exact(False)
    enc.set_slices(2)
    assert enc.slices() == 2
    enc.close()
    big = h264mi.BatchEncoder(1920, 1080, 1000000, 1)  # 68 MB rows: the decoder's 32 slices bound it
    big.set_slices(32)
    with pytest.raises(ValueError):
        big.set_slices(33)
    big.close()


_DROPIN = r'''
import ctypes, os, sys
import numpy as np
sys.path.insert(0, os.path.join(sys.argv[1], 'openh264-wasm_amd'))
sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))
import torch
import h264mi
from h264mi.synth import SyntheticStream
from _oracle import Oracle
from test_gpu_enc_slices import _check_syntax
torch.cuda.set_device(0)
L = h264mi.lib()
od = Oracle(os.path.join(sys.argv[1], 'oracle', 'build', 'libh264_oracle.so')).decoder()
w, h = 1920, 1080
assert L.init_encoder(w, h, 8000000) == 0 and L.init_decoder(0) == 0
g = SyntheticStream(0, w, h)
out = np.zeros(w * h * 3 // 2, np.uint8)
coded = 0
for t in range(45):  # the drop-in keeps the wrapper's frame skipping: frames after the IDR are skipped (0 bytes) first
    f = np.ascontiguousarray(g.frame(t))
    p, sz = ctypes.POINTER(ctypes.c_ubyte)(), ctypes.c_int(0)
    L.encode_frame_yuv_i420(f.ctypes.data, w, h, ctypes.byref(p), ctypes.byref(sz))
    assert t > 0 or sz.value > 0
    if sz.value <= 0:
        continue
    coded += 1
    u = ctypes.string_at(p, sz.value)
    _check_syntax(u, 8, 120, 68, t == 0)
    rc, pic, ow, oh = od.decode(u)
    assert rc == 1 and (ow, oh) == (w, h)
    a = np.frombuffer(u, np.uint8).copy()
    gw, gh = ctypes.c_int(-1), ctypes.c_int(-1)
    L.decode_frame_yuv_i420(0, a.ctypes.data, len(u), out.ctypes.data, ctypes.byref(gw), ctypes.byref(gh))
    assert (gw.value, gh.value) == (w, h) and np.array_equal(out, pic), t
    if coded == 2:  # the IDR and one P frame
        break
assert coded == 2, coded
L.deinit_decoder(0)
print('dropin ok')
'''


def test_dropin_env_8_slices(gpu_lib, oracle, tmp_path):
    """H264MI_ENC_SLICES=8 in a fresh process: the nine drop-in functions code the 1080p IDR and a P frame as 8 slices
    each, and decode_frame_yuv_i420 (8 slice waves) gives the oracle decoder's pictures"""
    script = tmp_path / 'dropin_slices.py'
    script.write_text(_DROPIN)
    env = dict(os.environ, H264MI_ENC_SLICES='8')
    r = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'dropin ok' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
