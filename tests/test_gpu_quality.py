"""GPU: per-frame SSE / SSIM records (h264mi_quality) -- the standalone call on pairs of I420 frames and the
encoder's own records -- against tests/qualityref.py. The definition is integer arithmetic plus correctly rounded
double operations, so every comparison is exact equality."""
import ctypes
import functools

import numpy as np
import pytest

import qualityref

pytestmark = pytest.mark.gpu

KEYS = ('sse', 'ssim_fix', 'windows', 'coded')


def _rec(q):
    """the exact fields of a record (a Quality structure or BatchEncoder.quality()'s dict)"""
    if isinstance(q, dict):
        return {k: q[k] for k in KEYS}
    return {'sse': [int(v) for v in q.sse], 'ssim_fix': [int(v) for v in q.ssim_fix], 'windows': [int(v) for v in q.windows],
            'coded': int(q.coded)}


def _pairs(w, h, n, seed, amp=12):
    """n random frames and the same frames plus noise of at most +-amp, clipped"""
    rng = np.random.default_rng(seed)
    fb = w * h + 2 * (w // 2) * (h // 2)
    a = rng.integers(0, 256, (n, fb), dtype=np.uint8)
    b = np.clip(a.astype(np.int32) + rng.integers(-amp, amp + 1, a.shape), 0, 255).astype(np.uint8)
    return a, b


def _device(x, shift=0):
    """x's bytes on the device, `shift` bytes into a larger allocation"""
    import torch
    whole = torch.zeros(x.size + shift + 64, dtype=torch.uint8, device='cuda')
    view = whole[shift:shift + x.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(x).ravel()))
    return view


def _standalone(a, b, w, h, n, shift=0):
    import torch
    import h264mi
    out = torch.full((8 * n,), -1, dtype=torch.int64, device='cuda')  # the call clears it
    da, db = _device(a, shift), _device(b, shift)
    if shift:
        assert da.data_ptr() % 2 == 1 and db.data_ptr() % 2 == 1
    h264mi.i420_quality(out, da, db, w, h, n)
    recs = h264mi.quality_records(out, n)
    assert all(r.reserved == 0 for r in recs)
    return [_rec(r) for r in recs], out.cpu().numpy().tobytes()


# 16x16: one chroma window; 36x18: w % 8 != 0, chroma 18x9 with samples outside every window; 38x22: rows that are no
# multiple of 4 bytes; 176x144: several row segments; the same at an odd address; 256x24 and 508x40: more than one
# 64-column strip per wave row (a strip of a single column; chroma 254 wide: 63 blocks and a 2-sample tail)
STANDALONE = [(16, 16, 0), (36, 18, 0), (38, 22, 0), (176, 144, 0), (176, 144, 1), (256, 24, 0), (508, 40, 0)]


@pytest.mark.parametrize('w,h,shift', STANDALONE, ids=[f'{c[0]}x{c[1]}' + ('-odd-address' if c[2] else '') for c in STANDALONE])
def test_standalone_vs_reference(gpu_lib, w, h, shift):
    n = 3
    a, b = _pairs(w, h, n, 1000 + w + h)
    got, _ = _standalone(a, b, w, h, n, shift)
    for f in range(n):
        assert got[f] == qualityref.frame_quality(a[f], b[f], w, h), f'pair {f}'


def test_sse_needs_64_bits(gpu_lib):
    w, h = 352, 288
    fb = w * h * 3 // 2
    a, b = np.zeros((1, fb), np.uint8), np.full((1, fb), 255, np.uint8)
    got, _ = _standalone(a, b, w, h, 1)
    assert got[0]['sse'][0] == 352 * 288 * 65025 == 6591974400 and got[0]['sse'][0] > 1 << 32
    assert got[0]['sse'][1] == got[0]['sse'][2] == 176 * 144 * 65025
    assert got[0] == qualityref.frame_quality(a[0], b[0], w, h)


def test_identical_frames_and_repeatability(gpu_lib):
    w, h = 176, 144
    a, _ = _pairs(w, h, 2, 5)
    got, raw = _standalone(a, a.copy(), w, h, 2)
    for r in got:
        assert r['sse'] == [0, 0, 0] and r['coded'] == 1
        assert r['windows'] == [43 * 35, 21 * 17]
        assert r['ssim_fix'] == [r['windows'][0] << 32, r['windows'][1] << 32, r['windows'][1] << 32]
    a, b = _pairs(w, h, 2, 6)
    _, raw1 = _standalone(a, b, w, h, 2)
    _, raw2 = _standalone(a, b, w, h, 2)
    assert raw1 == raw2


def test_standalone_bad_arguments(gpu_lib):
    import torch
    L = gpu_lib
    o = torch.zeros(64, dtype=torch.int64, device='cuda')
    a = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    po, pa = ctypes.c_void_p(o.data_ptr()), ctypes.c_void_p(a.data_ptr())
    fn = L.h264mi_i420_quality_dev
    assert fn(po, pa, pa, 16, 16, 1, None) == 0
    for w, h, n in ((15, 16, 1), (16, 15, 1), (14, 16, 1), (16, 14, 1), (16, 16, 0), (16, 16, -1)):
        assert fn(po, pa, pa, w, h, n, None) == -1
    assert fn(None, pa, pa, 16, 16, 1, None) == -1 and fn(po, None, pa, 16, 16, 1, None) == -1 and fn(po, pa, None, 16, 16, 1, None) == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the encoder's records


def _crop_frame(buf, cw, ch, w, h):
    """tight w x h I420 from contiguous coded-size planes"""
    y = buf[:cw * ch].reshape(ch, cw)[:h, :w]
    u = buf[cw * ch:cw * ch * 5 // 4].reshape(ch // 2, cw // 2)[:h // 2, :w // 2]
    v = buf[cw * ch * 5 // 4:cw * ch * 3 // 2].reshape(ch // 2, cw // 2)[:h // 2, :w // 2]
    return np.concatenate([y.ravel(), u.ravel(), v.ravel()])


def _recon(enc, s):
    import h264mi
    cw, ch = (enc.w + 15) // 16 * 16, (enc.h + 15) // 16 * 16
    buf = np.empty(cw * ch * 3 // 2, np.uint8)
    h264mi._hip_memcpy_d2h(buf.ctypes.data, enc.recon_ptr(s), buf.size)
    return _crop_frame(buf, cw, ch, enc.w, enc.h)


def _sizes(enc):
    """NAL byte counts, also of a step in which a stream failed (h264mi_enc_nal_bytes returns -2 then)"""
    out = (ctypes.c_int * enc.S)()
    assert enc._L.h264mi_enc_nal_bytes(enc._e, out) in (0, -2)
    return list(out)


@functools.lru_cache(maxsize=None)
def _sources(w, h, S, nf):
    from h264mi.synth import SyntheticStream
    gs = [SyntheticStream(s, w, h) for s in range(S)]
    return [np.stack([np.ascontiguousarray(g.frame(t)) for g in gs]) for t in range(nf)]


def _run(w, h, br, S, nf, skip=False, quality=(), inject=None):
    """nf frame steps of S streams; quality: the steps during which the option is on; inject: {step: stream} to fail.
    Per step: the NAL bytes, rc_state, frames_skipped, and (while on) the records and the reconstructions."""
    import torch
    import h264mi
    src = _sources(w, h, S, nf)
    enc = h264mi.BatchEncoder(w, h, br, S)
    enc.set_frame_skip(skip)
    assert not enc.quality_enabled() and enc.quality_ptr() is None
    steps = []
    for t in range(nf):
        enc.set_quality(t in quality)
        if inject and t in inject:
            enc.inject_error(inject[t])
        frames = torch.from_numpy(src[t].ravel()).cuda()  # held until _sizes() has synchronised
        enc.encode(frames)
        sizes = _sizes(enc)
        st = {'nal': [enc.nal_bytes(s, sizes[s]) if sizes[s] > 0 else b'' for s in range(S)],
              'rc': [enc.rc_state(s) for s in range(S)], 'skipped': [enc.frames_skipped(s) for s in range(S)]}
        if t in quality:
            assert enc.quality_enabled() and enc.quality_ptr()
            st['q'] = [enc.quality(s) for s in range(S)]
            st['recon'] = [_recon(enc, s) for s in range(S)]
        else:
            assert enc.quality_ptr() is None
            with pytest.raises(RuntimeError):
                enc.quality(0)
        steps.append(st)
    enc.close()
    return src, steps


def _nal_types(nal):
    b = bytes(nal)
    return [b[i + 3] & 31 for i in range(len(b) - 3) if b[i:i + 3] == b'\x00\x00\x01']


@pytest.mark.parametrize('w,h', [(176, 144), (72, 40)], ids=['qcif', 'cropped-72x40'])
def test_encoder_records_vs_reference_and_option_is_free(gpu_lib, w, h):
    S, nf, br = 2, 4, 300000
    src, on = _run(w, h, br, S, nf, quality=range(nf))
    _, off = _run(w, h, br, S, nf)
    for t in range(nf):
        for s in range(S):
            assert len(on[t]['nal'][s]) > 0
            q = on[t]['q'][s]
            want = qualityref.frame_quality(src[t][s], on[t]['recon'][s], w, h)
            assert _rec(q) == want, f'frame {t} stream {s}'
            assert want['sse'][0] > 0 and q['psnr'][0] == pytest.approx(10 * np.log10(65025 * w * h / want['sse'][0]), abs=1e-9)
            assert 0 < q['ssim'][0] <= 1 and q['ssim'][0] == want['ssim_fix'][0] / (want['windows'][0] * 2.0 ** 32)
            assert on[t]['nal'][s] == off[t]['nal'][s], f'frame {t} stream {s}: NAL bytes differ with the option on'
            assert on[t]['rc'][s] == off[t]['rc'][s], f'frame {t} stream {s}: rate-control state differs'


def test_failed_frame_reports_nothing_coded(gpu_lib):
    w, h, S, nf = 176, 144, 2, 4
    src, st = _run(w, h, 300000, S, nf, quality=range(nf), inject={2: 1})
    assert st[2]['nal'][1] == b'' and len(st[2]['nal'][0]) > 0
    q = st[2]['q'][1]
    assert _rec(q) == qualityref.ZERO and q['psnr'] is None and q['ssim'] is None
    assert _rec(st[2]['q'][0]) == qualityref.frame_quality(src[2][0], st[2]['recon'][0], w, h)
    assert 5 in _nal_types(st[3]['nal'][1]) and 5 not in _nal_types(st[3]['nal'][0])  # the step after it: an IDR
    for s in range(S):
        assert _rec(st[3]['q'][s]) == qualityref.frame_quality(src[3][s], st[3]['recon'][s], w, h)


def test_skipped_frames_report_nothing_coded(gpu_lib):
    w, h, S, nf = 176, 144, 2, 8
    src, st = _run(w, h, 20000, S, nf, skip=True, quality=range(nf))
    prev = [0] * S
    for t in range(nf):
        for s in range(S):
            skipped = st[t]['skipped'][s] > prev[s]
            assert (st[t]['q'][s]['coded'] == 0) == skipped, f'frame {t} stream {s}'
            assert skipped == (st[t]['nal'][s] == b'')
            if skipped:
                assert _rec(st[t]['q'][s]) == qualityref.ZERO
            else:
                assert _rec(st[t]['q'][s]) == qualityref.frame_quality(src[t][s], st[t]['recon'][s], w, h)
        prev = st[t]['skipped']


def test_decoded_pictures_give_the_encoders_records(gpu_lib):
    import torch
    import h264mi
    w, h, nf = 176, 144, 3
    fb = w * h * 3 // 2
    src, st = _run(w, h, 300000, 1, nf, quality=range(nf))
    nals = [torch.from_numpy(np.frombuffer(st[t]['nal'][0], np.uint8).copy()).cuda() for t in range(nf)]
    dec = h264mi.BatchDecoder(w, h, 1, max_frames=nf)
    pics = torch.zeros(nf * fb, dtype=torch.uint8, device='cuda')
    got = torch.zeros(nf, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    dec.decode_frames([n.data_ptr() for n in nals], nal_sizes=[n.numel() for n in nals],
                      out_ptrs=[pics[t * fb:(t + 1) * fb].data_ptr() for t in range(nf)], got_ptrs=[got[t:t + 1].data_ptr() for t in range(nf)])
    torch.cuda.synchronize()
    assert got.cpu().tolist() == [1] * nf
    dec.close()
    out = torch.zeros(8 * nf, dtype=torch.int64, device='cuda')
    h264mi.i420_quality(out, torch.from_numpy(np.concatenate([src[t][0] for t in range(nf)])).cuda(), pics, w, h, nf)
    recs = h264mi.quality_records(out, nf)
    for t in range(nf):
        assert _rec(recs[t]) == _rec(st[t]['q'][0]), f'frame {t}'


def test_toggling_on_a_running_encoder(gpu_lib):
    w, h, S, nf = 176, 144, 2, 6
    src, tog = _run(w, h, 300000, S, nf, quality=(2, 3))  # _run checks that records exist exactly while it is on
    _, off = _run(w, h, 300000, S, nf)
    for t in range(nf):
        assert tog[t]['nal'] == off[t]['nal'], f'frame {t}'
        assert ('q' in tog[t]) == (t in (2, 3))
    for t in (2, 3):
        for s in range(S):
            assert _rec(tog[t]['q'][s]) == qualityref.frame_quality(src[t][s], tog[t]['recon'][s], w, h)


def test_small_encoders_refuse(gpu_lib):
    import h264mi
    enc = h264mi.BatchEncoder(8, 8, 100000, 1)
    with pytest.raises(ValueError):
        enc.set_quality(True)
    assert not enc.quality_enabled()
    enc.close()
