#!/usr/bin/env python3
"""The scene-cut detector (h264mi.i420_scenecut, csrc/scenecut.hip) and the key-frame policy measured two ways. The
tables assert nothing.

(a) timing, at 128 frames 1920x1080: the detector as the encoder runs it (statistics, thumbnails advanced in place: one
memset and one launch) against the denoiser as the encoder runs it (dst = cur, dst2 = prev: one launch) on the same
frames. Each sample is one window of calls between two device events; the two alternate, sample by sample, in the same
run. Reported: the median, minimum and maximum time of one call, GB/s from the call's algorithmic bytes (detector: one
luma plane read, 1/16 of it read and written; denoiser: two frames read, two written), and that as a share of a
device-to-device copy's rate measured in the same run, and of the 6.29 TB/s a float4 copy reaches on this chip. One frame
is compared against tests/scenecutref.py first.

(a2) the detector and the decision as an encoder step pays for them: one encoder of 128 streams 1920x1080 coding its own
input area (a still picture, frame skipping off, so that every step does the same work), with the policy off, period
only (share 0: the decision kernel alone) and the documented default (detector and decision). The three settings
alternate window by window in the same run, timed by events on the encoder's stream; the differences of the medians
are the cost per step, beside the spread of the step itself.

(b) effect: stream 0 of the benchmark's synthetic clip at 1920x1080 (its window wraps at frame 22: a scene change),
coded at the benchmark's bitrate with the policy off and with the documented default; frame skipping off (with it on,
one stream at this bitrate skips every frame behind the first). Reported per frame 20..30: bytes, luma PSNR
(h264mi_enc_set_quality), whether it is an IDR, enc_mb_kernel's time, and the changed blocks the detector counted.

Writes scenecut_ab.json and scenecut_ab.md into --out.

    python tools/scenecut_ab.py --out profiles/scenecut
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'openh264-wasm_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
N, W, H = 128, 1920, 1080
DENOISE = (128, 64, 12, 24)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=10, help='calls per timed window')
    ap.add_argument('--repeats', type=int, default=21, help='timed windows per version')
    ap.add_argument('--warmup', type=int, default=2, help='untimed windows per version')
    ap.add_argument('--frames', type=int, default=31, help='frames of the effect run')
    ap.add_argument('--bitrate', type=int, default=1000000, help="the benchmark's default")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scenecut'))
    a = ap.parse_args()
    import numpy as np
    import torch
    import h264mi
    import scenecutref as ref
    from h264mi.synth import SyntheticStream
    if not torch.cuda.is_available():
        raise SystemExit('scenecut_ab.py measures on the GPU: no device found')
    hip = h264mi._hiprt()
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    params = h264mi.SCENECUT_DEFAULT

    def window(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls  # ms per call

    def stats(v, nbytes):
        med = statistics.median(v)
        return {'median_ms': med, 'min_ms': min(v), 'max_ms': max(v), 'bytes_per_call': nbytes, 'gbps': nbytes / (med * 1e-3) / 1e9}

    res = {'calls_per_window': a.calls, 'windows': a.repeats, 'device': torch.cuda.get_device_name(0), 'params': list(params),
           'denoise_params': list(DENOISE), 'what': f'{N} frames {W}x{H}'}
    fb = ref.frame_bytes(W, H)
    tw, th = ref.thumb_size(W, H)
    prev = torch.randint(0, 256, (N, fb), dtype=torch.uint8, device='cuda')
    cur = (prev.to(torch.int16) + torch.randint(-5, 6, (N, fb), dtype=torch.int16, device='cuda')).clamp(0, 255).to(torch.uint8)
    state = prev.clone()
    thumbs = torch.zeros(N * tw * th, dtype=torch.uint8, device='cuda')
    words = torch.zeros(8 * N, dtype=torch.int32, device='cuda')
    big = torch.zeros((2, 2 * N * fb), dtype=torch.uint8, device='cuda')
    stream = h264mi._hip_stream(None)
    h264mi.i420_scenecut(prev, W, H, N, params, thumb_out=thumbs)
    tp = thumbs[(N - 1) * tw * th:].cpu().numpy().reshape(th, tw).copy()

    def detect():
        h264mi.i420_scenecut(cur, W, H, N, params, thumb_out=thumbs, thumb_prev=thumbs, stats=words)

    def denoise():
        h264mi.i420_denoise(cur, cur, state, W, H, N, DENOISE, dst2=state)

    def copy():
        hip.hipMemcpyAsync(ctypes.c_void_p(big[1].data_ptr()), ctypes.c_void_p(big[0].data_ptr()), big[0].numel(), 3, stream)

    detect()
    torch.cuda.synchronize()
    tc = ref.thumbnail(cur[N - 1].cpu().numpy(), W, H)
    assert np.array_equal(thumbs[(N - 1) * tw * th:].cpu().numpy().reshape(th, tw), tc), 'kernel != tests/scenecutref.py'
    assert words[8 * (N - 1):].cpu().numpy().view(np.uint32).tolist() == ref.frame_stats(tc, tp, params), 'kernel != tests/scenecutref.py'
    nbytes = {'detector': N * (W * H + 2 * tw * th), 'denoiser': 4 * N * fb, 'copy': 4 * N * fb}
    runs = (('detector', detect), ('denoiser', denoise), ('copy', copy))
    for _ in range(a.warmup):
        for k, fn in runs:
            window(fn, a.calls)
    t = {k: [] for k, _ in runs}
    for _ in range(a.repeats):  # alternate
        for k, fn in runs:
            t[k].append(window(fn, a.calls))
    res['timing'] = {k: stats(t[k], nbytes[k]) for k, _ in runs}
    for k in ('detector', 'denoiser'):
        res['timing'][k]['share_of_copy_rate'] = res['timing'][k]['gbps'] / res['timing']['copy']['gbps']
    res['timing']['detector_over_denoiser_time'] = res['timing']['detector']['median_ms'] / res['timing']['denoiser']['median_ms']
    res['timing']['detector']['share_of_measured_hbm_copy_peak'] = res['timing']['detector']['gbps'] / 6290.0
    del prev, cur, state, big
    torch.cuda.empty_cache()

    # (a2) encoder steps
    est = torch.cuda.Stream()  # the encoder's stream: the windows' events are recorded on it
    enc = h264mi.BatchEncoder(W, H, a.bitrate, N, stream=est)
    enc.set_frame_skip(False)
    src = enc._L.h264mi_enc_input_buffer(enc._e)
    still = torch.from_numpy(np.ascontiguousarray(SyntheticStream(0, W, H).frame(0)).ravel()).cuda().repeat(N)
    hip.hipMemcpyAsync(ctypes.c_void_p(src), ctypes.c_void_p(still.data_ptr()), still.numel(), 3, stream)
    torch.cuda.synchronize()

    def step():
        if enc._L.h264mi_enc_encode(enc._e, ctypes.c_void_p(src)) != 0:
            raise RuntimeError('h264mi_enc_encode failed')

    settings = (('off', None), ('period only', (0, 0, 0, 65535, 0)), ('default', params))
    ts = {k: [] for k, _ in settings}
    for r in range(a.warmup + a.repeats):
        for k, p in settings:
            enc.set_scenecut(p)
            step()  # untimed: the first frame of a setting only stores thumbnails
            torch.cuda.synchronize()
            with torch.cuda.stream(est):
                v = window(step, a.calls)
            enc.nal_sizes()  # raises if a kernel reported an error
            if r >= a.warmup:
                ts[k].append(v)
    enc.close()
    med = {k: statistics.median(v) for k, v in ts.items()}
    res['encoder_step'] = {'what': f'{N} streams {W}x{H}, still picture, {a.calls} steps a window, {a.repeats} windows a setting',
                           'settings': {k: {'median_ms': med[k], 'min_ms': min(v), 'max_ms': max(v)} for k, v in ts.items()},
                           'decision_ms': med['period only'] - med['off'], 'detector_and_decision_ms': med['default'] - med['off']}

    g = SyntheticStream(0, W, H)
    res['effect'] = {}
    for name, setting in (('off', None), ('on', params)):
        enc = h264mi.BatchEncoder(W, H, a.bitrate, 1)
        enc.set_frame_skip(False)
        enc.set_quality(True)
        enc.set_timing(True)
        enc.set_scenecut(setting)
        rows = []
        for f in range(a.frames):
            frames = torch.from_numpy(np.ascontiguousarray(g.frame(f)).ravel()).cuda()
            ms0, _ = enc.kernel_time()
            enc.encode(frames)
            size = enc.nal_sizes()[0]
            ms1, _ = enc.kernel_time()
            q = enc.quality(0)
            nal = enc.nal_bytes(0, size) if size > 0 else b''
            b = np.frombuffer(nal, np.uint8)
            idr = any(b[i] == 0 and b[i + 1] == 0 and b[i + 2] == 1 and (b[i + 3] & 31) == 5 for i in range(max(len(b) - 3, 0)))
            rows.append({'frame': f, 'bytes': size, 'psnr_y': (q['psnr'] or [None])[0], 'idr': bool(idr), 'enc_mb_ms': ms1 - ms0,
                         'state': enc.scenecut_state(0) if setting else None})
        enc.close()
        res['effect'][name] = rows

    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'scenecut_ab.json'), 'w') as f:
        json.dump(res, f, indent=1)
    T = res['timing']
    lines = [f'(a) timing: {res["what"]}, {a.repeats} windows per version ({a.calls} calls a window), alternating; {res["device"]}; parameters {tuple(params)}', '',
             '| version | median ms | min ms | max ms | algorithmic GB | GB/s | of the copy\'s rate |', '|---|---|---|---|---|---|---|']
    for k in ('detector', 'denoiser', 'copy'):
        x = T[k]
        share = f'{100 * x["share_of_copy_rate"]:.0f} %' if k != 'copy' else ''
        lines.append(f'| {k} | {x["median_ms"]:.4f} | {x["min_ms"]:.4f} | {x["max_ms"]:.4f} | {x["bytes_per_call"] / 1e9:.3f} | {x["gbps"]:.0f} | {share} |')
    lines += ['', f'The detector takes {100 * T["detector_over_denoiser_time"]:.0f} % of the denoiser\'s time on the same frames. (detector: one memset and one launch, '
              'luma read once, thumbnails read and written in place; denoiser: dst = cur, dst2 = prev; copy: one device-to-device hipMemcpyAsync that reads '
              'and writes two frame-sizes per frame. No hardware counter was collected.)', '',
              f'(a2) encoder step, {res["encoder_step"]["what"]}', '', '| policy | median ms | min ms | max ms |', '|---|---|---|---|'] + [
              f'| {k} | {x["median_ms"]:.4f} | {x["min_ms"]:.4f} | {x["max_ms"]:.4f} |' for k, x in res['encoder_step']['settings'].items()] + [
              '', f'Differences of the medians: the decision kernel {1000 * res["encoder_step"]["decision_ms"]:.1f} us a step, the detector and the decision '
              f'{1000 * res["encoder_step"]["detector_and_decision_ms"]:.1f} us a step. The detector alone reaches '
              f'{100 * T["detector"]["share_of_measured_hbm_copy_peak"]:.0f} % of the 6.29 TB/s of a float4 copy (bandwidth-bound: one byte read per sample).', '',
              f'(b) effect: stream 0 of the synthetic clip at {W}x{H}, {a.bitrate} bit/s, policy off and {tuple(params)}', '',
              '| frame | bytes off | bytes on | PSNR-Y off | PSNR-Y on | IDR off | IDR on | enc_mb ms off | enc_mb ms on | changed / blocks |', '|---|---|---|---|---|---|---|---|---|---|']
    fmt = lambda v: 'skipped' if v is None else f'{v:.2f}'
    for off, on in zip(res['effect']['off'], res['effect']['on']):
        if off['frame'] >= 20:
            lines.append(f'| {off["frame"]} | {off["bytes"]} | {on["bytes"]} | {fmt(off["psnr_y"])} | {fmt(on["psnr_y"])} | {int(off["idr"])} | {int(on["idr"])} | '
                         f'{off["enc_mb_ms"]:.3f} | {on["enc_mb_ms"]:.3f} | {on["state"]["stats"][0]} / {on["state"]["stats"][1]} |')
    text = '\n'.join(lines) + '\n'
    with open(os.path.join(a.out, 'scenecut_ab.md'), 'w') as f:
        f.write(text)
    print(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
