#!/usr/bin/env python3
"""The deinterlacer (h264mi.i420_deinterlace, csrc/deinterlace.hip) measured. The table asserts nothing.

(a) the standalone call at 128 frames 1920x1080 and 8 frames 1920x1080, adaptive (edge-directed, temporal), in place
with state (dst = cur, prev = prev_out = the state: the encoder's form), without statistics:
  deint-moving : two buffers of random content taken in turn, so that every sample has moved: the whole rule runs
  deint-still  : the frames equal the state: every dword is woven (the m == 0 short cut)
  denoise      : the temporal denoiser in its encoder form (dst = cur, dst2 = prev) on frames near their state
  copy         : one device-to-device hipMemcpyAsync of 1.75 frame-sizes of bytes per frame, which reads and writes
                 the deinterlacer's algorithmic traffic: cur and the state read, the missing half of cur and the state
                 written = 3.5 frame-sizes
Each sample is one window of calls between two device events; the versions alternate, sample by sample, in the same
run. Reported: the median, minimum and maximum time of one call, GB/s from each version's own algorithmic bytes (the
denoiser: two frames read, two written), and that as a share of the copy's rate. One frame is compared with
tests/deintref.py first.

(b) an encoder step (encode() + the wait for its NAL sizes) of 8 streams 1920x1080 with the filter off and on, two
encoders fed the same woven frames in alternating windows; host clock, since the step ends in a synchronise.

Writes deint_ab.json and deint_ab.md into --out.

    python tools/deint_ab.py --out profiles/deinterlace
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'openh264-wasm_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
TIMING = (('batch', 128, 1920, 1080), ('few', 8, 1920, 1080))
PARAMS = (0, 1, 1, 8)
DENOISE = (128, 64, 12, 24)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=10, help='calls per timed window')
    ap.add_argument('--repeats', type=int, default=21, help='timed windows per version')
    ap.add_argument('--warmup', type=int, default=2, help='untimed windows per version')
    ap.add_argument('--steps', type=int, default=6, help='encoder steps per timed window')
    ap.add_argument('--bitrate', type=int, default=1000000, help="the benchmark's default")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'deinterlace'))
    a = ap.parse_args()
    import numpy as np
    import torch
    import h264mi
    import deintref
    from h264mi.synth import SyntheticStream
    if not torch.cuda.is_available():
        raise SystemExit('deint_ab.py measures on the GPU: no device found')
    hip = h264mi._hiprt()
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]

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

    res = {'calls_per_window': a.calls, 'windows': a.repeats, 'device': torch.cuda.get_device_name(0), 'params': PARAMS, 'denoise': DENOISE,
           'timing': {}, 'encoder': {}}
    for name, n, w, h in TIMING:
        fb = deintref.frame_bytes(w, h)
        # against the reference first: one frame out of place, and the in-place form with state on the same bytes
        cur = torch.randint(0, 256, (n, fb), dtype=torch.uint8, device='cuda')
        state = torch.randint(0, 256, (n, fb), dtype=torch.uint8, device='cuda')
        want, _ = deintref.deint_frame(cur[n - 1].cpu().numpy(), state[n - 1].cpu().numpy(), w, h, PARAMS)
        c0 = cur.clone()
        h264mi.i420_deinterlace(cur, cur, w, h, n, PARAMS, prev=state, prev_out=state)
        torch.cuda.synchronize()
        assert np.array_equal(cur[n - 1].cpu().numpy(), want), 'kernel != tests/deintref.py'
        assert torch.equal(state, c0), 'the state is not the unfiltered input'
        del c0
        bufs = [cur, torch.randint(0, 256, (n, fb), dtype=torch.uint8, device='cuda')]
        still, still_state = state.clone(), state.clone()
        near = (state.to(torch.int16) + torch.randint(-5, 6, (n, fb), dtype=torch.int16, device='cuda')).clamp(0, 255).to(torch.uint8)
        dn_state = state.clone()
        big = torch.zeros((2, 7 * n * fb // 4), dtype=torch.uint8, device='cuda')
        stream = h264mi._hip_stream(None)
        turn = [0]

        def moving_call():
            turn[0] ^= 1
            h264mi.i420_deinterlace(bufs[turn[0]], bufs[turn[0]], w, h, n, PARAMS, prev=state, prev_out=state)

        def still_call():  # the frames equal their state and stay so: woven, nothing changes
            h264mi.i420_deinterlace(still, still, w, h, n, PARAMS, prev=still_state, prev_out=still_state)

        def denoise_call():
            h264mi.i420_denoise(near, near, dn_state, w, h, n, DENOISE, dst2=dn_state)

        def copy_call():
            hip.hipMemcpyAsync(ctypes.c_void_p(big[1].data_ptr()), ctypes.c_void_p(big[0].data_ptr()), big[0].numel(), 3, stream)

        nbytes = {'deint-moving': 7 * n * fb // 2, 'deint-still': 7 * n * fb // 2, 'denoise': 4 * n * fb, 'copy': 2 * big[0].numel()}
        runs = (('deint-moving', moving_call), ('deint-still', still_call), ('denoise', denoise_call), ('copy', copy_call))
        for _ in range(a.warmup):
            for k, fn in runs:
                window(fn, a.calls)
        t = {k: [] for k, _ in runs}
        for _ in range(a.repeats):  # alternate
            for k, fn in runs:
                t[k].append(window(fn, a.calls))
        d = {'what': f'{n} frames {w}x{h}'}
        for k, _ in runs:
            d[k] = stats(t[k], nbytes[k])
        for k in ('deint-moving', 'deint-still', 'denoise'):
            d[k]['share_of_copy'] = d[k]['gbps'] / d['copy']['gbps']
        res['timing'][name] = d
        del bufs, cur, state, still, still_state, near, dn_state, big
        torch.cuda.empty_cache()

    # (b) the encoder step, filter off and on
    S, w, h = 8, 1920, 1080
    g = [SyntheticStream(s, w, h) for s in range(S)]
    nfr = 4
    prog = [[np.ascontiguousarray(g[s].frame(t)).ravel() for t in range(2 * nfr)] for s in range(S)]
    woven = [deintref.interlace(prog[s], w, h, 0) for s in range(S)]
    dev = [torch.from_numpy(np.stack([woven[s][t] for s in range(S)]).ravel()).cuda() for t in range(nfr)]
    encs = {}
    for k, setting in (('off', None), ('on', PARAMS)):
        e = h264mi.BatchEncoder(w, h, a.bitrate, S)
        e.set_frame_skip(False)
        e.set_deinterlace(setting)
        encs[k] = e
    at = {'off': 0, 'on': 0}

    def enc_window(k):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            encs[k].encode(dev[at[k] % nfr])
            encs[k].nal_sizes()
            at[k] += 1
        return (time.perf_counter() - t0) * 1e3 / a.steps

    for _ in range(a.warmup):
        for k in encs:
            enc_window(k)
    te = {k: [] for k in encs}
    for _ in range(a.repeats):
        for k in encs:
            te[k].append(enc_window(k))
    for k in encs:
        res['encoder'][k] = {'median_ms': statistics.median(te[k]), 'min_ms': min(te[k]), 'max_ms': max(te[k])}
        encs[k].close()
    res['encoder']['what'] = f'{S} streams {w}x{h}, {a.steps} steps a window, woven synthetic frames'

    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'deint_ab.json'), 'w') as f:
        json.dump(res, f, indent=1)
    lines = [f'(a) timing: {a.repeats} windows per version ({a.calls} calls a window), alternating; {res["device"]}; parameters {PARAMS}, in place with state', '',
             '| case | version | median ms | min ms | max ms | algorithmic bytes | GB/s | of the copy\'s rate |', '|---|---|---|---|---|---|---|---|']
    for name, d in res['timing'].items():
        for k in ('deint-moving', 'deint-still', 'denoise', 'copy'):
            x = d[k]
            share = f'{100 * x["share_of_copy"]:.0f} %' if k != 'copy' else ''
            lines.append(f'| {name} ({d["what"]}) | {k} | {x["median_ms"]:.4f} | {x["min_ms"]:.4f} | {x["max_ms"]:.4f} | {x["bytes_per_call"]} | {x["gbps"]:.0f} | {share} |')
    lines += ['', '(bytes: deint-moving reads cur and the state and writes half of cur and the state, 3.5 frame-sizes, deint-still '
              'the same; the denoiser reads two and writes two; copy is one device-to-device hipMemcpyAsync that reads and writes '
              '1.75 frame-sizes each. No hardware counter was collected.)', '',
              f'(b) encoder step ({res["encoder"]["what"]}), host clock around encode() and the wait for the NAL sizes', '',
              '| deinterlacer | median ms | min ms | max ms |', '|---|---|---|---|']
    for k in ('off', 'on'):
        x = res['encoder'][k]
        lines.append(f'| {k} | {x["median_ms"]:.3f} | {x["min_ms"]:.3f} | {x["max_ms"]:.3f} |')
    text = '\n'.join(lines) + '\n'
    with open(os.path.join(a.out, 'deint_ab.md'), 'w') as f:
        f.write(text)
    print(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
