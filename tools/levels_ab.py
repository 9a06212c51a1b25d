#!/usr/bin/env python3
"""Histograms, level tables and automatic levels (h264mi.i420_hist, i420_lut, i420_levels, csrc/levels.hip) measured.
The tables assert nothing but the equality of the bytes and words that are compared first.

Workloads: 128 frames of 1920x1080 and of 640x360; content random, natural-like (a ramp plus noise), flat, and two-level
(every sample 16 or 235 at random: a clipped picture, whose samples crowd two bins without being equal across a wave).
  hist        : the library call, one memset and one launch
  lut         : the library call out of place with per-frame random tables, one launch
  levels-auto : the whole AUTO call out of place (memset, histogram, decide, apply)
  levels-fixed: the FIXED call out of place (decide, apply); minus lut it bounds the decide kernel, which no call runs alone
  torch-hist  : what a caller had before: per plane one torch.bincount over (samples + 256 x frame index)
  torch-lut   : what a caller had before: per plane an indexed lookup table[frame, samples]
  copy        : one device-to-device hipMemcpyAsync of the n frames
Each sample is one window of calls between two device events; the versions alternate, sample by sample, in the same
run. Reported: the median, minimum and maximum time of one call, the frame bytes a call covers per second, that as a
share of the copy's rate (the copy reads and writes the bytes, the histogram only reads them: no traffic is equated,
the copy is a yardstick), the multiple of the torch expression, and the histogram's flat-to-random and two-level-to-random ratios.

The encoder: one frame step (encode and the wait for its sizes) of 128 streams 640x360 and 16 streams 1920x1080 with the
stage on (AUTO) against the stage off, alternating windows, natural-like content.

Writes levels_ab.json and levels_ab.md into --out.

    python tools/levels_ab.py --out profiles/levels
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
WORKLOADS = (('full-hd', 128, 1920, 1080), ('360p', 128, 640, 360))
CONTENTS = ('random', 'natural', 'flat', 'two-level')
ENCODERS = ((128, 640, 360), (16, 1920, 1080))
AUTO = (0, 655, 655, 0, 0, 16, 235, 256, 37, 64)
FIXED = (1, 0, 0, 30, 200, 16, 235, 64, 1, 80)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=10, help='calls per timed window')
    ap.add_argument('--repeats', type=int, default=15, help='timed windows per version')
    ap.add_argument('--warmup', type=int, default=2, help='untimed windows per version')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'levels'))
    a = ap.parse_args()
    import numpy as np
    import torch
    import h264mi
    import levelsref
    if not torch.cuda.is_available():
        raise SystemExit('levels_ab.py measures on the GPU: no device found')
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
        return {'median_ms': med, 'min_ms': min(v), 'max_ms': max(v), 'gbps': nbytes / (med * 1e-3) / 1e9}

    def content(kind, n, w, h):
        fb = levelsref.frame_bytes(w, h)
        g = torch.Generator(device='cuda').manual_seed(11)
        if kind == 'random':
            return torch.randint(0, 256, (n, fb), dtype=torch.uint8, device='cuda', generator=g)
        if kind == 'two-level':
            return torch.where(torch.randint(0, 2, (n, fb), device='cuda', generator=g) == 1, 235, 16).to(torch.uint8)
        if kind == 'flat':
            return (torch.arange(n, device='cuda', dtype=torch.int64)[:, None] * 37 % 256).to(torch.uint8).expand(n, fb).contiguous()
        ramp = (torch.arange(fb, device='cuda', dtype=torch.int64) * 3 // 16) % 160 + 40
        noise = torch.randint(-4, 5, (n, fb), device='cuda', generator=g)
        return (ramp[None, :] + noise).clamp(0, 255).to(torch.uint8)

    def plane_views(t, w, h):
        y, c = w * h, (w // 2) * (h // 2)
        return [t[:, :y], t[:, y:y + c], t[:, y + c:y + 2 * c]]

    res = {'calls_per_window': a.calls, 'windows': a.repeats, 'device': torch.cuda.get_device_name(0), 'timing': {}, 'encoder': []}
    for name, n, w, h in WORKLOADS:
        fb = levelsref.frame_bytes(w, h)
        nbytes = n * fb
        stream = h264mi._hip_stream(None)
        hist = torch.zeros(n * 768, dtype=torch.int32, device='cuda')
        thist = torch.zeros((n, 768), dtype=torch.int64, device='cuda')
        luts = torch.randint(0, 256, (n, 768), dtype=torch.uint8, device='cuda')
        work = torch.zeros(h264mi.levels_work_bytes(n), dtype=torch.uint8, device='cuda')
        state = torch.zeros(4 * n, dtype=torch.int32, device='cuda')
        out = [torch.zeros((n, fb), dtype=torch.uint8, device='cuda') for _ in range(3)]
        base = torch.arange(n, device='cuda', dtype=torch.int64)[:, None] * 256
        for kind in CONTENTS:
            src = content(kind, n, w, h)

            def torch_hist():
                for pl, P in enumerate(plane_views(src, w, h)):
                    thist[:, 256 * pl:256 * pl + 256] = torch.bincount((P.long() + base).ravel(), minlength=256 * n).view(n, 256)

            def torch_lut():
                for pl, (P, O) in enumerate(zip(plane_views(src, w, h), plane_views(out[1], w, h))):
                    O.copy_(torch.gather(luts[:, 256 * pl:256 * pl + 256], 1, P.long()))

            runs = (('hist', lambda: h264mi.i420_hist(hist, src, w, h, n)),
                    ('lut', lambda: h264mi.i420_lut(out[0], src, w, h, n, luts, per_frame=True)),
                    ('levels-auto', lambda: h264mi.i420_levels(out[2], src, w, h, n, AUTO, work, state=state)),
                    ('levels-fixed', lambda: h264mi.i420_levels(out[2], src, w, h, n, FIXED, work)),
                    ('torch-hist', torch_hist), ('torch-lut', torch_lut),
                    ('copy', lambda: hip.hipMemcpyAsync(ctypes.c_void_p(out[1].data_ptr()), ctypes.c_void_p(src.data_ptr()), nbytes, 3, stream)))
            h264mi.i420_hist(hist, src, w, h, n)
            torch_hist()
            h264mi.i420_lut(out[0], src, w, h, n, luts, per_frame=True)
            torch_lut()
            torch.cuda.synchronize()
            assert torch.equal(hist.view(n, 768).long(), thist), f'{name} {kind}: histogram != torch'
            assert torch.equal(out[0], out[1]), f'{name} {kind}: lut != torch'
            assert np.array_equal(hist.view(n, 768)[n - 1].cpu().numpy().view(np.uint32), levelsref.hist_frame(src[n - 1].cpu().numpy(), w, h)), 'kernel != tests/levelsref.py'
            slow = ('torch-hist', 'torch-lut')
            for _ in range(a.warmup):
                for k, fn in runs:
                    window(fn, 2 if k in slow else a.calls)
            t = {k: [] for k, _ in runs}
            for _ in range(a.repeats):  # alternate
                for k, fn in runs:
                    t[k].append(window(fn, 2 if k in slow else a.calls))
            d = {'what': f'{n} frames {w}x{h}', 'content': kind, 'bytes_per_call': nbytes}
            for k, _ in runs:
                d[k] = stats(t[k], nbytes)
                d[k]['share_of_copy'] = d[k]['gbps'] / stats(t['copy'], nbytes)['gbps']
            d['hist']['times_torch'] = d['torch-hist']['median_ms'] / d['hist']['median_ms']
            d['lut']['times_torch'] = d['torch-lut']['median_ms'] / d['lut']['median_ms']
            d['decide_bound_ms'] = d['levels-fixed']['median_ms'] - d['lut']['median_ms']
            res['timing'][f'{name} {kind}'] = d
            del src
        r = res['timing'][f'{name} random']
        for kind in ('flat', 'two-level'):
            res['timing'][f'{name} {kind}']['hist_to_random'] = res['timing'][f'{name} {kind}']['hist']['median_ms'] / r['hist']['median_ms']
        del out, hist, thist, luts, work
        torch.cuda.empty_cache()

    for S, w, h in ENCODERS:
        frames = content('natural', S, w, h).ravel()
        encs = {}
        for k, setting in (('off', None), ('on', AUTO)):
            enc = h264mi.BatchEncoder(w, h, 2000000, S)
            enc.set_frame_skip(False)
            enc.set_levels(setting)
            encs[k] = enc

        def step(enc):
            enc.encode(frames)
            enc.nal_sizes()

        t = {k: [] for k in encs}
        for rep in range(a.warmup + a.repeats):
            for k, enc in encs.items():
                ms = window(lambda: step(enc), a.calls)
                if rep >= a.warmup:
                    t[k].append(ms)
        for enc in encs.values():
            enc.close()
        e = {'what': f'{S} streams {w}x{h}', 'off': stats(t['off'], S * levelsref.frame_bytes(w, h)), 'on': stats(t['on'], S * levelsref.frame_bytes(w, h))}
        e['added_ms'] = e['on']['median_ms'] - e['off']['median_ms']
        res['encoder'].append(e)

    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'levels_ab.json'), 'w') as f:
        json.dump(res, f, indent=1)
    lines = [f'timing: {a.repeats} windows per version ({a.calls} calls a window, 2 for torch), alternating; {res["device"]}', '',
             '| case | version | median ms | min ms | max ms | GB/s of frame bytes | of the copy\'s rate | x torch |', '|---|---|---|---|---|---|---|---|']
    for name, d in res['timing'].items():
        for k in ('hist', 'lut', 'levels-auto', 'levels-fixed', 'torch-hist', 'torch-lut', 'copy'):
            x = d[k]
            share = f'{100 * x["share_of_copy"]:.0f} %' if k != 'copy' else ''
            times = f'{x["times_torch"]:.1f}' if 'times_torch' in x else ''
            lines.append(f'| {name} ({d["what"]}) | {k} | {x["median_ms"]:.4f} | {x["min_ms"]:.4f} | {x["max_ms"]:.4f} | {x["gbps"]:.0f} | {share} | {times} |')
        lines.append(f'| {name} | levels-fixed minus lut (bounds the decide kernel) | {d["decide_bound_ms"]:.4f} | | | | | |')
        if 'hist_to_random' in d:
            lines.append(f'| {name} | histogram, this content\'s time / random time | {d["hist_to_random"]:.2f} | | | | | |')
    lines += ['', '(GB/s from the n frames\' bytes once, whatever a version reads and writes. copy is one device-to-device hipMemcpyAsync of the n frames. '
              'No hardware counter was collected.)', '', 'encoder: one frame step (encode and the wait for its sizes), the stage off and on (AUTO), alternating windows', '',
              '| case | off median ms | off min..max | on median ms | on min..max | added ms |', '|---|---|---|---|---|---|']
    for e in res['encoder']:
        lines.append(f'| {e["what"]} | {e["off"]["median_ms"]:.4f} | {e["off"]["min_ms"]:.4f}..{e["off"]["max_ms"]:.4f} | {e["on"]["median_ms"]:.4f} | '
                     f'{e["on"]["min_ms"]:.4f}..{e["on"]["max_ms"]:.4f} | {e["added_ms"]:.4f} |')
    text = '\n'.join(lines) + '\n'
    with open(os.path.join(a.out, 'levels_ab.md'), 'w') as f:
        f.write(text)
    print(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
