#!/usr/bin/env python3
"""The I420 downscaler (h264mi.i420_scale, csrc/scale.hip) measured at the ladder's workload: n frames of 1920x1080 per
call (default 128) down to 1280x720, 960x540 and 640x360.

  scale  : h264mi.i420_scale, one launch for the n frames
  torch  : what a caller had before it -- per plane uint8 -> float, torch.nn.functional.interpolate(mode='area'),
           round, clamp, -> uint8 into the tight destination frames, on the same device (not the same bytes: its
           rounding is floating point)
  colour : h264mi.i420_to_rgba on the same n source frames, this project's own streaming kernel over the same planes,
           re-measured in the same run as the yardstick of "streaming speed here"

Each sample is one window of calls between two device events; the versions alternate, sample by sample, in the same
run. Reported per size pair: the median, minimum and maximum time of one n-frame call, GB/s from the algorithmic
1.5 * (sw * sh + dw * dh) * n bytes (5.5 * sw * sh * n for the colour kernel), that as a share of the 8 TB/s HBM peak
and of the 6.3 TB/s streaming ceiling, the ratio to the colour kernel's GB/s, and whether the kernel is ahead of the
torch path by more than both sides' min..max spread. The kernel's output is checked against tests/scaleref.py on the
first frame first. Writes scale_ab.json and scale_ab.md into --out.

    python tools/scale_ab.py --out profiles/scale
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'openh264-wasm_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
HBM_PEAK, HBM_CEILING = 8.0e12, 6.3e12
TARGETS = ((1280, 720), (960, 540), (640, 360))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--frames', type=int, default=128, help='frames per call')
    ap.add_argument('--calls', type=int, default=20, help='kernel calls per timed window')
    ap.add_argument('--torch-calls', type=int, default=3, help='torch-path calls per timed window')
    ap.add_argument('--repeats', type=int, default=21, help='timed windows per version')
    ap.add_argument('--warmup', type=int, default=3, help='untimed windows per version')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scale'))
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    import h264mi
    import scaleref
    if not torch.cuda.is_available():
        raise SystemExit('scale_ab.py measures on the GPU: no device found')
    sw, sh, n = a.width, a.height, a.frames
    sfb = scaleref.frame_bytes(sw, sh)
    src = torch.randint(0, 256, (n * sfb,), dtype=torch.uint8, device='cuda')
    rgba = torch.zeros(n * sw * sh * 4, dtype=torch.uint8, device='cuda')

    def torch_path(dst, dw, dh):
        s, d = src.view(n, sfb), dst.view(n, -1)
        so = do = 0
        for pw, ph, qw, qh in ((sw, sh, dw, dh), (sw // 2, sh // 2, dw // 2, dh // 2), (sw // 2, sh // 2, dw // 2, dh // 2)):
            p = s[:, so:so + pw * ph].reshape(n, 1, ph, pw).float()
            q = F.interpolate(p, size=(qh, qw), mode='area').round_().clamp_(0, 255).to(torch.uint8)
            d[:, do:do + qw * qh] = q.reshape(n, qw * qh)
            so += pw * ph
            do += qw * qh

    def window(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls  # ms per n-frame call

    def stats(v, nbytes):
        med = statistics.median(v)
        return {'median_ms': med, 'min_ms': min(v), 'max_ms': max(v), 'spread_ms': max(v) - min(v), 'gbps': nbytes / (med * 1e-3) / 1e9,
                'share_of_peak': nbytes / (med * 1e-3) / HBM_PEAK, 'share_of_ceiling': nbytes / (med * 1e-3) / HBM_CEILING}

    res = {'width': sw, 'height': sh, 'frames': n, 'calls_per_window': a.calls, 'torch_calls_per_window': a.torch_calls, 'windows': a.repeats,
           'device': torch.cuda.get_device_name(0), 'pairs': {}}
    colour_bytes = 5.5 * sw * sh * n
    for dw, dh in TARGETS:
        dfb = scaleref.frame_bytes(dw, dh)
        dst = [torch.zeros(n * dfb, dtype=torch.uint8, device='cuda') for _ in range(2)]
        runs = (('scale', lambda: h264mi.i420_scale(dst[0], src, sw, sh, dw, dh, n), a.calls),
                ('torch', lambda: torch_path(dst[1], dw, dh), a.torch_calls),
                ('colour', lambda: h264mi.i420_to_rgba(rgba, src, sw, sh, n), a.calls))
        runs[0][1]()
        torch.cuda.synchronize()
        want = scaleref.scale_frame(src[:sfb].cpu().numpy(), sw, sh, dw, dh)
        assert np.array_equal(dst[0][:dfb].cpu().numpy(), want), f'{dw}x{dh}: kernel != tests/scaleref.py'
        for _ in range(a.warmup):
            for _, fn, calls in runs:
                window(fn, calls)
        t = {k: [] for k, _, _ in runs}
        for _ in range(a.repeats):  # alternate
            for k, fn, calls in runs:
                t[k].append(window(fn, calls))
        nbytes = 1.5 * (sw * sh + dw * dh) * n
        d = {'bytes_per_call': nbytes, 'scale': stats(t['scale'], nbytes), 'torch': stats(t['torch'], nbytes),
             'colour': stats(t['colour'], colour_bytes)}
        d['gbps_vs_colour'] = d['scale']['gbps'] / d['colour']['gbps']
        d['speedup_vs_torch'] = d['torch']['median_ms'] / d['scale']['median_ms']
        d['gain_ms'] = d['torch']['median_ms'] - d['scale']['median_ms']
        d['ahead_by_more_than_spread'] = d['torch']['min_ms'] - d['scale']['max_ms'] > 0 and \
            d['gain_ms'] > d['torch']['spread_ms'] + d['scale']['spread_ms']
        res['pairs'][f'{dw}x{dh}'] = d
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'scale_ab.json'), 'w') as f:
        json.dump(res, f, indent=1)
    lines = [f'{n} frames of {sw}x{sh} per call; {a.repeats} windows per version ({a.calls} calls a window, torch path {a.torch_calls}), '
             f'alternating; {res["device"]}', '',
             '| to | version | median ms | min ms | max ms | GB/s (algorithmic) | of 8 TB/s peak | of 6.3 TB/s ceiling | GB/s vs colour kernel |',
             '|---|---|---|---|---|---|---|---|---|']
    for name, d in res['pairs'].items():
        for k in ('scale', 'torch', 'colour'):
            x = d[k]
            rel = f'{d["gbps_vs_colour"]:.2f}x' if k == 'scale' else ''
            lines.append(f'| {name} | {k} | {x["median_ms"]:.4f} | {x["min_ms"]:.4f} | {x["max_ms"]:.4f} | {x["gbps"]:.0f} | '
                         f'{100 * x["share_of_peak"]:.1f} % | {100 * x["share_of_ceiling"]:.1f} % | {rel} |')
        lines.append(f'| {name} | scale vs torch | {d["speedup_vs_torch"]:.2f}x, {d["gain_ms"]:.4f} ms ahead; more than both spreads: '
                     f'{d["ahead_by_more_than_spread"]} | | | | | | |')
    lines += ['', "(colour: i420_to_rgba on the same source frames, 5.5 * w * h * n bytes; torch: the bytes a caller wants moved, its own "
              'traffic is several times that.)']
    text = '\n'.join(lines) + '\n'
    with open(os.path.join(a.out, 'scale_ab.md'), 'w') as f:
        f.write(text)
    print(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
