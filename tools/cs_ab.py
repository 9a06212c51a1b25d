#!/usr/bin/env python3
"""A/B of the colour-specification kernels (csrc/colorspace.hip) against the default kernels of the same direction
(csrc/color.inc, csrc/overlay.hip), at the project's workload: n frames of w x h per call (default 128 x 1920x1080).

  rgba_to_i420  : default kernel | cs TOPLEFT (601 limited: the same bytes) | cs AVERAGE (709 full)
  i420_to_rgba  : default kernel | cs REPEAT (601 limited: the same bytes)  | cs BILINEAR (709 full)
  rgba_to_i420a : default kernel | cs AVERAGE (709 full)

Each sample is one window of --calls conversions of the whole batch between two device events; the versions of a
direction alternate, sample by sample, in the same run. Reported per version: the median, minimum and maximum time of
one n-frame conversion, GB/s from the algorithmic bytes (5.5 w h n: 4wh RGBA + 1.5wh I420; 6.5 w h n with the alpha
plane) and that as a share of the 6.3 TB/s streaming ceiling, and the ratio of its median to the default kernel's with
whether the difference exceeds the two versions' window spreads. Outputs are checked first: the cs kernels under the
default specification give the default kernels' bytes. Writes cs_ab.json and cs_ab.md into --out.

    python tools/cs_ab.py --out profiles/colorspace
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'openh264-wasm_amd'))
HBM_CEILING = 6.3e12


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--frames', type=int, default=128, help='frames per conversion call')
    ap.add_argument('--calls', type=int, default=20, help='conversion calls per timed window')
    ap.add_argument('--repeats', type=int, default=21, help='timed windows per version')
    ap.add_argument('--warmup', type=int, default=3, help='untimed windows per version')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'colorspace'))
    a = ap.parse_args()
    import torch
    import h264mi
    if not torch.cuda.is_available():
        raise SystemExit('cs_ab.py measures on the GPU: no device found')
    w, h, n = a.width, a.height, a.frames
    fr, fi, fa = w * h * 4, w * h * 3 // 2, h264mi.i420a_bytes(w, h)
    rgba = torch.randint(0, 256, (n * fr,), dtype=torch.uint8, device='cuda')
    yuv = torch.randint(0, 256, (n * fi,), dtype=torch.uint8, device='cuda')
    out_i = [torch.zeros(n * fi, dtype=torch.uint8, device='cuda') for _ in range(2)]
    out_r = [torch.zeros(n * fr, dtype=torch.uint8, device='cuda') for _ in range(2)]
    out_a = [torch.zeros(n * fa, dtype=torch.uint8, device='cuda') for _ in range(2)]
    dflt, hd_in, hd_out = h264mi.ColorSpec(0, 0, 0, 0), h264mi.ColorSpec(1, 1, 1, 0), h264mi.ColorSpec(1, 1, 0, 1)

    # direction: (algorithmic bytes, [(version, call)]); the first version is the default kernel
    runs = {
        'rgba_to_i420': (5.5 * w * h * n, [
            ('default kernel', lambda: h264mi.rgba_to_i420(out_i[0], rgba, w, h, n)),
            ('cs 601 limited TOPLEFT', lambda: h264mi.rgba_to_i420(out_i[1], rgba, w, h, n, spec=dflt)),
            ('cs 709 full AVERAGE', lambda: h264mi.rgba_to_i420(out_i[1], rgba, w, h, n, spec=hd_in))]),
        'i420_to_rgba': (5.5 * w * h * n, [
            ('default kernel', lambda: h264mi.i420_to_rgba(out_r[0], yuv, w, h, n)),
            ('cs 601 limited REPEAT', lambda: h264mi.i420_to_rgba(out_r[1], yuv, w, h, n, spec=dflt)),
            ('cs 709 full BILINEAR', lambda: h264mi.i420_to_rgba(out_r[1], yuv, w, h, n, spec=hd_out))]),
        'rgba_to_i420a': (6.5 * w * h * n, [
            ('default kernel', lambda: h264mi.rgba_to_i420a(out_a[0], rgba, w, h, n)),
            ('cs 709 full AVERAGE', lambda: h264mi.rgba_to_i420a(out_a[1], rgba, w, h, n, spec=hd_in))]),
    }
    # same bytes first
    for name, outs in (('rgba_to_i420', out_i), ('i420_to_rgba', out_r)):
        runs[name][1][0][1](); runs[name][1][1][1]()
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]), f'{name}: the cs kernel under the default specification != the default kernel'
    h264mi.rgba_to_i420a(out_a[0], rgba, w, h, n); h264mi.rgba_to_i420a(out_a[1], rgba, w, h, n, spec=dflt)
    torch.cuda.synchronize()
    assert torch.equal(out_a[0], out_a[1]), 'rgba_to_i420a: the cs kernel under the default specification != the default kernel'

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls  # ms per n-frame conversion

    res = {'width': w, 'height': h, 'frames': n, 'calls_per_window': a.calls, 'windows': a.repeats,
           'device': torch.cuda.get_device_name(0), 'directions': {}}
    for name, (nbytes, versions) in runs.items():
        for _ in range(a.warmup):
            for _, fn in versions:
                window(fn)
        t = {k: [] for k, _ in versions}
        for _ in range(a.repeats):  # alternate
            for k, fn in versions:
                t[k].append(window(fn))
        d = {'bytes_per_call': nbytes, 'versions': {}}
        for k, v in t.items():
            med = statistics.median(v)
            d['versions'][k] = {'median_ms': med, 'min_ms': min(v), 'max_ms': max(v), 'spread_ms': max(v) - min(v),
                                'gbps': nbytes / (med * 1e-3) / 1e9, 'share_of_ceiling': nbytes / (med * 1e-3) / HBM_CEILING}
        base = d['versions'][versions[0][0]]
        for k, _ in versions[1:]:
            x = d['versions'][k]
            x['ratio_to_default'] = x['median_ms'] / base['median_ms']
            x['differs_by_more_than_spread'] = abs(x['median_ms'] - base['median_ms']) > x['spread_ms'] + base['spread_ms']
        res['directions'][name] = d
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'cs_ab.json'), 'w') as f:
        json.dump(res, f, indent=1)
    lines = [f'{n} frames of {w}x{h} per call; {a.repeats} windows of {a.calls} calls per version, the versions of a direction '
             f'alternating; {res["device"]}', '',
             '| direction | version | median ms | min ms | max ms | GB/s | of 6.3 TB/s ceiling | median / default | beyond both spreads |',
             '|---|---|---|---|---|---|---|---|---|']
    for name, d in res['directions'].items():
        for k, x in d['versions'].items():
            ratio = f'{x["ratio_to_default"]:.3f}' if 'ratio_to_default' in x else ''
            beyond = str(x['differs_by_more_than_spread']) if 'ratio_to_default' in x else ''
            lines.append(f'| {name} | {k} | {x["median_ms"]:.4f} | {x["min_ms"]:.4f} | {x["max_ms"]:.4f} | {x["gbps"]:.0f} | '
                         f'{100 * x["share_of_ceiling"]:.1f} % | {ratio} | {beyond} |')
    text = '\n'.join(lines) + '\n'
    with open(os.path.join(a.out, 'cs_ab.md'), 'w') as f:
        f.write(text)
    print(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
