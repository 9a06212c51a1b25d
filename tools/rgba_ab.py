#!/usr/bin/env python3
"""A/B of the batched colour-conversion kernels against the per-picture kernels they replaced, at the
project's workload: n frames of w x h per call (default 128 x 1920x1080), both directions.

  batched : h264mi.rgba_to_i420 / i420_to_rgba, one launch for the n frames
  parent  : the previous per-picture kernels (tools/rgba_ab.hip, a verbatim copy), n launches

Each sample is one window of --calls conversions of the whole batch between two device events; the two
versions alternate, sample by sample, in the same run. Reported per direction: the median, minimum and maximum
time of one n-frame conversion, GB/s from the algorithmic 5.5 * w * h * n bytes (4wh RGBA + 1.5wh I420) and
that as a share of the 8 TB/s HBM peak (about 6.3 TB/s is the achievable streaming ceiling). The outputs of
the two versions are compared byte for byte first. Writes rgba_ab.json and rgba_ab.md into --out.

    python tools/rgba_ab.py --out profiles/rgba
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'openh264-wasm_amd'))
SRC = os.path.join(ROOT, 'tools', 'rgba_ab.hip')
LIB = os.path.join(ROOT, 'tools', 'build', 'librgba_ab.so')
HBM_PEAK, HBM_CEILING = 8.0e12, 6.3e12


def build_parent():
    if os.path.exists(LIB) and os.path.getmtime(LIB) >= os.path.getmtime(SRC):
        return LIB
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    subprocess.run(['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-o', LIB, SRC], check=True)
    return LIB


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--frames', type=int, default=128, help='frames per conversion call')
    ap.add_argument('--calls', type=int, default=20, help='conversion calls per timed window')
    ap.add_argument('--repeats', type=int, default=21, help='timed windows per version (>= 20)')
    ap.add_argument('--warmup', type=int, default=3, help='untimed windows per version')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rgba'))
    ap.add_argument('--build-only', action='store_true', help='compile the parent kernels and exit (no GPU needed)')
    a = ap.parse_args()
    parent_lib = build_parent()
    if a.build_only:
        return 0
    import torch  # before any library that links the HIP runtime: the process must hold torch's copy of it alone
    import h264mi
    P = ctypes.CDLL(parent_lib)
    if not torch.cuda.is_available():
        raise SystemExit('rgba_ab.py measures on the GPU: no device found')
    w, h, n = a.width, a.height, a.frames
    vp, ci = ctypes.c_void_p, ctypes.c_int
    for f in (P.rgba_ab_parent_rgba_to_i420, P.rgba_ab_parent_i420_to_rgba):
        f.restype, f.argtypes = ci, [vp, vp, ci, ci, ci, vp]
    fr, fi = w * h * 4, w * h * 3 // 2
    rgba = torch.randint(0, 256, (n * fr,), dtype=torch.uint8, device='cuda')
    yuv = torch.randint(0, 256, (n * fi,), dtype=torch.uint8, device='cuda')
    out_i = [torch.zeros(n * fi, dtype=torch.uint8, device='cuda') for _ in range(2)]
    out_r = [torch.zeros(n * fr, dtype=torch.uint8, device='cuda') for _ in range(2)]
    st = torch.cuda.current_stream()

    def parent(fn, dst, src):
        if fn(vp(dst.data_ptr()), vp(src.data_ptr()), w, h, n, vp(st.cuda_stream)) != 0:
            raise RuntimeError('parent launch failed')

    runs = {
        'rgba_to_i420': (lambda: h264mi.rgba_to_i420(out_i[0], rgba, w, h, n), lambda: parent(P.rgba_ab_parent_rgba_to_i420, out_i[1], rgba)),
        'i420_to_rgba': (lambda: h264mi.i420_to_rgba(out_r[0], yuv, w, h, n), lambda: parent(P.rgba_ab_parent_i420_to_rgba, out_r[1], yuv)),
    }
    for name, (new, old) in runs.items():  # same bytes first
        new(); old()
        torch.cuda.synchronize()
    assert torch.equal(out_i[0], out_i[1]), 'rgba_to_i420: batched != parent'
    assert torch.equal(out_r[0], out_r[1]), 'i420_to_rgba: batched != parent'

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls  # ms per n-frame conversion

    nbytes = 5.5 * w * h * n
    res = {'width': w, 'height': h, 'frames': n, 'calls_per_window': a.calls, 'windows': a.repeats, 'bytes_per_call': nbytes,
           'device': torch.cuda.get_device_name(0), 'directions': {}}
    for name, (new, old) in runs.items():
        for _ in range(a.warmup):
            window(new); window(old)
        t = {'batched': [], 'parent': []}
        for _ in range(a.repeats):  # alternate
            t['batched'].append(window(new))
            t['parent'].append(window(old))
        d = {}
        for k, v in t.items():
            med = statistics.median(v)
            d[k] = {'median_ms': med, 'min_ms': min(v), 'max_ms': max(v), 'spread_ms': max(v) - min(v),
                    'gbps': nbytes / (med * 1e-3) / 1e9, 'share_of_peak': nbytes / (med * 1e-3) / HBM_PEAK,
                    'share_of_ceiling': nbytes / (med * 1e-3) / HBM_CEILING}
        d['speedup'] = d['parent']['median_ms'] / d['batched']['median_ms']
        d['gain_ms'] = d['parent']['median_ms'] - d['batched']['median_ms']
        d['ahead_by_more_than_spread'] = d['parent']['min_ms'] - d['batched']['max_ms'] > 0 and \
            d['gain_ms'] > d['parent']['spread_ms'] + d['batched']['spread_ms']
        res['directions'][name] = d
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'rgba_ab.json'), 'w') as f:
        json.dump(res, f, indent=1)
    lines = [f'{n} frames of {w}x{h} per call, {nbytes / 1e9:.3f} GB algorithmic per call; {a.repeats} windows of {a.calls} calls per '
             f'version, alternating; {res["device"]}', '',
             '| direction | version | launches | median ms | min ms | max ms | GB/s | of 8 TB/s peak | of 6.3 TB/s ceiling |',
             '|---|---|---|---|---|---|---|---|---|']
    for name, d in res['directions'].items():
        for k, launches in (('batched', 1), ('parent', n)):
            x = d[k]
            lines.append(f'| {name} | {k} | {launches} | {x["median_ms"]:.4f} | {x["min_ms"]:.4f} | {x["max_ms"]:.4f} | {x["gbps"]:.0f} | '
                         f'{100 * x["share_of_peak"]:.1f} % | {100 * x["share_of_ceiling"]:.1f} % |')
        lines.append(f'| {name} | batched vs parent | | {d["speedup"]:.2f}x, {d["gain_ms"]:.4f} ms ahead; more than both spreads: '
                     f'{d["ahead_by_more_than_spread"]} | | | | | |')
    text = '\n'.join(lines) + '\n'
    with open(os.path.join(a.out, 'rgba_ab.md'), 'w') as f:
        f.write(text)
    print(text)
    print(json.dumps({k: {'batched_ms': v['batched']['median_ms'], 'parent_ms': v['parent']['median_ms']} for k, v in res['directions'].items()}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
