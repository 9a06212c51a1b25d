#!/usr/bin/env python3
"""The mesh warp (h264mi.i420_warp, csrc/warp.hip) measured on 128 frames of 1920x1080 -> 1920x1080, one shared mesh of
pitch 16 built by the library's own builders, each case with both filters:

  identity : the mesh that copies
  rotate7  : 7 degrees about the centre (affine builder), edge FILL
  radial   : barrel correction k1 = 0.2, k2 = 0.05 about the centre (radial builder)
  zoomout8 : every step eight source samples (affine builder): the footprints leave the staged class

beside the two nearest existing things that move the same frames without a gather, timed in the same run:

  copy     : a device-to-device copy of the 128 frames (torch Tensor.copy_)
  upscale  : h264mi.i420_upscale 1920x1080 -> 1920x1080 bicubic -- the same two-pass arithmetic, rows addressed from the
             output index alone

and, for rotate7, the same call with every tile forced onto the global-memory path (h264mi_i420_warp_path_dev, an entry
for this tool only, not in the header): what staging the footprint in LDS buys. rotate7 is also run at pitch 8 and 32.

Each sample is one window of calls between two device events; the versions alternate, sample by sample, in the same
run. Reported per version: the median, minimum and maximum time of one call and GB/s from the algorithmic bytes (every
source frame read once, every destination sample written once). Before timing, the identity's output is compared with
the source, one frame of every other case with tests/warpref.py, and the forced path's bytes with the chosen path's.
The table asserts nothing about speed. Writes warp_ab.json and warp_ab.md into --out.

    python tools/warp_ab.py --out profiles/warp
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'openh264-wasm_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
W, H, N = 1920, 1080, 128


def q16(v):
    return int(round(v * 65536))


def meshes(h264mi, np, g):
    c, s = q16(np.cos(np.radians(7))), q16(np.sin(np.radians(7)))
    G = 1 << g
    return {
        'identity': h264mi.warp_mesh_affine(W, H, g, [65536, 0, 0, 0, 65536, 0]),
        'rotate7': h264mi.warp_mesh_affine(W, H, g, [c, -s, (65536 * (W - 1) - c * (W - 1) + s * (H - 1)) // 2,
                                                   s, c, (65536 * (H - 1) - s * (W - 1) - c * (H - 1)) // 2]),
        'radial': h264mi.warp_mesh_radial(W, H, g, 8 * (W - 1), 8 * (H - 1), (8 * (W + 2 * G)) ** 2 + (8 * (H + 2 * G)) ** 2, q16(0.2), q16(0.05)),
        'zoomout8': h264mi.warp_mesh_affine(W, H, g, [8 * 65536, 0, 0, 0, 8 * 65536, 0]),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=5, help='calls per timed window')
    ap.add_argument('--repeats', type=int, default=15, help='timed windows per version')
    ap.add_argument('--warmup', type=int, default=2, help='untimed windows per version')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'warp'))
    a = ap.parse_args()
    import numpy as np
    import torch
    import h264mi
    import warpref
    if not torch.cuda.is_available():
        raise SystemExit('warp_ab.py measures on the GPU: no device found')
    import ctypes
    vp, ci = ctypes.c_void_p, ctypes.c_int
    path_dev = h264mi.lib().h264mi_i420_warp_path_dev
    path_dev.restype, path_dev.argtypes = ci, [vp, ci, ci, vp, ci, ci, ci, vp, ci, vp, ci, vp]
    fb = warpref.frame_bytes(W, H)
    nbytes = 2 * N * fb
    src = torch.randint(0, 256, (N, fb), dtype=torch.uint8, device='cuda')
    out = torch.zeros((N, fb), dtype=torch.uint8, device='cuda')
    out2 = torch.zeros((N, fb), dtype=torch.uint8, device='cuda')

    def window(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls  # ms per call

    def stats(v):
        med = statistics.median(v)
        return {'median_ms': med, 'min_ms': min(v), 'max_ms': max(v), 'gbps': nbytes / (med * 1e-3) / 1e9}

    def warp_call(d_mesh, prm, forced=False, dst=out):
        rec = h264mi.Warp(*prm)

        def fn():
            if forced:
                assert path_dev(dst.data_ptr(), W, H, src.data_ptr(), W, H, N, d_mesh.data_ptr(), 0, ctypes.byref(rec), 1,
                                torch.cuda.current_stream().cuda_stream) == 0
            else:
                h264mi.i420_warp(dst, src, W, H, W, H, N, d_mesh, prm)
        return fn

    runs = {'copy': lambda: out.copy_(src), 'upscale bicubic': lambda: h264mi.i420_upscale(out, src, W, H, W, H, N, h264mi.FILTER_BICUBIC)}
    classes = {}
    keep = []
    for g in (4, 3, 5):
        host = meshes(h264mi, np, g)
        mw, mh = h264mi.warp_mesh_size(W, H, g)
        for name, m in host.items():
            if g != 4 and name != 'rotate7':
                continue
            d_mesh = torch.from_numpy(m.reshape(-1)).cuda()
            keep.append(d_mesh)
            cl = [h264mi.warp_tile_class(m, W, H, W, H, g, p, tx, ty) for p in range(3) for ty in range(mh - 1) for tx in range(mw - 1)]
            classes[f'{name} pitch {1 << g}'] = {'tiles': len(cl), 'fallback_tiles': int(sum(cl))}
            for filt, fname in ((h264mi.FILTER_BILINEAR, 'bilinear'), (h264mi.FILTER_BICUBIC, 'bicubic')):
                prm = (filt, h264mi.WARP_FILL if name == 'rotate7' else h264mi.WARP_CLAMP, 16, 128, 128, g)
                key = f'{name} {fname}' + ('' if g == 4 else f' pitch {1 << g}')
                runs[key] = warp_call(d_mesh, prm)
                runs[key]()
                torch.cuda.synchronize()
                if name == 'identity':
                    assert torch.equal(out, src), 'the identity mesh did not copy'
                else:
                    want = warpref.warp_frame(src[N - 1].cpu().numpy(), W, H, W, H, m, prm)
                    assert np.array_equal(out[N - 1].cpu().numpy(), want), f'{key}: kernel != tests/warpref.py'
                if name == 'rotate7' and g == 4:
                    runs[key + ' (global path forced)'] = warp_call(d_mesh, prm, forced=True)
                    warp_call(d_mesh, prm, forced=True, dst=out2)()
                    torch.cuda.synchronize()
                    assert torch.equal(out, out2), 'the two paths gave different bytes'
    for _ in range(a.warmup):
        for fn in runs.values():
            window(fn, a.calls)
    t = {k: [] for k in runs}
    for _ in range(a.repeats):  # alternate
        for k, fn in runs.items():
            t[k].append(window(fn, a.calls))
    res = {'calls_per_window': a.calls, 'windows': a.repeats, 'device': torch.cuda.get_device_name(0), 'frames': N, 'width': W, 'height': H,
           'bytes_per_call': nbytes, 'tile_classes': classes, 'versions': {k: stats(v) for k, v in t.items()}}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'warp_ab.json'), 'w') as f:
        json.dump(res, f, indent=1)
    lines = [f'{N} frames {W}x{H} -> {W}x{H}; {a.repeats} windows per version, {a.calls} calls a window, alternating; {res["device"]}', '',
             '| version | median ms | min ms | max ms | GB/s (algorithmic) | against the copy | against upscale bicubic |', '|---|---|---|---|---|---|---|']
    v = res['versions']
    for k, x in v.items():
        lines.append(f'| {k} | {x["median_ms"]:.3f} | {x["min_ms"]:.3f} | {x["max_ms"]:.3f} | {x["gbps"]:.0f} | '
                     f'{x["median_ms"] / v["copy"]["median_ms"]:.2f}x | {x["median_ms"] / v["upscale bicubic"]["median_ms"]:.2f}x |')
    lines += ['', '| mesh | tiles a frame | of them on the global path |', '|---|---|---|']
    for k, c in classes.items():
        lines.append(f'| {k} | {c["tiles"]} | {c["fallback_tiles"]} |')
    for fname in ('bilinear', 'bicubic'):
        s, g = v[f'rotate7 {fname}'], v[f'rotate7 {fname} (global path forced)']
        verdict = 'faster' if s['max_ms'] < g['min_ms'] else 'slower' if s['min_ms'] > g['max_ms'] else 'equal within the spread'
        lines.append('')
        lines.append(f'rotate7 {fname}: staged against the forced global path: {verdict} ({g["median_ms"] / s["median_ms"]:.2f}x by the medians)')
    lines += ['', '(algorithmic bytes: every source frame read once, every destination sample written once. '
              '"faster" is claimed only where the two min..max ranges do not overlap.)']
    text = '\n'.join(lines) + '\n'
    with open(os.path.join(a.out, 'warp_ab.md'), 'w') as f:
        f.write(text)
    print(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
