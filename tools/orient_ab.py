#!/usr/bin/env python3
"""Rotating and mirroring (h264mi.i420_orient, csrc/orient.hip) measured at two workloads:

  batch    : 128 frames 1280x720, each of the eight orientations
  portrait : 8 frames 1080x1920 -> 1920x1080, ROT90 and ROT270

  orient : the library call, everything in one launch
  torch  : what a caller had before it -- torch.rot90 / flip / transpose(...).contiguous() plane by plane, batched over
           the frames of a case, copied into the destination's plane views
  copy   : one device-to-device hipMemcpyAsync of the same byte count: the ceiling a pure move can reach

Each sample is one window of calls between two device events; the versions alternate, sample by sample, in the same
run. Reported per case: the median, minimum and maximum time of one call, GB/s from the algorithmic bytes (2 x frame
bytes x n: every sample read once and written once), that as a share of the copy's rate, and the verdict against torch:
"faster" only if the two min..max ranges do not overlap, otherwise "equal within the spread" or "slower". The bytes of
both versions are compared first, and one frame against tests/orientref.py. The table asserts nothing.
Writes orient_ab.json and orient_ab.md into --out.

    python tools/orient_ab.py --out profiles/orient
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
NAMES = ('IDENTITY', 'ROT90', 'ROT180', 'ROT270', 'MIRROR', 'FLIP', 'TRANSPOSE', 'TRANSVERSE')
# (name, frames, source width, height, orientations)
CASES = (('batch', 128, 1280, 720, tuple(range(8))), ('portrait', 8, 1080, 1920, (1, 3)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=20, help='calls per timed window')
    ap.add_argument('--repeats', type=int, default=21, help='timed windows per version')
    ap.add_argument('--warmup', type=int, default=3, help='untimed windows per version')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'orient'))
    a = ap.parse_args()
    import numpy as np
    import torch
    import h264mi
    import orientref
    if not torch.cuda.is_available():
        raise SystemExit('orient_ab.py measures on the GPU: no device found')
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

    def planes(frames, w, h):
        """(n, frame bytes) -> views (n, h, w), (n, h/2, w/2), (n, h/2, w/2)"""
        y, c = w * h, (w // 2) * (h // 2)
        return [frames[:, :y].view(-1, h, w), frames[:, y:y + c].view(-1, h // 2, w // 2), frames[:, y + c:y + 2 * c].view(-1, h // 2, w // 2)]

    turn = {0: lambda p: p, 1: lambda p: torch.rot90(p, -1, (1, 2)), 2: lambda p: torch.flip(p, (1, 2)), 3: lambda p: torch.rot90(p, 1, (1, 2)),
            4: lambda p: torch.flip(p, (2,)), 5: lambda p: torch.flip(p, (1,)), 6: lambda p: p.transpose(1, 2),
            7: lambda p: torch.flip(p, (1, 2)).transpose(1, 2)}

    res = {'calls_per_window': a.calls, 'windows': a.repeats, 'device': torch.cuda.get_device_name(0), 'cases': {}}
    for name, n, sw, sh, orients in CASES:
        fb = orientref.frame_bytes(sw, sh)
        src = torch.randint(0, 256, (n, fb), dtype=torch.uint8, device='cuda')
        out = [torch.zeros((n, fb), dtype=torch.uint8, device='cuda') for _ in range(3)]
        nbytes = 2 * fb * n
        for orient in orients:
            dw, dh = h264mi.orient_size(orient, sw, sh)
            sp, dp = planes(src, sw, sh), planes(out[1], dw, dh)
            stream = h264mi._hip_stream(None)

            def lib_call():
                h264mi.i420_orient(out[0], src, sw, sh, n, orient)

            def torch_call():
                for d, s in zip(dp, sp):
                    d.copy_(turn[orient](s).contiguous())

            def copy_call():
                hip.hipMemcpyAsync(ctypes.c_void_p(out[2].data_ptr()), ctypes.c_void_p(src.data_ptr()), n * fb, 3, stream)

            lib_call()
            torch_call()
            copy_call()
            torch.cuda.synchronize()
            assert torch.equal(out[0], out[1]), f'{name} {NAMES[orient]}: kernel != torch'
            assert torch.equal(out[2], src), 'the copy did not copy'
            want = orientref.orient_frame(src[n - 1].cpu().numpy(), sw, sh, orient)  # the last frame against the numpy restatement
            assert np.array_equal(out[0][n - 1].cpu().numpy(), want), 'kernel != tests/orientref.py'
            runs = (('orient', lib_call), ('torch', torch_call), ('copy', copy_call))
            for _ in range(a.warmup):
                for _, fn in runs:
                    window(fn, a.calls)
            t = {k: [] for k, _ in runs}
            for _ in range(a.repeats):  # alternate
                for k, fn in runs:
                    t[k].append(window(fn, a.calls))
            d = {'what': f'{n} frames {sw}x{sh} -> {dw}x{dh}', 'orientation': NAMES[orient], 'bytes_per_call': nbytes}
            for k, _ in runs:
                d[k] = stats(t[k], nbytes)
            for k in ('orient', 'torch'):
                d[k]['share_of_copy'] = d[k]['gbps'] / d['copy']['gbps']
            if d['orient']['max_ms'] < d['torch']['min_ms']:
                d['verdict'] = 'faster'
            elif d['orient']['min_ms'] > d['torch']['max_ms']:
                d['verdict'] = 'slower'
            else:
                d['verdict'] = 'equal within the spread'
            d['ratio'] = d['torch']['median_ms'] / d['orient']['median_ms']
            res['cases'][f'{name} {NAMES[orient]}'] = d
        del out, src, sp, dp
        torch.cuda.empty_cache()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'orient_ab.json'), 'w') as f:
        json.dump(res, f, indent=1)
    lines = [f'{a.repeats} windows per version ({a.calls} calls a window), alternating; {res["device"]}', '',
             '| case | version | median ms | min ms | max ms | GB/s (2 x bytes) | of the copy\'s rate |', '|---|---|---|---|---|---|---|']
    for name, d in res['cases'].items():
        for k in ('orient', 'torch', 'copy'):
            x = d[k]
            share = f'{100 * x["share_of_copy"]:.0f} %' if k != 'copy' else ''
            lines.append(f'| {name} ({d["what"]}) | {k} | {x["median_ms"]:.4f} | {x["min_ms"]:.4f} | {x["max_ms"]:.4f} | {x["gbps"]:.0f} | {share} |')
        lines.append(f'| {name} | orient against torch: {d["verdict"]} ({d["ratio"]:.1f}x by the medians) | | | | | |')
    lines += ['', '(GB/s from 2 x frame bytes x n: every sample read once and written once. copy is one device-to-device '
              'hipMemcpyAsync of the same bytes. "faster" is claimed only where the two min..max ranges do not overlap.)']
    text = '\n'.join(lines) + '\n'
    with open(os.path.join(a.out, 'orient_ab.md'), 'w') as f:
        f.write(text)
    print(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
