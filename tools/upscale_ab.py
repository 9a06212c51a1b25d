#!/usr/bin/env python3
"""The upscaler (h264mi.i420_upscale and h264mi.i420_compose_any, csrc/upscale.hip) measured at three workloads, each
with both filters:

  rung    : 128 frames 640x360 -> 1280x720
  hd      : 8 frames 960x540 -> 1920x1080
  speaker : the active-speaker layout (h264mi.speaker_cells) of 9 sources of 640x360 on each of 16 canvases of 1280x720,
            canvas c with speaker c % 9: per canvas one enlarging cell (960x540) and eight shrinking ones (160x90)

  upscale : the library call, everything in one call
  torch   : what a caller had before it -- the same integer definition written with torch tensor ops on the device
            (int32, the tap indices and weights of a geometry made once and kept), plane by plane, batched over the
            frames of a case; in `speaker` the shrinking cells go through h264mi.i420_compose, which the caller had

Each sample is one window of calls between two device events; the versions alternate, sample by sample, in the same
run. Reported per case: the median, minimum and maximum time of one call, GB/s from the algorithmic bytes (every used
source frame read once, every destination sample written once), that as a share of the 6.3 TB/s streaming ceiling, and
the verdict: "faster" only if the two min..max ranges do not overlap, otherwise "equal within the spread" or "slower".
The bytes of both versions are compared first, and one frame against tests/upscaleref.py. The table asserts nothing.
Writes upscale_ab.json and upscale_ab.md into --out.

    python tools/upscale_ab.py --out profiles/upscale
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'openh264-wasm_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
HBM_CEILING = 6.3e12
# name: (frames or canvases, source width, height, destination width, height)
CASES = {'rung': (128, 640, 360, 1280, 720), 'hd': (8, 960, 540, 1920, 1080), 'speaker': (16, 640, 360, 1280, 720)}
NSRC = 9


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=20, help='library calls per timed window')
    ap.add_argument('--torch-calls', type=int, default=2, help='torch rounds per timed window')
    ap.add_argument('--repeats', type=int, default=21, help='timed windows per version')
    ap.add_argument('--warmup', type=int, default=3, help='untimed windows per version')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'upscale'))
    a = ap.parse_args()
    import numpy as np
    import torch
    import h264mi
    import scaleref
    import upscaleref
    if not torch.cuda.is_available():
        raise SystemExit('upscale_ab.py measures on the GPU: no device found')

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
        return {'median_ms': med, 'min_ms': min(v), 'max_ms': max(v), 'gbps': nbytes / (med * 1e-3) / 1e9,
                'share_of_ceiling': nbytes / (med * 1e-3) / HBM_CEILING}

    def planes(frames, w, h):
        """(n, frame bytes) -> views (n, h, w), (n, h/2, w/2), (n, h/2, w/2)"""
        y, c = w * h, (w // 2) * (h // 2)
        return [frames[:, :y].view(-1, h, w), frames[:, y:y + c].view(-1, h // 2, w // 2), frames[:, y + c:y + 2 * c].view(-1, h // 2, w // 2)]

    taps_cache = {}

    def taps(p, q, filt):
        """the definition's indices and weights of one axis, made on the device once per geometry: (q, 4) int64 and int32"""
        if (p, q, filt) not in taps_cache:
            o = torch.arange(q, dtype=torch.int64, device='cuda')
            P = torch.div(16 * ((2 * o + 1) * p - q) + q, 2 * q, rounding_mode='floor')
            i, f = P >> 4, (P & 15).to(torch.int32)
            idx = torch.clamp(i[:, None] + torch.arange(-1, 3, device='cuda')[None, :], 0, p - 1)
            if filt == h264mi.FILTER_BICUBIC:
                w = [-f ** 3 + 32 * f ** 2 - 256 * f, 3 * f ** 3 - 80 * f ** 2 + 8192, -3 * f ** 3 + 64 * f ** 2 + 256 * f, f ** 3 - 16 * f ** 2]
            else:
                w = [0 * f, (16 - f) * 512, f * 512, 0 * f]
            taps_cache[(p, q, filt)] = (idx, torch.stack(w, dim=1).to(torch.int32))
        return taps_cache[(p, q, filt)]

    def torch_up(dst, src, filt):
        """src (n, ph, pw) uint8 -> dst (n, qh, qw) uint8 views, the definition in int32 tensor ops"""
        (xi, wx), (yi, wy) = taps(src.shape[2], dst.shape[2], filt), taps(src.shape[1], dst.shape[1], filt)
        c = src.to(torch.int32)
        ks = range(4) if filt == h264mi.FILTER_BICUBIC else (1, 2)
        h = sum(c[:, :, xi[:, k]] * wx[:, k][None, None, :] for k in ks)
        hh = (h + 16) >> 5
        v = sum(hh[:, yi[:, k], :] * wy[:, k][None, :, None] for k in ks)
        dst.copy_(torch.clamp((v + (1 << 20)) >> 21, 0, 255).to(torch.uint8))

    res = {'calls_per_window': a.calls, 'torch_calls_per_window': a.torch_calls, 'windows': a.repeats, 'device': torch.cuda.get_device_name(0),
           'cases': {}}
    for name, (n, sw, sh, dw, dh) in CASES.items():
        for filt, fname in ((h264mi.FILTER_BILINEAR, 'bilinear'), (h264mi.FILTER_BICUBIC, 'bicubic')):
            sfb, dfb = scaleref.frame_bytes(sw, sh), scaleref.frame_bytes(dw, dh)
            nsrc = NSRC if name == 'speaker' else n
            src = torch.randint(0, 256, (nsrc, sfb), dtype=torch.uint8, device='cuda')
            base = torch.randint(0, 256, (n, dfb), dtype=torch.uint8, device='cuda')
            out = [base.clone(), base.clone()]
            if name == 'speaker':
                cells = [h264mi.Cell(c.src, canvas, c.sx, c.sy, c.sw, c.sh, c.dx, c.dy, c.dw, c.dh)
                         for canvas in range(n) for c in h264mi.speaker_cells(NSRC, canvas % NSRC, sw, sh, dw, dh)]
                big = [c for c in cells if c.dw > c.sw]
                small = [c for c in cells if c.dw <= c.sw]
                assert len(big) == n and len(small) == n * (NSRC - 1) and all(c.dh >= c.sh for c in big) and all(c.dh <= c.sh for c in small)
                sp, dp = planes(src, sw, sh), planes(out[1], dw, dh)
                pairs = []  # whole sources: (rectangle view (1, qh, qw), source plane view (1, ph, pw)) per enlarging cell and plane
                for c in big:
                    for k in range(3):
                        s = 1 if k else 0
                        pairs.append((dp[k][c.canvas:c.canvas + 1, c.dy >> s:(c.dy + c.dh) >> s, c.dx >> s:(c.dx + c.dw) >> s], sp[k][c.src:c.src + 1]))

                def lib_call():
                    h264mi.i420_compose_any(out[0], dw, dh, n, src, sw, sh, nsrc, cells, filt)

                def torch_call():
                    h264mi.i420_compose(out[1], dw, dh, n, src, sw, sh, nsrc, small)
                    for d, s in pairs:
                        torch_up(d, s, filt)

                nbytes = nsrc * sfb + sum(1.5 * c.dw * c.dh for c in cells)
                what = f'{len(big)} cells 640x360 -> {big[0].dw}x{big[0].dh} and {len(small)} -> {small[0].dw}x{small[0].dh} on {n} canvases {dw}x{dh}'
                launches = 'compose ' + str(-(-len(small) // 64)) + ' + upscale ' + str(-(-len(big) // 64))
            else:
                sp, dp = planes(src, sw, sh), planes(out[1], dw, dh)

                def lib_call():
                    h264mi.i420_upscale(out[0], src, sw, sh, dw, dh, n, filt)

                def torch_call():
                    for d, s in zip(dp, sp):
                        torch_up(d, s, filt)

                nbytes = n * (sfb + dfb)
                what = f'{n} frames {sw}x{sh} -> {dw}x{dh}'
                launches = 'upscale 1'
            lib_call()
            torch_call()
            torch.cuda.synchronize()
            assert torch.equal(out[0], out[1]), f'{name} {fname}: kernel != torch'
            if name != 'speaker':  # the last frame against the numpy restatement
                want = upscaleref.up_frame(src[n - 1].cpu().numpy(), sw, sh, dw, dh, filt)
                assert np.array_equal(out[0][n - 1].cpu().numpy(), want), 'kernel != tests/upscaleref.py'
            runs = (('upscale', lib_call, a.calls), ('torch', torch_call, a.torch_calls))
            for _ in range(a.warmup):
                for _, fn, calls in runs:
                    window(fn, calls)
            t = {k: [] for k, _, _ in runs}
            for _ in range(a.repeats):  # alternate
                for k, fn, calls in runs:
                    t[k].append(window(fn, calls))
            d = {'what': what, 'filter': fname, 'launches': launches, 'bytes_per_call': nbytes, 'upscale': stats(t['upscale'], nbytes),
                 'torch': stats(t['torch'], nbytes)}
            if d['upscale']['max_ms'] < d['torch']['min_ms']:
                d['verdict'] = 'faster'
            elif d['upscale']['min_ms'] > d['torch']['max_ms']:
                d['verdict'] = 'slower'
            else:
                d['verdict'] = 'equal within the spread'
            d['ratio'] = d['torch']['median_ms'] / d['upscale']['median_ms']
            res['cases'][f'{name} {fname}'] = d
            del out, src, base, sp, dp
            if name == 'speaker':
                del pairs
            torch.cuda.empty_cache()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'upscale_ab.json'), 'w') as f:
        json.dump(res, f, indent=1)
    lines = [f'{a.repeats} windows per version ({a.calls} calls a window, torch {a.torch_calls}), alternating; {res["device"]}', '',
             '| case | version | launches | median ms | min ms | max ms | GB/s (algorithmic) | of 6.3 TB/s ceiling |', '|---|---|---|---|---|---|---|---|']
    for name, d in res['cases'].items():
        for k in ('upscale', 'torch'):
            x = d[k]
            lines.append(f'| {name} ({d["what"]}) | {k} | {d["launches"] if k == "upscale" else "torch ops"} | {x["median_ms"]:.4f} | {x["min_ms"]:.4f} | '
                         f'{x["max_ms"]:.4f} | {x["gbps"]:.0f} | {100 * x["share_of_ceiling"]:.1f} % |')
        lines.append(f'| {name} | upscale against torch: {d["verdict"]} ({d["ratio"]:.1f}x by the medians) | | | | | | |')
    lines += ['', '(algorithmic bytes: every used source frame read once, every destination sample written once. '
              '"faster" is claimed only where the two min..max ranges do not overlap.)']
    text = '\n'.join(lines) + '\n'
    with open(os.path.join(a.out, 'upscale_ab.md'), 'w') as f:
        f.write(text)
    print(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
