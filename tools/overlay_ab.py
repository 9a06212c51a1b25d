#!/usr/bin/env python3
"""The overlay blend (h264mi.i420_overlay, csrc/overlay.hip) measured at three workloads on 1920x1080 canvases:

  logos  : 128 canvases, one 256x128 logo each (one launch of 128 / 64 = 2)
  full   : 8 canvases, a full-frame overlay each
  labels : 8 canvases, 16 labels of 320x48 each

Every placement has a sprite of its own, so no sprite byte is served twice.

  overlay : h264mi.i420_overlay, every placement in one call
  torch   : what a caller had before it -- the same integer formula written with torch tensor ops on the device, int32
            intermediates, placement by placement on views of the same buffers; the same bytes

Each sample is one window of calls between two device events; the versions alternate, sample by sample, in the same
run. Reported per case: the median, minimum and maximum time of one call, GB/s from the algorithmic bytes (the sprite's
four planes read once, the rectangle's canvas bytes read once and written once), that as a share of the 6.3 TB/s
streaming ceiling, and the verdict: "faster" only if the two min..max ranges do not overlap, otherwise "equal within the
spread" or "slower". The canvases of both versions are compared byte for byte first, and one placement against
tests/overlayref.py. The table asserts nothing. Writes overlay_ab.json and overlay_ab.md into --out.

    python tools/overlay_ab.py --out profiles/overlay
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
W, H = 1920, 1080
# name: (canvases, sprite width, sprite height, placements per canvas)
CASES = {'logos': (128, 256, 128, 1), 'full': (8, 1920, 1080, 1), 'labels': (8, 320, 48, 16)}


def placements(ncanvas, ow, oh, per):
    """`per` disjoint ow x oh rectangles on each canvas, a sprite each, opacities 129..256"""
    import h264mi
    cols = max(1, (W - 64) // (ow + 16)) if ow < W else 1
    out = []
    for c in range(ncanvas):
        for k in range(per):
            dx = 0 if ow == W else 32 + (k % cols) * (ow + 16)
            dy = 0 if oh == H else 24 + (k // cols) * (oh + 8)
            assert dx + ow <= W and dy + oh <= H
            out.append(h264mi.Overlay(c * per + k, c, 0, 0, ow, oh, dx, dy, 129 + (c * per + k) % 128, 0))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=20, help='overlay calls per timed window')
    ap.add_argument('--torch-calls', type=int, default=2, help='torch rounds per timed window')
    ap.add_argument('--repeats', type=int, default=21, help='timed windows per version')
    ap.add_argument('--warmup', type=int, default=3, help='untimed windows per version')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'overlay'))
    a = ap.parse_args()
    import numpy as np
    import torch
    import h264mi
    import overlayref
    import scaleref
    if not torch.cuda.is_available():
        raise SystemExit('overlay_ab.py measures on the GPU: no device found')
    fb = scaleref.frame_bytes(W, H)

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

    def planes(buf, w, h, alpha):
        y, c = w * h, (w // 2) * (h // 2)
        out = [buf[:y].view(h, w), buf[y:y + c].view(h // 2, w // 2), buf[y + c:y + 2 * c].view(h // 2, w // 2)]
        return out + [buf[y + 2 * c:2 * y + 2 * c].view(h, w)] if alpha else out

    res = {'width': W, 'height': H, 'calls_per_window': a.calls, 'torch_calls_per_window': a.torch_calls, 'windows': a.repeats,
           'device': torch.cuda.get_device_name(0), 'cases': {}}
    for name, (ncanvas, ow, oh, per) in CASES.items():
        ovs = placements(ncanvas, ow, oh, per)
        nspr, sb = len(ovs), h264mi.i420a_bytes(ow, oh)
        spr = torch.randint(0, 256, (nspr * sb,), dtype=torch.uint8, device='cuda')
        base = torch.randint(0, 256, (ncanvas * fb,), dtype=torch.uint8, device='cuda')
        canv = [base.clone(), base.clone()]
        views = []  # per placement: (effective-alpha inputs, (canvas view, sprite view) per plane)
        for p in ovs:
            sp = planes(spr[p.sprite * sb:(p.sprite + 1) * sb], ow, oh, True)
            cp = planes(canv[1][p.canvas * fb:(p.canvas + 1) * fb], W, H, False)
            pairs = []
            for k in range(3):
                s = 1 if k else 0
                pairs.append((cp[k][p.dy >> s:(p.dy + p.h) >> s, p.dx >> s:(p.dx + p.w) >> s],
                              sp[k][p.sy >> s:(p.sy + p.h) >> s, p.sx >> s:(p.sx + p.w) >> s]))
            views.append((sp[3][p.sy:p.sy + p.h, p.sx:p.sx + p.w], p.opacity, pairs))

        def overlay():
            h264mi.i420_overlay(canv[0], W, H, ncanvas, spr, ow, oh, nspr, ovs)

        def torch_blend():
            for A, op, pairs in views:
                al = (A.to(torch.int32) * op + 128) >> 8
                ac = (al[0::2, 0::2] + al[0::2, 1::2] + al[1::2, 0::2] + al[1::2, 1::2] + 2) >> 2
                for k, (d, s) in enumerate(pairs):
                    x = ac if k else al
                    d.copy_(((d.to(torch.int32) * (255 - x) + s.to(torch.int32) * x + 127) // 255).to(torch.uint8))

        overlay()
        torch_blend()
        torch.cuda.synchronize()
        assert torch.equal(canv[0], canv[1]), f'{name}: kernel != torch'
        p = ovs[-1]
        want = overlayref.blend(base[p.canvas * fb:(p.canvas + 1) * fb].cpu().numpy()[None], W, H,  # the last placement alone: the
                                spr[p.sprite * sb:(p.sprite + 1) * sb].cpu().numpy()[None], ow, oh,  # others do not touch its rectangle
                                [overlayref.O(0, 0, *overlayref.as_tuple(p)[2:])])
        got = canv[0][p.canvas * fb:(p.canvas + 1) * fb].cpu().numpy()
        for k, (g, w_) in enumerate(zip(scaleref.planes(got, W, H), scaleref.planes(want[0], W, H))):
            s = 1 if k else 0
            rect = (slice(p.dy >> s, (p.dy + p.h) >> s), slice(p.dx >> s, (p.dx + p.w) >> s))
            assert np.array_equal(g[rect], w_[rect]), 'kernel != tests/overlayref.py'
        runs = (('overlay', overlay, a.calls), ('torch', torch_blend, a.torch_calls))
        for _ in range(a.warmup):
            for _, fn, calls in runs:
                window(fn, calls)
        t = {k: [] for k, _, _ in runs}
        for _ in range(a.repeats):  # alternate
            for k, fn, calls in runs:
                t[k].append(window(fn, calls))
        nbytes = sum(2.5 * q.w * q.h + 2 * 1.5 * q.w * q.h for q in ovs)  # sprite planes once, rectangle read and written
        launches, k0 = 0, 0
        while k0 < len(ovs):  # the host's split: placements of one launch share no sample
            k1 = k0 + 1
            while k1 < len(ovs) and k1 - k0 < 64 and not any(
                    q.canvas == ovs[k1].canvas and q.dx < ovs[k1].dx + ovs[k1].w and ovs[k1].dx < q.dx + q.w and q.dy < ovs[k1].dy + ovs[k1].h
                    and ovs[k1].dy < q.dy + q.h for q in ovs[k0:k1]):
                k1 += 1
            launches, k0 = launches + 1, k1
        d = {'canvases': ncanvas, 'placements': len(ovs), 'sprite': f'{ow}x{oh}', 'launches_overlay': launches, 'bytes_per_call': nbytes,
             'overlay': stats(t['overlay'], nbytes), 'torch': stats(t['torch'], nbytes)}
        if d['overlay']['max_ms'] < d['torch']['min_ms']:
            d['verdict'] = 'faster'
        elif d['overlay']['min_ms'] > d['torch']['max_ms']:
            d['verdict'] = 'slower'
        else:
            d['verdict'] = 'equal within the spread'
        d['ratio'] = d['torch']['median_ms'] / d['overlay']['median_ms']
        res['cases'][name] = d
        del views, canv, spr, base
        torch.cuda.empty_cache()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'overlay_ab.json'), 'w') as f:
        json.dump(res, f, indent=1)
    lines = [f'{W}x{H} canvases; {a.repeats} windows per version ({a.calls} calls a window, torch {a.torch_calls}), alternating; {res["device"]}', '',
             '| case | version | launches | median ms | min ms | max ms | GB/s (algorithmic) | of 6.3 TB/s ceiling |', '|---|---|---|---|---|---|---|---|']
    for name, d in res['cases'].items():
        what = f'{d["placements"]} of {d["sprite"]} on {d["canvases"]} canvases'
        for k in ('overlay', 'torch'):
            x = d[k]
            lines.append(f'| {name} ({what}) | {k} | {d["launches_overlay"] if k == "overlay" else "torch ops"} | {x["median_ms"]:.4f} | {x["min_ms"]:.4f} | '
                         f'{x["max_ms"]:.4f} | {x["gbps"]:.0f} | {100 * x["share_of_ceiling"]:.1f} % |')
        lines.append(f'| {name} | overlay against torch: {d["verdict"]} ({d["ratio"]:.1f}x by the medians) | | | | | | |')
    lines += ['', '(algorithmic bytes: every sprite plane of a placement read once, its rectangle of the canvas read once and written once. '
              '"faster" is claimed only where the two min..max ranges do not overlap.)']
    text = '\n'.join(lines) + '\n'
    with open(os.path.join(a.out, 'overlay_ab.md'), 'w') as f:
        f.write(text)
    print(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
