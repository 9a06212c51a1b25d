#!/usr/bin/env python3
"""The I420 compositor (h264mi.i420_compose, csrc/compose.hip) measured at the gallery workload: 8 canvases of
1920x1080, each a G x G gallery of G * G of 128 source frames of 1920x1080 (h264mi.mosaic_cells), G = 4 (480x270 cells,
4:1) and G = 3 (640x360 cells, 3:1).

  compose : h264mi.i420_compose, every cell of every canvas in one call (64 cells to a launch)
  copies  : what a caller had before it -- one h264mi.i420_scale of the used source frames to the cell size into a
            temporary, then three hipMemcpy2DAsync per cell (Y, Cb, Cr) into the canvases; the same bytes
  scaler  : h264mi.i420_scale of 128 frames 1920x1080 -> 640x360, §5.3's row re-measured in the same run as the
            yardstick

Each sample is one window of calls between two device events; the versions alternate, sample by sample, in the same
run. Reported per gallery: the median, minimum and maximum time of one call, GB/s from the algorithmic bytes (every
used source frame read once, every rectangle written once), that as a share of the 6.3 TB/s streaming ceiling, and the
verdict: "faster" only if the two min..max ranges do not overlap, otherwise "equal within the spread" or "slower". The
canvases of both versions are compared byte for byte first, and one cell against tests/composeref.py. Writes
compose_ab.json and compose_ab.md into --out.

    python tools/compose_ab.py --out profiles/compose
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
HBM_CEILING = 6.3e12
W, H, NSRC, NCANVAS = 1920, 1080, 128, 8


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=20, help='compose / scaler calls per timed window')
    ap.add_argument('--copy-calls', type=int, default=3, help='scale-and-copy rounds per timed window')
    ap.add_argument('--repeats', type=int, default=21, help='timed windows per version')
    ap.add_argument('--warmup', type=int, default=3, help='untimed windows per version')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'compose'))
    a = ap.parse_args()
    import numpy as np
    import torch
    import h264mi
    import composeref
    import scaleref
    if not torch.cuda.is_available():
        raise SystemExit('compose_ab.py measures on the GPU: no device found')
    hip = ctypes.CDLL('libamdhip64.so')
    hip.hipMemcpy2DAsync.restype = ctypes.c_int
    hip.hipMemcpy2DAsync.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                     ctypes.c_int, ctypes.c_void_p]
    fb = scaleref.frame_bytes(W, H)
    src = torch.randint(0, 256, (NSRC * fb,), dtype=torch.uint8, device='cuda')
    canv = [torch.zeros(NCANVAS * fb, dtype=torch.uint8, device='cuda') for _ in range(2)]
    hs = torch.cuda.current_stream().cuda_stream

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

    s360 = torch.zeros(NSRC * scaleref.frame_bytes(640, 360), dtype=torch.uint8, device='cuda')
    res = {'width': W, 'height': H, 'sources': NSRC, 'canvases': NCANVAS, 'calls_per_window': a.calls, 'copy_calls_per_window': a.copy_calls,
           'windows': a.repeats, 'device': torch.cuda.get_device_name(0), 'galleries': {}}
    for G in (4, 3):
        per = G * G
        used = NCANVAS * per  # source frames 0 .. used - 1, each in one cell
        cells = []
        for c in range(NCANVAS):
            for k, cell in enumerate(h264mi.mosaic_cells(per, W, H, W, H)):
                cell.src, cell.canvas = c * per + k, c
                cells.append(cell)
        dw, dh = cells[0].dw, cells[0].dh
        assert all((c.dw, c.dh) == (dw, dh) for c in cells)
        tfb = scaleref.frame_bytes(dw, dh)
        tmp = torch.zeros(used * tfb, dtype=torch.uint8, device='cuda')
        copies = []  # (dst, dpitch, src, spitch, width, height) of every plane of every cell
        for c in cells:
            t0, d0 = tmp.data_ptr() + c.src * tfb, canv[1].data_ptr() + c.canvas * fb
            copies.append((d0 + c.dy * W + c.dx, W, t0, dw, dw, dh))
            for p in range(2):
                copies.append((d0 + W * H + p * (W // 2) * (H // 2) + (c.dy // 2) * (W // 2) + c.dx // 2, W // 2,
                               t0 + dw * dh + p * (dw // 2) * (dh // 2), dw // 2, dw // 2, dh // 2))

        def compose():
            h264mi.i420_compose(canv[0], W, H, NCANVAS, src, W, H, NSRC, cells)

        def scale_and_copy():
            h264mi.i420_scale(tmp, src, W, H, dw, dh, used)
            for d, dp, s, sp, wd, ht in copies:
                if hip.hipMemcpy2DAsync(d, dp, s, sp, wd, ht, 3, hs) != 0:  # hipMemcpyDeviceToDevice
                    raise RuntimeError('hipMemcpy2DAsync failed')

        def scaler():
            h264mi.i420_scale(s360, src, W, H, 640, 360, NSRC)

        compose()
        scale_and_copy()
        torch.cuda.synchronize()
        assert torch.equal(canv[0], canv[1]), f'{G}x{G}: compose != scale and copy'
        c0 = cells[per - 1]
        want = composeref.compose(np.zeros((1, fb), np.uint8), W, H, src[:used * fb].cpu().numpy().reshape(used, fb)[c0.src:c0.src + 1], W, H,
                                  [composeref.C(0, 0, *composeref.as_tuple(c0)[2:])])
        ys = scaleref.planes(canv[0][:fb].cpu().numpy(), W, H)[0][c0.dy:c0.dy + dh, c0.dx:c0.dx + dw]
        assert np.array_equal(ys, scaleref.planes(want[0], W, H)[0][c0.dy:c0.dy + dh, c0.dx:c0.dx + dw]), 'kernel != tests/composeref.py'
        runs = (('compose', compose, a.calls), ('copies', scale_and_copy, a.copy_calls), ('scaler', scaler, a.calls))
        for _ in range(a.warmup):
            for _, fn, calls in runs:
                window(fn, calls)
        t = {k: [] for k, _, _ in runs}
        for _ in range(a.repeats):  # alternate
            for k, fn, calls in runs:
                t[k].append(window(fn, calls))
        nbytes = 1.5 * (W * H * used + dw * dh * len(cells))
        d = {'cells': len(cells), 'cell': f'{dw}x{dh}', 'enqueues_copies': 1 + len(copies), 'launches_compose': (len(cells) + 63) // 64,
             'bytes_per_call': nbytes, 'compose': stats(t['compose'], nbytes), 'copies': stats(t['copies'], nbytes),
             'scaler': stats(t['scaler'], 1.5 * (W * H + 640 * 360) * NSRC)}
        if d['compose']['max_ms'] < d['copies']['min_ms']:
            d['verdict'] = 'faster'
        elif d['compose']['min_ms'] > d['copies']['max_ms']:
            d['verdict'] = 'slower'
        else:
            d['verdict'] = 'equal within the spread'
        d['ratio'] = d['copies']['median_ms'] / d['compose']['median_ms']
        res['galleries'][f'{G}x{G}'] = d
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'compose_ab.json'), 'w') as f:
        json.dump(res, f, indent=1)
    lines = [f'{NCANVAS} canvases of {W}x{H}, each a G x G gallery of G * G of {NSRC} source frames of {W}x{H}; {a.repeats} windows per version '
             f'({a.calls} calls a window, scale-and-copy {a.copy_calls}), alternating; {res["device"]}', '',
             '| gallery | version | enqueues | median ms | min ms | max ms | GB/s (algorithmic) | of 6.3 TB/s ceiling |', '|---|---|---|---|---|---|---|---|']
    for name, d in res['galleries'].items():
        for k, enq in (('compose', d['launches_compose']), ('copies', d['enqueues_copies']), ('scaler', 1)):
            x = d[k]
            label = {'compose': f'compose ({d["cells"]} cells of {d["cell"]})', 'copies': 'scale + 3 copies per cell',
                     'scaler': f'scaler, {NSRC} frames 1080p -> 360p'}[k]
            lines.append(f'| {name} | {label} | {enq} | {x["median_ms"]:.4f} | {x["min_ms"]:.4f} | {x["max_ms"]:.4f} | {x["gbps"]:.0f} | '
                         f'{100 * x["share_of_ceiling"]:.1f} % |')
        lines.append(f'| {name} | compose against scale + copies: {d["verdict"]} ({d["ratio"]:.2f}x by the medians) | | | | | | |')
    lines += ['', '(algorithmic bytes: every used source frame read once, every rectangle written once; the scale-and-copy path moves the '
              'rectangles three times. "faster" is claimed only where the two min..max ranges do not overlap.)']
    text = '\n'.join(lines) + '\n'
    with open(os.path.join(a.out, 'compose_ab.md'), 'w') as f:
        f.write(text)
    print(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
