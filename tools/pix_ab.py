#!/usr/bin/env python3
"""Pixel formats and pitched layouts (h264mi.pix_to_i420 / i420_to_pix, csrc/pixfmt.hip) measured on 128 frames of
1280x720: each of the five formats tight, both directions, and NV12 also as a surface wider than the picture (pitch
1536, a multiple of 256; the chroma plane on row align16(h)).

  pix   : the library call, everything in one launch
  torch : what a caller had before it -- strided views of the planes, copy_ plane by plane (the 4:2:2 average in int16)
  copy  : one device-to-device hipMemcpyAsync that moves the same number of bytes (it reads and writes half of them each):
          the ceiling a pure move can reach

Each sample is one window of calls between two device events; the versions alternate, sample by sample, in the same
run. Reported per case: the median, minimum and maximum time of one call, GB/s from the bytes moved (the named bytes of
the source read once plus those of the destination written once), that as a share of the copy's rate, and the verdict
against torch: "faster" only if the two min..max ranges do not overlap. The bytes of both versions are compared first,
and one frame against tests/pixref.py. The table asserts nothing. Writes pix_ab.json and pix_ab.md into --out.

    python tools/pix_ab.py --out profiles/pixfmt
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
N, W, H = 128, 1280, 720


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=20, help='calls per timed window')
    ap.add_argument('--repeats', type=int, default=21, help='timed windows per version')
    ap.add_argument('--warmup', type=int, default=3, help='untimed windows per version')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pixfmt'))
    a = ap.parse_args()
    import numpy as np
    import torch
    import h264mi
    import pixref
    if not torch.cuda.is_available():
        raise SystemExit('pix_ab.py measures on the GPU: no device found')
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

    def plane_views(buf, L):
        """(n, rows, row bytes) strided views of the planes of the N frames in layout L at buf"""
        return [torch.as_strided(buf, (N, rows, rb), (L.frame_stride, L.pitch[p], 1), L.offset[p])
                for p, (rb, rows) in enumerate(pixref.planes(L.pix, W, H))]

    def torch_pack(pl, yuv, pix):
        y, u, v = yuv
        if pix == pixref.I420:
            for d, s in zip(pl, yuv):
                d.copy_(s)
        elif pix in (pixref.NV12, pixref.NV21):
            pl[0].copy_(y)
            first, second = (u, v) if pix == pixref.NV12 else (v, u)
            pl[1][:, :, 0::2].copy_(first)
            pl[1][:, :, 1::2].copy_(second)
        else:
            yo = 0 if pix == pixref.YUY2 else 1
            pl[0][:, :, yo::2].copy_(y)
            pl[0][:, :, 1 - yo::4].copy_(u.repeat_interleave(2, dim=1))
            pl[0][:, :, 3 - yo::4].copy_(v.repeat_interleave(2, dim=1))

    def torch_unpack(yuv, pl, pix):
        y, u, v = yuv
        if pix == pixref.I420:
            for d, s in zip(yuv, pl):
                d.copy_(s)
        elif pix in (pixref.NV12, pixref.NV21):
            y.copy_(pl[0])
            first, second = (u, v) if pix == pixref.NV12 else (v, u)
            first.copy_(pl[1][:, :, 0::2])
            second.copy_(pl[1][:, :, 1::2])
        else:
            yo = 0 if pix == pixref.YUY2 else 1
            y.copy_(pl[0][:, :, yo::2])
            for d, k in ((u, 1 - yo), (v, 3 - yo)):
                c = pl[0][:, :, k::4].to(torch.int16)
                d.copy_(((c[:, 0::2] + c[:, 1::2] + 1) >> 1).to(torch.uint8))

    fb = pixref.frame_bytes(W, H)
    tight420 = pixref.tight(pixref.I420, W, H)
    surface = pixref.Layout(pixref.NV12, [1536, 1536], [0, 1536 * H], 1536 * (H + 368))  # 368 = align16(H / 2) rows of chroma
    assert H % 16 == 0 and pixref.layout_ok(surface, W, H)
    cases = [(pixref.NAMES[p] + ' tight', pixref.tight(p, W, H)) for p in pixref.ALL] + [('NV12 pitch 1536', surface)]
    res = {'calls_per_window': a.calls, 'windows': a.repeats, 'device': torch.cuda.get_device_name(0), 'frames': N, 'size': [W, H], 'cases': {}}
    stream = h264mi._hip_stream(None)
    for name, L in cases:
        named = sum(rb * rows for rb, rows in pixref.planes(L.pix, W, H))
        total = N * L.frame_stride
        lay = h264mi.PixLayout(L.pix, L.pitch, L.offset, L.frame_stride)
        for direction in ('to layout', 'to I420'):
            pack = direction == 'to layout'
            src = torch.randint(0, 256, (N * fb if pack else total,), dtype=torch.uint8, device='cuda')
            out = [torch.zeros(total if pack else N * fb, dtype=torch.uint8, device='cuda') for _ in range(2)]
            moved = N * (fb + named)
            cp_src = torch.randint(0, 256, (moved // 2,), dtype=torch.uint8, device='cuda')
            cp_dst = torch.zeros(moved // 2, dtype=torch.uint8, device='cuda')
            i420_views = plane_views(src if pack else out[1], tight420)
            pix_views = plane_views(out[1] if pack else src, L)

            def lib_call():
                if pack:
                    h264mi.i420_to_pix(out[0], lay, src, W, H, N)
                else:
                    h264mi.pix_to_i420(out[0], src, lay, W, H, N)

            def torch_call():
                if pack:
                    torch_pack(pix_views, i420_views, L.pix)
                else:
                    torch_unpack(i420_views, pix_views, L.pix)

            def copy_call():
                hip.hipMemcpyAsync(ctypes.c_void_p(cp_dst.data_ptr()), ctypes.c_void_p(cp_src.data_ptr()), moved // 2, 3, stream)

            lib_call()
            torch_call()
            copy_call()
            torch.cuda.synchronize()
            assert torch.equal(out[0], out[1]), f'{name} {direction}: kernel != torch'
            assert torch.equal(cp_dst, cp_src), 'the copy did not copy'
            last = (N - 1) * (L.frame_stride if pack else fb)  # the last frame against the numpy restatement
            if pack:
                want = pixref.pack(src[(N - 1) * fb:].cpu().numpy(), L, W, H, np.zeros(pixref.span(L, W, H), np.uint8))
                got = out[0][last:last + want.size].cpu().numpy()
            else:
                want = pixref.unpack(src[(N - 1) * L.frame_stride:].cpu().numpy(), L, W, H)
                got = out[0][last:last + fb].cpu().numpy()
            assert np.array_equal(got, want), 'kernel != tests/pixref.py'
            runs = (('pix', lib_call), ('torch', torch_call), ('copy', copy_call))
            for _ in range(a.warmup):
                for _, fn in runs:
                    window(fn, a.calls)
            t = {k: [] for k, _ in runs}
            for _ in range(a.repeats):  # alternate
                for k, fn in runs:
                    t[k].append(window(fn, a.calls))
            d = {'what': f'{N} frames {W}x{H}', 'layout': repr(L), 'bytes_moved_per_call': moved}
            for k, _ in runs:
                d[k] = stats(t[k], moved)
            for k in ('pix', 'torch'):
                d[k]['share_of_copy'] = d[k]['gbps'] / d['copy']['gbps']
            if d['pix']['max_ms'] < d['torch']['min_ms']:
                d['verdict'] = 'faster'
            elif d['pix']['min_ms'] > d['torch']['max_ms']:
                d['verdict'] = 'slower'
            else:
                d['verdict'] = 'equal within the spread'
            d['ratio'] = d['torch']['median_ms'] / d['pix']['median_ms']
            res['cases'][f'{name}, {direction}'] = d
            del src, out, cp_src, cp_dst, i420_views, pix_views
            torch.cuda.empty_cache()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'pix_ab.json'), 'w') as f:
        json.dump(res, f, indent=1)
    lines = [f'{N} frames {W}x{H}; {a.repeats} windows per version ({a.calls} calls a window), alternating; {res["device"]}', '',
             '| case | version | median ms | min ms | max ms | GB/s (bytes moved) | of the copy\'s rate |', '|---|---|---|---|---|---|---|']
    for name, d in res['cases'].items():
        for k in ('pix', 'torch', 'copy'):
            x = d[k]
            share = f'{100 * x["share_of_copy"]:.0f} %' if k != 'copy' else ''
            lines.append(f'| {name} | {k} | {x["median_ms"]:.4f} | {x["min_ms"]:.4f} | {x["max_ms"]:.4f} | {x["gbps"]:.0f} | {share} |')
        lines.append(f'| {name} | pix against torch: {d["verdict"]} ({d["ratio"]:.1f}x by the medians) | | | | | |')
    lines += ['', '(GB/s from the bytes moved: the named bytes of the source read once plus those of the destination written once. copy is '
              'one device-to-device hipMemcpyAsync of half that many bytes, which moves as many. "faster" is claimed only where the two '
              'min..max ranges do not overlap.)']
    text = '\n'.join(lines) + '\n'
    with open(os.path.join(a.out, 'pix_ab.md'), 'w') as f:
        f.write(text)
    print(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
