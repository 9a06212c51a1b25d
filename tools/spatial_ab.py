#!/usr/bin/env python3
"""The spatial filter (h264mi.i420_spatial, csrc/spatial.hip) measured two ways. The tables assert nothing.

(a) timing, at 128 frames 1280x720 and 8 frames 1920x1080, for radius 1 and radius 3 on every plane (amount 40, core 2):
  spatial : the library call, one launch
  torch   : what a caller had before it -- replicate padding, the two binomial passes as float32 convolutions (exact:
            every value stays below 2^24), the sample rule as torch expressions
  copy    : one device-to-device hipMemcpyAsync of n frames (the filter's algorithmic traffic: one read and one write
            of a frame)
Each sample is one window of calls between two device events; the versions alternate, sample by sample, in the same
run. Reported: the median, minimum and maximum time of one call, GB/s from 2 x frame bytes x n, and that as a share of the
copy's rate. The bytes of both versions are compared first, and one frame against tests/spatialref.py.

(b) effect on coding: h264mi.synth content at 1920x1080 coded as a 640x360 rung through encode_scaled, one stream, at a
fixed bitrate, with the filter off and with (1, 1, 40, 40, 2); frame skipping off. Reported: bits per frame, the share of
P_Skip macroblocks over the P frames, and PSNR / SSIM of the reconstruction against the *unsharpened* rung (the
downscaled source). Numbers only.

Writes spatial_ab.json, spatial_ab.md and quality.md into --out.

    python tools/spatial_ab.py --out profiles/spatial
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
TIMING = (('batch', 128, 1280, 720), ('full-hd', 8, 1920, 1080))
SETTINGS = (('r=1', (1, 1, 40, 40, 2)), ('r=3', (3, 3, 40, 40, 2)))
RUNG = (1, 1, 40, 40, 2)
MI_PSKIP = 3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=10, help='calls per timed window')
    ap.add_argument('--repeats', type=int, default=21, help='timed windows per version')
    ap.add_argument('--warmup', type=int, default=2, help='untimed windows per version')
    ap.add_argument('--frames', type=int, default=24, help='frames per effect run')
    ap.add_argument('--bitrate', type=int, default=600000, help='the fixed bitrate of the rung')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'spatial'))
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    import h264mi
    import spatialref
    from h264mi.synth import SyntheticStream
    if not torch.cuda.is_available():
        raise SystemExit('spatial_ab.py measures on the GPU: no device found')
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
        y, c = w * h, (w // 2) * (h // 2)
        return [frames[:, :y].view(-1, h, w), frames[:, y:y + c].view(-1, h // 2, w // 2), frames[:, y + c:y + 2 * c].view(-1, h // 2, w // 2)]

    def torch_spatial(out, src, w, h, params):
        ry, rc, ay, ac, core = params
        for pl, (S, O) in enumerate(zip(planes(src, w, h), planes(out, w, h))):
            r, amount = (ry, ay) if pl == 0 else (rc, ac)
            x = S.to(torch.float32)[:, None]
            k = torch.tensor(spatialref.WEIGHTS[r], dtype=torch.float32, device='cuda')
            s = F.conv2d(F.conv2d(F.pad(x, (r, r, r, r), mode='replicate'), k.view(1, 1, 1, -1)), k.view(1, 1, -1, 1))
            d = x - torch.floor((s + (1 << (4 * r - 1))) / (1 << (4 * r)))
            o = (x + torch.floor((amount * d + 32) / 64)).clamp(0, 255)
            if amount > 0:
                o = torch.where(d.abs() <= core, x, o)
            O.copy_(o[:, 0].to(torch.uint8))

    res = {'calls_per_window': a.calls, 'windows': a.repeats, 'device': torch.cuda.get_device_name(0), 'timing': {}, 'effect': []}
    for name, n, w, h in TIMING:
        fb = spatialref.frame_bytes(w, h)
        g = SyntheticStream(0, w, h)
        base = torch.from_numpy(np.stack([np.ascontiguousarray(g.frame(t)).ravel() for t in range(4)])).cuda()
        src = base.repeat((n + 3) // 4, 1)[:n].contiguous()
        out = [torch.zeros((n, fb), dtype=torch.uint8, device='cuda') for _ in range(2)]
        big = torch.zeros((2, n * fb), dtype=torch.uint8, device='cuda')
        nbytes = 2 * fb * n
        stream = h264mi._hip_stream(None)
        for label, params in SETTINGS:
            def lib_call():
                h264mi.i420_spatial(out[0], src, w, h, n, params)

            def torch_call():
                torch_spatial(out[1], src, w, h, params)

            def copy_call():
                hip.hipMemcpyAsync(ctypes.c_void_p(big[1].data_ptr()), ctypes.c_void_p(big[0].data_ptr()), big[0].numel(), 3, stream)

            lib_call()
            torch_call()
            torch.cuda.synchronize()
            assert torch.equal(out[0], out[1]), f'{name} {label}: kernel != torch'
            assert np.array_equal(out[0][n - 1].cpu().numpy(), spatialref.spatial_frame(src[n - 1].cpu().numpy(), w, h, params)), 'kernel != tests/spatialref.py'
            runs = (('spatial', lib_call), ('torch', torch_call), ('copy', copy_call))
            for _ in range(a.warmup):
                for k, fn in runs:
                    window(fn, 2 if k == 'torch' else a.calls)
            t = {k: [] for k, _ in runs}
            for _ in range(a.repeats):  # alternate
                for k, fn in runs:
                    t[k].append(window(fn, 2 if k == 'torch' else a.calls))
            d = {'what': f'{n} frames {w}x{h}', 'params': params, 'bytes_per_call': nbytes}
            for k, _ in runs:
                d[k] = stats(t[k], nbytes)
            for k in ('spatial', 'torch'):
                d[k]['share_of_copy'] = d[k]['gbps'] / d['copy']['gbps']
            res['timing'][f'{name} {label}'] = d
        del out, big, src, base
        torch.cuda.empty_cache()

    # (b) the rung
    sw, sh, w, h = 1920, 1080, 640, 360
    cw, ch, nmb = (w + 15) // 16 * 16, (h + 15) // 16 * 16, ((w + 15) // 16) * ((h + 15) // 16)
    g = SyntheticStream(0, sw, sh)
    fb = spatialref.frame_bytes(w, h)
    for setting in (None, RUNG):
        enc = h264mi.BatchEncoder(w, h, a.bitrate, 1)
        enc.set_frame_skip(False)
        enc.set_spatial(setting)
        info = np.zeros((nmb, 128), np.uint8)
        rec = np.empty(cw * ch * 3 // 2, np.uint8)
        qrec = torch.zeros(64, dtype=torch.uint8, device='cuda')
        small = torch.zeros(fb, dtype=torch.uint8, device='cuda')
        bits, skips, psnr, ssim = [], [], [], []
        for t in range(a.frames):
            frames = torch.from_numpy(np.ascontiguousarray(g.frame(t)).ravel()).cuda()
            h264mi.i420_scale(small, frames, sw, sh, w, h, 1)
            enc.encode_scaled(frames, sw, sh)
            bits.append(8 * enc.nal_sizes()[0])
            assert enc._L.h264mi_enc_mbinfo(enc._e, 0, info.ctypes.data) == 0
            if t > 0:
                skips.append(float((info[:, 0] == MI_PSKIP).mean()))
            h264mi._hip_memcpy_d2h(rec.ctypes.data, enc.recon_ptr(0), rec.size)
            Y = rec[:cw * ch].reshape(ch, cw)[:h, :w]
            U = rec[cw * ch:cw * ch * 5 // 4].reshape(ch // 2, cw // 2)[:h // 2, :w // 2]
            V = rec[cw * ch * 5 // 4:].reshape(ch // 2, cw // 2)[:h // 2, :w // 2]
            tight = torch.from_numpy(np.concatenate([Y.ravel(), U.ravel(), V.ravel()])).cuda()
            h264mi.i420_quality(qrec, tight, small, w, h, 1)
            q = h264mi.quality_records(qrec, 1)[0].as_dict(w, h)
            psnr.append(q['psnr'][0])
            ssim.append(q['ssim'][0])
        enc.close()
        res['effect'].append({'rung': f'{sw}x{sh} -> {w}x{h}', 'spatial': 'off' if setting is None else str(setting), 'bitrate': a.bitrate,
                              'bits_per_frame': sum(bits) / len(bits), 'bits_per_p_frame': sum(bits[1:]) / (len(bits) - 1),
                              'pskip_share': sum(skips) / len(skips), 'psnr_y_vs_unsharpened_db': sum(psnr) / len(psnr),
                              'ssim_y_vs_unsharpened': sum(ssim) / len(ssim)})

    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'spatial_ab.json'), 'w') as f:
        json.dump(res, f, indent=1)
    lines = [f'timing: {a.repeats} windows per version ({a.calls} calls a window, 2 for torch), alternating; {res["device"]}; amount 40, core 2 on every plane', '',
             '| case | version | median ms | min ms | max ms | GB/s (2 x bytes) | of the copy\'s rate |', '|---|---|---|---|---|---|---|']
    for name, d in res['timing'].items():
        for k in ('spatial', 'torch', 'copy'):
            x = d[k]
            share = f'{100 * x["share_of_copy"]:.0f} %' if k != 'copy' else ''
            lines.append(f'| {name} ({d["what"]}) | {k} | {x["median_ms"]:.4f} | {x["min_ms"]:.4f} | {x["max_ms"]:.4f} | {x["gbps"]:.0f} | {share} |')
    lines += ['', '(GB/s from 2 x frame bytes x n: a frame read, a frame written. copy is one device-to-device hipMemcpyAsync of n frames, '
              'which reads and writes that much: the same traffic. No hardware counter was collected.)']
    text = '\n'.join(lines) + '\n'
    with open(os.path.join(a.out, 'spatial_ab.md'), 'w') as f:
        f.write(text)
    qlines = [f'one stream, {a.frames} frames of h264mi.synth content, {a.bitrate} bit/s, frame skipping off, through encode_scaled; PSNR and SSIM of the '
              'reconstruction\'s luma against the unsharpened rung (the downscaled source)', '',
              '| rung | spatial | bits / frame | bits / P frame | P_Skip share of P frames | PSNR-Y dB | SSIM-Y |', '|---|---|---|---|---|---|---|']
    for r in res['effect']:
        qlines.append(f'| {r["rung"]} | {r["spatial"]} | {r["bits_per_frame"]:.0f} | {r["bits_per_p_frame"]:.0f} | {100 * r["pskip_share"]:.1f} % | '
                      f'{r["psnr_y_vs_unsharpened_db"]:.2f} | {r["ssim_y_vs_unsharpened"]:.4f} |')
    qtext = '\n'.join(qlines) + '\n'
    with open(os.path.join(a.out, 'quality.md'), 'w') as f:
        f.write(qtext)
    print(text)
    print(qtext)
    return 0


if __name__ == '__main__':
    sys.exit(main())
