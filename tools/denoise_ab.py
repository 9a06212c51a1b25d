#!/usr/bin/env python3
"""The temporal denoiser (h264mi.i420_denoise, csrc/denoise.hip) measured two ways. The table asserts nothing.

(a) timing, at 128 frames 1280x720 and 8 frames 1920x1080, out of place, without statistics:
  denoise : the library call, one launch
  torch   : what a caller had before it -- the block gate and the sample rule as torch expressions over int16 planes
  copy    : one device-to-device hipMemcpyAsync of three frame-sizes of bytes per frame (the filter's algorithmic
            traffic: two reads and one write)
Each sample is one window of calls between two device events; the versions alternate, sample by sample, in the same run.
Reported: the median, minimum and maximum time of one call, GB/s from 3 x frame bytes x n, and that as a share of the
copy's rate. The bytes of both versions are compared first, and one frame against tests/denoiseref.py.

(b) effect: h264mi.synth content -- as it is ('pan': the whole picture moves by (3, 2) samples a frame) and its frame 0
held ('still': a fixed camera) -- plus seeded Gaussian noise (sigma 2 and 4) at 176x144 and 1280x720, one stream, coded
at the benchmark's bitrate with the pre-filter off and with (128, 64, 12, 24); frame skipping off. Reported: bits per
frame, the share of P_Skip macroblocks over the P frames (h264mi_enc_mbinfo), and the luma PSNR of the reconstruction
against the *clean* source. Whether the filter helps is the result, whichever way it falls.

Writes denoise_ab.json and denoise_ab.md into --out.

    python tools/denoise_ab.py --out profiles/denoise
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
PARAMS = (128, 64, 12, 24)
MI_PSKIP = 3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=10, help='calls per timed window')
    ap.add_argument('--repeats', type=int, default=21, help='timed windows per version')
    ap.add_argument('--warmup', type=int, default=2, help='untimed windows per version')
    ap.add_argument('--frames', type=int, default=24, help='frames per effect run')
    ap.add_argument('--bitrate', type=int, default=1000000, help="the benchmark's default")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'denoise'))
    a = ap.parse_args()
    import numpy as np
    import torch
    import h264mi
    import denoiseref
    from h264mi.synth import SyntheticStream
    if not torch.cuda.is_available():
        raise SystemExit('denoise_ab.py measures on the GPU: no device found')
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

    ky, kc, T, motion = PARAMS

    def torch_denoise(out, cur, prev, w, h):  # sides that are multiples of 8: whole blocks only
        C, P, O = planes(cur, w, h), planes(prev, w, h), planes(out, w, h)
        d = [c.to(torch.int16) - p.to(torch.int16) for c, p in zip(C, P)]
        sad = d[0].abs().to(torch.int32).view(-1, h // 8, 8, w // 8, 8).sum(dim=(2, 4))
        moving = 4 * sad > motion * 64
        for pl in range(3):
            K, r = (ky, 8) if pl == 0 else (kc, 4)
            mv = moving.repeat_interleave(r, dim=1).repeat_interleave(r, dim=2)
            ab = d[pl].abs()
            k = torch.div(K * (T - ab).clamp(min=0), T, rounding_mode='floor')
            m = torch.where((ab < T) & ~mv, (ab * k + 128) >> 8, torch.zeros_like(ab))
            O[pl].copy_((C[pl].to(torch.int16) - torch.sign(d[pl]) * m).to(torch.uint8))

    res = {'calls_per_window': a.calls, 'windows': a.repeats, 'device': torch.cuda.get_device_name(0), 'params': PARAMS, 'timing': {}, 'effect': []}
    for name, n, w, h in TIMING:
        fb = denoiseref.frame_bytes(w, h)
        prev = torch.randint(0, 256, (n, fb), dtype=torch.uint8, device='cuda')
        noise = torch.randint(-5, 6, (n, fb), dtype=torch.int16, device='cuda')
        cur = (prev.to(torch.int16) + noise).clamp(0, 255).to(torch.uint8)
        pc = planes(cur, w, h)
        for pl, r in ((0, 8), (1, 4), (2, 4)):  # every fourth block of a block row moves
            pc[pl].view(n, h // 8, r, w // 8, r)[:, :, :, 3::4, :] = torch.randint(0, 256, (n, h // 8, r, len(range(3, w // 8, 4)), r), dtype=torch.uint8, device='cuda')
        del noise, pc
        out = [torch.zeros((n, fb), dtype=torch.uint8, device='cuda') for _ in range(2)]
        big = torch.zeros((2, 3 * n * fb // 2), dtype=torch.uint8, device='cuda')  # the copy: 1.5 n frames read, 1.5 written
        nbytes = 3 * fb * n
        stream = h264mi._hip_stream(None)

        def lib_call():
            h264mi.i420_denoise(out[0], cur, prev, w, h, n, PARAMS)

        def torch_call():
            torch_denoise(out[1], cur, prev, w, h)

        def copy_call():
            hip.hipMemcpyAsync(ctypes.c_void_p(big[1].data_ptr()), ctypes.c_void_p(big[0].data_ptr()), big[0].numel(), 3, stream)

        lib_call()
        torch_call()
        torch.cuda.synchronize()
        assert torch.equal(out[0], out[1]), f'{name}: kernel != torch'
        want, st = denoiseref.denoise_frame(cur[n - 1].cpu().numpy(), prev[n - 1].cpu().numpy(), w, h, PARAMS)
        assert np.array_equal(out[0][n - 1].cpu().numpy(), want), 'kernel != tests/denoiseref.py'
        runs = (('denoise', lib_call), ('torch', torch_call), ('copy', copy_call))
        for _ in range(a.warmup):
            for k, fn in runs:
                window(fn, 2 if k == 'torch' else a.calls)
        t = {k: [] for k, _ in runs}
        for _ in range(a.repeats):  # alternate
            for k, fn in runs:
                t[k].append(window(fn, 2 if k == 'torch' else a.calls))
        d = {'what': f'{n} frames {w}x{h}', 'bytes_per_call': nbytes, 'moving_blocks_last_frame': st[0], 'blocks': st[1]}
        for k, _ in runs:
            d[k] = stats(t[k], nbytes)
        for k in ('denoise', 'torch'):
            d[k]['share_of_copy'] = d[k]['gbps'] / d['copy']['gbps']
        res['timing'][name] = d
        del out, big, cur, prev
        torch.cuda.empty_cache()

    def psnr_y(x, y):
        mse = float(np.mean((x.astype(np.float64) - y.astype(np.float64)) ** 2))
        return 100.0 if mse == 0 else 10 * np.log10(65025.0 / mse)

    for w, h in ((176, 144), (1280, 720)):
        g = SyntheticStream(0, w, h)
        cw, ch, nmb = (w + 15) // 16 * 16, (h + 15) // 16 * 16, ((w + 15) // 16) * ((h + 15) // 16)
        # 'pan': the synthetic stream as it is, every sample moving by (3, 2) a frame; 'still': its frame 0 held, a fixed camera
        for content, sigma in (('pan', 2), ('pan', 4), ('still', 2), ('still', 4)):
            clean = [np.ascontiguousarray(g.frame(t if content == 'pan' else 0)).ravel() for t in range(a.frames)]
            rng = np.random.default_rng(1000 * sigma + w)
            noisy = [np.clip(np.rint(f + rng.normal(0, sigma, f.size)), 0, 255).astype(np.uint8) for f in clean]
            for setting in (None, PARAMS):
                enc = h264mi.BatchEncoder(w, h, a.bitrate, 1)
                enc.set_frame_skip(False)
                enc.set_denoise(setting)
                info = np.zeros((nmb, 128), np.uint8)
                rec = np.empty(cw * ch * 3 // 2, np.uint8)
                bits, skips, psnr = [], [], []
                for t in range(a.frames):
                    frames = torch.from_numpy(noisy[t]).cuda()
                    enc.encode(frames)
                    bits.append(8 * enc.nal_sizes()[0])
                    assert enc._L.h264mi_enc_mbinfo(enc._e, 0, info.ctypes.data) == 0
                    if t > 0:
                        skips.append(float((info[:, 0] == MI_PSKIP).mean()))
                    h264mi._hip_memcpy_d2h(rec.ctypes.data, enc.recon_ptr(0), rec.size)
                    psnr.append(psnr_y(rec[:cw * ch].reshape(ch, cw)[:h, :w], clean[t][:w * h].reshape(h, w)))
                enc.close()
                res['effect'].append({'size': f'{w}x{h}', 'content': content, 'sigma': sigma, 'denoise': 'off' if setting is None else str(setting),
                                      'bits_per_frame': sum(bits) / len(bits), 'bits_per_p_frame': sum(bits[1:]) / (len(bits) - 1),
                                      'pskip_share': sum(skips) / len(skips), 'psnr_y_vs_clean_db': sum(psnr) / len(psnr),
                                      'psnr_y_noisy_input_vs_clean_db': float(np.mean([psnr_y(n_[:w * h], c_[:w * h]) for n_, c_ in zip(noisy, clean)]))})

    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'denoise_ab.json'), 'w') as f:
        json.dump(res, f, indent=1)
    lines = [f'(a) timing: {a.repeats} windows per version ({a.calls} calls a window, 2 for torch), alternating; {res["device"]}; parameters {PARAMS}', '',
             '| case | version | median ms | min ms | max ms | GB/s (3 x bytes) | of the copy\'s rate |', '|---|---|---|---|---|---|---|']
    for name, d in res['timing'].items():
        for k in ('denoise', 'torch', 'copy'):
            x = d[k]
            share = f'{100 * x["share_of_copy"]:.0f} %' if k != 'copy' else ''
            lines.append(f'| {name} ({d["what"]}) | {k} | {x["median_ms"]:.4f} | {x["min_ms"]:.4f} | {x["max_ms"]:.4f} | {x["gbps"]:.0f} | {share} |')
    lines += ['', '(GB/s from 3 x frame bytes x n: two frames read, one written. copy is one device-to-device hipMemcpyAsync of 1.5 x '
              'frame bytes x n, which reads and writes that much: the same traffic. No hardware counter was collected.)', '',
              f'(b) effect: one stream, {a.frames} frames, {a.bitrate} bit/s, frame skipping off; PSNR of the reconstruction\'s luma against the clean source', '',
              '| size | content | sigma | denoise | bits / frame | bits / P frame | P_Skip share of P frames | PSNR-Y vs clean dB | noisy input vs clean dB |', '|---|---|---|---|---|---|---|---|---|']
    for r in res['effect']:
        lines.append(f'| {r["size"]} | {r["content"]} | {r["sigma"]} | {r["denoise"]} | {r["bits_per_frame"]:.0f} | {r["bits_per_p_frame"]:.0f} | {100 * r["pskip_share"]:.1f} % | '
                     f'{r["psnr_y_vs_clean_db"]:.2f} | {r["psnr_y_noisy_input_vs_clean_db"]:.2f} |')
    text = '\n'.join(lines) + '\n'
    with open(os.path.join(a.out, 'denoise_ab.md'), 'w') as f:
        f.write(text)
    print(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
