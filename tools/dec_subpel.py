"""Decode-only throughput on content with sub-sample motion: what the decoder's on-the-fly six-tap interpolation
(dec_recon.inc, dec_luma_frac) costs where it runs. bench.py's streams move by whole samples, so their vectors
are almost all whole-sample and the filters never run there.

One 1080p stream of SyntheticStream 0 seen through a window that moves by (5, 3) quarter luma samples per frame
(bilinear between the four integer neighbours, the generator of tests/test_recon_reference.subsample_frames) is
encoded on the GPU, IPPP, frame skipping off; the timed steps decode it in 8 decoders at once, batches of 16
frames, as bench.py --config 4 does. Prints frames/s and, from the encoder's own macroblock records
(h264mi_enc_mbinfo: type and the 16 block vectors), the share of inter macroblocks per fractional class -- whole
sample, b only (yFrac 0), h only (xFrac 0), positions that read j, other quarter positions -- and the share of
macroblocks whose blocks all lie inside the decoder's window.

usage: dec_subpel.py [--steps K] [--warmup W] [--clip N] [--decoders S] [--group G] [--bitrate B]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'openh264-wasm_amd'))

STEP = (5, 3)   # quarter luma samples per frame: every fractional phase in x and y comes round within four frames
J_POS = {6, 9, 10, 11, 14}   # yFrac * 4 + xFrac of the positions that read j (8.4.2.2.1)


def window(tex, qx, qy, w, h):
    ix, fx, iy, fy = qx >> 2, qx & 3, qy >> 2, qy & 3
    a = tex[iy:iy + h + 1, ix:ix + w + 1].astype(np.int32)
    top = (4 - fx) * a[:-1, :-1] + fx * a[:-1, 1:]
    bot = (4 - fx) * a[1:, :-1] + fx * a[1:, 1:]
    return (((4 - fy) * top + fy * bot + 8) >> 4).astype(np.uint8)


def frame(g, t, w, h):
    qx, qy = 16 + (STEP[0] * t) % 176, 16 + (STEP[1] * t) % 176   # inside the textures' 64-sample margin
    return np.concatenate([window(g.ty, qx, qy, w, h).ravel(), window(g.tu, qx >> 1, qy >> 1, w // 2, h // 2).ravel(),
                           window(g.tv, qx >> 1, qy >> 1, w // 2, h // 2).ravel()])


def classes(info, counts):
    """info: uint8 [macroblocks, 128] (MbInfo: type at 0, mv[16][2] int16 at 60)"""
    typ = info[:, 0]
    mv = info[:, 60:124].copy().view(np.int16).reshape(-1, 16, 2).astype(np.int32)
    inter = (typ >= 2) & (typ <= 6)
    pos = (mv[:, :, 1] & 3) * 4 + (mv[:, :, 0] & 3)
    whole = (pos == 0).all(axis=1)
    reads_j = np.isin(pos, list(J_POS)).any(axis=1)
    b_only = ~whole & ((mv[:, :, 1] & 3) == 0).all(axis=1)
    h_only = ~whole & ((mv[:, :, 0] & 3) == 0).all(axis=1)
    b4 = np.arange(16)
    lo_ok = hi_ok = np.ones(len(info), bool)
    for ax, p in ((0, 4 * (b4 & 3)), (1, 4 * (b4 >> 2))):
        f = (mv[:, :, ax] & 3) != 0
        d = p[None, :] + (mv[:, :, ax] >> 2)
        c = p[None, :] // 2 + (mv[:, :, ax] >> 3)
        lo_ok = lo_ok & ((d - 2 * f >= -24) & (c >= -12)).all(axis=1)
        hi_ok = hi_ok & ((d + 3 + 3 * f < 40) & (c + 2 < 20)).all(axis=1)
    counts['macroblocks'] += len(info)
    counts['inter'] += int(inter.sum())
    counts['whole'] += int((inter & whole).sum())
    counts['b_only'] += int((inter & b_only).sum())
    counts['h_only'] += int((inter & h_only).sum())
    counts['reads_j'] += int((inter & reads_j).sum())
    counts['other_quarter'] += int((inter & ~whole & ~b_only & ~h_only & ~reads_j).sum())
    counts['in_window'] += int((inter & lo_ok & hi_ok).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=192)
    ap.add_argument('--warmup', type=int, default=32)
    ap.add_argument('--clip', type=int, default=32)
    ap.add_argument('--decoders', type=int, default=8)
    ap.add_argument('--group', type=int, default=16)
    ap.add_argument('--bitrate', type=int, default=1000000)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--height', type=int, default=1080)
    a = ap.parse_args()
    import torch
    import h264mi
    from h264mi.synth import SyntheticStream
    assert torch.cuda.is_available(), 'dec_subpel.py needs a GPU'
    dev = torch.device('cuda:0')
    W, H, S, G, n = a.width, a.height, a.decoders, a.group, a.clip
    g = SyntheticStream(0, W, H)
    enc = h264mi.BatchEncoder(W, H, a.bitrate, 1)
    enc.set_frame_skip(False)
    slot = 1 << 21
    units = torch.empty((n, slot), dtype=torch.uint8, device=dev)
    usz = torch.zeros((n,), dtype=torch.int32, device=dev)
    nmb = ((W + 15) // 16) * ((H + 15) // 16)
    info = np.zeros((nmb, 128), np.uint8)
    counts = dict.fromkeys(['macroblocks', 'inter', 'whole', 'b_only', 'h_only', 'reads_j', 'other_quarter', 'in_window'], 0)
    for t in range(n):
        if t == 0:
            enc.force_idr(0)
        enc.encode(torch.from_numpy(np.ascontiguousarray(frame(g, t, W, H))).to(dev))
        enc.copy_nals(units[t], slot, usz[t:t + 1])
        torch.cuda.synchronize()
        assert enc._L.h264mi_enc_mbinfo(enc._e, 0, info.ctypes.data) == 0
        classes(info, counts)
    nbytes = usz.cpu().tolist()
    ds = torch.cuda.Stream(device=dev)
    dec = h264mi.BatchDecoder(W, H, S, stream=ds, max_frames=G)
    state = {'t': 0}

    def run_steps(k):
        with torch.cuda.stream(ds):
            while k > 0:
                m = min(G, k, n - state['t'] % n)   # a call never wraps past the clip end (the next one starts at the IDR)
                t0 = state['t'] % n
                dec.decode_frames([units[t0 + j].data_ptr() for j in range(m) for _ in range(S)],
                                  size_ptrs=[usz[t0 + j:t0 + j + 1].data_ptr() for j in range(m) for _ in range(S)])
                state['t'] += m
                k -= m

    run_steps(a.warmup)
    torch.cuda.synchronize()
    rc, got = dec.status()
    ok = rc == 0 and all(got)
    dec.set_timing(True)
    t0 = time.perf_counter()
    run_steps(a.steps)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    rms, rn = dec.kernel_time(0)
    pics = [dec.picture_i420(s) for s in range(S)]
    ok = ok and all(p == pics[0] for p in pics)
    bytes_dev = dec.device_bytes()
    dec.close()
    enc.close()
    inter = max(counts['inter'], 1)
    print(json.dumps({
        'metric': 'decode-only frames/sec, sub-sample motion', 'value': S * a.steps / el, 'ms_per_step': 1e3 * el / a.steps,
        'decoders': S, 'group': G, 'steps': a.steps, 'clip': n, 'mean_bytes_per_frame': sum(nbytes) // n,
        'dec_recon_kernel_avg_ms': rms / max(rn, 1), 'decoder_device_bytes': bytes_dev,
        'inter_share_of_macroblocks': counts['inter'] / max(counts['macroblocks'], 1),
        'share_of_inter_macroblocks': {k: round(counts[k] / inter, 4) for k in ('whole', 'b_only', 'h_only', 'reads_j', 'other_quarter', 'in_window')},
        'selfcheck_ok': bool(ok)}))
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
