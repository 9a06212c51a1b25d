"""What n slices per picture buy and cost: n in {1, 2, 4, 8, 16} on the 1080p synthetic stream at
1 and 8 Mbps. A GPU tool, not a test; bench.py does not call it.

  * single-call C-ABI, warm, median of the repeats (the method of capi_latency.py: host buffers, one frame per call,
    the caller waits): IDR encode ms (force_key_frame before each), IDR decode ms, P-frame decode ms, bytes per
    frame. The slice count comes from H264MI_ENC_SLICES, read by init_encoder.
  * batch encoder, 128 streams, frame skipping off: enc_mb_kernel ms per launch (h264mi_enc_kernel_time) over
    frames 5..24 and the total bytes of those frames.
  * every line is compared with the n = 1 line of the same run (ratios); compare that line with another tree's.

usage: slices_ab.py [--out profiles/slices/slices_ab.md] [--streams 128] [--repeats 7] [--no-batch]
Prints one JSON line per measurement and writes a markdown table.
"""
import argparse, ctypes, json, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'openh264-wasm_amd'))
W, H = 1920, 1080
NS = (1, 2, 4, 8, 16)


def capi(L, frames, br, n, repeats):
    os.environ['H264MI_ENC_SLICES'] = str(n)
    try:
        assert L.init_encoder(W, H, br) == 0 and L.init_decoder(0) == 0
    finally:
        os.environ.pop('H264MI_ENC_SLICES', None)
    yuv = np.zeros(W * H * 3 // 2, np.uint8)
    ow, oh = ctypes.c_int(), ctypes.c_int()

    def enc(f, idr):
        if idr:
            L.force_key_frame()
        p, sz = ctypes.POINTER(ctypes.c_ubyte)(), ctypes.c_int(0)
        t0 = time.perf_counter()
        L.encode_frame_yuv_i420(f.ctypes.data_as(ctypes.c_void_p), W, H, ctypes.byref(p), ctypes.byref(sz))
        dt = (time.perf_counter() - t0) * 1e3
        return dt, (np.frombuffer(ctypes.string_at(p, sz.value), np.uint8).copy() if sz.value > 0 else None)

    def dec(nal):
        t0 = time.perf_counter()
        L.decode_frame_yuv_i420(0, nal.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(int(nal.size)),
                                yuv.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ow), ctypes.byref(oh))
        dt = (time.perf_counter() - t0) * 1e3
        assert (ow.value, oh.value) == (W, H)
        return dt

    enc(frames[0], True)  # warm-up: allocations
    ie, idd, pd, ib, pb = [], [], [], [], []
    for r in range(repeats):  # an IDR, then the P frames the rate control codes behind it
        dt, nal = enc(frames[0], True)
        ie.append(dt); ib.append(int(nal.size)); idd.append(dec(nal))
        for k in range(45):  # the wrapper's frame skipping drops frames behind an IDR: go on to the first coded P frame
            dt, nal = enc(frames[1 + k % (len(frames) - 1)], False)
            if nal is not None:
                pb.append(int(nal.size)); pd.append(dec(nal))
                break
    L.deinit_decoder(0)
    med = lambda v: round(float(np.median(v)), 3) if v else None
    return {'idr_encode_ms': med(ie), 'idr_decode_ms': med(idd), 'p_decode_ms': med(pd), 'idr_bytes': med(ib), 'p_bytes': med(pb),
            'p_frames': len(pd)}


def batch_clip(S):
    """frames 0..24 of S synthetic streams, resident on the GPU (one tensor of S frames per step)"""
    import torch
    from h264mi.synth import SyntheticStream
    gs = [SyntheticStream(s, W, H) for s in range(S)]
    return [torch.from_numpy(np.stack([np.ascontiguousarray(g.frame(t)) for g in gs])).cuda() for t in range(25)]


def batch(clip, br, n, S):
    import h264mi
    enc = h264mi.BatchEncoder(W, H, br, S)
    enc.set_frame_skip(False)
    enc.set_slices(n)
    total = 0
    for t in range(25):
        if t == 5:
            enc.set_timing(True)
        enc.encode(clip[t])
        nb = enc.nal_sizes()
        if t >= 5:
            total += sum(nb)
    ms, k = enc.kernel_time()
    enc.close()
    return {'enc_mb_kernel_ms': round(ms / max(k, 1), 4), 'launches': k, 'bytes_frames_5_24': total}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'slices', 'slices_ab.md'))
    ap.add_argument('--streams', type=int, default=128)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--no-batch', action='store_true')
    a = ap.parse_args()
    import torch
    import h264mi
    from h264mi.synth import SyntheticStream
    torch.cuda.set_device(0)
    L = h264mi.lib()
    src = SyntheticStream(0, W, H)
    frames = [np.ascontiguousarray(src.frame(t)) for t in range(4)]
    rows = []
    clip = None if a.no_batch else batch_clip(a.streams)
    for br in (1000000, 8000000):
        base = None
        for n in NS:
            r = {'bitrate': br, 'slices': n}
            r.update(capi(L, frames, br, n, a.repeats))
            if not a.no_batch:
                r.update(batch(clip, br, n, a.streams))
            base = base or r
            for k in ('idr_encode_ms', 'idr_decode_ms', 'p_decode_ms', 'idr_bytes', 'p_bytes', 'enc_mb_kernel_ms', 'bytes_frames_5_24'):
                if r.get(k) and base.get(k):
                    r[k + '_vs_n1'] = round(r[k] / base[k], 3)
            print(json.dumps(r), flush=True)
            rows.append(r)
    cols = ['bitrate', 'slices', 'idr_encode_ms', 'idr_decode_ms', 'idr_decode_ms_vs_n1', 'p_decode_ms', 'idr_bytes', 'idr_bytes_vs_n1',
            'p_bytes', 'p_bytes_vs_n1', 'enc_mb_kernel_ms', 'enc_mb_kernel_ms_vs_n1', 'bytes_frames_5_24_vs_n1']
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(f'# slices_ab.py: 1080p synthetic stream, {h264mi.version()}\n\n')
        f.write('| ' + ' | '.join(cols) + ' |\n|' + '---|' * len(cols) + '\n')
        for r in rows:
            f.write('| ' + ' | '.join(str(r.get(c, '')) for c in cols) + ' |\n')


if __name__ == '__main__':
    main()
