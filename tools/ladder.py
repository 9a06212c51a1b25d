"""One source, four renditions: S synthetic 1080p streams coded as an ABR ladder by four
BatchEncoders -- 1920x1080, 1280x720, 960x540, 640x360 -- all fed from one source buffer per step: the 1080p
encoder by encode(), the other three by encode_scaled(), which area-averages the source frames into the encoder's
input area on the device. Quality records are on, so every rung reports the PSNR / SSIM of its own scaled source
against its reconstruction. A GPU tool, not a test; it asserts nothing about the figures.

Per rung: total bytes of all frames and streams, mean PSNR-Y (dB, per frame from its SSE) and mean SSIM-Y over frames
and streams, and the mean time of one frame step (all S streams; device events around the rung's call, scale launch
included) over the frames behind the first.

usage: ladder.py [--out profiles/scale/ladder.md] [--streams 8] [--frames 12]
"""
import argparse, ctypes, json, os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'openh264-wasm_amd'))
W, H = 1920, 1080
RUNGS = ((1920, 1080, 4000000), (1280, 720, 2500000), (960, 540, 1200000), (640, 360, 700000))


def records(enc):
    """every stream's record of the last frame step, one copy"""
    import h264mi
    buf = (h264mi.Quality * enc.S)()
    h264mi._hip_memcpy_d2h(ctypes.addressof(buf), enc.quality_ptr(), 64 * enc.S)
    return list(buf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scale', 'ladder.md'))
    ap.add_argument('--streams', type=int, default=8)
    ap.add_argument('--frames', type=int, default=12)
    a = ap.parse_args()
    import torch
    import h264mi
    from h264mi.synth import SyntheticStream
    torch.cuda.set_device(0)
    S, NF = a.streams, a.frames
    gs = [SyntheticStream(s, W, H) for s in range(S)]
    st = torch.cuda.Stream()  # the encoders' stream, and the one the events are recorded on
    encs = []
    for w, h, br in RUNGS:
        e = h264mi.BatchEncoder(w, h, br, S, stream=st)
        e.set_frame_skip(False)
        e.set_quality(True)
        encs.append(e)
    acc = [{'bytes': 0, 'psnr': [], 'ssim': [], 'ms': []} for _ in RUNGS]
    for t in range(NF):
        src = torch.from_numpy(np.stack([np.ascontiguousarray(g.frame(t)) for g in gs])).cuda().view(-1)  # the one source buffer
        torch.cuda.synchronize()  # uploaded before the encoders' stream reads it
        for (w, h, _), e, r in zip(RUNGS, encs, acc):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record(st)
            if (w, h) == (W, H):
                e.encode(src)
            else:
                e.encode_scaled(src, W, H)
            ev1.record(st)
            ev1.synchronize()
            nb = e.nal_sizes()  # synchronises
            q = records(e)
            assert all(x.coded == 1 for x in q) and all(n > 0 for n in nb)
            r['bytes'] += sum(nb)
            r['psnr'] += [h264mi.psnr(x.sse[0], w * h) for x in q]
            r['ssim'] += [x.ssim_fix[0] / (x.windows[0] * 4294967296.0) for x in q]
            if t > 0:
                r['ms'].append(ev0.elapsed_time(ev1))
    for e in encs:
        e.close()
    rows = []
    for (w, h, br), r in zip(RUNGS, acc):
        row = {'rung': f'{w}x{h}', 'bitrate': br, 'input': 'encode' if (w, h) == (W, H) else 'encode_scaled', 'bytes': int(r['bytes']),
               'psnr_y_mean': round(float(np.mean(r['psnr'])), 3), 'ssim_y_mean': round(float(np.mean(r['ssim'])), 5),
               'ms_per_step': round(float(np.mean(r['ms'])), 3)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    cols = ['rung', 'bitrate', 'input', 'bytes', 'psnr_y_mean', 'ssim_y_mean', 'ms_per_step']
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(f'# ladder.py: {S} synthetic 1080p streams, frames 0..{NF - 1}, one source buffer per step, frame skipping off, '
                f'{h264mi.version()}, {torch.cuda.get_device_name(0)}\n\n')
        f.write('bytes: all frames and streams; PSNR-Y / SSIM-Y: each rung\'s own (scaled) source against its reconstruction, mean over\n'
                'frames and streams; ms_per_step: one frame step of all streams, mean over frames 1.., the scale launch included.\n\n')
        f.write('| ' + ' | '.join(cols) + ' |\n|' + '---|' * len(cols) + '\n')
        for r in rows:
            f.write('| ' + ' | '.join(str(r[c]) for c in cols) + ' |\n')


if __name__ == '__main__':
    main()
