"""Rate and distortion side by side: the 1080p synthetic content coded with the encoder's
quality records on (h264mi_enc_set_quality), so that a setting is judged by its bytes and by the PSNR / SSIM those
bytes bought. A GPU tool, not a test; bench.py does not call it.

  * table (default): 8 streams, frames 0..24, frame skipping off, at 1 and 8 Mbps; settings: 1, 2, 4, 8 slices (MB-row
    QP plan), then exact GOM rate control at one slice. Per setting: total bytes of all frames and streams, the mean
    and the minimum over frames and streams of PSNR-Y (dB, per frame from its SSE), the mean SSIM-Y, and the same
    means for frames 5..24 (behind the IDR and the rate control's settling, the span §3.7's byte counts use).
  * --cost: encode-only frames/s at 128 streams with the records off and on -- two encoders in one process, passes
    alternating, each pass timed with GPU events around `steps` frame steps issued without a host round trip --,
    and the quality launch alone on 128 pairs of 1080p frames (h264mi_i420_quality_dev, GPU events).

usage: rd_table.py [--out profiles/quality/rd_table.md] [--streams 8]
       rd_table.py --cost [--out profiles/quality/quality_cost.txt] [--streams 128] [--steps 48] [--passes 3]
Prints one JSON line per measurement and writes the table / the report.
"""
import argparse, ctypes, json, os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'openh264-wasm_amd'))
W, H = 1920, 1080
NF = 25
SETTINGS = (('slices 1', 1, False), ('slices 2', 2, False), ('slices 4', 4, False), ('slices 8', 8, False),
            ('slices 1, exact GOM', 1, True))


def clip(S, nf):
    """frames 0..nf-1 of S synthetic streams, resident on the GPU (one tensor of S frames per step)"""
    import torch
    from h264mi.synth import SyntheticStream
    gs = [SyntheticStream(s, W, H) for s in range(S)]
    return [torch.from_numpy(np.stack([np.ascontiguousarray(g.frame(t)) for g in gs])).cuda() for t in range(nf)]


def records(enc):
    """every stream's record of the last frame step, one copy"""
    import h264mi
    buf = (h264mi.Quality * enc.S)()
    h264mi._hip_memcpy_d2h(ctypes.addressof(buf), enc.quality_ptr(), 64 * enc.S)
    return list(buf)


def rd(frames, br, slices, gom, S):
    import h264mi
    enc = h264mi.BatchEncoder(W, H, br, S)
    enc.set_frame_skip(False)
    if gom:
        enc.set_gom_exact(True)
    enc.set_slices(slices)
    enc.set_quality(True)
    nbytes, psnr, ssim = [], [], []
    for t in range(NF):
        enc.encode(frames[t])
        nb = enc.nal_sizes()  # synchronises
        q = records(enc)
        assert all(r.coded == 1 for r in q) and all(n > 0 for n in nb)
        nbytes.append(sum(nb))
        psnr.append([h264mi.psnr(r.sse[0], W * H) for r in q])
        ssim.append([r.ssim_fix[0] / (r.windows[0] * 4294967296.0) for r in q])
    enc.close()
    psnr, ssim = np.array(psnr), np.array(ssim)
    return {'bytes': int(sum(nbytes)), 'psnr_y_mean': round(float(psnr.mean()), 3), 'psnr_y_min': round(float(psnr.min()), 3),
            'ssim_y_mean': round(float(ssim.mean()), 5), 'bytes_5_24': int(sum(nbytes[5:])),
            'psnr_y_mean_5_24': round(float(psnr[5:].mean()), 3), 'ssim_y_mean_5_24': round(float(ssim[5:].mean()), 5)}


def table(a):
    import h264mi
    frames = clip(a.streams, NF)
    rows = []
    for br in (1000000, 8000000):
        base = None
        for name, n, gom in SETTINGS:
            r = {'bitrate': br, 'setting': name}
            r.update(rd(frames, br, n, gom, a.streams))
            base = base or r
            r['bytes_vs_first'] = round(r['bytes'] / base['bytes'], 4)
            r['bytes_5_24_vs_first'] = round(r['bytes_5_24'] / base['bytes_5_24'], 4)
            r['psnr_y_mean_vs_first_db'] = round(r['psnr_y_mean'] - base['psnr_y_mean'], 3)
            r['psnr_y_mean_5_24_vs_first_db'] = round(r['psnr_y_mean_5_24'] - base['psnr_y_mean_5_24'], 3)
            print(json.dumps(r), flush=True)
            rows.append(r)
    cols = ['bitrate', 'setting', 'bytes', 'bytes_vs_first', 'psnr_y_mean', 'psnr_y_mean_vs_first_db', 'psnr_y_min', 'ssim_y_mean',
            'bytes_5_24', 'bytes_5_24_vs_first', 'psnr_y_mean_5_24', 'psnr_y_mean_5_24_vs_first_db', 'ssim_y_mean_5_24']
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(f'# rd_table.py: 1080p synthetic content, {a.streams} streams, frames 0..{NF - 1}, frame skipping off, {h264mi.version()}\n\n')
        f.write('Means and the minimum are over frames and streams; PSNR-Y in dB per frame from its SSE; _vs_first: against the\n'
                'first setting of the same bitrate (bytes as a ratio, PSNR as a difference in dB).\n\n')
        f.write('| ' + ' | '.join(cols) + ' |\n|' + '---|' * len(cols) + '\n')
        for r in rows:
            f.write('| ' + ' | '.join(str(r.get(c, '')) for c in cols) + ' |\n')


def cost(a):
    import torch
    import h264mi
    S, nclip = a.streams, 12
    frames = clip(S, nclip)
    st = torch.cuda.Stream()  # the encoders' stream, and the one the events are recorded on
    torch.cuda.synchronize()
    encs = {}
    for mode in ('off', 'on'):
        e = h264mi.BatchEncoder(W, H, 1000000, S, stream=st)
        e.set_frame_skip(False)
        e.set_quality(mode == 'on')
        encs[mode] = e
    lines, fps = [], {'off': [], 'on': []}
    t = {'off': 0, 'on': 0}

    def run(mode, steps):
        e = encs[mode]
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(st)
        for _ in range(steps):
            e.encode(frames[t[mode] % nclip])
            t[mode] += 1
        ev1.record(st)
        ev1.synchronize()
        e.nal_sizes()  # raises if a kernel reported an error
        return ev0.elapsed_time(ev1)

    for mode in ('off', 'on'):
        run(mode, 8)  # warm-up: the IDR and the rate control's first frames
    for p in range(a.passes):
        for mode in ('off', 'on'):
            ms = run(mode, a.steps)
            r = {'pass': p, 'quality': mode, 'streams': S, 'steps': a.steps, 'ms_per_step': round(ms / a.steps, 4),
                 'encode_frames_per_s': round(S * a.steps / ms * 1e3, 1)}
            fps[mode].append(r['encode_frames_per_s'])
            print(json.dumps(r), flush=True)
            lines.append(json.dumps(r))
    for e in encs.values():
        e.close()
    # the launch alone: S pairs of 1080p frames (two frames of the clip), clearing of the records included
    out = torch.zeros(8 * S, dtype=torch.int64, device='cuda')
    fa, fb = frames[0].view(-1), frames[1].view(-1)
    for _ in range(3):
        h264mi.i420_quality(out, fa, fb, W, H, S, stream=st)
    reps = 20
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record(st)
    for _ in range(reps):
        h264mi.i420_quality(out, fa, fb, W, H, S, stream=st)
    ev1.record(st)
    ev1.synchronize()
    ms = ev0.elapsed_time(ev1) / reps
    gb = 2 * S * W * H * 1.5 / 1e9
    k = {'quality_launch_ms': round(ms, 4), 'pairs': S, 'bytes_read_GB': round(gb, 4), 'GB_per_s': round(gb / ms * 1e3, 1)}
    print(json.dumps(k), flush=True)
    med = {m: float(np.median(v)) for m, v in fps.items()}
    s = {'median_encode_frames_per_s_off': med['off'], 'median_encode_frames_per_s_on': med['on'],
         'on_vs_off': round(med['on'] / med['off'], 4), 'ms_per_step_added': round(S * 1e3 / med['on'] - S * 1e3 / med['off'], 4)}
    print(json.dumps(s), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(f'rd_table.py --cost: 1080p synthetic content, 1 Mbps, frame skipping off, {S} streams, {h264mi.version()}\n')
        f.write(f'encode only, {a.steps} frame steps per pass between two GPU events, passes alternating off / on in one process\n')
        f.write('\n'.join(lines) + '\n' + json.dumps(s) + '\n')
        f.write('the quality launch alone (h264mi_i420_quality_dev, mean of 20 back-to-back calls between two GPU events):\n')
        f.write(json.dumps(k) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cost', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--streams', type=int, default=0)
    ap.add_argument('--steps', type=int, default=48)
    ap.add_argument('--passes', type=int, default=3)
    a = ap.parse_args()
    a.streams = a.streams or (128 if a.cost else 8)
    a.out = a.out or os.path.join(ROOT, 'profiles', 'quality', 'quality_cost.txt' if a.cost else 'rd_table.md')
    import torch
    torch.cuda.set_device(0)
    (cost if a.cost else table)(a)


if __name__ == '__main__':
    main()
