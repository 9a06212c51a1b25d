"""The multipoint loop end to end: N synthetic 1080p streams are encoded by one BatchEncoder, decoded
by one BatchDecoder with frames out into one back-to-back buffer, and composed into one 1080p encoder per receiver
(encode_composed: background fill, a gallery of all N streams in the receiver's own order, frame step). A GPU tool, not
a test; it asserts nothing about the figures.

Per step (frames behind the first): the time of the whole loop (device events on the one stream everything runs on,
the upload of the synthetic frames excluded), of the receivers' encode_composed calls, and of fill plus compose alone
(the same fill and cells into a scratch canvas, timed on their own right after), and the share of the step that is.

usage: mosaic.py [--out profiles/compose/mosaic.md] [--streams 16] [--receivers 4] [--frames 8]
"""
import argparse, json, os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'openh264-wasm_amd'))
W, H = 1920, 1080


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'compose', 'mosaic.md'))
    ap.add_argument('--streams', type=int, default=16)
    ap.add_argument('--receivers', type=int, default=4)
    ap.add_argument('--frames', type=int, default=8)
    a = ap.parse_args()
    import torch
    import h264mi
    from h264mi.synth import SyntheticStream
    torch.cuda.set_device(0)
    N, R, NF = a.streams, a.receivers, a.frames
    fb = W * H * 3 // 2
    gs = [SyntheticStream(s, W, H) for s in range(N)]
    st = torch.cuda.Stream()
    bg = (16, 128, 128)
    with torch.cuda.stream(st):
        enc = h264mi.BatchEncoder(W, H, 4000000, N, stream=st)
        enc.set_frame_skip(False)
        dec = h264mi.BatchDecoder(W, H, N, stream=st)
        rx = [h264mi.BatchEncoder(W, H, 4000000, 1, stream=st) for _ in range(R)]
        for e in rx:
            e.set_frame_skip(False)
        decoded = torch.zeros(N * fb, dtype=torch.uint8, device='cuda')
        got = torch.zeros(N, dtype=torch.int32, device='cuda')
        scratch = torch.zeros(fb, dtype=torch.uint8, device='cuda')
    layouts = []
    for r in range(R):  # receiver r sees the streams rotated by r: its own picture last
        cells = h264mi.mosaic_cells(N, W, H, W, H)
        for k, c in enumerate(cells):
            c.src = (k + r + 1) % N
        layouts.append(cells)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    acc = {'step': [], 'composed': [], 'fill_compose': [], 'bytes': 0}
    for t in range(NF):
        src = torch.from_numpy(np.stack([np.ascontiguousarray(g.frame(t)) for g in gs])).cuda().view(-1)
        torch.cuda.synchronize()
        e0, e1, e2, e3 = ev(), ev(), ev(), ev()
        e0.record(st)
        enc.encode(src)
        sizes = enc.nal_sizes()  # synchronises
        dec.decode_frames(enc.nal_ptrs(), nal_sizes=sizes, out_ptrs=[decoded[s * fb:].data_ptr() for s in range(N)],
                          got_ptrs=[got[s:s + 1].data_ptr() for s in range(N)])
        e1.record(st)
        for e, cells in zip(rx, layouts):
            e.encode_composed(decoded, W, H, N, cells, bg=bg)
        e2.record(st)
        nb = [e.nal_sizes()[0] for e in rx]  # synchronises
        f0 = ev()
        f0.record(st)
        for cells in layouts:  # fill plus compose alone, as often as the step ran them
            h264mi.i420_fill(scratch, W, H, 1, *bg, stream=st)
            h264mi.i420_compose(scratch, W, H, 1, decoded, W, H, N, cells, stream=st)
        e3.record(st)
        e3.synchronize()
        assert got.cpu().tolist() == [1] * N and all(n > 0 for n in nb)
        acc['bytes'] += sum(nb)
        if t > 0:
            acc['step'].append(e0.elapsed_time(e2))
            acc['composed'].append(e1.elapsed_time(e2))
            acc['fill_compose'].append(f0.elapsed_time(e3))
        print(json.dumps({'frame': t, 'step_ms': round(e0.elapsed_time(e2), 3), 'encode_composed_ms': round(e1.elapsed_time(e2), 3),
                          'fill_compose_ms': round(f0.elapsed_time(e3), 3)}), flush=True)
    for x in [enc, dec] + rx:
        x.close()
    step, comp, fc = (float(np.mean(acc[k])) for k in ('step', 'composed', 'fill_compose'))
    row = {'streams': N, 'receivers': R, 'cell': f'{layouts[0][0].dw}x{layouts[0][0].dh}', 'ms_per_step': round(step, 3),
           'encode_composed_ms': round(comp, 3), 'fill_compose_ms': round(fc, 3), 'fill_compose_share': f'{100 * fc / step:.2f} %',
           'receiver_bytes': int(acc['bytes'])}
    print(json.dumps(row), flush=True)
    cols = list(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(f'# mosaic.py: {N} synthetic 1080p streams encoded, decoded with frames out, composed into {R} 1080p receiver encoders, '
                f'frames 0..{NF - 1}, frame skipping off, {h264mi.version()}, {torch.cuda.get_device_name(0)}\n\n')
        f.write('ms_per_step: encode of the N streams, decode, and the receivers\' encode_composed calls, mean over frames 1..; '
                'encode_composed_ms: the\nreceivers\' calls of it (fill, compose, frame step); fill_compose_ms: the same fills and cells into '
                'a scratch canvas, timed alone;\nfill_compose_share: of ms_per_step; receiver_bytes: all receivers, all frames.\n\n')
        f.write('| ' + ' | '.join(cols) + ' |\n|' + '---|' * len(cols) + '\n')
        f.write('| ' + ' | '.join(str(row[c]) for c in cols) + ' |\n')


if __name__ == '__main__':
    main()
