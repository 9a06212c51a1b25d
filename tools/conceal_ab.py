#!/usr/bin/env python3
"""What slice-copy concealment costs. 1080p streams of the GPU encoder at 8 slices (8 distinct ones,
repeated over the decoder's streams), an IDR and 4 P pictures decoded one access unit per call:

  * 128 streams, kernel time per call from set_timing / kernel_time (parse side: dec_parse_kernel, dec_conceal_kernel,
    dec_resolve_kernel; reconstruction side: the reconstruction + deblocking launch): concealment off, on without loss,
    on with one of 8 slices lost in every stream of every P picture;
  * 1 stream (what a drop-in decoder slot is), wall time per synchronous call: streamed (the default there), not
    streamed, concealment on -- the last two differ by the conceal launch alone, the first two by the streaming that a
    concealing decoder gives up.

Usage: conceal_ab.py [--streams 128] [--reps 5] > profiles/conceal/conceal_ab.md"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'openh264-wasm_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=128)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    import torch
    import h264mi
    from h264mi.synth import SyntheticStream
    from test_syntax_streams import _split_nals
    torch.cuda.set_device(0)
    w, h, nsrc, nf, nsl, lost = 1920, 1080, 8, 5, 8, 3
    enc = h264mi.BatchEncoder(w, h, 4000000, nsrc)
    enc.set_frame_skip(False)
    enc.set_slices(nsl)
    gs = [SyntheticStream(s, w, h) for s in range(nsrc)]
    units = []
    for t in range(nf):
        enc.encode(torch.from_numpy(np.stack([np.ascontiguousarray(g.frame(t)) for g in gs])).cuda())
        nb = enc.nal_sizes()
        units.append([enc.nal_bytes(s, nb[s]) for s in range(nsrc)])
    enc.close()
    lossy = [units[0]] + [[b''.join(x for i, x in enumerate(_split_nals(u)) if i != lost) for u in fr] for fr in units[1:]]
    mbs_lost = (h264mi.slice_first_row(68, nsl, lost + 1) - h264mi.slice_first_row(68, nsl, lost)) * 120

    def upload(frames, S):
        dev = [[torch.from_numpy(np.frombuffer(fr[s % nsrc], np.uint8).copy()).cuda() for s in range(S)] for fr in frames]
        return dev, [[len(fr[s % nsrc]) for s in range(S)] for fr in frames]

    def run(S, conceal, frames, streamed=None, wall=False):
        dec = h264mi.BatchDecoder(w, h, S, groups=2 if wall else 0)
        dec.set_slice_waves(8)
        if streamed is not None:
            dec.set_streamed(streamed)
        dec.set_conceal(conceal)
        dev, sizes = upload(frames, S)
        mode = dec.streamed()
        best = None
        for rep in range(a.reps + 1):
            dec.set_timing(True)
            t0 = time.perf_counter()
            for f in range(nf):
                dec.decode_frames([d.data_ptr() for d in dev[f]], nal_sizes=sizes[f])
                if wall:
                    rc, got = dec.status()
            rc, got = dec.status()
            t1 = time.perf_counter()
            assert rc == 0 and got == [1] * S, (rc, got[:4])
            con = dec.concealed()[0]
            assert con == [mbs_lost if conceal and frames is lossy else 0] * S, con[:4]
            rec, nr = dec.kernel_time(0)
            par, npar = dec.kernel_time(1)
            cur = (par / npar, rec / nr, (t1 - t0) * 1e3 / nf)
            if rep > 0:  # the first repetition warms up
                best = cur if best is None else tuple(min(x, y) for x, y in zip(best, cur))
        dec.close()
        return best, mode

    S = a.streams
    print('# Slice-copy concealment: cost of the decode kernels (`tools/conceal_ab.py`)\n')
    print(f'1920x1080, 8 slices per picture, an IDR and 4 P pictures, one access unit per call, best of {a.reps} repetitions.\n')
    print(f'## {S} streams: kernel time per call (ms), HIP events around the launches\n')
    print('| case | parse + conceal + resolve | reconstruction + deblocking | streamed |')
    print('|---|---|---|---|')
    rows = [('concealment off, clean', 0, units), ('concealment on, clean', 1, units),
            (f'concealment on, slice {lost} of 8 lost in every P picture ({mbs_lost} MBs per picture)', 1, lossy)]
    for name, c, fr in rows:
        (par, rec, _), mode = run(S, c, fr)
        print(f'| {name} | {par:.3f} | {rec:.3f} | {mode} |')
    print('\n## 1 stream: wall time per synchronous call (ms), decode_frames + status\n')
    print('| case | per call | streamed |')
    print('|---|---|---|')
    for name, c, fr, st in (('concealment off, streamed (default)', 0, units, None), ('concealment off, not streamed', 0, units, 0),
                            ('concealment on, clean', 1, units, None), ('concealment on, one slice lost', 1, lossy, None)):
        (_, _, wl), mode = run(1, c, fr, streamed=st, wall=True)
        print(f'| {name} | {wl:.3f} | {mode} |')


if __name__ == '__main__':
    main()
