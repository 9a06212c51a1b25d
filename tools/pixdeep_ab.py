#!/usr/bin/env python3
"""The deeper and wider pixel layouts (ids 16..24; h264mi.pix_to_i420 / i420_to_pix, csrc/pixdeep.hip) measured by the
method of tools/pix_ab.py on 128 frames of 1280x720: each format tight, both directions, and P010 also at pitch 3072.

  pix   : the library call, everything in one launch (depth rule ROUND)
  torch : what a caller had before it -- strided views of the planes, integer tensor ops, copy_ plane by plane
  copy  : one device-to-device hipMemcpyAsync that moves the same number of bytes: the ceiling a pure move can reach

Each sample is one window of calls between two device events; the versions alternate, sample by sample, in the same
run. Reported per case: the median, minimum and maximum time of one call, GB/s from the bytes moved (the named bytes of
the source read once plus those of the destination written once) and that as a share of the copy's rate -- the figure
to read; the five formats of pixfmt.hip reached 92 to 103 % of it by this method (profiles/pixfmt/pix_ab.md). The bytes
of both versions are compared first, and one frame against tests/pixdeepref.py. The table asserts nothing. Writes
pixdeep_ab.json and pixdeep_ab.md into --out.

    python tools/pixdeep_ab.py --out profiles/pixdeep
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
    ap.add_argument('--calls', type=int, default=10, help='calls per timed window')
    ap.add_argument('--repeats', type=int, default=15, help='timed windows per version')
    ap.add_argument('--warmup', type=int, default=2, help='untimed windows per version')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pixdeep'))
    a = ap.parse_args()
    import numpy as np
    import torch
    import h264mi
    import pixref
    import pixdeepref as R
    if not torch.cuda.is_available():
        raise SystemExit('pixdeep_ab.py measures on the GPU: no device found')
    hip = h264mi._hiprt()
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    i16, i32, i64, u8 = torch.int16, torch.int32, torch.int64, torch.uint8

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

    def plane_views(buf, L, planes, u):
        """(n, rows, row units) strided views of the planes of the N frames in layout L at buf, in units of u bytes"""
        el = buf if u == 1 else buf.view(i16 if u == 2 else i32)
        return [torch.as_strided(el, (N, rows, rb // u), (L.frame_stride // u, L.pitch[p] // u, 1), L.offset[p] // u)
                for p, (rb, rows) in enumerate(planes)]

    def avg_rows(c):
        return (c[:, 0::2] + c[:, 1::2] + 1) >> 1

    def narrow(v):
        return torch.clamp((v + 2) >> 2, max=255).to(u8)

    def v210_fields(wd, ks, n):
        f = [(wd[:, :, k // 3::4] >> (10 * (k % 3))) & 1023 for k in ks]
        return torch.stack(f, dim=-1).reshape(N, H, -1)[:, :, :n]

    def torch_unpack(yuv, pl, pix):
        y, u, v = yuv
        if pix in (R.I422, R.I444, R.NV16, R.Y800):
            y.copy_(pl[0])
            if pix == R.Y800:
                u.fill_(128)
                v.fill_(128)
            elif pix == R.I444:
                for d, s in ((u, pl[1]), (v, pl[2])):
                    c = s.to(i16)
                    d.copy_(((c[:, 0::2, 0::2] + c[:, 0::2, 1::2] + c[:, 1::2, 0::2] + c[:, 1::2, 1::2] + 2) >> 2).to(u8))
            else:
                cb, cr = (pl[1], pl[2]) if pix == R.I422 else (pl[1][:, :, 0::2], pl[1][:, :, 1::2])
                u.copy_(avg_rows(cb.to(i16)).to(u8))
                v.copy_(avg_rows(cr.to(i16)).to(u8))
            return
        if pix == R.V210:
            wd = pl[0].to(i64) & 0xffffffff
            y.copy_(narrow(v210_fields(wd, (1, 3, 5, 7, 9, 11), W)))
            u.copy_(narrow(avg_rows(v210_fields(wd, (0, 4, 8), W // 2))))
            v.copy_(narrow(avg_rows(v210_fields(wd, (2, 6, 10), W // 2))))
            return
        val = (lambda t: (t.to(i32) & 0xffff) >> 6) if pix in (R.P010, R.P210) else (lambda t: t.to(i32) & 1023)
        y.copy_(narrow(val(pl[0])))
        cb, cr = (pl[1][:, :, 0::2], pl[1][:, :, 1::2]) if pix in (R.P010, R.P210) else (pl[1], pl[2])
        cb, cr = val(cb), val(cr)
        if pix in (R.P210, R.I210):
            cb, cr = avg_rows(cb), avg_rows(cr)
        u.copy_(narrow(cb))
        v.copy_(narrow(cr))

    def torch_pack(pl, yuv, pix):
        y, u, v = yuv
        u2, v2 = u.repeat_interleave(2, dim=1), v.repeat_interleave(2, dim=1)
        if pix in (R.I422, R.I444, R.NV16, R.Y800):
            pl[0].copy_(y)
            if pix == R.I422:
                pl[1].copy_(u2)
                pl[2].copy_(v2)
            elif pix == R.I444:
                pl[1].copy_(u2.repeat_interleave(2, dim=2))
                pl[2].copy_(v2.repeat_interleave(2, dim=2))
            elif pix == R.NV16:
                pl[1][:, :, 0::2].copy_(u2)
                pl[1][:, :, 1::2].copy_(v2)
            return
        if pix == R.V210:
            ng = (W + 5) // 6
            pad = lambda t, n: torch.nn.functional.pad(t.to(i64) << 2, (0, n - t.shape[2]))
            src = {'Y': pad(y, 6 * ng), 'Cb': pad(u2, 3 * ng), 'Cr': pad(v2, 3 * ng)}
            order = ('Cb0', 'Y0', 'Cr0', 'Y1', 'Cb1', 'Y2', 'Cr1', 'Y3', 'Cb2', 'Y4', 'Cr2', 'Y5')
            for wi in range(4):
                wd = 0
                for k in range(3):
                    name = order[3 * wi + k]
                    wd = wd | (src[name[:-1]][:, :, int(name[-1])::(6 if name[0] == 'Y' else 3)] << (10 * k))
                pl[0][:, :, wi::4].copy_(wd.to(i32))
            return
        word = (lambda t: (t.to(i32) << 8).to(i16)) if pix in (R.P010, R.P210) else (lambda t: t.to(i16) << 2)
        pl[0].copy_(word(y))
        cu, cv = (u, v) if pix in (R.P010, R.I010) else (u2, v2)
        if pix in (R.P010, R.P210):
            pl[1][:, :, 0::2].copy_(word(cu))
            pl[1][:, :, 1::2].copy_(word(cv))
        else:
            pl[1].copy_(word(cu))
            pl[2].copy_(word(cv))

    fb = pixref.frame_bytes(W, H)
    tight420 = pixref.tight(pixref.I420, W, H)
    pitched = pixref.Layout(R.P010, [3072, 3072], [0, 3072 * H], 3072 * (H + H // 2))
    assert R.layout_ok(pitched, W, H)
    cases = [(R.NAMES[p] + ' tight', R.tight(p, W, H)) for p in R.ALL] + [('P010 pitch 3072', pitched)]
    res = {'calls_per_window': a.calls, 'windows': a.repeats, 'device': torch.cuda.get_device_name(0), 'frames': N, 'size': [W, H], 'cases': {}}
    stream = h264mi._hip_stream(None)
    for name, L in cases:
        planes = R.planes(L.pix, W, H)
        named = sum(rb * rows for rb, rows in planes)
        total = N * L.frame_stride
        lay = h264mi.PixLayout(L.pix, L.pitch, L.offset, L.frame_stride)
        for direction in ('to layout', 'to I420'):
            pack = direction == 'to layout'
            src = torch.randint(0, 256, (N * fb if pack else total,), dtype=u8, device='cuda')
            out = [torch.zeros(total if pack else N * fb, dtype=u8, device='cuda') for _ in range(2)]
            moved = N * (fb + named) - (N * 2 * (W // 2) * (H // 2) if L.pix == R.Y800 and pack else 0)  # Y800 never reads the chroma
            half = moved // 2
            cp_src = torch.randint(0, 256, (half,), dtype=u8, device='cuda')
            cp_dst = torch.zeros(half, dtype=u8, device='cuda')
            i420_views = plane_views(src if pack else out[1], tight420, pixref.planes(pixref.I420, W, H), 1)
            pix_views = plane_views(out[1] if pack else src, L, planes, R.unit(L.pix))

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
                hip.hipMemcpyAsync(ctypes.c_void_p(cp_dst.data_ptr()), ctypes.c_void_p(cp_src.data_ptr()), half, 3, stream)

            lib_call()
            torch_call()
            copy_call()
            torch.cuda.synchronize()
            assert torch.equal(out[0], out[1]), f'{name} {direction}: kernel != torch'
            assert torch.equal(cp_dst, cp_src), 'the copy did not copy'
            last = (N - 1) * (L.frame_stride if pack else fb)  # the last frame against the numpy restatement
            if pack:
                want = R.pack(src[(N - 1) * fb:].cpu().numpy(), L, W, H, np.zeros(R.span(L, W, H), np.uint8))
                got = out[0][last:last + want.size].cpu().numpy()
            else:
                want = R.unpack(src[(N - 1) * L.frame_stride:].cpu().numpy(), L, W, H)
                got = out[0][last:last + fb].cpu().numpy()
            assert np.array_equal(got, want), 'kernel != tests/pixdeepref.py'
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
            d['ratio'] = d['torch']['median_ms'] / d['pix']['median_ms']
            res['cases'][f'{name}, {direction}'] = d
            del src, out, cp_src, cp_dst, i420_views, pix_views
            torch.cuda.empty_cache()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'pixdeep_ab.json'), 'w') as f:
        json.dump(res, f, indent=1)
    lines = [f'{N} frames {W}x{H}; {a.repeats} windows per version ({a.calls} calls a window), alternating; {res["device"]}', '',
             'For comparison: the five formats of pixfmt.hip reached 92 to 103 % of the copy\'s rate by this method (profiles/pixfmt/pix_ab.md).', '',
             '| case | version | median ms | min ms | max ms | GB/s (bytes moved) | of the copy\'s rate |', '|---|---|---|---|---|---|---|']
    for name, d in res['cases'].items():
        for k in ('pix', 'torch', 'copy'):
            x = d[k]
            share = f'{100 * x["share_of_copy"]:.0f} %' if k != 'copy' else ''
            lines.append(f'| {name} | {k} | {x["median_ms"]:.4f} | {x["min_ms"]:.4f} | {x["max_ms"]:.4f} | {x["gbps"]:.0f} | {share} |')
        lines.append(f'| {name} | pix against torch: {d["ratio"]:.1f}x by the medians | | | | | |')
    lines += ['', '(GB/s from the bytes moved: the named bytes of the source read once plus those of the destination written once. copy is '
              'one device-to-device hipMemcpyAsync of half that many bytes, which moves as many.)']
    text = '\n'.join(lines) + '\n'
    with open(os.path.join(a.out, 'pixdeep_ab.md'), 'w') as f:
        f.write(text)
    print(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
