"""GPU: slice-copy concealment of lost slices (h264mi_dec_set_conceal / H264MI_DEC_CONCEAL). The rule is
exact, so every check is bit for bit: the GPU decoder, concealment on, decodes the lossy access units; the oracle
decodes the full ones (tests/concealgen.py: at the place of each gap an all-skip slice with the donor's QP and
loop-filter fields); every picture, and every later picture of the sequence, must be equal, and concealed() must be
the macroblock count of the lost slices. Both modes of set_resolve run every small case."""
import os
import subprocess
import sys

import numpy as np
import pytest

from concealgen import Pair, runs
from streamgen import BitWriter, nal
from test_syntax_streams import _split_nals

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L4 = [dict(first=0, qp_delta=1), dict(first=25, qp_delta=-3, dbk=(0, 2, -1)), dict(first=52), dict(first=80, qp_delta=4, dbk=(2, -1, 1))]


class Dec:
    """a BatchDecoder fed from host bytes: decode(frames) with frames[f][s] -> (status rc, got[f][s], pictures[f][s])"""

    def __init__(self, w, h, S=1, B=1, resolve=1, conceal=1, waves=1):
        import h264mi
        self.w, self.h, self.S = w, h, S
        self.dec = h264mi.BatchDecoder(w, h, S, max_frames=B)
        self.dec.set_resolve(resolve)
        self.dec.set_slice_waves(waves)
        self.dec.set_conceal(conceal)

    def decode(self, frames):
        import torch
        n, S, fb = len(frames), self.S, self.w * self.h * 3 // 2
        flat = [u for fr in frames for u in fr]
        assert len(flat) == n * S
        dev = [torch.from_numpy(np.frombuffer(u, np.uint8).copy()).cuda() for u in flat]
        out = torch.zeros((n * S, fb), dtype=torch.uint8, device='cuda')
        got = torch.full((n * S,), -1, dtype=torch.int32, device='cuda')
        self.dec.decode_frames([d.data_ptr() for d in dev], nal_sizes=[len(u) for u in flat],
                               out_ptrs=[out[i].data_ptr() for i in range(n * S)], got_ptrs=[got[i:].data_ptr() for i in range(n * S)])
        rc, _ = self.dec.status()
        g, o = got.cpu().numpy().reshape(n, S).tolist(), out.cpu().numpy().reshape(n, S, fb)
        return rc, g, o

    def one(self, unit):
        rc, g, o = self.decode([[unit]])
        return rc, g[0][0], o[0][0]

    def close(self):
        self.dec.close()


def _follow(dec, od, full, lossy, nlost, what):
    """the oracle on the full unit, the GPU on the lossy one: the same picture, and the concealed count"""
    rc, pic, _, _ = od.decode(full)
    assert rc == 1, what
    grc, got, out = dec.one(lossy)
    assert (grc, got) == (0, 1), f'{what}: status {grc}, got {got}'
    assert np.array_equal(out, pic), f'{what}: {int(np.count_nonzero(out != pic))} samples differ'
    assert dec.dec.concealed() == [[nlost]], what


@pytest.mark.parametrize('resolve', [1, 0])
def test_positions(gpu_lib, oracle, resolve):
    """4 slices with mid-row boundaries; lose the first, a middle one (the rest permuted), the last, two adjacent ones,
    the first and the last; a clean picture after each lossy one predicts from the concealed reference"""
    g, od, dec = Pair(11, 9, seed=71, init_qp=27), oracle.decoder(), Dec(176, 144, resolve=resolve, waves=2)
    u = g.idr(slices=L4)
    _follow(dec, od, u, u, 0, 'idr')
    for lost, order in (((0,), None), ((1,), [3, 0, 2]), ((3,), None), ((1, 2), None), ((0, 3), [2, 1])):
        full, lossy, nlost = g.lossy(L4, lost, order=order)
        assert nlost > 0 and len(_split_nals(lossy)) == 4 - len(lost)
        _follow(dec, od, full, lossy, nlost, f'lost {lost}')
        full, clean, _ = g.lossy(L4, ())
        assert full == clean
        _follow(dec, od, full, clean, 0, f'clean after {lost}')
    dec.close()


FILTER = {
    'I-slice neighbours': ([dict(first=0, intra=True, qp_delta=-2), dict(first=25), dict(first=52, intra=True), dict(first=80)], (1,)),
    'donor idc 2 with offsets': ([dict(first=0, dbk=(2, 3, -2)), dict(first=25), dict(first=52, dbk=(0, -3, 2)), dict(first=80)], (1,)),
    'donor idc 2, last slice': ([dict(first=0), dict(first=25), dict(first=52, dbk=(2, -2, 3), qp_delta=5), dict(first=80)], (3,)),
    'donor idc 1': ([dict(first=0, dbk=(1, 0, 0)), dict(first=25), dict(first=52), dict(first=80)], (1,)),
    'donor idc 1, first slice lost': ([dict(first=0), dict(first=25, dbk=(1, 0, 0), qp_delta=-6), dict(first=52), dict(first=80)], (0,)),
    'QPs 20 apart': ([dict(first=0, qp_delta=-10), dict(first=25), dict(first=52, qp_delta=10), dict(first=80)], (1,)),
}


@pytest.mark.parametrize('resolve', [1, 0])
@pytest.mark.parametrize('name', list(FILTER))
def test_filter_classes_at_gap_edges(gpu_lib, oracle, name, resolve):
    layout, lost = FILTER[name]
    g, od, dec = Pair(11, 9, seed=80 + len(name), init_qp=28, cqp=-3), oracle.decoder(), Dec(176, 144, resolve=resolve)
    u = g.idr(slices=L4)
    _follow(dec, od, u, u, 0, 'idr')
    for k, lo in enumerate(((), lost, ())):
        full, lossy, nlost = g.lossy(layout, lo)
        _follow(dec, od, full, lossy, nlost, f'{name} picture {k}')
    dec.close()


@pytest.mark.parametrize('resolve', [1, 0])
def test_failed_and_short_slice(gpu_lib, oracle, resolve):
    """a slice whose data cannot parse (same header, one mb_skip_run larger than the picture) counts as lost; a good
    slice that ends before the next received one leaves a gap that starts mid-row"""
    g, od, dec = Pair(11, 9, seed=91), oracle.decoder(), Dec(176, 144, resolve=resolve, waves=4)
    u = g.idr(slices=L4)
    _follow(dec, od, u, u, 0, 'idr')
    full, lossy, nlost = g.lossy(L4, (2,), failed=(2,))
    assert len(_split_nals(lossy)) == 4
    bad = oracle.decoder()
    assert bad.decode(u)[0] == 1 and bad.decode(lossy)[0] != 1, 'the oracle must not accept the failed slice'
    _follow(dec, od, full, lossy, nlost, 'failed slice')
    full, lossy, nlost = g.lossy(L4, (0,), failed=(0,), order=[1, 0, 3, 2])
    _follow(dec, od, full, lossy, nlost, 'failed first slice, permuted')
    short = [dict(first=0), dict(first=25, qp_delta=-5, dbk=(0, 1, 1)), dict(first=30), dict(first=52), dict(first=80)]
    full, lossy, nlost = g.lossy(short, (2,))   # slice 1 covers 25..29 only; 30..51 never arrive
    assert nlost == 22
    _follow(dec, od, full, lossy, nlost, 'short slice')
    full, clean, _ = g.lossy(L4, ())
    _follow(dec, od, full, clean, 0, 'clean')
    dec.close()


@pytest.mark.parametrize('geo', [(1, 9, 0, [0, 3, 6]), (11, 1, 0, [0, 4, 8]), (13, 8, 4, [0, 30, 71])], ids=['16x144', '176x16', '208x120'])
def test_geometry(gpu_lib, oracle, geo):
    mbw, mbh, cb, firsts = geo
    w, h = mbw * 16, mbh * 16 - 2 * cb
    layout = [dict(first=f, qp_delta=k - 1) for k, f in enumerate(firsts)]
    g, od, dec = Pair(mbw, mbh, seed=100 + mbw, crop_bottom=cb), oracle.decoder(), Dec(w, h)
    u = g.idr(slices=layout)
    _follow(dec, od, u, u, 0, 'idr')
    for lost in ((0,), (1,), (2,), (), (0, 1)):
        full, lossy, nlost = g.lossy(layout, lost)
        _follow(dec, od, full, lossy, nlost, f'{w}x{h} lost {lost}')
    dec.close()


@pytest.mark.parametrize('resolve', [1, 0])
def test_non_reference_picture_concealed(gpu_lib, oracle, resolve):
    """ref_idc 0: the concealed picture is output and the following P still predicts from the last reference"""
    g, od, dec = Pair(11, 9, seed=111), oracle.decoder(), Dec(176, 144, resolve=resolve)
    u = g.idr(slices=L4)
    _follow(dec, od, u, u, 0, 'idr')
    full, lossy, nlost = g.lossy(L4, (1,), ref_idc=0)
    _follow(dec, od, full, lossy, nlost, 'non-reference, lossy')
    full, clean, _ = g.lossy(L4, ())
    _follow(dec, od, full, clean, 0, 'P after it')
    skipper = oracle.decoder()   # the same P without the non-reference picture: the same samples
    g2 = Pair(11, 9, seed=111)
    assert skipper.decode(g2.idr(slices=L4))[0] == 1
    g2.lossy(L4, (1,), ref_idc=0)
    rc, pic, _, _ = skipper.decode(g2.lossy(L4, ())[0])
    assert rc == 1 and np.array_equal(pic, od.out[:pic.size])
    dec.close()


def test_not_concealed(gpu_lib, oracle):
    """concealment on changes nothing for: an IDR missing a slice, a P picture before any reference, a unit whose only
    slice is the failed one, two overlapping good slices -- no picture, the same status as with it off, and the next
    clean IDR decodes"""
    g = Pair(11, 9, seed=121)
    idr = g.idr(slices=L4)
    nals = _split_nals(idr)
    idr_lossy = b''.join(nals[:3] + nals[4:])   # SPS, PPS, slices 0, 2, 3
    full, p_lossy, _ = g.lossy(L4, (2,))
    _, only_failed, _ = g.lossy(L4, (0, 1, 2, 3)[1:], failed=(1,), order=[1])
    pn = _split_nals(g.lossy(L4, ())[0])
    overlap = pn[0] + pn[1] + pn[1] + pn[3]     # slice 2 lost, slice 1 twice
    g3 = Pair(11, 9, seed=122)
    idr2 = g3.idr(slices=L4)
    ref = oracle.decoder().decode(idr2)[1]
    for units in ([idr_lossy], [idr_lossy, p_lossy], [idr, only_failed], [idr, overlap]):
        res = []
        for conceal in (1, 0):
            dec = Dec(176, 144, conceal=conceal, waves=2)
            for u in units[:-1]:
                dec.one(u)
            rc, got, _ = dec.one(units[-1])
            res.append((rc, got, dec.dec.concealed()))
            rc, got, out = dec.one(idr2)
            assert (rc, got) == (0, 1) and np.array_equal(out, ref)
            dec.close()
        assert res[0] == res[1] == (-2, 0, [[0]]), res


def test_off_is_today(gpu_lib, oracle):
    import h264mi
    g, od = Pair(11, 9, seed=131), oracle.decoder()
    dec = Dec(176, 144, conceal=0)
    assert dec.dec.conceal() == 0
    u = g.idr(slices=L4)
    _follow(dec, od, u, u, 0, 'idr')
    _, lossy, _ = g.lossy(L4, (1,))
    assert od.decode(lossy)[0] == 2
    rc, got, _ = dec.one(lossy)
    assert (rc, got) == (-2, 0) and dec.dec.concealed() == [[0]]
    # the last picture stays the reference: a P picture coded against it decodes (the lossy one took no frame_num: resend it whole)
    g2 = Pair(11, 9, seed=131)
    g2.idr(slices=L4)
    full = g2.lossy(L4, ())[0]
    _follow(dec, od, full, full, 0, 'P after the dropped picture')
    with pytest.raises(ValueError):
        dec.dec.set_conceal(2)
    assert gpu_lib.h264mi_dec_set_conceal(dec.dec._d, -1) == -1 and gpu_lib.h264mi_dec_set_conceal(None, 1) == -1 and dec.dec.conceal() == 0
    for mode in (1, 0):
        dec.dec.set_streamed(mode)
        assert dec.dec.streamed() == mode
        dec.dec.set_conceal(1)
        assert dec.dec.conceal() == 1 and dec.dec.streamed() == 0
        dec.dec.set_conceal(0)
        assert dec.dec.conceal() == 0 and dec.dec.streamed() == mode
    dec.close()


# ---- the GPU encoder's streams: the substitute all-skip slice is written here from the donor slice's header
def _unescape(x):
    out, z = bytearray(), 0
    for b in x[5:]:
        if z >= 2 and b == 3:
            z = 0
            continue
        out.append(b)
        z = z + 1 if b == 0 else 0
    return bytes(out)


def _ue(rbsp, pos):
    bit = lambda p: (rbsp[p >> 3] >> (7 - (p & 7))) & 1
    lz = 0
    while bit(pos + lz) == 0:
        lz += 1
    v = 0
    for k in range(lz + 1):
        v = (v << 1) | bit(pos + lz + k)
    return v - 1, pos + 2 * lz + 1


def skip_slice_like(donor, first, run):
    """an all-skip P slice NAL: first_mb_in_slice `first`, one mb_skip_run `run`, every other header field (frame_num,
    slice_qp_delta, the loop-filter fields) copied bit for bit from the donor slice of the encoder's stream (its SPS:
    15-bit frame_num, POC type 2; non-IDR P slices of a reference picture)"""
    r = _unescape(donor)
    bit = lambda p: (r[p >> 3] >> (7 - (p & 7))) & 1
    _, p0 = _ue(r, 0)                 # first_mb_in_slice
    st, p = _ue(r, p0)                # slice_type
    assert st % 5 == 0 and donor[4] & 31 == 1 and (donor[4] >> 5) & 3
    _, p = _ue(r, p)                  # pic_parameter_set_id
    p += 15                           # frame_num
    if bit(p):                        # num_ref_idx_active_override_flag
        _, p = _ue(r, p + 1)
    else:
        p += 1
    p += 1
    if bit(p - 1):                    # ref_pic_list_modification_flag_l0: {idc, value} pairs up to idc 3
        while True:
            op, p = _ue(r, p)
            if op == 3:
                break
            _, p = _ue(r, p)
    assert bit(p) == 0                # adaptive_ref_pic_marking_mode_flag: sliding window
    p += 1
    _, p = _ue(r, p)                  # slice_qp_delta
    idc, p = _ue(r, p)                # disable_deblocking_filter_idc
    if idc != 1:
        _, p = _ue(r, p)
        _, p = _ue(r, p)
    w = BitWriter()
    w.ue(first)
    for q in range(p0, p):
        w.u(bit(q), 1)
    w.ue(run)
    return nal((donor[4] >> 5) & 3, 1, w.rbsp())


def _encode(w, h, S, nslices, nframes, sid):
    """-> units[t][s], first MB of every slice (+ the total)"""
    import torch
    import h264mi
    from h264mi.synth import SyntheticStream
    gs = [SyntheticStream(sid + s, w, h) for s in range(S)]
    enc = h264mi.BatchEncoder(w, h, 4000000 if w > 1000 else 400000, S)
    enc.set_frame_skip(False)
    enc.set_slices(nslices)
    units = []
    for t in range(nframes):
        enc.encode(torch.from_numpy(np.stack([np.ascontiguousarray(g.frame(t)) for g in gs])).cuda())
        nb = enc.nal_sizes()
        assert all(x > 0 for x in nb)
        units.append([enc.nal_bytes(s, nb[s]) for s in range(S)])
    enc.close()
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    return units, [h264mi.slice_first_row(mbh, nslices, k) * mbw for k in range(nslices)] + [mbw * mbh]


def _lose(unit, lost, firsts):
    """a P unit of the encoder with the slices `lost` removed -> (lossy unit, substituted unit for the oracle, MBs lost)"""
    nals = _split_nals(unit)
    assert len(nals) == len(firsts) - 1 and all(x[4] & 31 == 1 for x in nals)
    sub, n = list(nals), 0
    for run in runs(lost):
        donor = nals[run[0] - 1 if run[0] > 0 else run[-1] + 1]
        first, end = firsts[run[0]], firsts[run[-1] + 1]
        sub[run[0]] = skip_slice_like(donor, first, end - first)
        for i in run[1:]:
            sub[i] = b''
        n += end - first
    return b''.join(x for i, x in enumerate(nals) if i not in lost), b''.join(sub), n


def test_batch_multiframe(gpu_lib, oracle):
    """16 streams of the GPU encoder at 3 slices; one decode_frames call of 3 frames in which different streams lose
    different slices in frames 0 and 1: a concealed frame f is the reference of frame f + 1 of the same call"""
    S = 16
    units, firsts = _encode(176, 144, S, 3, 4, sid=40)
    plan = lambda f, s: {0: [(), (0,), (1,), (2,), (0, 1), (1, 2)][s % 6], 1: [(2,), (), (0,), (1,), ()][s % 5], 2: ()}[f]
    lossy = [[None] * S for _ in range(3)]
    want = [[None] * S for _ in range(3)]
    mbs = [[0] * S for _ in range(3)]
    for s in range(S):
        od = oracle.decoder()
        assert od.decode(units[0][s])[0] == 1
        for f in range(3):
            lossy[f][s], sub, mbs[f][s] = _lose(units[1 + f][s], plan(f, s), firsts)
            rc, pic, _, _ = od.decode(sub)
            assert rc == 1, (f, s)
            want[f][s] = pic
    assert sum(m > 0 for row in mbs for m in row) >= 20
    for resolve in (1, 0):
        dec = Dec(176, 144, S=S, B=3, resolve=resolve, waves=3)
        rc, got, _ = dec.decode([units[0]])
        assert rc == 0 and got == [[1] * S]
        rc, got, out = dec.decode(lossy)
        assert rc == 0 and got == [[1] * S] * 3
        for f in range(3):
            for s in range(S):
                assert np.array_equal(out[f][s], want[f][s]), f'resolve {resolve} frame {f} stream {s}: {int(np.count_nonzero(out[f][s] != want[f][s]))} samples differ'
        assert dec.dec.concealed() == mbs
        import ctypes
        host = (ctypes.c_int * (3 * S))()
        h264mi = sys.modules['h264mi']
        h264mi._hip_memcpy_d2h(ctypes.addressof(host), dec.dec.concealed_ptr(), 4 * 3 * S)
        assert list(host) == [m for row in mbs for m in row]
        dec.close()


def test_1080p_8_slices(gpu_lib, oracle):
    S = 2
    units, firsts = _encode(1920, 1080, S, 8, 3, sid=50)
    lost = {(0, 0): (3,), (0, 1): (0,)}
    dec = Dec(1920, 1080, S=S, B=2, waves=8)
    ods = [oracle.decoder() for _ in range(S)]
    for s in range(S):
        assert ods[s].decode(units[0][s])[0] == 1
    rc, got, _ = dec.decode([units[0]])
    assert rc == 0 and got == [[1] * S]
    lossy, want, mbs = [[None] * S for _ in range(2)], [[None] * S for _ in range(2)], [[0] * S for _ in range(2)]
    for s in range(S):
        for f in range(2):
            lossy[f][s], sub, mbs[f][s] = _lose(units[1 + f][s], lost.get((f, s), ()), firsts)
            rc, want[f][s], _, _ = ods[s].decode(sub)
            assert rc == 1
    rc, got, out = dec.decode(lossy)
    assert rc == 0 and got == [[1] * S] * 2
    for f in range(2):
        for s in range(S):
            assert np.array_equal(out[f][s], want[f][s]), f'frame {f} stream {s}'
    assert dec.dec.concealed() == mbs and mbs[0][0] > 900 and mbs[1] == [0, 0]
    dec.close()


_DROPIN = r'''
import ctypes, os, sys
import numpy as np
sys.path.insert(0, os.path.join(sys.argv[1], 'openh264-wasm_amd'))
sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))
import torch
import h264mi
from _oracle import Oracle
from concealgen import Pair
from test_gpu_decoder import gpu_decode
torch.cuda.set_device(0)
L = h264mi.lib()
od = Oracle(os.path.join(sys.argv[1], 'oracle', 'build', 'libh264_oracle.so')).decoder()
L4 = [dict(first=0, qp_delta=1), dict(first=25, dbk=(2, 1, -1)), dict(first=52), dict(first=80)]
g = Pair(11, 9, seed=141)
assert L.init_decoder(3) == 0
idr = g.idr(slices=L4)
rc, pic, _, _ = od.decode(idr)
gw, gh, got = gpu_decode(L, 3, idr, 176, 144)
assert rc == 1 and (gw, gh) == (176, 144) and np.array_equal(got, pic)
full, lossy, n = g.lossy(L4, (1,))
rc, pic, _, _ = od.decode(full)
gw, gh, got = gpu_decode(L, 3, lossy, 176, 144)
if os.environ.get('H264MI_DEC_CONCEAL') == '1':
    assert rc == 1 and (gw, gh) == (176, 144) and np.array_equal(got, pic)
    gw, gh, rgba = gpu_decode(L, 3, g.lossy(L4, (3,))[1], 176, 144, rgba=True)
    assert (gw, gh) == (176, 144)
    print('dropin concealed')
else:
    assert (gw, gh) == (0, 0)
    print('dropin dropped')
L.deinit_decoder(3)
'''


@pytest.mark.parametrize('on', [True, False])
def test_dropin_env(gpu_lib, oracle, tmp_path, on):
    """H264MI_DEC_CONCEAL=1 in a fresh process: decode_frame_yuv_i420 returns the concealed picture (== the oracle on
    the full unit); without the variable the lossy unit gives width and height 0"""
    script = tmp_path / 'dropin_conceal.py'
    script.write_text(_DROPIN)
    env = {k: v for k, v in os.environ.items() if k != 'H264MI_DEC_CONCEAL'}
    if on:
        env['H264MI_DEC_CONCEAL'] = '1'
    r = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and ('dropin concealed' if on else 'dropin dropped') in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
