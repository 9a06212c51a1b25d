"""GPU: the mesh warp -- the standalone call h264mi_i420_warp_dev and the encoder's warped input
h264mi_enc_encode_warped -- against tests/warpref.py. The rule is exact integers, so every comparison is equality of
bytes; every destination sits between 64 guard bytes of 0xA5 that must stay as they were, and the sources and meshes are
compared afterwards to show they were not written. The shapes, the mesh set and the settings are warpref's, shared with
tests/test_warp_host.py, which shows that the set holds tiles of both of the kernel's classes."""
import ctypes
import functools

import numpy as np
import pytest

import warpref

pytestmark = pytest.mark.gpu

GUARD = 64
N = warpref.N


def _device(x, shift=0, align=4):
    """x's bytes on the device, `shift` bytes past a multiple of `align` of a larger allocation"""
    import torch
    x = np.ascontiguousarray(x)
    raw = x.view(np.uint8).ravel()
    whole = torch.zeros(raw.size + shift + 64 + align, dtype=torch.uint8, device='cuda')
    at = (-whole.data_ptr()) % align + shift
    view = whole[at:at + raw.size]
    view.copy_(torch.from_numpy(raw))
    return view


def _guarded(nbytes, shift=0):
    """(whole, view): a destination of nbytes between 64 bytes of 0xA5 on each side, `shift` bytes into its allocation"""
    import torch
    whole = torch.full((shift + nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    return whole, whole[shift + GUARD:shift + GUARD + nbytes]


def _guards_intact(whole, nbytes, shift=0):
    h = whole.cpu().numpy()
    return bool((h[:shift + GUARD] == 0xA5).all() and (h[shift + GUARD + nbytes:] == 0xA5).all())


def _mesh_tensor(view):
    import torch
    assert view.data_ptr() % 4 == 0
    return view.view(torch.int32)


def _warp(d_src, src, dst, meshes, per_frame, prm, shift=0):
    """the standalone call on the N frames at d_src under `meshes` (one array, or N stacked): the N warped frames as an
    array; guards, source and meshes checked"""
    import h264mi
    (sw, sh), (dw, dh) = src, dst
    fb = warpref.frame_bytes(dw, dh)
    d_mesh = _device(meshes)
    whole, d = _guarded(N * fb, shift)
    if shift:
        assert d_src.data_ptr() % 2 == 1 and d.data_ptr() % 2 == 1
    before = d_src.cpu().numpy().copy()
    h264mi.i420_warp(d, d_src, sw, sh, dw, dh, N, _mesh_tensor(d_mesh), prm, mesh_per_frame=per_frame)
    out = d.cpu().numpy().reshape(N, fb)
    assert _guards_intact(whole, N * fb, shift), 'bytes outside the destination frames were written'
    assert np.array_equal(d_src.cpu().numpy(), before), 'the source was written'
    assert np.array_equal(d_mesh.cpu().numpy(), np.ascontiguousarray(meshes).view(np.uint8).ravel()), 'the mesh was written'
    return out


@pytest.mark.parametrize('g', warpref.GRIDS)
@pytest.mark.parametrize('case', warpref.SHAPES, ids=[warpref.shape_id(c) for c in warpref.SHAPES])
def test_standalone_vs_reference(gpu_lib, case, g):
    """every mesh of the set x both filters x both edge modes, once with the mesh shared by the three frames and once
    with three per-frame meshes (mesh k, k + 1, k + 2 of the set)"""
    src, dst, shift = case
    K = len(warpref.MESHES)
    d_src = _device(warpref.frames(src), shift)
    for k in range(K):
        for filt, edge in warpref.SETTINGS:
            prm = warpref.params(filt, edge, g)
            got = _warp(d_src, src, dst, warpref.mesh(k, src, dst, g), False, prm, shift)
            for f in range(N):
                want = warpref.reference(src, dst, g, k, filt, edge, f)
                assert np.array_equal(got[f], want), f'{warpref.MESHES[k][0]} {prm} shared, frame {f}: {int((got[f] != want).sum())} bytes differ'
            ks = [(k + f) % K for f in range(N)]
            got = _warp(d_src, src, dst, np.stack([warpref.mesh(j, src, dst, g) for j in ks]), True, prm, shift)
            for f in range(N):
                want = warpref.reference(src, dst, g, ks[f], filt, edge, f)
                assert np.array_equal(got[f], want), f'{warpref.MESHES[k][0]} {prm} per frame, frame {f}: {int((got[f] != want).sum())} bytes differ'


def test_identity_copies_and_orientations_turn(gpu_lib):
    import orientref
    src = (130, 66)
    fr = warpref.frames(src)
    d_src = _device(fr)
    for g in warpref.GRIDS:
        prm = warpref.params(warpref.BICUBIC, warpref.CLAMP, g)
        assert np.array_equal(_warp(d_src, src, src, warpref.mesh(0, src, src, g), False, prm), fr)
        for orient in orientref.ALL:
            m, dw, dh = warpref.mesh_orient(orient, 130, 66, g)
            got = _warp(d_src, src, (dw, dh), m, False, prm)
            for f in range(N):
                assert np.array_equal(got[f], orientref.orient_frame(fr[f], 130, 66, orient)), (g, orient, f)


def test_repeatability(gpu_lib):
    src = dst = (130, 66)
    d_src = _device(warpref.frames(src))
    for k in (2, 7, 8):  # rotation (staged), zoom out and random (fallback)
        prm = warpref.params(warpref.BICUBIC, warpref.FILL, 4)
        a = _warp(d_src, src, dst, warpref.mesh(k, src, dst, 4), False, prm)
        b = _warp(d_src, src, dst, warpref.mesh(k, src, dst, 4), False, prm)
        assert a.tobytes() == b.tobytes()


def test_standalone_bad_arguments(gpu_lib):
    """one refusal per item of the header's list, each before a launch: the destination stays as it was"""
    import torch
    import h264mi
    fn = gpu_lib.h264mi_i420_warp_dev
    sw, sh, dw, dh, g = 34, 18, 18, 34, 3
    fb_s, fb_d = warpref.frame_bytes(sw, sh), warpref.frame_bytes(dw, dh)
    s = torch.zeros(N * fb_s + N * fb_d, dtype=torch.uint8, device='cuda')
    m = _device(np.stack([warpref.mesh(0, (sw, sh), (dw, dh), g)] * N))
    whole, d = _guarded(N * fb_d)
    ps, pd, pm = ctypes.c_void_p(s.data_ptr()), ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(m.data_ptr())
    good = h264mi.Warp(1, 0, 0, 0, 0, g)
    pp = ctypes.byref(good)
    assert fn(pd, dw, dh, ps, sw, sh, N, pm, 1, pp, None) == 0
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == 0).all()
    d.fill_(0xA5)
    # a null pointer
    assert fn(None, dw, dh, ps, sw, sh, N, pm, 0, pp, None) == -1 and fn(pd, dw, dh, None, sw, sh, N, pm, 0, pp, None) == -1
    assert fn(pd, dw, dh, ps, sw, sh, N, None, 0, pp, None) == -1 and fn(pd, dw, dh, ps, sw, sh, N, pm, 0, None, None) == -1
    # a bad side, either picture
    for bad in (0, 1, 17, 8194, -2):
        assert fn(pd, bad, dh, ps, sw, sh, 1, pm, 0, pp, None) == -1 and fn(pd, dw, bad, ps, sw, sh, 1, pm, 0, pp, None) == -1, bad
        assert fn(pd, dw, dh, ps, bad, sh, 1, pm, 0, pp, None) == -1 and fn(pd, dw, dh, ps, sw, bad, 1, pm, 0, pp, None) == -1, bad
    # n < 1
    assert fn(pd, dw, dh, ps, sw, sh, 0, pm, 0, pp, None) == -1 and fn(pd, dw, dh, ps, sw, sh, -1, pm, 0, pp, None) == -1
    # a setting h264mi_warp_ok refuses; a mesh count flag that is neither
    for bad in (h264mi.Warp(2, 0, 0, 0, 0, g), h264mi.Warp(1, 2, 0, 0, 0, g), h264mi.Warp(1, 1, 256, 0, 0, g), h264mi.Warp(1, 0, 0, 0, 0, 2),
                h264mi.Warp(1, 0, 0, 0, 0, 6)):
        assert fn(pd, dw, dh, ps, sw, sh, N, pm, 0, ctypes.byref(bad), None) == -1, bad
    assert fn(pd, dw, dh, ps, sw, sh, N, pm, 2, pp, None) == -1
    # a mesh address that is no multiple of 4
    for off in (1, 2, 3):
        assert fn(pd, dw, dh, ps, sw, sh, 1, ctypes.c_void_p(m.data_ptr() + off), 0, pp, None) == -1
    # a destination that overlaps the source (first and last byte) or the mesh
    for off in (0, N * fb_s - 1):
        assert fn(ctypes.c_void_p(s.data_ptr() + off), dw, dh, ps, sw, sh, N, pm, 0, pp, None) == -1
    assert fn(ctypes.c_void_p(s.data_ptr() - N * fb_d + 1), dw, dh, ps, sw, sh, N, pm, 0, pp, None) == -1
    assert fn(pm, dw, dh, ps, sw, sh, 1, pm, 0, pp, None) == -1
    assert fn(ctypes.c_void_p(m.data_ptr() + m.numel() - 1), dw, dh, ps, sw, sh, N, pm, 1, pp, None) == -1  # the third mesh's last byte
    torch.cuda.synchronize()
    assert _guards_intact(whole, N * fb_d) and (d.cpu().numpy() == 0xA5).all(), 'a refused call wrote'


# ---------------------------------------------------------------- the encoder's warped input

ENC_W, ENC_H, SRC_W, SRC_H, ENC_S, ENC_NF, ENC_G = 48, 32, 66, 50, 2, 4, 4


@functools.lru_cache(maxsize=None)
def _sources():
    from h264mi.synth import SyntheticStream
    gs = [SyntheticStream(s, SRC_W, SRC_H) for s in range(ENC_S)]
    return [np.stack([np.ascontiguousarray(g.frame(t)).ravel() for g in gs]) for t in range(ENC_NF)]


@functools.lru_cache(maxsize=None)
def _enc_meshes():
    """a rotation per stream: 7 degrees one way, 5 the other"""
    out = []
    for deg in (7.0, -5.0):
        c, s = warpref._q16(np.cos(np.radians(deg))), warpref._q16(np.sin(np.radians(deg)))
        out.append(warpref.mesh_affine(ENC_W, ENC_H, ENC_G, [c, -s, (65536 * (SRC_W - 1) - c * (ENC_W - 1) + s * (ENC_H - 1)) // 2,
                                                            s, c, (65536 * (SRC_H - 1) - s * (ENC_W - 1) - c * (ENC_H - 1)) // 2]))
    return np.stack(out)


ENC_PARAMS = warpref.params(warpref.BICUBIC, warpref.FILL, ENC_G)


@functools.lru_cache(maxsize=None)
def _warped_sources():
    m = _enc_meshes()
    return [np.stack([warpref.warp_frame(step[s], SRC_W, SRC_H, ENC_W, ENC_H, m[s], ENC_PARAMS) for s in range(ENC_S)]) for step in _sources()]


def _run(steps, feed, prepare=None):
    """one encoder over `steps` (a list of (S, frame bytes) arrays), fed by feed(enc, device frames): per step the NAL
    bytes and rc_state"""
    import torch
    import h264mi
    enc = h264mi.BatchEncoder(ENC_W, ENC_H, 200000, ENC_S)
    enc.set_frame_skip(False)
    if prepare:
        prepare(enc)
    out = []
    for fr in steps:
        frames = torch.from_numpy(np.ascontiguousarray(fr).ravel()).cuda()  # held until nal_sizes() has synchronised
        feed(enc, frames)
        sizes = enc.nal_sizes()
        out.append({'nal': [enc.nal_bytes(s, sizes[s]) for s in range(ENC_S)], 'rc': [enc.rc_state(s) for s in range(ENC_S)]})
    enc.close()
    return out


def _same(got, want):
    for t in range(len(want)):
        for s in range(ENC_S):
            assert len(got[t]['nal'][s]) > 0
            assert got[t]['nal'][s] == want[t]['nal'][s], f'frame {t} stream {s}: NAL bytes'
            assert got[t]['rc'][s] == want[t]['rc'][s], f'frame {t} stream {s}: rate-control state'


def test_encode_warped_equals_encode_of_reference_frames(gpu_lib):
    d_mesh = _mesh_tensor(_device(_enc_meshes()))
    got = _run(_sources(), lambda e, f: e.encode_warped(f, SRC_W, SRC_H, d_mesh, ENC_PARAMS, mesh_per_stream=True))
    want = _run(_warped_sources(), lambda e, f: e.encode(f))
    _same(got, want)
    one = _mesh_tensor(_device(_enc_meshes()[0]))  # one mesh for both streams
    got = _run(_sources()[:2], lambda e, f: e.encode_warped(f, SRC_W, SRC_H, one, ENC_PARAMS))
    ref = [np.stack([warpref.warp_frame(step[s], SRC_W, SRC_H, ENC_W, ENC_H, _enc_meshes()[0], ENC_PARAMS) for s in range(ENC_S)])
           for step in _sources()[:2]]
    _same(got, _run(ref, lambda e, f: e.encode(f)))


def test_encode_warped_runs_the_chain_behind_the_warp(gpu_lib):
    """the denoiser and an overlay list on: encode_warped of the sources equals encode of the reference-warped frames on
    an encoder that holds the same settings, and differs from a plain one"""
    import torch
    import h264mi
    d_mesh = _mesh_tensor(_device(_enc_meshes()))
    rng = np.random.default_rng(81)
    sprite = torch.from_numpy(rng.integers(0, 256, h264mi.i420a_bytes(16, 16), dtype=np.uint8)).cuda()
    ov = [h264mi.Overlay(0, 0, 0, 0, 16, 16, 20, 8, 256, 0)]

    def prepare(enc):
        enc.set_denoise((224, 224, 32, 1020))  # the gate open: every block is filtered
        enc.set_overlays(sprite, 16, 16, 1, ov)
        assert enc.overlays() == 1 and enc.denoise() is not None

    got = _run(_sources(), lambda e, f: e.encode_warped(f, SRC_W, SRC_H, d_mesh, ENC_PARAMS, mesh_per_stream=True), prepare)
    want = _run(_warped_sources(), lambda e, f: e.encode(f), prepare)
    plain = _run(_warped_sources(), lambda e, f: e.encode(f))
    _same(got, want)
    assert got[0]['nal'][0] != plain[0]['nal'][0], 'the overlay changed nothing: the test shows nothing'
    assert any(got[t]['nal'][1] != plain[t]['nal'][1] for t in range(1, ENC_NF)), 'the denoiser changed nothing: the test shows nothing'


def test_encode_warped_refusals_leave_the_encoder_untouched(gpu_lib):
    import torch
    import h264mi
    d_mesh = _mesh_tensor(_device(_enc_meshes()))
    src = _warped_sources()[:2]
    fresh = _run(src, lambda e, f: e.encode(f))
    other = torch.zeros(ENC_S * warpref.frame_bytes(SRC_W, SRC_H), dtype=torch.uint8, device='cuda')
    good = h264mi.Warp(*ENC_PARAMS)

    def feed(enc, frames):
        fn = enc._L.h264mi_enc_encode_warped
        po, pm, pp = ctypes.c_void_p(other.data_ptr()), ctypes.c_void_p(d_mesh.data_ptr()), ctypes.byref(good)
        assert fn(None, po, SRC_W, SRC_H, pm, 1, pp) == -1 and fn(enc._e, None, SRC_W, SRC_H, pm, 1, pp) == -1
        assert fn(enc._e, po, SRC_W, SRC_H, None, 1, pp) == -1 and fn(enc._e, po, SRC_W, SRC_H, pm, 1, None) == -1
        assert fn(enc._e, po, SRC_W + 1, SRC_H, pm, 1, pp) == -1 and fn(enc._e, po, SRC_W, 8194, pm, 1, pp) == -1
        assert fn(enc._e, po, SRC_W, SRC_H, pm, 2, pp) == -1
        assert fn(enc._e, po, SRC_W, SRC_H, ctypes.c_void_p(d_mesh.data_ptr() + 2), 0, pp) == -1
        assert fn(enc._e, po, SRC_W, SRC_H, pm, 1, ctypes.byref(h264mi.Warp(1, 1, 0, 0, 0, 6))) == -1
        with pytest.raises(ValueError):
            enc.encode_warped(other, SRC_W, SRC_H, d_mesh, (1, 3, 0, 0, 0, ENC_G), mesh_per_stream=True)
        inp = enc._L.h264mi_enc_input_buffer(enc._e)  # frames or a mesh that overlap the encoder's input area
        nb = ENC_S * warpref.frame_bytes(ENC_W, ENC_H)
        assert fn(enc._e, ctypes.c_void_p(inp), SRC_W, SRC_H, pm, 1, pp) == -1
        assert fn(enc._e, ctypes.c_void_p(inp + nb - 1), SRC_W, SRC_H, pm, 1, pp) == -1
        assert fn(enc._e, po, SRC_W, SRC_H, ctypes.c_void_p(inp + (-inp) % 4), 1, pp) == -1
        enc.encode(frames)

    _same(_run(src, feed), fresh)

    def feed_deinterlaced(enc, frames):  # refused while the deinterlacer is on; the plain call goes on
        with pytest.raises(ValueError):
            enc.encode_warped(other, SRC_W, SRC_H, d_mesh, ENC_PARAMS, mesh_per_stream=True)
        enc.encode(frames)

    def prepare(enc):
        enc.set_deinterlace((0, 1, 1, 24))

    _same(_run(src, feed_deinterlaced, prepare), _run(src, lambda e, f: e.encode(f), prepare))
