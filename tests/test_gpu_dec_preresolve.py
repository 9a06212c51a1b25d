"""GPU: record resolution ahead of the reconstruction (dec_resolve_kernel). A call that is not
streamed resolves the motion vectors (8.4.1.1, 8.4.1.3) and Intra4x4 modes (8.3.1.1) of all its pictures in one
launch and reconstructs from resolved records (dec_recon_pre_kernel); a streamed call resolves inside its
reconstruction (dec_recon_kernel). Both share the rule functions, and both must give the oracle decoder's
pictures byte for byte, on tests/streamgen.py's full-syntax streams (every Baseline macroblock type), through
the batch decoder:

  - the geometries at which neighbour selection can go wrong: 1x1 and 1x3 MBs (no A / C / D), 2x2 (the C -> D
    fallback at the last column), 3x2 and 4x3 (the three-slot ring of above-row MBs wraps), 11x9 (control);
  - multi-slice pictures with slice boundaries in mid-row and at a row start (availability by first_mb);
  - one call of 4 frames x 3 streams of different content (every picture of a call in one launch);
  - P pictures with I_NxN macroblocks beside inter ones (predicted mode 2 across inter neighbours, and the
    intra sample wait, which the pre-resolved build keeps);
  - the same streams streamed;
  - a picture whose slice data is cut short: no picture, as the oracle, and the stream decodes on.

The CPU test at the top pins that the generator writes and the oracle decodes every geometry used."""
import numpy as np
import pytest

from test_syntax_streams import MULTI, SO, _multi_units

GEOMS = [(1, 1), (1, 3), (2, 2), (3, 2), (4, 3), (11, 9)]
# 4 x 3: slices starting in mid-row (MB 2, 6), at a row start (MB 4, 8) and a last one-MB slice
MULTI_4x3 = [dict(first=0), dict(first=2, qp_delta=3), dict(first=4), dict(first=6, dbk=(2, 1, -1)), dict(first=8, intra=True), dict(first=11)]
I4_MIX = {'i4': 4, 'skip': 2, 'p16': 2, 'p16x8': 1, 'p8x16': 1, 'p8x8': 2}

_cache = {}


def _ref(oracle, key, make):
    """units of one stream and the oracle's picture of each (None: no picture), computed once per key"""
    if key not in _cache:
        units = make()
        od = oracle.decoder()
        pics = []
        for u in units:
            rc, pic, _, _ = od.decode(u)
            pics.append(pic.copy() if rc == 1 else None)
        _cache[key] = (units, pics)
    return _cache[key]


def _plain(oracle, mbw, mbh, seed, mix=None):
    def make():
        from streamgen import SyntaxGen
        g = SyntaxGen(SO, mbw, mbh, seed)
        return [g.idr()] + [g.p(mix) for _ in range(3)]
    return _ref(oracle, ('plain', mbw, mbh, seed, None if mix is None else tuple(sorted(mix.items()))), make)


def _sliced(oracle, mbw, mbh, seed, layout_id, layout):
    return _ref(oracle, ('multi', mbw, mbh, seed, layout_id), lambda: [u for u, _ in _multi_units(seed, layout, mbw, mbh)[1]])


@pytest.mark.parametrize('geom', GEOMS, ids=[f'{a}x{b}' for a, b in GEOMS])
def test_generator_and_oracle_accept_geometry(oracle, geom):
    units, pics = _plain(oracle, geom[0], geom[1], 50 + geom[0] * 16 + geom[1])
    assert len(units) == 4 and all(p is not None and p.size == geom[0] * geom[1] * 384 for p in pics)


def _decode_call(mbw, mbh, streams, streamed):
    """all frames of `streams` (S lists of n access units) in ONE decode call -> ([f][s] picture or None, launches)"""
    import torch
    import h264mi
    S, n = len(streams), len(streams[0])
    w, h = mbw * 16, mbh * 16
    F = w * h * 3 // 2
    dec = h264mi.BatchDecoder(w, h, S, max_frames=n)
    dec.set_streamed(1 if streamed else 0)  # 0: never streamed automatically either, so the resolution pass runs
    dev = [[torch.from_numpy(np.frombuffer(streams[s][f], np.uint8).copy()).cuda() for s in range(S)] for f in range(n)]
    out = torch.zeros((n, S, F), dtype=torch.uint8, device='cuda')
    got = torch.full((n, S), -1, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    dec.decode_frames([dev[f][s].data_ptr() for f in range(n) for s in range(S)],
                      nal_sizes=[len(streams[s][f]) for f in range(n) for s in range(S)],
                      out_ptrs=[out[f, s].data_ptr() for f in range(n) for s in range(S)],
                      got_ptrs=[got[f, s:s + 1].data_ptr() for f in range(n) for s in range(S)])
    rc, _ = dec.status()
    torch.cuda.synchronize()
    launches = dec.resolve_launches()
    dec.close()
    g, host = got.cpu().numpy(), out.cpu().numpy()
    return rc, [[host[f, s] if g[f, s] == 1 else None for s in range(S)] for f in range(n)], launches


def _check(mbw, mbh, refs, streamed):
    rc, pics, launches = _decode_call(mbw, mbh, [u for u, _ in refs], streamed)
    assert launches == (0 if streamed else 1)  # the path under test was the one taken
    for f in range(len(pics)):
        for s, (_, want) in enumerate(refs):
            a, b = pics[f][s], want[f]
            assert (a is None) == (b is None), f'frame {f} stream {s}: picture {a is not None}, oracle {b is not None}'
            if b is not None:
                assert np.array_equal(a, b), f'frame {f} stream {s}: {int(np.count_nonzero(a != b))} samples differ'
    return rc


STREAMED = pytest.mark.parametrize('streamed', [0, 1], ids=['resolved-ahead', 'streamed'])


@pytest.mark.gpu
@STREAMED
@pytest.mark.parametrize('geom', GEOMS, ids=[f'{a}x{b}' for a, b in GEOMS])
def test_geometries_vs_oracle(gpu_lib, oracle, geom, streamed):
    assert _check(geom[0], geom[1], [_plain(oracle, geom[0], geom[1], 50 + geom[0] * 16 + geom[1])], streamed) == 0


@pytest.mark.gpu
@STREAMED
@pytest.mark.parametrize('case', ['4x3', '11x9-0', '11x9-1', '11x9-2'])
def test_multislice_vs_oracle(gpu_lib, oracle, case, streamed):
    if case == '4x3':
        mbw, mbh, ref = 4, 3, _sliced(oracle, 4, 3, 61, 'a', MULTI_4x3)
    else:
        k = int(case[-1])
        mbw, mbh, ref = 11, 9, _sliced(oracle, 11, 9, 62 + k, k, MULTI[k])
    assert all(p is not None for p in ref[1])
    assert _check(mbw, mbh, [ref], streamed) == 0


@pytest.mark.gpu
@STREAMED
def test_four_frames_three_streams_one_call(gpu_lib, oracle, streamed):
    refs = [_plain(oracle, 11, 9, 70), _plain(oracle, 11, 9, 71), _sliced(oracle, 11, 9, 64, 2, MULTI[2])]
    assert _check(11, 9, refs, streamed) == 0


@pytest.mark.gpu
@STREAMED
@pytest.mark.parametrize('geom', [(4, 3), (11, 9)], ids=['4x3', '11x9'])
def test_intra4x4_beside_inter_vs_oracle(gpu_lib, oracle, geom, streamed):
    assert _check(geom[0], geom[1], [_plain(oracle, geom[0], geom[1], 80 + geom[0], I4_MIX)], streamed) == 0


@pytest.mark.gpu
@STREAMED
def test_truncated_slice_no_picture_and_no_hang(gpu_lib, oracle, streamed):
    """frame 2 of stream 1 loses the second half of its slice data: the parse fails mid-picture, the resolution
    pass leaves that picture alone and ends, the frame yields no picture (as the oracle) and frame 3 decodes
    from the last good reference; stream 0 is untouched"""
    good = _plain(oracle, 11, 9, 90)

    def make():
        units = list(_plain(oracle, 11, 9, 91)[0])
        units[2] = units[2][:len(units[2]) // 2]
        return units
    bad = _ref(oracle, ('cut', 91), make)
    assert bad[1][2] is None and bad[1][3] is not None  # the oracle drops the cut picture and decodes on
    _check(11, 9, [good, bad], streamed)
