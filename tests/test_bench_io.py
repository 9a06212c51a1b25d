"""bench.py's input loader and output dump (no GPU): the clip cut from the textures on the device holds the
bytes SyntheticStream.frame() gives, and --dump-outputs writes float arrays from which the outputs read back."""
import importlib.util
import os
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('h264mi_bench', os.path.join(ROOT, 'bench.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_load_clip_matches_frames():
    import torch
    from h264mi.synth import SyntheticStream
    W, H, sids, T = 48, 34, [3, 0, 7], 70  # T > 64 / 3: the window offsets wrap
    F = W * H * 3 // 2
    clip = torch.zeros((T, len(sids) * F), dtype=torch.uint8)
    _bench().load_clip(clip, sids, W, H, torch, SyntheticStream, torch.device('cpu'))
    for i, sid in enumerate(sids):
        g = SyntheticStream(sid, W, H)
        for t in range(T):
            assert np.array_equal(clip[t, i * F:(i + 1) * F].numpy(), g.frame(t)), (sid, t)


def test_dump_outputs_round_trip(tmp_path):
    b = _bench()
    W, H, S = 32, 18, 5
    F = W * H * 3 // 2
    rng = np.random.default_rng(1)
    pics = [rng.integers(0, 256, F, dtype=np.uint8).tobytes() for _ in range(S)]
    sizes = [7, 0, 300, 1, 12]
    nals = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes]
    nal = b''.join(nals)
    a = types.SimpleNamespace(dump_outputs=str(tmp_path / 'out'), width=W, height=H)
    b.dump_outputs(a, np, 0, 1, sizes, nals, pics)
    got = {f[:-4]: np.load(os.path.join(a.dump_outputs, f)) for f in os.listdir(a.dump_outputs)}
    assert sorted(got) == ['nal_bytes', 'nal_sizes', 'picture_row_sums', 'picture_sample', 'picture_sample_index']
    assert all(x.dtype in (np.float32, np.float64) for x in got.values())
    assert got['nal_sizes'].tolist() == sizes and got['nal_bytes'].astype(np.uint8).tobytes() == nal
    p = np.stack([np.frombuffer(x, np.uint8) for x in pics])
    idx = got['picture_sample_index'].astype(np.int64)
    assert len(idx) == F and np.array_equal(got['picture_sample'], p[:, idx])  # a small picture is kept whole
    assert np.array_equal(got['picture_row_sums'], p.reshape(S, F // W, W).sum(axis=2))
    # the sample is the same draw in every run, and a 128-stream 1080p dump stays under 64 MB
    b.dump_outputs(a, np, 0, 1, sizes, nals, pics)
    assert np.array_equal(np.load(os.path.join(a.dump_outputs, 'picture_sample_index.npy')), got['picture_sample_index'])
    F2 = 1920 * 1080 * 3 // 2
    n = min(F2, b.DUMP_SAMPLE_BYTES // 4 // 128)
    assert 128 * (n * 4 + F2 // 1920 * 8 + 8) + n * 8 + b.DUMP_NAL_BYTES + 5 * 128 < 64 * 10 ** 6


def test_dump_outputs_cuts_long_units(tmp_path, monkeypatch):
    b = _bench()
    monkeypatch.setattr(b, 'DUMP_NAL_BYTES', 4 * 20)
    a = types.SimpleNamespace(dump_outputs=str(tmp_path), width=2, height=2)
    nals = [bytes(range(30)), bytes(range(100, 105))]
    b.dump_outputs(a, np, 0, 1, [30, 5], nals, None)
    assert np.load(tmp_path / 'nal_sizes.npy').tolist() == [30, 5]
    assert np.load(tmp_path / 'nal_bytes.npy').tolist() == list(range(10)) + list(range(100, 105))
