"""GPU: a plain bench.py run (the test is about the benchmark's own command line, so it starts it): --steps sets
the timed steps, the line carries ms_per_step and no baseline or parity work, and what --dump-outputs writes for
the last timed step is what the oracle computes for the same synthetic streams."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_last_step(gpu_lib, oracle, tmp_path):
    from h264mi.synth import SyntheticStream
    W, H, S, BR, CLIP, K, WU = 176, 144, 2, 300000, 4, 6, 5  # a 4-frame call and a frame-by-frame tail; the 4-frame clip wraps
    out = str(tmp_path / 'dump')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(K), '--warmup', str(WU),
                        '--streams', str(S), '--width', str(W), '--height', str(H), '--bitrate', str(BR), '--clip', str(CLIP),
                        '--dump-outputs', out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d['steps'] == K and d['warmup'] == WU and d['unit'] == 'frames/s' and d['dtype'] == 'u8' and d['higher_is_better'] is True
    assert d['ms_per_step'] > 0 and d['value'] == pytest.approx(S * 1e3 / d['ms_per_step'])
    assert d['kernels']['enc_mb_kernel']['launches'] == K  # the timed region ran K frame steps
    assert d['cpu_baseline'] is None and d['roofline']['traffic'] is None and 'skipped' in d['parity']['vs_oracle']
    got = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert sorted(got) == ['nal_bytes', 'nal_sizes', 'picture_row_sums', 'picture_sample', 'picture_sample_index']
    assert all(x.dtype in (np.float32, np.float64) for x in got.values())
    nals, pics = [], []
    for s in range(S):
        g, e, dec = SyntheticStream(s, W, H), oracle.encoder(W, H, BR), oracle.decoder()
        e.set_frame_skip(False)
        for t in range(WU + K):
            nal = e.encode(g.frame(t % CLIP))
            rc, pic, _, _ = dec.decode(nal)
            assert rc == 1
        nals.append(nal)
        pics.append(pic)
    assert got['nal_sizes'].tolist() == [len(x) for x in nals]
    assert got['nal_bytes'].astype(np.uint8).tobytes() == b''.join(nals)
    p = np.stack(pics)
    assert np.array_equal(got['picture_row_sums'], p.reshape(S, H * 3 // 2, W).sum(axis=2))
    idx = got['picture_sample_index'].astype(np.int64)
    assert len(idx) == W * H * 3 // 2 and np.array_equal(got['picture_sample'], p[:, idx])
