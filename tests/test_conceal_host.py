"""CPU: the gap rule of slice-copy concealment (csrc/conceal_host.h, exported as h264mi_conceal_gaps --
the function dec_conceal_kernel calls) against a plain restatement on directed and random slice tables, the same
tables through a stand-alone program under the host sanitizers, and the claim the rule rests on, pinned on the oracle:
in the full access unit that a lossy one must decode like (tests/concealgen.py), the macroblocks of an all-skip slice
are, before the loop filter, the co-located samples of the previous picture, with zero vectors and the donor's QP."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from concealgen import Pair, ref_gaps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (total MBs, [(first, end, ok)], expected): the tables tools/conceal_host_san.cc also runs (tests/golden/conceal_tables.txt)
DIRECTED = {
    'exact tiling': (99, [(0, 30, 1), (30, 61, 1), (61, 99, 1)], []),
    'gap at the start': (99, [(25, 60, 1), (60, 99, 1)], [(0, 25, 0)]),
    'gap in the middle': (99, [(0, 25, 1), (60, 99, 1)], [(25, 60, 0)]),
    'gap at the end': (99, [(0, 25, 1), (25, 60, 1)], [(60, 99, 1)]),
    'two adjacent lost slices': (99, [(0, 13, 1), (70, 99, 1)], [(13, 70, 0)]),
    'two separate gaps': (99, [(0, 13, 1), (40, 70, 1), (90, 99, 1)], [(13, 40, 0), (70, 90, 1)]),
    'first and last': (99, [(40, 70, 1), (13, 40, 1)], [(0, 13, 1), (70, 99, 0)]),
    'permuted order': (99, [(60, 99, 1), (0, 25, 1), (40, 60, 1)], [(25, 40, 1)]),
    'a failed slice': (99, [(0, 25, 1), (25, 31, 0), (60, 99, 1)], [(25, 60, 0)]),
    'a failed slice that claims everything': (99, [(0, 25, 1), (25, 99, 0), (60, 99, 1)], [(25, 60, 0)]),
    'a short slice': (99, [(0, 20, 1), (30, 99, 1)], [(20, 30, 0)]),
    'an empty and an overlong slice are not good': (99, [(0, 50, 1), (50, 50, 1), (50, 100, 1)], [(50, 99, 0)]),
    'an overlap': (99, [(0, 31, 1), (30, 99, 1)], None),
    'a slice twice': (99, [(0, 30, 1), (0, 30, 1), (30, 99, 1)], None),
    'an overlap of a failed slice does not reject': (99, [(0, 31, 1), (30, 60, 0), (60, 99, 1)], [(31, 60, 0)]),
    'no good slice': (99, [(0, 30, 0), (30, 99, 0)], None),
    'one MB': (1, [(0, 1, 1)], []),
    '32 slices, every other one lost': (6400, [(100 * k, 100 * (k + 1), 1) for k in range(0, 64, 2)],
                                        [(100 * k, 100 * (k + 1), k // 2) for k in range(1, 64, 2)]),
    '32 slices of one MB, reversed': (33, [(k, k + 1, 1) for k in range(31, -1, -1)], [(32, 33, 0)]),
}


@pytest.mark.parametrize('name', list(DIRECTED))
def test_gap_rule_directed(libpath, name):
    import h264mi
    total, slices, want = DIRECTED[name]
    assert ref_gaps(total, slices) == want, 'the restatement disagrees with the table'
    assert h264mi.conceal_gaps(total, slices) == want


def test_gap_rule_arguments(libpath):
    import h264mi
    ok = [(0, 10, 1)]
    assert h264mi.conceal_gaps(0, ok) is None and h264mi.conceal_gaps(-5, ok) is None
    assert h264mi.conceal_gaps(20, []) is None and h264mi.conceal_gaps(33, [(k, k + 1, 1) for k in range(33)]) is None
    # fewer triples than gaps: the count is still reported, nothing is written past max_gaps
    import ctypes
    L = h264mi.lib()
    f, e, k = (ctypes.c_int * 2)(10, 30), (ctypes.c_int * 2)(20, 40), (ctypes.c_int * 2)(1, 1)
    out = (ctypes.c_int * 6)(*[-7] * 6)
    assert L.h264mi_conceal_gaps(50, 2, f, e, k, out, 1) == 3 and list(out) == [0, 10, 0, -7, -7, -7]
    assert L.h264mi_conceal_gaps(50, 2, f, e, k, None, 0) == 3 and L.h264mi_conceal_gaps(50, 2, f, e, k, None, 1) == -1
    assert L.h264mi_conceal_gaps(50, 2, None, e, k, out, 2) == -1


def test_gap_rule_random(libpath):
    import h264mi
    rng = np.random.default_rng(20)
    rejected = tiled = gapped = 0
    for it in range(4000):
        total = int(rng.choice([1, 2, 7, 99, 396, 8160]))
        n = int(rng.integers(1, 33))
        if it % 2:  # cut the picture into n pieces, then damage the table a little
            cuts = sorted(set([0, total] + [int(v) for v in rng.integers(0, total + 1, n - 1)]))
            slices = [[a, b, 1] for a, b in zip(cuts, cuts[1:])]
            for sl in slices:
                r = rng.random()
                if r < 0.15:
                    sl[2] = 0
                elif r < 0.25:
                    sl[1] = int(rng.integers(sl[0], sl[1] + 1))      # short (or empty)
                elif r < 0.28:
                    sl[1] = min(total + 1, sl[1] + int(rng.integers(1, 4)))  # into the next one, or past the picture
            keep = rng.random(len(slices)) > 0.15
            slices = [tuple(sl) for sl, k in zip(slices, keep) if k] or [tuple(slices[0])]
            rng.shuffle(slices)
            slices = [tuple(int(v) for v in sl) for sl in slices]
        else:       # anything
            slices = [(int(rng.integers(-2, total + 2)), int(rng.integers(-2, total + 3)), int(rng.integers(0, 2))) for _ in range(n)]
        want = ref_gaps(total, slices)
        assert h264mi.conceal_gaps(total, slices) == want, (total, slices)
        rejected += want is None
        tiled += want == []
        gapped += bool(want)
    assert rejected > 400 and tiled > 20 and gapped > 1000, (rejected, tiled, gapped)


def tables_text():
    """the directed tables as tools/conceal_host_san.cc reads them"""
    lines = []
    for total, slices, want in DIRECTED.values():
        v = [total, len(slices)] + [x for sl in slices for x in sl] + [-1 if want is None else len(want)] + [x for gp in (want or []) for x in gp]
        lines.append(' '.join(map(str, v)))
    return '\n'.join(lines) + '\n'


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_gap_rule_under_host_sanitizers(tmp_path):
    """tools/conceal_host_san.cc, a program of its own (nothing is loaded into Python): conceal_gaps and conceal_clean
    over the directed tables above (tests/golden/conceal_tables.txt), every array in a heap block of exactly its size,
    under ASan and UBSan; its output is the one recorded in profiles/conceal/conceal_host_san.txt"""
    tables = os.path.join(ROOT, 'tests', 'golden', 'conceal_tables.txt')
    assert open(tables).read() == tables_text(), 'tests/golden/conceal_tables.txt is not the DIRECTED tables'
    exe = str(tmp_path / 'conceal_host_san')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-fno-omit-frame-pointer', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', os.path.join(ROOT, 'tools', 'conceal_host_san.cc'), '-o', exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
    r = subprocess.run([exe, tables], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.endswith('ok\n'), r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout == open(os.path.join(ROOT, 'profiles', 'conceal', 'conceal_host_san.txt')).read()


LAYOUT = [dict(first=0, qp_delta=2), dict(first=17, qp_delta=-4, dbk=(2, 1, -1)), dict(first=41, dbk=(1, 0, 0)),
          dict(first=70, qp_delta=6), dict(first=93)]


@pytest.mark.parametrize('lost', [(0,), (2,), (4,), (1, 2), (0, 4), (1, 3)], ids=str)
def test_construction_on_the_oracle(oracle, lost):
    """the full unit of a lossy one, decoded by the oracle: every MB of an all-skip slice is P_Skip with zero vectors,
    refIdx 0, the synthetic slice's first_mb, the donor's QP and loop-filter fields, and before the loop filter it is
    the co-located block of the previous picture (8.4.1.1: in a slice of nothing but skips mvp is never used)"""
    from concealgen import full_layout, runs, slice_end
    g = Pair(11, 9, seed=60 + sum(lost), init_qp=30)
    d = oracle.decoder()
    d.set_capture(True)
    rc, prev, _, _ = d.decode(g.idr(slices=LAYOUT))
    assert rc == 1
    rc, prev, _, _ = d.decode(g.lossy(LAYOUT, ())[0])   # a P picture first: the reference has motion and residue in it
    assert rc == 1
    full, lossy, nlost = g.lossy(LAYOUT, lost)
    assert len(lossy) < len(full)
    rc, pic, w, h = d.decode(full)
    assert rc == 1 and (w, h) == (176, 144)
    Y, U, V = d.prefilter()
    rec = d.records()
    py = prev[:w * h].reshape(h, w)
    pu = prev[w * h:w * h * 5 // 4].reshape(h // 2, w // 2)
    pv = prev[w * h * 5 // 4:].reshape(h // 2, w // 2)
    seen = 0
    for run in runs(lost):
        donor = LAYOUT[run[0] - 1 if run[0] > 0 else run[-1] + 1]
        first, end = LAYOUT[run[0]]['first'], slice_end(LAYOUT, run[-1], 99)
        idc, fa, fb = donor.get('dbk', (0, 0, 0))
        for addr in range(first, end):
            r, x, y = rec[addr], addr % 11 * 16, addr // 11 * 16
            assert r[0] == 3 and r[1] == 30 + donor.get('qp_delta', 0) and not r[2:18].any()
            assert list(r[18:22]) == [0] * 4 and not r[22:54].any()
            assert r[54] == first and (r[55], r[56], r[57]) == (idc, 2 * fa if idc != 1 else 0, 2 * fb if idc != 1 else 0)
            assert np.array_equal(Y[y:y + 16, x:x + 16], py[y:y + 16, x:x + 16])
            assert np.array_equal(U[y // 2:y // 2 + 8, x // 2:x // 2 + 8], pu[y // 2:y // 2 + 8, x // 2:x // 2 + 8])
            assert np.array_equal(V[y // 2:y // 2 + 8, x // 2:x // 2 + 8], pv[y // 2:y // 2 + 8, x // 2:x // 2 + 8])
            seen += 1
    assert seen == nlost > 0
    # and the gap rule, fed the lossy unit's slice table, names exactly these synthetic slices
    import h264mi
    table = [(LAYOUT[i]['first'], slice_end(LAYOUT, i, 99), 1) for i in range(len(LAYOUT)) if i not in lost]
    kept = [i for i in range(len(LAYOUT)) if i not in lost]
    gaps = h264mi.conceal_gaps(99, table)
    assert [(a, b, kept[k]) for a, b, k in gaps] == [(LAYOUT[r[0]]['first'], slice_end(LAYOUT, r[-1], 99), r[0] - 1 if r[0] > 0 else r[-1] + 1)
                                                      for r in runs(lost)]
