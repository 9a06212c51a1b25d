"""Class audit of the frame-level rate control, CPU half.

tests/rcref.py restates the frame-level rate control from the fixture and DESIGN §3.6 and names every outcome of every
decision as a class. This module

  * holds every class to one of three states: required (claimed by exactly one directed sequence of rcaudit.DIRECTED or
    one long run, and reached by it), excluded with a derivation (no sequence may ever reach it), or not reached with
    a reason;
  * holds the oracle to the model on every frame of every directed sequence in all sixteen fields of rc_state, the model
    fed with the oracle's slice bytes and average QP and its complexity from rcref.frame_complexity;
  * holds the oracle's sequence parameters to rcref.seq_params around every threshold;
  * shows that each single mutation of the model is caught by a directed sequence against the oracle;
  * measures which classes the inputs of the GPU tests that were there before reach, and prints the report.

tests/test_gpu_rc_audit.py drives the same sequences through the GPU encoder.
"""
import ctypes

import pytest

import rcaudit
import rcref


def test_classes_partition():
    known = set(rcref.RC_CLASSES)
    assert set(rcaudit.EXCLUDED) <= known and set(rcaudit.NOT_REACHED) <= known
    assert not set(rcaudit.EXCLUDED) & set(rcaudit.NOT_REACHED)
    for k, why in {**rcaudit.EXCLUDED, **rcaudit.NOT_REACHED}.items():
        assert len(why) > 80, f'{k}: an exclusion needs its derivation'
    claims = [t for s in list(rcaudit.directed_seqs()) + list(rcaudit.long_runs().values()) for t in s.targets]
    assert sorted(claims) == sorted(rcaudit.required()), (set(rcaudit.required()) - set(claims), [c for c in claims if claims.count(c) > 1])
    for fam in ('SKIP_', 'POST_', 'REFRESH_', 'VGOP_', 'TGT_', 'IDRQP_', 'PQP_', 'PRATIO_', 'IRATIO_', 'QSTEP_', 'UPD_', 'SEQ_', 'FC_'):
        assert any(c.startswith(fam) for c in known), fam


def test_directed_sequences_keep_to_small_geometries():
    for s in rcaudit.directed_seqs():
        assert (s.w, s.h) in rcaudit.GEOMETRIES + rcaudit.TABLE_GEOMETRIES and len(s) <= 40, s.name
        assert (s.w, s.h) not in rcaudit.TABLE_GEOMETRIES or len(s) == 1, s.name


def test_oracle_equals_model_and_sequences_reach_their_classes(oracle):
    """every frame, all sixteen fields; every sequence reaches what it claims; nothing reaches an excluded class"""
    for s, run in zip(rcaudit.directed_seqs(), rcaudit.directed_runs()):
        m, bad = rcaudit.replay(s, run)
        assert bad is None, f'{s.name}: frame {bad[0]} field {bad[1]}: model {bad[2]} != oracle {bad[3]}'
        missed = [t for t in s.targets if not m.counts[t]]
        assert not missed, f'{s.name} no longer reaches {missed}'
        hit = [k for k in m.counts if k in rcaudit.EXCLUDED or k in rcaudit.NOT_REACHED]
        assert not hit, f'{s.name} reaches {hit}: the derivation is wrong'


@pytest.mark.parametrize('which', ['p', 'idr'])
def test_long_runs(oracle, which):
    """33 000 static P frames (pframe_num past 254, frame_num past 32767) and 300 IDRs (idr_num past 254): the oracle
    == the model on every frame; the frames' bytes are kept only in the windows the GPU test compares"""
    s = rcaudit.long_runs()[which]
    keep = {t for w in rcaudit.LONG_WINDOWS[which] for t in w}
    m, bad = rcaudit.replay(s, rcaudit.oracle_run(oracle, s, keep))
    assert bad is None, f'{s.name}: frame {bad[0]} field {bad[1]}: model {bad[2]} != oracle {bad[3]}'
    assert all(m.counts[t] for t in s.targets), s.name
    assert not [k for k in m.counts if k in rcaudit.EXCLUDED]
    assert m.state()['pframes' if which == 'p' else 'idrs'] == 255


def test_seq_params_vs_oracle(oracle):
    """the table part around every threshold: every cell of the 4 x 5 table from both sides of its bpp threshold, both
    sides of the three area thresholds, and bpp == threshold exactly"""
    seen = set()
    for w, h, br in rcaudit.table_cases():
        p = rcref.seq_params(w, h, br)
        lo, hi = ctypes.c_int(), ctypes.c_int()
        q = oracle.L.h264o_rc_idr_params(w, h, br, ctypes.byref(lo), ctypes.byref(hi))
        assert (q, lo.value, hi.value) == (p['init_qp'], p['idr_lo'], p['idr_hi']), (w, h, br, p)
        seen.add((p['area'], p['col']))
    assert len(seen) == 20, sorted(seen)
    assert rcref.seq_params(16, 16, 3840)['col'] == 0 and rcref.seq_params(16, 16, 3841)['col'] == 1
    assert [rcref.seq_params(w, h, 300000)['area'] for w, h in ((256, 112), (1808, 16), (480, 240), (656, 176), (800, 576), (544, 848))] == [0, 1, 1, 2, 2, 3]
    # bits per frame, the bit bounds, the skip buffer and the skip QP show in the first frame's state
    for w, h, br in ((16, 16, 3840), (496, 16, 64000), (48, 48, 123457)):
        s = rcaudit.Seq(w, h, br, True, 'nn')
        run = rcaudit.oracle_run(oracle, s)
        m, bad = rcaudit.replay(s, run)
        assert bad is None and run[0][1]['bpf'] == rcref.seq_params(w, h, br)['bpf'], (w, h, br, bad)


def test_sensitivity(oracle):
    """each single mutation of the model disagrees with the oracle on at least one directed sequence (the two
    saturations: on the first 300 frames of their long run), so the sequences would notice a kernel wrong in that way"""
    caught = {}
    longs = rcaudit.long_runs()
    for mut in rcref.PyRc.MUTATIONS:
        if mut in ('pframes_unsaturated', 'idrs_unsaturated'):
            s = longs['p' if mut.startswith('p') else 'idr']
            bad = rcaudit.replay(s, _long_head(oracle, mut[0]), mut, stop=300)[1]
            if bad:
                caught[mut] = (s.name, bad)
            continue
        for s, run in zip(rcaudit.directed_seqs(), rcaudit.directed_runs()):
            bad = rcaudit.replay(s, run, mut)[1]
            if bad:
                caught[mut] = (s.name, bad)
                break
    print()
    for mut, (name, bad) in caught.items():
        print(f'mutation {mut}: caught by {name} at frame {bad[0]} in {bad[1]}')
    missing = sorted(set(rcref.PyRc.MUTATIONS) - set(caught))
    assert not missing, missing


_HEADS = {}


def _long_head(oracle, which):
    if which not in _HEADS:
        s = rcaudit.long_runs()['p' if which == 'p' else 'idr']
        head = rcaudit.Seq(s.w, s.h, s.br, s.skip, s.schedule[:300], [t for t in s.idr if t < 300])
        _HEADS[which] = rcaudit.oracle_run(oracle, head, keep=())
    return _HEADS[which]


def test_report(oracle):
    """class, count over the directed sequences, first directed sequence, and the suite's reach before this audit:
    count and first input over the inputs of the GPU tests that were there"""
    total, first = {}, {}
    seqs = list(rcaudit.directed_seqs())
    for s, run in zip(seqs, rcaudit.directed_runs()):
        m, _ = rcaudit.replay(s, run)
        for k, n in m.counts.items():
            total[k] = total.get(k, 0) + n
            first.setdefault(k, s.name)
    for s in rcaudit.long_runs().values():
        for t in s.targets:
            total.setdefault(t, 1)
            first.setdefault(t, s.name)
    suite = rcaudit.suite_reach()
    print()
    for c in rcref.RC_CLASSES:
        state = 'excluded' if c in rcaudit.EXCLUDED else 'not reached' if c in rcaudit.NOT_REACHED else ''
        sn, sf = suite.get(c, (0, '-'))
        print(f'{c:28s} {total.get(c, 0):6d} {first.get(c, state or "-"):48s} suite {sn:6d} {sf}')
    req = rcaudit.required()
    took = [c for c in req if c in suite]
    print(f'classes {len(rcref.RC_CLASSES)}: required {len(req)}, excluded {len(rcaudit.EXCLUDED)}, not reached {len(rcaudit.NOT_REACHED)}; '
          f'the suite\'s inputs before this audit took {len(took)} of the {len(req)} required; missed: {" ".join(c for c in req if c not in suite)}')
    assert not [c for c in suite if c in rcaudit.EXCLUDED], 'a suite input reaches an excluded class'
    assert all(total.get(c, 0) > 0 for c in req)
