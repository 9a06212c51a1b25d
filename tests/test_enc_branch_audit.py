"""Decision-branch audit of the encoder, CPU half.

The oracle encoder names every outcome of its forward decisions -- P_Skip judge, intra alternative, integer search,
sub-pel refinement, quantiser and CBP rules, QP inside a frame, each P-slice family at the picture's edges -- as a class
(oracle/h264o_enc.c BRANCH_CLASSES) and counts them. This module

  * runs the oracle over every input the GPU encoder-vs-oracle tests feed (encaudit.suite_clips) and counts the classes
    those inputs reach;
  * holds every class to one of three states: reached by the suite's inputs or by a directed clip that names it
    (encaudit.DIRECTED), excluded with a derivation (encaudit.EXCLUDED; no content may ever reach it), or on the
    not-reached list of at most three (encaudit.NOT_REACHED; none of the judge, intra, sub-pel or residual families);
  * checks on every directed frame that the oracle decoder reproduces the oracle encoder's reconstruction, and that
    tests/parseref.py parses the directed streams (its CAVLC class counters are reported);
  * checks the macroblock-level mismatch message on an encoder fed a frame that differs in one sample.

tests/test_gpu_enc_branches.py drives the directed clips through the GPU encoder.
"""
import functools

import numpy as np

import encaudit
import parseref


@functools.lru_cache(maxsize=None)
def suite_counts():
    """classes the suite's own inputs reach: (small geometries, 720p / 1080p), each input run once"""
    import os
    from _oracle import Oracle
    oracle = Oracle(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle', 'build', 'libh264_oracle.so'))
    out = []
    for group in encaudit.suite_clips(oracle):
        tot = np.zeros(len(oracle.branch_names()), np.int64)
        for c in group:
            tot += encaudit.run_clip(oracle, c)[0]
        out.append(tot)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def directed_runs():
    import os
    from _oracle import Oracle
    oracle = Oracle(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle', 'build', 'libh264_oracle.so'))
    return tuple(encaudit.run_clip(oracle, c, decode=True) for c in encaudit.directed_clips())


def test_class_table(oracle):
    names = oracle.branch_names()
    assert len(names) == len(set(names)) == oracle.L.h264o_enc_branch_classes() and len(names) <= 64 * oracle.L.h264o_enc_branch_words()
    assert oracle.L.h264o_enc_branch_name(len(names)) is None
    for fam in ('J_', 'IA_', 'II_', 'IP_', 'S_', 'SP_HALF_', 'SP_QUARTER_', 'R_', 'Q_ROW_', 'Q_GOM_', 'G_'):
        assert any(n.startswith(fam) for n in names), fam
    known = set(names)
    assert set(encaudit.EXCLUDED) <= known and set(encaudit.NOT_REACHED) <= known
    for c in encaudit.directed_clips():
        assert set(c.targets) <= known, c.name


def test_directed_clips_keep_to_the_issue_s_limits():
    for c in encaudit.directed_clips():
        assert (c.w, c.h) in ((16, 16), (16, 48), (48, 16), (48, 48), (80, 48), (176, 144)) and len(c.frames) <= 8 and not c.skip, c.name


def test_directed_clips_reach_their_classes_and_decode(oracle):
    """every directed clip reaches each class it is in the set for; run_clip(decode=True) has held the oracle decoder
    to the encoder's reconstruction on every frame"""
    names = oracle.branch_names()
    for clip, (counts, frames) in zip(encaudit.directed_clips(), directed_runs()):
        missed = [t for t in clip.targets if counts[names.index(t)] == 0]
        assert not missed, f'{clip.name} no longer reaches {missed}'
        assert all(nal for nal, _, _ in frames), clip.name  # frame skipping is off: every frame is coded


def test_every_class_is_reached_excluded_or_listed(oracle):
    names = oracle.branch_names()
    small, large = suite_counts()
    suite = small + large
    directed = sum(c for c, _ in directed_runs())
    aimed = {t for c in encaudit.directed_clips() for t in c.targets}
    for k, n in enumerate(names):
        if n in encaudit.EXCLUDED:
            assert suite[k] == 0 and directed[k] == 0, f'excluded class {n} was reached: its derivation is wrong'
            assert len(encaudit.EXCLUDED[n]) > 80, f'{n}: an exclusion needs its derivation'
        elif n in encaudit.NOT_REACHED:
            assert suite[k] == 0 and directed[k] == 0, f'{n} is reached: take it off the not-reached list'
        else:
            assert suite[k] > 0 or (n in aimed and directed[k] > 0), f'{n}: not reached by the suite, and no directed clip is held to it'
    assert len(encaudit.NOT_REACHED) <= 3
    assert not [n for n in encaudit.NOT_REACHED if n.startswith(('J_', 'IA_', 'II_', 'IP_', 'SP_', 'R_'))]
    assert not set(encaudit.EXCLUDED) & set(encaudit.NOT_REACHED)
    # the directed set alone reaches everything that is not excluded: the GPU module sees every class at a small geometry
    alone = [n for k, n in enumerate(names) if directed[k] == 0 and n not in encaudit.EXCLUDED and n not in encaudit.NOT_REACHED]
    assert not alone, alone
    print(f'\nclasses {len(names)}: suite inputs reach {int((suite > 0).sum())} (small geometries {int((small > 0).sum())}), '
          f'with the directed clips {int(((suite + directed) > 0).sum())}, excluded {len(encaudit.EXCLUDED)}, not reached {len(encaudit.NOT_REACHED)}')


def test_counters_agree_with_me_stats(oracle):
    """h264o_enc_me_stats keeps working, and its six counters are sums of classes"""
    names = oracle.branch_names()
    clip = encaudit.directed_clips()[10]
    oe = clip.encoder(oracle)
    for f in clip.frames:
        oe.encode(f)
    st = np.zeros(6, np.int32)
    oracle.L.h264o_enc_me_stats(oe.e, st.ctypes.data)
    c = dict(zip(names, oe.branch_counts().tolist()))
    assert st[0] == c['S_CROSS_STAYED'] + c['S_CROSS_MOVED_H'] + c['S_CROSS_MOVED_V'] > 0
    assert st[1] == c['S_CROSS_MOVED_H'] + c['S_CROSS_MOVED_V']
    assert st[2] >= c['S_START_A'] + c['S_START_B'] + c['S_START_C'] + c['S_START_C_TOPLEFT'] > 0  # st[2] counts every improvement
    assert st[3] == sum(c[k] for k in ('J_TAKE_SAD_ZERO', 'J_TAKE_BELOW_PRED_SAD', 'J_TAKE_BELOW_COLOC_SAD', 'J_TAKE_RESIDUAL', 'J_NOT_TAKEN')) > 0
    assert st[4] == c['J_DOUBLE_CHECK'] and st[5] == c['IA_AFTER_SKIP_WON'] + c['IA_AFTER_SEARCH_WON']
    # the per-MB records of the last frame hold exactly the classes of that frame
    before = oe.branch_counts()
    oe.encode(clip.frames[-1])
    frame = oe.branch_counts() - before
    rec = oe.mb_branches()
    assert len(rec) == ((clip.w + 15) // 16) * ((clip.h + 15) // 16)
    assert {k for r in rec for k in r} == set(np.flatnonzero(frame).tolist())


def test_parse_reference_over_directed_streams(oracle):
    """the writer side: tests/parseref.py parses every directed stream; its CAVLC class counters are reported"""
    total = parseref.Counter()
    for clip, (_, frames) in zip(encaudit.directed_clips(), directed_runs()):
        state = parseref.State()
        for nal, _, _ in frames:
            p = parseref.parse(nal, state)
            assert p.size == (clip.w, clip.h), clip.name
            total.update(p.counts)
    req = parseref.required_classes()
    hit = sum(1 for k in req if total[k])
    assert hit > 0
    print(f'\nparse classes reached by the directed encoder streams: {hit} of {len(req)}')


def _one_sample_off(clip, t, mb, mbw):
    f = clip.frames[t].copy()
    i = (mb // mbw * 16 + 5) * clip.w + (mb % mbw) * 16 + 7
    f[i] = f[i] + 90 if f[i] < 128 else f[i] - 90
    return f


def test_mismatch_message_names_the_macroblock(oracle):
    """an encoder fed a frame that differs in one sample of one macroblock stands in for a diverging GPU: the message
    names that macroblock with both sides' values and the oracle's classes, through the macroblock records (batch
    path) and through the bytes alone (C-ABI path)"""
    clip = encaudit.directed_clips()[12]  # 80x48 at 3 Mbps
    mbw, mb, t_bad = 5, 7, 2
    for by_records in (True, False):
        ref, bad = clip.encoder(oracle), clip.encoder(oracle)
        ex = encaudit.Explainer(oracle, ref, clip.name, gpu=(lambda: bad.mbinfo()) if by_records else None)
        msg = None
        for t in range(t_bad + 1):
            r = ref.encode(clip.frames[t])
            g = bad.encode(clip.frames[t] if t < t_bad else _one_sample_off(clip, t, mb, mbw))
            try:
                ex.check(t, g, r)
            except AssertionError as e:
                msg = str(e)
        assert msg is not None
        assert f'frame {t_bad}' in msg and f'first differing macroblock {mb} (x 2, y 1)' in msg, msg
        assert ' | oracle ' in msg and 'GPU ' in msg and 'oracle classes: ' in msg and 'QP ' in msg and 'mv (' in msg, msg
        assert any(n in msg.split('oracle classes: ')[1] for n in oracle.branch_names()), msg


def test_mismatch_message_without_a_record_difference(oracle):
    names = oracle.branch_names()
    info = np.zeros((4, 8), np.int32)
    msg = encaudit.explain_mismatch('x frame 0', names, 2, info, info.copy(), [[0]] * 4, 10, 12)
    assert '10 B vs 12 B' in msg and 'every macroblock agrees' in msg
    assert 'no macroblock record' in encaudit.explain_mismatch('x frame 0', names, 2, None, info, [[0]] * 4)
