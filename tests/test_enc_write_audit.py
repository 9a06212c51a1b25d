"""Write-class audit of the encoder's bit writer, CPU half.

tests/writeaudit.py names every path of csrc/enc_bits.inc's CAVLC and packer that the bytes can tell apart as a class and
counts the classes from an access unit's bytes. This module runs the oracle over writeaudit.directed_clips() and the small
clips of encaudit.suite_clips() and holds every class to one of two states: required, and then reached by the directed
clip that claims it, or not reached with a reason from the syntax or the encoder's rules (no clip may then reach it). The
classes of slice index > 0 are claimed here and reached in tests/test_gpu_enc_write.py, on the GPU encoder's three-slice
bytes: the oracle encoder codes one slice per picture. Every directed clip decodes with the oracle decoder to the
encoder's reconstruction."""
import functools
import os
import re

import encaudit
import writeaudit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle():
    from _oracle import Oracle
    return Oracle(os.path.join(ROOT, 'oracle', 'build', 'libh264_oracle.so'))


@functools.lru_cache(maxsize=None)
def directed_counts():
    """per directed clip the classes of the oracle's bytes; run_clip(decode=True) holds the oracle decoder to the
    encoder's reconstruction on every frame"""
    oracle = _oracle()
    out = []
    for c in writeaudit.directed_clips():
        _, frames = encaudit.run_clip(oracle, c, decode=True)
        assert all(nal for nal, _, _ in frames), c.name
        out.append(writeaudit.count_clip([nal for nal, _, _ in frames]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def suite_counts():
    """the classes the suite's own small clips reach, and the first clip to reach each"""
    oracle = _oracle()
    total, first = writeaudit.Counter(), {}
    for c in encaudit.suite_clips(oracle)[0]:
        got = writeaudit.count_clip([nal for nal, _, _ in encaudit.run_clip(oracle, c)[1]])
        for k in got:
            if got[k]:
                first.setdefault(k, c.name)
        total.update(got)
    return total, first


def test_constants_follow_the_source(oracle):
    src = open(os.path.join(ROOT, 'openh264-wasm_amd', 'csrc', 'enc_bits.inc')).read()
    assert int(re.search(r'#define H264MI_PACK_THREADS (\d+)', src).group(1)) == writeaudit.PACK_THREADS
    assert {int(v) for v in re.findall(r'constexpr int PACK_MBT = (\d+);', src)} == {writeaudit.PACK_MBT}
    assert {int(v) for v in re.findall(r'constexpr int EPB = (\d+);', src)} == {writeaudit.EPB}
    assert 'per = ((nmb + PACK_THREADS - 1) / PACK_THREADS + 3) & ~3' in src
    assert 'mg = m0 & ~3, per = ((m1 - mg + PACK_THREADS - 1) / PACK_THREADS + 3) & ~3' in src
    for line in writeaudit.position_classes().values():   # the quoted lines are the source's
        for q in re.findall(r'"([^"]+)"', line):
            for part in q.split('...'):
                assert part.strip() in src, part


def test_block_cuts_follow_parseref_s_names(oracle):
    """writeaudit cuts a macroblock's words (parseref.Parsed.words) into residual blocks by the name 'coeff_token' and
    drops the run by the name 'mb_skip_run': as many such words as parseref counted code words of either kind"""
    import parseref
    clip = next(c for c in writeaudit.directed_clips() if c.name.startswith('mix_80x48'))
    state, tokens, runs, want_tokens, want_runs = parseref.State(), 0, 0, 0, 0
    for nal, _, _ in encaudit.run_clip(oracle, clip)[1]:
        p = parseref.parse(nal, state)
        words = [e for mb in range(p.syntax.shape[0]) for e in p.words(mb)]
        tokens += sum('coeff_token' in e[0] for e in words)
        runs += sum(e[0] == 'mb_skip_run' for e in words)
        want_tokens += sum(v for k, v in p.counts.items() if k[0] == 'coeff_token')
        want_runs += sum(1 for e in words if e[0] == 'mb_skip_run')
        if int(p.syntax[0, 1]) == 0:
            assert any(e[0] == 'mb_skip_run' for e in words)
    assert tokens == want_tokens > 0 and runs == want_runs > 0


def test_class_lists():
    allc, req = writeaudit.all_classes(), writeaudit.required()
    assert set(writeaudit.NOT_REACHED) <= allc
    assert req | set(writeaudit.NOT_REACHED) == allc and not req & set(writeaudit.NOT_REACHED)
    assert all(len(r) > 60 for r in writeaudit.NOT_REACHED.values())
    clips = writeaudit.directed_clips()
    claimed = [t for c in clips for t in c.targets + c.slice_targets]
    assert len(claimed) == len(set(claimed)), 'a class is claimed twice'
    assert set(claimed) == req, sorted(req ^ set(claimed), key=str)
    for c in clips:
        assert not [t for t in c.targets if writeaudit.is_slice_class(t)], c.name
        assert all(writeaudit.is_slice_class(t) for t in c.slice_targets), c.name
        assert 2 <= len(c.frames) <= 4 and not c.skip and not c.gom, c.name
    geo = {(c.w, c.h) for c in clips}
    assert {(16, 4096), (8192, 16)} <= geo
    assert any(writeaudit.thread_ranges(0, (c.w // 16) * (c.h // 16))[1] > writeaudit.PACK_MBT for c in clips)


def test_directed_clips_reach_their_classes_and_decode(oracle):
    for clip, got in zip(writeaudit.directed_clips(), directed_counts()):
        missed = [t for t in clip.targets if not got[t]]
        assert not missed, f'{clip.name} no longer reaches {missed}'


def test_every_class_is_reached_or_listed(oracle):
    clips, counts = writeaudit.directed_clips(), directed_counts()
    total, first = writeaudit.Counter(), {}
    for clip, got in zip(clips, counts):
        for k in got:
            if got[k]:
                first.setdefault(k, clip.name)
        total.update(got)
    suite, suite_first = suite_counts()
    for k, why in writeaudit.NOT_REACHED.items():
        assert not total[k] and not suite[k], f'{k} is reached by {first.get(k) or suite_first.get(k)}: its reason is wrong'
    claim = {t: c.name for c in clips for t in c.targets}
    cpu = {k for k in writeaudit.required() if not writeaudit.is_slice_class(k)}
    missing = {}
    for k in cpu:
        if not counts[[c.name for c in clips].index(claim[k])][k]:
            missing.setdefault(claim[k], []).append(k)
    assert not missing, f'classes no longer reached, by the clip that claims them: {missing}'
    assert not [k for k in total if total[k] and writeaudit.is_slice_class(k)]   # one slice per picture on this side
    print(f'\nwriter classes {len(writeaudit.all_classes())}: required {len(writeaudit.required())} ({len(cpu)} on one-slice bytes), '
          f'not reached {len(writeaudit.NOT_REACHED)}; the suite\'s small clips alone reach {sum(1 for k in cpu if suite[k])} of {len(cpu)}')
    print('position classes the suite\'s small clips miss:', sorted((k for k in cpu if not suite[k] and k in writeaudit.position_classes()), key=str))
    for k in sorted(cpu, key=str):
        print(f'  {k}: {total[k]}, first {first[k]}' + (f'; suite {suite[k]}, first {suite_first[k]}' if suite[k] else '; suite 0'))
