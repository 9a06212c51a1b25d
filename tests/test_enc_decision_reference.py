"""CPU: the oracle encoder's P-macroblock decisions held to tests/mdref.py: on every directed clip coded
with one slice, every frame, every macroblock; on the suite's inputs up to 352x288; every mutation of the non-slice kinds
caught on the oracle's bytes by the clip that claims it; the mismatch message."""
import functools

import numpy as np
import pytest

import encaudit
import mdaudit
import mdref

CLIPS = {c.name: c for c in mdaudit.clips()}


@functools.lru_cache(maxsize=None)
def _pictures(oracle, name):
    c = CLIPS[name]
    return tuple(mdaudit.chain(c, mdaudit.oracle_units(oracle, c)))


def _bound_open_rows(clip, k):
    """exact GOM only (out of scope): a row without a carrier of mb_qp_delta is accepted at any QP of the
    window. Such a row is one whose macroblocks are all skipped or without residual; in every exact-GOM input at least
    half of the rows hold content that changes in every frame (the moving half and the row the edge cuts, fresh noise, a
    moving synthetic scene), so more than half of the rows open means the check has loosened. Without exact GOM none is."""
    if clip.gom:
        assert 2 * k.free_rows <= k.rows_planned, f'{clip.name}: {k.free_rows} of {k.rows_planned} rows of P pictures are without a carrier'
    else:
        assert k.free_rows == 0, clip.name


@pytest.mark.parametrize('name', list(CLIPS))
def test_directed_clip_decisions_vs_mdref(oracle, name):
    """reference == the oracle's bytes on every macroblock of every frame, and the mutations the clip claims are caught"""
    pics = _pictures(oracle, name)
    k = mdref.Checked()
    mm = mdaudit.check_all(pics, None, k)
    assert mm is None, str(mm)
    assert k.mbs == sum(p.nmb for p in pics)
    print(f'{name}: {k.mbs} macroblocks, outcomes {k.outcomes}, intra macroblocks whose I4 / I16 kind is not restated: {k.intra_kind_open}, '
          f'I16x16 modes checked: {k.i16_modes}, exact-GOM rows without a carrier: {k.free_rows}')
    _bound_open_rows(CLIPS[name], k)
    for m in mdref.MUTATIONS:
        if m.kind != 'slice' and mdaudit.CLAIMS[m.name][0] == name:
            got = mdaudit.catches(pics, m)
            assert got is not None, f'{name}: "{m.name}" is not caught on the oracle\'s bytes'
            assert f'macroblock {got.mb} ' in str(got)
            if CLIPS[name].gom:   # exact GOM leaves a row without a carrier open: the catch must not rest on such a row
                p = next(q for q in pics if q.label in str(got))
                r = got.mb // p.mbw
                assert p.carrier[r * p.mbw:(r + 1) * p.mbw].any(), f'{name}: "{m.name}" is caught in a row without a carrier'


def test_every_mutation_is_claimed_by_a_clip():
    for m in mdref.MUTATIONS:
        clip, n = mdaudit.CLAIMS[m.name]
        assert clip in CLIPS and (n > 1) == (m.kind == 'slice'), m.name
    assert len({m.name for m in mdref.MUTATIONS}) == len(mdref.MUTATIONS) == len(mdaudit.CLAIMS)


N_SUITE = 39   # encaudit.suite_clips' clips up to 352x288, one test case each to keep a case short


@functools.lru_cache(maxsize=None)
def _suite(oracle):
    return tuple(c for c in encaudit.suite_clips(oracle)[0] if c.w * c.h <= 352 * 288)


@pytest.mark.parametrize('i', range(N_SUITE))
def test_suite_inputs_decisions_vs_mdref(oracle, i):
    """encaudit.suite_clips up to 352x288 (the exact-GOM ones with the row QP from their carriers)"""
    clips = _suite(oracle)
    assert len(clips) == N_SUITE
    c = clips[i]
    k = mdref.Checked()
    mm = mdaudit.check_all(mdaudit.chain(c, mdaudit.oracle_units(oracle, c)), None, k)
    assert mm is None, str(mm)
    assert k.mbs > 0
    _bound_open_rows(c, k)
    print(f'{c.name}: {k.mbs} macroblocks, outcomes {k.outcomes}, intra macroblocks whose I4 / I16 kind is not restated: {k.intra_kind_open}')


def test_skip_sads_carried_in_effect(oracle):
    """the skip SADs the reference carries decide what the oracle's decide: with them dropped (no co-located SAD, no
    predicted SAD) the reference leaves the oracle's bytes on the clips held to those two reasons"""
    for name in ('right_80x48_s4_d2_-67_3000000_off', 'slide_48x16_s6_d0_0_30000_off'):
        pics = _pictures(oracle, name)
        assert mdaudit.check_all(pics) is None
        saved = [(p.prev_sksad, p.sksad) for p in pics]
        try:
            for p in pics:
                p.prev_sksad = None
                p.sksad = np.where(p.sksad >= 0, 0, p.sksad)
            assert mdaudit.check_all(pics) is not None, name
        finally:
            for p, (a, b) in zip(pics, saved):
                p.prev_sksad, p.sksad = a, b


def test_mismatch_message_names_the_macroblock(oracle):
    """a second oracle is fed a frame differing in one sample region: held to the first one's source, its bytes leave the
    rule at that macroblock, and the message names it and the step"""
    c = CLIPS['right_80x48_s4_d2_-67_3000000_off']
    frames = [f.copy() for f in c.frames]
    y = frames[3][:c.w * c.h].reshape(c.h, c.w)
    y[16:32, 32:48] = np.roll(y[16:32, 32:48], 5, axis=1)   # macroblock 7 (x 2, y 1)
    other = encaudit.Clip(c.name + ' (one region changed)', c.w, c.h, c.br, frames)
    units = mdaudit.oracle_units(oracle, other)
    assert units[:3] == mdaudit.oracle_units(oracle, c)[:3] and units[3] != mdaudit.oracle_units(oracle, c)[3]
    mm = mdaudit.check_all(mdaudit.chain(c, units)[:4])
    assert mm is not None and mm.mb == 7, str(mm)
    s = str(mm)
    assert 'macroblock 7 (x 2, y 1)' in s and 'frame 3' in s and 'the rules demand' in s and 'the bytes hold' in s
    assert 'steps:' in s and 'try ' in s and 'mvp ' in s and 'code words:' in s and 'mb_type' in s
