"""Cell audit of the encoder's forward residual path, CPU half.

tests/fwdref.py states the forward transform, both DC transforms, the table quantiser and the way levels become the
coded_block_pattern a third time, from DESIGN.md §3.4 and the pinned tables; tests/fwdaudit.py names the cells of the
tables and counts which the content pins. Here the oracle encoder's bytes of fwdaudit.directed_clips() and of the suite's
earlier inputs are held to fwdref, every selectable cell to one of two states (pinned on both sides by the directed clip
that claims it, or listed in NOT_PINNED, and then pinned by none), and every mutation of fwdref to a clip that catches it."""
import functools
import os
import time

import numpy as np

import encaudit
import fwdaudit
import fwdref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle():
    from _oracle import Oracle
    return Oracle(os.path.join(ROOT, 'oracle', 'build', 'libh264_oracle.so'))


@functools.lru_cache(maxsize=None)
def directed():
    """per directed clip (clip, chain()'s frames, cells pinned on both sides, pins, classes); run_clip(decode=True) holds
    the oracle decoder to the encoder's reconstruction on every frame"""
    oracle, out = _oracle(), []
    for c in fwdaudit.directed_clips():
        _, fr = encaudit.run_clip(oracle, c, decode=True)
        assert all(nal for nal, _, _ in fr), c.name
        frames = fwdaudit.chain(c, [nal for nal, _, _ in fr])
        out.append((c, frames) + fwdaudit.count_frames(frames))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def suite():
    """the suite's earlier inputs through the same chain and counter -> (first Mismatch message or None, {cell: first
    input to pin it on both sides}, frames checked, seconds)"""
    oracle, first, bad, n, t0 = _oracle(), {}, None, 0, time.time()
    for c in fwdaudit.suite_inputs(oracle):
        frames = fwdaudit.chain(c, [nal for nal, _, _ in encaudit.run_clip(oracle, c)[1]])
        n += len(frames)
        bad = bad or next((str(mm) for _, mm, _ in frames if mm), None)
        for k in fwdaudit.count_frames(frames)[0]:
            first.setdefault(k, c.name)
    return bad, first, n, time.time() - t0


# ---------------------------------------------------------------- fwdref against hand-worked blocks
def _quant_block(x, qp, intra):
    c = fwdref.forward(np.array(x, np.int64))
    col = np.arange(16).reshape(4, 4) & 7
    return c, fwdref.quant(c, fwdref.FF[qp + 6 * intra][col], fwdref.MF[qp][col])


def test_flat_residual_by_hand():
    """a flat +-255 residual: only c00 = 16 x 255 = 4080. QP 28 inter: MF 1024, FF 11 -> (4091 x 1024) >> 16 = 63;
    QP 12 intra: row 18, MF 6554, FF 3 -> (4083 x 6554) >> 16 = 408 (4083 x 6554 = 26 759 982 = 408 x 65536 + 21 294)"""
    for s in (1, -1):
        c, lv = _quant_block(np.full((4, 4), 255 * s), 28, 0)
        assert c[0, 0] == 4080 * s and np.count_nonzero(c) == 1 and lv[0, 0] == 63 * s and np.count_nonzero(lv) == 1
        assert _quant_block(np.full((4, 4), 255 * s), 12, 1)[1][0, 0] == 408 * s
    # sixteen such blocks: the Hadamard gathers everything in its first cell, (16 x 4080 + 1) >> 1 = 32640; DC quantiser at
    # QP 28 intra: ff = 2 x FF[34][0] = 42, mf = 1024 >> 1 -> (32682 x 512) >> 16 = 255; negative: (-65280 + 1) >> 1 = -32640
    for s in (1, -1):
        had = (fwdref.H4 @ np.full((4, 4), 4080 * s) @ fwdref.H4.T + 1) >> 1
        assert had[0, 0] == 32640 * s and np.count_nonzero(had) == 1
        ff, mf = fwdref.dc_params(fwdref.FF[34][0], fwdref.MF[28][0])
        assert (int(ff), int(mf)) == (42, 512) and fwdref.quant(had, ff, mf)[0, 0] == 255 * s
    assert (np.array([-3, -1, 3]) + 1 >> 1).tolist() == [-1, 0, 2]      # the arithmetic shift on negative odd values


def test_single_impulse_at_each_position_by_hand():
    """an impulse of 64 at (x, y): c[v, u] = 64 x Cf[v][y] x Cf[u][x], the outer product of two columns of Cf, typed here
    column by column; QP 24 inter (MF row 1638 / 1008 / 655, FF row 7 / 11 / 17)"""
    cols = [[1, 2, 1, 1], [1, 1, -1, -2], [1, -1, -1, 2], [1, -2, 1, -1]]     # column k of Cf
    mf = [[1638, 1008, 1638, 1008], [1008, 655, 1008, 655]] * 2
    ff = [[7, 11, 7, 11], [11, 17, 11, 17]] * 2
    for y in range(4):
        for x in range(4):
            imp = np.zeros((4, 4), np.int64)
            imp[y, x] = 64
            c, lv = _quant_block(imp, 24, 0)
            for v in range(4):
                for u in range(4):
                    want = 64 * cols[y][v] * cols[x][u]
                    assert c[v, u] == want, (x, y, u, v)
                    assert lv[v, u] == (1 if want > 0 else -1) * (((abs(want) + ff[v][u]) * mf[v][u]) >> 16), (x, y, u, v)


def test_one_below_every_threshold_by_hand():
    """QP 30 intra (MF 819 / 504 / 328, FF row 36: 27 / 43 / 67): the smallest |c| with level 1 is ceil(65536 / MF) - FF =
    81 - 27 = 54, 131 - 43 = 88, 200 - 67 = 133 for the classes 0 / 2 / 1. A block of coefficients one below gives no level,
    the block at the thresholds gives sixteen levels of 1 with the signs of the coefficients."""
    t = np.array([[54, 88, 54, 88], [88, 133, 88, 133]] * 2, np.int64)
    sign = np.array([[1, -1, 1, -1], [-1, 1, -1, 1]] * 2, np.int64)
    col = np.arange(16).reshape(4, 4) & 7
    q = lambda c: fwdref.quant(c, fwdref.FF[36][col], fwdref.MF[30][col])
    assert not q((t - 1) * sign).any()
    assert (q(t * sign) == sign).all()
    # both DC kinds at QP 30 intra: ff = 54, mf = 409 -> ceil(65536 / 409) - 54 = 161 - 54 = 107
    ff, mf = fwdref.dc_params(fwdref.FF[36][0], fwdref.MF[30][0])
    assert fwdref.quant(np.array([106, -106, 107, -107]), ff, mf).tolist() == [0, 0, 1, -1]


def test_padding_and_chroma_qp_by_hand():
    src = np.arange(18 * 18 * 3 // 2, dtype=np.uint8)
    Y, U, V = fwdref.pad_source(src, 18, 18)
    assert Y.shape == (32, 32) and U.shape == (16, 16)
    assert (Y[3, 18:] == Y[3, 17]).all() and (Y[18:] == Y[17]).all() and (U[9:, 9:] == U[8, 8]).all() and Y[31, 31] == src[18 * 18 - 1]
    assert [fwdref.QPC[q] for q in (29, 30, 34, 39, 42, 51)] == [29, 29, 32, 35, 37, 39]


# ---------------------------------------------------------------- the lists
def test_cells_partition_the_table():
    cells, sel, exc = fwdaudit.all_cells(), fwdaudit.selectable(), fwdaudit.excluded()
    npin = {fwdaudit.cell_of(n) for n in fwdaudit.NOT_PINNED}
    assert len(cells) == len(set(cells)) and set(sel) | set(exc) == set(cells) and not set(sel) & set(exc)
    assert npin <= set(sel) and all(fwdaudit.cell_name(fwdaudit.cell_of(n)) == n for n in fwdaudit.NOT_PINNED)
    assert all(len(why) > 60 for why in exc.values()) and all(len(why) > 60 and tried > 0 for why, tried in fwdaudit.NOT_PINNED.values())
    claimed = [t for c in fwdaudit.directed_clips() for t in c.targets]
    assert len(claimed) == len(set(claimed)), 'a cell is claimed twice'
    assert {fwdaudit.cell_of(t) for t in claimed} == set(sel) - npin, 'claimed and not-pinned cells do not partition the selectable set'
    assert not fwdaudit.not_pinned_ok(), fwdaudit.not_pinned_ok()
    rest = [r for c in fwdaudit.directed_clips() for r in c.classes]
    assert sorted(rest) == sorted(list(fwdaudit.CLASSES) + [m.name for m in fwdref.MUTATIONS]), 'every class and every listed mutation is claimed once'
    for c in fwdaudit.directed_clips():
        assert (c.w, c.h) in fwdaudit.GEOMETRIES and 2 <= len(c.frames) <= 8 and not c.skip and not c.gom, c.name


def test_directed_clips_agree_with_fwdref_and_decode(oracle):
    for c, frames, _, _, _ in directed():
        for _, mm, _ in frames:
            assert mm is None, str(mm)


def test_directed_clips_reach_their_claims(oracle):
    exc = fwdaudit.excluded()
    npin = {fwdaudit.cell_of(n) for n in fwdaudit.NOT_PINNED}
    for c, frames, both, pins, cl in directed():
        missed = [t for t in c.targets if fwdaudit.cell_of(t) not in both]
        assert not missed, f'{c.name} no longer pins {missed} on both sides'
        missed = [k for k in c.classes if k in fwdaudit.CLASSES and not cl[k]]
        assert not missed, f'{c.name} no longer reaches {missed}'
        assert not [fwdaudit.cell_name(k) for k in pins if k in exc], f'{c.name} reads an excluded cell: its derivation is wrong'
        assert not [k for k in fwdaudit.CLASS_EXCLUDED if cl[k]], c.name
        assert not [fwdaudit.cell_name(k) for k in both if k in npin], f'{c.name} pins a cell listed in NOT_PINNED'


def test_every_mutation_is_caught(oracle):
    """the listed mutations on the clip that claims each, the two FF mutations of every pinned cell on the clip that claims
    the cell; the mutations run on the cached frames"""
    runs = {c.name: (c, frames) for c, frames, _, _, _ in directed()}
    by_name = {m.name: m for m in fwdref.MUTATIONS}
    t0, lines, n = time.time(), [], 0
    for c, frames, _, _, _ in directed():
        muts = [by_name[k] for k in c.classes if k in by_name] + fwdaudit.ff_mutations([fwdaudit.cell_of(t) for t in c.targets])
        for m in muts:
            mm = fwdaudit.catches(frames, m)
            assert mm is not None, f'{m.name}: not caught by {c.name}'
            n += 1
            if m.name in by_name:
                lines.append(f'  {m.name}: {str(mm).split(" | code words")[0]}')
    assert n == len(by_name) + 2 * sum(len(c.targets) for c, _ in runs.values())
    print(f'\n{n} mutations caught ({len(by_name)} listed, {n - len(by_name)} of FF cells) in {time.time() - t0:.1f} s; the listed ones:')
    print('\n'.join(lines))


def test_suite_inputs_agree_with_fwdref_and_their_reach(oracle):
    bad, first, n, secs = suite()
    assert bad is None, bad
    exc = fwdaudit.excluded()
    assert not [fwdaudit.cell_name(k) for k in first if k in exc], 'an input of the suite reads an excluded cell'
    print(f'\n{n} frames of the suite\'s earlier inputs agree with fwdref ({secs:.0f} s)')


def test_report(oracle):
    sel, exc = fwdaudit.selectable(), fwdaudit.excluded()
    _, before, _, _ = suite()
    claim = {fwdaudit.cell_of(t): c.name for c in fwdaudit.directed_clips() for t in c.targets}
    print('\nfamily: cells / selectable / excluded / pinned by the suite before / pinned by the directed clips / not pinned')
    for kind in range(4):
        for intra in (0, 1):
            fam = [c for c in fwdaudit.all_cells() if (c[0], c[2]) == (kind, intra)]
            if fam:
                s = [c for c in fam if c in set(sel)]
                print(f'  {fwdref.KINDS[kind]} {"intra" if intra else "inter"}: {len(fam)} / {len(s)} / {len(fam) - len(s)} / {sum(c in before for c in s)} / '
                      f'{sum(c in claim for c in s)} / {sum(fwdaudit.cell_name(c) in fwdaudit.NOT_PINNED for c in s)}')
    print(f'  all: {len(fwdaudit.all_cells())} / {len(sel)} / {len(exc)} / {sum(c in before for c in sel)} / {len(claim)} / {len(fwdaudit.NOT_PINNED)}')
    for c in sel:
        n = fwdaudit.cell_name(c)
        print(f'  {n}: {claim.get(c) or "NOT PINNED: " + fwdaudit.NOT_PINNED[n][0][:40] + "..."}; suite before: {before.get(c, "-")}')
    for c, _, _, _, cl in directed():
        if c.classes:
            print(f'  {c.name}: ' + ', '.join(f'{k} {cl[k]}' for k in c.classes if k in fwdaudit.CLASSES))
    assert set(claim) | {fwdaudit.cell_of(n) for n in fwdaudit.NOT_PINNED} == set(sel)


def test_mismatch_message_names_the_cell(oracle):
    """a source differing in one sample from the one that was coded: the message names macroblock, plane, block, scan index,
    coefficient, QP, table row and column, both levels and the macroblock's code words"""
    c, frames, _, _, _ = next(d for d in directed() if d[0].w == 48 and d[0].h == 48)
    fr = frames[0][0]
    src = c.frames[0].copy()
    src[20 * 48 + 37] ^= 0x80     # luma sample (37, 20): macroblock 5, block 5
    other = fwdref.frame(src, c.w, c.h, fr.parsed, type('R', (), dict(pred=fr.pred, records=_records(fr), skip_mv=fr.skip_mv)), 'changed source')
    mm = fwdref.structure(other) or fwdref.check(other)
    assert mm is not None and mm.mb == 5
    text = str(mm)
    for part in ('macroblock 5 (x 2, y 1)', 'plane Y', 'block 5', 'scan index', 'coefficient', 'QP ', 'table row', 'column', 'level demanded', 'found', 'mb_type'):
        assert part in text, (part, text)
    print('\n' + text[:700] + ' ...')


def _records(fr):
    rec = np.zeros((fr.nmb, 60), np.int64)
    rec[:, 0], rec[:, 1], rec[:, 22:24] = fr.typ, fr.qp, fr.mv
    return rec
