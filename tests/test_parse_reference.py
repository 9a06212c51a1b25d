"""CPU: entropy decoding -- the byte stream, parameter sets, slice header, slice data, macroblock layer, Exp-Golomb and
CAVLC (clauses 7.3, 9.1, 9.2) -- against an independent reference, tests/parseref.py, and an audit of which parse
classes the suite's streams reach.

  * outside pin: OpenH264's encoder VLC tables, cut as bytes out of the reference's prebuilt module into
    tests/golden/openh264_vlc_tables.json (tools/wasm_tables.py), == the oracle's tables == parseref's printed bit strings;
  * parse check: parseref.parse(bytes) == the oracle's h264o_dec_syntax, int for int, on every stream of
    test_recon_reference.STREAMS and on the directed streams below;
  * from-bytes chain: bytes -> parseref -> reconref -> dbkref == the oracle decoder's pictures: the whole decoder restated
    without the oracle. tests/test_gpu_parse_reference.py compares the GPU against this chain;
  * cross-writer check: streams whose residual blocks parseref's writer wrote parse in the oracle as written;
  * sensitivity: two equal-length code words swapped in one of parseref's trees make the parse check fail;
  * audit: every class of parseref.required_classes() is reached by the streams the GPU modules decode, or excluded
    with the clause that rules it out.

`python tests/test_parse_reference.py` prints the audit table of DESIGN.md (class group by hits, per stream family)."""
import copy
import functools
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'openh264-wasm_amd'))

import dbkref  # noqa: E402
import parseref  # noqa: E402
import reconref  # noqa: E402
import test_recon_reference as trr  # noqa: E402
from test_dbk_reference import _gen, _oracle_table, _pcm  # noqa: E402
from test_recon_reference import SO, _check_mblog, _nal_ref_idc  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'openh264_vlc_tables.json')


# ---------------------------------------------------------------------------------------------------------------
# tables: OpenH264's == the oracle's == the printed bit strings


def _word(code, length):
    return format(code, 'b').zfill(length) if length else None


def _golden_words():
    """{table: {row: {value: bit string}}} of the golden file, in the shape of parseref.printed_tables()"""
    g = json.load(open(GOLDEN))['tables']
    ct = g['coeff_token']['values']
    out = {'coeff_token': {cls: {(tc, t1): _word(*ct[c][tc][t1]) for tc in range(17) for t1 in range(4) if ct[c][tc][t1][1]}
                           for c, cls in enumerate(parseref.NC_CLASSES)}}
    for name, key in (('total_zeros', 'total_zeros'), ('total_zeros_dc', 'total_zeros_chroma_dc'), ('run_before', 'run_before')):
        out[name] = {r + 1: {v: _word(*p) for v, p in enumerate(row) if p[1]} for r, row in enumerate(g[key]['values'])}
    return out


def _oracle_words(oracle):
    out = {}
    L, C = _oracle_table(oracle, 'ct_len', 272), _oracle_table(oracle, 'ct_code', 272)
    out['coeff_token'] = {cls: {(tc, t1): _word(C[68 * c + 4 * tc + t1], L[68 * c + 4 * tc + t1]) for tc in range(17) for t1 in range(4)
                                if L[68 * c + 4 * tc + t1]} for c, cls in enumerate(parseref.NC_CLASSES[:4])}
    L, C = _oracle_table(oracle, 'ct_dc_len', 20), _oracle_table(oracle, 'ct_dc_code', 20)
    out['coeff_token']['dc'] = {(tc, t1): _word(C[4 * tc + t1], L[4 * tc + t1]) for tc in range(5) for t1 in range(4) if L[4 * tc + t1]}
    for name, ln, cn, rows, width in (('total_zeros', 'tz_len', 'tz_code', 15, 16), ('total_zeros_dc', 'tz_dc_len', 'tz_dc_code', 3, 4),
                                      ('run_before', 'rb_len', 'rb_code', 7, 15)):
        L, C = _oracle_table(oracle, ln, rows * width), _oracle_table(oracle, cn, rows * width)
        out[name] = {r + 1: {v: _word(C[r * width + v], L[r * width + v]) for v in range(width) if L[r * width + v]} for r in range(rows)}
    return out


def test_vlc_tables_three_way(oracle):
    """Tables 9-5 and 9-7 to 9-10, entry by entry: OpenH264's encoder tables (bytes of the prebuilt module) == the oracle's
    (oracle/h264o_tables.h, which test_recon_reference ties to both kernel copies) == parseref's printed bit strings"""
    gold, orc, typed = _golden_words(), _oracle_words(oracle), parseref.TABLES
    for name in typed:
        assert set(gold[name]) == set(orc[name]) == set(typed[name]), name
        for row in typed[name]:
            assert gold[name][row] == typed[name][row], f'{name} row {row}: OpenH264 != the printed table'
            assert orc[name][row] == typed[name][row], f'{name} row {row}: the oracle != the printed table'
    assert sum(len(w) for w in typed['coeff_token'].values()) == 4 * 62 + 14
    assert sum(len(w) for w in typed['total_zeros'].values()) == 135 and sum(len(w) for w in typed['total_zeros_dc'].values()) == 9
    assert sum(len(w) for w in typed['run_before'].values()) == 42


def test_golden_holds_numbers_only():
    g = json.load(open(GOLDEN))
    for t in g['tables'].values():
        assert set(t) == {'address', 'file_offset', 'type', 'shape', 'meaning', 'values'}
        assert all(isinstance(v, int) and 0 <= v < 256 for v in np.asarray(t['values']).ravel().tolist())
        assert list(np.asarray(t['values']).shape) == t['shape']


def test_ring_size_matches_the_kernel_source():
    src = open(os.path.join(ROOT, 'openh264-wasm_amd', 'csrc', 'dec_parse.inc')).read()
    assert int(re.search(r'constexpr int RING_BYTES = (\d+);', src).group(1)) == parseref.RING_BYTES
    assert 'r.wi - r.wb >= 16' in src and 'r.wi - r.wb >= 40' in src   # vr_slide / vr_reslide: the ('mb_dwords', ...) classes


# ---------------------------------------------------------------------------------------------------------------
# directed streams: the classes the audit found the existing streams to miss, by construction


def _limit(qp):
    return max(1, 2048 // (25 << (qp // 6)))   # streamgen's bound: no dequantised value leaves 16 bits (8.5.12)


class Sweep:
    """SyntaxGen block hook that steers every residual block towards a parse class not yet written: a coeff_token
    (nC class, TotalCoeff, TrailingOnes), a total_zeros entry, or a level at a chosen (suffixLength, level_prefix, sign)
    behind a ramp of levels that raises suffixLength to it. Levels beyond streamgen's bound are written only as the last
    level of a Luma4x4 block at QP 0 with every zero used up before it -- scan position 0, where LevelScale is 160 and
    2528 * 10 stays inside 16 bits (8.5.12), together with the ramp's small levels."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        T = parseref.TABLES
        self.tokens = {cls: set(T['coeff_token'][cls]) for cls in parseref.NC_CLASSES}
        self.zeros = {(mx, tc, tz) for mx in (16, 15) for tc, col in T['total_zeros'].items() for tz in col if tc + tz <= mx}
        self.zeros |= {(4, tc, tz) for tc, col in T['total_zeros_dc'].items() for tz in col}
        self.levels = {(sl, p, s) for sl in range(7) for p in range(16) for s in '+-'}
        self.levels -= {(0, p, '+-'[1 - p % 2]) for p in range(14)}
        self.levels |= {('mag', sl, (3 if sl == 0 else 3 << (sl - 1)) + d) for sl in range(6) for d in (0, 1)}

    def left(self):
        return sum(len(v) for v in self.tokens.values()) + len(self.zeros) + len(self.levels)

    def _pick(self, pool):
        pool = sorted(pool, key=str)
        return pool[int(self.rng.integers(len(pool)))] if pool else None

    def _level_plan(self, goal, t1, long_block):
        """-> (levels in decoding order after the trailing ones, whether the last exceeds the usual bound) or None"""
        rng, sl_goal = self.rng, goal[1] if goal[0] == 'mag' else goal[0]
        cur, seq = (1 if long_block and t1 < 3 else 0), []
        if cur > sl_goal:
            return None
        while cur < sl_goal:
            if cur == 0:
                mag, cur = (2, 1) if sl_goal == 1 else (4, 2)
            else:
                mag, cur = (3 << (cur - 1)) + 1, cur + 1
            seq.append(int(mag * rng.choice([-1, 1])))
        first = not seq and t1 < 3
        if goal[0] == 'mag':
            v = goal[2]
            if first and v < 2:
                return None
        else:
            sl, p, sign = goal
            if sl == 0:
                code = p if p < 14 else (14 + int(rng.integers(16)) if p == 14 else 30 + int(rng.integers(4096)))
            else:
                code = (p << sl) + int(rng.integers(1 << sl)) if p < 15 else (15 << sl) + int(rng.integers(4096))
            if (code % 2 == 0) != (sign == '+'):
                code ^= 1
            if first:
                code += 2
            v = (code + 2) >> 1 if code % 2 == 0 else (-code - 1) >> 1
            if sl == 0 and p < 14 and first and t1 == 0 and abs(v) == 1:
                return None
        if t1 < 3 and not seq and abs(v) == 1:
            return None   # would be a trailing one
        return seq + [int(v)], abs(v)

    def __call__(self, what, maxnum, nc, qp):
        rng = self.rng
        cls = 'dc' if nc < 0 else parseref.NC_CLASSES[0 if nc < 2 else 1 if nc < 4 else 2 if nc < 8 else 3]
        lim = 8 if what in ('i16dc', 'chroma_dc') else _limit(qp)
        tok = self._pick({k for k in self.tokens[cls] if k[0] <= maxnum})
        plan = None
        if self.levels and what in ('luma', 'i16ac', 'chroma_ac') and (tok is None or rng.random() < 0.5):
            goal = self._pick(self.levels)
            t1 = int(rng.integers(0, 4))
            plan = self._level_plan(goal, t1, False)
            if plan is not None:
                big = plan[1] > lim
                if big and not (what == 'luma' and qp == 0 and plan[1] <= 2528):
                    plan = None
                elif t1 + len(plan[0]) > min(maxnum, 10):
                    plan = None
        if plan is not None:
            lv = [int(rng.choice([-1, 1])) for _ in range(t1)] + plan[0]
            if not big:   # small levels may follow: the goal need not be the last level
                lv += [int(rng.choice([-2, 2])) for _ in range(int(rng.integers(0, max(1, min(3, 10 - len(lv))))))]
            tc = len(lv)
            self.levels.discard(goal)
        else:
            tc, t1 = tok if tok is not None else (int(rng.integers(0, maxnum + 1)), 0)
            if tok is None:
                t1 = int(rng.integers(0, min(3, tc) + 1))
            lv = [int(rng.choice([-1, 1])) for _ in range(t1)]
            for i in range(tc - t1):
                m = int(rng.integers(2 if (i == 0 and t1 < 3) else 1, min(lim, 6) + 1)) if lim >= 2 else 1
                lv.append(int(m * rng.choice([-1, 1])))
            if lim < 2 and t1 < min(3, tc):   # only +-1 allowed here: the token's TrailingOnes cannot be below min(3, tc)
                t1 = min(3, tc)
            big = False
        out = np.zeros(maxnum, np.int16)
        if tc == 0:
            self.tokens[cls].discard((0, 0))
            return out
        zgoal = self._pick({k for k in self.zeros if k[0] == maxnum and k[1] == tc and not (big and tc == 1 and k[2])})
        tz = zgoal[2] if zgoal else int(rng.integers(0, maxnum - tc + 1))
        # runs: tz zeros among the coefficients; a big last level takes none (scan position 0)
        runs = [0] * tc
        for _ in range(tz):
            runs[int(rng.integers(0, tc - 1 if big else tc))] += 1
        pos = -1
        for i in range(tc - 1, -1, -1):
            pos += runs[i] + 1
            out[pos] = lv[i]
        # account for what the block holds as the parser will see it
        nz = [int(v) for v in out[::-1] if v]
        seen_t1 = 0
        while seen_t1 < min(3, tc) and abs(nz[seen_t1]) == 1:
            seen_t1 += 1
        self.tokens[cls].discard((tc, seen_t1))
        self.zeros.discard((maxnum, tc, tz))
        return out


def _d_sweep(seed, npics=10):
    """80x48 at QP 0 (mb_qp_delta always 0): Sweep-steered blocks, residual written by parseref's writer"""
    def build(oracle):
        g = _gen(5, 3, seed, init_qp=0)
        g.block_hook, g.dq_hook, g.writer = Sweep(seed), (lambda qp: 0), parseref.write_residual_block
        g.mblogs = []
        lay = [dict(first=0), dict(first=8)]
        units = [g.idr(slices=lay, mix={'i4': 4, 'i16': 3})]
        g.mblogs.append(g.mblog)
        for k in range(npics):
            units.append(g.p(slices=lay if k % 2 else None, mix={'p16': 3, 'p8x8': 1, 'i4': 3, 'i16': 3, 'skip': 1}, max_mvd=8))
            g.mblogs.append(g.mblog)
        build.gen = g
        return units, (80, 48)
    return build


def _d_types(oracle):
    """48x48: every mb_type of I and P slices (P_8x8ref0 included), every sub_mb_type, all 48 codeNums of
    coded_block_pattern in both columns, mb_qp_delta -26, +25 and a wrap; I_PCM behind 0..7 alignment bits falls out of
    the mix; I_PCM samples 0, 0, 1 (an emulation prevention byte inside pcm_sample) and a last macroblock whose final
    samples 0, 0, 1 put one into the last three bytes of the NAL"""
    g = _gen(3, 3, 71, init_qp=26)
    g.writer = parseref.write_residual_block
    dqs = iter([-26, 25, 25, -26, -26, 0])
    g.dq_hook = lambda qp: next(dqs, None)
    rng = np.random.default_rng(71)
    i16 = [dict(kind='i16', cbp=(15 if t >= 12 else 0) | ((t // 4) % 3) << 4) for t in range(24)]
    units, codes = [], list(range(48))
    pcm = _pcm(rng, 100, 20)
    pcm[5:8] = (0, 0, 1)
    tail = _pcm(rng, 100, 20)
    tail[381:384] = (0, 0, 1)
    units.append(g.idr(script={a: dict(kind='i4', cbp=reconref.CBP_TABLE[a][0]) for a in range(9)}))
    for k in range(1, 6):
        s = {a: dict(kind='i4', cbp=reconref.CBP_TABLE[9 * k + a][0]) for a in range(9) if 9 * k + a < 48}
        if k == 5:
            s[4], s[8] = dict(kind='pcm', samples=pcm), dict(kind='pcm', samples=tail)
        units.append(g.p(script=s, slices=[dict(first=0, intra=True)]))
    for k in range(6):
        kinds = ['p16', 'p16x8', 'p8x16', 'p8x8', 'p8x8ref0', 'p8x8', 'p16', 'p8x8ref0', 'p16x8']
        s = {a: dict(kind=kinds[(a + k) % 9], cbp=reconref.CBP_TABLE[(9 * k + a) % 48][1]) for a in range(9)}
        if k == 5:
            s[8] = dict(kind='pcm', samples=tail)
        units.append(g.p(script=s, max_mvd=6))
    for k in range(3):   # the 24 Intra16x16 types in I slices and, with pictures of P slices, in P slices
        units.append(g.p(script={a: i16[(9 * k + a) % 24] for a in range(9)}, slices=[dict(first=0, intra=True)]))
        units.append(g.p(script={a: i16[(9 * k + a) % 24] for a in range(9)}))
    return units, (48, 48)


def _d_ring(oracle):
    """176x144, one slice of I_PCM and QP 4 macroblocks: its RBSP exceeds two LDS rings, macroblocks exceed 16 and 40 dwords"""
    g = _gen(11, 9, 72, init_qp=4)
    g.dq_hook = lambda qp: 0
    rng = np.random.default_rng(72)
    script = {a: dict(kind='pcm', samples=_pcm(rng, 128, 100)) for a in range(99) if a % 8 != 3}
    g.tc_choice = [8, 12, 16]
    units = [g.idr(script=script, mix={'i4': 1})]
    units += [g.p(script={a: s for a, s in script.items() if a % 3 != k}, mix={'i4': 1, 'p16': 1, 'skip': 1}) for k in (0, 1)]
    return units, (176, 144)


PARSE_DIRECTED = {
    'sweep_a_80x48': _d_sweep(73),
    'sweep_b_80x48': _d_sweep(74),
    'types_48x48': _d_types,
    'ring_176x144': _d_ring,
}
CROSS_WRITER = ('sweep_a_80x48', 'sweep_b_80x48')
MULTISLICE = 'sweep_a_80x48'
RING = 'ring_176x144'


# ---------------------------------------------------------------------------------------------------------------
# analysis: every stream parsed once


class ParseAnalysis:
    def __init__(self, name):
        from _oracle import Oracle
        oracle = Oracle(SO)
        self.directed = name in PARSE_DIRECTED
        if self.directed:
            self.units, self.size = PARSE_DIRECTED[name](oracle)
        else:
            a = trr.analysed(name)
            self.units, self.size = a.units, a.size
        d = oracle.decoder()
        d.set_capture(True)
        state = parseref.State()
        self.counts, self.parse_bad, self.chain_bad = parseref.Counter(), None, None
        self.parsed, self.chain, self.oracle_syntax = [], [], []
        prev = None
        for k, u in enumerate(self.units):
            rc, pic, w, h = d.decode(u)
            assert rc == 1, f'{name} unit {k}: oracle decode rc {rc}'
            syn = d.syntax()
            self.oracle_syntax.append(syn)
            p = parseref.parse(u, state)
            self.parsed.append(p)
            self.counts.update(p.counts)
            cw, ch = d.coded_size()
            if self.parse_bad is None:
                self.parse_bad = first_syntax_difference(p, syn, (cw // 16, ch // 16), (w, h), k)
            if self.directed:   # the chain from bytes alone; for the other streams Analysis holds it (equal syntax, equal chain)
                res = reconref.reconstruct(p.syntax, p.geometry, prev)
                out = dbkref.deblock(res.planes, res.records)
                self.chain.append(out.i420(w, h))
                if self.chain_bad is None and not np.array_equal(self.chain[-1], pic):
                    self.chain_bad = f'picture {k}: ' + (reconref.first_difference(res, d.prefilter(), cw, ch) or 'differs after the loop filter')
                if _nal_ref_idc(u):
                    prev = out.planes
                assert p.ref_idc == (1 if _nal_ref_idc(u) else 0)


def first_syntax_difference(p, syn, geometry, size, k):
    if p.geometry != geometry or p.size != size:
        return f'picture {k}: geometry {p.geometry} {p.size}, oracle {geometry} {size}'
    ne = np.argwhere(p.syntax != syn)
    if not len(ne):
        return None
    a, c = (int(v) for v in ne[0])
    return (f'picture {k} MB {a} syntax int {c}: reference {int(p.syntax[a, c])}, oracle {int(syn[a, c])}; ' + ' | '.join(p.explain(a)))[:3000]


@functools.lru_cache(maxsize=None)
def parsed(name):
    return ParseAnalysis(name)


ALL = list(trr.STREAMS) + list(PARSE_DIRECTED)


@pytest.mark.parametrize('name', ALL)
def test_parse_equals_oracle(oracle, name):
    """parseref.parse(bytes) == h264o_dec_syntax int for int, the geometry and the cropped size"""
    a = parsed(name)
    assert a.parse_bad is None, f'{name}: {a.parse_bad}'


@pytest.mark.parametrize('name', ALL)
def test_from_bytes_chain_equals_oracle(oracle, name):
    """bytes -> parseref -> reconref -> dbkref == the oracle decoder's pictures. For the streams of test_recon_reference the
    chain over the same syntax is Analysis's (computed once per session): equal syntax, equal chain"""
    a = parsed(name)
    assert a.parse_bad is None, f'{name}: {a.parse_bad}'
    if a.directed:
        assert a.chain_bad is None, f'{name}: {a.chain_bad}'
    else:
        assert trr.analysed(name).chain_bad is None, f'{name}: {trr.analysed(name).chain_bad}'


@pytest.mark.parametrize('name', CROSS_WRITER)
def test_cross_writer(oracle, name):
    """residual blocks written by parseref.write_residual_block parse in the oracle as written"""
    a = parsed(name)
    logs = PARSE_DIRECTED[name].gen.mblogs
    assert len(logs) == len(a.units)
    for k, (syn, log) in enumerate(zip(a.oracle_syntax, logs)):
        _check_mblog(syn, log, f'{name} picture {k}')


def test_writers_agree(oracle):
    """parseref's writer == the oracle's writer, bit for bit, on blocks of every kind"""
    import ctypes
    oracle.L.h264o_cavlc_bits.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    sw, bits = Sweep(5), np.zeros(1024, np.uint8)
    for k in range(3000):
        what, mx = [('luma', 16), ('i16ac', 15), ('chroma_dc', 4), ('i16dc', 16)][k % 4]
        nc = -1 if mx == 4 else int(sw.rng.integers(0, 17))
        coef = np.ascontiguousarray(sw(what, mx, nc, 0), np.int16)
        n = oracle.L.h264o_cavlc_bits(coef.ctypes.data, mx, nc, bits.ctypes.data, bits.size)
        assert ''.join(map(str, bits[:n])) == parseref.write_residual_block(coef, nc, mx), (what, nc, coef.tolist())


def test_existing_streams_unchanged(oracle):
    """SyntaxGen's new hooks leave the default streams byte-identical"""
    import hashlib
    import test_dbk_reference as tdr
    from test_syntax_streams import CASES, MULTI, _multi_units, _stream
    units, _ = _stream(oracle, CASES[1])
    assert hashlib.sha256(b''.join(units)).hexdigest() == tdr.SYNTAX_CASE1_SHA256
    _, mu = _multi_units(21, MULTI[1])
    assert hashlib.sha256(b''.join(u for u, _ in mu)).hexdigest() == tdr.MULTI1_SHA256


# ---------------------------------------------------------------------------------------------------------------
# sensitivity

# per table: (row, two values whose code words have equal length) among entries the audit reports as reached
SWAPS = [('coeff_token', '0-1', (2, 0), (3, 1)), ('coeff_token', 'dc', (1, 0), (2, 1)), ('total_zeros', 2, 0, 1),
         ('total_zeros_dc', 1, 2, 3), ('run_before', 3, 0, 1)]
SENSITIVITY_STREAMS = ('syntax_5x3_crop20_cqp-12', 'recon_qp_80x48')


@pytest.mark.parametrize('swap', SWAPS, ids=[f'{s[0]}_{s[1]}' for s in SWAPS])
def test_sensitivity(oracle, swap):
    name, row, a, b = swap
    t = copy.deepcopy(parseref.TABLES)
    wa, wb = t[name][row][a], t[name][row][b]
    assert len(wa) == len(wb) and wa != wb
    t[name][row][a], t[name][row][b] = wb, wa
    trees = parseref.build_trees(t)
    failed = False
    for s in SENSITIVITY_STREAMS:
        an = parsed(s)
        assert an.parse_bad is None
        state = parseref.State()
        for u, syn in zip(an.units, an.oracle_syntax):
            try:
                p = parseref.parse(u, state, trees=trees)
            except parseref.ParseError:
                failed = True
                break
            if not np.array_equal(p.syntax, syn):
                failed = True
                break
    assert failed, f'{name} row {row}: swapping {a} and {b} went unnoticed'


# ---------------------------------------------------------------------------------------------------------------
# coverage

_SIGN = ('9.2.2.1: at suffixLength 0 a level_prefix below 14 has no level_suffix, levelCode is level_prefix, and the sign is its '
         'parity (even: positive)')
_ROOM = ('7.3.5.3.2 / 9.2.3: TotalCoeff + total_zeros cannot exceed maxNumCoeff; a block of 15 coefficients (Intra16x16ACLevel, '
         'ChromaACLevel) has no room for this entry')
EXCLUDED = {('level', 0, p, '+-'[1 - p % 2]): _SIGN for p in range(14)}
EXCLUDED.update({('total_zeros', 15, tc, tz): _ROOM for tc, col in parseref.TABLES['total_zeros'].items() for tz in col if tc + tz > 15})
EXCLUDED[('total_zeros', 15, 15, 0)] = ('7.3.5.3.2: total_zeros is read only when TotalCoeff < maxNumCoeff; a block of 15 coefficients '
                                       'with TotalCoeff 15 holds none (the class total_zeros_absent 15)')

GPU_FAMILIES = ('CASES', 'MULTI', 'LONG', 'DIRECTED', 'RECON', 'PARSE')   # what the GPU decoder modules decode


def family_of(name):
    return 'PARSE' if name in PARSE_DIRECTED else trr.STREAMS[name][0]


def family_counts(families):
    total = parseref.Counter()
    for name in ALL:
        if family_of(name) in families:
            total.update(parsed(name).counts)
    return total


def test_every_parse_class_is_reached(oracle):
    hit = family_counts(GPU_FAMILIES)
    missing = sorted((k for k in parseref.required_classes() if k not in EXCLUDED and hit[k] == 0), key=str)
    assert not missing, f'{len(missing)} classes never reached: {missing}'
    assert all(hit[k] == 0 for k in EXCLUDED), 'an excluded class occurred'
    assert set(EXCLUDED) <= parseref.required_classes()


def audit_table():
    fams = ['CASES', 'MULTI', 'LONG', 'encoder', 'DIRECTED', 'RECON', 'PARSE']
    per = {f: family_counts((f,)) for f in fams}
    req = parseref.required_classes()
    groups = sorted({k[0] for k in req})
    rows = ['| class group | classes | excluded | ' + ' | '.join(f'{f} hits (classes)' for f in fams) + ' |', '|---|---:|---:|' + '---:|' * len(fams)]
    for g in groups:
        ks = [k for k in req if k[0] == g]
        cells = [f'{sum(per[f][k] for k in ks)} ({sum(1 for k in ks if per[f][k])})' for f in fams]
        rows.append(f'| `{g}` | {len(ks)} | {sum(1 for k in ks if k in EXCLUDED)} | ' + ' | '.join(cells) + ' |')
    old = family_counts(('CASES', 'MULTI', 'LONG', 'DIRECTED', 'RECON'))
    missed = sorted((k for k in req if k not in EXCLUDED and old[k] == 0), key=str)
    return '\n'.join(rows) + f'\n\nmissed by the existing streams ({len(missed)}):\n' + '\n'.join(str(k) for k in missed)


if __name__ == '__main__':
    print(audit_table())
