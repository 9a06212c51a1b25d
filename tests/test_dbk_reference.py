"""CPU: the loop filter against an independent reference of clause 8.7 (tests/dbkref.py), and an audit of which of
the filter's branches the suite's streams reach.

The oracle's filter (oracle/h264o_common.c) and the product's (csrc/deblock.inc) are two restatements by one hand, so
"GPU picture == oracle picture" cannot see a shared misreading. Here the oracle decoder hands over what its filter
consumes -- the picture before the filter and every macroblock's record (h264o_dec_set_capture / _prefilter /
_records) -- dbkref filters it by the standard's text, and the result must be the oracle's output picture byte for
byte. dbkref also counts the branch classes of 8.7 every line takes; the coverage test asserts that the syntax
streams, the multi-slice streams and the DIRECTED streams below together reach every class (dbkref.required_classes),
so a wrong variant of the branch-free filt_reg cannot hide in a branch no stream selects. tests/test_gpu_dbk_reference.py
runs the same streams through the GPU decoder and the encoder's reconstruction.

`python tests/test_dbk_reference.py` prints the audit table of DESIGN.md (class by hits, per stream family)."""
import functools
import hashlib
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, 'oracle', 'build', 'libh264_oracle.so')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'openh264-wasm_amd'))

import dbkref  # noqa: E402
from test_syntax_streams import CASES, MULTI, _multi_units, _stream  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------
# tables


def _oracle_table(oracle, name, n):
    import ctypes
    out = (ctypes.c_double * n)()
    assert oracle.L.h264o_table(name.encode(), out) == n
    return [int(v) for v in out]


def test_tables_match_the_oracle(oracle):
    """Tables 8-16 / 8-17 / 8-15 as typed in dbkref.py == the oracle's copies (oracle/h264o_tables.h)"""
    assert _oracle_table(oracle, 'dbk_alpha', 52) == dbkref.ALPHA
    assert _oracle_table(oracle, 'dbk_beta', 52) == dbkref.BETA
    tc0 = _oracle_table(oracle, 'dbk_tc0', 156)
    for b in (1, 2, 3):
        assert tc0[b - 1::3] == dbkref.TC0[b], f'tC0 row of bS {b}'
    assert _oracle_table(oracle, 'chroma_qp', 52) == dbkref.QPC


def _initialiser(src, name):
    m = re.search(name + r'(?:\[\d+\])+\s*=\s*\{(.*?)\};', src, re.S)
    assert m, name
    return [int(v) for v in re.findall(r'\d+', m.group(1))]


def test_tables_match_the_kernel_source():
    """the same tables == the initialisers of DBK_ALPHA / DBK_BETA / DBK_TC0 in csrc/deblock.inc, by value"""
    src = open(os.path.join(ROOT, 'openh264-wasm_amd', 'csrc', 'deblock.inc')).read()
    assert _initialiser(src, 'DBK_ALPHA') == dbkref.ALPHA
    assert _initialiser(src, 'DBK_BETA') == dbkref.BETA
    tc0 = _initialiser(src, 'DBK_TC0')
    assert len(tc0) == 156
    for b in (1, 2, 3):
        assert tc0[b - 1::3] == dbkref.TC0[b], f'tC0 row of bS {b}'


def test_table_monotony():
    """what Tables 8-16 / 8-17 guarantee by construction: thresholds never fall with the index, t'C0 never falls with bS"""
    for t in (dbkref.ALPHA, dbkref.BETA, dbkref.TC0[1], dbkref.TC0[2], dbkref.TC0[3]):
        assert all(a <= b for a, b in zip(t, t[1:]))
    assert all(a <= b <= c for a, b, c in zip(dbkref.TC0[1], dbkref.TC0[2], dbkref.TC0[3]))


# ---------------------------------------------------------------------------------------------------------------
# streams: name -> (family, builder(oracle) -> (access units, (w, h)))


def _syntax(case):
    def build(oracle):
        units, _ = _stream(oracle, case)
        return units, (case[0] * 16 - 2 * case[2], case[1] * 16 - 2 * case[3])
    return build


def _multi(k):
    def build(oracle):
        _, units = _multi_units(20 + k, MULTI[k])
        return [u for u, _ in units], (176, 144)
    return build


def _committed(oracle):
    data = open(os.path.join(ROOT, 'tests', 'golden', 'synth3_qcif_3f.h264'), 'rb').read()
    starts = [k for k in range(len(data) - 3) if data[k:k + 4] == b'\x00\x00\x00\x01']
    cuts = [0] + [k for k in starts if data[k + 4] & 31 == 1] + [len(data)]
    return [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])], (176, 144)


def _oracle_encoded(w, h, sid=0, br=300000, nf=4):
    def build(oracle):
        from h264mi.synth import SyntheticStream
        g, oe = SyntheticStream(sid, w, h), oracle.encoder(w, h, br)
        oe.set_frame_skip(False)
        return [oe.encode(np.ascontiguousarray(g.frame(t))) for t in range(nf)], (w, h)
    return build



# ---- directed streams: the classes the audit found the random streams not to reach (pictures one macroblock wide or
# high, an idc 1 macroblock modified across a vertical edge), and streams that reach by construction, and often,
# what the random streams reach a handful of times (Clip1 saturating, the bS 4 threshold |p0 - q0| < (alpha >> 2) + 2
# at its last true / first false value, the index clips). name -> builder(oracle) -> (access units, (w, h)).


def _gen(mbw, mbh, seed, **kw):
    from streamgen import SyntaxGen
    return SyntaxGen(SO, mbw, mbh, seed, **kw)


def _d_one_mb(oracle):
    """16x16: one macroblock -- no macroblock edge at all, the row is first and last, no hand-over from above"""
    g = _gen(1, 1, 41, init_qp=34)
    return [g.idr(), g.p(), g.p(dbk=(0, 2, 2)), g.p(qp_delta=8)], (16, 16)


def _strip(mbw, mbh, seed):
    def build(oracle):
        g = _gen(mbw, mbh, seed, init_qp=36, cqp=-5)
        a = [dict(first=0), dict(first=1, dbk=(1, 0, 0)), dict(first=2, dbk=(0, 3, 3))]   # idc 1 between idc 0 neighbours
        b = [dict(first=0), dict(first=1, dbk=(2, 0, 0)), dict(first=2, dbk=(2, -2, 2))]  # idc 2: slice edges unfiltered
        return [g.idr(slices=a), g.p(slices=a), g.p(), g.p(slices=b), g.p(slices=a, qp_delta=6)], (mbw * 16, mbh * 16)
    return build


def _d_slices(oracle):
    """80x48 (5 x 3 macroblocks), five slices per picture starting mid-row: idc 2, 1, 0 with offsets, an I slice, idc 0"""
    g = _gen(5, 3, 44, init_qp=32)
    lay = [dict(first=0, dbk=(2, 1, -1)), dict(first=3, dbk=(1, 0, 0)), dict(first=7, qp_delta=4, dbk=(0, -2, 2)),
           dict(first=11, dbk=(2, 0, 0), intra=True), dict(first=14)]
    return [g.idr(slices=lay)] + [g.p(slices=lay) for _ in range(3)], (80, 48)


def _pcm(rng, base_y, amp, base_c=None):
    """384 pcm_sample values: luma base_y and chroma base_c (default base_y), each +- amp of noise, inside 0..255"""
    base = np.concatenate([np.full(256, base_y), np.full(128, base_y if base_c is None else base_c)])
    return np.clip(base + rng.integers(-amp, amp + 1, 384), 0, 255)


def _d_saturation(oracle):
    """176x144: a checkerboard of I_PCM macroblocks near white (255 - noise) and near black, random I_NxN / I_16x16
    between them predicted from those samples (QP 40: their internal bS 3 edges filter), then P pictures of the same
    content -- Clip1 of 8-476 / 8-477 saturates at 0 and at 255 on many lines"""
    g = _gen(11, 9, 45, init_qp=40)
    rng = np.random.default_rng(45)
    script = {y * 11 + x: dict(kind='pcm', samples=_pcm(rng, 255 if (x // 2 + y // 2) & 1 else 0, 12))
              for y in range(9) for x in range(11) if (x + y) % 2 == 0}
    units = [g.idr(mix={'i4': 1, 'i16': 1}, script=script)]
    units += [g.p(mix={'p16': 3, 'p8x8': 1, 'skip': 1, 'i4': 1}, max_mvd=6, dbk=(0, k, k)) for k in (0, 3)]
    return units, (176, 144)


def _d_steps(oracle):
    """176x144: a checkerboard of I_PCM macroblocks (a base level and a noise amplitude each) and I_16x16 macroblocks
    without coefficients that copy the I_PCM macroblock on their left (horizontal prediction; in column 0: the one
    above, vertical prediction). Every macroblock edge is bS 4 between chosen levels at qPav (0 + 51 + 1) >> 1 = 26:
    steps on both sides of alpha, beta and (alpha >> 2) + 2, flat and noisy sides (p / q strong and weak in every
    combination). FilterOffsetA / B +12 and -6 move the indices. Then P pictures of short vectors without residual:
    bS 0 / 1 by a vector difference of exactly 3 / 4 on the filtered content."""
    g = _gen(11, 9, 46, init_qp=51)
    rng = np.random.default_rng(46)

    def script():
        s = {}
        for y in range(9):
            for x in range(11):
                if (x + y) % 2 == 0:
                    s[y * 11 + x] = dict(kind='pcm', samples=_pcm(rng, 120 + int(rng.integers(-12, 13)), int(rng.choice([0, 0, 1, 3, 7])),
                                                                  128 + int(rng.integers(-6, 7))))
                else:
                    s[y * 11 + x] = dict(kind='i16', mode=1 if x > 0 else 0, dq=0)
        return s
    units = [g.idr(script=script()), g.p(script=script(), dbk=(0, 6, 6)), g.p(script=script(), dbk=(0, -3, 3))]
    units += [g.p(mix={'p16': 3, 'skip': 1}, max_mvd=3, cbp_fixed=0, qp_delta=-17) for _ in range(2)]
    return units, (176, 144)


def _index_clips(seed, iqp, cqp, off):
    """80x48: QPY near 51 with offsets +12, or QPY near 0 with offsets -12 (indexA / indexB clipped at that end, luma
    and chroma), chroma_qp_index_offset 12 / -12 clipped by 8-313's Clip3"""
    def build(oracle):
        g = _gen(5, 3, seed, init_qp=iqp, cqp=cqp)
        return [g.idr(dbk=(0, off, off)), g.p(dbk=(0, off, off)), g.p(dbk=(0, off, -off))], (80, 48)
    return build


DIRECTED = {
    'one_mb_16x16': _d_one_mb,
    'column_16x48': _strip(1, 3, 42),
    'row_48x16': _strip(3, 1, 43),
    'slices_80x48': _d_slices,
    'index_high_80x48': _index_clips(47, 49, 12, 6),
    'index_low_80x48': _index_clips(48, 3, -12, -6),
    'saturation_176x144': _d_saturation,
    'steps_176x144': _d_steps,
}
MULTISLICE_DIRECTED = 'slices_80x48'   # the directed stream the GPU test runs with several slice waves

STREAMS = {}
for c in CASES:
    STREAMS[f'syntax_{c[0]}x{c[1]}_crop{c[2]}{c[3]}_cqp{c[4]}'] = ('CASES', _syntax(c))
for k in range(len(MULTI)):
    STREAMS[f'multi_{k}'] = ('MULTI', _multi(k))
STREAMS['committed_qcif'] = ('encoder', _committed)
# the oracle encoder codes one slice per picture (it has no slice-count setting); streams of three slices come from
# the GPU encoder and are checked in tests/test_gpu_dbk_reference.py
STREAMS['oracle_enc_80x48'] = ('encoder', _oracle_encoded(80, 48, br=100000))
STREAMS['oracle_enc_176x144'] = ('encoder', _oracle_encoded(176, 144))
for name, b in DIRECTED.items():
    STREAMS[f'directed_{name}'] = ('DIRECTED', b)


def reference_pictures(oracle, units, explain=False):
    """decode units with the oracle, the capture on -> per picture (dbkref Result, the oracle's cropped picture, w, h)"""
    d = oracle.decoder()
    d.set_capture(True)
    out = []
    for k, u in enumerate(units):
        rc, pic, w, h = d.decode(u)
        assert rc == 1, f'unit {k}: oracle decode rc {rc}'
        out.append((dbkref.deblock(d.prefilter(), d.records(), explain=explain), pic, w, h))
    return out


def explain_difference(oracle, units, k, got_planes, w, h):
    """the assertion message for picture k of units: where got_planes leave the reference, and the reference's classes there"""
    res = reference_pictures(oracle, units[:k + 1], explain=True)[k][0]
    return dbkref.first_difference(res, got_planes, w, h)


def planes_of(i420, w, h):
    a = np.frombuffer(i420, np.uint8) if isinstance(i420, (bytes, bytearray)) else np.asarray(i420)
    n = w * h
    return a[:n].reshape(h, w), a[n:n + n // 4].reshape(h // 2, w // 2), a[n + n // 4:n + n // 2].reshape(h // 2, w // 2)


@functools.lru_cache(maxsize=None)
def _analysed(name):
    """(counts, first mismatch message or None, units) of one stream -- computed once, shared by the parity, coverage and
    audit tests"""
    from _oracle import Oracle
    oracle = Oracle(SO)
    units, _ = STREAMS[name][1](oracle)
    counts, bad = dbkref.Counter(), None
    for k, (res, pic, w, h) in enumerate(reference_pictures(oracle, units)):
        counts.update(res.counts)
        if bad is None and not np.array_equal(res.i420(w, h), pic):
            bad = f'picture {k}: ' + explain_difference(oracle, units, k, planes_of(pic, w, h), w, h)
    return counts, bad


@pytest.mark.parametrize('name', list(STREAMS))
def test_reference_equals_oracle(oracle, name):
    """dbkref(the oracle's picture before its filter, the oracle's records) == the oracle's output picture"""
    _, bad = _analysed(name)
    assert bad is None, f'{name}: oracle picture != clause 8.7 reference: {bad}'


def test_existing_streams_unchanged(oracle):
    """SyntaxGen's new hooks leave the bits of the existing seeds alone (the GPU syntax tests decode these streams)"""
    units, _ = _stream(oracle, CASES[1])
    assert hashlib.sha256(b''.join(units)).hexdigest() == SYNTAX_CASE1_SHA256
    _, mu = _multi_units(21, MULTI[1])
    assert hashlib.sha256(b''.join(u for u, _ in mu)).hexdigest() == MULTI1_SHA256


SYNTAX_CASE1_SHA256 = '3234ab9158b4339b5eb779fc5efcd370184ec09de96653d57cf245f0f3b00461'
MULTI1_SHA256 = '201c0c5cde9ee4e9e87b7d2011b6e448f82793bf85853f3e803f8ca20a9af967'

# Classes of dbkref's list that cannot occur in a frame-coded Baseline picture, with the clause that excludes them.
# (dbkref does not even form 'mbedge_bs3' / 'inner_bs4': 8.7.2.1 gives bS 4 to a macroblock edge with an intra side
# and bS 3 to such an edge inside a macroblock when mixedModeEdgeFlag is 0 and the picture is a frame.) Nothing else.
_QPC_MAX = ('chroma: qPav <= 39, the largest QPC of Table 8-15 (8.7.2.2, 8-459), and FilterOffsetA / B <= 12 (7.4.3: '
            'slice_alpha_c0_offset_div2 / slice_beta_offset_div2 <= 6), so qPav + offset <= 51 is never clipped (8-460, 8-461)')
EXCLUDED = {('chroma', d, c): _QPC_MAX for d in 'vh' for c in ('indexA_clip51', 'indexB_clip51')}


def family_counts(families):
    total = dbkref.Counter()
    for name, (fam, _) in STREAMS.items():
        if fam in families:
            total.update(_analysed(name)[0])
    return total


def test_every_branch_class_is_reached(oracle):
    """every class of clause 8.7 that dbkref counts, per plane and direction, is reached by CASES + MULTI + DIRECTED --
    the streams tests/test_gpu_syntax.py, test_gpu_multislice.py and test_gpu_dbk_reference.py put through the GPU"""
    hit = family_counts(('CASES', 'MULTI', 'DIRECTED'))
    missing = sorted(k for k in dbkref.required_classes() if k not in EXCLUDED and hit[k] == 0)
    assert not missing, f'{len(missing)} classes never reached: {missing}'
    assert all(hit[k] == 0 for k in EXCLUDED), 'an excluded class occurred'


def audit_table():
    fams = ['CASES', 'MULTI', 'encoder', 'DIRECTED']
    per = {f: family_counts((f,)) for f in fams}
    order = {c: i for i, c in enumerate(dbkref.CLASSES_BOTH + dbkref.CLASSES_V + dbkref.CLASSES_H + dbkref.CLASSES_LUMA + dbkref.CLASSES_CHROMA)}
    rows = ['| plane | dir | class | ' + ' | '.join(fams) + ' |', '|---|---|---|' + '---:|' * len(fams)]
    for key in sorted(dbkref.required_classes(), key=lambda k: (k[0] != 'luma', order[k[2]], k[1])):
        rows.append(f'| {key[0]} | {key[1]} | `{key[2]}` | ' + ' | '.join(str(per[f][key]) for f in fams) + ' |')
    return '\n'.join(rows)


if __name__ == '__main__':
    print(audit_table())
