"""An independent reference of the H.264 parse -- the byte stream (Annex B, 7.3.1), parameter sets (7.3.2.1, 7.3.2.2),
slice_header (7.3.3), slice_data (7.3.4), the macroblock layer (7.3.5), Exp-Golomb codes (9.1) and CAVLC (9.2) -- for
the Baseline subset both decoders accept: CAVLC, frame macroblocks, one slice group, one active reference, no weighted
or constrained intra prediction. The rest raises ParseError, as the decoders reject it. TEST INFRASTRUCTURE, written
from the standard's clauses and tables, not from the oracle's h264o_dec.c / cavlc_read_block nor from the product's
dec_parse.inc / cavlc_blk.inc.

It is also built differently from both, so that a slip of transcription cannot carry over:
  * Tables 9-5 and 9-7 to 9-10 are typed as the bit strings the standard prints, and a code word is decoded by walking
    a prefix tree built from those strings, bit by bit. There are no (length, code) arrays and nothing is looked up by
    peeked bits;
  * nC (9.2.1) is not computed per case. The picture carries, per 4x4 block of each colour plane, the TotalCoeff
    "known" so far and the slice that set it; a neighbouring block is available when it lies in the picture and its
    entry was set by the current slice. A macroblock writes its entries when it opens (0 for P_Skip, for a clear
    coded_block_pattern bit and for Intra16x16 without AC, 16 for I_PCM) and overwrites them block by block, so the
    rules of 9.2.1 for those neighbours, and for a neighbour in another slice, fall out of the map.

parse(access_unit_bytes, state) -> Parsed: the syntax elements of every macroblock in the layout of h264o_dec_syntax
(oracle/h264o_api.h: 872 int32 per macroblock), the geometry, a Counter of parse classes and explain(mb): the code
words of that macroblock with their bit positions in the slice's RBSP. reconref.reconstruct and dbkref.deblock run
behind it unchanged. write_residual_block(levels, nC, maxNumCoeff) is the writer from the same printed tables.
"""
from collections import Counter

import numpy as np

from reconref import BLK_XY, CBP_TABLE   # 6.4.3 block positions and Table 9-4, typed there from the standard

SYN_INTS = 872
RING_BYTES = 16384   # csrc/dec_parse.inc RING_BYTES (tests/test_parse_reference.py reads the source and compares)

# ---------------------------------------------------------------------------------------------------------------
# Table 9-5: coeff_token. One line per (TrailingOnes, TotalCoeff); columns 0 <= nC < 2, 2 <= nC < 4, 4 <= nC < 8, 8 <= nC,
# nC == -1 ('-': no such code)
_TABLE_9_5 = """
0 0   1                   11                1111          000011  01
0 1   000101              001011            001111        000000  000111
1 1   01                  10                1110          000001  1
0 2   00000111            000111            001011        000100  000100
1 2   000100              00111             01111         000101  000110
2 2   001                 011               1101          000110  001
0 3   000000111           0000111           001000        001000  000011
1 3   00000110            001010            01100         001001  0000011
2 3   0000101             001001            01110         001010  0000010
3 3   00011               0101              1100          001011  000101
0 4   0000000111          00000111          0001111       001100  000010
1 4   000000110           000110            01010         001101  00000011
2 4   00000101            000101            01011         001110  00000010
3 4   000011              0100              1011          001111  0000000
0 5   00000000111         00000100          0001011       010000  -
1 5   0000000110          0000110           01000         010001  -
2 5   000000101           0000101           01001         010010  -
3 5   0000100             00110             1010          010011  -
0 6   0000000001111       000000111         0001001       010100  -
1 6   00000000110         00000110          001110        010101  -
2 6   0000000101          00000101          001101        010110  -
3 6   00000100            001000            1001          010111  -
0 7   0000000001011       00000001111       0001000       011000  -
1 7   0000000001110       000000110         001010        011001  -
2 7   00000000101         000000101         001001        011010  -
3 7   000000100           000100            1000          011011  -
0 8   0000000001000       00000001011       00001111      011100  -
1 8   0000000001010       00000001110       0001110       011101  -
2 8   0000000001101       00000001101       0001101       011110  -
3 8   0000000100          0000100           01101         011111  -
0 9   00000000001111      000000001111      00001011      100000  -
1 9   00000000001110      00000001010       00001110      100001  -
2 9   0000000001001       00000001001       0001010       100010  -
3 9   00000000100         000000100         001100        100011  -
0 10  00000000001011      000000001011      000001111     100100  -
1 10  00000000001010      000000001110      00001010      100101  -
2 10  00000000001101      000000001101      00001101      100110  -
3 10  0000000001100       00000001100       0001100       100111  -
0 11  000000000001111     000000001000      000001011     101000  -
1 11  000000000001110     000000001010      000001110     101001  -
2 11  00000000001001      000000001001      00001001      101010  -
3 11  00000000001100      00000001000       00001100      101011  -
0 12  000000000001011     0000000001111     000001000     101100  -
1 12  000000000001010     0000000001110     000001010     101101  -
2 12  000000000001101     0000000001101     000001101     101110  -
3 12  00000000001000      000000001100      00001000      101111  -
0 13  0000000000001111    0000000001011     0000001101    110000  -
1 13  000000000000001     0000000001010     000000111     110001  -
2 13  000000000001001     0000000001001     000001001     110010  -
3 13  000000000001100     0000000001100     000001100     110011  -
0 14  0000000000001011    0000000000111     0000001001    110100  -
1 14  0000000000001110    00000000001011    0000001100    110101  -
2 14  0000000000001101    0000000000110     0000001011    110110  -
3 14  000000000001000     0000000001000     0000001010    110111  -
0 15  0000000000000111    00000000001001    0000000101    111000  -
1 15  0000000000001010    00000000001000    0000001000    111001  -
2 15  0000000000001001    00000000001010    0000000111    111010  -
3 15  0000000000001100    0000000000001     0000000110    111011  -
0 16  0000000000000100    00000000000111    0000000001    111100  -
1 16  0000000000000110    00000000000110    0000000100    111101  -
2 16  0000000000000101    00000000000101    0000000011    111110  -
3 16  0000000000001000    00000000000100    0000000010    111111  -
"""
# Tables 9-7 and 9-8: total_zeros of 4x4 blocks. One line per total_zeros; columns tzVlcIndex 1..15
_TABLE_9_7_8 = """
0   1          111     0101    00011  0101   000001  000001  000001  000001  00001  0000  0000  000  00  0
1   011        110     111     111    0100   00001   00001   0001    000000  00000  0001  0001  001  01  1
2   010        101     110     0101   0011   111     101     00001   0001    001    001   01    1    1   -
3   0011       100     101     0100   111    110     100     011     11      11     010   1     01   -   -
4   0010       011     0100    110    110    101     011     11      10      10     1     001   -    -   -
5   00011      0101    0011    101    101    100     11      10      001     01     011   -     -    -   -
6   00010      0100    100     100    100    011     010     010     01      0001   -     -     -    -   -
7   000011     0011    011     0011   011    010     0001    001     00001   -      -     -     -    -   -
8   000010     0010    0010    011    0010   0001    001     000000  -       -      -     -     -    -   -
9   0000011    00011   00011   0010   00001  001     000000  -       -       -      -     -     -    -   -
10  0000010    00010   00010   00010  0001   000000  -       -       -       -      -     -     -    -   -
11  00000011   000011  000001  00001  00000  -       -       -       -       -      -     -     -    -   -
12  00000010   000010  00001   00000  -      -       -       -       -       -      -     -     -    -   -
13  000000011  000001  000000  -      -      -       -       -       -       -      -     -     -    -   -
14  000000010  000000  -       -      -      -       -       -       -       -      -     -     -    -   -
15  000000001  -       -       -      -      -       -       -       -       -      -     -     -    -   -
"""
# Table 9-9 (a): total_zeros of chroma DC 2x2 blocks; columns tzVlcIndex 1..3
_TABLE_9_9 = """
0  1    1   1
1  01   01  0
2  001  00  -
3  000  -   -
"""
# Table 9-10: run_before. One line per run_before; columns zerosLeft 1..6 and > 6
_TABLE_9_10 = """
0   1  1   11  11   11   11   111
1   0  01  10  10   10   000  110
2   -  00  01  01   011  001  101
3   -  -   00  001  010  011  100
4   -  -   -   000  001  010  011
5   -  -   -   -    000  101  010
6   -  -   -   -    -    100  001
7   -  -   -   -    -    -    0001
8   -  -   -   -    -    -    00001
9   -  -   -   -    -    -    000001
10  -  -   -   -    -    -    0000001
11  -  -   -   -    -    -    00000001
12  -  -   -   -    -    -    000000001
13  -  -   -   -    -    -    0000000001
14  -  -   -   -    -    -    00000000001
"""
NC_CLASSES = ('0-1', '2-3', '4-7', '8+', 'dc')


def _columns(text, nkey):
    """the printed table as one {key: bit string} per column"""
    rows = [ln.split() for ln in text.strip().splitlines()]
    ncol = len(rows[0]) - nkey
    assert all(len(r) == nkey + ncol for r in rows)
    cols = [{} for _ in range(ncol)]
    for r in rows:
        key = tuple(int(v) for v in r[:nkey])
        for c, w in enumerate(r[nkey:]):
            if w != '-':
                assert set(w) <= {'0', '1'}
                cols[c][key if nkey > 1 else key[0]] = w
    return cols


def printed_tables():
    """{table name: {row: {value: bit string}}} as typed above. coeff_token: row = nC class, value = (TotalCoeff,
    TrailingOnes); total_zeros / total_zeros_dc: row = tzVlcIndex; run_before: row = min(zerosLeft, 7)"""
    ct = _columns(_TABLE_9_5, 2)
    return {
        'coeff_token': {NC_CLASSES[c]: {(tc, t1): w for (t1, tc), w in ct[c].items()} for c in range(5)},
        'total_zeros': {c + 1: col for c, col in enumerate(_columns(_TABLE_9_7_8, 1))},
        'total_zeros_dc': {c + 1: col for c, col in enumerate(_columns(_TABLE_9_9, 1))},
        'run_before': {c + 1: col for c, col in enumerate(_columns(_TABLE_9_10, 1))},
    }


def build_tree(words):
    """prefix tree of {value: bit string}: a node is a two-element list, a leaf the value (an int or a tuple)"""
    root = [None, None]
    for value, w in words.items():
        node = root
        for ch in w[:-1]:
            i = int(ch)
            if node[i] is None:
                node[i] = [None, None]
            assert isinstance(node[i], list), f'{w}: a shorter code word is its prefix'
            node = node[i]
        assert node[int(w[-1])] is None, f'{w}: the code word occurs twice or is a prefix of another'
        node[int(w[-1])] = value
    return root


def build_trees(tables=None):
    t = tables or printed_tables()
    return {name: {row: build_tree(words) for row, words in rows.items()} for name, rows in t.items()}


TABLES = printed_tables()
_TREES = build_trees(TABLES)


class ParseError(Exception):
    pass


# ---------------------------------------------------------------------------------------------------------------
# classes


def required_classes():
    """every parse class the suite's streams must reach (tests/test_parse_reference.py), see the module's audit"""
    req = set()
    for cls in NC_CLASSES:
        req |= {('coeff_token', cls, tc, t1) for (tc, t1) in TABLES['coeff_token'][cls]}
    req |= {('nC', kind, av) for kind in ('luma', 'i16dc', 'i16ac', 'cb_ac', 'cr_ac') for av in ('neither', 'left', 'upper', 'both')}
    req |= {('nC_neighbour', why) for why in ('skipped', 'cbp_clear', 'i16_no_ac', 'pcm', 'other_slice')}
    req |= {('trailing_ones', n) for n in (1, 2, 3)} | {('trailing_ones_sign', n, s) for n in (1, 2, 3) for s in '+-'}
    req |= {('level', sl, p, s) for sl in range(7) for p in range(16) for s in '+-'}
    req |= {('level_escape', c) for c in ('prefix14_suffixLength0', 'prefix15_plus15', 'prefix15_plain')}
    req |= {('level_first_minus2',), ('suffixLength_init', 1)} | {('suffixLength_inc', k) for k in range(6)}
    req |= {('level_threshold', sl, c) for sl in range(6) for c in ('at', 'above')}
    req |= {('total_zeros', mx, tc, tz) for mx in (16, 15) for tc, col in TABLES['total_zeros'].items() for tz in col}
    req |= {('total_zeros_dc', tc, tz) for tc, col in TABLES['total_zeros_dc'].items() for tz in col}
    req |= {('total_zeros_absent', mx) for mx in (16, 15, 4)}
    req |= {('run_before', zl, rb) for zl, col in TABLES['run_before'].items() for rb in col}
    req |= {('run_before', 'zeros_exhausted'), ('run_before', 'last_takes_remainder')}
    req |= {('mb_type', 'I', n) for n in range(26)} | {('mb_type', 'P', n) for n in range(31)}
    req |= {('sub_mb_type', n) for n in range(4)}
    req |= {('cbp_codeNum', col, n) for col in ('intra', 'inter') for n in range(48)}
    req |= {('mb_qp_delta', c) for c in ('-26', '+25', 'wrap')}
    req |= {('mb_skip_run', c) for c in ('zero', 'spans_row_end', 'ends_slice')}
    req |= {('pcm_alignment_zero_bits', n) for n in range(8)}
    req |= {('rbsp_stop_one_bit', n) for n in range(8)}
    req |= {('emulation_prevention', c) for c in ('slice_data', 'pcm_sample', 'nal_tail')}
    # ---- position classes, from the stream alone, where the parse kernels have a boundary:
    # a code word across a 32-bit boundary of the slice's RBSP (the ring holds the RBSP from the byte after the NAL
    # header, dec_parse.inc open_nal "RS.in_pos = s + 1"; the 64-bit cache takes one ring dword at a time, dec_parse.inc
    # vr_fill "if (r.n <= 32)" and the H264MI_RF* refills of cavlc_blk.inc "cache refill check in line, its body out of line")
    req |= {('straddle32', k) for k in ('coeff_token', 'level_escape', 'total_zeros', 'run_before', 'exp_golomb')}
    # a macroblock longer than the distances at which the VGPR windows are reloaded (dec_parse.inc vr_slide
    # "if (r.wi - r.wb >= 16)", vr_reslide "r.wi - r.wb >= 40"; cavlc_blk.inc "reload the windows once the reader is 40 dwords into w0")
    req |= {('mb_dwords', 'gt16'), ('mb_dwords', 'gt40')}
    # a slice whose RBSP exceeds one and two LDS rings (dec_parse.inc "constexpr int RING_BYTES = 16384", ring_fill topped
    # up from vr_slide "if (r.wb >= refill_at)" and before I_PCM samples "if ((byte0 >> 2) >= refill_at)")
    req |= {('slice_rings', 'gt1'), ('slice_rings', 'gt2')}
    return req


# ---------------------------------------------------------------------------------------------------------------
# bytes


def split_nals(data):
    """Annex B: the NAL units of a byte stream, each without its start code and trailing_zero_8bits"""
    n, k, starts = len(data), 0, []
    while k + 2 < n:
        if data[k] == 0 and data[k + 1] == 0 and data[k + 2] == 1:
            starts.append(k + 3)
            k += 3
        else:
            k += 1
    out = []
    for a, b in zip(starts, starts[1:] + [n + 3]):
        e = min(b - 3, n)
        while e > a and data[e - 1] == 0:    # zero_byte of the next start code, trailing_zero_8bits
            e -= 1
        if e > a:
            out.append(bytes(data[a:e]))
    return out


def unescape(payload):
    """7.3.1: the RBSP of a NAL unit's bytes after its header -> (rbsp, the RBSP byte index in front of which an
    emulation_prevention_three_byte stood, the index of each such byte in the payload)"""
    out, before, where, zeros = bytearray(), [], [], 0
    for k, c in enumerate(payload):
        if zeros >= 2 and c == 3:
            before.append(len(out))
            where.append(k)
            zeros = 0
            continue
        out.append(c)
        zeros = zeros + 1 if c == 0 else 0
    return bytes(out), before, where


class Reader:
    """the bits of one RBSP; every read is logged as (name, first bit, one past the last bit, value)"""

    def __init__(self, rbsp, counts):
        self.s = bin(int.from_bytes(b'\x01' + rbsp, 'big'))[3:]
        self.p = 0
        self.stop = self.s.rfind('1')     # rbsp_stop_one_bit (7.3.2.11): the last 1 bit
        if self.stop < 0:
            raise ParseError('no rbsp_stop_one_bit')
        self.counts = counts
        self.log = None

    def _note(self, name, a, value, straddle=None):
        if self.log is not None:
            self.log.append((name, a, self.p, value))
        if straddle and (a >> 5) != ((self.p - 1) >> 5):
            self.counts[('straddle32', straddle)] += 1

    def u(self, n, name='u', straddle=None):
        a = self.p
        if a + n > self.stop:
            raise ParseError(f'{name}: read past the end of the RBSP')
        v = int(self.s[a:a + n], 2) if n else 0
        self.p = a + n
        self._note(name, a, v, straddle)
        return v

    def ue(self, name='ue'):
        a = self.p
        one = self.s.find('1', a)
        z = one - a
        if one < 0 or one + z >= self.stop or z > 31:
            raise ParseError(f'{name}: Exp-Golomb code past the end of the RBSP')
        v = int(self.s[one:one + z + 1], 2) - 1      # 9-1: 2^z - 1 + read_bits(z)
        self.p = one + z + 1
        self._note(name, a, v, 'exp_golomb')
        return v

    def se(self, name='se'):
        a = self.p
        log, self.log = self.log, None
        k = self.ue(name)
        self.log = log
        v = (k + 1) // 2 if k & 1 else -(k // 2)     # Table 9-3
        if log is not None:
            log.append((name, a, self.p, v))
        return v

    def walk(self, tree, name, straddle):
        a, node, p, s = self.p, tree, self.p, self.s
        while True:
            if p >= self.stop:
                raise ParseError(f'{name}: code word past the end of the RBSP')
            node = node[s[p] == '1']
            p += 1
            if node is None:
                raise ParseError(f'{name}: no such code word ({s[a:p]})')
            if not isinstance(node, list):
                break
        self.p = p
        self._note(name, a, node, straddle)
        return node

    def more_rbsp_data(self):
        return self.p < self.stop


# ---------------------------------------------------------------------------------------------------------------
# parameter sets


class State:
    """what lasts from one access unit to the next: the parameter sets"""

    def __init__(self):
        self.sps = self.pps = None


_HIGH = (100, 110, 122, 244, 44, 83, 86, 118, 128)


def parse_sps(r):
    s = dict(profile=r.u(8, 'profile_idc'))
    r.u(8, 'constraint_flags'); r.u(8, 'level_idc'); r.ue('seq_parameter_set_id')
    if s['profile'] in _HIGH:
        raise ParseError('profile with chroma_format_idc: out of scope')
    s['log2_max_frame_num'] = r.ue('log2_max_frame_num_minus4') + 4
    s['poc_type'] = r.ue('pic_order_cnt_type')
    s['log2_max_poc_lsb'] = s['delta_always_zero'] = 0
    if s['poc_type'] == 0:
        s['log2_max_poc_lsb'] = r.ue('log2_max_pic_order_cnt_lsb_minus4') + 4
    elif s['poc_type'] == 1:
        s['delta_always_zero'] = r.u(1, 'delta_pic_order_always_zero_flag')
        r.se('offset_for_non_ref_pic'); r.se('offset_for_top_to_bottom_field')
        for _ in range(r.ue('num_ref_frames_in_pic_order_cnt_cycle')):
            r.se('offset_for_ref_frame')
    r.ue('max_num_ref_frames'); r.u(1, 'gaps_in_frame_num_value_allowed_flag')
    s['mbw'] = r.ue('pic_width_in_mbs_minus1') + 1
    s['mbh'] = r.ue('pic_height_in_map_units_minus1') + 1
    if not r.u(1, 'frame_mbs_only_flag'):
        raise ParseError('field or MBAFF coding: out of scope')
    r.u(1, 'direct_8x8_inference_flag')
    s['crop'] = [0, 0, 0, 0]
    if r.u(1, 'frame_cropping_flag'):
        s['crop'] = [r.ue('frame_crop_offset') for _ in range(4)]   # left, right, top, bottom
    if s['mbw'] > 1024 or s['mbh'] > 1024:
        raise ParseError('picture size')
    return s   # vui_parameters_present_flag and what follows change nothing of the parse


def parse_pps(r):
    p = {}
    r.ue('pic_parameter_set_id'); r.ue('seq_parameter_set_id')
    if r.u(1, 'entropy_coding_mode_flag'):
        raise ParseError('CABAC: out of scope')
    p['bottom_field_poc'] = r.u(1, 'bottom_field_pic_order_in_frame_present_flag')
    if r.ue('num_slice_groups_minus1'):
        raise ParseError('slice groups: out of scope')
    p['num_ref_default'] = r.ue('num_ref_idx_l0_default_active_minus1') + 1
    r.ue('num_ref_idx_l1_default_active_minus1')
    weighted = r.u(1, 'weighted_pred_flag'); r.u(2, 'weighted_bipred_idc')
    p['pic_init_qp'] = 26 + r.se('pic_init_qp_minus26'); r.se('pic_init_qs_minus26')
    p['cqp'] = r.se('chroma_qp_index_offset')
    p['dbk_control'] = r.u(1, 'deblocking_filter_control_present_flag')
    constrained = r.u(1, 'constrained_intra_pred_flag')
    p['redundant'] = r.u(1, 'redundant_pic_cnt_present_flag')
    if constrained or weighted:
        raise ParseError('constrained intra prediction or weighted prediction: out of scope')
    return p


# ---------------------------------------------------------------------------------------------------------------
# the picture


class _Picture:
    def __init__(self, mbw, mbh):
        self.mbw, self.mbh = mbw, mbh
        self.syntax = np.zeros((mbw * mbh, SYN_INTS), np.int32)
        # TotalCoeff known so far, the slice that set it (-1: nobody yet) and why, per 4x4 block: luma, Cb, Cr
        self.tc = [np.zeros((4 * mbh, 4 * mbw), np.int32)] + [np.zeros((2 * mbh, 2 * mbw), np.int32) for _ in (1, 2)]
        self.by = [np.full(a.shape, -1, np.int32) for a in self.tc]
        self.why = [np.zeros(a.shape, np.int8) for a in self.tc]
        self.done = np.zeros(mbw * mbh, bool)
        self.words = {}     # macroblock address -> its logged code words
        self.span = {}      # macroblock address -> (first bit, one past the last bit) of its macroblock_layer()
        self.nslices = 0


_WHY = {'coded': 0, 'skipped': 1, 'cbp_clear': 2, 'i16_no_ac': 3, 'pcm': 4}
_WHY_NAME = {v: k for k, v in _WHY.items()}


class Parsed:
    def __init__(self, pic, size, counts, ref_idc):
        self.syntax, self.geometry, self.size, self.counts, self.ref_idc = pic.syntax, (pic.mbw, pic.mbh), size, counts, ref_idc
        self._words = pic.words
        self._span = pic.span

    def layer_span(self, mb):
        """(first bit, one past the last bit) of macroblock mb's macroblock_layer() in its slice's RBSP, the mb_skip_run in
        front of it not included; None for a skipped macroblock, which has no macroblock_layer()"""
        return self._span.get(mb)

    def words(self, mb):
        """the logged code words of macroblock mb: (name, first bit, one past the last bit, value), positions in its
        slice's RBSP, in stream order, an mb_skip_run in front of the macroblock included. tests/writeaudit.py cuts a
        macroblock into its residual blocks by these names: a block opens with the word whose name holds 'coeff_token',
        and the run is named 'mb_skip_run' (tests/test_enc_write_audit.py holds both names to a written block)"""
        return list(self._words.get(mb, []))

    def explain(self, mb):
        """the code words of macroblock mb: 'bits a..b name = value', positions in its slice's RBSP"""
        return [f'bits {a}..{b - 1} {name} = {v}' for name, a, b, v in self._words.get(mb, [])]


class _Slice:
    """slice_data() of one slice over the picture's maps"""

    def __init__(self, pic, r, counts, trees, sid, first, st, qp, cqp):
        self.pic, self.r, self.c, self.t, self.sid, self.first, self.st, self.qp, self.cqp = pic, r, counts, trees, sid, first, st, qp, cqp

    # ---- 9.2.1
    def _nc(self, plane, x, y, kind):
        """nC of the block at 4x4 coordinates (x, y) of the plane's map"""
        tc, by, why = self.pic.tc[plane], self.pic.by[plane], self.pic.why[plane]
        n = []
        for nx, ny in ((x - 1, y), (x, y - 1)):
            if nx < 0 or ny < 0:
                n.append(None)
            elif by[ny, nx] != self.sid:
                if by[ny, nx] >= 0:
                    self.c[('nC_neighbour', 'other_slice')] += 1
                n.append(None)
            else:
                if why[ny, nx]:
                    self.c[('nC_neighbour', _WHY_NAME[int(why[ny, nx])])] += 1
                n.append(int(tc[ny, nx]))
        a, b = n
        self.c[('nC', kind, {(0, 0): 'neither', (1, 0): 'left', (0, 1): 'upper', (1, 1): 'both'}[(a is not None, b is not None)])] += 1
        if a is not None and b is not None:
            return (a + b + 1) >> 1
        return a if a is not None else (b if b is not None else 0)

    # ---- 7.3.5.3.2 / 9.2
    def residual_block(self, nc, maxnum, what):
        """-> (coeffLevel list of maxnum, TotalCoeff)"""
        r, c = self.r, self.c
        cls = 'dc' if nc < 0 else NC_CLASSES[0 if nc < 2 else 1 if nc < 4 else 2 if nc < 8 else 3]
        tc, t1 = r.walk(self.t['coeff_token'][cls], f'{what} coeff_token(nC {nc})', 'coeff_token')
        c[('coeff_token', cls, tc, t1)] += 1
        if tc > maxnum:
            raise ParseError(f'{what}: TotalCoeff {tc} of at most {maxnum}')
        out = [0] * maxnum
        if tc == 0:
            return out, 0
        if t1:
            c[('trailing_ones', t1)] += 1
        sl = 1 if tc > 10 and t1 < 3 else 0
        if sl:
            c[('suffixLength_init', 1)] += 1
        level = []
        for i in range(tc):
            if i < t1:
                s = r.u(1, 'trailing_ones_sign_flag')
                level.append(1 - 2 * s)
                c[('trailing_ones_sign', t1, '-' if s else '+')] += 1
                continue
            a = r.p
            one = r.s.find('1', a)
            prefix = one - a
            if one < 0 or one >= r.stop or prefix > 15:
                raise ParseError(f'{what}: level_prefix above 15 or past the end')
            r.p = one + 1
            code = min(15, prefix) << sl
            size = 4 if (prefix == 14 and sl == 0) else (prefix - 3 if prefix >= 15 else sl)
            if size:
                log, r.log = r.log, None
                code += r.u(size, 'level_suffix')
                r.log = log
            if prefix >= 15 and sl == 0:
                code += 15
                c[('level_escape', 'prefix15_plus15')] += 1
            elif prefix >= 15:
                c[('level_escape', 'prefix15_plain')] += 1
            elif prefix == 14 and sl == 0:
                c[('level_escape', 'prefix14_suffixLength0')] += 1
            if i == t1 and t1 < 3:
                code += 2
                c[('level_first_minus2',)] += 1
            v = (code + 2) >> 1 if code % 2 == 0 else (-code - 1) >> 1
            r._note(f'level(suffixLength {sl}, level_prefix {prefix})', a, v, 'level_escape' if prefix >= 14 else None)
            c[('level', sl, prefix, '+' if v > 0 else '-')] += 1
            thr = 3 if sl == 0 else 3 << (sl - 1)
            if sl < 6 and abs(v) in (thr, thr + 1):
                c[('level_threshold', sl, 'at' if abs(v) == thr else 'above')] += 1
            level.append(v)
            was = sl
            if sl == 0:
                sl = 1
            if abs(v) > (3 << (sl - 1)) and sl < 6:
                sl += 1
            for k in range(was, sl):
                c[('suffixLength_inc', k)] += 1
        if tc < maxnum:
            if maxnum == 4:
                zeros = r.walk(self.t['total_zeros_dc'][tc], f'total_zeros(chroma DC, TotalCoeff {tc})', 'total_zeros')
                c[('total_zeros_dc', tc, zeros)] += 1
            else:
                zeros = r.walk(self.t['total_zeros'][tc], f'total_zeros(TotalCoeff {tc})', 'total_zeros')
                c[('total_zeros', maxnum, tc, zeros)] += 1
            if tc + zeros > maxnum:
                raise ParseError(f'{what}: total_zeros {zeros} with TotalCoeff {tc} of {maxnum}')
        else:
            zeros = 0
            c[('total_zeros_absent', maxnum)] += 1
        run, left = [], zeros
        for i in range(tc - 1):
            if left > 0:
                rb = r.walk(self.t['run_before'][min(left, 7)], f'run_before(zerosLeft {left})', 'run_before')
                c[('run_before', min(left, 7), rb)] += 1
                if rb > left:
                    raise ParseError(f'{what}: run_before {rb} with zerosLeft {left}')
                left -= rb
                if left == 0:
                    c[('run_before', 'zeros_exhausted')] += 1
            else:
                rb = 0
            run.append(rb)
        run.append(left)
        if left > 0:
            c[('run_before', 'last_takes_remainder')] += 1
        pos = -1
        for i in range(tc - 1, -1, -1):
            pos += run[i] + 1
            out[pos] = level[i]
        return out, tc

    # ---- 7.3.5
    def _open(self, addr, mb_type):
        pic = self.pic
        if pic.done[addr]:
            raise ParseError(f'macroblock {addr} twice')
        pic.done[addr] = True
        s = pic.syntax[addr]
        s[:] = 0
        s[0], s[1], s[73], s[74], s[75] = mb_type, self.st, self.slice_qp, self.first, self.cqp
        s[77], s[78], s[79] = self.dbk
        return s

    def _set_map(self, addr, luma, chroma, why_l, why_c):
        mx, my = addr % self.pic.mbw, addr // self.pic.mbw
        for pl, n, v, w in ((0, 4, luma, why_l), (1, 2, chroma, why_c), (2, 2, chroma, why_c)):
            sl = (slice(n * my, n * my + n), slice(n * mx, n * mx + n))
            self.pic.tc[pl][sl] = v
            self.pic.by[pl][sl] = self.sid
            self.pic.why[pl][sl] = _WHY[w]

    def _put(self, plane, x, y, tc):
        self.pic.tc[plane][y, x] = tc
        self.pic.why[plane][y, x] = 0

    def slice_data(self, dbk):
        pic, r, c = self.pic, self.r, self.c
        self.dbk, self.slice_qp = dbk, self.qp
        total, addr, more = pic.mbw * pic.mbh, self.first, True
        while more:
            if addr >= total:
                raise ParseError('slice data past the end of the picture')
            pending = r.log = []
            start = r.p
            if self.st == 0:
                run = r.ue('mb_skip_run')
                if run > total - addr:
                    raise ParseError('mb_skip_run past the end of the picture')
                if run == 0:
                    c[('mb_skip_run', 'zero')] += 1
                elif addr // pic.mbw != (addr + run - 1) // pic.mbw:
                    c[('mb_skip_run', 'spans_row_end')] += 1
                for _ in range(run):
                    self._open(addr, -1)
                    self._set_map(addr, 0, 0, 'skipped', 'skipped')
                    addr += 1
                if run:
                    more = r.more_rbsp_data()
                    if not more:
                        c[('mb_skip_run', 'ends_slice')] += 1
                        pic.words.setdefault(addr - 1, []).extend(pending)
                        break
                    if addr >= total:
                        raise ParseError('slice data past the end of the picture')
            r.log = pic.words.setdefault(addr, [])
            r.log.extend(pending)
            layer = r.p
            self.macroblock_layer(addr)
            pic.span[addr] = (layer, r.p)
            bits = r.p - start
            if bits > 16 * 32:
                c[('mb_dwords', 'gt16')] += 1
            if bits > 40 * 32:
                c[('mb_dwords', 'gt40')] += 1
            more = r.more_rbsp_data()
            addr += 1
        r.log = None

    def macroblock_layer(self, addr):
        pic, r, c = self.pic, self.r, self.c
        mt = r.ue('mb_type')
        it = mt if self.st == 2 else mt - 5     # Table 7-11 number, negative: a P macroblock type of Table 7-13
        if it > 25:
            raise ParseError(f'mb_type {mt}')
        c[('mb_type', 'I' if self.st == 2 else 'P', mt)] += 1
        s = self._open(addr, mt)
        mx, my = addr % pic.mbw, addr // pic.mbw
        if it == 25:                                # I_PCM
            n = -r.p % 8
            if r.u(n, 'pcm_alignment_zero_bit'):
                raise ParseError('pcm_alignment_zero_bit not zero')
            c[('pcm_alignment_zero_bits', n)] += 1
            b0 = r.p // 8
            if any(b0 < e <= b0 + 383 for e in self.epb_before):
                c[('emulation_prevention', 'pcm_sample')] += 1
            log, r.log = r.log, None
            s[488:872] = [r.u(8, 'pcm_sample') for _ in range(384)]
            r.log = log
            log.append(('pcm_sample x 384', b0 * 8, r.p, '...'))
            self._set_map(addr, 16, 16, 'pcm', 'pcm')
            return
        i16 = it >= 1
        if it == 0:
            for k in range(16):
                s[38 + k] = r.u(1, f'prev_intra4x4_pred_mode_flag[{k}]')
                if not s[38 + k]:
                    s[54 + k] = r.u(3, f'rem_intra4x4_pred_mode[{k}]')
        if it >= 0:
            s[70] = r.ue('intra_chroma_pred_mode')
            if s[70] > 3:
                raise ParseError('intra_chroma_pred_mode')
        else:
            counts = {0: [1], 1: [1, 1], 2: [1, 1]}.get(mt)
            if counts is None:                      # P_8x8, P_8x8ref0: sub_mb_pred (7.3.5.2)
                for k in range(4):
                    s[2 + k] = r.ue(f'sub_mb_type[{k}]')
                    if s[2 + k] > 3:
                        raise ParseError('sub_mb_type')
                    c[('sub_mb_type', int(s[2 + k]))] += 1
                counts = [{0: 1, 1: 2, 2: 2, 3: 4}[int(s[2 + k])] for k in range(4)]
            # one active reference: no ref_idx_l0 (num_ref_idx_l0_active_minus1 is 0)
            for k in range(sum(counts)):
                s[6 + 2 * k] = r.se(f'mvd_l0[{k}][0]')
                s[7 + 2 * k] = r.se(f'mvd_l0[{k}][1]')
        if i16:
            cbp = (15 if it >= 13 else 0) | ((((it - 1) // 4) % 3) << 4)
        else:
            code = r.ue('coded_block_pattern')
            if code > 47:
                raise ParseError('coded_block_pattern')
            c[('cbp_codeNum', 'intra' if it == 0 else 'inter', code)] += 1
            cbp = CBP_TABLE[code][0 if it == 0 else 1]
            s[71], s[76] = cbp, code
        self._set_map(addr, 0, 0, 'i16_no_ac' if i16 and not cbp & 15 else 'cbp_clear', 'cbp_clear')
        if not (cbp or i16):
            return
        dq = r.se('mb_qp_delta')
        if not -26 <= dq <= 25:
            raise ParseError('mb_qp_delta')
        s[72] = dq
        if dq in (-26, 25):
            c[('mb_qp_delta', '-26' if dq < 0 else '+25')] += 1
        if not 0 <= self.qp + dq <= 51:
            c[('mb_qp_delta', 'wrap')] += 1
        self.qp = (self.qp + dq + 52) % 52            # 7-37
        # residual() 7.3.5.3
        if i16:
            s[80:96], _ = self.residual_block(self._nc(0, 4 * mx, 4 * my, 'i16dc'), 16, 'Intra16x16DCLevel')
        for blk in range(16):
            if not (cbp >> (blk >> 2)) & 1:
                continue
            x, y = 4 * mx + BLK_XY[blk][0] // 4, 4 * my + BLK_XY[blk][1] // 4
            if i16:
                lv, tc = self.residual_block(self._nc(0, x, y, 'i16ac'), 15, f'Intra16x16ACLevel[{blk}]')
                s[96 + 16 * blk:96 + 16 * blk + 15] = lv
            else:
                lv, tc = self.residual_block(self._nc(0, x, y, 'luma'), 16, f'LumaLevel4x4[{blk}]')
                s[96 + 16 * blk:96 + 16 * blk + 16] = lv
            self._put(0, x, y, tc)
        if cbp >> 4:
            for k in (0, 1):
                s[352 + 4 * k:356 + 4 * k], _ = self.residual_block(-1, 4, f'ChromaDCLevel[{k}]')
            if cbp >> 4 == 2:
                for k in (0, 1):
                    for blk in range(4):
                        x, y = 2 * mx + (blk & 1), 2 * my + (blk >> 1)
                        lv, tc = self.residual_block(self._nc(1 + k, x, y, ('cb_ac', 'cr_ac')[k]), 15, f'ChromaACLevel[{k}][{blk}]')
                        s[360 + 64 * k + 16 * blk:360 + 64 * k + 16 * blk + 15] = lv
                        self._put(1 + k, x, y, tc)


def _slice(pic, state, payload, nal_type, ref_idc, counts, trees):
    rbsp, before, where = unescape(payload)
    r = Reader(rbsp, counts)
    sps, pps = state.sps, state.pps
    if sps is None or pps is None:
        raise ParseError('slice before its parameter sets')
    if nal_type == 5 and ref_idc == 0:
        raise ParseError('IDR picture with nal_ref_idc 0')
    first = r.ue('first_mb_in_slice')
    st = r.ue('slice_type') % 5
    r.ue('pic_parameter_set_id')
    if st not in (0, 2) or (nal_type == 5 and st != 2):
        raise ParseError('slice_type')
    if first >= pic.mbw * pic.mbh:
        raise ParseError('first_mb_in_slice')
    r.u(sps['log2_max_frame_num'], 'frame_num')
    if nal_type == 5:
        r.ue('idr_pic_id')
    if sps['poc_type'] == 0:
        r.u(sps['log2_max_poc_lsb'], 'pic_order_cnt_lsb')
        if pps['bottom_field_poc']:
            r.se('delta_pic_order_cnt_bottom')
    elif sps['poc_type'] == 1 and not sps['delta_always_zero']:
        r.se('delta_pic_order_cnt[0]')
        if pps['bottom_field_poc']:
            r.se('delta_pic_order_cnt[1]')
    if pps['redundant']:
        r.ue('redundant_pic_cnt')
    nref = pps['num_ref_default']
    if st == 0:
        if r.u(1, 'num_ref_idx_active_override_flag'):
            nref = r.ue('num_ref_idx_l0_active_minus1') + 1
        if r.u(1, 'ref_pic_list_modification_flag_l0'):
            while r.ue('modification_of_pic_nums_idc') != 3:
                r.ue('abs_diff_pic_num_minus1 / long_term_pic_num')
        if nref > 1:
            raise ParseError('more than one active reference: out of scope')
    if ref_idc:
        if nal_type == 5:
            r.u(1, 'no_output_of_prior_pics_flag'); r.u(1, 'long_term_reference_flag')
        elif r.u(1, 'adaptive_ref_pic_marking_mode_flag'):
            while True:
                op = r.ue('memory_management_control_operation')
                if op == 0:
                    break
                if op in (1, 3):
                    r.ue('difference_of_pic_nums_minus1')
                if op == 2:
                    r.ue('long_term_pic_num')
                if op in (3, 6):
                    r.ue('long_term_frame_idx')
                if op == 4:
                    r.ue('max_long_term_frame_idx_plus1')
    qp = pps['pic_init_qp'] + r.se('slice_qp_delta')
    idc = fa = fb = 0
    if pps['dbk_control']:
        idc = r.ue('disable_deblocking_filter_idc')
        if idc > 2:
            raise ParseError('disable_deblocking_filter_idc')
        if idc != 1:
            fa, fb = 2 * r.se('slice_alpha_c0_offset_div2'), 2 * r.se('slice_beta_offset_div2')
            if not (-12 <= fa <= 12 and -12 <= fb <= 12):
                raise ParseError('deblocking filter offsets')
    if not 0 <= qp <= 51 or not -12 <= pps['cqp'] <= 12:
        raise ParseError('SliceQPY or chroma_qp_index_offset')
    data_byte = r.p // 8
    sl = _Slice(pic, r, counts, trees, pic.nslices, first, st, qp, pps['cqp'])
    sl.epb_before = before
    pic.nslices += 1
    sl.slice_data((idc, fa, fb))
    # ---- byte classes
    counts[('rbsp_stop_one_bit', r.stop % 8)] += 1
    if r.p != r.stop:
        raise ParseError('slice data does not end at the rbsp_stop_one_bit')
    if any(e > data_byte for e in before):
        counts[('emulation_prevention', 'slice_data')] += 1
    if any(k >= len(payload) - 3 for k in where):
        counts[('emulation_prevention', 'nal_tail')] += 1
    if len(rbsp) > RING_BYTES:
        counts[('slice_rings', 'gt1')] += 1
    if len(rbsp) > 2 * RING_BYTES:
        counts[('slice_rings', 'gt2')] += 1


def parse(access_unit, state, trees=None):
    """one access unit (parameter sets, if any, and all slices of one picture) -> Parsed. state: a State, kept by the
    caller from unit to unit. trees: build_trees() of other tables (the sensitivity test)"""
    trees = trees or _TREES
    counts = Counter()
    pic = size = None
    pic_key = None
    for nal in split_nals(access_unit):
        if nal[0] & 0x80:
            raise ParseError('forbidden_zero_bit')
        ref_idc, typ = (nal[0] >> 5) & 3, nal[0] & 31
        if typ == 7:
            state.sps = parse_sps(Reader(unescape(nal[1:])[0], counts))
        elif typ == 8:
            state.pps = parse_pps(Reader(unescape(nal[1:])[0], counts))
        elif typ in (1, 5):
            if state.sps is None:
                raise ParseError('slice before its parameter sets')
            if pic is None:
                sps = state.sps
                pic = _Picture(sps['mbw'], sps['mbh'])
                cl, cr, ct, cb = sps['crop']
                size = (16 * sps['mbw'] - 2 * (cl + cr), 16 * sps['mbh'] - 2 * (ct + cb))
                pic_key = (typ == 5, ref_idc != 0)
            elif pic_key != (typ == 5, ref_idc != 0):
                raise ParseError('slices of one picture differ in IDR-ness or nal_ref_idc being 0 (7.4.1.2.4)')
            _slice(pic, state, nal[1:], typ, ref_idc, counts, trees)
    if pic is None:
        raise ParseError('no slice in the access unit')
    if not pic.done.all():
        raise ParseError('the slices do not cover the picture')
    return Parsed(pic, size, counts, int(pic_key[1]))


# ---------------------------------------------------------------------------------------------------------------
# the writer (9.2 read backwards, from the same printed tables)


def write_residual_block(levels, nC, maxNumCoeff, tables=None):
    """the bits of residual_block_cavlc(levels (scan order, maxNumCoeff of them), nC) as a string of '0' / '1'"""
    t = tables or TABLES
    levels = [int(v) for v in levels]
    assert len(levels) == maxNumCoeff
    nz = [k for k, v in enumerate(levels) if v]
    tc = len(nz)
    lv = [levels[k] for k in reversed(nz)]      # highest frequency first
    t1 = 0
    while t1 < min(3, tc) and abs(lv[t1]) == 1:
        t1 += 1
    cls = 'dc' if nC < 0 else NC_CLASSES[0 if nC < 2 else 1 if nC < 4 else 2 if nC < 8 else 3]
    out = [t['coeff_token'][cls][(tc, t1)]]
    if tc == 0:
        return out[0]
    out += ['1' if v < 0 else '0' for v in lv[:t1]]
    sl = 1 if tc > 10 and t1 < 3 else 0
    for i in range(t1, tc):
        v = lv[i]
        code = 2 * v - 2 if v > 0 else -2 * v - 1
        if i == t1 and t1 < 3:
            code -= 2
        if sl == 0:
            if code < 14:
                out.append('0' * code + '1')
            elif code < 30:
                out.append('0' * 14 + '1' + format(code - 14, '04b'))
            else:
                assert code - 30 < 4096, f'level {v} has no code with level_prefix <= 15'
                out.append('0' * 15 + '1' + format(code - 30, '012b'))
        elif code < (15 << sl):
            out.append('0' * (code >> sl) + '1' + format(code & ((1 << sl) - 1), f'0{sl}b'))
        else:
            assert code - (15 << sl) < 4096, f'level {v} has no code with level_prefix <= 15'
            out.append('0' * 15 + '1' + format(code - (15 << sl), '012b'))
        if sl == 0:
            sl = 1
        if abs(v) > (3 << (sl - 1)) and sl < 6:
            sl += 1
    zeros = nz[-1] + 1 - tc
    if tc < maxNumCoeff:
        out.append(t['total_zeros_dc' if maxNumCoeff == 4 else 'total_zeros'][tc][zeros])
    left = zeros
    for i in range(tc - 1):
        if left <= 0:
            break
        hi, lo = nz[tc - 1 - i], nz[tc - 2 - i]
        rb = hi - lo - 1
        out.append(t['run_before'][min(left, 7)][rb])
        left -= rb
    return ''.join(out)
