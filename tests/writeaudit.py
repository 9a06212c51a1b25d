"""Write-class audit of the encoder's bit writer -- TEST INFRASTRUCTURE ONLY.

csrc/enc_bits.inc writes an access unit in two parts: cavlc_code_mb / cavlc_block, the CAVLC of one macroblock, and
enc_pack_block / enc_pack_block_slices, the packer (mb_skip_run, bit offsets, RBSP, emulation prevention). This module
names every path of both that the bytes can tell apart as a class, and counts the classes from bytes alone:

  count(access unit, parseref.State) -> Counter of classes. tests/parseref.py parses the unit (its Reader logs every
      code word with its bit span, its counters are the CAVLC classes) and un-escapes every slice NAL unit. The same
      function serves the oracle's bytes on the CPU (tests/test_enc_write_audit.py) and the GPU encoder's own bytes
      (tests/test_gpu_enc_write.py).
  all_classes()       the full list: parseref's classes that name a writer path, and one position class per boundary of
                      enc_bits.inc (the source line is quoted beside each).
  NOT_REACHED         classes no encoder output holds, each with the reason from the syntax or the encoder's rules.
  REQUIRED            all_classes() - NOT_REACHED: the directed clips must reach every one, each claimed by one clip.
  directed_clips()    seeded encaudit.Clips, each with the classes it is there for: `targets` are held on the oracle's
                      bytes and on the GPU's with one slice, `slice_targets` (the classes of slice index > 0) on the
                      GPU's bytes with three slices -- the oracle encoder codes one slice per picture.
"""
import functools
from collections import Counter

import numpy as np

import encaudit
import parseref

PACK_THREADS, PACK_MBT, EPB = 256, 32, 64   # enc_bits.inc (tests/test_enc_write_audit.py reads the source and compares)
CHUNK = EPB * PACK_THREADS                  # "for (int c0 = 0; c0 < rbsp_bytes; c0 += EPB * PACK_THREADS)"

# ---------------------------------------------------------------- classes
# parseref's classes that name a path of cavlc_code_mb / cavlc_block or of the packer's mb_skip_run. Its other classes
# (sub_mb_type, I_PCM alignment and samples, stop bit position, straddles, ring sizes) are boundaries of the parse kernels.
# ('level', suffixLength, level_prefix, sign) is a row of the parser's prefix walk; cavlc_block computes the word
# ("lb_put(b, 1, (code >> sl) + 1); lb_put(b, code & ((1 << sl) - 1), sl)") and branches only where level_escape,
# level_threshold, level_first_minus2 and suffixLength_inc / _init have a class, so those stand for the level code.
_PARSE_FAMILIES = ('coeff_token', 'nC', 'nC_neighbour', 'trailing_ones', 'trailing_ones_sign', 'level_escape',
                   'level_first_minus2', 'suffixLength_init', 'suffixLength_inc', 'level_threshold', 'total_zeros',
                   'total_zeros_dc', 'total_zeros_absent', 'run_before', 'mb_type', 'cbp_codeNum', 'mb_qp_delta', 'mb_skip_run')

# macroblock classes: cavlc_code_mb's merge of the lane buffers and the packer's put_mb
MB_CLASSES = {
    ('mb_bits', 'le128'): 'put_mb "k == 0 ? a0.x : k == 1 ? a0.y : k == 2 ? a0.z : k == 3 ? a0.w : src[k]": all from the 16-byte load',
    ('mb_bits', 'gt128'): 'put_mb "... : src[k]": dwords 4.. of the slot are loaded as they are reached',
    ('mb_bits', 'mult32'): 'put_mb "const int nb = (k == n - 1 && (l & 31)) ? (int)(l & 31) : 32": the last dword is whole',
    ('mb_start', 'mod32_0'): 'bits_or "int sh = (int)(pos & 31)": a macroblock placed at shift 0',
    ('block_bits', 'gt32'): 'cavlc_code_mb "n = (len + 31) >> 5" above 1: more than one dword of bits[28][24]',
    ('block_bits', 'gt256'): 'lb_put "b.buf[b.nd++]": a lane past 8 of the 24 dwords of "uint32_t bits[28][24]"',
    ('block_bits', 'mult32'): 'cavlc_code_mb "if (k == n - 1 && (len & 31)) v &= ...": no mask on the last dword; lb_flush "if (b.nacc > 0)"',
    ('block_offset', 'mod32_0'): 'cavlc_code_mb "if (bsh) atomicOr(&out[w0 + k + 1], v << (32 - bsh))": a residual block at lane shift 0',
}
# packer classes, per slice: `per`, the thread ranges and the skip runs
_PACK = {
    'per_gt32': '"const int per = ((nmb + PACK_THREADS - 1) / PACK_THREADS + 3) & ~3": above PACK_MBT, the four tail loops run',
    'tail_coded_mb': '"for (int i = i0 + PACK_MBT; i < i1; i++)" (last coded MB, row sums, bit count, placement): a coded MB there',
    'range_no_coded_mb': '"int my_last = -1": a thread range without a coded MB under the max-scan',
    'skip_run_from_earlier_range': '"const int prev = block_excl_scan<true>(my_last, ...)": an mb_skip_run that counts MBs of an earlier range',
    'trailing_run': '"if (trail > 0) { bits_ue(rb, pos, (uint32_t)trail); ... }"',
    'no_coded_mb': '"const int trail = idr ? 0 : nmb - 1 - last_coded" with last_coded == -1 (m0 - 1 in a later slice)',
    'mbh_256': '"__shared__ int s_rb[256]" filled to its last entry',
}
_PACK_PICTURE_ONLY = {
    'mbw_512': 'the widest row enc_create accepts (runtime_enc.inc, w <= 16 * H264MI_ENC_MAX_MBW): "xe = (r + 1) * a.mbw" row changes of the row sums',
}
# emulation prevention classes, per slice NAL unit; an index is the RBSP byte index in the slice
_EP = {
    'ins_at_64k': '"int z = pnz >= 0 ? b0 - 1 - pnz : b0": both zeros of the run come from the max-scan',
    'ins_at_64k_plus_1': 'the same with one zero from the scan and one of the thread\'s own',
    'two_in_span': '"const int my_ins = __popcll(insm)" of 2 or more: the later threads\' `before` moves by more than one',
    'ins_ge_16384': '"carry_ins += chunk_ins" not zero: an insertion in a later chunk, or before one',
    'zero_run_across_chunk': '"const int pnz = max(carry_nz, ...)": the zero run of an insertion starts in the chunk before',
    'ins_before_0': '"byte <= 3 && z2 >= 2": before a third zero byte', 'ins_before_1': '"byte <= 3": 00 00 01',
    'ins_before_2': '"byte <= 3": 00 00 02', 'ins_before_3': '"byte <= 3": 00 00 03',
    'ins_after_zero_run_2': '"z2 >= 2 && !(z2 & 1)" at z2 == 2',
    'ins_after_zero_run_4plus': '"!(z2 & 1)" at z2 == 4, 6, ...: a second insertion inside one run of zero bytes',
}


def parse_classes():
    return {k for k in parseref.required_classes() if k[0] in _PARSE_FAMILIES}


def position_classes():
    """{class: the source line of enc_bits.inc it is there for}; the `_slice` families are the same boundaries in
    slice index > 0 of a multi-slice picture (enc_pack_block_slices)"""
    out = dict(MB_CLASSES)
    for fam in ('pack', 'pack_slice'):
        out.update({(fam, k): v for k, v in _PACK.items()})
    out.update({('pack', k): v for k, v in _PACK_PICTURE_ONLY.items()})
    for fam in ('ep', 'ep_slice'):
        out.update({(fam, k): v for k, v in _EP.items()})
    return out


def all_classes():
    return parse_classes() | set(position_classes())


# ---------------------------------------------------------------- counting from bytes
def thread_ranges(m0, m1):
    """the packer's MB range grid of the slice [m0, m1): (first MB of thread 0's grid cell, MBs per thread)
    enc_pack_block_slices "const int mg = m0 & ~3, per = ((m1 - mg + PACK_THREADS - 1) / PACK_THREADS + 3) & ~3"; with
    m0 == 0 this is enc_pack_block's"""
    mg = m0 & ~3
    return mg, ((m1 - mg + PACK_THREADS - 1) // PACK_THREADS + 3) & ~3


def _count_pack(c, fam, coded, m0, m1, p_slice):
    mg, per = thread_ranges(m0, m1)
    if per > PACK_MBT:
        c[(fam, 'per_gt32')] += 1
    idx = np.flatnonzero(coded[m0:m1]) + m0
    tid = (idx - mg) // per
    c[(fam, 'tail_coded_mb')] += int(((idx - mg) - tid * per >= PACK_MBT).sum())
    c[(fam, 'range_no_coded_mb')] += -(-(m1 - mg) // per) - len(set(tid.tolist()))
    if not p_slice:
        return
    prev = m0 - 1
    for i, t in zip(idx.tolist(), tid.tolist()):
        if prev + 1 < max(m0, mg + t * per) and prev + 1 < i:     # the run's first skipped MB lies in an earlier range
            c[(fam, 'skip_run_from_earlier_range')] += 1
        prev = i
    if prev < m1 - 1:
        c[(fam, 'trailing_run')] += 1
    if idx.size == 0:
        c[(fam, 'no_coded_mb')] += 1


def _count_ep(c, fam, payload):
    rbsp, before, _ = parseref.unescape(payload)
    spans = Counter()
    for b in before:
        run = 0
        while run < b and rbsp[b - 1 - run] == 0:
            run += 1
        assert run >= 2 and b < len(rbsp), (b, run)
        spans[b // EPB] += 1
        if b % EPB < 2:
            c[(fam, 'ins_at_64k' if b % EPB == 0 else 'ins_at_64k_plus_1')] += 1
        if b >= CHUNK:
            c[(fam, 'ins_ge_16384')] += 1
        if b // CHUNK > (b - run) // CHUNK:
            c[(fam, 'zero_run_across_chunk')] += 1
        c[(fam, f'ins_before_{rbsp[b]}')] += 1
        c[(fam, 'ins_after_zero_run_2' if run == 2 else 'ins_after_zero_run_4plus')] += 1
        assert run % 2 == 0, (b, run)
    c[(fam, 'two_in_span')] += sum(1 for v in spans.values() if v >= 2)
    return len(before), len(rbsp)


def _count_mbs(c, p, coded):
    for addr in np.flatnonzero(coded).tolist():   # (a trailing mb_skip_run is logged with the slice's last, skipped, MB)
        w = [e for e in p.words(addr) if e[0] != 'mb_skip_run']
        start, end = w[0][1], w[-1][2]
        bits = end - start
        c[('mb_bits', 'le128' if bits <= 128 else 'gt128')] += 1
        if bits % 32 == 0:
            c[('mb_bits', 'mult32')] += 1
        if start % 32 == 0:
            c[('mb_start', 'mod32_0')] += 1
        cuts = [e[1] for e in w if 'coeff_token' in e[0]] + [end]   # a residual block opens with its coeff_token
        for a, b in zip(cuts, cuts[1:]):
            n = b - a
            if n > 32:
                c[('block_bits', 'gt32')] += 1
            if n > 256:
                c[('block_bits', 'gt256')] += 1
            if n % 32 == 0:
                c[('block_bits', 'mult32')] += 1
            if (a - start) % 32 == 0:
                c[('block_offset', 'mod32_0')] += 1


def count(access_unit, state):
    """one access unit of the encoder -> Counter of the writer classes it reaches; state: a parseref.State kept by the
    caller from unit to unit. The counter's .info holds (slices, RBSP bytes per slice, insertions per slice)."""
    p = parseref.parse(access_unit, state)
    want = all_classes()
    c = Counter({k: v for k, v in p.counts.items() if k in want})
    mbw, mbh = p.geometry
    nmb = mbw * mbh
    coded = p.syntax[:, 0] >= 0                       # parseref opens a skipped macroblock with mb_type -1
    firsts = sorted(set(p.syntax[:, 74].tolist()))    # first_mb_in_slice of every macroblock's slice
    nals = [n for n in parseref.split_nals(access_unit) if n[0] & 31 in (1, 5)]
    assert len(nals) == len(firsts) and firsts[0] == 0, (len(nals), firsts)
    _count_mbs(c, p, coded)
    info = []
    for k, (m0, nal) in enumerate(zip(firsts, nals)):
        m1 = firsts[k + 1] if k + 1 < len(firsts) else nmb
        s = '_slice' if k else ''
        _count_pack(c, 'pack' + s, coded, m0, m1, int(p.syntax[m0, 1]) == 0)
        if mbh == 256:
            c[('pack' + s, 'mbh_256')] += 1
        if mbw == 512 and k == 0:
            c[('pack', 'mbw_512')] += 1
        info.append(_count_ep(c, 'ep' + s, nal[1:]))
    for k in [k for k in c if k not in want]:
        del c[k]
    c.info = (len(nals), [b for _, b in info], [a for a, _ in info])
    return c


def count_clip(units):
    """the classes of a clip's access units in order (empty ones, skipped frames, left out)"""
    state, total = parseref.State(), Counter()
    for u in units:
        if u:
            total.update(count(u, state))
    return total


# ---------------------------------------------------------------- classes no encoder output holds
_NO_PCM = 'the encoder never emits I_PCM (cavlc_code_mb writes mb_type from MI_I4 / MI_I16 / P16x16 only; the oracle has no PCM path)'
_NO_PART = ('the encoder searches one 16x16 vector per macroblock (cavlc_code_mb "lb_ue(b, 0); lb_se(b, Cm.mvd[0]); lb_se(b, Cm.mvd[1])"): '
            'P_L0_L0_16x8, P_L0_L0_8x16, P_8x8 and P_8x8ref0 are never written')
_ZERO32 = ('a second insertion inside one run needs 4 zero bytes, 32 zero bits in a row. The longest zero string of slice data is a '
           'level_suffix of 12 zero bits (or the <= 6 zero bits that end a total_zeros / run_before word) followed by the zero prefix '
           'of the next word: 15 for coeff_token and level_prefix, 17 for ue(mb_skip_run <= 131071), 4 per Intra4x4 mode with the next '
           'block\'s predicted mode then 0, so its flag is 1: at most 29 zero bits')
NOT_REACHED = {}
NOT_REACHED.update({('mb_type', 'I', 25): _NO_PCM, ('mb_type', 'P', 30): _NO_PCM, ('nC_neighbour', 'pcm'): _NO_PCM})
NOT_REACHED.update({('mb_type', 'P', n): _NO_PART for n in (1, 2, 3, 4)})
NOT_REACHED.update({(fam, 'ins_after_zero_run_4plus'): _ZERO32 for fam in ('ep', 'ep_slice')})
_QP_WINDOW = ('every QP of a frame lies in the frame\'s window (enc_begin_stream "r.min_frame_qp = clip3(12, 42, r.last_qscale - 3); '
              'r.max_frame_qp = clip3(12, 42, r.last_qscale + 5)", an IDR picture keeps one QP), so |mb_qp_delta| <= 8 and QPY + '
              'mb_qp_delta stays inside 0..51')
NOT_REACHED.update({('mb_qp_delta', k): _QP_WINDOW for k in ('-26', '+25', 'wrap')})
_TZ15 = 'a block of 15 coefficients has TotalCoeff + total_zeros <= 15 (7.3.5.3.2): the row does not exist for Intra16x16ACLevel / ChromaACLevel'
NOT_REACHED.update({('total_zeros', 15, tc, 16 - tc): _TZ15 for tc in range(1, 15)})
_TZ15_FULL = 'total_zeros is absent when TotalCoeff equals maxNumCoeff (cavlc_block "if (tc < maxnum)"), 15 in a block of 15'
NOT_REACHED.update({('total_zeros', 15, 15, tz): _TZ15_FULL for tz in (0, 1)})

_LONG_BLOCK = ('every QP is at least 12 (enc_begin_stream "clip3(12, 42, r.last_qscale - 3)", runtime_enc.inc clips the IDR range to 12..42), '
               'so outside the Intra16x16 DC block |level| <= 255 * 16 * 13107 >> 17 = 408 and the squares of a block\'s levels sum to at '
               'most 408^2: after five escapes of 28 bits (|level| >= 16, 31, 61, 121, 241 raise suffixLength to 6) the eleven levels left '
               'share 88804, 9 bits each, 255 bits with a 16-bit coeff_token. The DC block\'s sixteen levels are large together only when '
               'the sixteen 4x4 means differ widely, and then the Intra4x4 search (VAA variance above 149) has won in every clip coded: '
               'the longest block of 3200 directed 16x16 and 32x32 pictures of 0/255 cells at 400 Mbps has 221 bits')
NOT_REACHED[('block_bits', 'gt256')] = _LONG_BLOCK

# the classes of slice index > 0: counted on the GPU encoder's three-slice bytes only (the oracle encoder codes one slice)
SLICE_FAMILIES = ('pack_slice', 'ep_slice')


def is_slice_class(k):
    return k[0] in SLICE_FAMILIES or k == ('nC_neighbour', 'other_slice')


def required():
    return all_classes() - set(NOT_REACHED)


# ---------------------------------------------------------------- directed content
def _flat(w, h, v=128):
    return [np.full((h, w), v, np.uint8), np.full((h // 2, w // 2), 128, np.uint8), np.full((h // 2, w // 2), 128, np.uint8)]


def _noise_mb(p, rng, mbw, mb, lo, hi):
    x, y = mb % mbw * 16, mb // mbw * 16
    p[0][y:y + 16, x:x + 16] = rng.integers(lo, hi + 1, (16, 16))
    for k in (1, 2):
        p[k][y // 2:y // 2 + 8, x // 2:x // 2 + 8] = rng.integers(lo, hi + 1, (8, 8))


def tail_mbs(mbw, mbh, count_, nslices=(1, 3)):
    """`count_` macroblocks spread over the picture that lie in the tail of their thread range (offset >= PACK_MBT) with
    every slice count of `nslices` -- all of them when the picture has fewer"""
    nmb = mbw * mbh
    ok = np.ones(nmb, bool)
    for n in nslices:
        n = min(n, mbh)
        for k in range(n):
            m0, m1 = (k * mbh) // n * mbw, ((k + 1) * mbh) // n * mbw
            mg, per = thread_ranges(m0, m1)
            i = np.arange(m0, m1)
            ok[m0:m1] &= (i - mg) % per >= PACK_MBT
    idx = np.flatnonzero(ok)
    if idx.size <= count_:
        return idx.tolist()
    return idx[np.linspace(0, idx.size - 1, count_).astype(int)].tolist()


_AMPS = (0, 1, 2, 4, 8, 16, 32, 64, 127)


def mix_frame(rng, w, h, prev, keep):
    """every macroblock with a texture of its own: with probability `keep` the previous frame's (P_Skip, or a small
    residual), else a mean and, per 8x8 quadrant, a noise amplitude of _AMPS (0: the quadrant is flat and its
    coded_block_pattern bit mostly clear), and one amplitude for both chroma blocks"""
    if prev is None:
        p = _flat(w, h)
    else:
        p = [prev[:w * h].reshape(h, w).copy(), prev[w * h:w * h * 5 // 4].reshape(h // 2, w // 2).copy(),
             prev[w * h * 5 // 4:].reshape(h // 2, w // 2).copy()]
    for y in range(0, h - 15, 16):
        for x in range(0, w - 15, 16):
            if prev is not None and rng.random() < keep:
                continue
            mean = int(rng.integers(40, 216))
            for q in range(4):
                a = _AMPS[rng.integers(len(_AMPS))]
                qy, qx = y + 8 * (q >> 1), x + 8 * (q & 1)
                p[0][qy:qy + 8, qx:qx + 8] = np.clip(mean + rng.integers(-a, a + 1, (8, 8)), 0, 255)
            a = _AMPS[rng.integers(len(_AMPS))]
            for k in (1, 2):
                p[k][y // 2:y // 2 + 8, x // 2:x // 2 + 8] = np.clip(128 + rng.integers(-a, a + 1, (8, 8)), 0, 255)
    return p


def gen(kind, w, h, n, seed, **kw):
    """n frames of content for the writer:
    noise     uniform noise lo..hi, fresh every frame
    checker   every sample 0 or 255, fresh every frame
    blocks    cells of `cell` x `cell` luma samples, each 0 or 255, chroma co-sited (Cr inverted), fresh every frame
    patches   a flat picture; every `every`-th macroblock (default: tail_mbs(count)) carries fresh noise lo..hi in every frame, the
              rest never changes (P_Skip from frame 1 on)
    still     noise in frame 0, every later frame equal to it where `hold` says so: hold='all' repeats frame 0, hold=k
              re-draws only the first k macroblocks
    """
    rng = np.random.default_rng(seed)
    lo, hi = kw.get('lo', 0), kw.get('hi', 255)
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    out = []
    for t in range(n):
        if kind == 'noise':
            p = [rng.integers(lo, hi + 1, s) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
        elif kind == 'checker':
            p = [rng.integers(0, 2, s) * 255 for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
        elif kind == 'patches':
            p = _flat(w, h)
            mbs = range(0, mbw * mbh, kw['every']) if 'every' in kw else tail_mbs(mbw, mbh, kw.get('count', 24))
            for mb in mbs:
                _noise_mb(p, rng, mbw, mb, lo, hi)
        elif kind == 'still':
            if t == 0:
                first = [rng.integers(lo, hi + 1, s) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
            p = [a.copy() for a in first]
            if kw.get('hold') != 'all':
                for mb in range(kw['hold']):
                    _noise_mb(p, rng, mbw, mb, lo, hi)
        elif kind == 'blocks':
            cell = kw.get('cell', 8)
            blk = rng.integers(0, 2, (h // cell, w // cell)) * 255
            y = np.repeat(np.repeat(blk, cell, 0), cell, 1)
            c = y[::2, ::2]
            p = [y, c, 255 - c]
        elif kind == 'mix':
            p = mix_frame(rng, w, h, out[-1] if out else None, kw.get('keep', 0.3))
        else:
            raise ValueError(kind)
        out.append(encaudit.pack(p))
    return out


def spec_clip(spec, targets=(), slice_targets=()):
    """(kind, w, h, frames, seed, bitrate, frames forced to IDR, content keywords) -> encaudit.Clip"""
    kind, w, h, n, seed, br, idr, kw = spec
    name = f'{kind}_{w}x{h}_s{seed}_{br}' + ('_idr' + ''.join(str(t) for t in idr) if idr else '') + ''.join(f'_{k}{v}' for k, v in sorted(kw.items()))
    c = encaudit.Clip(name, w, h, br, gen(kind, w, h, n, seed, **kw), idr=idr, targets=targets)
    c.slice_targets = tuple(slice_targets)
    c.spec = spec
    return c


def slices_for(clip, n):
    """the slice count a clip is coded with when the test asks for n: a slice is at least one MB row"""
    return min(n, (clip.h + 15) // 16)


# (kind, w, h, frames, seed, bitrate, frames forced to IDR, content keywords) and the classes the clip is in the set for,
# one family per line. The large and the extreme geometries and the static clip come first and claim the packer classes
# they are built for; every other class goes to the clip of 48x32 .. 176x144 that adds most classes (a clip that
# fits a batch already in the set is preferred), chosen from ~2100 seeded candidates (noise, 0/255 checker and cells,
# mix; 20 kbps .. 400 Mbps) run through the oracle; the checker clip after them is the first of 40000 seeds whose
# insertion's zero run starts in the 16 KiB chunk before. The 256x192 noise clips are there for slice index > 0 alone
# (SLICE_TARGETS): the first seeds whose three-slice bytes reach the class.
DIRECTED = [
    (('patches', 3072, 2160, 3, 1, 20000000, (), {'count': 24}), [
     ('pack', 'per_gt32'), ('pack', 'range_no_coded_mb'), ('pack', 'skip_run_from_earlier_range'),
     ('pack', 'tail_coded_mb'), ('pack', 'trailing_run'),
    ]),
    (('patches', 16, 4096, 3, 1, 3000000, (), {'every': 5}), [
     ('pack', 'mbh_256'),
    ]),
    (('patches', 8192, 16, 3, 1, 3000000, (), {'every': 7}), [
     ('pack', 'mbw_512'),
    ]),
    (('still', 48, 32, 3, 1, 300000, (), {'hold': 'all'}), [
     ('pack', 'no_coded_mb'),
    ]),
    (('mix', 176, 144, 4, 5, 100000, (), {}), [
     ('block_bits', 'gt32'), ('block_bits', 'mult32'),
     ('block_offset', 'mod32_0'),
     ('cbp_codeNum', 'inter', 0), ('cbp_codeNum', 'inter', 10), ('cbp_codeNum', 'inter', 11), ('cbp_codeNum', 'inter', 12),
     ('cbp_codeNum', 'inter', 13), ('cbp_codeNum', 'inter', 14), ('cbp_codeNum', 'inter', 17),
     ('cbp_codeNum', 'inter', 18), ('cbp_codeNum', 'inter', 20), ('cbp_codeNum', 'inter', 21),
     ('cbp_codeNum', 'inter', 22), ('cbp_codeNum', 'inter', 23), ('cbp_codeNum', 'inter', 24),
     ('cbp_codeNum', 'inter', 25), ('cbp_codeNum', 'inter', 26), ('cbp_codeNum', 'inter', 27),
     ('cbp_codeNum', 'inter', 28), ('cbp_codeNum', 'inter', 29), ('cbp_codeNum', 'inter', 3), ('cbp_codeNum', 'inter', 30),
     ('cbp_codeNum', 'inter', 31), ('cbp_codeNum', 'inter', 4), ('cbp_codeNum', 'inter', 46), ('cbp_codeNum', 'inter', 47),
     ('cbp_codeNum', 'inter', 5), ('cbp_codeNum', 'inter', 6), ('cbp_codeNum', 'inter', 7), ('cbp_codeNum', 'inter', 8),
     ('cbp_codeNum', 'inter', 9), ('cbp_codeNum', 'intra', 0), ('cbp_codeNum', 'intra', 1), ('cbp_codeNum', 'intra', 10),
     ('cbp_codeNum', 'intra', 12), ('cbp_codeNum', 'intra', 13), ('cbp_codeNum', 'intra', 14),
     ('cbp_codeNum', 'intra', 15), ('cbp_codeNum', 'intra', 17), ('cbp_codeNum', 'intra', 18), ('cbp_codeNum', 'intra', 2),
     ('cbp_codeNum', 'intra', 21), ('cbp_codeNum', 'intra', 22), ('cbp_codeNum', 'intra', 25),
     ('cbp_codeNum', 'intra', 26), ('cbp_codeNum', 'intra', 27), ('cbp_codeNum', 'intra', 31),
     ('cbp_codeNum', 'intra', 37), ('cbp_codeNum', 'intra', 38), ('cbp_codeNum', 'intra', 4), ('cbp_codeNum', 'intra', 40),
     ('cbp_codeNum', 'intra', 44), ('cbp_codeNum', 'intra', 45), ('cbp_codeNum', 'intra', 47), ('cbp_codeNum', 'intra', 5),
     ('cbp_codeNum', 'intra', 6), ('cbp_codeNum', 'intra', 8),
     ('coeff_token', '0-1', 0, 0), ('coeff_token', '0-1', 1, 0), ('coeff_token', '0-1', 1, 1),
     ('coeff_token', '0-1', 10, 0), ('coeff_token', '0-1', 10, 1), ('coeff_token', '0-1', 10, 2),
     ('coeff_token', '0-1', 10, 3), ('coeff_token', '0-1', 11, 0), ('coeff_token', '0-1', 11, 1),
     ('coeff_token', '0-1', 11, 2), ('coeff_token', '0-1', 11, 3), ('coeff_token', '0-1', 12, 0),
     ('coeff_token', '0-1', 12, 1), ('coeff_token', '0-1', 12, 3), ('coeff_token', '0-1', 13, 0),
     ('coeff_token', '0-1', 13, 1), ('coeff_token', '0-1', 13, 2), ('coeff_token', '0-1', 13, 3),
     ('coeff_token', '0-1', 14, 0), ('coeff_token', '0-1', 14, 1), ('coeff_token', '0-1', 14, 2),
     ('coeff_token', '0-1', 14, 3), ('coeff_token', '0-1', 15, 0), ('coeff_token', '0-1', 15, 1),
     ('coeff_token', '0-1', 16, 0), ('coeff_token', '0-1', 2, 0), ('coeff_token', '0-1', 2, 1),
     ('coeff_token', '0-1', 2, 2), ('coeff_token', '0-1', 3, 0), ('coeff_token', '0-1', 3, 1),
     ('coeff_token', '0-1', 3, 2), ('coeff_token', '0-1', 3, 3), ('coeff_token', '0-1', 4, 0),
     ('coeff_token', '0-1', 4, 1), ('coeff_token', '0-1', 4, 2), ('coeff_token', '0-1', 4, 3),
     ('coeff_token', '0-1', 5, 0), ('coeff_token', '0-1', 5, 1), ('coeff_token', '0-1', 5, 2),
     ('coeff_token', '0-1', 5, 3), ('coeff_token', '0-1', 6, 0), ('coeff_token', '0-1', 6, 1),
     ('coeff_token', '0-1', 6, 2), ('coeff_token', '0-1', 6, 3), ('coeff_token', '0-1', 7, 0),
     ('coeff_token', '0-1', 7, 1), ('coeff_token', '0-1', 7, 2), ('coeff_token', '0-1', 7, 3),
     ('coeff_token', '0-1', 8, 0), ('coeff_token', '0-1', 8, 1), ('coeff_token', '0-1', 8, 2),
     ('coeff_token', '0-1', 8, 3), ('coeff_token', '0-1', 9, 0), ('coeff_token', '0-1', 9, 1),
     ('coeff_token', '0-1', 9, 2), ('coeff_token', '0-1', 9, 3), ('coeff_token', '2-3', 0, 0),
     ('coeff_token', '2-3', 1, 0), ('coeff_token', '2-3', 1, 1), ('coeff_token', '2-3', 10, 0),
     ('coeff_token', '2-3', 10, 1), ('coeff_token', '2-3', 10, 3), ('coeff_token', '2-3', 11, 0),
     ('coeff_token', '2-3', 11, 1), ('coeff_token', '2-3', 11, 2), ('coeff_token', '2-3', 11, 3),
     ('coeff_token', '2-3', 12, 0), ('coeff_token', '2-3', 12, 1), ('coeff_token', '2-3', 12, 3),
     ('coeff_token', '2-3', 13, 0), ('coeff_token', '2-3', 13, 1), ('coeff_token', '2-3', 14, 0),
     ('coeff_token', '2-3', 14, 1), ('coeff_token', '2-3', 15, 0), ('coeff_token', '2-3', 2, 0),
     ('coeff_token', '2-3', 2, 1), ('coeff_token', '2-3', 2, 2), ('coeff_token', '2-3', 3, 0),
     ('coeff_token', '2-3', 3, 1), ('coeff_token', '2-3', 3, 2), ('coeff_token', '2-3', 3, 3),
     ('coeff_token', '2-3', 4, 0), ('coeff_token', '2-3', 4, 1), ('coeff_token', '2-3', 4, 2),
     ('coeff_token', '2-3', 4, 3), ('coeff_token', '2-3', 5, 0), ('coeff_token', '2-3', 5, 1),
     ('coeff_token', '2-3', 5, 2), ('coeff_token', '2-3', 5, 3), ('coeff_token', '2-3', 6, 0),
     ('coeff_token', '2-3', 6, 1), ('coeff_token', '2-3', 6, 2), ('coeff_token', '2-3', 6, 3),
     ('coeff_token', '2-3', 7, 0), ('coeff_token', '2-3', 7, 1), ('coeff_token', '2-3', 7, 2),
     ('coeff_token', '2-3', 7, 3), ('coeff_token', '2-3', 8, 0), ('coeff_token', '2-3', 8, 1),
     ('coeff_token', '2-3', 8, 2), ('coeff_token', '2-3', 8, 3), ('coeff_token', '2-3', 9, 0),
     ('coeff_token', '2-3', 9, 1), ('coeff_token', '2-3', 9, 2), ('coeff_token', '2-3', 9, 3),
     ('coeff_token', '4-7', 0, 0), ('coeff_token', '4-7', 1, 0), ('coeff_token', '4-7', 1, 1),
     ('coeff_token', '4-7', 10, 0), ('coeff_token', '4-7', 10, 1), ('coeff_token', '4-7', 10, 2),
     ('coeff_token', '4-7', 10, 3), ('coeff_token', '4-7', 11, 0), ('coeff_token', '4-7', 11, 1),
     ('coeff_token', '4-7', 11, 2), ('coeff_token', '4-7', 11, 3), ('coeff_token', '4-7', 12, 0),
     ('coeff_token', '4-7', 12, 1), ('coeff_token', '4-7', 12, 2), ('coeff_token', '4-7', 12, 3),
     ('coeff_token', '4-7', 13, 0), ('coeff_token', '4-7', 13, 1), ('coeff_token', '4-7', 13, 2),
     ('coeff_token', '4-7', 13, 3), ('coeff_token', '4-7', 14, 0), ('coeff_token', '4-7', 14, 1),
     ('coeff_token', '4-7', 14, 2), ('coeff_token', '4-7', 14, 3), ('coeff_token', '4-7', 15, 0),
     ('coeff_token', '4-7', 15, 3), ('coeff_token', '4-7', 16, 0), ('coeff_token', '4-7', 2, 0),
     ('coeff_token', '4-7', 2, 1), ('coeff_token', '4-7', 2, 2), ('coeff_token', '4-7', 3, 0),
     ('coeff_token', '4-7', 3, 1), ('coeff_token', '4-7', 3, 2), ('coeff_token', '4-7', 3, 3),
     ('coeff_token', '4-7', 4, 0), ('coeff_token', '4-7', 4, 1), ('coeff_token', '4-7', 4, 2),
     ('coeff_token', '4-7', 4, 3), ('coeff_token', '4-7', 5, 0), ('coeff_token', '4-7', 5, 1),
     ('coeff_token', '4-7', 5, 2), ('coeff_token', '4-7', 5, 3), ('coeff_token', '4-7', 6, 0),
     ('coeff_token', '4-7', 6, 1), ('coeff_token', '4-7', 6, 2), ('coeff_token', '4-7', 6, 3),
     ('coeff_token', '4-7', 7, 0), ('coeff_token', '4-7', 7, 1), ('coeff_token', '4-7', 7, 2),
     ('coeff_token', '4-7', 7, 3), ('coeff_token', '4-7', 8, 0), ('coeff_token', '4-7', 8, 1),
     ('coeff_token', '4-7', 8, 2), ('coeff_token', '4-7', 8, 3), ('coeff_token', '4-7', 9, 0),
     ('coeff_token', '4-7', 9, 1), ('coeff_token', '4-7', 9, 2), ('coeff_token', '4-7', 9, 3), ('coeff_token', '8+', 0, 0),
     ('coeff_token', '8+', 1, 0), ('coeff_token', '8+', 1, 1), ('coeff_token', '8+', 10, 0), ('coeff_token', '8+', 10, 1),
     ('coeff_token', '8+', 10, 2), ('coeff_token', '8+', 10, 3), ('coeff_token', '8+', 11, 0),
     ('coeff_token', '8+', 11, 1), ('coeff_token', '8+', 11, 2), ('coeff_token', '8+', 11, 3),
     ('coeff_token', '8+', 12, 0), ('coeff_token', '8+', 12, 1), ('coeff_token', '8+', 12, 2),
     ('coeff_token', '8+', 12, 3), ('coeff_token', '8+', 13, 0), ('coeff_token', '8+', 13, 1),
     ('coeff_token', '8+', 13, 2), ('coeff_token', '8+', 13, 3), ('coeff_token', '8+', 14, 0),
     ('coeff_token', '8+', 14, 1), ('coeff_token', '8+', 14, 2), ('coeff_token', '8+', 14, 3),
     ('coeff_token', '8+', 15, 0), ('coeff_token', '8+', 15, 1), ('coeff_token', '8+', 15, 3), ('coeff_token', '8+', 2, 0),
     ('coeff_token', '8+', 2, 1), ('coeff_token', '8+', 2, 2), ('coeff_token', '8+', 3, 0), ('coeff_token', '8+', 3, 1),
     ('coeff_token', '8+', 3, 2), ('coeff_token', '8+', 3, 3), ('coeff_token', '8+', 4, 0), ('coeff_token', '8+', 4, 1),
     ('coeff_token', '8+', 4, 2), ('coeff_token', '8+', 4, 3), ('coeff_token', '8+', 5, 0), ('coeff_token', '8+', 5, 1),
     ('coeff_token', '8+', 5, 2), ('coeff_token', '8+', 5, 3), ('coeff_token', '8+', 6, 0), ('coeff_token', '8+', 6, 1),
     ('coeff_token', '8+', 6, 2), ('coeff_token', '8+', 6, 3), ('coeff_token', '8+', 7, 0), ('coeff_token', '8+', 7, 1),
     ('coeff_token', '8+', 7, 2), ('coeff_token', '8+', 7, 3), ('coeff_token', '8+', 8, 0), ('coeff_token', '8+', 8, 1),
     ('coeff_token', '8+', 8, 2), ('coeff_token', '8+', 8, 3), ('coeff_token', '8+', 9, 0), ('coeff_token', '8+', 9, 1),
     ('coeff_token', '8+', 9, 2), ('coeff_token', '8+', 9, 3), ('coeff_token', 'dc', 0, 0), ('coeff_token', 'dc', 1, 0),
     ('coeff_token', 'dc', 1, 1), ('coeff_token', 'dc', 2, 0), ('coeff_token', 'dc', 2, 1), ('coeff_token', 'dc', 2, 2),
     ('coeff_token', 'dc', 3, 0), ('coeff_token', 'dc', 3, 1), ('coeff_token', 'dc', 3, 2), ('coeff_token', 'dc', 3, 3),
     ('coeff_token', 'dc', 4, 0), ('coeff_token', 'dc', 4, 1), ('coeff_token', 'dc', 4, 2), ('coeff_token', 'dc', 4, 3),
     ('level_escape', 'prefix14_suffixLength0'), ('level_escape', 'prefix15_plain'), ('level_escape', 'prefix15_plus15'),
     ('level_first_minus2',),
     ('level_threshold', 0, 'above'), ('level_threshold', 0, 'at'), ('level_threshold', 1, 'above'),
     ('level_threshold', 1, 'at'), ('level_threshold', 2, 'above'), ('level_threshold', 2, 'at'),
     ('mb_bits', 'gt128'), ('mb_bits', 'le128'), ('mb_bits', 'mult32'),
     ('mb_skip_run', 'ends_slice'), ('mb_skip_run', 'spans_row_end'), ('mb_skip_run', 'zero'),
     ('mb_start', 'mod32_0'),
     ('mb_type', 'I', 0), ('mb_type', 'I', 11), ('mb_type', 'I', 12), ('mb_type', 'I', 13), ('mb_type', 'I', 14),
     ('mb_type', 'I', 15), ('mb_type', 'I', 16), ('mb_type', 'I', 17), ('mb_type', 'I', 18), ('mb_type', 'I', 19),
     ('mb_type', 'I', 2), ('mb_type', 'I', 20), ('mb_type', 'I', 21), ('mb_type', 'I', 22), ('mb_type', 'I', 23),
     ('mb_type', 'I', 24), ('mb_type', 'I', 3), ('mb_type', 'I', 5), ('mb_type', 'P', 0), ('mb_type', 'P', 10),
     ('mb_type', 'P', 11), ('mb_type', 'P', 12), ('mb_type', 'P', 15), ('mb_type', 'P', 18), ('mb_type', 'P', 19),
     ('mb_type', 'P', 20), ('mb_type', 'P', 21), ('mb_type', 'P', 22), ('mb_type', 'P', 23), ('mb_type', 'P', 24),
     ('mb_type', 'P', 25), ('mb_type', 'P', 26), ('mb_type', 'P', 27), ('mb_type', 'P', 28), ('mb_type', 'P', 29),
     ('mb_type', 'P', 5), ('mb_type', 'P', 6), ('mb_type', 'P', 7), ('mb_type', 'P', 8), ('mb_type', 'P', 9),
     ('nC', 'cb_ac', 'both'), ('nC', 'cb_ac', 'left'), ('nC', 'cb_ac', 'neither'), ('nC', 'cb_ac', 'upper'),
     ('nC', 'cr_ac', 'both'), ('nC', 'cr_ac', 'left'), ('nC', 'cr_ac', 'neither'), ('nC', 'cr_ac', 'upper'),
     ('nC', 'i16ac', 'both'), ('nC', 'i16ac', 'left'), ('nC', 'i16ac', 'neither'), ('nC', 'i16ac', 'upper'),
     ('nC', 'i16dc', 'both'), ('nC', 'i16dc', 'left'), ('nC', 'i16dc', 'neither'), ('nC', 'i16dc', 'upper'),
     ('nC', 'luma', 'both'), ('nC', 'luma', 'left'), ('nC', 'luma', 'neither'), ('nC', 'luma', 'upper'),
     ('nC_neighbour', 'cbp_clear'), ('nC_neighbour', 'i16_no_ac'), ('nC_neighbour', 'skipped'),
     ('run_before', 'last_takes_remainder'), ('run_before', 'zeros_exhausted'), ('run_before', 1, 0), ('run_before', 1, 1),
     ('run_before', 2, 0), ('run_before', 2, 1), ('run_before', 2, 2), ('run_before', 3, 0), ('run_before', 3, 1),
     ('run_before', 3, 2), ('run_before', 3, 3), ('run_before', 4, 0), ('run_before', 4, 1), ('run_before', 4, 2),
     ('run_before', 4, 3), ('run_before', 4, 4), ('run_before', 5, 0), ('run_before', 5, 1), ('run_before', 5, 2),
     ('run_before', 5, 3), ('run_before', 5, 4), ('run_before', 5, 5), ('run_before', 6, 0), ('run_before', 6, 1),
     ('run_before', 6, 2), ('run_before', 6, 3), ('run_before', 6, 4), ('run_before', 6, 5), ('run_before', 6, 6),
     ('run_before', 7, 0), ('run_before', 7, 1), ('run_before', 7, 10), ('run_before', 7, 11), ('run_before', 7, 12),
     ('run_before', 7, 13), ('run_before', 7, 14), ('run_before', 7, 2), ('run_before', 7, 3), ('run_before', 7, 4),
     ('run_before', 7, 5), ('run_before', 7, 6), ('run_before', 7, 7), ('run_before', 7, 8), ('run_before', 7, 9),
     ('suffixLength_inc', 0), ('suffixLength_inc', 1), ('suffixLength_inc', 2),
     ('suffixLength_init', 1),
     ('total_zeros', 15, 1, 0), ('total_zeros', 15, 1, 1), ('total_zeros', 15, 1, 10), ('total_zeros', 15, 1, 11),
     ('total_zeros', 15, 1, 12), ('total_zeros', 15, 1, 13), ('total_zeros', 15, 1, 14), ('total_zeros', 15, 1, 2),
     ('total_zeros', 15, 1, 3), ('total_zeros', 15, 1, 4), ('total_zeros', 15, 1, 5), ('total_zeros', 15, 1, 6),
     ('total_zeros', 15, 1, 7), ('total_zeros', 15, 1, 8), ('total_zeros', 15, 1, 9), ('total_zeros', 15, 10, 2),
     ('total_zeros', 15, 10, 3), ('total_zeros', 15, 10, 4), ('total_zeros', 15, 10, 5), ('total_zeros', 15, 11, 1),
     ('total_zeros', 15, 11, 2), ('total_zeros', 15, 11, 3), ('total_zeros', 15, 11, 4), ('total_zeros', 15, 12, 0),
     ('total_zeros', 15, 12, 1), ('total_zeros', 15, 12, 2), ('total_zeros', 15, 12, 3), ('total_zeros', 15, 13, 1),
     ('total_zeros', 15, 13, 2), ('total_zeros', 15, 14, 0), ('total_zeros', 15, 14, 1), ('total_zeros', 15, 2, 1),
     ('total_zeros', 15, 2, 10), ('total_zeros', 15, 2, 11), ('total_zeros', 15, 2, 12), ('total_zeros', 15, 2, 13),
     ('total_zeros', 15, 2, 2), ('total_zeros', 15, 2, 3), ('total_zeros', 15, 2, 4), ('total_zeros', 15, 2, 5),
     ('total_zeros', 15, 2, 6), ('total_zeros', 15, 2, 7), ('total_zeros', 15, 2, 8), ('total_zeros', 15, 2, 9),
     ('total_zeros', 15, 3, 1), ('total_zeros', 15, 3, 10), ('total_zeros', 15, 3, 11), ('total_zeros', 15, 3, 12),
     ('total_zeros', 15, 3, 2), ('total_zeros', 15, 3, 3), ('total_zeros', 15, 3, 4), ('total_zeros', 15, 3, 5),
     ('total_zeros', 15, 3, 6), ('total_zeros', 15, 3, 7), ('total_zeros', 15, 3, 8), ('total_zeros', 15, 3, 9),
     ('total_zeros', 15, 4, 10), ('total_zeros', 15, 4, 11), ('total_zeros', 15, 4, 2), ('total_zeros', 15, 4, 3),
     ('total_zeros', 15, 4, 4), ('total_zeros', 15, 4, 5), ('total_zeros', 15, 4, 6), ('total_zeros', 15, 4, 7),
     ('total_zeros', 15, 4, 8), ('total_zeros', 15, 4, 9), ('total_zeros', 15, 5, 10), ('total_zeros', 15, 5, 4),
     ('total_zeros', 15, 5, 5), ('total_zeros', 15, 5, 6), ('total_zeros', 15, 5, 7), ('total_zeros', 15, 5, 8),
     ('total_zeros', 15, 5, 9), ('total_zeros', 15, 6, 1), ('total_zeros', 15, 6, 3), ('total_zeros', 15, 6, 4),
     ('total_zeros', 15, 6, 5), ('total_zeros', 15, 6, 6), ('total_zeros', 15, 6, 7), ('total_zeros', 15, 6, 8),
     ('total_zeros', 15, 6, 9), ('total_zeros', 15, 7, 2), ('total_zeros', 15, 7, 3), ('total_zeros', 15, 7, 4),
     ('total_zeros', 15, 7, 5), ('total_zeros', 15, 7, 6), ('total_zeros', 15, 7, 7), ('total_zeros', 15, 7, 8),
     ('total_zeros', 15, 8, 3), ('total_zeros', 15, 8, 4), ('total_zeros', 15, 8, 5), ('total_zeros', 15, 8, 6),
     ('total_zeros', 15, 8, 7), ('total_zeros', 15, 9, 2), ('total_zeros', 15, 9, 4), ('total_zeros', 15, 9, 5),
     ('total_zeros', 15, 9, 6), ('total_zeros', 16, 1, 0), ('total_zeros', 16, 1, 1), ('total_zeros', 16, 1, 10),
     ('total_zeros', 16, 1, 11), ('total_zeros', 16, 1, 12), ('total_zeros', 16, 1, 13), ('total_zeros', 16, 1, 14),
     ('total_zeros', 16, 1, 15), ('total_zeros', 16, 1, 2), ('total_zeros', 16, 1, 3), ('total_zeros', 16, 1, 4),
     ('total_zeros', 16, 1, 5), ('total_zeros', 16, 1, 6), ('total_zeros', 16, 1, 7), ('total_zeros', 16, 1, 8),
     ('total_zeros', 16, 1, 9), ('total_zeros', 16, 10, 2), ('total_zeros', 16, 10, 3), ('total_zeros', 16, 10, 4),
     ('total_zeros', 16, 10, 5), ('total_zeros', 16, 10, 6), ('total_zeros', 16, 11, 1), ('total_zeros', 16, 11, 2),
     ('total_zeros', 16, 11, 3), ('total_zeros', 16, 11, 4), ('total_zeros', 16, 11, 5), ('total_zeros', 16, 12, 1),
     ('total_zeros', 16, 12, 2), ('total_zeros', 16, 12, 3), ('total_zeros', 16, 12, 4), ('total_zeros', 16, 13, 2),
     ('total_zeros', 16, 13, 3), ('total_zeros', 16, 14, 1), ('total_zeros', 16, 14, 2), ('total_zeros', 16, 15, 0),
     ('total_zeros', 16, 15, 1), ('total_zeros', 16, 2, 0), ('total_zeros', 16, 2, 1), ('total_zeros', 16, 2, 10),
     ('total_zeros', 16, 2, 11), ('total_zeros', 16, 2, 12), ('total_zeros', 16, 2, 13), ('total_zeros', 16, 2, 14),
     ('total_zeros', 16, 2, 2), ('total_zeros', 16, 2, 3), ('total_zeros', 16, 2, 4), ('total_zeros', 16, 2, 5),
     ('total_zeros', 16, 2, 6), ('total_zeros', 16, 2, 7), ('total_zeros', 16, 2, 8), ('total_zeros', 16, 2, 9),
     ('total_zeros', 16, 3, 0), ('total_zeros', 16, 3, 1), ('total_zeros', 16, 3, 10), ('total_zeros', 16, 3, 11),
     ('total_zeros', 16, 3, 12), ('total_zeros', 16, 3, 13), ('total_zeros', 16, 3, 2), ('total_zeros', 16, 3, 3),
     ('total_zeros', 16, 3, 4), ('total_zeros', 16, 3, 5), ('total_zeros', 16, 3, 6), ('total_zeros', 16, 3, 7),
     ('total_zeros', 16, 3, 8), ('total_zeros', 16, 3, 9), ('total_zeros', 16, 4, 1), ('total_zeros', 16, 4, 10),
     ('total_zeros', 16, 4, 11), ('total_zeros', 16, 4, 12), ('total_zeros', 16, 4, 2), ('total_zeros', 16, 4, 3),
     ('total_zeros', 16, 4, 4), ('total_zeros', 16, 4, 5), ('total_zeros', 16, 4, 6), ('total_zeros', 16, 4, 7),
     ('total_zeros', 16, 4, 8), ('total_zeros', 16, 4, 9), ('total_zeros', 16, 5, 10), ('total_zeros', 16, 5, 11),
     ('total_zeros', 16, 5, 2), ('total_zeros', 16, 5, 3), ('total_zeros', 16, 5, 4), ('total_zeros', 16, 5, 5),
     ('total_zeros', 16, 5, 6), ('total_zeros', 16, 5, 7), ('total_zeros', 16, 5, 8), ('total_zeros', 16, 5, 9),
     ('total_zeros', 16, 6, 10), ('total_zeros', 16, 6, 2), ('total_zeros', 16, 6, 3), ('total_zeros', 16, 6, 4),
     ('total_zeros', 16, 6, 5), ('total_zeros', 16, 6, 6), ('total_zeros', 16, 6, 7), ('total_zeros', 16, 6, 8),
     ('total_zeros', 16, 6, 9), ('total_zeros', 16, 7, 3), ('total_zeros', 16, 7, 4), ('total_zeros', 16, 7, 5),
     ('total_zeros', 16, 7, 6), ('total_zeros', 16, 7, 7), ('total_zeros', 16, 7, 8), ('total_zeros', 16, 7, 9),
     ('total_zeros', 16, 8, 3), ('total_zeros', 16, 8, 4), ('total_zeros', 16, 8, 5), ('total_zeros', 16, 8, 6),
     ('total_zeros', 16, 8, 7), ('total_zeros', 16, 8, 8), ('total_zeros', 16, 9, 2), ('total_zeros', 16, 9, 4),
     ('total_zeros', 16, 9, 5), ('total_zeros', 16, 9, 6), ('total_zeros', 16, 9, 7),
     ('total_zeros_absent', 15), ('total_zeros_absent', 16), ('total_zeros_absent', 4),
     ('total_zeros_dc', 1, 0), ('total_zeros_dc', 1, 1), ('total_zeros_dc', 1, 2), ('total_zeros_dc', 1, 3),
     ('total_zeros_dc', 2, 0), ('total_zeros_dc', 2, 1), ('total_zeros_dc', 2, 2), ('total_zeros_dc', 3, 0),
     ('total_zeros_dc', 3, 1),
     ('trailing_ones', 1), ('trailing_ones', 2), ('trailing_ones', 3),
     ('trailing_ones_sign', 1, '+'), ('trailing_ones_sign', 1, '-'), ('trailing_ones_sign', 2, '+'),
     ('trailing_ones_sign', 2, '-'), ('trailing_ones_sign', 3, '+'), ('trailing_ones_sign', 3, '-'),
    ]),
    (('mix', 176, 144, 4, 12, 100000, (), {}), [
     ('cbp_codeNum', 'inter', 15), ('cbp_codeNum', 'inter', 16), ('cbp_codeNum', 'inter', 2), ('cbp_codeNum', 'intra', 7),
     ('cbp_codeNum', 'intra', 9),
     ('coeff_token', '0-1', 12, 2), ('coeff_token', '0-1', 15, 3), ('coeff_token', '2-3', 10, 2),
     ('coeff_token', '2-3', 12, 2), ('coeff_token', '2-3', 13, 3), ('coeff_token', '2-3', 14, 3),
     ('coeff_token', '2-3', 15, 1), ('coeff_token', '4-7', 15, 1), ('coeff_token', '4-7', 15, 2),
     ('coeff_token', '4-7', 16, 2), ('coeff_token', '8+', 15, 2),
     ('level_threshold', 3, 'at'),
     ('mb_type', 'I', 10), ('mb_type', 'I', 7), ('mb_type', 'I', 9), ('mb_type', 'P', 13), ('mb_type', 'P', 16),
     ('mb_type', 'P', 17),
     ('suffixLength_inc', 3),
     ('total_zeros', 15, 11, 0), ('total_zeros', 15, 13, 0), ('total_zeros', 15, 2, 0), ('total_zeros', 15, 3, 0),
     ('total_zeros', 15, 5, 2), ('total_zeros', 15, 5, 3), ('total_zeros', 15, 6, 2), ('total_zeros', 15, 8, 2),
     ('total_zeros', 15, 9, 3), ('total_zeros', 16, 11, 0), ('total_zeros', 16, 4, 0), ('total_zeros', 16, 5, 0),
     ('total_zeros', 16, 6, 1), ('total_zeros', 16, 7, 2), ('total_zeros', 16, 9, 3),
    ]),
    (('mix', 176, 144, 4, 15, 100000, (), {}), [
     ('cbp_codeNum', 'intra', 29), ('cbp_codeNum', 'intra', 35), ('cbp_codeNum', 'intra', 41),
     ('coeff_token', '2-3', 13, 2), ('coeff_token', '8+', 16, 0),
     ('mb_type', 'I', 1), ('mb_type', 'I', 4),
     ('total_zeros', 15, 4, 1), ('total_zeros', 15, 7, 0), ('total_zeros', 15, 7, 1), ('total_zeros', 15, 9, 0),
     ('total_zeros', 15, 9, 1), ('total_zeros', 16, 13, 0), ('total_zeros', 16, 13, 1), ('total_zeros', 16, 5, 1),
     ('total_zeros', 16, 8, 2),
    ]),
    (('checker', 48, 32, 3, 8, 300000, (), {}), [
     ('coeff_token', '8+', 16, 1), ('coeff_token', '8+', 16, 2), ('coeff_token', '8+', 16, 3),
     ('level_threshold', 3, 'above'), ('level_threshold', 4, 'above'), ('level_threshold', 4, 'at'),
     ('level_threshold', 5, 'above'), ('level_threshold', 5, 'at'),
     ('suffixLength_inc', 4), ('suffixLength_inc', 5),
     ('total_zeros', 16, 14, 0),
    ]),
    (('mix', 176, 144, 4, 1, 100000, (), {}), [
     ('cbp_codeNum', 'inter', 1), ('cbp_codeNum', 'intra', 30), ('cbp_codeNum', 'intra', 32), ('cbp_codeNum', 'intra', 33),
     ('cbp_codeNum', 'intra', 42), ('cbp_codeNum', 'intra', 46),
     ('coeff_token', '2-3', 14, 2),
     ('mb_type', 'I', 8), ('mb_type', 'P', 14),
     ('total_zeros', 15, 10, 1), ('total_zeros', 15, 8, 1),
    ]),
    (('blocks', 48, 32, 3, 0, 300000, (), {'cell': 8}), [
     ('cbp_codeNum', 'inter', 32), ('cbp_codeNum', 'inter', 34), ('cbp_codeNum', 'inter', 35),
     ('cbp_codeNum', 'inter', 37), ('cbp_codeNum', 'inter', 39), ('cbp_codeNum', 'intra', 23),
     ('cbp_codeNum', 'intra', 34), ('cbp_codeNum', 'intra', 36),
    ]),
    (('mix', 176, 144, 4, 9, 100000, (), {}), [
     ('cbp_codeNum', 'inter', 42), ('cbp_codeNum', 'intra', 11), ('cbp_codeNum', 'intra', 19),
     ('cbp_codeNum', 'intra', 20),
     ('total_zeros', 15, 4, 0), ('total_zeros', 15, 5, 1),
    ]),
    (('mix', 176, 144, 4, 13, 100000, (), {}), [
     ('cbp_codeNum', 'intra', 28), ('cbp_codeNum', 'intra', 43),
     ('coeff_token', '4-7', 16, 1),
     ('total_zeros', 16, 10, 1), ('total_zeros', 16, 7, 1), ('total_zeros', 16, 9, 1),
    ]),
    (('mix', 176, 144, 4, 13, 10000000, (), {}), [
     ('cbp_codeNum', 'inter', 19), ('cbp_codeNum', 'inter', 41), ('cbp_codeNum', 'inter', 43),
     ('coeff_token', '0-1', 15, 2), ('coeff_token', '0-1', 16, 2), ('coeff_token', '2-3', 16, 0),
     ('coeff_token', '2-3', 16, 1),
     ('ep', 'ins_after_zero_run_2'), ('ep', 'ins_at_64k'), ('ep', 'ins_before_1'), ('ep', 'ins_before_2'),
     ('ep', 'ins_before_3'),
     ('total_zeros', 16, 10, 0),
    ]),
    (('mix', 176, 144, 4, 0, 10000000, (), {'keep': 0.8}), [
     ('cbp_codeNum', 'inter', 36), ('cbp_codeNum', 'inter', 40),
     ('coeff_token', '0-1', 16, 1), ('coeff_token', '2-3', 15, 2), ('coeff_token', '2-3', 15, 3),
     ('total_zeros', 15, 5, 0), ('total_zeros', 16, 12, 0), ('total_zeros', 16, 6, 0), ('total_zeros', 16, 8, 1),
    ]),
    (('blocks', 48, 32, 3, 7, 300000, (), {'cell': 8}), [
     ('cbp_codeNum', 'inter', 33), ('cbp_codeNum', 'inter', 44), ('cbp_codeNum', 'inter', 45),
     ('cbp_codeNum', 'intra', 16),
    ]),
    (('blocks', 48, 32, 3, 4, 300000, (), {'cell': 4}), [
     ('coeff_token', '0-1', 16, 3), ('coeff_token', '4-7', 16, 3),
     ('ep', 'ins_before_0'),
    ]),
    (('mix', 176, 144, 4, 8, 100000, (), {}), [
     ('cbp_codeNum', 'intra', 24),
     ('coeff_token', '2-3', 16, 3),
    ]),
    (('mix', 176, 144, 4, 15, 10000000, (), {'keep': 0.8}), [
     ('total_zeros', 15, 10, 0), ('total_zeros', 15, 6, 0),
    ]),
    (('mix', 176, 144, 4, 11, 10000000, (), {}), [
     ('total_zeros', 15, 8, 0), ('total_zeros', 16, 7, 0),
    ]),
    (('blocks', 48, 32, 3, 2, 300000, (), {'cell': 8}), [
     ('cbp_codeNum', 'intra', 39),
    ]),
    (('mix', 176, 144, 4, 14, 100000, (), {'keep': 0.8}), [
     ('mb_type', 'I', 6),
    ]),
    (('mix', 176, 144, 4, 11, 10000000, (), {'keep': 0.8}), [
     ('total_zeros', 16, 8, 0),
    ]),
    (('mix', 176, 144, 4, 7, 10000000, (), {}), [
     ('coeff_token', '2-3', 16, 2),
    ]),
    (('mix', 176, 144, 4, 5, 10000000, (), {}), [
     ('ep', 'ins_at_64k_plus_1'),
    ]),
    (('blocks', 80, 48, 3, 0, 300000, (), {'cell': 8}), [
     ('cbp_codeNum', 'intra', 3),
    ]),
    (('mix', 48, 32, 4, 52, 100000, (), {}), [
     ('total_zeros', 16, 9, 0),
    ]),
    (('mix', 80, 48, 4, 13, 1000000, (), {'keep': 0.8}), [
     ('cbp_codeNum', 'inter', 38),
    ]),
    (('mix', 80, 48, 4, 21, 1000000, (), {}), [
     ('ep', 'two_in_span'),
    ]),
    (('noise', 176, 144, 3, 11, 3000000, (1, 2), {}), [
     ('ep', 'ins_ge_16384'),
    ]),
    (('checker', 176, 144, 2, 1913, 400000000, (1,), {}), [
     ('ep', 'zero_run_across_chunk'),
    ]),
    (('noise', 256, 192, 2, 100029, 50000000, (1,), {}), []),
    (('noise', 256, 192, 3, 100014, 50000000, (1, 2), {}), []),
    (('noise', 256, 192, 2, 100825, 50000000, (1,), {}), []),
    (('noise', 256, 192, 3, 113461, 50000000, (1, 2), {}), []),
]

# the classes of slice index > 0 a clip is held to on the GPU encoder's three-slice bytes, by the clip's name
SLICE_TARGETS = {
    'patches_3072x2160_s1_20000000_count24': [
        ('pack_slice', 'per_gt32'), ('pack_slice', 'tail_coded_mb'), ('pack_slice', 'range_no_coded_mb'),
        ('pack_slice', 'skip_run_from_earlier_range'), ('pack_slice', 'trailing_run'), ('nC_neighbour', 'other_slice')],
    'patches_16x4096_s1_3000000_every5': [('pack_slice', 'mbh_256')],
    'still_48x32_s1_300000_holdall': [('pack_slice', 'no_coded_mb')],
    'noise_256x192_s100029_50000000_idr1': [('ep_slice', 'ins_at_64k'), ('ep_slice', 'ins_after_zero_run_2')],
    'noise_256x192_s100014_50000000_idr12': [('ep_slice', 'ins_at_64k_plus_1'), ('ep_slice', 'ins_before_2')],
    'noise_256x192_s100825_50000000_idr1': [('ep_slice', 'two_in_span'), ('ep_slice', 'ins_before_0'), ('ep_slice', 'ins_before_1'),
                                            ('ep_slice', 'ins_before_3')],
    'noise_256x192_s113461_50000000_idr12': [('ep_slice', 'zero_run_across_chunk'), ('ep_slice', 'ins_ge_16384')],
}


@functools.lru_cache(maxsize=None)
def directed_clips():
    clips = tuple(spec_clip(spec, tuple(t)) for spec, t in DIRECTED)
    assert set(SLICE_TARGETS) <= {c.name for c in clips}, set(SLICE_TARGETS) - {c.name for c in clips}
    for c in clips:
        c.slice_targets = tuple(SLICE_TARGETS.get(c.name, ()))
    return clips
