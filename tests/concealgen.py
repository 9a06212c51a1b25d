"""Lossy multi-slice pictures and the full pictures they must decode to (TEST INFRASTRUCTURE).

The rule of slice-copy concealment is exact: the macroblocks no good slice covers are decoded as one P slice per gap
that is a single mb_skip_run, with the QP and loop-filter fields of the donor slice. So for every lossy access unit
there is a conforming full one that any decoder must decode to the same samples: the received slices as they are,
and at the place of each gap an all-skip slice with the donor's qp_delta and dbk. Two generators with one seed write
the two in lockstep: the sender's unit (its lost slices as the sender cut them) and the full unit (one all-skip slice
per gap). Every macroblock of a lost slice is scripted as skipped in both, so both consume the same random draws and
the received slices come out byte for byte the same -- which lossy() asserts."""
from streamgen import BitWriter, SyntaxGen, nal
from test_syntax_streams import SO, _split_nals


def ref_gaps(total, slices):
    """the gap rule restated: slices = [(first, end, ok)] -> [(first, end, donor)] in address order, None: reject"""
    good = sorted((f, e, j) for j, (f, e, ok) in enumerate(slices) if ok and 0 <= f < e <= total)
    if not good or total <= 0 or len(slices) > 32:
        return None
    covered = [0] * total
    for f, e, _ in good:
        for a in range(f, e):
            covered[a] += 1
    if max(covered) > 1:
        return None
    ends = {e: j for f, e, j in good}
    begins = {f: j for f, e, j in good}
    gaps, a = [], 0
    while a < total:
        if covered[a]:
            a += 1
            continue
        b = a
        while b < total and not covered[b]:
            b += 1
        gaps.append((a, b, ends[a] if a > 0 else begins[b]))
        a = b
    return gaps


def runs(lost):
    """maximal runs of consecutive lost slice indices"""
    out = []
    for i in sorted(lost):
        if out and out[-1][-1] == i - 1:
            out[-1].append(i)
        else:
            out.append([i])
    return out


def full_layout(layout, lost):
    """the full unit's layout for the sender's `layout` with the slices `lost` missing: one all-skip P slice per run of
    lost slices with the donor's qp_delta / dbk -> (layout, index in it of every sender slice, None for a merged one)"""
    out, index = [], []
    donors = {}
    for run in runs(lost):
        d = run[0] - 1 if run[0] > 0 else run[-1] + 1
        assert 0 <= d < len(layout) and d not in lost, 'a gap needs a received donor'
        donors[run[0]] = d
    for i, sl in enumerate(layout):
        if i in lost and i not in donors:
            index.append(None)      # merged into the run's first slice
            continue
        if i in donors:
            d = layout[donors[i]]
            sl = dict(first=sl['first'], qp_delta=d.get('qp_delta', 0), dbk=d.get('dbk', (0, 0, 0)))
        index.append(len(out))
        out.append(sl)
    return out, index


def slice_end(layout, i, total):
    return layout[i + 1]['first'] if i + 1 < len(layout) else total


class Pair:
    """two SyntaxGen of one seed in lockstep: .a writes what the sender sent, .b the full units for the oracle"""

    def __init__(self, mbw, mbh, seed, **kw):
        self.a, self.b = SyntaxGen(SO, mbw, mbh, seed, **kw), SyntaxGen(SO, mbw, mbh, seed, **kw)
        self.total = mbw * mbh

    def idr(self, **kw):
        u = self.a.idr(**kw)
        assert u == self.b.idr(**kw)
        return u

    def lossy(self, layout, lost, order=None, ref_idc=2, failed=(), **kw):
        """one P picture -> (full unit, lossy unit, MBs lost). lost: indices into layout; order: the lossy unit's slice
        order (indices into layout, the lost ones left out); failed: lost slices whose NAL is not dropped but replaced
        by one that cannot parse (failed_nal)"""
        lost = set(lost)
        script = {}
        for i in lost:
            for addr in range(layout[i]['first'], slice_end(layout, i, self.total)):
                script[addr] = {'kind': 'skip'}
        sender = [dict(sl, intra=False) if i in lost else sl for i, sl in enumerate(layout)]
        fl, index = full_layout(layout, lost)
        ua = self.a.p(slices=sender, script=script, ref_idc=ref_idc, **kw)
        ub = self.b.p(slices=fl, script=script, ref_idc=ref_idc, **kw)
        na, nb = _split_nals(ua), _split_nals(ub)
        assert len(na) == len(layout) and len(nb) == len(fl)
        for i in range(len(layout)):
            if i not in lost:
                assert na[i] == nb[index[i]], 'the received slices of the two units differ'
        keep = [i for i in (order or range(len(layout))) if i not in lost or i in failed]
        unit = b''.join(failed_nal(na[i], slice_end(layout, i, self.total) - layout[i]['first'], self.total) if i in failed else na[i]
                        for i in keep)
        return ub, unit, len(script)


def _unescape(payload):
    out, z = bytearray(), 0
    for c in payload:
        if z >= 2 and c == 3:
            z = 0
            continue
        out.append(c)
        z = z + 1 if c == 0 else 0
    return bytes(out)


def _ue_bits(v):
    return 2 * (v + 1).bit_length() - 1


def skip_slice_header_bits(unit_nal, run):
    """the slice_header() bits of an all-skip slice NAL whose slice_data() is the single mb_skip_run `run`"""
    rbsp = _unescape(unit_nal[5:])
    bits = ''.join(f'{c:08b}' for c in rbsp).rstrip('0')[:-1]   # rbsp_trailing_bits
    return bits[:len(bits) - _ue_bits(run)]


def failed_nal(unit_nal, run, total):
    """the all-skip slice's NAL with the same header and a slice_data() of one mb_skip_run larger than the picture: no
    conforming parser accepts it (7.4.4: the run cannot exceed the macroblocks left)"""
    w = BitWriter()
    for ch in skip_slice_header_bits(unit_nal, run):
        w.u(int(ch), 1)
    w.ue(total + 1)
    return nal((unit_nal[4] >> 5) & 3, unit_nal[4] & 31, w.rbsp())
