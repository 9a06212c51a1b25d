"""CPU: h264mi_i420_compose_dev and h264mi_i420_compose_any_dev check a cell list by one rule (csrc/picture_host.h,
cells_ok) that differs between them in one place only: whether a rectangle may be larger than its crop. Starting from
the valid lists of test_compose_host.py and test_upscale_host.py, every field of a cell is corrupted in turn, two cells
are made to touch and to share a sample, and both calls must refuse exactly what the rule table below -- include/h264mi.h
restated in plain Python, not read from the C code -- refuses. Only lists that must be refused reach a device call here:
the pointers are never dereferenced. What the calls accept is the GPU suite's business."""
import ctypes

import pytest

from test_compose_host import OK_CELL
from test_upscale_host import DOWN_CELL, UP_CELL

FIELDS = ('src', 'canvas', 'sx', 'sy', 'sw', 'sh', 'dx', 'dy', 'dw', 'dh')
MAX_SRC, MAX_CANVAS, MAX_CELLS = 4096, 8192, 4096


def accepted(cw, ch, ncanvas, src_w, src_h, nsrc, cells, may_enlarge):
    """the rule table: True where the call must go on to its launches"""
    if ncanvas < 1 or nsrc < 1 or not 1 <= len(cells) <= MAX_CELLS:
        return False
    for v, top in ((cw, MAX_CANVAS), (ch, MAX_CANVAS), (src_w, MAX_SRC), (src_h, MAX_SRC)):
        if v % 2 or not 2 <= v <= top:
            return False
    for src, canvas, sx, sy, sw, sh, dx, dy, dw, dh in cells:
        if not 0 <= src < nsrc or not 0 <= canvas < ncanvas:
            return False
        if any(v % 2 for v in (sx, sy, sw, sh, dx, dy, dw, dh)):
            return False
        if sx < 0 or sy < 0 or sw < 2 or sh < 2 or sx + sw > src_w or sy + sh > src_h:  # the crop lies in the source
            return False
        if dx < 0 or dy < 0 or dw < 2 or dh < 2 or dx + dw > cw or dy + dh > ch:        # the rectangle in the canvas
            return False
        shrinks, enlarges = dw <= sw and dh <= sh, dw >= sw and dh >= sh
        if not (shrinks or (may_enlarge and enlarges)):                                 # never one axis each way
            return False
    for i, a in enumerate(cells):
        for b in cells[:i]:  # two cells of one canvas share a sample
            if a[1] == b[1] and a[6] < b[6] + b[8] and b[6] < a[6] + a[8] and a[7] < b[7] + b[9] and b[7] < a[7] + a[9]:
                return False
    return True


def _cells(tuples):
    import h264mi
    return (h264mi.Cell * len(tuples))(*[h264mi.Cell(*t) for t in tuples])


def _refused_where_the_table_says(geo, cells):
    """(compose accepted, compose_any accepted) by the table; each call that must refuse is made and must return -1"""
    import h264mi
    L = h264mi.lib()
    d, s = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x20000000)
    cw, ch, ncanvas, src_w, src_h, nsrc = geo
    arr = _cells(cells)
    want = accepted(*geo, cells, False), accepted(*geo, cells, True)
    if not want[0]:
        assert L.h264mi_i420_compose_dev(d, cw, ch, ncanvas, s, src_w, src_h, nsrc, arr, len(cells), None) == -1, (geo, cells)
    for filt in (0, 1):
        if not want[1]:
            assert L.h264mi_i420_compose_any_dev(d, cw, ch, ncanvas, s, src_w, src_h, nsrc, arr, len(cells), filt, None) == -1, (geo, cells, filt)
    return want


# (cw, ch, ncanvas, src_w, src_h, nsrc), cells: the lists the two host tests start from
ROOMY_DOWN = (0, 0, 2, 2, 16, 16, 4, 4, 8, 8)   # test_compose_host.py's base of the odd-field cases
ROOMY_UP = (0, 0, 2, 2, 8, 8, 4, 4, 16, 16)     # test_upscale_host.py's
BASES = [((32, 32, 1, 32, 32, 1), [OK_CELL]), ((32, 32, 1, 32, 32, 1), [ROOMY_DOWN]),
         ((64, 64, 1, 32, 32, 1), [UP_CELL, DOWN_CELL]), ((64, 64, 1, 32, 32, 1), [ROOMY_UP])]


def test_the_bases_are_what_the_host_tests_say():
    assert [accepted(*g, c, False) for g, c in BASES] == [True, True, False, False]  # compose refuses an enlarging cell
    assert [accepted(*g, c, True) for g, c in BASES] == [True, True, True, True]


def _corruptions(geo, cell, f):
    """field f of cell made odd, negative, one past the source or canvas, and running over the edge"""
    cw, ch, ncanvas, src_w, src_h, nsrc = geo
    _, _, sx, sy, sw, sh, dx, dy, dw, dh = cell
    past = (nsrc, ncanvas, src_w + 2, src_h + 2, src_w + 2, src_h + 2, cw + 2, ch + 2, cw + 2, ch + 2)
    edge = (None, None, src_w - sw + 2, src_h - sh + 2, src_w - sx + 2, src_h - sy + 2, cw - dw + 2, ch - dh + 2, cw - dx + 2, ch - dy + 2)
    out = {'odd': cell[f] + 1, 'negative': -1 if f < 2 else -2, 'past': past[f]}
    if edge[f] is not None:
        out['edge'] = edge[f]
    return out


@pytest.mark.parametrize('field', range(10), ids=FIELDS)
def test_every_corrupted_field_is_refused_by_both_calls(libpath, field):
    n = 0
    for geo, cells in BASES:
        for k, cell in enumerate(cells):
            for kind, v in _corruptions(geo, cell, field).items():
                bad = list(cells)
                bad[k] = cell[:field] + (v,) + cell[field + 1:]
                # the table itself, spelled out: each of these corruptions is a refusal whatever the rule on sizes
                assert _refused_where_the_table_says(geo, bad) == (False, False), (kind, geo, bad)
                n += 1
    assert n == 5 * (3 if field < 2 else 4)


def test_enlarging_is_where_the_two_calls_differ(libpath):
    geo = (64, 64, 1, 32, 32, 1)
    for base in (ROOMY_DOWN, ROOMY_UP, (0, 0, 2, 2, 8, 8, 4, 4, 8, 8)):
        src, canvas, sx, sy, sw, sh, dx, dy, _, _ = base
        cell = lambda dw, dh: [(src, canvas, sx, sy, sw, sh, dx, dy, dw, dh)]
        # larger than the crop on one axis only, the other smaller: refused by both
        assert _refused_where_the_table_says(geo, cell(sw + 2, sh - 2)) == (False, False)
        assert _refused_where_the_table_says(geo, cell(sw - 2, sh + 2)) == (False, False)
        # larger on one axis, equal on the other, and larger on both: compose refuses, compose_any does not
        assert _refused_where_the_table_says(geo, cell(sw + 2, sh)) == (False, True)
        assert _refused_where_the_table_says(geo, cell(sw, sh + 2)) == (False, True)
        assert _refused_where_the_table_says(geo, cell(sw + 2, sh + 2)) == (False, True)
        assert _refused_where_the_table_says(geo, cell(2 * sw, 2 * sh)) == (False, True)
        # no larger on either: both go on
        assert _refused_where_the_table_says(geo, cell(sw, sh)) == (True, True)
        assert _refused_where_the_table_says(geo, cell(sw - 2, sh)) == (True, True)


def test_cells_that_touch_go_on_and_cells_that_share_a_sample_do_not(libpath):
    geo = (64, 64, 2, 32, 32, 1)
    a = (0, 0, 0, 0, 16, 16, 0, 0, 16, 16)
    other = lambda canvas, dx, dy, dw=16, dh=16: (0, canvas, 0, 0, 16, 16, dx, dy, dw, dh)
    for b in (other(0, 16, 0), other(0, 0, 16), other(0, 16, 16), other(0, 16, 0, 32, 32)):  # touching: an edge, a corner
        assert _refused_where_the_table_says(geo, [a, b])[1] is True and _refused_where_the_table_says(geo, [b, a])[1] is True
    assert _refused_where_the_table_says(geo, [a, other(0, 16, 0)]) == (True, True)
    for b in (other(0, 14, 14), other(0, 14, 0), other(0, 0, 14), other(0, 0, 0), other(0, 14, 14, 32, 32)):  # 14, 14: one chroma sample
        assert _refused_where_the_table_says(geo, [a, b]) == (False, False)
        assert _refused_where_the_table_says(geo, [b, a]) == (False, False)
        assert _refused_where_the_table_says(geo, [a, other(0, 32, 32), b]) == (False, False)
    for b in (other(1, 14, 14), other(1, 0, 0)):  # the same rectangles on different canvases
        assert _refused_where_the_table_says(geo, [a, b]) == (True, True)
    assert _refused_where_the_table_says(geo, [a, other(1, 0, 0, 32, 32)]) == (False, True)
