"""CPU: the encoder's slice partition -- slice k of a picture of mbh MB rows coded as n slices
starts at MB row (k * mbh) // n. h264mi.slice_first_row and the C function behind it (h264mi_slice_first_row, host
only: no GPU call) over every picture height up to 1088 rows of samples and every slice count the encoder accepts."""
import ctypes

import pytest

MAX_SLICES = 32  # H264MI_MAX_SLICES: what the decoder parses of one picture


@pytest.fixture(scope='module')
def cfn(libpath):
    L = ctypes.CDLL(libpath)
    L.h264mi_slice_first_row.restype = ctypes.c_int
    L.h264mi_slice_first_row.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    return L.h264mi_slice_first_row


def test_partition_every_height_and_count(cfn):
    import h264mi
    for mbh in range(1, 69):
        for n in range(1, min(mbh, MAX_SLICES) + 1):
            rows = [h264mi.slice_first_row(mbh, n, k) for k in range(n + 1)]
            assert rows == [cfn(mbh, n, k) for k in range(n + 1)], (mbh, n)
            assert rows == [(k * mbh) // n for k in range(n + 1)], (mbh, n)
            assert rows[0] == 0 and rows[n] == mbh, (mbh, n, rows)
            assert all(a < b for a, b in zip(rows, rows[1:])), (mbh, n, rows)  # no empty slice


def test_bad_arguments(cfn):
    import h264mi
    for f in (h264mi.slice_first_row, cfn):
        assert f(9, 0, 0) == -1          # n == 0
        assert f(68, 33, 0) == -1        # n > 32
        assert f(9, 10, 0) == -1         # n > mbh
        assert f(9, 3, 4) == -1          # k > n
        assert f(9, 3, -1) == -1
        assert f(0, 1, 0) == -1
        assert f(9, 3, 3) == 9 and f(68, 32, 32) == 68
