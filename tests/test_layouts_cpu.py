"""CPU: the layout helper of the strided-operand tests catches what it is there to catch.

numpy stands in for the kernel: a column scaling `out[b][:, j] = 2 * a[b][:, j]` written against
the raw buffers with (offset, ld, stride), once correctly and once with each of the mistakes the
GPU tests must not let through.
"""
import numpy as np
import pytest

import _layouts as L

B, ROWS, COLS = 3, 5, 4


def _kernel(src, dst, rows=ROWS, cols=COLS, batch=B, extra_row=False, gap_write=False,
            read_pad=False, tight_ld=False):
    s, d = src.buf, dst.buf
    ld_d = rows if tight_ld else dst.ld
    for b in range(batch):
        for j in range(cols):
            so = src.offset + b * src.stride + j * src.ld
            do = dst.offset + b * dst.stride + j * ld_d
            n_read = rows + 1 if read_pad and j == 1 else rows
            col = s[so:so + n_read]
            d[do:do + rows] = 2.0 * col[:rows]
            if read_pad and j == 1:
                d[do] += 0.0 * col[rows]                 # a padding element enters the sum
            if extra_row and j == 2 and b == 1:
                d[do + rows] = 1.0                       # one element past the column's end
        if gap_write and b == 0:
            d[dst.offset + b * dst.stride + cols * dst.ld] = 0.0    # between two problems


def _pair(case):
    a = np.random.default_rng(0).standard_normal((B, COLS, ROWS))
    return a, L.place(a, case), L.blank_case((B, COLS, ROWS), case)


@pytest.mark.parametrize("case", L.CASES)
def test_layout_dims_meet_their_table(case):
    rows, cols = 129, 129
    off, ld, stride = L.dims(case, rows, cols)
    assert ld >= rows and stride >= ld * cols
    want = {"tight": (0, ld == rows, stride == rows * cols),
            "odd_ld": (0, ld % 2 == 1, stride == ld * cols),
            "off8": (1, ld % 2 == 0 and ld % 16 != 0, stride == ld * cols),
            "off16": (2, ld % 16 == 0, stride % 16 == 0),
            "odd_stride": (0, ld % 16 == 0, stride == ld * cols + 1),
            "gap16": (0, ld % 16 == 0 and ld > rows, stride % 16 == 0 and stride > ld * cols)}
    assert (off, True, True) == want[case]
    # 128 rows: "even, not a multiple of 16" needs the extra pair of rows
    assert L.dims("off8", 128, 128)[1] == 130


@pytest.mark.parametrize("case", L.CASES)
def test_correct_kernel_passes(case):
    a, src, dst = _pair(case)
    _kernel(src, dst)
    dst.check()
    src.check(written=False)
    np.testing.assert_array_equal(dst.extract(), 2.0 * a)
    # the guard is at least as long as the tight extent of the whole batch
    assert dst.size - (dst.offset + (B - 1) * dst.stride + COLS * dst.ld) >= B * COLS * ROWS


@pytest.mark.parametrize("case", ["odd_ld", "off8", "off16", "odd_stride", "gap16"])
def test_write_past_a_columns_end_is_caught(case):
    _, src, dst = _pair(case)
    _kernel(src, dst, extra_row=True)
    with pytest.raises(AssertionError, match="outside the written region"):
        dst.check()


@pytest.mark.parametrize("case", ["odd_stride", "gap16"])
def test_write_into_the_gap_between_problems_is_caught(case):
    _, src, dst = _pair(case)
    _kernel(src, dst, gap_write=True)
    with pytest.raises(AssertionError, match="outside the written region"):
        dst.check()


@pytest.mark.parametrize("case", ["odd_ld", "off8", "gap16"])
def test_read_of_a_padding_element_is_caught(case):
    _, src, dst = _pair(case)
    _kernel(src, dst, read_pad=True)
    dst.check()                                          # nothing stray was written ...
    with pytest.raises(AssertionError, match="non-finite"):
        dst.extract()                                    # ... but the NaN padding was read


@pytest.mark.parametrize("case", ["odd_ld", "gap16"])
def test_tight_ld_in_place_of_ld_is_caught_inside_the_allocation(case):
    a, src, dst = _pair(case)
    _kernel(src, dst, tight_ld=True)                     # stays inside the buffer: no IndexError
    with pytest.raises(AssertionError):
        dst.check()
        np.testing.assert_array_equal(dst.extract(), 2.0 * a)


def test_partial_write_masks_and_unwritten_elements():
    """`written` narrows what may change (the lower triangle of a factorisation); an element of
    the written region the kernel skipped is still the NaN sentinel and fails `extract`."""
    n = 6
    a = np.random.default_rng(1).standard_normal((1, n, n))
    lower = np.triu(np.ones((n, n), bool))[None]         # memory order: row >= col
    buf = L.place(a, "off8", mask=lower)
    buf.check(written=False)
    buf.buf[buf.pos(0, 1, 3)] = 5.0                    # (row 3, col 1): lower, allowed
    buf.check(written=lower)
    buf.buf[buf.pos(0, 3, 1)] = 5.0                    # (row 1, col 3): strict upper
    with pytest.raises(AssertionError, match="outside the written region"):
        buf.check(written=lower)
    out = L.blank_case((1, n, n), "gap16")
    with pytest.raises(AssertionError, match="non-finite"):
        out.extract()


def test_float32_buffers_use_their_own_sentinel():
    out = L.blank((1, 3, 7), offset=1, ld=9, dtype=np.float32)
    assert out.buf.dtype == np.float32 and np.isnan(out.buf).all()
    out.region(out.buf)[...] = 1.0
    out.check()
    out.buf[out.offset + 7] = 1.0
    with pytest.raises(AssertionError):
        out.check()
