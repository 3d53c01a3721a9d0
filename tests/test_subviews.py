"""The sub-view helper (tests/subviews.py) on NumPy arrays, and the alignment requirement that
``ksp_flagger_fused`` states: neither needs a GPU.

tests/test_gpu_subviews.py relies on the helper to notice a launcher that writes outside its
rows; the first half of this file proves that it does notice, with "kernels" that are plain
NumPy stores into the flat allocation."""

import ctypes

import numpy as np
import pytest

from tests import subviews

DTYPES = [np.uint8, np.int16, np.float32, np.complex64, np.complex128]
# (rows, cols, stride, offset)
LAYOUTS = [(5, 7, 7, 0), (5, 7, 11, 0), (5, 7, 8, 1), (1, 300, 301, 3), (300, 1, 2, 1), (3, 64, 64, 0)]


def make_output(dtype, rows, cols, stride, offset):
    blank = subviews.sentinel_array((rows, cols), dtype)
    return subviews.build_host(dtype, blank, stride, offset)


def element(layout, row, col):
    """Index into the flat allocation of (row, col) relative to the view."""
    return layout.start + row * layout.stride + col


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows, cols, stride, offset", LAYOUTS)
def test_layout(dtype, rows, cols, stride, offset):
    flat, layout = make_output(dtype, rows, cols, stride, offset)
    itemsize = np.dtype(dtype).itemsize
    # margins: a whole row stride plus 256 bytes at either end, the front one a multiple of 256
    assert layout.margin * itemsize >= stride * itemsize + 256
    assert layout.margin * itemsize % 256 == 0
    assert layout.start == layout.margin + offset
    assert flat.size == layout.start + rows * stride + layout.margin
    assert np.all(flat.view(np.uint8) == subviews.SENTINEL)
    view = layout.view(flat)
    assert view.shape == (rows, cols) and np.shares_memory(view, flat)
    assert view.strides == (stride * itemsize, itemsize)
    assert np.count_nonzero(layout.inside()) == rows * cols
    last = element(layout, rows - 1, cols - 1)
    assert layout.locate(last * itemsize + itemsize - 1) == (rows - 1, cols - 1)
    assert layout.locate((layout.start - 1) * itemsize) == (-1, stride - 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows, cols, stride, offset", LAYOUTS)
def test_rows_only_pass(dtype, rows, cols, stride, offset):
    """A kernel that writes every element of every row, and nothing else."""
    flat, layout = make_output(dtype, rows, cols, stride, offset)
    data = (np.arange(rows * cols).reshape(rows, cols) % 100).astype(dtype)
    layout.view(flat)[...] = data
    got = subviews.check_host(flat, layout, "out")
    assert got.flags.c_contiguous and got.dtype == np.dtype(dtype)
    np.testing.assert_array_equal(data, got)


def written_at(dtype, rows, cols, stride, offset, index, byte=0):
    """check_host after a kernel that also changes one byte: byte `byte` of element `index`."""
    flat, layout = make_output(dtype, rows, cols, stride, offset)
    layout.view(flat)[...] = 1
    flat.view(np.uint8)[index * layout.dtype.itemsize + byte] ^= 0x01
    with pytest.raises(AssertionError) as info:
        subviews.check_host(flat, layout, "out")
    return str(info.value)


@pytest.mark.parametrize("dtype", DTYPES)
def test_padding_write_fails(dtype):
    """One byte of the padding behind a row: the first, the last, any byte of an element."""
    rows, cols, stride, offset = 5, 7, 11, 1
    layout = subviews.Layout((rows, cols), dtype, stride, offset)
    last_byte = np.dtype(dtype).itemsize - 1
    message = written_at(dtype, rows, cols, stride, offset, element(layout, 2, cols))
    assert "out: 1 bytes outside the rows" in message and f"row 2, column {cols} " in message
    message = written_at(dtype, rows, cols, stride, offset, element(layout, 0, stride - 1), last_byte)
    assert f"row 0, column {stride - 1} " in message
    # the strides behind the last row's data are outside as well
    message = written_at(dtype, rows, cols, stride, offset, element(layout, rows - 1, cols))
    assert f"row {rows - 1}, column {cols} " in message


@pytest.mark.parametrize("dtype", DTYPES)
def test_write_before_first_row_fails(dtype):
    rows, cols, stride, offset = 5, 7, 11, 1
    layout = subviews.Layout((rows, cols), dtype, stride, offset)
    last_byte = np.dtype(dtype).itemsize - 1
    # the element just in front of the view (what an aligned-down vector store would hit)
    assert "row -1, column 10 " in written_at(dtype, rows, cols, stride, offset, layout.start - 1, last_byte)
    # a whole row in front, and the very first byte of the allocation
    assert "row -1, column 0 " in written_at(dtype, rows, cols, stride, offset, layout.start - stride)
    assert "outside the rows" in written_at(dtype, rows, cols, stride, offset, 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_write_after_last_row_fails(dtype):
    rows, cols, stride, offset = 5, 7, 11, 1
    layout = subviews.Layout((rows, cols), dtype, stride, offset)
    assert f"row {rows}, column 0 " in written_at(dtype, rows, cols, stride, offset, element(layout, rows, 0))
    assert f"row {rows}, column 3 " in written_at(dtype, rows, cols, stride, offset, element(layout, rows, 3))
    last = layout.size - 1
    assert "outside the rows" in written_at(dtype, rows, cols, stride, offset, last, np.dtype(dtype).itemsize - 1)


def test_first_offender_is_reported():
    flat, layout = make_output(np.float32, 4, 6, 9, 2)
    flat[element(layout, 3, 7)] = 0
    flat[element(layout, 1, 8)] = 0
    with pytest.raises(AssertionError, match=r"8 bytes outside the rows.*row 1, column 8 "):
        subviews.check_host(flat, layout, "out")


@pytest.mark.parametrize("dtype", DTYPES)
def test_poison(dtype):
    """Inputs: NaN (in both parts of a complex number) or 0xFF everywhere but in the rows."""
    data = np.ones((3, 5), dtype)
    flat, layout = subviews.build_host(dtype, data, 8, 1, poison=True)
    np.testing.assert_array_equal(layout.view(flat), data)
    outside = flat[~layout.inside()]
    assert outside.size == flat.size - 15
    if np.dtype(dtype).kind == "c":
        assert np.isnan(outside.real).all() and np.isnan(outside.imag).all()
    elif np.dtype(dtype).kind == "f":
        assert np.isnan(outside).all()
    else:
        assert np.all(outside.view(np.uint8) == 0xFF)


# ------------------------------------------------------------------ argument validation
@pytest.fixture(scope="module")
def lib():
    import os

    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    return _lib.load()


def test_fused_flagger_alignment_validation_without_gpu(lib):
    """The one alignment requirement of the ABI: an even vis_stride and a 16-byte aligned vis,
    refused with a message before any device call."""
    from katsdpsigproc_amd import _lib

    p = ctypes.c_void_p(64)  # never dereferenced: every call below fails its checks first
    scales = (ctypes.c_double * 4)(1.0, 0.8, 0.7, 0.6)

    def call(vis=p, flags=p, channels=64, baselines=10, vis_stride=10, flags_stride=15,
             width=13, is_amplitude=0):  # fmt: skip
        rc = lib.ksp_flagger_fused(
            0, None, vis, None, flags, None, None, channels, baselines, vis_stride, 0,
            flags_stride, 0, width, is_amplitude, 0, 1, 11.0, scales, 4, 1, None)  # fmt: skip
        assert rc != 0
        assert lib.ksp_flagger_fused_last_path() == 0  # nothing was launched
        return _lib.last_error()

    assert "vis_stride must be even" in call(vis_stride=11)
    assert "vis_stride must be even" in call(vis_stride=13, is_amplitude=1)
    for address in (65, 68, 72, 80 - 1):
        assert "vis must be 16-byte aligned" in call(vis=ctypes.c_void_p(address))
    assert "vis must be 16-byte aligned" in call(vis=ctypes.c_void_p(72), channels=8192)
    assert "vis must be 16-byte aligned" in call(vis=ctypes.c_void_p(72), width=21)
    # the other arrays carry no such requirement: these fail for their own reasons
    assert "stride smaller than row" in call(flags=ctypes.c_void_p(65), flags_stride=9)
    assert "NULL buffer" in call(vis=None)
