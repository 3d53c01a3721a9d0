"""Percentile5 on rows of 16385 to 65536 columns without a GPU: template wiring, the
template's limit and the launcher's range check."""

import ctypes
import os

import pytest

from tests.fakes import FakeContext


@pytest.mark.parametrize(
    "max_columns, shape, column_range, is_amplitude",
    [
        (16385, (7, 16385), None, True),
        (40000, (33, 40003), (3, 40003), False),
        (65536, (5, 65600), (64, 65600), True),
        (65536, (2, 65536), (1, 16386), False),
    ],
)
def test_long_template_wires_up(max_columns, shape, column_range, is_amplitude):
    from katsdpsigproc_amd import percentile

    ctx = FakeContext()
    queue = ctx.create_command_queue()
    template = percentile.Percentile5Template(ctx, max_columns=max_columns, is_amplitude=is_amplitude)
    fn = template.instantiate(queue, shape, column_range)
    fn.ensure_all_bound()
    fn()
    name, args = queue.launches[-1]
    assert name == "ksp_percentile5_float"
    lo, hi = column_range if column_range else (0, shape[1])
    in_stride = fn.buffer("src").padded_shape[1]
    out_stride = fn.buffer("dest").padded_shape[1]
    assert in_stride >= shape[1] and out_stride >= shape[0]
    assert [int(a) for a in args[2:]] == [shape[0], in_stride, out_stride, lo, hi - lo, int(is_amplitude)]


def test_long_template_rejects_beyond_range():
    from katsdpsigproc_amd import percentile

    with pytest.raises(ValueError, match="65536"):
        percentile.Percentile5Template(FakeContext(), max_columns=65537)
    assert percentile.MAX_COLUMNS_SUPPORTED == 65536


def test_long_column_range_wider_than_max_columns():
    from katsdpsigproc_amd import percentile

    ctx = FakeContext()
    queue = ctx.create_command_queue()
    template = percentile.Percentile5Template(ctx, max_columns=40000)
    with pytest.raises(ValueError):
        template.instantiate(queue, (4, 65536))
    with pytest.raises(ValueError):
        template.instantiate(queue, (4, 65536), (100, 40101))
    template.instantiate(queue, (4, 65536), (100, 40100))


def test_launcher_rejects_columns_before_device_calls():
    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    for n_cols in (65537, 10**6):
        rc = lib.ksp_percentile5_float(0, None, buf, buf, 1, n_cols, 1, 0, n_cols, 1)
        assert rc != 0
        assert str(n_cols) in _lib.last_error() and "1..65536" in _lib.last_error()
