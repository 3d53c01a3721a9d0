"""Percentile5 on rows of 16385 to 65536 columns on the GPU (the radix-select kernel of
percentile_long.h): every output bit-exact against the CPU oracle, and for float32 input
against numpy's "lower" percentiles as well."""

import numpy as np
import pytest

from tests import inputs

pytestmark = pytest.mark.gpu

# among them the smallest and the largest width of every kernel instantiation (32, 48 and 64
# values per thread: up to 32768, 49152, 65536)
WIDTHS = [16385, 16448, 20000, 32767, 32768, 32769, 40001, 49152, 49153, 65535, 65536]


@pytest.fixture(scope="module")
def context():
    from katsdpsigproc_amd import accel

    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


@pytest.fixture(scope="module")
def oracle():
    from oracle import rfi_oracle

    rfi_oracle.set_threads(min(rfi_oracle.max_threads(), 16))
    yield rfi_oracle
    rfi_oracle.set_threads(1)


def pad_dimension(dim, extra):
    from katsdpsigproc_amd import accel

    accel.Dimension(dim.size, min_padded_size=dim.size + extra).link(dim)


def run(context, queue, ary, column_range=None, pad=True):
    """percentile5 of `ary` on the device; src and dest padded unless `pad` is False."""
    from katsdpsigproc_amd import percentile

    lo, hi = column_range if column_range else (0, ary.shape[1])
    template = percentile.Percentile5Template(
        context, max_columns=hi - lo, is_amplitude=not np.iscomplexobj(ary)
    )
    fn = template.instantiate(queue, ary.shape, column_range)
    if pad:
        pad_dimension(fn.slots["src"].dimensions[0], 1)
        pad_dimension(fn.slots["src"].dimensions[1], 4)
        pad_dimension(fn.slots["dest"].dimensions[0], 2)
        pad_dimension(fn.slots["dest"].dimensions[1], 3)
    fn.ensure_all_bound()
    fn.buffer("src").set(queue, ary)
    fn()
    return fn.buffer("dest").get(queue)


def check(oracle, ary, out, column_range=None):
    np.testing.assert_array_equal(oracle.percentile5(ary, column_range), out)
    if not np.iscomplexobj(ary):
        lo, hi = column_range if column_range else (0, ary.shape[1])
        expected = np.percentile(ary[:, lo:hi], [0, 100, 25, 75, 50], axis=1, method="lower")
        np.testing.assert_array_equal(expected.astype(np.float32), out)


def random_rows(rows, cols, complex_, seed):
    rs = np.random.RandomState(seed)
    if complex_:
        return inputs.complex_normal(rs, size=(rows, cols)).astype(np.complex64)
    return np.abs(rs.randn(rows, cols)).astype(np.float32)


@pytest.mark.parametrize("complex_", [False, True], ids=["float32", "complex64"])
@pytest.mark.parametrize("cols", WIDTHS)
def test_widths(cols, complex_, context, command_queue, oracle):
    ary = random_rows(37, cols, complex_, seed=cols)
    check(oracle, ary, run(context, command_queue, ary))


@pytest.mark.parametrize("complex_", [False, True], ids=["float32", "complex64"])
@pytest.mark.parametrize(
    "cols, column_range",
    [
        (16400, (1, 16386)),  # unaligned first column: element loads
        (40010, (3, 40003)),
        (70000, (20000, 70000)),  # ends at the last column of a wider array
        (65600, (32, 65568)),  # a full 65536 range inside a wider row
        (65600, (4, 65540)),
    ],
)
def test_column_ranges(cols, column_range, complex_, context, command_queue, oracle):
    ary = random_rows(19, cols, complex_, seed=column_range[0] + 7)
    check(oracle, ary, run(context, command_queue, ary, column_range), column_range)


@pytest.mark.parametrize("cols", [16385, 16388])
def test_unpadded_rows(cols, context, command_queue, oracle):
    """Rows packed back to back: 16-byte loads only where the stride allows them."""
    ary = random_rows(11, cols, False, seed=3)
    check(oracle, ary, run(context, command_queue, ary, pad=False))


def hard_rows(n, seed):
    """One float32 row per awkward case."""
    rs = np.random.RandomState(seed)
    rows = []
    rows.append((rs.randint(-4, 5, n) * 0.25).astype(np.float32))  # signed ties
    rows.append(np.full(n, 2.5, np.float32))  # constant row
    rows.append(np.full(n, -1.5, np.float32))  # constant negative row
    zeros = np.zeros(n, np.float32)
    zeros[rs.random_sample(n) < 0.5] = -0.0
    rows.append(zeros)  # a mix of -0.0 and 0.0
    mixed = zeros.copy()
    mixed[rs.random_sample(n) < 0.2] = 1.0
    mixed[rs.random_sample(n) < 0.2] = -1.0
    rows.append(mixed)
    # keys sharing their top 22 bits: passes 2 and 3 decide
    rows.append((np.float32(1.0) + rs.randint(0, 700, n) * np.float32(2.0**-23)).astype(np.float32))
    rows.append((np.float32(-1.0) - rs.randint(0, 3, n) * np.float32(2.0**-23)).astype(np.float32))
    # the three ranks in different top-level bins (decades apart, both signs)
    spread = np.concatenate(
        [
            -np.exp2(rs.uniform(60, 80, n // 4)),
            np.exp2(rs.uniform(-80, -60, n // 4)),
            np.exp2(rs.uniform(-10, 10, n // 4)),
            np.exp2(rs.uniform(60, 80, n - 3 * (n // 4))),
        ]
    ).astype(np.float32)
    rows.append(spread[rs.permutation(n)])
    # denormals and +inf among ordinary values
    den = rs.standard_normal(n).astype(np.float32)
    sel = rs.random_sample(n) < 0.4
    den[sel] = (rs.standard_normal(int(sel.sum())) * 1e-40).astype(np.float32)
    den[rs.random_sample(n) < 0.02] = np.inf
    den[rs.random_sample(n) < 0.02] = -np.inf
    rows.append(den)
    rows.append((rs.standard_normal(n) * 1e-41).astype(np.float32))  # all denormal
    # every value distinct and signed
    rows.append(rs.permutation(np.arange(-(n // 2), n - n // 2)).astype(np.float32))
    # a single value different from the rest, at the top and at the bottom
    one = np.full(n, 3.0, np.float32)
    one[rs.randint(n)] = 4.0
    rows.append(one)
    one = np.full(n, 3.0, np.float32)
    one[rs.randint(n)] = -4.0
    rows.append(one)
    return np.stack(rows)


@pytest.mark.parametrize("cols", [16385, 20000, 40001, 65536])
def test_hard_data(cols, context, command_queue, oracle):
    ary = hard_rows(cols, seed=cols)
    check(oracle, ary, run(context, command_queue, ary))
    # the same rows through an unaligned column range of a wider array
    wide = np.zeros((ary.shape[0], cols + 5), np.float32)
    wide[:, 1 : cols + 1] = ary
    check(oracle, wide, run(context, command_queue, wide, (1, cols + 1)), (1, cols + 1))


def test_nan_rows_leave_the_others_alone(context, command_queue, oracle):
    """A NaN makes its own row's result undefined (as for shorter rows), nothing else."""
    ary = random_rows(9, 30000, False, seed=4)
    ary[3, 17] = np.nan
    ary[5, ::3] = np.nan
    out = run(context, command_queue, ary)
    keep = [r for r in range(ary.shape[0]) if r not in (3, 5)]
    np.testing.assert_array_equal(oracle.percentile5(ary[keep]), out[:, keep])


@pytest.mark.parametrize(
    "rows, cols, complex_", [(4096, 32768, False), (1024, 65536, True)], ids=["f32", "c64"]
)
def test_full_size(rows, cols, complex_, context, command_queue, oracle):
    ary = random_rows(rows, cols, complex_, seed=99)
    out = run(context, command_queue, ary, pad=False)
    np.testing.assert_array_equal(oracle.percentile5(ary), out)
