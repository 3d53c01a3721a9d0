"""NoiseEstMADT on bands of 16385 to 262144 channels on the GPU, and the kernel-per-stage
flagger built on it: noise float32-equal and flags bit for bit against the CPU oracle."""

import numpy as np
import pytest

from tests import inputs

pytestmark = pytest.mark.gpu

CHANNELS = [16385, 20000, 32767, 32768, 38913, 65536, 131071, 262144]


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


def run_madt(context, queue, dev, pad=0):
    """Noise of channel-major float32 `dev` through the baseline-major operation, its rows
    padded by `pad` elements."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import device

    channels, baselines = dev.shape
    fn = device.NoiseEstMADTDeviceTemplate(context, channels).instantiate(queue, channels, baselines)
    if pad:
        dim = fn.slots["deviations"].dimensions[1]
        accel.Dimension(dim.size, min_padded_size=dim.size + pad).link(dim)
    fn.ensure_all_bound()
    assert fn.buffer("deviations").padded_shape[1] >= channels + pad
    fn.buffer("deviations").set(queue, np.ascontiguousarray(dev.T))
    fn()
    return fn.buffer("noise").get(queue)


def check(oracle, out, dev):
    expected = oracle.NoiseEstMADHost()(dev).astype(np.float32)
    np.testing.assert_array_equal(expected, out)


def gaussian(channels, baselines, seed):
    rs = np.random.RandomState(seed=seed)
    dev = rs.standard_normal((channels, baselines)).astype(np.float32)
    dev[rs.random_sample((channels, baselines)) < 0.1] = 0.0
    return dev


def degenerate_rows(channels, seed=5):
    """One baseline per awkward case (channel-major)."""
    rs = np.random.RandomState(seed=seed)
    n = channels
    cols = []

    def shuffled(col):
        return col[rs.permutation(n)]

    cols.append(np.zeros(n, np.float32))  # nothing non-zero: NaN
    one = np.zeros(n, np.float32)
    one[rs.randint(n)] = -3.25
    cols.append(one)  # a single non-zero value
    cols.append(np.full(n, 1.5, np.float32))  # constant row: every value in one bin
    cols.append(shuffled(np.where(np.arange(n) % 2 == 0, 1.5, -1.5).astype(np.float32)))
    for hi in (np.float32(2.0), np.nextafter(np.float32(1.0), np.float32(2.0)),
               np.float32(1.0) + np.float32(2.0**-14)):  # fmt: skip
        # two distinct values in another top bin / the same 22-bit prefix / another
        # middle digit, with the two middle values distinct (count even, split evenly) ...
        col = np.zeros(n, np.float32)
        m = (n - n % 2) // 2
        col[:m] = 1.0
        col[m : 2 * m] = hi
        cols.append(shuffled(col))
        # ... equal (one more of the upper value) and an odd count
        col = col.copy()
        col[m - 1] = hi
        cols.append(shuffled(col))
        col = col.copy()
        col[0] = 1.0
        col[2 * m - 1] = 0.0
        cols.append(shuffled(col))
    g = rs.standard_normal(n).astype(np.float32)
    for k in (0, 1, 2, 3):  # non-zero counts of each parity
        col = g.copy()
        col[rs.permutation(n)[: 1000 + k]] = 0.0
        cols.append(col)
    # denormals, -0.0 and +inf among ordinary values
    col = (rs.standard_normal(n) * 1e-39).astype(np.float32)
    col[rs.random_sample(n) < 0.05] = -0.0
    col[rs.random_sample(n) < 0.01] = np.inf
    cols.append(col)
    col = (rs.standard_normal(n) * 1e-40).astype(np.float32)  # all denormal
    cols.append(col)
    col = g.copy()
    col[rs.random_sample(n) < 0.3] = -np.inf  # many infinities around the median
    col[rs.random_sample(n) < 0.1] = -0.0
    cols.append(col)
    # heavily quantised data: a handful of distinct magnitudes
    cols.append(np.round(rs.standard_normal(n) * 4).astype(np.float32) / np.float32(4))
    cols.append(np.round(rs.standard_normal(n)).astype(np.float32))
    return np.stack(cols, axis=1)


class TestLongMADT:
    @pytest.mark.parametrize("baselines", [1, 3, 64])
    @pytest.mark.parametrize("channels", CHANNELS)
    def test_gaussian(self, channels, baselines, context, command_queue, oracle):
        dev = gaussian(channels, baselines, seed=channels + baselines)
        check(oracle, run_madt(context, command_queue, dev), dev)

    @pytest.mark.parametrize("channels", CHANNELS)
    def test_many_baselines(self, channels, context, command_queue, oracle):
        baselines = min(1000, (1 << 26) // channels)
        dev = gaussian(channels, baselines, seed=3)
        check(oracle, run_madt(context, command_queue, dev), dev)

    @pytest.mark.parametrize("pad", [1, 3, 4, 64])
    @pytest.mark.parametrize("channels", [16385, 32767, 38913, 131071])
    def test_padded_stride(self, channels, pad, context, command_queue, oracle):
        dev = gaussian(channels, 5, seed=pad)
        check(oracle, run_madt(context, command_queue, dev, pad=pad), dev)

    @pytest.mark.parametrize("channels", CHANNELS)
    def test_degenerate_rows(self, channels, context, command_queue, oracle):
        dev = degenerate_rows(channels)
        out = run_madt(context, command_queue, dev)
        check(oracle, out, dev)
        assert np.isnan(out[0]) and not np.isnan(out[1:]).any()

    @pytest.mark.parametrize("channels", [32768, 262144])
    def test_degenerate_rows_padded(self, channels, context, command_queue, oracle):
        dev = degenerate_rows(channels, seed=6)
        check(oracle, run_madt(context, command_queue, dev, pad=7), dev)


def run_sequence(context, queue, vis, flags, mode, width):
    from katsdpsigproc_amd.rfi import device

    template = device.FlaggerDeviceTemplate(
        device.BackgroundMedianFilterDeviceTemplate(context, width,
                                                    use_flags=device.BackgroundFlags[mode]),
        device.NoiseEstMADTDeviceTemplate(context, vis.shape[0]),
        device.ThresholdSumDeviceTemplate(context, 4),
    )  # fmt: skip
    fn = template.instantiate(queue, *vis.shape, threshold_args=dict(n_sigma=11.0))
    assert isinstance(fn, device.FlaggerDevice)
    fn.ensure_all_bound()
    fn.buffer("vis").set(queue, vis)
    if flags is not None:
        fn.buffer("input_flags").set(queue, flags)
    fn()
    return fn.buffer("flags").get(queue), fn.buffer("noise").get(queue)


def check_sequence(oracle, vis, flags, width, out_flags, out_noise):
    dev32 = oracle.BackgroundMedianFilterHost(width)(vis, flags).astype(np.float32)
    noise32 = oracle.NoiseEstMADHost()(dev32).astype(np.float32)
    expected = oracle.ThresholdSumHost(11.0, 4)(dev32, noise32)
    np.testing.assert_array_equal(noise32, out_noise)
    np.testing.assert_array_equal(expected, out_flags)
    assert expected.sum() > 0


class TestLongFlagger:
    @pytest.fixture(scope="class")
    def block(self):
        vis = inputs.add_rfi(inputs.generate_data(32768, 256, seed=11), seed=12)
        rs = np.random.RandomState(seed=13)
        flags = (rs.random_sample(vis.shape) < 1.0 / 16.0).astype(np.uint8)
        return vis, flags

    @pytest.mark.parametrize("mode", ["NONE", "CHANNEL", "FULL"])
    @pytest.mark.parametrize("width", [13, 63])
    def test_sequence(self, width, mode, block, context, command_queue, oracle):
        vis, full = block
        flags = {"NONE": None, "CHANNEL": np.ascontiguousarray(full[:, 0]), "FULL": full}[mode]
        out_flags, out_noise = run_sequence(context, command_queue, vis, flags, mode, width)
        check_sequence(oracle, vis, flags, width, out_flags, out_noise)

    @pytest.mark.parametrize("channels, baselines", [(65536, 32), (262144, 4)])
    def test_longer_bands(self, channels, baselines, context, command_queue, oracle):
        vis = inputs.add_rfi(inputs.generate_data(channels, baselines, seed=14), seed=15)
        out_flags, out_noise = run_sequence(context, command_queue, vis, None, "NONE", 13)
        check_sequence(oracle, vis, None, 13, out_flags, out_noise)
