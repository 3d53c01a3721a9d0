"""Preparing correlator dumps on the GPU (``rfi.ingest.PrepareTemplate``, ``ksp_prepare``):
every comparison is of bit patterns, against ``rfi.host.PrepareHost``. Nothing is left out:
the operation cannot produce a NaN."""

import ctypes

import numpy as np
import pytest

from tests import inputs
from tests.subviews import SENTINEL, CompactViews, flat_device_array, sentinel_array

pytestmark = pytest.mark.gpu

# A lane owns a run of 16 baselines of 4 adjacent rows (2 without weights), and the runs are dealt
# to 256-thread workgroups: a row ends in a partial run unless baselines is a multiple of 16, a
# wavefront spans 1024 baselines and a workgroup 4096; 1 and 7 channels end in a partial group of
# rows either way, 2 with weights.
WORKGROUP_COLS = 256 * 16
BASELINES = [1, 3, 15, 16, 17, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025,
             WORKGROUP_COLS - 1, WORKGROUP_COLS, WORKGROUP_COLS + 1]  # fmt: skip
CHANNELS = [1, 2, 7, 8]
LOST = -(2**31)
VARIANTS = [(False, False), (True, False), (False, True), (True, True)]  # (channel mask, weights)
SCALES = [1.0, 2.0**-8, float(np.float32(1.0 / 3.0)), 2.0**-140]
MAPS = ["identity", "reversal", "permutation", "one"]
N_AUTO = 6  # the first input baselines are the autocorrelations
INVALID = [-1, None, LOST, 2**31 - 1]  # (None: in_baselines, the first index past the end)


@pytest.fixture(scope="module")
def context():
    from katsdpsigproc_amd import accel

    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


def in_baselines_choices(baselines):
    return [1, baselines, baselines + 5, 2 * baselines]


def make_vis_in(rs, channels, in_baselines):
    """int32 (channels, in_baselines, 2): full-range values, about 5 % sentinels in re (and
    some in im alone, which are data), +-(2**31 - 1), values half way between two float32
    (odd multiples of 2**(e - 24) in [2**e, 2**(e + 1))), small values whose product with
    2**-140 is denormal; the first N_AUTO baselines are autocorrelations: mostly positive over
    the whole range, some zero, negative and lost."""
    shape = (channels, in_baselines)
    v = rs.randint(-(2**31) + 1, 2**31, shape + (2,), np.int64)
    kind = rs.random_sample(shape + (2,))
    e = rs.randint(24, 31, shape + (2,))
    ties = (2**e + (2 * rs.randint(0, 2**22, shape + (2,)) + 1) * 2 ** (e - 24))
    ties = ties * np.where(rs.random_sample(shape + (2,)) < 0.5, 1, -1)
    v = np.where(kind < 0.15, ties, v)
    v = np.where((kind >= 0.15) & (kind < 0.20), 2**31 - 1, v)
    v = np.where((kind >= 0.20) & (kind < 0.25), -(2**31) + 1, v)
    v = np.where((kind >= 0.25) & (kind < 0.35), rs.randint(-(2**12), 2**12, shape + (2,)), v)
    n_auto = min(N_AUTO, in_baselines)
    power = np.exp2(rs.uniform(0, 31, (channels, n_auto))).astype(np.int64)
    akind = rs.random_sample((channels, n_auto))
    power = np.where(akind < 0.08, 0, power)
    power = np.where((akind >= 0.08) & (akind < 0.16), -power, power)
    power = np.clip(power, -(2**31) + 1, 2**31 - 1)
    v[:, :n_auto, 0] = np.where((akind >= 0.16) & (akind < 0.24), LOST, power)
    v[:, :n_auto, 1] = 0
    v[..., 0] = np.where(rs.random_sample(shape) < 0.05, LOST, v[..., 0])
    v[..., 1] = np.where(rs.random_sample(shape) < 0.03, LOST, v[..., 1])
    return v.astype(np.int32)


def make_source(rs, kind, baselines, in_baselines):
    """Valid indices only: every map is taken modulo in_baselines."""
    j = np.arange(baselines)
    if kind == "identity":
        s = j % in_baselines
    elif kind == "reversal":
        s = (in_baselines - 1 - j) % in_baselines
    elif kind == "permutation":
        if in_baselines >= baselines:
            s = rs.permutation(in_baselines)[:baselines]
        else:
            s = rs.randint(0, in_baselines, baselines)
    else:
        s = np.full(baselines, int(rs.randint(0, in_baselines)))
    return s.astype(np.int32)


def make_auto_source(rs, baselines, in_baselines):
    return rs.randint(0, min(N_AUTO, in_baselines), (baselines, 2)).astype(np.int32)


def make_case(seed, channels, baselines, in_baselines, kind):
    rs = np.random.RandomState(seed)
    vis_in = make_vis_in(rs, channels, in_baselines)
    source = make_source(rs, kind, baselines, in_baselines)
    auto_source = make_auto_source(rs, baselines, in_baselines)
    channel_flags = np.where(rs.random_sample(channels) < 0.4,
                             rs.randint(1, 256, channels), 0).astype(np.uint8)  # fmt: skip
    return vis_in, source, channel_flags, auto_source


def assert_same(want, got, what=""):
    assert want.dtype == got.dtype and want.shape == got.shape, what
    if want.dtype == np.uint8:
        np.testing.assert_array_equal(want, got, err_msg=what)
        return
    want = np.ascontiguousarray(want).view(np.uint32)
    got = np.ascontiguousarray(got).view(np.uint32)
    bad = want != got
    assert not bad.any(), (
        f"{what}: {np.count_nonzero(bad)} of {bad.size} words differ, first at "
        f"{np.argwhere(bad)[0]}: want {want[bad][0]:#010x}, got {got[bad][0]:#010x}")  # fmt: skip


def write_padded(queue, array, data):
    """`data` into `array`, sentinel bytes into its padding."""
    raw = sentinel_array(array.padded_shape, array.dtype)
    raw[tuple(slice(0, n) for n in array.shape)] = data
    queue.enqueue_write_buffer(array.buffer, raw)


def read_checked(queue, array, name):
    """The data of `array`, after checking that its padding still holds the sentinel."""
    raw = np.empty(array.padded_shape, array.dtype)
    queue.enqueue_read_buffer(array.buffer, raw)
    padding = np.ascontiguousarray(raw[..., array.shape[-1] :]).view(np.uint8)
    assert np.all(padding == SENTINEL), f"wrote into the padding of {name}"
    return np.ascontiguousarray(raw[..., : array.shape[-1]])


def run_device(context, queue, case, variant, scale=1.0, lost_flag=8, weight_scale=1.0, pad=0):
    """(vis, input_flags, weights or None) of the operation; the outputs start out full of
    sentinel bytes, padding included, and every padding is checked afterwards."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import ingest

    vis_in, source, channel_flags, auto_source = case
    use_mask, use_weights = variant
    channels, in_baselines = vis_in.shape[:2]
    template = ingest.PrepareTemplate(context, scale, lost_flag, use_mask, use_weights, weight_scale)
    fn = template.instantiate(queue, channels, len(source), in_baselines)
    if pad:
        for name in ("vis_in", "vis", "input_flags", "weights"):
            if name in fn.slots:
                dim = fn.slots[name].dimensions[1]
                accel.Dimension(dim.size, min_padded_size=dim.size + pad).link(dim)
    fn.ensure_all_bound()
    outputs = ["vis", "input_flags"] + (["weights"] if use_weights else [])
    for name in outputs:
        assert fn.buffer(name).padded_shape[1] >= len(source) + pad
        write_padded(queue, fn.buffer(name), sentinel_array((1,), fn.buffer(name).dtype)[0])
    assert fn.buffer("vis_in").padded_shape[1] >= in_baselines + pad
    write_padded(queue, fn.buffer("vis_in"), vis_in)
    fn.buffer("source").set(queue, source)
    if use_mask:
        fn.buffer("channel_flags").set(queue, channel_flags)
    if use_weights:
        fn.buffer("auto_source").set(queue, auto_source)
    fn()
    got = [read_checked(queue, fn.buffer(name), name) for name in outputs]
    return got[0], got[1], (got[2] if use_weights else None)


def run_host(case, variant, scale=1.0, lost_flag=8, weight_scale=1.0):
    from katsdpsigproc_amd.rfi import host

    vis_in, source, channel_flags, auto_source = case
    use_mask, use_weights = variant
    return host.PrepareHost(scale, lost_flag, weight_scale)(
        vis_in, source, channel_flags if use_mask else None, auto_source if use_weights else None)


def compare(context, queue, case, variant, what, **kwargs):
    want = run_host(case, variant, **{k: v for k, v in kwargs.items() if k != "pad"})
    got = run_device(context, queue, case, variant, **kwargs)
    for name, w, g in zip(("vis", "input_flags", "weights"), want, got):
        if w is None:
            assert g is None
        else:
            assert_same(w, g, f"{name} {what} {variant} {kwargs}")
    return want


def test_data_covers_the_cases():
    """The generated dumps do contain what the tests are meant to exercise."""
    case = make_case(1, 8, 257, 262, "permutation")
    vis_in = case[0]
    assert 0.03 < np.mean(vis_in[..., 0] == LOST) < 0.08
    assert ((vis_in[..., 1] == LOST) & (vis_in[..., 0] != LOST)).any()
    assert (vis_in == 2**31 - 1).any() and (vis_in == -(2**31) + 1).any()
    big = np.abs(vis_in.astype(np.int64))
    big = big[(big >= 2**24) & (big < 2**31 - 1)]
    step = 2 ** (np.floor(np.log2(big)).astype(np.int64) - 23)  # float32 spacing at that size
    assert np.count_nonzero(big % step == step // 2) > 0.1 * vis_in.size  # exact ties
    autos = vis_in[:, :N_AUTO, 0]
    assert (autos > 0).any() and (autos == 0).any() and (autos < 0).any() and (autos == LOST).any()
    vis, flags, weights = run_host(case, (True, True), scale=2.0**-140)
    tiny = np.abs(vis.real[vis.real != 0])
    assert (tiny < np.finfo(np.float32).tiny).any()  # denormal products
    vis, flags, weights = run_host(case, (True, True), scale=2.0**-8, weight_scale=2.0**20)
    assert (weights == 0).any() and (weights > 0).any() and np.isfinite(weights).all()
    assert (flags & 8).any() and (flags & ~np.uint8(8)).any()


@pytest.mark.parametrize("channels", CHANNELS)
def test_shapes(channels, context, command_queue):
    """Every width with every kernel variant; in_baselines, map and scale are drawn (the
    next test crosses them)."""
    rs = np.random.RandomState(channels)
    for baselines in BASELINES:
        for variant in VARIANTS:
            in_baselines = in_baselines_choices(baselines)[rs.randint(4)]
            kind = MAPS[rs.randint(4)]
            scale = SCALES[rs.randint(4)]
            case = make_case(channels * 10007 + baselines, channels, baselines, in_baselines, kind)
            compare(context, command_queue, case, variant,
                    f"{channels}x{baselines} from {in_baselines} ({kind})", scale=scale,
                    weight_scale=2.0**20)  # fmt: skip


@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("scale", SCALES)
def test_maps_scales_and_input_sizes(scale, kind, context, command_queue):
    for channels, baselines in [(7, 65), (8, 1025)]:
        for in_baselines in in_baselines_choices(baselines):
            case = make_case(baselines + in_baselines, channels, baselines, in_baselines, kind)
            for variant in ((False, False), (True, True)):
                compare(context, command_queue, case, variant,
                        f"{channels}x{baselines} from {in_baselines} ({kind})", scale=scale,
                        lost_flag=0x81, weight_scale=3.0)  # fmt: skip


@pytest.mark.parametrize("variant", VARIANTS)
def test_tall(variant, context, command_queue):
    """More rows than a grid dimension of 65535 could number."""
    case = make_case(70000, 70000, 3, 8, "permutation")
    compare(context, command_queue, case, variant, "70000x3", scale=2.0**-8)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("channels, baselines, pad", [(8, 65, 29), (7, 1025, 3), (5, 256, 16)])
def test_padding(channels, baselines, pad, variant, context, command_queue):
    """Rows padded beyond what the slots ask for, the input's as well; run_device looks at the
    sentinels in the padding of all three outputs."""
    case = make_case(pad, channels, baselines, baselines + 5, "permutation")
    compare(context, command_queue, case, variant, f"pad {pad}", scale=2.0**-8, pad=pad)


ALIGNED_STRIDES = {"vis_in": 24, "vis": 42, "input_flags": 48, "weights": 44}
ODD_STRIDES = {"vis_in": 23, "vis": 41, "input_flags": 39, "weights": 43}


@pytest.mark.parametrize("variant", [(False, False), (True, True)])
@pytest.mark.parametrize("offset, strides", [(1, ODD_STRIDES), (4, ODD_STRIDES), (12, ODD_STRIDES),
                                             (16, ALIGNED_STRIDES)])  # fmt: skip
def test_raw_abi_subviews(offset, strides, variant, context, command_queue):
    """Sub-views: pointers `offset` elements into their allocations and a stride of its own
    per array. Odd strides take the element-wise path (offset 1 leaves vis_in on an odd
    multiple of 4 bytes); 16 elements and strides that keep the rows on 16 bytes take the
    16-byte path from the middle of an allocation."""
    check_raw_abi(offset, strides, variant, 37, False, context, command_queue)


@pytest.mark.parametrize("variant", [(False, False), (True, True)])
@pytest.mark.parametrize("baselines", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("offset, strides", [(1, ODD_STRIDES), (16, ALIGNED_STRIDES)])
def test_raw_abi_subviews_ragged(offset, strides, baselines, variant, context, command_queue):
    """The same at the widths around a run of 16 (no run, a run short of one baseline, a whole
    run, runs followed by one baseline), 4 bytes off and aligned, with indices outside the
    input in the last baseline: the last element of a ragged run that is there. (What makes
    that safe to run is said in front of test_invalid_indices.)"""
    check_raw_abi(offset, strides, variant, baselines, True, context, command_queue)


def check_raw_abi(offset, strides, variant, baselines, invalid_last, context, command_queue,
                  views=None):
    """`views` makes the strided arrays (tests/subviews.py: CompactViews unless given) and may
    choose other strides of the same kind."""
    from katsdpsigproc_amd import _lib

    queue = command_queue
    views = views or CompactViews(context, queue)
    # vis_in as rows of int32: a pair stride of n is a row stride of 2 n words
    strides = dict(strides, vis_in=2 * strides["vis_in"])

    def make(name, dtype, data, poison=False):
        """(view, pointer); the stride the launcher gets is the one the view was made with"""
        made = views(name, dtype, data, strides[name], offset, poison)
        strides[name] = made[0].stride
        return made

    channels, in_baselines = 6, 21
    use_mask, use_weights = variant
    case = list(make_case(offset, channels, baselines, in_baselines, "permutation"))
    if invalid_last:
        case[1][-1] = in_baselines
        case[3][-1] = [-1, 2**31 - 1]
    vis_in, source, channel_flags, auto_source = case
    d_in = make("vis_in", np.int32, vis_in.reshape(channels, -1), poison=True)
    assert strides["vis_in"] % 2 == 0
    d_source = flat_device_array(context, queue, np.int32, source[np.newaxis, :], baselines,
                                 offset, poison=True)  # fmt: skip
    d_auto = flat_device_array(context, queue, np.int32, auto_source.reshape(1, -1),
                               2 * baselines, offset, poison=True)  # fmt: skip
    d_mask = flat_device_array(context, queue, np.uint8, channel_flags[np.newaxis, :], channels,
                               offset, poison=True)  # fmt: skip
    dtypes = {"vis": np.complex64, "input_flags": np.uint8, "weights": np.float32}
    out = {name: make(name, dtype, sentinel_array((channels, baselines), dtype))
           for name, dtype in dtypes.items()}  # fmt: skip
    null = ctypes.c_void_p(0)
    _lib.call("ksp_prepare", context.device.index, ctypes.c_void_p(queue.stream), d_in[1],
              d_source[1], d_auto[1] if use_weights else null, d_mask[1] if use_mask else null,
              out["vis"][1], out["input_flags"][1], out["weights"][1] if use_weights else null,
              channels, in_baselines, baselines, strides["vis_in"] // 2, strides["vis"],
              strides["input_flags"], strides["weights"], 2.0**-8, 2.0**20, 0x10)  # fmt: skip
    want = run_host(case, variant, scale=2.0**-8, lost_flag=0x10, weight_scale=2.0**20)
    for name, w in zip(dtypes, want):
        got = out[name][0].read(name)
        if w is None:  # no weights: nothing at all was written to that allocation
            assert np.all(got.view(np.uint8) == SENTINEL)
        else:
            assert_same(w, got, f"{name} at offset {offset}")
    for view in (d_in, d_source, d_auto, d_mask):
        view[0].read("an input")  # (asserts that nothing wrote to it)


def test_host_from_device(context, command_queue):
    from katsdpsigproc_amd.rfi import host, ingest

    case = make_case(11, 12, 70, 90, "permutation")
    vis_in, source, channel_flags, auto_source = case
    for use_mask, use_weights in VARIANTS:
        template = ingest.PrepareTemplate(context, 2.0**-8, 0x40, use_mask, use_weights, 2.0**20)
        args = (vis_in, source, channel_flags if use_mask else None,
                auto_source if use_weights else None)  # fmt: skip
        got = ingest.PrepareHostFromDevice(template, command_queue)(*args)
        want = host.PrepareHost(2.0**-8, 0x40, 2.0**20)(*args)
        assert (got[2] is None) == (not use_weights)
        for name, w, g in zip(("vis", "input_flags", "weights"), want, got):
            if w is not None:
                assert_same(w, g, name)


def chain_dump(seed, channels, in_baselines):
    """Integer noise of amplitude about 1e5 with spikes of 5e6 to 7e6, autocorrelations around
    1e6 in the first N_AUTO baselines, and about 3 % lost samples."""
    rs = np.random.RandomState(seed)
    noise = inputs.generate_data(channels, in_baselines, seed=seed)
    vis = inputs.add_rfi(noise, seed=seed + 100)
    vis_in = np.empty((channels, in_baselines, 2), np.int32)
    vis_in[..., 0] = np.rint(vis.real * 1e5)
    vis_in[..., 1] = np.rint(vis.imag * 1e5)
    vis_in[rs.random_sample((channels, in_baselines)) < 0.03, 0] = LOST
    vis_in[:, :N_AUTO, 0] = 1000000 + np.rint(noise.real[:, :N_AUTO] * 1e5)  # (no spikes, none lost)
    vis_in[:, :N_AUTO, 1] = 0
    return vis_in


def test_in_front_of_the_chain(context, command_queue):
    """Three dumps through prepare -> fused flagger -> accumulate -> finalise in one sequence,
    `vis`, `input_flags` and `weights` shared, against PrepareHost + FlaggerHost + AveragerHost."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import device, host, ingest

    queue = command_queue
    channels, baselines, in_baselines, cf = 64, 40, 50, 4
    full = device.BackgroundFlags.FULL
    scale, lost_flag, weight_scale = 2.0**-8, 0x08, 2.0**24
    prepare = ingest.PrepareTemplate(context, scale, lost_flag, True, True, weight_scale).instantiate(
        queue, channels, baselines, in_baselines)  # fmt: skip
    flagger = device.FlaggerDeviceTemplate(
        device.BackgroundMedianFilterDeviceTemplate(context, 13, use_flags=full),
        device.NoiseEstMADTDeviceTemplate(context, channels),
        device.ThresholdSumDeviceTemplate(context),
        fused=True, tuning={"vis_pad": 0},
    ).instantiate(queue, channels, baselines, threshold_args={"n_sigma": 11.0})
    assert isinstance(flagger, device.FusedFlaggerDevice)
    accumulate = device.AccumulateTemplate(context, use_weights=True, input_flags=full).instantiate(
        queue, channels, baselines)  # fmt: skip
    finalise = device.FinaliseTemplate(context, channel_factor=cf).instantiate(
        queue, channels, baselines)  # fmt: skip
    acc = ("acc_vis", "acc_weights", "acc_flags")
    compounds = {
        "vis": ["prepare:vis", "flagger:vis", "accumulate:vis"],
        "input_flags": ["prepare:input_flags", "flagger:input_flags", "accumulate:input_flags"],
        "weights": ["prepare:weights", "accumulate:weights"],
        "flags": ["flagger:flags", "accumulate:flags"],
    }
    compounds.update({name: ["accumulate:" + name, "finalise:" + name] for name in acc})
    seq = accel.OperationSequence(
        queue, [("prepare", prepare), ("flagger", flagger), ("accumulate", accumulate),
                ("finalise", finalise)], compounds=compounds)  # fmt: skip
    for name in device.FusedFlaggerDevice._OPTIONAL:
        del seq.slots["flagger:" + name]
    seq.ensure_all_bound()
    for name in acc:
        seq.buffer(name).zero(queue)
    rs = np.random.RandomState(9)
    source = rs.permutation(in_baselines)[:baselines].astype(np.int32)
    auto_source = rs.randint(0, N_AUTO, (baselines, 2)).astype(np.int32)
    mask = inputs.channel_mask(channels, seed=4, fraction=1.0 / 8.0) * np.uint8(0x20)
    assert mask.any() and not mask.all()
    seq.buffer("prepare:source").set(queue, source)
    seq.buffer("prepare:auto_source").set(queue, auto_source)
    seq.buffer("prepare:channel_flags").set(queue, mask)
    prepare_host = host.PrepareHost(scale, lost_flag, weight_scale)
    flagger_host = host.FlaggerHost(host.BackgroundMedianFilterHost(13), host.NoiseEstMADHost(),
                                    host.ThresholdSumHost(11.0))  # fmt: skip
    averager = host.AveragerHost(channels, baselines, cf, full)

    def host_dump(vis_in):
        vis, input_flags, weights = prepare_host(vis_in, source, mask, auto_source)
        flags = flagger_host(vis, input_flags)
        averager.add(vis, flags, weights, input_flags=input_flags)
        return vis, input_flags, weights, flags

    flagged = lost = 0
    for d in range(3):
        vis_in = chain_dump(20 + d, channels, in_baselines)
        seq.buffer("prepare:vis_in").set(queue, vis_in)
        prepare()
        flagger()
        accumulate()
        want = host_dump(vis_in)
        for name, w in zip(("vis", "input_flags", "weights", "flags"), want):
            assert_same(w, seq.buffer(name).get(queue), f"{name}, dump {d}")
        flagged += np.count_nonzero(want[3])
        lost += np.count_nonzero(want[1] & lost_flag)
        assert np.all((want[2] > 0.1) & (want[2] < 10))  # weights of order 1
    assert flagged > 0 and lost > 0
    finalise()
    want = averager.finalise()
    out = ("vis", "weights", "flags")
    for name, w in zip(out, want):
        assert_same(w, seq.buffer("finalise:" + name).get(queue), name)
    # spikes were left out of every output that had unflagged data: the averages are noise of
    # about 400, not the 2e4 of the spikes
    clean = (want[2] == 0) & (source >= N_AUTO)[np.newaxis, :]
    assert clean.any() and np.abs(want[0][clean]).max() < 4000
    # and once more through the sequence as a whole
    vis_in = chain_dump(40, channels, in_baselines)
    seq.buffer("prepare:vis_in").set(queue, vis_in)
    seq()
    host_dump(vis_in)
    for name, w in zip(out, averager.finalise()):
        assert_same(w, seq.buffer("finalise:" + name).get(queue), name)


# The test below puts indices outside 0 .. in_baselines - 1 into source and auto_source. The
# result is defined (a lost sample, a power of 0), and what makes it safe to run is
# prep_clamp() of csrc/prepare.hip: an index is compared as an unsigned number with
# in_baselines and replaced by 0 before any address is formed from it, on the 16-byte path
# and on the element-wise one.
@pytest.mark.parametrize("variant", VARIANTS)
def test_invalid_indices(variant, context, command_queue):
    for channels, baselines, in_baselines in [(7, 65, 70), (8, 1025, 1025), (3, 16, 1), (5, 4097, 9000)]:
        case = list(make_case(baselines, channels, baselines, in_baselines, "permutation"))
        rs = np.random.RandomState(baselines)
        invalid = np.array([in_baselines if v is None else v for v in INVALID], np.int32)
        source, auto_source = case[1].copy(), case[3].copy()
        hit = rs.random_sample(baselines) < 0.3
        hit[: len(invalid)] = True
        hit[-1] = True  # the last element of the row's last run, ragged or not
        source[hit] = invalid[np.arange(np.count_nonzero(hit)) % len(invalid)]
        hit = rs.random_sample((baselines, 2)) < 0.3
        hit[-1:] = True
        auto_source[hit] = invalid[np.arange(np.count_nonzero(hit)) % len(invalid)]
        case[1], case[3] = source, auto_source
        want = compare(context, command_queue, case, variant, f"invalid {channels}x{baselines}",
                       scale=2.0**-8, weight_scale=2.0**20)  # fmt: skip
        bad = (source < 0) | (source >= in_baselines)
        assert bad[:4].all() and not want[0][:, bad].any() and (want[1][:, bad] & 8).all()
        if want[2] is not None:
            assert not want[2][:, hit.any(axis=1)].any()
