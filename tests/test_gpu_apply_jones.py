"""Applying Jones matrices on the GPU (``rfi.ingest.ApplyJonesTemplate``, ``ksp_apply_jones``):
every comparison is of bit patterns, against ``rfi.host.ApplyJonesHost``, with nothing left out
but the payload of a NaN that the host has as a NaN too. A baseline that no quad names must
come back untouched: the sentinel out of place, the input in place."""

import ctypes

import numpy as np
import pytest

from tests import inputs_apply_jones as gen
from tests.inputs_apply_jones import assert_same
from tests.subviews import CompactViews, poison_array, sentinel_array
from tests.test_gpu_prepare import N_AUTO
from tests.test_gpu_solve_jones import CHAIN, CHAIN_NOISE, ChainHost
from tests.test_solve_jones import ACCURACY_BOUND

pytestmark = pytest.mark.gpu

# The sizes at which csrc/apply_jones.hip changes path (aj_make_geometry, aj_stage_rows). A
# lane owns a quad and a workgroup has THREADS lanes. A tile is the narrowest power of two of
# quads that holds the table, at most THREADS: the tile width changes at 1, 2, 4, ... 256 quads
# and stays 256 from there on, so tables beyond 256, 512, ... quads take one more tile. The
# THREADS / tile width lanes that share a quad take different rows, and a workgroup's chunk of
# rows is at least that many (256 rows for one quad, 64 for up to 4, one for 256 or more). A
# stage holds stage_rows(n_inputs) rows of jones in LDS_ROWS = 2048 slots of 16 bytes, so with
# short tables a workgroup walks several stages.
THREADS = 256
LDS_ROWS = 2048
TILE_WIDTHS = [1 << k for k in range(9)]  # 1 .. 256


def stage_rows(n_inputs):
    return min(THREADS, LDS_ROWS // n_inputs)


def geometry(channels, n_quads, target=1024):
    """(tile width, tiles, chunk of rows, workgroups) of a launch."""
    width = next(w for w in TILE_WIDTHS if w >= min(n_quads, THREADS))
    tiles = -(-n_quads // width)
    slots = THREADS // width
    chunk = max(slots, min(channels, channels * tiles // target // slots * slots))
    return width, tiles, chunk, -(-channels // chunk) * tiles


N_QUADS = sorted({1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1025}
                 | {max(w + d, 1) for w in TILE_WIDTHS + [2 * THREADS] for d in (-1, 0, 1)})  # fmt: skip
CHANNELS = [1, 2, 7, 8]
N_INPUTS = [2, 4, 6, 34, 64, 66, 2046, 2048]
VARIANTS = [(True, True), (True, False), (False, True), (False, False)]
NAMES = ("out_vis", "out_weights", "out_flags")
KINDS = ("vis", "weights", "flags")
DTYPES = {"vis": np.complex64, "weights": np.float32, "flags": np.uint8}
TABLES = ("jones", "quad_antennas", "quads")
BIG_ANT = 45  # 1035 quads, 4095 baselines: room for every entry of N_QUADS
f32 = np.float32


@pytest.fixture(scope="module")
def context():
    from katsdpsigproc_amd import accel

    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


def want_of(case, weights, flags, flag_value=128):
    from katsdpsigproc_amd.rfi import host

    return host.ApplyJonesHost(flag_value)(
        case["vis"], case["jones"], case["quad_antennas"], case["quads"],
        case["weights"] if weights else None, case["flags"] if flags else None)  # fmt: skip


def hostile(padded_shape, dtype):
    """What the padding of an input holds: NaN, or bytes of 0xFF."""
    return poison_array(int(np.prod(padded_shape)), dtype).reshape(padded_shape)


def kinds_of(weights, flags):
    return ["vis"] + (["weights"] if weights else []) + (["flags"] if flags else [])


def run_device(context, queue, case, weights, flags, in_place, flag_value=128, pad=0):
    """The operation's outputs, whole rows of `baselines` each, as a dict by kind. The padding
    of the inputs holds NaN or 0xFF; the outputs start out full of sentinel bytes. Afterwards
    every byte of padding is what it was, and so is every byte of the tables and, out of place,
    of the inputs."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import ingest

    channels, baselines = case["vis"].shape
    n_inputs = case["jones"].shape[1]
    template = ingest.ApplyJonesTemplate(context, weights=weights, flags=flags, flag_value=flag_value)
    fn = template.instantiate(queue, channels, baselines, n_inputs, len(case["quads"]))
    kinds = kinds_of(weights, flags)
    for kind in kinds:
        dim = fn.slots[kind].dimensions[1]
        if pad:
            accel.Dimension(dim.size, min_padded_size=dim.size + pad).link(dim)
            out = fn.slots["out_" + kind].dimensions[1]
            accel.Dimension(dim.size, min_padded_size=dim.size + 2 * pad).link(out)
        if in_place:
            dim.link(fn.slots["out_" + kind].dimensions[1])
    if pad:
        dim = fn.slots["jones"].dimensions[1]
        accel.Dimension(dim.size, min_padded_size=dim.size + pad).link(dim)
    fn.ensure_all_bound()
    if in_place:
        fn.bind(**{"out_" + kind: fn.buffer(kind) for kind in kinds})
    uploaded = {}
    for name in kinds + list(TABLES):
        d = fn.buffer(name)
        width = case[name].shape[1]
        assert d.padded_shape[1] >= width + (pad if name in kinds + ["jones"] else 0)
        assert d.padded_shape[2:] == case[name].shape[2:]
        raw = hostile(d.padded_shape, d.dtype)
        raw[: case[name].shape[0], :width] = case[name]
        queue.enqueue_write_buffer(d.buffer, raw)
        uploaded[name] = raw
    if not in_place:
        for kind in kinds:
            d = fn.buffer("out_" + kind)
            queue.enqueue_write_buffer(d.buffer, sentinel_array(d.padded_shape, d.dtype))
    fn()
    out = {}
    for kind in kinds:
        d = fn.buffer("out_" + kind)
        raw = np.empty(d.padded_shape, d.dtype)
        queue.enqueue_read_buffer(d.buffer, raw)
        padding = np.ones(d.padded_shape, bool)
        padding[:channels, :baselines] = False
        before = uploaded[kind] if in_place else sentinel_array(d.padded_shape, d.dtype)
        same = raw.view(np.uint8) == before.view(np.uint8)
        assert same[np.repeat(padding, d.dtype.itemsize, axis=1)].all(), \
            f"wrote into the padding of out_{kind}"  # fmt: skip
        out[kind] = np.ascontiguousarray(raw[:channels, :baselines])
    for name, before in uploaded.items():
        if in_place and name in kinds:
            continue
        d = fn.buffer(name)
        raw = np.empty(d.padded_shape, d.dtype)
        queue.enqueue_read_buffer(d.buffer, raw)
        assert (raw.view(np.uint8) == before.view(np.uint8)).all(), f"{name} was modified"
    return out


def assert_outputs(case, want, got, kinds, in_place, what):
    """`got` (by kind, whole rows) is `want` at the baselines a quad names, and untouched at
    the others: the input in place, the sentinel out of place."""
    cover = gen.covered(case["quads"], case["vis"].shape[1])
    for kind, w in zip(KINDS, want):
        assert (w is not None) == (kind in kinds), kind
        if w is None:
            continue
        g = got[kind]
        assert_same(np.ascontiguousarray(w[:, cover]), np.ascontiguousarray(g[:, cover]),
                    f"out_{kind} {what}")  # fmt: skip
        rest = np.ascontiguousarray(g[:, ~cover])
        before = (np.ascontiguousarray(case[kind][:, ~cover]) if in_place
                  else sentinel_array(rest.shape, rest.dtype))  # fmt: skip
        assert (rest.view(np.uint8) == before.view(np.uint8)).all(), \
            f"out_{kind} {what}: a baseline in no quad was written"  # fmt: skip


def compare(context, queue, case, weights, flags, in_place, what, flag_value=128, pad=0):
    want = want_of(case, weights, flags, flag_value)
    got = run_device(context, queue, case, weights, flags, in_place, flag_value, pad)
    assert_outputs(case, want, got, kinds_of(weights, flags), in_place, what)
    return want


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("weights, flags", VARIANTS)
def test_n_quads(weights, flags, in_place, context, command_queue):
    """Every table length around a tile width, on the first quads of one large layout (the
    other baselines are then in no quad), with the channels and the baseline order rotating."""
    seen = set()
    for i, n_quads in enumerate(N_QUADS):
        channels = CHANNELS[i % len(CHANNELS)]
        order = gen.ORDERS[i % len(gen.ORDERS)]
        case = gen.make_case(100 + i, channels, BIG_ANT, order, gen.DISHES[i % 3], n_quads=n_quads)
        seen.add(geometry(channels, n_quads)[:2])
        compare(context, command_queue, case, weights, flags, in_place,
                f"{channels} channels, {n_quads} quads, {order}")  # fmt: skip
    assert {width for width, _ in seen} == set(TILE_WIDTHS)
    assert {tiles for _, tiles in seen} >= {1, 2, 3, 4, 5}


@pytest.mark.parametrize("n_inputs", N_INPUTS)
def test_n_inputs_and_stages(n_inputs, context, command_queue):
    """A few quads among many inputs, and rows around the end of a stage and of a workgroup's
    chunk: with 12 quads (tiles of 16: chunks of 16 rows) and with 3 (tiles of 4: 64 rows)."""
    rows = stage_rows(n_inputs)
    assert rows == {2: 256, 4: 256, 6: 256, 34: 60, 64: 32, 66: 31, 2046: 1, 2048: 1}[n_inputs]
    channels_list = sorted(set(CHANNELS) | {max(rows + d, 1) for d in (-1, 0, 1)}
                           | {2 * rows + 1, 15, 16, 17, 63, 64, 65})  # fmt: skip
    for i, channels in enumerate(channels_list):
        for n_quads in (12, 3):
            weights, flags = VARIANTS[i % 4]
            case = gen.make_sparse_case(77 * channels + n_quads, channels, n_inputs, n_quads)
            compare(context, command_queue, case, weights, flags, bool(i % 2),
                    f"{channels} channels, {n_inputs} inputs, {len(case['quads'])} quads")  # fmt: skip


@pytest.mark.parametrize("n_ant", gen.ANTENNAS)
@pytest.mark.parametrize("order", gen.ORDERS)
def test_layouts(order, n_ant, context, command_queue):
    """Every layout in every baseline order, the three ways of listing a dish's cross hands,
    clean tables and spoilt ones, and baselines behind the layout that no quad names."""
    for i, dish in enumerate(gen.DISHES):
        for spoil in (False, True):
            case = gen.make_case(7 * n_ant + i, 9, n_ant, order, dish, spoil=spoil, extra=3 * i)
            if order == "random" and n_ant >= 3 and not spoil:
                assert (case["quads"] < 0).any()
            weights, flags = VARIANTS[(i + spoil) % 4]
            compare(context, command_queue, case, weights, flags, bool((i + n_ant) % 2),
                    f"{n_ant} antennas, {order}, {dish}, spoil {spoil}")  # fmt: skip


@pytest.mark.parametrize("kind", gen.SPOILS)
def test_spoils(kind, context, command_queue):
    """Each way of spoiling a table on its own, and the other flag values."""
    case = gen.make_case(5, 20, 17, "random", "one", spoil=(kind,), flag_value=1)
    assert (case["flags"] & 1).any()
    want = compare(context, command_queue, case, True, True, False, kind, flag_value=1)
    assert (want[2] != case["flags"]).any()  # samples that got the bit
    case = gen.make_case(6, 9, 4, "adjacent", "both", spoil=(kind,), flag_value=255)
    compare(context, command_queue, case, True, True, True, kind, flag_value=255)


@pytest.mark.parametrize("channels, n_ant, pad", [(8, 3, 29), (7, 17, 3), (5, 4, 16), (70, 1, 40),
                                                  (3, 32, 35)])  # fmt: skip
@pytest.mark.parametrize("in_place", [False, True])
def test_padding(channels, n_ant, pad, in_place, context, command_queue):
    """Rows padded beyond what the slots ask for, `pad` elements for the inputs and the
    matrices and twice that for the outputs (so the strides differ); run_device checks every
    byte of padding and, out of place, of the inputs."""
    case = gen.make_case(pad, channels, n_ant, "random", "one", spoil=True, extra=2)
    for weights, flags in VARIANTS:
        compare(context, command_queue, case, weights, flags, in_place, f"pad {pad}", pad=pad)


def odd_strides(baselines, n_inputs):
    return [(baselines + k) | 1 for k in (6, 2, 4, 8, 10, 12)], (n_inputs + 2) | 1


@pytest.mark.parametrize("channels, n_ant", [(6, 3), (3, 32), (70, 1), (9, 17)])
@pytest.mark.parametrize("offset", [1, 3, 16])
def test_raw_abi_subviews(offset, channels, n_ant, context, command_queue):
    """Sub-views: the sample pointers `offset` elements into their allocations and an odd
    stride of its own per array; `jones` one row (16 bytes) into its allocation with an odd
    stride. The variants rotate; in place and out of place both."""
    from katsdpsigproc_amd import _lib

    queue = command_queue
    views = CompactViews(context, queue)
    seed = 31 * offset + n_ant
    weights, flags = VARIANTS[seed % 4]
    case = gen.make_case(seed, channels, n_ant, gen.ORDERS[seed % 3], "one", spoil=True, extra=1)
    baselines, n_inputs = case["vis"].shape[1], 2 * n_ant
    data_strides, jones_stride = odd_strides(baselines, n_inputs)
    want = want_of(case, weights, flags)
    kinds = kinds_of(weights, flags)
    stride_of = dict(zip(("vis", "weights", "flags", "out_vis", "out_weights", "out_flags"),
                         data_strides))  # fmt: skip
    # a row of jones as two complex64: the view counts complex64, the launcher rows
    flat_jones = case["jones"].reshape(channels, 2 * n_inputs)
    d_jones = views("jones", np.complex64, flat_jones, 2 * jones_stride, 2, poison=True)
    d_ants = views("quad_antennas", np.int32, case["quad_antennas"], 2, 0, poison=True)
    d_quads = views("quads", np.int32, case["quads"], 4, 0, poison=True)
    for in_place in (False, True):
        d_in, d_out = {}, {}
        for kind in kinds:
            # in place the array is an output: sentinels around it instead of poison
            d_in[kind] = views(kind, DTYPES[kind], case[kind], stride_of[kind], offset,
                               poison=not in_place)  # fmt: skip
            if in_place:
                d_out[kind] = d_in[kind]
            else:
                blank = sentinel_array((channels, baselines), DTYPES[kind])
                d_out[kind] = views("out_" + kind, DTYPES[kind], blank, stride_of["out_" + kind],
                                    offset, poison=False)  # fmt: skip

        def ptr(views, kind):
            return views[kind][1] if kind in views else None

        def stride(views, kind):
            return views[kind][0].stride if kind in views else 0

        _lib.call("ksp_apply_jones", context.device.index, ctypes.c_void_p(queue.stream),
                  ptr(d_in, "vis"), ptr(d_in, "weights"), ptr(d_in, "flags"), d_jones[1],
                  d_ants[1], d_quads[1], ptr(d_out, "vis"), ptr(d_out, "weights"),
                  ptr(d_out, "flags"), channels, baselines, n_inputs, len(case["quads"]),
                  stride(d_in, "vis"), stride(d_in, "weights"), stride(d_in, "flags"),
                  jones_stride, stride(d_out, "vis"), stride(d_out, "weights"),
                  stride(d_out, "flags"), 128)  # fmt: skip
        got = {kind: d_out[kind][0].read("out_" + kind) for kind in kinds}  # (checks the margins)
        assert_outputs(case, want, got, kinds, in_place, f"at {offset}, in place {in_place}")
        if not in_place:
            for kind in kinds:
                d_in[kind][0].read(kind)  # (asserts that nothing wrote to it)
    for view, name in ((d_jones, "jones"), (d_ants, "quad_antennas"), (d_quads, "quads")):
        view[0].read(name)


def test_more_workgroups_than_compute_units(context, command_queue):
    """300 channels x 32 antennas: 528 quads in 3 tiles, chunks of one row: 900 workgroups."""
    assert geometry(300, 528) == (256, 3, 1, 900)
    case = gen.make_case(300, 300, 32, "blocks", "one", spoil=True)
    compare(context, command_queue, case, True, True, False, "300 x 32 antennas")
    compare(context, command_queue, case, True, True, True, "300 x 32 antennas in place")


def test_host_from_device(context, command_queue):
    """The adapter builds the table and passes the baselines of no quad through."""
    from katsdpsigproc_amd.rfi import host, ingest

    case = gen.make_case(11, 12, 4, "random", "one", extra=3)
    quad_antennas, quads = host.ApplyJonesHost.quad_table(case["inputs"], 8)
    assert (quads == case["quads"]).all() and not gen.covered(quads, len(case["inputs"]))[-3:].any()
    for weights, flags in VARIANTS:
        template = ingest.ApplyJonesTemplate(context, weights=weights, flags=flags, flag_value=2)
        adapter = ingest.ApplyJonesHostFromDevice(template, command_queue)
        got = adapter(case["vis"], case["jones"], case["inputs"],
                      case["weights"] if weights else None, case["flags"] if flags else None)  # fmt: skip
        for name, w, g in zip(NAMES, want_of(case, weights, flags, 2), got):
            assert (w is None) == (g is None)
            if w is not None:
                assert_same(w, g, name)


# ------------------------------------------------------------------------------ the chain
#: the largest |out_vis - I| over the unflagged samples between dishes, in units of
#: CHAIN_NOISE, measured on the host classes alone (the figures :func:`chain_host` prints:
#: 1.248 after three dumps, 1.881 after the fourth, every one of the 384 samples unflagged both
#: times); the test asserts twice the larger
APPLY_CHAIN_MEASURED_FACTOR = 1.89
CHAIN_FLAG = 0x40


class ApplyChainHost(ChainHost):
    """The host chain of tests/test_gpu_solve_jones.py on a layout with the autocorrelations
    of all eight inputs, with ApplyJonesHost and CompressWeightsHost behind the solve."""

    def __init__(self):
        from katsdpsigproc_amd.rfi import device, host

        self.n_inputs = n_inputs = 8
        rs = np.random.RandomState(9)
        cross = np.array(np.triu_indices(n_inputs, 1)).T
        cross = cross[rs.permutation(len(cross))]
        swap = (rs.random_sample(len(cross)) < 0.5) & (cross[:, 0] // 2 != cross[:, 1] // 2)
        cross[swap] = cross[swap][:, ::-1]
        autos = np.repeat(np.arange(n_inputs)[:, np.newaxis], 2, axis=1)
        self.ants = np.ascontiguousarray(np.concatenate([cross[:20], autos, cross[20:]]), np.int32)
        self.baselines = len(self.ants)
        self.in_baselines = 60
        self.source = (N_AUTO + rs.permutation(self.in_baselines - N_AUTO)[: self.baselines]).astype(
            np.int32)  # fmt: skip
        self.auto_source = rs.randint(0, N_AUTO, (self.baselines, 2)).astype(np.int32)
        from tests import inputs_solve_jones

        self.truth = inputs_solve_jones.make_jones(5, 1, n_inputs, span=1.0)[0].astype(np.complex128)
        self.pairs = host.SolveJonesHost.pair_table(self.ants, n_inputs)
        self.quad_antennas, self.quads = host.ApplyJonesHost.quad_table(self.ants, n_inputs)
        self.prepare = host.PrepareHost(1 / CHAIN["unit"], CHAIN["lost_flag"], CHAIN["weight_scale"])
        self.flagger = host.FlaggerHost(host.BackgroundMedianFilterHost(13), host.NoiseEstMADHost(),
                                        host.ThresholdSumHost(11.0))  # fmt: skip
        self.averager = host.AveragerHost(CHAIN["channels"], self.baselines, CHAIN["cf"],
                                          device.BackgroundFlags.FULL)  # fmt: skip
        self.solve = host.SolveJonesHost(CHAIN["max_iterations"], corrections=True)
        self.apply = host.ApplyJonesHost(CHAIN_FLAG)
        self.compress = host.CompressWeightsHost()

    def outputs(self):
        out = super().outputs()
        cal_vis, cal_weights, cal_flags = self.apply(
            out["avg_vis"], out["jones"], self.quad_antennas, self.quads, out["avg_weights"],
            out["avg_flags"])  # fmt: skip
        weights8, weights_channel = self.compress(cal_weights)
        out.update({"apply:out_vis": cal_vis, "cal_weights": cal_weights,
                    "apply:out_flags": cal_flags, "compress:weights8": weights8,
                    "compress:weights_channel": weights_channel})  # fmt: skip
        return out

    def residual(self, out):
        """(the largest |out_vis - I| over the unflagged samples between dishes, in units of
        CHAIN_NOISE; the fraction of those samples that is unflagged)."""
        assert not out["solve:status"].any()
        a, b = self.ants[:, 0], self.ants[:, 1]
        between = a // 2 != b // 2
        ideal = np.where(a % 2 == b % 2, 1.0, 0.0)[between]
        vis = out["apply:out_vis"][:, between].astype(np.complex128)
        kept = out["apply:out_flags"][:, between] == 0
        assert between.sum() == 24
        return float(np.abs(vis - ideal)[kept].max()) / CHAIN_NOISE, float(kept.mean())


def chain_host():
    """The measurement behind APPLY_CHAIN_MEASURED_FACTOR, on the host classes alone."""
    chain = ApplyChainHost()
    for d in range(3):
        chain.dump(20 + d)
    first = chain.residual(chain.outputs())
    chain.dump(40)
    second = chain.residual(chain.outputs())
    print(f"chain: residual over noise {first[0]:.3f} ({first[1]:.3f} unflagged) after three "
          f"dumps, {second[0]:.3f} ({second[1]:.3f}) after four")  # fmt: skip
    return first, second


def test_in_the_chain(context, command_queue):
    """Three dumps of 64 channels x 4 dual-feed antennas with all autocorrelations through
    prepare -> fused flagger -> accumulate -> finalise -> solve_jones(corrections=True) ->
    apply_jones -> compress in one sequence, against the host classes chained the same way, bit
    for bit; and ``out_vis`` between dishes is the identity coherency to within twice
    APPLY_CHAIN_MEASURED_FACTOR times the noise (the rounding of ACCURACY_BOUND is far below
    it, and is added), with at least 70 % of those samples unflagged."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import device, ingest

    queue = command_queue
    chain = ApplyChainHost()
    channels, cf, baselines, n_inputs = CHAIN["channels"], CHAIN["cf"], chain.baselines, chain.n_inputs
    full = device.BackgroundFlags.FULL
    prepare = ingest.PrepareTemplate(
        context, 1 / CHAIN["unit"], CHAIN["lost_flag"], False, True, CHAIN["weight_scale"]
    ).instantiate(queue, channels, baselines, chain.in_baselines)
    flagger = device.FlaggerDeviceTemplate(
        device.BackgroundMedianFilterDeviceTemplate(context, 13, use_flags=full),
        device.NoiseEstMADTDeviceTemplate(context, channels),
        device.ThresholdSumDeviceTemplate(context),
        fused=True, tuning={"vis_pad": 0},
    ).instantiate(queue, channels, baselines, threshold_args={"n_sigma": 11.0})
    accumulate = device.AccumulateTemplate(context, use_weights=True, input_flags=full).instantiate(
        queue, channels, baselines)  # fmt: skip
    finalise = device.FinaliseTemplate(context, channel_factor=cf).instantiate(
        queue, channels, baselines)  # fmt: skip
    solve = ingest.SolveJonesTemplate(
        context, max_iterations=CHAIN["max_iterations"], corrections=True
    ).instantiate(queue, channels // cf, baselines, n_inputs)
    apply_jones = ingest.ApplyJonesTemplate(context, flag_value=CHAIN_FLAG).instantiate(
        queue, channels // cf, baselines, n_inputs, len(chain.quads))  # fmt: skip
    compress = ingest.CompressWeightsTemplate(context).instantiate(queue, channels // cf, baselines)
    acc = ("acc_vis", "acc_weights", "acc_flags")
    compounds = {
        "vis": ["prepare:vis", "flagger:vis", "accumulate:vis"],
        "input_flags": ["prepare:input_flags", "flagger:input_flags", "accumulate:input_flags"],
        "weights": ["prepare:weights", "accumulate:weights"],
        "flags": ["flagger:flags", "accumulate:flags"],
        "avg_vis": ["finalise:vis", "solve:vis", "apply:vis"],
        "avg_weights": ["finalise:weights", "solve:weights", "apply:weights"],
        "avg_flags": ["finalise:flags", "solve:flags", "apply:flags"],
        "jones": ["solve:jones", "apply:jones"],
        "cal_weights": ["apply:out_weights", "compress:weights"],
    }
    compounds.update({name: ["accumulate:" + name, "finalise:" + name] for name in acc})
    seq = accel.OperationSequence(
        queue, [("prepare", prepare), ("flagger", flagger), ("accumulate", accumulate),
                ("finalise", finalise), ("solve", solve), ("apply", apply_jones),
                ("compress", compress)],
        compounds=compounds)  # fmt: skip
    for name in device.FusedFlaggerDevice._OPTIONAL:
        del seq.slots["flagger:" + name]
    seq.ensure_all_bound()
    assert finalise.buffer("vis") is solve.buffer("vis") is apply_jones.buffer("vis")
    assert solve.buffer("jones") is apply_jones.buffer("jones")
    assert apply_jones.buffer("out_weights") is compress.buffer("weights")
    for name in acc:
        seq.buffer(name).zero(queue)
    seq.buffer("prepare:source").set(queue, chain.source)
    seq.buffer("prepare:auto_source").set(queue, chain.auto_source)
    seq.buffer("solve:pairs").set(queue, chain.pairs)
    seq.buffer("apply:quad_antennas").set(queue, chain.quad_antennas)
    seq.buffer("apply:quads").set(queue, chain.quads)
    assert gen.covered(chain.quads, baselines).all()

    def check_outputs():
        out = chain.outputs()
        for name, w in out.items():
            assert_same(w, seq.buffer(name).get(queue), name)
        return out

    for d in range(3):
        seq.buffer("prepare:vis_in").set(queue, chain.dump(20 + d))
        prepare()
        flagger()
        accumulate()
    finalise()
    solve()
    apply_jones()
    compress()
    bound = 2 * APPLY_CHAIN_MEASURED_FACTOR + ACCURACY_BOUND / CHAIN_NOISE
    first = chain.residual(check_outputs())
    # and once more through the sequence as a whole
    seq.buffer("prepare:vis_in").set(queue, chain.dump(40))
    seq()
    second = chain.residual(check_outputs())
    print(f"chain: residual over noise {first[0]:.3f} ({first[1]:.3f} unflagged) after three "
          f"dumps, {second[0]:.3f} ({second[1]:.3f}) after four")  # fmt: skip
    assert first[0] <= bound and second[0] <= bound
    assert first[1] >= 0.7 and second[1] >= 0.7
