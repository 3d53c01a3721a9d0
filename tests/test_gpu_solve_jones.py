"""Solving Jones matrices on the GPU (``rfi.ingest.SolveJonesTemplate``, ``ksp_solve_jones``):
every comparison is of bit patterns, against ``rfi.host.SolveJonesHost``: ``jones`` (with
nothing left out but the payload of a NaN that the host has as a NaN too), ``iterations`` and
``status``."""

import ctypes
import functools
import itertools

import numpy as np
import pytest

from tests import inputs_solve_jones as gen
from tests.inputs_solve_jones import assert_same
from tests.subviews import CompactViews, poison_array, sentinel_array
from tests.test_gpu_prepare import LOST, N_AUTO
from tests.test_solve_jones import ACCURACY_BOUND, matrices

pytestmark = pytest.mark.gpu

# The sizes at which csrc/solve_jones.hip changes shape: a sum runs in blocks of 32 inputs, so
# 32, 64 and 96 are the last sizes with 1, 2 and 3 blocks; the workgroup has n * blocks threads
# rounded up to whole wavefronts (64 for up to 32 inputs, 512 for 128); 2 inputs have no
# baseline that counts, and 128 is the limit.
N_INPUTS = [2, 4, 6, 30, 32, 34, 62, 64, 66, 96, 126, 128]
CHANNELS = [1, 2, 7]
VARIANTS = list(itertools.product([True, False], repeat=3))  # weights, flags, initial
OUTPUTS = ("jones", "iterations", "status")
f32 = np.float32


@pytest.fixture(scope="module")
def context():
    from katsdpsigproc_amd import accel

    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


@functools.lru_cache(maxsize=None)
def cached_case(seed, channels, n_inputs, table, data, extra):
    case = gen.make_case(seed, channels, n_inputs, table, data, extra)
    for value in case.values():
        value.setflags(write=False)  # shared between tests: nobody changes it
    return case


def given_of(case, variant):
    weights, flags, initial = variant
    return {"vis": case["vis"], "pairs": case["pairs"],
            "weights": case["weights"] if weights else None,
            "flags": case["flags"] if flags else None,
            "initial": case["initial"] if initial else None}  # fmt: skip


def want_of(case, variant, settings):
    from katsdpsigproc_amd.rfi import host

    given = given_of(case, variant)
    return host.SolveJonesHost(*settings)(
        given["vis"], given["pairs"], given["weights"], given["flags"], given["initial"])


def hostile(padded_shape, dtype):
    """What the padding of an input holds: NaN, or bytes of 0xFF (a `pairs` entry of -1, which
    would name baseline 0, and a flag byte that is all set)."""
    return poison_array(int(np.prod(padded_shape)), dtype).reshape(padded_shape)


def run_device(context, queue, case, variant, settings, pad=0, in_place=False):
    """(jones, iterations, status) of the operation. The padding of the inputs holds NaN or
    0xFF; the outputs start out full of sentinel bytes. Afterwards every byte of padding is what
    it was, and so is every byte of the inputs."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import ingest

    weights, flags, initial = variant
    channels = case["vis"].shape[0]
    n_inputs = case["pairs"].shape[0]
    template = ingest.SolveJonesTemplate(context, weights, flags, initial, *settings)
    fn = template.instantiate(queue, channels, case["vis"].shape[1], n_inputs)
    given = {name: value for name, value in given_of(case, variant).items() if value is not None}
    if pad:
        for i, name in enumerate(list(given) + ["jones"]):
            dim = fn.slots[name].dimensions[1]
            accel.Dimension(dim.size, min_padded_size=dim.size + pad + i).link(dim)
        for i, name in enumerate(["iterations", "status", "pairs"]):  # and more rows
            dim = fn.slots[name].dimensions[0]
            accel.Dimension(dim.size, min_padded_size=dim.size + pad + i).link(dim)
    if in_place:
        fn.slots["initial"].dimensions[1].link(fn.slots["jones"].dimensions[1])
    fn.ensure_all_bound()
    if in_place:
        fn.bind(jones=fn.buffer("initial"))
    uploaded = {}
    for name, value in given.items():
        d = fn.buffer(name)
        assert d.padded_shape[1] >= value.shape[1] + pad
        raw = hostile(d.padded_shape, d.dtype)
        raw[: value.shape[0], : value.shape[1]] = value
        queue.enqueue_write_buffer(d.buffer, raw)
        uploaded[name] = raw
    for name in OUTPUTS:
        if not (in_place and name == "jones"):
            d = fn.buffer(name)
            queue.enqueue_write_buffer(d.buffer, sentinel_array(d.padded_shape, d.dtype))
    fn()
    out = []
    for name in OUTPUTS:
        d = fn.buffer(name)
        raw = np.empty(d.padded_shape, d.dtype)
        queue.enqueue_read_buffer(d.buffer, raw)
        data = (slice(channels), slice(n_inputs))[: min(raw.ndim, 2)]
        assert raw.ndim < 3 or raw.shape[2] == 2
        padding = np.ones(d.padded_shape, bool)
        padding[data] = False
        before = uploaded["initial"] if in_place and name == "jones" else sentinel_array(
            d.padded_shape, d.dtype)  # fmt: skip
        same = raw.view(np.uint8) == before.view(np.uint8)
        assert same[np.repeat(padding, d.dtype.itemsize, axis=-1)].all(), \
            f"wrote into the padding of {name}"  # fmt: skip
        out.append(np.ascontiguousarray(raw[data]))
    for name, before in uploaded.items():
        if in_place and name == "initial":
            continue
        d = fn.buffer(name)
        raw = np.empty(d.padded_shape, d.dtype)
        queue.enqueue_read_buffer(d.buffer, raw)
        assert (raw.view(np.uint8) == before.view(np.uint8)).all(), f"{name} was modified"
    return tuple(out)


def assert_outputs(want, got, what):
    assert_same(want[0], got[0], f"jones {what}")
    for name, w, g in zip(OUTPUTS[1:], want[1:], got[1:]):
        assert w.dtype == g.dtype and w.shape == g.shape, name
        assert (w == g).all(), f"{name} {what}: want {w}, got {g}"


def compare(context, queue, case, variant, settings, what, pad=0, in_place=False):
    want = want_of(case, variant, settings)
    got = run_device(context, queue, case, variant, settings, pad, in_place)
    assert_outputs(want, got, what)
    return want


DEFAULT = (30, 1e-5, 0, 0xFF, False)


@pytest.mark.parametrize("n_inputs", N_INPUTS)
def test_sizes(n_inputs, context, command_queue):
    """Every size with 1, 2 and 7 channels; the table, the data, the width of the array (the
    full triangle, or wider with the table naming a part) and the variant rotate."""
    for i, channels in enumerate(CHANNELS):
        k = N_INPUTS.index(n_inputs) + i
        table = gen.TABLES[k % len(gen.TABLES)]
        data = gen.DATA[k % len(gen.DATA)]
        extra = (0, 37)[k % 2]
        variant = VARIANTS[k % len(VARIANTS)]
        case = cached_case(100 + k, channels, n_inputs, table, data, extra)
        settings = (30, 1e-5, min(k % 3, n_inputs // 2 - 1), 0xFF, bool(k % 2))
        compare(context, command_queue, case, variant, settings,
                f"{channels} channels, {n_inputs} inputs, {table}, {data}, +{extra}, {variant}")  # fmt: skip


@pytest.mark.parametrize("data", gen.DATA)
@pytest.mark.parametrize("table", gen.TABLES)
def test_tables_and_data(table, data, context, command_queue):
    """Every table and data class of the inputs module, at a size of two blocks and one that
    fills a wavefront exactly."""
    for n_inputs, extra in ((34, 0), (8, 5)):
        case = cached_case(7, 3, n_inputs, table, data, extra)
        for variant in ((True, True, False), (True, True, True)):
            want = compare(context, command_queue, case, variant, DEFAULT, f"{table}, {data}")
            if data == "all_flagged":
                assert want[2][-1] & 2 and np.isnan(want[0][-1]).all()
            if data == "feed1_flagged" and not variant[2]:
                # from the identity det never rises above 0 in that channel
                assert want[2][-1] & 8 and np.isnan(want[0][-1, 1::2]).all()


def two_dead_case(data):
    """A table in which one antenna has no data at all and another has one dead feed; returns
    the case and the two antennas."""
    n_inputs = 34
    case = dict(cached_case(15, 2, n_inputs, "dead_antenna", data, 3))
    silent = gen.dead_antenna_of(15, n_inputs)
    half = (silent + 5) % (n_inputs // 2)
    pairs = case["pairs"].copy()
    for i in range(n_inputs):
        if i // 2 != half:
            pairs[min(i, 2 * half + 1), max(i, 2 * half + 1)] = 0
    case["pairs"] = pairs
    return case, silent, half


@pytest.mark.parametrize("weights, flags, initial", VARIANTS)
def test_variants(weights, flags, initial, context, command_queue):
    """weights / flags / initial on and off, with and without corrections, and every kind of
    reference: none, the first antenna, the last, one without data and one with a dead feed."""
    n_inputs = 34
    for data in ("clean", "hostile"):
        case, silent, half = two_dead_case(data)
        assert len({0, n_inputs // 2 - 1, silent, half}) == 4
        for corrections in (False, True):
            for reference in (-1, 0, n_inputs // 2 - 1, silent, half):
                settings = (30, 1e-5, reference, 0xFF, corrections)
                want = compare(context, command_queue, case, (weights, flags, initial), settings,
                               f"{data}, reference {reference}, corrections {corrections}")  # fmt: skip
                assert np.isnan(want[0][:, 2 * silent : 2 * silent + 2]).all()
                assert np.isnan(want[0][:, 2 * half + 1]).all()
                assert np.isnan(want[0][:, 2 * half]).all() == corrections
                if reference in (-1, silent, half):
                    assert (want[2] & 4).all()
                elif data == "clean":
                    assert not (want[2] & 4).any()
                    if not corrections:
                        for i in range(2):
                            assert (want[0][:, 2 * reference + i, i].imag == 0).all()


def staggered_case():
    """Seven clean channels whose starting matrices are the truth (channel 0) or further and
    further from it, so that the channels of one launch stop at different counts."""
    case = dict(cached_case(21, 7, 40, "missing", "clean", 0))
    rs = np.random.RandomState(3)
    shape = case["truth"].shape[:2]
    spread = np.exp2(rs.uniform(-1, 1, shape) * np.arange(7)[:, np.newaxis] / 6)
    case["initial"] = (case["truth"] * spread[:, :, np.newaxis]).astype(np.complex64)
    return case


@pytest.mark.parametrize("tol", [0.0, 1e-5, 1e-2])
@pytest.mark.parametrize("max_iterations", [1, 2, 3, 30])
def test_iterations_and_tol(max_iterations, tol, context, command_queue):
    case = staggered_case()
    settings = (max_iterations, tol, 0, 0xFF, False)
    want = compare(context, command_queue, case, (True, True, True), settings,
                   f"{max_iterations} iterations, tol {tol}")  # fmt: skip
    assert want[1].max() <= max_iterations
    if max_iterations == 1:
        assert (want[1] == 1).all() and (want[2] & 1).all()
    if max_iterations == 30 and tol == 1e-2:
        # channels of one launch stop at different counts
        assert want[1].tolist() == [2, 4, 4, 4, 6, 6, 6] and not want[2].any()


@pytest.mark.parametrize("n_inputs, channels, pad", [(4, 7, 5), (34, 2, 1), (64, 3, 16),
                                                     (128, 1, 3), (2, 5, 9)])  # fmt: skip
def test_padding(n_inputs, channels, pad, context, command_queue):
    """Rows padded beyond what the slots ask for, by another amount for every array (so the
    strides differ), and more rows of `pairs`, `iterations` and `status`; run_device checks
    every byte of padding and of the inputs."""
    case = cached_case(40 + pad, channels, n_inputs, "junk", "hostile", 4)
    for variant in ((True, True, True), (False, False, False), (True, False, True)):
        compare(context, command_queue, case, variant, DEFAULT, f"pad {pad}", pad=pad)
    compare(context, command_queue, case, (True, True, True), DEFAULT, f"pad {pad}, in place",
            pad=pad, in_place=True)  # fmt: skip


RAW_SHAPES = [(6, 6, 0), (3, 128, 3), (70, 2, 0), (3, 34, 11), (9, 64, 1)]  # channels, inputs, extra
RAW_OFFSETS = [1, 3, 16]


def raw_variant(offset, shape):
    """The variant of a shape at an offset: they rotate so that every offset has shapes with
    `initial` (read at that offset, and written there in place) and shapes without."""
    return VARIANTS[(RAW_SHAPES.index(shape) + 3 * RAW_OFFSETS.index(offset)) % len(VARIANTS)]


for _offset in RAW_OFFSETS:
    _with_initial = [raw_variant(_offset, shape)[2] for shape in RAW_SHAPES]
    assert sum(_with_initial) >= 2 and not all(_with_initial), (_offset, _with_initial)
assert {raw_variant(o, s) for o in RAW_OFFSETS for s in RAW_SHAPES} == set(VARIANTS)


@pytest.mark.parametrize("channels, n_inputs, extra", RAW_SHAPES)
@pytest.mark.parametrize("offset", RAW_OFFSETS)
def test_raw_abi_subviews(offset, channels, n_inputs, extra, context, command_queue):
    """Sub-views: pointers `offset` elements into their allocations and an odd stride of its own
    per array; the variants rotate (:func:`raw_variant`); with `initial`, jones apart from it
    and in place. A row of `initial` or `jones` is 2 n_inputs complex64 in a view whose stride is
    twice the odd count of 16-byte rows the launcher is given, `offset` complex64 in: 8 bytes
    off a multiple of 16 for the odd offsets."""
    from katsdpsigproc_amd import _lib
    from katsdpsigproc_amd.rfi import host

    queue = command_queue
    views = CompactViews(context, queue)
    seed = 31 * offset + n_inputs
    variant = raw_variant(offset, (channels, n_inputs, extra))
    case = cached_case(seed, channels, n_inputs, gen.TABLES[seed % len(gen.TABLES)], "hostile",
                       extra)  # fmt: skip
    given = given_of(case, variant)
    baselines = case["vis"].shape[1]
    fn = host.SolveJonesHost(30, 1e-5, n_inputs // 2 - 1, 0x7F, True)
    want = fn(given["vis"], given["pairs"], given["weights"], given["flags"], given["initial"])
    stride_of = {"vis": (baselines + 6) | 1, "weights": (baselines + 2) | 1,
                 "flags": (baselines + 4) | 1, "pairs": (n_inputs + 2) | 1,
                 "initial": (n_inputs + 4) | 1, "jones": (n_inputs + 8) | 1}  # fmt: skip

    def view(name, data, stride, poison):
        return views(name, data.dtype, data, stride, offset, poison=poison)

    def flat(rows):
        """(channels, n_inputs, 2) as the (channels, 2 n_inputs) the view helpers take."""
        return rows.reshape(rows.shape[0], -1)

    inputs = {name: view(name, value, stride_of[name], True)
              for name, value in given.items() if value is not None and name != "initial"}  # fmt: skip
    for in_place in (False, True) if given["initial"] is not None else (False,):
        d_initial = None
        if given["initial"] is not None:
            # in place the array is an output: sentinels around it instead of poison
            d_initial = view("jones" if in_place else "initial", flat(given["initial"]),
                             2 * stride_of["initial"], not in_place)  # fmt: skip
        if in_place:
            d_jones = d_initial
        else:
            blank = sentinel_array((channels, 2 * n_inputs), np.complex64)
            d_jones = view("jones", blank, 2 * stride_of["jones"], False)
        d_iterations = view("iterations", sentinel_array((1, channels), np.int32), channels, False)
        d_status = view("status", sentinel_array((1, channels), np.uint8), channels, False)

        def ptr(name):
            return inputs[name][1] if name in inputs else None

        def stride(name):
            return inputs[name][0].stride if name in inputs else 0

        _lib.call("ksp_solve_jones", context.device.index, ctypes.c_void_p(queue.stream),
                  ptr("vis"), ptr("weights"), ptr("flags"), ptr("pairs"),
                  d_initial[1] if d_initial is not None else None, d_jones[1], d_iterations[1],
                  d_status[1], channels, baselines, n_inputs, stride("vis"), stride("weights"),
                  stride("flags"), stride("pairs"),
                  d_initial[0].stride // 2 if d_initial is not None else 0,
                  d_jones[0].stride // 2, fn.max_iterations, float(fn.tol2), fn.reference,
                  fn.mask, 1)  # fmt: skip
        # (read asserts that nothing around the rows changed)
        got = (d_jones[0].read("jones").reshape(channels, n_inputs, 2),
               d_iterations[0].read("iterations")[0], d_status[0].read("status")[0])  # fmt: skip
        assert_outputs(want, got, f"at {offset}, in place {in_place}")
        if d_initial is not None and not in_place:
            d_initial[0].read("initial")  # (asserts that nothing wrote to it)
    for name, (d, _) in inputs.items():
        d.read(name)


def test_more_workgroups_than_compute_units(context, command_queue):
    case = cached_case(300, 600, 8, "reversed", "hostile", 2)
    compare(context, command_queue, case, (True, True, False), (30, 1e-3, 0, 0xFF, True),
            "600 channels")  # fmt: skip


def test_host_from_device(context, command_queue):
    from katsdpsigproc_amd.rfi import ingest

    case = cached_case(11, 5, 12, "reversed", "hostile", 4)
    inputs = gen.inputs_of(case["pairs"], case["vis"].shape[1])
    for variant in VARIANTS:
        template = ingest.SolveJonesTemplate(context, *variant, max_iterations=20, mask=0x0F)
        adapter = ingest.SolveJonesHostFromDevice(template, command_queue)
        given = given_of(case, variant)
        got = adapter(case["vis"], inputs, 12, given["weights"], given["flags"], given["initial"])
        assert_outputs(want_of(case, variant, (20, 1e-5, 0, 0x0F, False)), got, str(variant))


# ------------------------------------------------------------------------------ the chain
CHAIN_NOISE = 0.01  # per sample of a dump, against matrices of order 1
#: the largest |C_a V_ab C_b^H - I| over the kept samples between dishes, in units of
#: CHAIN_NOISE, measured on the host classes alone (the figures :func:`chain_host` prints:
#: 1.532 after three dumps, 2.118 after the fourth); the test asserts twice the larger
CHAIN_MEASURED_FACTOR = 2.12


def chain_layout():
    """Four dual-feed antennas: the 28 pairs of their 8 inputs, in a random order and
    direction (24 between dishes and the 4 cross-feed autocorrelations, which the solver must
    leave out), and 4 autocorrelations in their midst."""
    n_inputs = 8
    rs = np.random.RandomState(9)
    cross = np.array(np.triu_indices(n_inputs, 1)).T
    cross = cross[rs.permutation(len(cross))]
    swap = rs.random_sample(len(cross)) < 0.5
    cross[swap] = cross[swap][:, ::-1]
    autos = np.repeat(np.arange(4)[:, np.newaxis], 2, axis=1)
    ants = np.ascontiguousarray(np.concatenate([cross[:20], autos, cross[20:]]), np.int32)
    in_baselines = 60
    source = (N_AUTO + rs.permutation(in_baselines - N_AUTO)[: len(ants)]).astype(np.int32)
    auto_source = rs.randint(0, N_AUTO, (len(ants), 2)).astype(np.int32)
    truth = gen.make_jones(5, 1, n_inputs, span=1.0)[0].astype(np.complex128)
    return n_inputs, in_baselines, ants, source, auto_source, truth


def model_dump(seed, channels, in_baselines, source, ants, truth, unit):
    """int32 (channels, in_baselines, 2): ``z_p . conj(z_q)`` of an unpolarised unit source
    plus CHAIN_NOISE, in units of 1 / `unit`, at the input baselines `source` names (the
    cross-feed autocorrelations have their own signal too); autocorrelations of about 8 in
    the first N_AUTO; noise everywhere else; about 3 % lost samples."""
    rs = np.random.RandomState(seed)
    shape = (channels, in_baselines)
    noise = CHAIN_NOISE * (rs.standard_normal(shape) + 1j * rs.standard_normal(shape))
    vis = noise.copy()
    vis[:, source] += (truth[ants[:, 0]] * np.conj(truth[ants[:, 1]])).sum(axis=1)
    vis[:, :N_AUTO] = 8 + noise[:, :N_AUTO].real
    vis_in = np.empty(shape + (2,), np.int32)
    vis_in[..., 0] = np.rint(vis.real * unit)
    vis_in[..., 1] = np.rint(vis.imag * unit)
    lost = rs.random_sample(shape) < 0.03
    lost[:, :N_AUTO] = False
    vis_in[lost, 0] = LOST
    return vis_in


CHAIN = dict(channels=64, cf=4, unit=2.0**17, lost_flag=0x08, weight_scale=64.0,
             max_iterations=100)  # fmt: skip


class ChainHost:
    """PrepareHost + FlaggerHost + AveragerHost + SolveJonesHost(corrections=True) chained as
    the device sequence of test_in_the_chain is."""

    def __init__(self):
        from katsdpsigproc_amd.rfi import device, host

        (self.n_inputs, self.in_baselines, self.ants, self.source, self.auto_source,
         self.truth) = chain_layout()  # fmt: skip
        self.baselines = len(self.ants)
        self.pairs = host.SolveJonesHost.pair_table(self.ants, self.n_inputs)
        self.prepare = host.PrepareHost(1 / CHAIN["unit"], CHAIN["lost_flag"], CHAIN["weight_scale"])
        self.flagger = host.FlaggerHost(host.BackgroundMedianFilterHost(13), host.NoiseEstMADHost(),
                                        host.ThresholdSumHost(11.0))  # fmt: skip
        self.averager = host.AveragerHost(CHAIN["channels"], self.baselines, CHAIN["cf"],
                                          device.BackgroundFlags.FULL)  # fmt: skip
        self.solve = host.SolveJonesHost(CHAIN["max_iterations"], corrections=True)

    def dump(self, seed):
        vis_in = model_dump(seed, CHAIN["channels"], self.in_baselines, self.source, self.ants,
                            self.truth, CHAIN["unit"])  # fmt: skip
        vis, input_flags, weights = self.prepare(vis_in, self.source, None, self.auto_source)
        flags = self.flagger(vis, input_flags)
        self.averager.add(vis, flags, weights, input_flags=input_flags)
        return vis_in

    def outputs(self):
        vis, weights, flags = self.averager.finalise()
        jones, iterations, status = self.solve(vis, self.pairs, weights, flags)
        return {"avg_vis": vis, "avg_weights": weights, "avg_flags": flags, "jones": jones,
                "solve:iterations": iterations, "solve:status": status}  # fmt: skip

    def residual(self, out):
        """The largest |C_a V_ab C_b^H - I| over the baselines between dishes, all four
        products of a dish pair kept, in units of CHAIN_NOISE; formed in float64."""
        assert not out["solve:status"].any()
        c = matrices(out["jones"])  # (channels, antennas, 2, 2)
        vis, flags = out["avg_vis"].astype(np.complex128), out["avg_flags"]
        at = {(int(a), int(b)): j for j, (a, b) in enumerate(self.ants)}
        worst, seen = 0.0, 0
        for a in range(self.n_inputs // 2):
            for b in range(a + 1, self.n_inputs // 2):
                v = np.empty((vis.shape[0], 2, 2), np.complex128)
                kept = np.ones(vis.shape[0], bool)
                for i in range(2):
                    for k in range(2):
                        p, q = 2 * a + i, 2 * b + k
                        j = at.get((p, q))
                        v[:, i, k] = vis[:, j] if j is not None else np.conj(vis[:, at[(q, p)]])
                        kept &= flags[:, j if j is not None else at[(q, p)]] == 0
                calibrated = c[:, a] @ v @ np.conj(c[:, b].transpose(0, 2, 1))
                worst = max(worst, float(np.abs(calibrated[kept] - np.eye(2)).max()))
                seen += int(kept.sum())
        assert seen > 0.7 * 6 * vis.shape[0]
        return worst / CHAIN_NOISE


def chain_host():
    """The measurement behind CHAIN_MEASURED_FACTOR, on the host classes alone."""
    chain = ChainHost()
    for d in range(3):
        chain.dump(20 + d)
    first = chain.residual(chain.outputs())
    chain.dump(40)
    second = chain.residual(chain.outputs())
    print(f"chain: residual over noise {first:.3f} after three dumps, {second:.3f} after four")
    return first, second


def test_in_the_chain(context, command_queue):
    """Three dumps of 64 channels x 4 dual-feed antennas through prepare -> fused flagger ->
    accumulate -> finalise -> solve_jones(corrections=True) in one sequence, against the host
    classes chained the same way, bit for bit; and the calibrated products C_a V_ab C_b^H,
    formed here in NumPy, are the identity to within twice CHAIN_MEASURED_FACTOR times the
    noise (the rounding of ACCURACY_BOUND is far below it, and is added)."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import device, ingest

    queue = command_queue
    chain = ChainHost()
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
    acc = ("acc_vis", "acc_weights", "acc_flags")
    compounds = {
        "vis": ["prepare:vis", "flagger:vis", "accumulate:vis"],
        "input_flags": ["prepare:input_flags", "flagger:input_flags", "accumulate:input_flags"],
        "weights": ["prepare:weights", "accumulate:weights"],
        "flags": ["flagger:flags", "accumulate:flags"],
        "avg_vis": ["finalise:vis", "solve:vis"],
        "avg_weights": ["finalise:weights", "solve:weights"],
        "avg_flags": ["finalise:flags", "solve:flags"],
        "jones": ["solve:jones"],
    }
    compounds.update({name: ["accumulate:" + name, "finalise:" + name] for name in acc})
    seq = accel.OperationSequence(
        queue, [("prepare", prepare), ("flagger", flagger), ("accumulate", accumulate),
                ("finalise", finalise), ("solve", solve)],
        compounds=compounds)  # fmt: skip
    for name in device.FusedFlaggerDevice._OPTIONAL:
        del seq.slots["flagger:" + name]
    seq.ensure_all_bound()
    assert finalise.buffer("vis") is solve.buffer("vis")
    for name in acc:
        seq.buffer(name).zero(queue)
    seq.buffer("prepare:source").set(queue, chain.source)
    seq.buffer("prepare:auto_source").set(queue, chain.auto_source)
    seq.buffer("solve:pairs").set(queue, chain.pairs)

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
    bound = 2 * CHAIN_MEASURED_FACTOR + ACCURACY_BOUND / CHAIN_NOISE
    first = chain.residual(check_outputs())
    # and once more through the sequence as a whole
    seq.buffer("prepare:vis_in").set(queue, chain.dump(40))
    seq()
    second = chain.residual(check_outputs())
    print(f"chain: residual over noise {first:.3f} after three dumps, {second:.3f} after four")
    assert first <= bound and second <= bound
