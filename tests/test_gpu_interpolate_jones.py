"""Filling solved Jones matrices across flagged channels on the GPU
(``rfi.ingest.InterpolateJonesTemplate``, ``ksp_interpolate_jones``) and the diagonal of a table
(``rfi.ingest.JonesDiagonalTemplate``, ``ksp_jones_diagonal``): every comparison is of bit
patterns, of all outputs, against ``rfi.host.InterpolateJonesHost`` and
``rfi.host.JonesDiagonalHost``, with nothing left out but the payload of a NaN that the host
has as a NaN too."""

import ctypes
import functools
import itertools

import numpy as np
import pytest

from tests import inputs_interpolate_jones as gen
from tests.inputs_interpolate_jones import assert_same
from tests.subviews import CompactViews, poison_array, sentinel_array

pytestmark = pytest.mark.gpu

# The sizes at which csrc/interpolate_jones.hip changes path. The workgroup has as many threads
# as the next power of two at or above the channels, at least 64 (one wavefront: 1, 2, 3 and up
# to 64 channels) and at most 1024, so the thread count steps behind 64, 128, 256 and 512
# channels, and with it the number of wavefronts whose ballots make the words of kept bits (one
# wavefront scans them up to 4096 channels, two to four above) and the levels of the amplitude's
# tree that cross wavefronts. From 1025 channels on a thread owns ceil(channels / 1024) channels
# and the tree's thread-local levels are those of the next power of two (2, 4, 8, 16 terms).
# The four elements go through one LDS column at every size, so the size at which four columns
# would stop fitting (4096) is no step of this kernel; it is in the list as the step of the
# scan. Each group below is one step: one channel below it, at it and one above.
STEPS = [[1, 2, 3]] + [[n - 1, n, n + 1] for n in (64, 128, 256, 512, 1024, 2048, 3072, 4096,
                                                   5120, 8192, 12288)] + [[16383, 16384]]  # fmt: skip
N_ANT = [1, 2, 3, 64, 65]
SMOOTHS = [1, 3, 31]
#: status, model, scale, normalise, corrections
VARIANTS = list(itertools.product([True, False], repeat=5))
FULL = (True, True, True, True, True)
OUTPUTS = ("out", "kept", "filled", "fill_status", "mean_amplitude")
DTYPES = {"out": np.complex64, "kept": np.int32, "filled": np.int32, "fill_status": np.uint8,
          "mean_amplitude": np.float32}  # fmt: skip
MASK = 0x0F


@pytest.fixture(scope="module")
def context():
    from katsdpsigproc_amd import accel

    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


@functools.lru_cache(maxsize=None)
def cached_case(seed, channels, n_ant, max_gap, first=0):
    """{jones, status, model, scale}: never modified."""
    jones, status, model, scale, _ = gen.make_case(seed, channels, n_ant, max_gap, first, MASK)
    case = {"jones": jones, "status": status, "model": model, "scale": scale}
    for array in case.values():
        array.flags.writeable = False
    return case


def inputs_of(case, variant):
    """The arguments of the host class after jones, None for what `variant` leaves out."""
    return [case[name] if wanted else None
            for name, wanted in zip(("status", "model", "scale"), variant)]  # fmt: skip


def outputs_of(variant):
    return [name for name in OUTPUTS if name != "mean_amplitude" or variant[3]]


@functools.lru_cache(maxsize=None)
def cached_want(key, smooth, variant):
    """What the host gives for cached_case(*key), by name. Never modified."""
    from katsdpsigproc_amd.rfi import host

    case = cached_case(*key)
    fn = host.InterpolateJonesHost(key[3], smooth, variant[3], MASK, variant[4])
    want = dict(zip(OUTPUTS, fn(case["jones"], *inputs_of(case, variant))))
    for array in want.values():
        if array is not None:
            array.flags.writeable = False
    return want


def hostile(padded_shape, dtype):
    """What the padding of an input holds: NaN, or bytes of 0xFF."""
    return poison_array(int(np.prod(padded_shape)), dtype).reshape(padded_shape)


def padded_dimension(slot):
    """The dimension of `slot` that rows are padded in: the inputs of a table (its last axis
    is exact), else the only or last one."""
    return slot.dimensions[1] if len(slot.dimensions) == 3 else slot.dimensions[-1]


def run_device(context, queue, case, max_gap, smooth, variant, pad=0, in_place=False):
    """The outputs of the operation by name. The padding of the inputs holds NaN or 0xFF; the
    outputs start out full of sentinel bytes (in place, `out` starts as jones in hostile
    padding). Afterwards every byte of padding is what it was, and so is every byte of the
    inputs that are not also the output."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import ingest

    with_status, with_model, with_scale, normalise, corrections = variant
    channels, n_inputs = case["jones"].shape[:2]
    template = ingest.InterpolateJonesTemplate(context, max_gap, smooth, normalise, with_status,
                                               MASK, with_model, with_scale, corrections)  # fmt: skip
    fn = template.instantiate(queue, channels, n_inputs)
    if pad:
        for k, (name, slot) in enumerate(fn.slots.items()):
            if in_place and name == "out":
                k = 0  # (the padding of jones)
            dim = padded_dimension(slot)
            accel.Dimension(dim.size, min_padded_size=dim.size + (k + 1) * pad).link(dim)
    if in_place:
        fn.ensure_bound("jones")
        fn.bind(out=fn.buffer("jones"))
    fn.ensure_all_bound()
    uploaded = {}
    for name, wanted in zip(("jones", "status", "model", "scale"), (True,) + tuple(variant[:3])):
        if not wanted:
            continue
        d = fn.buffer(name)
        raw = hostile(d.padded_shape, d.dtype)
        raw[tuple(slice(n) for n in case[name].shape)] = case[name]
        queue.enqueue_write_buffer(d.buffer, raw)
        uploaded[name] = raw
    outputs = outputs_of(variant)
    before = {}
    for name in outputs:
        d = fn.buffer(name)
        before[name] = sentinel_array(d.padded_shape, d.dtype)
        if in_place and name == "out":
            before[name] = uploaded.pop("jones")
        else:
            queue.enqueue_write_buffer(d.buffer, before[name])
    fn()
    out = {}
    for name in outputs:
        d = fn.buffer(name)
        raw = np.empty(d.padded_shape, d.dtype)
        queue.enqueue_read_buffer(d.buffer, raw)
        data = tuple(slice(n) for n in d.shape)
        padding = np.ones(d.padded_shape, bool)
        padding[data] = False
        same = raw.view(np.uint8) == before[name].view(np.uint8)
        assert same[np.repeat(padding, d.dtype.itemsize, axis=-1)].all(), \
            f"wrote into the padding of {name}"  # fmt: skip
        out[name] = np.ascontiguousarray(raw[data])
    for name, sent in uploaded.items():
        d = fn.buffer(name)
        raw = np.empty(d.padded_shape, d.dtype)
        queue.enqueue_read_buffer(d.buffer, raw)
        assert (raw.view(np.uint8) == sent.view(np.uint8)).all(), f"{name} was modified"
    return out


def compare(context, queue, key, smooth=1, variant=FULL, pad=0, in_place=False):
    case = cached_case(*key)
    want = cached_want(key, smooth, variant)
    got = run_device(context, queue, case, key[3], smooth, variant, pad, in_place)
    assert list(got) == outputs_of(variant)
    for name, g in got.items():
        assert_same(want[name], g, f"{name} of {key}, smooth {smooth}, {variant}")
    return want


@pytest.mark.parametrize("step", STEPS, ids=lambda step: str(step[-2]))
def test_every_step_of_the_geometry(step, context, command_queue):
    """One channel below, at and one above every size at which the kernel changes path; the
    number of antennas, the kinds they start with, max_gap, smooth and the variant rotate."""
    for i, channels in enumerate(step):
        turn = i + len(step) * STEPS.index(step)
        n_ant = (5, 8, 3)[i % 3] if channels <= 1025 else (3, 2, 4)[i % 3]
        key = (turn, channels, n_ant, (8, 1, 70, 3)[turn % 4], 5 * turn)
        compare(context, command_queue, key, SMOOTHS[turn % 3], VARIANTS[(7 * turn) % 32])
        compare(context, command_queue, key, SMOOTHS[(turn + 1) % 3])


@pytest.mark.parametrize("n_ant", N_ANT)
def test_antennas(n_ant, context, command_queue):
    """One workgroup, odd strides, and several of every kind of data at 64 and 65 antennas."""
    seen = set()
    for channels, max_gap in ((37, 2), (300, 8), (1500, 5)):
        want = compare(context, command_queue, (n_ant, channels, n_ant, max_gap, n_ant), 3)
        seen |= set(want["fill_status"].tolist())
    if n_ant >= 64:
        assert seen == {0, 1, 2}


def test_most_inputs(context, command_queue):
    """n_inputs 2048: 1024 workgroups, four per compute unit."""
    compare(context, command_queue, (7, 8, 1024, 2, 0), 3)


@pytest.mark.parametrize("first", range(0, len(gen.KINDS), 4))
def test_kinds(first, context, command_queue):
    """Four kinds of data at a time, each on its own among the antennas of a launch, at lengths
    on either side of every path of the kernel; the gaps of max_gap and max_gap + 1 channels lie
    across the wavefront's end at 64, the workgroup's at its thread count, and 4096."""
    for channels, max_gap in ((2, 1), (3, 0), (64, 3), (129, 8), (2048, 16), (5000, 100)):
        key = (first, channels, 4, max_gap, first)
        compare(context, command_queue, key)
        compare(context, command_queue, key, 3, (False, True, False, True, False))
        compare(context, command_queue, key, 1, (False, False, False, False, False))


@pytest.mark.parametrize("smooth", SMOOTHS)
def test_smooth(smooth, context, command_queue):
    """Windows that run over both ends of the band (5 and 20 channels at 31), windows whose
    only kept channel is their centre (`alternating` and `one_kept` at 3), and windows that
    reach into the next wavefront and the next round of the workgroup."""
    for channels in (5, 20, 100, 1030, 3000):
        key = (smooth, channels, len(gen.KINDS), 6, 0)
        compare(context, command_queue, key, smooth)
        compare(context, command_queue, key, smooth, (True, False, False, True, True))


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "".join("ft"[x] for x in v))
def test_variants(variant, context, command_queue):
    """Every option, with the running mean (the pass that leaves s in `out`) and without it
    (where only the normalisation asks for that pass)."""
    compare(context, command_queue, (11, 150, 19, 4, 3), 3, variant)
    compare(context, command_queue, (11, 150, 19, 4, 3), 1, variant)


@pytest.mark.parametrize("channels, n_ant, pad", [(5, 3, 5), (130, 9, 1), (1100, 17, 16),
                                                   (4100, 3, 35)])  # fmt: skip
def test_in_place_and_padding(channels, n_ant, pad, context, command_queue):
    """`out` bound to the buffer of `jones`, and rows padded beyond what the slots ask for, by
    a different amount for every slot (so the strides differ); run_device checks every byte of
    padding and of the inputs."""
    key = (pad, channels, n_ant, 7, pad)
    for variant in VARIANTS[::5]:
        compare(context, command_queue, key, 3, variant, in_place=True)
        compare(context, command_queue, key, 3, variant, pad=pad)
        compare(context, command_queue, key, 1, variant, pad=pad, in_place=True)


@pytest.mark.parametrize("channels, n_ant", [(6, 3), (3, 64), (70, 1), (300, 17), (1100, 2)])
@pytest.mark.parametrize("offset", [1, 3, 16])
def test_raw_abi_subviews(offset, channels, n_ant, context, command_queue):
    """Sub-views: pointers `offset` complex64 into their allocations (so the tables are
    aligned to 8 bytes, not 16) and an odd stride of its own for jones, model and out, with
    sentinels around every row; the variants rotate."""
    from katsdpsigproc_amd import _lib

    queue = command_queue
    views = CompactViews(context, queue)
    n_inputs = 2 * n_ant
    seed = 31 * offset + n_ant
    variant = VARIANTS[seed % 32]
    with_status, with_model, with_scale, normalise, corrections = variant
    key = (seed, channels, n_ant, 5, seed)
    case = cached_case(*key)
    want = cached_want(key, 3, variant)

    def view(name, data, stride, poison):
        return views(name, data.dtype, data, stride, offset, poison=poison)

    def blank(name, shape, stride):
        return view(name, sentinel_array(shape, DTYPES[name]), stride, False)

    # a table as rows of 2 n_inputs complex64, its stride an odd number of rows of two
    jones_stride, out_stride = (n_inputs + 4) | 1, (n_inputs + 8) | 1
    d_in = {"jones": view("jones", case["jones"].reshape(channels, 2 * n_inputs),
                          2 * jones_stride, True)}  # fmt: skip
    if with_status:
        d_in["status"] = view("status", case["status"][np.newaxis, :], channels, True)
    if with_model:
        d_in["model"] = view("model", case["model"], (n_inputs + 12) | 1, True)
    if with_scale:
        d_in["scale"] = view("scale", case["scale"][np.newaxis, :], n_inputs, True)
    d_out = {name: blank(name, (1, n_ant), n_ant) for name in outputs_of(variant)[1:]}
    d_out["out"] = blank("out", (channels, 2 * n_inputs), 2 * out_stride)

    def pointer(views_by_name, name):
        return views_by_name[name][1] if name in views_by_name else None

    _lib.call("ksp_interpolate_jones", context.device.index, ctypes.c_void_p(queue.stream),
              pointer(d_in, "jones"), pointer(d_in, "status"), pointer(d_in, "model"),
              pointer(d_in, "scale"), pointer(d_out, "out"), pointer(d_out, "kept"),
              pointer(d_out, "filled"), pointer(d_out, "fill_status"),
              pointer(d_out, "mean_amplitude"), channels, n_inputs, jones_stride,
              d_in["model"][0].stride if with_model else 0, out_stride, 5, 3, MASK,
              int(corrections))  # fmt: skip
    for name, (d, _) in d_out.items():
        got = d.read(name)  # (asserts that nothing around the rows changed)
        got = got.reshape(channels, n_inputs, 2) if name == "out" else got[0]
        assert_same(want[name], got, f"{name} at {offset}")
    for name, (d, _) in d_in.items():
        d.read(name)  # (asserts that nothing wrote to it)


def test_largest(context, command_queue):
    """The longest band with the widest window, and the shape of the time measurement."""
    compare(context, command_queue, (3, 16384, 3, 16384, 0), 31)
    compare(context, command_queue, (4, 4096, 64, 8, 0), 9, (True, True, False, True, True))


def test_host_from_device(context, command_queue):
    from katsdpsigproc_amd.rfi import ingest

    key = (21, 90, 9, 4, 0)
    case = cached_case(*key)
    for variant in VARIANTS[::3]:
        with_status, with_model, with_scale, normalise, corrections = variant
        template = ingest.InterpolateJonesTemplate(context, 4, 3, normalise, with_status, MASK,
                                                   with_model, with_scale, corrections)  # fmt: skip
        adapter = ingest.InterpolateJonesHostFromDevice(template, command_queue)
        got = adapter(case["jones"], *inputs_of(case, variant))
        want = cached_want(key, 3, variant)
        assert len(got) == 5 and (got[4] is not None) == normalise
        for name, g in zip(OUTPUTS, got):
            if g is not None:
                assert_same(want[name], g, f"{name} of {variant}")


# ---------------------------------------------------------------------------- the diagonal
@pytest.mark.parametrize("channels, n_inputs", [(1, 2), (7, 6), (300, 130)])
def test_jones_diagonal(channels, n_inputs, context, command_queue):
    """The adapter, rows padded by different amounts with sentinels in the padding of `gains`,
    and the C-ABI on sub-views at odd strides, 3 complex64 into their allocations."""
    from katsdpsigproc_amd import _lib, accel
    from katsdpsigproc_amd.rfi import host, ingest

    queue = command_queue
    jones = cached_case(channels, channels, n_inputs // 2, 3)["jones"]
    want = host.JonesDiagonalHost()(jones)
    template = ingest.JonesDiagonalTemplate(context)
    assert_same(want, ingest.JonesDiagonalHostFromDevice(template, queue)(jones), "adapter")
    fn = template.instantiate(queue, channels, n_inputs)
    accel.Dimension(n_inputs, min_padded_size=n_inputs + 3).link(fn.slots["jones"].dimensions[1])
    accel.Dimension(n_inputs, min_padded_size=n_inputs + 9).link(fn.slots["gains"].dimensions[1])
    fn.ensure_all_bound()
    d_jones, d_gains = fn.buffer("jones"), fn.buffer("gains")
    raw = hostile(d_jones.padded_shape, np.complex64)
    raw[:, :n_inputs] = jones
    queue.enqueue_write_buffer(d_jones.buffer, raw)
    before = sentinel_array(d_gains.padded_shape, np.complex64)
    queue.enqueue_write_buffer(d_gains.buffer, before)
    fn()
    got = np.empty(d_gains.padded_shape, np.complex64)
    queue.enqueue_read_buffer(d_gains.buffer, got)
    assert_same(want, np.ascontiguousarray(got[:, :n_inputs]), "padded")
    assert (got[:, n_inputs:].view(np.uint8) == before[:, n_inputs:].view(np.uint8)).all()
    views = CompactViews(context, queue)
    v_jones, p_jones = views("jones", np.complex64, jones.reshape(channels, 2 * n_inputs),
                             2 * ((n_inputs + 4) | 1), 3, poison=True)  # fmt: skip
    v_gains, p_gains = views("gains", np.complex64, sentinel_array((channels, n_inputs), np.complex64),
                             (n_inputs + 6) | 1, 3, poison=False)  # fmt: skip
    _lib.call("ksp_jones_diagonal", context.device.index, ctypes.c_void_p(queue.stream), p_jones,
              p_gains, channels, n_inputs, (n_inputs + 4) | 1, v_gains.stride)  # fmt: skip
    assert_same(want, v_gains.read("gains"), "sub-view")
    v_jones.read("jones")


# ------------------------------------------------------------------------------- the chain
def test_in_the_chain(context, command_queue):
    """The scan of tests/inputs_interpolate_jones.py (256 channels x 4 dual-feed antennas, 36
    baselines, 40 calibrator channels flagged in runs of at most 8) through solve_jones ->
    jones_diagonal -> fit_delays -> interpolate_jones(corrections=True) -> apply_jones in one
    sequence, bit for bit against the host classes chained the same way. No target sample is
    flagged and the target is the identity coherency to within twice CHAIN_MEASURED; with the
    solver's own corrections applied directly, every sample of the 40 channels is flagged."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import ingest

    queue = command_queue
    scan = gen.chain_scan()
    want = gen.chain_host(scan)
    channels, n_inputs, baselines = gen.CHAIN["channels"], gen.CHAIN["n_inputs"], scan["baselines"]
    flagged, flag_value = scan["flagged"], gen.CHAIN["flag_value"]
    iterations = gen.CHAIN["max_iterations"]

    def apply_of():
        return ingest.ApplyJonesTemplate(context, flag_value=flag_value).instantiate(
            queue, channels, baselines, n_inputs, len(scan["quads"]))  # fmt: skip

    solve = ingest.SolveJonesTemplate(context, max_iterations=iterations).instantiate(
        queue, channels, baselines, n_inputs)  # fmt: skip
    diagonal = ingest.JonesDiagonalTemplate(context).instantiate(queue, channels, n_inputs)
    fit = ingest.FitDelaysTemplate(context, gen.CHAIN["width"]).instantiate(queue, channels, n_inputs)
    interp = ingest.InterpolateJonesTemplate(
        context, gen.CHAIN["max_gap"], corrections=True).instantiate(queue, channels, n_inputs)  # fmt: skip
    apply_jones = apply_of()
    seq = accel.OperationSequence(
        queue, [("solve", solve), ("diagonal", diagonal), ("fit", fit), ("interp", interp),
                ("apply", apply_jones)],
        compounds={"jones": ["solve:jones", "diagonal:jones", "interp:jones"],
                   "status": ["solve:status", "fit:status", "interp:status"],
                   "gains": ["diagonal:gains", "fit:gains"],
                   "k": ["fit:model", "interp:model"],
                   "corr": ["interp:out", "apply:jones"]})  # fmt: skip
    seq.ensure_all_bound()
    assert solve.buffer("jones") is diagonal.buffer("jones") is interp.buffer("jones")
    assert diagonal.buffer("gains") is fit.buffer("gains")
    assert fit.buffer("model") is interp.buffer("model")
    assert interp.buffer("out") is apply_jones.buffer("jones")
    uploads = (("solve:vis", "cal_vis"), ("solve:weights", "weights"), ("solve:flags", "cal_flags"),
               ("solve:pairs", "pairs"), ("apply:vis", "target_vis"), ("apply:weights", "weights"),
               ("apply:flags", "target_flags"), ("apply:quad_antennas", "quad_antennas"),
               ("apply:quads", "quads"))  # fmt: skip
    for name, source in uploads:
        seq.buffer(name).set(queue, scan[source])
    seq()
    for name, w in want.items():
        assert_same(w, seq.buffer(name).get(queue), name)
    # every gap was filled, no sample is flagged, and the target is the sky in every channel
    assert not want["fit:fit_status"].any() and not want["interp:fill_status"].any()
    assert (want["interp:kept"] == channels - 40).all() and (want["interp:filled"] == 40).all()
    assert not seq.buffer("apply:out_flags").get(queue).any()
    distance = gen.chain_distance(scan, seq.buffer("apply:out_vis").get(queue))
    print(f"chain: calibrated target within {distance:.5f} of the identity coherency")
    assert distance <= 2 * gen.CHAIN_MEASURED

    # without the new steps: the solver's own corrections, applied directly
    solve_direct = ingest.SolveJonesTemplate(
        context, max_iterations=iterations, corrections=True).instantiate(
        queue, channels, baselines, n_inputs)  # fmt: skip
    direct = accel.OperationSequence(
        queue, [("solve", solve_direct), ("apply", apply_of())],
        compounds={"corr": ["solve:jones", "apply:jones"]})
    direct.ensure_all_bound()
    for name, source in uploads:
        direct.buffer(name).set(queue, scan[source])
    direct()
    lost = direct.buffer("apply:out_flags").get(queue)
    assert (lost[flagged] == flag_value).all() and not lost[~flagged].any()
