"""What a workgroup of the persistent ring kernel carries from strip to strip -- the MAD hint,
the amplitudes and the NaN watch of the next strip's first chunk, the tickets, the way back from
the sorted-window fallback -- on data in which neighbouring baselines differ
(tests/inputs_ring_strips.py), at strip counts around those where the ticket lists behave
differently, and with one workspace shared by ring and 4-baseline launches in turn.

Flags and noise of two launches are compared with the CPU oracle for exact equality. Every test
first asserts, on the CPU, that the input it is about to use holds the classes it is there for
(as tests/test_ring_strips.py does at the shape of a 256-CU device): an input that stops
reaching its case fails instead of passing for nothing.

Width 13, 11 sigma, 4 windows, 4096 channels, ``8 * (2 * n_cu + 1)`` baselines per family."""

import collections
import ctypes

import numpy as np
import pytest

from tests import inputs
from tests import inputs_ring_strips as rs_in

pytestmark = pytest.mark.gpu

CHANNELS = rs_in.CHANNELS
STRIP = rs_in.STRIP
N_SIGMA = 11.0

Case = collections.namedtuple("Case", "family flags noise noise64 dev bins lower_below")


@pytest.fixture(scope="module")
def context():
    from katsdpsigproc_amd import accel

    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


@pytest.fixture(scope="module")
def n_cu(context):
    return rs_in.compute_units(context)


@pytest.fixture(scope="module")
def oracle():
    from oracle import rfi_oracle

    rfi_oracle.set_threads(rfi_oracle.max_threads())
    yield rfi_oracle
    rfi_oracle.set_threads(1)


@pytest.fixture(scope="module")
def cases(oracle, n_cu):
    """family name -> Case: the input, the oracle's flags and noise (float32), its float64
    deviations where a test derives other thresholds from them, and the classification. The
    oracle runs once per input; everything is shared, read-only, by the tests that follow."""
    made = {}

    def get(name):
        if name not in made:
            family = rs_in.FAMILIES[name](rs_in.baselines_for(n_cu))
            with np.errstate(all="ignore"):
                flags, noise, dev = oracle.flagger_full(
                    family.vis, width=rs_in.WIDTH, n_sigma=N_SIGMA, n_windows=4, want_deviations=True)
            bins = rs_in.mad_bin(dev, hint=rs_in.EDGE_TOP)._replace(keys=None)
            noise32 = noise.astype(np.float32)
            for array in (family.vis, flags, noise32, noise, dev):
                array.setflags(write=False)
            keep = name in ("edges", "mixed")
            lower_below = None
            if name == "mixed":
                lower_below = np.zeros(family.vis.shape[1], bool)
                small = np.flatnonzero(family.kind == family.kinds.index("2^-140"))
                lower_below[small] = rs_in.narrowed_lower_below(dev[:, small], 256)  # (LIST_CAP of both kernels)
            made[name] = Case(family, flags, noise32, noise, dev if keep else None, bins, lower_below)
        return made[name]

    return get


# ------------------------------------------------------------------- what an input must hold
def largest_share(top):
    """The largest share of one top among the baselines of one position ``b % 8``."""
    return max(np.unique(top[w::STRIP], return_counts=True)[1].max() / len(top[w::STRIP])
               for w in range(STRIP))  # fmt: skip


def check_binades(case, baselines=None):
    """No top on more than 5 % of the baselines of a position (tests/test_ring_strips.py saw 2.4 %
    at 4104 baselines); of a few leading baselines, whose exponents are drawn from 121 values, at
    least a third as many distinct tops as there are baselines or exponents."""
    top = case.bins.top[:baselines]
    assert (top >= 0).all()
    if baselines is None:
        found = largest_share(top)
        print(f"binades: largest share of one top at a position {found:.3f}")
        assert found <= 0.05
    else:
        distinct = len(np.unique(top))
        print(f"binades, {baselines} baselines: {distinct} distinct tops")
        assert 3 * distinct >= min(baselines, 121)


def check_neighbours(case):
    A = rs_in.NEIGHBOUR_TOP
    for w in range(STRIP):
        share = np.array([(case.bins.top[w::STRIP] == A + s).mean() for s in (-1, 0, 1)])
        assert share.sum() == 1.0 and share.min() >= 0.20, (w, share)
    print("neighbours: tops", {A + s: int((case.bins.top == A + s).sum()) for s in (-1, 0, 1)})


def check_edges(case):
    family, bins = case.family, case.bins
    counts = rs_in.position_counts(family.kind, len(family.kinds))
    print("edges: fewest baselines at a position:", dict(zip(family.kinds, counts.min(axis=0).tolist())))
    assert (counts[:, :3] >= 0.15 * (len(family.kind) // STRIP)).all() and (counts[:, 3:] >= 8).all()
    low, high = bins.rank - bins.lb, bins.rank - (bins.lb + bins.cnt)
    for k in range(3, len(family.kinds)):
        want_low, want_high = rs_in.EDGE_RIMS[family.kinds[k].rsplit("_", 1)[0]]
        mine = family.kind == k
        assert want_low is None or (low[mine] == want_low).all(), family.kinds[k]
        assert want_high is None or (high[mine] == want_high).all(), family.kinds[k]
    filler = family.kind < 3
    np.testing.assert_array_equal(bins.top[filler], rs_in.EDGE_TOP - 1 + family.kind[filler])
    assert case.flags[:, ~filler].any()


def check_mixed(case, baselines=None):
    """Every kind is there (at least 4 times at every position of the whole family), the two early
    returns of the search are taken by the kinds meant to take them and the sorted-window
    fallback has its non-finite amplitudes."""
    family, bins = case.family, case.bins
    kind = family.kind[:baselines]
    name = np.array(family.kinds)[kind]
    if baselines is None:
        counts = rs_in.position_counts(kind, len(family.kinds))
        print("mixed: fewest baselines at a position:", dict(zip(family.kinds, counts.min(axis=0).tolist())))
        assert (counts >= 4).all()
        # subnormal deviations share key 1: the bin is narrowed to one float32 value, and where
        # the lower median lies below that value it still lies inside the key's bin
        print("mixed: baselines with the lower median below the narrowed bin:", int(case.lower_below.sum()))
        assert case.lower_below.sum() >= 8
    assert set(kind.tolist()) == set(range(len(family.kinds)))
    nan_noise = np.isnan(case.noise[:baselines])
    np.testing.assert_array_equal(nan_noise, (name == "zero") | (name == "constant"))
    np.testing.assert_array_equal(~bins.searched[:baselines] & ~nan_noise, name == "tiny")
    with np.errstate(all="ignore"):
        finite = np.isfinite(np.abs(family.vis[:, :baselines])).all(axis=0)
    np.testing.assert_array_equal(~finite, np.isin(name, ["nan", "inf", "overflow"]))


CHECKS = {"binades": check_binades, "neighbours": check_neighbours, "edges": check_edges,
          "mixed": check_mixed}  # fmt: skip


# --------------------------------------------------------------------------------- the runs
def run_ring(context, queue, vis, ref_flags, ref_noise, threshold="sum", flag_value=1, vis_pad=0,
             flags_pad=0, ring=1):
    """The flagger without the deviations output, ring kernel forced (`ring` -1: the 4-baseline
    kernel instead); twice, because the second launch finds the scheduling counters as the
    first left them. After either launch the workspace reads all zero, and flags and noise
    equal the oracle's."""
    from katsdpsigproc_amd import _lib, accel
    from katsdpsigproc_amd.rfi import device

    if threshold == "sum":
        th = device.ThresholdSumDeviceTemplate(context, 4, flag_value=flag_value)
    else:
        th = device.ThresholdSimpleDeviceTemplate(context, False, flag_value=flag_value)
    template = device.FlaggerDeviceTemplate(
        device.BackgroundMedianFilterDeviceTemplate(context, rs_in.WIDTH),
        device.NoiseEstMADTDeviceTemplate(context, 10240), th,
        keep_deviations=False, tuning={"vis_pad": vis_pad})  # fmt: skip
    fn = template.instantiate(queue, *vis.shape, threshold_args={"n_sigma": N_SIGMA})
    assert isinstance(fn, device.FusedFlaggerDevice)
    if flags_pad:
        # (a padded row: the zero fill ahead of the kernel goes row by row, fused_zero_rows_kernel)
        dim = fn.slots["flags"].dimensions[-1]
        dim.link(accel.Dimension(dim.size, min_padded_size=dim.size + flags_pad))
    fn.ensure_all_bound()
    baselines = vis.shape[1]
    assert fn.buffer("vis").padded_shape[1] >= baselines + vis_pad
    assert fn.buffer("flags").padded_shape[1] >= baselines + flags_pad
    fn.buffer("vis").set(queue, vis)
    prefill = fn.buffer("flags").empty_like()
    accel.HostArray.padded_view(prefill)[...] = 255
    for launch in range(2):
        fn.buffer("flags").set(queue, prefill)
        with _lib.fused_ring_mode(ring):
            fn()
        path = _lib.call("ksp_flagger_fused_last_path")
        if ring == 1:
            assert path & _lib.FUSED_PATH_RING, f"expected the ring kernel, last path = {path}"
            assert bool(path & _lib.FUSED_PATH_STRIP) == bool(baselines % STRIP), path
        else:
            assert path == _lib.FUSED_PATH_STRIP, path
        assert not fn._workspace.get(queue).any(), f"workspace after launch {launch}"
        noise = fn.buffer("noise").get(queue)
        flags = fn.buffer("flags").get(queue)
        np.testing.assert_array_equal(ref_noise, noise)
        np.testing.assert_array_equal(ref_flags, flags)
        # (the rows' padding is not the kernel's to write)
        assert (accel.HostArray.padded_view(flags)[:, baselines:] == 255).all()


@pytest.mark.parametrize("name", list(rs_in.FAMILIES))
def test_family(name, context, command_queue, cases):
    case = cases(name)
    CHECKS[name](case)
    run_ring(context, command_queue, case.family.vis, case.flags, case.noise)


@pytest.mark.parametrize("name", ["edges", "mixed"])
def test_family_simple_threshold(name, context, command_queue, cases, oracle):
    case = cases(name)
    CHECKS[name](case)
    # the oracle's own threshold stage on the deviations and the float64 noise it gave: what
    # flagger_full chains for threshold="simple" (tests/test_ring_strips.py holds it to that)
    with np.errstate(all="ignore"):
        ref_flags = oracle.ThresholdSimpleHost(N_SIGMA)(case.dev, case.noise64)
    assert ref_flags.any()
    run_ring(context, command_queue, case.family.vis, ref_flags, case.noise, threshold="simple")


@pytest.mark.parametrize("name", ["edges", "mixed"])
def test_family_flag_value_padded_vis(name, context, command_queue, cases):
    """``flag_value`` 0x80 and rows of `vis` padded by 16 elements. (The oracle writes
    `flag_value` where it writes 1: tests/test_ring_strips.py holds it to that.)"""
    case = cases(name)
    CHECKS[name](case)
    assert set(np.unique(case.flags).tolist()) == {0, 1}
    run_ring(context, command_queue, case.family.vis, case.flags * np.uint8(0x80), case.noise,
             flag_value=0x80, vis_pad=16)  # fmt: skip


@pytest.mark.parametrize("ring", [1, -1])
def test_lower_median_below_narrowed_bin(ring, context, command_queue, cases):
    """The baselines of `mixed` whose lower median lies below the narrowed bin and inside the
    key's, on their own, through the ring kernel and through the 4-baseline kernel (``mad_noise``
    is the same in both; it once took the value below the key's bin, a zero, there)."""
    case = cases("mixed")
    chosen = np.flatnonzero(case.lower_below)[:16]
    assert len(chosen) == 16
    vis = np.ascontiguousarray(case.family.vis[:, chosen])
    run_ring(context, command_queue, vis, case.flags[:, chosen], case.noise[chosen], ring=ring)


# Strip counts: grids smaller than the 8 ticket lists and grids that are no multiple of 8 leave
# lists that no workgroup owns, whose strips have to be stolen; n_cu and 2 n_cu are even shares.
BY_CU = {"n_cu-1": lambda n: n - 1, "n_cu": lambda n: n, "n_cu+1": lambda n: n + 1, "2*n_cu": lambda n: 2 * n}
STRIP_COUNTS = [2, 3, 7, 8, 9, 15, 16, 17, 63, 65] + list(BY_CU)
# (strips, baselines beyond them, elements of padding in the rows of `flags`)
STRIP_SHAPES = [(n, 0, 0) for n in STRIP_COUNTS] + [
    (3, 1, 5), (3, 7, 0), (9, 1, 0), (9, 7, 0), ("n_cu+1", 1, 0), ("n_cu+1", 7, 5)]  # fmt: skip


@pytest.mark.parametrize("strips, tail, flags_pad", STRIP_SHAPES)
@pytest.mark.parametrize("name", ["binades", "mixed"])
def test_strip_counts(name, strips, tail, flags_pad, n_cu, context, command_queue, cases):
    """The leading baselines of a family: the oracle's results for them are the leading columns
    of its results for the family (a baseline's flags and noise depend on nothing else)."""
    case = cases(name)
    if isinstance(strips, str):
        strips = BY_CU[strips](n_cu)
    baselines = STRIP * strips + tail
    assert baselines <= case.family.vis.shape[1]
    CHECKS[name](case, baselines)
    vis = np.ascontiguousarray(case.family.vis[:, :baselines])
    run_ring(context, command_queue, vis, case.flags[:, :baselines], case.noise[:baselines],
             flags_pad=flags_pad)  # fmt: skip


def test_one_workspace_many_launches(n_cu, context, command_queue, cases, oracle):
    """One 16-word workspace, zeroed once, through the C ABI: ring and 4-baseline launches in
    turn, the latter with at least 2048 strips of 4 baselines, for which ``set_schedule``
    (csrc/flagger_fused.hip) hands the last strips out dynamically, from the same words. Exact
    results and an all-zero workspace after every call."""
    from katsdpsigproc_amd import _lib, accel

    binades, mixed, edges = cases("binades"), cases("mixed"), cases("edges")
    check_binades(binades, 257 * STRIP)
    check_mixed(mixed, 9 * STRIP + 3)
    check_edges(edges)
    last = min(513 * STRIP, edges.family.vis.shape[1])  # (the family itself on a 256-CU device)
    ring, strip4 = _lib.FUSED_PATH_RING, _lib.FUSED_PATH_STRIP
    calls = [(binades, 257 * STRIP, ring), ((64, 8200), None, strip4),
             (mixed, 9 * STRIP + 3, ring | strip4), ((1024, 8196), None, strip4),
             (edges, last, ring)]  # fmt: skip
    device, stream = context.device.index, ctypes.c_void_p(command_queue.stream)
    scales = (ctypes.c_double * 4)(*[pow(1.2, -i) for i in range(4)])
    workspace = accel.DeviceArray(context, (16,), np.uint32)
    workspace.zero(command_queue)
    for source, baselines, want_path in calls:
        if baselines is None:
            channels, baselines = source
            assert -(-baselines // 4) >= 2048  # strips of 4: enough for a dynamic tail
            vis = inputs.add_rfi(inputs.generate_data(channels, baselines, seed=channels), seed=7)
            ref_flags, ref_noise = oracle.flagger_full(vis, width=rs_in.WIDTH, n_sigma=N_SIGMA, n_windows=4)
            ref_noise = ref_noise.astype(np.float32)
            assert ref_flags.any()
        else:
            channels = CHANNELS
            vis = source.family.vis[:, :baselines]
            ref_flags, ref_noise = source.flags[:, :baselines], source.noise[:baselines]
        what = f"{channels} x {baselines}"
        stride = baselines + baselines % 2  # (`vis` needs an even stride)
        d_vis = accel.DeviceArray(context, vis.shape, np.complex64, (channels, stride))
        d_flags = accel.DeviceArray(context, vis.shape, np.uint8)
        d_noise = accel.DeviceArray(context, (baselines,), np.float32)
        d_vis.set(command_queue, vis)
        d_flags.set(command_queue, np.full(vis.shape, 255, np.uint8))
        with _lib.fused_ring_mode(1):
            _lib.call("ksp_flagger_fused", device, stream, ctypes.c_void_p(d_vis.buffer.ptr), None,
                      ctypes.c_void_p(d_flags.buffer.ptr), None, ctypes.c_void_p(d_noise.buffer.ptr),
                      channels, baselines, stride, 0, baselines, 0, rs_in.WIDTH, 0, 0, 1, N_SIGMA,
                      scales, 4, 1, ctypes.c_void_p(workspace.buffer.ptr))  # fmt: skip
            assert _lib.call("ksp_flagger_fused_last_path") == want_path, what
        assert not workspace.get(command_queue).any(), "the workspace was not left zeroed: " + what
        np.testing.assert_array_equal(ref_noise, d_noise.get(command_queue), err_msg=what)
        np.testing.assert_array_equal(ref_flags, d_flags.get(command_queue), err_msg=what)
