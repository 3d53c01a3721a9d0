"""The inputs of tests/inputs_ring_strips.py on the CPU, at the shape of a 256-CU device (4104
baselines): the oracle alone reaches what each family is for, and the hit test of the hinted MAD
search cannot be off by one on them without changing a result (``hinted_search`` with the true
test and with wrong ones). tests/test_gpu_ring_strips.py then runs the ring kernel on the
same inputs."""

import numpy as np
import pytest

from tests import inputs_ring_strips as rs_in

BASELINES = rs_in.baselines_for(256)
POSITIONS = rs_in.STRIP


@pytest.fixture(scope="module")
def oracle():
    from oracle import rfi_oracle

    rfi_oracle.set_threads(rfi_oracle.max_threads())
    yield rfi_oracle
    rfi_oracle.set_threads(1)


@pytest.fixture(scope="module")
def reference(oracle):
    """name -> (family, oracle flags, oracle noise, MadBin); each computed once."""
    made = {}

    def get(name):
        if name not in made:
            family = rs_in.FAMILIES[name](BASELINES)
            with np.errstate(all="ignore"):
                flags, noise, dev = oracle.flagger_full(
                    family.vis, width=rs_in.WIDTH, n_sigma=11.0, n_windows=4, want_deviations=True)
            made[name] = (family, flags, noise, rs_in.mad_bin(dev), dev if name == "edges" else None)
        return made[name]

    return get


def shares(values, position):
    """The share of each distinct value among the baselines at one position ``b % 8``."""
    mine = values[position :: rs_in.STRIP]
    found, count = np.unique(mine, return_counts=True)
    return dict(zip(found.tolist(), (count / len(mine)).tolist()))


def test_shape():
    assert BASELINES == 4104
    for build in rs_in.FAMILIES.values():
        family = build(64)  # (the builders take any count)
        assert family.vis.shape == (4096, 64) and family.vis.dtype == np.complex64
        assert family.kind.shape == (64,)


def test_binades(reference):
    family, _, _, bins, _ = reference("binades")
    assert bins.searched.all()
    e = family.extra["e"]
    assert e.min() == -60 and e.max() == 60
    # samples below the short division's lower limit (2^-63 for the larger component) among
    # ordinary ones, in at least a strip's worth of baselines; e <= 60 keeps every sample below
    # the upper limit of 2^65, which the 2^100 baselines of `mixed` are beyond
    larger = np.maximum(np.abs(family.vis.real), np.abs(family.vis.imag))
    small = (larger < 2.0 ** -63).sum(axis=0)
    assert ((small > 0) & (small < rs_in.CHANNELS)).sum() >= 8
    assert larger.max() < 2.0 ** 65
    largest, distinct = 0.0, []
    for w in range(POSITIONS):
        share = shares(bins.top, w)
        largest = max(largest, max(share.values()))
        distinct.append(len(share))
    print(f"binades: largest share of one top {largest:.3f}, distinct tops per position {distinct}")
    assert largest <= 0.05


def test_neighbours(reference):
    family, _, _, bins, _ = reference("neighbours")
    A = rs_in.NEIGHBOUR_TOP
    assert bins.searched.all()
    np.testing.assert_array_equal(bins.top, A - 1 + family.kind)
    for w in range(POSITIONS):
        share = shares(bins.top, w)
        print(f"neighbours, position {w}: {share}")
        assert set(share) == {A - 1, A, A + 1}
        assert min(share.values()) >= 0.20


def test_edges(reference):
    family, flags, noise, bins, dev = reference("edges")
    h = rs_in.EDGE_TOP
    counts = rs_in.position_counts(family.kind, len(family.kinds))
    print("edges, baselines per position and kind:", dict(zip(family.kinds, counts.T.tolist())))
    per_position = BASELINES // POSITIONS
    assert (counts[:, :3] >= 0.15 * per_position).all()
    assert (counts[:, 3:] >= 8).all()
    # the fillers have the tops they are there for
    filler = family.kind < 3
    np.testing.assert_array_equal(bins.top[filler], h - 1 + family.kind[filler])
    # every deviation of a constructed baseline is its x, and nothing else deviates
    built = ~filler
    np.testing.assert_array_equal(dev[4::8][:, built], family.extra["x"][:, built])
    rest = np.ones(rs_in.CHANNELS, bool)
    rest[4::8] = False
    assert not dev[rest][:, built].any()
    # the rank lies where the class says, for the hint h
    at_h = rs_in.mad_bin(dev, hint=h)
    low, high = at_h.rank - at_h.lb, at_h.rank - (at_h.lb + at_h.cnt)
    for k in range(3, len(family.kinds)):
        cls, parity = family.kinds[k].rsplit("_", 1)
        mine = family.kind == k
        nonzero = rs_in.TOTAL - at_h.zeros[mine]
        assert (nonzero == (512 if parity == "even" else 511)).all(), family.kinds[k]
        want_low, want_high = rs_in.EDGE_RIMS[cls]
        if want_low is not None:
            assert (low[mine] == want_low).all(), family.kinds[k]
        if want_high is not None:
            assert (high[mine] == want_high).all(), family.kinds[k]
        assert (at_h.cnt[mine] >= 1).all()
        on_h = cls in ("last_of_h", "first_of_h", "straddle")
        assert ((bins.top[mine] == h) == on_h).all(), family.kinds[k]
        if cls == "straddle":
            # the two middle samples: the last value below the bin, the first one inside it
            both = np.sort(np.abs(dev[:, mine]), axis=0)[[-257, -256]]
            np.testing.assert_array_equal(both[0], (rs_in.K_IN_LO - 1) * 2.0 ** -23)
            np.testing.assert_array_equal(both[1], rs_in.K_IN_LO * 2.0 ** -23)
    # values that only the key's rounding carries into the next top, on both rims
    k = np.abs(family.extra["x"][:, built]) * 2.0 ** 23
    assert ((k >= rs_in.K_IN_LO) & (k < 8192)).sum() >= built.sum()
    assert ((k > rs_in.K_IN_HI) & (k < 16384)).sum() >= built.sum()
    # the reference flags the excursions of +2^-3 (the thresholds are one-sided)
    planted = family.extra["x"][:, built] == 0.125
    assert planted.sum() >= built.sum() and (flags[4::8][:, built][planted] == 1).all()


def test_mixed(reference, oracle):
    family, flags, noise, bins, _ = reference("mixed")
    counts = rs_in.position_counts(family.kind, len(family.kinds))
    print("mixed, baselines per position and kind:", dict(zip(family.kinds, counts.T.tolist())))
    assert (counts >= 4).all()
    every = set(range(len(family.kinds)))
    assert set(family.kind[:16].tolist()) == every and set(family.kind[-16:].tolist()) == every
    name = np.array(family.kinds)[family.kind]
    np.testing.assert_array_equal(np.isnan(noise), (name == "zero") | (name == "constant"))
    # the early returns of the search: no deviation at all, and the median among the +-2^-150
    np.testing.assert_array_equal(bins.zeros == rs_in.TOTAL, np.isnan(noise))
    np.testing.assert_array_equal(~bins.searched & ~np.isnan(noise), name == "tiny")
    assert (bins.tiny[name == "tiny"] >= 1).all()
    np.testing.assert_array_equal(noise[name == "tiny"], 2.0 ** -150 * 1.4826)
    # the sorted-window fallback is taken for an amplitude that is NaN or infinite
    with np.errstate(all="ignore"):
        amp = np.abs(family.vis)
    np.testing.assert_array_equal(
        (~np.isfinite(amp)).any(axis=0), np.isin(name, ["nan", "inf", "overflow"]))
    # a lower median below the narrowed bin, inside the key's (subnormal deviations all have key 1)
    small = name == "2^-140"
    _, _, dev = oracle.flagger_full(np.ascontiguousarray(family.vis[:, small]), n_sigma=11.0, want_deviations=True)
    found = int(rs_in.narrowed_lower_below(dev, 256).sum())
    print(f"mixed: {found} of {int(small.sum())} baselines of 2^-140 with the lower median inside the key's bin")
    assert found >= 8
    larger = np.maximum(np.abs(family.vis.real), np.abs(family.vis.imag))[:, name == "2^100"]
    assert (larger >= 2.0 ** 65).all()  # beyond the short division's upper limit
    assert flags.any()


def hints_at_positions(top):
    """(baseline, hint) pairs: every baseline with every top that occurs at its position ``b % 8``
    (what an earlier strip of its wavefront may have left) and with no hint."""
    baseline, hint = [], []
    for w in range(POSITIONS):
        mine = np.arange(w, len(top), rs_in.STRIP)
        tops = np.unique(np.concatenate([top[mine][top[mine] >= 0], [-1]]))
        baseline.append(np.repeat(mine, len(tops)))
        hint.append(np.tile(tops, len(mine)))
    return np.concatenate(baseline), np.concatenate(hint)


@pytest.mark.parametrize("name", list(rs_in.FAMILIES))
def test_model_equals_classifier(name, reference):
    """The true hit test finds the key at the MAD's rank whatever hint arrives."""
    bins = reference(name)[3]
    baseline, hint = hints_at_positions(bins.top)
    live = bins.searched[baseline]
    baseline, hint = baseline[live], hint[live]
    key, steps = rs_in.hinted_search(bins.keys, bins.rank[baseline], hint, rs_in.TRUE, baseline)
    np.testing.assert_array_equal(key, bins.key[baseline])
    np.testing.assert_array_equal(steps == 7, (hint == bins.top[baseline]))
    print(f"{name}: {len(baseline)} searches, {int((steps == 7).sum())} hits")


def test_data_bites(reference):
    """Each wrong hit test changes the key bin of some ``edges`` baseline, under each of the
    hints h - 1, h and h + 1 taken together. ``lb < rank`` is the exception that the search
    itself allows: a hit refused falls through to the full search, which is exact, so that
    mistake costs time and no result -- the test shows the refused hits instead."""
    family, _, _, bins, _ = reference("edges")
    h = rs_in.EDGE_TOP
    every = np.flatnonzero(bins.searched)
    changed = {variant: 0 for variant in rs_in.WRONG_VARIANTS}
    refused = 0
    for hint in (h - 1, h, h + 1):
        true_key, true_steps = rs_in.hinted_search(bins.keys, bins.rank[every], hint, rs_in.TRUE, every)
        np.testing.assert_array_equal(true_key, bins.key[every])
        for variant in rs_in.WRONG_VARIANTS:
            key, steps = rs_in.hinted_search(bins.keys, bins.rank[every], hint, variant, every)
            changed[variant] += int((key != true_key).sum())
            if variant == rs_in.LT_LOWER:
                refused += int(((steps == 15) & (true_steps == 7)).sum())
    print(f"edges: key bins changed {changed}, hits refused by 'lb < rank': {refused}")
    assert changed[rs_in.LE_UPPER] >= 1 and changed[rs_in.ALWAYS] >= 1 and changed[rs_in.LE_LOWER] >= 1
    assert changed[rs_in.LT_LOWER] == 0 and refused >= 1


@pytest.mark.parametrize("name", ["edges", "mixed"])
def test_other_thresholds_from_one_reference(name, reference, oracle):
    """tests/test_gpu_ring_strips.py calls ``flagger_full`` once per input and derives the simple
    threshold and ``flag_value`` 0x80 from that call's deviations, noise and flags: on the first
    and last 64 baselines, ``flagger_full`` asked for them directly gives the same."""
    family, flags, noise, _, _ = reference(name)
    for part in (slice(0, 64), slice(BASELINES - 64, BASELINES)):
        vis = np.ascontiguousarray(family.vis[:, part])
        with np.errstate(all="ignore"):
            _, _, dev = oracle.flagger_full(vis, n_sigma=11.0, want_deviations=True)
            simple, simple_noise = oracle.flagger_full(vis, threshold="simple", n_sigma=11.0)
            staged = oracle.ThresholdSimpleHost(11.0)(dev, noise[part])
            valued, _ = oracle.flagger_full(vis, n_sigma=11.0, flag_value=0x80)
        np.testing.assert_array_equal(simple_noise, noise[part])
        np.testing.assert_array_equal(staged, simple)
        np.testing.assert_array_equal(flags[:, part] * np.uint8(0x80), valued)
        assert simple.any() and valued.any()
