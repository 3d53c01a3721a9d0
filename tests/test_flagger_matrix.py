"""The case table of tests/flagger_matrix.py, without a GPU: it covers every pair of option
levels, every case has something to find, and ``rfi.host.FlaggerHost`` equals the oracle on
every case (the ingest tests take the host classes as their reference)."""

import warnings
from collections import Counter

import numpy as np
import pytest

from tests import flagger_matrix as fm

CASE_IDS = [case.id for case in fm.CASES]


class TestTable:
    def test_levels_are_the_agreed_ones(self):
        """No level of the agreed factors has been dropped (more may be added)."""
        agreed = {
            "channels": {40, 200, 700, 3000, 4096, 5000, 9100, 13000},
            "width": {3, 7, 13, 21, 31, 63},
            "threshold": {"simple", "sum1", "sum4", "sum6", "sum8"},
            "mask": {"NONE", "CHANNEL", "FULL"},
            "input": {"complex", "amplitude"},
            "keep_deviations": {False, True},
            "baselines": {3, 8, 11, 17},
            "flag_value": {1, 0x80},
            "sigma": {(11.0, 1.2), (6.0, 1.5)},
            "engine": {"auto", "seq_mad_cm", "seq_madt_cm", "seq_mad_t", "seq_madt_t"},
            "data": {"sparse", "broad", "ties", "specials"},
            "vis_pad": {0, 16},
        }
        table = dict(fm.FACTORS)
        assert set(table) == set(agreed)
        for name, levels in agreed.items():
            assert levels <= set(table[name]), name

    def test_cases_use_known_levels_and_are_distinct(self):
        for case in fm.CASES:
            for (name, levels), value in zip(fm.FACTORS, case):
                assert value in levels, (case.id, name)
        assert len(set(CASE_IDS)) == len(CASE_IDS)
        assert len({case.seed for case in fm.CASES}) == len(fm.CASES)

    def test_every_pair_of_levels_occurs(self):
        wanted = set(fm.all_pairs())
        levels = [len(lv) for _, lv in fm.FACTORS]
        assert len(wanted) == (sum(levels) ** 2 - sum(n * n for n in levels)) // 2
        covered = set()
        for case in fm.PAIRWISE_CASES:
            covered |= fm.pairs_of(case)
        missing = sorted(wanted - covered, key=repr)
        assert not missing, [
            (fm.FACTOR_NAMES[i], a, fm.FACTOR_NAMES[j], b) for i, a, j, b in missing[:10]]

    def test_ring_cases_are_the_hand_placed_ones(self):
        eligible = [case for case in fm.CASES if fm.ring_eligible(case)]
        assert eligible == list(fm.RING_CASES)
        assert len(eligible) >= 6
        assert {c.threshold for c in eligible} == {"simple", "sum1", "sum4"}
        assert {c.baselines for c in eligible} == {8, 11, 17}
        assert {c.flag_value for c in eligible} == {1, 0x80}
        assert {c.sigma for c in eligible} == {(11.0, 1.2), (6.0, 1.5)}
        assert {c.data for c in eligible} == {"sparse", "broad", "ties", "specials"}
        assert {c.vis_pad for c in eligible} == {0, 16}

    def test_every_kernel_class_is_met_in_combination(self):
        """Each class of the fused dispatch runs at least twice without the ring kernel, and
        with amplitude input, a mask, kept deviations, the simple threshold and the other flag
        value at least once each; the sequence runs under every wiring."""
        by_class = {}
        for case in fm.CASES:
            by_class.setdefault(fm.kernel_class(case, ring_allowed=False), []).append(case)
        for name in ("strip4", "strip16", "strip64", "long4", "long3"):
            cases = by_class[name]
            assert len(cases) >= 2, name
            assert any(c.amplitudes for c in cases), name
            assert any(c.mask == "FULL" for c in cases), name
            assert any(c.keep_deviations for c in cases), name
            assert any(not c.keep_deviations for c in cases), name
            assert any(c.threshold == "simple" for c in cases), name
            assert any(c.flag_value == 0x80 for c in cases), name
            assert any(c.vis_pad == 16 for c in cases), name
        assert {c.engine for c in by_class["sequence"]} == set(dict(fm.FACTORS)["engine"])
        # under "auto" the sequence takes what the fused kernels decline, for each of their reasons
        declined = [c for c in by_class["sequence"] if not c.forced_sequence]
        assert any(c.width > 31 for c in declined)
        assert any(c.channels > 12288 for c in declined)
        assert any(c.channels > 4096 and c.n_windows > 4 for c in declined)
        assert any(4096 < c.channels <= 12288 and c.width != 13 for c in declined)

    def test_class_counts(self):
        """The counts the table was built to: recorded here so that a change shows."""
        counts = Counter(fm.kernel_class(case) for case in fm.CASES)
        assert len(fm.PAIRWISE_CASES) == 50 and len(fm.CASES) == 71
        assert counts == {"sequence": 44, "strip64": 12, "ring": 7, "strip4": 2, "strip16": 2,
                          "long4": 2, "long3": 2}  # fmt: skip


@pytest.mark.parametrize("case", fm.CASES, ids=CASE_IDS)
class TestCases:
    def test_case_is_worth_running(self, case):
        flags, noise, dev = fm.reference(case)
        assert set(np.unique(flags)) == {0, case.flag_value}  # some flags, not all
        assert np.isfinite(noise).any()
        assert np.isfinite(dev).all() or case.data == "specials"
        mask = fm.make_mask(case)
        if mask is not None:
            under = np.broadcast_to(mask[:, None] if mask.ndim == 1 else mask, flags.shape) != 0
            assert under.any() and not under.all()
            if case.n_windows == 1:
                # (a wider window flags all its samples, masked ones of deviation 0 included)
                assert not flags[under].any()
            # the mask has hidden something that would have been flagged
            assert fm.reference_flags(case, masked=False)[under].any()
        if case.data == "broad" and case.n_windows >= 6 and case.channels >= 700:
            # the widest window has found something the narrower ones do not
            narrower = fm.reference_flags(case, n_windows=case.n_windows - 1)
            assert (flags != narrower).any()
        if case.data == "specials":
            # all-zero and constant baselines: no non-zero deviation, NaN noise, nothing flagged
            assert np.isnan(noise[:2]).all() and not flags[:, :2].any()

    def test_host_flagger_equals_oracle(self, case):
        from katsdpsigproc_amd.rfi import host

        background = host.BackgroundMedianFilterHost(case.width, case.amplitudes)
        if case.sum_threshold:
            threshold = host.ThresholdSumHost(case.n_sigma, case.n_windows,
                                              case.threshold_falloff, case.flag_value)  # fmt: skip
        else:
            threshold = host.ThresholdSimpleHost(case.n_sigma, case.flag_value)
        flagger = host.FlaggerHost(background, host.NoiseEstMADHost(), threshold)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore", RuntimeWarning)
            flags = flagger(fm.make_input(case), fm.make_mask(case))
        np.testing.assert_array_equal(fm.reference(case)[0], flags)
