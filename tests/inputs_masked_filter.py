"""Seeded inputs of the masked Gaussian filter cases, shared by
``golden/make_golden_masked_filter.py`` and the tests that check against its fixture."""

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "rfi_masked_filter_golden.npz")  # fmt: skip

#: name -> (shape, dtype, sigma, passes, data kind, flags kind, seed); the reference's
#: results for these are in GOLDEN. "lognormal" amplitudes span many binades, so that the
#: rounding of every running sum depends on the order of its additions.
CASES = {
    "half": ((77, 53), "float32", (5.0, 2.3), 4, "uniform", "half", 1),
    "block": ((77, 53), "float32", (3.0, 3.3), 4, "uniform", "block", 2),
    "half_f64_p3": ((77, 53), "float64", (5.0, 2.3), 3, "lognormal", "half", 3),
    "p5": ((40, 70), "float32", (4.0, 6.0), 5, "lognormal", "half", 4),
    "p1_f64": ((40, 70), "float64", (2.0, 3.0), 1, "lognormal", "half", 5),
    "p2": ((40, 70), "float32", (3.0, 1.5), 2, "lognormal", "sparse", 6),
    "p8_f64": ((30, 45), "float64", (2.0, 3.0), 8, "lognormal", "sparse", 7),
    # d = 69: float32 pow rounds 69 ** 4 to 22667122, squaring gives 22667120
    "d69_axis0": ((100, 12), "float32", (40.0, 0.0), 4, "lognormal", "sparse", 8),
    "d69_axis1": ((12, 100), "float32", (0.0, 40.0), 4, "lognormal", "sparse", 9),
    # box wider than the line
    "wide_axis0": ((3, 200), "float32", (30.0, 0.0), 4, "lognormal", "sparse", 10),
    "wide_axis1": ((200, 3), "float32", (0.0, 30.0), 4, "lognormal", "sparse", 11),
    "axis1_only": ((40, 70), "float32", (0.0, 9.0), 4, "lognormal", "half", 12),
    "axis0_only": ((40, 70), "float32", (30.0, 0.0), 4, "lognormal", "half", 13),
    "copy": ((20, 30), "float32", (0.0, 0.0), 4, "uniform", "half", 14),
}


def radius(sigma, passes):
    """Box radius of the reference's ``_box_gaussian_filter`` for one axis."""
    return int(0.5 * np.sqrt(12.0 * np.float64(sigma) ** 2 / passes + 1))


def make_data(shape, dtype, kind, seed):
    rs = np.random.RandomState(seed)
    if kind == "uniform":
        data = rs.uniform(0.0, 1.0, shape)
    elif kind == "lognormal":
        data = np.exp(6.0 * rs.standard_normal(shape))
    else:
        raise ValueError(kind)
    return data.astype(dtype)


def make_flags(shape, kind, seed):
    """Boolean flags. half: every sample with probability 1/2; sparse: 1/10; block: only
    [30:70, 10:40] of the last two axes; none; all."""
    rs = np.random.RandomState(seed + 1000)
    if kind == "half":
        return rs.uniform(size=shape) < 0.5
    if kind == "sparse":
        return rs.uniform(size=shape) < 0.1
    flags = np.zeros(shape, np.bool_)
    if kind == "block":
        flags[..., 30:70, 10:40] = True
    elif kind == "all":
        flags[:] = True
    elif kind != "none":
        raise ValueError(kind)
    return flags


def make_inputs(shape, dtype, data_kind, flags_kind, seed):
    return make_data(shape, dtype, data_kind, seed), make_flags(shape, flags_kind, seed)


def make_case(name):
    shape, dtype, _sigma, _passes, data_kind, flags_kind, seed = CASES[name]
    return make_inputs(shape, dtype, data_kind, flags_kind, seed)


def case_list():
    return [{"name": n, "shape": list(c[0]), "dtype": c[1], "sigma": list(c[2]), "passes": c[3],
             "data": c[4], "flags": c[5], "seed": c[6]} for n, c in CASES.items()]  # fmt: skip
