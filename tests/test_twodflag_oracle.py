"""The NumPy oracle of the 2-D flagger against the reference's goldens, bit for bit, stage
by stage; the workspace layout query, without a GPU."""

import ctypes
import json

import numpy as np
import pytest

from katsdpsigproc_amd.rfi import twodflag
from oracle import twodflag_oracle as oracle
from tests import inputs_twodflag as inputs


@pytest.fixture(scope="module")
def golden():
    with np.load(inputs.GOLDEN) as g:
        return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def stages_golden():
    with np.load(inputs.STAGES_GOLDEN) as g:
        return {k: g[k] for k in g.files}


def unpack(packed, shape):
    return np.unpackbits(packed)[: int(np.prod(shape))].reshape(shape).astype(np.bool_)


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", sorted(inputs.CASES))
def test_oracle_matches_golden_flags(golden, name):
    shape, _, _, params = inputs.CASES[name]
    data, flags = inputs.make_case(name)
    out, _ = oracle.flag(data, flags, **params)
    expected = unpack(golden[name + "_flags"], shape)
    assert np.array_equal(out, expected), f"{int((out != expected).sum())} flags differ"


def test_oracle_matches_chunks1_stages(golden):
    name = inputs.STAGE_CASE
    data, flags = inputs.make_case(name)
    _, st = oracle.flag(data, flags, **inputs.CASES[name][3])
    assert same_bits(st["background"], golden[name + "_background"])
    tfl = st["time_flags"].astype(np.bool_)
    assert np.array_equal(tfl, unpack(golden[name + "_time_flags"], tfl.shape))


def test_stage_golden_lists_its_cases(stages_golden):
    assert json.loads(str(stages_golden["cases"])) == inputs.STAGE_CASES
    wide = [inputs.CASES[n][3] for n in inputs.STAGE_CASES]
    # at least one recorded case has a box radius of 32 or more
    assert max(oracle.radius(kw.get("spike_width_time", 12.5) * kw.get("background_iterations", 1))
               for kw in wide) >= 32  # fmt: skip


@pytest.mark.parametrize("name", inputs.STAGE_CASES)
def test_oracle_matches_every_recorded_stage(stages_golden, name):
    data, flags = inputs.make_case(name)
    _, st = oracle.flag(data, flags, **inputs.CASES[name][3])
    mine = dict(st)
    mine["unaveraged"] = (st["row_flags"] | st["row_all"][:, :, None]
                          | st["col_all"][:, None, :])  # fmt: skip
    for stage, is_float in inputs.RECORDED_STAGES.items():
        ref = stages_golden[f"{name}_{stage}"]
        if is_float:
            ok = same_bits(mine[stage], ref)
        else:
            ok = np.array_equal(mine[stage].astype(np.bool_), unpack(ref, mine[stage].shape))
        assert ok, f"{name}: stage {stage} differs"


def test_oracle_conditions_like_the_host_class():
    """The oracle's own conditioning agrees with the parameters the launcher receives."""
    kw = {"windows_time": inputs.WINDOWS_TIME_32[:31] + [100], "windows_freq": [8, 1, 5, 3, 3, 60],
          "average_freq": 3, "freq_chunks": 7, "rho": 1.7, "spike_width_freq": 10.0}  # fmt: skip
    cfg = oracle.Config(24, 70, **kw)
    p = twodflag.SumThresholdFlagger(**kw)._params(24, 70, False)
    assert cfg.windows_time == [p.windows_time[i] for i in range(p.n_windows_time)]
    assert cfg.windows_time == inputs.WINDOWS_TIME_32[:31]  # order and duplicates kept, 100 > 70
    assert cfg.windows_freq == [p.windows_freq[i] for i in range(p.n_windows_freq)] == [1, 2, 3, 20]
    assert cfg.tf_time == [p.tf_time[i] for i in range(p.n_windows_time)]
    assert cfg.chunks == [(p.chunk_ends[i], p.chunk_ends[i + 1]) for i in range(p.n_chunks)]
    assert cfg.spike_width_freq == p.spike_width_freq
    assert cfg.threshold_scale == p.threshold_scale and cfg.reject_scale == p.reject_scale


def test_box_divisor_is_numba_float32_squaring():
    assert oracle.divisor(10) == np.float32(21**4)
    assert oracle.divisor(32) == np.float32(17850624.0)  # 65 ** 4 = 17850625
    assert oracle.divisor(34) == np.float32(22667120.0)  # NumPy's float32 power: 22667122


# ------------------------------------------------------------------ layout query
@pytest.fixture(scope="module")
def lib():
    import os

    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    return _lib.load()


def stage_bytes(params, batch):
    """stage -> bytes of its region for `batch` baselines."""
    T, F = params.n_time, params.n_freq
    A = (F + params.average_freq - 1) // params.average_freq
    dims = {"B": batch, "T": T, "A": A, "F": F}
    return {name: int(np.prod([dims[c] for c in axes])) * np.dtype(dtype).itemsize
            for name, (dtype, axes) in oracle.STAGES.items()}  # fmt: skip


def test_layout_checks_arguments(lib):
    from katsdpsigproc_amd import _lib

    p = twodflag.SumThresholdFlagger()._params(16, 64, False)
    out = _lib.TwodflagOffsets()
    assert lib.ksp_twodflag_layout(ctypes.byref(p), 1, ctypes.byref(out)) == 0
    assert lib.ksp_twodflag_layout(ctypes.byref(p), 1, None) != 0
    assert "NULL" in _lib.last_error()
    assert lib.ksp_twodflag_layout(None, 1, ctypes.byref(out)) != 0
    assert "NULL" in _lib.last_error()
    assert lib.ksp_twodflag_layout(ctypes.byref(p), 0, ctypes.byref(out)) != 0
    assert "batch" in _lib.last_error()
    for field, value, word in [("n_time", 5000, "n_time"), ("n_freq", 0, "n_freq"),
                               ("n_chunks", 600, "n_chunks"), ("n_windows_freq", 33, "windows"),
                               ("background_iterations", -1, "iterations"),
                               ("spike_width_time", 5000.0, "spike width")]:  # fmt: skip
        q = twodflag.SumThresholdFlagger()._params(16, 64, False)
        setattr(q, field, value)
        assert lib.ksp_twodflag_layout(ctypes.byref(q), 1, ctypes.byref(out)) != 0, field
        assert word in _lib.last_error(), field


@pytest.mark.parametrize("shape, kw, batch", [
    ((16, 64), {}, 1),
    ((1, 1), {}, 3),
    ((48, 4096), {"average_freq": 7, "freq_chunks": 37}, 8),
    ((4096, 48), {"windows_time": inputs.WINDOWS_TIME_32, "spike_width_time": 2360.0}, 2),
    ((8, 65536), {"freq_chunks": 512, "spike_width_freq": 2360.0}, 2),
])  # fmt: skip
def test_layout_offsets_aligned_disjoint_inside_workspace(lib, shape, kw, batch):
    from katsdpsigproc_amd import _lib

    p = twodflag.SumThresholdFlagger(**kw)._params(*shape, False)
    out = _lib.TwodflagOffsets()
    assert lib.ksp_twodflag_layout(ctypes.byref(p), batch, ctypes.byref(out)) == 0
    size = ctypes.c_size_t()
    assert lib.ksp_twodflag_workspace(ctypes.byref(p), batch, ctypes.byref(size)) == 0
    sizes = stage_bytes(p, batch)
    assert sorted(sizes) == sorted(name for name, _ in _lib.TwodflagOffsets._fields_)
    regions = sorted((getattr(out, name), getattr(out, name) + n, name)
                     for name, n in sizes.items())  # fmt: skip
    for start, end, name in regions:
        assert start % 256 == 0, name
        assert end <= size.value, name
    for (_, end, a), (start, _, b) in zip(regions, regions[1:]):
        assert end <= start, f"{a} overlaps {b}"
