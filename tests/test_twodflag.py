"""2-D SumThreshold flagger: constructor conditioning, argument errors and the C-ABI
checks, without a GPU."""

import ctypes
import json

import numpy as np
import pytest

from katsdpsigproc_amd.rfi import twodflag
from tests import inputs_twodflag as inputs


def test_windows_freq_scaled_and_unique():
    f = twodflag.SumThresholdFlagger(windows_freq=[1, 2, 4, 8, 3], average_freq=4)
    np.testing.assert_array_equal(f.windows_freq, [1, 2])
    assert f.windows_freq.dtype == np.int_
    f = twodflag.SumThresholdFlagger(windows_freq=[8, 1, 5], average_freq=3)
    np.testing.assert_array_equal(f.windows_freq, [1, 2, 3])


def test_spike_width_and_min_dtypes():
    f = twodflag.SumThresholdFlagger(spike_width_freq=10.0, average_freq=4, time_extend=300)
    assert f.spike_width_freq == 2.5
    assert f.average_freq.dtype == np.uint8 and int(f.average_freq) == 4
    assert f.time_extend.dtype == np.uint16 and f.freq_extend.dtype == np.uint8


def test_chunk_ends_and_window_clipping():
    f = twodflag.SumThresholdFlagger(freq_chunks=3, average_freq=3,
                                     windows_time=[1, 2, 40, 60], windows_freq=[3, 30, 300])  # fmt: skip
    p = f._params(24, 50, False)
    # 17 averaged channels; numpy.linspace(0, 17, 4).astype(int)
    assert [p.chunk_ends[i] for i in range(4)] == [0, 5, 11, 17]
    # windows_time is clipped against the CHANNEL count (50), not the 24 dumps
    assert [p.windows_time[i] for i in range(p.n_windows_time)] == [1, 2, 40]
    assert [p.windows_freq[i] for i in range(p.n_windows_freq)] == [1, 10]
    assert p.tf_time[2] == pow(1.3, np.log2(40))


def test_more_chunks_than_channels():
    p = twodflag.SumThresholdFlagger(freq_chunks=40)._params(8, 24, False)
    ends = [p.chunk_ends[i] for i in range(41)]
    assert ends == list(np.linspace(0, 24, 41).astype(int))
    assert ends[1] == 0  # empty chunks


def test_argument_errors():
    f = twodflag.SumThresholdFlagger()
    with pytest.raises(ValueError):
        f.get_flags(np.zeros((4, 8, 2), np.float32), np.zeros((4, 8, 3), np.bool_))
    with pytest.raises(ValueError):
        f.get_flags(np.zeros((4, 8), np.float32), np.zeros((4, 8), np.bool_))
    with pytest.raises(TypeError):
        f.get_flags(np.zeros((4, 8, 2), np.complex128), np.zeros((4, 8, 2), np.bool_))
    with pytest.raises(TypeError):
        f.get_flags(np.zeros((4, 8, 2), np.float64), np.zeros((4, 8, 2), np.bool_))
    with pytest.raises(ValueError, match="n_time"):
        f._params(5000, 64, False)
    with pytest.raises(ValueError, match="channels"):
        f._params(10, 70000, False)
    with pytest.raises(ValueError, match="freq_chunks"):
        twodflag.SumThresholdFlagger(freq_chunks=513)
    with pytest.raises(ValueError, match="zero-size"):
        twodflag.SumThresholdFlagger(windows_time=[4])._params(10, 2, False)


@pytest.fixture(scope="module")
def lib():
    import os

    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    return _lib.load()


def test_launchers_check_arguments_without_gpu(lib):
    from katsdpsigproc_amd import _lib

    p = twodflag.SumThresholdFlagger()._params(16, 64, False)
    size = ctypes.c_size_t()
    assert lib.ksp_twodflag_workspace(ctypes.byref(p), 2, ctypes.byref(size)) == 0
    assert size.value > 2 * 16 * 64 * 4
    v = ctypes.c_void_p(8)
    # every failure below is reported before any device call
    rc = lib.ksp_twodflag(0, None, None, v, v, 2, 128 * 2, 2, 0, 2, ctypes.byref(p), v, size.value)
    assert rc != 0 and "NULL" in _lib.last_error()
    rc = lib.ksp_twodflag(0, None, v, v, v, 2, 64 * 2, 2, 1, 2, ctypes.byref(p), v, size.value)
    assert rc != 0 and "bl0" in _lib.last_error()
    rc = lib.ksp_twodflag(0, None, v, v, v, 2, 64 * 2, 2, 0, 2, ctypes.byref(p), v, 16)
    assert rc != 0 and "workspace" in _lib.last_error()
    for field, value, word in [("n_time", 5000, "n_time"), ("n_freq", 0, "n_freq"),
                               ("n_chunks", 600, "n_chunks"), ("n_windows_time", 0, "windows"),
                               ("background_iterations", 65, "iterations")]:  # fmt: skip
        q = twodflag.SumThresholdFlagger()._params(16, 64, False)
        setattr(q, field, value)
        rc = lib.ksp_twodflag_workspace(ctypes.byref(q), 1, ctypes.byref(size))
        assert rc != 0 and word in _lib.last_error(), field
    q = twodflag.SumThresholdFlagger()._params(16, 64, False)
    q.chunk_ends[q.n_chunks] = 63
    assert lib.ksp_twodflag_workspace(ctypes.byref(q), 1, ctypes.byref(size)) != 0
    assert "chunk_ends" in _lib.last_error()


def test_golden_cases_match_inputs():
    with np.load(inputs.GOLDEN) as g:
        cases = json.loads(str(g["cases"]))
        assert cases == json.loads(json.dumps(inputs.case_list(), sort_keys=True))
        for case in cases:
            n = int(np.prod(case["shape"]))
            assert g[case["name"] + "_flags"].size == (n + 7) // 8
        stage = inputs.CASES[inputs.STAGE_CASE][0]
        assert g[inputs.STAGE_CASE + "_background"].shape == (stage[2], stage[0], stage[1])
