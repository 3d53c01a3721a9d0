"""The C-ABI library loads without a GPU and exports exactly what the header declares."""

import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "katsdpsigproc_hip.h")


def header_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ksp_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    return _lib.load()


def test_header_and_binding_agree():
    from katsdpsigproc_amd import _lib

    assert header_functions() == _lib.declared_symbols()


def test_every_declared_symbol_is_exported(lib):
    for name in header_functions():
        assert hasattr(lib, name), f"{name} is declared in the header but not exported"


def test_abi_version_and_no_device_calls(lib):
    from katsdpsigproc_amd import _lib

    assert lib.ksp_abi_version() == _lib.ABI_VERSION == 5
    count = ctypes.c_int(-1)
    assert lib.ksp_device_count(ctypes.byref(count)) == 0
    assert count.value >= 0  # 0 in the CPU container
    assert lib.ksp_flagger_fused_supported(4096, 13, 4) == 1
    assert lib.ksp_flagger_fused_supported(8192, 13, 4) == 1
    assert lib.ksp_flagger_fused_supported(10240, 13, 4) == 1
    assert lib.ksp_flagger_fused_supported(12289, 13, 4) == 0
    assert lib.ksp_flagger_fused_supported(8192, 5, 4) == 0
    assert lib.ksp_flagger_fused_supported(4096, 5, 4) == 1
    assert lib.ksp_flagger_fused_supported(4096, 25, 4) == 1  # (round 3: widths up to 31)
    assert lib.ksp_flagger_fused_supported(4096, 33, 4) == 0
    assert lib.ksp_flagger_fused_supported(4096, 13, 8) == 1  # (round 3: up to 8 windows)
    assert lib.ksp_flagger_fused_supported(4096, 13, 9) == 0
    assert lib.ksp_flagger_fused_supported(8192, 13, 5) == 0
    assert lib.ksp_flagger_fused_last_path() == 0  # no launch yet on this thread
    before = lib.ksp_flagger_fused_ring_mode(1)
    assert before in (-1, 0, 1) and lib.ksp_flagger_fused_ring_mode(7) == 1  # (7: query only)
    assert lib.ksp_flagger_fused_ring_mode(before) == 1
    assert lib.ksp_flagger_fused_supported(4096, 12, 4) == 0
    seg_len, n_segs = ctypes.c_int(-1), ctypes.c_int(-1)
    out = (ctypes.byref(seg_len), ctypes.byref(n_segs))
    assert lib.ksp_background_median_filter_geometry(4096, 8192, 13, 0, *out) == 0
    assert (seg_len.value, n_segs.value) == (64, 64)  # the 64 segments of test_config3_shape
    assert lib.ksp_background_median_filter_geometry(417, 313, 13, 4, *out) == 0
    assert (seg_len.value, n_segs.value) == (105, 4)


def test_missing_library_fails_loudly(tmp_path, monkeypatch):
    """No CPU fallback: a missing library is a RuntimeError, not a silent detour."""
    from katsdpsigproc_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(RuntimeError, match="no CPU fallback|not been built"):
        _lib.load(str(tmp_path / "nope.so"))


def test_argument_validation_without_gpu(lib):
    """Launchers validate shapes before touching the device."""
    from katsdpsigproc_amd import _lib

    rc = lib.ksp_madnz_t(0, None, None, None, 16, 4, 16)
    assert rc != 0 and "NULL" in _lib.last_error()
    rc = lib.ksp_threshold_sum(0, None, ctypes.c_void_p(8), ctypes.c_void_p(8),
                               ctypes.c_void_p(8), 16, 4, 16, 11.0,
                               (ctypes.c_float * 9)(), 9, 1, 0)  # fmt: skip
    assert rc != 0 and "n_windows" in _lib.last_error()
    seg_len, n_segs = ctypes.c_int(), ctypes.c_int()
    rc = lib.ksp_background_median_filter_geometry(4096, 64, 33, 0, ctypes.byref(seg_len),
                                                   ctypes.byref(n_segs))  # fmt: skip
    assert rc != 0 and "width 33" in _lib.last_error()


def test_fused_ring_mode_and_path_names(lib):
    """_lib.fused_ring_mode sets the calling thread's mode for its block and restores the one
    before, in order when nested and when the block raises; the path names are the header's."""
    from katsdpsigproc_amd import _lib

    def mode():
        return lib.ksp_flagger_fused_ring_mode(7)  # (7: query only)

    start = mode()
    with _lib.fused_ring_mode(1):
        assert mode() == 1
        with _lib.fused_ring_mode(-1):
            assert mode() == -1
            with _lib.fused_ring_mode(0):
                assert mode() == 0
            assert mode() == -1
        assert mode() == 1
        with pytest.raises(ZeroDivisionError):
            with _lib.fused_ring_mode(-1):
                assert mode() == -1
                1 / 0
        assert mode() == 1
    assert mode() == start
    defines = dict(re.findall(r"^#define (KSP_FUSED_PATH_\w+) (\d+)$", open(HEADER).read(), re.M))
    names = ("FUSED_PATH_STRIP", "FUSED_PATH_LONG", "FUSED_PATH_RING")
    assert defines == {"KSP_" + name: str(getattr(_lib, name)) for name in names}
    assert [getattr(_lib, name) for name in names] == [1, 2, 4]
