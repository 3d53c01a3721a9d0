"""masked_gaussian_filter without a GPU: the NumPy restatement against the reference's
results, the public interface, argument checks of the Python layer and of the C ABI, slot
wiring."""

import ctypes
import inspect
import json
import os

import numpy as np
import pytest

from tests import inputs_masked_filter as inputs
from tests import masked_filter_oracle as oracle
from tests.fakes import FakeContext


@pytest.fixture(scope="module")
def golden():
    with np.load(inputs.GOLDEN) as g:
        return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def lib():
    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    return _lib.load()


def test_golden_cases_match_inputs(golden):
    cases = json.loads(str(golden["cases"]))
    assert cases == json.loads(json.dumps(inputs.case_list(), sort_keys=True))
    for case in cases:
        assert golden[case["name"]].shape == tuple(case["shape"])
        assert golden[case["name"]].dtype == np.dtype(case["dtype"])
    # the cases cover both types and every number of passes the GPU tests name
    assert {c["dtype"] for c in cases} == {"float32", "float64"}
    assert {c["passes"] for c in cases} >= {1, 2, 3, 4, 5, 8}
    assert os.path.getsize(inputs.GOLDEN) < 500_000


@pytest.mark.parametrize("name", sorted(inputs.CASES))
def test_restatement_reproduces_reference(golden, name):
    _shape, _dtype, sigma, passes = inputs.CASES[name][:4]
    data, flags = inputs.make_case(name)
    out = oracle.masked_filter(data, flags, sigma, passes)
    expected = golden[name]
    assert out.dtype == expected.dtype
    assert np.array_equal(np.isnan(out), np.isnan(expected))
    assert np.array_equal(out, expected, equal_nan=True)


def test_golden_nan_case_is_not_vacuous(golden):
    nan = np.isnan(golden["block"]).mean()
    assert nan > 0.01 and 1 - nan > 0.5
    copy = golden["copy"]
    data, flags = inputs.make_case("copy")
    assert np.array_equal(np.isnan(copy), flags)
    assert np.array_equal(copy[~flags], data[~flags])


def test_divisor_is_numbas_power():
    # float32 pow gives 22667122 for 69 ** 4; squaring in float32 gives 22667120
    from katsdpsigproc_amd.rfi import twodflag

    assert twodflag._filter_divisor(34, 4, np.float32) == 22667120.0
    assert twodflag._filter_divisor(34, 4, np.float64) == 69.0**4
    for dtype in (np.float32, np.float64):
        for r in (0, 1, 7, 34, 600, 2047):
            for passes in range(1, 9):
                assert twodflag._filter_divisor(r, passes, dtype) == float(
                    oracle.divisor(r, passes, dtype))  # fmt: skip
    assert twodflag._filter_radius(40.0, 4) == 34 == inputs.radius(40.0, 4)
    assert twodflag._filter_radius(0.28, 4) == 0 and twodflag._filter_radius(2.3, 4) == 2


def test_public_name_and_signature():
    """The reference's second public name, with its parameter names and default."""
    from katsdpsigproc_amd.rfi.twodflag import masked_gaussian_filter

    params = inspect.signature(masked_gaussian_filter).parameters
    assert list(params)[:5] == ["data", "flags", "sigma", "out", "passes"]
    assert params["passes"].default == 4
    for name in ("data", "flags", "sigma", "out"):
        assert params[name].default is inspect.Parameter.empty
    assert params["context"].kind is inspect.Parameter.KEYWORD_ONLY


def test_host_function_argument_errors():
    """Every check below is made before a device is looked for."""
    from katsdpsigproc_amd.rfi.twodflag import masked_gaussian_filter as mgf

    data = np.zeros((6, 5), np.float32)
    flags = np.zeros((6, 5), np.bool_)
    out = np.zeros((6, 5), np.float32)
    with pytest.raises(TypeError, match="float16"):
        mgf(data.astype(np.float16), flags, (1, 1), out)
    with pytest.raises(TypeError, match="complex64"):
        mgf(data.astype(np.complex64), flags, (1, 1), out)
    with pytest.raises(TypeError, match="float64"):
        mgf(data, flags, (1, 1), out.astype(np.float64))
    with pytest.raises(TypeError, match="float32"):
        mgf(data, flags.astype(np.float32), (1, 1), out)
    with pytest.raises(ValueError, match="shape mismatch between data and flags"):
        mgf(data, flags[:5], (1, 1), out)
    with pytest.raises(ValueError, match="shape mismatch between data and out"):
        mgf(data, flags, (1, 1), out[:, :4])
    with pytest.raises(ValueError, match="dimensions"):
        mgf(data[0], flags[0], (1, 1), out[0])
    for sigma in ((1, 1, 1), (), np.ones((2, 2))):
        with pytest.raises(ValueError, match="sigma"):
            mgf(data, flags, sigma, out)
    for passes in (0, -1, 9):
        with pytest.raises(ValueError, match=r"passes must be in 1\.\.8"):
            mgf(data, flags, (1, 1), out, passes)
    with pytest.raises(TypeError, match="passes"):
        mgf(data, flags, (1, 1), out, 2.5)
    with pytest.raises(ValueError, match=r"radius outside 0\.\.2047"):
        mgf(data, flags, (1, 5000.0), out)
    with pytest.raises(ValueError, match="finite"):
        mgf(data, flags, (1, np.inf), out)
    with pytest.raises(ValueError, match="passes = 1"):
        mgf(data, flags, (0, 4.0), out, passes=1)  # radius 6 on an axis of 5


def test_operation_argument_errors():
    from katsdpsigproc_amd.rfi import twodflag

    context = FakeContext()
    queue = context.create_command_queue()
    with pytest.raises(TypeError, match="int32"):
        twodflag.MaskedGaussianFilterTemplate(context, np.int32)
    with pytest.raises(ValueError, match="passes"):
        twodflag.MaskedGaussianFilterTemplate(context, np.float32, passes=0)
    template = twodflag.MaskedGaussianFilterTemplate(context)
    assert template.passes == 4 and template.dtype == np.float32
    for shape in ((0, 5), (5, 0), (65537, 4), (4, 65537), (2, 0, 4)):
        with pytest.raises(ValueError, match=r"1\.\.65536"):
            template.instantiate(queue, shape, (1, 1))
    with pytest.raises(ValueError, match="images"):
        template.instantiate(queue, (0, 4, 4), (1, 1))
    with pytest.raises(ValueError, match="shape"):
        template.instantiate(queue, (4,), (1, 1))
    with pytest.raises(ValueError, match="sigma"):
        template.instantiate(queue, (4, 4), (1, 1, 1))
    with pytest.raises(ValueError, match="2047"):
        template.instantiate(queue, (4, 4), (2400.0, 1))
    assert template.instantiate(queue, (4, 4), (2364.0, 1)).radii == (2047, 1)


def test_slots_parameters_and_batches(lib):
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import twodflag

    context = FakeContext()
    queue = context.create_command_queue()
    template = twodflag.MaskedGaussianFilterTemplate(context, np.float64, passes=3)
    op = template.instantiate(queue, (5, 40, 70), (5.0, 2.3), batch=2)
    assert set(op.slots) == {"data", "flags", "out"}
    assert op.slots["data"].dtype == op.slots["out"].dtype == np.float64
    assert op.slots["flags"].dtype == np.uint8
    for slot in op.slots.values():
        assert slot.shape == (5, 40, 70)
    assert op.parameters() == {"shape": (5, 40, 70), "dtype": "float64", "passes": 3,
                               "sigma": (5.0, 2.3), "radii": (5, 2), "batch": 2}  # fmt: skip
    size = ctypes.c_size_t()
    assert lib.ksp_masked_filter_workspace(40, 70, 2, 5, 2, 3, 8, ctypes.byref(size)) == 0
    assert op.workspace_bytes == size.value and op.workspace.shape == (size.value,)
    # padded on both axes, through the shared dimensions
    op.slots["flags"].dimensions[1].link(accel.Dimension(40, min_padded_size=48))
    op.slots["out"].dimensions[2].link(accel.Dimension(70, min_padded_size=96))
    op.ensure_all_bound()
    for name in op.slots:
        assert op.buffer(name).padded_shape == (5, 48, 96)
    op()
    assert [name for name, _ in queue.launches] == ["ksp_masked_filter"] * 3
    for k, (_, args) in enumerate(queue.launches):
        assert [int(a) for a in args[3:10]] == [40, 70, 5, 48 * 96, 96, 2 * k, 2 if k < 2 else 1]
        assert [int(a) for a in args[10:13]] == [5, 2, 3]
        assert args[13:15] == [11.0**3, 5.0**3] and args[15] == 8
        assert int(args[17]) == size.value
    # a 2-D shape is one image; the default batch fits the workspace budget
    op2 = twodflag.MaskedGaussianFilterTemplate(context).instantiate(queue, (77, 53), (5.0, 2.3))
    assert (op2.images, op2.rows, op2.cols, op2.batch) == (1, 77, 53, 1)


def test_default_batch_fits_the_workspace_budget(lib, monkeypatch):
    from katsdpsigproc_amd.rfi import twodflag

    monkeypatch.setattr(twodflag, "DEFAULT_WORKSPACE_BYTES", 1 << 20)
    queue = FakeContext().create_command_queue()
    template = twodflag.MaskedGaussianFilterTemplate(queue.context)
    many = template.instantiate(queue, (1000, 40, 70), (5.0, 2.3))
    assert 1 < many.batch < 1000 and many.workspace_bytes <= 1 << 20
    size = ctypes.c_size_t()
    assert lib.ksp_masked_filter_workspace(40, 70, many.batch + 1, 5, 2, 4, 4, ctypes.byref(size)) == 0
    assert size.value > 1 << 20
    # at least one image per batch, however large
    big = template.instantiate(queue, (3, 512, 512), (5.0, 2.3))
    assert big.batch == 1 and big.workspace_bytes > 1 << 20


def test_launchers_check_arguments_without_gpu(lib):
    """Both C-ABI functions refuse bad arguments before any device call."""
    from katsdpsigproc_amd import _lib

    size = ctypes.c_size_t()
    ws = lib.ksp_masked_filter_workspace
    assert ws(40, 70, 2, 5, 2, 4, 4, ctypes.byref(size)) == 0
    # W and O, and the padded lines of the axis that needs more of them
    lines = max(2 * 2 * 70 * (40 + 5 * 4), 2 * 2 * 40 * (70 + 2 * 4))
    assert size.value >= (2 * 2 * 40 * 70 + lines) * 4
    assert size.value < (2 * 2 * 40 * 70 + lines) * 4 + 1024
    assert ws(40, 70, 2, 5, 2, 4, 4, None) != 0 and "NULL" in _lib.last_error()
    for args, word in [((0, 70, 2, 5, 2, 4, 4), "rows"), ((65537, 70, 2, 5, 2, 4, 4), "rows"),
                       ((40, 0, 2, 5, 2, 4, 4), "cols"), ((40, 65537, 2, 5, 2, 4, 4), "cols"),
                       ((40, 70, 0, 5, 2, 4, 4), "batch"), ((40, 70, 2, 5, 2, 0, 4), "passes"),
                       ((40, 70, 2, 5, 2, 9, 4), "passes"), ((40, 70, 2, -1, 2, 4, 4), "radius"),
                       ((40, 70, 2, 2048, 2, 4, 4), "radius"), ((40, 70, 2, 5, 2048, 4, 4), "radius"),
                       ((40, 70, 2, 41, 2, 1, 4), "passes = 1"), ((40, 70, 2, 5, 71, 1, 4), "passes = 1"),
                       ((40, 70, 2, 5, 2, 4, 2), "itemsize"), ((40, 70, 2, 5, 2, 4, 16), "itemsize")]:  # fmt: skip
        assert ws(*args, ctypes.byref(size)) != 0 and word in _lib.last_error(), args
    assert ws(40, 70, 2, 40, 70, 1, 8, ctypes.byref(size)) == 0  # radius = length is allowed
    assert ws(40, 70, 2, 5, 2, 4, 4, ctypes.byref(size)) == 0

    v = ctypes.c_void_p(8)
    run = lib.ksp_masked_filter

    def call(data=v, flags=v, out=v, rows=40, cols=70, images=5, si=40 * 70, sr=70, image0=0,
             batch=2, r0=5, r1=2, passes=4, d0=14641.0, d1=625.0, itemsize=4, workspace=v,
             workspace_bytes=None):  # fmt: skip
        if workspace_bytes is None:
            workspace_bytes = size.value
        return run(0, None, data, flags, out, rows, cols, images, si, sr, image0, batch, r0, r1,
                   passes, d0, d1, itemsize, workspace, workspace_bytes)  # fmt: skip

    for kw, word in [({"data": None}, "NULL"), ({"flags": None}, "NULL"), ({"out": None}, "NULL"),
                     ({"workspace": None}, "NULL"), ({"rows": 0}, "rows"), ({"cols": 70000}, "cols"),
                     ({"passes": 0}, "passes"), ({"passes": 9}, "passes"), ({"r0": 2048}, "radius"),
                     ({"r1": -1}, "radius"), ({"itemsize": 2}, "itemsize"),
                     ({"batch": 0}, "batch"), ({"image0": 4}, "image0"), ({"image0": -1}, "image0"),
                     ({"images": 0}, "image0"), ({"sr": 69}, "strides"), ({"si": 40 * 70 - 1}, "strides"),
                     ({"d0": 0.0}, "divisor"), ({"d1": float("nan")}, "divisor"),
                     ({"workspace_bytes": size.value - 1}, "workspace too small"),
                     ({"itemsize": 8}, "workspace too small"),
                     ({"batch": 3}, "workspace too small")]:  # fmt: skip
        assert call(**kw) != 0 and word in _lib.last_error(), kw
