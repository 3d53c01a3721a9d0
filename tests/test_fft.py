"""FFT operations over hipFFT against numpy.fft (reference test/test_fft.py)."""

import numpy as np
import pytest

from katsdpsigproc_amd import accel


def test_argument_checks_need_no_gpu():
    from katsdpsigproc_amd import fft

    with pytest.raises(TypeError):  # not a HIP context
        fft.FftTemplate(object(), 1, (8,), np.complex64, np.complex64, (8,), (8,))
    assert fft.FftMode.FORWARD.value == 0 and fft.FftMode.INVERSE.value == 1


@pytest.fixture(scope="module")
def context():
    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


@pytest.mark.gpu
class TestFft:
    def _run(self, context, command_queue, template, mode, src):
        from katsdpsigproc_amd import fft

        fn = template.instantiate(command_queue, mode)
        fn.ensure_all_bound()
        fn.buffer("src").set(command_queue, src)
        fn()
        assert ("work_area" in fn.slots) == (template._work_size > 0)
        return fn.buffer("dest").get(command_queue)

    @pytest.mark.parametrize("precision", [np.complex64, np.complex128])
    def test_complex_2d_batched_with_padding(self, precision, context, command_queue):
        from katsdpsigproc_amd import fft

        shape, padded_src, padded_dest = (3, 2, 48, 64), (3, 2, 50, 72), (3, 2, 48, 80)
        rs = np.random.RandomState(1)
        src = (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(precision)
        template = fft.FftTemplate(context, 2, shape, precision, precision, padded_src, padded_dest)
        tol = 1e-4 if precision == np.complex64 else 1e-11
        out = self._run(context, command_queue, template, fft.FftMode.FORWARD, src)
        np.testing.assert_allclose(out, np.fft.fftn(src, axes=(2, 3)), rtol=tol, atol=tol * 50)
        out = self._run(context, command_queue, template, fft.FftMode.INVERSE, src)
        expected = np.fft.ifftn(src, axes=(2, 3)) * (48 * 64)  # unnormalised
        np.testing.assert_allclose(out, expected, rtol=tol, atol=tol * 50)

    def test_real_transforms(self, context, command_queue):
        from katsdpsigproc_amd import fft

        shape = (5, 30, 40)
        rs = np.random.RandomState(2)
        real = rs.standard_normal(shape).astype(np.float32)
        r2c = fft.FftTemplate(context, 2, shape, np.float32, np.complex64, (5, 30, 48), (5, 30, 24))
        spectrum = self._run(context, command_queue, r2c, fft.FftMode.FORWARD, real)
        assert spectrum.shape == (5, 30, 21)
        np.testing.assert_allclose(spectrum, np.fft.rfftn(real, axes=(1, 2)), rtol=1e-4, atol=5e-3)
        c2r = fft.FftTemplate(context, 2, shape, np.complex64, np.float32, (5, 30, 21), (5, 30, 40))
        back = self._run(context, command_queue, c2r, fft.FftMode.INVERSE, spectrum)
        np.testing.assert_allclose(back, real * (30 * 40), rtol=1e-4, atol=5e-2)
        with pytest.raises(ValueError):
            r2c.instantiate(command_queue, fft.FftMode.INVERSE)
        with pytest.raises(ValueError):
            c2r.instantiate(command_queue, fft.FftMode.FORWARD)

    def test_bad_shapes(self, context):
        from katsdpsigproc_amd import fft

        with pytest.raises(ValueError):  # batch dimension padded
            fft.FftTemplate(context, 1, (4, 16), np.complex64, np.complex64, (5, 16), (4, 16))
        with pytest.raises(ValueError):
            fft.FftTemplate(context, 1, (4, 16), np.complex64, np.complex64, (4, 16), (16,))
        with pytest.raises(ValueError):
            fft.FftTemplate(context, 1, (4, 16), np.float32, np.float32, (4, 16), (4, 16))


# --------------------------------------------------------------------------------------
# Every rank, odd and prime lengths, both precisions, with guarded padding. The oracle is
# numpy.fft on the input widened to double precision; the tolerance is the reference's
# (test/test_fft.py): atol = resolution of the precision * max|expected|, rtol = 0.
SENTINEL = -7777.0  # in the destination's padding before a transform, and expected after


def _window(shape):
    return tuple(slice(0, n) for n in shape)


def _transform(command_queue, template, mode, src_host, check_src=True):
    """Run `template` on `src_host`. The source's padding holds NaN (which would spread
    through a result if it were read), the destination holds the sentinel everywhere. Checks
    that the destination's padding comes back bit for bit, and the whole source too unless
    the library may use it as scratch. Returns the unpadded result."""
    fn = template.instantiate(command_queue, mode)
    fn.ensure_all_bound()
    assert ("work_area" in fn.slots) == (template._work_size > 0)
    src, dest = fn.buffer("src"), fn.buffer("dest")
    assert src.padded_shape == template.padded_shape_src and src.shape == src_host.shape
    assert dest.padded_shape == template.padded_shape_dest
    src_padded = np.full(src.padded_shape, np.nan, src.dtype)
    src_padded[_window(src.shape)] = src_host
    before = np.full(dest.padded_shape, SENTINEL, dest.dtype)
    command_queue.enqueue_write_buffer(src.buffer, src_padded)
    command_queue.enqueue_write_buffer(dest.buffer, before)
    fn()
    after = np.empty_like(before)
    command_queue.enqueue_read_buffer(dest.buffer, after)
    padding = np.ones(dest.padded_shape, bool)
    padding[_window(dest.shape)] = False
    assert padding.sum() == before.size - np.prod(dest.shape)
    unsigned = np.uint32 if dest.dtype == np.float32 else np.uint64  # compare bits
    np.testing.assert_array_equal(after[padding].view(unsigned), before[padding].view(unsigned),
                                  err_msg="the transform wrote into the destination's padding")  # fmt: skip
    if check_src:
        src_after = np.empty_like(src_padded)
        command_queue.enqueue_read_buffer(src.buffer, src_after)
        assert src_after.tobytes() == src_padded.tobytes(), "the transform changed its source"
    return after[_window(dest.shape)].copy()


def _check(got, expected, dtype):
    """The reference's tolerance; the figure printed is the error in units of it."""
    assert got.shape == expected.shape
    scale = np.max(np.abs(expected))
    tol = np.finfo(dtype).resolution * scale
    error = np.max(np.abs(got.astype(expected.dtype) - expected))
    print(f"max error {error / scale:.3e} of max|expected|, {error / tol:.3f} of the tolerance")
    np.testing.assert_allclose(got, expected, rtol=0, atol=tol)


def _complex_normal(rs, shape, dtype):
    return (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(dtype)


# N, shape, padded source, padded destination
COMPLEX_CASES = [
    (2, (7, 16, 48), (7, 16, 48), (7, 18, 51)),  # the reference's
    (1, (5, 3, 97), (5, 3, 101), (5, 3, 97)),  # a prime length
    (3, (2, 6, 10, 12), (2, 7, 11, 16), (2, 6, 12, 13)),
    (2, (16, 48), (16, 48), (18, 51)),  # no batch dimension
]
# shape, padded real side, padded complex side (the reference's)
REAL_CASES = [
    ((3, 2, 16, 48), (3, 2, 24, 64), (3, 2, 20, 27)),
    ((3, 2, 15, 47), (3, 2, 23, 63), (3, 2, 17, 24)),  # odd: 47 // 2 + 1 == 48 // 2
]
_IDS = dict(ids=lambda value: "x".join(map(str, value)) if isinstance(value, tuple) else None)


@pytest.mark.gpu
class TestFftShapes:
    @pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
    @pytest.mark.parametrize("dtype", [np.complex64, np.complex128], ids=["c2c", "z2z"])
    @pytest.mark.parametrize("N, shape, padded_src, padded_dest", COMPLEX_CASES, **_IDS)
    def test_complex(self, N, shape, padded_src, padded_dest, dtype, inverse, context,
                     command_queue):  # fmt: skip
        from katsdpsigproc_amd import fft

        src = _complex_normal(np.random.RandomState(1), shape, dtype)
        template = fft.FftTemplate(context, N, shape, dtype, dtype, padded_src, padded_dest)
        axes = tuple(range(-N, 0))
        wide = src.astype(np.complex128)
        if inverse:
            expected = np.fft.ifftn(wide, axes=axes) * np.prod(shape[-N:])  # unnormalised
        else:
            expected = np.fft.fftn(wide, axes=axes)
        mode = fft.FftMode.INVERSE if inverse else fft.FftMode.FORWARD
        _check(_transform(command_queue, template, mode, src), expected, dtype)

    @pytest.mark.parametrize("real, cplx", [(np.float32, np.complex64), (np.float64, np.complex128)],
                             ids=["r2c", "d2z"])  # fmt: skip
    @pytest.mark.parametrize("shape, padded_real, padded_complex", REAL_CASES, **_IDS)
    def test_real_to_complex(self, shape, padded_real, padded_complex, real, cplx, context,
                             command_queue):  # fmt: skip
        from katsdpsigproc_amd import fft

        src = np.random.RandomState(1).standard_normal(shape).astype(real)
        template = fft.FftTemplate(context, 2, shape, real, cplx, padded_real, padded_complex)
        expected = np.fft.rfftn(src.astype(np.float64), axes=(-2, -1))
        assert expected.shape == shape[:-1] + (shape[-1] // 2 + 1,)
        _check(_transform(command_queue, template, fft.FftMode.FORWARD, src), expected, real)

    @pytest.mark.parametrize("real, cplx", [(np.float32, np.complex64), (np.float64, np.complex128)],
                             ids=["c2r", "z2d"])  # fmt: skip
    @pytest.mark.parametrize("shape, padded_real, padded_complex", REAL_CASES, **_IDS)
    def test_complex_to_real(self, shape, padded_real, padded_complex, real, cplx, context,
                             command_queue):  # fmt: skip
        """The source is the spectrum of a real signal, rounded to the precision; the last
        length of the real side (47 as much as 46 would fit 24 complex elements) is the
        template's. The library may overwrite the source of this transform, so it is not
        looked at afterwards."""
        from katsdpsigproc_amd import fft

        signal = np.random.RandomState(1).standard_normal(shape) + 3
        src = np.fft.rfftn(signal, axes=(-2, -1)).astype(cplx)
        template = fft.FftTemplate(context, 2, shape, cplx, real, padded_complex, padded_real)
        expected = np.fft.irfftn(src.astype(np.complex128), s=shape[-2:], axes=(-2, -1))
        expected *= shape[-2] * shape[-1]  # unnormalised
        got = _transform(command_queue, template, fft.FftMode.INVERSE, src, check_src=False)
        _check(got, expected, cplx)

    def test_one_template_two_queues(self, context, command_queue):
        """The plan belongs to the template and its stream is set per call: operations on
        two queues, called alternately on different data, each get their own answer."""
        from katsdpsigproc_amd import fft

        shape, padded_dest = (7, 16, 48), (7, 18, 51)
        template = fft.FftTemplate(context, 2, shape, np.complex64, np.complex64, shape, padded_dest)
        queues = [command_queue, context.create_command_queue()]
        fns = [template.instantiate(queue, fft.FftMode.FORWARD) for queue in queues]
        for fn in fns:
            fn.ensure_all_bound()
        rs = np.random.RandomState(5)
        for _ in range(3):
            inputs = [_complex_normal(rs, shape, np.complex64) for _ in fns]
            for fn, queue, data in zip(fns, queues, inputs):
                fn.buffer("src").set_async(queue, data)
            for fn in fns + fns:
                fn()
            for fn, queue, data in zip(fns, queues, inputs):
                expected = np.fft.fftn(data.astype(np.complex128), axes=(-2, -1))
                _check(np.array(fn.buffer("dest").get(queue)), expected, np.complex64)
