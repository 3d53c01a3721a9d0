"""The layout arithmetic of tests/farviews.py, without a GPU: aliases against hand-worked
cases, the three conditions of a layout, the host side of the whole-allocation audit."""

import numpy as np
import pytest

from tests import farviews
from tests.farviews import GUARD, FarLayout, LayoutError, aliases, far_stride, low32
from tests.subviews import SENTINEL, sentinel_array

G2, G4 = 2**31, 2**32


def test_low32():
    assert low32(5) == (5, 5)
    assert low32(G2 - 1) == (G2 - 1, G2 - 1)
    assert low32(G2) == (G2, -G2)
    assert low32(G4 - 4) == (G4 - 4, -4)
    assert low32(G4) == (0, 0)
    assert low32(G4 + 12) == (12, 12)
    assert low32(3 * G4 + G2 + 8) == (G2 + 8, -G2 + 8)


@pytest.mark.parametrize("row, stride, itemsize, want", [
    # offsets below 2**31 in bytes and in elements: nothing to truncate
    (1, G2 - 16, 1, []),
    (1, 2**27 - 2, 16, []),
    (3, 100, 8, []),
    # just above 2**31 bytes: the unsigned reading is the true offset, the signed one negative
    (1, G2 // 4 + 4, 4, [-G2 + 16]),
    (2, G2 // 16 + 1, 8, [-G2 + 16]),
    # 1-byte items: bytes and elements coincide, one alias each way
    (2, G2 - 16, 1, [-32]),
    (3, G2 - 16, 1, [G2 - 48]),  # 2**32 + 2**31 - 48 loses its 2**32
    (6, 2**30 + 4, 1, [-G2 + 24, G2 + 24]),  # 2**32 + 2**31 + 24 does too, and goes negative
    # a byte stride of 2**32 plus a remainder: every byte alias is the small remainder
    (1, G4 // 8 + 24, 8, [192]),
    (2, G4 // 8 + 24, 8, [384]),
    (1, G4 // 16 + 3, 16, [48]),
    (2, G4 // 4 + 5, 4, [-2 * G4 + 40, 40]),  # element offset 2**31 + 10: signed, times 4
    (4, G4 // 4 + 5, 4, [80]),  # element offset 2**32 + 20 wraps to 20
    # just above 2**32 bytes with 4-byte items: the element offset is far below 2**31
    (4, G4 // 16 + 4, 4, [64]),
])  # fmt: skip
def test_aliases(row, stride, itemsize, want):
    assert aliases(row, stride, itemsize) == sorted(want)
    true = row * stride * itemsize
    assert true not in aliases(row, stride, itemsize)


def conditions(layout):
    """The three conditions, worked out again from the layout's own lists."""
    rows = [(layout.start + o, layout.start + o + layout.row_bytes) for o in layout.true]
    for r, o in enumerate(layout.true):
        for a in aliases(r, layout.stride, layout.itemsize):
            lo, hi = layout.start + a - GUARD, layout.start + a + layout.row_bytes + GUARD
            assert 0 <= lo and hi <= layout.size  # inside the allocation
            assert any(s_lo <= lo and hi <= s_hi for s_lo, s_hi in layout.segments)
            for row_lo, row_hi in rows:  # not on a true row, nor on its guard bands
                assert hi <= row_lo - GUARD or lo >= row_hi + GUARD
    for (_, hi), (lo, _) in zip(rows, rows[1:]):
        assert lo - hi >= 2 * GUARD
    assert rows[0][0] >= GUARD and rows[-1][1] + GUARD <= layout.size
    for (_, hi), (lo, _) in zip(layout.segments, layout.segments[1:]):
        assert hi < lo  # disjoint, so that the audit counts no byte twice


@pytest.mark.parametrize("rows, cols, dtype, like", [
    (2, 100, np.complex64, 112), (3, 100, np.complex64, 113), (3, 100, np.float32, 113),
    (5, 5, np.float32, 8), (37, 100, np.complex64, 113), (67, 129, np.uint16, 145),
    (129, 67, np.complex128, 96), (4096, 12, np.uint8, 17), (4096, 12, np.complex64, 14),
    (2, 100, np.uint8, 112), (3, 100, np.uint8, 113), (4, 100, np.uint8, 113),
    (8193, 6, np.float32, 9),
])  # fmt: skip
def test_far_stride(rows, cols, dtype, like):
    itemsize = np.dtype(dtype).itemsize
    stride = far_stride(rows, cols, dtype, like)
    assert stride % 16 == like % 16 and cols <= stride <= farviews.MAX_STRIDE
    layout = FarLayout((rows, cols), dtype, stride)
    conditions(layout)
    assert layout.size <= 9 * 2**30
    last = (rows - 1) * stride * itemsize
    if rows >= 4 or itemsize >= 4 and rows >= 2:
        assert last > G4  # the last row lies beyond 2**32 bytes
        assert any(G2 <= o for o in layout.true)
    else:  # as far as an int stride takes so few rows of so small elements
        assert stride > farviews.MAX_STRIDE - 2**16
    if itemsize == 1 and rows >= 3:
        assert (rows - 1) * stride >= G2  # element offsets of 2**31 and more
    # a front margin only where a signed alias asks for one
    if not any(a < 0 for a in layout.alias):
        assert layout.start == GUARD


def test_offset_and_alignment():
    for offset in (0, 1, 12):
        layout = FarLayout((3, 10), np.complex64, G4 // 8 + 128, offset)
        assert layout.start == GUARD + 8 * offset
        conditions(layout)
        for lo, hi in layout.segments:
            assert (lo - layout.start) % 8 == 0 and (hi - lo) % 8 == 0


@pytest.mark.parametrize("shape, dtype, stride, why", [
    # row 1's signed byte alias, -64, falls on row 0
    ((2, 100), np.float32, G4 // 4 - 16, "overlaps row 0"),
    # 2**32 / 3: row 3 wraps to offset 0, onto row 0 itself
    ((4, 16), np.uint8, 1431655766, "overlaps row 0"),
    # a byte stride of 2**32 + 64: row 1's alias lies in the guard band behind row 0
    ((2, 3), np.float32, G4 // 4 + 16, "overlaps row 0"),
    # a byte stride of 2**31: row 2 wraps onto row 0, row 3 onto row 1
    ((4, 4), np.complex64, 2**28, "overlaps row"),
    ((3, 100), np.float32, 50, "stride 50"),  # narrower than the rows
    ((2, 4), np.uint8, 2**31, "stride"),  # no int
    ((3, 100), np.float32, 200, "guard bands"),  # compact: rows closer than their guards
])  # fmt: skip
def test_rejected(shape, dtype, stride, why):
    with pytest.raises(LayoutError, match=why):
        FarLayout(shape, dtype, stride)


def test_image_and_check():
    rs = np.random.RandomState(1)
    data = rs.standard_normal((3, 10)).astype(np.float32)
    layout = FarLayout(data.shape, np.float32, far_stride(3, 10, np.float32, 17), offset=1)
    assert len(layout.alias) > 0
    # an input: poison everywhere but in the rows, alias windows included
    before = layout.image(data, poison=True)
    assert [c.size for c in before] == [hi - lo for lo, hi in layout.segments]
    np.testing.assert_array_equal(layout.rows_of(before), data)
    for chunk, outside in zip(before, layout.outside()):
        assert np.isnan(chunk.view(np.float32)[outside[::4]]).all()
    after = [c.copy() for c in before]
    np.testing.assert_array_equal(farviews.check_segments(layout, before, after, True), data)
    after[-1][3] ^= 1
    with pytest.raises(AssertionError, match="an input was written to"):
        farviews.check_segments(layout, before, after, True)
    # an output: sentinels; writing the rows is fine, a guard band or an alias window is not
    blank = sentinel_array(data.shape, np.float32)
    before = layout.image(blank, poison=False)
    assert all((c == SENTINEL).all() for c in before)
    after = layout.image(data, poison=False)
    np.testing.assert_array_equal(farviews.check_segments(layout, before, after, False), data)
    k, where = layout.row_slices()[1]
    for at in (where.start - 1, where.stop):  # the bytes next to row 1, on either side
        bad = [c.copy() for c in after]
        bad[k][at] = 0
        with pytest.raises(AssertionError, match="outside the rows"):
            farviews.check_segments(layout, before, bad, False)
    alias_only = [i for i, m in enumerate(layout.outside()) if m.all()]
    assert alias_only  # segments that hold alias windows alone
    bad = [c.copy() for c in after]
    bad[alias_only[0]][GUARD] = 0
    with pytest.raises(AssertionError, match="outside the rows"):
        farviews.check_segments(layout, before, bad, False)


def test_expected_count():
    data = np.arange(1, 31, dtype=np.uint8).reshape(3, 10)
    data[1, 4] = SENTINEL  # a result byte that happens to be the sentinel is not counted
    layout = FarLayout(data.shape, np.uint8, far_stride(3, 10, np.uint8, 16))
    assert farviews.expected_count(layout.image(data, poison=False)) == 29
    # an input in poison: every byte of every window but the sentinel-valued one
    chunks = layout.image(data, poison=True)
    assert farviews.expected_count(chunks) == sum(c.size for c in chunks) - 1
    # float32 NaN poison has no sentinel byte either
    chunks = FarLayout((2, 3), np.float32, G4 // 4 + 256).image(np.ones((2, 3), np.float32), True)
    assert farviews.expected_count(chunks) == sum(c.size for c in chunks)
    # what the device would count: a whole allocation of sentinels with the segments laid in
    small = FarLayout((2, 8), np.uint8, 2048)
    chunks = small.image(np.zeros((2, 8), np.uint8), poison=False)
    whole = np.full(small.size, SENTINEL, np.uint8)
    for (lo, hi), chunk in zip(small.segments, chunks):
        whole[lo:hi] = chunk
    assert np.count_nonzero(whole != SENTINEL) == farviews.expected_count(chunks) == 16


class NoArena:
    """Stands in for the device arena where only the choice of strides is tested."""

    used = 0

    def reset(self):
        self.used = 0


@pytest.mark.parametrize("rows, cols, like", [(3, 5, 16), (3, 1027, 1041), (5, 257, 272),
                                              (65, 2100, 2113), (2100, 65, 80)])  # fmt: skip
@pytest.mark.parametrize("far", [("deviations",), ("flags",), ("deviations", "flags")])
def test_shared_stride(rows, cols, like, far):
    """One stride for float32 deviations and uint8 flags: the far role's type decides (the
    narrower one if both are), the layouts of both types accept it, and together they stay
    within what one arena of 31 GiB holds."""
    views = farviews.FarViews(NoArena(), far, None)
    arrays = [("deviations", rows, cols, np.float32), ("flags", rows, cols, np.uint8)]
    stride = views.shared_stride(like, arrays)
    assert stride % 16 == like % 16 and stride <= farviews.MAX_STRIDE
    layouts = [FarLayout((rows, cols), dtype, stride) for _, _, _, dtype in arrays]
    for layout in layouts:
        conditions(layout)
    assert sum(layout.size for layout in layouts) <= 31 * 2**30
    decides = np.uint8 if "flags" in far else np.float32
    assert (rows - 1) * stride * np.dtype(decides).itemsize > G4 - 2**12 * rows
    assert farviews.FarViews(NoArena(), (), None).shared_stride(like, arrays) == like


@pytest.mark.parametrize("rows, cols", [(3, 1920), (120, 48), (32, 192), (3072, 2)])
def test_long_strides_and_spans(rows, cols):
    """Launchers with ``long long`` strides: three rows of bytes may cross 2**32, which no int
    stride allows; and a span of a little over 2**31 for views that cannot afford 2**32."""
    stride = far_stride(rows, cols, np.uint8, cols + 5, max_stride=farviews.LONG_STRIDE)
    assert (rows - 1) * stride > G4 and stride % 16 == (cols + 5) % 16
    if rows == 3:
        assert stride > farviews.MAX_STRIDE
        with pytest.raises(LayoutError, match="stride"):
            FarLayout((rows, cols), np.uint8, stride)
    conditions(FarLayout((rows, cols), np.uint8, stride, 0, farviews.LONG_STRIDE))
    views = farviews.FarViews(NoArena(), {"flags"}, None, G2 + 2**24, farviews.LONG_STRIDE)
    arrays = [("data", rows, cols, np.float32), ("flags", rows, cols, np.uint8)]
    stride = views.shared_stride(cols + 5, arrays)
    assert G2 < (rows - 1) * stride < G2 + 2**25
    layouts = [FarLayout((rows, cols), dtype, stride, 0, farviews.LONG_STRIDE) for *_, dtype in arrays]
    for layout in layouts:
        conditions(layout)
    assert layouts[0].true[-1] > 2 * G4 and min(layouts[0].alias) < -G4  # element offsets beyond 2**31
