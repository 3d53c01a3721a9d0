"""Region-transfer cases for ``DeviceArray.copy_region`` / ``set_region`` / ``get_region``,
shared by tests/test_transfers.py (fake backend) and tests/test_gpu_transfers.py (device).

The definition of a region copy is NumPy indexing on host arrays::

    expected = <dest's previous padded contents>
    expected[dest_region] = src[src_region]

A case is ``(src_shape, src_padded, dest_shape, dest_padded, src_region, dest_region, dtype)``;
a padded shape of None means no padding. ``CASES`` is the literal table (name -> case): every
row is there for a reason that ``features`` can compute, and tests/test_transfers.py pins what
each row exercises. ``generate(seed, n)`` builds `n` more cases that are valid by construction.
The helpers below build the padded host images of a case and NumPy's answer; they never call
the code under test.
"""

from collections import namedtuple

import numpy as np

SENTINEL = 0xAB  # tests/subviews.py's: every byte of a destination before the copy
SOURCE_PADDING = 0x5C  # every byte of a source's padding: copying it shows as a wrong byte

Case = namedtuple(
    "Case", "src_shape src_padded dest_shape dest_padded src_region dest_region dtype")  # fmt: skip

DTYPES = (np.uint8, np.int16, np.float32, np.complex64, np.complex128)  # 1, 2, 4, 8, 16 bytes
NEW = np.newaxis
u8, i16, f32, c64, c128 = DTYPES

CASES = {
    # ---- ranks and the paths of the rect copy
    "0d": Case((), (), (), (), (), (), f32),
    "1d": Case((17,), (19,), (13,), (16,), np.s_[3:11], np.s_[5:13], i16),
    "2d_rows_merge": Case((6, 8), None, (9, 8), None, np.s_[1:4], np.s_[5:8, :], f32),
    "2d_pitched": Case((7, 9), (8, 12), (5, 11), (6, 13), np.s_[2:6, 1:8], np.s_[0:4, 3:10], c64),
    "3d_loop": Case((4, 5, 6), (5, 6, 8), (5, 6, 7), (5, 8, 9),
                    np.s_[1:4, 0:4, 2:6], np.s_[2:5, 2:6, 0:4], u8),
    "4d_recurse": Case((3, 4, 6, 9), (3, 5, 7, 10), (4, 4, 7, 9), (5, 5, 7, 11),
                       np.s_[0:3, 1:4, 0:6:2, 1:8], np.s_[1:4, 0:3, 1:7:2, 0:7], i16),
    "5d_recurse": Case((4, 3, 4, 6, 7), (4, 4, 4, 7, 8), (3, 4, 4, 6, 7), (4, 4, 5, 6, 8),
                       np.s_[0:4:2, 1:3, ::2, 0:6:2, 2:6], np.s_[1:3, 0:4:2, 0:4:2, 0:6:2, 3:7],
                       u8),
    # ---- steps
    "step_divides": Case((10,), (12,), (10,), None, np.s_[1:7:2], np.s_[2:8:2], f32),
    "step_ragged_inner": Case((4, 10), (4, 12), (4, 7), (5, 8),
                              np.s_[:, 0:10:3], np.s_[:, 1:5], c64),
    "step_ragged_outer": Case((9, 6), (10, 8), (5, 6), (5, 7), np.s_[::4, 1:5], np.s_[1:4, 2:6], u8),
    "step_ragged_both": Case((5, 10), (6, 11), (9, 11), (9, 12),
                             np.s_[::2, 0:10:3], np.s_[::4, 1:11:3], c128),
    "step_single_element": Case((10, 3), (10, 4), (4, 3), None, np.s_[8:10:3], np.s_[3:4], i16),
    # ---- indexing forms
    "int_indices": Case((5, 6, 7), (5, 7, 8), (6, 7), (6, 9), np.s_[3, 1:5, 2], np.s_[1:5, 4], f32),
    "negative_ints": Case((6, 5), (7, 6), (4, 8), (4, 9), np.s_[-2, 1:4], np.s_[-4, -3:], u8),
    "negative_bounds": Case((12, 9), (12, 10), (8, 10), (9, 12),
                            np.s_[-7:-1:2, -6:-2], np.s_[-8:-5, -10:-2:2], c64),
    "newaxis_src": Case((9,), None, (4, 9), (4, 10), np.s_[NEW, 2:7], np.s_[3:, 1:6], c128),
    "newaxis_dest": Case((3, 8), (4, 8), (11,), (12,), np.s_[1:2, 0:8:2], np.s_[NEW, 3:7], i16),
    "missing_axes": Case((6, 4, 5), (6, 5, 6), (8, 4, 5), (8, 4, 7), np.s_[2:5], np.s_[4:7], f32),
    "middle_size_one": Case((4, 1, 6), (5, 2, 7), (6, 1, 6), (6, 3, 8),
                            np.s_[0:3, :, 1:5], np.s_[2:5, :, 0:4], c64),
    # ---- the shapes of the reference's own region tests, restated
    "ref_4d": Case((7, 5, 12, 19), (8, 9, 14, 25), (7, 5, 12, 19), (10, 8, 12, 21),
                   np.s_[2:4, :, 3:7:2, 10:], np.s_[1:3, 0:5, 4:8:2, 10:], np.int32),
    "ref_1d": Case((3, 5), (4, 6), (5, 7), (7, 10), np.s_[1, 0:3], np.s_[2, 1:4], np.int32),
    "ref_2d": Case((3, 5), (4, 6), (5, 7), (7, 10), np.s_[:1, 0:3], np.s_[-1:, 1:4], np.int32),
    "ref_missing_axes": Case((3, 5), (4, 6), (5, 5), (7, 10), np.s_[:1], np.s_[-1:], np.int32),
    "ref_newaxis": Case((10,), None, (10, 10), None, np.s_[NEW, 4:6], np.s_[:1, 7:9], np.int32),
    "ref_negative": Case((10, 12), None, (7, 8), None, np.s_[-4, -3:-1], np.s_[-7, -8:-4:2],
                         np.int32),
}  # fmt: skip


# ------------------------------------------------------------------ what a case exercises
def _items(region):
    return region if isinstance(region, tuple) else (region,)


def _slices(region, shape):
    """(start, stop, step, count) of every slice of `region`, count as NumPy counts."""
    out = []
    axis = 0
    for item in _items(region):
        if item is NEW:
            continue
        if isinstance(item, slice):
            start, stop, step = item.indices(shape[axis])
            out.append((start, stop, step, len(range(start, stop, step))))
        axis += 1
    return out


def ragged_axes(region, shape):
    """Positions, counted from the innermost axis of `shape`, of the slices of `region` whose
    step does not divide their extent (where a floor count differs from NumPy's)."""
    out = set()
    axis = 0
    for item in _items(region):
        if item is NEW:
            continue
        if isinstance(item, slice):
            start, stop, step = item.indices(shape[axis])
            if (stop - start) % step:
                out.add(len(shape) - 1 - axis)
        axis += 1
    return out


def is_ragged(case):
    return bool(ragged_axes(case.src_region, case.src_shape)
                or ragged_axes(case.dest_region, case.dest_shape))  # fmt: skip


def features(case):
    """The indexing forms of `case`, as a set of words (read off the regions alone)."""
    out = set()
    for region, shape in ((case.src_region, case.src_shape), (case.dest_region, case.dest_shape)):
        items = _items(region)
        consumed = sum(item is not NEW for item in items)
        for item in items:
            if item is NEW:
                out.add("newaxis")
            elif isinstance(item, slice):
                if any(v is not None and v < 0 for v in (item.start, item.stop)):
                    out.add("negative_bound")
            else:
                out.add("negative_int" if item < 0 else "int")
        if consumed < len(shape):
            out.add("missing_axes")
        ragged = ragged_axes(region, shape)
        if 0 in ragged:
            out.add("ragged_inner")
        if ragged - {0}:
            out.add("ragged_outer")
        for start, stop, step, count in _slices(region, shape):
            if step > 1:
                out.add("step")
                if count == 1:
                    out.add("single_element_step")
        if len(shape) >= 3 and 1 in shape[1:-1]:
            out.add("middle_size_one")
    return out


# ------------------------------------------------------------------------ host images
def padded_of(shape, padded):
    return tuple(shape) if padded is None else tuple(padded)


def window(full, shape):
    """The ``[:shape]`` window of a padded array."""
    return full[tuple(slice(0, n) for n in shape)] if shape else full


def filled(padded_shape, dtype, byte):
    dtype = np.dtype(dtype)
    count = int(np.prod(padded_shape, dtype=np.int64))
    return np.full(count * dtype.itemsize, byte, np.uint8).view(dtype).reshape(padded_shape)


def values(shape, dtype, seed):
    """Distinct-looking finite data of `dtype`."""
    dtype = np.dtype(dtype)
    rs = np.random.RandomState(seed)
    if dtype.kind == "c":
        data = rs.standard_normal(shape) * 100 + 1j * rs.standard_normal(shape) * 100
        return np.asarray(data).astype(dtype)
    if dtype.kind == "f":
        return np.asarray(rs.standard_normal(shape) * 100).astype(dtype)
    info = np.iinfo(dtype)
    return rs.randint(info.min, info.max + 1, size=shape, dtype=np.int64).astype(dtype)


def host_images(case, seed=0):
    """(src_full, dest_full, expected): the padded source (data in its window, SOURCE_PADDING
    around it), the padded destination before the copy (every byte SENTINEL) and after it."""
    src_full = filled(padded_of(case.src_shape, case.src_padded), case.dtype, SOURCE_PADDING)
    window(src_full, case.src_shape)[...] = values(case.src_shape, case.dtype, seed)
    dest_full = filled(padded_of(case.dest_shape, case.dest_padded), case.dtype, SENTINEL)
    expected = dest_full.copy()
    src = window(src_full, case.src_shape)
    window(expected, case.dest_shape)[case.dest_region] = src[case.src_region]
    return src_full, dest_full, expected


def same_bytes(want, got, what):
    """Byte for byte, naming the first differing element."""
    assert want.dtype == got.dtype and want.shape == got.shape, what
    a = np.ascontiguousarray(want).reshape(-1).view(np.uint8)
    b = np.ascontiguousarray(got).reshape(-1).view(np.uint8)
    bad = np.flatnonzero(a != b)
    if bad.size:
        first = int(bad[0]) // want.dtype.itemsize
        index = np.unravel_index(first, want.shape) if want.shape else ()
        raise AssertionError(
            f"{what}: {bad.size} bytes differ, the first in padded element {tuple(map(int, index))}"
            f" (want byte {int(a[bad[0]]):#04x}, got {int(b[bad[0]]):#04x})")  # fmt: skip


# ------------------------------------------------------- running a case on a backend
# These work on the fake backend and on a device alike: whole padded buffers go up and come
# back through enqueue_write_buffer / enqueue_read_buffer, never through a region call.
def upload(context, queue, shape, padded, full):
    from katsdpsigproc_amd import accel

    array = accel.DeviceArray(context, shape, full.dtype, padded)
    assert array.padded_shape == full.shape
    queue.enqueue_write_buffer(array.buffer, full)
    return array


def download(queue, array):
    out = np.empty(array.padded_shape, array.dtype)
    queue.enqueue_read_buffer(array.buffer, out)
    return out


def host_array(shape, padded, full, context=None):
    """A HostArray (pinned if `context` is given) whose whole allocation holds `full`."""
    from katsdpsigproc_amd import accel

    array = accel.HostArray(shape, full.dtype, padded, context=context)
    accel.HostArray.padded_view(array)[...] = full
    return array


def check_copy_region(context, queue, case, seed=0, what="copy_region"):
    src_full, dest_full, expected = host_images(case, seed)
    src = upload(context, queue, case.src_shape, case.src_padded, src_full)
    dest = upload(context, queue, case.dest_shape, case.dest_padded, dest_full)
    src.copy_region(queue, dest, case.src_region, case.dest_region)
    same_bytes(expected, download(queue, dest), what + ": destination")
    same_bytes(src_full, download(queue, src), what + ": source")


def check_set_region(context, queue, case, plain, blocking=True, pinned=None, seed=0,
                     what="set_region"):  # fmt: skip
    """`plain`: hand over a plain ndarray (a view of the padded image, so it is staged),
    otherwise a HostArray, pinned through `pinned` (a context) if given."""
    from katsdpsigproc_amd import accel

    src_full, dest_full, expected = host_images(case, seed)
    if plain:
        keep = src_full.copy()
        source = window(src_full, case.src_shape)
        assert not accel.HostArray.safe(source)
    else:
        keep = src_full
        source = host_array(case.src_shape, case.src_padded, src_full, pinned)
    dest = upload(context, queue, case.dest_shape, case.dest_padded, dest_full)
    dest.set_region(queue, source, case.dest_region, case.src_region, blocking=blocking)
    if not blocking:
        queue.finish()
    same_bytes(expected, download(queue, dest), what + ": destination")
    held = src_full if plain else accel.HostArray.padded_view(source)
    same_bytes(keep, held, what + ": source")


def check_get_region(context, queue, case, blocking=True, pinned=None, seed=0, what="get_region"):
    from katsdpsigproc_amd import accel

    src_full, dest_full, expected = host_images(case, seed)
    src = upload(context, queue, case.src_shape, case.src_padded, src_full)
    target = host_array(case.dest_shape, case.dest_padded, dest_full, pinned)
    src.get_region(queue, target, case.src_region, case.dest_region, blocking=blocking)
    if not blocking:
        queue.finish()
    same_bytes(expected, accel.HostArray.padded_view(target), what + ": destination")
    same_bytes(src_full, download(queue, src), what + ": source")


# -------------------------------------------------------------------------- generator
CPU_SEED = 20240611  # tests/test_transfers.py: 300 cases on the fake backend
GPU_SEED = 77001  # tests/test_gpu_transfers.py: 100 cases on the device

# largest extent of an axis and largest padding per axis, by rank: keeps every array under 64 kB
_MAX_EXTENT = {1: 20, 2: 20, 3: 11, 4: 6, 5: 4}
_MAX_PAD = {1: 3, 2: 3, 3: 2, 4: 1, 5: 1}


def _axis_for(rs, count, limit):
    """(length, start, step) of an axis of at most `limit` elements on which a slice with
    `count` elements fits, all chosen at random."""
    step = int(rs.randint(1, 5))
    if count > 1:
        step = min(step, (limit - 1) // (count - 1))
    elif rs.rand() < 0.5:
        step = 1
    span = (count - 1) * step + 1
    start = int(rs.randint(0, min(3, limit - span) + 1))
    tail = int(rs.randint(0, min(3, limit - span - start) + 1))
    return start + span + tail, start, step


def _spell_slice(rs, length, start, step, count):
    """A slice object selecting `count` elements from `start` by `step`: any stop that NumPy
    counts the same, bounds negative at times, defaults left out at times."""
    last = start + (count - 1) * step
    stop = int(rs.randint(last + 1, min(length, last + step) + 1))
    if last + step <= length and rs.rand() < 0.6:
        stop = last + step  # the step divides the extent
    lo = start
    hi = stop
    if rs.rand() < 0.3:
        lo = start - length
    if hi == length and rs.rand() < 0.5:
        hi = None
    elif hi < length and rs.rand() < 0.3:
        hi = hi - length
    if lo == 0 and rs.rand() < 0.5:
        lo = None
    return slice(lo, hi, step if step > 1 or rs.rand() < 0.5 else None)


def _spell_int(rs, length):
    index = int(rs.randint(0, length))
    return index - length if rs.rand() < 0.3 else index


def _side(rs, counts, rank):
    """(shape, region) of one side: an array of `rank` axes and an index expression selecting
    `counts`. Every count above 1 takes a slice; a count of 1 takes a slice or, when the
    axes run out or by chance, a newaxis; the remaining axes take integers."""
    n_slices = sum(c > 1 for c in counts)
    ones = [i for i, c in enumerate(counts) if c == 1]
    spare = rank - n_slices
    sliced_ones = set()
    for i in ones:
        if spare > 0 and rs.rand() < 0.7:
            sliced_ones.add(i)
            spare -= 1
    # where the `spare` integer axes go: before item k of the region, or behind the last
    int_slots = sorted(int(rs.randint(0, len(counts) + 1)) for _ in range(spare))
    limit = _MAX_EXTENT[rank]
    shape, region = [], []
    for k, count in enumerate(counts):
        while int_slots and int_slots[0] == k:
            int_slots.pop(0)
            length = int(rs.randint(1, limit + 1))
            shape.append(length)
            region.append(_spell_int(rs, length))
        if count == 1 and k not in sliced_ones:
            region.append(NEW)
            continue
        length, start, step = _axis_for(rs, count, limit)
        shape.append(length)
        region.append(_spell_slice(rs, length, start, step, count))
    for _ in int_slots:
        length = int(rs.randint(1, limit + 1))
        shape.append(length)
        region.append(_spell_int(rs, length))
    # trailing slices that take their axis whole may be left out
    while region and isinstance(region[-1], slice) and rs.rand() < 0.5:
        start, stop, step = region[-1].indices(shape[-1])
        if (start, stop, step) != (0, shape[-1], 1):
            break
        region.pop()
    pad = _MAX_PAD[rank]
    padded = None if rs.rand() < 0.2 else tuple(n + int(rs.randint(0, pad + 1)) for n in shape)
    return tuple(shape), padded, tuple(region)


def generate(seed, n):
    """`n` valid cases from `seed`: a rank of 1 to 5 for each side, a common region shape of
    counts of 1 to 4, then for each side axes on which those counts fit with random starts,
    steps of 1 to 4, integers and newaxes. Nothing is generated and then rejected."""
    rs = np.random.RandomState(seed)
    cases = []
    for _ in range(n):
        src_rank = int(rs.randint(1, 6))
        dest_rank = int(rs.randint(1, 6))
        small = min(src_rank, dest_rank)
        limit = min(_MAX_EXTENT[src_rank], _MAX_EXTENT[dest_rank])
        n_big = int(rs.randint(0, small + 1))  # counts above 1: each needs an axis on both sides
        counts = [int(rs.randint(2, min(4, limit) + 1)) for _ in range(n_big)]
        counts += [1] * int(rs.randint(0, 3))
        counts = [counts[i] for i in rs.permutation(len(counts))]
        dtype = DTYPES[int(rs.randint(0, len(DTYPES)))]
        src_shape, src_padded, src_region = _side(rs, counts, src_rank)
        dest_shape, dest_padded, dest_region = _side(rs, counts, dest_rank)
        cases.append(Case(src_shape, src_padded, dest_shape, dest_padded, src_region, dest_region,
                          dtype))  # fmt: skip
    return cases
