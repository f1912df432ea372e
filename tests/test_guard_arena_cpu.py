"""The guard arena's checker (tests/guard_arena.py) on plain CPU tensors: a stray element in either guard, an element left
unwritten and an element that depends on what the memory held before are each reported at the right index, and a clean fill
passes; so do 2-byte elements, an element written where a `written=` mask says untouched, and the guards of in-place
state.  This is what shows the checker has teeth: the GPU tests (tests/test_gpu_guard_bands.py,
tests/test_gpu_guard_bands_state.py) mutate no kernel."""
import numpy as np
import pytest
import torch

from tests import guard_arena as ga

SHAPES = [((3, 5, 4), torch.float32), ((1, 5, 260), torch.float32), ((3, 5, 4), torch.uint8), ((12, 68), torch.float64),
          ((5, 4), torch.float32)]
IDS = ["rates-3x5x4", "rates-1x5x260", "spikes-3x5x4", "state-12x68", "noise-5x4"]


def _fill(view, seed=0):
    """what a correct kernel does: every element of the view, values no canary"""
    rs = np.random.RandomState(seed)
    if view.dtype == torch.uint8:
        view.copy_(torch.from_numpy(rs.randint(0, 2, view.shape).astype(np.uint8)))
    else:
        view.copy_(torch.from_numpy(rs.uniform(0, 1, view.shape)).to(view.dtype))


@pytest.mark.parametrize("canary", ga.CANARIES)
@pytest.mark.parametrize("shape,dtype", SHAPES, ids=IDS)
def test_layout_and_clean_fill(shape, dtype, canary):
    arena = ga.GuardArena(canary)
    v = arena.view(shape, dtype)
    buf = arena.base(v)
    size = buf.element_size()
    assert v.shape == shape and v.dtype == dtype and v.is_contiguous() and v.data_ptr() % 16 == 0
    front = (v.data_ptr() - buf.data_ptr()) // size
    g = max(4096, 64 * shape[-1])
    assert front >= g and len(buf) - front - v.numel() >= g
    assert v.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()          # ONE allocation
    word = ga.canary_bits(canary, size)
    assert (buf.view(ga._INT[size]) == word).all()
    if dtype != torch.uint8:
        assert bool(torch.isnan(buf).all()) == (canary == "nan")
        if canary == "finite":
            assert (buf == -7.0).all()
    with pytest.raises(ga.GuardError) as e:                                            # nothing written yet
        arena.check(v)
    assert e.value.kind == "unwritten" and e.value.count == v.numel()
    assert e.value.first == (0,) * len(shape) and e.value.last == tuple(d - 1 for d in shape)
    _fill(v)
    got = arena.check(v)
    assert isinstance(got, np.ndarray) and got.shape == shape
    np.testing.assert_array_equal(got, v.numpy())
    # the other canary's run of the same "kernel": the same bits
    other = ga.GuardArena(ga.CANARIES[1 - ga.CANARIES.index(canary)])
    w = other.view(shape, dtype)
    _fill(w)
    np.testing.assert_array_equal(other.check(w, other=got), got)


def test_coords():
    assert ga.coords(0, (3, 5, 4)) == (0, 0, 0)
    assert ga.coords(59, (3, 5, 4)) == (2, 4, 3)
    assert ga.coords(60, (3, 5, 4)) == (3, 0, 0)           # cell 0 of the row behind the last one
    assert ga.coords(20, (1, 5, 4)) == (1, 0, 0)
    assert ga.coords(-1, (3, 5, 4)) == (-1, 4, 3)
    assert ga.coords(-21, (3, 5, 4)) == (-2, 4, 3)
    assert ga.coords(-6, (3, 5, 4)) == (-1, 3, 2)
    assert ga.coords(68 * 12 + 5, (12, 68)) == (12, 5)


@pytest.mark.parametrize("canary", ga.CANARIES)
@pytest.mark.parametrize("shape,dtype", SHAPES, ids=IDS)
def test_strays_in_the_guards_are_located(shape, dtype, canary):
    arena = ga.GuardArena(canary)
    v = arena.view(shape, dtype)
    _fill(v)
    flat = arena.base(v)
    front = (v.data_ptr() - flat.data_ptr()) // flat.element_size()
    n = v.numel()
    row = n // shape[0]
    # behind the view: the store for "cell n" of the last row = the first element of row T, and one more, 7 further
    flat[front + n] = 0.5 if dtype != torch.uint8 else 1
    flat[front + n + 7] = 0.5 if dtype != torch.uint8 else 1
    with pytest.raises(ga.GuardError) as e:
        arena.check(v)
    assert e.value.kind == "back guard" and e.value.count == 2
    assert e.value.first == ga.coords(n, shape) == (shape[0],) + (0,) * (len(shape) - 1)
    assert e.value.last == ga.coords(n + 7, shape)
    word = ga.canary_bits(canary, flat.element_size())
    flat.view(ga._INT[flat.element_size()])[front + n:front + n + 8] = word
    arena.check(v)
    # in front of it: one element, the last lane of the row before row 0
    flat[front - 1] = 0
    with pytest.raises(ga.GuardError) as e:
        arena.check(v)
    assert e.value.kind == "front guard" and e.value.count == 1
    assert e.value.first == e.value.last == (-1,) + tuple(d - 1 for d in shape[1:])
    flat.view(ga._INT[flat.element_size()])[front - 1] = word
    # ... and the far ends of both guards are read too
    flat[0] = 0
    with pytest.raises(ga.GuardError) as e:
        arena.check(v)
    assert e.value.kind == "front guard" and e.value.first == ga.coords(-front, shape)
    flat.view(ga._INT[flat.element_size()])[0] = word
    flat[len(flat) - 1] = 0
    with pytest.raises(ga.GuardError) as e:
        arena.check(v)
    assert e.value.kind == "back guard" and e.value.last == ga.coords(len(flat) - 1 - front, shape)
    assert row > 0


@pytest.mark.parametrize("canary", ga.CANARIES)
@pytest.mark.parametrize("shape,dtype", SHAPES[:4], ids=IDS[:4])
def test_an_unwritten_element_is_located(shape, dtype, canary):
    arena = ga.GuardArena(canary)
    v = arena.view(shape, dtype)
    _fill(v)
    idx = tuple(d - 1 for d in shape[:-1]) + (shape[-1] - 2,)       # the ragged edge: last cell, last lane but one
    v.view(ga._INT[v.element_size()])[idx] = ga.canary_bits(canary, v.element_size())
    with pytest.raises(ga.GuardError) as e:
        arena.check(v)
    assert e.value.kind == "unwritten" and e.value.count == 1 and e.value.first == e.value.last == idx
    assert str(idx) in str(e.value)


@pytest.mark.parametrize("shape,dtype", SHAPES[:4], ids=IDS[:4])
def test_a_canary_dependent_element_is_located(shape, dtype):
    """a kernel that, say, accumulates into its output instead of storing: finite with the finite canary (so neither guard
    nor interior check fires), another value with the other canary"""
    runs = []
    for canary in ga.CANARIES:
        arena = ga.GuardArena(canary)
        v = arena.view(shape, dtype)
        _fill(v)
        runs.append((arena, v))
    idx = (0,) * (len(shape) - 1) + (3,)
    got = runs[0][0].check(runs[0][1])
    runs[1][0].check(runs[1][1], other=got)                          # identical so far
    runs[1][1][idx] = 1 - runs[1][1][idx] if dtype == torch.uint8 else runs[1][1][idx] + 0.25
    with pytest.raises(ga.GuardError) as e:
        runs[1][0].check(runs[1][1], other=got)
    assert e.value.kind == "canary-dependent" and e.value.count == 1 and e.value.first == e.value.last == idx
    # -0.0 against +0.0 are different bits: the comparison is not a float one
    if dtype != torch.uint8:
        runs[1][1].copy_(runs[0][1])
        runs[0][1][idx] = 0.0
        runs[1][1][idx] = -0.0
        with pytest.raises(ga.GuardError) as e:
            runs[1][0].check(runs[1][1], other=runs[0][0].check(runs[0][1]))
        assert e.value.kind == "canary-dependent" and e.value.first == idx


# ---- 2-byte elements (the rate maps' bin ids) ---------------------------------------------------------------------------
BIN_SHAPE = (3, 68)


@pytest.mark.parametrize("canary", ga.CANARIES)
def test_two_byte_canaries_are_no_bin_id(canary):
    bits = ga._BITS[canary][2]
    assert 4096 <= bits < 0xFFFF                    # no valid bin id (< RIAB_RATEMAP_MAX_BINS), not RIAB_RATEMAP_DROPPED
    assert ga._BITS["nan"][2] != ga._BITS["finite"][2]
    assert ga.canary_bits(canary, 2) == np.array(bits, dtype=np.uint16).view(np.int16)


@pytest.mark.parametrize("canary", ga.CANARIES)
def test_two_byte_views(canary):
    """uint16 [T][B]: the layout, a clean fill with bin ids and 0xFFFF, then a stray behind, one in front and one element
    left unwritten, each at its index"""
    arena = ga.GuardArena(canary)
    v = arena.view(BIN_SHAPE, torch.uint16)
    buf = arena.base(v)
    assert v.dtype == torch.uint16 and v.shape == BIN_SHAPE and v.data_ptr() % 16 == 0 and buf.element_size() == 2
    front = (v.data_ptr() - buf.data_ptr()) // 2
    assert front >= 4096 and len(buf) - front - v.numel() >= 4096
    word = ga.canary_bits(canary, 2)
    raw = buf.view(torch.int16)
    assert (raw == word).all()
    with pytest.raises(ga.GuardError) as e:
        arena.check(v)
    assert e.value.kind == "unwritten" and e.value.count == v.numel()
    ids = np.random.RandomState(2).randint(0, 4096, BIN_SHAPE).astype(np.uint16)
    ids[:, -3:] = 0xFFFF                             # padding lanes
    v.view(torch.int16).copy_(torch.from_numpy(ids.view(np.int16)))
    got = arena.check(v)
    assert got.dtype == np.uint16
    np.testing.assert_array_equal(got, ids)
    n = v.numel()
    raw[front + n + 5] = 7                           # row T, lane 5
    with pytest.raises(ga.GuardError) as e:
        arena.check(v)
    assert e.value.kind == "back guard" and e.value.count == 1 and e.value.first == e.value.last == (3, 5)
    raw[front + n + 5] = word
    raw[front - 2] = -1                              # 0xFFFF in front: a padding lane of row -1
    with pytest.raises(ga.GuardError) as e:
        arena.check(v)
    assert e.value.kind == "front guard" and e.value.first == (-1, 66)
    raw[front - 2] = word
    v.view(torch.int16)[2, 63] = word
    with pytest.raises(ga.GuardError) as e:
        arena.check(v)
    assert e.value.kind == "unwritten" and e.value.first == e.value.last == (2, 63)
    # ... and the other canary's run of the same ids compares equal
    other = ga.GuardArena(ga.CANARIES[1 - ga.CANARIES.index(canary)])
    w = other.view(BIN_SHAPE, torch.uint16)
    w.view(torch.int16).copy_(torch.from_numpy(ids.view(np.int16)))
    other.check(w, other=ids)
    w.view(torch.int16)[1, 4] += 1
    with pytest.raises(ga.GuardError) as e:
        other.check(w, other=ids)
    assert e.value.kind == "canary-dependent" and e.value.first == e.value.last == (1, 4)


# ---- check(view, written=mask) ------------------------------------------------------------------------------------------
MASKED = [((7, 3, 68), torch.float64), ((6, 2, 4), torch.float64), ((3, 68), torch.uint16), ((5, 4), torch.int32)]
MASKED_IDS = ["future-7x3x68", "z_out-6x2x4", "bin_ids-3x68", "count-5x4"]


def _mask(shape):
    """a ragged contract: lane b has the first 1 + b % shape[0] entries of the leading axis written"""
    k = np.arange(shape[0]).reshape((-1,) + (1,) * (len(shape) - 1))
    b = np.arange(shape[-1]).reshape((1,) * (len(shape) - 1) + (-1,))
    return np.broadcast_to(k <= b % shape[0], shape).copy()


def _fill_where(view, mask, seed=0):
    rs = np.random.RandomState(seed)
    size = view.element_size()
    raw = view.view(ga._INT[size])
    vals = rs.randint(1, 4000, view.shape) if not view.dtype.is_floating_point else \
        rs.uniform(0, 1, view.shape).view(np.int64)
    m = torch.from_numpy(mask)
    raw[m] = torch.from_numpy(vals).to(raw.dtype)[m]


@pytest.mark.parametrize("canary", ga.CANARIES)
@pytest.mark.parametrize("shape,dtype", MASKED, ids=MASKED_IDS)
def test_written_mask(shape, dtype, canary):
    arena = ga.GuardArena(canary)
    v = arena.view(shape, dtype)
    mask = _mask(shape)
    assert mask.any() and not mask.all()
    size = v.element_size()
    raw, word = v.view(ga._INT[size]), ga.canary_bits(canary, size)
    with pytest.raises(ga.GuardError) as e:                         # nothing written: every True element is reported
        arena.check(v, written=mask)
    assert e.value.kind == "unwritten" and e.value.count == int(mask.sum()) and e.value.first == (0,) * len(shape)
    _fill_where(v, mask)
    got = arena.check(v, written=mask)
    assert got.shape == shape
    with pytest.raises(ga.GuardError) as e:                         # without the mask the untouched ones are "unwritten"
        arena.check(v)
    assert e.value.kind == "unwritten" and e.value.count == int((~mask).sum())
    # one element past a lane's last entry written: the new kind, at its index
    lane = shape[-1] - 2
    idx = (lane % shape[0] + 1,) + (0,) * (len(shape) - 2) + (lane,)
    assert not mask[idx]
    raw[idx] = 3
    with pytest.raises(ga.GuardError) as e:
        arena.check(v, written=mask)
    assert e.value.kind == ga.UNTOUCHED == "written where the contract says untouched"
    assert e.value.count == 1 and e.value.first == e.value.last == idx and str(idx) in str(e.value)
    # two of them: first, last and the count
    idx2 = (shape[0] - 1,) + (0,) * (len(shape) - 2) + (0,)
    assert not mask[idx2] and idx2 > idx
    raw[idx2] = 3
    with pytest.raises(ga.GuardError) as e:
        arena.check(v, written=mask)
    assert e.value.kind == ga.UNTOUCHED and e.value.count == 2 and e.value.first == idx and e.value.last == idx2
    raw[idx], raw[idx2] = word, word
    arena.check(v, written=mask)
    # an element the contract says is written and that was skipped
    idx3 = (0,) * (len(shape) - 1) + (shape[-1] - 1,)
    assert mask[idx3]
    keep = raw[idx3].clone()
    raw[idx3] = word
    with pytest.raises(ga.GuardError) as e:
        arena.check(v, written=mask)
    assert e.value.kind == "unwritten" and e.value.count == 1 and e.value.first == idx3
    raw[idx3] = keep
    # the guards are checked as ever
    flat = arena.base(v).view(ga._INT[size])
    front = (v.data_ptr() - flat.data_ptr()) // size
    flat[front + v.numel()] = 1
    with pytest.raises(ga.GuardError) as e:
        arena.check(v, written=mask)
    assert e.value.kind == "back guard" and e.value.first == (shape[0],) + (0,) * (len(shape) - 1)


@pytest.mark.parametrize("shape,dtype", MASKED[:2], ids=MASKED_IDS[:2])
def test_written_mask_compares_the_written_elements_only(shape, dtype):
    mask = _mask(shape)
    runs = []
    for canary in ga.CANARIES:
        arena = ga.GuardArena(canary)
        v = arena.view(shape, dtype)
        _fill_where(v, mask)
        runs.append((arena, v))
    got = runs[0][0].check(runs[0][1], written=mask)
    runs[1][0].check(runs[1][1], written=mask, other=got)          # the untouched elements differ (two canaries): no error
    idx = (0,) * (len(shape) - 1) + (2,)
    assert mask[idx]
    runs[1][1][idx] += 0.25
    with pytest.raises(ga.GuardError) as e:
        runs[1][0].check(runs[1][1], written=mask, other=got)
    assert e.value.kind == "canary-dependent" and e.value.count == 1 and e.value.first == e.value.last == idx


# ---- check(view, inplace=True) ------------------------------------------------------------------------------------------
INPLACE = [((12, 68), torch.float64), ((2, 4), torch.float64), ((4096,), torch.float64), ((2, 132), torch.int32)]
INPLACE_IDS = ["state-12x68", "displacement-2x4", "counts-4096", "flags-2x132"]


@pytest.mark.parametrize("canary", ga.CANARIES)
@pytest.mark.parametrize("shape,dtype", INPLACE, ids=INPLACE_IDS)
def test_inplace(shape, dtype, canary):
    arena = ga.GuardArena(canary)
    v = arena.view(shape, dtype)
    size = v.element_size()
    word = ga.canary_bits(canary, size)
    arena.check(v, inplace=True)                       # nothing is "unwritten" by its bits, not even the canary itself
    v.zero_()
    v.view(-1)[1] = 3
    got = arena.check(v, inplace=True)
    assert got.shape == shape and got.reshape(-1)[1] == 3 and got.reshape(-1)[0] == 0
    v.view(ga._INT[size]).view(-1)[2] = word           # a real value that happens to be the canary's bits
    arena.check(v, inplace=True)
    with pytest.raises(ga.GuardError):
        arena.check(v)
    v.view(-1)[2] = 0
    # guards
    flat = arena.base(v).view(ga._INT[size])
    front = (v.data_ptr() - flat.data_ptr()) // size
    n = v.numel()
    flat[front + n + 3] = 0
    with pytest.raises(ga.GuardError) as e:
        arena.check(v, inplace=True)
    assert e.value.kind == "back guard" and e.value.count == 1 and e.value.first == e.value.last == ga.coords(n + 3, shape)
    flat[front + n + 3] = word
    flat[front - 1] = 0
    with pytest.raises(ga.GuardError) as e:
        arena.check(v, inplace=True)
    assert e.value.kind == "front guard" and e.value.first == ga.coords(-1, shape)
    flat[front - 1] = word
    # `other`: the two canaries' interiors, bit for bit
    other = ga.GuardArena(ga.CANARIES[1 - ga.CANARIES.index(canary)])
    w = other.view(shape, dtype)
    w.copy_(v)
    other.check(w, inplace=True, other=got)
    last = tuple(d - 1 for d in shape)
    w[last] += 1
    with pytest.raises(ga.GuardError) as e:
        other.check(w, inplace=True, other=got)
    assert e.value.kind == "canary-dependent" and e.value.count == 1 and e.value.first == e.value.last == last


def test_inplace_and_written_exclude_each_other():
    arena = ga.GuardArena("nan")
    v = arena.view((2, 4), torch.float64)
    with pytest.raises(AssertionError):
        arena.check(v, written=np.ones((2, 4), dtype=bool), inplace=True)
    with pytest.raises(AssertionError):                # the mask must have the view's shape and be boolean
        arena.check(v, written=np.ones((4, 2), dtype=bool))
    with pytest.raises(AssertionError):
        arena.check(v, written=np.ones((2, 4)))


def test_guard_width():
    assert ga.guard_elements((3, 5, 4)) == 4096
    assert ga.guard_elements((1, 17, 1028)) == 64 * 1028
    assert ga.guard_elements((12, 68)) == 64 * 68
