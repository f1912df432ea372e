"""The guard arena's checker (tests/guard_arena.py) on plain CPU tensors: a stray element in either guard, an element left
unwritten and an element that depends on what the memory held before are each reported at the right index, and a clean fill
passes.  This is what shows the checker has teeth: the GPU tests (tests/test_gpu_guard_bands.py) mutate no kernel."""
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


def test_guard_width():
    assert ga.guard_elements((3, 5, 4)) == 4096
    assert ga.guard_elements((1, 17, 1028)) == 64 * 1028
    assert ga.guard_elements((12, 68)) == 64 * 68
