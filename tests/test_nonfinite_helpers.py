"""The planter and the comparer of the non-finite tests, on the CPU (tests/nonfinite.py).

* Every ``kind`` x ``where`` is really planted: the values stand at the returned positions, nothing else changed, and
  every named place is the place its name says.
* An ``inf_pair`` meets in one reduction: the sum over the axis (or over the group) is NaN.
* The comparer accepts a reference compared with itself and rejects four wrong stand-ins by name.
"""
import math

import pytest
import torch

from nonfinite import KINDS, WHERES, assert_same_nonfinite, plant

TOL = dict(rtol=1e-5, atol=1e-5)
SHAPES = [(71,), (70, 7), (3, 66, 5)]


def _base(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * 1.95 + 0.05, g


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("where", WHERES)
@pytest.mark.parametrize("kind", KINDS)
def test_every_kind_and_place_is_planted(kind, where, shape):
    t0, g = _base(shape)
    t = t0.clone()
    ptr = torch.tensor([0, 9, 9, 40, 71]) if (where == "per_graph" and len(shape) == 1) else None
    pos = plant(t, kind, where, g, ptr=ptr)
    graphs = (3 if ptr is not None else shape[0]) if where == "per_graph" else 1
    assert pos.dtype == torch.int64 and pos.shape == (graphs * (2 if kind == "inf_pair" else 1), len(shape))
    assert len({tuple(p) for p in pos.tolist()}) == pos.size(0)  # distinct positions
    changed = torch.zeros(shape, dtype=torch.bool)
    for i, p in enumerate(pos.tolist()):
        v = float(t[tuple(p)])
        changed[tuple(p)] = True
        if kind == "nan":
            assert math.isnan(v)
        elif kind == "inf_pair":
            assert v == (math.inf if i % 2 == 0 else -math.inf)
        else:
            assert v == float(kind)
    assert torch.equal(t[~changed], t0[~changed]) and bool(torch.isfinite(t[~changed]).all())
    assert int((~torch.isfinite(t)).sum()) == pos.size(0)
    flat = [int(sum(p[d] * math.prod(shape[d + 1:]) for d in range(len(shape)))) for p in pos.tolist()]
    n = t.numel()
    if where == "first":
        assert flat[0] == 0
    if where == "last":
        assert flat[0] == n - 1
    if where == "tail":
        assert flat[0] % 4 != 0 and flat[0] >= n - 5
        if n % 4 >= 2:
            assert flat[0] >= 4 * (n // 4)  # inside the remainder of a 4-wide loop
    if where == "tile_row":
        assert pos[0, max(len(shape) - 2, 0)] == 63
    if where == "per_graph" and ptr is None:
        assert pos[:: 2 if kind == "inf_pair" else 1, 0].tolist() == list(range(shape[0]))
    if where == "per_graph" and ptr is not None:  # one per non-empty segment, a pair inside its segment
        owner = (torch.bucketize(pos[:, 0], ptr, right=True) - 1).tolist()
        assert owner == ([0, 0, 2, 2, 3, 3] if kind == "inf_pair" else [0, 2, 3])
    if kind == "inf_pair" and len(shape) > 1:  # the pair meets in the sum over the last axis
        for a, b in zip(pos[0::2].tolist(), pos[1::2].tolist()):
            assert a[:-1] == b[:-1] and a[-1] != b[-1]
            assert math.isnan(float(t[tuple(a[:-1])].sum()))


def test_tile_row_of_a_short_tensor_and_a_smaller_tile():
    t, g = _base((20, 3))
    assert plant(t, "nan", "tile_row", g)[0, 0] == 19
    t, g = _base((2, 70, 3))
    assert plant(t, "nan", "tile_row", g, tile=32)[0, 1] == 31


def test_pair_along_another_axis_and_inside_a_group():
    t, g = _base((2, 9, 6))
    pos = plant(t, "inf_pair", "first", g, axis=-2)
    assert pos[0, 2] == pos[1, 2] and pos[0, 1] != pos[1, 1] and bool(torch.isnan(t.sum(-2)[0, 0]))
    w, g = _base((12,))
    group = torch.tensor([0, 1, 1, 2, 0, 3, 3, 3, 2, 1, 0, 4])
    pos = plant(w, "inf_pair", "first", g, group=group)
    assert pos[0, 0] == 0 and int(group[pos[1, 0]]) == 0 and pos[1, 0] != 0
    sums = torch.zeros(5).index_add_(0, group, w)
    assert bool(torch.isnan(sums[0])) and bool(torch.isfinite(sums[1:]).all())
    with pytest.raises(ValueError):  # the group of row 11 has one member
        plant(w.clone(), "inf_pair", "last", g, group=group)


def test_per_graph_with_offsets_skips_empty_graphs():
    x, g = _base((10, 4))
    ptr = torch.tensor([0, 3, 3, 9, 10])
    pos = plant(x, "+inf", "per_graph", g, ptr=ptr)
    assert pos.size(0) == 3
    assert [int(torch.bucketize(p, ptr, right=True)) - 1 for p in pos[:, 0]] == [0, 2, 3]


def test_bad_arguments_raise():
    t, g = _base((8,))
    for call in (lambda: plant(t, "inf", "first", g), lambda: plant(t, "nan", "middle", g),
                 lambda: plant(torch.arange(4), "nan", "first", g), lambda: plant(t, "nan", "per_graph", g),
                 lambda: plant(torch.zeros(1), "nan", "tail", g)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        assert_same_nonfinite(t, t)


# ------------------------------------------------------------------------------------------------ the comparer
def _reference():
    t, g = _base((3, 40, 6), seed=1)
    plant(t, "nan", "tail", g)
    plant(t[1], "+inf", "first", g)
    plant(t[2], "-inf", "last", g)
    return t


def test_the_comparer_accepts_the_reference_and_a_close_result():
    want = _reference()
    assert_same_nonfinite(want.clone(), want, **TOL)
    near = want * (1 + 1e-6)
    assert_same_nonfinite(near, want, **TOL)
    nan_other_payload = want.clone()
    nan_other_payload[torch.isnan(want)] = -float("nan")
    assert_same_nonfinite(nan_other_payload, want, **TOL)
    assert_same_nonfinite(torch.tensor([0.0, -0.0]), torch.tensor([-0.0, 0.0]), **TOL)  # the sign of zero is not compared
    assert_same_nonfinite(torch.tensor([[1, 2], [3, 4]]), torch.tensor([[1, 2], [3, 4]]))
    seen = []
    assert_same_nonfinite(want.double(), want.double(), close=lambda a, b, what: seen.append((a.numel(), what)), what="x")
    assert seen == [(want.numel() - 3, "x")]


def test_a_nan_replaced_by_the_finite_maximum_is_rejected():
    """What fmaxf does to a max over a group with a NaN member."""
    want = _reference()
    bad = want.clone()
    bad[torch.isnan(want)] = want[torch.isfinite(want)].max()
    with pytest.raises(AssertionError, match="NaN masks differ.*where the reference is NaN"):
        assert_same_nonfinite(bad, want, **TOL)


def test_a_nan_where_the_reference_is_finite_is_rejected():
    want = _reference()
    bad = want.clone()
    bad[0, 0, 0] = float("nan")
    with pytest.raises(AssertionError, match="NaN where the reference is not"):
        assert_same_nonfinite(bad, want, **TOL)


def test_an_infinity_with_its_sign_flipped_is_rejected():
    want = _reference()
    bad = want.clone()
    bad[torch.isinf(want)] = -want[torch.isinf(want)]
    with pytest.raises(AssertionError, match="infinity of the other sign"):
        assert_same_nonfinite(bad, want, **TOL)
    finite = want.clone()
    finite[torch.isinf(want)] = 3.0e38
    with pytest.raises(AssertionError, match="infinity masks differ"):
        assert_same_nonfinite(finite, want, **TOL)


def test_a_zero_loss_where_the_reference_is_nan_is_rejected():
    """The fused link loss of a diverged model: sqrt(fmaxf(NaN, 0)) = 0."""
    with pytest.raises(AssertionError, match="NaN masks differ"):
        assert_same_nonfinite(torch.tensor(0.0), torch.tensor(float("nan")), **TOL)


def test_finite_errors_shapes_and_integers_are_still_compared():
    want = _reference()
    off = want.clone()
    off[0, 1, 1] *= 1.001
    with pytest.raises(AssertionError):
        assert_same_nonfinite(off, want, **TOL)
    with pytest.raises(AssertionError, match="shape"):
        assert_same_nonfinite(want[:2], want, **TOL)
    with pytest.raises(AssertionError, match="integer tensors differ"):
        assert_same_nonfinite(torch.tensor([[0, 1], [1, 0]]), torch.tensor([[0, 1], [1, 1]]))
    with pytest.raises(AssertionError, match="dtype"):
        assert_same_nonfinite(torch.tensor([1.0]), torch.tensor([1]))
