"""Non-finite inputs for the operator tests (tests/test_gpu_nonfinite.py, tests/test_nonfinite_helpers.py).

:func:`plant` writes a NaN, an infinity or a pair of opposite infinities into a tensor at a named place and says where;
:func:`assert_same_nonfinite` compares a product with its reference under the rule "NaN where the reference is NaN,
the same infinity where the reference is infinite, close everywhere else".  Neither knows an operator.
"""
import torch

KINDS = ("nan", "+inf", "-inf", "inf_pair")
WHERES = ("first", "last", "tail", "tile_row", "per_graph")
_VALUE = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}


def _pick(n, generator):
    return int(torch.randint(0, n, (1,), generator=generator))


def _partner(t, pos, axis, group, generator, seg=None):
    """A second position that meets ``pos`` in one reduction: another member of the same ``group`` (dimension 0), or
    another index along ``axis`` (inside the graph's rows ``seg`` = (lo, hi) where the axis is dimension 0)."""
    if group is not None:
        members = (group == group[pos[0]]).nonzero().view(-1).tolist()
        members = [m for m in members if m != pos[0]]
        if not members:
            raise ValueError(f"group {int(group[pos[0]])} has one member: no place for the second infinity")
        return (members[_pick(len(members), generator)],) + tuple(pos[1:])
    axis = axis % t.dim()
    lo, hi = seg if (seg is not None and axis == 0) else (0, t.size(axis))
    if hi - lo < 2:
        raise ValueError("the reduced axis has one element: no place for the second infinity")
    other = lo + (pos[axis] - lo + 1 + _pick(hi - lo - 1, generator)) % (hi - lo)
    return tuple(other if d == axis else p for d, p in enumerate(pos))


def plant(t, kind, where, generator, *, axis=-1, tile=64, ptr=None, group=None):
    """Write ``kind`` into ``t`` IN PLACE at ``where``; returns the planted positions as a [P, t.dim()] int64 tensor.

    kind      "nan", "+inf", "-inf", or "inf_pair": +inf at the position and -inf at a partner that meets it in one
              reduction -- another index along ``axis``, or with ``group`` (int64 [t.size(0)]: the reduction a row
              belongs to, e.g. a coalesce key) another row of the same group.  Both positions are returned, +inf first.
    where     "first"      element 0 of the flattened tensor
              "last"       its last element
              "tail"       a flat index that is no multiple of 4 inside the remainder a 4-wide vector loop leaves
                           (4 * (n // 4) + 1); with a remainder of fewer than two elements the highest such index
                           below the last element
              "tile_row"   row min(tile, rows) - 1 of dimension -2 (dimension 0 of a vector): the last row of the first
                           tile; the other indices are drawn
              "per_graph"  one drawn element in every graph: every slice of dimension 0, or with ``ptr`` ([B + 1]
                           offsets into dimension 0; a vector needs them) every non-empty segment -- a pair along
                           dimension 0 stays inside its segment
    """
    if kind not in KINDS:
        raise ValueError(f"kind {kind!r} not in {KINDS}")
    if where not in WHERES:
        raise ValueError(f"where {where!r} not in {WHERES}")
    if not t.is_floating_point() or t.numel() == 0:
        raise ValueError("plant needs a non-empty floating-point tensor")
    shape = tuple(t.shape)

    def unflat(i):
        out = []
        for s in reversed(shape):
            out.append(i % s)
            i //= s
        return tuple(reversed(out))

    n = t.numel()
    if where == "first":
        spots = [unflat(0)]
    elif where == "last":
        spots = [unflat(n - 1)]
    elif where == "tail":
        q4 = 4 * (n // 4)
        if n - q4 >= 2:
            spots = [unflat(q4 + 1)]
        else:
            cand = [i for i in range(max(n - 5, 0), n - 1) if i % 4 != 0]
            if not cand:
                raise ValueError("the tensor is too short for a tail position")
            spots = [unflat(cand[-1])]
    elif where == "tile_row":
        rdim = t.dim() - 2 if t.dim() >= 2 else 0
        spots = [tuple(min(tile, s) - 1 if d == rdim else _pick(s, generator) for d, s in enumerate(shape))]
    else:
        if ptr is None and t.dim() == 1:
            raise ValueError("one per graph in a vector needs the graphs' offsets (ptr)")
        if ptr is None:
            starts, stops = list(range(shape[0])), list(range(1, shape[0] + 1))
        else:
            starts, stops = ptr[:-1].tolist(), ptr[1:].tolist()
        spots, segs = [], {}
        for a, b in zip(starts, stops):
            if b > a:
                segs[len(spots)] = (a, b) if ptr is not None else None
                spots.append((a + _pick(b - a, generator),) + tuple(_pick(s, generator) for s in shape[1:]))
        if not spots:
            raise ValueError("no graph has a row")
    placed = []
    for i, pos in enumerate(spots):
        if kind == "inf_pair":
            other = _partner(t, pos, axis, group, generator, segs.get(i) if where == "per_graph" else None)
            t[pos] = float("inf")
            t[other] = float("-inf")
            placed += [pos, other]
        else:
            t[pos] = _VALUE[kind]
            placed.append(pos)
    return torch.tensor(placed, dtype=torch.int64).view(len(placed), t.dim())


def assert_same_nonfinite(got, want, what="output", close=None, **tol):
    """``got`` equals ``want`` in the sense of the operator tests:

    * integer and bool tensors: ``torch.equal``;
    * float tensors: equal shapes, equal ``isnan`` masks, equal ``isinf`` masks with equal signs, and the remaining
      entries compared with ``torch.testing.assert_close(**tol)`` -- or, with ``close``, by ``close(got_rest, want_rest,
      what)`` on the two vectors of remaining entries (the float64 rule of tests/test_gpu_dense_pool.py).

    NaN payloads and the sign of zero are not compared.  A tolerance must be given for a float tensor."""
    assert isinstance(got, torch.Tensor) and isinstance(want, torch.Tensor), f"{what}: not two tensors"
    got, want = got.detach().cpu(), want.detach().cpu()
    assert tuple(got.shape) == tuple(want.shape), f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    if not want.is_floating_point():
        assert not got.is_floating_point(), f"{what}: dtype {got.dtype}, the reference is {want.dtype}"
        assert torch.equal(got.to(torch.int64), want.to(torch.int64)), f"{what}: integer tensors differ"
        return
    assert got.is_floating_point(), f"{what}: dtype {got.dtype}, the reference is {want.dtype}"
    if close is None and not tol:
        raise TypeError("assert_same_nonfinite needs a tolerance (rtol=, atol=) or close= for a float tensor")
    g_nan, w_nan = torch.isnan(got), torch.isnan(want)
    if not torch.equal(g_nan, w_nan):
        lost, made = (w_nan & ~g_nan).nonzero(), (g_nan & ~w_nan).nonzero()
        msg = f"{what}: NaN masks differ"
        if lost.size(0):
            p = tuple(lost[0].tolist())
            msg += f"; {lost.size(0)} entries finite or infinite where the reference is NaN, first {p}: {got[p].item()!r}"
        if made.size(0):
            p = tuple(made[0].tolist())
            msg += f"; {made.size(0)} entries NaN where the reference is not, first {p}: reference {want[p].item()!r}"
        raise AssertionError(msg)
    g_inf, w_inf = torch.isinf(got), torch.isinf(want)
    if not torch.equal(g_inf, w_inf):
        bad = (g_inf != w_inf).nonzero()
        p = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: infinity masks differ at {bad.size(0)} entries, first {p}: {got[p].item()!r} "
                             f"against the reference's {want[p].item()!r}")
    if bool(w_inf.any()):
        flipped = (w_inf & ((got > 0) != (want > 0))).nonzero()
        if flipped.size(0):
            p = tuple(flipped[0].tolist())
            raise AssertionError(f"{what}: an infinity of the other sign at {flipped.size(0)} entries, first {p}: "
                                 f"{got[p].item()!r} against the reference's {want[p].item()!r}")
    rest = ~(w_nan | w_inf)
    if not bool(rest.any()):
        return
    if close is not None:
        close(got[rest], want[rest], what)
    else:
        torch.testing.assert_close(got[rest], want[rest], msg=lambda m: f"{what}: {m}", **tol)
