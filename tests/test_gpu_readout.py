"""The aggregation readout on the MI355X: ``GlobalReduce`` / ``AggrReduce`` and the aggregation classes against the
reference's stored results and against the float64 restatement on shapes chosen to reach every route of
csrc/segment_aggr.hip (scalar and 16-byte loads; short segments, segments of exactly one chunk, the split route;
contiguous, dense, masked and gathered rows).

Tolerances are derived, not measured.  Max and min are selections: ``torch.equal``.  Sums of small integers are exact
in any order: ``torch.equal``.  A float32 sum of n terms in ANY order is within n * 2^-24 * sum|x_i| of the exact sum
(each of the at most n - 1 additions rounds a partial sum no larger than sum|x_i|); the mean adds the rounding of one
division.  Gradients of integer-valued inputs are at most two float32 roundings from the float64 value: rtol 1e-6."""
import pytest
import torch

import readout_restatement as R

from tgp import kernels as K
from tgp.reduce import AggrReduce, GlobalReduce, MultiAggregation, SumAggregation, get_aggr
from tgp.select import SelectOutput

pytestmark = pytest.mark.gpu

CASES = R.load_cases()
U = 2.0 ** -24  # float32 unit roundoff
ALL4 = ("sum", "mean", "max", "min")


def dev():
    return torch.device("cuda:0")


def mv(t):
    return None if t is None else t.to(dev())


def make_so(i, x_dtype=torch.float32, weight=None):
    """The SelectOutput of a fixture-shaped assignment on the device; ``weight`` (a leaf) is handed out as ``so.weight``."""
    w = i["weight"] if weight is None else weight.detach()
    so = SelectOutput(node_index=mv(i["node_index"]), cluster_index=mv(i["cluster_index"]),
                      weight=None if w is None else mv(w).to(x_dtype), num_nodes=i["num_nodes"],
                      num_supernodes=i["num_supernodes"])
    if weight is not None:
        assert torch.equal(so.node_index, mv(i["node_index"]))  # (ascending rows: the values keep their order)
        so._hold_values(weight)
    return so


def run_public(case, x, weight=None):
    """The public classes on a fixture case: (x_pool, batch_pool)."""
    i = case["inputs"]
    op, kw = case["op"], case["op_kwargs"]
    if case["kind"] == "global":
        return GlobalReduce(op, **kw)(x, batch=mv(i.get("batch")), size=i.get("size"), mask=mv(i.get("mask"))), None
    reducer = AggrReduce(get_aggr(op, **kw))
    if "node_index" in i:
        return reducer(x, make_so(i, x.dtype, weight), batch=mv(i["batch"]))
    return reducer(x, batch=mv(i.get("batch")), size=i.get("size"))


def check_against_f64(out, ops, src64, index, groups, what=""):
    """``out`` [G, n_ops * F] (float32, any device) against the float64 restatement over the rows ``src64`` [n, F]."""
    out = out.detach().cpu()
    F = src64.size(1)
    n = torch.zeros(groups, dtype=torch.float64).index_add_(0, index, torch.ones(index.numel(), dtype=torch.float64))
    sum_abs = torch.zeros(groups, F, dtype=torch.float64).index_add_(0, index, src64.abs())
    for k, op in enumerate(ops):
        got = out[:, k * F:(k + 1) * F]
        want = R.scatter(src64, index, groups, op)
        if op in ("max", "min"):
            assert torch.equal(got.double(), want), f"{what} {op}"
            continue
        bound = n.view(-1, 1) * U * sum_abs
        if op == "mean":
            bound = bound / n.clamp(min=1).view(-1, 1) + U * want.abs()
        err = (got.double() - want).abs()
        assert bool((err <= bound).all()), f"{what} {op}: max excess {(err - bound).max().item():.3e}"


# ------------------------------------------------------------------------------------------------ the fixture
@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_parity_through_the_public_classes(name):
    c = CASES[name]
    e = c["expected"]
    with torch.no_grad():
        out, bp = run_public(c, mv(c["inputs"]["x"]))
    assert out.dtype == torch.float32 and out.shape == e["x"].shape
    if c["op"] in ("max", "min"):
        assert torch.equal(out.cpu(), e["x"]), name
    torch.testing.assert_close(out.cpu(), e["x"], rtol=1e-5, atol=1e-5)  # (at most 64 rows per group in every case)
    if e["batch"] is None:
        assert bp is None
    else:
        assert torch.equal(bp.cpu(), e["batch"]), name
    # the float64 bound per (group, feature), through the restatement's own rows
    i = c["inputs"]
    ops = R.ops_of(c["op"], c["op_kwargs"])
    if "node_index" in i:
        src = i["x"].double()[i["node_index"]]
        if i["weight"] is not None:
            src = (i["x"][i["node_index"]] * i["weight"].view(-1, 1)).double()  # the product is rounded before the add
        check_against_f64(out, ops, src, i["cluster_index"], i["num_supernodes"], name)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_gradients(name):
    c = CASES[name]
    i = c["inputs"]
    x = mv(i["x"]).requires_grad_(True)
    w = None
    if i.get("weight") is not None:
        w = mv(i["weight"]).requires_grad_(True)
    out, _ = run_public(c, x, w)
    leaves = [x] + ([w] if w is not None else [])
    grads = torch.autograd.grad((out ** 2).sum(), leaves)
    torch.testing.assert_close(grads[0].cpu().double(), c["f64"]["grads"]["x"], rtol=1e-5, atol=1e-5)
    if w is not None:
        torch.testing.assert_close(grads[1].cpu().double(), c["f64"]["grads"]["weight"], rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------ contiguous segments
def segment_batch(longest):
    lengths = [0, 1, 2, 63, 64, 65, 0, longest]
    return torch.cat([torch.full((n,), g, dtype=torch.long) for g, n in enumerate(lengths)]), len(lengths) + 2


@pytest.mark.parametrize("split", [False, True], ids=["one_chunk", "split"])
@pytest.mark.parametrize("F", [1, 3, 32, 67, 260])
def test_segment_lengths_around_the_wave_and_the_chunk(F, split):
    chunk = K.segment_aggr_chunk_rows()
    batch, size = segment_batch(chunk + 1 if split else chunk)  # chunk + 1: the first length that takes the split route
    gen = torch.Generator().manual_seed(F)
    x = torch.randn(batch.numel(), F, generator=gen)
    reducer = AggrReduce(MultiAggregation(list(ALL4)))
    with torch.no_grad():
        out, bp = reducer(mv(x), batch=mv(batch), size=size)
        xi = torch.randint(-8, 9, x.shape, generator=gen).float()
        out_i, _ = reducer(mv(xi), batch=mv(batch), size=size)
    assert out.shape == (size, 4 * F) and torch.equal(bp.cpu(), torch.arange(size))
    check_against_f64(out, ALL4, x.double(), batch, size, f"F={F}")
    assert torch.equal(out_i.cpu(), R.aggregate(xi, batch, size, ALL4))  # integers: exact, the mean's division included
    assert bool((out[[0, 6, 8, 9]] == 0).all())  # graphs without nodes, the trailing groups of `size`


def test_row_strided_views_aligned_and_not():
    base = torch.randn(100, 40, generator=torch.Generator().manual_seed(5))
    batch = torch.arange(4).repeat_interleave(25)
    xd = mv(base)
    for first in (0, 1, 4):  # 16-byte aligned rows of stride 40; rows off by 4 bytes (scalar loads); aligned again
        with torch.no_grad():
            out = GlobalReduce("multi", aggrs=["sum", "max"])(xd[:, first:first + 32], batch=mv(batch))
        check_against_f64(out, ("sum", "max"), base[:, first:first + 32].double(), batch, 4, f"first column {first}")


# ------------------------------------------------------------------------------------------------ dense input
def dense_masks(B, N):
    prefix = torch.arange(N).view(1, -1) < torch.tensor([N, 33, 1]).view(-1, 1)
    holes = torch.rand(B, N, generator=torch.Generator().manual_seed(3)) < 0.5
    empty_row = holes.clone()
    empty_row[1] = False
    return {"none": None, "prefix": prefix, "holes": holes, "empty_row": empty_row}


@pytest.mark.parametrize("split", [False, True], ids=["one_chunk", "split"])
@pytest.mark.parametrize("F", [5, 8])
@pytest.mark.parametrize("which", ["none", "prefix", "holes", "empty_row"])
def test_dense_readout_reads_the_mask(which, F, split):
    B, N = 3, (K.segment_aggr_chunk_rows() + 44 if split else 70)
    mask = dense_masks(B, N)[which]
    x = torch.randn(B, N, F, generator=torch.Generator().manual_seed(7))
    xd = mv(x)
    if mask is not None:
        xd = torch.where(mv(mask).unsqueeze(-1), xd, torch.full_like(xd, float("nan")))  # a masked row is never read
    with torch.no_grad():
        out = GlobalReduce("multi", aggrs=list(ALL4))(xd, mask=mv(mask))
    keep = torch.ones(B * N, dtype=torch.bool) if mask is None else mask.reshape(-1)
    index = torch.arange(B).repeat_interleave(N)[keep]
    check_against_f64(out, ALL4, x.reshape(-1, F)[keep].double(), index, B, which)
    if which == "empty_row":
        assert bool((out[1] == 0).all())


# ------------------------------------------------------------------------------------------------ sparse assignments
def sparse_cases(F):
    gen = torch.Generator().manual_seed(11 + F)
    chunk = K.segment_aggr_chunk_rows()
    n = 2 * chunk + 40
    big = torch.randint(1, 5, (n,), generator=gen)
    big[torch.randperm(n, generator=gen)[:2 * chunk + 1]] = 0  # supernode 0 owns 2 * chunk + 1 nodes: three chunks
    return {
        "topk": dict(x=torch.randn(50, F, generator=gen), node_index=torch.randperm(50, generator=gen)[:20].sort().values,
                     cluster_index=torch.randperm(20, generator=gen), weight=torch.rand(20, generator=gen) + 0.1,
                     num_nodes=50, num_supernodes=20),
        "pairs": dict(x=torch.randn(40, F, generator=gen), node_index=torch.arange(40),
                      cluster_index=torch.arange(20).repeat(2)[torch.randperm(40, generator=gen)], weight=None,
                      num_nodes=40, num_supernodes=20),
        "empty_supernode": dict(x=torch.randn(30, F, generator=gen), node_index=torch.arange(30),
                                cluster_index=torch.tensor([0, 1, 3, 6])[torch.randint(0, 4, (30,), generator=gen)],
                                weight=torch.rand(30, generator=gen) + 0.1, num_nodes=30, num_supernodes=8),
        "split": dict(x=torch.randn(n, F, generator=gen), node_index=torch.arange(n), cluster_index=big,
                      weight=torch.rand(n, generator=gen) + 0.1, num_nodes=n, num_supernodes=5),
    }


@pytest.mark.parametrize("F", [5, 32])
@pytest.mark.parametrize("which", ["topk", "pairs", "empty_supernode", "split"])
def test_sparse_assignment_gathers_in_the_kernel(which, F):
    i = sparse_cases(F)[which]
    so = make_so(i)
    batch = torch.zeros(i["num_nodes"], dtype=torch.long)
    with torch.no_grad():
        out, bp = AggrReduce(MultiAggregation(list(ALL4)))(mv(i["x"]), so, batch=mv(batch))
    src = i["x"][i["node_index"]]
    if i["weight"] is not None:
        src = src * i["weight"].view(-1, 1)
    check_against_f64(out, ALL4, src.double(), i["cluster_index"], i["num_supernodes"], which)
    assert bp.shape == (i["num_supernodes"],)
    if which == "empty_supernode":
        assert bool((out[[2, 4, 5, 7]] == 0).all())


# ------------------------------------------------------------------------------------------------ properties
def test_multi_equals_the_three_single_calls():
    chunk = K.segment_aggr_chunk_rows()
    for longest in (40, chunk + 1):
        batch, size = segment_batch(longest)
        x = mv(torch.randn(batch.numel(), 32, generator=torch.Generator().manual_seed(13)))
        with torch.no_grad():
            multi = GlobalReduce("multi", aggrs=["sum", "mean", "max"])(x, batch=mv(batch), size=size)
            singles = [GlobalReduce(op)(x, batch=mv(batch), size=size) for op in ("sum", "mean", "max")]
            swapped = GlobalReduce("multi", aggrs=["max", "sum", "sum"])(x, batch=mv(batch), size=size)
        assert torch.equal(multi, torch.cat(singles, dim=-1))
        assert torch.equal(swapped, torch.cat([singles[2], singles[0], singles[0]], dim=-1))


def test_nan_propagates_as_in_amax():
    chunk = K.segment_aggr_chunk_rows()
    for longest in (40, chunk + 1):
        batch, size = segment_batch(longest)
        x = torch.randn(batch.numel(), 8, generator=torch.Generator().manual_seed(17))
        x[5, 2] = float("nan")  # a row of the 63-node graph
        x[-1, 3] = float("nan")  # the last row of the longest graph: the last chunk of the split route
        with torch.no_grad():
            out = GlobalReduce("multi", aggrs=list(ALL4))(mv(x), batch=mv(batch), size=size).cpu()
        want = R.aggregate(x, batch, size, ALL4)
        assert torch.equal(torch.isnan(out), torch.isnan(want))
        assert int(torch.isnan(out).sum()) == 8  # two entries, four operations
        for k, op in enumerate(ALL4):
            if op in ("max", "min"):
                torch.testing.assert_close(out[:, 8 * k:8 * k + 8], want[:, 8 * k:8 * k + 8], rtol=0, atol=0, equal_nan=True)


def test_two_calls_give_the_same_bits():
    chunk = K.segment_aggr_chunk_rows()
    batch, size = segment_batch(3 * chunk + 7)
    x = mv(torch.randn(batch.numel(), 32, generator=torch.Generator().manual_seed(19))).requires_grad_(True)
    runs = []
    for _ in range(2):
        out = GlobalReduce("multi", aggrs=list(ALL4))(x, batch=mv(batch), size=size)
        runs.append((out.detach().clone(), torch.autograd.grad((out ** 2).sum(), x)[0]))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    i = sparse_cases(32)["split"]
    w = mv(i["weight"]).requires_grad_(True)
    runs = []
    for _ in range(2):
        out, _ = AggrReduce(MultiAggregation(list(ALL4)))(x[: i["num_nodes"]], make_so(i, weight=w))
        runs.append((out.detach().clone(),) + torch.autograd.grad((out ** 2).sum(), [x, w]))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ------------------------------------------------------------------------------------------------ gradients with ties
def f64_grads(out_fn, leaves):
    leaves = [t.detach().double().cpu().requires_grad_(True) for t in leaves]
    return torch.autograd.grad((out_fn(*leaves) ** 2).sum(), leaves)


def assert_grad(got, want64, bound=None, what=""):
    """|got - want| <= 1e-6 |want| (+ ``bound``, per element, where the value is a float32 sum of several terms)."""
    err = (got.detach().cpu().double() - want64).abs()
    allowed = 1e-6 * want64.abs() + (0.0 if bound is None else bound)
    assert bool((err <= allowed).all()), f"{what}: max excess {(err - allowed).max().item():.3e}"


def per_op_grads(out_fn, leaves, ops):
    """Float64 gradients of sum(out ** 2) for every operation alone (the loss of a ``multi`` is their sum)."""
    return [f64_grads(lambda *t, op=op: out_fn(*t, (op,)), leaves) for op in ops]


@pytest.mark.parametrize("op", ["sum", "mean", "max", "min", "multi"])
def test_gradients_split_among_tied_rows(op):
    """Integer-valued x in [-2, 2]: every group has tied extremes and every sum is exact, so a single operation's dX is
    at most two float32 roundings from the float64 value (the mean's division, the division by the tie count or by the
    mean's count): the issue's rtol 1e-6, no atol.

    Two values are float32 SUMS of several terms that may cancel, so a relative bound alone cannot hold for them and
    an absolute term is added -- a departure from the issue's stated figure, per element and from the float64 terms,
    never from what the kernels give.  ``multi``: dX = sum of n terms t_k (one per operation), each within two
    roundings, added with n - 1 more: within (n + 1) U sum_k |t_k|.  d weight[a] = sum over F columns of d[a, f] x[f],
    a float32 dot product: within (F + 2 + n) U sum_f sum_k |d_k[a, f] x[f]|.  With a weight, dX carries one more
    product: (n + 2) U sum_k |t_k|."""
    ops = ALL4 if op == "multi" else (op,)
    kw = {"aggrs": list(ALL4)} if op == "multi" else {}
    n = len(ops)
    chunk = K.segment_aggr_chunk_rows()
    gen = torch.Generator().manual_seed(23)

    def multi_bound(parts, factor):  # parts: one float64 gradient per operation
        return None if n == 1 else factor * U * sum(p.abs() for p in parts)

    # contiguous segments, the split route included
    batch, size = segment_batch(chunk + 1)
    x = torch.randint(-2, 3, (batch.numel(), 8), generator=gen).float()
    xd = mv(x).requires_grad_(True)
    got = torch.autograd.grad((GlobalReduce(op, **kw)(xd, batch=mv(batch), size=size) ** 2).sum(), xd)[0]
    parts = [g[0] for g in per_op_grads(lambda t, o: R.aggregate(t, batch, size, o), [x], ops)]
    assert_grad(got, sum(parts), multi_bound(parts, n + 1), "segments")
    # dense with a mask with holes and an all-false row: one chunk, then the split route
    for nodes in (70, chunk + 44):
        mask = dense_masks(3, nodes)["empty_row"]
        x = torch.randint(-2, 3, (3, nodes, 5), generator=gen).float()
        xd = mv(x).requires_grad_(True)
        got = torch.autograd.grad((GlobalReduce(op, **kw)(xd, mask=mv(mask)) ** 2).sum(), xd)[0]
        parts = [g[0] for g in per_op_grads(lambda t, o: R.readout(t, o, mask=mask)[0], [x], ops)]
        assert_grad(got, sum(parts), multi_bound(parts, n + 1), f"dense N={nodes}")
        assert bool((got.cpu()[~mask] == 0).all())
    # sparse assignments with integer weights in {1, 2}: a supernode without members, then one on the split route
    for which in ("empty_supernode", "split"):
        i = dict(sparse_cases(8)[which])
        i["x"] = torch.randint(-2, 3, i["x"].shape, generator=gen).float()
        i["weight"] = torch.randint(1, 3, i["weight"].shape, generator=gen).float()
        xd, wd = mv(i["x"]).requires_grad_(True), mv(i["weight"]).requires_grad_(True)
        out, _ = AggrReduce(get_aggr(op, **kw))(xd, make_so(i, weight=wd))
        got = torch.autograd.grad((out ** 2).sum(), [xd, wd])

        def sparse64(t, w, o):
            return R.reduce_sparse(t, o, i["node_index"], i["cluster_index"], w, i["num_supernodes"])[0]

        parts = per_op_grads(sparse64, [i["x"], i["weight"]], ops)
        assert_grad(got[0], sum(p[0] for p in parts), multi_bound([p[0] for p in parts], n + 2), f"{which} dX")
        # d weight: the terms of its dot product, from d src = the gradient with respect to the weighted rows
        rows64 = i["x"].double()[i["node_index"]]

        def from_rows(src, o):
            return R.aggregate(src, i["cluster_index"], i["num_supernodes"], o)

        d_src = per_op_grads(from_rows, [rows64 * i["weight"].double().view(-1, 1)], ops)
        terms = sum((d[0] * rows64).abs() for d in d_src).sum(-1)
        assert_grad(got[1], sum(p[1] for p in parts), (8 + 2 + n) * U * terms, f"{which} d weight")


@pytest.mark.parametrize("op", ["max", "min"])
def test_gradient_of_an_extreme_that_is_exactly_zero(op):
    """Regression, found by the seeded family sweep (readout draws of one and two rows per group, integer-valued x): a
    group whose max / min is exactly 0.  The kernel's backward splits the gradient among the tied rows; the composed
    form (float64, unsorted batch vectors) and the restatement started ``scatter_reduce`` from zeros, whose backward
    counts that initial 0 as one more tied entry: the rows received 1 / (ties + 1).  All three routes now agree."""
    x = torch.tensor([[0.0, -1.0, 3.0], [0.0, 2.0, 3.0], [0.0, 5.0, -4.0]])
    batch = torch.tensor([0, 0, 1])
    first = [0.5, 0.0, 0.5] if op == "max" else [0.5, 1.0, 0.5]
    want = torch.tensor([first, [0.5, 1.0 - first[1], 0.5], [1.0, 1.0, 1.0]])
    order = torch.tensor([2, 0, 1])
    for name, xs, bs, ws in (("kernel", x, batch, want), ("float64", x.double(), batch, want.double()),
                             ("unsorted", x[order], batch[order], want[order])):
        xd = mv(xs).requires_grad_(True)
        out = GlobalReduce(op)(xd, batch=mv(bs), size=3)
        assert torch.equal(out.cpu(), R.scatter(xs, bs, 3, op)), name
        assert torch.equal(torch.autograd.grad(out.sum(), xd)[0].cpu(), ws), name
    x64 = x.double().requires_grad_(True)
    assert torch.equal(torch.autograd.grad(R.scatter(x64, batch, 3, op).sum(), x64)[0], want.double())


# ------------------------------------------------------------------------------------------------ routing
def test_dtype_and_order_routing():
    batch, size = segment_batch(40)
    x = torch.randn(batch.numel(), 8, generator=torch.Generator().manual_seed(29))
    g = GlobalReduce("multi", aggrs=list(ALL4))
    for dtype in (torch.float16, torch.bfloat16):  # fp32 arithmetic, the result in the input's dtype
        xh = x.to(dtype)
        out = g(mv(xh), batch=mv(batch), size=size)
        assert out.dtype == dtype
        want = R.aggregate(xh.float(), batch, size, ALL4).to(dtype)
        torch.testing.assert_close(out.cpu().float(), want.float(), rtol=2.0 ** -7, atol=2.0 ** -7)
    out64 = g(mv(x.double()), batch=mv(batch), size=size)  # float64: the composed torch form, in float64
    assert out64.dtype == torch.float64
    torch.testing.assert_close(out64.cpu(), R.aggregate(x.double(), batch, size, ALL4), rtol=1e-12, atol=1e-12)
    perm = torch.randperm(batch.numel(), generator=torch.Generator().manual_seed(31))
    out_u = g(mv(x[perm]), batch=mv(batch[perm]), size=size)  # an unsorted batch vector: the reference's sort, then the call
    check_against_f64(out_u, ALL4, x.double(), batch, size, "unsorted")
    agg = SumAggregation()
    torch.testing.assert_close(agg(mv(x), index=mv(batch), dim_size=size).cpu(), R.scatter(x, batch, size, "sum"),
                               rtol=1e-5, atol=1e-5)
    assert agg(mv(x)).shape == (1, 8) and agg(mv(x), index=mv(batch)).shape == (8, 8)


def test_a_reference_style_net_trains_one_step():
    from tgp.nn import GraphConv
    from tgp.poolers import get_pooler

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = GraphConv(16, 1)
            self.pool = get_pooler("topk", in_channels=16, ratio=0.5)
            self.readout = GlobalReduce(reduce_op="sum")
            self.lin = torch.nn.Linear(16, 3)

        def forward(self, x, edge_index, batch):
            h = x * torch.tanh(self.conv(x, edge_index))
            out = self.pool(x=h, adj=edge_index, batch=batch)
            return self.lin(self.readout(out.x, batch=out.batch))

    gen = torch.Generator().manual_seed(37)
    sizes = [12, 9, 15]
    batch = torch.cat([torch.full((n,), g) for g, n in enumerate(sizes)])
    x = torch.randn(sum(sizes), 16, generator=gen)
    blocks = torch.block_diag(*[(torch.rand(n, n, generator=gen) < 0.3).float() for n in sizes])
    edge_index = (blocks + blocks.t()).fill_diagonal_(0).nonzero().t().contiguous()
    net = Net().to(dev())
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    logits = net(mv(x), mv(edge_index), mv(batch))
    assert logits.shape == (3, 3)
    loss = torch.nn.functional.cross_entropy(logits, mv(torch.tensor([0, 1, 2])))
    loss.backward()
    before = [p.detach().clone() for p in net.parameters()]
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    opt.step()
    assert any(not torch.equal(a, b) for a, b in zip(before, net.parameters()))
