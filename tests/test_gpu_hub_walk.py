"""The hub route (csrc/hub_walk.hip) on the MI355X: every operator on one list with planted hazards against a float64
restatement (tests/fuzz_compare.py's rule), the non-hub rows and edges bit-equal to the one-wave entries on the full
index, arg-max positions exactly, the same bits with the index rebuilt and with the hub embedded in another list, and the
gradients of the ASAP fitness and the SAG scorer one path at a time.  The threshold is lowered by ``min_group``; hub
lengths are relative to the chunk the library reports.  Without the feature this module fails at the first wrapper."""
import copy

import pytest
import torch

import asap_restatement as R
from fuzz_compare import forward_errors
from test_gpu_grad_paths import check_grad_paths

from tgp import functions as Fn
from tgp import kernels as K
from tgp.poolers import ASAPooling, SAGPooling
from tgp.utils import add_remaining_self_loops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MG, N_NODES, SLOPE = 40, 48, 0.2
NAN_SRC = 33  # the x_pool row that is NaN in the query's case: a source of the last hub only


def hazard_list(extra=0):
    """(edge_index [2, E] unsorted, dst-groups' lengths): hubs of C + 1 (node 0), 2 C (node 1, adjacent), 2 C + 1 (node 20,
    its second chunk all out-of-range sources), MG + 1 (node 6), 65 C + 3 (node n - 1, with NAN_SRC in one chunk, a
    self-loop and duplicates); node 5 has exactly MG entries.  ``extra`` edges into node 9 come first: they shift every
    position without touching a hub group."""
    C, n = K.hub_chunk(), N_NODES
    g = torch.Generator().manual_seed(7)
    lens = {0: C + 1, 1: 2 * C, 20: 2 * C + 1, 6: MG + 1, 5: MG, n - 1: 65 * C + 3}
    src, dst = [torch.arange(extra) % 30], [torch.full((extra,), 9)]  # (no draw: the rest of the list stays as it is)
    for i in range(n):
        k = lens.get(i, 1 + i % 7)
        s = torch.randint(0, 32, (k,), generator=g)  # many duplicates; sources 32.. are planted below
        if i == 20:
            s[C:2 * C] = torch.tensor([n + 5, -1]).repeat(C // 2)
        if i == n - 1:
            s[3 * C + 5], s[70], s[71] = NAN_SRC, n - 1, n - 1
        src.append(s)
        dst.append(torch.full((k,), i))
    return torch.stack([torch.cat(src), torch.cat(dst)])


def index_with_plan(ei, reverse=(1,)):
    """The by-destination index of the list in its given order and the same index carrying the plan.  The entries of
    the nodes in ``reverse`` are reversed, so a later chunk holds the lower positions (ties must still go to them)."""
    order = torch.argsort(ei[1], stable=True)
    ptr = torch.zeros(N_NODES + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.bincount(ei[1], minlength=N_NODES), 0)
    for i in reverse:
        order[ptr[i]:ptr[i + 1]] = order[ptr[i]:ptr[i + 1]].flip(0)
    full = K.AssignIndex(ptr.to(torch.int32).to(DEV), order.to(torch.int32).to(DEV), ei.size(1), N_NODES)
    hubbed = K.AssignIndex(full.row_ptr, full.perm, full.nnz, N_NODES)
    hubbed.hub = K.build_hub_plan(hubbed, min_group=MG)
    assert hubbed.hub.hub_ids.tolist() == [0, 1, 6, 20, N_NODES - 1] and full.hub is None
    return full, hubbed


def inputs(f, strided, seed=1):
    g = torch.Generator().manual_seed(seed)
    wide = torch.randn(N_NODES, f + 5 if strided else f, generator=g)
    t = {"x": wide[:, :f], "wt": torch.randn(f, generator=g), "c": torch.randn(1, generator=g),
         "w3": torch.randn(3, f, generator=g), "g": torch.randn(N_NODES, f, generator=g)}
    for k in ("sq", "sp", "gq", "p1", "q", "bias"):
        t[k] = torch.randn(1 if k == "bias" else N_NODES, generator=g)
    t["x"][3] = t["x"][7]  # equal rows: bit-equal maxima in two chunks
    return t, g


def restate(ei, t, per_edge, dtype):
    """Every operator on the valid edges of the list in ``dtype`` on the CPU, outputs by name."""
    n, E = N_NODES, ei.size(1)
    c = {k: v.to(dtype) for k, v in {**t, **per_edge}.items()}
    ok = (ei[0] >= 0) & (ei[0] < n)
    pos, (src, dst) = ok.nonzero().view(-1), ei[:, ok]
    put = lambda v: torch.zeros(E, dtype=dtype).index_copy(0, pos, v)  # noqa: E731
    add = lambda idx, v: torch.zeros((n,) + v.shape[1:], dtype=dtype).index_add(0, idx, v)  # noqa: E731
    rows = c["x"][src]
    mx = R.scatter_max(rows, dst, n)
    hit = (rows == mx[dst]) | (rows.isnan() & mx[dst].isnan())
    arg = torch.full(mx.shape, E, dtype=torch.long).scatter_reduce(
        0, dst.view(-1, 1).expand_as(rows), torch.where(hit, pos.view(-1, 1), E), reduce="amin")
    out = {"argpos": arg, "sq": mx @ c["wt"] + c["c"]}
    logit = c["sq"][dst] + c["sp"][src]
    alpha = R.softmax(torch.nn.functional.leaky_relu(logit, SLOPE), dst, n)
    out["alpha"] = put(alpha)
    out["x_new"] = add(dst, rows * c["val"][pos].view(-1, 1))
    out["p"] = (out["x_new"] @ c["w3"].t()).t().contiguous()
    w = c["ew"][pos]
    s, wsum = add(dst, w * c["p1"][src]), add(dst, w)
    out["leconv"] = torch.sigmoid((c["q"] + c["bias"]) + s + (c["c"] - c["sp"]) * wsum)  # p = (p1, sp, q), b1 = c, b3 = bias
    size = torch.bincount(ei[1], minlength=n).clamp(min=1).to(dtype)
    out["sag"] = torch.tanh(add(dst, c["p1"][src]) / size + c["bias"] + c["q"])
    out["edge_dot"] = put((c["g"][dst] * rows).sum(-1))
    a, ga = c["val"][pos], c["ga"][pos]  # any alpha and g_alpha
    g_l = a * (ga - add(dst, a * ga)[dst]) * torch.where(logit > 0, 1.0, SLOPE).to(dtype)
    out["g_l"], out["g_sq"] = put(g_l), add(dst, g_l)
    match = (c["arg"][src] == pos.view(-1, 1)).to(dtype)  # the group's own index in the by-source role
    out["query_bwd"] = add(dst, match * c["gq"][src].view(-1, 1)) * c["wt"]
    return out


def run(grp, ei, t, per_edge):
    d = {k: v.to(DEV) for k, v in {**t, **per_edge}.items()}
    if not t["x"].is_contiguous():  # keep the row stride on the device
        wide = torch.zeros(N_NODES, t["x"].stride(0), device=DEV)
        wide[:, :t["x"].size(1)] = d["x"]
        d["x"] = wide[:, :t["x"].size(1)]
    src = ei[0].to(DEV)
    sq, arg = K.asap_query(grp, src, d["x"], d["wt"], d["c"], want_arg=True)
    x_new, p = K.asap_attend(grp, src, d["x"], d["val"], d["w3"])
    g_l, g_sq = K.asap_softmax_bwd(grp, src, d["val"], d["ga"], d["sq"], d["sp"], SLOPE)
    return {"argpos": arg, "sq": sq, "alpha": K.asap_edge_softmax(grp, src, d["sq"], d["sp"], SLOPE), "x_new": x_new,
            "p": p, "leconv": K.asap_leconv(grp, src, torch.stack([d["p1"], d["sp"], d["q"]]), d["ew"], d["c"], d["bias"],
                                            "sigmoid"),
            "sag": K.sag_aggregate(grp, src, d["p1"], d["q"], d["bias"], mean=True, tanh=True),
            "edge_dot": K.asap_edge_dot(grp, src, d["g"], d["x"]), "g_l": g_l, "g_sq": g_sq,
            "query_bwd": K.asap_query_bwd(grp, src, d["arg"], d["gq"], d["wt"])}


PER_EDGE = ("alpha", "edge_dot", "g_l")


@pytest.mark.parametrize("f,strided", [(1, False), (5, False), (64, False), (67, True), (260, False)])
def test_every_operator_on_the_hazard_list(f, strided):
    ei = hazard_list()
    full, hubbed = index_with_plan(ei)
    t, g = inputs(f, strided)
    E = ei.size(1)
    per_edge = {"val": torch.rand(E, generator=g), "ga": torch.randn(E, generator=g), "ew": torch.rand(E, generator=g) + 0.1}
    r32 = restate(ei, t, {**per_edge, "arg": torch.zeros(N_NODES, f, dtype=torch.long)}, torch.float32)
    per_edge["arg"] = r32["argpos"].clamp(max=E - 1).to(torch.int32)  # a real arg-max table for query_bwd
    r64, r32 = restate(ei, t, per_edge, torch.float64), restate(ei, t, per_edge, torch.float32)
    for r in (r64, r32):
        r["argpos"] = torch.where(r["argpos"] == E, -1, r["argpos"])
    got, one_wave = run(hubbed, ei, t, per_edge), run(full, ei, t, per_edge)
    fails = forward_errors(f"hub/F={f}", got, r64, r32, exact=("argpos",), exact_ref=r32)
    assert not fails, "\n".join(fails)
    hub_node = torch.zeros(N_NODES, dtype=torch.bool)
    hub_node[hubbed.hub.hub_ids.long().cpu()] = True
    for name, have in got.items():  # what the light run wrote is what the one-wave entry writes on the full index
        rest = ~hub_node[ei[1]] if name in PER_EDGE else ~hub_node
        a, b = have.cpu(), one_wave[name].cpu()
        a, b = (a[:, rest], b[:, rest]) if name == "p" else (a[rest], b[rest])
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), name
    assert torch.equal(got["alpha"][ei[0].to(DEV) >= N_NODES], torch.zeros(K.hub_chunk() // 2, device=DEV))


def test_a_nan_row_in_one_chunk_wins_its_hub_and_nothing_else():
    ei = hazard_list()
    _, hubbed = index_with_plan(ei)
    t, _ = inputs(5, False)
    t["x"][NAN_SRC, 2] = float("nan")
    d = {k: v.to(DEV) for k, v in t.items()}
    sq, arg = K.asap_query(hubbed, ei[0].to(DEV), d["x"], d["wt"], d["c"], want_arg=True)
    last = N_NODES - 1
    where = ((ei[1] == last) & (ei[0] == NAN_SRC)).nonzero().view(-1)
    assert bool(sq[last].isnan()) and bool(torch.isfinite(sq[:last]).all()) and arg[last, 2].item() == where.min().item()


def test_the_bits_do_not_depend_on_the_call_or_on_the_rest_of_the_list():
    """Run to run with index and plan rebuilt, and the same hub groups embedded in a list with 7 more edges in front."""
    t, g = inputs(67, True)
    outs = []
    for extra in (0, 0, 7):
        ei = hazard_list(extra)
        _, hubbed = index_with_plan(ei)
        E = ei.size(1)
        g = torch.Generator().manual_seed(5)
        tail = {k: torch.rand(E - extra, generator=g) + 0.1 for k in ("val", "ga", "ew")}
        per_edge = {k: torch.cat([torch.ones(extra), v]) for k, v in tail.items()}
        per_edge["arg"] = torch.randint(0, 40, (N_NODES, 67), generator=g).to(torch.int32) + extra
        got = run(hubbed, ei, t, per_edge)
        hubs = hubbed.hub.hub_ids.long()
        on_hub = torch.isin(ei[1].to(DEV), hubs)
        outs.append({k: (v[on_hub] if k in PER_EDGE else v[:, hubs] if k == "p" else v[hubs]) for k, v in got.items()})
        outs[-1]["argpos"] = outs[-1]["argpos"] - extra
    for other in outs[1:]:
        for k, v in outs[0].items():
            assert torch.equal(v.contiguous().view(torch.int32), other[k].contiguous().view(torch.int32)), k


def in_and_out_hub(n=300):
    """Node 0 is the destination of 2 C + 9 edges and the source of as many: both by-destination and by-source plans."""
    k = 2 * K.hub_chunk() + 9
    g = torch.Generator().manual_seed(2)
    far = torch.randint(1, n, (k,), generator=g)
    ring = torch.arange(n)
    return torch.cat([torch.stack([far, torch.zeros(k, dtype=torch.long)]), torch.stack([torch.zeros(k, dtype=torch.long), far]),
                      torch.stack([ring, (ring + 1) % n])], 1), n


def test_gradients_through_both_hubs_one_path_at_a_time(monkeypatch):
    monkeypatch.setattr(K, "HUB_MIN_GROUP", MG)
    ei, n = in_and_out_hub()
    torch.manual_seed(4)
    state = {k: v.clone() for k, v in ASAPooling(8).state_dict().items()}
    x0 = torch.randn(n, 8, generator=torch.Generator().manual_seed(6))
    names = sorted(state)

    def asap():
        p = ASAPooling(8).to(DEV)
        p.load_state_dict(state)
        x, e = x0.to(DEV).requires_grad_(True), ei.to(DEV)
        _, x_new, score = p.fitness(x, e, None, mask=None, act="sigmoid")
        assert all(K.sag_edge_group(e, n, by_destination=b).hub.H == 1 for b in (True, False))
        return {"x_new": x_new, "score": score}, {"x": x, **{k: dict(p.named_parameters())[k] for k in names}}

    def asap_oracle(dtype):
        x = x0.to(dtype).requires_grad_(True)
        par = {k: v.to(dtype).requires_grad_(True) for k, v in state.items()}
        _, x_new, fit = R.fitness_reference_shaped(x, x, ei, None, par, 0.2, None)
        return {"x_new": x_new, "score": torch.sigmoid(fit)}, {"x": x, **par}

    check_grad_paths("hub/asap", asap, asap_oracle, ["x"] + names)
    w0 = torch.randn(3, 8, generator=torch.Generator().manual_seed(8))

    def leaves(dtype, dev):
        return [v.to(dev, dtype).requires_grad_(True) for v in (x0, w0[0], w0[1], w0[2, :1])]

    def sag():
        x, w_rel, w_root, b = leaves(torch.float32, DEV)
        return {"score": Fn.sag_score(x, ei.to(DEV), w_rel, w_root, b, True, True)}, dict(x=x, w_rel=w_rel, w_root=w_root, b=b)

    def sag_oracle(dtype):
        x, w_rel, w_root, b = leaves(dtype, "cpu")
        size = torch.bincount(ei[1], minlength=n).clamp(min=1).to(dtype)
        agg = torch.zeros(n, dtype=dtype).index_add(0, ei[1], (x @ w_rel)[ei[0]]) / size
        return {"score": torch.tanh(agg + b + x @ w_root)}, dict(x=x, w_rel=w_rel, w_root=w_root, b=b)

    check_grad_paths("hub/sag", sag, sag_oracle, ["x", "w_rel", "w_root", "b"])


@pytest.mark.parametrize("cls", [ASAPooling, SAGPooling])
def test_the_public_classes_take_the_hub_route_and_match_their_composed_form(cls, monkeypatch):
    """Forward and ``loss.backward()`` of the pooler on the in-hub / out-hub graph with the threshold lowered, against
    the same module in float64 (which takes the composed form): selections exactly, values and gradients at the
    fixture tolerance.  The indices the native run built carry a plan."""
    monkeypatch.setattr(K, "HUB_MIN_GROUP", MG)
    ei, n = in_and_out_hub()
    torch.manual_seed(9)
    native = cls(in_channels=8, ratio=0.5).to(DEV)
    composed = copy.deepcopy(native).double()
    x0, e = torch.randn(n, 8, generator=torch.Generator().manual_seed(10)), ei.to(DEV)
    got = []
    for p, dtype in ((native, torch.float32), (composed, torch.float64)):
        x = x0.to(DEV, dtype).requires_grad_(True)
        out = p(x=x, adj=e)
        (out.x ** 2).sum().backward()
        got.append((out, x.grad, [q.grad for q in p.parameters()]))
        if p is native:
            indexed = add_remaining_self_loops(e, None, num_nodes=n)[0] if cls is ASAPooling else e
            memo = K._SAG_GROUPS.get(indexed)
            assert memo is not None and all(memo[(n, by_dst)].hub.H == 1 for by_dst in (True, False))
    (o32, gx32, gp32), (o64, gx64, gp64) = got
    assert torch.equal(o32.so.node_index, o64.so.node_index) and torch.equal(o32.edge_index, o64.edge_index)
    close = lambda a, b: torch.testing.assert_close(a.double(), b, rtol=1e-5, atol=1e-5)  # noqa: E731
    close(o32.x, o64.x)
    close(o32.so.weight, o64.so.weight)
    close(gx32, gx64)
    for a, b in zip(gp32, gp64):
        assert (a is None) == (b is None)
        if a is not None:
            close(a, b)
