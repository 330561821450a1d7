"""MaxCut's hub route (csrc/maxcut_hub.hip) on the MI355X: the layer on a hazard list against float64 (fuzz_compare's
rule) and bit for bit against the one-wave entry, the other index form and a shifted list; the rounds exactly against the
composed routine; the public classes native on a hub.  ``min_group`` lowers the threshold, lengths follow the chunk."""
import pytest
import torch

import maxcut_restatement as R
from fuzz_compare import forward_errors
from test_gpu_grad_paths import check_grad_paths
from test_gpu_maxcut import Routes, composed_labels, selection

from tgp import kernels as K
from tgp.poolers import MaxCutPooling, MaxCutSelect

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MG, N_NODES, N_P, DELTA, NAN_SRC, HUBS = 40, 48, 45, 1.5, 33, [0, 1, 6, 7, 20, 46, 47]


def hazard_list(extra=0):
    """Shuffled [2, E] list.  In-groups: node 0 C + 1, node 1 2 C, node 20 2 C + 1 (second chunk all out-of-range), node 6
    C + MG + 1 (first chunk self-loops only), node 7 MG + 2 (self-loops and invalid only), node 46 MG + 3 and node 47
    65 C + 3 with NAN_SRC (both at or above N_P), node 5 exactly MG; duplicates abound.  ``extra`` edges into node 9 first."""
    C, n, g = K.hub_chunk(), N_NODES, torch.Generator().manual_seed(7)
    lens = {0: C + 1, 1: 2 * C, 20: 2 * C + 1, 6: C + MG + 1, 7: MG + 2, 46: MG + 3, 5: MG, n - 1: 65 * C + 3}
    src, dst = [], []
    for i in range(n):
        k = lens.get(i, 1 + i % 7)
        s = torch.randint(0, 32, (k,), generator=g)
        if i == 20:
            s[C:2 * C] = torch.tensor([n + 5, -1]).repeat(C // 2)
        if i == 6:
            s[:C] = 6
        if i == 7:
            s[:] = torch.tensor([7, -1]).repeat(k // 2)
        if i == n - 1:
            s[3 * C + 5], s[70] = NAN_SRC, n - 1
        src.append(s)
        dst.append(torch.full((k,), i))
    ei = torch.stack([torch.cat(src), torch.cat(dst)])
    ei = ei[:, torch.randperm(ei.size(1), generator=g)]
    return torch.cat([torch.stack([torch.arange(extra) % 30, torch.full((extra,), 9)]), ei], 1)


def indices(ei, coef, sort):
    """(list, coef, full index, the index with its plan): as it is (permutation) or stably sorted (offsets only)."""
    order = torch.argsort(ei[1], stable=True)
    ptr = torch.zeros(N_NODES + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.bincount(ei[1], minlength=N_NODES), 0)
    if sort:
        ei, coef = ei[:, order], coef[order]
    perm = None if sort else order.to(torch.int32).to(DEV)
    full = K.AssignIndex(ptr.to(torch.int32).to(DEV), perm, ei.size(1), N_NODES)
    hubbed = K.AssignIndex(full.row_ptr, perm, full.nnz, N_NODES)
    hubbed.hub = K.build_hub_plan(hubbed, min_group=MG)
    return ei, coef, full, hubbed


def restate(ei, coef, t, act, dtype):
    c = {k: v.to(dtype) for k, v in t.items()}
    ok = (ei[0] >= 0) & (ei[0] < N_NODES) & (ei[0] != ei[1])
    src, dst = ei[:, ok]
    agg = torch.zeros_like(c["z"]).index_add(0, dst, c["z"][src] * coef[ok].to(dtype).view(-1, 1))
    has = (torch.bincount(dst, minlength=N_NODES) > 0).view(-1, 1)  # no entry: no off-diagonal term at all
    below = (torch.arange(N_NODES) < N_P).view(-1, 1)
    pre = torch.where(below, (1 - DELTA) * c["z"], 0) + torch.where(has, (DELTA * c["dinv"]).view(-1, 1) * agg, 0)
    out = {"h": R.ACTS[act](pre + c["b"])}
    if "wn" in c:
        out["z_next"] = out["h"] @ c["wn"].t()
    return out


def run(grp, ei, coef, t, act):
    d = {k: v.to(DEV) for k, v in t.items()}
    h, zn = K.maxcut_layer(grp, ei[0].to(DEV), coef.to(DEV), d["dinv"], d["z"], d["b"],
                           torch.tensor([N_P], device=DEV), DELTA, act, d.get("wn"))
    return {"h": h, "z_next": zn} if zn is not None else {"h": h}


@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("sort", [True, False], ids=["offsets", "permutation"])
@pytest.mark.parametrize("C,Cn", [(1, 1), (5, 3), (32, 33), (33, 64), (64, None)])
def test_the_layer_on_the_hazard_list(C, Cn, sort, act):
    g = torch.Generator().manual_seed(C)
    t = {"z": torch.randn(N_NODES, C, generator=g), "b": torch.randn(C, generator=g) * 0.5,
         "dinv": torch.rand(N_NODES, generator=g) + 0.2, **({"wn": torch.randn(Cn, C, generator=g)} if Cn else {})}
    t["z"][NAN_SRC], t["dinv"][7] = float("nan"), float("nan")
    bits = lambda v, rows: v[rows].contiguous().view(torch.int32)  # noqa: E731
    hub_rows = {}
    for extra, srt in ((0, sort), (0, not sort), (100, False)):
        ei = hazard_list(extra)
        coef = torch.cat([torch.ones(extra), torch.rand(ei.size(1) - extra, generator=torch.Generator().manual_seed(5)) + 0.1])
        ei, coef, full, hubbed = indices(ei, coef, srt)
        assert hubbed.hub.hub_ids.tolist() == sorted(HUBS + [9] * (extra > 0)) and full.hub is None
        got = run(hubbed, ei, coef, t, act)
        hub_rows[(extra, srt)] = {k: bits(v, HUBS) for k, v in got.items()}
        if (extra, srt) != (0, sort):
            continue
        r64, r32 = restate(ei, coef, t, act, torch.float64), restate(ei, coef, t, act, torch.float32)
        fails = forward_errors(f"mchub/C={C}", got, r64, r32)
        assert not fails, "\n".join(fails)
        one_wave, rest = run(full, ei, coef, t, act), [i for i in range(N_NODES) if i not in HUBS]
        for k, v in got.items():
            assert torch.equal(v.isnan().cpu(), r64[k].isnan()), k
            assert torch.equal(bits(v, rest), bits(one_wave[k], rest)), k  # what the light run wrote
        h = got["h"].cpu()  # the NaN source reaches its hub; the NaN dinv of node 7 does not: the empty group's value
        assert bool(h[N_NODES - 1].isnan().all())  # (the pre-activation is exact, tanhf is within 2 ulp)
        torch.testing.assert_close(h[7], R.ACTS[act]((1 - DELTA) * t["z"][7] + t["b"]), rtol=0, atol=2.0 ** -20)
    for other in ((0, not sort), (100, False)):  # the bits depend on the group alone
        for k, v in hub_rows[(0, sort)].items():
            assert torch.equal(v, hub_rows[other][k]), (other, k)


def vote_list():
    """Kept nodes 0 .. 9 carry labels 1 .. 10, nodes 30 and 31 never get one.  Hub 20: label 3 wins its first chunk (100
    to 70), label 7 its second (90 to 60), label 5 wins summed (130).  Hub 21: labels 4 and 2 tie at 70 in different
    chunks.  Hub 5 is kept, hub 22 has no labelled source, hub 23 gets label 8 in round 1 and feeds hub 24 in round 2."""
    C = K.hub_chunk()
    rep = lambda *pairs: torch.cat([torch.full((k,), s) for s, k in pairs])  # noqa: E731
    groups = {20: rep((2, 100), (4, 70), (30, C - 170), (6, 90), (4, 60), (31, 10)),
              21: rep((3, 70), (30, C - 70), (1, 70), (31, 5)), 5: rep((0, C + 5)), 22: rep((30, C), (31, 9)),
              23: rep((7, C + 1)), 24: rep((30, 3), (23, C + 3)), 40: rep((9, 2), (8, 1)), 41: rep((40, 1))}
    order = sorted(groups, reverse=True)  # descending destinations: the index needs its permutation
    dst = torch.cat([torch.full((groups[i].numel(),), i) for i in order])
    return torch.arange(10), torch.stack([torch.cat([groups[i] for i in order]), dst]), 48


@pytest.mark.parametrize("rounds", [1, 3])
def test_assignment_rounds_on_the_vote_list(rounds):
    kept, d, n = (v.to(DEV) if torch.is_tensor(v) else v for v in vote_list())
    by_dst = K.sag_edge_group(d, n, by_destination=True)
    hubbed = K.AssignIndex(by_dst.row_ptr, by_dst.perm, by_dst.nnz, n)
    hubbed.hub = K.build_hub_plan(hubbed, min_group=MG)
    assert by_dst.perm is not None and by_dst.hub is None and hubbed.hub.hub_ids.tolist() == [5, 20, 21, 22, 23, 24]
    labels = torch.cat([torch.arange(1, 11), torch.zeros(n - 10, dtype=torch.long)]).to(DEV, torch.int32)
    got = K.maxcut_assign_rounds(hubbed, d[0].contiguous(), labels, rounds, 10).long()
    assert torch.equal(got, composed_labels(kept, d, n, rounds))
    assert got[[5, 20, 21, 22, 23, 24, 40, 41]].tolist() == [6, 5, 2, 0, 8, 8 if rounds > 1 else 0, 10, 10 if rounds > 1 else 0]
    assert torch.equal(got, K.maxcut_assign_rounds(hubbed, d[0].contiguous(), labels, rounds).long())  # K read from the labels


def star_graph(n=4300):
    """Node 0 is the destination and the source of HUB_MIN_GROUP + 5 edges; three random in-edges for every node."""
    k, g = K.HUB_MIN_GROUP + 5, torch.Generator().manual_seed(2)
    far, zero = torch.arange(1, k + 1), torch.zeros(k, dtype=torch.long)
    rest = torch.stack([torch.randint(0, n, (3 * n,), generator=g), torch.arange(n).repeat(3)])
    ei = torch.cat([torch.stack([far, zero]), torch.stack([zero, far]), rest], 1)
    return ei[:, torch.randperm(ei.size(1), generator=g)].contiguous(), n


def test_the_public_classes_stay_native_on_a_graph_with_a_hub():
    (ei, n), cfg = star_graph(), dict(mp_units=[33, 16, 5], mlp_units=[8])
    d, w0 = ei.to(DEV), torch.rand(ei.size(1), generator=torch.Generator().manual_seed(5)) + 0.1
    x0 = torch.randn(n, 6, generator=torch.Generator().manual_seed(7))
    torch.manual_seed(3)
    state = {k: v.clone() for k, v in MaxCutPooling(6, **cfg).state_dict().items()}

    def kernel():
        p = MaxCutPooling(6, **cfg)
        p.load_state_dict(state)
        p, x = p.to(DEV), x0.to(DEV).requires_grad_(True)
        with Routes() as r:
            s = p.selector.score_net(x, d, w0.to(DEV)).view(-1)
        assert r.score == 1, "the score net left the kernels on a hub"
        assert all(K.sag_edge_group(d, n, by_destination=b).hub.H == 1 for b in (True, False))
        return {"scores": s}, {"x": x, **dict(p.named_parameters())}

    def oracle(dtype):
        par = {k: v.to(dtype).requires_grad_(True) for k, v in state.items()}
        x = x0.to(dtype).requires_grad_(True)
        return {"scores": R.scores_reference_shaped(par, cfg, x, ei, w0.to(dtype))}, {"x": x, **par}

    check_grad_paths("maxcut/star", kernel, oracle, ["x"] + sorted(state))
    x0, runs = x0.detach(), []  # (the float32 oracle made x0 itself a leaf)
    for _ in range(2):  # two training calls: identical bits
        outs, leaves = kernel()
        (outs["scores"] * torch.linspace(-1, 1, n, device=DEV)).sum().backward()
        runs.append([outs["scores"].detach()] + [v.grad for v in leaves.values()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    composed = MaxCutPooling(6, **cfg)
    composed.load_state_dict(state)
    with torch.no_grad():  # the scores against the composed form in float64
        want = composed.double().to(DEV).selector.score_net(x0.to(DEV).double(), d, w0.to(DEV).double()).view(-1)
    torch.testing.assert_close(runs[0][0].double(), want, rtol=1e-5, atol=1e-5)
    kept = torch.arange(10, n, 5, device=DEV)
    with Routes() as r:
        got = MaxCutSelect(4, mp_units=[4], mlp_units=[]).assign(selection(kept, n), d, None,
                                                                 torch.zeros(n, dtype=torch.long, device=DEV), 3)
    assert r.rounds == 1, "the assignment left the kernels on a hub"
    reached = composed_labels(kept, d, n, 3)
    assert int(reached[0]) > 0 and torch.equal(got.cluster_index[reached > 0], reached[reached > 0] - 1)
