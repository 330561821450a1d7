#!/usr/bin/env python3
"""Generate the golden vectors of the reference's NON-FINITE behaviour (``tests/golden/golden_nonfinite_v1.pt``).

TEST INFRASTRUCTURE ONLY — run in the BUILD container, never on the GPU box.

Same recipe as ``make_golden.py``: the real reference (tgp 1.0.1) over the PyG stand-in runs its own ``sparse_connect``,
``postprocess_adj_pool_dense`` / ``_sparse``, loss functions and ``TopkSelect`` on tiny inputs (N <= 12, K <= 4) that
hold a NaN, an infinity or both infinities in one reduction.  Only the data file travels.

What is pinned is where torch propagates a NaN: ``clamp``, ``max``, ``amax`` / ``amin``, ``norm``, ``softmax`` and the
sums.  One PyG leaf takes part in that rule: ``coalesce(reduce="min" / "max")`` goes through ``scatter``, which PyG maps
to ``Tensor.scatter_reduce_(reduce="amin" / "amax", include_self=False)``; ``pyg_shim.scatter`` carries exactly that
mapping, so a NaN merged with finite duplicates comes out NaN here as it does under PyG.  The limit README.md states
for every "bit-exact" claim applies: a shared misreading of a leaf would pass both sides.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nonfinite.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import torch  # noqa: E402

import make_golden as G  # noqa: E402  (installs the stand-in and imports the reference)
from tgp.connect import sparse_connect  # noqa: E402
from tgp.select import TopkSelect  # noqa: E402
from tgp.utils import losses as RL  # noqa: E402
from tgp.utils.ops import postprocess_adj_pool_dense, postprocess_adj_pool_sparse  # noqa: E402

NAN, INF = float("nan"), float("inf")
CASES = {}
FLAGS = {"plain": dict(remove_self_loops=False, degree_norm=False, edge_weight_norm=False),
         "flags": dict(remove_self_loops=True, degree_norm=True, edge_weight_norm=True)}


def gen_connect():
    """8 nodes -> 4 supernodes (two graphs of two).  Groups of the coalesce, by (row, col) of the supernodes:
    (0,1) a NaN merged with two finite duplicates; (1,0) a lone NaN; (2,3) +inf and -inf with a finite one;
    (3,2) a lone +inf; (0,0) / (3,3) self loops; the rest finite, one of them a group of two."""
    cluster = torch.tensor([0, 0, 1, 1, 2, 2, 3, 3])
    ei = torch.tensor([[0, 1, 0, 2, 4, 5, 4, 6, 0, 7, 2, 3, 6, 5],
                       [2, 3, 3, 0, 6, 7, 7, 4, 1, 6, 3, 1, 5, 4]])
    ew = torch.tensor([0.5, NAN, 1.5, NAN, INF, -INF, 0.75, INF, 0.25, 1.25, 2.0, 0.5, 0.6, 0.9])
    batch_pooled = torch.tensor([0, 0, 1, 1])
    for op in ("sum", "mean", "min", "max", "mul"):
        exp = {}
        for tag, flags in FLAGS.items():
            oi, ow = sparse_connect(ei, ew, node_index=torch.arange(8), cluster_index=cluster, num_nodes=8,
                                    num_supernodes=4, reduce_op=op, batch_pooled=batch_pooled, **flags)
            exp[tag + "_ei"], exp[tag + "_ew"] = G.t(oi), G.t(ow)
        CASES[f"connect_{op}"] = {"inputs": dict(edge_index=ei, edge_weight=ew, cluster_index=cluster,
                                                 batch_pooled=batch_pooled, num_supernodes=4),
                                  "cfg": dict(reduce_op=op), "expected": exp}


def gen_postprocess():
    g = torch.Generator().manual_seed(1)
    a = torch.rand(3, 4, 4, generator=g) + 0.1
    a[0, 1, 2] = NAN                      # a NaN entry
    a[1, 2, 0], a[1, 2, 3] = INF, -INF    # a row whose sum is inf - inf
    a[2, 3] = torch.tensor([-2.0, 0.5, -1.0, 0.25])  # a negative row sum: clamp(min=eps)
    exp = {}
    for rsl in (True, False):
        for dn in (True, False):
            for at in (True, False):
                for ewn in (True, False):
                    o = postprocess_adj_pool_dense(a.clone(), rsl, dn, at, ewn)
                    exp[f"rsl{int(rsl)}_dn{int(dn)}_at{int(at)}_ewn{int(ewn)}"] = G.t(o)
    CASES["postprocess_dense"] = {"inputs": dict(adj_pool=a), "cfg": {}, "expected": exp}

    # the sparse twin on 6 supernodes in two graphs: row 0 holds a NaN, row 2 both infinities, row 4 sums below zero
    ei = torch.tensor([[0, 0, 1, 1, 2, 2, 2, 3, 4, 4, 5, 5],
                       [1, 2, 0, 1, 0, 1, 2, 5, 3, 5, 4, 3]])
    ew = torch.tensor([NAN, 0.5, 1.5, 0.25, INF, -INF, 1.0, 2.0, -3.0, 0.5, 0.75, 1.25])
    bp = torch.tensor([0, 0, 0, 1, 1, 1])
    exp = {}
    for rsl in (True, False):
        for dn in (True, False):
            for ewn in (True, False):
                oi, ow = postprocess_adj_pool_sparse(ei, ew, num_nodes=6, remove_self_loops=rsl, degree_norm=dn,
                                                     edge_weight_norm=ewn, batch_pooled=bp)
                key = f"rsl{int(rsl)}_dn{int(dn)}_ewn{int(ewn)}"
                exp[key + "_ei"], exp[key + "_ew"] = G.t(oi), G.t(ow)
    CASES["postprocess_sparse"] = {"inputs": dict(edge_index=ei, edge_weight=ew, batch_pooled=bp, num_nodes=6),
                                   "cfg": {}, "expected": exp}


def gen_losses():
    """The four dense losses on [2, 6, .] tensors and their sparse / unbatched forms on the same two graphs."""
    g = torch.Generator().manual_seed(2)
    B, N, K = 2, 6, 3
    s0 = torch.softmax(torch.randn(B, N, K, generator=g), -1)
    up = torch.triu((torch.rand(B, N, N, generator=g) < 0.5).float() * (torch.rand(B, N, N, generator=g) + 0.1), 1)
    a0 = up + up.transpose(1, 2)
    for tag in ("nan_in_s", "inf_in_adj"):
        s, a = s0.clone(), a0.clone()
        if tag == "nan_in_s":
            s[0, 4, 1] = NAN
        else:
            a[1, 2, 3] = a[1, 3, 2] = INF
        raw = torch.matmul(torch.matmul(s.transpose(1, 2), a), s)
        exp = {"mincut": G.t(RL.mincut_loss(a, s, raw)), "ortho": G.t(RL.orthogonality_loss(s)),
               "link": G.t(RL.link_pred_loss(s, a, normalize_loss=False)),
               "link_normalized": G.t(RL.link_pred_loss(s, a, normalize_loss=True)),
               "entropy": G.t(RL.entropy_loss(s, B * N))}
        b, r, c = a.nonzero(as_tuple=True)  # (an infinite entry is an edge of infinite weight)
        ei, ew = torch.stack([r + b * N, c + b * N]), a[b, r, c]
        batch = torch.arange(B).repeat_interleave(N)
        sf = s.reshape(B * N, K)
        exp.update(sparse_mincut=G.t(RL.sparse_mincut_loss(ei, sf, ew, batch)),
                   unbatched_ortho=G.t(RL.unbatched_orthogonality_loss(sf, batch)),
                   sparse_link=G.t(RL.sparse_link_pred_loss(sf, ei, ew, batch, normalize_loss=False)),
                   unbatched_entropy=G.t(RL.unbatched_entropy_loss(sf, B * N)))
        CASES[f"losses_{tag}"] = {"inputs": dict(s=s, adj=a, edge_index=ei, edge_weight=ew, batch=batch),
                                  "cfg": {}, "expected": exp}


def gen_topk():
    score = torch.tensor([0.5, INF, -1.0, NAN, -INF, 0.5, 2.0, -0.0, 0.0])
    batch = torch.tensor([0, 0, 0, 0, 0, 1, 1, 1, 1])
    for tag, cfg in (("ratio_half", dict(ratio=0.5)), ("ratio_two", dict(ratio=2)), ("min_score", dict(min_score=0.2))):
        so = TopkSelect(in_channels=None, act="linear", **cfg)(score.clone(), batch=batch)
        CASES[f"topk_{tag}"] = {"inputs": dict(score=score, batch=batch), "cfg": cfg,
                                "expected": dict(node_index=G.t(so.node_index), cluster_index=G.t(so.cluster_index),
                                                 weight=G.t(so.weight), num_supernodes=so.num_supernodes)}


def main():
    gen_connect()
    gen_postprocess()
    gen_losses()
    gen_topk()
    for name, c in CASES.items():
        c["inputs"] = {k: G.t(v) for k, v in c["inputs"].items()}
        n = sum(int((~torch.isfinite(v)).sum()) for v in c["expected"].values()
                if isinstance(v, torch.Tensor) and v.is_floating_point())
        print(f"{name}: {len(c['expected'])} outputs, {n} non-finite entries")
    out = os.path.join(HERE, "golden_nonfinite_v1.pt")
    torch.save({"tgp_version": G.tgp.__version__, "torch": str(torch.__version__), "cases": CASES}, out)
    print(f"wrote {len(CASES)} cases -> {out} ({os.path.getsize(out) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
