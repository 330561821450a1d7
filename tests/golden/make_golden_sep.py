#!/usr/bin/env python3
"""Generate the golden vectors of SEP pooling (``tests/golden/golden_sep_v1.pt``).

TEST INFRASTRUCTURE ONLY -- run in the BUILD container on the CPU, never on the GPU box.

Same recipe as ``make_golden_kmis.py``: the real reference (tgp 1.0.1) over the PyG stand-in runs ``SEPPooling`` on small
seeded inputs.  The reference's decisions are comparisons of float64 sums, and its singleton order is Python's ``set``
order, so a case is kept only if
  (a) the float64 restatement (``tests/sep_restatement.py``), the restatement in the kernel's arithmetic and the
      reference give the same partition,
  (b) the reference's labels equal the project's label order,
  (c) in the kernel-arithmetic run every decision's gap to the best candidate with other inputs is at least 1e-9 of the
      largest absolute term of the two sums, and
  (d) in the float64 run that gap is at least 1e-5 (the project's fp32 tolerance: rounding elsewhere cannot reorder it).
Candidates with equal input tuples are ties (decided by id, identically everywhere); equal values from different
inputs are a gap of 0.  Seeds are walked graph by graph (a graph's decisions do not depend on its neighbours in the
batch): per family ``PROBE`` consecutive seeds are judged, at most one in ten may fail (asserted), and the first ones
that pass make up the case, which is judged once more as a whole and stored with its seeds.  A hand graph that fails is
left out, and its name is printed.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sep.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

import make_golden as G  # noqa: E402  (installs the PyG stand-in and imports the reference)
import sep_restatement as R  # noqa: E402
from make_golden_dmon import directed_graphs  # noqa: E402
from tgp.poolers.sep import SEPPooling  # noqa: E402

CASES = {}
PROBE = 20
GAP_KERNEL, GAP_F64 = 1e-9, 1e-5


def partition(labels):
    groups = {}
    for i, c in enumerate(labels.tolist() if hasattr(labels, "tolist") else labels):
        groups.setdefault(int(c), []).append(i)
    return sorted(groups.values())


def usable(inputs, ref_labels):
    """None if the case passes (a)-(d), else the letter of the first condition it fails."""
    n = inputs["x"].size(0)
    ei = inputs["edge_index"].numpy()
    ew = None if inputs["edge_weight"] is None else inputs["edge_weight"].numpy()
    bt = None if inputs["batch"] is None else inputs["batch"].numpy()
    g64, gk = {}, {}
    lab64, _ = R.sep_select(n, ei, ew, bt, "f64", g64)
    labk, _ = R.sep_select(n, ei, ew, bt, "kernel", gk)
    if not (partition(lab64) == partition(labk) == partition(ref_labels)):
        return "a"
    if lab64.tolist() != ref_labels.tolist() or labk.tolist() != ref_labels.tolist():
        return "b"
    if gk.get("min_ratio", float("inf")) < GAP_KERNEL:
        return "c"
    if g64.get("min_ratio", float("inf")) < GAP_F64:
        return "d"
    return None


def run_reference(cfg, inputs):
    pooler = SEPPooling(**cfg).eval()
    with torch.no_grad():
        out = pooler(x=inputs["x"], adj=inputs["edge_index"], edge_weight=inputs["edge_weight"], batch=inputs["batch"])
        lifted = pooler(x=out.x, so=out.so, lifting=True)
    return out, lifted


def store(name, cfg, inputs, out, lifted, seed):
    assert name not in CASES, name
    CASES[name] = {"seed": seed, "cfg": cfg, "inputs": {k: G.t(v) for k, v in inputs.items()},
                   "expected": {"cluster_index": G.t(out.so.cluster_index), "num_supernodes": int(out.so.num_supernodes),
                                "x": G.t(out.x), "edge_index": G.t(out.edge_index), "edge_weight": G.t(out.edge_weight),
                                "batch": G.t(out.batch), "x_lifted": G.t(lifted)}}


def add_family(name, cfg, draw, first_seed, batched=True, edgeless_at=None):
    """Walk seeds graph by graph: ``draw(seed)`` is one graph ``(x, edge_index, edge_weight)``; a graph that fails
    (a)-(d) is dropped.  ``PROBE`` draws are judged; the first ones that pass make up the case."""
    gen = torch.Generator().manual_seed(first_seed)
    want = int(torch.randint(4, 7, (1,), generator=gen)) if batched else 1
    failed, kept = [], []
    for seed in range(first_seed, first_seed + PROBE):
        x, ei, ew = draw(seed)
        one = dict(x=x, edge_index=ei, edge_weight=ew, batch=None)
        out, _ = run_reference({}, one)
        why = usable(one, out.so.cluster_index)
        if why is not None:
            failed.append((seed, why))
        elif len(kept) < want:
            kept.append((seed, x, ei, ew))
    assert 10 * len(failed) <= PROBE, f"{name}: {len(failed)} of {PROBE} seeds dropped: {failed}"
    assert len(kept) == want, name
    if edgeless_at is not None:
        kept.insert(edgeless_at, (-1, torch.ones(6, 4), torch.zeros(2, 0, dtype=torch.long), torch.zeros(0)))
    xs, eis, ews, bs, off = [], [], [], [], 0
    for g, (_, x, ei, ew) in enumerate(kept):
        xs.append(x), eis.append(ei + off), ews.append(ew), bs.append(torch.full((x.size(0),), g, dtype=torch.long))
        off += x.size(0)
    weighted = kept[0][3] is not None
    inputs = dict(x=torch.cat(xs), edge_index=torch.cat(eis, 1).contiguous(),
                  edge_weight=torch.cat(ews).contiguous() if weighted else None,
                  batch=torch.cat(bs) if batched else None)
    out, lifted = run_reference(cfg, inputs)
    why = usable(inputs, out.so.cluster_index)
    assert why is None, f"{name}: the assembled batch fails ({why})"
    seeds = [k[0] for k in kept]
    store(name, cfg, inputs, out, lifted, seeds)
    print(f"{name}: seeds {seeds}, N={inputs['x'].size(0)}, K={out.so.num_supernodes}, dropped {failed}")


# ---- random families: one graph per seed ---------------------------------------------------------------------------------
def graph_of(seed, weighted, p=0.15):
    gen = torch.Generator().manual_seed(seed)
    n = int(torch.randint(5, 41, (1,), generator=gen))
    ei, ew = G.er_graph(n, p, gen, weighted)
    return torch.randn(n, 4, generator=gen), ei, ew


def unweighted_graph(seed):
    return graph_of(seed, False)


def weighted_graph(seed):
    return graph_of(seed, True)


def directed_graph(seed):
    gen = torch.Generator().manual_seed(seed)
    n = int(torch.randint(5, 31, (1,), generator=gen))
    x, ei, ew, _ = directed_graphs([n], 0.1, gen, 4)
    return x, ei, ew


def isolated_nodes_graph(seed):
    x, ei, ew = graph_of(seed, True)
    keep = (ei[0] % 7 != 3) & (ei[1] % 7 != 3)  # every 7th node loses its edges
    return x, ei[:, keep].contiguous(), ew[keep].contiguous()


def single_graph(seed):
    gen = torch.Generator().manual_seed(seed)
    ei, ew = G.er_graph(30, 0.15, gen, True)
    return torch.randn(30, 4, generator=gen), ei, ew


def duplicates_and_loops(seed):
    x, ei, ew = graph_of(seed, True)
    gen = torch.Generator().manual_seed(seed + 7919)
    pick = torch.randperm(ei.size(1), generator=gen)[: ei.size(1) // 4]  # a quarter of the entries listed twice more
    loops = torch.arange(0, x.size(0), 3)
    ei2 = torch.cat([ei, ei[:, pick], torch.stack([loops, loops]), ei[:, pick]], 1).contiguous()
    ew2 = torch.cat([ew, torch.rand(pick.numel(), generator=gen) + 0.1, torch.rand(loops.numel(), generator=gen) + 0.1,
                     torch.rand(pick.numel(), generator=gen) + 0.1]).contiguous()
    return x, ei2, ew2


# ---- hand graphs ----------------------------------------------------------------------------------------------------------
def undirected(pairs, n):
    ei = torch.tensor([[a for a, b in pairs] + [b for a, b in pairs], [b for a, b in pairs] + [a for a, b in pairs]])
    return dict(x=torch.arange(n * 2, dtype=torch.float32).view(n, 2) / n, edge_index=ei, edge_weight=None, batch=None)


HAND = {
    "path7": undirected([(i, i + 1) for i in range(6)], 7),
    "cycle8": undirected([(i, (i + 1) % 8) for i in range(8)], 8),
    "star6": undirected([(0, i) for i in range(1, 7)], 7),
    "k5": undirected([(i, j) for i in range(5) for j in range(i + 1, 5)], 5),
    "grid4x4": undirected([(4 * r + c, 4 * r + c + 1) for r in range(4) for c in range(3)]
                          + [(4 * r + c, 4 * r + c + 4) for r in range(3) for c in range(4)], 16),
    "two_triangles": undirected([(0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5), (2, 3)], 6),
    "two_nodes": undirected([(0, 1)], 2),
}


def main():
    add_family("sep_unweighted", {}, unweighted_graph, 100)
    add_family("sep_weighted", {}, weighted_graph, 200)
    add_family("sep_directed", {}, directed_graph, 300)
    add_family("sep_edgeless_isolated", {}, isolated_nodes_graph, 400, edgeless_at=1)
    add_family("sep_single_graph", {}, single_graph, 500, batched=False)
    add_family("sep_duplicates_self_loops", {}, duplicates_and_loops, 600)
    add_family("sep_degree_norm_off", dict(degree_norm=False), weighted_graph, 700)
    add_family("sep_edge_weight_norm", dict(edge_weight_norm=True), weighted_graph, 800)
    add_family("sep_keep_self_loops", dict(remove_self_loops=False), duplicates_and_loops, 900)
    add_family("sep_lift_round_trip", dict(degree_norm=False), unweighted_graph, 1000)
    for name, inputs in HAND.items():
        out, lifted = run_reference({}, inputs)
        why = usable(inputs, out.so.cluster_index)
        if why is not None:
            print(f"hand graph {name}: left out, fails ({why})")
            continue
        store(f"sep_hand_{name}", {}, inputs, out, lifted, -1)
        print(f"sep_hand_{name}: N={inputs['x'].size(0)}, K={out.so.num_supernodes}, "
              f"labels {out.so.cluster_index.tolist()}")
    path = os.path.join(HERE, "golden_sep_v1.pt")
    torch.save({"tgp_version": G.tgp.__version__, "torch": str(torch.__version__), "cases": CASES}, path)
    print(f"wrote {len(CASES)} cases -> {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
