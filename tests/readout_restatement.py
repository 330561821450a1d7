"""Plain-torch restatement of the aggregation readout (reference reduce/aggr_reduce.py + global_reduce.py over PyG's
``scatter``): what ``AggrReduce`` / ``GlobalReduce`` return for sum / mean / max / min and a ``multi`` of them, in any
float dtype, on any device.  ``test_readout_restatement.py`` holds it against every case of ``golden_readout_v1.pt``;
the GPU tests use it in float64 as the reference of shapes the fixture does not hold.

Values are the reference's everywhere.  The BACKWARD of max / min differs from the reference's in one case: a group whose
extreme is exactly 0.  The reference starts ``scatter_reduce`` from zeros, and ATen's backward counts that initial 0 as
one more tied entry (each tied row gets 1 / (ties + 1)); here the extremes start from -inf / +inf and each tied row gets
1 / ties, which is the derivative and what the kernels compute.  The fixture's gradients (of ``sum(out ** 2)``, zero
wherever the output is) cannot tell the two apart."""
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
MULTI = ("sum", "mean", "max")


def load_cases():
    return torch.load(os.path.join(HERE, "golden", "golden_readout_v1.pt"), weights_only=True)["cases"]


def ops_of(op, op_kwargs=None):
    return tuple((op_kwargs or {}).get("aggrs", MULTI)) if op == "multi" else (op,)


def scatter(src, index, dim_size, op):
    """PyG's ``scatter(src, index, 0, dim_size, op)``: empty groups give 0, the mean divides by max(count, 1)."""
    out = src.new_zeros((dim_size,) + tuple(src.shape[1:]))
    if op in ("sum", "mean"):
        out = out.index_add(0, index, src)
        if op == "mean":
            count = src.new_zeros(dim_size).index_add(0, index, src.new_ones(index.numel())).clamp(min=1)
            out = out / count.view(-1, 1)
        return out
    # (the extremes start from -inf / +inf, not from the zeros an empty group ends with: the backward of ATen's
    #  scatter_reduce counts the initial value among the tied entries even with include_self=False, so a group whose
    #  extreme is exactly 0 would hand its rows 1 / (ties + 1) of the gradient instead of 1 / ties)
    idx = index.view(-1, 1).expand_as(src)
    start = torch.full_like(out, float("-inf") if op == "max" else float("inf"))
    ext = start.scatter_reduce(0, idx, src, reduce="amax" if op == "max" else "amin", include_self=False)
    some = torch.zeros(dim_size, dtype=torch.bool, device=src.device).index_fill(0, index, True)
    return torch.where(some.view((-1,) + (1,) * (src.dim() - 1)), ext, out)


def aggregate(src, index, dim_size, ops):
    return torch.cat([scatter(src, index, dim_size, op) for op in ops], dim=-1)


def readout(x, ops, batch=None, size=None, mask=None):
    """(x_pool, batch_pool) of ``AggrReduce(so=None)``; ``mask`` as ``GlobalReduce`` takes it for a dense ``x``."""
    if x.dim() == 3:
        B, N, F = x.shape
        index = torch.arange(B, device=x.device).repeat_interleave(N)
        rows = x.reshape(-1, F)
        if mask is not None:
            keep = mask.reshape(-1)
            rows, index = rows[keep], index[keep]
        groups = B if size is None else size
        return aggregate(rows, index, groups, ops), torch.arange(groups, device=x.device)
    if batch is None:
        return aggregate(x, torch.zeros(x.size(0), dtype=torch.long, device=x.device), 1, ops), None
    groups = size if size is not None else (int(batch.max()) + 1 if batch.numel() else 1)
    return aggregate(x, batch, groups, ops), torch.arange(groups, device=x.device)


def reduce_sparse(x, ops, node_index, cluster_index, weight, num_supernodes, batch=None):
    """(x_pool, batch_pool) of ``AggrReduce`` with a sparse assignment."""
    src = x[node_index]
    if weight is not None:
        src = src * weight.view(-1, 1)
    batch_pool = None
    if batch is not None:
        batch_pool = torch.arange(num_supernodes, device=x.device)
        batch_pool[cluster_index] = batch[node_index]
    return aggregate(src, cluster_index, num_supernodes, ops), batch_pool


def run_case(case, dtype=torch.float32, device="cpu", grad=False):
    """The restatement on a fixture case: (x_pool, batch_pool, leaves)."""
    i = case["inputs"]
    mv = lambda t: None if t is None else t.to(device)  # noqa: E731
    ops = ops_of(case["op"], case.get("op_kwargs"))
    x = mv(i["x"]).to(dtype).requires_grad_(grad)
    leaves = [x]
    if "node_index" in i:
        w = None
        if i["weight"] is not None:
            w = mv(i["weight"]).to(dtype).requires_grad_(grad)
            leaves.append(w)
        out, bp = reduce_sparse(x, ops, mv(i["node_index"]), mv(i["cluster_index"]), w, i["num_supernodes"], mv(i["batch"]))
    else:
        out, bp = readout(x, ops, mv(i.get("batch")), i.get("size"), mv(i.get("mask")))
        if case["kind"] == "global":
            bp = None
    return out, bp, leaves
