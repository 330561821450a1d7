#!/usr/bin/env python3
"""Generate the golden vectors of BN-Pool (``tests/golden/golden_bnpool_v1.pt``).

TEST INFRASTRUCTURE ONLY — run in the BUILD container, never on the GPU box.

Same recipe as ``make_golden_hosc.py`` (whose helpers it imports): the real reference (tgp 1.0.1) over the PyG stand-in
runs ``get_pooler("bnpool")`` / ``get_pooler("bnpool_u")`` and the four BN-Pool loss functions on small seeded inputs.

Two things of a pooler run are random and cannot be reproduced on another device: the stick fractions
(``Beta.rsample``) and, unbatched, the sampled non-edges.  Both are captured by wrapping the reference's calls and
stored with the case (``z``, ``neg_edge_index``); a consumer injects them.  In every pooler case ``K`` is overwritten
with a seeded ASYMMETRIC matrix before the call (the default is symmetric and hides orientation errors).

The reference's pooler does not run in float64 (``DPSelect`` allocates pi as float32), so float64 expectations exist
for the loss FUNCTIONS only, with the gradient of the reconstruction loss with respect to the logits.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_bnpool.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import torch  # noqa: E402
from torch.distributions import Beta  # noqa: E402

import make_golden as G  # noqa: E402  (installs the PyG stand-in and imports the reference)
from make_golden_dmon import directed_graphs  # noqa: E402
from make_golden_hosc import _as_float  # noqa: E402
import tgp.poolers.bnpool as RB  # noqa: E402
from tgp.poolers import get_pooler  # noqa: E402
from tgp.utils import losses as RL  # noqa: E402

CASES = {}


class Capture:
    """Record what ``Beta.rsample`` and the reference's negative samplers return during one pooler call."""

    def __enter__(self):
        self.z, self.neg = [], []
        self._rsample = Beta.rsample
        self._samplers = (RB.negative_edge_sampling, RB.batched_negative_edge_sampling)
        cap = self

        def rsample(dist, *a, **k):
            out = cap._rsample(dist, *a, **k)
            cap.z.append(out.detach().clone())
            return out

        def wrap(fn):
            def sampler(*a, **k):
                out = fn(*a, **k)
                cap.neg.append(out.detach().clone())
                return out
            return sampler

        Beta.rsample = rsample
        RB.negative_edge_sampling = wrap(self._samplers[0])
        RB.batched_negative_edge_sampling = wrap(self._samplers[1])
        return self

    def __exit__(self, *exc):
        Beta.rsample = self._rsample
        RB.negative_edge_sampling, RB.batched_negative_edge_sampling = self._samplers


def add_pool(name, alias, cfg, inputs, seed):
    torch.manual_seed(seed)
    pooler = get_pooler(alias, **cfg).eval()
    k = cfg["k"]
    with torch.no_grad():
        pooler.K.copy_(torch.randn(k, k, generator=torch.Generator().manual_seed(100 + seed)))
    kw = dict(inputs)
    if "edge_index" in kw:
        kw["adj"] = kw.pop("edge_index")
    with torch.no_grad(), Capture() as cap:
        out = pooler(**kw)
    assert len(cap.z) == 1 and len(cap.neg) == (1 if alias.endswith("_u") else 0), (name, len(cap.z), len(cap.neg))
    expected = G.pool_dict(out)
    expected["loss"] = {k_: _as_float(v, torch.float32) for k_, v in out.loss.items()}
    assert name not in CASES, name
    CASES[name] = {"kind": "pool", "alias": alias, "inputs": {k_: G.t(v) for k_, v in inputs.items()},
                   "params": G.params_of(pooler), "cfg": cfg, "expected": expected, "z": cap.z[0],
                   "neg_edge_index": cap.neg[0] if cap.neg else None}


def gen_poolers():
    sizes = [9, 6, 12]
    gen = torch.Generator().manual_seed(11)
    x, ei, ew, batch = directed_graphs(sizes, 0.4, gen, 5)
    for mode in ("", "_u"):
        for tag, flags in (
            ("default", dict()),
            ("sparse_out", dict(sparse_output=True)),
            ("noT_ewn", dict(adj_transpose=False, edge_weight_norm=True)),
            ("raw", dict(remove_self_loops=False, degree_norm=False)),
            ("fixed_K", dict(train_K=False)),
            ("hyper", dict(alpha_DP=2.5, eta=0.3, K_var=0.5, K_mu=3.0)),
            ("mlp2", dict(in_channels=[5, 7], act="relu")),
            ("k2", dict(k=2)),
        ):
            cfg = dict(in_channels=5, k=4)
            cfg.update(flags)
            add_pool(f"bnpool{mode}_{tag}", "bnpool" + mode, cfg, dict(x=x, edge_index=ei, edge_weight=ew, batch=batch), 1)
        add_pool(f"bnpool{mode}_unweighted", "bnpool" + mode, dict(in_channels=5, k=4),
                 dict(x=x, edge_index=ei, edge_weight=None, batch=batch), 1)
    # single graph, no batch vector, both modes
    gen = torch.Generator().manual_seed(6)
    xs, eis, ews, _ = directed_graphs([10], 0.4, gen, 5)
    for mode in ("", "_u"):
        add_pool(f"bnpool{mode}_single_graph", "bnpool" + mode, dict(in_channels=5, k=3),
                 dict(x=xs, edge_index=eis, edge_weight=ews, batch=None), 3)
    # a batch with an edgeless graph
    keep = batch[ei[0]] != 1
    ei2, ew2 = ei[:, keep].contiguous(), ew[keep].contiguous()
    for mode in ("", "_u"):
        add_pool(f"bnpool{mode}_edgeless_graph", "bnpool" + mode, dict(in_channels=5, k=4),
                 dict(x=x, edge_index=ei2, edge_weight=ew2, batch=batch), 1)
    # already-dense padded inputs + explicit mask; "dirty": the padded rows and columns of A are not zero; a mask that
    # is no prefix of the rows; no mask at all
    gen = torch.Generator().manual_seed(8)
    B, N, F = 3, 8, 5
    a = (torch.rand(B, N, N, generator=gen) < 0.4).float() * (torch.rand(B, N, N, generator=gen) * 2 + 0.1)
    mask = torch.ones(B, N, dtype=torch.bool)
    mask[1, 6:] = False
    mask[2, 5:] = False
    xd = torch.randn(B, N, F, generator=gen) * mask.unsqueeze(-1)
    clean = a * mask.unsqueeze(1) * mask.unsqueeze(2)
    add_pool("bnpool_dense_inputs_mask", "bnpool", dict(in_channels=F, k=3), dict(x=xd, adj=clean, mask=mask), 4)
    add_pool("bnpool_dense_inputs_mask_dirty", "bnpool", dict(in_channels=F, k=3), dict(x=xd, adj=a, mask=mask), 4)
    holes = torch.ones(B, N, dtype=torch.bool)
    holes[0, 2] = False
    holes[1, [0, 3, 7]] = False
    holes[2, 4:6] = False
    add_pool("bnpool_dense_inputs_mask_holes", "bnpool", dict(in_channels=F, k=3),
             dict(x=torch.randn(B, N, F, generator=gen), adj=a, mask=holes), 4)
    add_pool("bnpool_dense_inputs_nomask", "bnpool", dict(in_channels=F, k=3), dict(x=xd, adj=clean), 4)


def gen_functions():
    """Each public loss on its own, float32 and float64."""
    gen = torch.Generator().manual_seed(21)
    B, N, Kc = 4, 7, 4
    mask = torch.ones(B, N, dtype=torch.bool)
    mask[0, 5:] = False
    mask[3, [1, 4]] = False
    adj = (torch.rand(B, N, N, generator=gen) < 0.35).float() * (torch.rand(B, N, N, generator=gen) * 3 + 0.2)
    adj[1] = torch.rand(N, N, generator=gen) * 3 + 0.2  # a complete graph (self-loops included)
    adj[2] = 0.0                                        # an empty graph
    logits = torch.randn(B, N, N, generator=gen) * 3
    alpha = torch.rand(B, N, Kc - 1, generator=gen) * 3 + 0.2
    beta = torch.rand(B, N, Kc - 1, generator=gen) * 3 + 0.2
    prior_a, prior_b = torch.ones(Kc - 1), torch.ones(Kc - 1) * 2.5
    batch = torch.tensor([0] * 6 + [1] * 9 + [2] * 5)
    alpha_f = torch.rand(batch.numel(), Kc - 1, generator=gen) * 3 + 0.2
    beta_f = torch.rand(batch.numel(), Kc - 1, generator=gen) * 3 + 0.2
    Km = torch.randn(Kc, Kc, generator=gen)
    K_mu = 3.0 * torch.eye(Kc) - 3.0 * (1 - torch.eye(Kc))
    e_logit = torch.randn(40, generator=gen) * 4
    e_y = (torch.rand(40, generator=gen) < 0.5).float()
    e_batch = torch.randint(0, 3, (40,), generator=gen).sort().values
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        adj_, lg = adj.to(dt), logits.to(dt)
        n2 = mask.sum(-1) ** 2
        exp = {
            "rec_mask": RL.weighted_bce_reconstruction_loss(lg, adj_, mask, normalizing_const=n2),
            "rec_mask_sum": RL.weighted_bce_reconstruction_loss(lg, adj_, mask, normalizing_const=n2,
                                                                batch_reduction="sum"),
            "rec_nomask": RL.weighted_bce_reconstruction_loss(lg, adj_, None, normalizing_const=torch.tensor(N) ** 2),
            "rec_nonorm": RL.weighted_bce_reconstruction_loss(lg, adj_, mask),
            "rec_unbalanced": RL.weighted_bce_reconstruction_loss(lg, adj_, mask, balance_links=False,
                                                                  normalizing_const=n2),
            "rec_unbalanced_nomask": RL.weighted_bce_reconstruction_loss(lg, adj_, None, balance_links=False),
            "rec_pm30": RL.weighted_bce_reconstruction_loss(lg * 10, adj_, mask, normalizing_const=n2),
            "prior": RL.cluster_connectivity_prior_loss(Km.to(dt), K_mu.to(dt), torch.tensor(0.5, dtype=dt)),
            "prior_vec": RL.cluster_connectivity_prior_loss(Km.to(dt), K_mu.to(dt), torch.tensor(0.5, dtype=dt),
                                                            normalizing_const=n2),
            "prior_vec_sum": RL.cluster_connectivity_prior_loss(Km.to(dt), K_mu.to(dt), torch.tensor(0.5, dtype=dt),
                                                                normalizing_const=n2, batch_reduction="sum"),
            "prior_scalar": RL.cluster_connectivity_prior_loss(Km.to(dt), K_mu.to(dt), torch.tensor(0.5, dtype=dt),
                                                               normalizing_const=torch.tensor(N) ** 2),
        }
        q, p = Beta(alpha.to(dt), beta.to(dt)), Beta(prior_a.to(dt), prior_b.to(dt))
        qf = Beta(alpha_f.to(dt), beta_f.to(dt))
        exp["kl_mask"] = RL.kl_loss(q, p, mask=mask, normalizing_const=n2)
        exp["kl_mask_sum"] = RL.kl_loss(q, p, mask=mask, batch_reduction="sum")
        exp["kl_nomask"] = RL.kl_loss(q, p, normalizing_const=torch.tensor(N) ** 2)
        exp["kl_flat"] = RL.kl_loss(qf, p)
        exp["bce_global"], exp["bce_global_count"] = RL.sparse_bce_reconstruction_loss(e_logit.to(dt), e_y.to(dt))
        if dt == torch.float32:  # (the reference scatters into float32 buffers: these do not run in float64)
            exp["kl_batch"] = RL.kl_loss(qf, p, batch=batch, batch_size=3, normalizing_const=torch.tensor([4., 9., 2.]))
            exp["bce_batch"], exp["bce_batch_count"] = RL.sparse_bce_reconstruction_loss(
                e_logit, e_y, edges_batch_id=e_batch, batch_size=3)
            exp["bce_batch_sum"], _ = RL.sparse_bce_reconstruction_loss(
                e_logit, e_y, edges_batch_id=e_batch, batch_size=4, batch_reduction="sum")
        else:  # the gradient of the reconstruction loss with respect to the logits
            for key, scale in (("rec_mask", 1.0), ("rec_pm30", 10.0)):
                leaf = (lg * scale).clone().requires_grad_(True)
                RL.weighted_bce_reconstruction_loss(leaf, adj_, mask, normalizing_const=n2).backward()
                exp[f"grad_{key}"] = leaf.grad
        CASES[f"bnpool_functions_{tag}"] = {
            "kind": "functions",
            "inputs": {"logits": lg, "adj": adj_, "mask": mask, "alpha": alpha.to(dt), "beta": beta.to(dt),
                       "prior_alpha": prior_a.to(dt), "prior_beta": prior_b.to(dt), "batch": batch,
                       "alpha_flat": alpha_f.to(dt), "beta_flat": beta_f.to(dt), "K": Km.to(dt), "K_mu": K_mu.to(dt),
                       "K_var": torch.tensor(0.5, dtype=dt), "edge_logits": e_logit.to(dt), "edge_y": e_y.to(dt),
                       "edge_batch": e_batch},
            "expected": {k: G.t(v) for k, v in exp.items()}}


def main():
    gen_poolers()
    gen_functions()
    out = os.path.join(HERE, "golden_bnpool_v1.pt")
    torch.save({"tgp_version": G.tgp.__version__, "torch": str(torch.__version__), "cases": CASES}, out)
    print(f"wrote {len(CASES)} cases -> {out} ({os.path.getsize(out) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
