"""BN-Pool's public surface on the CPU: the reference's names, signatures and defaults (poolers/bnpool.py:141-163,
select/dp_select.py:87-95, utils/losses.py:1268-1275, 1359-1367, 1446-1452, 1520-1526), state-dict names, the
constructor's errors, the float64 loss forms against the reference's float64 values (tests/golden/golden_bnpool_v1.pt) at
1e-12, the selector with injected sticks, and the negative-edge sampler's contract on seeded host inputs."""
import inspect
import os

import pytest
import torch
from torch.distributions import Beta

import bnpool_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_bnpool_v1.pt"), weights_only=True)["cases"]
EMPTY = inspect.Parameter.empty


def _params(fn):
    return [(n, p.default) for n, p in inspect.signature(fn).parameters.items() if n != "self"]


def test_constructors_match_the_reference():
    from tgp.poolers import BNPool
    from tgp.select import DPSelect, MLPSelect
    assert _params(BNPool.__init__) == [
        ("in_channels", EMPTY), ("k", EMPTY), ("alpha_DP", 1.0), ("K_var", 1.0), ("K_mu", 10.0), ("K_init", 1.0),
        ("eta", 1.0), ("train_K", True), ("act", None), ("dropout", 0.0), ("remove_self_loops", True),
        ("degree_norm", True), ("edge_weight_norm", False), ("adj_transpose", True), ("lift", "precomputed"),
        ("s_inv_op", "transpose"), ("batched", True), ("sparse_output", False), ("cache_preprocessing", False),
        ("num_neg_samples", None)]
    assert _params(DPSelect.__init__) == [("in_channels", EMPTY), ("k", EMPTY), ("batched_representation", True),
                                          ("act", None), ("dropout", 0.0), ("s_inv_op", "transpose")]
    assert issubclass(DPSelect, MLPSelect)
    sel = DPSelect(5, 4)
    assert sel.k == 4 and sel.mlp.lins[-1].weight.shape == (6, 5)
    assert "float32" in DPSelect.__doc__ and "dtype of ``z``" in DPSelect.__doc__  # the documented divergence
    assert _params(BNPool.compute_loss) == [("adj", EMPTY), ("mask", EMPTY), ("so", EMPTY)]
    assert _params(BNPool.compute_sparse_loss) == [("adj", EMPTY), ("batch", EMPTY), ("so", EMPTY)]
    assert _params(BNPool.sample_negative_edges) == [("edge_index", EMPTY), ("batch", EMPTY)]
    for name in ("reset_parameters", "get_rec_adj", "get_prob_link_logit", "extra_repr_args"):
        assert callable(getattr(BNPool, name)), name


def test_loss_function_signatures_match_the_reference():
    from tgp.utils import losses, ops
    want = {
        "weighted_bce_reconstruction_loss": [("rec_adj", EMPTY), ("adj", EMPTY), ("mask", None), ("balance_links", True),
                                             ("normalizing_const", None), ("batch_reduction", "mean")],
        "kl_loss": [("q", EMPTY), ("p", EMPTY), ("mask", None), ("batch", None), ("batch_size", None),
                    ("normalizing_const", None), ("batch_reduction", "mean")],
        "cluster_connectivity_prior_loss": [("K", EMPTY), ("K_mu", EMPTY), ("K_var", EMPTY), ("normalizing_const", None),
                                            ("batch_reduction", "mean")],
        "sparse_bce_reconstruction_loss": [("link_prob_loigit", EMPTY), ("true_y", EMPTY), ("edges_batch_id", None),
                                           ("batch_size", None), ("batch_reduction", "mean")],
        "bnpool_rec_loss_terms": [("S", EMPTY), ("K_", EMPTY), ("adj", EMPTY), ("mask", None)],
    }
    for name, params in want.items():
        assert _params(getattr(losses, name)) == params, name
    assert issubclass(losses._BNPoolRecFn, torch.autograd.Function)
    assert _params(ops.negative_edge_sampling) == [("edge_index", EMPTY), ("num_nodes", None), ("num_neg_samples", None),
                                                   ("method", "auto"), ("force_undirected", False)]
    assert _params(ops.batched_negative_edge_sampling) == [("edge_index", EMPTY), ("batch", EMPTY),
                                                           ("num_neg_samples", None), ("method", "auto"),
                                                           ("force_undirected", False)]


def test_exports_and_alias_set():
    import tgp.poolers as P
    import tgp.select as S
    import tgp.utils as U
    from tgp import _native
    assert "BNPool" in P.pooler_classes and "BNPool" in P.__all__ and "DPSelect" in S.__all__
    assert "bnpool" not in P.pooler_map  # the alias is a follow-up (the alias set is pinned to five poolers)
    assert "bnpool" in P.__doc__
    assert P.BNPool._loss_kind == "bnpool"
    assert "bnpool" in P._DenseMLPPooling._LOSS_ONLY_KINDS and "bnpool" in P._DenseMLPPooling._DENSE_ADJ_LOSS_KINDS
    assert not P.BNPool(in_channels=3, k=2)._wants_raw
    assert type(P.BNPool(in_channels=3, k=2).selector) is S.DPSelect
    assert "negative_edge_sampling" in U.__all__ and "batched_negative_edge_sampling" in U.__all__
    for name in ("tgp_bnpool_rec_fwd_f32", "tgp_bnpool_rec_bwd_f32", "tgp_bnpool_part_floats", "tgp_bnpool_max_clusters"):
        assert name in _native.SIGNATURES, name


def test_native_entries_reject_bad_arguments_without_a_gpu():
    import ctypes
    from tgp import _native
    lib = _native.lib()
    d = (ctypes.c_int64 * 4)()
    p = ctypes.addressof(d)
    assert lib.tgp_bnpool_max_clusters() == 256
    assert lib.tgp_bnpool_part_floats(3, 70) == 3 * 3 * 4
    assert lib.tgp_bnpool_rec_fwd_f32(p, p, None, None, 2, 8, 4, p, 1 << 20, p, p, None) == -1  # null adjacency
    assert b"null pointer" in lib.tgp_last_error()
    assert lib.tgp_bnpool_rec_fwd_f32(p, p, p, None, 2, 8, 257, p, 1 << 20, p, p, None) == -4     # K out of range
    assert lib.tgp_bnpool_rec_fwd_f32(p, p, p, None, 2, 0, 4, p, 1 << 20, p, p, None) == -1       # N out of range
    assert lib.tgp_bnpool_rec_fwd_f32(p, p, p, None, 2, 70, 4, p, 23, p, p, None) == -1           # 2 * 3 * 4 = 24 needed
    assert b"workspace too small" in lib.tgp_last_error()
    assert lib.tgp_bnpool_rec_bwd_f32(p, p, p, None, p, p, 2, 8, 0, p, p, None) == -1
    assert lib.tgp_bnpool_rec_bwd_f32(p, p, p, None, p, None, 2, 8, 4, p, p, None) == -1
    assert lib.tgp_bnpool_rec_bwd_f32(p, p, p, None, p, p, 1 << 16, 8, 4, p, p, None) == -4


def test_state_dict_names_and_repr_args():
    from tgp.poolers import BNPool
    for name in ("bnpool_default", "bnpool_mlp2", "bnpool_u_single_graph", "bnpool_k2", "bnpool_fixed_K"):
        c = CASES[name]
        p = BNPool(**c["cfg"], batched=c["alias"] == "bnpool")
        assert sorted(p.state_dict()) == sorted(c["params"]), name
        p.load_state_dict(c["params"])
        assert p.K.requires_grad == c["cfg"].get("train_K", True)
    p = BNPool(in_channels=5, k=4, alpha_DP=2.5, K_var=0.5, K_mu=3.0, K_init=2.0, eta=0.3, train_K=False,
               batched=False, num_neg_samples=7)
    assert p.extra_repr_args() == {"batched": False, "alpha_DP": 2.5, "k_prior_variance": 0.5, "k_prior_mean": 3.0,
                                   "k_init_value": 2.0, "eta": 0.3, "train_K": False, "num_neg_samples": 7}
    eye = torch.eye(4)
    torch.testing.assert_close(p.K.detach(), 2.0 * eye - 2.0 * (1 - eye))
    torch.testing.assert_close(p.K_mu, 3.0 * eye - 3.0 * (1 - eye))
    torch.testing.assert_close(p.beta_prior, torch.full((3,), 2.5))
    with torch.no_grad():
        p.K.zero_()
    p.reset_parameters()
    torch.testing.assert_close(p.K.detach(), 2.0 * eye - 2.0 * (1 - eye))


@pytest.mark.parametrize("kw,msg", [(dict(alpha_DP=0.0), "alpha_DP must be positive"),
                                    (dict(K_var=-1.0), "K_var must be positive"), (dict(eta=0.0), "eta must be positive"),
                                    (dict(k=0), "max_k must be positive")])
def test_constructor_errors(kw, msg):
    from tgp.poolers import BNPool
    cfg = dict(in_channels=4, k=3)
    cfg.update(kw)
    with pytest.raises(ValueError, match=msg):
        BNPool(**cfg)


def _function_values(i, f32):
    from tgp.utils.losses import (cluster_connectivity_prior_loss, kl_loss, sparse_bce_reconstruction_loss,
                                  weighted_bce_reconstruction_loss)
    lg, adj, mask = i["logits"], i["adj"], i["mask"]
    n2, nn = mask.sum(-1) ** 2, torch.tensor(adj.size(-1), device=adj.device) ** 2
    q, p = Beta(i["alpha"], i["beta"]), Beta(i["prior_alpha"], i["prior_beta"])
    qf = Beta(i["alpha_flat"], i["beta_flat"])
    out = {
        "rec_mask": weighted_bce_reconstruction_loss(lg, adj, mask, normalizing_const=n2),
        "rec_mask_sum": weighted_bce_reconstruction_loss(lg, adj, mask, normalizing_const=n2, batch_reduction="sum"),
        "rec_nomask": weighted_bce_reconstruction_loss(lg, adj, None, normalizing_const=nn),
        "rec_nonorm": weighted_bce_reconstruction_loss(lg, adj, mask),
        "rec_unbalanced": weighted_bce_reconstruction_loss(lg, adj, mask, balance_links=False, normalizing_const=n2),
        "rec_unbalanced_nomask": weighted_bce_reconstruction_loss(lg, adj, None, balance_links=False),
        "rec_pm30": weighted_bce_reconstruction_loss(lg * 10, adj, mask, normalizing_const=n2),
        "prior": cluster_connectivity_prior_loss(i["K"], i["K_mu"], i["K_var"]),
        "prior_vec": cluster_connectivity_prior_loss(i["K"], i["K_mu"], i["K_var"], normalizing_const=n2),
        "prior_vec_sum": cluster_connectivity_prior_loss(i["K"], i["K_mu"], i["K_var"], normalizing_const=n2,
                                                         batch_reduction="sum"),
        "prior_scalar": cluster_connectivity_prior_loss(i["K"], i["K_mu"], i["K_var"], normalizing_const=nn),
        "kl_mask": kl_loss(q, p, mask=mask, normalizing_const=n2),
        "kl_mask_sum": kl_loss(q, p, mask=mask, batch_reduction="sum"),
        "kl_nomask": kl_loss(q, p, normalizing_const=nn),
        "kl_flat": kl_loss(qf, p),
    }
    out["bce_global"], out["bce_global_count"] = sparse_bce_reconstruction_loss(i["edge_logits"], i["edge_y"])
    if f32:
        out["kl_batch"] = kl_loss(qf, p, batch=i["batch"], batch_size=3,
                                  normalizing_const=torch.tensor([4., 9., 2.], device=adj.device))
        out["bce_batch"], out["bce_batch_count"] = sparse_bce_reconstruction_loss(
            i["edge_logits"], i["edge_y"], edges_batch_id=i["edge_batch"], batch_size=3)
        out["bce_batch_sum"], _ = sparse_bce_reconstruction_loss(
            i["edge_logits"], i["edge_y"], edges_batch_id=i["edge_batch"], batch_size=4, batch_reduction="sum")
    return out


@pytest.mark.parametrize("tag,tol", [("f64", 1e-12), ("f32", 1e-5)])
def test_loss_forms_match_the_reference(tag, tol):
    """The four composed loss functions on host tensors (they take logits and distributions that already exist):
    float64 at 1e-12 relative to the value's magnitude, float32 at the project's tolerance."""
    c = CASES[f"bnpool_functions_{tag}"]
    e = c["expected"]
    got = _function_values(c["inputs"], tag == "f32")
    assert set(got) == {k for k in e if not k.startswith("grad_")}
    for name, v in got.items():
        assert v.dtype == e[name].dtype and v.shape == e[name].shape, name
        err = float((v - e[name]).abs().max())
        assert err <= tol * float(e[name].abs().max()), (name, v, e[name])


def test_float64_logit_gradient_matches_the_reference():
    from tgp.utils.losses import weighted_bce_reconstruction_loss
    c = CASES["bnpool_functions_f64"]
    i, e = c["inputs"], c["expected"]
    n2 = i["mask"].sum(-1) ** 2
    for key, scale in (("rec_mask", 1.0), ("rec_pm30", 10.0)):
        leaf = (i["logits"] * scale).clone().requires_grad_(True)
        weighted_bce_reconstruction_loss(leaf, i["adj"], i["mask"], normalizing_const=n2).backward()
        want = e[f"grad_{key}"]
        assert float((leaf.grad - want).abs().max()) <= 1e-12 * float(want.abs().max()), key


def test_float32_host_tensors_have_no_cpu_fallback():
    from tgp import _native
    from tgp.poolers import BNPool
    from tgp.utils.losses import bnpool_rec_loss_terms
    s = torch.softmax(torch.randn(2, 5, 3), -1)
    adj = (torch.rand(2, 5, 5) < 0.4).float()
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        bnpool_rec_loss_terms(s, torch.randn(3, 3), adj)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        BNPool(in_channels=4, k=3)(x=torch.randn(2, 5, 4), adj=adj)
    # float64 anywhere: the composed form, on the host too
    k = torch.randn(3, 3, dtype=torch.float64)
    got = bnpool_rec_loss_terms(s.double(), k, adj.double())
    torch.testing.assert_close(got, R.rec_terms(s.double(), k, adj.double()), rtol=1e-12, atol=0)


def test_dpselect_with_injected_sticks():
    """The stored stick fractions through a float64 DPSelect: the restatement's float64 S at 1e-12, and the reference's
    float32 S (the reference cannot run its selector in float64) at float32's rounding."""
    from tgp.select import DPSelect
    for name in ("bnpool_dense_inputs_mask_holes", "bnpool_dense_inputs_nomask", "bnpool_u_mlp2", "bnpool_u_k2"):
        c = CASES[name]
        i, cfg = c["inputs"], c["cfg"]
        batched = c["alias"] == "bnpool"
        sel = DPSelect(cfg["in_channels"], cfg["k"], batched_representation=batched, act=cfg.get("act")).double()
        sel.load_state_dict({k[len("selector."):]: v.double() for k, v in c["params"].items()
                             if k.startswith("selector.")})
        z = c["z"].double()
        seen = []
        sel.sample_sticks = lambda q_z: (seen.append(q_z), z)[1]
        so = sel(i["x"].double(), mask=i.get("mask")) if batched else sel(i["x"].double(), batch=i.get("batch"))
        want = R.sticks_to_s(z, i.get("mask") if batched else None)
        assert so.s.dtype == torch.float64 and so.q_z is seen[0]
        assert float((so.s - want).abs().max()) <= 1e-12
        ref = c["expected"]["so"]["s"]
        assert float((so.s - ref.double()).abs().max()) <= 4 * torch.finfo(torch.float32).eps
        # the posterior's parameters: the restated MLP + softplus + clamp
        ws = [v.double() for k, v in sorted(c["params"].items()) if k.startswith("selector") and k.endswith("weight")]
        bs = [v.double() for k, v in sorted(c["params"].items()) if k.startswith("selector") and k.endswith("bias")]
        alpha, beta = R.selector_params(i["x"].double(), ws, bs, cfg.get("act"))
        with torch.no_grad():
            assert float((so.q_z.concentration1 - alpha.reshape(so.q_z.concentration1.shape)).abs().max()) <= 1e-12
            assert float((so.q_z.concentration0 - beta.reshape(so.q_z.concentration0.shape)).abs().max()) <= 1e-12
    # the default draw is the distribution's reparameterised sample
    sel = DPSelect(3, 4)
    torch.manual_seed(0)
    a = sel.sample_sticks(Beta(torch.ones(5, 3), torch.ones(5, 3) * 2))
    torch.manual_seed(0)
    b = Beta(torch.ones(5, 3), torch.ones(5, 3) * 2).rsample()
    assert torch.equal(a, b)


def test_float64_select_and_loss_on_the_host_match_the_restatement():
    """A float64 BNPool's Select and compute_loss run on host tensors (composed route; Reduce and Connect have no host
    form): the three losses against the restatement."""
    from tgp.poolers import BNPool
    for name in ("bnpool_dense_inputs_mask_dirty", "bnpool_dense_inputs_mask_holes", "bnpool_dense_inputs_nomask"):
        c = CASES[name]
        i = c["inputs"]
        p = BNPool(**c["cfg"]).double().eval()
        p.load_state_dict({k: v.double() for k, v in c["params"].items()})
        z = c["z"].double()
        p.selector.sample_sticks = lambda q_z: z
        # (forward() hands compute_loss an all-true mask when the caller gave none, as the reference's does)
        mask = i["mask"] if "mask" in i else torch.ones(i["x"].shape[:2], dtype=torch.bool)
        so = p.select(x=i["x"].double(), mask=mask)
        loss = p.compute_loss(i["adj"].double(), mask, so)
        import test_bnpool_restatement as T
        _, want = T.restated_case(c, torch.float64)
        assert list(loss) == ["quality", "kl", "K_prior"]
        for k in loss:
            assert loss[k].dtype == torch.float64 and loss[k].dim() == 0
            assert abs(float(loss[k].detach()) - float(want[k])) <= 1e-12 * abs(float(want[k])), (name, k)


# ----------------------------------------------------------------------------------------------- the sampler's contract
def _seeded_batch(sizes, p, seed):
    gen = torch.Generator().manual_seed(seed)
    eis, bs, off = [], [], 0
    for g, n in enumerate(sizes):
        a = torch.rand(n, n, generator=gen) < p
        a.fill_diagonal_(False)
        eis.append(a.nonzero().t() + off)
        bs.append(torch.full((n,), g, dtype=torch.long))
        off += n
    return torch.cat(eis, 1), torch.cat(bs)


def check_sampler_contract(edge_index, batch, neg, num_neg_samples, force_undirected):
    """The conditions every returned set of negative edges satisfies (shared with the device test)."""
    edge_index, batch, neg = edge_index.cpu(), batch.cpu(), neg.cpu()
    assert neg.dtype == torch.long and neg.dim() == 2 and neg.size(0) == 2
    n = batch.numel()
    sizes = torch.bincount(batch)
    if neg.size(1):
        assert int(neg.min()) >= 0 and int(neg.max()) < n
    assert bool((batch[neg[0]] == batch[neg[1]]).all()), "a pair crosses two graphs"
    assert bool((neg[0] != neg[1]).all()), "a self-loop"
    edges = set((edge_index[0] * n + edge_index[1]).tolist())
    keys = (neg[0] * n + neg[1]).tolist()
    assert not edges.intersection(keys), "an existing edge"
    assert len(set(keys)) == len(keys), "a pair twice"
    if force_undirected:
        assert set(keys) == set((neg[1] * n + neg[0]).tolist()), "a pair without its reverse"
    e_g = torch.bincount(batch[edge_index[0]], minlength=sizes.numel())
    got = torch.bincount(batch[neg[0]], minlength=sizes.numel())
    cap = torch.minimum(e_g, sizes * sizes - e_g) if num_neg_samples is None else torch.full_like(sizes, num_neg_samples)
    if force_undirected:
        cap = cap // 2 * 2
    assert bool((got <= cap).all()), (got.tolist(), cap.tolist())
    return got, cap


@pytest.mark.parametrize("method", ["auto", "sparse"])
@pytest.mark.parametrize("undirected", [False, True])
@pytest.mark.parametrize("num", [None, 5, 0])
def test_sampler_contract_on_host_inputs(method, undirected, num):
    from tgp.utils.ops import batched_negative_edge_sampling
    ei, batch = _seeded_batch([7, 2, 12, 1, 9], 0.3, 3)
    # graph 1 (two nodes) gets both of its edges, and a complete graph of 5 nodes is appended: neither has room
    n = batch.numel()
    full = (~torch.eye(5, dtype=torch.bool)).nonzero().t() + n
    ei = torch.cat([ei[:, batch[ei[0]] != 1], torch.tensor([[7, 8], [8, 7]]), full], 1)
    batch = torch.cat([batch, torch.full((5,), 5)])
    torch.manual_seed(0)
    neg = batched_negative_edge_sampling(ei, batch, num_neg_samples=num, method=method, force_undirected=undirected)
    got, cap = check_sampler_contract(ei, batch, neg, num, undirected)
    assert got[1] == 0 and got[3] == 0 and got[5] == 0  # the 2-node, the 1-node and the complete graph: no room
    if method == "auto" and num != 0 and not undirected:
        # every pair was enumerated and a directed graph has n^2 - n - E >= its cap free pairs here: the cap is filled
        # (undirected, a pair is free only when neither direction is an edge: there may be fewer than the cap)
        assert got[0] == cap[0] and got[2] == cap[2] and got[4] == cap[4]
    if num != 0:
        assert got[0] > 0 and got[2] > 0 and got[4] > 0


def test_sampler_single_graph_and_host_reads(monkeypatch):
    from tgp.utils import ops
    ei, batch = _seeded_batch([15], 0.2, 5)
    torch.manual_seed(1)
    neg = ops.negative_edge_sampling(ei, num_nodes=15, force_undirected=True)
    check_sampler_contract(ei, batch, neg, None, True)
    assert ops.negative_edge_sampling(ei[:, :0], num_nodes=3).shape == (2, 0)  # no edges: the cap is 0
    with pytest.raises(NotImplementedError):
        ops.negative_edge_sampling(ei, num_nodes=(3, 4))
    # every host read of the sampler goes through one helper: the same number for 3 graphs and for 40
    reads = []
    real = ops._sampler_host_read
    monkeypatch.setattr(ops, "_sampler_host_read", lambda t: (reads.append(1), real(t))[1])
    counts = []
    for sizes in ([5, 9, 4], list(range(3, 43))):
        ei, batch = _seeded_batch(sizes, 0.3, 7)
        del reads[:]
        ops.batched_negative_edge_sampling(ei, batch, force_undirected=True)
        counts.append(len(reads))
    assert counts[0] == counts[1] == 1
