"""GTVConv's public surface on the CPU: import paths, constructor, the reference's own three tests restated, the layer on
host tensors (composed form) against every fixture case, and the argument checks of the three native entries."""
import ctypes
import os

import pytest
import torch

from test_gpu_grad_paths import FACTOR, FLOOR

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = torch.load(os.path.join(HERE, "golden", "golden_gtv_v1.pt"), weights_only=True)["cases"]


def build_layer(c, device="cpu", dtype=torch.float32):
    from tgp.mp import GTVConv
    conv = GTVConv(**c["cfg"]).to(device, dtype)
    with torch.no_grad():
        conv.weight.copy_(c["params"]["weight"])
        if conv.bias is not None:
            conv.bias.copy_(c["params"]["bias"])
    return conv


def layer_inputs(c, device="cpu", dtype=torch.float32):
    """(x, second argument, edge_weight, mask) of a fixture case as the layer is called with them."""
    i = c["inputs"]
    x = i["x"].to(device, dtype)
    mask = None if i.get("mask") is None else i["mask"].to(device)
    if "adj" in i:
        return x, i["adj"].to(device, dtype), None, mask
    w = None if i["edge_weight"] is None else i["edge_weight"].to(device, dtype)
    ei = i["edge_index"].to(device)
    if i.get("coo"):
        return x, torch.sparse_coo_tensor(ei, w, (x.size(0), x.size(0))).coalesce(), None, mask
    return x, ei, w, mask


def fixture_error(out, c):
    want = c["f64"]["out"]
    assert out.shape == want.shape
    return float(torch.linalg.vector_norm(out.detach().cpu().double() - want)) / float(torch.linalg.vector_norm(want))


def test_import_paths_and_all():
    import tgp.mp
    from tgp.mp import GTVConv, gtv_adj_weights, gtv_propagate_composed  # noqa: F401
    assert tgp.mp.__all__ == ["GTVConv", "gtv_adj_weights"]
    import tgp.nn
    assert "GTVConv" not in tgp.nn.__all__


def test_constructor_defaults_repr_and_reset():
    from tgp.mp import GTVConv
    torch.manual_seed(0)
    conv = GTVConv(5, 7)
    assert tuple(conv.weight.shape) == (5, 7) and tuple(conv.bias.shape) == (7,)
    assert conv.delta_coeff == 1.0 and conv.eps == 1e-3 and isinstance(conv.act, torch.nn.ReLU)
    assert float(conv.bias.abs().max()) == 0.0 and float(conv.weight.abs().max()) > 0.0
    assert "GTVConv(5, 7" in repr(conv) and "delta_coeff=1.0" in repr(conv) and "eps=0.001" in repr(conv)
    with torch.no_grad():
        conv.bias.fill_(3.0)
        before = conv.weight.clone()
    conv.reset_parameters()
    assert float(conv.bias.abs().max()) == 0.0 and not torch.equal(conv.weight, before)
    assert GTVConv(5, 7, bias=False).bias is None
    assert isinstance(GTVConv(2, 2, act=torch.nn.Tanh()).act, torch.nn.Tanh)
    assert isinstance(GTVConv(2, 2, act="elu").act, torch.nn.ELU)
    assert GTVConv(2, 2, act=torch.sigmoid).act is torch.sigmoid
    with pytest.raises(ValueError, match="Could not resolve activation"):
        GTVConv(2, 2, act="no-such-activation")


def test_reference_gtv_adj_weights_source_to_target():
    from tgp.mp import gtv_adj_weights
    ei, ew = gtv_adj_weights(edge_index=torch.tensor([[0, 1], [1, 0]]), edge_weight=torch.tensor([1.0, 1.0]),
                             num_nodes=2, flow="source_to_target", coeff=1.0)
    assert ei.size(1) == 4
    assert torch.allclose(ew, torch.tensor([1.0, 1.0, 0.0, 0.0]))
    # weighted, directed, an existing loop, both flows: I - coeff (D - A) by hand
    ei0, ew0 = torch.tensor([[0, 1, 1], [1, 0, 1]]), torch.tensor([1.0, 2.0, 3.0])
    ei, ew = gtv_adj_weights(ei0, ew0, 3, "source_to_target", 0.5)
    assert ei.tolist() == [[0, 1, 0, 1, 2], [1, 0, 0, 1, 2]]
    # in-degrees 2, 4, 0: diagonal 1 - 0.5 (deg - a_ii) = 0, 0.5, 1
    assert torch.allclose(ew, torch.tensor([0.5, 1.0, 0.0, 0.5, 1.0]))
    _, ew = gtv_adj_weights(ei0, ew0, 3, "target_to_source", 0.5)  # out-degrees 1, 5, 0
    assert torch.allclose(ew, torch.tensor([0.5, 1.0, 0.5, 0.0, 1.0]))
    assert float(ew0[2]) == 3.0  # the caller's weights are not written


def test_reference_forward_shapes_and_finiteness():
    from tgp.mp import GTVConv
    torch.manual_seed(1)
    x = torch.randn(3, 2)
    ei = torch.tensor([[0, 1, 0, 1, 2], [1, 2, 0, 1, 2]])  # the path 0 -> 1 -> 2 and a loop on every node
    conv = GTVConv(2, 4, delta_coeff=1.0, eps=1e-4, act=torch.nn.PReLU()).eval()
    out = conv(x, ei, torch.ones(5))
    assert out.shape == (3, 4) and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("bias", [True, False])
def test_reference_dense_forward_and_a_masked_row_is_zero(bias):
    from tgp.mp import GTVConv
    torch.manual_seed(2)
    x = torch.randn(2, 3, 2)
    adj = torch.ones(3, 3).unsqueeze(0).repeat(2, 1, 1)
    conv = GTVConv(2, 4, bias=bias, delta_coeff=0.5, eps=1e-3, act="relu").eval()
    out = conv(x, adj)
    assert out.shape == (2, 3, 4) and bool(torch.isfinite(out).all())
    masked = conv(x, adj, mask=torch.tensor([1, 0, 1], dtype=torch.bool).expand(2, 3))
    assert masked.shape == (2, 3, 4)
    assert torch.allclose(masked[:, 1], torch.zeros_like(masked[:, 1]))
    assert torch.equal(masked[:, 0], out[:, 0])


@pytest.mark.parametrize("name", sorted(CASES))
def test_layer_on_host_tensors_reproduces_the_fixture(name):
    """Host tensors take the composed form; its error against the float64 run is held to the float32 reference's own."""
    from tgp import kernels as K
    c = CASES[name]
    before = K.gtv_record()
    out = build_layer(c)(*layer_inputs(c))
    after = K.gtv_record()
    assert after["route"] == "composed" and after["composed"] == before["composed"] + 1
    assert after["native"] == before["native"]
    e = fixture_error(out, c)
    bound = max(FACTOR * c["e_ref32"], FLOOR)
    print(f"{name}: e {e:.2e}, e_ref32 {c['e_ref32']:.2e}, bound {bound:.2e}")
    assert e <= bound, (name, e, bound)


def test_layer_in_float64_on_the_host_matches_the_fixture_and_its_gradients():
    for name in ("gtv_undirected_weighted", "gtv_dense_batch_mask", "gtv_zero_distance"):
        c = CASES[name]
        conv = build_layer(c, dtype=torch.float64)
        x, conn, w, mask = layer_inputs(c, dtype=torch.float64)
        x.requires_grad_(True)
        edge = conn if "adj" in c["inputs"] else w
        edge.requires_grad_(True)
        out = conv(x, conn, w, mask)
        torch.testing.assert_close(out, c["f64"]["out"], rtol=1e-11, atol=1e-11)
        leaves = {"x": x, "weight": conv.weight, "bias": conv.bias, ("adj" if "adj" in c["inputs"] else "edge_weight"): edge}
        got = torch.autograd.grad(out, list(leaves.values()), c["f64"]["upstream"])
        for (leaf, _), g in zip(leaves.items(), got):  # (the dense case: adj needs a gradient -> the matrix form)
            torch.testing.assert_close(g, c["f64"]["grads"][leaf], rtol=1e-9, atol=1e-10, msg=lambda m: f"{name}/{leaf}: {m}")


def test_native_entries_reject_bad_arguments_without_a_gpu():
    from tgp import _native
    lib = _native.lib()
    d = (ctypes.c_int64 * 4)()
    p = ctypes.addressof(d)
    big = 1 << 31
    # forward: h, N, C, src_ptr, src_perm, col, w, E, bias, mask, delta, eps, act, out, d, stream
    assert lib.tgp_gtv_edge_fwd_f32(None, 4, 8, p, None, p, None, 3, None, None, 1.0, 1e-3, 1, p, None, None) == -1
    assert b"tgp_gtv_edge_fwd_f32" in lib.tgp_last_error()
    assert lib.tgp_gtv_edge_fwd_f32(p, 4, 8, p, None, p, None, 3, None, None, 1.0, 1e-3, 1, None, None, None) == -1
    assert lib.tgp_gtv_edge_fwd_f32(p, 4, 8, p, None, None, None, 3, None, None, 1.0, 1e-3, 1, p, None, None) == -1
    assert lib.tgp_gtv_edge_fwd_f32(p, 4, 8, p, None, p, None, 3, None, None, 1.0, 1e-3, 7, p, None, None) == -1
    assert lib.tgp_gtv_edge_fwd_f32(p, 4, 0, p, None, p, None, 3, None, None, 1.0, 1e-3, 1, p, None, None) == -1
    assert lib.tgp_gtv_edge_fwd_f32(p, 4, 600, p, None, p, None, 3, None, None, 1.0, 1e-3, 1, p, None, None) == -1
    assert b"distance buffer" in lib.tgp_last_error()
    assert lib.tgp_gtv_edge_fwd_f32(p, big, 8, p, None, p, None, 3, None, None, 1.0, 1e-3, 1, p, None, None) == -4
    assert lib.tgp_gtv_edge_fwd_f32(p, 4, 8, p, None, p, None, big, None, None, 1.0, 1e-3, 1, p, None, None) == -4
    assert lib.tgp_gtv_edge_fwd_f32(p, 4, 32768, p, None, p, None, 3, None, None, 1.0, 1e-3, 1, p, p, None) == -4
    assert lib.tgp_gtv_edge_fwd_f32(None, 0, 8, None, None, None, None, 0, None, None, 1.0, 1e-3, 1, None, None, None) == 0
    # edge terms: h, out, g_out, N, C, src_ptr, src_perm, col, w, E, d, mask, delta, eps, act, g, gw, t, stream
    assert lib.tgp_gtv_edge_bwd_terms_f32(p, p, None, 4, 8, p, None, p, None, 3, p, None, 1.0, 1e-3, 1, p, None, p, None) == -1
    assert b"tgp_gtv_edge_bwd_terms_f32" in lib.tgp_last_error()
    assert lib.tgp_gtv_edge_bwd_terms_f32(p, p, p, 4, 8, p, None, p, None, 3, None, None, 1.0, 1e-3, 1, p, None, p, None) == -1
    assert lib.tgp_gtv_edge_bwd_terms_f32(p, p, p, 4, 8, p, None, p, None, 3, p, None, 1.0, 1e-3, 1, p, None, None, None) == -1
    assert lib.tgp_gtv_edge_bwd_terms_f32(p, p, p, 4, 32768, p, None, p, None, 3, p, None, 1.0, 1e-3, 1, p, None, p, None) == -4
    assert lib.tgp_gtv_edge_bwd_terms_f32(p, p, p, big, 8, p, None, p, None, 3, p, None, 1.0, 1e-3, 1, p, None, p, None) == -4
    assert lib.tgp_gtv_edge_bwd_terms_f32(None, None, None, 0, 8, None, None, None, None, 0, None, None, 1.0, 1e-3, 0, None,
                                          None, None, None) == 0
    # node gradient: h, g, N, C, src_ptr, src_perm, dst_ptr, dst_perm, row, col, w, E, d, t, delta, eps, dh, stream
    assert lib.tgp_gtv_edge_bwd_nodes_f32(p, p, 4, 8, p, None, None, None, p, p, None, 3, p, p, 1.0, 1e-3, p, None) == -1
    assert b"tgp_gtv_edge_bwd_nodes_f32" in lib.tgp_last_error()
    assert lib.tgp_gtv_edge_bwd_nodes_f32(p, p, 4, 8, p, None, p, None, p, p, None, 3, p, p, 1.0, 1e-3, None, None) == -1
    assert lib.tgp_gtv_edge_bwd_nodes_f32(p, p, 4, 8, p, None, p, None, None, p, None, 3, p, p, 1.0, 1e-3, p, None) == -1
    assert lib.tgp_gtv_edge_bwd_nodes_f32(p, p, 4, 8, p, None, p, None, p, p, None, big, p, p, 1.0, 1e-3, p, None) == -4
    assert lib.tgp_gtv_edge_bwd_nodes_f32(p, p, 4, 40000, p, None, p, None, p, p, None, 3, p, p, 1.0, 1e-3, p, None) == -4
    assert lib.tgp_gtv_edge_bwd_nodes_f32(None, None, 0, 8, None, None, None, None, None, None, None, 0, None, None, 1.0,
                                          1e-3, None, None) == 0


def test_wrappers_raise_value_errors_before_any_launch():
    """The wrappers check shapes and dtypes first: a malformed call is a ValueError even on host tensors, where a
    well-formed one is refused for having no device to run on."""
    from tgp import _native
    from tgp import kernels as K
    idx = K.AssignIndex(torch.tensor([0, 1, 2, 2], dtype=torch.int32), None, 2, 3)
    col = torch.tensor([1, 2])
    h = torch.zeros(3, 4)
    for bad in (dict(h=h.double()), dict(h=torch.zeros(3, 8)[:, ::2]), dict(h=torch.zeros(12)), dict(col=col.int()),
                dict(col=torch.tensor([1, 2, 0])), dict(edge_weight=torch.ones(2, 1)), dict(edge_weight=torch.ones(3)),
                dict(edge_weight=torch.ones(2, dtype=torch.float64)), dict(bias=torch.zeros(5)),
                dict(mask=torch.ones(3)), dict(mask=torch.ones(2, dtype=torch.bool)), dict(act_code=3),
                dict(by_src=K.AssignIndex(torch.zeros(3, dtype=torch.int32), None, 2, 2))):
        kw = dict(h=h, col=col, edge_weight=None, by_src=idx, bias=None, mask=None, delta=1.0, eps=1e-3, act_code=0)
        kw.update(bad)
        with pytest.raises(ValueError, match="gtv_edge_fwd"):
            K.gtv_edge_fwd(**kw)
    with pytest.raises(ValueError, match="gtv_edge_bwd_terms"):
        K.gtv_edge_bwd_terms(h, h, torch.zeros(3, 5), col, None, idx, torch.zeros(2), None, 1.0, 1e-3, 0)
    with pytest.raises(ValueError, match="gtv_edge_bwd_terms"):
        K.gtv_edge_bwd_terms(h, h, h, col, None, idx, torch.zeros(3), None, 1.0, 1e-3, 0)
    with pytest.raises(ValueError, match="gtv_edge_bwd_nodes"):
        K.gtv_edge_bwd_nodes(h, h, torch.tensor([0, 1, 1]), col, None, idx, idx, torch.zeros(2), torch.zeros(2), 1.0, 1e-3)
    with pytest.raises(ValueError, match="gtv_edge_bwd_nodes"):
        K.gtv_edge_bwd_nodes(h, h, col, col, None, idx, idx, torch.zeros(2), torch.zeros(1), 1.0, 1e-3)
    with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
        K.gtv_edge_fwd(h, col, None, idx, None, None, 1.0, 1e-3, 0)
