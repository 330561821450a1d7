"""The row operand of the native wrappers (``kernels._row_operand``): the wrappers that convert take any float dtype and
any row-strided view and give the float64 answer exactly on small-integer data; the wrappers that refuse keep refusing;
a failed native call is reported under the symbol that was called."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F = 5  # odd: no 16-byte row path
LAYOUTS = ("contiguous", "column_slice", "float64", "float16")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _as_layout(x32: torch.Tensor, layout: str, dev) -> torch.Tensor:
    """``x32`` [rows, 5] on the device as one of the operand forms the wrappers meet; the values are unchanged (the callers
    pass small integers, or accept the rounding of float16)."""
    if layout == "contiguous":
        return x32.to(dev)
    if layout == "column_slice":  # row stride 8, base 4 bytes off a 16-byte boundary, other columns poisoned
        buf = torch.full((x32.size(0), 8), 1000.0, device=dev)
        buf[:, 1:6] = x32.to(dev)
        return buf[:, 1:6]
    return x32.to(dev, torch.float64 if layout == "float64" else torch.float16)


def _ints(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=g).to(torch.float32)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows", [65, 1])
def test_converting_wrappers_are_exact_on_small_integers(dev, rows, layout):
    """row_dot, weighted_colsum and edge_contract_raw on integer-valued x, w in [-8, 8]: every product and partial sum is
    exact in float16, float32 and float64, so the result equals the float64 expression bit for bit."""
    from tgp import kernels as K
    x32, w, gvec = _ints((rows, F), 1000 + rows), _ints((F,), 7), _ints((rows,), 11)
    x = _as_layout(x32, layout, dev)
    x64 = x32.double()

    got = K.row_dot(x, w.to(dev))
    assert got.dtype == torch.float32 and torch.equal(got.double().cpu(), (x64 * w.double()).sum(-1))

    got = K.weighted_colsum(x, gvec.to(dev))
    assert got.dtype == torch.float32 and torch.equal(got.double().cpu(), (gvec.double()[:, None] * x64).sum(0))

    g = torch.Generator().manual_seed(rows)
    ei = torch.randint(0, rows, (2, 12), generator=g)
    w2, bias = _ints((2 * F,), 13), torch.tensor([3.0])
    got = K.edge_contract_raw(x, ei.to(dev), w2.to(dev), bias.to(dev))
    want = (x64[ei[0]] * w2[:F].double()).sum(-1) + (x64[ei[1]] * w2[F:].double()).sum(-1) + 3.0
    assert got.dtype == torch.float32 and torch.equal(got.double().cpu(), want)


@pytest.mark.parametrize("tanh", [True, False])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows", [65, 1])
def test_topk_score_converts_and_keeps_its_tolerance(dev, rows, layout, tanh):
    """topk_score divides and takes tanh: random inputs, the tolerance of test_gpu_topk's kernel test, against float64 of
    the float32-rounded input (float16 and float32 convert exactly; float64 is rounded once, by the wrapper)."""
    from tgp import kernels as K
    g = torch.Generator().manual_seed(50 + rows)
    x = _as_layout(torch.randn(rows, F, generator=g), layout, dev)
    w = torch.randn(1, F, generator=g).to(dev)
    xr = x.to(torch.float32).double()
    want = (xr * w.double()).sum(-1) / w.double().norm(p=2, dim=-1)
    want = torch.tanh(want) if tanh else want
    got = K.topk_score(x, w, tanh)
    assert got.dtype == torch.float32
    assert torch.allclose(got.double(), want, rtol=1e-5, atol=1e-6)


def test_topk_select_takes_float64_features(dev):
    """TopkSelect on float64 device features (the score goes through row_dot): no error, and exactly the top-k nodes of
    the float64 score.  x_i = c_i w / ||w|| gives score_i = tanh(c_i) with the c_i 1/16 apart: no near-tie."""
    from tgp.select import TopkSelect
    sel = TopkSelect(in_channels=F, ratio=0.5).to(dev)
    w = sel.weight.detach().double().reshape(-1)
    g = torch.Generator().manual_seed(3)
    c = ((torch.randperm(65, generator=g) - 32).double() / 16).to(dev)
    x = c[:, None] * (w / w.norm())
    with torch.no_grad():
        so = sel(x)
    score = torch.tanh((x * w).sum(-1) / w.norm())
    k = 33  # ceil(0.5 * 65)
    want = torch.sort(torch.topk(score, k).indices).values
    assert so.num_supernodes == k
    assert torch.equal(so.node_index, want)


def test_strict_wrappers_still_refuse_float64(dev):
    from tgp import kernels as K
    x = torch.zeros(65, F, dtype=torch.float64, device=dev)
    ptr = torch.tensor([0, 65], device=dev)
    with pytest.raises(ValueError, match="segment readout expects float32"):
        K.segment_aggr(x, K.segment_ops_mask(["sum"]), 1, 65, ptr=ptr)
    groups = K.build_assign_index(torch.zeros(65, dtype=torch.long, device=dev), 1)
    theta = torch.ones(65, 2, device=dev)
    with pytest.raises(ValueError, match="eigenpool_reduce expects float32"):
        K.eigenpool_reduce(theta, groups, x)
    with pytest.raises(ValueError, match="eigenpool_reduce expects float32"):
        K.eigenpool_reduce(theta.double(), groups, x.float())


def test_a_failed_call_is_reported_under_its_own_symbol(dev):
    """bmm_into(accumulate=True) calls tgp_bmm_accumulate_f32; a row count beyond the library's int32 range is refused
    by its argument checks, before anything is launched (the views below alias one element each: nothing that large
    exists)."""
    from tgp import kernels as K
    from tgp import _native as N
    big = 1 << 31
    one = torch.zeros(1, device=dev)
    a = one.as_strided((1, big, 1), (0, 0, 1))
    out = torch.zeros(1, device=dev).as_strided((1, big, 1), (0, 0, 1))
    b = torch.zeros(1, 1, 1, device=dev)
    with pytest.raises(N.TgpNativeError, match="tgp_bmm_accumulate_f32 failed"):
        K.bmm_into(a, b, out, accumulate=True)
    with pytest.raises(N.TgpNativeError, match="tgp_bmm_f32 failed"):
        K.bmm_into(a, b, out)
