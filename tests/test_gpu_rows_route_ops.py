"""The operators of the dense poolers' un-padded rows route, one at a time, against float64.

The pooler tests reach these ``tgp.kernels`` wrappers only through whole pooler calls at five cluster counts; here
``segment_gemm_tn3`` (with and without the folded post-processing), ``segment_gemm_nn_into``, ``segment_gemm_tn_into`` +
``slab_sum_split``, ``bmm_into``, ``copy_cols2`` / ``copy_cols3``, ``softmax_bwd_ex`` and ``pool_rows_forward`` /
``pool_rows_backward`` are driven directly, at the shapes where their dispatch forks (tests/rows_route_refs.py lists the
cases and what each reaches).

Every comparison: float32 inputs from the host with fixed seeds; the reference is the same operation in plain torch on
their float64 casts, the same code in float32 gives e_oracle32; the error is max|got - ref| / max|ref| PER GRAPH AND PER
OUTPUT and must stay within max(FACTOR e_oracle32, FLOOR) <= CAP (the constants of tests/test_gpu_grad_paths.py).  A block
whose reference is exactly zero (an empty graph) must come out exactly zero.  Identities the code promises ("the same
adds in the same slab order", "the same launches") are asserted bit for bit.  Operands that are column blocks of a wider
buffer sit in 1e30: a load or a store that leaks past its block shows.  Each test prints one line per case."""
import pytest
import torch

import rows_route_refs as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _filled(shape, dev):
    return torch.full(shape, R.BIG, dtype=torch.float32, device=dev)


def _untouched(buf, before, rows, cols):
    """Is every element of ``buf`` outside [rows, cols] (slices of the last two dimensions) bit-identical to ``before``?"""
    keep = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    keep[..., rows, cols] = False
    return torch.equal(_bits(buf)[keep], _bits(before)[keep])


# ========================================================================= 1. S^T [Y0 | Y1 | Y2] and the post-processing
def _tn3_refs(s, ys, sizes, dtype):
    outs = [R.seg_tn_ref(s.to(dtype), y.to(dtype), sizes) for y in ys]
    post = {(fl, tr): R.post_ref(outs[0], fl, tr) for fl in R.POST_FLAGS[1:] for tr in (False, True)}
    return outs, post


def _tn3_runs(w, tag, sd, ysd, ys, s, sizes, ptr, flag_sets):
    """Run the operator for both ``transpose0`` and each flag set; float64 bounds + the bit-for-bit identities."""
    from tgp import kernels as K
    names = ["raw", "x_pool", "gram"][: len(ys)]
    (o64, p64), (o32, p32) = _tn3_refs(s, ys, sizes, torch.float64), _tn3_refs(s, ys, sizes, torch.float32)
    got = {}
    for tr in (False, True):
        for fl in flag_sets:
            word = None if fl is None else K.dense_flags(*fl)
            got[(tr, fl)] = K.segment_gemm_tn3(sd, ysd, ptr, max(sizes), transpose0=tr, post_flags=word)
    torch.cuda.synchronize()
    base = got[(False, None)]
    for (tr, fl), outs in got.items():
        run = f"{tag} transpose0={int(tr)} flags={fl}"
        assert len(outs) == len(ys) + (fl is not None)
        for j, name in enumerate(names):
            tpose = tr and j == 0
            w.add(f"{run} {name}", outs[j], o64[j].transpose(1, 2) if tpose else o64[j],
                  o32[j].transpose(1, 2) if tpose else o32[j])
            want = base[j].transpose(1, 2) if tpose else base[j]
            if not _same_bits(outs[j], want):
                diff = float((outs[j] - want).abs().max())
                w.fail(f"{run}: {name} is not bit-identical to the plain transpose0=0 call's (max |diff| {diff:.3e})")
        if fl is not None:
            w.add(f"{run} adj_pool", outs[-1], p64[(fl, tr)], p32[(fl, tr)])


@pytest.mark.parametrize("name", [c[0] for c in R.TN3_CASES])
def test_segment_gemm_tn3_with_and_without_post(dev, name):
    """raw, x_pool, gram and adj_pool for transpose0 in {0, 1} x the six flag choices; raw(transpose0) = raw^T, and
    x_pool, gram and raw independent of transpose0 and of the flags, bit for bit."""
    from tgp import kernels as K
    sizes, k, f, s, x, ei, ew = R.tn3_case(name)
    n = sum(sizes)
    sd, xd, eid, ewd, ptr = s.to(dev), x.to(dev), ei.to(dev), ew.to(dev), R.ptr_of(sizes).to(dev)
    td = K.spmm_csr(K.csr_offsets(eid, n), eid, ewd, n, sd)
    t = td.cpu()  # Y0 as the operator receives it: float32, an input
    w = R.Worst(f"tn3/{name}")
    blocks = R.blocks_of(sizes)
    w.add("T = A S", td, R.spmm_ref(ei, ew.double(), s.double()), R.spmm_ref(ei, ew, s), blocks)
    _tn3_runs(w, "3 rhs", sd, [td, xd, sd], [t, x, s], s, sizes, ptr, R.POST_FLAGS)
    if name in R.FEWER_RHS_CASES:
        _tn3_runs(w, "1 rhs", sd, [td], [t], s, sizes, ptr, R.POST_FLAGS[:3:2])
        _tn3_runs(w, "2 rhs", sd, [td, xd], [t, x], s, sizes, ptr, R.POST_FLAGS[:3:2])
    w.finish()


# ============================================================================== 2. products on column-block views
def _operand_buffer(k, f, blk, dev):
    """[T | X | 1 0 0 0 | S | T'] written into a buffer that holds 1e30 everywhere first."""
    L = R.view_layout(k, f)
    n = blk["t"].size(0)
    buf = _filled((n, L["ld"]), dev)
    for name in ("t", "x", "s", "v"):
        buf[:, L[name]:L[name] + blk[name].size(1)] = blk[name].to(dev)
    buf[:, L["one"]:L["one"] + 4] = torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev)
    return buf, L


@pytest.mark.parametrize("k,f", R.VIEW_KF)
def test_segment_gemm_nn_into_on_column_blocks(dev, k, f):
    """gS-shaped (a = the T' block, bm = K rows of a taller tensor) and gX-shaped (a = [S | T'] as one 2K-wide view) products
    into a column block of a 1e30 buffer: the block within the bound, everything around it untouched."""
    from tgp import kernels as K
    sizes = R.VIEW_SIZES
    blk, bm, bx = R.view_case(k, f)
    buf, L = _operand_buffer(k, f, blk, dev)
    ptr, blocks, n, B = R.ptr_of(sizes).to(dev), R.blocks_of(sizes), sum(sizes), len(sizes)
    w = R.Worst(f"nn_into/K{k}-F{f}")

    tall = _filled((B, L["ld"], k), dev)
    tall[:, 1:1 + k, :] = bm.to(dev)
    out_buf = _filled((n, L["ld"]), dev)
    before = out_buf.clone()
    cols = slice(L["s"], L["s"] + k)
    K.segment_gemm_nn_into(buf[:, L["v"]:L["v"] + k], tall[:, 1:1 + k, :], ptr, out_buf[:, cols], max(sizes))
    w.add("gS block", out_buf[:, cols], R.seg_nn_ref(blk["v"].double(), bm.double(), sizes),
          R.seg_nn_ref(blk["v"], bm, sizes), blocks)
    if not _untouched(out_buf, before, slice(None), cols):
        w.fail("gS: an element outside the output block changed")

    sv = torch.cat([blk["s"], blk["v"]], 1)
    out_buf = _filled((n, L["ld"]), dev)
    cols = slice(L["x"], L["x"] + f)
    K.segment_gemm_nn_into(buf[:, L["s"]:], bx.to(dev), ptr, out_buf[:, cols], max(sizes))
    w.add("gX block", out_buf[:, cols], R.seg_nn_ref(sv.double(), bx.double(), sizes), R.seg_nn_ref(sv, bx, sizes), blocks)
    if not _untouched(out_buf, before, slice(None), cols):
        w.fail("gX: an element outside the output block changed")
    w.finish()


@pytest.mark.parametrize("k,f", R.VIEW_KF)
def test_segment_gemm_tn_into_and_slab_sum_split(dev, k, f):
    """[gW | gb] = T'^T [X | 1 0 0 0] over row slabs of the operand buffer, then the slab sum: gW = T'^T X, gb = the column
    sums of T', for 1, 7, 8, 9 and 40 slabs."""
    from tgp import kernels as K
    blk, _, _ = R.view_case(k, f)
    buf, L = _operand_buffer(k, f, blk, dev)
    n = blk["v"].size(0)
    x1 = torch.cat([blk["x"], torch.tensor([1.0, 0.0, 0.0, 0.0]).expand(n, 4)], 1)
    w = R.Worst(f"tn_into+slab_sum/K{k}-F{f}")
    for slabs in R.SLAB_COUNTS:
        sp = R.slab_ptr(n, slabs)
        sl = (sp[1:] - sp[:-1]).tolist()
        part = K.segment_gemm_tn_into(buf[:, L["v"]:], buf[:, L["x"]:L["x"] + f + 4], sp.to(dev))
        assert tuple(part.shape) == (slabs, k, f + 4)
        w.add(f"{slabs} slabs: part", part, R.seg_tn_ref(blk["v"].double(), x1.double(), sl), R.seg_tn_ref(blk["v"], x1, sl))
        gw, gb = K.slab_sum_split(part, f)
        w.add(f"{slabs} slabs: gw", gw[None], (blk["v"].double().t() @ blk["x"].double())[None],
              (blk["v"].t() @ blk["x"])[None])
        w.add(f"{slabs} slabs: gb", gb[None], blk["v"].double().sum(0)[None], blk["v"].sum(0)[None])
        gw1, none = K.slab_sum_split(part, f, want_gb=False)
        none2, gb1 = K.slab_sum_split(part, f, want_gw=False)
        if none is not None or none2 is not None or not _same_bits(gw1, gw) or not _same_bits(gb1, gb):
            w.fail(f"{slabs} slabs: slab_sum_split with one output differs from the call with both")
    w.finish()


@pytest.mark.parametrize("G,M,Nc,Kd", R.BMM_SHAPES)
def test_bmm_into_on_views(dev, G, M, Nc, Kd):
    """out (+)= op(a) b with all three as interior views of 1e30 buffers, trans_a x accumulate."""
    from tgp import kernels as K
    a, b, c = R.bmm_case(G, M, Nc, Kd)
    w = R.Worst(f"bmm_into/G{G}-M{M}-N{Nc}-Kd{Kd}")
    for trans_a in (False, True):
        for acc in (False, True):
            ar, ac = (Kd, M) if trans_a else (M, Kd)
            a_buf, b_buf, o_buf = _filled((G, ar + 3, ac + 5), dev), _filled((G, Kd + 2, Nc + 3), dev), _filled((G, M + 2, Nc + 6), dev)
            av, bv = a_buf[:, 2:2 + ar, 3:3 + ac], b_buf[:, 1:1 + Kd, 1:1 + Nc]
            rows, cols = slice(1, 1 + M), slice(5, 5 + Nc)
            av.copy_(a.transpose(1, 2) if trans_a else a)
            bv.copy_(b)
            if acc:
                o_buf[:, rows, cols] = c.to(dev)
            before = o_buf.clone()
            K.bmm_into(av, bv, o_buf[:, rows, cols], trans_a=trans_a, accumulate=acc)
            ref64 = a.double() @ b.double() + (c.double() if acc else 0.0)
            ref32 = a @ b + (c if acc else 0.0)
            run = f"trans_a={int(trans_a)} accumulate={int(acc)}"
            w.add(run, o_buf[:, rows, cols], ref64, ref32)
            if not _untouched(o_buf, before, rows, cols):
                w.fail(f"{run}: an element outside the output view changed")
    w.finish()


@pytest.mark.parametrize("k,f,n", [(40, 24, 345), (10, 7, 345), (66, 10, 1), (8, 6, 70)])
def test_copy_cols_write_their_blocks_and_nothing_else(dev, k, f, n):
    """copy_cols3 builds [T | X | 1 0 0 0 | S | .] (16-byte vectors at K 40 F 24, scalar at the others), copy_cols2 then
    drops T' into the last block next to a zero-width source: exact values, the rest of dst untouched."""
    from tgp import kernels as K
    blk = R.view_blocks(k, f, n, seed=k + n)
    L = R.view_layout(k, f)
    t, x, s, v = (blk[c].to(dev) for c in ("t", "x", "s", "v"))
    dst = _filled((n, L["ld"]), dev)
    K.copy_cols3(t, x, s, dst, L["t"], L["x"], L["s"], one_col=L["one"])
    one = torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev).expand(n, 4)
    want = torch.cat([t, x, one, s, _filled((n, k), dev)], 1)
    assert _same_bits(dst, want)
    K.copy_cols2(v, v.new_empty(n, 0), dst, L["v"], L["v"])  # (as the backward places T' = A^T S)
    assert _same_bits(dst, torch.cat([t, x, one, s, v], 1))
    dst = _filled((n, L["ld"]), dev)
    K.copy_cols2(x, s, dst, L["x"], L["s"])  # no [1 0 0 0] block asked for
    big = _filled((n, k), dev)
    assert _same_bits(dst, torch.cat([big, x, _filled((n, 4), dev), s, big], 1))
    dst = _filled((n, L["ld"]), dev)
    K.copy_cols3(t, x.new_empty(n, 0), s, dst, L["t"], L["x"], L["s"])
    assert _same_bits(dst, torch.cat([t, _filled((n, f + 4), dev), s, big], 1))
    print(f"copy_cols/K{k}-F{f}-N{n} | exact")


# ==================================================================================================== 3. softmax_bwd_ex
@pytest.mark.parametrize("k", R.SOFTMAX_K)
def test_softmax_bwd_ex_every_term_subset(dev, k):
    """Padded [B,N,K], un-padded [Ntot,K] with and without ``batch``; every subset of {extra, c1 + deg, entropy}; out
    returned and out as a column block of a 1e30 buffer; the all-zero row of S gives an exactly zero row; no optional term
    = softmax_bwd bit for bit."""
    from tgp import kernels as K
    eps = K.losses_eps()
    w = R.Worst(f"softmax_bwd_ex/K{k}")
    for form, (sizes, padded) in R.SOFTMAX_FORMS.items():
        data = R.softmax_case(form, k)
        graph, blocks, n = R.batch_of(sizes), R.blocks_of(sizes), sum(sizes)
        shape = (len(sizes), padded, k) if padded else (n, k)
        sd, dsd = data["s"].to(dev).view(shape), data["ds"].to(dev).view(shape)
        batch = graph.to(dev) if form == "batch" else None
        for terms in R.SOFTMAX_TERMS:
            refs = [R.softmax_bwd_ex_ref(data["s"].to(dt), data["ds"].to(dt), **R.softmax_args(data, terms, dt),
                                         ent_scale=R.ENT_SCALE, eps=eps, graph=graph) for dt in (torch.float64, torch.float32)]
            a = {name: (None if v is None else v.to(dev)) for name, v in R.softmax_args(data, terms, torch.float32).items()}
            if a["extra"] is not None:
                a["extra"] = a["extra"].view(shape)
            kw = dict(extra=a["extra"], c1=a["c1"], deg=a["deg"], ent_g=a["ent_g"],
                      ent_scale=R.ENT_SCALE if "entropy" in terms else 0.0, batch=batch)
            run = f"{form} {'+'.join(terms) or 'plain'}"
            got = K.softmax_bwd_ex(sd, dsd, **kw)
            assert got.shape == sd.shape
            w.add(run, got.reshape(n, k), refs[0], refs[1], blocks)
            if not torch.equal(got.reshape(n, k)[2], torch.zeros(k, device=dev)):
                w.fail(f"{run}: the all-zero row of S does not give an exactly zero row")
            wide = _filled((n, 2 * k + 7), dev)
            before = wide.clone()
            cols = slice(k + 3, 2 * k + 3)
            view = wide[:, cols] if not padded else wide.view(len(sizes), padded, 2 * k + 7)[:, :, cols]
            K.softmax_bwd_ex(sd, dsd, out=view, **kw)
            if not _same_bits(wide[:, cols], got.reshape(n, k)):
                w.fail(f"{run}: the strided output differs from the returned one")
            if not _untouched(wide, before, slice(None), cols):
                w.fail(f"{run}: an element outside the output block changed")
            if not terms and not _same_bits(got, K.softmax_bwd(sd, dsd)):
                diff = float((got - K.softmax_bwd(sd, dsd)).abs().max())
                w.fail(f"{run}: not bit-identical to softmax_bwd (max |diff| {diff:.3e})")
    w.finish()


@pytest.mark.parametrize("k", [16, 17, 24, 32, 33, 64])
def test_softmax_bwd_ex_without_terms_is_softmax_bwd_on_many_rows(dev, k):
    """The bit-for-bit identity again on 4099 rows, at every K where either kernel changes its lane-group width (16 lanes
    per row up to some K, 64 above): a different order of adds in one of the two shows on some row."""
    from tgp import kernels as K
    g = torch.Generator().manual_seed(k)
    s = torch.softmax(2.0 * torch.randn(4099, k, generator=g), -1).to(dev)
    ds = torch.randn(4099, k, generator=g).to(dev)
    got, want = K.softmax_bwd_ex(s, ds), K.softmax_bwd(s, ds)
    rows = int((_bits(got) != _bits(want)).any(-1).sum())
    print(f"softmax_bwd_ex == softmax_bwd/K{k} | rows that differ: {rows} of 4099")
    assert rows == 0


# ============================================================================ 4. one native call = the composed operators
def _pool_batch(sizes, f, seed):
    """A sorted batch with a mirrored, unit-weight list (A = A^T: the training step's one-call backward takes it)."""
    from test_gpu_unbatched_dense import _batch
    return _batch(sizes, f, 8.0, seed=seed, weighted=False)


def _pool_runs(pooler, x, ei, batch, dev):
    """Inference outputs and one training step's gradients of a pooler call, as a dict of tensors."""
    lins = pooler.selector.mlp.lins
    args = dict(adj=ei.to(dev), batch=batch.to(dev))
    out = {}
    pooler.eval()
    with torch.no_grad():
        o = pooler(x=x.to(dev), **args)
    out.update(s=o.so.s, x=o.x, adj=o.edge_index)
    for i, v in enumerate(o.loss.values()):
        out[f"loss{i + 1}"] = v
    pooler.train()
    pooler.zero_grad(set_to_none=True)
    xg = x.to(dev).requires_grad_(True)
    o = pooler(x=xg, **args)
    g = torch.Generator().manual_seed(5)
    wx, wa = torch.randn(o.x.shape, generator=g).to(dev), torch.randn(o.edge_index.shape, generator=g).to(dev)
    l1, l2 = list(o.loss.values())
    ((o.x * wx).sum() + (o.edge_index * wa).sum() + 0.7 * l1 + 1.3 * l2).backward()
    out.update(train_x=o.x.detach(), train_adj=o.edge_index.detach(), train_loss1=l1.detach(), train_loss2=l2.detach(),
               dX=xg.grad.clone())
    for i, lin in enumerate(lins):  # (every layer of the selector: one, or two with a hidden layer)
        out.update({f"dW{i}": lin.weight.grad.clone(), f"db{i}": lin.bias.grad.clone()})
    torch.cuda.synchronize()
    return out


ONE_CALL_CASES = [  # alias, graph sizes, K, F or [F, hidden width], rows-route density to force (batched poolers)
    ("mincut_u", [130, 97, 160], 40, 24, None),
    ("diff_u", [130, 97, 160], 40, 24, None),
    ("mincut_u", [700, 90], 80, 33, None),
    ("diff_u", [700, 90], 80, 33, None),
    ("mincut", [260, 199], 72, 16, 2.0),
    ("mincut_u", [130, 97], 40, [24, 8], None),  # a hidden layer: S is handed to the native call and to the node
    ("diff", [260, 199], 72, [16, 8], 2.0),
]


@pytest.mark.parametrize("alias,sizes,k,f,density", ONE_CALL_CASES)
def test_one_native_call_equals_the_composed_operators(dev, monkeypatch, alias, sizes, k, f, density):
    """kernels.pool_rows_forward / pool_rows_backward make the launches of the operator-by-operator path
    (csrc/pool_rows.cpp): so.s, x, adj, both losses in inference and dX, dW, db of a training step are bit-identical with
    ``_POOL_ROWS_ONE_CALL`` on and off.  The spies make sure the two runs really took the two paths.  With a hidden layer
    the selector runs in front and hands S over: the forward's one call takes it, the backward's is not asked."""
    import tgp.poolers as P
    from tgp import kernels as K
    from tgp.poolers import get_pooler
    if density is not None:
        monkeypatch.setattr(P, "_ROWS_ROUTE_DENSITY", density)
    took = {"fwd": 0, "bwd": 0}
    fwd, bwd = K.pool_rows_forward, K.pool_rows_backward

    def spy(name, fn):
        def call(*a, **kw):
            r = fn(*a, **kw)
            took[name] += r is not None
            return r
        return call

    monkeypatch.setattr(K, "pool_rows_forward", spy("fwd", fwd))
    monkeypatch.setattr(K, "pool_rows_backward", spy("bwd", bwd))
    hidden = isinstance(f, list)
    x, ei, _, batch = _pool_batch(sizes, f[0] if hidden else f, seed=sum(sizes) + k)
    pooler = get_pooler(alias, in_channels=f, k=k).to(dev)
    want = {"fwd": 2, "bwd": 0 if hidden else 1}  # inference, training forward, training backward
    monkeypatch.setattr(K, "_POOL_ROWS_ONE_CALL", True)
    one = _pool_runs(pooler, x, ei, batch, dev)
    assert took == want, took
    monkeypatch.setattr(K, "_POOL_ROWS_ONE_CALL", False)
    composed = _pool_runs(pooler, x, ei, batch, dev)
    assert took == want, took  # (the composed run took none)
    differ = [f"{name} (max |diff| {float((one[name] - composed[name]).abs().max()):.3e})"
              for name in one if not _same_bits(one[name], composed[name])]
    print(f"one_call/{alias}-K{k}-F{f} | {len(one)} values compared bit for bit | differ: {differ or 'none'}")
    assert not differ, differ


_COMPOSED_SIZES, _COMPOSED_K, _COMPOSED_F = [30, 80, 50], 5, 7


@pytest.mark.parametrize("selector", [False, True], ids=["s_given", "selector"])
@pytest.mark.parametrize("transposed", [False, True], ids=["plain", "transposed"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_composed_forward_equals_the_one_native_call(dev, mode, transposed, selector):
    """kernels.pool_rows_forward_composed makes the launches of kernels.pool_rows_forward one operator at a time
    (csrc/pool_rows.cpp: "the same launches"): the two dicts have the same keys and every value is bit-identical, for the
    three loss modes, both orientations of the pooled adjacency, S handed in and S from the selector's Linear."""
    from tgp import kernels as K
    sizes, k, f = _COMPOSED_SIZES, _COMPOSED_K, _COMPOSED_F
    from test_gpu_unbatched_dense import _batch
    x, ei, ew, _ = _batch(sizes, f, 6.0, seed=17)  # row-sorted and duplicate-free, a random weight per direction
    n = sum(sizes)
    g = torch.Generator().manual_seed(23)
    weight, bias = (0.5 * torch.randn(k, f, generator=g)).to(dev), (0.1 * torch.randn(k, generator=g)).to(dev)
    xd, eid, w, ptr = x.to(dev), ei.to(dev), ew.to(dev), R.ptr_of(sizes).to(dev)
    s = None if selector else torch.softmax(xd @ weight.t() + bias, -1)
    args = (xd, weight if selector else None, bias if selector else None, s, K.csr_offsets(eid, n), eid, w, ptr, max(sizes),
            transposed, K.dense_flags(True, True, transposed, False), mode, (1.0 / n, 0.5 / n), float(torch.dot(ew, ew)))
    one, composed = K.pool_rows_forward(*args), K.pool_rows_forward_composed(*args)
    torch.cuda.synchronize()
    assert one is not None and set(one) == set(composed), (one and sorted(one), sorted(composed))
    differ = [name for name in one if (one[name] is None) != (composed[name] is None)
              or (one[name] is not None and not _same_bits(one[name], composed[name]))]
    print(f"composed/mode{mode}-transposed{int(transposed)}-selector{int(selector)} | {len(one)} values compared bit for bit"
          f" | differ: {differ or 'none'}")
    assert not differ, differ
