"""The readout's public interface without a GPU: signatures and reprs, alias resolution, every error path the
reference has, the missing CPU fallback of the native aggregations, a user module on the composed route with host
tensors, and the kernel entry points' argument checks."""
import ctypes
import inspect

import pytest
import torch

import readout_restatement as R

from tgp import _native
from tgp.reduce import (Aggregation, AggrReduce, GlobalReduce, MaxAggregation, MeanAggregation, MinAggregation,
                        MultiAggregation, Reduce, SumAggregation, get_aggr, resolve_reduce_op)
from tgp.reduce.aggr import native_ops
from tgp.reduce.get_aggr import _AGGR_ALIASES
from tgp.select import SelectOutput


class SquareSum(Aggregation):
    """A user aggregation: nothing the kernels know, so AggrReduce calls it after the reference's stable sort."""

    def forward(self, x, index=None, ptr=None, dim_size=None, dim=0):
        assert bool((index[1:] >= index[:-1]).all()), "the composed route sorts by index first"
        return x.new_zeros(dim_size, x.size(1)).index_add_(0, index, x * x)


def test_signatures_and_reprs():
    assert list(inspect.signature(AggrReduce.__init__).parameters) == ["self", "aggr"]
    p = inspect.signature(AggrReduce.forward).parameters
    assert list(p)[:3] == ["self", "x", "so"] and p["so"].default is None
    assert p["batch"].kind is inspect.Parameter.KEYWORD_ONLY and p["size"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(GlobalReduce.forward).parameters) == ["self", "x", "batch", "size", "mask"]
    assert inspect.signature(GlobalReduce.__init__).parameters["reduce_op"].default == "sum"
    call = inspect.signature(SumAggregation.forward).parameters
    assert list(call) == ["self", "x", "index", "ptr", "dim_size", "dim"] and call["dim"].default == 0
    assert issubclass(GlobalReduce, AggrReduce) and issubclass(AggrReduce, Reduce)
    assert repr(GlobalReduce()) == "GlobalReduce(aggr=SumAggregation())"
    assert repr(AggrReduce(MeanAggregation())) == "AggrReduce(aggr=MeanAggregation())"
    assert repr(MultiAggregation(["sum", MaxAggregation()])) == \
        "MultiAggregation([\n  SumAggregation(),\n  MaxAggregation(),\n], mode=cat)"


def test_aliases_resolve_as_in_the_reference():
    for alias, cls in ((" Sum ", SumAggregation), ("MEAN", MeanAggregation), ("max", MaxAggregation),
                       ("min", MinAggregation)):
        assert type(get_aggr(alias)) is cls
        assert type(get_aggr(alias, in_channels=8, processing_steps=3)) is cls  # kwargs the class does not take are dropped
    multi = get_aggr("multi", aggrs=["sum", "mean", "max"], in_channels=4)
    assert native_ops(multi) == ("sum", "mean", "max")
    assert native_ops(MultiAggregation([MinAggregation(), "sum"])) == ("min", "sum")
    assert native_ops(SquareSum()) is None and native_ops(MultiAggregation([SquareSum(), "sum"])) is None
    assert len(_AGGR_ALIASES) == 26
    with pytest.raises(ValueError, match="Unknown aggregator alias: 'nope'"):
        get_aggr("nope")
    for alias in sorted(set(_AGGR_ALIASES) - {"sum", "mean", "max", "min", "multi"}):
        with pytest.raises(NotImplementedError, match=alias):
            get_aggr(alias.replace("_", "-").upper(), in_channels=4)
    with pytest.raises(NotImplementedError, match="mode"):
        MultiAggregation(["sum", "max"], mode="proj")
    agg = MaxAggregation()
    assert resolve_reduce_op(agg) is agg and type(resolve_reduce_op("min")) is MinAggregation
    with pytest.raises(TypeError, match="reduce_op must be a string alias or a PyG Aggregation instance"):
        resolve_reduce_op(3)
    with pytest.raises(TypeError, match="aggr must be a PyG Aggregation"):
        AggrReduce(torch.nn.Linear(2, 2))
    assert type(GlobalReduce("multi", aggrs=["max", "min"]).aggr) is MultiAggregation


def test_error_paths_of_the_reference():
    x2, x3 = torch.randn(6, 3), torch.randn(2, 3, 3)
    g = GlobalReduce(SquareSum())
    with pytest.raises(ValueError, match="readout expects x to be 2D"):
        g(torch.randn(6))
    with pytest.raises(ValueError, match="mask must have shape"):
        g(x3, mask=torch.ones(2, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="mask is only supported for dense x"):
        g(x2, mask=torch.ones(2, 3, dtype=torch.bool))
    with pytest.raises(ValueError, match="size is only supported for sparse readout when batch is provided"):
        g(x2, size=2)
    with pytest.raises(ValueError, match="Readout mode expects x to be 2D"):
        AggrReduce(SquareSum())(torch.randn(2, 2, 2, 2))
    with pytest.raises(ValueError, match="AggrReduce supports only sparse SelectOutput assignments"):
        AggrReduce(SumAggregation())(x2, SelectOutput(s=torch.rand(6, 2)))


def test_native_aggregations_have_no_cpu_fallback():
    x, batch = torch.randn(6, 3), torch.tensor([0, 0, 1, 1, 2, 2])
    so = SelectOutput(cluster_index=torch.tensor([0, 0, 1, 1, 2, 2]))
    for aggr in (SumAggregation(), MeanAggregation(), MaxAggregation(), MinAggregation(), MultiAggregation(["sum", "max"])):
        with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
            aggr(x, index=batch, dim_size=3)
        with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
            GlobalReduce(aggr)(x, batch=batch)
        with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
            GlobalReduce(aggr)(x.view(2, 3, 3), mask=torch.ones(2, 3, dtype=torch.bool))
        with pytest.raises(_native.TgpNativeError, match="no CPU fallback"):
            AggrReduce(aggr)(x, so)


def test_a_user_module_runs_the_composed_route_on_host_tensors():
    x, batch = torch.randn(7, 3), torch.tensor([2, 0, 1, 0, 2, 2, 1])
    want = torch.zeros(4, 3).index_add_(0, batch, x * x)
    out, bp = AggrReduce(SquareSum())(x, batch=batch, size=4)
    torch.testing.assert_close(out, want)
    assert torch.equal(bp, torch.arange(4))
    torch.testing.assert_close(GlobalReduce(SquareSum())(x), (x * x).sum(0, keepdim=True))
    mask = torch.tensor([[True, False, True], [False, False, False]])
    x3 = torch.randn(2, 3, 3)
    torch.testing.assert_close(GlobalReduce(SquareSum())(x3, mask=mask),
                               torch.stack([(x3[0, [0, 2]] ** 2).sum(0), torch.zeros(3)]))
    so = SelectOutput(cluster_index=torch.tensor([1, 0, 1, 0, 2, 2, 1]), weight=torch.rand(7) + 0.5,
                      batch=torch.tensor([0, 0, 0, 0, 1, 1, 0]))
    out, bp = AggrReduce(SquareSum())(x, so)
    src = x[so.node_index] * so.weight.view(-1, 1)
    torch.testing.assert_close(out, torch.zeros(3, 3).index_add_(0, so.cluster_index, src * src))
    assert bp.tolist() == [0, 0, 1]


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _native.lib()
    d = (ctypes.c_int64 * 4)()
    p = ctypes.addressof(d)
    none5 = [None, None, None, None]  # row_ptr, perm, node_index, weight
    fwd = lib.tgp_segment_aggr_f32
    assert fwd(p, 4, 4, 4, p, 0, None, *none5, 0, 1, 4, 0, p, None, None, None, 0, None) == -1  # no operation
    assert b"tgp_segment_aggr_f32" in lib.tgp_last_error()
    assert fwd(p, 4, 4, 4, p, 0, None, *none5, 0, 1, 4, 32, p, None, None, None, 0, None) == -1  # an unknown bit (mul)
    assert fwd(p, 4, 4, 4, None, 0, None, *none5, 0, 1, 4, 1, p, None, None, None, 0, None) == -1  # no row source
    assert fwd(p, 4, 4, 4, p, 2, None, *none5, 0, 2, 4, 1, p, None, None, None, 0, None) == -1  # two row sources
    assert fwd(p, 4, 4, 4, p, 0, p, *none5, 0, 1, 4, 1, p, None, None, None, 0, None) == -1  # a mask without the dense layout
    assert fwd(p, 4, 4, 2, p, 0, None, *none5, 0, 1, 4, 1, p, None, None, None, 0, None) == -1  # row stride below F
    assert fwd(p, 6, 4, 4, None, 2, None, *none5, 0, 2, 2, 1, p, None, None, None, 0, None) == -1  # G * nodes != rows
    assert fwd(p, 4, 4, 4, None, 0, None, None, None, p, None, 3, 2, 1, 1, p, None, None, None, 0, None) == -1  # one-to-one: nnz != G
    assert fwd(p, 4, 4, 4, p, 0, None, *none5, 0, 1, 4, 1, None, None, None, None, 0, None) == -1  # no output
    assert fwd(p, 1 << 31, 4, 4, p, 0, None, *none5, 0, 1, 4, 1, p, None, None, None, 0, None) == -4  # rows beyond int32
    assert fwd(p, 1 << 29, 4, 4, p, 0, None, *none5, 0, 1, 4, 1, p, None, None, None, 0, None) == -4  # N * F beyond int32
    assert fwd(p, 4, 4, 4, p, 0, None, *none5, 0, 1 << 31, 4, 1, p, None, None, None, 0, None) == -4  # G beyond int32
    assert fwd(p, 4, 4, 4, None, 0, None, p, p, p, None, 1 << 31, 2, 1, 1, p, None, None, None, 0, None) == -4  # nnz
    assert fwd(p, 1 << 20, 4, 4, p, 0, None, *none5, 0, 1, 1 << 20, 1, p, None, None, None, 0, None) == -2  # split route, no workspace
    assert b"workspace too small" in lib.tgp_last_error()
    assert fwd(None, 0, 4, 4, p, 0, None, *none5, 0, 0, 0, 1, None, None, None, None, 0, None) == 0  # nothing to do
    bwd = lib.tgp_segment_aggr_bwd_f32
    assert bwd(p, p, 4, 4, 4, None, 0, None, None, None, None, 1, 0, p, None) == -1
    assert bwd(p, p, 4, 4, 4, None, 0, None, None, None, None, 1, 8, p, None) == -1  # max without out / ties
    assert b"tgp_segment_aggr_bwd_f32" in lib.tgp_last_error()
    assert bwd(p, p, 4, 4, 4, None, 0, None, None, None, None, 1, 2, p, None) == -1  # mean without count
    assert bwd(p, p, 4, 4, 4, p, 2, None, None, None, None, 2, 1, p, None) == -1  # batch and dense at once
    assert bwd(p, p, 1 << 31, 4, 4, None, 0, None, None, None, None, 1, 1, p, None) == -4


def test_workspace_query_follows_the_route():
    lib = _native.lib()
    chunk = lib.tgp_segment_aggr_chunk_rows()
    assert chunk >= 64
    q = lib.tgp_segment_aggr_workspace_bytes
    assert q(2048, 32, 1, 60) == 0 and q(1, 128, 1, chunk) == 0  # short segments write the output themselves
    two = q(1, 128, 1, chunk + 1)
    assert two >= 2 * 128 * 4  # two chunk records of one sum slot
    assert q(1, 128, 1 | 8, chunk + 1) >= 2 * 5 * 128 * 4  # sum + (min, max, their tie counts)
    big = q(1, 128, 1 | 2 | 8, 1 << 20)
    assert big >= (1 << 20) // chunk * 5 * 128 * 4 and big < 64 << 20  # one 1M-node graph: 4096 chunks, a few MB
    assert q(100000, 32, 1, 1 << 20) == 0  # that many segments fill the device without a split
    assert q(8, 128, 1, 1 << 22) < 64 << 20  # the number of records is bounded


def test_restatement_of_the_batch_pool_of_a_sparse_assignment():
    c = R.load_cases()["aggr_so_pairs_sum"]
    assert c["expected"]["batch"].tolist() == [0, 0, 0, 0, 1, 1, 1]
