"""The hub route's host side without a GPU: the plan builder against a host argsort on hand-made offsets, the new
entries of the C ABI and their refusals.  Without the feature this module fails at the first missing wrapper."""
import ctypes

import pytest
import torch

from tgp import _native
from tgp import kernels as K

ENTRIES = ["tgp_hubwalk_attend_f32", "tgp_hubwalk_chunk", "tgp_hubwalk_edge_dot_f32", "tgp_hubwalk_edge_softmax_f32",
           "tgp_hubwalk_query_bwd_f32", "tgp_hubwalk_query_f32", "tgp_hubwalk_scalar_f32",
           "tgp_hubwalk_softmax_bwd_f32", "tgp_hubwalk_workspace_bytes"]


def index_of(lens, shuffled):
    """An AssignIndex over a hand-made list: group i owns lens[i] positions (a stable argsort when ``shuffled``)."""
    tgt = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))
    if shuffled:
        tgt = tgt[torch.randperm(tgt.numel(), generator=torch.Generator().manual_seed(3))]
    ptr = torch.zeros(len(lens) + 1, dtype=torch.int32)
    ptr[1:] = torch.cumsum(torch.tensor(lens), 0)
    perm = torch.argsort(tgt, stable=True).to(torch.int32) if shuffled else None
    return K.AssignIndex(ptr, perm, tgt.numel(), len(lens)), tgt


@pytest.mark.parametrize("shuffled", [False, True])
def test_the_plan_against_a_host_argsort(shuffled):
    lens, mg, C = [9, 0, 8, 3, 17, 8, 1, 10], 8, 4  # 8 entries: exactly the threshold, not a hub; 9: one
    grp, tgt = index_of(lens, shuffled)
    plan = K.build_hub_plan(grp, min_group=mg, chunk=C)
    assert plan.hub_ids.tolist() == [0, 4, 7] and plan.hub_ids.dtype == torch.int32
    assert plan.chunk_ptr.tolist() == [0, 3, 8, 11] and plan.chunks == 11 and plan.H == 3  # ceil(9/4), ceil(17/4), ceil(10/4)
    light = plan.light
    assert light.row_ptr.tolist() == [0, 0, 0, 8, 11, 11, 19, 20, 20] and light.nnz == grp.nnz
    order = torch.argsort(tgt, stable=True)
    keep = order[~torch.isin(tgt[order], plan.hub_ids.long())]  # the surviving positions, in the order they had
    assert light.perm.tolist() == keep.tolist() and light.perm.dtype == torch.int32


def test_no_hub_gives_no_plan():
    grp, _ = index_of([3, 8, 8, 0], False)
    assert K.build_hub_plan(grp, min_group=8, chunk=4) is None  # the longest group has exactly the threshold
    assert K.build_hub_plan(grp) is None and grp.hub is None  # the whole list is shorter than HUB_MIN_GROUP
    assert K.HUB_MIN_GROUP >= 4096 and K.hub_chunk() == _native.lib().tgp_hubwalk_chunk() > 0


def test_the_entries_are_declared_and_refuse():
    assert sorted(n for n in _native.SIGNATURES if n.startswith("tgp_hubwalk_")) == ENTRIES
    lib = _native.lib()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    big, q = 1 << 31, p + 1024
    assert lib.tgp_hubwalk_workspace_bytes(0, 8) == 0 and lib.tgp_hubwalk_workspace_bytes(3, 0) >= 3 * 16
    assert lib.tgp_hubwalk_workspace_bytes(3, 5) >= 2 * 3 * 5 * 4 + 3 * 16
    # (grp_ptr, grp_perm, src, hub_ids, chunk_ptr, H, T | ...): an empty plan is 0 whatever else is handed over
    assert lib.tgp_hubwalk_scalar_f32(None, None, None, None, None, 0, 0, None, None, None, None, None, 4, 4, 0, 0, 0,
                                      None, None, None, 0, None) == 0
    assert lib.tgp_hubwalk_query_f32(None, None, None, None, None, 0, 0, None, 0, None, None, 4, 4, 8, None, None, None,
                                     0, None) == 0
    assert lib.tgp_hubwalk_edge_dot_f32(None, None, None, None, None, 0, 0, None, None, 0, 4, 4, 8, None, None) == 0
    assert lib.tgp_hubwalk_scalar_f32(None, None, None, None, None, 0, 0, None, None, None, None, None, 4, 4, 0, 0, 7,
                                      None, None, None, 0, None) == 0  # ... an unknown act included
    scalar = lambda *a: lib.tgp_hubwalk_scalar_f32(*a)  # noqa: E731
    ok = [p, None, p, p, p, 1, 1, None, q, None, None, None, 4, 4, 0, 0, 0, None, p, p, 64, None]
    for at, value, want in [(0, None, -1), (3, None, -1), (4, None, -1), (8, None, -1), (18, None, -1), (19, None, -1),
                            (20, 8, -1), (18, q, -1), (16, 3, -1), (12, big, -4), (13, big, -4), (5, big + 1, -4)]:
        args = list(ok)
        args[at] = value
        assert scalar(*args) == want, (at, value)
    assert b"tgp_hubwalk_scalar_f32" in lib.tgp_last_error()
    # the row entries: a row stride below F, no workspace, the input as the output
    assert lib.tgp_hubwalk_query_f32(p, None, p, p, p, 1, 1, p, 4, p, p, 4, 4, 8, p, None, p, 4096, None) == -1
    assert lib.tgp_hubwalk_query_f32(p, None, p, p, p, 1, 1, p, 8, p, p, 4, 4, 8, p, None, None, 0, None) == -1
    assert lib.tgp_hubwalk_attend_f32(p, None, p, p, p, 1, 1, None, q, 8, None, 4, 4, 4, 8, q, None, p, 4096, None) == -1
    assert lib.tgp_hubwalk_edge_softmax_f32(p, None, p, p, p, 1, 1, q, p, 4, 4, 0.2, q, p, 4096, None) == -1
    assert lib.tgp_hubwalk_softmax_bwd_f32(p, None, p, p, p, 1, 1, q, p, p, p, 4, 4, 0.2, q, p, p, 4096, None) == -1
    assert lib.tgp_hubwalk_query_bwd_f32(p, None, p, p, p, 1, big + 1, p, p, p, 4, 4, 8, q, p, 4096, None) == -4
