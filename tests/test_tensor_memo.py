"""tgp._memo.TensorMemo on host tensors: the hit rule, the store rule and tgp.clear_memos() (no device needed)."""
import gc
import weakref

import torch

import tgp
from tgp import _memo
from tgp import kernels as K
from tgp.select import _NDP_INPUTS
from tgp.utils import ops


def _t(*values):
    return torch.tensor(values or (0, 1, 2))


def test_hit_needs_the_same_live_object_at_the_same_version():
    m = _memo.TensorMemo(16)
    t = _t()
    assert m.get(t) is None and len(m) == 0
    m.put(t, "fact")
    assert m.get(t) == "fact" and len(m) == 1
    assert m.get(t.clone()) is None            # equal values, another object
    t.add_(0)                                  # an in-place op bumps the version counter
    assert m.get(t) is None
    m.put(t, False)
    assert m.get(t) is False and len(m) == 1   # (a stored False is a hit, not a miss)


def test_a_dead_tensors_entry_never_answers_for_a_tensor_that_reuses_its_id():
    m = _memo.TensorMemo(16)
    t = _t()
    old_id, version = id(t), t._version
    m.put(t, "old")
    dead = weakref.ref(t)
    del t
    gc.collect()
    assert dead() is None and len(m) == 0      # the entry went with its tensor
    keep, new = [], None
    for _ in range(2000):                      # the allocator usually hands the address out again at once
        cand = _t()
        if id(cand) == old_id:
            new = cand
            break
        keep.append(cand)
    if new is None:
        new = _t()
    assert m.get(new) is None
    # and had the entry still been there (same id, same version, a reference that no longer resolves): no answer either
    m._d[id(new)] = (dead, version, None, None, None, "old")
    assert new._version == version and len(m) == 1
    assert m.get(new) is None and m.other(new) is None and m.pop(new) is None and len(m) == 0


def test_second_tensor_rule():
    m = _memo.TensorMemo(16)
    t, w, w2 = _t(), _t(1.0, 2.0), _t(1.0, 2.0)
    m.put(t, True, w)
    assert m.get(t, w) is True and m.other(t) is w
    assert m.get(t) is None and m.get(t, None) is None      # stored with weights: not found without
    assert m.get(t, w2) is None                             # equal weights, another object
    w.mul_(1)
    assert m.get(t, w) is None and m.other(t) is w          # the weights changed in place
    m.put(t, True)
    assert m.get(t) is True and m.get(t, w) is None and m.other(t) is None   # stored without: found only without


def test_extra_key_rule():
    m = _memo.TensorMemo(16)
    t = _t()
    m.put(t, True, extra=3)
    assert m.get(t, extra=3) is True and m.get(t, extra=4) is None and m.get(t) is None
    m.put(t, True, extra=4)
    assert m.get(t, extra=4) is True and m.get(t, extra=3) is None and len(m) == 1


def test_capacity_keeps_the_youngest_and_a_restore_makes_young():
    m = _memo.TensorMemo(16)
    ts = [_t(i) for i in range(40)]
    for i, t in enumerate(ts):
        m.put(t, i)
    assert len(m) == 16
    assert [m.get(t) for t in ts] == [None] * 24 + list(range(24, 40))
    m.put(ts[24], "again")                     # the oldest survivor becomes the youngest
    fresh = [_t(i) for i in range(15)]
    for t in fresh:
        m.put(t, True)
    assert len(m) == 16 and m.get(ts[24]) == "again"
    assert all(m.get(t) is None for t in ts[25:]) and all(m.get(t) is True for t in fresh)


def test_dead_entries_go_before_live_ones():
    m = _memo.TensorMemo(16)
    live = _t()
    m.put(live, "live")                        # the OLDEST entry
    dead = [_t(i) for i in range(15)]
    for t in dead:
        m.put(t, True)
    assert len(m) == 16
    del dead, t
    gc.collect()
    assert len(m) == 1                         # (they go with their tensors, before any store)
    new = _t()
    m.put(new, "new")
    assert m.get(live) == "live" and m.get(new) == "new" and len(m) == 2


def test_the_value_of_a_dead_key_is_released_by_the_next_store():
    m = _memo.TensorMemo(16)
    key, value = _t(), torch.zeros(8)
    m.put(key, value)
    value_ref = weakref.ref(value)
    del key, value
    gc.collect()
    other_key = _t()
    m.put(other_key, torch.ones(8))
    gc.collect()
    assert value_ref() is None and len(m) == 1 and m.get(other_key) is not None


def test_discard_pop_and_clear():
    m = _memo.TensorMemo(8)
    a, b = _t(), _t()
    m.put(a, 1)
    m.put(b, 2)
    m.discard(a)
    m.discard(a)                               # (not an error when there is nothing)
    assert m.get(a) is None and len(m) == 1
    assert m.pop(b) == 2 and m.pop(b) is None and len(m) == 0
    m.put(a, 1)
    a.add_(0)
    assert m.pop(a) is None and len(m) == 0    # a stale entry is removed without answering
    m.put(a, 1)
    m.clear()
    assert len(m) == 0 and m.get(a) is None


def test_stamp_helper():
    t = _t()
    s = _memo.stamp(t)
    assert _memo.unchanged(s, t) and not _memo.unchanged(s, t.clone())
    t.add_(0)
    assert not _memo.unchanged(s, t)


def test_clear_memos_empties_every_memo_behind_the_wrappers():
    ei = torch.tensor([[0, 0, 1], [1, 2, 2]])
    w, ptr, batch = torch.ones(3), torch.tensor([0, 3]), torch.tensor([0, 0, 1])
    K.remember_coalesced(ei, 3)
    K._remember_rows_sorted(ei, True)
    K._DECLINED_LISTS.put(ei, True)
    K._HUB_LISTS.put(ei, True)
    K._SYMMETRIC_ADJ.put(ei, True, w)
    K._EDGE_RANGES.put(ei, torch.tensor([0, 3]), ptr)
    K._ROW_OFFSETS.put(ei, torch.tensor([0, 2, 3, 3]), extra=3)
    _NDP_INPUTS.put(ei, (torch.tensor([0, 2, 3, 3]), w), w, 3)
    ops._PREFETCHED_FACTS.put(batch, (0.0, None))
    info = ops.batch_info(batch)
    assert ops.batch_info(batch) is info and info.num_graphs == 2
    assert K.coalesced_memo(ei, 3) and K._rows_sorted_memo(ei) is True and K.sparse_pool_small_declined(ei)
    assert K._adj_symmetric_memo(ei, w) is True and K._edge_ptr_memo(ei, ptr) is not None
    mine = (K._STRICTLY_SORTED, K._SORTED_ROWS, K._DECLINED_LISTS, K._HUB_LISTS, K._SYMMETRIC_ADJ, K._EDGE_RANGES,
            K._ROW_OFFSETS, _NDP_INPUTS, ops._PREFETCHED_FACTS, ops._INFO_OF_BATCH)
    assert all(len(m) >= 1 for m in mine) and all(any(m is r for r in _memo._ALL) for m in mine)
    tgp.clear_memos()
    assert all(len(m) == 0 for m in _memo._ALL)
    assert not K.coalesced_memo(ei, 3) and K._rows_sorted_memo(ei) is None and not K.sparse_pool_small_declined(ei)
    assert K._adj_symmetric_memo(ei, w) is None and K._edge_ptr_memo(ei, ptr) is None
    assert K._HUB_LISTS.get(ei) is None and _NDP_INPUTS.get(ei, w, 3) is None
    again = ops.batch_info(batch)
    assert again is not info and again.num_graphs == 2


def test_rows_sorted_answers_from_the_memo_and_cannot_see_a_write_through_data():
    ei = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    assert K._rows_sorted_memo(ei) is None
    assert K._rows_sorted(ei, ei[0]) is True and K._rows_sorted_memo(ei) is True
    ei.data[0, 0] = 5                          # the version counter does not move: the blind spot clear_memos() is for
    assert not bool((ei[0][1:] >= ei[0][:-1]).all())
    assert K._rows_sorted(ei, ei[0]) is True   # answered from the memo, not computed
    tgp.clear_memos()
    assert K._rows_sorted(ei, ei[0]) is False and K._rows_sorted_memo(ei) is False
    ei[0, 0] = 0                               # an in-place torch operation is seen
    assert K._rows_sorted_memo(ei) is None and K._rows_sorted(ei, ei[0]) is True
