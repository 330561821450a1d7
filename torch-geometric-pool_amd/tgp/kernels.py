"""Tensor-level entry points of the hot path: allocate outputs/workspaces with PyTorch,
hand raw device pointers + the current HIP stream to the C ABI (``include/tgp_hip.h``).

Each function names the reference lines whose arithmetic it replaces.  Nothing here runs
on the CPU and nothing falls back to ATen kernels.
"""
from __future__ import annotations

import ctypes
import os
import threading
from collections import namedtuple
from types import SimpleNamespace
from typing import Optional, Sequence, Tuple
from weakref import ref as _weakref

import torch
from torch import Tensor

from . import _native as N
from ._memo import TensorMemo


_OPS_MODULE = None


def ops_eps() -> float:
    """``tgp.utils.ops.eps`` read at CALL time, as the reference's ops functions read their module global
    (utils/ops.py:21,72,318,377,395; reference tests monkeypatch it: tests/connect/test_dense_conn.py:444-463)."""
    global _OPS_MODULE
    if _OPS_MODULE is None:
        from .utils import ops
        _OPS_MODULE = ops
    return float(_OPS_MODULE.eps)


def losses_eps() -> float:
    from .utils import losses
    return float(losses.eps)


# ------------------------------------------------------------------------- A1 / A2
class AssignIndex:
    """Inverted index of a sparse assignment (supernode -> its assignments, in ascending
    assignment order).  A function of the SelectOutput only, so SelectOutput caches it."""

    __slots__ = ("_row_ptr", "perm", "nnz", "num_targets", "_device", "pack", "pack_key", "member_directory",
                 "member_directory_key", "_max_members")

    def __init__(self, row_ptr: Optional[Tensor], perm: Optional[Tensor], nnz: int, num_targets: int, device=None):
        # row_ptr None: exactly one assignment per target (TopK, NDP) -- the table is arange and the Reduce kernel
        # skips reading it; it is materialised only for a consumer that wants the general form.  perm None (with
        # row_ptr None): target t owns assignment t -- the transposed index of a one-over-K assignment whose
        # node_index is 0..N-1 (Graclus): nothing to build, the kernel reads no table at all
        if row_ptr is None and nnz != num_targets:
            raise ValueError("an AssignIndex without row_ptr must be one-to-one")
        if perm is None and device is None and row_ptr is None:
            raise ValueError("an AssignIndex without perm and row_ptr must name its device")
        self._row_ptr, self.perm, self.nnz, self.num_targets = row_ptr, perm, nnz, num_targets
        # one-to-one indices (TopK, NDP) may carry the PACKED form: pack[c] = {int32 source row, fp32 weight} of target
        # c's single assignment (int64 words), valid for exactly the (source_index, weight) storage named by pack_key =
        # (source_index.data_ptr(), weight.data_ptr() or 0).  It is a snapshot of the selector's own output: like the
        # inverted index itself it is not refreshed if a caller edits S's indices / values in place afterwards.
        self.pack, self.pack_key = None, None
        # r5 (TopkSelect on large graphs): int32 [5 * blocks] = the kept-node bitmap (4 words per 128-node block) followed
        # by the rank directory (kept nodes in front of every block), by-products of the selector's compaction pass that
        # the subgraph Connect of the same selection starts from (tgp_connect_subgraph_single's member_bits_in)
        # ... valid for exactly the node_index storage named by member_directory_key = (data_ptr, length) (a
        # SelectOutput whose S was replaced must not get a Connect relabelled by the stale selection)
        self.member_directory = None
        self.member_directory_key = None
        self._max_members = 1 if row_ptr is None else None
        self._device = perm.device if perm is not None else (row_ptr.device if row_ptr is not None else
                                                              torch.device(device))

    @property
    def one_to_one(self) -> bool:
        return self._row_ptr is None

    @property
    def max_members(self) -> int:
        """Assignments of the largest target (one host read, remembered): the segment readout picks its route by it."""
        if self._max_members is None:
            rp = self._row_ptr
            self._max_members = int((rp[1:] - rp[:-1]).max()) if self.num_targets > 0 else 0
        return self._max_members

    @property
    def row_ptr(self) -> Tensor:
        if self._row_ptr is None:
            self._row_ptr = torch.arange(self.num_targets + 1, dtype=torch.int32, device=self._device)
        return self._row_ptr

    def walk(self, other: Optional[Tensor], E: int):
        """The three pointers a kernel that walks the groups of an edge index is handed: the offsets, the positions
        (None: the identity) and ``other``, the edge row at the far end of every position (no pointer for an empty
        list)."""
        return N.ptr(self.row_ptr), N.ptr(self.perm), N.ptr(other) if E else None


def build_assign_index(target_index: Tensor, num_targets: int) -> AssignIndex:
    dev = N.require_device(target_index)
    target_index = N.i64c(target_index)
    nnz = target_index.numel()
    row_ptr = torch.empty(num_targets + 1, dtype=torch.int32, device=dev)
    perm = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
    L = N.lib()
    wsb = L.tgp_assign_index_workspace_bytes(nnz, num_targets)
    ws = N.workspace(wsb, dev)
    _checked(L.tgp_assign_index_build, N.ptr(target_index), nnz, num_targets, N.ptr(row_ptr), N.ptr(perm), N.ptr(ws),
             ws.numel(), N.stream_ptr(dev))
    return AssignIndex(row_ptr, perm, nnz, num_targets)


def reduce_sparse(x: Tensor, source_index: Tensor, weight: Optional[Tensor], index: AssignIndex,
                  identity_source: bool = False, unit_weight: bool = False) -> Tensor:
    """out[t,:] = sum_{i: target[i]==t} weight[i] * x[source_index[i],:]
    (reduce/base_reduce.py:146-153; lift/base_lift.py:102-111 with the roles swapped).
    ``identity_source`` / ``unit_weight``: the caller KNOWS that source_index is 0..nnz-1 / that every weight is 1.0 (a
    clustering: GraclusSelect, a cluster vector) -- the fp32 kernel then skips those two loads per assignment; same bits."""
    dev = N.require_device(x, source_index, weight)
    squeeze = x.dim() == 1
    x2 = x.view(-1, 1) if squeeze else x
    if x2.dim() != 2:
        raise ValueError(f"sparse reduce expects x of shape [N, F], got {tuple(x.shape)}")
    if x2.dtype == torch.float64 or (weight is not None and weight.dtype == torch.float64):
        # float64 features or weights: the product promotes to fp64 in the reference (base_reduce.py:146-153) -- fp64
        # kernel, same summation order
        x2 = N.f64c(x2) if x2.stride(1) == 1 and x2.dtype == torch.float64 else x2.to(torch.float64).contiguous()
        src64 = N.i64c(source_index)
        w64 = None if weight is None else N.f64c(weight.reshape(-1))
        out = torch.empty(index.num_targets, x2.size(1), dtype=torch.float64, device=dev)
        _checked(N.lib().tgp_reduce_sparse_f64, N.ptr(x2), x2.size(0), x2.size(1), x2.stride(0), N.ptr(src64),
                 N.ptr(w64), N.ptr(index._row_ptr), N.ptr(index.perm), index.nnz, index.num_targets, N.ptr(out),
                 N.stream_ptr(dev))
        return out.view(-1) if squeeze else out
    x2 = x2.to(torch.float32) if x2.dtype != torch.float32 else x2
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    source_index = N.i64c(source_index)
    w = N.opt_f32_flat(weight)
    F = x2.size(1)
    out = torch.empty(index.num_targets, F, dtype=torch.float32, device=dev)
    if (index.pack is not None and index.pack_key == (source_index.data_ptr(), 0 if w is None else w.data_ptr())
            and F % 4 == 0 and F >= 32 and x2.stride(0) % 4 == 0 and x2.data_ptr() % 16 == 0):
        # one node per target (TopK, NDP): the packed index, one streamed 8-byte load per pooled row
        _checked(N.lib().tgp_reduce_one_to_one_f32, N.ptr(x2), x2.size(0), F, x2.stride(0), N.ptr(index.pack),
                 0 if w is None else 1, index.num_targets, N.ptr(out), N.stream_ptr(dev))
        return out.view(-1) if squeeze else out
    fast = index._row_ptr is not None and index.nnz <= x2.size(0)
    _checked(N.lib().tgp_reduce_sparse_f32, N.ptr(x2), x2.size(0), F, x2.stride(0),
             None if (identity_source and fast) else N.ptr(source_index), None if unit_weight else N.ptr(w),
             N.ptr(index._row_ptr), N.ptr(index.perm), index.nnz, index.num_targets, N.ptr(out), N.stream_ptr(dev))
    return out.view(-1) if squeeze else out


def one_to_one_index(node_index: Tensor, cluster_index: Tensor, weight: Optional[Tensor]) -> AssignIndex:
    """Inverted index of an assignment whose supernodes own exactly one node each (cluster_index a permutation of
    0..k-1: TopK, NDP): perm = the inverse permutation, plus the packed {source row, weight} form the Reduce kernel
    streams -- one launch, no sort (select/base_select.py:58 keeps the assignment node-sorted)."""
    dev = N.require_device(node_index, cluster_index, weight)
    ni, ci = N.i64c(node_index), N.i64c(cluster_index)
    w = N.opt_f32_flat(weight)
    k = ci.numel()
    perm = torch.empty(max(k, 1), dtype=torch.int32, device=dev)
    pack = torch.empty(max(k, 1), dtype=torch.int64, device=dev)
    _checked(N.lib().tgp_one_to_one_index_build, N.ptr(ni), N.ptr(ci), N.ptr(w), k, N.ptr(perm), N.ptr(pack),
             N.stream_ptr(dev))
    index = AssignIndex(None, perm, k, k)
    index.pack, index.pack_key = pack, (ni.data_ptr(), 0 if w is None else w.data_ptr())
    return index


def reduce_batch_sparse(batch: Tensor, node_index: Tensor, cluster_index: Tensor, num_supernodes: int,
                        every_cluster_has_a_node: bool = False) -> Tensor:
    """reduce/base_reduce.py:37-41.  ``every_cluster_has_a_node``: the caller knows that no supernode is empty (the
    ``arange`` underneath the scatter never shows): one launch instead of two."""
    dev = N.require_device(batch, node_index, cluster_index)
    batch, node_index, cluster_index = N.i64c(batch), N.i64c(node_index), N.i64c(cluster_index)
    out = torch.empty(num_supernodes, dtype=torch.int64, device=dev)
    _checked(N.lib().tgp_reduce_batch_i64, N.ptr(batch), N.ptr(node_index), N.ptr(cluster_index), node_index.numel(),
             num_supernodes, 1 if every_cluster_has_a_node else 0, N.ptr(out), N.stream_ptr(dev))
    return out


# ------------------------------------------------------------------------- A4 / A5 / A6
def _edge_rows(edge_index: Tensor) -> Tuple[Tensor, Tensor]:
    """The two rows of a [2, E] list as contiguous int64 vectors.  The C ABI takes them as two pointers, so a list whose
    ROWS are contiguous (e.g. the narrowed capacity buffers of ``sparse_pool_small``) needs no copy."""
    ei = edge_index
    if ei.dtype != torch.int64:
        ei = ei.to(torch.int64)
    if not (ei.dim() == 2 and ei.size(0) == 2 and (ei.stride(1) == 1 or ei.size(1) <= 1)):
        ei = ei.contiguous()
    return ei[0], ei[1]


def _row_operand(x: Tensor, who: str, convert: bool = False, packed: bool = False) -> Tuple[Tensor, int]:
    """THE row operand of the wrappers: ``(x, ld)`` = ``x`` as float32 [rows, F] with unit column stride, and the row
    stride its kernel is handed.  Another dtype is converted (``convert``) or refused under the caller's name ``who``.
    A view keeps its row stride -- a column slice of a wider buffer is read where it lies -- and is copied only when its
    columns are strided or its rows overlap; ``packed`` (a kernel that takes no row stride): whenever it is not
    contiguous."""
    if x.dim() != 2 or (x.dtype != torch.float32 and not convert):
        raise ValueError(f"{who} expects {'' if convert else 'float32 '}x of shape [rows, F], got {x.dtype} "
                         f"{tuple(x.shape)}")
    if x.dtype != torch.float32:
        x = x.to(torch.float32)
    rows, F = x.shape
    if (not x.is_contiguous()) if packed else ((F > 1 and x.stride(1) != 1) or (rows > 1 and x.stride(0) < F)):
        x = x.contiguous()
    return x, (x.stride(0) if rows > 1 else max(x.stride(0), F))


# ------------------------------------------------------------------------- A1 + A2 + A4/A5 + A6, batches of small graphs
_SPS_STATE: dict = {}  # (device index, stream handle) -> _SpsState
_SPS_WORDS: dict = {}  # (graphs, mode) -> look-back words of the one-launch kernel (a native call otherwise)
_EPOCH_LIMIT = (1 << 29) - 1  # the epoch at which a state's status buffer is cleared and its epochs start over
# r6: the exact-size outputs of the one-launch sparse pooling are carved out of ONE allocation of at most this many bytes
# (what a retained x' can pin); TGP_SPS_ARENA=0: four allocations of their own, sized once the count has arrived
_SPS_ARENA = os.environ.get("TGP_SPS_ARENA", "1") != "0"
_SPS_ARENA_BYTES = 16 << 20
_SPS_ONE_ALLOC_BYTES = 32 << 20  # outputs of the one-launch sparse pooling below this size share one allocation
_SPS_GIVE_PTRS = os.environ.get("TGP_SPS_GIVE_PTRS", "1") != "0"  # A/B switch: hand the per-graph offsets to the kernel
_GRACLUS_FUSED = os.environ.get("TGP_GRACLUS_FUSED", "1") != "0"  # A/B switch: one-launch GraclusSelect of small graphs
_PUBLISH_COUNTS = os.environ.get("TGP_PUBLISH_COUNTS", "1") != "0"  # A/B switch of _read_count (read once)
SPS_COMPACT_BYTES = 1 << 30  # capacity buffers above this are replaced by exact copies when mostly empty

# Output contract of the single-call operators (r5).  The reference hands out new tensors of exactly the pooled size
# (connect/base_conn.py:103-112; SURVEY 8(b) "Ownership"); the one-launch kernels write into CAPACITY-sized buffers
# because the count is only known afterwards.  Default (False): exact-size outputs -- ``edge_index`` a contiguous [2, E']
# tensor that owns 16 E' bytes -- filled from the capacity scratch by one native launch (tgp_edges_compact).  True: the
# r4 behaviour, ``edge_index`` a [2, E'] VIEW of the capacity buffer (row stride E, E-sized storage kept alive; no copy)
# for callers that consume the pooled graph at once, e.g. straight into SparseGather or the next pooling level.
_OUTPUT_VIEWS_DEFAULT = os.environ.get("TGP_OUTPUT_VIEWS", "0") == "1"
_OUTPUT_VIEWS_LOCAL = threading.local()  # per thread: a `with output_views()` in one thread must not
#                                                        change the layout other threads (autograd workers) hand out


def _output_views() -> bool:
    return getattr(_OUTPUT_VIEWS_LOCAL, "value", _OUTPUT_VIEWS_DEFAULT)


def set_output_views(enable: bool) -> bool:
    """Choose the layout of the pooled edge lists of the single-call operators for THIS thread (default: the process-wide
    ``TGP_OUTPUT_VIEWS`` setting); returns the previous setting."""
    prev = _output_views()
    _OUTPUT_VIEWS_LOCAL.value = bool(enable)
    return prev


class output_views:
    """``with tgp.kernels.output_views():`` -- capacity views inside the block (opt-in), restored afterwards."""

    def __init__(self, enable: bool = True):
        self.enable = enable

    def __enter__(self):
        self.prev = set_output_views(self.enable)
        return self

    def __exit__(self, *exc):
        set_output_views(self.prev)
        return False


def _compact_edges(L, st, dev, row_p: int, col_p: int, w_p, w_dtype, id_p, n_out: int):
    """Exact-size (edge_index [2,n], weight [n] or None, edge_id [n] or None) from the first n entries of capacity
    arrays: two or three allocations and ONE launch."""
    out_ei = torch.empty(2, n_out, dtype=torch.int64, device=dev)
    out_w = None if w_p is None else torch.empty(n_out, dtype=w_dtype, device=dev)
    out_id = None if id_p is None else torch.empty(n_out, dtype=torch.int64, device=dev)
    if n_out:
        o = out_ei.data_ptr()
        _checked(L.tgp_edges_compact, row_p, col_p, w_p, 0 if w_p is None else out_w.element_size(), id_p, n_out, o,
                 o + 8 * n_out, N.ptr(out_w), N.ptr(out_id), st)
    return out_ei, out_w, out_id


class _SpsState:
    """Per (device, stream): the look-back words of the one-launch kernels (``tgp_sparse_pool_small_f32``, the single-pass
    subgraph Connect, the coalesce Connect's scans, the one-launch GraclusSelect; device memory, never cleared: every
    word carries the epoch of the call that wrote it), the epoch counter, and ONE pinned host word the kernel's last
    workgroup stores {epoch, refused, total} into -- the host polls it instead of paying a device-to-host copy kernel
    and a stream synchronise for eight bytes (``tgp_count_publish`` gives every count -> fill pair the same read)."""

    __slots__ = ("status", "epoch", "pinned", "host", "words", "ticket", "facts_pinned", "facts_host", "facts_tag")

    def __init__(self, dev, words):
        self.status = torch.zeros(max(int(words), 4096), dtype=torch.int64, device=dev)
        self.epoch = 0
        self.pinned = torch.zeros(8, dtype=torch.int64).pin_memory()
        self.host = self.pinned.numpy()  # the same memory
        self.words = (self.status.data_ptr(), self.status.numel(), self.pinned.data_ptr())  # what every call is handed
        # the one-launch batch facts (utils.ops._batch_facts_sorted): arrival ticket + flag word (zero between calls) and
        # the pinned words {tag, B - 1, flags, longest graph, non-empty graphs, sum of TopK keep counts}
        self.ticket = torch.zeros(8, dtype=torch.int32, device=dev)  # words 0-1 batch facts, 2-3 edge facts / symmetry,
        #                                                               4 the MinCut tail's batch means (r6)
        self.facts_pinned = torch.zeros(8 * 8, dtype=torch.int64).pin_memory()  # 8 slots of 8 words (prefetched calls)
        self.facts_host = self.facts_pinned.numpy()
        self.facts_tag = 0

    def next_facts_tag(self) -> int:
        self.facts_tag += 1
        return self.facts_tag

    def facts_slot(self, tag: int) -> int:
        """Address of the pinned result words of call ``tag`` (calls rotate through eight slots: a prefetched call's
        words are not overwritten by the calls enqueued behind it)."""
        return self.facts_pinned.data_ptr() + 64 * (tag & 7)

    def _spin(self, host, at: int, arrived, error: str) -> int:
        """The pinned word ``host[at]`` once ``arrived(word)`` holds.  Spins on it; after 4 000 000 looks the device is
        synchronised (which surfaces a device fault, if that is what happened), the word is read once more and, still not
        there, ``error`` is raised: a stuck device becomes an error instead of a hang."""
        spins = 0
        while True:
            word = int(host[at])
            if arrived(word):
                return word
            spins += 1
            if spins > 4_000_000:
                torch.cuda.synchronize(self.status.device)
                word = int(host[at])
                if arrived(word):
                    return word
                raise N.TgpNativeError(error)

    def wait_facts(self, tag: int):
        host, o = self.facts_host, 8 * (tag & 7)
        self._spin(host, o, lambda have: have == tag, "tgp_batch_facts_sorted_i64 finished without storing its result word")
        return int(host[o + 1]), int(host[o + 2]), int(host[o + 3]), int(host[o + 4]), int(host[o + 5])

    def peek_facts(self, tag: int):
        """The flag word of call ``tag``, or None when its slot has been reused by a later call (eight slots rotate)."""
        host, o = self.facts_host, 8 * (tag & 7)
        have = self._spin(host, o, lambda have: have >= tag, "a facts launch finished without storing its result word")
        return int(host[o + 2]) if have == tag else None

    def next_epoch(self) -> int:
        self.epoch += 1
        if self.epoch >= _EPOCH_LIMIT:  # epochs of a buffer never repeat: start over on a cleared buffer
            torch.cuda.synchronize(self.status.device)
            self.status.zero_()
            self.host[0] = 0
            self.epoch = 1
        return self.epoch

    def wait(self, epoch: int) -> int:
        """The result word of call ``epoch`` (spins on the pinned word; a stuck device is turned into an error)."""
        return self._spin(self.host, 0, lambda word: (word >> 34) == epoch,
                          "a kernel that hands its count over in a pinned host word finished without storing it")

    def open_call(self) -> "_PublishedCall":
        """Advance the epoch: the handle of the one call that may now store the pinned result word."""
        return _PublishedCall(self)


class _PublishedCall:
    """One call's claim on the pinned result word of an :class:`_SpsState`: what the kernel is handed -- ``lookback``
    (status words, their count, pinned word, epoch) for the look-back kernels, ``publish`` (pinned word, epoch) for
    ``tgp_count_publish`` / ``tgp_mask_index_count`` -- and the wait for, and the decoding of, the word it stores."""

    __slots__ = ("state", "epoch", "publish", "lookback")

    def __init__(self, state: _SpsState):
        self.state, self.epoch = state, state.next_epoch()
        self.lookback = state.words + (self.epoch,)
        self.publish = self.lookback[2:]

    def total(self) -> Optional[int]:
        """The one-launch kernels' word {refused: bit 31, total: bits 0..30}: the total, or None when the kernel refused
        its input."""
        word = self.state.wait(self.epoch)
        return None if word & 0x80000000 else word & 0x7FFFFFFF

    def count(self) -> int:
        """The signed 34-bit count of a count kernel's word (decline codes are negative)."""
        return _decode_count(self.state.wait(self.epoch))

    def refused_for_ids(self) -> bool:
        """After a refusal: did a chunk of this call meet an id outside its table?  It says so in word [1] of the status
        buffer, tagged with the call's epoch (one device read, on the error path only)."""
        return (int(self.state.status[1]) & 0xFFFFFFFF) == self.epoch


def _sps_state(dev: torch.device, stream: int, words: int) -> "_SpsState":
    key = (dev.index, stream)
    ent = _SPS_STATE.get(key)
    if ent is None or ent.status.numel() < words:
        ent = _SpsState(dev, words)
        _SPS_STATE[key] = ent
    return ent


_DECLINED_LISTS = TensorMemo(16)


def sparse_pool_small_declined(edge_index: Tensor) -> bool:
    """Did the one-launch kernel refuse this very edge list before (unsorted rows, an edge between two graphs, ...)?
    Remembered per tensor object, like the row order, so that a refusal costs one launch once."""
    return _DECLINED_LISTS.get(edge_index) is not None


def sparse_pool_small_max_graph_nodes() -> int:
    return int(N.lib().tgp_sparse_pool_small_max_graph_nodes())


_EDGE_RANGES = TensorMemo(16)  # (edge_index, graph_ptr) -> the per-graph edge ranges of graph_edge_ptr
_edge_ptr_memo = _EDGE_RANGES.get


def graph_edge_ptr(edge_index: Tensor, graph_ptr: Tensor) -> Tensor:
    """First edge of every graph of a sorted batch in a row-sorted list ([B+1] int64: lower bounds of ``graph_ptr`` in the
    row array), remembered per (edge list object + version, graph_ptr object + version): one tiny launch for a new pair,
    nothing for a pair that is pooled again.  ``sparse_pool_small`` and the one-launch GraclusSelect re-check what they
    read through it (a wrong table is a refusal); ``dense_pool_select_sparse`` clamps the ranges into [0, E] and
    ``dmon_edge_degrees`` reads them as they are: both trust that the table belongs to the list ("What is
    remembered between calls")."""
    hit = _edge_ptr_memo(edge_index, graph_ptr)
    if hit is not None:
        return hit
    dev = edge_index.device
    gp = N.i64c(graph_ptr)
    out = torch.empty(gp.numel(), dtype=torch.int64, device=dev)
    row = edge_index[0]
    _checked(N.lib().tgp_graph_lower_bounds_i64, N.ptr(row) if row.numel() else None, row.numel(), N.ptr(gp),
             gp.numel() - 1, N.ptr(out), N.stream_ptr(dev))
    _EDGE_RANGES.put(edge_index, out, graph_ptr)
    return out


def sparse_pool_small(x: Tensor, graph_ptr: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor],
                      assign_index: Tensor, weight: Optional[Tensor], num_supernodes: int,
                      mode: int, reduce_op: str = "sum", remove_self_loops: bool = True, want_batch: bool = True,
                      assign_ptr: Optional[Tensor] = None, views: Optional[bool] = None, checked: bool = False):
    """Sparse Reduce + Connect of a sorted batch of graphs of at most 64 nodes in ONE launch
    (reduce/base_reduce.py:14-53,141-155; connect/base_conn.py:79-89; the filters of utils/ops.py:370-380):
    ``(x_pool [K,F], batch_pool [K] or None, edge_index' [2,E'], edge_weight' [E'] or None)``, bit-identical to
    ``reduce_sparse`` + ``reduce_batch_sparse`` + ``filter_edges`` (mode 0) / ``coalesce_edges`` (mode 1).  The pooled
    edges are written once at their final offsets of capacity-E scratch and -- by default -- moved into exact-size
    outputs by one more launch once the count is known (four tensors of their own, ``edge_index'`` contiguous);
    ``views=True`` (default: ``tgp.kernels.output_views``) hands out the r4 layout instead: all four outputs carved out
    of ONE allocation, ``edge_index'`` a view of the capacity buffer whose two rows are contiguous, no copy.
    ``assign_index`` [2, nnz] = (node_index, cluster_index), the indices of the sparse S.  None: a precondition checked
    on the device does not hold (the caller takes the staged operators)."""
    if views is None:
        views = _output_views()
    # (this wrapper sits in front of a ~10 us kernel: pointers by arithmetic instead of row views; `checked`: the caller
    #  -- SRCPooling.reduce_connect -- has validated x, edge_index and the weights' dtypes: no second pass over them)
    if checked:
        dev = x.device
        if not (graph_ptr.is_cuda and assign_index.is_cuda and (weight is None or weight.is_cuda)):
            dev = N.require_device(x, graph_ptr, edge_index, edge_weight, assign_index, weight)
    else:
        dev = N.require_device(x, graph_ptr, edge_index, edge_weight, assign_index, weight)
        if x.dim() != 2 or x.dtype != torch.float32 or x.stride(1) != 1:
            raise ValueError("sparse_pool_small expects float32 x [N, F] with unit feature stride")
    ei = edge_index
    es0, es1 = ei.stride() if ei.dim() == 2 else (0, 0)
    if not (ei.dtype == torch.int64 and ei.dim() == 2 and ei.size(0) == 2 and (es1 == 1 or ei.size(1) <= 1)):
        ei = N.i64c(ei)
        es0 = ei.stride(0)
    E = ei.size(1)
    row_p = ei.data_ptr()
    col_p = row_p + 8 * es0
    w = edge_weight
    if w is not None and not (w.dim() == 1 and w.dtype == torch.float32 and (w.stride(0) == 1 or E <= 1)):
        w = N.f32c(w.reshape(-1))
    ai = assign_index
    as0, as1 = ai.stride() if ai.dim() == 2 else (0, 0)
    if not (ai.dtype == torch.int64 and ai.dim() == 2 and ai.size(0) == 2 and (as1 == 1 or ai.size(1) <= 1)):
        ai = N.i64c(ai)
        as0 = ai.stride(0)
    nnz = ai.size(1)
    ni_p = ai.data_ptr()
    ci_p = ni_p + 8 * as0
    gp = graph_ptr if (graph_ptr.dtype == torch.int64 and graph_ptr.is_contiguous()) else N.i64c(graph_ptr)
    wt = weight
    if wt is not None and not (wt.dim() == 1 and wt.dtype == torch.float32 and (wt.stride(0) == 1 or nnz <= 1)):
        wt = N.f32c(wt.reshape(-1))
    (n, F), K, B = x.shape, int(num_supernodes), gp.numel() - 1
    ecap = max(E, 1)
    # ONE allocation for all four outputs when they are small (a batch of small graphs: a few MB): only addresses are
    # needed to launch, and the typed views are made WHILE the kernel runs, behind the launch -- this wrapper sits in
    # front of a ~10 us kernel and every allocation in front of the launch is ~1.2 us the GPU idles.  (Large inputs keep
    # separate buffers: a retained x_pool must not pin tens of MB of edge capacity.)
    #   views (tgp.kernels.output_views):  x' | batch' | rows cap | cols cap | w cap        edge_index' = [2, n] of row
    #                                      stride ecap, no copy
    #   default (r6: the arena):           x' | batch' | rows cap + room for n cols | w cap | col scratch
    #                                      the kernel's rows and weights ARE the outputs; one launch moves the n columns
    #                                      behind the n rows once the count is known: edge_index' contiguous [2, n]
    ob = (K * F * 4 + 15) & ~15
    oe = (ob + (K * 8 if want_batch else 0) + 15) & ~15
    ow = (oe + 2 * ecap * 8 + 15) & ~15
    oc = (ow + (ecap * 4 if w is not None else 0) + 15) & ~15
    arena = (not views) and _SPS_ARENA and E > 0 and oc + 8 * ecap <= _SPS_ARENA_BYTES
    one = views and oc <= _SPS_ONE_ALLOC_BYTES
    if one or arena:
        buf = torch.empty((oc + (8 * ecap if arena else 0)) >> 3, dtype=torch.int64, device=dev)
        base = buf.data_ptr()
        xp_p, bp_p, cap_p, cw_p = base, (base + ob) if want_batch else None, base + oe, (base + ow) if w is not None else None
        col_out = base + oc if arena else cap_p + 8 * ecap
    elif not views:
        # exact outputs: x' and batch' are sized before the launch; the edges go through one capacity scratch buffer
        x_pool = torch.empty(K, F, dtype=torch.float32, device=dev)
        batch_pool = torch.empty(K, dtype=torch.int64, device=dev) if want_batch else None
        scratch = torch.empty(2 * ecap * 8 + (ecap * 4 if w is not None else 0), dtype=torch.uint8, device=dev)
        cap_p = scratch.data_ptr()
        cw_p = cap_p + 16 * ecap if w is not None else None
        xp_p, bp_p = x_pool.data_ptr(), N.ptr(batch_pool)
        col_out = cap_p + 8 * ecap
    else:
        x_pool = torch.empty(K, F, dtype=torch.float32, device=dev)
        batch_pool = torch.empty(K, dtype=torch.int64, device=dev) if want_batch else None
        cap = torch.empty(2, ecap, dtype=torch.int64, device=dev)
        cap_w = None if w is None else torch.empty(ecap, dtype=torch.float32, device=dev)
        xp_p, bp_p, cap_p, cw_p = x_pool.data_ptr(), N.ptr(batch_pool), cap.data_ptr(), N.ptr(cap_w)
        col_out = cap_p + 8 * ecap
    L = N.lib()
    st = N.stream_ptr(dev)
    words = _SPS_WORDS.get((B, mode))
    if words is None:
        if len(_SPS_WORDS) > 256:
            _SPS_WORDS.clear()
        words = _SPS_WORDS[(B, mode)] = int(L.tgp_sparse_pool_small_status_words(B, mode))
    # (the handshake is written out here and not taken from `open_call`: no handle object and no tuples in front of a
    #  ~10 us kernel, as long as nobody has measured that they cost nothing)
    state = _sps_state(dev, st, words)
    epoch = state.next_epoch()
    flags = (N.REMOVE_SELF_LOOPS if remove_self_loops else 0) | (N.EPS_FILTER if w is not None else 0)
    # per-graph offsets the caller side already has: the kernel skips its searches (and re-checks what it reads).  r5: an
    # edge list that is NEW to this process (every mini-batch of a training loop) no longer pays a lower-bounds launch
    # for them: the kernel searches for its ranges as it did before r4 and LEAVES them in `eptr_out`, which is remembered
    # for the next call on the same tensors
    eptr = _edge_ptr_memo(edge_index, graph_ptr) if (E and _SPS_GIVE_PTRS) else None
    eptr_out = None
    if eptr is None and E and _SPS_GIVE_PTRS:
        eptr_out = torch.empty(B + 1, dtype=torch.int64, device=dev)
    aptr = None
    if eptr is not None and mode == 0:
        if assign_ptr is not None and assign_ptr.dtype == torch.int64 and assign_ptr.numel() == B + 1 and assign_ptr.is_cuda:
            aptr = assign_ptr if assign_ptr.is_contiguous() else assign_ptr.contiguous()
        else:
            eptr = None  # (mode 0 needs both tables)
    pinned_p = state.pinned.data_ptr()
    _checked(L.tgp_sparse_pool_small_f32, x.data_ptr(), n, F, x.stride(0), gp.data_ptr(), B, N.ptr(eptr), N.ptr(aptr),
             N.ptr(eptr_out), row_p if E else None, col_p if E else None, N.ptr(w), E, ni_p, ci_p, N.ptr(wt), nnz, K,
             mode, N.REDUCE_OPS[reduce_op], flags, ops_eps(), xp_p, bp_p, cap_p, col_out, cw_p, state.status.data_ptr(),
             state.status.numel(), pinned_p, epoch, st)
    if one or arena:  # (behind the launch: the kernel is running)
        f32 = buf.view(torch.float32)
        x_pool = torch.as_strided(f32, (K, F), (F, 1), 0)
        batch_pool = torch.as_strided(buf, (K,), (1,), ob >> 3) if want_batch else None
    if eptr_out is not None:  # (forgotten again below if the kernel refuses the input)
        _EDGE_RANGES.put(edge_index, eptr_out, graph_ptr)
    if arena:
        # the call's one host wait (the reference's .item() syncs) and the column move, in one native call (r6)
        _checked(L.tgp_result_wait_pack_cols, pinned_p, epoch, col_out, cap_p, st)
        total = int(state.host[0])
        if (total >> 34) != epoch:
            raise N.TgpNativeError("tgp_result_wait_pack_cols returned before the result word of its call was stored")
    else:
        total = state.wait(epoch)
    if total & 0x80000000:
        if eptr_out is not None:
            _EDGE_RANGES.discard(edge_index)
        _DECLINED_LISTS.put(edge_index, True)
        return None
    n_out = total & 0x7FFFFFFF
    if arena:
        ei = torch.as_strided(buf, (2, n_out), (max(n_out, 1), 1), oe >> 3)
        ew = torch.as_strided(f32, (n_out,), (1,), ow >> 2) if w is not None else None
        return x_pool, batch_pool, ei, ew
    if not views:
        ei, ew, _ = _compact_edges(L, st, dev, cap_p, col_out, cw_p, torch.float32, None, n_out)
        return x_pool, batch_pool, ei, ew
    if one:
        ei = torch.as_strided(buf, (2, n_out), (ecap, 1), oe >> 3)
        ew = torch.as_strided(f32, (n_out,), (1,), ow >> 2) if w is not None else None
    else:
        ei = cap[:, :n_out]
        ew = None if cap_w is None else cap_w[:n_out]
    if E * 16 > SPS_COMPACT_BYTES and 2 * n_out < E:
        ei, ew = ei.contiguous(), None if ew is None else ew.clone()
    return x_pool, batch_pool, ei, ew


def _decode_count(word: int) -> int:
    """The count of a published result word: bits 0..33, two's complement (decline codes are negative)."""
    n = word & ((1 << 34) - 1)
    return n - (1 << 34) if n >= 1 << 33 else n


def _read_count(d_count: Tensor) -> int:
    # the single host wait of a count -> fill pair (the reference pays `.item()` syncs too).  r4: a one-thread kernel
    # stores the count into a pinned host word this thread polls -- a few microseconds instead of the copy kernel +
    # stream synchronise of `.item()`; the wait stays in the MIDDLE of the call, so the fill still overlaps whatever
    # the caller launches next.  Under stream capture neither form is legal: the count routes are not capturable.
    if _PUBLISH_COUNTS and not torch.cuda.is_current_stream_capturing():
        dev = d_count.device
        st = N.stream_ptr(dev)
        call = _sps_state(dev, st, 0).open_call()
        _checked(N.lib().tgp_count_publish, N.ptr(d_count), *call.publish, st)
        n = call.count()
    else:
        n = int(d_count.item())
    if n == -2:  # refusal code of the count kernels: an endpoint (or cluster id) outside its table
        raise IndexError("edge_index holds node ids outside [0, num_nodes) (or cluster ids outside [0, num_supernodes)): "
                         "the reference's index ops raise for these inputs too")
    return n


_checked = N.checked  # every native call goes through it: a failure is reported under the symbol that was called


def _count_fill(dev, nbytes: int, count, fill, w_dtype=None, edge_id: bool = False,
                call: Optional[_PublishedCall] = None, rows: int = 2, declines: bool = False):
    """A count -> fill pair: size the workspace, launch ``count(workspace, its bytes, count word)``, read the count on
    the host (the call's single wait: ``call``'s published word when the count kernel stores one, else `_read_count`),
    allocate the exact-size outputs -- index ``[rows, n]``, weight ``[n]`` of ``w_dtype`` or None, with ``edge_id`` an
    int64 ``[n]`` -- and launch ``fill(workspace, n, row' .. , weight', [edge_id'])`` on their pointers.
    Returns the outputs, or -- for a pair that ``declines`` -- the count itself when it is negative: what a decline code
    means is the caller's business.
    (Known difference, kept: only `_read_count` raises for the code -2; a published count hands it back like any other
    decline, and the sort-based route that then runs raises for the same input.)"""
    ws = N.workspace(nbytes, dev)
    d_count = torch.empty(1, dtype=torch.int64, device=dev)
    count(N.ptr(ws), ws.numel(), N.ptr(d_count))
    n = _read_count(d_count) if call is None else call.count()
    if n < 0 and declines:
        return n
    index = torch.empty(rows, n, dtype=torch.int64, device=dev)
    out = (index, None if w_dtype is None else torch.empty(n, dtype=w_dtype, device=dev))
    if edge_id:
        out += (torch.empty(n, dtype=torch.int64, device=dev),)
    if n:
        ptrs = [index.data_ptr() + 8 * n * r for r in range(rows)] + [N.ptr(t) for t in out[1:]]
    else:  # an empty tensor has no device pointer to hand over
        ptrs = [None] * (rows + len(out) - 1)
    fill(N.ptr(ws), n, *ptrs)
    return out


def member_directory_for(assign: Optional["AssignIndex"], node_index: Optional[Tensor]) -> Optional[Tensor]:
    """The selector's kept-node bitmap + rank directory, if it still describes ``node_index`` (the same storage and length
    as when TopkSelect wrote it: a SelectOutput whose ``s`` was replaced does not get the old selection's directory);
    None otherwise."""
    if assign is None or node_index is None:
        return None
    md, key = getattr(assign, "member_directory", None), getattr(assign, "member_directory_key", None)
    if md is None or key is None or key != (node_index.data_ptr(), node_index.numel()):
        return None
    return md


def filter_edges(edge_index: Tensor, edge_weight: Optional[Tensor], node_index: Optional[Tensor],
                 num_nodes: int, remove_self_loops: bool, want_edge_id: bool = False, views: Optional[bool] = None,
                 member_directory: Optional[Tensor] = None):
    """Induced subgraph + relabel (connect/base_conn.py:79-82) fused with remove_self_loops and the
    |w| > eps filter (utils/ops.py:370-380).  node_index=None: filters only.  Keeps input order.
    ``want_edge_id``: also return the input position of every kept edge (what the backward of the weight
    pass-through scatters by).  ``views`` (default ``tgp.kernels.output_views``, i.e. False): hand out views of the
    single-pass kernel's capacity-E buffers instead of exact-size tensors.  ``member_directory``: the selector's own
    bitmap + rank directory of ``node_index`` (``AssignIndex.member_directory``; node_index must be ascending, as a
    SelectOutput's is): the call is then ONE launch -- no memset, no scatter of the kept nodes, no directory scan."""
    if views is None:
        views = _output_views()
    dev = N.require_device(edge_index, edge_weight, node_index)
    row, col = _edge_rows(edge_index)
    E = row.numel()
    f64 = edge_weight is not None and edge_weight.dtype == torch.float64  # fp64 weights pass through as they are
    w = None if edge_weight is None else (N.f64c if f64 else N.f32c)(edge_weight.reshape(-1))
    ni = N.opt_i64(node_index)
    flags = (N.REMOVE_SELF_LOOPS if remove_self_loops else 0) | (N.EPS_FILTER if w is not None else 0)
    if want_edge_id:
        flags |= N.WANT_EDGE_ID
    if ni is not None:
        flags |= N.NODE_FILTER
        if ni.numel() == 0:  # no node kept: no edge survives (an empty tensor has no device pointer to hand over)
            out = (torch.empty(2, 0, dtype=torch.int64, device=dev),
                   None if w is None else torch.empty(0, dtype=w.dtype, device=dev))
            return out + (torch.empty(0, dtype=torch.int64, device=dev),) if want_edge_id else out
    L = N.lib()
    st = N.stream_ptr(dev)
    eps = ops_eps()
    if E > 0 and not torch.cuda.is_current_stream_capturing():
        # ONE pass (r4): survivors written once at their final offsets of capacity-E buffers, which are then narrowed
        # (edge_index' is a view whose two rows are contiguous); the count arrives in a pinned host word
        md = member_directory if (ni is not None and member_directory is not None and member_directory.is_cuda
                                  and member_directory.dtype == torch.int32
                                  and member_directory.numel() == 5 * int(L.tgp_topk_select_directory_blocks(num_nodes))
                                  ) else None
        got = _filter_edges_single(L, dev, st, row, col, w, E, ni, num_nodes, flags, eps, want_edge_id, views, md)
        if got is None and f64:  # (a look-back spin bound on a shared device: once more; fp64 has no count -> fill pair)
            got = _filter_edges_single(L, dev, st, row, col, w, E, ni, num_nodes, flags, eps, want_edge_id, views, md)
        if got is not None:
            return got
    if f64 and E == 0:
        out = (torch.empty(2, 0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.float64, device=dev))
        return out + (torch.empty(0, dtype=torch.int64, device=dev),) if want_edge_id else out
    if f64:
        # the single pass declined twice (a look-back spin bound: the device is shared) or a stream is being captured:
        # staged route for float64 weights -- the count -> fill pair on the indices alone (node filter + self loops) with
        # the kept edges' input positions, then the |w| > eps test on the gathered weights IN DOUBLE (this
        # used to raise)
        ei2, _, eid = filter_edges(edge_index, None, node_index, num_nodes, remove_self_loops, want_edge_id=True,
                                   views=views)
        w2 = w[eid]
        keep = w2.abs() > eps
        ei2, w2, eid = ei2[:, keep].contiguous(), w2[keep], eid[keep]
        return (ei2, w2, eid) if want_edge_id else (ei2, w2)
    return _count_fill(
        dev, L.tgp_connect_subgraph_workspace_bytes(E, num_nodes),
        lambda ws, ws_bytes, cnt: _checked(L.tgp_connect_subgraph_count, N.ptr(row), N.ptr(col), N.ptr(w), E, N.ptr(ni),
                                           0 if ni is None else ni.numel(), num_nodes, flags, eps, ws, ws_bytes, cnt, st),
        lambda ws, n_out, r, c, ow, oid=None: _checked(L.tgp_connect_subgraph_fill, N.ptr(row), N.ptr(col), N.ptr(w), E,
                                                       num_nodes, flags, eps, ws, n_out, r, c, ow, oid, st),
        None if w is None else torch.float32, edge_id=want_edge_id)


def _filter_edges_single(L, dev, st, row, col, w, E, ni, num_nodes, flags, eps, want_edge_id, views=False, md=None):
    """``tgp_connect_subgraph_single``; None when the kernel refused for a reason other than bad node ids (a look-back
    spin bound on a shared device): the caller takes the count -> fill pair."""
    ws = N.workspace(L.tgp_connect_subgraph_single_workspace_bytes(num_nodes), dev)
    cap = torch.empty(2, E, dtype=torch.int64, device=dev)
    cap_w = None if w is None else torch.empty(E, dtype=w.dtype, device=dev)
    cap_id = torch.empty(E, dtype=torch.int64, device=dev) if want_edge_id else None
    call = _sps_state(dev, st, L.tgp_connect_subgraph_single_status_words(E)).open_call()
    cap_p = cap.data_ptr()
    entry = (L.tgp_connect_subgraph_single_f64 if (w is not None and w.dtype == torch.float64)
             else L.tgp_connect_subgraph_single)
    nblk = 0 if md is None else md.numel() // 5
    _checked(entry, row.data_ptr(), col.data_ptr(), N.ptr(w), E, N.ptr(ni), 0 if ni is None else ni.numel(), num_nodes,
             flags, eps, ws.data_ptr(), ws.numel(), cap_p, cap_p + 8 * E, N.ptr(cap_w), N.ptr(cap_id),
             None if md is None else md.data_ptr(), None if md is None else md.data_ptr() + 16 * nblk, *call.lookback,
             st)
    n_out = call.total()
    if n_out is None:
        # refused: node ids outside [0, num_nodes) -- the reference's index ops raise for these inputs too -- or a
        # look-back spin bound
        if call.refused_for_ids():
            raise IndexError("edge_index holds node ids outside [0, num_nodes) (or cluster ids outside "
                             "[0, num_supernodes)): the reference's index ops raise for these inputs too")
        return None
    if not views:  # exact-size outputs (the default): one launch moves the survivors out of the capacity buffers
        out_ei, out_w, out_id = _compact_edges(L, st, dev, cap_p, cap_p + 8 * E, N.ptr(cap_w),
                                               None if cap_w is None else cap_w.dtype, N.ptr(cap_id), n_out)
        return (out_ei, out_w, out_id) if want_edge_id else (out_ei, out_w)
    out_ei, out_w = cap[:, :n_out], None if cap_w is None else cap_w[:n_out]
    out_id = None if cap_id is None else cap_id[:n_out]
    if E * 16 > SPS_COMPACT_BYTES and 4 * n_out < E:  # mostly empty capacity buffers of a large list: exact copies
        out_ei = out_ei.contiguous()
        out_w = None if out_w is None else out_w.clone()
        out_id = None if out_id is None else out_id.clone()
    return (out_ei, out_w, out_id) if want_edge_id else (out_ei, out_w)


FUSED_MAX_SUPERNODES = 32 * 1024  # 1024 tiles of 32 supernode rows
# ... and while supernode rows are short on average: a row of more than 64 raw entries is sorted by the whole workgroup,
# one such row at a time, with its successors waiting in their look-back (a batch of denser mid-size graphs -- the
# reference's own timing harness, 27 entries per row on average -- took 1.45 ms in the fused kernel, 0.1 ms staged)
FUSED_MAX_AVG_ROW = 16


def _coalesce_fused(q):
    """Row-local route as ONE kernel (``tgp_connect_coalesce_fused_*``; float32 only): survivors written at their final
    offsets through a decoupled look-back, the weights into a capacity-E buffer.  Declines with -3 (more tiles than one
    launch wave holds) or -1 (unsorted rows, or a supernode row too long for it)."""
    L, (E, _, _) = q.L, q.sizes
    cap_w = None if q.w is None else torch.empty(max(E, 1), dtype=torch.float32, device=q.dev)
    got = _count_fill(
        q.dev, L.tgp_connect_coalesce_fused_workspace_bytes(*q.sizes),
        lambda ws, ws_bytes, cnt: _checked(L.tgp_connect_coalesce_fused_count, *q.rc, q.cptr, q.ccol, *q.rest,
                                           N.ptr(q.index.row_ptr), N.ptr(q.index.perm), q.op, q.flags, q.eps,
                                           N.ptr(cap_w), ws, ws_bytes, cnt, q.st),
        lambda ws, n, r, c, _: _checked(L.tgp_connect_coalesce_fused_fill, ws, *q.sizes, n, r, c, q.st),
        declines=True)
    if q.w is None or isinstance(got, int):
        return got
    n_out = got[0].size(1)  # the kernel wrote the weights at their final offsets of the capacity-E buffer
    return got[0], cap_w[:n_out] if 2 * n_out >= E else cap_w[:n_out].clone()


def _coalesce_rows(q):
    """Row-local route as the staged pipeline (``tgp_connect_coalesce_rows_*``: any member count per supernode).
    Declines with -1 (unsorted rows) or -5 (a hub row: a supernode row beyond 1024 raw entries).  float32 answers -5 by
    one more attempt with the huge-row kernels and remembers the list in ``_HUB_LISTS``, so that later calls ask for them
    at once; the float64 library has no huge-row form and reads no such memo."""
    L, f64 = q.L, q.f64
    hub = not f64 and _HUB_LISTS.get(q.edge_index) is not None
    # float32: the published count is an A/B switch and is not capturable; float64 has the published entry only (its
    # preconditions exclude capture)
    published = f64 or (_PUBLISH_COUNTS and not torch.cuda.is_current_stream_capturing())
    while True:
        fl = q.flags | (N.HUGE_ROWS if hub else 0)
        nbytes = (L.tgp_connect_coalesce_rows_huge_workspace_bytes if hub else
                  q.entry("tgp_connect_coalesce_rows_workspace_bytes"))(*q.sizes)
        members = (N.ptr(q.index.row_ptr), N.ptr(q.index.perm), q.cptr, q.op, fl, q.eps)
        call = None
        if published:
            # the survivor scan is one look-back launch whose last workgroup stores the count into a pinned host word: no
            # scan pair, no copy kernel, no stream synchronise; int32 columns when Select's CSR holds them (float32)
            call = _sps_state(q.dev, q.st, L.tgp_connect_coalesce_rows_count_status_words(q.sizes[2], q.sizes[1])).open_call()
            count = lambda ws, ws_bytes, cnt: _checked(  # noqa: E731
                q.entry("tgp_connect_coalesce_rows_count_published"), *q.rc, q.ccol, *q.rest, *members, ws, ws_bytes,
                cnt, *call.lookback, q.st)
        else:
            count = lambda ws, ws_bytes, cnt: _checked(  # noqa: E731
                L.tgp_connect_coalesce_rows_count, *q.rc, *q.rest, *members, ws, ws_bytes, cnt, q.st)
        # fill mode (float32 only): bit 0 = weights, bit 1 = huge rows
        mode = () if f64 else ((0 if q.w is None else 1) | (2 if hub else 0),)
        got = _count_fill(q.dev, nbytes, count,
                          lambda ws, n, r, c, w: _checked(q.entry("tgp_connect_coalesce_rows_fill"), ws, *q.sizes, *mode,
                                                          n, r, c, w, q.st),
                          q.w_dtype, call=call, declines=True)
        if got != -5 or hub or f64:  # (outputs, another decline, or no huge-row form to try)
            return got
        hub = True
        _HUB_LISTS.put(q.edge_index, True)


def _coalesce_grouped(q):
    """Sort by supernode row only (half the radix passes of the general route: for more than 32 bits of (row, col) key)
    and order the short rows in LDS; float32 only.  Declines (-1) when a supernode row is too long for that."""
    L = q.L
    return _count_fill(
        q.dev, L.tgp_connect_coalesce_grouped_workspace_bytes(*q.sizes),
        lambda ws, ws_bytes, cnt: _checked(L.tgp_connect_coalesce_grouped_count, *q.rc, *q.rest, q.op, q.flags, q.eps, ws,
                                           ws_bytes, cnt, q.st),
        lambda ws, n, r, c, w: _checked(L.tgp_connect_coalesce_rows_fill, ws, *q.sizes, 0 if q.w is None else 1, n, r, c,
                                        w, q.st),
        q.w_dtype, declines=True)


def _coalesce_general(q):
    """Device-wide sort by the whole (row, col) key: takes every list and never declines."""
    return _count_fill(
        q.dev, q.entry("tgp_connect_coalesce_workspace_bytes")(*q.sizes),
        lambda ws, ws_bytes, cnt: _checked(q.entry("tgp_connect_coalesce_count"), *q.rc, *q.rest, q.op, q.flags, q.eps,
                                           ws, ws_bytes, cnt, q.st),
        lambda ws, n, r, c, w: _checked(q.entry("tgp_connect_coalesce_fill"), ws, *q.sizes, 0 if q.w is None else 1,
                                        q.flags, n, r, c, w, q.st),
        q.w_dtype)


def coalesce_edges(edge_index: Tensor, edge_weight: Optional[Tensor], cluster_index: Tensor,
                   num_supernodes: int, reduce_op: str, remove_self_loops: bool,
                   eps_filter: bool = True, assign_index: Optional[AssignIndex] = None,
                   route: Optional[str] = None, csr: Optional[Tuple[Tensor, Tensor]] = None
                   ) -> Tuple[Tensor, Optional[Tensor]]:
    """cluster_index[edge_index] + PyG coalesce (connect/base_conn.py:86-89) fused with
    remove_self_loops and the |w| > eps filter (utils/ops.py:370-380).

    With the supernode->member index of the assignment at hand (``assign_index``) the sort-free row-local
    path is tried first; it declines (count = -1) for unsorted rows or very long supernode rows.
    The row-local path is first tried as ONE fused kernel (``tgp_connect_coalesce_fused_*``: survivors written at
    their final offsets through a decoupled look-back), then as the staged pipeline (any member count per supernode).
    float64 weights are merged in float64 (the reference's coalesce / scatter do), by the staged row-local pipeline or
    the general route.
    ``csr`` = (row_ptr int32 [N+1], col int32 [E] or None) of exactly this row-sorted edge list (GraclusSelect builds
    the offsets): the pass over the row array is skipped; the fused kernel can also stream the 4-byte columns.
    ``route`` ("fused" / "staged" / "rows" / "grouped" / "general"; tests): take exactly that route, raise if it
    declines ("rows" = fused, then staged)."""
    if route not in (None, "fused", "staged", "rows", "grouped", "general"):
        raise ValueError(f"unknown route {route!r}")
    if reduce_op not in N.REDUCE_OPS:
        raise ValueError(f"unknown reduce_op '{reduce_op}', expected one of {sorted(N.REDUCE_OPS)}")
    dev = N.require_device(edge_index, edge_weight, cluster_index)
    f64 = edge_weight is not None and edge_weight.dtype == torch.float64
    if f64 and route not in (None, "general", "staged", "rows"):
        raise RuntimeError("float64 edge weights take the staged row-local or the general coalesce route")
    row, col = _edge_rows(edge_index)
    E = row.numel()
    w = None if edge_weight is None else (N.f64c if f64 else N.f32c)(edge_weight.reshape(-1))
    cl = N.i64c(cluster_index)
    if csr is not None:
        cptr, ccol = csr
        if (cptr.dtype != torch.int32 or cptr.numel() != cl.numel() + 1 or not cptr.is_contiguous()
                or (ccol is not None and not f64 and (ccol.dtype != torch.int32 or ccol.numel() != E
                                                      or not ccol.is_contiguous()))):  # (float64 reads no columns of it)
            raise ValueError("csr must be (int32 [N+1], int32 [E] or None) contiguous tensors of this edge list")
    # (float64 used to build the index of a forced row-local route before it looked at `csr`; a malformed `csr` now
    #  raises the same ValueError without that launch, as float32 always did)
    rowish = route in ("fused", "staged", "rows")
    if rowish and assign_index is None:
        assign_index = build_assign_index(cl, num_supernodes)
    L = N.lib()
    # what every route function is handed.  The tuples are the runs of positional arguments the native entry points share:
    #   rc    = (row, col)                            the edge list's two rows
    #   rest  = (w, E, cluster, N, num_supernodes)    what follows them in every count entry (w: None without weights)
    #   sizes = (E, N, num_supernodes)                what every *_workspace_bytes and every fill entry takes
    #   cptr, ccol = the caller's CSR offsets / int32 columns (None: not given; float64 reads no columns)
    #   entry(name) = the symbol of this value type (`name` or `name_f64`); index = the supernode -> member AssignIndex
    q = SimpleNamespace(
        L=L, dev=dev, st=N.stream_ptr(dev), f64=f64, edge_index=edge_index, w=w, w_dtype=None if w is None else w.dtype,
        entry=lambda name: getattr(L, name + "_f64" if f64 else name), index=assign_index,
        sizes=(E, cl.numel(), num_supernodes), rc=(N.ptr(row), N.ptr(col)),
        rest=(N.ptr(w), E, N.ptr(cl), cl.numel(), num_supernodes), op=N.REDUCE_OPS[reduce_op], eps=ops_eps(),
        flags=(N.REMOVE_SELF_LOOPS if remove_self_loops else 0) | (N.EPS_FILTER if (w is not None and eps_filter) else 0),
        cptr=None if csr is None else N.ptr(csr[0]), ccol=None if (csr is None or f64) else N.ptr(csr[1]))

    # ---- the ladder: fused -> rows (staged) -> grouped -> general; float64 has the rows and the general route only.
    # A route hands back its outputs or its negative decline code; a forced route that declines raises.
    rows_ok = ((route is None or rowish) and assign_index is not None and assign_index.nnz == cl.numel()
               and assign_index.num_targets == num_supernodes and num_supernodes < (1 << 26)
               and (rowish or csr is not None or _rows_sorted_memo(edge_index) is not False)
               and not (f64 and (E == 0 or torch.cuda.is_current_stream_capturing())))
    # the fused kernel's workgroups wait for their predecessors: it is used while all tiles are resident at once
    # (<= 1024 of them: one launch wave), i.e. for batches of small graphs, where the staged pipeline's ten launches
    # dominate; large lists take the staged pipeline, whose kernels never wait for each other
    if rows_ok and not f64 and route != "staged" and (route == "fused" or (
            num_supernodes <= FUSED_MAX_SUPERNODES and E <= FUSED_MAX_AVG_ROW * num_supernodes)):
        got = _coalesce_fused(q)
        if not isinstance(got, int):
            return got
        if route == "fused":
            raise RuntimeError(f"fused coalesce route declined (code {got})")
        # -3: only the fused kernel's tile limit; -1 on a list whose rows ARE sorted: a supernode row too long for the
        # fused kernel -- the staged pipeline takes both (it sorts hub rows device-wide)
        if got != -3 and E > 1 and csr is None and _rows_sorted_memo(edge_index) is None:
            _rows_sorted(edge_index, row)
        rows_ok = got == -3 or (got == -1 and (csr is not None or _rows_sorted_memo(edge_index) is True))
    if rows_ok:
        got = _coalesce_rows(q)
        if not isinstance(got, int):
            return got
        if rowish:
            raise RuntimeError("row-local coalesce route declined (unsorted rows or a supernode row too long)")
        # remember WHY for this tensor object (one comparison pass, once): an unsorted list skips the row-local attempt
        # (~50 us + a host round trip) on every later call
        if (got == -1 and csr is None if f64 else E > 1) and _rows_sorted_memo(edge_index) is None:
            _rows_sorted(edge_index, row)
    if rowish:
        raise RuntimeError("row-local coalesce route not applicable" if f64 else
                           "row-local coalesce route declined or not applicable")
    if not f64 and (route == "grouped" or (route is None and 65536 < num_supernodes < (1 << 26))):
        got = _coalesce_grouped(q)
        if not isinstance(got, int):
            return got
        if route == "grouped":
            raise RuntimeError("grouped coalesce route declined (a supernode row too long for the in-LDS sort)")
    return _coalesce_general(q)


def normalize_edges_(edge_index: Tensor, edge_weight: Tensor, num_nodes: int, degree_norm: bool,
                     edge_weight_norm: bool, batch_pooled: Optional[Tensor], num_graphs: int) -> Tensor:
    """In-place D^-1/2 A D^-1/2 and per-graph max-abs normalisation (utils/ops.py:383-417)."""
    dev = N.require_device(edge_index, edge_weight, batch_pooled)
    row, col = _edge_rows(edge_index)
    flags = (N.DEGREE_NORM if degree_norm else 0) | (N.EDGE_WEIGHT_NORM if edge_weight_norm else 0)
    if flags == 0 or row.numel() == 0:
        return edge_weight
    bp = N.opt_i64(batch_pooled)
    L, f64 = N.lib(), edge_weight.dtype == torch.float64
    ws = N.workspace((L.tgp_postprocess_sparse_workspace_bytes_f64 if f64 else L.tgp_postprocess_sparse_workspace_bytes)(
        row.numel(), num_nodes, num_graphs), dev)
    _checked(L.tgp_postprocess_sparse_norm_f64 if f64 else L.tgp_postprocess_sparse_norm_f32, N.ptr(row), N.ptr(col),
             N.ptr(edge_weight), row.numel(), num_nodes, flags, ops_eps(), N.ptr(bp), num_graphs, N.ptr(ws), ws.numel(),
             N.stream_ptr(dev))
    return edge_weight


# ------------------------------------------------------------------------- A3 / A7 / A8
def _any_f64(*ts) -> bool:
    """Does any operand carry float64?  Then the product runs on the fp64 matrix path (r5: the reference's
    torch.matmul computes model.double() inputs in fp64, base_reduce.py:158-161, dense_conn.py:111-122)."""
    return any(isinstance(t, Tensor) and t.dtype == torch.float64 for t in ts)


def dense_flags(remove_self_loops: bool, degree_norm: bool, adj_transpose: bool, edge_weight_norm: bool) -> int:
    return ((N.REMOVE_SELF_LOOPS if remove_self_loops else 0) | (N.DEGREE_NORM if degree_norm else 0)
            | (N.SUM_AXIS_ROWS if adj_transpose else 0) | (N.EDGE_WEIGHT_NORM if edge_weight_norm else 0))


def _dense_adj_layout(adj: Tensor, dtype: torch.dtype = torch.float32) -> Tuple[Tensor, int]:
    """Accept A [B,N,N] as contiguous or as the transposed view produced by
    DenseSRCPooling.preprocessing (src.py:442-443) without materialising the transpose."""
    if adj.dtype != dtype:
        adj = adj.to(dtype)
    if adj.is_contiguous():
        return adj, 0
    t = adj.transpose(-1, -2)
    if t.is_contiguous():
        return t, N.ADJ_TRANSPOSED
    return adj.contiguous(), 0


def _out_buffer(out: Optional[Tensor], shape, dev, dtype: torch.dtype = torch.float32) -> Tensor:
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != dev or not out.is_contiguous():
        raise ValueError(f"output buffer must be a contiguous {dtype} {tuple(shape)} tensor on {dev}, got "
                         f"{tuple(out.shape)} {out.dtype} on {out.device}")
    return out


def dense_pool(s: Tensor, adj: Optional[Tensor], x: Optional[Tensor], flags: int = 0, want_raw: bool = False,
               want_post: bool = True, graph_sizes: Optional[Tensor] = None, out_x: Optional[Tensor] = None,
               out_adj: Optional[Tensor] = None, mincut_terms: bool = False, diff_stats: bool = False):
    """(x_pool, adj_raw, adj_pool) = (S^T X, S^T A S, postprocess(S^T A S)) for a padded batch
    (reduce/base_reduce.py:158-161, connect/dense_conn.py:111-122, utils/ops.py:282-335).  ``graph_sizes`` [B]
    (optional): real nodes per graph when they are the leading rows and the padding is zero (to_dense_batch layout).
    ``mincut_terms``: return a fourth value, the [2,B] per-graph tails of MinCut's losses taken inside the pooling
    kernel (batches of small graphs only; None when the batch takes another kernel).  float64 operands (any of the
    three) run the fp64 form of the same call (tgp_dense_pool_f64, on v_mfma_f64_16x16x4_f64): it has neither the loss
    terms nor the records, and ``graph_sizes`` is a speed hint it does not use."""
    f64 = _any_f64(s, adj, x)
    conv, dt = (N.f64c, torch.float64) if f64 else (N.f32c, torch.float32)
    dev = N.require_device(s, adj, x)
    s = conv(s)
    B, Nn, K = s.shape
    F = 0
    x_pool = adj_raw = adj_pool = None
    if x is not None:
        x = conv(x)
        if x.shape[:2] != (B, Nn):
            raise ValueError(f"x {tuple(x.shape)} does not match s {tuple(s.shape)}")
        F = x.size(2)
        x_pool = _out_buffer(out_x, (B, K, F), dev, dt)  # caller-provided: e.g. a slot of an all-gather send buffer
    a = None
    if adj is not None:
        if adj.shape != (B, Nn, Nn):
            raise ValueError(f"adj {tuple(adj.shape)} does not match s {tuple(s.shape)}")
        a, tflag = _dense_adj_layout(adj, dt)
        flags |= tflag
        if want_raw:
            adj_raw = torch.empty(B, K, K, dtype=dt, device=dev)
        if want_post:
            adj_pool = _out_buffer(out_adj, (B, K, K), dev, dt)
    L = N.lib()
    if f64:
        ws = N.workspace(L.tgp_dense_pool_workspace_bytes_f64(B, Nn, K, F), dev)
        _checked(L.tgp_dense_pool_f64, N.ptr(s), N.ptr(a), N.ptr(x), B, Nn, K, F, flags, ops_eps(), N.ptr(x_pool),
                 N.ptr(adj_raw), N.ptr(adj_pool), N.ptr(ws), ws.numel(), N.stream_ptr(dev))
        return (x_pool, adj_raw, adj_pool, None) if mincut_terms else (x_pool, adj_raw, adj_pool)
    if diff_stats:
        # (r6) a fourth value: DiffPool's per-graph records [B,4] from the one-wave-per-graph kernel (:func:`diffpool_stats_tail`),
        # or None when the batch does not take that kernel (the caller computes the losses from the adjacency)
        if (a is None or x is None or out_x is not None or out_adj is not None or not (want_raw or want_post)
                or not L.tgp_dense_pool_is_small(B, Nn, K, F)):
            return dense_pool(s, adj, x, flags & ~N.ADJ_TRANSPOSED, want_raw, want_post, graph_sizes, out_x, out_adj) + (None,)
        stats = torch.empty(B, 4, dtype=torch.float32, device=dev)
        _checked(L.tgp_dense_pool_small_diff_f32, N.ptr(s), N.ptr(a), N.ptr(x), None, None, None, B, Nn, K, F, flags,
                 ops_eps(), losses_eps(), None, N.ptr(x_pool), N.ptr(adj_raw), N.ptr(adj_pool), N.ptr(stats), None,
                 N.stream_ptr(dev))
        return x_pool, adj_raw, adj_pool, stats
    ws = N.workspace(L.tgp_dense_pool_workspace_bytes(B, Nn, K, F), dev)
    if mincut_terms:
        terms = None
        if a is not None and L.tgp_dense_pool_is_small(B, Nn, K, F):
            terms = torch.empty(2, B, dtype=torch.float32, device=dev)
            _checked(L.tgp_dense_pool_mincut_f32, N.ptr(s), N.ptr(a), N.ptr(x), B, Nn, K, F, flags, ops_eps(),
                     losses_eps(), N.ptr(x_pool), N.ptr(adj_raw), N.ptr(adj_pool), N.ptr(terms), N.ptr(ws), ws.numel(),
                     N.stream_ptr(dev))
            return x_pool, adj_raw, adj_pool, terms
    gs = _sizes_arg(graph_sizes, B, dev)
    _checked(L.tgp_dense_pool_f32, N.ptr(s), N.ptr(a), N.ptr(x), B, Nn, K, F, flags, ops_eps(), N.ptr(gs),
             N.ptr(x_pool), N.ptr(adj_raw), N.ptr(adj_pool), N.ptr(ws), ws.numel(), N.stream_ptr(dev))
    return (x_pool, adj_raw, adj_pool, None) if mincut_terms else (x_pool, adj_raw, adj_pool)


def dense_pool_select(x: Tensor, adj: Tensor, weight: Tensor, bias: Optional[Tensor], mask: Optional[Tensor], flags: int,
                      want_raw: bool = False, mincut_terms: bool = False, want_batch: bool = False,
                      diff_stats: bool = False):
    """(s, x_pool, adj_raw, adj_pool, terms): MLPSelect's last Linear + softmax + mask, Reduce, Connect and the
    post-processing of a batch of small graphs in ONE launch (select/mlp_select.py:105-147, base_reduce.py:158-161,
    dense_conn.py:111-122, utils/ops.py:282-335); callers check :func:`dense_pool_is_small` first.  ``want_batch``: a
    sixth value, the pooled batch vector ``arange(B).repeat_interleave(K)`` (utils/ops.py:152-169) written by the same
    launch."""
    dev = N.require_device(x, adj, weight, bias, mask)
    x, weight = N.f32c(x), N.f32c(weight)
    B, Nn, F = x.shape
    K = weight.size(0)
    if weight.shape != (K, F) or adj.shape != (B, Nn, Nn):
        raise ValueError(f"dense_pool_select: shapes x {tuple(x.shape)}, adj {tuple(adj.shape)}, weight {tuple(weight.shape)}")
    a, tflag = _dense_adj_layout(adj)
    b = N.opt_f32(bias)
    m = None
    if mask is not None:
        m = mask.to(torch.uint8) if mask.dtype != torch.uint8 and mask.dtype != torch.bool else mask
        m = m.contiguous().view(torch.uint8) if m.dtype == torch.bool else m.contiguous()
        if tuple(m.shape) != (B, Nn):
            raise ValueError(f"dense_pool_select: mask {tuple(mask.shape)} does not match x {tuple(x.shape)}")
    s = torch.empty(B, Nn, K, dtype=torch.float32, device=dev)
    x_pool = torch.empty(B, K, F, dtype=torch.float32, device=dev)
    adj_pool = torch.empty(B, K, K, dtype=torch.float32, device=dev)
    adj_raw = torch.empty(B, K, K, dtype=torch.float32, device=dev) if want_raw else None
    terms = torch.empty(2, B, dtype=torch.float32, device=dev) if mincut_terms else None
    bp = torch.empty(B * K, dtype=torch.int64, device=dev) if want_batch else None
    if diff_stats:  # (r6) DiffPool: `terms` holds the per-graph records [B,4] of :func:`diffpool_stats_tail` instead
        terms = torch.empty(B, 4, dtype=torch.float32, device=dev)
        _checked(N.lib().tgp_dense_pool_small_diff_f32, None, N.ptr(a), N.ptr(x), N.ptr(weight), N.ptr(b), N.ptr(m), B,
                 Nn, K, F, flags | tflag, ops_eps(), losses_eps(), N.ptr(s), N.ptr(x_pool), N.ptr(adj_raw),
                 N.ptr(adj_pool), N.ptr(terms), N.ptr(bp), N.stream_ptr(dev))
        return (s, x_pool, adj_raw, adj_pool, terms, bp) if want_batch else (s, x_pool, adj_raw, adj_pool, terms)
    _checked(N.lib().tgp_dense_pool_select_f32, N.ptr(x), N.ptr(a), N.ptr(weight), N.ptr(b), N.ptr(m), B, Nn, K, F,
             flags | tflag, ops_eps(), losses_eps(), N.ptr(s), N.ptr(x_pool), N.ptr(adj_raw), N.ptr(adj_pool),
             N.ptr(terms), N.ptr(bp), N.stream_ptr(dev))
    if want_batch:
        return s, x_pool, adj_raw, adj_pool, terms, bp
    return s, x_pool, adj_raw, adj_pool, terms


def edge_facts_launch(edge_index: Tensor, batch: Tensor):
    """Enqueue ``tgp_edge_facts_sorted_i64`` for a NEW row-sorted edge list: the per-graph edge ranges land in a device
    buffer the consumer can be launched on at once, the verdict (rows sorted?) in a pinned host word that
    :func:`edge_facts_finish` reads afterwards.  None when there is nothing to look at (no entries) or a stream is being
    captured."""
    row, _ = _edge_rows(edge_index)
    E, n = row.numel(), batch.numel()
    if E == 0 or n == 0 or torch.cuda.is_current_stream_capturing():
        return None
    dev = edge_index.device
    st = N.stream_ptr(dev)
    state = _sps_state(dev, st, 0)
    buf = torch.empty(n + 2, dtype=torch.long, device=dev)
    tag = state.next_facts_tag()
    _checked(N.lib().tgp_edge_facts_sorted_i64, N.ptr(row), E, N.ptr(N.i64c(batch)), n, N.ptr(buf),
             state.ticket.data_ptr() + 8, state.facts_slot(tag), tag, st)
    return state, tag, buf


def edge_facts_finish(handle, edge_index: Tensor, graph_ptr: Tensor) -> bool:
    """The verdict of :func:`edge_facts_launch`: True = the rows are grouped by ascending source node and the ranges in the
    buffer are exact (both are remembered for this tensor object: later calls need no launch), False = not (remembered
    as well: later calls skip the attempt)."""
    state, tag, buf = handle
    _, flags, _, _, _ = state.wait_facts(tag)
    if flags:
        _remember_rows_sorted(edge_index, False)
        return False
    _remember_rows_sorted(edge_index, True)
    _EDGE_RANGES.put(edge_index, buf[: graph_ptr.numel()], graph_ptr)
    return True


_STRICTLY_SORTED = TensorMemo(16)  # edge lists known to be strictly row-major sorted (no duplicates) for a node count


def coalesced_memo(edge_index: Tensor, num_nodes: int) -> bool:
    return _STRICTLY_SORTED.get(edge_index, extra=num_nodes) is not None


def remember_coalesced(edge_index: Tensor, num_nodes: int) -> None:
    _STRICTLY_SORTED.put(edge_index, True, extra=num_nodes)


_SYMMETRIC_ADJ = TensorMemo(16)  # (edge_index, edge_weight or None) -> is the adjacency symmetric?
_adj_symmetric_memo = _SYMMETRIC_ADJ.get


class AdjSymmetry:
    """Is the dense adjacency ``to_dense_adj`` built from this edge list symmetric?  Asked in the forward of the dense
    poolers' training step (one launch over the entries, tgp_adj_symmetry_f32, verdict into a pinned host word),
    answered in its backward -- hundreds of microseconds later, so the answer is simply there.  A symmetric A makes
    V = A^T S equal to U = A S: the backward then runs ONE N^2 K product less.  Remembered per (edge_index, edge_weight)
    tensor objects.  ``get()`` = True only when the answer is known to be yes."""

    __slots__ = ("state", "tag", "answer", "ei", "ew")

    def __init__(self, edge_index: Tensor, edge_weight: Optional[Tensor], adj: Tensor, batch: Tensor, ptr: Tensor):
        self.state = self.tag = None
        self.ei, self.ew = _weakref(edge_index), (None if edge_weight is None else _weakref(edge_weight))
        self.answer = _adj_symmetric_memo(edge_index, edge_weight)
        if self.answer is not None:
            return
        row, col = _edge_rows(edge_index)
        E = row.numel()
        if (E == 0 or adj.dim() != 3 or adj.size(1) != adj.size(2) or not adj.is_contiguous() or adj.dtype != torch.float32
                or torch.cuda.is_current_stream_capturing()):
            self.answer = E == 0 and not torch.cuda.is_current_stream_capturing()
            return
        dev = adj.device
        st = N.stream_ptr(dev)
        self.state = _sps_state(dev, st, 0)
        self.tag = self.state.next_facts_tag()
        _checked(N.lib().tgp_adj_symmetry_f32, N.ptr(row), N.ptr(col), E, N.ptr(N.i64c(batch)), N.ptr(N.i64c(ptr)),
                 adj.size(1), N.ptr(adj), self.state.ticket.data_ptr() + 8, self.state.facts_slot(self.tag), self.tag,
                 st)

    @classmethod
    def of_dense(cls, adj: Tensor) -> "AdjSymmetry":
        """The same question for a dense [B,N,N] float32 adjacency the caller holds (tgp_dense_symmetry_f32: one pass over
        the matrix); remembered for this tensor object + version, so a fixed dense graph pooled every epoch pays it once."""
        self = cls.__new__(cls)
        self.state = self.tag = None
        self.ei, self.ew = _weakref(adj), None
        self.answer = _adj_symmetric_memo(adj, None)
        if self.answer is not None:
            return self
        if (adj.dim() != 3 or adj.size(1) != adj.size(2) or adj.dtype != torch.float32 or not adj.is_cuda
                or not adj.is_contiguous() or adj.numel() == 0 or torch.cuda.is_current_stream_capturing()):
            self.answer = False
            return self
        dev = adj.device
        st = N.stream_ptr(dev)
        self.state = _sps_state(dev, st, 0)
        self.tag = self.state.next_facts_tag()
        _checked(N.lib().tgp_dense_symmetry_f32, N.ptr(adj), adj.size(0), adj.size(1), self.state.ticket.data_ptr() + 8,
                 self.state.facts_slot(self.tag), self.tag, st)
        return self

    @classmethod
    def of_edge_list(cls, key_index: Tensor, key_weight: Optional[Tensor], edge_index: Tensor,
                     edge_weight: Optional[Tensor], row_ptr: Tensor, num_nodes: int) -> "AdjSymmetry":
        """The same question for a COALESCED row-sorted list with its CSR offsets (tgp_edge_symmetry_f32: every entry must
        have a mirror entry of equal weight); remembered for the (key_index, key_weight) objects the caller holds."""
        self = cls.__new__(cls)
        self.state = self.tag = None
        self.ei, self.ew = _weakref(key_index), (None if key_weight is None else _weakref(key_weight))
        self.answer = _adj_symmetric_memo(key_index, key_weight)
        if self.answer is not None:
            return self
        row, col = _edge_rows(edge_index)
        E = row.numel()
        if E == 0 or torch.cuda.is_current_stream_capturing():
            self.answer = E == 0 and not torch.cuda.is_current_stream_capturing()
            return self
        dev = edge_index.device
        st = N.stream_ptr(dev)
        self.state = _sps_state(dev, st, 0)
        self.tag = self.state.next_facts_tag()
        w = N.opt_f32_flat(edge_weight)
        _checked(N.lib().tgp_edge_symmetry_f32, N.ptr(row), N.ptr(col), N.ptr(w), E, N.ptr(row_ptr), num_nodes,
                 self.state.ticket.data_ptr() + 8, self.state.facts_slot(self.tag), self.tag, st)
        return self

    def get(self) -> bool:
        if self.answer is None:
            flags = self.state.peek_facts(self.tag)
            self.answer = flags == 0 if flags is not None else False  # (slot reused by later calls: not known)
            if flags is not None:
                ei, ew = self.ei(), (None if self.ew is None else self.ew())
                if ei is not None and (self.ew is None or ew is not None):
                    _SYMMETRIC_ADJ.put(ei, self.answer, ew)
        return bool(self.answer)


def dense_pool_select_sparse(x: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor], batch: Tensor,
                             node_ptr: Tensor, edge_ptr: Tensor, num_graphs: int, max_nodes: int, weight: Tensor,
                             bias: Optional[Tensor], flags: int, adj_transpose: bool, want_raw: bool = False,
                             mincut_terms: bool = False, want_dense: bool = False, diff_stats: bool = False):
    """(s [B,N,K], mask [B,N], x_pool, adj_raw, adj_pool, terms, batch_pool): :func:`dense_pool_select` straight from
    the un-padded batch -- x [Ntot,F], a ROW-SORTED ``edge_index`` with the per-graph ranges ``node_ptr`` / ``edge_ptr``
    [B+1] -- in ONE launch: the adjacency tiles are built in LDS from the edges, neither ``to_dense_batch`` nor
    ``to_dense_adj`` runs, no [B,N,N] tensor exists (src.py:434-450 + select/mlp_select.py:105-147 + the fused Reduce /
    Connect call).  The caller has checked the row order (``_rows_sorted``) and the ranges (``graph_edge_ptr``)."""
    dev = N.require_device(x, edge_index, edge_weight, batch, node_ptr, edge_ptr, weight, bias)
    x, weight = N.f32c(x), N.f32c(weight)
    F = x.size(1)
    K, B, Nn = weight.size(0), int(num_graphs), int(max_nodes)
    if weight.shape != (K, F) or batch.numel() != x.size(0) or node_ptr.numel() != B + 1 or edge_ptr.numel() < B + 1:
        raise ValueError("dense_pool_select_sparse: inconsistent shapes")
    row, col = _edge_rows(edge_index)
    E = row.numel()
    w = N.opt_f32_flat(edge_weight)
    b = N.opt_f32(bias)
    s = torch.empty(B, Nn, K, dtype=torch.float32, device=dev)
    mask = torch.empty(B, Nn, dtype=torch.bool, device=dev)
    x_pool = torch.empty(B, K, F, dtype=torch.float32, device=dev)
    adj_pool = torch.empty(B, K, K, dtype=torch.float32, device=dev)
    adj_raw = torch.empty(B, K, K, dtype=torch.float32, device=dev) if want_raw else None
    terms = torch.empty(2, B, dtype=torch.float32, device=dev) if mincut_terms else None
    bp = torch.empty(B * K, dtype=torch.int64, device=dev)
    # want_dense (training): also the zero-padded x [B,N,F] and the adjacency [B,N,N] the backward kernels read
    # (want_dense="adj": the adjacency alone -- DiffPool's losses read it in inference)
    xd = torch.empty(B, Nn, F, dtype=torch.float32, device=dev) if want_dense is True else None
    ad = torch.empty(B, Nn, Nn, dtype=torch.float32, device=dev) if want_dense else None
    # diff_stats (r6): a LAST value [B,4] = per-graph (sum A^2, trace(S^T A S), |S^T S|_F^2, entropy sum): DiffPool's two
    # losses without the dense adjacency (:func:`diffpool_stats_tail`)
    dstats = torch.empty(B, 4, dtype=torch.float32, device=dev) if diff_stats else None
    _checked(N.lib().tgp_dense_pool_select_sparse_f32, N.ptr(x), x.size(0), N.ptr(row) if E else None,
             N.ptr(col) if E else None, N.ptr(w), E, N.ptr(N.i64c(batch)), N.ptr(N.i64c(node_ptr)),
             N.ptr(N.i64c(edge_ptr)), N.ptr(weight), N.ptr(b), B, Nn, K, F, flags, 1 if adj_transpose else 0, ops_eps(),
             losses_eps(), N.ptr(s), mask.data_ptr(), N.ptr(x_pool), N.ptr(adj_raw), N.ptr(adj_pool), N.ptr(terms),
             N.ptr(bp), N.ptr(xd), N.ptr(ad), N.ptr(dstats), N.stream_ptr(dev))
    tail = (dstats,) if diff_stats else ()
    if want_dense:
        return (s, mask, x_pool, adj_raw, adj_pool, terms, bp, xd, ad) + tail
    return (s, mask, x_pool, adj_raw, adj_pool, terms, bp) + tail


def diffpool_stats_tail(stats: Tensor, link_scale: float, ent_scale: float) -> Tensor:
    """[2]: DiffPool's (link loss * link_scale, entropy sum * ent_scale) from the [B,4] records of
    ``dense_pool_select_sparse(diff_stats=True)`` (utils/losses.py:644-658, 476-483), one launch."""
    dev = N.require_device(stats)
    stats = N.f32c(stats)
    out = torch.empty(2, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_diffpool_stats_tail_f32, N.ptr(stats), stats.size(0), float(link_scale), float(ent_scale),
             N.ptr(out), N.stream_ptr(dev))
    return out


def dense_pool_is_small(B: int, Nn: int, K: int, F: int) -> bool:
    """Does the one-wave-per-graph kernel take this padded batch (and so its fused backward)?"""
    return bool(N.lib().tgp_dense_pool_is_small(B, Nn, K, F))


def _bcast_or_dense(t: Optional[Tensor], shape) -> Tuple[Optional[Tensor], bool]:
    """An upstream gradient as the kernel takes it: (contiguous fp32 tensor, False), or (one-element tensor, True) when
    every stride is zero -- `loss = out.sum()` sends an expanded scalar, which is read as one value instead of being
    materialised as a [B,K,F] copy."""
    if t is None:
        return None, False
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"upstream gradient {tuple(t.shape)} does not match {tuple(shape)}")
    if t.dtype == torch.float32 and t.numel() > 1 and not any(t.stride()):
        return t.as_strided((1,), (1,)), True
    return N.f32c(t), False


def dense_pool_small_bwd(s: Tensor, adj: Tensor, x: Optional[Tensor], flags: int, g_x_pool: Optional[Tensor],
                         g_adj_pool: Optional[Tensor], g_adj_raw: Optional[Tensor], g_terms: Optional[Tensor],
                         want_gx: bool = True, g_diff: Optional[Tensor] = None, diff_losses: Optional[Tensor] = None,
                         link_scale: float = 0.0, ent_scale: float = 0.0, g_mean_terms=(None, None),
                         g_diff_pair=(None, None)):
    """Gradients (gS, gX) of ``dense_pool`` (with its in-kernel MinCut terms) for a batch of small graphs, one launch:
    base_reduce.py:158-161, dense_conn.py:111-122, utils/ops.py:282-335, utils/losses.py:39-70 under autograd.
    ``g_mean_terms`` = upstream gradients (0-dim tensors or None) of the batch MEANS of the two per-graph terms;
    ``g_diff_pair`` = those of DiffPool's (link, entropy) losses as two 0-dim tensors (``g_diff`` [2] is the other form)."""
    dev = N.require_device(s, adj, x)
    s = N.f32c(s)
    B, Nn, K = s.shape
    a, tflag = _dense_adj_layout(adj)
    F = 0
    if x is not None:
        x = N.f32c(x)
        F = x.size(2)

    def grad(t, shape):
        if t is None:
            return None
        t = N.f32c(t)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"upstream gradient {tuple(t.shape)} does not match {tuple(shape)}")
        return t

    g_x_pool, bx = _bcast_or_dense(g_x_pool, (B, K, F)) if x is not None else (None, False)
    g_adj_pool, ba = _bcast_or_dense(g_adj_pool, (B, K, K))
    g_adj_raw = grad(g_adj_raw, (B, K, K))
    g_terms = grad(g_terms, (2, B))
    g_link, g_ent = g_diff_pair
    if g_diff is not None:
        g_diff = grad(g_diff, (2,))
        g_link, g_ent = g_diff[0], g_diff[1]
    g_link, g_ent = grad(g_link, ()), grad(g_ent, ())
    g_cut, g_ortho = grad(g_mean_terms[0], ()), grad(g_mean_terms[1], ())
    diff_losses = grad(diff_losses, (2,)) if (g_link is not None or g_ent is not None) else None
    gs = torch.empty(B, Nn, K, dtype=torch.float32, device=dev)
    gx = torch.empty(B, Nn, F, dtype=torch.float32, device=dev) if (want_gx and x is not None) else None
    _checked(N.lib().tgp_dense_pool_small_bwd_f32, N.ptr(s), N.ptr(a), N.ptr(x), B, Nn, K, F, flags | tflag, ops_eps(),
             losses_eps(), N.ptr(g_x_pool), N.ptr(g_adj_pool), N.ptr(g_adj_raw), N.ptr(g_terms), N.ptr(g_cut),
             N.ptr(g_ortho), N.ptr(g_link), N.ptr(g_ent), N.ptr(diff_losses), float(link_scale), float(ent_scale),
             losses_eps(), (1 if bx else 0) | (2 if ba else 0), N.ptr(gs), N.ptr(gx), N.stream_ptr(dev))
    return gs, gx


def mlp_select_bwd_fits(K: int, F: int) -> bool:
    return bool(N.lib().tgp_mlp_select_bwd_fits(F, K))


def mlp_select_bwd(s: Tensor, g_s: Tensor, x: Tensor, weight: Tensor, want_gx: bool = True, want_gw: bool = True,
                   want_gb: bool = True, gx_accumulate: Optional[Tensor] = None):
    """(gx, gw, gb) of ``mlp_select`` in one pass over S, dS and X + a tiny combine of the workgroups' partial gw / gb
    (select/mlp_select.py:139-145 under autograd; K <= 32, F <= 64):
    dY = S (dS - <dS,S>), gx = dY W -- added IN PLACE to ``gx_accumulate`` when that is given (the gradient the pooling
    backward already holds for the same X) --, gw = dY^T X, gb = column sums of dY."""
    dev = N.require_device(s, g_s, x, weight)
    s, g_s, x, weight = N.f32c(s), N.f32c(g_s), N.f32c(x), N.f32c(weight)
    K = s.size(-1)
    F = x.size(-1)
    M = s.numel() // max(K, 1)
    if g_s.shape != s.shape or x.numel() != M * F or weight.shape != (K, F):
        raise ValueError(f"mlp_select_bwd: shapes s {tuple(s.shape)}, g_s {tuple(g_s.shape)}, x {tuple(x.shape)}, "
                         f"weight {tuple(weight.shape)}")
    gx = None
    if gx_accumulate is not None:
        if (gx_accumulate.dtype != torch.float32 or not gx_accumulate.is_contiguous()
                or gx_accumulate.numel() != M * F):
            raise ValueError("mlp_select_bwd: gx_accumulate must be a contiguous float32 tensor of x's size")
        gx = gx_accumulate
    elif want_gx:
        gx = torch.empty_like(x)
    gw = torch.empty(K, F, dtype=torch.float32, device=dev) if (want_gw or want_gb) else None
    gb = torch.empty(K, dtype=torch.float32, device=dev) if want_gb else None
    L = N.lib()
    st = N.stream_ptr(dev)
    ws = None
    if gw is not None:
        ws = N.workspace(L.tgp_mlp_select_bwd_workspace_bytes(M, F, K), dev)
    _checked(L.tgp_mlp_select_bwd_f32, N.ptr(s), N.ptr(g_s), N.ptr(x), N.ptr(weight), M, F, K, N.ptr(gx),
             1 if gx_accumulate is not None else 0, N.ptr(gw), N.ptr(gb), N.ptr(ws), 0 if ws is None else ws.numel(),
             st)
    return gx, (gw if want_gw else None), gb


def postprocess_dense(adj_pool: Tensor, flags: int, inplace: bool = False) -> Tensor:
    """utils/ops.py:282-335 on a [B,K,K] tensor."""
    dev = N.require_device(adj_pool)
    f64 = adj_pool.dtype == torch.float64  # a float64 pooled adjacency is post-processed in fp64 (utils/ops.py:282-335)
    src = (N.f64c if f64 else N.f32c)(adj_pool)
    dst = src if inplace else torch.empty_like(src)
    B, K = src.size(0), src.size(1)
    L = N.lib()
    ws = N.workspace((L.tgp_postprocess_dense_workspace_bytes_f64 if f64 else L.tgp_postprocess_dense_workspace_bytes)(B, K),
                     dev)
    _checked(L.tgp_postprocess_dense_f64 if f64 else L.tgp_postprocess_dense_f32, N.ptr(src), N.ptr(dst), B, K, flags,
             ops_eps(), N.ptr(ws), ws.numel(), N.stream_ptr(dev))
    return dst


def postprocess_dense_bwd(raw: Tensor, g_post: Tensor, flags: int) -> Optional[Tensor]:
    """Gradient of :func:`postprocess_dense` with respect to its input (utils/ops.py:282-335 under autograd), one
    launch; None when the kernel does not take the case (K > 4096)."""
    dev = N.require_device(raw, g_post)
    raw = N.f32c(raw)
    B, K = raw.size(0), raw.size(1)
    if K > 4096 or tuple(g_post.shape) != tuple(raw.shape):
        return None
    # an expanded scalar (the gradient of a plain `.sum()`) is handed over as one value: no [B,K,K] copy of it (r6)
    g_post, one = _bcast_or_dense(g_post, raw.shape)
    out = torch.empty_like(raw)
    _checked(N.lib().tgp_postprocess_dense_bwd_f32, N.ptr(raw), N.ptr(g_post), B, K, flags | ((1 << 16) if one else 0),
             ops_eps(), N.ptr(out), N.stream_ptr(dev))
    return out


def entropy_bwd(s: Tensor, g: Tensor, scale: float = 1.0) -> Tensor:
    """-(log(s + eps) + s / (s + eps)) * g * scale, g a 0-d device tensor (utils/losses.py:476-483 under autograd)."""
    dev = N.require_device(s, g)
    s32 = N.f32c(s)
    out = torch.empty_like(s32)
    _checked(N.lib().tgp_entropy_bwd_f32, N.ptr(s32), s32.numel(), losses_eps(), N.ptr(N.f32c(g.reshape(1))),
             float(scale), N.ptr(out), N.stream_ptr(dev))
    return out


def _sizes_arg(graph_sizes: Optional[Tensor], num_graphs: int, dev) -> Optional[Tensor]:
    if graph_sizes is None:
        return None
    gs = N.i64c(graph_sizes)
    if gs.numel() != num_graphs or gs.device != dev:
        raise ValueError(f"graph_sizes must hold one count per graph on {dev}, got {tuple(gs.shape)} on {gs.device}")
    return gs


def link_loss_sq(s: Tensor, adj: Tensor, graph_sizes: Optional[Tensor] = None) -> Tensor:
    """sq[b] = ||adj[b] - s[b] s[b]^T||_F^2 without materialising s s^T (utils/losses.py:644-708).  float64: s s^T on
    the fp64 matrix path and the residual as the reference writes it (losses.py:644-652)."""
    dev = N.require_device(s, adj)
    if _any_f64(s, adj):
        s64 = N.f64c(s)
        sst = bmm(s64, s64.transpose(1, 2).contiguous())
        return ((adj.to(torch.float64) - sst) ** 2).sum(dim=(1, 2))
    s, adj = N.f32c(s), N.f32c(adj)
    B, Nn, K = s.shape
    if adj.shape != (B, Nn, Nn):
        raise ValueError(f"adj {tuple(adj.shape)} does not match s {tuple(s.shape)}")
    sq = torch.empty(B, dtype=torch.float32, device=dev)
    L = N.lib()
    ws = N.workspace(L.tgp_link_loss_workspace_bytes(B, Nn, K), dev)
    _checked(L.tgp_link_loss_f32, N.ptr(s), N.ptr(adj), B, Nn, K, N.ptr(_sizes_arg(graph_sizes, B, dev)), N.ptr(sq),
             N.ptr(ws), ws.numel(), N.stream_ptr(dev))
    return sq


def _entropy_partials(s: Tensor, dev, st) -> Tuple[Tensor, int]:
    """(buffer, n): the per-workgroup shares of sum(-s log(s + eps)) that the DiffPool tails add up, and their number."""
    s32, L = N.f32c(s), N.lib()
    ws = N.workspace(L.tgp_entropy_sum_workspace_bytes(s32.numel()), dev)
    n_partial = ctypes.c_int(0)
    _checked(L.tgp_entropy_partials_f32, N.ptr(s32), s32.numel(), losses_eps(), N.ptr(ws), ws.numel(),
             ctypes.addressof(n_partial), st)
    return ws, n_partial.value


def diffpool_loss_tail(s: Tensor, adj: Tensor, graph_sizes: Optional[Tensor], link_scale: float,
                       ent_scale: float) -> Tensor:
    """[2]: DiffPool's link-prediction loss sqrt(sum_b ||adj_b - s_b s_b^T||^2) * link_scale and entropy loss
    sum(-s log(s + eps)) * ent_scale (poolers/diffpool.py:262-284) -- the two native partial reductions and ONE tail
    launch (outside autograd)."""
    dev = N.require_device(s, adj)
    sq = link_loss_sq(s, adj, graph_sizes)
    st = N.stream_ptr(dev)
    ws, n_partial = _entropy_partials(s, dev, st)
    out = torch.empty(2, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_diffpool_loss_tail_f32, N.ptr(sq), sq.numel(), N.ptr(ws), n_partial, float(link_scale),
             float(ent_scale), N.ptr(out), st)
    return out


def entropy_sum(s: Tensor) -> Tensor:
    """0-d tensor sum(-s log(s + eps)) over every element (utils/losses.py:476-483 before / num_nodes)."""
    dev = N.require_device(s)
    if s.dtype == torch.float64:  # one elementwise pass + a sum, in double like the reference's
        return (-(s * torch.log(s + losses_eps()))).sum()
    s = N.f32c(s)
    out = torch.empty((), dtype=torch.float32, device=dev)
    L = N.lib()
    ws = N.workspace(L.tgp_entropy_sum_workspace_bytes(s.numel()), dev)
    _checked(L.tgp_entropy_sum_f32, N.ptr(s), s.numel(), losses_eps(), N.ptr(out), N.ptr(ws), ws.numel(),
             N.stream_ptr(dev))
    return out


def _cut_terms_f32(dev, adj: Tensor, s: Tensor, graph_sizes: Optional[Tensor], want_den: bool):
    """(deg [B,N], q [B,N], den [B] or None) from one launch of ``tgp_cut_terms_f32``."""
    adj, s = N.f32c(adj), N.f32c(s)
    B, Nn, K = s.shape
    if adj.shape != (B, Nn, Nn):
        raise ValueError(f"adj {tuple(adj.shape)} does not match s {tuple(s.shape)}")
    deg = torch.empty(B, Nn, dtype=torch.float32, device=dev)
    q = torch.empty(B, Nn, dtype=torch.float32, device=dev)
    den = torch.empty(B, dtype=torch.float32, device=dev) if want_den else None
    _checked(N.lib().tgp_cut_terms_f32, N.ptr(adj), N.ptr(s), B, Nn, K, N.ptr(_sizes_arg(graph_sizes, B, dev)),
             N.ptr(deg), N.ptr(q), N.ptr(den), N.stream_ptr(dev))
    return deg, q, den


def cut_terms(adj: Tensor, s: Tensor, graph_sizes: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """(deg [B,N], q [B,N], den [B]): row sums of adj, squared row norms of s, trace(s^T D s)
    (utils/losses.py:39-81)."""
    dev = N.require_device(adj, s)
    if _any_f64(adj, s):
        a64, s64 = adj.to(torch.float64), s.to(torch.float64)
        deg, q = a64.sum(-1), (s64 * s64).sum(-1)
        return deg, q, (deg * q).sum(-1)
    return _cut_terms_f32(dev, adj, s, graph_sizes, True)


def cut_rows(adj: Tensor, s: Tensor, graph_sizes: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(deg [B,N], q [B,N]) of :func:`cut_terms` without the per-graph dot product (one launch: the training step's fused
    loss tail forms den itself, :func:`mincut_terms_fused`)."""
    return _cut_terms_f32(N.require_device(adj, s), adj, s, graph_sizes, False)[:2]


def mincut_terms_fused(raw: Tensor, gram: Tensor, deg: Optional[Tensor], q: Optional[Tensor],
                       ptr: Optional[Tensor] = None, want_means: bool = False, edges=None):
    """(den [B], terms [2,B], stats [B,4][, means [2]]): MinCut's per-graph loss tails with den = sum_i deg_i q_i formed
    in the same launch (utils/losses.py:39-70); stats = (trace(raw), |G|^2, trace(G), |Y|) per graph, the scalars the
    backward's right-hand sides need; ``want_means``: also the batch means of the two terms (what the pooler hands out)."""
    dev = N.require_device(raw, gram, deg, q)
    raw, gram = N.f32c(raw), N.f32c(gram)
    deg = N.opt_f32(deg)
    q = N.opt_f32(q)  # (None: deg already carries the factor, den = sum of deg)
    # edges = (row_ptr int32 [Ntot+1], edge_index, weights or None) of an un-padded batch: den = sum_e w_e q[col_e], the
    # in-degree form (S^T A^T S of the batched poolers on the rows route); deg is then not read
    e_rp = e_col = e_w = None
    if edges is not None:
        if ptr is None or q is None:
            raise ValueError("mincut_terms_fused(edges=...) needs ptr and q")
        e_rp, e_ei, e_w = edges
        e_col = _edge_rows(e_ei)[1]
        e_w = N.opt_f32_flat(e_w)
    B, Kc, Nn = raw.size(0), raw.size(-1), (deg if deg is not None else q).size(-1)
    den = torch.empty(B, dtype=torch.float32, device=dev)
    out = torch.empty(2, B, dtype=torch.float32, device=dev)
    stats = torch.empty(B, 4, dtype=torch.float32, device=dev)
    st = N.stream_ptr(dev)
    means = ticket = None
    if want_means and B <= 256 and not torch.cuda.is_current_stream_capturing():
        # the batch means come with the same launch (its last workgroup adds the terms up in graph order); for thousands
        # of graphs the arrival tickets on ONE word cost more than the reduction launch they save (2048 graphs: +40 us)
        means = torch.empty(2, dtype=torch.float32, device=dev)
        ticket = _sps_state(dev, st, 0).ticket.data_ptr() + 16
    # ptr: deg / q belong to an un-padded batch (graph b owns entries ptr[b] .. ptr[b+1])
    _checked(N.lib().tgp_mincut_terms_fused_f32, N.ptr(raw), N.ptr(gram), N.ptr(deg), N.ptr(q), B, Nn, Kc, losses_eps(),
             N.ptr(den), N.ptr(out), N.ptr(stats), N.ptr(N.opt_i64(ptr)), ticket, N.ptr(means), N.ptr(e_rp),
             N.ptr(e_col), N.ptr(e_w), st)
    if want_means:
        return den, out, stats, (means if means is not None else out.mean(dim=1))
    return den, out, stats


def dense_pool_train_fwd(s: Tensor, adj_mem: Tensor, x: Tensor, flags: int, acat: Tensor, want_gram: bool,
                         want_post: bool = True):
    """(x_pool, raw, adj_pool, gram): forward of the dense poolers' training step beyond the one-wave kernels
    (base_reduce.py:158-161, dense_conn.py:111-122, utils/ops.py:282-335).  ``adj_mem`` is the contiguous adjacency
    memory (``flags`` carries ``ADJ_TRANSPOSED`` when it holds A^T), ``acat`` [B,N,3K+F+4] the operand buffer of the
    backward whose first K columns receive U = A S; ``gram`` = S^T S when asked for."""
    dev = N.require_device(s, adj_mem, x, acat)
    B, Nn, Kc = s.shape
    F = x.size(2)
    ld = acat.size(2)
    if (adj_mem.shape != (B, Nn, Nn) or x.shape[:2] != (B, Nn) or acat.shape[:2] != (B, Nn) or ld < Kc
            or not (s.is_contiguous() and adj_mem.is_contiguous() and x.is_contiguous() and acat.is_contiguous())):
        raise ValueError("dense_pool_train_fwd: inconsistent shapes or non-contiguous operands")
    x_pool = torch.empty(B, Kc, F, dtype=torch.float32, device=dev)
    raw = torch.empty(B, Kc, Kc, dtype=torch.float32, device=dev)
    adj_pool = torch.empty(B, Kc, Kc, dtype=torch.float32, device=dev) if want_post else None
    gram = torch.empty(B, Kc, Kc, dtype=torch.float32, device=dev) if want_gram else None
    L = N.lib()
    ws = N.workspace(L.tgp_dense_pool_train_workspace_bytes(B, Nn, Kc, F), dev)
    _checked(L.tgp_dense_pool_train_fwd_f32, N.ptr(s), N.ptr(adj_mem), N.ptr(x), B, Nn, Kc, F, flags, ops_eps(),
             N.ptr(acat), ld, N.ptr(x_pool), N.ptr(raw), N.ptr(adj_pool), N.ptr(gram), N.ptr(ws), ws.numel(),
             N.stream_ptr(dev))
    return x_pool, raw, adj_pool, gram


def dense_pool_train_rhs(g_raw_a: Optional[Tensor], g_raw_b: Optional[Tensor], mode: int, stats: Optional[Tensor],
                         den: Optional[Tensor], gram: Optional[Tensor], g_la: Optional[Tensor], g_lb: Optional[Tensor],
                         scale: float, link_loss: Optional[Tensor], link_scale: float, g_x: Optional[Tensor],
                         gx_bcast: bool, symmetric: bool, weight: Optional[Tensor], B: int, Kc: int, F: int, dev):
    """(rcat [B,3K+F+4,K], c1 [B] or None, gw [B,2K,F] or None): the right-hand sides [RU ; RX ; 0 ; RS ; RV] of the
    training step's backward GEMM and, with the selector's ``weight``, [g_x ; W] for gX = [S | dY] [g_x ; W]
    (see tgp_dense_pool_train_rhs_f32 in include/tgp_hip.h).  ``symmetric``: bool, or the flag word (bit 0: A = A^T,
    bit 1: the RU / RV slots trade places)."""
    rcat = torch.empty(B, train_columns(Kc, F).ld, Kc, dtype=torch.float32, device=dev)
    c1 = torch.empty(B, dtype=torch.float32, device=dev) if mode == 1 else None
    gw = torch.empty(B, 2 * Kc, F, dtype=torch.float32, device=dev) if weight is not None else None
    w = None if weight is None else N.f32c(weight.detach())
    _checked(N.lib().tgp_dense_pool_train_rhs_f32, N.ptr(g_raw_a), N.ptr(g_raw_b), mode, N.ptr(stats), N.ptr(den),
             N.ptr(gram), N.ptr(g_la), N.ptr(g_lb), float(scale), N.ptr(link_loss), float(link_scale), losses_eps(),
             N.ptr(g_x), 1 if gx_bcast else 0, int(symmetric), N.ptr(w), B, Kc, F, N.ptr(rcat), N.ptr(c1), N.ptr(gw),
             N.stream_ptr(dev))
    return rcat, c1, gw


def softmax_bwd_ex(s: Tensor, ds: Tensor, extra: Optional[Tensor] = None, c1: Optional[Tensor] = None,
                   deg: Optional[Tensor] = None, ent_g: Optional[Tensor] = None, ent_scale: float = 0.0,
                   out: Optional[Tensor] = None, batch: Optional[Tensor] = None) -> Tensor:
    """:func:`softmax_bwd` on dS + extra + 2 c1[graph] deg[row] S - ent_g ent_scale (log(S + eps) + S / (S + eps)):
    the elementwise parts of the pooling step's gradient folded into the selector's softmax backward.  s [B,N,K];
    ``out``: a [B,N,K] float32 view with unit last stride and uniform row stride (a column block of a wider buffer)."""
    dev = N.require_device(s, ds)
    if s.dim() == 2:  # un-padded batch [Ntot,K]: the graph of a row comes from ``batch`` (one graph without it)
        B, (Nn, Kc) = 1, s.shape
    else:
        B, Nn, Kc = s.shape
    s2, d2 = N.f32c(s), N.f32c(ds)
    ex = N.opt_f32(extra)
    if d2.numel() != s2.numel() or (ex is not None and ex.numel() != s2.numel()):
        raise ValueError("softmax_bwd_ex: gradient shapes do not match s")
    if out is None:
        out = torch.empty_like(s2)
    elif (out.shape != s2.shape or out.dtype != torch.float32 or out.stride(-1) != 1
          or (out.dim() == 3 and out.stride(0) != Nn * out.stride(1))):
        raise ValueError("softmax_bwd_ex: out must be a float32 view of s's shape with a uniform row stride")
    _checked(N.lib().tgp_softmax_bwd_ex_f32, N.ptr(s2), N.ptr(d2), N.ptr(ex), N.ptr(N.opt_f32(c1)),
             N.ptr(N.opt_f32(deg)), Nn, N.ptr(None if ent_g is None else N.f32c(ent_g.reshape(1))), float(ent_scale),
             losses_eps(), out.data_ptr(), out.stride(-2), B * Nn, Kc, N.ptr(N.opt_i64(batch)), N.stream_ptr(dev))
    return out


TRAIN_PAD = 4  # width of the [1 0 0 0] column block of the training step's operand buffer (csrc/losses.hip)


# the training step's operand buffer [U | X | 1 0 0 0 | S | V]: its row length and where the blocks behind U begin
TrainColumns = namedtuple("TrainColumns", "ld c_x c_one c_s c_v")


def train_columns(Kc: int, F: int) -> TrainColumns:
    return TrainColumns(3 * Kc + F + TRAIN_PAD, Kc, Kc + F, Kc + F + TRAIN_PAD, 2 * Kc + F + TRAIN_PAD)


def copy_cols2(a: Tensor, b: Tensor, dst: Tensor, col_a: int, col_b: int, one_col: int = -1) -> None:
    """dst[:, col_a:col_a+wa] = a, dst[:, col_b:col_b+wb] = b for row-major 2-D float32 tensors, one launch;
    ``one_col >= 0``: also dst[:, one_col:one_col+4] = [1 0 0 0]."""
    dev = N.require_device(a, b, dst)
    if not (a.is_contiguous() and b.is_contiguous() and dst.is_contiguous()) or a.size(0) != dst.size(0) \
            or b.size(0) != dst.size(0):
        raise ValueError("copy_cols2: operands must be contiguous with equal row counts")
    _checked(N.lib().tgp_copy_cols2_f32, N.ptr(a), a.size(1), N.ptr(b), b.size(1), dst.size(0), N.ptr(dst), dst.size(1),
             col_a, col_b, one_col, N.stream_ptr(dev))


def copy_cols3(a: Tensor, b: Tensor, c: Tensor, dst: Tensor, col_a: int, col_b: int, col_c: int, one_col: int = -1) -> None:
    """:func:`copy_cols2` with a third source block: dst[:, col_c:col_c+wc] = c."""
    dev = N.require_device(a, b, c, dst)
    if not all(t.is_contiguous() and t.size(0) == dst.size(0) for t in (a, b, c)) or not dst.is_contiguous():
        raise ValueError("copy_cols3: operands must be contiguous with equal row counts")
    _checked(N.lib().tgp_copy_cols3_f32, N.ptr(a), a.size(1), N.ptr(b), b.size(1), N.ptr(c), c.size(1), dst.size(0),
             N.ptr(dst), dst.size(1), col_a, col_b, col_c, one_col, N.stream_ptr(dev))


def slab_sum_split(part: Tensor, F: int, want_gw: bool = True, want_gb: bool = True):
    """(gw [K,F], gb [K]) from part [slabs,K,W]: columns 0..F-1 and column F of the slab sum as two contiguous tensors."""
    dev = N.require_device(part)
    slabs, Kc, W = part.shape
    gw = torch.empty(Kc, F, dtype=torch.float32, device=dev) if want_gw else None
    gb = torch.empty(Kc, dtype=torch.float32, device=dev) if want_gb else None
    _checked(N.lib().tgp_slab_sum_split_f32, N.ptr(part), slabs, Kc, F, W, N.ptr(gw), N.ptr(gb), N.stream_ptr(dev))
    return gw, gb


def bmm_into(a: Tensor, b: Tensor, out: Tensor, trans_a: bool = False, accumulate: bool = False) -> Tensor:
    """out[g] (+)= op(a[g]) @ b[g] for float32 3-D VIEWS: any batch / row strides, unit stride along the last dimension
    (column blocks of a wider buffer: no copies in, no copy out)."""
    dev = N.require_device(a, b, out)
    for t in (a, b, out):
        if t.dim() != 3 or t.dtype != torch.float32 or t.stride(2) != 1:
            raise ValueError("bmm_into: float32 3-D views with unit last stride expected")
    G = out.size(0)
    Kd, M = (a.size(1), a.size(2)) if trans_a else (a.size(2), a.size(1))
    Nc = b.size(2)
    if b.size(1) != Kd or out.shape[1:] != (M, Nc) or a.size(0) not in (1, G) or b.size(0) not in (1, G):
        raise ValueError(f"bmm_into: shapes {tuple(a.shape)} x {tuple(b.shape)} -> {tuple(out.shape)}")
    sA = 0 if a.size(0) == 1 else a.stride(0)
    sB = 0 if b.size(0) == 1 else b.stride(0)
    L = N.lib()
    _checked(L.tgp_bmm_accumulate_f32 if accumulate else L.tgp_bmm_f32, a.data_ptr(), b.data_ptr(), out.data_ptr(), G,
             M, Nc, Kd, 1 if trans_a else 0, a.stride(1), b.stride(1), out.stride(1), sA, sB, out.stride(0),
             N.stream_ptr(dev))
    return out


def _adj_grad_operands(who: str, s: Tensor, adj: Optional[Tensor], **square):
    """Shared checks of the two adjacency-gradient wrappers: s [B,N,K] float32 with unit last stride, adj [B,N,N]
    contiguous float32 or None, every ``square`` operand [B,K,K] or None."""
    if s.dim() != 3 or s.dtype != torch.float32 or s.stride(2) != 1 or s.size(2) < 1:
        raise ValueError(f"{who}: s must be a float32 [B,N,K] tensor (K >= 1) with unit last stride, got "
                         f"{tuple(s.shape)} {s.dtype}")
    B, Nn, Kc = s.shape
    if adj is not None and (adj.shape != (B, Nn, Nn) or adj.dtype != torch.float32 or not adj.is_contiguous()):
        raise ValueError(f"{who}: adj must be a contiguous float32 {(B, Nn, Nn)} tensor, got {tuple(adj.shape)} {adj.dtype}")
    for name, t in square.items():
        if t is not None and (t.shape != (B, Kc, Kc) or t.dtype != torch.float32):
            raise ValueError(f"{who}: {name} must be a float32 {(B, Kc, Kc)} tensor, got {tuple(t.shape)} {t.dtype}")
    return B, Nn, Kc


def _dev_scalar(who: str, name: str, t: Optional[Tensor]) -> Optional[Tensor]:
    """A 0-dim / one-element float32 device value of a native call (never read on the host), or None."""
    if t is None:
        return None
    if t.numel() != 1:
        raise ValueError(f"{who}: {name} must hold one value, got {tuple(t.shape)}")
    return N.f32c(t.reshape(1))


def dense_pool_adj_grad(s: Tensor, adj: Optional[Tensor], m: Tensor, gamma: Optional[Tensor] = None,
                        q: Optional[Tensor] = None, g_link: Optional[Tensor] = None,
                        link_loss: Optional[Tensor] = None, link_scale: float = 0.0) -> Tensor:
    """dA [B,N,N] = S M S^T + gamma_b q_i + c A of the dense poolers' training step (connect/dense_conn.py:111-122,
    utils/losses.py:39-56, 644-652 under autograd), any N and K: ``m`` [B,K,K] = the total gradient of S^T A S (a view
    with unit last stride: the RV block of :func:`dense_pool_train_rhs`), ``gamma`` [B] = its ``c1`` (MinCut) with
    ``q`` [B,N] = |s_i|^2 (:func:`cut_rows`; None: formed in the kernel), ``g_link`` / ``link_loss`` = DiffPool's upstream
    gradient and forward value (0-dim device tensors: c = link_scale^2 g_link / link_loss, ``adj`` is read only then).
    T = S M (:func:`bmm_into`'s kernel) + one N^2 K launch on the fp32 matrix cores that writes dA once."""
    who = "dense_pool_adj_grad"
    dev = N.require_device(s, adj, m, gamma, q, g_link, link_loss)
    B, Nn, Kc = _adj_grad_operands(who, s, adj)
    if m.dim() != 3 or m.shape != (B, Kc, Kc) or m.dtype != torch.float32 or m.stride(2) != 1:
        raise ValueError(f"{who}: m must be a float32 {(B, Kc, Kc)} view with unit last stride, got {tuple(m.shape)} {m.dtype}")
    if gamma is not None:
        gamma = N.f32c(gamma)
        if gamma.shape != (B,):
            raise ValueError(f"{who}: gamma must be [{B}], got {tuple(gamma.shape)}")
    if q is not None:
        q = N.f32c(q)
        if q.shape != (B, Nn):
            raise ValueError(f"{who}: q must be {(B, Nn)}, got {tuple(q.shape)}")
    g_link, link_loss = _dev_scalar(who, "g_link", g_link), _dev_scalar(who, "link_loss", link_loss)
    if g_link is not None and (link_loss is None or adj is None):
        raise ValueError(f"{who}: g_link needs link_loss and adj")
    out = torch.empty(B, Nn, Nn, dtype=torch.float32, device=dev)
    t = torch.empty(B, Nn, Kc, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_dense_pool_adj_grad_f32, s.data_ptr(), s.stride(1), s.stride(0), N.ptr(adj), m.data_ptr(),
             m.stride(1), m.stride(0), N.ptr(gamma), N.ptr(q), N.ptr(g_link), N.ptr(link_loss), float(link_scale), B, Nn,
             Kc, N.ptr(t), N.ptr(out), N.stream_ptr(dev))
    return out


def dense_pool_adj_grad_small(s: Tensor, adj: Tensor, ga: Optional[Tensor] = None, g_raw: Optional[Tensor] = None,
                              raw: Optional[Tensor] = None, g_terms: Optional[Tensor] = None,
                              g_mean_cut: Optional[Tensor] = None, g_link: Optional[Tensor] = None,
                              link_loss: Optional[Tensor] = None, link_scale: float = 0.0) -> Tensor:
    """:func:`dense_pool_adj_grad` for batches of small graphs (N <= 64, K <= 32: what ``dense_pool_is_small`` accepts),
    one wave per graph, one launch behind :func:`dense_pool_small_bwd`.  M is formed in the kernel: ``ga`` (the output of
    :func:`postprocess_dense_bwd`) + ``g_raw`` (each [B,K,K] or None) - (g_b / (den_b + eps) + c) I with g_b =
    ``g_terms``[0,b] + ``g_mean_cut`` / B (each optional; they need ``raw`` = the forward's S^T A S)."""
    who = "dense_pool_adj_grad_small"
    dev = N.require_device(s, adj, ga, g_raw, raw, g_terms, g_mean_cut, g_link, link_loss)
    s = N.f32c(s)
    B, Nn, Kc = _adj_grad_operands(who, s, adj, ga=ga, g_raw=g_raw, raw=raw)
    if Nn > 64 or Kc > 32:
        raise ValueError(f"{who}: one wave per graph takes N <= 64 and K <= 32, got N = {Nn}, K = {Kc}")
    ga, g_raw, raw = N.opt_f32(ga), N.opt_f32(g_raw), N.opt_f32(raw)
    if g_terms is not None:
        g_terms = N.f32c(g_terms)
        if g_terms.shape != (2, B):
            raise ValueError(f"{who}: g_terms must be {(2, B)}, got {tuple(g_terms.shape)}")
    g_mean_cut = _dev_scalar(who, "g_mean_cut", g_mean_cut)
    g_link, link_loss = _dev_scalar(who, "g_link", g_link), _dev_scalar(who, "link_loss", link_loss)
    if (g_terms is not None or g_mean_cut is not None) and raw is None:
        raise ValueError(f"{who}: the cut term needs raw")
    if g_link is not None and link_loss is None:
        raise ValueError(f"{who}: g_link needs link_loss")
    out = torch.empty(B, Nn, Nn, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_dense_pool_adj_grad_small_f32, N.ptr(s), N.ptr(adj), N.ptr(ga), N.ptr(g_raw), N.ptr(raw),
             N.ptr(g_terms), N.ptr(g_mean_cut), N.ptr(g_link), N.ptr(link_loss), float(link_scale), losses_eps(), B, Nn,
             Kc, N.ptr(out), N.stream_ptr(dev))
    return out


def mincut_loss_terms(raw: Tensor, den: Tensor, gram: Tensor) -> Tensor:
    """[2,B]: per-graph -trace(raw)/(den + eps) and ||G/||G|| - I/sqrt(K)||_F (utils/losses.py:39-70), one launch."""
    dev = N.require_device(raw, den, gram)
    raw, den, gram = N.f32c(raw), N.f32c(den), N.f32c(gram)
    B, Kc = raw.size(0), raw.size(-1)
    out = torch.empty(2, B, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_mincut_loss_terms_f32, N.ptr(raw), N.ptr(den), N.ptr(gram), B, Kc, losses_eps(), N.ptr(out),
             N.stream_ptr(dev))
    return out


def mincut_loss_terms_bwd(raw: Tensor, den: Tensor, gram: Tensor, g_terms: Tensor):
    """(g_raw [B,K,K], c1 [B], W [B,K,K]): gradients of :func:`mincut_loss_terms` with respect to raw, den and gram from
    the upstream gradients [2,B] (utils/losses.py:39-70 under autograd), one launch."""
    dev = N.require_device(raw, den, gram, g_terms)
    raw, den, gram, g_terms = N.f32c(raw), N.f32c(den), N.f32c(gram), N.f32c(g_terms)
    B, Kc = raw.size(0), raw.size(-1)
    g_raw = torch.empty_like(raw)
    W = torch.empty_like(raw)
    c1 = torch.empty(B, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_mincut_loss_terms_bwd_f32, N.ptr(raw), N.ptr(den), N.ptr(gram), N.ptr(g_terms), B, Kc,
             losses_eps(), N.ptr(g_raw), N.ptr(c1), N.ptr(W), N.stream_ptr(dev))
    return g_raw, c1, W


_PART_ROWS = 64  # rows of one graph per workgroup of the DMoN / HOSC / Just Balance partial passes (PART_ROWS, csrc/loss_common.h)


def _mask_bytes(mask: Optional[Tensor], B: int, Nn: int) -> Optional[Tensor]:
    if mask is None:
        return None
    if tuple(mask.shape) != (B, Nn):
        raise ValueError(f"mask {tuple(mask.shape)} does not match the batch ({B}, {Nn})")
    m = mask if mask.dtype == torch.bool else mask != 0
    return m.contiguous().view(torch.uint8)


def dmon_dense_terms(adj: Optional[Tensor], s: Tensor, mask: Optional[Tensor] = None,
                     graph_sizes: Optional[Tensor] = None, deg: Optional[Tensor] = None) -> Tuple[Optional[Tensor], Tensor]:
    """(deg [B,N] or None, part [B,ceil(N/64),2K+2]) of a padded batch: degrees d = row sums of adj on real rows (one pass
    over adj) and the per-block partial sums (S^T d | S^T 1 | sum d | node count) of DMoN's losses
    (utils/losses.py:1083-1148, 1216-1265).  ``adj`` None: the degrees ``deg`` [B,N] given (:func:`dmon_edge_degrees`),
    or none (the cluster loss alone)."""
    dev = N.require_device(adj, s, mask, deg)
    s = N.f32c(s)
    B, Nn, Kc = s.shape
    a = None
    if adj is not None:
        a = N.f32c(adj)
        if a.shape != (B, Nn, Nn):
            raise ValueError(f"adj {tuple(adj.shape)} does not match s {tuple(s.shape)}")
    nsplit = max(1, -(-Nn // _PART_ROWS))
    if a is not None:
        deg = torch.empty(B, Nn, dtype=torch.float32, device=dev)
    elif deg is not None:
        deg = N.f32c(deg)
        if deg.shape != (B, Nn):
            raise ValueError(f"deg {tuple(deg.shape)} does not match s {tuple(s.shape)}")
    part = torch.empty(B, nsplit, 2 * Kc + 2, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_dmon_dense_terms_f32, N.ptr(a), N.ptr(s), B, Nn, Kc, N.ptr(_sizes_arg(graph_sizes, B, dev)),
             N.ptr(_mask_bytes(mask, B, Nn)), nsplit, N.ptr(deg), N.ptr(part), N.stream_ptr(dev))
    return deg, part


def dmon_edge_degrees(edge_index: Tensor, edge_weight: Optional[Tensor], node_ptr: Tensor, edge_ptr: Tensor,
                      max_nodes: int, in_degrees: bool) -> Tensor:
    """deg [B,max_nodes] (padded) of a row-sorted edge list with per-graph node / edge offsets: the row sums of the
    densified adjacency (``in_degrees``: of its transpose, what the batched poolers densify when adj_transpose), one
    launch, summed in edge order."""
    dev = N.require_device(edge_index, edge_weight, node_ptr, edge_ptr)
    row, col = _edge_rows(edge_index)
    key = col if in_degrees else row
    w = N.opt_f32_flat(edge_weight)
    B = node_ptr.numel() - 1
    deg = torch.empty(B, int(max_nodes), dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_dmon_edge_degrees_f32, N.ptr(key) if key.numel() else None, N.ptr(w), key.numel(),
             N.ptr(N.i64c(node_ptr)), N.ptr(N.i64c(edge_ptr)), B, int(max_nodes), N.ptr(deg), N.stream_ptr(dev))
    return deg


def dmon_node_terms(s: Tensor, deg: Optional[Tensor], ptr: Tensor, max_nodes: int) -> Tensor:
    """part [B,ceil(max_nodes/64),2K+2] of :func:`dmon_dense_terms` for an un-padded batch: s [Ntot,K], deg [Ntot] (None:
    the cluster loss alone), ptr [B+1] node offsets of the sorted batch, ``max_nodes`` its largest graph."""
    dev = N.require_device(s, deg, ptr)
    s, ptr = N.f32c(s), N.i64c(ptr)
    d = N.opt_f32_flat(deg)
    if d is not None and d.numel() != s.size(0):
        raise ValueError("dmon_node_terms: deg must hold one value per row of s")
    B, Kc = ptr.numel() - 1, s.size(1)
    nsplit = max(1, -(-int(max_nodes) // _PART_ROWS))
    part = torch.empty(B, nsplit, 2 * Kc + 2, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_dmon_node_terms_f32, N.ptr(s), N.ptr(d), N.ptr(ptr), B, Kc, nsplit, N.ptr(part),
             N.stream_ptr(dev))
    return part


def dmon_loss_terms(part: Tensor, raw: Optional[Tensor], tr: Optional[Tensor], gram: Optional[Tensor], sqrt_k: float,
                    clamp_m: bool, coeffs=(1.0, 1.0, 1.0)):
    """(out [3,B], ca [B,K], cs [B,K], stats [B,4]): DMoN's per-graph spectral, cluster and orthogonality terms, each
    times its coefficient in ``coeffs``, in one launch from the partial sums of :func:`dmon_dense_terms` /
    :func:`dmon_node_terms`; trace(S^T A S) from the diagonal of ``raw`` or from ``tr`` [B]; ``gram`` None: the
    orthogonality row is 0."""
    dev = N.require_device(part, raw, tr, gram)
    part = N.f32c(part)
    B, nsplit, P = part.shape
    Kc = (P - 2) // 2
    raw = N.opt_f32(raw)
    tr = N.opt_f32_flat(tr)
    gram = N.opt_f32(gram)
    for t, shape in ((raw, (B, Kc, Kc)), (gram, (B, Kc, Kc)), (tr, (B,))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"dmon_loss_terms: operand {tuple(t.shape)}, expected {shape}")
    out = torch.empty(3, B, dtype=torch.float32, device=dev)
    ca = torch.empty(B, Kc, dtype=torch.float32, device=dev)
    cs = torch.empty(B, Kc, dtype=torch.float32, device=dev)
    stats = torch.empty(B, 4, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_dmon_loss_terms_f32, N.ptr(part), nsplit, N.ptr(raw), N.ptr(tr), N.ptr(gram), B, Kc,
             float(sqrt_k), 1 if clamp_m else 0, losses_eps(), *(float(c) for c in coeffs), N.ptr(out), N.ptr(ca),
             N.ptr(cs), N.ptr(stats), N.stream_ptr(dev))
    return out, ca, cs, stats


def dmon_loss_terms_bwd(g_terms: Tensor, stats: Tensor, gram: Optional[Tensor], Kc: int, sqrt_k: float, want_raw: bool,
                        want_tr: bool, coeffs=(1.0, 1.0, 1.0)):
    """(g_raw [B,K,K] or None, g_tr [B] or None, coef [B,2], W [B,K,K] or None): the gradients of
    :func:`dmon_loss_terms` (same ``coeffs``) from the upstream gradients [3,B], one launch (see
    tgp_dmon_loss_terms_bwd_f32)."""
    dev = N.require_device(g_terms, stats, gram)
    g_terms, stats = N.f32c(g_terms), N.f32c(stats)
    gram = N.opt_f32(gram)
    B = stats.size(0)
    g_raw = torch.empty(B, Kc, Kc, dtype=torch.float32, device=dev) if want_raw else None
    g_tr = torch.empty(B, dtype=torch.float32, device=dev) if want_tr else None
    W = torch.empty(B, Kc, Kc, dtype=torch.float32, device=dev) if gram is not None else None
    coef = torch.empty(B, 2, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_dmon_loss_terms_bwd_f32, N.ptr(g_terms), N.ptr(stats), N.ptr(gram), B, Kc, float(sqrt_k),
             *(float(c) for c in coeffs), N.ptr(g_raw), N.ptr(g_tr), N.ptr(coef), N.ptr(W), N.stream_ptr(dev))
    return g_raw, g_tr, coef, W


def dmon_ds(deg: Optional[Tensor], ca: Tensor, cs: Tensor, coef: Tensor, rows: int, nodes_per_graph: int,
            batch: Optional[Tensor], out: Tensor, accumulate: bool) -> Tensor:
    """out[r,k] (+)= coef[b,0] deg[r] ca[b,k] + coef[b,1] cs[b,k] over the ``rows`` rows of S: the spectral and cluster
    parts of DMoN's dS, one elementwise pass.  Graph of a row: batch[r] (un-padded) or r // nodes_per_graph."""
    dev = N.require_device(deg, ca, cs, coef, batch, out)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != rows * ca.size(1):
        raise ValueError("dmon_ds: out must be a contiguous float32 tensor of rows x K values")
    d = N.opt_f32_flat(deg)
    b = N.opt_i64(batch)
    _checked(N.lib().tgp_dmon_ds_f32, N.ptr(d), N.ptr(N.f32c(ca)), N.ptr(N.f32c(cs)), N.ptr(N.f32c(coef)), rows,
             nodes_per_graph, N.ptr(b), ca.size(0), ca.size(1), 1 if accumulate else 0, out.data_ptr(),
             N.stream_ptr(dev))
    return out


def jb_terms(s: Tensor, mask: Optional[Tensor] = None, graph_sizes: Optional[Tensor] = None,
             ptr: Optional[Tensor] = None, max_nodes: Optional[int] = None, normalize: bool = True,
             num_nodes: Optional[int] = None, num_supernodes: Optional[int] = None, scale: float = 1.0,
             want_coef: bool = True, want_mean: bool = False):
    """(out [B], coef [B,K]): Just Balance's per-graph loss -sum_k sqrt(sum_i S_ik^2 + eps) / sqrt(n_b K) times
    ``scale`` (utils/losses.py:553-594, 1013-1080; only the diagonal of S^T S is computed) and the coefficients
    -scale / (sqrt(c_k + eps) sqrt(n_b K)) of its backward.  Padded ``s`` [B,N,K]: every graph's rows below
    ``graph_sizes`` (None: all N) are summed; n_b = the mask's true entries, else the graph's size, else ``num_nodes``
    (None: N).  Un-padded ``s`` [Ntot,K] with ``ptr`` [B+1] of the sorted batch and ``max_nodes`` its largest graph:
    n_b = the graph's rows.  One launch when no graph has more than 64 rows, a partial pass and a tail otherwise.
    ``want_coef`` False (inference): coef is None and not written.  ``want_mean``: a third value, the 0-dim batch mean
    of out, from one more launch of the same native call (a fixed order of additions)."""
    dev = N.require_device(s, mask, graph_sizes, ptr)
    s = N.f32c(s)
    if ptr is None:
        if s.dim() != 3:
            raise ValueError(f"jb_terms: a padded batch is [B,N,K], got {tuple(s.shape)}")
        B, Nn, Kc = s.shape
        rows_max = Nn
        sizes, m, p = _sizes_arg(graph_sizes, B, dev), _mask_bytes(mask, B, Nn), None
    else:
        if s.dim() != 2 or mask is not None or graph_sizes is not None or max_nodes is None:
            raise ValueError("jb_terms: an un-padded batch is [Ntot,K] with ptr and max_nodes, without mask or sizes")
        p = N.i64c(ptr)
        B, Nn, Kc = p.numel() - 1, 0, s.size(1)
        rows_max = int(max_nodes)
        sizes = m = None
    if Kc < 1:
        raise ValueError("jb_terms: S needs at least one column")
    nsplit = max(1, -(-rows_max // _PART_ROWS))
    part = torch.empty(B, nsplit, Kc, dtype=torch.float32, device=dev) if nsplit > 1 else None
    out = torch.empty(B, dtype=torch.float32, device=dev)
    coef = torch.empty(B, Kc, dtype=torch.float32, device=dev) if want_coef else None
    mean = torch.empty((), dtype=torch.float32, device=dev) if want_mean else None
    _checked(N.lib().tgp_jb_terms_f32, N.ptr(s), B, Nn, Kc, N.ptr(sizes), N.ptr(m), N.ptr(p), rows_max,
             1 if normalize else 0, float(Nn if num_nodes is None else num_nodes),
             float(Kc if num_supernodes is None else num_supernodes), losses_eps(), float(scale), N.ptr(part),
             N.ptr(out), N.ptr(coef), N.ptr(mean), N.stream_ptr(dev))
    return (out, coef, mean) if want_mean else (out, coef)


def jb_ds(s: Tensor, coef: Tensor, g: Tensor, batch: Optional[Tensor] = None) -> Tensor:
    """dS = g_b coef[b,k] S of :func:`jb_terms` in one elementwise launch, into a fresh tensor of S's shape.  ``g`` [B]
    upstream gradients (an expanded scalar, what a mean over the batch sends, is read as one value); the graph of a
    row is batch[r] (un-padded ``s`` [Ntot,K]; None: one graph) or its first index (padded [B,N,K])."""
    dev = N.require_device(s, coef, g, batch)
    s, coef = N.f32c(s), N.f32c(coef)
    B, Kc = coef.shape
    g, bcast = _bcast_or_dense(g, (B,))
    if s.dim() == 3:
        rows, per, b = s.size(0) * s.size(1), max(s.size(1), 1), None
    else:
        rows, per, b = s.size(0), max(s.size(0), 1), N.opt_i64(batch)
    out = torch.empty_like(s)
    _checked(N.lib().tgp_jb_ds_f32, N.ptr(s), N.ptr(coef), N.ptr(g), 1 if bcast else 0, rows, per, N.ptr(b), B, Kc,
             N.ptr(out), N.stream_ptr(dev))
    return out


def hosc_small_graph_nodes() -> int:
    """The largest graph (and cluster count) the one-launch HOSC forward takes (A[b] and two [N,K] buffers in LDS)."""
    return int(N.lib().tgp_hosc_small_graph_nodes())


def hosc_matvec(adj: Tensor, v: Optional[Tensor], graph_sizes: Optional[Tensor] = None) -> Tensor:
    """y [B,N] = adj [B,N,N] @ v [B,N] (``v`` None: ones), 0 on the rows beyond ``graph_sizes``: one streaming pass over
    adj; three of them give the motif degrees d3 = A (A (A 1)) without A A A (utils/losses.py:218-316)."""
    dev = N.require_device(adj, v)
    a = N.f32c(adj)
    if a.dim() != 3 or a.size(1) != a.size(2):
        raise ValueError(f"hosc_matvec: adj {tuple(adj.shape)} is not [B,N,N]")
    B, Nn = a.size(0), a.size(1)
    if v is not None:
        v = N.f32c(v)
        if tuple(v.shape) != (B, Nn):
            raise ValueError(f"hosc_matvec: v {tuple(v.shape)} does not match adj {tuple(adj.shape)}")
    y = torch.empty(B, Nn, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_hosc_matvec_f32, N.ptr(a), N.ptr(v), B, Nn, N.ptr(_sizes_arg(graph_sizes, B, dev)), N.ptr(y),
             N.stream_ptr(dev))
    return y


def _hosc_rows(t: Optional[Tensor], rows: int, width: int):
    """(float32 tensor, row stride in elements) of an optional operand of ``rows`` x ``width`` values: contiguous, or a
    column block of a wider row-major buffer (2-D with unit column stride; 1-D with any stride when ``width`` is 1)."""
    if t is None:
        return None, 0
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    if t.numel() != rows * width:
        raise ValueError(f"operand {tuple(t.shape)} does not hold {rows} x {width} values")
    if t.is_contiguous():
        return t, width
    if t.dim() == 1 and width == 1:
        return t, t.stride(0)
    if t.dim() == 2 and t.stride(1) == 1:
        return t, t.stride(0)
    return t.contiguous(), width


def _hosc_ld(pairs, what: str) -> int:
    lds = {ld for t, ld in pairs if t is not None}
    if len(lds) > 1:
        raise ValueError(f"{what}: operands of one kind must share their row stride")
    return lds.pop() if lds else 0


def hosc_node_terms(s: Tensor, z: Optional[Tensor], z1: Optional[Tensor], d3: Optional[Tensor], d1: Optional[Tensor],
                    mask: Optional[Tensor] = None, graph_sizes: Optional[Tensor] = None, ptr: Optional[Tensor] = None,
                    max_nodes: Optional[int] = None) -> Tensor:
    """part [B,nsplit,record]: per block of 64 rows of a graph the column square sums of S, num = sum S (.) Z,
    den3 = sum d3_i |S_i|^2, num1 = sum S (.) Z1, den1 = sum d1_i |S_i|^2 and the node count, in one pass.  Padded batch
    (s [B,N,K], ``mask`` / ``graph_sizes``) or un-padded (s [Ntot,K] with ``ptr`` [B+1] and ``max_nodes``); z / z1 and
    d3 / d1 may be column blocks of wider buffers (e.g. the K+1 columns of a CSR product on [S | 1])."""
    dev = N.require_device(s, z, z1, d3, d1, mask, ptr)
    s = N.f32c(s)
    if ptr is None:
        B, Nn, Kc = s.shape
        rows, nsplit = B * Nn, max(1, -(-Nn // _PART_ROWS))
        p = None
    else:
        p = N.i64c(ptr)
        B, Nn, Kc = p.numel() - 1, 0, s.size(1)
        rows, nsplit = s.size(0), max(1, -(-int(max_nodes) // _PART_ROWS))
    zs = [_hosc_rows(t, rows, Kc) for t in (z, z1)]
    ds_ = [_hosc_rows(t, rows, 1) for t in (d3, d1)]
    L = N.lib()
    part = torch.empty(B, nsplit, int(L.tgp_hosc_record_floats(Kc)), dtype=torch.float32, device=dev)
    _checked(L.tgp_hosc_node_terms_f32, N.ptr(s), N.ptr(zs[0][0]), N.ptr(zs[1][0]), _hosc_ld(zs, "hosc_node_terms"),
             N.ptr(ds_[0][0]), N.ptr(ds_[1][0]), _hosc_ld(ds_, "hosc_node_terms"), B, Nn, Kc,
             N.ptr(_sizes_arg(graph_sizes, B, dev) if ptr is None else None),
             N.ptr(_mask_bytes(mask, B, Nn) if ptr is None else None), N.ptr(p), nsplit, N.ptr(part), N.stream_ptr(dev))
    return part


def hosc_is_small(Nn: int, Kc: int) -> bool:
    """Does a padded batch of ``Nn`` nodes per graph and ``Kc`` clusters take the one-launch forward (:func:`hosc_small`)?"""
    return bool(1 <= Nn <= hosc_small_graph_nodes() and 1 <= Kc <= hosc_small_graph_nodes())


def hosc_small(adj: Tensor, s: Tensor, mask: Optional[Tensor] = None, graph_sizes: Optional[Tensor] = None):
    """(z [B,N,K], d1 [B,N], d3 [B,N], part [B,1,record]) of a padded batch of small graphs (N, K <= 64) in ONE launch:
    what three :func:`hosc_matvec`, three products and :func:`hosc_node_terms` give on the general route."""
    dev = N.require_device(adj, s, mask)
    a, s = N.f32c(adj), N.f32c(s)
    B, Nn, Kc = s.shape
    if a.shape != (B, Nn, Nn):
        raise ValueError(f"adj {tuple(adj.shape)} does not match s {tuple(s.shape)}")
    L = N.lib()
    z = torch.empty(B, Nn, Kc, dtype=torch.float32, device=dev)
    d = torch.empty(2, B, Nn, dtype=torch.float32, device=dev)
    part = torch.empty(B, 1, int(L.tgp_hosc_record_floats(Kc)), dtype=torch.float32, device=dev)
    _checked(L.tgp_hosc_small_f32, N.ptr(a), N.ptr(s), B, Nn, Kc, N.ptr(_sizes_arg(graph_sizes, B, dev)),
             N.ptr(_mask_bytes(mask, B, Nn)), N.ptr(z), N.ptr(d[0]), N.ptr(d[1]), N.ptr(part), N.stream_ptr(dev))
    return z, d[0], d[1], part


def hosc_loss_terms(part: Tensor, Kc: int, raw: Optional[Tensor], gram: Optional[Tensor], alpha: float, mu: float,
                    inv_k: float, hosc_ortho: bool):
    """(out [2,B], cn [B,K], stats [B,6]): HOSC's per-graph terms ((1 - alpha) cut + alpha ho_cut) * inv_k and mu * ortho
    in one launch from the partial records; trace(S^T A S) from the diagonal of ``raw``, else from the records' num1;
    ``gram`` given: MinCut's orthogonality term, else (``hosc_ortho``) the column-norm form."""
    dev = N.require_device(part, raw, gram)
    part = N.f32c(part)
    B, nsplit = part.size(0), part.size(1)
    raw = N.opt_f32(raw)
    gram = N.opt_f32(gram)
    for t in (raw, gram):
        if t is not None and tuple(t.shape) != (B, Kc, Kc):
            raise ValueError(f"hosc_loss_terms: operand {tuple(t.shape)}, expected {(B, Kc, Kc)}")
    if part.size(2) != int(N.lib().tgp_hosc_record_floats(Kc)):
        raise ValueError("hosc_loss_terms: part does not hold records of K clusters")
    out = torch.empty(2, B, dtype=torch.float32, device=dev)
    cn = torch.empty(B, Kc, dtype=torch.float32, device=dev)
    stats = torch.empty(B, 6, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_hosc_loss_terms_f32, N.ptr(part), nsplit, N.ptr(raw), N.ptr(gram), B, Kc, float(alpha),
             float(mu), float(inv_k), 1 if hosc_ortho else 0, losses_eps(), N.ptr(out), N.ptr(cn), N.ptr(stats),
             N.stream_ptr(dev))
    return out, cn, stats


def hosc_loss_terms_bwd(g_terms: Tensor, stats: Tensor, gram: Optional[Tensor], Kc: int, alpha: float, mu: float,
                        inv_k: float, hosc_ortho: bool, want_raw: bool):
    """(g_raw [B,K,K] or None, coef [B,5], W [B,K,K] or None): the gradients of :func:`hosc_loss_terms` from the upstream
    gradients [2,B], one launch (see tgp_hosc_loss_terms_bwd_f32)."""
    dev = N.require_device(g_terms, stats, gram)
    g_terms, stats = N.f32c(g_terms), N.f32c(stats)
    gram = N.opt_f32(gram)
    B = stats.size(0)
    g_raw = torch.empty(B, Kc, Kc, dtype=torch.float32, device=dev) if want_raw else None
    W = torch.empty(B, Kc, Kc, dtype=torch.float32, device=dev) if gram is not None else None
    coef = torch.empty(B, 5, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_hosc_loss_terms_bwd_f32, N.ptr(g_terms), N.ptr(stats), N.ptr(gram), B, Kc, float(alpha),
             float(mu), float(inv_k), 1 if hosc_ortho else 0, N.ptr(g_raw), N.ptr(coef), N.ptr(W), N.stream_ptr(dev))
    return g_raw, coef, W


def hosc_ds(s: Tensor, z: Optional[Tensor], zt: Optional[Tensor], z1: Optional[Tensor], z1t: Optional[Tensor],
            d3: Optional[Tensor], d1: Optional[Tensor], cn: Optional[Tensor], coef: Tensor, nodes_per_graph: int,
            batch: Optional[Tensor], out: Tensor, accumulate: bool) -> Tensor:
    """out (+)= c_num (Z + Zt) + 2 c_den d3 S + c_ortho S / cn + 2 c_den1 d1 S + c_num1 (Z1 + Z1t) over the rows of S: the
    elementwise part of HOSC's dS, one launch.  ``zt`` / ``z1t`` None: A = A^T, the forward's product counts twice.
    Graph of a row: batch[r] (un-padded) or r // nodes_per_graph."""
    dev = N.require_device(s, z, zt, z1, z1t, d3, d1, cn, coef, batch, out)
    s = N.f32c(s)
    Kc = s.size(-1)
    rows = s.numel() // Kc
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != rows * Kc:
        raise ValueError("hosc_ds: out must be a contiguous float32 tensor of rows x K values")
    zs = [_hosc_rows(t, rows, Kc) for t in (z, z1)]
    zts = [_hosc_rows(t, rows, Kc) for t in (zt, z1t)]
    ds_ = [_hosc_rows(t, rows, 1) for t in (d3, d1)]
    b = N.opt_i64(batch)
    c = N.opt_f32(cn)
    coef = N.f32c(coef)
    _checked(N.lib().tgp_hosc_ds_f32, N.ptr(s), N.ptr(zs[0][0]), N.ptr(zts[0][0]), N.ptr(zs[1][0]), N.ptr(zts[1][0]),
             _hosc_ld(zs, "hosc_ds"), _hosc_ld(zts, "hosc_ds"), N.ptr(ds_[0][0]), N.ptr(ds_[1][0]),
             _hosc_ld(ds_, "hosc_ds"), N.ptr(c), N.ptr(coef), rows, int(nodes_per_graph), N.ptr(b), coef.size(0), Kc,
             1 if accumulate else 0, out.data_ptr(), N.stream_ptr(dev))
    return out


def bnpool_max_clusters() -> int:
    """The largest K the BN-Pool reconstruction kernels take (S's fragment sits in registers, a 32-row tile in LDS)."""
    return int(N.lib().tgp_bnpool_max_clusters())


def _bnpool_operands(t: Tensor, s: Tensor, adj: Tensor, mask: Optional[Tensor], what: str):
    dev = N.require_device(t, s, adj, mask)
    t, s, a = N.f32c(t), N.f32c(s), N.f32c(adj)
    if s.dim() != 3 or t.shape != s.shape or a.shape != (s.size(0), s.size(1), s.size(1)):
        raise ValueError(f"{what}: T {tuple(t.shape)}, S {tuple(s.shape)}, adj {tuple(adj.shape)} are not "
                         "[B,N,K], [B,N,K], [B,N,N]")
    m = None
    if mask is not None:
        if mask.shape != s.shape[:2]:
            raise ValueError(f"{what}: mask {tuple(mask.shape)} does not match S {tuple(s.shape)}")
        m = (mask if mask.dtype == torch.bool else mask != 0).contiguous()
    return dev, t, s, a, m


def bnpool_rec_fwd(t: Tensor, s: Tensor, adj: Tensor, mask: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(rec [B], stats [B,2] = (c | n^2)): BN-Pool's per-graph class-balanced BCE between the logits T S^T (T = S K) and
    ``adj``, divided by n^2 (utils/losses.py:1268-1356 as poolers/bnpool.py:400-416 calls it).  One launch over the
    32x32 logit tiles (exact-fp32 MFMA) that reads ``adj`` once, one tail launch; the logits are never written."""
    dev, t, s, a, m = _bnpool_operands(t, s, adj, mask, "bnpool_rec_fwd")
    B, Nn, Kc = s.shape
    rec = torch.empty(B, dtype=torch.float32, device=dev)
    stats = torch.empty(B, 2, dtype=torch.float32, device=dev)
    if B == 0:
        return rec, stats
    nfl = int(N.lib().tgp_bnpool_part_floats(B, Nn))
    part = torch.empty(max(nfl, 1), dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_bnpool_rec_fwd_f32, N.ptr(t), N.ptr(s), N.ptr(a), N.ptr(m), B, Nn, Kc, N.ptr(part),
             part.numel(), N.ptr(rec), N.ptr(stats), N.stream_ptr(dev))
    return rec, stats


def bnpool_rec_bwd(t: Tensor, s: Tensor, adj: Tensor, mask: Optional[Tensor], g: Tensor,
                   stats: Tensor) -> Tuple[Tensor, Tensor]:
    """(P, Q) = (G S, G^T T), both [B,N,K], for G = d sum_b g_b rec_b / d logits: two launches that recompute the logit
    tiles and keep G on chip (no float atomics)."""
    dev, t, s, a, m = _bnpool_operands(t, s, adj, mask, "bnpool_rec_bwd")
    N.require_device(g, stats)
    B, Nn, Kc = s.shape
    g, stats = N.f32c(g), N.f32c(stats)
    if g.numel() != B or stats.shape != (B, 2):
        raise ValueError(f"bnpool_rec_bwd: g {tuple(g.shape)} / stats {tuple(stats.shape)} do not match B = {B}")
    p = torch.empty(B, Nn, Kc, dtype=torch.float32, device=dev)
    q = torch.empty(B, Nn, Kc, dtype=torch.float32, device=dev)
    if B > 0:
        _checked(N.lib().tgp_bnpool_rec_bwd_f32, N.ptr(t), N.ptr(s), N.ptr(a), N.ptr(m), N.ptr(g), N.ptr(stats), B, Nn,
                 Kc, N.ptr(p), N.ptr(q), N.stream_ptr(dev))
    return p, q


_ACC_TV_ROWS = 16  # rows of the adjacency per workgroup of the dense total-variation pass (csrc/asym_cheeger.hip)
ACC_ROUTES = ("auto", "count", "radix")


def acc_small_graph_nodes() -> int:
    """The largest graph the counting quantile select takes (its columns sit in LDS); larger ones take the radix select."""
    return int(N.lib().tgp_acc_small_graph_nodes())


def acc_tv_dense(adj: Tensor, s: Tensor, graph_sizes: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(part [B,ceil(N/16)] float32, cnt [B,ceil(N/16)] int32): per block of 16 rows of a padded batch the sum of
    a_ij ||s_i - s_j||_1 over its nonzero entries, and their number (utils/losses.py:780-862).  One pass over ``adj``;
    64-column chunks without a nonzero cost nothing more than their load."""
    dev = N.require_device(adj, s)
    a, s = N.f32c(adj), N.f32c(s)
    if s.dim() != 3 or a.shape != (s.size(0), s.size(1), s.size(1)):
        raise ValueError(f"adj {tuple(adj.shape)} does not match s {tuple(s.shape)}")
    B, Nn, Kc = s.shape
    nrb = max(1, -(-Nn // _ACC_TV_ROWS))
    part = torch.empty(B, nrb, dtype=torch.float32, device=dev)
    cnt = torch.empty(B, nrb, dtype=torch.int32, device=dev)
    _checked(N.lib().tgp_acc_tv_dense_f32, N.ptr(a), N.ptr(s), B, Nn, Kc, N.ptr(_sizes_arg(graph_sizes, B, dev)), nrb,
             N.ptr(part), N.ptr(cnt), N.stream_ptr(dev))
    return part, cnt


def acc_tv_dense_bwd(adj: Tensor, s: Tensor, graph_sizes: Optional[Tensor], g_tv: Tensor, ecnt: Tensor,
                     c_tv: float) -> Tensor:
    """dS [B,N,K] of the dense total variation: g_b c_tv / (2 E_b) sum_j (a_ij + a_ji) sign(s_i - s_j), every row
    written; row i and column i of ``adj`` are both read (the column through a transposed LDS tile)."""
    dev = N.require_device(adj, s, g_tv, ecnt)
    a, s = N.f32c(adj), N.f32c(s)
    B, Nn, Kc = s.shape
    ds = torch.empty(B, Nn, Kc, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_acc_tv_dense_bwd_f32, N.ptr(a), N.ptr(s), B, Nn, Kc, N.ptr(_sizes_arg(graph_sizes, B, dev)),
             N.ptr(N.f32c(g_tv)), N.ptr(ecnt), float(c_tv), N.ptr(ds), N.stream_ptr(dev))
    return ds


def edge_group(edge_index: Tensor, num_nodes: int, by_destination: bool = False) -> AssignIndex:
    """The edge positions grouped by source or by destination, edge-list order inside a group: the summation order of
    every float sum that runs over a node's edges (the edge-form total variation and its backward, the k-MIS degrees and
    "w-greedy" scores, the edge-contraction softmax, LaPool's by-source sums)."""
    row, col = _edge_rows(edge_index)
    return build_assign_index(col if by_destination else row, num_nodes)


def acc_tv_edge(s: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor], by_src: AssignIndex) -> Tensor:
    """node_tv [N]: per node the sum over its out-edges of w_e ||s_i - s_dst||_1 (utils/losses.py:865-917), one wave per
    node, added in edge-list order."""
    dev = N.require_device(s, edge_index, edge_weight)
    s = N.f32c(s)
    _, col = _edge_rows(edge_index)
    w = N.opt_f32_flat(edge_weight)
    n, Kc, E = s.size(0), s.size(1), col.numel()
    if w is not None and w.numel() != E:
        raise ValueError("acc_tv_edge: one weight per edge")
    out = torch.empty(n, dtype=torch.float32, device=dev)
    src_ptr, src_perm, col_p = by_src.walk(col, E)
    _checked(N.lib().tgp_acc_tv_edge_f32, N.ptr(s), n, Kc, col_p, N.ptr(w), E, src_ptr, src_perm, N.ptr(out),
             N.stream_ptr(dev))
    return out


def acc_tv_edge_bwd(s: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor], by_src: AssignIndex,
                    by_dst: AssignIndex, batch: Optional[Tensor], g_tv: Tensor, ecnt: Tensor, c_tv: float) -> Tensor:
    """dS [N,K] of the edge-form total variation: every node adds over its out-edges and its in-edges (no scatter)."""
    dev = N.require_device(s, edge_index, edge_weight, batch, g_tv, ecnt)
    s = N.f32c(s)
    row, col = _edge_rows(edge_index)
    w = N.opt_f32_flat(edge_weight)
    n, Kc, E = s.size(0), s.size(1), col.numel()
    ds = torch.empty(n, Kc, dtype=torch.float32, device=dev)
    b = N.opt_i64(batch)
    src_ptr, src_perm, col_p = by_src.walk(col, E)  # (out-edges: the far end is the destination; in-edges: the source)
    dst_ptr, dst_perm, row_p = by_dst.walk(row, E)
    _checked(N.lib().tgp_acc_tv_edge_bwd_f32, N.ptr(s), n, Kc, row_p, col_p, N.ptr(w), E, src_ptr, src_perm, dst_ptr,
             dst_perm, N.ptr(b), N.ptr(N.f32c(g_tv)), N.ptr(ecnt), float(c_tv), ecnt.numel(), N.ptr(ds),
             N.stream_ptr(dev))
    return ds


def acc_quantile(s: Tensor, k: int, mask: Optional[Tensor] = None, graph_sizes: Optional[Tensor] = None,
                 ptr: Optional[Tensor] = None, max_nodes: Optional[int] = None, route: str = "auto"):
    """(q [B,K], qnode [B,K] int32, colsum [B,K], cge [B,K] int32, nreal [B] int32, route taken): per graph and column
    of ``s`` the entry a descending sort has at position min(floor(n / k), n - 1) among the graph's n real rows -- exact,
    without sorting -- the LOWEST row (relative to the graph's first) that holds it, the asymmetric-norm sum
    sum_i rho(s_ik - q_k) and the number of rows with s_ik >= q_k (utils/losses.py:503-550, 920-1010).  Padded layout:
    s [B,N,K] with ``mask`` / ``graph_sizes``; un-padded: s [Ntot,K] with node offsets ``ptr`` [B+1] and ``max_nodes``.
    ``route``: "count" (graphs of at most :func:`acc_small_graph_nodes` rows, ranked by counting in LDS), "radix"
    (8-bit radix select) or "auto"."""
    dev = N.require_device(s, mask, graph_sizes, ptr)
    s = N.f32c(s)
    if ptr is None:
        if s.dim() != 3:
            raise ValueError("acc_quantile: the padded layout takes s [B,N,K]")
        B, Nn, Kc = s.shape
        mx, p = Nn, None
        m, gs = _mask_bytes(mask, B, Nn), _sizes_arg(graph_sizes, B, dev)
    else:
        if s.dim() != 2 or mask is not None or graph_sizes is not None or max_nodes is None:
            raise ValueError("acc_quantile: the un-padded layout takes s [Ntot,K], ptr and max_nodes")
        p = N.i64c(ptr)
        B, Nn, Kc, mx, m, gs = p.numel() - 1, 0, s.size(1), int(max_nodes), None, None
    code = ACC_ROUTES.index(route)
    taken = "count" if code == 1 or (code == 0 and mx <= acc_small_graph_nodes()) else "radix"
    q = torch.empty(B, Kc, dtype=torch.float32, device=dev)
    colsum = torch.empty(B, Kc, dtype=torch.float32, device=dev)
    qnode = torch.empty(B, Kc, dtype=torch.int32, device=dev)
    cge = torch.empty(B, Kc, dtype=torch.int32, device=dev)
    nreal = torch.empty(B, dtype=torch.int32, device=dev)
    _checked(N.lib().tgp_acc_quantile_f32, N.ptr(s), B, Nn, Kc, N.ptr(gs), N.ptr(m), N.ptr(p), mx, int(k), code,
             N.ptr(q), N.ptr(qnode), N.ptr(colsum), N.ptr(cge), N.ptr(nreal), N.stream_ptr(dev))
    return q, qnode, colsum, cge, nreal, taken


def acc_tail(B: int, Kc: int, k: int, dev, tv=None, colsum: Optional[Tensor] = None,
                   nreal: Optional[Tensor] = None, coeffs=(1.0, 1.0)) -> Tuple[Tensor, Tensor]:
    """(out [2,B], ecnt [B] int32): the per-graph total-variation and balance terms times ``coeffs`` in one launch, the
    partial sums added in a fixed order.  ``tv``: None, ("dense", part, cnt) of :func:`acc_tv_dense` or
    ("edge", node_tv, by_src, ptr) of :func:`acc_tv_edge`; ``colsum`` / ``nreal`` of :func:`acc_quantile` or None."""
    out = torch.empty(2, B, dtype=torch.float32, device=dev)
    ecnt = torch.empty(B, dtype=torch.int32, device=dev)
    vals = cnt = src_ptr = ptr = None
    nrb = 0
    if tv is not None and tv[0] == "dense":
        vals, cnt = tv[1], tv[2]
        nrb = vals.size(1)
    elif tv is not None:
        vals, src_ptr, ptr = tv[1], tv[2].row_ptr, N.i64c(tv[3])
    _checked(N.lib().tgp_acc_loss_terms_f32, N.ptr(vals), N.ptr(cnt), N.ptr(src_ptr), N.ptr(ptr), nrb, N.ptr(colsum),
             N.ptr(nreal), B, Kc, int(k), float(coeffs[0]), float(coeffs[1]), N.ptr(out), N.ptr(ecnt),
             N.stream_ptr(dev))
    return out, ecnt


def acc_asym_bwd(s: Tensor, k: int, q: Tensor, qnode: Tensor, cge: Tensor, nreal: Tensor, g_bal: Tensor, c_bal: float,
                 out: Tensor, accumulate: bool, mask: Optional[Tensor] = None, graph_sizes: Optional[Tensor] = None,
                 ptr: Optional[Tensor] = None, batch: Optional[Tensor] = None) -> Tensor:
    """out (+)= dS of the balance term: one elementwise pass, the column's total added on the quantile node."""
    dev = N.require_device(s, q, qnode, cge, nreal, g_bal, out, mask, graph_sizes, ptr, batch)
    s = N.f32c(s)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.shape != s.shape:
        raise ValueError("acc_asym_bwd: out must be a contiguous float32 tensor shaped like s")
    B, Kc = q.shape
    if ptr is None:
        rows, Nn = s.size(0) * s.size(1), s.size(1)
        m, gs, p, b = _mask_bytes(mask, B, Nn), _sizes_arg(graph_sizes, B, dev), None, None
    else:
        rows, Nn, m, gs, p = s.size(0), 0, None, None, N.i64c(ptr)
        b = N.opt_i64(batch)
    _checked(N.lib().tgp_acc_asym_bwd_f32, N.ptr(s), rows, Nn, Kc, N.ptr(b), N.ptr(p), N.ptr(gs), N.ptr(m), N.ptr(q),
             N.ptr(qnode), N.ptr(cge), N.ptr(nreal), N.ptr(N.f32c(g_bal)), float(c_bal), int(k), B,
             1 if accumulate else 0, out.data_ptr(), N.stream_ptr(dev))
    return out


def topk_minscore(score: Tensor, ptr: Tensor, min_score: float, tol: float = 1e-7) -> Tuple[Tensor, Tensor]:
    """(prob [N], node_index [k]): per-graph softmax of ``score`` and the nodes above the min_score threshold, ascending
    (select/topk_select.py:186-194 with PyG's softmax / topk); ``ptr`` = node offsets of the sorted batch."""
    dev = N.require_device(score, ptr)
    score, ptr = N.f32c(score.reshape(-1)), N.i64c(ptr)
    n, B = score.numel(), ptr.numel() - 1
    prob = torch.empty(n, dtype=torch.float32, device=dev)
    L = N.lib()
    st = N.stream_ptr(dev)
    node_index, _ = _count_fill(
        dev, L.tgp_topk_minscore_workspace_bytes(n, B),
        lambda ws, ws_bytes, cnt: _checked(L.tgp_topk_minscore_count, N.ptr(score), N.ptr(ptr), n, B, float(min_score),
                                           float(tol), N.ptr(prob), ws, ws_bytes, cnt, st),
        lambda ws, k, out, _: _checked(L.tgp_topk_minscore_fill, ws, N.ptr(ptr), n, B, k, out, st), rows=1)
    return prob, node_index[0]


def topk_plan(sizes: Tensor, ratio: float) -> Tuple[Tensor, Tensor]:
    """(k [B], koff [B+1]): nodes kept per graph (PyG topk: ceil(ratio * n) in fp32, or min(ratio, n)) and their
    exclusive prefix sums, in one launch."""
    dev = N.require_device(sizes)
    sizes = N.i64c(sizes)
    B = sizes.numel()
    k = torch.empty(B, dtype=torch.int64, device=dev)
    koff = torch.empty(B + 1, dtype=torch.int64, device=dev)
    _checked(N.lib().tgp_topk_plan, N.ptr(sizes), B, float(ratio), N.ptr(k), N.ptr(koff), N.stream_ptr(dev))
    return k, koff


def topk_select(score: Tensor, batch: Optional[Tensor], num_graphs: int, ptr: Tensor, k: Tensor, koff: Tensor,
                k_total: int, segments_max_nodes: int = 0, with_values: bool = False, with_lift: bool = False):
    """Per-graph top-k (select/topk_select.py:194 -> PyG ``topk``) fused with the row sort of SelectOutput
    (select/base_select.py:58): (index [2, k_total] = node_index ascending over cluster_index, supernode -> assignment
    index[, values = score[node_index] when ``with_values``: no gradient][, the node -> assignment index when
    ``with_lift``: what Reduce's backward and Lift walk, from the same compaction])."""
    dev = N.require_device(score, batch, ptr, k, koff)
    score = N.f32c(score.reshape(-1))
    n = score.numel()
    kk = max(k_total, 1)
    one = with_values and 32 * kk <= _SPS_ONE_ALLOC_BYTES  # (index 16 B + values 4 + perm 4 + pack 8 per kept node)
    if one:
        # the selector's outputs of a batch of small graphs are a few hundred KB: ONE allocation, typed views behind the
        # launch (every torch.empty in front of a ~5 us kernel is ~1.2 us of idle GPU)
        o_val = (16 * k_total + 15) & ~15
        o_perm = (o_val + 4 * k_total + 15) & ~15
        o_pack = (o_perm + 4 * kk + 15) & ~15
        buf = torch.empty((o_pack + 8 * kk + 15) & ~15, dtype=torch.uint8, device=dev)
        base = buf.data_ptr()
        idx_p, val_p, perm_p, pack_p = base, base + o_val, base + o_perm, base + o_pack
    else:
        index = torch.empty(2, k_total, dtype=torch.int64, device=dev)  # the indices of the sparse S, written in place
        values = torch.empty(k_total, dtype=torch.float32, device=dev) if with_values else None
        perm = torch.empty(kk, dtype=torch.int32, device=dev)
        # the packed one-to-one index {node, score} the sparse Reduce streams (when the scores ARE the weights of S)
        pack = torch.empty(kk, dtype=torch.int64, device=dev) if with_values else None
        idx_p, val_p, perm_p, pack_p = index.data_ptr(), N.ptr(values), perm.data_ptr(), N.ptr(pack)
    lift_ptr = torch.empty(n + 1, dtype=torch.int32, device=dev) if with_lift and n > 0 else None
    with_lift = lift_ptr is not None
    L = N.lib()
    ws = N.workspace(L.tgp_topk_select_workspace_bytes(n), dev)
    # r5: graphs beyond the per-graph sort routes (the device-wide route) also get the kept-node bitmap and its rank
    # directory from the compaction pass -- what the subgraph Connect of this very selection starts from
    directory = None
    wrote = ctypes.c_int(0)
    if n > 0 and k_total > 0 and not (0 < segments_max_nodes <= 8192):
        nblk = int(L.tgp_topk_select_directory_blocks(n))
        directory = torch.empty(5 * nblk, dtype=torch.int32, device=dev)  # [4 nblk] bitmap words | [nblk] rank128
    _checked(L.tgp_topk_select, N.ptr(score), N.ptr(N.opt_i64(batch)), n, num_graphs, N.ptr(N.i64c(ptr)),
             N.ptr(N.i64c(k)), N.ptr(N.i64c(koff)), segments_max_nodes, N.ptr(ws), ws.numel(), idx_p,
             idx_p + 8 * k_total, perm_p, val_p, N.ptr(lift_ptr), pack_p,
             None if directory is None else directory.data_ptr(),
             None if directory is None else directory.data_ptr() + 16 * nblk,
             ctypes.addressof(wrote) if directory is not None else None, N.stream_ptr(dev))
    if not wrote.value:
        directory = None
    if one:
        i64, i32, f32 = buf.view(torch.int64), buf.view(torch.int32), buf.view(torch.float32)
        index = torch.as_strided(i64, (2, k_total), (k_total, 1), 0)
        values = torch.as_strided(f32, (k_total,), (1,), o_val >> 2)
        perm = torch.as_strided(i32, (kk,), (1,), o_perm >> 2)
        pack = torch.as_strided(i64, (kk,), (1,), o_pack >> 3)
    assign = AssignIndex(None, perm, k_total, k_total)
    assign.member_directory = directory  # (bitmap | rank128) of the kept nodes, or None
    assign.member_directory_key = (index.data_ptr(), k_total) if directory is not None else None
    if pack is not None and k_total > 0 and n < (1 << 31):
        assign.pack, assign.pack_key = pack, (index.data_ptr(), values.data_ptr())
    out = (index, assign) + ((values,) if with_values else ())
    return out + ((AssignIndex(lift_ptr, None, k_total, n),) if with_lift else ())


_HUB_LISTS = TensorMemo(16)  # edge lists on which the row-local coalesce met a supernode row beyond its LDS sort
_SORTED_ROWS = TensorMemo(16)  # edge_index -> are its rows ascending?  (None: it has not been looked at)
_rows_sorted_memo = _SORTED_ROWS.get
_remember_rows_sorted = _SORTED_ROWS.put


def _rows_sorted(edge_index: Tensor, row: Tensor) -> bool:
    """Is the list grouped by ascending source node?  Remembered per tensor object, so an unchanged edge_index costs one
    host round trip in total, not one per call."""
    flag = _rows_sorted_memo(edge_index)
    if flag is None:
        flag = bool((row[1:] >= row[:-1]).all())
        _remember_rows_sorted(edge_index, flag)
    return flag


def graclus_match(edge_index: Tensor, edge_weight: Optional[Tensor], num_nodes: int,
                  max_rounds: Optional[int] = None, return_row_ptr: bool = False,
                  graph_ptr: Optional[Tensor] = None, max_graph_nodes: Optional[int] = None,
                  relabel: bool = False):
    """label[i] = min(i, partner) of a heavy-edge maximal matching (select/graclus_select.py:66 ->
    torch_cluster.graclus_cluster): handshake rounds on the device until a round matches nothing, however many that
    takes (a path with monotone weights matches one pair per round: n/2 rounds; torch_cluster iterates until done
    too).  ``max_rounds`` bounds the loop for callers that accept a non-maximal matching; if it is hit a
    RuntimeWarning says so.  ``return_row_ptr``: also return the int32 CSR offsets [num_nodes + 1] of the list when
    it is row-sorted (else None) -- the matcher builds them anyway and SparseConnect can reuse them.
    ``graph_ptr`` [B+1] / ``max_graph_nodes``: node offsets of the graphs of a sorted batch and its longest graph; when
    every graph fits one workgroup all rounds of all graphs run as ONE launch (same matching).
    ``relabel``: return ``(index [2, N], K, assign_index, ones [N])`` instead of the labels -- row 0 = 0..N-1, row 1 = the consecutive cluster id
    of every node (``torch.unique(label, return_inverse=True)[1]``, graclus_select.py:68) from two more launches, its
    count read back together with the matcher's status word."""
    dev = N.require_device(edge_index, edge_weight)
    row, col = _edge_rows(edge_index)
    E = row.numel()
    w = N.opt_f32_flat(edge_weight)
    L = N.lib()
    st = N.stream_ptr(dev)
    if (relabel and max_rounds is None and graph_ptr is not None and max_graph_nodes is not None and E > 0
            and num_nodes > 0 and graph_ptr.numel() >= 2 and max_graph_nodes <= 64 and _GRACLUS_FUSED
            and _rows_sorted_memo(edge_index) is not False and not torch.cuda.is_current_stream_capturing()):
        # r4: matching + relabelling + members index of a batch of small graphs in ONE launch, straight from the edge list
        # (no CSR); the kernel validates row order itself, so a list nobody has looked at yet needs no check pass
        gp = N.i64c(graph_ptr)
        B = gp.numel() - 1
        call = _sps_state(dev, st, L.tgp_graclus_match_graphs_fused_status_words(B)).open_call()
        # one allocation for the four outputs (a batch of small graphs: a few hundred KB); the typed views are made
        # behind the launch, while the kernel runs
        o_idx = 0
        o_ptr = (o_idx + 16 * num_nodes + 15) & ~15
        o_perm = (o_ptr + 4 * (num_nodes + 1) + 15) & ~15
        o_ones = (o_perm + 4 * num_nodes + 15) & ~15
        buf = torch.empty((o_ones + 4 * num_nodes + 15) & ~15, dtype=torch.uint8, device=dev)
        base = buf.data_ptr()
        # (a list pooled before brings its per-graph offsets along; a new one lets the kernel search: r5, no launch for them)
        eptr = _edge_ptr_memo(edge_index, graph_ptr) if _SPS_GIVE_PTRS else None
        _checked(L.tgp_graclus_match_graphs_fused, N.ptr(row), N.ptr(col), N.ptr(w), num_nodes, E, N.ptr(gp), B,
                 N.ptr(eptr), None, base + o_idx, base + o_ptr, base + o_perm, base + o_ones, *call.lookback, st)
        i64, i32, f32 = buf.view(torch.int64), buf.view(torch.int32), buf.view(torch.float32)
        index = torch.as_strided(i64, (2, num_nodes), (num_nodes, 1), o_idx >> 3)
        a_ptr = torch.as_strided(i32, (num_nodes + 1,), (1,), o_ptr >> 2)
        a_perm = torch.as_strided(i32, (num_nodes,), (1,), o_perm >> 2)
        ones = torch.as_strided(f32, (num_nodes,), (1,), o_ones >> 2)
        k = call.total()
        if k is not None:
            if E > 1 and _rows_sorted_memo(edge_index) is None:
                _remember_rows_sorted(edge_index, True)  # (the kernel refuses lists whose rows are not ascending)
            out = (index, k, AssignIndex(a_ptr[:k + 1], a_perm, num_nodes, k), ones)
            return (out, None) if return_row_ptr else out
        del index, a_ptr, a_perm, ones  # refused: the staged route below decides why
    label = torch.empty(num_nodes, dtype=torch.int64, device=dev)
    sorted_ptr = None
    # PyG lists are sorted by source: one comparison pass + round trip decides whether the CSR needs a sort at all
    # (remembered per edge_index object: full-batch training pools the same graph every epoch)
    words = torch.empty(4, dtype=torch.int32, device=dev)  # [status, rows-not-sorted flag, K (int64)]
    per_graph = (max_rounds is None and graph_ptr is not None and max_graph_nodes is not None and E > 0
                 and num_nodes > 0 and max_graph_nodes <= L.tgp_graclus_match_max_graph_nodes()
                 and graph_ptr.numel() >= 2)
    # a list nobody has looked at yet, on the one-launch route: go on as if it were sorted, the check rides on the
    # offsets kernel and its flag is read with the status word (no round trip of its own)
    optimistic = per_graph and E > 1 and _rows_sorted_memo(edge_index) is None
    if optimistic or (E > 1 and _rows_sorted(edge_index, row)):
        row_ptr, perm = torch.empty(num_nodes + 1, dtype=torch.int32, device=dev), None
        if optimistic:
            _checked(L.tgp_rowptr_from_sorted_flag_i64, N.ptr(row), E, num_nodes, N.ptr(row_ptr), N.ptr(words[1:]), st)
        else:
            _checked(L.tgp_rowptr_from_sorted_i64, N.ptr(row), E, num_nodes, N.ptr(row_ptr), st)
        sorted_ptr = row_ptr
    else:
        index = build_assign_index(row, num_nodes)
        row_ptr, perm = index.row_ptr, index.perm
    ws = N.workspace(L.tgp_graclus_match_workspace_bytes(num_nodes, E), dev)
    finished = num_nodes == 0 or E == 0

    pairs = {}

    def relabelled():
        index = torch.empty(2, num_nodes, dtype=torch.int64, device=dev)
        rws = N.workspace(L.tgp_graclus_relabel_workspace_bytes(num_nodes), dev)
        # the supernode -> members index comes out of the same kernels (a matching: a representative and at most one
        # partner per cluster), so Reduce / Connect do not build it from the ids
        pairs["row_ptr"] = torch.empty(num_nodes + 1, dtype=torch.int32, device=dev)
        pairs["perm"] = torch.empty(max(num_nodes, 1), dtype=torch.int32, device=dev)
        pairs["ones"] = torch.empty(num_nodes, dtype=torch.float32, device=dev)  # the values of S, same launch
        _checked(L.tgp_graclus_relabel_i64, N.ptr(label), num_nodes, N.ptr(rws), rws.numel(), N.ptr(index),
                 N.ptr(words[2:]), N.ptr(pairs["row_ptr"]), N.ptr(pairs["perm"]), N.ptr(pairs["ones"]), st)
        return index

    def finish(index=None, k=None):
        out = label
        if relabel:
            if index is None:
                index = relabelled()
                k = words.tolist()[2]
            k = int(k)
            out = (index, k, AssignIndex(pairs["row_ptr"][:k + 1], pairs["perm"], num_nodes, k), pairs["ones"])
        return (out, sorted_ptr) if return_row_ptr else out

    def start(init_state=1):
        _checked(L.tgp_graclus_match_start, N.ptr(row), N.ptr(col), N.ptr(w), N.ptr(row_ptr), N.ptr(perm), num_nodes, E,
                 N.ptr(ws), ws.numel(), N.ptr(label), init_state, st)
    start(0 if (per_graph and not finished) else 1)  # (the one-launch route sets the labels itself)
    if not finished and per_graph:
        gp = N.i64c(graph_ptr)
        _checked(L.tgp_graclus_match_graphs, N.ptr(row_ptr), num_nodes, E, N.ptr(ws), N.ptr(gp), gp.numel() - 1,
                 int(max_graph_nodes), N.ptr(label), N.ptr(words), st)
        index = relabelled() if relabel else None  # (optimistic: one round trip for the status word and the count)
        got = words.tolist()
        if optimistic:
            _remember_rows_sorted(edge_index, got[1] == 0)
            if got[1] != 0:  # not sorted after all: everything above walked meaningless offsets -- again, knowing it
                return graclus_match(edge_index, edge_weight, num_nodes, max_rounds, return_row_ptr, graph_ptr,
                                     max_graph_nodes, relabel)
        if got[0] == 0:
            return finish(index, got[2])
        start()  # an entry that leaves its graph (or a longer graph than declared): the device-wide rounds, from scratch
    done, step = 0, 6  # late rounds are cheap (free nodes are packed before scanning): prefer fewer round trips
    while not finished and (max_rounds is None or done < max_rounds):
        if max_rounds is not None:
            step = min(step, max_rounds - done)
        matched = torch.empty(step + 1, dtype=torch.int32, device=dev)  # [round flags ..., tail status]
        _checked(L.tgp_graclus_match_rounds, N.ptr(row_ptr), num_nodes, E, N.ptr(ws), step, N.ptr(matched),
                 N.ptr(label), st)
        done += step
        if max_rounds is None:
            # the few thousand nodes that are still free after these rounds: all their remaining rounds in one workgroup
            # (declines when there are more than that), read back with the round flags
            _checked(L.tgp_graclus_match_tail, N.ptr(row_ptr), num_nodes, E, N.ptr(ws), N.ptr(label),
                     N.ptr(matched[step:]), st)
            last, tail = matched[step - 1:].tolist()
            finished = last == 0 or tail == 1
        else:
            finished = int(matched[step - 1].item()) == 0  # one round trip per batch of rounds
        # random-like graphs finish in a handful of rounds; a long tail means chain-like structure: batch more
        # rounds per round trip (4, then doubling up to 256) so that n/2 rounds cost n/512 host synchronisations
        step = 4 if done <= 6 else min(2 * step, 256)
    if not finished:
        import warnings
        warnings.warn(f"graclus_match stopped after max_rounds={max_rounds} rounds: the matching is not maximal",
                      RuntimeWarning)
    return finish()


# ------------------------------------------- what the k-MIS and edge-contraction selectors share (csrc/graph_frame.h)
def _rank_of(count: int, perm: Optional[Tensor], what: str, dev) -> Tensor:
    """int32 [count]: the rank ``perm`` gives every item (first = 0); the list order for None."""
    if perm is None:
        return torch.arange(count, dtype=torch.int32, device=dev)
    if perm.numel() != count:
        raise ValueError(f"perm must have one entry per {what} ({count}), got {perm.numel()}")
    rank = torch.empty(count, dtype=torch.int32, device=dev)
    rank[perm.reshape(-1)] = torch.arange(count, dtype=torch.int32, device=dev)
    return rank


def _frame_route(limit: str, need_edges: bool, num_nodes: int, num_edges: int, graph_ptr: Optional[Tensor],
                 max_graph_nodes: Optional[int], route: Optional[str] = None) -> str:
    """"graphs" (one workgroup per graph) for a sorted batch whose longest graph fits the frame (``limit``: the getter of
    the selector's bound), "rounds" (device-wide launches) for everything else; ``route`` overrides, where it can."""
    fits = (graph_ptr is not None and max_graph_nodes is not None and graph_ptr.numel() >= 2 and num_nodes > 0
            and (num_edges > 0 or not need_edges) and 0 < max_graph_nodes <= getattr(N.lib(), limit)())
    if route is None:
        return "graphs" if fits else "rounds"
    if route not in ("graphs", "rounds"):
        raise ValueError(f"route must be 'graphs' or 'rounds', got {route!r}")
    if route == "graphs" and not fits:
        raise ValueError("the per-graph route needs a sorted batch whose longest graph fits one workgroup")
    return route


def _frame_done(status: int, name: str, route: Optional[str], what: str) -> bool:
    """The status word of a per-graph launch: True = every graph done, False = declined (the device-wide route goes on)."""
    if status == 0:
        return True
    if status & 2:
        raise N.TgpNativeError(f"{name}: a graph did not finish within its round bound")
    if route == "graphs":
        raise N.TgpNativeError(f"{name} declined: the edge list is not grouped by graph or {what} joins two graphs")
    return False


def _run_rounds(launch, n: int, name: str, what: str, dev) -> Tuple[int, int]:
    """Device-wide rounds in batches of 4, 8, ... 256, one host wait per batch: ``launch(done, step, flags)`` enqueues
    rounds done .. done + step - 1, flags[j] = 0 for an idle one.  Returns (rounds launched, index of the first idle round)."""
    done, step, idle = 0, 4, None
    while idle is None:
        if done >= n + 4:  # every round retires a node while anything is left: n rounds is a hard cap
            raise N.TgpNativeError(f"{name}: {what} is not maximal after num_nodes rounds")
        flags = torch.empty(step, dtype=torch.int32, device=dev)
        launch(done, step, flags)
        got = flags.tolist()  # one host wait per batch of rounds
        if 0 in got:
            idle = done + got.index(0)
        done += step
        step = min(2 * step, 256)  # a long tail means chain-like structure: more rounds per host wait
    return done, idle


def _owner_labels(n: int, name: str, dev, st):
    """(label [n], index [2, n], words [4] int32, relabel): ``relabel()`` numbers the owners (label[i] == i) consecutively
    into ``index`` (flags + exclusive scan, no sort, no torch.unique) and leaves their count in words[2:] as one int64."""
    L = N.lib()
    if n > L.tgp_graclus_relabel_max_nodes():
        raise N.TgpNativeError(f"{name}: {n} nodes exceed the relabelling kernels' {L.tgp_graclus_relabel_max_nodes()}")
    label = torch.empty(n, dtype=torch.int64, device=dev)
    index = torch.empty(2, n, dtype=torch.int64, device=dev)
    words = torch.empty(4, dtype=torch.int32, device=dev)
    rws = N.workspace(L.tgp_graclus_relabel_workspace_bytes(n), dev)

    def relabel():
        _checked(L.tgp_graclus_relabel_i64, N.ptr(label), n, N.ptr(rws), rws.numel(), N.ptr(index), N.ptr(words[2:]),
                 None, None, None, st)
    return label, index, words, relabel


# ------------------------------------------------------------------------- k-MIS selection (csrc/kmis_select.hip)
def kmis_degree(edge_index: Tensor, edge_weight: Optional[Tensor], num_nodes: int) -> Tensor:
    """Weighted in-degree (select/kmis_select.py:21-32): deg[c] = sum of the weights of the edges into c, added in
    edge-list order (no float atomics: the same bits on every call)."""
    dev = N.require_device(edge_index, edge_weight)
    out = torch.zeros(num_nodes, dtype=torch.float32, device=dev)
    if num_nodes == 0 or edge_index.size(1) == 0:
        return out
    w = N.opt_f32_flat(edge_weight)
    grp = edge_group(edge_index, num_nodes, by_destination=True)
    _checked(N.lib().tgp_kmis_degree_f32, N.ptr(grp.row_ptr), N.ptr(grp.perm), N.ptr(w), num_nodes, N.ptr(out),
             N.stream_ptr(dev))
    return out


def kmis_updated_score(score: Tensor, edge_index: Tensor, order_k: int, heuristic: Optional[str]) -> Tensor:
    """score / (A^T + I)^k 1 ("greedy") or score / (A^T + I)^k score ("w-greedy") (select/kmis_select.py:264-282), the
    device-wide kernels.  "greedy" counts in integers; "w-greedy" adds every destination's terms in edge-list order
    starting from the node's own value."""
    dev = N.require_device(score, edge_index)
    score = N.f32c(score.reshape(-1))
    n = score.numel()
    if heuristic is None or n == 0:
        return score
    row, col = _edge_rows(edge_index)
    E, L, st = row.numel(), N.lib(), N.stream_ptr(dev)
    out = torch.empty_like(score)
    if heuristic == "greedy":
        ws = N.workspace(L.tgp_kmis_workspace_bytes(n), dev)
        _checked(L.tgp_kmis_greedy_f32, N.ptr(row), N.ptr(col), E, n, int(order_k), N.ptr(score), N.ptr(ws), ws.numel(),
                 N.ptr(out), st)
        return out
    if heuristic != "w-greedy":
        raise ValueError(f"Unrecognized `score_heuristic` value: {heuristic}")
    if order_k <= 0 or E == 0:
        return score / score
    grp = edge_group(edge_index, n, by_destination=True)
    cur, spare = score, [torch.empty_like(score), torch.empty_like(score)] if order_k > 1 else []
    for h in range(order_k):
        last = h == order_k - 1
        dst = out if last else spare[h % 2]
        _checked(L.tgp_kmis_wsum_f32, N.ptr(row), N.ptr(grp.row_ptr), N.ptr(grp.perm), N.ptr(cur),
                 N.ptr(score) if last else None, n, N.ptr(dst), st)
        cur = dst
    return out


class KMISResult:
    """What one k-MIS selection leaves: ``index`` [2, N] (row 0 = 0..N-1, row 1 = cluster id), ``k`` clusters, ``mis``
    [k] (the MIS nodes, ascending = the node of every cluster id), ``updated`` (the score the priorities came from, or
    None for an explicit permutation), ``route`` ("graphs" / "rounds") and ``rounds`` launched on the device-wide route."""
    __slots__ = ("index", "k", "mis", "updated", "route", "rounds")


def kmis_route(num_nodes: int, num_edges: int, graph_ptr: Optional[Tensor], max_graph_nodes: Optional[int]) -> str:
    """The route a selection takes, from what the host already knows (:func:`_frame_route`)."""
    return _frame_route("tgp_kmis_max_graph_nodes", False, num_nodes, num_edges, graph_ptr, max_graph_nodes)


def kmis_select(edge_index: Tensor, num_nodes: int, order_k: int = 1, score: Optional[Tensor] = None,
                heuristic: Optional[str] = None, perm: Optional[Tensor] = None, graph_ptr: Optional[Tensor] = None,
                max_graph_nodes: Optional[int] = None, route: Optional[str] = None) -> KMISResult:
    """Maximal k-independent set + clusters (select/kmis_select.py:35-170) by node priority: ``perm`` (a permutation,
    first = highest priority), else descending ``heuristic``-updated ``score`` with ties to the lower node index, else
    the node order.  ``graph_ptr`` / ``max_graph_nodes``: offsets and longest graph of a sorted batch.  ``route``: None
    picks (``kmis_route``); "rounds" forces the device-wide kernels (tests run both on one input); a "graphs" call the
    kernel declines (an edge between two graphs, a list not grouped by graph) goes on device-wide.  One host wait per
    call on the per-graph route (status + cluster count); one per batch of rounds device-wide."""
    dev = N.require_device(edge_index, score, perm)
    row, col = _edge_rows(edge_index)
    E, n, k = row.numel(), int(num_nodes), int(order_k)
    if k < 1:
        raise ValueError(f"order_k must be at least 1, got {order_k}")
    L, st = N.lib(), N.stream_ptr(dev)
    res = KMISResult()
    res.updated, res.rounds = None, 0
    if n == 0:
        res.index = torch.empty(2, 0, dtype=torch.int64, device=dev)
        res.k, res.mis, res.route = 0, torch.empty(0, dtype=torch.int64, device=dev), "rounds"
        return res
    rank = None
    if perm is not None or score is None:
        rank = _rank_of(n, perm, "node", dev)
    else:
        score = N.f32c(score.reshape(-1))
        if score.numel() != n:
            raise ValueError(f"score must have one entry per node ({n}), got {score.numel()}")
        if heuristic not in (None, "greedy", "w-greedy"):
            raise ValueError(f"Unrecognized `score_heuristic` value: {heuristic}")
    want = _frame_route("tgp_kmis_max_graph_nodes", False, n, E, graph_ptr, max_graph_nodes, route)
    label, index, words, relabel_owners = _owner_labels(n, "kmis_select", dev, st)  # words: [status, -, K (int64)]
    mis = torch.empty(n, dtype=torch.int64, device=dev)

    def relabel():
        relabel_owners()
        _checked(L.tgp_kmis_mis_index_i64, N.ptr(label), N.ptr(index), n, N.ptr(mis), st)

    updated = None
    if want == "graphs":
        mode = 0 if rank is not None else (2 if heuristic == "greedy" else 1)
        if rank is None:
            updated = kmis_updated_score(score, edge_index, k, heuristic) if heuristic == "w-greedy" else score
            if mode == 2:
                updated = torch.empty_like(score)
        gp = N.i64c(graph_ptr)
        _checked(L.tgp_kmis_graphs, N.ptr(row), N.ptr(col), E, n, N.ptr(gp), gp.numel() - 1, int(max_graph_nodes), k,
                 mode, N.ptr(score if mode == 2 else updated), N.ptr(rank), N.ptr(updated) if mode == 2 else None,
                 N.ptr(label), N.ptr(words), st)
        relabel()
        got = words.tolist()  # the one host wait: status and K together
        if _frame_done(got[0], "tgp_kmis_graphs", route, "an edge"):
            res.index, res.k, res.mis, res.updated, res.route = index, int(got[2]), mis[:int(got[2])], updated, "graphs"
            return res
        if mode == 2:
            updated = None  # (graphs that declined left theirs unwritten)
    if rank is None and updated is None:
        updated = kmis_updated_score(score, edge_index, k, heuristic)
    ws = N.workspace(L.tgp_kmis_workspace_bytes(n), dev)
    _checked(L.tgp_kmis_rounds_start, N.ptr(rank), N.ptr(updated), n, N.ptr(ws), ws.numel(), st)

    def launch(done, step, flags):
        _checked(L.tgp_kmis_rounds, N.ptr(row), N.ptr(col), E, n, k, N.ptr(ws), done, step, N.ptr(flags), st)
    done, _ = _run_rounds(launch, n, "tgp_kmis_rounds", "the set", dev)
    _checked(L.tgp_kmis_clusters, N.ptr(row), N.ptr(col), E, n, k, N.ptr(ws), done, N.ptr(label), st)
    relabel()
    kk = int(words.tolist()[2])
    res.index, res.k, res.mis, res.updated, res.route, res.rounds = index, kk, mis[:kk], updated, "rounds", done
    return res


# ------------------------------------------------------------------------- edge contraction (csrc/edge_contract.hip)
EC_METHODS = {"softmax": 0, "tanh": 1, "sigmoid": 2}


def edge_contract_raw(x: Tensor, edge_index: Tensor, weight: Tensor, bias: Optional[Tensor] = None) -> Tensor:
    """raw[e] = x[row[e]].w[:F] + x[col[e]].w[F:] + b, float32 [E]: the reference's ``lin(cat([x[row], x[col]]))``
    (select/edge_contraction_select.py:217-218) as two per-node projections from one pass over ``x`` plus two gathered
    scalars per entry; the E x 2F matrix is never formed.  ``weight``: the 2F weights of ``Linear(2F, 1)``."""
    dev = N.require_device(x, edge_index, weight, bias)
    (x, ld), w = _row_operand(x, "edge_contract_raw", convert=True), N.f32c(weight.reshape(-1))
    n, F = x.size(0), x.size(1)
    if w.numel() != 2 * F:
        raise ValueError(f"weight must have 2 * F = {2 * F} entries, got {w.numel()}")
    b = N.opt_f32_flat(bias)
    row, col = _edge_rows(edge_index)
    E, L, st = row.numel(), N.lib(), N.stream_ptr(dev)
    p = torch.empty(2 * max(n, 1), dtype=torch.float32, device=dev)
    raw = torch.empty(E, dtype=torch.float32, device=dev)
    _checked(L.tgp_edge_contract_project_f32, N.ptr(x), n, F, ld, N.ptr(w), N.ptr(p), st)
    _checked(L.tgp_edge_contract_raw_f32, N.ptr(row), N.ptr(col), E, n, N.ptr(p), N.ptr(b), N.ptr(raw), st)
    return raw


def edge_contract_normalize(raw: Tensor, edge_index: Optional[Tensor], num_nodes: Optional[int],
                            method: str = "softmax", add_to_edge_score: float = 0.0) -> Tensor:
    """f(raw) + add_to_edge_score, float32 [E]; f = "softmax" over the entries that share ``col[e]``, "tanh" or
    "sigmoid" (select/edge_contraction_select.py:175-200, :221; the last two need neither ``edge_index`` nor
    ``num_nodes``).  The softmax takes each target's maximum and sum in the order of the by-destination index, without
    float atomics: the same bits on every call, and exactly ``1 + add_to_edge_score`` on a target with one incoming
    entry."""
    dev = N.require_device(raw, edge_index)
    if method not in EC_METHODS:
        raise ValueError(f"method must be one of {sorted(EC_METHODS)}, got {method!r}")
    raw = N.f32c(raw.reshape(-1))
    E, L, st = raw.numel(), N.lib(), N.stream_ptr(dev)
    out = torch.empty(E, dtype=torch.float32, device=dev)
    if E == 0:
        return out
    n, col, grp, seg, hubs, cap = 0, None, None, None, None, 0
    if method == "softmax":
        n = int(num_nodes)
        _, col = _edge_rows(edge_index)
        if col.numel() != E:
            raise ValueError(f"raw must have one entry per edge ({col.numel()}), got {E}")
        grp = edge_group(edge_index, n, by_destination=True)
        seg = torch.empty(2 * max(n, 1), dtype=torch.float32, device=dev)
        cap = E // int(L.tgp_edge_contract_hub_degree()) + 1
        hubs = torch.empty(cap + 1, dtype=torch.int32, device=dev)
    _checked(L.tgp_edge_contract_normalize_f32, N.ptr(raw), N.ptr(col), E, n, EC_METHODS[method],
             float(add_to_edge_score), N.ptr(grp.row_ptr) if grp else None, N.ptr(grp.perm) if grp else None,
             N.ptr(seg), N.ptr(hubs), cap, N.ptr(out), st)
    return out


def edge_contract_scores(x: Tensor, edge_index: Tensor, weight: Tensor, bias: Optional[Tensor] = None,
                         method: str = "softmax", add_to_edge_score: float = 0.5) -> Tensor:
    """The edge scores of EdgeContractionSelect without dropout (select/edge_contraction_select.py:217-221):
    :func:`edge_contract_raw` then :func:`edge_contract_normalize`."""
    raw = edge_contract_raw(x, edge_index, weight, bias)
    return edge_contract_normalize(raw, edge_index, x.size(0), method, add_to_edge_score)


class EdgeContractResult:
    """What one edge-contraction selection leaves: ``index`` [2, N] (row 0 = 0..N-1, row 1 = cluster id), ``k`` clusters,
    ``match`` (positions of the matched entries, ascending; compacted on first access), ``matched`` uint8 [E] (its flags),
    ``medge`` [N] (the matched entry of every node, -1 for a singleton), ``weight`` [N] (the matched entry's score for
    both members, 1 for a singleton; None for an explicit permutation), ``route`` ("graphs" / "rounds") and ``rounds``
    (rounds that still met a live entry)."""
    __slots__ = ("index", "k", "matched", "medge", "weight", "route", "rounds", "_match")

    @property
    def match(self) -> Tensor:
        if self._match is None:
            m = self.matched
            got = mask_index(m) if 0 < m.numel() < (1 << 31) else None
            self._match = got[0][0] if got is not None else m.nonzero().view(-1)
        return self._match


def edge_contract_route(num_nodes: int, num_edges: int, graph_ptr: Optional[Tensor],
                        max_graph_nodes: Optional[int]) -> str:
    """The route a matching takes, from what the host already knows (:func:`_frame_route`; no entries: "rounds")."""
    return _frame_route("tgp_edge_contract_max_graph_nodes", True, num_nodes, num_edges, graph_ptr, max_graph_nodes)


def edge_contract_select(edge_index: Tensor, num_nodes: int, score: Optional[Tensor] = None,
                         graph_ptr: Optional[Tensor] = None, max_graph_nodes: Optional[int] = None,
                         route: Optional[str] = None, perm: Optional[Tensor] = None) -> EdgeContractResult:
    """Maximal matching + clusters (select/edge_contraction_select.py:14-111, :223-236) by entry priority: ``perm`` (a
    permutation of the entries, first = highest priority), else descending ``score`` with ties to the lower position, else
    the list order.  Entries are directed and distinct: duplicates carry different ranks, a self-loop matches its node
    with itself.  ``cluster[col[m]] = row[m]`` for a matched entry ``m`` (the source represents the pair), ids are the
    rank of the representative among all representatives.  ``graph_ptr`` / ``max_graph_nodes``: offsets and longest graph
    of a sorted batch.  ``route``: None picks (``edge_contract_route``); "rounds" forces the device-wide kernels; a
    "graphs" call the kernel declines (an entry between two graphs, a list not grouped by graph) goes on device-wide.
    One host wait per call on the per-graph route (status, rounds and cluster count together); one per batch of rounds
    device-wide plus one for the count."""
    dev = N.require_device(edge_index, score, perm)
    row, col = _edge_rows(edge_index)
    E, n = row.numel(), int(num_nodes)
    L, st = N.lib(), N.stream_ptr(dev)
    if E >= (1 << 32):
        raise N.TgpNativeError(f"edge_contract_select: {E} entries exceed the 32-bit entry positions of the keys")
    res = EdgeContractResult()
    res.weight, res.rounds, res._match = None, 0, None
    if n == 0:
        res.index = torch.empty(2, 0, dtype=torch.int64, device=dev)
        res.k, res.route = 0, "rounds"
        res.matched = torch.zeros(E, dtype=torch.uint8, device=dev)
        res.medge = torch.empty(0, dtype=torch.int64, device=dev)
        res.weight = None if score is None else torch.empty(0, dtype=torch.float32, device=dev)
        return res
    rank = None
    if perm is not None or score is None:
        rank, score = _rank_of(E, perm, "edge", dev), None
    else:
        score = N.f32c(score.reshape(-1))
        if score.numel() != E:
            raise ValueError(f"score must have one entry per edge ({E}), got {score.numel()}")
    want = _frame_route("tgp_edge_contract_max_graph_nodes", True, n, E, graph_ptr, max_graph_nodes, route)
    label, index, words, relabel = _owner_labels(n, "edge_contract_select", dev, st)  # [status, rounds, K (int64)]
    matched = torch.empty(E, dtype=torch.uint8, device=dev)
    medge = torch.empty(n, dtype=torch.int64, device=dev)
    weight = None if score is None else torch.empty(n, dtype=torch.float32, device=dev)

    def finish():
        relabel()
        if weight is not None:
            _checked(L.tgp_edge_contract_weights_f32, N.ptr(medge), N.ptr(score), n, E, N.ptr(weight), st)

    res.index, res.matched, res.medge, res.weight = index, matched, medge, weight
    if want == "graphs":
        gp = N.i64c(graph_ptr)
        _checked(L.tgp_edge_contract_graphs, N.ptr(row), N.ptr(col), E, n, N.ptr(gp), gp.numel() - 1,
                 int(max_graph_nodes), N.ptr(score), N.ptr(rank), N.ptr(matched), N.ptr(label), N.ptr(medge),
                 N.ptr(words), st)
        finish()
        got = words.tolist()  # the one host wait: status, rounds and K together
        if _frame_done(got[0], "tgp_edge_contract_graphs", route, "an entry"):
            res.k, res.route, res.rounds = int(got[2]), "graphs", int(got[1])
            return res
    ws = N.workspace(L.tgp_edge_contract_workspace_bytes(n), dev)
    _checked(L.tgp_edge_contract_rounds_start, n, E, N.ptr(ws), ws.numel(), N.ptr(matched), N.ptr(label), N.ptr(medge),
             st)

    def launch(done, step, flags):
        _checked(L.tgp_edge_contract_rounds, N.ptr(row), N.ptr(col), E, n, N.ptr(score), N.ptr(rank), N.ptr(ws), done,
                 step, N.ptr(flags), N.ptr(matched), N.ptr(label), N.ptr(medge), st)
    _, live = _run_rounds(launch, n, "tgp_edge_contract_rounds", "the matching", dev)
    finish()
    res.k, res.route, res.rounds = int(words.tolist()[2]), "rounds", live
    return res


def row_dot(x: Tensor, w: Tensor) -> Tensor:
    """out[i] = <x[i,:], w> (select/topk_select.py:176) in one pass over x."""
    dev = N.require_device(x, w)
    (x, ld), w = _row_operand(x, "row_dot", convert=True), N.f32c(w.reshape(-1))
    out = torch.empty(x.size(0), dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_row_dot_f32, N.ptr(x), x.size(0), x.size(1), ld, N.ptr(w), N.ptr(out), N.stream_ptr(dev))
    return out


def topk_score(x: Tensor, w: Tensor, tanh: bool) -> Tensor:
    """act(x.w / ||w||_2), act = tanh or identity: TopkSelect's ratio-mode score (select/topk_select.py:176-184) in
    the one pass over x (no gradient: inference and detached inputs)."""
    dev = N.require_device(x, w)
    (x, ld), w = _row_operand(x, "topk_score", convert=True), N.f32c(w.reshape(-1))
    out = torch.empty(x.size(0), dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_topk_score_f32, N.ptr(x), x.size(0), x.size(1), ld, N.ptr(w), 1 if tanh else 0, N.ptr(out),
             N.stream_ptr(dev))
    return out


def weighted_colsum(x: Tensor, g: Tensor) -> Tensor:
    """out[f] = sum_i g[i] x[i,f]: the weight gradient of :func:`row_dot`."""
    dev = N.require_device(x, g)
    (x, ld), g = _row_operand(x, "weighted_colsum", convert=True), N.f32c(g.reshape(-1))
    out = torch.empty(x.size(1), dtype=torch.float32, device=dev)
    L = N.lib()
    ws = N.workspace(L.tgp_weighted_colsum_workspace_bytes(x.size(1)), dev)
    _checked(L.tgp_weighted_colsum_f32, N.ptr(x), x.size(0), x.size(1), ld, N.ptr(g), N.ptr(out), N.ptr(ws), ws.numel(),
             N.stream_ptr(dev))
    return out


def topk_pool_bwd_fits(x: Tensor, w: Tensor) -> bool:
    """Shapes / layouts :func:`topk_pool_bwd` takes (the others keep the operator-by-operator backward)."""
    return bool(x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and w.dtype == torch.float32
                and w.numel() == x.size(1) and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0
                and N.lib().tgp_topk_pool_bwd_fits(x.size(1)))


def topk_pool_bwd(x: Tensor, node_index: Tensor, cluster_index: Optional[Tensor], values: Tensor,
                  g_xpool: Optional[Tensor], g_values: Optional[Tensor], w: Tensor, use_tanh: bool,
                  want_gx: bool, want_gw: bool):
    """``(gx [N,F] or None, gw [F] or None)``: backward of TopK pooling's trained path -- score, kept values of S, gated
    Reduce -- in one pass over the kept rows (``tgp_topk_pool_bwd_f32``; poolers/topk.py:150-190)."""
    dev = N.require_device(x, node_index, cluster_index, values, g_xpool, g_values, w)
    n, F = x.size(0), x.size(1)
    k = node_index.numel()
    ni = N.i64c(node_index)
    ci = N.opt_i64(cluster_index)
    vals = N.f32c(values.reshape(-1))
    gp = None if g_xpool is None else N.f32c(g_xpool.reshape(k, F))
    gv = N.opt_f32_flat(g_values)
    wc = N.f32c(w.reshape(-1))
    # 16-byte loads: an upstream gradient or a parameter that is a view at an odd offset of a larger buffer (a flattened
    # parameter bucket, a slice of a concatenation) is copied once
    if gp is not None and gp.data_ptr() % 16:
        gp = gp.clone()
    if wc.data_ptr() % 16:
        wc = wc.clone()
    gx = torch.empty(n, F, dtype=torch.float32, device=dev) if want_gx else None
    gw = torch.empty(F, dtype=torch.float32, device=dev) if want_gw else None
    L = N.lib()
    ws = N.workspace(L.tgp_topk_pool_bwd_workspace_bytes(F), dev) if want_gw else None
    _checked(L.tgp_topk_pool_bwd_f32, x.data_ptr(), n, F, x.stride(0), N.ptr(ni), N.ptr(ci), N.ptr(vals), k, N.ptr(gp),
             N.ptr(gv), N.ptr(wc), 1 if use_tanh else 0, N.ptr(gx), N.ptr(gw), N.ptr(ws),
             ws.numel() if ws is not None else 0, N.stream_ptr(dev))
    return gx, gw


def pair_dot(a: Tensor, ia: Tensor, b: Tensor, ib: Tensor) -> Tensor:
    """out[e] = <a[ia_e,:], b[ib_e,:]>: the assignment-weight gradient of the sparse Reduce / Lift."""
    dev = N.require_device(a, ia, b, ib)
    a, b, ia, ib = N.f32c(a), N.f32c(b), N.i64c(ia), N.i64c(ib)
    if a.dim() != 2 or b.dim() != 2 or a.size(1) != b.size(1) or ia.numel() != ib.numel():
        raise ValueError(f"pair_dot: a {tuple(a.shape)}, b {tuple(b.shape)}, {ia.numel()} / {ib.numel()} indices")
    out = torch.empty(ia.numel(), dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_pair_dot_f32, N.ptr(ia), N.ptr(ib), ia.numel(), N.ptr(a), N.ptr(b), a.size(1), N.ptr(out),
             N.stream_ptr(dev))
    return out


def edge_dot(s: Tensor, edge_index: Tensor) -> Tensor:
    """ss[e] = <S[row_e], S[col_e]> (utils/losses.py:73-127, 661-708: ``(S[src] * S[dst]).sum(-1)``) in one pass."""
    dev = N.require_device(s, edge_index)
    row, col = _edge_rows(edge_index)
    if s.dtype == torch.float64:
        return (s[row] * s[col]).sum(-1)
    s = N.f32c(s)
    out = torch.empty(row.numel(), dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_edge_dot_f32, N.ptr(row), N.ptr(col), row.numel(), N.ptr(s), s.size(0), s.size(1), N.ptr(out),
             N.stream_ptr(dev))
    return out


def bmm(a: Tensor, b: Tensor, trans_a: bool = False, accumulate_into: Optional[Tensor] = None) -> Tensor:
    """C[g] = op(A[g]) @ B[g] on the fp32 matrix cores.  a: [G,M,Kd] (or [G,Kd,M] when trans_a),
    b: [G,Kd,Nc]; 2-D operands are treated as G = 1.  ``accumulate_into`` (contiguous fp32 [G,M,Nc]): C += product in
    the GEMM epilogue, returned as that tensor.  A float64 operand sends the product to the fp64 matrix path
    (tgp_bmm_f64); the result is float64."""
    dev = N.require_device(a, b)
    f64 = _any_f64(a, b) or (accumulate_into is not None and accumulate_into.dtype == torch.float64)
    conv, dt = (N.f64c, torch.float64) if f64 else (N.f32c, torch.float32)
    a3 = conv(a if a.dim() == 3 else a.unsqueeze(0))
    b3 = conv(b if b.dim() == 3 else b.unsqueeze(0))
    G = max(a3.size(0), b3.size(0))
    if trans_a:
        Kd, M = a3.size(1), a3.size(2)
    else:
        M, Kd = a3.size(1), a3.size(2)
    if b3.size(1) != Kd:
        raise ValueError(f"bmm inner dimensions differ: {tuple(a.shape)} x {tuple(b.shape)}")
    Nc = b3.size(2)
    sA = 0 if a3.size(0) == 1 else a3.stride(0)
    sB = 0 if b3.size(0) == 1 else b3.stride(0)
    acc = accumulate_into is not None
    if acc:
        out = accumulate_into
        if (out.dtype != dt or not out.is_contiguous() or out.numel() != G * M * Nc or out.device != dev):
            raise ValueError(f"bmm: accumulate_into must be a contiguous {dt} tensor of the product's shape")
    else:
        out = torch.empty(G, M, Nc, dtype=dt, device=dev)
    L = N.lib()
    args = (N.ptr(a3), N.ptr(b3), N.ptr(out), G, M, Nc, Kd, 1 if trans_a else 0, a3.stride(1), b3.stride(1), Nc, sA, sB,
            M * Nc)
    if f64:  # (one float64 entry: accumulation is a flag of it)
        _checked(L.tgp_bmm_f64, *args, 1 if acc else 0, N.stream_ptr(dev))
    else:
        _checked(L.tgp_bmm_accumulate_f32 if acc else L.tgp_bmm_f32, *args, N.stream_ptr(dev))
    return out if (acc or a.dim() == 3 or b.dim() == 3) else out[0]


# ------------------------------------------------------------------------- A13
def mlp_select(x: Tensor, weight: Tensor, bias: Optional[Tensor], mask: Optional[Tensor]) -> Tensor:
    """S = softmax(x W^T + b) * mask[..., None] (select/mlp_select.py:139-145, single Linear: :67) in one pass over
    x.  x [..., F], weight [K, F], bias [K] or None, mask broadcastable to x.shape[:-1] (bool) or None."""
    dev = N.require_device(x, weight)
    lead = x.shape[:-1]
    x2 = N.f32c(x).reshape(-1, x.size(-1))
    w, b = N.f32c(weight), N.opt_f32(bias)
    M, F, Kc = x2.size(0), x2.size(1), w.size(0)
    if w.size(1) != F:
        raise ValueError(f"mlp_select: weight {tuple(weight.shape)} does not match features {F}")
    m8 = None
    if mask is not None:
        m8 = mask.reshape(-1)
        if m8.numel() != M:
            raise ValueError(f"mlp_select: mask {tuple(mask.shape)} does not match x {tuple(x.shape)}")
        if m8.dtype != torch.bool and m8.dtype != torch.uint8:
            m8 = m8 != 0
        m8 = m8.contiguous().view(torch.uint8)
    L = N.lib()
    st = N.stream_ptr(dev)
    if Kc <= L.tgp_mlp_select_max_fused_k():
        out = torch.empty(M, Kc, dtype=torch.float32, device=dev)
        _checked(L.tgp_mlp_select_f32, N.ptr(x2), N.ptr(w), N.ptr(b), N.ptr(m8), M, F, Kc, N.ptr(out), st)
    else:  # wider than eight accumulator tiles: tiled GEMM for the logits, then bias + softmax + mask in place
        out = bmm(x2, w.t().contiguous())
        _checked(L.tgp_softmax_rows_f32, N.ptr(out), N.ptr(b), N.ptr(m8), M, Kc, st)
    return out.view(*lead, Kc)


def softmax_bwd(s: Tensor, ds: Tensor) -> Tensor:
    """dY = S * (dS - <dS, S>_row): gradient of S = softmax(Y) * mask w.r.t. Y (masked rows have S = 0)."""
    dev = N.require_device(s, ds)
    s2, d2 = N.f32c(s).reshape(-1, s.size(-1)), N.f32c(ds).reshape(-1, s.size(-1))
    out = torch.empty_like(s2)
    _checked(N.lib().tgp_softmax_bwd_f32, N.ptr(s2), N.ptr(d2), N.ptr(out), s2.size(0), s2.size(1), N.stream_ptr(dev))
    return out.view(s.shape)


def segment_gemm_tn(s: Tensor, y: Tensor, ptr: Tensor, max_nodes: int) -> Tensor:
    """C[b] = S_b^T Y_b over node rows ptr[b]..ptr[b+1] (reduce/base_reduce.py:170-182,
    connect/dense_conn.py:195-206) in one launch."""
    dev = N.require_device(s, y, ptr)
    f64 = _any_f64(s, y)
    conv = N.f64c if f64 else N.f32c
    s, y, ptr = conv(s), conv(y), N.i64c(ptr)
    B = ptr.numel() - 1
    K, F = s.size(1), y.size(1)
    out = torch.empty(B, K, F, dtype=s.dtype, device=dev)
    L = N.lib()
    ws = N.workspace((L.tgp_segment_gemm_tn_workspace_bytes_f64 if f64 else L.tgp_segment_gemm_tn_workspace_bytes)(
        B, K, F, max_nodes), dev)
    _checked(L.tgp_segment_gemm_tn_f64 if f64 else L.tgp_segment_gemm_tn_f32, N.ptr(s), N.ptr(y), N.ptr(ptr),
             N.ptr(out), B, s.size(0), K, F, max_nodes, N.ptr(ws), ws.numel(), N.stream_ptr(dev))
    return out


def segment_gemm_nn(a: Tensor, bm: Tensor, ptr: Tensor, max_nodes: int) -> Tensor:
    """C[rows of graph b] = A[rows of graph b] @ Bm[b] (lift/base_lift.py:138-247 on an un-padded batch; the
    backward of :func:`segment_gemm_tn`) in one launch.  a: [Ntot,Kd], bm: [B,Kd,Nc]."""
    dev = N.require_device(a, bm, ptr)
    f64 = _any_f64(a, bm)
    conv = N.f64c if f64 else N.f32c
    a, bm, ptr = conv(a), conv(bm), N.i64c(ptr)
    B = ptr.numel() - 1
    if bm.dim() != 3 or bm.size(0) != B or bm.size(1) != a.size(1):
        raise ValueError(f"segment_gemm_nn: a {tuple(a.shape)} x bm {tuple(bm.shape)} with {B} graphs")
    out = torch.empty(a.size(0), bm.size(2), dtype=a.dtype, device=dev)
    L = N.lib()
    _checked(L.tgp_segment_gemm_nn_f64 if f64 else L.tgp_segment_gemm_nn_f32, N.ptr(a), N.ptr(bm), N.ptr(ptr),
             N.ptr(out), B, a.size(0), a.size(1), bm.size(2), max_nodes, N.stream_ptr(dev))
    return out


def rowptr_from_sorted(row: Tensor, num_rows: int, out: Tensor) -> Tensor:
    """CSR offsets (int32 [num_rows+1]) of an ascending int64 row vector."""
    dev = N.require_device(row, out)
    row = N.i64c(row)
    _checked(N.lib().tgp_rowptr_from_sorted_i64, N.ptr(row), row.numel(), num_rows, N.ptr(out), N.stream_ptr(dev))
    return out


def _spmm_sorted(edge_index: Tensor, edge_weight: Optional[Tensor], num_rows: int, s: Tensor, f64: bool):
    """(T, row_ptr int32 [num_rows+1]): T = A S for a row-sorted (coalesced) edge list and the CSR offsets built on the
    way, the operands taken as float32 or -- ``f64`` -- as float64."""
    dev = N.require_device(edge_index, edge_weight, s)
    row, col = _edge_rows(edge_index)
    conv = N.f64c if f64 else N.f32c
    s = conv(s)
    w = None if edge_weight is None else conv(edge_weight)
    L = N.lib()
    st = N.stream_ptr(dev)
    row_ptr = torch.empty(num_rows + 1, dtype=torch.int32, device=dev)
    _checked(L.tgp_rowptr_from_sorted_i64, N.ptr(row), row.numel(), num_rows, N.ptr(row_ptr), st)
    out = torch.empty(num_rows, s.size(1), dtype=s.dtype, device=dev)
    _checked(L.tgp_spmm_csr_f64 if f64 else L.tgp_spmm_csr_f32, N.ptr(row_ptr), N.ptr(col), N.ptr(w), num_rows,
             row.numel(), N.ptr(s), s.size(1), N.ptr(out), st)
    return out, row_ptr


def spmm_sorted_csr(edge_index: Tensor, edge_weight: Optional[Tensor], num_rows: int, s: Tensor):
    """(T, row_ptr int32 [num_rows+1]): :func:`spmm_sorted` for float32 operands, handing the CSR offsets it built back."""
    return _spmm_sorted(edge_index, edge_weight, num_rows, s, False)


def spmm_sorted(edge_index: Tensor, edge_weight: Optional[Tensor], num_rows: int, s: Tensor) -> Tensor:
    """T = A S for a row-sorted (coalesced) edge list (connect/dense_conn.py:165,204), in float64 when S or a weight is."""
    return _spmm_sorted(edge_index, edge_weight, num_rows, s, _any_f64(s, edge_weight))[0]


_ROW_OFFSETS = TensorMemo(16)


def csr_offsets(edge_index: Tensor, num_rows: int) -> Tensor:
    """int32 [num_rows+1] CSR offsets of a row-sorted list: one launch for a new list, remembered per tensor object +
    version (full-batch training pools the same ``edge_index`` every step), like the per-graph edge ranges."""
    hit = _ROW_OFFSETS.get(edge_index, extra=num_rows)
    if hit is not None:
        return hit
    row, _ = _edge_rows(edge_index)
    out = torch.empty(num_rows + 1, dtype=torch.int32, device=edge_index.device)
    rowptr_from_sorted(row, num_rows, out)
    if not torch.cuda.is_current_stream_capturing():
        _ROW_OFFSETS.put(edge_index, out, extra=num_rows)
    return out


def spmm_csr(row_ptr: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor], num_rows: int, s: Tensor,
             want_stats: bool = False):
    """T = A S for a row-sorted coalesced float32 list whose CSR offsets the caller holds (one launch).
    ``want_stats``: ``(T, deg, q)`` -- the row sums of the weights and |S_i|^2 from the same launch
    (:func:`edge_row_stats` without its own pass; needs num_rows == S rows)."""
    dev = N.require_device(edge_index, edge_weight, s, row_ptr)
    _, col = _edge_rows(edge_index)
    s = N.f32c(s)
    w = N.opt_f32_flat(edge_weight)
    out = torch.empty(num_rows, s.size(1), dtype=torch.float32, device=dev)
    if want_stats == "entropy":
        # (T, partials or None): DiffPool's entropy sum over S rides along as per-workgroup shares (None: this shape does
        # not take the row kernel; diffpool_unbatched_tail then runs its own pass over S)
        if s.size(0) != num_rows:
            raise ValueError("spmm_csr(want_stats='entropy') needs a square A: one row of S per row of A")
        part = torch.empty(max(num_rows, 1), dtype=torch.float32, device=dev)
        n_part = ctypes.c_int(-1)
        _checked(N.lib().tgp_spmm_csr_entropy_f32, N.ptr(row_ptr), N.ptr(col), N.ptr(w), num_rows, col.numel(),
                 N.ptr(s), s.size(1), N.ptr(out), losses_eps(), N.ptr(part), ctypes.addressof(n_part),
                 N.stream_ptr(dev))
        return out, (part[: n_part.value] if n_part.value >= 0 else None)
    if want_stats:
        if s.size(0) != num_rows:
            raise ValueError("spmm_csr(want_stats=True) needs a square A: one row of S per row of A")
        dq = torch.empty(2, num_rows, dtype=torch.float32, device=dev)
        _checked(N.lib().tgp_spmm_csr_stats_f32, N.ptr(row_ptr), N.ptr(col), N.ptr(w), num_rows, col.numel(), N.ptr(s),
                 s.size(1), N.ptr(out), dq.data_ptr(), dq.data_ptr() + 4 * num_rows, N.stream_ptr(dev))
        return out, dq[0], dq[1]
    _checked(N.lib().tgp_spmm_csr_f32, N.ptr(row_ptr), N.ptr(col), N.ptr(w), num_rows, col.numel(), N.ptr(s), s.size(1),
             N.ptr(out), N.stream_ptr(dev))
    return out


def edge_row_stats(row_ptr: Tensor, edge_weight: Optional[Tensor], s: Tensor) -> Tuple[Tensor, Tensor]:
    """(deg [N], q [N]): row sums of the weights of a CSR edge list (entry counts without weights) and |S_i|^2, one
    launch (utils/losses.py:73-127: the degree term of sparse_mincut_loss without an index_add)."""
    dev = N.require_device(row_ptr, edge_weight, s)
    s = N.f32c(s)
    n = s.size(0)
    w = N.opt_f32_flat(edge_weight)
    deg = torch.empty(n, dtype=torch.float32, device=dev)
    q = torch.empty(n, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_edge_row_stats_f32, N.ptr(row_ptr), N.ptr(w), N.ptr(s), n, s.size(1), N.ptr(deg), N.ptr(q),
             N.stream_ptr(dev))
    return deg, q


def segment_gemm_tn3(s: Tensor, ys, ptr: Tensor, max_nodes: int, transpose0: bool = False,
                     post_flags: Optional[int] = None):
    """[S_b^T Y_j,b for j] for up to three float32 right-hand sides [Ntot,F_j] over node rows ptr[b]..ptr[b+1]: ONE
    product grid + one combine launch (the unbatched dense poolers' S^T [A S | X | S]).
    ``post_flags`` (r6; ys[0] must be [Ntot,K]): a last value ``adj_pool`` = the post-processing of the first product
    (utils/ops.py:282-335) from the same native call -- for 64 < K <= 176 its launch sums the slabs of all the products
    itself, no combine launch."""
    dev = N.require_device(s, ptr, *ys)
    s, ptr = N.f32c(s), N.i64c(ptr)
    ys = [N.f32c(y) for y in ys]
    if not 1 <= len(ys) <= 3 or any(y.dim() != 2 or y.size(0) != s.size(0) for y in ys):
        raise ValueError("segment_gemm_tn3: one to three [Ntot,F] right-hand sides expected")
    B, Kc = ptr.numel() - 1, s.size(1)
    fs = [y.size(1) for y in ys] + [0] * (3 - len(ys))
    outs = [torch.empty(B, Kc, y.size(1), dtype=torch.float32, device=dev) for y in ys]
    yp = [N.ptr(y) for y in ys] + [None] * (3 - len(ys))
    op = [N.ptr(o) for o in outs] + [None] * (3 - len(ys))
    L = N.lib()
    if post_flags is not None:
        if fs[0] != Kc:
            raise ValueError("segment_gemm_tn3(post_flags=...): the first right-hand side must be [Ntot,K]")
        adj_pool = torch.empty(B, Kc, Kc, dtype=torch.float32, device=dev)
        ws = N.workspace(L.tgp_segment_gemm_tn3_post_workspace_bytes(B, Kc, fs[1], fs[2], max_nodes), dev)
        _checked(L.tgp_segment_gemm_tn3_post_f32, N.ptr(s), yp[0], yp[1], fs[1], yp[2], fs[2], N.ptr(ptr), op[0], op[1],
                 op[2], N.ptr(adj_pool), B, s.size(0), Kc, max_nodes, 1 if transpose0 else 0, int(post_flags),
                 ops_eps(), N.ptr(ws), ws.numel(), N.stream_ptr(dev))
        return outs + [adj_pool]
    ws = N.workspace(L.tgp_segment_gemm_tn3_workspace_bytes(B, Kc, fs[0], fs[1], fs[2], max_nodes), dev)
    # transpose0: the first result (K x K) leaves the combine launch transposed
    _checked(L.tgp_segment_gemm_tn3_f32, N.ptr(s), yp[0], fs[0], yp[1], fs[1], yp[2], fs[2], N.ptr(ptr), op[0], op[1],
             op[2], B, s.size(0), Kc, max_nodes, 1 if transpose0 else 0, N.ptr(ws), ws.numel(), N.stream_ptr(dev))
    return outs


_POOL_ROWS_ONE_CALL = os.environ.get("TGP_POOL_ROWS_ONE_CALL", "1") != "0"  # A/B switch (read once)


def pool_rows_forward(x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], s_given: Optional[Tensor],
                      row_ptr: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor], ptr: Tensor, max_nodes: int,
                      transposed: bool, flags: int, mode: int, scales=(0.0, 0.0), sw2=0.0):
    """The forward of the dense poolers' un-padded rows route as ONE native call (``tgp_pool_rows_fwd_f32``: selector,
    T = A S with the losses' row statistics, S^T [T | X | S] + post-processing, loss tail) -- the launches of
    :func:`mlp_select`, :func:`spmm_csr`, :func:`segment_gemm_tn3` and :func:`mincut_terms_fused` /
    :func:`diffpool_unbatched_tail`, without the host work between them.  ``mode`` 0: no losses, 1: MinCut, 2: DiffPool.
    Returns a dict: s, t, raw, x_pool, gram, adj_pool and -- mode 1 -- deg, q, den, terms, stats, both; -- mode 2 --
    lossv.  None when the case is not this entry's (the caller composes the operators): float32 contiguous operands, a
    selector of at most 256 clusters."""
    if not _POOL_ROWS_ONE_CALL or x.dtype != torch.float32 or x.dim() != 2 or not x.is_contiguous():
        return None
    selector = s_given is None
    n, F = x.shape
    if selector:
        if (weight is None or weight.dtype != torch.float32 or weight.dim() != 2 or weight.size(1) != F
                or not weight.is_contiguous() or weight.size(0) > 256
                or (bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous()))):
            return None
        Kc = weight.size(0)
    else:
        if s_given.dtype != torch.float32 or s_given.dim() != 2 or s_given.size(0) != n or not s_given.is_contiguous():
            return None
        Kc = s_given.size(1)
    if (n == 0 or Kc == 0 or row_ptr.dtype != torch.int32 or row_ptr.numel() != n + 1 or ptr.dtype != torch.int64
            or not ptr.is_contiguous()):
        return None
    w = edge_weight
    if w is not None:
        if w.dtype != torch.float32:
            return None
        w = w.reshape(-1)
        if not w.is_contiguous():
            w = w.contiguous()
    dev = N.require_device(x, weight, bias, s_given, row_ptr, edge_index, w, ptr)
    _, col = _edge_rows(edge_index)
    B = ptr.numel() - 1
    f32 = dict(dtype=torch.float32, device=dev)
    s = torch.empty(n, Kc, **f32) if selector else s_given
    t = torch.empty(n, Kc, **f32)
    raw = torch.empty(B, Kc, Kc, **f32)
    x_pool = torch.empty(B, Kc, F, **f32)
    adj_pool = torch.empty(B, Kc, Kc, **f32)
    gram = torch.empty(B, Kc, Kc, **f32) if mode else None
    rowstat = den = terms = stats = means = dstats = out2 = None
    ticket = None
    L = N.lib()
    st = N.stream_ptr(dev)
    sw2_dev = None
    if mode == 1:
        rowstat = torch.empty(2, n, **f32)
        den, terms, stats = torch.empty(B, **f32), torch.empty(2, B, **f32), torch.empty(B, 4, **f32)
        if B <= 256 and not torch.cuda.is_current_stream_capturing():
            means = torch.empty(2, **f32)
            ticket = _sps_state(dev, st, 0).ticket.data_ptr() + 16
    elif mode == 2:
        rowstat = torch.empty(n, **f32)
        dstats, out2 = torch.empty(B, 2, **f32), torch.empty(2, **f32)
        sw2_dev = N.f32c(sw2.reshape(1)) if isinstance(sw2, Tensor) else None
    ws = N.workspace(L.tgp_pool_rows_fwd_workspace_bytes(B, Kc, F, max_nodes, n), dev)
    _checked(L.tgp_pool_rows_fwd_f32, x.data_ptr(), n, F, N.ptr(weight) if selector else None,
             N.ptr(bias) if selector else None, s.data_ptr(), row_ptr.data_ptr(), N.ptr(col), N.ptr(w), col.numel(),
             ptr.data_ptr(), B, Kc, max_nodes, 1 if transposed else 0, int(flags), ops_eps(), losses_eps(), int(mode),
             N.ptr(sw2_dev), 0.0 if (sw2_dev is not None or mode != 2) else float(sw2), float(scales[0]),
             float(scales[1]), t.data_ptr(), raw.data_ptr(), x_pool.data_ptr(), N.ptr(gram), adj_pool.data_ptr(),
             N.ptr(rowstat), N.ptr(den), N.ptr(terms), N.ptr(stats), N.ptr(means), ticket, N.ptr(dstats), N.ptr(out2),
             ws.data_ptr(), ws.numel(), st)
    out = dict(s=s, t=t, raw=raw, x_pool=x_pool, gram=gram, adj_pool=adj_pool)
    if mode == 1:
        out.update(deg=rowstat[0], q=rowstat[1], den=den, terms=terms, stats=stats,
                   both=means if means is not None else terms.mean(dim=1))
    elif mode == 2:
        out.update(lossv=out2)
    return out


def pool_rows_forward_composed(x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], s_given: Optional[Tensor],
                               row_ptr: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor], ptr: Tensor,
                               max_nodes: int, transposed: bool, flags: int, mode: int, scales=(0.0, 0.0), sw2=0.0):
    """:func:`pool_rows_forward` one operator at a time: the same launches, the same dict, for any case.
    ``transposed``: the pooled adjacency is S^T A^T S (what the BATCHED poolers compute from a sparse input with
    adj_transpose=True, src.py:442-443) = the transpose of S^T (A S); MinCut's degrees are then the in-degrees."""
    n, out = x.size(0), {}
    s = mlp_select(x, weight, bias, None) if s_given is None else s_given
    if mode == 1:  # MinCut: out-degrees and |S_i|^2 ride along with T = A S
        t, deg, q = spmm_csr(row_ptr, edge_index, edge_weight, n, s, want_stats=True)
    elif mode == 2:  # DiffPool: the entropy sum over S rides along
        t, ent_part = spmm_csr(row_ptr, edge_index, edge_weight, n, s, want_stats="entropy")
    else:
        t = spmm_csr(row_ptr, edge_index, edge_weight, n, s)
    raw, x_pool, gram, adj_pool = segment_gemm_tn3(s, [t, x, s], ptr, max_nodes, transpose0=transposed, post_flags=flags)
    if mode == 1:
        # transposed: den = sum_j indeg_j q_j = sum_e w_e q[col_e], the tail walks the graph's entries itself
        den, terms, stats, both = mincut_terms_fused(raw, gram, None if transposed else deg, q, ptr=ptr, want_means=True,
                                                     edges=(row_ptr, edge_index, edge_weight) if transposed else None)
        out.update(deg=deg, q=q, den=den, terms=terms, stats=stats, both=both)
    elif mode == 2:
        out.update(lossv=diffpool_unbatched_tail(raw, gram, s, sw2, scales[0], scales[1], ent_partials=ent_part))
    out.update(s=s, t=t, raw=raw, x_pool=x_pool, gram=gram if mode else None, adj_pool=adj_pool)
    return out


def pool_rows(*args):
    """The rows route's forward: :func:`pool_rows_forward` where the case is that entry's, else the composed operators
    (same arguments, same dict)."""
    out = pool_rows_forward(*args)
    return out if out is not None else pool_rows_forward_composed(*args)


def pool_rows_backward(s: Tensor, t: Tensor, x: Tensor, weight: Tensor, raw: Tensor, gram, stats, den, deg, lossv,
                       ptr: Tensor, batch, slab_ptr: Tensor, max_nodes: int, flags: int, mode: int, transposed: bool,
                       scales, g_adj, g_raw, g_xp, g_s, g_la, g_lb, want_gx: bool, want_gw: bool, want_gb: bool):
    """(gX, gW, gbias) of the rows route's training step as ONE native call (``tgp_pool_rows_bwd_f32``) for the common
    case -- the selector folded in, A = A^T --, or None when an operand is not float32 / contiguous (the caller then makes
    the same launches one by one).  See functions._PoolUnbatchedFn.backward for the arithmetic."""
    if not _POOL_ROWS_ONE_CALL:
        return None
    n, Kc = s.shape
    F = x.size(1)
    B = ptr.numel() - 1
    dev = s.device
    f32 = torch.float32

    def ok(v, shape=None):
        return v is None or (v.dtype == f32 and v.is_contiguous() and (shape is None or tuple(v.shape) == tuple(shape)))

    if not (ok(s) and ok(t, (n, Kc)) and ok(x, (n, F)) and ok(weight, (Kc, F)) and ok(raw, (B, Kc, Kc)) and ok(gram)
            and ok(stats) and ok(den) and ok(deg) and ok(lossv) and ptr.dtype == torch.int64 and ptr.is_contiguous()
            and (batch is None or (batch.dtype == torch.int64 and batch.is_contiguous())) and ok(g_raw, (B, Kc, Kc))
            and ok(g_s, (n, Kc)) and (g_la is None or g_la.dtype == f32) and (g_lb is None or g_lb.dtype == f32)):
        return None
    ga_bc = gx_bc = False
    if g_adj is not None:
        if tuple(g_adj.shape) != (B, Kc, Kc) or g_adj.dtype != f32:
            return None
        g_adj, ga_bc = _bcast_or_dense(g_adj, (B, Kc, Kc))
    if g_xp is not None:
        if tuple(g_xp.shape) != (B, Kc, F) or g_xp.dtype != f32:
            return None
        g_xp, gx_bc = _bcast_or_dense(g_xp, (B, Kc, F))
    pad, ld = TRAIN_PAD, train_columns(Kc, F).ld
    e = dict(dtype=f32, device=dev)
    ga = torch.empty(B, Kc, Kc, **e) if g_adj is not None else None
    rcat = torch.empty(B, ld, Kc, **e)
    c1 = torch.empty(B, **e) if mode == 1 else None
    gwcat = torch.empty(B, 2 * Kc, F, **e) if want_gx else None
    acat = torch.empty(n, ld, **e)
    gs = torch.empty(n, Kc, **e)
    gx = torch.empty(n, F, **e) if want_gx else None
    slabs = slab_ptr.numel() - 1
    part = torch.empty(slabs, Kc, F + pad, **e) if (want_gw or want_gb) else None
    gw = torch.empty(Kc, F, **e) if want_gw else None
    gb = torch.empty(Kc, **e) if want_gb else None
    _checked(N.lib().tgp_pool_rows_bwd_f32, s.data_ptr(), t.data_ptr(), x.data_ptr(), weight.data_ptr(), raw.data_ptr(),
             N.ptr(gram), N.ptr(stats), N.ptr(den), N.ptr(deg), N.ptr(lossv), ptr.data_ptr(), N.ptr(batch),
             slab_ptr.data_ptr(), slabs, n, B, Kc, F, max_nodes, int(flags), ops_eps(), losses_eps(), int(mode),
             1 if transposed else 0, 1.0 / B, float(scales[0]) if mode == 2 else 0.0,
             float(scales[1]) if mode == 2 else 0.0, N.ptr(g_adj), 1 if ga_bc else 0, N.ptr(g_raw), N.ptr(g_xp),
             1 if gx_bc else 0, N.ptr(g_s), N.ptr(g_la), N.ptr(g_lb), N.ptr(ga), rcat.data_ptr(), N.ptr(c1),
             N.ptr(gwcat), acat.data_ptr(), gs.data_ptr(), N.ptr(gx), N.ptr(part), N.ptr(gw), N.ptr(gb),
             N.stream_ptr(dev))
    return gx, gw, gb


def segment_gemm_nn_into(a: Tensor, bm: Tensor, ptr: Tensor, out: Tensor, max_nodes: int) -> Tensor:
    """out[rows of graph b] = a[rows of graph b] @ bm[b] for float32 VIEWS with unit last stride: ``a`` [Ntot,Kd] and
    ``out`` [Ntot,Nc] with any row stride (column blocks of a wider buffer), ``bm`` [B,Kd,Nc] with any row / batch stride."""
    dev = N.require_device(a, bm, ptr, out)
    if (a.dim() != 2 or bm.dim() != 3 or out.dim() != 2 or a.stride(1) != 1 or bm.stride(2) != 1 or out.stride(1) != 1
            or bm.size(1) != a.size(1) or out.size(1) != bm.size(2) or out.size(0) != a.size(0)
            or any(t.dtype != torch.float32 for t in (a, bm, out))):
        raise ValueError(f"segment_gemm_nn_into: {tuple(a.shape)} x {tuple(bm.shape)} -> {tuple(out.shape)}")
    ptr = N.i64c(ptr)
    _checked(N.lib().tgp_segment_gemm_nn_ld_f32, a.data_ptr(), a.stride(0), bm.data_ptr(), bm.stride(1), bm.stride(0),
             N.ptr(ptr), out.data_ptr(), out.stride(0), ptr.numel() - 1, a.size(0), a.size(1), bm.size(2), max_nodes,
             N.stream_ptr(dev))
    return out


def segment_gemm_tn_into(a: Tensor, y: Tensor, ptr: Tensor) -> Tensor:
    """[a[rows of b]^T @ y[rows of b] for b] -> [B,M,Nc] for float32 2-D VIEWS with unit last stride and any row stride
    (no node-range split: meant for short row ranges, e.g. the row slabs of a weight gradient)."""
    dev = N.require_device(a, y, ptr)
    if (a.dim() != 2 or y.dim() != 2 or a.stride(1) != 1 or y.stride(1) != 1 or a.size(0) != y.size(0)
            or a.dtype != torch.float32 or y.dtype != torch.float32):
        raise ValueError(f"segment_gemm_tn_into: {tuple(a.shape)}^T x {tuple(y.shape)}")
    ptr = N.i64c(ptr)
    B = ptr.numel() - 1
    out = torch.empty(B, a.size(1), y.size(1), dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_segment_gemm_tn_ld_f32, a.data_ptr(), a.stride(0), y.data_ptr(), y.stride(0), N.ptr(ptr),
             N.ptr(out), B, a.size(0), a.size(1), y.size(1), N.stream_ptr(dev))
    return out


def diffpool_unbatched_tail(raw: Tensor, gram: Tensor, s: Tensor, sw2, link_scale: float, ent_scale: float,
                            ent_partials: Optional[Tensor] = None) -> Tensor:
    """[2]: DiffPool's unbatched link-prediction loss sqrt(max(sum_e w_e^2 - 2 sum_b trace(raw_b) + sum_b |gram_b|^2, 0))
    * link_scale and entropy loss sum(-s log(s + eps)) * ent_scale (utils/losses.py:661-708, 476-483); ``sw2``: a
    0-dim device tensor or a Python number.  ``ent_partials``: shares of the entropy sum that are already there
    (``spmm_csr(want_stats="entropy")``): no pass over S here."""
    dev = N.require_device(raw, gram, s, ent_partials)
    raw, gram = N.f32c(raw), N.f32c(gram)
    B, Kc = raw.size(0), raw.size(-1)
    st = N.stream_ptr(dev)
    if ent_partials is not None:
        ws = N.f32c(ent_partials.reshape(-1))
        n_partial = ws.numel()
    else:
        ws, n_partial = _entropy_partials(s, dev, st)
    stats = torch.empty(B, 2, dtype=torch.float32, device=dev)
    out = torch.empty(2, dtype=torch.float32, device=dev)
    sw2_dev = N.f32c(sw2.reshape(1)) if isinstance(sw2, Tensor) else None
    _checked(N.lib().tgp_diffpool_unbatched_tail_f32, N.ptr(raw), N.ptr(gram), B, Kc, N.ptr(sw2_dev),
             0.0 if sw2_dev is not None else float(sw2), N.ptr(ws), n_partial, float(link_scale),
             float(ent_scale), N.ptr(stats), N.ptr(out), st)
    return out


# ------------------------------------------------------------------------- A14 (NDP)
def ndp_max_graph_nodes() -> int:
    return int(N.lib().tgp_ndp_max_graph_nodes())


def ndp_symmetric_max(edge_index: Tensor, weight: Optional[Tensor], num_nodes: int, indptr: Tensor):
    """(w_max [E], flag [1] int32): for a list that already is row-major sorted, duplicate-free, loop-free and
    pattern-symmetric, the weights NDPSelect's symmetrisation would produce (max with the reverse entry) and flag = 0;
    flag = 1 when the list is anything else (ndp_select.py:198-202 then needs the general route)."""
    dev = N.require_device(edge_index, weight, indptr)
    row, col = _edge_rows(edge_index)
    w = N.opt_f32_flat(weight)
    out = torch.empty(row.numel(), dtype=torch.float32, device=dev)
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    _checked(N.lib().tgp_ndp_symmetric_max_f32, N.ptr(row), N.ptr(col), N.ptr(w), row.numel(), num_nodes, N.ptr(indptr),
             N.ptr(out), N.ptr(flag), N.stream_ptr(dev))
    return out, flag


def ndp_partition(indptr: Tensor, col: Tensor, weight: Optional[Tensor], num_nodes: int, graph_ptr: Tensor,
                  max_graph_nodes: int, seed: int, max_iter: int = 500, tol: float = 1e-6, raw_keep: bool = False):
    """(keep [N] bool, info [B] int32, status int): NDPSelect's per-graph spectral +-1 partition
    (select/ndp_select.py:187-256) on a symmetric, self-loop-free CSR adjacency.  info[g] = LOBPCG steps used, -1 =
    the reference's random fallback (cut < 0.5); status != 0: declined, see include/tgp_hip.h.  ``tol``: relative
    eigen-residual |Ls x - lambda x| <= tol * lambda at which the iteration stops."""
    dev = N.require_device(indptr, col, weight, graph_ptr)
    if indptr.dtype != torch.int32:
        raise ValueError("ndp_partition: indptr must be int32")
    col, graph_ptr = N.i64c(col), N.i64c(graph_ptr)
    w = N.opt_f32_flat(weight)
    B = graph_ptr.numel() - 1
    # status | info | keep in one allocation, laid out as tgp_ndp_partition clears them with a single memset (r6)
    b_pad, n_keep = (max(B, 1) + 3) // 4 * 4, max(num_nodes, 1)
    buf = torch.empty(16 + 4 * b_pad + n_keep, dtype=torch.uint8, device=dev)
    status = buf[:4].view(torch.int32)
    info = buf[16:16 + 4 * b_pad].view(torch.int32)
    keep = buf[16 + 4 * b_pad:]
    _checked(N.lib().tgp_ndp_partition, N.ptr(indptr.contiguous()), N.ptr(col), N.ptr(w), num_nodes, col.numel(),
             N.ptr(graph_ptr), B, max_graph_nodes, int(seed) & ((1 << 64) - 1), max_iter, float(tol), N.ptr(keep),
             N.ptr(info), N.ptr(status), N.stream_ptr(dev))
    return (keep[:num_nodes] if raw_keep else keep[:num_nodes].bool()), info[:B], status


_MASK_INDEX_SCRATCH: dict = {}


def mask_index(mask: Tensor, declined: Optional[Tensor] = None, want_rank: bool = False, want_ones: bool = False,
               want_assign: bool = False, want_node_rank: bool = False):
    """The sorted positions of the non-zero bytes of ``mask`` [n] uint8 -- `mask.nonzero().view(-1)` in two launches with
    one pinned-word wait between them (torch's own: seven launches and a synchronising copy) -- as row 0 of an int64
    ``[2, k]`` array whose row 1 is ``arange(k)`` (``want_rank``; the indices of NDPSelect's S), plus ``ones [k]`` fp32
    (``want_ones``; its values).  ``declined`` (int32 [1] on the device): when non-zero the call returns None (the flag
    of the kernel that made the mask; read with the count, no copy of its own).  Returns (index [2,k] or [1,k], ones or
    None) -- and with ``want_assign`` (needs both) a third item: the one-to-one :class:`AssignIndex` (perm + packed
    {row, weight}) of the assignment these arrays describe, which :func:`one_to_one_index` would build in a launch of its
    own.  ``want_node_rank``: one more item, int32 ``[n + 1]`` = set positions in front of every position (total at
    ``[n]``): what :func:`kron_batched` takes as ``node_rank``.  reference: select/ndp_select.py:257-262."""
    dev = N.require_device(mask, declined)
    if mask.dtype != torch.uint8 or not mask.is_contiguous():
        raise ValueError("mask_index: a contiguous uint8 mask is required")
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("mask_index reads its count on the host between two launches: not capturable")
    n = mask.numel()
    L = N.lib()
    st = N.stream_ptr(dev)
    words = int(L.tgp_mask_index_scratch_words(n))
    key = (dev.index, st)
    scratch = _MASK_INDEX_SCRATCH.get(key)
    if scratch is None or scratch.numel() < words:
        scratch = torch.zeros(max(words, 1024), dtype=torch.int32, device=dev)
        _MASK_INDEX_SCRATCH[key] = scratch
    call = _sps_state(dev, st, 0).open_call()
    _checked(L.tgp_mask_index_count, N.ptr(mask), n, N.ptr(declined), N.ptr(scratch), *call.publish, st)
    k = call.count()
    if k < 0:
        return None
    rows = 2 if want_rank else 1
    index = torch.empty((rows, k), dtype=torch.long, device=dev)
    ones = torch.empty(k, dtype=torch.float32, device=dev) if want_ones else None
    assign = want_assign and want_rank and want_ones and 0 < k and n < (1 << 31)
    perm = torch.empty(k, dtype=torch.int32, device=dev) if assign else None
    pack = torch.empty(k, dtype=torch.int64, device=dev) if assign else None
    node_rank = torch.empty(n + 1, dtype=torch.int32, device=dev) if want_node_rank and n else None
    if k or node_rank is not None:
        _checked(L.tgp_mask_index_fill, N.ptr(mask), n, N.ptr(scratch), k, N.ptr(index) if k else None,
                 index.data_ptr() + 8 * k if want_rank and k else None, N.ptr(ones) if k else None, N.ptr(perm),
                 N.ptr(pack), N.ptr(node_rank), st)
    out = (index, ones)
    if want_assign:
        a_index = None
        if assign:
            a_index = AssignIndex(None, perm, k, k)
            a_index.pack, a_index.pack_key = pack, (index.data_ptr(), ones.data_ptr())
        out = out + (a_index,)
    if want_node_rank:
        out = out + (node_rank,)
    return out


def ndp_partition_large(indptr: Tensor, col: Tensor, weight: Optional[Tensor], p0: int, p1: int, seed: int,
                        keep: Tensor, status: Tensor, max_iter: int = 2000, tol: float = 1e-6,
                        steps_per_batch: int = 16, want_state: bool = False):
    """NDPSelect's spectral +-1 partition (select/ndp_select.py:187-256) of ONE large graph -- the nodes [p0, p1) of a
    symmetric, self-loop-free CSR -- on the whole chip: the LOBPCG iteration of :func:`ndp_partition` with grid-wide
    vector kernels (tgp_ndp_large_*).  Writes keep[p0:p1] (uint8 view of the caller's mask); returns the steps used
    (-1: the reference's random fallback).  One host read per ``steps_per_batch`` steps (the done flag)."""
    dev = N.require_device(indptr, col, weight, keep, status)
    if indptr.dtype != torch.int32 or keep.dtype != torch.uint8 or status.dtype != torch.int32:
        raise ValueError("ndp_partition_large: indptr / status must be int32, keep uint8")
    col = N.i64c(col)
    w = N.opt_f32_flat(weight)
    L = N.lib()
    n = p1 - p0
    ws = N.workspace(L.tgp_ndp_large_workspace_bytes(n), dev)
    st = N.stream_ptr(dev)
    _checked(L.tgp_ndp_large_start, N.ptr(indptr), N.ptr(col), N.ptr(w), p0, p1, max_iter, N.ptr(ws), ws.numel(),
             N.ptr(status), st)
    progress = torch.zeros(2, dtype=torch.int32, device=dev)
    done = False
    while not done:
        _checked(L.tgp_ndp_large_steps, N.ptr(indptr), N.ptr(col), N.ptr(w), p0, p1, steps_per_batch, float(tol),
                 N.ptr(ws), ws.numel(), N.ptr(progress), N.ptr(status), st)
        flag, it = progress.tolist()  # one round trip per batch of steps
        done = flag != 0 or it >= max_iter
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    _checked(L.tgp_ndp_large_finish, N.ptr(indptr), N.ptr(col), N.ptr(w), p0, p1, int(seed) & ((1 << 64) - 1),
             N.ptr(ws), ws.numel(), N.ptr(keep), N.ptr(info), st)
    if want_state:
        out = (ctypes.c_double * 5)()
        _checked(L.tgp_ndp_large_state, N.ptr(ws), n, ctypes.addressof(out), st)
        return info, {"lambda": out[0], "residual_sq": out[1], "steps": int(out[2]), "random": bool(out[3]),
                      "cut": out[4]}
    return info


# ------------------------------------------------------------------------- A9
def kron_max_graph_nodes() -> int:
    return int(N.lib().tgp_kron_batched_max_graph_nodes())


_KRON_CAPS: dict = {}


def _kron_caps(graph_sizes_host, limit: Optional[int] = None) -> Tuple[int, int, int]:
    """Workspace figures of the Kron kernels from the graphs' node counts: (sum of n^2 over the graphs inside the size
    limit of THIS call -- the kernels' own, or the smaller ``limit`` a caller declared: graphs beyond it are skipped by
    the kernel and get no slab --, sum of n (n | 1) over those beyond the LDS kernel's 128 nodes, how many those are).
    Vectorised and remembered per sizes list (r5: three Python passes over 2048 graphs were ~120 us of every NDP pooler
    call); the memo holds the list object and re-checks its length, its sum and the limit, so a list edited in place
    does not hand back stale figures."""
    import numpy as np
    lim = kron_max_graph_nodes() if limit is None else max(1, min(int(limit), kron_max_graph_nodes()))
    key = id(graph_sizes_host)
    hit = _KRON_CAPS.get(key)
    v = None
    if hit is not None and hit[0] is graph_sizes_host and hit[1] == len(graph_sizes_host) and hit[3] == lim:
        v = np.asarray(graph_sizes_host, dtype=np.int64)
        if int(v.sum()) == hit[4]:
            return hit[2]
    if v is None:
        v = np.asarray(graph_sizes_host, dtype=np.int64)
    total = int(v.sum())
    v = v[v <= lim]
    big = v[v > 128]
    caps = (int((v * v).sum()), int((big * (big | 1)).sum()), int(big.size))
    if len(_KRON_CAPS) > 16:
        _KRON_CAPS.clear()
    _KRON_CAPS[key] = (graph_sizes_host, len(graph_sizes_host), caps, lim, total)  # (holds the list: the id stays its own)
    return caps


def kron_batched(indptr: Tensor, col: Tensor, val: Optional[Tensor], perm: Optional[Tensor], from_adjacency: bool,
                 num_nodes: int, graph_ptr: Tensor, max_graph_nodes: int, node_index: Tensor,
                 threshold: float, skip_oversize: bool = False,
                 graph_sizes_host: Optional[Sequence[int]] = None,
                 node_rank: Optional[Tensor] = None) -> Optional[Tuple[Tensor, Tensor]]:
    """Block-batched Kron reduction (connect/kron_conn.py:117-165): one workgroup per graph, fp64 elimination of the
    dropped nodes, thresholded fp32 edge list in row-major order.  ``indptr`` int32 [N+1] / ``col`` int64 / ``val``
    fp32 or fp64 (None = ones) / ``perm`` int32 (None = identity) describe the Laplacian entries, or the edge weights
    when ``from_adjacency``.  ``graph_sizes_host``: the graphs' node counts on the host (the caller's memoised
    batch info): the workspace is then sized from the real graphs instead of num_nodes x longest graph.
    ``node_rank`` (int32 [num_nodes + 1], optional): kept nodes in front of every node, from the selector that compacted
    ``node_index`` itself (:func:`mask_index`): the call skips its flag scatter and scan.
    Returns None when the library declines (see include/tgp_hip.h)."""
    dev = N.require_device(indptr, col, val, perm, graph_ptr, node_index)
    cap_dense = cap_big = num_big = -1
    if graph_sizes_host is not None:
        cap_dense, cap_big, num_big = _kron_caps(graph_sizes_host, max_graph_nodes)
    if indptr.dtype != torch.int32 or (perm is not None and perm.dtype != torch.int32):
        raise ValueError("kron_batched: indptr / perm must be int32")
    col, graph_ptr, node_index = N.i64c(col), N.i64c(graph_ptr), N.i64c(node_index)
    v32 = v64 = None
    if val is not None:
        if val.dtype == torch.float64:
            v64 = val.contiguous()
        else:
            v32 = N.f32c(val.reshape(-1))
    B = graph_ptr.numel() - 1
    L = N.lib()
    if node_rank is not None and not (node_rank.dtype == torch.int32 and node_rank.numel() == num_nodes + 1
                                      and node_rank.is_contiguous() and node_rank.device == dev):
        node_rank = None  # (not the table of THIS batch: the call builds its own)
    st = N.stream_ptr(dev)
    got = _count_fill(
        dev, L.tgp_kron_batched_workspace_bytes(num_nodes, B, max_graph_nodes, cap_dense, cap_big),
        lambda ws, ws_bytes, cnt: _checked(
            L.tgp_kron_batched_count, N.ptr(indptr.contiguous()), N.ptr(col), N.ptr(v32), N.ptr(v64),
            N.ptr(None if perm is None else perm.contiguous()), (1 if from_adjacency else 0) | (2 if skip_oversize else 0),
            num_nodes, col.numel(), N.ptr(graph_ptr), B, max_graph_nodes, cap_dense, cap_big, num_big, N.ptr(node_index),
            node_index.numel(), float(threshold), N.ptr(node_rank), ws, ws_bytes, cnt, st),
        lambda ws, n_out, r, c, w: _checked(L.tgp_kron_batched_fill, ws, num_nodes, B, max_graph_nodes, cap_dense, cap_big,
                                            num_big, N.ptr(graph_ptr), n_out, r, c, w, N.ptr(node_rank), st),
        torch.float32, declines=True)
    return None if isinstance(got, int) else got


# ------------------------------------------------------------------------- A10
def block_diag_edges(adj_pool: Tensor, relabel: Optional[Tensor] = None,
                     remove_self_loops: bool = False) -> Tuple[Tensor, Tensor]:
    """dense_to_block_diag (utils/ops.py:53-82) with the optional valid-supernode renumbering of
    DenseSRCPooling._finalize_sparse_output (src.py:526-552)."""
    dev = N.require_device(adj_pool, relabel)
    f64 = adj_pool.dtype == torch.float64
    a = (N.f64c if f64 else N.f32c)(adj_pool if adj_pool.dim() == 3 else adj_pool.unsqueeze(0))
    B, K = a.size(0), a.size(1)
    rl = N.opt_i64(relabel)
    flags = N.REMOVE_SELF_LOOPS if remove_self_loops else 0
    L = N.lib()
    st = N.stream_ptr(dev)
    eps = ops_eps()
    count, fill = ((L.tgp_block_diag_count_f64, L.tgp_block_diag_fill_f64) if f64 else
                   (L.tgp_block_diag_count, L.tgp_block_diag_fill))
    return _count_fill(
        dev, L.tgp_block_diag_workspace_bytes(B, K),
        lambda ws, ws_bytes, cnt: _checked(count, N.ptr(a), B, K, N.ptr(rl), flags, eps, ws, ws_bytes, cnt, st),
        lambda ws, n_out, r, c, w: _checked(fill, N.ptr(a), B, K, N.ptr(rl), flags, eps, ws, n_out, r, c, w, st), a.dtype)


# ------------------------------------------------------------------------- A11
def to_dense_adj(edge_index: Tensor, edge_weight: Optional[Tensor], batch: Tensor, ptr: Tensor, num_graphs: int,
                 max_nodes: int, transposed: bool, zeroed_out: Optional[Tensor] = None) -> Tensor:
    """PyG to_dense_adj (src.py:434-443): [B,Nmax,Nmax], duplicates summed; optionally written transposed.
    ``zeroed_out``: a zero-filled [B,Nmax,Nmax] buffer to add into (:func:`to_dense_batch` can zero it in its launch)."""
    dev = N.require_device(edge_index, edge_weight, batch, ptr)
    row, col = _edge_rows(edge_index)
    w = N.opt_f32_flat(edge_weight)
    batch, ptr = N.i64c(batch), N.i64c(ptr)
    adj = zeroed_out if zeroed_out is not None else torch.empty(num_graphs, max_nodes, max_nodes, dtype=torch.float32,
                                                                device=dev)
    if tuple(adj.shape) != (num_graphs, max_nodes, max_nodes) or adj.dtype != torch.float32 or not adj.is_contiguous():
        raise ValueError("to_dense_adj: zeroed_out must be a contiguous float32 [B,Nmax,Nmax] tensor")
    _checked(N.lib().tgp_to_dense_adj_f32, N.ptr(row), N.ptr(col), N.ptr(w), row.numel(), N.ptr(batch), N.ptr(ptr),
             num_graphs, max_nodes, 1 if transposed else 0, 1 if zeroed_out is not None else 0, N.ptr(adj),
             N.stream_ptr(dev))
    return adj


def to_dense_adj_channels(edge_index: Tensor, edge_attr: Tensor, batch: Tensor, ptr: Tensor, num_graphs: int,
                          max_nodes: int, transposed: bool) -> Tensor:
    """PyG to_dense_adj with multi-channel edge attributes [E, C] (src.py:434): [B,Nmax,Nmax,C], duplicates summed."""
    dev = N.require_device(edge_index, edge_attr, batch, ptr)
    row, col = _edge_rows(edge_index)
    E = row.numel()
    a = N.f32c(edge_attr.reshape(E, -1))
    C = a.size(1)
    batch, ptr = N.i64c(batch), N.i64c(ptr)
    adj = torch.empty(num_graphs, max_nodes, max_nodes, C, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_to_dense_adj_channels_f32, N.ptr(row), N.ptr(col), N.ptr(a), E, C, N.ptr(batch), N.ptr(ptr),
             num_graphs, max_nodes, 1 if transposed else 0, N.ptr(adj), N.stream_ptr(dev))
    return adj.view((num_graphs, max_nodes, max_nodes) + tuple(edge_attr.shape[1:]))


def from_dense_adj(grad_adj: Tensor, edge_index: Tensor, batch: Tensor, ptr: Tensor, max_nodes: int,
                   transposed: bool) -> Tensor:
    """grad of :func:`to_dense_adj` w.r.t. the edge weights: one gather kernel."""
    dev = N.require_device(grad_adj, edge_index, batch, ptr)
    row, col = _edge_rows(edge_index)
    g = N.f32c(grad_adj)
    batch, ptr = N.i64c(batch), N.i64c(ptr)
    out = torch.empty(row.numel(), dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_from_dense_adj_f32, N.ptr(g), N.ptr(row), N.ptr(col), row.numel(), N.ptr(batch), N.ptr(ptr),
             g.size(0), max_nodes, 1 if transposed else 0, N.ptr(out), N.stream_ptr(dev))
    return out


def from_dense_batch(dense: Tensor, batch: Tensor, ptr: Tensor, max_nodes: int) -> Tensor:
    """[B,Nmax,F] -> [N,F]: the rows that to_dense_batch scattered, gathered back (its backward)."""
    dev = N.require_device(dense, batch, ptr)
    d = N.f32c(dense.reshape(dense.size(0), dense.size(1), -1))
    batch, ptr = N.i64c(batch), N.i64c(ptr)
    n, F = batch.numel(), d.size(2)
    out = torch.empty(n, F, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_from_dense_batch_f32, N.ptr(d), n, F, N.ptr(batch), N.ptr(ptr), d.size(0), max_nodes,
             N.ptr(out), N.stream_ptr(dev))
    return out.view((n,) + tuple(dense.shape[2:]))


def to_dense_batch(x: Tensor, batch: Tensor, ptr: Tensor, num_graphs: int, max_nodes: int,
                   also_zero: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """PyG to_dense_batch (src.py:448-450): ([B,Nmax,F], mask [B,Nmax]).  ``also_zero``: a contiguous float32 buffer to
    zero-fill on the way (in the same launch when the batch vector is sorted)."""
    dev = N.require_device(x, batch, ptr)
    x2 = N.f32c(x if x.dim() == 2 else x.reshape(x.size(0), -1))
    batch, ptr = N.i64c(batch), N.i64c(ptr)
    F = x2.size(1)
    out = torch.empty(num_graphs, max_nodes, F, dtype=torch.float32, device=dev)
    mask = torch.empty(num_graphs, max_nodes, dtype=torch.bool, device=dev)
    from .utils.ops import batch_info
    if F > 0 and ptr.numel() == num_graphs + 1 and batch_info(batch).is_sorted:
        # sorted batch vector (memoised fact): one output-parallel kernel writes rows, padding and mask -- no memsets
        _checked(N.lib().tgp_to_dense_batch_sorted_f32, N.ptr(x2), x2.size(0), F, N.ptr(ptr), num_graphs, max_nodes,
                 N.ptr(out), N.ptr(mask), N.ptr(also_zero), also_zero.numel() if also_zero is not None else 0,
                 N.stream_ptr(dev))
        return out.view((num_graphs, max_nodes) + tuple(x.shape[1:])), mask
    if also_zero is not None:
        also_zero.zero_()
    _checked(N.lib().tgp_to_dense_batch_f32, N.ptr(x2), x2.size(0), F, N.ptr(batch), N.ptr(ptr), num_graphs, max_nodes,
             N.ptr(out), N.ptr(mask), N.stream_ptr(dev))
    return out.view((num_graphs, max_nodes) + tuple(x.shape[1:])), mask


# ------------------------------------------------------------------------- LaPool's selector (csrc/lapool.hip)
class LaPoolLeaders:
    """The leaders of one batch: ``flags`` (bool, the batch's shape without the feature axis), ``col_of`` int32 [rows]
    (a leader's column inside its graph, -1 otherwise), ``leaders`` int32 [rows] (graph b's leader rows, ascending,
    stored from the graph's first row on), ``k`` int32 [B] and ``k_max`` = max_b k_b.  Reading ``k_max`` is the
    selector's one host wait.  The layout rides along: padded (``ptr`` None, ``N`` rows per graph, ``mask`` bytes or
    None) or un-padded (``ptr`` [B + 1], ``batch`` [rows] or None with one graph)."""
    __slots__ = ("flags", "col_of", "leaders", "k", "_k_max_dev", "_k_max", "rows", "B", "N", "mask", "ptr", "batch")

    @property
    def k_max(self) -> int:
        if self._k_max is None:
            self._k_max = _read_count(self._k_max_dev)
        return self._k_max


def _lapool_dense_args(x: Tensor, adj: Optional[Tensor], mask: Optional[Tensor]):
    if x.dim() != 3:
        raise ValueError(f"x must be [B, N, F], got {tuple(x.shape)}")
    B, Nn = x.size(0), x.size(1)
    if adj is not None and tuple(adj.shape) != (B, Nn, Nn):
        raise ValueError(f"adj {tuple(adj.shape)} does not match x {tuple(x.shape)}")
    return B, Nn, _mask_bytes(mask, B, Nn)


def lapool_edge_group(edge_index: Tensor, num_nodes: int) -> AssignIndex:
    """The edge positions grouped by source, edge-list order inside a node: the order every sum of the edge form adds in
    (an empty list has an index of zeros: nothing to build).  Two routes: a list whose sources ascend needs only its
    CSR offsets (``perm`` None); any other list gets the by-source index, whose build sorts (a fixed 8 MB scratch).  A
    stable sort by source keeps each node's order, so both routes add the same numbers in the same order."""
    if edge_index.size(1) == 0:
        dev = edge_index.device
        return AssignIndex(torch.zeros(num_nodes + 1, dtype=torch.int32, device=dev),
                           torch.zeros(1, dtype=torch.int32, device=dev), 0, num_nodes)
    row, _ = _edge_rows(edge_index)
    if _rows_sorted(edge_index, row):
        # the usual layout: the offsets are the whole index (perm None = identity), one launch and no sort workspace
        return AssignIndex(csr_offsets(edge_index, num_nodes), None, edge_index.size(1), num_nodes)
    return edge_group(edge_index, num_nodes)


def _lapool_by_src(edge_index: Tensor, num_nodes: int, by_src: Optional[AssignIndex]) -> AssignIndex:
    if by_src is None:
        by_src = lapool_edge_group(edge_index, num_nodes)
    if by_src.num_targets != num_nodes or by_src.nnz != edge_index.size(1):
        raise ValueError("the by-source index does not belong to this edge list")
    return by_src


def lapool_variation(x: Tensor, adj: Optional[Tensor] = None, mask: Optional[Tensor] = None, *,
                     edge_index: Optional[Tensor] = None, edge_weight: Optional[Tensor] = None,
                     by_src: Optional[AssignIndex] = None) -> Tensor:
    """v_i = ||deg_i x_i - sum_j a_ij x_j||_2 (select/lapool_select.py:229-233, 366-376).  Padded form: ``x`` [B,N,F],
    ``adj`` [B,N,N], ``mask`` [B,N] -> [B,N], one pass over ``adj``, padded rows and columns count as zero.  Edge form:
    ``x`` [n,F], ``edge_index`` [2,E] (+ ``edge_weight``, + its by-source index) -> [n]; self-loops are dropped and
    duplicates add, in edge-list order."""
    if (adj is None) == (edge_index is None):
        raise ValueError("lapool_variation takes either a padded adjacency or an edge list")
    dev = N.require_device(x, adj, mask, edge_index, edge_weight)
    x, st = N.f32c(x), N.stream_ptr(dev)
    if adj is not None:
        B, Nn, mb = _lapool_dense_args(x, adj, mask)
        a = N.f32c(adj)
        v = torch.empty(B, Nn, dtype=torch.float32, device=dev)
        _checked(N.lib().tgp_lapool_variation_dense_f32, N.ptr(a), N.ptr(x), B, Nn, x.size(2), N.ptr(mb), N.ptr(v), st)
        return v
    if x.dim() != 2:
        raise ValueError(f"x must be [n, F], got {tuple(x.shape)}")
    n, E = x.size(0), edge_index.size(1)
    v = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return v
    _, col = _edge_rows(edge_index)
    w = N.opt_f32_flat(edge_weight)
    if w is not None and w.numel() != E:
        raise ValueError("lapool_variation: one weight per edge")
    grp = _lapool_by_src(edge_index, n, by_src)
    _checked(N.lib().tgp_lapool_variation_csr_f32, *grp.walk(col, E), N.ptr(w), N.ptr(x), n, E, x.size(1), N.ptr(v), st)
    return v


def lapool_columns(flags: Tensor, mask: Optional[Tensor] = None, batch: Optional[Tensor] = None,
                   ptr: Optional[Tensor] = None, fallback: bool = False) -> LaPoolLeaders:
    """Columns for a given leader mask: ``flags`` [B,N] (padded, with ``mask``) or [n] (un-padded, with the sorted
    ``batch`` and its offsets ``ptr``, both None for one graph).  ``fallback``: a graph with a real node and no leader
    makes all its real nodes leaders.  Padded rows never lead."""
    dev = N.require_device(flags, mask, batch, ptr)
    f = (flags if flags.dtype == torch.bool else flags != 0).contiguous().clone().view(torch.uint8)
    res = LaPoolLeaders()
    if f.dim() == 2:
        B, Nn = f.shape
        res.mask, res.ptr, res.batch = _mask_bytes(mask, B, Nn), None, None
    elif f.dim() == 1:
        if mask is not None:
            raise ValueError("a mask belongs to a padded batch")
        if (batch is None) != (ptr is None):
            raise ValueError("an un-padded batch gives its batch vector and its offsets together")
        Nn = 0
        if batch is None:
            ptr = torch.tensor([0, f.numel()], dtype=torch.int64, device=dev)
        elif batch.numel() != f.numel():
            raise ValueError("one batch entry per node")
        res.mask, res.ptr, res.batch = None, N.i64c(ptr), N.opt_i64(batch)
        B = res.ptr.numel() - 1
    else:
        raise ValueError(f"flags must be [B, N] or [n], got {tuple(flags.shape)}")
    rows = f.numel()
    res.rows, res.B, res.N, res._k_max = rows, B, Nn, None
    res.col_of = torch.empty(rows, dtype=torch.int32, device=dev)
    res.leaders = torch.empty(rows, dtype=torch.int32, device=dev)
    res.k = torch.empty(B, dtype=torch.int32, device=dev)
    res._k_max_dev = torch.empty(1, dtype=torch.int64, device=dev)
    _checked(N.lib().tgp_lapool_columns, N.ptr(f) if rows else None, rows, B, Nn, N.ptr(res.mask), N.ptr(res.ptr),
             int(bool(fallback)), N.ptr(res.col_of), N.ptr(res.leaders), N.ptr(res.k), N.ptr(res._k_max_dev),
             N.stream_ptr(dev))
    res.flags = f.view(torch.bool)
    return res


def lapool_leaders(v: Tensor, adj: Optional[Tensor] = None, mask: Optional[Tensor] = None, *,
                   edge_index: Optional[Tensor] = None, by_src: Optional[AssignIndex] = None,
                   batch: Optional[Tensor] = None, ptr: Optional[Tensor] = None) -> LaPoolLeaders:
    """leader_i = v_i >= v_j for every neighbour j (select/lapool_select.py:235-242, 378-388), then the fall-back of a
    graph without a leader and the leaders' columns, all on the device.  Padded form: a second pass over ``adj``,
    neighbours are the nonzero entries on real columns.  Edge form: the entries left after self-loop removal, explicit
    zero weights included.  (The reference's "every Laplacian weight is zero" branch needs no code: v is 0 everywhere
    then and every comparison holds.)"""
    if (adj is None) == (edge_index is None):
        raise ValueError("lapool_leaders takes either a padded adjacency or an edge list")
    dev = N.require_device(v, adj, mask, edge_index, batch, ptr)
    v, st = N.f32c(v), N.stream_ptr(dev)
    flags = torch.empty(v.shape, dtype=torch.uint8, device=dev)
    if adj is not None:
        if v.dim() != 2 or tuple(adj.shape) != (v.size(0), v.size(1), v.size(1)):
            raise ValueError(f"adj {tuple(adj.shape)} does not match v {tuple(v.shape)}")
        B, Nn = v.shape
        _checked(N.lib().tgp_lapool_flags_dense_f32, N.ptr(N.f32c(adj)), N.ptr(v), B, Nn,
                 N.ptr(_mask_bytes(mask, B, Nn)), N.ptr(flags), st)
        return lapool_columns(flags, mask=mask, fallback=True)
    if v.dim() != 1:
        raise ValueError(f"v must be [n], got {tuple(v.shape)}")
    n, E = v.numel(), edge_index.size(1)
    if n:
        _, col = _edge_rows(edge_index)
        grp = _lapool_by_src(edge_index, n, by_src)
        _checked(N.lib().tgp_lapool_flags_csr_f32, *grp.walk(col, E), N.ptr(v), n, E, N.ptr(flags), st)
    return lapool_columns(flags, batch=batch, ptr=ptr, fallback=True)


def _lapool_rows(x: Tensor, lead: LaPoolLeaders) -> Tensor:
    x = N.f32c(x)
    if x.numel() // max(x.size(-1), 1) != lead.rows or (x.dim() == 3) != (lead.ptr is None):
        raise ValueError(f"x {tuple(x.shape)} does not match the leaders' batch of {lead.rows} rows")
    return x


def lapool_assign(x: Tensor, lead: LaPoolLeaders) -> Tuple[Tensor, Tensor]:
    """(S, row norms): per graph the softmax over the cosine similarities to that graph's own leaders
    (select/lapool_select.py:26-76, 274-311), leader rows one-hot, padded rows and the columns from k_b on zero.
    S is [B,N,K_max] for a padded batch and [n,K_max] otherwise; nothing of size N_total x K_total is formed."""
    dev = N.require_device(x, lead.col_of)
    x = _lapool_rows(x, lead)
    Kc, F = lead.k_max, x.size(-1)
    s = torch.empty(tuple(x.shape[:-1]) + (Kc,), dtype=torch.float32, device=dev)
    nrm = torch.empty(lead.rows, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_lapool_assign_f32, N.ptr(x), lead.rows, F, lead.B, lead.N, N.ptr(lead.mask), N.ptr(lead.ptr),
             N.ptr(lead.batch), N.ptr(lead.col_of), N.ptr(lead.leaders), N.ptr(lead.k), Kc, ops_eps(), N.ptr(nrm),
             N.ptr(s) if s.numel() else None, N.stream_ptr(dev))
    return s, nrm


def lapool_assign_bwd(x: Tensor, nrm: Tensor, s: Tensor, ds: Tensor, lead: LaPoolLeaders) -> Tensor:
    """dX of `lapool_assign`: through the softmax and the cosine, to a row itself and to the leaders it was compared
    with; leader and padded rows of ``ds`` pass nothing.  Work buffers: two [rows, K_max] and one [rows]."""
    dev = N.require_device(x, nrm, s, ds)
    x, s, ds = _lapool_rows(x, lead), N.f32c(s), N.f32c(ds)
    if s.shape != ds.shape or s.shape[:-1] != x.shape[:-1]:
        raise ValueError(f"s {tuple(s.shape)}, ds {tuple(ds.shape)} and x {tuple(x.shape)} do not match")
    Kc = s.size(-1)
    dx = torch.empty_like(x)
    g = torch.empty(2, lead.rows, max(Kc, 1), dtype=torch.float32, device=dev)
    alpha = torch.empty(max(lead.rows, 1), dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_lapool_assign_bwd_f32, N.ptr(x), N.ptr(nrm), N.ptr(s) if Kc else None,
             N.ptr(ds) if Kc else None, lead.rows, x.size(-1), lead.B, lead.N, N.ptr(lead.mask), N.ptr(lead.ptr),
             N.ptr(lead.batch), N.ptr(lead.col_of), N.ptr(lead.leaders), N.ptr(lead.k), Kc, ops_eps(), N.ptr(g[0]),
             N.ptr(g[1]), N.ptr(alpha), N.ptr(dx) if dx.numel() else None, N.stream_ptr(dev))
    return dx


# ------------------------------------------------------------------------- SAGPooling's scorer (csrc/sag_score.hip)
_SAG_GROUPS = TensorMemo(16)  # edge_index -> {(num_nodes, by_destination): AssignIndex}


def row_project2(x: Tensor, w0: Tensor, w1: Tensor) -> Tuple[Tensor, Tensor]:
    """(x w0, x w1): both dot products of every row from one pass over ``x`` [N,F] (any row stride)."""
    dev = N.require_device(x, w0, w1)
    x, ld = _row_operand(x, "row_project2", convert=True)
    w0, w1 = N.f32c(w0.reshape(-1)), N.f32c(w1.reshape(-1))
    if w0.numel() != x.size(1) or w1.numel() != x.size(1):
        raise ValueError(f"row_project2: x {tuple(x.shape)} against weights of {w0.numel()} and {w1.numel()} entries")
    out = torch.empty(2, x.size(0), dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_row_project2_f32, N.ptr(x), x.size(0), x.size(1), ld, N.ptr(w0), N.ptr(w1), N.ptr(out[0]),
             N.ptr(out[1]), N.stream_ptr(dev))
    return out[0], out[1]


def sag_edge_group(edge_index: Tensor, num_nodes: int, by_destination: bool = True) -> AssignIndex:
    """The index the scorer's sums run over: edge positions grouped by destination (forward) or by source (backward),
    edge-list order inside a node.  A list that already ascends in that row needs only its CSR offsets (``perm`` None);
    any other list gets the stable sort of :func:`edge_group`, so both routes add the same numbers in the same order.
    Remembered per tensor object and version: full-batch training scores the same ``edge_index`` every step."""
    key = (int(num_nodes), bool(by_destination))
    memo = _SAG_GROUPS.get(edge_index)
    if memo is not None and key in memo:
        return memo[key]
    dev, E = edge_index.device, edge_index.size(1)
    if E == 0:
        grp = AssignIndex(torch.zeros(num_nodes + 1, dtype=torch.int32, device=dev), None, 0, num_nodes)
    else:
        row, col = _edge_rows(edge_index)
        tgt = col if by_destination else row
        ascending = bool((col[1:] >= col[:-1]).all()) if by_destination else _rows_sorted(edge_index, row)
        if ascending:
            ptr = torch.empty(num_nodes + 1, dtype=torch.int32, device=dev)
            rowptr_from_sorted(tgt, num_nodes, ptr)
            grp = AssignIndex(ptr, None, E, num_nodes)
        else:
            grp = edge_group(edge_index, num_nodes, by_destination=by_destination)
    if not torch.cuda.is_current_stream_capturing():
        if memo is None:
            memo = {}
            _SAG_GROUPS.put(edge_index, memo)
        memo[key] = grp
    return grp


def sag_aggregate(grp: AssignIndex, src: Tensor, p: Tensor, q: Optional[Tensor] = None, bias: Optional[Tensor] = None,
                  mean: bool = False, tanh: bool = False, want_t: bool = False):
    """a = act((sum over node i's group of p[src] [/ max(group size, 1)] + bias) + q_i), act = tanh or identity, the sum in
    the order of ``grp`` (no float atomics).  ``want_t``: ``(t, a)`` with the pre-activation as well."""
    dev = N.require_device(src, p, q, bias, grp.row_ptr)
    p, src = N.f32c(p.reshape(-1)), N.i64c(src)
    n, E = grp.num_targets, src.numel()
    if p.numel() != n or grp.nnz != E or grp.row_ptr.numel() != n + 1 or (q is not None and q.numel() != n):
        raise ValueError(f"sag_aggregate: {n} nodes and {grp.nnz} indexed edges against p {tuple(p.shape)}, "
                         f"{E} edges" + ("" if q is None else f", q {tuple(q.shape)}"))
    q = N.opt_f32_flat(q)
    b = N.opt_f32_flat(bias)
    out = torch.empty(2 if want_t else 1, n, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_sag_aggregate_f32, *grp.walk(src, E), N.ptr(p), N.ptr(q), N.ptr(b), n, E, int(bool(mean)),
             int(bool(tanh)), N.ptr(out[0]) if want_t else None, N.ptr(out[-1]), N.stream_ptr(dev))
    return (out[0], out[1]) if want_t else out[0]


def sag_score_bwd_x(g_q: Tensor, g_p: Tensor, w_root: Tensor, w_rel: Tensor, g_x: Optional[Tensor] = None) -> Tensor:
    """dX = g_q (x) w_root + g_p (x) w_rel in one pass, added to ``g_x`` ([N,F] float32 contiguous, in place) when given."""
    dev = N.require_device(g_q, g_p, w_root, w_rel, g_x)
    g_q, g_p = N.f32c(g_q.reshape(-1)), N.f32c(g_p.reshape(-1))
    w_root, w_rel = N.f32c(w_root.reshape(-1)), N.f32c(w_rel.reshape(-1))
    n, F = g_q.numel(), w_root.numel()
    if g_p.numel() != n or w_rel.numel() != F:
        raise ValueError("sag_score_bwd_x: one g_q and g_p per node, one w_root and w_rel per column")
    acc = g_x is not None
    if acc and (g_x.dtype != torch.float32 or tuple(g_x.shape) != (n, F) or not g_x.is_contiguous()):
        raise ValueError(f"sag_score_bwd_x: g_x must be a contiguous float32 [{n}, {F}]")
    out = g_x if acc else torch.empty(n, F, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_sag_score_bwd_x_f32, N.ptr(g_q), N.ptr(g_p), N.ptr(w_root), N.ptr(w_rel), n, F, int(acc),
             N.ptr(out), N.stream_ptr(dev))
    return out


def sag_score(x: Tensor, edge_index: Tensor, w_rel: Tensor, w_root: Optional[Tensor], bias: Optional[Tensor],
              mean: bool = False, tanh: bool = False, want_t: bool = False):
    """The whole scorer, two launches: act(lin_rel(aggr_j x_j) + lin_root(x_i)) at one output channel as
    project-then-aggregate.  ``w_root`` None (SAGEConv with ``root_weight=False``): no root term."""
    p, q = row_project2(x, w_rel, w_rel if w_root is None else w_root)
    row, _ = _edge_rows(edge_index)
    grp = sag_edge_group(edge_index, x.size(0), by_destination=True)
    return sag_aggregate(grp, row, p, None if w_root is None else q, bias, mean, tanh, want_t)


# ------------------------------------------------------------------------- ASAPooling's fitness (csrc/asap.hip)
ASAP_ACTS = {"identity": 0, "tanh": 1, "sigmoid": 2}


def _asap_group(name: str, grp: AssignIndex, src: Tensor) -> Tuple[Tensor, int, int]:
    src = N.i64c(src)
    n, E = grp.num_targets, src.numel()
    if grp.nnz != E or grp.row_ptr.numel() != n + 1:
        raise ValueError(f"{name}: an index of {grp.nnz} edges over {n} nodes against {E} edges")
    return src, n, E


def asap_query(grp: AssignIndex, src: Tensor, x_pool: Tensor, w_tilde: Tensor, c: Tensor, want_arg: bool = False):
    """sq[i] = <max over node i's group of x_pool[src], w_tilde> + c (c: one device float).  A NaN among a column's
    candidates gives NaN, as ``torch.amax`` does; a node without in-edges gives c.  ``want_arg``: ``(sq, argpos)`` with
    the int32 [n, F] edge positions of the maxima (lowest position on a tie, -1 for a node without in-edges)."""
    dev = N.require_device(src, x_pool, w_tilde, c, grp.row_ptr)
    src, n, E = _asap_group("asap_query", grp, src)
    x_pool, ld = _row_operand(x_pool, "asap_query", convert=True)
    w_tilde, c = N.f32c(w_tilde.reshape(-1)), N.f32c(c.reshape(-1))
    if x_pool.size(0) != n or w_tilde.numel() != x_pool.size(1) or c.numel() != 1:
        raise ValueError(f"asap_query: x_pool {tuple(x_pool.shape)} against {n} nodes, w_tilde of {w_tilde.numel()} and "
                         f"c of {c.numel()} entries")
    sq = torch.empty(n, dtype=torch.float32, device=dev)
    arg = torch.empty(n, x_pool.size(1), dtype=torch.int32, device=dev) if want_arg else None
    _checked(N.lib().tgp_asap_query_f32, *grp.walk(src, E), N.ptr(x_pool), ld, N.ptr(w_tilde), N.ptr(c), n, E,
             x_pool.size(1), N.ptr(sq), N.ptr(arg), N.stream_ptr(dev))
    return (sq, arg) if want_arg else sq


def asap_edge_dot(grp: AssignIndex, src: Tensor, g: Tensor, x: Tensor) -> Tensor:
    """out[pos] = <g[i], x[src[pos]]> for every edge of node i's group: the gradient of the attend kernel's ``val``."""
    dev = N.require_device(src, g, x, grp.row_ptr)
    src, n, E = _asap_group("asap_edge_dot", grp, src)
    g, (x, ld) = N.f32c(g), _row_operand(x, "asap_edge_dot", convert=True)
    if g.dim() != 2 or g.size(0) != n or x.size(0) != n or g.size(1) != x.size(1):
        raise ValueError(f"asap_edge_dot: g {tuple(g.shape)} and x {tuple(x.shape)} against {n} nodes")
    out = torch.empty(E, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_asap_edge_dot_f32, *grp.walk(src, E), N.ptr(g), N.ptr(x), ld, n, E, x.size(1),
             N.ptr(out) if E else None, N.stream_ptr(dev))
    return out


def asap_softmax_bwd(grp: AssignIndex, src: Tensor, alpha: Tensor, g_alpha: Tensor, sq: Tensor, sp: Tensor,
                     negative_slope: float) -> Tuple[Tensor, Tensor]:
    """(g_l [E], g_sq [n]): the backward of :func:`asap_edge_softmax` through the softmax and the leaky ReLU."""
    dev = N.require_device(src, alpha, g_alpha, sq, sp, grp.row_ptr)
    src, n, E = _asap_group("asap_softmax_bwd", grp, src)
    alpha, g_alpha = N.f32c(alpha.reshape(-1)), N.f32c(g_alpha.reshape(-1))
    sq, sp = N.f32c(sq.reshape(-1)), N.f32c(sp.reshape(-1))
    if alpha.numel() != E or g_alpha.numel() != E or sq.numel() != n or sp.numel() != n:
        raise ValueError(f"asap_softmax_bwd: alpha and g_alpha per edge ({E}), sq and sp per node ({n})")
    g_l = torch.empty(E, dtype=torch.float32, device=dev)
    g_sq = torch.empty(n, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_asap_softmax_bwd_f32, *grp.walk(src, E), N.ptr(alpha) if E else None,
             N.ptr(g_alpha) if E else None, N.ptr(sq), N.ptr(sp), n, E, float(negative_slope),
             N.ptr(g_l) if E else None, N.ptr(g_sq), N.stream_ptr(dev))
    return g_l, g_sq


def asap_query_bwd(by_src: AssignIndex, dst: Tensor, argpos: Tensor, g_sq: Tensor, w_tilde: Tensor) -> Tensor:
    """g_x_pool [n, F] of :func:`asap_query`: row j collects ``g_sq[dst] * w_tilde[f]`` from the out-edges of j whose
    position is the arg-max of (dst, f).  ``by_src`` is the by-source group, ``dst`` the destination row."""
    dev = N.require_device(dst, argpos, g_sq, w_tilde, by_src.row_ptr)
    dst, n, E = _asap_group("asap_query_bwd", by_src, dst)
    g_sq, w_tilde = N.f32c(g_sq.reshape(-1)), N.f32c(w_tilde.reshape(-1))
    F = w_tilde.numel()
    if argpos.dtype != torch.int32 or tuple(argpos.shape) != (n, F) or not argpos.is_contiguous() or g_sq.numel() != n:
        raise ValueError(f"asap_query_bwd: argpos must be a contiguous int32 [{n}, {F}], g_sq [{n}]")
    out = torch.empty(n, F, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_asap_query_bwd_f32, *by_src.walk(dst, E), N.ptr(argpos), N.ptr(g_sq), N.ptr(w_tilde), n, E, F,
             N.ptr(out), N.stream_ptr(dev))
    return out


def asap_edge_softmax(grp: AssignIndex, src: Tensor, sq: Tensor, sp: Tensor, negative_slope: float) -> Tensor:
    """alpha [E]: the softmax of leaky_relu(sq[dst] + sp[src]) over every node's group (``+ 1e-16`` in the denominator),
    at the edges' own positions."""
    dev = N.require_device(src, sq, sp, grp.row_ptr)
    src, n, E = _asap_group("asap_edge_softmax", grp, src)
    sq, sp = N.f32c(sq.reshape(-1)), N.f32c(sp.reshape(-1))
    if sq.numel() != n or sp.numel() != n:
        raise ValueError(f"asap_edge_softmax: one sq and one sp per node ({n}), got {sq.numel()} and {sp.numel()}")
    alpha = torch.empty(E, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_asap_edge_softmax_f32, *grp.walk(src, E), N.ptr(sq), N.ptr(sp), n, E, float(negative_slope),
             N.ptr(alpha) if E else None, N.stream_ptr(dev))
    return alpha


def asap_attend(grp: AssignIndex, src: Tensor, x: Tensor, val: Optional[Tensor] = None,
                proj: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor]]:
    """(out [n, F], p [3, n] or None): out[i] = sum over node i's group of val[pos] x[src] (``val`` None: 1), one row
    gather per edge; with ``proj`` [3, F] also the three projections of every finished row."""
    dev = N.require_device(src, x, val, proj, grp.row_ptr)
    src, n, E = _asap_group("asap_attend", grp, src)
    x, ld = _row_operand(x, "asap_attend", convert=True)
    F = x.size(1)
    val = N.opt_f32_flat(val)
    proj = N.opt_f32(proj)
    if (val is not None and val.numel() != E) or (proj is not None and tuple(proj.shape) != (3, F)):
        raise ValueError(f"asap_attend: one value per edge ({E}) and projections [3, {F}]")
    out = torch.empty(n, F, dtype=torch.float32, device=dev)
    p = None if proj is None else torch.empty(3, n, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_asap_attend_f32, *grp.walk(src, E), N.ptr(val), N.ptr(x), ld, N.ptr(proj), n, x.size(0), E, F,
             N.ptr(out), N.ptr(p), N.stream_ptr(dev))
    return out, p


def asap_leconv(grp: AssignIndex, src: Tensor, p: Tensor, edge_weight: Optional[Tensor] = None,
                b1: Optional[Tensor] = None, b3: Optional[Tensor] = None, act: str = "identity",
                want_t: bool = False):
    """a = act(((p3 + b3) + sum_e w_e p1[src_e]) + (b1 - p2) sum_e w_e) over every node's group in its order; ``p`` is
    [3, n].  ``want_t``: ``(t, a)`` with the pre-activation as well."""
    if act not in ASAP_ACTS:
        raise ValueError(f"asap_leconv: act {act!r} is not one of {sorted(ASAP_ACTS)}")
    dev = N.require_device(src, p, edge_weight, b1, b3, grp.row_ptr)
    src, n, E = _asap_group("asap_leconv", grp, src)
    p = N.f32c(p)
    ew = N.opt_f32_flat(edge_weight)
    if tuple(p.shape) != (3, n) or (ew is not None and ew.numel() != E):
        raise ValueError(f"asap_leconv: p must be [3, {n}] and edge_weight [{E}]")
    b1 = N.opt_f32_flat(b1)
    b3 = N.opt_f32_flat(b3)
    out = torch.empty(2 if want_t else 1, n, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_asap_leconv_f32, *grp.walk(src, E), N.ptr(ew), N.ptr(p), N.ptr(b1), N.ptr(b3), n, E,
             ASAP_ACTS[act], N.ptr(out[0]) if want_t else None, N.ptr(out[-1]), N.stream_ptr(dev))
    return (out[0], out[1]) if want_t else out[0]


# ------------------------------------------------------------------------- segment readout (csrc/segment_aggr.hip)
SEGMENT_OPS = ("sum", "mean", "min", "max")  # the order of their enum values = the order of the output's column blocks


def segment_ops_mask(ops: Sequence[str]) -> int:
    mask = 0
    for op in ops:
        if op not in SEGMENT_OPS:
            raise ValueError(f"segment readout: unknown operation {op!r}")
        mask |= 1 << N.REDUCE_OPS[op]
    if mask == 0:
        raise ValueError("segment readout: no operation requested")
    return mask


def segment_aggr_chunk_rows() -> int:
    """Rows of the longest segment the readout still adds in one chain; one more row takes the split route."""
    return int(N.lib().tgp_segment_aggr_chunk_rows())


def segment_aggr(x: Tensor, ops_mask: int, num_groups: int, max_len: int, ptr: Optional[Tensor] = None,
                 dense_nodes: int = 0, mask: Optional[Tensor] = None, index: Optional[AssignIndex] = None,
                 node_index: Optional[Tensor] = None, weight: Optional[Tensor] = None, want_aux: bool = False):
    """One pass over ``x`` [rows, F] -> out [G, n_ops * F] (column blocks in ``SEGMENT_OPS`` order), plus with
    ``want_aux`` the tie counts of min / max and the group sizes the backward reads.  Row source: ``ptr`` [G + 1]
    (contiguous segments), ``dense_nodes`` (+ ``mask`` [rows] bytes), or ``index`` + ``node_index`` (+ ``weight``):
    the rows of a sparse assignment (reduce/aggr_reduce.py:99-103 without the [nnz, F] product)."""
    dev = N.require_device(x, ptr, mask, node_index, weight)
    x, ld = _row_operand(x, "segment readout")
    ptr = N.opt_i64(ptr)
    node_index = N.opt_i64(node_index)
    weight = N.opt_f32_flat(weight)
    mask = None if mask is None else mask.reshape(-1).contiguous()
    if index is not None and (node_index is None or node_index.numel() != index.nnz
                              or (weight is not None and weight.numel() != index.nnz)):
        raise ValueError("segment readout: node_index and weight hold one entry per assignment of the index")
    rows, F = x.shape
    n_ops = bin(ops_mask).count("1")
    n_mm = bin(ops_mask & ((1 << N.REDUCE_OPS["min"]) | (1 << N.REDUCE_OPS["max"]))).count("1")
    out = torch.empty(num_groups, n_ops * F, dtype=torch.float32, device=dev)
    ties = torch.empty(num_groups, n_mm * F, dtype=torch.int32, device=dev) if want_aux and n_mm else None
    count = torch.empty(num_groups, dtype=torch.int32, device=dev) if want_aux else None
    L = N.lib()
    wsb = L.tgp_segment_aggr_workspace_bytes(num_groups, F, ops_mask, max_len)
    ws = N.workspace(wsb, dev) if wsb else None
    gathered = index is not None
    _checked(L.tgp_segment_aggr_f32, N.ptr(x), rows, F, ld, N.ptr(ptr), dense_nodes, N.ptr(mask),
             N.ptr(index._row_ptr) if gathered else None, N.ptr(index.perm) if gathered else None, N.ptr(node_index),
             N.ptr(weight), index.nnz if gathered else 0, num_groups, max_len, ops_mask, N.ptr(out), N.ptr(ties),
             N.ptr(count), N.ptr(ws), wsb, N.stream_ptr(dev))
    return out, ties, count


def segment_aggr_bwd(g_out: Tensor, x: Tensor, out: Tensor, ties: Optional[Tensor], count: Tensor, ops_mask: int,
                     num_groups: int, batch: Optional[Tensor] = None, dense_nodes: int = 0,
                     mask: Optional[Tensor] = None) -> Tensor:
    """dX [rows, F] of :func:`segment_aggr` for the contiguous and the dense sources, one launch, written once."""
    dev = N.require_device(g_out, x, out, batch, mask)
    g_out, (x, ld) = N.f32c(g_out), _row_operand(x, "segment readout")
    rows, F = x.shape
    dx = torch.empty(rows, F, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_segment_aggr_bwd_f32, N.ptr(g_out), N.ptr(x), rows, F, ld, N.ptr(batch), dense_nodes,
             N.ptr(mask), N.ptr(out), N.ptr(ties), N.ptr(count), num_groups, ops_mask, N.ptr(dx), N.stream_ptr(dev))
    return dx


# ------------------------------------------------------------------------- MaxCutPooling (csrc/maxcut.hip)
MAXCUT_ACTS = {"identity": 0, "tanh": 1, "relu": 2}
MAXCUT_ASSIGN_MAX_GROUP = 4096  # in-edges of one destination above which the assignment takes the composed rounds: one
#                                  wave walks a group once per DISTINCT label among its sources (length x labels / 64 steps)
MAXCUT_SCORE_MAX_GROUP = 4096  # the score net takes the composed form when the longest by-destination group exceeds this
MAXCUT_SCORE_GROUP_SHARE = 256  # ... and E / this: one wave adds a group's rows in every layer
_MAXCUT_NP = TensorMemo(16)  # edge_index -> one device int64: the list's largest endpoint + 1 (0 for an empty list)
_MAXCUT_NP_HOST = TensorMemo(16)  # edge_index -> the same number on the host (read once, for a call without a batch vector)
_MAXCUT_ONE_GRAPH_PTR: dict = {}  # (n, device) -> the offsets [0, n] of a single graph (the loss without a batch vector)


def maxcut_max_width() -> int:
    """The widest row the layer, tail and weight-gradient kernels take."""
    return int(N.lib().tgp_maxcut_max_width())


def maxcut_tail_max_params() -> int:
    return int(N.lib().tgp_maxcut_tail_max_params())


def maxcut_n_p(edge_index: Tensor) -> Tensor:
    """``n_P`` of the delta-GCN matrix as one device word: the reference infers the size of ``P`` from the list
    (``max(edge_index) + 1``), so nodes above every endpoint get no diagonal term.  One reduction, remembered per tensor
    object and version; the host never reads it."""
    got = _MAXCUT_NP.get(edge_index)
    if got is None:
        if edge_index.numel():
            got = (edge_index.max() + 1).reshape(1).to(torch.int64)
        else:
            got = torch.zeros(1, dtype=torch.int64, device=edge_index.device)
        if not torch.cuda.is_current_stream_capturing():
            _MAXCUT_NP.put(edge_index, got)
    return got


def maxcut_n_p_host(edge_index: Tensor) -> int:
    """:func:`maxcut_n_p` as a Python int: one host read per list, remembered like the device word."""
    got = _MAXCUT_NP_HOST.get(edge_index)
    if got is None:
        got = (int(maxcut_n_p(edge_index)),)
        if not torch.cuda.is_current_stream_capturing():
            _MAXCUT_NP_HOST.put(edge_index, got)
    return got[0]


def maxcut_one_graph_ptr(n: int, device) -> Tensor:
    """int64 [0, n] on ``device``: the node offsets of a single graph, kept for the last few sizes."""
    key = (int(n), torch.device(device))
    got = _MAXCUT_ONE_GRAPH_PTR.get(key)
    if got is None:
        if len(_MAXCUT_ONE_GRAPH_PTR) >= 8:
            _MAXCUT_ONE_GRAPH_PTR.clear()
        got = _MAXCUT_ONE_GRAPH_PTR[key] = torch.tensor([0, int(n)], dtype=torch.long, device=device)
    return got


def maxcut_score_has_hub(edge_index: Tensor, num_nodes: int) -> bool:
    """Is the longest group (by destination or by source) too long for the layer kernel's one wave per group?  Measured on one MI355X
    (profiles/maxcut_forward.txt): the wave adds about one row per 0.23 us and layer, the composed form costs about
    2.2 ns per edge and layer stack of four, so the two meet near a group of E / 400 edges; the gate stands at
    ``max(MAXCUT_SCORE_MAX_GROUP, E / MAXCUT_SCORE_GROUP_SHARE)``.  The longest group is remembered with the index (one
    host read on a list's first sight)."""
    longest = max(sag_edge_group(edge_index, num_nodes, by_destination=True).max_members,  # the forward's walks
                  sag_edge_group(edge_index, num_nodes, by_destination=False).max_members)  # the backward's
    return longest > max(MAXCUT_SCORE_MAX_GROUP, edge_index.size(1) // MAXCUT_SCORE_GROUP_SHARE)


def maxcut_degree(by_src: AssignIndex, edge_index: Tensor, edge_weight: Optional[Tensor] = None, want_coef: bool = True,
                  want_coef_t: bool = False):
    """(dinv [N], coef [E] or None, coef_t [E] or None): ``dinv = deg^-1/2`` (inf -> 0) of the degrees by source without
    self-loops, ``coef_e = w_e dinv[src_e]`` (the forward's per-edge factor), ``coef_t_e = w_e dinv[dst_e]`` (the
    backward's)."""
    dev = N.require_device(edge_index, edge_weight, by_src.row_ptr)
    row, col = _edge_rows(edge_index)
    n, E = by_src.num_targets, row.numel()
    if by_src.nnz != E or by_src.row_ptr.numel() != n + 1:
        raise ValueError(f"maxcut_degree: an index of {by_src.nnz} edges over {n} nodes against {E} edges")
    ew = N.opt_f32_flat(edge_weight)
    if ew is not None and ew.numel() != E:
        raise ValueError(f"maxcut_degree: {ew.numel()} weights for {E} edges")
    dinv = torch.empty(n, dtype=torch.float32, device=dev)
    coef = torch.empty(E, dtype=torch.float32, device=dev) if want_coef else None
    coef_t = torch.empty(E, dtype=torch.float32, device=dev) if want_coef_t else None
    _checked(N.lib().tgp_maxcut_degree_f32, *by_src.walk(row, E), N.ptr(col) if E else None, N.ptr(ew), n, E,
             N.ptr(dinv), N.ptr(coef) if E else None, N.ptr(coef_t) if E else None, N.stream_ptr(dev))
    return dinv, coef, coef_t


def maxcut_layer(grp: AssignIndex, other: Tensor, coef: Optional[Tensor], dinv: Tensor, z: Tensor,
                 bias: Optional[Tensor], n_p: Optional[Tensor], delta: float, act: str = "identity",
                 w_next: Optional[Tensor] = None, want_h: bool = True):
    """(h [N, C] or None, z_next [N, C_next] or None): one delta-GCN layer on the projected rows ``z``,
    ``h_i = act((1 - delta) [i < n_p] z_i + delta dinv_i sum coef_e z[other_e] + bias)`` over node i's group without its
    self-loops, and in the same launch ``z_next = h w_next^T``."""
    if act not in MAXCUT_ACTS:
        raise ValueError(f"maxcut_layer: act {act!r} is not one of {sorted(MAXCUT_ACTS)}")
    dev = N.require_device(other, coef, dinv, z, bias, n_p, w_next, grp.row_ptr)
    other, n, E = _asap_group("maxcut_layer", grp, other)
    z, dinv = N.f32c(z), N.f32c(dinv.reshape(-1))
    if z.dim() != 2 or z.size(0) != n or dinv.numel() != n or (E and (coef is None or coef.numel() != E)):
        raise ValueError(f"maxcut_layer: z {tuple(z.shape)} and dinv [{dinv.numel()}] against {n} nodes, one coefficient "
                         f"per edge ({E})")
    C = z.size(1)
    coef = N.opt_f32_flat(coef)
    bias = N.opt_f32_flat(bias)
    if bias is not None and bias.numel() != C:
        raise ValueError(f"maxcut_layer: bias of {bias.numel()} entries for {C} channels")
    if n_p is not None and (n_p.dtype != torch.int64 or n_p.numel() != 1):
        raise ValueError("maxcut_layer: n_p is one device int64")
    w_next = N.opt_f32(w_next)
    if w_next is not None and (w_next.dim() != 2 or w_next.size(1) != C):
        raise ValueError(f"maxcut_layer: w_next {tuple(w_next.shape)} against {C} channels")
    if not want_h and w_next is None:
        raise ValueError("maxcut_layer: no output asked for")
    Cn = 0 if w_next is None else w_next.size(0)
    h = torch.empty(n, C, dtype=torch.float32, device=dev) if want_h else None
    zn = torch.empty(n, Cn, dtype=torch.float32, device=dev) if w_next is not None else None
    _checked(N.lib().tgp_maxcut_layer_f32, *grp.walk(other, E), N.ptr(coef) if E else None, N.ptr(dinv), N.ptr(z),
             N.ptr(bias), n, E, C, N.ptr(n_p), float(delta), MAXCUT_ACTS[act], N.ptr(h), N.ptr(w_next), Cn, N.ptr(zn),
             N.stream_ptr(dev))
    return h, zn


def maxcut_tail_fits(width: int, layers: Sequence) -> bool:
    """Do the row MLP's widths and parameter count fit the tail kernel (``layers``: the Linear modules, final last)?"""
    wmax = maxcut_max_width()
    outs = [lin.weight.size(0) for lin in layers]
    ins = [lin.weight.size(1) for lin in layers]
    if len(layers) < 1 or len(layers) > 9 or outs[-1] != 1 or ins != [width] + outs[:-1]:
        return False
    if any(o < 1 or o > wmax for o in outs) or width > wmax or any(lin.bias is None for lin in layers):
        return False
    return sum(lin.weight.numel() + lin.bias.numel() for lin in layers) <= maxcut_tail_max_params()


def maxcut_tail(h: Tensor, weights: Sequence[Tensor], biases: Sequence[Tensor], mlp_act: str, act: str) -> Tensor:
    """score [N] = act(final(mlp(h))): ``weights`` / ``biases`` of the mlp's Linear layers in order, the final
    ``Linear(., 1)`` last; one pass over ``h`` [N, C], the parameters in LDS."""
    if mlp_act not in MAXCUT_ACTS or act not in MAXCUT_ACTS:
        raise ValueError(f"maxcut_tail: activations must be among {sorted(MAXCUT_ACTS)}")
    dev = N.require_device(h, *weights, *biases)
    h = N.f32c(h)
    if h.dim() != 2 or len(weights) != len(biases) or not weights:
        raise ValueError("maxcut_tail: h must be [N, C] and every Linear needs its weight and bias")
    packed = torch.cat([t.detach().to(torch.float32).reshape(-1) for wb in zip(weights, biases) for t in wb])
    widths = [w.size(0) for w in weights[:-1]]
    arr = (ctypes.c_int64 * max(len(widths), 1))(*widths)
    score = torch.empty(h.size(0), dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_maxcut_tail_f32, N.ptr(h), h.size(0), h.size(1), ctypes.addressof(arr), len(widths),
             N.ptr(packed), packed.numel(), MAXCUT_ACTS[mlp_act], MAXCUT_ACTS[act], N.ptr(score), N.stream_ptr(dev))
    return score


def maxcut_wgrad(a: Tensor, b: Tensor) -> Tensor:
    """``a^T b`` [Ca, Cb] of two [N, .] row blocks at widths up to :func:`maxcut_max_width`: partial sums of fixed row
    chunks folded in ascending order, the same bits on every call."""
    dev = N.require_device(a, b)
    a, b = N.f32c(a), N.f32c(b)
    if a.dim() != 2 or b.dim() != 2 or a.size(0) != b.size(0):
        raise ValueError(f"maxcut_wgrad: a {tuple(a.shape)} and b {tuple(b.shape)} do not share their rows")
    L = N.lib()
    out = torch.empty(a.size(1), b.size(1), dtype=torch.float32, device=dev)
    wsb = L.tgp_maxcut_wgrad_workspace_bytes(a.size(0), a.size(1), b.size(1))
    ws = N.workspace(wsb, dev)
    _checked(L.tgp_maxcut_wgrad_f32, N.ptr(a), N.ptr(b), a.size(0), a.size(1), b.size(1), N.ptr(out), N.ptr(ws), wsb,
             N.stream_ptr(dev))
    return out


def maxcut_cut(grp: AssignIndex, other: Tensor, s: Tensor, edge_weight: Optional[Tensor] = None, want_cut: bool = True,
               want_wsum: bool = True):
    """(az, cut, wsum) [N] each (the unwanted ones None): ``az_i = sum over node i's group of w_e s[other_e]`` on the raw
    list, ``cut_i = s_i az_i``, ``wsum_i = sum w_e``."""
    dev = N.require_device(other, s, edge_weight, grp.row_ptr)
    other, n, E = _asap_group("maxcut_cut", grp, other)
    s = N.f32c(s.reshape(-1))
    ew = N.opt_f32_flat(edge_weight)
    if s.numel() != n or (ew is not None and ew.numel() != E):
        raise ValueError(f"maxcut_cut: one score per node ({n}) and one weight per edge ({E})")
    out = torch.empty(3, n, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_maxcut_cut_f32, *grp.walk(other, E), N.ptr(ew), N.ptr(s), n, E, N.ptr(out[0]),
             N.ptr(out[1]) if want_cut else None, N.ptr(out[2]) if want_wsum else None, N.stream_ptr(dev))
    return out[0], out[1] if want_cut else None, out[2] if want_wsum else None


def maxcut_assign_rounds(by_dst: AssignIndex, src: Tensor, labels: Tensor, rounds: int) -> Tensor:
    """``rounds`` rounds of the nearest-supernode label propagation on int32 labels [N] (1 .. K, 0 = none), launched back
    to back on two buffers without a host wait; returns the labels after the last round."""
    dev = N.require_device(src, labels, by_dst.row_ptr)
    src, n, E = _asap_group("maxcut_assign_rounds", by_dst, src)
    if labels.dtype != torch.int32 or labels.numel() != n or not labels.is_contiguous():
        raise ValueError(f"maxcut_assign_rounds: labels must be a contiguous int32 [{n}]")
    cur, nxt = labels, torch.empty_like(labels)
    fn = N.lib().tgp_maxcut_assign_round_i32
    for _ in range(int(rounds)):
        _checked(fn, *by_dst.walk(src, E), N.ptr(cur), n, E, N.ptr(nxt), N.stream_ptr(dev))
        cur, nxt = nxt, cur
    return cur


# ------------------------------------------------------------------------------------------------ EigenPooling
EIG_BAD_INPUT, EIG_ASYMMETRIC, EIG_OVER_LIMIT = 1, 2, 4  # status bits of tgp_eigenpool_modes_f32


def eigenpool_max_group_nodes() -> int:
    """Nodes of the largest (graph, cluster) group the modes kernel solves in LDS; one more takes the composed route."""
    return int(N.lib().tgp_eigenpool_max_group_nodes())


def eigenpool_modes(by_src: AssignIndex, dst: Tensor, edge_weight: Optional[Tensor], gid: Tensor, groups: AssignIndex,
                    num_modes: int, max_group: int, normalized: bool = True, embed: bool = False,
                    want_degree: bool = False):
    """theta_modes [N, H] float32 of the groups named by ``gid`` [N] int32 (``groups``: its inverted index), and the
    kernel's status word as a host int (bits ``EIG_*``; a flagged group is left at zero) -- plus, with ``want_degree``,
    the induced degrees [N].  ``max_group`` bounds the largest group the launch has to hold (at most
    :func:`eigenpool_max_group_nodes`; larger groups are flagged, not solved)."""
    dev = N.require_device(dst, edge_weight, gid, by_src.row_ptr, groups.row_ptr)
    dst, n, E = _asap_group("eigenpool_modes", by_src, dst)
    ew = N.opt_f32_flat(edge_weight)
    if gid.dtype != torch.int32 or gid.numel() != n or not gid.is_contiguous():
        raise ValueError(f"eigenpool_modes: gid must be a contiguous int32 [{n}]")
    if groups.nnz != n or (ew is not None and ew.numel() != E):
        raise ValueError(f"eigenpool_modes: one group per node ({n}) and one weight per edge ({E})")
    H = int(num_modes)
    theta = torch.zeros(n, max(H, 1), dtype=torch.float32, device=dev)
    deg = torch.zeros(n, dtype=torch.float32, device=dev) if want_degree else None
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _checked(N.lib().tgp_eigenpool_modes_f32, *by_src.walk(dst, E), N.ptr(ew), N.ptr(gid), N.ptr(groups.row_ptr),
             N.ptr(groups.perm), n, E, groups.num_targets, H, int(max_group), 1 if normalized else 0, 1 if embed else 0,
             N.ptr(theta), N.ptr(deg), N.ptr(status), N.stream_ptr(dev))
    st = int(status.item())
    if st & EIG_BAD_INPUT:
        raise N.TgpNativeError("tgp_eigenpool_modes_f32: an index outside its table (an edge endpoint, an edge position "
                               "or a label out of range); nothing out of range was read")
    return (theta, st, deg) if want_degree else (theta, st)


def eigenpool_reduce(theta_modes: Tensor, groups: AssignIndex, x: Tensor, max_len: int = 0) -> Tensor:
    """X_pool [G, H F]: ``X_pool[g, h F + f] = sum_{i in group g} theta_modes[i, h] x[i, f]``, nodes ascending, one pass
    over x, the same bits on every call.  ``max_len``: an upper bound of the longest group (0: short groups); it picks
    how many waves share a group, never the result's validity."""
    dev = N.require_device(theta_modes, x, groups.row_ptr)
    theta_modes, _ = _row_operand(theta_modes, "eigenpool_reduce", packed=True)
    x, _ = _row_operand(x, "eigenpool_reduce", packed=True)
    n, H = theta_modes.shape
    if x.size(0) != n or groups.nnz != n or H < 1:
        raise ValueError(f"eigenpool_reduce: theta_modes {tuple(theta_modes.shape)}, x {tuple(x.shape)} and an index of "
                         f"{groups.nnz} nodes do not go together")
    F, G = x.size(1), groups.num_targets
    out = torch.empty(G, H * F, dtype=torch.float32, device=dev)
    if G and F:
        _checked(N.lib().tgp_eigenpool_reduce_f32, N.ptr(theta_modes), N.ptr(groups.row_ptr), N.ptr(groups.perm),
                 N.ptr(x), F, n, G, H, F, int(max_len), N.ptr(out), N.stream_ptr(dev))
    return out


def eigenpool_lift(theta_modes: Tensor, gid: Tensor, x_pool: Tensor, num_groups: int) -> Tensor:
    """X_lift [N, F]: ``X_lift[i, f] = sum_h theta_modes[i, h] x_pool[gid[i], h F + f]`` (the adjoint of the Reduce)."""
    dev = N.require_device(theta_modes, gid, x_pool)
    theta_modes, _ = _row_operand(theta_modes, "eigenpool_lift", packed=True)
    x_pool, _ = _row_operand(x_pool, "eigenpool_lift", packed=True)
    n, H = theta_modes.shape
    if gid.dtype != torch.int32 or gid.numel() != n or not gid.is_contiguous():
        raise ValueError(f"eigenpool_lift: gid must be a contiguous int32 [{n}]")
    if H < 1 or x_pool.size(0) != num_groups or x_pool.size(1) % H:
        raise ValueError(f"eigenpool_lift: x_pool {tuple(x_pool.shape)} is not [{num_groups}, {H} F]")
    F = x_pool.size(1) // H
    out = torch.empty(n, F, dtype=torch.float32, device=dev)
    if n and F:
        _checked(N.lib().tgp_eigenpool_lift_f32, N.ptr(theta_modes), N.ptr(gid), N.ptr(x_pool), n, num_groups, H, F,
                 N.ptr(out), N.stream_ptr(dev))
    return out


# ------------------------------------------------------------------------------------------------ NMF pooling
NMF_BAD_INPUT, NMF_NON_FINITE, NMF_OVER_LIMIT = 1, 2, 4  # status bits of tgp_nmf_factorize_f32 / tgp_nmf_init_f32


def nmf_max_nodes() -> int:
    """Nodes of the largest graph the NMF kernel factorises in LDS; one more takes the composed route."""
    return int(N.lib().tgp_nmf_max_nodes())


def nmf_max_k() -> int:
    """The largest ``K`` the NMF kernel's LDS frame holds."""
    return int(N.lib().tgp_nmf_max_k())


def _nmf_args(name: str, by_src: AssignIndex, dst: Tensor, edge_weight: Optional[Tensor], gid: Tensor,
              graphs: AssignIndex):
    dst, n, E = _asap_group(name, by_src, dst)
    ew = N.opt_f32_flat(edge_weight)
    if gid.dtype != torch.int32 or gid.numel() != n or not gid.is_contiguous():
        raise ValueError(f"{name}: gid must be a contiguous int32 [{n}]")
    if graphs.nnz != n or (ew is not None and ew.numel() != E):
        raise ValueError(f"{name}: one graph per node ({n}) and one weight per edge ({E})")
    return dst, ew, n, E


def nmf_init(by_src: AssignIndex, dst: Tensor, edge_weight: Optional[Tensor], gid: Tensor, graphs: AssignIndex, k: int,
             max_n: int, seed: int = 0):
    """(W0 [N, K], H0^T [N, K], status): the default init of the NMF kernel alone (zeros for the graphs that are not
    factorised, and for a flagged graph)."""
    dev = N.require_device(dst, edge_weight, gid, by_src.row_ptr, graphs.row_ptr)
    dst, ew, n, E = _nmf_args("nmf_init", by_src, dst, edge_weight, gid, graphs)
    w0 = torch.zeros(2, n, max(int(k), 1), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _checked(N.lib().tgp_nmf_init_f32, *by_src.walk(dst, E), N.ptr(ew), N.ptr(gid), N.ptr(graphs.row_ptr),
             N.ptr(graphs.perm), n, E, graphs.num_targets, int(k), int(max_n), int(seed), N.ptr(w0[0]), N.ptr(w0[1]),
             N.ptr(status), N.stream_ptr(dev))
    return w0[0], w0[1], int(status.item())


def nmf_factorize(by_src: AssignIndex, dst: Tensor, edge_weight: Optional[Tensor], gid: Tensor, graphs: AssignIndex,
                  k: int, out_cols: int, max_n: int, seed: int = 0, tol: float = 1e-4, max_iter: int = 5000,
                  init: Optional[Tuple[Tensor, Tensor]] = None, want_factors: bool = False) -> dict:
    """One launch of the per-graph NMF kernel: ``s`` [N, out_cols] (softmax of H^T, zero columns behind ``ka``; zeros for
    a flagged graph), ``status`` (a host int, bits ``NMF_*``: the call's one host wait), ``iters`` [G] int32 and
    ``ratio`` [G], and with ``want_factors`` the raw ``w`` / ``ht`` [N, K].  ``init``: (W0, H0^T) [N, K] node-major."""
    dev = N.require_device(dst, edge_weight, gid, by_src.row_ptr, graphs.row_ptr)
    dst, ew, n, E = _nmf_args("nmf_factorize", by_src, dst, edge_weight, gid, graphs)
    Kc, G = int(k), graphs.num_targets
    w0 = h0t = None
    if init is not None:
        w0, h0t = N.f32c(init[0]), N.f32c(init[1])
        if tuple(w0.shape) != (n, Kc) or tuple(h0t.shape) != (n, Kc):
            raise ValueError(f"nmf_factorize: an explicit init is (W0, H0^T), both [{n}, {Kc}]")
    s = torch.zeros(n, int(out_cols), dtype=torch.float32, device=dev)
    fac = torch.zeros(2, n, max(Kc, 1), dtype=torch.float32, device=dev) if want_factors else None
    iters = torch.zeros(G, dtype=torch.int32, device=dev)
    ratio = torch.zeros(G, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _checked(N.lib().tgp_nmf_factorize_f32, *by_src.walk(dst, E), N.ptr(ew), N.ptr(gid), N.ptr(graphs.row_ptr),
             N.ptr(graphs.perm), n, E, G, Kc, int(out_cols), int(max_n), int(seed), float(tol), int(max_iter),
             N.ptr(w0), N.ptr(h0t), N.ptr(s), N.ptr(fac[0]) if want_factors else None,
             N.ptr(fac[1]) if want_factors else None, N.ptr(iters), N.ptr(ratio), N.ptr(status), N.stream_ptr(dev))
    out = {"s": s, "status": int(status.item()), "iters": iters, "ratio": ratio}
    if want_factors:
        out["w"], out["ht"] = fac[0], fac[1]
    return out


# ------------------------------------------------------------------------------------------------ SEP (csrc/sep_select.hip)
SEP_BAD_INPUT, SEP_BAD_WEIGHT, SEP_OVER_LIMIT = 1, 2, 4  # status bits of tgp_sep_select_f32


def sep_max_nodes() -> int:
    """Nodes of the largest graph whose coding tree the SEP kernel grows in LDS; one more takes the host route."""
    return int(N.lib().tgp_sep_max_nodes())


def sep_select(edge_index: Tensor, edge_weight: Optional[Tensor], gid: Tensor, graph_ptr: Tensor, num_nodes: int,
               max_n: int, cluster_index: Optional[Tensor] = None) -> dict:
    """The per-graph SEP selector (three launches, one host wait): ``cluster_index`` [N] int64 (left as it was for a
    flagged graph; ``cluster_index`` given: that tensor is written), ``counts`` / ``offsets`` [G] int32, ``status`` (a
    host int, bits ``SEP_*``) and ``total``, the number of supernodes of the graphs that were written."""
    dev = N.require_device(edge_index, edge_weight, gid, graph_ptr)
    n, G = int(num_nodes), graph_ptr.numel() - 1
    row, col = _edge_rows(edge_index)
    E = row.numel()
    ew = N.opt_f32_flat(edge_weight)
    if gid.dtype != torch.int32 or gid.numel() != n or not gid.is_contiguous():
        raise ValueError(f"sep_select: gid must be a contiguous int32 [{n}]")
    if graph_ptr.dtype != torch.int32 or G < 0 or not graph_ptr.is_contiguous():
        raise ValueError("sep_select: graph_ptr must be a contiguous int32 [G + 1]")
    if ew is not None and ew.numel() != E:
        raise ValueError(f"sep_select: {ew.numel()} weights for {E} edges")
    by_src = sag_edge_group(edge_index, n, by_destination=False)  # (remembered per edge_index tensor)
    by_dst = sag_edge_group(edge_index, n, by_destination=True)
    if cluster_index is None:
        cluster_index = torch.empty(n, dtype=torch.int64, device=dev)
    elif cluster_index.dtype != torch.int64 or cluster_index.numel() != n or not cluster_index.is_contiguous():
        raise ValueError(f"sep_select: cluster_index must be a contiguous int64 [{n}]")
    counts = torch.empty(2, max(G, 1), dtype=torch.int32, device=dev)
    words = torch.empty(2, dtype=torch.int32, device=dev)
    _checked(N.lib().tgp_sep_select_f32, N.ptr(by_src.row_ptr), N.ptr(by_src.perm), N.ptr(by_dst.row_ptr),
             N.ptr(by_dst.perm), N.ptr(row) if E else None, N.ptr(col) if E else None, N.ptr(ew), N.ptr(gid),
             N.ptr(graph_ptr), n, E, G, int(max_n), N.ptr(cluster_index), N.ptr(counts[0]), N.ptr(counts[1]),
             N.ptr(words), N.stream_ptr(dev))
    status, total = words.tolist()  # the call's one host wait
    return {"cluster_index": cluster_index, "counts": counts[0, :G], "offsets": counts[1, :G], "status": status,
            "total": total}


# ------------------------------------------------------------------------------------------------ PAN (csrc/pan.hip)
PAN_BAD_INPUT, PAN_CROSS_GRAPH, PAN_OVER_LIMIT = 1, 2, 4  # status bits of the tgp_pan_met_* entries
PAN_MAX_FILTER = 64

# edge lists the MET kernel declined before (an edge between two graphs), per graph offsets and node count: the same
# list with other graphs (no batch vector: one graph) is tried again
_PAN_DECLINED = TensorMemo(16)
_PAN_MET = TensorMemo(16)       # the sparse M a PANConv returned -> its PanMet record (what PANPooling starts from)


def pan_max_graph_nodes() -> int:
    """Nodes of the largest graph whose MET rows the kernel keeps in LDS; one more takes the composed route."""
    return int(N.lib().tgp_pan_max_graph_nodes())


_PAN_ONE_GRAPH_PTR: dict = {}


def pan_one_graph_ptr(n: int, device) -> Tensor:
    """int32 [0, n] on ``device``: the node offsets of a single graph, kept for the last few sizes."""
    key = (int(n), torch.device(device))
    got = _PAN_ONE_GRAPH_PTR.get(key)
    if got is None:
        if len(_PAN_ONE_GRAPH_PTR) >= 8:
            _PAN_ONE_GRAPH_PTR.clear()
        got = _PAN_ONE_GRAPH_PTR[key] = torch.tensor([0, int(n)], dtype=torch.int32, device=device)
    return got


class PanMet:
    """A MET matrix as the layers pass it on: ``index`` [2, nnz] (row-major sorted, coalesced), ``values`` [nnz] (the
    tensor autograd tracks), ``row_ptr`` int32 [N + 1], and -- native route only -- ``dinv`` [N] and ``frame``, the
    operands of the row walk that the backward repeats.  ``col_group`` is built on first use and kept."""

    __slots__ = ("index", "values", "row_ptr", "dinv", "frame", "num_nodes", "_col_group", "__weakref__")

    def __init__(self, index, values, row_ptr, num_nodes, dinv=None, frame=None):
        self.index, self.values, self.row_ptr, self.num_nodes = index, values, row_ptr, int(num_nodes)
        self.dinv, self.frame, self._col_group = dinv, frame, None

    @property
    def col_group(self) -> AssignIndex:
        """M's entries grouped by column, row order inside a column: the order of the score's column sums and of
        ``M^T g`` in the backward of ``M x``."""
        if self._col_group is None:
            self._col_group = edge_group(self.index, self.num_nodes, by_destination=True)
        return self._col_group


def pan_record(m: Tensor) -> Optional[PanMet]:
    """The record :class:`tgp.nn.PANConv` left for the sparse matrix ``m`` it returned (None: not one of them)."""
    return _PAN_MET.get(m)


def pan_remember(m: Tensor, met: PanMet) -> None:
    if not torch.cuda.is_current_stream_capturing():
        _PAN_MET.put(m, met)


def pan_route(edge_index: Tensor, weight: Tensor, num_nodes: int, graph_ptr: Optional[Tensor],
              max_graph_nodes: Optional[int]) -> str:
    """"native" for device tensors with float32 weights, nodes grouped by graph (``graph_ptr`` given) and a largest graph
    within :func:`pan_max_graph_nodes`; "composed" for everything else, and for a list the kernel declined before."""
    n, E = int(num_nodes), edge_index.size(1)
    ok = (edge_index.is_cuda and weight.is_cuda and weight.dtype == torch.float32 and graph_ptr is not None
          and max_graph_nodes is not None and n > 0 and 0 < int(max_graph_nodes) <= pan_max_graph_nodes()
          and weight.numel() - 1 <= PAN_MAX_FILTER and E < 2 ** 31 and n * int(max_graph_nodes) < 2 ** 31
          and _PAN_DECLINED.get(edge_index, other=graph_ptr, extra=n) is None)
    return "native" if ok else "composed"


def pan_met(edge_index: Tensor, weight: Tensor, num_nodes: int, gid: Optional[Tensor], graph_ptr: Tensor,
            max_graph_nodes: int) -> Optional[PanMet]:
    """The MET matrix of ``weight`` [L + 1] over the graphs ``graph_ptr`` (int32 [G + 1]; ``gid`` int32 [N] names every
    node's graph, None for one graph): a count -> fill pair with its single host wait.  None when the kernel declines (an
    edge whose endpoints lie in two graphs: remembered for this list and these graphs); an index outside its table
    raises.  The count checks every edge of the list at its source node, so its verdict is complete before the fill."""
    dev = N.require_device(edge_index, weight, gid, graph_ptr)
    row, col = _edge_rows(edge_index)
    n, E, G = int(num_nodes), row.numel(), graph_ptr.numel() - 1
    w = N.f32c(weight.detach().reshape(-1))
    if gid is not None and (gid.dtype != torch.int32 or gid.numel() != n or not gid.is_contiguous()):
        raise ValueError(f"pan_met: gid must be a contiguous int32 [{n}]")
    if graph_ptr.dtype != torch.int32 or G < 1 or not graph_ptr.is_contiguous() or w.numel() < 1:
        raise ValueError("pan_met: graph_ptr must be a contiguous int32 [G + 1] and weight hold at least one entry")
    by_src = sag_edge_group(edge_index, n, by_destination=False)  # (remembered per edge_index tensor)
    L, st = N.lib(), N.stream_ptr(dev)
    frame = (*by_src.walk(col, E), N.ptr(gid), N.ptr(graph_ptr), n, E, G, w.numel() - 1, int(max_graph_nodes))
    keep = (by_src, col, gid, graph_ptr)  # what the pointers of `frame` point into
    row_ptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
    dinv = torch.empty(n, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def count(ws, nbytes, d_count):
        _checked(L.tgp_pan_met_count, *frame, N.ptr(row_ptr), N.ptr(dinv), ws, nbytes, N.ptr(status), d_count, st)

    def fill(ws, nnz, r, c, v):
        _checked(L.tgp_pan_met_fill_f32, *frame, N.ptr(w), N.ptr(row_ptr), N.ptr(dinv), nnz, r, c, v, N.ptr(status), st)

    out = _count_fill(dev, L.tgp_pan_met_workspace_bytes(n), count, fill, w_dtype=torch.float32, declines=True)
    if isinstance(out, int):
        bits = int(status.item())
        if bits & PAN_BAD_INPUT:
            raise IndexError("pan_met: an index outside its table (an edge endpoint or edge position out of range, a node "
                             "outside its graph's range); nothing out of range was read")
        if bits & PAN_OVER_LIMIT:
            raise N.TgpNativeError(f"pan_met: a graph of more than max_graph_nodes = {max_graph_nodes} nodes")
        if not torch.cuda.is_current_stream_capturing():
            _PAN_DECLINED.put(edge_index, True, other=graph_ptr, extra=n)
        return None
    index, values = out
    return PanMet(index, values, row_ptr, n, dinv, (frame, keep))


def pan_met_bwd(met: PanMet, g_values: Tensor) -> Tensor:
    """part [N, L + 1]: per row of ``met`` the gradient shares of the series coefficients ``c_n`` (their sum over the
    rows is dL/dc), from the row powers recomputed in LDS."""
    frame, _ = met.frame
    dev = N.require_device(g_values, met.index, met.dinv)
    g = N.f32c(g_values.reshape(-1))
    nnz = met.index.size(1)
    if g.numel() != nnz:
        raise ValueError(f"pan_met_bwd: {g.numel()} gradient entries for {nnz} stored ones")
    n, L = met.num_nodes, frame[8]
    part = torch.zeros(n, L + 1, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _, col = _edge_rows(met.index)
    _checked(N.lib().tgp_pan_met_bwd_f32, *frame, N.ptr(met.row_ptr), N.ptr(col) if nnz else None,
             N.ptr(g) if nnz else None, N.ptr(met.dinv), nnz, N.ptr(part), N.ptr(status), N.stream_ptr(dev))
    return part


def pan_score(x: Tensor, p: Tensor, beta: Tensor, col_group: AssignIndex, values: Tensor, tanh: bool,
              want_terms: bool = False):
    """act(beta[0] <x_i, p> + beta[1] sum_{e: col(e) = i} values[e]) [N] in one launch, act = tanh or identity;
    ``want_terms``: ``(score, dot, colsum)`` with the two terms as well (what the backward needs)."""
    dev = N.require_device(x, p, beta, values, col_group.row_ptr)
    x, ld = _row_operand(x, "pan_score")
    p, beta, values = N.f32c(p.reshape(-1)), N.f32c(beta.reshape(-1)), N.f32c(values.reshape(-1))
    n, F, nnz = x.size(0), x.size(1), values.numel()
    if p.numel() != F or beta.numel() != 2 or col_group.num_targets != n or col_group.nnz != nnz:
        raise ValueError(f"pan_score: x {tuple(x.shape)}, p of {p.numel()}, beta of {beta.numel()} entries and an index of "
                         f"{col_group.nnz} entries over {col_group.num_targets} nodes against {nnz} values")
    out = torch.empty(3 if want_terms else 1, n, dtype=torch.float32, device=dev)
    _checked(N.lib().tgp_pan_score_f32, N.ptr(x), n, F, ld, N.ptr(p), N.ptr(beta), N.ptr(col_group.row_ptr),
             N.ptr(col_group.perm), N.ptr(values) if nnz else None, nnz, int(bool(tanh)), N.ptr(out[0]),
             N.ptr(out[1]) if want_terms else None, N.ptr(out[2]) if want_terms else None, N.stream_ptr(dev))
    return (out[0], out[1], out[2]) if want_terms else out[0]


# ------------------------------------------------------------------------------------------ GTVConv (csrc/gtvconv.hip)
GTV_ACT_CODES = {"identity": 0, "relu": 1, "elu": 2}  # the activations the forward kernel applies itself
GTV_MAX_CHANNELS = 32767
GTV_REGISTER_CHANNELS = 512  # wider rows take the chunked kernels, which need the distance buffer in the forward too

# How the last call of :class:`tgp.mp.GTVConv` / ``tgp.mp.gtv_propagate`` was served, and how many calls each route took
GTV_RECORD = {"route": None, "native": 0, "composed": 0}

_GTV_VALID = TensorMemo(16)  # edge_index (+ node count) -> True, or the positions of the edges with both ends in range


def gtv_record() -> dict:
    """A copy of the route record: ``route`` ("native" / "composed") of the last call and the two counters."""
    return dict(GTV_RECORD)


def gtv_note(route: str) -> None:
    GTV_RECORD["route"] = route
    GTV_RECORD[route] += 1


def gtv_edges_in_range(edge_index: Tensor, num_nodes: int):
    """None when every endpoint lies in [0, num_nodes); otherwise the positions (int64, ascending) of the edges whose
    ends both do.  One host wait per ``edge_index`` object, remembered: the edge indexes are built from the sources and
    the destinations, so a list is only handed to them with every id in range."""
    got = _GTV_VALID.get(edge_index, extra=int(num_nodes))
    if got is None:
        if edge_index.numel() == 0:
            got = True
        else:
            ok = ((edge_index >= 0) & (edge_index < num_nodes)).all(dim=0)
            got = True if bool(ok.all()) else ok.nonzero().view(-1)
        if not torch.cuda.is_current_stream_capturing():
            _GTV_VALID.put(edge_index, got, extra=int(num_nodes))
    return None if got is True else got


def _gtv_frame(who: str, h: Tensor, col: Tensor, edge_weight: Optional[Tensor], by_src: AssignIndex):
    """Shapes of what every GTV entry shares, checked before any launch: (n, C, E, w)."""
    if h.dim() != 2 or h.dtype != torch.float32 or not h.is_contiguous():
        raise ValueError(f"{who}: h must be a contiguous float32 [N, C], got {h.dtype} {tuple(h.shape)}")
    n, C = h.shape
    if not 1 <= C <= GTV_MAX_CHANNELS:
        raise ValueError(f"{who}: {C} channels (1 .. {GTV_MAX_CHANNELS})")
    if col.dim() != 1 or col.dtype != torch.int64 or not col.is_contiguous():
        raise ValueError(f"{who}: the edge rows must be contiguous int64 vectors")
    E = col.numel()
    if E >= 2 ** 31 or n >= 2 ** 31:
        raise ValueError(f"{who}: {n} nodes and {E} edges are beyond the int32 index")
    if by_src.num_targets != n or by_src.nnz != E or by_src.row_ptr.numel() != n + 1 or (
            by_src.perm is not None and E and by_src.perm.numel() < E):
        raise ValueError(f"{who}: an index of {by_src.nnz} edges over {by_src.num_targets} nodes against {E} edges over "
                         f"{n} nodes")
    w = edge_weight
    if w is not None and (w.dim() != 1 or w.numel() != E or w.dtype != torch.float32):
        raise ValueError(f"{who}: edge_weight must be float32 [{E}], got {w.dtype} {tuple(w.shape)}")
    return n, C, E, (None if w is None else N.f32c(w))


def _gtv_mask(who: str, mask: Optional[Tensor], n: int) -> Optional[Tensor]:
    if mask is None:
        return None
    if mask.numel() != n or mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{who}: mask must hold one bool per node ({n}), got {mask.dtype} {tuple(mask.shape)}")
    return mask.reshape(-1).contiguous().view(torch.uint8)


def _gtv_row_like(who: str, name: str, t: Tensor, h: Tensor) -> Tensor:
    if t.shape != h.shape or t.dtype != torch.float32:
        raise ValueError(f"{who}: {name} {t.dtype} {tuple(t.shape)} does not match h {tuple(h.shape)}")
    return t if t.is_contiguous() else t.contiguous()


def gtv_edge_fwd(h: Tensor, col: Tensor, edge_weight: Optional[Tensor], by_src: AssignIndex, bias: Optional[Tensor],
                 mask: Optional[Tensor], delta: float, eps: float, act_code: int, want_d: bool = False):
    """(out [N,C], d [E] or None): GTVConv's propagation of the projected rows ``h`` (mp/gtvconv.py:137-167),
    out_i = act((h_i + delta sum over i's out-edges of w_e / max(d_e, eps) (h_col - h_i) + bias) [* mask_i]) with
    d_e = ||h_i - h_col||_1, one pass over every node's out-edges in the order of ``by_src``; self-loops and edges with
    an end out of range are skipped.  ``want_d``: the distances as well (what a backward needs; 0 at a skipped edge)."""
    who = "gtv_edge_fwd"
    n, C, E, w = _gtv_frame(who, h, col, edge_weight, by_src)
    if act_code not in (0, 1, 2):
        raise ValueError(f"{who}: act_code {act_code} (0 identity, 1 relu, 2 elu)")
    b = None
    if bias is not None:
        if bias.numel() != C or bias.dtype != torch.float32:
            raise ValueError(f"{who}: bias must be float32 [{C}], got {bias.dtype} {tuple(bias.shape)}")
        b = N.f32c(bias.reshape(-1))
    m = _gtv_mask(who, mask, n)
    dev = N.require_device(h, col, w, b, m)
    out = torch.empty_like(h)
    d = torch.zeros(E, dtype=torch.float32, device=dev) if (want_d or C > GTV_REGISTER_CHANNELS) and E else None
    src_ptr, src_perm, col_p = by_src.walk(col, E)
    _checked(N.lib().tgp_gtv_edge_fwd_f32, N.ptr(h), n, C, src_ptr, src_perm, col_p, N.ptr(w), E, N.ptr(b), N.ptr(m),
             float(delta), float(eps), int(act_code), N.ptr(out), N.ptr(d), N.stream_ptr(dev))
    if want_d and d is None:
        d = torch.zeros(0, dtype=torch.float32, device=dev)
    return out, (d if want_d else None)


def gtv_edge_bwd_terms(h: Tensor, out: Tensor, g_out: Tensor, col: Tensor, edge_weight: Optional[Tensor],
                       by_src: AssignIndex, d: Tensor, mask: Optional[Tensor], delta: float, eps: float, act_code: int,
                       want_gw: bool = False):
    """(g [N,C], gw [E] or None, t [E]) of the propagation's backward: g = g_out act'(out) mask, per out-edge
    s_e = delta <g_i, h_col - h_i>, gw_e = s_e / max(d_e, eps) (the gradient of the edge weight) and the gradient of
    d_e, t_e = -s_e gamma_e / d_e where d_e >= eps and 0 where the clamp holds (zeros at a skipped edge)."""
    who = "gtv_edge_bwd_terms"
    n, C, E, w = _gtv_frame(who, h, col, edge_weight, by_src)
    out, g_out = _gtv_row_like(who, "out", out, h), _gtv_row_like(who, "g_out", g_out, h)
    if d.numel() != E or d.dtype != torch.float32 or act_code not in (0, 1, 2):
        raise ValueError(f"{who}: d must be float32 [{E}] and act_code one of 0, 1, 2")
    m = _gtv_mask(who, mask, n)
    dev = N.require_device(h, out, g_out, col, w, d, m)
    g = torch.empty_like(h)
    terms = torch.zeros(2 if want_gw else 1, max(E, 1), dtype=torch.float32, device=dev)
    src_ptr, src_perm, col_p = by_src.walk(col, E)
    _checked(N.lib().tgp_gtv_edge_bwd_terms_f32, N.ptr(h), N.ptr(out), N.ptr(g_out), n, C, src_ptr, src_perm, col_p,
             N.ptr(w), E, N.ptr(N.f32c(d)), N.ptr(m), float(delta), float(eps), int(act_code), N.ptr(g),
             N.ptr(terms[1]) if want_gw else None, N.ptr(terms[0]), N.stream_ptr(dev))
    return g, (terms[1, :E] if want_gw else None), terms[0, :E]


def gtv_edge_bwd_nodes(h: Tensor, g: Tensor, row: Tensor, col: Tensor, edge_weight: Optional[Tensor],
                       by_src: AssignIndex, by_dst: AssignIndex, d: Tensor, t: Tensor, delta: float,
                       eps: float) -> Tensor:
    """dh [N,C]: every node adds over its out-edges and then its in-edges (no scatter),
    dh_i = g_i (1 - delta sum_out gamma_e) + sum_out t_e sign(h_i - h_col) + sum_in (delta gamma_e g_row - t_e
    sign(h_row - h_i))."""
    who = "gtv_edge_bwd_nodes"
    n, C, E, w = _gtv_frame(who, h, col, edge_weight, by_src)
    g = _gtv_row_like(who, "g", g, h)
    if row.shape != col.shape or row.dtype != torch.int64 or not row.is_contiguous():
        raise ValueError(f"{who}: the edge rows must be contiguous int64 vectors of one length")
    if by_dst.num_targets != n or by_dst.nnz != E or by_dst.row_ptr.numel() != n + 1:
        raise ValueError(f"{who}: a by-destination index of {by_dst.nnz} edges over {by_dst.num_targets} nodes against "
                         f"{E} edges over {n} nodes")
    if d.numel() != E or t.numel() != E or d.dtype != torch.float32 or t.dtype != torch.float32:
        raise ValueError(f"{who}: d and t must be float32 [{E}]")
    dev = N.require_device(h, g, row, col, w, d, t)
    dh = torch.empty_like(h)
    src_ptr, src_perm, col_p = by_src.walk(col, E)
    dst_ptr, dst_perm, row_p = by_dst.walk(row, E)
    _checked(N.lib().tgp_gtv_edge_bwd_nodes_f32, N.ptr(h), N.ptr(g), n, C, src_ptr, src_perm, dst_ptr, dst_perm, row_p,
             col_p, N.ptr(w), E, N.ptr(N.f32c(d)), N.ptr(N.f32c(t)), float(delta), float(eps), N.ptr(dh),
             N.stream_ptr(dev))
    return dh
