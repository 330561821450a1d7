/*
 * tgp_hip.h — C ABI of the MI355X-native SRC pooling hot path (Reduce + Connect).
 *
 * The reference (tgp-team/torch-geometric-pool 1.0.1) has no FFI: its operator API is a
 * Python class protocol whose arithmetic is delegated to ATen / torch_geometric /
 * torch_scatter.  This header defines the boundary *underneath* that protocol: one entry
 * point per row of SURVEY.md section 8(a), each citing the reference lines it replaces.
 * The host-side mirror of the protocol (torch-geometric-pool_amd/tgp) binds these symbols
 * with ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc / PyTorch caching allocator) unless
 *     the name ends in `_host`; index tensors are int64 (reference: utils/ops.py:472-476),
 *     features / weights are fp32; `[2,E]` edge lists are given as two row pointers.
 *   - fp32 is the default value type (the reference's default dtype: torch.ones(E) at ops.py:385,547;
 *     base_select.py:64; north_star's 1e-5 tolerance is stated in it).  r4: the HBM-bound operators also exist for
 *     float64 values (`*_f64`: sparse Reduce, subgraph / coalesce Connect, block-diagonal export, sparse and dense
 *     post-processing; see the section near the end), because the reference's ATen ops compute model.double() inputs
 *     in fp64.  r5: the dense GEMM path has fp64 forms too (tgp_bmm_f64, tgp_dense_pool_f64, tgp_segment_gemm_*_f64,
 *     tgp_spmm_csr_f64 on the fp64 matrix instruction); only the fused small-graph kernels and the fused loss kernels
 *     are fp32-only, and the host mirror does not route float64 tensors to them.  Two algorithms whose RESULT depends on wider arithmetic run in fp64
 *     inside their kernels regardless of the I/O type: the Kron reduction (tgp_kron_batched_*) and NDPSelect's
 *     eigen-iteration (tgp_ndp_*); KronConnect also accepts fp64 Laplacian values (`val64`).
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous on it and
 *     never synchronises, allocates or frees.  Scratch memory comes from the caller
 *     (`ws`, sized by the matching *_workspace_bytes()).
 *   - data-dependent output sizes use a count -> fill pair: *_count leaves the number of
 *     surviving edges in `*d_count` (device int64); the caller reads it (the one host
 *     sync the reference's own `.item()` calls also pay), allocates exact outputs and
 *     calls *_fill with the SAME workspace.
 *   - `eps` arguments: the reference reads its module-level `eps` (tgp/__init__.py:6, 1e-8) at CALL time
 *     (utils/ops.py:72,318,377,395; utils/losses.py:498; tests monkeypatch it), so it is an argument of every
 *     entry point that filters or clamps with it, never a compiled-in constant.
 *   - *d_count < 0 is a refusal, not a size: -1 = this fast path declines (preconditions not met: the caller
 *     takes its general route; -3 / -5: declines that name the entry point to call instead, see there), -2 = bad input (a node id outside [0, num_nodes) or a cluster id outside
 *     [0, num_supernodes): never dereferenced; the reference's index ops raise for it too).
 *   - return value 0 = ok; otherwise a negative tgp_status and tgp_last_error() holds a
 *     thread-local message.  No exceptions cross the boundary; no global mutable state.
 */
#ifndef TGP_HIP_H
#define TGP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TGP_ABI_VERSION 10044 /* 1.0.1 of the reference, ABI revision 43 (k-MIS selection: tgp_kmis_graphs, tgp_kmis_rounds_start, tgp_kmis_rounds, tgp_kmis_clusters, tgp_kmis_greedy_f32, tgp_kmis_wsum_f32, tgp_kmis_degree_f32, tgp_kmis_mis_index_i64; appended without a new revision, AsymCheegerCut's losses: tgp_acc_small_graph_nodes, tgp_acc_tv_dense_f32 / _bwd_f32, tgp_acc_tv_edge_f32 / _bwd_f32, tgp_acc_quantile_f32, tgp_acc_loss_terms_f32, tgp_acc_asym_bwd_f32; HOSC's losses: tgp_hosc_small_graph_nodes, tgp_hosc_record_floats, tgp_hosc_matvec_f32, tgp_hosc_node_terms_f32, tgp_hosc_small_f32, tgp_hosc_loss_terms_f32 / _bwd_f32, tgp_hosc_ds_f32; BN-Pool's reconstruction loss: tgp_bnpool_max_clusters, tgp_bnpool_part_floats, tgp_bnpool_rec_fwd_f32 / _bwd_f32; edge-contraction selection: tgp_edge_contract_max_graph_nodes, tgp_edge_contract_edge_cache, tgp_edge_contract_hub_degree, tgp_edge_contract_workspace_bytes, tgp_edge_contract_project_f32, tgp_edge_contract_raw_f32, tgp_edge_contract_normalize_f32, tgp_edge_contract_graphs, tgp_edge_contract_rounds_start, tgp_edge_contract_rounds, tgp_edge_contract_weights_f32; the segment readout: tgp_segment_aggr_chunk_rows, tgp_segment_aggr_workspace_bytes, tgp_segment_aggr_f32 / _bwd_f32; EigenPooling: tgp_eigenpool_max_group_nodes, tgp_eigenpool_modes_f32, tgp_eigenpool_reduce_f32, tgp_eigenpool_lift_f32; PAN: tgp_pan_max_graph_nodes, tgp_pan_met_workspace_bytes, tgp_pan_met_count, tgp_pan_met_fill_f32, tgp_pan_met_bwd_f32, tgp_pan_score_f32; GTVConv: tgp_gtv_edge_fwd_f32, tgp_gtv_edge_bwd_terms_f32, tgp_gtv_edge_bwd_nodes_f32; the dense poolers' adjacency gradient: tgp_dense_pool_adj_grad_f32, tgp_dense_pool_adj_grad_small_f32) */

enum tgp_status {
  TGP_OK = 0,
  TGP_ERR_INVALID = -1,   /* bad argument (null pointer, negative size, unknown enum) */
  TGP_ERR_WORKSPACE = -2, /* workspace too small */
  TGP_ERR_LAUNCH = -3,    /* HIP reported an error at launch */
  TGP_ERR_RANGE = -4      /* size beyond what the int32 internal indices can address */
};

/* coalesce reduction, reference: utils/typing.py ConnectionType, connect/base_conn.py:87 */
enum tgp_reduce_op { TGP_SUM = 0, TGP_MEAN = 1, TGP_MIN = 2, TGP_MAX = 3, TGP_MUL = 4 };

/* flag bits shared by the Connect / post-processing entry points */
enum tgp_flags {
  TGP_REMOVE_SELF_LOOPS = 1, /* utils/ops.py:370-371, 307-308 */
  TGP_DEGREE_NORM = 2,       /* utils/ops.py:383-401, 311-319 */
  TGP_EDGE_WEIGHT_NORM = 4,  /* utils/ops.py:404-417, 322-333 */
  TGP_SUM_AXIS_ROWS = 8,     /* dense: degree = sum over axis -2 (adj_transpose=True, ops.py:312-314) */
  TGP_EPS_FILTER = 16,       /* sparse: drop |w| <= 1e-8 when weights are given (ops.py:374-380) */
  TGP_ADJ_TRANSPOSED = 32,   /* dense: A is handed over as the transposed view (src.py:442-443) */
  TGP_NODE_FILTER = 64,      /* subgraph_fill: node_index was given to the matching _count call */
  TGP_WANT_EDGE_ID = 128,    /* subgraph_count + _fill: also stage / emit the input position of every kept edge */
  TGP_HUGE_ROWS = 256        /* coalesce_rows_count: supernode rows beyond 1024 raw entries (hubs) are sorted device-wide
                                instead of declining the call (workspace: ..._rows_huge_workspace_bytes) */
};

int tgp_version(void);
const char* tgp_last_error(void);
/* number of compute units of the current device (sizing persistent grids); <0 on error */
int tgp_device_cu_count(void);

/* ------------------------------------------------------------------------------------
 * A1  BaseReduce.forward, sparse path  (reduce/base_reduce.py:141-155)
 *     x_pool[c,:] = sum_{i: cluster_index[i]==c} weight[i] * x[node_index[i],:]
 * The inverted index (assignments grouped by supernode, ascending i inside a group) is a
 * function of the SelectOutput alone, so it is built once and may be cached by the caller.
 * ---------------------------------------------------------------------------------- */
size_t tgp_assign_index_workspace_bytes(int64_t nnz, int64_t num_supernodes);
int tgp_assign_index_build(const int64_t* cluster_index, int64_t nnz, int64_t num_supernodes,
                           int32_t* row_ptr /* [num_supernodes+1] */, int32_t* perm /* [nnz] */,
                           void* ws, size_t ws_bytes, void* stream);
int tgp_reduce_sparse_f32(const float* x, int64_t num_nodes, int64_t num_features, int64_t x_row_stride,
                          const int64_t* node_index, const float* weight /* may be NULL = ones */,
                          const int32_t* row_ptr /* NULL = one assignment per supernode (nnz == K): TopK, NDP */,
                          const int32_t* perm /* NULL = identity */, int64_t nnz,
                          int64_t num_supernodes, float* x_pool /* [K,F] contiguous */, void* stream);

/* A1 for selectors whose supernodes own exactly ONE node (TopK, NDP; r4), with the PACKED index: pack[c] = low word the
 * int32 source row node_index[a], high word the fp32 weight[a] of supernode c's single assignment a -- one streamed
 * 8-byte load per supernode instead of perm[c] + two random gathers.  x_pool[c,:] = 0 + weight * x[row,:], the bits of
 * tgp_reduce_sparse_f32.  tgp_one_to_one_index_build derives perm and pack from (node_index, cluster_index, weight) in
 * one launch (cluster_index a permutation of 0..k-1); tgp_topk_select emits the pack itself.  F % 4 == 0, F >= 32 and
 * 16-byte aligned rows (other shapes: tgp_reduce_sparse_f32). */
int tgp_one_to_one_index_build(const int64_t* node_index, const int64_t* cluster_index,
                               const float* weight /* NULL = ones */, int64_t k, int32_t* perm /* [k] */,
                               uint64_t* pack /* [k] */, void* stream);
int tgp_reduce_one_to_one_f32(const float* x, int64_t num_nodes, int64_t num_features, int64_t x_row_stride,
                              const uint64_t* pack, int has_weight, int64_t num_supernodes, float* x_pool, void* stream);

/* A2  Reduce.reduce_batch, sparse branch (reduce/base_reduce.py:37-41):
 *     out = arange(K); out[cluster_index[i]] = batch[node_index[i]]                      */
int tgp_reduce_batch_i64(const int64_t* batch, const int64_t* node_index, const int64_t* cluster_index,
                         int64_t nnz, int64_t num_supernodes,
                         int every_cluster_has_a_node /* 1: the arange is never visible (selectors that create a
                                                         supernode per kept node / matched pair): one launch */,
                         int64_t* batch_pool, void* stream);

/* ------------------------------------------------------------------------------------
 * A5 + A6  sparse_connect, TopK branch (connect/base_conn.py:79-82 -> PyG subgraph with
 * relabel_nodes=True) fused with the edge filters of postprocess_adj_pool_sparse
 * (utils/ops.py:370-380).  Output keeps INPUT edge order; endpoints are relabelled to
 * their position in the ascending `node_index`.  node_index == NULL turns the node
 * filter/relabel off (plain remove_self_loops + eps filter on an edge list).
 * ---------------------------------------------------------------------------------- */
size_t tgp_connect_subgraph_workspace_bytes(int64_t num_edges, int64_t num_nodes);
int tgp_connect_subgraph_count(const int64_t* row, const int64_t* col, const float* edge_weight /* NULL ok */,
                               int64_t num_edges, const int64_t* node_index /* NULL ok */, int64_t num_kept,
                               int64_t num_nodes, int flags, float eps, void* ws, size_t ws_bytes,
                               int64_t* d_count, void* stream);
int tgp_connect_subgraph_fill(const int64_t* row, const int64_t* col, const float* edge_weight,
                              int64_t num_edges, int64_t num_nodes, int flags, float eps, const void* ws,
                              int64_t num_out, int64_t* out_row, int64_t* out_col, float* out_weight,
                              int64_t* out_edge_id /* NULL ok: input position of every kept edge (the map the
                                                      backward of the weight pass-through needs); requires
                                                      TGP_WANT_EDGE_ID in `flags` of _count and _fill */,
                              void* stream);

/* The same operator in ONE pass (r4): survivors are written once, in their final int64 form at their final offsets of
 * CAPACITY-num_edges outputs (out_row / out_col / out_weight / out_edge_id: the first `total` entries are the result,
 * identical to the count -> fill pair above), through an epoch-tagged decoupled look-back over the 4096-edge chunks
 * (`status`: >= tgp_connect_subgraph_single_status_words(E) 64-bit words of device memory, caller-owned, never
 * cleared, one buffer per stream; 0 < epoch < 2^29 different for every call on it).  `*result` (device-accessible, e.g.
 * pinned host memory the caller polls) receives {epoch << 34 | refused << 31 | total} when the last chunk is done;
 * refused = an endpoint outside [0, num_nodes) was met (the count -> fill pair reports -2 for it), or a look-back
 * spin bound was hit (the device is shared: use the pair).  The two are told apart by word [1] of `status`: a chunk that
 * met a bad endpoint stores `epoch` into its low 32 bits (r5; r4 used a zeroed word of the workspace).  num_edges > 0.
 * member_bits_in / rank128_in (r5, NULL ok, both or neither): the kept-node bitmap [4 * blocks] and its rank directory
 * [blocks] (kept nodes with id < 128 b), blocks = tgp_topk_select_directory_blocks(num_nodes), as tgp_topk_select
 * writes them for the selection whose ASCENDING node_index is passed here.  The call is then ONE launch: no memset, no
 * scatter of the kept nodes into bitmap + relabel table, no directory scan in every workgroup (r4: 118 us per call at
 * N = 1M / E = 10M of which the stage kernel was 76).  Needs bitmap + directory to fit LDS (num_nodes <= ~1.2 M);
 * otherwise they are ignored. */
size_t tgp_connect_subgraph_single_workspace_bytes(int64_t num_nodes);
int64_t tgp_connect_subgraph_single_status_words(int64_t num_edges);
int tgp_connect_subgraph_single(const int64_t* row, const int64_t* col, const float* edge_weight /* NULL ok */,
                                int64_t num_edges, const int64_t* node_index /* NULL = filters only */, int64_t k,
                                int64_t num_nodes, int flags, float eps, void* ws, size_t ws_bytes, int64_t* out_row,
                                int64_t* out_col, float* out_weight, int64_t* out_edge_id /* NULL ok */,
                                const uint32_t* member_bits_in, const uint32_t* rank128_in,
                                uint64_t* status, int64_t status_words, uint64_t* result, uint32_t epoch, void* stream);

/* ------------------------------------------------------------------------------------
 * A4 + A6  sparse_connect, one-over-K branch (connect/base_conn.py:83-89 -> PyG coalesce):
 * relabel endpoints by cluster_index, sort by (row, col) (stable), merge duplicates with
 * `reduce_op`, then the filters of utils/ops.py:370-380.  Output is row-major sorted and
 * unique.  edge_weight == NULL keeps the result unweighted (out_weight unused).
 * ---------------------------------------------------------------------------------- */
size_t tgp_connect_coalesce_workspace_bytes(int64_t num_edges, int64_t num_nodes, int64_t num_supernodes);
int tgp_connect_coalesce_count(const int64_t* row, const int64_t* col, const float* edge_weight /* NULL ok */,
                               int64_t num_edges, const int64_t* cluster_index, int64_t num_nodes,
                               int64_t num_supernodes, int reduce_op, int flags, float eps, void* ws, size_t ws_bytes,
                               int64_t* d_count, void* stream);
int tgp_connect_coalesce_fill(const void* ws, int64_t num_edges, int64_t num_nodes, int64_t num_supernodes, int has_weight,
                              int flags, int64_t num_out, int64_t* out_row, int64_t* out_col,
                              float* out_weight, void* stream);

/* A4 + A6 fast path for ROW-SORTED edge lists (the PyG default): no global sort.  Edges are grouped by
 * supernode row through the CSR of the input and the supernode->member index of the assignment
 * (assign_row_ptr / assign_perm = what tgp_assign_index_build returns for cluster_index), then every short
 * row segment is ordered by column, merged and filtered inside LDS.  Same output as the sort-based pair
 * above.  If the rows are not sorted *d_count is set to -1 and the caller uses tgp_connect_coalesce_{count,fill}
 * instead.  A supernode row of more than 1024 raw entries (a hub of a power-law graph): *d_count = -5 unless
 * TGP_HUGE_ROWS is in `flags` (r4) -- then the entries of such rows alone go through a device-wide stable sort (at most
 * 4096 of them per call, else -1) while every other row stays in LDS, and `ws` must hold
 * tgp_connect_coalesce_rows_huge_workspace_bytes(); the matching _fill call takes the same workspace. */
size_t tgp_connect_coalesce_rows_workspace_bytes(int64_t num_edges, int64_t num_nodes, int64_t num_supernodes);
size_t tgp_connect_coalesce_rows_huge_workspace_bytes(int64_t num_edges, int64_t num_nodes, int64_t num_supernodes);
int tgp_connect_coalesce_rows_count(const int64_t* row, const int64_t* col, const float* edge_weight /* NULL ok */,
                                    int64_t num_edges, const int64_t* cluster_index, int64_t num_nodes,
                                    int64_t num_supernodes, const int32_t* assign_row_ptr,
                                    const int32_t* assign_perm,
                                    const int32_t* csr_ptr /* NULL, or CSR offsets [N+1] of this row-sorted list */,
                                    int reduce_op, int flags, float eps, void* ws,
                                    size_t ws_bytes, int64_t* d_count, void* stream);
int tgp_connect_coalesce_rows_fill(const void* ws, int64_t num_edges, int64_t num_nodes, int64_t num_supernodes,
                                   int has_weight /* bit 0: weights; bit 1: the count call ran with TGP_HUGE_ROWS */,
                                   int64_t num_out, int64_t* out_row, int64_t* out_col,
                                   float* out_weight, void* stream);

/* The host read of any count -> fill pair below without a device-to-host copy: stores
 * {epoch << 34 | *d_count as a 34-bit two's complement number} with system scope into `*result` (pinned host memory the
 * caller polls; epoch as for tgp_sparse_pool_small_f32).  Stands in for the reference's `.item()` reads
 * (connect/base_conn.py:79-82 via torch_geometric.utils.subgraph, utils/ops.py:370-380). */
int tgp_count_publish(const int64_t* d_count, uint64_t* result, uint32_t epoch, void* stream);

/* tgp_connect_coalesce_rows_count with its survivor scan as ONE launch that also hands the count to the host (r4):
 * the scan takes the survivors in front of every block of 4096 supernode rows from an epoch-tagged decoupled look-back
 * (`status`: >= ..._status_words(K, N) 64-bit words of device memory, caller-owned, never cleared, one buffer per stream;
 * 0 < epoch < 2^29 different for every call on it; the member segments of the front end take their offsets from a second
 * look-back over the same buffer -- member degree sums, their scan and the CSR check are ONE launch on this route) and its last workgroup stores {epoch << 34 | *d_count as a 34-bit
 * two's complement number} with system scope into `*result` (pinned host memory the caller polls; same word format as
 * tgp_count_publish).  *d_count is written as well; tgp_connect_coalesce_rows_fill follows as for the plain count.
 * `csr_col` (NULL ok, only with csr_ptr): the int32 copy of `col` that GraclusSelect's CSR holds for this very list --
 * half the column stream of the gather kernel; `col` is still needed (hub rows).
 * Measured alternatives (profiles/r04_coalesce_tail_experiments.md): the look-back inside the FILL (64-row tiles) and the
 * fill inside the count call (host wait at the end) are both slower. */
int64_t tgp_connect_coalesce_rows_count_status_words(int64_t num_supernodes, int64_t num_nodes);
int tgp_connect_coalesce_rows_count_published(const int64_t* row, const int64_t* col, const int32_t* csr_col /* NULL ok */,
                                              const float* edge_weight /* NULL ok */, int64_t num_edges,
                                              const int64_t* cluster_index, int64_t num_nodes, int64_t num_supernodes,
                                              const int32_t* assign_row_ptr, const int32_t* assign_perm,
                                              const int32_t* csr_ptr /* NULL ok */, int reduce_op, int flags, float eps,
                                              void* ws, size_t ws_bytes, int64_t* d_count, uint64_t* status,
                                              int64_t status_words, uint64_t* result, uint32_t epoch, void* stream);
/* r5: the same row-local pipeline for float64 edge weights (they took the general sort-based route before: 0.6 ms
 * against 0.24 at C4).  Values are staged, merged (sum / mean / min / max / mul) and eps-filtered in double, as the
 * reference's coalesce does for a double tensor (connect/base_conn.py:86-89).  Workspace of ..._workspace_bytes_f64;
 * TGP_HUGE_ROWS is refused (float32 only): a list with a supernode row beyond 1024 raw entries answers -5 and the caller
 * runs tgp_connect_coalesce_count_f64.  tgp_connect_coalesce_rows_fill_f64 follows a count >= 0. */
size_t tgp_connect_coalesce_rows_workspace_bytes_f64(int64_t num_edges, int64_t num_nodes, int64_t num_supernodes);
int tgp_connect_coalesce_rows_count_published_f64(const int64_t* row, const int64_t* col, const int32_t* csr_col /* NULL ok */,
                                                  const double* edge_weight, int64_t num_edges,
                                                  const int64_t* cluster_index, int64_t num_nodes, int64_t num_supernodes,
                                                  const int32_t* assign_row_ptr, const int32_t* assign_perm,
                                                  const int32_t* csr_ptr /* NULL ok */, int reduce_op, int flags,
                                                  double eps, void* ws, size_t ws_bytes, int64_t* d_count,
                                                  uint64_t* status, int64_t status_words, uint64_t* result,
                                                  uint32_t epoch, void* stream);
int tgp_connect_coalesce_rows_fill_f64(const void* ws, int64_t num_edges, int64_t num_nodes, int64_t num_supernodes,
                                       int64_t num_out, int64_t* out_row, int64_t* out_col, double* out_weight,
                                       void* stream);

/* A4 + A6, row-sorted input, as ONE heavy kernel + a widening fill (r3).  Every workgroup derives its rows' member
 * edge ranges, LDS slots and survivor counts locally; the survivors in front of it come from a decoupled look-back, so
 * weights are written once, at their final place, into `out_weight_cap` (capacity num_edges: the first *d_count
 * entries are the result), and tgp_connect_coalesce_fused_fill only widens the columns and generates the rows.
 * Optional CSR of the SAME edge list (csr_ptr [N+1], csr_col [E], int32; e.g. the one GraclusSelect builds of a
 * symmetric input): the pass over `row` (CSR offsets + sortedness check) is skipped and 4-byte columns are streamed;
 * row / col may then be NULL.  *d_count: >= 0 the output size; -1 declined (unsorted rows, a supernode row of more
 * than 1024 raw entries, ...: use the radix routes); -3 declined by this kernel's tile limit only (more than 256
 * members in a tile of rows): tgp_connect_coalesce_rows_{count,fill} takes the call.  Output identical to the other
 * coalesce routes. */
size_t tgp_connect_coalesce_fused_workspace_bytes(int64_t num_edges, int64_t num_nodes, int64_t num_supernodes);
int tgp_connect_coalesce_fused_count(const int64_t* row, const int64_t* col, const int32_t* csr_ptr /* NULL ok */,
                                     const int32_t* csr_col /* NULL ok */, const float* edge_weight /* NULL ok */,
                                     int64_t num_edges, const int64_t* cluster_index, int64_t num_nodes,
                                     int64_t num_supernodes, const int32_t* assign_row_ptr,
                                     const int32_t* assign_perm, int reduce_op, int flags, float eps,
                                     float* out_weight_cap /* [num_edges] when weighted */, void* ws, size_t ws_bytes,
                                     int64_t* d_count, void* stream);
int tgp_connect_coalesce_fused_fill(const void* ws, int64_t num_edges, int64_t num_nodes, int64_t num_supernodes,
                                    int64_t num_out, int64_t* out_row, int64_t* out_col, void* stream);

/* A1 + A2 + (A5 | A4) + A6 filters for a BATCH OF SMALL GRAPHS in ONE launch (r4): sparse Reduce
 * (reduce/base_reduce.py:14-53,141-155) and sparse Connect (connect/base_conn.py:79-89 + the self-loop / |w| > eps
 * filters of utils/ops.py:370-380) of a PyG-style batch whose `batch` vector is sorted and whose graphs have at most
 * tgp_sparse_pool_small_max_graph_nodes() nodes: one wave per graph.  `graph_ptr` [B+1] = node offsets of the graphs.
 *   mode 0 (kept-node selection: TopK, NDP-shaped S): node_index ascending, one supernode per kept node, numbered
 *          graph-major; induced subgraph, endpoints relabelled to their position in node_index, input edge order kept.
 *   mode 1 (every node in exactly one cluster: Graclus, ...): node_index = 0..N-1, cluster ids contiguous per graph and
 *          ascending over the graphs; endpoints mapped through cluster_index, duplicates merged with `reduce_op` in input
 *          order, output in (row, col) order (PyG coalesce).
 * Outputs: x_pool [K,F], batch_pool [K] (NULL ok), and the surviving edges written ONCE at their final offsets of the
 * capacity-E buffers out_row / out_col / out_weight (NULL iff edge_weight is NULL): the first `total` entries are the
 * result, identical to tgp_reduce_sparse_f32 + tgp_reduce_batch_i64 + tgp_connect_{subgraph,coalesce_*}_{count,fill}.
 * `status` (>= tgp_sparse_pool_small_status_words(B, mode) 64-bit words of device memory, caller-owned, kept between
 * calls on ONE stream, never cleared: every word carries `epoch` in its bits 34.., 0 < epoch < 2^29, a different value
 * for every call on that buffer) holds the look-back state.  `*result` receives ONE word when the last graph is done:
 * bits 34.. = epoch, bit 31 = refused (a precondition above does not hold, checked on the device -- an edge leaving its
 * graph, unsorted rows, a graph too large, more than 512 edges in a mode-1 graph, ...: outputs are then unspecified
 * and the caller takes the staged entry points), bits 0..30 = total.  It is stored with system scope, so `result` may
 * point into pinned host memory that the caller polls for the call's epoch (the call's one host wait: no copy kernel,
 * no stream synchronise); with a device pointer the caller copies the word back after the launch.
 * `edge_ptr` / `assign_ptr` (NULL ok; [B+1] int64): the first edge / first assignment (mode 0) of every graph, when the
 * caller has them -- tgp_graph_lower_bounds_i64 of graph_ptr in `row` (worth keeping per edge list and batch vector) and
 * TopkSelect's keep-count prefix.  The kernel then skips its own searches (three dependent rounds + a boundary pass: 5.8
 * of 13.4 us on 2048 PROTEINS-shaped graphs); nothing is trusted -- the ranges must tile the arrays, every edge and kept
 * node is range-checked as without them, a wrong table is a refusal. */
int tgp_sparse_pool_small_max_graph_nodes(void);
int64_t tgp_sparse_pool_small_status_words(int64_t num_graphs, int mode);
/* out[g] = first position of the ascending `values` [n] that is >= graph_ptr[g], g = 0 .. num_graphs. */
int tgp_graph_lower_bounds_i64(const int64_t* values, int64_t n, const int64_t* graph_ptr, int64_t num_graphs,
                               int64_t* out /* [num_graphs + 1] */, void* stream);
int tgp_sparse_pool_small_f32(const float* x, int64_t num_nodes, int64_t num_features, int64_t x_row_stride,
                              const int64_t* graph_ptr /* [B+1] */, int64_t num_graphs,
                              const int64_t* edge_ptr /* NULL ok */, const int64_t* assign_ptr /* NULL ok */,
                              int64_t* edge_ptr_out /* NULL ok; [B+1]: r5 -- a call WITHOUT edge_ptr leaves the edge
                                                       ranges it searched for here (valid when the call is not refused):
                                                       a new edge list costs no tgp_graph_lower_bounds_i64 launch, the
                                                       same list pooled again gets them back as edge_ptr */,
                              const int64_t* row,
                              const int64_t* col, const float* edge_weight /* NULL ok */, int64_t num_edges,
                              const int64_t* node_index, const int64_t* cluster_index,
                              const float* weight /* NULL = ones */, int64_t nnz, int64_t num_supernodes, int mode,
                              int reduce_op, int flags, float eps, float* x_pool, int64_t* batch_pool /* NULL ok */,
                              int64_t* out_row, int64_t* out_col, float* out_weight, uint64_t* status,
                              int64_t status_words, uint64_t* result /* device-ACCESSIBLE: may be pinned host memory */,
                              uint32_t epoch, void* stream);

/* A4 for edge lists in ANY order, two-level: a stable radix sort by supernode row only (log2 K bits instead of the
 * 2 log2 K bits of the (row, col) key above) carrying (cluster column, weight) as payload, then the same in-row
 * sort / merge as the row-sorted path.  Same output as the other two pairs.  *d_count = -1 if a supernode row
 * exceeds the in-LDS sort (1024 raw entries): use tgp_connect_coalesce_{count,fill} then.  The fill half is
 * tgp_connect_coalesce_rows_fill with this workspace. */
size_t tgp_connect_coalesce_grouped_workspace_bytes(int64_t num_edges, int64_t num_nodes, int64_t num_supernodes);
int tgp_connect_coalesce_grouped_count(const int64_t* row, const int64_t* col, const float* edge_weight /* NULL ok */,
                                       int64_t num_edges, const int64_t* cluster_index, int64_t num_nodes,
                                       int64_t num_supernodes, int reduce_op, int flags, float eps, void* ws,
                                       size_t ws_bytes, int64_t* d_count, void* stream);

/* A6 (rest)  degree / per-graph max normalisation of a pooled edge list, in place
 * (utils/ops.py:383-417).  edge_weight must be initialised (ones when the list was
 * unweighted, ops.py:384-385).  ws: tgp_postprocess_sparse_workspace_bytes().           */
size_t tgp_postprocess_sparse_workspace_bytes(int64_t num_edges, int64_t num_nodes, int64_t num_graphs);
int tgp_postprocess_sparse_norm_f32(const int64_t* row, const int64_t* col, float* edge_weight,
                                    int64_t num_edges, int64_t num_nodes, int flags, float eps,
                                    const int64_t* batch_pooled /* needed for EDGE_WEIGHT_NORM */,
                                    int64_t num_graphs, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * A3 + A7 + A8  dense pooling of a padded batch
 *   x_pool  [B,K,F] = S^T X                  (reduce/base_reduce.py:158-161)
 *   adj_raw [B,K,K] = S^T A S                (connect/dense_conn.py:111-122)
 *   adj_pool[B,K,K] = postprocess(adj_raw)   (utils/ops.py:282-335)
 * S [B,N,K], X [B,N,F] contiguous fp32; A [B,N,N] contiguous, or its transposed view when
 * TGP_ADJ_TRANSPOSED is set (then element (b,i,j) is read from A[b*N*N + j*N + i]).
 * x / x_pool, adj_raw, adj_pool may each be NULL to skip that product.  MinCut
 * (poolers/mincut.py:226-237) asks for adj_raw AND adj_pool; DiffPool only adj_pool.
 * graph_sizes (optional): graph b's real nodes are its first graph_sizes[b] rows and everything beyond them in
 * S, A, X is zero (the layout of to_dense_batch / to_dense_adj, src.py:434-450); kernels then stop at the real
 * size instead of the padded one.  NULL = every row may be non-zero.
 * Graphs beyond the one-wave / one-workgroup kernels take U = A S, S^T [U | X] split over N into partial slabs, and a
 * slab combine with the post-processing; where U = A S runs one 128-column tile (K <= 128, K and F multiples of 4,
 * F <= 64, N <= 1024, at least 256 row tiles of 128) the second product is folded into the first launch: one partial
 * slab per 128-row tile, U never in memory.  The workspace is sized for the larger slab count of the two routes.
 * ---------------------------------------------------------------------------------- */
size_t tgp_dense_pool_workspace_bytes(int64_t B, int64_t N, int64_t K, int64_t F);
int tgp_dense_pool_f32(const float* S, const float* A, const float* X, int64_t B, int64_t N, int64_t K,
                       int64_t F, int flags, float eps, const int64_t* graph_sizes /* [B] or NULL */, float* x_pool,
                       float* adj_raw, float* adj_pool, void* ws, size_t ws_bytes, void* stream);

/* The same call for batches the one-wave-per-graph kernel takes (tgp_dense_pool_is_small(B,N,K,F) != 0: N <= 64,
 * K, F <= 32, B >= 64), which can also leave the per-graph tails of MinCut's two auxiliary losses in
 * mincut_terms [2,B] while S, A and the raw S^T A S sit in registers / LDS (poolers/mincut.py:226-237 computes them
 * between Reduce and Connect): [0,b] = -trace(S^T A S) / (trace(S^T D S) + loss_eps) (utils/losses.py:39-56),
 * [1,b] = || S^T S / ||S^T S||_F - I / sqrt(K) ||_F (utils/losses.py:59-70). */
int tgp_dense_pool_is_small(int64_t B, int64_t N, int64_t K, int64_t F);
int tgp_dense_pool_mincut_f32(const float* S, const float* A, const float* X, int64_t B, int64_t N, int64_t K,
                              int64_t F, int flags, float eps, float loss_eps, float* x_pool, float* adj_raw,
                              float* adj_pool, float* mincut_terms, void* ws, size_t ws_bytes, void* stream);

/* The same call with the selector folded in (A13 + A3 + A7 + A8 in ONE launch, same batches): S = softmax(X W^T + b) * mask
 * (select/mlp_select.py:105-147 for a single Linear; W [K,F], bias [K] or NULL, mask [B,N] bytes or NULL) is formed by the
 * graph's wave from the X it has just loaded, written once to S_out [B,N,K] (SelectOutput.s) and used from registers. */
int tgp_dense_pool_select_f32(const float* X, const float* A, const float* W, const float* bias,
                              const unsigned char* mask, int64_t B, int64_t N, int64_t K, int64_t F, int flags,
                              float eps, float loss_eps, float* S_out, float* x_pool, float* adj_raw, float* adj_pool,
                              float* mincut_terms /* [2,B] or NULL */,
                              int64_t* batch_pool /* [B*K] or NULL: arange(B).repeat_interleave(K), utils/ops.py:152-169 */,
                              void* stream);

/* r5: the same call on the batch as a PyG loader hands it over -- x [Ntot,F] un-padded, a ROW-SORTED edge list
 * (row, col, w or NULL = ones; E entries), batch [Ntot] sorted, node_ptr / edge_ptr [B+1] = first node / first edge of
 * every graph.  The graph's wave builds its adjacency tile in LDS from its edges (duplicates summed, entries beyond N
 * dropped, a column of another graph placed by its local id there: to_dense_adj, src.py:434-443; adj_transpose != 0:
 * the transposed scatter of src.py:442-443), reads its own rows of x, and writes S_out [B,N,K] (zero rows behind the
 * graph's nodes) and mask_out [B,N] (to_dense_batch's mask): neither to_dense_batch nor to_dense_adj runs and no [B,N,N]
 * tensor exists -- three launches -> one in front of a dense pooler on sparse inputs.  N = the longest graph (<= 64).
 * The caller guarantees the row order and the ranges (tgp_graph_lower_bounds_i64, or tgp_edge_facts_sorted_i64 below,
 * whose flag word may be read AFTER this launch: what is read through edge_ptr is clamped to [0, E], columns outside
 * [0, Ntot) are dropped).  x_dense_out / adj_dense_out (optional): the zero-padded x and the adjacency tiles as the kernel
 * holds them, for a training step -- the backward kernels read the padded tensors; what to_dense_batch / to_dense_adj
 * would have written, without their launches and without the zero fill. */
int tgp_dense_pool_select_sparse_f32(const float* x, int64_t Ntot, const int64_t* row, const int64_t* col, const float* w,
                                     int64_t E, const int64_t* batch, const int64_t* node_ptr, const int64_t* edge_ptr,
                                     const float* W, const float* bias, int64_t B, int64_t N, int64_t K, int64_t F,
                                     int flags, int adj_transpose, float eps, float loss_eps, float* S_out,
                                     unsigned char* mask_out, float* x_pool, float* adj_raw, float* adj_pool,
                                     float* mincut_terms /* [2,B] or NULL */, int64_t* batch_pool /* [B*K] or NULL */,
                                     float* x_dense_out /* [B,N,F] or NULL */, float* adj_dense_out /* [B,N,N] or NULL */,
                                     float* diff_stats /* r6, [B,4] or NULL: (sum A^2, trace(S^T A S), |S^T S|_F^2,
                                                          sum -S log(S + loss_eps)) per graph: DiffPool's two losses
                                                          (utils/losses.py:644-658, 476-483) without the dense adjacency */,
                                     void* stream);
/* r6: the same records from the one-wave-per-graph kernel on PADDED inputs (x [B,N,F], adj [B,N,N]; what the second
 * pooling layer of a hierarchical model is handed): S [B,N,K] given (W = NULL), or the selector folded in (S = NULL: W
 * [K,F], bias, mask [B,N] bytes or NULL; S_out [B,N,K] is written).  Batches tgp_dense_pool_is_small accepts. */
int tgp_dense_pool_small_diff_f32(const float* S, const float* A, const float* X, const float* W, const float* bias,
                                  const unsigned char* mask, int64_t B, int64_t N, int64_t K, int64_t F, int flags,
                                  float eps, float loss_eps, float* S_out, float* x_pool, float* adj_raw, float* adj_pool,
                                  float* diff_stats /* [B,4] */, int64_t* batch_pool /* [B*K] or NULL */, void* stream);
/* r6: DiffPool's link-prediction and entropy losses from those records: out2[0] = sqrt(max(sum_b (a2 - 2 tr + fro), 0)) *
 * link_scale, out2[1] = (sum_b ent) * ent_scale; one launch (the residual product, its partial sum, the entropy pass and
 * the tail were four). */
int tgp_diffpool_stats_tail_f32(const float* stats /* [B,4], 16-byte aligned */, int64_t B, float link_scale,
                                float ent_scale, float* out2, void* stream);

/* Facts of a NEW edge list for that call, one launch, no host round trip in front of the consumer: edge_ptr [N+2]
 * (entries [0, B] written: first entry whose source node belongs to a graph >= g) and one flag word in pinned host
 * memory (result[2]; result[0] = tag stored last): 1 = rows not grouped by ascending source node, 2 = a source id outside
 * [0, N), 4 = more than 64 consecutive graph ids without an entry.  ticket: two zeroed uint32 words owned by the caller
 * per (device, stream), left zero (not the pair of tgp_batch_facts_sorted_i64).  E > 0, N > 0, batch sorted. */
int tgp_edge_facts_sorted_i64(const int64_t* row, int64_t E, const int64_t* batch, int64_t N, int64_t* edge_ptr,
                              uint32_t* ticket, uint64_t* result, uint64_t tag, void* stream);

/* Backward of that call for the same batches (what autograd derives operator by operator from base_reduce.py:158-161,
 * dense_conn.py:111-122, utils/ops.py:282-335 and utils/losses.py:39-70: ~80 launches in a MinCut training step), ONE
 * launch: from the upstream gradients of x_pool [B,K,F], of the post-processed adj_pool [B,K,K], of the raw S^T A S
 * [B,K,K] and of the two per-graph terms [2,B] (each may be NULL = zero) it writes gS [B,N,K] and, when gX is given,
 * gX [B,N,F].  flags as in the forward call (TGP_EDGE_WEIGHT_NORM is refused); A receives no gradient.
 * DiffPool's two batch-wide losses (utils/losses.py:644-658) ride along when diff_losses [2] (their forward values,
 * tgp_diffpool_loss_tail_f32's output) and g_link / g_ent (device scalars: the upstream gradients of
 * link = link_scale * ||A - S S^T||_F and ent = ent_scale * sum(-S log(S + ent_eps)); each may be NULL) are given.
 * r5: g_mean_cut / g_mean_ortho (device scalars, each may be NULL): upstream gradients of the MEANS over the batch of
 * the two per-graph terms -- what poolers/mincut.py:226-237 returns as cut_loss / ortho_loss -- added to g_terms[.,b]
 * as *g / B inside the kernel; grad_bcast bit 0 / bit 1: g_x_pool / g_adj_pool points at ONE value that stands for
 * every element (the gradient of `x_pool.sum()` arrives from autograd as an expanded scalar; no [B,K,F] copy is made). */
int tgp_dense_pool_small_bwd_f32(const float* S, const float* A, const float* X, int64_t B, int64_t N, int64_t K,
                                 int64_t F, int flags, float eps, float loss_eps, const float* g_x_pool,
                                 const float* g_adj_pool, const float* g_adj_raw, const float* g_terms,
                                 const float* g_mean_cut, const float* g_mean_ortho, const float* g_link,
                                 const float* g_ent, const float* diff_losses, float link_scale, float ent_scale,
                                 float ent_eps, int grad_bcast, float* gS, float* gX, void* stream);

/* Generic batched fp32 GEMM on the matrix cores, C[b] = op(A[b]) B[b] with B[b] [Kd,Nc] row-major.
 * trans_a = 0: A[b] is [M,Kd] row-major; 1: A[b] is stored [Kd,M] (C = A^T B).  Used by
 * BaseLift (lift/base_lift.py:138-247: S_inv^T X_pool) and exposed for callers' own products. */
int tgp_bmm_f32(const float* A, const float* Bm, float* C, int64_t batch, int64_t M, int64_t Nc, int64_t Kd,
                int trans_a, int64_t lda, int64_t ldb, int64_t ldc, int64_t sA, int64_t sB, int64_t sC,
                void* stream);
/* C += op(A) Bm, same arguments (r4): a second product accumulates in the GEMM epilogue into the buffer the first one
 * wrote (two-term gradients of the dense Connect under autograd) */
int tgp_bmm_accumulate_f32(const float* A, const float* Bm, float* C, int64_t batch, int64_t M, int64_t Nc, int64_t Kd,
                int trans_a, int64_t lda, int64_t ldb, int64_t ldc, int64_t sA, int64_t sB, int64_t sC,
                void* stream);

/* A3' / A7'  un-padded batch (reduce/base_reduce.py:170-182, connect/dense_conn.py:195-206):
 * C[b] = S_b^T Y_b where graph b owns node rows ptr[b]..ptr[b+1] of S [Ntot,K] and Y [Ntot,F].
 * One launch instead of the reference's Python loop over graphs. max_nodes = max_b (ptr[b+1]-ptr[b]).
 * Long graphs are split along their node range across workgroups; the partial products live in the
 * workspace and are added in a fixed order. */
size_t tgp_segment_gemm_tn_workspace_bytes(int64_t B, int64_t K, int64_t F, int64_t max_nodes);
int tgp_segment_gemm_tn_f32(const float* S, const float* Y, const int64_t* ptr, float* C, int64_t B,
                            int64_t Ntot, int64_t K, int64_t F, int64_t max_nodes, void* ws, size_t ws_bytes,
                            void* stream);

/* Row-side counterpart on the same un-padded batch: C[rows of graph b] = A[rows of graph b] Bm[b] with
 * A [Ntot,Kd], Bm [B,Kd,Nc], C [Ntot,Nc].  BaseLift on dense [N,K] assignments with a batch vector
 * (lift/base_lift.py:138-247 loops over graphs) and the backward of tgp_segment_gemm_tn_f32
 * (dS_b = Y_b G_b^T, dY_b = S_b G_b). */
int tgp_segment_gemm_nn_f32(const float* A, const float* Bm, const int64_t* ptr, float* C, int64_t B,
                            int64_t Ntot, int64_t Kd, int64_t Nc, int64_t max_nodes, void* stream);

/* ----------------------------------------------------------------------------------
 * A12  TopkSelect, ratio mode (select/topk_select.py:163-203 -> PyG topk(score, ratio, batch), then the
 * row sort of SelectOutput, select/base_select.py:58).  Graph g keeps its k[g] highest-scoring nodes; kept
 * node i becomes supernode koff[g] + (its rank in the graph's descending score order), ties by lower node id.
 *   ptr  [B+1] exclusive prefix sums of the graph sizes,  k [B],  koff [B+1] exclusive prefix sums of k.
 * Outputs (k_total = koff[B] entries, ordered by ascending node id = the reference's row-sorted COO):
 *   node_index, cluster_index (int64) and assign_perm (int32): assign_perm[c] = position of supernode c's
 *   single assignment, i.e. the inverted index the sparse Reduce consumes (tgp_assign_index_build's perm).
 * batch may be NULL when B == 1.  segments_max_nodes > 0 promises that the batch vector is sorted (graph g owns nodes
 * ptr[g] .. ptr[g+1]) and that no graph has more nodes than that: graphs are then sorted one per wave / workgroup
 * instead of by a device-wide radix sort (0 = no promise). */
int tgp_topk_plan(const int64_t* sizes, int64_t B, double ratio, int64_t* k /* [B] */, int64_t* koff /* [B+1] */,
                  void* stream); /* k[g] = ceil(fp32(ratio) * n_g) (ratio < 1) or min(ratio, n_g); koff = prefix sums */
size_t tgp_topk_select_workspace_bytes(int64_t N);
int tgp_topk_select(const float* score, const int64_t* batch, int64_t N, int64_t B, const int64_t* ptr,
                    const int64_t* k, const int64_t* koff, int64_t segments_max_nodes, void* ws, size_t ws_bytes,
                    int64_t* node_index, int64_t* cluster_index, int32_t* assign_perm,
                    float* values /* optional [k_total]: score[node_index], the weights of S */,
                    int32_t* lift_row_ptr /* optional [N+1]: CSR offsets of the node -> assignment index (the
                                             transposed index Reduce's backward and Lift walk; its perm is the identity) */,
                    uint64_t* assign_pack /* optional [k_total]: the packed one-to-one index of
                                             tgp_reduce_one_to_one_f32, {node id, score} of supernode c */,
                    uint32_t* member_bits /* optional, with rank128 and directory_written (r5): by-products for the
                                             subgraph Connect of the SAME selection -- the kept-node bitmap
                                             [4 * tgp_topk_select_directory_blocks(N)] and */,
                    uint32_t* rank128 /* the rank directory [..._directory_blocks(N)]: kept nodes with id < 128 b; hand
                                         both to tgp_connect_subgraph_single (member_bits_in / rank128_in) */,
                    int* directory_written /* HOST int: 1 when this call wrote them (the device-wide route, i.e. large
                                              graphs; the per-graph sort routes of small-graph batches do not) */,
                    void* stream);
int64_t tgp_topk_select_directory_blocks(int64_t N);

/* ----------------------------------------------------------------------------------
 * A14  GraclusSelect's matching (select/graclus_select.py:62-81 -> torch_cluster 1.6.3 graclus_cluster, absent
 * from the reference tree; its published algorithm: pair every node with its heaviest unmatched neighbour).
 * Data-parallel handshake rounds over the CSR of the edge list (row_ptr / perm = tgp_assign_index_build of the
 * source ids; perm may be NULL when the list is already sorted by source, with row_ptr from
 * tgp_rowptr_from_sorted_i64); label[i] = min(i, partner) or i.  _start gathers the CSR and resets the state,
 * _rounds runs `rounds` propose/match rounds and sets matched[r] = 1 if round r formed a pair (device memory):
 * the matching is maximal once a round matches nothing.  _start also symmetrises the list (a pair weighs the larger
 * of its two directions, entries without a reverse are ignored): pairs form by mutual proposal. */
size_t tgp_graclus_match_workspace_bytes(int64_t num_nodes, int64_t num_edges);
int tgp_graclus_match_start(const int64_t* row, const int64_t* col, const float* weight /* NULL = ones */, const int32_t* row_ptr,
                            const int32_t* perm, int64_t num_nodes, int64_t num_edges, void* ws, size_t ws_bytes,
                            int64_t* label, int init_state /* 1; 0 only in front of tgp_graclus_match_graphs, which sets
                                                              the labels itself and keeps its free flags in LDS */,
                            void* stream);
int tgp_graclus_match_rounds(const int32_t* row_ptr, int64_t num_nodes, int64_t num_edges, void* ws, int rounds,
                             unsigned int* matched, int64_t* label, void* stream);
/* The remaining rounds in two launches once at most 16384 free nodes are left (after tgp_graclus_match_rounds, same
 * workspace): one workgroup runs them over the list of those nodes (same pairs: a proposal depends on the free set
 * only).  *d_status = 1: the matching is now maximal; 0: too many free nodes, nothing was changed. */
int tgp_graclus_match_tail(const int32_t* row_ptr, int64_t num_nodes, int64_t num_edges, void* ws, int64_t* label,
                           int* d_status, void* stream);
/* All rounds of every graph in ONE launch (instead of tgp_graclus_match_rounds, after tgp_graclus_match_start) for a
 * batch whose graphs own contiguous node ranges graph_ptr[b] .. graph_ptr[b+1] of at most
 * tgp_graclus_match_max_graph_nodes() nodes: one workgroup per graph, the matching the device-wide rounds give.
 * max_graph_nodes: the caller's bound on the longest graph (64 or less: one wave per graph).
 * *d_status != 0: not applicable (1: a graph longer than the bound, 2: an entry that leaves its graph); the caller
 * then runs tgp_graclus_match_start + _rounds again. */
int tgp_graclus_match_max_graph_nodes(void);
int tgp_graclus_match_graphs(const int32_t* row_ptr, int64_t num_nodes, int64_t num_edges, void* ws,
                             const int64_t* graph_ptr, int64_t num_graphs, int64_t max_graph_nodes, int64_t* label,
                             int* d_status, void* stream);
/* r4: the whole GraclusSelect of a sorted batch of SMALL graphs in ONE launch -- matching (select/graclus_select.py:66, the
 * pairs of tgp_graclus_match_graphs), consecutive cluster ids (`:68-70`, as tgp_graclus_relabel_i64) and the supernode ->
 * members index -- from the row-sorted edge list itself (no CSR, no workspace): one wave per graph of at most
 * tgp_graclus_match_graphs_fused_max_graph_nodes() (= 64) nodes and 512 entries.  index [2, N] int64 (row 0 = 0..N-1, row
 * 1 = cluster id), assign_row_ptr [N + 1] / assign_perm [N] int32 (the first K + 1 offsets are written), ones [N] fp32,
 * label [N] int64 (NULL ok: the pair's smaller node id).  `status` / `epoch` / `*result` as for tgp_sparse_pool_small_f32:
 * *result = {epoch << 34 | K}, or {epoch << 34 | 1 << 31 | ...} when the kernel refused (a graph beyond 64 nodes or 512
 * entries, an entry that leaves its graph, rows not ascending): run tgp_graclus_match_start + _graphs / _rounds then. */
int tgp_graclus_match_graphs_fused_max_graph_nodes(void);
int64_t tgp_graclus_match_graphs_fused_status_words(int64_t num_graphs);
int tgp_graclus_match_graphs_fused(const int64_t* row, const int64_t* col, const float* edge_weight /* NULL ok */,
                                   int64_t num_nodes, int64_t num_edges, const int64_t* graph_ptr, int64_t num_graphs,
                                   const int64_t* edge_ptr /* NULL ok: tgp_graph_lower_bounds_i64 of graph_ptr in row */,
                                   int64_t* label /* NULL ok */, int64_t* index, int32_t* assign_row_ptr,
                                   int32_t* assign_perm, float* ones, uint64_t* status, int64_t status_words,
                                   uint64_t* result, uint32_t epoch, void* stream);
/* Matching labels -> consecutive cluster ids, the torch.unique(cluster, return_inverse=True) of the reference's
 * select/graclus_select.py:66-70 without a sort (representatives label[r] == r keep their order, which is the order
 * unique() gives: the label of a pair is its smaller node id).  index_out [2, N] int64: row 0 = 0..N-1, row 1 = ids;
 * *d_k = number of ids.  N <= tgp_graclus_relabel_max_nodes(). */
int64_t tgp_graclus_relabel_max_nodes(void);
size_t tgp_graclus_relabel_workspace_bytes(int64_t num_nodes);
int tgp_graclus_relabel_i64(const int64_t* label, int64_t num_nodes, void* ws, size_t ws_bytes, int64_t* index_out,
                            int64_t* d_k,
                            int32_t* assign_row_ptr /* optional [N + 1] (the first K + 1 entries are written) */,
                            int32_t* assign_perm /* optional [N]; both or neither: the supernode -> members index the
                                                    sparse Reduce and the coalesce Connect walk (what
                                                    tgp_assign_index_build derives from the ids), valid when every
                                                    label is shared by at most two nodes -- a matching */,
                            float* ones /* optional [N]: filled with 1.0f, the values of the assignment matrix */,
                            void* stream);

/* k-MIS selection (select/kmis_select.py; csrc/kmis_select.hip).  A node's priority is the 64-bit key (prio << 32) | node,
 * smaller first: prio = the node's rank in a caller's permutation, or its updated score's bits in descending order, so ties
 * go to the lower node index.  Every entry writes label [N] int64 = the MIS node that owns each node (an MIS node owns
 * itself); tgp_graclus_relabel_i64 turns the owners into consecutive ids in ascending owner order.
 *
 * tgp_kmis_graphs: a sorted batch (graph_ptr [B + 1]) whose longest graph has at most max_graph_nodes <=
 * tgp_kmis_max_graph_nodes() nodes, one workgroup per graph, all rounds in LDS, one launch.  mode 0: rank [N] int32;
 * 1: score [N] compared as it is; 2: score / (A^T + I)^k 1 ("greedy", integer counts), also written to updated [N].
 * words[0] != 0: declined (bit 0: an edge list that is not grouped by graph, an edge between two graphs, a graph longer
 * than declared; bit 1: the round bound) -- the caller runs the device-wide entries instead.
 *
 * Device-wide: tgp_kmis_rounds_start (keys from rank, or from updated when rank is null; ws of
 * tgp_kmis_workspace_bytes(N)), then tgp_kmis_rounds any number of times (round_base = rounds launched so far;
 * open_flags[j] = 1 when round j still met an unmasked node, so the first 0 says the set is maximal; 2 * order_k launches
 * per round), then tgp_kmis_clusters (rounds_done = rounds launched in all).
 *
 * tgp_kmis_greedy_f32: updated = score / (A^T + I)^k 1 device-wide (uses the same workspace, before the rounds).
 * tgp_kmis_wsum_f32: out[c] = in[c] + sum of in[row[e]] over the edges e into c in the order of the by-destination index
 * (grp_ptr [N + 1], grp_perm [E] of tgp_assign_index_build over col: edge-list order inside a group); with score,
 * out[c] = score[c] / that sum ("w-greedy": one call per hop, score on the last).  tgp_kmis_degree_f32: the weighted
 * in-degree in the same order (w null: the edge count).  tgp_kmis_mis_index_i64: mis[id] = owner of cluster id. */
int tgp_kmis_max_graph_nodes(void);
size_t tgp_kmis_workspace_bytes(int64_t num_nodes);
int tgp_kmis_graphs(const int64_t* row, const int64_t* col, int64_t num_edges, int64_t num_nodes, const int64_t* graph_ptr,
                    int64_t num_graphs, int max_graph_nodes, int order_k, int mode, const float* score,
                    const int32_t* rank, float* updated, int64_t* label, int32_t* words, void* stream);
int tgp_kmis_rounds_start(const int32_t* rank, const float* updated, int64_t num_nodes, void* ws, size_t ws_bytes,
                          void* stream);
int tgp_kmis_rounds(const int64_t* row, const int64_t* col, int64_t num_edges, int64_t num_nodes, int order_k, void* ws,
                    int64_t round_base, int rounds, int32_t* open_flags, void* stream);
int tgp_kmis_clusters(const int64_t* row, const int64_t* col, int64_t num_edges, int64_t num_nodes, int order_k, void* ws,
                      int64_t rounds_done, int64_t* label, void* stream);
int tgp_kmis_greedy_f32(const int64_t* row, const int64_t* col, int64_t num_edges, int64_t num_nodes, int order_k,
                        const float* score, void* ws, size_t ws_bytes, float* updated, void* stream);
int tgp_kmis_wsum_f32(const int64_t* row, const int32_t* grp_ptr, const int32_t* grp_perm, const float* in,
                      const float* score, int64_t num_nodes, float* out, void* stream);
int tgp_kmis_degree_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const float* w, int64_t num_nodes, float* out,
                        void* stream);
int tgp_kmis_mis_index_i64(const int64_t* label, const int64_t* index, int64_t num_nodes, int64_t* mis, void* stream);

/* Edge-contraction selection (select/edge_contraction_select.py; csrc/edge_contract.hip; appended under ABI 10044).
 *
 * Scores.  tgp_edge_contract_project_f32: p [2 N] with p[i] = <x[i,:], w[:F]> and p[N + i] = <x[i,:], w[F:]>, w [2 F] the
 * weight row of Linear(2 F, 1), one pass over x [N, F] (row stride ldx).  tgp_edge_contract_raw_f32: raw[e] = p[row[e]] +
 * p[N + col[e]] + bias[0] (bias on the device, null = 0; an entry with an endpoint outside [0, N) gets 0) -- the
 * reference's lin(cat(x[row], x[col])) without the E x 2F matrix.  tgp_edge_contract_normalize_f32: out[e] = f(raw)[e] +
 * add, method 0 = softmax over the entries that share col[e], 1 = tanh, 2 = sigmoid.  The softmax walks the
 * by-destination index (grp_ptr [N + 1], grp_perm [E] of tgp_assign_index_build over col) in a fixed order without float
 * atomics, so a target with one incoming entry scores exactly 1 + add; seg [2 N] fp32, 8-byte aligned (each target's
 * {maximum, sum} pair on return) and hubs [hub_cap + 1] int32, hub_cap >= E / tgp_edge_contract_hub_degree(), are scratch (targets with more
 * incoming entries than that degree take a workgroup each).  raw and out are different arrays.
 *
 * Matching (maximal_matching, `:14-73`).  An entry's priority is the 64-bit key (prio << 32) | position, smaller first:
 * prio = rank [E] int32 (the entry's rank in a caller's permutation) or, rank null, the bits of score [E] in descending
 * order, so ties go to the lower position.  E < 2^32 (TGP_ERR_RANGE otherwise).  Outputs: match [E] bytes (1 = matched),
 * label [N] int64 (label[col[m]] = row[m] for a matched entry m, label[i] = i otherwise: tgp_graclus_relabel_i64 turns it
 * into consecutive ids), medge [N] int64 (the matched entry of a node, -1 for a singleton).
 * tgp_edge_contract_graphs: a sorted batch (graph_ptr [B + 1]) whose longest graph has at most max_graph_nodes <=
 * tgp_edge_contract_max_graph_nodes() nodes, one workgroup per graph, all rounds in LDS (the first
 * tgp_edge_contract_edge_cache() entries of a graph too), one launch.  words [2] int32: words[0] != 0: declined (bit 0: a
 * list that is not grouped by graph, an entry between two graphs, a graph longer than declared; bit 1: the round bound)
 * -- the caller runs the device-wide entries instead; words[1] = rounds of the slowest graph.
 * Device-wide: tgp_edge_contract_rounds_start (ws of tgp_edge_contract_workspace_bytes(N); clears match, label, medge),
 * then tgp_edge_contract_rounds any number of times (round_base = rounds launched so far; open_flags[j] = 1 when round j
 * still met a live entry, so the first 0 says the matching is maximal; two launches per round, and the rounds of a call
 * behind such a 0 leave without reading the edge list).
 * tgp_edge_contract_weights_f32: weight[i] = score[medge[i]], 1 for a singleton. */
int tgp_edge_contract_max_graph_nodes(void);
int tgp_edge_contract_edge_cache(void);
int tgp_edge_contract_hub_degree(void);
size_t tgp_edge_contract_workspace_bytes(int64_t num_nodes);
int tgp_edge_contract_project_f32(const float* x, int64_t N, int64_t F, int64_t ldx, const float* w, float* p,
                                  void* stream);
int tgp_edge_contract_raw_f32(const int64_t* row, const int64_t* col, int64_t num_edges, int64_t num_nodes, const float* p,
                              const float* bias, float* raw, void* stream);
int tgp_edge_contract_normalize_f32(const float* raw, const int64_t* col, int64_t num_edges, int64_t num_nodes, int method,
                                    float add, const int32_t* grp_ptr, const int32_t* grp_perm, float* seg, int32_t* hubs,
                                    int64_t hub_cap, float* out, void* stream);
int tgp_edge_contract_graphs(const int64_t* row, const int64_t* col, int64_t num_edges, int64_t num_nodes,
                             const int64_t* graph_ptr, int64_t num_graphs, int max_graph_nodes, const float* score,
                             const int32_t* rank, uint8_t* match, int64_t* label, int64_t* medge, int32_t* words,
                             void* stream);
int tgp_edge_contract_rounds_start(int64_t num_nodes, int64_t num_edges, void* ws, size_t ws_bytes, uint8_t* match,
                                   int64_t* label, int64_t* medge, void* stream);
int tgp_edge_contract_rounds(const int64_t* row, const int64_t* col, int64_t num_edges, int64_t num_nodes,
                             const float* score, const int32_t* rank, void* ws, int64_t round_base, int rounds,
                             int32_t* open_flags, uint8_t* match, int64_t* label, int64_t* medge, void* stream);
int tgp_edge_contract_weights_f32(const int64_t* medge, const float* score, int64_t num_nodes, int64_t num_edges,
                                  float* weight, void* stream);

/* TopkSelect scoring (select/topk_select.py:176, score = (x * w).sum(-1)): out[i] = <x[i,:], w>, one pass over
 * x [N,F] (row stride ldx); and the matching weight gradient out[f] = sum_i g[i] x[i,f] (fixed-order two-level
 * sum, deterministic). */
int tgp_row_dot_f32(const float* x, int64_t N, int64_t F, int64_t ldx, const float* w, float* out, void* stream);
/* The whole ratio-mode score of select/topk_select.py:176-184 in that one pass, for callers that need no gradient:
 * out[i] = act(<x[i,:], w> / ||w||_2), act 0 = identity ("linear"), 1 = tanh. */
int tgp_topk_score_f32(const float* x, int64_t N, int64_t F, int64_t ldx, const float* w, int act, float* out,
                       void* stream);
size_t tgp_weighted_colsum_workspace_bytes(int64_t F);
int tgp_weighted_colsum_f32(const float* x, int64_t N, int64_t F, int64_t ldx, const float* g, float* out, void* ws,
                            size_t ws_bytes, void* stream);
/* Backward of TopK pooling's trained path in one pass over the KEPT rows (r5; the reference gets it from ATen autograd
 * through poolers/topk.py:150-190 = select/topk_select.py:176-184 (t = x w / ||w||, s = act(t)), the kept scores as
 * the values of S (select/base_select.py:19-71) and reduce/base_reduce.py:141-155 (x'[c_a] = s_a x[i_a])).
 * Inputs: x [N,F] (row stride ldx, 16-byte aligned rows), node / cluster / values [K] = the assignments of the
 * one-to-one S (cluster NULL: 0..K-1), g_xpool = dL/dx' [K,F] contiguous or NULL, g_values = dL/d(values of S) [K] or
 * NULL, w [F], act 0 = identity, 1 = tanh.  Outputs: gx [N,F] contiguous, written entirely (rows of nodes that were
 * not kept are zero; NULL: not wanted), gw [F] (NULL: not wanted; fixed-order sums, run-to-run identical).
 * F % 4 == 0, F <= 256 (tgp_topk_pool_bwd_fits); other widths keep the operator-by-operator backward. */
int tgp_topk_pool_bwd_fits(int64_t F);
size_t tgp_topk_pool_bwd_workspace_bytes(int64_t F);
int tgp_topk_pool_bwd_f32(const float* x, int64_t N, int64_t F, int64_t ldx, const int64_t* node,
                          const int64_t* cluster, const float* values, int64_t K, const float* g_xpool,
                          const float* g_values, const float* w, int act, float* gx, float* gw, void* ws,
                          size_t ws_bytes, void* stream);

/* ss[e] = <S[row_e,:], S[col_e,:]> for every edge: the entries of S S^T that the sparse (unbatched) losses
 * read (utils/losses.py:73-127 sparse_mincut_loss, :661-708 sparse_link_pred_loss: (S[src] * S[dst]).sum(-1)),
 * without the two [E,K] gathers.  Any edge order; S [N,K] row-major. */
int tgp_edge_dot_f32(const int64_t* row, const int64_t* col, int64_t E, const float* S, int64_t N, int64_t K,
                     float* out, void* stream);
/* Two-matrix form, out[e] = <A[ia_e,:], Bm[ib_e,:]> (both [*,K] row-major): the assignment-weight gradient of the
 * sparse Reduce, dw_i = <x[node_i], dX'[cluster_i]> (autograd of reduce/base_reduce.py:146-153). */
int tgp_pair_dot_f32(const int64_t* ia, const int64_t* ib, int64_t E, const float* A, const float* Bm, int64_t K,
                     float* out, void* stream);

/* ----------------------------------------------------------------------------------
 * N3  auxiliary losses of the dense poolers, fused.
 *
 * tgp_link_loss_f32: sq[b] = || A[b] - S[b] S[b]^T ||_F^2 (utils/losses.py:644-708 link_pred_loss
 *   materialises S S^T [B,N,N]; here its tiles exist only in the MFMA accumulators and the GEMM
 *   epilogue reduces the squared residual).  S [B,N,K], A [B,N,N], sq [B].  The caller takes
 *   sqrt(sum_b sq[b]) (and / numel when normalize_loss).
 * tgp_entropy_sum_f32: out[0] = sum over all n elements of -S log(S + 1e-8)
 *   (utils/losses.py:476-483 entropy_loss before the / num_nodes).
 * tgp_cut_terms_f32: deg[b,i] = sum_j A[b,i,j]; q[b,i] = sum_k S[b,i,k]^2; den[b] = sum_i deg q
 *   = trace(S^T D S) of utils/losses.py:39-81 mincut_loss without forming D.  deg, q [B,N] are
 *   returned because the backward pass needs them.
 * ---------------------------------------------------------------------------------- */
size_t tgp_link_loss_workspace_bytes(int64_t B, int64_t N, int64_t K);
int tgp_link_loss_f32(const float* S, const float* A, int64_t B, int64_t N, int64_t K,
                      const int64_t* graph_sizes /* [B] or NULL, as in tgp_dense_pool_f32 */, float* sq, void* ws,
                      size_t ws_bytes, void* stream);
size_t tgp_entropy_sum_workspace_bytes(int64_t n);
int tgp_entropy_sum_f32(const float* S, int64_t n, float eps, float* out, void* ws, size_t ws_bytes, void* stream);
/* Backward of that sum (utils/losses.py:476-483 under autograd): out[i] = -(log(S[i] + eps) + S[i] / (S[i] + eps)) *
 * g[0] * scale, g a device scalar (the upstream gradient), one elementwise pass. */
int tgp_entropy_bwd_f32(const float* S, int64_t n, float eps, const float* g, float scale, float* out, void* stream);
/* DiffPool's losses (poolers/diffpool.py:262-284) from the native partial results in one launch:
 * out2[0] = sqrt(sum_b sq[b]) * link_scale (sq from tgp_link_loss_f32), out2[1] = (sum of ent_partial) * ent_scale
 * (ent_partial from tgp_entropy_partials_f32: *n_partial_out block sums of -S log(S + eps) in `ws`). */
int tgp_entropy_partials_f32(const float* S, int64_t n, float eps, void* ws, size_t ws_bytes, int* n_partial_out,
                             void* stream);
int tgp_diffpool_loss_tail_f32(const float* sq, int64_t B, const float* ent_partial, int n_partial, float link_scale,
                               float ent_scale, float* out2, void* stream);
int tgp_cut_terms_f32(const float* A, const float* S, int64_t B, int64_t N, int64_t K,
                      const int64_t* graph_sizes /* [B] or NULL */, float* deg, float* q, float* den, void* stream);
/* Per-graph tails of MinCut's losses in one launch: out[0,b] = -trace(raw[b]) / (den[b] + eps) (utils/losses.py:39-56),
 * out[1,b] = || G_b / ||G_b||_F - I / sqrt(K) ||_F (utils/losses.py:59-70); raw, gram [B,K,K], den [B], out [2,B]. */
int tgp_mincut_loss_terms_f32(const float* raw, const float* den, const float* gram, int64_t B, int64_t K, float eps,
                              float* out, void* stream);
/* Backward of those two tails in one launch: from the upstream gradients g_terms [2,B] it writes g_raw [B,K,K] (the
 * gradient with respect to raw: -(g_cut / (den + eps)) on the diagonal), c1 [B] (the gradient with respect to den:
 * g_cut trace(raw) / (den + eps)^2; d den / dS = 2 D S) and W [B,K,K] (the gradient with respect to gram = S^T S;
 * dS = S (W + W^T)). */
int tgp_mincut_loss_terms_bwd_f32(const float* raw, const float* den, const float* gram, const float* g_terms, int64_t B,
                                  int64_t K, float eps, float* g_raw, float* c1, float* W, void* stream);

/* ------------------------------------------------------------------------------------
 * DMoN's auxiliary losses (poolers/dmon.py, utils/losses.py:435-473, 1083-1265):
 *   spectral[b] = -(trace(S^T A S) - ||ca_b||^2 / 2m_b) / 2m_b,  ca_b = S_b^T d_b,  2m_b = sum_i d_{b,i}
 *   cluster[b]  = ||cs_b|| sqrt(K) / n_b - 1,                      cs_b = S_b^T 1
 *   ortho[b]    = || G_b / ||G_b||_F - I / sqrt(K) ||_F,           G = S^T S
 * The K-vectors are reduced in two stages: ``part`` [B][nsplit][2K+2] holds, per block of 64 rows of a graph,
 * (ca | cs | sum of d | node count); the loss tail adds the blocks of a graph in a fixed order.
 *
 * tgp_dmon_dense_terms_f32: padded batch, S [B,N,K], nsplit = ceil(N / 64).  With A [B,N,N]: deg[b,i] = sum_j A[b,i,j]
 *   on real rows (graph_sizes [B] and mask [B,N] (bytes) both optional), else 0, written to deg; one pass over A.  A NULL:
 *   deg [B,N] is read as the degrees (e.g. from tgp_dmon_edge_degrees_f32), NULL = none (cluster loss only).  The node
 *   count n_b is the mask's true entries (N without a mask).  One pass over S.
 * tgp_dmon_edge_degrees_f32: deg [B,N] (padded) of a row-sorted edge list with node offsets node_ptr [B+1] and edge
 *   offsets edge_ptr [B+1]: deg[b,j] = sum of w (NULL: 1) over the graph's edges whose key is node node_ptr[b] + j; key =
 *   the rows (out-degrees) or the columns (in-degrees: the row sums of the densified A^T).  N <= 1024.
 * tgp_dmon_node_terms_f32: un-padded batch, S [Ntot,K], deg [Ntot] (NULL: cluster loss only), ptr [B+1] node offsets,
 *   nsplit = ceil(largest graph / 64).  n_b = ptr[b+1] - ptr[b].
 * tgp_dmon_loss_terms_f32: out [3,B] = (c_spec spectral, c_clu cluster, c_ort ortho) per graph (the pooler's loss
 *   coefficients; 1 for the bare losses); trace(S^T A S) from the diagonal of raw
 *   [B,K,K], else from tr [B], else 0; gram [B,K,K] NULL: ortho = 0.  sqrt_k multiplies the cluster term.  clamp_m = 0:
 *   a graph with m = 0 has spectral 0 (batched form); 1: m is clamped to eps (unbatched form).  Writes ca, cs [B,K] and
 *   stats [B,4] = (2m as used or 0 | n_b | ||cs_b|| | trace) for the backward.
 * tgp_dmon_loss_terms_bwd_f32: from the upstream gradients g_terms [3,B] (times the same coefficients): g_raw [B,K,K] = -(g_spec / 2m) I (NULL: not
 *   written), g_tr [B] = -g_spec / 2m (NULL: not written), coef [B,2] = (2 g_spec / (2m)^2, g_clu sqrt(K) / (n_b ||cs||)),
 *   and with gram W [B,K,K] = d ortho / d G (dS = S (W + W^T)).
 * tgp_dmon_ds_f32: ds[r,k] (+)= coef[b,0] deg[r] ca[b,k] + coef[b,1] cs[b,k] over rows r of S; b = batch[r] when batch
 *   is given (un-padded), else r / N (padded).  deg NULL: only the cluster part.  accumulate != 0: adds into ds.
 * ---------------------------------------------------------------------------------- */
int tgp_dmon_dense_terms_f32(const float* A, const float* S, int64_t B, int64_t N, int64_t K, const int64_t* graph_sizes,
                             const uint8_t* mask, int64_t nsplit, float* deg, float* part, void* stream);
int tgp_dmon_edge_degrees_f32(const int64_t* key, const float* w, int64_t E, const int64_t* node_ptr,
                              const int64_t* edge_ptr, int64_t B, int64_t N, float* deg, void* stream);
int tgp_dmon_node_terms_f32(const float* S, const float* deg, const int64_t* ptr, int64_t B, int64_t K, int64_t nsplit,
                            float* part, void* stream);
int tgp_dmon_loss_terms_f32(const float* part, int64_t nsplit, const float* raw, const float* tr, const float* gram,
                            int64_t B, int64_t K, float sqrt_k, int clamp_m, float eps, float c_spec, float c_clu,
                            float c_ort, float* out, float* ca, float* cs, float* stats, void* stream);
int tgp_dmon_loss_terms_bwd_f32(const float* g_terms, const float* stats, const float* gram, int64_t B, int64_t K,
                                float sqrt_k, float c_spec, float c_clu, float c_ort, float* g_raw, float* g_tr,
                                float* coef, float* W, void* stream);
int tgp_dmon_ds_f32(const float* deg, const float* ca, const float* cs, const float* coef, int64_t rows, int64_t N,
                    const int64_t* batch, int64_t B, int64_t K, int accumulate, float* ds, void* stream);

/* ------------------------------------------------------------------------------------
 * Just Balance pooling's auxiliary loss (poolers/just_balance.py, utils/losses.py:553-594, 1013-1080;
 * csrc/just_balance.hip).  Per graph b, with c_k = sum_i S_ik^2 over the graph's rows:
 *   out[b] = -sum_k sqrt(c_k + eps) / denom_b * scale,  denom_b = sqrt(n_b * num_supernodes) when normalize, else 1
 * (the diagonal of sqrt(S^T S + eps); S^T S is never formed).  No float atomics: every sum has a fixed order.
 * tgp_jb_terms_f32: S [rows,K] fp32.  Padded (ptr NULL, max_rows = N): graph b owns rows b N .. b N + graph_sizes[b]
 *   (NULL: all N); n_b = the true entries of mask[b] (bytes, [B,N]) when mask is given, else graph_sizes[b], else
 *   num_nodes.  Un-padded: rows ptr[b] .. ptr[b+1] (ptr [B+1], sorted batch; neither graph_sizes nor mask), n_b = the
 *   graph's rows, max_rows = the largest graph.  max_rows <= 64: ONE launch, part is not touched (NULL ok); beyond, a
 *   partial pass into part [B, ceil(max_rows / 64), K] and a one-workgroup-per-graph tail.  Writes out [B] and
 *   coef [B,K] = -scale / (sqrt(c_k + eps) denom_b) for the backward (NULL: not written).  mean (NULL ok): one more
 *   launch leaves the batch mean of out there, summed in a fixed order.  16-byte loads when K % 4 == 0 and S, part,
 *   coef are 16-byte aligned, element loads otherwise.
 * tgp_jb_ds_f32: ds[r,k] = g_b coef[b,k] S[r,k] over rows r of S (a fresh ds, nothing is accumulated); b = batch[r]
 *   when batch is given (un-padded), else r / N; g [B], or one value for every graph when g_bcast != 0.
 * TGP_ERR_INVALID: a NULL input or output, K < 1, sizes below zero, a layout that contradicts itself, a misaligned
 * pointer (int64 tables 8 bytes, floats 4); TGP_ERR_RANGE: B, N, K, max_rows or B x splits beyond the int32 internals,
 * a mask over N >= 2^24.  Both are found before any HIP call.
 * ---------------------------------------------------------------------------------- */
int tgp_jb_terms_f32(const float* S, int64_t B, int64_t N, int64_t K, const int64_t* graph_sizes, const uint8_t* mask,
                     const int64_t* ptr, int64_t max_rows, int normalize, float num_nodes, float num_supernodes,
                     float eps, float scale, float* part, float* out, float* coef, float* mean, void* stream);
int tgp_jb_ds_f32(const float* S, const float* coef, const float* g, int g_bcast, int64_t rows, int64_t N,
                  const int64_t* batch, int64_t B, int64_t K, float* ds, void* stream);

/* ------------------------------------------------------------------------------------
 * HOSC pooling's auxiliary losses (poolers/hosc.py, utils/losses.py:218-316, 392-432, 597-641), motif adjacency
 * M = A A A never formed:
 *   cut[b]    = -trace(S^T A S) / (den1 + eps),   den1 = sum_i d1_i |S_i|^2,  d1 = A 1
 *   ho_cut[b] = -num / (den3 + eps),  num = sum S (.) Z,  Z = A (A (A S)),  den3 = sum_i d3_i |S_i|^2,  d3 = A (A (A 1))
 *   out[0,b]  = (1 - alpha) cut inv_k + alpha ho_cut inv_k          (a part whose weight is 0 is not evaluated)
 *   out[1,b]  = mu || G / ||G||_F - I / sqrt(K) ||_F  (gram given)  or, hosc_ortho,
 *               mu (sqrt(K) - sum_j ||S_*j|| / sqrt(n_b)) / (sqrt(K) - 1), 0 when K <= 1;  0 when mu = 0
 * ``part`` [B][nsplit][tgp_hosc_record_floats(K)] holds, per block of 64 rows of a graph, the K column square sums, per
 * block of 64 columns (num | den3 | num1 = sum S (.) (A S) | den1), and the node count; the tail adds the blocks of a graph
 * in a fixed order.
 *
 * tgp_hosc_matvec_f32: y[b,i] = sum_j A[b,i,j] v[b,j] (v NULL: ones) on the rows below graph_sizes[b] (NULL: all), 0 on
 *   the others; A [B,N,N], v and y [B,N]; one streaming pass over A.  The columns are not cut.
 * tgp_hosc_node_terms_f32: S [rows,K]; Z, Z1 with row stride ldz, d3, d1 with element stride ldd (each NULL: its sums are
 *   0).  Padded (ptr NULL): graph b owns rows b N .. b N + graph_sizes[b] (NULL: N), nsplit = ceil(N / 64), n_b = the
 *   mask's (bytes, [B,N]) true entries (NULL: N).  Un-padded: rows ptr[b] .. ptr[b+1], nsplit = ceil(largest graph / 64),
 *   n_b = the graph's rows.
 * tgp_hosc_small_f32: padded batch with N, K <= tgp_hosc_small_graph_nodes() (64): d1, d3 [B,N], Z [B,N,K] and part
 *   (nsplit = 1) in ONE launch, one workgroup per graph with A[b] and two [N,K] buffers in LDS.
 * tgp_hosc_loss_terms_f32: out [2,B]; trace(S^T A S) from the diagonal of raw [B,K,K], else from the num1 partials.
 *   Writes cn [B,K] = ||S_*k|| and stats [B,6] = (num | den3 + eps | n_b | trace | den1 + eps | sum_k cn_k).
 * tgp_hosc_loss_terms_bwd_f32: from the upstream gradients g_terms [2,B]: coef [B,5] = (c_num = -g0 alpha inv_k / D3,
 *   c_den = g0 alpha inv_k num / D3^2, c_ortho = -g1 mu / (sqrt(n_b) (sqrt(K) - 1)) (hosc_ortho, else 0),
 *   c_den1 = g0 (1 - alpha) inv_k trace / D1^2, c_num1 = -g0 (1 - alpha) inv_k / D1), g_raw [B,K,K] = c_num1 I (NULL: not
 *   written) and, with gram, W [B,K,K] = d out[1] / d G (dS = S (W + W^T)).
 * tgp_hosc_ds_f32: ds[r,k] (+)= c_num (Z + Zt) + 2 c_den d3_r S + c_ortho S / cn[b,k] + 2 c_den1 d1_r S
 *   + c_num1 (Z1 + Z1t); Zt = A^T (A^T (A^T S)), Z1t = A^T S with row stride ldzt, NULL: A = A^T, the forward's product
 *   counts twice.  b = batch[r] when given (un-padded), else r / N.  A column of norm 0 gets no c_ortho term.
 * ---------------------------------------------------------------------------------- */
int tgp_hosc_small_graph_nodes(void);
int64_t tgp_hosc_record_floats(int64_t K);
int tgp_hosc_matvec_f32(const float* A, const float* v, int64_t B, int64_t N, const int64_t* graph_sizes, float* y,
                        void* stream);
int tgp_hosc_node_terms_f32(const float* S, const float* Z, const float* Z1, int64_t ldz, const float* d3,
                            const float* d1, int64_t ldd, int64_t B, int64_t N, int64_t K, const int64_t* graph_sizes,
                            const uint8_t* mask, const int64_t* ptr, int64_t nsplit, float* part, void* stream);
int tgp_hosc_small_f32(const float* A, const float* S, int64_t B, int64_t N, int64_t K, const int64_t* graph_sizes,
                       const uint8_t* mask, float* Z, float* d1, float* d3, float* part, void* stream);
int tgp_hosc_loss_terms_f32(const float* part, int64_t nsplit, const float* raw, const float* gram, int64_t B, int64_t K,
                            float alpha, float mu, float inv_k, int hosc_ortho, float eps, float* out, float* cn,
                            float* stats, void* stream);
int tgp_hosc_loss_terms_bwd_f32(const float* g_terms, const float* stats, const float* gram, int64_t B, int64_t K,
                                float alpha, float mu, float inv_k, int hosc_ortho, float* g_raw, float* coef, float* W,
                                void* stream);
int tgp_hosc_ds_f32(const float* S, const float* Z, const float* Zt, const float* Z1, const float* Z1t, int64_t ldz,
                    int64_t ldzt, const float* d3, const float* d1, int64_t ldd, const float* cn, const float* coef,
                    int64_t rows, int64_t N, const int64_t* batch, int64_t B, int64_t K, int accumulate, float* ds,
                    void* stream);

/* ------------------------------------------------------------------------------------
 * BN-Pool's reconstruction loss (poolers/bnpool.py:359-447, utils/losses.py:1268-1356), logits L = T S^T, T = S K,
 * never written to memory.  Per graph b, m the node mask (bytes [B,N], NULL: all ones), n = sum m,
 * e = #{(i,j): a_ij != 0, m_i m_j}, c = max(n^2 - e, 1) / max(e, 1), bce(l, a) = max(l, 0) - l a + log1p(exp(-|l|)):
 *   rec[b] = (c sum_{a != 0} bce + sum_{a == 0} bce) / n^2,   both sums over m_i m_j = 1
 * T, S [B,N,K] and A [B,N,N] contiguous float32; 1 <= K <= tgp_bnpool_max_clusters() (256), N >= 1.
 *
 * tgp_bnpool_rec_fwd_f32: one launch over the 32x32 tiles of L (exact-fp32 MFMA, T's rows and S's fragment on chip) that
 *   reads each tile of A once and writes one record (sum a != 0 | sum a == 0 | count, int bits | 0) per (graph, block
 *   of 32 columns) into ``part`` (``part_floats`` >= tgp_bnpool_part_floats(B, N) floats), then one tail launch that
 *   adds a graph's records in a fixed order: rec [B], stats [B,2] = (c | n^2).  Bit-reproducible.
 * tgp_bnpool_rec_bwd_f32: with G_ij = g[b] w_ij (sigmoid(l_ij) - a_ij) m_i m_j / n^2, w = c where a != 0, else 1
 *   (stats from the forward), P = G S and Q = G^T T, both [B,N,K], from two launches that recompute the logit tiles
 *   and keep G on chip (the second reads A's tiles transposed through LDS); no float atomics.  The caller forms
 *   dS = P K^T + Q and dK = sum_b S^T P.  A gets no gradient.
 * ---------------------------------------------------------------------------------- */
int tgp_bnpool_max_clusters(void);
int64_t tgp_bnpool_part_floats(int64_t B, int64_t N);
int tgp_bnpool_rec_fwd_f32(const float* T, const float* S, const float* A, const uint8_t* mask, int64_t B, int64_t N,
                           int64_t K, float* part, int64_t part_floats, float* rec, float* stats, void* stream);
int tgp_bnpool_rec_bwd_f32(const float* T, const float* S, const float* A, const uint8_t* mask, const float* g,
                           const float* stats, int64_t B, int64_t N, int64_t K, float* P, float* Q, void* stream);

/* ------------------------------------------------------------------------------------
 * AsymCheegerCut's auxiliary losses (poolers/asym_cheeger_cut.py, utils/losses.py:503-550, 780-1010):
 *   totvar[b]  = sum_ij a_ij ||s_i - s_j||_1 / (2 E_b),  E_b clamped to >= 1
 *   balance[b] = (n (k-1) - sum_ik rho(s_ik - q_k)) / (n (k-1)),  q_k the idx-th largest entry of column k among the n
 *                real nodes, idx = min(floor(n / k), n - 1), rho(d) = (k-1) d for d >= 0 and -d for d < 0
 * No float atomics: every sum has a fixed order.  Graph b owns rows b N .. of S in the padded layout (ptr NULL; its real
 * rows: the first graph_sizes[b] (NULL: N) of them whose mask byte (NULL: all) is set) or rows ptr[b] .. ptr[b+1] in the
 * un-padded one.
 *
 * tgp_acc_small_graph_nodes: the largest graph the counting select takes (128).
 * tgp_acc_tv_dense_f32: A [B,N,N], S [B,N,K], nrb = ceil(N / 16): part [B,nrb] = per block of 16 rows the sum of
 *   a_ij ||s_i - s_j||_1 over its nonzero a_ij, cnt [B,nrb] (int32) = its nonzeros.  A wave skips 64-column chunks of A
 *   that hold no nonzero.  Rows and columns beyond graph_sizes[b] are not read.
 * tgp_acc_tv_dense_bwd_f32: dS [B,N,K] = g_terms[b] c_tv / (2 ecnt[b]) sum_j (a_ij + a_ji) sign(s_i - s_j), sign(0) = 0;
 *   every row is written.  g_terms [B], ecnt [B] (int32, >= 1) from tgp_acc_loss_terms_f32.
 * tgp_acc_tv_edge_f32: S [nodes,K], col [E] destinations, w [E] (NULL: ones), (src_ptr [nodes+1], src_perm [E]) (int32)
 *   the edges grouped by source in edge-list order (tgp_assign_index_build over the sources): node_tv[i] = sum over the
 *   out-edges of i of w_e ||s_i - s_dst||_1.
 * tgp_acc_tv_edge_bwd_f32: dS [nodes,K] from the out-edges and the in-edges (dst_ptr, dst_perm: grouped by destination)
 *   of every node; an edge belongs to the graph batch[source] (batch NULL: graph 0).
 * tgp_acc_quantile_f32: per (graph, column) q [B,K] = the quantile, qnode [B,K] (int32) = the LOWEST row, relative to the
 *   graph's first, that holds it (-1: none), colsum [B,K] = sum_i rho(s_ik - q_k), cge [B,K] (int32) = rows with
 *   s_ik >= q_k; nreal [B] (int32) = real rows.  kq = the k of the loss.  max_nodes = the largest graph (N when padded).
 *   route 0: the counting select when max_nodes <= tgp_acc_small_graph_nodes(), else the radix select; 1 / 2 force one.
 *   Exact: the bits of the entry a descending sort has at position idx (-0 and +0 are one value, NaN the largest).
 * tgp_acc_loss_terms_f32: out [2,B] = (c_tv totvar, c_bal balance), ecnt [B] (int32) = E_b clamped.  tv NULL: row 0 is 0;
 *   dense form: tv = part, cnt, nrb; edge form: tv = node_tv, src_ptr, ptr (E_b = the edges whose source lies in graph
 *   b).  colsum NULL: row 1 is 0.
 * tgp_acc_asym_bwd_f32: dS[r,k] (+)= -g_bal[b] c_bal rho'(s - q_k) / (n (k-1)) on real rows, plus
 *   g_bal[b] c_bal sum_i rho'(d_ik) / (n (k-1)) on the quantile node; rho'(d) = k-1 for d >= 0, -1 otherwise.  Graph of a
 *   row: r / N (padded), batch[r] (un-padded; batch NULL: 0).
 * ---------------------------------------------------------------------------------- */
int tgp_acc_small_graph_nodes(void);
int tgp_acc_tv_dense_f32(const float* A, const float* S, int64_t B, int64_t N, int64_t K, const int64_t* graph_sizes,
                         int64_t nrb, float* part, int* cnt, void* stream);
int tgp_acc_tv_dense_bwd_f32(const float* A, const float* S, int64_t B, int64_t N, int64_t K, const int64_t* graph_sizes,
                             const float* g_terms, const int* ecnt, float c_tv, float* dS, void* stream);
int tgp_acc_tv_edge_f32(const float* S, int64_t nodes, int64_t K, const int64_t* col, const float* w, int64_t E,
                        const int* src_ptr, const int* src_perm, float* node_tv, void* stream);
int tgp_acc_tv_edge_bwd_f32(const float* S, int64_t nodes, int64_t K, const int64_t* row, const int64_t* col,
                            const float* w, int64_t E, const int* src_ptr, const int* src_perm, const int* dst_ptr,
                            const int* dst_perm, const int64_t* batch, const float* g_terms, const int* ecnt, float c_tv,
                            int64_t B, float* dS, void* stream);
int tgp_acc_quantile_f32(const float* S, int64_t B, int64_t N, int64_t K, const int64_t* graph_sizes, const uint8_t* mask,
                         const int64_t* ptr, int64_t max_nodes, int64_t kq, int route, float* q, int* qnode, float* colsum,
                         int* cge, int* nreal, void* stream);
int tgp_acc_loss_terms_f32(const float* tv, const int* cnt, const int* src_ptr, const int64_t* ptr, int64_t nrb,
                           const float* colsum, const int* nreal, int64_t B, int64_t K, int64_t kq, float c_tv, float c_bal,
                           float* out, int* ecnt, void* stream);
int tgp_acc_asym_bwd_f32(const float* S, int64_t rows, int64_t N, int64_t K, const int64_t* batch, const int64_t* ptr,
                         const int64_t* graph_sizes, const uint8_t* mask, const float* q, const int* qnode, const int* cge,
                         const int* nreal, const float* g_bal, float c_bal, int64_t kq, int64_t B, int accumulate, float* dS,
                         void* stream);

/* ------------------------------------------------------------------------------------
 * N1 (r6)  The dense poolers' TRAINING step for graphs beyond the one-wave / one-workgroup kernels (C2: B = 32,
 * N = 1024, K = 128, F = 64), as the pieces ONE autograd node is made of (host side: functions._PoolLargeFn).  What the
 * reference gets from ATen autograd over poolers/mincut.py:220-237 / diffpool.py:208-218 (harness:
 * examples/time_and_mem_test.py:396-401).
 *
 * The operand buffer of the backward, acat [B][N][3K+F+4], has the column blocks  [U | X | 1 0 0 0 | S | V]:
 *   gS = acat [RU ; RX ; 0 ; RS ; RV]  is ONE product; for a symmetric A (V = U) its first 2K+F+4 columns / rows suffice
 *   and V is never formed; dY^T [X | 1 0 0 0] is the selector's weight AND bias gradient; dY is written over the V block,
 *   which lies behind S, so gX = [S | dY] [g_x ; W] is one product as well.
 *
 * tgp_dense_pool_train_fwd_f32: tgp_dense_pool_f32's three launches (U = A S; S^T [U | X | S] split over N; slab
 *   combine + post-processing), with U written where the caller says -- row stride ldu >= K: column block 0 of acat --
 *   and, when `gram` is not NULL, G = S^T S [B,K,K] as a third right-hand side of the second product.  adj_raw is
 *   required, adj_pool optional; flags as tgp_dense_pool_f32 (TGP_ADJ_TRANSPOSED: A is stored transposed).
 * tgp_mincut_terms_fused_f32: MinCut's per-graph loss tails out [2,B] (as tgp_mincut_loss_terms_f32) with
 *   den[b] = sum_i deg[b,i] q[b,i] formed in the same launch (deg, q [B,N] from tgp_cut_terms_f32) and kept for the
 *   backward together with stats [B,4] = (trace(raw), |G|_F^2, trace(G), |G / |G| - I / sqrt(K)|_F) per graph (optional).
 *   ptr (optional, [B+1]): deg / q are those of an UN-padded batch, graph b owns entries ptr[b] .. ptr[b+1] (N unused).
 *   q may be NULL: den[b] = sum_i deg[b,i] (the caller's deg already carries the factor, e.g. (A q)_i).
 *   means (optional, [2]): the batch means of the two terms, formed by the workgroup that arrives last (terms added in
 *   graph order: independent of the arrival order); needs `ticket`, one zeroed uint32 word per (device, stream) that the
 *   call leaves zero.
 * tgp_dense_pool_train_rhs_f32: the right-hand sides into rcat [B][3K+F+4][K], rows [RU ; RX ; four zero rows ; RS ; RV]:
 *   with gR = g_raw_a + g_raw_b (either may be NULL) + the loss' diagonal term, RV = gR, RU = gR^T (`symmetric` bit 0:
 *   RU = gR + gR^T, RV not written; bit 1: RU = gR, RV = gR^T -- the buffer's first block holds A S while raw = S^T A^T S), RX = g_x^T (g_x [B,K,F], or one value when gx_bcast), RS by mode:
 *   0: zeros;
 *   1 (MinCut): RS = W + W^T, gR -= (g_cut / (den + eps)) I, c1[b] = g_cut trace(raw) / (den + eps)^2 (the per-graph
 *      scalars from the forward's `stats`: the launch is purely elementwise, 32 x 32 tiles), with
 *      g_cut = *g_la * scale, g_ortho = *g_lb * scale (0-dim device values or NULL; scale = 1 / B for the batch means);
 *   2 (DiffPool): c = link_scale^2 *g_la / *link_loss (0 when the loss is 0), gR -= c I, RS = 2 c G.
 *   gw (optional, [B][2K][F], needs the selector weight W [K][F]): gw[b] = [g_x[b] ; W].
 * tgp_softmax_bwd_ex_f32: tgp_softmax_bwd_f32 on dS + extra + 2 c1[m / rows_per_graph] deg[m] S
 *   - *ent_g ent_scale (log(S + eps) + S / (S + eps))   (extra, c1/deg, ent_g: each optional); dy with row stride ld_dy;
 *   batch (optional, [M]): the graph of row m is batch[m] (un-padded batch) instead of m / rows_per_graph.
 * tgp_copy_cols2_f32: dst[r, col_a:col_a+wa] = a[r,:], dst[r, col_b:col_b+wb] = b[r,:] (row stride ld) in one pass;
 *   one_col >= 0: also dst[r, one_col:one_col+4] = [1 0 0 0].
 * tgp_adj_symmetry_f32: is the [B,Nmax,Nmax] adjacency the edge list (row, col) was scattered into symmetric?  One
 *   thread per entry compares adj[b,r,c] with adj[b,c,r]; the verdict arrives in pinned host words (protocol of
 *   tgp_edge_facts_sorted_i64: result word 0 = tag stored last, word 2 = 1 when some entry differs from its mirror).
 * ---------------------------------------------------------------------------------- */
size_t tgp_dense_pool_train_workspace_bytes(int64_t B, int64_t N, int64_t K, int64_t F);
int tgp_dense_pool_train_fwd_f32(const float* S, const float* A, const float* X, int64_t B, int64_t N, int64_t K,
                                 int64_t F, int flags, float eps, float* U, int64_t ldu, float* x_pool, float* adj_raw,
                                 float* adj_pool, float* gram, void* ws, size_t ws_bytes, void* stream);
/* (edge_row_ptr / edge_col / edge_w, optional, un-padded batches only: den = sum over a graph's entries of
 *  w_e q[col_e] = sum_j indeg_j q_j, the in-degree form of the batched poolers' S^T A^T S -- deg is then not read) */
int tgp_mincut_terms_fused_f32(const float* raw, const float* gram, const float* deg, const float* q, int64_t B,
                               int64_t N, int64_t K, float eps, float* den, float* out, float* stats, const int64_t* ptr,
                               uint32_t* ticket, float* means, const int32_t* edge_row_ptr, const int64_t* edge_col,
                               const float* edge_w, void* stream);
int tgp_dense_pool_train_rhs_f32(const float* g_raw_a, const float* g_raw_b, int mode, const float* stats, const float* den,
                                 const float* gram, const float* g_la, const float* g_lb, float scale,
                                 const float* link_loss, float link_scale, float eps, const float* g_x, int gx_bcast,
                                 int symmetric, const float* W, int64_t B, int64_t K, int64_t F, float* rcat, float* c1,
                                 float* gw, void* stream);
int tgp_softmax_bwd_ex_f32(const float* s, const float* ds, const float* extra, const float* c1, const float* deg,
                           int64_t rows_per_graph, const float* ent_g, float ent_scale, float ent_eps, float* dy,
                           int64_t ld_dy, int64_t M, int64_t K, const int64_t* batch, void* stream);
/* ------------------------------------------------------------------------------------
 * N3 (r6)  The UNBATCHED dense poolers' forward (mincut_u / diff_u: S [Ntot,K], sparse A) from the products their
 * Connect forms anyway -- no per-edge dot products, no index_add scatters (utils/losses.py:73-127, 204-240, 661-708;
 * connect/dense_conn.py:140-208; reduce/base_reduce.py:170-182):
 *   sum_{e in g} w_e <S_row, S_col> = trace(S_g^T (A S)_g) = trace(raw_g)       (sparse_mincut_loss' numerator)
 *   |A - S S^T|_F^2 = sum_e w_e^2 - 2 sum_g trace(raw_g) + sum_g |S_g^T S_g|_F^2  (sparse_link_pred_loss)
 * tgp_segment_gemm_tn3_f32: C_j[b] = S_b^T Y_j,b for up to three right-hand sides Y_j [Ntot,F_j] in one grid (+ one
 *   combine launch): S^T [A S | X | S] = raw pooled adjacency, pooled features, per-graph Gram matrices.  transpose0:
 *   the first output (K x K) is written transposed by the combine launch (S^T A^T S from the slabs of S^T (A S)).
 * tgp_edge_row_stats_f32: deg[i] = sum of w over CSR row i (entry count when w is NULL), q[i] = |S_i|^2.
 * tgp_diffpool_unbatched_tail_f32: out2 = (sqrt(max(sw2 - 2 sum_b trace(raw_b) + sum_b |gram_b|^2, 0)) link_scale,
 *   (sum of ent_partial) ent_scale); sw2 = sum_e w_e^2 from *sw2_dev when not NULL, else sw2_host; stats [B,2] scratch.
 * ---------------------------------------------------------------------------------- */
size_t tgp_segment_gemm_tn3_workspace_bytes(int64_t B, int64_t K, int64_t F0, int64_t F1, int64_t F2, int64_t max_nodes);
int tgp_segment_gemm_tn3_f32(const float* S, const float* Y0, int64_t F0, const float* Y1, int64_t F1, const float* Y2,
                             int64_t F2, const int64_t* ptr, float* C0, float* C1, float* C2, int64_t B, int64_t Ntot,
                             int64_t K, int64_t max_nodes, int transpose0, void* ws, size_t ws_bytes, void* stream);
/* r6: the same products (Y0 must be [Ntot,K]: the first output is raw = S^T Y0 [B,K,K]) and raw's post-processing
 * (utils/ops.py:282-335; flags = TGP_REMOVE_SELF_LOOPS | TGP_DEGREE_NORM | ..., eps its degree clamp) -> adj_pool [B,K,K]
 * in one call: for 64 < K <= 176 the post-processing launch sums the slabs of all three products itself (two launches in
 * all); otherwise the combine launch and the post-processing kernels of that size follow the product. */
size_t tgp_segment_gemm_tn3_post_workspace_bytes(int64_t B, int64_t K, int64_t F1, int64_t F2, int64_t max_nodes);
int tgp_segment_gemm_tn3_post_f32(const float* S, const float* Y0, const float* Y1, int64_t F1, const float* Y2, int64_t F2,
                                  const int64_t* ptr, float* raw, float* C1, float* C2, float* adj_pool, int64_t B,
                                  int64_t Ntot, int64_t K, int64_t max_nodes, int transpose0, int flags, float eps,
                                  void* ws, size_t ws_bytes, void* stream);
/* r6 (late): the forward of the un-padded rows route as ONE call (host time: four wrapper calls -> one).  Strings together
 * tgp_mlp_select_f32 (W != NULL: S [Ntot,K] is written; W == NULL: S is read), tgp_spmm_csr_{,stats_,entropy_}f32 (T = A S
 * [Ntot,K]; rowstat = [2,Ntot] deg | q for mode 1, [Ntot] entropy shares for mode 2), tgp_segment_gemm_tn3_post_f32 (raw,
 * x_pool [B,K,F], gram (modes 1, 2), adj_pool) and the loss tail: mode 1 tgp_mincut_terms_fused_f32 (den [B], terms [2,B],
 * stats [B,4], means [2] + ticket or NULL; transposed: the in-degree denominator from the entries), mode 2
 * tgp_diffpool_unbatched_tail_f32 (dstats [B,2], out2 [2]; sw2 as for that entry).  Same launches, same results. */
size_t tgp_pool_rows_fwd_workspace_bytes(int64_t B, int64_t K, int64_t F, int64_t max_nodes, int64_t Ntot);
int tgp_pool_rows_fwd_f32(const float* x, int64_t Ntot, int64_t F, const float* W, const float* bias, float* S,
                          const int32_t* row_ptr, const int64_t* col, const float* w, int64_t nnz, const int64_t* ptr,
                          int64_t B, int64_t K, int64_t max_nodes, int transposed, int post_flags, float eps,
                          float loss_eps, int mode, const float* sw2_dev, float sw2_host, float link_scale,
                          float ent_scale, float* T, float* raw, float* x_pool, float* gram, float* adj_pool,
                          float* rowstat, float* den, float* terms, float* stats, float* means, uint32_t* ticket,
                          float* dstats, float* out2, void* ws, size_t ws_bytes, void* stream);
/* ... and its backward for the common case -- selector folded in (W [K,F]), A = A^T (T serves as U and V) -- as ONE call:
 * tgp_postprocess_dense_bwd_f32 (g_adj, an expanded scalar when g_adj_bcast), tgp_dense_pool_train_rhs_f32,
 * tgp_copy_cols3_f32, tgp_segment_gemm_nn_ld_f32 (gS, gX), tgp_softmax_bwd_ex_f32, tgp_segment_gemm_tn_ld_f32 over
 * `slabs` row ranges slab_ptr [slabs+1] and tgp_slab_sum_split_f32.  Saved by the forward: S, T, raw, gram, stats, den, deg,
 * link_loss ([1], mode 2).  Upstream gradients (each may be NULL): g_adj, g_raw [B,K,K], g_x [B,K,F] (one value when
 * g_x_bcast), g_s [Ntot,K], g_la / g_lb (0-dim: the two losses).  Buffers: ga [B,K,K] (with g_adj), rcat [B,3K+F+4,K], c1
 * [B] (mode 1), gwcat [B,2K,F] (with gX), acat [Ntot,3K+F+4], gS [Ntot,K], part [slabs,K,F+4] (with gW / gbias).
 * Outputs: gX [Ntot,F], gW [K,F], gbias [K] (each optional). */
int tgp_pool_rows_bwd_f32(const float* S, const float* T, const float* X, const float* W, const float* raw,
                          const float* gram, const float* stats, const float* den, const float* deg,
                          const float* link_loss, const int64_t* ptr, const int64_t* batch, const int64_t* slab_ptr,
                          int64_t slabs, int64_t Ntot, int64_t B, int64_t K, int64_t F, int64_t max_nodes, int post_flags,
                          float eps, float loss_eps, int mode, int transposed, float inv_b, float link_scale,
                          float ent_scale, const float* g_adj, int g_adj_bcast, const float* g_raw, const float* g_x,
                          int g_x_bcast, const float* g_s, const float* g_la, const float* g_lb, float* ga, float* rcat,
                          float* c1, float* gwcat, float* acat, float* gS, float* gX, float* part, float* gW, float* gbias,
                          void* stream);
int tgp_edge_row_stats_f32(const int32_t* row_ptr, const float* w, const float* S, int64_t N, int64_t K, float* deg,
                           float* q, void* stream);
/* the two segment products with explicit row strides (operands that are column blocks of a wider buffer: the unbatched
 * training step): nn: C[rows of b] = A[rows of b, 0:Kd] Bm[b] (A row stride lda; Bm [B][Kd][Nc], row stride ldb, batch
 * stride sB; C row stride ldc);  tn: C[b] = A[rows of b]^T Y[rows of b] ([B][M][Nc], no node-range split). */
int tgp_segment_gemm_nn_ld_f32(const float* A, int64_t lda, const float* Bm, int64_t ldb, int64_t sB, const int64_t* ptr,
                               float* C, int64_t ldc, int64_t B, int64_t Ntot, int64_t Kd, int64_t Nc, int64_t max_nodes,
                               void* stream);
int tgp_segment_gemm_tn_ld_f32(const float* A, int64_t lda, const float* Y, int64_t ldy, const int64_t* ptr, float* C,
                               int64_t B, int64_t Ntot, int64_t M, int64_t Nc, void* stream);
/* is the COALESCED row-sorted list (row, col, w) with CSR offsets row_ptr symmetric: has every entry (r, c, w) a mirror
 * entry (c, r, w)?  Verdict as tgp_adj_symmetry_f32 (pinned result word 2 = 1: no). */
/* ... and for a dense [B,N,N] adjacency: every entry equals its mirror image?  (one pass, 32 x 32 tile pairs) */
int tgp_dense_symmetry_f32(const float* adj, int64_t B, int64_t N, uint32_t* ticket, uint64_t* result, uint64_t tag,
                           void* stream);
int tgp_edge_symmetry_f32(const int64_t* row, const int64_t* col, const float* w, int64_t E, const int32_t* row_ptr,
                          int64_t N, uint32_t* ticket, uint64_t* result, uint64_t tag, void* stream);
int tgp_diffpool_unbatched_tail_f32(const float* raw, const float* gram, int64_t B, int64_t K, const float* sw2_dev,
                                    float sw2_host, const float* ent_partial, int n_partial, float link_scale,
                                    float ent_scale, float* stats, float* out2, void* stream);

/* part [slabs][K][W] (W >= F + 1: dY^T [X | 1 0 0 0] per row slab) -> gw [K][F] (columns 0..F-1) and gb [K] (column F), the
 * slabs added in order; either output may be NULL. */
int tgp_slab_sum_split_f32(const float* part, int64_t slabs, int64_t K, int64_t F, int64_t W, float* gw, float* gb,
                           void* stream);
int tgp_adj_symmetry_f32(const int64_t* row, const int64_t* col, int64_t E, const int64_t* batch, const int64_t* ptr,
                         int64_t Nmax, const float* adj, uint32_t* ticket, uint64_t* result, uint64_t tag, void* stream);
int tgp_copy_cols2_f32(const float* a, int64_t wa, const float* b, int64_t wb, int64_t rows, float* dst, int64_t ld,
                       int64_t col_a, int64_t col_b, int64_t one_col, void* stream);
/* the same with a third source block c [rows, wc] -> dst[:, col_c : col_c + wc] */
int tgp_copy_cols3_f32(const float* a, int64_t wa, const float* b, int64_t wb, const float* c, int64_t wc, int64_t rows,
                       float* dst, int64_t ld, int64_t col_a, int64_t col_b, int64_t col_c, int64_t one_col, void* stream);

/* A7'  sparse A times dense S (connect/dense_conn.py:165,204: torch.sparse.mm), A in CSR built from a
 * row-sorted coalesced edge list: T[i,:] = sum_{e in row i} w[e] * S[col[e],:].  w may be NULL. */
int tgp_rowptr_from_sorted_i64(const int64_t* rows, int64_t n, int64_t num_rows, int32_t* row_ptr, void* stream);
/* the same for a list whose order has not been checked: *d_unsorted (zeroed by the entry) = 1 when a row id descends;
 * the offsets of such a list are meaningless but stay in [0, n] (callers go on and read the flag with their next
 * read-back instead of synchronising for the check first) */
int tgp_rowptr_from_sorted_flag_i64(const int64_t* rows, int64_t n, int64_t num_rows, int32_t* row_ptr, int* d_unsorted,
                                    void* stream);
int tgp_spmm_csr_f32(const int32_t* row_ptr, const int64_t* col, const float* w, int64_t num_rows, int64_t nnz,
                     const float* S, int64_t K, float* T, void* stream);
/* r6: the same product with MinCut's degree term riding along (utils/losses.py:73-127): deg[i] = sum of row i's weights
 * (entry count when w is NULL), q[i] = |S_i|^2 -- the outputs of tgp_edge_row_stats_f32 without its launch. */
int tgp_spmm_csr_stats_f32(const int32_t* row_ptr, const int64_t* col, const float* w, int64_t num_rows, int64_t nnz,
                           const float* S, int64_t K, float* T, float* deg, float* q, void* stream);
/* r6: ... and with DiffPool's entropy loss riding along (utils/losses.py:476-483): partial[0 .. *n_partial) = per-workgroup
 * shares of sum(-S log(S + eps)) over S [num_rows,K] (partial: >= num_rows floats; the sum of the shares is what
 * tgp_diffpool_unbatched_tail_f32 takes as its entropy partials).  *n_partial = -1: the shape does not take the row
 * kernel -- T is computed, the shares are not. */
int tgp_spmm_csr_entropy_f32(const int32_t* row_ptr, const int64_t* col, const float* w, int64_t num_rows, int64_t nnz,
                             const float* S, int64_t K, float* T, float eps, float* partial, int* n_partial, void* stream);

/* A8 alone: post-process a [B,K,K] pooled adjacency (src may equal dst).                */
size_t tgp_postprocess_dense_workspace_bytes(int64_t B, int64_t K);
int tgp_postprocess_dense_f32(const float* src, float* dst, int64_t B, int64_t K, int flags, float eps, void* ws,
                              size_t ws_bytes, void* stream);
/* Its backward (what autograd derives from utils/ops.py:282-335): g_raw [B,K,K] from the raw S^T A S and the upstream
 * gradient of the post-processed tensor; one launch, K <= 4096, TGP_EDGE_WEIGHT_NORM refused (not differentiated here).
 * flags bit 16 (r6): g_post is ONE value that stands for every element (the gradient of a plain sum: an expanded scalar). */
int tgp_postprocess_dense_bwd_f32(const float* raw, const float* g_post, int64_t B, int64_t K, int flags, float eps,
                                  float* g_raw, void* stream);

/* A11  DenseSRCPooling.preprocessing (src.py:374-452 -> PyG to_dense_adj / to_dense_batch): the step
 * right before the timed path.  batch must be sorted; ptr[B+1] = exclusive prefix of the graph sizes.
 * adj [B,Nmax,Nmax] / out [B,Nmax,F] / mask [B,Nmax] are zero-filled inside.  transposed != 0 writes
 * A^T (what src.py:442-443 produces as a view).  Duplicated edges are summed (float atomics).  adj_is_zeroed != 0: the
 * caller has zero-filled adj already (tgp_to_dense_batch_sorted_f32 can do it in its own launch). */
int tgp_to_dense_adj_f32(const int64_t* row, const int64_t* col, const float* edge_weight /* NULL = ones */,
                         int64_t num_edges, const int64_t* batch, const int64_t* ptr, int64_t B, int64_t Nmax,
                         int transposed, int adj_is_zeroed, float* adj, void* stream);
/* the same for multi-channel edge attributes [E, C] (PyG to_dense_adj with a 2-D edge_attr): adj [B,Nmax,Nmax,C],
 * zero-filled inside, duplicates summed per channel (r5) */
int tgp_to_dense_adj_channels_f32(const int64_t* row, const int64_t* col, const float* edge_attr /* [E, C] */,
                                  int64_t num_edges, int64_t num_channels, const int64_t* batch, const int64_t* ptr,
                                  int64_t B, int64_t Nmax, int transposed, float* adj, void* stream);
/* inverse gather of tgp_to_dense_adj_f32 (its backward w.r.t. the edge weights, which the reference gets from ATen
 * autograd over PyG's scatter, src.py:434): grad_weight[e] = grad_adj[slot of e], 0 for dropped entries */
int tgp_from_dense_adj_f32(const float* grad_adj, const int64_t* row, const int64_t* col, int64_t num_edges,
                           const int64_t* batch, const int64_t* ptr, int64_t B, int64_t Nmax, int transposed,
                           float* grad_weight, void* stream);
/* inverse gather of tgp_to_dense_batch_f32 (its backward): x[i,:] = dense[batch[i], i - ptr[batch[i]], :] */
int tgp_from_dense_batch_f32(const float* dense, int64_t N, int64_t F, const int64_t* batch, const int64_t* ptr,
                             int64_t B, int64_t Nmax, float* x, void* stream);
/* Facts about a batch vector for ONE host read (what PyG's to_dense_batch / the reference's src.py:434-450 obtain with
 * batch.max().item() and a bincount): sizes [N + 1] int64 = node count per graph id (the caller keeps sizes[:B]),
 * facts int64[5] = {B - 1, bit 0: not sorted | bit 1: an id outside [0, N] (sizes are then meaningless), nodes of the
 * longest graph, number of non-empty graphs, sum over graphs of TopkSelect's k_g for topk_ratio (tgp_topk_plan's
 * arithmetic; 0 when topk_ratio <= 0)}. */
int tgp_batch_facts_i64(const int64_t* batch, int64_t N, int64_t* sizes, int64_t* facts, double topk_ratio, void* stream);
/* r5: the same facts for a SORTED vector in ONE launch, no memset, no copy back: ptr [N + 2] (CSR offsets: graph g owns
 * nodes ptr[g] .. ptr[g + 1]), sizes [N + 1], and for topk_ratio > 0 TopkSelect's plan k [N + 1] / koff [N + 2] (NULL:
 * not wanted).  `ticket`: two uint32 words owned by the caller per (device, stream), zero at entry, left zero.  `result`:
 * six words of pinned host memory -- {tag, B - 1, flags, longest graph, non-empty graphs, sum_g k_g}, word 0 stored last
 * (the caller polls it).  flags != 0 (1: not sorted, 2: an id outside [0, N], 4: more than 64 consecutive ids without a
 * node): nothing else is meaningful, take tgp_batch_facts_i64. */
int tgp_batch_facts_sorted_i64(const int64_t* batch, int64_t N, int64_t* ptr, int64_t* sizes, double topk_ratio,
                               int64_t* k, int64_t* koff, uint32_t* ticket, uint64_t* result, uint64_t tag,
                               void* stream);
/* to_dense_batch for a SORTED batch vector (graph b = nodes ptr[b] .. ptr[b+1]): output-parallel, padding and mask
 * written by the same kernel (no memsets in front).  zero_buf / zero_count (optional): a second float buffer to zero-fill
 * in the same launch (the adjacency tgp_to_dense_adj_f32 scatters into next). */
int tgp_to_dense_batch_sorted_f32(const float* x, int64_t num_nodes, int64_t F, const int64_t* ptr, int64_t B,
                                  int64_t Nmax, float* out, uint8_t* mask, float* zero_buf /* NULL ok */,
                                  int64_t zero_count, void* stream);
int tgp_to_dense_batch_f32(const float* x, int64_t num_nodes, int64_t num_features, const int64_t* batch,
                           const int64_t* ptr, int64_t B, int64_t Nmax, float* out, uint8_t* mask, void* stream);

/* A10  dense_to_block_diag (utils/ops.py:53-82): entries with |a| > 1e-8 in (b,row,col)
 * order, offset by b*K; optional valid-supernode mask [B*K] (src.py:526-552) drops and
 * renumbers supernodes (relabel[B*K] int64: new id or -1, NULL = keep all).             */
size_t tgp_block_diag_workspace_bytes(int64_t B, int64_t K);
int tgp_block_diag_count(const float* adj_pool, int64_t B, int64_t K, const int64_t* relabel /* NULL ok */,
                         int flags, float eps, void* ws, size_t ws_bytes, int64_t* d_count, void* stream);
int tgp_block_diag_fill(const float* adj_pool, int64_t B, int64_t K, const int64_t* relabel, int flags,
                        float eps, const void* ws, int64_t num_out, int64_t* out_row, int64_t* out_col,
                        float* out_weight, void* stream);

/* ------------------------------------------------------------------------------------
 * A14  NDPSelect._spectral_partition (select/ndp_select.py:187-256) for every graph of a batch, one workgroup each:
 *      largest eigenvector of Ls = I - D^-1/2 A D^-1/2 by a one-vector LOBPCG iteration (fp64, vectors and matrix in LDS), sign partition,
 *      cut = z^T L z / (2 vol), random +-1 partition (node 0 kept, node 1 dropped, rest from `seed`) when cut < 0.5.
 *      Input: CSR over all nodes (`indptr` [N+1], `col`, `w` or NULL = ones) of the SYMMETRIC adjacency without self
 *      loops (the caller symmetrises with max: to_undirected(reduce="max"), ndp_select.py:198-202); `graph_ptr` [B+1].
 *      Output: keep[v] = 1 for the positive side; info[g] = iterations used, -1 = random fallback, -2 = the graph is
 *      beyond tgp_ndp_max_graph_nodes(): left unpartitioned (keep = 0 on its nodes), the caller partitions those few
 *      graphs itself (pass max_graph_nodes = min(longest graph, tgp_ndp_max_graph_nodes()));
 *      *d_status: 0 ok, bit 1 = an entry that couples two graphs.
 * ---------------------------------------------------------------------------------- */
/* The symmetrisation in front of it (ndp_select.py:198-202: duplicates summed, self loops dropped, max with the
 * transpose) when the list already is row-major sorted, duplicate-free, loop-free and pattern-symmetric: w_out[e] =
 * max(w[e], w[reverse of e]) and *d_flag = 0; any violation (checked per entry; `indptr` = tgp_rowptr_from_sorted_i64 of
 * `row`) sets *d_flag = 1 and the caller takes the general coalesce route. */
int tgp_ndp_symmetric_max_f32(const int64_t* row, const int64_t* col, const float* w /* NULL = ones */, int64_t E,
                              int64_t num_nodes, const int32_t* indptr, float* w_out, int* d_flag, void* stream);
int tgp_ndp_max_graph_nodes(void);
int tgp_ndp_partition(const int32_t* indptr, const int64_t* col, const float* w /* NULL ok */, int64_t num_nodes,
                      int64_t nnz, const int64_t* graph_ptr, int64_t num_graphs, int64_t max_graph_nodes,
                      uint64_t seed, int max_iter, double tol, uint8_t* keep, int32_t* info, int* d_status,
                      void* stream);

/* One LARGE graph (beyond tgp_ndp_max_graph_nodes(); e.g. N = 1M, E = 10M of BASELINE configs[3]) on the whole
 * chip: the same LOBPCG iteration with every vector pass as a grid-wide kernel over fp64 work vectors in `ws`
 * (tgp_ndp_large_workspace_bytes(n): seven fp64 vectors + one fp32), scalars handed from kernel to kernel in device
 * memory.  The graph is the node range [p0, p1) of the same symmetric, self-loop-free CSR.
 *   start : degrees, start vector, first product.
 *   steps : `steps` LOBPCG steps (no-ops once |Ls x - lambda x| <= tol * lambda or max_iter steps are done);
 *           d_progress[0] = done flag, [1] = steps taken so far: the host reads it once per batch of steps.
 *   finish: sign partition, cut test, the reference's random fallback (ndp_select.py:171-185, 250-252);
 *           keep[p0 .. p1) is written, *info = steps used or -1 (random fallback).
 *   state : (diagnostics; synchronises the stream) lambda, |residual|^2, steps, random flag, cut. */
size_t tgp_ndp_large_workspace_bytes(int64_t num_graph_nodes);
int tgp_ndp_large_start(const int32_t* indptr, const int64_t* col, const float* w /* NULL ok */, int64_t p0,
                        int64_t p1, int max_iter, void* ws, size_t ws_bytes, int* d_status, void* stream);
int tgp_ndp_large_steps(const int32_t* indptr, const int64_t* col, const float* w, int64_t p0, int64_t p1, int steps,
                        double tol, void* ws, size_t ws_bytes, int32_t* d_progress, int* d_status, void* stream);
int tgp_ndp_large_finish(const int32_t* indptr, const int64_t* col, const float* w, int64_t p0, int64_t p1,
                         uint64_t seed, void* ws, size_t ws_bytes, uint8_t* keep, int32_t* info, void* stream);
int tgp_ndp_large_state(const void* ws, int64_t num_graph_nodes, double* out5, void* stream);

/* ------------------------------------------------------------------------------------
 * A9  KronConnect.forward (connect/kron_conn.py:117-165), block-batched: the batch Laplacian is block diagonal, so
 *     every graph's Kron reduction  L' = L[+,+] - L[+,-] L[-,-]^-1 L[-,+]  is independent.  The graph's dense
 *     Laplacian is formed in fp64 -- in LDS by one workgroup per graph up to 128 nodes; in a workspace slab, reduced
 *     panel by panel by many workgroups per graph, up to tgp_kron_batched_max_graph_nodes() -- the dropped nodes are
 *     eliminated, then A = -L', |A| > threshold, zero diagonal,
 *     fp32 cast; edges come out in row-major order of the pooled batch (what the reference's CSR -> COO gives).
 *     Entries: CSR over ALL nodes of the batch (`indptr` [N+1], `col` [nnz], values fp32 or fp64 or NULL = ones,
 *     optional `perm` = CSR slot -> entry).  from_adjacency = 0: the entries ARE the Laplacian (SelectOutput.L);
 *     from_adjacency = 1: they are edge weights and L = D - A is formed in the kernel (get_laplacian,
 *     kron_conn.py:88-92; self loops skipped, duplicates summed).  `graph_ptr` [B+1]: node offsets of the graphs
 *     (sorted batch vector); `node_index`: kept nodes, ascending (pooled id = position).  An exactly singular
 *     L[-,-] block is redone with the reference's 1e-6 I damping (kron_conn.py:131-135), per graph.
 *     *d_count = -1: declined (node_index not ascending, a graph beyond the size limit, or an entry that couples two
 *     graphs) - the caller keeps its generic route.  from_adjacency bit 1 (value 2, TGP_KRON_SKIP_OVERSIZE): graphs
 *     beyond the size limit do not decline the call, they are left out (no scratch, no edges) and the caller reduces
 *     those few graphs itself (pass max_graph_nodes = min(longest graph, tgp_kron_batched_max_graph_nodes())).
 * ---------------------------------------------------------------------------------- */
size_t tgp_kron_batched_workspace_bytes(int64_t num_nodes, int64_t num_graphs, int64_t max_graph_nodes,
                                        int64_t cap_dense, int64_t cap_big);
int tgp_kron_batched_max_graph_nodes(void);
/* cap_dense / cap_big: sizes (elements) of the k x k result buffer and of the fp64 scratch for graphs beyond the LDS
 * capacity.  Exact figures from the caller (sum over graphs of n_g^2; sum of n_g * (n_g | 1) over the graphs of more
 * than 128 nodes) keep the workspace at what the batch needs; -1 = the worst case from max_graph_nodes alone
 * (num_nodes * max_graph_nodes).  The real totals are checked on the device (too small: *d_count = -1).
 * num_big: how many graphs have more than 128 (and at most tgp_kron_batched_max_graph_nodes()) nodes, an upper
 * bound, -1 = unknown (num_graphs): it sizes the launches of the multi-workgroup elimination those graphs take.
 * node_rank (r6, optional, [num_nodes + 1] on the device): node_rank[i] = kept nodes in front of node i (so
 * node_rank[num_nodes] = num_kept), from a caller that compacted the kept nodes itself (tgp_mask_index_fill) and thereby
 * knows node_index to be ascending and in range: the call then skips its own flag scatter and scan (three launches). */
int tgp_kron_batched_count(const int32_t* indptr, const int64_t* col, const float* val32, const double* val64,
                           const int32_t* perm, int from_adjacency, int64_t num_nodes, int64_t nnz,
                           const int64_t* graph_ptr, int64_t num_graphs, int64_t max_graph_nodes, int64_t cap_dense,
                           int64_t cap_big, int64_t num_big, const int64_t* node_index, int64_t num_kept,
                           double threshold, const uint32_t* node_rank, void* ws, size_t ws_bytes, int64_t* d_count,
                           void* stream);
int tgp_kron_batched_fill(const void* ws, int64_t num_nodes, int64_t num_graphs, int64_t max_graph_nodes,
                          int64_t cap_dense, int64_t cap_big, int64_t num_big, const int64_t* graph_ptr,
                          int64_t num_out, int64_t* out_row, int64_t* out_col, float* out_weight,
                          const uint32_t* node_rank /* what the count call was given, or NULL */, void* stream);

/* A12, min_score mode (select/topk_select.py:186-194): prob = per-graph softmax of `score` (PyG utils.softmax: max
 * subtraction, +1e-16 in the denominator), kept = prob > min(max_g(prob) - tol, min_score) (PyG topk; tol 1e-7), kept
 * nodes in ascending order (nonzero()).  `ptr` [B+1]: node offsets of the graphs of the SORTED batch vector.  count
 * writes prob [N] and leaves the number of kept nodes in *d_count; fill writes node_index [num_out]. */
size_t tgp_topk_minscore_workspace_bytes(int64_t num_nodes, int64_t num_graphs);
int tgp_topk_minscore_count(const float* score, const int64_t* ptr, int64_t num_nodes, int64_t num_graphs,
                            float min_score, float tol, float* prob, void* ws, size_t ws_bytes, int64_t* d_count,
                            void* stream);
int tgp_topk_minscore_fill(const void* ws, const int64_t* ptr, int64_t num_nodes, int64_t num_graphs, int64_t num_out,
                           int64_t* node_index, void* stream);

/* ------------------------------------------------------------------------------------
 * A13  MLPSelect's last layer, one pass over the node features
 *   S[m,:] = softmax(X[m,:] W^T + b) * mask[m]       (select/mlp_select.py:139-145; single Linear(F,K): :67)
 * x [M,F], weight [K,F] (torch.nn.Linear layout), bias [K] or NULL, mask [M] bytes (0 = padded row) or NULL,
 * s_out [M,K]; all contiguous fp32.  K <= tgp_mlp_select_max_fused_k() (256: eight 32-column accumulator tiles per
 * wave); wider selectors run tgp_bmm_f32 for the logits and tgp_softmax_rows_f32 (bias + softmax + mask, in place).
 * tgp_softmax_bwd_f32: dY = S * (dS - <dS,S>_row), the gradient w.r.t. the logits (0 on masked rows, whose S is 0).
 * ---------------------------------------------------------------------------------- */
int tgp_mlp_select_max_fused_k(void);
int tgp_mlp_select_f32(const float* x, const float* weight, const float* bias, const unsigned char* mask, int64_t M,
                       int64_t F, int64_t K, float* s_out, void* stream);
int tgp_softmax_rows_f32(float* y, const float* bias, const unsigned char* mask, int64_t M, int64_t K, void* stream);
int tgp_softmax_bwd_f32(const float* s, const float* ds, float* dy, int64_t M, int64_t K, void* stream);
/* r5: the whole backward of that layer (K <= 32, F <= 64: tgp_mlp_select_bwd_fits) in one pass over S, dS and X: it
 * forms dY = S (dS - <dS,S>) and writes gx [M,F] = dY W (accumulate_gx != 0: adds to what gx holds -- the gradient the
 * pooling backward already left there), gw [K,F] = dY^T X and gb [K] = column sums of dY (gx / gw / gb may be NULL; gb
 * needs gw).  What autograd derives from select/mlp_select.py:139-145 as softmax backward + two matmul backwards + a bias
 * reduction + the accumulation of the two gradients of X: eight launches; here one, plus -- when gw is asked for -- a
 * second tiny one that adds the workgroups' partial gw / gb (in `ws`, tgp_mlp_select_bwd_workspace_bytes) in a fixed
 * order.  No float atomics: results are run-to-run identical. */
int tgp_mlp_select_bwd_fits(int64_t F, int64_t K);
size_t tgp_mlp_select_bwd_workspace_bytes(int64_t M, int64_t F, int64_t K);
int tgp_mlp_select_bwd_f32(const float* s, const float* ds, const float* x, const float* weight, int64_t M, int64_t F,
                           int64_t K, float* gx, int accumulate_gx, float* gw, float* gb, void* ws, size_t ws_bytes,
                           void* stream);

/* ------------------------------------------------------------------------------------
 * test hooks for the shared primitives (device-wide stable LSD radix sort, block scan)
 * ---------------------------------------------------------------------------------- */
size_t tgp_debug_sort_workspace_bytes(int64_t n);
int tgp_debug_sort_pairs_u64(const uint64_t* keys_in, const uint32_t* vals_in, int64_t n, int key_bits,
                             uint64_t* keys_out, uint32_t* vals_out, void* ws, size_t ws_bytes, void* stream);

/* Output contract of the single-call operators (r5).  tgp_sparse_pool_small_f32 and tgp_connect_subgraph_single write
 * survivors at their final offsets of CAPACITY-sized buffers; the reference hands out new tensors of exactly the pooled
 * size (connect/base_conn.py:103-112, SURVEY 8(b) "Ownership").  Once the count has arrived the caller allocates exact
 * outputs and this ONE launch moves the first n entries of the capacity arrays there (weight: 4- or 8-byte values or
 * NULL, edge_id: NULL ok), so edge_index is a contiguous [2, n] tensor and nothing pins E-sized scratch. */
int tgp_edges_compact(const int64_t* row, const int64_t* col, const void* weight, int weight_bytes,
                      const int64_t* edge_id, int64_t n, int64_t* out_row, int64_t* out_col, void* out_weight,
                      int64_t* out_edge_id, void* stream);
/* The same kernel for up to eight unrelated arrays (host arrays of `count` device pointers / byte counts, each a multiple
 * of 4): the merged outputs of a gathered step (tgp/data/collate.py:144-153) leave the receive buffer as exact-size
 * tensors in one launch. */
int tgp_copy_arrays(const void* const* src, void* const* dst, const int64_t* bytes, int count, void* stream);
/* r6: a byte mask [n] as the sorted list of its non-zero positions -- the `nonzero` with which NDPSelect turns its +-1
 * partition into the kept nodes, and the [2, k] index / value arrays of the one-node-per-supernode S built around it
 * (select/ndp_select.py:257-262, select/base_select.py:142-161).  tgp_mask_index_count: per-tile counts into `scratch`
 * (tgp_mask_index_scratch_words(n) 32-bit words, word 0 an arrival ticket that is zero between calls: clear the buffer
 * once), then {epoch << 34 | k} in the PINNED word `result` (k = -3 in 34-bit two's complement when `*declined` (device,
 * optional) is non-zero).  tgp_mask_index_fill, once the host has read k: pos_out[k] the positions in increasing order,
 * rank_out[k] = 0..k-1 and ones_out[k] = 1 (both optional); perm_out[k] = 0..k-1 (int32) and pack_out[k] = {uint32
 * position, fp32 1.0} (both optional): the one-to-one inverted index tgp_one_to_one_index_build would make of the three
 * arrays, for the Reduce of the same selection; node_rank_out[n + 1] (optional): non-zero bytes in front of every
 * position, total at [n] (what tgp_kron_batched_count takes as node_rank).  n < 2^31. */
int64_t tgp_mask_index_scratch_words(int64_t n);
int tgp_mask_index_count(const uint8_t* mask, int64_t n, const int32_t* declined, uint32_t* scratch, uint64_t* result,
                         uint32_t epoch, void* stream);
int tgp_mask_index_fill(const uint8_t* mask, int64_t n, const uint32_t* scratch, int64_t k, int64_t* pos_out,
                        int64_t* rank_out, float* ones_out, int32_t* perm_out, uint64_t* pack_out,
                        uint32_t* node_rank_out, void* stream);
/* r6: the host wait of tgp_sparse_pool_small_f32 + the launch that makes its edge_index contiguous, in one call (the
 * reference's own host reads: `.item()` in utils/ops.py:370-380 / the nonzero of connect/base_conn.py:79-89).  Spins on
 * the PINNED result word until call `epoch` has stored it; unless the kernel refused the input (bit 31 of the word) the
 * n = word & 0x7fffffff columns the kernel left in `col_scratch` are moved behind the n rows at the front of `out_rows`
 * (capacity >= 2 n: edge_index' [2, n] contiguous afterwards).  The caller reads the word from the pinned memory. */
int tgp_result_wait_pack_cols(const uint64_t* result, uint32_t epoch, const int64_t* col_scratch, int64_t* out_rows,
                              void* stream);

/* ------------------------------------------------------------------------------------
 * float64 value types of the HBM-bound operators (r4).  The reference's ATen ops compute model.double() inputs in fp64
 * (reduce/base_reduce.py:141-155, utils/ops.py:282-419); these entry points do the same for the operators that only
 * move and add values -- sparse Reduce, the edge-list Connect (subgraph / coalesce / block-diagonal export) and both
 * post-processings -- with the argument meaning of their fp32 twins above (`eps` as a double).  Same summation orders,
 * products rounded before the add.  (The dense GEMM path's fp64 forms follow in the next section, r5.)
 * ---------------------------------------------------------------------------------- */
int tgp_reduce_sparse_f64(const double* x, int64_t num_nodes, int64_t num_features, int64_t x_row_stride,
                          const int64_t* node_index, const double* weight /* NULL = ones */,
                          const int32_t* row_ptr /* NULL = one assignment per supernode */,
                          const int32_t* perm /* NULL = identity */, int64_t nnz, int64_t num_supernodes, double* x_pool,
                          void* stream);
int tgp_connect_subgraph_single_f64(const int64_t* row, const int64_t* col, const double* edge_weight /* NULL ok */,
                                    int64_t num_edges, const int64_t* node_index, int64_t k, int64_t num_nodes, int flags,
                                    double eps, void* ws /* tgp_connect_subgraph_single_workspace_bytes */,
                                    size_t ws_bytes, int64_t* out_row, int64_t* out_col, double* out_weight,
                                    int64_t* out_edge_id, const uint32_t* member_bits_in, const uint32_t* rank128_in,
                                    uint64_t* status, int64_t status_words, uint64_t* result, uint32_t epoch,
                                    void* stream);
size_t tgp_connect_coalesce_workspace_bytes_f64(int64_t num_edges, int64_t num_nodes, int64_t num_supernodes);
int tgp_connect_coalesce_count_f64(const int64_t* row, const int64_t* col, const double* edge_weight /* NULL ok */,
                                   int64_t num_edges, const int64_t* cluster_index, int64_t num_nodes,
                                   int64_t num_supernodes, int reduce_op, int flags, double eps, void* ws,
                                   size_t ws_bytes, int64_t* d_count, void* stream);
int tgp_connect_coalesce_fill_f64(const void* ws, int64_t num_edges, int64_t num_nodes, int64_t num_supernodes,
                                  int has_weight, int flags, int64_t num_out, int64_t* out_row, int64_t* out_col,
                                  double* out_weight, void* stream);
size_t tgp_postprocess_sparse_workspace_bytes_f64(int64_t num_edges, int64_t num_nodes, int64_t num_graphs);
int tgp_postprocess_sparse_norm_f64(const int64_t* row, const int64_t* col, double* edge_weight /* in place */,
                                    int64_t num_edges, int64_t num_nodes, int flags, double eps,
                                    const int64_t* batch_pooled, int64_t num_graphs, void* ws, size_t ws_bytes,
                                    void* stream);
int tgp_block_diag_count_f64(const double* adj, int64_t B, int64_t K, const int64_t* relabel, int flags, double eps,
                             void* ws /* tgp_block_diag_workspace_bytes */, size_t ws_bytes, int64_t* d_count,
                             void* stream);
int tgp_block_diag_fill_f64(const double* adj, int64_t B, int64_t K, const int64_t* relabel, int flags, double eps,
                            const void* ws, int64_t num_out, int64_t* out_row, int64_t* out_col, double* out_weight,
                            void* stream);
size_t tgp_postprocess_dense_workspace_bytes_f64(int64_t B, int64_t K);
int tgp_postprocess_dense_f64(const double* src, double* dst /* may alias src */, int64_t B, int64_t K, int flags,
                              double eps, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * float64 dense path (r5): S^T X, S^T A S and the products of their gradients on v_mfma_f64_16x16x4_f64.  The reference
 * computes model.double() inputs with torch.matmul in fp64 (reduce/base_reduce.py:158-161, connect/dense_conn.py:111-122;
 * unbatched: base_reduce.py:170-190, dense_conn.py:140-208); the host mirror routes float64 tensors here, so the dense
 * poolers pass torch.autograd.gradcheck in double.  Argument meaning of the fp32 twins above; same association
 * (U = A S, then S^T [U | X] over slices of the node range, slabs added in slice order).
 *   tgp_bmm_f64            C[b] (+)= op(A[b]) Bm[b]            (accumulate != 0: C += product)
 *   tgp_dense_pool_f64     fused A3 + A7 + A8 of a padded batch (flags: TGP_* of tgp_dense_pool_f32, incl. TGP_ADJ_TRANSPOSED)
 *   tgp_segment_gemm_*_f64 the per-graph products of an un-padded batch
 *   tgp_spmm_csr_f64       T = A S for a row-sorted coalesced edge list (w NULL = ones)
 * ---------------------------------------------------------------------------------- */
int tgp_bmm_f64(const double* A, const double* Bm, double* C, int64_t batch, int64_t M, int64_t Nc, int64_t Kd,
                int trans_a, int64_t lda, int64_t ldb, int64_t ldc, int64_t sA, int64_t sB, int64_t sC, int accumulate,
                void* stream);
size_t tgp_dense_pool_workspace_bytes_f64(int64_t B, int64_t N, int64_t K, int64_t F);
int tgp_dense_pool_f64(const double* S, const double* A /* NULL ok */, const double* X /* NULL ok */, int64_t B,
                       int64_t N, int64_t K, int64_t F, int flags, double eps, double* x_pool, double* adj_raw,
                       double* adj_pool, void* ws, size_t ws_bytes, void* stream);
size_t tgp_segment_gemm_tn_workspace_bytes_f64(int64_t B, int64_t K, int64_t F, int64_t max_nodes);
int tgp_segment_gemm_tn_f64(const double* S, const double* Y, const int64_t* ptr, double* C, int64_t B, int64_t Ntot,
                            int64_t K, int64_t F, int64_t max_nodes, void* ws, size_t ws_bytes, void* stream);
int tgp_segment_gemm_nn_f64(const double* A, const double* Bm, const int64_t* ptr, double* C, int64_t B, int64_t Ntot,
                            int64_t Kd, int64_t Nc, int64_t max_nodes, void* stream);
int tgp_spmm_csr_f64(const int32_t* row_ptr, const int64_t* col, const double* w, int64_t num_rows, int64_t nnz,
                     const double* S, int64_t K, double* T, void* stream);

/* ------------------------------------------------------------------------------------
 * pack / unpack of the variable-size all-gather of pooled sparse outputs (r4).  A rank's pooled graphs
 * (x [K,F], batch [K] int64 or NULL, edge_index rows [E] int64, edge_weight [E] or NULL) go into one byte buffer of
 * `capacity` bytes behind a 128-byte header {magic, K, E, B, F, w_words, needed_bytes, x_words}; when needed_bytes >
 * capacity only the header is written (every rank then sees how much room the largest rank needs).  r5: the VALUES
 * travel as 4-byte words -- `F` and `x_row_stride` count words per feature row, `x_words` / `w_words` the words per
 * element (1 = fp32 / int32, 2 = fp64 / int64; w_words 0 = no weights) -- so float64 features and weights cross ranks
 * bit for bit (they were narrowed to fp32 before).  The buffers of all ranks are all-gathered as they are;
 * tgp_gather_unpack_f32 reads `world` of them ([world, capacity] bytes) and writes the merged tensors, node ids of rank
 * r shifted by the supernodes, graph ids by the graphs of the ranks before it (tgp/data/collate.py:144-153).  Output
 * sizes = sums over the headers (the caller reads them once).
 * ---------------------------------------------------------------------------------- */
int64_t tgp_gather_pack_bytes(int64_t num_supernodes, int64_t num_edges, int64_t feature_words, int w_words);
int tgp_gather_pack_f32(const float* x, int64_t x_row_stride, const int64_t* batch /* NULL ok */, const int64_t* row,
                        const int64_t* col, const float* edge_weight /* NULL ok */, int64_t num_supernodes,
                        int64_t num_edges, int64_t num_graphs, int64_t feature_words, int w_words, int x_words,
                        int64_t capacity, void* out, void* stream);
int tgp_gather_unpack_f32(const void* gathered, int64_t capacity,
                          int64_t rank_stride /* bytes between two ranks' buffers (>= capacity: several steps' slots may be
                                                 gathered as one bucket) */,
                          int world, int64_t max_words /* 4-byte words of the largest payload: sizes the grid */,
                          int64_t k_cap, int64_t e_cap /* rows the outputs can hold */,
                          int64_t feature_words, int w_words, int x_words /* what THIS rank packed: every header must
                                                                             say the same */,
                          float* x_out, int64_t* batch_out /* NULL ok */, int64_t* row_out, int64_t* col_out,
                          float* weight_out /* NULL ok */,
                          uint64_t* result /* NULL, or 5 words of device-accessible (pinned host) memory: {tag, K total,
                                              E total, largest needed_bytes, status}, word 0 stored last.  status bits:
                                              1 = every header valid, 2 = every rank agrees on feature_words / w_words /
                                              x_words, 4 = the totals fit k_cap / e_cap; a payload that does not fit
                                              capacity, or a status other than 7, makes the launch a no-op apart from
                                              this report */,
                          uint64_t tag, void* stream);
/* The same for a whole BUCKET of steps in one launch each (r4): step j of at most tgp_gather_max_bucket_steps() (= 8) is
 * packed into out + j * capacity; after the single collective over the bucket ([world][n * capacity] bytes, rank_stride =
 * n * capacity or more) one launch unpacks all its steps.  ptrs / dims are HOST arrays read during the call:
 *   pack:   ptrs [n][5] = {x, batch (NULL ok), row, col, edge_weight (NULL ok)}, dims [n][7] = {x_row_stride,
 *           num_supernodes, num_edges, num_graphs, feature_words, w_words, x_words};
 *   unpack: ptrs [n][6] = {x_out, batch_out (NULL ok), row_out, col_out, weight_out (NULL ok), result (NULL ok)},
 *           dims [n][6] = {k_cap, e_cap, tag, feature_words, w_words, x_words}. */
int tgp_gather_max_bucket_steps(void);
int tgp_gather_pack_bucket_f32(const void* const* ptrs, const int64_t* dims, int num_steps, int64_t capacity, void* out,
                               void* stream);
int tgp_gather_unpack_bucket_f32(const void* gathered, int64_t capacity, int64_t rank_stride, int world,
                                 int64_t max_words, int num_steps, void* const* ptrs, const int64_t* dims, void* stream);

/* ------------------------------------------------------------------------------------
 * LaPool's selector (reference select/lapool_select.py), csrc/lapool.hip.  fp32, no float atomics, the same bits on
 * every call; no buffer of N_total x K_total elements.
 * Layouts.  Padded batch: ptr NULL, rows = B N, graph b owns rows b N .. b N + N - 1, `mask` ([B N] bytes, NULL = every
 * row real) marks the real ones.  Un-padded batch: ptr [B + 1] (int64 row offsets), no mask, `batch` [rows] names each
 * row's graph (NULL only with B <= 1); rows of a graph are contiguous.
 *   variation   v_i = || deg_i x_i - sum_j a_ij x_j ||_2, deg_i = sum_j a_ij.  dense: rows and columns of padded nodes
 *               count as zero, v = 0 on padded rows, one pass over A (16-byte loads when N % 4 == 0 and A is 16-byte
 *               aligned).  csr: an edge list grouped by source (row_ptr [n + 1], perm [E] edge positions or NULL =
 *               identity, col [E] by edge position, w NULL = ones); self-loops are dropped, duplicates add, an endpoint
 *               outside [0, n) is skipped.
 *   flags       1 where v_i >= v_j for every neighbour j (dense: a_ij != 0 on real columns; csr: the entries left after
 *               self-loop removal, explicit zeros included), 0 elsewhere and on padded rows.
 *   columns     per graph: with fallback != 0 a graph that has a real row and no leader makes every real row a leader
 *               (flags is rewritten); col_of [rows] = a leader's rank among its graph's leaders, -1 otherwise;
 *               leaders [rows]: graph b's leader rows, ascending, stored from the graph's first row on; k [B];
 *               *k_max = max_b k_b (device word, zeroed by the call).
 *   assign      nrm [rows] = ||x_i||_2 and S [rows, K]: a padded row is 0, a leader row its one-hot column, every other
 *               row softmax_c( x_i . x_l(c) / (|x_i| |x_l(c)| + eps) ) over its own graph's k_b leaders; columns >= k_b
 *               are 0.  K >= max_b k_b.
 *   assign_bwd  dX [rows, F] from dS: through the softmax and the cosine to the row itself and to the leaders it was
 *               compared with; leader and padded rows of dS are not read.  g1, g2 [rows, K] and alpha [rows] are work
 *               buffers of the caller.
 * TGP_ERR_INVALID: a NULL output or input, a layout that contradicts itself; TGP_ERR_RANGE: rows, N, F, K or E beyond
 * the int32 internals.  Both are found before any HIP call.
 * ---------------------------------------------------------------------------------- */
int tgp_lapool_variation_dense_f32(const float* A, const float* X, int64_t B, int64_t N, int64_t F,
                                   const uint8_t* mask /* NULL ok */, float* v, void* stream);
int tgp_lapool_variation_csr_f32(const int32_t* row_ptr, const int32_t* perm /* NULL ok */, const int64_t* col,
                                 const float* w /* NULL ok */, const float* X, int64_t n, int64_t E, int64_t F, float* v,
                                 void* stream);
int tgp_lapool_flags_dense_f32(const float* A, const float* v, int64_t B, int64_t N, const uint8_t* mask /* NULL ok */,
                               uint8_t* flags, void* stream);
int tgp_lapool_flags_csr_f32(const int32_t* row_ptr, const int32_t* perm /* NULL ok */, const int64_t* col,
                             const float* v, int64_t n, int64_t E, uint8_t* flags, void* stream);
int tgp_lapool_columns(uint8_t* flags, int64_t rows, int64_t B, int64_t N, const uint8_t* mask /* NULL ok */,
                       const int64_t* ptr /* NULL: padded */, int fallback, int32_t* col_of, int32_t* leaders, int32_t* k,
                       int64_t* k_max, void* stream);
int tgp_lapool_assign_f32(const float* X, int64_t rows, int64_t F, int64_t B, int64_t N, const uint8_t* mask /* NULL ok */,
                          const int64_t* ptr /* NULL: padded */, const int64_t* batch /* NULL ok */,
                          const int32_t* col_of, const int32_t* leaders, const int32_t* k, int64_t K, float eps,
                          float* nrm, float* S, void* stream);
int tgp_lapool_assign_bwd_f32(const float* X, const float* nrm, const float* S, const float* dS, int64_t rows, int64_t F,
                              int64_t B, int64_t N, const uint8_t* mask /* NULL ok */,
                              const int64_t* ptr /* NULL: padded */, const int64_t* batch /* NULL ok */,
                              const int32_t* col_of, const int32_t* leaders, const int32_t* k, int64_t K, float eps,
                              float* g1, float* g2, float* alpha, float* dX, void* stream);

/* ------------------------------------------------------------------------------------
 * SAGPooling's scorer (reference poolers/sag.py with PyG's GraphConv / SAGEConv at one output channel),
 * csrc/sag_score.hip.  fp32, no float atomics, the same bits on every call; nothing of size E x F or N x F is formed.
 *   row_project2  out0[i] = <x[i,:], w0>, out1[i] = <x[i,:], w1> from ONE pass over x (row stride ldx >= F; 16-byte
 *                 loads when x is 16-byte aligned and ldx % 4 == 0, a row's last F % 4 columns by scalar loads).
 *   aggregate     t[i] = (sum over group i of p[src[pos]] [/ max(size of group i, 1) when mean] + bias[0]) + q[i],
 *                 a[i] = act(t[i]), act 0 = identity, 1 = tanh.  Group i = positions grp_perm[grp_ptr[i] .. grp_ptr[i+1])
 *                 of the edge list (grp_perm NULL: the positions themselves, a list already grouped), added in that
 *                 order.  A src outside [0, N) or a position outside [0, E) is skipped, never dereferenced (it still
 *                 counts in the group's size).  With the by-destination index and src = the source row this is the
 *                 forward; with the by-source index and src = the destination row it is the backward's g_p.
 *   bwd_x         g_x[i,:] = g_q[i] w_root + g_p[i] w_rel (accumulate != 0: added to what g_x holds); g_x is [N,F]
 *                 contiguous.
 * TGP_ERR_INVALID: a NULL input or output, p given as an output, sizes below zero; TGP_ERR_RANGE: N or E beyond the int32
 * index, F >= 2^31.  Both are found before any HIP call.
 * ---------------------------------------------------------------------------------- */
int tgp_row_project2_f32(const float* x, int64_t N, int64_t F, int64_t ldx, const float* w0, const float* w1, float* out0,
                         float* out1, void* stream);
int tgp_sag_aggregate_f32(const int32_t* grp_ptr, const int32_t* grp_perm /* NULL: list already grouped */,
                          const int64_t* src, const float* p, const float* q /* NULL ok */,
                          const float* bias /* NULL ok; one device float */, int64_t N, int64_t E, int mean, int act,
                          float* t_out /* NULL ok */, float* a_out /* NULL ok, not both */, void* stream);
int tgp_sag_score_bwd_x_f32(const float* g_q, const float* g_p, const float* w_root, const float* w_rel, int64_t N,
                            int64_t F, int accumulate, float* g_x, void* stream);

/* ------------------------------------------------------------------------------------
 * ASAPooling's fitness (reference poolers/asap.py:205-237 with PyG's LEConv at one output channel), csrc/asap.hip.
 * fp32, no float atomics, the same bits on every call; nothing of size E x F is formed and the F x F Linear is never
 * applied to a row.  Every entry takes an edge group as the SAG aggregate does: group i = positions
 * grp_perm[grp_ptr[i] .. grp_ptr[i+1]) of the edge list (grp_perm NULL: the positions themselves), src the endpoint
 * gathered through a position.  A position outside [0, E) or an endpoint outside its range is skipped, never
 * dereferenced.
 *   query         sq[i] = <max over group i of x_pool[src,:], w_tilde> + c[0]; an empty group gives c[0]; a NaN among
 *                 the candidates of a column gives NaN (torch's amax).  Rows of x_pool have stride ldx >= F; 16-byte
 *                 loads under row_project2's rule.
 *                 With argpos ([N,F] int32) it also writes the edge POSITION that gave each maximum: the lowest
 *                 position among equal candidates, the lowest NaN position when a NaN wins, -1 for an empty group.
 *                 Positions, not source ids: a by-source backward that matched ids would count a duplicate edge twice.
 *   edge_softmax  alpha[pos] = exp(l - m_i) / (sum over group i of exp(l - m_i) + 1e-16), l = leaky_relu(sq[i] + sp[src]),
 *                 written at the edge's own position (an edge whose endpoint is out of range gets 0).
 *   attend        out[i,:] = sum over group i of val[pos] x[src,:] (val NULL: 1), out [N,F] contiguous, x [N_src,F] with
 *                 row stride ldx; with w3 ([3,F] contiguous) also p[k*N + i] = <out[i,:], w3[k,:]>, k = 0, 1, 2, taken from
 *                 the finished row in registers.  By destination with src = the source row it is x_new; by source with
 *                 src = the destination row and x = a gradient of x_new it is that gradient's pull-back to x.
 *   leconv        t[i] = ((p[2N+i] + b3) + sum_e w_e p[src_e]) + (b1 - p[N+i]) sum_e w_e over group i in its order
 *                 (w_e = edge_weight[pos], or 1), a[i] = act(t[i]), act 0 = identity, 1 = tanh, 2 = sigmoid.
 *   edge_dot      out[pos] = <g[i,:], x[src,:]> for every edge of group i (g [N,F] contiguous): the backward's g_alpha.
 *   softmax_bwd   d = sum over group i of alpha g_alpha; g_l[pos] = alpha (g_alpha - d) * (sq[i] + sp[src] > 0 ? 1 :
 *                 negative_slope); g_sq[i] = sum over group i of g_l.
 *   query_bwd     out[j,f] = w_tilde[f] * sum over group j (BY SOURCE, dst the gathered endpoint) of g_sq[dst] where
 *                 argpos[dst,f] is that edge's position: the master query's backward, out [N,F] contiguous.
 * The orders of the sums are those of csrc/asap.hip's head comment.  One wave walks one group in query, edge_softmax and
 * attend, whatever its length.
 * TGP_ERR_INVALID: a NULL input or output, an input given as the output, sizes below zero, ldx < F, an unknown act;
 * TGP_ERR_RANGE: N or E beyond the int32 index, F >= 2^31.  Both are found before any HIP call.
 * ---------------------------------------------------------------------------------- */
int tgp_asap_query_f32(const int32_t* grp_ptr, const int32_t* grp_perm /* NULL: list already grouped */,
                       const int64_t* src, const float* x_pool, int64_t ldx, const float* w_tilde,
                       const float* c /* one device float */, int64_t N, int64_t E, int64_t F, float* sq,
                       int32_t* argpos /* NULL ok; [N,F] */, void* stream);
int tgp_asap_edge_softmax_f32(const int32_t* grp_ptr, const int32_t* grp_perm /* NULL ok */, const int64_t* src,
                              const float* sq, const float* sp, int64_t N, int64_t E, float negative_slope, float* alpha,
                              void* stream);
int tgp_asap_attend_f32(const int32_t* grp_ptr, const int32_t* grp_perm /* NULL ok */, const int64_t* src,
                        const float* val /* NULL ok */, const float* x, int64_t ldx, const float* w3 /* NULL ok */,
                        int64_t N, int64_t N_src, int64_t E, int64_t F, float* out, float* p /* NULL iff w3 is */,
                        void* stream);
int tgp_asap_leconv_f32(const int32_t* grp_ptr, const int32_t* grp_perm /* NULL ok */, const int64_t* src,
                        const float* edge_weight /* NULL ok */, const float* p, const float* b1 /* NULL ok */,
                        const float* b3 /* NULL ok */, int64_t N, int64_t E, int act, float* t_out /* NULL ok */,
                        float* a_out /* NULL ok, not both */, void* stream);

int tgp_asap_edge_dot_f32(const int32_t* grp_ptr, const int32_t* grp_perm /* NULL ok */, const int64_t* src,
                          const float* g, const float* x, int64_t ldx, int64_t N, int64_t E, int64_t F, float* out,
                          void* stream);
int tgp_asap_softmax_bwd_f32(const int32_t* grp_ptr, const int32_t* grp_perm /* NULL ok */, const int64_t* src,
                             const float* alpha, const float* g_alpha, const float* sq, const float* sp, int64_t N,
                             int64_t E, float negative_slope, float* g_l, float* g_sq, void* stream);
int tgp_asap_query_bwd_f32(const int32_t* grp_ptr, const int32_t* grp_perm /* NULL ok */, const int64_t* dst,
                           const int32_t* argpos, const float* g_sq, const float* w_tilde, int64_t N, int64_t E,
                           int64_t F, float* out, void* stream);

/* ------------------------------------------------------------------------------------
 * Segment readout (reference reduce/aggr_reduce.py, reduce/global_reduce.py over PyG's Sum / Mean / Max / Min /
 * MultiAggregation), csrc/segment_aggr.hip.  fp32, no float atomics, the same bits on every call.
 *   `ops` is a mask of (1 << TGP_SUM) | (1 << TGP_MEAN) | (1 << TGP_MIN) | (1 << TGP_MAX); ONE pass over x fills
 *   out [G, n_ops * F], the requested operations side by side in enum order (sum, mean, min, max).  An empty group
 *   gives 0 for every operation, the mean divides by max(count, 1), min / max are exact and NaN wins as in
 *   torch.amax / amin.  Row source, exactly one of:
 *     ptr [G + 1]      group g owns rows ptr[g] .. ptr[g + 1] - 1 of x (a sorted batch vector's offsets);
 *     dense_nodes > 0  x is [G, dense_nodes, F] (num_rows = G * dense_nodes), `mask` ([num_rows] bytes, NULL = every
 *                      row) names the rows that exist: the others are neither loaded nor counted;
 *     node_index       gathered rows x[node_index[a], :] * weight[a] over the supernode -> assignment index of a
 *                      sparse assignment (row_ptr [G + 1] and perm [nnz] of tgp_assign_index_build; row_ptr NULL: one
 *                      assignment per group, perm [G] or NULL = identity; weight NULL = ones); the product is rounded
 *                      before the add, as in tgp_reduce_sparse_f32.  A position, assignment or row outside its table
 *                      is skipped, never dereferenced.
 *   Every (group, feature) is added in ascending row order by one lane.  max_len is an upper bound of the longest
 *   group (it only chooses the route, never the result's validity): beyond tgp_segment_aggr_chunk_rows() rows the
 *   segments are cut into row chunks whose partial records (`ws`, tgp_segment_aggr_workspace_bytes; 0 = not needed)
 *   a second kernel folds in a fixed order (runs of consecutive chunks, then the runs, both ascending).  16-byte
 *   loads when F % 4 == 0, ldx % 4 == 0 and x / out / ties are 16-byte aligned; scalar loads otherwise.
 *   ties (NULL ok) [G, n_mm * F] int32, min then max: the number of rows that attain the extreme; count (NULL ok) [G]
 *   int32: the rows of each group.  The backward reads both.
 *   bwd: dx [num_rows, F] (contiguous) = sum over the requested operations of g, g / max(count, 1) and
 *   g [x == out] / ties, written once; g_out and out are [G, n_ops * F].  `batch` [num_rows] names every row's group
 *   (NULL: the dense layout, or one group); rows of a group outside [0, G) and masked rows get 0.  The gathered
 *   source has no native backward.
 * TGP_ERR_INVALID: no or several row sources, an empty or unknown ops mask, a NULL input or output, sizes below
 * zero; TGP_ERR_RANGE: G, num_rows * F or nnz beyond the int32 range.  Both are found before any HIP call.
 * ---------------------------------------------------------------------------------- */
int tgp_segment_aggr_chunk_rows(void);
size_t tgp_segment_aggr_workspace_bytes(int64_t G, int64_t F, int ops, int64_t max_len);
int tgp_segment_aggr_f32(const float* x, int64_t num_rows, int64_t F, int64_t ldx, const int64_t* ptr /* NULL ok */,
                         int64_t dense_nodes, const uint8_t* mask /* NULL ok */, const int32_t* row_ptr /* NULL ok */,
                         const int32_t* perm /* NULL ok */, const int64_t* node_index /* NULL ok */,
                         const float* weight /* NULL ok */, int64_t nnz, int64_t G, int64_t max_len, int ops, float* out,
                         int32_t* ties /* NULL ok */, int32_t* count /* NULL ok */, void* ws, size_t ws_bytes,
                         void* stream);
int tgp_segment_aggr_bwd_f32(const float* g_out, const float* x, int64_t num_rows, int64_t F, int64_t ldx,
                             const int64_t* batch /* NULL ok */, int64_t dense_nodes, const uint8_t* mask /* NULL ok */,
                             const float* out, const int32_t* ties, const int32_t* count, int64_t G, int ops, float* dx,
                             void* stream);

/* ------------------------------------------------------------------------------------
 * MaxCutPooling (reference select/maxcut_select.py, utils/ops.py delta_gcn_matrix and propagate_assignments_sparse,
 * utils/losses.py maxcut_loss), csrc/maxcut.hip.  fp32, no float atomics, the same bits on every call.  grp_ptr [N + 1]
 * and grp_perm [E] (NULL: the list is already grouped) are the edge positions by destination or by source, edge-list
 * order inside a node; `other` is the row of the opposite endpoints.  One wave walks one group whatever its length.
 *   degree:  over the by-source group, deg_i = the summed weight of i's out-edges that are not self-loops (weight NULL:
 *            ones), dinv = deg^-1/2 with inf -> 0; then coef[e] = w_e dinv[src_e] and coef_t[e] = w_e dinv[dst_e]
 *            (either NULL: not written).
 *   layer:   h_i = act((1 - delta) [i < n_p] z_i + (delta dinv_i) sum over i's group, self-loops skipped, of
 *            coef[e] z[other_e] + bias), z [N, C], C in 1 .. tgp_maxcut_max_width(); n_p one DEVICE word (NULL: N);
 *            act 0 identity, 1 tanh, 2 relu.  h_out [N, C] (NULL ok) and, with w_next [C_next, C], z_next = h w_next^T
 *            [N, C_next] (both NULL and C_next 0: no projection); at least one output.  A slot of the wave adds every
 *            (64 / G)-th edge of the group in group order (G = C rounded up to a power of two), the slots fold at
 *            offsets 32 .. G, the projection adds the channels in ascending order.
 *   tail:    score_i = act(<mlp(h_i), w> + b): n_layers Linear + mlp_act (widths [n_layers], a HOST array, every width
 *            in 1 .. tgp_maxcut_max_width()), then Linear(., 1).  params packs, per layer, W [out, in] and b [out], then
 *            w and b; n_params must be exactly that count and at most tgp_maxcut_tail_max_params().
 *   wgrad:   out [Ca, Cb] = a^T b for a [N, Ca], b [N, Cb]: partial sums of 1024 consecutive rows each (ws,
 *            tgp_maxcut_wgrad_workspace_bytes), added in ascending chunk order.
 *   cut:     az_i = sum over i's group of w_e s[other_e] (self-loops and duplicates included), cut_i = s_i az_i,
 *            wsum_i = sum of w_e; any of the three outputs may be NULL, not all.
 *   assign_round: one round of label propagation over the by-destination group.  Labels 1 .. K, 0 = none; a labelled
 *            node keeps its label, another takes the label most of its labelled sources carry (duplicates counted, the
 *            lowest label on a tie), or stays 0.  Reads label_in only.
 * TGP_ERR_INVALID: a NULL input or output, an input given as an output, sizes below zero, a width outside its range, an
 * unknown act, a parameter count that does not fit the widths; TGP_ERR_RANGE: N or E beyond the int32 index;
 * TGP_ERR_WORKSPACE: ws_bytes below the query.  All are found before any HIP call.
 * ---------------------------------------------------------------------------------- */
int tgp_maxcut_max_width(void);
int tgp_maxcut_tail_max_params(void);
int tgp_maxcut_degree_f32(const int32_t* grp_ptr, const int32_t* grp_perm /* NULL ok */, const int64_t* src,
                          const int64_t* dst, const float* edge_weight /* NULL ok */, int64_t N, int64_t E, float* dinv,
                          float* coef /* NULL ok */, float* coef_t /* NULL ok */, void* stream);
int tgp_maxcut_layer_f32(const int32_t* grp_ptr, const int32_t* grp_perm /* NULL ok */, const int64_t* other,
                         const float* coef, const float* dinv, const float* z, const float* bias /* NULL ok */, int64_t N,
                         int64_t E, int64_t C, const int64_t* n_p /* NULL ok */, float delta, int act,
                         float* h_out /* NULL ok */, const float* w_next /* NULL ok */, int64_t C_next,
                         float* z_next /* NULL iff w_next is */, void* stream);
int tgp_maxcut_tail_f32(const float* h, int64_t N, int64_t C, const int64_t* widths /* host */, int64_t n_layers,
                        const float* params, int64_t n_params, int mlp_act, int act, float* score, void* stream);
size_t tgp_maxcut_wgrad_workspace_bytes(int64_t N, int64_t Ca, int64_t Cb);
int tgp_maxcut_wgrad_f32(const float* a, const float* b, int64_t N, int64_t Ca, int64_t Cb, float* out, void* ws,
                         size_t ws_bytes, void* stream);
int tgp_maxcut_cut_f32(const int32_t* grp_ptr, const int32_t* grp_perm /* NULL ok */, const int64_t* other,
                       const float* edge_weight /* NULL ok */, const float* s, int64_t N, int64_t E,
                       float* az /* NULL ok */, float* cut /* NULL ok */, float* wsum /* NULL ok */, void* stream);
int tgp_maxcut_assign_round_i32(const int32_t* grp_ptr, const int32_t* grp_perm /* NULL ok */, const int64_t* src,
                                const int32_t* label_in, int64_t N, int64_t E, int32_t* label_out, void* stream);

/* ------------------------------------------------------------------------------------
 * EigenPooling (reference select/eigenpool_select.py, reduce/eigenpool_reduce.py, lift/eigenpool_lift.py),
 * csrc/eigenpool.hip.  The reference's pooling matrix Theta [n, K H] has at most H non-zeros per row; it is kept as
 * theta_modes [N, H] (node i's entry in mode h of its own cluster) plus the inverted index of the groups, a group being
 * a (graph, cluster) pair: theta_ptr [G + 1] and theta_perm [N] of tgp_assign_index_build over gid [N] (ascending node
 * index inside a group).
 *   modes:   one workgroup per group.  The induced sub-adjacency is gathered from the by-source edge index (grp_ptr
 *            [N + 1], grp_perm [E] or NULL for a list that is grouped already; duplicates are added in edge-list order
 *            in fp32), the reference's Laplacian is formed in float64 (degrees = column sums; normalized: plus the
 *            smallest positive fp32 subnormal, L = I - D^-1/2 A D^-1/2; otherwise D - A) and solved by a cyclic Jacobi
 *            iteration with a fixed round-robin rotation order.  Eigenpairs ascending, ties to the lower column; mode
 *            h of a group of m nodes is eigenvector min(h, m - 1), negated when its first entry (the group's lowest
 *            node) is negative; a one-node group gets its self-loop weight in all H modes; an empty group writes
 *            nothing.  embed != 0 (needs normalized): every row is scaled by deg^-1/2 (1 for a node without induced
 *            edges), the spectral embedding of the labeller.  deg [N] (NULL ok): the column sums.  One rounding to
 *            fp32 at the end.  A group whose Laplacian has a NaN or an infinite entry gets NaN in all its modes (eigh
 *            refuses such a matrix); the other groups are not touched by it.
 *            max_m in 1 .. tgp_eigenpool_max_group_nodes() sizes the LDS frame (an upper bound of the largest group).
 *            *status (one zeroed device word) collects: bit 0 an index outside its table (a member that is not a node
 *            of its group, an unsorted member list, an edge position or endpoint out of range), bit 1 a group whose
 *            induced adjacency is not symmetric, bit 2 a group of more than max_m nodes.  A flagged group is left
 *            unwritten; nothing out of range is dereferenced.
 *   reduce:  out [G, H F]: out[g, h F + f] = sum over the group's nodes, ascending, of theta[i, h] x[i, f].  A row of x
 *            is read once for (up to 8) modes; one lane adds every (group, mode, feature): no float atomics, the same
 *            bits on every call.  max_len is an upper bound of the longest group (it only chooses the route, never the
 *            result's validity; 0 = short groups): beyond 128 rows 4, beyond 1024 rows 16 waves share a group, each
 *            adding one run of consecutive rows, the runs folded in ascending order.  An empty group gives a zero
 *            row; a member outside [0, N) is skipped.
 *   lift:    out [N, F]: out[i, f] = sum_h theta[i, h] x_pool[gid[i], h F + f]; a node whose gid is outside [0, G) gets
 *            zeros.  reduce and lift are each other's adjoint.
 * TGP_ERR_INVALID: a NULL input or output, an input given as the output, sizes below zero, H < 1, ldx < F, max_m
 * outside its range; TGP_ERR_RANGE: N, E, G or F beyond the int32 index.  All are found before any HIP call.
 * ---------------------------------------------------------------------------------- */
int tgp_eigenpool_max_group_nodes(void);
int tgp_eigenpool_modes_f32(const int32_t* grp_ptr, const int32_t* grp_perm /* NULL ok */, const int64_t* dst,
                            const float* edge_weight /* NULL ok */, const int32_t* gid, const int32_t* theta_ptr,
                            const int32_t* theta_perm, int64_t N, int64_t E, int64_t G, int64_t H, int64_t max_m,
                            int normalized, int embed, float* theta_modes, float* deg /* NULL ok */, int32_t* status,
                            void* stream);
int tgp_eigenpool_reduce_f32(const float* theta_modes, const int32_t* theta_ptr, const int32_t* theta_perm,
                             const float* x, int64_t ldx, int64_t N, int64_t G, int64_t H, int64_t F, int64_t max_len,
                             float* out, void* stream);
int tgp_eigenpool_lift_f32(const float* theta_modes, const int32_t* gid, const float* x_pool, int64_t N, int64_t G,
                           int64_t H, int64_t F, float* out, void* stream);

/* ------------------------------------------------------------------------------------
 * NMF pooling (reference select/nmf_select.py), csrc/nmf.hip: A ~ W H per graph by scikit-learn's coordinate descent
 * (solver "cd", shuffle off, no regularisation), S = softmax(H^T).  One workgroup per graph; the graph's nodes come from
 * the inverted index of gid [N] (graph_ptr [G + 1], graph_perm [N] of tgp_assign_index_build: ascending node index inside
 * a graph, which is the node's LOCAL index), its edges from the by-source edge index (grp_ptr [N + 1], grp_perm [E] or
 * NULL for a list that is grouped already).  Duplicate edges are added in edge-list order in fp32, the sum is clamped at
 * 0.  With n nodes and ka = max(1, min(K, n)):  n > 1 and ka >= n gives the identity, ka == 1 a column of ones, both
 * without a factorisation; otherwise W [n, ka] and H^T [n, ka] start from the explicit init (w0, h0t [N, K] node-major,
 * columns >= ka ignored, both or neither) or from the default one, avg * 2u with avg = sqrt(mean(A) / ka) and u in (0, 1]
 * a 32-bit hash of (seed, factor, local node index, component), and iteration it = 1 .. max_iter updates W, then H:
 *     Gram = F^T F, P = A F (A^T F for H), F the other factor; per row i, t = 0 .. ka - 1 in order:
 *     grad = -P[i,t] + sum_r Gram[t,r] U[i,r];  violation += |U[i,t] == 0 ? min(0, grad) : grad|;
 *     if Gram[t,t] != 0: U[i,t] = max(U[i,t] - grad / Gram[t,t], 0)
 * and stops when the first iteration's violation is 0 or violation / first violation <= tol (a NaN ratio runs to
 * max_iter).  All sums are fp32 in ascending index order (the row violations: lane l of one wave adds rows l, l + 64, then
 * an xor butterfly); no fused multiply-add, no float atomics: the same bits on every call.
 *   factorize: s [N, out_cols] gets softmax over the ka columns and zeros behind them (out_cols >= ka of every graph).
 *              Optional (NULL ok): w_out, ht_out [N, K] the raw factors (zeros behind column ka; not written for a
 *              graph that is not factorised), iters [G] the iteration at which a factorised graph stopped,
 *              violation_ratio [G] its last ratio (0 when the first violation is 0).
 *   init:      w0, h0t [N, K] of the default init alone (rows of graphs that are not factorised are not written).
 * max_n in 1 .. tgp_nmf_max_nodes() sizes the LDS frame (an upper bound of the largest graph).  *status (one zeroed
 * device word) collects: bit 0 an index outside its table (a member that is not a node of its graph, an unsorted member
 * list, an edge position or endpoint out of range, an edge whose endpoints lie in two graphs, out_cols < ka), bit 1 a NaN
 * or infinite entry of a factorised graph's clamped adjacency, bit 2 a graph of more than max_n nodes or K >
 * tgp_nmf_max_k().  A flagged graph is left unwritten; nothing out of range is dereferenced.
 * TGP_ERR_INVALID: a NULL input or output, sizes below zero, K < 1, out_cols < 1, max_iter < 1, tol < 0 or NaN, max_n
 * outside its range, one of w0 / h0t without the other; TGP_ERR_RANGE: a size beyond the int32 index.  All are found
 * before any HIP call.
 * ---------------------------------------------------------------------------------- */
int tgp_nmf_max_nodes(void);
int tgp_nmf_max_k(void);
int tgp_nmf_init_f32(const int32_t* grp_ptr, const int32_t* grp_perm /* NULL ok */, const int64_t* dst,
                     const float* edge_weight /* NULL ok */, const int32_t* gid, const int32_t* graph_ptr,
                     const int32_t* graph_perm, int64_t N, int64_t E, int64_t G, int64_t K, int64_t max_n, int64_t seed,
                     float* w0, float* h0t, int32_t* status, void* stream);
int tgp_nmf_factorize_f32(const int32_t* grp_ptr, const int32_t* grp_perm /* NULL ok */, const int64_t* dst,
                          const float* edge_weight /* NULL ok */, const int32_t* gid, const int32_t* graph_ptr,
                          const int32_t* graph_perm, int64_t N, int64_t E, int64_t G, int64_t K, int64_t out_cols,
                          int64_t max_n, int64_t seed, float tol, int64_t max_iter, const float* w0 /* NULL ok */,
                          const float* h0t /* NULL ok */, float* s, float* w_out /* NULL ok */,
                          float* ht_out /* NULL ok */, int32_t* iters /* NULL ok */, float* violation_ratio /* NULL ok */,
                          int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------
 * PAN convolution and pooling (reference poolers/pan.py over PyG's PANConv), csrc/pan.hip: the MET matrix
 *     M = D^-1/2 (sum_{n=0..L} c_n A_t^n) D^-1/2,  A_t[dst, src] = multiplicity of the edge src -> dst,
 *     tmp_0 = w_0 I, tmp_n = w_n (tmp_{n-1} A_t), S = sum_n tmp_n (c_n = w_0 ... w_n),
 *     deg_i = stored entries of row i (a count), dinv = deg^-1/2, M_ij = (dinv_j S_ij) dinv_i.
 * The pattern is structural: (i, j) is stored iff a walk of length <= L joins them, whatever the value; the diagonal is
 * always stored.  One wave owns a row and keeps it in LDS over the n nodes of the row's graph; the graphs are the node
 * ranges graph_ptr [G + 1] (nodes grouped by graph), gid [N] names every node's graph (NULL: one graph), the edges come
 * through the by-source edge index (grp_ptr [N + 1], grp_perm [E] or NULL for a list that is grouped already) and are
 * added in edge-list order: fp32, no fused multiply-add, no float atomics, the same bits on every call.
 *   count: row_ptr [N + 1] int32 (the CSR offsets of M, row_ptr[N] = nnz), dinv [N], *d_count = nnz -- or -1 when the
 *          status word is set (the fill must not run then).  Row i checks every edge that starts at node i, so the
 *          status word of the count covers every edge of the list.  ws: tgp_pan_met_workspace_bytes(N).
 *   fill:  (out_row, out_col, out_val) [nnz] row-major sorted, ascending columns inside a row: coalesced, no sort.
 *   bwd:   part [N, L + 1], part[i, n] = sum over row i's stored entries e of (g_val[e] dinv[col[e]]) dinv[i]
 *          (A_t^n)[i, col[e]]; the column sums over i are the gradient with respect to c.
 * max_n in 1 .. tgp_pan_max_graph_nodes() sizes the LDS frame (an upper bound of the largest graph).  *status (one zeroed
 * device word) collects: bit 0 an index outside its table (a node outside its graph's range, an edge position or endpoint
 * out of range, offsets that are not those of this pattern), bit 1 an edge whose endpoints lie in two graphs, bit 2 a graph
 * of more than max_n nodes.  A flagged row is left unwritten; nothing out of range is dereferenced.
 *   score: score[i] = act(beta[0] <x[i,:], p> + beta[1] sum_{e in column group i} val[e]), act 0 = identity, 1 = tanh;
 *          col_ptr [N + 1] / col_perm [nnz] (NULL: grouped already) index M's entries by column.  dot_out, colsum_out
 *          [N] (NULL ok) receive the two terms.
 * TGP_ERR_INVALID: a NULL input or output, sizes below zero, L outside 0 .. 64, max_n outside its range, an empty count;
 * TGP_ERR_RANGE: a size (or N x max_n) beyond the int32 index; TGP_ERR_WORKSPACE: ws too small.  All are found before
 * any HIP call.
 * ---------------------------------------------------------------------------------- */
int tgp_pan_max_graph_nodes(void);
size_t tgp_pan_met_workspace_bytes(int64_t N);
int tgp_pan_met_count(const int32_t* grp_ptr, const int32_t* grp_perm /* NULL ok */, const int64_t* dst,
                      const int32_t* gid /* NULL ok */, const int32_t* graph_ptr, int64_t N, int64_t E, int64_t G,
                      int64_t L, int64_t max_n, int32_t* row_ptr, float* dinv, void* ws, size_t ws_bytes,
                      int32_t* status, int64_t* d_count, void* stream);
int tgp_pan_met_fill_f32(const int32_t* grp_ptr, const int32_t* grp_perm /* NULL ok */, const int64_t* dst,
                         const int32_t* gid /* NULL ok */, const int32_t* graph_ptr, int64_t N, int64_t E, int64_t G,
                         int64_t L, int64_t max_n, const float* weight, const int32_t* row_ptr, const float* dinv,
                         int64_t nnz, int64_t* out_row, int64_t* out_col, float* out_val, int32_t* status,
                         void* stream);
int tgp_pan_met_bwd_f32(const int32_t* grp_ptr, const int32_t* grp_perm /* NULL ok */, const int64_t* dst,
                        const int32_t* gid /* NULL ok */, const int32_t* graph_ptr, int64_t N, int64_t E, int64_t G,
                        int64_t L, int64_t max_n, const int32_t* row_ptr, const int64_t* col, const float* g_val,
                        const float* dinv, int64_t nnz, float* part, int32_t* status, void* stream);
int tgp_pan_score_f32(const float* x, int64_t N, int64_t F, int64_t ldx, const float* p, const float* beta,
                      const int32_t* col_ptr, const int32_t* col_perm /* NULL ok */, const float* val, int64_t nnz,
                      int act, float* score, float* dot_out /* NULL ok */, float* colsum_out /* NULL ok */,
                      void* stream);

/* ------------------------------------------------------------------------------------
 * GTVConv's propagation (reference mp/gtvconv.py), csrc/gtvconv.hip.  With h = x W [N, C] already projected:
 *     out_i = act((h_i + delta sum_{e: row(e) = i, col(e) != i} gamma_e (h_col(e) - h_i) + bias) [* mask_i]),
 *     d_e = ||h_row(e) - h_col(e)||_1,  gamma_e = w_e / max(d_e, eps)  (w NULL: 1).
 * A group of 8, 16, 32 or 64 lanes owns a node and keeps h_i in registers; every h_col is loaded once per edge (twice
 * beyond 512 channels) and nothing of size E x C is formed.  Sums over a node's edges run in the order of the by-source
 * index (src_ptr [N + 1], src_perm [E] or NULL for a list that is grouped already) and, in the node gradient, of the
 * by-destination index (dst_ptr, dst_perm) after it: edge-list order inside a node, no float atomics, the same bits on
 * every call.  A self-loop, an edge with an endpoint outside [0, N) and an index position outside [0, E) are skipped and
 * never dereferenced; their d, gw and t entries are left as the caller initialised them (zeros).
 *   fwd:       act_code 0 identity, 1 relu, 2 elu (alpha 1); mask [N] bytes (NULL ok, 0 = the row becomes act(0));
 *              d [E] (NULL ok up to 512 channels) receives the distances a backward needs.
 *   bwd_terms: g [N, C] = g_out act'(out) mask; per edge s_e = delta <g_i, h_col - h_i>, gw_e = s_e / max(d_e, eps)
 *              (gw NULL ok: the gradient of w), t_e = -s_e gamma_e / d_e where d_e >= eps, else 0.
 *   bwd_nodes: dh_i = g_i (1 - delta sum_out gamma_e) + sum_out t_e sign(h_i - h_col)
 *                   + sum_in (delta gamma_e g_row - t_e sign(h_row - h_i)),  sign(0) = 0.
 * Vector loads are used when C % 4 == 0 and every row buffer is 16-byte aligned.  nodes == 0 returns TGP_OK.
 * TGP_ERR_INVALID: a NULL input or output, sizes below zero, C < 1, an unknown act_code; TGP_ERR_RANGE: nodes or E >= 2^31
 * or C >= 32768.  All are found before any HIP call.
 * ---------------------------------------------------------------------------------- */
int tgp_gtv_edge_fwd_f32(const float* h, int64_t nodes, int64_t C, const int32_t* src_ptr,
                         const int32_t* src_perm /* NULL ok */, const int64_t* col, const float* w /* NULL ok */,
                         int64_t E, const float* bias /* NULL ok */, const uint8_t* mask /* NULL ok */, float delta,
                         float eps, int act_code, float* out, float* d /* NULL ok */, void* stream);
int tgp_gtv_edge_bwd_terms_f32(const float* h, const float* out, const float* g_out, int64_t nodes, int64_t C,
                               const int32_t* src_ptr, const int32_t* src_perm /* NULL ok */, const int64_t* col,
                               const float* w /* NULL ok */, int64_t E, const float* d, const uint8_t* mask /* NULL ok */,
                               float delta, float eps, int act_code, float* g, float* gw /* NULL ok */, float* t,
                               void* stream);
int tgp_gtv_edge_bwd_nodes_f32(const float* h, const float* g, int64_t nodes, int64_t C, const int32_t* src_ptr,
                               const int32_t* src_perm /* NULL ok */, const int32_t* dst_ptr,
                               const int32_t* dst_perm /* NULL ok */, const int64_t* row, const int64_t* col,
                               const float* w /* NULL ok */, int64_t E, const float* d, const float* t, float delta,
                               float eps, float* dh, void* stream);

/* ----------------------------------------------------------------------------------
 * SEP pooling's selector (Wu et al., ICML 2022; reference select/sep_select.py with levels = 1; DESIGN 4.26;
 * csrc/sep_select.hip): per graph a structural-entropy coding tree grown by greedy merging and compressed to height 2;
 * every node is labelled with its depth-1 cluster.  One workgroup per graph, all graphs in one launch, then two small
 * launches: the exclusive prefix of the per-graph counts and its addition to the labels.
 *   src_ptr / src_perm, dst_ptr / dst_perm: the edge positions grouped by source and by destination, edge-list order
 *   inside a node (perm NULL: the list is grouped already); src, dst [E] the two edge rows; edge_weight [E] or NULL (1).
 *   gid [N] the graph of every node; graph_ptr [G + 1]: graph g owns the nodes graph_ptr[g] .. graph_ptr[g + 1] - 1 (a
 *   sorted batch vector).  max_n in 1 .. tgp_sep_max_nodes() sizes the LDS frame (an upper bound of the largest graph
 *   the kernel is to take); tgp_sep_max_nodes() is what fits the 160 KiB of a CU.
 * Outputs: cluster_index [N] int64 (ids offset by the exclusive prefix of the counts, in graph order), counts [G],
 * offsets [G], words [2] = {status, number of supernodes}; counts and words are zeroed by the call.  Status bits:
 * 1 = an index outside its table (an edge position, endpoint or CSR offset out of range, a node whose gid is not its
 * graph, an edge between two graphs), 2 = a non-finite or negative weight after duplicates are summed, 4 = a graph of
 * more than max_n nodes.  A flagged graph is left unwritten (its count stays 0 and its cluster_index entries are not
 * touched); nothing out of range is dereferenced.  Self-loops are dropped.  The same input gives the same bits, wherever
 * the graph stands in the batch.  G == 0 or N == 0 returns TGP_OK.
 * TGP_ERR_INVALID: a NULL pointer, a negative size, max_n outside its range; TGP_ERR_RANGE: N, E or G >= 2^31.  All are
 * found before any HIP call.
 * ---------------------------------------------------------------------------------- */
int tgp_sep_max_nodes(void);
int tgp_sep_select_f32(const int32_t* src_ptr, const int32_t* src_perm /* NULL ok */, const int32_t* dst_ptr,
                       const int32_t* dst_perm /* NULL ok */, const int64_t* src, const int64_t* dst,
                       const float* edge_weight /* NULL ok */, const int32_t* gid, const int32_t* graph_ptr, int64_t N,
                       int64_t E, int64_t G, int64_t max_n, int64_t* cluster_index, int32_t* counts, int32_t* offsets,
                       int32_t* words, void* stream);

/* ------------------------------------------------------------------------------------
 * The dense poolers' gradient with respect to a dense adjacency that was handed in (DiffPool, MinCut; padded batch,
 * float32; what the reference gets from ATen autograd over connect/dense_conn.py:111-122, utils/losses.py:39-56 and
 * :644-652).  Per graph b, with R = S^T A S and M = the total gradient of R (post-processing backward + upstream + the
 * loss' diagonal term: -(g_cut / (den + eps)) I for MinCut, -c I for DiffPool):
 *     dA_b = S_b M_b S_b^T + gamma_b q_b 1^T + c A_b,      q_i = |s_i|^2,
 *     gamma_b = g_cut trace(R_b) / (den_b + eps)^2   (MinCut: the gradient of den_b = sum_i (A 1)_i q_i),
 *     c = link_scale^2 *g_link / *link_loss          (DiffPool: ONE scalar for the batch; 0 when the loss is 0).
 * dA [B,N,N] is written once, one writer per element, no atomics: the same bits on every call.  Every coefficient is a
 * device value; nothing is read back.
 *
 * tgp_dense_pool_adj_grad_f32 (graphs beyond the one-wave kernels; any N, K): M [B][K][K] with row stride ldm and batch
 *   stride sM (the RV block of tgp_dense_pool_train_rhs_f32's rcat), S with row stride lds and batch stride sS, gamma
 *   [B] or NULL (the c1 of that call), q [B,N] or NULL (formed from S then), g_link / link_loss 0-dim or NULL (A is
 *   read only then).  T [B,N,K] is scratch for S M (tgp_bmm_f32); the N^2 K product T S^T runs on the fp32 matrix cores
 *   and its epilogue adds the other two terms while the tile is in registers.  Two launches.
 * tgp_dense_pool_adj_grad_small_f32 (N <= 64, K <= 32: the batches tgp_dense_pool_is_small accepts), one wave per graph,
 *   one launch behind tgp_dense_pool_small_bwd_f32: M = ga + g_raw - (g_b / (den_b + loss_eps) + c) I is formed here from
 *   ga (tgp_postprocess_dense_bwd_f32's output) and g_raw (each [B,K,K] or NULL), g_b = g_terms[0,b] + *g_mean_cut / B
 *   (each optional; raw [B,K,K] = the forward's S^T A S and A are needed with either), den_b from one pass over A.
 * TGP_ERR_INVALID: a NULL required operand, sizes below zero, K < 1, a row stride below K, dA given as an operand, a
 * coefficient without what it is formed from, (small) N > 64 or K > 32; TGP_ERR_RANGE: N, K or the grid beyond the int32
 * internals.  All are found before any HIP call; B == 0 or N == 0 returns TGP_OK.
 * ---------------------------------------------------------------------------------- */
int tgp_dense_pool_adj_grad_f32(const float* S, int64_t lds, int64_t sS, const float* A, const float* M, int64_t ldm,
                                int64_t sM, const float* gamma, const float* q, const float* g_link,
                                const float* link_loss, float link_scale, int64_t B, int64_t N, int64_t K, float* T,
                                float* dA, void* stream);
int tgp_dense_pool_adj_grad_small_f32(const float* S, const float* A, const float* ga, const float* g_raw,
                                      const float* raw, const float* g_terms, const float* g_mean_cut,
                                      const float* g_link, const float* link_loss, float link_scale, float loss_eps,
                                      int64_t B, int64_t N, int64_t K, float* dA, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TGP_HIP_H */
