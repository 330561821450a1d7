// PAN convolution and pooling (Ma et al., NeurIPS 2020; reference poolers/pan.py over PyG's PANConv): the
// maximal-entropy-transition matrix
//   M = D^-1/2 (sum_{n=0..L} c_n A_t^n) D^-1/2,   A_t[dst, src] = multiplicity of the edge src -> dst,
//   tmp_0 = w_0 I,  tmp_n = w_n (tmp_{n-1} A_t)   (so c_n = w_0 ... w_n),   S = sum_n tmp_n,
//   deg_i = stored entries of row i of S (a count),  M_ij = (dinv_j S_ij) dinv_i,
// and PAN pooling's score act(beta_0 <x_i, p> + beta_1 sum_{e: col(e) = i} M_e).
//
// Row i of tmp A_t depends on row i of tmp only, and its nonzeros lie within L hops of node i inside node i's graph.  So
// one wave owns one row of M and keeps it in LDS as a dense vector over the graph's n nodes: no sparse-sparse product, no
// concatenated list of L + 1 partial matrices and no sort.
//   step:     next[j] = w_n * sum_{edges j -> k} cur[k], the edges of j in edge-list order through the by-source edge
//             index; the wave's lanes own the columns j = lane, lane + 64, ...
//   pattern:  structural.  reach_0 = {i}, reach_{n+1} = reach_n + {j : some edge j -> k has k in reach_n}: a byte mask in
//             LDS, independent of the values (a zero or cancelling weight keeps the entry).  The float walk skips the
//             columns outside the final mask: they stay zero.
//   count:    deg_i = |reach_L|, dinv_i = 1 / sqrt(deg_i); an exclusive scan of deg gives every row's offset in M.
//             Row i also checks every edge that starts at node i (the reach walk skips and leaves early, so it does
//             not see every edge): the count's verdict covers the whole edge list.
//   fill:     the mask again, the float walk, then the row's entries (i, j, (dinv_j S_ij) dinv_i) in ascending j at the
//             row's offset: M comes out coalesced and row-major sorted.
//   backward: the unweighted row powers P_n = e_i A_t^n walked the same way; per row the L + 1 numbers
//             sum_e G_e dinv_i dinv_col(e) P_n[col(e)] over the row's stored entries.
// fp32 throughout, no fused multiply-add (-ffp-contract=off), no float atomics: the same bits on every call.
// An index outside its table, an edge that leaves its graph and a graph beyond the LDS frame set a bit of the status
// word; nothing out of range is dereferenced.
#include "primitives.h"

namespace tgp {
namespace {

// Per wave: three float rows (cur, next, sum) and the byte mask = 13 bytes per node.  1024 nodes are 13 KB per wave, 52 KB
// per 4-wave workgroup: three workgroups = 12 waves on a CU's 160 KB.
constexpr int PAN_MAX_NODES = 1024;
constexpr int PAN_WAVES = 4;
constexpr int PAN_MAX_FILTER = 64;  // (a power series that long has no use; the bound keeps L + 1 an int)

constexpr int PAN_BAD_INPUT = 1;    // an index outside its table
constexpr int PAN_CROSS_GRAPH = 2;  // an edge whose endpoints lie in two graphs
constexpr int PAN_OVER_LIMIT = 4;   // a graph of more than max_n nodes

constexpr int64_t I32_MAX = 2147483647;

struct PanGraph {
  const int32_t* grp_ptr;    // [N + 1] by-source offsets
  const int32_t* grp_perm;   // [E] edge positions by source (NULL: the list is grouped already)
  const int64_t* dst;        // [E]
  const int32_t* gid;        // [N] graph of every node (NULL: one graph)
  const int32_t* graph_ptr;  // [G + 1] node offsets of the graphs (nodes grouped by graph)
  int N, E, G, L, max_n;
  int32_t* status;
};

// what one wave needs of the LDS frame
__host__ __device__ inline size_t pan_wave_bytes(int max_n, bool floats) {
  const size_t mask = (static_cast<size_t>(max_n) + 15) / 16 * 16;
  return mask + (floats ? 3 * sizeof(float) * static_cast<size_t>(max_n) : 0);
}

// writes and reads of LDS by different lanes of ONE wave: order them (the compiler must not move them across, and the
// wave's LDS instructions complete in issue order)
__device__ __forceinline__ void pan_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the graph of row i: its first node and size (wave-uniform); false and a status bit when it cannot be walked
__device__ __forceinline__ bool pan_frame(const PanGraph& p, int i, int& base, int& n, int& bad) {
  const int g = p.gid ? p.gid[i] : 0;
  if (g < 0 || g >= p.G) {
    bad |= PAN_BAD_INPUT;
    return false;
  }
  const int t0 = p.graph_ptr[g], t1 = p.graph_ptr[g + 1];
  if (t0 < 0 || t1 > p.N || i < t0 || i >= t1) {
    bad |= PAN_BAD_INPUT;
    return false;
  }
  if (t1 - t0 > p.max_n) {
    bad |= PAN_OVER_LIMIT;
    return false;
  }
  base = t0;
  n = t1 - t0;
  return true;
}

// the by-source edge range of node v, clamped into the list
__device__ __forceinline__ void pan_edge_range(const PanGraph& p, int v, int& e0, int& e1, int& bad) {
  e0 = p.grp_ptr[v];
  e1 = p.grp_ptr[v + 1];
  if (e0 < 0 || e1 < e0 || e1 > p.E) {
    bad |= PAN_BAD_INPUT;
    e0 = e1 = 0;
  }
}

// the local index of the far end of position e of the index, or -1 (a status bit says why)
__device__ __forceinline__ int pan_far_end(const PanGraph& p, int e, int base, int n, int& bad) {
  const int pos = p.grp_perm ? p.grp_perm[e] : e;
  if (static_cast<unsigned>(pos) >= static_cast<unsigned>(p.E)) {
    bad |= PAN_BAD_INPUT;
    return -1;
  }
  const int64_t k = p.dst[pos];
  if (k < 0 || k >= p.N) {
    bad |= PAN_BAD_INPUT;
    return -1;
  }
  if (k < base || k >= static_cast<int64_t>(base) + n) {
    bad |= PAN_CROSS_GRAPH;
    return -1;
  }
  return static_cast<int>(k - base);
}

// mask [n] = the nodes within L hops of `self` against the edge direction; returns how many (the same in every lane)
__device__ __forceinline__ int pan_reach(const PanGraph& p, unsigned char* mask, int base, int n, int self, int lane,
                                         int& bad) {
  for (int j = lane; j < n; j += 64) mask[j] = j == self ? 1 : 0;
  pan_wave_sync();
  int count = 1;
  for (int step = 0; step < p.L; ++step) {
    uint32_t fresh = 0;  // bit t: column lane + 64 t joins (n <= 1024: 16 bits)
    int t = 0;
    for (int j = lane; j < n; j += 64, ++t) {
      if (mask[j]) continue;
      int e0, e1;
      pan_edge_range(p, base + j, e0, e1, bad);
      for (int e = e0; e < e1; ++e) {
        const int k = pan_far_end(p, e, base, n, bad);
        if (k >= 0 && mask[k]) {
          fresh |= 1u << t;
          break;
        }
      }
    }
    pan_wave_sync();  // every lane has read the old mask
    t = 0;
    for (int j = lane; j < n; j += 64, ++t)
      if ((fresh >> t) & 1u) mask[j] = 1;
    pan_wave_sync();
    const int added = wave_sum(static_cast<int>(__popc(fresh)));
    if (added == 0) break;  // (wave-uniform) nothing new: the later steps add nothing either
    count += added;
  }
  return count;
}

// one step of the row: nxt[j] = scale * sum_{edges j -> k} cur[k] on the columns of the mask, 0 elsewhere
__device__ __forceinline__ void pan_step(const PanGraph& p, const unsigned char* mask, const float* cur, float* nxt,
                                         float scale, bool scaled, int base, int n, int lane, int& bad) {
  for (int j = lane; j < n; j += 64) {
    float acc = 0.0f;
    if (mask[j]) {
      int e0, e1;
      pan_edge_range(p, base + j, e0, e1, bad);
      for (int e = e0; e < e1; ++e) {
        const int k = pan_far_end(p, e, base, n, bad);
        if (k >= 0) acc += cur[k];
      }
      if (scaled) acc = scale * acc;
    }
    nxt[j] = acc;
  }
  pan_wave_sync();
}

__device__ __forceinline__ void pan_flag(int32_t* status, int bad, int lane) {
  bad = wave_or(bad);
  if (bad && lane == 0) atomicOr(status, bad);
}

// deg [N + 1] (the last word 0: the scan's total lands behind the last row) and dinv [N]
__global__ __launch_bounds__(PAN_WAVES * 64) void pan_count_kernel(PanGraph p, uint32_t* __restrict__ deg,
                                                                   float* __restrict__ dinv) {
  extern __shared__ float pan_smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned char* const mask = reinterpret_cast<unsigned char*>(pan_smem) + wave * pan_wave_bytes(p.max_n, false);
  const int64_t i64 = static_cast<int64_t>(blockIdx.x) * PAN_WAVES + wave;
  if (i64 == p.N && lane == 0) deg[p.N] = 0u;
  if (i64 >= p.N) return;
  const int i = static_cast<int>(i64);
  int bad = 0, base = 0, n = 0, count = 0;
  if (pan_frame(p, i, base, n, bad)) {
    // The reach walk skips masked columns and leaves a column at its first hit, so it does not see every edge.  The
    // verdict on the input must not depend on that: row i checks every edge that STARTS at node i, whatever the walk
    // does.  Every edge starts at exactly one node, so the count flags every edge that leaves its graph or its table.
    int e0, e1;
    pan_edge_range(p, i, e0, e1, bad);
    for (int e = e0 + lane; e < e1; e += 64) (void)pan_far_end(p, e, base, n, bad);
    count = pan_reach(p, mask, base, n, i - base, lane, bad);
  }
  if (lane == 0) {
    deg[i] = static_cast<uint32_t>(count);
    dinv[i] = count > 0 ? 1.0f / sqrtf(static_cast<float>(count)) : 0.0f;
  }
  pan_flag(p.status, bad, lane);
}

// *d_count = the scan's total, or -1 when the count kernel flagged anything (the fill must not run then)
__global__ void pan_finish_count_kernel(const int32_t* __restrict__ status, const int64_t* __restrict__ total,
                                        int64_t* __restrict__ d_count) {
  *d_count = *status ? static_cast<int64_t>(-1) : *total;
}

__global__ __launch_bounds__(PAN_WAVES * 64) void pan_fill_kernel(PanGraph p, const float* __restrict__ weight,
                                                                  const int32_t* __restrict__ row_ptr,
                                                                  const float* __restrict__ dinv, int64_t nnz,
                                                                  int64_t* __restrict__ out_row,
                                                                  int64_t* __restrict__ out_col,
                                                                  float* __restrict__ out_val) {
  extern __shared__ float pan_smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  char* const frame = reinterpret_cast<char*>(pan_smem) + wave * pan_wave_bytes(p.max_n, true);
  float* cur = reinterpret_cast<float*>(frame);
  float* nxt = cur + p.max_n;
  float* const sum = nxt + p.max_n;
  unsigned char* const mask = reinterpret_cast<unsigned char*>(sum + p.max_n);
  const int64_t i64 = static_cast<int64_t>(blockIdx.x) * PAN_WAVES + wave;
  if (i64 >= p.N) return;
  const int i = static_cast<int>(i64);
  int bad = 0, base = 0, n = 0;
  if (!pan_frame(p, i, base, n, bad)) {
    pan_flag(p.status, bad, lane);
    return;
  }
  const int self = i - base;
  const int count = pan_reach(p, mask, base, n, self, lane, bad);
  const int64_t off = row_ptr[i], end = row_ptr[i + 1];
  if (off < 0 || end - off != count || end > nnz) {  // the offsets are not those of this pattern: write nothing
    pan_flag(p.status, bad | PAN_BAD_INPUT, lane);
    return;
  }
  const float w0 = weight[0];
  for (int j = lane; j < n; j += 64) {
    const float v = j == self ? w0 : 0.0f;
    cur[j] = v;
    sum[j] = v;
  }
  pan_wave_sync();
  for (int step = 1; step <= p.L; ++step) {
    pan_step(p, mask, cur, nxt, weight[step], true, base, n, lane, bad);
    for (int j = lane; j < n; j += 64) sum[j] += nxt[j];  // (a lane's own columns)
    float* const t = cur;
    cur = nxt;
    nxt = t;
  }
  const float di = dinv[i];
  int64_t at = off;
  for (int j0 = 0; j0 < n; j0 += 64) {  // ascending columns: a ballot ranks the stored ones of every 64
    const int j = j0 + lane;
    const bool keep = j < n && mask[j];
    const unsigned long long m = __ballot(keep);
    if (keep) {
      const int64_t e = at + __popcll(m & lanemask_lt());
      out_row[e] = i;
      out_col[e] = base + j;
      out_val[e] = (dinv[base + j] * sum[j]) * di;
    }
    at += __popcll(m);
  }
  pan_flag(p.status, bad, lane);
}

// part [N, L + 1]: part[i, n] = sum over row i's stored entries e of (g_e dinv_col(e)) dinv_i P_n[col(e)]
__global__ __launch_bounds__(PAN_WAVES * 64) void pan_bwd_kernel(PanGraph p, const int32_t* __restrict__ row_ptr,
                                                                 const int64_t* __restrict__ col,
                                                                 const float* __restrict__ g_val,
                                                                 const float* __restrict__ dinv, int64_t nnz,
                                                                 float* __restrict__ part) {
  extern __shared__ float pan_smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  char* const frame = reinterpret_cast<char*>(pan_smem) + wave * pan_wave_bytes(p.max_n, true);
  float* cur = reinterpret_cast<float*>(frame);
  float* nxt = cur + p.max_n;
  unsigned char* const mask = reinterpret_cast<unsigned char*>(nxt + 2 * p.max_n);
  const int64_t i64 = static_cast<int64_t>(blockIdx.x) * PAN_WAVES + wave;
  if (i64 >= p.N) return;
  const int i = static_cast<int>(i64);
  int bad = 0, base = 0, n = 0;
  float* const out = part + i64 * (p.L + 1);
  if (!pan_frame(p, i, base, n, bad)) {
    pan_flag(p.status, bad, lane);
    return;
  }
  int64_t off = row_ptr[i], end = row_ptr[i + 1];
  if (off < 0 || end < off || end > nnz) {
    bad |= PAN_BAD_INPUT;
    off = end = 0;
  }
  // the row's pattern as M stores it: only these columns are read below, so only they are walked
  for (int j = lane; j < n; j += 64) {
    mask[j] = 0;
    cur[j] = j == i - base ? 1.0f : 0.0f;
  }
  pan_wave_sync();
  for (int64_t e = off + lane; e < end; e += 64) {
    const int64_t c = col[e];
    if (c < base || c >= static_cast<int64_t>(base) + n) bad |= PAN_BAD_INPUT;
    else mask[c - base] = 1;
  }
  pan_wave_sync();
  const float di = dinv[i];
  for (int step = 0; step <= p.L; ++step) {
    if (step > 0) {
      pan_step(p, mask, cur, nxt, 1.0f, false, base, n, lane, bad);
      float* const t = cur;
      cur = nxt;
      nxt = t;
    }
    float acc = 0.0f;
    for (int64_t e = off + lane; e < end; e += 64) {
      const int64_t c = col[e];
      if (c >= base && c < static_cast<int64_t>(base) + n) acc += ((g_val[e] * dinv[c]) * di) * cur[c - base];
    }
    acc = wave_sum(acc);
    if (lane == 0) out[step] = acc;
  }
  pan_flag(p.status, bad, lane);
}

// 16 lanes per node: <x_i, p> over the columns and the sum of M's values over node i's column group (the group's order,
// strided by lane, then the xor butterfly: a fixed order)
__global__ __launch_bounds__(256) void pan_score_kernel(const float* __restrict__ x, int64_t n, int F, int64_t ldx,
                                                        const float* __restrict__ pvec, const float* __restrict__ beta,
                                                        const int32_t* __restrict__ col_ptr,
                                                        const int32_t* __restrict__ col_perm,
                                                        const float* __restrict__ val, int64_t nnz, int act,
                                                        float* __restrict__ score, float* __restrict__ dot_out,
                                                        float* __restrict__ colsum_out) {
  constexpr int G = 16;
  const int sub = threadIdx.x % G;
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) / G;
  float d = 0.0f, c = 0.0f;
  if (i < n) {
    const float* const a = x + i * ldx;
    for (int k = sub; k < F; k += G) d += a[k] * pvec[k];
    int64_t e0 = col_ptr[i], e1 = col_ptr[i + 1];
    if (e0 < 0) e0 = 0;
    if (e1 > nnz) e1 = nnz;
    for (int64_t e = e0 + sub; e < e1; e += G) {
      const int64_t pos = col_perm ? static_cast<int64_t>(col_perm[e]) : e;
      if (static_cast<uint64_t>(pos) < static_cast<uint64_t>(nnz)) c += val[pos];
    }
  }
  d = wave_sum<G>(d);
  c = wave_sum<G>(c);
  if (i < n && sub == 0) {
    const float t = beta[0] * d + beta[1] * c;
    score[i] = act ? tanhf(t) : t;
    if (dot_out) dot_out[i] = d;
    if (colsum_out) colsum_out[i] = c;
  }
}

int pan_check_graph(const char* what, const int32_t* grp_ptr, const int64_t* dst, const int32_t* gid,
                    const int32_t* graph_ptr, int64_t N, int64_t E, int64_t G, int64_t L, int64_t max_n,
                    const int32_t* status) {
  TGP_REQUIRE(N >= 0 && E >= 0 && G >= 0, TGP_ERR_INVALID, "%s: negative size", what);
  TGP_REQUIRE(L >= 0 && L <= PAN_MAX_FILTER, TGP_ERR_INVALID, "%s: filter_size = %lld outside 0 .. %d", what,
              static_cast<long long>(L), PAN_MAX_FILTER);
  TGP_REQUIRE(max_n >= 1 && max_n <= PAN_MAX_NODES, TGP_ERR_INVALID, "%s: max_n = %lld outside 1 .. %d", what,
              static_cast<long long>(max_n), PAN_MAX_NODES);
  TGP_REQUIRE(grp_ptr && graph_ptr && status, TGP_ERR_INVALID, "%s: NULL pointer", what);
  TGP_REQUIRE(gid || G <= 1, TGP_ERR_INVALID, "%s: NULL gid with more than one graph", what);
  TGP_REQUIRE(E == 0 || dst, TGP_ERR_INVALID, "%s: NULL dst with E > 0", what);
  TGP_REQUIRE(N <= I32_MAX && E <= I32_MAX && G <= I32_MAX && N * max_n <= I32_MAX, TGP_ERR_RANGE,
              "%s: N, E, G or N x max_n beyond the int32 index", what);
  return TGP_OK;
}

}  // namespace
}  // namespace tgp

using namespace tgp;

extern "C" int tgp_pan_max_graph_nodes(void) { return PAN_MAX_NODES; }

extern "C" size_t tgp_pan_met_workspace_bytes(int64_t N) {
  if (N < 0) N = 0;
  const size_t nt = static_cast<size_t>(cdiv(N + 1, SCAN_TILE));
  return align_up(sizeof(uint32_t) * static_cast<size_t>(N + 1)) + align_up(sizeof(uint32_t) * 2 * nt) +
         align_up(sizeof(int64_t));
}

extern "C" int tgp_pan_met_count(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* dst,
                                 const int32_t* gid, const int32_t* graph_ptr, int64_t N, int64_t E, int64_t G,
                                 int64_t L, int64_t max_n, int32_t* row_ptr, float* dinv, void* ws, size_t ws_bytes,
                                 int32_t* status, int64_t* d_count, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int rc = pan_check_graph("tgp_pan_met_count", grp_ptr, dst, gid, graph_ptr, N, E, G, L, max_n, status);
  if (rc != TGP_OK) return rc;
  TGP_REQUIRE(N >= 1 && G >= 1, TGP_ERR_INVALID, "tgp_pan_met_count: no node or no graph");
  TGP_REQUIRE(row_ptr && dinv && ws && d_count, TGP_ERR_INVALID, "tgp_pan_met_count: NULL pointer");
  TGP_REQUIRE(ws_bytes >= tgp_pan_met_workspace_bytes(N), TGP_ERR_WORKSPACE,
              "tgp_pan_met_count: workspace too small (%zu < %zu)", ws_bytes, tgp_pan_met_workspace_bytes(N));
  Carver c(ws);
  uint32_t* deg = c.take<uint32_t>(static_cast<size_t>(N + 1));
  uint32_t* tiles = c.take<uint32_t>(2 * static_cast<size_t>(cdiv(N + 1, SCAN_TILE)));
  int64_t* total = c.take<int64_t>(1);
  PanGraph p{grp_ptr, grp_perm, dst, gid, graph_ptr, static_cast<int>(N), static_cast<int>(E), static_cast<int>(G),
             static_cast<int>(L), static_cast<int>(max_n), status};
  const size_t lds = PAN_WAVES * pan_wave_bytes(p.max_n, false);
  hipLaunchKernelGGL(pan_count_kernel, dim3(static_cast<unsigned>(cdiv(N + 1, PAN_WAVES))), dim3(PAN_WAVES * 64), lds,
                     stream, p, deg, dinv);
  // the offsets of the N rows and, behind them, the total: row_ptr [N + 1] (int32: N x max_n was checked)
  device_scan_u32(deg, N + 1, reinterpret_cast<uint32_t*>(row_ptr), total, tiles, stream);
  hipLaunchKernelGGL(pan_finish_count_kernel, dim3(1), dim3(1), 0, stream, status, total, d_count);
  return check_launch("tgp_pan_met_count");
}

extern "C" int tgp_pan_met_fill_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* dst,
                                    const int32_t* gid, const int32_t* graph_ptr, int64_t N, int64_t E, int64_t G,
                                    int64_t L, int64_t max_n, const float* weight, const int32_t* row_ptr,
                                    const float* dinv, int64_t nnz, int64_t* out_row, int64_t* out_col, float* out_val,
                                    int32_t* status, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int rc = pan_check_graph("tgp_pan_met_fill_f32", grp_ptr, dst, gid, graph_ptr, N, E, G, L, max_n, status);
  if (rc != TGP_OK) return rc;
  TGP_REQUIRE(nnz >= 0 && nnz <= I32_MAX, TGP_ERR_RANGE, "tgp_pan_met_fill_f32: nnz = %lld outside the int32 index",
              static_cast<long long>(nnz));
  if (N == 0 || nnz == 0) return TGP_OK;
  TGP_REQUIRE(weight && row_ptr && dinv && out_row && out_col && out_val, TGP_ERR_INVALID,
              "tgp_pan_met_fill_f32: NULL pointer");
  PanGraph p{grp_ptr, grp_perm, dst, gid, graph_ptr, static_cast<int>(N), static_cast<int>(E), static_cast<int>(G),
             static_cast<int>(L), static_cast<int>(max_n), status};
  const size_t lds = PAN_WAVES * pan_wave_bytes(p.max_n, true);
  hipLaunchKernelGGL(pan_fill_kernel, dim3(static_cast<unsigned>(cdiv(N, PAN_WAVES))), dim3(PAN_WAVES * 64), lds, stream,
                     p, weight, row_ptr, dinv, nnz, out_row, out_col, out_val);
  return check_launch("tgp_pan_met_fill_f32");
}

extern "C" int tgp_pan_met_bwd_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* dst,
                                   const int32_t* gid, const int32_t* graph_ptr, int64_t N, int64_t E, int64_t G,
                                   int64_t L, int64_t max_n, const int32_t* row_ptr, const int64_t* col,
                                   const float* g_val, const float* dinv, int64_t nnz, float* part, int32_t* status,
                                   void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int rc = pan_check_graph("tgp_pan_met_bwd_f32", grp_ptr, dst, gid, graph_ptr, N, E, G, L, max_n, status);
  if (rc != TGP_OK) return rc;
  TGP_REQUIRE(nnz >= 0 && nnz <= I32_MAX, TGP_ERR_RANGE, "tgp_pan_met_bwd_f32: nnz = %lld outside the int32 index",
              static_cast<long long>(nnz));
  if (N == 0) return TGP_OK;
  TGP_REQUIRE(row_ptr && dinv && part && (nnz == 0 || (col && g_val)), TGP_ERR_INVALID,
              "tgp_pan_met_bwd_f32: NULL pointer");
  PanGraph p{grp_ptr, grp_perm, dst, gid, graph_ptr, static_cast<int>(N), static_cast<int>(E), static_cast<int>(G),
             static_cast<int>(L), static_cast<int>(max_n), status};
  const size_t lds = PAN_WAVES * pan_wave_bytes(p.max_n, true);
  hipLaunchKernelGGL(pan_bwd_kernel, dim3(static_cast<unsigned>(cdiv(N, PAN_WAVES))), dim3(PAN_WAVES * 64), lds, stream,
                     p, row_ptr, col, g_val, dinv, nnz, part);
  return check_launch("tgp_pan_met_bwd_f32");
}

extern "C" int tgp_pan_score_f32(const float* x, int64_t N, int64_t F, int64_t ldx, const float* p, const float* beta,
                                 const int32_t* col_ptr, const int32_t* col_perm, const float* val, int64_t nnz,
                                 int act, float* score, float* dot_out, float* colsum_out, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(N >= 0 && F >= 0 && nnz >= 0 && ldx >= F, TGP_ERR_INVALID, "tgp_pan_score_f32: bad size");
  TGP_REQUIRE(act == 0 || act == 1, TGP_ERR_INVALID, "tgp_pan_score_f32: act must be 0 (identity) or 1 (tanh)");
  TGP_REQUIRE(N <= I32_MAX && F <= I32_MAX && nnz <= I32_MAX, TGP_ERR_RANGE,
              "tgp_pan_score_f32: N, F or nnz beyond the int32 index");
  if (N == 0) return TGP_OK;
  TGP_REQUIRE(beta && col_ptr && score && (F == 0 || (x && p)) && (nnz == 0 || val), TGP_ERR_INVALID,
              "tgp_pan_score_f32: NULL pointer");
  hipLaunchKernelGGL(pan_score_kernel, dim3(static_cast<unsigned>(cdiv(N * 16, 256))), dim3(256), 0, stream, x, N,
                     static_cast<int>(F), ldx, p, beta, col_ptr, col_perm, val, nnz, act, score, dot_out, colsum_out);
  return check_launch("tgp_pan_score_f32");
}
