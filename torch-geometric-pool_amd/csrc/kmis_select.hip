// k-MIS selection (Bacciu et al., AAAI 2023; reference select/kmis_select.py): a maximal k-independent set chosen
// greedily by node priority, and the assignment of every node to the MIS node whose priority reached it within k hops.
//
// A node's priority is ONE 64-bit key, (prio << 32) | node, smaller = earlier.  prio is either the rank a caller's
// permutation gives the node, or the bits of its (heuristic-updated) score mapped so that unsigned order is DESCENDING
// score order; the node index in the low word makes keys unique, breaks ties towards the lower index (what a stable
// descending argsort does) and names the owner in the cluster pass.  No sort runs anywhere.
//
// One round (reference kmis_select.py:76-116): every unmasked node offers its key, keys travel k hops along row -> col
// taking minima (each hop from the PREVIOUS hop's values: double-buffered), a node that sees its own key joins the MIS,
// the MIS flag travels k hops the same way and becomes the mask.  Min / max are order-independent, so integer atomics
// leave the result a pure function of the inputs.
//
// Two routes, same results bit for bit:
//  * kmis_graphs_kernel: one workgroup per graph of a sorted batch, everything in LDS, __syncthreads() between hops,
//    behind the frame of graph_frame.h: a list that is not grouped by graph, or has an edge between two graphs, is
//    declined (status word), never misread.
//  * device-wide rounds: one launch per hop, one lane per edge pushing with a 64-bit atomic min into the destination
//    (a hub of degree 100 000 is 100 000 independent lanes, not one long row), three rotating buffers so that a hop
//    reads X, writes Y and resets Z without a launch of its own.  "Some node is still unmasked" is a flag per round the
//    host reads every few rounds.  No grid-wide barrier, no persistent kernel.
#include "graph_frame.h"

namespace tgp {

// ------------------------------------------------------------------------------------------------ per-graph route
struct KmGraphArgs {
  const int64_t* row;
  const int64_t* col;
  int64_t E, N;
  const int64_t* gptr;
  int k, mode;  // mode 0: rank given; 1: score is the updated score; 2: "greedy" (score / (A^T + I)^k 1)
  const float* score;
  const int32_t* rank;
  float* updated;
  int64_t* label;
  int32_t* words;  // [0] status: 0 = done, bit 0 = declined (input), bit 1 = round bound hit
  int nmax, ecap;
};

__global__ __launch_bounds__(1024) void kmis_graphs_kernel(KmGraphArgs p) {
  extern __shared__ unsigned long long km_lds[];
  unsigned long long* s_key = km_lds;
  unsigned long long* s_a = s_key + p.nmax;
  unsigned long long* s_b = s_a + p.nmax;
  uint32_t* s_edge = reinterpret_cast<uint32_t*>(s_b + p.nmax);
  uint8_t* s_mis = reinterpret_cast<uint8_t*>(s_edge + p.ecap);
  uint8_t* s_mask = s_mis + p.nmax;
  uint8_t* s_ma = s_mask + p.nmax;
  uint8_t* s_mb = s_ma + p.nmax;

  GraphFrame f;
  if (!graph_frame_open(p.row, p.col, p.E, p.N, p.gptr, p.nmax, p.ecap, s_edge, p.words, f, [](int64_t, int64_t) {}))
    return;  // (uniform)
  const int T = blockDim.x, tid = threadIdx.x;
  const int n = f.n;
  const int64_t n0 = f.n0, ne = f.ne;

  // ---- priorities
  if (p.mode == 2) {
    // counts of (A^T + I)^k 1 in integers: exact, and atomics on integers commute
    for (int i = tid; i < n; i += T) s_a[i] = 1ull;
    __syncthreads();
    for (int h = 0; h < p.k; ++h) {
      for (int i = tid; i < n; i += T) s_b[i] = s_a[i];
      __syncthreads();
      for (int64_t e = tid; e < ne; e += T) {
        int r, c;
        f.edge_at(e, r, c);
        atomicAdd(&s_b[c], s_a[r]);
      }
      __syncthreads();
      unsigned long long* t = s_a;
      s_a = s_b;
      s_b = t;
    }
  }
  for (int i = tid; i < n; i += T) {
    uint32_t prio;
    if (p.mode == 0) {
      prio = static_cast<uint32_t>(p.rank[n0 + i]);
    } else {
      float u = p.score[n0 + i];
      if (p.mode == 2) {
        u = u / static_cast<float>(s_a[i]);
        p.updated[n0 + i] = u;
      }
      prio = desc_bits(u);
    }
    s_key[i] = make_key(prio, i);
    s_mis[i] = 0;
    s_mask[i] = 0;
  }
  __syncthreads();

  // k hops of min over s_a (result left in s_a); stops early at a fixed point (further hops change nothing)
  auto min_hops = [&]() {
    for (int h = 0; h < p.k; ++h) {
      for (int i = tid; i < n; i += T) s_b[i] = s_a[i];
      __syncthreads();
      int changed = 0;
      for (int64_t e = tid; e < ne; e += T) {
        int r, c;
        f.edge_at(e, r, c);
        const unsigned long long v = s_a[r];
        if (v < s_a[c]) {  // (s_b[c] <= s_a[c]: anything not below s_a[c] cannot lower it)
          atomicMin(&s_b[c], v);
          changed = 1;
        }
      }
      const int any = __syncthreads_or(changed);
      unsigned long long* t = s_a;
      s_a = s_b;
      s_b = t;
      if (!any) break;
    }
  };

  // ---- rounds: each adds at least one node while an unmasked one exists, so n rounds is a hard cap
  bool finished = false;
  for (int round = 0; round <= n; ++round) {
    int open = 0;
    for (int i = tid; i < n; i += T) {
      const bool m = s_mask[i] != 0;
      open |= !m;
      s_a[i] = m ? KEY_INF : s_key[i];
    }
    if (!__syncthreads_or(open)) {
      finished = true;
      break;
    }
    min_hops();
    for (int i = tid; i < n; i += T) {
      if (s_a[i] == s_key[i]) s_mis[i] = 1;
      s_ma[i] = s_mis[i] | (s_a[i] == s_key[i] ? 1 : 0);
    }
    __syncthreads();
    for (int h = 0; h < p.k; ++h) {
      for (int i = tid; i < n; i += T) s_mb[i] = s_ma[i];
      __syncthreads();
      int changed = 0;
      for (int64_t e = tid; e < ne; e += T) {
        int r, c;
        f.edge_at(e, r, c);
        if (s_ma[r] && !s_ma[c]) {
          s_mb[c] = 1;
          changed = 1;
        }
      }
      const int any = __syncthreads_or(changed);
      uint8_t* t = s_ma;
      s_ma = s_mb;
      s_mb = t;
      if (!any) break;
    }
    for (int i = tid; i < n; i += T) s_mask[i] = s_ma[i];
    __syncthreads();
  }
  if (!finished) {
    if (tid == 0) atomicOr(p.words, 2);
    return;
  }
  // ---- clusters: the MIS keys travel k hops; the low word of what arrives names the owner
  for (int i = tid; i < n; i += T) s_a[i] = s_mis[i] ? s_key[i] : KEY_INF;
  __syncthreads();
  min_hops();
  for (int i = tid; i < n; i += T) {
    const unsigned long long v = s_a[i];
    p.label[n0 + i] = n0 + (v == KEY_INF ? static_cast<int64_t>(i) : static_cast<int64_t>(v & 0xFFFFFFFFull));
  }
}

// ------------------------------------------------------------------------------------------------ device-wide route
__global__ __launch_bounds__(256) void kmis_key_kernel(const int32_t* __restrict__ rank, const float* __restrict__ upd,
                                                       int64_t n, unsigned long long* __restrict__ key) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t prio = rank ? static_cast<uint32_t>(rank[i]) : desc_bits(upd[i]);
  key[i] = make_key(prio, i);
}

// One hop of min.  Items [0, E) are edges (push src(row) into y[col]), items [E, E + N) are nodes (push the node's own
// value, reset z for the hop after the next).  SRC 0: src = x; 1: the round's start (key of unmasked nodes);
// 2: the cluster pass's start (key of MIS nodes).
template <int SRC>
__global__ __launch_bounds__(256) void kmis_min_hop_kernel(const int64_t* __restrict__ row,
                                                           const int64_t* __restrict__ col, int64_t E, int64_t n,
                                                           const unsigned long long* __restrict__ key,
                                                           const unsigned long long* x, unsigned long long* y,
                                                           unsigned long long* z, const uint8_t* __restrict__ sel,
                                                           int32_t* __restrict__ open_flag) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  auto src = [&](int64_t i) -> unsigned long long {
    if (SRC == 0) return x[i];
    if (SRC == 1) return sel[i] ? KEY_INF : key[i];
    return sel[i] ? key[i] : KEY_INF;
  };
  if (idx < E) {
    const int64_t r = row[idx], c = col[idx];
    if (r == c || static_cast<uint64_t>(r) >= static_cast<uint64_t>(n) ||
        static_cast<uint64_t>(c) >= static_cast<uint64_t>(n))
      return;
    const unsigned long long v = src(r);
    // the destination only ever decreases during the hop: a value that is not below what a plain load sees cannot win
    if (v != KEY_INF && v < __hip_atomic_load(&y[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&y[c], v);
  } else if (idx < E + n) {
    const int64_t i = idx - E;
    const unsigned long long v = src(i);
    if (v != KEY_INF) {
      atomicMin(&y[i], v);
      if (SRC == 1) *open_flag = 1;
    }
    z[i] = KEY_INF;
  }
}

// One hop of the mask.  FIRST: the source is "in the MIS", old members or the ones this round adds (f[i] == key[i]); the
// node part also records the new members.  A lane may read mis[r] while r's own lane sets it: both conditions it ORs
// give the same answer then.
template <bool FIRST>
__global__ __launch_bounds__(256) void kmis_mask_hop_kernel(const int64_t* __restrict__ row,
                                                            const int64_t* __restrict__ col, int64_t E, int64_t n,
                                                            const unsigned long long* __restrict__ key,
                                                            const unsigned long long* __restrict__ f, uint8_t* mis,
                                                            const uint8_t* x, uint8_t* y, uint8_t* z) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  auto src = [&](int64_t i) -> bool {
    if (FIRST) return mis[i] != 0 || f[i] == key[i];
    return x[i] != 0;
  };
  if (idx < E) {
    const int64_t r = row[idx], c = col[idx];
    if (r == c || static_cast<uint64_t>(r) >= static_cast<uint64_t>(n) ||
        static_cast<uint64_t>(c) >= static_cast<uint64_t>(n))
      return;
    if (src(r)) y[c] = 1;
  } else if (idx < E + n) {
    const int64_t i = idx - E;
    if (src(i)) {
      y[i] = 1;
      if (FIRST) mis[i] = 1;
    }
    z[i] = 0;
  }
}

__global__ __launch_bounds__(256) void kmis_label_kernel(const unsigned long long* __restrict__ f, int64_t n,
                                                         int64_t* __restrict__ label) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long v = f[i];
  const int64_t o = static_cast<int64_t>(v & 0xFFFFFFFFull);
  label[i] = (v == KEY_INF || o >= n) ? i : o;
}

// ---- "greedy": counts of (A^T + I)^k 1, device-wide, same three-buffer rotation (y and z start at zero)
__global__ __launch_bounds__(256) void kmis_count_hop_kernel(const int64_t* __restrict__ row,
                                                             const int64_t* __restrict__ col, int64_t E, int64_t n,
                                                             const unsigned long long* x, unsigned long long* y,
                                                             unsigned long long* z, int first) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (idx < E) {
    const int64_t r = row[idx], c = col[idx];
    if (static_cast<uint64_t>(r) >= static_cast<uint64_t>(n) || static_cast<uint64_t>(c) >= static_cast<uint64_t>(n))
      return;
    atomicAdd(&y[c], first ? 1ull : x[r]);
  } else if (idx < E + n) {
    const int64_t i = idx - E;
    atomicAdd(&y[i], first ? 1ull : x[i]);
    z[i] = 0ull;
  }
}

__global__ __launch_bounds__(256) void kmis_divide_count_kernel(const float* __restrict__ score,
                                                                const unsigned long long* __restrict__ cnt, int64_t n,
                                                                float* __restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i < n) out[i] = score[i] / static_cast<float>(cnt ? cnt[i] : 1ull);
}

// ---- float sums by destination, in the order of the by-destination index (= edge-list order inside a group), starting
// from the node's own value: one order, fixed by the edge list, whoever calls.  One lane per destination.
__global__ __launch_bounds__(256) void kmis_wsum_kernel(const int64_t* __restrict__ row,
                                                        const int32_t* __restrict__ grp_ptr,
                                                        const int32_t* __restrict__ grp_perm,
                                                        const float* __restrict__ in, const float* __restrict__ score,
                                                        int64_t n, float* __restrict__ out) {
  const int64_t c = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (c >= n) return;
  float acc = in[c];
  const int32_t b = grp_ptr[c], e = grp_ptr[c + 1];
  for (int32_t j = b; j < e; ++j) {
    const int64_t r = row[grp_perm[j]];
    if (static_cast<uint64_t>(r) < static_cast<uint64_t>(n)) acc = acc + in[r];
  }
  out[c] = score ? score[c] / acc : acc;
}

__global__ __launch_bounds__(256) void kmis_degree_kernel(const int32_t* __restrict__ grp_ptr,
                                                          const int32_t* __restrict__ grp_perm,
                                                          const float* __restrict__ w, int64_t n,
                                                          float* __restrict__ out) {
  const int64_t c = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (c >= n) return;
  float acc = 0.0f;
  const int32_t b = grp_ptr[c], e = grp_ptr[c + 1];
  for (int32_t j = b; j < e; ++j) acc = acc + (w ? w[grp_perm[j]] : 1.0f);
  out[c] = acc;
}

// mis[id of i] = i for the owners (label[i] == i); ids ascend with the node index, so the list comes out sorted
__global__ __launch_bounds__(256) void kmis_mis_index_kernel(const int64_t* __restrict__ label,
                                                             const int64_t* __restrict__ index, int64_t n,
                                                             int64_t* __restrict__ mis) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n || label[i] != i) return;
  const int64_t id = index[n + i];
  if (id >= 0 && id < n) mis[id] = i;
}

struct KmWs {
  unsigned long long* key;
  unsigned long long* b[3];
  uint8_t* mis;
  uint8_t* m[3];
};
static KmWs km_carve(void* ws, int64_t n) {
  Carver cv(ws);
  KmWs w;
  w.key = cv.take<unsigned long long>(n);
  for (int q = 0; q < 3; ++q) w.b[q] = cv.take<unsigned long long>(n);
  w.mis = cv.take<uint8_t>(n);
  for (int q = 0; q < 3; ++q) w.m[q] = cv.take<uint8_t>(n);
  return w;
}

}  // namespace tgp

using namespace tgp;

extern "C" int tgp_kmis_max_graph_nodes(void) { return FRAME_GRAPH_MAX; }

extern "C" size_t tgp_kmis_workspace_bytes(int64_t num_nodes) {
  const size_t n = static_cast<size_t>(num_nodes > 0 ? num_nodes : 1);
  return 4 * align_up(n * sizeof(unsigned long long)) + 4 * align_up(n) + 256;
}

static bool km_args_ok(int64_t N, int64_t E, int k) {
  return N >= 0 && E >= 0 && k >= 0 && N < (1ll << 31) && E < (1ll << 40);
}

// Steps 2-5 of a sorted batch whose longest graph has at most max_graph_nodes (<= tgp_kmis_max_graph_nodes()) nodes, one
// workgroup per graph.  label[i] = the MIS node that owns i (an MIS node owns itself); words[0] = 0 when every graph was
// done, else the call is declined and label is meaningless.  mode 0: rank [N] int32 (rank of each node in the caller's
// permutation); 1: score [N] is compared as it is; 2: score / (A^T + I)^k 1, also written to updated [N].
extern "C" int tgp_kmis_graphs(const int64_t* row, const int64_t* col, int64_t E, int64_t N, const int64_t* graph_ptr,
                               int64_t B, int max_graph_nodes, int order_k, int mode, const float* score,
                               const int32_t* rank, float* updated, int64_t* label, int32_t* words, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(km_args_ok(N, E, order_k) && B >= 0 && B < (1ll << 31) && mode >= 0 && mode <= 2, TGP_ERR_INVALID,
              "tgp_kmis_graphs: bad argument");
  TGP_REQUIRE(max_graph_nodes >= 1 && max_graph_nodes <= FRAME_GRAPH_MAX, TGP_ERR_RANGE,
              "tgp_kmis_graphs: a graph of %d nodes does not fit one workgroup (max %d)", max_graph_nodes, FRAME_GRAPH_MAX);
  TGP_REQUIRE(words && graph_ptr && label && (E == 0 || (row && col)) && (mode == 0 ? rank != nullptr : score != nullptr) &&
                  (mode != 2 || updated),
              TGP_ERR_INVALID, "tgp_kmis_graphs: null pointer");
  (void)hipMemsetAsync(words, 0, sizeof(int32_t), stream);
  if (B == 0 || N == 0) return check_launch("tgp_kmis_graphs");
  KmGraphArgs p;
  p.row = row; p.col = col; p.E = E; p.N = N; p.gptr = graph_ptr; p.k = order_k; p.mode = mode;
  p.score = score; p.rank = rank; p.updated = updated; p.label = label; p.words = words;
  const FrameGeometry geo = graph_frame_geometry(max_graph_nodes);
  p.nmax = geo.nmax; p.ecap = geo.ecap;
  const size_t lds = static_cast<size_t>(p.nmax) * (3 * sizeof(unsigned long long) + 4) + static_cast<size_t>(p.ecap) * 4;
  hipLaunchKernelGGL(kmis_graphs_kernel, dim3(static_cast<unsigned>(B)), dim3(geo.threads), lds, stream, p);
  return check_launch("tgp_kmis_graphs");
}

// Device-wide route, step 0: keys from rank [N] int32 (or, rank null, from updated [N] float), cleared state.
extern "C" int tgp_kmis_rounds_start(const int32_t* rank, const float* updated, int64_t N, void* ws, size_t ws_bytes,
                                     void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(km_args_ok(N, 0, 0) && (N == 0 || rank || updated), TGP_ERR_INVALID, "tgp_kmis_rounds_start: bad argument");
  if (N == 0) return TGP_OK;
  TGP_REQUIRE(ws && ws_bytes >= tgp_kmis_workspace_bytes(N), TGP_ERR_WORKSPACE,
              "tgp_kmis_rounds_start: workspace too small");
  KmWs w = km_carve(ws, N);
  for (int q = 0; q < 3; ++q) {
    (void)hipMemsetAsync(w.b[q], 0xFF, static_cast<size_t>(N) * sizeof(unsigned long long), stream);
    (void)hipMemsetAsync(w.m[q], 0, static_cast<size_t>(N), stream);
  }
  (void)hipMemsetAsync(w.mis, 0, static_cast<size_t>(N), stream);
  hipLaunchKernelGGL(kmis_key_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, rank, updated, N, w.key);
  return check_launch("tgp_kmis_rounds_start");
}

// `rounds` rounds, numbered from `round_base` (rounds already launched since tgp_kmis_rounds_start: the buffer rotation
// follows the hop count).  open_flags[j] = 1 when round j met an unmasked node; a round that meets none changes
// nothing, so launching more rounds than needed is harmless.  2 * order_k launches per round.
extern "C" int tgp_kmis_rounds(const int64_t* row, const int64_t* col, int64_t E, int64_t N, int order_k, void* ws,
                               int64_t round_base, int rounds, int32_t* open_flags, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(km_args_ok(N, E, order_k) && order_k >= 1 && rounds >= 0 && round_base >= 0 && open_flags && ws &&
                  (E == 0 || (row && col)),
              TGP_ERR_INVALID, "tgp_kmis_rounds: bad argument");
  (void)hipMemsetAsync(open_flags, 0, sizeof(int32_t) * static_cast<size_t>(rounds > 0 ? rounds : 1), stream);
  if (N == 0 || rounds == 0) return check_launch("tgp_kmis_rounds");
  KmWs w = km_carve(ws, N);
  const dim3 grid(cdiv(E + N, 256)), block(256);
  for (int j = 0; j < rounds; ++j) {
    const int64_t h0 = (round_base + j) * order_k;  // hops done before this round, of either kind
    for (int h = 0; h < order_k; ++h) {
      const int64_t t = h0 + h;
      unsigned long long *x = w.b[t % 3], *y = w.b[(t + 1) % 3], *z = w.b[(t + 2) % 3];
      if (h == 0)
        hipLaunchKernelGGL(kmis_min_hop_kernel<1>, grid, block, 0, stream, row, col, E, N, w.key, x, y, z, w.m[h0 % 3],
                           open_flags + j);
      else
        hipLaunchKernelGGL(kmis_min_hop_kernel<0>, grid, block, 0, stream, row, col, E, N, w.key, x, y, z,
                           static_cast<const uint8_t*>(nullptr), static_cast<int32_t*>(nullptr));
    }
    const unsigned long long* f = w.b[(h0 + order_k) % 3];
    for (int h = 0; h < order_k; ++h) {
      const int64_t u = h0 + h;
      uint8_t *x = w.m[u % 3], *y = w.m[(u + 1) % 3], *z = w.m[(u + 2) % 3];
      if (h == 0)
        hipLaunchKernelGGL(kmis_mask_hop_kernel<true>, grid, block, 0, stream, row, col, E, N, w.key, f, w.mis, x, y, z);
      else
        hipLaunchKernelGGL(kmis_mask_hop_kernel<false>, grid, block, 0, stream, row, col, E, N, w.key, f, w.mis, x, y, z);
    }
  }
  return check_launch("tgp_kmis_rounds");
}

// After the rounds: label[i] = owner of i.  `rounds_done` = rounds launched since tgp_kmis_rounds_start.
extern "C" int tgp_kmis_clusters(const int64_t* row, const int64_t* col, int64_t E, int64_t N, int order_k, void* ws,
                                 int64_t rounds_done, int64_t* label, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(km_args_ok(N, E, order_k) && order_k >= 1 && rounds_done >= 0 && (N == 0 || (label && ws)) &&
                  (E == 0 || (row && col)),
              TGP_ERR_INVALID, "tgp_kmis_clusters: bad argument");
  if (N == 0) return TGP_OK;
  KmWs w = km_carve(ws, N);
  const dim3 grid(cdiv(E + N, 256)), block(256);
  const int64_t h0 = rounds_done * order_k;
  for (int h = 0; h < order_k; ++h) {
    const int64_t t = h0 + h;
    unsigned long long *x = w.b[t % 3], *y = w.b[(t + 1) % 3], *z = w.b[(t + 2) % 3];
    if (h == 0)
      hipLaunchKernelGGL(kmis_min_hop_kernel<2>, grid, block, 0, stream, row, col, E, N, w.key, x, y, z, w.mis,
                         static_cast<int32_t*>(nullptr));
    else
      hipLaunchKernelGGL(kmis_min_hop_kernel<0>, grid, block, 0, stream, row, col, E, N, w.key, x, y, z,
                         static_cast<const uint8_t*>(nullptr), static_cast<int32_t*>(nullptr));
  }
  hipLaunchKernelGGL(kmis_label_kernel, dim3(cdiv(N, 256)), block, 0, stream, w.b[(h0 + order_k) % 3], N, label);
  return check_launch("tgp_kmis_clusters");
}

// updated[i] = score[i] / ((A^T + I)^k 1)[i], the counts kept in 64-bit integers (ws as for the rounds, used before them)
extern "C" int tgp_kmis_greedy_f32(const int64_t* row, const int64_t* col, int64_t E, int64_t N, int order_k,
                                   const float* score, void* ws, size_t ws_bytes, float* updated, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(km_args_ok(N, E, order_k) && (N == 0 || (score && updated)) && (E == 0 || (row && col)), TGP_ERR_INVALID,
              "tgp_kmis_greedy_f32: bad argument");
  if (N == 0) return TGP_OK;
  TGP_REQUIRE(ws && ws_bytes >= tgp_kmis_workspace_bytes(N), TGP_ERR_WORKSPACE, "tgp_kmis_greedy_f32: workspace too small");
  KmWs w = km_carve(ws, N);
  const dim3 grid(cdiv(E + N, 256)), block(256);
  if (order_k > 0) {
    (void)hipMemsetAsync(w.b[1], 0, static_cast<size_t>(N) * sizeof(unsigned long long), stream);
    (void)hipMemsetAsync(w.b[2], 0, static_cast<size_t>(N) * sizeof(unsigned long long), stream);
  }
  for (int h = 0; h < order_k; ++h)
    hipLaunchKernelGGL(kmis_count_hop_kernel, grid, block, 0, stream, row, col, E, N, w.b[h % 3], w.b[(h + 1) % 3],
                       w.b[(h + 2) % 3], h == 0 ? 1 : 0);
  hipLaunchKernelGGL(kmis_divide_count_kernel, dim3(cdiv(N, 256)), block, 0, stream, score,
                     order_k > 0 ? w.b[order_k % 3] : static_cast<unsigned long long*>(nullptr), N, updated);
  return check_launch("tgp_kmis_greedy_f32");
}

// out[c] = in[c] + sum over the edges (r, c) of in[r], in the order of the by-destination index (grp_ptr [N+1],
// grp_perm [E]: edge positions grouped by col, ascending inside a group); with `score`, out[c] = score[c] / that sum.
extern "C" int tgp_kmis_wsum_f32(const int64_t* row, const int32_t* grp_ptr, const int32_t* grp_perm, const float* in,
                                 const float* score, int64_t N, float* out, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(N >= 0 && (N == 0 || (grp_ptr && grp_perm && in && out)), TGP_ERR_INVALID, "tgp_kmis_wsum_f32: bad argument");
  if (N == 0) return TGP_OK;
  hipLaunchKernelGGL(kmis_wsum_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, row, grp_ptr, grp_perm, in, score, N, out);
  return check_launch("tgp_kmis_wsum_f32");
}

// out[c] = sum of w over the edges into c (w null: their number), same order as tgp_kmis_wsum_f32
extern "C" int tgp_kmis_degree_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const float* w, int64_t N, float* out,
                                   void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(N >= 0 && (N == 0 || (grp_ptr && grp_perm && out)), TGP_ERR_INVALID, "tgp_kmis_degree_f32: bad argument");
  if (N == 0) return TGP_OK;
  hipLaunchKernelGGL(kmis_degree_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, grp_ptr, grp_perm, w, N, out);
  return check_launch("tgp_kmis_degree_f32");
}

// mis[c] = the node that owns cluster c, from the owners (label) and the relabelled index [2, N]
extern "C" int tgp_kmis_mis_index_i64(const int64_t* label, const int64_t* index, int64_t N, int64_t* mis, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(N >= 0 && (N == 0 || (label && index && mis)), TGP_ERR_INVALID, "tgp_kmis_mis_index_i64: bad argument");
  if (N == 0) return TGP_OK;
  hipLaunchKernelGGL(kmis_mis_index_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, label, index, N, mis);
  return check_launch("tgp_kmis_mis_index_i64");
}
