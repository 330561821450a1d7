// What the per-graph routes of the k-MIS selector (kmis_select.hip) and the edge-contraction selector
// (edge_contract.hip) share: the 64-bit priority key, the limits of one workgroup's frame, the prologue that finds and
// CHECKS a graph's edges before anything is read out of LDS, and the launch geometry.  (graclus_match.hip's per-graph
// kernel works from a CSR and validates differently: it is not a client.)
#pragma once
#include "common.h"
#include "lookback.h"

namespace tgp {

constexpr int FRAME_GRAPH_MAX = 1024;       // nodes of a graph one workgroup holds in LDS (local ids are 16-bit pairs)
constexpr int FRAME_EDGE_CACHE_MAX = 4096;  // edges of a graph staged in LDS as packed local pairs; the rest stay in L2
constexpr unsigned long long KEY_INF = ~0ull;

// float -> uint32 whose ASCENDING unsigned order is DESCENDING float order; -0 ties with +0 and every NaN sorts first,
// as torch's descending sort has them
__device__ __forceinline__ uint32_t desc_bits(float v) {
  if (v != v) return 0u;
  if (v == 0.0f) v = 0.0f;
  const uint32_t b = __float_as_uint(v);
  const uint32_t asc = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ~asc;
}

// (prio << 32) | id, smaller = earlier: the id in the low word makes keys unique, breaks ties towards the lower id (what
// a stable descending argsort does) and names the owner of whatever minimum arrives somewhere
__device__ __forceinline__ unsigned long long make_key(uint32_t prio, int64_t id) {
  return (static_cast<unsigned long long>(prio) << 32) | static_cast<unsigned long long>(id);
}

// One graph of a sorted batch as its workgroup sees it: nodes [n0, n0 + n), edges [lo, lo + ne) of the list, the first
// `ecap` of them in LDS as (local row << 16) | local col.
struct GraphFrame {
  const int64_t* row;
  const int64_t* col;
  const uint32_t* cache;
  int64_t n0, lo, ne;
  int n, ecap;
  // local endpoints of edge e.  A client with a word of its own beside each cached pair tests cached(e) ONCE and reads both
  // in that branch: edge_at() followed by a second test of the same condition measured 9 % slower on EdgePool's matching
  // of 2048 small graphs (profiles/selector_frame_ab.txt).
  __device__ __forceinline__ bool cached(int64_t e) const { return e < ecap; }
  __device__ __forceinline__ void cached_edge(int64_t e, int& r, int& c) const {
    const uint32_t pk = cache[e];
    r = static_cast<int>(pk >> 16);
    c = static_cast<int>(pk & 0xFFFFu);
  }
  __device__ __forceinline__ void listed_edge(int64_t e, int& r, int& c) const {
    r = static_cast<int>(row[lo + e] - n0);
    c = static_cast<int>(col[lo + e] - n0);
  }
  __device__ __forceinline__ void edge_at(int64_t e, int& r, int& c) const {
    if (cached(e)) cached_edge(e, r, c);
    else listed_edge(e, r, c);
  }
};

// Opens the frame of graph blockIdx.x; every thread of the workgroup calls it.  The graph's edges are the entries of
// `row` in [n0, n1), found by two in-wave lower bounds; the ranges of consecutive graphs tile [0, E), so a list that is
// not grouped by graph, or has an edge between two graphs, has an edge outside its graph in SOME workgroup.  Refused
// (bit 0 of *status set by thread 0): a graph longer than nmax or outside [0, N), a broken edge range, an edge with an
// endpoint outside the graph.  Returns false for a refused and for an empty graph: the caller returns, having written
// nothing.  Every return and every barrier is workgroup-uniform; the barrier before a `true` makes the cache (and what
// on_cached wrote) visible.  on_cached(e, list position) runs once per edge that went into the cache, in the same pass
// (a client stages a word of its own beside the pair).  cache: LDS, ecap words.
template <class OnCached>
__device__ __forceinline__ bool graph_frame_open(const int64_t* row, const int64_t* col, int64_t E, int64_t N,
                                                 const int64_t* gptr, int nmax, int ecap, uint32_t* cache,
                                                 int32_t* status, GraphFrame& f, OnCached on_cached) {
  __shared__ int64_t s_range[2];
  const int T = blockDim.x, tid = threadIdx.x;
  const int64_t n0 = gptr[blockIdx.x], n1 = gptr[blockIdx.x + 1];
  const int64_t n64 = n1 - n0;
  if (n64 <= 0) return false;  // (uniform)
  if (n64 > nmax || n0 < 0 || n1 > N) {
    if (tid == 0) atomicOr(status, 1);
    return false;
  }
  const int n = static_cast<int>(n64);
  if (tid < 64) {
    const int64_t* const arr[2] = {row, row};
    const int64_t len[2] = {E, E}, key[2] = {n0, n1};
    int64_t res[2];
    wave_lower_bounds<2>(arr, len, key, res);
    if (tid == 0) {
      s_range[0] = res[0];
      s_range[1] = res[1];
    }
  }
  __syncthreads();
  const int64_t lo = s_range[0];
  const int64_t ne = s_range[1] - lo;
  if (ne < 0 || lo < 0 || s_range[1] > E) {
    if (tid == 0) atomicOr(status, 1);
    return false;
  }
  int bad = 0;
  for (int64_t e = tid; e < ne; e += T) {
    const int64_t r = row[lo + e] - n0, c = col[lo + e] - n0;
    if (r < 0 || r >= n || c < 0 || c >= n) {
      bad = 1;
    } else if (e < ecap) {
      cache[e] = (static_cast<uint32_t>(r) << 16) | static_cast<uint32_t>(c);
      on_cached(e, lo + e);
    }
  }
  if (__syncthreads_or(bad)) {
    if (tid == 0) atomicOr(status, 1);
    return false;
  }
  f = GraphFrame{row, col, cache, n0, lo, ne, n, ecap};
  return true;
}

// Launch geometry of a frame for graphs of at most max_graph_nodes nodes; each client adds up its own dynamic LDS
struct FrameGeometry { int nmax, ecap, threads; };
static inline FrameGeometry graph_frame_geometry(int max_graph_nodes) {
  const int nmax = (max_graph_nodes + 63) / 64 * 64;
  const int ecap = 16 * nmax > FRAME_EDGE_CACHE_MAX ? FRAME_EDGE_CACHE_MAX : 16 * nmax;
  return {nmax, ecap, nmax <= 64 ? 64 : (nmax <= 256 ? 256 : 1024)};
}

}  // namespace tgp
