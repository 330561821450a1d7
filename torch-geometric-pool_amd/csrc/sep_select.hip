// SEP pooling's selector (Wu et al., ICML 2022; reference select/sep_select.py, levels = 1): per graph a coding tree
// grown by greedy merging, compressed to height 2; the root's children are the clusters.  DESIGN 4.26 states the
// algorithm, tests/sep_restatement.py is its brute-force form.
//
// One workgroup of 256 threads per graph, thread x owning row / slot x (a graph has at most SEP_MAX_NODES <= 256 nodes).
//   gather:      row x adds its node's edges, out-edges and in-edges merged by edge position (edge-list order), into the
//                fp32 cut table C in LDS; self-loops are skipped.  C[x][y] and C[y][x] receive the same numbers in the
//                same order: the table is symmetric to the bit.
//   components:  min-label propagation over C's nonzeros, double-buffered.
//   merging:     one global sequence of merges (merges of different components are independent; inside a component the
//                order is the minimum of (delta, a, b) by creation id).  Every live row keeps its best partner; a merge
//                of slots sa, sb writes C[sa][.] = C[sa][.] + C[sb][.] (the new cluster reuses slot sa), rescans the rows
//                whose best named sa or sb and the new row (a wave per row, lanes over the columns), and offers the new
//                row's deltas to every other row.  Deltas are fp64, written as the restatement writes them; the library
//                is built with -ffp-contract=off.
//   compressing: per round true heights by a leaf walk (integer atomicMax in LDS), depths by a pointer walk, the minimum
//                of (child_cut * ln(vol_parent / vol_u), u) over the eligible nodes is removed.
//   labels:      per component (by smallest node) the root's internal children by creation id, then its leaf children by
//                node; the per-graph counts are prefix-summed and added by two small launches behind the kernel.
// No float atomics and no dependence on the graph's place in the batch: the same input gives the same bits.
#include "common.h"

#include <float.h>
#include <limits.h>

namespace tgp {
namespace {

constexpr int SEP_THREADS = 256;
constexpr size_t SEP_LDS_BYTES = 160 * 1024;

constexpr int SEP_BAD_INPUT = 1;   // an index outside its table, an edge across two graphs
constexpr int SEP_BAD_WEIGHT = 2;  // a non-finite or negative summed weight
constexpr int SEP_OVER_LIMIT = 4;  // a graph of more than max_n nodes

struct SepLds {
  int ldc;
  size_t c, vol, g, cc, bestd, dnew, compvol, redd, parent, height, cid, alive, label, label2, slot_node, live, best_p,
      need, nextcid, keyv, first, redi, total;
};
inline SepLds sep_lds_layout(int m) {
  SepLds l;
  l.ldc = m | 1;  // odd row stride: a column walk does not stay on one bank
  const size_t tn = 2 * static_cast<size_t>(m);  // tree nodes: m leaves and at most m - 1 merges
  size_t off = 0;
  l.vol = off;       off += sizeof(double) * tn;
  l.g = off;         off += sizeof(double) * tn;
  l.cc = off;        off += sizeof(double) * tn;
  l.bestd = off;     off += sizeof(double) * m;
  l.dnew = off;      off += sizeof(double) * m;
  l.compvol = off;   off += sizeof(double) * m;
  l.redd = off;      off += sizeof(double) * 4;
  l.c = off;         off += sizeof(float) * m * l.ldc;
  l.parent = off;    off += sizeof(int) * tn;
  l.height = off;    off += sizeof(int) * tn;
  l.cid = off;       off += sizeof(int) * tn;
  l.alive = off;     off += sizeof(int) * tn;
  l.label = off;     off += sizeof(int) * m;
  l.label2 = off;    off += sizeof(int) * m;
  l.slot_node = off; off += sizeof(int) * m;
  l.live = off;      off += sizeof(int) * m;
  l.best_p = off;    off += sizeof(int) * m;
  l.need = off;      off += sizeof(int) * m;
  l.nextcid = off;   off += sizeof(int) * m;
  l.keyv = off;      off += sizeof(int) * m;
  l.first = off;     off += sizeof(int) * m;
  l.redi = off;      off += sizeof(int) * 16;
  l.total = off;
  return l;
}
inline int sep_max_nodes() {
  static const int limit = [] {
    int m = 1;
    while (m < SEP_THREADS && sep_lds_layout(m + 1).total <= SEP_LDS_BYTES) ++m;
    return m;
  }();
  return limit;
}

struct SepArgs {
  const int32_t* src_ptr;   // [N + 1] by-source offsets
  const int32_t* src_perm;  // [E] edge positions by source (NULL: the list is grouped already)
  const int32_t* dst_ptr;   // [N + 1] by-destination offsets
  const int32_t* dst_perm;  // [E] or NULL
  const int64_t* src;       // [E]
  const int64_t* dst;       // [E]
  const float* w;           // [E] or NULL
  const int32_t* gid;       // [N] graph of every node
  const int32_t* graph_ptr; // [G + 1]: graph g owns nodes graph_ptr[g] .. graph_ptr[g + 1] - 1
  int N, E, G, max_n;
  int64_t* cluster;         // [N] local labels (the offsets are added behind the kernel)
  int32_t* counts;          // [G]
  int32_t* status;
  SepLds l;
};

// a candidate: the value and the (lo, hi) ids that break ties; s0, s1 are what the winner hands back
struct SepKey {
  double d;
  int lo, hi, s0, s1;
};
__device__ __forceinline__ SepKey sep_none() { return SepKey{__builtin_huge_val(), INT_MAX, INT_MAX, INT_MAX, INT_MAX}; }
__device__ __forceinline__ bool sep_less(const SepKey& a, const SepKey& b) {
  if (a.d != b.d) return a.d < b.d;
  if (a.lo != b.lo) return a.lo < b.lo;
  if (a.hi != b.hi) return a.hi < b.hi;
  return a.s0 < b.s0;
}
__device__ __forceinline__ SepKey sep_wave_min(SepKey k) {
  for (int off = 32; off >= 1; off >>= 1) {
    SepKey o;
    o.d = __shfl_xor(k.d, off);
    o.lo = __shfl_xor(k.lo, off);
    o.hi = __shfl_xor(k.hi, off);
    o.s0 = __shfl_xor(k.s0, off);
    o.s1 = __shfl_xor(k.s1, off);
    if (sep_less(o, k)) k = o;
  }
  return k;
}
// the minimum over the workgroup, the same in every thread (two barriers; redd / redi are free again behind them)
__device__ __forceinline__ SepKey sep_block_min(SepKey k, double* redd, int* redi) {
  k = sep_wave_min(k);
  const int wv = wave_id();
  __syncthreads();
  if (lane_id() == 0) {
    redd[wv] = k.d;
    redi[wv * 4 + 0] = k.lo;
    redi[wv * 4 + 1] = k.hi;
    redi[wv * 4 + 2] = k.s0;
    redi[wv * 4 + 3] = k.s1;
  }
  __syncthreads();
  SepKey best = sep_none();
  for (int v = 0; v < SEP_THREADS / 64; ++v) {
    const SepKey o{redd[v], redi[v * 4 + 0], redi[v * 4 + 1], redi[v * 4 + 2], redi[v * 4 + 3]};
    if (sep_less(o, best)) best = o;
  }
  return best;
}

__device__ __forceinline__ double sep_log2(double x) { return log(x) / log(2.0); }

// the entropy change of merging a and b (a: the lower creation id), as tests/sep_restatement.py writes it
__device__ __forceinline__ double sep_delta(double va, double ga, double vb, double gb, double cut, double VOL) {
  const double vab = va + vb;
  const double t1 = (va - ga) * sep_log2(vab / va);
  const double t2 = (vb - gb) * sep_log2(vab / vb);
  const double t3 = (2.0 * cut) * sep_log2(VOL / vab);
  return (t1 + t2 - t3) / VOL;
}

struct SepFrame {
  float* C;
  double *vol, *g, *cc, *bestd, *dnew, *compvol, *redd;
  int *parent, *height, *cid, *alive, *label, *label2, *slot_node, *live, *best_p, *need, *nextcid, *keyv, *first, *redi;
  int ldc;
};

// the candidate (row r, column x): both live, adjacent
__device__ __forceinline__ SepKey sep_pair(const SepFrame& f, int r, int x) {
  const int tr = f.slot_node[r], tx = f.slot_node[x];
  const int cr = f.cid[tr], cx = f.cid[tx];
  const double cut = static_cast<double>(f.C[r * f.ldc + x]);
  const double VOL = f.compvol[f.label[r]];
  SepKey k;
  if (cr < cx) {
    k.d = sep_delta(f.vol[tr], f.g[tr], f.vol[tx], f.g[tx], cut, VOL);
    k.lo = cr, k.hi = cx, k.s0 = r, k.s1 = x;
  } else {
    k.d = sep_delta(f.vol[tx], f.g[tx], f.vol[tr], f.g[tr], cut, VOL);
    k.lo = cx, k.hi = cr, k.s0 = x, k.s1 = r;
  }
  return k;
}

// one wave scans row r over the columns; lane 0 stores the row's best partner.  fill: also dnew[x] for every column
__device__ __forceinline__ void sep_scan_row(const SepFrame& f, int r, int n, bool fill) {
  SepKey best = sep_none();
  int partner = -1;
  for (int x = lane_id(); x < n; x += 64) {
    const bool ok = x != r && f.live[x] && f.C[r * f.ldc + x] != 0.0f;
    SepKey k = sep_none();
    if (ok) k = sep_pair(f, r, x);
    if (fill) f.dnew[x] = k.d;
    if (ok && sep_less(k, best)) best = k, partner = x;
  }
  // the partner rides along in s1 (s0 breaks a tie between equal (d, lo, hi): impossible inside one row)
  best.s0 = partner < 0 ? INT_MAX : partner;
  best = sep_wave_min(best);
  if (lane_id() == 0) {
    f.bestd[r] = best.d;
    f.best_p[r] = best.s0 == INT_MAX ? -1 : best.s0;
  }
}

__global__ __launch_bounds__(SEP_THREADS) void sep_select_kernel(SepArgs p) {
  extern __shared__ double sep_smem[];
  char* const base = reinterpret_cast<char*>(sep_smem);
  SepFrame f;
  f.C = reinterpret_cast<float*>(base + p.l.c);
  f.vol = reinterpret_cast<double*>(base + p.l.vol);
  f.g = reinterpret_cast<double*>(base + p.l.g);
  f.cc = reinterpret_cast<double*>(base + p.l.cc);
  f.bestd = reinterpret_cast<double*>(base + p.l.bestd);
  f.dnew = reinterpret_cast<double*>(base + p.l.dnew);
  f.compvol = reinterpret_cast<double*>(base + p.l.compvol);
  f.redd = reinterpret_cast<double*>(base + p.l.redd);
  f.parent = reinterpret_cast<int*>(base + p.l.parent);
  f.height = reinterpret_cast<int*>(base + p.l.height);
  f.cid = reinterpret_cast<int*>(base + p.l.cid);
  f.alive = reinterpret_cast<int*>(base + p.l.alive);
  f.label = reinterpret_cast<int*>(base + p.l.label);
  f.label2 = reinterpret_cast<int*>(base + p.l.label2);
  f.slot_node = reinterpret_cast<int*>(base + p.l.slot_node);
  f.live = reinterpret_cast<int*>(base + p.l.live);
  f.best_p = reinterpret_cast<int*>(base + p.l.best_p);
  f.need = reinterpret_cast<int*>(base + p.l.need);
  f.nextcid = reinterpret_cast<int*>(base + p.l.nextcid);
  f.keyv = reinterpret_cast<int*>(base + p.l.keyv);
  f.first = reinterpret_cast<int*>(base + p.l.first);
  f.redi = reinterpret_cast<int*>(base + p.l.redi);
  f.ldc = p.l.ldc;
  const int ldc = f.ldc, tid = threadIdx.x, T = SEP_THREADS;
  const int g = blockIdx.x;

  // ---- per-workgroup (uniform) decisions
  const int t0 = p.graph_ptr[g], t1 = p.graph_ptr[g + 1];
  if (t0 < 0 || t1 < t0 || t1 > p.N) {
    if (tid == 0) atomicOr(p.status, SEP_BAD_INPUT);
    return;
  }
  const int n = t1 - t0;
  if (n == 0) return;
  if (n > p.max_n) {
    if (tid == 0) atomicOr(p.status, SEP_OVER_LIMIT);
    return;
  }
  const bool has = tid < n;  // (n <= max_n <= 256 threads: thread x owns row x)
  const int node = t0 + tid;

  // ---- the cut table: row x adds its node's edges in edge-list order (out- and in-edges merged by position)
  for (int i = tid; i < n * ldc; i += T) f.C[i] = 0.0f;
  __syncthreads();
  int bad = 0;
  if (has) {
    if (p.gid[node] != g) bad = 1;
    const int s0 = p.src_ptr[node], s1 = p.src_ptr[node + 1];
    const int d0 = p.dst_ptr[node], d1 = p.dst_ptr[node + 1];
    if (s0 < 0 || s1 < s0 || s1 > p.E || d0 < 0 || d1 < d0 || d1 > p.E) {
      bad = 1;
    } else {
      int i = s0, j = d0;
      while (i < s1 || j < d1) {
        const int ps = i < s1 ? (p.src_perm ? p.src_perm[i] : i) : INT_MAX;
        const int pd = j < d1 ? (p.dst_perm ? p.dst_perm[j] : j) : INT_MAX;
        const bool from_src = ps <= pd;
        const int pos = from_src ? ps : pd;
        if (from_src) ++i;
        else ++j;
        if (pos < 0 || pos >= p.E) {
          bad = 1;
          continue;
        }
        const int64_t mine = from_src ? p.src[pos] : p.dst[pos];
        const int64_t other = from_src ? p.dst[pos] : p.src[pos];
        if (mine != node || other < 0 || other >= p.N) {
          bad = 1;
          continue;
        }
        if (other == node) continue;  // a self-loop (it stands in both lists)
        const int64_t b = other - t0;
        if (p.gid[other] != g || b < 0 || b >= n) {  // an edge that leaves the graph
          bad = 1;
          continue;
        }
        f.C[tid * ldc + static_cast<int>(b)] += p.w ? p.w[pos] : 1.0f;
      }
    }
  }
  if (__syncthreads_or(bad)) {
    if (tid == 0) atomicOr(p.status, SEP_BAD_INPUT);
    return;
  }
  // ---- weights finite and >= 0; the leaves' volumes: the fp32 entries in ascending column order into fp64
  if (has) {
    double rs = 0.0;
    for (int b = 0; b < n; ++b) {
      const float v = f.C[tid * ldc + b];
      if (!(v >= 0.0f && v <= FLT_MAX)) bad = 1;
      rs += static_cast<double>(v);
    }
    f.vol[tid] = f.g[tid] = rs;
    f.cc[tid] = 0.0;
    f.parent[tid] = -1;
    f.height[tid] = 0;
    f.alive[tid] = 1;
    f.slot_node[tid] = tid;
    f.live[tid] = 1;
    f.label[tid] = tid;
  }
  if (__syncthreads_or(bad)) {
    if (tid == 0) atomicOr(p.status, SEP_BAD_WEIGHT);
    return;
  }
  // ---- connected components: every node takes the smallest label among its neighbours' (and that label's label)
  {
    int* cur = f.label;
    int* nxt = f.label2;
    for (int it = 0; it <= n; ++it) {
      int changed = 0;
      if (has) {
        int m = cur[tid];
        for (int b = 0; b < n; ++b)
          if (f.C[tid * ldc + b] != 0.0f && cur[b] < m) m = cur[b];
        if (cur[m] < m) m = cur[m];
        changed = m != cur[tid];
        nxt[tid] = m;
      }
      const int any = __syncthreads_or(changed);
      int* const t = cur;
      cur = nxt;
      nxt = t;
      if (!any) break;
    }
    if (cur != f.label) {  // (uniform)
      if (has) f.label[tid] = cur[tid];
      __syncthreads();
    }
  }
  // ---- leaves: creation id = rank inside the component; VOL and the next id per component (kept at its label)
  if (has) {
    const int lab = f.label[tid];
    int rank = 0;
    for (int b = 0; b < tid; ++b) rank += f.label[b] == lab;
    f.cid[tid] = rank;
    if (lab == tid) {
      double V = 0.0;
      int size = 0;
      for (int b = 0; b < n; ++b)
        if (f.label[b] == tid) V += f.vol[b], ++size;
      f.compvol[tid] = V;
      f.nextcid[tid] = size;
    }
  }
  __syncthreads();
  // ---- every row's best partner
  if (has) {
    SepKey best = sep_none();
    int partner = -1;
    for (int x = 0; x < n; ++x) {
      if (x == tid || f.C[tid * ldc + x] == 0.0f) continue;
      const SepKey k = sep_pair(f, tid, x);
      if (sep_less(k, best)) best = k, partner = x;
    }
    f.bestd[tid] = best.d;
    f.best_p[tid] = partner;
  }
  __syncthreads();

  // ---- merging
  int next_node = n;  // (uniform: every thread counts the merges)
  for (;;) {
    SepKey mine = sep_none();
    if (has && f.live[tid] && f.best_p[tid] >= 0) {
      const int x = f.best_p[tid];
      const int ca = f.cid[f.slot_node[tid]], cb = f.cid[f.slot_node[x]];
      mine.d = f.bestd[tid];
      if (ca < cb) mine.lo = ca, mine.hi = cb, mine.s0 = tid, mine.s1 = x;
      else mine.lo = cb, mine.hi = ca, mine.s0 = x, mine.s1 = tid;
    }
    const SepKey win = sep_block_min(mine, f.redd, f.redi);
    if (win.s0 == INT_MAX) break;  // no adjacent live pair is left: every component is one cluster
    const int sa = win.s0, sb = win.s1, t = next_node++;
    if (has) {
      if (tid != sa && tid != sb) {
        const float v = f.C[sa * ldc + tid] + f.C[sb * ldc + tid];
        f.C[sa * ldc + tid] = v;
        f.C[tid * ldc + sa] = v;
        f.need[tid] = f.live[tid] && (f.best_p[tid] == sa || f.best_p[tid] == sb);
      } else {
        f.need[tid] = tid == sa;
      }
    }
    if (tid == 0) {
      const int ta = f.slot_node[sa], tb = f.slot_node[sb];
      const double cut = static_cast<double>(f.C[sa * ldc + sb]);
      f.vol[t] = f.vol[ta] + f.vol[tb];
      f.g[t] = f.g[ta] + f.g[tb] - 2.0 * cut;
      f.cc[t] = cut;
      f.height[t] = (f.height[ta] > f.height[tb] ? f.height[ta] : f.height[tb]) + 1;
      f.parent[ta] = f.parent[tb] = t;
      f.parent[t] = -1;
      f.alive[t] = 1;
      const int lab = f.label[sa];
      f.cid[t] = f.nextcid[lab];
      f.nextcid[lab] += 1;
      f.slot_node[sa] = t;
      f.live[sb] = 0;
    }
    __syncthreads();
    for (int r = wave_id(); r < n; r += T / 64)  // (r and need[r] are uniform inside a wave)
      if (f.need[r]) sep_scan_row(f, r, n, r == sa);
    __syncthreads();
    if (has && f.live[tid] && !f.need[tid]) {  // the new cluster is offered to every other row
      const double d = f.dnew[tid];
      if (d < __builtin_huge_val()) {
        const int x = f.best_p[tid], mc = f.cid[f.slot_node[tid]];
        bool take = x < 0;
        if (!take) {
          const int xc = f.cid[f.slot_node[x]];
          const SepKey cur{f.bestd[tid], mc < xc ? mc : xc, mc < xc ? xc : mc, 0, 0};
          const SepKey neu{d, mc, f.cid[t], 0, 0};  // (the new cluster's id is the largest of its component)
          take = sep_less(neu, cur);
        }
        if (take) f.bestd[tid] = d, f.best_p[tid] = sa;
      }
    }
    __syncthreads();
  }

  // ---- compressing every component's tree to height 2
  const int num_nodes = next_node;  // tree nodes: leaves 0 .. n - 1, merges n .. num_nodes - 1
  for (;;) {
    for (int u = n + tid; u < num_nodes; u += T) f.height[u] = 0;
    __syncthreads();
    if (has) {
      int k = 0;
      for (int u = f.parent[tid]; u >= 0; u = f.parent[u]) atomicMax(&f.height[u], ++k);
    }
    __syncthreads();
    SepKey mine = sep_none();
    for (int u = n + tid; u < num_nodes; u += T) {
      const int pu = f.parent[u];
      if (!f.alive[u] || pu < 0) continue;
      int depth = 0;
      for (int a = pu; a >= 0; a = f.parent[a]) ++depth;
      if (depth + f.height[u] <= 2) continue;
      const SepKey k{f.cc[u] * log(f.vol[pu] / f.vol[u]), f.cid[u], u, u, pu};
      if (sep_less(k, mine)) mine = k;
    }
    const SepKey win = sep_block_min(mine, f.redd, f.redi);
    if (win.s0 == INT_MAX) break;  // every root's height is at most 2
    const int u = win.s0, pu = win.s1;
    for (int c = tid; c < num_nodes; c += T)
      if (c != u && f.alive[c] && f.parent[c] == u) f.parent[c] = pu;
    if (tid == 0) {
      f.cc[pu] += f.cc[u];
      f.alive[u] = 0;
    }
    __syncthreads();
  }

  // ---- labels: components by smallest node; the root's internal children by creation id, then its leaf children
  constexpr int IDS = 2 * SEP_THREADS;  // creation ids and node indices stay below it
  if (has) {
    const int pu = f.parent[tid];
    const bool single = pu < 0 || f.parent[pu] < 0;
    f.keyv[tid] = f.label[tid] * (2 * IDS) + (single ? IDS + tid : f.cid[pu]);
  }
  __syncthreads();
  if (has) {
    int first = 1;
    for (int b = 0; b < tid; ++b) first &= f.keyv[b] != f.keyv[tid];
    f.first[tid] = first;
  }
  __syncthreads();
  if (has) {
    int rank = 0;
    for (int b = 0; b < n; ++b) rank += f.first[b] && f.keyv[b] < f.keyv[tid];
    p.cluster[node] = rank;
  }
  if (tid == 0) {
    int k = 0;
    for (int b = 0; b < n; ++b) k += f.first[b];
    p.counts[g] = k;
  }
}

// exclusive prefix of the per-graph counts (one workgroup walks the graphs in chunks of 256); words[1] = the total
__global__ __launch_bounds__(SEP_THREADS) void sep_offsets_kernel(const int32_t* counts, int32_t* offsets, int G,
                                                                   int32_t* words) {
  __shared__ int sh[SEP_THREADS];
  const int tid = threadIdx.x;
  int carry = 0;
  for (int b0 = 0; b0 < G; b0 += SEP_THREADS) {
    const int i = b0 + tid;
    const int c = i < G ? counts[i] : 0;
    sh[tid] = c;
    __syncthreads();
    for (int off = 1; off < SEP_THREADS; off <<= 1) {
      const int v = tid >= off ? sh[tid - off] : 0;
      __syncthreads();
      sh[tid] += v;
      __syncthreads();
    }
    if (i < G) offsets[i] = carry + sh[tid] - c;
    carry += sh[SEP_THREADS - 1];
    __syncthreads();
  }
  if (tid == 0) words[1] = carry;
}

// a graph without a count was flagged (or is empty): its nodes stay as they are
__global__ void sep_add_offsets_kernel(const int32_t* gid, const int32_t* counts, const int32_t* offsets, int N, int G,
                                       int64_t* cluster) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int g = gid[i];
  if (g < 0 || g >= G || counts[g] <= 0) return;
  cluster[i] += offsets[g];
}

constexpr int64_t I32_MAX = 2147483647;

}  // namespace
}  // namespace tgp

using namespace tgp;

extern "C" int tgp_sep_max_nodes(void) { return sep_max_nodes(); }

extern "C" int tgp_sep_select_f32(const int32_t* src_ptr, const int32_t* src_perm, const int32_t* dst_ptr,
                                  const int32_t* dst_perm, const int64_t* src, const int64_t* dst,
                                  const float* edge_weight, const int32_t* gid, const int32_t* graph_ptr, int64_t N,
                                  int64_t E, int64_t G, int64_t max_n, int64_t* cluster_index, int32_t* counts,
                                  int32_t* offsets, int32_t* words, void* stream) {
  TGP_REQUIRE(N >= 0 && E >= 0 && G >= 0, TGP_ERR_INVALID, "tgp_sep_select_f32: negative size");
  TGP_REQUIRE(max_n >= 1 && max_n <= sep_max_nodes(), TGP_ERR_INVALID, "tgp_sep_select_f32: max_n = %lld outside 1 .. %d",
              static_cast<long long>(max_n), sep_max_nodes());
  TGP_REQUIRE(src_ptr && dst_ptr && gid && graph_ptr && cluster_index && counts && offsets && words, TGP_ERR_INVALID,
              "tgp_sep_select_f32: NULL pointer");
  TGP_REQUIRE(E == 0 || (src && dst), TGP_ERR_INVALID, "tgp_sep_select_f32: NULL edge rows with E > 0");
  TGP_REQUIRE(N <= I32_MAX && E <= I32_MAX && G <= I32_MAX, TGP_ERR_RANGE,
              "tgp_sep_select_f32: N, E or G beyond the int32 index");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(words, 0, 2 * sizeof(int32_t), st) != hipSuccess) return check_launch("tgp_sep_select_f32");
  if (G == 0 || N == 0) return TGP_OK;
  if (hipMemsetAsync(counts, 0, static_cast<size_t>(G) * sizeof(int32_t), st) != hipSuccess)
    return check_launch("tgp_sep_select_f32");
  SepArgs a{src_ptr, src_perm, dst_ptr, dst_perm, src, dst, edge_weight, gid, graph_ptr, static_cast<int>(N),
            static_cast<int>(E), static_cast<int>(G), static_cast<int>(max_n), cluster_index, counts, words,
            sep_lds_layout(static_cast<int>(max_n))};
  if (a.l.total > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(sep_select_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(a.l.total));
  hipLaunchKernelGGL(sep_select_kernel, dim3(static_cast<unsigned>(G)), dim3(SEP_THREADS), a.l.total, st, a);
  int rc = check_launch("tgp_sep_select_f32");
  if (rc != TGP_OK) return rc;
  hipLaunchKernelGGL(sep_offsets_kernel, dim3(1), dim3(SEP_THREADS), 0, st, counts, offsets, static_cast<int>(G), words);
  rc = check_launch("tgp_sep_select_f32 (offsets)");
  if (rc != TGP_OK) return rc;
  hipLaunchKernelGGL(sep_add_offsets_kernel, dim3(static_cast<unsigned>(cdiv(N, 256))), dim3(256), 0, st, gid, counts,
                     offsets, static_cast<int>(N), static_cast<int>(G), cluster_index);
  return check_launch("tgp_sep_select_f32 (add offsets)");
}
