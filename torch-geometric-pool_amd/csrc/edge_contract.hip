// Edge-contraction selection (EdgePool: Diehl 2019, Landolfi 2022; reference select/edge_contraction_select.py): score
// every directed edge entry, take a maximal matching greedily by descending score, contract the matched pairs.
//
// Scores.  The reference's lin(cat(x[row], x[col])) is p1[row] + p2[col] + b with p1 = X w[:F], p2 = X w[F:]: one pass
// over X (ec_project_kernel), two gathered scalars per entry (ec_raw_kernel), no E x 2F matrix.  tanh / sigmoid act per
// entry; the softmax runs over the entries that share a target, through the by-destination inverted index
// (tgp_assign_index_build over col).  Every float sum has ONE order fixed by the index (lane l of a target's group adds
// positions l, l + G, ..., then a fixed butterfly), no float atomics: the scores, and with them the matching, are a pure
// function of the inputs, and a target with one incoming entry scores exactly 1 + add.
//
// Matching (reference maximal_matching, Blelloch's rounds).  An entry's rank is ONE 64-bit key, (prio << 32) | position,
// smaller = earlier; prio is the rank a caller's permutation gives the entry or the bits of its score mapped so that
// unsigned order is DESCENDING score order, so ties go to the lower position (a stable descending argsort) and no sort
// runs.  One round: every live entry (neither endpoint matched yet) offers its key to both endpoints (integer atomic
// min), an entry that finds its own key at both endpoints is matched, its endpoints are marked.  Min is order-independent,
// so the result is a pure function of the inputs.  Two routes, same bits:
//  * ec_graphs_kernel: one workgroup per graph of a sorted batch, node minima / flags / the first entries in LDS,
//    __syncthreads() between the phases of a round, behind the frame of graph_frame.h (which finds and CHECKS the
//    graph's entries, or declines the call through the status word).
//  * device-wide rounds: two launches per round (push; decide + reset of the other minima buffer), one lane per entry,
//    "some entry is still live" is a flag per round that the host reads every few rounds.  No grid-wide barrier, no
//    persistent kernel.
// Both write match [E] (bytes), label [N] (cluster[col[m]] = row[m]: the SOURCE represents the pair) and medge [N] (the
// matched entry of a node, -1 for a singleton); tgp_graclus_relabel_i64 turns the labels into consecutive ids (flags +
// exclusive scan, no sort), ec_weight_kernel hands the matched entry's score to both members.
#include "graph_frame.h"

namespace tgp {

constexpr int EC_GROUP = 8;              // lanes that share one target in the softmax statistics pass
constexpr int EC_HUB_DEGREE = 512;       // targets with more incoming entries get a whole workgroup each
constexpr int EC_HUB_BLOCKS = 256;       // workgroups of the hub pass (each walks the hub queue with this stride)

__device__ __forceinline__ uint32_t ec_prio(const int32_t* __restrict__ rank, const float* __restrict__ score, int64_t e) {
  return rank ? static_cast<uint32_t>(rank[e]) : desc_bits(score[e]);
}

// ------------------------------------------------------------------------------------------------ scores
// p[i] = <x[i,:], w[:F]>, p[n + i] = <x[i,:], w[F:]>.  LPR lanes share a row (a power of two, rows never straddle a
// wave); VEC: 16-byte loads (F, ldx multiples of 4, x and w 16-byte aligned).
template <bool VEC>
__global__ __launch_bounds__(256) void ec_project_kernel(const float* __restrict__ x, int64_t n, int F, int64_t ldx,
                                                         const float* __restrict__ w, int lpr, float* __restrict__ p) {
  const int rows_per_block = 256 / lpr;
  const int sub = threadIdx.x % lpr;
  for (int64_t i0 = static_cast<int64_t>(blockIdx.x) * rows_per_block; i0 < n;
       i0 += static_cast<int64_t>(gridDim.x) * rows_per_block) {
    const int64_t i = i0 + threadIdx.x / lpr;
    float a1 = 0.0f, a2 = 0.0f;
    if (i < n) {
      const float* xr = x + i * ldx;
      if (VEC) {
        for (int c = sub * 4; c < F; c += lpr * 4) {
          const float4 v = *reinterpret_cast<const float4*>(xr + c);
          const float4 u1 = *reinterpret_cast<const float4*>(w + c);
          const float4 u2 = *reinterpret_cast<const float4*>(w + F + c);
          a1 = a1 + v.x * u1.x;
          a1 = a1 + v.y * u1.y;
          a1 = a1 + v.z * u1.z;
          a1 = a1 + v.w * u1.w;
          a2 = a2 + v.x * u2.x;
          a2 = a2 + v.y * u2.y;
          a2 = a2 + v.z * u2.z;
          a2 = a2 + v.w * u2.w;
        }
      } else {
        for (int c = sub; c < F; c += lpr) {
          const float v = xr[c];
          a1 = a1 + v * w[c];
          a2 = a2 + v * w[F + c];
        }
      }
    }
    // the order of wave_butterfly at a run-time group width (uniform trip count: every lane of the wave takes part)
    for (int m = lpr >> 1; m >= 1; m >>= 1) {
      a1 = a1 + __shfl_xor(a1, m);
      a2 = a2 + __shfl_xor(a2, m);
    }
    if (i < n && sub == 0) {
      p[i] = a1;
      p[n + i] = a2;
    }
  }
}

__global__ __launch_bounds__(256) void ec_raw_kernel(const int64_t* __restrict__ row, const int64_t* __restrict__ col,
                                                     int64_t E, int64_t n, const float* __restrict__ p,
                                                     const float* __restrict__ bias, float* __restrict__ raw) {
  const float b = bias ? bias[0] : 0.0f;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; e < E; e += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t r = row[e], c = col[e];
    if (static_cast<uint64_t>(r) >= static_cast<uint64_t>(n) || static_cast<uint64_t>(c) >= static_cast<uint64_t>(n)) {
      raw[e] = 0.0f;  // (an entry that leaves the graph never matches: the matching kernels skip it)
      continue;
    }
    raw[e] = (p[r] + p[n + c]) + b;
  }
}

// method 1: tanh, 2: sigmoid
__global__ __launch_bounds__(256) void ec_pointwise_kernel(const float* __restrict__ raw, int64_t E, int method, float add,
                                                           float* __restrict__ out) {
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; e < E; e += static_cast<int64_t>(gridDim.x) * 256) {
    const float v = raw[e];
    const float f = method == 1 ? tanhf(v) : 1.0f / (1.0f + expf(-v));
    out[e] = f + add;
  }
}

// Softmax statistics of the targets with at most EC_HUB_DEGREE entries: EC_GROUP lanes per target, lane l takes the
// positions l, l + EC_GROUP, ... of the target's group in index order, then a fixed butterfly.  Longer groups are queued
// (hubs[0] = count, hubs[1 + q] = target) for ec_softmax_hub_kernel.
__global__ __launch_bounds__(256) void ec_softmax_stats_kernel(const float* __restrict__ raw,
                                                               const int32_t* __restrict__ grp_ptr,
                                                               const int32_t* __restrict__ grp_perm, int64_t n,
                                                               float2* __restrict__ seg, int32_t* __restrict__ hubs,
                                                               int hub_cap) {
  const int sub = threadIdx.x % EC_GROUP;
  const int64_t c = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) / EC_GROUP;
  const bool live = c < n;
  const int32_t b = live ? grp_ptr[c] : 0, e = live ? grp_ptr[c + 1] : 0;
  const bool hub = e - b > EC_HUB_DEGREE;
  const bool first = !hub && b + sub < e;
  const float v0 = first ? raw[grp_perm[b + sub]] : -INFINITY;  // (most targets have one entry per lane at most)
  float mx = v0, sum = 0.0f;
  if (!hub) {
    for (int32_t j = b + sub + EC_GROUP; j < e; j += EC_GROUP) mx = fmaxf(mx, raw[grp_perm[j]]);
  }
  mx = wave_max<EC_GROUP>(mx);
  if (first) sum = expf(v0 - mx);
  if (!hub) {
    for (int32_t j = b + sub + EC_GROUP; j < e; j += EC_GROUP) sum = sum + expf(raw[grp_perm[j]] - mx);
  }
  sum = wave_sum<EC_GROUP>(sum);
  if (!live || sub != 0) return;
  if (hub) {
    const int q = atomicAdd(hubs, 1);
    if (q < hub_cap) hubs[1 + q] = static_cast<int32_t>(c);
    return;
  }
  seg[c] = make_float2(mx, sum);
}

// One workgroup per queued hub: thread t takes positions t, t + 1024, ..., then a fixed tree in LDS.  The order in
// which the hubs were queued decides which workgroup serves which hub, never a value.
__global__ __launch_bounds__(1024) void ec_softmax_hub_kernel(const float* __restrict__ raw,
                                                              const int32_t* __restrict__ grp_ptr,
                                                              const int32_t* __restrict__ grp_perm,
                                                              float2* __restrict__ seg,
                                                              const int32_t* __restrict__ hubs, int hub_cap) {
  __shared__ float s_red[1024];
  const int tid = threadIdx.x;
  int count = hubs[0];
  if (count > hub_cap) count = hub_cap;
  for (int q = blockIdx.x; q < count; q += gridDim.x) {
    const int32_t c = hubs[1 + q];
    const int32_t b = grp_ptr[c], e = grp_ptr[c + 1];
    float mx = -INFINITY;
    for (int32_t j = b + tid; j < e; j += 1024) mx = fmaxf(mx, raw[grp_perm[j]]);
    s_red[tid] = mx;
    __syncthreads();
    for (int d = 512; d >= 1; d >>= 1) {
      if (tid < d) s_red[tid] = fmaxf(s_red[tid], s_red[tid + d]);
      __syncthreads();
    }
    mx = s_red[0];
    __syncthreads();
    float sum = 0.0f;
    for (int32_t j = b + tid; j < e; j += 1024) sum = sum + expf(raw[grp_perm[j]] - mx);
    s_red[tid] = sum;
    __syncthreads();
    for (int d = 512; d >= 1; d >>= 1) {
      if (tid < d) s_red[tid] = s_red[tid] + s_red[tid + d];
      __syncthreads();
    }
    if (tid == 0) seg[c] = make_float2(mx, s_red[0]);
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void ec_softmax_apply_kernel(const float* __restrict__ raw,
                                                               const int64_t* __restrict__ col, int64_t E, int64_t n,
                                                               const float2* __restrict__ seg, float add,
                                                               float* __restrict__ out) {
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; e < E; e += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t c = col[e];
    if (static_cast<uint64_t>(c) >= static_cast<uint64_t>(n)) {
      out[e] = add;
      continue;
    }
    const float2 ms = seg[c];  // {maximum, sum} of the target: one gathered 8-byte load
    out[e] = expf(raw[e] - ms.x) / ms.y + add;
  }
}

// ------------------------------------------------------------------------------------------------ per-graph route
struct EcGraphArgs {
  const int64_t* row;
  const int64_t* col;
  int64_t E, N;
  const int64_t* gptr;
  const float* score;
  const int32_t* rank;
  uint8_t* match;
  int64_t* label;
  int64_t* medge;
  int32_t* words;  // [0] status: 0 = done, bit 0 = declined (input), bit 1 = round bound hit; [1] rounds (max over graphs)
  int nmax, ecap;
};

__global__ __launch_bounds__(1024) void ec_graphs_kernel(EcGraphArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long ec_lds[];
  unsigned long long* s_min = ec_lds;
  uint32_t* s_edge = reinterpret_cast<uint32_t*>(s_min + p.nmax);
  uint32_t* s_prio = s_edge + p.ecap;
  uint8_t* s_m = reinterpret_cast<uint8_t*>(s_prio + p.ecap);

  GraphFrame f;
  if (!graph_frame_open(p.row, p.col, p.E, p.N, p.gptr, p.nmax, p.ecap, s_edge, p.words, f,
                        [&](int64_t e, int64_t pos) { s_prio[e] = ec_prio(p.rank, p.score, pos); }))
    return;  // (uniform)
  const int T = blockDim.x, tid = threadIdx.x;
  const int n = f.n;
  const int64_t n0 = f.n0, lo = f.lo, ne = f.ne;
  // a graph that declined leaves label / medge unwritten: they are meaningless on a declined call, and
  // tgp_edge_contract_rounds_start sets both again.  The first barrier of the round loop orders s_m before its reads.
  for (int i = tid; i < n; i += T) {
    s_m[i] = 0;
    p.label[n0 + i] = n0 + i;
    p.medge[n0 + i] = -1;
  }
  auto entry_at = [&](int64_t e, int& r, int& c) -> unsigned long long {
    if (f.cached(e)) {
      f.cached_edge(e, r, c);
      return make_key(s_prio[e], e);
    }
    f.listed_edge(e, r, c);
    return make_key(ec_prio(p.rank, p.score, lo + e), e);
  };

  // ---- rounds: each matches at least one entry (the live entry with the smallest key) and thereby retires at least one
  // node, so n rounds is a hard cap
  bool finished = false;
  int round = 0;
  for (; round <= n; ++round) {
    for (int i = tid; i < n; i += T) s_min[i] = KEY_INF;
    __syncthreads();
    int open = 0;
    for (int64_t e = tid; e < ne; e += T) {
      int r, c;
      const unsigned long long key = entry_at(e, r, c);
      if (s_m[r] || s_m[c]) continue;
      open = 1;
      atomicMin(&s_min[r], key);
      if (c != r) atomicMin(&s_min[c], key);
    }
    if (!__syncthreads_or(open)) {
      finished = true;
      break;
    }
    for (int64_t e = tid; e < ne; e += T) {
      int r, c;
      const unsigned long long key = entry_at(e, r, c);
      if (s_min[r] == key && s_min[c] == key) {  // (keys are unique: only the live entry that pushed it finds its key)
        p.match[lo + e] = 1;
        s_m[r] = 1;
        s_m[c] = 1;
        p.label[n0 + c] = n0 + r;
        p.medge[n0 + r] = lo + e;
        p.medge[n0 + c] = lo + e;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (!finished) atomicOr(p.words, 2);
    atomicMax(p.words + 1, round);
  }
}

// ------------------------------------------------------------------------------------------------ device-wide route
__global__ __launch_bounds__(256) void ec_init_kernel(int64_t n, int64_t* __restrict__ label, int64_t* __restrict__ medge) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  label[i] = i;
  medge[i] = -1;
}

// every live entry offers its key to both endpoints
__global__ __launch_bounds__(256) void ec_push_kernel(const int64_t* __restrict__ row, const int64_t* __restrict__ col,
                                                      int64_t E, int64_t n, const int32_t* __restrict__ rank,
                                                      const float* __restrict__ score,
                                                      const uint8_t* __restrict__ matched, unsigned long long* nmin,
                                                      const int32_t* __restrict__ prev_flag, int32_t* open_flag) {
  // the round before (of this call) met no live entry: none can be live now, and nothing is streamed
  if (prev_flag && *prev_flag == 0) return;
  const int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= E) return;
  const int64_t r = row[e], c = col[e];
  if (static_cast<uint64_t>(r) >= static_cast<uint64_t>(n) || static_cast<uint64_t>(c) >= static_cast<uint64_t>(n)) return;
  if (matched[r] || matched[c]) return;
  *open_flag = 1;
  const unsigned long long key = make_key(ec_prio(rank, score, e), e);
  // a minimum only ever decreases during the launch: a key that is not below what a plain load sees cannot win
  if (key < __hip_atomic_load(&nmin[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&nmin[r], key);
  if (c != r && key < __hip_atomic_load(&nmin[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&nmin[c], key);
}

// Items [0, E): an entry that finds its own key at both endpoints is matched.  Items [E, E + N): reset the minima the
// NEXT round pushes into (the buffer of the round before this one).
__global__ __launch_bounds__(256) void ec_decide_kernel(const int64_t* __restrict__ row, const int64_t* __restrict__ col,
                                                        int64_t E, int64_t n, const int32_t* __restrict__ rank,
                                                        const float* __restrict__ score,
                                                        const unsigned long long* __restrict__ nmin,
                                                        unsigned long long* __restrict__ next_min,
                                                        uint8_t* __restrict__ matched, uint8_t* __restrict__ match,
                                                        int64_t* __restrict__ label, int64_t* __restrict__ medge,
                                                        const int32_t* __restrict__ open_flag) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (idx < E) {
    if (*open_flag == 0) return;  // nothing was pushed this round: nothing to decide
    const int64_t r = row[idx], c = col[idx];
    if (static_cast<uint64_t>(r) >= static_cast<uint64_t>(n) || static_cast<uint64_t>(c) >= static_cast<uint64_t>(n)) return;
    const unsigned long long vr = nmin[r];
    if (vr == KEY_INF || (vr & 0xFFFFFFFFull) != static_cast<unsigned long long>(idx)) return;  // (the low word names the entry)
    const unsigned long long key = make_key(ec_prio(rank, score, idx), idx);
    if (vr == key && nmin[c] == key) {
      match[idx] = 1;
      matched[r] = 1;
      matched[c] = 1;
      label[c] = r;
      medge[r] = idx;
      medge[c] = idx;
    }
  } else if (idx < E + n) {
    next_min[idx - E] = KEY_INF;
  }
}

// weight[i] = the score of the entry that matched i, 1 for a singleton (reference :227-236: the pair's score goes to both
// members through new_edge_score[cluster])
__global__ __launch_bounds__(256) void ec_weight_kernel(const int64_t* __restrict__ medge, const float* __restrict__ score,
                                                        int64_t n, int64_t E, float* __restrict__ weight) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t m = medge[i];
  weight[i] = (m >= 0 && m < E) ? score[m] : 1.0f;
}

struct EcWs {
  unsigned long long* nmin[2];
  uint8_t* matched;
};
static EcWs ec_carve(void* ws, int64_t n) {
  Carver cv(ws);
  EcWs w;
  w.nmin[0] = cv.take<unsigned long long>(n);
  w.nmin[1] = cv.take<unsigned long long>(n);
  w.matched = cv.take<uint8_t>(n);
  return w;
}

static int ec_grid(int64_t items) {  // grid-stride kernels: enough workgroups to fill the chip, no more
  const int64_t b = (items + 255) / 256;
  return static_cast<int>(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

static bool ec_sizes_ok(int64_t N, int64_t E) { return N >= 0 && E >= 0 && N < (1ll << 31); }

}  // namespace tgp

using namespace tgp;

extern "C" int tgp_edge_contract_max_graph_nodes(void) { return FRAME_GRAPH_MAX; }
extern "C" int tgp_edge_contract_edge_cache(void) { return FRAME_EDGE_CACHE_MAX; }
extern "C" int tgp_edge_contract_hub_degree(void) { return EC_HUB_DEGREE; }

extern "C" size_t tgp_edge_contract_workspace_bytes(int64_t num_nodes) {
  const size_t n = static_cast<size_t>(num_nodes > 0 ? num_nodes : 1);
  return 2 * align_up(n * sizeof(unsigned long long)) + align_up(n) + 256;
}

// p [2 N]: p[i] = <x[i,:], w[:F]>, p[N + i] = <x[i,:], w[F:]> (w [2 F] = the weight row of Linear(2 F, 1)); one pass over x
extern "C" int tgp_edge_contract_project_f32(const float* x, int64_t N, int64_t F, int64_t ldx, const float* w, float* p,
                                             void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(N >= 0 && F >= 0 && F < (1ll << 30) && ldx >= F, TGP_ERR_INVALID, "tgp_edge_contract_project_f32: bad argument");
  if (N == 0) return TGP_OK;
  TGP_REQUIRE(p && (F == 0 || (x && w)), TGP_ERR_INVALID, "tgp_edge_contract_project_f32: null pointer");
  const bool vec = F > 0 && F % 4 == 0 && ldx % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(w) % 16 == 0;
  const int64_t per_lane = vec ? (F + 3) / 4 : F;
  int lpr = 1;
  while (lpr < 64 && lpr < per_lane) lpr <<= 1;
  const int rows_per_block = 256 / lpr;
  const int64_t blocks = (N + rows_per_block - 1) / rows_per_block;
  const dim3 grid(static_cast<unsigned>(blocks > 16384 ? 16384 : blocks));
  if (vec)
    hipLaunchKernelGGL(ec_project_kernel<true>, grid, dim3(256), 0, stream, x, N, static_cast<int>(F), ldx, w, lpr, p);
  else
    hipLaunchKernelGGL(ec_project_kernel<false>, grid, dim3(256), 0, stream, x, N, static_cast<int>(F), ldx, w, lpr, p);
  return check_launch("tgp_edge_contract_project_f32");
}

// raw[e] = p[row[e]] + p[N + col[e]] + bias[0] (bias on the device, null = 0); an entry with an endpoint outside [0, N)
// gets 0.
extern "C" int tgp_edge_contract_raw_f32(const int64_t* row, const int64_t* col, int64_t E, int64_t N, const float* p,
                                         const float* bias, float* raw, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(ec_sizes_ok(N, E), TGP_ERR_INVALID, "tgp_edge_contract_raw_f32: bad argument");
  TGP_REQUIRE(E < (1ll << 32), TGP_ERR_RANGE, "tgp_edge_contract_raw_f32: %lld entries exceed the 32-bit entry positions",
              static_cast<long long>(E));
  if (E == 0) return TGP_OK;
  TGP_REQUIRE(row && col && p && raw, TGP_ERR_INVALID, "tgp_edge_contract_raw_f32: null pointer");
  hipLaunchKernelGGL(ec_raw_kernel, dim3(ec_grid(E)), dim3(256), 0, stream, row, col, E, N, p, bias, raw);
  return check_launch("tgp_edge_contract_raw_f32");
}

// out[e] = f(raw)[e] + add.  method 0: softmax over the entries that share col[e] (grp_ptr [N + 1], grp_perm [E]: the
// by-destination index of tgp_assign_index_build over col; seg [2 N] fp32 scratch, 8-byte aligned, that leaves with each
// target's {maximum, sum} pair; hubs [hub_cap + 1] int32 scratch, hub_cap >= E / tgp_edge_contract_hub_degree()); 1: tanh; 2: sigmoid (the
// index, seg and hubs are not read).  raw and out are different arrays.
extern "C" int tgp_edge_contract_normalize_f32(const float* raw, const int64_t* col, int64_t E, int64_t N, int method,
                                               float add, const int32_t* grp_ptr, const int32_t* grp_perm, float* seg,
                                               int32_t* hubs, int64_t hub_cap, float* out, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(ec_sizes_ok(N, E) && method >= 0 && method <= 2, TGP_ERR_INVALID,
              "tgp_edge_contract_normalize_f32: bad argument");
  if (E == 0) return TGP_OK;
  TGP_REQUIRE(raw && out && raw != out, TGP_ERR_INVALID, "tgp_edge_contract_normalize_f32: null pointer / raw == out");
  if (method != 0) {
    hipLaunchKernelGGL(ec_pointwise_kernel, dim3(ec_grid(E)), dim3(256), 0, stream, raw, E, method, add, out);
    return check_launch("tgp_edge_contract_normalize_f32");
  }
  TGP_REQUIRE(E < (1ll << 31), TGP_ERR_RANGE, "tgp_edge_contract_normalize_f32: the by-destination index is 32-bit");
  TGP_REQUIRE(col && grp_ptr && grp_perm && seg && hubs, TGP_ERR_INVALID,
              "tgp_edge_contract_normalize_f32: null pointer");
  TGP_REQUIRE(hub_cap >= E / EC_HUB_DEGREE && hub_cap < (1ll << 31), TGP_ERR_WORKSPACE,
              "tgp_edge_contract_normalize_f32: hub queue too small");
  (void)hipMemsetAsync(hubs, 0, sizeof(int32_t), stream);
  float2* seg2 = reinterpret_cast<float2*>(seg);
  hipLaunchKernelGGL(ec_softmax_stats_kernel, dim3(cdiv(N * EC_GROUP, 256)), dim3(256), 0, stream, raw, grp_ptr, grp_perm,
                     N, seg2, hubs, static_cast<int>(hub_cap));
  if (E > EC_HUB_DEGREE)  // (no target can be a hub otherwise)
    hipLaunchKernelGGL(ec_softmax_hub_kernel, dim3(EC_HUB_BLOCKS), dim3(1024), 0, stream, raw, grp_ptr, grp_perm, seg2,
                       hubs, static_cast<int>(hub_cap));
  hipLaunchKernelGGL(ec_softmax_apply_kernel, dim3(ec_grid(E)), dim3(256), 0, stream, raw, col, E, N, seg2, add,
                     out);
  return check_launch("tgp_edge_contract_normalize_f32");
}

// The matching of a sorted batch whose longest graph has at most max_graph_nodes (<= tgp_edge_contract_max_graph_nodes())
// nodes, one workgroup per graph, one launch.  Priorities: rank [E] int32 (an entry's rank in the caller's permutation),
// else score [E] (descending, ties to the lower position).  match [E] bytes, label [N], medge [N] as described above;
// words[0] = 0 when every graph was done (else declined: label / match are meaningless), words[1] = rounds of the
// slowest graph.
extern "C" int tgp_edge_contract_graphs(const int64_t* row, const int64_t* col, int64_t E, int64_t N,
                                        const int64_t* graph_ptr, int64_t B, int max_graph_nodes, const float* score,
                                        const int32_t* rank, uint8_t* match, int64_t* label, int64_t* medge,
                                        int32_t* words, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(ec_sizes_ok(N, E) && B >= 0 && B < (1ll << 31), TGP_ERR_INVALID, "tgp_edge_contract_graphs: bad argument");
  TGP_REQUIRE(E < (1ll << 32), TGP_ERR_RANGE, "tgp_edge_contract_graphs: %lld entries exceed the 32-bit entry positions",
              static_cast<long long>(E));
  TGP_REQUIRE(max_graph_nodes >= 1 && max_graph_nodes <= FRAME_GRAPH_MAX, TGP_ERR_RANGE,
              "tgp_edge_contract_graphs: a graph of %d nodes does not fit one workgroup (max %d)", max_graph_nodes,
              FRAME_GRAPH_MAX);
  TGP_REQUIRE(words && graph_ptr && (N == 0 || (label && medge)) && (E == 0 || (row && col && match && (rank || score))),
              TGP_ERR_INVALID, "tgp_edge_contract_graphs: null pointer");
  (void)hipMemsetAsync(words, 0, 2 * sizeof(int32_t), stream);
  if (E > 0) (void)hipMemsetAsync(match, 0, static_cast<size_t>(E), stream);
  if (B == 0 || N == 0) return check_launch("tgp_edge_contract_graphs");
  EcGraphArgs p;
  p.row = row; p.col = col; p.E = E; p.N = N; p.gptr = graph_ptr; p.score = score; p.rank = rank;
  p.match = match; p.label = label; p.medge = medge; p.words = words;
  const FrameGeometry geo = graph_frame_geometry(max_graph_nodes);
  p.nmax = geo.nmax; p.ecap = geo.ecap;
  const size_t lds = static_cast<size_t>(p.nmax) * (sizeof(unsigned long long) + 1) + static_cast<size_t>(p.ecap) * 8;
  hipLaunchKernelGGL(ec_graphs_kernel, dim3(static_cast<unsigned>(B)), dim3(geo.threads), lds, stream, p);
  return check_launch("tgp_edge_contract_graphs");
}

// Device-wide route, step 0: cleared state (ws of tgp_edge_contract_workspace_bytes(N)), label[i] = i, medge[i] = -1,
// match cleared.
extern "C" int tgp_edge_contract_rounds_start(int64_t N, int64_t E, void* ws, size_t ws_bytes, uint8_t* match,
                                              int64_t* label, int64_t* medge, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(ec_sizes_ok(N, E), TGP_ERR_INVALID, "tgp_edge_contract_rounds_start: bad argument");
  TGP_REQUIRE(E < (1ll << 32), TGP_ERR_RANGE,
              "tgp_edge_contract_rounds_start: %lld entries exceed the 32-bit entry positions", static_cast<long long>(E));
  TGP_REQUIRE(E == 0 || match, TGP_ERR_INVALID, "tgp_edge_contract_rounds_start: null pointer");
  if (E > 0) (void)hipMemsetAsync(match, 0, static_cast<size_t>(E), stream);
  if (N == 0) return check_launch("tgp_edge_contract_rounds_start");
  TGP_REQUIRE(label && medge, TGP_ERR_INVALID, "tgp_edge_contract_rounds_start: null pointer");
  TGP_REQUIRE(ws && ws_bytes >= tgp_edge_contract_workspace_bytes(N), TGP_ERR_WORKSPACE,
              "tgp_edge_contract_rounds_start: workspace too small");
  EcWs w = ec_carve(ws, N);
  (void)hipMemsetAsync(w.nmin[0], 0xFF, static_cast<size_t>(N) * sizeof(unsigned long long), stream);
  (void)hipMemsetAsync(w.nmin[1], 0xFF, static_cast<size_t>(N) * sizeof(unsigned long long), stream);
  (void)hipMemsetAsync(w.matched, 0, static_cast<size_t>(N), stream);
  hipLaunchKernelGGL(ec_init_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, N, label, medge);
  return check_launch("tgp_edge_contract_rounds_start");
}

// `rounds` rounds, numbered from `round_base` (rounds launched since tgp_edge_contract_rounds_start: the two minima
// buffers alternate).  open_flags[j] = 1 when round j met a live entry; a round that meets none changes nothing, so
// launching more rounds than needed is harmless, and the rounds of a call that follow such a round leave without
// reading the edge list.  Two launches per round.
extern "C" int tgp_edge_contract_rounds(const int64_t* row, const int64_t* col, int64_t E, int64_t N, const float* score,
                                        const int32_t* rank, void* ws, int64_t round_base, int rounds,
                                        int32_t* open_flags, uint8_t* match, int64_t* label, int64_t* medge,
                                        void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(ec_sizes_ok(N, E) && rounds >= 0 && round_base >= 0 && open_flags, TGP_ERR_INVALID,
              "tgp_edge_contract_rounds: bad argument");
  TGP_REQUIRE(E < (1ll << 32), TGP_ERR_RANGE, "tgp_edge_contract_rounds: %lld entries exceed the 32-bit entry positions",
              static_cast<long long>(E));
  (void)hipMemsetAsync(open_flags, 0, sizeof(int32_t) * static_cast<size_t>(rounds > 0 ? rounds : 1), stream);
  if (N == 0 || E == 0 || rounds == 0) return check_launch("tgp_edge_contract_rounds");
  TGP_REQUIRE(row && col && ws && match && label && medge && (rank || score), TGP_ERR_INVALID,
              "tgp_edge_contract_rounds: null pointer");
  EcWs w = ec_carve(ws, N);
  const dim3 block(256);
  for (int j = 0; j < rounds; ++j) {
    const int64_t t = round_base + j;
    unsigned long long *cur = w.nmin[t % 2], *nxt = w.nmin[(t + 1) % 2];
    hipLaunchKernelGGL(ec_push_kernel, dim3(cdiv(E, 256)), block, 0, stream, row, col, E, N, rank, score, w.matched, cur,
                       j > 0 ? open_flags + j - 1 : static_cast<const int32_t*>(nullptr), open_flags + j);
    hipLaunchKernelGGL(ec_decide_kernel, dim3(cdiv(E + N, 256)), block, 0, stream, row, col, E, N, rank, score, cur, nxt,
                       w.matched, match, label, medge, open_flags + j);
  }
  return check_launch("tgp_edge_contract_rounds");
}

// weight[i] = score[medge[i]] for a matched node, 1 for a singleton
extern "C" int tgp_edge_contract_weights_f32(const int64_t* medge, const float* score, int64_t N, int64_t E, float* weight,
                                             void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(ec_sizes_ok(N, E), TGP_ERR_INVALID, "tgp_edge_contract_weights_f32: bad argument");
  if (N == 0) return TGP_OK;
  TGP_REQUIRE(medge && weight && (E == 0 || score), TGP_ERR_INVALID, "tgp_edge_contract_weights_f32: null pointer");
  hipLaunchKernelGGL(ec_weight_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, medge, score, N, E, weight);
  return check_launch("tgp_edge_contract_weights_f32");
}
