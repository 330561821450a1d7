// NMF pooling for graphs past the LDS limit of csrc/nmf.hip: the same coordinate descent (scikit-learn's solver "cd",
// shuffle off, no regularisation; S = softmax(H^T)), the same special cases, default init and stopping rule -- without a
// dense adjacency.
//
// One workgroup of 1024 threads per LISTED graph.  A row of A is the node's by-source edge group, a row of A^T its
// by-destination group, an entry is clamp_min(w_e, 0).  That is the dense matrix only for a COALESCED list: every
// by-source group strictly ascending in destination, every by-destination group strictly ascending in source, the graph's
// nodes one run of consecutive indices.  The workgroup checks this first and declines (TGP_NMF_NOT_COALESCED, graph
// unwritten) otherwise.  Then a row walk in ascending entry order adds the terms of the dense walk in the same order: the terms it
// skips are exact zeros.
//   factors:     W and H^T [n, K] live in LDS (odd row stride) when 2 n (K | 1) floats fit behind the fixed part of the
//                frame, else in the graph's rows of w_out / ht_out in HBM (one workgroup, __syncthreads(): workgroup-scope
//                visibility).  The choice is uniform per workgroup; the code is one template over the home.
//   half-sweep:  Gram = F^T F on the matrix cores (v_mfma_f32_32x32x2_f32, columns >= K fed as zeros): the 16 waves take
//                contiguous row slices, their 32 x 32 partial tiles are added in ascending wave order through four LDS
//                slots, thread t * 32 + r owning Gram[t, r].  Then the thread that owns row i (rows tid, tid + 1024, ..)
//                forms P[i, 0..K) in registers over the row's entries, F[j, 0..K) read per entry, and runs the K dependent
//                coordinate updates with u in registers.  There is no A buffer and no P buffer.
//   order:       ascending entry, ascending r, fp32, no fused multiply-add (-ffp-contract=off), no float atomics: the
//                same bits on every call.  The violations: a thread's rows ascending, the xor butterfly of a wave, the
//                16 waves ascending (block_fold_seq).
//   leaving:     thread 0 writes the decision into one LDS word that every wave reads behind a barrier; max_iter caps the
//                loop whatever the violations are.
#include "common.h"

#include <float.h>

#include <type_traits>

namespace tgp {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int NR_THREADS = 1024;
constexpr int NR_WAVES = NR_THREADS / 64;
constexpr int NR_TILE = 32;           // the MFMA tile: K <= 32
constexpr int NR_SLOTS = 4;           // partial Gram tiles in flight during the fold
constexpr int NR_LDS_BYTES = 160 * 1024;

// the LDS frame in floats: the fixed part, then W [n, K | 1] and H^T [n, K | 1]
constexpr int NR_GRAM = 0;                                        // [32][32]
constexpr int NR_SCRATCH = NR_GRAM + NR_TILE * NR_TILE;           // [NR_SLOTS][32][32]
constexpr int NR_RED = NR_SCRATCH + NR_SLOTS * NR_TILE * NR_TILE; // [NR_WAVES] wave partials of a block fold
constexpr int NR_CTL = NR_RED + NR_WAVES;                         // 4 words
constexpr int NR_FACTORS = NR_CTL + 4;

// (the status bits: enum tgp_nmf_status of tgp_hip.h, shared with csrc/nmf.hip)

inline int rows_lds_nodes(int K) { return (NR_LDS_BYTES / 4 - NR_FACTORS) / (2 * (K | 1)); }

// csrc/nmf.hip's nmf_uniform
__device__ __forceinline__ float rows_uniform(uint32_t seed, uint32_t which, uint32_t i, uint32_t t) {
  uint32_t h = seed * 0x9E3779B9u + which * 0x85EBCA6Bu + i * 0xC2B2AE35u + t * 0x27D4EB2Fu + 0x165667B1u;
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return static_cast<float>((h >> 8) + 1u) * (1.0f / 16777216.0f);
}

// row of the 32 x 32 MFMA result that accumulator register q of a lane in half h (lane >> 5) holds
__device__ __forceinline__ int rows_acc_row(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

struct RowsArgs {
  const int32_t* sptr;        // [N + 1] by-source offsets
  const int32_t* sperm;       // [E] edge positions by source (NULL: grouped already)
  const int64_t* dst;         // [E]
  const int32_t* dptr;        // [N + 1] by-destination offsets
  const int32_t* dperm;       // [E] or NULL
  const int64_t* src;         // [E]
  const float* w;             // [E] or NULL
  const int32_t* gid;         // [N]
  const int32_t* graph_ptr;   // [G + 1]
  const int32_t* graph_perm;  // [N]
  const int32_t* list;        // [L] the graphs to run
  int N, E, G, K, out_cols, max_iter, home, lds_nodes;
  float tol;
  uint32_t seed;
  const float* w0;
  const float* h0t;
  float* s;
  float* w_out;
  float* ht_out;
  int32_t* iters;
  float* ratio;
  int32_t* status;
};

// One group of `node` checked entry by entry: positions and far ends in range and inside the graph's run
// [base, base + n), the near end `own` equal to the node, far ends strictly ascending; `sum` (when wanted) gets the
// clamped entries in order.  Returns status bits.  Nothing out of range is read.
template <bool SUM>
__device__ __forceinline__ int rows_check_group(const int32_t* ptr, const int32_t* perm, const int64_t* other,
                                                const int64_t* own, const float* w, int node, int base, int n, int E,
                                                float& sum) {
  const int e0 = ptr[node], e1 = ptr[node + 1];
  if (e0 < 0 || e1 < e0 || e1 > E) return TGP_NMF_BAD_INPUT;
  int flags = 0;
  int64_t prev = -1;
  for (int e = e0; e < e1; ++e) {
    const int pos = perm ? perm[e] : e;
    if (pos < 0 || pos >= E) {
      flags |= TGP_NMF_BAD_INPUT;
      continue;
    }
    const int64_t j = other[pos];
    if (j < base || j >= static_cast<int64_t>(base) + n || own[pos] != node) {  // (an edge that leaves the graph)
      flags |= TGP_NMF_BAD_INPUT;
      continue;
    }
    if (j <= prev) flags |= TGP_NMF_NOT_COALESCED;
    prev = j;
    if (SUM) {
      const float v = clamp_min(w ? w[pos] : 1.0f, 0.0f);
      if (!(v <= FLT_MAX)) flags |= TGP_NMF_NON_FINITE;
      sum += v;
    }
  }
  return flags;
}

// Gram [32][32] = F^T F over the n rows of F (row stride ld, columns >= ka read as zeros).  Wave w multiplies the rows
// [w rpw, (w + 1) rpw) two per MFMA (A[i][k] = B[k][i] = F[row + k][i]: one operand register serves both sides; a row
// past the slice is fed as zero); the partial tiles are added in ascending wave order, four waves per round.  Ends
// behind a barrier.
template <typename IdxT>
__device__ __forceinline__ void rows_gram(const float* F, int ld, int n, int ka, float* smem, int tid) {
  const int lane = tid & 63, wave = tid >> 6, lm = lane & 31, h = lane >> 5;
  const int64_t rpw = ((static_cast<int64_t>(n) + NR_WAVES - 1) / NR_WAVES + 1) & ~static_cast<int64_t>(1);
  const int64_t lo = wave * rpw, hi = lo + rpw;
  const int r0 = static_cast<int>(lo < n ? lo : n), r1 = static_cast<int>(hi < n ? hi : n);
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
  for (int r = r0; r < r1; r += 2) {
    const int row = r + h;
    const float v = (row < r1 && lm < ka) ? F[static_cast<IdxT>(row) * ld + lm] : 0.0f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v, v, acc, 0, 0, 0);
  }
  float* const scratch = smem + NR_SCRATCH;
  const int busy = static_cast<int>((n + rpw - 1) / rpw);     // waves with rows; the tiles behind them are zeros
  const int rounds = (busy + NR_SLOTS - 1) / NR_SLOTS;        // (adding a zero tile changes no bit: skipped)
  float sum = 0.0f;
  for (int round = 0; round < rounds; ++round) {
    if (wave / NR_SLOTS == round) {
      float* const slot = scratch + (wave % NR_SLOTS) * NR_TILE * NR_TILE;
#pragma unroll
      for (int q = 0; q < 16; ++q) slot[rows_acc_row(q, h) * NR_TILE + lm] = acc[q];
    }
    __syncthreads();
#pragma unroll
    for (int sl = 0; sl < NR_SLOTS; ++sl) sum += scratch[sl * NR_TILE * NR_TILE + tid];
    __syncthreads();
  }
  smem[NR_GRAM + tid] = sum;
  __syncthreads();
}

// The uniform column count, opaque to the compiler: the KC comparisons against it are made where they are used and not
// kept, one scalar register pair each, across the loops around them.
__device__ __forceinline__ int rows_fresh(int ka) {
  asm volatile("" : "+s"(ka));
  return ka;
}

// One half-sweep over the rows this thread owns: P[i, :] = sum over the row's entries of a_ij F[j, :] in registers
// (four entries' indices and values loaded ahead of their use), then scikit-learn's _update_cdnmf_fast for the row.
// Returns the thread's violation, its rows in ascending order.
template <typename IdxT, int KC>
__device__ __forceinline__ float rows_sweep(const int32_t* ptr, const int32_t* perm, const int64_t* other,
                                            const float* w, float* U, const float* F, int ld, const float* Gm, int base,
                                            int n, int ka, int tid) {
  float viol = 0.0f;
  for (int i = tid; i < n; i += NR_THREADS) {
    const int node = base + i;
    float p[KC], u[KC];
#pragma unroll
    for (int t = 0; t < KC; ++t) p[t] = 0.0f;
    const int e0 = ptr[node], e1 = ptr[node + 1];
    for (int e = e0; e < e1; e += 4) {
      int jj[4];
      float vv[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (e + b < e1) {
          const int pos = perm ? perm[e + b] : e + b;
          jj[b] = static_cast<int>(other[pos] - base);
          vv[b] = clamp_min(w ? w[pos] : 1.0f, 0.0f);
        }
      }
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (e + b < e1) {
          const float* const f = F + static_cast<IdxT>(jj[b]) * ld;
          const int kb = rows_fresh(ka);
#pragma unroll
          for (int t = 0; t < KC; ++t)
            if (t < kb) p[t] += vv[b] * f[t];
        }
      }
    }
    float* const urow = U + static_cast<IdxT>(i) * ld;
    const int ku = rows_fresh(ka);
#pragma unroll
    for (int t = 0; t < KC; ++t) u[t] = t < ku ? urow[t] : 0.0f;
    float rv = 0.0f;
#pragma unroll
    for (int t = 0; t < KC; ++t) {  // (no guard on ka: behind it p, u and the Gram entries are exact zeros, the
      float grad = -p[t];           //  terms they add change no bit and a zero Hessian leaves u alone)
      int row = t * NR_TILE;        // opaque to the compiler: the Gram row is read here, for this row of U, and not
      asm volatile("" : "+v"(row)); // hoisted out of the loop over the rows into a thousand registers
      const float* const gr = Gm + row;
#pragma unroll
      for (int r = 0; r < KC; ++r) grad += gr[r] * u[r];
      const float ut = u[t];
      const float pg = ut == 0.0f ? fminf(0.0f, grad) : grad;
      rv += fabsf(pg);
      const float hess = gr[t];
      if (hess != 0.0f) u[t] = fmaxf(ut - grad / hess, 0.0f);
    }
    const int ks = rows_fresh(ka);
#pragma unroll
    for (int t = 0; t < KC; ++t)
      if (t < ks) urow[t] = u[t];
    viol += rv;
  }
  return viol;
}

// init, the iteration loop and the outputs of one factorised graph (ka == K < n); HBM: the factors' home
template <bool HBM, int KC>
__device__ __forceinline__ void rows_solve(const RowsArgs& p, float* smem, int g, int base, int n, float total, int tid) {
  using IdxT = std::conditional_t<HBM, int64_t, int>;
  const int ka = p.K;
  const int ld = HBM ? p.K : (p.K | 1);
  float* const W = HBM ? p.w_out + static_cast<int64_t>(base) * p.K : smem + NR_FACTORS;
  float* const Ht = HBM ? p.ht_out + static_cast<int64_t>(base) * p.K : W + n * ld;
  float* const Gm = smem + NR_GRAM;
  float* const red = smem + NR_RED;
  int* const ctl = reinterpret_cast<int*>(smem + NR_CTL);

  const float avg = sqrtf((total / static_cast<float>(static_cast<int64_t>(n) * n)) / static_cast<float>(ka));
  for (int i = tid; i < n; i += NR_THREADS) {
    const int64_t at = (static_cast<int64_t>(base) + i) * p.K;
    float* const wr = W + static_cast<IdxT>(i) * ld;
    float* const hr = Ht + static_cast<IdxT>(i) * ld;
    for (int t = 0; t < ka; ++t) {
      if (p.w0) {
        wr[t] = p.w0[at + t];
        hr[t] = p.h0t[at + t];
      } else {
        wr[t] = avg * (2.0f * rows_uniform(p.seed, 0u, static_cast<uint32_t>(i), static_cast<uint32_t>(t)));
        hr[t] = avg * (2.0f * rows_uniform(p.seed, 1u, static_cast<uint32_t>(i), static_cast<uint32_t>(t)));
      }
    }
  }
  __syncthreads();

  int done = 0;
  float vinit = 0.0f, last_ratio = 0.0f;  // (thread 0's are the ones used)
  for (int it = 1; it <= p.max_iter; ++it) {
    rows_gram<IdxT>(Ht, ld, n, ka, smem, tid);                                                     // H H^T
    float viol = rows_sweep<IdxT, KC>(p.sptr, p.sperm, p.dst, p.w, W, Ht, ld, Gm, base, n, ka, tid);   // A H^T
    __syncthreads();
    rows_gram<IdxT>(W, ld, n, ka, smem, tid);                                                      // W^T W
    viol += rows_sweep<IdxT, KC>(p.dptr, p.dperm, p.src, p.w, Ht, W, ld, Gm, base, n, ka, tid);        // A^T W
    const float sum = block_fold_seq<NR_THREADS>(viol, red);
    if (tid == 0) {
      if (it == 1) vinit = sum;
      const bool stop = vinit == 0.0f || sum / vinit <= p.tol;  // (a NaN ratio: false)
      last_ratio = vinit == 0.0f ? 0.0f : sum / vinit;
      ctl[0] = stop ? 1 : 0;
    }
    __syncthreads();
    done = it;
    if (ctl[0]) break;  // one LDS word, read by every wave behind the barrier: all waves leave together
  }

  // a row's owner wrote it last: no barrier needed before its own read
  for (int i = tid; i < n; i += NR_THREADS) {
    const int64_t node = static_cast<int64_t>(base) + i;
    const float* const hrow = Ht + static_cast<IdxT>(i) * ld;
    float h[KC];
#pragma unroll
    for (int t = 0; t < KC; ++t) h[t] = t < ka ? hrow[t] : 0.0f;
    if (!HBM) {
      const float* const wrow = W + static_cast<IdxT>(i) * ld;
      for (int t = 0; t < ka; ++t) p.w_out[node * p.K + t] = wrow[t];
#pragma unroll
      for (int t = 0; t < KC; ++t)
        if (t < ka) p.ht_out[node * p.K + t] = h[t];
    }
    float m = h[0];
#pragma unroll
    for (int t = 1; t < KC; ++t)
      if (t < ka) m = nan_max(m, h[t]);
    float sum = 0.0f;
#pragma unroll
    for (int t = 0; t < KC; ++t)
      if (t < ka) sum += expf(h[t] - m);
    float* const out = p.s + node * p.out_cols;
#pragma unroll
    for (int t = 0; t < KC; ++t)
      if (t < ka) out[t] = expf(h[t] - m) / sum;
    for (int t = ka; t < p.out_cols; ++t) out[t] = 0.0f;
  }
  if (tid == 0) {
    if (p.iters) p.iters[g] = done;
    if (p.ratio) p.ratio[g] = last_ratio;
  }
}

// the bitwise OR of `v` over the workgroup through one LDS word (an integer OR: any order gives the same word); the
// kernel has no static LDS, so the whole 160 KiB is the dynamic frame
__device__ __forceinline__ int rows_block_or(int v, int* word) {
  if (threadIdx.x == 0) *word = 0;
  __syncthreads();
  if (v) atomicOr(word, v);
  __syncthreads();
  const int all = *word;
  __syncthreads();
  return all;
}

template <int KC>
__global__ __launch_bounds__(NR_THREADS) void nmf_rows_kernel(RowsArgs p) {
  extern __shared__ __align__(16) float nmf_rows_smem[];
  float* const smem = nmf_rows_smem;
  int* const ctl = reinterpret_cast<int*>(smem + NR_CTL);
  const int tid = threadIdx.x;

  // ---- per-workgroup (uniform) decisions
  const int g = p.list[blockIdx.x];
  if (g < 0 || g >= p.G) {
    if (tid == 0) atomicOr(p.status, TGP_NMF_BAD_INPUT);
    return;
  }
  const int t0 = p.graph_ptr[g], t1 = p.graph_ptr[g + 1];
  if (t0 < 0 || t1 < t0 || t1 > p.N) {
    if (tid == 0) atomicOr(p.status, TGP_NMF_BAD_INPUT);
    return;
  }
  const int n = t1 - t0;
  if (n == 0) return;
  const int ka = p.K < n ? p.K : n;
  if (ka > p.out_cols) {
    if (tid == 0) atomicOr(p.status, TGP_NMF_BAD_INPUT);
    return;
  }
  // the members: nodes of this graph, and one run base, base + 1, ..
  const int base = p.graph_perm[t0];
  int flags = 0;
  for (int a = tid; a < n; a += NR_THREADS) {
    const int node = p.graph_perm[t0 + a];
    if (node < 0 || node >= p.N || p.gid[node] != g) flags |= TGP_NMF_BAD_INPUT;
    else if (static_cast<int64_t>(node) != static_cast<int64_t>(base) + a) flags |= TGP_NMF_NOT_COALESCED;
  }
  flags = rows_block_or(flags, ctl);
  if (flags) {  // (an index outside its table first: a list with both is refused, not declined)
    if (tid == 0) atomicOr(p.status, (flags & TGP_NMF_BAD_INPUT) ? TGP_NMF_BAD_INPUT : TGP_NMF_NOT_COALESCED);
    return;
  }
  // every group of the graph, both directions; the clamped entries' sum on the way (a thread's rows ascending)
  float total = 0.0f;
  for (int i = tid; i < n; i += NR_THREADS) {
    float rs = 0.0f, none = 0.0f;
    flags |= rows_check_group<true>(p.sptr, p.sperm, p.dst, p.src, p.w, base + i, base, n, p.E, rs);
    flags |= rows_check_group<false>(p.dptr, p.dperm, p.src, p.dst, p.w, base + i, base, n, p.E, none);
    total += rs;
  }
  flags = rows_block_or(flags, ctl);
  if (flags & (TGP_NMF_BAD_INPUT | TGP_NMF_NOT_COALESCED)) {
    if (tid == 0) atomicOr(p.status, (flags & TGP_NMF_BAD_INPUT) ? TGP_NMF_BAD_INPUT : TGP_NMF_NOT_COALESCED);
    return;
  }
  // the reference's rules that need no factorisation (nmf_select.py:63-69)
  if ((n > 1 && ka >= n) || ka == 1) {
    const bool eye = n > 1 && ka >= n;
    for (int64_t idx = tid; idx < static_cast<int64_t>(n) * p.out_cols; idx += NR_THREADS) {
      const int64_t a = idx / p.out_cols, c = idx - a * p.out_cols;
      p.s[(base + a) * p.out_cols + c] = eye ? (c == a ? 1.0f : 0.0f) : (c == 0 ? 1.0f : 0.0f);
    }
    return;
  }
  if (flags & TGP_NMF_NON_FINITE) {
    if (tid == 0) atomicOr(p.status, TGP_NMF_NON_FINITE);
    return;
  }
  total = block_fold_seq<NR_THREADS, true>(total, smem + NR_RED);
  if (p.home == 1 || n > p.lds_nodes) rows_solve<true, KC>(p, smem, g, base, n, total, tid);
  else rows_solve<false, KC>(p, smem, g, base, n, total, tid);
}

constexpr int64_t I32_MAX = 2147483647;

template <int KC>
int rows_launch(const RowsArgs& a, int listed, void* stream) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(nmf_rows_kernel<KC>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            NR_LDS_BYTES);
  hipLaunchKernelGGL(nmf_rows_kernel<KC>, dim3(static_cast<unsigned>(listed)), dim3(NR_THREADS), NR_LDS_BYTES,
                     static_cast<hipStream_t>(stream), a);
  return check_launch("tgp_nmfrows_factorize_f32");
}

}  // namespace
}  // namespace tgp

using namespace tgp;

extern "C" int tgp_nmfrows_lds_nodes(int64_t K) {
  if (K < 1 || K > tgp_nmf_max_k() || K > NR_TILE) return 0;
  return rows_lds_nodes(static_cast<int>(K));
}

extern "C" int tgp_nmfrows_factorize_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* dst,
                                         const float* edge_weight, const int32_t* gid, const int32_t* graph_ptr,
                                         const int32_t* graph_perm, int64_t N, int64_t E, int64_t G, int64_t K,
                                         int64_t out_cols, int64_t seed, float tol, int64_t max_iter, const float* w0,
                                         const float* h0t, float* s, float* w_out, float* ht_out, int32_t* iters,
                                         float* violation_ratio, int32_t* status, const int32_t* dgrp_ptr,
                                         const int32_t* dgrp_perm, const int64_t* src, const int32_t* graph_list,
                                         int64_t num_listed, int64_t home, void* stream) {
  TGP_REQUIRE(N >= 0 && E >= 0 && G >= 0 && num_listed >= 0, TGP_ERR_INVALID,
              "tgp_nmfrows_factorize_f32: negative size");
  TGP_REQUIRE(K >= 1, TGP_ERR_INVALID, "tgp_nmfrows_factorize_f32: K = %lld < 1", static_cast<long long>(K));
  TGP_REQUIRE(K <= tgp_nmf_max_k() && K <= NR_TILE, TGP_ERR_INVALID, "tgp_nmfrows_factorize_f32: K = %lld > %d",
              static_cast<long long>(K), tgp_nmf_max_k());
  TGP_REQUIRE(out_cols >= 1, TGP_ERR_INVALID, "tgp_nmfrows_factorize_f32: out_cols = %lld < 1",
              static_cast<long long>(out_cols));
  TGP_REQUIRE(max_iter >= 1, TGP_ERR_INVALID, "tgp_nmfrows_factorize_f32: max_iter = %lld < 1",
              static_cast<long long>(max_iter));
  TGP_REQUIRE(tol >= 0.0f, TGP_ERR_INVALID, "tgp_nmfrows_factorize_f32: tol = %g is negative or NaN",
              static_cast<double>(tol));
  TGP_REQUIRE(home == 0 || home == 1, TGP_ERR_INVALID, "tgp_nmfrows_factorize_f32: home = %lld is neither 0 nor 1",
              static_cast<long long>(home));
  TGP_REQUIRE(grp_ptr && dgrp_ptr && gid && graph_ptr && graph_perm && s && w_out && ht_out && status, TGP_ERR_INVALID,
              "tgp_nmfrows_factorize_f32: NULL pointer");
  TGP_REQUIRE(num_listed == 0 || graph_list, TGP_ERR_INVALID, "tgp_nmfrows_factorize_f32: NULL graph list");
  TGP_REQUIRE(E == 0 || (dst && src), TGP_ERR_INVALID, "tgp_nmfrows_factorize_f32: NULL dst or src with E > 0");
  TGP_REQUIRE((w0 == nullptr) == (h0t == nullptr), TGP_ERR_INVALID,
              "tgp_nmfrows_factorize_f32: an explicit init needs both W0 and H0^T");
  TGP_REQUIRE(N <= I32_MAX && E <= I32_MAX && G <= I32_MAX && out_cols <= I32_MAX && max_iter <= I32_MAX &&
                  num_listed <= I32_MAX,
              TGP_ERR_RANGE, "tgp_nmfrows_factorize_f32: N, E, G, out_cols, max_iter or the list beyond the int32 index");
  if (G == 0 || N == 0 || num_listed == 0) return TGP_OK;
  const int Kc = static_cast<int>(K);
  RowsArgs a{grp_ptr, grp_perm, dst, dgrp_ptr, dgrp_perm, src, edge_weight, gid, graph_ptr, graph_perm, graph_list,
             static_cast<int>(N), static_cast<int>(E), static_cast<int>(G), Kc, static_cast<int>(out_cols),
             static_cast<int>(max_iter), static_cast<int>(home), rows_lds_nodes(Kc), tol,
             static_cast<uint32_t>(static_cast<uint64_t>(seed) & 0xFFFFFFFFull), w0, h0t, s, w_out, ht_out, iters,
             violation_ratio, status};
  const int listed = static_cast<int>(num_listed);
  if (Kc <= 4) return rows_launch<4>(a, listed, stream);
  if (Kc <= 8) return rows_launch<8>(a, listed, stream);
  if (Kc <= 16) return rows_launch<16>(a, listed, stream);
  return rows_launch<32>(a, listed, stream);
}
