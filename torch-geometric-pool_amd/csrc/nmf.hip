// NMF pooling (Bacciu and Di Sotto 2019; reference select/nmf_select.py): A ~ W H per graph by scikit-learn's coordinate
// descent (solver "cd", shuffle off, no regularisation), S = softmax(H^T).
//
// One workgroup per graph.  The graph's adjacency is gathered from the by-source edge index into LDS (duplicates added in
// edge-list order in fp32, then clamped at 0), and A, W, H^T, the n x ka product buffer and the ka x ka Gram matrix stay
// there for the whole run: the iteration loop, the convergence test and the softmax are one launch.
//   half-sweep:  Gram = F^T F and P = A F (or A^T F), every entry summed in ascending index order by one lane; then row i
//                of the other factor is updated by thread i, its ka components in order (they depend on each other; rows
//                do not).  fp32 throughout, no fused multiply-add (the library is built with -ffp-contract=off), no float
//                atomics: the same bits on every call.
//   leaving:     wave 0 adds the row violations in a fixed order and writes the decision into one LDS word; every wave
//                reads that word behind a barrier, so all waves leave in the same iteration.  max_iter caps the loop
//                whatever the violations are (a NaN ratio compares false and runs to the cap).
//   init:        the default W0 / H0 are a hash of (seed, which factor, graph-local node index, component) scaled to
//                scikit-learn's avg = sqrt(mean(A) / ka); an explicit init replaces them.
#include "common.h"

#include <float.h>

namespace tgp {
namespace {

constexpr int NMF_MAX_NODES = 128;  // 128 x 129 fp32 adjacency + three 128 x 33 factor buffers + the Gram matrix = 119 KB
constexpr int NMF_MAX_K = 32;       // of the 160 KB LDS of a CU
constexpr int NMF_SMALL_NODES = 64; // launches whose graphs all fit run 128 threads (a row update uses one thread per node)

constexpr int NMF_BAD_INPUT = 1;    // an index outside its table, an edge across two graphs
constexpr int NMF_NON_FINITE = 2;   // a NaN or infinite entry of the clamped adjacency
constexpr int NMF_OVER_LIMIT = 4;   // a graph of more than max_n nodes, or K > NMF_MAX_K

struct NmfLds {
  int lda, ldk;
  size_t a, w, ht, p, gram, row, mem, ctl, total;
};
inline NmfLds nmf_lds_layout(int max_n, int kc) {
  NmfLds l;
  l.lda = max_n | 1;  // odd row strides: a column walk does not stay on one bank
  l.ldk = kc | 1;
  size_t off = 0;
  l.a = off;    off += sizeof(float) * max_n * l.lda;
  l.w = off;    off += sizeof(float) * max_n * l.ldk;
  l.ht = off;   off += sizeof(float) * max_n * l.ldk;
  l.p = off;    off += sizeof(float) * max_n * l.ldk;
  l.gram = off; off += sizeof(float) * kc * l.ldk;
  l.row = off;  off += sizeof(float) * max_n;
  l.mem = off;  off += sizeof(int) * max_n;
  l.ctl = off;  off += sizeof(int) * 4;
  l.total = off;
  return l;
}

// position of `node` in the ascending list mem[0 .. m), or -1
__device__ __forceinline__ int nmf_local_of(const int* mem, int m, int node) {
  int lo = 0, hi = m;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (mem[mid] < node) lo = mid + 1;
    else hi = mid;
  }
  return (lo < m && mem[lo] == node) ? lo : -1;
}

// The default init's uniform u in (0, 1]: 32-bit integer arithmetic only (tests/nmf_restatement.py states the same hash
// with masked int64 operations).  `i` is the node's index inside its graph: a graph's init does not depend on where
// the graph stands in the batch.
__device__ __forceinline__ float nmf_uniform(uint32_t seed, uint32_t which, uint32_t i, uint32_t t) {
  uint32_t h = seed * 0x9E3779B9u + which * 0x85EBCA6Bu + i * 0xC2B2AE35u + t * 0x27D4EB2Fu + 0x165667B1u;
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return static_cast<float>((h >> 8) + 1u) * (1.0f / 16777216.0f);  // exact: 24 bits
}

struct NmfArgs {
  const int32_t* grp_ptr;     // [N + 1] by-source offsets
  const int32_t* grp_perm;    // [E] edge positions by source (NULL: the list is grouped already)
  const int64_t* dst;         // [E]
  const float* w;             // [E] or NULL
  const int32_t* gid;         // [N] graph of every node
  const int32_t* graph_ptr;   // [G + 1]
  const int32_t* graph_perm;  // [N] nodes by graph, ascending
  int N, E, G, K, out_cols, max_n, max_iter, init_only;
  float tol;
  uint32_t seed;
  const float* w0;            // [N, K] explicit init (both or neither)
  const float* h0t;           // [N, K]
  float* s;                   // [N, out_cols]
  float* w_out;               // [N, K] or NULL
  float* ht_out;              // [N, K] or NULL
  int32_t* iters;             // [G] or NULL
  float* ratio;               // [G] or NULL
  int32_t* status;
  NmfLds l;
};

// Gram = F^T F [ka, ka] and P = A F (transposed: A^T F) [n, ka]; every entry by one lane, j ascending
__device__ __forceinline__ void nmf_gram_product(const float* A, int lda, bool transposed, const float* F, float* Gm,
                                                 float* P, int n, int ka, int ldk, int tid, int T) {
  for (int idx = tid; idx < ka * ka; idx += T) {
    const int t = idx / ka, r = idx - t * ka;
    float acc = 0.0f;
    for (int j = 0; j < n; ++j) acc += F[j * ldk + t] * F[j * ldk + r];
    Gm[t * ldk + r] = acc;
  }
  for (int idx = tid; idx < n * ka; idx += T) {
    const int i = idx / ka, t = idx - i * ka;
    float acc = 0.0f;
    if (transposed) {
      for (int j = 0; j < n; ++j) acc += A[j * lda + i] * F[j * ldk + t];
    } else {
      for (int j = 0; j < n; ++j) acc += A[i * lda + j] * F[j * ldk + t];
    }
    P[i * ldk + t] = acc;
  }
}

// scikit-learn's _update_cdnmf_fast for row `tid` of U: the components in order, each using the row's updated entries;
// returns the row's projected-gradient violation
__device__ __forceinline__ float nmf_row_update(float* U, const float* Gm, const float* P, int n, int ka, int ldk,
                                                int tid) {
  float viol = 0.0f;
  if (tid < n) {
    float* const u = U + tid * ldk;
    const float* const p = P + tid * ldk;
    for (int t = 0; t < ka; ++t) {
      float grad = -p[t];
      for (int r = 0; r < ka; ++r) grad += Gm[t * ldk + r] * u[r];
      const float ut = u[t];
      const float pg = ut == 0.0f ? fminf(0.0f, grad) : grad;
      viol += fabsf(pg);
      const float hess = Gm[t * ldk + t];
      if (hess != 0.0f) u[t] = fmaxf(ut - grad / hess, 0.0f);
    }
  }
  return viol;
}

__global__ __launch_bounds__(256) void nmf_factorize_kernel(NmfArgs p) {
  extern __shared__ float nmf_smem[];
  char* const base = reinterpret_cast<char*>(nmf_smem);
  float* const A = reinterpret_cast<float*>(base + p.l.a);
  float* const W = reinterpret_cast<float*>(base + p.l.w);
  float* const Ht = reinterpret_cast<float*>(base + p.l.ht);
  float* const P = reinterpret_cast<float*>(base + p.l.p);
  float* const Gm = reinterpret_cast<float*>(base + p.l.gram);
  float* const rowbuf = reinterpret_cast<float*>(base + p.l.row);
  int* const mem = reinterpret_cast<int*>(base + p.l.mem);
  int* const ctl = reinterpret_cast<int*>(base + p.l.ctl);
  const int lda = p.l.lda, ldk = p.l.ldk, tid = threadIdx.x, T = blockDim.x;
  const int g = blockIdx.x;

  // ---- per-workgroup (uniform) decisions
  const int t0 = p.graph_ptr[g], t1 = p.graph_ptr[g + 1];
  if (t0 < 0 || t1 < t0 || t1 > p.N) {
    if (tid == 0) atomicOr(p.status, NMF_BAD_INPUT);
    return;
  }
  const int n = t1 - t0;
  if (n == 0) return;
  if (n > p.max_n || p.K > NMF_MAX_K) {
    if (tid == 0) atomicOr(p.status, NMF_OVER_LIMIT);
    return;
  }
  const int ka = p.K < n ? p.K : n;  // (K >= 1, n >= 1)
  if (!p.init_only && ka > p.out_cols) {
    if (tid == 0) atomicOr(p.status, NMF_BAD_INPUT);
    return;
  }
  // the members, ascending; every one must be a node of this graph
  int bad = 0;
  for (int a = tid; a < n; a += T) {
    const int node = p.graph_perm[t0 + a];
    if (node < 0 || node >= p.N || p.gid[node] != g) {
      bad = 1;
      mem[a] = 0;
    } else {
      mem[a] = node;
    }
  }
  for (int i = tid; i < n * lda; i += T) A[i] = 0.0f;
  if (__syncthreads_or(bad)) {
    if (tid == 0) atomicOr(p.status, NMF_BAD_INPUT);
    return;
  }
  for (int a = tid + 1; a < n; a += T)
    if (mem[a - 1] >= mem[a]) bad = 1;
  if (__syncthreads_or(bad)) {
    if (tid == 0) atomicOr(p.status, NMF_BAD_INPUT);
    return;
  }
  // the adjacency: row a is owned by one thread, which adds its node's edges in edge-list order
  for (int a = tid; a < n; a += T) {
    const int node = mem[a];
    const int e0 = p.grp_ptr[node], e1 = p.grp_ptr[node + 1];
    if (e0 < 0 || e1 < e0 || e1 > p.E) {
      bad = 1;
      continue;
    }
    for (int e = e0; e < e1; ++e) {
      const int pos = p.grp_perm ? p.grp_perm[e] : e;
      if (pos < 0 || pos >= p.E) {
        bad = 1;
        continue;
      }
      const int64_t j = p.dst[pos];
      if (j < 0 || j >= p.N || p.gid[j] != g) {  // (an edge that leaves the graph is refused, as the reference's
        bad = 1;                                 //  per-graph to_dense_adj refuses it)
        continue;
      }
      const int b = nmf_local_of(mem, n, static_cast<int>(j));
      if (b < 0) {
        bad = 1;
        continue;
      }
      A[a * lda + b] += p.w ? p.w[pos] : 1.0f;
    }
  }
  if (__syncthreads_or(bad)) {
    if (tid == 0) atomicOr(p.status, NMF_BAD_INPUT);
    return;
  }
  // the reference's rules that need no factorisation (nmf_select.py:63-69)
  if ((n > 1 && ka >= n) || ka == 1) {
    if (p.init_only) return;
    const bool eye = n > 1 && ka >= n;
    for (int idx = tid; idx < n * p.out_cols; idx += T) {
      const int a = idx / p.out_cols, c = idx - a * p.out_cols;
      p.s[static_cast<int64_t>(mem[a]) * p.out_cols + c] = eye ? (c == a ? 1.0f : 0.0f) : (c == 0 ? 1.0f : 0.0f);
    }
    return;
  }
  // clamp at 0 (a NaN falls through, as Tensor.clamp lets it), refuse what scikit-learn's input check refuses, row sums
  for (int a = tid; a < n; a += T) {
    float rs = 0.0f;
    for (int b = 0; b < n; ++b) {
      const float v = clamp_min(A[a * lda + b], 0.0f);
      if (!(v <= FLT_MAX)) bad = 1;
      A[a * lda + b] = v;
      rs += v;
    }
    rowbuf[a] = rs;
  }
  if (__syncthreads_or(bad)) {
    if (tid == 0) atomicOr(p.status, NMF_NON_FINITE);
    return;
  }
  // ---- init
  if (p.w0) {
    for (int idx = tid; idx < n * ka; idx += T) {
      const int i = idx / ka, t = idx - i * ka;
      const int64_t at = static_cast<int64_t>(mem[i]) * p.K + t;
      W[i * ldk + t] = p.w0[at];
      Ht[i * ldk + t] = p.h0t[at];
    }
  } else {
    float total = 0.0f;  // every thread adds the row sums in ascending order: the same value in all of them
    for (int a = 0; a < n; ++a) total += rowbuf[a];
    const float avg = sqrtf((total / static_cast<float>(n * n)) / static_cast<float>(ka));
    for (int idx = tid; idx < n * ka; idx += T) {
      const int i = idx / ka, t = idx - i * ka;
      W[i * ldk + t] = avg * (2.0f * nmf_uniform(p.seed, 0u, static_cast<uint32_t>(i), static_cast<uint32_t>(t)));
      Ht[i * ldk + t] = avg * (2.0f * nmf_uniform(p.seed, 1u, static_cast<uint32_t>(i), static_cast<uint32_t>(t)));
    }
  }
  __syncthreads();

  // ---- the coordinate descent
  int done = 0;
  float vinit = 0.0f, last_ratio = 0.0f;  // (thread 0's are the ones used)
  if (!p.init_only) {
    for (int it = 1; it <= p.max_iter; ++it) {
      nmf_gram_product(A, lda, false, Ht, Gm, P, n, ka, ldk, tid, T);  // H H^T and A H^T
      __syncthreads();
      float viol = nmf_row_update(W, Gm, P, n, ka, ldk, tid);
      __syncthreads();
      nmf_gram_product(A, lda, true, W, Gm, P, n, ka, ldk, tid, T);    // W^T W and A^T W
      __syncthreads();
      viol += nmf_row_update(Ht, Gm, P, n, ka, ldk, tid);
      if (tid < n) rowbuf[tid] = viol;
      __syncthreads();
      if (tid < 64) {  // wave 0: lane l adds rows l, l + 64 in order, then the xor butterfly of wave_sum
        float s = 0.0f;
        for (int a = tid; a < n; a += 64) s += rowbuf[a];
        s = wave_sum(s);
        if (tid == 0) {
          if (it == 1) vinit = s;
          const bool stop = vinit == 0.0f || s / vinit <= p.tol;  // (a NaN ratio: false)
          last_ratio = vinit == 0.0f ? 0.0f : s / vinit;
          ctl[0] = stop ? 1 : 0;
        }
      }
      __syncthreads();
      done = it;
      if (ctl[0]) break;  // one LDS word, read by every wave behind the barrier: all waves leave together
    }
  }

  // ---- outputs
  if (tid < n) {
    const int64_t node = mem[tid];
    if (p.w_out) {
      for (int t = 0; t < p.K; ++t) p.w_out[node * p.K + t] = t < ka ? W[tid * ldk + t] : 0.0f;
    }
    if (p.ht_out) {
      for (int t = 0; t < p.K; ++t) p.ht_out[node * p.K + t] = t < ka ? Ht[tid * ldk + t] : 0.0f;
    }
    if (!p.init_only) {  // softmax over the ka columns, zero columns up to out_cols
      const float* const h = Ht + tid * ldk;
      float m = h[0];
      for (int t = 1; t < ka; ++t) m = nan_max(m, h[t]);
      float sum = 0.0f;
      for (int t = 0; t < ka; ++t) sum += expf(h[t] - m);
      float* const out = p.s + node * p.out_cols;
      for (int t = 0; t < p.out_cols; ++t) out[t] = t < ka ? expf(h[t] - m) / sum : 0.0f;
    }
  }
  if (tid == 0 && !p.init_only) {
    if (p.iters) p.iters[g] = done;
    if (p.ratio) p.ratio[g] = last_ratio;
  }
}

constexpr int64_t I32_MAX = 2147483647;

int nmf_launch(const char* what, NmfArgs a, void* stream) {
  const int kc = a.K < NMF_MAX_K ? a.K : NMF_MAX_K;
  a.l = nmf_lds_layout(a.max_n, kc);
  if (a.l.total > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(nmf_factorize_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(a.l.total));
  const int threads = a.max_n <= NMF_SMALL_NODES ? 128 : 256;
  hipLaunchKernelGGL(nmf_factorize_kernel, dim3(static_cast<unsigned>(a.G)), dim3(threads), a.l.total,
                     static_cast<hipStream_t>(stream), a);
  return check_launch(what);
}

}  // namespace
}  // namespace tgp

using namespace tgp;

extern "C" int tgp_nmf_max_nodes(void) { return NMF_MAX_NODES; }
extern "C" int tgp_nmf_max_k(void) { return NMF_MAX_K; }

extern "C" int tgp_nmf_init_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* dst,
                                const float* edge_weight, const int32_t* gid, const int32_t* graph_ptr,
                                const int32_t* graph_perm, int64_t N, int64_t E, int64_t G, int64_t K, int64_t max_n,
                                int64_t seed, float* w0, float* h0t, int32_t* status, void* stream) {
  TGP_REQUIRE(N >= 0 && E >= 0 && G >= 0, TGP_ERR_INVALID, "tgp_nmf_init_f32: negative size");
  TGP_REQUIRE(K >= 1, TGP_ERR_INVALID, "tgp_nmf_init_f32: K = %lld < 1", static_cast<long long>(K));
  TGP_REQUIRE(max_n >= 1 && max_n <= NMF_MAX_NODES, TGP_ERR_INVALID, "tgp_nmf_init_f32: max_n = %lld outside 1 .. %d",
              static_cast<long long>(max_n), NMF_MAX_NODES);
  TGP_REQUIRE(grp_ptr && gid && graph_ptr && graph_perm && w0 && h0t && status, TGP_ERR_INVALID,
              "tgp_nmf_init_f32: NULL pointer");
  TGP_REQUIRE(E == 0 || dst, TGP_ERR_INVALID, "tgp_nmf_init_f32: NULL dst with E > 0");
  TGP_REQUIRE(N <= I32_MAX && E <= I32_MAX && G <= I32_MAX && K <= I32_MAX, TGP_ERR_RANGE,
              "tgp_nmf_init_f32: N, E, G or K beyond the int32 index");
  if (G == 0 || N == 0) return TGP_OK;
  NmfArgs a{grp_ptr, grp_perm, dst, edge_weight, gid, graph_ptr, graph_perm, static_cast<int>(N), static_cast<int>(E),
            static_cast<int>(G), static_cast<int>(K), static_cast<int>(K), static_cast<int>(max_n), 0, 1, 0.0f,
            static_cast<uint32_t>(static_cast<uint64_t>(seed) & 0xFFFFFFFFull), nullptr, nullptr, nullptr, w0, h0t,
            nullptr, nullptr, status, NmfLds{}};
  return nmf_launch("tgp_nmf_init_f32", a, stream);
}

extern "C" int tgp_nmf_factorize_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* dst,
                                     const float* edge_weight, const int32_t* gid, const int32_t* graph_ptr,
                                     const int32_t* graph_perm, int64_t N, int64_t E, int64_t G, int64_t K,
                                     int64_t out_cols, int64_t max_n, int64_t seed, float tol, int64_t max_iter,
                                     const float* w0, const float* h0t, float* s, float* w_out, float* ht_out,
                                     int32_t* iters, float* violation_ratio, int32_t* status, void* stream) {
  TGP_REQUIRE(N >= 0 && E >= 0 && G >= 0, TGP_ERR_INVALID, "tgp_nmf_factorize_f32: negative size");
  TGP_REQUIRE(K >= 1, TGP_ERR_INVALID, "tgp_nmf_factorize_f32: K = %lld < 1", static_cast<long long>(K));
  TGP_REQUIRE(out_cols >= 1, TGP_ERR_INVALID, "tgp_nmf_factorize_f32: out_cols = %lld < 1",
              static_cast<long long>(out_cols));
  TGP_REQUIRE(max_iter >= 1, TGP_ERR_INVALID, "tgp_nmf_factorize_f32: max_iter = %lld < 1",
              static_cast<long long>(max_iter));
  TGP_REQUIRE(tol >= 0.0f, TGP_ERR_INVALID, "tgp_nmf_factorize_f32: tol = %g is negative or NaN",
              static_cast<double>(tol));
  TGP_REQUIRE(max_n >= 1 && max_n <= NMF_MAX_NODES, TGP_ERR_INVALID,
              "tgp_nmf_factorize_f32: max_n = %lld outside 1 .. %d", static_cast<long long>(max_n), NMF_MAX_NODES);
  TGP_REQUIRE(grp_ptr && gid && graph_ptr && graph_perm && s && status, TGP_ERR_INVALID,
              "tgp_nmf_factorize_f32: NULL pointer");
  TGP_REQUIRE(E == 0 || dst, TGP_ERR_INVALID, "tgp_nmf_factorize_f32: NULL dst with E > 0");
  TGP_REQUIRE((w0 == nullptr) == (h0t == nullptr), TGP_ERR_INVALID,
              "tgp_nmf_factorize_f32: an explicit init needs both W0 and H0^T");
  TGP_REQUIRE(N <= I32_MAX && E <= I32_MAX && G <= I32_MAX && K <= I32_MAX && out_cols <= I32_MAX &&
                  max_iter <= I32_MAX,
              TGP_ERR_RANGE, "tgp_nmf_factorize_f32: N, E, G, K, out_cols or max_iter beyond the int32 index");
  if (G == 0 || N == 0) return TGP_OK;
  NmfArgs a{grp_ptr, grp_perm, dst, edge_weight, gid, graph_ptr, graph_perm, static_cast<int>(N), static_cast<int>(E),
            static_cast<int>(G), static_cast<int>(K), static_cast<int>(out_cols), static_cast<int>(max_n),
            static_cast<int>(max_iter), 0, tol, static_cast<uint32_t>(static_cast<uint64_t>(seed) & 0xFFFFFFFFull), w0,
            h0t, s, w_out, ht_out, iters, violation_ratio, status, NmfLds{}};
  return nmf_launch("tgp_nmf_factorize_f32", a, stream);
}
