// DMoN's auxiliary losses (reference poolers/dmon.py, utils/losses.py:435-473, 1083-1265):
//
//   spectral[b] = -(trace(S^T A S) - ||S^T d||^2 / 2m) / 2m       d = degrees, 2m = sum_i d_i (0 when m = 0 batched,
//                                                                  m clamped to eps unbatched)
//   cluster[b]  = ||S^T 1|| sqrt(K) / n_b - 1                      n_b = real nodes (mask.sum(1), N without a mask)
//   ortho[b]    = || G / ||G||_F - I / sqrt(K) ||_F                G = S^T S (as MinCut's)
//
// The per-graph K-vectors ca = S^T d and cs = S^T 1 are reduced in two stages: every workgroup of the partial pass
// writes the sums over its 64 rows, the tail adds the partials of a graph in a fixed order (no float atomics).
// trace(S^T A S) comes from the raw Connect product (or, for an edge list, from a per-graph vector).
#include "loss_common.h"

namespace tgp {
namespace {

// One workgroup per (64 columns, 64 rows, graph): part[b][split] = [ca (K) | cs (K) | sum of d | node count].
// Graph b owns rows start .. start + count of S and deg: padded (ptr == NULL: start = b N, count = graph size or N)
// or un-padded (start = ptr[b], count = ptr[b+1] - ptr[b]).  The node count follows the reference: the mask's true
// entries among the N padded rows (N without a mask), the graph's rows when un-padded.
__global__ __launch_bounds__(256) void dmon_part_kernel(const float* __restrict__ S, const float* __restrict__ deg,
                                                        int N, int K, const int64_t* __restrict__ sizes,
                                                        const uint8_t* __restrict__ mask,
                                                        const int64_t* __restrict__ ptr, int nsplit,
                                                        float* __restrict__ part) {
  __shared__ float sh_ca[4][64], sh_cs[4][64];
  __shared__ float sh[8];
  const int kc = blockIdx.x, split = blockIdx.y, b = blockIdx.z;
  const int c = threadIdx.x & 63, r = threadIdx.x >> 6;
  const int k = kc * 64 + c;
  int64_t start, count;
  graph_rows(b, N, sizes, ptr, start, count);
  const int64_t span = ptr ? count : N;
  const int64_t lo = static_cast<int64_t>(split) * PART_ROWS;
  const int64_t hi = count < lo + PART_ROWS ? count : lo + PART_ROWS;
  float ca = 0.f, cs = 0.f;
  if (k < K) {
#pragma unroll 4
    for (int64_t i = lo + r; i < hi; i += 4) {
      const int64_t row = start + i;
      const float s = S[row * K + k];
      cs += s;
      if (deg) ca = fmaf(deg[row], s, ca);
    }
  }
  sh_ca[r][c] = ca;
  sh_cs[r][c] = cs;
  __syncthreads();
  float* out = part + (static_cast<int64_t>(b) * nsplit + split) * (2 * K + 2);
  if (r == 0 && k < K) {
    out[k] = (sh_ca[0][c] + sh_ca[1][c]) + (sh_ca[2][c] + sh_ca[3][c]);
    out[K + k] = (sh_cs[0][c] + sh_cs[1][c]) + (sh_cs[2][c] + sh_cs[3][c]);
  }
  if (kc == 0) {  // (uniform over the workgroup)
    float dsum = 0.f, nr = 0.f;
    if (threadIdx.x < PART_ROWS) {
      const int64_t i = lo + threadIdx.x;
      if (deg && i < hi) dsum = deg[start + i];
      if (i < span) nr = (ptr || !mask) ? 1.f : (mask[start + i] ? 1.f : 0.f);
    }
    float v[2] = {dsum, nr};
    block_sums<256, 2>(v, sh);
    if (threadIdx.x == 0) {
      out[2 * K] = v[0];
      out[2 * K + 1] = v[1];
    }
  }
}

// One workgroup per graph: the partials summed in split order, then the three terms times their coefficients (out [3,B]).  Also written for the
// backward: ca, cs [B,K] and stats [B,4] = (2m as used, 0 when the spectral term is 0 | n_b | ||cs|| | trace).
template <int T>
__global__ __launch_bounds__(T) void dmon_tail_kernel(const float* __restrict__ part, int nsplit,
                                                      const float* __restrict__ raw, const float* __restrict__ tr_in,
                                                      const float* __restrict__ gram, int K, float sqrt_k, int clamp_m,
                                                      float eps, float c_spec, float c_clu, float c_ort, int B,
                                                      float* __restrict__ out,
                                                      float* __restrict__ ca_out, float* __restrict__ cs_out,
                                                      float* __restrict__ stats) {
  __shared__ float sh[6 * (T / 64)];
  const int b = blockIdx.x;
  const int P = 2 * K + 2;
  const float* pb = part + static_cast<int64_t>(b) * nsplit * P;
  float casq = 0.f, cssq = 0.f;
  for (int k = threadIdx.x; k < K; k += T) {
    float a = 0.f, s = 0.f;
#pragma unroll 8
    for (int j = 0; j < nsplit; ++j) {
      a += pb[static_cast<int64_t>(j) * P + k];
      s += pb[static_cast<int64_t>(j) * P + K + k];
    }
    ca_out[static_cast<int64_t>(b) * K + k] = a;
    cs_out[static_cast<int64_t>(b) * K + k] = s;
    casq = fmaf(a, a, casq);
    cssq = fmaf(s, s, cssq);
  }
  float m2 = 0.f, nr = 0.f;
  for (int j = threadIdx.x; j < nsplit; j += T) {
    m2 += pb[static_cast<int64_t>(j) * P + 2 * K];
    nr += pb[static_cast<int64_t>(j) * P + 2 * K + 1];
  }
  const int64_t off = static_cast<int64_t>(b) * K * K;
  float tr = 0.f, sq = 0.f;
  if (raw)
    for (int i = threadIdx.x; i < K; i += T) tr += raw[off + static_cast<int64_t>(i) * K + i];
  if (gram)
    for (int i = threadIdx.x; i < K * K; i += T) sq = fmaf(gram[off + i], gram[off + i], sq);
  float v[6] = {casq, cssq, m2, nr, tr, sq};
  block_sums<T, 6>(v, sh);
  casq = v[0], cssq = v[1], m2 = v[2], nr = v[3], tr = v[4], sq = v[5];
  const float ortho = gram ? ortho_term<T>(gram + off, K, sq, sh) : 0.f;
  if (threadIdx.x == 0) {
    if (!raw) tr = tr_in ? tr_in[b] : 0.f;
    float m = 0.5f * m2;
    bool active = m > 0.f;
    if (clamp_m) {
      m = fmaxf(m, eps);
      active = true;
    }
    const float den = 2.0f * m;
    const float ncs = sqrtf(cssq);
    out[b] = (active ? -(tr - casq / den) / den : 0.f) * c_spec;
    out[B + b] = (ncs / nr * sqrt_k - 1.0f) * c_clu;
    out[2 * B + b] = ortho * c_ort;
    float* st = stats + static_cast<int64_t>(b) * 4;
    st[0] = active ? den : 0.f;
    st[1] = nr;
    st[2] = ncs;
    st[3] = tr;
  }
}

// Backward of the tail, one workgroup per graph, from the upstream gradients g [3,B] (times the coefficients):
//   g_tr[b] = -g_spec / 2m          (gradient with respect to trace(S^T A S); g_raw = g_tr I)
//   coef[b] = (alpha, beta) = (2 g_spec / (2m)^2, g_clu sqrt(K) / (n_b ||cs||))   dS_i += alpha d_i ca + beta cs
//   W[b]    = d ortho / d G (ortho_term_bwd; dS = S (W + W^T))
template <int T>
__global__ __launch_bounds__(T) void dmon_tail_bwd_kernel(const float* __restrict__ g, const float* __restrict__ stats,
                                                          const float* __restrict__ gram, int K, float sqrt_k,
                                                          float c_spec, float c_clu, float c_ort, int B,
                                                          float* __restrict__ g_raw, float* __restrict__ g_tr,
                                                          float* __restrict__ coef, float* __restrict__ W) {
  __shared__ float sh[2 * (T / 64)];
  const int b = blockIdx.x;
  const int64_t off = static_cast<int64_t>(b) * K * K;
  const float* st = stats + static_cast<int64_t>(b) * 4;
  const float den = st[0], nr = st[1], ncs = st[2];
  const float g_spec = g[b] * c_spec, g_clu = g[B + b] * c_clu, g_ort = g[2 * B + b] * c_ort;
  const float gt = den > 0.f ? -g_spec / den : 0.f;
  if (W && gram) ortho_term_bwd<T>(gram + off, K, g_ort, W + off, sh);
  if (g_raw)
    for (int i = threadIdx.x; i < K * K; i += T) g_raw[off + i] = (i / K == i % K) ? gt : 0.f;
  if (threadIdx.x == 0) {
    if (g_tr) g_tr[b] = gt;
    coef[2 * b] = den > 0.f ? 2.0f * g_spec / (den * den) : 0.f;
    coef[2 * b + 1] = ncs > 0.f ? g_clu * sqrt_k / (nr * ncs) : 0.f;
  }
}

// dS[row, k] (+)= alpha_b d_row ca[b,k] + beta_b cs[b,k]; b = row / N (padded) or batch[row] (un-padded)
__global__ __launch_bounds__(256) void dmon_ds_kernel(const float* __restrict__ deg, const float* __restrict__ ca,
                                                      const float* __restrict__ cs, const float* __restrict__ coef,
                                                      int64_t rows, int N, const int64_t* __restrict__ batch, int K,
                                                      int B, int accumulate, float* __restrict__ ds) {
  const int64_t total = rows * K;
  for (int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; idx < total;
       idx += 256ll * gridDim.x) {
    const int64_t row = idx / K;
    const int k = static_cast<int>(idx - row * K);
    const int64_t b = batch ? batch[row] : row / N;
    float v = 0.f;
    if (b >= 0 && b < B) {
      const float a = deg ? coef[2 * b] * deg[row] : 0.f;
      v = fmaf(a, ca[b * K + k], coef[2 * b + 1] * cs[b * K + k]);
    }
    ds[idx] = accumulate ? ds[idx] + v : v;
  }
}

// One workgroup per graph of a row-sorted edge list (edges edge_ptr[b] .. edge_ptr[b+1]): deg[b,j] = sum of w_e over the
// graph's edges whose key (row: out-degrees, col: in-degrees) is node ptr[b] + j, in edge order (staged through LDS).
__global__ __launch_bounds__(256) void dmon_edge_deg_kernel(const int64_t* __restrict__ key, const float* __restrict__ w,
                                                            const int64_t* __restrict__ node_ptr,
                                                            const int64_t* __restrict__ edge_ptr, int N,
                                                            float* __restrict__ deg) {
  __shared__ int sk[256];
  __shared__ float sw[256];
  const int b = blockIdx.x;
  const int64_t base = node_ptr[b], e0 = edge_ptr[b], e1 = edge_ptr[b + 1];
  float d[4] = {0.f, 0.f, 0.f, 0.f};  // nodes threadIdx.x + 256 q
  for (int64_t c = e0; c < e1; c += 256) {
    const int64_t e = c + threadIdx.x;
    const int64_t rel = e < e1 ? key[e] - base : -1;
    sk[threadIdx.x] = (rel >= 0 && rel < N) ? static_cast<int>(rel) : -1;
    sw[threadIdx.x] = e < e1 ? (w ? w[e] : 1.f) : 0.f;
    __syncthreads();
    const int n = e1 - c < 256 ? static_cast<int>(e1 - c) : 256;
    for (int i = 0; i < n; ++i) {
      const int j = sk[i] - static_cast<int>(threadIdx.x);
      if (j >= 0 && (j & 255) == 0 && j < 1024) d[j >> 8] += sw[i];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = threadIdx.x + 256 * q;
    if (j < N) deg[static_cast<int64_t>(b) * N + j] = d[q];
  }
}

int launch_part(const float* S, const float* deg, int64_t B, int64_t N, int64_t K, const int64_t* sizes,
                const uint8_t* mask, const int64_t* ptr, int64_t nsplit, float* part, hipStream_t stream) {
  const dim3 grid(static_cast<unsigned>(cdiv(K, 64)), static_cast<unsigned>(nsplit), static_cast<unsigned>(B));
  hipLaunchKernelGGL(dmon_part_kernel, grid, dim3(256), 0, stream, S, deg, static_cast<int>(N), static_cast<int>(K),
                     sizes, mask, ptr, static_cast<int>(nsplit), part);
  return TGP_OK;
}

}  // namespace
}  // namespace tgp

using namespace tgp;

extern "C" int tgp_dmon_dense_terms_f32(const float* A, const float* S, int64_t B, int64_t N, int64_t K,
                                        const int64_t* graph_sizes, const uint8_t* mask, int64_t nsplit, float* deg,
                                        float* part, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(B >= 0 && N >= 0 && K >= 1, TGP_ERR_INVALID, "tgp_dmon_dense_terms_f32: bad shape");
  TGP_REQUIRE(nsplit == cdiv(N, PART_ROWS) || (N == 0 && nsplit == 1), TGP_ERR_INVALID,
              "tgp_dmon_dense_terms_f32: nsplit must be ceil(N / 64)");
  if (B == 0) return TGP_OK;
  TGP_REQUIRE(S && part && (!A || deg), TGP_ERR_INVALID, "tgp_dmon_dense_terms_f32: null pointer");
  TGP_REQUIRE(B < 65536 && N < (1ll << 31) && K < 32768 && B * N < (1ll << 33) && nsplit < 65536, TGP_ERR_RANGE,
              "tgp_dmon_dense_terms_f32: too large");
  const int64_t rows = B * N;
  const float* ones = nullptr;  // deg = A 1
  if (A && rows > 0) TGP_LAUNCH_A_ROWS(false, A, ones, rows, static_cast<int>(N), graph_sizes, mask, deg, stream);
  launch_part(S, deg, B, N, K, graph_sizes, mask, nullptr, nsplit, part, stream);
  return check_launch("tgp_dmon_dense_terms_f32");
}

extern "C" int tgp_dmon_edge_degrees_f32(const int64_t* key, const float* w, int64_t E, const int64_t* node_ptr,
                                         const int64_t* edge_ptr, int64_t B, int64_t N, float* deg, void* stream_) {
  TGP_REQUIRE(B >= 0 && N >= 0 && E >= 0, TGP_ERR_INVALID, "tgp_dmon_edge_degrees_f32: negative size");
  if (B == 0 || N == 0) return TGP_OK;
  TGP_REQUIRE(node_ptr && edge_ptr && deg && (E == 0 || key), TGP_ERR_INVALID, "tgp_dmon_edge_degrees_f32: null pointer");
  TGP_REQUIRE(N <= 1024 && B < (1ll << 31), TGP_ERR_RANGE, "tgp_dmon_edge_degrees_f32: at most 1024 nodes per graph");
  hipLaunchKernelGGL(dmon_edge_deg_kernel, dim3(static_cast<unsigned>(B)), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), key, w, node_ptr, edge_ptr, static_cast<int>(N), deg);
  return check_launch("tgp_dmon_edge_degrees_f32");
}

extern "C" int tgp_dmon_node_terms_f32(const float* S, const float* deg, const int64_t* ptr, int64_t B, int64_t K,
                                       int64_t nsplit, float* part, void* stream_) {
  TGP_REQUIRE(B >= 0 && K >= 1 && nsplit >= 1, TGP_ERR_INVALID, "tgp_dmon_node_terms_f32: bad shape");
  if (B == 0) return TGP_OK;
  TGP_REQUIRE(S && ptr && part, TGP_ERR_INVALID, "tgp_dmon_node_terms_f32: null pointer");
  TGP_REQUIRE(B < 65536 && K < 32768 && nsplit < 65536, TGP_ERR_RANGE, "tgp_dmon_node_terms_f32: too large");
  launch_part(S, deg, B, 0, K, nullptr, nullptr, ptr, nsplit, part, static_cast<hipStream_t>(stream_));
  return check_launch("tgp_dmon_node_terms_f32");
}

extern "C" int tgp_dmon_loss_terms_f32(const float* part, int64_t nsplit, const float* raw, const float* tr,
                                       const float* gram, int64_t B, int64_t K, float sqrt_k, int clamp_m, float eps,
                                       float c_spec, float c_clu, float c_ort, float* out, float* ca, float* cs,
                                       float* stats, void* stream_) {
  TGP_REQUIRE(B >= 0 && K >= 1 && K < 32768 && nsplit >= 1, TGP_ERR_INVALID, "tgp_dmon_loss_terms_f32: bad shape");
  if (B == 0) return TGP_OK;
  TGP_REQUIRE(part && out && ca && cs && stats, TGP_ERR_INVALID, "tgp_dmon_loss_terms_f32: null pointer");
  TGP_REQUIRE(B < (1ll << 31) && nsplit < 65536, TGP_ERR_RANGE, "tgp_dmon_loss_terms_f32: too many graphs");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_LAUNCH_PER_GRAPH(dmon_tail_kernel, B, K, stream, part, static_cast<int>(nsplit), raw, tr, gram, static_cast<int>(K),
                       sqrt_k, clamp_m, eps, c_spec, c_clu, c_ort, static_cast<int>(B), out, ca, cs, stats);
  return check_launch("tgp_dmon_loss_terms_f32");
}

extern "C" int tgp_dmon_loss_terms_bwd_f32(const float* g_terms, const float* stats, const float* gram, int64_t B,
                                           int64_t K, float sqrt_k, float c_spec, float c_clu, float c_ort, float* g_raw,
                                           float* g_tr, float* coef, float* W, void* stream_) {
  TGP_REQUIRE(B >= 0 && K >= 1 && K < 32768, TGP_ERR_INVALID, "tgp_dmon_loss_terms_bwd_f32: bad shape");
  if (B == 0) return TGP_OK;
  TGP_REQUIRE(g_terms && stats && coef && (!gram || W), TGP_ERR_INVALID, "tgp_dmon_loss_terms_bwd_f32: null pointer");
  TGP_REQUIRE(B < (1ll << 31), TGP_ERR_RANGE, "tgp_dmon_loss_terms_bwd_f32: too many graphs");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_LAUNCH_PER_GRAPH(dmon_tail_bwd_kernel, B, K, stream, g_terms, stats, gram, static_cast<int>(K), sqrt_k, c_spec,
                       c_clu, c_ort, static_cast<int>(B), g_raw, g_tr, coef, W);
  return check_launch("tgp_dmon_loss_terms_bwd_f32");
}

extern "C" int tgp_dmon_ds_f32(const float* deg, const float* ca, const float* cs, const float* coef, int64_t rows,
                               int64_t N, const int64_t* batch, int64_t B, int64_t K, int accumulate, float* ds,
                               void* stream_) {
  TGP_REQUIRE(rows >= 0 && B >= 0 && K >= 1 && (batch || N >= 1), TGP_ERR_INVALID, "tgp_dmon_ds_f32: bad shape");
  if (rows == 0) return TGP_OK;
  TGP_REQUIRE(ca && cs && coef && ds, TGP_ERR_INVALID, "tgp_dmon_ds_f32: null pointer");
  TGP_REQUIRE(N < (1ll << 31) && K < 32768 && B < (1ll << 31) && rows < (1ll << 40), TGP_ERR_RANGE,
              "tgp_dmon_ds_f32: too large");
  const int64_t total = rows * K;
  const int64_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(dmon_ds_kernel, dim3(static_cast<unsigned>(blocks < 65536 ? blocks : 65536)), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), deg, ca, cs, coef, rows, static_cast<int>(N), batch,
                     static_cast<int>(K), static_cast<int>(B), accumulate, ds);
  return check_launch("tgp_dmon_ds_f32");
}
