// Just Balance pooling's auxiliary loss (reference poolers/just_balance.py, utils/losses.py:553-594, 1013-1080):
//
//   L[b] = -sum_k sqrt(c_k + eps) / denom_b * scale        c_k = sum_i S_ik^2        denom_b = sqrt(n_b K) or 1
//
// The reference forms S^T S, adds eps, takes the elementwise square root and keeps the trace: only the diagonal
// survives, and only the diagonal is computed here.  The column sums are reduced in two stages as DMoN's and HOSC's
// are: every workgroup of the partial pass writes the sums over its PART_ROWS rows, the tail adds the partials of a
// graph in split order (no float atomics; every addition has a fixed place).  A batch whose graphs all fit one split
// gets both stages from ONE launch.  The tail also writes coef[b,k] = -scale / (sqrt(c_k + eps) denom_b), from which
// the backward is one elementwise pass dS = g_b coef_bk S (inference asks for no coef and, instead, for the batch mean
// from one more launch of the same call).
#include "loss_common.h"

namespace tgp {
namespace {

// The workgroup's 256 threads as 256 / L row groups of L lanes (L a power of two, at most 64): lane c of group r owns
// the column unit u = kc L + c (VEC4: four adjacent columns, one 16-byte load per row; else one column) and adds the
// squares of rows r, r + 256 / L, ... of the nrows rows at `rows` (row stride K).  The groups' sums meet in LDS and
// are added in ascending group order by the threads t < L, which leave with the unit's sums in a[].
template <bool VEC4>
__device__ __forceinline__ void jb_unit_sums(const float* __restrict__ rows, int nrows, int K, int L, int u, int U,
                                             float (*sh)[256], float (&a)[4]) {
  const int t = threadIdx.x;
  const int R = 256 / L;
  const int r = t / L;
  a[0] = a[1] = a[2] = a[3] = 0.f;
  if (u < U) {
    if (VEC4) {
      const f32x4* p = reinterpret_cast<const f32x4*>(rows) + u;
      const int ld = K >> 2;
#pragma unroll 4
      for (int i = r; i < nrows; i += R) {
        const f32x4 s = p[static_cast<int64_t>(i) * ld];
        a[0] = fmaf(s.x, s.x, a[0]);
        a[1] = fmaf(s.y, s.y, a[1]);
        a[2] = fmaf(s.z, s.z, a[2]);
        a[3] = fmaf(s.w, s.w, a[3]);
      }
    } else {
#pragma unroll 4
      for (int i = r; i < nrows; i += R) {
        const float s = rows[static_cast<int64_t>(i) * K + u];
        a[0] = fmaf(s, s, a[0]);
      }
    }
  }
  __syncthreads();  // (the reads of the previous unit are done)
#pragma unroll
  for (int q = 0; q < (VEC4 ? 4 : 1); ++q) sh[q][t] = a[q];
  __syncthreads();
  if (t < L) {
#pragma unroll
    for (int q = 0; q < (VEC4 ? 4 : 1); ++q) {
      float s = 0.f;
      for (int g = 0; g < R; ++g) s += sh[q][g * L + t];
      a[q] = s;
    }
  }
}

// Real nodes of graph b as the reference counts them: the graph's rows when un-padded, else the mask's true entries
// among the N padded rows, else the graph's size, else the caller's scalar.  T threads; sh: T / 64 floats.  Uniform
// over the workgroup (block_sum holds barriers).
template <int T>
__device__ __forceinline__ float jb_real_nodes(int b, int N, int64_t count, const int64_t* __restrict__ sizes,
                                               const uint8_t* __restrict__ mask, const int64_t* __restrict__ ptr,
                                               float n_scalar, float* sh) {
  if (ptr) return static_cast<float>(count);
  if (mask) {
    const uint8_t* m = mask + static_cast<int64_t>(b) * N;
    int c = 0;
    for (int i = threadIdx.x; i < N; i += T) c += m[i] ? 1 : 0;
    return block_sum<T>(static_cast<float>(c), sh);  // (whole numbers below 2^24: exact in any order)
  }
  return sizes ? static_cast<float>(count) : n_scalar;
}

// One workgroup per (graph, PART_ROWS rows): part[b][split][K] = column sums of squares of the split's rows.  Graph b
// owns rows start .. start + count of S (loss_common.h graph_rows: padded with ptr NULL, un-padded with ptr).
template <bool VEC4>
__global__ __launch_bounds__(256) void jb_part_kernel(const float* __restrict__ S, int N, int K, int L,
                                                      const int64_t* __restrict__ sizes,
                                                      const int64_t* __restrict__ ptr, int nsplit,
                                                      float* __restrict__ part) {
  __shared__ float sh[4][256];
  const int b = blockIdx.x / nsplit, split = blockIdx.x - b * nsplit;
  int64_t start, count;
  graph_rows(b, N, sizes, ptr, start, count);
  const int64_t lo = static_cast<int64_t>(split) * PART_ROWS;
  const int64_t hi = count < lo + PART_ROWS ? count : lo + PART_ROWS;
  const int nrows = hi > lo ? static_cast<int>(hi - lo) : 0;
  const float* rows = S + (start + lo) * K;
  float* out = part + static_cast<int64_t>(blockIdx.x) * K;
  const int U = VEC4 ? K >> 2 : K;
  const int c = threadIdx.x & (L - 1);
  for (int u0 = 0; u0 < U; u0 += L) {
    const int u = u0 + c;
    float a[4];
    jb_unit_sums<VEC4>(rows, nrows, K, L, u, U, sh, a);
    if (threadIdx.x < L && u < U) {
      if (VEC4) {
        f32x4 v = {a[0], a[1], a[2], a[3]};
        *reinterpret_cast<f32x4*>(out + 4 * u) = v;
      } else {
        out[u] = a[0];
      }
    }
  }
}

// One workgroup per graph: the partials of every column added in ascending split order, sqrt(c_k + eps) summed over k
// (thread-strided, then block_sums' order), divided by denom_b, times scale.
template <int T>
__global__ __launch_bounds__(T) void jb_tail_kernel(const float* __restrict__ part, int nsplit, int N, int K,
                                                    const int64_t* __restrict__ sizes,
                                                    const uint8_t* __restrict__ mask,
                                                    const int64_t* __restrict__ ptr, int normalize, float n_scalar,
                                                    float k_den, float eps, float scale, float* __restrict__ out,
                                                    float* __restrict__ coef) {
  __shared__ float sh[T / 64];
  const int b = blockIdx.x;
  int64_t start, count;
  graph_rows(b, N, sizes, ptr, start, count);
  const float nb = jb_real_nodes<T>(b, N, count, sizes, mask, ptr, n_scalar, sh);
  const float denom = normalize ? sqrtf(nb * k_den) : 1.0f;
  const float* pb = part + static_cast<int64_t>(b) * nsplit * K;
  float acc = 0.f;
  for (int k = threadIdx.x; k < K; k += T) {
    float c = 0.f;
#pragma unroll 8
    for (int j = 0; j < nsplit; ++j) c += pb[static_cast<int64_t>(j) * K + k];
    const float r = sqrtf(c + eps);
    acc += r;
    if (coef) coef[static_cast<int64_t>(b) * K + k] = -scale / (r * denom);
  }
  const float total = block_sum<T>(acc, sh);
  if (threadIdx.x == 0) out[b] = (-total / denom) * scale;
}

// Both stages for a batch whose graphs have at most PART_ROWS rows each: one workgroup per graph.  (One graph per
// workgroup although K is small: 2048 graphs are 2048 workgroups of four waves, eight per CU, and every workgroup
// keeps the barriers of the block sums to itself; packing four graphs into one would save no launch.)
template <bool VEC4>
__global__ __launch_bounds__(256) void jb_one_kernel(const float* __restrict__ S, int N, int K, int L,
                                                     const int64_t* __restrict__ sizes,
                                                     const uint8_t* __restrict__ mask,
                                                     const int64_t* __restrict__ ptr, int normalize, float n_scalar,
                                                     float k_den, float eps, float scale, float* __restrict__ out,
                                                     float* __restrict__ coef) {
  __shared__ float sh[4][256];
  __shared__ float sh_sum[4];
  const int b = blockIdx.x;
  int64_t start, count;
  graph_rows(b, N, sizes, ptr, start, count);
  const int nrows = count < PART_ROWS ? static_cast<int>(count) : PART_ROWS;
  const float nb = jb_real_nodes<256>(b, N, count, sizes, mask, ptr, n_scalar, sh_sum);
  const float denom = normalize ? sqrtf(nb * k_den) : 1.0f;
  const float* rows = S + start * K;
  float* cb = coef ? coef + static_cast<int64_t>(b) * K : nullptr;
  const int U = VEC4 ? K >> 2 : K;
  const int c = threadIdx.x & (L - 1);
  float acc = 0.f;
  for (int u0 = 0; u0 < U; u0 += L) {
    const int u = u0 + c;
    float a[4];
    jb_unit_sums<VEC4>(rows, nrows, K, L, u, U, sh, a);
    if (threadIdx.x < L && u < U) {
#pragma unroll
      for (int q = 0; q < (VEC4 ? 4 : 1); ++q) {
        const float r = sqrtf(a[q] + eps);
        acc += r;
        if (cb) cb[(VEC4 ? 4 * u : u) + q] = -scale / (r * denom);
      }
    }
  }
  const float total = block_sum<256>(acc, sh_sum);
  if (threadIdx.x == 0) out[b] = (-total / denom) * scale;
}

// mean[0] = sum_b out[b] / B: thread t adds out[t], out[t + 256], ..., then block_sums' order (one workgroup)
__global__ __launch_bounds__(256) void jb_mean_kernel(const float* __restrict__ out, int B, float* __restrict__ mean) {
  __shared__ float sh[4];
  float acc = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) acc += out[b];
  const float total = block_sum<256>(acc, sh);
  if (threadIdx.x == 0) mean[0] = total / static_cast<float>(B);
}

// dS[row, k] = g_b coef[b, k] S[row, k]; b = batch[row] (un-padded) or row / N (padded); g one value when g_bcast.
// A row whose graph is outside 0 .. B gets 0.
template <bool VEC4>
__global__ __launch_bounds__(256) void jb_ds_kernel(const float* __restrict__ S, const float* __restrict__ coef,
                                                    const float* __restrict__ g, int g_bcast, int64_t rows, int N,
                                                    const int64_t* __restrict__ batch, int B, int K,
                                                    float* __restrict__ ds) {
  constexpr int V = VEC4 ? 4 : 1;
  const int64_t total = rows * K / V;
  for (int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; idx < total; idx += 256ll * gridDim.x) {
    const int64_t e = idx * V;
    const int64_t row = e / K;
    const int k = static_cast<int>(e - row * K);
    const int64_t b = batch ? batch[row] : row / N;
    const bool in = b >= 0 && b < B;
    const float gb = in ? g[g_bcast ? 0 : b] : 0.f;
    if (VEC4) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (in) {
        const f32x4 s = *reinterpret_cast<const f32x4*>(S + e);
        const f32x4 cf = *reinterpret_cast<const f32x4*>(coef + b * K + k);
        v.x = gb * cf.x * s.x;
        v.y = gb * cf.y * s.y;
        v.z = gb * cf.z * s.z;
        v.w = gb * cf.w * s.w;
      }
      *reinterpret_cast<f32x4*>(ds + e) = v;
    } else {
      ds[e] = in ? gb * coef[b * K + k] * S[e] : 0.f;
    }
  }
}

// lanes of a row group: the smallest power of two that covers the U column units of a row, at most a wave
int unit_lanes(int64_t U) {
  int L = 1;
  while (L < 64 && L < U) L <<= 1;
  return L;
}

bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

}  // namespace
}  // namespace tgp

using namespace tgp;

extern "C" int tgp_jb_terms_f32(const float* S, int64_t B, int64_t N, int64_t K, const int64_t* graph_sizes,
                                const uint8_t* mask, const int64_t* ptr, int64_t max_rows, int normalize,
                                float num_nodes, float num_supernodes, float eps, float scale, float* part, float* out,
                                float* coef, float* mean, void* stream_) {
  TGP_REQUIRE(B >= 0 && N >= 0 && K >= 1 && max_rows >= 0, TGP_ERR_INVALID, "tgp_jb_terms_f32: bad shape");
  TGP_REQUIRE(!ptr || (!graph_sizes && !mask), TGP_ERR_INVALID,
              "tgp_jb_terms_f32: an un-padded batch (ptr) takes neither graph sizes nor a mask");
  TGP_REQUIRE(ptr || max_rows == N, TGP_ERR_INVALID, "tgp_jb_terms_f32: a padded batch has max_rows = N");
  if (B == 0) return TGP_OK;
  TGP_REQUIRE(S && out, TGP_ERR_INVALID, "tgp_jb_terms_f32: null pointer");
  const int64_t nsplit = max_rows > PART_ROWS ? (max_rows + PART_ROWS - 1) / PART_ROWS : 1;
  TGP_REQUIRE(nsplit == 1 || part, TGP_ERR_INVALID, "tgp_jb_terms_f32: graphs beyond one split need the part buffer");
  TGP_REQUIRE(B < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31) && max_rows < (1ll << 31) &&
                  B * nsplit < (1ll << 31) && (!mask || N < (1ll << 24)),
              TGP_ERR_RANGE, "tgp_jb_terms_f32: too large");
  TGP_REQUIRE(aligned(S, 4) && aligned(out, 4) && aligned(coef, 4) && aligned(part, 4) && aligned(mean, 4) &&
                  aligned(ptr, 8) && aligned(graph_sizes, 8),
              TGP_ERR_INVALID, "tgp_jb_terms_f32: misaligned pointer");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int Ni = static_cast<int>(N), Ki = static_cast<int>(K), ns = static_cast<int>(nsplit);
  // 16-byte loads: every row of S starts on a 16-byte boundary (and so do the rows of part and coef the kernels write)
  const bool vec = (K & 3) == 0 && aligned(S, 16) && aligned(coef, 16) && aligned(part, 16);
  const int L = unit_lanes(vec ? K / 4 : K);
  if (nsplit == 1) {
    if (vec)
      hipLaunchKernelGGL(jb_one_kernel<true>, dim3(static_cast<unsigned>(B)), dim3(256), 0, stream, S, Ni, Ki, L,
                         graph_sizes, mask, ptr, normalize, num_nodes, num_supernodes, eps, scale, out, coef);
    else
      hipLaunchKernelGGL(jb_one_kernel<false>, dim3(static_cast<unsigned>(B)), dim3(256), 0, stream, S, Ni, Ki, L,
                         graph_sizes, mask, ptr, normalize, num_nodes, num_supernodes, eps, scale, out, coef);
  } else {
    const dim3 grid(static_cast<unsigned>(B * nsplit));
    if (vec)
      hipLaunchKernelGGL(jb_part_kernel<true>, grid, dim3(256), 0, stream, S, Ni, Ki, L, graph_sizes, ptr, ns, part);
    else
      hipLaunchKernelGGL(jb_part_kernel<false>, grid, dim3(256), 0, stream, S, Ni, Ki, L, graph_sizes, ptr, ns, part);
    TGP_LAUNCH_PER_GRAPH(jb_tail_kernel, B, K, stream, part, ns, Ni, Ki, graph_sizes, mask, ptr, normalize, num_nodes,
                         num_supernodes, eps, scale, out, coef);
  }
  if (mean) hipLaunchKernelGGL(jb_mean_kernel, dim3(1), dim3(256), 0, stream, out, static_cast<int>(B), mean);
  return check_launch("tgp_jb_terms_f32");
}

extern "C" int tgp_jb_ds_f32(const float* S, const float* coef, const float* g, int g_bcast, int64_t rows, int64_t N,
                             const int64_t* batch, int64_t B, int64_t K, float* ds, void* stream_) {
  TGP_REQUIRE(rows >= 0 && B >= 0 && K >= 1 && (batch || N >= 1), TGP_ERR_INVALID, "tgp_jb_ds_f32: bad shape");
  if (rows == 0) return TGP_OK;
  TGP_REQUIRE(S && coef && g && ds, TGP_ERR_INVALID, "tgp_jb_ds_f32: null pointer");
  TGP_REQUIRE(N < (1ll << 31) && K < (1ll << 31) && B < (1ll << 31) && rows < (1ll << 40) && rows * K < (1ll << 46),
              TGP_ERR_RANGE, "tgp_jb_ds_f32: too large");
  TGP_REQUIRE(aligned(S, 4) && aligned(coef, 4) && aligned(g, 4) && aligned(ds, 4) && aligned(batch, 8), TGP_ERR_INVALID,
              "tgp_jb_ds_f32: misaligned pointer");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const bool vec = (K & 3) == 0 && aligned(S, 16) && aligned(coef, 16) && aligned(ds, 16);
  const int64_t total = rows * K / (vec ? 4 : 1);
  const int64_t blocks = (total + 255) / 256;
  const dim3 grid(static_cast<unsigned>(blocks < 65536 ? blocks : 65536));
  if (vec)
    hipLaunchKernelGGL(jb_ds_kernel<true>, grid, dim3(256), 0, stream, S, coef, g, g_bcast, rows, static_cast<int>(N),
                       batch, static_cast<int>(B), static_cast<int>(K), ds);
  else
    hipLaunchKernelGGL(jb_ds_kernel<false>, grid, dim3(256), 0, stream, S, coef, g, g_bcast, rows, static_cast<int>(N),
                       batch, static_cast<int>(B), static_cast<int>(K), ds);
  return check_launch("tgp_jb_ds_f32");
}
