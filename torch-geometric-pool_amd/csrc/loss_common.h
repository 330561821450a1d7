// What the dense-loss kernels (losses.hip, dmon.hip, hosc.hip, asym_cheeger.hip, just_balance.hip) share: the fixed-order block sums, the
// orthogonality term and its gradient, the rows a graph owns, the streaming row pass over a padded A, and the launch of a
// one-workgroup-per-graph tail.  Templates, inline device functions and launch macros only: nothing lands in a code
// object that does not use it, and no kernel instantiation is in two of them.
#pragma once
#include "common.h"

namespace tgp {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int PART_ROWS = 64;  // rows of one graph per workgroup of a partial pass (dmon_part_kernel, hosc_part_kernel, jb_part_kernel)

// ---- the orthogonality term || G / ||G||_F - I / sqrt(K) ||_F of one graph (utils/losses.py:59-70) -----------------
// T threads, G [K,K]; sq = ||G||_F^2, which the caller reduces beside its other sums.  sh: T / 64 floats.
template <int T>
__device__ __forceinline__ float ortho_term(const float* __restrict__ G, int K, float sq, float* sh) {
  const float n = sqrtf(sq);
  const float t = 1.0f / sqrtf(static_cast<float>(K));
  float acc = 0.f;
  for (int i = threadIdx.x; i < K * K; i += T) {
    const float y = G[i] / n - ((i / K == i % K) ? t : 0.f);
    acc = fmaf(y, y, acc);
  }
  return sqrtf(block_sum<T>(acc, sh));
}

// Its gradient times the upstream g: W = g / (|Y| |G|) (Y - G <G,Y> / |G|^2), Y = G / |G| - I / sqrt(K); W = 0 when
// |Y| = 0 (dS = S (W + W^T)).  sh: 2 * T / 64 floats.
template <int T>
__device__ __forceinline__ void ortho_term_bwd(const float* __restrict__ G, int K, float g, float* __restrict__ W,
                                               float* sh) {
  float sq = 0.f;
  for (int i = threadIdx.x; i < K * K; i += T) sq = fmaf(G[i], G[i], sq);
  sq = block_sum<T>(sq, sh);
  const float n = sqrtf(sq);
  const float t = 1.0f / sqrtf(static_cast<float>(K));
  float v[2] = {0.f, 0.f};  // |Y|^2, <G, Y>
  for (int i = threadIdx.x; i < K * K; i += T) {
    const float y = G[i] / n - ((i / K == i % K) ? t : 0.f);
    v[0] = fmaf(y, y, v[0]);
    v[1] = fmaf(G[i], y, v[1]);
  }
  block_sums<T, 2>(v, sh);
  const float ny = sqrtf(v[0]), gy = v[1];
  const float cw = ny > 0.f ? g / (ny * n) : 0.f;
  for (int i = threadIdx.x; i < K * K; i += T) {
    const float y = G[i] / n - ((i / K == i % K) ? t : 0.f);
    W[i] = cw * (y - G[i] * (gy / sq));
  }
}

// ---- rows of S (deg, mask ...) that graph b owns -------------------------------------------------------------------
// un-padded (ptr): ptr[b] .. ptr[b+1]; padded (ptr NULL): b N .. + the graph's size clamped to 0 .. N (N without sizes).
// A negative size owns no rows: every caller walks i = 0 .. count - 1, so the clamp at 0 changes nothing for those that
// did without it.
template <typename C>
__device__ __forceinline__ void graph_rows(int b, int N, const int64_t* sizes, const int64_t* ptr, int64_t& start,
                                           C& count) {
  if (ptr) {
    start = ptr[b];
    count = static_cast<C>(ptr[b + 1] - start);
  } else {
    start = static_cast<int64_t>(b) * N;
    int64_t c = sizes ? sizes[b] : N;
    c = c < 0 ? 0 : (c > N ? N : c);
    count = static_cast<C>(c);
  }
}

// ---- the streaming row pass over a padded A [B,N,N] ----------------------------------------------------------------
// G lanes per node row: y[b,i] = sum_j A[b,i,j] v[b,j] (v NULL: ones, the degrees) on real rows (graph size, mask), 0
// elsewhere; 256 / G rows per workgroup.  16-byte non-temporal loads of A when N % 4 == 0 and A, v are 16-byte aligned,
// element loads otherwise; v (4 N bytes per graph) stays in cache.  The columns are not cut at the graph size: a
// zero-padded A adds nothing there, a caller's own padding counts as it does in the reference's A A A.
// V = false: the caller never has a vector (DMoN's degrees) and v is not looked at; that instantiation carries no code
// for it (with it, the degree pass behind two passes over the same A measured 2 us slower on 134 MB).  The two callers
// instantiate different V, so each instantiation is in one code object.
// (cut_rows_kernel in losses.hip is the same walk with ||S_i||^2 from the same lanes; it stays a kernel of its own.)
template <int G, bool V>
__global__ __launch_bounds__(256) void a_rows_kernel(const float* __restrict__ A, const float* __restrict__ v,
                                                     int64_t rows, int N, const int64_t* __restrict__ sizes,
                                                     const uint8_t* __restrict__ mask, float* __restrict__ y) {
  const int sub = threadIdx.x % G;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * (256 / G) + threadIdx.x / G;
  float d = 0.f;
  const bool real = row < rows && (!sizes || row % N < sizes[row / N]) && (!mask || mask[row]);
  if (real) {
    const float* a = A + row * N;
    const float* x = (V && v) ? v + (row / N) * N : nullptr;
    if ((N & 3) == 0 && reinterpret_cast<uintptr_t>(A) % 16 == 0 && (!V || reinterpret_cast<uintptr_t>(v) % 16 == 0)) {
      const f32x4* a4 = reinterpret_cast<const f32x4*>(a);
      const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
      if (x) {
        for (int j = sub; j < N / 4; j += G) {
          const f32x4 p = __builtin_nontemporal_load(a4 + j);
          const f32x4 q = x4[j];
          d += (p.x * q.x + p.y * q.y) + (p.z * q.z + p.w * q.w);
        }
      } else {
        for (int j = sub; j < N / 4; j += G) {
          const f32x4 p = __builtin_nontemporal_load(a4 + j);
          d += (p.x + p.y) + (p.z + p.w);
        }
      }
    } else if (x) {
      for (int j = sub; j < N; j += G) d = fmaf(a[j], x[j], d);
    } else {
      for (int j = sub; j < N; j += G) d += a[j];
    }
  }
  // the order of wave_sum<G> (wave.h), written out: a call here changes the kernel's instruction stream
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
  if (row < rows && sub == 0) y[row] = d;
}

// G = 64 for long rows; batches of small graphs (N <= 64: a row is at most 16 float4) use G = 16, four rows per wave.
// (A macro, as the launch below: a function here would instantiate the kernel in every file that includes this one.)
#define TGP_LAUNCH_A_ROWS(V, A, v, rows, N, sizes, mask, y, stream)                                                     \
  do {                                                                                                                  \
    if ((N) <= 64)                                                                                                      \
      hipLaunchKernelGGL((a_rows_kernel<16, V>), dim3(cdiv(rows, 16)), dim3(256), 0, stream, A, v, rows, N, sizes,      \
                         mask, y);                                                                                      \
    else                                                                                                                \
      hipLaunchKernelGGL((a_rows_kernel<64, V>), dim3(cdiv(rows, 4)), dim3(256), 0, stream, A, v, rows, N, sizes, mask, \
                         y);                                                                                            \
  } while (0)

// ---- one workgroup per graph: 1024 threads for K >= 64 (few graphs, K^2 elements each: the 256-thread form of MinCut's
// tail took 28 us at B = 32, K = 128), 256 below
#define TGP_LAUNCH_PER_GRAPH(kernel, B, K, stream, ...)                                                                 \
  do {                                                                                                                  \
    if ((K) >= 64)                                                                                                      \
      hipLaunchKernelGGL(kernel<1024>, dim3(static_cast<unsigned>(B)), dim3(1024), 0, stream, __VA_ARGS__);             \
    else                                                                                                                \
      hipLaunchKernelGGL(kernel<256>, dim3(static_cast<unsigned>(B)), dim3(256), 0, stream, __VA_ARGS__);               \
  } while (0)

}  // namespace tgp
