// SAGPooling's scorer (reference poolers/sag.py:199-202 with PyG's GraphConv / SAGEConv at one output channel):
//   a_i = act( lin_rel( aggr_{e: dst(e) = i} x_src(e) ) + lin_root(x_i) ).
// One output channel makes projection and aggregation commute, so nothing of size E x F or N x F is formed:
//   p_i = <x_i, w_rel>, q_i = <x_i, w_root>                 one pass over X           (row_project2_kernel)
//   t_i = (sum_{e: dst(e) = i} p_src(e) [/ max(indeg_i, 1)] + b) + q_i,  a_i = act(t_i)  E scalar gathers (sag_aggregate_kernel)
// The sums run in edge-list order inside a node over a by-destination index (no float atomics: the score decides a
// top-k, the same bits on every call).  The backward is the same aggregate over the by-source index plus one pass that
// writes dX = g_q (x) w_root + g_p (x) w_rel (sag_score_bwd_x_kernel).
#include "common.h"

namespace tgp {
namespace {

// Both dot products of a row from one read of it.  Lane layout and loads are row_dot_kernel's (csrc/topk_select.hip): G
// lanes share a row, a float4 each when VEC (16-byte aligned base, row stride a multiple of 4), both weight rows in
// registers.  A row whose length is no multiple of 4 ends in scalar loads.
template <int G, bool VEC>
__global__ __launch_bounds__(256) void row_project2_kernel(const float* __restrict__ x, int64_t n, int F, int64_t ldx,
                                                           const float* __restrict__ w0, const float* __restrict__ w1,
                                                           float* __restrict__ out0, float* __restrict__ out1) {
  constexpr int PER_WAVE = 64 / G;
  constexpr int MAXC = 8;  // column chunks per lane kept in registers (covers F <= G*4*8)
  constexpr int W = VEC ? 4 : 1;
  constexpr int STEP = G * W;
  const int lane = threadIdx.x & 63, sub = lane % G, slot = lane / G;
  const int64_t wave = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * 4;
  float wa[MAXC][W], wb[MAXC][W];
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int k = sub * W + c * STEP;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      wa[c][j] = (k + j < F) ? w0[k + j] : 0.f;
      wb[c][j] = (k + j < F) ? w1[k + j] : 0.f;
    }
  }
  for (int64_t base = wave * PER_WAVE; base < n; base += nwaves * PER_WAVE) {
    const int64_t i = base + slot;
    float acc0 = 0.f, acc1 = 0.f;
    if (i < n) {
      const float* a = x + i * ldx;
#pragma unroll
      for (int c = 0; c < MAXC; ++c) {
        const int k = sub * W + c * STEP;
        if (k >= F) break;
        if constexpr (VEC) {
          if (k + 4 <= F) {
            const float4 v = *reinterpret_cast<const float4*>(a + k);
            acc0 = fmaf(v.x, wa[c][0], acc0); acc0 = fmaf(v.y, wa[c][1], acc0);
            acc0 = fmaf(v.z, wa[c][2], acc0); acc0 = fmaf(v.w, wa[c][3], acc0);
            acc1 = fmaf(v.x, wb[c][0], acc1); acc1 = fmaf(v.y, wb[c][1], acc1);
            acc1 = fmaf(v.z, wb[c][2], acc1); acc1 = fmaf(v.w, wb[c][3], acc1);
          } else {  // the row's last, partial chunk
#pragma unroll
            for (int j = 0; j < 3; ++j) {
              if (k + j < F) {
                const float v = a[k + j];
                acc0 = fmaf(v, wa[c][j], acc0);
                acc1 = fmaf(v, wb[c][j], acc1);
              }
            }
          }
        } else {
          const float v = a[k];
          acc0 = fmaf(v, wa[c][0], acc0);
          acc1 = fmaf(v, wb[c][0], acc1);
        }
      }
      for (int k = sub * W + MAXC * STEP; k < F; k += STEP) {  // very wide rows
#pragma unroll
        for (int j = 0; j < W; ++j) {
          if (k + j < F) {
            const float v = a[k + j];
            acc0 = fmaf(v, w0[k + j], acc0);
            acc1 = fmaf(v, w1[k + j], acc1);
          }
        }
      }
    }
    // the order of wave_butterfly<G> (wave.h), written out: a call here changes the kernel's instruction stream
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
      acc0 += __shfl_xor(acc0, off);
      acc1 += __shfl_xor(acc1, off);
    }
    if (i < n && sub == 0) {
      out0[i] = acc0;
      out1[i] = acc1;
    }
  }
}

template <int G, bool VEC>
void launch_row_project2(const float* x, int64_t n, int F, int64_t ldx, const float* w0, const float* w1, float* out0,
                         float* out1, hipStream_t stream) {
  int64_t blocks = cdiv(n, static_cast<int64_t>(4) * (64 / G));
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL((row_project2_kernel<G, VEC>), dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, x, n, F,
                     ldx, w0, w1, out0, out1);
}

// One lane per node: t_i = (sum over the node's group of p[src] [/ max(group size, 1)] + b) + q_i in the order of the
// index (= edge-list order inside a group).  A source outside [0, n) is skipped and never dereferenced; offsets and
// positions outside the edge list are clamped / skipped the same way.
__global__ __launch_bounds__(256) void sag_aggregate_kernel(const int32_t* __restrict__ grp_ptr,
                                                            const int32_t* __restrict__ grp_perm,
                                                            const int64_t* __restrict__ src,
                                                            const float* __restrict__ p, const float* __restrict__ q,
                                                            const float* __restrict__ bias, int64_t n, int64_t E,
                                                            int mean, int act, float* __restrict__ t_out,
                                                            float* __restrict__ a_out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  int64_t b = grp_ptr[i], e = grp_ptr[i + 1];
  if (b < 0) b = 0;
  if (e > E) e = E;
  float acc = 0.0f;
  for (int64_t j = b; j < e; ++j) {
    const int64_t pos = grp_perm ? static_cast<int64_t>(grp_perm[j]) : j;
    if (static_cast<uint64_t>(pos) >= static_cast<uint64_t>(E)) continue;
    const int64_t r = src[pos];
    if (static_cast<uint64_t>(r) < static_cast<uint64_t>(n)) acc = acc + p[r];
  }
  if (mean) acc = acc / static_cast<float>(e - b > 1 ? e - b : 1);
  float t = acc + (bias ? bias[0] : 0.0f);
  if (q) t = t + q[i];
  if (t_out) t_out[i] = t;
  if (a_out) a_out[i] = act ? tanhf(t) : t;
}

// dX[i,:] (+)= g_q[i] w_root + g_p[i] w_rel: one pass over dX, a float4 per lane when F % 4 == 0 and dX is 16-byte
// aligned (rows are contiguous).
template <bool VEC>
__global__ __launch_bounds__(256) void sag_score_bwd_x_kernel(const float* __restrict__ g_q,
                                                              const float* __restrict__ g_p,
                                                              const float* __restrict__ w_root,
                                                              const float* __restrict__ w_rel, int64_t n, int F,
                                                              int accumulate, float* __restrict__ g_x) {
  constexpr int W = VEC ? 4 : 1;
  const int chunks = F / W;
  const int64_t total = n * chunks;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
  for (int64_t u = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; u < total; u += stride) {
    const int64_t i = u / chunks;
    const int k = static_cast<int>(u - i * chunks) * W;
    const float gq = g_q[i], gp = g_p[i];
    float* dst = g_x + i * F + k;
    if constexpr (VEC) {
      const float4 wr = *reinterpret_cast<const float4*>(w_root + k);
      const float4 wl = *reinterpret_cast<const float4*>(w_rel + k);
      float4 o = make_float4(gq * wr.x + gp * wl.x, gq * wr.y + gp * wl.y, gq * wr.z + gp * wl.z,
                             gq * wr.w + gp * wl.w);
      if (accumulate) {
        const float4 old = *reinterpret_cast<const float4*>(dst);
        o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w;
      }
      *reinterpret_cast<float4*>(dst) = o;
    } else {
      float o = gq * w_root[k] + gp * w_rel[k];
      if (accumulate) o += dst[0];
      dst[0] = o;
    }
  }
}

}  // namespace
}  // namespace tgp

using namespace tgp;

extern "C" int tgp_row_project2_f32(const float* x, int64_t N, int64_t F, int64_t ldx, const float* w0,
                                    const float* w1, float* out0, float* out1, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(N >= 0 && F >= 0 && ldx >= F, TGP_ERR_INVALID, "tgp_row_project2_f32: bad size");
  if (N == 0) return TGP_OK;
  TGP_REQUIRE(out0 && out1 && out0 != out1 && (F == 0 || (x && w0 && w1)), TGP_ERR_INVALID,
              "tgp_row_project2_f32: null pointer or one buffer for both outputs");
  TGP_REQUIRE(F < (1ll << 31), TGP_ERR_RANGE, "tgp_row_project2_f32: F too large");
  const int f = static_cast<int>(F);
  const bool vec = F >= 4 && (ldx % 4 == 0) && (reinterpret_cast<uintptr_t>(x) % 16 == 0);
  const int64_t units = vec ? (F + 3) / 4 : F;
  if (vec) {
    if (units <= 1) launch_row_project2<1, true>(x, N, f, ldx, w0, w1, out0, out1, stream);
    else if (units <= 2) launch_row_project2<2, true>(x, N, f, ldx, w0, w1, out0, out1, stream);
    else if (units <= 4) launch_row_project2<4, true>(x, N, f, ldx, w0, w1, out0, out1, stream);
    else if (units <= 8) launch_row_project2<8, true>(x, N, f, ldx, w0, w1, out0, out1, stream);
    else if (units <= 16) launch_row_project2<16, true>(x, N, f, ldx, w0, w1, out0, out1, stream);
    else if (units <= 32) launch_row_project2<32, true>(x, N, f, ldx, w0, w1, out0, out1, stream);
    else launch_row_project2<64, true>(x, N, f, ldx, w0, w1, out0, out1, stream);
  } else {
    if (units <= 4) launch_row_project2<4, false>(x, N, f, ldx, w0, w1, out0, out1, stream);
    else if (units <= 16) launch_row_project2<16, false>(x, N, f, ldx, w0, w1, out0, out1, stream);
    else launch_row_project2<64, false>(x, N, f, ldx, w0, w1, out0, out1, stream);
  }
  return check_launch("tgp_row_project2_f32");
}

extern "C" int tgp_sag_aggregate_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* src,
                                     const float* p, const float* q, const float* bias, int64_t N, int64_t E, int mean,
                                     int act, float* t_out, float* a_out, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(N >= 0 && E >= 0, TGP_ERR_INVALID, "tgp_sag_aggregate_f32: bad size");
  TGP_REQUIRE(N < (1ll << 31) && E <= INT32_MAX, TGP_ERR_RANGE,
              "tgp_sag_aggregate_f32: N=%lld or E=%lld beyond the int32 index", static_cast<long long>(N),
              static_cast<long long>(E));
  TGP_REQUIRE((mean == 0 || mean == 1) && (act == 0 || act == 1), TGP_ERR_INVALID,
              "tgp_sag_aggregate_f32: mean must be 0 or 1, act 0 (identity) or 1 (tanh)");
  if (N == 0) return TGP_OK;
  TGP_REQUIRE(grp_ptr && p && (t_out || a_out) && (E == 0 || src), TGP_ERR_INVALID,
              "tgp_sag_aggregate_f32: null pointer");
  TGP_REQUIRE(p != t_out && p != a_out, TGP_ERR_INVALID, "tgp_sag_aggregate_f32: p is read by other nodes, it cannot be an output");
  hipLaunchKernelGGL(sag_aggregate_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, grp_ptr, grp_perm, src, p, q, bias,
                     N, E, mean, act, t_out, a_out);
  return check_launch("tgp_sag_aggregate_f32");
}

extern "C" int tgp_sag_score_bwd_x_f32(const float* g_q, const float* g_p, const float* w_root, const float* w_rel,
                                       int64_t N, int64_t F, int accumulate, float* g_x, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(N >= 0 && F >= 0, TGP_ERR_INVALID, "tgp_sag_score_bwd_x_f32: bad size");
  TGP_REQUIRE(F < (1ll << 31), TGP_ERR_RANGE, "tgp_sag_score_bwd_x_f32: F too large");
  if (N == 0 || F == 0) return TGP_OK;
  TGP_REQUIRE(g_q && g_p && w_root && w_rel && g_x, TGP_ERR_INVALID, "tgp_sag_score_bwd_x_f32: null pointer");
  const bool vec = (F % 4 == 0) && (reinterpret_cast<uintptr_t>(g_x) % 16 == 0) &&
                   (reinterpret_cast<uintptr_t>(w_root) % 16 == 0) && (reinterpret_cast<uintptr_t>(w_rel) % 16 == 0);
  const int64_t total = N * (vec ? F / 4 : F);
  int64_t blocks = cdiv(total, 256);
  if (blocks > 256 * 32) blocks = 256 * 32;
  if (vec)
    hipLaunchKernelGGL(sag_score_bwd_x_kernel<true>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, g_q, g_p,
                       w_root, w_rel, N, static_cast<int>(F), accumulate, g_x);
  else
    hipLaunchKernelGGL(sag_score_bwd_x_kernel<false>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, g_q, g_p,
                       w_root, w_rel, N, static_cast<int>(F), accumulate, g_x);
  return check_launch("tgp_sag_score_bwd_x_f32");
}
