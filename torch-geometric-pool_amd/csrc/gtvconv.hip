// GTVConv's propagation (reference tgp/mp/gtvconv.py, Hansen & Bianchi, "Total Variation Graph Neural Networks"): with
// h = x W already projected,
//     out_i = act((h_i + delta sum_{e: row(e) = i, col(e) != i} gamma_e (h_col(e) - h_i) + bias) [* mask_i]),
//     d_e = ||h_row(e) - h_col(e)||_1,   gamma_e = w_e / max(d_e, eps).
// The reference composes this from x[row], x[col], their difference, its absolute value, a Laplacian, a concatenation and
// a scatter: five E x C temporaries.  Here a node's group of lanes keeps h_i in registers, loads every h_col once, folds
// |h_i - h_col| inside the group, forms gamma_e and accumulates gamma_e (h_col - h_i) from the same registers.  Nothing of
// size E x C exists.
//
// Layout.  A group of G lanes (8, 16, 32 or 64, the smallest with 4 G >= C) owns a node, so a wave holds 64 / G nodes and
// a width of 1..32 keeps 8 nodes busy where a full wave would idle 56 lanes.  A lane holds R channels (4; 8 for G = 64,
// which covers C <= 512): with VEC (C % 4 == 0 and 16-byte aligned bases) as float4 at channel 4 (l + G t), otherwise one
// by one at channel l + G r.  Channels from C on are held as 0 and never stored.  C > 512 takes the chunked kernels
// further down: one wave per node, 512 channels at a time, h_col read a second time.
//
// Order.  Every sum over a node's edges runs in the order of the by-source (out-edges) or by-destination (in-edges) edge
// index, edge-list order inside a node; the fold inside a group is wave_fold<G> (wave.h).  No float atomics: the same
// bits on every call.  An edge is skipped -- and its far end never dereferenced -- when it is a self-loop, when an
// endpoint lies outside [0, nodes) or when its position lies outside [0, E).
#include "common.h"

namespace tgp {

constexpr int GTV_REG_CHANNELS = 512;  // what one register pass holds at G = 64, R = 8

__device__ __forceinline__ float gtv_sign(float v) { return static_cast<float>((v > 0.f) - (v < 0.f)); }

// channel of register r of lane l
template <int G, bool VEC>
__device__ __forceinline__ int gtv_channel(int l, int r) {
  if constexpr (VEC) return 4 * (l + G * (r >> 2)) + (r & 3);
  return l + G * r;
}

template <int G, int R, bool VEC>
__device__ __forceinline__ void gtv_load(const float* __restrict__ p, int C, int l, float (&v)[R]) {
  if constexpr (VEC) {
#pragma unroll
    for (int t = 0; t < R / 4; ++t) {
      const int c = 4 * (l + G * t);
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < C) x = *reinterpret_cast<const float4*>(p + c);
      v[4 * t] = x.x, v[4 * t + 1] = x.y, v[4 * t + 2] = x.z, v[4 * t + 3] = x.w;
    }
  } else {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int c = l + G * r;
      v[r] = c < C ? p[c] : 0.f;
    }
  }
}

template <int G, int R, bool VEC>
__device__ __forceinline__ void gtv_store(float* __restrict__ p, int C, int l, const float (&v)[R]) {
  if constexpr (VEC) {
#pragma unroll
    for (int t = 0; t < R / 4; ++t) {
      const int c = 4 * (l + G * t);
      if (c < C) *reinterpret_cast<float4*>(p + c) = make_float4(v[4 * t], v[4 * t + 1], v[4 * t + 2], v[4 * t + 3]);
    }
  } else {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int c = l + G * r;
      if (c < C) p[c] = v[r];
    }
  }
}

// act: 0 identity, 1 relu, 2 elu (alpha = 1)
__device__ __forceinline__ float gtv_act(float v, int act) {
  if (act == 1) return v > 0.f ? v : 0.f;
  if (act == 2) return v > 0.f ? v : expm1f(v);
  return v;
}
// the activation's derivative from its OUTPUT o (elu: o = e^v - 1 for v <= 0, so the slope is o + 1)
__device__ __forceinline__ float gtv_act_slope(float o, int act) {
  if (act == 1) return o > 0.f ? 1.f : 0.f;
  if (act == 2) return o > 0.f ? 1.f : o + 1.f;
  return 1.f;
}

// the far end of edge position p of node i's group, or -1 for an edge that is skipped; *e_out = the edge
__device__ __forceinline__ int64_t gtv_far_end(const int* __restrict__ perm, const int64_t* __restrict__ other, int p,
                                               int64_t i, int64_t nodes, int64_t E, int* e_out) {
  const int e = perm ? perm[p] : p;
  *e_out = e;
  if (e < 0 || e >= E) return -1;
  const int64_t j = other[e];
  return (j == i || j < 0 || j >= nodes) ? -1 : j;
}

// ------------------------------------------------------------------------------------------------------------ forward
template <int G, int R, bool VEC>
__global__ __launch_bounds__(256) void gtv_edge_fwd_kernel(
    const float* __restrict__ h, int64_t nodes, int C, const int* __restrict__ src_ptr,
    const int* __restrict__ src_perm, const int64_t* __restrict__ col, int64_t E, const float* __restrict__ w,
    const float* __restrict__ bias, const uint8_t* __restrict__ mask, float delta, float eps, int act,
    float* __restrict__ out, float* __restrict__ d) {
  const int l = threadIdx.x & (G - 1);
  const int64_t i = static_cast<int64_t>(blockIdx.x) * (256 / G) + threadIdx.x / G;
  if (i >= nodes) return;  // (whole groups leave: the folds below stay inside a group)
  float hi[R], acc[R];
  gtv_load<G, R, VEC>(h + i * C, C, l, hi);
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.f;
  const int p1 = src_ptr[i + 1];
  for (int p = src_ptr[i]; p < p1; ++p) {
    int e;
    const int64_t j = gtv_far_end(src_perm, col, p, i, nodes, E, &e);
    if (j < 0) continue;
    float hj[R];
    gtv_load<G, R, VEC>(h + j * C, C, l, hj);
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) s += fabsf(hi[r] - hj[r]);
    s = wave_fold<G>(s, op_add{});
    if (d && l == 0) d[e] = s;
    const float gam = (w ? w[e] : 1.f) / clamp_min(s, eps);
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] += gam * (hj[r] - hi[r]);
  }
  const bool keep = mask ? mask[i] != 0 : true;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int c = gtv_channel<G, VEC>(l, r);
    float v = hi[r] + delta * acc[r];
    if (bias && c < C) v += bias[c];
    if (!keep) v *= 0.f;
    acc[r] = gtv_act(v, act);
  }
  gtv_store<G, R, VEC>(out + i * C, C, l, acc);
}

// ------------------------------------------------------------------------------------------- backward, the edge terms
// Gbuf[i,:] = g_out[i,:] act'(out[i,:]) mask_i; per out-edge s_e = delta <g_i, h_j - h_i>, gw_e = s_e / max(d_e, eps),
// t_e = -s_e gamma_e / d_e where d_e >= eps (the gradient mask of torch's clamp(min=)), else 0.
template <int G, int R, bool VEC>
__global__ __launch_bounds__(256) void gtv_edge_bwd_terms_kernel(
    const float* __restrict__ h, const float* __restrict__ out, const float* __restrict__ gout, int64_t nodes, int C,
    const int* __restrict__ src_ptr, const int* __restrict__ src_perm, const int64_t* __restrict__ col, int64_t E,
    const float* __restrict__ w, const float* __restrict__ d, const uint8_t* __restrict__ mask, float delta, float eps,
    int act, float* __restrict__ Gbuf, float* __restrict__ gw, float* __restrict__ t) {
  const int l = threadIdx.x & (G - 1);
  const int64_t i = static_cast<int64_t>(blockIdx.x) * (256 / G) + threadIdx.x / G;
  if (i >= nodes) return;
  float hi[R], g[R];
  {
    float o[R];
    gtv_load<G, R, VEC>(out + i * C, C, l, o);
    gtv_load<G, R, VEC>(gout + i * C, C, l, g);
    const float m = (mask && mask[i] == 0) ? 0.f : 1.f;
#pragma unroll
    for (int r = 0; r < R; ++r) g[r] = g[r] * gtv_act_slope(o[r], act) * m;
  }
  gtv_store<G, R, VEC>(Gbuf + i * C, C, l, g);
  gtv_load<G, R, VEC>(h + i * C, C, l, hi);
  const int p1 = src_ptr[i + 1];
  for (int p = src_ptr[i]; p < p1; ++p) {
    int e;
    const int64_t j = gtv_far_end(src_perm, col, p, i, nodes, E, &e);
    if (j < 0) continue;
    float hj[R];
    gtv_load<G, R, VEC>(h + j * C, C, l, hj);
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) s += g[r] * (hj[r] - hi[r]);
    s = delta * wave_fold<G>(s, op_add{});
    if (l == 0) {
      const float de = d[e], den = clamp_min(de, eps);
      if (gw) gw[e] = s / den;
      t[e] = de >= eps ? -(s * ((w ? w[e] : 1.f) / den)) / de : 0.f;
    }
  }
}

// ------------------------------------------------------------------------------------------ backward, the node gradient
// dh_i = g_i (1 - delta sum_out gamma_e) + sum_out t_e sign(h_i - h_col)
//      + sum_in (delta gamma_e g_row - t_e sign(h_row - h_i)),   sign(0) = 0: out-edges, then in-edges, no scatter.
template <int G, int R, bool VEC>
__global__ __launch_bounds__(256) void gtv_edge_bwd_nodes_kernel(
    const float* __restrict__ h, const float* __restrict__ Gbuf, int64_t nodes, int C, const int* __restrict__ src_ptr,
    const int* __restrict__ src_perm, const int* __restrict__ dst_ptr, const int* __restrict__ dst_perm,
    const int64_t* __restrict__ row, const int64_t* __restrict__ col, int64_t E, const float* __restrict__ w,
    const float* __restrict__ d, const float* __restrict__ t, float delta, float eps, float* __restrict__ dh) {
  const int l = threadIdx.x & (G - 1);
  const int64_t i = static_cast<int64_t>(blockIdx.x) * (256 / G) + threadIdx.x / G;
  if (i >= nodes) return;
  float hi[R], acc[R];
  gtv_load<G, R, VEC>(h + i * C, C, l, hi);
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.f;
  float sg = 0.f;
  const int p1 = src_ptr[i + 1];
  for (int p = src_ptr[i]; p < p1; ++p) {
    int e;
    const int64_t j = gtv_far_end(src_perm, col, p, i, nodes, E, &e);
    if (j < 0) continue;
    sg += (w ? w[e] : 1.f) / clamp_min(d[e], eps);
    const float te = t[e];
    if (te == 0.f) continue;  // (a clamped edge: d_e carries no gradient, h_col is not needed)
    float hj[R];
    gtv_load<G, R, VEC>(h + j * C, C, l, hj);
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] += te * gtv_sign(hi[r] - hj[r]);
  }
  const int q1 = dst_ptr[i + 1];
  for (int p = dst_ptr[i]; p < q1; ++p) {
    int e;
    const int64_t j = gtv_far_end(dst_perm, row, p, i, nodes, E, &e);
    if (j < 0) continue;
    const float dg = delta * ((w ? w[e] : 1.f) / clamp_min(d[e], eps));
    const float te = t[e];
    float v[R];
    gtv_load<G, R, VEC>(Gbuf + j * C, C, l, v);
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] += dg * v[r];
    if (te == 0.f) continue;
    gtv_load<G, R, VEC>(h + j * C, C, l, v);
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] -= te * gtv_sign(v[r] - hi[r]);
  }
  {
    float gi[R];
    gtv_load<G, R, VEC>(Gbuf + i * C, C, l, gi);
    const float self = 1.f - delta * sg;
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = gi[r] * self + acc[r];
  }
  gtv_store<G, R, VEC>(dh + i * C, C, l, acc);
}

// ------------------------------------------------------------------------------------- C > 512: the chunked kernels
// One wave per node, lane l holds channels c0 + l + 64 r of the current 512-channel chunk.  The distances need every
// channel before the first gamma exists, so they are a kernel of their own (d is required); the second kernel re-reads
// h_col chunk by chunk.
__device__ __forceinline__ void gtv_chunk_load(const float* __restrict__ p, int C, int c0, int lane, float (&v)[8]) {
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int c = c0 + lane + 64 * r;
    v[r] = c < C ? p[c] : 0.f;
  }
}

__global__ __launch_bounds__(256) void gtv_wide_dist_kernel(const float* __restrict__ h, int64_t nodes, int C,
                                                            const int* __restrict__ src_ptr,
                                                            const int* __restrict__ src_perm,
                                                            const int64_t* __restrict__ col, int64_t E,
                                                            float* __restrict__ d) {
  const int lane = threadIdx.x & 63;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (i >= nodes) return;
  const float* hi = h + i * C;
  const int p1 = src_ptr[i + 1];
  for (int p = src_ptr[i]; p < p1; ++p) {
    int e;
    const int64_t j = gtv_far_end(src_perm, col, p, i, nodes, E, &e);
    if (j < 0) continue;
    const float* hj = h + j * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += fabsf(hi[c] - hj[c]);
    s = wave_fold<64>(s, op_add{});
    if (lane == 0) d[e] = s;
  }
}

__global__ __launch_bounds__(256) void gtv_wide_fwd_kernel(
    const float* __restrict__ h, int64_t nodes, int C, const int* __restrict__ src_ptr,
    const int* __restrict__ src_perm, const int64_t* __restrict__ col, int64_t E, const float* __restrict__ w,
    const float* __restrict__ bias, const uint8_t* __restrict__ mask, float delta, float eps, int act,
    float* __restrict__ out, const float* __restrict__ d) {
  const int lane = threadIdx.x & 63;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (i >= nodes) return;
  const bool keep = mask ? mask[i] != 0 : true;
  const int p0 = src_ptr[i], p1 = src_ptr[i + 1];
  for (int c0 = 0; c0 < C; c0 += GTV_REG_CHANNELS) {
    float hi[8], acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    gtv_chunk_load(h + i * C, C, c0, lane, hi);
    for (int p = p0; p < p1; ++p) {
      int e;
      const int64_t j = gtv_far_end(src_perm, col, p, i, nodes, E, &e);
      if (j < 0) continue;
      const float gam = (w ? w[e] : 1.f) / clamp_min(d[e], eps);
      float hj[8];
      gtv_chunk_load(h + j * C, C, c0, lane, hj);
#pragma unroll
      for (int r = 0; r < 8; ++r) acc[r] += gam * (hj[r] - hi[r]);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int c = c0 + lane + 64 * r;
      if (c >= C) continue;
      float v = hi[r] + delta * acc[r];
      if (bias) v += bias[c];
      if (!keep) v *= 0.f;
      out[i * C + c] = gtv_act(v, act);
    }
  }
}

__global__ __launch_bounds__(256) void gtv_wide_bwd_terms_kernel(
    const float* __restrict__ h, const float* __restrict__ out, const float* __restrict__ gout, int64_t nodes, int C,
    const int* __restrict__ src_ptr, const int* __restrict__ src_perm, const int64_t* __restrict__ col, int64_t E,
    const float* __restrict__ w, const float* __restrict__ d, const uint8_t* __restrict__ mask, float delta, float eps,
    int act, float* __restrict__ Gbuf, float* __restrict__ gw, float* __restrict__ t) {
  const int lane = threadIdx.x & 63;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (i >= nodes) return;
  const float m = (mask && mask[i] == 0) ? 0.f : 1.f;
  const float* hi = h + i * C;
  float* gi = Gbuf + i * C;
  // every lane writes the channels lane, lane + 64, .. of Gbuf's row and reads back exactly those below
  for (int c = lane; c < C; c += 64) gi[c] = gout[i * C + c] * gtv_act_slope(out[i * C + c], act) * m;
  const int p1 = src_ptr[i + 1];
  for (int p = src_ptr[i]; p < p1; ++p) {
    int e;
    const int64_t j = gtv_far_end(src_perm, col, p, i, nodes, E, &e);
    if (j < 0) continue;
    const float* hj = h + j * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += gi[c] * (hj[c] - hi[c]);
    s = delta * wave_fold<64>(s, op_add{});
    if (lane == 0) {
      const float de = d[e], den = clamp_min(de, eps);
      if (gw) gw[e] = s / den;
      t[e] = de >= eps ? -(s * ((w ? w[e] : 1.f) / den)) / de : 0.f;
    }
  }
}

__global__ __launch_bounds__(256) void gtv_wide_bwd_nodes_kernel(
    const float* __restrict__ h, const float* __restrict__ Gbuf, int64_t nodes, int C, const int* __restrict__ src_ptr,
    const int* __restrict__ src_perm, const int* __restrict__ dst_ptr, const int* __restrict__ dst_perm,
    const int64_t* __restrict__ row, const int64_t* __restrict__ col, int64_t E, const float* __restrict__ w,
    const float* __restrict__ d, const float* __restrict__ t, float delta, float eps, float* __restrict__ dh) {
  const int lane = threadIdx.x & 63;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (i >= nodes) return;
  const int p0 = src_ptr[i], p1 = src_ptr[i + 1], q0 = dst_ptr[i], q1 = dst_ptr[i + 1];
  for (int c0 = 0; c0 < C; c0 += GTV_REG_CHANNELS) {
    float hi[8], acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, v[8];
    gtv_chunk_load(h + i * C, C, c0, lane, hi);
    float sg = 0.f;
    for (int p = p0; p < p1; ++p) {
      int e;
      const int64_t j = gtv_far_end(src_perm, col, p, i, nodes, E, &e);
      if (j < 0) continue;
      sg += (w ? w[e] : 1.f) / clamp_min(d[e], eps);
      const float te = t[e];
      if (te == 0.f) continue;
      gtv_chunk_load(h + j * C, C, c0, lane, v);
#pragma unroll
      for (int r = 0; r < 8; ++r) acc[r] += te * gtv_sign(hi[r] - v[r]);
    }
    for (int p = q0; p < q1; ++p) {
      int e;
      const int64_t j = gtv_far_end(dst_perm, row, p, i, nodes, E, &e);
      if (j < 0) continue;
      const float dg = delta * ((w ? w[e] : 1.f) / clamp_min(d[e], eps));
      const float te = t[e];
      gtv_chunk_load(Gbuf + j * C, C, c0, lane, v);
#pragma unroll
      for (int r = 0; r < 8; ++r) acc[r] += dg * v[r];
      if (te == 0.f) continue;
      gtv_chunk_load(h + j * C, C, c0, lane, v);
#pragma unroll
      for (int r = 0; r < 8; ++r) acc[r] -= te * gtv_sign(v[r] - hi[r]);
    }
    gtv_chunk_load(Gbuf + i * C, C, c0, lane, v);
    const float self = 1.f - delta * sg;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int c = c0 + lane + 64 * r;
      if (c < C) dh[i * C + c] = v[r] * self + acc[r];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------- dispatch
inline bool gtv_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// calls f(kernel group width G, registers R, vectorised) for the layout of width C (C <= GTV_REG_CHANNELS)
template <typename F>
inline void gtv_pick(int C, bool vec, F f) {
#define TGP_GTV_CASE(G_, R_)                                       \
  {                                                                \
    if (vec)                                                       \
      f(std::integral_constant<int, G_>{}, std::integral_constant<int, R_>{}, std::true_type{});  \
    else                                                           \
      f(std::integral_constant<int, G_>{}, std::integral_constant<int, R_>{}, std::false_type{}); \
    return;                                                        \
  }
  if (C <= 32) TGP_GTV_CASE(8, 4)
  if (C <= 64) TGP_GTV_CASE(16, 4)
  if (C <= 128) TGP_GTV_CASE(32, 4)
  if (C <= 256) TGP_GTV_CASE(64, 4)
  TGP_GTV_CASE(64, 8)
#undef TGP_GTV_CASE
}

}  // namespace tgp

using namespace tgp;

extern "C" int tgp_gtv_edge_fwd_f32(const float* h, int64_t nodes, int64_t C, const int32_t* src_ptr,
                                    const int32_t* src_perm, const int64_t* col, const float* w, int64_t E,
                                    const float* bias, const uint8_t* mask, float delta, float eps, int act_code,
                                    float* out, float* d, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(nodes >= 0 && C >= 1 && E >= 0, TGP_ERR_INVALID, "tgp_gtv_edge_fwd_f32: bad shape");
  TGP_REQUIRE(act_code >= 0 && act_code <= 2, TGP_ERR_INVALID, "tgp_gtv_edge_fwd_f32: act_code must be 0, 1 or 2");
  if (nodes == 0) return TGP_OK;
  TGP_REQUIRE(h && src_ptr && out && (E == 0 || col), TGP_ERR_INVALID, "tgp_gtv_edge_fwd_f32: null pointer");
  TGP_REQUIRE(nodes < (1ll << 31) && E < (1ll << 31) && C < 32768, TGP_ERR_RANGE, "tgp_gtv_edge_fwd_f32: too large");
  TGP_REQUIRE(C <= GTV_REG_CHANNELS || d || E == 0, TGP_ERR_INVALID,
              "tgp_gtv_edge_fwd_f32: more than 512 channels need the distance buffer d");
  const int Ci = static_cast<int>(C);
  if (C > GTV_REG_CHANNELS) {
    const dim3 grid(static_cast<unsigned>(cdiv(nodes, 4)));
    if (E > 0)
      hipLaunchKernelGGL(gtv_wide_dist_kernel, grid, dim3(256), 0, stream, h, nodes, Ci, src_ptr, src_perm, col, E, d);
    hipLaunchKernelGGL(gtv_wide_fwd_kernel, grid, dim3(256), 0, stream, h, nodes, Ci, src_ptr, src_perm, col, E, w, bias,
                       mask, delta, eps, act_code, out, d);
    return check_launch("tgp_gtv_edge_fwd_f32");
  }
  const bool vec = C % 4 == 0 && gtv_aligned16(h) && gtv_aligned16(out);
  gtv_pick(Ci, vec, [&](auto g, auto r, auto v) {
    constexpr int G = decltype(g)::value, R = decltype(r)::value;
    constexpr bool V = decltype(v)::value;
    hipLaunchKernelGGL((gtv_edge_fwd_kernel<G, R, V>), dim3(static_cast<unsigned>(cdiv(nodes, 256 / G))), dim3(256), 0,
                       stream, h, nodes, Ci, src_ptr, src_perm, col, E, w, bias, mask, delta, eps, act_code, out, d);
  });
  return check_launch("tgp_gtv_edge_fwd_f32");
}

extern "C" int tgp_gtv_edge_bwd_terms_f32(const float* h, const float* out, const float* g_out, int64_t nodes, int64_t C,
                                          const int32_t* src_ptr, const int32_t* src_perm, const int64_t* col,
                                          const float* w, int64_t E, const float* d, const uint8_t* mask, float delta,
                                          float eps, int act_code, float* g, float* gw, float* t, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(nodes >= 0 && C >= 1 && E >= 0, TGP_ERR_INVALID, "tgp_gtv_edge_bwd_terms_f32: bad shape");
  TGP_REQUIRE(act_code >= 0 && act_code <= 2, TGP_ERR_INVALID,
              "tgp_gtv_edge_bwd_terms_f32: act_code must be 0, 1 or 2");
  if (nodes == 0) return TGP_OK;
  TGP_REQUIRE(h && out && g_out && src_ptr && g && (E == 0 || (col && d && t)), TGP_ERR_INVALID,
              "tgp_gtv_edge_bwd_terms_f32: null pointer");
  TGP_REQUIRE(nodes < (1ll << 31) && E < (1ll << 31) && C < 32768, TGP_ERR_RANGE,
              "tgp_gtv_edge_bwd_terms_f32: too large");
  const int Ci = static_cast<int>(C);
  if (C > GTV_REG_CHANNELS) {
    hipLaunchKernelGGL(gtv_wide_bwd_terms_kernel, dim3(static_cast<unsigned>(cdiv(nodes, 4))), dim3(256), 0, stream, h,
                       out, g_out, nodes, Ci, src_ptr, src_perm, col, E, w, d, mask, delta, eps, act_code, g, gw, t);
    return check_launch("tgp_gtv_edge_bwd_terms_f32");
  }
  const bool vec = C % 4 == 0 && gtv_aligned16(h) && gtv_aligned16(out) && gtv_aligned16(g_out) && gtv_aligned16(g);
  gtv_pick(Ci, vec, [&](auto gg, auto r, auto v) {
    constexpr int G = decltype(gg)::value, R = decltype(r)::value;
    constexpr bool V = decltype(v)::value;
    hipLaunchKernelGGL((gtv_edge_bwd_terms_kernel<G, R, V>), dim3(static_cast<unsigned>(cdiv(nodes, 256 / G))),
                       dim3(256), 0, stream, h, out, g_out, nodes, Ci, src_ptr, src_perm, col, E, w, d, mask, delta, eps,
                       act_code, g, gw, t);
  });
  return check_launch("tgp_gtv_edge_bwd_terms_f32");
}

extern "C" int tgp_gtv_edge_bwd_nodes_f32(const float* h, const float* g, int64_t nodes, int64_t C,
                                          const int32_t* src_ptr, const int32_t* src_perm, const int32_t* dst_ptr,
                                          const int32_t* dst_perm, const int64_t* row, const int64_t* col,
                                          const float* w, int64_t E, const float* d, const float* t, float delta,
                                          float eps, float* dh, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(nodes >= 0 && C >= 1 && E >= 0, TGP_ERR_INVALID, "tgp_gtv_edge_bwd_nodes_f32: bad shape");
  if (nodes == 0) return TGP_OK;
  TGP_REQUIRE(h && g && src_ptr && dst_ptr && dh && (E == 0 || (row && col && d && t)), TGP_ERR_INVALID,
              "tgp_gtv_edge_bwd_nodes_f32: null pointer");
  TGP_REQUIRE(nodes < (1ll << 31) && E < (1ll << 31) && C < 32768, TGP_ERR_RANGE,
              "tgp_gtv_edge_bwd_nodes_f32: too large");
  const int Ci = static_cast<int>(C);
  if (C > GTV_REG_CHANNELS) {
    hipLaunchKernelGGL(gtv_wide_bwd_nodes_kernel, dim3(static_cast<unsigned>(cdiv(nodes, 4))), dim3(256), 0, stream, h, g,
                       nodes, Ci, src_ptr, src_perm, dst_ptr, dst_perm, row, col, E, w, d, t, delta, eps, dh);
    return check_launch("tgp_gtv_edge_bwd_nodes_f32");
  }
  const bool vec = C % 4 == 0 && gtv_aligned16(h) && gtv_aligned16(g) && gtv_aligned16(dh);
  gtv_pick(Ci, vec, [&](auto gg, auto r, auto v) {
    constexpr int G = decltype(gg)::value, R = decltype(r)::value;
    constexpr bool V = decltype(v)::value;
    hipLaunchKernelGGL((gtv_edge_bwd_nodes_kernel<G, R, V>), dim3(static_cast<unsigned>(cdiv(nodes, 256 / G))),
                       dim3(256), 0, stream, h, g, nodes, Ci, src_ptr, src_perm, dst_ptr, dst_perm, row, col, E, w, d, t,
                       delta, eps, dh);
  });
  return check_launch("tgp_gtv_edge_bwd_nodes_f32");
}
