// ASAPooling's fitness (reference poolers/asap.py:205-237) without anything of size E x F and without the F x F Linear:
//   x_q[i,:] = max over i's in-edges of x_pool[src,:],  sq[i] = <x_q[i,:], w~> + c      (asap_query_kernel)
//   alpha_e  = softmax over i's in-edges of leaky(sq[i] + sp[src_e])                     (asap_edge_softmax_kernel)
//   x_new[i,:] = sum_e alpha_e x[src_e,:],  p_k[i] = <x_new[i,:], w_k>, k = 1, 2, 3      (asap_attend_kernel)
//   fit[i] = p3[i] + b3 + sum_e w_e p1[src_e] + (b1 - p2[i]) sum_e w_e,  a = act(fit)    (asap_leconv_kernel)
// w~ = W_lin^T a1, c = <a1, b_lin> + b_att and sp = <x_pool, a2> come from the caller (att = [a1 | a2] is linear).
// The backward's pieces of E x F scale are here too: g_alpha_e = <g_x_new[dst_e,:], x[src_e,:]> (asap_edge_dot_kernel), the
// softmax and leaky backward per destination (asap_softmax_bwd_kernel) and the master query's backward by source over the
// stored arg-max edge positions (asap_query_bwd_kernel); g_x is the attend kernel over the by-source group.
// One wave owns one group in the row kernels: G lanes share a row (a float4 each when VEC), the 64 / G "slots" of a wave
// take every (64 / G)-th edge of the group.  No float atomics; every sum has one order, fixed by the group: a slot adds
// its edges in group order, the slots are folded by the xor butterfly at offsets 32 .. G, a dot product folds its G lanes
// at offsets G / 2 .. 1.  A group with very many edges is walked by its one wave: there is no hub route.
// A position outside [0, E) or an endpoint outside [0, n) is skipped and never dereferenced.
#include <math.h>

#include "common.h"

namespace tgp {
namespace {

struct Group {
  int64_t b, e;
};

__device__ __forceinline__ Group group_of(const int32_t* __restrict__ grp_ptr, int64_t i, int64_t E) {
  int64_t b = grp_ptr[i], e = grp_ptr[i + 1];
  if (b < 0) b = 0;
  if (e > E) e = E;
  return {b, e};
}

// the source row of group entry j, or -1 when the position or the source is out of range
__device__ __forceinline__ int64_t source_of(const int32_t* __restrict__ grp_perm, const int64_t* __restrict__ src,
                                              int64_t j, int64_t E, int64_t n, int64_t* pos_out) {
  const int64_t pos = grp_perm ? static_cast<int64_t>(grp_perm[j]) : j;
  *pos_out = pos;
  if (static_cast<uint64_t>(pos) >= static_cast<uint64_t>(E)) return -1;
  const int64_t r = src[pos];
  return static_cast<uint64_t>(r) < static_cast<uint64_t>(n) ? r : -1;
}

// W columns of a row starting at column k (columns at or beyond F read as `fill`)
template <bool VEC>
__device__ __forceinline__ void load_unit(const float* __restrict__ row, int k, int F, float fill, float (&v)[VEC ? 4 : 1]) {
  if constexpr (VEC) {
    if (k + 4 <= F) {
      const float4 t = *reinterpret_cast<const float4*>(row + k);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (k + j < F) ? row[k + j] : fill;
    }
  } else {
    v[0] = (k < F) ? row[k] : fill;
  }
}

// does candidate (v, pos) replace the running (m, arg)?  A larger value does, an equal one at a lower position does, a
// NaN replaces any number (and among NaNs the lower position stays)
__device__ __forceinline__ bool better(float v, int32_t pos, float m, int32_t arg) {
  const bool vn = v != v, mn = m != m;
  if (vn || mn) return vn && (!mn || pos < arg);
  return v > m || (v == m && pos < arg);
}

template <int G, bool VEC>
__global__ __launch_bounds__(256) void asap_query_kernel(const int32_t* __restrict__ grp_ptr,
                                                         const int32_t* __restrict__ grp_perm,
                                                         const int64_t* __restrict__ src, const float* __restrict__ x,
                                                         int64_t ldx, const float* __restrict__ wt,
                                                         const float* __restrict__ c, int64_t n, int64_t E, int F,
                                                         float* __restrict__ sq, int32_t* __restrict__ argpos) {
  constexpr int W = VEC ? 4 : 1;
  constexpr int PER = 64 / G;
  const int lane = threadIdx.x & 63, sub = lane % G, slot = lane / G;
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (i >= n) return;  // wave-uniform
  const Group g = group_of(grp_ptr, i, E);
  float acc = 0.0f;
  for (int kb = 0; kb < F; kb += G * W) {  // one pass over the group per block of G * W columns (one block: F <= 256 / 64)
    const int k = kb + sub * W;
    float m[W];
    int32_t arg[W];  // the edge position that gave m: the lowest one among equals (kept only when argpos is asked for)
    bool any = false;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      m[j] = -INFINITY;
      arg[j] = INT32_MAX;
    }
    for (int64_t e = g.b + slot; e < g.e; e += PER) {
      int64_t pos;
      const int64_t r = source_of(grp_perm, src, e, E, n, &pos);
      if (r < 0) continue;
      any = true;
      if (k < F) {
        float v[W];
        load_unit<VEC>(x + r * ldx, k, F, -INFINITY, v);
#pragma unroll
        for (int j = 0; j < W; ++j) {
          if (argpos && better(v[j], static_cast<int32_t>(pos), m[j], arg[j])) arg[j] = static_cast<int32_t>(pos);
          m[j] = nan_max(m[j], v[j]);
        }
      }
    }
    // the slots of the wave: a maximum has no order to keep (a NaN in any slot wins); equal maxima keep the lower position
    if (argpos) {
#pragma unroll
      for (int o = 32; o >= G; o >>= 1) {
#pragma unroll
        for (int j = 0; j < W; ++j) {
          const float om = __shfl_xor(m[j], o, 64);
          const int32_t oa = __shfl_xor(arg[j], o, 64);
          if (better(om, oa, m[j], arg[j])) arg[j] = oa;
          m[j] = nan_max(m[j], om);
        }
      }
      if (slot == 0 && k < F) {
#pragma unroll
        for (int j = 0; j < W; ++j)
          if (k + j < F) argpos[i * F + k + j] = arg[j] == INT32_MAX ? -1 : arg[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < W; ++j) m[j] = wave_fold<64, G>(m[j], op_nanmax{});
    }
    const bool have = __any(any);
    float part = 0.0f;
    if (have && k < F) {
#pragma unroll
      for (int j = 0; j < W; ++j)
        if (k + j < F) part = fmaf(m[j], wt[k + j], part);
    }
    acc = acc + wave_sum<G>(part);  // the G lanes of a row, offsets G / 2 .. 1; column blocks in ascending order
  }
  if (lane == 0) sq[i] = acc + c[0];
}

// One wave per destination, lanes over its edges: l_e = leaky(sq[i] + sp[src_e]); m = max, s = sum exp(l_e - m) (each
// lane adds its every-64th edge in group order, then the butterfly 32 .. 1), alpha[pos] = exp(l_e - m) / (s + 1e-16).
__global__ __launch_bounds__(256) void asap_edge_softmax_kernel(const int32_t* __restrict__ grp_ptr,
                                                                const int32_t* __restrict__ grp_perm,
                                                                const int64_t* __restrict__ src,
                                                                const float* __restrict__ sq,
                                                                const float* __restrict__ sp, int64_t n, int64_t E,
                                                                float slope, float* __restrict__ alpha) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (i >= n) return;
  const Group g = group_of(grp_ptr, i, E);
  const float q = sq[i];
  float m = -INFINITY;
  for (int64_t e = g.b + lane; e < g.e; e += 64) {
    int64_t pos;
    const int64_t r = source_of(grp_perm, src, e, E, n, &pos);
    if (r < 0) continue;
    const float t = q + sp[r];
    m = nan_max(m, t > 0.0f ? t : t * slope);
  }
  m = wave_nanmax(m);
  float s = 0.0f;
  for (int64_t e = g.b + lane; e < g.e; e += 64) {
    int64_t pos;
    const int64_t r = source_of(grp_perm, src, e, E, n, &pos);
    if (r < 0) continue;
    const float t = q + sp[r];
    s = s + expf((t > 0.0f ? t : t * slope) - m);
  }
  s = wave_sum(s) + 1e-16f;
  for (int64_t e = g.b + lane; e < g.e; e += 64) {
    int64_t pos;
    const int64_t r = source_of(grp_perm, src, e, E, n, &pos);
    if (r < 0) {
      if (static_cast<uint64_t>(pos) < static_cast<uint64_t>(E)) alpha[pos] = 0.0f;  // a source out of range attends to nothing
      continue;
    }
    const float t = q + sp[r];
    alpha[pos] = expf((t > 0.0f ? t : t * slope) - m) / s;
  }
}

template <int G, bool VEC>
__global__ __launch_bounds__(256) void asap_attend_kernel(const int32_t* __restrict__ grp_ptr,
                                                          const int32_t* __restrict__ grp_perm,
                                                          const int64_t* __restrict__ src,
                                                          const float* __restrict__ val, const float* __restrict__ x,
                                                          int64_t ldx, const float* __restrict__ w3, int64_t n,
                                                          int64_t n_src, int64_t E, int F, float* __restrict__ out,
                                                          float* __restrict__ p) {
  constexpr int W = VEC ? 4 : 1;
  constexpr int PER = 64 / G;
  const int lane = threadIdx.x & 63, sub = lane % G, slot = lane / G;
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (i >= n) return;
  const Group g = group_of(grp_ptr, i, E);
  const bool vec_store = VEC && (F % 4 == 0);
  float p1 = 0.0f, p2 = 0.0f, p3 = 0.0f;
  for (int kb = 0; kb < F; kb += G * W) {
    const int k = kb + sub * W;
    float acc[W];
#pragma unroll
    for (int j = 0; j < W; ++j) acc[j] = 0.0f;
    for (int64_t e = g.b + slot; e < g.e; e += PER) {
      int64_t pos;
      const int64_t r = source_of(grp_perm, src, e, E, n_src, &pos);
      if (r < 0 || k >= F) continue;
      const float a = val ? val[pos] : 1.0f;
      float v[W];
      load_unit<VEC>(x + r * ldx, k, F, 0.0f, v);
#pragma unroll
      for (int j = 0; j < W; ++j) acc[j] = fmaf(a, v[j], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < W; ++j) acc[j] = wave_sum<64, G>(acc[j]);  // the slots: offsets 32 .. G
    if (slot == 0 && k < F) {
      float* o = out + i * F + k;
      if (vec_store) {
        if constexpr (VEC) *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
      } else {
#pragma unroll
        for (int j = 0; j < W; ++j)
          if (k + j < F) o[j] = acc[j];
      }
    }
    if (w3) {  // the finished row is still in registers: its three projections
      float a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
      if (k < F) {
#pragma unroll
        for (int j = 0; j < W; ++j) {
          if (k + j < F) {
            a1 = fmaf(acc[j], w3[k + j], a1);
            a2 = fmaf(acc[j], w3[F + k + j], a2);
            a3 = fmaf(acc[j], w3[2 * static_cast<int64_t>(F) + k + j], a3);
          }
        }
      }
      p1 = p1 + wave_sum<G>(a1);
      p2 = p2 + wave_sum<G>(a2);
      p3 = p3 + wave_sum<G>(a3);
    }
  }
  if (w3 && lane == 0) {
    p[i] = p1;
    p[n + i] = p2;
    p[2 * n + i] = p3;
  }
}

// One lane per node, its group in order: s = sum_e w_e p1[src_e], W = sum_e w_e (w_e = 1 without weights; a skipped edge
// adds to neither), t = ((p3 + b3) + s) + (b1 - p2) W.
__global__ __launch_bounds__(256) void asap_leconv_kernel(const int32_t* __restrict__ grp_ptr,
                                                          const int32_t* __restrict__ grp_perm,
                                                          const int64_t* __restrict__ src,
                                                          const float* __restrict__ ew, const float* __restrict__ p,
                                                          const float* __restrict__ b1, const float* __restrict__ b3,
                                                          int64_t n, int64_t E, int act, float* __restrict__ t_out,
                                                          float* __restrict__ a_out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const Group g = group_of(grp_ptr, i, E);
  float s = 0.0f, wsum = 0.0f;
  for (int64_t e = g.b; e < g.e; ++e) {
    int64_t pos;
    const int64_t r = source_of(grp_perm, src, e, E, n, &pos);
    if (r < 0) continue;
    const float w = ew ? ew[pos] : 1.0f;
    s = fmaf(w, p[r], s);
    wsum = wsum + w;
  }
  const float t = ((p[2 * n + i] + (b3 ? b3[0] : 0.0f)) + s) + ((b1 ? b1[0] : 0.0f) - p[n + i]) * wsum;
  if (t_out) t_out[i] = t;
  if (a_out) a_out[i] = act == 1 ? tanhf(t) : act == 2 ? 1.0f / (1.0f + expf(-t)) : t;
}

// ---- the backward's pieces of E x F scale -------------------------------------------------------------------------
// g_alpha[pos] = <g[i,:], x[src,:]> for every edge of group i: the first G * W columns of the g row stay in registers,
// the x rows are gathered; a slot takes an edge, its G lanes fold the dot product at offsets G / 2 .. 1.
template <int G, bool VEC>
__global__ __launch_bounds__(256) void asap_edge_dot_kernel(const int32_t* __restrict__ grp_ptr,
                                                            const int32_t* __restrict__ grp_perm,
                                                            const int64_t* __restrict__ src, const float* __restrict__ g,
                                                            const float* __restrict__ x, int64_t ldx, int64_t n,
                                                            int64_t E, int F, float* __restrict__ out) {
  constexpr int W = VEC ? 4 : 1;
  constexpr int PER = 64 / G;
  const int lane = threadIdx.x & 63, sub = lane % G, slot = lane / G;
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (i >= n) return;
  const Group gr = group_of(grp_ptr, i, E);
  const float* grow = g + i * F;  // contiguous [n, F]: 16-byte loads only when F % 4 == 0 (the host picks VEC so)
  float g0[W];
  load_unit<VEC>(grow, sub * W, F, 0.0f, g0);
  const int64_t rounds = (gr.e - gr.b + PER - 1) / PER;  // every lane takes part in every fold
  for (int64_t t = 0; t < rounds; ++t) {
    const int64_t e = gr.b + t * PER + slot;
    int64_t pos = -1, r = -1;
    if (e < gr.e) r = source_of(grp_perm, src, e, E, n, &pos);
    float acc = 0.0f;
    if (r >= 0) {
      const float* row = x + r * ldx;
      for (int k = sub * W; k < F; k += G * W) {
        float gv[W], xv[W];
        if (k == sub * W) {
#pragma unroll
          for (int j = 0; j < W; ++j) gv[j] = g0[j];
        } else {
          load_unit<VEC>(grow, k, F, 0.0f, gv);
        }
        load_unit<VEC>(row, k, F, 0.0f, xv);
#pragma unroll
        for (int j = 0; j < W; ++j) acc = fmaf(gv[j], xv[j], acc);
      }
    }
    acc = wave_sum<G>(acc);
    if (sub == 0 && e < gr.e && static_cast<uint64_t>(pos) < static_cast<uint64_t>(E)) out[pos] = r >= 0 ? acc : 0.0f;
  }
}

// Softmax and leaky-ReLU backward of one destination: d = sum_e alpha_e g_alpha_e (lane-strided, then the butterfly),
// g_l[pos] = alpha_e (g_alpha_e - d) * (sq[i] + sp[src_e] > 0 ? 1 : slope), g_sq[i] = sum_e g_l (the same order).
__global__ __launch_bounds__(256) void asap_softmax_bwd_kernel(const int32_t* __restrict__ grp_ptr,
                                                               const int32_t* __restrict__ grp_perm,
                                                               const int64_t* __restrict__ src,
                                                               const float* __restrict__ alpha,
                                                               const float* __restrict__ g_alpha,
                                                               const float* __restrict__ sq,
                                                               const float* __restrict__ sp, int64_t n, int64_t E,
                                                               float slope, float* __restrict__ g_l,
                                                               float* __restrict__ g_sq) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (i >= n) return;
  const Group g = group_of(grp_ptr, i, E);
  const float q = sq[i];
  float d = 0.0f;
  for (int64_t e = g.b + lane; e < g.e; e += 64) {
    int64_t pos;
    if (source_of(grp_perm, src, e, E, n, &pos) < 0) continue;
    d = fmaf(alpha[pos], g_alpha[pos], d);
  }
  d = wave_sum(d);
  float s = 0.0f;
  for (int64_t e = g.b + lane; e < g.e; e += 64) {
    int64_t pos;
    const int64_t r = source_of(grp_perm, src, e, E, n, &pos);
    if (r < 0) {
      if (static_cast<uint64_t>(pos) < static_cast<uint64_t>(E)) g_l[pos] = 0.0f;
      continue;
    }
    float v = alpha[pos] * (g_alpha[pos] - d);
    if (!(q + sp[r] > 0.0f)) v = v * slope;
    g_l[pos] = v;
    s = s + v;
  }
  s = wave_sum(s);
  if (lane == 0) g_sq[i] = s;
}

// The master query's backward by source: out[j,f] = w~_f * sum over j's out-edges e with argpos[dst_e, f] == e of
// g_sq[dst_e].  Group j = the by-source group, `dst` the gathered endpoint; positions, not source ids, are matched, so a
// duplicate edge is counted once.
template <int G, bool VEC>
__global__ __launch_bounds__(256) void asap_query_bwd_kernel(const int32_t* __restrict__ grp_ptr,
                                                             const int32_t* __restrict__ grp_perm,
                                                             const int64_t* __restrict__ dst,
                                                             const int32_t* __restrict__ argpos,
                                                             const float* __restrict__ g_sq,
                                                             const float* __restrict__ wt, int64_t n, int64_t E, int F,
                                                             float* __restrict__ out) {
  constexpr int W = VEC ? 4 : 1;
  constexpr int PER = 64 / G;
  const int lane = threadIdx.x & 63, sub = lane % G, slot = lane / G;
  const int64_t j = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (j >= n) return;
  const Group g = group_of(grp_ptr, j, E);
  for (int kb = 0; kb < F; kb += G * W) {
    const int k = kb + sub * W;
    float acc[W];
#pragma unroll
    for (int u = 0; u < W; ++u) acc[u] = 0.0f;
    for (int64_t e = g.b + slot; e < g.e; e += PER) {
      int64_t pos;
      const int64_t i = source_of(grp_perm, dst, e, E, n, &pos);
      if (i < 0 || k >= F) continue;
      const float gq = g_sq[i];
      const int32_t* a = argpos + i * F + k;
#pragma unroll
      for (int u = 0; u < W; ++u)
        if (k + u < F && static_cast<int64_t>(a[u]) == pos) acc[u] = acc[u] + gq;
    }
#pragma unroll
    for (int u = 0; u < W; ++u) acc[u] = wave_sum<64, G>(acc[u]);
    if (slot == 0 && k < F) {
#pragma unroll
      for (int u = 0; u < W; ++u)
        if (k + u < F) out[j * F + k + u] = acc[u] * wt[k + u];
    }
  }
}

template <template <int, bool> class Launch, typename... Args>
void dispatch_row_layout(bool vec, int64_t units, Args... args) {
  if (vec) {
    if (units <= 1) Launch<1, true>::go(args...);
    else if (units <= 2) Launch<2, true>::go(args...);
    else if (units <= 4) Launch<4, true>::go(args...);
    else if (units <= 8) Launch<8, true>::go(args...);
    else if (units <= 16) Launch<16, true>::go(args...);
    else if (units <= 32) Launch<32, true>::go(args...);
    else Launch<64, true>::go(args...);
  } else {
    if (units <= 1) Launch<1, false>::go(args...);
    else if (units <= 4) Launch<4, false>::go(args...);
    else if (units <= 16) Launch<16, false>::go(args...);
    else Launch<64, false>::go(args...);
  }
}

template <int G, bool VEC>
struct LaunchQuery {
  static void go(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* src, const float* x, int64_t ldx,
                 const float* wt, const float* c, int64_t n, int64_t E, int F, float* sq, int32_t* argpos,
                 hipStream_t stream) {
    hipLaunchKernelGGL((asap_query_kernel<G, VEC>), dim3(cdiv(n, 4)), dim3(256), 0, stream, grp_ptr, grp_perm, src, x,
                       ldx, wt, c, n, E, F, sq, argpos);
  }
};

template <int G, bool VEC>
struct LaunchEdgeDot {
  static void go(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* src, const float* g, const float* x,
                 int64_t ldx, int64_t n, int64_t E, int F, float* out, hipStream_t stream) {
    hipLaunchKernelGGL((asap_edge_dot_kernel<G, VEC>), dim3(cdiv(n, 4)), dim3(256), 0, stream, grp_ptr, grp_perm, src, g,
                       x, ldx, n, E, F, out);
  }
};

template <int G, bool VEC>
struct LaunchQueryBwd {
  static void go(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* dst, const int32_t* argpos,
                 const float* g_sq, const float* wt, int64_t n, int64_t E, int F, float* out, hipStream_t stream) {
    hipLaunchKernelGGL((asap_query_bwd_kernel<G, VEC>), dim3(cdiv(n, 4)), dim3(256), 0, stream, grp_ptr, grp_perm, dst,
                       argpos, g_sq, wt, n, E, F, out);
  }
};

template <int G, bool VEC>
struct LaunchAttend {
  static void go(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* src, const float* val, const float* x,
                 int64_t ldx, const float* w3, int64_t n, int64_t n_src, int64_t E, int F, float* out, float* p,
                 hipStream_t stream) {
    hipLaunchKernelGGL((asap_attend_kernel<G, VEC>), dim3(cdiv(n, 4)), dim3(256), 0, stream, grp_ptr, grp_perm, src,
                       val, x, ldx, w3, n, n_src, E, F, out, p);
  }
};

// 16-byte loads under row_project2's rule: x 16-byte aligned, a row stride that is a multiple of 4, at least 4 columns
inline bool rows_vectorise(const float* x, int64_t F, int64_t ldx) {
  return F >= 4 && (ldx % 4 == 0) && (reinterpret_cast<uintptr_t>(x) % 16 == 0);
}

inline int check_index_sizes(const char* what, int64_t N, int64_t E) {
  TGP_REQUIRE(N >= 0 && E >= 0, TGP_ERR_INVALID, "%s: bad size", what);
  TGP_REQUIRE(N < (1ll << 31) && E <= INT32_MAX, TGP_ERR_RANGE, "%s: N=%lld or E=%lld beyond the int32 index", what,
              static_cast<long long>(N), static_cast<long long>(E));
  return TGP_OK;
}

}  // namespace
}  // namespace tgp

using namespace tgp;

extern "C" int tgp_asap_query_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* src, const float* x_pool,
                                  int64_t ldx, const float* w_tilde, const float* c, int64_t N, int64_t E, int64_t F,
                                  float* sq, int32_t* argpos, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (int rc = check_index_sizes("tgp_asap_query_f32", N, E)) return rc;
  TGP_REQUIRE(F >= 0 && ldx >= F, TGP_ERR_INVALID, "tgp_asap_query_f32: bad size");
  TGP_REQUIRE(F < (1ll << 31), TGP_ERR_RANGE, "tgp_asap_query_f32: F too large");
  if (N == 0) return TGP_OK;
  TGP_REQUIRE(grp_ptr && c && sq && (E == 0 || src) && (F == 0 || (x_pool && w_tilde)), TGP_ERR_INVALID,
              "tgp_asap_query_f32: null pointer");
  const bool vec = rows_vectorise(x_pool, F, ldx);
  dispatch_row_layout<LaunchQuery>(vec, vec ? (F + 3) / 4 : F, grp_ptr, grp_perm, src, x_pool, ldx, w_tilde, c, N, E,
                                   static_cast<int>(F), sq, argpos, stream);
  return check_launch("tgp_asap_query_f32");
}

extern "C" int tgp_asap_edge_softmax_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* src,
                                         const float* sq, const float* sp, int64_t N, int64_t E, float negative_slope,
                                         float* alpha, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (int rc = check_index_sizes("tgp_asap_edge_softmax_f32", N, E)) return rc;
  if (N == 0 || E == 0) return TGP_OK;
  TGP_REQUIRE(grp_ptr && src && sq && sp && alpha, TGP_ERR_INVALID, "tgp_asap_edge_softmax_f32: null pointer");
  TGP_REQUIRE(alpha != sq && alpha != sp, TGP_ERR_INVALID,
              "tgp_asap_edge_softmax_f32: sq and sp are read by other waves, they cannot be the output");
  hipLaunchKernelGGL(asap_edge_softmax_kernel, dim3(cdiv(N, 4)), dim3(256), 0, stream, grp_ptr, grp_perm, src, sq, sp, N,
                     E, negative_slope, alpha);
  return check_launch("tgp_asap_edge_softmax_f32");
}

extern "C" int tgp_asap_attend_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* src, const float* val,
                                   const float* x, int64_t ldx, const float* w3, int64_t N, int64_t N_src, int64_t E,
                                   int64_t F, float* out, float* p, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (int rc = check_index_sizes("tgp_asap_attend_f32", N, E)) return rc;
  TGP_REQUIRE(F >= 0 && ldx >= F && N_src >= 0, TGP_ERR_INVALID, "tgp_asap_attend_f32: bad size");
  TGP_REQUIRE(F < (1ll << 31) && N_src < (1ll << 31), TGP_ERR_RANGE, "tgp_asap_attend_f32: F or N_src too large");
  if (N == 0) return TGP_OK;
  TGP_REQUIRE(grp_ptr && (E == 0 || src) && (F == 0 || (x && out)) && ((w3 == nullptr) == (p == nullptr)),
              TGP_ERR_INVALID, "tgp_asap_attend_f32: null pointer, or the projections without their output");
  TGP_REQUIRE(out != x, TGP_ERR_INVALID, "tgp_asap_attend_f32: x is read by other waves, it cannot be the output");
  const bool vec = rows_vectorise(x, F, ldx) && (F % 4 != 0 || reinterpret_cast<uintptr_t>(out) % 16 == 0);
  dispatch_row_layout<LaunchAttend>(vec, vec ? (F + 3) / 4 : F, grp_ptr, grp_perm, src, val, x, ldx, w3, N, N_src, E,
                                    static_cast<int>(F), out, p, stream);
  return check_launch("tgp_asap_attend_f32");
}

extern "C" int tgp_asap_leconv_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* src,
                                   const float* edge_weight, const float* p, const float* b1, const float* b3, int64_t N,
                                   int64_t E, int act, float* t_out, float* a_out, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (int rc = check_index_sizes("tgp_asap_leconv_f32", N, E)) return rc;
  TGP_REQUIRE(act >= 0 && act <= 2, TGP_ERR_INVALID,
              "tgp_asap_leconv_f32: act must be 0 (identity), 1 (tanh) or 2 (sigmoid)");
  if (N == 0) return TGP_OK;
  TGP_REQUIRE(grp_ptr && p && (t_out || a_out) && (E == 0 || src), TGP_ERR_INVALID, "tgp_asap_leconv_f32: null pointer");
  TGP_REQUIRE(p != t_out && p != a_out, TGP_ERR_INVALID,
              "tgp_asap_leconv_f32: p is read by other nodes, it cannot be an output");
  hipLaunchKernelGGL(asap_leconv_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, grp_ptr, grp_perm, src, edge_weight,
                     p, b1, b3, N, E, act, t_out, a_out);
  return check_launch("tgp_asap_leconv_f32");
}

extern "C" int tgp_asap_edge_dot_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* src, const float* g,
                                     const float* x, int64_t ldx, int64_t N, int64_t E, int64_t F, float* out,
                                     void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (int rc = check_index_sizes("tgp_asap_edge_dot_f32", N, E)) return rc;
  TGP_REQUIRE(F >= 0 && ldx >= F, TGP_ERR_INVALID, "tgp_asap_edge_dot_f32: bad size");
  TGP_REQUIRE(F < (1ll << 31), TGP_ERR_RANGE, "tgp_asap_edge_dot_f32: F too large");
  if (N == 0 || E == 0) return TGP_OK;
  TGP_REQUIRE(grp_ptr && src && out && (F == 0 || (g && x)), TGP_ERR_INVALID, "tgp_asap_edge_dot_f32: null pointer");
  // g is [N, F] contiguous: its rows take 16-byte loads only when F % 4 == 0 and g is aligned
  const bool vec = rows_vectorise(x, F, ldx) && F % 4 == 0 && reinterpret_cast<uintptr_t>(g) % 16 == 0;
  dispatch_row_layout<LaunchEdgeDot>(vec, vec ? (F + 3) / 4 : F, grp_ptr, grp_perm, src, g, x, ldx, N, E,
                                     static_cast<int>(F), out, stream);
  return check_launch("tgp_asap_edge_dot_f32");
}

extern "C" int tgp_asap_softmax_bwd_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* src,
                                        const float* alpha, const float* g_alpha, const float* sq, const float* sp,
                                        int64_t N, int64_t E, float negative_slope, float* g_l, float* g_sq,
                                        void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (int rc = check_index_sizes("tgp_asap_softmax_bwd_f32", N, E)) return rc;
  if (N == 0) return TGP_OK;
  TGP_REQUIRE(grp_ptr && sq && sp && g_sq && (E == 0 || (src && alpha && g_alpha && g_l)), TGP_ERR_INVALID,
              "tgp_asap_softmax_bwd_f32: null pointer");
  // (a list without edges hands every per-edge pointer as NULL: only g_sq, all zeros, is written)
  TGP_REQUIRE((E == 0 || (g_l != alpha && g_l != g_alpha)) && g_sq != sq && g_sq != sp, TGP_ERR_INVALID,
              "tgp_asap_softmax_bwd_f32: an input given as an output");
  hipLaunchKernelGGL(asap_softmax_bwd_kernel, dim3(cdiv(N, 4)), dim3(256), 0, stream, grp_ptr, grp_perm, src, alpha,
                     g_alpha, sq, sp, N, E, negative_slope, g_l, g_sq);
  return check_launch("tgp_asap_softmax_bwd_f32");
}

extern "C" int tgp_asap_query_bwd_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* dst,
                                      const int32_t* argpos, const float* g_sq, const float* w_tilde, int64_t N,
                                      int64_t E, int64_t F, float* out, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (int rc = check_index_sizes("tgp_asap_query_bwd_f32", N, E)) return rc;
  TGP_REQUIRE(F >= 0, TGP_ERR_INVALID, "tgp_asap_query_bwd_f32: bad size");
  TGP_REQUIRE(F < (1ll << 31), TGP_ERR_RANGE, "tgp_asap_query_bwd_f32: F too large");
  if (N == 0 || F == 0) return TGP_OK;
  TGP_REQUIRE(grp_ptr && argpos && g_sq && w_tilde && out && (E == 0 || dst), TGP_ERR_INVALID,
              "tgp_asap_query_bwd_f32: null pointer");
  dispatch_row_layout<LaunchQueryBwd>(false, F, grp_ptr, grp_perm, dst, argpos, g_sq, w_tilde, N, E, static_cast<int>(F),
                                      out, stream);
  return check_launch("tgp_asap_query_bwd_f32");
}
