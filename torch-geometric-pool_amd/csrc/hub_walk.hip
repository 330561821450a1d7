// The hub route of ASAPooling's fitness (asap.hip) and SAGPooling's scorer (sag_score.hip): a group with very many
// entries is cut into chunks of HW_CHUNK entries and ONE WAVE OWNS ONE (hub, chunk), so a power-law graph no longer runs
// as long as its largest node.  The host plan (tgp/kernels.py: hub_ids [H] ascending, chunk_ptr [H + 1]) names the hubs;
// chunk c of a hub covers entries b + c C .. min(b + (c + 1) C, e) of its group [b, e), a function of the group alone.
// Inside a chunk the lane layout is asap.hip's (edge_walk.h).  Every chunk leaves a partial record in the workspace and a
// tail folds the records of a hub in a fixed order, then writes the hub node's outputs over what the run on the light
// index (every hub group emptied) left there:
//   scalar aggregate   (s, wsum) per chunk; tail: one wave per hub, lane l adds records l, l + 64, .. in ascending order,
//                      then the butterfly 32 .. 1, then t and act(t) as sag_aggregate_kernel / asap_leconv_kernel do
//   query              m[F], arg[F] (edge POSITIONS) and "any valid entry"; tail: better() across the chunks, sq, argpos
//   edge softmax       (m, sum exp(l - m)); pass 2 is chunk-parallel again: every chunk wave folds the hub's records to
//                      (M, S + 1e-16) and writes alpha at its edges' own positions
//   attend             a partial row; tail: the sum, the stored row and its three projections
//   edge dot           no record: chunks are independent
//   softmax backward   sum alpha g_alpha; pass 2 writes g_l per edge and leaves sum g_l; tail: g_sq
//   query backward     a partial row of matched g_sq; tail: the sum times w~
// Row tails: one workgroup of 1024 per hub = 16 slots x 64 columns; slot s folds records s, s + 16, .. of a column in
// ascending order, LDS hands the 16 partial values to slot 0, which folds them in slot order; column blocks of 64 in
// ascending order.  No float atomics and one order per sum, so the same bits on every call; the order depends on the
// group alone, never on the device or on the rest of the list.  A position outside [0, E) or an endpoint outside its
// range is skipped and never dereferenced; a record index is clamped to the workspace the plan sized.
#include <math.h>

#include "common.h"
#include "edge_walk.h"
#include "hub_plan.h"  // HW_CHUNK, HW_TAIL_SLOTS, HubPlan, HubItem, hub_of, hub_item

namespace tgp {
namespace {

// sum of one float of every record of a hub: lane-strided in ascending order, then the butterfly
__device__ __forceinline__ float fold_records(const float* __restrict__ rec, int stride, const HubItem& it, int lane) {
  float s = 0.0f;
  for (int c = lane; c < it.count; c += 64) s = s + rec[static_cast<int64_t>(it.first + c) * stride];
  return wave_sum(s);
}

__device__ __forceinline__ float leaky(float t, float slope) { return t > 0.0f ? t : t * slope; }

// ---- the scalar aggregate (SAG's sum of p[src], ASAP's LEConv) ---------------------------------------------------------
__global__ __launch_bounds__(256) void hub_scalar_chunk_kernel(HubPlan pl, const int32_t* __restrict__ grp_ptr,
                                                               const int32_t* __restrict__ grp_perm,
                                                               const int64_t* __restrict__ src,
                                                               const float* __restrict__ ew, const float* __restrict__ p,
                                                               int64_t n, int64_t E, float2* __restrict__ rec) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (w >= pl.T) return;  // wave-uniform
  HubItem it;
  float s = 0.0f, wsum = 0.0f;
  if (hub_item(pl, grp_ptr, w, n, E, &it)) {
    for (int64_t e = it.b + lane; e < it.e; e += 64) {
      int64_t pos;
      const int64_t r = source_of(grp_perm, src, e, E, n, &pos);
      if (r < 0) continue;
      const float wgt = ew ? ew[pos] : 1.0f;
      s = fmaf(wgt, p[r], s);
      wsum = wsum + wgt;
    }
  }
  s = wave_sum(s);
  wsum = wave_sum(wsum);
  if (lane == 0) rec[w] = make_float2(s, wsum);
}

// leconv != 0: t = ((p[2n + i] + b3) + s) + (b1 - p[n + i]) W (bias = b3); else t = (s [/ max(size, 1)] + bias) + q[i]
__global__ __launch_bounds__(256) void hub_scalar_tail_kernel(HubPlan pl, const int32_t* __restrict__ grp_ptr,
                                                              const float2* __restrict__ rec, const float* __restrict__ p,
                                                              const float* __restrict__ q, const float* __restrict__ bias,
                                                              const float* __restrict__ b1, int64_t n, int64_t E,
                                                              int leconv, int mean, int act, float* __restrict__ t_out,
                                                              float* __restrict__ a_out) {
  const int lane = threadIdx.x & 63;
  const int64_t h = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (h >= pl.H) return;
  HubItem it;
  if (!hub_of(pl, static_cast<int>(h), n, &it)) return;
  const float* r = reinterpret_cast<const float*>(rec);
  const float s = fold_records(r, 2, it, lane), wsum = fold_records(r + 1, 2, it, lane);
  if (lane != 0) return;
  const int64_t i = it.node;
  float t;
  if (leconv) {
    t = ((p[2 * n + i] + (bias ? bias[0] : 0.0f)) + s) + ((b1 ? b1[0] : 0.0f) - p[n + i]) * wsum;
  } else {
    const Group g = group_of(grp_ptr, i, E);
    float acc = s;
    if (mean) acc = acc / static_cast<float>(g.e - g.b > 1 ? g.e - g.b : 1);
    t = acc + (bias ? bias[0] : 0.0f);
    if (q) t = t + q[i];
  }
  if (t_out) t_out[i] = t;
  if (a_out) a_out[i] = act == 1 ? tanhf(t) : act == 2 ? 1.0f / (1.0f + expf(-t)) : t;
}

// ---- the row operators: chunk kernels -----------------------------------------------------------------------------------
// the maxima of a chunk, column by column: asap_query_kernel's walk over the chunk's entries
template <int G, bool VEC>
__global__ __launch_bounds__(256) void hub_query_chunk_kernel(HubPlan pl, const int32_t* __restrict__ grp_ptr,
                                                              const int32_t* __restrict__ grp_perm,
                                                              const int64_t* __restrict__ src,
                                                              const float* __restrict__ x, int64_t ldx, int64_t n,
                                                              int64_t E, int F, float* __restrict__ rec,
                                                              int32_t* __restrict__ arg_rec, int32_t* __restrict__ any_rec) {
  constexpr int W = VEC ? 4 : 1;
  constexpr int PER = 64 / G;
  const int lane = threadIdx.x & 63, sub = lane % G, slot = lane / G;
  const int64_t w = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (w >= pl.T) return;
  HubItem it;
  if (!hub_item(pl, grp_ptr, w, n, E, &it)) it.b = it.e = 0;
  bool any = false;
  for (int kb = 0; kb < F; kb += G * W) {
    const int k = kb + sub * W;
    float m[W];
    int32_t arg[W];
#pragma unroll
    for (int j = 0; j < W; ++j) {
      m[j] = -INFINITY;
      arg[j] = INT32_MAX;
    }
    for (int64_t e = it.b + slot; e < it.e; e += PER) {
      int64_t pos;
      const int64_t r = source_of(grp_perm, src, e, E, n, &pos);
      if (r < 0) continue;
      any = true;
      if (k < F) {
        float v[W];
        load_unit<VEC>(x + r * ldx, k, F, -INFINITY, v);
#pragma unroll
        for (int j = 0; j < W; ++j) {
          if (arg_rec && better(v[j], static_cast<int32_t>(pos), m[j], arg[j])) arg[j] = static_cast<int32_t>(pos);
          m[j] = nan_max(m[j], v[j]);
        }
      }
    }
    if (arg_rec) {
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
    } else {
#pragma unroll
      for (int j = 0; j < W; ++j) m[j] = wave_fold<64, G>(m[j], op_nanmax{});
    }
    if (slot == 0 && k < F) {
#pragma unroll
      for (int j = 0; j < W; ++j) {
        if (k + j < F) {
          rec[w * F + k + j] = m[j];
          if (arg_rec) arg_rec[w * F + k + j] = arg[j];
        }
      }
    }
  }
  const bool have = __any(any);
  if (lane == 0) any_rec[w] = have ? 1 : 0;
}

// the partial row of a chunk: asap_attend_kernel's walk
template <int G, bool VEC>
__global__ __launch_bounds__(256) void hub_attend_chunk_kernel(HubPlan pl, const int32_t* __restrict__ grp_ptr,
                                                               const int32_t* __restrict__ grp_perm,
                                                               const int64_t* __restrict__ src,
                                                               const float* __restrict__ val, const float* __restrict__ x,
                                                               int64_t ldx, int64_t n, int64_t n_src, int64_t E, int F,
                                                               float* __restrict__ rec) {
  constexpr int W = VEC ? 4 : 1;
  constexpr int PER = 64 / G;
  const int lane = threadIdx.x & 63, sub = lane % G, slot = lane / G;
  const int64_t w = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (w >= pl.T) return;
  HubItem it;
  if (!hub_item(pl, grp_ptr, w, n, E, &it)) it.b = it.e = 0;
  for (int kb = 0; kb < F; kb += G * W) {
    const int k = kb + sub * W;
    float acc[W];
#pragma unroll
    for (int j = 0; j < W; ++j) acc[j] = 0.0f;
    for (int64_t e = it.b + slot; e < it.e; e += PER) {
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
    for (int j = 0; j < W; ++j) acc[j] = wave_sum<64, G>(acc[j]);
    if (slot == 0 && k < F) {
#pragma unroll
      for (int j = 0; j < W; ++j)
        if (k + j < F) rec[w * F + k + j] = acc[j];
    }
  }
}

// the matched g_sq of a chunk of a by-source group: asap_query_bwd_kernel's walk (w~ is applied by the tail)
template <int G, bool VEC>
__global__ __launch_bounds__(256) void hub_query_bwd_chunk_kernel(HubPlan pl, const int32_t* __restrict__ grp_ptr,
                                                                  const int32_t* __restrict__ grp_perm,
                                                                  const int64_t* __restrict__ dst,
                                                                  const int32_t* __restrict__ argpos,
                                                                  const float* __restrict__ g_sq, int64_t n, int64_t E,
                                                                  int F, float* __restrict__ rec) {
  constexpr int W = VEC ? 4 : 1;
  constexpr int PER = 64 / G;
  const int lane = threadIdx.x & 63, sub = lane % G, slot = lane / G;
  const int64_t w = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (w >= pl.T) return;
  HubItem it;
  if (!hub_item(pl, grp_ptr, w, n, E, &it)) it.b = it.e = 0;
  for (int kb = 0; kb < F; kb += G * W) {
    const int k = kb + sub * W;
    float acc[W];
#pragma unroll
    for (int u = 0; u < W; ++u) acc[u] = 0.0f;
    for (int64_t e = it.b + slot; e < it.e; e += PER) {
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
        if (k + u < F) rec[w * F + k + u] = acc[u];
    }
  }
}

// g_alpha of a chunk's edges: asap_edge_dot_kernel's walk, the g row's first column block in registers per wave
template <int G, bool VEC>
__global__ __launch_bounds__(256) void hub_edge_dot_kernel(HubPlan pl, const int32_t* __restrict__ grp_ptr,
                                                           const int32_t* __restrict__ grp_perm,
                                                           const int64_t* __restrict__ src, const float* __restrict__ g,
                                                           const float* __restrict__ x, int64_t ldx, int64_t n, int64_t E,
                                                           int F, float* __restrict__ out) {
  constexpr int W = VEC ? 4 : 1;
  constexpr int PER = 64 / G;
  const int lane = threadIdx.x & 63, sub = lane % G, slot = lane / G;
  const int64_t w = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (w >= pl.T) return;
  HubItem it;
  if (!hub_item(pl, grp_ptr, w, n, E, &it)) return;  // wave-uniform
  const float* grow = g + it.node * F;
  float g0[W];
  load_unit<VEC>(grow, sub * W, F, 0.0f, g0);
  const int64_t rounds = (it.e - it.b + PER - 1) / PER;  // every lane takes part in every fold
  for (int64_t t = 0; t < rounds; ++t) {
    const int64_t e = it.b + t * PER + slot;
    int64_t pos = -1, r = -1;
    if (e < it.e) r = source_of(grp_perm, src, e, E, n, &pos);
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
    if (sub == 0 && e < it.e && static_cast<uint64_t>(pos) < static_cast<uint64_t>(E)) out[pos] = r >= 0 ? acc : 0.0f;
  }
}

// ---- the row tail ---------------------------------------------------------------------------------------------------------
enum { HW_QUERY = 0, HW_ATTEND = 1, HW_QUERY_BWD = 2 };

// One workgroup per hub.  HW_QUERY: the maxima and their positions across the chunks (a chunk without a valid entry
// contributes nothing), argpos, sq = <m, w~> + c.  HW_ATTEND: the summed row to out, p[k n + i] = <row, w3[k]>.
// HW_QUERY_BWD: the summed row times w~ to out.
template <int MODE>
__global__ __launch_bounds__(64 * HW_TAIL_SLOTS) void hub_row_tail_kernel(
    HubPlan pl, const float* __restrict__ rec, const int32_t* __restrict__ arg_rec, const int32_t* __restrict__ any_rec,
    const float* __restrict__ wt, const float* __restrict__ c, int64_t n, int F, float* __restrict__ out,
    float* __restrict__ sq, int32_t* __restrict__ argpos, float* __restrict__ p) {
  __shared__ float sh_v[HW_TAIL_SLOTS][64];
  __shared__ int32_t sh_a[HW_TAIL_SLOTS][64];
  const int col = threadIdx.x & 63, slot = threadIdx.x >> 6;
  HubItem it;
  if (!hub_of(pl, static_cast<int>(blockIdx.x), n, &it)) return;  // uniform over the workgroup
  const int64_t i = it.node;
  bool have = false;
  if (MODE == HW_QUERY && slot == 0) {
    int a = 0;
    for (int ch = col; ch < it.count; ch += 64) a |= any_rec[it.first + ch];
    have = __any(a != 0);
  }
  float d1 = 0.0f, d2 = 0.0f, d3 = 0.0f;
  for (int kb = 0; kb < F; kb += 64) {
    const int k = kb + col;
    float v = MODE == HW_QUERY ? -INFINITY : 0.0f;
    int32_t arg = INT32_MAX;
    if (k < F) {
      for (int ch = slot; ch < it.count; ch += HW_TAIL_SLOTS) {
        const int64_t at = static_cast<int64_t>(it.first + ch) * F + k;
        if (MODE == HW_QUERY) {
          if (!any_rec[it.first + ch]) continue;
          const float o = rec[at];
          if (arg_rec) {
            const int32_t oa = arg_rec[at];
            if (better(o, oa, v, arg)) arg = oa;
          }
          v = nan_max(v, o);
        } else {
          v = v + rec[at];
        }
      }
    }
    sh_v[slot][col] = v;
    if (MODE == HW_QUERY) sh_a[slot][col] = arg;
    __syncthreads();
    if (slot == 0 && k < F) {
      for (int s = 1; s < HW_TAIL_SLOTS; ++s) {
        const float o = sh_v[s][col];
        if (MODE == HW_QUERY) {
          const int32_t oa = sh_a[s][col];
          if (arg_rec && better(o, oa, v, arg)) arg = oa;
          v = nan_max(v, o);
        } else {
          v = v + o;
        }
      }
      if (MODE == HW_QUERY) {
        if (argpos) argpos[i * F + k] = arg == INT32_MAX ? -1 : arg;
        if (have) d1 = fmaf(v, wt[k], d1);
      } else if (MODE == HW_ATTEND) {
        out[i * F + k] = v;
        if (wt) {
          d1 = fmaf(v, wt[k], d1);
          d2 = fmaf(v, wt[F + k], d2);
          d3 = fmaf(v, wt[2 * static_cast<int64_t>(F) + k], d3);
        }
      } else {
        out[i * F + k] = v * wt[k];
      }
    }
    __syncthreads();
  }
  if (slot != 0) return;
  if (MODE == HW_QUERY) {
    d1 = wave_sum(d1);
    if (col == 0) sq[i] = d1 + c[0];
  } else if (MODE == HW_ATTEND && wt) {
    d1 = wave_sum(d1);
    d2 = wave_sum(d2);
    d3 = wave_sum(d3);
    if (col == 0) {
      p[i] = d1;
      p[n + i] = d2;
      p[2 * n + i] = d3;
    }
  }
}

// ---- the edge softmax and its backward ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hub_softmax_chunk_kernel(HubPlan pl, const int32_t* __restrict__ grp_ptr,
                                                                const int32_t* __restrict__ grp_perm,
                                                                const int64_t* __restrict__ src,
                                                                const float* __restrict__ sq, const float* __restrict__ sp,
                                                                int64_t n, int64_t E, float slope,
                                                                float2* __restrict__ rec) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (w >= pl.T) return;
  HubItem it;
  float m = -INFINITY, s = 0.0f;
  if (hub_item(pl, grp_ptr, w, n, E, &it)) {
    const float q = sq[it.node];
    for (int64_t e = it.b + lane; e < it.e; e += 64) {
      int64_t pos;
      const int64_t r = source_of(grp_perm, src, e, E, n, &pos);
      if (r >= 0) m = nan_max(m, leaky(q + sp[r], slope));
    }
    m = wave_nanmax(m);
    for (int64_t e = it.b + lane; e < it.e; e += 64) {
      int64_t pos;
      const int64_t r = source_of(grp_perm, src, e, E, n, &pos);
      if (r >= 0) s = s + expf(leaky(q + sp[r], slope) - m);
    }
    s = wave_sum(s);
  }
  if (lane == 0) rec[w] = make_float2(m, s);
}

__global__ __launch_bounds__(256) void hub_softmax_write_kernel(HubPlan pl, const int32_t* __restrict__ grp_ptr,
                                                                const int32_t* __restrict__ grp_perm,
                                                                const int64_t* __restrict__ src,
                                                                const float* __restrict__ sq, const float* __restrict__ sp,
                                                                int64_t n, int64_t E, float slope,
                                                                const float2* __restrict__ rec, float* __restrict__ alpha) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (w >= pl.T) return;
  HubItem it;
  if (!hub_item(pl, grp_ptr, w, n, E, &it)) return;
  // every chunk folds the hub's records the same way: the maximum has no order, the sum goes lane-strided in ascending
  // chunk order and through the butterfly; a chunk without a valid entry left (-inf, 0) and adds nothing
  float m = -INFINITY;
  for (int ch = lane; ch < it.count; ch += 64) m = nan_max(m, rec[it.first + ch].x);
  m = wave_nanmax(m);
  float s = 0.0f;
  for (int ch = lane; ch < it.count; ch += 64) {
    const float2 r = rec[it.first + ch];
    if (r.y != 0.0f) s = s + r.y * expf(r.x - m);
  }
  s = wave_sum(s) + 1e-16f;
  const float q = sq[it.node];
  for (int64_t e = it.b + lane; e < it.e; e += 64) {
    int64_t pos;
    const int64_t r = source_of(grp_perm, src, e, E, n, &pos);
    if (r < 0) {
      if (static_cast<uint64_t>(pos) < static_cast<uint64_t>(E)) alpha[pos] = 0.0f;
      continue;
    }
    alpha[pos] = expf(leaky(q + sp[r], slope) - m) / s;
  }
}

__global__ __launch_bounds__(256) void hub_softmax_bwd_chunk_kernel(HubPlan pl, const int32_t* __restrict__ grp_ptr,
                                                                    const int32_t* __restrict__ grp_perm,
                                                                    const int64_t* __restrict__ src,
                                                                    const float* __restrict__ alpha,
                                                                    const float* __restrict__ g_alpha, int64_t n,
                                                                    int64_t E, float* __restrict__ rec_d) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (w >= pl.T) return;
  HubItem it;
  float d = 0.0f;
  if (hub_item(pl, grp_ptr, w, n, E, &it)) {
    for (int64_t e = it.b + lane; e < it.e; e += 64) {
      int64_t pos;
      if (source_of(grp_perm, src, e, E, n, &pos) < 0) continue;
      d = fmaf(alpha[pos], g_alpha[pos], d);
    }
  }
  d = wave_sum(d);
  if (lane == 0) rec_d[w] = d;
}

__global__ __launch_bounds__(256) void hub_softmax_bwd_write_kernel(HubPlan pl, const int32_t* __restrict__ grp_ptr,
                                                                    const int32_t* __restrict__ grp_perm,
                                                                    const int64_t* __restrict__ src,
                                                                    const float* __restrict__ alpha,
                                                                    const float* __restrict__ g_alpha,
                                                                    const float* __restrict__ sq,
                                                                    const float* __restrict__ sp, int64_t n, int64_t E,
                                                                    float slope, const float* __restrict__ rec_d,
                                                                    float* __restrict__ rec_s, float* __restrict__ g_l) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (w >= pl.T) return;
  HubItem it;
  float s = 0.0f;
  if (hub_item(pl, grp_ptr, w, n, E, &it)) {
    const float d = fold_records(rec_d, 1, it, lane);
    const float q = sq[it.node];
    for (int64_t e = it.b + lane; e < it.e; e += 64) {
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
  }
  s = wave_sum(s);
  if (lane == 0) rec_s[w] = s;
}

// out[hub node] = the sum of one float per record: one wave per hub
__global__ __launch_bounds__(256) void hub_sum_tail_kernel(HubPlan pl, const float* __restrict__ rec, int64_t n,
                                                           float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t h = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (h >= pl.H) return;
  HubItem it;
  if (!hub_of(pl, static_cast<int>(h), n, &it)) return;
  const float s = fold_records(rec, 1, it, lane);
  if (lane == 0) out[it.node] = s;
}

// ---- host -------------------------------------------------------------------------------------------------------------
template <int G, bool VEC>
struct LaunchHubQuery {
  static void go(HubPlan pl, const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* src, const float* x,
                 int64_t ldx, int64_t n, int64_t E, int F, float* rec, int32_t* arg_rec, int32_t* any_rec,
                 hipStream_t stream) {
    hipLaunchKernelGGL((hub_query_chunk_kernel<G, VEC>), dim3(cdiv(pl.T, 4)), dim3(256), 0, stream, pl, grp_ptr, grp_perm,
                       src, x, ldx, n, E, F, rec, arg_rec, any_rec);
  }
};

template <int G, bool VEC>
struct LaunchHubAttend {
  static void go(HubPlan pl, const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* src, const float* val,
                 const float* x, int64_t ldx, int64_t n, int64_t n_src, int64_t E, int F, float* rec,
                 hipStream_t stream) {
    hipLaunchKernelGGL((hub_attend_chunk_kernel<G, VEC>), dim3(cdiv(pl.T, 4)), dim3(256), 0, stream, pl, grp_ptr,
                       grp_perm, src, val, x, ldx, n, n_src, E, F, rec);
  }
};

template <int G, bool VEC>
struct LaunchHubQueryBwd {
  static void go(HubPlan pl, const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* dst, const int32_t* argpos,
                 const float* g_sq, int64_t n, int64_t E, int F, float* rec, hipStream_t stream) {
    hipLaunchKernelGGL((hub_query_bwd_chunk_kernel<G, VEC>), dim3(cdiv(pl.T, 4)), dim3(256), 0, stream, pl, grp_ptr,
                       grp_perm, dst, argpos, g_sq, n, E, F, rec);
  }
};

template <int G, bool VEC>
struct LaunchHubEdgeDot {
  static void go(HubPlan pl, const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* src, const float* g,
                 const float* x, int64_t ldx, int64_t n, int64_t E, int F, float* out, hipStream_t stream) {
    hipLaunchKernelGGL((hub_edge_dot_kernel<G, VEC>), dim3(cdiv(pl.T, 4)), dim3(256), 0, stream, pl, grp_ptr, grp_perm,
                       src, g, x, ldx, n, E, F, out);
  }
};

// the workspace: float rec [T, F] | int32 arg [T, F] | 4 floats per chunk (pairs, flags, scalar records)
struct HubWorkspace {
  float* rec;
  int32_t* arg;
  float* misc;
};

inline size_t hub_workspace_bytes(int64_t T, int64_t F) {
  const size_t rows = align_up(static_cast<size_t>(T) * static_cast<size_t>(F) * 4);
  return 2 * rows + align_up(static_cast<size_t>(T) * 16);
}

inline HubWorkspace carve_hub_workspace(void* ws, int64_t T, int64_t F) {
  const size_t rows = align_up(static_cast<size_t>(T) * static_cast<size_t>(F) * 4);
  char* base = static_cast<char*>(ws);
  return {reinterpret_cast<float*>(base), reinterpret_cast<int32_t*>(base + rows),
          reinterpret_cast<float*>(base + 2 * rows)};
}

// 1: nothing to do (an empty plan or no node); 0: go on; below zero: refused
inline int check_hub_call(const char* what, const int32_t* grp_ptr, const int32_t* hub_ids, const int32_t* chunk_ptr,
                          int64_t H, int64_t T, int64_t N, int64_t E, int64_t F, const void* ws, size_t ws_bytes,
                          bool needs_ws) {
  if (int rc = check_index_sizes(what, N, E)) return rc;
  TGP_REQUIRE(H >= 0 && T >= 0 && F >= 0, TGP_ERR_INVALID, "%s: bad size", what);
  TGP_REQUIRE(H <= INT32_MAX && T <= INT32_MAX && F < (1ll << 31), TGP_ERR_RANGE, "%s: H, T or F beyond int32", what);
  if (N == 0 || H == 0 || T == 0) return 1;
  TGP_REQUIRE(grp_ptr && hub_ids && chunk_ptr, TGP_ERR_INVALID, "%s: null index or plan pointer", what);
  if (needs_ws) {
    TGP_REQUIRE(ws && reinterpret_cast<uintptr_t>(ws) % 16 == 0, TGP_ERR_INVALID, "%s: no (16-byte aligned) workspace",
                what);
    TGP_REQUIRE(ws_bytes >= hub_workspace_bytes(T, F), TGP_ERR_INVALID, "%s: workspace of %zu bytes, %zu needed", what,
                ws_bytes, hub_workspace_bytes(T, F));
  }
  return 0;
}

#define HUB_CHECK(...)                          \
  do {                                          \
    const int rc_ = check_hub_call(__VA_ARGS__); \
    if (rc_ != 0) return rc_ < 0 ? rc_ : TGP_OK; \
  } while (0)

}  // namespace
}  // namespace tgp

using namespace tgp;

extern "C" int tgp_hubwalk_chunk(void) { return HW_CHUNK; }

extern "C" size_t tgp_hubwalk_workspace_bytes(int64_t T, int64_t F) {
  if (T <= 0 || F < 0) return 0;
  return hub_workspace_bytes(T, F);
}

extern "C" int tgp_hubwalk_scalar_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* src,
                                      const int32_t* hub_ids, const int32_t* chunk_ptr, int64_t H, int64_t T,
                                      const float* edge_weight, const float* p, const float* q, const float* bias,
                                      const float* b1, int64_t N, int64_t E, int leconv, int mean, int act, float* t_out,
                                      float* a_out, void* ws, size_t ws_bytes, void* stream_) {
  const char* what = "tgp_hubwalk_scalar_f32";
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HUB_CHECK(what, grp_ptr, hub_ids, chunk_ptr, H, T, N, E, 0, ws, ws_bytes, true);
  TGP_REQUIRE((leconv == 0 || leconv == 1) && (mean == 0 || mean == 1) && act >= 0 && act <= 2, TGP_ERR_INVALID,
              "%s: leconv and mean are 0 or 1, act 0 (identity), 1 (tanh) or 2 (sigmoid)", what);
  TGP_REQUIRE(p && (t_out || a_out) && (E == 0 || src), TGP_ERR_INVALID, "%s: null pointer", what);
  TGP_REQUIRE(p != t_out && p != a_out, TGP_ERR_INVALID, "%s: p is read by other nodes, it cannot be an output", what);
  const HubPlan pl{hub_ids, chunk_ptr, static_cast<int>(H), static_cast<int>(T)};
  float2* rec = reinterpret_cast<float2*>(carve_hub_workspace(ws, T, 0).misc);
  hipLaunchKernelGGL(hub_scalar_chunk_kernel, dim3(cdiv(T, 4)), dim3(256), 0, stream, pl, grp_ptr, grp_perm, src,
                     edge_weight, p, N, E, rec);
  hipLaunchKernelGGL(hub_scalar_tail_kernel, dim3(cdiv(H, 4)), dim3(256), 0, stream, pl, grp_ptr, rec, p, q, bias, b1, N,
                     E, leconv, mean, act, t_out, a_out);
  return check_launch(what);
}

extern "C" int tgp_hubwalk_query_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* src,
                                     const int32_t* hub_ids, const int32_t* chunk_ptr, int64_t H, int64_t T,
                                     const float* x_pool, int64_t ldx, const float* w_tilde, const float* c, int64_t N,
                                     int64_t E, int64_t F, float* sq, int32_t* argpos, void* ws, size_t ws_bytes,
                                     void* stream_) {
  const char* what = "tgp_hubwalk_query_f32";
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HUB_CHECK(what, grp_ptr, hub_ids, chunk_ptr, H, T, N, E, F, ws, ws_bytes, true);
  TGP_REQUIRE(ldx >= F, TGP_ERR_INVALID, "%s: bad size", what);
  TGP_REQUIRE(c && sq && (E == 0 || src) && (F == 0 || (x_pool && w_tilde)), TGP_ERR_INVALID, "%s: null pointer", what);
  const HubPlan pl{hub_ids, chunk_ptr, static_cast<int>(H), static_cast<int>(T)};
  const HubWorkspace w = carve_hub_workspace(ws, T, F);
  int32_t* any_rec = reinterpret_cast<int32_t*>(w.misc);
  const bool vec = rows_vectorise(x_pool, F, ldx);
  dispatch_row_layout<LaunchHubQuery>(vec, vec ? (F + 3) / 4 : F, pl, grp_ptr, grp_perm, src, x_pool, ldx, N, E,
                                      static_cast<int>(F), w.rec, argpos ? w.arg : nullptr, any_rec, stream);
  hipLaunchKernelGGL(hub_row_tail_kernel<HW_QUERY>, dim3(static_cast<unsigned>(H)), dim3(64 * HW_TAIL_SLOTS), 0, stream,
                     pl, w.rec, argpos ? w.arg : nullptr, any_rec, w_tilde, c, N, static_cast<int>(F), nullptr, sq,
                     argpos, nullptr);
  return check_launch(what);
}

extern "C" int tgp_hubwalk_edge_softmax_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* src,
                                            const int32_t* hub_ids, const int32_t* chunk_ptr, int64_t H, int64_t T,
                                            const float* sq, const float* sp, int64_t N, int64_t E, float negative_slope,
                                            float* alpha, void* ws, size_t ws_bytes, void* stream_) {
  const char* what = "tgp_hubwalk_edge_softmax_f32";
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HUB_CHECK(what, grp_ptr, hub_ids, chunk_ptr, H, T, N, E, 0, ws, ws_bytes, true);
  if (E == 0) return TGP_OK;
  TGP_REQUIRE(src && sq && sp && alpha, TGP_ERR_INVALID, "%s: null pointer", what);
  TGP_REQUIRE(alpha != sq && alpha != sp, TGP_ERR_INVALID,
              "%s: sq and sp are read by other waves, they cannot be the output", what);
  const HubPlan pl{hub_ids, chunk_ptr, static_cast<int>(H), static_cast<int>(T)};
  float2* rec = reinterpret_cast<float2*>(carve_hub_workspace(ws, T, 0).misc);
  hipLaunchKernelGGL(hub_softmax_chunk_kernel, dim3(cdiv(T, 4)), dim3(256), 0, stream, pl, grp_ptr, grp_perm, src, sq, sp,
                     N, E, negative_slope, rec);
  hipLaunchKernelGGL(hub_softmax_write_kernel, dim3(cdiv(T, 4)), dim3(256), 0, stream, pl, grp_ptr, grp_perm, src, sq, sp,
                     N, E, negative_slope, rec, alpha);
  return check_launch(what);
}

extern "C" int tgp_hubwalk_attend_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* src,
                                      const int32_t* hub_ids, const int32_t* chunk_ptr, int64_t H, int64_t T,
                                      const float* val, const float* x, int64_t ldx, const float* w3, int64_t N,
                                      int64_t N_src, int64_t E, int64_t F, float* out, float* p, void* ws,
                                      size_t ws_bytes, void* stream_) {
  const char* what = "tgp_hubwalk_attend_f32";
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HUB_CHECK(what, grp_ptr, hub_ids, chunk_ptr, H, T, N, E, F, ws, ws_bytes, true);
  TGP_REQUIRE(ldx >= F && N_src >= 0, TGP_ERR_INVALID, "%s: bad size", what);
  TGP_REQUIRE(N_src < (1ll << 31), TGP_ERR_RANGE, "%s: N_src too large", what);
  TGP_REQUIRE((E == 0 || src) && (F == 0 || (x && out)) && ((w3 == nullptr) == (p == nullptr)), TGP_ERR_INVALID,
              "%s: null pointer, or the projections without their output", what);
  TGP_REQUIRE(out != x, TGP_ERR_INVALID, "%s: x is read by other waves, it cannot be the output", what);
  const HubPlan pl{hub_ids, chunk_ptr, static_cast<int>(H), static_cast<int>(T)};
  const HubWorkspace w = carve_hub_workspace(ws, T, F);
  const bool vec = rows_vectorise(x, F, ldx);
  dispatch_row_layout<LaunchHubAttend>(vec, vec ? (F + 3) / 4 : F, pl, grp_ptr, grp_perm, src, val, x, ldx, N, N_src, E,
                                       static_cast<int>(F), w.rec, stream);
  hipLaunchKernelGGL(hub_row_tail_kernel<HW_ATTEND>, dim3(static_cast<unsigned>(H)), dim3(64 * HW_TAIL_SLOTS), 0, stream,
                     pl, w.rec, nullptr, nullptr, w3, nullptr, N, static_cast<int>(F), out, nullptr, nullptr, p);
  return check_launch(what);
}

extern "C" int tgp_hubwalk_edge_dot_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* src,
                                        const int32_t* hub_ids, const int32_t* chunk_ptr, int64_t H, int64_t T,
                                        const float* g, const float* x, int64_t ldx, int64_t N, int64_t E, int64_t F,
                                        float* out, void* stream_) {
  const char* what = "tgp_hubwalk_edge_dot_f32";
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HUB_CHECK(what, grp_ptr, hub_ids, chunk_ptr, H, T, N, E, F, nullptr, 0, false);
  TGP_REQUIRE(ldx >= F, TGP_ERR_INVALID, "%s: bad size", what);
  if (E == 0) return TGP_OK;
  TGP_REQUIRE(src && out && (F == 0 || (g && x)), TGP_ERR_INVALID, "%s: null pointer", what);
  const HubPlan pl{hub_ids, chunk_ptr, static_cast<int>(H), static_cast<int>(T)};
  const bool vec = rows_vectorise(x, F, ldx) && F % 4 == 0 && reinterpret_cast<uintptr_t>(g) % 16 == 0;
  dispatch_row_layout<LaunchHubEdgeDot>(vec, vec ? (F + 3) / 4 : F, pl, grp_ptr, grp_perm, src, g, x, ldx, N, E,
                                        static_cast<int>(F), out, stream);
  return check_launch(what);
}

extern "C" int tgp_hubwalk_softmax_bwd_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* src,
                                           const int32_t* hub_ids, const int32_t* chunk_ptr, int64_t H, int64_t T,
                                           const float* alpha, const float* g_alpha, const float* sq, const float* sp,
                                           int64_t N, int64_t E, float negative_slope, float* g_l, float* g_sq, void* ws,
                                           size_t ws_bytes, void* stream_) {
  const char* what = "tgp_hubwalk_softmax_bwd_f32";
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HUB_CHECK(what, grp_ptr, hub_ids, chunk_ptr, H, T, N, E, 0, ws, ws_bytes, true);
  TGP_REQUIRE(sq && sp && g_sq && (E == 0 || (src && alpha && g_alpha && g_l)), TGP_ERR_INVALID, "%s: null pointer",
              what);
  TGP_REQUIRE((E == 0 || (g_l != alpha && g_l != g_alpha)) && g_sq != sq && g_sq != sp, TGP_ERR_INVALID,
              "%s: an input given as an output", what);
  const HubPlan pl{hub_ids, chunk_ptr, static_cast<int>(H), static_cast<int>(T)};
  float* rec_d = carve_hub_workspace(ws, T, 0).misc;
  float* rec_s = rec_d + T;
  hipLaunchKernelGGL(hub_softmax_bwd_chunk_kernel, dim3(cdiv(T, 4)), dim3(256), 0, stream, pl, grp_ptr, grp_perm, src,
                     alpha, g_alpha, N, E, rec_d);
  hipLaunchKernelGGL(hub_softmax_bwd_write_kernel, dim3(cdiv(T, 4)), dim3(256), 0, stream, pl, grp_ptr, grp_perm, src,
                     alpha, g_alpha, sq, sp, N, E, negative_slope, rec_d, rec_s, g_l);
  hipLaunchKernelGGL(hub_sum_tail_kernel, dim3(cdiv(H, 4)), dim3(256), 0, stream, pl, rec_s, N, g_sq);
  return check_launch(what);
}

extern "C" int tgp_hubwalk_query_bwd_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* dst,
                                         const int32_t* hub_ids, const int32_t* chunk_ptr, int64_t H, int64_t T,
                                         const int32_t* argpos, const float* g_sq, const float* w_tilde, int64_t N,
                                         int64_t E, int64_t F, float* out, void* ws, size_t ws_bytes, void* stream_) {
  const char* what = "tgp_hubwalk_query_bwd_f32";
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HUB_CHECK(what, grp_ptr, hub_ids, chunk_ptr, H, T, N, E, F, ws, ws_bytes, true);
  if (F == 0) return TGP_OK;
  TGP_REQUIRE(argpos && g_sq && w_tilde && out && (E == 0 || dst), TGP_ERR_INVALID, "%s: null pointer", what);
  const HubPlan pl{hub_ids, chunk_ptr, static_cast<int>(H), static_cast<int>(T)};
  const HubWorkspace w = carve_hub_workspace(ws, T, F);
  dispatch_row_layout<LaunchHubQueryBwd>(false, F, pl, grp_ptr, grp_perm, dst, argpos, g_sq, N, E, static_cast<int>(F),
                                         w.rec, stream);
  hipLaunchKernelGGL(hub_row_tail_kernel<HW_QUERY_BWD>, dim3(static_cast<unsigned>(H)), dim3(64 * HW_TAIL_SLOTS), 0,
                     stream, pl, w.rec, nullptr, nullptr, w_tilde, nullptr, N, static_cast<int>(F), out, nullptr, nullptr,
                     nullptr);
  return check_launch(what);
}
