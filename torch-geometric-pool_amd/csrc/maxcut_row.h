// What the one-wave delta-GCN layer (maxcut.hip) and its hub route (maxcut_hub.hip) share: the walk's group and endpoint
// (edge_walk.h), the activation, the next weight in LDS, and the row epilogue -- ONE text of it, so a hub's row is
// finished exactly as every other row is:
//   t = has_edges ? (delta dinv_i) acc : 0;  i < n_P: t = (1 - delta) z_i + t;  t += b;  h = act(t);
//   z_next_i[o] = the fmaf chain of h[c] w_next[o, c] over ascending c.
#pragma once

#include <math.h>

#include "common.h"
#include "edge_walk.h"  // Group, group_of, source_of, check_index_sizes

namespace tgp {
namespace {

constexpr int kMaxWidth = 64;  // widest row a layer or the tail takes

// the other endpoint of group entry j, or -1 when the position or the endpoint is out of range
__device__ __forceinline__ int64_t endpoint_of(const int32_t* __restrict__ grp_perm, const int64_t* __restrict__ other,
                                                int64_t j, int64_t E, int64_t n, int64_t* pos_out) {
  return source_of(grp_perm, other, j, E, n, pos_out);
}

__device__ __forceinline__ float activate(float t, int act) {
  if (act == 1) return tanhf(t);
  if (act == 2) return t < 0.0f ? 0.0f : t;  // a NaN stays a NaN, as torch.relu keeps it
  return t;
}

// wt[c * C_next + o] = w_next[o * C + c] (wt: kMaxWidth * kMaxWidth floats of LDS), by every thread of the workgroup
template <int THREADS>
__device__ __forceinline__ void stage_next_weight(float* wt, const float* __restrict__ w_next, int C, int C_next) {
  if (w_next) {
    for (int idx = threadIdx.x; idx < C * C_next; idx += THREADS) {
      const int o = idx / C, c = idx - o * C;
      wt[c * C_next + o] = w_next[idx];
    }
    __syncthreads();
  }
}

struct LayerRow {
  const float* dinv;
  const float* z;
  const float* bias;  // NULL: none
  int C;
  int64_t np;  // n_P
  float delta;
  int act;
  float* h_out;     // NULL: not written
  const float* wt;  // the next weight in LDS (stage_next_weight), NULL: no projection
  int C_next;
  float* z_next;
};

// Row i from its summed off-diagonal term: called by all 64 lanes of one wave; lane `lane` holds channel `sub`'s sum in
// `acc`, the lanes of slot 0 (lane == sub) write.  has_edges: the group has a valid entry that is no self-loop -- a node
// without one has no off-diagonal entry at all, so a non-finite dinv_i must not reach it through 0 * NaN.
__device__ __forceinline__ void finish_layer_row(const LayerRow& r, int64_t i, float acc, bool has_edges, int lane,
                                                 int sub, int slot) {
  const float diag = 1.0f - r.delta;
  float h = 0.0f;
  if (sub < r.C) {
    float t = has_edges ? (r.delta * r.dinv[i]) * acc : 0.0f;
    if (i < r.np) t = diag * r.z[i * r.C + sub] + t;
    if (r.bias) t = t + r.bias[sub];
    h = activate(t, r.act);
    if (r.h_out && slot == 0) r.h_out[i * r.C + sub] = h;
  }
  if (r.wt) {  // lane o: <h, w_next[o, :]> in channel order; channel c sits in lane c (slot 0)
    float p = 0.0f;
    for (int c = 0; c < r.C; ++c) {
      const float hc = __shfl(h, c, 64);
      if (lane < r.C_next) p = fmaf(hc, r.wt[c * r.C_next + lane], p);
    }
    if (lane < r.C_next) r.z_next[i * r.C_next + lane] = p;
  }
}

}  // namespace
}  // namespace tgp
