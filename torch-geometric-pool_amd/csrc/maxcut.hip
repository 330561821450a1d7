// MaxCutPooling's three hot parts (reference select/maxcut_select.py, utils/ops.py:delta_gcn_matrix,
// utils/losses.py:maxcut_loss, utils/ops.py:propagate_assignments_sparse) on the memoised by-destination / by-source
// edge groups of SAG and ASAP.  The propagation matrix P = I - delta L_sym is never formed: one layer is
//   h'_i = act((1 - delta) [i < n_P] z_i + delta dinv_i sum_{r -> i, r != i} (w_e dinv_r) z_r + b),   z = h W^T
// with deg_r the summed weight of r's out-edges that are not self-loops, dinv = deg^-1/2 (inf -> 0), n_P = the list's
// largest endpoint + 1 (a device word: the host never waits for it).
//   maxcut_degree_kernel / maxcut_coef_kernel   dinv [N]; coef_e = w_e dinv[src_e], coef_t_e = w_e dinv[dst_e]  [E]
//   maxcut_layer_kernel<G>   one wave per node: G lanes share a z row (one channel each), the 64 / G slots take every
//                            (64 / G)-th edge of the group; the slots fold at offsets 32 .. G (wave_sum<64, G>); the
//                            finished row is projected by the next layer's weight (LDS, transposed) in channel order.
//                            The backward's g_z is the same kernel over the by-source group with coef_t, no bias, act 0.
//   maxcut_tail_kernel       Linear + act per mlp layer, the final Linear(., 1) and act: one wave per row, weights in LDS
//   maxcut_wgrad_*           out = a^T b as partial sums of fixed row chunks, then the chunks in ascending order
//   maxcut_cut_kernel        az_i = sum over i's group of w_e s[other_e], cut_i = s_i az_i, wsum_i = sum w_e (raw list)
//   maxcut_assign_kernel     one label-propagation round: an unlabelled node takes the label most of its labelled
//                            sources carry, duplicates counted, the lowest label on a tie
// No float atomics; every sum has one order, fixed by the group (a slot adds its edges in group order).  One wave walks
// a group whatever its length: there is no hub route.  A position outside [0, E) or an endpoint outside
// [0, N) is skipped and never dereferenced.
#include <math.h>

#include "common.h"

namespace tgp {
namespace {

constexpr int kMaxWidth = 64;        // widest row a layer or the tail takes
constexpr int kTailMaxParams = 8192;  // floats of the tail's packed parameters (LDS)
constexpr int kTailMaxLayers = 8;
constexpr int kWgradRows = 1024;  // rows per partial sum of the weight gradient
constexpr int kWgradTile = 16;

struct Group {
  int64_t b, e;
};

__device__ __forceinline__ Group group_of(const int32_t* __restrict__ grp_ptr, int64_t i, int64_t E) {
  int64_t b = grp_ptr[i], e = grp_ptr[i + 1];
  if (b < 0) b = 0;
  if (e > E) e = E;
  return {b, e};
}

// the other endpoint of group entry j, or -1 when the position or the endpoint is out of range
__device__ __forceinline__ int64_t endpoint_of(const int32_t* __restrict__ grp_perm, const int64_t* __restrict__ other,
                                                int64_t j, int64_t E, int64_t n, int64_t* pos_out) {
  const int64_t pos = grp_perm ? static_cast<int64_t>(grp_perm[j]) : j;
  *pos_out = pos;
  if (static_cast<uint64_t>(pos) >= static_cast<uint64_t>(E)) return -1;
  const int64_t r = other[pos];
  return static_cast<uint64_t>(r) < static_cast<uint64_t>(n) ? r : -1;
}

__device__ __forceinline__ float activate(float t, int act) {
  if (act == 1) return tanhf(t);
  if (act == 2) return t < 0.0f ? 0.0f : t;  // a NaN stays a NaN, as torch.relu keeps it
  return t;
}

// ---- degrees ------------------------------------------------------------------------------------------------------
// One wave per node over the by-source group: lane l adds entries l, l + 64, ..; the lanes fold at offsets 32 .. 1.
__global__ __launch_bounds__(256) void maxcut_degree_kernel(const int32_t* __restrict__ grp_ptr,
                                                            const int32_t* __restrict__ grp_perm,
                                                            const int64_t* __restrict__ dst,
                                                            const float* __restrict__ ew, int64_t n, int64_t E,
                                                            float* __restrict__ dinv) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (i >= n) return;  // wave-uniform
  const Group g = group_of(grp_ptr, i, E);
  float deg = 0.0f;
  for (int64_t e = g.b + lane; e < g.e; e += 64) {
    int64_t pos;
    const int64_t c = endpoint_of(grp_perm, dst, e, E, n, &pos);
    if (c < 0 || c == i) continue;
    deg = deg + (ew ? ew[pos] : 1.0f);
  }
  deg = wave_sum<64>(deg);
  if (lane == 0) {
    const float d = 1.0f / sqrtf(deg);  // a negative degree gives NaN, as pow(-0.5) does
    dinv[i] = (d == INFINITY) ? 0.0f : d;
  }
}

__global__ __launch_bounds__(256) void maxcut_coef_kernel(const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                          const float* __restrict__ ew, const float* __restrict__ dinv,
                                                          int64_t n, int64_t E, float* __restrict__ coef,
                                                          float* __restrict__ coef_t) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= E) return;
  const float w = ew ? ew[e] : 1.0f;
  const int64_t r = src[e], c = dst[e];
  if (coef) coef[e] = static_cast<uint64_t>(r) < static_cast<uint64_t>(n) ? w * dinv[r] : 0.0f;
  if (coef_t) coef_t[e] = static_cast<uint64_t>(c) < static_cast<uint64_t>(n) ? w * dinv[c] : 0.0f;
}

// ---- one layer ----------------------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(256) void maxcut_layer_kernel(const int32_t* __restrict__ grp_ptr,
                                                           const int32_t* __restrict__ grp_perm,
                                                           const int64_t* __restrict__ other,
                                                           const float* __restrict__ coef,
                                                           const float* __restrict__ dinv, const float* __restrict__ z,
                                                           const float* __restrict__ bias, int64_t n, int64_t E, int C,
                                                           const int64_t* __restrict__ n_p, float delta, int act,
                                                           float* __restrict__ h_out, const float* __restrict__ w_next,
                                                           int C_next, float* __restrict__ z_next) {
  constexpr int PER = 64 / G;
  __shared__ float wt[kMaxWidth * kMaxWidth];  // wt[c * C_next + o] = w_next[o * C + c]
  if (w_next) {
    for (int idx = threadIdx.x; idx < C * C_next; idx += 256) {
      const int o = idx / C, c = idx - o * C;
      wt[c * C_next + o] = w_next[idx];
    }
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, sub = lane % G, slot = lane / G, wave = threadIdx.x >> 6;
  const int64_t np = n_p ? n_p[0] : n;
  const float diag = 1.0f - delta;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 4 + wave; i < n; i += static_cast<int64_t>(gridDim.x) * 4) {
    const Group g = group_of(grp_ptr, i, E);
    float acc = 0.0f;
    bool any = false;
    if (sub < C) {
      for (int64_t e = g.b + slot; e < g.e; e += PER) {
        int64_t pos;
        const int64_t r = endpoint_of(grp_perm, other, e, E, n, &pos);
        if (r < 0 || r == i) continue;  // (a self-loop is not an edge of the Laplacian)
        any = true;
        acc = fmaf(coef[pos], z[r * C + sub], acc);
      }
    }
    acc = wave_sum<64, G>(acc);  // the slots: offsets 32 .. G
    // a node without an edge has no off-diagonal entry at all: a non-finite dinv_i must not reach it through 0 * NaN
    const bool has_edges = __ballot(any) != 0;
    float h = 0.0f;
    if (sub < C) {
      float t = has_edges ? (delta * dinv[i]) * acc : 0.0f;
      if (i < np) t = diag * z[i * C + sub] + t;
      if (bias) t = t + bias[sub];
      h = activate(t, act);
      if (h_out && slot == 0) h_out[i * C + sub] = h;
    }
    if (w_next) {  // lane o: <h, w_next[o, :]> in channel order; channel c sits in lane c (slot 0)
      float p = 0.0f;
      for (int c = 0; c < C; ++c) {
        const float hc = __shfl(h, c, 64);
        if (lane < C_next) p = fmaf(hc, wt[c * C_next + lane], p);
      }
      if (lane < C_next) z_next[i * C_next + lane] = p;
    }
  }
}

template <int G>
void launch_layer(int blocks, hipStream_t stream, const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* other,
                  const float* coef, const float* dinv, const float* z, const float* bias, int64_t n, int64_t E, int C,
                  const int64_t* n_p, float delta, int act, float* h_out, const float* w_next, int C_next,
                  float* z_next) {
  hipLaunchKernelGGL((maxcut_layer_kernel<G>), dim3(blocks), dim3(256), 0, stream, grp_ptr, grp_perm, other, coef, dinv,
                     z, bias, n, E, C, n_p, delta, act, h_out, w_next, C_next, z_next);
}

// ---- the row tail -------------------------------------------------------------------------------------------------
struct TailDims {
  int n_layers;                    // mlp layers (the final Linear(., 1) comes after them)
  int width[kTailMaxLayers + 1];  // width[0] = C, width[l + 1] = output width of mlp layer l
};

// params: per mlp layer W [out, in] then b [out]; then the final w [in] and b [1].  In LDS the matrices are transposed.
__global__ __launch_bounds__(256) void maxcut_tail_kernel(const float* __restrict__ h, int64_t n, TailDims d,
                                                          const float* __restrict__ params, int n_params, int mlp_act,
                                                          int act, float* __restrict__ score) {
  __shared__ float p[kTailMaxParams];
  {
    int off = 0;
    for (int l = 0; l < d.n_layers; ++l) {
      const int in = d.width[l], out = d.width[l + 1];
      for (int idx = threadIdx.x; idx < in * out; idx += 256) {
        const int o = idx / in, c = idx - o * in;
        p[off + c * out + o] = params[off + idx];
      }
      for (int idx = threadIdx.x; idx < out; idx += 256) p[off + in * out + idx] = params[off + in * out + idx];
      off += in * out + out;
    }
    for (int idx = threadIdx.x; off + idx < n_params; idx += 256) p[off + idx] = params[off + idx];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 4 + wave; i < n; i += static_cast<int64_t>(gridDim.x) * 4) {
    float v = lane < d.width[0] ? h[i * d.width[0] + lane] : 0.0f;
    int off = 0;
    for (int l = 0; l < d.n_layers; ++l) {
      const int in = d.width[l], out = d.width[l + 1];
      float a = 0.0f;
      for (int c = 0; c < in; ++c) {
        const float vc = __shfl(v, c, 64);
        if (lane < out) a = fmaf(vc, p[off + c * out + lane], a);
      }
      v = lane < out ? activate(a + p[off + in * out + lane], mlp_act) : 0.0f;
      off += in * out + out;
    }
    const int in = d.width[d.n_layers];
    float a = 0.0f;
    for (int c = 0; c < in; ++c) a = fmaf(__shfl(v, c, 64), p[off + c], a);
    if (lane == 0) score[i] = activate(a + p[off + in], act);
  }
}

// ---- weight gradient a^T b ----------------------------------------------------------------------------------------
// Block k adds rows [k * kWgradRows, (k + 1) * kWgradRows) in ascending order into part[k]; entry (p, q) belongs to one
// thread (up to 16 entries per thread at 64 x 64).
__global__ __launch_bounds__(256) void maxcut_wgrad_partial_kernel(const float* __restrict__ a,
                                                                   const float* __restrict__ b, int64_t n, int Ca, int Cb,
                                                                   float* __restrict__ part) {
  __shared__ float ta[kWgradTile][kMaxWidth], tb[kWgradTile][kMaxWidth];
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kWgradRows;
  int64_t r1 = r0 + kWgradRows;
  if (r1 > n) r1 = n;
  const int total = Ca * Cb;
  float acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0f;
  for (int64_t t0 = r0; t0 < r1; t0 += kWgradTile) {
    const int rows = static_cast<int>(r1 - t0 < kWgradTile ? r1 - t0 : kWgradTile);
    __syncthreads();
    for (int idx = threadIdx.x; idx < rows * Ca; idx += 256) ta[idx / Ca][idx % Ca] = a[t0 * Ca + idx];
    for (int idx = threadIdx.x; idx < rows * Cb; idx += 256) tb[idx / Cb][idx % Cb] = b[t0 * Cb + idx];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int idx = threadIdx.x + k * 256;
      if (idx < total) {
        const int pi = idx / Cb, qi = idx - pi * Cb;
        float s = acc[k];
        for (int r = 0; r < rows; ++r) s = fmaf(ta[r][pi], tb[r][qi], s);
        acc[k] = s;
      }
    }
  }
  float* out = part + static_cast<int64_t>(blockIdx.x) * total;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int idx = threadIdx.x + k * 256;
    if (idx < total) out[idx] = acc[k];
  }
}

__global__ __launch_bounds__(256) void maxcut_wgrad_fold_kernel(const float* __restrict__ part, int64_t chunks, int total,
                                                                float* __restrict__ out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  float s = 0.0f;
  for (int64_t k = 0; k < chunks; ++k) s = s + part[k * total + idx];
  out[idx] = s;
}

// ---- the cut loss's node terms -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void maxcut_cut_kernel(const int32_t* __restrict__ grp_ptr,
                                                         const int32_t* __restrict__ grp_perm,
                                                         const int64_t* __restrict__ other, const float* __restrict__ ew,
                                                         const float* __restrict__ s, int64_t n, int64_t E,
                                                         float* __restrict__ az, float* __restrict__ cut,
                                                         float* __restrict__ wsum) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (i >= n) return;
  const Group g = group_of(grp_ptr, i, E);
  float a = 0.0f, w = 0.0f;
  for (int64_t e = g.b + lane; e < g.e; e += 64) {
    int64_t pos;
    const int64_t c = endpoint_of(grp_perm, other, e, E, n, &pos);
    if (c < 0) continue;
    const float we = ew ? ew[pos] : 1.0f;
    a = fmaf(we, s[c], a);
    w = w + we;
  }
  a = wave_sum<64>(a);
  w = wave_sum<64>(w);
  if (lane == 0) {
    if (az) az[i] = a;
    if (cut) cut[i] = s[i] * a;
    if (wsum) wsum[i] = w;
  }
}

// ---- one round of the nearest-supernode assignment ---------------------------------------------------------------------
// Labels 1 .. K, 0 = none.  The distinct labels of the group are visited in ascending order: a walk counts the entries
// that carry `cur` and finds the smallest label above it; a strictly greater count replaces the best, so the lowest label
// wins a tie.  Reads only label_in (the labels of the round's start).
__global__ __launch_bounds__(256) void maxcut_assign_kernel(const int32_t* __restrict__ grp_ptr,
                                                            const int32_t* __restrict__ grp_perm,
                                                            const int64_t* __restrict__ src,
                                                            const int32_t* __restrict__ label_in, int64_t n, int64_t E,
                                                            int32_t* __restrict__ label_out) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (i >= n) return;
  const int32_t mine = label_in[i];
  if (mine > 0) {
    if (lane == 0) label_out[i] = mine;
    return;
  }
  const Group g = group_of(grp_ptr, i, E);
  int32_t cur = 0, best = 0, best_count = 0;
  while (true) {  // wave-uniform: cur, count and next are folded over the wave
    int32_t count = 0, next = INT32_MAX;
    for (int64_t e = g.b + lane; e < g.e; e += 64) {
      int64_t pos;
      const int64_t r = endpoint_of(grp_perm, src, e, E, n, &pos);
      if (r < 0) continue;
      const int32_t l = label_in[r];
      if (l == cur) ++count;
      if (l > cur && l < next) next = l;
    }
    count = wave_sum<64>(count);
    next = wave_min<64>(next);
    if (cur > 0 && count > best_count) {
      best = cur;
      best_count = count;
    }
    if (next == INT32_MAX) break;
    cur = next;
  }
  if (lane == 0) label_out[i] = best;
}

inline int check_index_sizes(const char* what, int64_t N, int64_t E) {
  TGP_REQUIRE(N >= 0 && E >= 0, TGP_ERR_INVALID, "%s: bad size", what);
  TGP_REQUIRE(N < (1ll << 31) && E <= INT32_MAX, TGP_ERR_RANGE, "%s: N=%lld or E=%lld beyond the int32 index", what,
              static_cast<long long>(N), static_cast<long long>(E));
  return TGP_OK;
}

inline int row_blocks(int64_t n) {  // four rows per workgroup, at most 8192 workgroups (the kernels stride over the rest)
  const int64_t b = (n + 3) / 4;
  return static_cast<int>(b < 8192 ? b : 8192);
}

inline int64_t wgrad_chunks(int64_t n) { return n > 0 ? (n + kWgradRows - 1) / kWgradRows : 1; }

}  // namespace
}  // namespace tgp

using namespace tgp;

extern "C" int tgp_maxcut_max_width(void) { return kMaxWidth; }
extern "C" int tgp_maxcut_tail_max_params(void) { return kTailMaxParams; }

extern "C" int tgp_maxcut_degree_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* src,
                                     const int64_t* dst, const float* edge_weight, int64_t N, int64_t E, float* dinv,
                                     float* coef, float* coef_t, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (int rc = check_index_sizes("tgp_maxcut_degree_f32", N, E)) return rc;
  if (N == 0) return TGP_OK;
  TGP_REQUIRE(grp_ptr && dinv && (E == 0 || (src && dst)), TGP_ERR_INVALID, "tgp_maxcut_degree_f32: null pointer");
  TGP_REQUIRE(dinv != edge_weight && (edge_weight == nullptr || (coef != edge_weight && coef_t != edge_weight)) &&
                  (coef == nullptr || coef != coef_t),
              TGP_ERR_INVALID, "tgp_maxcut_degree_f32: an input given as an output, or one buffer for both coefficients");
  hipLaunchKernelGGL(maxcut_degree_kernel, dim3(cdiv(N, 4)), dim3(256), 0, stream, grp_ptr, grp_perm, dst, edge_weight, N,
                     E, dinv);
  if (E > 0 && (coef || coef_t))
    hipLaunchKernelGGL(maxcut_coef_kernel, dim3(cdiv(E, 256)), dim3(256), 0, stream, src, dst, edge_weight, dinv, N, E,
                       coef, coef_t);
  return check_launch("tgp_maxcut_degree_f32");
}

extern "C" int tgp_maxcut_layer_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* other,
                                    const float* coef, const float* dinv, const float* z, const float* bias, int64_t N,
                                    int64_t E, int64_t C, const int64_t* n_p, float delta, int act, float* h_out,
                                    const float* w_next, int64_t C_next, float* z_next, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (int rc = check_index_sizes("tgp_maxcut_layer_f32", N, E)) return rc;
  TGP_REQUIRE(C >= 1 && C <= kMaxWidth && C_next >= 0 && C_next <= kMaxWidth, TGP_ERR_INVALID,
              "tgp_maxcut_layer_f32: widths must be 1 .. %d (C=%lld, C_next=%lld)", kMaxWidth, static_cast<long long>(C),
              static_cast<long long>(C_next));
  TGP_REQUIRE(act >= 0 && act <= 2, TGP_ERR_INVALID, "tgp_maxcut_layer_f32: act must be 0 (identity), 1 (tanh) or 2 (relu)");
  if (N == 0) return TGP_OK;
  TGP_REQUIRE(grp_ptr && dinv && z && (E == 0 || (other && coef)), TGP_ERR_INVALID, "tgp_maxcut_layer_f32: null pointer");
  TGP_REQUIRE((h_out || z_next) && ((w_next == nullptr) == (z_next == nullptr)) && (w_next == nullptr) == (C_next == 0),
              TGP_ERR_INVALID, "tgp_maxcut_layer_f32: no output, or the next weight without its width and output");
  TGP_REQUIRE(h_out != z && z_next != z, TGP_ERR_INVALID,
              "tgp_maxcut_layer_f32: z is read by other waves, it cannot be an output");
  const int c = static_cast<int>(C), cn = static_cast<int>(C_next), blocks = row_blocks(N);
#define TGP_MAXCUT_LAYER(G)                                                                                            \
  launch_layer<G>(blocks, stream, grp_ptr, grp_perm, other, coef, dinv, z, bias, N, E, c, n_p, delta, act, h_out, w_next, \
                  cn, z_next)
  if (c <= 1) TGP_MAXCUT_LAYER(1);
  else if (c <= 2) TGP_MAXCUT_LAYER(2);
  else if (c <= 4) TGP_MAXCUT_LAYER(4);
  else if (c <= 8) TGP_MAXCUT_LAYER(8);
  else if (c <= 16) TGP_MAXCUT_LAYER(16);
  else if (c <= 32) TGP_MAXCUT_LAYER(32);
  else TGP_MAXCUT_LAYER(64);
#undef TGP_MAXCUT_LAYER
  return check_launch("tgp_maxcut_layer_f32");
}

extern "C" int tgp_maxcut_tail_f32(const float* h, int64_t N, int64_t C, const int64_t* widths, int64_t n_layers,
                                   const float* params, int64_t n_params, int mlp_act, int act, float* score,
                                   void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(N >= 0 && C >= 1 && C <= kMaxWidth && n_layers >= 0 && n_layers <= kTailMaxLayers, TGP_ERR_INVALID,
              "tgp_maxcut_tail_f32: bad size (width 1 .. %d, at most %d mlp layers)", kMaxWidth, kTailMaxLayers);
  TGP_REQUIRE(N < (1ll << 31), TGP_ERR_RANGE, "tgp_maxcut_tail_f32: N beyond the int32 index");
  TGP_REQUIRE(mlp_act >= 0 && mlp_act <= 2 && act >= 0 && act <= 2, TGP_ERR_INVALID,
              "tgp_maxcut_tail_f32: activations must be 0 (identity), 1 (tanh) or 2 (relu)");
  TGP_REQUIRE(n_layers == 0 || widths, TGP_ERR_INVALID, "tgp_maxcut_tail_f32: null pointer");
  TailDims d;
  d.n_layers = static_cast<int>(n_layers);
  d.width[0] = static_cast<int>(C);
  int64_t need = 0, in = C;
  for (int l = 0; l < d.n_layers; ++l) {
    TGP_REQUIRE(widths[l] >= 1 && widths[l] <= kMaxWidth, TGP_ERR_INVALID,
                "tgp_maxcut_tail_f32: mlp width %lld outside 1 .. %d", static_cast<long long>(widths[l]), kMaxWidth);
    d.width[l + 1] = static_cast<int>(widths[l]);
    need += in * widths[l] + widths[l];
    in = widths[l];
  }
  need += in + 1;
  TGP_REQUIRE(n_params == need && need <= kTailMaxParams, TGP_ERR_INVALID,
              "tgp_maxcut_tail_f32: %lld packed parameters given, the widths need %lld (at most %d)",
              static_cast<long long>(n_params), static_cast<long long>(need), kTailMaxParams);
  if (N == 0) return TGP_OK;
  TGP_REQUIRE(h && params && score && score != h, TGP_ERR_INVALID,
              "tgp_maxcut_tail_f32: null pointer, or h given as the output");
  hipLaunchKernelGGL(maxcut_tail_kernel, dim3(row_blocks(N)), dim3(256), 0, stream, h, N, d, params,
                     static_cast<int>(n_params), mlp_act, act, score);
  return check_launch("tgp_maxcut_tail_f32");
}

extern "C" size_t tgp_maxcut_wgrad_workspace_bytes(int64_t N, int64_t Ca, int64_t Cb) {
  if (N < 0 || Ca < 1 || Cb < 1 || Ca > kMaxWidth || Cb > kMaxWidth) return 0;
  return align_up(static_cast<size_t>(wgrad_chunks(N)) * Ca * Cb * sizeof(float));
}

extern "C" int tgp_maxcut_wgrad_f32(const float* a, const float* b, int64_t N, int64_t Ca, int64_t Cb, float* out, void* ws,
                                    size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(N >= 0 && Ca >= 1 && Cb >= 1 && Ca <= kMaxWidth && Cb <= kMaxWidth, TGP_ERR_INVALID,
              "tgp_maxcut_wgrad_f32: bad size (widths 1 .. %d)", kMaxWidth);
  TGP_REQUIRE(N < (1ll << 31), TGP_ERR_RANGE, "tgp_maxcut_wgrad_f32: N beyond the int32 index");
  TGP_REQUIRE(out && ws && (N == 0 || (a && b)), TGP_ERR_INVALID, "tgp_maxcut_wgrad_f32: null pointer");
  TGP_REQUIRE(ws_bytes >= tgp_maxcut_wgrad_workspace_bytes(N, Ca, Cb), TGP_ERR_WORKSPACE,
              "tgp_maxcut_wgrad_f32: workspace too small");
  const int64_t chunks = wgrad_chunks(N);
  const int total = static_cast<int>(Ca * Cb);
  hipLaunchKernelGGL(maxcut_wgrad_partial_kernel, dim3(static_cast<unsigned>(chunks)), dim3(256), 0, stream, a, b, N,
                     static_cast<int>(Ca), static_cast<int>(Cb), static_cast<float*>(ws));
  hipLaunchKernelGGL(maxcut_wgrad_fold_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, static_cast<const float*>(ws),
                     chunks, total, out);
  return check_launch("tgp_maxcut_wgrad_f32");
}

extern "C" int tgp_maxcut_cut_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* other,
                                  const float* edge_weight, const float* s, int64_t N, int64_t E, float* az, float* cut,
                                  float* wsum, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (int rc = check_index_sizes("tgp_maxcut_cut_f32", N, E)) return rc;
  if (N == 0) return TGP_OK;
  TGP_REQUIRE(grp_ptr && s && (az || cut || wsum) && (E == 0 || other), TGP_ERR_INVALID,
              "tgp_maxcut_cut_f32: null pointer");
  TGP_REQUIRE(az != s && cut != s && wsum != s, TGP_ERR_INVALID,
              "tgp_maxcut_cut_f32: s is read by other waves, it cannot be an output");
  hipLaunchKernelGGL(maxcut_cut_kernel, dim3(cdiv(N, 4)), dim3(256), 0, stream, grp_ptr, grp_perm, other, edge_weight, s,
                     N, E, az, cut, wsum);
  return check_launch("tgp_maxcut_cut_f32");
}

extern "C" int tgp_maxcut_assign_round_i32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* src,
                                           const int32_t* label_in, int64_t N, int64_t E, int32_t* label_out,
                                           void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (int rc = check_index_sizes("tgp_maxcut_assign_round_i32", N, E)) return rc;
  if (N == 0) return TGP_OK;
  TGP_REQUIRE(grp_ptr && label_in && label_out && (E == 0 || src), TGP_ERR_INVALID,
              "tgp_maxcut_assign_round_i32: null pointer");
  TGP_REQUIRE(label_in != label_out, TGP_ERR_INVALID,
              "tgp_maxcut_assign_round_i32: a round reads the labels of its start, they cannot be the output");
  hipLaunchKernelGGL(maxcut_assign_kernel, dim3(cdiv(N, 4)), dim3(256), 0, stream, grp_ptr, grp_perm, src, label_in, N, E,
                     label_out);
  return check_launch("tgp_maxcut_assign_round_i32");
}
