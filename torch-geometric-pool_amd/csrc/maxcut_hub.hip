// The hub route of MaxCutPooling's two long walks (maxcut.hip: maxcut_layer_kernel, maxcut_assign_kernel).  A group the
// host plan names as a hub (hub_plan.h) is cut into chunks of HW_CHUNK entries and ONE WAVE OWNS ONE (hub, chunk); the
// one-wave kernels run on the light index first (every hub group emptied) and these entries overwrite the hub nodes' outputs.
//   layer, chunk   the wave loads its chunk's positions, endpoints and coefficients coalesced (HW_CHUNK / 64 entries per
//                  lane) and parks (endpoint or -1, coef) in LDS, 2 KB per wave: the dependent chain perm -> other -> coef
//                  is off the gather path.  Then the layer kernel's lane layout: G lanes share a z row, the 64 / G slots
//                  stride the chunk's entries; a slot issues kAhead row loads before it adds them, in entry order, into ONE
//                  accumulator; the slots fold at offsets 32 .. G (wave_sum<64, G>).  Slot 0 leaves the partial row [C] and
//                  "any valid entry that is no self-loop" in the chunk's record.
//   layer, tail    one workgroup of HW_TAIL_SLOTS x 64 per hub: slot s folds records s, s + 16, .. of a column in
//                  ascending order, LDS hands the sixteen partials to slot 0, which folds them in slot order and ORs the
//                  flags; then maxcut_row.h's epilogue (the text the one-wave kernel runs) writes h and z_next.
//   assign, chunk  an unlabelled hub: the wave reads its chunk's source labels, folds equal labels with a leader loop over
//                  ballots and adds the counts to the hub's row of K + 1 int32 counts with integer atomicAdd (exact in
//                  any order).  Label 0, labels outside 1 .. K and invalid entries count nothing.
//   assign, tail   one workgroup per hub: a labelled hub keeps its label; else every thread scans its strided share of
//                  labels 1 .. K (a strictly greater count replaces, so the lowest label wins a tie), the threads fold by
//                  (higher count, else lower label), and the counts that were read are zeroed for the next round.
// No float atomics and one order per sum: the bits repeat and depend on the group alone.  A position outside [0, E) or
// an endpoint outside [0, N) is skipped and never dereferenced; a record index is clamped to the workspace the plan sized.
#include <math.h>

#include "common.h"
#include "hub_plan.h"
#include "maxcut_row.h"

namespace tgp {
namespace {

constexpr int kPerLane = HW_CHUNK / 64;  // entries a lane loads and parks
constexpr int kAhead = 8;                // row loads a slot has in flight before it adds them
constexpr int kTailThreads = 64 * HW_TAIL_SLOTS;

// ---- the layer ------------------------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(256) void mchub_layer_chunk_kernel(HubPlan pl, const int32_t* __restrict__ grp_ptr,
                                                                const int32_t* __restrict__ grp_perm,
                                                                const int64_t* __restrict__ other,
                                                                const float* __restrict__ coef,
                                                                const float* __restrict__ z, int64_t n, int64_t E, int C,
                                                                float* __restrict__ rec, int32_t* __restrict__ any_rec) {
  constexpr int PER = 64 / G;
  __shared__ int32_t park_r[4][HW_CHUNK];  // the endpoint's row, -1: skip (out of range or a self-loop)
  __shared__ float park_c[4][HW_CHUNK];
  const int lane = threadIdx.x & 63, sub = lane % G, slot = lane / G, wave = threadIdx.x >> 6;
  const int64_t w = static_cast<int64_t>(blockIdx.x) * 4 + wave;
  HubItem it;
  const bool live = w < pl.T && hub_item(pl, grp_ptr, w, n, E, &it);  // wave-uniform; every wave reaches the barrier
  const int cnt = live ? static_cast<int>(it.e - it.b) : 0;
  bool valid = false;
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    const int j = k * 64 + lane;
    int32_t r = -1;
    float cf = 0.0f;
    if (j < cnt) {
      int64_t pos;
      const int64_t rr = endpoint_of(grp_perm, other, it.b + j, E, n, &pos);
      if (rr >= 0 && rr != it.node) {  // (a self-loop is not an edge of the Laplacian)
        r = static_cast<int32_t>(rr);
        cf = coef[pos];
      }
    }
    park_r[wave][j] = r;
    park_c[wave][j] = cf;
    valid = valid || r >= 0;
  }
  const bool any = __ballot(valid) != 0;
  __syncthreads();
  float acc = 0.0f;
  if (sub < C) {
    for (int j0 = slot; j0 < cnt; j0 += PER * kAhead) {
      int32_t r[kAhead];
      float cf[kAhead], v[kAhead];
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const int j = j0 + u * PER;
        r[u] = j < cnt ? park_r[wave][j] : -1;
        cf[u] = j < cnt ? park_c[wave][j] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < kAhead; ++u) v[u] = r[u] >= 0 ? z[static_cast<int64_t>(r[u]) * C + sub] : 0.0f;
#pragma unroll
      for (int u = 0; u < kAhead; ++u)
        if (r[u] >= 0) acc = fmaf(cf[u], v[u], acc);
    }
  }
  acc = wave_sum<64, G>(acc);  // the slots: offsets 32 .. G
  if (w >= pl.T) return;
  if (slot == 0 && sub < C) rec[w * C + sub] = acc;
  if (lane == 0) any_rec[w] = any ? 1 : 0;
}

__global__ __launch_bounds__(kTailThreads) void mchub_layer_tail_kernel(
    HubPlan pl, const float* __restrict__ rec, const int32_t* __restrict__ any_rec, const float* __restrict__ dinv,
    const float* __restrict__ z, const float* __restrict__ bias, int64_t n, int C, const int64_t* __restrict__ n_p,
    float delta, int act, float* __restrict__ h_out, const float* __restrict__ w_next, int C_next,
    float* __restrict__ z_next) {
  __shared__ float wt[kMaxWidth * kMaxWidth];  // wt[c * C_next + o] = w_next[o * C + c]
  __shared__ float sh_v[HW_TAIL_SLOTS][64];
  __shared__ int32_t sh_any[HW_TAIL_SLOTS];
  const int col = threadIdx.x & 63, slot = threadIdx.x >> 6;
  HubItem it;
  if (!hub_of(pl, static_cast<int>(blockIdx.x), n, &it)) return;  // uniform over the workgroup
  stage_next_weight<kTailThreads>(wt, w_next, C, C_next);
  float v = 0.0f;
  int32_t a = 0;
  for (int ch = slot; ch < it.count; ch += HW_TAIL_SLOTS) {
    if (col < C) v = v + rec[static_cast<int64_t>(it.first + ch) * C + col];
    a |= any_rec[it.first + ch];
  }
  sh_v[slot][col] = v;
  if (col == 0) sh_any[slot] = a;
  __syncthreads();
  if (slot != 0) return;
  for (int s = 1; s < HW_TAIL_SLOTS; ++s) {
    v = v + sh_v[s][col];
    a |= sh_any[s];
  }
  const LayerRow row{dinv, z, bias, C, n_p ? n_p[0] : n, delta, act, h_out, w_next ? wt : nullptr, C_next, z_next};
  finish_layer_row(row, it.node, v, a != 0, col, col, 0);
}

template <int G>
void launch_layer_chunks(HubPlan pl, hipStream_t stream, const int32_t* grp_ptr, const int32_t* grp_perm,
                         const int64_t* other, const float* coef, const float* z, int64_t n, int64_t E, int C, float* rec,
                         int32_t* any_rec) {
  hipLaunchKernelGGL((mchub_layer_chunk_kernel<G>), dim3(cdiv(pl.T, 4)), dim3(256), 0, stream, pl, grp_ptr, grp_perm,
                     other, coef, z, n, E, C, rec, any_rec);
}

// ---- one assignment round ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mchub_assign_chunk_kernel(HubPlan pl, const int32_t* __restrict__ grp_ptr,
                                                                 const int32_t* __restrict__ grp_perm,
                                                                 const int64_t* __restrict__ src,
                                                                 const int32_t* __restrict__ label_in, int64_t n,
                                                                 int64_t E, int K, int32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (w >= pl.T) return;  // wave-uniform, as the two below
  HubItem it;
  if (!hub_item(pl, grp_ptr, w, n, E, &it)) return;
  if (label_in[it.node] > 0) return;
  int32_t* cnt = counts + static_cast<int64_t>(it.hub) * (static_cast<int64_t>(K) + 1);
  for (int64_t e0 = it.b; e0 < it.e; e0 += 64) {  // every lane takes part in every ballot
    const int64_t e = e0 + lane;
    int32_t l = 0;
    if (e < it.e) {
      int64_t pos;
      const int64_t r = endpoint_of(grp_perm, src, e, E, n, &pos);
      if (r >= 0) l = label_in[r];
      if (l < 0 || l > K) l = 0;
    }
    unsigned long long todo = __ballot(l > 0);
    while (todo) {  // one atomic per distinct label of the 64 entries
      const int leader = __ffsll(todo) - 1;
      const int32_t ll = __shfl(l, leader, 64);
      const unsigned long long same = __ballot(l == ll);
      if (lane == leader) atomicAdd(&cnt[ll], __popcll(same));
      todo &= ~same;
    }
  }
}

// key of (count, label): a higher count is larger, at equal counts the LOWER label is
__device__ __forceinline__ unsigned long long vote_key(int32_t count, int32_t label) {
  return (static_cast<unsigned long long>(static_cast<uint32_t>(count)) << 32) | (0xFFFFFFFFu - static_cast<uint32_t>(label));
}

__global__ __launch_bounds__(kTailThreads) void mchub_assign_tail_kernel(HubPlan pl, const int32_t* __restrict__ label_in,
                                                                         int64_t n, int K, int32_t* __restrict__ counts,
                                                                         int32_t* __restrict__ label_out) {
  __shared__ unsigned long long sh[HW_TAIL_SLOTS];
  HubItem it;
  if (!hub_of(pl, static_cast<int>(blockIdx.x), n, &it)) return;  // uniform over the workgroup
  const int32_t mine = label_in[it.node];
  if (mine > 0) {  // (its chunks counted nothing)
    if (threadIdx.x == 0) label_out[it.node] = mine;
    return;
  }
  int32_t* cnt = counts + static_cast<int64_t>(blockIdx.x) * (static_cast<int64_t>(K) + 1);
  unsigned long long best = 0;  // count 0: no label
  for (int64_t l = 1 + threadIdx.x; l <= K; l += kTailThreads) {  // ascending: strictly greater replaces
    const int32_t c = cnt[l];
    if (c > 0) {
      cnt[l] = 0;  // for the next round
      const unsigned long long key = vote_key(c, static_cast<int32_t>(l));
      if (key > best) best = key;
    }
  }
  best = wave_fold<64>(best, op_max{});
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int s = 1; s < HW_TAIL_SLOTS; ++s)
    if (sh[s] > best) best = sh[s];
  label_out[it.node] = (best >> 32) ? static_cast<int32_t>(0xFFFFFFFFu - static_cast<uint32_t>(best)) : 0;
}

// ---- host -------------------------------------------------------------------------------------------------------------
// the layer's workspace: float rec [T, C] | int32 any [T]
inline size_t layer_workspace_bytes(int64_t T, int64_t C) {
  return align_up(static_cast<size_t>(T) * static_cast<size_t>(C) * 4) + align_up(static_cast<size_t>(T) * 4);
}

inline size_t assign_workspace_bytes(int64_t H, int64_t K) {
  return align_up(static_cast<size_t>(H) * (static_cast<size_t>(K) + 1) * 4);
}

// 1: nothing to do (an empty plan or no node); 0: go on; below zero: refused.  `size` is the entry's own size argument
// (C or K), `need` the workspace it asks for.
inline int check_mchub_call(const char* what, const int32_t* grp_ptr, const int32_t* hub_ids, const int32_t* chunk_ptr,
                            int64_t H, int64_t T, int64_t N, int64_t E, int64_t size, const void* ws, size_t ws_bytes,
                            size_t (*need)(int64_t, int64_t), int64_t need_rows) {
  if (int rc = check_index_sizes(what, N, E)) return rc;
  TGP_REQUIRE(H >= 0 && T >= 0 && size >= 0, TGP_ERR_INVALID, "%s: bad size", what);
  TGP_REQUIRE(H <= INT32_MAX && T <= INT32_MAX && size < INT32_MAX, TGP_ERR_RANGE, "%s: H, T, C or K beyond int32", what);
  if (N == 0 || H == 0 || T == 0) return 1;
  TGP_REQUIRE(grp_ptr && hub_ids && chunk_ptr, TGP_ERR_INVALID, "%s: null index or plan pointer", what);
  TGP_REQUIRE(ws && reinterpret_cast<uintptr_t>(ws) % 16 == 0, TGP_ERR_INVALID, "%s: no (16-byte aligned) workspace", what);
  TGP_REQUIRE(ws_bytes >= need(need_rows, size), TGP_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", what, ws_bytes,
              need(need_rows, size));
  return 0;
}

#define MCHUB_CHECK(...)                          \
  do {                                            \
    const int rc_ = check_mchub_call(__VA_ARGS__); \
    if (rc_ != 0) return rc_ < 0 ? rc_ : TGP_OK;   \
  } while (0)

}  // namespace
}  // namespace tgp

using namespace tgp;

extern "C" size_t tgp_mchub_workspace_bytes(int64_t T, int64_t C) {
  if (T <= 0 || C < 1 || C > kMaxWidth) return 0;
  return layer_workspace_bytes(T, C);
}

extern "C" size_t tgp_mchub_assign_workspace_bytes(int64_t H, int64_t K) {
  if (H <= 0 || K < 0 || K >= INT32_MAX) return 0;
  return assign_workspace_bytes(H, K);
}

extern "C" int tgp_mchub_layer_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* other,
                                   const int32_t* hub_ids, const int32_t* chunk_ptr, int64_t H, int64_t T,
                                   const float* coef, const float* dinv, const float* z, const float* bias, int64_t N,
                                   int64_t E, int64_t C, const int64_t* n_p, float delta, int act, float* h_out,
                                   const float* w_next, int64_t C_next, float* z_next, void* ws, size_t ws_bytes,
                                   void* stream_) {
  const char* what = "tgp_mchub_layer_f32";
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  MCHUB_CHECK(what, grp_ptr, hub_ids, chunk_ptr, H, T, N, E, C, ws, ws_bytes, layer_workspace_bytes, T);
  TGP_REQUIRE(C >= 1 && C <= kMaxWidth && C_next >= 0 && C_next <= kMaxWidth, TGP_ERR_INVALID,
              "%s: widths must be 1 .. %d (C=%lld, C_next=%lld)", what, kMaxWidth, static_cast<long long>(C),
              static_cast<long long>(C_next));
  TGP_REQUIRE(act >= 0 && act <= 2, TGP_ERR_INVALID, "%s: act must be 0 (identity), 1 (tanh) or 2 (relu)", what);
  TGP_REQUIRE(dinv && z && (E == 0 || (other && coef)), TGP_ERR_INVALID, "%s: null pointer", what);
  TGP_REQUIRE((h_out || z_next) && ((w_next == nullptr) == (z_next == nullptr)) && (w_next == nullptr) == (C_next == 0),
              TGP_ERR_INVALID, "%s: no output, or the next weight without its width and output", what);
  TGP_REQUIRE(h_out != z && z_next != z, TGP_ERR_INVALID, "%s: z is read by other waves, it cannot be an output", what);
  const HubPlan pl{hub_ids, chunk_ptr, static_cast<int>(H), static_cast<int>(T)};
  const int c = static_cast<int>(C);
  float* rec = static_cast<float*>(ws);
  int32_t* any_rec = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + align_up(static_cast<size_t>(T) * C * 4));
#define TGP_MCHUB_LAYER(G) launch_layer_chunks<G>(pl, stream, grp_ptr, grp_perm, other, coef, z, N, E, c, rec, any_rec)
  if (c <= 1) TGP_MCHUB_LAYER(1);
  else if (c <= 2) TGP_MCHUB_LAYER(2);
  else if (c <= 4) TGP_MCHUB_LAYER(4);
  else if (c <= 8) TGP_MCHUB_LAYER(8);
  else if (c <= 16) TGP_MCHUB_LAYER(16);
  else if (c <= 32) TGP_MCHUB_LAYER(32);
  else TGP_MCHUB_LAYER(64);
#undef TGP_MCHUB_LAYER
  hipLaunchKernelGGL(mchub_layer_tail_kernel, dim3(static_cast<unsigned>(H)), dim3(kTailThreads), 0, stream, pl, rec,
                     any_rec, dinv, z, bias, N, c, n_p, delta, act, h_out, w_next, static_cast<int>(C_next), z_next);
  return check_launch(what);
}

extern "C" int tgp_mchub_assign_round_i32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* src,
                                          const int32_t* hub_ids, const int32_t* chunk_ptr, int64_t H, int64_t T,
                                          const int32_t* label_in, int64_t N, int64_t E, int64_t K, int32_t* label_out,
                                          void* ws, size_t ws_bytes, void* stream_) {
  const char* what = "tgp_mchub_assign_round_i32";
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  MCHUB_CHECK(what, grp_ptr, hub_ids, chunk_ptr, H, T, N, E, K, ws, ws_bytes, assign_workspace_bytes, H);
  TGP_REQUIRE(label_in && label_out && (E == 0 || src), TGP_ERR_INVALID, "%s: null pointer", what);
  TGP_REQUIRE(label_in != label_out, TGP_ERR_INVALID,
              "%s: a round reads the labels of its start, they cannot be the output", what);
  const HubPlan pl{hub_ids, chunk_ptr, static_cast<int>(H), static_cast<int>(T)};
  int32_t* counts = static_cast<int32_t*>(ws);
  hipLaunchKernelGGL(mchub_assign_chunk_kernel, dim3(cdiv(T, 4)), dim3(256), 0, stream, pl, grp_ptr, grp_perm, src,
                     label_in, N, E, static_cast<int>(K), counts);
  hipLaunchKernelGGL(mchub_assign_tail_kernel, dim3(static_cast<unsigned>(H)), dim3(kTailThreads), 0, stream, pl, label_in,
                     N, static_cast<int>(K), counts, label_out);
  return check_launch(what);
}
