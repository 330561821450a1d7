// The wave and block reductions of the library, each order written down once.  Templates and inline device functions
// only: nothing lands in a code object that does not use it.
//
// The order of the additions is part of a kernel's contract (no float atomics: a loss is reproducible because its sum
// is taken in one fixed order), so a caller names the order it means and must not swap one for another:
//   wave_fold<G>        xor butterfly at offsets G/2 .. 1 inside every G-lane group, the result in every lane
//   wave_butterfly<G>   the same loop for several values (and ops) at once: one iteration advances all of them
//   wave_incl_scan<W>   shuffle-up inclusive scan at distances 1 .. W/2
//   dpp_row_fold        DPP row_ror 1, 2, 4, 8 inside the 16-lane rows; wave_half_fold adds one swizzle across the two
//                       rows of a half-wave, wave_sum_rows adds the four row sums as (r0 + r16) + (r32 + r48)
//   block_fold_seq      wave fold, one value per wave in LDS, then t = 0, t = op(t, sh[w]) for w = 0 .. T/64 - 1
//   block_fold_pair256  wave fold, then the four waves of a 256-thread workgroup as (sh0 op sh1) op (sh2 op sh3)
// The float results of two of these differ in the last bits.  Bit-equality between routes is asserted for the dense
// losses (the fused tail against the stand-alone kernels, losses.hip / dmon.hip / hosc.hip / just_balance.hip over
// block_fold_seq), for AsymCheegerCut's dense and sparse routes (block_fold_pair256), for the rows route against the
// padded one (dense.hip, dense_post.h) and for the NDP selector's one-wave and workgroup kernels (wave_sum_rows).
// A ladder of another order with a single user stays inline at its site, with a comment that names the order.  So does a
// ladder of one of these orders where a call in its place made the compiler schedule the kernel around it differently
// (this header was introduced without changing any kernel's instruction stream); its comment names the function it is.
#pragma once
#include <type_traits>

#include "common.h"

namespace tgp {

// ---- the ops ------------------------------------------------------------------------------------------------------
struct op_add {
  template <typename T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct op_fadd_rn {  // an addition the compiler may not contract or reassociate
  __device__ __forceinline__ float operator()(float a, float b) const { return __fadd_rn(a, b); }
};
struct op_or {
  template <typename T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a | b; }
};
struct op_max {  // floats: fmaxf / fmax (a NaN loses: see op_nanmax); integers: the later value only where it is larger
  __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
  __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); }
  template <typename T>
  __device__ __forceinline__ T operator()(T a, T b) const { return b > a ? b : a; }
};
struct op_min {
  template <typename T>
  __device__ __forceinline__ T operator()(T a, T b) const { return b < a ? b : a; }
};

// ---- the reference's NaN rule -------------------------------------------------------------------------------------
// torch's max / amax / amin / clamp propagate a NaN; fmaxf / fminf return the other operand.  Wherever the reference
// takes one of those over values a caller supplies, the kernels use these: a NaN operand is the result.  (IEEE 754-2019
// maximum / minimum: v_maximum3_f32 / v_minimum3_f32 on gfx950, one instruction like v_max_f32; fp64 gets v_max_f64
// and a select.)
template <typename T>
__device__ __forceinline__ T nan_max(T a, T b) { return __builtin_elementwise_maximum(a, b); }
template <typename T>
__device__ __forceinline__ T nan_min(T a, T b) { return __builtin_elementwise_minimum(a, b); }
// Tensor.clamp(min=lo): a NaN falls through
template <typename T>
__device__ __forceinline__ T clamp_min(T d, T lo) { return d < lo ? lo : d; }
struct op_nanmax {
  template <typename T>
  __device__ __forceinline__ T operator()(T a, T b) const { return nan_max(a, b); }
};
struct op_nanmin {
  template <typename T>
  __device__ __forceinline__ T operator()(T a, T b) const { return nan_min(a, b); }
};

// ---- xor butterfly ------------------------------------------------------------------------------------------------
// step(peer) runs once per offset G/2, .., 1; peer(x) is x of lane (lane ^ offset).  Several values advanced in one
// step share the loop iteration (three separate folds would be three loops, which may schedule differently).
template <int G = 64, typename Step>
__device__ __forceinline__ void wave_butterfly(Step step) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) step([o](auto x) { return __shfl_xor(x, o, 64); });
}

// LO > 1 stops the ladder after offset LO: a fold over the G / LO lanes that are LO apart (<64, 32>: the two half-waves)
template <int G = 64, int LO = 1, typename T, typename Op>
__device__ __forceinline__ T wave_fold(T v, Op op) {
#pragma unroll
  for (int o = G / 2; o >= LO; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  return v;
}
template <int G = 64, int LO = 1, typename T>
__device__ __forceinline__ T wave_sum(T v) { return wave_fold<G, LO>(v, op_add{}); }
template <int G = 64, typename T>
__device__ __forceinline__ T wave_max(T v) { return wave_fold<G>(v, op_max{}); }
template <int G = 64, typename T>
__device__ __forceinline__ T wave_min(T v) { return wave_fold<G>(v, op_min{}); }
template <int G = 64, typename T>
__device__ __forceinline__ T wave_nanmax(T v) { return wave_fold<G>(v, op_nanmax{}); }  // a NaN in any lane wins
template <int G = 64, typename T>
__device__ __forceinline__ T wave_nanmin(T v) { return wave_fold<G>(v, op_nanmin{}); }
template <int G = 64, typename T>
__device__ __forceinline__ T wave_or(T v) { return wave_fold<G>(v, op_or{}); }

// ---- inclusive scan over every W-lane group (shuffle up at distances 1, 2, .., W/2) -----------------------------------
template <int W = 64, typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
#pragma unroll
  for (int d = 1; d < W; d <<= 1) {
    const T t = __shfl_up(v, d, W);
    if ((lane_id() & (W - 1)) >= d) v += t;
  }
  return v;
}

// ---- DPP moves, lane reads and the row ladder ---------------------------------------------------------------------------
// One DPP move of a 32- or 64-bit value (a register move: no trip through the LDS pipe that a shuffle takes).  CTRL:
// row_shl:n = 0x100 + n, row_shr:n = 0x110 + n, row_ror:n = 0x120 + n, all inside a 16-lane row.  BOUND_CTRL: lanes
// shifted in from outside the row read 0.
template <int CTRL, bool BOUND_CTRL = false, typename T>
__device__ __forceinline__ T dpp(T v) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "dpp moves 32- and 64-bit values");
  if constexpr (sizeof(T) == 4) {
    return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, BOUND_CTRL));
  } else {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo =
        static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(u), CTRL, 0xF, 0xF, BOUND_CTRL));
    const unsigned hi =
        static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(u >> 32), CTRL, 0xF, 0xF, BOUND_CTRL));
    return __builtin_bit_cast(T, (static_cast<unsigned long long>(hi) << 32) | lo);
  }
}
// v of lane `lane` (wave-uniform) through scalar registers
__device__ __forceinline__ double readlane(double v, int lane) {
  const unsigned long long u = __double_as_longlong(v);
  const unsigned lo = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(u), lane));
  const unsigned hi = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(u >> 32), lane));
  return __longlong_as_double((static_cast<unsigned long long>(hi) << 32) | lo);
}
// fold over the 16 lanes of a row, the result in every lane of the row: row_ror 1, 2, 4, 8
template <typename T, typename Op>
__device__ __forceinline__ T dpp_row_fold(T v, Op op) {
  v = op(v, dpp<0x121>(v));
  v = op(v, dpp<0x122>(v));
  v = op(v, dpp<0x124>(v));
  v = op(v, dpp<0x128>(v));
  return v;
}
// fold over the 32 lanes of a half-wave, the result in every lane: the row ladder and ONE ds_swizzle across the two rows
// (an xor ladder is five trips through the LDS pipe)
template <typename Op>
__device__ __forceinline__ float wave_half_fold(float v, Op op) {
  v = dpp_row_fold(v, op);
  return op(v, __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x1F | (16 << 10))));
}
// sum over the 64 lanes, the same value in every lane: the row ladder, then the four row sums read through scalar
// registers and added (r0 + r16) + (r32 + r48).  NOT the order of wave_sum.
__device__ __forceinline__ double wave_sum_rows(double v) {
  v = dpp_row_fold(v, op_add{});
  return (readlane(v, 0) + readlane(v, 16)) + (readlane(v, 32) + readlane(v, 48));
}

struct fold_xor {  // the wave-level folds a block fold is built on
  template <typename T, typename Op>
  __device__ __forceinline__ T operator()(T v, Op op) const { return wave_fold<64>(v, op); }
};
struct fold_rows {  // (sums only)
  __device__ __forceinline__ double operator()(double v, op_add) const { return wave_sum_rows(v); }
};

// ---- block folds --------------------------------------------------------------------------------------------------------
// Sequential form.  NV folds over the T threads of a workgroup behind ONE pair of barriers (sh: NV * T / 64 values);
// every thread gets every result.  The order: the wave-level fold `wave` (fold_xor: offsets 32, 16, 8, 4, 2, 1); one value
// per wave in sh; then t = 0, t = op(t, sh[w]) for w = 0 .. T / 64 - 1.  The fold starts from 0 for every op: a max over
// negative values would give 0 (the sums of the losses and of the NDP selector are its users today).  T == 64: the wave's fold is the result,
// no barrier and sh is not touched.
// Barriers: one before the write of sh, one before its reads, and one behind them only with TAIL.  Without TAIL a second
// call may follow directly (its first barrier comes after every thread's reads of this one); a caller that touches sh by
// other means between two calls needs a barrier of its own.  Memory a caller wrote to LDS before the call is visible to
// every thread after it.
template <int T, bool TAIL = false, int NV, typename V, typename Wave = fold_xor, typename Op = op_add>
__device__ __forceinline__ void block_fold_seq(V (&v)[NV], V* sh, Wave wave = Wave{}, Op op = Op{}) {
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    if constexpr (std::is_same_v<Wave, fold_xor>) {  // (wave_fold's ladder, written out: a call here moves instructions)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v[q] = op(v[q], __shfl_xor(v[q], o, 64));
    } else {
      v[q] = wave(v[q], op);
    }
  }
  if constexpr (T == 64) return;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < NV; ++q) sh[q * (T / 64) + (threadIdx.x >> 6)] = v[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    V t = 0;
#pragma unroll
    for (int w = 0; w < T / 64; ++w) t = op(t, sh[q * (T / 64) + w]);
    v[q] = t;
  }
  if constexpr (TAIL) __syncthreads();
}
template <int T, bool TAIL = false, typename V, typename Wave = fold_xor, typename Op = op_add>
__device__ __forceinline__ V block_fold_seq(V v, V* sh, Wave wave = Wave{}, Op op = Op{}) {  // sh: T / 64 values
  V one[1] = {v};
  block_fold_seq<T, TAIL>(one, sh, wave, op);
  return one[0];
}

// the float / double / integer sums of the sequential form under the names the loss kernels use
template <int T, int NV, typename V>
__device__ __forceinline__ void block_sums(V (&v)[NV], V* sh) { block_fold_seq<T>(v, sh); }
template <int T, typename V>
__device__ __forceinline__ V block_sum(V v, V* sh) {
  V one[1] = {v};
  block_fold_seq<T>(one, sh);
  return one[0];
}

// Pairwise form for a 256-thread workgroup (sh: 4 values): the xor fold inside the waves, then
// (sh0 op sh1) op (sh2 op sh3) -- for a float sum NOT the rounding of block_fold_seq<256>.  Barriers as above.
template <bool TAIL, typename V, typename Op>
__device__ __forceinline__ V block_fold_pair256(V v, V* sh, Op op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const V t = op(op(sh[0], sh[1]), op(sh[2], sh[3]));
  if constexpr (TAIL) __syncthreads();
  return t;
}

}  // namespace tgp
