// The walk of an edge-group index that ASAPooling's kernels (asap.hip) and the hub route (hub_walk.hip) share: group i =
// positions grp_perm[grp_ptr[i] .. grp_ptr[i + 1]) of the edge list (grp_perm NULL: the positions themselves), the far
// endpoint gathered through a position.  A position outside [0, E) or an endpoint outside [0, n) is skipped and never
// dereferenced.  Lane layout of the row kernels: G lanes share a row (a float4 each when VEC, under row_project2's
// alignment rule), the 64 / G slots of a wave take every (64 / G)-th entry.
#pragma once

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
