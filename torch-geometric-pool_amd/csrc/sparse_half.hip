// 16-bit storage forms (bfloat16 / float16) of the HBM-bound row operators: the sparse Reduce (and the Lift, the same
// kernel with node and supernode swapped), the packed one-to-one Reduce and the segment readout with its backward.
//
// Storage is 16 bits, arithmetic is fp32: every element is widened in registers right after its load, the sums run in
// fp32 in the order of the fp32 kernels (members of a supernode in ascending assignment order, the rows of a (group,
// feature) in ascending row order, the split route's fold of segment_plan.h), every product is rounded before its add,
// and the result is rounded to the storage type ONCE, to nearest even, at the store.  Widening is exact, so the bytes
// are those of  fp32_kernel(x.float()).to(dtype) -- without the N x F fp32 copy of x and the fp32 output in between.
//
// Work split (not the fp32 one): a lane owns EIGHT adjacent features, one 16-byte load; a lane group is the power of
// two covering F / 8, so an F = 128 row is 16 lanes and a wave holds four supernodes (or readout items).  A 16-bit row
// is half the sectors of an fp32 one, so a group keeps more rows in flight than its fp32 twin to have as many bytes
// on the way: eight in the general Reduce, four in the packed one-to-one form, eight in the readout.  All index levels
// (table entry -> node id + weight -> row) are issued level by level from clamped indices; a clamped load's value is
// dropped by a select.  F % 8 != 0, a row stride that is no multiple of 8 elements or a pointer off 16 bytes: one lane
// per feature (the *_scalar kernels below).
#include "common.h"
#include "segment_plan.h"

namespace tgp {

typedef uint32_t h_u32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------ the two storage types
struct Bf16 {  // widening is a 16-bit shift; narrowing rounds to nearest even, a NaN becomes a quiet NaN
  static __device__ __forceinline__ float up(uint32_t h) { return __uint_as_float(h << 16); }
  static __device__ __forceinline__ uint32_t down(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x0040u;
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
  }
};
struct Fp16 {  // _Float16 conversions: exact up, round-to-nearest-even down (a sum past 65504 gives inf)
  static __device__ __forceinline__ float up(uint32_t h) {
    return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(h)));
  }
  static __device__ __forceinline__ uint32_t down(float f) {
    return __builtin_bit_cast(uint16_t, static_cast<_Float16>(f));
  }
};

template <typename T>
__device__ __forceinline__ void h_widen8(const h_u32x4 t, float* v) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[2 * j] = T::up(t[j] & 0xFFFFu);
    v[2 * j + 1] = T::up(t[j] >> 16);
  }
}
template <typename T>
__device__ __forceinline__ h_u32x4 h_narrow8(const float* v) {
  h_u32x4 t;
#pragma unroll
  for (int j = 0; j < 4; ++j) t[j] = T::down(v[2 * j]) | (T::down(v[2 * j + 1]) << 16);
  return t;
}
// VEC (8 or 1) elements at p
template <typename T, int VEC>
__device__ __forceinline__ void h_get(const uint16_t* p, float* v) {
  if constexpr (VEC == 8) h_widen8<T>(*reinterpret_cast<const h_u32x4*>(p), v);
  else v[0] = T::up(p[0]);
}
template <typename T, int VEC>
__device__ __forceinline__ void h_put(uint16_t* p, const float* v) {
  if constexpr (VEC == 8) *reinterpret_cast<h_u32x4*>(p) = h_narrow8<T>(v);
  else p[0] = static_cast<uint16_t>(T::down(v[0]));
}

// ------------------------------------------------------------------------------------------------ sparse Reduce / Lift
// One group of G lanes per supernode, lane g owns features [8g, 8g + 8) (+ 8G strides).  U supernodes x MP members are
// requested per round: slots, then node ids + weights, then the U * MP rows, each level side by side.
template <typename T, int G, int U, int MP>
__global__ __launch_bounds__(256) void reduce_h16_kernel(const uint16_t* __restrict__ x, int64_t num_nodes, int64_t F,
                                                         int64_t ld, const int64_t* __restrict__ node_index,
                                                         const float* __restrict__ weight,
                                                         const int32_t* __restrict__ row_ptr,
                                                         const int32_t* __restrict__ perm, int64_t nnz, int64_t K,
                                                         uint16_t* __restrict__ out) {
  constexpr int GROUPS = 256 / G;
  const int g = threadIdx.x % G;
  const int64_t group = static_cast<int64_t>(blockIdx.x) * GROUPS + threadIdx.x / G;
  const int64_t ngroups = static_cast<int64_t>(gridDim.x) * GROUPS;
  const int32_t last = static_cast<int32_t>(nnz > 0 ? nnz - 1 : 0);
  for (int64_t c0 = group; c0 < K; c0 += ngroups * U) {
    int32_t beg[U], len[U];
    int32_t maxlen = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t c = c0 + u * ngroups;
      const int64_t cc = c < K ? c : K - 1;
      if (row_ptr) {
        beg[u] = row_ptr[cc];
        len[u] = row_ptr[cc + 1] - beg[u];
      } else {  // one assignment per supernode
        beg[u] = static_cast<int32_t>(cc);
        len[u] = 1;
      }
      if (c >= K) len[u] = -1;
      maxlen = len[u] > maxlen ? len[u] : maxlen;
    }
    for (int64_t f = 8 * g; f < F; f += 8 * G) {
      float acc[U][8];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[u][j] = 0.f;
      for (int32_t m0 = 0; m0 < maxlen; m0 += MP) {  // (nnz > 0 inside: some supernode has a member)
        int32_t a[U][MP];
        float w[U][MP];
        int64_t n[U][MP];
        h_u32x4 v[U][MP];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int q = 0; q < MP; ++q) {
            int32_t slot = beg[u] + (m0 + q < len[u] ? m0 + q : 0);
            slot = slot < 0 ? 0 : (slot < last ? slot : last);
            const int32_t as = perm ? perm[slot] : slot;
            a[u][q] = static_cast<uint32_t>(as) <= static_cast<uint32_t>(last) ? as : 0;
          }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int q = 0; q < MP; ++q) {
            w[u][q] = weight ? weight[a[u][q]] : 1.0f;
            const int64_t nn = node_index ? node_index[a[u][q]] : static_cast<int64_t>(a[u][q]);
            n[u][q] = static_cast<uint64_t>(nn) < static_cast<uint64_t>(num_nodes) ? nn : -1;
          }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int q = 0; q < MP; ++q)  // rows are read once: keep them out of the way of the index tables
            v[u][q] = __builtin_nontemporal_load(
                reinterpret_cast<const h_u32x4*>(x + (n[u][q] < 0 ? 0 : n[u][q]) * ld + f));
#pragma unroll
        for (int q = 0; q < MP; ++q)
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const bool on = m0 + q < len[u] && n[u][q] >= 0;  // (a row outside x is skipped, never read)
            float r[8];
            h_widen8<T>(v[u][q], r);
#pragma unroll
            for (int j = 0; j < 8; ++j) {  // the product is rounded before the add
              const float s = __fadd_rn(acc[u][j], __fmul_rn(r[j], w[u][q]));
              acc[u][j] = on ? s : acc[u][j];
            }
          }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t c = c0 + u * ngroups;
        if (len[u] >= 0)
          __builtin_nontemporal_store(h_narrow8<T>(acc[u]), reinterpret_cast<h_u32x4*>(out + c * F + f));
      }
    }
  }
}

// The packed one-to-one index (TopK, NDP): pack[c] = {int32 source row, fp32 weight}, one streamed 8-byte load per
// supernode, then U rows in flight per group.  out = 0 + x * w: the products of the general kernel.
template <typename T, int G, int U, bool HAS_W>
__global__ __launch_bounds__(256) void reduce_one_to_one_h16_kernel(const uint16_t* __restrict__ x, int64_t num_nodes,
                                                                    int64_t F, int64_t ld,
                                                                    const uint2* __restrict__ pack, int64_t K,
                                                                    uint16_t* __restrict__ out) {
  constexpr int GROUPS = 256 / G;
  const int g = threadIdx.x % G;
  const int64_t group = static_cast<int64_t>(blockIdx.x) * GROUPS + threadIdx.x / G;
  const int64_t ngroups = static_cast<int64_t>(gridDim.x) * GROUPS;
  for (int64_t c0 = group; c0 < K; c0 += ngroups * U) {
    int64_t c[U];
    uint2 pk[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      c[u] = c0 + u * ngroups;
      pk[u] = pack[c[u] < K ? c[u] : K - 1];
    }
    for (int64_t f = 8 * g; f < F; f += 8 * G) {
      h_u32x4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t n = static_cast<int64_t>(pk[u].x) < num_nodes ? static_cast<int64_t>(pk[u].x) : 0;
        v[u] = __builtin_nontemporal_load(reinterpret_cast<const h_u32x4*>(x + n * ld + f));
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (c[u] < K) {
          const float w = HAS_W ? __uint_as_float(pk[u].y) : 1.0f;
          const bool on = static_cast<int64_t>(pk[u].x) < num_nodes;
          float r[8];
          h_widen8<T>(v[u], r);
#pragma unroll
          for (int j = 0; j < 8; ++j) r[j] = on ? __fadd_rn(0.f, __fmul_rn(r[j], w)) : 0.f;
          __builtin_nontemporal_store(h_narrow8<T>(r), reinterpret_cast<h_u32x4*>(out + c[u] * F + f));
        }
      }
    }
  }
}

// one lane per (supernode, feature): every shape; `pack` given: the packed one-to-one index instead of the tables
template <typename T>
__global__ __launch_bounds__(256) void reduce_h16_scalar_kernel(const uint16_t* __restrict__ x, int64_t num_nodes,
                                                                int64_t F, int64_t ld,
                                                                const int64_t* __restrict__ node_index,
                                                                const float* __restrict__ weight,
                                                                const int32_t* __restrict__ row_ptr,
                                                                const int32_t* __restrict__ perm,
                                                                const uint2* __restrict__ pack, int has_weight,
                                                                int64_t nnz, int64_t K, uint16_t* __restrict__ out) {
  const int64_t total = K * F;
  for (int64_t o = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; o < total;
       o += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t c = o / F, f = o - c * F;
    float acc = 0.f;
    if (pack) {
      const uint2 pk = pack[c];
      if (static_cast<int64_t>(pk.x) < num_nodes)
        acc = __fadd_rn(0.f, __fmul_rn(T::up(x[static_cast<int64_t>(pk.x) * ld + f]),
                                       has_weight ? __uint_as_float(pk.y) : 1.0f));
    } else {
      int64_t p_beg = row_ptr ? row_ptr[c] : c, p_end = row_ptr ? row_ptr[c + 1] : c + 1;
      p_beg = p_beg < 0 ? 0 : p_beg;
      p_end = p_end > nnz ? nnz : p_end;
      for (int64_t p = p_beg; p < p_end; ++p) {
        const int64_t a = perm ? static_cast<int64_t>(perm[p]) : p;
        if (static_cast<uint64_t>(a) >= static_cast<uint64_t>(nnz)) continue;
        const int64_t n = node_index ? node_index[a] : a;
        if (static_cast<uint64_t>(n) >= static_cast<uint64_t>(num_nodes)) continue;
        acc = __fadd_rn(acc, __fmul_rn(T::up(x[n * ld + f]), weight ? weight[a] : 1.0f));
      }
    }
    out[o] = static_cast<uint16_t>(T::down(acc));
  }
}

// ------------------------------------------------------------------------------------------------ segment readout
constexpr int SH_U = 8;  // rows a lane group has in flight
constexpr int SH_OPS_ALL = (1 << TGP_SUM) | (1 << TGP_MEAN) | (1 << TGP_MIN) | (1 << TGP_MAX);
constexpr int SH_OPS_SUMS = (1 << TGP_SUM) | (1 << TGP_MEAN);
constexpr int SH_OPS_MM = (1 << TGP_MIN) | (1 << TGP_MAX);

struct ShSrc {
  const uint16_t* x;
  int64_t num_rows, F, ld;
  const int64_t* ptr;         // contiguous segments [G + 1]
  int64_t dense_nodes;        // > 0: group g owns rows g * dense_nodes ...
  const uint8_t* mask;        // dense only, NULL = every row
  const int32_t* row_ptr;     // gathered: NULL = group g owns assignment g
  const int32_t* perm;        // gathered: NULL = positions are assignments
  const int64_t* node_index;  // gathered
  const float* weight;        // gathered, NULL = ones
  int64_t nnz;
};

struct ShOut {
  uint16_t* out;      // [G, n_ops * F], operations in enum order
  int32_t* ties;      // [G, n_mm * F] (min, then max) or NULL
  int32_t* count;     // [G] or NULL
  int ops, n_ops, n_mm;
  float* part;        // split route: [items, slots, F], fp32 records (only the fold's last write rounds)
  int32_t* part_cnt;  // split route: [items]
};

template <int VEC>
struct ShAcc {
  float sum[VEC], mn[VEC], mx[VEC];
  int32_t cmn[VEC], cmx[VEC];
  int32_t cnt;
  __device__ __forceinline__ void init() {
    cnt = 0;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      sum[j] = 0.f;
      mn[j] = __builtin_inff();
      mx[j] = -__builtin_inff();
      cmn[j] = cmx[j] = 0;
    }
  }
};

// rows of group g: positions beg .. beg + len - 1 of the source's position space, never outside it
__device__ __forceinline__ void sh_extent(const ShSrc& s, int64_t g, int64_t& beg, int64_t& len) {
  int64_t b, e, lim;
  if (s.ptr) {
    b = s.ptr[g];
    e = s.ptr[g + 1];
    lim = s.num_rows;
  } else if (s.dense_nodes > 0) {
    b = g * s.dense_nodes;
    e = b + s.dense_nodes;
    lim = s.num_rows;
  } else {
    b = s.row_ptr ? static_cast<int64_t>(s.row_ptr[g]) : g;
    e = s.row_ptr ? static_cast<int64_t>(s.row_ptr[g + 1]) : g + 1;
    lim = s.nnz;
  }
  b = b < 0 ? 0 : (b > lim ? lim : b);
  e = e < b ? b : (e > lim ? lim : e);
  beg = b;
  len = e - b;
}

// one more row: NaN wins the extremes (torch.amax / amin), the counters hold the rows that attain them
template <bool SUMS, bool MM>
__device__ __forceinline__ void sh_add(float v, float& sum, float& mn, float& mx, int32_t& cmn, int32_t& cmx) {
  if constexpr (SUMS) sum = sum + v;
  if constexpr (MM) {
    const bool nan = v != v;
    const bool gt = v > mx, lt = v < mn;
    cmx = gt ? 1 : (v == mx ? cmx + 1 : cmx);
    cmn = lt ? 1 : (v == mn ? cmn + 1 : cmn);
    mx = (gt || nan) ? v : mx;
    mn = (lt || nan) ? v : mn;
  }
}

// fold a later partial into an earlier one
__device__ __forceinline__ void sh_fold_extreme(float& m, int32_t& c, float pm, int32_t pc, bool is_max) {
  if (m != m) return;  // NaN stays
  if (pm != pm) {
    m = pm;
    return;
  }
  const bool better = is_max ? pm > m : pm < m;
  c = better ? pc : (pm == m ? c + pc : c);
  m = better ? pm : m;
}

template <int VEC, typename V>
__device__ __forceinline__ void sh_store32(V* p, const V* v) {  // fp32 records and int32 counters
  if constexpr (VEC >= 4) {
#pragma unroll
    for (int j = 0; j < VEC; j += 4) {
      h_u32x4 t;
#pragma unroll
      for (int k = 0; k < 4; ++k) t[k] = __builtin_bit_cast(uint32_t, v[j + k]);
      *reinterpret_cast<h_u32x4*>(p + j) = t;
    }
  } else {
    p[0] = v[0];
  }
}

// the finished group, rounded here and nowhere else: empty groups give 0, the mean divides by max(count, 1)
template <typename T, int VEC>
__device__ __forceinline__ void sh_emit(const ShOut& o, int64_t F, int64_t g, int64_t f, const ShAcc<VEC>& a) {
  uint16_t* row = o.out + g * (static_cast<int64_t>(o.n_ops) * F) + f;
  const float denom = static_cast<float>(a.cnt > 1 ? a.cnt : 1);
  const bool any = a.cnt > 0;
  float v[VEC];
  int slot = 0;
  if (o.ops & (1 << TGP_SUM)) {
    h_put<T, VEC>(row + slot * F, a.sum);
    ++slot;
  }
  if (o.ops & (1 << TGP_MEAN)) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) v[j] = a.sum[j] / denom;
    h_put<T, VEC>(row + slot * F, v);
    ++slot;
  }
  if (o.ops & (1 << TGP_MIN)) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) v[j] = any ? a.mn[j] : 0.f;
    h_put<T, VEC>(row + slot * F, v);
    ++slot;
  }
  if (o.ops & (1 << TGP_MAX)) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) v[j] = any ? a.mx[j] : 0.f;
    h_put<T, VEC>(row + slot * F, v);
    ++slot;
  }
  if (o.ties) {
    int32_t* trow = o.ties + g * (static_cast<int64_t>(o.n_mm) * F) + f;
    int j = 0;
    if (o.ops & (1 << TGP_MIN)) {
      sh_store32<VEC>(trow + j * F, a.cmn);
      ++j;
    }
    if (o.ops & (1 << TGP_MAX)) sh_store32<VEC>(trow + j * F, a.cmx);
  }
  if (o.count && f == 0) o.count[g] = a.cnt;
}

// A group of 2^lg_shift lanes owns one (segment, row chunk) item, a lane VEC adjacent features of it: the lane adds
// its rows one after the other in ascending row order, SH_U row loads in flight.
template <typename T, int VEC, bool SUMS, bool MM, bool GATHER>
__global__ __launch_bounds__(256) void segment_aggr_h16_kernel(ShSrc s, ShOut o, int64_t G, int lg_shift, int64_t chunk,
                                                               int64_t n_chunks) {
  const int lg = 1 << lg_shift;
  const int lane = threadIdx.x & (lg - 1);
  const int64_t item = static_cast<int64_t>(blockIdx.x) * (256 >> lg_shift) + (threadIdx.x >> lg_shift);
  const int64_t f = (static_cast<int64_t>(blockIdx.y) * lg + lane) * VEC;
  if (item >= G * n_chunks || f >= s.F) return;
  const int64_t g = item / n_chunks, c = item - g * n_chunks;
  int64_t beg, len;
  sh_extent(s, g, beg, len);
  const int64_t r0 = c * chunk;
  if (c > 0 && r0 >= len) return;  // (the fold knows from len which chunks ran)
  const int64_t r1 = (c == n_chunks - 1 || r0 + chunk > len) ? len : r0 + chunk;

  ShAcc<VEC> a;
  a.init();
  for (int64_t r = r0; r < r1; r += SH_U) {
    bool on[SH_U];
    int64_t row[SH_U];
    float w[SH_U];
    float v[SH_U][VEC];
    if constexpr (GATHER) {  // position -> assignment -> (source row, weight), level by level, from clamped indices
      int64_t as[SH_U];
#pragma unroll
      for (int u = 0; u < SH_U; ++u) {
        on[u] = r + u < r1;
        const int64_t p = beg + (on[u] ? r + u : r);
        as[u] = s.perm ? static_cast<int64_t>(s.perm[p]) : p;
      }
#pragma unroll
      for (int u = 0; u < SH_U; ++u) {
        on[u] = on[u] && static_cast<uint64_t>(as[u]) < static_cast<uint64_t>(s.nnz);
        const int64_t ac = on[u] ? as[u] : 0;  // (nnz > 0 here: the loop runs only over existing positions)
        row[u] = s.node_index[ac];
        w[u] = s.weight ? s.weight[ac] : 1.0f;
      }
#pragma unroll
      for (int u = 0; u < SH_U; ++u) on[u] = on[u] && static_cast<uint64_t>(row[u]) < static_cast<uint64_t>(s.num_rows);
    } else {
#pragma unroll
      for (int u = 0; u < SH_U; ++u) {
        on[u] = r + u < r1;
        row[u] = beg + r + u;
        w[u] = 1.0f;
      }
      if (s.mask) {
#pragma unroll
        for (int u = 0; u < SH_U; ++u) on[u] = on[u] && s.mask[on[u] ? row[u] : beg] != 0;
      }
    }
#pragma unroll
    for (int u = 0; u < SH_U; ++u) {
      if (on[u]) {
        h_get<T, VEC>(s.x + row[u] * s.ld + f, v[u]);
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[u][j] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < SH_U; ++u) {
      if (on[u]) {
        ++a.cnt;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const float t = GATHER ? __fmul_rn(v[u][j], w[u]) : v[u][j];  // the product is rounded before the add
          sh_add<SUMS, MM>(t, a.sum[j], a.mn[j], a.mx[j], a.cmn[j], a.cmx[j]);
        }
      }
    }
  }

  if (n_chunks == 1) {
    sh_emit<T, VEC>(o, s.F, g, f, a);
    return;
  }
  constexpr int SLOTS = (SUMS ? 1 : 0) + (MM ? 4 : 0);
  float* rec = o.part + item * (SLOTS * s.F) + f;
  int slot = 0;
  if constexpr (SUMS) {
    sh_store32<VEC>(rec, a.sum);
    slot = 1;
  }
  if constexpr (MM) {
    sh_store32<VEC>(rec + slot * s.F, a.mn);
    sh_store32<VEC>(rec + (slot + 1) * s.F, a.mx);
    sh_store32<VEC>(reinterpret_cast<int32_t*>(rec + (slot + 2) * s.F), a.cmn);
    sh_store32<VEC>(reinterpret_cast<int32_t*>(rec + (slot + 3) * s.F), a.cmx);
  }
  if (f == 0) o.part_cnt[item] = a.cnt;
}

// split route, second kernel: the fold of segment_aggr.hip over the same fp32 records -- one workgroup per (group,
// 4 features), SA_FOLD_PARTS threads per feature each fold a contiguous run of chunk records in ascending order, then
// one thread folds the runs in ascending order -- and the one rounding at the end.
template <bool SUMS, bool MM>
__device__ __forceinline__ void sh_fold_record(ShAcc<1>& a, float sum, float mn, int32_t cmn, float mx, int32_t cmx) {
  if constexpr (SUMS) a.sum[0] = a.sum[0] + sum;
  if constexpr (MM) {
    sh_fold_extreme(a.mn[0], a.cmn[0], mn, cmn, false);
    sh_fold_extreme(a.mx[0], a.cmx[0], mx, cmx, true);
  }
}

template <typename T, bool SUMS, bool MM>
__global__ __launch_bounds__(256) void segment_aggr_fold_h16_kernel(ShSrc s, ShOut o, int64_t G, int64_t chunk,
                                                                    int64_t n_chunks) {
  constexpr int SLOTS = (SUMS ? 1 : 0) + (MM ? 4 : 0);
  __shared__ float sh_f[3][SA_FOLD_PARTS][4];
  __shared__ int32_t sh_i[3][SA_FOLD_PARTS][4];
  const int j = threadIdx.x & 3, p = threadIdx.x >> 2;
  const int64_t tiles = (s.F + 3) / 4;
  const int64_t g = blockIdx.x / tiles, f = (blockIdx.x - g * tiles) * 4 + j;
  int64_t beg, len;
  sh_extent(s, g, beg, len);
  int64_t n_run = (len + chunk - 1) / chunk;  // chunk 0 always ran; chunk c > 0 ran when c * chunk < len
  n_run = n_run < 1 ? 1 : (n_run > n_chunks ? n_chunks : n_run);
  const int64_t per = (n_run + SA_FOLD_PARTS - 1) / SA_FOLD_PARTS;
  const int64_t c0 = p * per, c1 = c0 + per < n_run ? c0 + per : n_run;
  ShAcc<1> a;
  a.init();
  if (f < s.F) {
    for (int64_t c = c0; c < c1; ++c) {
      const int64_t item = g * n_chunks + c;
      const float* rec = o.part + item * (SLOTS * s.F) + f;
      const int32_t* reci = reinterpret_cast<const int32_t*>(rec);
      a.cnt += o.part_cnt[item];
      constexpr int m0 = SUMS ? 1 : 0;
      sh_fold_record<SUMS, MM>(a, SUMS ? rec[0] : 0.f, MM ? rec[m0 * s.F] : 0.f, MM ? reci[(m0 + 2) * s.F] : 0,
                               MM ? rec[(m0 + 1) * s.F] : 0.f, MM ? reci[(m0 + 3) * s.F] : 0);
    }
  }
  sh_f[0][p][j] = a.sum[0], sh_f[1][p][j] = a.mn[0], sh_f[2][p][j] = a.mx[0];
  sh_i[0][p][j] = a.cmn[0], sh_i[1][p][j] = a.cmx[0], sh_i[2][p][j] = a.cnt;
  __syncthreads();
  if (p != 0 || f >= s.F) return;
  const int parts = static_cast<int>((n_run + per - 1) / per);
  for (int q = 1; q < parts; ++q) {
    a.cnt += sh_i[2][q][j];
    sh_fold_record<SUMS, MM>(a, sh_f[0][q][j], sh_f[1][q][j], sh_i[0][q][j], sh_f[2][q][j], sh_i[1][q][j]);
  }
  sh_emit<T, 1>(o, s.F, g, f, a);
}

// dX[row, :] = sum over the requested operations of that operation's share of its group's upstream gradient: the
// terms of the fp32 backward in its order (sum, mean, min, max), over widened g_out / x / out, rounded once
template <typename T, int VEC>
__global__ __launch_bounds__(256) void segment_aggr_bwd_h16_kernel(
    const uint16_t* __restrict__ go, const uint16_t* __restrict__ x, int64_t num_rows, int64_t F, int64_t ld,
    const int64_t* __restrict__ batch, int64_t dense_nodes, const uint8_t* __restrict__ mask,
    const uint16_t* __restrict__ out, const int32_t* __restrict__ ties, const int32_t* __restrict__ count, int64_t G,
    int ops, int n_ops, int n_mm, uint16_t* __restrict__ dx) {
  const int64_t fv = F / VEC;
  const int64_t total = num_rows * fv;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t row = i / fv, f = (i - row * fv) * VEC;
    const int64_t g = batch ? batch[row] : (dense_nodes > 0 ? row / dense_nodes : 0);
    float acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
    if (static_cast<uint64_t>(g) < static_cast<uint64_t>(G) && (!mask || mask[row] != 0)) {
      const uint16_t* grow = go + g * (static_cast<int64_t>(n_ops) * F) + f;
      float gv[VEC];
      int slot = 0, mm = 0;
      if (ops & (1 << TGP_SUM)) {
        h_get<T, VEC>(grow + slot * F, gv);
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] = acc[j] + gv[j];
        ++slot;
      }
      if (ops & (1 << TGP_MEAN)) {
        const int32_t cnt = count[g];
        const float denom = static_cast<float>(cnt > 1 ? cnt : 1);
        h_get<T, VEC>(grow + slot * F, gv);
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] = acc[j] + gv[j] / denom;
        ++slot;
      }
      if (ops & SH_OPS_MM) {
        float xv[VEC], ov[VEC];
        h_get<T, VEC>(x + row * ld + f, xv);
#pragma unroll
        for (int op = TGP_MIN; op <= TGP_MAX; ++op) {
          if (ops & (1 << op)) {
            h_get<T, VEC>(out + g * (static_cast<int64_t>(n_ops) * F) + slot * F + f, ov);
            h_get<T, VEC>(grow + slot * F, gv);
            const int32_t* trow = ties + g * (static_cast<int64_t>(n_mm) * F) + mm * F + f;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
              const float share = gv[j] / static_cast<float>(trow[j] > 1 ? trow[j] : 1);
              acc[j] = acc[j] + (xv[j] == ov[j] ? share : 0.f);
            }
            ++slot;
            ++mm;
          }
        }
      }
    }
    h_put<T, VEC>(dx + row * F + f, acc);
  }
}

}  // namespace tgp

using namespace tgp;

static bool h_aligned(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }
static bool h_dtype_ok(int dtype) { return dtype == TGP_BF16 || dtype == TGP_F16; }
static int h_popcount(int v) { return __builtin_popcount(static_cast<unsigned>(v)); }
static int h_lane_group(int64_t lanes) {  // the power of two covering `lanes`, at most a wave
  int G = 1;
  while (G < lanes && G < 64) G <<= 1;
  return G;
}
static dim3 h_reduce_grid(int64_t K, int G, int U) {  // persistent: at most 8 workgroups per compute unit
  const int64_t per_block = static_cast<int64_t>(256 / G) * U;
  int64_t blocks = (K + per_block - 1) / per_block;
  blocks = blocks > 256 * 8 ? 256 * 8 : (blocks < 1 ? 1 : blocks);
  return dim3(static_cast<unsigned>(blocks));
}
static dim3 h_scalar_grid(int64_t total) {
  int64_t blocks = (total + 255) / 256;
  return dim3(static_cast<unsigned>(blocks > 256 * 16 ? 256 * 16 : (blocks < 1 ? 1 : blocks)));
}

// the lane-group widths every vector kernel is built for
#define TGP_H_SWITCH_G(G, LAUNCH) \
  switch (G) {                    \
    case 1: LAUNCH(1); break;     \
    case 2: LAUNCH(2); break;     \
    case 4: LAUNCH(4); break;     \
    case 8: LAUNCH(8); break;     \
    case 16: LAUNCH(16); break;   \
    case 32: LAUNCH(32); break;   \
    default: LAUNCH(64); break;   \
  }

template <typename T>
static void h_reduce_sparse(const uint16_t* x, int64_t num_nodes, int64_t F, int64_t ld, const int64_t* node_index,
                            const float* weight, const int32_t* row_ptr, const int32_t* perm, int64_t nnz, int64_t K,
                            uint16_t* out, hipStream_t stream) {
  if (F % 8 != 0 || ld % 8 != 0 || !h_aligned(x) || !h_aligned(out)) {
    hipLaunchKernelGGL(reduce_h16_scalar_kernel<T>, h_scalar_grid(K * F), dim3(256), 0, stream, x, num_nodes, F, ld,
                       node_index, weight, row_ptr, perm, static_cast<const uint2*>(nullptr), 0, nnz, K, out);
    return;
  }
  const int G = h_lane_group(F / 8);
  // eight rows in flight per group: supernodes of at most two members (a matching, the Lift of a one-over-K selector)
  // ask for two members of four supernodes, longer member lists for four members of two
  if (nnz <= 2 * K) {
#define TGP_H_LAUNCH(GG)                                                                                              \
  hipLaunchKernelGGL((reduce_h16_kernel<T, GG, 4, 2>), h_reduce_grid(K, GG, 4), dim3(256), 0, stream, x, num_nodes, F, \
                     ld, node_index, weight, row_ptr, perm, nnz, K, out)
    TGP_H_SWITCH_G(G, TGP_H_LAUNCH)
#undef TGP_H_LAUNCH
  } else {
#define TGP_H_LAUNCH(GG)                                                                                              \
  hipLaunchKernelGGL((reduce_h16_kernel<T, GG, 2, 4>), h_reduce_grid(K, GG, 2), dim3(256), 0, stream, x, num_nodes, F, \
                     ld, node_index, weight, row_ptr, perm, nnz, K, out)
    TGP_H_SWITCH_G(G, TGP_H_LAUNCH)
#undef TGP_H_LAUNCH
  }
}

extern "C" int tgp_reduce_sparse_h16(int dtype, const void* x, int64_t num_nodes, int64_t F, int64_t x_stride,
                                     const int64_t* node_index, const float* weight, const int32_t* row_ptr,
                                     const int32_t* perm, int64_t nnz, int64_t K, void* x_pool, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(h_dtype_ok(dtype), TGP_ERR_INVALID, "tgp_reduce_sparse_h16: dtype is neither TGP_BF16 nor TGP_F16");
  TGP_REQUIRE(num_nodes >= 0 && F >= 0 && K >= 0 && nnz >= 0 && x_stride >= F && (row_ptr || nnz == K),
              TGP_ERR_INVALID, "tgp_reduce_sparse_h16: bad argument");  // row_ptr == NULL: one assignment per supernode
  TGP_REQUIRE(nnz < (1ll << 31) && K < (1ll << 31), TGP_ERR_RANGE, "tgp_reduce_sparse_h16: nnz or K >= 2^31");
  if (K == 0 || F == 0) return TGP_OK;
  TGP_REQUIRE(x_pool && (nnz == 0 || (x && num_nodes > 0)), TGP_ERR_INVALID, "tgp_reduce_sparse_h16: null pointer");
  TGP_REQUIRE(node_index || nnz <= num_nodes, TGP_ERR_INVALID,
              "tgp_reduce_sparse_h16: node_index may only be omitted when assignment i reads row i (nnz <= num_nodes)");
  const uint16_t* xs = static_cast<const uint16_t*>(x);
  uint16_t* os = static_cast<uint16_t*>(x_pool);
  if (dtype == TGP_BF16)
    h_reduce_sparse<Bf16>(xs, num_nodes, F, x_stride, node_index, weight, row_ptr, perm, nnz, K, os, stream);
  else
    h_reduce_sparse<Fp16>(xs, num_nodes, F, x_stride, node_index, weight, row_ptr, perm, nnz, K, os, stream);
  return check_launch("tgp_reduce_sparse_h16");
}

template <typename T>
static void h_reduce_one_to_one(const uint16_t* x, int64_t num_nodes, int64_t F, int64_t ld, const uint2* pack,
                                int has_weight, int64_t K, uint16_t* out, hipStream_t stream) {
  if (F % 8 != 0 || ld % 8 != 0 || !h_aligned(x) || !h_aligned(out)) {
    hipLaunchKernelGGL(reduce_h16_scalar_kernel<T>, h_scalar_grid(K * F), dim3(256), 0, stream, x, num_nodes, F, ld,
                       static_cast<const int64_t*>(nullptr), static_cast<const float*>(nullptr),
                       static_cast<const int32_t*>(nullptr), static_cast<const int32_t*>(nullptr), pack, has_weight, K,
                       K, out);
    return;
  }
  const int G = h_lane_group(F / 8);
  // four rows in flight per group (the fp32 form settled on one): a 16-bit row is half the bytes, and an F = 128 group
  // is a quarter of a wave, so a wave still has sixteen 256-byte rows on the way
#define TGP_H_LAUNCH(GG)                                                                                              \
  do {                                                                                                                \
    if (has_weight)                                                                                                   \
      hipLaunchKernelGGL((reduce_one_to_one_h16_kernel<T, GG, 4, true>), h_reduce_grid(K, GG, 4), dim3(256), 0, stream, \
                         x, num_nodes, F, ld, pack, K, out);                                                          \
    else                                                                                                              \
      hipLaunchKernelGGL((reduce_one_to_one_h16_kernel<T, GG, 4, false>), h_reduce_grid(K, GG, 4), dim3(256), 0,      \
                         stream, x, num_nodes, F, ld, pack, K, out);                                                  \
  } while (0)
  TGP_H_SWITCH_G(G, TGP_H_LAUNCH)
#undef TGP_H_LAUNCH
}

extern "C" int tgp_reduce_one_to_one_h16(int dtype, const void* x, int64_t num_nodes, int64_t F, int64_t x_stride,
                                         const uint64_t* pack, int has_weight, int64_t K, void* x_pool, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(h_dtype_ok(dtype), TGP_ERR_INVALID, "tgp_reduce_one_to_one_h16: dtype is neither TGP_BF16 nor TGP_F16");
  TGP_REQUIRE(num_nodes >= 0 && F >= 0 && K >= 0 && x_stride >= F, TGP_ERR_INVALID,
              "tgp_reduce_one_to_one_h16: bad argument");
  TGP_REQUIRE(num_nodes < (1ll << 31) && K < (1ll << 31), TGP_ERR_RANGE,
              "tgp_reduce_one_to_one_h16: num_nodes or K >= 2^31");
  if (K == 0 || F == 0) return TGP_OK;
  TGP_REQUIRE(x && pack && x_pool && num_nodes > 0, TGP_ERR_INVALID, "tgp_reduce_one_to_one_h16: null pointer");
  const uint16_t* xs = static_cast<const uint16_t*>(x);
  const uint2* pk = reinterpret_cast<const uint2*>(pack);
  uint16_t* os = static_cast<uint16_t*>(x_pool);
  if (dtype == TGP_BF16) h_reduce_one_to_one<Bf16>(xs, num_nodes, F, x_stride, pk, has_weight, K, os, stream);
  else h_reduce_one_to_one<Fp16>(xs, num_nodes, F, x_stride, pk, has_weight, K, os, stream);
  return check_launch("tgp_reduce_one_to_one_h16");
}

template <typename T>
static void h_segment_aggr(const ShSrc& s, const ShOut& o, int64_t G, int64_t chunk, int64_t n_chunks, bool vec,
                           dim3 grid, int lg_shift, hipStream_t stream) {
  const bool sums = (o.ops & SH_OPS_SUMS) != 0, mm = (o.ops & SH_OPS_MM) != 0, gather = s.node_index != nullptr;
#define TGP_SH_LAUNCH(VEC, SUMS, MM, GATHER)                                                                         \
  hipLaunchKernelGGL((segment_aggr_h16_kernel<T, VEC, SUMS, MM, GATHER>), grid, dim3(256), 0, stream, s, o, G, lg_shift, \
                     chunk, n_chunks)
#define TGP_SH_SOURCE(VEC, SUMS, MM)                \
  do {                                              \
    if (gather) TGP_SH_LAUNCH(VEC, SUMS, MM, true); \
    else TGP_SH_LAUNCH(VEC, SUMS, MM, false);       \
  } while (0)
#define TGP_SH_OPS(VEC)                             \
  do {                                              \
    if (sums && mm) TGP_SH_SOURCE(VEC, true, true); \
    else if (sums) TGP_SH_SOURCE(VEC, true, false); \
    else TGP_SH_SOURCE(VEC, false, true);           \
  } while (0)
  if (vec) TGP_SH_OPS(8);
  else TGP_SH_OPS(1);
#undef TGP_SH_OPS
#undef TGP_SH_SOURCE
#undef TGP_SH_LAUNCH
  if (n_chunks > 1) {
    const dim3 fgrid(static_cast<unsigned>(G * ((s.F + 3) / 4)));  // (G <= SA_MAX_ITEMS / 2 here, F < 2^19: in range)
    if (sums && mm)
      hipLaunchKernelGGL((segment_aggr_fold_h16_kernel<T, true, true>), fgrid, dim3(256), 0, stream, s, o, G, chunk,
                         n_chunks);
    else if (sums)
      hipLaunchKernelGGL((segment_aggr_fold_h16_kernel<T, true, false>), fgrid, dim3(256), 0, stream, s, o, G, chunk,
                         n_chunks);
    else
      hipLaunchKernelGGL((segment_aggr_fold_h16_kernel<T, false, true>), fgrid, dim3(256), 0, stream, s, o, G, chunk,
                         n_chunks);
  }
}

extern "C" int tgp_segment_aggr_h16(int dtype, const void* x, int64_t num_rows, int64_t F, int64_t ldx,
                                    const int64_t* ptr, int64_t dense_nodes, const uint8_t* mask, const int32_t* row_ptr,
                                    const int32_t* perm, const int64_t* node_index, const float* weight, int64_t nnz,
                                    int64_t G, int64_t max_len, int ops, void* out, int32_t* ties, int32_t* count,
                                    void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(h_dtype_ok(dtype), TGP_ERR_INVALID, "tgp_segment_aggr_h16: dtype is neither TGP_BF16 nor TGP_F16");
  TGP_REQUIRE(num_rows >= 0 && F >= 0 && G >= 0 && nnz >= 0 && max_len >= 0 && dense_nodes >= 0 && ldx >= F,
              TGP_ERR_INVALID, "tgp_segment_aggr_h16: negative size or a row stride below F");
  TGP_REQUIRE(ops != 0 && (ops & ~SH_OPS_ALL) == 0, TGP_ERR_INVALID,
              "tgp_segment_aggr_h16: ops must be a non-empty mask of sum, mean, min and max bits");
  const int n_src = (ptr ? 1 : 0) + (dense_nodes > 0 ? 1 : 0) + (node_index ? 1 : 0);
  TGP_REQUIRE(n_src == 1, TGP_ERR_INVALID,
              "tgp_segment_aggr_h16: exactly one row source (ptr, dense_nodes or node_index) must be given");
  TGP_REQUIRE(!mask || dense_nodes > 0, TGP_ERR_INVALID, "tgp_segment_aggr_h16: a mask needs the dense source");
  TGP_REQUIRE(node_index || (!row_ptr && !perm && !weight && nnz == 0), TGP_ERR_INVALID,
              "tgp_segment_aggr_h16: row_ptr, perm, weight and nnz belong to the gathered source");
  TGP_REQUIRE(!node_index || row_ptr || nnz == G, TGP_ERR_INVALID,
              "tgp_segment_aggr_h16: a gathered source without row_ptr has one assignment per group");
  TGP_REQUIRE(dense_nodes == 0 || G * dense_nodes == num_rows, TGP_ERR_INVALID,
              "tgp_segment_aggr_h16: the dense source has G * dense_nodes rows");
  TGP_REQUIRE(G < (1ll << 31) && nnz < (1ll << 31) && num_rows < (1ll << 31) &&
                  (F == 0 || num_rows <= ((1ll << 31) - 1) / F),
              TGP_ERR_RANGE, "tgp_segment_aggr_h16: G, N * F or nnz beyond the int32 range");
  if (G == 0 || F == 0) return TGP_OK;
  const int n_ops = h_popcount(ops), n_mm = h_popcount(ops & SH_OPS_MM);
  TGP_REQUIRE(G * n_ops <= ((1ll << 31) - 1) / F, TGP_ERR_RANGE, "tgp_segment_aggr_h16: the output exceeds 2^31 elements");
  TGP_REQUIRE(out && (num_rows == 0 || x), TGP_ERR_INVALID, "tgp_segment_aggr_h16: null pointer");
  int64_t chunk, n_chunks;
  sa_plan(G, F, max_len, &chunk, &n_chunks);  // the fp32 readout's cut: the same chunks, the same fold
  const size_t need = tgp_segment_aggr_workspace_bytes(G, F, ops, max_len);
  TGP_REQUIRE(n_chunks == 1 || (ws && ws_bytes >= need), TGP_ERR_WORKSPACE, "tgp_segment_aggr_h16: workspace too small");

  ShSrc s{static_cast<const uint16_t*>(x), num_rows, F, ldx, ptr, dense_nodes, mask, row_ptr, perm, node_index, weight, nnz};
  ShOut o{static_cast<uint16_t*>(out), (ops & SH_OPS_MM) ? ties : nullptr, count, ops, n_ops, n_mm, nullptr, nullptr};
  if (n_chunks > 1) {
    Carver cv(ws);
    o.part_cnt = cv.take<int32_t>(static_cast<size_t>(G * n_chunks));
    const int slots = ((ops & SH_OPS_SUMS) ? 1 : 0) + ((ops & SH_OPS_MM) ? 4 : 0);
    o.part = cv.take<float>(static_cast<size_t>(G * n_chunks) * slots * static_cast<size_t>(F));
  }
  const bool vec = F % 8 == 0 && ldx % 8 == 0 && h_aligned(x) && h_aligned(out) && h_aligned(o.ties) && h_aligned(o.part);
  const int64_t lanes = vec ? F / 8 : F;
  int lg_shift = 0;
  while ((1ll << lg_shift) < lanes && lg_shift < 8) ++lg_shift;
  const int64_t items = G * n_chunks, per_block = 256 >> lg_shift;
  const dim3 grid(static_cast<unsigned>((items + per_block - 1) / per_block),
                  static_cast<unsigned>((lanes + (1ll << lg_shift) - 1) >> lg_shift));
  TGP_REQUIRE(grid.y <= 65535u, TGP_ERR_RANGE, "tgp_segment_aggr_h16: F beyond the grid");
  if (dtype == TGP_BF16) h_segment_aggr<Bf16>(s, o, G, chunk, n_chunks, vec, grid, lg_shift, stream);
  else h_segment_aggr<Fp16>(s, o, G, chunk, n_chunks, vec, grid, lg_shift, stream);
  return check_launch("tgp_segment_aggr_h16");
}

extern "C" int tgp_segment_aggr_bwd_h16(int dtype, const void* g_out, const void* x, int64_t num_rows, int64_t F,
                                        int64_t ldx, const int64_t* batch, int64_t dense_nodes, const uint8_t* mask,
                                        const void* out, const int32_t* ties, const int32_t* count, int64_t G, int ops,
                                        void* dx, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(h_dtype_ok(dtype), TGP_ERR_INVALID, "tgp_segment_aggr_bwd_h16: dtype is neither TGP_BF16 nor TGP_F16");
  TGP_REQUIRE(num_rows >= 0 && F >= 0 && G >= 0 && dense_nodes >= 0 && ldx >= F, TGP_ERR_INVALID,
              "tgp_segment_aggr_bwd_h16: negative size or a row stride below F");
  TGP_REQUIRE(ops != 0 && (ops & ~SH_OPS_ALL) == 0, TGP_ERR_INVALID,
              "tgp_segment_aggr_bwd_h16: ops must be a non-empty mask of sum, mean, min and max bits");
  TGP_REQUIRE(!(batch && dense_nodes > 0) && (!mask || dense_nodes > 0), TGP_ERR_INVALID,
              "tgp_segment_aggr_bwd_h16: a batch vector or the dense layout, and a mask only with the latter");
  TGP_REQUIRE(dense_nodes == 0 || G * dense_nodes == num_rows, TGP_ERR_INVALID,
              "tgp_segment_aggr_bwd_h16: the dense source has G * dense_nodes rows");
  TGP_REQUIRE(G < (1ll << 31) && num_rows < (1ll << 31) && (F == 0 || num_rows <= ((1ll << 31) - 1) / F), TGP_ERR_RANGE,
              "tgp_segment_aggr_bwd_h16: G or N * F beyond the int32 range");
  if (num_rows == 0 || F == 0) return TGP_OK;
  TGP_REQUIRE(g_out && dx && (!(ops & SH_OPS_MM) || (x && out && ties)) && (!(ops & (1 << TGP_MEAN)) || count),
              TGP_ERR_INVALID, "tgp_segment_aggr_bwd_h16: null pointer (min / max need x, out and ties; mean needs count)");
  const int n_ops = h_popcount(ops), n_mm = h_popcount(ops & SH_OPS_MM);
  const bool vec = F % 8 == 0 && ldx % 8 == 0 && h_aligned(g_out) && h_aligned(x) && h_aligned(out) && h_aligned(dx);
  const dim3 grid = h_scalar_grid(num_rows * (vec ? F / 8 : F));
  const uint16_t *gs = static_cast<const uint16_t*>(g_out), *xs = static_cast<const uint16_t*>(x),
                 *os = static_cast<const uint16_t*>(out);
  uint16_t* ds = static_cast<uint16_t*>(dx);
#define TGP_SH_BWD(TT, VEC)                                                                                          \
  hipLaunchKernelGGL((segment_aggr_bwd_h16_kernel<TT, VEC>), grid, dim3(256), 0, stream, gs, xs, num_rows, F, ldx, batch, \
                     dense_nodes, mask, os, ties, count, G, ops, n_ops, n_mm, ds)
  if (dtype == TGP_BF16) {
    if (vec) TGP_SH_BWD(Bf16, 8);
    else TGP_SH_BWD(Bf16, 1);
  } else {
    if (vec) TGP_SH_BWD(Fp16, 8);
    else TGP_SH_BWD(Fp16, 1);
  }
#undef TGP_SH_BWD
  return check_launch("tgp_segment_aggr_bwd_h16");
}
