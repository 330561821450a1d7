// Segment readout: sum / mean / min / max of the rows of every group from ONE pass over X (reference
// reduce/aggr_reduce.py + global_reduce.py over PyG's Sum/Mean/Max/Min/MultiAggregation, i.e. scatter(reduce=...)).
//
// Row sources: contiguous segments of X named by a ptr (a sorted batch vector), a dense [B,N,F] block with an optional
// byte mask (masked rows are neither loaded nor counted), or gathered rows x[node_index[a]] * weight[a] through the
// supernode -> assignment index of a sparse SelectOutput (the product is rounded before the add, as in reduce_sparse).
//
// Work split.  A group of LG lanes (LG = the power of two covering F / VEC, at most one workgroup) owns one
// (segment, row chunk) item and every lane owns VEC adjacent features of it, so a lane adds its rows one after the
// other in ascending row order: the order of the sequential CPU scatter, the same bits on every call, no atomics.
//   - short segments: 256 / LG items per workgroup, written straight to the output;
//   - wide rows (F / VEC >= 256): one workgroup per (segment, 256 * VEC features);
//   - a batch whose longest segment exceeds SA_CHUNK rows: every segment is cut into row chunks, the items leave
//     partial records in the workspace and a second kernel folds them: runs of consecutive chunks in ascending order,
//     then the runs in ascending order (a fixed order too).
// Min / max are exact, NaN wins as in torch.amax / amin, and the same pass counts the rows that attain the extreme
// (`ties`), which is all the backward needs to split the gradient among them.
#include "common.h"

namespace tgp {

constexpr int SA_CHUNK = 256;       // rows a lane group adds in a row; a longer segment sends the batch to the split route
constexpr int SA_MAX_ITEMS = 8192;  // (segment, chunk) items of the split route: bounds its workspace and idle items
constexpr int SA_MIN_CHUNK = 16;    // ... and the shortest chunk the split route cuts when the batch has few segments
constexpr int SA_TARGET_LANES = 256 * 8 * 64;  // lanes that fill the device: 8 waves on each of 256 compute units
constexpr int SA_U = 8;             // rows a lane group has in flight

constexpr int SA_OPS_ALL = (1 << TGP_SUM) | (1 << TGP_MEAN) | (1 << TGP_MIN) | (1 << TGP_MAX);
constexpr int SA_OPS_SUMS = (1 << TGP_SUM) | (1 << TGP_MEAN);
constexpr int SA_OPS_MM = (1 << TGP_MIN) | (1 << TGP_MAX);

struct SaSrc {
  const float* x;
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

struct SaOut {
  float* out;       // [G, n_ops * F], operations in enum order
  int32_t* ties;    // [G, n_mm * F] (min, then max) or NULL
  int32_t* count;   // [G] or NULL
  int ops, n_ops, n_mm;
  float* part;        // split route: [items, slots, F]
  int32_t* part_cnt;  // split route: [items]
};

template <int VEC>
struct SaAcc {
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
__device__ __forceinline__ void sa_extent(const SaSrc& s, int64_t g, int64_t& beg, int64_t& len) {
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

template <bool SUMS, bool MM>
__device__ __forceinline__ void sa_add(float v, float& sum, float& mn, float& mx, int32_t& cmn, int32_t& cmx) {
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
__device__ __forceinline__ void sa_fold_extreme(float& m, int32_t& c, float pm, int32_t pc, bool is_max) {
  if (m != m) return;  // NaN stays
  if (pm != pm) {
    m = pm;
    return;
  }
  const bool better = is_max ? pm > m : pm < m;
  c = better ? pc : (pm == m ? c + pc : c);
  m = better ? pm : m;
}

template <int VEC>
__device__ __forceinline__ void sa_store(float* p, const float* v) {
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    p[0] = v[0];
  }
}
template <int VEC>
__device__ __forceinline__ void sa_store_i(int32_t* p, const int32_t* v) {
  if constexpr (VEC == 4) {
    *reinterpret_cast<int4*>(p) = make_int4(v[0], v[1], v[2], v[3]);
  } else {
    p[0] = v[0];
  }
}

// the finished group: empty groups give 0 for every operation, the mean divides by max(count, 1)
template <int VEC>
__device__ __forceinline__ void sa_emit(const SaOut& o, int64_t F, int64_t g, int64_t f, const SaAcc<VEC>& a) {
  float* row = o.out + g * (static_cast<int64_t>(o.n_ops) * F) + f;
  const float denom = static_cast<float>(a.cnt > 1 ? a.cnt : 1);
  const bool any = a.cnt > 0;
  float v[VEC];
  int slot = 0;
  if (o.ops & (1 << TGP_SUM)) {
    sa_store<VEC>(row + slot * F, a.sum);
    ++slot;
  }
  if (o.ops & (1 << TGP_MEAN)) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) v[j] = a.sum[j] / denom;
    sa_store<VEC>(row + slot * F, v);
    ++slot;
  }
  if (o.ops & (1 << TGP_MIN)) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) v[j] = any ? a.mn[j] : 0.f;
    sa_store<VEC>(row + slot * F, v);
    ++slot;
  }
  if (o.ops & (1 << TGP_MAX)) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) v[j] = any ? a.mx[j] : 0.f;
    sa_store<VEC>(row + slot * F, v);
    ++slot;
  }
  if (o.ties) {
    int32_t* trow = o.ties + g * (static_cast<int64_t>(o.n_mm) * F) + f;
    int j = 0;
    if (o.ops & (1 << TGP_MIN)) {
      sa_store_i<VEC>(trow + j * F, a.cmn);
      ++j;
    }
    if (o.ops & (1 << TGP_MAX)) sa_store_i<VEC>(trow + j * F, a.cmx);
  }
  if (o.count && f == 0) o.count[g] = a.cnt;
}

template <int VEC, bool SUMS, bool MM, bool GATHER>
__global__ __launch_bounds__(256) void segment_aggr_kernel(SaSrc s, SaOut o, int64_t G, int lg_shift, int64_t chunk,
                                                           int64_t n_chunks) {
  const int lg = 1 << lg_shift;
  const int lane = threadIdx.x & (lg - 1);
  const int64_t item = static_cast<int64_t>(blockIdx.x) * (256 >> lg_shift) + (threadIdx.x >> lg_shift);
  const int64_t f = (static_cast<int64_t>(blockIdx.y) * lg + lane) * VEC;
  if (item >= G * n_chunks || f >= s.F) return;
  const int64_t g = item / n_chunks, c = item - g * n_chunks;
  int64_t beg, len;
  sa_extent(s, g, beg, len);
  const int64_t r0 = c * chunk;
  if (c > 0 && r0 >= len) return;  // (the fold knows from len which chunks ran)
  const int64_t r1 = (c == n_chunks - 1 || r0 + chunk > len) ? len : r0 + chunk;

  SaAcc<VEC> a;
  a.init();
  for (int64_t r = r0; r < r1; r += SA_U) {
    bool on[SA_U];
    int64_t row[SA_U];
    float w[SA_U];
    float v[SA_U][VEC];
    if constexpr (GATHER) {  // position -> assignment -> (source row, weight), level by level, from clamped indices
      int64_t as[SA_U];
#pragma unroll
      for (int u = 0; u < SA_U; ++u) {
        on[u] = r + u < r1;
        const int64_t p = beg + (on[u] ? r + u : r);
        as[u] = s.perm ? static_cast<int64_t>(s.perm[p]) : p;
      }
#pragma unroll
      for (int u = 0; u < SA_U; ++u) {
        on[u] = on[u] && static_cast<uint64_t>(as[u]) < static_cast<uint64_t>(s.nnz);
        const int64_t ac = on[u] ? as[u] : 0;  // (nnz > 0 here: the loop runs only over existing positions)
        row[u] = s.node_index[ac];
        w[u] = s.weight ? s.weight[ac] : 1.0f;
      }
#pragma unroll
      for (int u = 0; u < SA_U; ++u) on[u] = on[u] && static_cast<uint64_t>(row[u]) < static_cast<uint64_t>(s.num_rows);
    } else {
#pragma unroll
      for (int u = 0; u < SA_U; ++u) {
        on[u] = r + u < r1;
        row[u] = beg + r + u;
        w[u] = 1.0f;
      }
      if (s.mask) {
#pragma unroll
        for (int u = 0; u < SA_U; ++u) on[u] = on[u] && s.mask[on[u] ? row[u] : beg] != 0;
      }
    }
#pragma unroll
    for (int u = 0; u < SA_U; ++u) {
      if (on[u]) {
        const float* src = s.x + row[u] * s.ld + f;
        if constexpr (VEC == 4) {
          const float4 t = *reinterpret_cast<const float4*>(src);
          v[u][0] = t.x, v[u][1] = t.y, v[u][2] = t.z, v[u][3] = t.w;
        } else {
          v[u][0] = src[0];
        }
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[u][j] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < SA_U; ++u) {
      if (on[u]) {
        ++a.cnt;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const float t = GATHER ? v[u][j] * w[u] : v[u][j];  // (no contraction: the product is rounded before the add)
          sa_add<SUMS, MM>(t, a.sum[j], a.mn[j], a.mx[j], a.cmn[j], a.cmx[j]);
        }
      }
    }
  }

  if (n_chunks == 1) {
    sa_emit<VEC>(o, s.F, g, f, a);
    return;
  }
  constexpr int SLOTS = (SUMS ? 1 : 0) + (MM ? 4 : 0);
  float* rec = o.part + item * (SLOTS * s.F) + f;
  int slot = 0;
  if constexpr (SUMS) {
    sa_store<VEC>(rec, a.sum);
    slot = 1;
  }
  if constexpr (MM) {
    sa_store<VEC>(rec + slot * s.F, a.mn);
    sa_store<VEC>(rec + (slot + 1) * s.F, a.mx);
    sa_store_i<VEC>(reinterpret_cast<int32_t*>(rec + (slot + 2) * s.F), a.cmn);
    sa_store_i<VEC>(reinterpret_cast<int32_t*>(rec + (slot + 3) * s.F), a.cmx);
  }
  if (f == 0) o.part_cnt[item] = a.cnt;
}

// split route, second kernel: one workgroup per (group, 4 features).  SA_FOLD_PARTS threads per feature each fold a
// contiguous run of the group's chunk records in ascending chunk order, then one thread folds the runs in ascending
// order: a fixed order, whatever the launch.
constexpr int SA_FOLD_PARTS = 64;

template <bool SUMS, bool MM>
__device__ __forceinline__ void sa_fold_record(SaAcc<1>& a, float sum, float mn, int32_t cmn, float mx, int32_t cmx) {
  if constexpr (SUMS) a.sum[0] = a.sum[0] + sum;
  if constexpr (MM) {
    sa_fold_extreme(a.mn[0], a.cmn[0], mn, cmn, false);
    sa_fold_extreme(a.mx[0], a.cmx[0], mx, cmx, true);
  }
}

template <bool SUMS, bool MM>
__global__ __launch_bounds__(256) void segment_aggr_fold_kernel(SaSrc s, SaOut o, int64_t G, int64_t chunk,
                                                                int64_t n_chunks) {
  constexpr int SLOTS = (SUMS ? 1 : 0) + (MM ? 4 : 0);
  __shared__ float sh_f[3][SA_FOLD_PARTS][4];
  __shared__ int32_t sh_i[3][SA_FOLD_PARTS][4];
  const int j = threadIdx.x & 3, p = threadIdx.x >> 2;
  const int64_t tiles = (s.F + 3) / 4;
  const int64_t g = blockIdx.x / tiles, f = (blockIdx.x - g * tiles) * 4 + j;
  int64_t beg, len;
  sa_extent(s, g, beg, len);
  int64_t n_run = (len + chunk - 1) / chunk;  // chunk 0 always ran; chunk c > 0 ran when c * chunk < len
  n_run = n_run < 1 ? 1 : (n_run > n_chunks ? n_chunks : n_run);
  const int64_t per = (n_run + SA_FOLD_PARTS - 1) / SA_FOLD_PARTS;
  const int64_t c0 = p * per, c1 = c0 + per < n_run ? c0 + per : n_run;
  SaAcc<1> a;
  a.init();
  if (f < s.F) {
    for (int64_t c = c0; c < c1; ++c) {
      const int64_t item = g * n_chunks + c;
      const float* rec = o.part + item * (SLOTS * s.F) + f;
      const int32_t* reci = reinterpret_cast<const int32_t*>(rec);
      a.cnt += o.part_cnt[item];
      constexpr int m0 = SUMS ? 1 : 0;
      sa_fold_record<SUMS, MM>(a, SUMS ? rec[0] : 0.f, MM ? rec[m0 * s.F] : 0.f, MM ? reci[(m0 + 2) * s.F] : 0,
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
    sa_fold_record<SUMS, MM>(a, sh_f[0][q][j], sh_f[1][q][j], sh_i[0][q][j], sh_f[2][q][j], sh_i[1][q][j]);
  }
  sa_emit<1>(o, s.F, g, f, a);
}

// dX[row, :] = sum over the requested operations of that operation's share of its group's upstream gradient
template <int VEC>
__global__ __launch_bounds__(256) void segment_aggr_bwd_kernel(const float* __restrict__ go, const float* __restrict__ x,
                                                               int64_t num_rows, int64_t F, int64_t ld,
                                                               const int64_t* __restrict__ batch, int64_t dense_nodes,
                                                               const uint8_t* __restrict__ mask,
                                                               const float* __restrict__ out,
                                                               const int32_t* __restrict__ ties,
                                                               const int32_t* __restrict__ count, int64_t G, int ops,
                                                               int n_ops, int n_mm, float* __restrict__ dx) {
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
      const float* grow = go + g * (static_cast<int64_t>(n_ops) * F) + f;
      int slot = 0, mm = 0;
      if (ops & (1 << TGP_SUM)) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] = acc[j] + grow[slot * F + j];
        ++slot;
      }
      if (ops & (1 << TGP_MEAN)) {
        const int32_t cnt = count[g];
        const float denom = static_cast<float>(cnt > 1 ? cnt : 1);
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] = acc[j] + grow[slot * F + j] / denom;
        ++slot;
      }
#pragma unroll
      for (int op = TGP_MIN; op <= TGP_MAX; ++op) {
        if (ops & (1 << op)) {
          const float* orow = out + g * (static_cast<int64_t>(n_ops) * F) + slot * F + f;
          const int32_t* trow = ties + g * (static_cast<int64_t>(n_mm) * F) + mm * F + f;
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            const float share = grow[slot * F + j] / static_cast<float>(trow[j] > 1 ? trow[j] : 1);
            acc[j] = acc[j] + (x[row * ld + f + j] == orow[j] ? share : 0.f);
          }
          ++slot;
          ++mm;
        }
      }
    }
    sa_store<VEC>(dx + row * F + f, acc);
  }
}

}  // namespace tgp

using namespace tgp;

static int sa_popcount(int v) { return __builtin_popcount(static_cast<unsigned>(v)); }

// rows per chunk and chunks per segment; n_chunks == 1: no workspace, the items write the output themselves.  The split
// route cuts finer than SA_CHUNK while the batch has fewer items than the device has lanes for (32 graphs of 1024 rows
// would otherwise be 128 lane groups), down to SA_MIN_CHUNK rows, and coarser when SA_MAX_ITEMS bounds the records.
static void sa_plan(int64_t G, int64_t F, int64_t max_len, int64_t* chunk, int64_t* n_chunks) {
  *chunk = max_len > 0 ? max_len : 1;
  *n_chunks = 1;
  if (max_len <= SA_CHUNK || G <= 0) return;
  const int64_t cap = SA_MAX_ITEMS / G;
  if (cap < 2) return;  // thousands of segments already fill the device
  const int64_t lanes = F % 4 == 0 ? F / 4 : F;
  int64_t lg = 1;
  while (lg < lanes && lg < 256) lg <<= 1;
  int64_t n = (SA_TARGET_LANES / lg + G - 1) / G;
  const int64_t lo = (max_len + SA_CHUNK - 1) / SA_CHUNK, hi = (max_len + SA_MIN_CHUNK - 1) / SA_MIN_CHUNK;
  n = n < lo ? lo : (n > hi ? hi : n);
  if (n > cap) n = cap;
  *chunk = (max_len + n - 1) / n;
  *n_chunks = (max_len + *chunk - 1) / *chunk;
}

static int sa_part_slots(int ops) { return ((ops & SA_OPS_SUMS) ? 1 : 0) + ((ops & SA_OPS_MM) ? 4 : 0); }

extern "C" int tgp_segment_aggr_chunk_rows(void) { return SA_CHUNK; }

extern "C" size_t tgp_segment_aggr_workspace_bytes(int64_t G, int64_t F, int ops, int64_t max_len) {
  int64_t chunk, n_chunks;
  sa_plan(G, F, max_len, &chunk, &n_chunks);
  if (n_chunks == 1 || F <= 0) return 0;
  const size_t items = static_cast<size_t>(G) * static_cast<size_t>(n_chunks);
  return align_up(items * sizeof(int32_t)) +
         align_up(items * static_cast<size_t>(sa_part_slots(ops)) * static_cast<size_t>(F) * sizeof(float));
}

extern "C" int tgp_segment_aggr_f32(const float* x, int64_t num_rows, int64_t F, int64_t ldx, const int64_t* ptr,
                                    int64_t dense_nodes, const uint8_t* mask, const int32_t* row_ptr,
                                    const int32_t* perm, const int64_t* node_index, const float* weight, int64_t nnz,
                                    int64_t G, int64_t max_len, int ops, float* out, int32_t* ties, int32_t* count,
                                    void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(num_rows >= 0 && F >= 0 && G >= 0 && nnz >= 0 && max_len >= 0 && dense_nodes >= 0 && ldx >= F,
              TGP_ERR_INVALID, "tgp_segment_aggr_f32: negative size or a row stride below F");
  TGP_REQUIRE(ops != 0 && (ops & ~SA_OPS_ALL) == 0, TGP_ERR_INVALID,
              "tgp_segment_aggr_f32: ops must be a non-empty mask of sum, mean, min and max bits");
  const int n_src = (ptr ? 1 : 0) + (dense_nodes > 0 ? 1 : 0) + (node_index ? 1 : 0);
  TGP_REQUIRE(n_src == 1, TGP_ERR_INVALID,
              "tgp_segment_aggr_f32: exactly one row source (ptr, dense_nodes or node_index) must be given");
  TGP_REQUIRE(!mask || dense_nodes > 0, TGP_ERR_INVALID, "tgp_segment_aggr_f32: a mask needs the dense source");
  TGP_REQUIRE(node_index || (!row_ptr && !perm && !weight && nnz == 0), TGP_ERR_INVALID,
              "tgp_segment_aggr_f32: row_ptr, perm, weight and nnz belong to the gathered source");
  TGP_REQUIRE(!node_index || row_ptr || nnz == G, TGP_ERR_INVALID,
              "tgp_segment_aggr_f32: a gathered source without row_ptr has one assignment per group");
  TGP_REQUIRE(dense_nodes == 0 || G * dense_nodes == num_rows, TGP_ERR_INVALID,
              "tgp_segment_aggr_f32: the dense source has G * dense_nodes rows");
  TGP_REQUIRE(G < (1ll << 31) && nnz < (1ll << 31) && num_rows < (1ll << 31) &&
                  (F == 0 || num_rows <= ((1ll << 31) - 1) / F),
              TGP_ERR_RANGE, "tgp_segment_aggr_f32: G, N * F or nnz beyond the int32 range");
  if (G == 0 || F == 0) return TGP_OK;
  const int n_ops = sa_popcount(ops), n_mm = sa_popcount(ops & SA_OPS_MM);
  TGP_REQUIRE(G * n_ops <= ((1ll << 31) - 1) / F, TGP_ERR_RANGE, "tgp_segment_aggr_f32: the output exceeds 2^31 elements");
  TGP_REQUIRE(out && (num_rows == 0 || x), TGP_ERR_INVALID, "tgp_segment_aggr_f32: null pointer");
  int64_t chunk, n_chunks;
  sa_plan(G, F, max_len, &chunk, &n_chunks);
  const size_t need = tgp_segment_aggr_workspace_bytes(G, F, ops, max_len);
  TGP_REQUIRE(n_chunks == 1 || (ws && ws_bytes >= need), TGP_ERR_WORKSPACE, "tgp_segment_aggr_f32: workspace too small");

  SaSrc s{x, num_rows, F, ldx, ptr, dense_nodes, mask, row_ptr, perm, node_index, weight, nnz};
  SaOut o{out, (ops & SA_OPS_MM) ? ties : nullptr, count, ops, n_ops, n_mm, nullptr, nullptr};
  if (n_chunks > 1) {
    Carver cv(ws);
    o.part_cnt = cv.take<int32_t>(static_cast<size_t>(G * n_chunks));
    o.part = cv.take<float>(static_cast<size_t>(G * n_chunks) * sa_part_slots(ops) * static_cast<size_t>(F));
  }
  const auto aligned = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
  const bool vec = F % 4 == 0 && ldx % 4 == 0 && aligned(x) && aligned(out) && aligned(o.ties) && aligned(o.part);
  const int64_t lanes = vec ? F / 4 : F;
  int lg_shift = 0;
  while ((1ll << lg_shift) < lanes && lg_shift < 8) ++lg_shift;
  const int64_t items = G * n_chunks, per_block = 256 >> lg_shift;
  const dim3 grid(static_cast<unsigned>((items + per_block - 1) / per_block),
                  static_cast<unsigned>((lanes + (1ll << lg_shift) - 1) >> lg_shift));
  TGP_REQUIRE(grid.y <= 65535u, TGP_ERR_RANGE, "tgp_segment_aggr_f32: F beyond the grid");
  const bool sums = (ops & SA_OPS_SUMS) != 0, mm = (ops & SA_OPS_MM) != 0, gather = node_index != nullptr;
#define TGP_SA_LAUNCH(VEC, SUMS, MM, GATHER)                                                                          \
  hipLaunchKernelGGL((segment_aggr_kernel<VEC, SUMS, MM, GATHER>), grid, dim3(256), 0, stream, s, o, G, lg_shift, chunk, \
                     n_chunks)
#define TGP_SA_SOURCE(VEC, SUMS, MM)       \
  do {                                     \
    if (gather) TGP_SA_LAUNCH(VEC, SUMS, MM, true); \
    else TGP_SA_LAUNCH(VEC, SUMS, MM, false);       \
  } while (0)
#define TGP_SA_OPS(VEC)                                   \
  do {                                                    \
    if (sums && mm) TGP_SA_SOURCE(VEC, true, true);       \
    else if (sums) TGP_SA_SOURCE(VEC, true, false);       \
    else TGP_SA_SOURCE(VEC, false, true);                 \
  } while (0)
  if (vec) TGP_SA_OPS(4);
  else TGP_SA_OPS(1);
#undef TGP_SA_OPS
#undef TGP_SA_SOURCE
#undef TGP_SA_LAUNCH
  if (n_chunks > 1) {
    const dim3 fgrid(static_cast<unsigned>(G * ((F + 3) / 4)));  // (G <= SA_MAX_ITEMS / 2 here, F < 2^18: grid.y bound)
    if (sums && mm)
      hipLaunchKernelGGL((segment_aggr_fold_kernel<true, true>), fgrid, dim3(256), 0, stream, s, o, G, chunk, n_chunks);
    else if (sums)
      hipLaunchKernelGGL((segment_aggr_fold_kernel<true, false>), fgrid, dim3(256), 0, stream, s, o, G, chunk, n_chunks);
    else
      hipLaunchKernelGGL((segment_aggr_fold_kernel<false, true>), fgrid, dim3(256), 0, stream, s, o, G, chunk, n_chunks);
  }
  return check_launch("tgp_segment_aggr_f32");
}

extern "C" int tgp_segment_aggr_bwd_f32(const float* g_out, const float* x, int64_t num_rows, int64_t F, int64_t ldx,
                                        const int64_t* batch, int64_t dense_nodes, const uint8_t* mask,
                                        const float* out, const int32_t* ties, const int32_t* count, int64_t G, int ops,
                                        float* dx, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(num_rows >= 0 && F >= 0 && G >= 0 && dense_nodes >= 0 && ldx >= F, TGP_ERR_INVALID,
              "tgp_segment_aggr_bwd_f32: negative size or a row stride below F");
  TGP_REQUIRE(ops != 0 && (ops & ~SA_OPS_ALL) == 0, TGP_ERR_INVALID,
              "tgp_segment_aggr_bwd_f32: ops must be a non-empty mask of sum, mean, min and max bits");
  TGP_REQUIRE(!(batch && dense_nodes > 0) && (!mask || dense_nodes > 0), TGP_ERR_INVALID,
              "tgp_segment_aggr_bwd_f32: a batch vector or the dense layout, and a mask only with the latter");
  TGP_REQUIRE(dense_nodes == 0 || G * dense_nodes == num_rows, TGP_ERR_INVALID,
              "tgp_segment_aggr_bwd_f32: the dense source has G * dense_nodes rows");
  TGP_REQUIRE(G < (1ll << 31) && num_rows < (1ll << 31) && (F == 0 || num_rows <= ((1ll << 31) - 1) / F), TGP_ERR_RANGE,
              "tgp_segment_aggr_bwd_f32: G or N * F beyond the int32 range");
  if (num_rows == 0 || F == 0) return TGP_OK;
  TGP_REQUIRE(g_out && dx && (!(ops & SA_OPS_MM) || (x && out && ties)) && (!(ops & (1 << TGP_MEAN)) || count),
              TGP_ERR_INVALID, "tgp_segment_aggr_bwd_f32: null pointer (min / max need x, out and ties; mean needs count)");
  const int n_ops = sa_popcount(ops), n_mm = sa_popcount(ops & SA_OPS_MM);
  const auto aligned = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
  const bool vec = F % 4 == 0 && aligned(dx);  // (the inputs are read by scalar loads the compiler may widen)
  const int64_t total = num_rows * (vec ? F / 4 : F);
  int64_t blocks = (total + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;
  const dim3 grid(static_cast<unsigned>(blocks));
  if (vec)
    hipLaunchKernelGGL(segment_aggr_bwd_kernel<4>, grid, dim3(256), 0, stream, g_out, x, num_rows, F, ldx, batch,
                       dense_nodes, mask, out, ties, count, G, ops, n_ops, n_mm, dx);
  else
    hipLaunchKernelGGL(segment_aggr_bwd_kernel<1>, grid, dim3(256), 0, stream, g_out, x, num_rows, F, ldx, batch,
                       dense_nodes, mask, out, ties, count, G, ops, n_ops, n_mm, dx);
  return check_launch("tgp_segment_aggr_bwd_f32");
}
