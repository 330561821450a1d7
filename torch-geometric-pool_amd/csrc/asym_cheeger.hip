// AsymCheegerCut's auxiliary losses (reference poolers/asym_cheeger_cut.py, utils/losses.py:503-550, 780-1010):
//
//   totvar[b]  = sum_ij a_ij ||s_i - s_j||_1 / (2 E_b)            E_b = nonzeros of adj[b] (dense form) or the edges whose
//                                                                  source lies in graph b (edge form), clamped to >= 1
//   balance[b] = (n (k-1) - sum_ik rho(s_ik - q_k)) / (n (k-1))   q_k = the idx-th largest entry of column k among the n
//                                                                  real nodes, idx = min(floor(n / k), n - 1);
//                                                                  rho(d) = (k-1) d for d >= 0, -d for d < 0
//
// Neither is a matrix product.  The total variation walks the nonzeros of A (a ballot over the loaded values lets a wave
// skip empty chunks); the quantile is selected without sorting (rank by counting for small graphs, an 8-bit radix select
// otherwise) on unsigned keys whose order is the float order.  No float atomics: every sum has a fixed order, so two calls
// on the same inputs return the same bits.  Where several nodes hold the quantile value, the LOWEST node index is the one
// reported (and the one that receives the quantile's gradient).
#include "loss_common.h"

namespace tgp {
namespace {

constexpr int AC_SMALL_NODES = 128;  // graphs up to this many rows: the counting select, the graph's columns in LDS
constexpr int AC_COLS = 32;          // columns of S per pass / workgroup of the select kernels
constexpr int AC_RG = 8;             // row groups of a 256-thread workgroup over AC_COLS columns
constexpr int AC_TV_ROWS = 16;       // rows of A per workgroup of the dense forward (4 per wave)
constexpr int AC_BWD_ROWS = 32;      // rows of dS per workgroup of the dense backward (8 per wave)

// unsigned key with the order of the floats: -0 and +0 are one value, NaN is the largest (as a descending sort has it)
__device__ __forceinline__ uint32_t ac_key(float v) {
  if (v != v) return 0xFFFFFFFFu;
  if (v == 0.0f) v = 0.0f;
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ac_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

__device__ __forceinline__ float ac_sign(float d) { return static_cast<float>((d > 0.f) - (d < 0.f)); }

// ------------------------------------------------------------------------------------------------ dense total variation
// One workgroup per (16 rows, graph); a wave owns 4 rows and walks them 256 columns at a time.  VEC: lane l holds columns
// j0 + 4 l .. + 3 (one 16-byte load per row), else columns j0 + 64 q + l.  part[b][rb] = sum over the block's nonzeros of
// a_ij ||s_i - s_j||_1, cnt[b][rb] = its nonzeros.  Rows and columns beyond the graph's size are not read.
template <bool VEC>
__global__ __launch_bounds__(256) void acc_tv_dense_kernel(const float* __restrict__ A, const float* __restrict__ S, int N,
                                                           int K, const int64_t* __restrict__ sizes, int nrb,
                                                           float* __restrict__ part, int* __restrict__ cnt_out) {
  __shared__ float sh[4];
  __shared__ long long shc[4];
  const int b = blockIdx.y, rb = blockIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int64_t start;
  int count;
  graph_rows(b, N, sizes, nullptr, start, count);
  const float* Ab = A + static_cast<int64_t>(b) * N * N;
  const float* Sb = S + start * K;
  const int i0 = rb * AC_TV_ROWS + w * 4;
  float acc = 0.f;
  long long cnt = 0;
  if (i0 < count) {
    for (int j0 = 0; j0 < count; j0 += 256) {
      float a[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + r;
        if (VEC) {
          const int j = j0 + 4 * lane;
          f32x4 v = {0.f, 0.f, 0.f, 0.f};
          if (i < count && j < count)  // (N % 4 == 0: the four columns are inside the row)
            v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(Ab + static_cast<int64_t>(i) * N + j));
          a[r][0] = v.x;
          a[r][1] = j + 1 < count ? v.y : 0.f;
          a[r][2] = j + 2 < count ? v.z : 0.f;
          a[r][3] = j + 3 < count ? v.w : 0.f;
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int j = j0 + 64 * q + lane;
            a[r][q] = (i < count && j < count) ? __builtin_nontemporal_load(Ab + static_cast<int64_t>(i) * N + j) : 0.f;
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* Si = Sb + static_cast<int64_t>(i0 + r) * K;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const unsigned long long nz = __ballot(a[r][q] != 0.f);
          if (!nz) continue;  // (uniform over the wave)
          cnt += __popcll(nz);
          for (int k0 = 0; k0 < K; k0 += 256) {
            float si[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) si[t] = k0 + 64 * t + lane < K ? Si[k0 + 64 * t + lane] : 0.f;
            unsigned long long m = nz;
            while (m) {
              const int l = __ffsll(static_cast<long long>(m)) - 1;
              m &= m - 1;
              const float aj = __shfl(a[r][q], l, 64);
              const int j = VEC ? j0 + 4 * l + q : j0 + 64 * q + l;
              const float* Sj = Sb + static_cast<int64_t>(j) * K;
#pragma unroll
              for (int t = 0; t < 4; ++t) {
                const int k = k0 + 64 * t + lane;
                if (k < K) acc = fmaf(aj, fabsf(si[t] - Sj[k]), acc);
              }
            }
          }
        }
      }
    }
  }
  const float total = block_fold_pair256<true>(acc, sh, op_add{});
  const long long c = block_fold_seq<256, true>(lane == 0 ? cnt : 0, shc);
  if (threadIdx.x == 0) {
    part[static_cast<int64_t>(b) * nrb + rb] = total;
    cnt_out[static_cast<int64_t>(b) * nrb + rb] = static_cast<int>(c);
  }
}

// dS[b,i,:] = scale_b sum_j (a_ij + a_ji) sign(s_i - s_j), scale_b = g_b c_tv / (2 E_b).  One workgroup per (32 rows i,
// graph): row i of A is read as it lies, column i through a transposed 64 x 32 tile in LDS (128-byte row segments), both
// 64 columns j at a time, so that lane l of the wave that owns row i holds a_ij + a_ji for j = j0 + l.  The sum over j runs
// in ascending j per lane-owned k.  Every row of the padded batch is written (0 beyond the graph's size).
__global__ __launch_bounds__(256) void acc_tv_dense_bwd_kernel(const float* __restrict__ A, const float* __restrict__ S,
                                                               int N, int K, const int64_t* __restrict__ sizes,
                                                               const float* __restrict__ g, const int* __restrict__ ecnt,
                                                               float c_tv, float* __restrict__ dS) {
  __shared__ float tile[64][AC_BWD_ROWS + 1];
  const int b = blockIdx.y, i0 = blockIdx.x * AC_BWD_ROWS;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int64_t start;
  int count;
  graph_rows(b, N, sizes, nullptr, start, count);
  const float* Ab = A + static_cast<int64_t>(b) * N * N;
  const float* Sb = S + start * K;
  const int e = ecnt[b] > 1 ? ecnt[b] : 1;
  const float scale = g[b] * c_tv / (2.0f * static_cast<float>(e));
  for (int k0 = 0; k0 < K; k0 += 256) {
    float acc[8][4];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[r][t] = 0.f;
    if (i0 < count) {  // (uniform over the workgroup)
      for (int j0 = 0; j0 < count; j0 += 64) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int jj = (threadIdx.x >> 5) + 8 * u, ii = threadIdx.x & 31;
          const int j = j0 + jj, i = i0 + ii;
          tile[jj][ii] = (j < count && i < count) ? Ab[static_cast<int64_t>(j) * N + i] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const int i = i0 + w * 8 + r;
          const int j = j0 + lane;
          const float a_row = (i < count && j < count) ? Ab[static_cast<int64_t>(i) * N + j] : 0.f;
          const float a = a_row + tile[lane][w * 8 + r];
          const unsigned long long nz = __ballot(a != 0.f);
          if (!nz) continue;
          const float* Si = Sb + static_cast<int64_t>(i) * K;
          float si[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) si[t] = k0 + 64 * t + lane < K ? Si[k0 + 64 * t + lane] : 0.f;
          unsigned long long m = nz;
          while (m) {
            const int l = __ffsll(static_cast<long long>(m)) - 1;
            m &= m - 1;
            const float aj = __shfl(a, l, 64);
            const float* Sj = Sb + static_cast<int64_t>(j0 + l) * K;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              const int k = k0 + 64 * t + lane;
              if (k < K) acc[r][t] = fmaf(aj, ac_sign(si[t] - Sj[k]), acc[r][t]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int i = i0 + w * 8 + r;
      if (i >= N) continue;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int k = k0 + 64 * t + lane;
        if (k < K) dS[(static_cast<int64_t>(b) * N + i) * K + k] = scale * acc[r][t];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------- edge total variation
// One wave per node i: node_tv[i] = sum over the out-edges e of i (by-source index, edge-list order) of
// w_e ||s_i - s_dst(e)||_1.
__global__ __launch_bounds__(256) void acc_tv_edge_kernel(const float* __restrict__ S, int64_t nodes, int K,
                                                          const int64_t* __restrict__ col, const float* __restrict__ w,
                                                          const int* __restrict__ src_ptr,
                                                          const int* __restrict__ src_perm,
                                                          float* __restrict__ node_tv) {
  const int lane = threadIdx.x & 63;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (i >= nodes) return;
  const float* Si = S + i * K;
  float acc = 0.f;
  for (int p = src_ptr[i]; p < src_ptr[i + 1]; ++p) {
    const int e = src_perm[p];
    const int64_t j = col[e];
    if (j < 0 || j >= nodes) continue;
    const float we = w ? w[e] : 1.f;
    const float* Sj = S + j * K;
    for (int k = lane; k < K; k += 64) acc = fmaf(we, fabsf(Si[k] - Sj[k]), acc);
  }
  // the order of wave_sum (wave.h), written out: a call here changes the kernel's instruction stream
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) node_tv[i] = acc;
}

// One wave per node i: dS[i,:] = sum over out-edges of w_e sc(b(i)) sign(s_i - s_dst) + sum over in-edges (by-destination
// index) of w_e sc(b(src)) sign(s_i - s_src), sc(b) = g_b c_tv / (2 E_b): an edge belongs to the graph of its source.
__global__ __launch_bounds__(256) void acc_tv_edge_bwd_kernel(
    const float* __restrict__ S, int64_t nodes, int K, const int64_t* __restrict__ row, const int64_t* __restrict__ col,
    const float* __restrict__ w, const int* __restrict__ src_ptr, const int* __restrict__ src_perm,
    const int* __restrict__ dst_ptr, const int* __restrict__ dst_perm, const int64_t* __restrict__ batch,
    const float* __restrict__ g, const int* __restrict__ ecnt, float c_tv, int B, float* __restrict__ dS) {
  const int lane = threadIdx.x & 63;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (i >= nodes) return;
  const float* Si = S + i * K;
  const int64_t bi = batch ? batch[i] : 0;
  float sc_i = 0.f;
  if (bi >= 0 && bi < B) sc_i = g[bi] * c_tv / (2.0f * static_cast<float>(ecnt[bi] > 1 ? ecnt[bi] : 1));
  for (int k0 = 0; k0 < K; k0 += 256) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, si[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) si[t] = k0 + 64 * t + lane < K ? Si[k0 + 64 * t + lane] : 0.f;
    for (int p = src_ptr[i]; p < src_ptr[i + 1]; ++p) {
      const int e = src_perm[p];
      const int64_t j = col[e];
      if (j < 0 || j >= nodes) continue;
      const float c = (w ? w[e] : 1.f) * sc_i;
      const float* Sj = S + j * K;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int k = k0 + 64 * t + lane;
        if (k < K) acc[t] = fmaf(c, ac_sign(si[t] - Sj[k]), acc[t]);
      }
    }
    for (int p = dst_ptr[i]; p < dst_ptr[i + 1]; ++p) {
      const int e = dst_perm[p];
      const int64_t j = row[e];
      if (j < 0 || j >= nodes) continue;
      const int64_t bj = batch ? batch[j] : 0;
      if (bj < 0 || bj >= B) continue;
      const float c = (w ? w[e] : 1.f) * (g[bj] * c_tv / (2.0f * static_cast<float>(ecnt[bj] > 1 ? ecnt[bj] : 1)));
      const float* Sj = S + j * K;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int k = k0 + 64 * t + lane;
        if (k < K) acc[t] = fmaf(c, ac_sign(si[t] - Sj[k]), acc[t]);
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int k = k0 + 64 * t + lane;
      if (k < K) dS[i * K + k] = acc[t];
    }
  }
}

// ------------------------------------------------------------------------------------------------------ quantile select
// What both select kernels leave per (graph, column): q = the idx-th largest entry among the graph's real rows, qnode =
// the lowest row (relative to the graph's first) that holds it, colsum = sum_i rho(s_ik - q_k), cge = rows with
// s_ik >= q_k; per graph nreal = its real rows.  A graph without real rows (or kq <= 1): q = 0, qnode = -1, sums 0.
__device__ __forceinline__ int ac_real_rows(int count, const uint8_t* mask, int64_t start, int* sh_n) {
  if (!mask) return count;
  if (threadIdx.x == 0) *sh_n = 0;
  __syncthreads();
  int c = 0;
  for (int i = threadIdx.x; i < count; i += 256) c += mask[start + i] ? 1 : 0;
  if (c) atomicAdd(sh_n, c);
  __syncthreads();
  return *sh_n;
}

__device__ __forceinline__ float ac_rho(float d, float km1) { return d >= 0.f ? km1 * d : -d; }

// rank by counting: one workgroup per graph of at most AC_SMALL_NODES rows, 32 columns at a time in LDS
__global__ __launch_bounds__(256) void acc_select_count_kernel(const float* __restrict__ S, int N, int K,
                                                               const int64_t* __restrict__ sizes,
                                                               const uint8_t* __restrict__ mask,
                                                               const int64_t* __restrict__ ptr, int kq,
                                                               float* __restrict__ q_out, int* __restrict__ qnode_out,
                                                               float* __restrict__ colsum, int* __restrict__ cge_out,
                                                               int* __restrict__ nreal) {
  __shared__ float sv[AC_SMALL_NODES][AC_COLS + 1];
  __shared__ uint8_t real[AC_SMALL_NODES];
  __shared__ int qn[AC_COLS];
  __shared__ float sh_sum[AC_RG][AC_COLS];
  __shared__ int sh_ge[AC_RG][AC_COLS];
  __shared__ int sh_n;
  const int b = blockIdx.x;
  const int c = threadIdx.x & (AC_COLS - 1), rg = threadIdx.x / AC_COLS;
  int64_t start;
  int count;
  graph_rows(b, N, sizes, ptr, start, count);
  if (count > AC_SMALL_NODES) count = AC_SMALL_NODES;  // (the host checks; never index LDS beyond the tile)
  const int n = ac_real_rows(count, mask, start, &sh_n);
  if (threadIdx.x < AC_SMALL_NODES)
    real[threadIdx.x] = threadIdx.x < count && (!mask || mask[start + threadIdx.x]) ? 1 : 0;
  if (threadIdx.x == 0) nreal[b] = n;
  const int idx = n > 0 ? (n / (kq > 1 ? kq : 1) < n - 1 ? n / (kq > 1 ? kq : 1) : n - 1) : 0;
  const float km1 = static_cast<float>(kq - 1);
  for (int kc = 0; kc < K; kc += AC_COLS) {
    const int k = kc + c;
    __syncthreads();
    if (threadIdx.x < AC_COLS) qn[threadIdx.x] = 0x7FFFFFFF;
    for (int i = rg; i < count; i += AC_RG) sv[i][c] = k < K ? S[(start + i) * K + k] : 0.f;
    __syncthreads();
    if (n > 0 && kq > 1) {
      for (int i = rg; i < count; i += AC_RG) {
        if (!real[i]) continue;
        const uint32_t ki = ac_key(sv[i][c]);
        int gt = 0, eq = 0;
        for (int j = 0; j < count; ++j) {
          const uint32_t kj = ac_key(sv[j][c]);
          gt += (real[j] && kj > ki) ? 1 : 0;
          eq += (real[j] && kj == ki) ? 1 : 0;
        }
        if (gt <= idx && idx < gt + eq) atomicMin(&qn[c], i);
      }
    }
    __syncthreads();
    const int node = qn[c];
    const bool have = node != 0x7FFFFFFF;
    const float q = have ? sv[node][c] : 0.f;
    float sum = 0.f;
    int ge = 0;
    if (have) {
      for (int i = rg; i < count; i += AC_RG) {
        if (!real[i]) continue;
        const float d = sv[i][c] - q;
        sum += ac_rho(d, km1);
        ge += d >= 0.f ? 1 : 0;
      }
    }
    sh_sum[rg][c] = sum;
    sh_ge[rg][c] = ge;
    __syncthreads();
    if (rg == 0 && k < K) {
      float t = 0.f;
      int g = 0;
#pragma unroll
      for (int r = 0; r < AC_RG; ++r) {
        t += sh_sum[r][c];
        g += sh_ge[r][c];
      }
      const int64_t o = static_cast<int64_t>(b) * K + k;
      q_out[o] = q;
      qnode_out[o] = have ? node : -1;
      colsum[o] = t;
      cge_out[o] = g;
    }
  }
}

// radix select, 8 bits per pass: one workgroup per (32 columns, graph); a lane per column so that the reads of a row
// coalesce, 8 row groups; histograms [256 bins][32 columns] in LDS filled with integer LDS atomics.  Four passes fix the
// key of the idx-th largest entry, a fifth finds the lowest row that holds it and forms the column sums.
__global__ __launch_bounds__(256) void acc_select_radix_kernel(const float* __restrict__ S, int N, int K,
                                                               const int64_t* __restrict__ sizes,
                                                               const uint8_t* __restrict__ mask,
                                                               const int64_t* __restrict__ ptr, int kq,
                                                               float* __restrict__ q_out, int* __restrict__ qnode_out,
                                                               float* __restrict__ colsum, int* __restrict__ cge_out,
                                                               int* __restrict__ nreal) {
  __shared__ unsigned hist[256][AC_COLS];
  __shared__ unsigned gsum[AC_RG][AC_COLS];
  __shared__ unsigned sel_prefix[AC_COLS];
  __shared__ unsigned sel_rank[AC_COLS];
  __shared__ int qn[AC_COLS];
  __shared__ float sh_sum[AC_RG][AC_COLS];
  __shared__ int sh_ge[AC_RG][AC_COLS];
  __shared__ int sh_n;
  const int b = blockIdx.y;
  const int c = threadIdx.x & (AC_COLS - 1), rg = threadIdx.x / AC_COLS;
  const int k = blockIdx.x * AC_COLS + c;
  int64_t start;
  int count;
  graph_rows(b, N, sizes, ptr, start, count);
  const int n = ac_real_rows(count, mask, start, &sh_n);
  if (threadIdx.x == 0 && blockIdx.x == 0) nreal[b] = n;
  const int64_t o = static_cast<int64_t>(b) * K + k;
  if (n <= 0 || kq <= 1) {  // (uniform over the workgroup)
    if (rg == 0 && k < K) {
      q_out[o] = 0.f;
      qnode_out[o] = -1;
      colsum[o] = 0.f;
      cge_out[o] = 0;
    }
    return;
  }
  const int idx = n / kq < n - 1 ? n / kq : n - 1;
  const float km1 = static_cast<float>(kq - 1);
  const float* Sc = S + start * K + k;
  const uint8_t* mk = mask ? mask + start : nullptr;
  if (rg == 0) {
    sel_prefix[c] = 0u;
    sel_rank[c] = static_cast<unsigned>(idx);
    qn[c] = 0x7FFFFFFF;
  }
  unsigned prefix = 0u;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int t = threadIdx.x; t < 256 * AC_COLS; t += 256) (&hist[0][0])[t] = 0u;
    __syncthreads();
    if (k < K) {
      for (int i = rg; i < count; i += AC_RG) {
        if (mk && !mk[i]) continue;
        const uint32_t key = ac_key(Sc[static_cast<int64_t>(i) * K]);
        if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255u][c], 1u);
      }
    }
    __syncthreads();
    {
      unsigned t = 0u;
#pragma unroll 8
      for (int u = 0; u < 32; ++u) t += hist[rg * 32 + u][c];
      gsum[rg][c] = t;
    }
    __syncthreads();
    if (rg == 0) {  // descending: walk the bins from the top until the rank falls inside one
      unsigned r = sel_rank[c];
      int grp = AC_RG - 1;
      while (grp > 0 && r >= gsum[grp][c]) {
        r -= gsum[grp][c];
        --grp;
      }
      int bin = grp * 32 + 31;
      while (bin > grp * 32 && r >= hist[bin][c]) {
        r -= hist[bin][c];
        --bin;
      }
      sel_rank[c] = r;
      sel_prefix[c] = prefix | (static_cast<unsigned>(bin) << shift);
    }
    __syncthreads();
    prefix = sel_prefix[c];
  }
  const float q = ac_unkey(prefix);
  float sum = 0.f;
  int ge = 0, first = 0x7FFFFFFF;
  if (k < K) {
    for (int i = rg; i < count; i += AC_RG) {
      if (mk && !mk[i]) continue;
      const float s = Sc[static_cast<int64_t>(i) * K];
      if (first == 0x7FFFFFFF && ac_key(s) == prefix) first = i;
      const float d = s - q;
      sum += ac_rho(d, km1);
      ge += d >= 0.f ? 1 : 0;
    }
  }
  if (first != 0x7FFFFFFF) atomicMin(&qn[c], first);
  sh_sum[rg][c] = sum;
  sh_ge[rg][c] = ge;
  __syncthreads();
  if (rg == 0 && k < K) {
    float t = 0.f;
    int g = 0;
#pragma unroll
    for (int r = 0; r < AC_RG; ++r) {
      t += sh_sum[r][c];
      g += sh_ge[r][c];
    }
    const int node = qn[c];
    const bool have = node != 0x7FFFFFFF;
    q_out[o] = have ? Sc[static_cast<int64_t>(node) * K] : q;  // (the node's own bits)
    qnode_out[o] = have ? node : -1;
    colsum[o] = t;
    cge_out[o] = g;
  }
}

// ------------------------------------------------------------------------------------------------------------- the tail
// One workgroup per graph: out[0][b] = c_tv tv_b / (2 E_b), out[1][b] = c_bal (n (k-1) - sum_k colsum) / (n (k-1)); ecnt[b]
// = E_b for the backward.  tv values of graph b: tv[b nrb .. (b+1) nrb) with their counts in cnt (dense form) or
// tv[ptr[b] .. ptr[b+1]) with E_b = src_ptr[ptr[b+1]] - src_ptr[ptr[b]] (edge form), added in a fixed order.
__global__ __launch_bounds__(256) void acc_tail_kernel(const float* __restrict__ tv, const int* __restrict__ cnt,
                                                       const int* __restrict__ src_ptr, const int64_t* __restrict__ ptr,
                                                       int nrb, const float* __restrict__ colsum,
                                                       const int* __restrict__ nreal, int K, int kq, float c_tv,
                                                       float c_bal, int B, float* __restrict__ out,
                                                       int* __restrict__ ecnt) {
  __shared__ float sh[4];
  __shared__ long long shc[4];
  const int b = blockIdx.x;
  float t = 0.f, a = 0.f;
  long long e = 0;
  if (tv) {
    const int64_t lo = src_ptr ? ptr[b] : static_cast<int64_t>(b) * nrb;
    const int64_t hi = src_ptr ? ptr[b + 1] : lo + nrb;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
      t += tv[i];
      if (cnt) e += cnt[i];
    }
    t = block_fold_pair256<true>(t, sh, op_add{});
    e = src_ptr ? static_cast<long long>(src_ptr[hi]) - src_ptr[lo] : block_fold_seq<256, true>(e, shc);
  }
  if (colsum) {
    for (int k = threadIdx.x; k < K; k += 256) a += colsum[static_cast<int64_t>(b) * K + k];
    a = block_fold_pair256<true>(a, sh, op_add{});
  }
  if (threadIdx.x == 0) {
    const long long e1 = e > 1 ? e : 1;
    out[b] = tv ? c_tv * (t / (2.0f * static_cast<float>(e1))) : 0.f;
    float bal = 0.f;
    if (colsum && kq > 1 && nreal[b] > 0) {
      const float beta = static_cast<float>(nreal[b]) * static_cast<float>(kq - 1);
      bal = (beta - a) / beta;
    }
    out[B + b] = c_bal * bal;
    if (ecnt) ecnt[b] = static_cast<int>(e1 < 0x7FFFFFFF ? e1 : 0x7FFFFFFF);
  }
}

// dS[row,k] (+)= -g_b rho'(s - q_k) / (n (k-1)), plus the column's total + g_b sum_i rho'(d_ik) / (n (k-1)) on the quantile
// node; rho'(d) = k-1 for d >= 0, -1 for d < 0; rows that are not real get 0.
__global__ __launch_bounds__(256) void acc_asym_bwd_kernel(const float* __restrict__ S, int64_t rows, int N, int K,
                                                           const int64_t* __restrict__ batch,
                                                           const int64_t* __restrict__ ptr,
                                                           const int64_t* __restrict__ sizes,
                                                           const uint8_t* __restrict__ mask, const float* __restrict__ q,
                                                           const int* __restrict__ qnode, const int* __restrict__ cge,
                                                           const int* __restrict__ nreal, const float* __restrict__ g,
                                                           float c_bal, int kq, int B, int accumulate,
                                                           float* __restrict__ dS) {
  const int64_t total = rows * K;
  for (int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; idx < total; idx += 256ll * gridDim.x) {
    const int64_t row = idx / K;
    const int k = static_cast<int>(idx - row * K);
    const int64_t b = ptr ? (batch ? batch[row] : 0) : row / N;
    float v = 0.f;
    if (b >= 0 && b < B && kq > 1 && nreal[b] > 0) {
      int64_t start;
      int count;
      graph_rows(static_cast<int>(b), N, sizes, ptr, start, count);
      const int64_t i = row - start;
      if (i >= 0 && i < count && (!mask || mask[row])) {
        const float n = static_cast<float>(nreal[b]);
        const float km1 = static_cast<float>(kq - 1);
        const float beta = n * km1;
        const float gb = g[b] * c_bal;
        const int64_t o = b * K + k;
        v = -gb * (S[idx] - q[o] >= 0.f ? km1 : -1.f) / beta;
        if (i == qnode[o]) {
          const float ge = static_cast<float>(cge[o]);
          v += gb * (km1 * ge - (n - ge)) / beta;
        }
      }
    }
    dS[idx] = accumulate ? dS[idx] + v : v;
  }
}

}  // namespace
}  // namespace tgp

using namespace tgp;

extern "C" int tgp_acc_small_graph_nodes(void) { return AC_SMALL_NODES; }

extern "C" int tgp_acc_tv_dense_f32(const float* A, const float* S, int64_t B, int64_t N, int64_t K,
                                    const int64_t* graph_sizes, int64_t nrb, float* part, int* cnt, void* stream_) {
  TGP_REQUIRE(B >= 0 && N >= 0 && K >= 1, TGP_ERR_INVALID, "tgp_acc_tv_dense_f32: bad shape");
  TGP_REQUIRE(nrb == cdiv(N, AC_TV_ROWS) || (N == 0 && nrb == 1), TGP_ERR_INVALID,
              "tgp_acc_tv_dense_f32: nrb must be ceil(N / 16)");
  if (B == 0) return TGP_OK;
  TGP_REQUIRE(part && cnt && (N == 0 || (A && S)), TGP_ERR_INVALID, "tgp_acc_tv_dense_f32: null pointer");
  TGP_REQUIRE(B < 65536 && N < (1ll << 24) && K < 32768 && nrb < (1ll << 31), TGP_ERR_RANGE,
              "tgp_acc_tv_dense_f32: too large");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const dim3 grid(static_cast<unsigned>(nrb), static_cast<unsigned>(B));
  const int n = static_cast<int>(N), k = static_cast<int>(K), r = static_cast<int>(nrb);
  if ((N & 3) == 0 && reinterpret_cast<uintptr_t>(A) % 16 == 0)
    hipLaunchKernelGGL(acc_tv_dense_kernel<true>, grid, dim3(256), 0, stream, A, S, n, k, graph_sizes, r, part, cnt);
  else
    hipLaunchKernelGGL(acc_tv_dense_kernel<false>, grid, dim3(256), 0, stream, A, S, n, k, graph_sizes, r, part, cnt);
  return check_launch("tgp_acc_tv_dense_f32");
}

extern "C" int tgp_acc_tv_dense_bwd_f32(const float* A, const float* S, int64_t B, int64_t N, int64_t K,
                                        const int64_t* graph_sizes, const float* g_terms, const int* ecnt, float c_tv,
                                        float* dS, void* stream_) {
  TGP_REQUIRE(B >= 0 && N >= 0 && K >= 1, TGP_ERR_INVALID, "tgp_acc_tv_dense_bwd_f32: bad shape");
  if (B == 0 || N == 0) return TGP_OK;
  TGP_REQUIRE(A && S && g_terms && ecnt && dS, TGP_ERR_INVALID, "tgp_acc_tv_dense_bwd_f32: null pointer");
  TGP_REQUIRE(B < 65536 && N < (1ll << 24) && K < 32768, TGP_ERR_RANGE, "tgp_acc_tv_dense_bwd_f32: too large");
  const dim3 grid(static_cast<unsigned>(cdiv(N, AC_BWD_ROWS)), static_cast<unsigned>(B));
  hipLaunchKernelGGL(acc_tv_dense_bwd_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream_), A, S,
                     static_cast<int>(N), static_cast<int>(K), graph_sizes, g_terms, ecnt, c_tv, dS);
  return check_launch("tgp_acc_tv_dense_bwd_f32");
}

extern "C" int tgp_acc_tv_edge_f32(const float* S, int64_t nodes, int64_t K, const int64_t* col, const float* w,
                                   int64_t E, const int* src_ptr, const int* src_perm, float* node_tv, void* stream_) {
  TGP_REQUIRE(nodes >= 0 && K >= 1 && E >= 0, TGP_ERR_INVALID, "tgp_acc_tv_edge_f32: bad shape");
  if (nodes == 0) return TGP_OK;
  TGP_REQUIRE(S && src_ptr && node_tv && (E == 0 || (col && src_perm)), TGP_ERR_INVALID,
              "tgp_acc_tv_edge_f32: null pointer");
  TGP_REQUIRE(nodes < (1ll << 31) && E < (1ll << 31) && K < 32768, TGP_ERR_RANGE, "tgp_acc_tv_edge_f32: too large");
  hipLaunchKernelGGL(acc_tv_edge_kernel, dim3(static_cast<unsigned>(cdiv(nodes, 4))), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), S, nodes, static_cast<int>(K), col, w, src_ptr, src_perm, node_tv);
  return check_launch("tgp_acc_tv_edge_f32");
}

extern "C" int tgp_acc_tv_edge_bwd_f32(const float* S, int64_t nodes, int64_t K, const int64_t* row, const int64_t* col,
                                       const float* w, int64_t E, const int* src_ptr, const int* src_perm,
                                       const int* dst_ptr, const int* dst_perm, const int64_t* batch,
                                       const float* g_terms, const int* ecnt, float c_tv, int64_t B, float* dS,
                                       void* stream_) {
  TGP_REQUIRE(nodes >= 0 && K >= 1 && E >= 0 && B >= 1, TGP_ERR_INVALID, "tgp_acc_tv_edge_bwd_f32: bad shape");
  if (nodes == 0) return TGP_OK;
  TGP_REQUIRE(S && src_ptr && dst_ptr && g_terms && ecnt && dS && (E == 0 || (row && col && src_perm && dst_perm)),
              TGP_ERR_INVALID, "tgp_acc_tv_edge_bwd_f32: null pointer");
  TGP_REQUIRE(nodes < (1ll << 31) && E < (1ll << 31) && K < 32768 && B < (1ll << 31), TGP_ERR_RANGE,
              "tgp_acc_tv_edge_bwd_f32: too large");
  hipLaunchKernelGGL(acc_tv_edge_bwd_kernel, dim3(static_cast<unsigned>(cdiv(nodes, 4))), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), S, nodes, static_cast<int>(K), row, col, w, src_ptr, src_perm,
                     dst_ptr, dst_perm, batch, g_terms, ecnt, c_tv, static_cast<int>(B), dS);
  return check_launch("tgp_acc_tv_edge_bwd_f32");
}

extern "C" int tgp_acc_quantile_f32(const float* S, int64_t B, int64_t N, int64_t K, const int64_t* graph_sizes,
                                    const uint8_t* mask, const int64_t* ptr, int64_t max_nodes, int64_t kq, int route,
                                    float* q, int* qnode, float* colsum, int* cge, int* nreal, void* stream_) {
  TGP_REQUIRE(B >= 0 && N >= 0 && K >= 1 && max_nodes >= 0, TGP_ERR_INVALID, "tgp_acc_quantile_f32: bad shape");
  TGP_REQUIRE(route >= 0 && route <= 2, TGP_ERR_INVALID, "tgp_acc_quantile_f32: route must be 0, 1 or 2");
  TGP_REQUIRE(!(ptr && (mask || graph_sizes)), TGP_ERR_INVALID,
              "tgp_acc_quantile_f32: a mask or graph sizes belong to the padded layout");
  TGP_REQUIRE(ptr || max_nodes == N, TGP_ERR_INVALID, "tgp_acc_quantile_f32: max_nodes must be N in the padded layout");
  TGP_REQUIRE(route != 1 || max_nodes <= AC_SMALL_NODES, TGP_ERR_RANGE,
              "tgp_acc_quantile_f32: the counting select takes graphs of at most 128 nodes");
  if (B == 0) return TGP_OK;
  TGP_REQUIRE(q && qnode && colsum && cge && nreal && (max_nodes == 0 || S), TGP_ERR_INVALID,
              "tgp_acc_quantile_f32: null pointer");
  TGP_REQUIRE(B < 65536 && max_nodes < (1ll << 31) && K < 32768 && kq < (1ll << 31) && kq > -(1ll << 31), TGP_ERR_RANGE,
              "tgp_acc_quantile_f32: too large");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int n = static_cast<int>(N), k = static_cast<int>(K), kk = static_cast<int>(kq);
  const bool small = route == 1 || (route == 0 && max_nodes <= AC_SMALL_NODES);
  if (small)
    hipLaunchKernelGGL(acc_select_count_kernel, dim3(static_cast<unsigned>(B)), dim3(256), 0, stream, S, n, k, graph_sizes,
                       mask, ptr, kk, q, qnode, colsum, cge, nreal);
  else
    hipLaunchKernelGGL(acc_select_radix_kernel, dim3(static_cast<unsigned>(cdiv(K, AC_COLS)), static_cast<unsigned>(B)),
                       dim3(256), 0, stream, S, n, k, graph_sizes, mask, ptr, kk, q, qnode, colsum, cge, nreal);
  return check_launch("tgp_acc_quantile_f32");
}

extern "C" int tgp_acc_loss_terms_f32(const float* tv, const int* cnt, const int* src_ptr, const int64_t* ptr, int64_t nrb,
                                      const float* colsum, const int* nreal, int64_t B, int64_t K, int64_t kq, float c_tv,
                                      float c_bal, float* out, int* ecnt, void* stream_) {
  TGP_REQUIRE(B >= 0 && K >= 1 && nrb >= 0, TGP_ERR_INVALID, "tgp_acc_loss_terms_f32: bad shape");
  TGP_REQUIRE(!tv || (src_ptr ? (ptr != nullptr && !cnt) : (cnt != nullptr && nrb >= 1)), TGP_ERR_INVALID,
              "tgp_acc_loss_terms_f32: the dense form takes cnt and nrb, the edge form src_ptr and ptr");
  TGP_REQUIRE(!colsum || nreal, TGP_ERR_INVALID, "tgp_acc_loss_terms_f32: colsum needs nreal");
  if (B == 0) return TGP_OK;
  TGP_REQUIRE(out, TGP_ERR_INVALID, "tgp_acc_loss_terms_f32: null pointer");
  TGP_REQUIRE(B < (1ll << 31) && K < 32768 && nrb < (1ll << 31) && kq < (1ll << 31) && kq > -(1ll << 31), TGP_ERR_RANGE,
              "tgp_acc_loss_terms_f32: too large");
  hipLaunchKernelGGL(acc_tail_kernel, dim3(static_cast<unsigned>(B)), dim3(256), 0, static_cast<hipStream_t>(stream_), tv,
                     cnt, src_ptr, ptr, static_cast<int>(nrb), colsum, nreal, static_cast<int>(K), static_cast<int>(kq),
                     c_tv, c_bal, static_cast<int>(B), out, ecnt);
  return check_launch("tgp_acc_loss_terms_f32");
}

extern "C" int tgp_acc_asym_bwd_f32(const float* S, int64_t rows, int64_t N, int64_t K, const int64_t* batch,
                                    const int64_t* ptr, const int64_t* graph_sizes, const uint8_t* mask, const float* q,
                                    const int* qnode, const int* cge, const int* nreal, const float* g_bal, float c_bal,
                                    int64_t kq, int64_t B, int accumulate, float* dS, void* stream_) {
  TGP_REQUIRE(rows >= 0 && K >= 1 && B >= 0 && (ptr || N >= 1), TGP_ERR_INVALID, "tgp_acc_asym_bwd_f32: bad shape");
  TGP_REQUIRE(!(ptr && (mask || graph_sizes)), TGP_ERR_INVALID,
              "tgp_acc_asym_bwd_f32: a mask or graph sizes belong to the padded layout");
  if (rows == 0) return TGP_OK;
  TGP_REQUIRE(S && q && qnode && cge && nreal && g_bal && dS, TGP_ERR_INVALID, "tgp_acc_asym_bwd_f32: null pointer");
  TGP_REQUIRE(N < (1ll << 31) && K < 32768 && B < (1ll << 31) && rows < (1ll << 40) && kq < (1ll << 31) &&
                  kq > -(1ll << 31),
              TGP_ERR_RANGE, "tgp_acc_asym_bwd_f32: too large");
  const int64_t total = rows * K;
  const int64_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(acc_asym_bwd_kernel, dim3(static_cast<unsigned>(blocks < 65536 ? blocks : 65536)), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), S, rows, static_cast<int>(N), static_cast<int>(K), batch, ptr,
                     graph_sizes, mask, q, qnode, cge, nreal, g_bal, c_bal, static_cast<int>(kq), static_cast<int>(B),
                     accumulate, dS);
  return check_launch("tgp_acc_asym_bwd_f32");
}
