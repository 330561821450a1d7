// LaPool's selector (reference select/lapool_select.py): the Laplacian signal variation v_i = ||(L X)_i||, the leaders
// (nodes whose v is no smaller than any neighbour's), their per-graph columns, and the per-graph softmax over cosine
// similarities with its backward.  fp32, no float atomics, every output element written by exactly one place: the same
// bits on every call.  Nothing here is sized N_total x K_total: a graph's rows see that graph's leaders only, through
// the list `leaders` (graph b's leaders, ascending, stored from the graph's first row on: k_b <= n_b, so [rows] ints
// hold every graph's list without a prefix sum over the graphs).
//
// Rows and graphs.  Padded batch (ptr NULL): graph b owns rows b N .. b N + N - 1, `mask` ([B N] bytes, NULL = all real)
// says which are real.  Un-padded batch (ptr [B + 1]): graph b owns rows ptr[b] .. ptr[b + 1] - 1, `batch` names the
// graph of a row (NULL with B = 1).
#include "loss_common.h"

namespace tgp {
namespace {

__device__ __forceinline__ int graph_of(int64_t row, int N, const int64_t* ptr, const int64_t* batch) {
  return ptr ? (batch ? static_cast<int>(batch[row]) : 0) : static_cast<int>(row / N);
}

// ---- v of a padded batch: one wave per row, one pass over A ---------------------------------------------------------
// A lane loads four columns of a 256-column chunk (one 16-byte load when VEC: N % 4 == 0 and A 16-byte aligned; four
// element loads otherwise), masked columns count as zero, and the wave then visits the NONZERO columns only (ballot):
// for each, deg += a and, lane f, acc_f += a x_jf.  Both paths add in the same order: the same bits.
template <bool VEC>
__global__ __launch_bounds__(256) void lapool_var_dense_kernel(const float* __restrict__ A, const float* __restrict__ X,
                                                               int64_t rows, int N, int F,
                                                               const uint8_t* __restrict__ mask, float* __restrict__ v) {
  const int lane = threadIdx.x & 63;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  if (mask && !mask[row]) {
    if (lane == 0) v[row] = 0.f;
    return;
  }
  const int64_t g0 = row / N * N;
  const float* a = A + row * N;
  const float* xg = X + g0 * F;
  const uint8_t* mg = mask ? mask + g0 : nullptr;
  float ss = 0.f;
  for (int f0 = 0; f0 < F; f0 += 64) {
    const int f = f0 + lane;
    const bool fin = f < F;
    float deg = 0.f, acc = 0.f;
    for (int j0 = 0; j0 < N; j0 += 256) {
      const int jb = j0 + lane * 4;
      float p[4] = {0.f, 0.f, 0.f, 0.f};
      if (VEC) {
        if (jb < N) {
          const f32x4 q = *reinterpret_cast<const f32x4*>(a + jb);
          p[0] = q.x, p[1] = q.y, p[2] = q.z, p[3] = q.w;
        }
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (jb + t < N) p[t] = a[jb + t];
      }
      if (mg) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (jb + t < N && !mg[jb + t]) p[t] = 0.f;
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        unsigned long long m = __ballot(p[t] != 0.f);
        while (m) {
          const int l = __ffsll(static_cast<long long>(m)) - 1;
          m &= m - 1;
          const float av = __shfl(p[t], l, 64);
          const int j = j0 + l * 4 + t;
          deg += av;
          if (fin) acc = fmaf(av, xg[static_cast<int64_t>(j) * F + f], acc);
        }
      }
    }
    const float d = fin ? deg * xg[(row - g0) * F + f] - acc : 0.f;
    ss = fmaf(d, d, ss);
  }
  ss = wave_sum(ss);
  if (lane == 0) v[row] = sqrtf(ss);
}

// ---- v of an edge list grouped by source: G lanes per node, the node's entries in edge-list order --------------------
// get_laplacian's rules: a self-loop is dropped, deg is the sum of what is left, duplicates add.  An endpoint outside
// [0, n) is skipped (the reference's index ops raise for it).
__global__ __launch_bounds__(256) void lapool_var_csr_kernel(const int32_t* __restrict__ row_ptr,
                                                             const int32_t* __restrict__ perm,
                                                             const int64_t* __restrict__ col, const float* __restrict__ w,
                                                             const float* __restrict__ X, int64_t n, int F, int G,
                                                             float* __restrict__ v) {
  const int sub = threadIdx.x % G;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * (256 / G) + threadIdx.x / G;
  float ss = 0.f;
  if (row < n) {
    const int e0 = row_ptr[row], e1 = row_ptr[row + 1];
    for (int f = sub; f < F; f += G) {
      float deg = 0.f, acc = 0.f;
      for (int e = e0; e < e1; ++e) {
        const int p = perm ? perm[e] : e;
        const int64_t c = col[p];
        if (c == row || c < 0 || c >= n) continue;
        const float wv = w ? w[p] : 1.f;
        deg += wv;
        acc = fmaf(wv, X[c * F + f], acc);
      }
      const float d = deg * X[row * F + f] - acc;
      ss = fmaf(d, d, ss);
    }
  }
  for (int o = G / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);  // the order of wave_sum at a run-time group width
  if (row < n && sub == 0) v[row] = sqrtf(ss);
}

// ---- leader flags ----------------------------------------------------------------------------------------------------
// Padded: a second pass over A, one wave per row; the graph's v (4 N bytes) stays in cache.  flag = real row and
// v_i >= v_j for every real column j with a_ij != 0.
__global__ __launch_bounds__(256) void lapool_flags_dense_kernel(const float* __restrict__ A, const float* __restrict__ v,
                                                                 int64_t rows, int N, const uint8_t* __restrict__ mask,
                                                                 uint8_t* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  if (mask && !mask[row]) {
    if (lane == 0) flags[row] = 0;
    return;
  }
  const int64_t g0 = row / N * N;
  const float* a = A + row * N;
  const float* vg = v + g0;
  const uint8_t* mg = mask ? mask + g0 : nullptr;
  const float vi = v[row];
  bool ok = true;
  for (int j = lane; j < N; j += 64)
    if (a[j] != 0.f && (!mg || mg[j])) ok = ok && (vi >= vg[j]);
  const bool all = __all(ok);
  if (lane == 0) flags[row] = all ? 1 : 0;
}

// Edge list: one thread per node over its entries; a self-loop is no neighbour, an explicit zero weight is one.
__global__ __launch_bounds__(256) void lapool_flags_csr_kernel(const int32_t* __restrict__ row_ptr,
                                                               const int32_t* __restrict__ perm,
                                                               const int64_t* __restrict__ col, const float* __restrict__ v,
                                                               int64_t n, uint8_t* __restrict__ flags) {
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (row >= n) return;
  const float vi = v[row];
  bool ok = true;
  for (int e = row_ptr[row], e1 = row_ptr[row + 1]; e < e1; ++e) {
    const int64_t c = col[perm ? perm[e] : e];
    if (c == row || c < 0 || c >= n) continue;
    ok = ok && (vi >= v[c]);
  }
  flags[row] = ok ? 1 : 0;
}

// ---- columns: one workgroup per graph ---------------------------------------------------------------------------------
// fallback != 0: a graph with a real row and no leader makes every real row a leader (written back to flags).  Then the
// rank of every leader among its graph's leaders (a block scan per 256 rows), the leader list, k_b and max_b k_b.
__global__ __launch_bounds__(256) void lapool_columns_kernel(uint8_t* __restrict__ flags, int N,
                                                             const uint8_t* __restrict__ mask,
                                                             const int64_t* __restrict__ ptr, int fallback,
                                                             int32_t* __restrict__ col_of, int32_t* __restrict__ leaders,
                                                             int32_t* __restrict__ k, unsigned long long* __restrict__ k_max) {
  __shared__ int wsum[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int64_t start;
  int64_t count;
  graph_rows(b, N, nullptr, ptr, start, count);
  int any_real = 0, any_leader = 0;
  for (int64_t i = tid; i < count; i += 256) {
    const bool real = !mask || mask[start + i];
    any_real |= real;
    any_leader |= real && flags[start + i];
  }
  any_real = __syncthreads_or(any_real);
  any_leader = __syncthreads_or(any_leader);
  const bool all_lead = fallback && any_real && !any_leader;
  int base = 0;
  for (int64_t i0 = 0; i0 < count; i0 += 256) {
    const int64_t i = i0 + tid;
    bool f = false;
    if (i < count) {
      const bool real = !mask || mask[start + i];
      f = real && (all_lead || flags[start + i]);
      if (all_lead || !real) flags[start + i] = f ? 1 : 0;
    }
    const unsigned long long m = __ballot(f);
    if (lane == 0) wsum[wv] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q < wv) before += wsum[q];
      total += wsum[q];
    }
    __syncthreads();
    if (i < count) {
      const int c = base + before + __popcll(m & lanemask_lt());
      col_of[start + i] = f ? c : -1;
      if (f) leaders[start + c] = static_cast<int32_t>(start + i);
    }
    base += total;
  }
  if (tid == 0) {
    k[b] = base;
    atomicMax(k_max, static_cast<unsigned long long>(base));
  }
}

// ---- row norms: G lanes per row ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lapool_norm_kernel(const float* __restrict__ X, int64_t rows, int F, int G,
                                                          float* __restrict__ nrm) {
  const int sub = threadIdx.x % G;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * (256 / G) + threadIdx.x / G;
  float ss = 0.f;
  if (row < rows)
    for (int f = sub; f < F; f += G) ss = fmaf(X[row * F + f], X[row * F + f], ss);
  for (int o = G / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);  // the order of wave_sum at a run-time group width
  if (row < rows && sub == 0) nrm[row] = sqrtf(ss);
}

// x_r . x_l added f = 0 .. F - 1 in that order on both paths
template <bool VEC>
__device__ __forceinline__ float row_dot(const float* __restrict__ xr, const float* __restrict__ xl, int F) {
  float d = 0.f;
  if (VEC) {
    for (int f = 0; f < F; f += 4) {
      const f32x4 p = *reinterpret_cast<const f32x4*>(xr + f);
      const f32x4 q = *reinterpret_cast<const f32x4*>(xl + f);
      d = fmaf(p.x, q.x, d);
      d = fmaf(p.y, q.y, d);
      d = fmaf(p.z, q.z, d);
      d = fmaf(p.w, q.w, d);
    }
  } else {
    for (int f = 0; f < F; ++f) d = fmaf(xr[f], xl[f], d);
  }
  return d;
}

// ---- S: one wave per row, a lane per leader of the row's graph (64 at a time) ------------------------------------------
// A padded row is 0, a leader row is its one-hot column, every other row the softmax over its graph's k_b cosines; the
// columns from k_b on are 0.  The logits pass through the row of S itself (a lane reads back what it wrote).
template <bool VEC>
__global__ __launch_bounds__(256) void lapool_assign_kernel(const float* __restrict__ X, const float* __restrict__ nrm,
                                                            int64_t rows, int F, int N, const uint8_t* __restrict__ mask,
                                                            const int64_t* __restrict__ ptr,
                                                            const int64_t* __restrict__ batch,
                                                            const int32_t* __restrict__ col_of,
                                                            const int32_t* __restrict__ leaders,
                                                            const int32_t* __restrict__ k, int K, float eps,
                                                            float* __restrict__ S) {
  const int lane = threadIdx.x & 63;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float* s = S + row * K;
  const int own = (mask && !mask[row]) ? -2 : col_of[row];
  if (own != -1) {  // padded (-2) or leader (its column)
    for (int c = lane; c < K; c += 64) s[c] = c == own ? 1.f : 0.f;
    return;
  }
  const int b = graph_of(row, N, ptr, batch);
  int64_t start;
  int64_t count;
  graph_rows(b, N, nullptr, ptr, start, count);
  const int kb = k[b];
  const int32_t* lead = leaders + start;
  const float* xr = X + row * F;
  const float nr = nrm[row];
  float mx = -INFINITY;
  for (int c = lane; c < kb; c += 64) {
    const int64_t l = lead[c];
    const float z = row_dot<VEC>(xr, X + l * F, F) / (nr * nrm[l] + eps);
    s[c] = z;
    mx = fmaxf(mx, z);
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int c = lane; c < kb; c += 64) {
    const float e = expf(s[c] - mx);
    s[c] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  for (int c = lane; c < K; c += 64) s[c] = c < kb ? s[c] / sum : 0.f;
}

// ---- backward, first pass: one wave per non-leader real row -------------------------------------------------------------
// g_c = S_c (dS_c - sum_c' S_c' dS_c') is the gradient of logit z_c = d_c / den_c, d_c = x_r . x_l(c),
// den_c = |x_r| |x_l(c)| + eps.  g1[r,c] = g_c / den_c multiplies x_l(c) in dX_r and x_r in dX_l(c);
// g2[r,c] = g_c d_c |x_r| / (den_c^2 |x_l(c)|) multiplies -x_l(c) in dX_l(c); alpha[r] = sum_c g_c d_c |x_l(c)| /
// (den_c^2 |x_r|) multiplies -x_r in dX_r.  A zero norm passes no gradient (the subgradient torch's norm takes).
template <bool VEC>
__global__ __launch_bounds__(256) void lapool_bwd_terms_kernel(const float* __restrict__ X, const float* __restrict__ nrm,
                                                               const float* __restrict__ S, const float* __restrict__ dS,
                                                               int64_t rows, int F, int N,
                                                               const uint8_t* __restrict__ mask,
                                                               const int64_t* __restrict__ ptr,
                                                               const int64_t* __restrict__ batch,
                                                               const int32_t* __restrict__ col_of,
                                                               const int32_t* __restrict__ leaders,
                                                               const int32_t* __restrict__ k, int K, float eps,
                                                               float* __restrict__ g1, float* __restrict__ g2,
                                                               float* __restrict__ alpha) {
  const int lane = threadIdx.x & 63;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  if ((mask && !mask[row]) || col_of[row] >= 0) return;
  const int b = graph_of(row, N, ptr, batch);
  int64_t start;
  int64_t count;
  graph_rows(b, N, nullptr, ptr, start, count);
  const int kb = k[b];
  const int32_t* lead = leaders + start;
  const float* s = S + row * K;
  const float* ds = dS + row * K;
  const float* xr = X + row * F;
  const float nr = nrm[row];
  float sd = 0.f;
  for (int c = lane; c < kb; c += 64) sd = fmaf(s[c], ds[c], sd);
  sd = wave_sum(sd);
  float al = 0.f;
  for (int c = lane; c < kb; c += 64) {
    const int64_t l = lead[c];
    const float d = row_dot<VEC>(xr, X + l * F, F);
    const float nl = nrm[l];
    const float den = nr * nl + eps;
    const float g = s[c] * (ds[c] - sd);
    const float t = g * d / (den * den);
    g1[row * K + c] = g / den;
    g2[row * K + c] = nl > 0.f ? t * nr / nl : 0.f;
    al += nr > 0.f ? t * nl / nr : 0.f;
  }
  al = wave_sum(al);
  if (lane == 0) alpha[row] = al;
}

// ---- backward, second pass: one wave per row, lanes over the features ---------------------------------------------------
// padded row: 0.  Non-leader row: sum_c g1[r,c] x_l(c) - alpha_r x_r.  Leader row (column c of its graph): the sum over
// its graph's non-leader real rows i, in row order, of g1[i,c] x_i, minus (sum_i g2[i,c]) x_l.  Every row of dX has one
// writer.
__global__ __launch_bounds__(256) void lapool_bwd_dx_kernel(const float* __restrict__ X, const float* __restrict__ g1,
                                                            const float* __restrict__ g2, const float* __restrict__ alpha,
                                                            int64_t rows, int F, int N, const uint8_t* __restrict__ mask,
                                                            const int64_t* __restrict__ ptr,
                                                            const int64_t* __restrict__ batch,
                                                            const int32_t* __restrict__ col_of,
                                                            const int32_t* __restrict__ leaders,
                                                            const int32_t* __restrict__ k, int K, float* __restrict__ dX) {
  const int lane = threadIdx.x & 63;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float* out = dX + row * F;
  if (mask && !mask[row]) {
    for (int f = lane; f < F; f += 64) out[f] = 0.f;
    return;
  }
  const int b = graph_of(row, N, ptr, batch);
  int64_t start;
  int64_t count;
  graph_rows(b, N, nullptr, ptr, start, count);
  const int own = col_of[row];
  if (own < 0) {
    const int kb = k[b];
    const int32_t* lead = leaders + start;
    const float al = alpha[row];
    for (int f = lane; f < F; f += 64) {
      float acc = 0.f;
      for (int c = 0; c < kb; ++c) acc = fmaf(g1[row * K + c], X[static_cast<int64_t>(lead[c]) * F + f], acc);
      out[f] = acc - al * X[row * F + f];
    }
    return;
  }
  for (int f0 = 0; f0 < F; f0 += 64) {
    const int f = f0 + lane;
    float acc = 0.f, q = 0.f;
    for (int64_t i = start; i < start + count; ++i) {
      if ((mask && !mask[i]) || col_of[i] >= 0) continue;
      const float a = g1[i * K + own];
      q += g2[i * K + own];
      if (f < F) acc = fmaf(a, X[i * F + f], acc);
    }
    if (f < F) out[f] = acc - q * X[row * F + f];
  }
}

int lanes_for(int64_t F) { return F > 32 ? 64 : (F > 16 ? 32 : (F > 8 ? 16 : 8)); }

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// what every entry over rows checks: sizes that the int32 internals address
int check_sizes(const char* what, int64_t rows, int64_t N, int64_t F, int64_t K) {
  TGP_REQUIRE(rows >= 0 && N >= 0 && F >= 0 && K >= 0, TGP_ERR_INVALID, "%s: negative size", what);
  TGP_REQUIRE(rows <= INT32_MAX - 256 && N <= INT32_MAX - 256 && F <= INT32_MAX - 64 && K <= INT32_MAX - 64,
              TGP_ERR_RANGE, "%s: rows=%lld N=%lld F=%lld K=%lld beyond the int32 internals", what,
              static_cast<long long>(rows), static_cast<long long>(N), static_cast<long long>(F),
              static_cast<long long>(K));
  return TGP_OK;
}

// a batch layout: padded (ptr NULL, rows = B N) or un-padded (ptr given; batch NULL only with one graph)
int check_layout(const char* what, int64_t rows, int64_t B, int64_t N, const uint8_t* mask, const int64_t* ptr,
                 const int64_t* batch) {
  TGP_REQUIRE(B >= 0 && B <= INT32_MAX, TGP_ERR_RANGE, "%s: B=%lld beyond the int32 internals", what,
              static_cast<long long>(B));
  if (ptr) {
    TGP_REQUIRE(!mask, TGP_ERR_INVALID, "%s: a mask belongs to a padded batch (ptr NULL)", what);
    TGP_REQUIRE(batch || B <= 1, TGP_ERR_INVALID, "%s: an un-padded batch of %lld graphs needs the batch vector", what,
                static_cast<long long>(B));
  } else {
    TGP_REQUIRE(rows == B * N, TGP_ERR_INVALID, "%s: a padded batch has B N = %lld rows, got %lld", what,
                static_cast<long long>(B * N), static_cast<long long>(rows));
  }
  return TGP_OK;
}

}  // namespace
}  // namespace tgp

using namespace tgp;

extern "C" {

int tgp_lapool_variation_dense_f32(const float* A, const float* X, int64_t B, int64_t N, int64_t F, const uint8_t* mask,
                                   float* v, void* stream) {
  TGP_REQUIRE(v, TGP_ERR_INVALID, "tgp_lapool_variation_dense_f32: v is NULL");
  TGP_REQUIRE(B >= 0 && N >= 0 && B <= INT32_MAX && N <= INT32_MAX && B * N <= INT32_MAX - 256, TGP_ERR_RANGE,
              "tgp_lapool_variation_dense_f32: B=%lld N=%lld beyond the int32 internals", static_cast<long long>(B),
              static_cast<long long>(N));
  const int64_t rows = B * N;
  if (int rc = check_sizes("tgp_lapool_variation_dense_f32", rows, N, F, 0)) return rc;
  if (rows == 0) return TGP_OK;
  TGP_REQUIRE(A && (X || F == 0), TGP_ERR_INVALID, "tgp_lapool_variation_dense_f32: A or X is NULL");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if ((N & 3) == 0 && aligned16(A))
    hipLaunchKernelGGL(lapool_var_dense_kernel<true>, dim3(cdiv(rows, 4)), dim3(256), 0, st, A, X, rows,
                       static_cast<int>(N), static_cast<int>(F), mask, v);
  else
    hipLaunchKernelGGL(lapool_var_dense_kernel<false>, dim3(cdiv(rows, 4)), dim3(256), 0, st, A, X, rows,
                       static_cast<int>(N), static_cast<int>(F), mask, v);
  return check_launch("tgp_lapool_variation_dense_f32");
}

int tgp_lapool_variation_csr_f32(const int32_t* row_ptr, const int32_t* perm, const int64_t* col, const float* w,
                                 const float* X, int64_t n, int64_t E, int64_t F, float* v, void* stream) {
  TGP_REQUIRE(v, TGP_ERR_INVALID, "tgp_lapool_variation_csr_f32: v is NULL");
  if (int rc = check_sizes("tgp_lapool_variation_csr_f32", n, 0, F, 0)) return rc;
  TGP_REQUIRE(E >= 0 && E <= INT32_MAX, TGP_ERR_RANGE, "tgp_lapool_variation_csr_f32: E=%lld beyond the int32 internals",
              static_cast<long long>(E));
  if (n == 0) return TGP_OK;
  TGP_REQUIRE(row_ptr && (col || E == 0) && (X || F == 0), TGP_ERR_INVALID,
              "tgp_lapool_variation_csr_f32: row_ptr, col or X is NULL");
  const int G = lanes_for(F);
  hipLaunchKernelGGL(lapool_var_csr_kernel, dim3(cdiv(n, 256 / G)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     row_ptr, perm, col, w, X, n, static_cast<int>(F), G, v);
  return check_launch("tgp_lapool_variation_csr_f32");
}

int tgp_lapool_flags_dense_f32(const float* A, const float* v, int64_t B, int64_t N, const uint8_t* mask, uint8_t* flags,
                               void* stream) {
  TGP_REQUIRE(flags, TGP_ERR_INVALID, "tgp_lapool_flags_dense_f32: flags is NULL");
  TGP_REQUIRE(B >= 0 && N >= 0 && B <= INT32_MAX && N <= INT32_MAX && B * N <= INT32_MAX - 256, TGP_ERR_RANGE,
              "tgp_lapool_flags_dense_f32: B=%lld N=%lld beyond the int32 internals", static_cast<long long>(B),
              static_cast<long long>(N));
  const int64_t rows = B * N;
  if (rows == 0) return TGP_OK;
  TGP_REQUIRE(A && v, TGP_ERR_INVALID, "tgp_lapool_flags_dense_f32: A or v is NULL");
  hipLaunchKernelGGL(lapool_flags_dense_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, static_cast<hipStream_t>(stream), A, v,
                     rows, static_cast<int>(N), mask, flags);
  return check_launch("tgp_lapool_flags_dense_f32");
}

int tgp_lapool_flags_csr_f32(const int32_t* row_ptr, const int32_t* perm, const int64_t* col, const float* v, int64_t n,
                             int64_t E, uint8_t* flags, void* stream) {
  TGP_REQUIRE(flags, TGP_ERR_INVALID, "tgp_lapool_flags_csr_f32: flags is NULL");
  TGP_REQUIRE(n >= 0 && E >= 0, TGP_ERR_INVALID, "tgp_lapool_flags_csr_f32: negative size");
  TGP_REQUIRE(n <= INT32_MAX - 256 && E <= INT32_MAX, TGP_ERR_RANGE,
              "tgp_lapool_flags_csr_f32: n=%lld E=%lld beyond the int32 internals", static_cast<long long>(n),
              static_cast<long long>(E));
  if (n == 0) return TGP_OK;
  TGP_REQUIRE(row_ptr && (col || E == 0) && v, TGP_ERR_INVALID, "tgp_lapool_flags_csr_f32: row_ptr, col or v is NULL");
  hipLaunchKernelGGL(lapool_flags_csr_kernel, dim3(cdiv(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), row_ptr,
                     perm, col, v, n, flags);
  return check_launch("tgp_lapool_flags_csr_f32");
}

int tgp_lapool_columns(uint8_t* flags, int64_t rows, int64_t B, int64_t N, const uint8_t* mask, const int64_t* ptr,
                       int fallback, int32_t* col_of, int32_t* leaders, int32_t* k, int64_t* k_max, void* stream) {
  TGP_REQUIRE(col_of && leaders && k && k_max, TGP_ERR_INVALID, "tgp_lapool_columns: an output is NULL");
  if (int rc = check_sizes("tgp_lapool_columns", rows, N, 0, 0)) return rc;
  if (int rc = check_layout("tgp_lapool_columns", rows, B, N, mask, ptr, ptr /* no row -> graph lookup here */)) return rc;
  TGP_REQUIRE(flags || rows == 0, TGP_ERR_INVALID, "tgp_lapool_columns: flags is NULL");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(k_max, 0, sizeof(int64_t), st) != hipSuccess) return check_launch("tgp_lapool_columns (memset)");
  if (B == 0) return TGP_OK;
  hipLaunchKernelGGL(lapool_columns_kernel, dim3(static_cast<unsigned>(B)), dim3(256), 0, st, flags, static_cast<int>(N),
                     mask, ptr, fallback, col_of, leaders, k, reinterpret_cast<unsigned long long*>(k_max));
  return check_launch("tgp_lapool_columns");
}

int tgp_lapool_assign_f32(const float* X, int64_t rows, int64_t F, int64_t B, int64_t N, const uint8_t* mask,
                          const int64_t* ptr, const int64_t* batch, const int32_t* col_of, const int32_t* leaders,
                          const int32_t* k, int64_t K, float eps, float* nrm, float* S, void* stream) {
  TGP_REQUIRE(nrm && (S || K == 0), TGP_ERR_INVALID, "tgp_lapool_assign_f32: an output is NULL");
  if (int rc = check_sizes("tgp_lapool_assign_f32", rows, N, F, K)) return rc;
  if (int rc = check_layout("tgp_lapool_assign_f32", rows, B, N, mask, ptr, batch)) return rc;
  if (rows == 0) return TGP_OK;
  TGP_REQUIRE((X || F == 0) && col_of && leaders && k, TGP_ERR_INVALID, "tgp_lapool_assign_f32: an input is NULL");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int G = lanes_for(F);
  hipLaunchKernelGGL(lapool_norm_kernel, dim3(cdiv(rows, 256 / G)), dim3(256), 0, st, X, rows, static_cast<int>(F), G,
                     nrm);
  if (K == 0) return check_launch("tgp_lapool_assign_f32");
  if ((F & 3) == 0 && aligned16(X))
    hipLaunchKernelGGL(lapool_assign_kernel<true>, dim3(cdiv(rows, 4)), dim3(256), 0, st, X, nrm, rows,
                       static_cast<int>(F), static_cast<int>(N), mask, ptr, batch, col_of, leaders, k,
                       static_cast<int>(K), eps, S);
  else
    hipLaunchKernelGGL(lapool_assign_kernel<false>, dim3(cdiv(rows, 4)), dim3(256), 0, st, X, nrm, rows,
                       static_cast<int>(F), static_cast<int>(N), mask, ptr, batch, col_of, leaders, k,
                       static_cast<int>(K), eps, S);
  return check_launch("tgp_lapool_assign_f32");
}

int tgp_lapool_assign_bwd_f32(const float* X, const float* nrm, const float* S, const float* dS, int64_t rows, int64_t F,
                              int64_t B, int64_t N, const uint8_t* mask, const int64_t* ptr, const int64_t* batch,
                              const int32_t* col_of, const int32_t* leaders, const int32_t* k, int64_t K, float eps,
                              float* g1, float* g2, float* alpha, float* dX, void* stream) {
  TGP_REQUIRE(dX || rows == 0 || F == 0, TGP_ERR_INVALID, "tgp_lapool_assign_bwd_f32: dX is NULL");
  if (int rc = check_sizes("tgp_lapool_assign_bwd_f32", rows, N, F, K)) return rc;
  if (int rc = check_layout("tgp_lapool_assign_bwd_f32", rows, B, N, mask, ptr, batch)) return rc;
  if (rows == 0 || F == 0) return TGP_OK;
  TGP_REQUIRE(X && nrm && col_of && leaders && k && alpha && (K == 0 || (S && dS && g1 && g2)), TGP_ERR_INVALID,
              "tgp_lapool_assign_bwd_f32: an input or a work buffer is NULL");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if ((F & 3) == 0 && aligned16(X))
    hipLaunchKernelGGL(lapool_bwd_terms_kernel<true>, dim3(cdiv(rows, 4)), dim3(256), 0, st, X, nrm, S, dS, rows,
                       static_cast<int>(F), static_cast<int>(N), mask, ptr, batch, col_of, leaders, k,
                       static_cast<int>(K), eps, g1, g2, alpha);
  else
    hipLaunchKernelGGL(lapool_bwd_terms_kernel<false>, dim3(cdiv(rows, 4)), dim3(256), 0, st, X, nrm, S, dS, rows,
                       static_cast<int>(F), static_cast<int>(N), mask, ptr, batch, col_of, leaders, k,
                       static_cast<int>(K), eps, g1, g2, alpha);
  hipLaunchKernelGGL(lapool_bwd_dx_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, X, g1, g2, alpha, rows,
                     static_cast<int>(F), static_cast<int>(N), mask, ptr, batch, col_of, leaders, k, static_cast<int>(K),
                     dX);
  return check_launch("tgp_lapool_assign_bwd_f32");
}

}  // extern "C"
