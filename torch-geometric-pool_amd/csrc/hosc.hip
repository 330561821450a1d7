// HOSC pooling's auxiliary losses (reference poolers/hosc.py, utils/losses.py:218-316, 392-432, 597-641):
//
//   cut[b]    = -trace(S^T A S) / (sum_i d1_i |S_i|^2 + eps)                d1 = A 1           (MinCut's first-order cut)
//   ho_cut[b] = -num / (den + eps),  num = sum S (.) Z,  Z = A (A (A S)),   den = sum_i d3_i |S_i|^2,  d3 = A (A (A 1))
//   hosc[b]   = ((1 - alpha) cut + alpha ho_cut) / k
//   ortho[b]  = mu || G / ||G||_F - I / sqrt(K) ||_F   (G = S^T S, MinCut's)   or, hosc_ortho,
//               mu (sqrt(K) - sum_j ||S_*j|| / sqrt(n_b)) / (sqrt(K) - 1)      (0 when K <= 1)
//
// The motif adjacency M = A A A is never formed: d3 is three matrix-vector passes over A (a_rows_kernel), Z three
// N^2 K products on the fp32-MFMA bmm (or three CSR SpMMs for an edge list), num / den / the column norms one pass over
// S, Z and the degree vectors (hosc_part_kernel) reduced per graph in a fixed order by the tail (no float atomics).
// Batches of small graphs (N, K <= 64) get d1, d3, Z and the partial record from ONE launch (hosc_small_kernel).
#include "loss_common.h"

namespace tgp {
namespace {

constexpr int HS_SMALL = 64;        // the small-graph kernel: at most this many nodes and clusters
constexpr int HS_REC = 4;           // floats per 64-column block of a partial record: num | den3 | num1 | den1

__host__ __device__ inline int hs_record(int K) { return K + HS_REC * ((K + 63) / 64) + 1; }

// One workgroup per (64 columns kc, 64 rows, graph): part[b][split] = [ sum_i S_ik^2 (K) | per kc: num = sum S Z,
// den3 = sum d3_i S_ik^2, num1 = sum S Z1, den1 = sum d1_i S_ik^2 | node count ].  Z, Z1 have row stride ldz, d3 and d1
// element stride ldd (columns of a wider buffer); each of Z, Z1, d3, d1 may be NULL (its sum is 0).
// Graph b owns rows start .. start + count: padded (ptr == NULL: start = b N, count = graph size or N) or un-padded
// (ptr[b] .. ptr[b+1]).  Node count: the mask's true entries among the N padded rows (N without a mask), the graph's rows
// when un-padded.
__global__ __launch_bounds__(256) void hosc_part_kernel(const float* __restrict__ S, const float* __restrict__ Z,
                                                        const float* __restrict__ Z1, int ldz,
                                                        const float* __restrict__ d3, const float* __restrict__ d1,
                                                        int ldd, int N, int K, const int64_t* __restrict__ sizes,
                                                        const uint8_t* __restrict__ mask,
                                                        const int64_t* __restrict__ ptr, int nsplit,
                                                        float* __restrict__ part) {
  __shared__ float sh_sq[4][64];
  __shared__ float sh[5 * 4];
  const int kc = blockIdx.x, split = blockIdx.y, b = blockIdx.z;
  const int c = threadIdx.x & 63, r = threadIdx.x >> 6;
  const int k = kc * 64 + c;
  int64_t start, count;
  graph_rows(b, N, sizes, ptr, start, count);
  const int64_t span = ptr ? count : N;
  const int64_t lo = static_cast<int64_t>(split) * PART_ROWS;
  const int64_t hi = count < lo + PART_ROWS ? count : lo + PART_ROWS;
  float sq = 0.f, num = 0.f, den3 = 0.f, num1 = 0.f, den1 = 0.f;
  if (k < K) {
#pragma unroll 4
    for (int64_t i = lo + r; i < hi; i += 4) {
      const int64_t row = start + i;
      const float s = S[row * K + k];
      const float s2 = s * s;
      sq += s2;
      if (Z) num = fmaf(s, Z[row * ldz + k], num);
      if (Z1) num1 = fmaf(s, Z1[row * ldz + k], num1);
      if (d3) den3 = fmaf(d3[row * ldd], s2, den3);
      if (d1) den1 = fmaf(d1[row * ldd], s2, den1);
    }
  }
  sh_sq[r][c] = sq;
  float nr = 0.f;
  if (kc == 0 && threadIdx.x < PART_ROWS) {
    const int64_t i = lo + threadIdx.x;
    if (i < span) nr = (ptr || !mask) ? 1.f : (mask[start + i] ? 1.f : 0.f);
  }
  float v[5] = {num, den3, num1, den1, nr};
  block_sums<256, 5>(v, sh);  // (its barriers also publish sh_sq)
  const int nkc = (K + 63) / 64;
  float* out = part + (static_cast<int64_t>(b) * nsplit + split) * hs_record(K);
  if (r == 0 && k < K) out[k] = (sh_sq[0][c] + sh_sq[1][c]) + (sh_sq[2][c] + sh_sq[3][c]);
  if (threadIdx.x == 0) {
    float* rec = out + K + HS_REC * kc;
    rec[0] = v[0], rec[1] = v[1], rec[2] = v[2], rec[3] = v[3];
    if (kc == 0) out[K + HS_REC * nkc] = v[4];
  }
}

// One workgroup per graph of a padded batch with N, K <= 64: A[b] (row stride 65: lane = row reads are conflict-free) and
// two ping-pong [N,K] buffers in LDS (48.3 KB), the thread's own entries of S in registers.  Three rounds T <- A T give
// Z = A (A (A S)); wave 0 carries d <- A d beside them (d1 after the first round, d3 after the third).  Writes Z [B,N,K],
// d1, d3 [B,N] and the partial record of hosc_part_kernel (nsplit = 1; num1 = sum S (.) (A S) from the first round).
// A wave holds R = 64 / KP rows at once, KP = K rounded up to a power of two, at least 4 (lane = (row in the group,
// column)): with
// K = 20 no more than 12 of 32 lanes idle, and a thread carries 16 / R rows.  With graph sizes (a zero-padded batch) the
// summation index stops at the graph's size; rows beyond it are computed and dropped (a test on the row inside the
// inner loop serialised its LDS reads: 187 us against 118 us on 2048 graphs of 20-60 nodes).
template <int KP>
__global__ __launch_bounds__(256) void hosc_small_kernel(const float* __restrict__ A, const float* __restrict__ S, int N,
                                                         int K, const int64_t* __restrict__ sizes,
                                                         const uint8_t* __restrict__ mask, float* __restrict__ Zout,
                                                         float* __restrict__ d1out, float* __restrict__ d3out,
                                                         float* __restrict__ part) {
  __shared__ float sA[HS_SMALL * (HS_SMALL + 1)];
  __shared__ float sT[2][HS_SMALL * HS_SMALL];
  __shared__ float sd[2][HS_SMALL];
  __shared__ float sh_sq[256];
  __shared__ float sh[5 * 4];
  const int b = blockIdx.x;
  constexpr int R = HS_SMALL / KP, NQ = 16 / R;  // rows a wave holds at once; rows per thread
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = lane & (KP - 1);
  const int row0 = wave * R + lane / KP;  // the thread's rows: row0 + 4 R q, q < NQ
  const int n = sizes ? static_cast<int>(sizes[b] < N ? sizes[b] : N) : N;  // rows of the graph
  const int nj = sizes ? n : N;  // columns that can hold a nonzero
  const float* Ab = A + static_cast<int64_t>(b) * N * N;
  const float* Sb = S + static_cast<int64_t>(b) * N * K;
  for (int e = threadIdx.x; e < N * N; e += 256) sA[(e / N) * (HS_SMALL + 1) + e % N] = Ab[e];
  float s[NQ], d1r[NQ], acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    s[q] = d1r[q] = acc[q] = 0.f;
    const int i = row0 + 4 * R * q;
    if (i < N && k < K) s[q] = Sb[i * K + k];
    if (k < K) sT[0][i * HS_SMALL + k] = s[q];
  }
  if (threadIdx.x < HS_SMALL) sd[0][threadIdx.x] = 1.f;
  __syncthreads();
  float num1 = 0.f;
  int cur = 0;
  for (int round = 0; round < 3; ++round) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.f;
    if (k < K) {
      for (int j = 0; j < nj; ++j) {
        const float t = sT[cur][j * HS_SMALL + k];
#pragma unroll
        for (int q = 0; q < NQ; ++q)  // (no branch in here: the NQ + 1 LDS reads of a step are in flight together)
          acc[q] = fmaf(sA[(row0 + 4 * R * q) * (HS_SMALL + 1) + j], t, acc[q]);
      }
    }
    if (threadIdx.x < HS_SMALL) {  // wave 0: d <- A d on the graph's rows
      float d = 0.f;
      if (static_cast<int>(threadIdx.x) < n)
        for (int j = 0; j < nj; ++j) d = fmaf(sA[threadIdx.x * (HS_SMALL + 1) + j], sd[cur][j], d);
      sd[cur ^ 1][threadIdx.x] = d;
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int i = row0 + 4 * R * q;
      if (i >= n) acc[q] = 0.f;  // (rows beyond the graph: 0, as the general route's products leave them)
      if (k < K) sT[cur ^ 1][i * HS_SMALL + k] = acc[q];
      if (round == 0) num1 = fmaf(s[q], acc[q], num1);
    }
    __syncthreads();
    cur ^= 1;
    if (round == 0) {
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        d1r[q] = sd[cur][row0 + 4 * R * q];
      if (threadIdx.x < N) d1out[static_cast<int64_t>(b) * N + threadIdx.x] = sd[cur][threadIdx.x];
    }
  }
  if (threadIdx.x < N) d3out[static_cast<int64_t>(b) * N + threadIdx.x] = sd[cur][threadIdx.x];
  float sq = 0.f, num = 0.f, den3 = 0.f, den1 = 0.f;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = row0 + 4 * R * q;
    if (i < N && k < K) {
      Zout[(static_cast<int64_t>(b) * N + i) * K + k] = acc[q];
      if (i < n) {
        const float s2 = s[q] * s[q];
        sq += s2;
        num = fmaf(s[q], acc[q], num);
        den3 = fmaf(sd[cur][i], s2, den3);
        den1 = fmaf(d1r[q], s2, den1);
      }
    }
  }
  sh_sq[threadIdx.x] = sq;
  float nr = 0.f;
  if (threadIdx.x < N) nr = mask ? (mask[static_cast<int64_t>(b) * N + threadIdx.x] ? 1.f : 0.f) : 1.f;
  float v[5] = {num, den3, num1, den1, nr};
  block_sums<256, 5>(v, sh);  // (its barriers also publish sh_sq)
  float* out = part + static_cast<int64_t>(b) * hs_record(K);
  if (static_cast<int>(threadIdx.x) < K) {  // column threadIdx.x: its 256 / KP row groups in a fixed order
    float c = 0.f;
    for (int gidx = 0; gidx < 256 / KP; ++gidx) c += sh_sq[gidx * KP + threadIdx.x];
    out[threadIdx.x] = c;
  }
  if (threadIdx.x == 0) {
    out[K] = v[0], out[K + 1] = v[1], out[K + 2] = v[2], out[K + 3] = v[3];
    out[K + HS_REC] = v[4];
  }
}

// One workgroup per graph: the partials summed in split order, then the two terms (out [2,B]).  Also written for the
// backward: cn [B,K] = ||S_*k|| and stats [B,6] = (num | den3 + eps | n_b | trace | den1 + eps | sum_k cn_k).
//   trace(S^T A S): the diagonal of raw [B,K,K], else the num1 partials.
template <int T>
__global__ __launch_bounds__(T) void hosc_tail_kernel(const float* __restrict__ part, int nsplit,
                                                      const float* __restrict__ raw, const float* __restrict__ gram,
                                                      int K, float alpha, float mu, float inv_k, int hosc_ortho,
                                                      float eps, int B, float* __restrict__ out,
                                                      float* __restrict__ cn_out, float* __restrict__ stats) {
  __shared__ float sh[7 * (T / 64)];
  const int b = blockIdx.x;
  const int P = hs_record(K), nkc = (K + 63) / 64;
  const float* pb = part + static_cast<int64_t>(b) * nsplit * P;
  float cnsum = 0.f;
  for (int k = threadIdx.x; k < K; k += T) {
    float a = 0.f;
#pragma unroll 8
    for (int j = 0; j < nsplit; ++j) a += pb[static_cast<int64_t>(j) * P + k];
    const float c = sqrtf(a);
    cn_out[static_cast<int64_t>(b) * K + k] = c;
    cnsum += c;
  }
  float num = 0.f, den3 = 0.f, num1 = 0.f, den1 = 0.f, nr = 0.f;
  for (int j = threadIdx.x; j < nsplit; j += T) {
    const float* rec = pb + static_cast<int64_t>(j) * P + K;
    for (int q = 0; q < nkc; ++q) {
      num += rec[HS_REC * q];
      den3 += rec[HS_REC * q + 1];
      num1 += rec[HS_REC * q + 2];
      den1 += rec[HS_REC * q + 3];
    }
    nr += rec[HS_REC * nkc];
  }
  const int64_t off = static_cast<int64_t>(b) * K * K;
  float tr = 0.f, sq = 0.f;
  if (raw)
    for (int i = threadIdx.x; i < K; i += T) tr += raw[off + static_cast<int64_t>(i) * K + i];
  if (gram)
    for (int i = threadIdx.x; i < K * K; i += T) sq = fmaf(gram[off + i], gram[off + i], sq);
  float v[7] = {cnsum, num, den3, num1, den1, nr, tr};
  block_sums<T, 7>(v, sh);
  cnsum = v[0], num = v[1], den3 = v[2], num1 = v[3], den1 = v[4], nr = v[5], tr = v[6];
  float ortho = 0.f;
  if (gram) {
    sq = block_sum<T>(sq, sh);
    ortho = ortho_term<T>(gram + off, K, sq, sh);
  } else if (hosc_ortho && K > 1) {
    const float sqrt_k = sqrtf(static_cast<float>(K));
    ortho = (sqrt_k - cnsum / sqrtf(nr)) / (sqrt_k - 1.0f);
  }
  if (threadIdx.x == 0) {
    if (!raw) tr = num1;
    const float D3 = den3 + eps, D1 = den1 + eps;
    const float cut = alpha < 1.f ? -(tr / D1) : 0.f;
    const float ho = alpha > 0.f ? -(num / D3) : 0.f;
    out[b] = (1.0f - alpha) * (cut * inv_k) + alpha * (ho * inv_k);
    out[B + b] = mu != 0.f ? mu * ortho : 0.f;
    float* st = stats + static_cast<int64_t>(b) * 6;
    st[0] = num, st[1] = D3, st[2] = nr, st[3] = tr, st[4] = D1, st[5] = cnsum;
  }
}

// Backward of the tail, one workgroup per graph, from the upstream gradients g [2,B]:
//   coef[b] = (c_num, c_den, c_ortho, c_den1, c_num1):
//     c_num  = -g0 alpha / (k D3)            dS += c_num (Z + Zt)           Zt = A^T (A^T (A^T S))
//     c_den  = +g0 alpha num / (k D3^2)      dS += 2 c_den d3_i S_i
//     c_ortho = -g1 mu / (sqrt(n_b) (sqrt(K) - 1))    dS_ik += c_ortho S_ik / ||S_*k||     (hosc_ortho)
//     c_den1 = +g0 (1 - alpha) trace / (k D1^2)       dS += 2 c_den1 d1_i S_i
//     c_num1 = -g0 (1 - alpha) / (k D1)      g_raw = c_num1 I  (or, without raw, dS += c_num1 (Z1 + Z1t))
//   W[b] = d (mu ortho) / d G (ortho_term_bwd; dS = S (W + W^T)), with gram.
template <int T>
__global__ __launch_bounds__(T) void hosc_tail_bwd_kernel(const float* __restrict__ g, const float* __restrict__ stats,
                                                          const float* __restrict__ gram, int K, float alpha, float mu,
                                                          float inv_k, int hosc_ortho, int B,
                                                          float* __restrict__ g_raw, float* __restrict__ coef,
                                                          float* __restrict__ W) {
  __shared__ float sh[2 * (T / 64)];
  const int b = blockIdx.x;
  const int64_t off = static_cast<int64_t>(b) * K * K;
  const float* st = stats + static_cast<int64_t>(b) * 6;
  const float num = st[0], D3 = st[1], nr = st[2], tr = st[3], D1 = st[4];
  const float g0 = g[b], g1 = g[B + b];
  const float gc = alpha < 1.f ? g0 * (1.0f - alpha) * inv_k : 0.f;
  const float gh = alpha > 0.f ? g0 * alpha * inv_k : 0.f;
  const float c_num1 = -gc / D1;
  if (W && gram) ortho_term_bwd<T>(gram + off, K, g1 * mu, W + off, sh);
  if (g_raw)
    for (int i = threadIdx.x; i < K * K; i += T) g_raw[off + i] = (i / K == i % K) ? c_num1 : 0.f;
  if (threadIdx.x == 0) {
    float* c = coef + static_cast<int64_t>(b) * 5;
    c[0] = -gh / D3;
    c[1] = gh * num / (D3 * D3);
    const float sqrt_k = sqrtf(static_cast<float>(K));
    c[2] = (hosc_ortho && K > 1 && mu != 0.f && nr > 0.f) ? -g1 * mu / (sqrtf(nr) * (sqrt_k - 1.0f)) : 0.f;
    c[3] = gc * tr / (D1 * D1);
    c[4] = c_num1;
  }
}

// ds[row,k] (+)= c_num (Z + Zt) + 2 c_den d3_row S + c_ortho S / cn[b,k] + 2 c_den1 d1_row S + c_num1 (Z1 + Z1t)
// b = row / N (padded) or batch[row] (un-padded).  Zt / Z1t NULL: A = A^T, the forward's product counts twice.  Each of
// Z, d3, cn, d1, Z1 NULL: its term is 0.  A column whose norm is 0 gets no orthogonality gradient.
__global__ __launch_bounds__(256) void hosc_ds_kernel(const float* __restrict__ S, const float* __restrict__ Z,
                                                      const float* __restrict__ Zt, const float* __restrict__ Z1,
                                                      const float* __restrict__ Z1t, int ldz, int ldzt,
                                                      const float* __restrict__ d3, const float* __restrict__ d1,
                                                      int ldd, const float* __restrict__ cn,
                                                      const float* __restrict__ coef, int64_t rows, int N,
                                                      const int64_t* __restrict__ batch, int K, int B, int accumulate,
                                                      float* __restrict__ ds) {
  const int64_t total = rows * K;
  for (int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; idx < total; idx += 256ll * gridDim.x) {
    const int64_t row = idx / K;
    const int k = static_cast<int>(idx - row * K);
    const int64_t b = batch ? batch[row] : row / N;
    float v = 0.f;
    if (b >= 0 && b < B) {
      const float* c = coef + b * 5;
      const float s = S[idx];
      if (Z) v = c[0] * (Z[row * ldz + k] + (Zt ? Zt[row * ldzt + k] : Z[row * ldz + k]));
      if (Z1) v = fmaf(c[4], Z1[row * ldz + k] + (Z1t ? Z1t[row * ldzt + k] : Z1[row * ldz + k]), v);
      float diag = 0.f;
      if (d3) diag = 2.0f * c[1] * d3[row * ldd];
      if (d1) diag = fmaf(2.0f * c[3], d1[row * ldd], diag);
      if (cn) {
        const float nk = cn[b * K + k];
        if (nk > 0.f) diag += c[2] / nk;
      }
      v = fmaf(diag, s, v);
    }
    ds[idx] = accumulate ? ds[idx] + v : v;
  }
}

}  // namespace
}  // namespace tgp

using namespace tgp;

extern "C" int tgp_hosc_small_graph_nodes(void) { return HS_SMALL; }

extern "C" int64_t tgp_hosc_record_floats(int64_t K) { return K >= 1 && K < 32768 ? hs_record(static_cast<int>(K)) : 0; }

extern "C" int tgp_hosc_matvec_f32(const float* A, const float* v, int64_t B, int64_t N, const int64_t* graph_sizes,
                                   float* y, void* stream_) {
  TGP_REQUIRE(B >= 0 && N >= 0, TGP_ERR_INVALID, "tgp_hosc_matvec_f32: bad shape");
  const int64_t rows = B * N;
  if (rows == 0) return TGP_OK;
  TGP_REQUIRE(A && y, TGP_ERR_INVALID, "tgp_hosc_matvec_f32: null pointer");
  TGP_REQUIRE(B < 65536 && N < (1ll << 31) && rows < (1ll << 33), TGP_ERR_RANGE, "tgp_hosc_matvec_f32: too large");
  const uint8_t* mask = nullptr;
  TGP_LAUNCH_A_ROWS(true, A, v, rows, static_cast<int>(N), graph_sizes, mask, y, static_cast<hipStream_t>(stream_));
  return check_launch("tgp_hosc_matvec_f32");
}

extern "C" int tgp_hosc_node_terms_f32(const float* S, const float* Z, const float* Z1, int64_t ldz, const float* d3,
                                       const float* d1, int64_t ldd, int64_t B, int64_t N, int64_t K,
                                       const int64_t* graph_sizes, const uint8_t* mask, const int64_t* ptr,
                                       int64_t nsplit, float* part, void* stream_) {
  TGP_REQUIRE(B >= 0 && N >= 0 && K >= 1 && nsplit >= 1 && ldz >= 0 && ldd >= 0, TGP_ERR_INVALID,
              "tgp_hosc_node_terms_f32: bad shape");
  if (B == 0) return TGP_OK;
  TGP_REQUIRE(S && part, TGP_ERR_INVALID, "tgp_hosc_node_terms_f32: null pointer");
  TGP_REQUIRE((!Z && !Z1) || ldz >= K, TGP_ERR_INVALID, "tgp_hosc_node_terms_f32: ldz < K");
  TGP_REQUIRE((!d3 && !d1) || ldd >= 1, TGP_ERR_INVALID, "tgp_hosc_node_terms_f32: ldd < 1");
  TGP_REQUIRE(ptr || nsplit == cdiv(N, PART_ROWS) || (N == 0 && nsplit == 1), TGP_ERR_INVALID,
              "tgp_hosc_node_terms_f32: nsplit must be ceil(N / 64)");
  TGP_REQUIRE(B < 65536 && N < (1ll << 31) && K < 32768 && nsplit < 65536 && ldz < (1ll << 31) && ldd < (1ll << 31),
              TGP_ERR_RANGE, "tgp_hosc_node_terms_f32: too large");
  const dim3 grid(static_cast<unsigned>(cdiv(K, 64)), static_cast<unsigned>(nsplit), static_cast<unsigned>(B));
  hipLaunchKernelGGL(hosc_part_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream_), S, Z, Z1,
                     static_cast<int>(ldz), d3, d1, static_cast<int>(ldd), static_cast<int>(N), static_cast<int>(K),
                     graph_sizes, mask, ptr, static_cast<int>(nsplit), part);
  return check_launch("tgp_hosc_node_terms_f32");
}

extern "C" int tgp_hosc_small_f32(const float* A, const float* S, int64_t B, int64_t N, int64_t K,
                                  const int64_t* graph_sizes, const uint8_t* mask, float* Z, float* d1, float* d3,
                                  float* part, void* stream_) {
  TGP_REQUIRE(B >= 0 && N >= 1 && K >= 1, TGP_ERR_INVALID, "tgp_hosc_small_f32: bad shape");
  TGP_REQUIRE(N <= HS_SMALL && K <= HS_SMALL, TGP_ERR_RANGE, "tgp_hosc_small_f32: at most 64 nodes and 64 clusters");
  if (B == 0) return TGP_OK;
  TGP_REQUIRE(A && S && Z && d1 && d3 && part, TGP_ERR_INVALID, "tgp_hosc_small_f32: null pointer");
  TGP_REQUIRE(B < (1ll << 31), TGP_ERR_RANGE, "tgp_hosc_small_f32: too many graphs");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
#define TGP_HOSC_SMALL(KP)                                                                                     \
  hipLaunchKernelGGL(hosc_small_kernel<KP>, dim3(static_cast<unsigned>(B)), dim3(256), 0, stream, A, S,         \
                     static_cast<int>(N), static_cast<int>(K), graph_sizes, mask, Z, d1, d3, part)
  if (K <= 4) TGP_HOSC_SMALL(4);
  else if (K <= 8) TGP_HOSC_SMALL(8);
  else if (K <= 16) TGP_HOSC_SMALL(16);
  else if (K <= 32) TGP_HOSC_SMALL(32);
  else TGP_HOSC_SMALL(64);
#undef TGP_HOSC_SMALL
  return check_launch("tgp_hosc_small_f32");
}

extern "C" int tgp_hosc_loss_terms_f32(const float* part, int64_t nsplit, const float* raw, const float* gram, int64_t B,
                                       int64_t K, float alpha, float mu, float inv_k, int hosc_ortho, float eps,
                                       float* out, float* cn, float* stats, void* stream_) {
  TGP_REQUIRE(B >= 0 && K >= 1 && K < 32768 && nsplit >= 1, TGP_ERR_INVALID, "tgp_hosc_loss_terms_f32: bad shape");
  if (B == 0) return TGP_OK;
  TGP_REQUIRE(part && out && cn && stats, TGP_ERR_INVALID, "tgp_hosc_loss_terms_f32: null pointer");
  TGP_REQUIRE(B < (1ll << 31) && nsplit < 65536, TGP_ERR_RANGE, "tgp_hosc_loss_terms_f32: too many graphs");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_LAUNCH_PER_GRAPH(hosc_tail_kernel, B, K, stream, part, static_cast<int>(nsplit), raw, gram, static_cast<int>(K),
                       alpha, mu, inv_k, hosc_ortho, eps, static_cast<int>(B), out, cn, stats);
  return check_launch("tgp_hosc_loss_terms_f32");
}

extern "C" int tgp_hosc_loss_terms_bwd_f32(const float* g_terms, const float* stats, const float* gram, int64_t B,
                                           int64_t K, float alpha, float mu, float inv_k, int hosc_ortho, float* g_raw,
                                           float* coef, float* W, void* stream_) {
  TGP_REQUIRE(B >= 0 && K >= 1 && K < 32768, TGP_ERR_INVALID, "tgp_hosc_loss_terms_bwd_f32: bad shape");
  if (B == 0) return TGP_OK;
  TGP_REQUIRE(g_terms && stats && coef && (!gram || W), TGP_ERR_INVALID, "tgp_hosc_loss_terms_bwd_f32: null pointer");
  TGP_REQUIRE(B < (1ll << 31), TGP_ERR_RANGE, "tgp_hosc_loss_terms_bwd_f32: too many graphs");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_LAUNCH_PER_GRAPH(hosc_tail_bwd_kernel, B, K, stream, g_terms, stats, gram, static_cast<int>(K), alpha, mu, inv_k,
                       hosc_ortho, static_cast<int>(B), g_raw, coef, W);
  return check_launch("tgp_hosc_loss_terms_bwd_f32");
}

extern "C" int tgp_hosc_ds_f32(const float* S, const float* Z, const float* Zt, const float* Z1, const float* Z1t,
                               int64_t ldz, int64_t ldzt, const float* d3, const float* d1, int64_t ldd, const float* cn,
                               const float* coef, int64_t rows, int64_t N, const int64_t* batch, int64_t B, int64_t K,
                               int accumulate, float* ds, void* stream_) {
  TGP_REQUIRE(rows >= 0 && B >= 0 && K >= 1 && (batch || N >= 1) && ldz >= 0 && ldzt >= 0 && ldd >= 0, TGP_ERR_INVALID,
              "tgp_hosc_ds_f32: bad shape");
  if (rows == 0) return TGP_OK;
  TGP_REQUIRE(S && coef && ds, TGP_ERR_INVALID, "tgp_hosc_ds_f32: null pointer");
  TGP_REQUIRE((!Z && !Z1) || ldz >= K, TGP_ERR_INVALID, "tgp_hosc_ds_f32: ldz < K");
  TGP_REQUIRE((!Zt && !Z1t) || ldzt >= K, TGP_ERR_INVALID, "tgp_hosc_ds_f32: ldzt < K");
  TGP_REQUIRE((!Zt || Z) && (!Z1t || Z1), TGP_ERR_INVALID, "tgp_hosc_ds_f32: a transposed product without its forward one");
  TGP_REQUIRE((!d3 && !d1) || ldd >= 1, TGP_ERR_INVALID, "tgp_hosc_ds_f32: ldd < 1");
  TGP_REQUIRE(N < (1ll << 31) && K < 32768 && B < (1ll << 31) && rows < (1ll << 40) && ldz < (1ll << 31) &&
                  ldzt < (1ll << 31) && ldd < (1ll << 31),
              TGP_ERR_RANGE, "tgp_hosc_ds_f32: too large");
  const int64_t total = rows * K;
  const int64_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(hosc_ds_kernel, dim3(static_cast<unsigned>(blocks < 65536 ? blocks : 65536)), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), S, Z, Zt, Z1, Z1t, static_cast<int>(ldz), static_cast<int>(ldzt),
                     d3, d1, static_cast<int>(ldd), cn, coef, rows, static_cast<int>(N), batch, static_cast<int>(K),
                     static_cast<int>(B), accumulate, ds);
  return check_launch("tgp_hosc_ds_f32");
}
