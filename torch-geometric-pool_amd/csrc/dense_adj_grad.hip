// The dense poolers' gradient with respect to a dense adjacency A [B,N,N] that was handed in (DiffPool, MinCut; what
// the reference gets from ATen autograd over connect/dense_conn.py:111-122, utils/losses.py:39-56 and :644-652).
// Per graph b, with S [N,K] (padded rows zero), R = S^T A S and M = the total gradient of R that the training step's
// backward already forms (post-processing backward + upstream + the loss' diagonal term):
//
//     dA_b = S_b M_b S_b^T  +  gamma_b q_b 1^T  +  c A_b
//
//   MinCut:   gamma_b = g_cut num_b / (den_b + eps)^2 (the gradient of den_b = sum_i d_i |s_i|^2, d = A 1), q_i = |s_i|^2
//   DiffPool: c = g_link link_scale / ||A - S S^T||_F, one scalar for the batch; the -S S^T part of the residual is the
//             -c I that M already carries
// [B,N,N] is written once: one writer per element, no atomics, a fixed summation order (k ascending).
//
// Two kernels.  Graphs beyond the one-wave kernels: T = S M is an N K^2 product (tgp_bmm_f32), adj_grad_tile_kernel is
// the N^2 K product T S^T on the fp32 matrix cores -- the 128 x 128 tile, the 32 x 32 x 2 MFMA operand order, the
// [rows][BK + 1] LDS tiles and the row permutation of gemm_mfma.h's n-major form (its MODE 1; the header itself is not
// included: its launchers would instantiate every GEMM kernel a second time in this object) -- whose epilogue adds
// gamma_b q_i and c A_ij while the tile is in registers: no second pass over [B,N,N].  Batches the one-wave-per-graph
// kernels take (N <= 64, K <= 32): adj_grad_small_kernel, one wave per graph, M and T in LDS, a launch of its own behind
// dense_pool_small_bwd_kernel (which is at its register cap).
#include "common.h"

namespace tgp {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int BK = 32, LDA_ROWMAJOR = BK + 1;  // the k-step and the odd row stride of an operand tile, as in gemm_mfma.h
// gemm_mfma.h's tile_row: the row of a [rows][BK + 1] tile served by slot t = 8 g + r (8 lanes per 128-byte row segment);
// the 8 rows one wave instruction stores are {4g .. 4g+3} u {4g+32 .. 4g+35}: distinct banks under the odd stride
__device__ __forceinline__ int tile_row(int t) {
  const int g = t >> 3, r = t & 7;
  return 4 * (g & 7) + (r & 3) + 32 * (r >> 2) + 64 * (g >> 3);
}

// c of the link loss from the forward's value (link = link_scale * norm): g link_scale / norm = g link_scale^2 / link;
// 0 where the loss is 0 (torch.norm's subgradient) -- the expression of train_rhs_kernel and dense_pool_small_bwd_kernel
__device__ __forceinline__ float link_coefficient(const float* g_link, const float* link_loss, float link_scale) {
  if (!g_link || !link_loss) return 0.f;
  const float lv = link_loss[0];
  return lv != 0.f ? g_link[0] * link_scale * link_scale / lv : 0.f;
}

// ------------------------------------------------------------------------------------------ beyond the one-wave kernels
struct AdjGradArgs {
  const float* T; long ldt, sT;  // [B][N][K] = S M
  const float* S; long lds, sS;  // [B][N][K] (a column block of a wider buffer: any row stride)
  const float* A;                // [B][N][N], read only where c != 0
  const float* gamma;            // [B] or NULL
  const float* q;                // [B][N] or NULL: |s_i|^2 is then formed here from the rows of S
  const float* g_link; const float* link_loss; float link_scale;
  float* dA;                     // [B][N][N]
  int N, K, tiles;               // tiles = cdiv(N, 128) in each direction
};

constexpr int AG_BM = 128, AG_THREADS = 512;                    // 8 waves as 4 (rows) x 2 (columns): 32 x 64 per wave
constexpr int AG_TILE_FLOATS = AG_BM * LDA_ROWMAJOR;            // one operand tile [128][BK + 1]
constexpr int AG_PATCH_FLOATS = (AG_THREADS / 64) * (32 * 36);  // the epilogue's per-wave patches [32][36]
constexpr int AG_LDS_FLOATS = (2 * AG_TILE_FLOATS > AG_PATCH_FLOATS ? 2 * AG_TILE_FLOATS : AG_PATCH_FLOATS) + AG_BM;

// one 16-byte piece of a row-major operand row: rows beyond `rows` and columns beyond K are zeros (the guarded edge)
__device__ __forceinline__ float4 ag_load(const float* base, long ld, int row, int rows, int k, int K, bool vec) {
  if (row >= rows || k >= K) return make_float4(0.f, 0.f, 0.f, 0.f);
  const float* p = base + static_cast<long>(row) * ld + k;
  if (vec && k + 3 < K) return *reinterpret_cast<const float4*>(p);
  float4 v = make_float4(p[0], 0.f, 0.f, 0.f);
  if (k + 1 < K) v.y = p[1];
  if (k + 2 < K) v.z = p[2];
  if (k + 3 < K) v.w = p[3];
  return v;
}

__global__ __launch_bounds__(AG_THREADS) void adj_grad_tile_kernel(AdjGradArgs g) {
  __shared__ __attribute__((aligned(16))) float smem[AG_LDS_FLOATS];
  float* Ts = smem;
  float* Ss = smem + AG_TILE_FLOATS;
  float* rowterm = smem + AG_LDS_FLOATS - AG_BM;  // gamma_b q_i of the tile's rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, lm = lane & 31, lk = lane >> 5;
  int bid = xcd_remap(blockIdx.x, gridDim.x);  // the tiles of one graph share T and S through one L2
  const int tn = bid % g.tiles; bid /= g.tiles;
  const int tm = bid % g.tiles;
  const int b = bid / g.tiles;
  const int N = g.N, K = g.K, m0 = tm * AG_BM, n0 = tn * AG_BM;
  const float* __restrict__ T = g.T + static_cast<long>(b) * g.sT;
  const float* __restrict__ S = g.S + static_cast<long>(b) * g.sS;
  const float* __restrict__ A = g.A ? g.A + static_cast<long>(b) * N * N : nullptr;
  float* __restrict__ D = g.dA + static_cast<long>(b) * N * N;
  const float c = A ? link_coefficient(g.g_link, g.link_loss, g.link_scale) : 0.f;  // (uniform)
  const bool use_a = c != 0.f;
  const bool vec_t = (g.ldt & 3) == 0 && (reinterpret_cast<uintptr_t>(T) & 15) == 0;
  const bool vec_s = (g.lds & 3) == 0 && (reinterpret_cast<uintptr_t>(S) & 15) == 0;
  // interior tiles of an aligned output leave (and read A) in 16-byte vectors; edge tiles element by element
  const bool interior = m0 + AG_BM <= N && n0 + AG_BM <= N && (N & 3) == 0 && (reinterpret_cast<uintptr_t>(D) & 15) == 0 &&
                        (!use_a || (reinterpret_cast<uintptr_t>(A) & 15) == 0);

  // the rows' rank-one term, before the k-loop's first barrier
  if (tid < AG_BM) {
    float rt = 0.f;
    const int row = m0 + tid;
    if (g.gamma && row < N) {
      float qi;
      if (g.q) {
        qi = g.q[static_cast<long>(b) * N + row];
      } else {
        qi = 0.f;
        const float* sr = S + static_cast<long>(row) * g.lds;
        for (int k = 0; k < K; ++k) qi = fmaf(sr[k], sr[k], qi);
      }
      rt = g.gamma[b] * qi;
    }
    rowterm[tid] = rt;
  }
  // the A tile is requested ahead of the product (interior tiles: the piece each lane adds in the epilogue)
  const int r8 = lane >> 3, c4 = (lane & 7) * 4;
  float4 apre[2][4];
  if (interior && use_a) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int qd = 0; qd < 4; ++qd)
        apre[j][qd] = *reinterpret_cast<const float4*>(A + static_cast<long>(m0 + wm * 32 + r8 + 8 * qd) * N + n0 +
                                                       wn * 64 + j * 32 + c4);
  }

  // operand staging: two 16-byte pieces of each tile per thread and k-step; 8 lanes per 128-byte row segment, rows in
  // tile_row order (conflict-free stores into the odd-stride tile)
  const int kc = (tid & 7) * 4;
  int trow[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) trow[i] = tile_row((tid >> 3) + i * (AG_THREADS / 8));
  float4 rt4[2], rs4[2];
  auto load_stage = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      rt4[i] = ag_load(T, g.ldt, m0 + trow[i], N, k0 + kc, K, vec_t);
      rs4[i] = ag_load(S, g.lds, n0 + trow[i], N, k0 + kc, K, vec_s);
    }
  };
  auto store_stage = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float* dt = Ts + trow[i] * LDA_ROWMAJOR + kc;
      dt[0] = rt4[i].x; dt[1] = rt4[i].y; dt[2] = rt4[i].z; dt[3] = rt4[i].w;
      float* ds = Ss + trow[i] * LDA_ROWMAJOR + kc;
      ds[0] = rs4[i].x; ds[1] = rs4[i].y; ds[2] = rs4[i].z; ds[3] = rs4[i].w;
    }
  };

  f32x16 acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  const int a_off = (wm * 32 + lm) * LDA_ROWMAJOR + lk;
  const int b_off = (wn * 64 + lm) * LDA_ROWMAJOR + lk;
  const int nk = (K + BK - 1) / BK;
  load_stage(0);
  for (int t = 0; t < nk; ++t) {
    __syncthreads();  // the previous step's operand reads are done (first step: rowterm is written)
    store_stage();
    __syncthreads();
    if (t + 1 < nk) load_stage((t + 1) * BK);  // in flight under this step's MFMAs
#pragma unroll
    for (int p = 0; p < BK / 2; ++p) {
      const float a = Ts[a_off + 2 * p];
      const float b0 = Ss[b_off + 2 * p], b1 = Ss[b_off + 32 * LDA_ROWMAJOR + 2 * p];
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[1], 0, 0, 0);
    }
  }
  __syncthreads();  // the tiles are spent: their LDS holds the epilogue's patches from here on

  // ---- epilogue: C/D layout col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) -----------------------------
  if (interior) {  // (workgroup-uniform)
    float* patch = smem + wave * (32 * 36);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int r = 0; r < 16; ++r) patch[((r & 3) + 8 * (r >> 2) + 4 * lk) * 36 + lm] = acc[j][r];
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        const int rr = r8 + 8 * qd;
        float4 v = *reinterpret_cast<const float4*>(patch + rr * 36 + c4);
        const float rt = rowterm[wm * 32 + rr];
        v.x += rt; v.y += rt; v.z += rt; v.w += rt;
        if (use_a) {
          const float4 a = apre[j][qd];
          v.x = fmaf(c, a.x, v.x); v.y = fmaf(c, a.y, v.y); v.z = fmaf(c, a.z, v.z); v.w = fmaf(c, a.w, v.w);
        }
        *reinterpret_cast<float4*>(D + static_cast<long>(m0 + wm * 32 + rr) * N + n0 + wn * 64 + j * 32 + c4) = v;
      }
      __builtin_amdgcn_wave_barrier();
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = n0 + wn * 64 + j * 32 + lm;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int lrow = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk, row = m0 + lrow;
      if (row < N && col < N) {
        const long e = static_cast<long>(row) * N + col;
        float v = acc[j][r] + rowterm[lrow];
        if (use_a) v = fmaf(c, A[e], v);
        D[e] = v;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ one wave per graph
struct AdjGradSmallArgs {
  const float* S; const float* A;
  const float* ga;          // [B,K,K] or NULL: the post-processing backward's gradient of R
  const float* g_raw;       // [B,K,K] or NULL: an upstream gradient of R itself
  const float* raw;         // [B,K,K]: R of the forward (its trace is MinCut's numerator); needed with g_terms / g_mean_cut
  const float* g_terms;     // [2,B] or NULL: row 0 = upstream gradients of the per-graph cut terms
  const float* g_mean_cut;  // 0-dim or NULL: upstream gradient of their batch mean
  const float* g_link; const float* link_loss; float link_scale, loss_eps;
  float* dA;
  int B, N, K;
};

constexpr int AGS_WAVES = 4, AGS_N = 64, AGS_K = 32, AGS_LDT = 36;
constexpr int AGS_WAVE_FLOATS = AGS_K * AGS_K + AGS_N * AGS_LDT;  // M [32][32], T [64][36]

__global__ __launch_bounds__(64 * AGS_WAVES) void adj_grad_small_kernel(AdjGradSmallArgs p) {
  __shared__ __attribute__((aligned(16))) float smem[AGS_WAVES * AGS_WAVE_FLOATS];
  const int lane = lane_id();
  const int w = __builtin_amdgcn_readfirstlane(wave_id());
  const int b = blockIdx.x * AGS_WAVES + w;
  if (b >= p.B) return;  // (no workgroup barrier below: the waves are independent)
  float* Ms = smem + w * AGS_WAVE_FLOATS;
  float* Ts = Ms + AGS_K * AGS_K;
  const int N = p.N, K = p.K;
  const float* Sb = p.S + static_cast<long>(b) * N * K;
  const float* Ab = p.A ? p.A + static_cast<long>(b) * N * N : nullptr;
  float* Db = p.dA + static_cast<long>(b) * N * N;
  const long kk = static_cast<long>(b) * K * K;

  // lane = node: its row of S in registers (zeros beyond N and K), q = |s|^2
  float s[AGS_K];
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < AGS_K; ++k) {
    s[k] = (lane < N && k < K) ? Sb[lane * K + k] : 0.f;
    q = fmaf(s[k], s[k], q);
  }
  const float c = Ab ? link_coefficient(p.g_link, p.link_loss, p.link_scale) : 0.f;  // (uniform)
  float g_cut = p.g_terms ? p.g_terms[b] : 0.f;
  if (p.g_mean_cut) g_cut += p.g_mean_cut[0] / static_cast<float>(p.B);
  float diag = -c, gamma = 0.f;
  if (g_cut != 0.f) {  // (uniform) den_b = sum_ij A_ij q_i over all of A, lane = column; num_b = trace(R)
    float part = 0.f;
    for (int i = 0; i < N; ++i) {
      const float a = lane < N ? Ab[i * N + lane] : 0.f;
      part = fmaf(a, __shfl(q, i, WAVE), part);
    }
    const float den = wave_sum(part) + p.loss_eps;
    const float num = wave_sum(lane < K ? p.raw[kk + lane * K + lane] : 0.f);
    diag -= g_cut / den;
    gamma = g_cut * num / (den * den);
  }
  // M = ga + g_raw + diag I into LDS, zero padded to 32 x 32
#pragma unroll
  for (int t = 0; t < AGS_K * AGS_K / 64; ++t) {
    const int e = lane + 64 * t, m = e >> 5, k = e & 31;
    float v = 0.f;
    if (m < K && k < K) {
      if (p.ga) v += p.ga[kk + m * K + k];
      if (p.g_raw) v += p.g_raw[kk + m * K + k];
      if (m == k) v += diag;
    }
    Ms[e] = v;
  }
  __builtin_amdgcn_wave_barrier();
  // T_i = s_i M (lane = node i), four columns at a time: M's rows are broadcast reads
#pragma unroll
  for (int kb = 0; kb < AGS_K / 4; ++kb) {
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (4 * kb < K) {  // (uniform)
#pragma unroll
      for (int m = 0; m < AGS_K; ++m) {
        const float4 mv = *reinterpret_cast<const float4*>(Ms + m * AGS_K + 4 * kb);
        t.x = fmaf(s[m], mv.x, t.x); t.y = fmaf(s[m], mv.y, t.y); t.z = fmaf(s[m], mv.z, t.z); t.w = fmaf(s[m], mv.w, t.w);
      }
    }
    *reinterpret_cast<float4*>(Ts + lane * AGS_LDT + 4 * kb) = t;
  }
  __builtin_amdgcn_wave_barrier();
  // dA[i][j] = <T_i, s_j> + gamma q_i + c A_ij, lane = column j: a row leaves as one contiguous run
  for (int i = 0; i < N; ++i) {
    float v = 0.f;
#pragma unroll
    for (int kb = 0; kb < AGS_K / 4; ++kb) {
      if (4 * kb < K) {  // (uniform)
        const float4 tv = *reinterpret_cast<const float4*>(Ts + i * AGS_LDT + 4 * kb);
        v = fmaf(tv.x, s[4 * kb], v); v = fmaf(tv.y, s[4 * kb + 1], v);
        v = fmaf(tv.z, s[4 * kb + 2], v); v = fmaf(tv.w, s[4 * kb + 3], v);
      }
    }
    v = fmaf(gamma, __shfl(q, i, WAVE), v);
    if (lane < N) {
      if (c != 0.f) v = fmaf(c, Ab[i * N + lane], v);
      Db[i * N + lane] = v;
    }
  }
}

}  // namespace tgp

using namespace tgp;

extern "C" int tgp_dense_pool_adj_grad_f32(const float* S, int64_t lds, int64_t sS, const float* A, const float* M,
                                           int64_t ldm, int64_t sM, const float* gamma, const float* q,
                                           const float* g_link, const float* link_loss, float link_scale, int64_t B,
                                           int64_t N, int64_t K, float* T, float* dA, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(B >= 0 && N >= 0 && K >= 0, TGP_ERR_INVALID, "tgp_dense_pool_adj_grad_f32: negative size");
  if (B == 0 || N == 0) return TGP_OK;
  TGP_REQUIRE(K >= 1 && S && M && T && dA, TGP_ERR_INVALID, "tgp_dense_pool_adj_grad_f32: S, M, T and dA are required, K >= 1");
  TGP_REQUIRE(lds >= K && ldm >= K && sS >= 0 && sM >= 0, TGP_ERR_INVALID,
              "tgp_dense_pool_adj_grad_f32: a row stride below K or a negative batch stride");
  TGP_REQUIRE(!g_link || (link_loss && A), TGP_ERR_INVALID,
              "tgp_dense_pool_adj_grad_f32: g_link needs the forward's link loss and A");
  TGP_REQUIRE(T != dA && static_cast<const float*>(dA) != A && static_cast<const float*>(dA) != S, TGP_ERR_INVALID,
              "tgp_dense_pool_adj_grad_f32: dA aliases an operand");
  TGP_REQUIRE(N < (1ll << 31) && K < (1ll << 31), TGP_ERR_RANGE, "tgp_dense_pool_adj_grad_f32: too large");
  const int64_t tiles = (N + AG_BM - 1) / AG_BM;
  TGP_REQUIRE(B * tiles * tiles < (1ll << 31), TGP_ERR_RANGE, "tgp_dense_pool_adj_grad_f32: grid too large");
  // T = S M: N K^2 flops
  const int st = tgp_bmm_f32(S, M, T, B, N, K, K, 0, lds, ldm, K, sS, sM, N * K, stream_);
  if (st != TGP_OK) return st;
  AdjGradArgs g{T, K, N * K, S, lds, sS, A, gamma, q, g_link, link_loss, link_scale, dA,
                static_cast<int>(N), static_cast<int>(K), static_cast<int>(tiles)};
  hipLaunchKernelGGL(adj_grad_tile_kernel, dim3(static_cast<unsigned>(B * tiles * tiles)), dim3(AG_THREADS), 0, stream, g);
  return check_launch("tgp_dense_pool_adj_grad_f32");
}

extern "C" int tgp_dense_pool_adj_grad_small_f32(const float* S, const float* A, const float* ga, const float* g_raw,
                                                 const float* raw, const float* g_terms, const float* g_mean_cut,
                                                 const float* g_link, const float* link_loss, float link_scale,
                                                 float loss_eps, int64_t B, int64_t N, int64_t K, float* dA,
                                                 void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  TGP_REQUIRE(B >= 0 && N >= 0 && K >= 0, TGP_ERR_INVALID, "tgp_dense_pool_adj_grad_small_f32: negative size");
  if (B == 0 || N == 0) return TGP_OK;
  TGP_REQUIRE(K >= 1 && S && dA, TGP_ERR_INVALID, "tgp_dense_pool_adj_grad_small_f32: S and dA are required, K >= 1");
  TGP_REQUIRE(N <= AGS_N && K <= AGS_K, TGP_ERR_INVALID,
              "tgp_dense_pool_adj_grad_small_f32: one wave per graph takes N <= 64 and K <= 32");
  TGP_REQUIRE(!(g_terms || g_mean_cut) || (A && raw), TGP_ERR_INVALID,
              "tgp_dense_pool_adj_grad_small_f32: the cut term needs A and the forward's raw S^T A S");
  TGP_REQUIRE(!g_link || (link_loss && A), TGP_ERR_INVALID,
              "tgp_dense_pool_adj_grad_small_f32: g_link needs the forward's link loss and A");
  TGP_REQUIRE(static_cast<const float*>(dA) != A && static_cast<const float*>(dA) != S, TGP_ERR_INVALID,
              "tgp_dense_pool_adj_grad_small_f32: dA aliases an operand");
  TGP_REQUIRE(B < (1ll << 31), TGP_ERR_RANGE, "tgp_dense_pool_adj_grad_small_f32: too many graphs");
  AdjGradSmallArgs p{S, A, ga, g_raw, raw, g_terms, g_mean_cut, g_link, link_loss, link_scale, loss_eps, dA,
                     static_cast<int>(B), static_cast<int>(N), static_cast<int>(K)};
  hipLaunchKernelGGL(adj_grad_small_kernel, dim3(static_cast<unsigned>((B + AGS_WAVES - 1) / AGS_WAVES)),
                     dim3(64 * AGS_WAVES), 0, stream, p);
  return check_launch("tgp_dense_pool_adj_grad_small_f32");
}
