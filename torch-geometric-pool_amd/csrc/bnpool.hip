// BN-Pool's reconstruction loss (reference poolers/bnpool.py:359-447, utils/losses.py:1268-1356) without the [B,N,N]
// logit tensor: every 32x32 tile of L = (S K) S^T is formed on the fp32 matrix cores from operands held on chip, meets
// the matching tile of the adjacency in registers and leaves as three numbers (forward) or as a 32-row slice of
// P = G S or Q = G^T T (backward).  include/tgp_hip.h holds the contract.
//
// One kernel, three modes.  A workgroup owns 32 COLUMNS c of the tile grid (the MFMA result keeps its column on the lane
// and its rows in the 16 accumulator registers); its four waves split the row blocks r = wave, wave + 4, ... and run
// independently (each stages the tiles it reads itself; only the final sum of the four slices meets at a barrier):
//   X[r][c] = sum_k U[r][k] V[c][k]         V's fragment stays in registers, a 32-row tile of U is staged in LDS
//   MODE 0  U = T, V = S: X = L[i=r][j=c];  bce(X, A[r][c]) summed by class (a != 0 | a == 0), one record per workgroup
//   MODE 1  U = T, V = S: Gx[r][c] = G[i=r][j=c];      out[c] = Q_c = sum_r Gx[r][c] T_r
//   MODE 2  U = S, V = T: X = L[i=c][j=r], Gx[r][c] = G[i=c][j=r] (A's tile transposed through LDS);
//                                                       out[c] = P_c = sum_r Gx[r][c] S_r
// The second product sums over the ROW index of the tile, so the accumulator registers are its B operand as they stand
// (register q, lane half h = rows acc_row(q, h)); nothing of G is written.  The four waves' slices are added in wave
// order through LDS: no float atomics anywhere, every result is reproducible bit for bit.
#include "common.h"

namespace tgp {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BNP_TILE = 32;
constexpr int BNP_WAVES = 4;
constexpr int BNP_MAX_K = 256;
constexpr int BNP_REC = 4;  // floats per record: sum over a != 0, sum over a == 0, the count of a != 0 (int bits), unused

// LDS written by some lanes of a wave and read by others of the SAME wave: the wave's LDS operations execute in issue
// order, so the compiler only has to keep them in program order
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// row of the 32x32 MFMA result that accumulator register q of a lane in half h (lane >> 5) holds
__device__ __forceinline__ int acc_row(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

// (two workgroups per CU wherever the registers allow it: 256 per lane, which K <= 128 fits except in the transposed mode)
template <int KT, int MODE>
__global__ __launch_bounds__(256, (KT <= 2 || (KT == 4 && MODE != 2)) ? 2 : 1) void bnpool_tile_kernel(
    const float* __restrict__ U, const float* __restrict__ V, const float* __restrict__ A,
    const uint8_t* __restrict__ mask, const float* __restrict__ g, const float* __restrict__ stats, int N, int K,
    float* __restrict__ out) {
  constexpr int KP = KT * 32, LDK = KP + 1, KS = KT * 16;
  __shared__ float u_lds[BNP_WAVES][BNP_TILE * LDK];
  __shared__ float a_lds[MODE == 2 ? BNP_WAVES : 1][MODE == 2 ? BNP_TILE * 33 : 1];
  __shared__ float red[BNP_WAVES][4];

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, lm = lane & 31, h = lane >> 5;
  const int b = blockIdx.y, cbase = blockIdx.x * BNP_TILE;
  const long gb = static_cast<long>(b) * N;
  const float* Ub = U + gb * K;
  const float* Vb = V + gb * K;
  const float* Ab = A + gb * N;
  const uint8_t* mb = mask ? mask + gb : nullptr;
  const int nrb = (N + BNP_TILE - 1) / BNP_TILE;
  float* ul = u_lds[w];

  // this lane's column and V's fragment: V[c][2 s + h]
  const int c = cbase + lm;
  const bool cvalid = c < N && (!mb || mb[c] != 0);
  float vr[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int k = 2 * s + h;
    vr[s] = (c < N && k < K) ? Vb[static_cast<long>(c) * K + k] : 0.f;
  }
  // 16-byte loads of U's rows when every row starts on a 16-byte boundary
  const bool vec4 = (K & 3) == 0 && (reinterpret_cast<uintptr_t>(U) & 15) == 0;
  float cw = 1.f, coef = 0.f;
  if (MODE != 0) {
    cw = stats[2 * b];
    coef = g[b] / stats[2 * b + 1];
  }

  float pos = 0.f, neg = 0.f;
  int cnt = 0;
  f32x16 oacc[MODE == 0 ? 1 : KT];
  if (MODE != 0) {
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
      for (int q = 0; q < 16; ++q) oacc[t][q] = 0.f;
  }

  for (int it = 0; it * BNP_WAVES < nrb; ++it) {
    const int rb = it * BNP_WAVES + w;
    const bool active = rb < nrb;
    const int rbase = rb * BNP_TILE;
    float av[16];
    unsigned rowbits = 0;
    if (active) {
      // the 32-row tile of U, zero beyond N and K: the loads of a batch are all issued before the first LDS write
      if (vec4) {
        constexpr int BATCH = 8, PER_LANE = BNP_TILE * KP / 4 / 64;  // float4 per lane: 4 KT
#pragma unroll
        for (int c0 = 0; c0 < PER_LANE; c0 += BATCH) {
          float4 tmp[BATCH];
#pragma unroll
          for (int u = 0; u < BATCH && c0 + u < PER_LANE; ++u) {
            const int idx = (c0 + u) * 64 + lane, row = idx / (KP / 4), k = 4 * (idx % (KP / 4)), r = rbase + row;
            tmp[u] = (r < N && k < K) ? *reinterpret_cast<const float4*>(Ub + static_cast<long>(r) * K + k)
                                      : make_float4(0.f, 0.f, 0.f, 0.f);
          }
#pragma unroll
          for (int u = 0; u < BATCH && c0 + u < PER_LANE; ++u) {
            const int idx = (c0 + u) * 64 + lane, row = idx / (KP / 4), k = 4 * (idx % (KP / 4));
            float* d = ul + row * LDK + k;
            d[0] = tmp[u].x; d[1] = tmp[u].y; d[2] = tmp[u].z; d[3] = tmp[u].w;
          }
        }
      } else {
        constexpr int BATCH = 16, PER_LANE = BNP_TILE * KP / 64;
#pragma unroll 1
        for (int c0 = 0; c0 < PER_LANE; c0 += BATCH) {
          float tmp[BATCH];
#pragma unroll
          for (int u = 0; u < BATCH; ++u) {
            const int idx = (c0 + u) * 64 + lane, row = idx / KP, k = idx % KP, r = rbase + row;
            tmp[u] = (r < N && k < K) ? Ub[static_cast<long>(r) * K + k] : 0.f;
          }
#pragma unroll
          for (int u = 0; u < BATCH; ++u) {
            const int idx = (c0 + u) * 64 + lane, row = idx / KP, k = idx % KP;
            ul[row * LDK + k] = tmp[u];
          }
        }
      }
      if (MODE == 2) {  // A[i = cbase + ii][j = rbase + lm]: rows of 32 consecutive floats, transposed on the way out
        float* at = a_lds[w];
#pragma unroll
        for (int p = 0; p < 16; ++p) {
          const int ii = 2 * p + h, i = cbase + ii, j = rbase + lm;
          at[ii * 33 + lm] = (i < N && j < N) ? Ab[static_cast<long>(i) * N + j] : 0.f;
        }
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int r = rbase + acc_row(q, h);
        const bool ok = cvalid && r < N && (!mb || mb[r] != 0);
        rowbits |= ok ? (1u << q) : 0u;
        if (MODE != 2) av[q] = ok ? Ab[static_cast<long>(r) * N + c] : 0.f;
      }
    }
    wave_sync();  // (each wave reads only the tiles it staged itself)
    if (active) {
      f32x16 x;
#pragma unroll
      for (int q = 0; q < 16; ++q) x[q] = 0.f;
#pragma unroll
      for (int s = 0; s < KS; ++s)
        x = __builtin_amdgcn_mfma_f32_32x32x2f32(ul[lm * LDK + 2 * s + h], vr[s], x, 0, 0, 0);
      if (MODE == 2) {
        const float* at = a_lds[w];
#pragma unroll
        for (int q = 0; q < 16; ++q) av[q] = at[lm * 33 + acc_row(q, h)];
      }
      if (MODE == 0) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const float l = x[q], a = av[q];
          const float bce = fmaxf(l, 0.f) - l * a + log1pf(expf(-fabsf(l)));
          const bool ok = (rowbits >> q) & 1u;
          const bool edge = ok && a != 0.f;
          pos += edge ? bce : 0.f;
          neg += (ok && !edge) ? bce : 0.f;
          cnt += edge ? 1 : 0;
        }
      } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const float l = x[q], a = av[q];
          const float e = expf(-fabsf(l));
          const float sig = (l >= 0.f ? 1.f : e) / (1.f + e);
          const bool ok = (rowbits >> q) & 1u;
          x[q] = ok ? (a != 0.f ? cw : 1.f) * (sig - a) * coef : 0.f;
        }
        // out^T[k][c] += sum_r U[r][k] Gx[r][c]: the tile as it stands is the B operand of k-step q
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
          for (int q = 0; q < 16; ++q)
            oacc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ul[acc_row(q, h) * LDK + 32 * t + lm], x[q], oacc[t], 0, 0, 0);
      }
    }
    wave_sync();
  }

  if (MODE == 0) {
    // the order of wave_butterfly (wave.h), written out: a call here changes the kernel's instruction stream
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      pos += __shfl_xor(pos, off);
      neg += __shfl_xor(neg, off);
      cnt += __shfl_xor(cnt, off);
    }
    if (lane == 0) {
      red[w][0] = pos;
      red[w][1] = neg;
      red[w][2] = __int_as_float(cnt);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      float p = 0.f, n = 0.f;
      int e = 0;
      for (int i = 0; i < BNP_WAVES; ++i) {
        p += red[i][0];
        n += red[i][1];
        e += __float_as_int(red[i][2]);
      }
      float* rec = out + (static_cast<long>(b) * gridDim.x + blockIdx.x) * BNP_REC;
      rec[0] = p;
      rec[1] = n;
      rec[2] = __int_as_float(e);
      rec[3] = 0.f;
    }
  } else {
    // the four waves' slices, [column][k] in each wave's tile buffer, added in wave order
    wave_sync();
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
      for (int q = 0; q < 16; ++q) ul[lm * LDK + 32 * t + acc_row(q, h)] = oacc[t][q];
    __syncthreads();
    for (int idx = threadIdx.x; idx < BNP_TILE * K; idx += 256) {
      const int cl = idx / K, k = idx % K;
      if (cbase + cl < N) {
        const int o = cl * LDK + k;
        out[(gb + cbase + cl) * K + k] = ((u_lds[0][o] + u_lds[1][o]) + u_lds[2][o]) + u_lds[3][o];
      }
    }
  }
}

// one wave per graph: the records of its column blocks in a fixed order, the node count, the class weight
__global__ __launch_bounds__(64) void bnpool_tail_kernel(const float* __restrict__ part, int ncb,
                                                         const uint8_t* __restrict__ mask, int N,
                                                         float* __restrict__ rec, float* __restrict__ stats) {
  const int b = blockIdx.x, lane = threadIdx.x;
  float pos = 0.f, neg = 0.f;
  long long e = 0, n = 0;
  for (int i = lane; i < ncb; i += 64) {
    const float* r = part + (static_cast<long>(b) * ncb + i) * BNP_REC;
    pos += r[0];
    neg += r[1];
    e += __float_as_int(r[2]);
  }
  if (mask) {
    for (int i = lane; i < N; i += 64) n += mask[static_cast<long>(b) * N + i] != 0 ? 1 : 0;
  }
  // the order of wave_butterfly (wave.h), written out: a call here changes the kernel's instruction stream
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    pos += __shfl_xor(pos, off);
    neg += __shfl_xor(neg, off);
    e += __shfl_xor(e, off);
    n += __shfl_xor(n, off);
  }
  if (lane == 0) {
    if (!mask) n = N;
    const long long n2 = n * n;
    const long long none = n2 - e > 1 ? n2 - e : 1, ne = e > 1 ? e : 1;
    const float cw = static_cast<float>(none) / static_cast<float>(ne);
    const float n2f = static_cast<float>(n2);
    rec[b] = (cw * pos + neg) / n2f;
    stats[2 * b] = cw;
    stats[2 * b + 1] = n2f;
  }
}

template <int MODE>
void launch_tile(int kt, dim3 grid, hipStream_t stream, const float* U, const float* V, const float* A,
                 const uint8_t* mask, const float* g, const float* stats, int N, int K, float* out) {
  switch (kt) {
    case 1:
      hipLaunchKernelGGL((bnpool_tile_kernel<1, MODE>), grid, dim3(256), 0, stream, U, V, A, mask, g, stats, N, K, out);
      break;
    case 2:
      hipLaunchKernelGGL((bnpool_tile_kernel<2, MODE>), grid, dim3(256), 0, stream, U, V, A, mask, g, stats, N, K, out);
      break;
    case 4:
      hipLaunchKernelGGL((bnpool_tile_kernel<4, MODE>), grid, dim3(256), 0, stream, U, V, A, mask, g, stats, N, K, out);
      break;
    default:
      hipLaunchKernelGGL((bnpool_tile_kernel<8, MODE>), grid, dim3(256), 0, stream, U, V, A, mask, g, stats, N, K, out);
      break;
  }
}

inline int k_tiles(int64_t K) { return K <= 32 ? 1 : K <= 64 ? 2 : K <= 128 ? 4 : 8; }

}  // namespace
}  // namespace tgp

using namespace tgp;

extern "C" int tgp_bnpool_max_clusters(void) { return BNP_MAX_K; }

extern "C" int64_t tgp_bnpool_part_floats(int64_t B, int64_t N) {
  if (B < 0 || N < 0) return 0;
  return B * ((N + BNP_TILE - 1) / BNP_TILE) * BNP_REC;
}

extern "C" int tgp_bnpool_rec_fwd_f32(const float* T, const float* S, const float* A, const uint8_t* mask, int64_t B,
                                      int64_t N, int64_t K, float* part, int64_t part_floats, float* rec, float* stats,
                                      void* stream_) {
  TGP_REQUIRE(B >= 0 && N >= 1 && K >= 1, TGP_ERR_INVALID, "tgp_bnpool_rec_fwd_f32: bad shape");
  TGP_REQUIRE(K <= BNP_MAX_K, TGP_ERR_RANGE, "tgp_bnpool_rec_fwd_f32: K > 256");
  TGP_REQUIRE(B < 65536 && N < (1ll << 24), TGP_ERR_RANGE, "tgp_bnpool_rec_fwd_f32: too large");
  if (B == 0) return TGP_OK;
  TGP_REQUIRE(T && S && A && part && rec && stats, TGP_ERR_INVALID, "tgp_bnpool_rec_fwd_f32: null pointer");
  TGP_REQUIRE(part_floats >= tgp_bnpool_part_floats(B, N), TGP_ERR_INVALID,
              "tgp_bnpool_rec_fwd_f32: workspace too small");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int ncb = cdiv(N, BNP_TILE);
  const dim3 grid(static_cast<unsigned>(ncb), static_cast<unsigned>(B));
  launch_tile<0>(k_tiles(K), grid, stream, T, S, A, mask, nullptr, nullptr, static_cast<int>(N), static_cast<int>(K),
                 part);
  int st = check_launch("tgp_bnpool_rec_fwd_f32");
  if (st != TGP_OK) return st;
  hipLaunchKernelGGL(bnpool_tail_kernel, dim3(static_cast<unsigned>(B)), dim3(64), 0, stream, part, ncb, mask,
                     static_cast<int>(N), rec, stats);
  return check_launch("tgp_bnpool_rec_fwd_f32 (tail)");
}

extern "C" int tgp_bnpool_rec_bwd_f32(const float* T, const float* S, const float* A, const uint8_t* mask,
                                      const float* g, const float* stats, int64_t B, int64_t N, int64_t K, float* P,
                                      float* Q, void* stream_) {
  TGP_REQUIRE(B >= 0 && N >= 1 && K >= 1, TGP_ERR_INVALID, "tgp_bnpool_rec_bwd_f32: bad shape");
  TGP_REQUIRE(K <= BNP_MAX_K, TGP_ERR_RANGE, "tgp_bnpool_rec_bwd_f32: K > 256");
  TGP_REQUIRE(B < 65536 && N < (1ll << 24), TGP_ERR_RANGE, "tgp_bnpool_rec_bwd_f32: too large");
  if (B == 0) return TGP_OK;
  TGP_REQUIRE(T && S && A && g && stats && P && Q, TGP_ERR_INVALID, "tgp_bnpool_rec_bwd_f32: null pointer");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const dim3 grid(static_cast<unsigned>(cdiv(N, BNP_TILE)), static_cast<unsigned>(B));
  launch_tile<1>(k_tiles(K), grid, stream, T, S, A, mask, g, stats, static_cast<int>(N), static_cast<int>(K), Q);
  int st = check_launch("tgp_bnpool_rec_bwd_f32 (Q)");
  if (st != TGP_OK) return st;
  launch_tile<2>(k_tiles(K), grid, stream, S, T, A, mask, g, stats, static_cast<int>(N), static_cast<int>(K), P);
  return check_launch("tgp_bnpool_rec_bwd_f32 (P)");
}
