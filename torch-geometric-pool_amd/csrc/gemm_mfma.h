// fp32-MFMA batched GEMM of the dense path (LDS-tiled, buffer-descriptor loads) and its launchers.
//
// GEMM kernel: 128x128 output tile per 512-thread workgroup: 8 waves as 4(M) x 2(N), each wave owns
// 32 x 64 = two 32x32 MFMA tiles (32 accumulator VGPRs); two waves per SIMD so one wave's LDS
// operand fetch hides behind the other's MFMAs.  BK = 32, register-staged double-buffered LDS,
// operands for k-step t+1 are fetched from LDS before the MFMAs of step t are issued.
// fp32 MFMA needs only one operand dword per lane per 64-cycle instruction, so LDS bandwidth is a
// non-issue; layouts are chosen for conflict-free ds_write/ds_read and coalesced global loads:
//   * row-major operand tile  (A of A.S):     LDS [128][BK+1]  (odd stride => conflict free)
//   * k-major operand tile    (S, U, X, A^T): LDS [BK][128]    (lanes read consecutive floats)
#pragma once
#include <stdlib.h>
#include <type_traits>

#include "common.h"

namespace tgp {


typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BK = 32;
#ifndef TGP_OPERAND_PREFETCH
#define TGP_OPERAND_PREFETCH 1
#endif
#ifndef TGP_LOAD_AT
#define TGP_LOAD_AT 7
#endif
#ifndef TGP_STORE_AT
#define TGP_STORE_AT 3
#endif
#ifndef TGP_STEADY_LOOP
#define TGP_STEADY_LOOP 1
#endif
#ifndef TGP_SPREAD
#define TGP_SPREAD 1
#endif
#ifndef TGP_MIRROR_ROWS
#define TGP_MIRROR_ROWS 1
#endif
#ifndef TGP_VEC_EPILOGUE
#define TGP_VEC_EPILOGUE 1
#endif

constexpr int LDA_ROWMAJOR = BK + 1;

// MODE 3 (U = A S of the dense poolers, see launch_gemm_skip_zeros): a k-step whose A chunk (128 x BK, as 1024 groups
// of 4 consecutive values) has at most this many groups holding a nonzero, and whose S rows are all finite, skips its
// MFMAs and accumulates over the nonzeros alone.  Set from the density sweep of tools/c2_density_sweep.py (DESIGN.md
// section 4): from about 6 % nonzeros (1 - 0.94^4 = 22 % of the groups) the MFMAs win at C2.
#ifndef TGP_SPARSE_CHUNK_GROUPS
#define TGP_SPARSE_CHUNK_GROUPS 224
#endif
// ... and after this many dense k-steps in a row the workgroup runs the rest of its k-loop in the plain MODE 0 form: no
// more records and decisions (they cost a dense input ~12 % of the launch when taken at every step).  Measured on
// uniformly random A only: a row panel that meets two dense chunks early (a dense diagonal block of community-ordered
// nodes, say) multiplies the rest of its k-range in full -- the results are the same, the skipping is lost there.
// With a row-major A the 16-wave 128 x 128 tile first takes its k-range in 128-column chunks (128 x 128, 4096 groups)
// for as long as they are sparse -- the wide front-end in gemm_f32_mfma_kernel -- and the 32-column stages above run
// from the first chunk that is not.  Same share of the groups as the narrow threshold (4 x 224), confirmed by the same
// sweep (profiles/adj_front.md).
#ifndef TGP_SPARSE_WIDE_GROUPS
#define TGP_SPARSE_WIDE_GROUPS 896
#endif
#ifndef TGP_DENSE_RUN
#define TGP_DENSE_RUN 2
#endif
// MODE 4 tail, each measured on its own (profiles/c2_tail.md).  TGP_FOLD_SKIP_ACC: a workgroup that ran no MFMA in its
// k-loop writes the walk's sums to the tail's U operand directly, without the accumulators' trip through LDS.
// TGP_FOLD_SPLIT: the tail's MFMAs in two phases, S^T U first; its result is parked in LDS and stored under S^T X.
#ifndef TGP_FOLD_SKIP_ACC
#define TGP_FOLD_SKIP_ACC 1
#endif
#ifndef TGP_FOLD_SPLIT
#define TGP_FOLD_SPLIT 1
#endif
// The two-phase tail's exits, each measured on its own (profiles/c2_slab_blocks.md).  TGP_FOLD_BLOCKS: both slab sets
// leave in the accumulators' own block order (fold_slab_floats), one 16-byte store per lane and 16 x 16 block, with no
// park in LDS and no barrier inside the X-part; post_rows_kernel<true> reads them through the inverse map.
// TGP_FOLD_SLAB_WT (with TGP_FOLD_BLOCKS): those slab stores are write-through (sc1), so the slabs are on their way to
// memory while the X-part still multiplies and the next launch does not wait for 25 MB of dirty lines.
#ifndef TGP_FOLD_BLOCKS
#define TGP_FOLD_BLOCKS 1
#endif
#ifndef TGP_FOLD_SLAB_WT
#define TGP_FOLD_SLAB_WT 1
#endif
#if !TGP_FOLD_SPLIT
#undef TGP_FOLD_BLOCKS
#define TGP_FOLD_BLOCKS 0
#endif
// TGP_FOLD_X_LATE (with TGP_FOLD_BLOCKS; profiles/c2_xpool.md): the tail multiplies S_r^T U_r only.  X_r is not requested,
// no S^T X slabs are written, and post_rows_kernel<true> forms x_pool = S^T X from S and X itself, in the blocks, chains
// and tile order the X-part had here.
#ifndef TGP_FOLD_X_LATE
#define TGP_FOLD_X_LATE 1
#endif
#if !TGP_FOLD_BLOCKS
#undef TGP_FOLD_X_LATE
#define TGP_FOLD_X_LATE 0
#endif

// One right-hand side / output pair.  A launch may carry up to three (column tiles >= tiles_n0 use the
// second, those >= tiles_n1 the third), which lets S^T [U | X] -- and, for the training step, S^T [U | X | S] --
// run as a single grid.
struct GemmRhs {
  const float* Bm;
  float* C;
  int Nc;
  long ldb, ldc, sB, sC, sCsplit;
};

struct GemmArgs {
  const float* A;
  long lda, sA;
  int M, Kd;               // C[M,Nc] = op(A)[M,Kd] * Bm[Kd,Nc]
  GemmRhs rhs[3];
  int tiles_m, tiles_n0, tiles_n;  // tiles_n = tiles_n0 + tiles of rhs[1] (+ tiles of rhs[2])
  int tiles_n1;            // first column tile of rhs[2]; 0 = there is no third right-hand side
  int splits;              // split of Kd across workgroups
  int k_per_split;         // multiple of BK
  const int64_t* k_ptr;    // optional [batches+1]: batch b reduces over rows k_ptr[b]..k_ptr[b+1]
  const int64_t* m_ptr;    // optional [batches+1] (row-major A only): batch b owns rows m_ptr[b]..m_ptr[b+1] of
                           // A and C (M = the longest range; sA = sC = 0) -- per-graph products on an un-padded batch
  // MODE 1 only (residual epilogue): nothing is stored; each workgroup writes sum((resid - C)^2) of its tile
  const float* resid;
  long ldr, sR;
  float* partial;          // [batches][tiles_m * tiles_n]
  int force_bm, force_bn;  // 0 = pick_tile decides
  // MODE 1 only, optional [batches]: rows / columns >= sizes[batch] of resid and op(A) Bm^T are zero (padded batch),
  // so tiles that lie entirely beyond them contribute nothing and are skipped
  const int64_t* sizes;
  // MODE 0, splits == 1: C += op(A) Bm (the second term of a two-term gradient lands in the first term's buffer: r4)
  int accumulate;
  // MODE 2 (= MODE 0 + this, r5): [batches][splits][tiles_m][rhs[0].Nc] partial COLUMN sums of the rhs[0] tiles, one
  // value per (row tile, column): the degree vector of the post-processing (utils/ops.py:311-320 with the sum over
  // dim -2) then needs 8 numbers per column instead of a pass over the K x K slabs
  float* colsum;
  int colsum_skip_diag;    // leave C[i][i] out of the sums (the post-processing clears the diagonal before it sums)
  // MODE 1, square tiles, Bm == A (the product is S S^T: symmetric) and resid square (r5): tile (I, J) with I < J also
  // takes the residual of its mirror image -- sum((resid[J-rows][I-cols] - C^T)^2) -- and tiles with I > J do nothing:
  // 36 instead of 64 products per graph at N = 1024
  int symmetric;
  // MODE 4 (MODE 3 + the second product folded in, see launch_gemm_fold): rhs[0].C is the slab set [batches][tiles_m]
  // [Nc][Nc] of S_r^T U_r (row tile r of batch b at b * sC + r * sCsplit; U itself is not stored), rhs[1] (Bm optional) is
  // X with its slab set [batches][tiles_m][Nc][rhs[1].Nc], colsum is [batches][tiles_m][Nc].  Under TGP_FOLD_BLOCKS a
  // slab is in block order (fold_slab_floats) and ldc is not used.  Under TGP_FOLD_X_LATE the kernel reads nothing of rhs[1]
  // and writes no X slabs (launch_gemm_fold still checks it: the route's conditions are the same)
};

// Row of a [rows][BK+1] LDS tile served by slot t = 8*g + r (8 lanes per slot, slot = one 128-byte row segment).
// The 8 rows one wave instruction touches are {4g..4g+3} u {4g+32..4g+35}: with the odd row stride their
// ds_write banks (33*row + 4*q + c) mod 64 are all distinct, where 8 consecutive rows would collide 2-way.
__device__ __forceinline__ int tile_row(int t) {
  const int g = t >> 3, r = t & 7;
  return 4 * (g & 7) + (r & 3) + 32 * (r >> 2) + 64 * (g >> 3);
}

#ifdef TGP_GEMM_STAMPS
// Diagnostic build only (make stamps): per-workgroup wall-clock stamps (100 MHz) at kernel entry, after the
// prologue, after the k-loop and after the epilogue, plus the hardware id (XCC / SE / CU) the workgroup ran on.
__device__ unsigned long long* g_gemm_stamps = nullptr;
__device__ int g_gemm_reverse = 0;  // experiment: hand the tiles out in reverse dispatch order
#define TGP_STAMP(slot)                                                                        \
  do {                                                                                          \
    if (g_gemm_stamps && threadIdx.x == 0)                                                      \
      g_gemm_stamps[static_cast<long>(blockIdx.x) * 16 + (slot)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#else
#define TGP_STAMP(slot) do {} while (0)
#endif

__device__ __forceinline__ float4 ld4_guarded(const float* p, bool ok) {
  return ok ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// Output tile BM x BN per workgroup of (BM/32) x WN waves; each wave owns a 32 x BN/WN strip = NT 32x32 MFMA
// tiles.  Shapes in use: 128 x 128 with 16 waves (4 x 4, NT = 1: 51 VGPRs, two workgroups per CU, A and B tiles
// loaded once per 128 x 128 of output - measured 143 TFLOP/s at C5 against 137 for the 8-wave NT = 2 form),
// 128 x 64 and 64 x 128 with 8 waves, 64 x 64 with 4 waves (when the bigger tiles would leave CUs idle).
// A_KMAJOR = false: A stored [M][Kd] (k contiguous).  true: stored [Kd][M] (m contiguous).
// ALIGNED: buffer-descriptor path, all traffic is 16-byte vectors with one predicate per vector; bases and
// leading dimensions need dword alignment only (see gemm_aligned).  Otherwise: scalar guarded path (matrices too
// large for 32-bit descriptor offsets).
// MODE 0: C = op(A) Bm (MODE 2: the same + GemmArgs.colsum; MODE 3: the same, skipping the MFMAs of sparse A chunks;
// MODE 4: MODE 3's k-loop, then Bm_r^T [C_r | X_r] over the tile's own rows instead of the store of C).  MODE 1 (link-prediction residual, utils/losses.py:644-708): Bm is stored
// [Nc][Kd] (n-major, i.e. the product is A Bm^T), and instead of storing C the epilogue accumulates
// sum((resid - C)^2) over the tile, so S S^T never exists in memory.
template <bool A_KMAJOR, bool ALIGNED, int BM, int BN, int MODE, int WN = 2>
__global__ __launch_bounds__(BM * 2 * WN) void gemm_f32_mfma_kernel(GemmArgs g) {
  constexpr int THREADS = BM * 2 * WN;              // (BM/32) x WN waves
  constexpr int NT = BN / (32 * WN);                // 32x32 MFMA tiles per wave (wave strip = 32 x BN/WN)
  constexpr int B_TILE_FLOATS = MODE == 1 ? BN * LDA_ROWMAJOR : BK * BN;
  constexpr int BN_LANES = BN / 4;                  // lanes per k-row of the B tile
  constexpr int A_TILE_FLOATS = BM * LDA_ROWMAJOR;  // >= BK*BM, used for both A layouts
  constexpr int STAGE_FLOATS = A_TILE_FLOATS + B_TILE_FLOATS;
  constexpr int A_VECS = BM * BK / 4 / THREADS;     // float4 per thread per stage (= 2)
  constexpr int B_VECS = BN * BK / 4 / THREADS;     // 2 (512 threads) or 4 (256 threads)
  constexpr int AK_LANES = BM / 4;                  // lanes per k-row of a k-major A tile
  // MODE 3: C = op(A) Bm where A is mostly zeros (an adjacency).  After each A chunk is staged the workgroup counts its
  // 4-value groups that hold a nonzero (and checks the chunk's Bm rows for Inf / NaN: 0 * Inf must stay NaN); a chunk
  // at or below TGP_SPARSE_CHUNK_GROUPS skips its MFMAs and each wave walks the nonzeros of the rows it owns (rows
  // wave + NW j) with v_fma_f32 into a register accumulator [S_ROWS][S_COLS per lane], merged into the MFMA accumulator
  // once at the end.  Skipping A_ij * S_jk is exact for A_ij = +-0 and finite S_jk, so both forms compute the same sums.
  constexpr bool FOLD = MODE == 4;
  constexpr bool SKIP = MODE == 3 || FOLD;
  static_assert(!FOLD || (BM == 128 && BN == 128 && WN == 4), "MODE 4: one 128 x 128 tile, 16 waves as 4 x 4");
  constexpr int NW = THREADS / 64;                  // waves
  constexpr int S_ROWS = BM / NW, S_COLS = BN / 64;  // MODE 3: rows a wave owns, columns a lane owns
  static_assert(!SKIP || (ALIGNED && S_ROWS % 2 == 0 && (S_COLS == 1 || S_COLS == 2) && NW <= 16 && BM * BN <= 2 * STAGE_FLOATS),
                "MODE 3: aligned tiles, two rows per ballot, one or two columns per lane");
  // k-major A tile: row stride in LDS (MODE 3 pads it so that the sparse walk's reads down a column of A spread
  // over the banks; [BK][BM + 4] is exactly the size of the row-major [BM][BK + 1] tile)
  constexpr int LDA_KM = SKIP ? BM + 4 : BM;
  static_assert(BK * LDA_KM <= A_TILE_FLOATS, "k-major A tile exceeds its LDS slot");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  TGP_STAMP(0);
#ifdef TGP_GEMM_STAMPS
  if (g_gemm_stamps && threadIdx.x == 0) {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    g_gemm_stamps[static_cast<long>(blockIdx.x) * 16 + 4] = hw;
    g_gemm_stamps[static_cast<long>(blockIdx.x) * 16 + 5] = xcc;
  }
#endif

  // logical block id, XCD-aware: tiles of one batch element share S / U through one L2
  int bid = xcd_remap(blockIdx.x, gridDim.x);
#ifdef TGP_GEMM_STAMPS
  if (g_gemm_reverse) bid = gridDim.x - 1 - bid;
#endif
  const int tn_all = bid % g.tiles_n; bid /= g.tiles_n;
  const int tm = bid % g.tiles_m; bid /= g.tiles_m;
  const int split = bid % g.splits;
  const int batch = bid / g.splits;
  const int which = tn_all >= g.tiles_n0 ? ((g.tiles_n1 && tn_all >= g.tiles_n1) ? 2 : 1) : 0;
  const int tn = which == 2 ? tn_all - g.tiles_n1 : (which ? tn_all - g.tiles_n0 : tn_all);
  const GemmRhs& R = g.rhs[which];

  const float* __restrict__ A = g.A + static_cast<long>(batch) * g.sA;
  const float* __restrict__ Bm = R.Bm + static_cast<long>(batch) * R.sB;
  float* __restrict__ C = R.C + static_cast<long>(batch) * R.sC + static_cast<long>(split) * R.sCsplit;
  const int Nc = R.Nc;
  const long lda = g.lda, ldb = R.ldb;

  const int m0 = tm * BM, n0 = tn * BN;
  if constexpr (MODE == 1) {
    if (g.sizes) {
      const int64_t nb = g.sizes[batch];
      if (m0 >= nb || n0 >= nb) {  // workgroup-uniform
        if (threadIdx.x == 0)
          g.partial[static_cast<long>(batch) * (g.tiles_m * g.tiles_n) + tm * g.tiles_n + tn_all] = 0.f;
        return;
      }
    }
    if (g.symmetric && m0 > n0) {  // the mirror tile (n0, m0) accounts for this one
      if (threadIdx.x == 0)
        g.partial[static_cast<long>(batch) * (g.tiles_m * g.tiles_n) + tm * g.tiles_n + tn_all] = 0.f;
      return;
    }
  }
  int M = g.M;
  if (g.m_ptr) {
    const long m_lo = g.m_ptr[batch];
    M = static_cast<int>(g.m_ptr[batch + 1] - m_lo);
    if (m0 >= M) return;  // workgroup-uniform: this graph is shorter than the longest one
    A += m_lo * lda;
    C += m_lo * R.ldc;
  }
  int k_lo = 0, k_hi = g.Kd;
  if (g.k_ptr) {
    k_lo = static_cast<int>(g.k_ptr[batch]);
    k_hi = static_cast<int>(g.k_ptr[batch + 1]);
  }
  // (not const: the wide sparse front-end of MODE 3 / MODE 4 moves the start of the k-loop behind the chunks it took)
  int k_begin = k_lo + split * g.k_per_split;
  const int k_end = min(k_hi, k_begin + g.k_per_split);
  int nk = k_end > k_begin ? (k_end - k_begin + BK - 1) / BK : 0;

  // register staging, two sets: tile t+2 is being loaded into one while tile t+1 is written to LDS from the other
  float4 ra[2][A_VECS], rb[2][B_VECS];

  // ALIGNED path: buffer loads.  Each operand gets a 128-bit resource descriptor (base of this batch element,
  // valid bytes) held in SGPRs, a per-lane byte offset computed ONCE (rows / columns outside the problem get an
  // offset past the end, which the hardware range check turns into zeros), and a scalar offset that advances
  // with the k-step.  The steady-state loop then issues its global loads without a single vector-ALU
  // instruction: measured per-wave time stamps showed ~0.5 us per k-step going to the address / predicate
  // arithmetic of plain global loads, which has to squeeze in between other waves' MFMAs.
  constexpr int OOB = static_cast<int>(0x80000000u);  // >= any valid size (matrices are < 2^31 bytes here)
  [[maybe_unused]] __amdgpu_buffer_rsrc_t rsrc_a, rsrc_b;
  [[maybe_unused]] int voff_a[A_VECS], voff_b[B_VECS];
  [[maybe_unused]] int kloc_a[A_VECS], kloc_b[B_VECS];  // this lane's k offset inside a stage (for the tail)
  if constexpr (ALIGNED) {
    const int a_bytes = A_KMAJOR ? (static_cast<int>(g.Kd - 1) * static_cast<int>(lda) + M) * 4
                                 : (static_cast<int>(M - 1) * static_cast<int>(lda) + g.Kd) * 4;
    const int b_bytes = MODE == 1 ? (static_cast<int>(Nc - 1) * static_cast<int>(ldb) + g.Kd) * 4
                                  : (static_cast<int>(g.Kd - 1) * static_cast<int>(ldb) + Nc) * 4;
    rsrc_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A), 0, a_bytes, 0x00020000);
    rsrc_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Bm), 0, b_bytes, 0x00020000);
#pragma unroll
    for (int i = 0; i < A_VECS; ++i) {
      if constexpr (!A_KMAJOR) {
        const int m = m0 + tile_row((tid >> 3) + i * (THREADS / 8));
        kloc_a[i] = (tid & 7) * 4;
        voff_a[i] = m < M ? (m * static_cast<int>(lda) + kloc_a[i]) * 4 : OOB;
      } else {
        const int m = m0 + (tid % AK_LANES) * 4;
        kloc_a[i] = tid / AK_LANES + i * (THREADS / AK_LANES);
        voff_a[i] = m < M ? (kloc_a[i] * static_cast<int>(lda) + m) * 4 : OOB;
      }
    }
#pragma unroll
    for (int i = 0; i < B_VECS; ++i) {
      if constexpr (MODE == 1) {
        const int n = n0 + tile_row((tid >> 3) + i * (THREADS / 8));
        kloc_b[i] = (tid & 7) * 4;
        voff_b[i] = n < Nc ? (n * static_cast<int>(ldb) + kloc_b[i]) * 4 : OOB;
      } else {
        const int n = n0 + (tid % BN_LANES) * 4;
        kloc_b[i] = tid / BN_LANES + i * (THREADS / BN_LANES);
        voff_b[i] = n < Nc ? (kloc_b[i] * static_cast<int>(ldb) + n) * 4 : OOB;
      }
    }
  }
  auto buf_ld4 = [&](__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
  };

  // one float4 of the A / B stage starting at k0 (tail = this stage is cut short by k_end)
  auto load_a = [&](int i, int k0, bool tail) -> float4 {
    if constexpr (ALIGNED) {
      const int soff = A_KMAJOR ? k0 * static_cast<int>(lda) * 4 : k0 * 4;
      if (!tail) return buf_ld4(rsrc_a, voff_a[i], soff);  // steady state: no per-lane arithmetic at all
      float4 v = buf_ld4(rsrc_a, k0 + kloc_a[i] < k_end ? voff_a[i] : OOB, soff);
      if constexpr (!A_KMAJOR) {  // k runs along the vector: a range that is not a multiple of 4 ends inside one
        const int rem = k_end - (k0 + kloc_a[i]);
        if (rem < 4) { v.w = 0.f; if (rem < 3) v.z = 0.f; if (rem < 2) v.y = 0.f; }
      }
      return v;
    } else {
      int m, k;
      if constexpr (!A_KMAJOR) {  // [BM m][32 k]: 8 lanes cover one 128-byte row segment
        m = m0 + tile_row((tid >> 3) + i * (THREADS / 8));
        k = k0 + (tid & 7) * 4;
      } else {                    // [32 k][BM m]: AK_LANES lanes cover one row
        k = k0 + tid / AK_LANES + i * (THREADS / AK_LANES);
        m = m0 + (tid % AK_LANES) * 4;
      }
      const float* p = A_KMAJOR ? A + static_cast<long>(k) * lda + m : A + static_cast<long>(m) * lda + k;
      float t[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool ok = A_KMAJOR ? (k < k_end && m + j < M) : (m < M && k + j < k_end);
        t[j] = ok ? p[j] : 0.f;
      }
      return make_float4(t[0], t[1], t[2], t[3]);
    }
  };
  auto load_b = [&](int i, int k0, bool tail) -> float4 {
    if constexpr (ALIGNED) {
      const int soff = MODE == 1 ? k0 * 4 : k0 * static_cast<int>(ldb) * 4;
      if (!tail) return buf_ld4(rsrc_b, voff_b[i], soff);
      float4 v = buf_ld4(rsrc_b, k0 + kloc_b[i] < k_end ? voff_b[i] : OOB, soff);
      if constexpr (MODE == 1) {
        const int rem = k_end - (k0 + kloc_b[i]);
        if (rem < 4) { v.w = 0.f; if (rem < 3) v.z = 0.f; if (rem < 2) v.y = 0.f; }
      }
      return v;
    } else {
      float t[4];
      if constexpr (MODE == 1) {        // [BN n][32 k]: 8 lanes cover one 128-byte row segment
        const int n = n0 + tile_row((tid >> 3) + i * (THREADS / 8)), k = k0 + (tid & 7) * 4;
        const float* p = Bm + static_cast<long>(n) * ldb + k;
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = (n < Nc && k + j < k_end) ? p[j] : 0.f;
      } else {                          // [32 k][BN n]: BN_LANES lanes cover one row
        const int k = k0 + tid / BN_LANES + i * (THREADS / BN_LANES), n = n0 + (tid % BN_LANES) * 4;
        const float* p = Bm + static_cast<long>(k) * ldb + n;
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = (k < k_end && n + j < Nc) ? p[j] : 0.f;
      }
      return make_float4(t[0], t[1], t[2], t[3]);
    }
  };
  auto store_a = [&](int i, const float4& v, float* As) {
    if constexpr (!A_KMAJOR) {
      float* d = As + tile_row((tid >> 3) + i * (THREADS / 8)) * LDA_ROWMAJOR + (tid & 7) * 4;
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    } else {
      *reinterpret_cast<float4*>(As + (tid / AK_LANES + i * (THREADS / AK_LANES)) * LDA_KM + (tid % AK_LANES) * 4) = v;
    }
  };
  auto store_b = [&](int i, const float4& v, float* Bs) {
    if constexpr (MODE == 1) {
      float* d = Bs + tile_row((tid >> 3) + i * (THREADS / 8)) * LDA_ROWMAJOR + (tid & 7) * 4;
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    } else {
      *reinterpret_cast<float4*>(Bs + (tid / BN_LANES + i * (THREADS / BN_LANES)) * BN + (tid % BN_LANES) * 4) = v;
    }
  };

  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  const int lm = lane & 31, lk = lane >> 5;
  // MODE 1: the residual tile is requested before the first k-step and consumed in the epilogue, so its
  // HBM latency hides behind the whole product (with Kd = K small the loop is only a few steps long).
  float rres[MODE == 1 ? NT : 1][16];
  [[maybe_unused]] float rmir[MODE == 1 ? NT : 1][16];  // the mirror tile's residual, transposed into the C/D layout
  [[maybe_unused]] const bool mirror = MODE == 1 && g.symmetric && m0 < n0;
  // the mirror tile read row-wise + an LDS transposition (interior, aligned tiles; one [32][33] patch per wave)
  constexpr bool MIRROR_PATCH_FITS = (THREADS / 64) * (32 * 33) <= 2 * STAGE_FLOATS;
  [[maybe_unused]] const bool mirror_rows = mirror && MIRROR_PATCH_FITS && TGP_MIRROR_ROWS && (g.ldr & 3) == 0 &&
                                            (reinterpret_cast<uintptr_t>(g.resid + static_cast<long>(batch) * g.sR) & 15) == 0 &&
                                            m0 + BM <= M && n0 + BN <= Nc && n0 + BN <= M && m0 + BM <= Nc;
  if constexpr (MODE == 1) {
    const float* __restrict__ Rm = g.resid + static_cast<long>(batch) * g.sR;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int col = n0 + wn * (BN / WN) + j * 32 + lm;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        rres[j][r] = (row < M && col < Nc) ? Rm[static_cast<long>(row) * g.ldr + col] : 0.f;
      }
    }
    if (mirror && mirror_rows) {
      // r5, late: the mirror tile is read the way it lies in memory -- 8 lanes per 128-byte row segment, a wave's 32 x 32
      // block in four passes -- and turned into the C/D layout through the wave's LDS patch in the epilogue.  Read
      // directly in that layout (below: lane = row of the residual, 16 bytes each) every lane touches another row:
      // 64 separate sectors per instruction for the half of the residual that goes this way.  (Measured at C2, same
      // box: 0.0757 -> 0.0745 ms per link-loss call -- the four passes of a lane cover its sector after all, the L2
      // absorbed the rest; the kernel is bound by its 4352 short-lived workgroups, not by these loads.)
      const float* __restrict__ base = Rm + static_cast<long>(n0 + wn * (BN / WN) + (lane >> 3)) * g.ldr + m0 + wm * 32 +
                                       4 * (lane & 7);
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 v = *reinterpret_cast<const float4*>(base + static_cast<long>(j * 32 + 8 * q) * g.ldr);
          rmir[j][4 * q] = v.x; rmir[j][4 * q + 1] = v.y; rmir[j][4 * q + 2] = v.z; rmir[j][4 * q + 3] = v.w;
        }
    } else if (mirror) {  // (workgroup-uniform)  resid[col][row]: a lane's four consecutive rows are 16 contiguous bytes
      const bool v4 = (g.ldr & 3) == 0 && (reinterpret_cast<uintptr_t>(Rm) & 15) == 0;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int col = n0 + wn * (BN / WN) + j * 32 + lm;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = m0 + wm * 32 + 8 * q + 4 * lk;
          const float* src = Rm + static_cast<long>(col) * g.ldr + row;
          if (v4 && col < Nc && row + 3 < M) {
            const float4 v = *reinterpret_cast<const float4*>(src);
            rmir[j][4 * q] = v.x; rmir[j][4 * q + 1] = v.y; rmir[j][4 * q + 2] = v.z; rmir[j][4 * q + 3] = v.w;
          } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) rmir[j][4 * q + u] = (col < Nc && row + u < M) ? src[u] : 0.f;
          }
        }
      }
    }
  }
  const int a_off = A_KMAJOR ? lk * LDA_KM + wm * 32 + lm : (wm * 32 + lm) * LDA_ROWMAJOR + lk;
  const int a_step = A_KMAJOR ? 2 * LDA_KM : 2;
  const int b_off = MODE == 1 ? (wn * (BN / WN) + lm) * LDA_ROWMAJOR + lk : lk * BN + wn * (BN / WN) + lm;
  constexpr int b_step = MODE == 1 ? 2 : 2 * BN;               // one k-pair
  constexpr int b_tile = MODE == 1 ? 32 * LDA_ROWMAJOR : 32;   // next 32 output columns
  // MFMAs of k-pairs [p0, p1) of one LDS stage.
  // LDS operand ring: the operands of k-pair p + PD are requested before the MFMAs of pair p are issued
  // (sched_group_barrier pins that order), so PD MFMA slots of latency are covered.
  constexpr int PD = TGP_OPERAND_PREFETCH;
  float a_r[PD + 1], b_r[PD + 1][NT];
  auto fetch_pair = [&](const float* As, const float* Bs, int p) {
    a_r[p % (PD + 1)] = As[a_off + p * a_step];
#pragma unroll
    for (int j = 0; j < NT; ++j) b_r[p % (PD + 1)][j] = Bs[b_off + p * b_step + b_tile * j];
  };
  auto mfma_pair = [&](int p) {
#pragma unroll
    for (int j = 0; j < NT; ++j)
      acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_r[p % (PD + 1)], b_r[p % (PD + 1)][j], acc[j], 0, 0, 0);
  };

  // MODE 3: per-wave chunk records in LDS behind the two stages, [2 parities][16 words, NW used]: the count of nonzero
  // groups in the part of the A chunk the wave staged, + 2^16 if its Bm values hold an Inf or NaN.  Written before the
  // stage's barrier, summed by every wave after it.
  [[maybe_unused]] unsigned* chunk_rec = reinterpret_cast<unsigned*>(smem + 2 * STAGE_FLOATS);
  [[maybe_unused]] float sacc[SKIP ? S_ROWS : 1][S_COLS];
  [[maybe_unused]] bool any_sparse = false;
  if constexpr (SKIP) {
#pragma unroll
    for (int j = 0; j < S_ROWS; ++j)
#pragma unroll
      for (int c = 0; c < S_COLS; ++c) sacc[j][c] = 0.f;
  }
  // (on the bits: a group holds a nonzero when some value has a bit below the sign -- +-0 are zeros, a NaN of A is a
  // nonzero and is kept; a value is not finite when its magnitude bits reach those of Inf)
  auto record_chunk = [&](auto par, const auto& va, const auto& vb) {  // (generic: no code outside MODE 3)
    unsigned n = 0;
#pragma unroll
    for (int i = 0; i < A_VECS; ++i)
      n += __popcll(__ballot(((__float_as_uint(va[i].x) | __float_as_uint(va[i].y) | __float_as_uint(va[i].z) |
                               __float_as_uint(va[i].w)) << 1) != 0u));
    unsigned mag = 0;
#pragma unroll
    for (int i = 0; i < B_VECS; ++i)
      mag = max(max(mag, max(__float_as_uint(vb[i].x) & 0x7fffffffu, __float_as_uint(vb[i].y) & 0x7fffffffu)),
                max(__float_as_uint(vb[i].z) & 0x7fffffffu, __float_as_uint(vb[i].w) & 0x7fffffffu));
    if (__ballot(mag >= 0x7f800000u)) n += 1u << 16;
    if (lane == 0) chunk_rec[par * 16 + wave] = n;
  };
  auto chunk_is_sparse = [&](auto par) -> bool {
    const uint4* r = reinterpret_cast<const uint4*>(chunk_rec + par * 16);
    unsigned n = 0;
#pragma unroll
    for (int q = 0; q < NW / 4; ++q) {
      const uint4 v = r[q];
      n += v.x + v.y + v.z + v.w;
    }
    return __builtin_amdgcn_readfirstlane(n) <= TGP_SPARSE_CHUNK_GROUPS;
  };
  // sacc[j][c] += sum over the chunk's nonzeros A[wave + NW j][k] * Bm[k][S_COLS lane + c]: two rows per ballot (lanes
  // 0-31 read row wave + NW 2i, lanes 32-63 row wave + NW (2i + 1)), then the set bits of each half, one k per
  // iteration, the A value taken from its lane (uniform k: v_readlane), the Bm row from LDS (one read per lane).
  // Each output element has one owner lane: no atomics, a fixed order.
  // The row reads of all ballots go out together, ahead of the first ballot.  Read one by one, each in front of its own
  // ballot, they were S_ROWS / 2 LDS round trips in a row in every sparse k-step: 2 to 3 us of the C2 launch at every
  // density below the threshold (profiles/adj_ring.md, which also has what did not pay: batching the Bm row reads).
  auto sparse_chunk = [&](auto As, auto Bs) {
    float va[S_ROWS / 2];
#pragma unroll
    for (int i = 0; i < S_ROWS / 2; ++i) {
      const int row = wave + NW * (2 * i + (lane >> 5)), k = lane & 31;
      va[i] = A_KMAJOR ? As[k * LDA_KM + row] : As[row * LDA_ROWMAJOR + k];
    }
#pragma unroll
    for (int i = 0; i < S_ROWS / 2; ++i) asm volatile("" : "+v"(va[i]));  // (keeps the reads from sinking to their ballots)
#pragma unroll
    for (int i = 0; i < S_ROWS / 2; ++i) {
      const float v = va[i];
      const unsigned long long nz = __ballot(v != 0.f);
      const int vbits = __float_as_int(v);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        for (unsigned m = static_cast<unsigned>(nz >> (32 * h)); m; m &= m - 1) {
          const int kk = __builtin_ctz(m);
          const float a = __int_as_float(__builtin_amdgcn_readlane(vbits, kk + 32 * h));
          if constexpr (S_COLS == 2) {
            const float2 b = *reinterpret_cast<const float2*>(Bs + kk * BN + 2 * lane);
            sacc[2 * i + h][0] = fmaf(a, b.x, sacc[2 * i + h][0]);
            sacc[2 * i + h][S_COLS - 1] = fmaf(a, b.y, sacc[2 * i + h][S_COLS - 1]);
          } else {
            sacc[2 * i + h][0] = fmaf(a, Bs[kk * BN + lane], sacc[2 * i + h][0]);
          }
        }
      }
    }
  };

  // Stage schedule.  Per-wave time stamps (tools/gemm_stamps.py) showed that a wave loses most of a k-step not
  // in the MFMAs but queueing behind the other 15 waves of the CU whenever all of them issue their global loads
  // or their LDS stores at the same point of the step (the texture-address path takes 16 clk per 1 KB load and a
  // wave cannot issue its next MFMA while it is stuck in that queue).  So the memory work of a stage is dealt
  // out ONE instruction at a time between MFMA pairs:
  //   pair 1: load A0(t+2) | 2: store A0(t+1) | 3: load A1 | 4: store A1 | 5: load B0 | 6: store B0 | ...
  // Tile t+2 is loaded into register set t&1 during stage t, written to LDS from there during stage t+1 (the
  // other LDS buffer than the one being read) and multiplied in stage t+2, so a load has a whole stage to land.
  float* L0 = smem;
  float* L1 = smem + STAGE_FLOATS;
  auto kof = [&](int t) { return k_begin + t * BK; };
  // STEADY (r5, late): the stage as the middle of the k-loop runs it -- tile t + 1 is stored, tile t + 2 is loaded, and
  // that tile is a full one -- with all three facts known at compile time.  The general form decides them per stage,
  // and the waits for the staged registers then sit inside conditional blocks: on the path that skips a block the
  // compiler must assume the loads into a register set are still pending when the next stage overwrites it, and it
  // put an `s_waitcnt vmcnt(0)` in front of the B tile's load -- right behind the two A loads of the same stage, so
  // every wave sat out a full memory round trip per k-step -- plus ~25 branches per step.
  // SK (MODE 3): the stage decides between the MFMAs and the sparse walk, and records the chunk it stores
  [[maybe_unused]] int dense_run = 0;       // MODE 3: dense k-steps in a row (workgroup-uniform)
  [[maybe_unused]] bool dense_rest = false; // MODE 3: TGP_DENSE_RUN reached: plain stages from here on
  [[maybe_unused]] bool any_dense = false;  // MODE 4: some stage ran its MFMAs, so acc may hold something (workgroup-uniform)
  auto stage = [&](auto par_c, auto steady_c, auto sk_c, int t) {
    constexpr int PAR = decltype(par_c)::value;
    constexpr bool STEADY = decltype(steady_c)::value;
    constexpr bool SK = decltype(sk_c)::value;
    const float* As = PAR ? L1 : L0;
    const float* Bs = As + A_TILE_FLOATS;
    float* An = PAR ? L0 : L1;
    float* Bn = An + A_TILE_FLOATS;
    const bool do_store = STEADY || t + 1 < nk, do_load = STEADY || t + 2 < nk;
    const int k2 = kof(t + 2);
    const bool tail = !STEADY && k2 + BK > k_end;
#ifdef TGP_GEMM_STAMPS
    // phase clock of one k-step in the middle of the loop (wave 0 of every workgroup): slots 8.. hold the time at
    // step start, before / after the LDS stores, before / after the global loads, before / after the barrier
    const bool probe = g_gemm_stamps && t == (nk / 2) && threadIdx.x == 0;
#define TGP_PHASE(i) do { if (probe) g_gemm_stamps[static_cast<long>(blockIdx.x) * 16 + 8 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define TGP_PHASE(i) do {} while (0)
#endif
    TGP_PHASE(0);
    bool sparse = false;  // (workgroup-uniform)
    if constexpr (SK) {
      // the dense form's first operand reads go out together with the reads of the chunk records, so the stage waits
      // for one LDS round trip before its first MFMA, as without the records (the empty asm keeps the compiler from
      // sinking the operand reads behind the branch)
#pragma unroll
      for (int p = 0; p < PD; ++p) fetch_pair(As, Bs, p);
      sparse = chunk_is_sparse(PAR);
#pragma unroll
      for (int p = 0; p < PD; ++p) {
        asm volatile("" ::"v"(a_r[p % (PD + 1)]));
#pragma unroll
        for (int j = 0; j < NT; ++j) asm volatile("" ::"v"(b_r[p % (PD + 1)][j]));
      }
      any_sparse = any_sparse || sparse;
      dense_run = sparse ? 0 : dense_run + 1;
      dense_rest = dense_run >= TGP_DENSE_RUN;
      if constexpr (FOLD) any_dense = any_dense || !sparse || dense_rest;  // (plain stages run only behind dense_rest)
      if (sparse) {
      // the stage's memory work in one block: tile t+2 is requested first, tile t+1 goes to LDS after the walk
#pragma unroll
      for (int v = 0; v < A_VECS + B_VECS; ++v)
        if (do_load) {
          if (v < A_VECS) ra[PAR][v] = load_a(v, k2, tail);
          else rb[PAR][v - A_VECS] = load_b(v - A_VECS, k2, tail);
        }
      sparse_chunk(As, Bs);
#pragma unroll
      for (int v = 0; v < A_VECS + B_VECS; ++v)
        if (do_store) {
          if (v < A_VECS) store_a(v, ra[1 - PAR][v], An);
          else store_b(v - A_VECS, rb[1 - PAR][v - A_VECS], Bn);
        }
      if (do_store) record_chunk(1 - PAR, ra[1 - PAR], rb[1 - PAR]);
      // (the accumulator passes this branch in the registers the MFMAs use: without this the compiler gave the loop
      // two homes for it and copied it back after every dense stage, behind the last MFMA's full latency)
#pragma unroll
      for (int j = 0; j < NT; ++j) asm volatile("" : "+v"(acc[j]));
      }
    }
    // (the sparse block above exists only in deciding stages: every other stage is the MODE 0 stage as it was)
    if (!SK || !sparse) {
    if constexpr (!SK) {
#pragma unroll
      for (int p = 0; p < PD; ++p) fetch_pair(As, Bs, p);
    }
#pragma unroll
    for (int p = 0; p < BK / 2; ++p) {
      if (p + PD < BK / 2) fetch_pair(As, Bs, p + PD);
      mfma_pair(p);
      if (p + PD < BK / 2) __builtin_amdgcn_sched_group_barrier(0x100, 1 + NT, 0);  // ds_reads of pair p+PD
      __builtin_amdgcn_sched_group_barrier(0x008, NT, 0);                            // NT x MFMA
      // memory work of the stage: loads of tile t+2 behind pair LOAD_AT, LDS stores of tile t+1 behind STORE_AT
      // (SPREAD: one vector per pair starting there, instead of all at once)
      constexpr int LOAD_AT = TGP_LOAD_AT, STORE_AT = TGP_STORE_AT, SPREAD = TGP_SPREAD;
      if (p == STORE_AT) TGP_PHASE(1);
      if (p == LOAD_AT) TGP_PHASE(3);
#pragma unroll
      for (int v = 0; v < A_VECS + B_VECS; ++v) {
        if (p == LOAD_AT + (SPREAD ? v : 0) && do_load) {
          if (v < A_VECS) ra[PAR][v] = load_a(v, k2, tail);
          else rb[PAR][v - A_VECS] = load_b(v - A_VECS, k2, tail);
        }
        if (p == STORE_AT + (SPREAD ? v : 0) && do_store) {
          if (v < A_VECS) store_a(v, ra[1 - PAR][v], An);
          else store_b(v - A_VECS, rb[1 - PAR][v - A_VECS], Bn);
        }
      }
      // MODE 3: tile t+1's record right behind its last LDS store, between MFMAs (at the end of the stage it held up
      // every wave's arrival at the barrier)
      if constexpr (SK) {
        if (p == STORE_AT + (SPREAD ? A_VECS + B_VECS : 1) && do_store) record_chunk(1 - PAR, ra[1 - PAR], rb[1 - PAR]);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (p == STORE_AT) TGP_PHASE(2);
      if (p == LOAD_AT) TGP_PHASE(4);
    }
    }
    TGP_PHASE(5);
    __syncthreads();
    TGP_PHASE(6);
  };
  // ---- MODE 3 / MODE 4, row-major A, the 16-wave 128 x 128 tile: the wide sparse front-end ---------------------------
  // While the next WIDE_K = 128 columns of the k-range form a sparse chunk of A (128 x 128, as 4096 groups of 4 values:
  // at most TGP_SPARSE_WIDE_GROUPS hold a nonzero, and the chunk's Bm rows are finite) the workgroup takes it here, in
  // one stage instead of four.  A is never a shared LDS tile here: it is an MFMA operand only in a dense chunk.  Wave w
  // loads the rows it owns in the walk (w + NW j) itself, two rows per 16-byte load (lanes 0-31 one row, lanes 32-63 the
  // other, 512 contiguous bytes each), and turns each pair through 1 KB of LDS of its own -- no barrier, a wave's LDS
  // operations complete in order -- into a lane per column, 64 columns per register: what the narrow walk reads from
  // the A tile.  The walk is then the narrow one, out of registers: ballot, v_readlane, one ds_read_b64 of the Bm row
  // and one taken branch per nonzero.  (Walked as loaded, four columns per lane, it needs a second level -- which of
  // the lane's four values -- and those scalar branches cost more than the front-end saves; loaded a lane per column,
  // sixteen dword loads per chunk, the loads do: profiles/adj_front.md.)  The Bm rows of the chunk lie in LDS as
  // [128][BN], the layout the narrow walk reads, in two buffers.  Chunk t + 1 (A as loaded, Bm in staging registers) is
  // requested before chunk t is walked, and turned, stored and recorded behind the walk: one barrier per chunk.  Per
  // output element the nonzeros are added in ascending k, as the narrow walk adds them, so the sums are bitwise those
  // of the 32-column stages wherever both walk.
  // The first chunk that is not sparse -- too many groups, an Inf / NaN in its Bm rows -- or fewer than 128 columns
  // left end the front-end for this workgroup: the register-staged loop below then starts at that k (its prologue,
  // records, TGP_DENSE_RUN and tail stages as they are) and runs zero stages when nothing is left.
  constexpr bool FRONT = SKIP && !A_KMAJOR && BM == 128 && BN == 128 && WN == 4;
  if constexpr (FRONT) {
    constexpr int WIDE_K = 128;
    constexpr int W_FLOATS = WIDE_K * BN;               // one Bm chunk in LDS; two buffers, the records behind them
    constexpr int W_VECS = WIDE_K * BN / 4 / THREADS;   // float4 of Bm per thread and chunk (= 4)
    constexpr int W_PAIRS = S_ROWS / 2;                 // row pairs of A per wave and chunk, one 16-byte load each (= 4)
    constexpr int W_REGS = S_ROWS * (WIDE_K / 64);      // A values per lane and chunk: row j, columns 64 p + lane (= 16)
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    unsigned* wide_rec = reinterpret_cast<unsigned*>(smem + 2 * W_FLOATS);  // [2 parities][16 words], as chunk_rec
    unsigned* wide_turn = wide_rec + 2 * 16 + wave * 256;                   // the wave's own 1 KB: one row pair
    u32x4 wr[W_PAIRS];   // the next chunk's rows as loaded
    unsigned wa[W_REGS];  // this chunk's rows, a lane per column
    float4 ws[W_VECS];
    int voff_w[W_PAIRS];
#pragma unroll
    for (int i = 0; i < W_PAIRS; ++i) {
      const int m = m0 + wave + NW * (2 * i + (lane >> 5));
      voff_w[i] = m < M ? (m * static_cast<int>(lda) + 4 * (lane & 31)) * 4 : OOB;  // (rows beyond M: zeros)
    }
    auto wide_load = [&](int k0) {  // the chunk at k0: A rows as loaded, the Bm rows into the staging registers
#pragma unroll
      for (int i = 0; i < W_PAIRS; ++i) wr[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_a, voff_w[i], k0 * 4, 0);
#pragma unroll
      for (int i = 0; i < W_VECS; ++i)
        ws[i] = buf_ld4(rsrc_b, voff_b[0], (k0 + i * (THREADS / BN_LANES)) * static_cast<int>(ldb) * 4);
    };
    // the staged Bm rows to LDS buffer PAR, the A rows turned into the registers the walk reads, and the wave's record
    // of that chunk: the groups of its own A registers that hold a nonzero (the bit test of record_chunk), + 2^16 if
    // the Bm values it staged hold an Inf or NaN
    auto wide_publish = [&](auto par_c) {
      constexpr int PAR = decltype(par_c)::value;
#pragma unroll
      for (int i = 0; i < W_VECS; ++i) store_b(i, ws[i], smem + PAR * W_FLOATS);
      unsigned n = 0;
#pragma unroll
      for (int i = 0; i < W_PAIRS; ++i) {
        n += __popcll(__ballot(((wr[i].x | wr[i].y | wr[i].z | wr[i].w) << 1) != 0u));
        // (the wave barriers only keep the compiler from moving the accesses across each other)
        *reinterpret_cast<u32x4*>(wide_turn + 4 * lane) = wr[i];  // row 2i: words 0 .. 127, row 2i + 1: 128 .. 255
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < 4; ++q) wa[4 * i + q] = wide_turn[64 * q + lane];
        __builtin_amdgcn_wave_barrier();
      }
      unsigned mag = 0;
#pragma unroll
      for (int i = 0; i < W_VECS; ++i)
        mag = max(max(mag, max(__float_as_uint(ws[i].x) & 0x7fffffffu, __float_as_uint(ws[i].y) & 0x7fffffffu)),
                  max(__float_as_uint(ws[i].z) & 0x7fffffffu, __float_as_uint(ws[i].w) & 0x7fffffffu));
      if (__ballot(mag >= 0x7f800000u)) n += 1u << 16;
      if (lane == 0) wide_rec[PAR * 16 + wave] = n;
    };
    auto wide_is_sparse = [&](auto par_c) -> bool {
      const uint4* r = reinterpret_cast<const uint4*>(wide_rec + decltype(par_c)::value * 16);
      unsigned n = 0;
#pragma unroll
      for (int q = 0; q < NW / 4; ++q) {
        const uint4 v = r[q];
        n += v.x + v.y + v.z + v.w;
      }
      return __builtin_amdgcn_readfirstlane(n) <= TGP_SPARSE_WIDE_GROUPS;
    };
    // sacc[j][c] += sum over the chunk's nonzeros A[wave + NW j][k] * Bm[k][2 lane + c], k ascending within each row:
    // per register one ballot (a != 0.f: -0 is a zero, a NaN is not), then its set bits as the narrow walk takes them.
    // One Bm row read at a time: requested one nonzero ahead of the adds it measured slower (profiles/adj_front.md).
    auto wide_walk = [&](auto par_c) {
      const float* Bs = smem + decltype(par_c)::value * W_FLOATS;
#pragma unroll
      for (int r = 0; r < W_REGS; ++r) {
        constexpr int PARTS = WIDE_K / 64;
        const int j = r / PARTS;
        const float* Bp = Bs + 64 * (r % PARTS) * BN + 2 * lane;
        const int vbits = static_cast<int>(wa[r]);
        for (unsigned long long m = __ballot(__int_as_float(vbits) != 0.f); m; m &= m - 1) {
          const int kk = __builtin_ctzll(m);
          const float a = __int_as_float(__builtin_amdgcn_readlane(vbits, kk));
          const float2 b = *reinterpret_cast<const float2*>(Bp + kk * BN);
          sacc[j][0] = fmaf(a, b.x, sacc[j][0]);
          sacc[j][1] = fmaf(a, b.y, sacc[j][1]);
        }
      }
    };
    int kw = k_begin;
    if (k_end - kw >= WIDE_K) {
      using P0 = std::integral_constant<int, 0>;
      using P1 = std::integral_constant<int, 1>;
      wide_load(kw);
      wide_publish(P0{});
      __syncthreads();
      // one chunk: decide, request the next, walk, publish the next.  Returns whether another chunk was published.
      auto wide_stage = [&](auto par_c) -> bool {
        constexpr int PAR = decltype(par_c)::value;
        // (not sparse: nothing of the wide buffers is read any more -- every walk lies behind a barrier -- and the loop
        // below stores into them only behind this point)
        if (!wide_is_sparse(par_c)) return false;
        const bool more = k_end - kw >= 2 * WIDE_K;  // (workgroup-uniform)
        if (more) wide_load(kw + WIDE_K);
        wide_walk(par_c);
        if (more) wide_publish(std::integral_constant<int, 1 - PAR>{});
        any_sparse = true;
        kw += WIDE_K;
        __syncthreads();  // chunk t + 1 is published; chunk t's buffer and record are free (and, at the end, the LDS)
        return more;
      };
      while (wide_stage(P0{}) && wide_stage(P1{})) {
      }
      k_begin = kw;
      nk = k_end > k_begin ? (k_end - k_begin + BK - 1) / BK : 0;
    }
  }
  if (nk > 0) {
#pragma unroll
    for (int i = 0; i < A_VECS; ++i) ra[0][i] = load_a(i, kof(0), kof(0) + BK > k_end);
#pragma unroll
    for (int i = 0; i < B_VECS; ++i) rb[0][i] = load_b(i, kof(0), kof(0) + BK > k_end);
  }
  if (nk > 1) {
#pragma unroll
    for (int i = 0; i < A_VECS; ++i) ra[1][i] = load_a(i, kof(1), kof(1) + BK > k_end);
#pragma unroll
    for (int i = 0; i < B_VECS; ++i) rb[1][i] = load_b(i, kof(1), kof(1) + BK > k_end);
  }
  if (nk > 0) {
#pragma unroll
    for (int i = 0; i < A_VECS; ++i) store_a(i, ra[0][i], L0);
#pragma unroll
    for (int i = 0; i < B_VECS; ++i) store_b(i, rb[0][i], L0 + A_TILE_FLOATS);
    if constexpr (SKIP) record_chunk(0, ra[0], rb[0]);
  }
  __syncthreads();
  TGP_STAMP(1);
  // MODE 4: the tail's operands -- rows m0 .. m0 + 127 of Bm (S_r) and of X (X_r) -- pass through registers: per thread
  // four vectors of S_r (its B-tile vector, 32 rows apart) and two of X_r (16 lanes per row of <= 64 values, 64 rows
  // apart).  Rows beyond the matrices and columns beyond Nc / F come back as zeros from the descriptors' range check.
  [[maybe_unused]] float4 fs[4], fx[2];
  auto fold_load = [&]() {
    if constexpr (FOLD) {
      const GemmRhs& RX = g.rhs[1];
      const int x_bytes = RX.Bm ? static_cast<int>(g.Kd) * static_cast<int>(RX.ldb) * 4 : 0;
      const __amdgpu_buffer_rsrc_t rsrc_x = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<float*>(RX.Bm ? RX.Bm + static_cast<long>(batch) * RX.sB : Bm), 0, x_bytes, 0x00020000);
      const int ldx4 = RX.Bm ? static_cast<int>(RX.ldb) * 4 : 0;
      const int voff_x = (RX.Bm && (tid & 15) * 4 < RX.Nc) ? (tid >> 4) * ldx4 + (tid & 15) * 16 : OOB;
#pragma unroll
      for (int i = 0; i < 4; ++i) fs[i] = buf_ld4(rsrc_b, voff_b[0], (m0 + 32 * i) * static_cast<int>(ldb) * 4);
      if constexpr (!TGP_FOLD_X_LATE) {  // (X_LATE: the second launch reads X itself)
#pragma unroll
      for (int i = 0; i < 2; ++i) fx[i] = buf_ld4(rsrc_x, voff_x, (m0 + 64 * i) * ldx4);
      }
    }
  };
  int t = 0;
  using std::integral_constant;
  using FALSE_C = integral_constant<bool, false>;
  using TRUE_C = integral_constant<bool, true>;
  if constexpr (!SKIP) {
  if constexpr (ALIGNED && TGP_STEADY_LOOP) {
    // pairs of stages whose loaded tiles (t + 2 and t + 3) exist and are full
    for (; t + 3 < nk && kof(t + 3) + BK <= k_end; t += 2) {
#ifdef TGP_GEMM_STAMPS
      if (t == (nk / 2 & ~1)) TGP_STAMP(6);
      if (t == ((3 * nk) / 4 & ~1)) TGP_STAMP(7);
#endif
      stage(integral_constant<int, 0>{}, TRUE_C{}, FALSE_C{}, t);
      stage(integral_constant<int, 1>{}, TRUE_C{}, FALSE_C{}, t + 1);
    }
  }
  for (; t < nk; t += 2) {
#ifdef TGP_GEMM_STAMPS
    if (t == (nk / 2 & ~1)) TGP_STAMP(6);
    if (t == ((3 * nk) / 4 & ~1)) TGP_STAMP(7);
#endif
    stage(integral_constant<int, 0>{}, FALSE_C{}, FALSE_C{}, t);
    if (t + 1 < nk) stage(integral_constant<int, 1>{}, FALSE_C{}, FALSE_C{}, t + 1);
  }
  } else {
    // MODE 3: deciding stages until TGP_DENSE_RUN dense k-steps in a row, then the MODE 0 loop (pairs of full stages);
    // the tail stages decide as long as the workgroup has not switched
    for (; t + 3 < nk && kof(t + 3) + BK <= k_end && !dense_rest; t += 2) {
      stage(integral_constant<int, 0>{}, TRUE_C{}, TRUE_C{}, t);
      stage(integral_constant<int, 1>{}, TRUE_C{}, TRUE_C{}, t + 1);
    }
    for (; t + 3 < nk && kof(t + 3) + BK <= k_end; t += 2) {
      stage(integral_constant<int, 0>{}, TRUE_C{}, FALSE_C{}, t);
      stage(integral_constant<int, 1>{}, TRUE_C{}, FALSE_C{}, t + 1);
    }
    auto tail_stage = [&](auto par_c, int t) {
      if (dense_rest) stage(par_c, FALSE_C{}, FALSE_C{}, t);
      else stage(par_c, FALSE_C{}, TRUE_C{}, t);
    };
    for (; t < nk; t += 2) {
      tail_stage(integral_constant<int, 0>{}, t);
      if (t + 1 < nk) tail_stage(integral_constant<int, 1>{}, t + 1);
    }
  }
  TGP_STAMP(2);
  fold_load();  // (MODE 4: the tail's operands are requested as the k-loop ends)
  if constexpr (SKIP && !FOLD) {  // (MODE 4 adds the walk's sums to U where the tail keeps it: in LDS, below)
    if (any_sparse) {  // (workgroup-uniform; the k-loop's last barrier has passed: the LDS is free)
#pragma unroll
      for (int j = 0; j < S_ROWS; ++j)
#pragma unroll
        for (int c = 0; c < S_COLS; ++c) smem[(wave + NW * j) * BN + S_COLS * lane + c] = sacc[j][c];
      __syncthreads();
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          acc[j][r] = __fadd_rn(acc[j][r],
                                smem[(wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk) * BN + wn * (BN / WN) + j * 32 + lm]);
      __syncthreads();  // (the epilogue's LDS patches may reuse these words)
    }
  }

  // ---- MODE 4 tail: P = S_r^T [U_r | X_r] over the tile's 128 rows, U_r taken from the accumulators -------------------
  // The 128 x 192 result is 8 x 12 blocks of 16 x 16 (v_mfma_f32_16x16x4_f32: the same exact fp32 chains as the 32 x 32
  // form), six per wave -- wave (wm, wn) owns rows 32 wm .. + 31 and columns 48 wn .. + 47 of [S^T U | S^T X] -- each over
  // the full k range, so every element has one owner and one summation order (k ascending) and nothing is added across
  // waves.  Both operands lie in LDS whole, S_r [128][128] and [U_r | X_r] [128][192]: exactly the 160 KB, so the rows
  // are not padded but swizzled -- column c of row k sits at c ^ 16 (k & 3), which keeps 16-byte vectors whole and puts
  // the four k rows of an operand read on different banks.  The result then goes to LDS as one tile [128][196] and
  // leaves in 16-byte stores; its column sums are taken from there in row order (16-row partials by eight thread
  // groups, added in order).  That is the one-phase form (TGP_FOLD_SPLIT = 0); the shipped one gives a wave other
  // columns of the same rows and lets S^T U leave while S^T X is multiplied -- same blocks, same orders: see there.
  if constexpr (FOLD) {
    constexpr int P_LD = 196;
    float* Sf = smem;
    float* UXf = smem + BM * BN;
    const GemmRhs& RX = g.rhs[1];
    const int F = RX.Bm ? RX.Nc : 0;
    const int l15 = lane & 15, lq = lane >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = (tid >> 5) + 32 * i;
      *reinterpret_cast<float4*>(Sf + k * BN + (((tid & 31) * 4) ^ ((k & 3) << 4))) = fs[i];
    }
    if constexpr (!TGP_FOLD_X_LATE) {  // (X_LATE: columns 128 .. 191 of the [U_r | X_r] rows stay free for the whole tail)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int k = (tid >> 4) + 64 * i;
      *reinterpret_cast<float4*>(UXf + k * 192 + ((BN + (tid & 15) * 4) ^ ((k & 3) << 4))) = fx[i];
    }
    }
    // (workgroup-uniform) no MFMA ran in the k-loop: acc is +0 everywhere, so U = 0 + sacc goes to LDS directly, each
    // element from the lane that owns it in the walk -- the same add as below (a -0 sum becomes +0 there too), without
    // the accumulators' trip through LDS and its barrier.  Rows beyond M: their A rows are zeros from the descriptor
    // and only finite S rows are walked, so their sums are +0.
    const bool direct = TGP_FOLD_SKIP_ACC && !any_dense;
    if (direct) {
#pragma unroll
      for (int j = 0; j < S_ROWS; ++j) {
        const int row = wave + NW * j;
        *reinterpret_cast<float2*>(UXf + row * 192 + ((2 * lane) ^ ((row & 3) << 4))) =
            make_float2(__fadd_rn(0.f, sacc[j][0]), __fadd_rn(0.f, sacc[j][S_COLS - 1]));
      }
    } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) {  // rows beyond M are zeros (0 * Inf of the k-loop is not)
      const int rl = (r & 3) + 8 * (r >> 2) + 4 * lk;
      UXf[(wm * 32 + rl) * 192 + ((wn * 32 + lm) ^ ((r & 3) << 4))] = m0 + wm * 32 + rl < M ? acc[0][r] : 0.f;
    }
    }
    f32x4 d[2][3];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) d[i][j][r] = 0.f;
    __syncthreads();
    if (any_sparse && !direct) {  // (workgroup-uniform) U += the walk's sums, each element by the lane that owns it: acc + sacc as in MODE 3
#pragma unroll
      for (int j = 0; j < S_ROWS; ++j) {
        const int row = wave + NW * j;
        float2* u = reinterpret_cast<float2*>(UXf + row * 192 + ((2 * lane) ^ ((row & 3) << 4)));
        float2 v = *u;
        v.x = __fadd_rn(v.x, sacc[j][0]);
        v.y = __fadd_rn(v.y, sacc[j][S_COLS - 1]);
        *u = v;
      }
      __syncthreads();
    }
    TGP_STAMP(8);  // (stamps build: slots 8 .. 11 are the tail's phases)
    if constexpr (TGP_FOLD_SPLIT) {
      // Two MFMA phases, the first one's result leaving under the second.  Wave (wm, wn) owns rows 32 wm .. + 31 of both
      // parts, columns 32 wn .. + 31 of S^T U (four blocks, d[i][0 .. 1]) and 16 wn .. + 15 of S^T X (two, d[i][2]): six
      // blocks and 192 MFMAs as in the one-phase form below, every block over the full k range in ascending k.
      //   U-part, 32 k-groups of four MFMAs; the 16-row column-sum partials are taken from its accumulators;
      //   X-part, 32 k-groups of two, with one memory instruction behind each pair:
      //     groups 0 .. 3, then the barrier behind which no wave reads U_r any more;
      //     groups 4 .. 11 with the sixteen ds_write_b32 that park S^T U in U_r's LDS words, then a barrier;
      //     groups 12 .. 19 with the 16-byte reads of the parked tile and their slab stores, four of each per thread;
      //     groups 20 .. 31.
      // S^T X then leaves straight from the accumulators (16 lanes per 64-byte row segment), and behind a last barrier
      // -- S_r is dead -- the partials go to LDS and are added in order.
      // (4 / 8 against 1 / 16, 2 / 8, 4 / 4 and 8 / 8: profiles/c2_tail.md)
      // That X-part is the row-major form (TGP_FOLD_BLOCKS = 0); the shipped one stores the blocks as they are: see there.
      constexpr int G_FREE = 4, G_PARK = 8, PARK_PER = 16 / G_PARK;
      int a_at[2], u_at[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) a_at[i] = lq * BN + ((wm * 32 + 16 * i + l15) ^ (lq << 4));
#pragma unroll
      for (int j = 0; j < 2; ++j) u_at[j] = lq * 192 + ((wn * 32 + 16 * j + l15) ^ (lq << 4));
      const int x_at = lq * 192 + ((BN + wn * 16 + l15) ^ (lq << 4));
      float a[2][2], b[2][2];
      auto fetch_u = [&](int s) {
#pragma unroll
        for (int i = 0; i < 2; ++i) a[s & 1][i] = Sf[4 * s * BN + a_at[i]];
#pragma unroll
        for (int j = 0; j < 2; ++j) b[s & 1][j] = UXf[4 * s * 192 + u_at[j]];
      };
      auto fetch_x = [&](int s) {  // (b[.][0] holds the X operand)
#pragma unroll
        for (int i = 0; i < 2; ++i) a[s & 1][i] = Sf[4 * s * BN + a_at[i]];
        b[s & 1][0] = UXf[4 * s * 192 + x_at];
      };
      fetch_u(0);
#pragma unroll
      for (int s = 0; s < 32; ++s) {
        if (s + 1 < 32) fetch_u(s + 1);
        else if constexpr (!TGP_FOLD_X_LATE) fetch_x(0);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 2; ++i)
            d[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s & 1][i], b[s & 1][j], d[i][j], 0, 0, 0);
        if (s + 1 < 32) __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);  // ds_reads of the next group
        else if constexpr (!TGP_FOLD_X_LATE) __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);                   // 4 x MFMA
        __builtin_amdgcn_sched_barrier(0);
      }
      TGP_STAMP(9);
      if constexpr (TGP_FOLD_X_LATE) {
        // No X-part: the four S^T U blocks leave at once, as the same write-through block stores (fold_slab_floats: block
        // (2 wm + i, 2 wn + j), blocks wholly beyond Nc fail the descriptor's range check), with the partials' adds
        // behind them.
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        constexpr int WT = TGP_FOLD_SLAB_WT ? 16 : 0;  // (aux bit 4: sc1)
        const int kb = (Nc + 15) >> 4;
        float* Ca = R.C + static_cast<long>(batch) * R.sC + static_cast<long>(tm) * R.sCsplit;
        const __amdgpu_buffer_rsrc_t rsrc_c = __builtin_amdgcn_make_buffer_rsrc(Ca, 0, kb * kb * 1024, 0x00020000);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int br = 2 * wm + i, bc = 2 * wn + j;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, d[i][j]), rsrc_c,
                                                   (br < kb && bc < kb) ? (br * kb + bc) * 1024 + lane * 16 : OOB, 0, WT);
          }
        TGP_STAMP(10);
      }
      // column sums of S^T U, the 16-row partial of block row 2 wm + i: a lane holds rows 4 lq + r of its column, so the
      // lanes lq = 0 add their four rows to 0 and hand the sum to lq = 1, and so on -- the sixteen adds in row order;
      // the lanes lq = 3 end up with the partial (rows >= Nc and, under colsum_skip_diag, the diagonal count as 0)
      float cpart[2][2];
      if (g.colsum) {  // (workgroup-uniform)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int col = wn * 32 + 16 * j + l15;
            float cs = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              if (q) cs = __shfl_up(cs, 16, 64);
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int row = wm * 32 + 16 * i + 4 * lq + r;
                cs = __fadd_rn(cs, (row >= Nc || (g.colsum_skip_diag && row == col)) ? 0.f : d[i][j][r]);
              }
            }
            cpart[i][j] = cs;
          }
      }
      if constexpr (TGP_FOLD_X_LATE) {
        // The eight 16-row partials per column go to the words X_r had -- columns 128 .. 191 of the operand rows, which
        // nothing reads or writes in this tail: partial q of column c at row 2 q + c / 64 -- so they do not wait for S_r
        // to die: one barrier, then the same ordered add as behind the X-part.
        TGP_STAMP(11);
        if (g.colsum) {  // (workgroup-uniform)
          auto part_at = [&](int q, int c) { return UXf + (2 * q + (c >> 6)) * 192 + BN + (c & 63); };
          if (lq == 3) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
              for (int j = 0; j < 2; ++j) *part_at(2 * wm + i, wn * 32 + 16 * j + l15) = cpart[i][j];
          }
          __syncthreads();
          if (tid < Nc) {
            float tot = 0.f;
#pragma unroll
            for (int qq = 0; qq < 8; ++qq) tot = __fadd_rn(tot, *part_at(qq, tid));
            g.colsum[(static_cast<long>(batch) * g.tiles_m + tm) * Nc + tid] = tot;
          }
        }
        TGP_STAMP(3);
        return;
      }
      if constexpr (TGP_FOLD_BLOCKS) {
        // Block-order slabs (fold_slab_floats): d[i][j] is block (2 wm + i, 2 wn + j) of S^T U and d[i][2] block
        // (2 wm + i, wn) of S^T X exactly as the wave holds them, so each leaves as one 16-byte store per lane, 1 KB per
        // wave.  Blocks wholly beyond Nc / F are not stored (their offset fails the descriptor's range check: no branch);
        // the out-of-range words of a partial block may hold anything and post_rows_kernel<true> does not read them.
        // The X-part runs its 32 k-groups with no barrier; the four S^T U stores go out behind its first four pairs.
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        constexpr int WT = TGP_FOLD_SLAB_WT ? 16 : 0;  // (aux bit 4: sc1)
        const int kb = (Nc + 15) >> 4, fb = (F + 15) >> 4;
        float* Ca = R.C + static_cast<long>(batch) * R.sC + static_cast<long>(tm) * R.sCsplit;
        const __amdgpu_buffer_rsrc_t rsrc_c = __builtin_amdgcn_make_buffer_rsrc(Ca, 0, kb * kb * 1024, 0x00020000);
        int voff_c[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int br = 2 * wm + i, bc = 2 * wn + j;
            voff_c[i][j] = (br < kb && bc < kb) ? (br * kb + bc) * 1024 + lane * 16 : OOB;
          }
#pragma unroll
        for (int s = 0; s < 32; ++s) {
          if (s == 12) TGP_STAMP(10);
          if (s + 1 < 32) fetch_x(s + 1);
#pragma unroll
          for (int i = 0; i < 2; ++i) d[i][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s & 1][i], b[s & 1][0], d[i][2], 0, 0, 0);
          if (s + 1 < 32) __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);  // ds_reads of the next group
          __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);                   // 2 x MFMA
          if (s < 4)
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, d[s >> 1][s & 1]), rsrc_c,
                                                   voff_c[s >> 1][s & 1], 0, WT);
          __builtin_amdgcn_sched_barrier(0);
        }
        TGP_STAMP(11);
        if (F) {  // (workgroup-uniform)
          float* Cx = RX.C + static_cast<long>(batch) * RX.sC + static_cast<long>(tm) * RX.sCsplit;
          const __amdgpu_buffer_rsrc_t rsrc_cx = __builtin_amdgcn_make_buffer_rsrc(Cx, 0, kb * fb * 1024, 0x00020000);
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const int br = 2 * wm + i;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, d[i][2]), rsrc_cx,
                                                   (br < kb && wn < fb) ? (br * fb + wn) * 1024 + lane * 16 : OOB, 0, WT);
          }
        }
      } else {
        float* Ca = R.C + static_cast<long>(batch) * R.sC + static_cast<long>(tm) * R.sCsplit;
        float* cp = Ca + static_cast<long>(tid >> 5) * R.ldc + (tid & 31) * 4;  // this thread's vector of slab row tid / 32
        const long cp_step = 32 * R.ldc;
        float4 pv = make_float4(0.f, 0.f, 0.f, 0.f);  // (one vector of the parked tile on its way to the slab)
#pragma unroll
        for (int s = 0; s < 32; ++s) {
          if (s == G_FREE) __syncthreads();  // (no wave reads U_r any more)
          if (s == G_FREE + G_PARK) {
            __syncthreads();  // (S^T U is parked)
            TGP_STAMP(10);
          }
          if (s + 1 < 32) fetch_x(s + 1);
#pragma unroll
          for (int i = 0; i < 2; ++i) d[i][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s & 1][i], b[s & 1][0], d[i][2], 0, 0, 0);
          if (s + 1 < 32) __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);  // ds_reads of the next group
          __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);                   // 2 x MFMA
          if (s >= G_FREE && s < G_FREE + G_PARK) {
            // S^T U to U_r's words [128][first 128 of 192], column c of row p at c ^ 16 ((p >> 2) & 1): the two lq of a
            // half-wave land on different halves of the 32 banks, so the ds_write_b32 are conflict-free, and 16-byte
            // vectors stay whole.  Two of the sixteen per group.
#pragma unroll
            for (int h = 0; h < PARK_PER; ++h) {
              const int e = PARK_PER * (s - G_FREE) + h, i = e >> 3, j = (e >> 2) & 1, r = e & 3;
              const int p = wm * 32 + 16 * i + 4 * lq + r;
              UXf[p * 192 + ((wn * 32 + 16 * j + l15) ^ ((lq & 1) << 4))] = d[i][j][r];
            }
          }
          if (s >= G_FREE + G_PARK && s < G_FREE + G_PARK + 8) {
            // rows and columns < Nc of the parked tile to the slab: 32 lanes per 512-byte row, one read or one store per group
            const int e = s - (G_FREE + G_PARK), q = e >> 1;
            const int row = (tid >> 5) + 32 * q, c4 = (tid & 31) * 4;
            if ((e & 1) == 0) pv = *reinterpret_cast<const float4*>(UXf + row * 192 + (c4 ^ (((row >> 2) & 1) << 4)));
            else if (row < Nc && c4 < Nc) *reinterpret_cast<float4*>(cp + q * cp_step) = pv;
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        TGP_STAMP(11);
        if (F) {  // columns < F of S^T X, rows < Nc (rows >= Nc are 0 * X: not zeros when X holds a NaN)
          float* Cx = RX.C + static_cast<long>(batch) * RX.sC + static_cast<long>(tm) * RX.sCsplit;
          const int col = wn * 16 + l15;
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = wm * 32 + 16 * i + 4 * lq + r;
              if (row < Nc && col < F) Cx[static_cast<long>(row) * RX.ldc + col] = d[i][2][r];
            }
        }
      }
      if (g.colsum) {  // (workgroup-uniform)
        __syncthreads();  // (S_r is dead: the eight partials per column lie there, [8][BN])
        float* part = smem;
        if (lq == 3) {
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) part[(2 * wm + i) * BN + wn * 32 + 16 * j + l15] = cpart[i][j];
        }
        __syncthreads();
        if (tid < Nc) {
          float tot = 0.f;
#pragma unroll
          for (int qq = 0; qq < 8; ++qq) tot = __fadd_rn(tot, part[qq * BN + tid]);
          g.colsum[(static_cast<long>(batch) * g.tiles_m + tm) * Nc + tid] = tot;
        }
      }
      TGP_STAMP(3);
      return;
    }
    {
      // operands of k-group s + 1 are requested before the MFMAs of group s; no branch inside (column blocks beyond
      // Nc / F -- X absent or F < 64, Nc < 128 -- are multiplied all the same and not written below: a wave-uniform
      // `if` per block compiled to a branch and a full LDS wait per block, 0.8 us of the C2 launch)
      int a_at[2], b_at[3];
#pragma unroll
      for (int i = 0; i < 2; ++i) a_at[i] = lq * BN + ((wm * 32 + 16 * i + l15) ^ (lq << 4));
#pragma unroll
      for (int j = 0; j < 3; ++j) b_at[j] = lq * 192 + ((wn * 48 + 16 * j + l15) ^ (lq << 4));
      float a[2][2], b[2][3];
      auto fetch = [&](int s) {
#pragma unroll
        for (int i = 0; i < 2; ++i) a[s & 1][i] = Sf[4 * s * BN + a_at[i]];
#pragma unroll
        for (int j = 0; j < 3; ++j) b[s & 1][j] = UXf[4 * s * 192 + b_at[j]];
      };
      fetch(0);
#pragma unroll
      for (int s = 0; s < 32; ++s) {
        if (s + 1 < 32) fetch(s + 1);
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
          for (int i = 0; i < 2; ++i)
            d[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s & 1][i], b[s & 1][j], d[i][j], 0, 0, 0);
        if (s + 1 < 32) __builtin_amdgcn_sched_group_barrier(0x100, 5, 0);  // ds_reads of group s + 1
        __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);                   // 6 x MFMA
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    TGP_STAMP(9);
    __syncthreads();  // (the result tile overwrites the operands)
    bool used[3];  // (wave-uniform) column blocks beyond Nc and beyond F are not written
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int c0 = wn * 48 + 16 * j;
      used[j] = c0 < BN ? c0 < Nc : c0 - BN < F;
    }
    float* P = smem;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (used[j]) {
#pragma unroll
          for (int r = 0; r < 4; ++r) P[(wm * 32 + 16 * i + 4 * lq + r) * P_LD + wn * 48 + 16 * j + l15] = d[i][j][r];
        }
    __syncthreads();
    TGP_STAMP(10);
    // the column sums first: they need LDS alone, and the launch then ends behind its stores
    if (g.colsum) {  // (workgroup-uniform)
      float* part = smem + BM * P_LD;  // [8][BN]
      const int j = tid & (BN - 1), q = tid >> 7;
      float cs = 0.f;
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int row = 16 * q + u;
        const float v = P[row * P_LD + j];
        cs = __fadd_rn(cs, (row >= Nc || (g.colsum_skip_diag && row == j)) ? 0.f : v);
      }
      part[q * BN + j] = cs;
      __syncthreads();
      if (tid < Nc) {
        float tot = 0.f;
#pragma unroll
        for (int qq = 0; qq < 8; ++qq) tot = __fadd_rn(tot, part[qq * BN + tid]);
        g.colsum[(static_cast<long>(batch) * g.tiles_m + tm) * Nc + tid] = tot;
      }
    }
    TGP_STAMP(11);
    // rows and columns < Nc of S^T U, columns < F of S^T X (rows >= Nc of P are 0 * U: not zeros when U holds a NaN)
    float* Ca = R.C + static_cast<long>(batch) * R.sC + static_cast<long>(tm) * R.sCsplit;
    const int kq = Nc >> 2, fq = F >> 2;
    for (int e = tid; e < Nc * kq; e += THREADS) {
      const int row = e / kq, c4 = (e - row * kq) * 4;
      *reinterpret_cast<float4*>(Ca + static_cast<long>(row) * R.ldc + c4) = *reinterpret_cast<const float4*>(P + row * P_LD + c4);
    }
    if (F) {
      float* Cx = RX.C + static_cast<long>(batch) * RX.sC + static_cast<long>(tm) * RX.sCsplit;
      for (int e = tid; e < Nc * fq; e += THREADS) {
        const int row = e / fq, c4 = (e - row * fq) * 4;
        *reinterpret_cast<float4*>(Cx + static_cast<long>(row) * RX.ldc + c4) =
            *reinterpret_cast<const float4*>(P + row * P_LD + BN + c4);
      }
    }
    TGP_STAMP(3);
    return;
  }

  // ---- epilogue: C/D layout col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5) -----------
  if constexpr (MODE == 1) {
    // rows / columns past the edge: operands were zero-filled, so acc = 0 = rres there
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float d = rres[j][r] - acc[j][r];
        sq = fmaf(d, d, sq);
      }
    if (mirror && mirror_rows) {  // (workgroup-uniform; the k-loop's last barrier has passed: the LDS is free)
      float* patch = smem + wave * (32 * 33);
#pragma unroll
      for (int j = 0; j < NT; ++j) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // patch[a][b] = resid[n0' + a][m0' + b]
          float* d = patch + ((lane >> 3) + 8 * q) * 33 + 4 * (lane & 7);
          d[0] = rmir[j][4 * q]; d[1] = rmir[j][4 * q + 1]; d[2] = rmir[j][4 * q + 2]; d[3] = rmir[j][4 * q + 3];
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float d = patch[lm * 33 + (r & 3) + 8 * (r >> 2) + 4 * lk] - acc[j][r];
          sq = fmaf(d, d, sq);
        }
        __builtin_amdgcn_wave_barrier();
      }
    } else if (mirror) {
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float d = rmir[j][r] - acc[j][r];
          sq = fmaf(d, d, sq);
        }
    }
    // fixed-order reduction: lanes (xor butterfly) -> waves (LDS, summed in wave order)
    // the order of wave_sum (wave.h), written out: a call here changes the kernel's instruction stream
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
    __syncthreads();
    if (lane == 0) smem[wave] = sq;
    __syncthreads();
    if (tid == 0) {
      float t = 0.f;
      for (int w = 0; w < THREADS / 64; ++w) t += smem[w];
      g.partial[static_cast<long>(batch) * (g.tiles_m * g.tiles_n) + tm * g.tiles_n + tn_all] = t;
    }
    return;
  }
  // Interior tiles of an aligned C leave as 16-byte stores (r5): a wave's 32 x 32 accumulator tile goes through its own
  // LDS patch [32][36] (the k-loop's last barrier has passed) and 8 lanes write one 128-byte row segment: 4 store
  // instructions per lane and tile where the scalar form issues 16 -- with 16 waves per CU the stores' address path
  // was ~1.5 us of the launch.  Edge tiles, C += and unaligned C keep the scalar stores.
  constexpr bool PATCH_FITS = (THREADS / 64) * (32 * 36) <= 2 * STAGE_FLOATS;  // (not the 16-wave 128 x 128 tile)
  const bool vec_store = ALIGNED && PATCH_FITS && TGP_VEC_EPILOGUE && !g.accumulate && (R.ldc & 3) == 0 &&
                         (reinterpret_cast<uintptr_t>(C) & 15) == 0 && m0 + BM <= M && n0 + BN <= Nc;
  if (vec_store) {  // (workgroup-uniform)
    float* patch = smem + wave * (32 * 36);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
      for (int r = 0; r < 16; ++r) patch[((r & 3) + 8 * (r >> 2) + 4 * lk) * 36 + lm] = acc[j][r];
      __builtin_amdgcn_wave_barrier();
      const int c4 = (lane & 7) * 4, r8 = lane >> 3;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int rr = r8 + 8 * q;
        const float4 v = *reinterpret_cast<const float4*>(patch + rr * 36 + c4);
        *reinterpret_cast<float4*>(C + static_cast<long>(m0 + wm * 32 + rr) * R.ldc + n0 + wn * (BN / WN) + j * 32 + c4) = v;
      }
      __builtin_amdgcn_wave_barrier();
    }
  } else {
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int col = n0 + wn * (BN / WN) + j * 32 + lm;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
      if (row < M && col < Nc) {
        float* dst = C + static_cast<long>(row) * R.ldc + col;
        *dst = g.accumulate ? __fadd_rn(*dst, acc[j][r]) : acc[j][r];
      }
    }
  }
  }
  if constexpr (MODE == 2) {
    if (vec_store) __syncthreads();  // (the patches are read; the column sums below reuse the same LDS)
    // column sums of this tile (rows beyond M are zero: the operands were zero-filled): registers in order, the two
    // half-waves, then the row waves in order through LDS (the k-loop's last barrier has passed: smem is free)
    if (g.colsum && which == 0) {  // (workgroup-uniform)
      // ... exact zeros unless the other operand holds an infinity: 0 * inf = NaN.  A tile that reaches beyond M (workgroup-
      // uniform; C is stored by now) clears those rows first, so that a NaN of the padding stays out of the degrees
      if (m0 + BM > M) {
        const int rows_left = M - (m0 + wm * 32 + 4 * lk);  // row offset of the first row beyond M
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if ((r & 3) + 8 * (r >> 2) >= rows_left) acc[j][r] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        float cs = 0.f;
        const int dcol = n0 + wn * (BN / WN) + j * 32 + lm - (m0 + wm * 32 + 4 * lk);  // row offset of the diagonal
#pragma unroll
        for (int r = 0; r < 16; ++r)
          cs = __fadd_rn(cs, (g.colsum_skip_diag && (r & 3) + 8 * (r >> 2) == dcol) ? 0.f : acc[j][r]);
        cs = wave_fold<64, 32>(cs, op_fadd_rn{});  // the two half-waves
        if (lk == 0) smem[wm * BN + wn * (BN / WN) + j * 32 + lm] = cs;
      }
      __syncthreads();
      if (tid < BN && n0 + tid < Nc) {
        float tot = 0.f;
#pragma unroll
        for (int q = 0; q < BM / 32; ++q) tot = __fadd_rn(tot, smem[q * BN + tid]);
        g.colsum[((static_cast<long>(batch) * g.splits + split) * g.tiles_m + tm) * Nc + n0 + tid] = tot;
      }
    }
  }
  TGP_STAMP(3);
}

// The buffer-load path needs dword alignment only (compute queues run in unaligned-access mode, so a 16-byte
// load may start on any dword): a vector that runs past the end of its row picks up the head of the next row,
// which is either masked (k tail, see load_a / load_b) or lands in output rows / columns that are never stored;
// past the end of the matrix the descriptor's per-dword range check returns zeros.  What remains a requirement
// is that every matrix fits the 32-bit byte offsets of a descriptor.  TGP_GEMM_SCALAR=1 forces the guarded
// scalar path (diagnostic).
static bool gemm_aligned(const GemmArgs& g, bool /*k_rows*/) {
  static const bool force_scalar = getenv("TGP_GEMM_SCALAR") && atoi(getenv("TGP_GEMM_SCALAR"));
  if (force_scalar) return false;
  auto ok = [](const void* p, long, long) { return reinterpret_cast<uintptr_t>(p) % 4 == 0; };
  bool a = ok(g.A, g.lda, g.sA);
  const long lim = (1l << 31) - 4096;
  a = a && (static_cast<long>(g.M) * g.lda * 4 < lim) && (static_cast<long>(g.Kd) * g.lda * 4 < lim);
  for (int w = 0; w < 3; ++w)
    if (w == 0 || (w == 1 && g.tiles_n > g.tiles_n0) || (w == 2 && g.tiles_n1))
      a = a && ok(g.rhs[w].Bm, g.rhs[w].ldb, g.rhs[w].sB) &&
          (static_cast<long>(g.Kd) * g.rhs[w].ldb * 4 < lim) && (static_cast<long>(g.rhs[w].Nc) * g.rhs[w].ldb * 4 < lim);
  return a;
}

// Tile shape: 128 x 128 unless that leaves the chip under two 512-thread workgroups per CU; then the
// tile is halved (128 x 64 first: twice the waves per SIMD at the same A traffic per CU-pair sharing
// an L2; 64 x 128 for short M).
struct TileCfg { int bm, bn; };
static TileCfg pick_tile(int64_t M, int64_t max_nc, int64_t batches_x_splits, const GemmArgs& g) {
  static const int fbm = getenv("TGP_GEMM_BM") ? atoi(getenv("TGP_GEMM_BM")) : 0;
  static const int fbn = getenv("TGP_GEMM_BN") ? atoi(getenv("TGP_GEMM_BN")) : 0;
  TileCfg t{128, 128};
  auto count = [&](int bm, int bn) {
    int64_t tn = 0;
    tn += (g.rhs[0].Nc + bn - 1) / bn;
    if (g.rhs[1].Bm) tn += (g.rhs[1].Nc + bn - 1) / bn;
    if (g.rhs[1].Bm && g.rhs[2].Bm) tn += (g.rhs[2].Nc + bn - 1) / bn;
    return ((M + bm - 1) / bm) * tn * batches_x_splits;
  };
  if (M <= 64) t.bm = 64;
  if (count(t.bm, 128) < 2 * 256 && max_nc >= 64) t.bn = 64;
  if (count(t.bm, t.bn) < 2 * 256 && t.bm == 128 && M > 64) t.bm = 64;
  if (g.force_bm) t.bm = g.force_bm;
  if (g.force_bn) t.bn = g.force_bn;
  if (fbm == 64 || fbm == 128) t.bm = fbm;
  if (fbn == 64 || fbn == 128) t.bn = fbn;
  return t;
}

template <bool A_KMAJOR, int BM, int BN, int MODE = 0, int WN = 2>
static void launch_gemm_cfg(const GemmArgs& g_in, int batches, hipStream_t stream) {
  const GemmArgs& g = g_in;
  const int nwg = batches * g.splits * g.tiles_m * g.tiles_n;
  const size_t lds = 2 * (BM * LDA_ROWMAJOR + (MODE == 1 ? BN * LDA_ROWMAJOR : BK * BN)) * sizeof(float);
  if (gemm_aligned(g, A_KMAJOR && MODE == 0))
    hipLaunchKernelGGL((gemm_f32_mfma_kernel<A_KMAJOR, true, BM, BN, MODE, WN>), dim3(nwg), dim3(BM * 2 * WN), lds, stream, g);
  else
    hipLaunchKernelGGL((gemm_f32_mfma_kernel<A_KMAJOR, false, BM, BN, MODE, WN>), dim3(nwg), dim3(BM * 2 * WN), lds, stream, g);
}

// g.tiles_* are filled in here: they follow from the tile shape chosen for this problem.  Returns whether g.colsum was
// written (only the 64 x 64 tile has the MODE 2 epilogue; *tiles_m_out = row tiles per batch element of that layout).
template <bool A_KMAJOR>
static bool launch_gemm(GemmArgs g, int batches, hipStream_t stream, int* tiles_m_out = nullptr) {
  int64_t max_nc = g.rhs[1].Bm && g.rhs[1].Nc > g.rhs[0].Nc ? g.rhs[1].Nc : g.rhs[0].Nc;
  const bool third = g.rhs[1].Bm && g.rhs[2].Bm;  // (a third right-hand side only behind a second one)
  if (third && g.rhs[2].Nc > max_nc) max_nc = g.rhs[2].Nc;
  const TileCfg t = pick_tile(g.M, max_nc, static_cast<int64_t>(batches) * g.splits, g);
  g.tiles_m = cdiv(g.M, t.bm);
  g.tiles_n0 = cdiv(g.rhs[0].Nc, t.bn);
  g.tiles_n = g.tiles_n0 + (g.rhs[1].Bm ? cdiv(g.rhs[1].Nc, t.bn) : 0);
  g.tiles_n1 = 0;
  if (third) {
    g.tiles_n1 = g.tiles_n;
    g.tiles_n += cdiv(g.rhs[2].Nc, t.bn);
  }
  if (tiles_m_out) *tiles_m_out = g.tiles_m;
  if (t.bm == 64 && t.bn == 64 && g.colsum) {
    launch_gemm_cfg<A_KMAJOR, 64, 64, 2>(g, batches, stream);
    return true;
  }
  if (t.bm == 64 && t.bn == 64) launch_gemm_cfg<A_KMAJOR, 64, 64>(g, batches, stream);
  else if (t.bm == 64) launch_gemm_cfg<A_KMAJOR, 64, 128>(g, batches, stream);
  else if (t.bn == 64) launch_gemm_cfg<A_KMAJOR, 128, 64>(g, batches, stream);
  else launch_gemm_cfg<A_KMAJOR, 128, 128, 0, 4>(g, batches, stream);  // 16 waves (4 x 4), one 32x32 tile each
  return false;
}

// U = A S of the dense poolers (MODE 3): A is an adjacency, mostly zeros, and the k-steps whose A chunk is sparse skip
// their MFMAs (see gemm_f32_mfma_kernel).  128 x 128 tiles, 16 waves: at K <= 128 one column tile, so every A panel is
// read from HBM once.  Grids of fewer than 256 such tiles (fewer graphs than C2's 32 at N = 1024) would leave CUs
// idle and keep pick_tile's tiles; so does what MODE 3 does not cover (split / accumulating / multi-rhs launches,
// operands past the 32-bit descriptor range).
template <bool A_KMAJOR>
static void launch_gemm_skip_zeros(GemmArgs g, int batches, hipStream_t stream) {
  if (g.splits != 1 || g.accumulate || g.rhs[1].Bm || g.colsum || g.m_ptr || g.k_ptr || !gemm_aligned(g, A_KMAJOR)) {
    launch_gemm<A_KMAJOR>(g, batches, stream);
    return;
  }
  constexpr int BM = 128, BN = 128, WN = 4;
  const int tiles_m = cdiv(g.M, BM), tiles_n = cdiv(g.rhs[0].Nc, BN);
  const int nwg = batches * tiles_m * tiles_n;
  if (nwg < 256) {  // a 128 x 128 grid would leave CUs idle: pick_tile's smaller tiles and the MODE 0 kernel
    launch_gemm<A_KMAJOR>(g, batches, stream);
    return;
  }
  g.tiles_m = tiles_m;
  g.tiles_n0 = g.tiles_n = tiles_n;
  g.tiles_n1 = 0;
  // row-major A: the wide front-end's two Bm chunks [128][BN], its records and 1 KB per wave (the k-loop's stages lie inside)
  constexpr size_t lds = A_KMAJOR ? 2 * (BM * LDA_ROWMAJOR + BK * BN) * sizeof(float) + 2 * 16 * sizeof(unsigned)
                                  : 2 * 128 * BN * sizeof(float) + (2 * 16 + 16 * 256) * sizeof(unsigned);
  static_assert(A_KMAJOR || 2 * 128 * BN >= 2 * (BM * LDA_ROWMAJOR + BK * BN) + 2 * 16, "MODE 3: the wide chunks cover the stages");
  if constexpr (!A_KMAJOR)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_f32_mfma_kernel<A_KMAJOR, true, BM, BN, 3, WN>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
  hipLaunchKernelGGL((gemm_f32_mfma_kernel<A_KMAJOR, true, BM, BN, 3, WN>), dim3(nwg), dim3(BM * 2 * WN), lds, stream, g);
}

// U = A S with S^T [U | X] folded in (MODE 4): where launch_gemm_skip_zeros takes MODE 3 with a single column tile, a
// workgroup ends its k-loop holding complete rows of U, and S_r^T [U_r | X_r] over those rows is one of tiles_m partial
// slabs of the second product -- no launch of its own, no U in memory, nothing shared between workgroups.  The caller
// has checked the shape (fold_tiles) and the slabs' alignment; this returns false, having launched nothing, when MODE 3
// would not be taken.  g.rhs[0].C / rhs[1] / colsum as described at GemmArgs.
constexpr int FOLD_BM = 128, FOLD_MAX_F = 64;
static int fold_tiles(int64_t N, int64_t K, int64_t F) {  // row tiles per graph, 0 = the shape does not fold
  return (K <= 128 && K % 4 == 0 && F <= FOLD_MAX_F && F % 4 == 0) ? cdiv(N, FOLD_BM) : 0;
}
// Floats of one slab of the folded route, rows x cols of S^T U (K x K) or S^T X (K x F).  TGP_FOLD_BLOCKS: an array of
// 16 x 16 blocks, block row major, 256 floats per block; element (p, c) lies in block (p / 16, c / 16) at word
// 4 lane + r with lane = 16 ((p % 16) / 4) + c % 16 and r = p % 4 -- d[r] of that lane in v_mfma_f32_16x16x4_f32's
// accumulator layout.  Blocks wholly beyond rows / cols do not exist; otherwise the slab is row-major.
static int64_t fold_slab_floats(int64_t rows, int64_t cols) {
  return TGP_FOLD_BLOCKS ? ((rows + 15) / 16) * ((cols + 15) / 16) * 256 : rows * cols;
}
template <bool A_KMAJOR>
static bool launch_gemm_fold(GemmArgs g, int batches, hipStream_t stream) {
  constexpr int BM = FOLD_BM, BN = 128, WN = 4;
  const GemmRhs x = g.rhs[1];
  g.rhs[1] = GemmRhs{};  // (gemm_aligned looks at the first right-hand side only: X is checked here)
  const long lim = (1l << 31) - 4096;
  if (!gemm_aligned(g, A_KMAJOR) || g.rhs[0].Nc > BN ||
      (x.Bm && (reinterpret_cast<uintptr_t>(x.Bm) % 4 != 0 || x.Nc > FOLD_MAX_F || (static_cast<long>(g.Kd) + BM) * x.ldb * 4 >= lim)))
    return false;
  g.rhs[1] = x;
  g.tiles_m = cdiv(g.M, BM);
  g.tiles_n0 = g.tiles_n = 1;
  g.tiles_n1 = 0;
  g.splits = 1;
  const int nwg = batches * g.tiles_m;
  if (nwg < 256) return false;
  // the tail's operands S_r [128][128] and [U_r | X_r] [128][192] (the k-loop's stages and the result tile lie inside)
  constexpr size_t lds = (BM * BN + BM * 192) * sizeof(float);  // = 160 KB: the whole LDS of a CU
  static_assert(BM * BN + BM * 192 >= BM * 196 + 8 * BN && BM * 196 + 8 * BN >= 2 * (BM * LDA_ROWMAJOR + BK * BN) + 2 * 16,
                "MODE 4: the tail's operands cover its result tile, which covers the k-loop's stages");
  static_assert(BM * BN + BM * 192 >= 2 * 128 * BN + 2 * 16 + 16 * 256, "MODE 4: ... and the wide front-end's two Bm chunks, records and turn areas");
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_f32_mfma_kernel<A_KMAJOR, true, BM, BN, 4, WN>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
  hipLaunchKernelGGL((gemm_f32_mfma_kernel<A_KMAJOR, true, BM, BN, 4, WN>), dim3(nwg), dim3(BM * 2 * WN), lds, stream, g);
  return true;
}

// MODE 1 launch: sum((resid - A Bm^T)^2) per tile into g.partial; returns tiles per batch element.
static int launch_gemm_residual(GemmArgs g, int batches, hipStream_t stream, bool dry_run = false) {
  TileCfg t = pick_tile(g.M, g.rhs[0].Nc, batches, g);
  // a short k-loop (Kd <= 8 stages: the link loss at K <= 256) is all prologue, residual loads and epilogue: 64 x 64
  // tiles keep four workgroups per CU in different phases (C2, symmetric form: 0.0903 -> 0.0764 ms for the call)
  if (g.symmetric && g.Kd <= 8 * BK && !g.force_bm && !g.force_bn && t.bm == 128 && t.bn == 128) t = TileCfg{64, 64};
  g.tiles_m = cdiv(g.M, t.bm);
  g.tiles_n0 = g.tiles_n = cdiv(g.rhs[0].Nc, t.bn);
  if (dry_run) return g.tiles_m * g.tiles_n;
  static const int no_sym = getenv("TGP_LINK_LOSS_FULL") ? atoi(getenv("TGP_LINK_LOSS_FULL")) : 0;
  if (t.bm != t.bn || g.M != g.rhs[0].Nc || g.rhs[0].Bm != g.A || g.rhs[0].sB != g.sA || g.rhs[0].ldb != g.lda || no_sym)
    g.symmetric = 0;  // (only S S^T against a square residual on square tiles)
  if (t.bm == 64 && t.bn == 64) launch_gemm_cfg<false, 64, 64, 1>(g, batches, stream);
  else if (t.bm == 64) launch_gemm_cfg<false, 64, 128, 1>(g, batches, stream);
  else if (t.bn == 64) launch_gemm_cfg<false, 128, 64, 1>(g, batches, stream);
  else launch_gemm_cfg<false, 128, 128, 1, 4>(g, batches, stream);
  return g.tiles_m * g.tiles_n;
}

}  // namespace tgp
