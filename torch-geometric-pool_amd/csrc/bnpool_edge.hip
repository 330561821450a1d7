// BN-Pool's sampled-edge reconstruction loss (unbatched mode; reference poolers/bnpool.py get_sparse_rec_loss,
// utils/losses.py:1520-1562) over a positive list P and a negative list Q that stay two lists:
//   l_e = <T[u], S[v]>, T = S K,   bce_e = max(l, 0) - l y + log1p(exp(-|l|)),   y = 1 on P, 0 on Q
//   node_loss[u] = sum over u's out-edges of bce_e: first its group in P, then its group in Q, each in edge-list order
// Nothing of size E' x K is formed.  Forward (bnedge_fwd_kernel): G lanes own one source node (64 / G nodes per wave),
// keep T[u] in registers and walk both by-source groups as one sequence in rounds of D edges.  A round's D rows of S are
// all requested before the first is consumed, and the D edge positions and endpoints of the NEXT round are requested
// before this round's arithmetic: the walk waits on gathers, never on a row it could have asked for earlier.  Every edge
// is a dot product over the lane's columns, the fold of wave_sum<G> (offsets G / 2 .. 1), and the loss in every lane of
// the group; d_e = sigmoid(l_e) - y_e is written at the edge's own position when a gradient is wanted.
// Backward (bnedge_bwd_kernel, launched by source and by destination): the owner of a row accumulates
//   dT[u] = sum_{e out of u} c d_e S[v_e]        dSv[v] = sum_{e into v} c d_e T[u_e]        c = c[graph of the SOURCE]
// in registers in the same order (P's group, then Q's) and writes the row once.  No float atomics anywhere: the same
// input gives the same bits.  An edge position outside its list, an endpoint outside [0, N) or a graph id outside
// [0, num_graphs) contributes nothing, is never dereferenced and sets a bit of the status word.
#include "common.h"
#include "edge_walk.h"

namespace tgp {
namespace {

constexpr int BNEDGE_DEPTH = 4;  // row gathers a lane group keeps in flight

struct EdgeList {  // an edge-group index over one list and the row of the list at the far end of every position
  const int32_t* ptr;
  const int32_t* perm;
  const int64_t* far;
  int64_t E;
};

// the lane's share of a row: C chunks of W columns, chunk c at column sub * W + c * G * W
template <int G, bool VEC>
struct RowShare {
  static constexpr int W = VEC ? 4 : 1;
  static constexpr int C = (!VEC && G == 64) ? 4 : 1;  // scalar loads of a row past 64 columns: up to four per lane
  float v[C][W];

  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int j = 0; j < W; ++j) v[c][j] = 0.0f;
  }
  __device__ __forceinline__ void load(const float* __restrict__ row, int sub, int K) {
#pragma unroll
    for (int c = 0; c < C; ++c) load_unit<VEC>(row, sub * W + c * G * W, K, 0.0f, v[c]);
  }
  __device__ __forceinline__ void store(float* __restrict__ row, int sub, int K) const {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int k = sub * W + c * G * W;
      if constexpr (VEC) {
        if (k + 4 <= K) {
          *reinterpret_cast<float4*>(row + k) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
          continue;
        }
      }
#pragma unroll
      for (int j = 0; j < W; ++j)
        if (k + j < K) row[k + j] = v[c][j];
    }
  }
};

struct Entry {  // one step of a node's walk: the edge's position in its list and its far endpoint (-1: skipped)
  int64_t pos, far;
  bool live, in_a;
};

// step t of the walk "group a, then group b"
__device__ __forceinline__ Entry entry_of(const EdgeList& A, const EdgeList& B, int64_t ba, int64_t bb, int len_a,
                                          int len, int t, int64_t n) {
  Entry en{-1, -1, t < len, t < len_a};
  if (en.live) {
    const EdgeList& L = en.in_a ? A : B;
    en.far = source_of(L.perm, L.far, en.in_a ? ba + t : bb + (t - len_a), L.E, n, &en.pos);
  }
  return en;
}

__device__ __forceinline__ int group_len(const Group& g) { return g.e > g.b ? static_cast<int>(g.e - g.b) : 0; }

template <int G, bool VEC>
__global__ __launch_bounds__(256) void bnedge_fwd_kernel(const float* __restrict__ S, const float* __restrict__ T,
                                                         int64_t n, int K, EdgeList P, EdgeList Q,
                                                         float* __restrict__ node_loss, float* __restrict__ d_p,
                                                         float* __restrict__ d_q, uint32_t* __restrict__ status) {
  using Row = RowShare<G, VEC>;
  constexpr int PER = 64 / G, D = BNEDGE_DEPTH;
  const int lane = threadIdx.x & 63, sub = lane % G, slot = lane / G;
  const int64_t wave = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6;
  if (wave * PER >= n) return;  // (the whole wave: the folds below need every lane of a wave that stays)
  const int64_t u = wave * PER + slot;
  const bool own = u < n;
  Group gp{0, 0}, gq{0, 0};
  Row t;
  t.zero();
  if (own) {
    gp = group_of(P.ptr, u, P.E);
    gq = group_of(Q.ptr, u, Q.E);
    t.load(T + u * K, sub, K);
  }
  const int len_p = group_len(gp), len = len_p + group_len(gq);
  const int rounds = wave_max((len + D - 1) / D);  // every lane takes part in every fold
  float acc = 0.0f;
  bool bad = false;
  Entry nxt[D];
#pragma unroll
  for (int d = 0; d < D; ++d) nxt[d] = entry_of(P, Q, gp.b, gq.b, len_p, len, d, n);
  for (int r = 0; r < rounds; ++r) {
    Entry cur[D];
    Row s[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      cur[d] = nxt[d];
      s[d].zero();
      if (cur[d].far >= 0) s[d].load(S + cur[d].far * K, sub, K);
    }
#pragma unroll
    for (int d = 0; d < D; ++d) nxt[d] = entry_of(P, Q, gp.b, gq.b, len_p, len, (r + 1) * D + d, n);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      float dot = 0.0f;
#pragma unroll
      for (int c = 0; c < Row::C; ++c)
#pragma unroll
        for (int j = 0; j < Row::W; ++j) dot = fmaf(t.v[c][j], s[d].v[c][j], dot);
      const float l = wave_sum<G>(dot);
      if (!cur[d].live) continue;
      if (cur[d].far < 0) bad = true;
      const float y = cur[d].in_a ? 1.0f : 0.0f;
      const float ex = expf(-fabsf(l));
      if (cur[d].far >= 0) acc = acc + ((fmaxf(l, 0.0f) - l * y) + log1pf(ex));
      float* dout = cur[d].in_a ? d_p : d_q;
      const int64_t E = cur[d].in_a ? P.E : Q.E;
      if (dout && sub == 0 && static_cast<uint64_t>(cur[d].pos) < static_cast<uint64_t>(E))
        dout[cur[d].pos] = cur[d].far >= 0 ? (l >= 0.0f ? 1.0f : ex) / (1.0f + ex) - y : 0.0f;
    }
  }
  if (own && sub == 0) {
    node_loss[u] = acc;
    if (bad) atomicOr(status, 1u);
  }
}

// out[i] = sum over i's groups in A and then in B of (c d_e) X[far_e], c = cvec[graph of the edge's source]: the source is
// the owner (far_is_source 0: the by-source walk, X = S) or the far endpoint (1: the by-destination walk, X = T).
template <int G, bool VEC>
__global__ __launch_bounds__(256) void bnedge_bwd_kernel(const float* __restrict__ X, int64_t n, int K, EdgeList A,
                                                         EdgeList B, const float* __restrict__ d_a,
                                                         const float* __restrict__ d_b, const int64_t* __restrict__ batch,
                                                         const float* __restrict__ cvec, int64_t num_graphs,
                                                         int far_is_source, float* __restrict__ out,
                                                         uint32_t* __restrict__ status) {
  using Row = RowShare<G, VEC>;
  constexpr int PER = 64 / G, D = BNEDGE_DEPTH;
  const int lane = threadIdx.x & 63, sub = lane % G, slot = lane / G;
  const int64_t i = ((static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6) * PER + slot;
  if (i >= n) return;
  const Group ga = group_of(A.ptr, i, A.E), gb = group_of(B.ptr, i, B.E);
  const int len_a = group_len(ga), len = len_a + group_len(gb);
  bool bad = false;
  float c_own = 0.0f;
  if (!far_is_source) {
    const int64_t g = batch ? batch[i] : 0;
    if (static_cast<uint64_t>(g) < static_cast<uint64_t>(num_graphs)) c_own = cvec[g];
    else bad = len > 0;
  }
  Row acc;
  acc.zero();
  Entry nxt[D];
#pragma unroll
  for (int d = 0; d < D; ++d) nxt[d] = entry_of(A, B, ga.b, gb.b, len_a, len, d, n);
  for (int r = 0; r * D < len; ++r) {
    Entry cur[D];
    Row x[D];
    float w[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      cur[d] = nxt[d];
      x[d].zero();
      w[d] = 0.0f;
      if (cur[d].far >= 0) {
        x[d].load(X + cur[d].far * K, sub, K);
        float c = c_own;
        if (far_is_source) {
          const int64_t g = batch ? batch[cur[d].far] : 0;
          if (static_cast<uint64_t>(g) < static_cast<uint64_t>(num_graphs)) c = cvec[g];
          else bad = true;
        }
        w[d] = c * (cur[d].in_a ? d_a : d_b)[cur[d].pos];
      } else if (cur[d].live) {
        bad = true;
      }
    }
#pragma unroll
    for (int d = 0; d < D; ++d) nxt[d] = entry_of(A, B, ga.b, gb.b, len_a, len, (r + 1) * D + d, n);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      if (cur[d].far < 0) continue;
#pragma unroll
      for (int c = 0; c < Row::C; ++c)
#pragma unroll
        for (int j = 0; j < Row::W; ++j) acc.v[c][j] = fmaf(w[d], x[d].v[c][j], acc.v[c][j]);
    }
  }
  acc.store(out + i * K, sub, K);
  if (bad && sub == 0) atomicOr(status, far_is_source ? 4u : 2u);
}

__global__ void bnedge_clear_kernel(uint32_t* status) { *status = 0u; }

inline unsigned bnedge_blocks(int64_t n, int G) { return static_cast<unsigned>(cdiv(n, 4 * (64 / G))); }

template <int G, bool VEC>
struct LaunchFwd {
  static void go(const float* S, const float* T, int64_t n, int K, EdgeList P, EdgeList Q, float* node_loss, float* d_p,
                 float* d_q, uint32_t* status, hipStream_t stream) {
    hipLaunchKernelGGL((bnedge_fwd_kernel<G, VEC>), dim3(bnedge_blocks(n, G)), dim3(256), 0, stream, S, T, n, K, P, Q,
                       node_loss, d_p, d_q, status);
  }
};

template <int G, bool VEC>
struct LaunchBwd {
  static void go(const float* X, int64_t n, int K, EdgeList A, EdgeList B, const float* d_a, const float* d_b,
                 const int64_t* batch, const float* cvec, int64_t num_graphs, int far_is_source, float* out,
                 uint32_t* status, hipStream_t stream) {
    hipLaunchKernelGGL((bnedge_bwd_kernel<G, VEC>), dim3(bnedge_blocks(n, G)), dim3(256), 0, stream, X, n, K, A, B, d_a,
                       d_b, batch, cvec, num_graphs, far_is_source, out, status);
  }
};

int check_lists(const char* what, int64_t N, int64_t K, const EdgeList& P, const EdgeList& Q) {
  if (int rc = check_index_sizes(what, N, P.E)) return rc;
  if (int rc = check_index_sizes(what, N, Q.E)) return rc;
  TGP_REQUIRE(P.E + Q.E <= INT32_MAX - 2 * BNEDGE_DEPTH, TGP_ERR_RANGE, "%s: the two lists together beyond the int32 walk", what);
  TGP_REQUIRE(K >= 1 && K <= tgp_bnpool_max_clusters(), TGP_ERR_INVALID, "%s: K=%lld outside 1 .. %d", what,
              static_cast<long long>(K), tgp_bnpool_max_clusters());
  TGP_REQUIRE(N == 0 || (P.ptr && Q.ptr && (P.E == 0 || P.far) && (Q.E == 0 || Q.far)), TGP_ERR_INVALID,
              "%s: null index pointer", what);
  return TGP_OK;
}

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace
}  // namespace tgp

using namespace tgp;

extern "C" int tgp_bnedge_fwd_f32(const float* S, const float* T, int64_t N, int64_t K, const int32_t* p_ptr,
                                  const int32_t* p_perm, const int64_t* p_dst, int64_t Ep, const int32_t* q_ptr,
                                  const int32_t* q_perm, const int64_t* q_dst, int64_t En, float* node_loss, float* d_p,
                                  float* d_q, uint32_t* status, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const EdgeList P{p_ptr, p_perm, p_dst, Ep}, Q{q_ptr, q_perm, q_dst, En};
  if (int rc = check_lists("tgp_bnedge_fwd_f32", N, K, P, Q)) return rc;
  TGP_REQUIRE(status, TGP_ERR_INVALID, "tgp_bnedge_fwd_f32: no status word");
  hipLaunchKernelGGL(bnedge_clear_kernel, dim3(1), dim3(1), 0, stream, status);
  if (N == 0) return check_launch("tgp_bnedge_fwd_f32");
  TGP_REQUIRE(S && T && node_loss, TGP_ERR_INVALID, "tgp_bnedge_fwd_f32: null pointer");
  const bool vec = K % 4 == 0 && aligned16(S) && aligned16(T);
  dispatch_row_layout<LaunchFwd>(vec, vec ? K / 4 : K, S, T, N, static_cast<int>(K), P, Q, node_loss, d_p, d_q, status,
                                 stream);
  return check_launch("tgp_bnedge_fwd_f32");
}

extern "C" int tgp_bnedge_bwd_f32(const float* S, const float* T, int64_t N, int64_t K, const int64_t* batch,
                                  const float* c, int64_t num_graphs, const int32_t* p_ptr, const int32_t* p_perm,
                                  const int64_t* p_dst, int64_t Ep, const int32_t* q_ptr, const int32_t* q_perm,
                                  const int64_t* q_dst, int64_t En, const int32_t* pd_ptr, const int32_t* pd_perm,
                                  const int64_t* p_src, const int32_t* qd_ptr, const int32_t* qd_perm,
                                  const int64_t* q_src, const float* d_p, const float* d_q, float* dT, float* dSv,
                                  uint32_t* status, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const EdgeList P{p_ptr, p_perm, p_dst, Ep}, Q{q_ptr, q_perm, q_dst, En};
  const EdgeList Pd{pd_ptr, pd_perm, p_src, Ep}, Qd{qd_ptr, qd_perm, q_src, En};
  if (int rc = check_lists("tgp_bnedge_bwd_f32", N, K, P, Q)) return rc;
  if (dSv)
    if (int rc = check_lists("tgp_bnedge_bwd_f32", N, K, Pd, Qd)) return rc;
  TGP_REQUIRE(status && num_graphs >= 1, TGP_ERR_INVALID, "tgp_bnedge_bwd_f32: no status word or no graph");
  hipLaunchKernelGGL(bnedge_clear_kernel, dim3(1), dim3(1), 0, stream, status);
  if (N == 0) return check_launch("tgp_bnedge_bwd_f32");
  TGP_REQUIRE(S && T && c && dT && (Ep == 0 || d_p) && (En == 0 || d_q), TGP_ERR_INVALID,
              "tgp_bnedge_bwd_f32: null pointer");
  const bool vec = K % 4 == 0 && aligned16(S) && aligned16(T) && aligned16(dT) && aligned16(dSv);
  const int64_t units = vec ? K / 4 : K;
  dispatch_row_layout<LaunchBwd>(vec, units, S, N, static_cast<int>(K), P, Q, d_p, d_q, batch, c, num_graphs, 0, dT,
                                 status, stream);
  if (dSv)
    dispatch_row_layout<LaunchBwd>(vec, units, T, N, static_cast<int>(K), Pd, Qd, d_p, d_q, batch, c, num_graphs, 1, dSv,
                                   status, stream);
  return check_launch("tgp_bnedge_bwd_f32");
}
