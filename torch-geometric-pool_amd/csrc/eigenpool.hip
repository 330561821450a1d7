// EigenPooling (reference select/eigenpool_select.py, reduce/eigenpool_reduce.py, lift/eigenpool_lift.py): the
// per-cluster eigenmodes of the induced Laplacians, and Reduce / Lift over the compact pooling matrix.
//
// The reference's Theta [n, K H] has at most H non-zeros per row (a node sits in one cluster and carries H eigenvector
// entries), so it is kept as theta_modes [N, H] plus the node list of every (graph, cluster) group.
//   modes:  one workgroup per group.  The induced sub-adjacency is gathered from the by-source edge index into LDS,
//           the reference's Laplacian is formed and its symmetric eigenproblem solved in float64 by a cyclic Jacobi
//           iteration whose rotation order (round-robin pairs) does not depend on the data; one rounding to fp32.
//   reduce: X_pool[g, h F + f] = sum over the group's nodes, ascending, of theta[i, h] x[i, f]; a row of x is read once
//           for (up to 8) modes, every (group, mode, feature) is added by one lane -- or, when the batch has a long
//           group, by 4 or 16 lanes over consecutive row ranges folded in ascending order: no float atomics, the same
//           bits on every call.
//   lift:   X_lift[i, f] = sum_h theta[i, h] X_pool[g(i), h F + f].  The two are each other's adjoint.
#include "common.h"

namespace tgp {
namespace {

constexpr int EIG_MAX_GROUP = 96;    // nodes of a group one workgroup solves: 2 x 96 x 97 doubles = 146 KB of the 160 KB LDS
constexpr int EIG_THREADS = 256;
constexpr int EIG_MAX_SWEEPS = 40;   // cyclic Jacobi converges quadratically: 6 .. 10 sweeps at these sizes
constexpr int EIG_MODE_CHUNK = 8;    // modes one pass of the Reduce kernel keeps in registers
constexpr int EIG_REDUCE_ONE_WAVE = 128;   // longest group one wave still adds alone; beyond it 4, beyond 1024 16 waves
constexpr int EIG_REDUCE_FOUR_WAVES = 1024;

// status bits of the modes kernel
constexpr int EIG_BAD_INPUT = 1;     // an index outside its table
constexpr int EIG_ASYMMETRIC = 2;    // a group whose induced adjacency is not symmetric: nothing written for it
constexpr int EIG_OVER_LIMIT = 4;    // a group larger than max_m: nothing written for it

struct EigLds {
  int ld;
  size_t a, v, cs, lam, dis, scl, mem, ord, total;
};
inline EigLds eig_lds_layout(int max_m) {
  EigLds l;
  l.ld = max_m | 1;  // odd row stride: a column walk does not stay in one bank pair
  size_t off = 0;
  l.a = off;   off += sizeof(double) * max_m * l.ld;
  l.v = off;   off += sizeof(double) * max_m * l.ld;
  l.cs = off;  off += sizeof(double) * 2 * (max_m / 2 + 1);
  l.lam = off; off += sizeof(double) * max_m;
  l.dis = off; off += sizeof(double) * max_m;
  l.scl = off; off += sizeof(double) * max_m;
  l.mem = off; off += sizeof(int) * max_m;
  l.ord = off; off += sizeof(int) * max_m;
  l.total = off;
  return l;
}

// position of `node` in the ascending list mem[0 .. m), or -1
__device__ __forceinline__ int eig_local_of(const int* mem, int m, int node) {
  int lo = 0, hi = m;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (mem[mid] < node) lo = mid + 1;
    else hi = mid;
  }
  return (lo < m && mem[lo] == node) ? lo : -1;
}

// pair i of step r of the round-robin schedule over n (even) players: n / 2 disjoint pairs, every pair once in n - 1 steps
__device__ __forceinline__ void eig_pair(int n, int r, int i, int& p, int& q) {
  int a, b;
  if (i == 0) {
    a = n - 1;
    b = r;
  } else {
    a = (r + i) % (n - 1);
    b = (r - i + (n - 1)) % (n - 1);
  }
  p = a < b ? a : b;
  q = a < b ? b : a;
}

struct ModesArgs {
  const int32_t* grp_ptr;    // [N + 1] by-source offsets
  const int32_t* grp_perm;   // [E] edge positions by source (NULL: the list is grouped already)
  const int64_t* dst;        // [E]
  const float* w;            // [E] or NULL
  const int32_t* gid;        // [N] group of every node
  const int32_t* theta_ptr;  // [G + 1]
  const int32_t* theta_perm; // [N]
  int N, E, G, H, max_m, normalized, embed;
  float* theta;              // [N, H]
  float* deg;                // [N] or NULL
  int32_t* status;
  EigLds l;
};

__global__ __launch_bounds__(EIG_THREADS) void eig_modes_kernel(ModesArgs p) {
  extern __shared__ double eig_smem[];
  char* const base = reinterpret_cast<char*>(eig_smem);
  double* const A = reinterpret_cast<double*>(base + p.l.a);
  double* const V = reinterpret_cast<double*>(base + p.l.v);
  double* const cs = reinterpret_cast<double*>(base + p.l.cs);
  double* const lam = reinterpret_cast<double*>(base + p.l.lam);
  double* const dis = reinterpret_cast<double*>(base + p.l.dis);
  double* const scl = reinterpret_cast<double*>(base + p.l.scl);
  int* const mem = reinterpret_cast<int*>(base + p.l.mem);
  int* const ord = reinterpret_cast<int*>(base + p.l.ord);
  const int ld = p.l.ld, tid = threadIdx.x, T = blockDim.x;
  const int g = blockIdx.x;

  const int t0 = p.theta_ptr[g], t1 = p.theta_ptr[g + 1];
  if (t0 < 0 || t1 < t0 || t1 > p.N) {  // (uniform)
    if (tid == 0) atomicOr(p.status, EIG_BAD_INPUT);
    return;
  }
  const int m = t1 - t0;
  if (m == 0) return;
  if (m > p.max_m) {
    if (tid == 0) atomicOr(p.status, EIG_OVER_LIMIT);
    return;
  }
  // the members, ascending; every one must be a node of this group
  int bad = 0;
  for (int a = tid; a < m; a += T) {
    const int node = p.theta_perm[t0 + a];
    if (node < 0 || node >= p.N || p.gid[node] != g) {
      bad = 1;
      mem[a] = 0;
    } else {
      mem[a] = node;
    }
  }
  for (int i = tid; i < m * ld; i += T) {
    A[i] = 0.0;
    V[i] = 0.0;
  }
  if (__syncthreads_or(bad)) {
    if (tid == 0) atomicOr(p.status, EIG_BAD_INPUT);
    return;
  }
  for (int a = tid + 1; a < m; a += T)
    if (mem[a - 1] >= mem[a]) bad = 1;
  if (__syncthreads_or(bad)) {
    if (tid == 0) atomicOr(p.status, EIG_BAD_INPUT);
    return;
  }
  // induced sub-adjacency: row a is owned by one thread, which adds its node's edges in edge-list order (fp32, as the
  // reference's dense adjacency is)
  for (int a = tid; a < m; a += T) {
    const int node = mem[a];
    const int e0 = p.grp_ptr[node], e1 = p.grp_ptr[node + 1];
    if (e0 < 0 || e1 < e0 || e1 > p.E) {
      bad = 1;
      continue;
    }
    for (int e = e0; e < e1; ++e) {
      const int pos = p.grp_perm ? p.grp_perm[e] : e;
      if (pos < 0 || pos >= p.E) {
        bad = 1;
        continue;
      }
      const int64_t j = p.dst[pos];
      if (j < 0 || j >= p.N) {
        bad = 1;
        continue;
      }
      if (p.gid[j] != g) continue;
      const int b = eig_local_of(mem, m, static_cast<int>(j));
      if (b < 0) {
        bad = 1;
        continue;
      }
      const float wv = p.w ? p.w[pos] : 1.0f;
      A[a * ld + b] = static_cast<double>(static_cast<float>(A[a * ld + b]) + wv);
    }
  }
  if (__syncthreads_or(bad)) {
    if (tid == 0) atomicOr(p.status, EIG_BAD_INPUT);
    return;
  }
  if (m == 1) {  // a one-node group carries its own self-loop weight in every mode
    const float v = static_cast<float>(A[0]);
    for (int h = tid; h < p.H; h += T) p.theta[static_cast<int64_t>(mem[0]) * p.H + h] = v;
    if (tid == 0 && p.deg) p.deg[mem[0]] = v;
    return;
  }
  // symmetric?  (a pair with a NaN in it does not count against the group: its modes are NaN on either route, and
  // they stay inside the group here)
  for (int i = tid; i < m * m; i += T) {
    const int a = i / m, b = i - a * m;
    if (a < b) {
      const double u = A[a * ld + b], v = A[b * ld + a];
      if (u != v && u == u && v == v) bad = 1;
    }
  }
  if (__syncthreads_or(bad)) {
    if (tid == 0) atomicOr(p.status, EIG_ASYMMETRIC);
    return;
  }
  // degrees: column sums, ascending rows
  for (int b = tid; b < m; b += T) {
    double d = 0.0;
    for (int a = 0; a < m; ++a) d += A[a * ld + b];
    lam[b] = d;
    if (p.deg) p.deg[mem[b]] = static_cast<float>(d);
    if (p.normalized) {
      const double dd = d + 1.401298464324817e-45;  // the smallest positive fp32 subnormal (np.spacing of an fp32 zero)
      dis[b] = 1.0 / sqrt(dd);
    }
    scl[b] = d > 0.0 ? 1.0 / sqrt(d) : 1.0;  // the embedding's D^-1/2; a node without induced edges keeps its entry
  }
  __syncthreads();
  // L (into A) and V = I
  for (int i = tid; i < m * m; i += T) {
    const int a = i / m, b = i - a * m;
    const double av = A[a * ld + b];
    double lv;
    if (p.normalized) lv = (a == b ? 1.0 : 0.0) - (dis[a] * av) * dis[b];
    else lv = (a == b ? lam[a] : 0.0) - av;
    A[a * ld + b] = lv;
    V[a * ld + b] = a == b ? 1.0 : 0.0;
  }
  __syncthreads();
  // rotation threshold: relative to the largest entry (uniform: every thread reads the same LDS)
  for (int a = tid; a < m; a += T) {
    double rmax = 0.0;
    for (int b = 0; b < m; ++b) {
      const double v = fabs(A[a * ld + b]);
      if (v > rmax) rmax = v;
      if (!(v <= 1.7976931348623157e308)) bad = 1;  // NaN or inf
    }
    lam[a] = rmax;
  }
  // a Laplacian with a non-finite entry has no eigenvectors (numpy's and torch's eigh refuse it): the group's modes are
  // NaN, as on the composed route, instead of whatever the rotations of the finite entries would leave
  if (__syncthreads_or(bad)) {
    const float qnan = __uint_as_float(0x7fc00000u);
    for (int i = tid; i < m * p.H; i += T) {
      const int a = i / p.H, h = i - a * p.H;
      p.theta[static_cast<int64_t>(mem[a]) * p.H + h] = qnan;
    }
    return;
  }
  double amax = 0.0;
  for (int a = 0; a < m; ++a)
    if (lam[a] > amax) amax = lam[a];
  __syncthreads();
  const double tol = amax * 1e-17;
  const int n = m + (m & 1), half = n >> 1;
  for (int sweep = 0; sweep < EIG_MAX_SWEEPS; ++sweep) {
    int rotated = 0;
    for (int r = 0; r < n - 1; ++r) {
      for (int i = tid; i < half; i += T) {
        int pp, qq;
        eig_pair(n, r, i, pp, qq);
        double c = 1.0, s = 0.0;
        if (qq < m) {
          const double apq = A[pp * ld + qq];
          if (fabs(apq) > tol) {
            const double th = (A[qq * ld + qq] - A[pp * ld + pp]) / (2.0 * apq);
            const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
            c = 1.0 / sqrt(t * t + 1.0);
            s = t * c;
            rotated = 1;
          }
        }
        cs[2 * i] = c;
        cs[2 * i + 1] = s;
      }
      __syncthreads();
      // columns p, q of A and of V
      for (int w = tid; w < half * m; w += T) {
        const int i = w / m, k = w - i * m;
        const double c = cs[2 * i], s = cs[2 * i + 1];
        if (s == 0.0) continue;
        int pp, qq;
        eig_pair(n, r, i, pp, qq);
        const double akp = A[k * ld + pp], akq = A[k * ld + qq];
        A[k * ld + pp] = c * akp - s * akq;
        A[k * ld + qq] = s * akp + c * akq;
        const double vkp = V[k * ld + pp], vkq = V[k * ld + qq];
        V[k * ld + pp] = c * vkp - s * vkq;
        V[k * ld + qq] = s * vkp + c * vkq;
      }
      __syncthreads();
      // rows p, q of A
      for (int w = tid; w < half * m; w += T) {
        const int i = w / m, k = w - i * m;
        const double c = cs[2 * i], s = cs[2 * i + 1];
        if (s == 0.0) continue;
        int pp, qq;
        eig_pair(n, r, i, pp, qq);
        const double apk = A[pp * ld + k], aqk = A[qq * ld + k];
        A[pp * ld + k] = c * apk - s * aqk;
        A[qq * ld + k] = s * apk + c * aqk;
      }
      __syncthreads();
    }
    if (!__syncthreads_or(rotated)) break;
  }
  // ascending eigenvalues, ties to the lower column
  for (int a = tid; a < m; a += T) {
    lam[a] = A[a * ld + a];
    ord[a] = 0;
  }
  __syncthreads();
  int rank_of = -1;
  if (tid < m) {
    const double la = lam[tid];
    int rk = 0;
    for (int b = 0; b < m; ++b) {
      const double lb = lam[b];
      if (lb < la || (lb == la && b < tid)) ++rk;
    }
    rank_of = rk;
  }
  __syncthreads();
  if (tid < m && rank_of >= 0 && rank_of < m) ord[rank_of] = tid;
  __syncthreads();
  for (int i = tid; i < m * p.H; i += T) {
    const int a = i / p.H, h = i - a * p.H;
    const int col = ord[h < m - 1 ? h : m - 1];
    double v = V[a * ld + col];
    if (V[col] < 0.0) v = -v;  // V[0 * ld + col]: the entry of the group's lowest node
    if (p.embed) v *= scl[a];
    p.theta[static_cast<int64_t>(mem[a]) * p.H + h] = static_cast<float>(v);
  }
}

struct PoolArgs {
  const float* theta;        // [N, H]
  const int32_t* theta_ptr;  // [G + 1]
  const int32_t* theta_perm; // [N]
  const float* x;            // [N, F], row stride ldx
  int64_t ldx;
  int N, G, H, F;
  float* out;                // [G, H F]
};

// WAVES waves per (group, 64-feature tile).  Wave w adds rows [w per, (w + 1) per) of the group, per = ceil(len / WAVES),
// in ascending order; wave 0 then folds the partial sums in ascending wave order.  WAVES = 1: the plain ascending sum.
// The host picks WAVES from the longest group alone, so the same input gives the same bits on every call.
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void eig_reduce_kernel(PoolArgs p) {
  __shared__ float part[WAVES][EIG_MODE_CHUNK][64];
  const int g = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.y * 64 + lane;
  const bool live = f < p.F;
  int t0 = p.theta_ptr[g], t1 = p.theta_ptr[g + 1];
  if (t0 < 0) t0 = 0;
  if (t1 > p.N) t1 = p.N;
  const int len = t1 > t0 ? t1 - t0 : 0;
  const int per = (len + WAVES - 1) / WAVES;
  const int a0 = t0 + wave * per;
  const int a1 = a0 + per < t0 + len ? a0 + per : t0 + len;
  float* const o = p.out + static_cast<int64_t>(g) * p.H * p.F + f;
  for (int h0 = 0; h0 < p.H; h0 += EIG_MODE_CHUNK) {
    float acc[EIG_MODE_CHUNK];
#pragma unroll
    for (int hh = 0; hh < EIG_MODE_CHUNK; ++hh) acc[hh] = 0.0f;
    if (live) {
      int a = a0;
      for (; a + 4 <= a1; a += 4) {  // four rows' loads issued together, added in row order
        int node[4];
        float xv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) node[u] = p.theta_perm[a + u];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (node[u] < 0 || node[u] >= p.N) node[u] = -1;  // never dereferenced
          xv[u] = node[u] >= 0 ? p.x[static_cast<int64_t>(node[u]) * p.ldx + f] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (node[u] < 0) continue;
          const float* const th = p.theta + static_cast<int64_t>(node[u]) * p.H + h0;
#pragma unroll
          for (int hh = 0; hh < EIG_MODE_CHUNK; ++hh)
            if (h0 + hh < p.H) acc[hh] += th[hh] * xv[u];
        }
      }
      for (; a < a1; ++a) {
        const int node = p.theta_perm[a];
        if (node < 0 || node >= p.N) continue;  // never dereferenced
        const float xv = p.x[static_cast<int64_t>(node) * p.ldx + f];
        const float* const th = p.theta + static_cast<int64_t>(node) * p.H + h0;
#pragma unroll
        for (int hh = 0; hh < EIG_MODE_CHUNK; ++hh)
          if (h0 + hh < p.H) acc[hh] += th[hh] * xv;
      }
    }
    if (WAVES > 1) {
#pragma unroll
      for (int hh = 0; hh < EIG_MODE_CHUNK; ++hh) part[wave][hh][lane] = acc[hh];
      __syncthreads();
      if (wave == 0) {
#pragma unroll
        for (int hh = 0; hh < EIG_MODE_CHUNK; ++hh) {
          float sum = part[0][hh][lane];
          for (int w = 1; w < WAVES; ++w) sum += part[w][hh][lane];
          acc[hh] = sum;
        }
      }
    }
    if (wave == 0 && live) {
#pragma unroll
      for (int hh = 0; hh < EIG_MODE_CHUNK; ++hh)
        if (h0 + hh < p.H) o[static_cast<int64_t>(h0 + hh) * p.F] = acc[hh];
    }
    if (WAVES > 1) __syncthreads();  // the partial sums are reused by the next chunk of modes
  }
}

struct LiftArgs {
  const float* theta;   // [N, H]
  const int32_t* gid;   // [N]
  const float* xp;      // [G, H F]
  int N, G, H, F;
  float* out;           // [N, F]
};

__global__ __launch_bounds__(256) void eig_lift_kernel(LiftArgs p) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= static_cast<int64_t>(p.N) * p.F) return;
  const int i = static_cast<int>(idx / p.F), f = static_cast<int>(idx - static_cast<int64_t>(i) * p.F);
  const int g = p.gid[i];
  float acc = 0.0f;
  if (g >= 0 && g < p.G) {
    const float* const th = p.theta + static_cast<int64_t>(i) * p.H;
    const float* const xr = p.xp + static_cast<int64_t>(g) * p.H * p.F + f;
    for (int h = 0; h < p.H; ++h) acc += th[h] * xr[static_cast<int64_t>(h) * p.F];
  }
  p.out[idx] = acc;
}

constexpr int64_t I32_MAX = 2147483647;

}  // namespace
}  // namespace tgp

using namespace tgp;

extern "C" int tgp_eigenpool_max_group_nodes(void) { return EIG_MAX_GROUP; }

extern "C" int tgp_eigenpool_modes_f32(const int32_t* grp_ptr, const int32_t* grp_perm, const int64_t* dst,
                                       const float* edge_weight, const int32_t* gid, const int32_t* theta_ptr,
                                       const int32_t* theta_perm, int64_t N, int64_t E, int64_t G, int64_t H,
                                       int64_t max_m, int normalized, int embed, float* theta_modes, float* deg,
                                       int32_t* status, void* stream) {
  TGP_REQUIRE(N >= 0 && E >= 0 && G >= 0, TGP_ERR_INVALID, "tgp_eigenpool_modes_f32: negative size");
  TGP_REQUIRE(H >= 1, TGP_ERR_INVALID, "tgp_eigenpool_modes_f32: H = %lld < 1", static_cast<long long>(H));
  TGP_REQUIRE(max_m >= 1 && max_m <= EIG_MAX_GROUP, TGP_ERR_INVALID,
              "tgp_eigenpool_modes_f32: max_m = %lld outside 1 .. %d", static_cast<long long>(max_m), EIG_MAX_GROUP);
  TGP_REQUIRE(grp_ptr && gid && theta_ptr && theta_perm && theta_modes && status, TGP_ERR_INVALID,
              "tgp_eigenpool_modes_f32: NULL pointer");
  TGP_REQUIRE(E == 0 || dst, TGP_ERR_INVALID, "tgp_eigenpool_modes_f32: NULL dst with E > 0");
  TGP_REQUIRE(N <= I32_MAX && E <= I32_MAX && G <= I32_MAX, TGP_ERR_RANGE,
              "tgp_eigenpool_modes_f32: N, E or G beyond the int32 index");
  if (G == 0 || N == 0) return TGP_OK;
  ModesArgs a{grp_ptr, grp_perm, dst, edge_weight, gid, theta_ptr, theta_perm, static_cast<int>(N),
              static_cast<int>(E), static_cast<int>(G), static_cast<int>(H), static_cast<int>(max_m), normalized,
              embed, theta_modes, deg, status, eig_lds_layout(static_cast<int>(max_m))};
  if (a.l.total > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(eig_modes_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(a.l.total));
  const int threads = max_m <= 8 ? 64 : (max_m <= 24 ? 128 : EIG_THREADS);
  hipLaunchKernelGGL(eig_modes_kernel, dim3(static_cast<unsigned>(G)), dim3(threads), a.l.total,
                     static_cast<hipStream_t>(stream), a);
  return check_launch("tgp_eigenpool_modes_f32");
}

extern "C" int tgp_eigenpool_reduce_f32(const float* theta_modes, const int32_t* theta_ptr, const int32_t* theta_perm,
                                        const float* x, int64_t ldx, int64_t N, int64_t G, int64_t H, int64_t F,
                                        int64_t max_len, float* out, void* stream) {
  TGP_REQUIRE(N >= 0 && G >= 0 && F >= 0 && max_len >= 0, TGP_ERR_INVALID, "tgp_eigenpool_reduce_f32: negative size");
  TGP_REQUIRE(H >= 1, TGP_ERR_INVALID, "tgp_eigenpool_reduce_f32: H = %lld < 1", static_cast<long long>(H));
  TGP_REQUIRE(theta_modes && theta_ptr && theta_perm && x && out, TGP_ERR_INVALID,
              "tgp_eigenpool_reduce_f32: NULL pointer");
  TGP_REQUIRE(ldx >= F, TGP_ERR_INVALID, "tgp_eigenpool_reduce_f32: ldx < F");
  TGP_REQUIRE(x != out, TGP_ERR_INVALID, "tgp_eigenpool_reduce_f32: x given as the output");
  TGP_REQUIRE(N <= I32_MAX && G <= I32_MAX && F <= I32_MAX && H <= I32_MAX && (F + 63) / 64 <= 65535, TGP_ERR_RANGE,
              "tgp_eigenpool_reduce_f32: N, G or F beyond the int32 index");
  if (G == 0 || F == 0) return TGP_OK;
  PoolArgs a{theta_modes, theta_ptr, theta_perm, x, ldx, static_cast<int>(N), static_cast<int>(G),
             static_cast<int>(H), static_cast<int>(F), out};
  const dim3 grid(static_cast<unsigned>(G), static_cast<unsigned>((F + 63) / 64));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (max_len <= EIG_REDUCE_ONE_WAVE) hipLaunchKernelGGL(eig_reduce_kernel<1>, grid, dim3(64), 0, st, a);
  else if (max_len <= EIG_REDUCE_FOUR_WAVES) hipLaunchKernelGGL(eig_reduce_kernel<4>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(eig_reduce_kernel<16>, grid, dim3(1024), 0, st, a);
  return check_launch("tgp_eigenpool_reduce_f32");
}

extern "C" int tgp_eigenpool_lift_f32(const float* theta_modes, const int32_t* gid, const float* x_pool, int64_t N,
                                      int64_t G, int64_t H, int64_t F, float* out, void* stream) {
  TGP_REQUIRE(N >= 0 && G >= 0 && F >= 0, TGP_ERR_INVALID, "tgp_eigenpool_lift_f32: negative size");
  TGP_REQUIRE(H >= 1, TGP_ERR_INVALID, "tgp_eigenpool_lift_f32: H = %lld < 1", static_cast<long long>(H));
  TGP_REQUIRE(theta_modes && gid && x_pool && out, TGP_ERR_INVALID, "tgp_eigenpool_lift_f32: NULL pointer");
  TGP_REQUIRE(x_pool != out, TGP_ERR_INVALID, "tgp_eigenpool_lift_f32: x_pool given as the output");
  TGP_REQUIRE(N <= I32_MAX && G <= I32_MAX && F <= I32_MAX && H <= I32_MAX && (N * F + 255) / 256 <= I32_MAX,
              TGP_ERR_RANGE, "tgp_eigenpool_lift_f32: N, G or F beyond the int32 index");
  if (N == 0 || F == 0) return TGP_OK;
  LiftArgs a{theta_modes, gid, x_pool, static_cast<int>(N), static_cast<int>(G), static_cast<int>(H),
             static_cast<int>(F), out};
  hipLaunchKernelGGL(eig_lift_kernel, dim3(static_cast<unsigned>((N * F + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a);
  return check_launch("tgp_eigenpool_lift_f32");
}
