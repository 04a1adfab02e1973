// Arithmetic on PAIRS of feature vectors in fp64, for precision / recall / density / coverage and KID, gfx950.
//
// One tile loop: a wave owns 16 query rows and a strip of centre tiles (VG_PAIR_NB at a time) and forms dot(q_i, c_j) over d on
// v_mfma_f64_16x16x4_f64.  Operands are fp32 in memory, widened in registers: for a k-step of 16 columns a lane reads the 4
// consecutive floats [k0 + 4 (lane >> 4), + 4) of row (lane & 15) - 64 contiguous bytes per row and k-step - and the t-th of the 4
// MFMAs of the step contracts the columns {k0 + 4 g + t : g = 0..3}.  The SAME walk (same instruction, same k-steps, same t order,
// accumulator from 0.0) gives the row norms, as the diagonal of the product of a 16-row tile with itself (vg_pair_norms_kernel): so
// for bit-equal rows x, x'  n_x = n_x' = dot(x, x') bit for bit and d2 = (n_x + n_x') - 2 dot is exactly 0.0.
//
// Three epilogues on the 16 x 16 tiles, compile-time variants:
//   KNN   d2 clamped at 0; per lane and row a sorted list of the K smallest (registers, K = 1..8), self skipped BY INDEX; at the end
//         the 16 lanes of a row are merged through LDS by one lane per row.
//   BALL  count_i = #{ j : d2 <= rad2_c[j] } (int32) and min_j d2 (fp64), the 16 lanes of a row folded by shuffles (integer adds and
//         minima: any order gives the same bits).
//   SUM   sum (dot / d + 1)^3, optionally without i == j: a per-lane chain in tile order, the wave's 64 lanes folded by lane 0 in
//         lane order, one partial per workgroup; vg_pair_sum_merge_kernel folds the partials in index order.  No atomics.
// There is no n x n buffer.  Column splits (grid.y) fill the chip at small nq; with more than one, the partial lists / counts /
// minima go to the workspace and a second small launch merges them in split order.  The split count is a function of (nq, nc)
// alone, so two runs are bit-equal; everything but SUM is an integer or a selected element of independently computed values and
// is bit-identical under any permutation of the centre rows too.
// Rows past the end of a set are read as the set's last row (in bounds, no branch around a load) and never counted or stored.
#include "../../include/vitgan_hip.h"
#include "vg_common.h"

namespace {

#define VG_PAIR_NB 4          // centre tiles per inner product pass
#define VG_PAIR_DMIN 16
#define VG_PAIR_DMAX 2048
#define VG_PAIR_KMAX 8
#define VG_PAIR_SPLITS 64     // at most this many column splits
#define VG_PAIR_FILL 2048     // waves wanted in flight: 256 CUs x 8

typedef double f64x4 __attribute__((ext_vector_type(4)));

enum { VG_PAIR_KNN = 0, VG_PAIR_BALL = 1, VG_PAIR_SUM = 2 };

struct PairPlan {
  int qtiles, groups, splits, gps;  // query tiles; groups of NB centre tiles; column splits; groups per split
};

PairPlan pair_plan(int nq, int nc) {
  PairPlan p;
  p.qtiles = (nq + 15) / 16;
  p.groups = (nc + 16 * VG_PAIR_NB - 1) / (16 * VG_PAIR_NB);
  int want = (VG_PAIR_FILL + p.qtiles - 1) / p.qtiles;
  if (want > VG_PAIR_SPLITS) want = VG_PAIR_SPLITS;
  if (want > p.groups) want = p.groups;
  if (want < 1) want = 1;
  p.gps = (p.groups + want - 1) / want;
  p.splits = (p.groups + p.gps - 1) / p.gps;  // no empty split
  return p;
}

__device__ __forceinline__ double pair_pick(const f64x4& v, int r) { return r == 0 ? v[0] : r == 1 ? v[1] : r == 2 ? v[2] : v[3]; }

// the K smallest seen so far, ascending; a value equal to the largest kept one changes nothing (the multiset is the same)
template <int K>
__device__ __forceinline__ void pair_insert(double (&list)[K], double v) {
  if (v < list[K - 1]) {
    list[K - 1] = v;
#pragma unroll
    for (int s = K - 1; s > 0; --s) {
      const double lo = fmin(list[s - 1], list[s]), hi = fmax(list[s - 1], list[s]);
      list[s - 1] = lo;
      list[s] = hi;
    }
  }
}

// grid (ceil(n / 16)), one wave: norm[i] = the diagonal of X_tile X_tile^T by the walk of vg_pair_kernel
__global__ __launch_bounds__(64) void vg_pair_norms_kernel(const float* __restrict__ X, long long ld, int n, int d, double* __restrict__ norm) {
  const int lane = threadIdx.x, lc = lane & 15, lr = lane >> 4, r0 = (int)blockIdx.x * 16;
  const int row = r0 + lc < n ? r0 + lc : n - 1;
  const float* __restrict__ xa = X + (size_t)row * (size_t)ld + 4 * lr;
  f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < d; k0 += 16) {
    float f[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) f[t] = xa[k0 + t];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)f[t], (double)f[t], acc, 0, 0, 0);
  }
  // C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg; the diagonal element of column lc sits in lane group lc & 3
  if ((lc & 3) == lr && r0 + lc < n) norm[r0 + lc] = pair_pick(acc, lc >> 2);
}

struct PairOut {
  double* rad2;      // KNN, one split: [nq]
  double* lists;     // KNN, splits > 1: [splits][nq][K]
  int* count;        // BALL: [nq], or [splits][nq]
  double* min_d2;    // BALL: [nq], or [splits][nq]
  double* partial;   // SUM: [splits][qtiles]
};

// grid (qtiles, splits), one wave per workgroup
template <int MODE, int K>
__global__ __launch_bounds__(64) void vg_pair_kernel(const float* __restrict__ Q, long long ldq, int nq, const float* __restrict__ Cn,
                                                     long long ldc, int nc, int d, const double* __restrict__ normq,
                                                     const double* __restrict__ normc, const double* __restrict__ rad2c, int skip_self,
                                                     int gps, int groups, PairOut out) {
  __shared__ double sh[MODE == VG_PAIR_KNN ? 64 * 4 * K : 64];
  const int lane = threadIdx.x, lc = lane & 15, lr = lane >> 4, q0 = (int)blockIdx.x * 16;
  const int qrow = q0 + lc < nq ? q0 + lc : nq - 1;
  const float* __restrict__ qa = Q + (size_t)qrow * (size_t)ldq + 4 * lr;
  const int g_lo = (int)blockIdx.y * gps, g_hi = g_lo + gps < groups ? g_lo + gps : groups;
  const double dd = (double)d;

  double nqv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) nqv[r] = MODE == VG_PAIR_SUM ? 0.0 : normq[q0 + lr + 4 * r < nq ? q0 + lr + 4 * r : nq - 1];

  double list[4][K];
  int cnt[4] = {0, 0, 0, 0};
  double mn[4], total = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    mn[r] = __builtin_inf();
#pragma unroll
    for (int s = 0; s < K; ++s) list[r][s] = __builtin_inf();
  }

  for (int g = g_lo; g < g_hi; ++g) {
    const int c0 = g * 16 * VG_PAIR_NB;
    const float* __restrict__ cb[VG_PAIR_NB];
#pragma unroll
    for (int b = 0; b < VG_PAIR_NB; ++b) {
      const int j = c0 + 16 * b + lc;
      cb[b] = Cn + (size_t)(j < nc ? j : nc - 1) * (size_t)ldc + 4 * lr;
    }
    f64x4 acc[VG_PAIR_NB];
#pragma unroll
    for (int b = 0; b < VG_PAIR_NB; ++b) acc[b] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
    for (int k0 = 0; k0 < d; k0 += 16) {
      float fa[4], fb[VG_PAIR_NB][4];
#pragma unroll
      for (int t = 0; t < 4; ++t) fa[t] = qa[k0 + t];
#pragma unroll
      for (int b = 0; b < VG_PAIR_NB; ++b)
#pragma unroll
        for (int t = 0; t < 4; ++t) fb[b][t] = cb[b][k0 + t];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const double a = (double)fa[t];
#pragma unroll
        for (int b = 0; b < VG_PAIR_NB; ++b) acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (double)fb[b][t], acc[b], 0, 0, 0);
      }
    }
    // C/D of the f64 MFMA: col = lane & 15 (centre), row = (lane >> 4) + 4 reg (query)
#pragma unroll
    for (int b = 0; b < VG_PAIR_NB; ++b) {
      const int j = c0 + 16 * b + lc;
      const bool jin = j < nc;
      double ncj = 0.0, rj = 0.0;
      if (MODE != VG_PAIR_SUM) ncj = normc[jin ? j : nc - 1];
      if (MODE == VG_PAIR_BALL) rj = rad2c[jin ? j : nc - 1];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = q0 + lr + 4 * r;
        const bool ok = jin && i < nq && !(skip_self && i == j);
        const double dot = acc[b][r];
        if (MODE == VG_PAIR_SUM) {
          const double t = __dadd_rn(__ddiv_rn(dot, dd), 1.0);
          if (ok) total = __dadd_rn(total, __dmul_rn(__dmul_rn(t, t), t));
        } else {
          const double d2 = fmax(__dsub_rn(__dadd_rn(nqv[r], ncj), __dmul_rn(2.0, dot)), 0.0);
          if (MODE == VG_PAIR_KNN) {
            if (ok) pair_insert<K>(list[r], d2);
          } else {
            cnt[r] += (ok && d2 <= rj) ? 1 : 0;
            mn[r] = ok ? fmin(mn[r], d2) : mn[r];
          }
        }
      }
    }
  }

  const bool direct = gridDim.y == 1;
  if (MODE == VG_PAIR_KNN) {
    // sh[row][lc][K]; then lane = row (0..15) folds the 16 lists of its row
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int s = 0; s < K; ++s) sh[((lr + 4 * r) * 16 + lc) * K + s] = list[r][s];
    __syncthreads();
    if (lane < 16 && q0 + lane < nq) {
      double best[K];
#pragma unroll
      for (int s = 0; s < K; ++s) best[s] = __builtin_inf();
      for (int e = 0; e < 16 * K; ++e) pair_insert<K>(best, sh[lane * 16 * K + e]);
      if (direct) {
        out.rad2[q0 + lane] = best[K - 1];
      } else {
        double* __restrict__ dst = out.lists + ((size_t)blockIdx.y * (size_t)nq + (size_t)(q0 + lane)) * K;
#pragma unroll
        for (int s = 0; s < K; ++s) dst[s] = best[s];
      }
    }
  } else if (MODE == VG_PAIR_BALL) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        cnt[r] += __shfl_xor(cnt[r], o, 16);
        mn[r] = fmin(mn[r], __shfl_xor(mn[r], o, 16));
      }
    if (lc == 0) {
      const size_t base = direct ? 0 : (size_t)blockIdx.y * (size_t)nq;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = q0 + lr + 4 * r;
        if (i < nq) {
          out.count[base + i] = cnt[r];
          out.min_d2[base + i] = mn[r];
        }
      }
    }
  } else {
    sh[lane] = total;
    __syncthreads();
    if (lane == 0) {
      double s = 0.0;
      for (int e = 0; e < 64; ++e) s = __dadd_rn(s, sh[e]);
      out.partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
  }
}

// one thread per query: the K smallest of the splits' lists, in split order
template <int K>
__global__ __launch_bounds__(256) void vg_pair_knn_merge_kernel(const double* __restrict__ lists, int nq, int splits, double* __restrict__ rad2) {
  const int i = (int)blockIdx.x * 256 + threadIdx.x;
  if (i >= nq) return;
  double best[K];
#pragma unroll
  for (int s = 0; s < K; ++s) best[s] = __builtin_inf();
  for (int p = 0; p < splits; ++p) {
    const double* __restrict__ src = lists + ((size_t)p * (size_t)nq + (size_t)i) * K;
#pragma unroll
    for (int s = 0; s < K; ++s) pair_insert<K>(best, src[s]);
  }
  rad2[i] = best[K - 1];
}

__global__ __launch_bounds__(256) void vg_pair_ball_merge_kernel(const int* __restrict__ pc, const double* __restrict__ pm, int nq, int splits,
                                                                 int* __restrict__ count, double* __restrict__ min_d2) {
  const int i = (int)blockIdx.x * 256 + threadIdx.x;
  if (i >= nq) return;
  int c = 0;
  double m = __builtin_inf();
  for (int p = 0; p < splits; ++p) {
    c += pc[(size_t)p * (size_t)nq + i];
    m = fmin(m, pm[(size_t)p * (size_t)nq + i]);
  }
  count[i] = c;
  min_d2[i] = m;
}

// one owner folds every workgroup's partial in index order
__global__ __launch_bounds__(64) void vg_pair_sum_merge_kernel(const double* __restrict__ partial, long long count, double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = 0.0;
  for (long long e = 0; e < count; ++e) s = __dadd_rn(s, partial[e]);
  out[0] = s;
}

// workspace: normq [nq] | normc [nc] | the partials of the widest mode, all in doubles
inline long long pair_norm_doubles(int nq, int nc) { return (long long)nq + (long long)nc; }

long long pair_ws_doubles(int nq, int nc, int k) {
  const PairPlan p = pair_plan(nq, nc);
  const long long per = k > 2 ? k : 2;  // BALL keeps a count and a minimum per query and split; SUM one double per workgroup
  long long part = (long long)p.splits * (long long)nq * per;
  const long long sums = (long long)p.splits * (long long)p.qtiles;
  if (sums > part) part = sums;
  return pair_norm_doubles(nq, nc) + part;
}

int pair_check(const float* Q, long long ldq, int nq, const float* Cn, long long ldc, int nc, int d) {
  if (!Q || !Cn || nq < 1 || nc < 1) return -1;
  if (d < VG_PAIR_DMIN || d > VG_PAIR_DMAX || (d & 15) || ldq < d || ldc < d) return -2;
  return 0;
}

void pair_norms(const float* X, long long ld, int n, int d, double* norm, hipStream_t st) {
  hipLaunchKernelGGL(vg_pair_norms_kernel, dim3((n + 15) / 16), dim3(64), 0, st, X, ld, n, d, norm);
}

template <int K>
void pair_knn_launch(const float* X, long long ld, int n, int d, double* rad2, double* ws, hipStream_t st) {
  const PairPlan p = pair_plan(n, n);
  double* norm = ws;
  PairOut out = {rad2, ws + pair_norm_doubles(n, n), nullptr, nullptr, nullptr};
  pair_norms(X, ld, n, d, norm, st);
  hipLaunchKernelGGL((vg_pair_kernel<VG_PAIR_KNN, K>), dim3(p.qtiles, p.splits), dim3(64), 0, st, X, ld, n, X, ld, n, d, norm, norm, nullptr, 1,
                     p.gps, p.groups, out);
  if (p.splits > 1)
    hipLaunchKernelGGL(vg_pair_knn_merge_kernel<K>, dim3((n + 255) / 256), dim3(256), 0, st, out.lists, n, p.splits, rad2);
}

}  // namespace

extern "C" long long vg_pair_ws_bytes(int nq, int nc, int k) {
  if (nq < 1 || nc < 1 || k < 0 || k > VG_PAIR_KMAX) return -1;
  return pair_ws_doubles(nq, nc, k) * (long long)sizeof(double);
}

extern "C" int vg_knn_radii(const float* X, long long ld, int n, int d, int k, double* rad2, void* ws, void* stream) {
  if (!rad2 || !ws) return -1;
  if (int rc = pair_check(X, ld, n, X, ld, n, d)) return rc;
  if (k < 1 || k > VG_PAIR_KMAX || k >= n) return -3;
  hipStream_t st = (hipStream_t)stream;
  double* w = (double*)ws;
  switch (k) {
    case 1: pair_knn_launch<1>(X, ld, n, d, rad2, w, st); break;
    case 2: pair_knn_launch<2>(X, ld, n, d, rad2, w, st); break;
    case 3: pair_knn_launch<3>(X, ld, n, d, rad2, w, st); break;
    case 4: pair_knn_launch<4>(X, ld, n, d, rad2, w, st); break;
    case 5: pair_knn_launch<5>(X, ld, n, d, rad2, w, st); break;
    case 6: pair_knn_launch<6>(X, ld, n, d, rad2, w, st); break;
    case 7: pair_knn_launch<7>(X, ld, n, d, rad2, w, st); break;
    default: pair_knn_launch<8>(X, ld, n, d, rad2, w, st); break;
  }
  return (int)hipGetLastError();
}

extern "C" int vg_ball_counts(const float* Q, long long ldq, int nq, const float* Cn, long long ldc, int nc, int d, const double* rad2_c,
                              int* count, double* min_d2, void* ws, void* stream) {
  if (!rad2_c || !count || !min_d2 || !ws) return -1;
  if (int rc = pair_check(Q, ldq, nq, Cn, ldc, nc, d)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const PairPlan p = pair_plan(nq, nc);
  double* normq = (double*)ws;
  double* normc = normq + nq;
  double* pm = normq + pair_norm_doubles(nq, nc);   // [splits][nq] minima, then [splits][nq] counts
  int* pc = (int*)(pm + (size_t)p.splits * (size_t)nq);
  pair_norms(Q, ldq, nq, d, normq, st);
  pair_norms(Cn, ldc, nc, d, normc, st);
  PairOut out = {nullptr, nullptr, p.splits > 1 ? pc : count, p.splits > 1 ? pm : min_d2, nullptr};
  hipLaunchKernelGGL((vg_pair_kernel<VG_PAIR_BALL, 1>), dim3(p.qtiles, p.splits), dim3(64), 0, st, Q, ldq, nq, Cn, ldc, nc, d, normq, normc,
                     rad2_c, 0, p.gps, p.groups, out);
  if (p.splits > 1)
    hipLaunchKernelGGL(vg_pair_ball_merge_kernel, dim3((nq + 255) / 256), dim3(256), 0, st, pc, pm, nq, p.splits, count, min_d2);
  return (int)hipGetLastError();
}

extern "C" int vg_poly_kernel_sum(const float* Q, long long ldq, int nq, const float* Cn, long long ldc, int nc, int d, int skip_diagonal,
                                  double* out_sum, void* ws, void* stream) {
  if (!out_sum || !ws) return -1;
  if (int rc = pair_check(Q, ldq, nq, Cn, ldc, nc, d)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const PairPlan p = pair_plan(nq, nc);
  double* partial = (double*)ws + pair_norm_doubles(nq, nc);
  PairOut out = {nullptr, nullptr, nullptr, nullptr, partial};
  hipLaunchKernelGGL((vg_pair_kernel<VG_PAIR_SUM, 1>), dim3(p.qtiles, p.splits), dim3(64), 0, st, Q, ldq, nq, Cn, ldc, nc, d, nullptr, nullptr,
                     nullptr, skip_diagonal ? 1 : 0, p.gps, p.groups, out);
  hipLaunchKernelGGL(vg_pair_sum_merge_kernel, dim3(1), dim3(64), 0, st, partial, (long long)p.splits * p.qtiles, out_sum);
  return (int)hipGetLastError();
}
