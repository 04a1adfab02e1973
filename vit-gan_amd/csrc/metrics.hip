// Streaming first and second moments of feature vectors in fp64, for the Frechet distance, gfx950.
//
// vg_moments_update: sum += sum_i x_i and gram += X^T X over an fp32 [n, d] batch, every product and every addition in fp64 on
// v_mfma_f64_16x16x4_f64.  The f64 MFMA's operand maps (one f64 per lane, k = lane >> 4, i|j = lane & 15) make BOTH operands of a Gram
// tile the same kind of load, X[r0 + (lane >> 4)][c0 + (lane & 15)]: 16 consecutive floats of 4 consecutive rows, widened in registers,
// so there is no fp64 copy of the batch and no LDS.  One wave owns a strip of the upper tile triangle: tile row ti and up to
// VG_MOM_NB tile columns from tj0 >= ti on; per k-group of 4 rows it loads one A fragment and VG_MOM_NB B fragments and issues
// VG_MOM_NB MFMAs (the diagonal tile uses one register for both operands).  The strip that starts on the diagonal also carries the
// column sums of its 16 columns as one more accumulator whose B operand is 1.0 (x * 1 is exact, so the sum is a plain fp64 chain).
// The accumulators START from gram / sum and walk the k-groups in order: one owner per output tile, a fixed k order, no atomics - two
// runs are bit-equal, and two updates are the chain of one update over the concatenation.  Tile (ti, tj > ti) is stored twice, as it
// is and transposed; a diagonal tile is symmetric bit for bit by itself (x_ki x_kj commutes exactly, the chain order is k's).
// Rows past n in the last k-group are loaded as exact zeros.
//
// vg_moments_finish: mean = sum / n, cov = (gram - n mean (x) mean) / (n - 1), elementwise fp64 without contraction.
// vg_widen_bf16_f32_launch: the bf16 [B, E] classifier input of the ViT as fp32 (vg_vit_features, engine.hip).
#include "../../include/vitgan_hip.h"
#include "vg_common.h"
#include "vg_kernels.h"

namespace {

#define VG_MOM_NB 4       // tile columns per strip
#define VG_MOM_UNROLL 4   // k-groups in flight per wave: (1 + NB) loads each
#define VG_MOM_DMIN 16
#define VG_MOM_DMAX 2048

typedef double f64x4 __attribute__((ext_vector_type(4)));

// grid (ceil(T / NB), T), one wave per workgroup: block (g, ti) owns tiles (ti, ti + g NB ... ) of the upper triangle
__global__ __launch_bounds__(64) void vg_moments_update_kernel(const float* __restrict__ X, long long ld, int n, int d,
                                                               double* __restrict__ sum, double* __restrict__ gram) {
  const int T = d >> 4, ti = blockIdx.y, tj0 = ti + (int)blockIdx.x * VG_MOM_NB;
  if (tj0 >= T) return;  // below the diagonal: blockIdx-wide
  const int lane = threadIdx.x, lc = lane & 15, lr = lane >> 4;
  const bool diag = blockIdx.x == 0;
  int cj[VG_MOM_NB];  // first column of each B tile; a strip that runs past the edge repeats the last tile and does not store it
#pragma unroll
  for (int b = 0; b < VG_MOM_NB; ++b) cj[b] = (tj0 + b < T ? tj0 + b : T - 1) << 4;
  const int ci = ti << 4;

  f64x4 acc[VG_MOM_NB], accs;
#pragma unroll
  for (int b = 0; b < VG_MOM_NB; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[b][r] = gram[(size_t)(ci + lr + 4 * r) * d + cj[b] + lc];
#pragma unroll
  for (int r = 0; r < 4; ++r) accs[r] = diag ? sum[ci + lr + 4 * r] : 0.0;

  const float* __restrict__ xa = X + ci + lc;
  for (int r0 = 0; r0 < n; r0 += 4 * VG_MOM_UNROLL) {
    float fa[VG_MOM_UNROLL], fb[VG_MOM_UNROLL][VG_MOM_NB];
#pragma unroll
    for (int u = 0; u < VG_MOM_UNROLL; ++u) {
      // a row past n reads row n - 1 (in bounds, no branch around the load) and is replaced by an exact zero
      const int row = r0 + 4 * u + lr;
      const bool in = row < n;
      const size_t off = (size_t)(in ? row : n - 1) * (size_t)ld;
      const float va = xa[off];
      fa[u] = in ? va : 0.f;
#pragma unroll
      for (int b = 0; b < VG_MOM_NB; ++b) {
        const float vb = X[off + cj[b] + lc];
        fb[u][b] = in ? vb : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < VG_MOM_UNROLL; ++u) {
      const double a = (double)fa[u];
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, diag ? a : (double)fb[u][0], acc[0], 0, 0, 0);
#pragma unroll
      for (int b = 1; b < VG_MOM_NB; ++b) acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (double)fb[u][b], acc[b], 0, 0, 0);
      if (diag) accs = __builtin_amdgcn_mfma_f64_16x16x4f64(a, 1.0, accs, 0, 0, 0);
    }
  }

  // C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
  for (int b = 0; b < VG_MOM_NB; ++b) {
    if (tj0 + b >= T) break;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gi = ci + lr + 4 * r, gj = cj[b] + lc;
      gram[(size_t)gi * d + gj] = acc[b][r];
      if (tj0 + b != ti) gram[(size_t)gj * d + gi] = acc[b][r];
    }
  }
  if (diag && lc == 0) {  // every column of the ones-product holds the same sums
#pragma unroll
    for (int r = 0; r < 4; ++r) sum[ci + lr + 4 * r] = accs[r];
  }
}

__global__ __launch_bounds__(256) void vg_moments_finish_kernel(const double* __restrict__ sum, const double* __restrict__ gram, double nn,
                                                                int d, double* __restrict__ mean, double* __restrict__ cov) {
  const long long total = (long long)d * d;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int i = (int)(e / d), j = (int)(e - (long long)i * d);
    const double mi = __ddiv_rn(sum[i], nn), mj = __ddiv_rn(sum[j], nn);
    // gram - n (mean_i mean_j), each step rounded on its own: mean_i mean_j commutes, so cov is symmetric wherever gram is
    cov[e] = __ddiv_rn(__dsub_rn(gram[e], __dmul_rn(nn, __dmul_rn(mi, mj))), nn - 1.0);
    if (i == 0) mean[j] = mj;
  }
}

__global__ __launch_bounds__(256) void vg_widen_bf16_f32_kernel(const bf16* __restrict__ src, float* __restrict__ dst, long long n) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) dst[e] = vg_bf2f(src[e]);
}

}  // namespace

int vg_widen_bf16_f32_launch(const bf16* src, float* dst, long long n, hipStream_t st) {
  long long blocks = (n + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(vg_widen_bf16_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, st, src, dst, n);
  return (int)hipGetLastError();
}

extern "C" int vg_moments_update(const float* feats, long long ld, int n, int d, double* sum, double* gram, void* stream) {
  if (!feats || !sum || !gram || n < 1) return -1;
  if (d < VG_MOM_DMIN || d > VG_MOM_DMAX || (d & 15) || ld < d) return -2;
  const int T = d >> 4;
  hipLaunchKernelGGL(vg_moments_update_kernel, dim3((T + VG_MOM_NB - 1) / VG_MOM_NB, T), dim3(64), 0, (hipStream_t)stream, feats, ld, n, d, sum,
                     gram);
  return (int)hipGetLastError();
}

extern "C" int vg_moments_finish(const double* sum, const double* gram, long long n, int d, double* mean, double* cov, void* stream) {
  if (!sum || !gram || !mean || !cov || n < 2) return -1;
  if (d < VG_MOM_DMIN || d > VG_MOM_DMAX || (d & 15)) return -2;
  long long blocks = ((long long)d * d + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(vg_moments_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, sum, gram, (double)n, d, mean, cov);
  return (int)hipGetLastError();
}
