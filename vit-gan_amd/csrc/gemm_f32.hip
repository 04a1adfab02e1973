// fp32 mode: the GEMM family on the exact f32-input MFMA (v_mfma_f32_16x16x4_f32: bit-for-bit a k-ordered fmaf chain, no xf32
// shortcut on gfx950), deterministic column sums, and the small elementwise kernels of the fp32 network.
//
// GEMM tile: 64 x 64 x 16 per 256-thread workgroup, staged global -> registers -> LDS (the next tile's loads are in flight while
// the current one is multiplied); each wave owns a 32 x 32 quadrant = 2 x 2 tiles of 16 x 16, each summed in 4 k chains (16
// independent accumulators per wave: the 16x16x4 form issues every 32 cycles with a 40-cycle dependent latency).  The LDS tiles are k-major with a row
// stride of 80 floats, so the four k rows one 16x16x4 step reads land in four distinct groups of 16 banks.
#include "vg_f32.h"
#include "vg_kernels.h"

#define F_BM 64
#define F_BN 64
#define F_BK 16
#define F_LD (F_BM + 16)

__device__ __forceinline__ float f32_gelu(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float f32_gelu_grad(float x) {
  return 0.5f * (1.0f + erff(x * 0.70710678118654752f)) + x * 0.39894228040143268f * expf(-0.5f * x * x);
}

// SIREN: the instantiation of the two sine epilogues (act 5, 6); the other codes run the <false> instantiation, which holds no sinf / cosf
template <bool SIREN>
__global__ __launch_bounds__(256) void vg_f32_gemm_kernel(const VgF32Gemm g) {
  __shared__ float As[F_BK][F_LD];
  __shared__ float Bs[F_BK][F_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.y * F_BM, n0 = blockIdx.x * F_BN, z = blockIdx.z;
  const int kbeg = z * g.kchunk, kend = min(g.K, kbeg + g.kchunk);
  // staging: 1024 elements per operand tile, 4 per thread, the operand's contiguous dimension across the lanes
  const bool a_kfast = g.sak == 1, b_nfast = g.sbn == 1;
  float ra[4], rb[4];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = tid + 256 * i;
      const int am = a_kfast ? (t >> 4) : (t & 63), ak = a_kfast ? (t & 15) : (t >> 6);
      const int gm = m0 + am, gk = k0 + ak;
      ra[i] = (gm < g.M && gk < kend) ? g.A[(long long)gm * g.sam + (long long)gk * g.sak] : 0.f;
      const int bn = b_nfast ? (t & 63) : (t >> 4), bk = b_nfast ? (t >> 6) : (t & 15);
      const int gn = n0 + bn, gkb = k0 + bk;
      rb[i] = (gn < g.N && gkb < kend) ? g.B[(long long)gkb * g.sbk + (long long)gn * g.sbn] : 0.f;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = tid + 256 * i;
      const int am = a_kfast ? (t >> 4) : (t & 63), ak = a_kfast ? (t & 15) : (t >> 6);
      As[ak][am] = ra[i];
      const int bn = b_nfast ? (t & 63) : (t >> 4), bk = b_nfast ? (t >> 6) : (t & 15);
      Bs[bk][bn] = rb[i];
    }
  };
  // four k chains per output (k-step kk of every k-tile feeds chain kk / 4), added pairwise at the end: a quarter of the chain
  // length halves the rounding error of the sum, and 16 independent accumulators per wave keep the MFMA pipe full
  f32x4 c00[4], c01[4], c10[4], c11[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) c00[q] = c01[q] = c10[q] = c11[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, li = lane & 15, lk = lane >> 4;
  if (kbeg < kend) load(kbeg);
  for (int k0 = kbeg; k0 < kend; k0 += F_BK) {
    __syncthreads();
    store();
    __syncthreads();
    if (k0 + F_BK < kend) load(k0 + F_BK);
#pragma unroll
    for (int kk = 0; kk < F_BK; kk += 4) {
      // 16x16x4 operand maps: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15]
      const float a0 = As[kk + lk][wm + li], a1 = As[kk + lk][wm + 16 + li];
      const float b0 = Bs[kk + lk][wn + li], b1 = Bs[kk + lk][wn + 16 + li];
      const int q = kk >> 2;
      c00[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, c00[q], 0, 0, 0);
      c01[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, c01[q], 0, 0, 0);
      c10[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, c10[q], 0, 0, 0);
      c11[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, c11[q], 0, 0, 0);
    }
  }
  const unsigned dkey = g.drop.thr ? vg_drop_key(g.drop.key, g.drop.step) : 0u;
  auto emit = [&](const f32x4& acc, int ti, int tj) {
    const int n = n0 + wn + 16 * tj + li;  // C/D map: col = lane & 15, row = 4 * (lane >> 4) + reg
    if (n >= g.N) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wm + 16 * ti + 4 * lk + r;
      if (m >= g.M) continue;
      float v = acc[r];
      if (g.c_split) {  // split-K slab: the raw partial product
        g.C[(long long)z * g.c_split + (long long)m * g.ldc + n] = v;
        continue;
      }
      if (g.bias) v += g.bias[n];
      if constexpr (SIREN) {  // the product omega0 * z is rounded to fp32 once, then the accurate sine / cosine of it
        if (g.act == VG_F32_ACT_SIN) {
          g.Z[(long long)m * g.ldz + n] = v;
          v = sinf(g.omega0 * v);
        } else {
          v *= g.omega0 * cosf(g.omega0 * g.aux[(long long)m * g.ldaux + n]);
        }
        g.C[(long long)m * g.ldc + n] = v;
        continue;
      }
      if (g.act == VG_F32_ACT_GELU) {
        if (g.Z) g.Z[(long long)m * g.ldz + n] = v;
        v = f32_gelu(v);
      } else if (g.act == VG_F32_ACT_TANH) {
        v = tanhf(v);
      } else if (g.act == VG_F32_MUL_GELU) {
        v *= f32_gelu_grad(g.aux[(long long)m * g.ldaux + n]);
      } else if (g.act == VG_F32_MUL_TANH) {
        const float t = g.aux[(long long)m * g.ldaux + n];
        v *= 1.0f - t * t;
      }
      if (g.drop.thr) {  // the element index of the row-major [M, N] output, as vg_dropout_apply counts it
        const unsigned idx = (unsigned)m * (unsigned)g.N + (unsigned)n;
        v *= vg_drop_factor(vg_drop_word(dkey, idx >> 2), idx & 3, g.drop.thr, g.drop.scale);
      }
      if (g.res) v += g.res[(long long)m * g.ldr + n];
      g.C[(long long)m * g.ldc + n] = v;
    }
  };
  emit((c00[0] + c00[1]) + (c00[2] + c00[3]), 0, 0); emit((c01[0] + c01[1]) + (c01[2] + c01[3]), 0, 1);
  emit((c10[0] + c10[1]) + (c10[2] + c10[3]), 1, 0); emit((c11[0] + c11[1]) + (c11[2] + c11[3]), 1, 1);
}

int vg_f32_gemm_launch(const VgF32Gemm& g, hipStream_t st) {
  if (!g.A || !g.B || !g.C) return -1;
  if (g.M < 1 || g.N < 1 || g.K < 1) return -2;
  if ((g.sak != 1 && g.sam != 1) || (g.sbn != 1 && g.sbk != 1)) return -3;
  if (g.splits < 1 || g.kchunk < 1 || (long long)g.splits * g.kchunk < g.K) return -3;
  if (g.splits > 1 && (!g.c_split || (g.kchunk % F_BK))) return -3;
  if ((g.act == VG_F32_MUL_GELU || g.act == VG_F32_MUL_TANH || g.act == VG_F32_MUL_COS) && !g.aux) return -1;
  const bool siren = g.act == VG_F32_ACT_SIN || g.act == VG_F32_MUL_COS;
  if (siren && (g.c_split || g.drop.thr || g.res || (g.act == VG_F32_ACT_SIN && !g.Z))) return -3;
  dim3 grid((g.N + F_BN - 1) / F_BN, (g.M + F_BM - 1) / F_BM, g.splits);
  if (siren) hipLaunchKernelGGL(vg_f32_gemm_kernel<true>, grid, dim3(256), 0, st, g);
  else hipLaunchKernelGGL(vg_f32_gemm_kernel<false>, grid, dim3(256), 0, st, g);
  return (int)hipGetLastError();
}

static VgF32Gemm f32_prob() {
  VgF32Gemm g = {};
  g.splits = 1;
  return g;
}

int vg_f32_linear_fwd(const float* X, const float* W, const float* bias, const float* res, float* Y, float* Z, int M, int N, int K, int act,
                      VgDrop drop, hipStream_t st) {
  if (act < VG_F32_ACT_NONE || act > VG_F32_ACT_TANH) return -4;
  VgF32Gemm g = f32_prob();
  g.A = X; g.sam = K; g.sak = 1;   // A(m, k) = X[m][k]
  g.B = W; g.sbk = 1; g.sbn = K;   // B(k, n) = W[n][k]
  g.M = M; g.N = N; g.K = K; g.kchunk = K;
  g.C = Y; g.ldc = N; g.bias = bias; g.act = act; g.Z = Z; g.ldz = N; g.res = res; g.ldr = N;
  g.drop = drop;
  return vg_f32_gemm_launch(g, st);
}

int vg_f32_linear_dgrad(const float* dY, const float* W, const float* aux, float* dX, int M, int N, int K, int act, hipStream_t st) {
  if (act != VG_F32_ACT_NONE && act != VG_F32_MUL_GELU && act != VG_F32_MUL_TANH) return -4;
  VgF32Gemm g = f32_prob();
  g.A = dY; g.sam = N; g.sak = 1;  // A(m, n) = dY[m][n]
  g.B = W; g.sbk = K; g.sbn = 1;   // B(n, k) = W[n][k]
  g.M = M; g.N = K; g.K = N; g.kchunk = N;
  g.C = dX; g.ldc = K; g.act = act; g.aux = aux; g.ldaux = K;
  return vg_f32_gemm_launch(g, st);
}

int vg_f32_siren_fwd(const float* X, const float* W, const float* bias, float* Y, float* Z, int M, int N, int K, float omega0, hipStream_t st) {
  if (!Z) return -1;
  VgF32Gemm g = f32_prob();
  g.A = X; g.sam = K; g.sak = 1;
  g.B = W; g.sbk = 1; g.sbn = K;
  g.M = M; g.N = N; g.K = K; g.kchunk = K;
  g.C = Y; g.ldc = N; g.bias = bias; g.act = VG_F32_ACT_SIN; g.Z = Z; g.ldz = N; g.omega0 = omega0;
  return vg_f32_gemm_launch(g, st);
}
int vg_f32_siren_dgrad(const float* dY, const float* W, const float* aux, float* dX, int M, int N, int K, float omega0, hipStream_t st) {
  VgF32Gemm g = f32_prob();
  g.A = dY; g.sam = N; g.sak = 1;
  g.B = W; g.sbk = K; g.sbn = 1;
  g.M = M; g.N = K; g.K = N; g.kchunk = N;
  g.C = dX; g.ldc = K; g.act = VG_F32_MUL_COS; g.aux = aux; g.ldaux = K; g.omega0 = omega0;
  return vg_f32_gemm_launch(g, st);
}

// split-K of the weight gradient: every slice a chain of at most 512 rows (the f32 MFMA's error grows with the chain length),
// at most 64 slices
static int wgrad_kchunk(int M) {
  int s = (M + 511) / 512;
  if (s > 64) s = 64;
  const int chunk = (M + s - 1) / s;
  return (chunk + F_BK - 1) / F_BK * F_BK;
}
static int wgrad_splits(int M) { const int c = wgrad_kchunk(M); return (M + c - 1) / c; }
long long vg_f32_wgrad_slab_floats(int M, int N, int K) {
  if (M < 1 || N < 1 || K < 1) return -2;
  const long long w = (long long)wgrad_splits(M) * N * K, b = (long long)vg_f32_colsum_parts(M) * N;  // weight slices; bias parts
  return w > b ? w : b;
}

// dst[i] += (slab[0][i] + slab[1][i] + ...), the slices added in slice order
__global__ __launch_bounds__(256) void vg_f32_fold_kernel(const float* __restrict__ slab, long long stride, int nslab,
                                                          float* __restrict__ dst, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float a = slab[i];
  for (int s = 1; s < nslab; ++s) a += slab[(long long)s * stride + i];
  dst[i] += a;
}

int vg_f32_linear_wgrad(const float* dY, const float* X, float* dW, float* db, float* slab, int M, int N, int K, hipStream_t st) {
  if (!dY || !X || !dW || !slab) return -1;
  if (M < 1 || N < 1 || K < 1) return -2;
  VgF32Gemm g = f32_prob();
  g.A = dY; g.sam = 1; g.sak = N;  // A(n, m) = dY[m][n]
  g.B = X; g.sbk = K; g.sbn = 1;   // B(m, k) = X[m][k]
  g.M = N; g.N = K; g.K = M;
  g.kchunk = wgrad_kchunk(M); g.splits = wgrad_splits(M);
  g.C = slab; g.ldc = K; g.c_split = (long long)N * K;
  VG_TRY(vg_f32_gemm_launch(g, st));
  const long long n = (long long)N * K;
  hipLaunchKernelGGL(vg_f32_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)slab, n, g.splits, dW, n);
  VG_CHECK_HIP(hipGetLastError());
  if (!db) return 0;
  // bias: column sums of dY, in the slab behind the weight slices' use (the fold above has read them by then: same stream)
  return vg_f32_colsum_launch(dY, N, M, slab, db, N, nullptr, 0, st);
}

// ---------------------------------------------------------------------------------------------------------------------
// column sums: part[chunk][c] = sum of X[r][c] over the chunk's 256 rows in fp64; then dst += the chunks summed in order
#define CS_F32_ROWS 256
int vg_f32_colsum_parts(int R) { return (R + CS_F32_ROWS - 1) / CS_F32_ROWS; }
__global__ __launch_bounds__(256) void vg_f32_colsum_part_kernel(const float* __restrict__ X, long long ld, int R, int N,
                                                                 float* __restrict__ part) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  const int r0 = blockIdx.y * CS_F32_ROWS, r1 = min(R, r0 + CS_F32_ROWS);
  double a = 0.0;
  for (int r = r0; r < r1; ++r) a += (double)X[(long long)r * ld + c];
  part[(long long)blockIdx.y * N + c] = (float)a;
}
__global__ __launch_bounds__(256) void vg_f32_colsum_fold_kernel(const float* __restrict__ part, int nparts, int N, float* __restrict__ d0,
                                                                 int n0, float* __restrict__ d1) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  double a = 0.0;
  for (int p = 0; p < nparts; ++p) a += (double)part[(long long)p * N + c];
  if (c < n0) d0[c] += (float)a;
  else d1[c - n0] += (float)a;
}
static int colsum_fold(const float* part, int nparts, float* d0, int n0, float* d1, int n1, hipStream_t st) {
  const int N = n0 + n1;
  hipLaunchKernelGGL(vg_f32_colsum_fold_kernel, dim3((N + 255) / 256), dim3(256), 0, st, part, nparts, N, d0, n0, d1);
  return (int)hipGetLastError();
}
int vg_f32_colsum_launch(const float* X, long long ld, int R, float* part, float* d0, int n0, float* d1, int n1, hipStream_t st) {
  if (!X || !part || !d0 || (n1 > 0 && !d1)) return -1;
  if (R < 1 || n0 < 1 || n1 < 0) return -2;
  const int N = n0 + n1, np = vg_f32_colsum_parts(R);
  hipLaunchKernelGGL(vg_f32_colsum_part_kernel, dim3((N + 255) / 256, np), dim3(256), 0, st, X, ld, R, N, part);
  VG_CHECK_HIP(hipGetLastError());
  return colsum_fold(part, np, d0, n0, d1, n1, st);
}

// LayerNorm affine gradients: part[chunk][c] = sum dy * xhat, part[chunk][E + c] = sum dy (fp64 per chunk)
__global__ __launch_bounds__(256) void vg_f32_ln_param_part_kernel(const float* __restrict__ dy, const float* __restrict__ x, long long xs,
                                                                   const float* __restrict__ mean, const float* __restrict__ rstd, int R, int E,
                                                                   float* __restrict__ part) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= E) return;
  const int r0 = blockIdx.y * CS_F32_ROWS, r1 = min(R, r0 + CS_F32_ROWS);
  double ag = 0.0, ab = 0.0;
  for (int r = r0; r < r1; ++r) {
    const float g = dy[(long long)r * E + c];
    const float xh = (x[(long long)r * xs + c] - mean[r]) * rstd[r];
    ag += (double)(g * xh);
    ab += (double)g;
  }
  part[(long long)blockIdx.y * 2 * E + c] = (float)ag;
  part[(long long)blockIdx.y * 2 * E + E + c] = (float)ab;
}
int vg_f32_ln_param_grads(const float* dy, const float* x, long long xs, const float* mean, const float* rstd, float* dgamma, float* dbeta,
                          float* part, int R, int E, hipStream_t st) {
  const int np = vg_f32_colsum_parts(R);
  hipLaunchKernelGGL(vg_f32_ln_param_part_kernel, dim3((E + 255) / 256, np), dim3(256), 0, st, dy, x, xs, mean, rstd, R, E, part);
  VG_CHECK_HIP(hipGetLastError());
  return colsum_fold(part, np, dgamma, E, dbeta, E, st);
}

// ---------------------------------------------------------------------------------------------------------------------
// elementwise
static inline unsigned nblk_f32(long long n) { return (unsigned)((n + 255) / 256); }

__global__ __launch_bounds__(256) void vg_f32_dropout_kernel(const float* __restrict__ x, float* __restrict__ y, long long n, VgDrop drop) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned dkey = vg_drop_key(drop.key, drop.step), idx = (unsigned)i;
  y[i] = x[i] * vg_drop_factor(vg_drop_word(dkey, idx >> 2), idx & 3, drop.thr, drop.scale);
}
int vg_f32_dropout_launch(const float* x, float* y, long long n, VgDrop drop, hipStream_t st) {
  if (!x || !y) return -1;
  if (n < 1) return -2;
  hipLaunchKernelGGL(vg_f32_dropout_kernel, dim3(nblk_f32(n)), dim3(256), 0, st, x, y, n, drop);
  return (int)hipGetLastError();
}

__global__ __launch_bounds__(256) void vg_f32_patchify_kernel(const float* __restrict__ img, float* __restrict__ tiles, int B, int Cc, int IH,
                                                              int P, int backward) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n = (long long)B * Cc * IH * IH;
  if (i >= n) return;
  const int x = (int)(i % IH), y = (int)((i / IH) % IH), c = (int)((i / ((long long)IH * IH)) % Cc);
  const long long b = i / ((long long)Cc * IH * IH);
  const int gw = IH / P, p = (y / P) * gw + x / P;
  const long long t = (b * gw * gw + p) * ((long long)Cc * P * P) + (long long)c * P * P + (y % P) * P + (x % P);
  if (backward) ((float*)img)[i] = tiles[t];
  else tiles[t] = img[i];
}
int vg_f32_patchify_launch(const float* img, float* tiles, int B, int C, int IH, int P, int backward, hipStream_t st) {
  if (!img || !tiles) return -1;
  if (B < 1 || C < 1 || P < 1 || IH % P) return -3;
  const long long n = (long long)B * C * IH * IH;
  hipLaunchKernelGGL(vg_f32_patchify_kernel, dim3(nblk_f32(n)), dim3(256), 0, st, img, tiles, B, C, IH, P, backward);
  return (int)hipGetLastError();
}

__global__ __launch_bounds__(256) void vg_f32_embed_assemble_kernel(const float* __restrict__ tok, const float* __restrict__ pos,
                                                                    const float* __restrict__ cls, float* __restrict__ X, int B, int S, int E,
                                                                    unsigned dthr, unsigned dkey0, float dscale, const unsigned* __restrict__ dstep) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * S * E) return;
  const int e = (int)(i % E);
  const long long row = i / E;
  const int s = (int)(row % S);
  const long long b = row / S;
  const int NP = S - 1;
  float v = s == 0 ? cls[e] : tok[(b * NP + s - 1) * E + e] + pos[(long long)(s - 1) * E + e];
  if (dthr) {
    const unsigned idx = (unsigned)i;
    v *= vg_drop_factor(vg_drop_word(vg_drop_key(dkey0, dstep), idx >> 2), idx & 3, dthr, dscale);
  }
  X[i] = v;
}
int vg_f32_embed_assemble_launch(const float* tok, const float* pos, const float* cls, float* X, int B, int S, int E, VgDrop drop,
                                 hipStream_t st) {
  const long long n = (long long)B * S * E;
  hipLaunchKernelGGL(vg_f32_embed_assemble_kernel, dim3(nblk_f32(n)), dim3(256), 0, st, tok, pos, cls, X, B, S, E, drop.thr, drop.key, drop.scale, drop.step);
  return (int)hipGetLastError();
}

__global__ __launch_bounds__(256) void vg_f32_embed_grad_kernel(const float* __restrict__ g, float* __restrict__ gm, float* __restrict__ gt,
                                                                int B, int S, int E, VgDrop drop) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * S * E) return;
  float v = g[i];
  if (drop.thr) {
    const unsigned idx = (unsigned)i;
    v *= vg_drop_factor(vg_drop_word(vg_drop_key(drop.key, drop.step), idx >> 2), idx & 3, drop.thr, drop.scale);
  }
  gm[i] = v;
  const int e = (int)(i % E);
  const long long row = i / E;
  const int s = (int)(row % S);
  const long long b = row / S;
  if (s > 0) gt[(b * (S - 1) + s - 1) * E + e] = v;
}
int vg_f32_embed_grad_launch(const float* g, float* gm, float* gt, int B, int S, int E, VgDrop drop, hipStream_t st) {
  const long long n = (long long)B * S * E;
  hipLaunchKernelGGL(vg_f32_embed_grad_kernel, dim3(nblk_f32(n)), dim3(256), 0, st, g, gm, gt, B, S, E, drop);
  return (int)hipGetLastError();
}
