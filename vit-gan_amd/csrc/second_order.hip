// Second-order kernels: the derivative OF the backward operators, which the gradient penalty of the reference's
// Wasserstein step needs (src/v2/utils.py:124-144: d/d theta of ||d D(x)/d x||).  With these every
// backward operator of the discriminator has its own backward; the GEMM-shaped second-order terms reuse the GEMM family
// (the backward of dX = dY W is d(dY) = ddX W^T and dW = dY^T ddX).  They serve the penalty term only - a few launches per
// step beside the fused passes - so the elementwise ones are written for clarity and determinism (fp32 math, no atomics); the
// attention double backward, which was 18 % of the penalty step as fp32 FMA loops, runs on the MFMA pipe since round 3 (attention.hip).
// Its comparison is the fp64 reference test (tests/test_second_order_gpu.py, every S from 1 to 80); the fp32 FMA form that used to
// stay here behind a build flag lives in history, last at commit de5f7cd.
#include "vg_common.h"
// the MFMA form of the attention double backward lives with the attention kernels (attention.hip)
int vg_attn_bwd_bwd_mfma_launch(const bf16* qkv, const bf16* d_o, const float* lse, const bf16* uqkv, bf16* d_do, bf16* d_qkv, int B, int H,
                                int S, int HE, float scale, hipStream_t st);

// ---------------------------------------------------------------------------------------------------------------------
// activations: f = gelu (mode 1, exact erf) or tanh (mode 3) on a stored bf16 pre-activation h
//   fwd      y  = f(h)
//   bwd      dh = dy f'(h)
//   bwd_bwd  given u = dL/d(dh):  d(dy) = u f'(h),   d(h) = u dy f''(h)
// gelu'(h) = Phi(h) + h phi(h);  gelu''(h) = phi(h) (2 - h^2);  tanh' = 1 - t^2;  tanh'' = -2 t (1 - t^2)
__device__ __forceinline__ void act_derivs(int mode, float h, float& f, float& d1, float& d2) {
  if (mode == 1) {
    float Phi, e;
    vg_phi_e(h, Phi, e);
    const float phi = 0.39894228040143268f * e;
    // a finite bf16 |h| >= 1.85e19 squares to +inf in fp32 while phi is exactly 0: 0 * -inf would be NaN where the derivative is 0.
    // Where phi has underflowed any finite h gives the same -0, so take one whose square is finite (every other h: unchanged bits).
    const float hs = (phi == 0.0f) ? 2.0f : h;
    f = h * Phi; d1 = Phi + h * phi; d2 = phi * (2.0f - hs * hs);
  } else {
    const float t = vg_tanh(h);
    f = t; d1 = 1.0f - t * t; d2 = -2.0f * t * d1;
  }
}
__global__ __launch_bounds__(256) void vg_act2_kernel(const bf16* __restrict__ h, const bf16* __restrict__ dy, const bf16* __restrict__ u,
                                                      bf16* __restrict__ o0, bf16* __restrict__ o1, long long n, int mode, int what) {
  const long long i4 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i4 >= n) return;
  const bf16x4 hv = *(const bf16x4*)(h + i4);
  bf16x4 dv = {0, 0, 0, 0}, uv = {0, 0, 0, 0};
  if (what >= 1) dv = *(const bf16x4*)(dy + i4);
  if (what == 2) uv = *(const bf16x4*)(u + i4);
  bf16x4 a, b;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float f, d1, d2;
    act_derivs(mode, vg_bf2f(hv[j]), f, d1, d2);
    if (what == 0) a[j] = vg_f2bf(f);
    else if (what == 1) a[j] = vg_f2bf(vg_bf2f(dv[j]) * d1);
    else { a[j] = vg_f2bf(vg_bf2f(uv[j]) * d1); b[j] = vg_f2bf(vg_bf2f(uv[j]) * vg_bf2f(dv[j]) * d2); }
  }
  *(bf16x4*)(o0 + i4) = a;
  if (what == 2) *(bf16x4*)(o1 + i4) = b;
}
int vg_act2_launch(const bf16* h, const bf16* dy, const bf16* u, bf16* o0, bf16* o1, long long n, int mode, int what, hipStream_t st) {
  if ((n & 3) || (mode != 1 && mode != 3) || what < 0 || what > 2) return -3;
  hipLaunchKernelGGL(vg_act2_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, h, dy, u, o0, o1, n, mode, what);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// LayerNorm backward's backward.  LN backward: g = dy*gamma, a = mean(g), b = mean(g*xh), dx = r (g - a - xh b) with
// xh = (x - mu) r, r = rstd.  Given u = dL/d(dx) (one row each):
//   d(g)  = r (u - mean(u) - xh mean(u xh))                      -> d(dy) = d(g) gamma,  d(gamma) += d(g) dy  (per column)
//   d(xh) = -r (g mean(u xh) + b u)          (explicit)           d(r) = <u, dx> / r =: c   (explicit)
//   d(x)  = r (d(xh) - mean(d(xh)) - xh mean(d(xh) xh)) - r^2 xh c / E
// One wave per row (E <= 1024: up to 16 elements per lane), fp32 math; d(gamma) leaves as one partial row per workgroup.
// NE = E / 64 elements per lane, a compile-time constant: with the runtime count of the first version (16-element arrays behind
// `if (i < NE)`) the kernel held 256 registers and 464 bytes of scratch at one wave per SIMD - 292 us per launch over 16 640 rows.
template <int NE>
__global__ __launch_bounds__(256) void vg_ln_bwd_bwd_kernel(const bf16* __restrict__ u, const bf16* __restrict__ dy, const bf16* __restrict__ x,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma, bf16* __restrict__ d_dy, bf16* __restrict__ d_x,
                                                            float* __restrict__ part, int R) {
  constexpr int E = 64 * NE;
  __shared__ float red[4][E];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float accg[NE], gam[NE];
#pragma unroll
  for (int i = 0; i < NE; ++i) { accg[i] = 0.f; gam[i] = gamma[lane + 64 * i]; }
  constexpr float invE = 1.0f / (float)E;
  for (int row = blockIdx.x * 4 + wv; row < R; row += gridDim.x * 4) {
    const float mu = mean[row], r = rstd[row];
    float xh[NE], g[NE], uu[NE], dyv[NE];
    float s_u = 0.f, s_ux = 0.f, s_g = 0.f, s_gx = 0.f;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const size_t o = (size_t)row * E + lane + 64 * i;
      xh[i] = (vg_bf2f(x[o]) - mu) * r;
      dyv[i] = vg_bf2f(dy[o]);
      uu[i] = vg_bf2f(u[o]);
    }
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      g[i] = dyv[i] * gam[i];
      s_u += uu[i]; s_ux += uu[i] * xh[i]; s_g += g[i]; s_gx += g[i] * xh[i];
    }
    s_u = vg_wave_sum(s_u) * invE; s_ux = vg_wave_sum(s_ux) * invE; s_g = vg_wave_sum(s_g) * invE; s_gx = vg_wave_sum(s_gx) * invE;
    // c = <u, dx> / r = sum u (g - a - xh b)
    float c = 0.f, s_d = 0.f, s_dx = 0.f;
    float dxh[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      c += uu[i] * (g[i] - s_g - xh[i] * s_gx);
      dxh[i] = -r * (g[i] * s_ux + s_gx * uu[i]);
      s_d += dxh[i]; s_dx += dxh[i] * xh[i];
    }
    c = vg_wave_sum(c); s_d = vg_wave_sum(s_d) * invE; s_dx = vg_wave_sum(s_dx) * invE;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const size_t o = (size_t)row * E + lane + 64 * i;
      const float dg = r * (uu[i] - s_u - xh[i] * s_ux);
      d_dy[o] = vg_f2bf(dg * gam[i]);
      accg[i] += dg * dyv[i];
      d_x[o] = vg_f2bf(r * (dxh[i] - s_d - xh[i] * s_dx) - r * r * xh[i] * c * invE);
    }
  }
#pragma unroll
  for (int i = 0; i < NE; ++i) red[wv][lane + 64 * i] = accg[i];
  __syncthreads();
  for (int c = threadIdx.x; c < E; c += 256) part[(size_t)blockIdx.x * E + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}
// one partial row of d(gamma) per workgroup.  2048, not 256: the kernel is a chain of row reductions, latency-bound - at 256 workgroups (one wave per
// SIMD) a launch over 16 640 rows took 292 us for 64 MB; with 8 workgroups per CU the other waves cover the chain
int vg_ln_bwd_bwd_nparts(int R) { const int n = (R + 3) / 4; return n < 2048 ? n : 2048; }
int vg_ln_bwd_bwd_launch(const bf16* u, const bf16* dy, const bf16* x, const float* mean, const float* rstd, const float* gamma,
                         bf16* d_dy, bf16* d_x, float* part, int R, int E, hipStream_t st) {
  if ((E & 63) || E > 1024 || R < 1) return -3;
#define VG_LNBB(NE_) hipLaunchKernelGGL((vg_ln_bwd_bwd_kernel<NE_>), dim3(vg_ln_bwd_bwd_nparts(R)), dim3(256), 0, st, u, dy, x, mean, rstd, gamma, d_dy, d_x, part, R)
  // every width the first-order LayerNorm and vg_vit_layout accept (E % 128 == 0, E <= 1024): the penalty step must not refuse a
  // network the plain step trains (640 and 896 were missing)
  switch (E / 64) {
    case 2: VG_LNBB(2); break;
    case 4: VG_LNBB(4); break;
    case 6: VG_LNBB(6); break;
    case 8: VG_LNBB(8); break;
    case 10: VG_LNBB(10); break;
    case 12: VG_LNBB(12); break;
    case 14: VG_LNBB(14); break;
    case 16: VG_LNBB(16); break;
    default: return -3;
  }
#undef VG_LNBB
  return (int)hipGetLastError();
}

// Attention backward's backward: the range check, then vg_attn_bwd_bwd2_kernel of attention.hip.
int vg_attn_bwd_bwd_launch(const bf16* qkv, const bf16* d_o, const float* lse, const bf16* uqkv, bf16* d_do, bf16* d_qkv, int B, int H,
                           int S, int HE, float scale, hipStream_t st) {
  if (S < 1 || S > 80 || B < 1 || H < 1) return -2;
  return vg_attn_bwd_bwd_mfma_launch(qkv, d_o, lse, uqkv, d_do, d_qkv, B, H, S, HE, scale, st);
}

// ---------------------------------------------------------------------------------------------------------------------
// Small kernels of the gradient penalty as ONE C call (vg_vit_penalty, engine.hip; reference: src/v2/utils.py:124-144).
// ---------------------------------------------------------------------------------------------------------------------
// interpolated = eps * real + (1 - eps) * fake, fp32 like the reference forms it (utils.py:130); eps [B]
__global__ __launch_bounds__(256) void vg_pen_interp_kernel(const bf16* __restrict__ real, const bf16* __restrict__ fake, const float* __restrict__ eps,
                                                            float* __restrict__ out, long long per, long long n) {
  const long long i4 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i4 >= n) return;
  const float e = eps[i4 / per], f = 1.0f - e;
  const bf16x4 r = *(const bf16x4*)(real + i4), k = *(const bf16x4*)(fake + i4);
  f32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = __fadd_rn(__fmul_rn(e, vg_bf2f(r[j])), __fmul_rn(f, vg_bf2f(k[j])));
  *(f32x4*)(out + i4) = o;
}
int vg_pen_interp_launch(const bf16* real, const bf16* fake, const float* eps, float* out, int B, long long per, hipStream_t st) {
  if (B < 1 || per < 4 || (per & 3)) return -3;
  const long long n = (long long)B * per;
  hipLaunchKernelGGL(vg_pen_interp_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, real, fake, eps, out, per, n);
  return (int)hipGetLastError();
}
// One workgroup per image: n_b = ||g_b||_2 over the image's `per` gradient elements (the patch rows of d A - the same numbers as the
// image gradient, permuted), pen_img[b] = (n_b - 1)^2 / B, and the direction the second backward starts from,
// u_b = coef (n_b - 1) / n_b g_b = d(weight * mean_b (n_b - 1)^2) / d g_b with coef = 2 weight / B  (utils.py:143-144).
// R1 = 1, the zero-centred penalty on the images themselves: pen_img[b] = n_b^2 / B and u_b = coef g_b = d(weight * mean_b n_b^2) / d g_b -
// the same sum in the same order, no square root and no division (a zero gradient needs no special case).
template <int R1>
__global__ __launch_bounds__(256) void vg_pen_norm_kernel(const bf16* __restrict__ g, bf16* __restrict__ u, float* __restrict__ pen_img, long long per,
                                                          float coef, float inv_b) {
  __shared__ float red[4];
  __shared__ float fac;
  const bf16* gb = g + (size_t)blockIdx.x * per;
  bf16* ub = u + (size_t)blockIdx.x * per;
  float a = 0.f;
  for (long long i = (long long)threadIdx.x * 4; i < per; i += 1024) {
    const bf16x4 v = *(const bf16x4*)(gb + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) { const float x = vg_bf2f(v[j]); a = fmaf(x, x, a); }
  }
  a = vg_wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  float f;
  if constexpr (R1) {
    if (threadIdx.x == 0) pen_img[blockIdx.x] = ((red[0] + red[1]) + (red[2] + red[3])) * inv_b;
    f = coef;
  } else {
    if (threadIdx.x == 0) {
      const float nb = sqrtf((red[0] + red[1]) + (red[2] + red[3]));
      pen_img[blockIdx.x] = (nb - 1.0f) * (nb - 1.0f) * inv_b;
      fac = nb > 0.f ? coef * (nb - 1.0f) / nb : 0.f;  // (torch's norm has the zero subgradient at 0)
    }
    __syncthreads();
    f = fac;
  }
  for (long long i = (long long)threadIdx.x * 4; i < per; i += 1024) {
    const bf16x4 v = *(const bf16x4*)(gb + i);
    bf16x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = vg_f2bf(f * vg_bf2f(v[j]));
    *(bf16x4*)(ub + i) = o;
  }
}
__global__ __launch_bounds__(256) void vg_pen_sum_kernel(const float* __restrict__ part, int n, float* __restrict__ out) {
  __shared__ float red[4];
  float a = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) a += part[i];
  a = vg_wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (red[0] + red[1]) + (red[2] + red[3]);
}
int vg_pen_norm_launch(const bf16* g, bf16* u, float* pen_img, float* pen_out, int B, long long per, float weight, int r1, hipStream_t st) {
  if (B < 1 || per < 4 || (per & 3)) return -3;
  const float coef = 2.0f * weight / (float)B, inv_b = 1.0f / (float)B;
  if (r1) hipLaunchKernelGGL(vg_pen_norm_kernel<1>, dim3(B), dim3(256), 0, st, g, u, pen_img, per, coef, inv_b);
  else hipLaunchKernelGGL(vg_pen_norm_kernel<0>, dim3(B), dim3(256), 0, st, g, u, pen_img, per, coef, inv_b);
  hipLaunchKernelGGL(vg_pen_sum_kernel, dim3(1), dim3(256), 0, st, pen_img, B, pen_out);
  return (int)hipGetLastError();
}
// Classifier head, second order: the first backward is g_pre = g_t (1 - t^2) with g_t[e] = sum_k W2[k, e] (grad_outputs = ones) and t = tanh(p).
// Given u = dL/d g_pre:  u_gt = u (1 - t^2)  (its batch sum is dL/dW2[k, :], every k)  and  s_p = u g_t (-2 t (1 - t^2)) = dL/dp.
__global__ __launch_bounds__(256) void vg_pen_head2_kernel(const bf16* __restrict__ u, const bf16* __restrict__ t, const float* __restrict__ W2,
                                                           bf16* __restrict__ u_gt, bf16* __restrict__ s_p, int B, int E, int Kc) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * E) return;
  const int e = (int)(i % E);
  float gt = 0.f;
  for (int k = 0; k < Kc; ++k) gt += W2[(size_t)k * E + e];
  gt = vg_bf2f(vg_f2bf(gt));  // (the operator chain hands g_t on as a bf16 tensor)
  const float tv = vg_bf2f(t[i]), uv = vg_bf2f(u[i]);
  const float d1 = 1.0f - tv * tv;
  u_gt[i] = vg_f2bf(uv * d1);
  s_p[i] = vg_f2bf(uv * gt * (-2.0f * tv * d1));
}
int vg_pen_head2_launch(const bf16* u, const bf16* t, const float* W2, bf16* u_gt, bf16* s_p, int B, int E, int Kc, hipStream_t st) {
  if (B < 1 || E < 1 || Kc < 1) return -3;
  hipLaunchKernelGGL(vg_pen_head2_kernel, dim3((unsigned)(((long long)B * E + 255) / 256)), dim3(256), 0, st, u, t, W2, u_gt, s_p, B, E, Kc);
  return (int)hipGetLastError();
}
// out = a + b (one rounding; out may alias a): where the second backward meets a gradient the double backward injected
__global__ __launch_bounds__(256) void vg_add_bf16_kernel(const bf16* __restrict__ a, const bf16* __restrict__ b, bf16* __restrict__ out, long long n) {
  const long long i8 = ((long long)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i8 >= n) return;
  const bf16x8 x = *(const bf16x8*)(a + i8), y = *(const bf16x8*)(b + i8);
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = vg_f2bf(vg_bf2f(x[j]) + vg_bf2f(y[j]));
  *(bf16x8*)(out + i8) = o;
}
int vg_add_bf16_launch(const bf16* a, const bf16* b, bf16* out, long long n, hipStream_t st) {
  if (n < 8 || (n & 7)) return -3;
  hipLaunchKernelGGL(vg_add_bf16_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, st, a, b, out, n);
  return (int)hipGetLastError();
}
__global__ __launch_bounds__(256) void vg_fill_f32_kernel(float* __restrict__ p, long long n, float v) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = v;
}
int vg_fill_f32_launch(float* p, long long n, float v, hipStream_t st) {
  if (n < 1) return -3;
  hipLaunchKernelGGL(vg_fill_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p, n, v);
  return (int)hipGetLastError();
}
