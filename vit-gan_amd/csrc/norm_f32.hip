// fp32 mode: LayerNorm forward / backward over E = 128 ... 1024 (multiples of 128), eps given, biased variance (nn.LayerNorm).
// One wave per row, the row in registers (E / 64 floats per lane), two-pass statistics; the affine gradients are deterministic
// chunked column sums (gemm_f32.hip).
#include "vg_f32.h"

template <int NV>
__global__ __launch_bounds__(256) void vg_f32_ln_fwd_kernel(const float* __restrict__ x, long long xs, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ y, long long ys,
                                                            float* __restrict__ mean, float* __restrict__ rstd, int R, float eps) {
  constexpr int E = 64 * NV;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;
  const float* xr = x + (long long)r * xs;
  float v[NV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) { v[i] = xr[lane + 64 * i]; s += v[i]; }
  const float mu = vg_wave_sum(s) / (float)E;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) { const float d = v[i] - mu; q = fmaf(d, d, q); }
  const float rs = 1.0f / sqrtf(vg_wave_sum(q) / (float)E + eps);
  float* yr = y + (long long)r * ys;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    yr[c] = fmaf((v[i] - mu) * rs, gamma[c], beta[c]);
  }
  if (lane == 0) { mean[r] = mu; rstd[r] = rs; }
}

template <int NV>
__global__ __launch_bounds__(256) void vg_f32_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, long long xs,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma, const float* __restrict__ gres,
                                                            float* __restrict__ dx, long long dxs, int R) {
  constexpr int E = 64 * NV;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;
  const float mu = mean[r], rs = rstd[r];
  float xh[NV], gy[NV];
  float a = 0.f, c2 = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    xh[i] = (x[(long long)r * xs + c] - mu) * rs;
    gy[i] = dy[(long long)r * E + c] * gamma[c];
    a = fmaf(gy[i], xh[i], a);
    c2 += gy[i];
  }
  const float m1 = vg_wave_sum(a) / (float)E, m2 = vg_wave_sum(c2) / (float)E;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    float v = rs * (gy[i] - m2 - xh[i] * m1);
    if (gres) v += gres[(long long)r * dxs + c];
    dx[(long long)r * dxs + c] = v;
  }
}

#define F32_NV_SWITCH(E_, CALL)                                                                             \
  switch ((E_) >> 7) {                                                                                      \
    case 1: CALL(2); break; case 2: CALL(4); break; case 3: CALL(6); break; case 4: CALL(8); break;         \
    case 5: CALL(10); break; case 6: CALL(12); break; case 7: CALL(14); break; case 8: CALL(16); break;     \
    default: return -3;                                                                                     \
  }
int vg_f32_ln_fwd_launch(const float* x, long long xs, const float* gamma, const float* beta, float* y, long long ys, float* mean,
                         float* rstd, int R, int E, float eps, hipStream_t st) {
  if (!x || !gamma || !beta || !y || !mean || !rstd) return -1;
  if (R < 1) return -2;
  if ((E & 127) || E > 1024 || E < 128) return -3;
#define LN_F32_FWD(NV_) hipLaunchKernelGGL(vg_f32_ln_fwd_kernel<NV_>, dim3((R + 3) / 4), dim3(256), 0, st, x, xs, gamma, beta, y, ys, mean, rstd, R, eps)
  F32_NV_SWITCH(E, LN_F32_FWD)
#undef LN_F32_FWD
  return (int)hipGetLastError();
}
int vg_f32_ln_bwd_launch(const float* dy, const float* x, long long xs, const float* mean, const float* rstd, const float* gamma,
                         const float* gres, float* dx, long long dxs, float* dgamma, float* dbeta, float* part, int R, int E, hipStream_t st) {
  if (!dy || !x || !mean || !rstd || !gamma || !dx) return -1;
  if ((dgamma || dbeta) && (!dgamma || !dbeta || !part)) return -1;
  if (R < 1) return -2;
  if ((E & 127) || E > 1024 || E < 128) return -3;
#define LN_F32_BWD(NV_) hipLaunchKernelGGL(vg_f32_ln_bwd_kernel<NV_>, dim3((R + 3) / 4), dim3(256), 0, st, dy, x, xs, mean, rstd, gamma, gres, dx, dxs, R)
  F32_NV_SWITCH(E, LN_F32_BWD)
#undef LN_F32_BWD
  VG_CHECK_HIP(hipGetLastError());
  if (!dgamma) return 0;
  return vg_f32_ln_param_grads(dy, x, xs, mean, rstd, dgamma, dbeta, part, R, E, st);
}
