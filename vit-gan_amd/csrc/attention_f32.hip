// fp32 mode: multi-head self-attention with dot-product scores (src/v2/modules.py:142-159), forward and backward, fp32 throughout.
// One 256-thread workgroup per (image, head); K and V of the head sit in LDS (rows padded to HE + 1 floats, so lane j reading
// row j hits bank j), each wave takes one query row at a time.  Scores use accurate expf / logf; the forward saves the lse and the
// backward recomputes P = exp(s - lse) from it.  The backward is deterministic: dQ from the row's dS in LDS, dK / dV from the
// whole head's P and dS matrices (kept in LDS, 2 x 80 x 81 floats) summed over the query rows in order.
#include "vg_f32.h"

#define FA_SMAX 80

template <int HE>
__global__ __launch_bounds__(256) void vg_f32_attn_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out, float* __restrict__ lse,
                                                              int H, int S, float scale) {
  __shared__ float Ks[FA_SMAX][HE + 1];
  __shared__ float Vs[FA_SMAX][HE + 1];
  __shared__ float qrow[4][HE];
  __shared__ float prow[4][FA_SMAX];
  const int bh = blockIdx.x, b = bh / H, h = bh % H;
  const int E = H * HE, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long ld = 3LL * E;
  const float* base = qkv + (long long)b * S * ld + h * HE;
  for (int t = threadIdx.x; t < S * HE; t += 256) {
    const int j = t / HE, d = t - j * HE;
    Ks[j][d] = base[j * ld + E + d];
    Vs[j][d] = base[j * ld + 2 * E + d];
  }
  __syncthreads();
  for (int i0 = 0; i0 < S; i0 += 4) {
    const int i = i0 + w;
    const bool valid = i < S;  // wave-uniform
    float m = 0.f, l = 1.f;
    if (valid)
      for (int d = lane; d < HE; d += 64) qrow[w][d] = base[i * ld + d];
    __syncthreads();
    if (valid) {
      float s0 = -INFINITY, s1 = -INFINITY;
      if (lane < S) {
        float a = 0.f;
#pragma unroll 8
        for (int d = 0; d < HE; ++d) a = fmaf(qrow[w][d], Ks[lane][d], a);
        s0 = a * scale;
      }
      if (lane + 64 < S) {
        float a = 0.f;
#pragma unroll 8
        for (int d = 0; d < HE; ++d) a = fmaf(qrow[w][d], Ks[lane + 64][d], a);
        s1 = a * scale;
      }
      m = vg_wave_max(fmaxf(s0, s1));
      const float p0 = lane < S ? expf(s0 - m) : 0.f, p1 = lane + 64 < S ? expf(s1 - m) : 0.f;
      l = vg_wave_sum(p0 + p1);
      if (lane < S) prow[w][lane] = p0;
      if (lane + 64 < S) prow[w][lane + 64] = p1;
    }
    __syncthreads();
    if (valid) {
      const float inv = 1.0f / l;
      for (int d = lane; d < HE; d += 64) {
        float a = 0.f;
        for (int j = 0; j < S; ++j) a = fmaf(prow[w][j], Vs[j][d], a);
        out[((long long)b * S + i) * E + h * HE + d] = a * inv;
      }
      if (lane == 0) lse[(long long)bh * S + i] = m + logf(l);
    }
    __syncthreads();
  }
}

template <int HE>
__global__ __launch_bounds__(256) void vg_f32_attn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ o,
                                                              const float* __restrict__ d_o, const float* __restrict__ lse,
                                                              float* __restrict__ dqkv, int H, int S, float scale) {
  __shared__ float Ks[FA_SMAX][HE + 1];
  __shared__ float Vs[FA_SMAX][HE + 1];
  __shared__ float Ps[FA_SMAX][FA_SMAX + 1];
  __shared__ float Ds[FA_SMAX][FA_SMAX + 1];
  __shared__ float qrow[4][HE];
  __shared__ float grow[4][HE];
  const int bh = blockIdx.x, b = bh / H, h = bh % H;
  const int E = H * HE, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long ld = 3LL * E;
  const float* base = qkv + (long long)b * S * ld + h * HE;
  float* dbase = dqkv + (long long)b * S * ld + h * HE;
  const float* obase = o + (long long)b * S * E + h * HE;
  const float* gbase = d_o + (long long)b * S * E + h * HE;
  for (int t = threadIdx.x; t < S * HE; t += 256) {
    const int j = t / HE, d = t - j * HE;
    Ks[j][d] = base[j * ld + E + d];
    Vs[j][d] = base[j * ld + 2 * E + d];
  }
  __syncthreads();
  // pass 1, one query row per wave: P and dS = P (dP - rowsum(dO o)) into LDS, dQ = scale dS K
  for (int i0 = 0; i0 < S; i0 += 4) {
    const int i = i0 + w;
    const bool valid = i < S;
    float Di = 0.f;
    if (valid) {
      for (int d = lane; d < HE; d += 64) {
        const float g = gbase[(long long)i * E + d];
        qrow[w][d] = base[i * ld + d];
        grow[w][d] = g;
        Di = fmaf(g, obase[(long long)i * E + d], Di);
      }
      Di = vg_wave_sum(Di);
    }
    __syncthreads();
    if (valid) {
      const float li = lse[(long long)bh * S + i];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int j = lane + 64 * half;
        if (j < S) {
          float s = 0.f, dp = 0.f;
#pragma unroll 8
          for (int d = 0; d < HE; ++d) {
            s = fmaf(qrow[w][d], Ks[j][d], s);
            dp = fmaf(grow[w][d], Vs[j][d], dp);
          }
          const float p = expf(s * scale - li);
          Ps[i][j] = p;
          Ds[i][j] = p * (dp - Di);
        }
      }
    }
    __syncthreads();
    if (valid)
      for (int d = lane; d < HE; d += 64) {
        float a = 0.f;
        for (int j = 0; j < S; ++j) a = fmaf(Ds[i][j], Ks[j][d], a);
        dbase[i * ld + d] = a * scale;
      }
  }
  __syncthreads();
  // pass 2, one key row per wave: dK = scale dS^T Q, dV = P^T dO (query rows in order)
  for (int j = w; j < S; j += 4)
    for (int d = lane; d < HE; d += 64) {
      float ak = 0.f, av = 0.f;
      for (int i = 0; i < S; ++i) {
        ak = fmaf(Ds[i][j], base[i * ld + d], ak);
        av = fmaf(Ps[i][j], gbase[(long long)i * E + d], av);
      }
      dbase[j * ld + E + d] = ak * scale;
      dbase[j * ld + 2 * E + d] = av;
    }
}

#define FA_DISPATCH(KERNEL, ...)                                                                                         \
  switch (HE) {                                                                                                          \
    case 32: hipLaunchKernelGGL(KERNEL<32>, dim3(B * H), dim3(256), 0, st, __VA_ARGS__); break;                          \
    case 64: hipLaunchKernelGGL(KERNEL<64>, dim3(B * H), dim3(256), 0, st, __VA_ARGS__); break;                          \
    case 96: hipLaunchKernelGGL(KERNEL<96>, dim3(B * H), dim3(256), 0, st, __VA_ARGS__); break;                          \
    default: return -3;                                                                                                  \
  }
int vg_f32_attn_fwd_launch(const float* qkv, float* out, float* lse, int B, int H, int S, int HE, float scale, hipStream_t st) {
  if (!qkv || !out || !lse) return -1;
  if (B < 1 || H < 1 || S < 1) return -2;
  if (S > FA_SMAX) return -3;
  FA_DISPATCH(vg_f32_attn_fwd_kernel, qkv, out, lse, H, S, scale)
  return (int)hipGetLastError();
}
int vg_f32_attn_bwd_launch(const float* qkv, const float* o, const float* d_o, const float* lse, float* dqkv, int B, int H, int S, int HE,
                           float scale, hipStream_t st) {
  if (!qkv || !o || !d_o || !lse || !dqkv) return -1;
  if (B < 1 || H < 1 || S < 1) return -2;
  if (S > FA_SMAX) return -3;
  FA_DISPATCH(vg_f32_attn_bwd_kernel, qkv, o, d_o, lse, dqkv, H, S, scale)
  return (int)hipGetLastError();
}
