// Differentiable augmentation of the discriminator's input (DiffAugment: color, translation, cutout) and its adjoint, gfx950.
//
// Per image  T = cutout o translation o contrast o saturation o brightness  with the parameters of vg_aug_draw (vg_common.h;
// the definition a test restates is in include/vitgan_hip.h).  bf16 [B, C, IH, IH] in and out, fp32 arithmetic.  With
//   Mx = mean of the image (C*IH*IH elements),  mx = mean over the C channels of one pixel,  live(i, j) = the output pixel has its
//   source (i - ty, j - tx) inside the frame and lies outside the cutout square
// the three color members collapse to one affine form in which the brightness never meets a subtraction:
//   forward   y[c,i,j]  = live ? (Mx + b) + k ((mx - Mx) + s (x[c, i-ty, j-tx] - mx)) : 0            (k = contrast, s = saturation)
//   adjoint   g[c,i,j]  = live'(i+ty, j+tx) ? dy[c, i+ty, j+tx] : 0      (live' = the same predicate at the output pixel (i+ty, j+tx))
//             dx[c,i,j] = k (s g + (1 - s) mean_channels(g)) + (1 - k) mean_image(g)                      (brightness contributes nothing)
// T is affine in x, so the adjoint needs dy and the key only.
//
// One workgroup per image, two passes over it and no scratch: pass 1 the image sum (forward: of x; adjoint: of the masked dy, read in
// place - the shift only permutes the terms), pass 2 the elements.  A thread owns chunks of 8 consecutive pixels of the IH*IH plane in
// all C channels: the store of a chunk is one 16-byte store per channel whenever IH*IH % 8 == 0 (every geometry of vg_vit_layout's
// patch grids), pass 1 and an untranslated pass 2 load 16 bytes alike; a translated source run starts at any element, so it is
// gathered with 2-byte loads that the first pass has just brought into the cache.  Other IH*IH take 2-byte accesses throughout.
//
// The sum has ONE order whatever the machine does: 8 elements of a chunk pairwise, chunks and channels serially in the thread's own
// order, the 64 lanes by the xor butterfly, the waves serially from LDS - no float atomics, bitwise reproducible.  Its depth, which
// the tests turn into their error bound: 3 + C * ceil(ceil(IH*IH / 8) / NT) + 6 + NT / 64 with NT = vg_aug_threads(IH).
#include "vg_common.h"
#include "vg_kernels.h"

namespace {

__device__ __forceinline__ float vg_aug_raw2f(uint16_t r) { return __uint_as_float((uint32_t)r << 16); }
__device__ __forceinline__ uint16_t vg_aug_f2raw(float v) {
  const bf16 h = vg_f2bf(v);
  return __builtin_bit_cast(uint16_t, h);
}

// 8 consecutive elements at p (valid: how many of them exist), as raw bf16 bits; vec: p is 16-byte aligned and all 8 exist
__device__ __forceinline__ void vg_aug_load8(const uint16_t* __restrict__ p, bool vec, int valid, uint16_t (&r)[8]) {
  if (vec) {
    const u32x4 w = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      r[2 * e] = (uint16_t)(w[e] & 0xFFFFu);
      r[2 * e + 1] = (uint16_t)(w[e] >> 16);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = e < valid ? p[e] : (uint16_t)0;
  }
}
__device__ __forceinline__ void vg_aug_store8(uint16_t* __restrict__ p, bool vec, int valid, const uint16_t (&r)[8]) {
  if (vec) {
    u32x4 w;
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = (uint32_t)r[2 * e] | ((uint32_t)r[2 * e + 1] << 16);
    *reinterpret_cast<u32x4*>(p) = w;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (e < valid) p[e] = r[e];
  }
}

// CT: the channel count when it is 1 or 3 (a chunk's channels stay in registers between the channel mean and the output), 0: any C
// (the chunk is read a second time).  ADJ: the adjoint.
// GATED (vg_diffaug_p_fwd / _bwd): every member of `policy_in` is applied to an image with probability prob[0], read HERE so that a
// replayed hipGraph sees the current value.  The workgroup is the image, so its effective policy is block-uniform, and from there on
// the image is processed as the plain kernel processes it under that policy: same draws, same code, same bits.  The plain
// instantiations never touch `prob` (a trailing argument, nullptr).
template <int CT, bool ADJ, bool GATED>
__global__ __launch_bounds__(1024) void vg_diffaug_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out,
                                                          float* __restrict__ params_out, int C, int IH, int policy_in, uint32_t key,
                                                          const unsigned* __restrict__ dstep, int accumulate,
                                                          const float* __restrict__ prob) {
  const int policy = GATED ? vg_aug_gate(key, dstep, (uint32_t)blockIdx.x, policy_in, prob[0]) : policy_in;
  const int n = blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
  const int Cn = CT ? CT : C;
  const int HW = IH * IH;
  const long long per = (long long)Cn * HW;
  const uint16_t* __restrict__ x = in + n * per;
  uint16_t* __restrict__ y = out + n * per;
  const VgAug a = vg_aug_draw(key, dstep, (uint32_t)n, IH, policy);
  if (params_out && tid == 0) {
    f32x4* po = reinterpret_cast<f32x4*>(params_out + 8ll * n);
    po[0] = f32x4{a.b, a.s, a.k, (float)a.tx};
    po[1] = f32x4{(float)a.ty, (float)a.cx, (float)a.cy, (float)policy};
  }
  const bool color = (policy & 1) != 0;
  const bool vec = (HW & 7) == 0;            // channel planes start on 16 bytes and every chunk is whole
  const bool straight = a.tx == 0 && a.ty == 0;
  const int nch = (HW + 7) >> 3;
  // the cutout square [r0, r1) x [c0, c1) in OUTPUT coordinates (empty when the member is off: vg_aug_draw puts it off the image)
  const int q4 = IH >> 2, half = IH >> 1;
  const int r0 = a.cy - q4, r1 = r0 + half, c0 = a.cx - q4, c1 = c0 + half;
  // output pixel (i, j) of the forward reads source (i - ty, j - tx); source pixel (i, j) of the adjoint reads output (i + ty, j + tx)
  const int dyv = ADJ ? a.ty : -a.ty, dxv = ADJ ? a.tx : -a.tx;
  auto in_cut = [&](int i, int j) { return i >= r0 && i < r1 && j >= c0 && j < c1; };
  auto in_frame = [&](int i, int j) { return (unsigned)i < (unsigned)IH && (unsigned)j < (unsigned)IH; };

  float Mx = 0.f;
  if (color) {
    float acc = 0.f;
    for (int ch = tid; ch < nch; ch += NT) {
      const int q = ch << 3;
      bool keep[8];
      if (ADJ) {  // dy[i', j'] reaches the input iff it is outside the cutout and its source pixel exists
        int i = q / IH, j = q - i * IH;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          keep[e] = !in_cut(i, j) && in_frame(i - a.ty, j - a.tx);
          if (++j == IH) { j = 0; ++i; }
        }
      }
      for (int c = 0; c < Cn; ++c) {
        uint16_t r[8];
        vg_aug_load8(x + (long long)c * HW + q, vec, HW - q, r);
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (!ADJ || keep[e]) ? vg_aug_raw2f(r[e]) : 0.f;
        acc += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
      }
    }
    acc = vg_wave_sum(acc);
    __shared__ float red[16];
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    float t = 0.f;
    for (int w = 0; w < (NT >> 6); ++w) t += red[w];
    Mx = t * (1.0f / (float)per);
  }
  const float invC = 1.0f / (float)Cn;

  for (int ch = tid; ch < nch; ch += NT) {
    const int q = ch << 3;
    const int valid = HW - q;
    int src[8];  // element offset inside a channel plane of what this element reads, -1: nothing (reads as zero)
    {
      int i = q / IH, j = q - i * IH;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int si = i + dyv, sj = j + dxv;
        const bool live = e < valid && in_frame(si, sj) && !(ADJ ? in_cut(si, sj) : in_cut(i, j));
        src[e] = live ? si * IH + sj : -1;
        if (++j == IH) { j = 0; ++i; }
      }
    }
    auto gather = [&](int c, uint16_t (&r)[8]) {
      const uint16_t* __restrict__ pl = x + (long long)c * HW;
      if (straight) {  // the source chunk is this chunk
        vg_aug_load8(pl + q, vec, valid, r);
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = src[e] >= 0 ? r[e] : (uint16_t)0;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = src[e] >= 0 ? pl[src[e]] : (uint16_t)0;
      }
    };
    if (!color) {  // translation and cutout move and drop bf16 values: bits in, bits out
      for (int c = 0; c < Cn; ++c) {
        uint16_t r[8];
        gather(c, r);
        uint16_t* yo = y + (long long)c * HW + q;
        if (ADJ && accumulate) {
          uint16_t o[8];
          vg_aug_load8(yo, vec, valid, o);
#pragma unroll
          for (int e = 0; e < 8; ++e) r[e] = vg_aug_f2raw(vg_aug_raw2f(o[e]) + vg_aug_raw2f(r[e]));
        }
        vg_aug_store8(yo, vec, valid, r);
      }
      continue;
    }
    uint16_t held[CT ? CT : 1][8];
    float mx[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) mx[e] = 0.f;
    for (int c = 0; c < Cn; ++c) {
      uint16_t r[8];
      gather(c, r);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        mx[e] += vg_aug_raw2f(r[e]);
        if (CT) held[CT ? c : 0][e] = r[e];
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) mx[e] *= invC;
    for (int c = 0; c < Cn; ++c) {
      uint16_t r[8];
      if (CT) {
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = held[CT ? c : 0][e];
      } else {
        gather(c, r);
      }
      uint16_t* yo = y + (long long)c * HW + q;
      uint16_t o[8];
      if (ADJ && accumulate) vg_aug_load8(yo, vec, valid, o);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float g = vg_aug_raw2f(r[e]);
        float v;
        if (!ADJ) {
          v = (Mx + a.b) + a.k * ((mx[e] - Mx) + a.s * (g - mx[e]));
          v = src[e] >= 0 ? v : 0.f;
        } else {
          v = a.k * (a.s * g + (1.0f - a.s) * mx[e]) + (1.0f - a.k) * Mx;
          if (accumulate) v += vg_aug_raw2f(o[e]);
        }
        r[e] = vg_aug_f2raw(v);
      }
      vg_aug_store8(yo, vec, valid, r);
    }
  }
}

template <bool ADJ, bool GATED>
int vg_diffaug_launch_t(const bf16* in, bf16* out, float* params_out, int accumulate, int B, int C, int IH, int policy, unsigned key,
                        const unsigned* dstep, const float* prob, hipStream_t st) {
  const dim3 grid(B), block(vg_aug_threads(IH));
  const uint16_t* i16 = (const uint16_t*)in;
  uint16_t* o16 = (uint16_t*)out;
  if (C == 3)
    hipLaunchKernelGGL((vg_diffaug_kernel<3, ADJ, GATED>), grid, block, 0, st, i16, o16, params_out, C, IH, policy, key, dstep, accumulate, prob);
  else if (C == 1)
    hipLaunchKernelGGL((vg_diffaug_kernel<1, ADJ, GATED>), grid, block, 0, st, i16, o16, params_out, C, IH, policy, key, dstep, accumulate, prob);
  else
    hipLaunchKernelGGL((vg_diffaug_kernel<0, ADJ, GATED>), grid, block, 0, st, i16, o16, params_out, C, IH, policy, key, dstep, accumulate, prob);
  return (int)hipGetLastError();
}

}  // namespace

// prob == nullptr: the plain kernels; else the gated ones, which read the probability from prob[0] on the device
int vg_diffaug_fwd_launch(const bf16* x, bf16* y, float* params_out, int B, int C, int IH, int policy, unsigned key, const unsigned* dstep,
                          hipStream_t st, const float* prob) {
  return prob ? vg_diffaug_launch_t<false, true>(x, y, params_out, 0, B, C, IH, policy, key, dstep, prob, st)
              : vg_diffaug_launch_t<false, false>(x, y, params_out, 0, B, C, IH, policy, key, dstep, nullptr, st);
}
int vg_diffaug_bwd_launch(const bf16* dy, bf16* dx, int accumulate, int B, int C, int IH, int policy, unsigned key, const unsigned* dstep,
                          hipStream_t st, const float* prob) {
  return prob ? vg_diffaug_launch_t<true, true>(dy, dx, nullptr, accumulate, B, C, IH, policy, key, dstep, prob, st)
              : vg_diffaug_launch_t<true, false>(dy, dx, nullptr, accumulate, B, C, IH, policy, key, dstep, nullptr, st);
}
