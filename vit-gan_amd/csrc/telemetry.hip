// Per-step telemetry written by the step itself (include/vitgan_hip.h: vg_grad_stats, vg_logit_stats, vg_telemetry_commit).
// Three small kernels, every one enqueue-only, deterministic (no float atomics: every sum is a fixed tree), plain C++ with vector
// stores.  The trees are restated operation for operation in tests/telemetry_ref.py; contraction is off wherever a product feeds a sum,
// so that restatement and the kernel round alike.
#include "vg_common.h"
#include "vg_kernels.h"
#include "../../include/vitgan_hip.h"

#define VG_GS_THREADS 256
#define VG_GS_CHUNK 4096      // elements per chunk at most: 256 threads x 4 loads of 16 bytes
#define VG_GS_MAX_GRID 2048
#define VG_GS_MAX_SEG 2048    // segments of one buffer (the second pass keeps one fp64 sum per segment in LDS)
#define VG_LS_THREADS 1024
#define VG_LS_MAX_N (1024 * 16)

// ---- pass 1: one partial per CHUNK (first, count, segment), so the result does not depend on the grid --------------------------------
// A chunk [first, first + count) is split at the 16-byte boundaries of g: head = (-first) & 3 elements (at most count), then nv whole
// float4, then the tail.  Thread t: a = 0; for k = 0..3, v = t + 256 k < nv: a += (x0 x0 + x1 x1) + (x2 x2 + x3 x3) of vector v (the four
// loads are issued before the first add); then thread t < head adds the square of head element t, then thread t < tail the square of
// tail element t.  The 256 values: wave butterfly (xor 32, 16, .., 1), then (w0 + w1) + (w2 + w3).  Non-finite elements are counted in
// integers.  Nothing outside the chunk is read; a table entry that does not lie inside [0, n) is skipped (its partial is +0, 0).
__global__ __launch_bounds__(VG_GS_THREADS) void vg_grad_stats_part_kernel(const float* __restrict__ g, long long n, const int* __restrict__ chunks,
                                                                           int n_chunks, float* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ float red[4];
  __shared__ unsigned cnt[4];
  const int t = threadIdx.x;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int first = chunks[3 * c], count = chunks[3 * c + 1];
    float a = 0.f;
    unsigned bad = 0;
    if (first >= 0 && count > 0 && count <= VG_GS_CHUNK && (long long)first + count <= n) {  // (block-uniform)
      int head = (4 - (first & 3)) & 3;
      if (head > count) head = count;
      const int nv = (count - head) >> 2, tail = (count - head) & 3;
      const float* body = g + first + head;  // 16-byte aligned: g is, and first + head is a multiple of 4
      f32x4 x[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int v = t + VG_GS_THREADS * k;
        x[k] = v < nv ? *reinterpret_cast<const f32x4*>(body + 4 * v) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        a += (x[k][0] * x[k][0] + x[k][1] * x[k][1]) + (x[k][2] * x[k][2] + x[k][3] * x[k][3]);
#pragma unroll
        for (int j = 0; j < 4; ++j) bad += !(fabsf(x[k][j]) <= 3.402823466e38f);
      }
      if (t < head) {
        const float h = g[first + t];
        a += h * h;
        bad += !(fabsf(h) <= 3.402823466e38f);
      }
      if (t < tail) {
        const float h = body[4 * nv + t];
        a += h * h;
        bad += !(fabsf(h) <= 3.402823466e38f);
      }
    }
    a = vg_wave_sum(a);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
    if ((t & 63) == 0) { red[t >> 6] = a; cnt[t >> 6] = bad; }
    __syncthreads();
    if (t == 0) {
      part[2 * c] = (red[0] + red[1]) + (red[2] + red[3]);
      part[2 * c + 1] = (float)((cnt[0] + cnt[1]) + (cnt[2] + cnt[3]));  // <= 4096: exact
    }
    __syncthreads();
  }
}

// ---- pass 2: one workgroup.  Thread t owns segments t, t + 256, ..: its chunks' partials added in chunk order in fp64 ---------------------
// The partials pass through LDS in tiles of 2048 chunks (loaded by all threads, coalesced), so the one long chain of a large tensor - the
// generator's mapping Linear is 3072 chunks - reads LDS, not memory: the ORDER of the additions is the chunk order whatever the tiling.
// norm_seg[s] = float(gscale sqrt(sum_s));  totals = (sum_s (double) norm_seg[s], gscale sqrt(sum_s sum_s), min(count, 2^24), 0), both sums
// in segment order in fp64 by thread 0, written as one 16-byte store.
#define VG_GS_TILE 2048
#define VG_GS_OWN (VG_GS_MAX_SEG / VG_GS_THREADS)
__global__ __launch_bounds__(VG_GS_THREADS) void vg_grad_stats_fold_kernel(const float* __restrict__ part, const int* __restrict__ seg_first, int n_seg,
                                                                           int n_chunks, float gscale, float* __restrict__ norm_seg,
                                                                           float* __restrict__ totals) {
#pragma clang fp contract(off)
  __shared__ double ssum[VG_GS_MAX_SEG];
  __shared__ float snorm[VG_GS_MAX_SEG];
  __shared__ float2 tile[VG_GS_TILE];
  __shared__ unsigned bad_all;
  const int t = threadIdx.x;
  if (t == 0) bad_all = 0u;
  double acc[VG_GS_OWN];
  float nb[VG_GS_OWN];
#pragma unroll
  for (int j = 0; j < VG_GS_OWN; ++j) { acc[j] = 0.0; nb[j] = 0.f; }
  for (int base = 0; base < n_chunks; base += VG_GS_TILE) {
    const int end = base + VG_GS_TILE < n_chunks ? base + VG_GS_TILE : n_chunks;
    for (int c = base + t; c < end; c += VG_GS_THREADS) tile[c - base] = *reinterpret_cast<const float2*>(part + 2 * c);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < VG_GS_OWN; ++j) {
      const int s = t + VG_GS_THREADS * j;
      if (s < n_seg) {
        int c0 = seg_first[s], c1 = seg_first[s + 1];
        if (c0 < base) c0 = base;
        if (c1 > end) c1 = end;
#pragma unroll 8
        for (int c = c0; c < c1; ++c) {
          const float2 p = tile[c - base];
          acc[j] += (double)p.x;
          nb[j] += p.y;  // integer-valued; saturates harmlessly far above 2^24
        }
      }
    }
    __syncthreads();
  }
  unsigned bad = 0;
#pragma unroll
  for (int j = 0; j < VG_GS_OWN; ++j) {
    const int s = t + VG_GS_THREADS * j;
    if (s < n_seg) {
      const float nrm = (float)((double)gscale * sqrt(acc[j]));
      ssum[s] = acc[j];
      snorm[s] = nrm;
      norm_seg[s] = nrm;
      bad += nb[j] >= 16777216.f ? 16777216u : (unsigned)nb[j];
    }
  }
  if (bad) atomicAdd(&bad_all, bad > 16777216u ? 16777216u : bad);  // integers: the order cannot matter (at most 256 x 2^24 < 2^32)
  __syncthreads();
  if (t == 0) {
    double total = 0.0, norms = 0.0;
    for (int s = 0; s < n_seg; ++s) {
      total += ssum[s];
      norms += (double)snorm[s];
    }
    const unsigned b = bad_all > 16777216u ? 16777216u : bad_all;
    *reinterpret_cast<f32x4*>(totals) = f32x4{(float)norms, (float)((double)gscale * sqrt(total)), (float)b, 0.f};
  }
}

int vg_grad_stats_launch(const float* g, long long n, const int* chunks, int n_chunks, const int* seg_first, int n_seg, float gscale,
                         float* scratch, float* norm_seg, float* totals, hipStream_t st) {
  const int grid = n_chunks < VG_GS_MAX_GRID ? n_chunks : VG_GS_MAX_GRID;
  hipLaunchKernelGGL(vg_grad_stats_part_kernel, dim3(grid), dim3(VG_GS_THREADS), 0, st, g, n, chunks, n_chunks, scratch);
  hipLaunchKernelGGL(vg_grad_stats_fold_kernel, dim3(1), dim3(VG_GS_THREADS), 0, st, scratch, seg_first, n_seg, n_chunks, gscale, norm_seg, totals);
  return (int)hipGetLastError();
}

// ---- logit statistics: workgroup j of the launch reads rows x_j[0, n) and writes slot role + j of out[3][4] ---------------------------
// Thread t: a = x[t] + x[t + 1024] + ... in index order (at most 16 terms); wave butterfly; the 16 wave sums by one more butterfly of
// wave 0 (lanes >= 16 hold +0); mean = sum / (float) n.  logit > 0 and logit < 0 are counted in integers (+-0 and NaN in neither),
// the fractions are one fp32 division each.  The slot is one 16-byte store (mean, frac_pos, frac_neg, n).
__global__ __launch_bounds__(VG_LS_THREADS) void vg_logit_stats_kernel(const float* __restrict__ x0, const float* __restrict__ x1, int n, int role,
                                                                       float* __restrict__ out) {
  __shared__ float red[16];
  __shared__ int pos[16], neg[16];
  const float* __restrict__ x = blockIdx.x == 0 ? x0 : x1;
  const int t = threadIdx.x;
  float a = 0.f;
  int p = 0, m = 0;
  for (int i = t; i < n; i += VG_LS_THREADS) {
    const float v = x[i];
    a += v;
    p += v > 0.f;
    m += v < 0.f;
  }
  a = vg_wave_sum(a);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    p += __shfl_xor(p, o, 64);
    m += __shfl_xor(m, o, 64);
  }
  if ((t & 63) == 0) { red[t >> 6] = a; pos[t >> 6] = p; neg[t >> 6] = m; }
  __syncthreads();
  if (t < 64) {
    float s = t < 16 ? red[t] : 0.f;
    int ps = t < 16 ? pos[t] : 0, ms = t < 16 ? neg[t] : 0;
    s = vg_wave_sum(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      ps += __shfl_xor(ps, o, 64);
      ms += __shfl_xor(ms, o, 64);
    }
    if (t == 0) {
      const float fn = (float)n;
      *reinterpret_cast<f32x4*>(out + 4 * (role + (int)blockIdx.x)) = f32x4{s / fn, (float)ps / fn, (float)ms / fn, fn};
    }
  }
}

int vg_logit_stats_launch(const float* x0, const float* x1, int n, int role, float* out, hipStream_t st) {
  hipLaunchKernelGGL(vg_logit_stats_kernel, dim3(x1 ? 2 : 1), dim3(VG_LS_THREADS), 0, st, x0, x1, n, role, out);
  return (int)hipGetLastError();
}

// ---- commit: row (t - 1) % cap of the rings, t = step[0] as vg_zero_tick left it -------------------------------------------------------
__device__ __forceinline__ float vg_tel_at(const float* p, int i) { return p ? p[i] : __builtin_nanf(""); }
__device__ __forceinline__ float vg_tel_field(const VgTelemetrySrc& s, int f) {
  switch (f) {
    case VG_TEL_LOSS_D_REAL: return vg_tel_at(s.losses, 0);
    case VG_TEL_LOSS_D_FAKE: return vg_tel_at(s.losses, 1);
    case VG_TEL_LOSS_G: return vg_tel_at(s.losses, 2);
    case VG_TEL_D_REAL_MEAN: return vg_tel_at(s.logit_stats, 0);
    case VG_TEL_D_FAKE_MEAN: return vg_tel_at(s.logit_stats, 4);
    case VG_TEL_D_REAL_ACC: return vg_tel_at(s.logit_stats, 1);   // fraction of real logits > 0
    case VG_TEL_D_FAKE_ACC: return vg_tel_at(s.logit_stats, 6);   // fraction of fake logits < 0
    case VG_TEL_G_MEAN: return vg_tel_at(s.logit_stats, 8);
    case VG_TEL_G_FRAC_POS: return vg_tel_at(s.logit_stats, 9);
    case VG_TEL_GNORM_D_SUM: return vg_tel_at(s.grad_d, 0);
    case VG_TEL_GNORM_D_L2: return vg_tel_at(s.grad_d, 1);
    case VG_TEL_GNORM_G_SUM: return vg_tel_at(s.grad_g, 0);
    case VG_TEL_GNORM_G_L2: return vg_tel_at(s.grad_g, 1);
    case VG_TEL_NONFINITE_D: return vg_tel_at(s.grad_d, 2);
    case VG_TEL_NONFINITE_G: return vg_tel_at(s.grad_g, 2);
    case VG_TEL_PENALTY: return s.penalty_due ? vg_tel_at(s.penalty, 0) : __builtin_nanf("");
    case VG_TEL_BCR_REAL: return vg_tel_at(s.bcr, 0);
    case VG_TEL_BCR_FAKE: return vg_tel_at(s.bcr, 1);
    case VG_TEL_ADA_P: return vg_tel_at(s.ada_state, 0);
    case VG_TEL_ADA_RT: return vg_tel_at(s.ada_state, 3);
    case VG_TEL_LR_D: return vg_tel_at(s.lr, 0);
    case VG_TEL_LR_G: return vg_tel_at(s.lr, 1);
    case VG_TEL_DIVERSITY: return vg_tel_at(s.diversity, 0);
    default: return __builtin_nanf("");
  }
}
__global__ __launch_bounds__(256) void vg_telemetry_commit_kernel(VgTelemetrySrc s, const int* __restrict__ step, int cap, int* __restrict__ ring_step,
                                                                  float* __restrict__ ring, float* __restrict__ ring_seg_d,
                                                                  float* __restrict__ ring_seg_g) {
  const int t = step[0];
  if (t < 1) return;  // no step has run: there is no row to write
  const long long row = (long long)((t - 1) % cap);
  const int i = threadIdx.x;
  if (i == 0) ring_step[row] = t;
  if (i < VG_TEL_NF) ring[row * VG_TEL_NF + i] = vg_tel_field(s, i);
  if (s.seg_d)
    for (int k = i; k < s.n_seg_d; k += 256) ring_seg_d[row * s.n_seg_d + k] = s.seg_d[k];
  if (s.seg_g)
    for (int k = i; k < s.n_seg_g; k += 256) ring_seg_g[row * s.n_seg_g + k] = s.seg_g[k];
}

int vg_telemetry_commit_launch(const VgTelemetrySrc* src, const int* step_dev, int cap, int* ring_step, float* ring, float* ring_seg_d,
                               float* ring_seg_g, hipStream_t st) {
  hipLaunchKernelGGL(vg_telemetry_commit_kernel, dim3(1), dim3(256), 0, st, *src, step_dev, cap, ring_step, ring, ring_seg_d, ring_seg_g);
  return (int)hipGetLastError();
}

// ---- the C entries: every argument error before any launch ------------------------------------------------------------------------------
static inline bool vg_tel_misaligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) != 0; }
extern "C" int vg_grad_stats(const float* g, long long n, const int* chunks, int n_chunks, const int* seg_first, int n_seg, float gscale,
                             float* scratch, float* norm_seg, float* totals, void* stream) {
  if (!g || !chunks || !seg_first || !scratch || !norm_seg || !totals) return -1;
  if (n < 1 || n >= (1LL << 31) || n_chunks < 1 || n_seg < 1 || n_seg > VG_GS_MAX_SEG || n_seg > n_chunks || !(gscale > 0.f) ||
      !(gscale <= 3.402823466e38f))
    return -2;
  if (vg_tel_misaligned(g, 16) || vg_tel_misaligned(totals, 16) || vg_tel_misaligned(scratch, 8)) return -3;
  return vg_grad_stats_launch(g, n, chunks, n_chunks, seg_first, n_seg, gscale, scratch, norm_seg, totals, (hipStream_t)stream);
}
extern "C" int vg_logit_stats(const float* x0, const float* x1, int n, int role, float* out, void* stream) {
  if (!x0 || !out) return -1;
  if (n < 1 || n > VG_LS_MAX_N || role < 0 || role > 2 || (x1 && role > 1)) return -2;
  if (vg_tel_misaligned(out, 16)) return -3;
  return vg_logit_stats_launch(x0, x1, n, role, out, (hipStream_t)stream);
}
extern "C" int vg_telemetry_commit(const VgTelemetrySrc* src, const int* step_dev, int cap, int* ring_step, float* ring, float* ring_seg_d,
                                   float* ring_seg_g, void* stream) {
  if (!src || !step_dev || !ring_step || !ring) return -1;
  if ((src->seg_d && !ring_seg_d) || (src->seg_g && !ring_seg_g)) return -1;
  if (cap < 1 || src->n_seg_d < 0 || src->n_seg_g < 0 || (src->penalty_due != 0 && src->penalty_due != 1)) return -2;
  if ((src->seg_d && src->n_seg_d < 1) || (src->seg_g && src->n_seg_g < 1)) return -3;
  return vg_telemetry_commit_launch(src, step_dev, cap, ring_step, ring, ring_seg_d, ring_seg_g, (hipStream_t)stream);
}
