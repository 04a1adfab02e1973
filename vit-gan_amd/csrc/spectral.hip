// Spectral normalisation of a set of weight matrices inside one flat parameter buffer (include/vitgan_hip.h: vg_spectral_*).
//
//   update  (3 launches for the whole table):  t = W^T u ; v = t / |t| ; w = W v ; sigma = |w| ; u = w / sigma ;
//                                              shadow = bf16(fp32(sigma0 / sigma) * W)
//   project (2 launches):                      G <- s (G - (<G, W> / sigma) u v^T),  s = sigma0 / sigma
//
// Every launch is a grid over (matrix, tile) work items found by a binary search in the device table; the kernel boundary is
// the only synchronisation.  All sums are fp32 fma chains in a fixed order followed by fixed trees (no atomics), norms that
// several workgroups need are recomputed by each of them with the same instruction sequence, so every workgroup holds the
// same bits and two runs are bit-equal.  Nothing is zero-filled: every scratch word is written before it is read.
#include "vg_kernels.h"
#include "vg_spectral.h"

#define SPEC_THREADS 256
#define SPEC_EPS 1e-12f

// ------------------------------------------------------------------------------------------ helpers
template <int WHICH>  // 0: blk_a (column tiles), 1: blk_b (row tiles), 2: blk_c (element chunks)
__device__ __forceinline__ int spec_first(const VgSpectralDesc& d) { return WHICH == 0 ? d.blk_a : WHICH == 1 ? d.blk_b : d.blk_c; }

// the matrix whose work items contain block b: the last entry with first block <= b (entries are in ascending block order)
template <int WHICH>
__device__ __forceinline__ int spec_find(const VgSpectralDesc* __restrict__ tab, int n, int b) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (spec_first<WHICH>(tab[mid]) <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// sum over the workgroup, the same bits in every thread: butterfly inside each wave, then the four wave sums in wave order
__device__ __forceinline__ float spec_block_sum(float v, float* red) {
  v = vg_wave_sum(v);
  __syncthreads();  // red may still be read from an earlier call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// |x|_2 of x[0..n): thread i takes x[i], x[i + 256], ... as one fma chain
__device__ __forceinline__ float spec_norm(const float* __restrict__ x, int n, float* red) {
  float a = 0.f;
  for (int i = threadIdx.x; i < n; i += SPEC_THREADS) { const float q = x[i]; a = fmaf(q, q, a); }
  return sqrtf(spec_block_sum(a, red));
}

__device__ __forceinline__ f32x4 spec_load4(const float* __restrict__ p, long long i, int valid, bool vec) {
  if (vec && valid >= 4) return *reinterpret_cast<const f32x4*>(p + i);
  f32x4 r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) if (j < valid) r[j] = p[i + j];
  return r;
}

// ------------------------------------------------------------------------------------------ update 1: t = W^T u
// A workgroup takes 64 columns: 16 lanes x 4 columns across, 16 row slots down (a wave reads four 256-byte row segments per
// step).  Thread (slot, lane) sums rows slot, slot + 16, ... as an fma chain; the 16 slot sums are added in slot order.
__global__ __launch_bounds__(SPEC_THREADS) void spec_wtu_kernel(const float* __restrict__ W, const float* __restrict__ state,
                                                                float* __restrict__ scratch, const VgSpectralDesc* __restrict__ tab, int n) {
  __shared__ float part[16][VG_SPEC_COLS];
  const VgSpectralDesc d = tab[spec_find<0>(tab, n, blockIdx.x)];
  const int tile = blockIdx.x - d.blk_a, N = d.N, K = d.K;
  const int cl = threadIdx.x & 15, rs = threadIdx.x >> 4;
  const int k0 = tile * VG_SPEC_COLS + cl * 4;
  const int valid = K - k0;  // columns of this thread inside the matrix (<= 0: none)
  const bool vec = ((d.w_off | (long long)K) & 3) == 0;
  const float* __restrict__ Wm = W + d.w_off;
  const float* __restrict__ u = state + d.u_off;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (valid > 0) {
    for (int r = rs; r < N; r += 16) {
      const float ur = u[r];
      const f32x4 w = spec_load4(Wm, (long long)r * K + k0, valid, vec);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = fmaf(w[j], ur, acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) part[rs][cl * 4 + j] = acc[j];
  __syncthreads();
  if (threadIdx.x < VG_SPEC_COLS) {
    const int k = tile * VG_SPEC_COLS + threadIdx.x;
    if (k < K) {
      float s = part[0][threadIdx.x];
#pragma unroll
      for (int r = 1; r < 16; ++r) s += part[r][threadIdx.x];
      scratch[d.t_off + k] = s;
    }
  }
}

// ------------------------------------------------------------------------------------------ update 2: v = t / |t| ; w = W v
// A workgroup takes 16 rows, a wave four of them one after the other: lane l sums columns 4l .. 4l+3, 4l+256 .. as one fma
// chain, then the butterfly.  Every workgroup of a matrix forms |t| itself; the one with the first rows stores v.
__global__ __launch_bounds__(SPEC_THREADS) void spec_wv_kernel(const float* __restrict__ W, float* __restrict__ state, float* __restrict__ scratch,
                                                               const VgSpectralDesc* __restrict__ tab, int n) {
  __shared__ float red[4];
  const VgSpectralDesc d = tab[spec_find<1>(tab, n, blockIdx.x)];
  const int tile = blockIdx.x - d.blk_b, N = d.N, K = d.K;
  const float* __restrict__ t = scratch + d.t_off;
  const float inv = 1.0f / fmaxf(spec_norm(t, K, red), SPEC_EPS);
  if (tile == 0) {
    float* __restrict__ v = state + d.v_off;
    for (int k = threadIdx.x; k < K; k += SPEC_THREADS) v[k] = t[k] * inv;
  }
  const bool vec = ((d.w_off | (long long)K) & 3) == 0;           // rows of W start on 16 bytes
  const bool tvec = (K & 3) == 0;                                  // t does (t_off % 4 == 0 by the plan)
  const float* __restrict__ Wm = W + d.w_off;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = 0; i < 4; ++i) {
    const int r = tile * VG_SPEC_ROWS + wave * 4 + i;  // wave-uniform
    if (r >= N) break;
    float a = 0.f;
    for (int k = lane * 4; k < K; k += 256) {
      const f32x4 w = spec_load4(Wm, (long long)r * K + k, K - k, vec);
      const f32x4 tv = spec_load4(t, k, K - k, tvec);
#pragma unroll
      for (int j = 0; j < 4; ++j) a = fmaf(w[j], tv[j] * inv, a);  // (columns past K: w = t = 0)
    }
    a = vg_wave_sum(a);
    if (lane == 0) scratch[d.w_tmp_off + r] = a;
  }
}

// ------------------------------------------------------------------------------------------ update 3: sigma, u, the scaled cast
// A workgroup takes VG_SPEC_CHUNK consecutive elements of one matrix.  iterate: sigma = |w| (formed by every workgroup), the first
// chunk's workgroup stores u and sigma; otherwise sigma is the stored one.
__global__ __launch_bounds__(SPEC_THREADS) void spec_cast_kernel(const float* __restrict__ W, bf16* __restrict__ shadow, float* __restrict__ state,
                                                                 const float* __restrict__ scratch, const VgSpectralDesc* __restrict__ tab, int n,
                                                                 int iterate) {
  __shared__ float red[4];
  const VgSpectralDesc d = tab[spec_find<2>(tab, n, blockIdx.x)];
  const int chunk = blockIdx.x - d.blk_c;
  const long long NK = (long long)d.N * d.K;
  float sigma;
  if (iterate) {
    const float* __restrict__ w = scratch + d.w_tmp_off;
    sigma = spec_norm(w, d.N, red);
    if (chunk == 0) {
      const float inv = 1.0f / fmaxf(sigma, SPEC_EPS);
      float* __restrict__ u = state + d.u_off;
      for (int r = threadIdx.x; r < d.N; r += SPEC_THREADS) u[r] = w[r] * inv;
      if (threadIdx.x == 0) state[d.s_off] = sigma;
    }
  } else {
    sigma = state[d.s_off];
  }
  const float s = state[d.s_off + 1] / fmaxf(sigma, SPEC_EPS);
  const bool vec = (d.w_off & 3) == 0;
  const float* __restrict__ Wm = W + d.w_off;
  bf16* __restrict__ out = shadow + d.w_off;
  const long long e0 = (long long)chunk * VG_SPEC_CHUNK;
#pragma unroll 2
  for (int it = 0; it < VG_SPEC_CHUNK / (4 * SPEC_THREADS); ++it) {
    const long long e = e0 + (long long)(it * SPEC_THREADS + threadIdx.x) * 4;
    if (e >= NK) break;
    const int valid = (int)(NK - e < 4 ? NK - e : 4);
    const f32x4 w = spec_load4(Wm, e, valid, vec);
    if (vec && valid == 4) {
      bf16x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = vg_f2bf(s * w[j]);
      *reinterpret_cast<bf16x4*>(out + e) = o;
    } else {
      for (int j = 0; j < valid; ++j) out[e + j] = vg_f2bf(s * w[j]);
    }
  }
}

// ------------------------------------------------------------------------------------------ project 1: partial <G, W>
__global__ __launch_bounds__(SPEC_THREADS) void spec_dot_kernel(const float* __restrict__ G, const float* __restrict__ W, float* __restrict__ scratch,
                                                                const VgSpectralDesc* __restrict__ tab, int n) {
  __shared__ float red[4];
  const VgSpectralDesc d = tab[spec_find<2>(tab, n, blockIdx.x)];
  const int chunk = blockIdx.x - d.blk_c;
  const long long NK = (long long)d.N * d.K;
  const bool vec = (d.w_off & 3) == 0;
  const float* __restrict__ Wm = W + d.w_off;
  const float* __restrict__ Gm = G + d.w_off;
  const long long e0 = (long long)chunk * VG_SPEC_CHUNK;
  float a = 0.f;
#pragma unroll 2
  for (int it = 0; it < VG_SPEC_CHUNK / (4 * SPEC_THREADS); ++it) {
    const long long e = e0 + (long long)(it * SPEC_THREADS + threadIdx.x) * 4;
    if (e >= NK) break;
    const int valid = (int)(NK - e < 4 ? NK - e : 4);
    const f32x4 w = spec_load4(Wm, e, valid, vec), g = spec_load4(Gm, e, valid, vec);
#pragma unroll
    for (int j = 0; j < 4; ++j) a = fmaf(g[j], w[j], a);
  }
  a = spec_block_sum(a, red);
  if (threadIdx.x == 0) scratch[d.dot_off + chunk] = a;
}

// ------------------------------------------------------------------------------------------ project 2: G <- s (G - c u v^T)
__global__ __launch_bounds__(SPEC_THREADS) void spec_proj_kernel(float* __restrict__ G, const float* __restrict__ state, const float* __restrict__ scratch,
                                                                 const VgSpectralDesc* __restrict__ tab, int n) {
  const VgSpectralDesc d = tab[spec_find<2>(tab, n, blockIdx.x)];
  const int chunk = blockIdx.x - d.blk_c, K = d.K;
  const long long NK = (long long)d.N * K;
  const int nchunk = (int)((NK + VG_SPEC_CHUNK - 1) / VG_SPEC_CHUNK);
  float dot = scratch[d.dot_off];
  for (int c = 1; c < nchunk; ++c) dot += scratch[d.dot_off + c];  // chunk order; wave-uniform loads
  const float sigma = fmaxf(state[d.s_off], SPEC_EPS);
  const float coef = dot / sigma, s = state[d.s_off + 1] / sigma;
  const float* __restrict__ u = state + d.u_off;
  const float* __restrict__ v = state + d.v_off;
  const bool vec = ((d.w_off | (long long)K) & 3) == 0;  // four elements then share one row, and v's four are 16-byte aligned
  float* __restrict__ Gm = G + d.w_off;
  const long long e0 = (long long)chunk * VG_SPEC_CHUNK;
#pragma unroll 2
  for (int it = 0; it < VG_SPEC_CHUNK / (4 * SPEC_THREADS); ++it) {
    const long long e = e0 + (long long)(it * SPEC_THREADS + threadIdx.x) * 4;
    if (e >= NK) break;
    if (vec) {  // NK % 4 == 0 here
      const int r = (int)(e / K), k = (int)(e - (long long)r * K);
      const float cu = coef * u[r];
      f32x4 g = *reinterpret_cast<const f32x4*>(Gm + e);
      const f32x4 vv = *reinterpret_cast<const f32x4*>(v + k);
#pragma unroll
      for (int j = 0; j < 4; ++j) g[j] = s * fmaf(-cu, vv[j], g[j]);
      *reinterpret_cast<f32x4*>(Gm + e) = g;
    } else {
      const int valid = (int)(NK - e < 4 ? NK - e : 4);
      for (int j = 0; j < valid; ++j) {
        const int r = (int)((e + j) / K), k = (int)(e + j - (long long)r * K);
        Gm[e + j] = s * fmaf(-(coef * u[r]), v[k], Gm[e + j]);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ host: the plan and the launches
static inline long long up4(long long x) { return (x + 3) & ~3LL; }

int vg_spectral_plan_host(VgSpectralDesc* tab, int n, long long* state_floats, long long* scratch_floats, int* blocks) {
  long long so = 0, sc = 0, ba = 0, bb = 0, bc = 0;
  for (int i = 0; i < n; ++i) {
    VgSpectralDesc& d = tab[i];
    if (d.N < 1 || d.K < 1 || d.w_off < 0) return -2;
    const long long NK = (long long)d.N * d.K;
    const long long nchunk = (NK + VG_SPEC_CHUNK - 1) / VG_SPEC_CHUNK;
    d.u_off = so; so += up4(d.N);
    d.v_off = so; so += up4(d.K);
    d.s_off = so; so += 4;  // sigma, sigma0, two spare words: every offset stays a multiple of 4 floats
    d.t_off = sc; sc += up4(d.K);
    d.w_tmp_off = sc; sc += up4(d.N);
    d.dot_off = sc; sc += up4(nchunk);
    if (ba > 0x3fffffff || bb > 0x3fffffff || bc > 0x3fffffff) return -2;
    d.blk_a = (int)ba; ba += (d.K + VG_SPEC_COLS - 1) / VG_SPEC_COLS;
    d.blk_b = (int)bb; bb += (d.N + VG_SPEC_ROWS - 1) / VG_SPEC_ROWS;
    d.blk_c = (int)bc; bc += nchunk;
    d.reserved = 0;
  }
  if (ba > 0x3fffffff || bb > 0x3fffffff || bc > 0x3fffffff) return -2;
  if (state_floats) *state_floats = so;
  if (scratch_floats) *scratch_floats = sc;
  if (blocks) { blocks[0] = (int)ba; blocks[1] = (int)bb; blocks[2] = (int)bc; }
  return 0;
}

int vg_spectral_update_launch(const float* W, bf16* shadow, float* state, float* scratch, const VgSpectralDesc* tab_dev, int n, const int* blocks,
                              int iterate, hipStream_t st) {
  if (iterate) {
    hipLaunchKernelGGL(spec_wtu_kernel, dim3(blocks[0]), dim3(SPEC_THREADS), 0, st, W, (const float*)state, scratch, tab_dev, n);
    hipLaunchKernelGGL(spec_wv_kernel, dim3(blocks[1]), dim3(SPEC_THREADS), 0, st, W, state, scratch, tab_dev, n);
  }
  hipLaunchKernelGGL(spec_cast_kernel, dim3(blocks[2]), dim3(SPEC_THREADS), 0, st, W, shadow, state, (const float*)scratch, tab_dev, n, iterate);
  VG_CHECK_HIP(hipGetLastError());
  return 0;
}

int vg_spectral_project_launch(float* G, const float* W, const float* state, float* scratch, const VgSpectralDesc* tab_dev, int n, const int* blocks,
                               hipStream_t st) {
  hipLaunchKernelGGL(spec_dot_kernel, dim3(blocks[2]), dim3(SPEC_THREADS), 0, st, (const float*)G, W, scratch, tab_dev, n);
  hipLaunchKernelGGL(spec_proj_kernel, dim3(blocks[2]), dim3(SPEC_THREADS), 0, st, G, state, (const float*)scratch, tab_dev, n);
  VG_CHECK_HIP(hipGetLastError());
  return 0;
}
