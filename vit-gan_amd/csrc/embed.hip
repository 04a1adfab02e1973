// The two ends of the discriminator around its encoder blocks, for the C1-C3 geometry (E = 384, 4 x 4 patches, K = 16 C <= 64):
// the patch embedding with block 0's LayerNorm as ONE launch, and its backward as one launch per side (image / parameters) plus one
// fold.  gfx950 only.
//
// Why: the contraction of the embedding is 48 deep and its dominant tensor a single [M, 384] activation, so the tiled GEMM ran one
// k-step under a full prologue and epilogue, X[0] went through HBM twice more for the CLS fill and the LayerNorm, and the backward
// read dL/dX[0] three times and copied it once only to drop the CLS rows (vg_take_rows) in front of a 96-workgroup split-K launch.
//
//   vg_embed_fwd_kernel    image -> Apatch, X[0], xn1[0], mean1[0], rstd1[0].  A workgroup owns 32 whole rows of the [B S, 384]
//                          token matrix (CLS rows included): its 8 waves sit side by side along n, 48 columns each, with their slice
//                          of conv_w in registers as MFMA fragments (k = 0..31, then 32..63 zero-padded beyond K: the k order of the
//                          tiled GEMM, so X[0] keeps its bits); the image is gathered straight into the other operand.  The epilogue
//                          rounds (acc + bias + pos) * mask - or cls * mask - to bf16 ONCE into an LDS tile; the tile is re-read
//                          row-wise, 16 lanes per row, by the statistics arithmetic of norm.hip (vg_ln_fwd_kernel), so every global
//                          store is a whole 768-byte row in 16-byte pieces.
//   vg_embed_dimg_kernel   d image = un-patchify(g_patch conv_w), bf16 NCHW.  A wave owns 16 patch rows and reads them IN PLACE from
//                          dL/dX[0] (rows 1..S-1 of each image); conv_w sits row-major in LDS and is consumed transposed
//                          (ds_read_b64_tr_b16).  A lane ends up with the 4 pixels of one (c, py) line of its patch: 8-byte stores.
//   vg_embed_wgrad_kernel  two kinds of workgroup in one launch.  (K slice, 64 columns): contracts that slice of the patch rows of g -
//                          read IN PLACE, rows 1..S-1 of each image - with the same rows of Apatch on the MFMA pipe into slab[slice] (both
//                          staged row-major, read transposed): the slices, 32-row k-steps and operand order of the split-K GEMM it
//                          replaces, so d conv_w keeps its bits, on twice the workgroups and without the gathered copy.  (token position
//                          s, 64 columns): tok_sum[s] = sum_b g[b, s, :] in vg_batch_sum_kernel's order (d cls, d pos, the terms of
//                          d conv_b).  No atomics: vg_embed_fold_kernel adds the slices and tok_sum into the gradient buffer in the
//                          order of the two folds it replaces.
//
// A row of the token matrix lands in different tiles depending on the batch it is part of; its bits must not (per-sample
// bit-independence, tests/test_fullsize_gpu.py).  As in gemm_row.hip, contraction is therefore OFF in this file and every fused
// multiply-add is written as fmaf().
#include "vg_kernels.h"
#pragma clang fp contract(off)

namespace {
constexpr int EM_E = 384;            // embedding width
constexpr int EM_TS = 2 * EM_E + 16; // forward: byte stride of a row of the bf16 epilogue tile
constexpr int EM_GS = 128 + 16;      // wgrad: byte stride of a staged row of 64 gradient columns

__device__ __forceinline__ float em_row16_sum(float v) {  // sum over the 16 lanes of a row group (norm.hip's order)
  v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 1, 64);
  return v;
}
__device__ __forceinline__ bf16x4 em_ld4(const float* p) {
  const f32x4 t = *(const f32x4*)p;
  return (bf16x4){vg_f2bf(t[0]), vg_f2bf(t[1]), vg_f2bf(t[2]), vg_f2bf(t[3])};
}
__device__ __forceinline__ bf16x4 em_ld4(const bf16* p) { return *(const bf16x4*)p; }
// fragment A[row = column i of the LDS image][k = 8 g + j] from rows 8 g .. 8 g + 7 of a row-major [k][columns] image at `base`
// (`base` already points at row 8 g + q, columns 4 p of the wanted 16: lane 4 q + p of its group)
__device__ __forceinline__ bf16x8 em_tr_frag(const unsigned char* base, int row_stride) {
  const bf16x4 lo = vg_lds_tr_read(base), hi = vg_lds_tr_read(base + 4 * row_stride);
  return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

}  // namespace

// (the kernels have external names: a trace shows them as vg_embed_*_kernel)
// ------------------------------------------------------------------------------------------------------------------------
template <typename T, int C>
__global__ __launch_bounds__(512, 4) void vg_embed_fwd_kernel(const T* __restrict__ img, const bf16* __restrict__ W, const float* __restrict__ bias,
                                                              const float* __restrict__ pos, const float* __restrict__ cls,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              bf16* __restrict__ Apatch, bf16* __restrict__ X, bf16* __restrict__ Xn,
                                                              float* __restrict__ mean, float* __restrict__ rstd, int B, int IH, float eps,
                                                              unsigned dthr, unsigned dkey0, float dscale, const unsigned* __restrict__ dstep) {
  constexpr int K = 16 * C, E = EM_E;
  __shared__ __attribute__((aligned(16))) unsigned char tile[32 * EM_TS + 3 * EM_E * 4];
  float* const gb = (float*)(tile + 32 * EM_TS);  // gamma | beta | bias: read from LDS per tile (hoisted out of the tile loop they cost 60 registers)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4, li = lane & 15;
  const int G = IH >> 2, NP = G * G, S = NP + 1, M = B * S;
  if (threadIdx.x < E) { gb[threadIdx.x] = gamma[threadIdx.x]; gb[E + threadIdx.x] = beta[threadIdx.x]; gb[2 * E + threadIdx.x] = bias[threadIdx.x]; }
  __syncthreads();
  const unsigned dkey = vg_drop_key(dkey0, dstep);
  // this wave's 48 columns of conv_w [E, K] as fragments: A[row = n][k = 32 ks + 8 g + j], zero beyond K
  bf16x8 wf[3][2];
#pragma unroll
  for (int nt = 0; nt < 3; ++nt) {
    const int n = wv * 48 + 16 * nt + li;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int k = 32 * ks + 8 * g;
      bf16x8 t = {0, 0, 0, 0, 0, 0, 0, 0};
      if (k < K) t = *(const bf16x8*)(W + (size_t)n * K + k);
      wf[nt][ks] = t;
    }
  }
  const int ntiles = (M + 31) >> 5;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    // every global load of the tile - the image of both m-tiles, their addend rows - goes out before the first product waits for one
    bf16x8 pf[2][2];
    f32x4 ad[2][3];
    bool pt[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int r = t * 32 + 16 * mt + li;  // the row this lane gathers (operand column li) AND finishes (accumulator column li)
      const int b = r / S, s = r - b * S;
      const bool patch = r < M && s > 0;
      const int p = s - 1, gy = p / G, gx = p - gy * G;
      pt[mt] = patch;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x4 h2[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {  // k = 32 ks + 8 g + 4 h + px  <->  (c, py) = cp >> 2, cp & 3
          const int cp = 8 * ks + 2 * g + h;
          bf16x4 v = {0, 0, 0, 0};
          if (patch && cp < 4 * C) v = em_ld4(img + (((size_t)b * C + (cp >> 2)) * IH + gy * 4 + (cp & 3)) * IH + gx * 4);
          h2[h] = v;
        }
        pf[mt][ks] = (bf16x8){h2[0][0], h2[0][1], h2[0][2], h2[0][3], h2[1][0], h2[1][1], h2[1][2], h2[1][3]};
      }
      const float* arow = patch ? pos + (size_t)p * E : cls;  // the row's fp32 addend: its position, or the CLS token itself
#pragma unroll
      for (int nt = 0; nt < 3; ++nt) ad[mt][nt] = *(const f32x4*)(arow + wv * 48 + 16 * nt + 4 * g);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        if (wv == 0 && patch && 32 * ks + 8 * g < K) *(bf16x8*)(Apatch + ((size_t)b * NP + p) * K + 32 * ks + 8 * g) = pf[mt][ks];
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int r = t * 32 + 16 * mt + li;
#pragma unroll
      for (int nt = 0; nt < 3; ++nt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = vg_mfma(wf[nt][0], pf[mt][0], acc);
        acc = vg_mfma(wf[nt][1], pf[mt][1], acc);
        // accumulator: row r, columns n .. n + 3
        const int n = wv * 48 + 16 * nt + 4 * g;
        f32x4 v = acc + *(const f32x4*)(gb + 2 * E + n);
        if (pt[mt]) v += ad[mt][nt];
        else v = ad[mt][nt];
        if (dthr) {  // dropout site 0 after every addend; element index of the full [B S, E] tensor
          const unsigned wd = vg_drop_word(dkey, ((unsigned)r * (unsigned)E + (unsigned)n) >> 2);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] *= vg_drop_factor(wd, j, dthr, dscale);
        }
        *(bf16x4*)(tile + (16 * mt + li) * EM_TS + 2 * n) = (bf16x4){vg_f2bf(v[0]), vg_f2bf(v[1]), vg_f2bf(v[2]), vg_f2bf(v[3])};
      }
    }
    __syncthreads();
    {  // row-wise: 16 lanes per row, lane `sub` owns the 16-byte chunks sub, sub + 16, sub + 32 (vg_ln_fwd_kernel's layout and order)
      const int rl = 4 * wv + g, sub = li;
      const int row = t * 32 + rl;
      const bool ok = row < M;
      float v[3][8];
      float sm = 0.f;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const bf16x8 o = *(const bf16x8*)(tile + rl * EM_TS + 16 * (sub + 16 * i));
        if (ok) *(bf16x8*)(X + (size_t)row * E + 8 * (sub + 16 * i)) = o;
#pragma unroll
        for (int j = 0; j < 8; ++j) { v[i][j] = vg_bf2f(o[j]); sm += v[i][j]; }
      }
      const float mu = em_row16_sum(sm) * (1.0f / E);
      float q = 0.f;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float c = v[i][j] - mu; q += c * c; }  // unfused, as norm.hip's build has it
      const float rs = rsqrtf(fmaf(em_row16_sum(q), 1.0f / E, eps));  // norm.hip's contracted form
      if (ok) {
        if (sub == 0) { mean[row] = mu; rstd[row] = rs; }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const int c = 8 * (sub + 16 * i);
          const f32x4 g0 = *(const f32x4*)(gb + c), g1 = *(const f32x4*)(gb + c + 4);
          const f32x4 b0 = *(const f32x4*)(gb + E + c), b1 = *(const f32x4*)(gb + E + c + 4);
          bf16x8 o;
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = vg_f2bf(fmaf((v[i][j] - mu) * rs, j < 4 ? g0[j] : g1[j - 4], j < 4 ? b0[j] : b1[j - 4]));
          *(bf16x8*)(Xn + (size_t)row * E + c) = o;
        }
      }
    }
    __syncthreads();  // the tile is rewritten by the next round
  }
}

// ------------------------------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256, 2) void vg_embed_dimg_kernel(const bf16* __restrict__ gX, const bf16* __restrict__ W, bf16* __restrict__ dimg,
                                                               int B, int IH) {
  constexpr int K = 16 * C, E = EM_E, RS = 2 * K + 16;  // conv_w [E, K] row-major in LDS, rows RS bytes apart
  __shared__ __attribute__((aligned(16))) unsigned char wl[E * RS];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, li = lane & 15;
  const int G = IH >> 2, NP = G * G, S = NP + 1, Mp = B * NP;
  for (int i = threadIdx.x; i < E * (K / 8); i += 256) {
    const int e = i / (K / 8), c = i - e * (K / 8);
    *(u32x4*)(wl + e * RS + 16 * c) = *(const u32x4*)(W + (size_t)e * K + 8 * c);
  }
  __syncthreads();
  const int nwt = (Mp + 15) >> 4;
  const unsigned char* wbase = wl + (8 * g + (li >> 2)) * RS + 8 * (li & 3);
  for (int wt = blockIdx.x * 4 + wv; wt < nwt; wt += gridDim.x * 4) {  // (wave-uniform trip count: the transposed reads need every lane)
    const int m = wt * 16 + li;
    const int mc = m < Mp ? m : Mp - 1;
    const int b = mc / NP, p = mc - b * NP;
    const bf16* gr = gX + ((size_t)b * S + 1 + p) * E + 8 * g;  // patch row p of image b is row 1 + p of its S rows
    bf16x8 gf[12];
#pragma unroll
    for (int ks = 0; ks < 12; ++ks) gf[ks] = *(const bf16x8*)(gr + 32 * ks);
    f32x4 acc[C];
#pragma unroll
    for (int kt = 0; kt < C; ++kt) acc[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 12; ++ks)
#pragma unroll
      for (int kt = 0; kt < C; ++kt)  // A[row = k index 16 kt + li][e = 32 ks + 8 g + j] = conv_w[e][k], B[e][col = row m] = g
        acc[kt] = vg_mfma(em_tr_frag(wbase + 32 * ks * RS + 32 * kt, RS), gf[ks], acc[kt]);
    if (m < Mp) {  // accumulator: row m, k = 16 kt + 4 g + reg  <->  channel kt, line py = g, pixels px = reg
      const int gy = p / G, gx = p - gy * G;
#pragma unroll
      for (int kt = 0; kt < C; ++kt)
        *(bf16x4*)(dimg + (((size_t)b * C + kt) * IH + gy * 4 + g) * IH + gx * 4) =
            (bf16x4){vg_f2bf(acc[kt][0]), vg_f2bf(acc[kt][1]), vg_f2bf(acc[kt][2]), vg_f2bf(acc[kt][3])};
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256, 2) void vg_embed_wgrad_kernel(const bf16* __restrict__ gX, const bf16* __restrict__ Apatch, float* __restrict__ slab,
                                                                float* __restrict__ tok_sum, int B, int S, int nmm, int kps) {
  constexpr int K = 16 * C, E = EM_E, KC = K / 8, AS = 2 * K + 16, GS = EM_GS;
  constexpr int NA = (128 * KC + 255) / 256;  // 16-byte pieces of a 128-row Apatch stage per thread
  __shared__ __attribute__((aligned(16))) unsigned char smem[128 * GS + 128 * AS];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= nmm) {
    // ---- the sums over the batch: tok_sum[s, e] = sum_b g[b, s, e], vg_batch_sum_kernel's workgroups, lanes and order ----
    float (*red)[65] = (float (*)[65])smem;
    const int bx = blockIdx.x - nmm;
    const int cl = tid & 7, bl = tid >> 3;  // 8 chunks of 8 columns, 32 batch lanes
    const int chunks = E / 64;
    const int s = bx / chunks, e0 = (bx - s * chunks) * 64 + 8 * cl;
    float a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = 0.f;
    const bf16* p = gX + (size_t)s * E + e0;
    const size_t bstride = (size_t)S * E;
    int b = bl;
    for (; b + 96 < B; b += 128) {
      bf16x8 t[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) t[u] = *(const bf16x8*)(p + (size_t)(b + 32 * u) * bstride);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] += vg_bf2f(t[u][j]);
    }
    for (; b < B; b += 32) {
      const bf16x8 t = *(const bf16x8*)(p + (size_t)b * bstride);
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] += vg_bf2f(t[j]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) red[bl][8 * cl + j] = a[j];
    __syncthreads();
    if (tid < 64) {
      float r = 0.f;
#pragma unroll
      for (int k = 0; k < 32; ++k) r += red[k][tid];
      tok_sum[(size_t)s * E + (bx - s * chunks) * 64 + tid] = r;
    }
    return;
  }
  // ---- d conv_w: K slice `split` of the patch rows x 64 columns of g, the split-K GEMM's slices, k-steps and operand order ----
  unsigned char* const gt = smem;              // [128 patch rows][64 columns of g]
  unsigned char* const at = smem + 128 * GS;   // [128 patch rows][K]
  const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, li = lane & 15;
  const int split = blockIdx.x / 6, e0 = (blockIdx.x - split * 6) * 64, NP = S - 1, Mp = B * NP;
  const int k_begin = split * kps, k_end = min(Mp, k_begin + kps);
  const int grow = tid >> 3, gch = tid & 7;
  u32x4 rg[4], ra[NA];
  auto fetch = [&](int m0) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int m = m0 + grow + 32 * u;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (m < k_end) {  // patch row p of image b is row 1 + p of its S rows: dL/dX[0] read in place
        const int b = m / NP, pp = m - b * NP;
        v = *(const u32x4*)(gX + ((size_t)b * S + 1 + pp) * E + e0 + 8 * gch);
      }
      rg[u] = v;
    }
#pragma unroll
    for (int u = 0; u < NA; ++u) {
      const int i = tid + 256 * u, row = i / KC, ch = i - row * KC, m = m0 + row;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (i < 128 * KC && m < k_end) v = *(const u32x4*)(Apatch + (size_t)m * K + 8 * ch);
      ra[u] = v;
    }
  };
  f32x4 acc[C];
#pragma unroll
  for (int kt = 0; kt < C; ++kt) acc[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const unsigned char* gbase = gt + (8 * g + (li >> 2)) * GS + 2 * (16 * wv + 4 * (li & 3));
  const unsigned char* abase = at + (8 * g + (li >> 2)) * AS + 8 * (li & 3);
  fetch(k_begin);
  for (int m0 = k_begin; m0 < k_end; m0 += 128) {
    __syncthreads();  // the previous stage has been consumed
#pragma unroll
    for (int u = 0; u < 4; ++u) *(u32x4*)(gt + (grow + 32 * u) * GS + 16 * gch) = rg[u];
#pragma unroll
    for (int u = 0; u < NA; ++u) {
      const int i = tid + 256 * u, row = i / KC, ch = i - row * KC;
      if (i < 128 * KC) *(u32x4*)(at + row * AS + 16 * ch) = ra[u];
    }
    __syncthreads();
    if (m0 + 128 < k_end) fetch(m0 + 128);  // in flight under the products below
    const int nk = min(4, (k_end - m0 + 31) >> 5);  // k-steps of 32 rows with anything in them (workgroup-uniform; rows beyond k_end are zero)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {  // A[row = k index][32 patch rows], B[32 patch rows][col = column of g]
      if (kk < nk) {
        const bf16x8 gf = em_tr_frag(gbase + 32 * kk * GS, GS);
#pragma unroll
        for (int kt = 0; kt < C; ++kt) acc[kt] = vg_mfma(em_tr_frag(abase + 32 * kk * AS + 32 * kt, AS), gf, acc[kt]);
      }
    }
  }
  // accumulator: column e0 + 16 wv + li of g, k = 16 kt + 4 g + reg
  float* dst = slab + ((size_t)split * E + e0 + 16 * wv + li) * K + 4 * g;
#pragma unroll
  for (int kt = 0; kt < C; ++kt) *(f32x4*)(dst + 16 * kt) = acc[kt];
}

// d conv_w += the K slices in slice order (vg_slab_reduce_kernel's order, the gradient first); d cls += tok_sum[0]; d pos += tok_sum[1:];
// d conv_b += sum_n tok_sum[1 + n] (vg_embed_small_grads_kernel's)
__global__ __launch_bounds__(256) void vg_embed_fold_kernel(const float* __restrict__ slab, int nslab, const float* __restrict__ tok_sum,
                                                            float* __restrict__ d_w, float* __restrict__ d_cls, float* __restrict__ d_pos,
                                                            float* __restrict__ d_bias, int S, int E, int K) {
  const int i = blockIdx.x * 256 + threadIdx.x, nw = E * K;
  if (i < nw) {
    float a = d_w[i];
#pragma unroll 8
    for (int n = 0; n < nslab; ++n) a += slab[(size_t)n * nw + i];
    d_w[i] = a;
    return;
  }
  const int j = i - nw;
  if (j >= S * E) return;
  const float t = tok_sum[j];
  if (j < E) d_cls[j] += t; else d_pos[j - E] += t;
  if (j < E) {
    float a = 0.f;
#pragma unroll 8
    for (int n = 1; n < S; ++n) a += tok_sum[(size_t)n * E + j];
    d_bias[j] += a;
  }
}

// The geometry these kernels are written for: E = 384, 4 x 4 patches, at most 4 channels (K = 16 C <= 64) - C1, C2, C3.
int vg_embed_fused_ok(int C, int IH, int P, int E) { return E == EM_E && P == 4 && C >= 1 && C <= 4 && IH >= 4 && IH % 4 == 0; }

#define EM_BY_C(CALL) \
  switch (C) { case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break; default: return -3; }

int vg_embed_fwd_launch(const void* img, int img_is_bf16, const bf16* W, const float* bias, const float* pos, const float* cls, const float* gamma,
                        const float* beta, bf16* Apatch, bf16* X, bf16* Xn, float* mean, float* rstd, int B, int C, int IH, float eps, VgDrop drop,
                        hipStream_t st) {
  if (!vg_embed_fused_ok(C, IH, 4, EM_E) || B < 1) return -3;
  const long long M = (long long)B * ((IH / 4) * (IH / 4) + 1);
  if (M * EM_E >= (1LL << 31)) return -3;  // dropout indices and row arithmetic are 32-bit
  const int ntiles = (int)((M + 31) / 32), grid = ntiles < 512 ? ntiles : 512;
#define EM_FWD(C_)                                                                                                                           \
  if (img_is_bf16) hipLaunchKernelGGL((vg_embed_fwd_kernel<bf16, C_>), dim3(grid), dim3(512), 0, st, (const bf16*)img, W, bias, pos, cls, gamma, \
                                      beta, Apatch, X, Xn, mean, rstd, B, IH, eps, drop.thr, drop.key, drop.scale, drop.step);              \
  else hipLaunchKernelGGL((vg_embed_fwd_kernel<float, C_>), dim3(grid), dim3(512), 0, st, (const float*)img, W, bias, pos, cls, gamma, beta,  \
                          Apatch, X, Xn, mean, rstd, B, IH, eps, drop.thr, drop.key, drop.scale, drop.step)
  EM_BY_C(EM_FWD)
#undef EM_FWD
  return (int)hipGetLastError();
}

int vg_embed_dimg_launch(const bf16* g, const bf16* W, bf16* dimg, int B, int C, int IH, hipStream_t st) {
  if (!vg_embed_fused_ok(C, IH, 4, EM_E) || B < 1) return -3;
  const long long Mp = (long long)B * (IH / 4) * (IH / 4);
  if ((Mp + B) * EM_E >= (1LL << 31)) return -3;
  const long long nwg = (Mp + 63) / 64;
  const int grid = (int)(nwg < 2048 ? nwg : 2048);
#define EM_DIMG(C_) hipLaunchKernelGGL((vg_embed_dimg_kernel<C_>), dim3(grid), dim3(256), 0, st, g, W, dimg, B, IH)
  EM_BY_C(EM_DIMG)
#undef EM_DIMG
  return (int)hipGetLastError();
}

// splits: the K slices asked for (the split-K launch's request; empty ones are dropped as vg_gemm_launch drops them).  slab: splits * E * K floats,
// tok_sum: S * E floats; both are written whole before the fold reads them
int vg_embed_wgrad_launch(const bf16* g, const bf16* Apatch, float* slab, float* tok_sum, float* d_w, float* d_bias, float* d_pos, float* d_cls, int B,
                          int C, int IH, int splits, hipStream_t st) {
  if (!vg_embed_fused_ok(C, IH, 4, EM_E) || B < 1 || splits < 1) return -3;
  const int NP = (IH / 4) * (IH / 4), S = NP + 1, K = 16 * C;
  if ((long long)B * S * EM_E >= (1LL << 31)) return -3;
  const int ksteps = (B * NP + 31) / 32, per = (ksteps + splits - 1) / splits;  // vg_gemm_launch's partition of the rows
  const int kps = per * 32, nsl = (ksteps + per - 1) / per, nmm = nsl * (EM_E / 64);
#define EM_WG(C_) \
  hipLaunchKernelGGL((vg_embed_wgrad_kernel<C_>), dim3(nmm + S * (EM_E / 64)), dim3(256), 0, st, g, Apatch, slab, tok_sum, B, S, nmm, kps)
  EM_BY_C(EM_WG)
#undef EM_WG
  VG_CHECK_HIP(hipGetLastError());
  const int n = EM_E * K + S * EM_E;
  hipLaunchKernelGGL(vg_embed_fold_kernel, dim3((n + 255) / 256), dim3(256), 0, st, slab, nsl, tok_sum, d_w, d_cls, d_pos, d_bias, S, EM_E, K);
  return (int)hipGetLastError();
}
