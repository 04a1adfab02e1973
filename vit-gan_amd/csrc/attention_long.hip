// Fused multi-head self-attention (forward and backward) for 80 < S <= 256 tokens: the ViT patch grids 9x9 .. 15x15 + CLS (224/16 =
// ViT-B/16: 197 tokens), the patch-grid generator up to 225 tokens and the v1 row generator up to 256 rows.  gfx950 only.
//
// One workgroup per (image, head) owns every key AND every query of the head, so every output element is summed by one wave in a
// fixed order: no float atomics, no hand-off between workgroups, bitwise reproducible run to run.  The conventions are those of
// attention.hip (helpers in vg_attn.h): scores are produced as S^T = K Q^T (a lane owns one query column and 4 consecutive keys of
// a 16-key tile), the exponentiated scores of a 32-key pair are packed to bf16 as the k-operand of the P.V product, and V (K, Q, dO)
// is read transposed from an XOR-swizzled LDS image filled by LDS-DMA.  What changes with S is that no S x S tile is held:
//   forward  - K and V of the head are staged once; each wave walks its query tiles and, per tile, the keys 32 at a time with an
//              online softmax (running max m per query, this lane's share of the sum l, the output accumulator rescaled by
//              exp(m_old - m_new) before each pair's P.V product).  Registers do not grow with S.
//   backward - phase A (lane = query) streams the key pairs of the K and V images and accumulates dQ = dS K; Q and dO are then
//              staged into the SAME two images and phase B (lane = key) streams the query pairs and accumulates dK = dS^T Q and
//              dV = P^T dO.  P and dS are recomputed from the saved lse and delta = rowsum(dO o O) (kept per query in LDS).
// Waves: min(ceil(S / 16), 8) per workgroup, each taking the 16-row tiles wv, wv + nw (at most two).  LDS (dynamic): two images of
// RP x HE bf16, RP = S rounded up to 32 - 53 KB at S = 197, HE = 64; 96 KB at S = 256, HE = 96 (+ 2 RP floats in the backward).
#include "vg_attn.h"
#include "vg_kernels.h"

#define VG_ATTN_LONG_WAVES 8  // at most; 512 threads, so the register budget is 256 per lane

template <int HE>
__global__ __launch_bounds__(64 * VG_ATTN_LONG_WAVES) void vg_attn_long_fwd_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ o,
                                                                                   float* __restrict__ lse, int B, int S, int H, float scale,
                                                                                   const void* __restrict__ zeros) {
  constexpr int KS = HE / 32, DT = HE / 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  const int RP = (S + 31) & ~31, NPAIR = RP / 32, NT = (S + 15) / 16;
  unsigned char* kl = sm;                // K: row-form fragments
  unsigned char* vl = sm + RP * HE * 2;  // V: transposed fragments
  int b, h;
  if (!attn_block(B, H, b, h)) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
  const int g = lane >> 4, li = lane & 15;
  const attn_head hd = head_view(qkv, b, h, S, H, HE);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  dma_head<HE>(kl, hd.k, hd.ld, S, RP, zeros, wv, nw, lane);
  dma_head<HE>(vl, hd.v, hd.ld, S, RP, zeros, wv, nw, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int qt = wv; qt < NT; qt += nw) {
    bf16x8 qf[KS];  // this tile's queries straight from global (nobody else needs them)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = gfrag(hd.q, hd.ld, 16 * qt, ks, S, lane);
    const int q = 16 * qt + li;
    float m = -INFINITY;  // running max of query q (the same in its 4 lane groups)
    float l = 0.f;        // this lane's share of the running sum, in units of exp(m)
    f32x4 oa[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) oa[dt] = zero;
    for (int u = 0; u < NPAIR; ++u) {  // keys 32 u .. 32 u + 31 (every pair holds at least one key < S)
      f32x4 sc[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x4 a = zero;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) a = vg_mfma(lfrag_row<HE>(kl, 32 * u + 16 * t, ks, lane), qf[ks], a);
        sc[t] = a;
      }
      float bm = -INFINITY;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = 32 * u + 16 * t + 4 * g + r;
          const float sv = (key < S) ? sc[t][r] * scale : -INFINITY;
          sc[t][r] = sv;
          bm = fmaxf(bm, sv);
        }
      const float mn = fmaxf(m, group_max(bm));
      const float alpha = __expf(m - mn);  // 0 on the first pair (m = -inf)
      m = mn;
      float ls = 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __expf(sc[t][r] - mn);
          sc[t][r] = p;
          ls += p;
        }
      l = l * alpha + ls;
      const bf16x8 pf = pack_pair(sc[0], sc[1]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) oa[dt] = vg_mfma(lfrag_tr<HE>(vl, u, 16 * dt, lane), pf, oa[dt] * alpha);
    }
    l = group_sum(l);
    if (g == 0 && q < S) lse[hd.offl + q] = m + __logf(l);
    store_tiles<DT>(hd.o_row(o, q < S ? q : 0), oa, 1.0f / l, g, q < S);
  }
}

// The recompute tiles (bwd_tile_q / bwd_tile_k) and row_delta are those of the short backward (vg_attn.h); the loops around them
// are this kernel's own: it streams the key (query) pairs and accumulates dQ (dK, dV) across them.
template <int HE>
__global__ __launch_bounds__(64 * VG_ATTN_LONG_WAVES) void vg_attn_long_bwd_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ o,
                                                                                   const bf16* __restrict__ d_o, const float* __restrict__ lse,
                                                                                   bf16* __restrict__ dqkv, int B, int S, int H, float scale,
                                                                                   const void* __restrict__ zeros) {
  constexpr int KS = HE / 32, DT = HE / 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  const int RP = (S + 31) & ~31, NPAIR = RP / 32, NT = (S + 15) / 16;
  unsigned char* s0 = sm;                      // K, then Q
  unsigned char* s1 = sm + RP * HE * 2;        // V, then dO
  float* dl = (float*)(sm + 2 * RP * HE * 2);  // delta[q] = sum_d dO*O (0 on the padding)
  float* ll = dl + RP;                         // lse[q]
  int b, h;
  if (!attn_block(B, H, b, h)) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
  const int g = lane >> 4, li = lane & 15;
  const attn_head hd = head_view(qkv, b, h, S, H, HE);
  const bf16* ob = hd.in_o(o);
  const bf16* dob = hd.in_o(d_o);
  const float* lb = hd.in_lse(lse);
  bf16* dqb = hd.in_qkv(dqkv);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  float unused = 0.f;  // the L2 row sum of the tile functions: dot-product scores only here

  dma_head<HE>(s0, hd.k, hd.ld, S, RP, zeros, wv, nw, lane);
  dma_head<HE>(s1, hd.v, hd.ld, S, RP, zeros, wv, nw, lane);
  for (int i = tid; i < RP; i += 64 * nw) ll[i] = (i < S) ? lb[i] : 0.f;
  for (int t = wv; t < RP / 16; t += nw) {  // every 16-row tile of the image, the padded one included (gfrag reads zeros there)
    bf16x8 of[KS], df[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      of[ks] = gfrag(ob, (size_t)hd.E, 16 * t, ks, S, lane);
      df[ks] = gfrag(dob, (size_t)hd.E, 16 * t, ks, S, lane);
    }
    const float delta = row_delta<KS>(df, of);
    if (g == 0) dl[16 * t + li] = delta;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // ---------------- phase A: S^T orientation (lane = query) -> dQ ----------------------
  for (int qt = wv; qt < NT; qt += nw) {
    bf16x8 qf[KS], dof[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      qf[ks] = gfrag(hd.q, hd.ld, 16 * qt, ks, S, lane);
      dof[ks] = gfrag(dob, (size_t)hd.E, 16 * qt, ks, S, lane);
    }
    const int q = 16 * qt + li;
    const float delta = dl[q];
    const float lse_q = ll[q];
    f32x4 dq[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) dq[dt] = zero;
    for (int u = 0; u < NPAIR; ++u) {
      f32x4 ds[2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
        ds[t] = bwd_tile_q<HE, false, false>(s0, s1, 32 * u + 16 * t, qf, dof, lse_q, delta, 0.f, nullptr, q < S, S, scale, unused, lane);
      const bf16x8 dsf = pack_pair(ds[0], ds[1]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) dq[dt] = vg_mfma(lfrag_tr<HE>(s0, u, 16 * dt, lane), dsf, dq[dt]);
    }
    store_tiles<DT>(dqb + (size_t)(q < S ? q : 0) * hd.ld, dq, 1.0f, g, q < S);
  }
  __syncthreads();  // every wave is done with K and V
  dma_head<HE>(s0, hd.q, hd.ld, S, RP, zeros, wv, nw, lane);
  dma_head<HE>(s1, dob, (size_t)hd.E, S, RP, zeros, wv, nw, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // ---------------- phase B: S orientation (lane = key) -> dK, dV ---------------------
  for (int kt = wv; kt < NT; kt += nw) {
    bf16x8 kf[KS], vf[KS];  // this tile's keys straight from global (L2: phase A's staging read the same rows)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      kf[ks] = gfrag(hd.k, hd.ld, 16 * kt, ks, S, lane);
      vf[ks] = gfrag(hd.v, hd.ld, 16 * kt, ks, S, lane);
    }
    const int key = 16 * kt + li;
    f32x4 dk[DT], dv[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) { dk[dt] = zero; dv[dt] = zero; }
    for (int u = 0; u < NPAIR; ++u) {
      f32x4 pr[2], ds[2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
        bwd_tile_k<HE, false, false>(s0, s1, 32 * u + 16 * t, kf, vf, ll, dl, nullptr, 0.f, key < S, S, scale, unused, lane, pr[t], ds[t]);
      const bf16x8 pf = pack_pair(pr[0], pr[1]);
      const bf16x8 dsf = pack_pair(ds[0], ds[1]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        dv[dt] = vg_mfma(lfrag_tr<HE>(s1, u, 16 * dt, lane), pf, dv[dt]);
        dk[dt] = vg_mfma(lfrag_tr<HE>(s0, u, 16 * dt, lane), dsf, dk[dt]);
      }
    }
    bf16* rowp = dqb + (size_t)(key < S ? key : 0) * hd.ld;
    store_tiles<DT>(rowp + hd.E, dk, 1.0f, g, key < S);
    store_tiles<DT>(rowp + 2 * hd.E, dv, 1.0f, g, key < S);
  }
}

static inline int long_rows(int S) { return (S + 31) & ~31; }
static inline int long_waves(int S) { const int nt = (S + 15) / 16; return nt < VG_ATTN_LONG_WAVES ? nt : VG_ATTN_LONG_WAVES; }
static inline size_t long_fwd_lds(int S, int HE) { return (size_t)2 * long_rows(S) * HE * 2; }
static inline size_t long_bwd_lds(int S, int HE) { return long_fwd_lds(S, HE) + (size_t)2 * long_rows(S) * 4; }
// dynamic LDS above 64 KiB (S = 256, HE = 96: 96 / 98 KiB): each kernel's limit is raised once, to what S = VG_ATTN_LONG_MAX_S needs
static int long_allow_lds(const void* fn, size_t bytes) { return (int)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes); }

template <int HE>
static int launch_long_fwd(const bf16* qkv, bf16* o, float* lse, int B, int H, int S, float scale, hipStream_t st) {
  const void* z = vg_attn_zeros();
  if (!z) return -5;
  static const int lim = long_allow_lds((const void*)vg_attn_long_fwd_kernel<HE>, long_fwd_lds(VG_ATTN_LONG_MAX_S, HE));
  if (lim) return lim;
  hipLaunchKernelGGL((vg_attn_long_fwd_kernel<HE>), dim3(attn_grid(B, H)), dim3(64 * long_waves(S)), long_fwd_lds(S, HE), st, qkv, o, lse, B, S, H,
                     scale, z);
  return (int)hipGetLastError();
}
template <int HE>
static int launch_long_bwd(const bf16* qkv, const bf16* o, const bf16* d_o, const float* lse, bf16* dqkv, int B, int H, int S, float scale,
                           hipStream_t st) {
  const void* z = vg_attn_zeros();
  if (!z) return -5;
  static const int lim = long_allow_lds((const void*)vg_attn_long_bwd_kernel<HE>, long_bwd_lds(VG_ATTN_LONG_MAX_S, HE));
  if (lim) return lim;
  hipLaunchKernelGGL((vg_attn_long_bwd_kernel<HE>), dim3(attn_grid(B, H)), dim3(64 * long_waves(S)), long_bwd_lds(S, HE), st, qkv, o, d_o, lse,
                     dqkv, B, S, H, scale, z);
  return (int)hipGetLastError();
}

// Dot-product scores only: mode 0 of vg_attn_fwd_launch / vg_attn_bwd_launch, which send 80 < S <= 256 here.  The kernels are
// correct for any 1 <= S <= VG_ATTN_LONG_MAX_S.  -2: shape out of range, -3: head dim not 32 / 64 / 96.
int vg_attn_long_fwd_launch(const bf16* qkv, bf16* o, float* lse, int B, int H, int S, int HE, float scale, hipStream_t st) {
  if (S < 1 || S > VG_ATTN_LONG_MAX_S || B < 1 || H < 1) return -2;
  return attn_by_head_dim(HE, [&](auto he) { return launch_long_fwd<decltype(he)::value>(qkv, o, lse, B, H, S, scale, st); });
}
int vg_attn_long_bwd_launch(const bf16* qkv, const bf16* o, const bf16* d_o, const float* lse, bf16* dqkv, int B, int H, int S, int HE,
                            float scale, hipStream_t st) {
  if (S < 1 || S > VG_ATTN_LONG_MAX_S || B < 1 || H < 1) return -2;
  return attn_by_head_dim(HE, [&](auto he) { return launch_long_bwd<decltype(he)::value>(qkv, o, d_o, lse, dqkv, B, H, S, scale, st); });
}
