// Fused multi-head self-attention (forward and backward) for short sequences (S <= 80): one workgroup
// per (image, head), ONE WAVE PER 16-ROW TILE (5 waves for S = 65).  gfx950 only.
// These kernels are HBM/latency bound (4 % of the step's FLOPs): every operand of a head is staged into LDS
// exactly once by LDS-DMA in a single load phase, everything is computed from LDS, and the outputs leave as
// 16-byte stores; the co-resident workgroups of a CU overlap each other's load / compute / store phases.
//
// The whole S x S score tile lives in MFMA accumulators; softmax runs in registers.
// Layout trick (cdna_hip_programming.md s3, "an accumulator tile as the next MFMA's operand"):
// scores are produced as S^T = K Q^T, so a lane owns ONE query column and 4 consecutive keys per
// tile.  The exponentiated registers are then, unchanged, the k-operand of the P.V product, whose
// other operand (V, keys along k) is read from LDS with ds_read_b64_tr_b16 in the matching key
// order.  No probability ever touches LDS or HBM.
//
// qkv layout: [B*S, 3E] bf16 row-major, columns [0,E) = Q, [E,2E) = K, [2E,3E) = V, head h at
// columns h*HE .. (h+1)*HE of each third.  o / d_o: [B*S, E].  lse: [B, H, S] fp32 (natural log).
#include "vg_attn.h"
#include "vg_kernels.h"

template <int HE, int NT, bool L2, bool FP8>
__global__ __launch_bounds__(64 * NT) void vg_attn_fwd_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ o,
                                                              float* __restrict__ lse, int B, int S, int H, float scale,
                                                              const void* __restrict__ zeros) {
  constexpr int KS = HE / 32, DT = HE / 16, KP = (NT + 1) / 2, RP = KP * 32, RK = 16 * NT;
  __shared__ __attribute__((aligned(16))) unsigned char sm[(RK + RP) * HE * 2 + (L2 ? RK * 4 : 0)];
  unsigned char* kl = sm;                 // K, rows [0, 16 NT): row-form fragments
  unsigned char* vl = sm + RK * HE * 2;   // V, rows [0, 32 KP): transposed fragments
  float* kn = (float*)(sm + (RK + RP) * HE * 2);  // L2 scores: |k|^2 per key
  int b, h;
  if (!attn_block(B, H, b, h)) return;
  const int tid = threadIdx.x, lane = tid & 63, qt = tid >> 6;  // wave qt owns query rows 16*qt .. 16*qt+15
  const int g = lane >> 4, li = lane & 15;
  const attn_head hd = head_view(qkv, b, h, S, H, HE);

  bf16x8 qf[KS];  // this wave's queries straight from global (nobody else needs them)
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) qf[ks] = gfrag(hd.q, hd.ld, 16 * qt, ks, S, lane);
  dma_head<HE>(kl, hd.k, hd.ld, S, RK, zeros, qt, NT, lane);
  dma_head<HE>(vl, hd.v, hd.ld, S, RP, zeros, (qt + 2) % NT, NT, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  float qn = 0.f;
  if (L2) {
    row_sqnorms<HE>(kl, kn, RK, tid, 64 * NT);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float f = vg_bf2f(qf[ks][j]); qn += f * f; }
    qn = group_sum(qn);
    __syncthreads();
  }

  f32x4 sc[NT];  // [kt]: rows = keys 16kt+4g+r, col = query 16qt+li
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) a = score_mfma<FP8>(lfrag_row<HE>(kl, 16 * kt, ks, lane), qf[ks], a);
    sc[kt] = a;
  }
  const int q = 16 * qt + li;
  float m = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = 16 * kt + 4 * g + r;
      const float raw = L2 ? l2_dist(sc[kt][r], qn, kn[key]) : sc[kt][r];
      const float sv = (key < S) ? raw * scale : -INFINITY;
      sc[kt][r] = sv;
      m = fmaxf(m, sv);
    }
  m = group_max(m);
  float l = 0.f;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = __expf(sc[kt][r] - m);
      sc[kt][r] = p;
      l += p;
    }
  l = group_sum(l);
  const float inv_l = 1.0f / l;
  if (g == 0 && q < S) lse[hd.offl + q] = m + __logf(l);

  f32x4 oa[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) oa[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < KP; ++u) {
    const f32x4 hi = tile_or_zero<NT>(sc, 2 * u + 1);  // shared by the fp8 and the bf16 packing
    if constexpr (FP8) {
      const fp8x8 pf = pack_pair_fp8(sc[2 * u], hi, VG_P_FP8_SCALE);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) oa[dt] = vg_mfma_fp8(to_fp8(lfrag_tr<HE>(vl, u, 16 * dt, lane)), pf, oa[dt]);
    } else {
      const bf16x8 pf = pack_pair(sc[2 * u], hi);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) oa[dt] = vg_mfma(lfrag_tr<HE>(vl, u, 16 * dt, lane), pf, oa[dt]);
    }
  }
  store_tiles<DT>(hd.o_row(o, q < S ? q : 0), oa, FP8 ? inv_l * (1.0f / VG_P_FP8_SCALE) : inv_l, g, q < S);
}

// Backward.  Phase A works in the S^T orientation (lane = query) and yields dQ; phase B in the
// S orientation (lane = key) and yields dK, dV.  Recomputing the 65x65 tile in both orientations
// costs 2 x 75 extra MFMAs per head and removes every register transpose.
// FP8: the score product is recomputed with the forward's e4m3 operands (so P matches the forward's lse exactly); every
// product that carries a gradient operand (dP, dV, dQ, dK) stays bf16 - gradients need the range.
// The arithmetic is bwd_phase_a / bwd_phase_b of vg_attn.h; the two kernels below are two stagings of those phases.
// Four images: everything a head needs is staged ONCE (K, V, Q, dO images by LDS-DMA + lse and delta per query).  One load
// phase, one compute phase, one store phase per workgroup; the co-resident workgroup overlaps them.
template <int HE, int NT, bool L2, bool FP8>
__global__ __launch_bounds__(64 * NT, 2) void vg_attn_bwd_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ o,
                                                         const bf16* __restrict__ d_o, const float* __restrict__ lse,
                                                         bf16* __restrict__ dqkv, int B, int S, int H, float scale,
                                                         const void* __restrict__ zeros) {
  constexpr int KS = HE / 32, KP = (NT + 1) / 2, RP = KP * 32;
  constexpr int IMG = RP * HE * 2;
  __shared__ __attribute__((aligned(16))) unsigned char sm[4 * IMG + (L2 ? 4 : 2) * RP * 4];
  unsigned char* lk = sm;
  unsigned char* lv = sm + IMG;
  unsigned char* lq = sm + 2 * IMG;
  unsigned char* ldo = sm + 3 * IMG;
  float* dl = (float*)(sm + 4 * IMG);  // delta[q] = sum_d dO*O
  float* ll = dl + RP;                 // lse[q]
  float* qn_l = ll + RP;               // L2 scores: |q|^2 per query, |k|^2 per key
  float* kn_l = qn_l + RP;
  int b, h;
  if (!attn_block(B, H, b, h)) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;  // wave wv owns query tile wv (phase A) / key tile wv (phase B)
  const int g = lane >> 4, li = lane & 15;
  const attn_head hd = head_view(qkv, b, h, S, H, HE);
  const bf16* ob = hd.in_o(o);
  const bf16* dob = hd.in_o(d_o);
  const float* lb = hd.in_lse(lse);
  const bwd_rows rw = {dl, ll, qn_l, kn_l};

  bf16x8 of[KS];  // O is only needed for delta: this wave's 16 query rows, straight from global
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) of[ks] = gfrag(ob, (size_t)hd.E, 16 * wv, ks, S, lane);
  dma_head<HE>(lk, hd.k, hd.ld, S, RP, zeros, wv, NT, lane);
  dma_head<HE>(lv, hd.v, hd.ld, S, RP, zeros, (wv + 1) % NT, NT, lane);
  dma_head<HE>(lq, hd.q, hd.ld, S, RP, zeros, (wv + 2) % NT, NT, lane);
  dma_head<HE>(ldo, dob, (size_t)hd.E, S, RP, zeros, (wv + 3) % NT, NT, lane);
  for (int i = tid; i < RP; i += 64 * NT) ll[i] = (i < S) ? lb[i] : 0.f;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  bf16x8 qf[KS], dof[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    qf[ks] = lfrag_row<HE>(lq, 16 * wv, ks, lane);
    dof[ks] = lfrag_row<HE>(ldo, 16 * wv, ks, lane);
  }
  const float delta = row_delta<KS>(dof, of);
  if (g == 0) dl[16 * wv + li] = delta;
  if (L2) { row_sqnorms<HE>(lq, qn_l, RP, tid, 64 * NT); row_sqnorms<HE>(lk, kn_l, RP, tid, 64 * NT); }
  __syncthreads();

  bwd_phase_a<HE, NT, L2, FP8>(lk, lv, lq, qf, dof, rw, hd.in_qkv(dqkv), hd.ld, S, scale, wv, lane);
  bf16x8 kf[KS], vf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    kf[ks] = lfrag_row<HE>(lk, 16 * wv, ks, lane);
    vf[ks] = lfrag_row<HE>(lv, 16 * wv, ks, lane);
  }
  bwd_phase_b<HE, NT, L2, FP8>(lq, ldo, lk, kf, vf, rw, hd.in_qkv(dqkv), hd.ld, hd.E, S, scale, wv, lane);
}

// The same backward with TWO LDS images instead of four (dot-product scores, S > 32): phase A needs K and V whole and only this
// wave's 16 rows of Q and dO (read straight from global as fragments), phase B needs Q and dO whole and only this wave's rows of K
// and V (fragments taken from the images before they are overwritten) - so Q and dO are staged into the SAME two images between
// the phases.  37 KB instead of 74 KB of LDS per workgroup: four workgroups (20 waves) per CU instead of two, and it is the
// co-resident workgroups that overlap one another's load / compute / store phases (the kernel is latency-bound: 4.0 TB/s of its
// 205 MB at two workgroups per CU).  HBM bytes are unchanged (the fragment reads of the own rows hit L2 or are the first touch of
// lines the second staging then finds there).  Results are bit-equal to vg_attn_bwd_kernel's because both kernels call the same two
// phases on the same operand values (the phases produce the output tiles two at a time: 96 registers at five waves per SIMD).
#ifndef VG_ATTN_BWD2_WPE
#define VG_ATTN_BWD2_WPE 5  // waves per SIMD the register budget is set for: 5 = four 5-wave workgroups per CU (96 VGPRs)
#endif
template <int HE, int NT, bool FP8>
__global__ __launch_bounds__(64 * NT, VG_ATTN_BWD2_WPE) void vg_attn_bwd2_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ o,
                                                                  const bf16* __restrict__ d_o, const float* __restrict__ lse,
                                                                  bf16* __restrict__ dqkv, int B, int S, int H, float scale,
                                                                  const void* __restrict__ zeros) {
  constexpr int KS = HE / 32, KP = (NT + 1) / 2, RP = KP * 32;
  constexpr int IMG = RP * HE * 2;
  __shared__ __attribute__((aligned(16))) unsigned char sm[2 * IMG + 2 * RP * 4];
  unsigned char* s0 = sm;        // K, then Q
  unsigned char* s1 = sm + IMG;  // V, then dO
  float* dl = (float*)(sm + 2 * IMG);  // delta[q] = sum_d dO*O
  float* ll = dl + RP;                 // lse[q]
  int b, h;
  if (!attn_block(B, H, b, h)) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;  // wave wv owns query tile wv (phase A) / key tile wv (phase B)
  const int g = lane >> 4, li = lane & 15;
  const attn_head hd = head_view(qkv, b, h, S, H, HE);
  const bf16* ob = hd.in_o(o);
  const bf16* dob = hd.in_o(d_o);
  const float* lb = hd.in_lse(lse);
  const bwd_rows rw = {dl, ll, nullptr, nullptr};

  dma_head<HE>(s0, hd.k, hd.ld, S, RP, zeros, wv, NT, lane);
  dma_head<HE>(s1, hd.v, hd.ld, S, RP, zeros, (wv + 1) % NT, NT, lane);
  bf16x8 qf[KS], dof[KS];
  {
    bf16x8 of[KS];  // this wave's 16 query rows of O, Q, dO straight from global
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      of[ks] = gfrag(ob, (size_t)hd.E, 16 * wv, ks, S, lane);
      dof[ks] = gfrag(dob, (size_t)hd.E, 16 * wv, ks, S, lane);
      qf[ks] = gfrag(hd.q, hd.ld, 16 * wv, ks, S, lane);
    }
    for (int i = tid; i < RP; i += 64 * NT) ll[i] = (i < S) ? lb[i] : 0.f;
    const float delta = row_delta<KS>(dof, of);
    if (g == 0) dl[16 * wv + li] = delta;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  bwd_phase_a<HE, NT, false, FP8>(s0, s1, nullptr, qf, dof, rw, hd.in_qkv(dqkv), hd.ld, S, scale, wv, lane);
  // this wave's key tile for phase B, before Q and dO take the images over
  bf16x8 kf[KS], vf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    kf[ks] = lfrag_row<HE>(s0, 16 * wv, ks, lane);
    vf[ks] = lfrag_row<HE>(s1, 16 * wv, ks, lane);
  }
  __syncthreads();  // (waits for the LDS reads above: every wave is done with K and V)
  dma_head<HE>(s0, hd.q, hd.ld, S, RP, zeros, wv, NT, lane);
  dma_head<HE>(s1, dob, (size_t)hd.E, S, RP, zeros, (wv + 1) % NT, NT, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  bwd_phase_b<HE, NT, false, FP8>(s0, s1, nullptr, kf, vf, rw, hd.in_qkv(dqkv), hd.ld, hd.E, S, scale, wv, lane);
}

// ---- the backward OF the attention backward (gradient penalty, src/v2/utils.py:124-144) on the MFMA pipe -------------------
// Forward: P = softmax(s Q K^T), O = P V.  Backward: dV = P^T dO ; dP = dO V^T ; delta_i = sum_j P_ij dP_ij ; dS = P (dP - delta) ;
// dQ = s dS K ; dK = s dS^T Q.  Given (uQ, uK, uV) = dL/d(dQ, dK, dV):
//   G = s (uQ K^T + Q uK^T) ; gam_i = sum_j G_ij P_ij ; H = P (G - gam)                       [dL/d dP]
//   Pi = dO uV^T + G (dP - delta) - gam dP ; pi_i = sum_j P_ij Pi_ij ; Sg = P (Pi - pi)       [dL/d S]
//   d(dO) = P uV + H V ;  d(Q) = s (dS uK + Sg K) ;  d(K) = s (dS^T uQ + Sg^T Q) ;  d(V) = H^T dO.
// Same two-orientation scheme as the first-order backward: phase A (lane = query; K, V, uK, uV as LDS images, this wave's 16 rows of
// Q, dO, uQ as fragments straight from global) computes the five S x S products of a query tile against every key tile in MFMA
// accumulators, the three row sums (delta, gam, pi; left in LDS for phase B) and the query-side outputs d(dO), d(Q); phase B
// (lane = key; Q, dO, uQ staged into the same images, this wave's rows of K, V, uK, uV kept as fragments) recomputes the products in
// the other orientation and yields d(K), d(V).  The S x S matrices never leave registers (round 2's kernel kept four of them as fp32
// in LDS and ran plain FMA loops: 1.2 ms per launch); they enter the output products as bf16, like P and dS in the first-order
// backward.  One workgroup per (image, head), five waves, 74 KB of LDS.
template <int HE>
__global__ __launch_bounds__(320, 2) void vg_attn_bwd_bwd2_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ d_o,
                                                                  const float* __restrict__ lse, const bf16* __restrict__ uqkv,
                                                                  bf16* __restrict__ d_do, bf16* __restrict__ d_qkv, int B, int S, int H,
                                                                  float scale, const void* __restrict__ zeros) {
  constexpr int NT = 5, KS = HE / 32, DT = HE / 16, KP = 3, RP = 96;
  constexpr int IMG = RP * HE * 2;
  __shared__ __attribute__((aligned(16))) unsigned char sm[4 * IMG + 4 * RP * 4];
  unsigned char* i0 = sm;            // K,  then Q
  unsigned char* i1 = sm + IMG;      // V,  then dO
  unsigned char* i2 = sm + 2 * IMG;  // uK, then uQ
  unsigned char* i3 = sm + 3 * IMG;  // uV
  float* dl = (float*)(sm + 4 * IMG);  // delta[q]
  float* gm = dl + RP;                 // gam[q]
  float* pl = gm + RP;                 // pi[q]
  float* ll = pl + RP;                 // lse[q]
  int b, h;
  if (!attn_block(B, H, b, h)) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  // The head's bases are spelled out here instead of taken from head_view (vg_attn.h), on measurement: with the view the scalar
  // preamble comes out a few instructions different and every launch at the hot shape 0.3 - 0.8 us (of 123) longer, in every order of
  // the libraries; with this text the instruction stream is the one it had before the shared header (profiles/attn_shared_phases.txt).
  const int E = H * HE;
  const size_t ld = 3 * (size_t)E;
  const bf16* qb = qkv + (size_t)b * S * ld + h * HE;
  const bf16* kb = qb + E;
  const bf16* vb = qb + 2 * E;
  const bf16* uqb = uqkv + (size_t)b * S * ld + h * HE;
  const bf16* ukb = uqb + E;
  const bf16* uvb = uqb + 2 * E;
  const bf16* dob = d_o + (size_t)b * S * E + h * HE;
  const float* lb = lse + ((size_t)b * H + h) * S;
  bf16* ddob = d_do + (size_t)b * S * E + h * HE;
  bf16* dqb = d_qkv + (size_t)b * S * ld + h * HE;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  dma_head<HE>(i0, kb, ld, S, RP, zeros, wv, NT, lane);
  dma_head<HE>(i1, vb, ld, S, RP, zeros, (wv + 1) % NT, NT, lane);
  dma_head<HE>(i2, ukb, ld, S, RP, zeros, (wv + 2) % NT, NT, lane);
  dma_head<HE>(i3, uvb, ld, S, RP, zeros, (wv + 3) % NT, NT, lane);
  bf16x8 qf[KS], dof[KS], uqf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    qf[ks] = gfrag(qb, ld, 16 * wv, ks, S, lane);
    dof[ks] = gfrag(dob, (size_t)E, 16 * wv, ks, S, lane);
    uqf[ks] = gfrag(uqb, ld, 16 * wv, ks, S, lane);
  }
  for (int i = tid; i < RP; i += 64 * NT) ll[i] = (i < S) ? lb[i] : 0.f;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // ---------------- phase A: lane = query li of tile wv; keys 16 kt + 4 g + r -------------------------------------------
  {
    const int q = 16 * wv + li;
    const float lse_q = ll[q];
    f32x4 Pm[NT], Dm[NT], Gm[NT], Tm[NT];
    float delta = 0.f, gam = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      f32x4 st = zero, dpt = zero, gt = zero, tt = zero;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const bf16x8 kr = lfrag_row<HE>(i0, 16 * kt, ks, lane);
        st = vg_mfma(kr, qf[ks], st);
        gt = vg_mfma(kr, uqf[ks], gt);
        gt = vg_mfma(lfrag_row<HE>(i2, 16 * kt, ks, lane), qf[ks], gt);
        dpt = vg_mfma(lfrag_row<HE>(i1, 16 * kt, ks, lane), dof[ks], dpt);
        tt = vg_mfma(lfrag_row<HE>(i3, 16 * kt, ks, lane), dof[ks], tt);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * kt + 4 * g + r;
        const float p = (key < S && q < S) ? __expf(st[r] * scale - lse_q) : 0.f;
        const float gv = gt[r] * scale;
        Pm[kt][r] = p; Dm[kt][r] = dpt[r]; Gm[kt][r] = gv; Tm[kt][r] = tt[r];
        delta += p * dpt[r];
        gam += p * gv;
      }
    }
    delta = group_sum(delta);
    gam = group_sum(gam);
    float pis = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float a = Dm[kt][r] - delta;
        const float pie = Tm[kt][r] + Gm[kt][r] * a - gam * Dm[kt][r];
        Tm[kt][r] = pie;                 // Pi
        Dm[kt][r] = a;                   // dP - delta
        pis += Pm[kt][r] * pie;
      }
    pis = group_sum(pis);
    if (g == 0) { dl[q] = delta; gm[q] = gam; pl[q] = pis; }
    // H = P (G - gam) -> Gm ;  dS = P (dP - delta) -> Dm ;  Sg = P (Pi - pi) -> Tm
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = Pm[kt][r];
        Gm[kt][r] = p * (Gm[kt][r] - gam);
        Dm[kt][r] = p * Dm[kt][r];
        Tm[kt][r] = p * (Tm[kt][r] - pis);
      }
    bf16x8 pf[KP], hf[KP], dsf[KP], sgf[KP];
#pragma unroll
    for (int u = 0; u < KP; ++u) {  // pair by pair over the four sets: packing set after set costs 17 packed float operations and 0.5 us
      pf[u] = pack_tiles_at<NT>(Pm, u);
      hf[u] = pack_tiles_at<NT>(Gm, u);
      dsf[u] = pack_tiles_at<NT>(Dm, u);
      sgf[u] = pack_tiles_at<NT>(Tm, u);
    }
    bf16* rowo = ddob + (size_t)(q < S ? q : 0) * E;
    bf16* rowq = dqb + (size_t)(q < S ? q : 0) * ld;
#pragma unroll
    for (int pp = 0; pp < DT / 2; ++pp) {  // two head-dim tiles at a time (one 16-byte store per lane)
      f32x4 o1[2] = {zero, zero}, o2[2] = {zero, zero};
#pragma unroll
      for (int u = 0; u < KP; ++u)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int d0 = 32 * pp + 16 * t;
          o1[t] = vg_mfma(lfrag_tr<HE>(i3, u, d0, lane), pf[u], o1[t]);   // P uV
          o1[t] = vg_mfma(lfrag_tr<HE>(i1, u, d0, lane), hf[u], o1[t]);   // + H V
          o2[t] = vg_mfma(lfrag_tr<HE>(i2, u, d0, lane), dsf[u], o2[t]);  // dS uK
          o2[t] = vg_mfma(lfrag_tr<HE>(i0, u, d0, lane), sgf[u], o2[t]);  // + Sg K
        }
      store_tiles<2>(rowo + 32 * pp, o1, 1.0f, g, q < S);
      store_tiles<2>(rowq + 32 * pp, o2, scale, g, q < S);
    }
  }
  // this wave's key tile for phase B, before Q, dO, uQ take the images over
  bf16x8 kf[KS], vf[KS], ukf[KS], uvf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    kf[ks] = lfrag_row<HE>(i0, 16 * wv, ks, lane);
    vf[ks] = lfrag_row<HE>(i1, 16 * wv, ks, lane);
    ukf[ks] = lfrag_row<HE>(i2, 16 * wv, ks, lane);
    uvf[ks] = lfrag_row<HE>(i3, 16 * wv, ks, lane);
  }
  __syncthreads();  // every wave is done with K, V, uK, uV (and delta / gam / pi of every query are in LDS)
  dma_head<HE>(i0, qb, ld, S, RP, zeros, wv, NT, lane);
  dma_head<HE>(i1, dob, (size_t)E, S, RP, zeros, (wv + 1) % NT, NT, lane);
  dma_head<HE>(i2, uqb, ld, S, RP, zeros, (wv + 2) % NT, NT, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // ---------------- phase B: lane = key li of tile wv; queries 16 qt + 4 g + r -------------------------------------------
  {
    const int key = 16 * wv + li;
    f32x4 Hm[NT], Dm[NT], Sm[NT];
#pragma unroll
    for (int qt = 0; qt < NT; ++qt) {
      f32x4 st = zero, dpt = zero, gt = zero, tt = zero;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const bf16x8 qr = lfrag_row<HE>(i0, 16 * qt, ks, lane);
        const bf16x8 dr = lfrag_row<HE>(i1, 16 * qt, ks, lane);
        st = vg_mfma(qr, kf[ks], st);
        gt = vg_mfma(qr, ukf[ks], gt);
        gt = vg_mfma(lfrag_row<HE>(i2, 16 * qt, ks, lane), kf[ks], gt);
        dpt = vg_mfma(dr, vf[ks], dpt);
        tt = vg_mfma(dr, uvf[ks], tt);
      }
      const f32x4 lq4 = *(const f32x4*)(ll + 16 * qt + 4 * g);
      const f32x4 dl4 = *(const f32x4*)(dl + 16 * qt + 4 * g);
      const f32x4 gm4 = *(const f32x4*)(gm + 16 * qt + 4 * g);
      const f32x4 pl4 = *(const f32x4*)(pl + 16 * qt + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = 16 * qt + 4 * g + r;
        const float p = ((q < S) && (key < S)) ? __expf(st[r] * scale - lq4[r]) : 0.f;
        const float gv = gt[r] * scale, a = dpt[r] - dl4[r];
        const float pie = tt[r] + gv * a - gm4[r] * dpt[r];
        Hm[qt][r] = p * (gv - gm4[r]);
        Dm[qt][r] = p * a;
        Sm[qt][r] = p * (pie - pl4[r]);
      }
    }
    bf16x8 hf[KP], dsf[KP], sgf[KP];
#pragma unroll
    for (int u = 0; u < KP; ++u) {
      hf[u] = pack_tiles_at<NT>(Hm, u);
      dsf[u] = pack_tiles_at<NT>(Dm, u);
      sgf[u] = pack_tiles_at<NT>(Sm, u);
    }
    bf16* rowp = dqb + (size_t)(key < S ? key : 0) * ld;
#pragma unroll
    for (int pp = 0; pp < DT / 2; ++pp) {
      f32x4 dk[2] = {zero, zero}, dv[2] = {zero, zero};
#pragma unroll
      for (int u = 0; u < KP; ++u)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int d0 = 32 * pp + 16 * t;
          dk[t] = vg_mfma(lfrag_tr<HE>(i2, u, d0, lane), dsf[u], dk[t]);  // dS^T uQ
          dk[t] = vg_mfma(lfrag_tr<HE>(i0, u, d0, lane), sgf[u], dk[t]);  // + Sg^T Q
          dv[t] = vg_mfma(lfrag_tr<HE>(i1, u, d0, lane), hf[u], dv[t]);   // H^T dO
        }
      store_tiles<2>(rowp + E + 32 * pp, dk, scale, g, key < S);
      store_tiles<2>(rowp + 2 * E + 32 * pp, dv, 1.0f, g, key < S);
    }
  }
}

// the 16-byte zero page every LDS-DMA staging reads its padded rows from (attention_long.hip's too); null if it cannot be resolved
__device__ __attribute__((aligned(16))) unsigned int vg_attn_zero_page[4] = {0u, 0u, 0u, 0u};
const void* vg_attn_zeros() {
  static void* zp = nullptr;  // one device per process
  if (!zp && hipGetSymbolAddress(&zp, HIP_SYMBOL(vg_attn_zero_page)) != hipSuccess) zp = nullptr;
  return zp;
}

template <int HE, int NT, int MODE>  // MODE: 0 dot-product bf16, 1 L2-distance scores, 2 dot-product with fp8 activation products
static int launch_fwd(const bf16* qkv, bf16* o, float* lse, int B, int H, int S, float scale, hipStream_t st) {
  const void* z = vg_attn_zeros();
  if (!z) return -5;
  hipLaunchKernelGGL((vg_attn_fwd_kernel<HE, NT, MODE == 1, MODE == 2>), dim3(attn_grid(B, H)), dim3(64 * NT), 0, st, qkv, o, lse, B, S, H, scale, z);
  return (int)hipGetLastError();
}
template <int HE, int NT, int MODE>
static int launch_bwd(const bf16* qkv, const bf16* o, const bf16* d_o, const float* lse, bf16* dqkv, int B, int H,
                      int S, float scale, hipStream_t st) {
  const void* z = vg_attn_zeros();
  if (!z) return -5;
#ifndef VG_ATTN_BWD_4IMG  // A/B builds (make var DEFS=-DVG_ATTN_BWD_4IMG): the four-image kernel everywhere
  constexpr bool two_images = MODE != 1 && NT == 5;
#else
  constexpr bool two_images = false;
#endif
  if constexpr (two_images)  // only the kernel that is launched is instantiated
    hipLaunchKernelGGL((vg_attn_bwd2_kernel<HE, NT, MODE == 2>), dim3(attn_grid(B, H)), dim3(64 * NT), 0, st, qkv, o, d_o, lse, dqkv, B, S, H, scale, z);
  else
    hipLaunchKernelGGL((vg_attn_bwd_kernel<HE, NT, MODE == 1, MODE == 2>), dim3(attn_grid(B, H)), dim3(64 * NT), 0, st, qkv, o, d_o, lse, dqkv, B, S, H, scale, z);
  return (int)hipGetLastError();
}

// Supported shapes: head dim 32, 64 or 96; S <= 32 (2 tiles) or S <= 80 (5 tiles).  (80 < S <= 256, mode 0: attention_long.hip.)
// mode = 0: dot-product scores (src/v2/modules.py:142-155, v1 lp = 1); 1: Euclidean-distance scores (v1 lp = 2);
// 2: dot-product scores with fp8 (e4m3) operands for Q.K^T (forward and recompute) and P.V (config C5).
#define VG_ATTN_BY_NT(FN, HE_, MODE_, ...) return small ? FN<HE_, 2, MODE_>(__VA_ARGS__) : FN<HE_, 5, MODE_>(__VA_ARGS__)
#define VG_ATTN_BY_MODE(FN, HE_, ...)                                  \
  do {                                                                 \
    if (mode == 0) { VG_ATTN_BY_NT(FN, HE_, 0, __VA_ARGS__); }         \
    if (mode == 1) { VG_ATTN_BY_NT(FN, HE_, 1, __VA_ARGS__); }         \
    VG_ATTN_BY_NT(FN, HE_, 2, __VA_ARGS__);                            \
  } while (0)
#define VG_ATTN_DISPATCH(FN, ...)                                      \
  do {                                                                 \
    if (S < 1 || S > 80 || B < 1 || H < 1) return -2;                  \
    if (mode < 0 || mode > 2) return -4;                               \
    const bool small = (S <= 32);                                      \
    return attn_by_head_dim(HE, [&](auto he) -> int {                  \
      constexpr int HE_ = decltype(he)::value;                         \
      VG_ATTN_BY_MODE(FN, HE_, __VA_ARGS__);                           \
    });                                                                \
  } while (0)
// 80 < S <= VG_ATTN_LONG_MAX_S with dot-product scores (mode 0): the streaming kernels of attention_long.hip; modes 1 and 2 stay S <= 80.
int vg_attn_fwd_launch(const bf16* qkv, bf16* o, float* lse, int B, int H, int S, int HE, float scale, int mode, hipStream_t st) {
  if (mode == 0 && S > VG_SHORT_MAX_S && S <= VG_ATTN_LONG_MAX_S) return vg_attn_long_fwd_launch(qkv, o, lse, B, H, S, HE, scale, st);
  VG_ATTN_DISPATCH(launch_fwd, qkv, o, lse, B, H, S, scale, st);
}
int vg_attn_bwd_launch(const bf16* qkv, const bf16* o, const bf16* d_o, const float* lse, bf16* dqkv, int B, int H,
                       int S, int HE, float scale, int mode, hipStream_t st) {
  if (mode == 0 && S > VG_SHORT_MAX_S && S <= VG_ATTN_LONG_MAX_S) return vg_attn_long_bwd_launch(qkv, o, d_o, lse, dqkv, B, H, S, HE, scale, st);
  VG_ATTN_DISPATCH(launch_bwd, qkv, o, d_o, lse, dqkv, B, H, S, scale, st);
}

// ---------------------------------------------------------------------------------------------------------------------
// Attention of the TOP encoder block as the classifier sees it (src/v2/modules.py:195 reads the CLS row only): ONE query - row 0 of
// every image - against all S keys.  Forward: o_cls[b, h*HE ..] = softmax(s q0 K^T) V; backward: dO is nonzero for that query
// only, so dK_j = ds_j q0, dV_j = p_j dO_0 are rank-one and dQ is zero off row 0.  Same arithmetic as the full kernels at that
// row (fp32 scores of bf16 operands, p and ds rounded to bf16 where the full kernels make them MFMA operands, 1 / l applied to
// the fp32 sum), 1/65 of their products and half their bytes (K and V in, dK and dV out).  One wave per (image, head).  (A first
// version with lanes over the KEYS - a lane reading and writing its own rows in 16-byte chunks, 64 row segments per instruction -
// took 65 us for the 2B backward, more than the full kernel's 57.)
// ---------------------------------------------------------------------------------------------------------------------
// Work layout of both kernels: a wave walks the head's K / V rows RPI at a time, lane = (row rr = lane / CPR, 16-byte chunk c = lane % CPR),
// so every load and store of a wave-instruction covers RPI whole 2 HE-byte row segments (HE = 96: 60 of the 64 lanes, 5 rows).
template <int HE, int KMAX>  // KMAX: key capacity (128 or 256) of the LDS score arrays
__global__ __launch_bounds__(64) void vg_attn_cls_fwd_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ o_cls, float* __restrict__ lse_cls,
                                                             int B, int S, int H, float scale) {
  constexpr int CPR = HE / 8, RPI = 64 / CPR;
  __shared__ float q0l[HE];
  constexpr int NR = KMAX / 64;  // keys per lane in the softmax
  __shared__ float part[KMAX * CPR];  // per (key, chunk) partial dot products; then the per-lane partial outputs
  __shared__ float pl[KMAX];
  int b, h;
  if (!attn_block(B, H, b, h)) return;
  const int lane = threadIdx.x;
  const int rr = lane / CPR, c = lane - rr * CPR;
  const bool act = rr < RPI;
  const attn_head hd = head_view(qkv, b, h, S, H, HE);
  const int E = hd.E;
  const size_t ld = hd.ld;
  const bf16 *qb = hd.q, *kb = hd.k, *vb = hd.v;
  for (int d = lane; d < HE; d += 64) q0l[d] = vg_bf2f(qb[d]);
  __syncthreads();
  float qc[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) qc[t] = q0l[8 * (act ? c : 0) + t];
  for (int r0 = 0; r0 < S; r0 += RPI) {
    const int r = r0 + rr;
    if (act && r < S) {
      const bf16x8 k8 = *(const bf16x8*)(kb + (size_t)r * ld + 8 * c);
      float a = 0.f;
#pragma unroll
      for (int t = 0; t < 8; ++t) a = fmaf(qc[t], vg_bf2f(k8[t]), a);
      part[r * CPR + c] = a;
    }
  }
  __syncthreads();
  float sv[NR];
#pragma unroll
  for (int rnd = 0; rnd < NR; ++rnd) {
    const int j = lane + 64 * rnd;
    float a = 0.f;
    if (j < S) {
#pragma unroll
      for (int cc = 0; cc < CPR; ++cc) a += part[j * CPR + cc];
    }
    sv[rnd] = (j < S) ? a * scale : -INFINITY;
  }
  float mx = sv[0];
#pragma unroll
  for (int rnd = 1; rnd < NR; ++rnd) mx = fmaxf(mx, sv[rnd]);
  const float m = vg_wave_max(mx);
  float pv[NR], ps = 0.f;
#pragma unroll
  for (int rnd = 0; rnd < NR; ++rnd) { pv[rnd] = __expf(sv[rnd] - m); ps = rnd ? ps + pv[rnd] : pv[rnd]; }  // exp(-inf) = 0 for the padded keys
  const float l = vg_wave_sum(ps);
#pragma unroll
  for (int rnd = 0; rnd < NR; ++rnd) pl[lane + 64 * rnd] = vg_bf2f(vg_f2bf(pv[rnd]));  // the full kernel multiplies V by bf16(p) (an MFMA operand) and divides the fp32 sum by l
  if (lane == 0) lse_cls[(size_t)b * H + h] = m + __logf(l);
  __syncthreads();
  // o[d] = sum_j p_j V[j][d] / l: every lane sums its chunk over its rows, then the RPI row slots are added up through LDS
  float oa[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) oa[t] = 0.f;
  for (int r0 = 0; r0 < S; r0 += RPI) {
    const int r = r0 + rr;
    if (act && r < S) {
      const bf16x8 v8 = *(const bf16x8*)(vb + (size_t)r * ld + 8 * c);
      const float pj = pl[r];
#pragma unroll
      for (int t = 0; t < 8; ++t) oa[t] = fmaf(pj, vg_bf2f(v8[t]), oa[t]);
    }
  }
#pragma unroll
  for (int t = 0; t < 8; ++t) part[lane * 8 + t] = oa[t];
  __syncthreads();
  const float inv_l = 1.0f / l;
  for (int d = lane; d < HE; d += 64) {
    float a = 0.f;
#pragma unroll
    for (int q = 0; q < RPI; ++q) a += part[(q * CPR + (d >> 3)) * 8 + (d & 7)];
    o_cls[(size_t)b * E + h * HE + d] = vg_f2bf(a * inv_l);
  }
}

template <int HE, int KMAX>
__global__ __launch_bounds__(64) void vg_attn_cls_bwd_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ o_cls, const bf16* __restrict__ do_cls,
                                                             const float* __restrict__ lse_cls, bf16* __restrict__ dqkv, int B, int S, int H,
                                                             float scale) {
  constexpr int CPR = HE / 8, RPI = 64 / CPR;
  __shared__ float q0l[HE], d0l[HE];
  __shared__ float ps[KMAX * CPR], pd[KMAX * CPR];  // per (key, chunk) partial dot products q0.K and dO0.V; ps then holds the partial dQ
  __shared__ float dsl[KMAX], pbl[KMAX];
  int b, h;
  if (!attn_block(B, H, b, h)) return;
  const int lane = threadIdx.x;
  const int rr = lane / CPR, c = lane - rr * CPR;
  const bool act = rr < RPI;
  const attn_head hd = head_view(qkv, b, h, S, H, HE);
  const int E = hd.E;
  const size_t ld = hd.ld;
  const bf16 *qb = hd.q, *kb = hd.k, *vb = hd.v;
  bf16* dqb = hd.in_qkv(dqkv);
  const float lse0 = lse_cls[(size_t)b * H + h];
  float dpart = 0.f;  // delta = sum_d dO_0[d] O_0[d]
  for (int d = lane; d < HE; d += 64) {
    q0l[d] = vg_bf2f(qb[d]);
    const float dv = vg_bf2f(do_cls[(size_t)b * E + h * HE + d]);
    d0l[d] = dv;
    dpart = fmaf(dv, vg_bf2f(o_cls[(size_t)b * E + h * HE + d]), dpart);
  }
  const float delta = vg_wave_sum(dpart);
  __syncthreads();
  float qc[8], dc[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) { qc[t] = q0l[8 * (act ? c : 0) + t]; dc[t] = d0l[8 * (act ? c : 0) + t]; }
  for (int r0 = 0; r0 < S; r0 += RPI) {
    const int r = r0 + rr;
    if (act && r < S) {
      const bf16x8 k8 = *(const bf16x8*)(kb + (size_t)r * ld + 8 * c);
      const bf16x8 v8 = *(const bf16x8*)(vb + (size_t)r * ld + 8 * c);
      float a = 0.f, e = 0.f;
#pragma unroll
      for (int t = 0; t < 8; ++t) { a = fmaf(qc[t], vg_bf2f(k8[t]), a); e = fmaf(dc[t], vg_bf2f(v8[t]), e); }
      ps[r * CPR + c] = a;
      pd[r * CPR + c] = e;
    }
  }
  __syncthreads();
#pragma unroll
  for (int rnd = 0; rnd < KMAX / 64; ++rnd) {
    const int j = lane + 64 * rnd;
    float dsv = 0.f, pb = 0.f;
    if (j < S) {
      float sc = 0.f, dp = 0.f;
#pragma unroll
      for (int cc = 0; cc < CPR; ++cc) { sc += ps[j * CPR + cc]; dp += pd[j * CPR + cc]; }
      const float p = __expf(sc * scale - lse0);
      dsv = vg_bf2f(vg_f2bf(p * (dp - delta) * scale));  // bf16: MFMA operands in the full kernel
      pb = vg_bf2f(vg_f2bf(p));
    }
    dsl[j] = dsv;
    pbl[j] = pb;
  }
  __syncthreads();
  // dK_j = ds_j q0, dV_j = p_j dO_0 (rank one in the CLS query); dQ_0 = sum_j ds_j K_j
  float qa[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) qa[t] = 0.f;
  for (int r0 = 0; r0 < S; r0 += RPI) {
    const int r = r0 + rr;
    if (act && r < S) {
      const bf16x8 k8 = *(const bf16x8*)(kb + (size_t)r * ld + 8 * c);
      const float dj = dsl[r], pj = pbl[r];
      bf16x8 dk8, dv8;
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        dk8[t] = vg_f2bf(dj * qc[t]);
        dv8[t] = vg_f2bf(pj * dc[t]);
        qa[t] = fmaf(dj, vg_bf2f(k8[t]), qa[t]);
      }
      bf16* rowp = dqb + (size_t)r * ld + 8 * c;
      *(bf16x8*)(rowp + E) = dk8;
      *(bf16x8*)(rowp + 2 * E) = dv8;
      if (r > 0) *(u32x4*)rowp = (u32x4){0u, 0u, 0u, 0u};  // dQ is zero off the CLS row
    }
  }
#pragma unroll
  for (int t = 0; t < 8; ++t) ps[lane * 8 + t] = qa[t];
  __syncthreads();
  for (int d = lane; d < HE; d += 64) {
    float a = 0.f;
#pragma unroll
    for (int q = 0; q < RPI; ++q) a += ps[(q * CPR + (d >> 3)) * 8 + (d & 7)];
    dqb[d] = vg_f2bf(a);
  }
}

// o_cls / do_cls: [B, E] (the CLS rows, compact); lse_cls: [B, H]; dqkv: the full [B*S, 3E] gradient.  Dot-product scores only
// (the engine keeps the full kernels for the top block when the fp8 mode is on); -3: head dim not 32 / 64 / 96.  S <= 128 runs the
// 128-key instance (half the LDS of the 256-key one: twice the workgroups per CU), 128 < S <= VG_ATTN_LONG_MAX_S the 256-key one.
int vg_attn_cls_fwd_launch(const bf16* qkv, bf16* o_cls, float* lse_cls, int B, int H, int S, int HE, float scale, hipStream_t st) {
  if (S < 1 || S > VG_ATTN_LONG_MAX_S || B < 1 || H < 1) return -2;
  return attn_by_head_dim(HE, [&](auto he) {
    constexpr int HE_ = decltype(he)::value;
    const dim3 grid(attn_grid(B, H));
    if (S <= 128) hipLaunchKernelGGL((vg_attn_cls_fwd_kernel<HE_, 128>), grid, dim3(64), 0, st, qkv, o_cls, lse_cls, B, S, H, scale);
    else hipLaunchKernelGGL((vg_attn_cls_fwd_kernel<HE_, 256>), grid, dim3(64), 0, st, qkv, o_cls, lse_cls, B, S, H, scale);
    return (int)hipGetLastError();
  });
}
int vg_attn_cls_bwd_launch(const bf16* qkv, const bf16* o_cls, const bf16* do_cls, const float* lse_cls, bf16* dqkv, int B, int H, int S, int HE,
                           float scale, hipStream_t st) {
  if (S < 1 || S > VG_ATTN_LONG_MAX_S || B < 1 || H < 1) return -2;
  return attn_by_head_dim(HE, [&](auto he) {
    constexpr int HE_ = decltype(he)::value;
    const dim3 grid(attn_grid(B, H));
    if (S <= 128) hipLaunchKernelGGL((vg_attn_cls_bwd_kernel<HE_, 128>), grid, dim3(64), 0, st, qkv, o_cls, do_cls, lse_cls, dqkv, B, S, H, scale);
    else hipLaunchKernelGGL((vg_attn_cls_bwd_kernel<HE_, 256>), grid, dim3(64), 0, st, qkv, o_cls, do_cls, lse_cls, dqkv, B, S, H, scale);
    return (int)hipGetLastError();
  });
}

// the second-order kernel above (S <= 80: padded to five 16-row tiles); -3: head dim not 32 / 64 / 96
int vg_attn_bwd_bwd_mfma_launch(const bf16* qkv, const bf16* d_o, const float* lse, const bf16* uqkv, bf16* d_do, bf16* d_qkv, int B, int H,
                                int S, int HE, float scale, hipStream_t st) {
  if (S < 1 || S > 80 || B < 1 || H < 1) return -2;
  const void* z = vg_attn_zeros();
  if (!z) return -5;
  return attn_by_head_dim(HE, [&](auto he) {
    hipLaunchKernelGGL((vg_attn_bwd_bwd2_kernel<decltype(he)::value>), dim3(attn_grid(B, H)), dim3(320), 0, st, qkv, d_o, lse, uqkv, d_do, d_qkv, B, S, H, scale, z);
    return (int)hipGetLastError();
  });
}
