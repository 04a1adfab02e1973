// The register epilogue of the bf16 GEMMs that write a bf16 result (gemm.hip, gemm_wr.hip): what happens to one slot - the 8
// consecutive columns of one output row a lane holds behind vg_pair_swap (vg_tile.h) - between the accumulators and memory.
// Both files compile with the default floating-point contraction; the contraction-off files must not include this header.
#pragma once
#include "vg_tile.h"

template <int ACT>
__device__ __forceinline__ float apply_act(float scale, float v) {
  if (ACT == VG_ACT_GELU) return vg_gelu(v);
  if (ACT == VG_ACT_SIN) return __sinf(scale * v);
  if (ACT == VG_ACT_TANH) return vg_tanh(v);
  return v;
}

// What an activation code makes the epilogue read besides the accumulators - asked by vg_epi_slot and by each caller's preloads,
// which must agree: a bf16 slot of Z (MUL_Z8: its 8 byte codes instead), or an fp32 slot of Zf.
constexpr bool vg_act_needs_zbf(int act) { return act == VG_ACT_MUL_GELU_GRAD || act == VG_ACT_MUL_TANH_GRAD || act == VG_ACT_MUL_Z || act == VG_ACT_MUL_Z8; }
constexpr bool vg_act_z8(int act) { return act == VG_ACT_MUL_Z8; }
constexpr bool vg_act_needs_zf(int act) { return act == VG_ACT_MUL_COS; }

// Epilogue operands of one problem.  A kernel copies them out of kernarg memory ONCE, in front of its main loop: a reference
// into kernarg memory is re-read after every store.
struct VgEpi {
  bf16* C; int ldc;
  bf16* C2; int ldc2, c2_gelu_grad;
  float* Cf; int ldcf, pre_f32;
  const bf16* res; const float* resf;  // only tested here: the caller has loaded the addends (pre_bf / pre_f*)
  float act_scale;
  int N;                               // the dropout mask index is (row * drop_row_mul) * N + col
  unsigned drop_thresh, drop_key; float drop_scale; int drop_post, drop_row_mul;
};
__device__ __forceinline__ VgEpi vg_epi_of(const VgGemmProb& P) {
  VgEpi e;
  e.C = P.C; e.ldc = P.ldc;
  e.C2 = P.C2; e.ldc2 = P.ldc2; e.c2_gelu_grad = P.c2_gelu_grad;
  e.Cf = P.Cf; e.ldcf = P.ldcf; e.pre_f32 = P.pre_f32;
  e.res = P.res; e.resf = P.resf;
  e.act_scale = P.act_scale;
  e.N = P.N;
  // the key mixes in a counter loaded from device memory: named uniform here, it lives in a scalar register across the main
  // loop (gemm_wr.hip has no vector register to spare for it; gemm.hip does not need the hint and only its SGPR counts move)
  e.drop_thresh = P.drop.thr; e.drop_key = __builtin_amdgcn_readfirstlane(vg_drop_key(P.drop.key, P.drop.step)); e.drop_scale = P.drop.scale;
  e.drop_post = P.drop_post; e.drop_row_mul = P.drop_row_mul > 1 ? P.drop_row_mul : 1;
  return e;
}

// One slot: v = the 8 bias-added accumulators of columns n .. n + 7 of output row out_row (both in range: the caller checks).
// pre_bf: the slot of Z (ACT = MUL_GELU_GRAD / MUL_TANH_GRAD / MUL_Z; MUL_Z8: its 8 byte codes in the first half) or else of the
// bf16 residual; pre_f0 / pre_f1: the slot of Zf (ACT = MUL_COS) or else of the fp32 addend.
// ISSUES NO GLOBAL LOAD.  vmcnt retires in order, so a load issued behind stores would wait for them: the caller loads the
// operands of a whole group of slots before the group's first call, and places its own waits.  The template parameters are the
// features COMPILED IN; each still tests its runtime operand.
template <int ACT, bool HAS_C2, bool HAS_PREF32, bool HAS_DROP, bool HAS_RES, bool HAS_RESF>
__device__ __forceinline__ void vg_epi_slot(const VgEpi& e, float (&v)[8], bf16x8 pre_bf, f32x4 pre_f0, f32x4 pre_f1, int out_row, int n) {
  constexpr bool NEED_ZBF = vg_act_needs_zbf(ACT), Z8 = vg_act_z8(ACT), NEED_ZF = vg_act_needs_zf(ACT);
  const int mo = out_row;
  if (HAS_PREF32 && e.pre_f32) {
    float* dst = e.Cf + (unsigned)(mo * e.ldcf + n);
    *(f32x4*)dst = (f32x4){v[0], v[1], v[2], v[3]};
    *(f32x4*)(dst + 4) = (f32x4){v[4], v[5], v[6], v[7]};
  }
  float gact[8];  // GELU: activation and derivative share one exp / rcp / polynomial
  if (ACT == VG_ACT_GELU) {
    float gd[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) vg_gelu_both(v[r], gact[r], gd[r]);
    if (HAS_C2 && e.C2) {
      if (e.c2_gelu_grad == 2) {
        const u32x2 c8 = {vg_g8_pack4(gd[0], gd[1], gd[2], gd[3]), vg_g8_pack4(gd[4], gd[5], gd[6], gd[7])};
        *(u32x2*)((unsigned char*)e.C2 + (unsigned)(mo * e.ldc2 + n)) = c8;
      } else {
        bf16x8 o;
#pragma unroll
        for (int r = 0; r < 8; ++r) o[r] = vg_f2bf(e.c2_gelu_grad ? gd[r] : v[r]);
        *(bf16x8*)(e.C2 + (unsigned)(mo * e.ldc2 + n)) = o;
      }
    }
  } else if (HAS_C2 && e.C2) {
    bf16x8 o;
#pragma unroll
    for (int r = 0; r < 8; ++r) o[r] = vg_f2bf(v[r]);
    *(bf16x8*)(e.C2 + (unsigned)(mo * e.ldc2 + n)) = o;
  }
  if (Z8) {
    const u32x4 cv = __builtin_bit_cast(u32x4, pre_bf);
#pragma unroll
    for (int r = 0; r < 4; ++r) { v[r] *= vg_g8_value(cv[0], r); v[r + 4] *= vg_g8_value(cv[1], r); }
  } else if (NEED_ZBF) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const float zv = vg_bf2f(pre_bf[r]);
      v[r] *= (ACT == VG_ACT_MUL_GELU_GRAD) ? vg_gelu_grad(zv) : ((ACT == VG_ACT_MUL_Z) ? zv : (1.f - zv * zv));
    }
  } else if (NEED_ZF) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      v[r] *= e.act_scale * __cosf(e.act_scale * pre_f0[r]);
      v[r + 4] *= e.act_scale * __cosf(e.act_scale * pre_f1[r]);
    }
  } else if (ACT == VG_ACT_GELU) {
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = gact[r];
  } else if (ACT != VG_ACT_NONE) {
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = apply_act<ACT>(e.act_scale, v[r]);
  }
  // dropout: in front of the residual (x + drop(y)), or behind every addend (drop_post: drop(y + pos))
  unsigned dw0 = 0, dw1 = 0;
  if (HAS_DROP && e.drop_thresh) {
    const unsigned i4 = (unsigned)(mo * e.drop_row_mul * e.N + n) >> 2;
    dw0 = vg_drop_word(e.drop_key, i4); dw1 = vg_drop_word(e.drop_key, i4 + 1);
    if (!e.drop_post) {
#pragma unroll
      for (int r = 0; r < 4; ++r) { v[r] *= vg_drop_factor(dw0, r, e.drop_thresh, e.drop_scale); v[r + 4] *= vg_drop_factor(dw1, r, e.drop_thresh, e.drop_scale); }
    }
  }
  if (HAS_RES && !NEED_ZBF && e.res) {
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] += vg_bf2f(pre_bf[r]);
  }
  if (HAS_RESF && !NEED_ZF && e.resf) {
#pragma unroll
    for (int r = 0; r < 4; ++r) { v[r] += pre_f0[r]; v[r + 4] += pre_f1[r]; }
  }
  if (HAS_DROP && e.drop_thresh && e.drop_post) {
#pragma unroll
    for (int r = 0; r < 4; ++r) { v[r] *= vg_drop_factor(dw0, r, e.drop_thresh, e.drop_scale); v[r + 4] *= vg_drop_factor(dw1, r, e.drop_thresh, e.drop_scale); }
  }
  if (e.C) {
    bf16x8 o;
#pragma unroll
    for (int r = 0; r < 8; ++r) o[r] = vg_f2bf(v[r]);
    *(bf16x8*)(e.C + (unsigned)(mo * e.ldc + n)) = o;
  }
}
