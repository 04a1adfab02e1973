// extern "C" single-operator entry points of include/vitgan_hip.h (thin argument adapters).
#include "../../include/vitgan_hip.h"
#include "vg_kernels.h"
#include "vg_row.h"
#include "vg_chain.h"
#include "vg_spectral.h"
#include <algorithm>
#include <cstring>
#include <vector>

extern "C" int vg_abi_version(void) { return VG_ABI_VERSION; }

extern "C" int vg_linear_fwd(const void* A, const void* W, const float* bias, const void* res, void* C, void* pre_bf16,
                             float* pre_f32, int M, int N, int K, int act, float act_scale, void* stream) {
  if (!A || !W || (!C && !pre_bf16 && !pre_f32)) return -1;
  if (act < 0 || act > 3) return -4;
  VgGemmProb p = vg_gemm_prob();
  p.A = (const bf16*)A; p.lda = K; p.B = (const bf16*)W; p.ldb = K; p.M = M; p.N = N; p.K = K;
  p.C = (bf16*)C; p.ldc = N; p.bias = bias; p.res = (const bf16*)res; p.ldr = N; p.C2 = (bf16*)pre_bf16; p.ldc2 = N;
  if (pre_f32) { p.pre_f32 = 1; p.Cf = pre_f32; p.ldcf = N; }
  p.act = act; p.act_scale = act_scale;
  return vg_gemm_launch(&p, 1, VG_NT, (hipStream_t)stream);
}
extern "C" int vg_linear_gelu_fwd(const void* A, const void* W, const float* bias, void* C, void* dcode, int M, int N, int K, void* stream) {
  if (!A || !W || !C || !dcode) return -1;
  VgGemmProb p = vg_gemm_prob();
  p.A = (const bf16*)A; p.lda = K; p.B = (const bf16*)W; p.ldb = K; p.M = M; p.N = N; p.K = K;
  p.C = (bf16*)C; p.ldc = N; p.bias = bias; p.C2 = (bf16*)dcode; p.ldc2 = N; p.c2_gelu_grad = 2; p.act = VG_ACT_GELU;
  return vg_gemm_launch(&p, 1, VG_NT, (hipStream_t)stream);
}
extern "C" int vg_linear_dgrad(const void* dY, const void* W, void* dX, int M, int N, int K, int mul_mode, const void* Z,
                               const float* Zf, float act_scale, void* stream) {
  if (!dY || !W || !dX) return -1;
  if (mul_mode != 0 && mul_mode != VG_ACT_MUL_GELU_GRAD && mul_mode != VG_ACT_MUL_COS && mul_mode != VG_ACT_MUL_TANH_GRAD && mul_mode != VG_ACT_MUL_Z && mul_mode != VG_ACT_MUL_Z8) return -4;
  if (((mul_mode == VG_ACT_MUL_GELU_GRAD || mul_mode == VG_ACT_MUL_TANH_GRAD || mul_mode == VG_ACT_MUL_Z || mul_mode == VG_ACT_MUL_Z8) && !Z) || (mul_mode == VG_ACT_MUL_COS && !Zf)) return -1;
  VgGemmProb p = vg_gemm_prob();
  p.A = (const bf16*)dY; p.lda = N; p.B = (const bf16*)W; p.ldb = K; p.M = M; p.N = K; p.K = N;
  p.C = (bf16*)dX; p.ldc = K; p.act = mul_mode; p.act_scale = act_scale;
  p.Z = (const bf16*)Z; p.ldz = K; p.Zf = Zf; p.ldzf = K;
  return vg_gemm_launch(&p, 1, VG_NN, (hipStream_t)stream);
}
extern "C" long long vg_linear_wgrad_slab_floats(int N, int K, int splits) {
  if (N < 1 || K < 1 || splits < 1 || splits > VG_WGRAD_MAX_SPLITS) return -2;
  return (long long)splits * N * K;
}
extern "C" int vg_linear_wgrad(const void* dY, const void* X, float* dW, float* slab_ws, long long slab_floats, int M, int N, int K,
                               int splits, int accumulate, void* stream) {
  if (!dY || !X || !dW || !slab_ws) return -1;
  const long long need = vg_linear_wgrad_slab_floats(N, K, splits);
  if (need < 0 || slab_floats < need || M < 1) return -2;  // the K slices are written at slab_ws + s*N*K: never past the caller's buffer
  VgGemmProb p = vg_gemm_prob();
  p.A = (const bf16*)dY; p.lda = N; p.B = (const bf16*)X; p.ldb = K; p.M = N; p.N = K; p.K = M;
  p.Cf = slab_ws; p.ldcf = K; p.cf_split_stride = (long long)N * K; p.splits = splits;
  VG_TRY(vg_gemm_launch(&p, 1, VG_TN, (hipStream_t)stream));
  return vg_slab_reduce_launch(slab_ws, (long long)N * K, p.splits, dW, (long long)N * K, accumulate, (hipStream_t)stream);
}
// Several weight gradients that share their row count as ONE grouped split-K launch and ONE fold: problem j writes its K slices at
// slab_ws + off[j] (+ s * region_floats per slice), the regions [off[j], off[j] + N[j] K[j]) must tile [0, region_floats) exactly -
// the layout of a block's weights in the flat gradient buffer - and dst[0 .. region_floats) (+)= the folded slices.
extern "C" int vg_linear_wgrad_group(int n, const void* const* dY, const void* const* X, const int* N, const int* K, const long long* off,
                                     int M, int splits, float* slab_ws, long long slab_floats, float* dst, long long region_floats,
                                     int accumulate, void* stream) {
  if (n < 1 || n > 8 || !dY || !X || !N || !K || !off || !slab_ws || !dst) return -1;
  if (M < 1 || splits < 1 || splits > VG_WGRAD_MAX_SPLITS || region_floats < 1) return -2;
  if (slab_floats < (long long)splits * region_floats) return -2;
  int order[8];
  for (int i = 0; i < n; ++i) order[i] = i;
  for (int i = 1; i < n; ++i)  // insertion sort by offset
    for (int j = i; j > 0 && off[order[j]] < off[order[j - 1]]; --j) { const int t = order[j]; order[j] = order[j - 1]; order[j - 1] = t; }
  long long at = 0;
  for (int i = 0; i < n; ++i) {
    const int j = order[i];
    if (!dY[j] || !X[j]) return -1;
    if (N[j] < 1 || K[j] < 1 || off[j] != at) return -2;  // a gap would fold uninitialised slab memory into dst, an overlap would race
    at += (long long)N[j] * K[j];
  }
  if (at != region_floats) return -2;
  VgGemmProb pr[8];
  for (int j = 0; j < n; ++j) {
    VgGemmProb p = vg_gemm_prob();
    p.A = (const bf16*)dY[j]; p.lda = N[j]; p.B = (const bf16*)X[j]; p.ldb = K[j]; p.M = N[j]; p.N = K[j]; p.K = M;
    p.Cf = slab_ws + off[j]; p.ldcf = K[j]; p.cf_split_stride = region_floats; p.splits = splits;
    pr[j] = p;
  }
  VG_TRY(vg_gemm_launch(pr, n, VG_TN, (hipStream_t)stream));
  return vg_slab_reduce_launch(slab_ws, region_floats, pr[0].splits, dst, region_floats, accumulate, (hipStream_t)stream);
}
extern "C" int vg_layernorm_fwd(const void* x, long long xs, const float* gamma, const float* beta, void* y, long long ys,
                                float* mean, float* rstd, int R, int E, float eps, void* stream) {
  if (!x || !gamma || !beta || !y || !mean || !rstd) return -1;
  return vg_ln_fwd_launch((const bf16*)x, xs, gamma, beta, (bf16*)y, ys, mean, rstd, R, E, eps, (hipStream_t)stream);
}
extern "C" int vg_layernorm_bwd_parts(int R) { return vg_ln_bwd_nparts(R); }
extern "C" int vg_layernorm_bwd(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                                const void* gres, void* dx, float* part, int R, int E, void* stream) {
  if (!dy || !x || !mean || !rstd || !gamma || !dx || !part) return -1;
  return vg_ln_bwd_launch((const bf16*)dy, (const bf16*)x, mean, rstd, gamma, (const bf16*)gres, (bf16*)dx, part, R, E,
                          nullptr, VgDrop(), (hipStream_t)stream);
}
extern "C" int vg_sln_fwd(const void* h, int h_bcast_rows, const void* w, const float* lw, const float* lb, const float* gs,
                          const float* bs, void* y, float* mean, float* rstd, int R, int E, float eps, void* stream) {
  if (!h || !w || !lw || !lb || !gs || !bs || !y || !mean || !rstd) return -1;
  return vg_sln_fwd_launch((const bf16*)h, h_bcast_rows, (const bf16*)w, lw, lb, gs, bs, (bf16*)y, mean, rstd, R, E, eps,
                           (hipStream_t)stream);
}
extern "C" int vg_sln_bwd(const void* dy, const void* h, int h_bcast_rows, const void* w, const float* mean, const float* rstd,
                          const float* lw, const float* lb, const float* gs, const float* bs, const void* gres, void* dh,
                          float* dw_acc, int dw_accumulate, float* part, int R, int E, void* stream) {
  if (!dy || !h || !w || !mean || !rstd || !lw || !lb || !gs || !bs || !dh || !dw_acc || !part) return -1;
  return vg_sln_bwd_launch((const bf16*)dy, (const bf16*)h, h_bcast_rows, (const bf16*)w, mean, rstd, lw, lb, gs, bs,
                           (const bf16*)gres, (bf16*)dh, dw_acc, dw_accumulate, part, R, E, nullptr, VgDrop(), (hipStream_t)stream);
}
extern "C" int vg_colsum_f32(const float* part, int rows, int width, float* d0, int n0, float* d1, int n1, float* d2, int n2,
                             float* d3, int n3, int accumulate, void* stream) {
  if (!part || rows < 1 || width < 1) return -1;
  return vg_colsum_f32_launch(part, rows, width, d0, n0, d1, n1, d2, n2, d3, n3, accumulate, (hipStream_t)stream);
}
extern "C" int vg_colsum_bf16_parts(int R) { return vg_colsum_bf16_nparts(R); }
extern "C" int vg_colsum_bf16(const void* X, long long ld, int R, int N, float* part_ws, float* dst, int accumulate, void* stream) {
  if (!X || !part_ws || !dst) return -1;
  return vg_colsum_bf16_launch((const bf16*)X, ld, R, N, part_ws, dst, accumulate, (hipStream_t)stream);
}
// (every entry that carries a mask makes its site with vg_drop_site, vg_common.h)
extern "C" int vg_dropout_apply(const void* x, void* y, long long n, float p, unsigned long long seed, int site,
                                const unsigned* step_dev, void* stream) {
  if (!x || !y || n < 1 || !vg_drop_p_ok(p)) return -1;
  return vg_dropout_apply_launch((const bf16*)x, (bf16*)y, n, vg_drop_site(p, seed, site, step_dev), (hipStream_t)stream);
}
// ---- the kernels at the two ends of the networks, one by one (elementwise.hip; tests/test_ends_gpu.py).  Every null pointer and every
// shape is refused by the launcher, before any launch; the mask-carrying entries refuse a probability outside [0, 1) here (-1).
extern "C" int vg_head_fwd(const void* t, const float* W2, const float* b2, float* logits, int B, int E, int Kc, void* stream) {
  return vg_head_fc2_launch((const bf16*)t, W2, b2, logits, B, E, Kc, (hipStream_t)stream);
}
// (vg_head_bwd_parts and vg_head_bwd_part_width are the launcher's own helpers, exported as they are: vg_kernels.h)
extern "C" int vg_head_bwd(const float* dlogits, const float* W2, const void* t, void* dz, float* dW2, float* db2, float* part, int B, int E, int Kc,
                           int want_wgrad, void* stream) {
  return vg_head_bwd_launch(dlogits, W2, (const bf16*)t, (bf16*)dz, dW2, db2, B, E, Kc, want_wgrad, (hipStream_t)stream, part);
}
extern "C" int vg_batch_sum(const void* g, float* out, int B, int S, int E, void* stream) {
  return vg_batch_sum_launch((const bf16*)g, out, B, S, E, (hipStream_t)stream);
}
extern "C" int vg_embed_small_grads(const float* tok_sum, float* d_cls, float* d_pos, float* d_bias, int S, int E, void* stream) {
  return vg_embed_small_grads_launch(tok_sum, d_cls, d_pos, d_bias, S, E, (hipStream_t)stream);
}
extern "C" int vg_take_rows(const void* in, void* out, int B, int S, int first, int n_take, int E, void* stream) {
  return vg_take_rows_launch((const bf16*)in, (bf16*)out, B, S, first, n_take, E, (hipStream_t)stream);
}
extern "C" int vg_scatter_cls(const void* src, void* g, void* gm, int B, int S, int E, float p, unsigned long long seed, int site,
                              const unsigned* step_dev, void* stream) {
  if (!vg_drop_p_ok(p)) return -1;
  return vg_scatter_cls_launch((const bf16*)src, (bf16*)g, B, S, E, (hipStream_t)stream, (bf16*)gm, vg_drop_site(p, seed, site, step_dev));
}
extern "C" int vg_scatter_cls_pair(const void* src_a, void* dst_a, const void* src_b, void* dst_b, int B, int S, int E, void* stream) {
  return vg_scatter_cls2_launch((const bf16*)src_a, (bf16*)dst_a, (const bf16*)src_b, (bf16*)dst_b, B, S, E, (hipStream_t)stream);
}
extern "C" int vg_fill_cls(void* x, const float* cls, int B, int S, int E, float p, unsigned long long seed, int site, const unsigned* step_dev,
                           void* stream) {
  if (!vg_drop_p_ok(p)) return -1;
  return vg_fill_cls_launch((bf16*)x, cls, B, S, E, vg_drop_site(p, seed, site, step_dev), (hipStream_t)stream);
}
extern "C" int vg_patchify(const void* img, int img_is_bf16, void* A, int B, int C, int IH, int P, void* stream) {
  return vg_patchify_launch(img, img_is_bf16, (bf16*)A, B, C, IH, P, (hipStream_t)stream);
}
extern "C" int vg_unpatchify(const void* dA, void* d_img, int B, int C, int IH, int P, void* stream) {
  return vg_unpatchify_launch((const bf16*)dA, (bf16*)d_img, B, C, IH, P, (hipStream_t)stream);
}
extern "C" int vg_slab_reduce(const float* slab, long long stride, int nslab, float* dst, long long n, int accumulate, void* stream) {
  return vg_slab_reduce_launch(slab, stride, nslab, dst, n, accumulate, (hipStream_t)stream);
}
extern "C" int vg_slab_reduce_pair(const float* slab0, const float* slab1, long long stride, int nslab, float* dst0, float* dst1, long long n,
                                   int accumulate, void* stream) {
  return vg_slab_reduce2_launch(slab0, slab1, stride, nslab, dst0, dst1, n, accumulate, (hipStream_t)stream);
}
extern "C" int vg_sin_grad(const void* dy, const float* z, void* dz, long long n, float w0, void* stream) {
  return vg_sin_grad_launch((const bf16*)dy, z, (bf16*)dz, n, w0, (hipStream_t)stream);
}
extern "C" int vg_add_table(void* x, const float* table, long long rows, int E, int period, void* stream) {
  return vg_add_table_launch((bf16*)x, table, rows, E, period, (hipStream_t)stream);
}
// ---- full-row Linear + LayerNorm (gemm_row.hip) ----
extern "C" long long vg_row_pack_elems_e(int E, int K) { return (!vg_row_width_ok(E) || K < 32 || (K & 31)) ? -2 : (long long)E * K; }
extern "C" long long vg_row_pack_elems(int K) { return vg_row_pack_elems_e(VG_ROW_N, K); }
extern "C" int vg_row_pack_weight_e(int E, const void* W, int ld, int K, int transposed, void* Wp, void* stream) {
  if (!W || !Wp) return -1;
  if (!vg_row_width_ok(E)) return -3;
  VgPackJobs pj;
  pj.N = E;
  pj.src = (const bf16*)W; pj.dst = (bf16*)Wp; pj.src_stride = 0; pj.dst_stride = 0; pj.nblocks = 1; pj.n = 1;
  pj.d[0] = {0, 0, K, ld, transposed ? 1 : 0};
  return vg_pack_rows_launch(pj, (hipStream_t)stream);
}
extern "C" int vg_row_pack_weight(const void* W, int ld, int K, int transposed, void* Wp, void* stream) {
  return vg_row_pack_weight_e(VG_ROW_N, W, ld, K, transposed, Wp, stream);
}
extern "C" int vg_row_parts(int M) { return vg_row_nwg(M); }
// the row and chain launchers answer 1 = enqueued, 0 = not of the kernel's kind, < 0 = -hipError: as a return code
static inline int row_status(int r) { return r > 0 ? 0 : (r < 0 ? -r : -3); }
extern "C" int vg_linear_ln_fwd_e(int E, const void* A, const void* Wp, const float* bias, const void* res, void* Y, void* Yn, float* mean,
                                float* rstd, const float* gamma, const float* beta, int M, int K, float eps, float drop_p,
                                unsigned long long seed, int site, const unsigned* step_dev, void* stream) {
  if (!vg_row_width_ok(E)) return -3;
  if (!A || !Wp || !Y || (Yn && (!mean || !rstd || !gamma || !beta)) || !vg_drop_p_ok(drop_p)) return -1;
  VgRowArgs ra = {};
  ra.N = E;
  ra.A = (const bf16*)A; ra.lda = K; ra.Wp = (const bf16*)Wp; ra.M = M; ra.K = K; ra.bias = bias; ra.res = (const bf16*)res;
  ra.Y = (bf16*)Y; ra.Yn = (bf16*)Yn; ra.mean_out = mean; ra.rstd_out = rstd; ra.gamma = gamma; ra.beta = beta; ra.eps = eps;
  ra.drop = vg_drop_site(drop_p, seed, site, step_dev);
  return row_status(vg_gemm_row_launch(ra, VG_ROW_LNFWD, (hipStream_t)stream));
}
extern "C" int vg_linear_ln_fwd(const void* A, const void* Wp, const float* bias, const void* res, void* Y, void* Yn, float* mean,
                                float* rstd, const float* gamma, const float* beta, int M, int K, float eps, float drop_p,
                                unsigned long long seed, int site, const unsigned* step_dev, void* stream) {
  return vg_linear_ln_fwd_e(VG_ROW_N, A, Wp, bias, res, Y, Yn, mean, rstd, gamma, beta, M, K, eps, drop_p, seed, site, step_dev, stream);
}
extern "C" long long vg_encoder_mlp_image_elems(void) { return (long long)VG_CH_MLP_STAGES * VG_CH_STAGE / 2; }
extern "C" int vg_encoder_mlp_pack(const void* W1, const void* W2, void* img, void* stream) {
  return vg_chain_mlp_pack_launch((const bf16*)W1, (const bf16*)W2, (bf16*)img, VG_CH_KNAT, (hipStream_t)stream);
}
extern "C" int vg_encoder_mlp_fwd(const void* xn, const void* img, const float* b1, const float* b2, const void* res, void* a1,
                                  void* dcode, void* Y, void* Yn, float* mean, float* rstd, const float* gamma, const float* beta,
                                  int M, float eps, float drop_p, unsigned long long seed, int site, const unsigned* step_dev,
                                  void* stream) {
  if (!xn || !img || !b1 || !b2 || !a1 || !dcode || !Y || (Yn && (!mean || !rstd || !gamma || !beta)) || !vg_drop_p_ok(drop_p)) return -1;
  VgChainMlpArgs ca = {};
  ca.xn = (const bf16*)xn; ca.ldx = VG_CH_E; ca.img = (const bf16*)img; ca.b1 = b1; ca.b2 = b2; ca.res = (const bf16*)res;
  ca.a1 = (bf16*)a1; ca.z8 = (unsigned char*)dcode; ca.Y = (bf16*)Y; ca.Yn = (bf16*)Yn; ca.mean_out = mean; ca.rstd_out = rstd;
  ca.gamma = gamma; ca.beta = beta; ca.eps = eps; ca.M = M;
  ca.drop = vg_drop_site(drop_p, seed, site, step_dev);
  return row_status(vg_chain_mlp_fwd_launch(ca, (hipStream_t)stream));
}
extern "C" long long vg_encoder_post_attention_image_elems(void) { return (long long)(VG_CH_MLP_STAGES + VG_CH_FRONT_STAGES) * VG_CH_STAGE / 2; }
extern "C" int vg_encoder_post_attention_pack(const void* Wo, const void* W1, const void* W2, void* img, void* stream) {
  return vg_chain_block_pack_launch((const bf16*)Wo, (const bf16*)W1, (const bf16*)W2, (bf16*)img, (hipStream_t)stream);
}
extern "C" int vg_encoder_post_attention_fwd(const void* ao, const void* x, const void* img, const float* bo, const float* b1, const float* b2,
                                             const float* gamma2, const float* beta2, const float* gamma, const float* beta, void* xmid, void* xn2,
                                             float* mean2, float* rstd2, void* a1, void* dcode, void* Y, void* Yn, float* mean, float* rstd, int M,
                                             float eps, float drop_p, unsigned long long seed, int site_attn, int site_mlp,
                                             const unsigned* step_dev, void* stream) {
  if (!ao || !x || !img || !b1 || !b2 || !gamma2 || !beta2 || !xmid || !xn2 || !mean2 || !rstd2 || !a1 || !dcode || !Y ||
      (Yn && (!mean || !rstd || !gamma || !beta)) || !vg_drop_p_ok(drop_p))
    return -1;
  VgChainMlpArgs ca = {};
  ca.ao = (const bf16*)ao; ca.xin = (const bf16*)x; ca.ldx = VG_CH_E; ca.img = (const bf16*)img; ca.bo = bo; ca.b1 = b1; ca.b2 = b2;
  ca.gamma2 = gamma2; ca.beta2 = beta2; ca.xmid = (bf16*)xmid; ca.xn_out = (bf16*)xn2; ca.mean2 = mean2; ca.rstd2 = rstd2;
  ca.a1 = (bf16*)a1; ca.z8 = (unsigned char*)dcode; ca.Y = (bf16*)Y; ca.Yn = (bf16*)Yn; ca.mean_out = mean; ca.rstd_out = rstd;
  ca.gamma = gamma; ca.beta = beta; ca.eps = eps; ca.M = M;
  ca.drop = vg_drop_site(drop_p, seed, site_mlp, step_dev); ca.drop_key_a = vg_site_key(seed, site_attn);
  return row_status(vg_chain_mlp_fwd_launch(ca, (hipStream_t)stream));
}
extern "C" int vg_linear_sln_fwd_e(int E, const void* A, const void* Wp, const float* bias, const void* res, const float* resf, int res_period,
                                 void* Y, void* Yn, float* mean, float* rstd, const void* wmod, const float* lw, const float* lb,
                                 const float* gs, const float* bs, int M, int K, float eps, float drop_p, unsigned long long seed,
                                 int site, const unsigned* step_dev, void* stream) {
  if (!vg_row_width_ok(E)) return -3;
  if (!A || !Wp || !Y || !Yn || !mean || !rstd || !wmod || !lw || !lb || !gs || !bs || !vg_drop_p_ok(drop_p)) return -1;
  if (res && resf) return -1;
  VgRowArgs ra = {};
  ra.N = E;
  ra.A = (const bf16*)A; ra.lda = K; ra.Wp = (const bf16*)Wp; ra.M = M; ra.K = K; ra.bias = bias; ra.res = (const bf16*)res;
  ra.resf = resf; ra.res_period = res_period;
  ra.Y = (bf16*)Y; ra.Yn = (bf16*)Yn; ra.mean_out = mean; ra.rstd_out = rstd; ra.gamma = lw; ra.beta = lb; ra.eps = eps;
  ra.wmod = (const bf16*)wmod; ra.gs = gs; ra.bs = bs;
  ra.drop = vg_drop_site(drop_p, seed, site, step_dev);
  return row_status(vg_gemm_row_launch(ra, VG_ROW_LNFWD, (hipStream_t)stream));
}
extern "C" int vg_linear_sln_fwd(const void* A, const void* Wp, const float* bias, const void* res, const float* resf, int res_period,
                                 void* Y, void* Yn, float* mean, float* rstd, const void* wmod, const float* lw, const float* lb,
                                 const float* gs, const float* bs, int M, int K, float eps, float drop_p, unsigned long long seed,
                                 int site, const unsigned* step_dev, void* stream) {
  return vg_linear_sln_fwd_e(VG_ROW_N, A, Wp, bias, res, resf, res_period, Y, Yn, mean, rstd, wmod, lw, lb, gs, bs, M, K, eps, drop_p, seed, site, step_dev, stream);
}
extern "C" int vg_linear_dgrad_sln_bwd_e(int E, const void* dY, const void* WpT, const void* h, int h_bcast_rows, const void* wmod,
                                       const float* mean, const float* rstd, const float* lw, const float* lb, const float* gs,
                                       const float* bs, const void* gres, void* dh, void* dhm, float* dw_acc, int dw_accumulate,
                                       float* part, int M, int K, float drop_p, unsigned long long seed, int site,
                                       const unsigned* step_dev, void* stream) {
  if (!vg_row_width_ok(E)) return -3;
  if (!dY || !WpT || !h || !wmod || !mean || !rstd || !lw || !lb || !gs || !bs || !dh || !dw_acc || !part || !vg_drop_p_ok(drop_p))
    return -1;
  VgRowArgs ra = {};
  ra.N = E;
  ra.A = (const bf16*)dY; ra.lda = K; ra.Wp = (const bf16*)WpT; ra.M = M; ra.K = K; ra.x = (const bf16*)h; ra.x_period = h_bcast_rows;
  ra.mean = mean; ra.rstd = rstd; ra.gamma = lw; ra.lbias = lb; ra.gs = gs; ra.bs = bs; ra.wmod = (const bf16*)wmod;
  ra.gres = (const bf16*)gres; ra.dx = (bf16*)dh; ra.dxm = (bf16*)dhm; ra.dw_acc = dw_acc; ra.dw_accumulate = dw_accumulate; ra.part = part;
  if (dhm) ra.drop = vg_drop_site(drop_p, seed, site, step_dev);
  return row_status(vg_gemm_row_launch(ra, VG_ROW_LNBWD, (hipStream_t)stream));
}
extern "C" int vg_linear_dgrad_sln_bwd(const void* dY, const void* WpT, const void* h, int h_bcast_rows, const void* wmod,
                                       const float* mean, const float* rstd, const float* lw, const float* lb, const float* gs,
                                       const float* bs, const void* gres, void* dh, void* dhm, float* dw_acc, int dw_accumulate,
                                       float* part, int M, int K, float drop_p, unsigned long long seed, int site,
                                       const unsigned* step_dev, void* stream) {
  return vg_linear_dgrad_sln_bwd_e(VG_ROW_N, dY, WpT, h, h_bcast_rows, wmod, mean, rstd, lw, lb, gs, bs, gres, dh, dhm, dw_acc, dw_accumulate, part, M, K, drop_p, seed, site, step_dev, stream);
}
extern "C" int vg_linear_dgrad_ln_bwd_e(int E, const void* dY, const void* WpT, const void* x, const float* mean, const float* rstd,
                                      const float* gamma, const void* gres, void* dx, void* dxm, float* part, int M, int K,
                                      float drop_p, unsigned long long seed, int site, const unsigned* step_dev, void* stream) {
  if (!vg_row_width_ok(E)) return -3;
  if (!dY || !WpT || !x || !mean || !rstd || !gamma || !dx || !part || !vg_drop_p_ok(drop_p)) return -1;
  VgRowArgs ra = {};
  ra.N = E;
  ra.A = (const bf16*)dY; ra.lda = K; ra.Wp = (const bf16*)WpT; ra.M = M; ra.K = K; ra.x = (const bf16*)x; ra.mean = mean; ra.rstd = rstd;
  ra.gamma = gamma; ra.gres = (const bf16*)gres; ra.dx = (bf16*)dx; ra.dxm = (bf16*)dxm; ra.part = part;
  if (dxm) ra.drop = vg_drop_site(drop_p, seed, site, step_dev);
  return row_status(vg_gemm_row_launch(ra, VG_ROW_LNBWD, (hipStream_t)stream));
}
extern "C" int vg_linear_dgrad_ln_bwd(const void* dY, const void* WpT, const void* x, const float* mean, const float* rstd,
                                      const float* gamma, const void* gres, void* dx, void* dxm, float* part, int M, int K,
                                      float drop_p, unsigned long long seed, int site, const unsigned* step_dev, void* stream) {
  return vg_linear_dgrad_ln_bwd_e(VG_ROW_N, dY, WpT, x, mean, rstd, gamma, gres, dx, dxm, part, M, K, drop_p, seed, site, step_dev, stream);
}
extern "C" int vg_attention_fwd(const void* qkv, void* out, float* lse, int B, int H, int S, int HE, float scale, void* stream) {
  if (!qkv || !out || !lse) return -1;
  return vg_attn_fwd_launch((const bf16*)qkv, (bf16*)out, lse, B, H, S, HE, scale, 0, (hipStream_t)stream);
}
extern "C" int vg_attention_cls_fwd(const void* qkv, void* out_cls, float* lse_cls, int B, int H, int S, int HE, float scale, void* stream) {
  if (!qkv || !out_cls || !lse_cls) return -1;
  return vg_attn_cls_fwd_launch((const bf16*)qkv, (bf16*)out_cls, lse_cls, B, H, S, HE, scale, (hipStream_t)stream);
}
extern "C" int vg_attention_cls_bwd(const void* qkv, const void* out_cls, const void* d_out_cls, const float* lse_cls, void* d_qkv, int B, int H,
                                    int S, int HE, float scale, void* stream) {
  if (!qkv || !out_cls || !d_out_cls || !lse_cls || !d_qkv) return -1;
  return vg_attn_cls_bwd_launch((const bf16*)qkv, (const bf16*)out_cls, (const bf16*)d_out_cls, lse_cls, (bf16*)d_qkv, B, H, S, HE, scale,
                                (hipStream_t)stream);
}
extern "C" int vg_attention_bwd(const void* qkv, const void* out, const void* d_out, const float* lse, void* d_qkv, int B, int H,
                                int S, int HE, float scale, void* stream) {
  if (!qkv || !out || !d_out || !lse || !d_qkv) return -1;
  return vg_attn_bwd_launch((const bf16*)qkv, (const bf16*)out, (const bf16*)d_out, lse, (bf16*)d_qkv, B, H, S, HE, scale, 0,
                            (hipStream_t)stream);
}
extern "C" int vg_attention_fp8_fwd(const void* qkv, void* out, float* lse, int B, int H, int S, int HE, float scale, void* stream) {
  if (!qkv || !out || !lse) return -1;
  return vg_attn_fwd_launch((const bf16*)qkv, (bf16*)out, lse, B, H, S, HE, scale, 2, (hipStream_t)stream);
}
extern "C" int vg_attention_fp8_bwd(const void* qkv, const void* out, const void* d_out, const float* lse, void* d_qkv, int B, int H,
                                    int S, int HE, float scale, void* stream) {
  if (!qkv || !out || !d_out || !lse || !d_qkv) return -1;
  return vg_attn_bwd_launch((const bf16*)qkv, (const bf16*)out, (const bf16*)d_out, lse, (bf16*)d_qkv, B, H, S, HE, scale, 2,
                            (hipStream_t)stream);
}
extern "C" int vg_attention_l2_fwd(const void* qkv, void* out, float* lse, int B, int H, int S, int HE, float scale, void* stream) {
  if (!qkv || !out || !lse) return -1;
  return vg_attn_fwd_launch((const bf16*)qkv, (bf16*)out, lse, B, H, S, HE, scale, 1, (hipStream_t)stream);
}
extern "C" int vg_attention_l2_bwd(const void* qkv, const void* out, const void* d_out, const float* lse, void* d_qkv, int B, int H,
                                   int S, int HE, float scale, void* stream) {
  if (!qkv || !out || !d_out || !lse || !d_qkv) return -1;
  return vg_attn_bwd_launch((const bf16*)qkv, (const bf16*)out, (const bf16*)d_out, lse, (bf16*)d_qkv, B, H, S, HE, scale, 1,
                            (hipStream_t)stream);
}
extern "C" int vg_unfold_tokens_fwd(const void* img, int img_is_bf16, void* tokens, int B, int C, int IH, int P, int overlap, void* stream) {
  if (!img || !tokens || B < 1 || C < 1) return -1;
  return vg_unfold_tokens_launch(img, img_is_bf16, (bf16*)tokens, B, C, IH, P, overlap, (hipStream_t)stream);
}
extern "C" int vg_unfold_tokens_bwd(const void* d_tokens, void* d_img, int B, int C, int IH, int P, int overlap, void* stream) {
  if (!d_tokens || !d_img || B < 1 || C < 1) return -1;
  return vg_unfold_tokens_bwd_launch((const bf16*)d_tokens, (bf16*)d_img, B, C, IH, P, overlap, (hipStream_t)stream);
}
extern "C" int vg_act_fwd(const void* h, void* y, long long n, int act, void* stream) {
  if (!h || !y || n < 1) return -1;
  return vg_act2_launch((const bf16*)h, nullptr, nullptr, (bf16*)y, nullptr, n, act, 0, (hipStream_t)stream);
}
extern "C" int vg_act_bwd(const void* dy, const void* h, void* dh, long long n, int act, void* stream) {
  if (!dy || !h || !dh || n < 1) return -1;
  return vg_act2_launch((const bf16*)h, (const bf16*)dy, nullptr, (bf16*)dh, nullptr, n, act, 1, (hipStream_t)stream);
}
extern "C" int vg_act_bwd_bwd(const void* u, const void* dy, const void* h, void* d_dy, void* d_h, long long n, int act, void* stream) {
  if (!u || !dy || !h || !d_dy || !d_h || n < 1) return -1;
  return vg_act2_launch((const bf16*)h, (const bf16*)dy, (const bf16*)u, (bf16*)d_dy, (bf16*)d_h, n, act, 2, (hipStream_t)stream);
}
extern "C" int vg_layernorm_bwd_bwd_parts(int R) { return vg_ln_bwd_bwd_nparts(R); }
extern "C" int vg_layernorm_bwd_bwd(const void* u, const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                                    void* d_dy, void* d_x, float* part, int R, int E, void* stream) {
  if (!u || !dy || !x || !mean || !rstd || !gamma || !d_dy || !d_x || !part) return -1;
  return vg_ln_bwd_bwd_launch((const bf16*)u, (const bf16*)dy, (const bf16*)x, mean, rstd, gamma, (bf16*)d_dy, (bf16*)d_x, part, R, E,
                              (hipStream_t)stream);
}
extern "C" int vg_attention_bwd_bwd(const void* qkv, const void* d_out, const float* lse, const void* u_qkv, void* d_d_out, void* d_qkv2,
                                    int B, int H, int S, int HE, float scale, void* stream) {
  if (!qkv || !d_out || !lse || !u_qkv || !d_d_out || !d_qkv2) return -1;
  return vg_attn_bwd_bwd_launch((const bf16*)qkv, (const bf16*)d_out, lse, (const bf16*)u_qkv, (bf16*)d_d_out, (bf16*)d_qkv2, B, H, S, HE,
                                scale, (hipStream_t)stream);
}
extern "C" int vg_gan_loss(const float* logits, float* dlogits, float* loss_out, int n, int kind, int role, float grad_scale,
                           void* stream) {
  if (!logits || !dlogits || !loss_out || n < 1) return -1;
  return vg_gan_loss_launch(logits, dlogits, loss_out, n, kind, role, grad_scale, (hipStream_t)stream);
}
extern "C" int vg_zero_tick(float* g, long long n, int* step_dev, void* stream) {
  if (!g) return -1;
  return vg_zero_tick_launch(g, n, step_dev, (hipStream_t)stream);
}
extern "C" int vg_step_inputs(const float* real, void* imgs_bf16, long long n_img, float* z, long long n_z, unsigned long long seed,
                              const int* step_dev, void* stream) {
  if ((!real && !z) || (real && !imgs_bf16)) return -1;
  return vg_step_inputs_launch(real, (bf16*)imgs_bf16, n_img, z, n_z, seed, step_dev, (hipStream_t)stream);
}
extern "C" int vg_gan_loss_pair(const float* logits, float* dlogits, float* loss_out, int n0, int role0, int n1, int role1, int kind,
                                float grad_scale, void* stream) {
  if (!logits || !dlogits || !loss_out) return -1;
  return vg_gan_loss_pair_launch(logits, dlogits, loss_out, n0, role0, n1, role1, kind, grad_scale, (hipStream_t)stream);
}
extern "C" int vg_bcr_loss(const float* logits_x, const float* logits_a, float* dlog_x, float* dlog_a, float* loss_out, int B_real, int B_fake,
                           int Kc, float w_real, float w_fake, int accumulate_x, int accumulate_a, float grad_scale, void* stream) {
  if (!logits_x || !logits_a || !dlog_x || !dlog_a || !loss_out || B_real < 1 || B_fake < 1 || Kc < 1) return -1;
  return vg_bcr_loss_launch(logits_x, logits_a, dlog_x, dlog_a, loss_out, B_real, B_fake, Kc, w_real, w_fake, accumulate_x, accumulate_a,
                            grad_scale, (hipStream_t)stream);
}
extern "C" int vg_adamw_step(float* p, const float* g, float* m, float* v, void* shadow_bf16, long long n, float lr, float beta1,
                             float beta2, float eps, float weight_decay, int step, const int* step_dev, float gscale,
                             void* stream) {
  if (!p || !g || !m || !v || !shadow_bf16 || n < 1 || (step < 1 && !step_dev)) return -1;
  return vg_adamw_launch(p, g, m, v, (bf16*)shadow_bf16, n, lr, beta1, beta2, eps, weight_decay, step, step_dev, gscale,
                         (hipStream_t)stream);
}
extern "C" int vg_adamw_ema_step(float* p, const float* g, float* m, float* v, void* shadow_bf16, float* ema, long long n, float lr,
                                 float beta1, float beta2, float eps, float weight_decay, int step, const int* step_dev, float gscale,
                                 float ema_decay, int ema_start, void* stream) {
  if (!p || !g || !m || !v || !shadow_bf16 || !ema || n < 1 || (step < 1 && !step_dev)) return -1;
  return vg_adamw_ema_launch(p, g, m, v, (bf16*)shadow_bf16, ema, n, lr, beta1, beta2, eps, weight_decay, step, step_dev, gscale, ema_decay,
                             ema_start, (hipStream_t)stream);
}
// ---- device-resident learning rate: AdamW reading lr_dev[0], and the schedule controller that writes it (elementwise.hip) ----
extern "C" int vg_adamw_step_dlr(float* p, const float* g, float* m, float* v, void* shadow_bf16, long long n, const float* lr_dev, float beta1,
                                 float beta2, float eps, float weight_decay, int step, const int* step_dev, float gscale, void* stream) {
  if (!p || !g || !m || !v || !shadow_bf16 || !lr_dev || n < 1 || (step < 1 && !step_dev)) return -1;
  return vg_adamw_dlr_launch(p, g, m, v, (bf16*)shadow_bf16, n, lr_dev, beta1, beta2, eps, weight_decay, step, step_dev, gscale,
                             (hipStream_t)stream);
}
extern "C" int vg_adamw_ema_step_dlr(float* p, const float* g, float* m, float* v, void* shadow_bf16, float* ema, long long n,
                                     const float* lr_dev, float beta1, float beta2, float eps, float weight_decay, int step,
                                     const int* step_dev, float gscale, float ema_decay, int ema_start, void* stream) {
  if (!p || !g || !m || !v || !shadow_bf16 || !ema || !lr_dev || n < 1 || (step < 1 && !step_dev)) return -1;
  return vg_adamw_ema_dlr_launch(p, g, m, v, (bf16*)shadow_bf16, ema, n, lr_dev, beta1, beta2, eps, weight_decay, step, step_dev, gscale,
                                 ema_decay, ema_start, (hipStream_t)stream);
}
extern "C" int vg_lr_schedule(const VgLrSched* d, const VgLrSched* g, const int* step_dev, const float* scale_dev, float* lr_out, void* stream) {
  return vg_lr_schedule_launch(d, g, step_dev, scale_dev, lr_out, (hipStream_t)stream);
}
extern "C" int vg_ema_update(float* ema, const float* p, long long n, float ema_decay, int ema_start, int step, const int* step_dev,
                             void* stream) {
  if (!ema || !p || n < 1 || (step < 1 && !step_dev)) return -1;
  return vg_ema_launch(ema, p, n, ema_decay, ema_start, step, step_dev, (hipStream_t)stream);
}
// ---- spectral normalisation (spectral.hip)
extern "C" int vg_spectral_plan(VgSpectralDesc* table_host, int n, long long* state_floats, long long* scratch_floats) {
  if (!table_host || n < 1) return -1;
  return vg_spectral_plan_host(table_host, n, state_floats, scratch_floats, nullptr);
}
// every argument error of vg_spectral_update / vg_spectral_project (see the header); blocks receives the three grid sizes
static int spectral_check(const VgSpectralDesc* th, int n, long long total, long long state_floats, long long scratch_floats, int* blocks) {
  std::vector<VgSpectralDesc> plan(th, th + n);
  long long need_state = 0, need_scratch = 0;
  const int rc = vg_spectral_plan_host(plan.data(), n, &need_state, &need_scratch, blocks);
  if (rc != 0) return rc;
  if (std::memcmp(plan.data(), th, sizeof(VgSpectralDesc) * (size_t)n) != 0) return -2;
  if (state_floats < need_state || scratch_floats < need_scratch) return -2;
  std::vector<std::pair<long long, long long>> r((size_t)n);
  for (int i = 0; i < n; ++i) {
    const long long nk = (long long)th[i].N * th[i].K;
    if (nk > total || th[i].w_off > total - nk) return -2;
    r[(size_t)i] = {th[i].w_off, th[i].w_off + nk};
  }
  std::sort(r.begin(), r.end());
  for (int i = 1; i < n; ++i)
    if (r[(size_t)i].first < r[(size_t)i - 1].second) return -3;
  return 0;
}
static inline bool misaligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) != 0; }
extern "C" int vg_spectral_update(const float* W, void* shadow_bf16, long long total, float* state, long long state_floats, float* scratch,
                                  long long scratch_floats, const VgSpectralDesc* table_host, const VgSpectralDesc* table_dev, int n, int iterate,
                                  void* stream) {
  if (!W || !shadow_bf16 || !state || !scratch || !table_host || !table_dev || n < 1) return -1;
  if (iterate != 0 && iterate != 1) return -4;
  int blocks[3];
  VG_TRY(spectral_check(table_host, n, total, state_floats, scratch_floats, blocks));
  if (misaligned(W, 16) || misaligned(state, 16) || misaligned(scratch, 16) || misaligned(shadow_bf16, 8)) return -3;
  return vg_spectral_update_launch(W, (bf16*)shadow_bf16, state, scratch, table_dev, n, blocks, iterate, (hipStream_t)stream);
}
extern "C" int vg_spectral_project(float* G, const float* W, long long total, const float* state, long long state_floats, float* scratch,
                                   long long scratch_floats, const VgSpectralDesc* table_host, const VgSpectralDesc* table_dev, int n,
                                   void* stream) {
  if (!G || !W || !state || !scratch || !table_host || !table_dev || n < 1) return -1;
  int blocks[3];
  VG_TRY(spectral_check(table_host, n, total, state_floats, scratch_floats, blocks));
  if (misaligned(G, 16) || misaligned(W, 16) || misaligned(state, 16) || misaligned(scratch, 16)) return -3;
  return vg_spectral_project_launch(G, W, state, scratch, table_dev, n, blocks, (hipStream_t)stream);
}
extern "C" int vg_diversity_loss(const void* images, void* d_images, float* loss_out, float* scratch, int B, int D, float weight,
                                void* stream) {
  if (!images || !loss_out || !scratch) return -1;
  return vg_diversity_launch((const bf16*)images, (bf16*)d_images, loss_out, scratch, B, D, weight, (hipStream_t)stream);
}
extern "C" int vg_grad_clip(float* g, long long n, float gscale, float max_norm, float* scratch, void* stream) {
  if (!g || !scratch || n < 1 || !(max_norm > 0.f)) return -1;
  return vg_grad_clip_launch(g, n, gscale, max_norm, scratch, (hipStream_t)stream);
}
extern "C" int vg_cast_f32_bf16(const float* src, void* dst_bf16, long long n, void* stream) {
  if (!src || !dst_bf16 || n < 1) return -1;
  return vg_cast_f32_bf16_launch(src, (bf16*)dst_bf16, n, (hipStream_t)stream);
}
// ---- differentiable augmentation (augment.hip) ----
static int vg_diffaug_args(const void* a, const void* b, int B, int C, int IH, int policy) {
  if (!a || !b || B < 1) return -1;
  if (policy < 0 || policy > 7 || C < 1 || IH < 8 || IH > 255) return -2;
  if (((long long)C * IH * IH) & 7) return -3;
  return 0;
}
extern "C" int vg_diffaug_fwd(const void* x, void* y, float* params_out, int B, int C, int IH, int policy, unsigned long long seed, int site,
                              const unsigned* step_dev, void* stream) {
  VG_TRY(vg_diffaug_args(x, y, B, C, IH, policy));
  return vg_diffaug_fwd_launch((const bf16*)x, (bf16*)y, params_out, B, C, IH, policy, vg_site_key(seed, site), step_dev, (hipStream_t)stream);
}
extern "C" int vg_diffaug_bwd(const void* dy, void* dx, int accumulate, int B, int C, int IH, int policy, unsigned long long seed, int site,
                              const unsigned* step_dev, void* stream) {
  VG_TRY(vg_diffaug_args(dy, dx, B, C, IH, policy));
  return vg_diffaug_bwd_launch((const bf16*)dy, (bf16*)dx, accumulate, B, C, IH, policy, vg_site_key(seed, site), step_dev, (hipStream_t)stream);
}
// the gated forms: every member of the policy applied per image with probability prob_dev[0] (read on the device)
extern "C" int vg_diffaug_p_fwd(const void* x, void* y, float* params_out, int B, int C, int IH, int policy, unsigned long long seed, int site,
                                const unsigned* step_dev, const float* prob_dev, void* stream) {
  VG_TRY(vg_diffaug_args(x, y, B, C, IH, policy));
  if (!prob_dev) return -1;
  return vg_diffaug_fwd_launch((const bf16*)x, (bf16*)y, params_out, B, C, IH, policy, vg_site_key(seed, site), step_dev, (hipStream_t)stream,
                               prob_dev);
}
extern "C" int vg_diffaug_p_bwd(const void* dy, void* dx, int accumulate, int B, int C, int IH, int policy, unsigned long long seed, int site,
                                const unsigned* step_dev, const float* prob_dev, void* stream) {
  VG_TRY(vg_diffaug_args(dy, dx, B, C, IH, policy));
  if (!prob_dev) return -1;
  return vg_diffaug_bwd_launch((const bf16*)dy, (bf16*)dx, accumulate, B, C, IH, policy, vg_site_key(seed, site), step_dev, (hipStream_t)stream,
                               prob_dev);
}
// ---- adaptive discriminator augmentation: the controller (elementwise.hip) ----
extern "C" int vg_ada_update(const float* logits_real, int n, float* state, float target, float step_per_image, int interval, const int* step_dev,
                             void* stream) {
  return vg_ada_update_launch(logits_real, n, state, target, step_per_image, interval, step_dev, (hipStream_t)stream);
}
// ---- class conditioning (elementwise.hip): every argument error comes back from the launchers before any launch ----
extern "C" int vg_draw_labels(int* labels, int n, int K, unsigned long long seed, int site, const unsigned* step_dev, void* stream) {
  return vg_draw_labels_launch(labels, n, K, vg_site_key(seed, site), step_dev, (hipStream_t)stream);
}
extern "C" int vg_class_add(void* wmod_bf16, const void* table_bf16, const int* labels, int B, int N, int K, void* stream) {
  return vg_class_add_launch((bf16*)wmod_bf16, (const bf16*)table_bf16, labels, B, N, K, (hipStream_t)stream);
}
extern "C" int vg_class_grad(const float* dw, const int* labels, float* dtable, int B, int N, int K, int accumulate, void* stream) {
  return vg_class_grad_launch(dw, labels, dtable, B, N, K, accumulate, (hipStream_t)stream);
}
extern "C" int vg_gan_loss_cond(const float* logits, const int* labels, float* dlogits, float* selected, float* loss_out, int n, int Kc, int kind,
                                int role, float grad_scale, void* stream) {
  return vg_gan_loss_cond_launch(logits, labels, dlogits, selected, loss_out, Kc, n, role, 0, 0, kind, grad_scale, (hipStream_t)stream);
}
extern "C" int vg_gan_loss_cond_pair(const float* logits, const int* labels, float* dlogits, float* selected, float* loss_out, int n0, int role0,
                                     int n1, int role1, int Kc, int kind, float grad_scale, void* stream) {
  if (n1 < 1) return -1;
  return vg_gan_loss_cond_launch(logits, labels, dlogits, selected, loss_out, Kc, n0, role0, n1, role1, kind, grad_scale, (hipStream_t)stream);
}
