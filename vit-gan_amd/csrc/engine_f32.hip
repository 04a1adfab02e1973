// fp32 mode of the v2 VisionTransformer (src/v2/modules.py:67-238): forward, input gradient and weight gradients with fp32
// activations, saved tensors, gradients and GEMM operands, reading the fp32 master P and accumulating into the fp32 gradient
// buffer G of the shared flat layout (vg_vit_layout).  Every row of every block runs (the top block is dense).  One stream; host
// code only enqueues work.  Also the extern "C" single-operator entry points of the mode.
#include "../../include/vitgan_hip.h"
#include "vg_f32.h"
#include "vg_kernels.h"

namespace {

struct F32Ws {
  float *tiles, *tok, *X, *xn1, *qkv, *ao, *xmid, *xn2, *z1, *a1, *lse, *mean1, *rstd1, *mean2, *rstd2;
  float *cn, *meanf, *rstdf, *th;                      // classifier head: normalised CLS rows, tanh(fc1)
  float *g[2], *gm, *gmid, *dz1, *dxn, *dao, *dqkv, *gt, *dtiles, *du, *dcn, *part, *slab;
};

long long lmax(long long a, long long b) { return a > b ? a : b; }

long long carve_f32(const VgVitDims& d, int B, void* base, F32Ws& w) {
  const long long E = d.E, NP = (long long)(d.IH / d.P) * (d.IH / d.P), S = NP + 1, M = (long long)B * S, L = d.L;
  const long long Kp = (long long)d.C * d.P * d.P, rE = (long long)d.R * E, T = (long long)B * NP;
  Carver c{(unsigned char*)base, 0};
  w.tiles = c.take<float>(T * Kp); w.tok = c.take<float>(T * E);
  w.X = c.take<float>((L + 1) * M * E);
  w.xn1 = c.take<float>(L * M * E); w.qkv = c.take<float>(L * M * 3 * E); w.ao = c.take<float>(L * M * E);
  w.xmid = c.take<float>(L * M * E); w.xn2 = c.take<float>(L * M * E);
  w.z1 = c.take<float>(L * M * rE); w.a1 = c.take<float>(L * M * rE);
  w.lse = c.take<float>(L * B * d.H * S);
  w.mean1 = c.take<float>(L * M); w.rstd1 = c.take<float>(L * M); w.mean2 = c.take<float>(L * M); w.rstd2 = c.take<float>(L * M);
  w.cn = c.take<float>(B * E); w.meanf = c.take<float>(B); w.rstdf = c.take<float>(B); w.th = c.take<float>(B * E);
  w.g[0] = c.take<float>(M * E); w.g[1] = c.take<float>(M * E);
  w.gm = c.take<float>(M * E); w.gmid = c.take<float>(M * E); w.dz1 = c.take<float>(M * rE); w.dxn = c.take<float>(M * E); w.dao = c.take<float>(M * E);
  w.dqkv = c.take<float>(M * 3 * E); w.gt = c.take<float>(T * E); w.dtiles = c.take<float>(T * Kp);
  w.du = c.take<float>(B * E); w.dcn = c.take<float>(B * E);
  long long part = (long long)vg_f32_colsum_parts((int)M) * lmax(lmax(3 * E, rE), 2 * E);
  part = lmax(part, (long long)vg_f32_colsum_parts(B) * S * E);
  part = lmax(part, (long long)vg_f32_colsum_parts((int)T) * E);
  w.part = c.take<float>(part);
  long long slab = vg_f32_wgrad_slab_floats((int)M, (int)(3 * E), (int)E);
  slab = lmax(slab, vg_f32_wgrad_slab_floats((int)M, (int)rE, (int)E));
  slab = lmax(slab, vg_f32_wgrad_slab_floats((int)M, (int)E, (int)rE));
  slab = lmax(slab, vg_f32_wgrad_slab_floats((int)T, (int)E, (int)Kp));
  slab = lmax(slab, vg_f32_wgrad_slab_floats(B, (int)E, (int)E));
  slab = lmax(slab, vg_f32_wgrad_slab_floats(B, d.Kc, (int)E));
  w.slab = c.take<float>(slab);
  return c.off;
}

int f32_tokens(const VgVitDims& d) { return (d.IH / d.P) * (d.IH / d.P) + 1; }

int check_net(const VgVitNet* net, int B, VgVitLayout& lay) {
  if (!net || !net->P || B < 1) return -1;
  VG_TRY(vg_vit_layout(&net->d, &lay));
  if (f32_tokens(net->d) > VG_SHORT_MAX_S) return -3;  // the fp32 attention kernels are S <= 80
  if (net->attn_fp8) return -4;
  return 0;
}

}  // namespace

extern "C" long long vg_vit_ws_bytes_f32(const VgVitDims* d, int B) {
  VgVitLayout lay;
  if (!d || B < 1 || vg_vit_layout(d, &lay) || f32_tokens(*d) > VG_SHORT_MAX_S) return -1;
  F32Ws w;
  return carve_f32(*d, B, nullptr, w);
}

extern "C" int vg_vit_forward_f32(const VgVitNet* net, int B, const float* img, void* ws, float* logits, void* stream) {
  if (!net || !img || !ws || !logits) return -1;
  VgVitLayout lay;
  VG_TRY(check_net(net, B, lay));
  const VgVitDims& d = net->d;
  hipStream_t st = (hipStream_t)stream;
  const int E = d.E, NP = (d.IH / d.P) * (d.IH / d.P), S = NP + 1, M = B * S, Kp = d.C * d.P * d.P, rE = d.R * E, HE = E / d.H;
  const long long ME = (long long)M * E;
  F32Ws w; carve_f32(d, B, ws, w);
  const float* P = net->P;
  const Drop dr = {net->dropout_p, net->dropout_seed, net->dropout_step};  // sites: 0 embedding, 1+2l attention, 2+2l MLP

  // patch embedding (modules.py:82-100): per-patch GEMM + bias, + pos_embedding, CLS row, dropout
  VG_TRY(vg_f32_patchify_launch(img, w.tiles, B, d.C, d.IH, d.P, 0, st));
  VG_TRY(vg_f32_linear_fwd(w.tiles, P + lay.conv_w, P + lay.conv_b, nullptr, w.tok, nullptr, B * NP, E, Kp, VG_F32_ACT_NONE, VgDrop(), st));
  VG_TRY(vg_f32_embed_assemble_launch(w.tok, P + lay.pos, P + lay.cls, w.X, B, S, E, dr.at(0), st));

  const float scale = 1.0f / sqrtf((float)HE);
  for (int l = 0; l < d.L; ++l) {  // Encoder.forward (modules.py:178-183), pre-LN
    const float* Pl = P + lay.layer0 + (long long)l * lay.layer_stride;
    float *X = w.X + l * ME, *Xn = w.X + (l + 1) * ME, *xn1 = w.xn1 + l * ME, *qkv = w.qkv + 3 * l * ME, *ao = w.ao + l * ME;
    float *xmid = w.xmid + l * ME, *xn2 = w.xn2 + l * ME, *z1 = w.z1 + (long long)l * M * rE, *a1 = w.a1 + (long long)l * M * rE;
    VG_TRY(vg_f32_ln_fwd_launch(X, E, Pl + lay.ln1_w, Pl + lay.ln1_b, xn1, E, w.mean1 + (long long)l * M, w.rstd1 + (long long)l * M, M, E,
                                1e-5f, st));
    VG_TRY(vg_f32_linear_fwd(xn1, Pl + lay.wqkv, Pl + lay.bqkv, nullptr, qkv, nullptr, M, 3 * E, E, VG_F32_ACT_NONE, VgDrop(), st));
    VG_TRY(vg_f32_attn_fwd_launch(qkv, ao, w.lse + (long long)l * B * d.H * S, B, d.H, S, HE, scale, st));
    VG_TRY(vg_f32_linear_fwd(ao, Pl + lay.wo, Pl + lay.bo, X, xmid, nullptr, M, E, E, VG_F32_ACT_NONE, dr.at(1 + 2 * l), st));
    VG_TRY(vg_f32_ln_fwd_launch(xmid, E, Pl + lay.ln2_w, Pl + lay.ln2_b, xn2, E, w.mean2 + (long long)l * M, w.rstd2 + (long long)l * M, M, E,
                                1e-5f, st));
    VG_TRY(vg_f32_linear_fwd(xn2, Pl + lay.w1, Pl + lay.b1, nullptr, a1, z1, M, rE, E, VG_F32_ACT_GELU, VgDrop(), st));
    VG_TRY(vg_f32_linear_fwd(a1, Pl + lay.w2, Pl + lay.b2, xmid, Xn, nullptr, M, E, rE, VG_F32_ACT_NONE, dr.at(2 + 2 * l), st));
  }
  // final LayerNorm on the CLS rows (the classifier reads x[:, 0], modules.py:195,236), Linear -> Tanh -> Linear
  const float* XL = w.X + (long long)d.L * ME;
  VG_TRY(vg_f32_ln_fwd_launch(XL, (long long)S * E, P + lay.lnf_w, P + lay.lnf_b, w.cn, E, w.meanf, w.rstdf, B, E, 1e-5f, st));
  VG_TRY(vg_f32_linear_fwd(w.cn, P + lay.hw1, P + lay.hb1, nullptr, w.th, nullptr, B, E, E, VG_F32_ACT_TANH, VgDrop(), st));
  return vg_f32_linear_fwd(w.th, P + lay.hw2, P + lay.hb2, nullptr, logits, nullptr, B, d.Kc, E, VG_F32_ACT_NONE, VgDrop(), st);
}

extern "C" int vg_vit_backward_f32(const VgVitNet* net, int B, void* ws, const float* dlogits, float* d_img, int want_wgrad, void* stream) {
  if (!net || !ws || !dlogits) return -1;
  VgVitLayout lay;
  VG_TRY(check_net(net, B, lay));
  if (want_wgrad && !net->G) return -1;
  const VgVitDims& d = net->d;
  hipStream_t st = (hipStream_t)stream;
  const int E = d.E, NP = (d.IH / d.P) * (d.IH / d.P), S = NP + 1, M = B * S, Kp = d.C * d.P * d.P, rE = d.R * E, HE = E / d.H;
  const long long ME = (long long)M * E;
  F32Ws w; carve_f32(d, B, ws, w);
  const float* P = net->P;
  float* G = net->G;
  const Drop dr = {net->dropout_p, net->dropout_seed, net->dropout_step};
  const bool wg = want_wgrad != 0;

  // classifier head
  if (wg) VG_TRY(vg_f32_linear_wgrad(dlogits, w.th, G + lay.hw2, G + lay.hb2, w.slab, B, d.Kc, E, st));
  VG_TRY(vg_f32_linear_dgrad(dlogits, P + lay.hw2, w.th, w.du, B, d.Kc, E, VG_F32_MUL_TANH, st));
  if (wg) VG_TRY(vg_f32_linear_wgrad(w.du, w.cn, G + lay.hw1, G + lay.hb1, w.slab, B, E, E, st));
  VG_TRY(vg_f32_linear_dgrad(w.du, P + lay.hw1, nullptr, w.dcn, B, E, E, VG_F32_ACT_NONE, st));
  // final LayerNorm: dL/dX[L] is the CLS rows' gradient, zero on every other row
  const float* XL = w.X + (long long)d.L * ME;
  VG_TRY(vg_fill_f32_launch(w.g[0], ME, 0.0f, st));  // (a kernel, not hipMemsetAsync: a memset node of a captured graph is not ordered with its neighbours)
  VG_TRY(vg_f32_ln_bwd_launch(w.dcn, XL, (long long)S * E, w.meanf, w.rstdf, P + lay.lnf_w, nullptr, w.g[0], (long long)S * E,
                              wg ? G + lay.lnf_w : nullptr, wg ? G + lay.lnf_b : nullptr, w.part, B, E, st));

  const float scale = 1.0f / sqrtf((float)HE);
  int cur = 0;
  for (int l = d.L - 1; l >= 0; --l) {
    const float* Pl = P + lay.layer0 + (long long)l * lay.layer_stride;
    float* Gl = wg ? G + lay.layer0 + (long long)l * lay.layer_stride : nullptr;
    const float *X = w.X + l * ME, *xn1 = w.xn1 + l * ME, *qkv = w.qkv + 3 * l * ME, *ao = w.ao + l * ME;
    const float *xmid = w.xmid + l * ME, *xn2 = w.xn2 + l * ME, *z1 = w.z1 + (long long)l * M * rE, *a1 = w.a1 + (long long)l * M * rE;
    const float* g = w.g[cur];
    float* gnext = w.g[cur ^ 1];
    // MLP half: X[l+1] = xmid + drop2(fc2(gelu(fc1(norm2(xmid)))))
    const float* gm = g;
    if (dr.on()) { VG_TRY(vg_f32_dropout_launch(g, w.gm, ME, dr.at(2 + 2 * l), st)); gm = w.gm; }
    if (wg) VG_TRY(vg_f32_linear_wgrad(gm, a1, Gl + lay.w2, Gl + lay.b2, w.slab, M, E, rE, st));
    VG_TRY(vg_f32_linear_dgrad(gm, Pl + lay.w2, z1, w.dz1, M, E, rE, VG_F32_MUL_GELU, st));
    if (wg) VG_TRY(vg_f32_linear_wgrad(w.dz1, xn2, Gl + lay.w1, Gl + lay.b1, w.slab, M, rE, E, st));
    VG_TRY(vg_f32_linear_dgrad(w.dz1, Pl + lay.w1, nullptr, w.dxn, M, rE, E, VG_F32_ACT_NONE, st));
    VG_TRY(vg_f32_ln_bwd_launch(w.dxn, xmid, E, w.mean2 + (long long)l * M, w.rstd2 + (long long)l * M, Pl + lay.ln2_w, g, w.gmid, E,
                                wg ? Gl + lay.ln2_w : nullptr, wg ? Gl + lay.ln2_b : nullptr, w.part, M, E, st));
    // attention half: xmid = X + drop1(out_projection(attention(norm1(X))))
    const float* ga = w.gmid;
    if (dr.on()) { VG_TRY(vg_f32_dropout_launch(w.gmid, w.gm, ME, dr.at(1 + 2 * l), st)); ga = w.gm; }
    if (wg) VG_TRY(vg_f32_linear_wgrad(ga, ao, Gl + lay.wo, Gl + lay.bo, w.slab, M, E, E, st));
    VG_TRY(vg_f32_linear_dgrad(ga, Pl + lay.wo, nullptr, w.dao, M, E, E, VG_F32_ACT_NONE, st));
    VG_TRY(vg_f32_attn_bwd_launch(qkv, ao, w.dao, w.lse + (long long)l * B * d.H * S, w.dqkv, B, d.H, S, HE, scale, st));
    if (wg) VG_TRY(vg_f32_linear_wgrad(w.dqkv, xn1, Gl + lay.wqkv, Gl + lay.bqkv, w.slab, M, 3 * E, E, st));
    VG_TRY(vg_f32_linear_dgrad(w.dqkv, Pl + lay.wqkv, nullptr, w.dxn, M, 3 * E, E, VG_F32_ACT_NONE, st));
    VG_TRY(vg_f32_ln_bwd_launch(w.dxn, X, E, w.mean1 + (long long)l * M, w.rstd1 + (long long)l * M, Pl + lay.ln1_w, w.gmid, gnext, E,
                                wg ? Gl + lay.ln1_w : nullptr, wg ? Gl + lay.ln1_b : nullptr, w.part, M, E, st));
    cur ^= 1;
  }
  // patch embedding: dropout, CLS / pos sums over the batch, conv bias and weight, the image
  VG_TRY(vg_f32_embed_grad_launch(w.g[cur], w.gm, w.gt, B, S, E, dr.at(0), st));
  if (wg) {
    VG_TRY(vg_f32_colsum_launch(w.gm, (long long)S * E, B, w.part, G + lay.cls, E, G + lay.pos, NP * E, st));
    VG_TRY(vg_f32_linear_wgrad(w.gt, w.tiles, G + lay.conv_w, G + lay.conv_b, w.slab, B * NP, E, Kp, st));
  }
  if (!d_img) return 0;
  VG_TRY(vg_f32_linear_dgrad(w.gt, P + lay.conv_w, nullptr, w.dtiles, B * NP, E, Kp, VG_F32_ACT_NONE, st));
  return vg_f32_patchify_launch(d_img, w.dtiles, B, d.C, d.IH, d.P, 1, st);
}

// ------------------------------------------------------------------------------------------------------------------------------
// single operators of the fp32 mode
extern "C" int vg_linear_f32_fwd(const float* X, const float* W, const float* bias, const float* res, float* Y, float* Z, int M, int N,
                                 int K, int act, float drop_p, unsigned long long seed, int site, const unsigned* step_dev, void* stream) {
  if (!X || !W || !Y) return -1;
  if (M < 1 || N < 1 || K < 1) return -2;
  if (act < 0 || act > 2 || !vg_drop_p_ok(drop_p)) return -4;
  return vg_f32_linear_fwd(X, W, bias, res, Y, Z, M, N, K, act, vg_drop_site(drop_p, seed, site, step_dev), (hipStream_t)stream);
}
extern "C" int vg_linear_f32_dgrad(const float* dY, const float* W, const float* aux, float* dX, int M, int N, int K, int act, void* stream) {
  if (!dY || !W || !dX || (act != 0 && !aux)) return -1;
  if (M < 1 || N < 1 || K < 1) return -2;
  if (act < 0 || act > 2) return -4;
  const int mode = act == 1 ? VG_F32_MUL_GELU : act == 2 ? VG_F32_MUL_TANH : VG_F32_ACT_NONE;
  return vg_f32_linear_dgrad(dY, W, aux, dX, M, N, K, mode, (hipStream_t)stream);
}
extern "C" long long vg_linear_f32_wgrad_slab_floats(int M, int N, int K) { return vg_f32_wgrad_slab_floats(M, N, K); }
extern "C" int vg_linear_f32_wgrad(const float* dY, const float* X, float* dW, float* db, float* slab, long long slab_floats, int M, int N,
                                   int K, void* stream) {
  if (!dY || !X || !dW || !slab) return -1;
  if (M < 1 || N < 1 || K < 1) return -2;
  if (slab_floats < vg_f32_wgrad_slab_floats(M, N, K)) return -2;
  return vg_f32_linear_wgrad(dY, X, dW, db, slab, M, N, K, (hipStream_t)stream);
}
extern "C" int vg_attention_f32_fwd(const float* qkv, float* out, float* lse, int B, int H, int S, int HE, float scale, void* stream) {
  return vg_f32_attn_fwd_launch(qkv, out, lse, B, H, S, HE, scale, (hipStream_t)stream);
}
extern "C" int vg_attention_f32_bwd(const float* qkv, const float* out, const float* d_out, const float* lse, float* d_qkv, int B, int H,
                                    int S, int HE, float scale, void* stream) {
  return vg_f32_attn_bwd_launch(qkv, out, d_out, lse, d_qkv, B, H, S, HE, scale, (hipStream_t)stream);
}
extern "C" int vg_layernorm_f32_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int R, int E,
                                    float eps, void* stream) {
  return vg_f32_ln_fwd_launch(x, E, gamma, beta, y, E, mean, rstd, R, E, eps, (hipStream_t)stream);
}
extern "C" long long vg_layernorm_f32_bwd_part_floats(int R, int E) {
  if (R < 1 || E < 1) return -2;
  return 2LL * E * vg_f32_colsum_parts(R);
}
extern "C" int vg_layernorm_f32_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, const float* gres,
                                    float* dx, float* dgamma, float* dbeta, float* part, int R, int E, void* stream) {
  return vg_f32_ln_bwd_launch(dy, x, E, mean, rstd, gamma, gres, dx, E, dgamma, dbeta, part, R, E, (hipStream_t)stream);
}
