/*
 * vitgan_hip.h - C ABI of libvitgan_hip.so, the MI355X (gfx950) compute library under the
 * ViTGAN nn.Module surface.
 *
 * The reference (krzkro4122/vit-gan) is pure Python on PyTorch ATen ops and has no FFI / operator
 * plugin interface of its own; its boundary for the hot path is the nn.Module surface
 * of src/v2/modules.py plus the step body of src/v2/training.py:170-211.  Each entry point below
 * names the reference code whose ATen call sequence it replaces.  The Python side binds these with
 * ctypes (vit-gan_amd/_lib.py); INTEGRATION.md shows the binding a maintainer of the reference adds.
 *
 * Conventions
 *   - plain pointers + sizes only; every pointer is DEVICE memory unless it says "host";
 *   - `bf16` tensors are passed as `void*` (2-byte IEEE bfloat16, row-major);
 *   - `stream` is a hipStream_t passed as void*; every call only ENQUEUES work on it (no host
 *     synchronisation, no allocation), so callers may capture a sequence of calls in a hipGraph;
 *   - return value: 0 on success, a positive hipError_t, or a negative argument-validation code
 *     (-1 bad count, -2 bad size, -3 unsupported shape/alignment, -4 bad mode).  Nothing is
 *     launched when the return value is negative.
 *   - ownership: the caller owns all memory; the library keeps no state between calls.
 */
#ifndef VITGAN_HIP_H
#define VITGAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VG_ABI_VERSION 9
int vg_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Single operators (parity-tested one by one; tests/test_ops_gpu.py)
 * ---------------------------------------------------------------------------------------- */

/* nn.Linear forward (+ fused epilogue):  C[M,N] = act(A[M,K] @ W[N,K]^T + bias) + res
 * replaces F.linear / nn.GELU / residual add of src/v2/modules.py:128-139,161,179-182 and
 * sin(30*Linear) of src/v1/siren.py:44-45.
 * act: 0 none, 1 GELU(erf), 2 sin(act_scale*v), 3 tanh.  bias fp32 [N] or NULL; res bf16 [M,N]
 * or NULL; pre_bf16 (bf16 [M,N]) / pre_f32 (fp32 [M,N]) receive the pre-activation or NULL. */
int vg_linear_fwd(const void* A, const void* W, const float* bias, const void* res, void* C,
                  void* pre_bf16, float* pre_f32, int M, int N, int K, int act, float act_scale,
                  void* stream);
/* fc1 of the encoder MLP as the engine runs it (src/v2/modules.py:128-139: Linear -> nn.GELU):  C = gelu(A W^T + bias) in bf16,
 * and dcode[M,N] = gelu'(A W^T + bias) as ONE BYTE per element: code = round(200 g) + 27 (27 <-> 0 and 227 <-> 1 exactly,
 * |error| <= 0.0025 over gelu's derivative range [-0.129, 1.129]) - all the backward keeps of the pre-activation.  N % 8 == 0. */
int vg_linear_gelu_fwd(const void* A, const void* W, const float* bias, void* C, void* dcode, int M, int N, int K,
                       void* stream);
/* input gradient of nn.Linear:  dX[M,K] = dY[M,N] @ W[N,K]   (autograd of F.linear)
 * mul_mode 0: none; 4: dX *= gelu'(Z) with Z bf16 [M,K]; 5: dX *= s*cos(s*Zf), Zf fp32 [M,K];
 * 6: dX *= 1 - Z^2 (Z = tanh output, bf16 [M,K]); 7: dX *= Z (Z = a derivative the forward stored, bf16 [M,K]:
 * 8: dX *= decode(Z), Z the byte codes [M,K] written by vg_linear_gelu_fwd - what the engine's fc2 input gradient uses). */
int vg_linear_dgrad(const void* dY, const void* W, void* dX, int M, int N, int K, int mul_mode,
                    const void* Z, const float* Zf, float act_scale, void* stream);
/* weight gradient of nn.Linear:  dW[N,K] (+)= dY[M,N]^T @ X[M,K], computed as `splits` slices of M
 * into fp32 slabs folded in a fixed order (deterministic).  slab_ws holds slab_floats floats and must be at
 * least vg_linear_wgrad_slab_floats(N, K, splits) = splits*N*K: a smaller workspace, or splits outside
 * [1, VG_WGRAD_MAX_SPLITS], returns -2 and launches nothing. */
#define VG_WGRAD_MAX_SPLITS 64
long long vg_linear_wgrad_slab_floats(int N, int K, int splits); /* host only; -2 for a bad argument */
int vg_linear_wgrad(const void* dY, const void* X, float* dW, float* slab_ws, long long slab_floats, int M,
                    int N, int K, int splits, int accumulate, void* stream);
/* n <= 8 weight gradients over the same M rows as ONE grouped split-K launch and ONE fold (ABI v7; what the gradient penalty's
 * double backward uses for a block's four Linears, src/v2/utils.py:124-144 through autograd of src/v2/modules.py:128-139,173-182):
 * problem j's slices go to slab_ws + off[j] + s*region_floats, the regions [off[j], off[j] + N[j]*K[j]) must tile
 * [0, region_floats) exactly (-2 otherwise: a gap would fold uninitialised memory), dst[0..region_floats) (+)= the fold. */
int vg_linear_wgrad_group(int n, const void* const* dY, const void* const* X, const int* N, const int* K, const long long* off,
                          int M, int splits, float* slab_ws, long long slab_floats, float* dst, long long region_floats,
                          int accumulate, void* stream);

/* nn.LayerNorm forward/backward (src/v2/modules.py:168,172,225; eps 1e-5, biased variance).
 * x,y bf16 [R,E] with row strides xs/ys (elements); mean/rstd fp32 [R]. E % 128 == 0, E <= 1024. */
int vg_layernorm_fwd(const void* x, long long xs, const float* gamma, const float* beta, void* y,
                     long long ys, float* mean, float* rstd, int R, int E, float eps, void* stream);
/* dx = (gres ? gres : 0) + LN'(dy).  part: fp32 [vg_layernorm_bwd_parts(R)][3E] scratch holding per
 * workgroup column sums (d gamma | d beta | colsum(dx)); fold with vg_colsum_f32. */
int vg_layernorm_bwd_parts(int R);
int vg_layernorm_bwd(const void* dy, const void* x, const float* mean, const float* rstd,
                     const float* gamma, const void* gres, void* dx, float* part, int R, int E,
                     void* stream);
/* Self-modulated LayerNorm (src/v1/spectral_layer_norm.py:19-20): y = w*(gs*(LN(h)*lw+lb)+bs).
 * h_bcast_rows > 0: h has that many rows and is broadcast over the batch (generator.py:62). */
int vg_sln_fwd(const void* h, int h_bcast_rows, const void* w, const float* lw, const float* lb,
               const float* gs, const float* bs, void* y, float* mean, float* rstd, int R, int E,
               float eps, void* stream);
/* part: fp32 [parts][3E+64]: d lw | d lb | colsum(dh) | d gs, d bs.  dw_acc fp32 [R,E]. */
int vg_sln_bwd(const void* dy, const void* h, int h_bcast_rows, const void* w, const float* mean,
               const float* rstd, const float* lw, const float* lb, const float* gs, const float* bs,
               const void* gres, void* dh, float* dw_acc, int dw_accumulate, float* part, int R,
               int E, void* stream);
/* Linear + LayerNorm in ONE kernel, for the Linears whose output is the embedding width 384 (rows owned whole by a
 * workgroup, statistics in the epilogue; csrc/gemm_row.hip).  M % 16 == 0, K % 64 == 0, K >= 128; other shapes return -3
 * (vg_row_parts(M) == 0 says so beforehand) and the caller uses vg_linear_* + vg_layernorm_*.
 * The weight operand is PACKED first: Wp = vg_row_pack_weight(W): [K/32][384][32] stage images, vg_row_pack_elems(K) bf16;
 *   transposed = 0: W is [384, K] row-major with leading dimension ld (nn.Linear weight whose out_features is 384: forward);
 *   transposed = 1: W is [K, 384] (nn.Linear weight whose in_features is 384: its input gradient dX = dY W).
 * vg_linear_ln_fwd:  Y = res + drop(A Wp^T + bias);  Yn = LayerNorm(Y) * gamma + beta, mean / rstd of Y   (Yn NULL: Y only)
 *   replaces out_projection / fc2 + dropout + residual add + the LayerNorm that reads the sum (src/v2/modules.py:168,172,179-183).
 *   drop(.) is dropout site `site` of (drop_p, seed) as in vg_dropout_apply (drop_p = 0: none).
 * vg_linear_dgrad_ln_bwd:  dx = gres + LayerNorm'(dY Wp);  dxm = dx * mask(site) (NULL: none);
 *   part: fp32 [vg_row_parts(M)][3*384] per-workgroup column sums d gamma | d beta | colsum(dxm ? dxm : dx), fold with vg_colsum_f32
 *   replaces autograd of queries|keys|values / fc1 and of the LayerNorm in front of them (modules.py:178-181). */
long long vg_row_pack_elems(int K); /* host only */
int vg_row_pack_weight(const void* W, int ld, int K, int transposed, void* Wp, void* stream);
int vg_row_parts(int M);            /* host only */
int vg_linear_ln_fwd(const void* A, const void* Wp, const float* bias, const void* res, void* Y, void* Yn, float* mean,
                     float* rstd, const float* gamma, const float* beta, int M, int K, float eps, float drop_p,
                     unsigned long long seed, int site, const unsigned* step_dev, void* stream);
int vg_linear_dgrad_ln_bwd(const void* dY, const void* WpT, const void* x, const float* mean, const float* rstd,
                           const float* gamma, const void* gres, void* dx, void* dxm, float* part, int M, int K,
                           float drop_p, unsigned long long seed, int site, const unsigned* step_dev, void* stream);

/* The same entry points for another embedding width (round 4; E = 384 or 512 - C4's width; anything else returns -3, and
 * vg_row_pack_elems_e -2): every [M, 384] operand above is [M, E], packed images are [K/32][E][32], partial rows 3 E (+ 64) wide.
 * E = 768 (C5) does not fit the kernel's LDS ring (one 32-deep stage of W alone is 48 KiB) and stays on vg_linear_* + vg_layernorm_*. */
long long vg_row_pack_elems_e(int E, int K); /* host only */
int vg_row_pack_weight_e(int E, const void* W, int ld, int K, int transposed, void* Wp, void* stream);
int vg_linear_ln_fwd_e(int E, const void* A, const void* Wp, const float* bias, const void* res, void* Y, void* Yn, float* mean,
                       float* rstd, const float* gamma, const float* beta, int M, int K, float eps, float drop_p,
                       unsigned long long seed, int site, const unsigned* step_dev, void* stream);
int vg_linear_dgrad_ln_bwd_e(int E, const void* dY, const void* WpT, const void* x, const float* mean, const float* rstd,
                             const float* gamma, const void* gres, void* dx, void* dxm, float* part, int M, int K,
                             float drop_p, unsigned long long seed, int site, const unsigned* step_dev, void* stream);
int vg_linear_sln_fwd_e(int E, const void* A, const void* Wp, const float* bias, const void* res, const float* resf, int res_period,
                        void* Y, void* Yn, float* mean, float* rstd, const void* wmod, const float* lw, const float* lb,
                        const float* gs, const float* bs, int M, int K, float eps, float drop_p, unsigned long long seed,
                        int site, const unsigned* step_dev, void* stream);
int vg_linear_dgrad_sln_bwd_e(int E, const void* dY, const void* WpT, const void* h, int h_bcast_rows, const void* wmod,
                              const float* mean, const float* rstd, const float* lw, const float* lb, const float* gs,
                              const float* bs, const void* gres, void* dh, void* dhm, float* dw_acc, int dw_accumulate,
                              float* part, int M, int K, float drop_p, unsigned long long seed, int site,
                              const unsigned* step_dev, void* stream);

/* The MLP half of an encoder block as ONE launch (csrc/chain.hip; E = 384, hidden 768):
 *   a1 = gelu(xn W1^T + b1);  Y = res + drop(a1 W2^T + b2);  Yn = LayerNorm(Y) * gamma + beta, mean / rstd of Y   (Yn NULL: Y only)
 * replaces fc1 -> nn.GELU -> fc2 -> dropout -> residual add of src/v2/modules.py:181-182 and the LayerNorm that reads the sum
 * (the next block's norm1, :168 / :178).  A wave keeps its 16 rows in registers for the whole chain: the hidden a1 [M,768] and
 * dcode [M,768] (gelu' as byte codes, as vg_linear_gelu_fwd) are written for the backward and never read back.
 * The weights come as a chain image: img = vg_encoder_mlp_pack(W1 [768,384], W2 [384,768]), vg_encoder_mlp_image_elems() bf16.
 * M % 16 == 0; other shapes return -3 and the caller uses vg_linear_gelu_fwd + vg_linear_ln_fwd.  drop(.) as in vg_linear_ln_fwd. */
long long vg_encoder_mlp_image_elems(void); /* host only */
int vg_encoder_mlp_pack(const void* W1, const void* W2, void* img, void* stream);
int vg_encoder_mlp_fwd(const void* xn, const void* img, const float* b1, const float* b2, const void* res, void* a1, void* dcode,
                       void* Y, void* Yn, float* mean, float* rstd, const float* gamma, const float* beta, int M, float eps,
                       float drop_p, unsigned long long seed, int site, const unsigned* step_dev, void* stream);

/* Everything of an encoder block BETWEEN its attention and the next block's, but for the QKV projection, as ONE launch (csrc/chain.hip, the MLP
 * chain with the out-projection in front):
 *   x_mid = x + drop_a(ao Wo^T + bo);  xn2 = LayerNorm2(x_mid);  a1 = gelu(xn2 W1^T + b1);  Y = x_mid + drop_m(a1 W2^T + b2);  Yn = LayerNorm(Y)
 * replaces out_projection + dropout1 + residual, norm2, fc1, nn.GELU, fc2 + dropout2 + residual (src/v2/modules.py:179-182) and the next block's
 * norm1 (:168).  x_mid, xn2 (+ mean2 / rstd2), a1, dcode, Y, Yn (+ mean / rstd) are written for the backward; none is read back.
 * img = vg_encoder_post_attention_pack(Wo [384,384], W1 [768,384], W2 [384,768]).  M % 16 == 0.  An operator with its tests and measurements
 * (DESIGN.md s3); the engine does not call it. */
long long vg_encoder_post_attention_image_elems(void); /* host only */
int vg_encoder_post_attention_pack(const void* Wo, const void* W1, const void* W2, void* img, void* stream);
int vg_encoder_post_attention_fwd(const void* ao, const void* x, const void* img, const float* bo, const float* b1, const float* b2,
                                  const float* gamma2, const float* beta2, const float* gamma, const float* beta, void* xmid, void* xn2,
                                  float* mean2, float* rstd2, void* a1, void* dcode, void* Y, void* Yn, float* mean, float* rstd, int M,
                                  float eps, float drop_p, unsigned long long seed, int site_attn, int site_mlp,
                                  const unsigned* step_dev, void* stream);

/* The same two kernels with the v1 generator's self-modulated LayerNorm (src/v1/spectral_layer_norm.py:19-20) in the epilogue:
 * vg_linear_sln_fwd:  Y = (res | resf[row % res_period]) + drop(A Wp^T + bias);  Yn = w * (gs * (LN(Y) * lw + lb) + bs)
 *   replaces output_linear / the block MLP + dropout + residual + the SLN that reads the sum (src/v1/transformer.py:85-88);
 *   resf: fp32 [res_period, 384] residual broadcast over the batch (block 0: the learned embedding, generator.py:62), or NULL.
 * vg_linear_dgrad_sln_bwd:  dh = gres + LN'(dy_eff), dy_eff = (dY Wp) * w * gs;  dhm = dh * mask(site) (NULL: none);
 *   dw_acc (+)= (dY Wp) * (gs * (xhat * lw + lb) + bs)  (fp32 [M,384]);  part: fp32 [vg_row_parts(M)][3*384 + 64]:
 *   d lw | d lb | colsum(dhm ? dhm : dh) | d gs, d bs;  h_bcast_rows > 0: h has that many rows, broadcast over the batch. */
int vg_linear_sln_fwd(const void* A, const void* Wp, const float* bias, const void* res, const float* resf, int res_period,
                      void* Y, void* Yn, float* mean, float* rstd, const void* wmod, const float* lw, const float* lb,
                      const float* gs, const float* bs, int M, int K, float eps, float drop_p, unsigned long long seed,
                      int site, const unsigned* step_dev, void* stream);
int vg_linear_dgrad_sln_bwd(const void* dY, const void* WpT, const void* h, int h_bcast_rows, const void* wmod,
                            const float* mean, const float* rstd, const float* lw, const float* lb, const float* gs,
                            const float* bs, const void* gres, void* dh, void* dhm, float* dw_acc, int dw_accumulate,
                            float* part, int M, int K, float drop_p, unsigned long long seed, int site,
                            const unsigned* step_dev, void* stream);

/* dst_k[c] (+)= sum_r part[r][off_k + c] for up to 4 consecutive column segments (NULL = skip). */
int vg_colsum_f32(const float* part, int rows, int width, float* d0, int n0, float* d1, int n1,
                  float* d2, int n2, float* d3, int n3, int accumulate, void* stream);

/* dst[c] (+)= sum_r X[r][c] for a bf16 matrix (bias gradients: autograd of the "+ bias" in F.linear).
 * part_ws: vg_colsum_bf16_parts(R) * N floats of scratch.  Deterministic two-stage reduction. */
int vg_colsum_bf16_parts(int R);
int vg_colsum_bf16(const void* X, long long ld, int R, int N, float* part_ws, float* dst, int accumulate,
                   void* stream);

/* y = x * mask / keep for dropout site `site` of a network run with (p, seed): exactly the mask the fused
 * passes apply (element index = position in the row-major tensor; n % 4 == 0).  D sites: 0 embedding,
 * 1+2l attention branch, 2+2l MLP branch of block l; G sites: 100+2l, 101+2l.  Used by tests and by the
 * backward where no producer kernel can fuse the mask.
 * The mask, which every masked entry of this header means by "as in vg_dropout_apply":
 *   thr   = the fp32 product 256 p rounded to an integer, halves to even (lrintf), clamped to [0, 255]: p is quantised to 1/256,
 *           thr = 0 is no dropout (y = x bitwise), and a p whose product rounds to 256 drops with thr = 255
 *   scale = the fp32 quotient 256 / (256 - thr), exactly 1 at thr = 0
 *   key   = the host key of (seed, site), mixed with the step counter: k = step_dev ? key ^ (step_dev[0] 0x9E3779B1 + 0x7F4A7C15) : key
 *           (32-bit arithmetic modulo 2^32; key and the counter hash h are written out under vg_diffaug_fwd below).  A NULL step_dev
 *           is not a counter of 0.
 *   element e of the row-major tensor is kept iff byte (e & 3) of the word h(k, e >> 2) is >= thr, byte 0 the lowest
 *   y[e]  = bf16(fp32(x[e]) * (kept ? scale : 0)): one fp32 product, rounded to nearest even
 * Returns -1: null x / y, n < 1 or p outside [0, 1);  -3: n % 4 != 0 - all before any launch. */
int vg_dropout_apply(const void* x, void* y, long long n, float p, unsigned long long seed, int site,
                     const unsigned* step_dev, void* stream);

/* Fused multi-head self-attention (src/v2/modules.py:128-159 after the projections; src/v1/attention.py
 * :43-52,:97-101).  qkv bf16 [B*S, 3*H*HE] (Q | K | V thirds, head-major inside each third);
 * out bf16 [B*S, H*HE]; lse fp32 [B,H,S].  softmax(scale * q.k).  HE in {32,64,96}, S <= 256
 * (S <= 80: csrc/attention.hip; 80 < S <= 256: csrc/attention_long.hip).  The fp8 and L2-distance forms are S <= 80. */
int vg_attention_fwd(const void* qkv, void* out, float* lse, int B, int H, int S, int HE,
                     float scale, void* stream);
int vg_attention_bwd(const void* qkv, const void* out, const void* d_out, const float* lse,
                     void* d_qkv, int B, int H, int S, int HE, float scale, void* stream);
/* The same attention for ONE query per image, row 0 (ABI v7): what the classifier sees of the top encoder block
 * (src/v2/modules.py:195 reads the CLS row only).  out_cls / d_out_cls bf16 [B, H*HE] (the CLS rows, compact), lse_cls fp32
 * [B, H]; d_qkv is the full [B*S, 3*H*HE] gradient (dK, dV of every key, dQ zero off row 0) - exactly what vg_attention_bwd
 * writes when d_out is zero on every other row.  S <= 256. */
int vg_attention_cls_fwd(const void* qkv, void* out_cls, float* lse_cls, int B, int H, int S, int HE, float scale, void* stream);
int vg_attention_cls_bwd(const void* qkv, const void* out_cls, const void* d_out_cls, const float* lse_cls, void* d_qkv, int B, int H,
                         int S, int HE, float scale, void* stream);

/* The same fused attention with the v1 discriminator's L2-distance scores (src/v1/attention.py:43-52,66-67, lp = 2):
 * out = softmax(cdist(q, k) * scale) @ v - the Euclidean distance itself, as the reference has it.  Same layouts. */
/* The same fused attention with fp8 (OCP e4m3) MFMA operands for the activation products: Q.K^T in the forward and in the
 * backward's recompute (so P agrees with the forward's lse) and P.V (numerators scaled by 256 into e4m3's normal range);
 * the products with a gradient operand (dP, dV, dQ, dK) stay bf16.  Same layouts; outputs within ~2^-4 of the fp32 math. */
int vg_attention_fp8_fwd(const void* qkv, void* out, float* lse, int B, int H, int S, int HE,
                         float scale, void* stream);
int vg_attention_fp8_bwd(const void* qkv, const void* out, const void* d_out, const float* lse,
                         void* d_qkv, int B, int H, int S, int HE, float scale, void* stream);

int vg_attention_l2_fwd(const void* qkv, void* out, float* lse, int B, int H, int S, int HE,
                        float scale, void* stream);
int vg_attention_l2_bwd(const void* qkv, const void* out, const void* d_out, const float* lse,
                        void* d_qkv, int B, int H, int S, int HE, float scale, void* stream);

/* v1 overlapping-window tokeniser (src/v1/patch_encoder.py:20-27,54-73): windows of P + 2*overlap pixels at stride
 * (IH - P - 2*overlap)/P + 1, n x n of them; tokens bf16 [B, n*n, C*W*W] is the reference's FLAT view of the
 * (b, c, ty, tx, wy, wx) unfold order (no permute).  img fp32 or bf16 [B,C,IH,IH]; _bwd is the adjoint (d_img bf16). */
int vg_unfold_tokens_fwd(const void* img, int img_is_bf16, void* tokens, int B, int C, int IH, int P,
                         int overlap, void* stream);
int vg_unfold_tokens_bwd(const void* d_tokens, void* d_img, int B, int C, int IH, int P, int overlap,
                         void* stream);

/* ---- second-order operators: the backward OF the backward operators --------------------------------------------------
 * The gradient penalty of the reference's Wasserstein step (src/v2/utils.py:124-144, called at training.py:101-106)
 * differentiates ||d D(x)/d x|| with respect to D's parameters: every backward operator on the input-gradient path needs a
 * backward of its own.  For nn.Linear that is the GEMM family again (backward of dX = dY W:  d(dY) = ddX W^T = vg_linear_fwd,
 * dW = dY^T ddX = vg_linear_wgrad); the three below are the non-linear ones.  u = dL/d(output of the backward operator). */
/* elementwise activation on a stored bf16 pre-activation h (act 1 = GELU(erf), nn.GELU of modules.py:174; 3 = tanh, :191):
 * fwd y = f(h); bwd dh = dy f'(h); bwd_bwd: d_dy = u f'(h), d_h = u dy f''(h).  n % 4 == 0. */
int vg_act_fwd(const void* h, void* y, long long n, int act, void* stream);
int vg_act_bwd(const void* dy, const void* h, void* dh, long long n, int act, void* stream);
int vg_act_bwd_bwd(const void* u, const void* dy, const void* h, void* d_dy, void* d_h, long long n, int act,
                   void* stream);
/* backward of vg_layernorm_bwd (without residual): given u = dL/d(dx), writes d_dy = dL/d(dy) and d_x = dL/d(x) (bf16
 * [R,E]) and per-workgroup partial sums of dL/d(gamma) (part: fp32 [vg_layernorm_bwd_bwd_parts(R)][E], fold with
 * vg_colsum_f32).  E % 64 == 0, E <= 1024. */
int vg_layernorm_bwd_bwd_parts(int R);
int vg_layernorm_bwd_bwd(const void* u, const void* dy, const void* x, const float* mean, const float* rstd,
                         const float* gamma, void* d_dy, void* d_x, float* part, int R, int E, void* stream);
/* backward of vg_attention_bwd: given u_qkv = dL/d(d_qkv) ([B*S, 3E], same layout as qkv), writes d_d_out = dL/d(d_out)
 * [B*S, E] and d_qkv2 = dL/d(qkv) [B*S, 3E].  lse from the forward ([B, H, S]).  Every 1 <= S <= 80 at HE = 32, 64 or 96 (one
 * five-tile MFMA instance, rows padded to 96, a fixed 74 KiB of LDS); -2: S outside that range, -3: another HE. */
int vg_attention_bwd_bwd(const void* qkv, const void* d_out, const float* lse, const void* u_qkv, void* d_d_out,
                         void* d_qkv2, int B, int H, int S, int HE, float scale, void* stream);

/* Start of a training step, two launches instead of torch's seven:
 * vg_zero_tick: g[0, n) = 0 (discriminator.zero_grad(), src/v2/training.py:177) and step_dev[0] += 1 (the device step counter that keys
 *   the dropout masks, AdamW's bias correction and the noise below); n % 4 == 0; step_dev may be NULL.
 * vg_step_inputs: imgs_bf16[0, n_img) = bf16(real) (real NULL: skipped) and z[0, n_z) ~ N(0, 1) (z NULL: skipped) - the latent batch of
 *   construct_noise (training.py:35-42 = torch.randn), counter-based on (seed, step_dev[0], index): Box-Muller of two hashed 24-bit
 *   uniforms, |z| <= 5.77; reproducible per (seed, step), fresh on every replay of a captured graph. */
int vg_zero_tick(float* g, long long n, int* step_dev, void* stream);
int vg_step_inputs(const float* real, void* imgs_bf16, long long n_img, float* z, long long n_z,
                   unsigned long long seed, const int* step_dev, void* stream);

/* A device-resident dataset (the reference feeds CIFAR-10 through a host DataLoader; the rule below has no counterpart there, so this
 * header is its definition): the step draws, decodes and labels its own real batch, keyed on the device step counter.  ONE launch, one
 * workgroup per output image.  images: uint8 on the device, [N, C, IH, IH] (layout 0) or [N, IH, IH, C] (layout 1); labels (nullable):
 * int32 [N]; lut: bf16 [C, 256], the decode table; imgs: bf16 [B, C, IH, IH].  All index arithmetic is uint32 (N < 2^31).
 * Which image.  s = step_dev[0] (the counter as vg_step_inputs reads it, BEFORE vg_zero_tick: 0 on the first step);
 *   nb = N / (B world) whole global batches per epoch (the remainder is dropped, like drop_last);  epoch = s / nb,  j = s % nb;
 *   image n of rank `rank` sits at position p = (j world + rank) B + n of the epoch;  its index is idx = perm_epoch(p) with flags bit 0
 *   (shuffle), else idx = p.
 * perm_epoch: a keyed bijection of [0, N), no table and no state - a 4-round Feistel network on 2k bits with cycle walking.
 *   k = max(1, ceil(bitlength(N - 1) / 2)),  m = 2^k - 1.  One pass on x: L = x >> k, R = x & m; for r = 0..3:
 *   (L, R) <- (R, L ^ (h(key_r, R) & m));  x = (L << k) | R.  Starting from x = p the pass is repeated while x >= N (it ends: it walks
 *   the cycle of a bijection of [0, 2^2k) that contains p < N).  h is the counter hash defined for vg_diffaug_fwd below,
 *   key_r = h(ke, r + 1),  ke = h(h(Kp, 0), epoch),  Kp = the (seed, site 4) key defined there.  N = 1 gives 0.
 * Flip.  With flags bit 1 the image at position p is mirrored left to right iff h(h(h(Kf, 0), epoch), p) >> 31, Kf = the (seed, site 5)
 *   key: keyed on the position of the visit, so ranks and epochs draw independently.
 * Pixels.  imgs[n, c, y, x] = lut[c][images[idx, ...]], the source read at (c, y, x') or (y, x', c) by layout, x' = IH - 1 - x when
 *   flipped.  With lut[c][v] = bf16(((float(v) / 255) - mean[c]) / std[c]) in fp32 this is ToTensor + Normalize + the bf16 cast of
 *   vg_step_inputs, bit for bit.  labels_out[n] = labels[idx] and index_out[n] = idx are written when the pointers are given.
 * The source image and the table are staged in LDS with 16-byte loads; every thread emits runs of 8 pixels as one 16-byte store.
 * Returns, all before any launch:  -1: null images / lut / imgs / step_dev, labels_out without labels, or N, C, IH or B < 1;  -2: world < 1, rank outside
 * [0, world), layout not 0 / 1, flags outside [0, 3], N < B world or N >= 2^31;  -3: IH IH % 8 != 0, C IH IH % 16 != 0, C > 4, one image
 * plus the table above 160 KiB of LDS, or images / lut / imgs not 16-byte aligned. */
int vg_dataset_fetch(const unsigned char* images, const int* labels /*nullable*/, long long N, int C, int IH, int layout,
                     const void* lut /*bf16 [C, 256]*/, void* imgs /*bf16 [B, C, IH, IH]*/, int* labels_out /*nullable*/,
                     int* index_out /*nullable*/, int B, int rank, int world, int flags, unsigned long long seed,
                     const int* step_dev, void* stream);

/* Differentiable augmentation of the discriminator's input (DiffAugment: color, translation, cutout; the reference has none, so this
 * header is its definition) and its adjoint.  x, y, dy, dx bf16 [B, C, IH, IH] (x and y, dy and dx must not overlap); fp32 arithmetic.
 * Per image n:  T = cutout o translation o contrast o saturation o brightness,  members switched by `policy` (bit 0 the three color
 * members together, bit 1 translation, bit 2 cutout; 0 = a plain copy) with parameters (b, s, k, tx, ty, cx, cy):
 *   brightness   x + b                                                          b = u0 - 0.5
 *   saturation   m + s (x - m),  m = mean over the C channels of the pixel      s = 2 u1
 *   contrast     M + k (x - M),  M = mean over the C*IH*IH elements of the image k = u2 + 0.5
 *   translation  y[i, j] = x[i - ty, j - tx], zero outside                      tx = I3(2r + 1) - r, ty = I4(2r + 1) - r, r = IH / 8
 *   cutout       zero for rows [cy - IH/4, cy - IH/4 + IH/2) x columns [cx - IH/4, cx - IH/4 + IH/2), clipped;  cx = I5(IH + 1), cy = I6(IH + 1)
 * (integer divisions round down).  The parameters are a pure function of (seed, site, step_dev[0], n, p), in 32-bit arithmetic modulo 2^32
 * behind the host key:
 *   key  = fold(splitmix64(seed + 0x9E3779B97F4A7C15 (site + 1)))   the key of vg_dropout_apply's (seed, site): z = that sum mod 2^64;
 *          z = (z ^ z >> 30) 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) 0x94D049BB133111EB;  z ^= z >> 31;  key = low 32 bits of (z ^ z >> 32)
 *   h(k, i) = the counter hash of the dropout masks: x = i 0x9E3779B1 + k;  x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;
 *          x *= 0x846CA68B;  x ^= x >> 16
 *   ks   = h(step_dev ? key ^ (step_dev[0] 0x9E3779B1 + 0x7F4A7C15) : key, 0);   kn = h(ks, n);   k_p = h(kn, p) >> 8   (24 bits)
 *   u_p  = k_p 2^-24 (exact in fp32, and so are b and s; k = u2 + 0.5 is that ONE fp32 addition, round to nearest even);   I_p(m) = (k_p m) >> 24
 * A member that is off takes its identity: b = 0, s = k = 1, tx = ty = 0, cx = cy = -IH (a square that misses the image).
 * params_out (nullable): fp32 [B, 8] = (b, s, k, tx, ty, cx, cy, policy) as the kernel used them.
 * T is affine in x, so the adjoint takes dy and the same (policy, seed, site, step) only: with g[i, j] = dy[i + ty, j + tx] where that
 * pixel is inside the frame and outside the cutout, else 0:  dx = k (s g + (1 - s) mean_channels(g)) + (1 - k) mean_image(g);
 * accumulate = 1 adds into dx.  One launch each, one workgroup per image, fixed-order sums (bitwise reproducible), no scratch.
 * Returns -1: null x / y or B < 1;  -2: policy outside [0, 7], C < 1, IH < 8 or IH > 255;  -3: C*IH*IH % 8 != 0 - all before any launch. */
int vg_diffaug_fwd(const void* x, void* y, float* params_out, int B, int C, int IH, int policy, unsigned long long seed,
                   int site, const unsigned* step_dev, void* stream);
int vg_diffaug_bwd(const void* dy, void* dx, int accumulate, int B, int C, int IH, int policy, unsigned long long seed,
                   int site, const unsigned* step_dev, void* stream);

/* The gated forms of the two calls above (adaptive discriminator augmentation; the reference has none, so this header is its
 * definition): every member of `policy` is applied to an image with probability p = prob_dev[0], a DEVICE pointer the kernel reads
 * itself - a replayed hipGraph sees the value of the moment, no host round trip and no recapture.  Per image n and member m (0 color,
 * 1 translation, 2 cutout), with kn and h of the definition above:
 *   member m is on  iff  bit m of `policy` is set  and  k_{8+m} < T,     k_{8+m} = h(kn, 8 + m) >> 8   (the parameters use draw indices 0..6)
 *   T = (uint32) floorf(clamp(p, 0, 1) 2^24);  a NaN clamps to 0.  An integer compare: p = 1 (T = 2^24) switches every member of the
 *   policy on, p = 0 every member off, and the set at p contains the set at any smaller p.
 * The members that are on form the image's EFFECTIVE policy, and the image is then processed exactly as vg_diffaug_fwd / _bwd process
 * an image under that policy: the parameter draws do not depend on the policy, the arithmetic is the same code - bit for bit the same
 * output.  An image with every gate off is a bitwise copy (adjoint: copy / add).  params_out[n, 7] holds the effective policy and
 * columns 0..6 the identities of what is off.  The adjoint takes the same (policy, seed, site, step, p) and uses the same gates.
 * Returns what vg_diffaug_fwd / _bwd return, and -1 for a null prob_dev - all before any launch. */
int vg_diffaug_p_fwd(const void* x, void* y, float* params_out, int B, int C, int IH, int policy, unsigned long long seed,
                     int site, const unsigned* step_dev, const float* prob_dev, void* stream);
int vg_diffaug_p_bwd(const void* dy, void* dx, int accumulate, int B, int C, int IH, int policy, unsigned long long seed,
                     int site, const unsigned* step_dev, const float* prob_dev, void* stream);

/* GAN losses on logits (src/v1/gan.py:16-20,227,238,250 for kind 0; hinge for kind 1;
 * kind 2 = the Wasserstein critic losses of src/v2/training.py:72,97).
 * role 0 D-real, 1 D-fake, 2 G.  loss_out[0] = mean loss, dlogits = d loss / d logits * grad_scale. */
int vg_gan_loss(const float* logits, float* dlogits, float* loss_out, int n, int kind, int role,
                float grad_scale, void* stream);
/* the same on two consecutive segments of one logit vector in ONE launch (the fused real + fake discriminator pass):
 * logits[0, n0) with role0 -> loss_out[0], logits[n0, n0 + n1) with role1 -> loss_out[1]; each mean is over its own segment. */
int vg_gan_loss_pair(const float* logits, float* dlogits, float* loss_out, int n0, int role0, int n1, int role1,
                     int kind, float grad_scale, void* stream);

/* Class conditioning (the reference's live loop hands [B, 10] logits and labels to a loss that cannot take them, so this header is the
 * definition).  Labels are int32, one per sample; EVERY kernel clamps a label into [0, K) before it indexes anything, so a bad label
 * selects class 0 or K - 1 and never leaves a buffer.  1 <= K <= 16 throughout (the head kernels' width).
 *
 * vg_draw_labels: labels[i] = (k_i K) >> 24,  k_i = h(ks, i) >> 8,  with ks and h exactly the launch key and the counter hash defined for
 *   vg_diffaug_fwd above (key from (seed, site), mixed with step_dev[0] when step_dev != NULL).  k_i is 24 bits and K <= 16, so the product
 *   stays inside 32 bits.  Reproducible per (seed, site, step), fresh on every replay of a captured graph.  The fused step draws its fake
 *   labels with the seed of its augmentation draws and site 3 (DiffAugment uses sites 0 and 1, bCR's transform site 2).
 *   -1: null labels or n < 1;  -2: K outside [1, 16].
 * vg_class_add: wmod[n, j] = bf16_rne(float(wmod[n, j]) + float(table[y_n, j])) in place (one fp32 addition, one rounding), wmod bf16 [B, N],
 *   table bf16 [K, N], y_n = clamp(labels[n]).  16-byte accesses.  -1: a null pointer, B < 1 or N < 1;  -2: K outside [1, 16];
 *   -3: N % 8 != 0 or wmod / table not 16-byte aligned.
 * vg_class_grad: s[k, j] = the fp32 sum of dw[n, j] over the n with clamp(labels[n]) == k, formed by ONE accumulator per output element that
 *   starts at +0 and adds the rows in ascending n (rows of other classes take no part).  accumulate == 0: dtable[k, j] = s[k, j] - a class
 *   with no sample writes +0;  accumulate == 1: dtable[k, j] = dtable[k, j] + s[k, j] (one addition) - a class with no sample leaves its row
 *   untouched.  dw fp32 [B, N], dtable fp32 [K, N].  No atomics: bitwise defined.  -1: a null pointer, B < 1 or N < 1;  -2: K outside
 *   [1, 16] or accumulate not 0 / 1;  -3: N % 4 != 0 or dw / dtable not 16-byte aligned.
 * vg_gan_loss_cond: the label-selected loss of a K-way head, D(x, y) = D(x)[y] (Mescheder et al. 2018).  logits, dlogits fp32 [n, Kc]; with
 *   s_i = logits[i, clamp(labels[i])]:  loss_out[0] and d_i are what vg_gan_loss computes on the n values s_i - the same code, the same
 *   order, the mean over n (not n Kc) - and dlogits[i, k] = (k == y_i) ? d_i : +0, every element written; selected (nullable, fp32 [n])
 *   receives s_i.  vg_gan_loss_cond_pair: rows [0, n0) with role0 -> loss_out[0], rows [n0, n0 + n1) with role1 -> loss_out[1], ONE launch of
 *   two workgroups like vg_gan_loss_pair; bit-equal to two single calls.  -1: a null logits / labels / dlogits / loss_out or a size < 1;
 *   -2: kind or a role outside [0, 2], Kc outside [1, 16], or (n0 + n1) Kc >= 2^31.
 * All argument errors come back before any launch. */
int vg_draw_labels(int* labels, int n, int K, unsigned long long seed, int site, const unsigned* step_dev, void* stream);
int vg_class_add(void* wmod_bf16 /*[B, N]*/, const void* table_bf16 /*[K, N]*/, const int* labels, int B, int N, int K, void* stream);
int vg_class_grad(const float* dw /*[B, N]*/, const int* labels, float* dtable /*[K, N]*/, int B, int N, int K, int accumulate,
                  void* stream);
int vg_gan_loss_cond(const float* logits /*[n, Kc]*/, const int* labels, float* dlogits /*[n, Kc]*/, float* selected /*[n], nullable*/,
                     float* loss_out, int n, int Kc, int kind, int role, float grad_scale, void* stream);
int vg_gan_loss_cond_pair(const float* logits, const int* labels, float* dlogits, float* selected, float* loss_out /*[2]*/, int n0,
                          int role0, int n1, int role1, int Kc, int kind, float grad_scale, void* stream);

/* Balanced consistency regularisation (bCR, Zhao et al. 2020; the reference has none, so this header is its definition) between the
 * discriminator's logits on a batch x and on its augmented partner a = T(x).  logits_x, logits_a, dlog_x, dlog_a: fp32 [B_real + B_fake, Kc],
 * the B_real real images first; the four must not overlap.  Per segment s (real: images [0, B_real), weight w_real; fake: the B_fake images
 * behind them, weight w_fake), with d = logits_x - logits_a elementwise (the difference first, then the square):
 *   loss_out[s] = 1/B_s sum_{n in s} sum_k d[n, k]^2                     the UNWEIGHTED mean over the B_s images (not over B_s Kc)
 *   dlog_x[n, k] (+)= g,   dlog_a[n, k] (-)= g,   g = ((2 w_s) / B_s) grad_scale d[n, k]      both branches carry gradient
 * accumulate_x / accumulate_a = 1 adds into what the adversarial loss kernel wrote, 0 overwrites and writes every element.  A zero
 * weight writes +0 (overwrite) or leaves the target untouched (accumulate); the loss is reported all the same.
 * ONE launch of two workgroups (one per segment), fp32, fixed order - per thread a strided chain, the wave butterfly, the four waves
 * in order, one product with the rounded 1 / B_s - no atomics: bitwise reproducible.
 * Returns -1: a null pointer or a non-positive size;  -2: a negative or NaN weight, an accumulate flag other than 0 / 1, or
 * (B_real + B_fake) Kc >= 2^31 - all before any launch. */
int vg_bcr_loss(const float* logits_x, const float* logits_a, float* dlog_x, float* dlog_a, float* loss_out /*[2]*/,
                int B_real, int B_fake, int Kc, float w_real, float w_fake,
                int accumulate_x, int accumulate_a, float grad_scale, void* stream);

/* The controller of the augmentation probability (ADA, Karras et al. 2020; the reference has none, so this header is its definition),
 * driven by the discriminator's overfitting signal r_t = E[sign(D(real))].  logits_real: fp32 [n], the real rows of the adversarial logits
 * of one step; state: fp32 [4] on the device, 16-byte aligned, = (p, acc_sign, acc_count, r_last); step_dev: the device step counter.
 * Every call, in fp32:
 *   acc_sign += sum_i sgn(logits_real[i]),  sgn(+-0) = sgn(NaN) = 0  (integer-valued, exact for n < 2^24: the order cannot matter)
 *   acc_count += n
 * and when step_dev[0] % interval == 0:
 *   s = sgn(acc_sign - target * acc_count)                     one multiply, one subtract (not fused)
 *   p = min(max(p + s * (step_per_image * acc_count), 0), 1)   (s is -1, 0 or 1, so the product with it is exact)
 *   r_last = acc_sign / acc_count;   acc_sign = acc_count = 0
 * ONE launch of one workgroup, no atomics, the state written as one 16-byte vector store; p is state[0], so &state[0] is the prob_dev
 * of vg_diffaug_p_fwd / _bwd and launches behind this one see the new value.
 * Returns -1: a null pointer or n < 1;  -2: interval < 1, target outside (-1, 1) or NaN, step_per_image not positive and finite, or
 * n >= 2^24;  -3: state not 16-byte aligned - all before any launch. */
int vg_ada_update(const float* logits_real, int n, float* state /*[4]*/, float target, float step_per_image, int interval,
                  const int* step_dev, void* stream);

/* torch.optim.AdamW step over a flat fp32 buffer (src/v2/training.py:150-157), also refreshing the
 * bf16 shadow the GEMMs read.  n % 4 == 0.  grads are multiplied by gscale first.  The step number
 * (1-based) comes from step_dev[0] (device int) when step_dev != NULL - for hipGraph replay - else
 * from `step`. */
int vg_adamw_step(float* p, const float* g, float* m, float* v, void* shadow_bf16, long long n,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                  const int* step_dev, float gscale, void* stream);
/* vg_adamw_step plus an exponential moving average of the updated weights in the same pass (38 B per parameter against 30; the
 * generator's sample / FID weights).  p, m, v and shadow_bf16 come out bit for bit as vg_adamw_step writes them.  With
 * t = step_dev ? step_dev[0] : step (read, never written) and p1 the updated weight:
 *   t <= max(1, ema_start):  ema = p1                    (the average follows the weights through the warm-up; the first step always
 *                                                         copies, whatever ema held - a zeroed step counter restarts the average)
 *   else:                    ema = fmaf(1 - d, p1 - ema, ema),  d = ema_decay.
 * ema (fp32, n elements) must not overlap another buffer.  -1: a null pointer, -3: n % 4 != 0, -2: ema_decay outside [0, 1) or
 * ema_start < 0 - all before any launch. */
int vg_adamw_ema_step(float* p, const float* g, float* m, float* v, void* shadow_bf16, float* ema, long long n,
                      float lr, float beta1, float beta2, float eps, float weight_decay, int step, const int* step_dev,
                      float gscale, float ema_decay, int ema_start, void* stream);
/* The same rule applied to given (already updated) weights p: bit-equal to vg_adamw_ema_step's ema.  For ranges whose AdamW ran
 * elsewhere (the sharded update of the generator's mapping Linear). */
int vg_ema_update(float* ema, const float* p, long long n, float ema_decay, int ema_start, int step, const int* step_dev,
                  void* stream);
/* The learning rates on the device (additive to ABI 9).  The reference meant to schedule its rates (src/v2/training.py:15 imports
 * ReduceLROnPlateau, :215-216 hold the commented scheduler steps) and never did, so this header is the definition.
 *
 * vg_lr_schedule: ONE launch of one workgroup, thread 0 = slot 0 (the discriminator, schedule *d), thread 1 = slot 1 (the generator, *g).
 * With t = max(step_dev[0], 1) - the device step counter as vg_zero_tick left it, 1 on the first step; a counter below 1 counts as 1 -
 * and per slot (base, kind, warmup, total, final_ratio), the factor is f = f_w f_d:
 *   f_w = t / warmup                      for 1 <= t <= warmup (so exactly 1 at t = warmup), and exactly 1 otherwise (warmup == 0 too)
 *   f_d = 1                               exactly, while t <= warmup and for kind == VG_LR_CONSTANT (total is then not read)
 *   f_d = final_ratio                     exactly, once t >= total
 *   else, s = (t - warmup) / (total - warmup):
 *     VG_LR_LINEAR   f_d = 1 - (1 - final_ratio) s
 *     VG_LR_COSINE   f_d = final_ratio + (1 - final_ratio) 0.5 (1 + cos(pi s))
 *   lr_out[slot] = (float)((double)base * f * (double)scale_dev[slot])
 * every exact case an explicit branch, everything in fp64 (not contracted) with ONE rounding to fp32 at the end: an fp64 evaluation
 * elsewhere agrees to one fp32 ulp, and where f and the scale are exactly 1 the result is base bit for bit.  A slot reads its own
 * scale only.  scale_dev, lr_out: two floats each on the device.  Plain stores, no atomics, no LDS.  The schedules are passed by
 * value: the pointers are host pointers, read before the call returns.
 * Returns -1: a null pointer (step_dev is required);  -2: kind out of range, warmup < 0, total <= warmup for a decaying kind,
 * final_ratio outside [0, 1] or NaN, base not finite and positive - all before any launch.
 *
 * vg_adamw_step_dlr / vg_adamw_ema_step_dlr: vg_adamw_step / vg_adamw_ema_step with the rate read on the device, lr = lr_dev[0] (one
 * uniform load per thread; a launch behind vg_lr_schedule on the same stream sees the rate it wrote), in the place of the float: a
 * captured hipGraph then replays with a fresh rate.  The update expressions are the same code: given lr_dev[0] equal to the float, p, m,
 * v, shadow_bf16 and ema come out bit for bit as the float forms write them.  Errors as there, lr_dev == NULL is -1. */
#define VG_LR_CONSTANT 0
#define VG_LR_LINEAR 1
#define VG_LR_COSINE 2
typedef struct VgLrSched {
  float base;        /* the rate the factor multiplies: finite, > 0 */
  int kind;          /* VG_LR_* */
  int warmup;        /* steps of linear warm-up, >= 0 */
  int total;         /* step from which the factor is final_ratio; > warmup for a decaying kind */
  float final_ratio; /* in [0, 1] */
} VgLrSched;
int vg_lr_schedule(const VgLrSched* d, const VgLrSched* g, const int* step_dev, const float* scale_dev /*[2]*/, float* lr_out /*[2]*/,
                   void* stream);
int vg_adamw_step_dlr(float* p, const float* g, float* m, float* v, void* shadow_bf16, long long n,
                      const float* lr_dev, float beta1, float beta2, float eps, float weight_decay, int step,
                      const int* step_dev, float gscale, void* stream);
int vg_adamw_ema_step_dlr(float* p, const float* g, float* m, float* v, void* shadow_bf16, float* ema, long long n,
                          const float* lr_dev, float beta1, float beta2, float eps, float weight_decay, int step, const int* step_dev,
                          float gscale, float ema_decay, int ema_start, void* stream);
/* diversity_loss of the reference's unreached generator step (src/v2/utils.py:147-152; training.py:73-74 adds 0.1 x it
 * to the generator loss): loss_out[0] = sum_{i,j} |x_i - x_j|_1 / (B (B-1)) over images bf16 [B, D]; when d_images is
 * not NULL, d_images (bf16 [B, D]) += weight * d loss / d images.  scratch: ceil(D/16) floats.  B <= 1024. */
int vg_diversity_loss(const void* images, void* d_images, float* loss_out, float* scratch, int B, int D,
                      float weight, void* stream);

/* torch.nn.utils.clip_grad_norm_ (the reference's Wasserstein step, src/v2/training.py:78,104) on a flat fp32 gradient
 * buffer: g *= min(1, max_norm / (gscale*|g|_2 + 1e-6)) in place; scratch: 1 + 1024 floats of device memory,
 * scratch[0] receives gscale*|g|_2.  Deterministic (no atomics).  n % 4 == 0. */
int vg_grad_clip(float* g, long long n, float gscale, float max_norm, float* scratch, void* stream);
int vg_cast_f32_bf16(const float* src, void* dst_bf16, long long n, void* stream);

/* The kernels at the two ends of the networks, one by one (additive to ABI 9; csrc/elementwise.hip, tests/test_ends_gpu.py): the
 * launches that vg_vit_forward / vg_vit_backward* / vg_gen_* make around the encoder blocks, exposed so that each is held to its own
 * contract.  Every entry refuses a NULL pointer (-1) and a shape its kernel cannot take (-3) on the host, before any launch; the
 * entries that carry a dropout mask take (p, seed, site, step_dev) as vg_dropout_apply does and refuse p outside [0, 1) (-1).
 *
 * vg_head_fwd:  logits[b, k] = sum_e t[b, e] W2[k, e] + b2[k]   (t bf16 [B, E], the tanh output of the classifier's fc1; W2 fp32 [Kc, E];
 *   fp32 accumulation).  B, E, Kc >= 1.
 * vg_head_bwd:  dz[b, e] = bf16((sum_k dlogits[b, k] W2[k, e]) (1 - t[b, e]^2)), the gradient at fc1's pre-activation, and with
 *   want_wgrad the gradients of fc2.  Returns 1, 0 or a negative code (a hipError_t comes back negated):
 *     1  (want_wgrad, Kc <= 16 and part != NULL): ONE launch; part, fp32
 *        [vg_head_bwd_parts(B)][vg_head_bwd_part_width(E, Kc)], receives per 32 rows b one partial row
 *        dW2 (Kc E: sum_b dlogits[b, k] t[b, e]) | db1 (E: sum_b of the ROUNDED dz) | db2 (Kc: sum_b dlogits[b, k]),
 *        to be folded with vg_colsum_f32; dW2 and db2 are not touched (they may be NULL).
 *     0  (Kc > 16, or part == NULL): the separate kernels; with want_wgrad dW2 [Kc, E] and db2 [Kc] are ACCUMULATED into (+=), and db1
 *        is the caller's column sum of dz (vg_colsum_bf16).  want_wgrad = 0 (any Kc, returns 0): dz only, the same bits.
 * vg_batch_sum:  out[s, e] = sum_b g[b S + s, e]   (g bf16 [B S, E], out fp32 [S, E], fixed order).  E % 64 == 0.
 * vg_embed_small_grads:  d_cls[e] += tok_sum[0, e];  d_pos[s - 1, e] += tok_sum[s, e] and d_bias[e] += sum_{s >= 1} tok_sum[s, e] for
 *   s = 1 .. S - 1   (tok_sum fp32 [S, E], the output of vg_batch_sum; d_pos is [(S - 1), E]).  S >= 2.
 * vg_take_rows:  out[b n_take + j, :] = in[b S + first + j, :]   (bf16).  E % 8 == 0, 0 <= first, first + n_take <= S.
 * vg_scatter_cls:  g[b S, :] = src[b, :], every other row of g [B S, E] = 0; with gm != NULL and p > 0 also gm = what vg_dropout_apply
 *   with the same (p, seed, site, step_dev) makes of the whole of g (p = 0: gm is not written).  vg_scatter_cls_pair: two sources
 *   into two tensors, no mask.  E % 8 == 0.
 * vg_fill_cls:  x[b S, e] = bf16(cls[e] mask / keep), the mask of element (b S) E + e of the [B S, E] tensor; no other row is written.
 * vg_patchify:  A[(b G + gy) G + gx, (c P + py) P + px] = bf16(img[b, c, gy P + py, gx P + px]), G = IH / P  (img fp32, or bf16 with
 *   img_is_bf16).  vg_unpatchify: its inverse on bf16.  IH % P == 0.
 * vg_slab_reduce:  dst[i] (+)= sum_s slab[s stride + i] for i < n, the slices added in slice order.  n % 4 == 0, nslab >= 1, and with more
 *   than one slice stride >= n, stride % 4 == 0.  vg_slab_reduce_pair: two folds of one shape in one launch.
 * vg_sin_grad:  dz[i] = bf16(dy[i] w0 cos(w0 z[i]))   (dy bf16, z fp32; the hardware cosine).  n % 4 == 0.
 * vg_add_table:  x[r, :] = bf16(x[r, :] + table[r % period, :]) in place (x bf16 [rows, E], table fp32 [period, E]).  E % 4 == 0. */
int vg_head_fwd(const void* t, const float* W2, const float* b2, float* logits, int B, int E, int Kc, void* stream);
int vg_head_bwd_parts(int B);               /* host only */
int vg_head_bwd_part_width(int E, int Kc);  /* host only */
int vg_head_bwd(const float* dlogits, const float* W2, const void* t, void* dz, float* dW2, float* db2, float* part, int B, int E, int Kc,
                int want_wgrad, void* stream);
int vg_batch_sum(const void* g, float* out, int B, int S, int E, void* stream);
int vg_embed_small_grads(const float* tok_sum, float* d_cls, float* d_pos, float* d_bias, int S, int E, void* stream);
int vg_take_rows(const void* in, void* out, int B, int S, int first, int n_take, int E, void* stream);
int vg_scatter_cls(const void* src, void* g, void* gm, int B, int S, int E, float p, unsigned long long seed, int site,
                   const unsigned* step_dev, void* stream);
int vg_scatter_cls_pair(const void* src_a, void* dst_a, const void* src_b, void* dst_b, int B, int S, int E, void* stream);
int vg_fill_cls(void* x, const float* cls, int B, int S, int E, float p, unsigned long long seed, int site, const unsigned* step_dev,
                void* stream);
int vg_patchify(const void* img, int img_is_bf16, void* A, int B, int C, int IH, int P, void* stream);
int vg_unpatchify(const void* dA, void* d_img, int B, int C, int IH, int P, void* stream);
int vg_slab_reduce(const float* slab, long long stride, int nslab, float* dst, long long n, int accumulate, void* stream);
int vg_slab_reduce_pair(const float* slab0, const float* slab1, long long stride, int nslab, float* dst0, float* dst1, long long n,
                        int accumulate, void* stream);
int vg_sin_grad(const void* dy, const float* z, void* dz, long long n, float w0, void* stream);
int vg_add_table(void* x, const float* table, long long rows, int E, int period, void* stream);

/* Spectral normalisation of a set of weight matrices that live inside one flat parameter buffer (ViTGAN's form,
 * W_eff = sigma_max(W_init) W / sigma_max(W); one power iteration per step as torch.nn.utils.spectral_norm runs in training).
 * The GEMMs read the bf16 shadow only, so normalising is a scaled cast of the fp32 master into the shadow plus one linear
 * correction of the gradient buffer before the optimizer.
 *
 * A table entry names one matrix W [N, K], row-major at element offset w_off of the flat buffers.  The caller fills w_off, N, K;
 * vg_spectral_plan (host only) fills every other field and returns the sizes, in floats, of
 *   state:   per matrix u [N] at u_off, v [K] at v_off, sigma at s_off, sigma0 at s_off + 1 (offsets are multiples of 4)
 *   scratch: per matrix t [K], w [N] and one partial sum per VG_SPEC_CHUNK elements; needs no initialisation.
 * The caller keeps the table twice, on the host (validated by every call) and as the same bytes on the device (read by the kernels).
 *
 * vg_spectral_update, iterate = 1, on the master W (3 launches for the whole table):
 *   t = W^T u ; v = t / max(|t|, 1e-12) ; w = W v ; sigma = |w| ; u = w / max(sigma, 1e-12)
 *   shadow[w_off + i] = bf16_rne(fp32(sigma0 / max(sigma, 1e-12)) * W[i])       for the table's ranges only
 * iterate = 0 (1 launch): the same cast from the stored sigma; u, v, sigma unchanged (after a plain cast of the whole buffer).
 * vg_spectral_project (2 launches), G = dL/dW_eff in the gradient buffer, with the stored (u, v, sigma), s = sigma0 / sigma:
 *   G[w_off + nK + k] <- s * fma(-(<G, W> / sigma) * u[n], v[k], G[..])         (u and v constants, as in torch)
 * fp32 throughout, fixed summation order, no atomics: two runs are bit-equal.  Elements outside the table's ranges are not written.
 * Errors, before any launch: -1 a null pointer or n < 1; -2 N < 1, K < 1, a range outside [0, total), a buffer smaller than the
 * plan's, or a table whose planned fields are not vg_spectral_plan's; -3 overlapping ranges, W / G / state / scratch not 16-byte or
 * shadow not 8-byte aligned; -4 iterate not 0 or 1. */
#define VG_SPEC_COLS 64     /* columns per workgroup of the W^T u pass */
#define VG_SPEC_ROWS 16     /* rows per workgroup of the W v pass */
#define VG_SPEC_CHUNK 8192  /* elements per workgroup of the cast / dot / projection passes */
typedef struct VgSpectralDesc {
  long long w_off;
  int N, K;
  long long u_off, v_off, s_off;        /* state */
  long long t_off, w_tmp_off, dot_off;  /* scratch */
  int blk_a, blk_b, blk_c, reserved;    /* first workgroup of this matrix in the three grids */
} VgSpectralDesc;
int vg_spectral_plan(VgSpectralDesc* table_host, int n, long long* state_floats, long long* scratch_floats); /* host only */
int vg_spectral_update(const float* W, void* shadow_bf16, long long total, float* state, long long state_floats, float* scratch,
                       long long scratch_floats, const VgSpectralDesc* table_host, const VgSpectralDesc* table_dev, int n, int iterate,
                       void* stream);
int vg_spectral_project(float* G, const float* W, long long total, const float* state, long long state_floats, float* scratch,
                        long long scratch_floats, const VgSpectralDesc* table_host, const VgSpectralDesc* table_dev, int n, void* stream);

/* ABI v9 (additive).  Streaming moments of feature vectors, the accumulator of the Frechet distance (metrics.hip); fp64 throughout.
 *
 * vg_moments_update: feats fp32 [n, d] with row stride ld (floats);  sum[j] += sum_i x_ij;  gram[j][k] += sum_i x_ij x_ik.
 * Every x is widened to fp64 exactly, every product and addition is fp64 on v_mfma_f64_16x16x4_f64: per output element one chain
 *   acc = gram[j][k];  for i = 0 .. n-1 in groups of 4 rows:  acc = mfma(x_i.j, x_i.k, acc)
 * so integer-valued features below 2^53 in sum come out exact, and otherwise the error is an fp64 dot product's.  One wave owns each
 * 16 x 16 tile of the upper triangle and walks the rows in order; there are no atomics: two runs are bit-equal, two updates equal one
 * update of the concatenation whenever the first n is a multiple of 4 (and always for exactly representable sums).  gram comes out
 * symmetric bit for bit (off-diagonal tiles are stored twice); the caller starts sum and gram from zeros and only passes them back in.
 * Rows past n in the last group of 4 count as exact zeros.  d % 16 == 0, 16 <= d <= 2048, n >= 1, ld >= d.
 * vg_moments_finish: mean = sum / n;  cov = (gram - n mean (x) mean) / (n - 1), the one-pass formula (torchmetrics' own), each
 * operation rounded once; n >= 2.  Elementwise - here so that a caller of this ABI has the whole accumulator.
 * Errors, before any launch: -1 a NULL pointer, n < 1 (finish: n < 2); -2 d or ld outside the above. */
int vg_moments_update(const float* feats, long long ld, int n, int d, double* sum /*[d]*/, double* gram /*[d, d]*/, void* stream);
int vg_moments_finish(const double* sum, const double* gram, long long n, int d, double* mean /*[d]*/, double* cov /*[d, d]*/, void* stream);

/* ABI v9 (additive).  Arithmetic on PAIRS of feature vectors (pairwise.hip): what precision / recall / density / coverage and KID
 * need beyond the moments.  Features fp32 [n, d] with a row stride in floats, widened exactly; every product and sum fp64 on
 * v_mfma_f64_16x16x4_f64.  Squared Euclidean distances d2(q_i, c_j) = max((|q_i|^2 + |c_j|^2) - 2 q_i.c_j, 0), where the norms are
 * the diagonal of the SAME product chain as the dots: bit-equal rows are at distance exactly 0.0.  Comparisons are inclusive.
 * No n x n buffer exists: tiles live in registers, `ws` (vg_pair_ws_bytes(nq, nc, k) bytes, k = 0 where there is none) holds the norms
 * and the per-column-split partials.  The split count depends on (nq, nc) only and partials are merged in split order, without
 * atomics: two runs are bit-equal; rad2, count and min_d2 are also bit-identical under any permutation of the centre rows.
 *
 * vg_knn_radii:  rad2[i] = the k-th smallest of { d2(x_i, x_j) : j != i }, the self-exclusion BY INDEX (a duplicate row at another
 *   index is a neighbour at 0.0).
 * vg_ball_counts:  count[i] = #{ j : d2(q_i, c_j) <= rad2_c[j] },  min_d2[i] = min_j d2(q_i, c_j).
 * vg_poly_kernel_sum:  out[0] = sum_ij (q_i.c_j / d + 1)^3, with skip_diagonal != 0 without the terms i == j; per-workgroup partials
 *   folded by one owner in index order.
 * All enqueue-only on `stream`.  Errors, before any launch: -1 a NULL pointer or an empty set; -2 d outside [16, 2048], d % 16 != 0
 * or a row stride below d; -3 k outside [1, 8] or k >= n.  vg_pair_ws_bytes: -1 for an empty set or k outside [0, 8]. */
long long vg_pair_ws_bytes(int nq, int nc, int k);
int vg_knn_radii(const float* X, long long ld, int n, int d, int k, double* rad2 /*[n]*/, void* ws, void* stream);
int vg_ball_counts(const float* Q, long long ldq, int nq, const float* Cn, long long ldc, int nc, int d, const double* rad2_c /*[nc]*/,
                   int* count /*[nq]*/, double* min_d2 /*[nq]*/, void* ws, void* stream);
int vg_poly_kernel_sum(const float* Q, long long ldq, int nq, const float* Cn, long long ldc, int nc, int d, int skip_diagonal,
                       double* out /*[1]*/, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * Whole-network passes (what the nn.Modules call: one C call per forward / backward)
 * ---------------------------------------------------------------------------------------- */

/* Execution context (second HIP stream + events) for concurrent weight-gradient work; host only.  One per
 * engine / process; the calls using it must come from one host thread. */
int vg_ctx_create(void** out_ctx);
int vg_ctx_destroy(void* ctx);

/* v2 VisionTransformer (src/v2/modules.py:202-238) = ViTDiscriminator.forward (:393-395). */
typedef struct VgVitDims {
  int C, IH, P, E, H, L, R, Kc; /* channels, image size, patch, embed, heads, layers, mlp ratio, classes */
} VgVitDims;
/* Flat parameter layout (element offsets, identical for fp32 master, bf16 shadow, fp32 grads). */
typedef struct VgVitLayout {
  long long conv_w, conv_b, pos, cls;           /* embedding.conv1.weight [E,C*P*P], .bias, pos_embedding, cls_token */
  long long layer0, layer_stride;               /* first encoder block, distance between blocks */
  long long wqkv, wo, w1, w2;                   /* per block, relative: queries|keys|values [3E,E], out_projection, fc1, fc2 */
  long long ln1_w, ln1_b, bqkv, bo, ln2_w, ln2_b, b1, b2;
  long long layer_weights;                      /* elements in [wqkv, w2 end) */
  long long lnf_w, lnf_b, hw1, hb1, hw2, hb2;   /* vit.norm, classifier.fc1, classifier.fc2 */
  long long total;
} VgVitLayout;
int vg_vit_layout(const VgVitDims* d, VgVitLayout* out); /* host only */
long long vg_vit_ws_bytes(const VgVitDims* d, int B);   /* host only: activation + scratch workspace */

/* Byte offsets inside the workspace of what a forward saves and a backward leaves behind (host only; used by the parity
 * tests to teacher-force single encoder blocks with the tensors the kernels produced).  M = B*(NP+1) rows.  Per block l:
 * X[l] at X + l*M*E*2 (X[L] = trunk output), xn1 / ao / xmid / xn2 likewise, qkv at qkv + l*M*3E*2, z1 (gelu') and a1
 * (gelu) at + l*M*R*E*2, lse at lse + l*B*H*S*4, mean / rstd at + l*M*4.  Backward scratch, one set per block parity:
 * the backward of block l reads dL/dX[l+1] from gin[l&1] and writes dL/dX[l] to gin[(l&1)^1]; gmid = dL/d x_mid. */
typedef struct VgVitWsMap {
  long long X, xn1, qkv, ao, xmid, xn2, z1, a1, lse, mean1, rstd1, mean2, rstd2;
  long long gin[2], gmid[2], dqkv[2], dz1[2];
  long long total;
  /* ABI v7 - the pruned tail of the TOP block: only the CLS rows of its output reach the classifier (modules.py:195), so behind its
   * attention the block runs on compact [B, E] tensors.  xtop = X[L] on the CLS rows (bf16 [B, E]; the rows of X at L*M*E are not
   * written any more), dxtop = dL/dX[L] on the CLS rows (bf16 [B, E], exactly zero on every other row; gin[] holds dL/dX[l] for l < L). */
  long long xtop, dxtop;
} VgVitWsMap;
int vg_vit_ws_map(const VgVitDims* d, int B, VgVitWsMap* out);

typedef struct VgVitNet {
  VgVitDims d;
  const float* P;   /* fp32 master parameters */
  const void* Pb;   /* bf16 shadow of P */
  float* G;         /* fp32 gradient accumulator (same layout); may be NULL when want_wgrad == 0 */
  /* nn.Dropout(p) at the reference's three sites (modules.py:80,170,176: embedding, after the attention
   * output projection, after fc2), fused into the GEMM epilogues.  p = 0 disables it (eval mode).  p is
   * quantised to 1/256; the mask is a counter-based hash of (dropout_seed, site, element index), so the
   * backward regenerates it: pass the SAME seed to the backward of a forward. */
  float dropout_p;
  unsigned long long dropout_seed;
  const unsigned* dropout_step; /* optional device counter mixed into the mask key (hipGraph replay); NULL = none */
  void* ctx;                    /* optional vg_ctx_create() handle: the backward runs its weight-gradient side on the
                                   context's second stream, concurrently with the input-gradient chain; NULL = one stream */
  int attn_fp8;                 /* 1: fp8 (OCP e4m3) MFMA operands for the attention's activation products, Q.K^T (forward
                                   and the backward's recompute) and P.V, as BASELINE.json's 128x128 configuration asks;
                                   gradient-carrying products stay bf16.  0 = bf16 everywhere (default; parity tiers) */
  int dense_top;                /* ABI v7.  0 (default): the top encoder block computes what the classifier reads - behind its attention
                                   only the B CLS rows (modules.py:195 takes x[:, 0, :]; the other rows of its output are never read and their
                                   gradient is exactly zero), forward, backward and weight gradients.  1: every row of it, like the blocks below -
                                   the reference's operator graph row for row (for A/B measurements and the test that the two agree) */
} VgVitNet;
/* img: [B,C,IH,IH] fp32 (img_is_bf16 = 0) or bf16; logits fp32 [B,Kc].  ws keeps everything the
 * backward needs; one ws per in-flight forward. */
int vg_vit_forward(const VgVitNet* net, int B, const void* img, int img_is_bf16, void* ws,
                   float* logits, void* stream);
/* ABI v9 (additive).  vg_vit_forward with identical arguments and side effects - the same launches in the same order, logits bit-equal,
 * ws valid for a following vg_vit_backward - that additionally writes feats fp32 [B, E]: the tensor the classifier's fc1 reads,
 * vit.norm(x)[:, 0, :] (modules.py:195,236), as the forward holds it (bf16, widened: every value is a bf16), on the pruned-tail path and
 * with dense_top alike.  The feature network of the Frechet distance (vg_moments_update below).  -1: a NULL pointer or B < 1. */
int vg_vit_features(const VgVitNet* net, int B, const void* img, int img_is_bf16, void* ws, float* logits, float* feats /*[B, E]*/,
                    void* stream);
/* dlogits fp32 [B,Kc].  d_img bf16 [B,C,IH,IH] or NULL.  want_wgrad: accumulate into net->G
 * (G += dL/dP); 0 skips every weight-gradient kernel (generator pass through D, training.py:204-210). */
int vg_vit_backward(const VgVitNet* net, int B, void* ws, const float* dlogits, void* d_img,
                    int want_wgrad, void* stream);
/* The same backward in pieces, for overlapping the data-parallel gradient all-reduce with compute:
 * stage 0 = classifier head + final LayerNorm, stages 1..L = encoder blocks L-1..0, stage L+1 = patch
 * embedding.  Calls must cover [0, L+2) in increasing order on one stream with the same arguments.
 * After a call returning stages up to s, the gradients of blocks >= L-s (a contiguous tail of the
 * flat buffer, from layer0 + (L-s)*layer_stride) are final for this backward. */
int vg_vit_backward_stages(const VgVitNet* net, int B, void* ws, const float* dlogits, void* d_img,
                           int want_wgrad, int stage_begin, int stage_end, void* stream);

/* ABI v9.  The WGAN-GP gradient penalty of the reference's Wasserstein step as ONE call (replaces the autograd double backward over
 * the operator set; reference: gradient_penalty, src/v2/utils.py:124-144, and its call site src/v2/training.py:101-106):
 *   penalty = mean_b (|| d sum(D(x^_b)) / d x^_b ||_2 - 1)^2,  x^ = eps real + (1 - eps) fake;   net->G += weight * d penalty / d theta;
 *   *penalty_out = penalty (device float).  real / fake: bf16 [B, C, IH, IH]; eps: device fp32 [B] (the reference draws torch.rand).
 * ws: a vg_vit_ws_bytes(d, B) workspace (the call runs its own forward in it); ws_pen: vg_vit_penalty_ws_bytes(d, B) bytes.
 * The discriminator runs in train mode like the reference's does: net->dropout_p / dropout_seed / dropout_step give the masks (one set
 * for all passes of the call).  net->dense_top and net->ctx are ignored (every row of the top block; one stream).  Every network
 * vg_vit_layout accepts; where the full-row kernels take the shape (E = 384 / 512, B * tokens a multiple of 16) the input gradients +
 * LayerNorm backwards are fused.  -3: attn_fp8 (the second-order attention kernel differentiates the bf16 one), B * E not a multiple of 8. */
long long vg_vit_penalty_ws_bytes(const VgVitDims* d, int B);
int vg_vit_penalty(const VgVitNet* net, int B, const void* real, const void* fake, const float* eps, float weight, void* ws, void* ws_pen,
                   float* penalty_out, void* stream);
/* The zero-centred R1 penalty on real images (Mescheder et al. 2018), the regulariser of the non-saturating / hinge recipes, as ONE
 * call (additive to ABI v9; the body is vg_vit_penalty's with another front and another seed of the second backward):
 *   penalty = mean_b || d sum_k D(x_b)_k / d x_b ||_2^2;   net->G += weight * d penalty / d theta;   *penalty_out = penalty (device
 *   float, unweighted).  The caller folds gamma / 2 and a lazy-regularisation interval into weight (weight = interval * gamma / 2).
 * x: bf16 [B, C, IH, IH], fed to the forward as it is (no interpolation launch, no fp32 copy).  ws / ws_pen: exactly vg_vit_ws_bytes(d, B)
 * and vg_vit_penalty_ws_bytes(d, B) bytes.  Dropout, dense_top, ctx and the return codes as in vg_vit_penalty: -1 a null argument,
 * B < 1 or net->G missing (decided on the host before any launch); -3 attn_fp8, more than 80 tokens, or the same alignment conditions. */
int vg_vit_r1(const VgVitNet* net, int B, const void* x, float weight, void* ws, void* ws_pen, float* penalty_out, void* stream);

/* fp32 mode of the same network (opt-in; the bf16 entry points above are unchanged): activations, saved tensors, gradients and GEMM
 * operands are fp32, the GEMMs run on the exact f32-input MFMA (v_mfma_f32_16x16x4_f32).  Reads net->P (fp32 master), accumulates
 * G += dL/dP into net->G (same flat layout); dropout_p / dropout_seed / dropout_step give the same masks as the bf16 engine
 * (vg_dropout_apply).  net->Pb, net->ctx and net->dense_top are ignored (every row of every block; one stream); net->attn_fp8 = 1
 * returns -4.  img / d_img: fp32 [B,C,IH,IH] (d_img may be NULL); logits / dlogits fp32 [B,Kc].  ws: vg_vit_ws_bytes_f32(d, B)
 * bytes, written by the forward and read by the backward of that forward.  -1 null pointer / B < 1, -3 a shape vg_vit_layout
 * refuses. */
long long vg_vit_ws_bytes_f32(const VgVitDims* d, int B); /* host only */
int vg_vit_forward_f32(const VgVitNet* net, int B, const float* img, void* ws, float* logits, void* stream);
int vg_vit_backward_f32(const VgVitNet* net, int B, void* ws, const float* dlogits, float* d_img, int want_wgrad, void* stream);

/* Single operators of the fp32 mode (all tensors fp32, row-major):
 * vg_linear_f32_fwd:   Y[M,N] = act(X[M,K] W[N,K]^T + bias) * mask(site) + res; act 0 none, 1 exact-erf GELU (Z = pre-activation,
 *                      nullable), 2 tanh; drop_p = 0: no dropout, else the mask of vg_dropout_apply over the [M,N] output.
 * vg_linear_f32_dgrad: dX[M,K] = (dY[M,N] W[N,K]) * f(aux); act 0: f = 1, 1: gelu'(aux) (aux = pre-activation), 2: 1 - aux^2 (aux = tanh out).
 * vg_linear_f32_wgrad: dW[N,K] += dY^T X, db[N] += column sums of dY (db nullable); split-K slices folded in a fixed order
 *                      (bitwise deterministic); slab: vg_linear_f32_wgrad_slab_floats(M, N, K) floats of scratch (-2 if smaller).
 * vg_attention_f32_fwd / _bwd: as vg_attention_fwd / _bwd in fp32 (HE in {32,64,96}, S <= 80; lse fp32 [B,H,S]).
 * vg_layernorm_f32_fwd / _bwd: nn.LayerNorm over E (a multiple of 128, <= 1024); bwd: dx = gres + LN'(dy) (gres nullable),
 *                      dgamma / dbeta += column sums (both NULL: skipped), part: vg_layernorm_f32_bwd_part_floats(R, E) floats. */
int vg_linear_f32_fwd(const float* X, const float* W, const float* bias, const float* res, float* Y, float* Z, int M, int N, int K, int act,
                      float drop_p, unsigned long long seed, int site, const unsigned* step_dev, void* stream);
int vg_linear_f32_dgrad(const float* dY, const float* W, const float* aux, float* dX, int M, int N, int K, int act, void* stream);
long long vg_linear_f32_wgrad_slab_floats(int M, int N, int K);
int vg_linear_f32_wgrad(const float* dY, const float* X, float* dW, float* db, float* slab, long long slab_floats, int M, int N, int K,
                        void* stream);
int vg_attention_f32_fwd(const float* qkv, float* out, float* lse, int B, int H, int S, int HE, float scale, void* stream);
int vg_attention_f32_bwd(const float* qkv, const float* out, const float* d_out, const float* lse, float* d_qkv, int B, int H, int S, int HE,
                         float scale, void* stream);
int vg_layernorm_f32_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int R, int E, float eps,
                         void* stream);
long long vg_layernorm_f32_bwd_part_floats(int R, int E);
int vg_layernorm_f32_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, const float* gres, float* dx,
                         float* dgamma, float* dbeta, float* part, int R, int E, void* stream);
/* v1 generator: mapping Linear -> L x TransformerSLN -> SLN -> SIREN x2 (src/v1/generator.py:58-69). */
typedef struct VgGenDims {
  int Z, T, E, H, L, O, CW; /* latent, tokens, embed, heads, layers, siren hidden, output features per token */
  float omega0;
  /* Token geometry.  patch == 0: the reference's v1 layout - one token per image ROW, CW = channels*image_w and the
   * [B, T*CW] result IS the image through a flat view (generator.py:19,25,66-68).
   * patch > 0: tokens on the discriminator's patch grid - T = (IH/patch)^2, CW = C*patch^2 in
   * conv1's (c, py, px) order - and the image is assembled by the un-patchify scatter.  Not in the reference. */
  int patch, C, IH;
} VgGenDims;
typedef struct VgGenLayout {
  long long emb, map_w, map_b;                  /* embedding [T,E], mapping Linear [T*E, Z], bias */
  long long layer0, layer_stride;
  long long wqkv, wo, wm;                       /* per block, relative: all q heads | k heads | v heads [3E,E]; output_linear; mlp */
  long long sln1_w, sln1_b, sln1_s, sln2_w, sln2_b, sln2_s, bo, bm; /* *_s: [gamma, beta] scalars */
  long long layer_weights;
  long long slnf_w, slnf_b, slnf_s, s1_w, s1_b, s2_w, s2_b;
  long long total;
} VgGenLayout;
int vg_gen_layout(const VgGenDims* d, VgGenLayout* out);
long long vg_gen_ws_bytes(const VgGenDims* d, int B);
/* Workspace introspection for the parity tests (host only), byte offsets; R = B*T rows.  Per block l: s1 / cat / htmp /
 * s2 / hout at + l*R*E*2, qkv at + l*R*3E*2.  wmod = the mapping output [R,E]; sf = final SLN output; y1 = first SIREN
 * output, zf1 / zf2 = fp32 SIREN pre-activations.  g[0..2]: gradient buffers of the backward - dL/d h entering block l
 * (from above) is in g[0] when L-1-l is even, g[2] when odd; g[1] holds dL/d h_tmp of the block being processed.
 * dw_acc: fp32 [R,E] gradient of the modulation vector, summed over the SLN uses processed so far. */
typedef struct VgGenWsMap {
  long long wmod, s1, qkv, cat, htmp, s2, hout, sf, y1, zf1, zf2, g[3], dw_acc, total;
} VgGenWsMap;
int vg_gen_ws_map(const VgGenDims* d, int B, VgGenWsMap* out);
typedef struct VgGenNet {
  VgGenDims d;
  const float* P;
  const void* Pb;
  float* G;
  /* Dropout after msha.output_linear and inside the block MLP (src/v1/config.py:36,39: 0.2 / 0.2). */
  float dropout_p;
  unsigned long long dropout_seed;
  const unsigned* dropout_step;
  /* Optional Fourier positional input of the SIREN (named by BASELINE.json's north_star; NOT in the reference):
   * fp32 [T, E] table added to the final SLN output of every image before output_network.0.  NULL = reference. */
  const float* pos_table;
} VgGenNet;
/* z fp32 [B,Z]; img bf16 [B, T*CW]: the flat view of generator.py:66-68 (patch == 0) or NCHW [B,C,IH,IH] (patch > 0). */
int vg_gen_forward(const VgGenNet* net, int B, const float* z, void* ws, void* img, void* stream);
int vg_gen_backward(const VgGenNet* net, int B, void* ws, const void* d_img, void* stream);
/* The same backward in pieces (data-parallel overlap, and block-by-block parity tests): stage 0 = SIREN output layers +
 * final SLN, stages 1..L = blocks L-1..0, stage L+1 = learned embedding + mapping Linear.  Calls must cover [0, L+2) in
 * increasing order on one stream with the same arguments.  After the call that returns stage s (1 <= s <= L) the
 * gradients from layer0 + (L-s)*layer_stride to the end of the flat buffer are final for this backward. */
int vg_gen_backward_stages(const VgGenNet* net, int B, void* ws, const void* d_img, int stage_begin,
                           int stage_end, void* stream);
/* The class-conditional generator: w = mapping(z) + class_embedding[y] - the classic cGAN input Linear([z ; onehot(y)]) with its K one-hot
 * columns evaluated as a gather.  table_bf16 / table_grad: the embedding [K, T*E] as the bf16 shadow the forward reads and the fp32
 * gradient the backward ACCUMULATES into (table_grad may be NULL for a forward); labels int32 [B] on the device.  The forward is
 * vg_gen_forward plus one vg_class_add on the mapping output; the backward adds one vg_class_grad in stage L+1, beside the mapping bias's
 * column sum.  cond == NULL is exactly the plain call (vg_gen_forward / _backward / _backward_stages ARE these with NULL).
 * -1: a null labels / table (backward: table_grad);  -2: K outside [1, 16] - before any launch. */
typedef struct VgGenCond {
  const int* labels;
  const void* table_bf16;
  float* table_grad;
  int K;
} VgGenCond;
int vg_gen_forward_cond(const VgGenNet* net, int B, const float* z, void* ws, void* img, const VgGenCond* cond, void* stream);
int vg_gen_backward_cond(const VgGenNet* net, int B, void* ws, const void* d_img, const VgGenCond* cond, void* stream);
int vg_gen_backward_stages_cond(const VgGenNet* net, int B, void* ws, const void* d_img, int stage_begin, int stage_end,
                                const VgGenCond* cond, void* stream);

/* fp32 mode of the generator (opt-in, additive to ABI v9; every entry point above is unchanged): activations, saved tensors, gradients
 * and GEMM operands are fp32, the GEMMs run on the exact f32-input MFMA, the SIREN's sine and cosine are the accurate library functions
 * of fl(omega0 * z) - the reference's own arithmetic, for holding the generator to the fp32 oracle and sampling a reference checkpoint.
 * Reads net->P (fp32 master) and accumulates G += dL/dP into net->G in the vg_gen_layout order; net->Pb is ignored.  Dropout at the bf16
 * generator's sites and element indices (100 + 2l behind output_linear, 101 + 2l inside the MLP), so one seed draws the same masks in
 * both modes; net->pos_table is honoured.  z fp32 [B, Z]; img / d_img fp32 [B, T*CW] (patch == 0) or NCHW (patch > 0).  ws:
 * vg_gen_ws_bytes_f32(d, B) bytes (-1 for arguments the calls refuse), written by the forward and read by the backward of that forward.
 * cond (NULL: unconditional) is the class table [K, T*E] and its gradient in fp32: w = mapping(z) + table[clamp(y)], the gradient by
 * vg_class_grad (ascending n, accumulated).  One stream, no atomics: two runs are bit-equal.
 * Refused on the host before any launch:  -1 a null pointer (net, P, z, ws, img; G and d_img for the backward; labels / table /
 * table_grad of a cond) or B < 1;  -2 K outside [1, 16];  -3 a shape vg_gen_layout refuses, T > 80 or E > 1024 (E / H outside
 * {32, 64, 96} is vg_gen_layout's). */
typedef struct VgGenCondF32 {
  const int* labels;
  const float* table;
  float* table_grad; /* NULL allowed for a forward */
  int K;
} VgGenCondF32;
long long vg_gen_ws_bytes_f32(const VgGenDims* d, int B); /* host only */
int vg_gen_forward_f32(const VgGenNet* net, int B, const float* z, void* ws, float* img, const VgGenCondF32* cond, void* stream);
int vg_gen_backward_f32(const VgGenNet* net, int B, void* ws, const float* d_img, const VgGenCondF32* cond, void* stream);
/* Its single operators (all tensors fp32, row-major):
 * vg_sln_f32_fwd / _bwd: vg_sln_fwd / vg_sln_bwd above in fp32 over rows [R, E], E a multiple of 128 and at most 1024; mean / rstd [R]
 *   saved.  bwd: dh = gres + LN'(dy w gs) (gres nullable); dw_acc [R, E] = (dw_accumulate 0) or += (1) dy (gs (xhat lw + lb) + bs);
 *   dlw, dlb [E] and dgs, dbs [1] += their sums over the rows (all four NULL: skipped) - fp64 inside a 256-row chunk, the chunks folded
 *   in order, bitwise repeatable.  part: vg_sln_f32_bwd_part_floats(R, E) floats of scratch, 8-byte aligned (-3 otherwise).
 * vg_siren_f32_fwd:   Z[M,N] = X[M,K] W[N,K]^T + bias (the fp32 pre-activation, required), Y = sin(fl(omega0 * Z)).
 * vg_siren_f32_dgrad: dX[M,K] = (dY[M,N] W[N,K]) * omega0 cos(fl(omega0 * aux)), aux [M,K] = the pre-activation of the layer below;
 *   W == NULL is the last layer's elementwise form over [M, N]: dX = dY * omega0 cos(fl(omega0 * aux)) (K ignored).
 *   Accurate sinf / cosf: the argument reaches hundreds of radians. */
int vg_sln_f32_fwd(const float* h, int h_bcast_rows, const float* w, const float* lw, const float* lb, const float* gs, const float* bs,
                   float* y, float* mean, float* rstd, int R, int E, float eps, void* stream);
long long vg_sln_f32_bwd_part_floats(int R, int E);
int vg_sln_f32_bwd(const float* dy, const float* h, int h_bcast_rows, const float* w, const float* mean, const float* rstd, const float* lw,
                   const float* lb, const float* gs, const float* bs, const float* gres, float* dh, float* dw_acc, int dw_accumulate,
                   float* dlw, float* dlb, float* dgs, float* dbs, float* part, int R, int E, void* stream);
int vg_siren_f32_fwd(const float* X, const float* W, const float* bias, float* Y, float* Z, int M, int N, int K, float omega0, void* stream);
int vg_siren_f32_dgrad(const float* dY, const float* W, const float* aux, float* dX, int M, int N, int K, float omega0, void* stream);

/* Per-step telemetry, written by the step itself (additive to ABI 9; csrc/telemetry.hip).  The reference's trainer collects per-step
 * series - gen_losses, disc_losses, gradient_norms_gen / _disc, disc_real_accuracies / disc_fake_accuracies (src/v2/training.py:80-84,
 * 112-123) - on the host; here the step writes them into rings on the device, keyed on the device step counter, and the host reads
 * them when it synchronises anyway.  All three entries are enqueue-only (no allocation, no synchronisation, no memset / memcpy node),
 * deterministic (no float atomics; every sum is a fixed tree) and use plain vector stores.
 *
 * vg_grad_stats: segmented gradient norms over a flat fp32 gradient buffer g[0, n) (16-byte aligned, n < 2^31).
 *   chunks: int32 [n_chunks][3] on the device = (first element, count, segment) with 1 <= count <= 4096; a chunk never crosses a
 *     segment, the chunks of a segment are adjacent and ascending.  seg_first: int32 [n_seg + 1] on the device, the index of each
 *     segment's first chunk (seg_first[n_seg] = n_chunks).  scratch: 2 n_chunks floats, 8-byte aligned.
 *   Pass 1 (at most 2048 workgroups of 256 threads walking the table grid-stride; ONE partial per chunk, so the result does not depend
 *     on the grid): the chunk is split at g's 16-byte boundaries into a head of (-first) & 3 elements, nv float4 and a tail.  Thread t:
 *     a = 0; for k = 0..3 with v = t + 256 k < nv: a += (x0 x0 + x1 x1) + (x2 x2 + x3 x3) of vector v; thread t < head then adds the
 *     square of head element t, thread t < tail the square of tail element t (products and sums rounded separately, fp32).  The 256
 *     values are folded by the wave butterfly (xor 32, 16, 8, 4, 2, 1) and then as (w0 + w1) + (w2 + w3).  Elements that are NaN or
 *     +-Inf are counted.  Nothing outside a chunk is read; a chunk that does not lie inside [0, n) is skipped.
 *   Pass 2 (one workgroup): per segment s the chunk partials are added in chunk order in fp64;
 *     norm_seg[s] = (float)(gscale sqrt(sum_s)),
 *     totals[0] = sum_s norm_seg[s]   (the rounded norms, added in segment order in fp64: sum(p.grad.norm() for p in parameters)),
 *     totals[1] = gscale sqrt(sum_s sum_s)   (what clip_grad_norm_ sees),  totals[2] = min(non-finite elements, 2^24),  totals[3] = 0.
 *   totals: 4 floats, 16-byte aligned.  Returns -1: a null pointer;  -2: n, n_chunks or n_seg out of range (n_seg <= 2048, n_seg <=
 *   n_chunks), gscale not positive and finite;  -3: a misaligned buffer - all before any launch.
 *
 * vg_logit_stats: statistics of n logits (1 <= n <= 16384) per row pointer; workgroup j of the launch reads x_j and writes slot
 *   role + j of out[3][4] (role: 0 = D on real, 1 = D on fake, 2 = the generator's pass; x1 may be NULL: one workgroup; with x1,
 *   role <= 1) as (mean, fraction of logits > 0, fraction of logits < 0, n) in one 16-byte store.  +-0 and NaN count in neither
 *   fraction ((real_output > 0) / (fake_output < 0), training.py:115-116).  Sum: thread t of 1024 adds x[t], x[t + 1024], .. in index
 *   order, the wave butterfly, then the 16 wave sums by one more butterfly (lanes >= 16 hold +0); mean = sum / (float) n; the counts
 *   are integers and each fraction is one fp32 division.  -1: x0 or out NULL;  -2: n or role out of range;  -3: out misaligned.
 *
 * vg_telemetry_commit: with t = step_dev[0] as vg_zero_tick left it (t < 1: nothing is written), row r = (t - 1) % cap receives
 *   ring_step[r] = t, ring[r][f] = field f (VG_TEL_*, below) gathered from the device pointers of *src (passed by value: a host
 *   pointer, read before the call returns), ring_seg_d[r][0, n_seg_d) = src->seg_d and ring_seg_g likewise.  A NULL source makes its
 *   fields NaN; the penalty field is NaN - written, not left over - when penalty_due is 0 (a step of lazy R1 on which the penalty does
 *   not run).  The row is a function of the counter: writing it twice (the warm-up of a captured step and its first replay) is
 *   idempotent.  One workgroup.  -1: a null pointer (a ring of a given source included);  -2: cap < 1, a negative size, penalty_due
 *   not 0 / 1;  -3: a source with size 0. */
#define VG_TEL_LOSS_D_REAL 0
#define VG_TEL_LOSS_D_FAKE 1
#define VG_TEL_LOSS_G 2
#define VG_TEL_D_REAL_MEAN 3
#define VG_TEL_D_FAKE_MEAN 4
#define VG_TEL_D_REAL_ACC 5   /* fraction of D's real logits > 0 */
#define VG_TEL_D_FAKE_ACC 6   /* fraction of D's fake logits < 0 */
#define VG_TEL_G_MEAN 7       /* the generator's pass through D: mean logit */
#define VG_TEL_G_FRAC_POS 8   /* ... and the fraction of its logits > 0 */
#define VG_TEL_GNORM_D_SUM 9
#define VG_TEL_GNORM_D_L2 10
#define VG_TEL_GNORM_G_SUM 11
#define VG_TEL_GNORM_G_L2 12
#define VG_TEL_NONFINITE_D 13
#define VG_TEL_NONFINITE_G 14
#define VG_TEL_PENALTY 15     /* gp_loss or r1_loss of this step */
#define VG_TEL_BCR_REAL 16
#define VG_TEL_BCR_FAKE 17
#define VG_TEL_ADA_P 18
#define VG_TEL_ADA_RT 19
#define VG_TEL_LR_D 20
#define VG_TEL_LR_G 21
#define VG_TEL_DIVERSITY 22
#define VG_TEL_NF 24          /* floats per row (23 is reserved and NaN) */
typedef struct VgTelemetrySrc {
  const float* losses;       /* [3] d_real, d_fake, g */
  const float* logit_stats;  /* [3][4] as vg_logit_stats writes it */
  const float* grad_d;       /* [4] totals of vg_grad_stats over the discriminator's gradient */
  const float* grad_g;       /* [4] ... over the generator's */
  const float* penalty;      /* [1] */
  const float* bcr;          /* [2] real, fake */
  const float* ada_state;    /* [4] (p, acc_sign, acc_count, r_last) */
  const float* lr;           /* [2] d, g */
  const float* diversity;    /* [1] */
  const float* seg_d;        /* [n_seg_d] norm_seg of the discriminator */
  const float* seg_g;        /* [n_seg_g] */
  int n_seg_d, n_seg_g;
  int penalty_due;           /* 0 or 1 */
} VgTelemetrySrc;
int vg_grad_stats(const float* g, long long n, const int* chunks, int n_chunks, const int* seg_first, int n_seg, float gscale,
                  float* scratch, float* norm_seg, float* totals /*[4]*/, void* stream);
int vg_logit_stats(const float* x0, const float* x1, int n, int role, float* out /*[3][4]*/, void* stream);
int vg_telemetry_commit(const VgTelemetrySrc* src, const int* step_dev, int cap, int* ring_step, float* ring, float* ring_seg_d,
                        float* ring_seg_g, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VITGAN_HIP_H */
