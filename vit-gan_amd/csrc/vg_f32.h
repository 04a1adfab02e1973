// Internal launch API of the fp32 mode (fp32 activations, saved tensors, gradients and GEMM operands).  All functions only
// enqueue work; negative returns are argument-validation codes (nothing launched).
#pragma once
#include "vg_common.h"

// C[m][n] = sum_k A(m,k) B(k,n); A(m,k) = A[m*sam + k*sak], B(k,n) = B[k*sbk + n*sbn] (sak == 1 or sam == 1; sbn == 1 or sbk == 1).
// Epilogue (forward forms): v = acc + bias[n]; act 1: Z[m][n] = v (nullable), v = gelu(v); act 2: v = tanh(v); v *= dropout factor of
// element m * N + n (drop.thr != 0); v += res[m][n].  Input-gradient forms: act 3: v *= gelu'(aux[m][n]) (aux = pre-activation);
// act 4: v *= 1 - aux^2 (aux = tanh output).  SIREN forms (an instantiation of their own; no dropout, no residual): act 5:
// Z[m][n] = v (required), v = sin(fl(omega0 * v)); act 6: v *= omega0 * cos(fl(omega0 * aux[m][n])) (aux = pre-activation) - the
// accurate sinf / cosf, whose argument reduction holds at hundreds of radians.  c_split != 0 (split-K): K is cut into `splits` slices of kchunk (a multiple of 16);
// slice z writes its own fp32 slab C + z * c_split with no epilogue, folded later in slice order.
struct VgF32Gemm {
  const float* A; long long sam, sak;
  const float* B; long long sbk, sbn;
  int M, N, K;
  float* C; long long ldc; long long c_split; int splits, kchunk;
  const float* bias; int act;
  const float* aux; long long ldaux;
  float* Z; long long ldz;
  const float* res; long long ldr;
  VgDrop drop;
  float omega0;
};
enum { VG_F32_ACT_NONE = 0, VG_F32_ACT_GELU = 1, VG_F32_ACT_TANH = 2, VG_F32_MUL_GELU = 3, VG_F32_MUL_TANH = 4, VG_F32_ACT_SIN = 5,
       VG_F32_MUL_COS = 6 };
int vg_f32_gemm_launch(const VgF32Gemm& g, hipStream_t st);

// nn.Linear in its three forms over row-major operands: X [M,K], W [N,K], Y [M,N]
int vg_f32_linear_fwd(const float* X, const float* W, const float* bias, const float* res, float* Y, float* Z, int M, int N, int K, int act,
                      VgDrop drop, hipStream_t st);
int vg_f32_linear_dgrad(const float* dY, const float* W, const float* aux, float* dX, int M, int N, int K, int act, hipStream_t st);
// SIREN layer: Y = sin(omega0 * (X W^T + bias)), Z = the fp32 pre-activation; its input gradient dX = (dY W) * omega0 cos(omega0 * aux)
int vg_f32_siren_fwd(const float* X, const float* W, const float* bias, float* Y, float* Z, int M, int N, int K, float omega0, hipStream_t st);
int vg_f32_siren_dgrad(const float* dY, const float* W, const float* aux, float* dX, int M, int N, int K, float omega0, hipStream_t st);
// dW [N,K] += dY^T X (split-K over M into slabs, folded in slice order); db [N] += column sums of dY (nullable)
long long vg_f32_wgrad_slab_floats(int M, int N, int K);
int vg_f32_linear_wgrad(const float* dY, const float* X, float* dW, float* db, float* slab, int M, int N, int K, hipStream_t st);

// deterministic column sums of X [R, n0 + n1]: d0[c] += sum_r X[r][c] (c < n0), d1[c - n0] += ... (n0 <= c < n0 + n1).  fp64 inside
// a 256-row chunk, the chunks folded in order; part: vg_f32_colsum_parts(R) * (n0 + n1) floats
int vg_f32_colsum_parts(int R);
int vg_f32_colsum_launch(const float* X, long long ld, int R, float* part, float* d0, int n0, float* d1, int n1, hipStream_t st);
// dgamma[c] += sum_r dy[r][c] * xhat[r][c], dbeta[c] += sum_r dy[r][c] (same chunking); part: 2E * vg_f32_colsum_parts(R) floats
int vg_f32_ln_param_grads(const float* dy, const float* x, long long xs, const float* mean, const float* rstd, float* dgamma, float* dbeta,
                          float* part, int R, int E, hipStream_t st);

// y = x * dropout mask over element indices [0, n) (the counter-based mask of vg_common.h)
int vg_f32_dropout_launch(const float* x, float* y, long long n, VgDrop drop, hipStream_t st);

// attention with dot-product scores: qkv [B*S, 3*H*HE], out [B*S, H*HE], lse [B,H,S]; HE in {32, 64, 96}, S <= 80
int vg_f32_attn_fwd_launch(const float* qkv, float* out, float* lse, int B, int H, int S, int HE, float scale, hipStream_t st);
int vg_f32_attn_bwd_launch(const float* qkv, const float* o, const float* d_o, const float* lse, float* dqkv, int B, int H, int S, int HE,
                           float scale, hipStream_t st);

// LayerNorm over E (a multiple of 128, <= 1024), biased variance; xs / ys / dxs: row strides
int vg_f32_ln_fwd_launch(const float* x, long long xs, const float* gamma, const float* beta, float* y, long long ys, float* mean,
                         float* rstd, int R, int E, float eps, hipStream_t st);
// dx = gres + LN'(dy) (gres nullable, same stride as dx; dy [R, E] dense); dgamma / dbeta += column sums (both NULL: skipped);
// part: 2E * vg_f32_colsum_parts(R) floats
int vg_f32_ln_bwd_launch(const float* dy, const float* x, long long xs, const float* mean, const float* rstd, const float* gamma,
                         const float* gres, float* dx, long long dxs, float* dgamma, float* dbeta, float* part, int R, int E, hipStream_t st);

// patch embedding: img [B,C,IH,IH] <-> tiles [B*NP, C*P*P] (backward: d_img from d_tiles; every pixel lies in exactly one tile)
int vg_f32_patchify_launch(const float* img, float* tiles, int B, int C, int IH, int P, int backward, hipStream_t st);
// X[b*S + s] = mask * (s == 0 ? cls : tok[b*NP + s-1] + pos[s-1]), mask of element (b*S + s) * E + e
int vg_f32_embed_assemble_launch(const float* tok, const float* pos, const float* cls, float* X, int B, int S, int E, VgDrop drop,
                                 hipStream_t st);
// gm = g * mask over [B*S, E]; gt[b*NP + p] = gm[b*S + 1 + p]
int vg_f32_embed_grad_launch(const float* g, float* gm, float* gt, int B, int S, int E, VgDrop drop, hipStream_t st);

// ---- the generator's fp32 pieces (gen_f32.hip)
// self-modulated LayerNorm: y = w * (gs * (LN(h) * lw + lb) + bs) over rows [R, E]; hb > 0: h is [hb, E], row r reads row r % hb
int vg_f32_sln_fwd_launch(const float* h, int hb, const float* w, const float* lw, const float* lb, const float* gs, const float* bs, float* y,
                          float* mean, float* rstd, int R, int E, float eps, hipStream_t st);
// dh = gres + LN'(dy w gs) (gres nullable); dw_acc (=, += with accumulate) dy (gs (xhat lw + lb) + bs); dlw / dlb [E], dgs / dbs [1] +=
// their sums (all four or none), fp64 inside a 256-row chunk, the chunks folded in order.  part: vg_f32_sln_part_floats(R, E) floats,
// 8-byte aligned
long long vg_f32_sln_part_floats(int R, int E);
int vg_f32_sln_bwd_launch(const float* dy, const float* h, int hb, const float* w, const float* mean, const float* rstd, const float* lw,
                          const float* lb, const float* gs, const float* bs, const float* gres, float* dh, float* dw_acc, int dw_accumulate,
                          float* dlw, float* dlb, float* dgs, float* dbs, float* part, int R, int E, hipStream_t st);
// dz = dy * omega0 cos(fl(omega0 * z)) over n elements
int vg_f32_sin_grad_launch(const float* dy, const float* z, float* dz, long long n, float omega0, hipStream_t st);
// y[i] = x[i % period] (+ add[i], nullable) over n elements: the embedding broadcast over the batch; x += table broadcast likewise
int vg_f32_bcast_launch(const float* x, long long period, const float* add, float* y, long long n, hipStream_t st);
// wmod[n][j] += table[clamp(labels[n], 0, K - 1)][j] over [B, N]
int vg_f32_class_add_launch(float* wmod, const float* table, const int* labels, int B, long long N, int K, hipStream_t st);
