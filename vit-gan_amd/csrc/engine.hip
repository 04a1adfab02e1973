// Whole-network passes: sequences the gfx950 kernels for the v2 VisionTransformer (discriminator)
// and the v1 SLN/SIREN generator.  Host code only enqueues work on one stream: no allocation, no
// synchronisation, so a pass (or a whole G/D step) can be captured into a hipGraph by the caller.
//
// Data layout (all row-major, bf16 unless noted):
//   tokens      X[l]   [B*S, E]      residual stream entering block l (X[L] = trunk output)
//   qkv[l]             [B*S, 3E]     Q | K | V thirds, head h at columns h*HE.. of each third
//   flat params        fp32 master P, bf16 shadow Pb, fp32 grads G share ONE offset table
//                      (VgVitLayout / VgGenLayout): per block the four GEMM weights are contiguous so
//                      their split-K wgrad slabs fold into G with a single streaming kernel.
#include "../../include/vitgan_hip.h"
#include "vg_kernels.h"
#include "vg_row.h"

static inline long long al64(long long x) { return (x + 63) & ~63LL; }

// Optional execution context: a second stream + events so that the weight-gradient side of a backward
// (wgrad GEMMs, bias / LayerNorm-affine reductions - everything that only writes the gradient buffer) runs
// concurrently with the input-gradient chain of the next block and fills the CUs its short tails leave idle.
#define VG_CTX_EVENTS 72
struct VgCtx {
  hipStream_t side;
  hipEvent_t ev_main[VG_CTX_EVENTS], ev_side[VG_CTX_EVENTS];
};
extern "C" int vg_ctx_create(void** out) {
  if (!out) return -1;
  VgCtx* c = new VgCtx();
  hipError_t e = hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking);
  if (e != hipSuccess) { delete c; return (int)e; }
  for (int i = 0; i < VG_CTX_EVENTS; ++i) {
    if ((e = hipEventCreateWithFlags(&c->ev_main[i], hipEventDisableTiming)) != hipSuccess) return (int)e;
    if ((e = hipEventCreateWithFlags(&c->ev_side[i], hipEventDisableTiming)) != hipSuccess) return (int)e;
  }
  *out = c;
  return 0;
}
extern "C" int vg_ctx_destroy(void* ctx) {
  if (!ctx) return 0;
  VgCtx* c = (VgCtx*)ctx;
  for (int i = 0; i < VG_CTX_EVENTS; ++i) { (void)hipEventDestroy(c->ev_main[i]); (void)hipEventDestroy(c->ev_side[i]); }
  (void)hipStreamDestroy(c->side);
  delete c;
  return 0;
}

// =============================================================================================
//                                       layouts
// =============================================================================================
extern "C" int vg_vit_layout(const VgVitDims* d, VgVitLayout* o) {
  if (!d || !o) return -1;
  const long long E = d->E, K = (long long)d->C * d->P * d->P, NP = (long long)(d->IH / d->P) * (d->IH / d->P);
  if (d->E % 128 || d->E % d->H || d->IH % d->P || (K & 7) || d->L < 1 || d->Kc < 1 || d->R < 1) return -3;
  const int HE = d->E / d->H;
  if (HE != 32 && HE != 64 && HE != 96) return -3;
  if (NP + 1 > VG_ATTN_LONG_MAX_S) return -3;  // attention: S <= 80 on every path, 80 < S <= 256 on the dot-product bf16 one
  // depth: the backward queues 3 deferred folds per block + 3 more (classifier head, final LayerNorm, the pruned top block's CLS-summed
  // bias row) and uses one event pair per block (+1 for the join)
  if (3 * d->L + 3 > VG_MAX_FOLD_JOBS || d->L >= VG_CTX_EVENTS - 1) return -3;
  long long p = 0;
  o->conv_w = p; p = al64(p + E * K);
  o->conv_b = p; p = al64(p + E);
  o->pos = p; p = al64(p + NP * E);
  o->cls = p; p = al64(p + E);
  // per block (relative offsets)
  long long q = 0;
  o->wqkv = q; q += 3 * E * E;
  o->wo = q; q += E * E;
  o->w1 = q; q += (long long)d->R * E * E;
  o->w2 = q; q += (long long)d->R * E * E;
  o->layer_weights = q;
  o->ln1_w = q; q = al64(q + E);
  o->ln1_b = q; q = al64(q + E);
  o->bqkv = q; q = al64(q + 3 * E);
  o->bo = q; q = al64(q + E);
  o->ln2_w = q; q = al64(q + E);
  o->ln2_b = q; q = al64(q + E);
  o->b1 = q; q = al64(q + (long long)d->R * E);
  o->b2 = q; q = al64(q + E);
  o->layer0 = p; o->layer_stride = q;
  p += q * d->L;
  o->lnf_w = p; p = al64(p + E);
  o->lnf_b = p; p = al64(p + E);
  o->hw1 = p; p = al64(p + E * E);
  o->hb1 = p; p = al64(p + E);
  o->hw2 = p; p = al64(p + (long long)d->Kc * E);
  o->hb2 = p; p = al64(p + d->Kc);
  o->total = p;
  return 0;
}

extern "C" int vg_gen_layout(const VgGenDims* d, VgGenLayout* o) {
  if (!d || !o) return -1;
  const long long E = d->E, T = d->T;
  if (d->E % 128 || d->E % d->H || (d->Z & 7) || (d->O & 7) || (d->CW & 7) || d->T > VG_ATTN_LONG_MAX_S || d->L < 1) return -3;
  const int HE = d->E / d->H;
  if (HE != 32 && HE != 64 && HE != 96) return -3;
  if (d->patch < 0) return -3;
  if (2 * d->L + 3 > VG_MAX_FOLD_JOBS) return -3;  // the backward queues 2L+1 deferred SLN folds + the two SIREN bias gradients
  if (d->patch > 0) {  // tokens on the patch grid: T and CW are determined by the image geometry
    if (d->C < 1 || d->IH < d->patch || d->IH % d->patch) return -3;
    const int gh = d->IH / d->patch;
    if (d->T != gh * gh || d->CW != d->C * d->patch * d->patch) return -3;
  }
  long long p = 0;
  o->emb = p; p = al64(p + T * E);
  o->map_w = p; p = al64(p + T * E * d->Z);
  o->map_b = p; p = al64(p + T * E);
  long long q = 0;
  o->wqkv = q; q += 3 * E * E;
  o->wo = q; q += E * E;
  o->wm = q; q += E * E;
  o->layer_weights = q;
  o->sln1_w = q; q = al64(q + E);
  o->sln1_b = q; q = al64(q + E);
  o->sln1_s = q; q = al64(q + 2);
  o->sln2_w = q; q = al64(q + E);
  o->sln2_b = q; q = al64(q + E);
  o->sln2_s = q; q = al64(q + 2);
  o->bo = q; q = al64(q + E);
  o->bm = q; q = al64(q + E);
  o->layer0 = p; o->layer_stride = q;
  p += q * d->L;
  o->slnf_w = p; p = al64(p + E);
  o->slnf_b = p; p = al64(p + E);
  o->slnf_s = p; p = al64(p + 2);
  o->s1_w = p; p = al64(p + (long long)d->O * E);
  o->s1_b = p; p = al64(p + d->O);
  o->s2_w = p; p = al64(p + (long long)d->CW * d->O);
  o->s2_b = p; p = al64(p + d->CW);
  o->total = p;
  return 0;
}

// =============================================================================================
//                                     small helpers
// =============================================================================================
static VgGemmProb mk(const bf16* A, int lda, const bf16* Bm, int ldb, int M, int N, int K) {
  VgGemmProb p = vg_gemm_prob();
  p.A = A; p.lda = lda; p.B = Bm; p.ldb = ldb; p.M = M; p.N = N; p.K = K;
  return p;
}
// forward Linear: C = act(A W^T + b) (+res)
static int lin_fwd(const bf16* A, int K, const bf16* W, const float* bias, bf16* C, int M, int N, int act, float ascale,
                   const bf16* res, bf16* pre_bf16, float* pre_f32, hipStream_t st, VgDrop drop = VgDrop(), int c2_gelu_grad = 0) {
  VgGemmProb p = mk(A, K, W, K, M, N, K);
  p.c2_gelu_grad = c2_gelu_grad;
  p.drop = drop;
  p.C = C; p.ldc = N; p.bias = bias; p.act = act; p.act_scale = ascale;
  p.res = res; p.ldr = N; p.C2 = pre_bf16; p.ldc2 = N;
  if (pre_f32) { p.pre_f32 = 1; p.Cf = pre_f32; p.ldcf = N; }
  return vg_gemm_launch(&p, 1, VG_NT, st);
}
// dgrad: dX[M,K] = dY[M,N] W[N,K]
static int lin_dgrad(const bf16* dY, const bf16* W, bf16* dX, int M, int N, int K, int mul, const bf16* Z, const float* Zf,
                     float ascale, hipStream_t st) {
  VgGemmProb p = mk(dY, N, W, K, M, K, N);  // GEMM (M x K_out=K) with reduction N
  p.C = dX; p.ldc = K; p.act = mul; p.act_scale = ascale; p.Z = Z; p.ldz = K; p.Zf = Zf; p.ldzf = K;
  return vg_gemm_launch(&p, 1, VG_NN, st);
}
// wgrad problem: dW[N,K] = dY[M,N]^T X[M,K] -> slab (fp32), k-dimension = M rows
static VgGemmProb wg(const bf16* dY, int N, const bf16* X, int K, int M, float* slab, long long split_stride, int splits) {
  VgGemmProb p = mk(dY, N, X, K, N, K, M);
  p.Cf = slab; p.ldcf = K; p.cf_split_stride = split_stride; p.splits = splits;
  return p;
}
static int pick_splits(long long tiles, int Krows, int cap) {
  const int ksteps = (Krows + 63) / 64;
  long long s = (640 + tiles - 1) / tiles;
  if (s > cap) s = cap;
  if (s > ksteps / 4) s = ksteps / 4;
  if (s < 1) s = 1;
  return (int)s;
}
static inline long long tiles128(long long m, long long n) { return ((m + 127) / 128) * ((n + 127) / 128); }
// Blocks whose widths are multiples of 384 run their weight gradients on 128 x 384 tiles, one 8-wave workgroup per CU
// (gemm_tn.hip): as many K slices as keep the grouped launch within one workgroup per CU.
// (tile width 384 when both widths are multiples of 384, else 512 when both are multiples of 512, else 0: tiled kernel)
static inline int wide_bn(int E, int hidden) {
  if (E % 384 == 0 && hidden % 384 == 0) return 384;
  if (E % 512 == 0 && hidden % 512 == 0) return 512;
  return 0;
}
static inline long long tiles_wide(long long m, long long n, int bn) { return ((m + 127) / 128) * (n / bn); }
static int pick_splits384(long long tiles, int Krows, int cap) {
  long long s = 256 / tiles;
  if (s > cap) s = cap;
  if (s > Krows / 256) s = Krows / 256;
  if (s < 1) s = 1;
  return (int)s;
}
// The full-row launch (gemm_row.hip) of both networks: Y or dx [M, N] from A [M, K] and the stage image Wp.  The site fills the other
// operands into `ra`; this adds the dropout mask of `site` - the forward's drop(.) whenever dropout is on, the backward's only where a
// masked copy is asked for - and turns the launcher's answer into a return code (a problem the kernel does not take is an error here).
static int row_launch(VgRowArgs ra, int N, const bf16* A, int K, const bf16* Wp, int M, int epi, const Drop& dr, int site, hipStream_t st) {
  ra.N = N; ra.A = A; ra.lda = K; ra.Wp = Wp; ra.M = M; ra.K = K;
  if (epi == VG_ROW_LNFWD ? dr.on() : ra.dxm != nullptr) ra.drop = dr.at(site);
  const int r = vg_gemm_row_launch(ra, epi, st);
  return r > 0 ? 0 : (r < 0 ? -r : -3);
}
enum { FP_GEMM = 1, FP_NORM = 2, FP_BOTH = 3 };  // a fused-or-pair job in two steps, where other launches sit between the pair's two

// =============================================================================================
//                                   ViT (discriminator)
// =============================================================================================
#define VIT_SPLIT_CAP 16
#define EMB_SPLIT_CAP 32
// Everything a pass derives from (dims, batch), once.
struct VitShape {
  int B, E, H, HE, L, Kc, NP, S, M, MP, Kp, rE;  // S = NP + 1 tokens, M = B S token rows, MP = B NP patch rows, Kp = C P P, rE = R E
  long long ME, MR, BW;  // elements of an [M, E] / [M, rE] tensor; width of a block's bias-gradient row (3E + rE + E)
  float scale;           // attention: 1 / sqrt(HE)
  int rown;              // workgroups (= LayerNorm-backward partial rows) of the full-row GEMMs, which take the block Linears whose output is the
                         // embedding when E = 384 / 512 and the rows come in whole units of 16; 0: the tiled path
  int lnparts, bbparts;  // partial rows of a LayerNorm backward over M rows (either form), and of its double backward
  bool emb_fused;        // the embedding and its backward run as the fused launches of embed.hip where the geometry is theirs (C1-C3)
  long long po_wo, po_w2, po_wqkvT, po_w1T;  // stage images of one block in VitWs::wpack (vit_pack_weights)
};
static VitShape vit_shape(const VgVitDims& d, int B) {
  VitShape s;
  s.B = B; s.E = d.E; s.H = d.H; s.HE = d.E / d.H; s.L = d.L; s.Kc = d.Kc;
  s.NP = (d.IH / d.P) * (d.IH / d.P); s.S = s.NP + 1; s.M = B * s.S; s.MP = B * s.NP; s.Kp = d.C * d.P * d.P; s.rE = d.R * d.E;
  s.ME = (long long)s.M * s.E; s.MR = (long long)s.M * s.rE; s.BW = 3LL * s.E + s.rE + s.E;
  s.scale = 1.0f / sqrtf((float)s.HE); s.emb_fused = vg_embed_fused_ok(d.C, d.IH, d.P, d.E) != 0;
  s.rown = vg_row_width_ok(d.E) ? vg_row_nwg(s.M) : 0;
  s.lnparts = s.rown ? s.rown : vg_ln_bwd_nparts(s.M); s.bbparts = vg_ln_bwd_bwd_nparts(s.M);
  s.po_wo = 0; s.po_w2 = s.po_wo + (long long)s.E * s.E; s.po_wqkvT = s.po_w2 + (long long)s.E * s.rE; s.po_w1T = s.po_wqkvT + 3LL * s.E * s.E;
  return s;
}
// full-row path: pack this call's weights (the backward of this workspace reads the transposed images)
static int vit_pack_weights(const VitShape& sh, const VgVitLayout& lay, const bf16* Pb, bf16* wpack, hipStream_t st) {
  const int E = sh.E, rE = sh.rE;
  VgPackJobs pj; pj.N = E;
  pj.src = Pb + lay.layer0; pj.dst = wpack; pj.src_stride = lay.layer_stride; pj.dst_stride = lay.layer_weights; pj.nblocks = sh.L; pj.n = 4;
  pj.d[0] = {lay.wo, sh.po_wo, E, E, 0};          // out-projection forward: W [E, E], contraction E
  pj.d[1] = {lay.w2, sh.po_w2, rE, rE, 0};        // fc2 forward: W [E, rE], contraction rE
  pj.d[2] = {lay.wqkv, sh.po_wqkvT, 3 * E, E, 1}; // QKV input gradient: W [3E, E] read transposed, contraction 3E
  pj.d[3] = {lay.w1, sh.po_w1T, rE, E, 1};        // fc1 input gradient: W [rE, E] read transposed, contraction rE
  return vg_pack_rows_launch(pj, st);
}

struct VitWs {
  bf16 *Apatch, *X, *xn1, *qkv, *ao, *xmid, *xn2, *a1, *xcls, *hcls, *th;
  unsigned char* z1;  // gelu'(fc1 pre-activation), one byte per element (vg_common.h vg_g8_pack4)
  float *lse, *mean1, *rstd1, *mean2, *rstd2, *meanf, *rstdf;
  // backward scratch, one set per block parity (block l uses set l&1; its LN1 backward writes gin/gm2 of set (l-1)&1):
  // the weight-gradient side of block l still reads set l&1 while the main stream works on block l-1 in the other set
  struct Set { bf16 *gin, *gm2, *gmid, *gm1, *dz1, *dqkv; } set[2];
  float* lnpart;  // [2L] LayerNorm-backward partial-sum blocks, folded by one launch at the end of a backward call
  float* bslab;   // [L][VIT_SPLIT_CAP][3E + rE + E] bias-gradient rows written by the weight-gradient GEMM, one per K slice
  bf16 *dxn, *dao, *gp, *dA, *dzh, *dhcls, *dxcls;
  float *part, *part_cs, *hpart, *tok_sum, *slab;
  bf16* wpack;  // E = 384: stage images of Wo | W2 | Wqkv^T | W1^T per block for the full-row GEMMs (gemm_row.hip)
  // Pruned tail of the TOP block.  The classifier reads the CLS row only (src/v2/modules.py:195), so behind the top block's attention
  // every row-local operator - out-projection, residual, norm2, fc1, GELU, fc2, residual - matters for the B CLS rows alone, and in the
  // backward dL/dX[L] is exactly zero on the other 64/65 of the rows: those operators (and their weight gradients) run on compact
  // [B, .] tensors, forward and backward; the values and gradients the reference defines are unchanged.
  bf16 *t_xmid, *t_xn2, *t_a1, *t_xtop; unsigned char* t_z1; float *t_mean2, *t_rstd2;
  bf16 *t_gb2, *t_dz1, *t_dxn2, *t_dxmid, *t_gb1, *t_dao;
  bf16* t_ao; float* t_lse;  // and its attention for the CLS query only (dot-product scores; the fp8 mode keeps the full kernels)
};
static long long carve_vit(const VitShape& sh, const VgVitLayout& lay, void* base, VitWs& w) {
  const long long B = sh.B, E = sh.E, S = sh.S, M = sh.M, L = sh.L, rE = sh.rE, ME = sh.ME, MR = sh.MR, AK = (long long)sh.MP * sh.Kp;
  Carver c{(unsigned char*)base, 0};
  w.Apatch = c.take<bf16>(AK);
  w.X = c.take<bf16>((L + 1) * ME);
  w.xn1 = c.take<bf16>(L * ME);
  w.qkv = c.take<bf16>(L * ME * 3);
  w.ao = c.take<bf16>(L * ME);
  w.xmid = c.take<bf16>(L * ME);
  w.xn2 = c.take<bf16>(L * ME);
  w.z1 = c.take<unsigned char>(L * MR);
  w.a1 = c.take<bf16>(L * MR);
  w.xcls = c.take<bf16>(B * E); w.hcls = c.take<bf16>(B * E); w.th = c.take<bf16>(B * E);
  w.lse = c.take<float>(L * B * sh.H * S);
  w.mean1 = c.take<float>(L * M); w.rstd1 = c.take<float>(L * M);
  w.mean2 = c.take<float>(L * M); w.rstd2 = c.take<float>(L * M);
  w.meanf = c.take<float>(B); w.rstdf = c.take<float>(B);
  for (int i = 0; i < 2; ++i) {
    VitWs::Set& t = w.set[i];
    t.gin = c.take<bf16>(ME); t.gm2 = c.take<bf16>(ME);   // dL/dX entering the block, and its dropout-masked copy
    t.gmid = c.take<bf16>(ME); t.gm1 = c.take<bf16>(ME);  // same after the MLP half of the block
    t.dz1 = c.take<bf16>(MR);
    t.dqkv = c.take<bf16>(ME * 3);
  }
  w.lnpart = c.take<float>(2 * L * (long long)vg_ln_bwd_nparts(sh.M) * 3 * E);
  w.bslab = c.take<float>(L * (long long)VIT_SPLIT_CAP * sh.BW);
  w.dxn = c.take<bf16>(ME);
  w.dao = c.take<bf16>(ME);
  w.gp = c.take<bf16>(sh.MP * E);
  w.dA = c.take<bf16>(AK);
  w.dzh = c.take<bf16>(B * E); w.dhcls = c.take<bf16>(B * E); w.dxcls = c.take<bf16>(B * E);
  w.part = c.take<float>((long long)vg_ln_bwd_nparts(sh.M) * 3 * E);
  w.part_cs = c.take<float>((long long)vg_colsum_bf16_nparts(sh.M) * 3 * E);
  w.hpart = c.take<float>(sh.Kc <= 16 ? (long long)vg_head_bwd_parts(sh.B) * vg_head_bwd_part_width(sh.E, sh.Kc) : 0);  // classifier head: partial gradient rows
  w.tok_sum = c.take<float>(S * E);
  long long slab = VIT_SPLIT_CAP * lay.layer_weights;
  if (EMB_SPLIT_CAP * E * sh.Kp > slab) slab = EMB_SPLIT_CAP * E * sh.Kp;
  w.slab = c.take<float>(slab);
  w.wpack = c.take<bf16>(sh.rown ? L * lay.layer_weights : 0);
  w.t_xmid = c.take<bf16>(B * E); w.t_xn2 = c.take<bf16>(B * E); w.t_a1 = c.take<bf16>(B * rE); w.t_xtop = c.take<bf16>(B * E);
  w.t_z1 = c.take<unsigned char>(B * rE); w.t_mean2 = c.take<float>(B); w.t_rstd2 = c.take<float>(B);
  w.t_gb2 = c.take<bf16>(B * E); w.t_dz1 = c.take<bf16>(B * rE); w.t_dxn2 = c.take<bf16>(B * E); w.t_dxmid = c.take<bf16>(B * E);
  w.t_gb1 = c.take<bf16>(B * E); w.t_dao = c.take<bf16>(B * E);
  w.t_ao = c.take<bf16>(B * E); w.t_lse = c.take<float>(B * sh.H);
  return c.off;
}
extern "C" long long vg_vit_ws_bytes(const VgVitDims* d, int B) {
  VgVitLayout lay;
  if (!d || B < 1 || vg_vit_layout(d, &lay)) return -1;
  VitWs w;
  return carve_vit(vit_shape(*d, B), lay, nullptr, w);
}

// Byte offsets of the saved activations / gradient scratch inside the workspace (introspection for the parity tests:
// they teacher-force each encoder block with the tensors the kernels really produced).
extern "C" int vg_vit_ws_map(const VgVitDims* d, int B, VgVitWsMap* o) {
  VgVitLayout lay;
  if (!d || !o || B < 1 || vg_vit_layout(d, &lay)) return -1;
  unsigned char* const fake = (unsigned char*)(uintptr_t)(1u << 20);  // never dereferenced
  VitWs w;
  o->total = carve_vit(vit_shape(*d, B), lay, fake, w);
  auto off = [&](const void* p) { return (long long)((const unsigned char*)p - fake); };
  o->X = off(w.X); o->xn1 = off(w.xn1); o->qkv = off(w.qkv); o->ao = off(w.ao); o->xmid = off(w.xmid); o->xn2 = off(w.xn2);
  o->z1 = off(w.z1); o->a1 = off(w.a1); o->lse = off(w.lse);
  o->mean1 = off(w.mean1); o->rstd1 = off(w.rstd1); o->mean2 = off(w.mean2); o->rstd2 = off(w.rstd2);
  for (int i = 0; i < 2; ++i) { o->gin[i] = off(w.set[i].gin); o->gmid[i] = off(w.set[i].gmid); o->dqkv[i] = off(w.set[i].dqkv); o->dz1[i] = off(w.set[i].dz1); }
  o->xtop = off(w.t_xtop); o->dxtop = off(w.dxcls);
  return 0;
}

// Block l as one pass sees it: its parameters, bf16 shadow and gradients (add a per-block offset of VgVitLayout; G is null
// without a gradient buffer), its saved activations, and its slots of the per-block scratch.  The only place that strides by l.
struct VitBlock {
  const float* P; const bf16* Pb; float* G;
  bf16 *x, *xn1, *qkv, *ao, *xmid, *xn2, *a1, *x_next; unsigned char* z1;  // x = X[l], x_next = X[l + 1]
  float *lse, *mean1, *rstd1, *mean2, *rstd2;
  const bf16* wp;        // the block's packed-weight images (full-row path): + VitShape::po_*
  float *part2, *part1;  // LayerNorm-backward partial rows of norm2 / norm1
  float* bslab;          // bias-gradient rows of the block's weight-gradient launch
};
static VitBlock vit_block(const VitWs& w, const VgVitLayout& lay, const VgVitNet* net, const VitShape& sh, int l) {
  const long long lo = lay.layer0 + (long long)l * lay.layer_stride;
  const size_t ME = (size_t)sh.ME, MR = (size_t)sh.MR, M = (size_t)sh.M, part_sz = (size_t)sh.lnparts * 3 * sh.E;
  VitBlock b;
  b.P = net->P + lo; b.Pb = (const bf16*)net->Pb + lo; b.G = net->G ? net->G + lo : nullptr;
  b.x = w.X + l * ME; b.x_next = w.X + (l + 1) * ME; b.xn1 = w.xn1 + l * ME; b.qkv = w.qkv + l * ME * 3; b.ao = w.ao + l * ME;
  b.xmid = w.xmid + l * ME; b.xn2 = w.xn2 + l * ME; b.z1 = w.z1 + l * MR; b.a1 = w.a1 + l * MR; b.lse = w.lse + (size_t)l * sh.B * sh.H * sh.S;
  b.mean1 = w.mean1 + l * M; b.rstd1 = w.rstd1 + l * M; b.mean2 = w.mean2 + l * M; b.rstd2 = w.rstd2 + l * M;
  b.wp = w.wpack + (size_t)l * lay.layer_weights; b.bslab = w.bslab + (size_t)l * VIT_SPLIT_CAP * sh.BW;
  b.part2 = w.lnpart + (size_t)(2 * l) * part_sz; b.part1 = w.lnpart + (size_t)(2 * l + 1) * part_sz;
  return b;
}

// The gradient penalty's own workspace (vg_vit_penalty below): per-block tensors at + l M {rE, E, 3E}
struct PenWs {
  float *xhat, *ones, *logits, *pen_img, *pbb;
  bf16 *h, *gin, *gm2, *da1, *dz1, *dxn2, *gmid, *gm1, *dao, *dqkv, *dxn1, *g0, *g0m, *xcls;
  bf16 *u_dA, *u_x[2], *u_dxn[2], *u_dxn2[2], *u_dqkv, *u_dao[2], *u_gmid, *u_dz1, *u_da1[2], *ucls, *u_gc, *u_gpre, *u_gt;  // [2]: operands of a PAIR of blocks' weight gradients
  bf16 *s_x, *s_qkv, *s_xmid, *s_h, *s_xcls, *tmp;
};
static long long carve_pen(const VgVitDims& d, const VitShape& sh, void* base, PenWs& q) {
  const long long B = sh.B, E = sh.E, L = sh.L, ME = sh.ME, MR = sh.MR;
  Carver c{(unsigned char*)base, 0};
  q.xhat = c.take<float>(B * d.C * d.IH * d.IH);
  q.ones = c.take<float>(B * sh.Kc); q.logits = c.take<float>(B * sh.Kc); q.pen_img = c.take<float>(B);
  q.pbb = c.take<float>((2 * L + 1) * (long long)sh.bbparts * E);
  q.h = c.take<bf16>(L * MR);
  q.gin = c.take<bf16>(L * ME); q.gm2 = c.take<bf16>(L * ME);
  q.da1 = c.take<bf16>(L * MR); q.dz1 = c.take<bf16>(L * MR);
  q.dxn2 = c.take<bf16>(L * ME); q.gmid = c.take<bf16>(L * ME); q.gm1 = c.take<bf16>(L * ME);
  q.dao = c.take<bf16>(L * ME); q.dqkv = c.take<bf16>(L * ME * 3); q.dxn1 = c.take<bf16>(L * ME);
  q.g0 = c.take<bf16>(ME); q.g0m = c.take<bf16>(ME); q.xcls = c.take<bf16>(B * E);
  q.u_dA = c.take<bf16>((long long)sh.MP * sh.Kp);
  q.u_x[0] = c.take<bf16>(ME); q.u_x[1] = c.take<bf16>(ME);
  for (int i = 0; i < 2; ++i) {
    q.u_dxn[i] = c.take<bf16>(ME); q.u_dxn2[i] = c.take<bf16>(ME); q.u_dao[i] = c.take<bf16>(ME); q.u_da1[i] = c.take<bf16>(MR);
  }
  q.u_dqkv = c.take<bf16>(ME * 3); q.u_gmid = c.take<bf16>(ME); q.u_dz1 = c.take<bf16>(MR);
  q.ucls = c.take<bf16>(B * E); q.u_gc = c.take<bf16>(B * E); q.u_gpre = c.take<bf16>(B * E); q.u_gt = c.take<bf16>(B * E);
  q.s_x = c.take<bf16>(L * ME); q.s_qkv = c.take<bf16>(L * ME * 3); q.s_xmid = c.take<bf16>(L * ME); q.s_h = c.take<bf16>(L * MR);
  q.s_xcls = c.take<bf16>(B * E); q.tmp = c.take<bf16>(ME);
  return c.off;
}
// Block l of the penalty's workspace.  h: fc1's pre-activation; gin .. dxn1: the gradients pass 2 keeps; gx / gxm: where pass 2 puts
// dL/dX[l] and its masked copy (block l-1's gin / gm2, or g0 / g0m below block 0); s_*: the gradients pass 4 injects into pass 5.
struct PenBlock {
  bf16 *h, *gin, *gm2, *da1, *dz1, *dxn2, *gmid, *gm1, *dao, *dqkv, *dxn1, *gx, *gxm, *s_x, *s_qkv, *s_xmid, *s_h;
};
static PenBlock pen_block(const PenWs& q, const VitShape& sh, int l) {
  const size_t ME = (size_t)sh.ME, MR = (size_t)sh.MR;
  PenBlock p;
  p.h = q.h + l * MR; p.gin = q.gin + l * ME; p.gm2 = q.gm2 + l * ME; p.da1 = q.da1 + l * MR; p.dz1 = q.dz1 + l * MR;
  p.dxn2 = q.dxn2 + l * ME; p.gmid = q.gmid + l * ME; p.gm1 = q.gm1 + l * ME; p.dao = q.dao + l * ME; p.dqkv = q.dqkv + l * ME * 3;
  p.dxn1 = q.dxn1 + l * ME; p.gx = l > 0 ? q.gin + (l - 1) * ME : q.g0; p.gxm = l > 0 ? q.gm2 + (l - 1) * ME : q.g0m;
  p.s_x = q.s_x + l * ME; p.s_qkv = q.s_qkv + l * ME * 3; p.s_xmid = q.s_xmid + l * ME; p.s_h = q.s_h + l * MR;
  return p;
}
// slot i of the LayerNorm double backward's partial rows: 2l / 2l + 1 = norm1 / norm2 of block l, 2L = the final LayerNorm
static float* pen_part(const PenWs& q, const VitShape& sh, int i) { return q.pbb + (size_t)i * sh.bbparts * sh.E; }

// What the stages of a pass share.  pen: the call is a pass of the gradient penalty - the forward keeps fc1's pre-activation in it
// ([L][M][rE]: the double backward needs gelu'', not the one-byte gelu' code) and the backward is the penalty's SECOND backward.
struct VitPass {
  const VgVitNet* net; VgVitLayout lay; VitShape sh; VitWs w; Drop dr;
  const float* P; const bf16* Pb; float* G;  // net's master parameters, bf16 shadow, gradients (nullable)
  hipStream_t st, sd;   // main stream; stream of the weight-gradient side work (the same without a context)
  VgFoldJobs folds;     // partial-sum folds queued by this call: one launch at its end
  const PenWs* pen; int want_wgrad;
  bool drop, tail, tail_row;  // dropout on; the top block's pruned tail; ... on the full-row kernels
  VitBlock blk(int l) const { return vit_block(w, lay, net, sh, l); }
  int begin(const VgVitNet* net_, int B, void* ws, void* stream, const PenWs* pen_, int want_wgrad_);
  int lin_ln_fwd(bool row, const struct LinLn& j) const, dgrad_ln_bwd(bool row, const struct DgradLn& j, int step = FP_BOTH) const;
  int forward(const void* img, int img_is_bf16, float* logits, float* feats = nullptr), backward(const float* dlogits, void* d_img, int stage_begin, int stage_end);
  int bwd_head(const float* dlogits), bwd_block(int l), bwd_wgrad(int la, int nb), bwd_embed(void* d_img);  // the backward's stages
  int pen_first_backward() const, pen_tangent_backward();                                                // the penalty's passes 2 and 4
};
// after the caller's own argument checks: layout, shape, carve, dropout, streams
int VitPass::begin(const VgVitNet* net_, int B, void* ws, void* stream, const PenWs* pen_, int want_wgrad_) {
  net = net_; pen = pen_; want_wgrad = want_wgrad_; folds.n = 0;
  P = net->P; Pb = (const bf16*)net->Pb; G = net->G;
  VG_TRY(vg_vit_layout(&net->d, &lay));
  sh = vit_shape(net->d, B);
  if (net->attn_fp8 && sh.S > VG_SHORT_MAX_S) return -3;  // the fp8 attention kernels are S <= 80
  carve_vit(sh, lay, ws, w);
  dr = Drop{net->dropout_p, net->dropout_seed, net->dropout_step};  // sites: 0 embedding, 1+2l attention branch, 2+2l MLP branch
  st = (hipStream_t)stream; sd = net->ctx ? ((VgCtx*)net->ctx)->side : st;
  drop = dr.on(); tail = !net->dense_top; tail_row = tail && sh.rown && !net->attn_fp8 && vg_row_nwg(B) > 0;
  return 0;
}

// y = res + drop(A W^T + bias) and yn = LayerNorm(y): ONE full-row launch where `row`, else the Linear and the LayerNorm launch.
// rows > 0: the compact problem of the pruned tail on the B CLS rows - A and res are read through their row strides, the dropout
// bits are those of rows b S of the full tensor.  Yn null: no LayerNorm follows.
struct LinLn {
  const bf16* A; int K; const bf16 *W, *Wp; const float* bias; const bf16* res;
  bf16 *Y, *Yn; float *mean, *rstd; const float *gamma, *beta; int site;
  int rows; long long lda, ldr;  // compact form only; ldr 0 = E
};
int VitPass::lin_ln_fwd(bool row, const LinLn& j) const {
  const int E = sh.E, rows = j.rows ? j.rows : sh.M;
  if (row) {
    VgRowArgs ra = {};
    ra.bias = j.bias; ra.res = j.res; ra.ldr = j.ldr; ra.Y = j.Y; ra.Yn = j.Yn; ra.mean_out = j.mean; ra.rstd_out = j.rstd;
    ra.gamma = j.gamma; ra.beta = j.beta; ra.eps = 1e-5f; ra.drop_row_mul = j.rows ? sh.S : 1;
    return row_launch(ra, E, j.A, j.K, j.Wp, rows, VG_ROW_LNFWD, dr, j.site, st);
  }
  if (j.rows) {
    VgGemmProb p = mk(j.A, (int)j.lda, j.W, j.K, rows, E, j.K);
    p.C = j.Y; p.ldc = E; p.bias = j.bias; p.res = j.res; p.ldr = j.ldr ? (int)j.ldr : E;
    p.drop = dr.at(j.site); p.drop_row_mul = sh.S;
    VG_TRY(vg_gemm_launch(&p, 1, VG_NT, st));
  } else {
    VG_TRY(lin_fwd(j.A, j.K, j.W, j.bias, j.Y, rows, E, VG_ACT_NONE, 0.f, j.res, nullptr, nullptr, st, dr.at(j.site)));
  }
  if (j.Yn) VG_TRY(vg_ln_fwd_launch(j.Y, E, j.gamma, j.beta, j.Yn, E, j.mean, j.rstd, rows, E, 1e-5f, st));
  return 0;
}
// dx = gres (+ inj) + LayerNorm'(dy W) and dxm = dx * mask: ONE full-row launch where `row`, else lin_dgrad into dxn and the
// LayerNorm backward.  inj: the gradient the penalty's double backward injected at the LayerNorm's input - an operand of the full-row
// kernel, added into the penalty's tmp for the pair.  rows > 0: compact problem on the B CLS rows.  keep_dy (the penalty's pass 2):
// dy W itself is kept in dxn by either form, and there are no column sums.  step: FP_GEMM / FP_NORM where the caller has other
// launches between the pair's two (the full-row launch belongs to FP_NORM).
struct DgradLn {
  const bf16* dy; int N; const bf16 *W, *Wp; bf16* dxn;
  const bf16* x; const float *mean, *rstd, *gamma;
  const bf16 *gres, *inj; bf16 *dx, *dxm; float* part; int site;
  int rows; bool keep_dy;
};
int VitPass::dgrad_ln_bwd(bool row, const DgradLn& j, int step) const {
  const int E = sh.E, rows = j.rows ? j.rows : sh.M, drm = j.rows ? sh.S : 1;
  if (row) {
    if (!(step & FP_NORM)) return 0;
    VgRowArgs ra = {};
    ra.x = j.x; ra.mean = j.mean; ra.rstd = j.rstd; ra.gamma = j.gamma; ra.gres = j.gres; ra.dx = j.dx; ra.dxm = j.dxm;
    ra.part = (want_wgrad && !j.keep_dy) ? j.part : nullptr;  // (no parameter gradients wanted: no column sums)
    ra.drop_row_mul = drm; ra.gres2 = j.inj; ra.dy_out = j.keep_dy ? j.dxn : nullptr;
    return row_launch(ra, E, j.dy, j.N, j.Wp, rows, (j.inj || j.keep_dy) ? VG_ROW_LNBWD_PEN : VG_ROW_LNBWD, dr, j.site, st);
  }
  const bf16* gres = j.gres;
  if ((step & FP_NORM) && j.inj) { VG_TRY(vg_add_bf16_launch(j.gres, j.inj, pen->tmp, sh.ME, st)); gres = pen->tmp; }
  if (step & FP_GEMM) VG_TRY(lin_dgrad(j.dy, j.W, j.dxn, rows, j.N, E, 0, nullptr, nullptr, 0.f, st));
  if (step & FP_NORM)
    VG_TRY(vg_ln_bwd_launch(j.dxn, j.x, j.mean, j.rstd, j.gamma, gres, j.dx, j.part, rows, E, j.dxm, dr.at(j.site), st, 1, drm));
  return 0;
}
// K slices per block of a PAIR of blocks' weight gradients: as many as keep the grouped launch at about one workgroup per CU.
// pruned: the pair holds the pruned top block, which contributes its QKV problem only (bwd_wgrad).
static int block_pair_splits(const VitShape& sh, bool pruned) {
  const int E = sh.E, rE = sh.rE;
  if (const int bn = wide_bn(E, rE); bn && sh.M % 32 == 0 && E % 128 == 0 && rE % 128 == 0) {
    const long long qkv = tiles_wide(3 * E, E, bn), all = qkv + tiles_wide(E, E, bn) + tiles_wide(rE, E, bn) + tiles_wide(E, rE, bn);
    return pick_splits384(pruned ? qkv + all : 2 * all, sh.M, VIT_SPLIT_CAP / 2);
  }
  const long long qkv = tiles128(3 * E, E), all = qkv + tiles128(E, E) + tiles128(rE, E) + tiles128(E, rE);
  return pick_splits(pruned ? qkv + all : 2 * all, sh.M, VIT_SPLIT_CAP / 2);
}

int VitPass::forward(const void* img, int img_is_bf16, float* logits, float* feats) {
  const VgVitDims& d = net->d;
  const int B = sh.B, E = sh.E, S = sh.S, M = sh.M, rE = sh.rE;

  // patch embedding (src/v2/modules.py:82-98): gather -> GEMM(+bias +pos, rows remapped past CLS) ; CLS row
  // C1-C3 (E = 384, 4 x 4 patches): ONE launch with block 0's norm1 (embed.hip); every other geometry keeps the launches below
  const VitBlock b0 = blk(0);
  if (sh.emb_fused) {
    VG_TRY(vg_embed_fwd_launch(img, img_is_bf16, Pb + lay.conv_w, P + lay.conv_b, P + lay.pos, P + lay.cls, b0.P + lay.ln1_w, b0.P + lay.ln1_b,
                               w.Apatch, b0.x, b0.xn1, b0.mean1, b0.rstd1, B, d.C, d.IH, 1e-5f, dr.at(0), st));
  } else {
    VG_TRY(vg_patchify_launch(img, img_is_bf16, w.Apatch, B, d.C, d.IH, d.P, st));
    VgGemmProb p = mk(w.Apatch, sh.Kp, Pb + lay.conv_w, sh.Kp, sh.MP, E, sh.Kp);
    p.C = b0.x; p.ldc = E; p.bias = P + lay.conv_b; p.resf = P + lay.pos; p.res_period = sh.NP;
    p.row_in_per = sh.NP; p.row_out_per = S; p.row_out_off = 1;
    p.drop = dr.at(0); p.drop_post = 1;
    VG_TRY(vg_gemm_launch(&p, 1, VG_NT, st));
    VG_TRY(vg_fill_cls_launch(b0.x, P + lay.cls, B, S, E, dr.at(0), st));
  }
  if (sh.rown) VG_TRY(vit_pack_weights(sh, lay, Pb, w.wpack, st));
  if (!sh.emb_fused)  // block 0's norm1; every later one comes with the fc2 of the block below
    VG_TRY(vg_ln_fwd_launch(b0.x, E, b0.P + lay.ln1_w, b0.P + lay.ln1_b, b0.xn1, E, b0.mean1, b0.rstd1, M, E, 1e-5f, st));

  for (int l = 0; l < sh.L; ++l) {
    const VitBlock b = blk(l);
    VG_TRY(lin_fwd(b.xn1, E, b.Pb + lay.wqkv, b.P + lay.bqkv, b.qkv, M, 3 * E, VG_ACT_NONE, 0.f, nullptr, nullptr, nullptr, st));
    const bool pruned = (l == sh.L - 1) && tail;      // top block: behind its attention only the CLS rows matter
    const bool cls_attn = pruned && !net->attn_fp8;   // ... and the CLS query is the only one the classifier sees
    if (cls_attn) VG_TRY(vg_attn_cls_fwd_launch(b.qkv, w.t_ao, w.t_lse, B, sh.H, S, sh.HE, sh.scale, st));
    else VG_TRY(vg_attn_fwd_launch(b.qkv, b.ao, b.lse, B, sh.H, S, sh.HE, sh.scale, net->attn_fp8 ? 2 : 0, st));
    if (pruned) {
      // Top block: only its CLS rows reach the classifier, so everything behind the attention runs on those B rows (compact tensors;
      // A = rows b S of `ao`, residual = rows b S of x by their leading dimension; dropout bits = those of rows b S of the full tensor).
      // Where they take M = B, on the same full-row kernels as the blocks below: out-projection + residual + norm2, then fc2 + residual
      // + the FINAL LayerNorm (its rows are exactly the CLS rows) - the tiled kernel covers so small a problem with 6-12 workgroups whose
      // 12-24 k-steps each wait out a full memory latency (22 us for the fc2 launch), the full-row kernel keeps two stages in flight
      const long long SE = (long long)S * E;
      VG_TRY(lin_ln_fwd(tail_row, {cls_attn ? w.t_ao : b.ao, E, b.Pb + lay.wo, b.wp + sh.po_wo, b.P + lay.bo, b.x, w.t_xmid, w.t_xn2, w.t_mean2,
                                        w.t_rstd2, b.P + lay.ln2_w, b.P + lay.ln2_b, 1 + 2 * l, B, cls_attn ? E : SE, SE}));
      VG_TRY(lin_fwd(w.t_xn2, E, b.Pb + lay.w1, b.P + lay.b1, w.t_a1, B, rE, VG_ACT_GELU, 0.f, nullptr, (bf16*)w.t_z1, nullptr, st, VgDrop(), 2));
      VG_TRY(lin_ln_fwd(tail_row, {w.t_a1, rE, b.Pb + lay.w2, b.wp + sh.po_w2, b.P + lay.b2, w.t_xmid, w.t_xtop, w.hcls, w.meanf, w.rstdf,
                                        P + lay.lnf_w, P + lay.lnf_b, 2 + 2 * l, B, rE, 0}));
      continue;
    }
    // x_mid = x + drop(out_projection(ao)) and norm2(x_mid)
    VG_TRY(lin_ln_fwd(sh.rown, {b.ao, E, b.Pb + lay.wo, b.wp + sh.po_wo, b.P + lay.bo, b.x, b.xmid, b.xn2, b.mean2, b.rstd2, b.P + lay.ln2_w,
                                   b.P + lay.ln2_b, 1 + 2 * l, 0, 0, 0}));
    // z1 keeps gelu'(pre-activation), the only thing the backward needs of it, as one byte per element
    if (pen) VG_TRY(lin_fwd(b.xn2, E, b.Pb + lay.w1, b.P + lay.b1, b.a1, M, rE, VG_ACT_GELU, 0.f, nullptr, pen_block(*pen, sh, l).h, nullptr, st));
    else VG_TRY(lin_fwd(b.xn2, E, b.Pb + lay.w1, b.P + lay.b1, b.a1, M, rE, VG_ACT_GELU, 0.f, nullptr, (bf16*)b.z1, nullptr, st, VgDrop(), 2));
    // X[l+1] = x_mid + drop(fc2(a1)) and the NEXT block's norm1 of it (the last block's output only feeds the CLS rows)
    const bool nx = l + 1 < sh.L;
    const VitBlock nb = nx ? blk(l + 1) : VitBlock{};
    VG_TRY(lin_ln_fwd(sh.rown, {b.a1, rE, b.Pb + lay.w2, b.wp + sh.po_w2, b.P + lay.b2, b.xmid, b.x_next, nb.xn1, nb.mean1, nb.rstd1,
                                   nx ? nb.P + lay.ln1_w : nullptr, nx ? nb.P + lay.ln1_b : nullptr, 2 + 2 * l, 0, 0, 0}));
  }
  // final LayerNorm: acts on every row in the reference (:236), only the CLS rows feed the classifier (:195); the pruned tail had it behind its fc2
  if (!tail) VG_TRY(vg_ln_fwd_launch(blk(sh.L - 1).x_next, (long long)S * E, P + lay.lnf_w, P + lay.lnf_b, w.hcls, E, w.meanf, w.rstdf, B, E, 1e-5f, st));
  VG_TRY(lin_fwd(w.hcls, E, Pb + lay.hw1, P + lay.hb1, w.th, B, E, VG_ACT_TANH, 0.f, nullptr, nullptr, nullptr, st));
  VG_TRY(vg_head_fc2_launch(w.th, P + lay.hw2, P + lay.hb2, logits, B, E, sh.Kc, st));
  // vg_vit_features: what the classifier's fc1 just read, norm(x)[:, 0, :], widened to fp32 (metrics.hip) - behind the head, so the
  // launches that make the logits are those of vg_vit_forward, in its order
  if (feats) VG_TRY(vg_widen_bf16_f32_launch(w.hcls, feats, (long long)B * E, st));
  return 0;
}
extern "C" int vg_vit_forward(const VgVitNet* net, int B, const void* img, int img_is_bf16, void* ws, float* logits,
                              void* stream) {
  if (!net || !img || !ws || !logits || B < 1) return -1;
  VitPass c;
  VG_TRY(c.begin(net, B, ws, stream, nullptr, 0));
  return c.forward(img, img_is_bf16, logits);
}
extern "C" int vg_vit_features(const VgVitNet* net, int B, const void* img, int img_is_bf16, void* ws, float* logits, float* feats,
                               void* stream) {
  if (!net || !img || !ws || !logits || !feats || B < 1) return -1;
  VitPass c;
  VG_TRY(c.begin(net, B, ws, stream, nullptr, 0));
  return c.forward(img, img_is_bf16, logits, feats);
}

// Backward stages: 0 = classifier head + final LN, 1..L = encoder blocks L-1 .. 0, L+1 = patch embedding.
// Running [stage_begin, stage_end) lets the caller all-reduce the gradients of finished blocks (a contiguous
// range of the flat buffer) on another stream while the remaining stages still compute.
// The gradient penalty's SECOND backward (vg_vit_penalty below; VitPass::pen) is this backward with gradients injected at the
// activations the double backward reaches: dL/d(fc1 pre-activation), dL/d(qkv), dL/d(x_mid), dL/d(X[l]) per block (PenBlock::s_*; the
// residual-stream ones go through PenWs::tmp where they are an operand of other launches too), dL/dX[L] on the CLS rows (s_xcls), and
// dL/d(classifier fc1 pre-activation), which w.dzh already holds, in place of the logits' gradient: no logits' backward, no fc2
// gradients.  gelu' is computed from the pre-activation the forward kept.

// ---- stage 0: classifier head + final LN (CLS rows only) ----
int VitPass::bwd_head(const float* dlogits) {
  const int B = sh.B, E = sh.E, S = sh.S, Kc = sh.Kc, top = sh.L - 1;
  // dz, and the gradients of fc2 and of fc1's bias as partial rows for the fold at the end of this call: one launch
  const int head1 = pen ? 0 :
                    vg_head_bwd_launch(dlogits, P + lay.hw2, w.th, w.dzh, want_wgrad ? G + lay.hw2 : nullptr, want_wgrad ? G + lay.hb2 : nullptr,
                                       B, E, Kc, want_wgrad, st, (want_wgrad && Kc <= 16) ? w.hpart : nullptr);
  if (head1 < 0) return -head1;
  if (want_wgrad) {
    if (head1) VG_TRY(vg_fold_push(folds, w.hpart, vg_head_bwd_parts(B), vg_head_bwd_part_width(E, Kc), G + lay.hw2, Kc * E, G + lay.hb1, E,
                                   G + lay.hb2, Kc, nullptr, 0));
    else VG_TRY(vg_colsum_bf16_launch(w.dzh, E, B, E, w.part_cs, G + lay.hb1, 1, st));
    // (a few K slices: with one, the three 128 x 384 tiles of this 384 x 384 x B problem are three workgroups walking 16 stages - 18 us at B = 512)
    VgGemmProb p = wg(w.dzh, E, w.hcls, E, B, w.slab, (long long)E * E, B >= 512 ? 4 : (B >= 256 ? 2 : 1));
    VG_TRY(vg_gemm_launch(&p, 1, VG_TN, st));
    VG_TRY(vg_slab_reduce_launch(w.slab, (long long)E * E, p.splits, G + lay.hw1, (long long)E * E, 1, st));
  }
  VG_TRY(lin_dgrad(w.dzh, Pb + lay.hw1, w.dhcls, B, E, E, 0, nullptr, nullptr, 0.f, st));
  if (tail) {
    // dL/dX[L] on the CLS rows (it is zero elsewhere) and its masked copy for the top block's MLP dropout - the bits of rows b S of the full tensor
    VG_TRY(vg_ln_bwd_launch(w.dhcls, w.t_xtop, w.meanf, w.rstdf, P + lay.lnf_w, nullptr, w.dxcls, w.part, B, E, drop ? w.t_gb2 : nullptr,
                            dr.at(2 + 2 * top), st, 1, S));
  } else {
    const VitWs::Set& ts = w.set[top & 1];
    VG_TRY(vg_ln_bwd_launch(w.dhcls, blk(top).x_next, w.meanf, w.rstdf, P + lay.lnf_w, nullptr, w.dxcls, w.part, B, E, nullptr, VgDrop(), st, S));
    if (pen) VG_TRY(vg_add_bf16_launch(w.dxcls, pen->s_xcls, w.dxcls, (long long)B * E, st));
    // dL/dX[L]: the CLS rows, zero elsewhere - and its masked copy for the last block's MLP dropout, in the same launch
    VG_TRY(vg_scatter_cls_launch(w.dxcls, ts.gin, B, S, E, st, drop ? ts.gm2 : nullptr, dr.at(2 + 2 * top)));
  }
  if (want_wgrad)  // (the final LayerNorm's own partial count: B rows, standalone kernel; w.part is nobody else's)
    VG_TRY(vg_fold_push(folds, w.part, vg_ln_bwd_nparts(B), 3 * E, G + lay.lnf_w, E, G + lay.lnf_b, E, nullptr, E, nullptr, 0));
  return 0;
}

// ---- one block's input-gradient chain (main stream) from dL/dX[l+1] in set l&1 down to dL/d(qkv); the norm1 backward follows in the stage loop ----
int VitPass::bwd_block(int l) {
  const int B = sh.B, E = sh.E, S = sh.S, M = sh.M, rE = sh.rE;
  const bool pruned = tail && l == sh.L - 1;
  const VitBlock b = blk(l); const VitWs::Set& cur = w.set[l & 1];
  if (pruned) {
    // Top block, pruned tail: dL/dX[L] lives on the B CLS rows only (w.dxcls; masked copy w.t_gb2), so the MLP half and the
    // out-projection run on compact [B, .] tensors; their results go back into zero-filled full-size tensors where the
    // attention backward (d ao) and the QKV input gradient's residual operand (d x_mid) need every row.
    const bf16* gb2c = drop ? w.t_gb2 : w.dxcls;
    VG_TRY(lin_dgrad(gb2c, b.Pb + lay.w2, w.t_dz1, B, E, rE, VG_ACT_MUL_Z8, (const bf16*)w.t_z1, nullptr, 0.f, st));
    // fc1 input gradient + norm2 backward, M = B (the forward's twin: see there)
    VG_TRY(dgrad_ln_bwd(tail_row, {w.t_dz1, rE, b.Pb + lay.w1, b.wp + sh.po_w1T, w.t_dxn2, w.t_xmid, w.t_mean2, w.t_rstd2, b.P + lay.ln2_w,
                                        w.dxcls, nullptr, w.t_dxmid, drop ? w.t_gb1 : nullptr, b.part2, 1 + 2 * l, B, false}));
    const bf16* gb1c = drop ? w.t_gb1 : w.t_dxmid;
    VG_TRY(lin_dgrad(gb1c, b.Pb + lay.wo, w.t_dao, B, E, E, 0, nullptr, nullptr, 0.f, st));
    if (!net->attn_fp8) VG_TRY(vg_scatter_cls_launch(w.t_dxmid, cur.gmid, B, S, E, st));  // (d ao stays compact: the CLS-query attention backward below)
    else VG_TRY(vg_scatter_cls2_launch(w.t_dao, w.dao, w.t_dxmid, cur.gmid, B, S, E, st));
  } else {
    const PenBlock pb = pen ? pen_block(*pen, sh, l) : PenBlock{};
    const bf16* gb2 = drop ? cur.gm2 : cur.gin;  // gradient w.r.t. the fc2 output (before dropout2)
    // d a1 = gb2 W2 ; dz1 = d a1 * gelu'(pre-activation), stored by the forward   (fused epilogue)
    if (pen) VG_TRY(lin_dgrad(gb2, b.Pb + lay.w2, cur.dz1, M, E, rE, VG_ACT_MUL_GELU_GRAD, pb.h, nullptr, 0.f, st));
    else VG_TRY(lin_dgrad(gb2, b.Pb + lay.w2, cur.dz1, M, E, rE, VG_ACT_MUL_Z8, (const bf16*)b.z1, nullptr, 0.f, st));
    if (pen) VG_TRY(vg_add_bf16_launch(cur.dz1, pb.s_h, cur.dz1, sh.MR, st));
    // fc1 input gradient + norm2 backward + the residual-stream gradient
    VG_TRY(dgrad_ln_bwd(sh.rown, {cur.dz1, rE, b.Pb + lay.w1, b.wp + sh.po_w1T, w.dxn, b.xmid, b.mean2, b.rstd2, b.P + lay.ln2_w, cur.gin, pb.s_xmid,
                                     cur.gmid, drop ? cur.gm1 : nullptr, b.part2, 1 + 2 * l, 0, false}));
    const bf16* gb1 = drop ? cur.gm1 : cur.gmid;  // gradient w.r.t. the out-projection output (before dropout1)
    VG_TRY(lin_dgrad(gb1, b.Pb + lay.wo, w.dao, M, E, E, 0, nullptr, nullptr, 0.f, st));
  }
  if (pruned && !net->attn_fp8)
    VG_TRY(vg_attn_cls_bwd_launch(b.qkv, w.t_ao, w.t_dao, w.t_lse, cur.dqkv, B, sh.H, S, sh.HE, sh.scale, st));
  else
    VG_TRY(vg_attn_bwd_launch(b.qkv, b.ao, w.dao, b.lse, cur.dqkv, B, sh.H, S, sh.HE, sh.scale, net->attn_fp8 ? 2 : 0, st));
  if (pen) VG_TRY(vg_add_bf16_launch(cur.dqkv, pen_block(*pen, sh, l).s_qkv, cur.dqkv, sh.ME * 3, st));
  return 0;
}

// ---- weight gradients of blocks la, la-1, .. (nb = 1 or 2): grouped launch + slab folds + bias partials, on the side stream ----
// The blocks of a single-stream call are taken in PAIRS - the eight problems of two blocks as ONE grouped split-K launch with half
// the K slices (same number of workgroups: 42 tiles x 6 instead of 21 x 12), which halves the fp32 slab traffic (85 -> 42 MB written
// and folded per block) and the prologues / epilogues per unit of work.
int VitPass::bwd_wgrad(int la, int nb) {
  const int B = sh.B, E = sh.E, S = sh.S, M = sh.M, rE = sh.rE, top = sh.L - 1;
  const long long BW = sh.BW;
  // the slab and bslab carves hold VIT_SPLIT_CAP slices in all: never more (round 1 overran them from an environment knob)
  // The K partition is that of a PAIR also for a block that goes alone (the odd one out, the side-stream schedule): every
  // schedule then adds the same slices in the same order, and staged, one-shot and side-stream backward agree bit for bit.
  int splits = block_pair_splits(sh, false);
#ifdef VG_TUNING  // experimental builds only (make var): the product library reads no environment
  static const int split_env = getenv("VG_VIT_SPLITS") ? atoi(getenv("VG_VIT_SPLITS")) : 0;
  if (split_env > 0 && split_env <= VIT_SPLIT_CAP / 2) splits = split_env;
#endif
  // K slices per BLOCK, the same in every schedule (so every schedule adds the same slices in the same order).  With the pruned tail the
  // top block contributes its QKV problem only: the launch that holds it and the block below is 33 tiles instead of 48, and at 5 slices
  // 165 workgroups on 256 CUs - those two blocks therefore take 7 slices (231 workgroups; 149 -> ~110 us), wherever they are launched.
  const int splits_top = (tail && top >= 1) ? block_pair_splits(sh, true) : splits;
  auto splits_of = [&](int lb) { return (tail && top >= 1 && (lb == top || lb == top - 1)) ? splits_top : splits; };
  VgGemmProb pr[8];
  int np = 0, first[2] = {0, 0};
  long long slab_off[2] = {0, 0};
  for (int j = 0; j < nb; ++j) {
    const int lb = la - j, sp = splits_of(lb);
    if (j + 1 < nb) slab_off[j + 1] = slab_off[j] + (long long)sp * lay.layer_weights;
    const VitBlock bb = blk(lb);
    const VitWs::Set& sb = w.set[lb & 1];
    float* slab = w.slab + slab_off[j];
    const bf16* gb1b = drop ? sb.gm1 : sb.gmid;
    const bf16* gb2b = drop ? sb.gm2 : sb.gin;
    // bias gradients = column sums of the same dY operands: they ride along in the GEMM (ones x A on the MFMA pipe),
    // one row per K slice, folded with the LayerNorm partials at the end.  fc2's bias: only the top block needs it
    // here (lower blocks get it from the LN1 partials of the block above).
    float* const bs = bb.bslab;
    VgGemmProb* q = pr + np;
    first[j] = np;
    q[0] = wg(sb.dqkv, 3 * E, bb.xn1, E, M, slab + lay.wqkv, lay.layer_weights, sp);
    q[0].colsum = bs; q[0].colsum_split_stride = BW;
    if (tail && lb == top) { np += 1; continue; }  // top block: the other three are sums over its B CLS rows (below)
    q[1] = wg(gb1b, E, bb.ao, E, M, slab + lay.wo, lay.layer_weights, sp);
    q[2] = wg(sb.dz1, rE, bb.xn2, E, M, slab + lay.w1, lay.layer_weights, sp);
    q[3] = wg(gb2b, E, bb.a1, rE, M, slab + lay.w2, lay.layer_weights, sp);
    q[2].colsum = bs + 3 * E; q[2].colsum_split_stride = BW;
    if (lb == top) { q[3].colsum = bs + 3 * E + rE; q[3].colsum_split_stride = BW; }  // (dense top block: fc2's bias rides along here)
    np += 4;
  }
  VG_TRY(vg_gemm_launch(pr, np, VG_TN, sd));
  const bool ptop = tail && la == top;  // this launch holds the pruned top block: its slab has the QKV part only
  if (nb == 2 && !ptop && pr[first[0]].splits == pr[first[1]].splits)  // both blocks' K slices in one launch
    VG_TRY(vg_slab_reduce2_launch(w.slab, w.slab + slab_off[1], lay.layer_weights, pr[first[0]].splits, blk(la).G, blk(la - 1).G,
                                  lay.layer_weights, 1, sd));
  for (int j = 0; j < nb; ++j) {
    const int lb = la - j;
    const VitBlock bb = blk(lb);
    float* bs = bb.bslab;
    const int ns = pr[first[j]].splits;  // (the launcher drops empty slices; every problem of a block has the same M rows)
    const bool pt = tail && lb == top;
    if (nb == 1 || ptop || pr[first[0]].splits != pr[first[nb - 1]].splits)  // (the pruned top block's slab holds its QKV part only: wqkv is the first region of a layer)
      VG_TRY(vg_slab_reduce_launch(w.slab + slab_off[j], lay.layer_weights, ns, bb.G, pt ? 3LL * E * E : lay.layer_weights, 1, sd));
    VG_TRY(vg_fold_push(folds, bs, ns, (int)BW, bb.G + lay.bqkv, 3 * E, pt ? nullptr : bb.G + lay.b1, rE, (lb == top && !pt) ? bb.G + lay.b2 : nullptr, E,
                        nullptr, 0));
    if (!pt) continue;
    // ---- top block: out-projection / fc1 / fc2 weight gradients as sums over the B CLS rows (every other row of their dY is exactly
    // zero), ONE K slice accumulated straight into the gradient buffer; b1 / b2 ride along as one partial row ----
    const bf16* gb1c = drop ? w.t_gb1 : w.t_dxmid;
    const bf16* gb2c = drop ? w.t_gb2 : w.dxcls;
    float* bsc = bs + (size_t)(VIT_SPLIT_CAP - 1) * BW;  // the last row of the block's carve: a block never has more than VIT_SPLIT_CAP / 2 slices
    VgGemmProb t[3];
    if (!net->attn_fp8) t[0] = wg(gb1c, E, w.t_ao, E, B, bb.G + lay.wo, 0, 1);  // the CLS query's attention output
    else { t[0] = wg(gb1c, E, bb.ao, E, B, bb.G + lay.wo, 0, 1); t[0].ldb = S * E; }  // rows b S of the full one
    t[1] = wg(w.t_dz1, rE, w.t_xn2, E, B, bb.G + lay.w1, 0, 1);
    t[2] = wg(gb2c, E, w.t_a1, rE, B, bb.G + lay.w2, 0, 1);
    for (int i = 0; i < 3; ++i) t[i].cf_accumulate = 1;
    t[1].colsum = bsc + 3 * E; t[1].colsum_split_stride = BW;
    t[2].colsum = bsc + 3 * E + rE; t[2].colsum_split_stride = BW;
    VG_TRY(vg_gemm_launch(t, 3, VG_TN, sd));
    VG_TRY(vg_fold_push(folds, bsc, 1, (int)BW, nullptr, 3 * E, bb.G + lay.b1, rE, bb.G + lay.b2, E, nullptr, 0));
  }
  return 0;
}

// ---- stage L+1: patch embedding ----
int VitPass::bwd_embed(void* d_img) {
  const VgVitDims& d = net->d;
  const int B = sh.B, E = sh.E, S = sh.S, Kp = sh.Kp;
  // dL/dX[0]: block 0 (set 0) wrote it into the other set - with dropout, the copy masked by the embedding dropout (second output of
  // block 0's LN1 backward)
  const bf16* g = drop ? w.set[1].gm2 : w.set[1].gin;
  const int splits = pick_splits(tiles128(E, Kp), sh.MP, EMB_SPLIT_CAP);
  if (sh.emb_fused) {  // C1-C3: dL/dX[0] read in place, one launch per side + one fold (embed.hip); the K slices of the launches below
    if (want_wgrad)
      VG_TRY(vg_embed_wgrad_launch(g, w.Apatch, w.slab, w.tok_sum, G + lay.conv_w, G + lay.conv_b, G + lay.pos, G + lay.cls, B, d.C, d.IH, splits, st));
    if (d_img) VG_TRY(vg_embed_dimg_launch(g, Pb + lay.conv_w, (bf16*)d_img, B, d.C, d.IH, st));
    return 0;
  }
  if (want_wgrad) {
    VG_TRY(vg_batch_sum_launch(g, w.tok_sum, B, S, E, st));
    VG_TRY(vg_embed_small_grads_launch(w.tok_sum, G + lay.cls, G + lay.pos, G + lay.conv_b, S, E, st));
  }
  if (want_wgrad || d_img) VG_TRY(vg_take_rows_launch(g, w.gp, B, S, 1, sh.NP, E, st));
  if (want_wgrad) {
    VgGemmProb p = wg(w.gp, E, w.Apatch, Kp, sh.MP, w.slab, (long long)E * Kp, splits);
    VG_TRY(vg_gemm_launch(&p, 1, VG_TN, st));
    VG_TRY(vg_slab_reduce_launch(w.slab, (long long)E * Kp, p.splits, G + lay.conv_w, (long long)E * Kp, 1, st));
  }
  if (d_img) {
    VG_TRY(lin_dgrad(w.gp, Pb + lay.conv_w, w.dA, sh.MP, E, Kp, 0, nullptr, nullptr, 0.f, st));
    VG_TRY(vg_unpatchify_launch(w.dA, (bf16*)d_img, B, d.C, d.IH, d.P, st));
  }
  return 0;
}

int VitPass::backward(const float* dlogits, void* d_img, int stage_begin, int stage_end) {
  VgCtx* ctx = (VgCtx*)net->ctx;
  const int B = sh.B, E = sh.E, L = sh.L, top = L - 1;
  if (stage_begin == 0) VG_TRY(bwd_head(dlogits));

  int last_side = -1;  // highest-index side event recorded by this call (for the join)
  // Weight gradients, single-stream schedule: the blocks of this call go in pairs (bwd_wgrad).  The launch sits in the SECOND
  // block of the pair, in front of its last kernel (QKV input gradient + norm1 backward): that kernel writes dL/dX into the other
  // scratch set, where the first block's fc2-gradient operand still lives.
  const int l_hi = L - (stage_begin > 1 ? stage_begin : 1), l_lo = L - ((stage_end < L + 1 ? stage_end : L + 1) - 1);
  const bool pairing = !ctx && want_wgrad;
  for (int l = L - 1; l >= 0; --l) {
    const int stage = L - l;
    if (stage < stage_begin) continue;
    if (stage >= stage_end) break;
    const VitBlock b = blk(l);
    // ---------------- input-gradient chain (main stream) ----------------
    VG_TRY(bwd_block(l));
    // QKV input gradient + norm1 backward: dL/dX[l], and its masked copy for the dropout it meets next, go into the OTHER set
    const VitWs::Set &cur = w.set[l & 1], &nxt = w.set[(l & 1) ^ 1];
    const DgradLn n1 = {cur.dqkv, 3 * E, b.Pb + lay.wqkv, b.wp + sh.po_wqkvT, w.dxn, b.x, b.mean1, b.rstd1, b.P + lay.ln1_w, cur.gmid,
                        pen ? pen_block(*pen, sh, l).s_x : nullptr, nxt.gin, drop ? nxt.gm2 : nullptr, b.part1, l > 0 ? 2 + 2 * (l - 1) : 0, 0, false};
    VG_TRY(dgrad_ln_bwd(sh.rown, n1, FP_GEMM));  // (the pair's GEMM goes in front of the weight gradients, the full-row launch behind them)
    if (pairing) {  // second block of a pair (or the odd one out at the end of this call): its and its partner's weight gradients
      const int idx = l_hi - l;
      if (idx & 1) VG_TRY(bwd_wgrad(l + 1, 2));
      else if (l == l_lo) VG_TRY(bwd_wgrad(l, 1));
    }
    // the OTHER set is what the weight-gradient side of block l+1 may still be reading: wait for it first
    if (ctx && want_wgrad && l + 1 <= top && l + 1 >= 0 && (L - (l + 1)) >= stage_begin)
      VG_CHECK_HIP(hipStreamWaitEvent(st, ctx->ev_side[l + 1], 0));
    VG_TRY(dgrad_ln_bwd(sh.rown, n1, FP_NORM));
    if (!want_wgrad) continue;
    // ---------------- weight-gradient side (second stream when a context is given) ----------------
    if (ctx) {
      VG_CHECK_HIP(hipEventRecord(ctx->ev_main[l], st));
      VG_CHECK_HIP(hipStreamWaitEvent(sd, ctx->ev_main[l], 0));
    }
    const int parts2 = (l == top && tail) ? (tail_row ? vg_row_nwg(B) : vg_ln_bwd_nparts(B)) : sh.lnparts;
    VG_TRY(vg_fold_push(folds, b.part2, parts2, 3 * E, b.G + lay.ln2_w, E, b.G + lay.ln2_b, E, b.G + lay.bo, E, nullptr, 0));
    if (!pairing) VG_TRY(bwd_wgrad(l, 1));  // side-stream schedule: block by block, behind the block's input-gradient chain
    // (fc2's bias of the block below: the column sums of dL/dX[l])
    VG_TRY(vg_fold_push(folds, b.part1, sh.lnparts, 3 * E, b.G + lay.ln1_w, E, b.G + lay.ln1_b, E, l > 0 ? blk(l - 1).G + lay.b2 : nullptr, E, nullptr, 0));
    if (ctx) { VG_CHECK_HIP(hipEventRecord(ctx->ev_side[l], sd)); last_side = l; }
  }
  // all LayerNorm partial sums of this call in one launch (behind the last block's side work)
  if (folds.n > 0) {
    // the partial rows come from kernels of the MAIN stream (head, final LayerNorm, the LayerNorm backwards): a call that runs no
    // encoder block (stage range [0, 1)) has recorded no main-stream event the side stream waits for - without this one the fold
    // raced the final LayerNorm's backward (seen at E = 768: d gamma / d beta of vit.norm zero or partial, run to run)
    if (ctx) { VG_CHECK_HIP(hipEventRecord(ctx->ev_main[VG_CTX_EVENTS - 1], st)); VG_CHECK_HIP(hipStreamWaitEvent(sd, ctx->ev_main[VG_CTX_EVENTS - 1], 0)); }
    VG_TRY(vg_colsum_f32_multi_launch(folds, sd));
    if (ctx) { VG_CHECK_HIP(hipEventRecord(ctx->ev_side[VG_CTX_EVENTS - 1], sd)); VG_CHECK_HIP(hipStreamWaitEvent(st, ctx->ev_side[VG_CTX_EVENTS - 1], 0)); }
  }
  // join: everything this call put on the side stream is ordered before whatever follows on the main stream
  if (ctx && last_side >= 0) VG_CHECK_HIP(hipStreamWaitEvent(st, ctx->ev_side[last_side], 0));
  if (stage_end < L + 2) return 0;
  return bwd_embed(d_img);
}

extern "C" int vg_vit_backward_stages(const VgVitNet* net, int B, void* ws, const float* dlogits, void* d_img, int want_wgrad,
                                      int stage_begin, int stage_end, void* stream) {
  if (!net || !ws || !dlogits || B < 1) return -1;
  if (stage_begin < 0 || stage_end > net->d.L + 2 || stage_begin >= stage_end) return -2;
  if (want_wgrad && !net->G) return -1;
  VitPass c;
  VG_TRY(c.begin(net, B, ws, stream, nullptr, want_wgrad));
  return c.backward(dlogits, d_img, stage_begin, stage_end);
}
extern "C" int vg_vit_backward(const VgVitNet* net, int B, void* ws, const float* dlogits, void* d_img, int want_wgrad,
                               void* stream) {
  if (!net) return -1;
  return vg_vit_backward_stages(net, B, ws, dlogits, d_img, want_wgrad, 0, net->d.L + 2, stream);
}

// =============================================================================================
//            gradient penalty (src/v2/utils.py:124-144, training.py:101-106) as ONE call
// =============================================================================================
// G += weight * d/d theta mean_b (|| d sum(D(x^)) / d x^ ||_2 - 1)^2 at x^ = eps real + (1 - eps) fake: five passes on one stream.
//   1. forward of x^ (every row of the top block; fc1's pre-activation kept - gelu'' needs it);
//   2. first backward, input gradient only, UNFUSED and with every intermediate gradient kept per block: they are the "dY operands"
//      of the second-order operators;
//   3. n_b = ||g_b||, the penalty, and u = d(weight * penalty) / d g;
//   4. the backward of pass 2 (the direction u travels UP the network: it is the forward-mode tangent of pass 1): per block the
//      LayerNorm / attention / GELU second-order kernels (second_order.hip, attention.hip), the Linear layers as forward GEMMs
//      (d(dY) = ddX W^T) and weight gradients dW += dY^T ddX (one grouped launch per block); each second-order kernel also yields a
//      gradient with respect to a forward activation (X[l], qkv, x_mid, the fc1 pre-activation) that
//   5. the ordinary fused backward of pass 1 picks up where it reaches that activation (VitPass::pen) - with nothing arriving from the logits.
// The operator arithmetic is that of vit-gan_amd/ops2.py (the autograd form this replaces, kept as the reference the tests compare
// with); dropout draws the engine's counter-based masks of net->dropout_seed, the same in all five passes.
//
// Every network the plain step trains in bf16 (E a multiple of 128: the alignment of the elementwise kernels follows); where the full-row
// kernels take the shape (E = 384 / 512, rows in whole units of 16) the input gradients and LayerNorm backwards of passes 2 and 5 are fused,
// elsewhere they are the GEMM + LayerNorm pairs.  -3: fp8 attention (the second-order attention kernel differentiates the bf16 one), or
// more than 80 tokens (the second-order attention kernel is S <= 80).
static int pen_shape_ok(const VgVitNet* net, const VitShape& sh) {
  const VgVitDims& d = net->d;
  return !net->attn_fp8 && sh.S <= VG_SHORT_MAX_S && ((long long)sh.B * sh.E) % 8 == 0 && ((long long)d.C * d.IH * d.IH) % 4 == 0 && sh.Kp % 4 == 0;
}
extern "C" long long vg_vit_penalty_ws_bytes(const VgVitDims* d, int B) {
  VgVitLayout lay;
  if (!d || B < 1 || vg_vit_layout(d, &lay)) return -1;
  PenWs q;
  return carve_pen(*d, vit_shape(*d, B), nullptr, q);
}

// ---- 2. first backward: d sum(logits) / d x^, every intermediate kept ----
int VitPass::pen_first_backward() const {
  const PenWs& q = *pen;
  const int B = sh.B, E = sh.E, S = sh.S, M = sh.M, rE = sh.rE, top = sh.L - 1;
  VG_TRY(vg_fill_f32_launch(q.ones, (long long)B * sh.Kc, 1.0f, st));
  { const int r = vg_head_bwd_launch(q.ones, P + lay.hw2, w.th, w.dzh, nullptr, nullptr, B, E, sh.Kc, 0, st); if (r < 0) return -r; }  // g_pre
  VG_TRY(lin_dgrad(w.dzh, Pb + lay.hw1, w.dhcls, B, E, E, 0, nullptr, nullptr, 0.f, st));                                             // g_c
  VG_TRY(vg_ln_bwd_launch(w.dhcls, blk(top).x_next, w.meanf, w.rstdf, P + lay.lnf_w, nullptr, w.dxcls, w.part, B, E, nullptr, VgDrop(), st, S));
  const PenBlock pt = pen_block(q, sh, top);
  VG_TRY(vg_scatter_cls_launch(w.dxcls, pt.gin, B, S, E, st, drop ? pt.gm2 : nullptr, dr.at(2 + 2 * top)));
  for (int l = top; l >= 0; --l) {
    const VitBlock b = blk(l);
    const PenBlock p = pen_block(q, sh, l);
    const bf16* gb2 = drop ? p.gm2 : p.gin;
    VG_TRY(lin_dgrad(gb2, b.Pb + lay.w2, p.da1, M, E, rE, 0, nullptr, nullptr, 0.f, st));
    VG_TRY(vg_act2_launch(p.h, p.da1, nullptr, p.dz1, nullptr, sh.MR, 1, 1, st));
    // fc1 input gradient + norm2 backward; the full-row kernel here also WRITES the GEMM result (the double backward's d xn2)
    VG_TRY(dgrad_ln_bwd(sh.rown, {p.dz1, rE, b.Pb + lay.w1, b.wp + sh.po_w1T, p.dxn2, b.xmid, b.mean2, b.rstd2, b.P + lay.ln2_w, p.gin, nullptr,
                                     p.gmid, drop ? p.gm1 : nullptr, w.part, 1 + 2 * l, 0, true}));
    VG_TRY(lin_dgrad(drop ? p.gm1 : p.gmid, b.Pb + lay.wo, p.dao, M, E, E, 0, nullptr, nullptr, 0.f, st));
    VG_TRY(vg_attn_bwd_launch(b.qkv, b.ao, p.dao, b.lse, p.dqkv, B, sh.H, S, sh.HE, sh.scale, 0, st));
    VG_TRY(dgrad_ln_bwd(sh.rown, {p.dqkv, 3 * E, b.Pb + lay.wqkv, b.wp + sh.po_wqkvT, p.dxn1, b.x, b.mean1, b.rstd1, b.P + lay.ln1_w, p.gmid, nullptr,
                                     p.gx, drop ? p.gxm : nullptr, w.part, l > 0 ? 2 + 2 * (l - 1) : 0, 0, true}));
  }
  VG_TRY(vg_take_rows_launch(drop ? q.g0m : q.g0, w.gp, B, S, 1, sh.NP, E, st));
  return lin_dgrad(w.gp, Pb + lay.conv_w, w.dA, sh.MP, E, sh.Kp, 0, nullptr, nullptr, 0.f, st);  // = the image gradient, patch by patch
}

// ---- 4. backward of pass 2, bottom to top ----
int VitPass::pen_tangent_backward() {
  const PenWs& q = *pen;
  const int B = sh.B, E = sh.E, S = sh.S, M = sh.M, rE = sh.rE, L = sh.L, Kp = sh.Kp;
  {  // patch embedding: d A = gp Wc  ->  u_gp = u_dA Wc^T (rows back behind the CLS rows, embedding dropout's mask), dWc += gp^T u_dA
    VG_TRY(vg_fill_f32_launch((float*)q.u_x[0], sh.ME / 2, 0.0f, st));  // (a kernel, not hipMemsetAsync: see DESIGN 7 - the memset node of a captured graph was not ordered with its neighbours)
    VgGemmProb p = mk(q.u_dA, Kp, Pb + lay.conv_w, Kp, sh.MP, E, Kp);
    p.C = q.u_x[0]; p.ldc = E; p.row_in_per = sh.NP; p.row_out_per = S; p.row_out_off = 1;
    p.drop = dr.at(0); p.drop_post = 1;
    VG_TRY(vg_gemm_launch(&p, 1, VG_NT, st));
    const int splits = pick_splits(tiles128(E, Kp), sh.MP, EMB_SPLIT_CAP);
    VgGemmProb pw = wg(w.gp, E, q.u_dA, Kp, sh.MP, w.slab, (long long)E * Kp, splits);
    VG_TRY(vg_gemm_launch(&pw, 1, VG_TN, st));
    VG_TRY(vg_slab_reduce_launch(w.slab, (long long)E * Kp, pw.splits, G + lay.conv_w, (long long)E * Kp, 1, st));
  }
  // the weight gradients dW += dY^T ddX of TWO blocks go out as one grouped split-K launch + one fold (half the K slices each: half the slab
  // traffic per unit of work, like the engine's own backward), so the tangent operands of a block live in one of two buffer sets
  const int sp = block_pair_splits(sh, false);
  VgGemmProb pr[8]; int npr = 0, cur = 0;
  for (int l = 0; l < L; ++l) {
    const VitBlock b = blk(l);
    const PenBlock p = pen_block(q, sh, l);
    const bf16* gb2 = drop ? p.gm2 : p.gin;
    const bf16* gb1 = drop ? p.gm1 : p.gmid;
    const bf16* u_gx = q.u_x[cur];
    bf16* u_up = q.u_x[cur ^ 1];
    const int ps = l & 1;  // operand set, and this block's half of the slab
    bf16 *u_dxn = q.u_dxn[ps], *u_dxn2 = q.u_dxn2[ps], *u_dao = q.u_dao[ps], *u_da1 = q.u_da1[ps];
    float* slab = w.slab + (size_t)ps * sp * lay.layer_weights;
    float *pb1 = pen_part(q, sh, 2 * l), *pb2 = pen_part(q, sh, 2 * l + 1);
    // gX = gmid + LN1'(dxn1; X): the norm's double backward; u reaches gmid unchanged (added below)
    VG_TRY(vg_ln_bwd_bwd_launch(u_gx, p.dxn1, b.x, b.mean1, b.rstd1, b.P + lay.ln1_w, u_dxn, p.s_x, pb1, M, E, st));
    VG_TRY(vg_fold_push(folds, pb1, sh.bbparts, E, b.G + lay.ln1_w, E, nullptr, 0, nullptr, 0, nullptr, 0));
    // dxn1 = dqkv Wqkv
    VG_TRY(lin_fwd(u_dxn, E, b.Pb + lay.wqkv, nullptr, q.u_dqkv, M, 3 * E, VG_ACT_NONE, 0.f, nullptr, nullptr, nullptr, st));
    pr[npr++] = wg(p.dqkv, 3 * E, u_dxn, E, M, slab + lay.wqkv, lay.layer_weights, sp);
    // dqkv = attention'(dao; qkv)
    VG_TRY(vg_attn_bwd_bwd_launch(b.qkv, p.dao, b.lse, q.u_dqkv, u_dao, p.s_qkv, B, sh.H, S, sh.HE, sh.scale, st));
    // dao = gb1 Wo ; gb1 = mask1 gmid  ->  u_gmid = u_gX + mask1 (u_dao Wo^T)
    VG_TRY(lin_fwd(u_dao, E, b.Pb + lay.wo, nullptr, q.u_gmid, M, E, VG_ACT_NONE, 0.f, u_gx, nullptr, nullptr, st, dr.at(1 + 2 * l)));
    pr[npr++] = wg(gb1, E, u_dao, E, M, slab + lay.wo, lay.layer_weights, sp);
    // gmid = gin + LN2'(dxn2; x_mid)
    VG_TRY(vg_ln_bwd_bwd_launch(q.u_gmid, p.dxn2, b.xmid, b.mean2, b.rstd2, b.P + lay.ln2_w, u_dxn2, p.s_xmid, pb2, M, E, st));
    VG_TRY(vg_fold_push(folds, pb2, sh.bbparts, E, b.G + lay.ln2_w, E, nullptr, 0, nullptr, 0, nullptr, 0));
    // dxn2 = dz1 W1
    VG_TRY(lin_fwd(u_dxn2, E, b.Pb + lay.w1, nullptr, q.u_dz1, M, rE, VG_ACT_NONE, 0.f, nullptr, nullptr, nullptr, st));
    pr[npr++] = wg(p.dz1, rE, u_dxn2, E, M, slab + lay.w1, lay.layer_weights, sp);
    // dz1 = da1 gelu'(h)
    VG_TRY(vg_act2_launch(p.h, p.da1, q.u_dz1, u_da1, p.s_h, sh.MR, 1, 2, st));
    // da1 = gb2 W2 ; gb2 = mask2 gin  ->  u_gin = u_gmid + mask2 (u_da1 W2^T)
    VG_TRY(lin_fwd(u_da1, rE, b.Pb + lay.w2, nullptr, u_up, M, E, VG_ACT_NONE, 0.f, q.u_gmid, nullptr, nullptr, st, dr.at(2 + 2 * l)));
    pr[npr++] = wg(gb2, E, u_da1, rE, M, slab + lay.w2, lay.layer_weights, sp);
    if (ps == 1 || l == L - 1) {  // the pair (or the odd block out) is complete
      VG_TRY(vg_gemm_launch(pr, npr, VG_TN, st));
      const int ns = pr[0].splits;  // (the launcher may lower the slice count; every problem has the same M rows)
      if (npr == 8)
        VG_TRY(vg_slab_reduce2_launch(w.slab, w.slab + (size_t)sp * lay.layer_weights, lay.layer_weights, ns, blk(l - 1).G, b.G, lay.layer_weights, 1, st));
      else
        VG_TRY(vg_slab_reduce_launch(w.slab, lay.layer_weights, ns, b.G, lay.layer_weights, 1, st));
      npr = 0;
    }
    cur ^= 1;
  }
  {  // final LayerNorm on the CLS rows and the classifier head
    float* pbf = pen_part(q, sh, 2 * L);
    VG_TRY(vg_take_rows_launch(q.u_x[cur], q.ucls, B, S, 0, 1, E, st));
    VG_TRY(vg_take_rows_launch(blk(L - 1).x_next, q.xcls, B, S, 0, 1, E, st));
    VG_TRY(vg_ln_bwd_bwd_launch(q.ucls, w.dhcls, q.xcls, w.meanf, w.rstdf, P + lay.lnf_w, q.u_gc, q.s_xcls, pbf, B, E, st));
    VG_TRY(vg_fold_push(folds, pbf, vg_ln_bwd_bwd_nparts(B), E, G + lay.lnf_w, E, nullptr, 0, nullptr, 0, nullptr, 0));
    VG_TRY(lin_fwd(q.u_gc, E, Pb + lay.hw1, nullptr, q.u_gpre, B, E, VG_ACT_NONE, 0.f, nullptr, nullptr, nullptr, st));  // g_c = g_pre Wh1
    VgGemmProb p = wg(w.dzh, E, q.u_gc, E, B, w.slab, (long long)E * E, B >= 512 ? 4 : (B >= 256 ? 2 : 1));
    VG_TRY(vg_gemm_launch(&p, 1, VG_TN, st));
    VG_TRY(vg_slab_reduce_launch(w.slab, (long long)E * E, p.splits, G + lay.hw1, (long long)E * E, 1, st));
    // g_pre = g_t tanh'(p): u_gt (its batch sum is every row of dWh2) and dL/dp, which the second backward starts from (in w.dzh)
    VG_TRY(vg_pen_head2_launch(q.u_gpre, w.th, P + lay.hw2, q.u_gt, w.dzh, B, E, sh.Kc, st));
    for (int k = 0; k < sh.Kc; ++k) VG_TRY(vg_colsum_bf16_launch(q.u_gt, E, B, E, w.part_cs, G + lay.hw2 + (long long)k * E, 1, st));
  }
  return vg_colsum_f32_multi_launch(folds, st);
}

// One body, two fronts.  r1 = 0: WGAN-GP - `real`, `fake`, `eps` make the fp32 interpolate and pass 3 penalises (||g|| - 1)^2 (vg_vit_penalty).
// r1 = 1: the zero-centred R1 penalty of Mescheder et al. 2018 - `real` is the batch itself (bf16, patchified as it is: no interpolation
// launch, no fp32 copy; fake / eps unused) and pass 3 penalises ||g||^2 (vg_vit_r1).  Passes 2, 4 and 5 are the same launches.
static int vit_penalty_impl(const VgVitNet* net0, int B, int r1, const void* real, const void* fake, const float* eps, float weight, void* ws,
                            void* ws_pen, float* penalty_out, void* stream) {
  if (!net0 || !real || (!r1 && (!fake || !eps)) || !ws || !ws_pen || !penalty_out || B < 1 || !net0->G) return -1;
  if (!pen_shape_ok(net0, vit_shape(net0->d, B))) return -3;
  VgVitNet net = *net0;
  net.dense_top = 1; net.ctx = nullptr;
  PenWs q;
  VitPass c;  // one context for the five passes (want_wgrad is pass 5's: the others compute no column sums)
  VG_TRY(c.begin(&net, B, ws, stream, &q, 1));
  carve_pen(net.d, c.sh, ws_pen, q);
  // ---- 1. forward of the interpolated images (R1: of the images themselves) ----
  if (!r1) VG_TRY(vg_pen_interp_launch((const bf16*)real, (const bf16*)fake, eps, q.xhat, B, (long long)net.d.C * net.d.IH * net.d.IH, c.st));
  VG_TRY(c.forward(r1 ? real : q.xhat, r1, q.logits));
  VG_TRY(c.pen_first_backward());
  // ---- 3. the penalty and the direction of the second backward ----
  VG_TRY(vg_pen_norm_launch(c.w.dA, q.u_dA, q.pen_img, penalty_out, B, (long long)c.sh.NP * c.sh.Kp, weight, r1, c.st));
  VG_TRY(c.pen_tangent_backward());
  // ---- 5. the ordinary backward of pass 1 under the injected gradients ----
  c.folds.n = 0;  // (pass 4 launched its own)
  return c.backward(q.ones, nullptr, 0, c.sh.L + 2);
}
extern "C" int vg_vit_penalty(const VgVitNet* net, int B, const void* real, const void* fake, const float* eps, float weight, void* ws,
                              void* ws_pen, float* penalty_out, void* stream) {
  return vit_penalty_impl(net, B, 0, real, fake, eps, weight, ws, ws_pen, penalty_out, stream);
}
// R1: penalty = mean_b ||d sum_k D(x_b)_k / d x_b||^2 on the caller's bf16 images; G += weight * d penalty / d theta (the caller folds
// gamma / 2 and the lazy interval into weight), *penalty_out = the unweighted penalty.  Same workspaces and return codes as vg_vit_penalty.
extern "C" int vg_vit_r1(const VgVitNet* net, int B, const void* x, float weight, void* ws, void* ws_pen, float* penalty_out, void* stream) {
  return vit_penalty_impl(net, B, 1, x, nullptr, nullptr, weight, ws, ws_pen, penalty_out, stream);
}

// =============================================================================================
//                                   generator (v1 SLN / SIREN)
// =============================================================================================
#define GEN_SPLIT_CAP 16
struct GenShape {
  int B, E, H, HE, L, T, R, O, CW, PW;  // R = B T rows; PW = 3E + 64: width of an SLN backward's partial row
  long long RE;   // elements of an [R, E] tensor
  float scale;    // softmax(q.k / sqrt(H*hd)), src/v1/attention.py:51,90
  // generator rows R = B*T: the full-row kernels (SLN in the epilogue) take the Linears whose output is the embedding when E = 384 / 512
  int rown;       // 0: the tiled path
  int parts;      // partial rows of an SLN backward over R rows, either form
  // stage images in GenWs::wpack (gen_pack_weights): Wo | Wm | Wqkv^T | Wm^T per block of `pack_block` elements, then s1_w^T
  long long pack_block, po_wo, po_wm, po_wqkvT, po_wmT, po_s1T;
};
static GenShape gen_shape(const VgGenDims& d, int B) {
  GenShape s;
  s.B = B; s.E = d.E; s.H = d.H; s.HE = d.E / d.H; s.L = d.L; s.T = d.T; s.R = B * d.T; s.O = d.O; s.CW = d.CW; s.PW = 3 * d.E + 64;
  s.RE = (long long)s.R * s.E; s.scale = 1.0f / sqrtf((float)s.E);
  s.rown = (vg_row_width_ok(d.E) && d.O % 64 == 0 && d.O >= 128) ? vg_row_nwg(s.R) : 0;
  s.parts = s.rown ? s.rown : vg_ln_bwd_nparts(s.R);
  const long long EE = (long long)s.E * s.E;
  s.pack_block = 6 * EE;  // E*E + E*E + 3E*E + E*E
  s.po_wo = 0; s.po_wm = EE; s.po_wqkvT = 2 * EE; s.po_wmT = 5 * EE; s.po_s1T = s.L * s.pack_block;
  return s;
}
// full-row path: every Linear whose output is the embedding carries the SLN behind it in its epilogue (gemm_row.hip)
static int gen_pack_weights(const GenShape& sh, const VgGenLayout& lay, const bf16* Pb, bf16* wpack, hipStream_t st) {
  const int E = sh.E;
  VgPackJobs pj; pj.N = E;
  pj.src = Pb + lay.layer0; pj.dst = wpack; pj.src_stride = lay.layer_stride; pj.dst_stride = sh.pack_block; pj.nblocks = sh.L; pj.n = 4;
  pj.d[0] = {lay.wo, sh.po_wo, E, E, 0};           // output_linear forward
  pj.d[1] = {lay.wm, sh.po_wm, E, E, 0};           // block MLP forward
  pj.d[2] = {lay.wqkv, sh.po_wqkvT, 3 * E, E, 1};  // q|k|v input gradient
  pj.d[3] = {lay.wm, sh.po_wmT, E, E, 1};          // block MLP input gradient
  VG_TRY(vg_pack_rows_launch(pj, st));
  VgPackJobs ph; ph.N = E;                         // first SIREN layer's input gradient: s1_w [O, E] read transposed
  ph.src = Pb + lay.s1_w; ph.dst = wpack + sh.po_s1T; ph.src_stride = 0; ph.dst_stride = 0; ph.nblocks = 1; ph.n = 1;
  ph.d[0] = {0, 0, sh.O, E, 1};
  return vg_pack_rows_launch(ph, st);
}
struct GenWs {
  bf16 *zb, *wmod, *s1, *qkv, *cat, *htmp, *s2, *hout, *sf, *y1;
  float *lse, *mean1, *rstd1, *mean2, *rstd2, *meanf, *rstdf, *zf1, *zf2;
  bf16 *g[3], *gm[2], *dz2, *dz1, *ds, *dcat, *dqkv, *dwb;
  bf16 *y2, *dy2;  // patch-grid variant only: token rows [R, CW] before the un-patchify / after the patchify of d_img
  float *dw_acc, *part, *part_cs, *part_cs2, *emb_sum, *slab;
  bf16* wpack;  // E = 384: stage images of Wo | Wm | Wqkv^T | Wm^T per block, then s1_w^T, for the full-row GEMMs (gemm_row.hip)
  bf16 *pdqkv, *pgm1, *pgm2;  // per-block copies of the weight-gradient dY operands (dropout on): two blocks' weight gradients go out as one launch
};
static long long carve_gen(const VgGenDims& d, const GenShape& sh, const VgGenLayout& lay, void* base, GenWs& w) {
  const long long B = sh.B, E = sh.E, T = sh.T, R = sh.R, L = sh.L, RE = sh.RE;
  Carver c{(unsigned char*)base, 0};
  w.zb = c.take<bf16>(B * d.Z);
  w.wmod = c.take<bf16>(RE);
  w.s1 = c.take<bf16>(L * RE);
  w.qkv = c.take<bf16>(L * RE * 3);
  w.cat = c.take<bf16>(L * RE);
  w.htmp = c.take<bf16>(L * RE);
  w.s2 = c.take<bf16>(L * RE);
  w.hout = c.take<bf16>(L * RE);
  w.sf = c.take<bf16>(RE);
  w.y1 = c.take<bf16>(R * d.O);
  w.lse = c.take<float>(L * B * d.H * T);
  w.mean1 = c.take<float>(L * R); w.rstd1 = c.take<float>(L * R);
  w.mean2 = c.take<float>(L * R); w.rstd2 = c.take<float>(L * R);
  w.meanf = c.take<float>(R); w.rstdf = c.take<float>(R);
  w.zf1 = c.take<float>(R * d.O);
  w.zf2 = c.take<float>(R * d.CW);
  for (int i = 0; i < 3; ++i) w.g[i] = c.take<bf16>(RE);
  for (int i = 0; i < 2; ++i) w.gm[i] = c.take<bf16>(RE);
  w.dz2 = c.take<bf16>(R * d.CW);
  w.dz1 = c.take<bf16>(R * d.O);
  w.ds = c.take<bf16>(RE);
  w.dcat = c.take<bf16>(RE);
  w.dqkv = c.take<bf16>(RE * 3);
  w.dwb = c.take<bf16>(RE);
  w.y2 = c.take<bf16>(d.patch > 0 ? R * d.CW : 0);
  w.dy2 = c.take<bf16>(d.patch > 0 ? R * d.CW : 0);
  w.dw_acc = c.take<float>(RE);
  w.pdqkv = c.take<bf16>(L * RE * 3); w.pgm1 = c.take<bf16>(L * RE); w.pgm2 = c.take<bf16>(L * RE);
  w.part = c.take<float>((2 * L + 1) * (long long)vg_ln_bwd_nparts(sh.R) * sh.PW);  // one block per SLN backward
  w.part_cs = c.take<float>((long long)vg_colsum_bf16_nparts(sh.R) * (d.O > 3 * E ? d.O : 3 * E));
  w.part_cs2 = c.take<float>((long long)vg_colsum_bf16_nparts(sh.R) * d.CW);
  w.emb_sum = c.take<float>(T * E);
  long long slab = GEN_SPLIT_CAP * lay.layer_weights;
  if (GEN_SPLIT_CAP * (long long)d.O * E > slab) slab = GEN_SPLIT_CAP * (long long)d.O * E;
  w.slab = c.take<float>(slab);
  w.wpack = c.take<bf16>(sh.rown ? L * sh.pack_block + (long long)d.O * E : 0);
  return c.off;
}
extern "C" long long vg_gen_ws_bytes(const VgGenDims* d, int B) {
  VgGenLayout lay;
  if (!d || B < 1 || vg_gen_layout(d, &lay)) return -1;
  GenWs w;
  return carve_gen(*d, gen_shape(*d, B), lay, nullptr, w);
}

extern "C" int vg_gen_ws_map(const VgGenDims* d, int B, VgGenWsMap* o) {
  VgGenLayout lay;
  if (!d || !o || B < 1 || vg_gen_layout(d, &lay)) return -1;
  unsigned char* const fake = (unsigned char*)(uintptr_t)(1u << 20);  // never dereferenced
  GenWs w;
  o->total = carve_gen(*d, gen_shape(*d, B), lay, fake, w);
  auto off = [&](const void* p) { return (long long)((const unsigned char*)p - fake); };
  o->wmod = off(w.wmod); o->s1 = off(w.s1); o->qkv = off(w.qkv); o->cat = off(w.cat); o->htmp = off(w.htmp); o->s2 = off(w.s2);
  o->hout = off(w.hout); o->sf = off(w.sf); o->y1 = off(w.y1); o->zf1 = off(w.zf1); o->zf2 = off(w.zf2);
  for (int i = 0; i < 3; ++i) o->g[i] = off(w.g[i]);
  o->dw_acc = off(w.dw_acc);
  return 0;
}

// Block l as one pass sees it (the only place that strides by l).  h: the block's input - the learned embedding [T, E] broadcast over
// the batch (hb = T rows) for block 0, the output of the block below otherwise (hb = 0).  gm2 / gm1 / dqkv: the dY operands of the
// block's weight gradients - one copy PER BLOCK with dropout on, so that the weight gradients of two blocks, which read them, can wait
// for each other and go out as ONE grouped launch (half the launches, folds and slab traffic; the discriminator's pairs); without
// dropout the unmasked rotating buffers, and every block launches its own.
struct GenBlock {
  const float* P; const bf16* Pb; float* G;  // + a per-block offset of VgGenLayout
  const bf16* h; int hb; bf16 *s1, *qkv, *cat, *htmp, *s2, *hout;
  float *lse, *mean1, *rstd1, *mean2, *rstd2;
  const bf16* wp;        // packed-weight images (full-row path): + GenShape::po_*
  float *part2, *part1;  // SLN-backward partial rows of SLN2 / SLN1
  bf16 *gm2, *gm1, *dqkv;
};
// slot i of the SLN backward's partial rows: 2l / 2l + 1 = SLN2 / SLN1 of block l, 2L = the final SLN (sized for the standalone kernels)
static float* gen_part(const GenWs& w, const GenShape& sh, int i) { return w.part + (size_t)i * vg_ln_bwd_nparts(sh.R) * sh.PW; }
static GenBlock gen_block(const GenWs& w, const VgGenLayout& lay, const VgGenNet* net, const GenShape& sh, int l, bool drop) {
  const long long lo = lay.layer0 + (long long)l * lay.layer_stride;
  const size_t RE = (size_t)sh.RE, R = (size_t)sh.R;
  GenBlock b;
  b.P = net->P + lo; b.Pb = (const bf16*)net->Pb + lo; b.G = net->G ? net->G + lo : nullptr;
  b.h = (l == 0) ? (const bf16*)net->Pb + lay.emb : w.hout + (l - 1) * RE; b.hb = (l == 0) ? sh.T : 0;
  b.s1 = w.s1 + l * RE; b.qkv = w.qkv + l * RE * 3; b.cat = w.cat + l * RE; b.htmp = w.htmp + l * RE; b.s2 = w.s2 + l * RE; b.hout = w.hout + l * RE;
  b.lse = w.lse + (size_t)l * sh.B * sh.H * sh.T; b.wp = w.wpack + (size_t)l * sh.pack_block;
  b.mean1 = w.mean1 + l * R; b.rstd1 = w.rstd1 + l * R; b.mean2 = w.mean2 + l * R; b.rstd2 = w.rstd2 + l * R;
  b.part2 = gen_part(w, sh, 2 * l); b.part1 = gen_part(w, sh, 2 * l + 1);
  b.gm2 = drop ? w.pgm2 + l * RE : w.gm[0]; b.gm1 = drop ? w.pgm1 + l * RE : w.gm[1]; b.dqkv = drop ? w.pdqkv + l * RE * 3 : w.dqkv;
  return b;
}
struct GenPass {
  const VgGenNet* net; VgGenLayout lay; GenShape sh; GenWs w; Drop dr; hipStream_t st;
  const float* P; const bf16* Pb; float* G;  // net's master parameters, bf16 shadow, gradients
  VgFoldJobs folds;  // partial-sum folds queued by this call: one launch at its end
  bool drop;
  GenBlock blk(int l) const { return gen_block(w, lay, net, sh, l, drop); }
  int begin(const VgGenNet* net_, int B, void* ws, void* stream);
  int row_fwd(const bf16* A, const bf16* Wp, const float* bias, const bf16* res, const float* resf, bf16* Y, bf16* Yn, float* mean, float* rstd,
              const struct SlnP& n, int site) const;
  int dgrad_sln_bwd(const struct DgradSln& j, int step = FP_BOTH) const;
  int bwd_wgrad(int la, int nb, int splits, const bf16* gb1 = nullptr, const bf16* gb2 = nullptr) const;
};
int GenPass::begin(const VgGenNet* net_, int B, void* ws, void* stream) {
  net = net_; folds.n = 0; P = net->P; Pb = (const bf16*)net->Pb; G = net->G;
  VG_TRY(vg_gen_layout(&net->d, &lay));
  sh = gen_shape(net->d, B);
  carve_gen(net->d, sh, lay, ws, w);
  dr = Drop{net->dropout_p, net->dropout_seed, net->dropout_step};  // sites: 100+2l after output_linear, 101+2l inside the MLP
  drop = dr.on(); st = (hipStream_t)stream;
  return 0;
}
// the three parameters of a self-modulated LayerNorm: weight, bias, and the (gamma, beta) scalar pair
struct SlnP { const float *w, *b, *s; };

// y = (res | emb table) + drop(A W^T + b);  yn = SLN(y, w): the full-row launch of the generator's forward
int GenPass::row_fwd(const bf16* A, const bf16* Wp, const float* bias, const bf16* res, const float* resf, bf16* Y, bf16* Yn, float* mean, float* rstd,
                     const SlnP& n, int site) const {
  VgRowArgs ra = {};
  ra.bias = bias; ra.res = res; ra.resf = resf; ra.res_period = sh.T; ra.Y = Y; ra.Yn = Yn;
  ra.mean_out = mean; ra.rstd_out = rstd; ra.gamma = n.w; ra.beta = n.b; ra.eps = 1e-5f; ra.wmod = w.wmod; ra.gs = n.s; ra.bs = n.s + 1;
  return row_launch(ra, sh.E, A, sh.E, Wp, sh.R, VG_ROW_LNFWD, dr, site, st);
}
// dh = gres + SLN'(dy W) and dhm = dh * mask, d w accumulated into dw_acc: ONE full-row launch on the full-row path, else lin_dgrad
// into w.ds and the SLN backward (dgrad_ln_bwd's counterpart; `step` as there)
struct DgradSln {
  const bf16* dy; int N; const bf16 *W, *Wp;
  const bf16* h; int hb; const float *mean, *rstd; SlnP n;
  const bf16* gres; bf16 *dh, *dhm; int accumulate; float* part; int site;
};
int GenPass::dgrad_sln_bwd(const DgradSln& j, int step) const {
  if (sh.rown) {
    if (!(step & FP_NORM)) return 0;
    VgRowArgs ra = {};
    ra.x = j.h; ra.x_period = j.hb; ra.mean = j.mean; ra.rstd = j.rstd; ra.gamma = j.n.w; ra.lbias = j.n.b;
    ra.gs = j.n.s; ra.bs = j.n.s + 1; ra.wmod = w.wmod; ra.gres = j.gres; ra.dx = j.dh; ra.dxm = j.dhm; ra.dw_acc = w.dw_acc; ra.dw_accumulate = j.accumulate;
    ra.part = j.part;
    return row_launch(ra, sh.E, j.dy, j.N, j.Wp, sh.R, VG_ROW_LNBWD, dr, j.site, st);
  }
  if (step & FP_GEMM) VG_TRY(lin_dgrad(j.dy, j.W, w.ds, sh.R, j.N, sh.E, 0, nullptr, nullptr, 0.f, st));
  if (step & FP_NORM)
    VG_TRY(vg_sln_bwd_launch(w.ds, j.h, j.hb, w.wmod, j.mean, j.rstd, j.n.w, j.n.b, j.n.s, j.n.s + 1, j.gres, j.dh, w.dw_acc, j.accumulate, j.part,
                             sh.R, sh.E, j.dhm, dr.at(j.site), st));
  return 0;
}

// the class-conditioning argument of the _cond passes: nullptr = the unconditioned network; else every field is checked before any launch
static int gen_cond_check(const VgGenNet* net, const VgGenCond* cond, bool backward) {
  if (!cond) return 0;
  if (!net || !cond->labels || !cond->table_bf16 || (backward && !cond->table_grad)) return -1;
  if (cond->K < 1 || cond->K > 16) return -2;
  return 0;
}
extern "C" int vg_gen_forward_cond(const VgGenNet* net, int B, const float* z, void* ws, void* img, const VgGenCond* cond, void* stream) {
  if (!net || !z || !ws || !img || B < 1) return -1;
  VG_TRY(gen_cond_check(net, cond, false));
  GenPass c;
  VG_TRY(c.begin(net, B, ws, stream));
  const VgGenDims& d = net->d;
  const VgGenLayout& lay = c.lay; const GenShape& sh = c.sh; const GenWs& w = c.w; const Drop& dr = c.dr;
  hipStream_t st = c.st;
  const int E = sh.E, T = sh.T, R = sh.R;
  const float* P = c.P; const bf16* Pb = c.Pb;
  const SlnP slnf = {P + lay.slnf_w, P + lay.slnf_b, P + lay.slnf_s};

  // mapping network (generator.py:59-61): w = Linear(z) viewed [B*T, E]
  VG_TRY(vg_cast_f32_bf16_launch(z, w.zb, (long long)B * d.Z, st));
  VG_TRY(lin_fwd(w.zb, d.Z, Pb + lay.map_w, P + lay.map_b, w.wmod, B, T * E, VG_ACT_NONE, 0.f, nullptr, nullptr, nullptr, st));
  if (cond)  // w += class_embedding[y]: the K one-hot input columns of the mapping Linear, as a gather
    VG_TRY(vg_class_add_launch(w.wmod, (const bf16*)cond->table_bf16, cond->labels, B, T * E, cond->K, st));
  if (sh.rown) VG_TRY(gen_pack_weights(sh, lay, Pb, w.wpack, st));

  for (int l = 0; l < sh.L; ++l) {
    const GenBlock b = c.blk(l);
    const SlnP sln1 = {b.P + lay.sln1_w, b.P + lay.sln1_b, b.P + lay.sln1_s}, sln2 = {b.P + lay.sln2_w, b.P + lay.sln2_b, b.P + lay.sln2_s};
    if (!sh.rown || l == 0)  // block 0 normalises the broadcast embedding; later blocks got s1 from the MLP epilogue of the block below
      VG_TRY(vg_sln_fwd_launch(b.h, b.hb, w.wmod, sln1.w, sln1.b, sln1.s, sln1.s + 1, b.s1, b.mean1, b.rstd1, R, E, 1e-5f, st));
    VG_TRY(lin_fwd(b.s1, E, b.Pb + lay.wqkv, nullptr, b.qkv, R, 3 * E, VG_ACT_NONE, 0.f, nullptr, nullptr, nullptr, st));
    VG_TRY(vg_attn_fwd_launch(b.qkv, b.cat, b.lse, B, sh.H, T, sh.HE, sh.scale, 0, st));
    if (sh.rown) {  // htmp = output_linear(cat) + h (block 0: + the broadcast embedding) and SLN2(htmp) in one kernel
      VG_TRY(c.row_fwd(b.cat, b.wp + sh.po_wo, b.P + lay.bo, l == 0 ? nullptr : b.h, l == 0 ? P + lay.emb : nullptr, b.htmp, b.s2, b.mean2, b.rstd2,
                         sln2, 100 + 2 * l));
      // hout = drop(mlp(s2)) + htmp and the NEXT SLN of it: the block above's SLN1, or the final SLN in front of the SIREN
      const bool nx = l + 1 < sh.L;
      const GenBlock nb = nx ? c.blk(l + 1) : GenBlock{};
      VG_TRY(c.row_fwd(b.s2, b.wp + sh.po_wm, b.P + lay.bm, b.htmp, nullptr, b.hout, nx ? nb.s1 : w.sf, nx ? nb.mean1 : w.meanf, nx ? nb.rstd1 : w.rstdf,
                       nx ? SlnP{nb.P + lay.sln1_w, nb.P + lay.sln1_b, nb.P + lay.sln1_s} : slnf, 101 + 2 * l));
    } else {
      {  // htmp = output_linear(cat) + h   (transformer.py:86); block 0 adds the broadcast embedding
        VgGemmProb p = mk(b.cat, E, b.Pb + lay.wo, E, R, E, E);
        p.C = b.htmp; p.ldc = E; p.bias = b.P + lay.bo;
        if (l == 0) { p.resf = P + lay.emb; p.res_period = T; } else { p.res = b.h; p.ldr = E; }
        p.drop = dr.at(100 + 2 * l);  // attention_dropout(msha(...)) + h, transformer.py:86
        VG_TRY(vg_gemm_launch(&p, 1, VG_NT, st));
      }
      VG_TRY(vg_sln_fwd_launch(b.htmp, 0, w.wmod, sln2.w, sln2.b, sln2.s, sln2.s + 1, b.s2, b.mean2, b.rstd2, R, E, 1e-5f, st));
      VG_TRY(lin_fwd(b.s2, E, b.Pb + lay.wm, b.P + lay.bm, b.hout, R, E, VG_ACT_NONE, 0.f, b.htmp, nullptr, nullptr, st,
                     dr.at(101 + 2 * l)));  // Sequential(Linear, Dropout) + htmp, muilti_layer_perceptron.py:26-28
    }
  }
  if (!sh.rown)
    VG_TRY(vg_sln_fwd_launch(c.blk(sh.L - 1).hout, 0, w.wmod, slnf.w, slnf.b, slnf.s, slnf.s + 1, w.sf, w.meanf, w.rstdf, R, E, 1e-5f, st));
  if (net->pos_table) VG_TRY(vg_add_table_launch(w.sf, net->pos_table, R, E, T, st));  // constant: the backward is unchanged
  VG_TRY(lin_fwd(w.sf, E, Pb + lay.s1_w, P + lay.s1_b, w.y1, R, d.O, VG_ACT_SIN, d.omega0, nullptr, nullptr, w.zf1, st));
  bf16* rows = d.patch > 0 ? w.y2 : (bf16*)img;
  VG_TRY(lin_fwd(w.y1, d.O, Pb + lay.s2_w, P + lay.s2_b, rows, R, d.CW, VG_ACT_SIN, d.omega0, nullptr, nullptr, w.zf2, st));
  if (d.patch > 0) VG_TRY(vg_unpatchify_launch(rows, (bf16*)img, B, d.C, d.IH, d.patch, st));  // token rows -> NCHW
  return 0;
}

extern "C" int vg_gen_forward(const VgGenNet* net, int B, const float* z, void* ws, void* img, void* stream) {
  return vg_gen_forward_cond(net, B, z, ws, img, nullptr, stream);
}

// K slices of a grouped weight-gradient launch over `nblocks` generator blocks (three problems each)
static int gen_block_splits(const GenShape& sh, int nblocks, int cap) {
  const int E = sh.E;
  if (const int bn = wide_bn(E, E); bn && sh.R % 32 == 0 && E % 128 == 0)
    return pick_splits384(nblocks * (tiles_wide(3 * E, E, bn) + 2 * tiles_wide(E, E, bn)), sh.R, cap);
  return pick_splits(nblocks * (tiles128(3 * E, E) + 2 * tiles128(E, E)), sh.R, cap);
}
// weight gradients of blocks la, la - 1 (nb = 2) or of la alone: grouped split-K launch + fold.  A pair, and the odd block out of a
// call with dropout on, take the K partition of a pair (every schedule adds the same slices); without dropout a block takes its own,
// and gb1 / gb2 - the rotating buffers - are its out-projection and MLP operands in place of the per-block copies.
int GenPass::bwd_wgrad(int la, int nb, int splits, const bf16* gb1, const bf16* gb2) const {
  const int E = sh.E, R = sh.R;
  VgGemmProb pr[6];
  for (int j = 0; j < nb; ++j) {
    const GenBlock b = blk(la - j);
    float* slab = w.slab + (size_t)j * splits * lay.layer_weights;
    pr[3 * j + 0] = wg(b.dqkv, 3 * E, b.s1, E, R, slab + lay.wqkv, lay.layer_weights, splits);
    pr[3 * j + 1] = wg(gb1 ? gb1 : b.gm1, E, b.cat, E, R, slab + lay.wo, lay.layer_weights, splits);
    pr[3 * j + 2] = wg(gb2 ? gb2 : b.gm2, E, b.s2, E, R, slab + lay.wm, lay.layer_weights, splits);
  }
  VG_TRY(vg_gemm_launch(pr, 3 * nb, VG_TN, st));
  if (nb == 2)
    return vg_slab_reduce2_launch(w.slab, w.slab + (size_t)splits * lay.layer_weights, lay.layer_weights, pr[0].splits, blk(la).G, blk(la - 1).G,
                                  lay.layer_weights, 1, st);
  return vg_slab_reduce_launch(w.slab, lay.layer_weights, pr[0].splits, blk(la).G, lay.layer_weights, 1, st);
}

// Backward stages: 0 = SIREN output layers + final SLN, 1..L = blocks L-1 .. 0, L+1 = learned embedding + mapping Linear.
// After a call returning stages up to s (1 <= s <= L) the gradients of blocks >= L-s and of everything behind the blocks
// (final SLN, SIREN) - a contiguous tail of the flat buffer from layer0 + (L-s)*layer_stride - are final.
extern "C" int vg_gen_backward_stages_cond(const VgGenNet* net, int B, void* ws, const void* d_img, int stage_begin, int stage_end,
                                           const VgGenCond* cond, void* stream) {
  if (!net || !ws || !d_img || !net->G || B < 1) return -1;
  if (stage_begin < 0 || stage_end > net->d.L + 2 || stage_begin >= stage_end) return -2;
  VG_TRY(gen_cond_check(net, cond, true));
  GenPass c;
  VG_TRY(c.begin(net, B, ws, stream));
  const VgGenDims& d = net->d;
  const VgGenLayout& lay = c.lay; const GenShape& sh = c.sh; const GenWs& w = c.w;
  hipStream_t st = c.st;
  const int E = sh.E, T = sh.T, R = sh.R, L = sh.L, PW = sh.PW;
  const float* P = c.P; const bf16* Pb = c.Pb; float* G = c.G;
  const bool drop = c.drop;
  bf16 *g = w.g[0], *gmid = w.g[1], *gin = w.g[2];
  if (stage_begin == 0) {
    // SIREN output layers (siren.py:44-45): y = sin(w0 z)  ->  dz = dy * w0 cos(w0 z)
    const bf16* d_rows = (const bf16*)d_img;
    if (d.patch > 0) {  // NCHW gradient -> token rows, the adjoint of the forward scatter
      VG_TRY(vg_patchify_launch(d_img, 1, w.dy2, B, d.C, d.IH, d.patch, st));
      d_rows = w.dy2;
    }
    VG_TRY(vg_sin_grad_launch(d_rows, w.zf2, w.dz2, (long long)R * d.CW, d.omega0, st));
    // bias gradients of the two SIREN layers = column sums of the weight gradients' dY operands: they ride along in those GEMMs (ones x dY on the
    // MFMA pipe, one row per K slice - two 11 us column-sum launches less) and are folded with the SLN partials at the end of this call
    auto siren_wgrad = [&](const bf16* dz, int N, const bf16* X, int K, float* part_cs, float* dW, float* db) -> int {
      int splits = pick_splits(tiles128(N, K), R, GEN_SPLIT_CAP);
      if (splits > vg_colsum_bf16_nparts(R)) splits = vg_colsum_bf16_nparts(R);  // (part_cs / part_cs2 hold that many rows)
      VgGemmProb p = wg(dz, N, X, K, R, w.slab, (long long)N * K, splits);
      p.colsum = part_cs; p.colsum_split_stride = N;
      VG_TRY(vg_gemm_launch(&p, 1, VG_TN, st));
      VG_TRY(vg_slab_reduce_launch(w.slab, (long long)N * K, p.splits, dW, (long long)N * K, 1, st));
      return vg_fold_push(c.folds, part_cs, p.splits, N, db, N, nullptr, 0, nullptr, 0, nullptr, 0);
    };
    VG_TRY(siren_wgrad(w.dz2, d.CW, w.y1, d.O, w.part_cs2, G + lay.s2_w, G + lay.s2_b));
    VG_TRY(lin_dgrad(w.dz2, Pb + lay.s2_w, w.dz1, R, d.CW, d.O, VG_ACT_MUL_COS, nullptr, w.zf1, d.omega0, st));
    VG_TRY(siren_wgrad(w.dz1, d.O, w.sf, E, w.part_cs, G + lay.s1_w, G + lay.s1_b));
    // first SIREN layer's input gradient + the final SLN's backward: dL/d(hout of the top block), masked for the MLP dropout it meets next
    const GenBlock bt = c.blk(L - 1);
    float* partf = gen_part(w, sh, 2 * L);
    VG_TRY(c.dgrad_sln_bwd({w.dz1, d.O, Pb + lay.s1_w, w.wpack + sh.po_s1T, bt.hout, 0, w.meanf, w.rstdf, {P + lay.slnf_w, P + lay.slnf_b, P + lay.slnf_s},
                             nullptr, g, drop ? bt.gm2 : nullptr, 0, partf, 101 + 2 * (L - 1)}));
    VG_TRY(vg_fold_push(c.folds, partf, sh.parts, PW, G + lay.slnf_w, E, G + lay.slnf_b, E, bt.G + lay.bm, E, G + lay.slnf_s, 2));
  }  // stage 0
  int pend[2], npend = 0;
  for (int l = L - 1; l >= 0; --l) {
    const int stage = L - l;
    if (stage >= stage_end) break;
    if (stage < stage_begin) { bf16* t = g; g = gin; gin = t; continue; }  // the buffers rotate once per block already done
    const GenBlock b = c.blk(l);
    // hout = drop(mlp(s2)) + htmp  (transformer.py:87; MLP is a single Linear, muilti_layer_perceptron.py:37-42)
    const bf16* gb2 = drop ? b.gm2 : g;
    // block MLP input gradient + SLN2 backward + the residual-stream gradient
    VG_TRY(c.dgrad_sln_bwd({gb2, E, b.Pb + lay.wm, b.wp + sh.po_wmT, b.htmp, 0, b.mean2, b.rstd2, {b.P + lay.sln2_w, b.P + lay.sln2_b, b.P + lay.sln2_s},
                             g, gmid, drop ? b.gm1 : nullptr, 1, b.part2, 100 + 2 * l}));
    const bf16* gb1 = drop ? b.gm1 : gmid;
    VG_TRY(vg_fold_push(c.folds, b.part2, sh.parts, PW, b.G + lay.sln2_w, E, b.G + lay.sln2_b, E, b.G + lay.bo, E, b.G + lay.sln2_s, 2));
    VG_TRY(lin_dgrad(gb1, b.Pb + lay.wo, w.dcat, R, E, E, 0, nullptr, nullptr, 0.f, st));
    VG_TRY(vg_attn_bwd_launch(b.qkv, b.cat, w.dcat, b.lse, b.dqkv, B, sh.H, T, sh.HE, sh.scale, 0, st));
    // q|k|v input gradient + SLN1 backward + the residual-stream gradient: dL/d(hout of the block below), masked for its MLP dropout
    const DgradSln n1 = {b.dqkv, 3 * E, b.Pb + lay.wqkv, b.wp + sh.po_wqkvT, b.h, b.hb, b.mean1, b.rstd1, {b.P + lay.sln1_w, b.P + lay.sln1_b, b.P + lay.sln1_s},
                         gmid, gin, (drop && l > 0) ? c.blk(l - 1).gm2 : nullptr, 1, b.part1, 101 + 2 * (l - 1)};
    VG_TRY(c.dgrad_sln_bwd(n1, FP_GEMM));
    if (!drop) {  // the operands are the rotating buffers: this block's weight gradients now
      VG_TRY(c.bwd_wgrad(l, 1, gen_block_splits(sh, 1, GEN_SPLIT_CAP), gb1, gb2));
    } else {  // per-block operands: two blocks per launch (the odd one out of a call goes alone, with the SAME K partition: every schedule adds the same slices)
      pend[npend++] = l;
      if (npend == 2) { VG_TRY(c.bwd_wgrad(pend[0], 2, gen_block_splits(sh, 2, GEN_SPLIT_CAP / 2))); npend = 0; }
    }
    VG_TRY(c.dgrad_sln_bwd(n1, FP_NORM));
    // (the MLP bias of the block below: the column sums of dL/d(its hout))
    VG_TRY(vg_fold_push(c.folds, b.part1, sh.parts, PW, b.G + lay.sln1_w, E, b.G + lay.sln1_b, E, l > 0 ? c.blk(l - 1).G + lay.bm : nullptr, E, b.G + lay.sln1_s, 2));
    bf16* t = g; g = gin; gin = t;
  }
  if (npend == 1) VG_TRY(c.bwd_wgrad(pend[0], 1, gen_block_splits(sh, 2, GEN_SPLIT_CAP / 2)));  // the odd block out of this call
  VG_TRY(vg_colsum_f32_multi_launch(c.folds, st));  // all SLN partial sums queued by this call in one launch
  if (stage_end < L + 2) return 0;
  // learned embedding (generator.py:24-26,62) is broadcast over the batch: its gradient is the batch sum
  VG_TRY(vg_batch_sum_launch(g, w.emb_sum, B, T, E, st));
  VG_TRY(vg_slab_reduce_launch(w.emb_sum, 0, 1, G + lay.emb, (long long)T * E, 1, st));
  // mapping Linear: d W = d w^T z ; d b = colsum(d w)   (d w accumulated in fp32 over the 2L+1 SLN uses)
  VG_TRY(vg_colsum_f32_launch(w.dw_acc, B, T * E, G + lay.map_b, T * E, nullptr, 0, nullptr, 0, nullptr, 0, 1, st));
  if (cond)  // class embedding: row k = the sum of d w over the samples of class k (accumulated, like every gradient)
    VG_TRY(vg_class_grad_launch(w.dw_acc, cond->labels, cond->table_grad, B, T * E, cond->K, 1, st));
  VG_TRY(vg_cast_f32_bf16_launch(w.dw_acc, w.dwb, sh.RE, st));
  {
    // K = B rows only: one K slice, accumulated straight into the gradient buffer (a 50 MB slab and its fold pass saved)
    VgGemmProb p = wg(w.dwb, T * E, w.zb, d.Z, B, G + lay.map_w, 0, 1);
    p.cf_accumulate = 1;
    VG_TRY(vg_gemm_launch(&p, 1, VG_TN, st));
  }
  return 0;
}

extern "C" int vg_gen_backward_stages(const VgGenNet* net, int B, void* ws, const void* d_img, int stage_begin, int stage_end,
                                      void* stream) {
  return vg_gen_backward_stages_cond(net, B, ws, d_img, stage_begin, stage_end, nullptr, stream);
}
extern "C" int vg_gen_backward_cond(const VgGenNet* net, int B, void* ws, const void* d_img, const VgGenCond* cond, void* stream) {
  if (!net) return -1;
  return vg_gen_backward_stages_cond(net, B, ws, d_img, 0, net->d.L + 2, cond, stream);
}
extern "C" int vg_gen_backward(const VgGenNet* net, int B, void* ws, const void* d_img, void* stream) {
  return vg_gen_backward_cond(net, B, ws, d_img, nullptr, stream);
}
