// fp32 mode of the v1 generator (src/v1/generator.py:58-69): mapping Linear -> L x TransformerSLN -> SLN -> SIREN x2 with fp32
// activations, saved tensors, gradients and GEMM operands, reading the fp32 master P and accumulating into the fp32 gradient buffer G
// of the shared flat layout (vg_gen_layout).  The Linears, the attention and the column sums are the fp32 mode's own (gemm_f32.hip,
// attention_f32.hip); this file adds the self-modulated LayerNorm, the SIREN's elementwise backward, the small broadcast / class-table
// kernels, the host code that chains them on one stream, and the extern "C" entry points.  No atomics: every sum has a fixed order.
#include "../../include/vitgan_hip.h"
#include "vg_f32.h"
#include "vg_kernels.h"

// ---------------------------------------------------------------------------------------------------------------------
// self-modulated LayerNorm (src/v1/spectral_layer_norm.py:19-20).  One wave per row, the row in registers (E / 64 floats per lane),
// two-pass statistics: norm_f32.hip's LayerNorm with the modulation behind it.
template <int NV>
__global__ __launch_bounds__(256) void vg_f32_sln_fwd_kernel(const float* __restrict__ h, int hb, const float* __restrict__ w,
                                                             const float* __restrict__ lw, const float* __restrict__ lb,
                                                             const float* __restrict__ gs, const float* __restrict__ bs, float* __restrict__ y,
                                                             float* __restrict__ mean, float* __restrict__ rstd, int R, float eps) {
  constexpr int E = 64 * NV;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;
  const float* hr = h + (long long)(hb > 0 ? r % hb : r) * E;
  float v[NV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) { v[i] = hr[lane + 64 * i]; s += v[i]; }
  const float mu = vg_wave_sum(s) / (float)E;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) { const float d = v[i] - mu; q = fmaf(d, d, q); }
  const float rs = 1.0f / sqrtf(vg_wave_sum(q) / (float)E + eps);
  const float g = gs[0], b = bs[0];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    const float l = fmaf((v[i] - mu) * rs, lw[c], lb[c]);
    y[(long long)r * E + c] = w[(long long)r * E + c] * fmaf(g, l, b);
  }
  if (lane == 0) { mean[r] = mu; rstd[r] = rs; }
}

__device__ __forceinline__ double f32_wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// dh, dw and the row's two scalar terms: rowsum[2r] = sum_c dy w l, rowsum[2r + 1] = sum_c dy w (l = xhat lw + lb), summed in fp64
template <int NV>
__global__ __launch_bounds__(256) void vg_f32_sln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ h, int hb,
                                                             const float* __restrict__ w, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, const float* __restrict__ lw,
                                                             const float* __restrict__ lb, const float* __restrict__ gs,
                                                             const float* __restrict__ bs, const float* __restrict__ gres, float* __restrict__ dh,
                                                             float* __restrict__ dw_acc, int dw_accumulate, double* __restrict__ rowsum, int R) {
  constexpr int E = 64 * NV;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;
  const float* hr = h + (long long)(hb > 0 ? r % hb : r) * E;
  const long long ro = (long long)r * E;
  const float mu = mean[r], rs = rstd[r], g = gs[0], b = bs[0];
  float xh[NV], gy[NV];
  float a = 0.f, c2 = 0.f;
  double sg = 0.0, sb = 0.0;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    xh[i] = (hr[c] - mu) * rs;
    const float l = fmaf(xh[i], lw[c], lb[c]), d = dy[ro + c], dyw = d * w[ro + c];
    const float dwv = d * fmaf(g, l, b);
    dw_acc[ro + c] = dw_accumulate ? dw_acc[ro + c] + dwv : dwv;
    sg += (double)(dyw * l);
    sb += (double)dyw;
    gy[i] = dyw * g * lw[c];
    a = fmaf(gy[i], xh[i], a);
    c2 += gy[i];
  }
  const float m1 = vg_wave_sum(a) / (float)E, m2 = vg_wave_sum(c2) / (float)E;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    float v = rs * (gy[i] - m2 - xh[i] * m1);
    if (gres) v += gres[ro + c];
    dh[ro + c] = v;
  }
  if (rowsum) {
    sg = f32_wave_sum_f64(sg);
    sb = f32_wave_sum_f64(sb);
    if (lane == 0) { rowsum[2 * (long long)r] = sg; rowsum[2 * (long long)r + 1] = sb; }
  }
}

// parameter sums of one 256-row chunk in fp64 (the rule of vg_f32_colsum_launch): part[chunk][c] = sum d xhat, part[chunk][E + c] =
// sum d with d = dy w gs; part[chunk][2E], [2E + 1] = the chunk's sums of the rows' scalar terms
#define SLN_F32_ROWS 256
__global__ __launch_bounds__(256) void vg_f32_sln_param_part_kernel(const float* __restrict__ dy, const float* __restrict__ h, int hb,
                                                                    const float* __restrict__ w, const float* __restrict__ mean,
                                                                    const float* __restrict__ rstd, const float* __restrict__ gs,
                                                                    const double* __restrict__ rowsum, int R, int E, float* __restrict__ part) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int r0 = blockIdx.y * SLN_F32_ROWS, r1 = min(R, r0 + SLN_F32_ROWS);
  float* prow = part + (long long)blockIdx.y * (2 * E + 2);
  if (c < E) {
    const float g = gs[0];
    double ag = 0.0, ab = 0.0;
    for (int r = r0; r < r1; ++r) {
      const float d = dy[(long long)r * E + c] * w[(long long)r * E + c] * g;
      const float xh = (h[(long long)(hb > 0 ? r % hb : r) * E + c] - mean[r]) * rstd[r];
      ag += (double)(d * xh);
      ab += (double)d;
    }
    prow[c] = (float)ag;
    prow[E + c] = (float)ab;
  }
  if (blockIdx.x == 0 && threadIdx.x < 2) {
    double s = 0.0;
    for (int r = r0; r < r1; ++r) s += rowsum[2 * (long long)r + threadIdx.x];
    prow[2 * E + threadIdx.x] = (float)s;
  }
}
// the chunks added in order (fp64), then one addition into the gradient
__global__ __launch_bounds__(256) void vg_f32_sln_param_fold_kernel(const float* __restrict__ part, int nparts, int E, float* __restrict__ dlw,
                                                                    float* __restrict__ dlb, float* __restrict__ dgs, float* __restrict__ dbs) {
  const int c = blockIdx.x * 256 + threadIdx.x, N = 2 * E + 2;
  if (c >= N) return;
  double a = 0.0;
  for (int p = 0; p < nparts; ++p) a += (double)part[(long long)p * N + c];
  float* dst = c < E ? dlw + c : c < 2 * E ? dlb + (c - E) : c == 2 * E ? dgs : dbs;
  *dst += (float)a;
}

#define SLN_F32_NV_SWITCH(E_, CALL)                                                                         \
  switch ((E_) >> 7) {                                                                                      \
    case 1: CALL(2); break; case 2: CALL(4); break; case 3: CALL(6); break; case 4: CALL(8); break;         \
    case 5: CALL(10); break; case 6: CALL(12); break; case 7: CALL(14); break; case 8: CALL(16); break;     \
    default: return -3;                                                                                     \
  }
static inline bool sln_f32_width_ok(int E) { return E >= 128 && E <= 1024 && !(E & 127); }
static inline long long sln_f32_part_row_floats(int R, int E) { return ((long long)vg_f32_colsum_parts(R) * (2 * E + 2) + 1) & ~1LL; }
long long vg_f32_sln_part_floats(int R, int E) {
  if (R < 1 || !sln_f32_width_ok(E)) return -2;
  return sln_f32_part_row_floats(R, E) + 4LL * R;  // the chunks' partial rows, then two doubles per row
}

int vg_f32_sln_fwd_launch(const float* h, int hb, const float* w, const float* lw, const float* lb, const float* gs, const float* bs, float* y,
                          float* mean, float* rstd, int R, int E, float eps, hipStream_t st) {
  if (!h || !w || !lw || !lb || !gs || !bs || !y || !mean || !rstd) return -1;
  if (R < 1 || hb < 0) return -2;
  if (!sln_f32_width_ok(E)) return -3;
#define SLN_F32_FWD(NV_) hipLaunchKernelGGL(vg_f32_sln_fwd_kernel<NV_>, dim3((R + 3) / 4), dim3(256), 0, st, h, hb, w, lw, lb, gs, bs, y, mean, rstd, R, eps)
  SLN_F32_NV_SWITCH(E, SLN_F32_FWD)
#undef SLN_F32_FWD
  return (int)hipGetLastError();
}

int vg_f32_sln_bwd_launch(const float* dy, const float* h, int hb, const float* w, const float* mean, const float* rstd, const float* lw,
                          const float* lb, const float* gs, const float* bs, const float* gres, float* dh, float* dw_acc, int dw_accumulate,
                          float* dlw, float* dlb, float* dgs, float* dbs, float* part, int R, int E, hipStream_t st) {
  if (!dy || !h || !w || !mean || !rstd || !lw || !lb || !gs || !bs || !dh || !dw_acc) return -1;
  const bool params = dlw || dlb || dgs || dbs;
  if (params && (!dlw || !dlb || !dgs || !dbs || !part)) return -1;
  if (R < 1 || hb < 0 || (dw_accumulate != 0 && dw_accumulate != 1)) return -2;
  if (!sln_f32_width_ok(E) || (params && ((uintptr_t)part & 7))) return -3;
  double* rowsum = params ? (double*)(part + sln_f32_part_row_floats(R, E)) : nullptr;
#define SLN_F32_BWD(NV_)                                                                                                                 \
  hipLaunchKernelGGL(vg_f32_sln_bwd_kernel<NV_>, dim3((R + 3) / 4), dim3(256), 0, st, dy, h, hb, w, mean, rstd, lw, lb, gs, bs, gres, dh, \
                     dw_acc, dw_accumulate, rowsum, R)
  SLN_F32_NV_SWITCH(E, SLN_F32_BWD)
#undef SLN_F32_BWD
  VG_CHECK_HIP(hipGetLastError());
  if (!params) return 0;
  const int np = vg_f32_colsum_parts(R);
  hipLaunchKernelGGL(vg_f32_sln_param_part_kernel, dim3((E + 255) / 256, np), dim3(256), 0, st, dy, h, hb, w, mean, rstd, gs,
                     (const double*)rowsum, R, E, part);
  VG_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(vg_f32_sln_param_fold_kernel, dim3((2 * E + 2 + 255) / 256), dim3(256), 0, st, (const float*)part, np, E, dlw, dlb, dgs, dbs);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// elementwise
static inline unsigned gen_f32_nblk(long long n) { return (unsigned)((n + 255) / 256); }

// the last SIREN layer's backward (siren.py:44-45): y = sin(w0 z) -> dz = dy * w0 cos(w0 z); the product w0 z rounded once, accurate cosf
__global__ __launch_bounds__(256) void vg_f32_sin_grad_kernel(const float* __restrict__ dy, const float* __restrict__ z, float* __restrict__ dz,
                                                              long long n, float w0) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  dz[i] = dy[i] * (w0 * cosf(w0 * z[i]));
}
int vg_f32_sin_grad_launch(const float* dy, const float* z, float* dz, long long n, float omega0, hipStream_t st) {
  if (!dy || !z || !dz) return -1;
  if (n < 1) return -2;
  hipLaunchKernelGGL(vg_f32_sin_grad_kernel, dim3(gen_f32_nblk(n)), dim3(256), 0, st, dy, z, dz, n, omega0);
  return (int)hipGetLastError();
}

// (add may be y itself: neither is restrict)
__global__ __launch_bounds__(256) void vg_f32_bcast_kernel(const float* __restrict__ x, long long period, const float* add, float* y, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = x[i % period];
  y[i] = add ? add[i] + v : v;
}
int vg_f32_bcast_launch(const float* x, long long period, const float* add, float* y, long long n, hipStream_t st) {
  if (!x || !y) return -1;
  if (n < 1 || period < 1) return -2;
  hipLaunchKernelGGL(vg_f32_bcast_kernel, dim3(gen_f32_nblk(n)), dim3(256), 0, st, x, period, add, y, n);
  return (int)hipGetLastError();
}

__global__ __launch_bounds__(256) void vg_f32_class_add_kernel(float* __restrict__ wmod, const float* __restrict__ table,
                                                               const int* __restrict__ labels, int B, long long N, int K) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * N) return;
  const int y = min(max(labels[i / N], 0), K - 1);
  wmod[i] += table[(long long)y * N + i % N];
}
int vg_f32_class_add_launch(float* wmod, const float* table, const int* labels, int B, long long N, int K, hipStream_t st) {
  if (!wmod || !table || !labels || B < 1 || N < 1) return -1;
  if (K < 1 || K > 16) return -2;
  hipLaunchKernelGGL(vg_f32_class_add_kernel, dim3(gen_f32_nblk((long long)B * N)), dim3(256), 0, st, wmod, table, labels, B, N, K);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// the whole network
namespace {

struct GenF32Ws {
  float *z, *wmod, *H, *s1, *qkv, *cat, *htmp, *s2, *sf, *y1, *zf1, *zf2, *rows;  // H: [L + 1][R, E], H[0] = the broadcast embedding
  float *lse, *mean1, *rstd1, *mean2, *rstd2, *meanf, *rstdf;
  float *g[2], *gmid, *gm, *ds, *dcat, *dqkv, *dz2, *dz1, *drows, *dw_acc, *part, *slab;
};

long long gmax(long long a, long long b) { return a > b ? a : b; }

long long carve_gen_f32(const VgGenDims& d, int B, void* base, GenF32Ws& w) {
  const long long E = d.E, T = d.T, R = (long long)B * T, L = d.L, RE = R * E, O = d.O, CW = d.CW;
  Carver c{(unsigned char*)base, 0};
  w.z = c.take<float>((long long)B * d.Z); w.wmod = c.take<float>(RE);
  w.H = c.take<float>((L + 1) * RE);
  w.s1 = c.take<float>(L * RE); w.qkv = c.take<float>(L * RE * 3); w.cat = c.take<float>(L * RE);
  w.htmp = c.take<float>(L * RE); w.s2 = c.take<float>(L * RE);
  w.sf = c.take<float>(RE); w.y1 = c.take<float>(R * O); w.zf1 = c.take<float>(R * O); w.zf2 = c.take<float>(R * CW);
  w.rows = c.take<float>(d.patch > 0 ? R * CW : 0);
  w.lse = c.take<float>(L * B * d.H * T);
  w.mean1 = c.take<float>(L * R); w.rstd1 = c.take<float>(L * R); w.mean2 = c.take<float>(L * R); w.rstd2 = c.take<float>(L * R);
  w.meanf = c.take<float>(R); w.rstdf = c.take<float>(R);
  w.g[0] = c.take<float>(RE); w.g[1] = c.take<float>(RE); w.gmid = c.take<float>(RE); w.gm = c.take<float>(RE);
  w.ds = c.take<float>(RE); w.dcat = c.take<float>(RE); w.dqkv = c.take<float>(RE * 3);
  w.dz2 = c.take<float>(R * CW); w.dz1 = c.take<float>(R * O); w.drows = c.take<float>(d.patch > 0 ? R * CW : 0);
  w.dw_acc = c.take<float>(RE);
  w.part = c.take<float>(gmax(vg_f32_sln_part_floats((int)R, (int)E), (long long)vg_f32_colsum_parts(B) * T * E));
  long long slab = vg_f32_wgrad_slab_floats((int)R, (int)CW, (int)O);
  slab = gmax(slab, vg_f32_wgrad_slab_floats((int)R, (int)O, (int)E));
  slab = gmax(slab, vg_f32_wgrad_slab_floats((int)R, (int)(3 * E), (int)E));
  slab = gmax(slab, vg_f32_wgrad_slab_floats(B, (int)(T * E), d.Z));
  w.slab = c.take<float>(slab);
  return c.off;
}

// -3: a shape vg_gen_layout refuses, more tokens than the fp32 attention kernels take, or an embedding wider than the SLN kernels'
int check_dims(const VgGenDims* d, VgGenLayout& lay) {
  if (vg_gen_layout(d, &lay)) return -3;
  if (d->T < 1 || d->T > VG_SHORT_MAX_S || d->E > 1024 || d->Z < 1 || d->O < 1 || d->CW < 1) return -3;
  return 0;
}
int check_cond(const VgGenCondF32* cond, bool backward) {
  if (!cond) return 0;
  if (!cond->labels || !cond->table || (backward && !cond->table_grad)) return -1;
  return 0;
}

struct SlnF { const float *w, *b, *s; };  // weight, bias, and the (gamma, beta) scalar pair
struct SlnG { float *w, *b, *s; };

}  // namespace

extern "C" long long vg_gen_ws_bytes_f32(const VgGenDims* d, int B) {
  VgGenLayout lay;
  if (!d || B < 1 || check_dims(d, lay)) return -1;
  GenF32Ws w;
  return carve_gen_f32(*d, B, nullptr, w);
}

extern "C" int vg_gen_forward_f32(const VgGenNet* net, int B, const float* z, void* ws, float* img, const VgGenCondF32* cond, void* stream) {
  if (!net || !net->P || !z || !ws || !img || B < 1) return -1;
  VG_TRY(check_cond(cond, false));
  if (cond && (cond->K < 1 || cond->K > 16)) return -2;
  VgGenLayout lay;
  VG_TRY(check_dims(&net->d, lay));
  const VgGenDims& d = net->d;
  hipStream_t st = (hipStream_t)stream;
  const int E = d.E, T = d.T, R = B * T, L = d.L, HE = E / d.H;
  const long long RE = (long long)R * E, TE = (long long)T * E;
  GenF32Ws w; carve_gen_f32(d, B, ws, w);
  const float* P = net->P;
  const Drop dr = {net->dropout_p, net->dropout_seed, net->dropout_step};  // sites: 100 + 2l after output_linear, 101 + 2l inside the MLP
  const float scale = 1.0f / sqrtf((float)E);                              // softmax(q.k / sqrt(H * hd)), src/v1/attention.py:51,90

  // mapping network (generator.py:59-61): w = Linear(z) viewed [B*T, E]; z is kept for the weight gradient
  VG_TRY(vg_f32_bcast_launch(z, (long long)B * d.Z, nullptr, w.z, (long long)B * d.Z, st));
  VG_TRY(vg_f32_linear_fwd(w.z, P + lay.map_w, P + lay.map_b, nullptr, w.wmod, nullptr, B, (int)TE, d.Z, VG_F32_ACT_NONE, VgDrop(), st));
  if (cond) VG_TRY(vg_f32_class_add_launch(w.wmod, cond->table, cond->labels, B, TE, cond->K, st));
  // the learned embedding, broadcast over the batch (generator.py:62)
  VG_TRY(vg_f32_bcast_launch(P + lay.emb, TE, nullptr, w.H, RE, st));

  for (int l = 0; l < L; ++l) {  // TransformerSLN.forward, src/v1/transformer.py:85-88
    const float* Pl = P + lay.layer0 + (long long)l * lay.layer_stride;
    const SlnF n1 = {Pl + lay.sln1_w, Pl + lay.sln1_b, Pl + lay.sln1_s}, n2 = {Pl + lay.sln2_w, Pl + lay.sln2_b, Pl + lay.sln2_s};
    const float* h = w.H + l * RE;
    float *hout = w.H + (l + 1) * RE, *s1 = w.s1 + l * RE, *qkv = w.qkv + 3 * l * RE, *cat = w.cat + l * RE, *htmp = w.htmp + l * RE, *s2 = w.s2 + l * RE;
    float* lse = w.lse + (long long)l * B * d.H * T;
    VG_TRY(vg_f32_sln_fwd_launch(h, 0, w.wmod, n1.w, n1.b, n1.s, n1.s + 1, s1, w.mean1 + (long long)l * R, w.rstd1 + (long long)l * R, R, E, 1e-5f, st));
    VG_TRY(vg_f32_linear_fwd(s1, Pl + lay.wqkv, nullptr, nullptr, qkv, nullptr, R, 3 * E, E, VG_F32_ACT_NONE, VgDrop(), st));
    VG_TRY(vg_f32_attn_fwd_launch(qkv, cat, lse, B, d.H, T, HE, scale, st));
    VG_TRY(vg_f32_linear_fwd(cat, Pl + lay.wo, Pl + lay.bo, h, htmp, nullptr, R, E, E, VG_F32_ACT_NONE, dr.at(100 + 2 * l), st));
    VG_TRY(vg_f32_sln_fwd_launch(htmp, 0, w.wmod, n2.w, n2.b, n2.s, n2.s + 1, s2, w.mean2 + (long long)l * R, w.rstd2 + (long long)l * R, R, E, 1e-5f, st));
    VG_TRY(vg_f32_linear_fwd(s2, Pl + lay.wm, Pl + lay.bm, htmp, hout, nullptr, R, E, E, VG_F32_ACT_NONE, dr.at(101 + 2 * l), st));
  }
  const SlnF nf = {P + lay.slnf_w, P + lay.slnf_b, P + lay.slnf_s};
  VG_TRY(vg_f32_sln_fwd_launch(w.H + L * RE, 0, w.wmod, nf.w, nf.b, nf.s, nf.s + 1, w.sf, w.meanf, w.rstdf, R, E, 1e-5f, st));
  if (net->pos_table) VG_TRY(vg_f32_bcast_launch(net->pos_table, TE, w.sf, w.sf, RE, st));  // constant: the backward is unchanged
  VG_TRY(vg_f32_siren_fwd(w.sf, P + lay.s1_w, P + lay.s1_b, w.y1, w.zf1, R, d.O, E, d.omega0, st));
  float* rows = d.patch > 0 ? w.rows : img;
  VG_TRY(vg_f32_siren_fwd(w.y1, P + lay.s2_w, P + lay.s2_b, rows, w.zf2, R, d.CW, d.O, d.omega0, st));
  if (d.patch > 0) VG_TRY(vg_f32_patchify_launch(img, rows, B, d.C, d.IH, d.patch, 1, st));  // token rows -> NCHW
  return 0;
}

extern "C" int vg_gen_backward_f32(const VgGenNet* net, int B, void* ws, const float* d_img, const VgGenCondF32* cond, void* stream) {
  if (!net || !net->P || !net->G || !ws || !d_img || B < 1) return -1;
  VG_TRY(check_cond(cond, true));
  if (cond && (cond->K < 1 || cond->K > 16)) return -2;
  VgGenLayout lay;
  VG_TRY(check_dims(&net->d, lay));
  const VgGenDims& d = net->d;
  hipStream_t st = (hipStream_t)stream;
  const int E = d.E, T = d.T, R = B * T, L = d.L, HE = E / d.H;
  const long long RE = (long long)R * E, TE = (long long)T * E;
  GenF32Ws w; carve_gen_f32(d, B, ws, w);
  const float* P = net->P;
  float* G = net->G;
  const Drop dr = {net->dropout_p, net->dropout_seed, net->dropout_step};
  const float scale = 1.0f / sqrtf((float)E);

  // SIREN output layers (siren.py:44-45)
  const float* d_rows = d_img;
  if (d.patch > 0) {  // NCHW gradient -> token rows, the adjoint of the forward scatter
    VG_TRY(vg_f32_patchify_launch(d_img, w.drows, B, d.C, d.IH, d.patch, 0, st));
    d_rows = w.drows;
  }
  VG_TRY(vg_f32_sin_grad_launch(d_rows, w.zf2, w.dz2, (long long)R * d.CW, d.omega0, st));
  VG_TRY(vg_f32_linear_wgrad(w.dz2, w.y1, G + lay.s2_w, G + lay.s2_b, w.slab, R, d.CW, d.O, st));
  VG_TRY(vg_f32_siren_dgrad(w.dz2, P + lay.s2_w, w.zf1, w.dz1, R, d.CW, d.O, d.omega0, st));
  VG_TRY(vg_f32_linear_wgrad(w.dz1, w.sf, G + lay.s1_w, G + lay.s1_b, w.slab, R, d.O, E, st));
  VG_TRY(vg_f32_linear_dgrad(w.dz1, P + lay.s1_w, nullptr, w.ds, R, d.O, E, VG_F32_ACT_NONE, st));
  // final SLN: the first use of the modulation vector this backward meets overwrites dw_acc
  int cur = 0;
  {
    const SlnF nf = {P + lay.slnf_w, P + lay.slnf_b, P + lay.slnf_s};
    const SlnG gf = {G + lay.slnf_w, G + lay.slnf_b, G + lay.slnf_s};
    VG_TRY(vg_f32_sln_bwd_launch(w.ds, w.H + L * RE, 0, w.wmod, w.meanf, w.rstdf, nf.w, nf.b, nf.s, nf.s + 1, nullptr, w.g[cur], w.dw_acc, 0, gf.w,
                                 gf.b, gf.s, gf.s + 1, w.part, R, E, st));
  }
  for (int l = L - 1; l >= 0; --l) {
    const float* Pl = P + lay.layer0 + (long long)l * lay.layer_stride;
    float* Gl = G + lay.layer0 + (long long)l * lay.layer_stride;
    const SlnF n1 = {Pl + lay.sln1_w, Pl + lay.sln1_b, Pl + lay.sln1_s}, n2 = {Pl + lay.sln2_w, Pl + lay.sln2_b, Pl + lay.sln2_s};
    const SlnG g1 = {Gl + lay.sln1_w, Gl + lay.sln1_b, Gl + lay.sln1_s}, g2 = {Gl + lay.sln2_w, Gl + lay.sln2_b, Gl + lay.sln2_s};
    const float *h = w.H + l * RE, *s1 = w.s1 + l * RE, *qkv = w.qkv + 3 * l * RE, *cat = w.cat + l * RE, *htmp = w.htmp + l * RE, *s2 = w.s2 + l * RE;
    const float* lse = w.lse + (long long)l * B * d.H * T;
    const float* g = w.g[cur];
    float* gnext = w.g[cur ^ 1];
    // hout = drop(mlp(s2)) + htmp  (transformer.py:87; the MLP is a single Linear, muilti_layer_perceptron.py:37-42)
    const float* gm = g;
    if (dr.on()) { VG_TRY(vg_f32_dropout_launch(g, w.gm, RE, dr.at(101 + 2 * l), st)); gm = w.gm; }
    VG_TRY(vg_f32_linear_wgrad(gm, s2, Gl + lay.wm, Gl + lay.bm, w.slab, R, E, E, st));
    VG_TRY(vg_f32_linear_dgrad(gm, Pl + lay.wm, nullptr, w.ds, R, E, E, VG_F32_ACT_NONE, st));
    VG_TRY(vg_f32_sln_bwd_launch(w.ds, htmp, 0, w.wmod, w.mean2 + (long long)l * R, w.rstd2 + (long long)l * R, n2.w, n2.b, n2.s, n2.s + 1, g, w.gmid,
                                 w.dw_acc, 1, g2.w, g2.b, g2.s, g2.s + 1, w.part, R, E, st));
    // htmp = drop(output_linear(attention(s1))) + h  (transformer.py:86)
    const float* ga = w.gmid;
    if (dr.on()) { VG_TRY(vg_f32_dropout_launch(w.gmid, w.gm, RE, dr.at(100 + 2 * l), st)); ga = w.gm; }
    VG_TRY(vg_f32_linear_wgrad(ga, cat, Gl + lay.wo, Gl + lay.bo, w.slab, R, E, E, st));
    VG_TRY(vg_f32_linear_dgrad(ga, Pl + lay.wo, nullptr, w.dcat, R, E, E, VG_F32_ACT_NONE, st));
    VG_TRY(vg_f32_attn_bwd_launch(qkv, cat, w.dcat, lse, w.dqkv, B, d.H, T, HE, scale, st));
    VG_TRY(vg_f32_linear_wgrad(w.dqkv, s1, Gl + lay.wqkv, nullptr, w.slab, R, 3 * E, E, st));
    VG_TRY(vg_f32_linear_dgrad(w.dqkv, Pl + lay.wqkv, nullptr, w.ds, R, 3 * E, E, VG_F32_ACT_NONE, st));
    VG_TRY(vg_f32_sln_bwd_launch(w.ds, h, 0, w.wmod, w.mean1 + (long long)l * R, w.rstd1 + (long long)l * R, n1.w, n1.b, n1.s, n1.s + 1, w.gmid, gnext,
                                 w.dw_acc, 1, g1.w, g1.b, g1.s, g1.s + 1, w.part, R, E, st));
    cur ^= 1;
  }
  // the learned embedding is broadcast over the batch: its gradient is the batch sum, images in ascending order
  VG_TRY(vg_f32_colsum_launch(w.g[cur], TE, B, w.part, G + lay.emb, (int)TE, nullptr, 0, st));
  // class embedding: row k = the sum of d w over the samples of class k (accumulated, like every gradient)
  if (cond) VG_TRY(vg_class_grad_launch(w.dw_acc, cond->labels, cond->table_grad, B, (int)TE, cond->K, 1, st));
  // mapping Linear: d W = d w^T z, d b = colsum(d w), d w summed in fp32 over the 2L + 1 SLN uses
  return vg_f32_linear_wgrad(w.dw_acc, w.z, G + lay.map_w, G + lay.map_b, w.slab, B, (int)TE, d.Z, st);
}

// ---------------------------------------------------------------------------------------------------------------------
// single operators
extern "C" int vg_sln_f32_fwd(const float* h, int h_bcast_rows, const float* w, const float* lw, const float* lb, const float* gs, const float* bs,
                              float* y, float* mean, float* rstd, int R, int E, float eps, void* stream) {
  return vg_f32_sln_fwd_launch(h, h_bcast_rows, w, lw, lb, gs, bs, y, mean, rstd, R, E, eps, (hipStream_t)stream);
}
extern "C" long long vg_sln_f32_bwd_part_floats(int R, int E) { return vg_f32_sln_part_floats(R, E); }
extern "C" int vg_sln_f32_bwd(const float* dy, const float* h, int h_bcast_rows, const float* w, const float* mean, const float* rstd,
                              const float* lw, const float* lb, const float* gs, const float* bs, const float* gres, float* dh, float* dw_acc,
                              int dw_accumulate, float* dlw, float* dlb, float* dgs, float* dbs, float* part, int R, int E, void* stream) {
  return vg_f32_sln_bwd_launch(dy, h, h_bcast_rows, w, mean, rstd, lw, lb, gs, bs, gres, dh, dw_acc, dw_accumulate, dlw, dlb, dgs, dbs, part, R, E,
                               (hipStream_t)stream);
}
extern "C" int vg_siren_f32_fwd(const float* X, const float* W, const float* bias, float* Y, float* Z, int M, int N, int K, float omega0,
                                void* stream) {
  if (!X || !W || !Y || !Z) return -1;
  if (M < 1 || N < 1 || K < 1) return -2;
  return vg_f32_siren_fwd(X, W, bias, Y, Z, M, N, K, omega0, (hipStream_t)stream);
}
extern "C" int vg_siren_f32_dgrad(const float* dY, const float* W, const float* aux, float* dX, int M, int N, int K, float omega0, void* stream) {
  if (!dY || !aux || !dX) return -1;
  if (M < 1 || N < 1 || (W && K < 1)) return -2;
  if (!W) return vg_f32_sin_grad_launch(dY, aux, dX, (long long)M * N, omega0, (hipStream_t)stream);  // the last layer: elementwise over [M, N]
  return vg_f32_siren_dgrad(dY, W, aux, dX, M, N, K, omega0, (hipStream_t)stream);
}
