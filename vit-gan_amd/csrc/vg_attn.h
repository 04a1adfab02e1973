// Device helpers shared by the attention kernels (attention.hip: S <= 80; attention_long.hip: 80 < S <= 256).
#pragma once
#include <type_traits>
#include "vg_common.h"

// LDS image of one head: row-major [rows][HE] bf16 whose 16-B chunks are XOR-swizzled by the row so that BOTH
// access patterns are bank-conflict free:
//   row form   (ds_read_b128, 16 lanes = 16 consecutive rows, same chunk)   and
//   transposed (ds_read_b64_tr_b16, 32 lanes = 8 consecutive rows x one 32-B chunk pair).
// HE = 96 / 32 (row pitch 48 / 16 banks: rows r and r+4 share a bank quadrant): position inside each 64-B window
//   is XORed with F[(r>>2)&3], F = {0,2,1,3} - rows r+4 move to the other pair, rows r+8 / r+12 swap halves.
// HE = 64 (pitch 32 banks: rows r and r+2 collide): pair index ^ (r>>1)&3, half ^ (r>>3)&1.
// The map is an involution on the chunk index, so the DMA applies the same function to its SOURCE chunk.
template <int HE>
__device__ __forceinline__ int swz_chunk(int r, int c) {
  if (HE == 64) return (((c >> 1) ^ ((r >> 1) & 3)) << 1) | ((c & 1) ^ ((r >> 3) & 1));
  const int x = (r >> 2) & 3;
  return (c & ~3) | ((c & 3) ^ (((x & 1) << 1) | (x >> 1)));
}
template <int HE>
__device__ __forceinline__ int lds_off(int r, int d) {
  return r * (HE * 2) + (swz_chunk<HE>(r, d >> 3) << 4) + ((d & 7) << 1);
}

// Stage rows [0, rows_alloc) x HE of one head into an LDS image by LDS-DMA (global_load_lds_dwordx4: no trip
// through registers, every request a whole 16-B chunk of a 64..192-B row segment).  One instruction fills
// 1 KiB lane-linearly, so LDS chunk (row r, position c') = linear chunk 64*piece + lane and the XOR swizzle
// (swz_chunk) is applied to the SOURCE chunk index.  Rows >= S come from a 16-byte zero page (the padded keys'
// V rows multiply p = 0 and must be finite).  rows_alloc * HE / 8 must be a multiple of 64.
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
template <int HE>
__device__ __forceinline__ void dma_head(unsigned char* img, const bf16* __restrict__ src, size_t ld, int S, int rows_alloc,
                                         const void* zeros, int wave, int nw, int lane) {  // nw waves share the pieces
  constexpr int CPR = HE / 8;  // 16-B chunks per row
  const int pieces = rows_alloc * CPR / 64;
  for (int pc = wave; pc < pieces; pc += nw) {
    const int ci = 64 * pc + lane;
    const int r = ci / CPR, cp = ci - r * CPR;
    const int c = swz_chunk<HE>(r, cp);
    const void* p = (r < S) ? (const void*)(src + (size_t)r * ld + 8 * c) : zeros;
    __builtin_amdgcn_global_load_lds((gptr_t)p, (lptr_t)(img + 1024 * pc), 16, 0, 0);
  }
}

// Accumulator tiles [dt] (lane = row li, 4 consecutive head-dim columns 16*dt + 4*g ..) -> bf16 row segments.
// v_permlane16_swap between the even and the odd tile of a pair hands every lane 8 CONSECUTIVE columns, so a lane
// stores 16 B and a wave-instruction covers 16 rows x 64 B (same exchange as the GEMM epilogue).
template <int DT>
__device__ __forceinline__ void store_tiles(bf16* __restrict__ rowp, const f32x4 (&acc)[DT], float mul, int g, bool ok) {
#pragma unroll
  for (int pr = 0; pr < DT / 2; ++pr) {
    const f32x4 te = acc[2 * pr], to = acc[2 * pr + 1];
    bf16x8 w;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(te[r] * mul), __float_as_uint(to[r] * mul), false, false);
      w[r] = vg_f2bf(__uint_as_float(sw[0]));
      w[r + 4] = vg_f2bf(__uint_as_float(sw[1]));
    }
    if (ok) *(bf16x8*)(rowp + 32 * pr + ((g & 1) << 4) + ((g & 2) << 2)) = w;
  }
}

// row-form fragment straight from global: rows r0+li, head-dim slice 32*ks + 8*g
__device__ __forceinline__ bf16x8 gfrag(const bf16* __restrict__ src, size_t ld, int r0, int ks, int S, int lane) {
  const int row = r0 + (lane & 15), d = 32 * ks + 8 * (lane >> 4);
  bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  if (row < S) z = *(const bf16x8*)(src + (size_t)row * ld + d);
  return z;
}
template <int HE>
__device__ __forceinline__ bf16x8 lfrag_row(const unsigned char* lds, int r0, int ks, int lane) {
  return *(const bf16x8*)(lds + lds_off<HE>(r0 + (lane & 15), 32 * ks + 8 * (lane >> 4)));
}
// transposed fragment: non-k index = head-dim columns d0..d0+15 (on the lane), k = rows
// (keys or queries) in the accumulator order {32u + 4g + j (j<4), 32u + 16 + 4g + (j-4)}.
template <int HE>
__device__ __forceinline__ bf16x8 lfrag_tr(const unsigned char* lds, int u, int d0, int lane) {
  const int g = lane >> 4, li = lane & 15, q = li >> 2, p = li & 3;
  typedef bf16x4 __attribute__((address_space(3))) * lds4;
  const int r = 32 * u + 4 * g + q;
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds4)(lds + lds_off<HE>(r, d0 + 4 * p)));
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds4)(lds + lds_off<HE>(r + 16, d0 + 4 * p)));
  bf16x8 o;
  o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = lo[3];
  o[4] = hi[0]; o[5] = hi[1]; o[6] = hi[2]; o[7] = hi[3];
  return o;
}
__device__ __forceinline__ bf16x8 pack_pair(f32x4 a, f32x4 b) {
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) { o[j] = vg_f2bf(a[j]); o[j + 4] = vg_f2bf(b[j]); }
  return o;
}
// NT accumulator tiles -> the (NT + 1) / 2 k-operands of an output product.  The odd-tail rule lives in tile_or_zero: an odd tile
// count pairs its last tile with zeros.  pack_tiles_at is pair u alone, for a kernel that packs several tile sets pair by pair.
template <int NT>
__device__ __forceinline__ f32x4 tile_or_zero(const f32x4 (&t)[NT], int i) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  return (i < NT) ? t[(i < NT) ? i : 0] : zero;
}
template <int NT>
__device__ __forceinline__ bf16x8 pack_tiles_at(const f32x4 (&t)[NT], int u) { return pack_pair(t[2 * u], tile_or_zero<NT>(t, 2 * u + 1)); }
template <int NT>
__device__ __forceinline__ void pack_tiles(const f32x4 (&t)[NT], bf16x8 (&f)[(NT + 1) / 2]) {
#pragma unroll
  for (int u = 0; u < (NT + 1) / 2; ++u) f[u] = pack_tiles_at<NT>(t, u);
}
__device__ __forceinline__ float group_sum(float v) {  // over the 4 lane groups (lane>>4)
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}
__device__ __forceinline__ float group_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  v = fmaxf(v, __shfl_xor(v, 32, 64));
  return v;
}

// workgroup -> (image, head).  The heads of one image read interleaved 2 HE-byte slices of the same rows of qkv / o / d_o
// (HE = 96: 192-byte segments, 1.5 cache lines - neighbouring heads share a line), and consecutive workgroup ids go round-robin
// over the 8 XCDs, each with its own L2: the heads of an image therefore sit on ONE XCD, as consecutive workgroups of it
// (id = 8 i + x: image 8 (i / H) + x, head i % H), so a shared line is fetched from HBM once.
__device__ __forceinline__ bool attn_block(int B, int H, int& b, int& h) {
#ifdef VG_ATTN_LINEAR_MAP  // A/B builds: the plain mapping
  b = blockIdx.x / H; h = blockIdx.x - b * H;
#else
  const int x = blockIdx.x & 7, i = blockIdx.x >> 3;
  b = (i / H) * 8 + x; h = i % H;
#endif
  return b < B;
}
static inline int attn_grid(int B, int H) { return ((B + 7) / 8) * 8 * H; }

// One head's slice of the tensors.  qkv-shaped tensors (qkv, dqkv, uqkv) are [B*S, 3E], Q | K | V thirds with head h at columns
// h*HE of each third; o-shaped ones (o, d_o, d_do) are [B*S, E]; lse is [B, H, S].  head_view() addresses them for every kernel
// but the double backward (attention.hip says why).
struct attn_head {
  const bf16 *q, *k, *v;  // row 0 of this head's Q, K, V
  size_t ld;              // row pitch of a qkv-shaped tensor, 3E
  int E;                  // row pitch of an o-shaped tensor
  size_t row0;            // the image's first row, b*S
  int col0;               // the head's first column in Q and in an o-shaped tensor, h*HE
  size_t offl;            // the head's first element of lse
  template <class T> __device__ __forceinline__ T* in_qkv(T* p) const { return p + row0 * ld + col0; }
  template <class T> __device__ __forceinline__ T* in_o(T* p) const { return p + row0 * E + col0; }
  template <class T> __device__ __forceinline__ T* o_row(T* p, int r) const { return p + (row0 + r) * E + col0; }  // row r of the head
  template <class T> __device__ __forceinline__ T* in_lse(T* p) const { return p + offl; }
};
__device__ __forceinline__ attn_head head_view(const bf16* __restrict__ qkv, int b, int h, int S, int H, int HE) {
  attn_head hd;
  hd.E = H * HE;
  hd.ld = 3 * (size_t)hd.E;
  hd.row0 = (size_t)b * S;
  hd.col0 = h * HE;
  hd.offl = ((size_t)b * H + h) * S;
  hd.q = hd.in_qkv(qkv);
  hd.k = hd.q + hd.E;
  hd.v = hd.q + 2 * hd.E;
  return hd;
}

// Head-dim dispatch of every attention launcher: f(std::integral_constant<int, HE>) for HE in {96, 64, 32}, -3 otherwise.
template <class F>
static inline int attn_by_head_dim(int HE, F&& f) {
  if (HE == 96) return f(std::integral_constant<int, 96>{});
  if (HE == 64) return f(std::integral_constant<int, 64>{});
  if (HE == 32) return f(std::integral_constant<int, 32>{});
  return -3;
}

// ---- fp8 (OCP e4m3) operands for the activation-side products (config C5: "fp8 MFMA attention") ------------------------
// An fp8 16x16x32 fragment is 8 bytes per lane, element j of lane group g pairing with element j of the other operand's
// lane group g exactly like the bf16 fragment's 8 elements - so a bf16 fragment converts element by element.
typedef long fp8x8;
__device__ __forceinline__ fp8x8 to_fp8(float a0, float a1, float a2, float a3, float a4, float a5, float a6, float a7) {
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(a0, a1, lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(a2, a3, lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(a4, a5, hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(a6, a7, hi, true);
  return (fp8x8)(((unsigned long)(unsigned)hi << 32) | (unsigned long)(unsigned)lo);
}
__device__ __forceinline__ fp8x8 to_fp8(bf16x8 v) {
  return to_fp8(vg_bf2f(v[0]), vg_bf2f(v[1]), vg_bf2f(v[2]), vg_bf2f(v[3]), vg_bf2f(v[4]), vg_bf2f(v[5]), vg_bf2f(v[6]), vg_bf2f(v[7]));
}
__device__ __forceinline__ fp8x8 pack_pair_fp8(f32x4 a, f32x4 b, float mul) {  // same element order as pack_pair
  return to_fp8(a[0] * mul, a[1] * mul, a[2] * mul, a[3] * mul, b[0] * mul, b[1] * mul, b[2] * mul, b[3] * mul);
}
__device__ __forceinline__ f32x4 vg_mfma_fp8(fp8x8 a, fp8x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, c, 0, 0, 0); }
// score product with either operand type (FP8: both operands rounded to e4m3; accumulation stays fp32)
template <bool FP8>
__device__ __forceinline__ f32x4 score_mfma(bf16x8 a, bf16x8 b, f32x4 c) {
  if constexpr (FP8) return vg_mfma_fp8(to_fp8(a), to_fp8(b), c);
  else return vg_mfma(a, b, c);
}
#define VG_P_FP8_SCALE 256.0f  // softmax numerators in (0, 1] are scaled into e4m3's normal range before the P.V product

// squared L2 norm of every row of an LDS head image -> out[rows] (rows >= S are zero rows).  One thread per row.
template <int HE>
__device__ __forceinline__ void row_sqnorms(const unsigned char* img, float* out, int rows, int tid, int nthreads) {
  for (int r = tid; r < rows; r += nthreads) {
    float a = 0.f;
#pragma unroll
    for (int c = 0; c < HE / 8; ++c) {
      const bf16x8 v = *(const bf16x8*)(img + lds_off<HE>(r, 8 * c));
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float f = vg_bf2f(v[j]); a += f * f; }
    }
    out[r] = a;
  }
}
// v1 attention score (src/v1/attention.py:66-67): the Euclidean distance |q - k| from q.k and the squared norms
__device__ __forceinline__ float l2_dist(float qk, float qn, float kn) { return sqrtf(fmaxf(qn + kn - 2.f * qk, 0.f)); }

// ---- the first-order backward, written once ---------------------------------------------------------------------------
// delta of the 16 rows whose dO and O fragments this wave holds: sum_d dO*O, complete in every lane group
template <int KS>
__device__ __forceinline__ float row_delta(const bf16x8 (&dof)[KS], const bf16x8 (&of)[KS]) {
  float dpart = 0.f;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int j = 0; j < 8; ++j) dpart += vg_bf2f(dof[ks][j]) * vg_bf2f(of[ks][j]);
  return group_sum(dpart);
}

// The two recompute tiles.  Both rebuild a 16 x 16 tile of P = exp(score * scale - lse) and return dS = P (dP - delta) * scale;
// L2: the score is the distance and the tile holds W = dS / dist (0 where dist = 0), which is also added to wsum.
// FP8: the score product takes the forward's e4m3 operands (so P matches the forward's lse); dP stays bf16.
// Query side (S^T orientation): lane = query (qf / dof are its tile's fragments, lse_q / delta / qn its row's values), rows = the
// 4 consecutive keys key0 + 4g + r of the K / V images.
template <int HE, bool L2, bool FP8>
__device__ __forceinline__ f32x4 bwd_tile_q(const unsigned char* lk, const unsigned char* lv, int key0, const bf16x8 (&qf)[HE / 32],
                                            const bf16x8 (&dof)[HE / 32], float lse_q, float delta, float qn, const float* kn_l, bool q_ok,
                                            int S, float scale, float& wsum, int lane) {
  const int g = lane >> 4;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 st = zero, dpt = zero;
#pragma unroll
  for (int ks = 0; ks < HE / 32; ++ks) {
    st = score_mfma<FP8>(lfrag_row<HE>(lk, key0, ks, lane), qf[ks], st);
    dpt = vg_mfma(lfrag_row<HE>(lv, key0, ks, lane), dof[ks], dpt);
  }
  f32x4 kn4 = zero;
  if (L2) kn4 = *(const f32x4*)(kn_l + key0 + 4 * g);
  f32x4 ds;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int key = key0 + 4 * g + r;
    const float raw = L2 ? l2_dist(st[r], qn, kn4[r]) : st[r];
    const float p = (key < S && q_ok) ? __expf(raw * scale - lse_q) : 0.f;
    float dsv = p * (dpt[r] - delta) * scale;
    if (L2) { dsv = raw > 0.f ? dsv / raw : 0.f; wsum += dsv; }  // d dist/dq = (q - k)/dist
    ds[r] = dsv;
  }
  return ds;
}
// Key side (S orientation): lane = key (kf / vf are its tile's fragments, kn its row's norm), rows = the 4 consecutive queries
// q0 + 4g + r of the Q / dO images, whose lse / delta / norm come from the per-query arrays ll / dl / qn_l.
template <int HE, bool L2, bool FP8>
__device__ __forceinline__ void bwd_tile_k(const unsigned char* lq, const unsigned char* ldo, int q0, const bf16x8 (&kf)[HE / 32],
                                           const bf16x8 (&vf)[HE / 32], const float* ll, const float* dl, const float* qn_l, float kn,
                                           bool key_ok, int S, float scale, float& wsum, int lane, f32x4& pr, f32x4& ds) {
  const int g = lane >> 4;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 s = zero, dp = zero;
#pragma unroll
  for (int ks = 0; ks < HE / 32; ++ks) {
    s = score_mfma<FP8>(lfrag_row<HE>(lq, q0, ks, lane), kf[ks], s);
    dp = vg_mfma(lfrag_row<HE>(ldo, q0, ks, lane), vf[ks], dp);
  }
  const f32x4 lq4 = *(const f32x4*)(ll + q0 + 4 * g);
  const f32x4 dl4 = *(const f32x4*)(dl + q0 + 4 * g);
  f32x4 qn4 = zero;
  if (L2) qn4 = *(const f32x4*)(qn_l + q0 + 4 * g);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = q0 + 4 * g + r;
    const bool ok = (q < S) && key_ok;
    const float raw = L2 ? l2_dist(s[r], qn4[r], kn) : s[r];
    const float p = ok ? __expf(raw * scale - lq4[r]) : 0.f;
    pr[r] = p;
    float dsv = p * (dp[r] - dl4[r]) * scale;
    if (L2) { dsv = raw > 0.f ? dsv / raw : 0.f; wsum += dsv; }  // d dist/dk = (k - q)/dist
    ds[r] = dsv;
  }
}

// Per-query / per-key rows the phases read from LDS: delta and lse of every query; L2 scores: |q|^2 and |k|^2 (else unused)
struct bwd_rows { const float *dl, *ll, *qn_l, *kn_l; };

// The two phases of the short backward (S <= 16 NT: the whole S x S tile in accumulators, wave wv owns tile wv).  Both kernels of
// attention.hip are stagings of these two calls.  The outputs are accumulated two head-dim tiles (32 columns = one 16-byte store
// per lane) per pass, for registers; per output element the MFMAs and their order are those of accumulating all tiles at once.
// Phase A, S^T orientation (lane = query): K / V images and this wave's Q / dO fragments in, dQ rows out.
// L2: dQ = rowsum(W) q - W K, the q row read from the image lq.
template <int HE, int NT, bool L2, bool FP8>
__device__ __forceinline__ void bwd_phase_a(const unsigned char* lk, const unsigned char* lv, const unsigned char* lq,
                                            const bf16x8 (&qf)[HE / 32], const bf16x8 (&dof)[HE / 32], const bwd_rows& rw, bf16* dqb,
                                            size_t ld, int S, float scale, int wv, int lane) {
  constexpr int DT = HE / 16, KP = (NT + 1) / 2, PW = 2;
  const int g = lane >> 4, q = 16 * wv + (lane & 15);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const float delta = rw.dl[q];
  const float lse_q = rw.ll[q];
  const float qn = L2 ? rw.qn_l[q] : 0.f;
  float wsum = 0.f;  // L2: sum_k W[q,k], W = dL/d dist / dist
  f32x4 ds[NT];
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) ds[kt] = bwd_tile_q<HE, L2, FP8>(lk, lv, 16 * kt, qf, dof, lse_q, delta, qn, rw.kn_l, q < S, S, scale, wsum, lane);
  if (L2) wsum = group_sum(wsum);
  bf16x8 dsf[KP];
  pack_tiles<NT>(ds, dsf);
  bf16* rowq = dqb + (size_t)(q < S ? q : 0) * ld;
#pragma unroll
  for (int pp = 0; pp < DT / PW; ++pp) {
    f32x4 dq[PW];
#pragma unroll
    for (int t = 0; t < PW; ++t) dq[t] = zero;
#pragma unroll
    for (int u = 0; u < KP; ++u)
#pragma unroll
      for (int t = 0; t < PW; ++t) dq[t] = vg_mfma(lfrag_tr<HE>(lk, u, 16 * (PW * pp + t), lane), dsf[u], dq[t]);
    if (L2) {
#pragma unroll
      for (int t = 0; t < PW; ++t) {
        const bf16x4 qv = *(const bf16x4*)(lq + lds_off<HE>(q, 16 * (PW * pp + t) + 4 * g));
#pragma unroll
        for (int r = 0; r < 4; ++r) dq[t][r] = wsum * vg_bf2f(qv[r]) - dq[t][r];
      }
    }
    store_tiles<PW>(rowq + 16 * PW * pp, dq, 1.0f, g, q < S);
  }
}
// Phase B, S orientation (lane = key): Q / dO images and this wave's K / V fragments in, dK and dV rows out.
// L2: dK = colsum(W) k - W^T Q, the k row read from the image lk.
template <int HE, int NT, bool L2, bool FP8>
__device__ __forceinline__ void bwd_phase_b(const unsigned char* lq, const unsigned char* ldo, const unsigned char* lk,
                                            const bf16x8 (&kf)[HE / 32], const bf16x8 (&vf)[HE / 32], const bwd_rows& rw, bf16* dqb,
                                            size_t ld, int E, int S, float scale, int wv, int lane) {
  constexpr int DT = HE / 16, KP = (NT + 1) / 2, PW = 2;
  const int g = lane >> 4, key = 16 * wv + (lane & 15);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const float kn = L2 ? rw.kn_l[key] : 0.f;
  float wsum = 0.f;  // L2: sum_q W[q,key]
  f32x4 pr[NT], ds[NT];
#pragma unroll
  for (int qt = 0; qt < NT; ++qt) bwd_tile_k<HE, L2, FP8>(lq, ldo, 16 * qt, kf, vf, rw.ll, rw.dl, rw.qn_l, kn, key < S, S, scale, wsum, lane, pr[qt], ds[qt]);
  if (L2) wsum = group_sum(wsum);
  bf16x8 pf[KP], dsf[KP];
  pack_tiles<NT>(pr, pf);
  pack_tiles<NT>(ds, dsf);
  bf16* rowp = dqb + (size_t)(key < S ? key : 0) * ld;
#pragma unroll
  for (int pp = 0; pp < DT / PW; ++pp) {
    f32x4 dv[PW], dk[PW];
#pragma unroll
    for (int t = 0; t < PW; ++t) { dv[t] = zero; dk[t] = zero; }
#pragma unroll
    for (int u = 0; u < KP; ++u)
#pragma unroll
      for (int t = 0; t < PW; ++t) {
        dv[t] = vg_mfma(lfrag_tr<HE>(ldo, u, 16 * (PW * pp + t), lane), pf[u], dv[t]);
        dk[t] = vg_mfma(lfrag_tr<HE>(lq, u, 16 * (PW * pp + t), lane), dsf[u], dk[t]);
      }
    if (L2) {
#pragma unroll
      for (int t = 0; t < PW; ++t) {
        const bf16x4 kv = *(const bf16x4*)(lk + lds_off<HE>(key, 16 * (PW * pp + t) + 4 * g));
#pragma unroll
        for (int r = 0; r < 4; ++r) dk[t][r] = wsum * vg_bf2f(kv[r]) - dk[t][r];
      }
    }
    store_tiles<PW>(rowp + E + 16 * PW * pp, dk, 1.0f, g, key < S);
    store_tiles<PW>(rowp + 2 * E + 16 * PW * pp, dv, 1.0f, g, key < S);
  }
}
