// Device helpers shared by the attention kernels (attention.hip: S <= 80; attention_long.hip: 80 < S <= 256).
#pragma once
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
template <int HE, int NW>
__device__ __forceinline__ void dma_head(unsigned char* img, const bf16* __restrict__ src, size_t ld, int S, int rows_alloc,
                                         const void* zeros, int wave, int lane) {
  constexpr int CPR = HE / 8;  // 16-B chunks per row
  const int pieces = rows_alloc * CPR / 64;
  for (int pc = wave; pc < pieces; pc += NW) {
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
