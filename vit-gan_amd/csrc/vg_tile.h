// Tile layouts of the bf16 MFMA GEMM family (gemm.hip, gemm_wr.hip, gemm_tn.hip, gemm_row.hip, chain.hip): the ONE definition of
// every rule a stager, a fragment reader, a packer and an epilogue have to agree on.  A swizzle that drifts between two of them
// does not fail loudly, it produces wrong tiles.  Integer and bit-move helpers only: the files compiled with floating-point
// contraction off include this header too, and no floating-point expression may cross a contraction setting.  (The register
// epilogue, which does arithmetic, is vg_epilogue.h.)
//
// The MFMA is issued "swapped": its A operand carries the GEMM's n index and its B operand the m index, so a lane's 4
// accumulator registers are 4 CONSECUTIVE n of one output row m (lane = 16 g + li: row li, columns 4 g .. 4 g + 3 of a 16 x 16 tile).
//
// Operand images in LDS.  They are filled by LDS-DMA (global_load_lds_dwordx4: 64 lanes x 16 B = 1 KiB per wave-instruction),
// whose LDS destination is wave-uniform base + lane*16: the images are lane-linear per 1-KiB piece and the XOR swizzles
// below are applied to the per-lane SOURCE address.
//   row form  [rows][32 k]  (64-B rows): 16-B chunk c of row r lives at chunk c ^ vg_row_swz(r).
//   tr  form  [32 k][128 cols]  (256-B rows, 8 KiB per image): 16-B chunk c of row k lives at c ^ (2*vg_tr_sigma(k)).
#pragma once
#include "vg_gemm.h"

typedef const __attribute__((address_space(1))) void* vg_gptr_t;  // the operand types of __builtin_amdgcn_global_load_lds
typedef __attribute__((address_space(3))) void* vg_lptr_t;

// row-form chunk swizzle {0,2,3,1}[(r>>2)&3]: the four 16-lane groups of a ds_read_b128 then each cover all 16 slots of a
// 256-B bank row (conflict-free).  Host too: the weight packer of gemm_row.hip writes images in this form.
__host__ __device__ __forceinline__ int vg_row_swz(int r) { return (0x78 >> (2 * ((r >> 2) & 3))) & 3; }

// tr-form row permutation: with chunk c of row k at c ^ (2*sigma(k)), the 32-lane halves of a ds_read_b64_tr_b16 touch all 64
// banks exactly once.
__device__ __forceinline__ int vg_tr_sigma(int kk) { return (kk & 3) | (((kk >> 3) & 1) << 2); }

// tr-form fragment address: byte offset, inside a set of consecutive [32 k][128 cols] images, of the lane's part of the MFMA
// fragment of columns col0 .. col0 + 15 (col0 a multiple of 16; col0 >> 7 selects the image).  The lane reads k rows
// 8 g + q (this address) and + 4 (at + 1024) with two ds_read_b64_tr_b16, each 4 columns = half a 16-B chunk.
__device__ __forceinline__ unsigned vg_tr_frag_off(int col0, int lane) {
  // sw = 2*vg_tr_sigma(kk0), spelled on g and q: through the function the compiler shares less of it with the stager's use of
  // the lane, and the tiled NN kernel's loop moves by 12 bytes (profiles/gemm_tile_header.txt)
  const int g = lane >> 4, li = lane & 15, q = li >> 2, p = li & 3, sw = 2 * (q | ((g & 1) << 2)), kk0 = 8 * g + q;
  const int c8 = ((col0 & 127) >> 2) + p;
  return (unsigned)((col0 >> 7) * 8192 + kk0 * 256 + (((c8 >> 1) ^ sw) << 4) + ((c8 & 1) << 3));
}

// what a ds_read_b128 / a pair of ds_read_b64_tr_b16 returned, as an MFMA operand
__device__ __forceinline__ bf16x8 vg_frag(u32x4 v) { return __builtin_bit_cast(bf16x8, v); }
__device__ __forceinline__ bf16x8 vg_frag(u32x2 lo, u32x2 hi) { return __builtin_bit_cast(bf16x8, (u32x4){lo[0], lo[1], hi[0], hi[1]}); }

// Register epilogues: a lane holds, per (n-tile, m-tile), 4 consecutive n of row li.  v_permlane16_swap between the even (te)
// and the odd (to) n-tile of a pair - rows 1,3 of the even tile's register <-> rows 0,2 of the odd tile's - hands every lane
// 8 CONSECUTIVE n of one tile (even lane-groups keep the even tile, odd lane-groups the odd one): lo = the first 4, hi = the
// next 4, so a lane loads / stores 16 B (bf16) or 32 B (fp32) per slot with no trip through LDS.
__device__ __forceinline__ void vg_pair_swap(f32x4 te, f32x4 to, f32x4& lo, f32x4& hi) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(te[r]), __float_as_uint(to[r]), false, false);
    lo[r] = __uint_as_float(sw[0]);
    hi[r] = __uint_as_float(sw[1]);
  }
}
// first of those 8 columns inside the pair's 32, for lane group g = lane >> 4: {0,16,8,24}[g].
// A macro (g is evaluated twice: pass a variable), so that the expression meets the `lane >> 4` it is applied to.  Every function
// form tried - __forceinline__, constexpr __forceinline__, a reference parameter, `|` for `+`, masks after the shifts - comes out
// of the compiler as a 5-bit bit reversal, and chain.hip's forward kernel then needs two more registers than it has; as a table in
// a constant it costs the tiled kernel a literal (profiles/gemm_tile_header.txt).
#define vg_pair_col(g) ((((g) & 1) << 4) + (((g) & 2) << 2))

// XCD-aware block order: blocks b, b+8, ... share an XCD (L2); give each XCD a contiguous run of tiles so the n-tiles of one
// m-panel (the tiles of one K slice) hit the same L2.  Bijective for any grid size.
__device__ __forceinline__ int vg_xcd_order(int block, int nblocks) {
  const int xcd = block & 7, q = nblocks >> 3, r = nblocks & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (block >> 3);
}

// tile of a grouped launch -> (problem, origin, K slice); bm x bn is the launch's tile size
struct VgTile { int pi, m0, n0, tn, split, k_begin, k_end; };
__device__ __forceinline__ VgTile vg_locate(const VgGemmGroup& grp, int bid, int bm, int bn) {
  VgTile t;
  t.pi = 0;
#pragma unroll
  for (int i = 1; i < VG_MAX_GROUP; ++i)
    if (i < grp.n && bid >= grp.p[i].tile_start) t.pi = i;
  const VgGemmProb& Q = grp.p[t.pi];
  const int local = bid - Q.tile_start;
  const int tiles_mn = Q.tiles_m * Q.tiles_n;
  t.split = local / tiles_mn;
  const int r = local - t.split * tiles_mn;
  const int tm = r / Q.tiles_n;
  t.tn = r - tm * Q.tiles_n;
  t.m0 = tm * bm; t.n0 = t.tn * bn;
  t.k_begin = t.split * Q.k_per_split;
  t.k_end = min(Q.K, t.k_begin + Q.k_per_split);
  return t;
}

// Host: the K slices of problem p (p.splits requested, p.tiles_m / p.tiles_n set) in stages of bk, and its place in the
// launch's tile numbering - the fields vg_locate reads.  Lowers p.splits where slices would be empty.
inline void vg_plan_splits(VgGemmProb& p, int bk, int* total) {
  const int want = p.splits > 0 ? p.splits : 1;
  const int ksteps = (p.K + bk - 1) / bk;
  const int per = (ksteps + want - 1) / want;
  p.k_per_split = per * bk;
  p.splits = (ksteps + per - 1) / per;  // drop empty slices
  p.tile_start = *total;
  *total += p.tiles_m * p.tiles_n * p.splits;
}
