// A device-resident dataset: the step's real batch drawn, decoded and labelled on the device, gfx950.
//
// vg_dataset_fetch (include/vitgan_hip.h holds the definition a test restates): image n of the launch is the dataset's image
// idx = perm_epoch(p), p its position in the epoch, epoch and p functions of the device step counter alone - a replayed hipGraph
// fetches a fresh batch with nothing from the host.  perm_epoch is a 4-round Feistel network on 2k bits, cycle-walked into [0, N):
// no table, no state, a handful of hashes per image, and every value in it is blockIdx-wide (the workgroup is the image), so the walk
// is uniform across the workgroup.  The decode is a table lookup: lut[c][byte] is bf16(((byte / 255) - mean[c]) / std[c]) as torch's
// fp32 computes it, built on the host once, so the batch is bit for bit what ToTensor, Normalize and the step's bf16 cast deliver.
//
// One workgroup per output image.  The source image (C*IH*IH bytes, either layout) and the table (C * 512 bytes) are staged in LDS with
// 16-byte global loads; behind one barrier every thread emits runs of 8 consecutive pixels of one output plane - 8 byte reads and 8
// table reads from LDS, one 16-byte store.  The flip and the channels-last layout only change the LDS address of a byte, never a
// global access.  Bytes per image: C*IH*IH in, 2*C*IH*IH out, no reduction, no scratch.
#include "../../include/vitgan_hip.h"
#include "vg_common.h"
#include "vg_kernels.h"

namespace {

#define VG_DATA_LDS_MAX (160 * 1024)  // one CU's LDS on gfx950
#define VG_DATA_SITE_PERM 4           // the engine's site numbering: 0-2 the augmentations, 3 the fake labels
#define VG_DATA_SITE_FLIP 5

struct VgFetch {
  uint32_t N, nb, B, rank, world, k;  // k: half the Feistel width
  uint32_t key_perm, key_flip;        // h(Kp, 0), h(Kf, 0): the epoch is mixed in on the device
  int C, IH, layout, flags;
};

// the keyed bijection of [0, N): one Feistel pass permutes [0, 2^2k), the walk follows p's cycle until it is back inside [0, N)
__device__ __forceinline__ uint32_t vg_perm_epoch(uint32_t p, uint32_t N, uint32_t k, uint32_t ke) {
  const uint32_t m = (1u << k) - 1u;
  uint32_t key[4];
#pragma unroll
  for (uint32_t r = 0; r < 4; ++r) key[r] = vg_drop_word(ke, r + 1u);
  uint32_t x = p;
  do {
    uint32_t L = x >> k, R = x & m;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t t = L ^ (vg_drop_word(key[r], R) & m);
      L = R;
      R = t;
    }
    x = (L << k) | R;
  } while (x >= N);
  return x;
}

__global__ __launch_bounds__(1024) void vg_dataset_fetch_kernel(const unsigned char* __restrict__ images, const int* __restrict__ labels,
                                                                const uint16_t* __restrict__ lut, uint16_t* __restrict__ imgs,
                                                                int* __restrict__ labels_out, int* __restrict__ index_out, VgFetch a,
                                                                const unsigned* __restrict__ dstep) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  const int n = blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
  const int C = a.C, IH = a.IH, HW = IH * IH, per = C * HW;
  uint16_t* tab = reinterpret_cast<uint16_t*>(sm);  // [C][256]
  unsigned char* src = sm + C * 512;                // the source image as it lies in memory
  // which image: everything here is a function of the counter and blockIdx
  const uint32_t s = dstep[0];
  const uint32_t epoch = s / a.nb, j = s - epoch * a.nb;
  const uint32_t p = (j * a.world + a.rank) * a.B + (uint32_t)n;  // < nb world B <= N
  const uint32_t idx = (a.flags & 1) ? vg_perm_epoch(p, a.N, a.k, vg_drop_word(a.key_perm, epoch)) : p;
  const bool flip = (a.flags & 2) && (vg_drop_word(vg_drop_word(a.key_flip, epoch), p) >> 31);

  const u32x4* __restrict__ g = reinterpret_cast<const u32x4*>(images + (size_t)idx * (size_t)per);
  for (int i = tid; i < (per >> 4); i += NT) reinterpret_cast<u32x4*>(src)[i] = g[i];
  for (int i = tid; i < C * 32; i += NT) reinterpret_cast<u32x4*>(tab)[i] = reinterpret_cast<const u32x4*>(lut)[i];
  if (tid == 0) {
    if (labels_out) labels_out[n] = labels[idx];
    if (index_out) index_out[n] = (int)idx;
  }
  __syncthreads();

  const int cpp = HW >> 3;  // runs of 8 pixels per plane
  uint16_t* __restrict__ out = imgs + (size_t)n * (size_t)per;
  for (int ch = tid; ch < C * cpp; ch += NT) {
    const int c = ch / cpp, q = (ch - c * cpp) << 3;
    int y = q / IH, x = q - y * IH;
    const uint16_t* __restrict__ tc = tab + c * 256;
    uint16_t r[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int xs = flip ? IH - 1 - x : x;
      const int off = a.layout ? (y * IH + xs) * C + c : c * HW + y * IH + xs;
      r[e] = tc[src[off]];
      if (++x == IH) { x = 0; ++y; }
    }
    u32x4 w;
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = (uint32_t)r[2 * e] | ((uint32_t)r[2 * e + 1] << 16);
    *reinterpret_cast<u32x4*>(out + ((size_t)ch << 3)) = w;  // plane c, pixel q: c HW + q = 8 ch
  }
}

inline bool misaligned16(const void* p) { return ((uintptr_t)p & 15u) != 0; }

}  // namespace

extern "C" int vg_dataset_fetch(const unsigned char* images, const int* labels, long long N, int C, int IH, int layout, const void* lut,
                                void* imgs, int* labels_out, int* index_out, int B, int rank, int world, int flags,
                                unsigned long long seed, const int* step_dev, void* stream) {
  if (!images || !lut || !imgs || !step_dev || (labels_out && !labels) || N < 1 || C < 1 || IH < 1 || B < 1) return -1;
  if (world < 1 || rank < 0 || rank >= world || (layout != 0 && layout != 1) || flags < 0 || flags > 3) return -2;
  if (N >= (1ll << 31) || (long long)B * world > N) return -2;
  const long long HW = (long long)IH * IH, per = (long long)C * HW;
  const long long lds = per + (long long)C * 512;
  if (C > 4 || (HW & 7) || (per & 15) || lds > VG_DATA_LDS_MAX) return -3;
  if (misaligned16(images) || misaligned16(lut) || misaligned16(imgs)) return -3;
  VgFetch a;
  a.N = (uint32_t)N; a.B = (uint32_t)B; a.rank = (uint32_t)rank; a.world = (uint32_t)world;
  a.nb = (uint32_t)(N / ((long long)B * world));
  uint32_t bits = 0;  // bitlength(N - 1)
  for (uint32_t v = (uint32_t)(N - 1); v; v >>= 1) ++bits;
  a.k = bits < 2 ? 1u : (bits + 1u) >> 1;
  auto h0 = [](uint32_t key) {  // vg_drop_word(key, 0) on the host
    uint32_t x = key;
    x ^= x >> 16; x *= 0x7FEB352Du;
    x ^= x >> 15; x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
  };
  a.key_perm = h0(vg_site_key(seed, VG_DATA_SITE_PERM));
  a.key_flip = h0(vg_site_key(seed, VG_DATA_SITE_FLIP));
  a.C = C; a.IH = IH; a.layout = layout; a.flags = flags;
  // dynamic LDS above 64 KiB (3 x 224 x 224: 148.5 KiB): the kernel's limit is raised to what the largest geometry seen so far needs
  static long long allowed = 64 * 1024;
  if (lds > allowed) {
    VG_CHECK_HIP(hipFuncSetAttribute((const void*)vg_dataset_fetch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    allowed = lds;
  }
  const long long runs = per >> 3;
  const int nt = runs >= 1024 ? 1024 : (int)((runs + 63) >> 6) << 6;
  hipLaunchKernelGGL(vg_dataset_fetch_kernel, dim3(B), dim3(nt < 64 ? 64 : nt), (size_t)lds, (hipStream_t)stream, images, labels,
                     (const uint16_t*)lut, (uint16_t*)imgs, labels_out, index_out, a, (const unsigned*)step_dev);
  return (int)hipGetLastError();
}
