// Bag feed on the device (include/mmf_amil.h: mmf_bag_gather): the G bags of a grouped window, each contiguous somewhere
// in HBM (feed.ResidentBagCache's arena), into the contiguous rows of the window's [sum N x L] matrix, every plane in ONE
// launch, converting fp32 <-> bf16 storage on the way.  Pure data movement: no LDS, no barrier, no atomics, no workgroup
// waits for another.
#include <cstdint>

#include "../../include/mmf_amil.h"
#include "mmf_common.h"
#include "mmf_kernels.h"

namespace mmf {

constexpr int GATHER_PLANES = 4;
constexpr int GATHER_THREADS = 256;
constexpr int GATHER_UNROLL = 4;     // independent 16-byte (fp32 source of a converting copy: 32-byte) loads per lane before the first store

// By value in the kernel arguments (as SegTable is): a call allocates nothing and copies nothing to the device.
struct GatherTable {
  int G;
  int cbeg[GROUP_MAX + 1];                        // bag g is workgroups cbeg[g] .. cbeg[g + 1] - 1 of a plane (chunks never straddle a bag)
  int64_t off[GROUP_MAX + 1];                     // destination rows of bag g: off[g] .. off[g + 1] - 1
  const void* src[GATHER_PLANES * GROUP_MAX];     // plane-major: src[plane * G + g]
  void* dst[GATHER_PLANES];
};

__device__ inline uint32_t narrow2(uint32_t lo, uint32_t hi) {
  // fp32 bits -> bf16 bits, round to nearest even in integer arithmetic (exact for denormals whatever the float mode;
  // +-inf and the largest finite value come out right by the carry); a NaN becomes the quiet NaN of its sign
  auto one = [](uint32_t u) -> uint32_t {
    const uint32_t r = (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
    return (u & 0x7FFFFFFFu) > 0x7F800000u ? ((u >> 16) | 0x7FC0u) : r;
  };
  return one(lo) | (one(hi) << 16);
}

template <bool SRC_BF16, bool DST_BF16, bool GUARD>
__device__ __forceinline__ void gather_tile(const uint4* __restrict__ s, uint4* __restrict__ d, int64_t base, int64_t u1) {
  constexpr int E = (SRC_BF16 || DST_BF16) ? 8 : 4;
  constexpr int SV = E * (SRC_BF16 ? 2 : 4) / 16, DV = E * (DST_BF16 ? 2 : 4) / 16;      // uint4 per unit on each side
  uint4 v[GATHER_UNROLL][SV];
#pragma unroll
  for (int k = 0; k < GATHER_UNROLL; ++k) {
    const int64_t u = base + (int64_t)k * GATHER_THREADS;
    if (!GUARD || u < u1) {
#pragma unroll
      for (int j = 0; j < SV; ++j) v[k][j] = s[u * SV + j];
    }
  }
#pragma unroll
  for (int k = 0; k < GATHER_UNROLL; ++k) {
    const int64_t u = base + (int64_t)k * GATHER_THREADS;
    if (!GUARD || u < u1) {
      if constexpr (SRC_BF16 == DST_BF16) {
        d[u] = v[k][0];
      } else if constexpr (DST_BF16) {                           // narrow: 8 fp32 -> 8 bf16
        const uint4 a = v[k][0], c = v[k][SV - 1];
        d[u] = make_uint4(narrow2(a.x, a.y), narrow2(a.z, a.w), narrow2(c.x, c.y), narrow2(c.z, c.w));
      } else {                                                   // widen: exact
        const uint4 a = v[k][0];
        d[u * DV] = make_uint4(a.x << 16, a.x & 0xFFFF0000u, a.y << 16, a.y & 0xFFFF0000u);
        d[u * DV + DV - 1] = make_uint4(a.z << 16, a.z & 0xFFFF0000u, a.w << 16, a.w & 0xFFFF0000u);
      }
    }
  }
}

template <bool SRC_BF16, bool DST_BF16>
__global__ __launch_bounds__(GATHER_THREADS) void bag_gather_kernel(const GatherTable t, const int L, const int chunk) {
  // one "unit" = E elements: 16 bytes of the narrower storage type on both sides of a plain copy, 16 + 32 of a conversion
  constexpr int E = (SRC_BF16 || DST_BF16) ? 8 : 4;
  constexpr int DB = DST_BF16 ? 2 : 4;
  const int b = blockIdx.x, plane = blockIdx.y;
  int lo = 0, hi = t.G;                                          // wave-uniform: the table is read with scalar loads
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (t.cbeg[mid] <= b) lo = mid; else hi = mid;
  }
  const int g = lo;
  const int64_t units = (t.off[g + 1] - t.off[g]) * (int64_t)(L / E);
  const int64_t u0 = (int64_t)(b - t.cbeg[g]) * chunk;
  const int64_t u1 = u0 + chunk < units ? u0 + chunk : units;
  const uint4* __restrict__ s = static_cast<const uint4*>(t.src[plane * t.G + g]);
  uint4* __restrict__ d = reinterpret_cast<uint4*>(static_cast<char*>(t.dst[plane]) + t.off[g] * (int64_t)L * DB);
  // full tiles (GATHER_THREADS x GATHER_UNROLL units, a wave-uniform test) issue every load before the first store;
  // only a bag's last tile pays for per-lane guards
  constexpr int64_t TILE = (int64_t)GATHER_THREADS * GATHER_UNROLL;
  for (int64_t tile = u0; tile < u1; tile += TILE) {
    const int64_t base = tile + threadIdx.x;
    if (tile + TILE <= u1) gather_tile<SRC_BF16, DST_BF16, false>(s, d, base, u1);
    else gather_tile<SRC_BF16, DST_BF16, true>(s, d, base, u1);
  }
}

}  // namespace mmf

using namespace mmf;

extern "C" int mmf_bag_gather(const int64_t* offsets, int32_t G, int32_t nplane, const void* const* src, void* const* dst,
                              int32_t L, int32_t src_bf16, int32_t dst_bf16, void* stream) {
  if (!offsets || !src || !dst) return MMF_ERR_ARG;
  if (G < 1 || G > GROUP_MAX || nplane < 1 || nplane > GATHER_PLANES) return MMF_ERR_SHAPE;
  if (L < 8 || L % 8 != 0) return MMF_ERR_SHAPE;
  if (offsets[0] != 0) return MMF_ERR_SHAPE;
  for (int g = 0; g < G; ++g)
    if (offsets[g + 1] <= offsets[g]) return MMF_ERR_SHAPE;      // empty or decreasing
  for (int i = 0; i < nplane * G; ++i)
    if (!src[i]) return MMF_ERR_ARG;
  for (int m = 0; m < nplane; ++m)
    if (!dst[m]) return MMF_ERR_ARG;
  auto aligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  for (int i = 0; i < nplane * G; ++i)
    if (!aligned(src[i])) return MMF_ERR_ALIGN;
  for (int m = 0; m < nplane; ++m)
    if (!aligned(dst[m])) return MMF_ERR_ALIGN;
  // units of work per workgroup: 2048 x 16 bytes = 32 KiB of the narrower side, two passes of the unrolled loop
  static const int chunk = tune_int("MMF_GATHER_CHUNK", 2048);
  if (chunk < 1) return MMF_ERR_ARG;
  const bool sb = src_bf16 != 0, db = dst_bf16 != 0;
  const int E = (sb || db) ? 8 : 4;
  GatherTable t{};
  t.G = G;
  int64_t cb = 0;
  for (int g = 0; g <= G; ++g) {
    t.off[g] = offsets[g];
    t.cbeg[g] = (int)cb;
    if (g < G) cb += ((offsets[g + 1] - offsets[g]) * (int64_t)(L / E) + chunk - 1) / chunk;
    if (cb > 0x7FFFFFFF) return MMF_ERR_SHAPE;
  }
  for (int i = 0; i < nplane * G; ++i) t.src[i] = src[i];
  for (int m = 0; m < nplane; ++m) t.dst[m] = dst[m];
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)cb, (unsigned)nplane), block(GATHER_THREADS);
  {
    ProfScope ps("bag_gather_kernel", st);
    if (sb && db) hipLaunchKernelGGL((bag_gather_kernel<true, true>), grid, block, 0, st, t, (int)L, chunk);
    else if (sb) hipLaunchKernelGGL((bag_gather_kernel<true, false>), grid, block, 0, st, t, (int)L, chunk);
    else if (db) hipLaunchKernelGGL((bag_gather_kernel<false, true>), grid, block, 0, st, t, (int)L, chunk);
    else hipLaunchKernelGGL((bag_gather_kernel<false, false>), grid, block, 0, st, t, (int)L, chunk);
  }
  return hipGetLastError() == hipSuccess ? MMF_OK : MMF_ERR_LAUNCH;
}
