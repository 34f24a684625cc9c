// The kernels of libyf_images.so that make the records of an image's tiles one image's records again (yf_images_gather_tiles_device):
// per image the concatenation of its tiles' records in tile order, translated to the image's pixels (the rule: yf_images_tiles.h).
// Included once by yf_images.hip; C-ABI and semantics: include/yf_images.h.
//
// Two launches.  prefix_kernel: one 256-thread workgroup per image (grid-striding) walks the image's tile counts in chunks of 256 -- an
// inclusive scan inside each wave by cross-lane moves, the four wave totals through LDS, the running base in a register -- and writes
// every tile's exclusive prefix to the workspace and the image's total to d_out_counts.  copy_kernel: one wave per tile, four per
// workgroup, grid-striding over the tiles; a wave whose tile has no record leaves after the one load of its count.  The others find
// their image by a wave-uniform binary search in d_first and copy the tile's 7 * m dwords, which are one contiguous span, with
// consecutive lanes, patching the frame and the four edges on the way.  What either launch costs follows the number of tiles and of
// records, never cap or out_cap.
//
// Safety: membership comes from d_first alone, and d_first, the prefixes and the counts are device memory that may hold anything.  Every
// index derived from them is range-checked before it is used: a range end is clamped to [0, t], a tile copies only if its image's range
// holds it, a prefix outside [0, out_cap) writes nothing and the records written stop at out_cap.  For a d_first that is not a
// non-decreasing sequence from 0 to t the output is unspecified (ranges that overlap race on a tile's prefix), but no access leaves the
// buffers.
#ifndef YF_IMAGES_TILES_HIP_H
#define YF_IMAGES_TILES_HIP_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/yf_images.h"
#include "yf_images_tiles.h"

namespace yftiles {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

__device__ __forceinline__ int clamp_range(int v, int t) { return v < 0 ? 0 : (v > t ? t : v); }

__global__ void __launch_bounds__(kThreads) prefix_kernel(const int* __restrict__ counts, int t, int cap, const int32_t* __restrict__ first,
                                                          long n, int32_t* __restrict__ prefix, int32_t* __restrict__ out_counts) {
  __shared__ int s_wave[2][kWaves];                     // two sets, used in turn: one barrier per chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int buf = 0;                                          // alternates over all chunks of all images of this workgroup
  for (long i = blockIdx.x; i < n; i += gridDim.x) {
    const long a = clamp_range(first[i], t), b = clamp_range(first[i + 1], t);      // the same in every lane
    int base = 0;                                       // at most t * cap < 2^31
    for (long c = a; c < b; c += kThreads, buf ^= 1) {
      const long j = c + tid;
      const int m = j < b ? yfi_tiles_clamp(counts[j], cap) : 0;
      int incl = m;
      for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(incl, off);
        if (lane >= off) incl += up;
      }
      if (lane == 63) s_wave[buf][wave] = incl;
      __syncthreads();
      int before = 0, all = 0;
      for (int w = 0; w < kWaves; ++w) {
        const int v = s_wave[buf][w];
        before += w < wave ? v : 0;
        all += v;
      }
      if (j < b) prefix[j] = base + before + incl - m;
      base += all;
    }
    if (tid == 0) out_counts[i] = base;
  }
}

__global__ void __launch_bounds__(kThreads) copy_kernel(const uint32_t* __restrict__ dets, const int* __restrict__ counts, int t, int cap,
                                                        const yf_tile* __restrict__ tiles, const int32_t* __restrict__ first, long n,
                                                        const int32_t* __restrict__ prefix, uint32_t* __restrict__ out, int out_cap) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * kWaves + (threadIdx.x >> 6), waves = (long)gridDim.x * kWaves;
  for (long j = wave; j < t; j += waves) {
    const int m = __builtin_amdgcn_readfirstlane(yfi_tiles_clamp(counts[j], cap));
    if (m == 0) continue;
    long lo = 0, hi = n;                                // the image: the last i in [0, n) with first[i] <= j
    while (hi - lo > 1) {
      const long mid = lo + (hi - lo) / 2;
      if (__builtin_amdgcn_readfirstlane(first[mid]) <= j) lo = mid; else hi = mid;
    }
    const long i = lo;
    const int a = __builtin_amdgcn_readfirstlane(first[i]), b = __builtin_amdgcn_readfirstlane(first[i + 1]);
    if (!(a <= j && j < b)) continue;                   // no image's range holds this tile
    const int at = __builtin_amdgcn_readfirstlane(prefix[j]);
    if (at < 0 || at >= out_cap) continue;              // beyond the cut (or not a prefix)
    const int room = out_cap - at, w = m < room ? m : room;
    const int32_t x0 = __builtin_amdgcn_readfirstlane(tiles[j].x0), y0 = __builtin_amdgcn_readfirstlane(tiles[j].y0);
    const uint32_t* src = dets + (size_t)j * (size_t)cap * 7u;
    uint32_t* dst = out + ((size_t)i * (size_t)out_cap + (size_t)at) * 7u;
    int q = lane % 7;                                   // 64 = 9 * 7 + 1: the dword's place in its record advances by one per step
    for (int d = lane; d < 7 * w; d += 64) {
      dst[d] = yfi_tiles_dword(src[d], q, (int32_t)i, x0, y0);
      q = q == 6 ? 0 : q + 1;
    }
  }
}

}  // namespace yftiles
#endif
