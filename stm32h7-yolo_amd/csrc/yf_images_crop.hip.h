// The kernels of libyf_images.so that cut face chips (yf_images_crop_records_device, yf_images_crop_records_yuv_device): every record's
// region of its picture, resized to out_h x out_w as cv2.resize does (the rule: yf_images_crop.h).  Included once by yf_images.hip; C-ABI
// and semantics: include/yf_images.h.
//
// Two launches.  first_kernel: ONE 256-thread workgroup walks the frames' counts in chunks of 1024 (four consecutive frames per lane) --
// an inclusive scan of the lanes' sums inside each wave by cross-lane moves, the four wave totals through LDS, the running base in a
// register -- and writes every frame's exclusive prefix and, behind the last one, the total.  chips_kernel / chips_yuv_kernel: one
// workgroup per chip, grid-striding over min(total, chips_cap).  A workgroup finds its chip's (frame, slot) by a binary search in d_first
// that is the same in every lane (above 64 frames one probe of 64 evenly spaced prefixes, a load and a ballot, narrows the range first:
// the search is a chain of dependent loads, and a workgroup that cuts one chip waits for all of it), reads the record and the descriptor,
// works out the region, builds the two tap tables in LDS (out_w + out_h taps, once per chip) and then computes every output pixel once:
// lanes take consecutive output columns, so the bytes of a sampled source row coalesce, four byte-wide reads per channel (two rows, two
// columns), horizontal then vertical pass, as prepare_frames does.  The byte orders are template parameters, so that the three channels
// of a sample are loads at constant offsets from one address; the row offsets are in the tap table as 64-bit products.
// The sizes are run-time values: a band of as many whole rows as fit the 8 KB stage is written to LDS and leaves with 16-byte stores
// (out_w * 3 is a multiple of 48: every row is whole vectors); a lane's pixel advances by 256 with one compare instead of a division.
// What either launch costs follows the frames and the records that exist, never cap or chips_cap: a workgroup beyond the total leaves
// after one load.
//
// Safety: d_counts and d_dets are device memory that may hold anything, and d_first is read back from memory.  Every index derived from
// them is range-checked before use: the total is clamped to [0, chips_cap], a chip is cut only if its frame's range in d_first holds it
// and its slot lies below both cap and the frame's clamped count, and the region comes out of yfi_crop_region clamped to the picture's
// sides, which yfi_image_ok / yfi_yuv_image_ok have tied to the buffer's size: no load leaves a picture's extent as its descriptor
// states it.  A record's edges may be anything (INT32_MIN, x1 > x2): the arithmetic is int64.
#ifndef YF_IMAGES_CROP_HIP_H
#define YF_IMAGES_CROP_HIP_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/yf_images.h"
#include "yf_images_crop.h"

namespace yfcrop {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPerLane = 4;                              // frames per lane and chunk of first_kernel
constexpr int kStageBytes = 8192;                        // the band: 10 rows at out_w = 256, 17 at 160, 24 at 112; 18 KB of LDS in all, 8 per CU
static_assert(kStageBytes >= YFI_CROP_MAX_OUT * 3 && kStageBytes % 16 == 0, "the stage holds at least one row of the widest chip");

struct Args {
  const uint8_t* px;
  uint64_t bytes;
  const void* imgs;                                      // yf_image[n] or yf_image_yuv[n]
  const yf_det* dets;
  const int* counts;
  long n;
  int cap, out_h, out_w;
  int margin, flags;
  uint8_t* chips;
  long chips_cap;
  const int32_t* first;
  yf_chip* info;
};

__global__ void __launch_bounds__(kThreads) first_kernel(const int* __restrict__ counts, long n, int cap, int32_t* __restrict__ first) {
  __shared__ int s_wave[2][kWaves];                      // two sets, used in turn: one barrier per chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0;                                          // at most n * cap < 2^31
  int buf = 0;
  for (long c = 0; c < n; c += kThreads * kPerLane, buf ^= 1) {
    const long j = c + (long)tid * kPerLane;
    int m[kPerLane], sum = 0;
#pragma unroll
    for (int q = 0; q < kPerLane; ++q) {
      m[q] = j + q < n ? yfi_crop_clamp(counts[j + q], cap) : 0;
      sum += m[q];
    }
    int incl = sum;
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
    int at = base + before + incl - sum;
#pragma unroll
    for (int q = 0; q < kPerLane; ++q) {
      if (j + q < n) first[j + q] = at;
      at += m[q];
    }
    base += all;
  }
  if (tid == 0) first[n] = base;
}

// What every chip kernel does before it samples: the chip's frame and slot, its record and, from the picture's sides, its region; the
// info row; the zero fill of a chip without a region.  `k` and everything derived from it is the same in every lane.
struct Chip {
  long frame;
  int slot;
  yf_det rec;
};

// the chip's frame by binary search (the last i in [0, n) with first[i] <= k) and its record; false: no frame's range holds the chip, or
// the slot is not a record of that frame
__device__ __forceinline__ bool find_chip(const Args& a, long k, Chip* c) {
  long lo = 0, hi = a.n;
  if (a.n > 64) {                                        // one probe of 64 evenly spaced prefixes narrows the range: six dependent loads fewer
    const long step = (a.n + 63) / 64, at = (long)(threadIdx.x & 63) * step;
    const uint64_t le = __ballot(at < a.n && (long)a.first[at < a.n ? at : 0] <= k);
    lo = le ? (long)(63 - __builtin_clzll(le)) * step : 0;
    hi = lo + step < a.n ? lo + step : a.n;
  }
  while (hi - lo > 1) {
    const long mid = lo + (hi - lo) / 2;
    if ((long)a.first[mid] <= k) lo = mid; else hi = mid;
  }
  const long lo_first = a.first[lo], hi_first = a.first[lo + 1];
  if (!(lo_first <= k && k < hi_first)) return false;
  const long s = k - lo_first;
  if (s >= (long)yfi_crop_clamp(a.counts[lo], a.cap)) return false;          // below cap too: the clamp
  c->frame = lo;
  c->slot = (int)s;
  c->rec = a.dets[lo * a.cap + s];
  return true;
}

__device__ __forceinline__ void write_info(const Args& a, long k, const Chip& c, const yf_chip& r, int status) {
  int32_t* o = (int32_t*)(a.info + k);
  const int tid = threadIdx.x;
  if (tid < 7) {
    const int32_t v = tid == 0 ? (int32_t)c.frame : tid == 1 ? c.slot : tid == 2 ? r.x0 : tid == 3 ? r.y0 : tid == 4 ? r.width
                    : tid == 5 ? r.height : status;
    o[tid] = v;
  }
}

__device__ __forceinline__ void zero_chip(int4* out, int vecs) {
  const int4 z = make_int4(0, 0, 0, 0);
  for (int q = threadIdx.x; q < vecs; q += kThreads) out[q] = z;
}

// the number of chips to cut: the total behind the last frame's prefix, clamped to [0, chips_cap]
__device__ __forceinline__ long chips_limit(const Args& a) {
  const long total = a.first[a.n];
  return total < 0 ? 0 : (total > a.chips_cap ? a.chips_cap : total);
}

struct YTap { int64_t o0, o1; int32_t w0, w1; };          // the byte offsets of the two rows in the picture, and the weights

// C: bytes per source pixel; SWAP: the chip's byte order is the reverse of the source's (compile time, so that the three channels of a
// sample are loads at constant offsets from one address, as in prepare_frames)
template <int C, bool SWAP>
__global__ void __launch_bounds__(kThreads) chips_kernel(Args a) {
  __shared__ int4 s_xt[YFI_CROP_MAX_OUT];                 // {s0 * C, s1 * C, w0, w1}
  __shared__ YTap s_yt[YFI_CROP_MAX_OUT];
  __shared__ int4 s_stage[kStageBytes / 16];
  const int tid = threadIdx.x;
  const int out_w = a.out_w, out_h = a.out_h, row_bytes = out_w * 3;
  const int chip_vecs = out_h * row_bytes / 16;
  const int band_rows = kStageBytes / row_bytes < out_h ? kStageBytes / row_bytes : out_h;
  const int dy = kThreads / out_w, dx = kThreads - dy * out_w;                 // a lane's next pixel: 256 further in row-major order
  const int y_first = tid / out_w, x_first = tid - y_first * out_w;
  const long limit = chips_limit(a);
  for (long k = blockIdx.x; k < limit; k += gridDim.x) {
    Chip c;
    if (!find_chip(a, k, &c)) continue;
    const yf_image im = ((const yf_image*)a.imgs)[c.frame];
    int4* out = (int4*)(a.chips + (size_t)k * (size_t)chip_vecs * 16u);
    yf_chip r;
    r.x0 = r.y0 = r.width = r.height = 0;
    int status = 2;
    if (yfi_image_ok(im.offset, im.height, im.width, im.row_stride, C, a.bytes))
      status = yfi_crop_region(c.rec.x1, c.rec.y1, c.rec.x2, c.rec.y2, im.width, im.height, a.margin, a.flags, &r);
    write_info(a, k, c, r, status);
    if (status != 0) {                                    // never read: the chip is all 0
      zero_chip(out, chip_vecs);
      continue;
    }
    __syncthreads();                                      // the previous chip's readers of the tap tables and the stage are done
    for (int t = tid; t < out_w + out_h; t += kThreads) {
      if (t < out_w) {
        const yfi_tap x = yfi_crop_tap(t, out_w, r.x0, r.width);
        s_xt[t] = make_int4(x.s0 * C, x.s1 * C, x.w0, x.w1);
      } else {
        const yfi_tap y = yfi_crop_tap(t - out_w, out_h, r.y0, r.height);
        s_yt[t - out_w] = YTap{(int64_t)y.s0 * im.row_stride, (int64_t)y.s1 * im.row_stride, y.w0, y.w1};
      }
    }
    __syncthreads();
    const uint8_t* base = a.px + im.offset;
    uint8_t* stage = (uint8_t*)s_stage;
    for (int r0 = 0; r0 < out_h; r0 += band_rows) {
      const int rows = out_h - r0 < band_rows ? out_h - r0 : band_rows;
      int yy = y_first, xx = x_first;
      for (int p = tid; p < rows * out_w; p += kThreads) {
        const int4 tx = s_xt[xx];
        const YTap ty = s_yt[r0 + yy];
        const uint8_t* ra = base + ty.o0;
        const uint8_t* rb = base + ty.o1;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const int sc = SWAP ? 2 - ch : ch;
          const int32_t h0 = yfi_hpass(ra[tx.x + sc], ra[tx.y + sc], tx.z, tx.w);
          const int32_t h1 = yfi_hpass(rb[tx.x + sc], rb[tx.y + sc], tx.z, tx.w);
          stage[p * 3 + ch] = (uint8_t)yfi_vpass(h0, h1, ty.w0, ty.w1);
        }
        xx += dx; yy += dy;
        if (xx >= out_w) { xx -= out_w; ++yy; }
      }
      __syncthreads();
      int4* dst = out + r0 * row_bytes / 16;
      for (int q = tid; q < rows * row_bytes / 16; q += kThreads) dst[q] = s_stage[q];
      __syncthreads();
    }
  }
}

// NV12 / NV21 surfaces: the same plan; the tap tables carry the chroma offsets beside the luma ones (yf_images_yuv.h), taken from the
// ABSOLUTE rows and columns of the surface, and an output pixel converts its four source pixels before it interpolates (yfi_yuv_sample).
template <bool VFIRST, bool OUT_BGR>
__global__ void __launch_bounds__(kThreads) chips_yuv_kernel(Args a) {
  __shared__ yfi_yuv_xtap s_xt[YFI_CROP_MAX_OUT];
  __shared__ yfi_yuv_ytap s_yt[YFI_CROP_MAX_OUT];
  __shared__ int4 s_stage[kStageBytes / 16];
  const int tid = threadIdx.x;
  const int out_w = a.out_w, out_h = a.out_h, row_bytes = out_w * 3;
  const int chip_vecs = out_h * row_bytes / 16;
  const int band_rows = kStageBytes / row_bytes < out_h ? kStageBytes / row_bytes : out_h;
  const int dy = kThreads / out_w, dx = kThreads - dy * out_w;
  const int y_first = tid / out_w, x_first = tid - y_first * out_w;
  const long limit = chips_limit(a);
  for (long k = blockIdx.x; k < limit; k += gridDim.x) {
    Chip c;
    if (!find_chip(a, k, &c)) continue;
    const yf_image_yuv im = ((const yf_image_yuv*)a.imgs)[c.frame];
    int4* out = (int4*)(a.chips + (size_t)k * (size_t)chip_vecs * 16u);
    yf_chip r;
    r.x0 = r.y0 = r.width = r.height = 0;
    int status = 2;
    if (yfi_yuv_image_ok(im.offset_y, im.offset_uv, im.height, im.width, im.stride_y, im.stride_uv, a.bytes))
      status = yfi_crop_region(c.rec.x1, c.rec.y1, c.rec.x2, c.rec.y2, im.width, im.height, a.margin, a.flags, &r);
    write_info(a, k, c, r, status);
    if (status != 0) {
      zero_chip(out, chip_vecs);
      continue;
    }
    __syncthreads();
    for (int t = tid; t < out_w + out_h; t += kThreads) {
      if (t < out_w) s_xt[t] = yfi_yuv_xtap_of(yfi_crop_tap(t, out_w, r.x0, r.width));
      else s_yt[t - out_w] = yfi_yuv_ytap_of(yfi_crop_tap(t - out_w, out_h, r.y0, r.height), im.stride_y, im.stride_uv);
    }
    __syncthreads();
    const uint8_t* yp = a.px + im.offset_y;
    const uint8_t* uvp = a.px + im.offset_uv;
    uint8_t* stage = (uint8_t*)s_stage;
    for (int r0 = 0; r0 < out_h; r0 += band_rows) {
      const int rows = out_h - r0 < band_rows ? out_h - r0 : band_rows;
      int yy = y_first, xx = x_first;
      for (int p = tid; p < rows * out_w; p += kThreads) {
        int32_t rgb[3];
        yfi_yuv_sample(yp, uvp, s_xt[xx], s_yt[r0 + yy], VFIRST, rgb);
        stage[p * 3 + 0] = (uint8_t)(OUT_BGR ? rgb[2] : rgb[0]);
        stage[p * 3 + 1] = (uint8_t)rgb[1];
        stage[p * 3 + 2] = (uint8_t)(OUT_BGR ? rgb[0] : rgb[2]);
        xx += dx; yy += dy;
        if (xx >= out_w) { xx -= out_w; ++yy; }
      }
      __syncthreads();
      int4* dst = out + r0 * row_bytes / 16;
      for (int q = tid; q < rows * row_bytes / 16; q += kThreads) dst[q] = s_stage[q];
      __syncthreads();
    }
  }
}

}  // namespace yfcrop
#endif
