// The kernels of libyf_images.so that describe detections (yf_images_describe_records_device, yf_images_describe_records_yuv_device):
// every record's region of its picture as an 8 x 8 grid of mean luma, a yf_face_desc (the rule: yf_images_describe.h).  Included once by
// yf_images.hip, behind yf_images_blur.hip.h; C-ABI and semantics: include/yf_images.h.
//
// Two launches.  The first is the crop's scan, yfcrop::first_kernel: d_first is the exclusive prefix of the clamped counts.
//
// records_kernel: one 256-thread workgroup per record that exists, grid-striding over first[n]; it finds its record's (frame, slot) with
// yfcrop::find_chip, READS the region and writes the 17 words of d_desc[frame][slot].  The walk is the blur's means launch at a fixed
// 8 x 8 grid: a unit of work is a band -- the rows of one row of cells, cut into chunks of 64 consecutive bytes -- and goes to one wave;
// a lane keeps one byte column, whose cell and channel are the same in every row of the band, loads it row after row (a wave's load is 64
// consecutive bytes of a pixel row, one byte wide, no alignment assumed, eight loads in flight before a lane adds) and adds its column
// sum, which 32 bits hold, times its channel's luma weight to its cell's 64-bit total in LDS: one LDS atomic per lane and band, 64-bit
// arithmetic only there and in the final division.  A region has at least eight bands, so every wave has work without the blur's row
// split.  The alpha byte of a four-byte pixel is never loaded.  Its first pass over the frames writes d_status, so that a frame without
// records has its status.
//
// Safety: as in yf_images_blur.hip.h.  d_counts and d_dets may hold anything and d_first is read back: the total is clamped to [0, n *
// cap], find_chip admits a record only if its frame's range in d_first holds it and its slot lies below cap, a region comes out of
// yfi_crop_region clamped to the picture's sides, which yfi_image_ok / yfi_yuv_image_ok have tied to the buffer's size: no load leaves a
// picture's or plane's extent, and the one store goes to d_desc[frame * cap + slot] with frame < n and slot < cap.
#ifndef YF_IMAGES_DESCRIBE_HIP_H
#define YF_IMAGES_DESCRIBE_HIP_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/yf_images.h"
#include "yf_images_describe.h"
#include "yf_images_crop.hip.h"

namespace yfdescribe {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRowsInFlight = 8;                          // rows of a band a lane loads before it adds
static_assert((uint64_t)YF_IMAGES_MAX_SIDE * 255 < (1ull << 32), "a lane's column sum in 32 bits");

struct Args {
  yfcrop::Args c;                                         // what find_chip reads: imgs, dets, counts, n, cap, first; and bytes, margin, flags
  const uint8_t* px;                                      // the pictures: only read
  uint32_t* desc;                                         // yf_face_desc[n][cap] as words
  int32_t* status;
};

// C: bytes per pixel of a packed format, BGR: blue first; C = 0: NV12 / NV21 surfaces, of which only the Y plane is read
template <int C, bool BGR>
__global__ void __launch_bounds__(kThreads) records_kernel(Args a) {
  constexpr int B = C == 0 ? 1 : C;                       // bytes per pixel of the plane that is read
  constexpr int G = YF_DESC_GRID;
  __shared__ unsigned long long s_sum[YF_DESC_BYTES];
  __shared__ uint32_t s_word[YF_DESC_BYTES / 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (long i = (long)blockIdx.x * kThreads + tid; i < a.c.n; i += (long)gridDim.x * kThreads) {
    int ok;
    if (C == 0) {
      const yf_image_yuv im = ((const yf_image_yuv*)a.c.imgs)[i];
      ok = yfi_yuv_image_ok(im.offset_y, im.offset_uv, im.height, im.width, im.stride_y, im.stride_uv, a.c.bytes);
    } else {
      const yf_image im = ((const yf_image*)a.c.imgs)[i];
      ok = yfi_image_ok(im.offset, im.height, im.width, im.row_stride, C, a.c.bytes);
    }
    a.status[i] = ok ? 0 : YFI_DESCRIBE_INVALID;
  }
  const long total = a.c.first[a.c.n], most = a.c.n * (long)a.c.cap;
  const long limit = total < 0 ? 0 : (total > most ? most : total);
  for (long rec = blockIdx.x; rec < limit; rec += gridDim.x) {
    yfcrop::Chip c;
    if (!yfcrop::find_chip(a.c, rec, &c)) continue;       // the same in every thread
    uint32_t* out = a.desc + ((size_t)c.frame * (size_t)a.c.cap + (size_t)c.slot) * YFI_DESC_WORDS;
    yf_chip r;
    const uint8_t* base = nullptr;
    int64_t stride = 0;
    bool valid;
    if (C == 0) {
      const yf_image_yuv im = ((const yf_image_yuv*)a.c.imgs)[c.frame];
      valid = yfi_yuv_image_ok(im.offset_y, im.offset_uv, im.height, im.width, im.stride_y, im.stride_uv, a.c.bytes) &&
              yfi_crop_region(c.rec.x1, c.rec.y1, c.rec.x2, c.rec.y2, im.width, im.height, a.c.margin, a.c.flags, &r) == 0;
      base = a.px + im.offset_y; stride = im.stride_y;
    } else {
      const yf_image im = ((const yf_image*)a.c.imgs)[c.frame];
      valid = yfi_image_ok(im.offset, im.height, im.width, im.row_stride, C, a.c.bytes) &&
              yfi_crop_region(c.rec.x1, c.rec.y1, c.rec.x2, c.rec.y2, im.width, im.height, a.c.margin, a.c.flags, &r) == 0;
      base = a.px + im.offset; stride = im.row_stride;
    }
    valid = valid && yfi_describe_region_ok(&r);
    if (!valid) {                                         // all 68 bytes zero; nothing of the picture is read
      if (tid < YFI_DESC_WORDS) out[tid] = 0u;
      continue;
    }
    __syncthreads();                                      // the previous record's readers of the sums and the words are done
    if (tid < YF_DESC_BYTES) s_sum[tid] = 0;
    __syncthreads();
    const int rb = r.width * B, chunks = (rb + 63) / 64, bands = G * chunks;
    for (int u = wave; u < bands; u += kWaves) {
      const int cy = u / chunks, j = (u - cy * chunks) * 64 + lane;
      const int x = j / B, ch = j - x * B;
      if (j >= rb || ch >= 3) continue;                   // beyond the row; the alpha byte
      const int32_t ya = yfi_blur_cell_at(cy, r.height, G), rows = yfi_blur_cell_at(cy + 1, r.height, G) - ya;
      const uint8_t* p = base + (int64_t)(r.y0 + ya) * stride + (int64_t)r.x0 * B + j;
      uint32_t sum = 0;
      for (int rr = 0; rr < rows; rr += kRowsInFlight) {
        uint32_t v[kRowsInFlight];
#pragma unroll
        for (int q = 0; q < kRowsInFlight; ++q) v[q] = rr + q < rows ? (uint32_t)p[(int64_t)(rr + q) * stride] : 0u;
#pragma unroll
        for (int q = 0; q < kRowsInFlight; ++q) sum += v[q];
      }
      const uint32_t w = C == 0 ? 1u : yfi_describe_weight(ch, BGR ? 1 : 0);
      atomicAdd(&s_sum[cy * G + yfi_blur_cell_of(x, r.width, G)], (unsigned long long)sum * w);
    }
    __syncthreads();
    if (tid < YF_DESC_BYTES) {                            // a thread per cell; four cells make a word
      const int cy = tid / G, cx = tid - cy * G;
      const uint64_t cnt = (uint64_t)(yfi_blur_cell_at(cx + 1, r.width, G) - yfi_blur_cell_at(cx, r.width, G)) *
                           (uint64_t)(yfi_blur_cell_at(cy + 1, r.height, G) - yfi_blur_cell_at(cy, r.height, G));
      uint32_t v = C == 0 ? yfi_blur_mean(s_sum[tid], cnt) : yfi_describe_luma(s_sum[tid], cnt);
      v <<= 8 * (tid & 3);
      v |= __shfl_xor(v, 1);
      v |= __shfl_xor(v, 2);
      if ((tid & 3) == 0) s_word[tid >> 2] = v;
    }
    __syncthreads();
    if (tid < YFI_DESC_WORDS) out[tid] = tid == 0 ? YF_DESC_VALID : s_word[tid - 1];
  }
}

}  // namespace yfdescribe
#endif
