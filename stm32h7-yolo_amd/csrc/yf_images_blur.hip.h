// The kernels of libyf_images.so that blur detections in place (yf_images_blur_records_device, yf_images_blur_records_yuv_device): every
// record's region of its picture replaced by a coarse grid of its own means, resized back to the region (the rule: yf_images_blur.h).
// Included once by yf_images.hip, behind yf_images_redact.hip.h; C-ABI and semantics: include/yf_images.h.
//
// Three launches.  The first is the crop's scan, yfcrop::first_kernel: d_first is the exclusive prefix of the clamped counts.
//
// means_kernel: one 256-thread workgroup per record with a slot (k < records_cap), grid-striding; it finds its record's (frame, slot) with
// yfcrop::find_chip, READS the region and writes the gy x gx means to slot k of the workspace.  The region is walked by rows, the rows of
// one row of cells at a time: consecutive lanes take consecutive bytes of a pixel row, every access one byte wide with no alignment
// assumed, eight rows' loads in flight before a lane adds, as mean_block keeps four.  A lane's byte column lies in one cell, so its sum
// over the band stays in a register (32 bits: at most 16384 rows) and goes to the cell's 64-bit total in LDS with one atomic per band
// (plane_sums).  Its first pass over the frames writes d_status (bit 0 and bit 1), so that a frame without records has its status.
//
// paint_kernel: one workgroup per record, grid-striding over first[n].  The slot's grid goes into LDS (1 KB); the records in front of this
// one in its frame whose region meets this region (surfaces: whose chroma region meets this chroma region) go into LDS as four uint16
// each, appended through an LDS counter, at most cap - 1 = 1199 entries -- the mosaic's list with pixel rectangles in place of block
// rectangles.  If one of them contains the whole region the workgroup leaves.  Otherwise rows go to the waves and consecutive pixels to
// the lanes (a lane looks up its taps, its four cells and its owner once for its pixel's colour bytes, which it stores one byte wide; a
// wave's stores of one channel cover the row's bytes between them): the vertical tap is the same in the whole wave, the horizontal tap comes
// from a table in LDS (regions up to 1024 pixels wide, built once per plane) or from yfi_axis_tap per pixel.  Every owned colour byte is
// written once and nothing else: not alpha, not row padding.  A record without a slot (k >= records_cap) takes the same walk with the fill's bytes.  Surfaces: the Y plane, then the chroma
// plane, in the same workgroup.
//
// No kernel reads a byte that another workgroup of its launch writes: the means read the pictures and write the slots, the paint reads the
// slots and the records and writes the pictures.
//
// Safety: as in yf_images_redact.hip.h.  d_counts and d_dets may hold anything and d_first is read back: the total is clamped to [0, n *
// cap], find_chip admits a record only if its frame's range in d_first holds it, a region comes out of yfi_crop_region clamped to the
// picture's sides, which yfi_image_ok / yfi_yuv_image_ok have tied to the buffer's size, and a slot index is below records_cap, which the
// host has tied to work_bytes: no load or store leaves a picture's or plane's extent or the workspace.
#ifndef YF_IMAGES_BLUR_HIP_H
#define YF_IMAGES_BLUR_HIP_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/yf_images.h"
#include "yf_images_blur.h"
#include "yf_images_crop.hip.h"

namespace yfblur {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRowsInFlight = 8;                          // rows of a band a lane loads before it adds
constexpr int kListCap = YF_IMAGES_NMS_WIDE_MAX_CAP - 1;  // the records in front of the last slot
constexpr int kCells = YF_BLUR_MAX_GRID * YF_BLUR_MAX_GRID;
constexpr int kSplitBelow = 8;                            // a region of fewer bands has each cut into kSplitBelow / bands row chunks
constexpr int kTapCap = 1024;                             // the widest region whose horizontal taps are kept in LDS (4 KB)
static_assert((uint64_t)YF_IMAGES_MAX_SIDE * 255 < (1ull << 32), "a lane's column sum in 32 bits");
static_assert(YF_IMAGES_MAX_SIDE <= 65536, "a pixel coordinate in 16 bits");
static_assert(YF_BLUR_MAX_GRID <= 16, "a tap's source cell in the table's top byte; cell arithmetic in 32 bits");

struct Args {
  yfcrop::Args c;                                         // what find_chip reads: imgs, dets, counts, n, cap, first; and bytes, margin, flags
  uint8_t* px;                                            // the pictures: read by the means, written by the paint
  int format, grid;
  uint32_t colour;
  uint32_t* work;                                         // slot k: grid * grid cells of four bytes
  long records_cap;
  int32_t* status;
};

// d_status of every frame, by the whole grid.  C: bytes per pixel of a packed format; 0: NV12 / NV21 surfaces
template <int C>
__device__ __forceinline__ void write_status(const Args& a) {
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < a.c.n; i += (long)gridDim.x * kThreads) {
    int ok;
    if (C == 0) {
      const yf_image_yuv im = ((const yf_image_yuv*)a.c.imgs)[i];
      ok = yfi_yuv_image_ok(im.offset_y, im.offset_uv, im.height, im.width, im.stride_y, im.stride_uv, a.c.bytes);
    } else {
      const yf_image im = ((const yf_image*)a.c.imgs)[i];
      ok = yfi_image_ok(im.offset, im.height, im.width, im.row_stride, C, a.c.bytes);
    }
    const long lo = a.c.first[i], hi = a.c.first[i + 1];
    a.status[i] = (ok ? 0 : YFI_BLUR_INVALID) | (hi > lo && hi > a.records_cap ? YFI_BLUR_FILLED : 0);
  }
}

// the number of records to visit: the total behind the last frame's prefix, clamped to [0, n * cap]
__device__ __forceinline__ long records_limit(const Args& a) {
  const long total = a.c.first[a.c.n], most = a.c.n * (long)a.c.cap;
  return total < 0 ? 0 : (total > most ? most : total);
}

// The sums of one plane's region.  A unit of work is a band -- the rows of one row of cells, cut into chunks of 64 consecutive bytes -- and
// goes to one wave: a lane keeps one byte column, whose cell and channel are the same in every row of the band, loads it row after row
// (a wave's load is 64 consecutive bytes of a pixel row, one byte wide, no alignment assumed; kRowsInFlight loads leave before the first
// is waited for) and adds its column sum, which 32 bits hold, to its cell's 64-bit total in LDS: one LDS atomic per lane and band, not per
// byte.  A region of fewer than kSplitBelow bands has its bands cut into row chunks, so that a region of one cell still occupies every
// wave.  s_sum[cell * 3 + at + channel] collects.  base: the plane's first byte; r: the region in the plane's pixels (pairs) of C bytes,
// the first NC of them colour; the same in every lane of a wave.
template <int C, int NC>
__device__ __forceinline__ void plane_sums(const uint8_t* base, int64_t stride, const yf_chip& r, int gx, int gy, int at, int lane, int wave,
                                           unsigned long long* s_sum) {
  const int rb = r.width * C, chunks = (rb + 63) / 64, bands = gy * chunks;
  const int parts = bands >= kSplitBelow ? 1 : kSplitBelow / bands;
  for (int u = wave; u < bands * parts; u += kWaves) {
    const int band = u / parts, part = u - band * parts;
    const int cy = band / chunks, j = (band - cy * chunks) * 64 + lane;
    const int32_t ya = yfi_blur_cell_at(cy, r.height, gy), h = yfi_blur_cell_at(cy + 1, r.height, gy) - ya;
    const int32_t ra = (int32_t)((int64_t)h * part / parts), rows = (int32_t)((int64_t)h * (part + 1) / parts) - ra;
    const int x = j / C, ch = j - x * C;
    if (j >= rb || ch >= NC) continue;
    const uint8_t* p = base + (int64_t)(r.y0 + ya + ra) * stride + (int64_t)r.x0 * C + j;
    uint32_t sum = 0;
    for (int rr = 0; rr < rows; rr += kRowsInFlight) {
      uint32_t v[kRowsInFlight];
#pragma unroll
      for (int q = 0; q < kRowsInFlight; ++q) v[q] = rr + q < rows ? (uint32_t)p[(int64_t)(rr + q) * stride] : 0u;
#pragma unroll
      for (int q = 0; q < kRowsInFlight; ++q) sum += v[q];
    }
    if (rows > 0) atomicAdd(&s_sum[(cy * gx + yfi_blur_cell_of(x, r.width, gx)) * 3 + at + ch], (unsigned long long)sum);
  }
}

__device__ __forceinline__ uint64_t cell_count(int cell, const yf_chip& r, int gx, int gy) {
  const int cy = cell / gx, cx = cell - cy * gx;
  return (uint64_t)(yfi_blur_cell_at(cx + 1, r.width, gx) - yfi_blur_cell_at(cx, r.width, gx)) *
         (uint64_t)(yfi_blur_cell_at(cy + 1, r.height, gy) - yfi_blur_cell_at(cy, r.height, gy));
}

// C: bytes per pixel of a packed format; 0: NV12 / NV21 surfaces
template <int C>
__global__ void __launch_bounds__(kThreads) means_kernel(Args a) {
  __shared__ unsigned long long s_sum[kCells * 3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = a.grid;
  write_status<C>(a);
  long limit = records_limit(a);
  if (limit > a.records_cap) limit = a.records_cap;
  for (long rec = blockIdx.x; rec < limit; rec += gridDim.x) {
    yfcrop::Chip c;
    if (!yfcrop::find_chip(a.c, rec, &c)) continue;
    yf_chip r, q;
    int gx, gy, hx = 1, hy = 1;
    const uint8_t* base;
    const uint8_t* uv = nullptr;
    int64_t stride, stride_uv = 0;
    if (C == 0) {
      const yf_image_yuv im = ((const yf_image_yuv*)a.c.imgs)[c.frame];
      if (!yfi_yuv_image_ok(im.offset_y, im.offset_uv, im.height, im.width, im.stride_y, im.stride_uv, a.c.bytes)) continue;
      if (yfi_crop_region(c.rec.x1, c.rec.y1, c.rec.x2, c.rec.y2, im.width, im.height, a.c.margin, a.c.flags, &r) != 0) continue;
      base = a.px + im.offset_y; uv = a.px + im.offset_uv; stride = im.stride_y; stride_uv = im.stride_uv;
      q = yfi_blur_chroma(&r);
      hx = yfi_blur_cells(q.width, g, YFI_BLUR_MIN_CELL_CHROMA); hy = yfi_blur_cells(q.height, g, YFI_BLUR_MIN_CELL_CHROMA);
    } else {
      const yf_image im = ((const yf_image*)a.c.imgs)[c.frame];
      if (!yfi_image_ok(im.offset, im.height, im.width, im.row_stride, C, a.c.bytes)) continue;
      if (yfi_crop_region(c.rec.x1, c.rec.y1, c.rec.x2, c.rec.y2, im.width, im.height, a.c.margin, a.c.flags, &r) != 0) continue;
      base = a.px + im.offset; stride = im.row_stride;
      q = r;
    }
    gx = yfi_blur_cells(r.width, g, YF_BLUR_MIN_CELL); gy = yfi_blur_cells(r.height, g, YF_BLUR_MIN_CELL);
    __syncthreads();                                      // the previous record's readers of the sums are done
    for (int t = tid; t < kCells * 3; t += kThreads) s_sum[t] = 0;
    __syncthreads();
    if (C == 0) {
      plane_sums<1, 1>(base, stride, r, gx, gy, 0, lane, wave, s_sum);
      plane_sums<2, 2>(uv, stride_uv, q, hx, hy, 1, lane, wave, s_sum);
    } else {
      plane_sums<(C == 0 ? 3 : C), 3>(base, stride, r, gx, gy, 0, lane, wave, s_sum);
    }
    __syncthreads();
    uint32_t* slot = a.work + (size_t)rec * (size_t)(g * g);
    if (tid < g * g) {                                    // kThreads == kCells: a thread per cell of the slot
      uint32_t v = 0;
      if (C == 0) {
        if (tid < gx * gy) v = yfi_blur_mean(s_sum[tid * 3], cell_count(tid, r, gx, gy));
        if (tid < hx * hy) {
          const uint64_t cnt = cell_count(tid, q, hx, hy);
          v |= yfi_blur_mean(s_sum[tid * 3 + 1], cnt) << 8 | yfi_blur_mean(s_sum[tid * 3 + 2], cnt) << 16;
        }
      } else if (tid < gx * gy) {
        const uint64_t cnt = cell_count(tid, r, gx, gy);
        v = yfi_blur_mean(s_sum[tid * 3], cnt) | yfi_blur_mean(s_sum[tid * 3 + 1], cnt) << 8 | yfi_blur_mean(s_sum[tid * 3 + 2], cnt) << 16;
      }
      slot[tid] = v;
    }
  }
}
static_assert(kThreads == kCells, "means_kernel and paint_kernel give a thread to every cell of a slot");

// The records in front of slot c.slot of its frame whose region meets `mine` (SH = 1: whose chroma region meets its chroma region), into
// s_list as pixel rectangles; s_ctl[0] their number, s_ctl[1] whether one of them contains `mine`.  Every thread of the workgroup calls
// it; true: the workgroup owns nothing.
template <int SH>
__device__ __forceinline__ bool earlier_owners(const Args& a, const yfcrop::Chip& c, int W, int H, const yf_chip& mine, ushort4* s_list,
                                               int* s_ctl) {
  __syncthreads();                                        // the previous record's readers of the list are done
  if (threadIdx.x < 2) s_ctl[threadIdx.x] = 0;
  __syncthreads();
  const int mx0 = mine.x0, my0 = mine.y0, mx1 = mine.x0 + mine.width - 1, my1 = mine.y0 + mine.height - 1;
  const yf_det* row = a.c.dets + c.frame * a.c.cap;
  for (int s = threadIdx.x; s < c.slot; s += kThreads) {
    const yf_det d = row[s];
    yf_chip r;
    if (yfi_crop_region(d.x1, d.y1, d.x2, d.y2, W, H, a.c.margin, a.c.flags, &r) != 0) continue;
    const int x0 = r.x0, y0 = r.y0, x1 = r.x0 + r.width - 1, y1 = r.y0 + r.height - 1;
    if ((x1 >> SH) < (mx0 >> SH) || (x0 >> SH) > (mx1 >> SH) || (y1 >> SH) < (my0 >> SH) || (y0 >> SH) > (my1 >> SH)) continue;
    if (x0 <= mx0 && x1 >= mx1 && y0 <= my0 && y1 >= my1) s_ctl[1] = 1;
    const int at = atomicAdd(&s_ctl[0], 1);
    if (at < kListCap) s_list[at] = make_ushort4((unsigned short)x0, (unsigned short)y0, (unsigned short)x1, (unsigned short)y1);
  }
  __syncthreads();
  return s_ctl[1] != 0;
}

// whether a list entry holds pixel (SH = 1: pair) (x, y) of the plane
template <int SH>
__device__ __forceinline__ bool owned_earlier(const ushort4* s_list, int listed, int x, int y) {
  bool taken = false;
  for (int q = 0; q < listed; ++q) {
    const ushort4 e = s_list[q];                          // the same address in every lane
    taken |= x >= (int)(e.x >> SH) && x <= (int)(e.z >> SH) && y >= (int)(e.y >> SH) && y <= (int)(e.w >> SH);
  }
  return taken;
}

// One plane of one record: the region r (in the plane's pixels or pairs, C bytes each, the first NC written) gets the resample of the
// gy x gx cells of s_grid (bytes at .. at + NC - 1 of a cell), or with filled the bytes f[0 .. NC - 1]; rows to the waves, consecutive
// pixels to the lanes.  Every thread of the workgroup calls it.
template <int C, int NC, int SH>
__device__ __forceinline__ void paint_plane(uint8_t* base, int64_t stride, const yf_chip& r, int gx, int gy, int at, bool filled,
                                            const uint8_t* f, const uint32_t* s_grid, uint32_t* s_tap, const ushort4* s_list, int listed) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool table = !filled && r.width <= kTapCap;
  __syncthreads();                                        // the previous plane's readers of the table are done
  if (table)
    for (int d = threadIdx.x; d < r.width; d += kThreads) {
      const yfi_tap t = yfi_axis_tap(d, r.width, gx);     // weights of at most 2048 in 12 bits each, the cell in the top byte
      s_tap[d] = (uint32_t)t.w0 | (uint32_t)t.w1 << 12 | (uint32_t)t.s0 << 24;
    }
  __syncthreads();
  for (int y = wave; y < r.height; y += kWaves) {
    yfi_tap ty = yfi_tap{0, 0, 0, 0};
    if (!filled) ty = yfi_axis_tap(y, r.height, gy);      // the same in the whole wave
    const int Y = r.y0 + y;
    uint8_t* row = base + (int64_t)Y * stride + (int64_t)r.x0 * C;
    const uint32_t* g0 = s_grid + ty.s0 * gx;
    const uint32_t* g1 = s_grid + ty.s1 * gx;
    for (int x = lane; x < r.width; x += 64) {            // a pixel per lane: its taps, its four cells and its owner once for its NC bytes
      if (listed != 0 && owned_earlier<SH>(s_list, listed, r.x0 + x, Y)) continue;
      uint8_t* q = row + x * C;
      if (filled) {
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) q[ch] = f[ch];
        continue;
      }
      yfi_tap tx;
      if (table) {
        const uint32_t t = s_tap[x];
        tx.s0 = (int32_t)(t >> 24); tx.s1 = tx.s0 + 1 < gx ? tx.s0 + 1 : gx - 1;
        tx.w0 = (int32_t)(t & 0xFFFu); tx.w1 = (int32_t)(t >> 12 & 0xFFFu);
      } else {
        tx = yfi_axis_tap(x, r.width, gx);
      }
      const uint32_t c00 = g0[tx.s0], c01 = g0[tx.s1], c10 = g1[tx.s0], c11 = g1[tx.s1];
#pragma unroll
      for (int ch = 0; ch < NC; ++ch) q[ch] = yfi_blur_mix(c00, c01, c10, c11, at + ch, tx, ty);
    }
  }
}

// C: bytes per pixel of a packed format; 0: NV12 / NV21 surfaces
template <int C>
__global__ void __launch_bounds__(kThreads) paint_kernel(Args a) {
  __shared__ ushort4 s_list[kListCap];
  __shared__ uint32_t s_grid[kCells];
  __shared__ uint32_t s_tap[kTapCap];
  __shared__ int s_ctl[2];
  const int tid = threadIdx.x, g = a.grid;
  uint8_t f[3];
  yfi_redact_fill_bytes(a.colour, a.format, f);
  const long limit = records_limit(a);
  for (long rec = blockIdx.x; rec < limit; rec += gridDim.x) {
    yfcrop::Chip c;
    if (!yfcrop::find_chip(a.c, rec, &c)) continue;
    const bool filled = rec >= a.records_cap;
    if (C == 0) {
      const yf_image_yuv im = ((const yf_image_yuv*)a.c.imgs)[c.frame];
      if (!yfi_yuv_image_ok(im.offset_y, im.offset_uv, im.height, im.width, im.stride_y, im.stride_uv, a.c.bytes)) continue;
      yf_chip r;
      if (yfi_crop_region(c.rec.x1, c.rec.y1, c.rec.x2, c.rec.y2, im.width, im.height, a.c.margin, a.c.flags, &r) != 0) continue;
      if (earlier_owners<1>(a, c, im.width, im.height, r, s_list, s_ctl)) continue;
      const int listed = s_ctl[0] < kListCap ? s_ctl[0] : kListCap;
      if (!filled) s_grid[tid] = tid < g * g ? a.work[(size_t)rec * (size_t)(g * g) + tid] : 0u;       // published by paint_plane's barrier
      const yf_chip q = yfi_blur_chroma(&r);
      paint_plane<1, 1, 0>(a.px + im.offset_y, im.stride_y, r, yfi_blur_cells(r.width, g, YF_BLUR_MIN_CELL),
                           yfi_blur_cells(r.height, g, YF_BLUR_MIN_CELL), 0, filled, f, s_grid, s_tap, s_list, listed);
      paint_plane<2, 2, 1>(a.px + im.offset_uv, im.stride_uv, q, yfi_blur_cells(q.width, g, YFI_BLUR_MIN_CELL_CHROMA),
                           yfi_blur_cells(q.height, g, YFI_BLUR_MIN_CELL_CHROMA), 1, filled, f + 1, s_grid, s_tap, s_list, listed);
    } else {
      const yf_image im = ((const yf_image*)a.c.imgs)[c.frame];
      if (!yfi_image_ok(im.offset, im.height, im.width, im.row_stride, C, a.c.bytes)) continue;
      yf_chip r;
      if (yfi_crop_region(c.rec.x1, c.rec.y1, c.rec.x2, c.rec.y2, im.width, im.height, a.c.margin, a.c.flags, &r) != 0) continue;
      if (earlier_owners<0>(a, c, im.width, im.height, r, s_list, s_ctl)) continue;
      const int listed = s_ctl[0] < kListCap ? s_ctl[0] : kListCap;
      if (!filled) s_grid[tid] = tid < g * g ? a.work[(size_t)rec * (size_t)(g * g) + tid] : 0u;
      paint_plane<(C == 0 ? 3 : C), 3, 0>(a.px + im.offset, im.row_stride, r, yfi_blur_cells(r.width, g, YF_BLUR_MIN_CELL),
                                          yfi_blur_cells(r.height, g, YF_BLUR_MIN_CELL), 0, filled, f, s_grid, s_tap, s_list, listed);
    }
  }
}

}  // namespace yfblur
#endif
