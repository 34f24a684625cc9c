// The kernels of libyf_images.so that redact detections in place (yf_images_redact_records_device, yf_images_redact_records_yuv_device):
// every record's region of its picture pixelated or filled with one colour (the rule: yf_images_redact.h).  Included once by
// yf_images.hip, behind yf_images_crop.hip.h; C-ABI and semantics: include/yf_images.h.
//
// Two launches.  The first is the crop's scan, yfcrop::first_kernel: d_first is the exclusive prefix of the clamped counts.  The second
// is one 256-thread workgroup per record, grid-striding over first[n]; it finds its record's (frame, slot) with yfcrop::find_chip, and
// its first pass over the frames writes d_status, so that a frame without records has its status too.
//
// Mosaic without a second copy of the pictures and without races: a block of the redacted set is OWNED by the lowest slot of its frame
// whose region touches it, and only the owner reads and writes it -- every block is read before it is written, and written once.  The
// workgroup of slot s walks the records s' < s of its frame (lanes striding, yfi_crop_region each) and keeps those whose block rectangle
// meets its own as four uint16 in LDS (block indices are at most 4095; at most cap - 1 = 1199 entries, 9.6 KB, appended through an LDS
// counter).  If one of them contains its rectangle, the workgroup leaves.  Otherwise its four waves take the blocks of its rectangle in
// turn and skip every block that a list entry holds.  The list is usually empty (records that survived a suppression rarely share
// blocks); its cost is bounded by cap, never by the picture.
// Within a block a group of lanes works, the whole wave or, for blocks of 4 x 4 and 8 x 8 pixels, 16 lanes (four blocks per wave at
// once): consecutive lanes take consecutive bytes of a pixel row (a narrow block puts several rows side by side across the lanes), so
// that a row's loads coalesce and every lane keeps one channel; a lane has four rows' loads in flight before it adds; the channel sums
// cross the group's lanes by __shfl_xor, the mean is computed once and written by the lanes that read.  Offsets and strides carry no alignment: every access is one byte wide.
//
// The fill needs no ownership: every workgroup writes its own region, a wave per row.
//
// Safety: d_counts and d_dets are device memory that may hold anything, and d_first is read back from memory.  The total is clamped to
// [0, n * cap]; find_chip admits a record only if its frame's range in d_first holds it and its slot lies below the frame's clamped
// count; a region comes out of yfi_crop_region clamped to the picture's sides and a block is clipped to them, and yfi_image_ok /
// yfi_yuv_image_ok have tied those sides to the buffer's size: no load or store leaves a picture's or plane's extent as its descriptor
// states it.  Pictures that share bytes (the aliasing contract of yf_images_redact.h) change what is read, never where.
#ifndef YF_IMAGES_REDACT_HIP_H
#define YF_IMAGES_REDACT_HIP_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/yf_images.h"
#include "yf_images_redact.h"
#include "yf_images_crop.hip.h"

namespace yfredact {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRowsInFlight = 4;                          // rows of a block a lane loads before it adds (eight need more than 64 VGPRs)
constexpr int kListCap =YF_IMAGES_NMS_WIDE_MAX_CAP - 1;  // the records in front of the last slot
static_assert(YFI_REDACT_MAX_BLOCK * YFI_REDACT_MAX_BLOCK * 255 < (1 << 30), "a block's channel sum in 32 bits");
static_assert(YF_IMAGES_MAX_SIDE / 4 <= 65536, "a block index in 16 bits");

struct Args {
  yfcrop::Args c;                                         // what find_chip reads: imgs, dets, counts, n, cap, first; and bytes, margin, flags
  uint8_t* px;                                            // the pictures, written
  int format, block;
  uint32_t colour;
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
    a.status[i] = ok ? 0 : 1;
  }
}

// the number of records to visit: the total behind the last frame's prefix, clamped to [0, n * cap]
__device__ __forceinline__ long records_limit(const Args& a) {
  const long total = a.c.first[a.c.n], most = a.c.n * (long)a.c.cap;
  return total < 0 ? 0 : (total > most ? most : total);
}

// The records in front of slot c.slot of its frame whose blocks meet `mine`, into s_list; s_ctl[0] their number, s_ctl[1] whether one of
// them contains `mine`.  Every thread of the workgroup calls it; true: the workgroup owns nothing.
__device__ __forceinline__ bool earlier_owners(const Args& a, const yfcrop::Chip& c, int W, int H, const yfi_blocks& mine, ushort4* s_list,
                                               int* s_ctl) {
  __syncthreads();                                        // the previous record's readers of the list are done
  if (threadIdx.x < 2) s_ctl[threadIdx.x] = 0;
  __syncthreads();
  const yf_det* row = a.c.dets + c.frame * a.c.cap;
  for (int s = threadIdx.x; s < c.slot; s += kThreads) {
    const yf_det d = row[s];
    yf_chip r;
    if (yfi_crop_region(d.x1, d.y1, d.x2, d.y2, W, H, a.c.margin, a.c.flags, &r) != 0) continue;
    const yfi_blocks b = yfi_redact_blocks(&r, a.block);
    if (b.bx1 < mine.bx0 || b.bx0 > mine.bx1 || b.by1 < mine.by0 || b.by0 > mine.by1) continue;
    if (b.bx0 <= mine.bx0 && b.bx1 >= mine.bx1 && b.by0 <= mine.by0 && b.by1 >= mine.by1) s_ctl[1] = 1;
    const int at = atomicAdd(&s_ctl[0], 1);
    if (at < kListCap) s_list[at] = make_ushort4((unsigned short)b.bx0, (unsigned short)b.by0, (unsigned short)b.bx1, (unsigned short)b.by1);
  }
  __syncthreads();
  return s_ctl[1] != 0;
}

// whether a list entry holds block (bx, by); the same in every lane of the wave
__device__ __forceinline__ bool owned_earlier(const ushort4* s_list, int listed, int bx, int by, int lane) {
  if (listed == 0) return false;
  bool taken = false;
  for (int q = lane; q < listed; q += 64) {
    const ushort4 e = s_list[q];
    taken |= bx >= (int)e.x && bx <= (int)e.z && by >= (int)e.y && by <= (int)e.w;
  }
  return __ballot(taken) != 0;
}

// One block by one group of G lanes (G = 16 or 64; `l` the lane's place in its group): `rows` rows of `rb` bytes, `stride` apart, the
// first at p; pixels of C bytes of which the first NC are colour.  L lanes (the largest multiple of C in G) take consecutive bytes;
// where a row is shorter than L, L / rb rows lie side by side.  L is a multiple of C and so is rb: a lane's bytes are all of one
// channel.  Every lane of the wave calls it; a group without a block comes with valid = false and touches no memory.
template <int C, int NC>
__device__ __forceinline__ void mean_block(uint8_t* p, int64_t stride, int rows, int rb, int l, int G, bool valid) {
  const int L = G / C * C;
  const int r0 = l / rb, j0 = l - r0 * rb;
  const int side = rb < L ? L / rb : 1;                   // rows side by side
  const int ch = j0 % C;
  const bool active = valid && l < L && r0 < side && ch < NC;
  uint32_t sum = 0;
  if (active)
    for (int r = r0; r < rows; r += kRowsInFlight * side)   // kRowsInFlight loads leave before the first is waited for
      for (int j = j0; j < rb; j += L) {
        uint32_t v[kRowsInFlight];
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u) {
          const int rr = r + u * side;
          v[u] = rr < rows ? (uint32_t)p[(int64_t)rr * stride + j] : 0u;
        }
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u) sum += v[u];
      }
  uint32_t total = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    uint32_t v = active && ch == c ? sum : 0u;
    for (int off = G >> 1; off >= 1; off >>= 1) v += __shfl_xor(v, off);      // partners stay inside the group
    if (ch == c) total = v;
  }
  if (active) {
    const uint8_t m = (uint8_t)yfi_redact_mean(total, (uint32_t)(rows * (rb / C)));
    for (int r = r0; r < rows; r += side) {
      uint8_t* q = p + (int64_t)r * stride;
      for (int j = j0; j < rb; j += L) q[j] = m;
    }
  }
}

// The blocks of a record's rectangle that its workgroup owns, to the lane groups in turn: a block of 4 x 4 or 8 x 8 pixels goes to 16
// lanes, four blocks per wave at once; a larger one to the whole wave.  -> the group's block (bx, by), or false when the group has none
// in this round (beyond the rectangle, or held by an earlier record).
struct Rounds {
  int G, per_wave, sub, l, nbx, nb;
  __device__ __forceinline__ Rounds(const yfi_blocks& mine, int k, int lane) {
    G = k <= 8 ? 16 : 64;
    per_wave = 64 / G;
    sub = lane / G;
    l = lane - sub * G;
    nbx = mine.bx1 - mine.bx0 + 1;
    nb = nbx * (mine.by1 - mine.by0 + 1);
  }
  __device__ __forceinline__ bool block(const yfi_blocks& mine, int b0, const ushort4* s_list, int listed, int lane, int* bx, int* by) const {
    const int b = b0 + sub;
    bool valid = b < nb;
    const int bb = valid ? b : b0;
    *by = mine.by0 + bb / nbx;
    *bx = mine.bx0 + bb % nbx;
    if (listed != 0)
      for (int q = 0; q < per_wave && b0 + q < nb; ++q) {                     // every group's block is looked up by the whole wave
        const bool taken = owned_earlier(s_list, listed, mine.bx0 + (b0 + q) % nbx, mine.by0 + (b0 + q) / nbx, lane);
        if (q == sub && taken) valid = false;
      }
    return valid;
  }
};

template <int C>
__global__ void __launch_bounds__(kThreads) mosaic_kernel(Args a) {
  __shared__ ushort4 s_list[kListCap];
  __shared__ int s_ctl[2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, k = a.block;
  write_status<C>(a);
  const long limit = records_limit(a);
  for (long rec = blockIdx.x; rec < limit; rec += gridDim.x) {
    yfcrop::Chip c;
    if (!yfcrop::find_chip(a.c, rec, &c)) continue;
    const yf_image im = ((const yf_image*)a.c.imgs)[c.frame];
    if (!yfi_image_ok(im.offset, im.height, im.width, im.row_stride, C, a.c.bytes)) continue;
    yf_chip r;
    if (yfi_crop_region(c.rec.x1, c.rec.y1, c.rec.x2, c.rec.y2, im.width, im.height, a.c.margin, a.c.flags, &r) != 0) continue;
    const yfi_blocks mine = yfi_redact_blocks(&r, k);
    if (earlier_owners(a, c, im.width, im.height, mine, s_list, s_ctl)) continue;
    const int listed = s_ctl[0] < kListCap ? s_ctl[0] : kListCap;
    const Rounds g(mine, k, lane);
    uint8_t* base = a.px + im.offset;
    for (int b0 = wave * g.per_wave; b0 < g.nb; b0 += kWaves * g.per_wave) {
      int bx, by;
      const bool valid = g.block(mine, b0, s_list, listed, lane, &bx, &by);
      int32_t x, w, y, h;
      yfi_redact_span(bx, k, im.width, &x, &w);
      yfi_redact_span(by, k, im.height, &y, &h);
      mean_block<C, 3>(base + (int64_t)y * im.row_stride + (int64_t)x * C, im.row_stride, h, w * C, g.l, g.G, valid);
    }
  }
}

__global__ void __launch_bounds__(kThreads) mosaic_yuv_kernel(Args a) {
  __shared__ ushort4 s_list[kListCap];
  __shared__ int s_ctl[2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, k = a.block;
  write_status<0>(a);
  const long limit = records_limit(a);
  for (long rec = blockIdx.x; rec < limit; rec += gridDim.x) {
    yfcrop::Chip c;
    if (!yfcrop::find_chip(a.c, rec, &c)) continue;
    const yf_image_yuv im = ((const yf_image_yuv*)a.c.imgs)[c.frame];
    if (!yfi_yuv_image_ok(im.offset_y, im.offset_uv, im.height, im.width, im.stride_y, im.stride_uv, a.c.bytes)) continue;
    yf_chip r;
    if (yfi_crop_region(c.rec.x1, c.rec.y1, c.rec.x2, c.rec.y2, im.width, im.height, a.c.margin, a.c.flags, &r) != 0) continue;
    const yfi_blocks mine = yfi_redact_blocks(&r, k);
    if (earlier_owners(a, c, im.width, im.height, mine, s_list, s_ctl)) continue;
    const int listed = s_ctl[0] < kListCap ? s_ctl[0] : kListCap;
    const Rounds g(mine, k, lane);
    uint8_t* yp = a.px + im.offset_y;
    uint8_t* uvp = a.px + im.offset_uv;
    for (int b0 = wave * g.per_wave; b0 < g.nb; b0 += kWaves * g.per_wave) {
      int bx, by;
      const bool valid = g.block(mine, b0, s_list, listed, lane, &bx, &by);
      int32_t x, w, y, h;
      yfi_redact_span(bx, k, im.width, &x, &w);
      yfi_redact_span(by, k, im.height, &y, &h);
      mean_block<1, 1>(yp + (int64_t)y * im.stride_y + x, im.stride_y, h, w, g.l, g.G, valid);
      yfi_redact_chroma_span(bx, k, im.width, &x, &w);
      yfi_redact_chroma_span(by, k, im.height, &y, &h);
      mean_block<2, 2>(uvp + (int64_t)y * im.stride_uv + 2 * x, im.stride_uv, h, 2 * w, g.l, g.G, valid);
    }
  }
}

// `rows` rows of `width` pixels of C bytes, the first at p: the first three bytes of every pixel (C = 1: the byte) get f[]
template <int C>
__device__ __forceinline__ void fill_rows(uint8_t* p, int64_t stride, int rows, int width, const uint8_t* f, int lane, int wave) {
  for (int y = wave; y < rows; y += kWaves) {
    uint8_t* q = p + (int64_t)y * stride;
    for (int j = lane; j < width * C; j += 64) {
      const int ch = j % C;
      if (ch < 3) q[j] = ch == 0 ? f[0] : ch == 1 ? f[1] : f[2];
    }
  }
}

template <int C>
__global__ void __launch_bounds__(kThreads) fill_kernel(Args a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  write_status<C>(a);
  uint8_t f[3];
  yfi_redact_fill_bytes(a.colour, a.format, f);
  const long limit = records_limit(a);
  for (long rec = blockIdx.x; rec < limit; rec += gridDim.x) {
    yfcrop::Chip c;
    if (!yfcrop::find_chip(a.c, rec, &c)) continue;
    const yf_image im = ((const yf_image*)a.c.imgs)[c.frame];
    if (!yfi_image_ok(im.offset, im.height, im.width, im.row_stride, C, a.c.bytes)) continue;
    yf_chip r;
    if (yfi_crop_region(c.rec.x1, c.rec.y1, c.rec.x2, c.rec.y2, im.width, im.height, a.c.margin, a.c.flags, &r) != 0) continue;
    fill_rows<C>(a.px + im.offset + (int64_t)r.y0 * im.row_stride + (int64_t)r.x0 * C, im.row_stride, r.height, r.width, f, lane, wave);
  }
}

template <bool VFIRST>
__global__ void __launch_bounds__(kThreads) fill_yuv_kernel(Args a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  write_status<0>(a);
  uint8_t f[3];
  yfi_redact_fill_bytes(a.colour, VFIRST ? YF_PIX_NV21 : YF_PIX_NV12, f);
  const uint8_t luma[3] = {f[0], f[0], f[0]}, chroma[3] = {f[1], f[2], 0};
  const long limit = records_limit(a);
  for (long rec = blockIdx.x; rec < limit; rec += gridDim.x) {
    yfcrop::Chip c;
    if (!yfcrop::find_chip(a.c, rec, &c)) continue;
    const yf_image_yuv im = ((const yf_image_yuv*)a.c.imgs)[c.frame];
    if (!yfi_yuv_image_ok(im.offset_y, im.offset_uv, im.height, im.width, im.stride_y, im.stride_uv, a.c.bytes)) continue;
    yf_chip r;
    if (yfi_crop_region(c.rec.x1, c.rec.y1, c.rec.x2, c.rec.y2, im.width, im.height, a.c.margin, a.c.flags, &r) != 0) continue;
    fill_rows<1>(a.px + im.offset_y + (int64_t)r.y0 * im.stride_y + r.x0, im.stride_y, r.height, r.width, luma, lane, wave);
    const int cx0 = r.x0 >> 1, cx1 = (r.x0 + r.width - 1) >> 1, cy0 = r.y0 >> 1, cy1 = (r.y0 + r.height - 1) >> 1;
    fill_rows<2>(a.px + im.offset_uv + (int64_t)cy0 * im.stride_uv + 2 * cx0, im.stride_uv, cy1 - cy0 + 1, cx1 - cx0 + 1, chroma, lane, wave);
  }
}

}  // namespace yfredact
#endif
