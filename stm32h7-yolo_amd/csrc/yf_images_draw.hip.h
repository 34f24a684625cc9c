// The kernels of libyf_images.so that draw detections in place (yf_images_draw_records_device, yf_images_draw_records_yuv_device): the
// outline of every record in its picture, in one colour or in a colour per record (the rule: yf_images_draw.h).  Included once by
// yf_images.hip, behind yf_images_redact.hip.h; C-ABI and semantics: include/yf_images.h.
//
// Two launches.  The first is the crop's scan, yfcrop::first_kernel.  The second is one 256-thread workgroup per record, grid-striding
// over first[n], exactly as the redaction's: yfcrop::find_chip gives the record's (frame, slot), and the first pass over the frames
// writes d_status (yfredact::write_status).
//
// What a record costs follows the pixels it writes, never its int32 edges: the edges are clipped to just outside the picture
// (yfi_draw_clip), a record that draws nothing there leaves at once (yfi_draw_visible: wholly outside, or the picture wholly in its
// interior), and the loops run over the clipped spans of the four bands (yfi_draw_bands_of) only.  The horizontal bands are rows of
// consecutive bytes: a wave takes a row, consecutive lanes consecutive bytes, as the redaction's fill_rows.  The vertical bands are
// 2h + 1 pixels per row: the rows lie across the workgroup's lanes.  The corner pixels belong to the horizontal bands, so every pixel
// is written by one lane.  Every lane asks yfi_draw_covers for its pixel: that rounds the corners, and keeps a thin box's interior right.
//
// Ownership with keys: a pixel drawn by several records of a frame belongs to the highest slot.  The workgroup of slot s walks the
// records s' > s of its frame (lanes striding) and keeps those that draw something and whose clipped outer box meets its own as four
// int16 in LDS (edges clipped to [-(h + 1), side + h] fit; at most cap - 1 = 1199 entries, 9.6 KB, appended through an LDS counter); a
// lane skips a pixel -- or a chroma pair -- that an entry covers (the entry is the same for all lanes: an LDS broadcast).  This is the
// redaction's earlier_owners / owned_earlier turned round.  The list is usually empty; its cost is bounded by cap, never by the
// picture.  Without keys every writer writes the same bytes and the walk is skipped altogether.
//
// NV12 / NV21: the Y plane is a packed plane of one byte per pixel.  The chroma plane is walked by the same bands in halved
// coordinates (a chroma row that holds a row of a horizontal band is a row of the chroma's horizontal band); a pair is written iff one
// of its four luma pixels is drawn by this record and none of them by a listed one.  For surfaces the outer boxes are grown to even
// bounds before they are compared, so that records which share only a chroma pair are listed too.
//
// Offsets and strides carry no alignment: every store is one byte wide.  Nothing is loaded from a picture.
//
// Safety: d_counts, d_dets, d_first read back, d_keys and d_palette are device memory that may hold anything.  find_chip admits a record
// only inside its frame's range and clamped count; the later slots walked lie below the same clamped count; a key is reduced modulo
// palette_n (1 .. 256, checked on the host) before it indexes the palette; every span is clipped to [0, W - 1] x [0, H - 1], which
// yfi_image_ok / yfi_yuv_image_ok have tied to the buffer's size (W and H even for surfaces, so a chroma pair of a luma pixel in the
// picture lies in the chroma plane): no store leaves a picture's or plane's extent as its descriptor states it.
#ifndef YF_IMAGES_DRAW_HIP_H
#define YF_IMAGES_DRAW_HIP_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/yf_images.h"
#include "yf_images_draw.h"
#include "yf_images_redact.hip.h"

namespace yfdraw {

constexpr int kThreads = yfredact::kThreads;
constexpr int kWaves = kThreads / 64;
constexpr int kListCap = YF_IMAGES_NMS_WIDE_MAX_CAP - 1;  // the records behind the first slot
static_assert(YF_IMAGES_MAX_SIDE + YFI_DRAW_MAX_HALF <= 32767, "a clipped edge in 16 bits");

struct Args {
  yfredact::Args r;                                       // what find_chip, write_status and records_limit read; px, format, colour, status
  int half;
  const uint8_t* keys;                                    // NULL: one colour
  int key_stride;
  const uint32_t* palette;
  int palette_n;
};

// the colour of the record in slot c.slot of frame c.frame
__device__ __forceinline__ uint32_t colour_of(const Args& a, const yfcrop::Chip& c) {
  if (!a.keys) return a.r.colour;
  const uint32_t key = *(const uint32_t*)(a.keys + (c.frame * (int64_t)a.r.c.cap + c.slot) * (int64_t)a.key_stride);
  return yfi_draw_key_colour(key, a.palette, a.palette_n);
}

// The records behind slot c.slot of its frame that draw something and whose clipped outer box (grown to even bounds with EVEN) meets
// that of `mine`, into s_list; -> their number.  Every thread of the workgroup calls it.
template <bool EVEN>
__device__ __forceinline__ int later_owners(const Args& a, const yfcrop::Chip& c, int W, int H, const yfi_draw_edges& mine, short4* s_list,
                                            int* s_ctl) {
  const int h = a.half, grow = EVEN ? 1 : 0;
  __syncthreads();                                        // the previous record's readers of the list are done
  if (threadIdx.x == 0) s_ctl[0] = 0;
  __syncthreads();
  const int m = yfi_crop_clamp(a.r.c.counts[c.frame], a.r.c.cap);
  const yf_det* row = a.r.c.dets + c.frame * a.r.c.cap;
  const int mx0 = (mine.xa - h) & ~grow, mx1 = (mine.xb + h) | grow, my0 = (mine.ya - h) & ~grow, my1 = (mine.yb + h) | grow;
  for (int s = c.slot + 1 + (int)threadIdx.x; s < m; s += kThreads) {
    const yf_det d = row[s];
    const yfi_draw_edges e = yfi_draw_clip(d.x1, d.y1, d.x2, d.y2, h, W, H);
    if (!yfi_draw_visible(&e, h, W, H)) continue;
    if (((e.xb + h) | grow) < mx0 || ((e.xa - h) & ~grow) > mx1 || ((e.yb + h) | grow) < my0 || ((e.ya - h) & ~grow) > my1) continue;
    const int at = atomicAdd(&s_ctl[0], 1);
    if (at < kListCap) s_list[at] = make_short4((short)e.xa, (short)e.ya, (short)e.xb, (short)e.yb);
  }
  __syncthreads();
  return s_ctl[0] < kListCap ? s_ctl[0] : kListCap;
}

// whether a listed record draws pixel (x, y)
__device__ __forceinline__ bool taken(const short4* s_list, int listed, int h, int x, int y) {
  for (int q = 0; q < listed; ++q) {
    const short4 v = s_list[q];
    const yfi_draw_edges e{v.x, v.y, v.z, v.w};
    if (yfi_draw_covers(&e, h, x, y)) return true;
  }
  return false;
}

// An element of a plane and whether this record writes it.  Luma (and packed pixels): element (x, y) is the pixel.  Chroma: element
// (x, y) is the pair of the luma pixels (2x + {0, 1}, 2y + {0, 1}), all four of which lie in the (even-sided) surface.
struct Pixels {
  yfi_draw_edges e;
  int h, listed;
  const short4* list;
  __device__ __forceinline__ bool writes(int x, int y) const { return yfi_draw_covers(&e, h, x, y) && !taken(list, listed, h, x, y); }
};
struct Pairs {
  yfi_draw_edges e;
  int h, listed;
  const short4* list;
  __device__ __forceinline__ bool writes(int x, int y) const {
    const int lx = 2 * x, ly = 2 * y;
    if (!(yfi_draw_covers(&e, h, lx, ly) || yfi_draw_covers(&e, h, lx + 1, ly) || yfi_draw_covers(&e, h, lx, ly + 1) ||
          yfi_draw_covers(&e, h, lx + 1, ly + 1)))
      return false;
    for (int q = 0; q < listed; ++q) {                    // one walk for the four
      const short4 v = list[q];
      const yfi_draw_edges o{v.x, v.y, v.z, v.w};
      if (yfi_draw_covers(&o, h, lx, ly) || yfi_draw_covers(&o, h, lx + 1, ly) || yfi_draw_covers(&o, h, lx, ly + 1) ||
          yfi_draw_covers(&o, h, lx + 1, ly + 1))
        return false;
    }
    return true;
  }
};

// The bands `b` of a plane whose elements are C bytes, of which the first NC get f[]: the rows b.top and b.bottom over the columns
// b.across, a wave per row and consecutive lanes consecutive bytes (with listed records, consecutive elements: the walk of the list is
// then made once per element); the rows b.between over the columns b.left and b.right, a row per lane.  Every span lies inside the plane.
template <int C, int NC, class What>
__device__ __forceinline__ void draw_bands(uint8_t* p, int64_t stride, const yfi_draw_bands& b, const uint8_t* f, const What& w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (b.across.n > 0)
    for (int k = wave; k < b.top.n + b.bottom.n; k += kWaves) {
      const int y = k < b.top.n ? b.top.at + k : b.bottom.at + (k - b.top.n);
      uint8_t* q = p + (int64_t)y * stride + (int64_t)b.across.at * C;
      if (w.listed == 0) {
        for (int j = lane; j < b.across.n * C; j += 64) {
          const int dx = j / C, ch = j - dx * C;
          if (ch < NC && w.writes(b.across.at + dx, y)) q[j] = ch == 0 ? f[0] : ch == 1 ? f[1] : f[2];
        }
      } else {                                            // a list to walk: once per element, not once per byte
        for (int dx = lane; dx < b.across.n; dx += 64)
          if (w.writes(b.across.at + dx, y)) {
#pragma unroll
            for (int ch = 0; ch < NC; ++ch) q[dx * C + ch] = f[ch];
          }
      }
    }
  if (b.left.n > 0 || b.right.n > 0)
    for (int k = threadIdx.x; k < b.between.n; k += kThreads) {
      const int y = b.between.at + k;
      uint8_t* q = p + (int64_t)y * stride;
      for (int side = 0; side < 2; ++side) {
        const yfi_draw_span s = side ? b.right : b.left;
        for (int x = s.at; x < s.at + s.n; ++x)
          if (w.writes(x, y)) {
#pragma unroll
            for (int ch = 0; ch < NC; ++ch) q[(int64_t)x * C + ch] = f[ch];
          }
      }
    }
}

// the bands of the chroma plane from those of the luma plane: every span in halved coordinates, and a chroma row or column that two
// spans share stays with the first of them (top before bottom before between; left before right)
__device__ __forceinline__ yfi_draw_span halved(const yfi_draw_span& s) {
  yfi_draw_span o;
  o.at = s.at >> 1;
  o.n = s.n > 0 ? ((s.at + s.n - 1) >> 1) - o.at + 1 : 0;
  return o;
}
__device__ __forceinline__ void start_behind(yfi_draw_span& s, const yfi_draw_span& first) {
  if (s.n <= 0 || first.n <= 0) return;
  const int end = s.at + s.n, at = first.at + first.n > s.at ? first.at + first.n : s.at;
  s.at = at;
  s.n = end - at > 0 ? end - at : 0;
}
__device__ __forceinline__ void end_before(yfi_draw_span& s, const yfi_draw_span& last) {
  if (s.n <= 0 || last.n <= 0) return;
  const int end = last.at < s.at + s.n ? last.at : s.at + s.n;
  s.n = end - s.at > 0 ? end - s.at : 0;
}
__device__ __forceinline__ yfi_draw_bands chroma_bands(const yfi_draw_bands& b) {
  yfi_draw_bands c;
  c.top = halved(b.top); c.bottom = halved(b.bottom); c.between = halved(b.between);
  c.across = halved(b.across); c.left = halved(b.left); c.right = halved(b.right);
  start_behind(c.between, c.top);                         // top, between and bottom are in ascending order, and so are left and right
  end_before(c.between, c.bottom);
  start_behind(c.bottom, c.top);
  start_behind(c.right, c.left);
  return c;
}

// C: bytes per pixel of a packed format
template <int C>
__global__ void __launch_bounds__(kThreads) outline_kernel(Args a) {
  __shared__ short4 s_list[kListCap];
  __shared__ int s_ctl[1];
  yfredact::write_status<C>(a.r);
  const int h = a.half;
  const long limit = yfredact::records_limit(a.r);
  for (long rec = blockIdx.x; rec < limit; rec += gridDim.x) {
    yfcrop::Chip c;
    if (!yfcrop::find_chip(a.r.c, rec, &c)) continue;
    const yf_image im = ((const yf_image*)a.r.c.imgs)[c.frame];
    if (!yfi_image_ok(im.offset, im.height, im.width, im.row_stride, C, a.r.c.bytes)) continue;
    const yfi_draw_edges e = yfi_draw_clip(c.rec.x1, c.rec.y1, c.rec.x2, c.rec.y2, h, im.width, im.height);
    if (!yfi_draw_visible(&e, h, im.width, im.height)) continue;
    const int listed = a.keys ? later_owners<false>(a, c, im.width, im.height, e, s_list, s_ctl) : 0;
    uint8_t f[3];
    yfi_redact_fill_bytes(colour_of(a, c), a.r.format, f);
    const yfi_draw_bands b = yfi_draw_bands_of(&e, h, im.width, im.height);
    draw_bands<C, 3>(a.r.px + im.offset, im.row_stride, b, f, Pixels{e, h, listed, s_list});
  }
}

template <bool VFIRST>
__global__ void __launch_bounds__(kThreads) outline_yuv_kernel(Args a) {
  __shared__ short4 s_list[kListCap];
  __shared__ int s_ctl[1];
  yfredact::write_status<0>(a.r);
  const int h = a.half;
  const long limit = yfredact::records_limit(a.r);
  for (long rec = blockIdx.x; rec < limit; rec += gridDim.x) {
    yfcrop::Chip c;
    if (!yfcrop::find_chip(a.r.c, rec, &c)) continue;
    const yf_image_yuv im = ((const yf_image_yuv*)a.r.c.imgs)[c.frame];
    if (!yfi_yuv_image_ok(im.offset_y, im.offset_uv, im.height, im.width, im.stride_y, im.stride_uv, a.r.c.bytes)) continue;
    const yfi_draw_edges e = yfi_draw_clip(c.rec.x1, c.rec.y1, c.rec.x2, c.rec.y2, h, im.width, im.height);
    if (!yfi_draw_visible(&e, h, im.width, im.height)) continue;
    const int listed = a.keys ? later_owners<true>(a, c, im.width, im.height, e, s_list, s_ctl) : 0;
    uint8_t f[3];
    yfi_redact_fill_bytes(colour_of(a, c), VFIRST ? YF_PIX_NV21 : YF_PIX_NV12, f);
    const uint8_t chroma[3] = {f[1], f[2], 0};
    const yfi_draw_bands b = yfi_draw_bands_of(&e, h, im.width, im.height);
    draw_bands<1, 1>(a.r.px + im.offset_y, im.stride_y, b, f, Pixels{e, h, listed, s_list});
    draw_bands<2, 2>(a.r.px + im.offset_uv, im.stride_uv, chroma_bands(b), chroma, Pairs{e, h, listed, s_list});
  }
}

}  // namespace yfdraw
#endif
