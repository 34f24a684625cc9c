/* Tiled detection: the tile grid of an image, the translation of a tile's record to its image's pixels and the rule of the merge
 * (yf_images_plan_tiles, yf_images_gather_tiles_device), shared by the device kernels (yf_images_tiles.hip.h), the host entry in
 * yf_images.hip and a host build (yf_images_host.c, libyf_images_host.so, which tests/test_tiles_host.py checks against a plain-Python
 * restatement).  Plain C.
 *
 * The reference has no tiling: its callers squeeze a whole photograph into one 56x56 frame.  Everything here -- the grid, the order of
 * the tiles, the order of the merged records, the saturation of a translated edge -- is the library's own definition, as the tie rules of
 * the suppression and of the scoring are.
 *
 * Grid, per axis, of length L with tile side T >= 1 and stride 1 <= S <= T:
 *   L <= T:   one tile, [0, L).
 *   L >  T:   k = (L - T + S - 1) / S + 1 tiles of side T; origin i * S for i < k - 1, and L - T for the last one, which is flush with
 *             the edge, so no tile is short.  (k - 2) * S < L - T <= (k - 1) * S: the origins ascend strictly and every pixel is covered.
 * An image's tiles are in row-major order (y outer, x inner).  With `whole`, an image whose grid has more than one tile gets one more
 * region in front of them: the whole image (origin 0, 0, H x W), which keeps the faces that fill the picture.  A one-tile grid already is
 * the whole image and is not doubled.
 *
 * Merge: image i owns the tiles first[i] <= j < first[i + 1]; its records are those tiles' records in ascending j, each tile's first
 * m_j = min(max(count, 0), cap) in their order.  A merged record is the tile's record with frame = i and the edges moved by the tile's
 * origin: the sum in int64, clamped to int32 (an INT32_MIN edge of YF_DECODE_PY moves by the origin; a saturated INT32_MAX edge of
 * YF_DECODE_FW stays, for an origin >= 0). */
#ifndef YF_IMAGES_TILES_H
#define YF_IMAGES_TILES_H
#include <stddef.h>
#include <stdint.h>
#include "../../include/yf_images.h"
#ifndef YFI_HD
#ifdef __HIPCC__
#define YFI_HD __host__ __device__ __forceinline__
#else
#define YFI_HD static inline
#endif
#endif

/* ---- the grid along one axis ---- */
YFI_HD int32_t yfi_tiles_axis_count(int32_t L, int32_t T, int32_t S) { return L <= T ? 1 : (L - T + S - 1) / S + 1; }
YFI_HD int32_t yfi_tiles_axis_side(int32_t L, int32_t T) { return L <= T ? L : T; }
/* origin of tile i of k = yfi_tiles_axis_count(L, T, S) */
YFI_HD int32_t yfi_tiles_axis_origin(int32_t L, int32_t T, int32_t S, int32_t i, int32_t k) {
  if (L <= T) return 0;
  return i < k - 1 ? i * S : L - T;
}

/* ---- the merge ---- */
/* the records of a tile that count: min(max(count, 0), cap), the suppression's clamp */
YFI_HD int32_t yfi_tiles_clamp(int32_t count, int32_t cap) { return count < 0 ? 0 : (count > cap ? cap : count); }

/* an edge moved by an origin: int64 sum, clamped to int32 */
YFI_HD int32_t yfi_tiles_shift(int32_t edge, int32_t origin) {
  const int64_t s = (int64_t)edge + (int64_t)origin;
  return s > (int64_t)INT32_MAX ? INT32_MAX : (s < (int64_t)INT32_MIN ? INT32_MIN : (int32_t)s);
}

/* THE translation: dword q (0..6) of a yf_det of a tile at (x0, y0), as the merged record of image `image` holds it.  Dword 0 is the
 * frame, 1 anchor / row / col / q_conf, 2 conf, 3..6 x1, y1, x2, y2. */
YFI_HD uint32_t yfi_tiles_dword(uint32_t v, int q, int32_t image, int32_t x0, int32_t y0) {
  if (q == 0) return (uint32_t)image;
  if (q == 3 || q == 5) return (uint32_t)yfi_tiles_shift((int32_t)v, x0);
  if (q == 4 || q == 6) return (uint32_t)yfi_tiles_shift((int32_t)v, y0);
  return v;
}

/* ---- the planner (host only): yf_images_plan_tiles of include/yf_images.h, with the error text returned through *err ---- */
static inline int yfi_tiles_channels(int format) {
  return format == YF_PIX_BGR8 || format == YF_PIX_RGB8 ? 3 : (format == YF_PIX_BGRA8 || format == YF_PIX_RGBA8 ? 4 : 0);
}

static inline long yfi_plan_tiles(const yf_image* images, long n, int format, int tile_h, int tile_w, int stride_y, int stride_x, int whole,
                                  yf_tile* tiles, yf_image* tile_images, int32_t* first, long tiles_cap, const char** err) {
  const int C = yfi_tiles_channels(format);
  *err = "";
  if (!C) { *err = "format must be YF_PIX_BGR8, YF_PIX_RGB8, YF_PIX_BGRA8 or YF_PIX_RGBA8"; return -1; }
  if (n < 0) { *err = "n < 0"; return -1; }
  if (n > 0 && !images) { *err = "images is NULL"; return -1; }
  if (tile_h < 1 || tile_w < 1) { *err = "tile_h and tile_w must be at least 1"; return -1; }
  if (stride_y < 1 || stride_y > tile_h || stride_x < 1 || stride_x > tile_w) { *err = "a stride must be in [1, tile side]"; return -1; }
  if (tiles && (!tile_images || !first)) { *err = "tile_images and first must be given with tiles"; return -1; }
  if (tiles && tiles_cap < 0) { *err = "tiles_cap < 0"; return -1; }
  int64_t t = 0;
  for (long i = 0; i < n; ++i) {
    const int32_t H = images[i].height, W = images[i].width;
    if (H < 1 || W < 1 || H > YF_IMAGES_MAX_SIDE || W > YF_IMAGES_MAX_SIDE) { *err = "an image's height and width must be in [1, 16384]"; return -1; }
    const int32_t ky = yfi_tiles_axis_count(H, tile_h, stride_y), kx = yfi_tiles_axis_count(W, tile_w, stride_x);
    const int64_t grid = (int64_t)ky * kx;
    t += grid + (whole && grid > 1 ? 1 : 0);
    if (t >= ((int64_t)1 << 31)) { *err = "2^31 tiles or more"; return -1; }
  }
  if (!tiles) return (long)t;
  if (t > (int64_t)tiles_cap) { *err = "more tiles than tiles_cap"; return -1; }
  long j = 0;
  for (long i = 0; i < n; ++i) {
    const yf_image p = images[i];
    const int32_t H = p.height, W = p.width;
    const int32_t ky = yfi_tiles_axis_count(H, tile_h, stride_y), kx = yfi_tiles_axis_count(W, tile_w, stride_x);
    const int32_t th = yfi_tiles_axis_side(H, tile_h), tw = yfi_tiles_axis_side(W, tile_w);
    first[i] = (int32_t)j;
    for (int32_t r = (whole && (int64_t)ky * kx > 1) ? -1 : 0; r < ky; ++r)
      for (int32_t c = 0; c < (r < 0 ? 1 : kx); ++c, ++j) {
        yf_tile q;
        q.image = (int32_t)i;
        q.x0 = r < 0 ? 0 : yfi_tiles_axis_origin(W, tile_w, stride_x, c, kx);
        q.y0 = r < 0 ? 0 : yfi_tiles_axis_origin(H, tile_h, stride_y, r, ky);
        q.height = r < 0 ? H : th;
        q.width = r < 0 ? W : tw;
        tiles[j] = q;
        tile_images[j].offset = p.offset + (uint64_t)q.y0 * (uint64_t)p.row_stride + (uint64_t)q.x0 * (uint64_t)C;
        tile_images[j].height = q.height;
        tile_images[j].width = q.width;
        tile_images[j].row_stride = p.row_stride;
      }
  }
  first[n] = (int32_t)j;
  return (long)t;
}

#endif
