/* Redaction by blur: every detection record's region of its picture replaced by a coarse grid of its own means, resized back to the
 * region (yf_images_blur_records_device, yf_images_blur_records_yuv_device), shared by the device kernels (yf_images_blur.hip.h), the
 * host entries in yf_images.hip, a host build (yf_images_host.c, libyf_images_host.so, which tests/test_blur_host.py checks against
 * ptq.blur_u8 and ptq.blur_yuv420sp) and the sanitizer program tests/csrc/blur_sanitize_main.c.  Plain C.
 *
 * The reference has no such step; the definition is the library's own.
 *
 * Records, regions, pictures: exactly the redaction's (yf_images_redact.h).  Of frame i the first m_i = yfi_crop_clamp(count, cap) records
 * count; a record's region is yfi_crop_region (margin, YF_CROP_SQUARE, clamp), a record without a region is skipped; the picture of
 * frame i is descriptor i, checked with yfi_image_ok / yfi_yuv_image_ok, and an invalid picture is neither read nor written.
 *
 * Grid: grid = g in [1, YF_BLUR_MAX_GRID].  A region of width x height pixels on a plane with minimum cell m has gx = max(1, min(g,
 * width / m)) columns of cells and gy likewise from height (yfi_blur_cells; integer division).  m = YF_BLUR_MIN_CELL = 4 for packed pixels
 * and the Y plane, YFI_BLUR_MIN_CELL_CHROMA = 2 for the chroma plane.  Without the minimum a region whose sides are <= g would come back
 * byte for byte; with it only a 1 x 1 region keeps its bytes.  Cell cx holds the region's columns [cx * width / gx, (cx + 1) * width / gx)
 * (yfi_blur_cell_at; never empty), rows likewise; column x lies in cell ((x + 1) * gx - 1) / width (yfi_blur_cell_of).
 *
 * Means: per cell and colour byte channel v = (sum + cnt / 2) / cnt over the cell's pixels AS THEY WERE BEFORE THE CALL (yfi_blur_mean,
 * yfi_redact_mean's rule in 64 bits: one cell can hold 16384 x 16384 pixels).  The fourth byte of BGRA / RGBA is neither read nor written.
 *
 * Resample: the region's new content is cv2.resize(G, (width, height)), INTER_LINEAR, of the [gy, gx, channels] grid of means G, as
 * yf_images_taps.h restates it: yfi_axis_tap(d, width, gx), yfi_axis_tap(d, height, gy), yfi_hpass, yfi_vpass (yfi_blur_sample).  A
 * constant region stays constant under these weights.
 *
 * NV12 / NV21: the Y plane is a one-channel picture over the region; the chroma plane a two-channel picture of pairs over the fill's chroma
 * region, cx in [x0 >> 1, (x0 + width - 1) >> 1], cy likewise (yfi_blur_chroma), with its own gx, gy (m = 2), means and resample.  First
 * bytes are averaged together and second bytes together: the blur does not care which of U and V comes first.
 *
 * Overlap: a pixel that lies in several regions of its frame belongs to the LOWEST slot whose region contains it and gets that record's
 * value; on a surface a chroma pair belongs to the lowest slot whose chroma region contains it (two regions that share no pixel can still
 * share a pair).  Every record's grid is computed from the pixels as they were before the call, whoever owns them.  So the order of a
 * frame's records matters only for who owns an overlap.  A second call blurs the blur: unlike the mosaic, the call is NOT idempotent.
 *
 * Workspace: record k = first[f] + s keeps its grid in slot k of the caller's workspace, a slot being g * g cells of four bytes (cell
 * cy * gx + cx; packed: the three means and a 0; surfaces: byte 0 the Y grid's cell, bytes 1 and 2 the chroma grid's cell of the same
 * index).  yfi_blur_workspace(records_cap, g) = records_cap * g * g * 4 rounded up to 16, 0 for arguments the call refuses.  The contents
 * are the library's own.  A record with k >= records_cap has no slot: it is FILLED with `colour` by the fill's rule (yfi_redact_fill_bytes,
 * the fill's chroma region) under the same ownership rule -- a face never stays visible because a buffer was small.  records_cap = 0 is
 * legal and turns the call into a fill.
 *
 * Status of frame f: bit 0 (YFI_BLUR_INVALID) the descriptor is invalid, the picture is untouched; bit 1 (YFI_BLUR_FILLED) the frame has a
 * record without a slot, first[f + 1] > first[f] and first[f + 1] > records_cap -- from d_first and records_cap alone, whether or not
 * that record has a region.  first[n] is the records_cap that would have sufficed.
 *
 * ALIASING.  The pictures of different frames must not share bytes; otherwise the contents are unspecified, but no access leaves a
 * picture's extent as its descriptor states it. */
#ifndef YF_IMAGES_BLUR_H
#define YF_IMAGES_BLUR_H
#include <stddef.h>
#include <stdint.h>
#include "../../include/yf_images.h"
#include "yf_images_crop.h"
#include "yf_images_redact.h"

#define YFI_BLUR_MIN_CELL_CHROMA 2
#define YFI_BLUR_INVALID 1
#define YFI_BLUR_FILLED  2

/* the cells along a side of `side` pixels (pairs, rows) with minimum cell m */
YFI_HD int32_t yfi_blur_cells(int32_t side, int g, int m) {
  const int32_t c = side / m < g ? side / m : g;
  return c < 1 ? 1 : c;
}

/* the first pixel of cell c of `cells` along a side (c = cells: the side); at most 16 * 16384 before the division */
YFI_HD int32_t yfi_blur_cell_at(int32_t c, int32_t side, int32_t cells) { return c * side / cells; }

/* ... and the cell that holds pixel x */
YFI_HD int32_t yfi_blur_cell_of(int32_t x, int32_t side, int32_t cells) { return ((x + 1) * cells - 1) / side; }

/* THE mean */
YFI_HD uint32_t yfi_blur_mean(uint64_t sum, uint64_t cnt) { return (uint32_t)((sum + cnt / 2) / cnt); }

/* the chroma region of a region: pairs and rows of the UV plane, inclusive origin and sizes */
YFI_HD yf_chip yfi_blur_chroma(const yf_chip* r) {
  yf_chip c;
  c.frame = 0; c.slot = 0; c.status = 0;
  c.x0 = r->x0 >> 1; c.y0 = r->y0 >> 1;
  c.width = ((r->x0 + r->width - 1) >> 1) - c.x0 + 1;
  c.height = ((r->y0 + r->height - 1) >> 1) - c.y0 + 1;
  return c;
}

/* THE resample of one byte: byte b of the four cells an output pixel's taps name (c00, c01 of grid row ty.s0 at columns tx.s0, tx.s1;
 * c10, c11 of row ty.s1) */
YFI_HD uint8_t yfi_blur_mix(uint32_t c00, uint32_t c01, uint32_t c10, uint32_t c11, int b, yfi_tap tx, yfi_tap ty) {
  const int sh = 8 * b;
  const int32_t h0 = yfi_hpass((int32_t)(c00 >> sh & 255u), (int32_t)(c01 >> sh & 255u), tx.w0, tx.w1);
  const int32_t h1 = yfi_hpass((int32_t)(c10 >> sh & 255u), (int32_t)(c11 >> sh & 255u), tx.w0, tx.w1);
  return (uint8_t)yfi_vpass(h0, h1, ty.w0, ty.w1);
}

/* ... from the grid: cells[cy * gx + cx] holds a cell's means, byte b of it the channel's; tx, ty the taps of the output pixel */
YFI_HD uint8_t yfi_blur_sample(const uint32_t* cells, int32_t gx, int b, yfi_tap tx, yfi_tap ty) {
  const uint32_t* r0 = cells + ty.s0 * gx;
  const uint32_t* r1 = cells + ty.s1 * gx;
  return yfi_blur_mix(r0[tx.s0], r0[tx.s1], r1[tx.s0], r1[tx.s1], b, tx, ty);
}

/* the bytes of the workspace; 0 for arguments the call refuses */
static inline size_t yfi_blur_workspace(long records_cap, int grid) {
  if (records_cap < 0 || records_cap >= (1l << 31) || grid < 1 || grid > YF_BLUR_MAX_GRID) return 0;
  return ((size_t)records_cap * (size_t)(grid * grid) * 4u + 15u) & ~(size_t)15u;
}

/* what the host can see of a call's arguments, in the order the entry points check them; NULL, or the text of the first fault */
static inline const char* yfi_blur_check(long n, int cap, int grid, uint32_t colour, int margin_permille, int flags, const void* work,
                                         size_t work_bytes, long records_cap) {
  if (n < 0 || n > 2147483646l) return "n must be in [0, 2^31 - 2]";
  if (cap < 1 || cap > YF_IMAGES_NMS_WIDE_MAX_CAP) return "cap must be in [1, 1200]";
  if ((uint64_t)n * (uint64_t)cap >= (1ull << 31)) return "n * cap must be below 2^31";
  if (grid < 1 || grid > YF_BLUR_MAX_GRID) return "grid must be in [1, 16]";
  if ((colour >> 24) != 0) return "colour must be 0x00RRGGBB (0x00YYUUVV): its top byte is not 0";
  if (margin_permille < 0 || margin_permille > 1000) return "margin_permille must be in [0, 1000]";
  if ((flags & ~YF_CROP_SQUARE) != 0) return "flags must be 0 or YF_CROP_SQUARE";
  if (records_cap < 0 || records_cap > n * (long)cap) return "records_cap must be in [0, n * cap]";
  if (work_bytes < yfi_blur_workspace(records_cap, grid)) return "work_bytes is below yf_images_blur_workspace(records_cap, grid)";
  if (yfi_blur_workspace(records_cap, grid) != 0 && (!work || ((uintptr_t)work & 15) != 0)) return "d_work is NULL or not 16-byte aligned";
  return NULL;
}

#endif
