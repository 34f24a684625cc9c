/* Drawing: the outline of every detection record drawn in place into the picture where it lies, in one colour or in a colour per record
 * taken from a palette by a key (yf_images_draw_records_device, yf_images_draw_records_yuv_device), shared by the device kernels
 * (yf_images_draw.hip.h), the host entries in yf_images.hip, a host build (yf_images_host.c, libyf_images_host.so, which
 * tests/test_draw_host.py checks against ptq.draw_rectangles_u8 and ptq.draw_rectangles_yuv420sp) and the sanitizer program
 * tests/csrc/draw_sanitize_main.c.  Plain C.
 *
 * This is where the reference's scripts end: cv2.rectangle(img, (x1, y1), (x2, y2), (0, 0, 255), 2) at
 * yoloface/tflite/tflite_prediction.py:59-64, and four one-pixel lines (LCD_DrawRectangle) in the firmware.
 *
 * Records, pictures, schedule: of frame i the first m_i = yfi_crop_clamp(count, cap) records count; the picture of frame i is descriptor i,
 * checked with yfi_image_ok / yfi_yuv_image_ok -- an invalid one gives status[i] = 1 and is neither read nor written, a valid one
 * status[i] = 0; first[n + 1] is the exclusive prefix of the m_i.  1 <= cap <= 1200, n * cap < 2^31.  All as the redaction.
 *
 * Corners: the record's four int32 edges as they are -- no margin, no square, no clamp, as the reference passes detect[0..3] to
 * cv2.rectangle.  xa = min(x1, x2), xb = max(x1, x2), ya = min(y1, y2), yb = max(y1, y2), in int64 (a YF_DECODE_PY edge can be INT32_MIN).
 *
 * Drawn set of a record, half = h in [0, 3].  For a pixel (x, y):
 *   ex = max(xa - x, x - xb, 0), ey likewise: the distances outside the box;
 *   ix = min(x - xa, xb - x), iy likewise: the distances inside the box.
 * The pixel is drawn iff   ex <= h and ey <= h
 *                    and   ex == 0 or ey == 0 or ex * ex + ey * ey <= h * h       (the outer corners are round)
 *                    and   ex > 0 or ey > 0 or min(ix, iy) <= h                   (the interior stays as it is)
 *                    and   the pixel lies in the picture.
 * yfi_draw_covers holds this.  h = 0 is the one-pixel outline of LCD_DrawRectangle and cv2.rectangle(..., 1).  h = 1 is what OpenCV's
 * drawing.cpp is read to draw for thickness 2 (PolyLine -> ThickLine: a band of three pixels per edge from FillConvexPoly and a filled
 * circle of radius 1 at each corner, so the four outermost corner pixels are missing); that reading is from memory of the source and has
 * NOT been pinned against a real cv2.  h = 2 and h = 3 are the library's own.  A point, a line, a box thinner than 2h + 1 need no special
 * case.
 *
 * The rule looks at the edges only through comparisons with pixels of the picture, so edges far outside say no more than edges just
 * outside: yfi_draw_clip moves every edge into [-(h + 1), side + h] (after the int64 min / max), which changes the answer for no pixel of
 * the picture (an edge at -(h + 1) is already more than h away from column 0 on the inside and not outside any column; one at side + h is
 * more than h beyond the last column), and from there on int32 -- int16 in the kernels' lists -- holds everything.
 *
 * Colour.  Without keys: colour = 0x00RRGGBB (NV12 / NV21: 0x00YYUUVV), a non-zero top byte is refused; the bytes come from
 * yfi_redact_fill_bytes; alpha is never written.  With keys: the colour of the record in slot s of frame f is
 * palette[key % palette_n] & 0xFFFFFF, key the uint32 at keys + (f * cap + s) * key_stride; key_stride a multiple of 4 in [4, 64] (the id
 * field of a yf_track_info array is passed as it lies, with stride 16), 1 <= palette_n <= 256; the palette's top bytes are ignored.
 *
 * Overlap: a pixel drawn by several records of its frame gets the colour of the HIGHEST slot that draws it -- what drawing them in slot
 * order gives.  Without keys all writers write the same bytes.
 *
 * NV12 / NV21: the Y byte of every drawn pixel; a chroma pair (cx, cy) is written iff at least one of its four luma pixels (2cx + {0, 1},
 * 2cy + {0, 1}) is drawn, and takes the chroma of the highest slot that draws any of them; (U, V) for NV12, (V, U) for NV21.  Nothing else
 * is written, row padding included.
 *
 * ALIASING.  With keys the pictures of different frames must not share bytes (otherwise unspecified contents, but never an access outside
 * an extent); without keys pictures may be shared. */
#ifndef YF_IMAGES_DRAW_H
#define YF_IMAGES_DRAW_H
#include <stddef.h>
#include <stdint.h>
#include "../../include/yf_images.h"
#include "yf_images_crop.h"
#include "yf_images_redact.h"

#define YFI_DRAW_MAX_HALF     3
#define YFI_DRAW_MAX_PALETTE  256
#define YFI_DRAW_MAX_STRIDE   64

/* a record's edges, ordered and moved into [-(h + 1), W + h] x [-(h + 1), H + h] */
typedef struct yfi_draw_edges { int32_t xa, ya, xb, yb; } yfi_draw_edges;

YFI_HD int32_t yfi_draw_clip1(int64_t v, int h, int32_t side) {
  const int64_t lo = -(int64_t)(h + 1), hi = (int64_t)side + h;
  return (int32_t)(v < lo ? lo : (v > hi ? hi : v));
}

YFI_HD yfi_draw_edges yfi_draw_clip(int32_t x1, int32_t y1, int32_t x2, int32_t y2, int h, int32_t W, int32_t H) {
  const int64_t xa = x1 < x2 ? x1 : x2, xb = x1 < x2 ? x2 : x1, ya = y1 < y2 ? y1 : y2, yb = y1 < y2 ? y2 : y1;
  yfi_draw_edges e;
  e.xa = yfi_draw_clip1(xa, h, W); e.xb = yfi_draw_clip1(xb, h, W);
  e.ya = yfi_draw_clip1(ya, h, H); e.yb = yfi_draw_clip1(yb, h, H);
  return e;
}

/* THE rule, for a pixel (x, y) of the picture (0 <= x < W, 0 <= y < H: the caller's part of it) */
YFI_HD int yfi_draw_covers(const yfi_draw_edges* e, int h, int32_t x, int32_t y) {
  const int32_t ax = e->xa - x, bx = x - e->xb, ay = e->ya - y, by = y - e->yb;
  const int32_t ex = ax > 0 ? ax : (bx > 0 ? bx : 0), ey = ay > 0 ? ay : (by > 0 ? by : 0);
  if (ex > h || ey > h) return 0;
  if (ex != 0 && ey != 0) return ex * ex + ey * ey <= h * h;
  if (ex != 0 || ey != 0) return 1;
  const int32_t ix = -ax < -bx ? -ax : -bx, iy = -ay < -by ? -ay : -by;
  return (ix < iy ? ix : iy) <= h;
}

/* whether the record draws anything at all in a picture of W x H: its outer box meets the picture, and the picture does not lie wholly in
 * the interior that stays as it is */
YFI_HD int yfi_draw_visible(const yfi_draw_edges* e, int h, int32_t W, int32_t H) {
  if (e->xa - h > W - 1 || e->xb + h < 0 || e->ya - h > H - 1 || e->yb + h < 0) return 0;
  return !(e->xa + h < 0 && e->xb - h > W - 1 && e->ya + h < 0 && e->yb - h > H - 1);
}

/* an inclusive span of rows or columns; n < 1: empty */
typedef struct yfi_draw_span { int32_t at, n; } yfi_draw_span;

YFI_HD yfi_draw_span yfi_draw_span_of(int32_t lo, int32_t hi, int32_t side) {
  yfi_draw_span s;
  if (lo < 0) lo = 0;
  if (hi > side - 1) hi = side - 1;
  s.at = lo; s.n = hi - lo + 1;
  if (s.n < 0) s.n = 0;
  return s;
}

/* The four bands of a record, clipped to the picture: every drawn pixel lies in exactly one of them.  The horizontal bands are the rows
 * `top` and `bottom` over the columns `across` (the corner pixels are theirs); the vertical bands are the rows `between` over the columns
 * `left` and `right`.  A thin box's bands run into each other: the later one starts behind the earlier one. */
typedef struct yfi_draw_bands { yfi_draw_span top, bottom, between, across, left, right; } yfi_draw_bands;

YFI_HD yfi_draw_bands yfi_draw_bands_of(const yfi_draw_edges* e, int h, int32_t W, int32_t H) {
  yfi_draw_bands b;
  const int32_t t1 = e->ya + h, b0 = e->yb - h > t1 + 1 ? e->yb - h : t1 + 1;
  const int32_t l1 = e->xa + h, r0 = e->xb - h > l1 + 1 ? e->xb - h : l1 + 1;
  b.top = yfi_draw_span_of(e->ya - h, t1, H);
  b.bottom = yfi_draw_span_of(b0, e->yb + h, H);
  b.between = yfi_draw_span_of(t1 + 1, b0 - 1, H);
  b.across = yfi_draw_span_of(e->xa - h, e->xb + h, W);
  b.left = yfi_draw_span_of(e->xa - h, l1, W);
  b.right = yfi_draw_span_of(r0, e->xb + h, W);
  return b;
}

/* the colour of a keyed record */
YFI_HD uint32_t yfi_draw_key_colour(uint32_t key, const uint32_t* palette, int palette_n) {
  return palette[key % (uint32_t)palette_n] & 0xFFFFFFu;
}

/* what the host can see of a call's arguments, in the order the entry points check them; NULL, or the text of the first fault */
static inline const char* yfi_draw_check(long n, int cap, int half, uint32_t colour, const void* keys, int key_stride, const void* palette,
                                         int palette_n) {
  if (n < 0 || n > 2147483646l) return "n must be in [0, 2^31 - 2]";
  if (cap < 1 || cap > YF_IMAGES_NMS_WIDE_MAX_CAP) return "cap must be in [1, 1200]";
  if ((uint64_t)n * (uint64_t)cap >= (1ull << 31)) return "n * cap must be below 2^31";
  if (half < 0 || half > YFI_DRAW_MAX_HALF) return "half must be in [0, 3]";
  if (!keys) {
    if ((colour >> 24) != 0) return "colour must be 0x00RRGGBB (0x00YYUUVV): its top byte is not 0";
    if (key_stride != 0 || palette != NULL || palette_n != 0) return "without d_keys, key_stride, d_palette and palette_n must be 0, NULL and 0";
    return NULL;
  }
  if (key_stride < 4 || key_stride > YFI_DRAW_MAX_STRIDE || key_stride % 4 != 0) return "key_stride must be a multiple of 4 in [4, 64]";
  if (!palette) return "d_palette is NULL with d_keys given";
  if (palette_n < 1 || palette_n > YFI_DRAW_MAX_PALETTE) return "palette_n must be in [1, 256]";
  if ((((uintptr_t)keys | (uintptr_t)palette) & 3) != 0) return "d_keys and d_palette must be 4-byte aligned";
  return NULL;
}

#endif
