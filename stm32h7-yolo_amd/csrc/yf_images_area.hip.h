// The kernels of libyf_images.so behind area-averaged frames (csrc/yf_images_area.h: the weights, the pixel, the fit).  Included once by
// yf_images.hip; C-ABI and semantics: include/yf_images.h.
//
// The work of a frame is its SOURCE bytes, so the plan is not the linear prepare's (one workgroup per frame, single bytes through tap
// tables): a frame is split into `bands` bands of whole output rows (yfi_area_bands: from n and out_hw alone) and a workgroup
// takes (frame, band) jobs, grid-striding.  A job reads only the source rows its output rows overlap; neighbouring rows (and so bands)
// share at most one source row.  Inside a job, per output row:
//   stage    the source rows of the output row's span, up to 16 KB (at 160: 32 KB) at a time (and, for rows wider than 8 KB, a range
//            of columns at a time), go to LDS by 16-byte loads that lie wholly inside the row's bytes -- the unaligned head and tail
//            of a row byte by byte --, each row at its own phase of 16, so that the LDS stores are aligned too;
//   reduce   thread t owns element t of the output row (column t / 3, channel t % 3; 256 threads at 56, 512 at 160): it sums its
//            column's span of each staged row out of LDS -- the first and the last source with their weights, the ones between
//            unweighted and times n_out once: a read and an add per source byte -- into 32 bits, and adds the row's sum times the
//            row's weight to its 64-bit accumulator;
//   divide   one 64-bit division per output element; the pair of output rows is staged in LDS and written with 16-byte stores.
// Integer sums do not depend on the order of addition, so neither the split into bands nor the staging by rows and column ranges shows
// in the frame.  A padded row or column of a letterboxed frame loads nothing.  NV12 / NV21: a source row is its Y row and its UV row;
// a thread converts its channel of every pixel of its span (yf_images_yuv.h: the luma term plus the pair's term of that channel).
#ifndef YF_IMAGES_AREA_HIP_H
#define YF_IMAGES_AREA_HIP_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/yf_images.h"
#include "yf_images_area.h"
#include "yf_images_yuv.h"
#include "yf_images_float.h"

namespace yfarea {

// threads of a workgroup: one per element of an output row (168 of 256 at 56, 480 of 512 at 160)
constexpr int threads_of(int out) { return out == 56 ? 256 : 512; }
// the staged source rows: 16 KB for the 256 threads of a 56 frame, 32 KB for the 512 of a 160 frame -- 32 waves per CU either way
constexpr int tile_bytes_of(int out) { return out == 56 ? 16384 : 32768; }
constexpr int per_cu_of(int out) { return out == 56 ? 8 : 4; }

struct Args {
  const uint8_t* px;
  uint64_t bytes;
  const void* imgs;            // yf_image[n], or yf_image_yuv[n] for the surfaces' kernels
  int32_t* status;
  long n;
  void* frames;                // int8, or fp16 bits
  int pad;                     // 0..255
  int fit;                     // YF_FIT_STRETCH, YF_FIT_LETTERBOX
  int bands;                   // per frame
};

template <int THREADS>
__device__ __forceinline__ void fill(int4* out, int vecs, int v, int tid) {
  for (int q = tid; q < vecs; q += THREADS) out[q] = make_int4(v, v, v, v);
}

// One staged line: `len` bytes from `src` to tile + at + ((uintptr_t)src & 15) + (0 .. len), vector i of the line by this thread.
__device__ __forceinline__ void stage_vector(uint8_t* tile, int at, const uint8_t* src, int len, int i) {
  const int phase = (int)((uintptr_t)src & 15);
  const int lo = 16 * i - phase;                 // the vector's first byte, relative to the line
  if (lo >= 0 && lo + 16 <= len) {
    *(int4*)(tile + at + 16 * i) = *(const int4*)(src + lo);
    return;
  }
  if (lo >= len) return;                         // past the line: the last vector of a pitch that a smaller phase does not need
  // the head or the tail of a line, byte by byte, four at a time: every load at an address inside the line (clamped) and none behind
  // a branch, so that the four are in flight together; then the stores of the bytes that belong to the line
#pragma unroll 1
  for (int q0 = 0; q0 < 16; q0 += 4) {
    uint8_t v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int b = lo + q0 + q;
      v[q] = src[b < 0 ? 0 : (b < len ? b : len - 1)];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int b = lo + q0 + q;
      if (b >= 0 && b < len) tile[at + 16 * i + q0 + q] = v[q];
    }
  }
}

// FMT: the format's code (0 BGR8, 1 RGB8, 2 BGRA8, 3 RGBA8, 4 NV12, 5 NV21); T: the frame's element, int8_t or uint16_t (fp16 bits)
template <int OUT, int FMT, typename T>
__global__ void __launch_bounds__(threads_of(OUT)) area_kernel(Args a) {
  constexpr int kThreads = threads_of(OUT), kTileBytes = tile_bytes_of(OUT);
  constexpr bool YUV = FMT >= 4, VFIRST = FMT == 5, BGR = FMT == 0 || FMT == 2, F16 = sizeof(T) == 2;
  constexpr int C = YUV ? 1 : (FMT < 2 ? 3 : 4);
  constexpr int ITEMS = OUT * 3, K = (ITEMS + kThreads - 1) / kThreads;
  constexpr int ROW_BYTES = ITEMS * (int)sizeof(T), PAIR_VECS = 2 * ROW_BYTES / 16, FRAME_BYTES = OUT * ROW_BYTES;
  // pixels of a row staged at once: at most 8 KB a line; one packed line, three lines of a surface fit the smaller tile
  constexpr int CHUNK = YUV ? 4096 : 2048;
  static_assert((2 * ROW_BYTES) % 16 == 0 && OUT % 2 == 0, "pairs of rows are whole 16-byte vectors");
  __shared__ int4 s_tile[kTileBytes / 16];
  __shared__ int4 s_stage[PAIR_VECS];
  __shared__ uint16_t s_half[F16 ? 256 : 1];       // the 256 halves, as the other fp16 prepares keep them: a look-up, no branch per element
  uint8_t* tile = (uint8_t*)s_tile;
  const int tid = threadIdx.x;
  if constexpr (F16) {
    static_assert(!F16 || kThreads == 256, "one half per thread");
    s_half[tid] = yfi_f16_of_u8(tid);
    __syncthreads();
  }
  const long jobs = a.n * a.bands;
  for (long j = blockIdx.x; j < jobs; j += gridDim.x) {
    const long f = j / a.bands;
    const int band = (int)(j - f * a.bands);
    const int r0 = yfi_area_band_row(band, a.bands, OUT), r1 = yfi_area_band_row(band + 1, a.bands, OUT);
    int h, w;
    int64_t rs, rs_uv = 0;
    uint64_t off, off_uv = 0;
    bool ok;
    if constexpr (YUV) {
      const yf_image_yuv im = ((const yf_image_yuv*)a.imgs)[f];
      h = im.height; w = im.width; rs = im.stride_y; rs_uv = im.stride_uv; off = im.offset_y; off_uv = im.offset_uv;
      ok = yfi_yuv_image_ok(off, off_uv, h, w, rs, rs_uv, a.bytes);
    } else {
      const yf_image im = ((const yf_image*)a.imgs)[f];
      h = im.height; w = im.width; rs = im.row_stride; off = im.offset;
      ok = yfi_image_ok(off, h, w, rs, C, a.bytes);
    }
    if (band == 0 && tid == 0) a.status[f] = ok ? 0 : 1;
    int4* out = (int4*)((char*)a.frames + f * FRAME_BYTES) + r0 / 2 * PAIR_VECS;
    if (!ok) {                                     // never read: the frame is all -128 (fp16: all 0, pixel 0)
      fill<kThreads>(out, (r1 - r0) / 2 * PAIR_VECS, F16 ? 0 : (int)0x80808080, tid);
      continue;
    }
    const yf_fit rect = yfi_area_rect(h, w, OUT, a.fit);
    const uint64_t D = (uint64_t)h * (uint64_t)w;
    // this thread's elements of an output row: their columns' spans, their channel's place in a pixel (YUV: its two chroma factors)
    yfi_area_span sx[K];
    bool inside[K];
    int sc[K], ku[K], kv[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int item = tid + k * kThreads, ox = item / 3, c = item - ox * 3;
      inside[k] = item < ITEMS && ox >= rect.x0 && ox < rect.x0 + rect.width;
      sx[k] = yfi_area_span_of(inside[k] ? ox - rect.x0 : 0, w, rect.width);
      sc[k] = BGR ? 2 - c : c;
      ku[k] = c == 0 ? 0 : (c == 1 ? YFI_YUV_CUG : YFI_YUV_CUB);
      kv[k] = c == 0 ? YFI_YUV_CVR : (c == 1 ? YFI_YUV_CVG : 0);
    }
    const uint8_t* base = a.px + off;
    const uint8_t* base_uv = a.px + off_uv;
    for (int y = r0; y < r1; y += 2) {             // a pair of output rows: whole 16-byte vectors of every frame type
      for (int yy = y; yy < y + 2; ++yy) {
        uint64_t acc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = 0;
        const bool row_in = yy >= rect.y0 && yy < rect.y0 + rect.height;     // the same for every thread, as every bound below
        if (row_in) {
          const yfi_area_span sy = yfi_area_span_of(yy - rect.y0, h, rect.height);
          for (int c0 = 0; c0 < w; c0 += CHUNK) {
            const int c1 = c0 + CHUNK < w ? c0 + CHUNK : w, len = (c1 - c0) * C;
            const int pitch = (len + 30) & ~15;    // a phase of up to 15, the line, rounded up to whole vectors
            const int nv = pitch / 16, cap = kTileBytes / pitch, R = YUV ? cap / 2 : cap;
            // this thread's sources within the column range
            int A[K], B[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
              A[k] = sx[k].first > c0 ? sx[k].first : c0;
              B[k] = sx[k].last < c1 - 1 ? sx[k].last : c1 - 1;
              if (!inside[k]) B[k] = A[k] - 1;
            }
            for (int g = sy.first; g <= sy.last; g += R) {
              const int rows = sy.last - g + 1 < R ? sy.last - g + 1 : R;
              const int lines = YUV ? 2 * rows : rows;
              __syncthreads();                     // the readers of the tile are done
              for (int idx = tid; idx < lines * nv; idx += kThreads) {
                const int l = idx / nv, i = idx - l * nv;
                const uint8_t* src;
                if constexpr (YUV) {
                  const int r = g + (l >> 1);
                  src = (l & 1) ? base_uv + (int64_t)(r >> 1) * rs_uv + c0 : base + (int64_t)r * rs + c0;
                } else {
                  src = base + (int64_t)(g + l) * rs + (int64_t)c0 * C;
                }
                stage_vector(tile, l * pitch, src, len, i);
              }
              __syncthreads();
              for (int l = 0; l < rows; ++l) {
                const int wy = yfi_area_span_weight(sy, g + l);
                if constexpr (YUV) {
                  const uint8_t* ys = base + (int64_t)(g + l) * rs + c0;
                  const uint8_t* us = base_uv + (int64_t)((g + l) >> 1) * rs_uv + c0;
                  const uint8_t* yl = tile + 2 * l * pitch + ((uintptr_t)ys & 15);
                  const uint8_t* ul = tile + (2 * l + 1) * pitch + ((uintptr_t)us & 15);
#pragma unroll
                  for (int k = 0; k < K; ++k) {
                    // one loop and no case for the ends: every branch of a lane costs the kernel a pair of SGPRs, and it has none to spare
                    uint32_t sum = 0;
                    for (int s = A[k]; s <= B[k]; ++s) {
                      const int at = (s - c0) & ~1;                          // c0 is even: the pair of pixel s
                      const int32_t u = ul[at + (VFIRST ? 1 : 0)] - 128, v = ul[at + (VFIRST ? 0 : 1)] - 128;
                      const int32_t term = (1 << (YFI_YUV_SHIFT - 1)) + kv[k] * v + ku[k] * u;
                      sum += (uint32_t)(yfi_area_span_weight(sx[k], s) * yfi_yuv_channel(yfi_yuv_luma(yl[s - c0]), term));
                    }
                    acc[k] += (uint64_t)wy * sum;
                  }
                } else {
                  const uint8_t* src = base + (int64_t)(g + l) * rs + (int64_t)c0 * C;
                  const uint8_t* line = tile + l * pitch + ((uintptr_t)src & 15);
#pragma unroll
                  for (int k = 0; k < K; ++k) {
                    int s = A[k], e = B[k];
                    if (s > e) continue;
                    uint32_t sum = 0, inner = 0;
                    if (s == sx[k].first) { sum = (uint32_t)sx[k].w_first * line[(s - c0) * C + sc[k]]; ++s; }
                    if (e == sx[k].last && e >= s) { sum += (uint32_t)sx[k].w_last * line[(e - c0) * C + sc[k]]; --e; }
                    const uint8_t* p = line + (s - c0) * C + sc[k];
                    for (; s <= e; ++s, p += C) inner += *p;
                    sum += inner * (uint32_t)sx[k].w_mid;
                    acc[k] += (uint64_t)wy * sum;
                  }
                }
              }
            }
          }
        }
        T* stage = (T*)s_stage + (yy - y) * ITEMS;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int item = tid + k * kThreads;
          if (item >= ITEMS) continue;
          const int v = row_in && inside[k] ? yfi_area_round(acc[k], D) : a.pad;
          if constexpr (F16) stage[item] = s_half[v];
          else stage[item] = (int8_t)(v - 128);
        }
      }
      __syncthreads();
      for (int q = tid; q < PAIR_VECS; q += kThreads) out[(y - r0) / 2 * PAIR_VECS + q] = s_stage[q];
      __syncthreads();                             // the pair is out before the next one is staged
    }
  }
}

}  // namespace yfarea
#endif
