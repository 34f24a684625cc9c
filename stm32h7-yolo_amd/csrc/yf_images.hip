// libyf_images.so: decoded images of any size -> the network's int8 frames (fp16 frames for the fp16 network), resized exactly as
// cv2.resize(img, (out, out)) (INTER_LINEAR, the arithmetic of yf_images_taps.h), and on through libyf_network.so's public C-ABI to
// detection records in each image's own pixels.
// C-ABI and semantics: include/yf_images.h.
//
// Prepare kernel: one 256-thread workgroup per frame (grid-striding over the batch).  Lanes build the out_hw x-taps and y-taps in LDS, then
// each lane computes whole output pixels: four byte-wide reads per channel (two source rows, two columns), horizontal then vertical pass,
// the -128 (or, for fp16 frames, the look-up of the half of pixel / 255. in a 256-entry LDS table) and the channel order fused; lanes of a
// wave take consecutive output columns, so the reads of a sampled source row coalesce.
// The frame (or a band of 20 rows at 160x160) is staged in LDS and written with 16-byte stores.  Loads are single bytes at addresses
// inside the image's extent: no load reaches past its last pixel.
// prepare_yuv_kernel / prepare_yuv_f16_kernel: the same plan for NV12 / NV21 surfaces, each source pixel converted as cv2.cvtColor does
// before the interpolation (yf_images_yuv.h).
// The other kernels: decode_ragged_kernel (7x7 heads, each image's own scales, one wave per frame), decode_f32_kernel (the fp16 network's
// float32 logits, the arithmetic of yf_images_float.h, one wave per frame) and nms_kernel (up to 256 records, one wave per frame) below; the decode of 20x20 heads and the suppression of up to 1200 records per frame in yf_images_wide.hip.h;
// the scoring of records against ground truth (match, average precision) in yf_images_eval.hip.h; the merge of the records of an image's
// tiles (tile grid, prefix, copy) in yf_images_tiles.h and yf_images_tiles.hip.h; the face chips (every record's region of its picture,
// resized) in yf_images_crop.h and yf_images_crop.hip.h; the redaction (every record's region pixelated or filled in place) in
// yf_images_redact.h and yf_images_redact.hip.h; the blur (every record's region replaced by a grid of its means resized back) in
// yf_images_blur.h and yf_images_blur.hip.h; the drawing (every record's outline in place, in one colour or a colour per record) in
// yf_images_draw.h and yf_images_draw.hip.h; the tracker (each frame's records associated with per-stream track state) in
// yf_images_track.h, with a motion model (a constant-velocity filter per edge, held-over boxes move on) in yf_images_motion.h, and with
// the optimal assignment in the place of the greedy match in yf_images_assign.h, the three kernels one step body in
// yf_images_step.hip.h; the CLEAR-MOT score of a tracker's records against labelled identities in yf_images_score.h and
// yf_images_score.hip.h; the appearance descriptors of the records and the re-identification of lost tracks behind a tracker in
// yf_images_describe.h, yf_images_describe.hip.h, yf_images_reid.h and yf_images_reid.hip.h; the letterboxed frames and their decodes (the picture's aspect kept, the rest padded, the
// boxes mapped back) in yf_images_fit.h and yf_images_fit.hip.h; the area-averaged frames (every source pixel counted, a job per band
// of a frame) in yf_images_area.h and yf_images_area.hip.h.
// After the kernels, the host layer: the error text, the argument checks (each stated once, whichever entry points share it), the
// launches, one body behind each uniform / ragged pair of run_decode entries, and the C entry points.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdarg>
#include <mutex>
#include <stdint.h>
#include <stdio.h>
#include "../../include/yf_images.h"
#include "yf_images_taps.h"
#include "yf_images_yuv.h"
#include "yf_images_nms.h"
#include "yf_decode.hip.h"
#include "gen/yf_decode_tables_gen.h"
#include "yf_images_decode160.h"
#include "yf_images_float.h"
#include "yf_images_wide.hip.h"
#include "yf_images_eval.hip.h"
#include "yf_images_tiles.hip.h"
#include "yf_images_crop.hip.h"
#include "yf_images_redact.hip.h"
#include "yf_images_blur.hip.h"
#include "yf_images_draw.hip.h"
#include "yf_images_step.hip.h"
#include "yf_images_score.hip.h"
#include "yf_images_describe.hip.h"
#include "yf_images_reid.hip.h"
#include "yf_images_fit.hip.h"
#include "yf_images_area.hip.h"

#ifndef YF_IMAGES_BUILD_ID
#define YF_IMAGES_BUILD_ID "unknown"
#endif

namespace {

constexpr int kThreads = 256;
constexpr int kHeadBytes = 7 * 7 * 18;

struct PrepArgs {
  const uint8_t* px;
  uint64_t bytes;
  const yf_image* imgs;        // ragged
  int32_t* status;             // ragged
  int h, w;                    // uniform
  int64_t rs, fs;              // uniform
  long n;
  void* frames;                // int8, or fp16 bits (prepare_f16_kernel)
};

struct YTap { int64_t o0, o1; int32_t w0, w1; };

template <int OUT> struct Band { static constexpr int ROWS = OUT == 56 ? 56 : 20; };

// T: the frame's element, int8_t (pixel - 128) or uint16_t (the fp16 bits of pixel / 255.: yfi_f16_of_u8)
template <int OUT, int C, bool BGR, bool RAGGED, typename T>
__device__ __forceinline__ void prepare_frames(const PrepArgs& a) {
  constexpr int ROWS = Band<OUT>::ROWS;
  constexpr bool F16 = sizeof(T) == 2;
  constexpr int FRAME_BYTES = OUT * OUT * 3 * (int)sizeof(T);
  constexpr int BAND_VECS = ROWS * OUT * 3 * (int)sizeof(T) / 16;
  static_assert((ROWS * OUT * 3) % 16 == 0 && OUT % ROWS == 0, "bands of whole 16-byte vectors");
  __shared__ int4 s_xt[OUT];                       // {s0 * C, s1 * C, w0, w1}
  __shared__ YTap s_yt[OUT];
  __shared__ int4 s_stage[BAND_VECS];
  __shared__ uint16_t s_half[F16 ? 256 : 1];
  const int tid = threadIdx.x;
  if constexpr (F16) s_half[tid] = yfi_f16_of_u8(tid);       // kThreads == 256; the barrier at the head of the frame loop publishes it
  for (long f = blockIdx.x; f < a.n; f += gridDim.x) {
    uint64_t off;
    int h, w;
    int64_t rs;
    if (RAGGED) {
      const yf_image im = a.imgs[f];
      off = im.offset; h = im.height; w = im.width; rs = im.row_stride;
    } else {
      off = (uint64_t)f * (uint64_t)a.fs; h = a.h; w = a.w; rs = a.rs;
    }
    int4* out = (int4*)((char*)a.frames + f * FRAME_BYTES);
    __syncthreads();                               // the previous frame's readers of the tap tables and the stage are done
    if (RAGGED) {
      const bool ok = yfi_image_ok(off, h, w, rs, C, a.bytes);
      if (tid == 0) a.status[f] = ok ? 0 : 1;
      if (!ok) {                                   // never read: the frame is all -128 (fp16: all 0, pixel 0)
        const int v = F16 ? 0 : (int)0x80808080;
        const int4 fill = make_int4(v, v, v, v);
        for (int q = tid; q < FRAME_BYTES / 16; q += kThreads) out[q] = fill;
        continue;
      }
    }
    for (int t = tid; t < 2 * OUT; t += kThreads) {
      if (t < OUT) {
        const yfi_tap x = yfi_axis_tap(t, OUT, w);
        s_xt[t] = make_int4(x.s0 * C, x.s1 * C, x.w0, x.w1);
      } else {
        const yfi_tap y = yfi_axis_tap(t - OUT, OUT, h);
        s_yt[t - OUT] = YTap{(int64_t)y.s0 * rs, (int64_t)y.s1 * rs, y.w0, y.w1};
      }
    }
    __syncthreads();
    const uint8_t* base = a.px + off;
    T* stage = (T*)s_stage;
    for (int r0 = 0; r0 < OUT; r0 += ROWS) {
      for (int p = tid; p < ROWS * OUT; p += kThreads) {
        const int yy = p / OUT, xx = p - yy * OUT;
        const int4 tx = s_xt[xx];
        const YTap ty = s_yt[r0 + yy];
        const uint8_t* ra = base + ty.o0;
        const uint8_t* rb = base + ty.o1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int sc = BGR ? 2 - c : c;
          const int32_t h0 = yfi_hpass(ra[tx.x + sc], ra[tx.y + sc], tx.z, tx.w);
          const int32_t h1 = yfi_hpass(rb[tx.x + sc], rb[tx.y + sc], tx.z, tx.w);
          const int32_t v = yfi_vpass(h0, h1, ty.w0, ty.w1);
          if constexpr (F16) stage[p * 3 + c] = s_half[v];
          else stage[p * 3 + c] = (int8_t)(v - 128);
        }
      }
      __syncthreads();
      int4* dst = out + r0 / ROWS * BAND_VECS;
      for (int q = tid; q < BAND_VECS; q += kThreads) dst[q] = s_stage[q];
      __syncthreads();
    }
  }
}

template <int OUT, int C, bool BGR, bool RAGGED>
__global__ void __launch_bounds__(kThreads) prepare_kernel(PrepArgs a) { prepare_frames<OUT, C, BGR, RAGGED, int8_t>(a); }

// fp16 frames [n][56][56][3] for yf_network_fp16_run_device: the fp16 network has no other size
template <int C, bool BGR, bool RAGGED>
__global__ void __launch_bounds__(kThreads) prepare_f16_kernel(PrepArgs a) { prepare_frames<56, C, BGR, RAGGED, uint16_t>(a); }

// ---- NV12 / NV21 surfaces (yf_images_yuv.h): the plan of prepare_frames with another source.  The tap tables carry the chroma offsets
// beside the luma ones; an output pixel reads four luma bytes and the chroma pairs of its four samples (a pair shared by two columns or
// two rows is read and converted once), converts the four source pixels and interpolates their bytes: yfi_yuv_sample, which the host
// build calls too.  Lanes of a wave on consecutive output columns: the luma bytes and the chroma pairs of a sampled row coalesce as the
// packed formats' pixels do, at 1 and 2 bytes per source pixel instead of 3 or 4.
struct YuvArgs {
  const uint8_t* px;
  uint64_t bytes;
  const yf_image_yuv* imgs;    // ragged
  int32_t* status;             // ragged
  int h, w;                    // uniform
  int64_t sy, suv, uv_off, fs; // uniform
  long n;
  void* frames;
};

template <int OUT, bool VFIRST, bool RAGGED, typename T>
__device__ __forceinline__ void prepare_yuv_frames(const YuvArgs& a) {
  constexpr int ROWS = Band<OUT>::ROWS;
  constexpr bool F16 = sizeof(T) == 2;
  constexpr int FRAME_BYTES = OUT * OUT * 3 * (int)sizeof(T);
  constexpr int BAND_VECS = ROWS * OUT * 3 * (int)sizeof(T) / 16;
  __shared__ yfi_yuv_xtap s_xt[OUT];
  __shared__ yfi_yuv_ytap s_yt[OUT];
  __shared__ int4 s_stage[BAND_VECS];
  __shared__ uint16_t s_half[F16 ? 256 : 1];
  const int tid = threadIdx.x;
  if constexpr (F16) s_half[tid] = yfi_f16_of_u8(tid);
  for (long f = blockIdx.x; f < a.n; f += gridDim.x) {
    uint64_t off_y, off_uv;
    int h, w;
    int64_t sy, suv;
    if (RAGGED) {
      const yf_image_yuv im = a.imgs[f];
      off_y = im.offset_y; off_uv = im.offset_uv; h = im.height; w = im.width; sy = im.stride_y; suv = im.stride_uv;
    } else {
      off_y = (uint64_t)f * (uint64_t)a.fs; off_uv = off_y + (uint64_t)a.uv_off; h = a.h; w = a.w; sy = a.sy; suv = a.suv;
    }
    int4* out = (int4*)((char*)a.frames + f * FRAME_BYTES);
    __syncthreads();                               // the previous frame's readers of the tap tables and the stage are done
    if (RAGGED) {
      const bool ok = yfi_yuv_image_ok(off_y, off_uv, h, w, sy, suv, a.bytes);
      if (tid == 0) a.status[f] = ok ? 0 : 1;
      if (!ok) {                                   // never read: the frame is all -128 (fp16: all 0)
        const int v = F16 ? 0 : (int)0x80808080;
        const int4 fill = make_int4(v, v, v, v);
        for (int q = tid; q < FRAME_BYTES / 16; q += kThreads) out[q] = fill;
        continue;
      }
    }
    for (int t = tid; t < 2 * OUT; t += kThreads) {
      if (t < OUT) s_xt[t] = yfi_yuv_xtap_of(yfi_axis_tap(t, OUT, w));
      else s_yt[t - OUT] = yfi_yuv_ytap_of(yfi_axis_tap(t - OUT, OUT, h), sy, suv);
    }
    __syncthreads();
    const uint8_t* yp = a.px + off_y;
    const uint8_t* uvp = a.px + off_uv;
    T* stage = (T*)s_stage;
    for (int r0 = 0; r0 < OUT; r0 += ROWS) {
      for (int p = tid; p < ROWS * OUT; p += kThreads) {
        const int yy = p / OUT, xx = p - yy * OUT;
        int32_t rgb[3];
        yfi_yuv_sample(yp, uvp, s_xt[xx], s_yt[r0 + yy], VFIRST, rgb);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if constexpr (F16) stage[p * 3 + c] = s_half[rgb[c]];
          else stage[p * 3 + c] = (int8_t)(rgb[c] - 128);
        }
      }
      __syncthreads();
      int4* dst = out + r0 / ROWS * BAND_VECS;
      for (int q = tid; q < BAND_VECS; q += kThreads) dst[q] = s_stage[q];
      __syncthreads();
    }
  }
}

template <int OUT, bool VFIRST, bool RAGGED>
__global__ void __launch_bounds__(kThreads) prepare_yuv_kernel(YuvArgs a) { prepare_yuv_frames<OUT, VFIRST, RAGGED, int8_t>(a); }

template <bool VFIRST, bool RAGGED>
__global__ void __launch_bounds__(kThreads) prepare_yuv_f16_kernel(YuvArgs a) { prepare_yuv_frames<56, VFIRST, RAGGED, uint16_t>(a); }

// Per-image-scale decode: one wave per frame, decode_frame of csrc/yf_decode.hip.h unchanged, the scales the script's W/56. and H/56. become
// on a float32 array.  An image whose descriptor was flagged (status 1) or whose sides are out of range gets count 0.
__global__ void __launch_bounds__(kThreads) decode_ragged_kernel(const int8_t* __restrict__ heads, const yf_image* __restrict__ imgs,
                                                                 const int32_t* __restrict__ status, long n, int mode,
                                                                 yf_det* __restrict__ dets, int* __restrict__ counts, int cap) {
  const int lane = threadIdx.x & 63;
  for (long f = (long)blockIdx.x * 4 + (threadIdx.x >> 6); f < n; f += (long)gridDim.x * 4) {
    const yf_image im = imgs[f];
    const bool ok = im.height >= 1 && im.height <= YF_IMAGES_MAX_SIDE && im.width >= 1 && im.width <= YF_IMAGES_MAX_SIDE &&
                    (status == nullptr || status[f] == 0);
    if (!ok) {
      if (lane == 0) counts[f] = 0;
      continue;
    }
    const float w_scale = (float)((double)im.width / 56.0), h_scale = (float)((double)im.height / 56.0);
    yfdec::decode_frame(heads + f * kHeadBytes, f, lane, mode, w_scale, h_scale, dets, counts, cap);
  }
}

// Decode of the fp16 network's float32 logits [n][7][7][18] (h5_predition.py:51-72, the arithmetic of yf_images_float.h): four frames per
// workgroup, one wave per frame.  A frame's 882 logits go to LDS with 14 lane-consecutive loads; the 147 candidates are visited in three
// passes of 64 lanes in the order (anchor, row, col): the confidence of each, a ballot and a prefix count per pass, so a record's slot is
// the number of firing candidates before it; boxes are assembled only for the candidates that fire and fit below cap, pass by pass.  RAGGED: each
// image's own scales; status 1 or a side out of range gives count 0.  Every wave of a workgroup makes the same number of trips (the
// barriers), a wave without a frame idles through them.
template <bool RAGGED>
__global__ void __launch_bounds__(kThreads) decode_f32_kernel(const float* __restrict__ logits, const yf_image* __restrict__ imgs,
                                                              const int32_t* __restrict__ status, long n, float w_scale, float h_scale,
                                                              yf_det* __restrict__ dets, int* __restrict__ counts, int cap) {
  __shared__ float s_t[4][YFI_F32_LOGITS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t below = (1ull << lane) - 1ull;
  float* t = s_t[wave];
  for (long g = blockIdx.x; g * 4 < n; g += gridDim.x) {
    const long f = g * 4 + wave;
    bool ok = f < n;
    float ws = w_scale, hs = h_scale;
    if (RAGGED && ok) {
      const yf_image im = imgs[f];
      ok = im.height >= 1 && im.height <= YF_IMAGES_MAX_SIDE && im.width >= 1 && im.width <= YF_IMAGES_MAX_SIDE &&
           (status == nullptr || status[f] == 0);
      if (!ok && lane == 0) counts[f] = 0;
      ws = (float)((double)im.width / 56.0); hs = (float)((double)im.height / 56.0);
    }
    __syncthreads();                               // the previous frames' readers of s_t are done
    if (ok) {
      const float* src = logits + f * YFI_F32_LOGITS;
      for (int q = lane; q < YFI_F32_LOGITS; q += 64) t[q] = src[q];
    }
    __syncthreads();
    if (!ok) continue;
    yf_det* out = dets + f * cap;
    int total = 0;
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {                  // one copy of the arithmetic: a pass is complete before the next begins
      const int i = 64 * c + lane;
      const float* p = t + yfi_f32_offset(i < YFI_F32_CAND ? i : 0);
      const float conf = yfi_sigmoid_f32(p[4]);
      const bool keep = i < YFI_F32_CAND && conf > 0.7f;
      const uint64_t mask = __ballot(keep);
      const int pos = total + __popcll(mask & below);
      total += __popcll(mask);
      if (keep && pos < cap) out[pos] = yfi_f32_candidate(p, i, (int32_t)f, conf, ws, hs);
    }
    if (lane == 0) counts[f] = total;
  }
}

// Greedy IoU suppression of one frame's records per wave (yoloface_test.py:165-190; the semantics: include/yf_images.h).  The first
// m = min(max(count, 0), cap) <= 256 records are read into LDS, all of them before anything is written (d_out may equal d_dets).
//   rank:   lane L holds records L, L + 64, L + 128, L + 192; a record's rank is the number of larger keys (yfi_nms_key: conf descending,
//           later record first), counted against the keys broadcast from LDS.  Edges and the other 12 bytes go to LDS at their rank.
//   greedy: lane L takes ranks L + 64 s; the ranks still alive are four wave-uniform 64-bit masks.  For each alive rank t in ascending
//           order, every lane tests its alive ranks above t against t's edges (an LDS broadcast) with yfi_nms_survives and the masks
//           drop the suppressed ones -- the reference's loop, which removes a suppressed record before it can suppress.
//   output: the alive ranks in ascending order are the kept records; a kept record's slot is the number of alive ranks below it.
constexpr int kNmsMax = YF_IMAGES_NMS_MAX_CAP;

__device__ __forceinline__ int nms_next_alive(const uint64_t (&alive)[4], int t) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int lo = t + 1 - 64 * s;
    if (lo >= 64) continue;
    const uint64_t mask = lo > 0 ? alive[s] & (~0ull << lo) : alive[s];
    if (mask) return 64 * s + __builtin_ctzll(mask);
  }
  return kNmsMax;
}

__global__ void __launch_bounds__(64) nms_kernel(const yf_det* dets, const int* counts, long n, int cap, double thr, yf_det* out,
                                                 int* out_counts) {
  __shared__ uint64_t s_key[kNmsMax];          // by record
  __shared__ int4 s_edge[kNmsMax];             // x1, y1, x2, y2 by rank
  __shared__ int s_head[3][kNmsMax];           // frame, anchor | row | col | q_conf, conf bits, by rank
  const int lane = threadIdx.x;
  const uint64_t below = (1ull << lane) - 1ull;
  for (long f = blockIdx.x; f < n; f += gridDim.x) {
    const int c = counts[f];
    const int m = c < 0 ? 0 : (c > cap ? cap : c);
    const int* in = (const int*)(dets + f * cap);
    uint64_t key[4];
    int w[4][7];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int r = lane + 64 * s;
      key[s] = 0;
      if (r < m) {
#pragma unroll
        for (int q = 0; q < 7; ++q) w[s][q] = in[r * 7 + q];
        key[s] = yfi_nms_key((uint32_t)w[s][2], (uint32_t)r);
        s_key[r] = key[s];
      }
    }
    __syncthreads();
    int rank[4] = {0, 0, 0, 0};
    for (int j = 0; j < m; ++j) {
      const uint64_t kj = s_key[j];
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (64 * s < m) rank[s] += kj > key[s];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (lane + 64 * s < m) {
        const int p = rank[s];
        s_edge[p] = make_int4(w[s][3], w[s][4], w[s][5], w[s][6]);
        s_head[0][p] = w[s][0]; s_head[1][p] = w[s][1]; s_head[2][p] = w[s][2];
      }
    }
    __syncthreads();
    int4 e[4];
    double area[4];
    uint64_t alive[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int p = lane + 64 * s;
      e[s] = make_int4(0, 0, 0, 0);
      if (p < m) e[s] = s_edge[p];
      area[s] = yfi_nms_area(e[s].x, e[s].y, e[s].z, e[s].w);
      alive[s] = __ballot(p < m);
    }
    for (int t = m > 0 ? 0 : kNmsMax; t < m; t = nms_next_alive(alive, t)) {
      const int4 a = s_edge[t];
      const double area_a = yfi_nms_area(a.x, a.y, a.z, a.w);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int lo = t + 1 - 64 * s;                         // no alive rank above t in this slot: skip it
        if (lo >= 64 || 64 * s >= m || (lo > 0 ? alive[s] & (~0ull << lo) : alive[s]) == 0) continue;
        const int p = lane + 64 * s;
        bool sup = false;
        if (p > t && ((alive[s] >> lane) & 1ull))
          sup = !yfi_nms_survives(a.x, a.y, a.z, a.w, area_a, e[s].x, e[s].y, e[s].z, e[s].w, area[s], thr);
        alive[s] &= ~__ballot(sup);
      }
    }
    int* o = (int*)(out + f * cap);
    int kept = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int p = lane + 64 * s;
      if (p < m && ((alive[s] >> lane) & 1ull)) {
        const int slot = kept + __popcll(alive[s] & below);
        o[slot * 7 + 0] = s_head[0][p]; o[slot * 7 + 1] = s_head[1][p]; o[slot * 7 + 2] = s_head[2][p];
        o[slot * 7 + 3] = e[s].x; o[slot * 7 + 4] = e[s].y; o[slot * 7 + 5] = e[s].z; o[slot * 7 + 6] = e[s].w;
      }
      kept += __popcll(alive[s]);
    }
    if (lane == 0) out_counts[f] = kept;
    __syncthreads();                           // the LDS of this frame is read before the next frame's records land
  }
}

// ---- host ----
// Every entry point checks all of its arguments before its first launch and reports the first fault it finds (the order of the checks is
// part of the behaviour).  fail() takes printf arguments and returns 0: "no frames" in an entry point, false in a check.
thread_local char g_err[256];

long fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return 0;
}

long fail_hip(const char* what, hipError_t e) { return fail("%s: %s", what, hipGetErrorString(e)); }

long network_failed(ai_handle net, const char* what) {
  const char* t = yf_network_last_error_text(net);
  return fail("%s: %s", what, t ? t : "(no text)");
}

// after a launch of n frames: n, or 0 and "<what>: <the runtime's text>"
long launched(const char* what, long n) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(what, e);
  return n;
}

// for `groups` grid-striding workgroups of which `per_cu` fit on a CU at once: no more than fill the device (256 CUs if the query fails)
dim3 grid_for(long groups, int per_cu) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
  const long g = (long)cus * per_cu;
  return dim3((unsigned)(groups < g ? groups : g));
}

int channels_of(int format) {
  switch (format) {
    case YF_PIX_BGR8: case YF_PIX_RGB8: return 3;
    case YF_PIX_BGRA8: case YF_PIX_RGBA8: return 4;
    default: return 0;
  }
}

// ---- argument checks ----  what a uniform and a ragged batch share:
bool check_batch(int format, long n, int out_hw, const void* d_frames) {
  if (format == YF_PIX_NV12 || format == YF_PIX_NV21)
    return fail("format YF_PIX_NV12 / YF_PIX_NV21: such surfaces go through yf_images_prepare_yuv_device, yf_images_prepare_yuv_ragged_device, "
                "yf_images_prepare_yuv_f16_device or yf_images_prepare_yuv_f16_ragged_device");
  if (!channels_of(format)) return fail("format must be YF_PIX_BGR8, YF_PIX_RGB8, YF_PIX_BGRA8 or YF_PIX_RGBA8");
  if (out_hw != 56 && out_hw != 160) return fail("out_hw must be 56 or 160");
  if (n < 0) return fail("n < 0");
  if (!d_frames || ((uintptr_t)d_frames & 15) != 0) return fail("d_frames is NULL or not 16-byte aligned");
  return true;
}

// Every argument of a uniform batch.  On success fills `a` (a->imgs == nullptr says "uniform").
bool check_uniform(const void* d_pixels, size_t pixels_bytes, int format, int height, int width, long row_stride, long frame_stride,
                   long n, int out_hw, void* d_frames, PrepArgs* a) {
  if (!check_batch(format, n, out_hw, d_frames)) return false;
  const int C = channels_of(format);
  if (height < 1 || width < 1 || height > YF_IMAGES_MAX_SIDE || width > YF_IMAGES_MAX_SIDE) return fail("height and width must be in [1, 16384]");
  if (row_stride < (long)width * C) return fail("row_stride < width * bytes per pixel");
  if (frame_stride < 0) return fail("frame_stride < 0");
  if (n > 0) {
    if (!d_pixels) return fail("d_pixels is NULL");
    if (!yfi_image_ok(0, height, width, row_stride, C, pixels_bytes)) return fail("the first image reaches outside [0, pixels_bytes)");
    const uint64_t extent = (uint64_t)(height - 1) * (uint64_t)row_stride + (uint64_t)width * C;
    if (n > 1 && frame_stride > 0 && (uint64_t)(n - 1) > (pixels_bytes - extent) / (uint64_t)frame_stride)
      return fail("the last image reaches outside [0, pixels_bytes)");
  }
  *a = PrepArgs{(const uint8_t*)d_pixels, (uint64_t)pixels_bytes, nullptr, nullptr, height, width, (int64_t)row_stride, (int64_t)frame_stride,
                n, d_frames};
  return true;
}

// ... and of a ragged batch: what the host can see (the descriptors are checked on the device, image by image: d_status).  With n > 0
// a->imgs is not nullptr.
bool check_ragged(const void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images, long n, int out_hw, void* d_frames,
                  int32_t* d_status, PrepArgs* a) {
  if (!check_batch(format, n, out_hw, d_frames)) return false;
  if (n > 0 && (!d_pixels || !d_images || ((uintptr_t)d_images & 7) != 0 || !d_status || ((uintptr_t)d_status & 3) != 0))
    return fail("d_pixels, d_images (8-byte aligned) or d_status (4-byte aligned) is NULL or misaligned");
  *a = PrepArgs{(const uint8_t*)d_pixels, (uint64_t)pixels_bytes, d_images, d_status, 0, 0, 0, 0, n, d_frames};
  return true;
}

// ---- NV12 / NV21 ----  what a uniform and a ragged batch of surfaces share ...
bool check_yuv_batch(int format, long n, int out_hw, const void* d_frames) {
  if (format != YF_PIX_NV12 && format != YF_PIX_NV21) return fail("format must be YF_PIX_NV12 or YF_PIX_NV21");
  if (out_hw != 56 && out_hw != 160) return fail("out_hw must be 56 or 160");
  if (n < 0) return fail("n < 0");
  if (!d_frames || ((uintptr_t)d_frames & 15) != 0) return fail("d_frames is NULL or not 16-byte aligned");
  return true;
}

// ... every argument of a uniform one (a->imgs == nullptr says "uniform") ...
bool check_yuv_uniform(const void* d_pixels, size_t pixels_bytes, int format, int height, int width, long stride_y, long uv_offset,
                       long stride_uv, long frame_stride, long n, int out_hw, void* d_frames, YuvArgs* a) {
  if (!check_yuv_batch(format, n, out_hw, d_frames)) return false;
  if (height < 2 || width < 2 || height > YF_IMAGES_MAX_SIDE || width > YF_IMAGES_MAX_SIDE) return fail("height and width must be in [2, 16384]");
  if ((height & 1) != 0 || (width & 1) != 0) return fail("height and width must be even");
  if (stride_y < (long)width) return fail("stride_y < width");
  if (stride_uv < (long)width) return fail("stride_uv < width");
  if (uv_offset < 0) return fail("uv_offset < 0");
  if (frame_stride < 0) return fail("frame_stride < 0");
  if (n > 0) {
    if (!d_pixels) return fail("d_pixels is NULL");
    if (!yfi_yuv_image_ok(0, (uint64_t)uv_offset, height, width, stride_y, stride_uv, pixels_bytes))
      return fail("the first surface reaches outside [0, pixels_bytes)");
    const uint64_t end_y = (uint64_t)(height - 1) * (uint64_t)stride_y + (uint64_t)width;
    const uint64_t end_uv = (uint64_t)uv_offset + (uint64_t)(height / 2 - 1) * (uint64_t)stride_uv + (uint64_t)width;
    const uint64_t extent = end_y > end_uv ? end_y : end_uv;
    if (n > 1 && frame_stride > 0 && (uint64_t)(n - 1) > (pixels_bytes - extent) / (uint64_t)frame_stride)
      return fail("the last surface reaches outside [0, pixels_bytes)");
  }
  *a = YuvArgs{(const uint8_t*)d_pixels, (uint64_t)pixels_bytes, nullptr, nullptr, height, width, (int64_t)stride_y, (int64_t)stride_uv,
               (int64_t)uv_offset, (int64_t)frame_stride, n, d_frames};
  return true;
}

// ... and what the host can see of a ragged one
bool check_yuv_ragged(const void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images, long n, int out_hw, void* d_frames,
                      int32_t* d_status, YuvArgs* a) {
  if (!check_yuv_batch(format, n, out_hw, d_frames)) return false;
  if (n > 0 && (!d_pixels || !d_images || ((uintptr_t)d_images & 7) != 0 || !d_status || ((uintptr_t)d_status & 3) != 0))
    return fail("d_pixels, d_images (8-byte aligned) or d_status (4-byte aligned) is NULL or misaligned");
  *a = YuvArgs{(const uint8_t*)d_pixels, (uint64_t)pixels_bytes, d_images, d_status, 0, 0, 0, 0, 0, 0, n, d_frames};
  return true;
}

// the descriptors of a decode from heads alone
bool check_descriptors(const yf_image* d_images, long n) {
  if (n > 0 && (!d_images || ((uintptr_t)d_images & 7) != 0)) return fail("d_images is NULL or not 8-byte aligned");
  return true;
}

bool check_decode(const void* d_heads, int mode, void* d_dets, void* d_counts, int cap) {
  if (mode != YF_DECODE_PY && mode != YF_DECODE_FW && mode != YF_DECODE_FW_HOST) return fail("mode must be YF_DECODE_PY, YF_DECODE_FW or YF_DECODE_FW_HOST");
  if (!d_heads || !d_dets || !d_counts || cap <= 0) return fail("d_heads, d_dets or d_counts is NULL, or cap <= 0");
  if (((uintptr_t)d_dets & 3) != 0 || ((uintptr_t)d_counts & 3) != 0) return fail("d_dets and d_counts must be 4-byte aligned");
  return true;
}

bool check_decode160(const void* d_heads, void* d_dets, void* d_counts, int cap) {
  if (!d_heads) return fail("d_heads is NULL");
  if (((uintptr_t)d_heads & 15) != 0) return fail("d_heads is not 16-byte aligned");
  if (!d_dets) return fail("d_dets is NULL");
  if (!d_counts) return fail("d_counts is NULL");
  if (((uintptr_t)d_dets & 3) != 0) return fail("d_dets is not 4-byte aligned");
  if (((uintptr_t)d_counts & 3) != 0) return fail("d_counts is not 4-byte aligned");
  if (cap <= 0 || cap > YF_IMAGES_CAND160) return fail("cap must be in [1, 1200]");
  return true;
}

bool check_decode_f32(const void* d_logits, void* d_dets, void* d_counts, int cap) {
  if (!d_logits) return fail("d_logits is NULL");
  if (((uintptr_t)d_logits & 3) != 0) return fail("d_logits is not 4-byte aligned");
  if (!d_dets) return fail("d_dets is NULL");
  if (!d_counts) return fail("d_counts is NULL");
  if (((uintptr_t)d_dets & 3) != 0) return fail("d_dets is not 4-byte aligned");
  if (((uintptr_t)d_counts & 3) != 0) return fail("d_counts is not 4-byte aligned");
  if (cap <= 0 || cap > YFI_F32_CAND) return fail("cap must be in [1, 147]");
  return true;
}

// the arguments of either suppression; max_cap is its kernel's limit
bool check_nms(const void* d_dets, const void* d_counts, long n, int cap, int max_cap, double iou_threshold, void* d_out, void* d_out_counts) {
  if (n < 0) return fail("n < 0");
  if (cap <= 0 || cap > max_cap) return fail("cap must be in [1, %d]", max_cap);
  if (std::isnan(iou_threshold)) return fail("iou_threshold is NaN");
  if (!d_dets) return fail("d_dets is NULL");
  if (!d_counts) return fail("d_counts is NULL");
  if (!d_out) return fail("d_out is NULL");
  if (!d_out_counts) return fail("d_out_counts is NULL");
  if (((uintptr_t)d_dets & 3) != 0) return fail("d_dets is not 4-byte aligned");
  if (((uintptr_t)d_out & 3) != 0) return fail("d_out is not 4-byte aligned");
  if (((uintptr_t)d_counts & 3) != 0 || ((uintptr_t)d_out_counts & 3) != 0) return fail("d_counts or d_out_counts is not 4-byte aligned");
  return true;
}

// what the match and the average precision share: the batch, the caps and the records
bool check_eval(const void* d_dets, const void* d_counts, long n, int cap, const int32_t* d_gt_counts, int gt_cap) {
  if (n < 0) return fail("n < 0");
  if (cap <= 0 || cap > YF_IMAGES_NMS_WIDE_MAX_CAP) return fail("cap must be in [1, %d]", YF_IMAGES_NMS_WIDE_MAX_CAP);
  if (gt_cap <= 0 || gt_cap > YF_IMAGES_EVAL_MAX_GT) return fail("gt_cap must be in [1, %d]", YF_IMAGES_EVAL_MAX_GT);
  if (!d_dets) return fail("d_dets is NULL");
  if (!d_counts) return fail("d_counts is NULL");
  if (!d_gt_counts) return fail("d_gt_counts is NULL");
  if (((uintptr_t)d_dets & 3) != 0) return fail("d_dets is not 4-byte aligned");
  if (((uintptr_t)d_counts & 3) != 0 || ((uintptr_t)d_gt_counts & 3) != 0) return fail("d_counts or d_gt_counts is not 4-byte aligned");
  return true;
}

// ---- launches (of checked arguments; an empty batch launches nothing) ----
using PrepKernel = void (*)(PrepArgs);
template <int OUT, bool RAGGED>                                    // indexed by pixel format
constexpr PrepKernel kPrepare[4] = {prepare_kernel<OUT, 3, true, RAGGED>, prepare_kernel<OUT, 3, false, RAGGED>,
                                    prepare_kernel<OUT, 4, true, RAGGED>, prepare_kernel<OUT, 4, false, RAGGED>};
static_assert(YF_PIX_BGR8 == 0 && YF_PIX_RGB8 == 1 && YF_PIX_BGRA8 == 2 && YF_PIX_RGBA8 == 3, "the order of kPrepare");

long prepare(int out_hw, int format, const PrepArgs& a, hipStream_t s) {
  if (a.n == 0) return 0;
  const PrepKernel* k = out_hw == 56 ? (a.imgs ? kPrepare<56, true> : kPrepare<56, false>) : (a.imgs ? kPrepare<160, true> : kPrepare<160, false>);
  hipLaunchKernelGGL(k[format], grid_for(a.n, 8), dim3(kThreads), 0, s, a);      // LDS per workgroup: 13.6 KB at 56, 14.6 KB at 160
  return launched("prepare kernel launch", a.n);
}

template <bool RAGGED>
constexpr PrepKernel kPrepareF16[4] = {prepare_f16_kernel<3, true, RAGGED>, prepare_f16_kernel<3, false, RAGGED>,
                                       prepare_f16_kernel<4, true, RAGGED>, prepare_f16_kernel<4, false, RAGGED>};

long prepare_f16(int format, const PrepArgs& a, hipStream_t s) {
  if (a.n == 0) return 0;
  const PrepKernel* k = a.imgs ? kPrepareF16<true> : kPrepareF16<false>;
  hipLaunchKernelGGL(k[format], grid_for(a.n, 6), dim3(kThreads), 0, s, a);      // LDS per workgroup: 23.5 KB
  return launched("prepare_f16 kernel launch", a.n);
}

using YuvKernel = void (*)(YuvArgs);
template <int OUT, bool RAGGED>                                    // indexed by chroma order: NV12, NV21
constexpr YuvKernel kPrepareYuv[2] = {prepare_yuv_kernel<OUT, false, RAGGED>, prepare_yuv_kernel<OUT, true, RAGGED>};
template <bool RAGGED>
constexpr YuvKernel kPrepareYuvF16[2] = {prepare_yuv_f16_kernel<false, RAGGED>, prepare_yuv_f16_kernel<true, RAGGED>};

// out_hw: 56 or 160; f16: fp16 frames (56 only)
long prepare_yuv(int out_hw, bool f16, int format, const YuvArgs& a, hipStream_t s) {
  if (a.n == 0) return 0;
  const YuvKernel* k = f16 ? (a.imgs ? kPrepareYuvF16<true> : kPrepareYuvF16<false>)
                           : out_hw == 56 ? (a.imgs ? kPrepareYuv<56, true> : kPrepareYuv<56, false>)
                                          : (a.imgs ? kPrepareYuv<160, true> : kPrepareYuv<160, false>);
  hipLaunchKernelGGL(k[format == YF_PIX_NV21], grid_for(a.n, f16 ? 6 : 8), dim3(kThreads), 0, s, a);
  return launched("prepare_yuv kernel launch", a.n);
}

// d_images == nullptr: the scalar scales; else per-image scales (and d_status, which may be nullptr)
long decode_f32(const void* d_logits, const yf_image* d_images, const int32_t* d_status, long n, float w_scale, float h_scale, void* d_dets,
                void* d_counts, int cap, hipStream_t s) {
  if (n == 0) return 0;
  const dim3 grid = grid_for((n + 3) / 4, 8);                                     // 13.8 KB of LDS per workgroup
  if (d_images)
    hipLaunchKernelGGL(decode_f32_kernel<true>, grid, dim3(kThreads), 0, s, (const float*)d_logits, d_images, d_status, n, 0.f, 0.f,
                       (yf_det*)d_dets, (int*)d_counts, cap);
  else
    hipLaunchKernelGGL(decode_f32_kernel<false>, grid, dim3(kThreads), 0, s, (const float*)d_logits, (const yf_image*)nullptr,
                       (const int32_t*)nullptr, n, w_scale, h_scale, (yf_det*)d_dets, (int*)d_counts, cap);
  return launched("decode_f32 kernel launch", n);
}

// The decode tables: 2 KB of __constant__ in this library's code object, one copy per device.  Every int8 decode first makes sure that copy is the
// pair it has to decode with -- the network's own (yf_network_decode_tables: a model file may bring another output quantisation) when the entry
// point takes a network, else the pair last given to yf_images_set_decode_tables (at first the shipped one) -- by comparing ids, and uploads when
// they differ.  The upload is synchronous (the first one on a device as every later one, which also waits for the device: a decode in flight
// reads the old pair to its end) and is refused inside stream capture.
std::mutex g_tables_mu;
bool g_tables_on[64];
uint64_t g_tables_id[64];
int g_q_thr160[64];                              // decode160's quantised confidence threshold under the pair on the device
uint32_t g_set_sig[256], g_set_exp[256];         // yf_images_set_decode_tables
uint64_t g_set_id;
bool g_set_valid;

// FNV-1a over sigmoid then exp: the id yf_network_decode_tables gives for the same contents
uint64_t tables_id(const uint32_t* sig, const uint32_t* ex) {
  uint64_t h = 1469598103934665603ull;
  for (int i = 0; i < 2048; ++i) { h ^= reinterpret_cast<const uint8_t*>(i < 1024 ? sig : ex)[i & 1023]; h *= 1099511628211ull; }
  return h;
}

bool tables_ready(ai_handle net, hipStream_t s, int* q_thr160 = nullptr) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return fail_hip("hipGetDevice", e);
  if (dev < 0 || dev >= 64) return fail("device index out of range");
  std::lock_guard<std::mutex> lk(g_tables_mu);
  if (!g_set_valid) {                            // the shipped pair (gen/yf_decode_tables_gen.h); its id as yf_network_decode_tables computes it
    memcpy(g_set_sig, yf_sigmoid_bits, sizeof g_set_sig); memcpy(g_set_exp, yf_exp_bits, sizeof g_set_exp);
    g_set_id = tables_id(g_set_sig, g_set_exp); g_set_valid = true;
  }
  uint64_t want = g_set_id;
  if (net && yf_network_decode_tables(net, nullptr, nullptr, &want) != 0) return network_failed(net, "yf_network_decode_tables");
  if (g_tables_on[dev] && g_tables_id[dev] == want) { if (q_thr160) *q_thr160 = g_q_thr160[dev]; return true; }
  uint32_t sig[256], ex[256];
  if (net) { if (yf_network_decode_tables(net, sig, ex, &want) != 0) return network_failed(net, "yf_network_decode_tables"); }
  else { memcpy(sig, g_set_sig, sizeof sig); memcpy(ex, g_set_exp, sizeof ex); }
  if (!yfi_d160_monotonic(sig)) return fail("sigmoid table is not monotonic");     // decode160 compares quantised confidences
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
    return fail("a decode whose tables are not on the device yet uploads them: make one call outside stream capture first");
  if (g_tables_on[dev] && (e = hipDeviceSynchronize()) != hipSuccess) return fail_hip("hipDeviceSynchronize", e);
  g_tables_on[dev] = false;
  if ((e = hipMemcpyToSymbol(HIP_SYMBOL(yfdec::d_sig_bits), sig, sizeof sig)) != hipSuccess) return fail_hip("hipMemcpyToSymbol(sigmoid)", e);
  if ((e = hipMemcpyToSymbol(HIP_SYMBOL(yfdec::d_exp_bits), ex, sizeof ex)) != hipSuccess) return fail_hip("hipMemcpyToSymbol(exp)", e);
  g_tables_on[dev] = true;
  g_tables_id[dev] = want;
  g_q_thr160[dev] = yfi_d160_q_threshold(sig);
  if (q_thr160) *q_thr160 = g_q_thr160[dev];
  return true;
}

// net: the network whose tables decode (nullptr: the pair of yf_images_set_decode_tables)
long decode_ragged(ai_handle net, const void* d_heads, const yf_image* d_images, const int32_t* d_status, long n, int mode, void* d_dets, void* d_counts,
                   int cap, hipStream_t s) {
  if (n == 0) return 0;
  if (!tables_ready(net, s)) return 0;
  const long groups = (n + 3) / 4;
  hipLaunchKernelGGL(decode_ragged_kernel, dim3((unsigned)(groups < 65536 ? groups : 65536)), dim3(kThreads), 0, s,
                     (const int8_t*)d_heads, d_images, d_status, n, mode, (yf_det*)d_dets, (int*)d_counts, cap);
  return launched("decode kernel launch", n);
}

// d_images == nullptr: the scalar scales; else per-image scales (and d_status, which may be nullptr)
long decode160(ai_handle net, const void* d_heads, const yf_image* d_images, const int32_t* d_status, long n, float w_scale, float h_scale, void* d_dets,
               void* d_counts, int cap, hipStream_t s) {
  if (n == 0) return 0;
  int q_thr = 128;
  if (!tables_ready(net, s, &q_thr)) return 0;
  const dim3 grid = grid_for(n, 8), block(yfwide::kThreads);                      // 9.2 KB of LDS per workgroup
  if (d_images)
    hipLaunchKernelGGL(yfwide::decode160_kernel<true>, grid, block, 0, s, (const int8_t*)d_heads, d_images, d_status, n, 0.f, 0.f, q_thr,
                       (yf_det*)d_dets, (int*)d_counts, cap);
  else
    hipLaunchKernelGGL(yfwide::decode160_kernel<false>, grid, block, 0, s, (const int8_t*)d_heads, (const yf_image*)nullptr,
                       (const int32_t*)nullptr, n, w_scale, h_scale, q_thr, (yf_det*)d_dets, (int*)d_counts, cap);
  return launched("decode160 kernel launch", n);
}

// ---- images -> frames -> heads -> records, of a checked batch `a`, uniform or ragged; on the stream: tables, prepare, network, decode ----
// 56x56: a uniform batch has one pair of scales, which the network's own fused decode takes; a ragged one needs this library's decode
long run_decode56(ai_handle net, int format, const PrepArgs& a, void* d_heads, int mode, void* d_dets, void* d_counts, int cap, void* stream) {
  const bool ragged = a.imgs != nullptr;
  if (!check_decode(d_heads, mode, d_dets, d_counts, cap)) return 0;
  if (a.n == 0) return 0;
  if (ragged && !tables_ready(net, (hipStream_t)stream)) return 0;
  if (prepare(56, format, a, (hipStream_t)stream) != a.n) return 0;
  if (ragged) {
    if (yf_network_run_device(net, a.frames, d_heads, a.n, stream) != a.n) return network_failed(net, "yf_network_run_device");
    return decode_ragged(net, d_heads, a.imgs, a.status, a.n, mode, d_dets, d_counts, cap, (hipStream_t)stream);
  }
  const float w_scale = (float)((double)a.w / 56.0), h_scale = (float)((double)a.h / 56.0);
  if (yf_network_run_decode_device(net, a.frames, d_heads, a.n, mode, w_scale, h_scale, d_dets, d_counts, cap, stream) != a.n)
    return network_failed(net, "yf_network_run_decode_device");
  return a.n;
}

// 160x160: the scalar scales count in a uniform batch only (a ragged one has a.w = a.h = 0, and its decode reads the descriptors)
long run_decode160(ai_handle net, int format, const PrepArgs& a, void* d_heads, void* d_dets, void* d_counts, int cap, void* stream) {
  if (!check_decode160(d_heads, d_dets, d_counts, cap)) return 0;
  if (a.n == 0) return 0;
  if (!tables_ready(net, (hipStream_t)stream)) return 0;
  if (prepare(160, format, a, (hipStream_t)stream) != a.n) return 0;
  if (yf_network_run_device_hw(net, 160, 160, a.frames, d_heads, a.n, stream) != a.n) return network_failed(net, "yf_network_run_device_hw");
  const float w_scale = (float)((double)a.w / 160.0), h_scale = (float)((double)a.h / 160.0);
  return decode160(net, d_heads, a.imgs, a.status, a.n, w_scale, h_scale, d_dets, d_counts, cap, (hipStream_t)stream);
}

// fp16 network: images -> fp16 frames -> float32 logits -> records; the scalar scales count in a uniform batch only.  Nothing is launched
// on a network without yf_network_fp16_init
long run_decode_f16(ai_handle net, int format, const PrepArgs& a, void* d_logits, void* d_dets, void* d_counts, int cap, void* stream) {
  if (!check_decode_f32(d_logits, d_dets, d_counts, cap)) return 0;
  if (!yf_network_fp16_ready(net)) return network_failed(net, "yf_network_fp16_ready");
  if (a.n == 0) return 0;
  if (prepare_f16(format, a, (hipStream_t)stream) != a.n) return 0;
  if (yf_network_fp16_run_device(net, a.frames, d_logits, a.n, stream) != a.n) return network_failed(net, "yf_network_fp16_run_device");
  const float w_scale = (float)((double)a.w / 56.0), h_scale = (float)((double)a.h / 56.0);
  return decode_f32(d_logits, a.imgs, a.status, a.n, w_scale, h_scale, d_dets, d_counts, cap, (hipStream_t)stream);
}

// ---- face chips (yf_images_crop.h) ----  the chip kernels by source format (the four packed formats in the order of their codes,
// then NV12, NV21) and by the chip's byte order (RGB, BGR): a packed kernel knows only whether the two orders differ
using CropKernel = void (*)(yfcrop::Args);
constexpr CropKernel kChips[6][2] = {{yfcrop::chips_kernel<3, true>, yfcrop::chips_kernel<3, false>},       // BGR8
                                     {yfcrop::chips_kernel<3, false>, yfcrop::chips_kernel<3, true>},       // RGB8
                                     {yfcrop::chips_kernel<4, true>, yfcrop::chips_kernel<4, false>},       // BGRA8
                                     {yfcrop::chips_kernel<4, false>, yfcrop::chips_kernel<4, true>},       // RGBA8
                                     {yfcrop::chips_yuv_kernel<false, false>, yfcrop::chips_yuv_kernel<false, true>},
                                     {yfcrop::chips_yuv_kernel<true, false>, yfcrop::chips_yuv_kernel<true, true>}};
static_assert(YF_PIX_NV12 == 4 && YF_PIX_NV21 == 5, "the order of kChips");

// workgroups of chip kernel `which` that fit on a CU at once, from the runtime's occupancy query (asked once per kernel; 4 if it fails)
int chips_per_cu(int format, int bgr) {
  static std::mutex mu;
  static int cached[6][2];
  std::lock_guard<std::mutex> lk(mu);
  int& c = cached[format][bgr];
  if (c == 0) {
    int blocks = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, kChips[format][bgr], yfcrop::kThreads, 0) != hipSuccess || blocks <= 0) {
      (void)hipGetLastError();
      blocks = 4;
    }
    c = blocks > 8 ? 8 : blocks;
  }
  return c;
}

// both entries behind their format check: every other argument, then the scan and the chips
long crop_records(const void* d_pixels, size_t pixels_bytes, int format, const void* d_images, const void* d_dets, const void* d_counts, long n,
                  int cap, int out_h, int out_w, int out_format, int margin_permille, int flags, void* d_chips, long chips_cap, int32_t* d_first,
                  yf_chip* d_info, void* stream) {
  const char* err = yfi_crop_check(n, cap, out_h, out_w, out_format, margin_permille, flags, chips_cap);
  if (err) return fail("%s", err);
  if (!d_dets || !d_counts || !d_first || !d_info) return fail("d_dets, d_counts, d_first or d_info is NULL");
  if ((((uintptr_t)d_dets | (uintptr_t)d_counts | (uintptr_t)d_first | (uintptr_t)d_info) & 3) != 0)
    return fail("d_dets, d_counts, d_first and d_info must be 4-byte aligned");
  if (!d_chips || ((uintptr_t)d_chips & 15) != 0) return fail("d_chips is NULL or not 16-byte aligned");
  if (!d_pixels) return fail("d_pixels is NULL");
  if (!d_images || ((uintptr_t)d_images & 7) != 0) return fail("d_images is NULL or not 8-byte aligned");
  if (n == 0) return 0;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(yfcrop::first_kernel, dim3(1), dim3(yfcrop::kThreads), 0, s, (const int*)d_counts, n, cap, d_first);
  const long most = n * (long)cap < chips_cap ? n * (long)cap : chips_cap;            // no more chips than that can exist
  if (most > 0) {
    const yfcrop::Args a{(const uint8_t*)d_pixels, (uint64_t)pixels_bytes, d_images, (const yf_det*)d_dets, (const int*)d_counts, n, cap, out_h,
                         out_w, margin_permille, flags, (uint8_t*)d_chips, chips_cap, d_first, d_info};
    const int bgr = out_format == YF_PIX_BGR8;
    hipLaunchKernelGGL(kChips[format][bgr], grid_for(most, chips_per_cu(format, bgr)), dim3(yfcrop::kThreads), 0, s, a);
  }
  return launched("crop_records kernel launches", n);
}

// ---- redaction (yf_images_redact.h) ----  the kernels by format (the four packed formats in the order of their codes, then NV12, NV21)
// and mode (mosaic, fill)
using RedactKernel = void (*)(yfredact::Args);
constexpr RedactKernel kRedact[6][2] = {{yfredact::mosaic_kernel<3>, yfredact::fill_kernel<3>},
                                        {yfredact::mosaic_kernel<3>, yfredact::fill_kernel<3>},
                                        {yfredact::mosaic_kernel<4>, yfredact::fill_kernel<4>},
                                        {yfredact::mosaic_kernel<4>, yfredact::fill_kernel<4>},
                                        {yfredact::mosaic_yuv_kernel, yfredact::fill_yuv_kernel<false>},
                                        {yfredact::mosaic_yuv_kernel, yfredact::fill_yuv_kernel<true>}};
static_assert(YF_REDACT_MOSAIC == 0 && YF_REDACT_FILL == 1, "the order of kRedact");

// both entries behind their format check: every other argument, then the crop's scan and the records
long redact_records(void* d_pixels, size_t pixels_bytes, int format, const void* d_images, const void* d_dets, const void* d_counts, long n,
                    int cap, int mode, int block, uint32_t colour, int margin_permille, int flags, int32_t* d_first, int32_t* d_status,
                    void* stream) {
  const char* err = yfi_redact_check(n, cap, mode, block, colour, margin_permille, flags);
  if (err) return fail("%s", err);
  if (!d_dets || !d_counts || !d_first || !d_status) return fail("d_dets, d_counts, d_first or d_status is NULL");
  if ((((uintptr_t)d_dets | (uintptr_t)d_counts | (uintptr_t)d_first | (uintptr_t)d_status) & 3) != 0)
    return fail("d_dets, d_counts, d_first and d_status must be 4-byte aligned");
  if (!d_pixels) return fail("d_pixels is NULL");
  if (!d_images || ((uintptr_t)d_images & 7) != 0) return fail("d_images is NULL or not 8-byte aligned");
  if (n == 0) return 0;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(yfcrop::first_kernel, dim3(1), dim3(yfcrop::kThreads), 0, s, (const int*)d_counts, n, cap, d_first);
  yfredact::Args a{};
  a.c.bytes = (uint64_t)pixels_bytes; a.c.imgs = d_images; a.c.dets = (const yf_det*)d_dets; a.c.counts = (const int*)d_counts;
  a.c.n = n; a.c.cap = cap; a.c.margin = margin_permille; a.c.flags = flags; a.c.first = d_first;
  a.px = (uint8_t*)d_pixels; a.format = format; a.block = block; a.colour = colour; a.status = d_status;
  // no more workgroups than records can exist; 9.6 KB of LDS per mosaic workgroup, eight waves per SIMD
  hipLaunchKernelGGL(kRedact[format][mode], grid_for(n * (long)cap, 8), dim3(yfredact::kThreads), 0, s, a);
  return launched("redact_records kernel launches", n);
}

// ---- blur (yf_images_blur.h) ----  the kernels by format (the four packed formats in the order of their codes, then NV12, NV21)
using BlurKernel = void (*)(yfblur::Args);
constexpr BlurKernel kBlurMeans[6] = {yfblur::means_kernel<3>, yfblur::means_kernel<3>, yfblur::means_kernel<4>, yfblur::means_kernel<4>,
                                      yfblur::means_kernel<0>, yfblur::means_kernel<0>};
constexpr BlurKernel kBlurPaint[6] = {yfblur::paint_kernel<3>, yfblur::paint_kernel<3>, yfblur::paint_kernel<4>, yfblur::paint_kernel<4>,
                                      yfblur::paint_kernel<0>, yfblur::paint_kernel<0>};

// both entries behind their format check: every other argument, then the crop's scan, the means and the paint
long blur_records(void* d_pixels, size_t pixels_bytes, int format, const void* d_images, const void* d_dets, const void* d_counts, long n,
                  int cap, int grid, uint32_t colour, int margin_permille, int flags, void* d_work, size_t work_bytes, long records_cap,
                  int32_t* d_first, int32_t* d_status, void* stream) {
  const char* err = yfi_blur_check(n, cap, grid, colour, margin_permille, flags, d_work, work_bytes, records_cap);
  if (err) return fail("%s", err);
  if (!d_dets || !d_counts || !d_first || !d_status) return fail("d_dets, d_counts, d_first or d_status is NULL");
  if ((((uintptr_t)d_dets | (uintptr_t)d_counts | (uintptr_t)d_first | (uintptr_t)d_status) & 3) != 0)
    return fail("d_dets, d_counts, d_first and d_status must be 4-byte aligned");
  if (!d_pixels) return fail("d_pixels is NULL");
  if (!d_images || ((uintptr_t)d_images & 7) != 0) return fail("d_images is NULL or not 8-byte aligned");
  if (n == 0) return 0;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(yfcrop::first_kernel, dim3(1), dim3(yfcrop::kThreads), 0, s, (const int*)d_counts, n, cap, d_first);
  yfblur::Args a{};
  a.c.bytes = (uint64_t)pixels_bytes; a.c.imgs = d_images; a.c.dets = (const yf_det*)d_dets; a.c.counts = (const int*)d_counts;
  a.c.n = n; a.c.cap = cap; a.c.margin = margin_permille; a.c.flags = flags; a.c.first = d_first;
  a.px = (uint8_t*)d_pixels; a.format = format; a.grid = grid; a.colour = colour; a.work = (uint32_t*)d_work; a.records_cap = records_cap;
  a.status = d_status;
  // the means: no more workgroups than slots, and one at least, for d_status (6 KB of LDS each); the paint: than records (14.7 KB)
  hipLaunchKernelGGL(kBlurMeans[format], grid_for(records_cap > 0 ? records_cap : 1, 8), dim3(yfblur::kThreads), 0, s, a);
  hipLaunchKernelGGL(kBlurPaint[format], grid_for(n * (long)cap, 8), dim3(yfblur::kThreads), 0, s, a);
  return launched("blur_records kernel launches", n);
}

// ---- drawing (yf_images_draw.h) ----  the kernels by format (the four packed formats in the order of their codes, then NV12, NV21)
using DrawKernel = void (*)(yfdraw::Args);
constexpr DrawKernel kDraw[6] = {yfdraw::outline_kernel<3>, yfdraw::outline_kernel<3>, yfdraw::outline_kernel<4>, yfdraw::outline_kernel<4>,
                                 yfdraw::outline_yuv_kernel<false>, yfdraw::outline_yuv_kernel<true>};

// both entries behind their format check: every other argument, then the crop's scan and the records
long draw_records(void* d_pixels, size_t pixels_bytes, int format, const void* d_images, const void* d_dets, const void* d_counts, long n,
                  int cap, int half, uint32_t colour, const void* d_keys, int key_stride, const uint32_t* d_palette, int palette_n,
                  int32_t* d_first, int32_t* d_status, void* stream) {
  const char* err = yfi_draw_check(n, cap, half, colour, d_keys, key_stride, d_palette, palette_n);
  if (err) return fail("%s", err);
  if (!d_dets || !d_counts || !d_first || !d_status) return fail("d_dets, d_counts, d_first or d_status is NULL");
  if ((((uintptr_t)d_dets | (uintptr_t)d_counts | (uintptr_t)d_first | (uintptr_t)d_status) & 3) != 0)
    return fail("d_dets, d_counts, d_first and d_status must be 4-byte aligned");
  if (!d_pixels) return fail("d_pixels is NULL");
  if (!d_images || ((uintptr_t)d_images & 7) != 0) return fail("d_images is NULL or not 8-byte aligned");
  if (n == 0) return 0;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(yfcrop::first_kernel, dim3(1), dim3(yfcrop::kThreads), 0, s, (const int*)d_counts, n, cap, d_first);
  yfdraw::Args a{};
  a.r.c.bytes = (uint64_t)pixels_bytes; a.r.c.imgs = d_images; a.r.c.dets = (const yf_det*)d_dets; a.r.c.counts = (const int*)d_counts;
  a.r.c.n = n; a.r.c.cap = cap; a.r.c.first = d_first;
  a.r.px = (uint8_t*)d_pixels; a.r.format = format; a.r.colour = colour; a.r.status = d_status;
  a.half = half; a.keys = (const uint8_t*)d_keys; a.key_stride = key_stride; a.palette = d_palette; a.palette_n = palette_n;
  // no more workgroups than records can exist; 9.6 KB of LDS per workgroup, eight waves per SIMD
  hipLaunchKernelGGL(kDraw[format], grid_for(n * (long)cap, 8), dim3(yfdraw::kThreads), 0, s, a);
  return launched("draw_records kernel launches", n);
}

// ---- tracking (yf_images_track.h, yf_images_motion.h, yf_images_assign.h) ----  what the three entries do behind their checks: `a` comes
// with what its kernel alone takes (the gains), gets what every step kernel takes, and is launched on one-wave workgroups of which
// `per_cu` fit on a CU.  -1 and the text: here 0 is a valid number of frames
template <class A>
long track_launch(void (*kernel)(A), A a, int per_cu, const char* what, const void* d_dets, const void* d_counts, long streams, long steps,
                  int layout, int cap, const yf_track_params& p, void* d_state, void* d_out, void* d_info, void* d_out_counts, int out_cap,
                  int32_t* d_status, void* stream) {
  const long n = streams * steps;
  if (n == 0) return 0;
  a.dets = (const yf_det*)d_dets; a.counts = (const int*)d_counts; a.streams = streams; a.steps = steps; a.layout = layout; a.cap = cap;
  a.match_iou = p.match_iou; a.min_hits = p.min_hits; a.max_misses = p.max_misses;
  a.state = (uint32_t*)d_state; a.out = (yf_det*)d_out; a.info = (yf_track_info*)d_info; a.out_counts = (int*)d_out_counts;
  a.out_cap = out_cap; a.status = d_status;
  hipLaunchKernelGGL(kernel, grid_for(streams, per_cu), dim3(64), 0, (hipStream_t)stream, a);
  return launched(what, n) == n ? n : -1;
}

yfstep::MotionArgs gains_of(const yf_track_motion_params* p) {
  yfstep::MotionArgs a{};
  a.alpha = p->alpha; a.beta = p->beta; a.damp = p->damp; a.smooth = p->smooth;
  return a;
}

long track(const void* d_dets, const void* d_counts, long streams, long steps, int layout, int cap, const yf_track_params* params,
           void* d_state, void* d_out, void* d_info, void* d_out_counts, int out_cap, int32_t* d_status, void* stream) {
  const char* err = yfi_track_check(d_dets, d_counts, streams, steps, layout, cap, params, d_state, d_out, d_info, d_out_counts, out_cap, d_status);
  if (err) return fail("%s", err) - 1;
  return track_launch(yftrack::step_kernel, yfstep::Args{}, yfstep::kPerCuTrack, "track kernel launch", d_dets, d_counts, streams, steps, layout,
                      cap, *params, d_state, d_out, d_info, d_out_counts, out_cap, d_status, stream);
}

// with a motion model: the contract of `track`
long track_motion(const void* d_dets, const void* d_counts, long streams, long steps, int layout, int cap, const yf_track_motion_params* params,
                  void* d_state, void* d_out, void* d_info, void* d_out_counts, int out_cap, int32_t* d_status, void* stream) {
  const char* err = yfi_motion_check(d_dets, d_counts, streams, steps, layout, cap, params, d_state, d_out, d_info, d_out_counts, out_cap, d_status);
  if (err) return fail("%s", err) - 1;
  return track_launch(yfmotion::step_kernel, gains_of(params), yfstep::kPerCuMotion, "track_motion kernel launch", d_dets, d_counts, streams,
                      steps, layout, cap, params->base, d_state, d_out, d_info, d_out_counts, out_cap, d_status, stream);
}

// with a motion model and a choice of the match: the contract of `track`; YF_ASSIGN_GREEDY is `track_motion` and its kernel
long track_motion_assign(const void* d_dets, const void* d_counts, long streams, long steps, int layout, int cap,
                         const yf_track_motion_params* params, int assign, void* d_state, void* d_out, void* d_info, void* d_out_counts,
                         int out_cap, int32_t* d_status, void* stream) {
  const char* err = yfi_assign_check(d_dets, d_counts, streams, steps, layout, cap, params, assign, d_state, d_out, d_info, d_out_counts, out_cap, d_status);
  if (err) return fail("%s", err) - 1;
  if (assign == YF_ASSIGN_GREEDY)
    return track_motion(d_dets, d_counts, streams, steps, layout, cap, params, d_state, d_out, d_info, d_out_counts, out_cap, d_status, stream);
  return track_launch(yfassign::step_kernel, gains_of(params), yfstep::kPerCuAssign, "track_motion_assign kernel launch", d_dets, d_counts,
                      streams, steps, layout, cap, params->base, d_state, d_out, d_info, d_out_counts, out_cap, d_status, stream);
}

// ---- scoring tracks (yf_images_score.h) ----  every argument, then one launch of one-wave workgroups; -1 and the text: 0 is a valid n
long score_tracks(const void* d_out, const void* d_info, const void* d_out_counts, int out_cap, const void* d_gt, const void* d_gt_counts,
                  int gt_cap, long streams, long steps, int layout, double score_iou, void* d_state, int32_t* d_match, int32_t* d_status,
                  void* stream) {
  const char* err = yfi_score_check(d_out, d_info, d_out_counts, out_cap, d_gt, d_gt_counts, gt_cap, streams, steps, layout, score_iou, d_state,
                                    d_match, d_status);
  if (err) return fail("%s", err) - 1;
  const long n = streams * steps;
  if (n == 0) return 0;
  yfscore::Args a{};
  a.out = (const yf_det*)d_out; a.info = (const yf_track_info*)d_info; a.out_counts = (const int*)d_out_counts; a.out_cap = out_cap;
  a.gt = (const yf_gt_track*)d_gt; a.gt_counts = (const int*)d_gt_counts; a.gt_cap = gt_cap;
  a.streams = streams; a.steps = steps; a.layout = layout; a.score_iou = score_iou;
  a.state = (yf_score_state*)d_state; a.match = d_match; a.status = d_status;
  hipLaunchKernelGGL(yfscore::clip_kernel, grid_for(streams, yfscore::kPerCuScore), dim3(64), 0, (hipStream_t)stream, a);
  return launched("score_tracks kernel launch", n) == n ? n : -1;
}

// ---- appearance descriptors (yf_images_describe.h) ----  the kernels by format (the four packed formats in the order of their codes,
// then NV12, NV21, which differ in the chroma plane only: one kernel)
using DescribeKernel = void (*)(yfdescribe::Args);
constexpr DescribeKernel kDescribe[6] = {yfdescribe::records_kernel<3, true>, yfdescribe::records_kernel<3, false>,
                                         yfdescribe::records_kernel<4, true>, yfdescribe::records_kernel<4, false>,
                                         yfdescribe::records_kernel<0, false>, yfdescribe::records_kernel<0, false>};

// both entries behind their format check: every other argument, then the crop's scan and the records
long describe_records(const void* d_pixels, size_t pixels_bytes, int format, const void* d_images, const void* d_dets, const void* d_counts,
                      long n, int cap, int margin_permille, int flags, void* d_desc, int32_t* d_first, int32_t* d_status, void* stream) {
  const char* err = yfi_describe_check(d_pixels, d_images, d_dets, d_counts, n, cap, margin_permille, flags, d_desc, d_first, d_status);
  if (err) return fail("%s", err);
  if (n == 0) return 0;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(yfcrop::first_kernel, dim3(1), dim3(yfcrop::kThreads), 0, s, (const int*)d_counts, n, cap, d_first);
  yfdescribe::Args a{};
  a.c.bytes = (uint64_t)pixels_bytes; a.c.imgs = d_images; a.c.dets = (const yf_det*)d_dets; a.c.counts = (const int*)d_counts;
  a.c.n = n; a.c.cap = cap; a.c.margin = margin_permille; a.c.flags = flags; a.c.first = d_first;
  a.px = (const uint8_t*)d_pixels; a.desc = (uint32_t*)d_desc; a.status = d_status;
  // no more workgroups than records can exist, and one at least, for d_status; 0.6 KB of LDS per workgroup, eight waves per SIMD
  hipLaunchKernelGGL(kDescribe[format], grid_for(n * (long)cap, 8), dim3(yfdescribe::kThreads), 0, s, a);
  return launched("describe_records kernel launches", n);
}

// ---- re-identification (yf_images_reid.h) ----  every argument, then one launch of one-wave workgroups; -1 and the text: 0 is a valid n
long reid(const void* d_info, const void* d_out_counts, const void* d_desc, int out_cap, long streams, long steps, int layout,
          const yf_reid_params* params, void* d_state, void* d_info_out, int32_t* d_what, int32_t* d_status, void* stream) {
  const char* err = yfi_reid_check(d_info, d_out_counts, d_desc, out_cap, streams, steps, layout, params, d_state, d_info_out, d_what, d_status);
  if (err) return fail("%s", err) - 1;
  const long n = streams * steps;
  if (n == 0) return 0;
  yfreid::Args a{};
  a.info = (const yf_track_info*)d_info; a.out_counts = (const int*)d_out_counts; a.desc = (const yf_face_desc*)d_desc; a.out_cap = out_cap;
  a.streams = streams; a.steps = steps; a.layout = layout;
  a.max_distance = params->max_distance; a.max_age = params->max_age; a.blend = params->blend;
  a.state = (yf_reid_state*)d_state; a.info_out = (yf_track_info*)d_info_out; a.what = d_what; a.status = d_status;
  hipLaunchKernelGGL(yfreid::stream_kernel, grid_for(streams, yfreid::kPerCuReid), dim3(64), 0, (hipStream_t)stream, a);
  return launched("reid kernel launch", n) == n ? n : -1;
}

// ---- letterboxed frames (yf_images_fit.h) ----  the prepare kernels by format (the four packed formats in the order of their codes,
// then NV12, NV21), for a frame side and an element type
using FitKernel = void (*)(yffit::Args);
template <int OUT, typename T>
constexpr FitKernel kFit[6] = {yffit::frames_kernel<OUT, 3, true, T>, yffit::frames_kernel<OUT, 3, false, T>,
                               yffit::frames_kernel<OUT, 4, true, T>, yffit::frames_kernel<OUT, 4, false, T>,
                               yffit::frames_yuv_kernel<OUT, false, T>, yffit::frames_yuv_kernel<OUT, true, T>};

// the four prepare entries: every argument (yfi_fit_check_prepare), then the launch.  yuv: the entry's family; f16: fp16 frames
long fit_prepare(bool yuv, bool f16, const void* d_pixels, size_t pixels_bytes, int format, const void* d_images, long n, int out_hw, int pad,
                 void* d_frames, int32_t* d_status, hipStream_t s) {
  const char* err = yfi_fit_check_prepare(yuv, f16, d_pixels, format, d_images, n, out_hw, pad, d_frames, d_status);
  if (err) return fail("%s", err);
  if (n == 0) return 0;
  const FitKernel* k = f16 ? kFit<56, uint16_t> : (out_hw == 56 ? kFit<56, int8_t> : kFit<160, int8_t>);
  const yffit::Args a{(const uint8_t*)d_pixels, (uint64_t)pixels_bytes, d_images, d_status, n, d_frames, pad};
  hipLaunchKernelGGL(k[format], grid_for(n, f16 ? 6 : 8), dim3(yffit::kThreads), 0, s, a);          // the plain prepare's LDS and grids
  return launched("prepare_fit kernel launch", n);
}

// of checked arguments; net: the network whose tables decode (nullptr: the pair of yf_images_set_decode_tables)
long fit_decode(ai_handle net, const void* d_heads, const yf_image* d_images, const int32_t* d_status, long n, int out_hw, void* d_dets,
                void* d_counts, int cap, hipStream_t s) {
  if (n == 0) return 0;
  int q_thr = 128;
  if (!tables_ready(net, s, &q_thr)) return 0;
  if (out_hw == 56) {
    const long groups = (n + yffit::kWaves - 1) / yffit::kWaves;
    hipLaunchKernelGGL(yffit::decode56_kernel, dim3((unsigned)(groups < 65536 ? groups : 65536)), dim3(yffit::kThreads), 0, s,
                       (const int8_t*)d_heads, d_images, d_status, n, (yf_det*)d_dets, (int*)d_counts, cap);
  } else {
    hipLaunchKernelGGL(yffit::decode160_kernel, grid_for(n, 8), dim3(yffit::kThreads), 0, s, (const int8_t*)d_heads, d_images, d_status, n,
                       q_thr, (yf_det*)d_dets, (int*)d_counts, cap);                                // 9.2 KB of LDS per workgroup
  }
  return launched("decode_fit kernel launch", n);
}

long fit_decode_f32(const void* d_logits, const yf_image* d_images, const int32_t* d_status, long n, void* d_dets, void* d_counts, int cap,
                    hipStream_t s) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(yffit::decode_f32_kernel, grid_for((n + yffit::kWaves - 1) / yffit::kWaves, 8), dim3(yffit::kThreads), 0, s,
                     (const float*)d_logits, d_images, d_status, n, (yf_det*)d_dets, (int*)d_counts, cap);       // 13.8 KB of LDS per workgroup
  return launched("decode_f32_fit kernel launch", n);
}

// ---- area-averaged frames (yf_images_area.h) ----  the kernels by format code, for a frame side and an element type
using AreaKernel = void (*)(yfarea::Args);
template <int OUT, typename T>
constexpr AreaKernel kArea[6] = {yfarea::area_kernel<OUT, 0, T>, yfarea::area_kernel<OUT, 1, T>, yfarea::area_kernel<OUT, 2, T>,
                                 yfarea::area_kernel<OUT, 3, T>, yfarea::area_kernel<OUT, 4, T>, yfarea::area_kernel<OUT, 5, T>};

// the four entries: every argument (yfi_area_check_prepare), then one launch of n * bands jobs.  yuv: the entry's family; f16: fp16 frames
long area_prepare(bool yuv, bool f16, const void* d_pixels, size_t pixels_bytes, int format, const void* d_images, long n, int out_hw, int fit,
                  int pad, void* d_frames, int32_t* d_status, hipStream_t s) {
  const char* err = yfi_area_check_prepare(yuv, f16, d_pixels, format, d_images, n, out_hw, fit, pad, d_frames, d_status);
  if (err) return fail("%s", err);
  if (n == 0) return 0;
  const AreaKernel* k = f16 ? kArea<56, uint16_t> : (out_hw == 56 ? kArea<56, int8_t> : kArea<160, int8_t>);
  const int bands = yfi_area_bands(n, out_hw);
  const yfarea::Args a{(const uint8_t*)d_pixels, (uint64_t)pixels_bytes, d_images, d_status, n, d_frames, pad, fit, bands};
  hipLaunchKernelGGL(k[format], grid_for(n * bands, yfarea::per_cu_of(out_hw)), dim3(yfarea::threads_of(out_hw)), 0, s, a);     // 32 waves per CU
  return launched("prepare_area kernel launch", n);
}

}  // namespace

extern "C" {

YF_API const char* yf_images_last_error_text(void) { return g_err; }
YF_API const char* yf_images_build_id(void) { return YF_IMAGES_BUILD_ID; }

YF_API long yf_images_prepare_device(const void* d_pixels, size_t pixels_bytes, int format, int height, int width, long row_stride,
                                     long frame_stride, long n, int out_hw, void* d_frames, void* stream) {
  PrepArgs a;
  if (!check_uniform(d_pixels, pixels_bytes, format, height, width, row_stride, frame_stride, n, out_hw, d_frames, &a)) return 0;
  return prepare(out_hw, format, a, (hipStream_t)stream);
}

YF_API long yf_images_prepare_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images, long n,
                                            int out_hw, void* d_frames, int32_t* d_status, void* stream) {
  PrepArgs a;
  if (!check_ragged(d_pixels, pixels_bytes, format, d_images, n, out_hw, d_frames, d_status, &a)) return 0;
  return prepare(out_hw, format, a, (hipStream_t)stream);
}

YF_API long yf_images_prepare_yuv_device(const void* d_pixels, size_t pixels_bytes, int format, int height, int width, long stride_y,
                                         long uv_offset, long stride_uv, long frame_stride, long n, int out_hw, void* d_frames,
                                         void* stream) {
  YuvArgs a;
  if (!check_yuv_uniform(d_pixels, pixels_bytes, format, height, width, stride_y, uv_offset, stride_uv, frame_stride, n, out_hw, d_frames, &a))
    return 0;
  return prepare_yuv(out_hw, false, format, a, (hipStream_t)stream);
}

YF_API long yf_images_prepare_yuv_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images, long n,
                                                int out_hw, void* d_frames, int32_t* d_status, void* stream) {
  YuvArgs a;
  if (!check_yuv_ragged(d_pixels, pixels_bytes, format, d_images, n, out_hw, d_frames, d_status, &a)) return 0;
  return prepare_yuv(out_hw, false, format, a, (hipStream_t)stream);
}

YF_API long yf_images_prepare_yuv_f16_device(const void* d_pixels, size_t pixels_bytes, int format, int height, int width, long stride_y,
                                             long uv_offset, long stride_uv, long frame_stride, long n, void* d_frames_f16, void* stream) {
  YuvArgs a;
  if (!check_yuv_uniform(d_pixels, pixels_bytes, format, height, width, stride_y, uv_offset, stride_uv, frame_stride, n, 56, d_frames_f16, &a))
    return 0;
  return prepare_yuv(56, true, format, a, (hipStream_t)stream);
}

YF_API long yf_images_prepare_yuv_f16_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images,
                                                    long n, void* d_frames_f16, int32_t* d_status, void* stream) {
  YuvArgs a;
  if (!check_yuv_ragged(d_pixels, pixels_bytes, format, d_images, n, 56, d_frames_f16, d_status, &a)) return 0;
  return prepare_yuv(56, true, format, a, (hipStream_t)stream);
}

YF_API long yf_images_run_decode_device(ai_handle net, const void* d_pixels, size_t pixels_bytes, int format, int height, int width,
                                        long row_stride, long frame_stride, long n, void* d_frames, void* d_heads, int mode,
                                        void* d_dets, void* d_counts, int cap, void* stream) {
  PrepArgs a;
  if (!net) return fail("network handle is NULL");
  if (!check_uniform(d_pixels, pixels_bytes, format, height, width, row_stride, frame_stride, n, 56, d_frames, &a)) return 0;
  return run_decode56(net, format, a, d_heads, mode, d_dets, d_counts, cap, stream);
}

YF_API long yf_images_run_decode_ragged_device(ai_handle net, const void* d_pixels, size_t pixels_bytes, int format,
                                               const yf_image* d_images, long n, void* d_frames, void* d_heads, int mode,
                                               void* d_dets, void* d_counts, int cap, int32_t* d_status, void* stream) {
  PrepArgs a;
  if (!net) return fail("network handle is NULL");
  if (!check_ragged(d_pixels, pixels_bytes, format, d_images, n, 56, d_frames, d_status, &a)) return 0;
  return run_decode56(net, format, a, d_heads, mode, d_dets, d_counts, cap, stream);
}

YF_API int yf_images_set_decode_tables(const uint32_t sig_bits[256], const uint32_t exp_bits[256], uint64_t id) {
  if (!sig_bits || !exp_bits) { fail("sig_bits or exp_bits is NULL"); return -1; }
  if (!yfi_d160_monotonic(sig_bits)) { fail("sigmoid table is not monotonic"); return -1; }
  std::lock_guard<std::mutex> lk(g_tables_mu);
  memcpy(g_set_sig, sig_bits, sizeof g_set_sig); memcpy(g_set_exp, exp_bits, sizeof g_set_exp);
  g_set_id = id; g_set_valid = true;
  return 0;
}

YF_API long yf_images_decode_ragged_device(const void* d_heads, const yf_image* d_images, long n, int mode, void* d_dets, void* d_counts,
                                           int cap, void* stream) {
  if (n < 0) return fail("n < 0");
  if (!check_decode(d_heads, mode, d_dets, d_counts, cap) || !check_descriptors(d_images, n)) return 0;
  return decode_ragged(nullptr, d_heads, d_images, nullptr, n, mode, d_dets, d_counts, cap, (hipStream_t)stream);
}

YF_API long yf_images_decode160_device(const void* d_heads, long n, float w_scale, float h_scale, void* d_dets, void* d_counts, int cap,
                                       void* stream) {
  if (n < 0) return fail("n < 0");
  if (!check_decode160(d_heads, d_dets, d_counts, cap)) return 0;
  return decode160(nullptr, d_heads, nullptr, nullptr, n, w_scale, h_scale, d_dets, d_counts, cap, (hipStream_t)stream);
}

YF_API long yf_images_decode160_ragged_device(const void* d_heads, const yf_image* d_images, const int32_t* d_status, long n, void* d_dets,
                                              void* d_counts, int cap, void* stream) {
  if (n < 0) return fail("n < 0");
  if (!check_decode160(d_heads, d_dets, d_counts, cap) || !check_descriptors(d_images, n)) return 0;
  if (((uintptr_t)d_status & 3) != 0) return fail("d_status is not 4-byte aligned");
  return decode160(nullptr, d_heads, d_images, d_status, n, 0.f, 0.f, d_dets, d_counts, cap, (hipStream_t)stream);
}

YF_API long yf_images_run_decode160_device(ai_handle net, const void* d_pixels, size_t pixels_bytes, int format, int height, int width,
                                           long row_stride, long frame_stride, long n, void* d_frames, void* d_heads, void* d_dets,
                                           void* d_counts, int cap, void* stream) {
  PrepArgs a;
  if (!net) return fail("network handle is NULL");
  if (!check_uniform(d_pixels, pixels_bytes, format, height, width, row_stride, frame_stride, n, 160, d_frames, &a)) return 0;
  return run_decode160(net, format, a, d_heads, d_dets, d_counts, cap, stream);
}

YF_API long yf_images_run_decode160_ragged_device(ai_handle net, const void* d_pixels, size_t pixels_bytes, int format,
                                                  const yf_image* d_images, long n, void* d_frames, void* d_heads, void* d_dets,
                                                  void* d_counts, int cap, int32_t* d_status, void* stream) {
  PrepArgs a;
  if (!net) return fail("network handle is NULL");
  if (!check_ragged(d_pixels, pixels_bytes, format, d_images, n, 160, d_frames, d_status, &a)) return 0;
  return run_decode160(net, format, a, d_heads, d_dets, d_counts, cap, stream);
}

YF_API long yf_images_prepare_f16_device(const void* d_pixels, size_t pixels_bytes, int format, int height, int width, long row_stride,
                                         long frame_stride, long n, void* d_frames_f16, void* stream) {
  PrepArgs a;
  if (!check_uniform(d_pixels, pixels_bytes, format, height, width, row_stride, frame_stride, n, 56, d_frames_f16, &a)) return 0;
  return prepare_f16(format, a, (hipStream_t)stream);
}

YF_API long yf_images_prepare_f16_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images, long n,
                                                void* d_frames_f16, int32_t* d_status, void* stream) {
  PrepArgs a;
  if (!check_ragged(d_pixels, pixels_bytes, format, d_images, n, 56, d_frames_f16, d_status, &a)) return 0;
  return prepare_f16(format, a, (hipStream_t)stream);
}

YF_API long yf_images_decode_f32_device(const void* d_logits, long n, float w_scale, float h_scale, void* d_dets, void* d_counts, int cap,
                                        void* stream) {
  if (n < 0) return fail("n < 0");
  if (!check_decode_f32(d_logits, d_dets, d_counts, cap)) return 0;
  return decode_f32(d_logits, nullptr, nullptr, n, w_scale, h_scale, d_dets, d_counts, cap, (hipStream_t)stream);
}

YF_API long yf_images_decode_f32_ragged_device(const void* d_logits, const yf_image* d_images, const int32_t* d_status, long n, void* d_dets,
                                               void* d_counts, int cap, void* stream) {
  if (n < 0) return fail("n < 0");
  if (!check_decode_f32(d_logits, d_dets, d_counts, cap) || !check_descriptors(d_images, n)) return 0;
  if (((uintptr_t)d_status & 3) != 0) return fail("d_status is not 4-byte aligned");
  return decode_f32(d_logits, d_images, d_status, n, 0.f, 0.f, d_dets, d_counts, cap, (hipStream_t)stream);
}

YF_API long yf_images_run_decode_f16_device(ai_handle net, const void* d_pixels, size_t pixels_bytes, int format, int height, int width,
                                            long row_stride, long frame_stride, long n, void* d_frames_f16, void* d_logits, void* d_dets,
                                            void* d_counts, int cap, void* stream) {
  PrepArgs a;
  if (!net) return fail("network handle is NULL");
  if (!check_uniform(d_pixels, pixels_bytes, format, height, width, row_stride, frame_stride, n, 56, d_frames_f16, &a)) return 0;
  return run_decode_f16(net, format, a, d_logits, d_dets, d_counts, cap, stream);
}

YF_API long yf_images_run_decode_f16_ragged_device(ai_handle net, const void* d_pixels, size_t pixels_bytes, int format,
                                                   const yf_image* d_images, long n, void* d_frames_f16, void* d_logits, void* d_dets,
                                                   void* d_counts, int cap, int32_t* d_status, void* stream) {
  PrepArgs a;
  if (!net) return fail("network handle is NULL");
  if (!check_ragged(d_pixels, pixels_bytes, format, d_images, n, 56, d_frames_f16, d_status, &a)) return 0;
  return run_decode_f16(net, format, a, d_logits, d_dets, d_counts, cap, stream);
}

YF_API long yf_images_nms_device(const void* d_dets, const void* d_counts, long n, int cap, double iou_threshold, void* d_out,
                                 void* d_out_counts, void* stream) {
  if (!check_nms(d_dets, d_counts, n, cap, YF_IMAGES_NMS_MAX_CAP, iou_threshold, d_out, d_out_counts)) return 0;
  if (n == 0) return 0;
  hipLaunchKernelGGL(nms_kernel, grid_for(n, 16), dim3(64), 0, (hipStream_t)stream, (const yf_det*)d_dets, (const int*)d_counts, n, cap,
                     iou_threshold, (yf_det*)d_out, (int*)d_out_counts);                  // one-wave workgroups, 9 KB of LDS each
  return launched("nms kernel launch", n);
}

YF_API long yf_images_nms_wide_device(const void* d_dets, const void* d_counts, long n, int cap, double iou_threshold, void* d_out,
                                      void* d_out_counts, void* stream) {
  if (!check_nms(d_dets, d_counts, n, cap, YF_IMAGES_NMS_WIDE_MAX_CAP, iou_threshold, d_out, d_out_counts)) return 0;
  if (n == 0) return 0;
  const long groups = (n + yfwide::kWaves - 1) / yfwide::kWaves;                  // four frames per workgroup, 43.5 KB of LDS each
  hipLaunchKernelGGL(yfwide::nms_wide_kernel, grid_for(groups, 3), dim3(yfwide::kThreads), 0, (hipStream_t)stream, (const yf_det*)d_dets,
                     (const int*)d_counts, n, cap, iou_threshold, (yf_det*)d_out, (int*)d_out_counts);
  return launched("nms_wide kernel launch", n);
}

YF_API long yf_images_match_device(const void* d_dets, const void* d_counts, long n, int cap, const yf_gt_box* d_gt,
                                   const int32_t* d_gt_counts, int gt_cap, double iou_threshold, uint8_t* d_tp, int32_t* d_best,
                                   void* stream) {
  if (!check_eval(d_dets, d_counts, n, cap, d_gt_counts, gt_cap)) return 0;
  if (std::isnan(iou_threshold)) return fail("iou_threshold is NaN");
  if (!d_gt) return fail("d_gt is NULL");
  if (!d_tp) return fail("d_tp is NULL");
  if (((uintptr_t)d_gt & 7) != 0) return fail("d_gt is not 8-byte aligned");
  if (((uintptr_t)d_best & 3) != 0) return fail("d_best is not 4-byte aligned");
  if (n == 0) return 0;
  hipLaunchKernelGGL(yfeval::match_kernel, grid_for(n, 12), dim3(64), 0, (hipStream_t)stream, (const yf_det*)d_dets, (const int*)d_counts,
                     n, cap, d_gt, d_gt_counts, gt_cap, iou_threshold, d_tp, d_best);      // one-wave workgroups, 12.4 KB of LDS each
  return launched("match kernel launch", n);
}

YF_API int yf_images_eval_sort_tile(void) { return yfeval::kTile; }

YF_API size_t yf_images_average_precision_workspace(long n, int cap) {
  if (n < 0 || cap <= 0 || cap > YF_IMAGES_NMS_WIDE_MAX_CAP || (uint64_t)n * (uint64_t)cap >= (1ull << 31)) return 0;
  return yfeval::layout(nullptr, n, cap).bytes;
}

YF_API long yf_images_average_precision_device(const void* d_dets, const void* d_counts, const uint8_t* d_tp, long n, int cap,
                                               const int32_t* d_gt_counts, int gt_cap, void* d_work, size_t work_bytes,
                                               yf_eval_result* d_result, double* d_curve, void* stream) {
  if (!check_eval(d_dets, d_counts, n, cap, d_gt_counts, gt_cap)) return 0;
  if ((uint64_t)n * (uint64_t)cap >= (1ull << 31)) return fail("n * cap must be below 2^31");
  if (!d_tp) return fail("d_tp is NULL");
  if (!d_work || ((uintptr_t)d_work & 15) != 0) return fail("d_work is NULL or not 16-byte aligned");
  if (!d_result || ((uintptr_t)d_result & 7) != 0) return fail("d_result is NULL or not 8-byte aligned");
  if (((uintptr_t)d_curve & 7) != 0) return fail("d_curve is not 8-byte aligned");
  const yfeval::Work w = yfeval::layout(d_work, n, cap);
  if (work_bytes < w.bytes)
    return fail("work_bytes %zu is below yf_images_average_precision_workspace(n, cap) = %zu", work_bytes, w.bytes);
  if (n == 0) return 0;
  const hipStream_t s = (hipStream_t)stream;
  const long tiles = ((long)n * cap + yfeval::kTile - 1) / yfeval::kTile;           // of the capacity: the kernels stride over the true number
  const dim3 one(1), scan(yfeval::kScan), wave(64), by_tile = grid_for(tiles, 16);
  hipLaunchKernelGGL(yfeval::offsets_kernel, one, scan, 0, s, (const int*)d_counts, d_gt_counts, n, cap, gt_cap, w.offsets, w.head);
  hipLaunchKernelGGL(yfeval::gather_kernel, grid_for((n + 3) / 4, 8), dim3(256), 0, s, (const yf_det*)d_dets, (const int*)d_counts, d_tp, n, cap,
                     w.offsets, w.key[0], w.val[0]);
  for (int pass = 0; pass < 4; ++pass) {                                            // the sorted keys and flags end in key[0], val[0]
    const int a = pass & 1, b = a ^ 1;
    hipLaunchKernelGGL(yfeval::hist_kernel, by_tile, wave, 0, s, w.key[a], 8 * pass, w.head, w.hist);
    hipLaunchKernelGGL(yfeval::digit_scan_kernel, one, scan, 0, s, w.head, w.hist);
    hipLaunchKernelGGL(yfeval::scatter_kernel, by_tile, wave, 0, s, w.key[a], w.val[a], w.key[b], w.val[b], 8 * pass, w.head, w.hist);
  }
  hipLaunchKernelGGL(yfeval::tile_count_kernel, by_tile, wave, 0, s, w.val[0], w.head, w.tile_sum);
  hipLaunchKernelGGL(yfeval::tile_base_kernel, one, scan, 0, s, w.head, w.tile_sum, w.tile_base);
  hipLaunchKernelGGL(yfeval::tile_max_kernel, by_tile, wave, 0, s, w.val[0], w.head, w.tile_base, w.tile_max);
  hipLaunchKernelGGL(yfeval::tile_sufmax_kernel, one, scan, 0, s, w.head, w.tile_max, w.tile_sufmax);
  hipLaunchKernelGGL(yfeval::curve_kernel, by_tile, wave, 0, s, w.val[0], w.head, w.tile_base, w.tile_sufmax, w.terms, d_curve);
  hipLaunchKernelGGL(yfeval::sum_kernel, one, wave, 0, s, w.head, w.terms, d_result);
  return launched("average precision kernel launches", n);
}

YF_API long yf_images_plan_tiles(const yf_image* images, long n, int format, int tile_h, int tile_w, int stride_y, int stride_x, int whole,
                                 yf_tile* tiles, yf_image* tile_images, int32_t* first, long tiles_cap) {
  const char* err = "";
  const long t = yfi_plan_tiles(images, n, format, tile_h, tile_w, stride_y, stride_x, whole, tiles, tile_images, first, tiles_cap, &err);
  if (t < 0) fail("%s", err);
  return t;
}

YF_API size_t yf_images_gather_tiles_workspace(long t) {
  if (t <= 0 || t >= (1l << 31)) return 0;
  return ((size_t)t * sizeof(int32_t) + 15) & ~(size_t)15;
}

YF_API long yf_images_gather_tiles_device(const void* d_dets, const void* d_counts, long t, int cap, const yf_tile* d_tiles,
                                          const int32_t* d_first, long n, void* d_out, void* d_out_counts, int out_cap, void* d_work,
                                          size_t work_bytes, void* stream) {
  if (n < 0 || n >= (1l << 31)) return fail("n must be in [0, 2^31)");
  if (t < 0) return fail("t < 0");
  if (cap <= 0 || cap > YF_IMAGES_CAND160) return fail("cap must be in [1, %d]", YF_IMAGES_CAND160);
  if (out_cap <= 0 || out_cap > YF_IMAGES_NMS_WIDE_MAX_CAP) return fail("out_cap must be in [1, %d]", YF_IMAGES_NMS_WIDE_MAX_CAP);
  if ((uint64_t)t * (uint64_t)cap >= (1ull << 31)) return fail("t * cap must be below 2^31");
  if (!d_dets || !d_counts || !d_tiles || !d_first || !d_out || !d_out_counts)
    return fail("d_dets, d_counts, d_tiles, d_first, d_out or d_out_counts is NULL");
  if ((((uintptr_t)d_dets | (uintptr_t)d_counts | (uintptr_t)d_tiles | (uintptr_t)d_first | (uintptr_t)d_out | (uintptr_t)d_out_counts) & 3) != 0)
    return fail("d_dets, d_counts, d_tiles, d_first, d_out and d_out_counts must be 4-byte aligned");
  if (!d_work || ((uintptr_t)d_work & 15) != 0) return fail("d_work is NULL or not 16-byte aligned");
  const size_t need = yf_images_gather_tiles_workspace(t);
  if (work_bytes < need) return fail("work_bytes %zu is below yf_images_gather_tiles_workspace(t) = %zu", work_bytes, need);
  if (n == 0 || t == 0) return n;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(yftiles::prefix_kernel, grid_for(n, 8), dim3(yftiles::kThreads), 0, s, (const int*)d_counts, (int)t, cap, d_first, n,
                     (int32_t*)d_work, (int32_t*)d_out_counts);
  const long groups = (t + yftiles::kWaves - 1) / yftiles::kWaves;                  // one wave per tile, four per workgroup
  hipLaunchKernelGGL(yftiles::copy_kernel, grid_for(groups, 8), dim3(yftiles::kThreads), 0, s, (const uint32_t*)d_dets, (const int*)d_counts,
                     (int)t, cap, d_tiles, d_first, n, (const int32_t*)d_work, (uint32_t*)d_out, out_cap);
  return launched("gather_tiles kernel launches", n);
}

YF_API long yf_images_crop_records_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images, const void* d_dets,
                                          const void* d_counts, long n, int cap, int out_h, int out_w, int out_format, int margin_permille,
                                          int flags, void* d_chips, long chips_cap, int32_t* d_first, yf_chip* d_info, void* stream) {
  if (format == YF_PIX_NV12 || format == YF_PIX_NV21)
    return fail("format YF_PIX_NV12 / YF_PIX_NV21: such surfaces go through yf_images_crop_records_yuv_device");
  if (!channels_of(format)) return fail("format must be YF_PIX_BGR8, YF_PIX_RGB8, YF_PIX_BGRA8 or YF_PIX_RGBA8");
  return crop_records(d_pixels, pixels_bytes, format, d_images, d_dets, d_counts, n, cap, out_h, out_w, out_format, margin_permille, flags,
                      d_chips, chips_cap, d_first, d_info, stream);
}

YF_API long yf_images_crop_records_yuv_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images,
                                              const void* d_dets, const void* d_counts, long n, int cap, int out_h, int out_w, int out_format,
                                              int margin_permille, int flags, void* d_chips, long chips_cap, int32_t* d_first,
                                              yf_chip* d_info, void* stream) {
  if (channels_of(format)) return fail("format YF_PIX_BGR8 / RGB8 / BGRA8 / RGBA8: packed pixels go through yf_images_crop_records_device");
  if (format != YF_PIX_NV12 && format != YF_PIX_NV21) return fail("format must be YF_PIX_NV12 or YF_PIX_NV21");
  return crop_records(d_pixels, pixels_bytes, format, d_images, d_dets, d_counts, n, cap, out_h, out_w, out_format, margin_permille, flags,
                      d_chips, chips_cap, d_first, d_info, stream);
}

YF_API long yf_images_redact_records_device(void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images, const void* d_dets,
                                            const void* d_counts, long n, int cap, int mode, int block, uint32_t colour, int margin_permille,
                                            int flags, int32_t* d_first, int32_t* d_status, void* stream) {
  if (format == YF_PIX_NV12 || format == YF_PIX_NV21)
    return fail("format YF_PIX_NV12 / YF_PIX_NV21: such surfaces go through yf_images_redact_records_yuv_device");
  if (!channels_of(format)) return fail("format must be YF_PIX_BGR8, YF_PIX_RGB8, YF_PIX_BGRA8 or YF_PIX_RGBA8");
  return redact_records(d_pixels, pixels_bytes, format, d_images, d_dets, d_counts, n, cap, mode, block, colour, margin_permille, flags, d_first,
                        d_status, stream);
}

YF_API long yf_images_redact_records_yuv_device(void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images,
                                                const void* d_dets, const void* d_counts, long n, int cap, int mode, int block, uint32_t colour,
                                                int margin_permille, int flags, int32_t* d_first, int32_t* d_status, void* stream) {
  if (channels_of(format)) return fail("format YF_PIX_BGR8 / RGB8 / BGRA8 / RGBA8: packed pixels go through yf_images_redact_records_device");
  if (format != YF_PIX_NV12 && format != YF_PIX_NV21) return fail("format must be YF_PIX_NV12 or YF_PIX_NV21");
  return redact_records(d_pixels, pixels_bytes, format, d_images, d_dets, d_counts, n, cap, mode, block, colour, margin_permille, flags, d_first,
                        d_status, stream);
}

YF_API size_t yf_images_blur_workspace(long records_cap, int grid) { return yfi_blur_workspace(records_cap, grid); }

YF_API long yf_images_blur_records_device(void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images, const void* d_dets,
                                          const void* d_counts, long n, int cap, int grid, uint32_t colour, int margin_permille, int flags,
                                          void* d_work, size_t work_bytes, long records_cap, int32_t* d_first, int32_t* d_status,
                                          void* stream) {
  if (format == YF_PIX_NV12 || format == YF_PIX_NV21)
    return fail("format YF_PIX_NV12 / YF_PIX_NV21: such surfaces go through yf_images_blur_records_yuv_device");
  if (!channels_of(format)) return fail("format must be YF_PIX_BGR8, YF_PIX_RGB8, YF_PIX_BGRA8 or YF_PIX_RGBA8");
  return blur_records(d_pixels, pixels_bytes, format, d_images, d_dets, d_counts, n, cap, grid, colour, margin_permille, flags, d_work,
                      work_bytes, records_cap, d_first, d_status, stream);
}

YF_API long yf_images_blur_records_yuv_device(void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images,
                                              const void* d_dets, const void* d_counts, long n, int cap, int grid, uint32_t colour,
                                              int margin_permille, int flags, void* d_work, size_t work_bytes, long records_cap,
                                              int32_t* d_first, int32_t* d_status, void* stream) {
  if (channels_of(format)) return fail("format YF_PIX_BGR8 / RGB8 / BGRA8 / RGBA8: packed pixels go through yf_images_blur_records_device");
  if (format != YF_PIX_NV12 && format != YF_PIX_NV21) return fail("format must be YF_PIX_NV12 or YF_PIX_NV21");
  return blur_records(d_pixels, pixels_bytes, format, d_images, d_dets, d_counts, n, cap, grid, colour, margin_permille, flags, d_work,
                      work_bytes, records_cap, d_first, d_status, stream);
}

YF_API long yf_images_draw_records_device(void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images, const void* d_dets,
                                          const void* d_counts, long n, int cap, int half, uint32_t colour, const void* d_keys, int key_stride,
                                          const uint32_t* d_palette, int palette_n, int32_t* d_first, int32_t* d_status, void* stream) {
  if (format == YF_PIX_NV12 || format == YF_PIX_NV21)
    return fail("format YF_PIX_NV12 / YF_PIX_NV21: such surfaces go through yf_images_draw_records_yuv_device");
  if (!channels_of(format)) return fail("format must be YF_PIX_BGR8, YF_PIX_RGB8, YF_PIX_BGRA8 or YF_PIX_RGBA8");
  return draw_records(d_pixels, pixels_bytes, format, d_images, d_dets, d_counts, n, cap, half, colour, d_keys, key_stride, d_palette, palette_n,
                      d_first, d_status, stream);
}

YF_API long yf_images_draw_records_yuv_device(void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images,
                                              const void* d_dets, const void* d_counts, long n, int cap, int half, uint32_t colour,
                                              const void* d_keys, int key_stride, const uint32_t* d_palette, int palette_n, int32_t* d_first,
                                              int32_t* d_status, void* stream) {
  if (channels_of(format)) return fail("format YF_PIX_BGR8 / RGB8 / BGRA8 / RGBA8: packed pixels go through yf_images_draw_records_device");
  if (format != YF_PIX_NV12 && format != YF_PIX_NV21) return fail("format must be YF_PIX_NV12 or YF_PIX_NV21");
  return draw_records(d_pixels, pixels_bytes, format, d_images, d_dets, d_counts, n, cap, half, colour, d_keys, key_stride, d_palette, palette_n,
                      d_first, d_status, stream);
}

YF_API size_t yf_images_track_motion_state_bytes(long streams) { return streams > 0 ? (size_t)streams * sizeof(yf_track_motion_state) : 0; }

YF_API long yf_images_track_motion_device(const void* d_dets, const void* d_counts, long streams, long steps, int layout, int cap,
                                          const yf_track_motion_params* params, void* d_state, void* d_out, void* d_info,
                                          void* d_out_counts, int out_cap, int32_t* d_status, void* stream) {
  return track_motion(d_dets, d_counts, streams, steps, layout, cap, params, d_state, d_out, d_info, d_out_counts, out_cap, d_status, stream);
}

YF_API long yf_images_track_motion_assign_device(const void* d_dets, const void* d_counts, long streams, long steps, int layout, int cap,
                                                 const yf_track_motion_params* params, int assign, void* d_state, void* d_out, void* d_info,
                                                 void* d_out_counts, int out_cap, int32_t* d_status, void* stream) {
  return track_motion_assign(d_dets, d_counts, streams, steps, layout, cap, params, assign, d_state, d_out, d_info, d_out_counts, out_cap, d_status,
                             stream);
}

YF_API size_t yf_images_score_state_bytes(long streams) { return streams > 0 ? (size_t)streams * sizeof(yf_score_state) : 0; }

YF_API long yf_images_score_tracks_device(const void* d_out, const void* d_info, const void* d_out_counts, int out_cap, const void* d_gt,
                                          const void* d_gt_counts, int gt_cap, long streams, long steps, int layout, double score_iou,
                                          void* d_state, int32_t* d_match, int32_t* d_status, void* stream) {
  return score_tracks(d_out, d_info, d_out_counts, out_cap, d_gt, d_gt_counts, gt_cap, streams, steps, layout, score_iou, d_state, d_match,
                      d_status, stream);
}

YF_API int yf_images_score_summary(const void* host_states, long streams, yf_score_summary* out) {
  if (yfi_score_summary(host_states, streams, out) != 0) { fail("out is NULL, streams < 0, or host_states is NULL with streams > 0"); return -1; }
  return 0;
}

YF_API long yf_images_describe_records_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images,
                                              const void* d_dets, const void* d_counts, long n, int cap, int margin_permille, int flags,
                                              void* d_desc, int32_t* d_first, int32_t* d_status, void* stream) {
  if (format == YF_PIX_NV12 || format == YF_PIX_NV21)
    return fail("format YF_PIX_NV12 / YF_PIX_NV21: such surfaces go through yf_images_describe_records_yuv_device");
  if (!channels_of(format)) return fail("format must be YF_PIX_BGR8, YF_PIX_RGB8, YF_PIX_BGRA8 or YF_PIX_RGBA8");
  return describe_records(d_pixels, pixels_bytes, format, d_images, d_dets, d_counts, n, cap, margin_permille, flags, d_desc, d_first, d_status,
                          stream);
}

YF_API long yf_images_describe_records_yuv_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images,
                                                  const void* d_dets, const void* d_counts, long n, int cap, int margin_permille, int flags,
                                                  void* d_desc, int32_t* d_first, int32_t* d_status, void* stream) {
  if (channels_of(format)) return fail("format YF_PIX_BGR8 / RGB8 / BGRA8 / RGBA8: packed pixels go through yf_images_describe_records_device");
  if (format != YF_PIX_NV12 && format != YF_PIX_NV21) return fail("format must be YF_PIX_NV12 or YF_PIX_NV21");
  return describe_records(d_pixels, pixels_bytes, format, d_images, d_dets, d_counts, n, cap, margin_permille, flags, d_desc, d_first, d_status,
                          stream);
}

YF_API size_t yf_images_reid_state_bytes(long streams) { return streams > 0 ? (size_t)streams * sizeof(yf_reid_state) : 0; }

YF_API long yf_images_reid_device(const void* d_info, const void* d_out_counts, const void* d_desc, int out_cap, long streams, long steps,
                                  int layout, const yf_reid_params* params, void* d_state, void* d_info_out, int32_t* d_what,
                                  int32_t* d_status, void* stream) {
  return reid(d_info, d_out_counts, d_desc, out_cap, streams, steps, layout, params, d_state, d_info_out, d_what, d_status, stream);
}

YF_API size_t yf_images_track_state_bytes(long streams) { return streams > 0 ? (size_t)streams * sizeof(yf_track_state) : 0; }

YF_API long yf_images_track_device(const void* d_dets, const void* d_counts, long streams, long steps, int layout, int cap,
                                   const yf_track_params* params, void* d_state, void* d_out, void* d_info, void* d_out_counts, int out_cap,
                                   int32_t* d_status, void* stream) {
  return track(d_dets, d_counts, streams, steps, layout, cap, params, d_state, d_out, d_info, d_out_counts, out_cap, d_status, stream);
}

YF_API int yf_images_fit(int height, int width, int out_hw, yf_fit* fit) {
  if (!fit) { fail("fit is NULL"); return -1; }
  if (out_hw != 56 && out_hw != 160) { fail("out_hw must be 56 or 160"); return -1; }
  if (!yfi_fit_sides_ok(height, width)) { fail("height and width must be in [1, 16384]"); return -1; }
  *fit = yfi_fit_of(height, width, out_hw);
  return 0;
}

YF_API long yf_images_prepare_fit_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images, long n,
                                                int out_hw, int pad, void* d_frames, int32_t* d_status, void* stream) {
  return fit_prepare(false, false, d_pixels, pixels_bytes, format, d_images, n, out_hw, pad, d_frames, d_status, (hipStream_t)stream);
}

YF_API long yf_images_prepare_fit_yuv_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images,
                                                    long n, int out_hw, int pad, void* d_frames, int32_t* d_status, void* stream) {
  return fit_prepare(true, false, d_pixels, pixels_bytes, format, d_images, n, out_hw, pad, d_frames, d_status, (hipStream_t)stream);
}

YF_API long yf_images_prepare_fit_f16_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images, long n,
                                                    int pad, void* d_frames_f16, int32_t* d_status, void* stream) {
  return fit_prepare(false, true, d_pixels, pixels_bytes, format, d_images, n, 56, pad, d_frames_f16, d_status, (hipStream_t)stream);
}

YF_API long yf_images_prepare_fit_yuv_f16_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images,
                                                        long n, int pad, void* d_frames_f16, int32_t* d_status, void* stream) {
  return fit_prepare(true, true, d_pixels, pixels_bytes, format, d_images, n, 56, pad, d_frames_f16, d_status, (hipStream_t)stream);
}

YF_API long yf_images_decode_fit_ragged_device(const void* d_heads, const yf_image* d_images, const int32_t* d_status, long n, int out_hw,
                                               void* d_dets, void* d_counts, int cap, void* stream) {
  const char* err = yfi_fit_check_decode(0, d_heads, d_images, d_status, n, out_hw, d_dets, d_counts, cap);
  if (err) return fail("%s", err);
  return fit_decode(nullptr, d_heads, d_images, d_status, n, out_hw, d_dets, d_counts, cap, (hipStream_t)stream);
}

YF_API long yf_images_decode_f32_fit_ragged_device(const void* d_logits, const yf_image* d_images, const int32_t* d_status, long n,
                                                   void* d_dets, void* d_counts, int cap, void* stream) {
  const char* err = yfi_fit_check_decode(1, d_logits, d_images, d_status, n, 56, d_dets, d_counts, cap);
  if (err) return fail("%s", err);
  return fit_decode_f32(d_logits, d_images, d_status, n, d_dets, d_counts, cap, (hipStream_t)stream);
}

// images -> letterboxed frames -> heads -> records on the stream: every argument first, then tables, prepare, network, decode
YF_API long yf_images_run_decode_fit_ragged_device(ai_handle net, const void* d_pixels, size_t pixels_bytes, int format,
                                                   const yf_image* d_images, long n, int out_hw, int pad, void* d_frames, void* d_heads,
                                                   void* d_dets, void* d_counts, int cap, int32_t* d_status, void* stream) {
  if (!net) return fail("network handle is NULL");
  const char* err = yfi_fit_check_prepare(0, 0, d_pixels, format, d_images, n, out_hw, pad, d_frames, d_status);
  if (!err) err = yfi_fit_check_decode(0, d_heads, d_images, d_status, n, out_hw, d_dets, d_counts, cap);
  if (err) return fail("%s", err);
  if (n == 0) return 0;
  const hipStream_t s = (hipStream_t)stream;
  if (!tables_ready(net, s)) return 0;
  if (fit_prepare(false, false, d_pixels, pixels_bytes, format, d_images, n, out_hw, pad, d_frames, d_status, s) != n) return 0;
  if (out_hw == 56) {
    if (yf_network_run_device(net, d_frames, d_heads, n, stream) != n) return network_failed(net, "yf_network_run_device");
  } else if (yf_network_run_device_hw(net, 160, 160, d_frames, d_heads, n, stream) != n) {
    return network_failed(net, "yf_network_run_device_hw");
  }
  return fit_decode(net, d_heads, d_images, d_status, n, out_hw, d_dets, d_counts, cap, s);
}

// ... on the fp16 network; nothing is launched on a network without yf_network_fp16_init
YF_API long yf_images_run_decode_fit_f16_ragged_device(ai_handle net, const void* d_pixels, size_t pixels_bytes, int format,
                                                       const yf_image* d_images, long n, int pad, void* d_frames_f16, void* d_logits,
                                                       void* d_dets, void* d_counts, int cap, int32_t* d_status, void* stream) {
  if (!net) return fail("network handle is NULL");
  const char* err = yfi_fit_check_prepare(0, 1, d_pixels, format, d_images, n, 56, pad, d_frames_f16, d_status);
  if (!err) err = yfi_fit_check_decode(1, d_logits, d_images, d_status, n, 56, d_dets, d_counts, cap);
  if (err) return fail("%s", err);
  if (!yf_network_fp16_ready(net)) return network_failed(net, "yf_network_fp16_ready");
  if (n == 0) return 0;
  const hipStream_t s = (hipStream_t)stream;
  if (fit_prepare(false, true, d_pixels, pixels_bytes, format, d_images, n, 56, pad, d_frames_f16, d_status, s) != n) return 0;
  if (yf_network_fp16_run_device(net, d_frames_f16, d_logits, n, stream) != n) return network_failed(net, "yf_network_fp16_run_device");
  return fit_decode_f32(d_logits, d_images, d_status, n, d_dets, d_counts, cap, s);
}

// ---- area-averaged frames ----
YF_API int yf_images_area_bands(long n, int out_hw) {
  if (n < 0 || (out_hw != 56 && out_hw != 160)) return 0;
  return yfi_area_bands(n, out_hw);
}

YF_API long yf_images_prepare_area_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images, long n,
                                                 int out_hw, int fit, int pad, void* d_frames, int32_t* d_status, void* stream) {
  return area_prepare(false, false, d_pixels, pixels_bytes, format, d_images, n, out_hw, fit, pad, d_frames, d_status, (hipStream_t)stream);
}

YF_API long yf_images_prepare_area_yuv_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images,
                                                     long n, int out_hw, int fit, int pad, void* d_frames, int32_t* d_status, void* stream) {
  return area_prepare(true, false, d_pixels, pixels_bytes, format, d_images, n, out_hw, fit, pad, d_frames, d_status, (hipStream_t)stream);
}

YF_API long yf_images_prepare_area_f16_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images, long n,
                                                     int fit, int pad, void* d_frames_f16, int32_t* d_status, void* stream) {
  return area_prepare(false, true, d_pixels, pixels_bytes, format, d_images, n, 56, fit, pad, d_frames_f16, d_status, (hipStream_t)stream);
}

YF_API long yf_images_prepare_area_yuv_f16_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images,
                                                         long n, int fit, int pad, void* d_frames_f16, int32_t* d_status, void* stream) {
  return area_prepare(true, true, d_pixels, pixels_bytes, format, d_images, n, 56, fit, pad, d_frames_f16, d_status, (hipStream_t)stream);
}

}  // extern "C"
