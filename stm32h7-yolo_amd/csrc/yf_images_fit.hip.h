// The kernels of libyf_images.so behind letterboxed frames (csrc/yf_images_fit.h: the fit, the frame, the boxes).  Included once by
// yf_images.hip; C-ABI and semantics: include/yf_images.h.
//
// Prepare: the plan of prepare_frames / prepare_yuv_frames of yf_images.hip -- one 256-thread workgroup per frame, grid-striding; tap
// tables in LDS, a band of the frame staged in LDS, 16-byte stores -- with the tables built per frame from the picture's fit: the tap of a
// padded column or row says "outside" (yfi_fit_tap), a pixel with such a tap stores the pad and loads nothing, and a band that lies wholly
// in the top or bottom padding is written as a fill straight to memory, without loads, LDS or barriers.  A pixel inside the rectangle does
// what the plain prepare does for it, after one test of its two taps.  Ragged only.
// Decode: decode56_kernel (7x7 int8 heads, one wave per frame, the tables read where decode_ragged_kernel reads them),
// decode160_kernel (20x20 int8 heads, the plan of yfwide::decode160_kernel) and decode_f32_kernel (the fp16 network's logits, the plan of
// decode_f32_kernel of yf_images.hip), each with the fit recomputed per frame from the descriptor's sides and yfi_fit_candidate's tail.
#ifndef YF_IMAGES_FIT_HIP_H
#define YF_IMAGES_FIT_HIP_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/yf_images.h"
#include "yf_images_fit.h"
#include "yf_images_yuv.h"
#include "yf_decode.hip.h"

namespace yffit {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

struct Args {
  const uint8_t* px;
  uint64_t bytes;
  const void* imgs;            // yf_image[n], or yf_image_yuv[n] for the surfaces' kernels
  int32_t* status;
  long n;
  void* frames;                // int8, or fp16 bits
  int pad;                     // 0..255
};

struct YTap { int64_t o0, o1; int32_t w0, w1; };

template <int OUT> struct Band { static constexpr int ROWS = OUT == 56 ? 56 : 20; };

// four bytes of a run of padded elements: the int8 (pad - 128) four times, or the half of pad / 255. twice
template <typename T>
__device__ __forceinline__ int pad_word(int pad) {
  const int v = sizeof(T) == 2 ? (int)yfi_f16_of_u8(pad) * 0x10001 : ((pad - 128) & 255) * 0x01010101;
  return v;
}

// `vecs` 16-byte vectors of one word, 16 bytes per lane and trip: a refused picture's frame, a band of padding.  Not inlined on purpose: the
// two rare paths then cost the frame loop of every prepare kernel one call each instead of their address arithmetic held in registers
// across the pixel loop (3 to 10 VGPRs per kernel as compiled).
__device__ __noinline__ void fill(int4* out, int vecs, int v, int tid) {
  for (int q = tid; q < vecs; q += kThreads) out[q] = make_int4(v, v, v, v);
}

// T: the frame's element, int8_t (pixel - 128) or uint16_t (the fp16 bits of pixel / 255.)
template <int OUT, int C, bool BGR, typename T>
__global__ void __launch_bounds__(kThreads) frames_kernel(Args a) {
  constexpr int ROWS = Band<OUT>::ROWS;
  constexpr bool F16 = sizeof(T) == 2;
  constexpr int FRAME_BYTES = OUT * OUT * 3 * (int)sizeof(T);
  constexpr int BAND_VECS = ROWS * OUT * 3 * (int)sizeof(T) / 16;
  static_assert((ROWS * OUT * 3) % 16 == 0 && OUT % ROWS == 0, "bands of whole 16-byte vectors");
  __shared__ int4 s_xt[OUT];                       // {s0 * C, s1 * C, w0, w1}; w0 < 0: a padded column
  __shared__ YTap s_yt[OUT];                       // w0 < 0: a padded row
  __shared__ int4 s_stage[BAND_VECS];
  __shared__ uint16_t s_half[F16 ? 256 : 1];
  const int tid = threadIdx.x;
  const yf_image* imgs = (const yf_image*)a.imgs;
  if constexpr (F16) s_half[tid] = yfi_f16_of_u8(tid);       // kThreads == 256; the barrier at the head of the frame loop publishes it
  const int padw = pad_word<T>(a.pad);
  const T pad1 = F16 ? (T)yfi_f16_of_u8(a.pad) : (T)(a.pad - 128);
  for (long f = blockIdx.x; f < a.n; f += gridDim.x) {
    const yf_image im = imgs[f];
    const uint64_t off = im.offset;
    const int h = im.height, w = im.width;
    const int64_t rs = im.row_stride;
    int4* out = (int4*)((char*)a.frames + f * FRAME_BYTES);
    __syncthreads();                               // the previous frame's readers of the tap tables and the stage are done
    const bool ok = yfi_image_ok(off, h, w, rs, C, a.bytes);
    if (tid == 0) a.status[f] = ok ? 0 : 1;
    if (!ok) {                                     // never read: the frame is all -128 (fp16: all 0, pixel 0)
      const int v = F16 ? 0 : (int)0x80808080;
      fill(out, FRAME_BYTES / 16, v, tid);
      continue;
    }
    const yf_fit fit = yfi_fit_of(h, w, OUT);
    for (int t = tid; t < OUT; t += kThreads) {    // one axis after the other: each has a division of its own in front of its loop
      const yfi_tap x = yfi_fit_tap(t, fit.x0, fit.width, w);
      s_xt[t] = make_int4(x.s0 * C, x.s1 * C, x.w0, x.w1);
    }
    for (int t = tid; t < OUT; t += kThreads) {
      const yfi_tap y = yfi_fit_tap(t, fit.y0, fit.height, h);
      s_yt[t] = YTap{(int64_t)y.s0 * rs, (int64_t)y.s1 * rs, y.w0, y.w1};
    }
    __syncthreads();
    const uint8_t* base = a.px + off;
    T* stage = (T*)s_stage;
    for (int r0 = 0; r0 < OUT; r0 += ROWS) {
      int4* dst = out + r0 / ROWS * BAND_VECS;
      if (r0 + ROWS <= fit.y0 || r0 >= fit.y0 + fit.height) {      // the same for every thread: a band of padding
        fill(dst, BAND_VECS, padw, tid);
        continue;
      }
      for (int p = tid; p < ROWS * OUT; p += kThreads) {
        const int yy = p / OUT, xx = p - yy * OUT;
        if ((s_xt[xx].z | s_yt[r0 + yy].w0) < 0) {                  // the two weights alone decide; the rest of the taps after the test
          stage[p * 3] = pad1; stage[p * 3 + 1] = pad1; stage[p * 3 + 2] = pad1;
          continue;
        }
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
      for (int q = tid; q < BAND_VECS; q += kThreads) dst[q] = s_stage[q];
      __syncthreads();
    }
  }
}

// NV12 / NV21 surfaces: the same with the taps and the sample of yf_images_yuv.h
template <int OUT, bool VFIRST, typename T>
__global__ void __launch_bounds__(kThreads) frames_yuv_kernel(Args a) {
  constexpr int ROWS = Band<OUT>::ROWS;
  constexpr bool F16 = sizeof(T) == 2;
  constexpr int FRAME_BYTES = OUT * OUT * 3 * (int)sizeof(T);
  constexpr int BAND_VECS = ROWS * OUT * 3 * (int)sizeof(T) / 16;
  __shared__ yfi_yuv_xtap s_xt[OUT];
  __shared__ yfi_yuv_ytap s_yt[OUT];
  __shared__ int4 s_stage[BAND_VECS];
  __shared__ uint16_t s_half[F16 ? 256 : 1];
  const int tid = threadIdx.x;
  const yf_image_yuv* imgs = (const yf_image_yuv*)a.imgs;
  if constexpr (F16) s_half[tid] = yfi_f16_of_u8(tid);
  const int padw = pad_word<T>(a.pad);
  for (long f = blockIdx.x; f < a.n; f += gridDim.x) {
    const yf_image_yuv im = imgs[f];
    const int h = im.height, w = im.width;
    int4* out = (int4*)((char*)a.frames + f * FRAME_BYTES);
    __syncthreads();                               // the previous frame's readers of the tap tables and the stage are done
    const bool ok = yfi_yuv_image_ok(im.offset_y, im.offset_uv, h, w, im.stride_y, im.stride_uv, a.bytes);
    if (tid == 0) a.status[f] = ok ? 0 : 1;
    if (!ok) {                                     // never read: the frame is all -128 (fp16: all 0)
      const int v = F16 ? 0 : (int)0x80808080;
      fill(out, FRAME_BYTES / 16, v, tid);
      continue;
    }
    const yf_fit fit = yfi_fit_of(h, w, OUT);
    for (int t = tid; t < OUT; t += kThreads) s_xt[t] = yfi_yuv_xtap_of(yfi_fit_tap(t, fit.x0, fit.width, w));
    for (int t = tid; t < OUT; t += kThreads) s_yt[t] = yfi_yuv_ytap_of(yfi_fit_tap(t, fit.y0, fit.height, h), im.stride_y, im.stride_uv);
    __syncthreads();
    const uint8_t* yp = a.px + im.offset_y;
    const uint8_t* uvp = a.px + im.offset_uv;
    T* stage = (T*)s_stage;
    for (int r0 = 0; r0 < OUT; r0 += ROWS) {
      int4* dst = out + r0 / ROWS * BAND_VECS;
      if (r0 + ROWS <= fit.y0 || r0 >= fit.y0 + fit.height) {      // the same for every thread: a band of padding
        fill(dst, BAND_VECS, padw, tid);
        continue;
      }
      for (int p = tid; p < ROWS * OUT; p += kThreads) {
        const int yy = p / OUT, xx = p - yy * OUT;
        const yfi_yuv_xtap tx = s_xt[xx];
        const yfi_yuv_ytap ty = s_yt[r0 + yy];
        int32_t rgb[3] = {a.pad, a.pad, a.pad};                      // a padded pixel keeps these: no sample, no load
        if ((tx.w0 | ty.w0) >= 0) yfi_yuv_sample(yp, uvp, tx, ty, VFIRST, rgb);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if constexpr (F16) stage[p * 3 + c] = s_half[rgb[c]];
          else stage[p * 3 + c] = (int8_t)(rgb[c] - 128);
        }
      }
      __syncthreads();
      for (int q = tid; q < BAND_VECS; q += kThreads) dst[q] = s_stage[q];
      __syncthreads();
    }
  }
}

// ---- decodes ----  a frame's descriptor is one for the whole wave (workgroup, at 160): its sides and its status are read through lane
// 0, so the branches on them are uniform by construction.  status 1 or a side outside [1, 16384]: count 0, no record.
__device__ __forceinline__ bool frame_ok(const yf_image* imgs, const int32_t* status, long f, int* h, int* w) {
  *h = __builtin_amdgcn_readfirstlane(imgs[f].height);
  *w = __builtin_amdgcn_readfirstlane(imgs[f].width);
  const int st = status == nullptr ? 0 : __builtin_amdgcn_readfirstlane(status[f]);
  return yfi_fit_sides_ok(*h, *w) && st == 0;
}

// 7x7 int8 heads: four frames per workgroup, one wave per frame; the 147 candidates in three passes of 64 lanes in the order (anchor,
// row, col): the confidence from the sigmoid table, conf > 0.7f, a ballot per pass, so a record's slot is the number of firing candidates
// before it; boxes only for the candidates that fire and fit below cap.
__global__ void __launch_bounds__(kThreads) decode56_kernel(const int8_t* __restrict__ heads, const yf_image* __restrict__ imgs,
                                                            const int32_t* __restrict__ status, long n, yf_det* __restrict__ dets,
                                                            int* __restrict__ counts, int cap) {
  const int lane = threadIdx.x & 63;
  const uint64_t below = (1ull << lane) - 1ull;
  for (long f = (long)blockIdx.x * kWaves + (threadIdx.x >> 6); f < n; f += (long)gridDim.x * kWaves) {
    int h, w;
    if (!frame_ok(imgs, status, f, &h, &w)) {
      if (lane == 0) counts[f] = 0;
      continue;
    }
    const yfi_fit_map m = yfi_fit_map_of(h, w, 56);
    const int8_t* head = heads + f * (7 * 7 * 18);
    yf_det* out = dets + f * cap;
    int total = 0;
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
      const int i = 64 * c + lane;
      const int8_t* p = head + yfi_fit_offset(i < 147 ? i : 0, 7);
      const bool keep = i < 147 && yfi_d160_bits(yfdec::d_sig_bits[p[4] + 128]) > 0.7f;
      const uint64_t mask = __ballot(keep);
      const int pos = total + __popcll(mask & below);
      total += __popcll(mask);
      if (keep && pos < cap) out[pos] = yfi_fit_candidate(p, i, 7, (int32_t)f, yfdec::d_sig_bits, yfdec::d_exp_bits, m);
    }
    if (lane == 0) counts[f] = total;
  }
}

// 20x20 int8 heads: one workgroup per frame; the tables and the frame's 7200 head bytes in LDS, wave w scans candidates
// [320 w, 320 w + 320) in five chunks of 64 (the confidence byte against q_thr, the smallest byte whose sigmoid passes conf > 0.7f), the
// waves' totals meet in LDS.
constexpr int kCand160 = YF_IMAGES_CAND160;
constexpr int kHead160 = YFI_D160_HEAD_BYTES;
constexpr int kChunks = (kCand160 + 64 * kWaves - 1) / (64 * kWaves);

__global__ void __launch_bounds__(kThreads) decode160_kernel(const int8_t* __restrict__ heads, const yf_image* __restrict__ imgs,
                                                             const int32_t* __restrict__ status, long n, int q_thr,
                                                             yf_det* __restrict__ dets, int* __restrict__ counts, int cap) {
  __shared__ int4 s_head[kHead160 / 16];
  __shared__ uint32_t s_sig[256], s_exp[256];
  __shared__ int s_total[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t below = (1ull << lane) - 1ull;
  s_sig[tid] = yfdec::d_sig_bits[tid];
  s_exp[tid] = yfdec::d_exp_bits[tid];
  for (long f = blockIdx.x; f < n; f += gridDim.x) {
    int h, w;
    if (!frame_ok(imgs, status, f, &h, &w)) {        // the same for every thread of the workgroup
      if (tid == 0) counts[f] = 0;
      continue;
    }
    const yfi_fit_map m = yfi_fit_map_of(h, w, 160);
    __syncthreads();                                 // the previous frame's readers of s_head and s_total are done
    const int4* src = (const int4*)(heads + f * kHead160);
    for (int q = tid; q < kHead160 / 16; q += kThreads) s_head[q] = src[q];
    __syncthreads();
    const int8_t* head = (const int8_t*)s_head;
    auto fires = [&](int c) {                          // chunk c of this wave: does this lane's candidate fire?
      const int i = 64 * (kChunks * wave + c) + lane;
      return i < kCand160 && head[yfi_fit_offset(i < kCand160 ? i : 0, YF_IMAGES_GRID160) + 4] >= q_thr;
    };
    int mine = 0;
#pragma unroll
    for (int c = 0; c < kChunks; ++c) mine += __popcll(__ballot(fires(c)));
    if (lane == 0) s_total[wave] = mine;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      const int t = s_total[k];
      before += k < wave ? t : 0;
      total += t;
    }
    yf_det* out = dets + f * cap;
    int slot0 = before;
#pragma unroll 1
    // One copy of the record's arithmetic, and each chunk's ballot a second time instead of five kept masks: unrolled with the masks kept
    // (the form of yfwide::decode160_kernel), hipcc 7.2's greedy register allocator crashes on this kernel.
    for (int c = 0; c < kChunks; ++c) {
      const bool keep = fires(c);
      const uint64_t mask = __ballot(keep);
      const int slot = slot0 + __popcll(mask & below);
      slot0 += __popcll(mask);
      if (keep && slot < cap) {
        const int i = 64 * (kChunks * wave + c) + lane;
        out[slot] = yfi_fit_candidate(head + yfi_fit_offset(i, YF_IMAGES_GRID160), i, YF_IMAGES_GRID160, (int32_t)f, s_sig, s_exp, m);
      }
    }
    if (tid == 0) counts[f] = total;
  }
}

// the fp16 network's float32 logits [n][7][7][18]: four frames per workgroup, one wave per frame, a frame's 882 logits in LDS; every wave
// of a workgroup makes the same number of trips (the barriers), a wave without a frame idles through them
__global__ void __launch_bounds__(kThreads) decode_f32_kernel(const float* __restrict__ logits, const yf_image* __restrict__ imgs,
                                                              const int32_t* __restrict__ status, long n, yf_det* __restrict__ dets,
                                                              int* __restrict__ counts, int cap) {
  __shared__ float s_t[kWaves][YFI_F32_LOGITS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t below = (1ull << lane) - 1ull;
  float* t = s_t[wave];
  for (long g = blockIdx.x; g * kWaves < n; g += gridDim.x) {
    const long f = g * kWaves + wave;
    bool ok = f < n;
    int h = 1, w = 1;
    if (ok) {
      ok = frame_ok(imgs, status, f, &h, &w);
      if (!ok && lane == 0) counts[f] = 0;
    }
    __syncthreads();                               // the previous frames' readers of s_t are done
    if (ok) {
      const float* src = logits + f * YFI_F32_LOGITS;
      for (int q = lane; q < YFI_F32_LOGITS; q += 64) t[q] = src[q];
    }
    __syncthreads();
    if (!ok) continue;
    const yfi_fit_map m = yfi_fit_map_of(h, w, 56);
    yf_det* out = dets + f * cap;
    int total = 0;
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {                  // one copy of the arithmetic: a pass is complete before the next begins
      const int i = 64 * c + lane;
      const float* p = t + yfi_fit_offset(i < YFI_F32_CAND ? i : 0, 7);
      const float conf = yfi_sigmoid_f32(p[4]);
      const bool keep = i < YFI_F32_CAND && conf > 0.7f;
      const uint64_t mask = __ballot(keep);
      const int pos = total + __popcll(mask & below);
      total += __popcll(mask);
      if (keep && pos < cap) out[pos] = yfi_fit_candidate_f32(p, i, (int32_t)f, conf, m);
    }
    if (lane == 0) counts[f] = total;
  }
}

}  // namespace yffit
#endif
