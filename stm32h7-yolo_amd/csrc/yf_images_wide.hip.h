// The two kernels of libyf_images.so behind 160x160 frames: the decode of 20x20 heads (1200 candidates per frame) and the IoU suppression
// of up to 1200 records per frame.  Included once by yf_images.hip; C-ABI and semantics: include/yf_images.h.
#ifndef YF_IMAGES_WIDE_HIP_H
#define YF_IMAGES_WIDE_HIP_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/yf_images.h"
#include "yf_images_nms.h"
#include "yf_images_decode160.h"
#include "yf_decode.hip.h"

namespace yfwide {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kCand = YF_IMAGES_CAND160;
constexpr int kHeadBytes = YFI_D160_HEAD_BYTES;                  // 7200 = 450 x 16
constexpr int kChunks = (kCand + 64 * kWaves - 1) / (64 * kWaves);   // 64-candidate chunks per wave: 5 (wave w takes chunks 5w .. 5w + 4)

// Decode of 20x20 heads: one 256-thread workgroup per frame, grid-striding.  The two tables (2 KB, from the __constant__ copies the
// per-image-scale decode of 7x7 heads uses) go to LDS once per workgroup, each frame's 7200 head bytes with 450 16-byte loads.  Candidate
// i = (anchor, row, col) in the script's loop order; wave w scans candidates [320 w, 320 w + 320) in five chunks of 64: the confidence
// byte against q_thr, a ballot per chunk.  The waves' totals meet in LDS, so a record's slot is the number of firing candidates before it;
// boxes are assembled (yfi_d160_candidate) only for the candidates that fire and fit below cap.
template <bool RAGGED>
__global__ void __launch_bounds__(kThreads) decode160_kernel(const int8_t* __restrict__ heads, const yf_image* __restrict__ imgs,
                                                             const int32_t* __restrict__ status, long n, float w_scale, float h_scale,
                                                             int q_thr, yf_det* __restrict__ dets, int* __restrict__ counts, int cap) {
  __shared__ int4 s_head[kHeadBytes / 16];
  __shared__ uint32_t s_sig[256], s_exp[256];
  __shared__ int s_total[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t below = (1ull << lane) - 1ull;
  s_sig[tid] = yfdec::d_sig_bits[tid];
  s_exp[tid] = yfdec::d_exp_bits[tid];
  for (long f = blockIdx.x; f < n; f += gridDim.x) {
    float ws = w_scale, hs = h_scale;
    if (RAGGED) {
      // one descriptor for the whole workgroup: scalar values (read through lane 0), so the branch below is uniform by construction
      const int ih = __builtin_amdgcn_readfirstlane(imgs[f].height), iw = __builtin_amdgcn_readfirstlane(imgs[f].width);
      const int st = status == nullptr ? 0 : __builtin_amdgcn_readfirstlane(status[f]);
      if (ih < 1 || ih > YF_IMAGES_MAX_SIDE || iw < 1 || iw > YF_IMAGES_MAX_SIDE || st != 0) {     // the same for every thread of the workgroup
        if (tid == 0) counts[f] = 0;
        continue;
      }
      ws = (float)((double)iw / 160.0); hs = (float)((double)ih / 160.0);
    }
    __syncthreads();                                 // the previous frame's readers of s_head and s_total are done
    const int4* src = (const int4*)(heads + f * kHeadBytes);
    for (int q = tid; q < kHeadBytes / 16; q += kThreads) s_head[q] = src[q];
    __syncthreads();
    const int8_t* head = (const int8_t*)s_head;
    int pos[kChunks];
    bool keep[kChunks];
    int mine = 0;
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
      const int i = 64 * (kChunks * wave + c) + lane;
      keep[c] = i < kCand && head[yfi_d160_offset(i < kCand ? i : 0) + 4] >= q_thr;
      const uint64_t mask = __ballot(keep[c]);
      pos[c] = mine + __popcll(mask & below);
      mine += __popcll(mask);
    }
    if (lane == 0) s_total[wave] = mine;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int t = s_total[w];
      before += w < wave ? t : 0;
      total += t;
    }
    yf_det* out = dets + f * cap;
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
      const int slot = before + pos[c];
      if (keep[c] && slot < cap) {
        const int i = 64 * (kChunks * wave + c) + lane;
        out[slot] = yfi_d160_candidate(head + yfi_d160_offset(i), i, (int32_t)f, s_sig, s_exp, ws, hs);
      }
    }
    if (tid == 0) counts[f] = total;
  }
}

// Greedy IoU suppression of up to 1200 records per frame (the semantics of nms_kernel, include/yf_images.h).  A 256-thread workgroup takes
// four consecutive frames at a time, grid-striding.  What a frame costs follows its own record count m = min(max(count, 0), cap):
//   m <= 64: one wave, one record per lane, registers only -- no LDS, no barrier.  Wave w takes frame w of the four.  Rank = the number of
//            larger keys (the keys go round by lane reads), the records move to the lane of their rank (ds_permute), the greedy pass reads
//            the kept record's edges from its lane; the alive ranks are one wave-uniform 64-bit mask.
//   m > 64:  the whole workgroup, one such frame after the other.  Keys by record, then edges and the other 12 bytes by rank in LDS (every
//            record of the frame is there before anything is written: d_out may equal d_dets).  Ranks are dealt in chunks of 64: chunk c
//            belongs to wave c % 4 as its slot c / 4, and its alive bits are one 64-bit word, in that wave's registers and in LDS.  For
//            each alive rank t in ascending order every wave tests its alive ranks above t against t's edges, publishes the words that
//            changed, and after one barrier finds the next alive rank in the published words.  Loop bounds come from m: the ranking runs m
//            steps over ceil(m / 256) slots, the greedy pass touches only chunks that hold ranks above t and below m.
// All four counts are read before anything is written (d_out_counts may equal d_counts).
constexpr int kWideMax = YF_IMAGES_NMS_WIDE_MAX_CAP;
constexpr int kSlots = (kWideMax + kThreads - 1) / kThreads;     // 5
constexpr int kWords = (kWideMax + 63) / 64;                     // 19

__device__ __forceinline__ int lane_read(int v, int src) { return __builtin_amdgcn_readlane(v, src); }

__device__ __forceinline__ void nms_one_wave(const int* in, int m, double thr, int* o, int* out_count, int lane) {
  const uint64_t below = (1ull << lane) - 1ull;
  int w[7] = {0, 0, 0, 0, 0, 0, 0};
  uint64_t key = 0;
  if (lane < m) {
#pragma unroll
    for (int q = 0; q < 7; ++q) w[q] = in[lane * 7 + q];
    key = yfi_nms_key_wide((uint32_t)w[2], (uint32_t)lane);
  }
  const int klo = (int)(uint32_t)key, khi = (int)(uint32_t)(key >> 32);
  int rank = 0;
  for (int j = 0; j < m; ++j) {
    const uint64_t kj = ((uint64_t)(uint32_t)lane_read(khi, j) << 32) | (uint64_t)(uint32_t)lane_read(klo, j);
    rank += kj > key;
  }
  if (lane >= m) rank = lane;                          // the lanes without a record keep their place: the ranks are a permutation of 0..63
#pragma unroll
  for (int q = 0; q < 7; ++q) w[q] = __builtin_amdgcn_ds_permute(rank << 2, w[q]);
  const double area = yfi_nms_area(w[3], w[4], w[5], w[6]);
  uint64_t alive = __ballot(lane < m);
  for (uint64_t todo = alive; todo != 0;) {
    const int t = __builtin_ctzll(todo);
    const int ax1 = lane_read(w[3], t), ay1 = lane_read(w[4], t), ax2 = lane_read(w[5], t), ay2 = lane_read(w[6], t);
    const double area_a = yfi_nms_area(ax1, ay1, ax2, ay2);
    bool sup = false;
    if (lane > t && ((alive >> lane) & 1ull)) sup = !yfi_nms_survives(ax1, ay1, ax2, ay2, area_a, w[3], w[4], w[5], w[6], area, thr);
    alive &= ~__ballot(sup);
    todo = t < 63 ? alive & (~0ull << (t + 1)) : 0ull;
  }
  if ((alive >> lane) & 1ull) {
    const int slot = __popcll(alive & below);
#pragma unroll
    for (int q = 0; q < 7; ++q) o[slot * 7 + q] = w[q];
  }
  if (lane == 0) *out_count = __popcll(alive);
}

__global__ void __launch_bounds__(kThreads) nms_wide_kernel(const yf_det* dets, const int* counts, long n, int cap, double thr, yf_det* out,
                                                            int* out_counts) {
  __shared__ uint64_t s_key[kWideMax];         // by record
  __shared__ int4 s_edge[kWideMax];            // x1, y1, x2, y2 by rank
  __shared__ int s_rest[3][kWideMax];          // frame, anchor | row | col | q_conf, conf bits, by rank
  __shared__ uint64_t s_alive[kWords];         // chunk c: ranks 64 c .. 64 c + 63
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t below = (1ull << lane) - 1ull;
  for (long f0 = (long)blockIdx.x * kWaves; f0 < n; f0 += (long)gridDim.x * kWaves) {
    int ms[kWaves];
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      const int c = f0 + k < n ? counts[f0 + k] : 0;
      ms[k] = c < 0 ? 0 : (c > cap ? cap : c);
    }
    __syncthreads();                           // every thread has the four counts; the previous group's LDS readers are done
    auto count_of = [&](int k) { return k == 0 ? ms[0] : (k == 1 ? ms[1] : (k == 2 ? ms[2] : ms[3])); };   // selects: ms stays in registers
    if (f0 + wave < n && count_of(wave) <= 64)
      nms_one_wave((const int*)(dets + (f0 + wave) * cap), count_of(wave), thr, (int*)(out + (f0 + wave) * cap), out_counts + f0 + wave, lane);
#pragma unroll 1
    for (int k = 0; k < kWaves; ++k) {
      const int m = count_of(k);
      if (m <= 64) continue;                   // the same for every thread of the workgroup
      const long f = f0 + k;
      const int* in = (const int*)(dets + f * cap);
      const int chunks = (m + 63) >> 6;
      uint64_t key[kSlots];
      int w[kSlots][7];
#pragma unroll
      for (int s = 0; s < kSlots; ++s) {
        const int r = tid + kThreads * s;
        key[s] = 0;
        if (r < m) {
#pragma unroll
          for (int q = 0; q < 7; ++q) w[s][q] = in[r * 7 + q];
          key[s] = yfi_nms_key_wide((uint32_t)w[s][2], (uint32_t)r);
          s_key[r] = key[s];
        }
      }
      __syncthreads();
      int rank[kSlots] = {0, 0, 0, 0, 0};
      for (int j = 0; j < m; ++j) {
        const uint64_t kj = s_key[j];
#pragma unroll
        for (int s = 0; s < kSlots; ++s)
          if (kThreads * s < m) rank[s] += kj > key[s];
      }
#pragma unroll
      for (int s = 0; s < kSlots; ++s) {
        if (tid + kThreads * s < m) {
          const int p = rank[s];
          s_edge[p] = make_int4(w[s][3], w[s][4], w[s][5], w[s][6]);
          s_rest[0][p] = w[s][0]; s_rest[1][p] = w[s][1]; s_rest[2][p] = w[s][2];
        }
      }
      __syncthreads();
      // chunk c = kWaves * s + wave is this wave's slot s: rank p = 64 c + lane
      int4 e[kSlots];
      double area[kSlots];
      uint64_t alive[kSlots];
#pragma unroll
      for (int s = 0; s < kSlots; ++s) {
        const int c = kWaves * s + wave, p = 64 * c + lane;
        e[s] = make_int4(0, 0, 0, 0);
        if (p < m) e[s] = s_edge[p];
        area[s] = yfi_nms_area(e[s].x, e[s].y, e[s].z, e[s].w);
        alive[s] = __ballot(p < m);
        if (c < kWords && lane == 0) s_alive[c] = alive[s];
      }
      __syncthreads();
      int t = 0;                               // rank 0 exists (m > 64) and is alive
      while (t < m) {
        const int4 a = s_edge[t];
        const double area_a = yfi_nms_area(a.x, a.y, a.z, a.w);
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
          const int c = kWaves * s + wave;
          const int lo = t + 1 - 64 * c;                         // ranks of this chunk at and above bit `lo` are above t
          if (c >= chunks || lo >= 64 || (lo > 0 ? alive[s] & (~0ull << lo) : alive[s]) == 0) continue;
          const int p = 64 * c + lane;
          bool sup = false;
          if (p > t && ((alive[s] >> lane) & 1ull))
            sup = !yfi_nms_survives(a.x, a.y, a.z, a.w, area_a, e[s].x, e[s].y, e[s].z, e[s].w, area[s], thr);
          const uint64_t gone = __ballot(sup);
          if (gone) {
            alive[s] &= ~gone;
            if (lane == 0) s_alive[c] = alive[s];
          }
        }
        __syncthreads();
        // the next alive rank above t.  A wave that is already a step ahead may have cleared bits above that rank meanwhile: the rank
        // itself and every bit below it are as this step left them.
        int next = m;
        for (int c = (t + 1) >> 6; c < chunks; ++c) {
          uint64_t word = s_alive[c];
          const int lo = t + 1 - 64 * c;
          if (lo > 0) word &= ~0ull << lo;
          if (word) { next = 64 * c + __builtin_ctzll(word); break; }
        }
        t = next;
      }
      __syncthreads();                         // (the last step published nothing after its barrier; this orders the output's reads anyway)
      int* o = (int*)(out + f * cap);
      int kept = 0;
      for (int c = 0; c < chunks; ++c) {
        const uint64_t word = s_alive[c];
        if ((c & (kWaves - 1)) == wave && ((word >> lane) & 1ull)) {
          const int p = 64 * c + lane, slot = kept + __popcll(word & below);
          const int4 ed = s_edge[p];
          o[slot * 7 + 0] = s_rest[0][p]; o[slot * 7 + 1] = s_rest[1][p]; o[slot * 7 + 2] = s_rest[2][p];
          o[slot * 7 + 3] = ed.x; o[slot * 7 + 4] = ed.y; o[slot * 7 + 5] = ed.z; o[slot * 7 + 6] = ed.w;
        }
        kept += __popcll(word);
      }
      if (tid == 0) out_counts[f] = kept;
      __syncthreads();                         // this frame's LDS is read before the next wide frame's records land
    }
  }
}

}  // namespace yfwide
#endif
