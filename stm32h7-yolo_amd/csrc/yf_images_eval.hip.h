// The kernels of libyf_images.so that score detection records against ground-truth boxes: the match of every frame's records to its
// ground truths and the average precision of the whole batch (calculate_iou / calculate_ap / calculate_map of
// yoloface/tensorflow/yolov3_train_tf.py:657-759; the arithmetic: yf_images_eval.h).  Included once by yf_images.hip; C-ABI and
// semantics: include/yf_images.h.  Every workgroup but those of the three one-workgroup scans is ONE wave, so a __syncthreads() orders
// that wave's LDS traffic and every loop bound around one is the same for all of its lanes.
#ifndef YF_IMAGES_EVAL_HIP_H
#define YF_IMAGES_EVAL_HIP_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/yf_images.h"
#include "yf_images_eval.h"

namespace yfeval {

constexpr int kMaxGt = YF_IMAGES_EVAL_MAX_GT;
constexpr int kMaxRec = YF_IMAGES_NMS_WIDE_MAX_CAP;
constexpr int kTile = YF_IMAGES_EVAL_SORT_TILE;                  // records per tile of the sort and of the curve: one wave's work
constexpr int kChunks = kTile / 64;
constexpr int kScan = 256;                                       // threads of a one-workgroup scan
static_assert(kTile % 64 == 0 && kMaxRec < 2048, "whole chunks; the claim key has 11 bits of slot");

// ---- match ----
// One wave per frame (one-wave workgroups, grid-striding), in passes of 64 records, so a frame costs records x ground truths of its own
// counts.  The frame's ground truths go to LDS once; lane L of a pass takes record 64 p + L: the IoU with every ground truth in order
// (LDS broadcasts), the best one, whether it is a candidate.  The claim is a minimum: every candidate puts its claim key (order of the
// detections, yfi_eval_claim_key) on its best ground truth with an LDS atomic min, and after the barrier the candidate whose key stands
// there is the true positive -- the one the reference's loop reaches first.
__global__ void __launch_bounds__(64) match_kernel(const yf_det* __restrict__ dets, const int* __restrict__ counts, long n, int cap,
                                                   const yf_gt_box* __restrict__ gt, const int32_t* __restrict__ gt_counts, int gt_cap,
                                                   double thr, uint8_t* __restrict__ tp, int32_t* __restrict__ best_out) {
  __shared__ double s_gt[kMaxGt * 4];
  __shared__ unsigned long long s_claim[kMaxGt];
  __shared__ int16_t s_cand[kMaxRec];                  // the best ground truth of a candidate, -1 for any other record
  const int lane = threadIdx.x;
  for (long f = blockIdx.x; f < n; f += gridDim.x) {
    const int m = __builtin_amdgcn_readfirstlane(yfi_eval_clamp(counts[f], cap));
    const int k = __builtin_amdgcn_readfirstlane(yfi_eval_clamp(gt_counts[f], gt_cap));
    __syncthreads();                                   // the previous frame's readers of the LDS are done
    const double* g = (const double*)(gt + f * gt_cap);
    for (int q = lane; q < 4 * k; q += 64) s_gt[q] = g[q];
    for (int q = lane; q < k; q += 64) s_claim[q] = ~0ull;
    __syncthreads();
    const int* in = (const int*)(dets + f * cap);
    for (int r = lane; r < m; r += 64) {
      const int32_t x1 = in[r * 7 + 3], y1 = in[r * 7 + 4], x2 = in[r * 7 + 5], y2 = in[r * 7 + 6];
      double best_iou = 0.0;
      int best = -1;
      for (int j = 0; j < k; ++j) {
        const double iou = yfi_eval_iou(x1, y1, x2, y2, s_gt[4 * j], s_gt[4 * j + 1], s_gt[4 * j + 2], s_gt[4 * j + 3]);
        if (iou > best_iou) { best_iou = iou; best = j; }
      }
      const bool cand = best_iou >= thr && best >= 0;
      s_cand[r] = (int16_t)(cand ? best : -1);
      if (best_out) best_out[f * cap + r] = best;
      if (cand) atomicMin(&s_claim[best], (unsigned long long)yfi_eval_claim_key((uint32_t)in[r * 7 + 2], (uint32_t)r));
    }
    __syncthreads();
    for (int r = lane; r < m; r += 64) {
      const int b = s_cand[r];
      tp[f * cap + r] = (uint8_t)(b >= 0 && s_claim[b] == yfi_eval_claim_key((uint32_t)in[r * 7 + 2], (uint32_t)r));
    }
  }
}

// ---- average precision ----
// The caller's workspace.  head: {m = records of the batch, num_gt, tiles = ceil(m / kTile), true positives}, written on the device
// and read by every later kernel: the host never learns m, so every grid is sized by the capacity n * cap and strides over `tiles`.
struct Work {
  int64_t* head;               // [8]
  double* tile_max;            // [tiles]  the largest precision inside a tile
  double* tile_sufmax;         // [tiles]  ... and over all later tiles
  double* terms;               // [n * cap] the term of the k-th true positive
  int32_t* offsets;            // [n + 1]  records before frame f
  uint32_t* key[2];            // [n * cap] order keys, ping and pong
  uint32_t* hist;              // [tiles][256] digit counts of a tile, then (scanned) where a tile's records of a digit go
  int32_t* tile_sum;           // [tiles]  true positives inside a tile
  int32_t* tile_base;          // [tiles]  ... and before it
  uint8_t* val[2];             // [n * cap] the flag that travels with a key
  size_t bytes;
};

inline Work layout(void* base, long n, int cap) {
  const size_t C = (size_t)n * (size_t)cap, tiles = (C + kTile - 1) / kTile;
  size_t off = 0;
  const auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 15) & ~(size_t)15; return (char*)base + at; };
  Work w;
  w.head = (int64_t*)take(64);
  w.tile_max = (double*)take(tiles * 8);
  w.tile_sufmax = (double*)take(tiles * 8);
  w.terms = (double*)take(C * 8);
  w.offsets = (int32_t*)take(((size_t)n + 1) * 4);
  w.key[0] = (uint32_t*)take(C * 4);
  w.key[1] = (uint32_t*)take(C * 4);
  w.hist = (uint32_t*)take(tiles * 256 * 4);
  w.tile_sum = (int32_t*)take(tiles * 4);
  w.tile_base = (int32_t*)take(tiles * 4);
  w.val[0] = (uint8_t*)take(C);
  w.val[1] = (uint8_t*)take(C);
  w.bytes = off;
  return w;
}

// One workgroup: the records before each frame (offsets[n] = m), the ground truths of the batch, the head.  Thread t takes a contiguous
// run of frames; the runs' sums meet in LDS.
__global__ void __launch_bounds__(kScan) offsets_kernel(const int* __restrict__ counts, const int32_t* __restrict__ gt_counts, long n, int cap,
                                                        int gt_cap, int32_t* __restrict__ offsets, int64_t* __restrict__ head) {
  __shared__ int64_t s_rec[kScan], s_gt[kScan];
  const int tid = threadIdx.x;
  const long seg = (n + kScan - 1) / kScan, lo = tid * seg < n ? tid * seg : n, hi = lo + seg < n ? lo + seg : n;
  int64_t rec = 0, gts = 0;
  for (long f = lo; f < hi; ++f) { rec += yfi_eval_clamp(counts[f], cap); gts += yfi_eval_clamp(gt_counts[f], gt_cap); }
  s_rec[tid] = rec; s_gt[tid] = gts;
  __syncthreads();
  int64_t run = 0;
  for (int t = 0; t < tid; ++t) run += s_rec[t];
  for (long f = lo; f < hi; ++f) { offsets[f] = (int32_t)run; run += yfi_eval_clamp(counts[f], cap); }
  if (tid == 0) {
    int64_t m = 0, num_gt = 0;
    for (int t = 0; t < kScan; ++t) { m += s_rec[t]; num_gt += s_gt[t]; }
    offsets[n] = (int32_t)m;
    head[0] = m; head[1] = num_gt; head[2] = (m + kTile - 1) / kTile; head[3] = 0;
  }
}

// One wave per frame: its records' order keys and flags to their positions in the batch (frame, then slot: already the order of ties)
__global__ void __launch_bounds__(256) gather_kernel(const yf_det* __restrict__ dets, const int* __restrict__ counts, const uint8_t* __restrict__ tp,
                                                     long n, int cap, const int32_t* __restrict__ offsets, uint32_t* __restrict__ key,
                                                     uint8_t* __restrict__ val) {
  const int lane = threadIdx.x & 63;
  for (long f = (long)blockIdx.x * 4 + (threadIdx.x >> 6); f < n; f += (long)gridDim.x * 4) {
    const int m = yfi_eval_clamp(counts[f], cap);
    const int* in = (const int*)(dets + f * cap);
    const long at = offsets[f];
    for (int r = lane; r < m; r += 64) {
      key[at + r] = yfi_eval_key((uint32_t)in[r * 7 + 2]);
      val[at + r] = (uint8_t)(tp[f * cap + r] != 0);
    }
  }
}

// The order: a stable least-significant-digit radix sort of the keys, 8 bits a pass, four passes of three launches.  A tile is kTile
// consecutive records and one wave's work.
// (1) the tile's count of each digit
__global__ void __launch_bounds__(64) hist_kernel(const uint32_t* __restrict__ key, int shift, const int64_t* __restrict__ head,
                                                  uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_cnt[256];
  const int lane = threadIdx.x;
  const long m = head[0], tiles = head[2];
  for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
#pragma unroll
    for (int q = 0; q < 4; ++q) s_cnt[lane + 64 * q] = 0;
    __syncthreads();
    for (int c = 0; c < kChunks; ++c) {
      const long i = t * kTile + c * 64 + lane;
      if (i < m) atomicAdd(&s_cnt[(key[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) hist[t * 256 + lane + 64 * q] = s_cnt[lane + 64 * q];
    __syncthreads();
  }
}

// (2) one workgroup, thread d owns digit d: counts -> where the records of digit d in tile t go (digits ascending, then tiles ascending)
__global__ void __launch_bounds__(kScan) digit_scan_kernel(const int64_t* __restrict__ head, uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_tot[256];
  const int d = threadIdx.x;
  const long tiles = head[2];
  uint32_t total = 0;
  for (long t = 0; t < tiles; ++t) total += hist[t * 256 + d];
  s_tot[d] = total;
  __syncthreads();
  uint32_t run = 0;
  for (int e = 0; e < d; ++e) run += s_tot[e];
  for (long t = 0; t < tiles; ++t) {
    const uint32_t v = hist[t * 256 + d];
    hist[t * 256 + d] = run;
    run += v;
  }
}

// (3) the tile's records to their places, chunk by chunk in input order: a record's place is its digit's running base (LDS) plus the
// number of lower lanes of the chunk with the same digit (eight ballots); the highest lane of each digit moves the base on.  Stable.
__global__ void __launch_bounds__(64) scatter_kernel(const uint32_t* __restrict__ key, const uint8_t* __restrict__ val,
                                                     uint32_t* __restrict__ key_out, uint8_t* __restrict__ val_out, int shift,
                                                     const int64_t* __restrict__ head, const uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_base[256];
  const int lane = threadIdx.x;
  const uint64_t below = (1ull << lane) - 1ull;
  const long m = head[0], tiles = head[2];
  for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
    __syncthreads();                                   // the previous tile's readers of s_base are done
#pragma unroll
    for (int q = 0; q < 4; ++q) s_base[lane + 64 * q] = hist[t * 256 + lane + 64 * q];
    __syncthreads();
    for (int c = 0; c < kChunks; ++c) {
      const long i = t * kTile + c * 64 + lane;
      const bool valid = i < m;
      const uint32_t k = valid ? key[i] : 0u;
      const uint8_t v = valid ? val[i] : (uint8_t)0;
      const uint32_t d = (k >> shift) & 255u;
      uint64_t same = __ballot(valid);
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const uint64_t bal = __ballot(bit);
        same &= bit ? bal : ~bal;
      }
      const uint32_t dest = valid ? s_base[d] + (uint32_t)__popcll(same & below) : 0u;
      __syncthreads();
      if (valid && (same >> lane) == 1ull) s_base[d] += (uint32_t)__popcll(same);
      __syncthreads();
      if (valid) { key_out[dest] = k; val_out[dest] = v; }
    }
  }
}

// The curve over the sorted flags, tile by tile.  (1) true positives inside each tile
__global__ void __launch_bounds__(64) tile_count_kernel(const uint8_t* __restrict__ val, const int64_t* __restrict__ head,
                                                        int32_t* __restrict__ tile_sum) {
  const int lane = threadIdx.x;
  const long m = head[0], tiles = head[2];
  for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
    int total = 0;
    for (int c = 0; c < kChunks; ++c) {
      const long i = t * kTile + c * 64 + lane;
      total += __popcll(__ballot(i < m && val[i] != 0));
    }
    if (lane == 0) tile_sum[t] = total;
  }
}

// (2) one workgroup: true positives before each tile, and of the batch (head[3])
__global__ void __launch_bounds__(kScan) tile_base_kernel(int64_t* __restrict__ head, const int32_t* __restrict__ tile_sum,
                                                          int32_t* __restrict__ tile_base) {
  __shared__ int64_t s_sum[kScan];
  const int tid = threadIdx.x;
  const long tiles = head[2];
  const long seg = (tiles + kScan - 1) / kScan, lo = tid * seg < tiles ? tid * seg : tiles, hi = lo + seg < tiles ? lo + seg : tiles;
  int64_t sum = 0;
  for (long t = lo; t < hi; ++t) sum += tile_sum[t];
  s_sum[tid] = sum;
  __syncthreads();
  int64_t run = 0;
  for (int t = 0; t < tid; ++t) run += s_sum[t];
  for (long t = lo; t < hi; ++t) { tile_base[t] = (int32_t)run; run += tile_sum[t]; }
  if (tid == kScan - 1) head[3] = run;                 // the last thread's run ends at the total (an empty run starts there)
}

__device__ __forceinline__ double dmax(double a, double b) { return b > a ? b : a; }

// (3) the largest precision inside each tile
__global__ void __launch_bounds__(64) tile_max_kernel(const uint8_t* __restrict__ val, const int64_t* __restrict__ head,
                                                      const int32_t* __restrict__ tile_base, double* __restrict__ tile_max) {
  const int lane = threadIdx.x;
  const uint64_t upto = (2ull << lane) - 1ull;         // this lane and the lower ones
  const long m = head[0], tiles = head[2];
  for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
    int base = tile_base[t];
    double best = 0.0;
    for (int c = 0; c < kChunks; ++c) {
      const long i = t * kTile + c * 64 + lane;
      const bool valid = i < m;
      const uint64_t bal = __ballot(valid && val[i] != 0);
      const double ctp = (double)(base + __popcll(bal & upto));
      if (valid) best = dmax(best, yfi_eval_precision(ctp, (double)(i + 1) - ctp));
      base += __popcll(bal);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) best = dmax(best, __shfl_xor(best, off));
    if (lane == 0) tile_max[t] = best;
  }
}

// (4) one workgroup: the largest precision over all later tiles (0.0 after the last one: no precision is below it)
__global__ void __launch_bounds__(kScan) tile_sufmax_kernel(const int64_t* __restrict__ head, const double* __restrict__ tile_max,
                                                            double* __restrict__ tile_sufmax) {
  __shared__ double s_max[kScan];
  const int tid = threadIdx.x;
  const long tiles = head[2];
  const long seg = (tiles + kScan - 1) / kScan, lo = tid * seg < tiles ? tid * seg : tiles, hi = lo + seg < tiles ? lo + seg : tiles;
  double mx = 0.0;
  for (long t = lo; t < hi; ++t) mx = dmax(mx, tile_max[t]);
  s_max[tid] = mx;
  __syncthreads();
  double run = 0.0;
  for (int t = tid + 1; t < kScan; ++t) run = dmax(run, s_max[t]);
  for (long t = hi - 1; t >= lo; --t) { tile_sufmax[t] = run; run = dmax(run, tile_max[t]); }
}

// (5) the tile from its last chunk to its first: the envelope (the running maximum from the back), the curve if it is wanted, and the
// term of every true positive at its rank among the true positives.  Position 0 has no term in the reference: a true positive there
// contributes 0.0.
__global__ void __launch_bounds__(64) curve_kernel(const uint8_t* __restrict__ val, const int64_t* __restrict__ head,
                                                   const int32_t* __restrict__ tile_base, const double* __restrict__ tile_sufmax,
                                                   double* __restrict__ terms, double* __restrict__ curve) {
  __shared__ int s_cbase[kChunks];
  const int lane = threadIdx.x;
  const uint64_t upto = (2ull << lane) - 1ull;
  const long m = head[0], tiles = head[2];
  const int64_t num_gt = head[1];
  for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
    __syncthreads();                                   // the previous tile's readers of s_cbase are done
    int base = tile_base[t];
    for (int c = 0; c < kChunks; ++c) {
      const long i = t * kTile + c * 64 + lane;
      if (lane == 0) s_cbase[c] = base;
      base += __popcll(__ballot(i < m && val[i] != 0));
    }
    __syncthreads();
    double later = tile_sufmax[t];
    for (int c = kChunks - 1; c >= 0; --c) {
      const long i = t * kTile + c * 64 + lane;
      const bool valid = i < m;
      const bool hit = valid && val[i] != 0;
      const uint64_t bal = __ballot(hit);
      const double ctp = (double)(s_cbase[c] + __popcll(bal & upto));
      double sm = valid ? yfi_eval_precision(ctp, (double)(i + 1) - ctp) : 0.0;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_down(sm, off);
        if (lane + off < 64) sm = dmax(sm, o);
      }
      const double env = dmax(sm, later);
      later = dmax(later, __shfl(sm, 0));
      if (valid && curve) { curve[2 * i] = yfi_eval_recall(ctp, num_gt); curve[2 * i + 1] = env; }
      if (hit) terms[(long)ctp - 1] = i >= 1 ? yfi_eval_term(ctp, num_gt, env) : 0.0;
    }
  }
}

// (6) one wave: the terms added in order.  Every lane adds the same 64 values of a pass one after the other (a broadcast each); the
// 0.0 beyond the last term leaves the sum as it is.
__global__ void __launch_bounds__(64) sum_kernel(const int64_t* __restrict__ head, const double* __restrict__ terms,
                                                 yf_eval_result* __restrict__ result) {
  const int lane = threadIdx.x;
  const int64_t tp = head[3];
  double ap = 0.0;
  for (int64_t b = 0; b < tp; b += 64) {
    const double v = b + lane < tp ? terms[b + lane] : 0.0;
#pragma unroll 8
    for (int l = 0; l < 64; ++l) ap += __shfl(v, l);
  }
  if (lane == 0) { result->ap = ap; result->detections = head[0]; result->ground_truths = head[1]; result->true_positives = tp; }
}

}  // namespace yfeval
#endif
