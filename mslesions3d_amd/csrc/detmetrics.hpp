// Device helpers shared by the detection-metric kernels (metrics.hip: one workgroup per IoU threshold; evaluate.hip: the
// multi-launch dataset sweep).  Both files are compiled with FMA contraction off: every helper keeps the host's
// (utils.py) operation order, so the outputs are bit-identical to calculate_mAP, NaNs included.
#pragma once
#include "common.hpp"
#pragma clang fp contract(off)

namespace msl {

// fp32, same operation order as utils.py::_iou_one_to_many / multibox.hip box_iou (a = detection, b = ground truth)
__device__ __forceinline__ float det_gt_iou(const float* a, const float* b) {
  float e[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float lo = fmaxf(a[i], b[i]);
    const float hi = fminf(a[3 + i], b[3 + i]);
    e[i] = fmaxf(hi - lo, 0.0f);
  }
  const float inter = e[0] * e[1] * e[2];
  const float va = (a[3] - a[0]) * (a[4] - a[1]) * (a[5] - a[2]);
  const float vb = (b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2]);
  return inter / (va + vb - inter);
}

struct Best {
  float v;
  int g;  // ground-truth index, -1 = none
};

// numpy argmax over a list: the first NaN if there is one, else the first maximum.  Commutative and associative on
// (value, index) pairs, so a butterfly over the wave gives every lane the same answer.
__device__ __forceinline__ Best pick(Best a, Best b) {
  if (b.g < 0) return a;
  if (a.g < 0) return b;
  const bool an = isnan(a.v), bn = isnan(b.v);
  if (an != bn) return an ? a : b;
  if (!an && a.v != b.v) return a.v > b.v ? a : b;
  return a.g < b.g ? a : b;
}

// pick() over the 64 lanes of the wave; every lane gets the answer
__device__ __forceinline__ Best wave_pick(Best best) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const Best c = {__shfl_xor(best.v, o, 64), __shfl_xor(best.g, o, 64)};
    best = pick(best, c);
  }
  return best;
}

// block-wide exclusive prefix of one int per thread (WAVES waves); `tot` receives the total.  Uses `scratch` (WAVES ints).
template <int WAVES>
__device__ __forceinline__ int block_excl_scan(int v, int* scratch, int& tot) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  __syncthreads();  // scratch may still be read by an earlier call
  if (lane == 63) scratch[w] = incl;
  __syncthreads();
  int before = 0;
  tot = 0;
  for (int k = 0; k < WAVES; ++k) {
    const int s = scratch[k];
    if (k < w) before += s;
    tot += s;
  }
  return before + incl - v;
}

constexpr int MT_NREC = 11;  // recall thresholds of the 11-point table (utils.py:336)

// precs.mean(dtype=float32) of the 11-point table: numpy's pairwise sum (eight accumulators, then the tail in sequence),
// then / 11
__device__ __forceinline__ float mean11_pairwise(const float* p) {
  float s = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
  s = s + p[8];
  s = s + p[9];
  s = s + p[10];
  return s / 11.0f;
}

}  // namespace msl
