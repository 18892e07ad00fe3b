// Prediction overlays on the device (devicedata.LesionPredictFeed, predict.py -c 1 -si 1).
// Host mirrors: datasets.fit_to_case_frame (msl_boxes_to_case) and utils.draw_boxes (msl_draw_boxes); both are
// bit-identical to them.
//
//   boxes_to_case : one thread per coordinate; c' = (c * t + (d + lo)) / s as three explicitly rounded f32 operations
//   draw          : one wave per (d, h) row of one image, four rows per workgroup.  A voxel holds j + 1 of the LAST box
//                   whose assignments cover it, i.e. a maximum over j: every lane walks the boxes in ascending j and
//                   overwrites, so no ordering between threads, no memset and no atomics are needed, and every voxel is
//                   written exactly once.  The boxes of the image are converted to voxel boxes DRAW_CHUNK at a time
//                   into LDS (any K works); a wave tests 64 of them at once against its row (one per lane), ballots,
//                   and only walks the hits, reading each from LDS at a wave-uniform address (a broadcast read).  At
//                   K = 100 boxes of ~10 voxels 99.7 % of the rows meet no box and cost two ballots.
//                   A lane owns eight consecutive w: one 16-byte store per plane.  The eight-voxel chunks are laid from
//                   the first 16-byte boundary of the row, so a row of any W at any (2-byte aligned) address takes the
//                   wide store on all but its first and last chunk, which are stored voxel by voxel.
#include "common.hpp"
#include "../../include/mslesions3d_hip.h"

namespace {

constexpr int DRAW_CHUNK = MSL_DRAW_BOXES_CHUNK;  // boxes staged in LDS at a time (one per thread)
constexpr int DRAW_THREADS = 256;                 // four waves = four rows
constexpr int DRAW_ROWS = DRAW_THREADS / MSL_WAVE;
constexpr int MAX_IDS = 32766;                    // j + 1 must fit int16
static_assert(DRAW_CHUNK == DRAW_THREADS, "one staged box per thread");

struct CaseGeom {
  float t[3], add[3], s[3];  // per axis: target size, d + lo, full size - as f32
};

__global__ __launch_bounds__(256) void boxes_to_case_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                            int n_coords, CaseGeom g) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_coords) return;
  const int a = i % 3;  // rows are (x0, y0, z0, x1, y1, z1)
  out[i] = __fdiv_rn(__fadd_rn(__fmul_rn(in[i], g.t[a]), g.add[a]), g.s[a]);
}

// trunc(clip(c, 0, 1) * n): numpy's clip(box, 0, 1) * shape as an f32 product, .astype(int)
__device__ __forceinline__ int voxel_of(float c, int n) {
  const float cl = fminf(fmaxf(c, 0.0f), 1.0f);
  return (int)__fmul_rn(cl, (float)n);
}

// Which voxels of row (x, y) the assignments of one box write: |1 the span [z0, z1), |2 the points z0 and z1,
// |4 the point z1.  style 0 "edges": six half-open faces; style 1 "preds": plus three edge lines and the far corner.
__device__ __forceinline__ int row_kind(int x0, int y0, int x1, int y1, int x, int y, int preds) {
  const bool inX = x >= x0 && x < x1, inY = y >= y0 && y < y1;
  const bool atX = x == x0 || x == x1, atY = y == y0 || y == y1;
  const bool cornerXY = preds && x == x1 && y == y1;
  int k = 0;
  if ((atX && inY) || (inX && atY) || cornerXY) k |= 1;
  if (inX && inY) k |= 2;
  if (preds && ((inX && y == y1) || (x == x1 && inY) || cornerXY)) k |= 4;
  return k;
}

typedef short short8 __attribute__((ext_vector_type(8)));

__global__ __launch_bounds__(DRAW_THREADS) void draw_boxes_kernel(
    const float* __restrict__ boxes, const long long* __restrict__ labels, const float* __restrict__ scores, int K,
    int D, int H, int W, int preds, double min_score, short* __restrict__ inst, short* __restrict__ cls) {
  __shared__ int4 s_lo[DRAW_CHUNK];  // x0, y0, z0, label
  __shared__ int4 s_hi[DRAW_CHUNK];  // x1, y1, z1, j + 1
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long rows = (long long)D * H;
  const long long row = (long long)blockIdx.x * DRAW_ROWS + wv;
  const bool live = row < rows;  // (a wave past the last row still stages boxes and meets the barriers)
  const int x = live ? (int)(row / H) : 0, y = live ? (int)(row % H) : 0;
  short* irow = inst + (live ? row : 0) * W;
  short* crow = cls ? cls + (live ? row : 0) * W : nullptr;
  // chunk c covers w in [head + 8 (c - 1), head + 8 c): chunk 0 is the part of the row before its first 16-byte boundary
  const int head = (int)(((16u - (unsigned)((uintptr_t)irow & 15u)) & 15u) >> 1);
  const bool cls_vec = crow && (((uintptr_t)crow ^ (uintptr_t)irow) & 15u) == 0;
  const int n_chunks = (W - head + 7) / 8 + 1;  // W < head: chunk 0 alone covers the row
  // `head` differs between the waves of a workgroup and the loop below holds barriers: its trip count comes from the
  // largest chunk count any head can give (head = 0), which depends on W alone.  One trip up to W = 504.
  const int max_chunks = (W + 7) / 8 + 1;

  for (int c0 = 0; c0 < max_chunks; c0 += MSL_WAVE) {
    const int c = c0 + lane;
    const int w0 = head + 8 * (c - 1);
    int val[8], lab[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) val[e] = lab[e] = 0;
    for (int k0 = 0; k0 < K; k0 += DRAW_CHUNK) {
      __syncthreads();  // the previous chunk has been read by every wave
      {
        const int j = k0 + (int)threadIdx.x;
        int4 lo = make_int4(-1, -1, -1, 0), hi = make_int4(-1, -1, -1, 0);  // an entry no row meets
        if (j < K) {
          const long long l = labels[j];
          if (!((double)scores[j] < min_score && preds) && l != 0) {
            const float* b = boxes + (size_t)j * 6;
            lo = make_int4(voxel_of(b[0], D), voxel_of(b[1], H), voxel_of(b[2], W), (int)l);
            hi = make_int4(min(voxel_of(b[3], D) + preds, D - 1), min(voxel_of(b[4], H) + preds, H - 1),
                           min(voxel_of(b[5], W) + preds, W - 1), j + 1);
          }
        }
        s_lo[threadIdx.x] = lo;
        s_hi[threadIdx.x] = hi;
      }
      __syncthreads();
      const int staged = min(DRAW_CHUNK, K - k0);
      for (int q0 = 0; q0 < staged && live; q0 += MSL_WAVE) {
        const int4 tl = s_lo[q0 + lane], th = s_hi[q0 + lane];  // (entries past `staged` are stale or unmet: masked)
        const bool hit = q0 + lane < staged && row_kind(tl.x, tl.y, th.x, th.y, x, y, preds) != 0;
        unsigned long long m = __ballot(hit);
        while (m) {
          const int q = q0 + __builtin_ctzll(m);  // ascending j
          m &= m - 1;
          const int4 lo = s_lo[q], hi = s_hi[q];  // wave-uniform address: a broadcast read
          const int kind = row_kind(lo.x, lo.y, hi.x, hi.y, x, y, preds);
          const int z0 = lo.z, z1 = hi.z;
          if (w0 + 7 < min(z0, z1) || w0 > max(z0, z1)) continue;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int w = w0 + e;
            const bool on = ((kind & 1) && w >= z0 && w < z1) || ((kind & 2) && (w == z0 || w == z1)) ||
                            ((kind & 4) && w == z1);
            val[e] = on ? hi.w : val[e];
            lab[e] = on ? lo.w : lab[e];
          }
        }
      }
    }
    if (!live || c >= n_chunks) continue;  // (no barrier follows in this trip)
    if (w0 >= 0 && w0 + 8 <= W) {
      short8 v;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (short)val[e];
      *reinterpret_cast<short8*>(irow + w0) = v;
      if (cls_vec) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (short)lab[e];
        *reinterpret_cast<short8*>(crow + w0) = v;
      } else if (crow) {
#pragma unroll
        for (int e = 0; e < 8; ++e) crow[w0 + e] = (short)lab[e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int w = w0 + e;
        if (w >= 0 && w < W) {
          irow[w] = (short)val[e];
          if (crow) crow[w] = (short)lab[e];
        }
      }
    }
  }
}

}  // namespace

extern "C" {

int msl_boxes_to_case(const float* boxes, const int* offsets, const int* geometry, int N, float* out, void* stream) {
  if (!offsets || !geometry || N < 1) return MSL_ERR_ARG;
  if (offsets[0] < 0) return MSL_ERR_ARG;
  for (int n = 0; n < N; ++n) {
    if (offsets[n + 1] < offsets[n]) return MSL_ERR_ARG;
    for (int a = 0; a < 3; ++a)  // t, n, s positive; lo within the case
      if (geometry[12 * n + a] < 1 || geometry[12 * n + 3 + a] < 1 || geometry[12 * n + 9 + a] < 1 ||
          geometry[12 * n + 6 + a] < 0)
        return MSL_ERR_ARG;
  }
  if (offsets[N] > 0 && (!boxes || !out)) return MSL_ERR_ARG;
  if ((long long)offsets[N] * 6 > 0x7FFFFFFFLL) return MSL_ERR_UNSUPPORTED;
  for (int n = 0; n < N; ++n) {
    const int k0 = offsets[n], cnt = offsets[n + 1] - k0;
    if (cnt == 0) continue;
    CaseGeom g;
    for (int a = 0; a < 3; ++a) {
      const int t = geometry[12 * n + a], m = geometry[12 * n + 3 + a], lo = geometry[12 * n + 6 + a];
      const int d = m < t ? -((t - m) / 2) : m / 2 - t / 2;
      g.t[a] = (float)t;
      g.add[a] = (float)(d + lo);
      g.s[a] = (float)geometry[12 * n + 9 + a];
    }
    MSL_LAUNCH(boxes_to_case_kernel, dim3(msl::cdiv(cnt * 6, 256)), dim3(256), 0, (hipStream_t)stream,
               boxes + (size_t)k0 * 6, out + (size_t)k0 * 6, cnt * 6, g);
  }
  MSL_LAUNCH_CHECK();
  return MSL_OK;
}

int msl_draw_boxes(const float* boxes, const long long* labels, const float* scores, const int* offsets, int N, int D,
                   int H, int W, int style, double min_score, short* instances, short* classes, void* stream) {
  if (!offsets || !instances || N < 1 || D < 1 || H < 1 || W < 1 || (style != 0 && style != 1)) return MSL_ERR_ARG;
  if (offsets[0] < 0) return MSL_ERR_ARG;
  for (int n = 0; n < N; ++n)
    if (offsets[n + 1] < offsets[n] || offsets[n + 1] - offsets[n] > MAX_IDS) return MSL_ERR_ARG;
  if (offsets[N] > 0 && (!boxes || !labels || !scores)) return MSL_ERR_ARG;
  if (((uintptr_t)instances & 1) || ((uintptr_t)classes & 1)) return MSL_ERR_ARG;
  const long long groups = ((long long)D * H + DRAW_ROWS - 1) / DRAW_ROWS;
  if (groups > 0x7FFFFFFFLL) return MSL_ERR_UNSUPPORTED;
  const size_t V = (size_t)D * H * W;
  for (int n = 0; n < N; ++n) {
    const int k0 = offsets[n];
    MSL_LAUNCH(draw_boxes_kernel, dim3((unsigned)groups), dim3(DRAW_THREADS), 0, (hipStream_t)stream,
               boxes ? boxes + (size_t)k0 * 6 : nullptr, labels ? labels + k0 : nullptr, scores ? scores + k0 : nullptr,
               offsets[n + 1] - k0, D, H, W, style, min_score, instances + n * V, classes ? classes + n * V : nullptr);
  }
  MSL_LAUNCH_CHECK();
  return MSL_OK;
}

}  // extern "C"
