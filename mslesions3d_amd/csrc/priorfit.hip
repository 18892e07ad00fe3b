// Prior fit report: which ground-truth boxes the prior set can match at all.
//
// For every ground-truth box g of a data set: the best IoU over all priors and the first prior attaining it, whether g keeps
// the prior the force-match of MultiBoxLoss (ssd3d.py:865-868) hands it, and per (threshold, feature map) the number of
// priors that become positives OF g in training.  These are functions of the (N,P) matching msl_multibox_match writes - 48
// bytes per image and prior - but only a few integers per box: nothing of size (N,P) is stored here.
//
// Two streaming passes over (image, tile of PF_TILE priors); a thread keeps PF_PER priors in registers and the image's boxes
// come through LDS PF_CHUNK at a time (every lane reads the same box: a broadcast, no bank conflict).
//   pass 1, per box: arg-max over priors as the maximum of the 64-bit key (IoU bits << 32) | (0xFFFFFFFF - p).  IoU >= +0, so
//     the bit order is the value order, and the inverted index makes the FIRST prior win.  Thread, wave (skipped when no lane
//     of the wave overlaps the box, which is the common case for small lesions), LDS atomicMax, one global atomicMax per
//     (workgroup, box) that overlapped.  A key starts as "IoU +0 at prior 0", the answer for a box no prior overlaps.
//   pass 2, per prior: the first-maximum box (ascending boxes, strict >) and, in the same loop, the force rule: a box whose
//     best prior (pass 1) is this one claims it, the last claimant stays.  The positives are counted into an LDS copy of the
//     pos rows of PF_CHUNK boxes (one LDS add per wave where the lanes agree) and flushed with integer atomicAdd.
// Everything is integer or max-of-keys: no dependence on scheduling.  The IoU arithmetic is boxmath.hpp's, shared with
// multibox.hip, FMA contraction off: the same bits as the matcher and the CPU oracle.
#include "common.hpp"
#include "../../include/mslesions3d_hip.h"
#pragma clang fp contract(off)

namespace {

#include "boxmath.hpp"

constexpr int PF_THREADS = 256;
constexpr int PF_TILE = MSL_PRIOR_FIT_TILE;    // priors per workgroup
constexpr int PF_PER = PF_TILE / PF_THREADS;   // priors per thread: the wave reduction of pass 1 is paid once for four
constexpr int PF_CHUNK = MSL_PRIOR_FIT_CHUNK;  // boxes staged in LDS at a time
constexpr int PF_MAX_S = MSL_PRIOR_FIT_MAX_SCALES, PF_MAX_T = MSL_PRIOR_FIT_MAX_THRESHOLDS;
constexpr unsigned long long PF_KEY_NONE = 0x00000000FFFFFFFFull;  // IoU +0 at prior 0
static_assert(PF_TILE % PF_THREADS == 0 && PF_CHUNK <= PF_THREADS, "tile / chunk shape");

struct PfSplit {  // the host arrays of the call, by value
  int scale_off[PF_MAX_S + 1];
  float thr[PF_MAX_T];
  int S, n_thr;
};

__device__ __forceinline__ unsigned long long pf_key(float iou, int p) {
  return ((unsigned long long)__float_as_uint(iou) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)p);
}

// the PF_PER priors of this thread as corner boxes (rows past the end repeat the last prior; callers mask them)
__device__ __forceinline__ void pf_load_tile(const float* __restrict__ priors_c, int P, int tile, Box (&pb)[PF_PER],
                                             float (&pv)[PF_PER]) {
#pragma unroll
  for (int u = 0; u < PF_PER; ++u) {
    const int p = tile * PF_TILE + u * PF_THREADS + (int)threadIdx.x;
    pb[u] = c_to_xyz(load_box(priors_c + (size_t)min(p, P - 1) * 6));
    pv[u] = box_vol(pb[u]);
  }
}

// boxes [g0, g0 + cnt) into LDS (cnt <= PF_CHUNK); the caller puts the barriers around it
__device__ __forceinline__ void pf_stage(const float* __restrict__ gt_boxes, int g0, int cnt, float* s_box, float* s_vol) {
  if ((int)threadIdx.x < cnt) {
    const Box g = load_box(gt_boxes + (size_t)(g0 + threadIdx.x) * 6);
#pragma unroll
    for (int q = 0; q < 6; ++q) s_box[threadIdx.x * 6 + q] = g.v[q];
    s_vol[threadIdx.x] = box_vol(g);
  }
}

__global__ __launch_bounds__(256) void pf_init_kernel(unsigned long long* __restrict__ keys, int G, int* __restrict__ pos,
                                                      int npos) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < G) keys[i] = PF_KEY_NONE;
  if (i < npos) pos[i] = 0;
}

// pass 1: keys[g] = max over priors of pf_key(IoU(g, p), p)
__global__ __launch_bounds__(PF_THREADS) void pf_object_best_kernel(const float* __restrict__ gt_boxes,
                                                                    const int* __restrict__ obj_off, int G,
                                                                    const float* __restrict__ priors_c, int P, int tiles,
                                                                    unsigned long long* __restrict__ keys) {
  __shared__ float s_box[PF_CHUNK * 6];
  __shared__ float s_vol[PF_CHUNK];
  __shared__ unsigned long long s_key[PF_CHUNK];
  const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
  const int o0 = max(obj_off[n], 0), o1 = min(obj_off[n + 1], G);
  if (o1 <= o0) return;  // an image without boxes (the same for every thread)
  Box pb[PF_PER];
  float pv[PF_PER];
  pf_load_tile(priors_c, P, tile, pb, pv);
  for (int c0 = o0; c0 < o1; c0 += PF_CHUNK) {
    const int cnt = min(PF_CHUNK, o1 - c0);
    __syncthreads();  // the flush of the chunk before has read s_key
    pf_stage(gt_boxes, c0, cnt, s_box, s_vol);
    if ((int)threadIdx.x < cnt) s_key[threadIdx.x] = 0ull;
    __syncthreads();
    for (int o = 0; o < cnt; ++o) {
      const Box g = load_box(s_box + o * 6);
      const float gv = s_vol[o];
      unsigned long long k = 0ull;
#pragma unroll
      for (int u = 0; u < PF_PER; ++u) {
        const int p = tile * PF_TILE + u * PF_THREADS + (int)threadIdx.x;
        const float v = box_iou(g, gv, pb[u], pv[u]);
        if (p < P && v > 0.f) {
          const unsigned long long ku = pf_key(v, p);
          k = ku > k ? ku : k;
        }
      }
      if (__ballot(k != 0ull) == 0ull) continue;  // wave-uniform: no prior of this wave overlaps the box
      for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(k, off);
        k = other > k ? other : k;
      }
      if ((threadIdx.x & 63) == 0) atomicMax(&s_key[o], k);
    }
    __syncthreads();
    if ((int)threadIdx.x < cnt && s_key[threadIdx.x] != 0ull) atomicMax(&keys[c0 + threadIdx.x], s_key[threadIdx.x]);
  }
}

// keys -> best_iou, best_prior; held[g] = no later box of the image has the same best prior (one workgroup per image)
__global__ __launch_bounds__(256) void pf_finalize_kernel(const int* __restrict__ obj_off, int N, int G,
                                                          const unsigned long long* __restrict__ keys,
                                                          float* __restrict__ best_iou, int* __restrict__ best_prior,
                                                          int* __restrict__ held) {
  for (int n = blockIdx.x; n < N; n += gridDim.x) {
    const int o0 = max(obj_off[n], 0), o1 = min(obj_off[n + 1], G);
    for (int o = o0 + threadIdx.x; o < o1; o += 256) {
      const unsigned long long k = keys[o];
      const unsigned inv = (unsigned)k;
      bool last = true;
      for (int o2 = o + 1; o2 < o1; ++o2) last = last && ((unsigned)keys[o2] != inv);
      best_iou[o] = __uint_as_float((unsigned)(k >> 32));
      best_prior[o] = (int)(0xFFFFFFFFu - inv);
      held[o] = last ? 1 : 0;
    }
  }
}

// pass 2: owner and overlap of every prior after the force-match, counted per (box, threshold, scale range)
__global__ __launch_bounds__(PF_THREADS) void pf_count_kernel(const float* __restrict__ gt_boxes,
                                                              const int* __restrict__ obj_off, int G,
                                                              const float* __restrict__ priors_c, int P, int tiles,
                                                              const int* __restrict__ best_prior, PfSplit sp,
                                                              int* __restrict__ pos) {
  __shared__ float s_box[PF_CHUNK * 6];
  __shared__ float s_vol[PF_CHUNK];
  __shared__ int s_bp[PF_CHUNK];
  __shared__ int s_pos[PF_CHUNK * PF_MAX_T * PF_MAX_S];
  const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
  const int o0 = max(obj_off[n], 0), o1 = min(obj_off[n + 1], G);
  if (o1 <= o0) return;
  const int nobj = o1 - o0, lane = threadIdx.x & 63;
  Box pb[PF_PER];
  float pv[PF_PER];
  pf_load_tile(priors_c, P, tile, pb, pv);
  float best[PF_PER];
  int own[PF_PER], forced[PF_PER];
#pragma unroll
  for (int u = 0; u < PF_PER; ++u) {
    best[u] = 0.f;
    own[u] = 0;
    forced[u] = -1;
  }
  for (int i0 = 0; i0 < nobj; i0 += PF_CHUNK) {
    const int cnt = min(PF_CHUNK, nobj - i0);
    __syncthreads();  // the loop of the chunk before has read the staged boxes
    pf_stage(gt_boxes, o0 + i0, cnt, s_box, s_vol);
    if ((int)threadIdx.x < cnt) s_bp[threadIdx.x] = best_prior[o0 + i0 + threadIdx.x];
    __syncthreads();
    for (int o = 0; o < cnt; ++o) {
      const Box g = load_box(s_box + o * 6);
      const float gv = s_vol[o];
      const int bp = s_bp[o], idx = i0 + o;
#pragma unroll
      for (int u = 0; u < PF_PER; ++u) {
        const int p = tile * PF_TILE + u * PF_THREADS + (int)threadIdx.x;
        const float v = box_iou(g, gv, pb[u], pv[u]);
        if (idx == 0 || v > best[u]) {  // first maximum over the boxes (ssd3d.py:801, :833-837)
          best[u] = v;
          own[u] = idx;
        }
        if (bp == p) forced[u] = idx;  // ascending boxes: the last claimant stays (ssd3d.py:865)
      }
    }
  }
  float ov[PF_PER];
  int sc[PF_PER];
#pragma unroll
  for (int u = 0; u < PF_PER; ++u) {
    const int p = tile * PF_TILE + u * PF_THREADS + (int)threadIdx.x;
    ov[u] = forced[u] >= 0 ? 1.0f : best[u];  // ssd3d.py:868
    own[u] = p >= P ? -1 : (forced[u] >= 0 ? forced[u] : own[u]);
    int s = 0;
    for (int j = 1; j < sp.S; ++j) s += p >= sp.scale_off[j];
    sc[u] = s;
  }
  const int row = sp.n_thr * sp.S;
  for (int i0 = 0; i0 < nobj; i0 += PF_CHUNK) {
    const int cnt = min(PF_CHUNK, nobj - i0);
    __syncthreads();  // the flush of the chunk before has read s_pos
    for (int i = threadIdx.x; i < cnt * row; i += PF_THREADS) s_pos[i] = 0;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PF_PER; ++u) {
      const bool in = own[u] >= i0 && own[u] < i0 + cnt;
      if (__ballot(in) == 0ull) continue;  // wave-uniform
      for (int t = 0; t < sp.n_thr; ++t) {
        const bool hit = in && ov[u] >= sp.thr[t];
        const int addr = hit ? (own[u] - i0) * row + t * sp.S + sc[u] : 0;
        const unsigned long long m = __ballot(hit);
        if (m == 0ull) continue;
        const int leader = __builtin_ctzll(m);
        const int a0 = __shfl(addr, leader);
        if (__ballot(hit && addr != a0) == 0ull) {  // every hit of the wave on one counter: one add
          if (lane == leader) atomicAdd(&s_pos[a0], __popcll(m));
        } else if (hit) {
          atomicAdd(&s_pos[addr], 1);
        }
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cnt * row; i += PF_THREADS) {
      const int v = s_pos[i];
      if (v != 0) atomicAdd(&pos[(size_t)(o0 + i0) * row + i], v);
    }
  }
}

}  // namespace

extern "C" {

size_t msl_prior_fit_workspace_bytes(int G) { return G > 0 ? (size_t)G * sizeof(unsigned long long) : 0; }

int msl_prior_fit(const float* gt_boxes, const int* obj_off, int N, int G, const float* priors_c, int P, const int* scale_off,
                  int S, const float* thr, int n_thr, void* workspace, size_t workspace_bytes, float* best_iou,
                  int* best_prior, int* held, int* pos, void* stream) {
  if (N <= 0 || G < 0 || P <= 0 || S <= 0 || n_thr <= 0 || !obj_off || !priors_c || !scale_off || !thr) return MSL_ERR_ARG;
  if (S > PF_MAX_S || n_thr > PF_MAX_T) return MSL_ERR_UNSUPPORTED;
  PfSplit sp;
  if (scale_off[0] != 0 || scale_off[S] != P) return MSL_ERR_ARG;
  for (int s = 0; s <= PF_MAX_S; ++s) sp.scale_off[s] = s <= S ? scale_off[s] : P;
  for (int s = 0; s < S; ++s)
    if (scale_off[s + 1] < scale_off[s]) return MSL_ERR_ARG;
  for (int t = 0; t < PF_MAX_T; ++t) {
    sp.thr[t] = t < n_thr ? thr[t] : 2.0f;
    if (sp.thr[t] != sp.thr[t]) return MSL_ERR_ARG;  // NaN
  }
  sp.S = S;
  sp.n_thr = n_thr;
  if (G == 0) return MSL_OK;
  if (!gt_boxes || !workspace || !best_iou || !best_prior || !held || !pos || ((uintptr_t)workspace & 7) != 0 ||
      workspace_bytes < msl_prior_fit_workspace_bytes(G))
    return MSL_ERR_ARG;
  const int tiles = msl::cdiv(P, PF_TILE);
  const long long blocks = (long long)tiles * N, npos = (long long)G * n_thr * S;
  if (blocks > 0x7FFFFFFFll || npos > 0x7FFFFFFFll) return MSL_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  MSL_LAUNCH(pf_init_kernel, dim3(msl::cdiv((int)npos, 256)), dim3(256), 0, st, keys, G, pos, (int)npos);
  MSL_LAUNCH(pf_object_best_kernel, dim3((unsigned)blocks), dim3(PF_THREADS), 0, st, gt_boxes, obj_off, G, priors_c, P, tiles,
             keys);
  MSL_LAUNCH(pf_finalize_kernel, dim3(N < 65536 ? N : 65536), dim3(256), 0, st, obj_off, N, G,
             (const unsigned long long*)keys, best_iou, best_prior, held);
  MSL_LAUNCH(pf_count_kernel, dim3((unsigned)blocks), dim3(PF_THREADS), 0, st, gt_boxes, obj_off, G, priors_c, P, tiles,
             (const int*)best_prior, sp, pos);
  MSL_LAUNCH_CHECK();
  return MSL_OK;
}

}  // extern "C"
