// Device-resident training data (mslesions3d_amd/devicedata.py): the per-sample host pipeline of datasets._Cases on the
// GPU.  Host mirrors: datasets._Cases.__getitem__ (NormalizeIntensity(nonzero)), datasets._aug_flip / _aug_rotate90 /
// _aug_affine (scipy.ndimage.affine_transform, mode "reflect") and datasets.boxes_from_segmentation (scipy.ndimage.label).
//
//   normalize : one workgroup per cached case, population mean / std of the non-zero voxels in f64 with a fixed
//               combination order, then (x - mean) / std in f32 as the host writes it
//   sampling  : six kernels resample a volume, all through the one core of resample.hpp (row decode, permuted source
//               view, axis taps, eight-corner sum, intensity operations, four-wide store), which follows scipy's
//               NI_GeometricTransform for order 0 / 1 operation by operation in f64 (this file is built with
//               -ffp-contract=off).  Each adds its coordinates and its layout:
//     resample: one launch per affine stage, c = o * zoom + offset under reflect; the first also gathers the sample from
//               the cache through its signed axis permutation (flip + rot90s)
//     affine  : c = M o + offset (rotation) with the boundaries reflect / nearest / constant and up to four f32
//               intensity operations applied in the store; without an affine drawn, a permuted copy with that arithmetic
//     fit     : affine on a ragged case of C channels behind a clamped shift (centred fit or window), four voxels a thread
//     warp    : zoom / grid distortion of a ragged case through three per-axis coordinate tables (msl_augment_warp_mc),
//               bit-identical to scipy.ndimage.map_coordinates on their meshgrid; one wave per output row
//     deform  : free-form deformation of a ragged case (msl_augment_deform_mc): the coordinates are q + d(q), d a cubic
//               B-spline of a 3 x L^3 lattice evaluated per voxel; one wave per output row, the row's part in LDS
//     regrid  : a native case onto the LPI 1 mm grid (signed axis permutation + per-axis step), bit-identical to
//               datasets.regrid; column entries in LDS; at the end of this file
//   boxes     : 6-connected components of every class by union-find (hook the larger root under the smaller: root =
//               minimum linear index = the component's first voxel in C raster order = scipy's numbering), per-tile
//               root counts, one scan into (image, class, tile) order, root ranks, integer min / max extents by
//               atomics, then one workgroup drops flat components and writes the packed targets of msl_multibox_match.
// Launch boundaries on one stream are the only hand-offs between workgroups, except the union-find links, which are
// read with agent-scope atomic loads and written with atomicMin (the result does not depend on the order).
#include "common.hpp"
#pragma clang fp contract(off)

namespace {

#include "resample.hpp"

constexpr int DP_THREADS = 256;
constexpr int NORM_THREADS = 1024;
constexpr int CC_PER_THREAD = 16;
constexpr int CC_TILE = DP_THREADS * CC_PER_THREAD;  // voxels per workgroup of the count / rank passes
constexpr int CC_MAX_CLASSES = 8;
constexpr int FIN_THREADS = 1024;
constexpr int SCAN_THREADS = 1024;
constexpr int BG = -1;  // background voxel in the link array; a root's rank r is stored as -(r + 2)

// ---- normalize ------------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {  // fixed tree order: run-to-run identical
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = NORM_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
    __syncthreads();
  }
  const T r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(NORM_THREADS) void normalize_kernel(float* __restrict__ img, long long V) {
  __shared__ double redd[NORM_THREADS];
  __shared__ long long redi[NORM_THREADS];
  float* x = img + (long long)blockIdx.x * V;
  double s = 0.0;
  long long c = 0;
  for (long long i = threadIdx.x; i < V; i += NORM_THREADS) {
    const float v = x[i];
    if (v != 0.0f) {
      s += (double)v;
      ++c;
    }
  }
  s = block_sum(s, redd);
  c = block_sum(c, redi);
  if (c == 0) return;  // all-zero volume: unchanged
  const double mean = s / (double)c;
  double q = 0.0;
  for (long long i = threadIdx.x; i < V; i += NORM_THREADS) {
    const float v = x[i];
    if (v != 0.0f) {
      const double d = (double)v - mean;
      q += d * d;
    }
  }
  q = block_sum(q, redd);
  const float mean_f = (float)mean;
  float std_f = (float)sqrt(q / (double)c);
  if (std_f == 0.0f) std_f = 1.0f;
  for (long long i = threadIdx.x; i < V; i += NORM_THREADS) {
    const float v = x[i];
    if (v != 0.0f) x[i] = __fdiv_rn(__fsub_rn(v, mean_f), std_f);
  }
}

// ---- resample -------------------------------------------------------------------------------------------------------
// params (N, PARAM_STRIDE) f64 per sample: the common head of a row (resample.hpp) with [7] affine on (1) / off (0), then
// zoom 0..2, offset 0..2.  With the affine on, voxel q of the permutation is sampled at c_a = o_a * zoom_a + offset_a
// under reflect.
__global__ __launch_bounds__(DP_THREADS) void resample_kernel(
    const float* __restrict__ src_img, const unsigned char* __restrict__ src_seg, int n_src,
    const double* __restrict__ params, int D, int H, int W, float* __restrict__ dst_img,
    unsigned char* __restrict__ dst_seg) {
  const long long V = (long long)D * H * W;
  const long long o = (long long)blockIdx.x * DP_THREADS + threadIdx.x;
  if (o >= V) return;
  const int n = blockIdx.y;
  const double* p = params + (size_t)n * PARAM_STRIDE;
  float* di = dst_img + (long long)n * V + o;
  unsigned char* ds = dst_seg + (long long)n * V + o;
  const SrcView<unsigned char> v = view_fixed(src_img, src_seg, n_src, p, D, H, W);
  if (!v.ok) {
    *di = 0.0f;
    *ds = 0;
    return;
  }
  const int oc[3] = {(int)(o / ((long long)H * W)), (int)((o / W) % H), (int)(o % W)};
  if (p[7] == 0.0) {
    const long long s = v.base + oc[0] * v.pst[0] + oc[1] * v.pst[1] + oc[2] * v.pst[2];
    *di = v.si[s];
    *ds = v.ss[s];
    return;
  }
  AxisTaps t[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double c = (double)oc[a] * p[8 + a];
    c = c + p[11 + a];
    t[a] = axis_taps(c, v.dims[a], boundary::REFLECT);
  }
  long long rows[2][2], col[2], s0;
  tap_offsets(v, t, rows, col, s0);
  double acc[1];
  trilinear<1>(v.si, v.V, rows, col, t[0].w, t[1].w, t[2].w, acc);
  *di = (float)acc[0];
  *ds = v.ss[s0];
}

// ---- rotating affine + intensity ------------------------------------------------------------------------------------
// params (N, AFFINE_STRIDE) f64 per sample (resample.hpp).  With the affine on, output voxel o samples the permuted volume
// at M o + offset, then the row's boundary map, then order 1 (image) / order 0 (mask).
// Every thread gathers its own eight corners straight from global memory: under the +-15 degree rotations of the
// recipe a wave's 64 outputs stay within a few source rows, which L2 serves.
__global__ __launch_bounds__(DP_THREADS) void affine_kernel(
    const float* __restrict__ src_img, const unsigned char* __restrict__ src_seg, int n_src,
    const double* __restrict__ params, int D, int H, int W, float* __restrict__ dst_img,
    unsigned char* __restrict__ dst_seg) {
  const long long V = (long long)D * H * W;
  const long long o = (long long)blockIdx.x * DP_THREADS + threadIdx.x;
  if (o >= V) return;
  const int n = blockIdx.y;
  const double* p = params + (size_t)n * AFFINE_STRIDE;
  float* di = dst_img + (long long)n * V + o;
  unsigned char* ds = dst_seg + (long long)n * V + o;
  const SrcView<unsigned char> v = view_fixed(src_img, src_seg, n_src, p, D, H, W);
  if (!v.ok) {
    *di = 0.0f;
    *ds = 0;
    return;
  }
  const int oc[3] = {(int)(o / ((long long)H * W)), (int)((o / W) % H), (int)(o % W)};
  if (p[7] == 0.0) {  // permuted copy, the intensity arithmetic in the store
    const long long s = v.base + oc[0] * v.pst[0] + oc[1] * v.pst[1] + oc[2] * v.pst[2];
    *di = apply_ops(v.si[s], p);
    *ds = v.ss[s];
    return;
  }
  const int mode = row_boundary(p);
  AxisTaps t[3];
#pragma unroll
  for (int h = 0; h < 3; ++h) t[h] = axis_taps(affine_coord(p, oc, h), v.dims[h], mode);
  if (t[0].outside || t[1].outside || t[2].outside) {  // scipy's constant: cval for image and mask alike, the
    *di = apply_ops(0.0f, p);                           // intensity operations still apply
    *ds = 0;
    return;
  }
  long long rows[2][2], col[2], s0;
  tap_offsets(v, t, rows, col, s0);
  double acc[1];
  trilinear<1>(v.si, v.V, rows, col, t[0].w, t[1].w, t[2].w, acc);
  *di = apply_ops((float)acc[0], p);
  *ds = v.ss[s0];
}

// ---- connected components -> boxes ----------------------------------------------------------------------------------
__device__ __forceinline__ int ld_link(const int* L, int i) {
  return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int find_root(const int* L, int x) {
  int p = ld_link(L, x);
  while (p != x) {
    x = p;
    p = ld_link(L, x);
  }
  return x;
}

__device__ void unite(int* L, int a, int b) {
  for (;;) {
    a = find_root(L, a);
    b = find_root(L, b);
    if (a == b) return;
    if (a < b) {
      const int old = atomicMin(L + b, a);
      if (old == b) return;
      b = old;
    } else {
      const int old = atomicMin(L + a, b);
      if (old == a) return;
      a = old;
    }
  }
}

__device__ __forceinline__ bool is_fg(unsigned v, int ncls) { return v >= 1u && v <= (unsigned)ncls; }

// links, component records (min z, y, x = INT_MAX, max = -1, class), header
__global__ __launch_bounds__(DP_THREADS) void cc_init_kernel(const unsigned char* __restrict__ seg, long long total,
                                                             int ncls, int* __restrict__ L, int* __restrict__ comp,
                                                             long long comp_words, int* __restrict__ hdr) {
  const long long stride = (long long)gridDim.x * DP_THREADS;
  for (long long i = (long long)blockIdx.x * DP_THREADS + threadIdx.x; i < total; i += stride)
    L[i] = is_fg(seg[i], ncls) ? (int)i : BG;
  for (long long i = (long long)blockIdx.x * DP_THREADS + threadIdx.x; i < comp_words; i += stride)
    comp[i] = (i & 7) < 3 ? 0x7FFFFFFF : -1;
  if (blockIdx.x == 0 && threadIdx.x < 4) hdr[threadIdx.x] = 0;
}

// grid (cdiv(V, 256), N): union with the -x, -y, -z neighbours of the same class
__global__ __launch_bounds__(DP_THREADS) void cc_merge_kernel(const unsigned char* __restrict__ seg, int D, int H, int W,
                                                              int ncls, int* __restrict__ L) {
  const long long V = (long long)D * H * W;
  const long long o = (long long)blockIdx.x * DP_THREADS + threadIdx.x;
  if (o >= V) return;
  const long long i = (long long)blockIdx.y * V + o;
  const unsigned v = seg[i];
  if (!is_fg(v, ncls)) return;
  const int x = (int)(o % W), y = (int)((o / W) % H), z = (int)(o / ((long long)H * W));
  if (x > 0 && seg[i - 1] == v) unite(L, (int)i, (int)(i - 1));
  if (y > 0 && seg[i - W] == v) unite(L, (int)i, (int)(i - W));
  if (z > 0 && seg[i - (long long)H * W] == v) unite(L, (int)i, (int)(i - (long long)H * W));
}

// grid (ntile, N): roots per class in each tile -> cnt[(n * ncls + c - 1) * ntile + tile]
__global__ __launch_bounds__(DP_THREADS) void cc_count_kernel(const unsigned char* __restrict__ seg,
                                                              const int* __restrict__ L, long long V, int ncls,
                                                              int ntile, int* __restrict__ cnt) {
  __shared__ int sc[CC_MAX_CLASSES];
  if (threadIdx.x < CC_MAX_CLASSES) sc[threadIdx.x] = 0;
  __syncthreads();
  const long long img = (long long)blockIdx.y * V;
  const long long t0 = (long long)blockIdx.x * CC_TILE;
  for (int k = threadIdx.x; k < CC_TILE; k += DP_THREADS) {
    const long long o = t0 + k;
    if (o < V && L[img + o] == (int)(img + o)) atomicAdd(&sc[seg[img + o] - 1], 1);  // integer: order-free
  }
  __syncthreads();
  if ((int)threadIdx.x < ncls) cnt[((long long)blockIdx.y * ncls + threadIdx.x) * ntile + blockIdx.x] = sc[threadIdx.x];
}

__device__ __forceinline__ int block_excl_scan(int v, int* lds, int* total) {  // SCAN_THREADS == FIN_THREADS lanes
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(inc, d, 64);
    if (lane >= d) inc += u;
  }
  if (lane == 63) lds[w] = inc;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) {
      const int s = lds[k];
      lds[k] = run;
      run += s;
    }
    lds[32] = run;
  }
  __syncthreads();
  const int r = lds[w] + inc - v;
  *total = lds[32];
  __syncthreads();
  return r;
}

// one workgroup: exclusive offsets of every (image, class, tile) count in that order; seg_off[s] = first rank of
// segment s = n * ncls + c - 1, seg_off[N * ncls] = number of components
__global__ __launch_bounds__(SCAN_THREADS) void cc_scan_kernel(const int* __restrict__ cnt, int nseg, int ntile,
                                                               int* __restrict__ off, int* __restrict__ seg_off) {
  __shared__ int lds[33];
  const int n = nseg * ntile;
  int carry = 0;
  for (int b = 0; b < n; b += SCAN_THREADS) {
    const int i = b + threadIdx.x;
    const int v = i < n ? cnt[i] : 0;
    int tot;
    const int e = block_excl_scan(v, lds, &tot);
    if (i < n) {
      off[i] = carry + e;
      if (i % ntile == 0) seg_off[i / ntile] = carry + e;
    }
    carry += tot;
  }
  if (threadIdx.x == 0) seg_off[nseg] = carry;
}

// grid (ntile, N): rank of every root (raster order within its (image, class) segment) into the link array; each
// thread owns CC_PER_THREAD consecutive voxels of the tile
__global__ __launch_bounds__(DP_THREADS) void cc_rank_kernel(const unsigned char* __restrict__ seg,
                                                             int* __restrict__ L, long long V, int ncls, int ntile,
                                                             const int* __restrict__ off, int comp_cap,
                                                             int* __restrict__ comp, int* __restrict__ hdr) {
  __shared__ int scan[CC_MAX_CLASSES][DP_THREADS + 1];
  const long long img = (long long)blockIdx.y * V;
  const long long o0 = (long long)blockIdx.x * CC_TILE + (long long)threadIdx.x * CC_PER_THREAD;
  int mine[CC_MAX_CLASSES];
#pragma unroll
  for (int c = 0; c < CC_MAX_CLASSES; ++c) mine[c] = 0;
  for (int k = 0; k < CC_PER_THREAD; ++k) {
    const long long o = o0 + k;
    if (o < V && L[img + o] == (int)(img + o)) {
      const int c = seg[img + o] - 1;
#pragma unroll
      for (int q = 0; q < CC_MAX_CLASSES; ++q) mine[q] += (q == c);
    }
  }
  for (int c = 0; c < ncls; ++c) scan[c][threadIdx.x + 1] = mine[c];
  if (threadIdx.x < CC_MAX_CLASSES) scan[threadIdx.x][0] = 0;
  __syncthreads();
  if ((int)threadIdx.x < ncls) {  // serial prefix per class: 256 adds
    int* row = scan[threadIdx.x];
    for (int k = 1; k <= DP_THREADS; ++k) row[k] += row[k - 1];
  }
  __syncthreads();
  int next[CC_MAX_CLASSES];
  for (int c = 0; c < ncls; ++c)
    next[c] = off[((long long)blockIdx.y * ncls + c) * ntile + blockIdx.x] + scan[c][threadIdx.x];
  for (int k = 0; k < CC_PER_THREAD; ++k) {
    const long long o = o0 + k;
    if (o < V && L[img + o] == (int)(img + o)) {
      const int c = seg[img + o] - 1;
      int r = 0;
      for (int q = 0; q < ncls; ++q)
        if (q == c) r = next[q]++;
      L[img + o] = -(r + 2);
      if (r < comp_cap) comp[(long long)r * 8 + 6] = c + 1;
      else atomicOr(&hdr[0], 2);
    }
  }
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
  return v;
}

// grid-stride over N * V: integer extents of every component (a wave whose voxels all lie in one component folds them
// first: one set of atomics instead of 64)
__global__ __launch_bounds__(DP_THREADS) void cc_box_kernel(const int* __restrict__ L, int N, int D, int H, int W,
                                                            int comp_cap, int* __restrict__ comp) {
  const long long V = (long long)D * H * W, total = (long long)N * V;
  const long long stride = (long long)gridDim.x * DP_THREADS;
  const long long start = (long long)blockIdx.x * DP_THREADS + threadIdx.x;
  const long long iters = (total + stride - 1) / stride;  // the same for every lane: the wave stays converged
  for (long long it = 0; it < iters; ++it) {
    const long long i = start + it * stride;
    int r = -1, z = 0, y = 0, x = 0;
    if (i < total) {
      int p = L[i];
      if (p != BG) {
        long long q = i;
        while (p >= 0) {
          q = p;
          p = L[q];
        }
        r = -p - 2;
        if (r >= comp_cap) r = -1;
        const long long o = i % V;
        x = (int)(o % W);
        y = (int)((o / W) % H);
        z = (int)(o / ((long long)H * W));
      }
    }
    const unsigned long long act = __ballot(r >= 0);
    if (act == 0) continue;
    const int r0 = __shfl(r, __ffsll((long long)act) - 1, 64);
    if (__all(r < 0 || r == r0)) {
      const bool a = r >= 0;
      const int mz = wave_min(a ? z : 0x7FFFFFFF), my = wave_min(a ? y : 0x7FFFFFFF), mx = wave_min(a ? x : 0x7FFFFFFF);
      const int Mz = wave_max(a ? z : -1), My = wave_max(a ? y : -1), Mx = wave_max(a ? x : -1);
      if ((threadIdx.x & 63) == 0) {
        int* b = comp + (long long)r0 * 8;
        atomicMin(b + 0, mz); atomicMin(b + 1, my); atomicMin(b + 2, mx);
        atomicMax(b + 3, Mz); atomicMax(b + 4, My); atomicMax(b + 5, Mx);
      }
    } else if (r >= 0) {
      int* b = comp + (long long)r * 8;
      atomicMin(b + 0, z); atomicMin(b + 1, y); atomicMin(b + 2, x);
      atomicMax(b + 3, z); atomicMax(b + 4, y); atomicMax(b + 5, x);
    }
  }
}

// one workgroup: drop flat components, write kept ones in rank order as packed targets; obj_off from the segment starts
__global__ __launch_bounds__(FIN_THREADS) void cc_final_kernel(const int* __restrict__ comp,
                                                               const int* __restrict__ seg_off, int N, int ncls, int D,
                                                               int H, int W, int comp_cap, int capacity,
                                                               int* __restrict__ kept, float* __restrict__ boxes,
                                                               long long* __restrict__ labels, int* __restrict__ obj_off,
                                                               int* __restrict__ hdr, int* __restrict__ overflow) {
  __shared__ int lds[33];
  const int total = seg_off[N * ncls];
  const int nc = total < comp_cap ? total : comp_cap;
  const float size[3] = {(float)D, (float)H, (float)W};
  int carry = 0;
  for (int b = 0; b < nc; b += FIN_THREADS) {
    const int k = b + threadIdx.x;
    int keep = 0;
    int e[7];
    if (k < nc) {
#pragma unroll
      for (int j = 0; j < 7; ++j) e[j] = comp[(long long)k * 8 + j];
      keep = e[3] > e[0] && e[4] > e[1] && e[5] > e[2];
    }
    int tot;
    const int row = carry + block_excl_scan(keep, lds, &tot);
    if (k < nc) {
      kept[k] = row;
      if (keep && row < capacity) {
#pragma unroll
        for (int j = 0; j < 6; ++j) boxes[(long long)row * 6 + j] = __fdiv_rn((float)e[j], size[j % 3]);
        labels[row] = e[6];
      }
    }
    carry += tot;
  }
  if (threadIdx.x == 0) kept[nc] = carry;
  __syncthreads();
  for (int n = threadIdx.x; n <= N; n += FIN_THREADS) {
    int s = n < N ? seg_off[n * ncls] : total;
    if (s > nc) s = nc;
    const int v = kept[s];
    obj_off[n] = v < capacity ? v : capacity;  // in bounds even on overflow (the flag says it happened)
  }
  if (threadIdx.x == 0) {
    const int f = hdr[0] | (carry > capacity ? 1 : 0);
    hdr[1] = carry;
    *overflow = f;
  }
}

struct CcPlan {
  size_t links, cnt, off, seg_off, comp, kept, hdr, total;
  int ntile;
};

CcPlan cc_plan(int N, int D, int H, int W, int ncls, int comp_cap) {
  CcPlan p;
  const long long V = (long long)D * H * W;
  p.ntile = (int)((V + CC_TILE - 1) / CC_TILE);
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  size_t at = 0;
  p.links = at; at += up((size_t)N * V * 4);
  p.cnt = at; at += up((size_t)N * ncls * p.ntile * 4);
  p.off = at; at += up((size_t)N * ncls * p.ntile * 4);
  p.seg_off = at; at += up(((size_t)N * ncls + 1) * 4);
  p.comp = at; at += up((size_t)comp_cap * 8 * 4);
  p.kept = at; at += up(((size_t)comp_cap + 1) * 4);
  p.hdr = at; at += 256;
  p.total = at;
  return p;
}

bool cc_supported(int N, int D, int H, int W, int ncls, int comp_cap) {
  return N > 0 && D > 0 && H > 0 && W > 0 && ncls >= 1 && ncls <= CC_MAX_CLASSES && comp_cap > 0 &&
         (long long)N * D * H * W < 0x7FFFFFF0LL && (long long)comp_cap * 8 < 0x7FFFFFF0LL;
}

int grid_for(long long n) {
  const long long g = (n + DP_THREADS - 1) / DP_THREADS;
  return (int)(g < 2048 ? (g > 0 ? g : 1) : 2048);
}

}  // namespace

extern "C" {

int msl_normalize_nonzero(float* img, int n_volumes, long long voxels, void* stream) {
  if (!img || n_volumes < 0 || voxels <= 0) return MSL_ERR_ARG;
  if (n_volumes == 0) return MSL_OK;
  MSL_LAUNCH(normalize_kernel, dim3(n_volumes), dim3(NORM_THREADS), 0, (hipStream_t)stream, img, voxels);
  MSL_LAUNCH_CHECK();
  return MSL_OK;
}

int msl_augment_resample(const float* src_img, const unsigned char* src_seg, int n_src, const double* params, int N,
                         int D, int H, int W, float* dst_img, unsigned char* dst_seg, void* stream) {
  if (!src_img || !src_seg || !params || !dst_img || !dst_seg || N <= 0 || n_src <= 0 || D <= 0 || H <= 0 || W <= 0)
    return MSL_ERR_ARG;
  if (N > 65535 || (long long)D * H * W >= (1LL << 40)) return MSL_ERR_UNSUPPORTED;
  const long long V = (long long)D * H * W;
  MSL_LAUNCH(resample_kernel, dim3((unsigned)((V + DP_THREADS - 1) / DP_THREADS), N), dim3(DP_THREADS), 0,
             (hipStream_t)stream, src_img, src_seg, n_src, params, D, H, W, dst_img, dst_seg);
  MSL_LAUNCH_CHECK();
  return MSL_OK;
}

int msl_augment_affine(const float* src_img, const unsigned char* src_seg, int n_src, const double* params, int N,
                       int D, int H, int W, float* dst_img, unsigned char* dst_seg, void* stream) {
  if (!src_img || !src_seg || !params || !dst_img || !dst_seg || N <= 0 || n_src <= 0 || D <= 0 || H <= 0 || W <= 0)
    return MSL_ERR_ARG;
  if (N > 65535 || (long long)D * H * W >= (1LL << 40)) return MSL_ERR_UNSUPPORTED;
  const long long V = (long long)D * H * W;
  MSL_LAUNCH(affine_kernel, dim3((unsigned)((V + DP_THREADS - 1) / DP_THREADS), N), dim3(DP_THREADS), 0,
             (hipStream_t)stream, src_img, src_seg, n_src, params, D, H, W, dst_img, dst_seg);
  MSL_LAUNCH_CHECK();
  return MSL_OK;
}

size_t msl_seg_boxes_workspace_bytes(int N, int D, int H, int W, int n_classes, int comp_cap) {
  if (!cc_supported(N, D, H, W, n_classes, comp_cap)) return 0;
  return cc_plan(N, D, H, W, n_classes, comp_cap).total;
}

int msl_seg_boxes(const unsigned char* seg, int N, int D, int H, int W, int n_classes, int capacity, int comp_cap,
                  void* workspace, size_t workspace_bytes, float* boxes, long long* labels, int* obj_off,
                  int* overflow, void* stream) {
  if (!seg || !workspace || !boxes || !labels || !obj_off || !overflow || capacity < 0) return MSL_ERR_ARG;
  if (!cc_supported(N, D, H, W, n_classes, comp_cap) || N > 65535) return MSL_ERR_UNSUPPORTED;
  const CcPlan p = cc_plan(N, D, H, W, n_classes, comp_cap);
  if (workspace_bytes < p.total) return MSL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int* L = (int*)(ws + p.links);
  int* cnt = (int*)(ws + p.cnt);
  int* off = (int*)(ws + p.off);
  int* seg_off = (int*)(ws + p.seg_off);
  int* comp = (int*)(ws + p.comp);
  int* kept = (int*)(ws + p.kept);
  int* hdr = (int*)(ws + p.hdr);
  const long long V = (long long)D * H * W, total = (long long)N * V;
  const unsigned vblocks = (unsigned)((V + DP_THREADS - 1) / DP_THREADS);
  MSL_LAUNCH(cc_init_kernel, dim3(grid_for(total > (long long)comp_cap * 8 ? total : (long long)comp_cap * 8)),
             dim3(DP_THREADS), 0, st, seg, total, n_classes, L, comp, (long long)comp_cap * 8, hdr);
  MSL_LAUNCH(cc_merge_kernel, dim3(vblocks, N), dim3(DP_THREADS), 0, st, seg, D, H, W, n_classes, L);
  MSL_LAUNCH(cc_count_kernel, dim3(p.ntile, N), dim3(DP_THREADS), 0, st, seg, (const int*)L, V, n_classes, p.ntile, cnt);
  MSL_LAUNCH(cc_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, (const int*)cnt, N * n_classes, p.ntile, off, seg_off);
  MSL_LAUNCH(cc_rank_kernel, dim3(p.ntile, N), dim3(DP_THREADS), 0, st, seg, L, V, n_classes, p.ntile,
             (const int*)off, comp_cap, comp, hdr);
  MSL_LAUNCH(cc_box_kernel, dim3(grid_for(total)), dim3(DP_THREADS), 0, st, (const int*)L, N, D, H, W, comp_cap, comp);
  MSL_LAUNCH(cc_final_kernel, dim3(1), dim3(FIN_THREADS), 0, st, (const int*)comp, (const int*)seg_off, N, n_classes,
             D, H, W, comp_cap, capacity, kept, boxes, labels, obj_off, hdr, overflow);
  MSL_LAUNCH_CHECK();
  return MSL_OK;
}

}  // extern "C"

// ---- clinical cases of C sequences (1 <= C <= 4): foreground box, ragged augment + fit / window, instance boxes ---------
// Host mirrors: datasets.foreground_box on a (D, H, W) or channel-first (C, D, H, W) image, datasets._LesionCases
// .__getitem__ with len(input_images) = C (augmentations at the cropped shape, then resize_with_pad_or_crop with edge
// replication) and datasets.boxes_from_instances.  The mask arena and the table are the same for every C; the image arena
// holds C contiguous planes per case, case k at element C * off_k.  There is one kernel of each kind: the one-channel
// entry points (msl_foreground_box, msl_augment_fit) are its C = 1 launch.
//
//   foreground : one wave per row of the C * D * H rows; the w extents stay in the lanes, the d / h extents are
//                wave-uniform; a row of any channel that holds a positive voxel extends the one box (the union of the
//                channels' supports); six integer atomics per wave, then one thread applies margin, clamp and the empty
//                rule
//   fit        : one thread per four output voxels along the last axis, for all C channels; the fit is a clamped shift
//                per axis, the permutation / affine / intensity arithmetic is affine_kernel's.  The clamp of the fit, the
//                f64 coordinate row, the boundary maps, the axis weights and the order-0 mask tap are computed once per
//                voxel; only the eight gathers, the f64 accumulation and the intensity operations repeat per channel,
//                each in the same operation order (a channel is bit-identical to a C = 1 launch on its plane); every
//                plane of the image stored as one 16-byte vector
//   window     : the same body (WIN) with the shift d read per sample from `windows` instead of centred: a training patch
//                or a validation tile (datasets.window).  With the affine off, a thread whose four
//                sources are one in-range run of an unreversed last axis reads them with one 16-byte load per plane and
//                one 8-byte load of the mask where those addresses are aligned (views.hip's rule) - a patch inside a
//                large head is that case nearly everywhere
//   instances  : one 16-byte load per eight voxels, nothing else while they are all background; runs of one id are
//                folded in registers before the integer min / max atomics into a per-image (32768, 6) extent table;
//                one workgroup compacts it in (image, threshold pair, ascending id) order by a fixed-order scan
namespace {

constexpr int FG_THREADS = 256;
constexpr int FIT_VEC = STORE_VEC;    // output voxels per thread
constexpr int FIT_MAX_CH = 4;         // the stem's limit
constexpr int INST_IDS = 32768;       // ids 1 .. 32767 (int16)
constexpr int INST_VEC = 8;           // voxels per 16-byte load
constexpr int INST_UNROLL = 4;        // loads in flight per thread
constexpr int INST_MAX_PAIRS = 8;
constexpr int INST_HDR = 4;           // ints per image: smallest id, largest id, background seen, unused
constexpr int IMAX = 0x7FFFFFFF;

__global__ void fg_init_kernel(int* __restrict__ box) {
  if (threadIdx.x < 6) box[threadIdx.x] = threadIdx.x < 3 ? IMAX : -1;
}

__global__ __launch_bounds__(FG_THREADS) void fg_reduce_kernel(const float* __restrict__ vol, int C, int D, int H, int W,
                                                               int* __restrict__ box) {
  const int lane = threadIdx.x & 63;
  const long long rows = (long long)C * D * H;
  const long long nwave = (long long)gridDim.x * (FG_THREADS / 64);
  int lo_d = IMAX, lo_h = IMAX, lo_w = IMAX, hi_d = -1, hi_h = -1, hi_w = -1;
  for (long long r = (long long)blockIdx.x * (FG_THREADS / 64) + (threadIdx.x >> 6); r < rows; r += nwave) {
    const float* row = vol + r * W;
    bool any = false;
    for (int w = lane; w < W; w += 64) {
      if (row[w] > 0.0f) {
        any = true;
        lo_w = min(lo_w, w);
        hi_w = max(hi_w, w);
      }
    }
    if (__any(any)) {  // wave-uniform
      long long cd = r / H;  // c * D + d with c < C <= FIT_MAX_CH: d by subtraction, not a second 64-bit division
      while (cd >= D) cd -= D;
      const int d = (int)cd, h = (int)(r % H);
      lo_d = min(lo_d, d); hi_d = max(hi_d, d);
      lo_h = min(lo_h, h); hi_h = max(hi_h, h);
    }
  }
  lo_w = wave_min(lo_w);
  hi_w = wave_max(hi_w);
  if (lane == 0 && hi_d >= 0) {
    atomicMin(box + 0, lo_d); atomicMin(box + 1, lo_h); atomicMin(box + 2, lo_w);
    atomicMax(box + 3, hi_d); atomicMax(box + 4, hi_h); atomicMax(box + 5, hi_w);
  }
}

__global__ void fg_final_kernel(int D, int H, int W, int margin, int* __restrict__ box) {
  if (threadIdx.x != 0) return;
  const int n[3] = {D, H, W};
  if (box[3] < 0) {  // no foreground: the whole volume
    for (int a = 0; a < 3; ++a) {
      box[a] = 0;
      box[3 + a] = n[a];
    }
    return;
  }
  for (int a = 0; a < 3; ++a) {
    const long long lo = (long long)box[a] - margin, hi = (long long)box[3 + a] + margin + 1;
    box[a] = lo < 0 ? 0 : (lo > n[a] ? n[a] : (int)lo);
    box[3 + a] = hi > n[a] ? n[a] : (hi < 0 ? 0 : (int)hi);
  }
}

// the three launches of a foreground box over the C * D * H rows of a channel-first volume
int foreground_box(const float* vol, int C, int D, int H, int W, int margin, int* box, void* stream) {
  if (!vol || !box || C < 1 || C > FIT_MAX_CH || D <= 0 || H <= 0 || W <= 0 || margin < 0) return MSL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const long long waves = ((long long)C * D * H + 3) / 4;
  MSL_LAUNCH(fg_init_kernel, dim3(1), dim3(64), 0, st, box);
  // the six atomics of every wave hit the same six words: few waves, many rows each
  MSL_LAUNCH(fg_reduce_kernel, dim3((unsigned)(waves < 512 ? waves : 512)), dim3(FG_THREADS), 0, st, vol, C, D, H, W, box);
  MSL_LAUNCH(fg_final_kernel, dim3(1), dim3(64), 0, st, D, H, W, margin, box);
  MSL_LAUNCH_CHECK();
  return MSL_OK;
}

// source index of output index o under the shift d on an axis of n voxels.  The fit's d is bounded by the sizes; a window's
// origin is any int (far outside the case it repeats the border voxel), so that sum is formed in 64 bits
template <bool WIN>
__device__ __forceinline__ int fit_src(int o, int d, int n) {
  if (!WIN) return min(max(o + d, 0), n - 1);
  const long long q = (long long)o + d;
  return q < 0 ? 0 : (q > n - 1 ? n - 1 : (int)q);
}

// Arenas and table: view_arena's (resample.hpp); params: msl_augment_affine's rows with [0] = case.  Output voxel o of the
// (T0, T1, T2) target reads voxel q of the permuted case (shape n'), q_a = clamp(o_a + d_a, 0, n'_a - 1) with the shift d
// of fit_shift (WIN: d_a = windows[n][a]); with the affine on, the permuted case is sampled at M q + offset as
// affine_kernel samples it.
template <int C, bool VEC, bool WIN>
__global__ __launch_bounds__(DP_THREADS) void fit_kernel(
    const float* __restrict__ src_img, const short* __restrict__ src_seg, long long seg_elems,
    const long long* __restrict__ table, int n_cases, const double* __restrict__ params,
    const int* __restrict__ windows, int T0, int T1, int T2, float* __restrict__ dst_img, short* __restrict__ dst_seg) {
  const int G = (T2 + FIT_VEC - 1) / FIT_VEC;
  const long long groups = (long long)T0 * T1 * G;
  const long long g = (long long)blockIdx.x * DP_THREADS + threadIdx.x;
  if (g >= groups) return;
  const int n = blockIdx.y;
  const int x0 = (int)(g % G) * FIT_VEC;
  const long long rowi = g / G;
  const int oc0 = (int)(rowi / T1), oc1 = (int)(rowi % T1);
  const long long TV = (long long)T0 * T1 * T2;
  const long long in_plane = ((long long)oc0 * T1 + oc1) * T2 + x0;
  const int cnt = (T2 - x0) < FIT_VEC ? (T2 - x0) : FIT_VEC;
  const double* p = params + (size_t)n * AFFINE_STRIDE;
  float vi[C][FIT_VEC];
  short vs[FIT_VEC];
#pragma unroll
  for (int j = 0; j < FIT_VEC; ++j) {
#pragma unroll
    for (int c = 0; c < C; ++c) vi[c][j] = 0.0f;
    vs[j] = 0;
  }
  const SrcView<short> v = view_arena<C>(src_img, src_seg, seg_elems, table, n_cases, p);
  if (v.ok) {
    const int T[3] = {T0, T1, T2};
    int dsh[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) dsh[a] = fit_shift(WIN ? windows + 3 * (long long)n + a : nullptr, v.dims[a], T[a]);
    const int q0 = fit_src<WIN>(oc0, dsh[0], v.dims[0]), q1 = fit_src<WIN>(oc1, dsh[1], v.dims[1]);
    const bool affine = p[7] != 0.0;
    const int mode = row_boundary(p);
    int qprev = -1;
    int jn = cnt;  // voxels the loop below still has to fill
    const long long xs = (long long)x0 + dsh[2];  // source of the thread's first voxel, before the clamp
    if (WIN && !affine && cnt == FIT_VEC && v.pst[2] == 1 && xs >= 0 && xs + FIT_VEC <= v.dims[2]) {
      // interior run: sources s .. s + 3 of one row of the case, the values the loop would read one by one
      const long long s = v.base + q0 * v.pst[0] + q1 * v.pst[1] + xs;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float* sp = v.si + c * v.V + s;
        float4 x;
        if (((uintptr_t)sp & 15u) == 0) {
          x = *reinterpret_cast<const float4*>(sp);
        } else {
          x = make_float4(sp[0], sp[1], sp[2], sp[3]);
        }
        vi[c][0] = apply_ops(x.x, p);
        vi[c][1] = apply_ops(x.y, p);
        vi[c][2] = apply_ops(x.z, p);
        vi[c][3] = apply_ops(x.w, p);
      }
      const short* mp = v.ss + s;
      if (((uintptr_t)mp & 7u) == 0) {
        typedef short short4v __attribute__((ext_vector_type(4)));
        const short4v m = *reinterpret_cast<const short4v*>(mp);
        vs[0] = m[0]; vs[1] = m[1]; vs[2] = m[2]; vs[3] = m[3];
      } else {
        vs[0] = mp[0]; vs[1] = mp[1]; vs[2] = mp[2]; vs[3] = mp[3];
      }
      jn = 0;
    }
    for (int j = 0; j < jn; ++j) {
      const int qc[3] = {q0, q1, fit_src<WIN>(x0 + j, dsh[2], v.dims[2])};
      if (j > 0 && qc[2] == qprev) {  // padded region along the last axis: the same source voxel, the same values
#pragma unroll
        for (int c = 0; c < C; ++c) vi[c][j] = vi[c][j - 1];
        vs[j] = vs[j - 1];
        continue;
      }
      qprev = qc[2];
      if (!affine) {
        const long long s = v.base + qc[0] * v.pst[0] + qc[1] * v.pst[1] + qc[2] * v.pst[2];
#pragma unroll
        for (int c = 0; c < C; ++c) vi[c][j] = apply_ops(v.si[c * v.V + s], p);
        vs[j] = v.ss[s];
        continue;
      }
      AxisTaps t[3];
#pragma unroll
      for (int h = 0; h < 3; ++h) t[h] = axis_taps(affine_coord(p, qc, h), v.dims[h], mode);
      if (t[0].outside || t[1].outside || t[2].outside) {  // scipy's constant: cval for image and mask alike, the
        const float cval = apply_ops(0.0f, p);              // intensity operations still apply
#pragma unroll
        for (int c = 0; c < C; ++c) vi[c][j] = cval;
        vs[j] = 0;
        continue;
      }
      long long rows[2][2], col[2], s0;
      tap_offsets(v, t, rows, col, s0);
      double acc[C];
      trilinear<C>(v.si, v.V, rows, col, t[0].w, t[1].w, t[2].w, acc);
#pragma unroll
      for (int c = 0; c < C; ++c) vi[c][j] = apply_ops((float)acc[c], p);
      vs[j] = v.ss[s0];
    }
  }
  // VEC: T2 % 4 == 0, so every group is whole
  store_group<C, VEC>(vi, vs, cnt, dst_img + (long long)n * C * TV + in_plane, TV, dst_seg + (long long)n * TV + in_plane);
}

template <int C, bool WIN>
void launch_fit(bool vec, dim3 grid, hipStream_t st, const float* arena_img, const short* arena_seg, long long seg_elems,
                const long long* table, int n_cases, const double* params, const int* windows, int T0, int T1, int T2,
                float* dst_img, short* dst_seg) {
  if (vec)
    MSL_LAUNCH(fit_kernel<C, true, WIN>, grid, dim3(DP_THREADS), 0, st, arena_img, arena_seg, seg_elems, table, n_cases,
               params, windows, T0, T1, T2, dst_img, dst_seg);
  else
    MSL_LAUNCH(fit_kernel<C, false, WIN>, grid, dim3(DP_THREADS), 0, st, arena_img, arena_seg, seg_elems, table, n_cases,
               params, windows, T0, T1, T2, dst_img, dst_seg);
}

// the launch of msl_augment_fit[_mc] (windows null: the centred fit) and msl_augment_window_mc
template <bool WIN>
int augment_mc(const float* arena_img, const short* arena_seg, long long seg_elems, int C, const long long* table,
               int n_cases, const double* params, const int* windows, int N, int T0, int T1, int T2, float* dst_img,
               short* dst_seg, void* stream) {
  if (!arena_img || !arena_seg || !table || !params || !dst_img || !dst_seg || seg_elems <= 0 || C < 1 ||
      C > FIT_MAX_CH || n_cases <= 0 || N <= 0 || T0 <= 0 || T1 <= 0 || T2 <= 0)
    return MSL_ERR_ARG;
  const long long groups = (long long)T0 * T1 * ((T2 + FIT_VEC - 1) / FIT_VEC);
  if (N > 65535 || (groups + DP_THREADS - 1) / DP_THREADS > 0x7FFFFFFFLL) return MSL_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)((groups + DP_THREADS - 1) / DP_THREADS), N);
  const bool vec = T2 % FIT_VEC == 0 && ((uintptr_t)dst_img & 15) == 0 && ((uintptr_t)dst_seg & 7) == 0;
  hipStream_t st = (hipStream_t)stream;
  return msl::dispatch_int<1, 2, 3, 4>(C, [&](auto ch) {
    launch_fit<decltype(ch)::value, WIN>(vec, grid, st, arena_img, arena_seg, seg_elems, table, n_cases, params, windows,
                                         T0, T1, T2, dst_img, dst_seg);
    MSL_LAUNCH_CHECK();
    return MSL_OK;
  });
}

// ---- separable warp (zoom / grid distortion): msl_augment_warp_mc -------------------------------------------------------
// Host mirrors: datasets._aug_zoom / _aug_griddistortion (scipy.ndimage.map_coordinates on np.meshgrid(t0, t1, t2)) and
// devicedata.warp_numpy.  The arenas, the table, the rows and the outputs are fit_kernel's; a row with [7] = 2 carries at
// [8] the element offset of its three coordinate tables in `coords` (n'0 + n'1 + n'2 doubles for the permuted shape n')
// and at [20] the boundary.  Output voxel o reads voxel q = clamp(o + d, 0, n' - 1) of the warped case, which samples the
// permuted case at (t0[q0], t1[q1], t2[q2]): from the coordinate on the core's arithmetic, with boundary 1 taken as
// NEAREST_UNCLAMPED.
//
// One wave per output row, a lane per voxel of it (x = lane, lane + 64, ...): q0, q1, their two table reads, boundary
// maps, tap indices and weights are the same for the whole row, so they are formed from a wave-uniform row index
// (readfirstlane) once per row, as are the four tap-row bases; along the row consecutive lanes read consecutive
// elements of t2 and store consecutive voxels.  A row with [7] = 0 is the permuted copy of fit_kernel (its values, by
// the same index arithmetic), any other row is written as zeros.
constexpr int WARP_WAVES = DP_THREADS / 64;  // output rows per workgroup

// The two rows every one-wave-per-row kernel (warp_kernel, deform_kernel) writes besides its own: zeros for a row the
// entry point rejects, and fit_kernel's permuted copy (its values, by the same index arithmetic) with the intensity
// arithmetic in the store.  di / dsg: the row's first voxel in plane 0 of the image and in the mask.
template <int C>
__device__ __forceinline__ void row_zeros(float* __restrict__ di, short* __restrict__ dsg, long long TV, int T2, int lane) {
  for (int x = lane; x < T2; x += 64) {
#pragma unroll
    for (int c = 0; c < C; ++c) di[c * TV + x] = 0.0f;
    dsg[x] = 0;
  }
}

template <int C>
__device__ __forceinline__ void row_copy(const SrcView<short>& v, const double* __restrict__ p, int q0, int q1, int d2,
                                         float* __restrict__ di, short* __restrict__ dsg, long long TV, int T2, int lane) {
  const long long rbase = v.base + q0 * v.pst[0] + q1 * v.pst[1];
  for (int x = lane; x < T2; x += 64) {
    const long long s = rbase + fit_src<true>(x, d2, v.dims[2]) * v.pst[2];
#pragma unroll
    for (int c = 0; c < C; ++c) di[c * TV + x] = apply_ops(v.si[c * v.V + s], p);
    dsg[x] = v.ss[s];
  }
}

template <int C>
__global__ __launch_bounds__(DP_THREADS) void warp_kernel(
    const float* __restrict__ src_img, const short* __restrict__ src_seg, long long seg_elems,
    const long long* __restrict__ table, int n_cases, const double* __restrict__ params,
    const double* __restrict__ coords, long long coords_len, const int* __restrict__ windows, int T0, int T1, int T2,
    float* __restrict__ dst_img, short* __restrict__ dst_seg) {
  const int lane = threadIdx.x & 63;
  // wave-uniform: everything derived from it alone is computed once per row (T0 * T1 fits an int: checked at launch)
  const int rowi = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * WARP_WAVES + (threadIdx.x >> 6)));
  if ((long long)rowi >= (long long)T0 * T1) return;
  const int n = blockIdx.y;
  const int oc0 = rowi / T1, oc1 = rowi % T1;
  const long long TV = (long long)T0 * T1 * T2;
  float* di = dst_img + (long long)n * C * TV + (long long)rowi * T2;
  short* dsg = dst_seg + (long long)n * TV + (long long)rowi * T2;
  const double* p = params + (size_t)n * AFFINE_STRIDE;
  const SrcView<short> v = view_arena<C>(src_img, src_seg, seg_elems, table, n_cases, p);
  const bool warp = p[7] == 2.0;
  bool ok = v.ok && (warp || p[7] == 0.0);
  long long toff = 0;
  if (ok && warp) {  // the three tables lie inside [0, coords_len): the sizes are below 2^20 each, so the sum is exact
    ok = p[8] >= 0.0 && p[8] <= (double)coords_len;
    if (ok) {
      toff = (long long)p[8];
      ok = toff + v.dims[0] + v.dims[1] + v.dims[2] <= coords_len;
    }
  }
  if (!ok) {
    row_zeros<C>(di, dsg, TV, T2, lane);
    return;
  }
  const int T[3] = {T0, T1, T2};
  int dsh[3];  // windows null: the centred fit's shift
#pragma unroll
  for (int a = 0; a < 3; ++a) dsh[a] = fit_shift(windows ? windows + 3 * (long long)n + a : nullptr, v.dims[a], T[a]);
  const int q0 = fit_src<true>(oc0, dsh[0], v.dims[0]), q1 = fit_src<true>(oc1, dsh[1], v.dims[1]);
  if (!warp) {
    row_copy<C>(v, p, q0, q1, dsh[2], di, dsg, TV, T2, lane);
    return;
  }
  // the row's "nearest" is scipy's own here, not affine_kernel's clamp of the coordinate (resample.hpp, at the codes)
  const int rb = row_boundary(p), mode = rb == boundary::NEAREST ? boundary::NEAREST_UNCLAMPED : rb;
  const double* t0 = coords + toff;
  const double* t1 = t0 + v.dims[0];
  const double* t2 = t1 + v.dims[1];
  const AxisTaps a0 = axis_taps(t0[q0], v.dims[0], mode), a1 = axis_taps(t1[q1], v.dims[1], mode);
  long long r1[2][2];  // the four tap rows of the image, the one of the mask
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) r1[a][b] = v.base + a0.i1[a] * v.pst[0] + a1.i1[b] * v.pst[1];
  const long long r0 = v.base + a0.i0 * v.pst[0] + a1.i0 * v.pst[1];
  const float cval = apply_ops(0.0f, p);  // scipy's constant: cval for image and mask alike, the operations still apply
  for (int x = lane; x < T2; x += 64) {
    const AxisTaps a2 = axis_taps(t2[fit_src<true>(x, dsh[2], v.dims[2])], v.dims[2], mode);
    if (a0.outside || a1.outside || a2.outside) {
#pragma unroll
      for (int c = 0; c < C; ++c) di[c * TV + x] = cval;
      dsg[x] = 0;
      continue;
    }
    const long long col[2] = {a2.i1[0] * v.pst[2], a2.i1[1] * v.pst[2]};
    double acc[C];
    trilinear<C>(v.si, v.V, r1, col, a0.w, a1.w, a2.w, acc);
#pragma unroll
    for (int c = 0; c < C; ++c) di[c * TV + x] = apply_ops((float)acc[c], p);
    dsg[x] = v.ss[r0 + a2.i0 * v.pst[2]];
  }
}

// ---- free-form deformation (elastic3d): msl_augment_deform_mc ------------------------------------------------------------
// Host mirrors: datasets.deform_coords / _aug_elastic3d (scipy.ndimage.map_coordinates at q + d(q)) and
// devicedata.deform_numpy; the contract is DESIGN.md section 4.15.  The arenas, the table, the rows and the outputs are
// warp_kernel's; a row with [7] = 3 carries at [8] the element offset of its lattice P in `lattices` (3 L^3 doubles,
// [m][i0][i1][i2]: component m displaces along axis m of the permuted case), at [9] L (4 .. 16 control points per axis)
// and at [20] the boundary.  Output voxel o reads voxel q = clamp(o + d, 0, n' - 1) of the deformed case, which samples
// the permuted case at q + d(q), d_m(q) the cubic B-spline of P[m]: per axis u = q (L - 3) / (n' - 1), cell, t and the
// four weights of spline_taps, then d_m = sum_k b2[k] * R_m[cell2 + k] with R_m[k2] = sum_j b1[j] * (sum_i b0[i] *
// P[m][cell0 + i][cell1 + j][k2]), every sum from 0.0 upwards, one rounded f64 operation each.
//
// One wave per output row, as warp_kernel.  q0, q1, their cells and weights belong to the row; so do the 3 L <= 48
// values R_m[k2], which lane 16 m + k2 computes (16 multiply-adds) and leaves in its wave's own LDS slot.  Along the row
// a lane forms its axis-2 weights, reads its 12 R values, and samples at the three coordinates through the core.
constexpr int DEFORM_MIN_L = 4, DEFORM_MAX_L = 16;

struct SplineTaps {  // one axis of one voxel: the first of its four control points, their weights
  int cell;
  double b[4];
};

// u = 0.0 on an axis of one voxel.  cell is clamped into [0, L - 4] as a double, so any u reads inside the lattice.
__device__ __forceinline__ SplineTaps spline_taps(int q, int n, int L) {
  SplineTaps r;
  const double u = n > 1 ? ((double)q * (double)(L - 3)) / (double)(n - 1) : 0.0;
  const double uf = floor(u);
  r.cell = !(uf >= 0.0) ? 0 : (uf > (double)(L - 4) ? L - 4 : (int)uf);
  const double t = u - (double)r.cell;  // 1.0 at the last voxel
  const double t2 = t * t, t3 = t2 * t, s = 1.0 - t;
  r.b[0] = ((s * s) * s) / 6.0;
  r.b[1] = (((3.0 * t3) - (6.0 * t2)) + 4.0) / 6.0;
  r.b[2] = ((((-3.0 * t3) + (3.0 * t2)) + (3.0 * t)) + 1.0) / 6.0;
  r.b[3] = t3 / 6.0;
  return r;
}

template <int C>
__global__ __launch_bounds__(DP_THREADS) void deform_kernel(
    const float* __restrict__ src_img, const short* __restrict__ src_seg, long long seg_elems,
    const long long* __restrict__ table, int n_cases, const double* __restrict__ params,
    const double* __restrict__ lattices, long long lattices_len, const int* __restrict__ windows, int T0, int T1, int T2,
    float* __restrict__ dst_img, short* __restrict__ dst_seg) {
  __shared__ double rows_r[WARP_WAVES][3 * DEFORM_MAX_L];  // R_m[k2] at [16 m + k2], one slot per wave
  const int lane = threadIdx.x & 63;
  const int rowi = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * WARP_WAVES + (threadIdx.x >> 6)));
  if ((long long)rowi >= (long long)T0 * T1) return;  // whole wave; the kernel has no workgroup barrier
  const int n = blockIdx.y;
  const int oc0 = rowi / T1, oc1 = rowi % T1;
  const long long TV = (long long)T0 * T1 * T2;
  float* di = dst_img + (long long)n * C * TV + (long long)rowi * T2;
  short* dsg = dst_seg + (long long)n * TV + (long long)rowi * T2;
  const double* p = params + (size_t)n * AFFINE_STRIDE;
  const SrcView<short> v = view_arena<C>(src_img, src_seg, seg_elems, table, n_cases, p);
  const bool deform = p[7] == 3.0;
  bool ok = v.ok && (deform || p[7] == 0.0);
  int L = 0;
  long long loff = 0;
  if (ok && deform) {  // L is one of 4 .. 16 and the 3 L^3 doubles lie inside [0, lattices_len)
    ok = p[9] >= (double)DEFORM_MIN_L && p[9] <= (double)DEFORM_MAX_L && p[8] >= 0.0 && p[8] <= (double)lattices_len;
    if (ok) {
      L = (int)p[9];
      loff = (long long)p[8];
      ok = p[9] == (double)L && loff + 3LL * L * L * L <= lattices_len;
    }
  }
  if (!ok) {
    row_zeros<C>(di, dsg, TV, T2, lane);
    return;
  }
  const int T[3] = {T0, T1, T2};
  int dsh[3];  // windows null: the centred fit's shift
#pragma unroll
  for (int a = 0; a < 3; ++a) dsh[a] = fit_shift(windows ? windows + 3 * (long long)n + a : nullptr, v.dims[a], T[a]);
  const int q0 = fit_src<true>(oc0, dsh[0], v.dims[0]), q1 = fit_src<true>(oc1, dsh[1], v.dims[1]);
  if (!deform) {
    row_copy<C>(v, p, q0, q1, dsh[2], di, dsg, TV, T2, lane);
    return;
  }
  double* R = rows_r[threadIdx.x >> 6];
  {
    const SplineTaps s0 = spline_taps(q0, v.dims[0], L), s1 = spline_taps(q1, v.dims[1], L);
    const int m = lane >> 4, k2 = lane & 15;
    if (m < 3 && k2 < L) {  // cell + 3 <= L - 1 on both axes and k2 <= L - 1: inside the sample's 3 L^3 doubles
      const double* P = lattices + loff + (((long long)m * L + s0.cell) * L + s1.cell) * L + k2;
      double r = 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        double in = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) in = in + s0.b[i] * P[(i * L + j) * L];
        r = r + s1.b[j] * in;
      }
      R[lane] = r;
    }
  }
  __builtin_amdgcn_wave_barrier();  // (a wave's LDS operations execute in order; this only pins the compiler's order)
  // the row's "nearest" is scipy's own, as warp_kernel's
  const int rb = row_boundary(p), mode = rb == boundary::NEAREST ? boundary::NEAREST_UNCLAMPED : rb;
  const float cval = apply_ops(0.0f, p);  // scipy's constant: cval for image and mask alike, the operations still apply
  for (int x = lane; x < T2; x += 64) {
    const int q[3] = {q0, q1, fit_src<true>(x, dsh[2], v.dims[2])};
    const SplineTaps s2 = spline_taps(q[2], v.dims[2], L);
    AxisTaps t[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      double d = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) d = d + s2.b[k] * R[16 * m + s2.cell + k];
      t[m] = axis_taps((double)q[m] + d, v.dims[m], mode);
    }
    if (t[0].outside || t[1].outside || t[2].outside) {
#pragma unroll
      for (int c = 0; c < C; ++c) di[c * TV + x] = cval;
      dsg[x] = 0;
      continue;
    }
    long long r1[2][2], col[2], r0;
    tap_offsets(v, t, r1, col, r0);
    double acc[C];
    trilinear<C>(v.si, v.V, r1, col, t[0].w, t[1].w, t[2].w, acc);
#pragma unroll
    for (int c = 0; c < C; ++c) di[c * TV + x] = apply_ops((float)acc[c], p);
    dsg[x] = v.ss[r0];
  }
}

// The launch of msl_augment_warp_mc / msl_augment_deform_mc, the one-wave-per-row kernels.  kernel_of(ch): the kernel for
// decltype(ch)::value channels; side / side_len: the f64 table that rides with the rows (coordinate tables / lattices).
template <typename KernelOf>
int augment_rows(KernelOf kernel_of, const float* arena_img, const short* arena_seg, long long seg_elems, int C,
                 const long long* table, int n_cases, const double* params, const double* side, long long side_len,
                 const int* windows, int N, int T0, int T1, int T2, float* dst_img, short* dst_seg, void* stream) {
  if (!arena_img || !arena_seg || !table || !params || !side || !dst_img || !dst_seg || seg_elems <= 0 || side_len <= 0 ||
      C < 1 || C > FIT_MAX_CH || n_cases <= 0 || N <= 0 || T0 <= 0 || T1 <= 0 || T2 <= 0)
    return MSL_ERR_ARG;
  const long long rows = (long long)T0 * T1;
  if (N > 65535 || rows > 0x7FFFFFFFLL - WARP_WAVES) return MSL_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)((rows + WARP_WAVES - 1) / WARP_WAVES), N);
  hipStream_t st = (hipStream_t)stream;
  return msl::dispatch_int<1, 2, 3, 4>(C, [&](auto ch) {
    MSL_LAUNCH(kernel_of(ch), grid, dim3(DP_THREADS), 0, st, arena_img, arena_seg, seg_elems, table, n_cases, params, side,
               side_len, windows, T0, T1, T2, dst_img, dst_seg);
    MSL_LAUNCH_CHECK();
    return MSL_OK;
  });
}

struct InstPairs {
  int n;
  int lo[INST_MAX_PAIRS], hi[INST_MAX_PAIRS];
};

__global__ __launch_bounds__(DP_THREADS) void inst_init_kernel(int* __restrict__ ext, long long ext_words,
                                                               int* __restrict__ hdr, int N, int* __restrict__ flags) {
  const long long stride = (long long)gridDim.x * DP_THREADS;
  if (blockIdx.x == 0 && threadIdx.x < 4) flags[threadIdx.x] = 0;
  for (long long i = (long long)blockIdx.x * DP_THREADS + threadIdx.x; i < ext_words; i += stride)
    ext[i] = (i % 6) < 3 ? IMAX : -1;
  for (long long i = (long long)blockIdx.x * DP_THREADS + threadIdx.x; i < (long long)N * INST_HDR; i += stride) {
    const int k = (int)(i % INST_HDR);
    hdr[i] = k == 0 ? IMAX : (k == 1 ? -1 : 0);
  }
}

struct InstRun {  // voxels of one id a thread met in a row of its walk
  int id, e[6];
};

__device__ __forceinline__ void inst_flush(const InstRun& r, int* __restrict__ ext, int* __restrict__ hdr) {
  if (r.id <= 0) return;
  int* b = ext + (long long)r.id * 6;
  atomicMin(b + 0, r.e[0]); atomicMin(b + 1, r.e[1]); atomicMin(b + 2, r.e[2]);
  atomicMax(b + 3, r.e[3]); atomicMax(b + 4, r.e[4]); atomicMax(b + 5, r.e[5]);
  atomicMin(hdr + 0, r.id);
  atomicMax(hdr + 1, r.id);
}

// grid (x, N), grid-stride over the image's chunks of eight voxels.  VEC: V % 8 == 0 and seg 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(DP_THREADS) void inst_extent_kernel(const short* __restrict__ seg, int V, int H, int W,
                                                                 int* __restrict__ ext_all, int* __restrict__ hdr_all,
                                                                 int* __restrict__ flags) {
  typedef short short8v __attribute__((ext_vector_type(8)));
  const int n = blockIdx.y;
  const short* s = seg + (long long)n * V;
  int* ext = ext_all + (long long)n * INST_IDS * 6;
  int* hdr = hdr_all + n * INST_HDR;
  const int chunks = (V + INST_VEC - 1) / INST_VEC;
  InstRun run;
  run.id = 0;
  bool zero = false, bad = false;
  const int stride = gridDim.x * DP_THREADS;
  for (int c0 = blockIdx.x * DP_THREADS + threadIdx.x; c0 < chunks; c0 += INST_UNROLL * stride) {
    short8v xs[INST_UNROLL];
    if (VEC) {  // the loads of a round leave back to back, on clamped (always valid) chunks
#pragma unroll
      for (int u = 0; u < INST_UNROLL; ++u) {
        const long long cu = (long long)c0 + (long long)u * stride;
        xs[u] = *reinterpret_cast<const short8v*>(s + (cu < chunks ? cu : (long long)c0) * INST_VEC);
      }
    }
#pragma unroll
    for (int u = 0; u < INST_UNROLL; ++u) {
      const long long cu = (long long)c0 + (long long)u * stride;
      if (cu >= chunks) break;
      const int o0 = (int)cu * INST_VEC;
      short v[INST_VEC];
      if (VEC) {
#pragma unroll
        for (int j = 0; j < INST_VEC; ++j) v[j] = xs[u][j];
      } else {
#pragma unroll
        for (int j = 0; j < INST_VEC; ++j) v[j] = o0 + j < V ? s[o0 + j] : (short)-1;  // -1 past the end: skipped below
      }
      int any = 0;
#pragma unroll
      for (int j = 0; j < INST_VEC; ++j) {
        any |= v[j];
        zero = zero || v[j] == 0;
      }
      if (any == 0) continue;  // background: one read and nothing else
#pragma unroll 1
      for (int j = 0; j < INST_VEC; ++j) {
        const int id = v[j];
        if (id == 0) continue;
        if (id < 0) {
          bad = bad || (o0 + j < V);
          continue;
        }
        const int o = o0 + j;
        const int x = o % W, y = (o / W) % H, z = o / (W * H);
        if (id != run.id) {
          inst_flush(run, ext, hdr);
          run.id = id;
          run.e[0] = run.e[3] = z; run.e[1] = run.e[4] = y; run.e[2] = run.e[5] = x;
        } else {
          run.e[0] = min(run.e[0], z); run.e[1] = min(run.e[1], y); run.e[2] = min(run.e[2], x);
          run.e[3] = max(run.e[3], z); run.e[4] = max(run.e[4], y); run.e[5] = max(run.e[5], x);
        }
      }
    }
  }
  inst_flush(run, ext, hdr);
  const bool wz = __any(zero), wb = __any(bad);
  if ((threadIdx.x & 63) == 0) {
    if (wz) atomicMax(hdr + 2, 1);
    if (wb) atomicMax(flags, 4);
  }
}

// The finalisation both clinical box routes (instances, binary) share: a box is kept where its inclusive integer extents
// differ on every axis (then, and only then, the f32 volume product is not 0) and is written as f32(extent) / f32(size).
__device__ __forceinline__ bool ext_has_volume(const int* e) { return e[3] > e[0] && e[4] > e[1] && e[5] > e[2]; }

__device__ __forceinline__ void write_box_row(const int* e, const float* size, int row, int label,
                                              float* __restrict__ boxes, long long* __restrict__ labels) {
#pragma unroll
  for (int j = 0; j < 6; ++j) boxes[(long long)row * 6 + j] = __fdiv_rn((float)e[j], size[j % 3]);
  labels[row] = label;
}

// one workgroup: rows in (image, pair, ascending id) order.  The first unique value of an image is discarded: 0 where
// there is background, the smallest id where there is none.
__global__ __launch_bounds__(FIN_THREADS) void inst_final_kernel(const int* __restrict__ ext_all,
                                                                 const int* __restrict__ hdr_all, InstPairs pairs, int N,
                                                                 int D, int H, int W, int capacity,
                                                                 float* __restrict__ boxes, long long* __restrict__ labels,
                                                                 int* __restrict__ obj_off, const int* __restrict__ flags,
                                                                 int* __restrict__ overflow) {
  __shared__ int lds[33];
  const float size[3] = {(float)D, (float)H, (float)W};
  int carry = 0;
  for (int n = 0; n < N; ++n) {
    if (threadIdx.x == 0) obj_off[n] = carry < capacity ? carry : capacity;
    const int* ext = ext_all + (long long)n * INST_IDS * 6;
    const int lo_id = hdr_all[n * INST_HDR], hi_id = hdr_all[n * INST_HDR + 1];
    const int lost = hdr_all[n * INST_HDR + 2] ? 0 : lo_id;
    for (int pi = 0; pi < pairs.n; ++pi) {
      const int lo = pairs.lo[pi] > 1 ? pairs.lo[pi] : 1;
      const int hi = pairs.hi[pi] <= hi_id ? pairs.hi[pi] : hi_id + 1;  // exclusive; hi_id = -1 on an empty image
      for (int b = lo; b < hi; b += FIN_THREADS) {
        const int id = b + (int)threadIdx.x;
        int keep = 0;
        int e[6];
        if (id < hi) {
#pragma unroll
          for (int j = 0; j < 6; ++j) e[j] = ext[(long long)id * 6 + j];
          keep = id != lost && ext_has_volume(e);  // absent ids have max -1 < min
        }
        int tot;
        const int row = carry + block_excl_scan(keep, lds, &tot);
        if (keep && row < capacity) write_box_row(e, size, row, pi + 1, boxes, labels);
        carry += tot;
      }
    }
  }
  if (threadIdx.x == 0) {
    obj_off[N] = carry < capacity ? carry : capacity;  // in bounds even on overflow (the flag says it happened)
    *overflow = flags[0] | (carry > capacity ? 1 : 0);
  }
}

size_t inst_ws_bytes(int N) { return ((size_t)N * INST_IDS * 6 + (size_t)N * INST_HDR + 4) * sizeof(int); }

}  // namespace

extern "C" {

int msl_foreground_box(const float* vol, int D, int H, int W, int margin, int* box, void* stream) {
  return foreground_box(vol, 1, D, H, W, margin, box, stream);
}

int msl_foreground_box_mc(const float* vol, int C, int D, int H, int W, int margin, int* box, void* stream) {
  return foreground_box(vol, C, D, H, W, margin, box, stream);
}

// one sequence: both arenas hold arena_elems elements, the C = 1 case of the launch below
int msl_augment_fit(const float* arena_img, const short* arena_seg, long long arena_elems, const long long* table,
                    int n_cases, const double* params, int N, int T0, int T1, int T2, float* dst_img, short* dst_seg,
                    void* stream) {
  return augment_mc<false>(arena_img, arena_seg, /*seg_elems=*/arena_elems, /*C=*/1, table, n_cases, params,
                           /*windows=*/nullptr, N, T0, T1, T2, dst_img, dst_seg, stream);
}

int msl_augment_fit_mc(const float* arena_img, const short* arena_seg, long long seg_elems, int C, const long long* table,
                       int n_cases, const double* params, int N, int T0, int T1, int T2, float* dst_img, short* dst_seg,
                       void* stream) {
  return augment_mc<false>(arena_img, arena_seg, seg_elems, C, table, n_cases, params, nullptr, N, T0, T1, T2, dst_img,
                           dst_seg, stream);
}

int msl_augment_window_mc(const float* arena_img, const short* arena_seg, long long seg_elems, int C,
                          const long long* table, int n_cases, const double* params, const int* windows, int N, int T0,
                          int T1, int T2, float* dst_img, short* dst_seg, void* stream) {
  if (!windows) return MSL_ERR_ARG;
  return augment_mc<true>(arena_img, arena_seg, seg_elems, C, table, n_cases, params, windows, N, T0, T1, T2, dst_img,
                          dst_seg, stream);
}

int msl_augment_warp_mc(const float* arena_img, const short* arena_seg, long long seg_elems, int C,
                        const long long* table, int n_cases, const double* params, const double* coords,
                        long long coords_len, const int* windows, int N, int T0, int T1, int T2, float* dst_img,
                        short* dst_seg, void* stream) {
  return augment_rows([](auto ch) { return warp_kernel<decltype(ch)::value>; }, arena_img, arena_seg, seg_elems, C, table,
                      n_cases, params, coords, coords_len, windows, N, T0, T1, T2, dst_img, dst_seg, stream);
}

int msl_augment_deform_mc(const float* arena_img, const short* arena_seg, long long seg_elems, int C,
                          const long long* table, int n_cases, const double* params, const double* lattices,
                          long long lattices_len, const int* windows, int N, int T0, int T1, int T2, float* dst_img,
                          short* dst_seg, void* stream) {
  return augment_rows([](auto ch) { return deform_kernel<decltype(ch)::value>; }, arena_img, arena_seg, seg_elems, C, table,
                      n_cases, params, lattices, lattices_len, windows, N, T0, T1, T2, dst_img, dst_seg, stream);
}

size_t msl_instance_boxes_workspace_bytes(int N) { return N > 0 && N <= 65535 ? inst_ws_bytes(N) : 0; }

int msl_instance_boxes(const short* seg, int N, int D, int H, int W, const int* thresholds, int n_pairs, int capacity,
                       void* workspace, size_t workspace_bytes, float* boxes, long long* labels, int* obj_off,
                       int* overflow, void* stream) {
  if (!seg || !thresholds || !workspace || !boxes || !labels || !obj_off || !overflow || capacity < 0) return MSL_ERR_ARG;
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || n_pairs <= 0) return MSL_ERR_ARG;
  if (N > 65535 || n_pairs > INST_MAX_PAIRS || (long long)D * H * W >= 0x7FFFFFF0LL) return MSL_ERR_UNSUPPORTED;
  if (workspace_bytes < inst_ws_bytes(N)) return MSL_ERR_ARG;
  InstPairs pairs;
  pairs.n = n_pairs;
  for (int k = 0; k < INST_MAX_PAIRS; ++k) {  // the table is read here, on the host: it need not outlive the call
    pairs.lo[k] = k < n_pairs ? thresholds[2 * k] : 0;
    pairs.hi[k] = k < n_pairs ? thresholds[2 * k + 1] : 0;
  }
  hipStream_t st = (hipStream_t)stream;
  int* ext = (int*)workspace;
  int* hdr = ext + (size_t)N * INST_IDS * 6;
  int* flags = hdr + (size_t)N * INST_HDR;
  const int V = D * H * W;
  const long long ext_words = (long long)N * INST_IDS * 6;
  MSL_LAUNCH(inst_init_kernel, dim3(grid_for(ext_words)), dim3(DP_THREADS), 0, st, ext, ext_words, hdr, N, flags);
  const int chunks = (V + INST_VEC - 1) / INST_VEC;
  int gx = (chunks + DP_THREADS - 1) / DP_THREADS;
  const int cap = (2048 + N - 1) / N;
  if (gx > cap) gx = cap;
  const bool vec = V % INST_VEC == 0 && ((uintptr_t)seg & 15) == 0;
  if (vec)
    MSL_LAUNCH(inst_extent_kernel<true>, dim3(gx, N), dim3(DP_THREADS), 0, st, seg, V, H, W, ext, hdr, flags);
  else
    MSL_LAUNCH(inst_extent_kernel<false>, dim3(gx, N), dim3(DP_THREADS), 0, st, seg, V, H, W, ext, hdr, flags);
  MSL_LAUNCH(inst_final_kernel, dim3(1), dim3(FIN_THREADS), 0, st, (const int*)ext, (const int*)hdr, pairs, N, D, H, W,
             capacity, boxes, labels, obj_off, (const int*)flags, overflow);
  MSL_LAUNCH_CHECK();
  return MSL_OK;
}

}  // extern "C"

// ---- binary masks: run-based connected components -> boxes ----------------------------------------------------------
// Host mirror: datasets.boxes_from_instances(seg, [(1, inf)], mode="binary") (scipy.ndimage.label, then the instance walk).
// The unit of the union-find is a run of consecutive non-zero voxels of one row: the mask is
// sparse, so everything behind the two dense reads scales with the number of runs, and no per-voxel array is kept.
//
//   count  : one wave per row (BIN_ROWS rows per round, their loads leaving back to back); a lane holds one aligned
//            16-byte chunk of the row as a bit mask, a run starts where a set bit follows a clear one (the neighbour
//            lane's last bit comes over a shuffle); the row's count is a plain store, a background voxel marks its image
//   scan   : one workgroup, exclusive offsets of the N*D*H counts in place: runs are numbered in raster order
//   write  : the count pass again on the rows that hold a run: the k-th start of a row is written by the lane that holds
//            it and the k-th end by the lane that holds that (both ranks from one packed wave scan), so a run may cross
//            lanes and spans without anybody walking along it
//   union  : one thread per run: the runs of rows y-1 and z-1 that share a column (binary search for the first, then a
//            walk while they overlap) are united, larger root under smaller: a component's root is its first run in
//            raster order, which holds its first voxel: scipy's numbering
//   fold   : one thread per run: integer min / max of its extents into the root's record (a wave whose runs share a root
//            folds them first); min z needs no record, it is the root's own row
//   final  : one workgroup ranks the roots of each image by the fixed-order scan, drops the first component of an image
//            without background (np.unique(...)[1:]) and the flat boxes, writes the rows with the instance route's
//            arithmetic
namespace {

constexpr int BIN_ROWS = 4;                // rows per wave and round
constexpr int BIN_SPAN = 64 * INST_VEC;    // voxels a wave covers with one load per lane
constexpr int BIN_EXT = 5;                 // ints per run: min y, min x, max z, max y, max x (of its component, at the root)
constexpr int BIN_WAVES = DP_THREADS / 64;

struct BinPlan {
  size_t rowoff, rrow, rx0, rx1, link, ext, bg, hdr, total;
};

bool bin_supported(int N, int D, int H, int W, int run_cap) {
  return N > 0 && D > 0 && H > 0 && W > 0 && run_cap > 0 && N <= 65535 && W <= 0x3FFFFFFF &&
         (long long)N * D * H < 0x7FFF0000LL && (long long)run_cap * BIN_EXT < 0x7FFFFFF0LL;
}

// rowoff (N*D*H + 1), four ints per run (row, first x, last x, link), BIN_EXT ints per run, one int per image, header
BinPlan bin_plan(int N, int D, int H, int run_cap) {
  BinPlan p;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  size_t at = 0;
  p.rowoff = at; at += up(((size_t)N * D * H + 1) * 4);
  p.rrow = at; at += up((size_t)run_cap * 4);
  p.rx0 = at; at += up((size_t)run_cap * 4);
  p.rx1 = at; at += up((size_t)run_cap * 4);
  p.link = at; at += up((size_t)run_cap * 4);
  p.ext = at; at += up((size_t)run_cap * BIN_EXT * 4);
  p.bg = at; at += up((size_t)N * 4);
  p.hdr = at; at += 256;
  p.total = at;
  return p;
}

typedef short short8v __attribute__((ext_vector_type(8)));

// eight voxels from global voxel g0 (a multiple of eight) of a buffer of `total` voxels; past the end reads as 0
template <bool VEC>
__device__ __forceinline__ short8v bin_load8(const short* __restrict__ seg, long long g0, long long total) {
  if (VEC && g0 + INST_VEC <= total) return *reinterpret_cast<const short8v*>(seg + g0);
  short8v v;
#pragma unroll
  for (int j = 0; j < INST_VEC; ++j) v[j] = g0 + j < total ? seg[g0 + j] : (short)0;
  return v;
}

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

__global__ __launch_bounds__(DP_THREADS) void bin_init_kernel(int* __restrict__ bg, int N) {
  for (int i = blockIdx.x * DP_THREADS + threadIdx.x; i < N; i += gridDim.x * DP_THREADS) bg[i] = 0;
}

// WRITE = false: rowoff[r] = runs of row r, bg[n] = 1 where image n holds a zero.  WRITE = true: rowoff holds the scanned
// offsets; the records of the runs below run_cap are written.  VEC: seg is 16-byte aligned (chunks are counted from the
// start of the buffer, so a row may begin inside one: the voxels of a chunk outside the row are masked out).
template <bool VEC, bool WRITE>
__global__ __launch_bounds__(DP_THREADS) void bin_rows_kernel(const short* __restrict__ seg, int N, int D, int H, int W,
                                                              int run_cap, int* __restrict__ rowoff,
                                                              int* __restrict__ rrow, int* __restrict__ rx0,
                                                              int* __restrict__ rx1, int* __restrict__ link,
                                                              int* __restrict__ ext, int* __restrict__ bg) {
  const int lane = threadIdx.x & 63;
  const int DH = D * H;
  const long long R = (long long)N * DH, total = R * W;
  const long long step = (long long)gridDim.x * BIN_WAVES * BIN_ROWS;
  int zimg = -1;
  bool zero = false;
  for (long long r0 = ((long long)blockIdx.x * BIN_WAVES + (threadIdx.x >> 6)) * BIN_ROWS; r0 < R; r0 += step) {
    short8v xs[BIN_ROWS];
    int base[BIN_ROWS], cnt[BIN_ROWS];
#pragma unroll
    for (int u = 0; u < BIN_ROWS; ++u) {  // the first loads of the round leave back to back
      const long long r = r0 + u;
      base[u] = 0;
      cnt[u] = r < R;
      if (WRITE && r < R) {
        base[u] = rowoff[r];
        cnt[u] = rowoff[r + 1] - base[u];  // a row without a run is not read again
      }
      xs[u] = (short8v)(short)0;
      if (cnt[u] > 0) {
        const long long g = r * W, gl = ((g >> 3) + lane) * INST_VEC;
        if (gl < g + W) xs[u] = bin_load8<VEC>(seg, gl, total);
      }
    }
#pragma unroll
    for (int u = 0; u < BIN_ROWS; ++u) {  // (unrolled: xs stays in registers)
      if (cnt[u] <= 0) continue;
      const int r = (int)(r0 + u);
      const long long g = (long long)r * W;
      const int y = r % H, z = (r / H) % D, n = r / DH;
      if (!WRITE && n != zimg) {  // a wave's rows ascend: one atomic per wave and image
        if (__any(zero) && lane == 0) atomicMax(bg + zimg, 1);
        zimg = n;
        zero = false;
      }
      const int nspan = (int)(((g & 7) + W + BIN_SPAN - 1) / BIN_SPAN);
      int carry_s = 0, carry_e = 0;
      unsigned carry_prev = 0;
      for (int s = 0; s < nspan; ++s) {
        const long long gl = ((g >> 3) + (long long)s * 64 + lane) * INST_VEC;
        short8v x = xs[u];
        if (s > 0) {
          x = (short8v)(short)0;
          if (gl < g + W) x = bin_load8<VEC>(seg, gl, total);
        }
        // bits of the chunk that lie in the row
        const long long lo = g - gl, hi = g + W - gl;
        const int blo = lo > 0 ? (int)lo : 0, bhi = hi < INST_VEC ? (int)hi : INST_VEC;
        const unsigned vmask = bhi > blo ? ((1u << bhi) - 1u) & ~((1u << blo) - 1u) : 0u;
        unsigned nz = 0;
#pragma unroll
        for (int j = 0; j < INST_VEC; ++j) nz |= (x[j] != 0 ? 1u : 0u) << j;
        const unsigned m = nz & vmask;
        if (!WRITE) zero = zero || (vmask & ~nz) != 0;
        if (__ballot(m != 0) == 0) {  // background: one read and nothing else
          carry_prev = 0;
          continue;
        }
        const unsigned up = (unsigned)__shfl_up((int)m, 1, 64);
        const unsigned prev = lane ? (up >> 7) & 1u : carry_prev;
        const unsigned starts = m & ~((m << 1) | prev) & 0xFFu;
        carry_prev = ((unsigned)__shfl((int)m, 63, 64) >> 7) & 1u;
        if (!WRITE) {
          int c = __popc(starts);
#pragma unroll
          for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
          carry_s += c;
        } else {
          const unsigned dn = (unsigned)__shfl_down((int)m, 1, 64);
          unsigned next = dn & 1u;
          if (lane == 63) {  // the voxel behind the span decides whether a run ends at its last voxel
            next = 0;
            if ((m >> 7) && gl + INST_VEC < g + W) next = seg[gl + INST_VEC] != 0;
          }
          const unsigned ends = m & ~((m >> 1) | (next << 7));
          const int packed = __popc(starts) | (__popc(ends) << 16);  // at most 256 of either per span
          const int inc = wave_incl_scan(packed, lane);
          const int tot = __shfl(inc, 63, 64);
          int si = base[u] + carry_s + ((inc - packed) & 0xFFFF);
          int ei = base[u] + carry_e + ((inc - packed) >> 16);
          const int end = base[u] + cnt[u] < run_cap ? base[u] + cnt[u] : run_cap;
          for (unsigned b = starts; b; b &= b - 1, ++si) {
            if (si >= end) break;
            const int xv = (int)(gl + (__ffs((int)b) - 1) - g);
            rrow[si] = r;
            rx0[si] = xv;
            link[si] = si;
            int* e = ext + (long long)si * BIN_EXT;
            e[0] = y; e[1] = xv; e[2] = z; e[3] = y;
          }
          for (unsigned b = ends; b; b &= b - 1, ++ei) {
            if (ei >= end) break;
            const int xv = (int)(gl + (__ffs((int)b) - 1) - g);
            rx1[ei] = xv;
            ext[(long long)ei * BIN_EXT + 4] = xv;
          }
          carry_s += tot & 0xFFFF;
          carry_e += tot >> 16;
        }
      }
      if (!WRITE && lane == 0) rowoff[r] = carry_s;
    }
  }
  if (!WRITE && __any(zero) && lane == 0) atomicMax(bg + zimg, 1);
}

// one workgroup: exclusive offsets of the R row counts in place, rowoff[R] = number of runs; eight rows per thread
__global__ __launch_bounds__(SCAN_THREADS) void bin_scan_kernel(int* __restrict__ rowoff, int R, int run_cap,
                                                                int* __restrict__ hdr) {
  __shared__ int lds[33];
  int carry = 0;
  for (long long b = 0; b < R; b += SCAN_THREADS * 8) {
    const long long i0 = b + (long long)threadIdx.x * 8;
    int v[8], sum = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      v[k] = i0 + k < R ? rowoff[i0 + k] : 0;
      sum += v[k];
    }
    int tot;
    int at = carry + block_excl_scan(sum, lds, &tot);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (i0 + k < R) rowoff[i0 + k] = at;
      at += v[k];
    }
    carry += tot;
  }
  if (threadIdx.x == 0) {
    rowoff[R] = carry;
    hdr[0] = carry > run_cap ? 8 : 0;
  }
}

__device__ __forceinline__ void bin_unite_row(int i, int x0, int x1, int lo, int hi, const int* __restrict__ rx0,
                                              const int* __restrict__ rx1, int* link) {
  int a = lo, b = hi;  // the first run of the row that ends at or behind x0 (the runs of a row ascend)
  while (a < b) {
    const int mid = a + (b - a) / 2;
    if (rx1[mid] < x0) a = mid + 1;
    else b = mid;
  }
  for (int j = a; j < hi && rx0[j] <= x1; ++j) unite(link, i, j);
}

__global__ __launch_bounds__(DP_THREADS) void bin_union_kernel(const int* __restrict__ rowoff,
                                                               const int* __restrict__ rrow, const int* __restrict__ rx0,
                                                               const int* __restrict__ rx1, int* link, int D, int H,
                                                               int R, int run_cap) {
  const int total = rowoff[R] < run_cap ? rowoff[R] : run_cap;
  for (int i = blockIdx.x * DP_THREADS + threadIdx.x; i < total; i += gridDim.x * DP_THREADS) {
    const int r = rrow[i], x0 = rx0[i], x1 = rx1[i];
    const int y = r % H, z = (r / H) % D;
    if (y > 0) bin_unite_row(i, x0, x1, rowoff[r - 1], rowoff[r], rx0, rx1, link);  // (r < its own index: below the cap)
    if (z > 0) bin_unite_row(i, x0, x1, rowoff[r - H], rowoff[r - H + 1], rx0, rx1, link);
  }
}

__global__ __launch_bounds__(DP_THREADS) void bin_fold_kernel(const int* __restrict__ rowoff,
                                                              const int* __restrict__ rrow, const int* __restrict__ rx0,
                                                              const int* __restrict__ rx1, const int* link,
                                                              int* __restrict__ ext, int D, int H, int R, int run_cap) {
  const int total = rowoff[R] < run_cap ? rowoff[R] : run_cap;
  const int stride = gridDim.x * DP_THREADS;
  const int start = blockIdx.x * DP_THREADS + threadIdx.x;
  const int iters = (total + stride - 1) / stride;  // the same for every lane: the wave stays converged
  for (int it = 0; it < iters; ++it) {
    const long long i = (long long)start + (long long)it * stride;
    int root = -1, y = 0, z = 0, x0 = 0, x1 = 0;
    if (i < total) {
      const int q = find_root(link, (int)i);
      if (q != (int)i) {  // a root's record already holds its own run
        root = q;
        const int r = rrow[i];
        y = r % H; z = (r / H) % D; x0 = rx0[i]; x1 = rx1[i];
      }
    }
    const unsigned long long act = __ballot(root >= 0);
    if (act == 0) continue;
    const int r0 = __shfl(root, __ffsll((long long)act) - 1, 64);
    if (__all(root < 0 || root == r0)) {
      const bool a = root >= 0;
      const int my = wave_min(a ? y : IMAX), mx = wave_min(a ? x0 : IMAX);
      const int Mz = wave_max(a ? z : -1), My = wave_max(a ? y : -1), Mx = wave_max(a ? x1 : -1);
      if ((threadIdx.x & 63) == 0) {
        int* e = ext + (long long)r0 * BIN_EXT;
        atomicMin(e + 0, my); atomicMin(e + 1, mx); atomicMax(e + 2, Mz); atomicMax(e + 3, My); atomicMax(e + 4, Mx);
      }
    } else if (root >= 0) {
      int* e = ext + (long long)root * BIN_EXT;
      atomicMin(e + 0, y); atomicMin(e + 1, x0); atomicMax(e + 2, z); atomicMax(e + 3, y); atomicMax(e + 4, x1);
    }
  }
}

// one workgroup: per image its roots in run order (= scipy's label order), label 1.  An image without a background voxel is
// one component, whose root is the image's first run: np.unique(...)[1:] drops it.
__global__ __launch_bounds__(FIN_THREADS) void bin_final_kernel(const int* __restrict__ rowoff,
                                                                const int* __restrict__ rrow,
                                                                const int* __restrict__ link,
                                                                const int* __restrict__ ext, const int* __restrict__ bg,
                                                                const int* __restrict__ hdr, int N, int D, int H, int W,
                                                                int run_cap, int capacity, float* __restrict__ boxes,
                                                                long long* __restrict__ labels, int* __restrict__ obj_off,
                                                                int* __restrict__ overflow) {
  __shared__ int lds[33];
  const float size[3] = {(float)D, (float)H, (float)W};
  const int DH = D * H;
  int carry = 0;
  for (int n = 0; n < N; ++n) {
    if (threadIdx.x == 0) obj_off[n] = carry < capacity ? carry : capacity;
    int lo = rowoff[(long long)n * DH], hi = rowoff[(long long)(n + 1) * DH];
    lo = lo < run_cap ? lo : run_cap;
    hi = hi < run_cap ? hi : run_cap;
    const int lost = bg[n] ? -1 : lo;
    for (int b = lo; b < hi; b += FIN_THREADS) {
      const int i = b + (int)threadIdx.x;
      int keep = 0;
      int e[6];
      if (i < hi && link[i] == i && i != lost) {
        e[0] = (rrow[i] / H) % D;  // the root is the component's first run in raster order: its row holds the smallest z
        e[1] = ext[(long long)i * BIN_EXT + 0]; e[2] = ext[(long long)i * BIN_EXT + 1];
        e[3] = ext[(long long)i * BIN_EXT + 2]; e[4] = ext[(long long)i * BIN_EXT + 3];
        e[5] = ext[(long long)i * BIN_EXT + 4];
        keep = ext_has_volume(e);
      }
      int tot;
      const int row = carry + block_excl_scan(keep, lds, &tot);
      if (keep && row < capacity) write_box_row(e, size, row, 1, boxes, labels);
      carry += tot;
    }
  }
  if (threadIdx.x == 0) {
    obj_off[N] = carry < capacity ? carry : capacity;  // in bounds even on overflow (the flag says it happened)
    *overflow = hdr[0] | (carry > capacity ? 1 : 0);
  }
}

}  // namespace

extern "C" {

size_t msl_binary_boxes_workspace_bytes(int N, int D, int H, int W, int run_cap) {
  return bin_supported(N, D, H, W, run_cap) ? bin_plan(N, D, H, run_cap).total : 0;
}

int msl_binary_boxes(const short* seg, int N, int D, int H, int W, int capacity, int run_cap, void* workspace,
                     size_t workspace_bytes, float* boxes, long long* labels, int* obj_off, int* overflow,
                     void* stream) {
  if (!seg || !workspace || !boxes || !labels || !obj_off || !overflow || capacity < 0) return MSL_ERR_ARG;
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || run_cap <= 0) return MSL_ERR_ARG;
  if (!bin_supported(N, D, H, W, run_cap)) return MSL_ERR_UNSUPPORTED;
  const BinPlan p = bin_plan(N, D, H, run_cap);
  if (workspace_bytes < p.total || ((uintptr_t)workspace & 3) != 0 || ((uintptr_t)seg & 1) != 0) return MSL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int* rowoff = (int*)(ws + p.rowoff);
  int* rrow = (int*)(ws + p.rrow);
  int* rx0 = (int*)(ws + p.rx0);
  int* rx1 = (int*)(ws + p.rx1);
  int* link = (int*)(ws + p.link);
  int* ext = (int*)(ws + p.ext);
  int* bg = (int*)(ws + p.bg);
  int* hdr = (int*)(ws + p.hdr);
  const int R = N * D * H;
  const long long rounds = ((long long)R + BIN_WAVES * BIN_ROWS - 1) / (BIN_WAVES * BIN_ROWS);
  const dim3 rgrid((unsigned)(rounds < 2048 ? rounds : 2048));
  const dim3 ugrid(grid_for(run_cap));
  const bool vec = ((uintptr_t)seg & 15) == 0;
  MSL_LAUNCH(bin_init_kernel, dim3(grid_for(N)), dim3(DP_THREADS), 0, st, bg, N);
  if (vec)
    MSL_LAUNCH(bin_rows_kernel<true, false>, rgrid, dim3(DP_THREADS), 0, st, seg, N, D, H, W, run_cap, rowoff, rrow, rx0,
               rx1, link, ext, bg);
  else
    MSL_LAUNCH(bin_rows_kernel<false, false>, rgrid, dim3(DP_THREADS), 0, st, seg, N, D, H, W, run_cap, rowoff, rrow,
               rx0, rx1, link, ext, bg);
  MSL_LAUNCH(bin_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, rowoff, R, run_cap, hdr);
  if (vec)
    MSL_LAUNCH(bin_rows_kernel<true, true>, rgrid, dim3(DP_THREADS), 0, st, seg, N, D, H, W, run_cap, rowoff, rrow, rx0,
               rx1, link, ext, bg);
  else
    MSL_LAUNCH(bin_rows_kernel<false, true>, rgrid, dim3(DP_THREADS), 0, st, seg, N, D, H, W, run_cap, rowoff, rrow, rx0,
               rx1, link, ext, bg);
  MSL_LAUNCH(bin_union_kernel, ugrid, dim3(DP_THREADS), 0, st, (const int*)rowoff, (const int*)rrow, (const int*)rx0,
             (const int*)rx1, link, D, H, R, run_cap);
  MSL_LAUNCH(bin_fold_kernel, ugrid, dim3(DP_THREADS), 0, st, (const int*)rowoff, (const int*)rrow, (const int*)rx0,
             (const int*)rx1, (const int*)link, ext, D, H, R, run_cap);
  MSL_LAUNCH(bin_final_kernel, dim3(1), dim3(FIN_THREADS), 0, st, (const int*)rowoff, (const int*)rrow,
             (const int*)link, (const int*)ext, (const int*)bg, (const int*)hdr, N, D, H, W, run_cap, capacity, boxes,
             labels, obj_off, overflow);
  MSL_LAUNCH_CHECK();
  return MSL_OK;
}

}  // extern "C"

// ---- native grid -> LPI at 1 mm: signed axis permutation + per-axis resample of one case -------------------------------
// Host mirror: datasets.regrid (np.transpose / np.flip, then scipy.ndimage.affine_transform with a diagonal matrix and
// mode "nearest": order 1 for the image planes, order 0 for the mask).  Output voxel o reads the reoriented volume at
// c_k = step_k * o_k + start_k, which is affine_kernel's coordinate row for a diagonal matrix (its off-diagonal terms
// add +0.0), then the core's taps and weights under NEAREST_UNCLAMPED (rg_axis below) and its eight-corner sum.
//
// The map is separable, so the per-axis entries (two source indices after the boundary map and the reversal, the order-0
// index, the f64 weight of the lower tap) are not per-voxel work: a workgroup builds the entries of its (up to RG_TW)
// output columns once, into LDS, and then walks output rows, one wave per row; the wave computes the two entries of
// the row's axes 0 and 1 once per row.  A lane owns four consecutive output voxels (one 16-byte image store per plane,
// one 8-byte mask store) and loops the C channels inside, so the indices, the weights and the mask tap are formed once
// per voxel.  FAST: the reoriented last axis is the source's last axis (flips and spacing only), so the taps of a lane
// group lie in the four contiguous source rows (2 x 2 taps of axes 0 and 1) and the column index is the element offset.
namespace {

constexpr int RG_TW = 1024;                   // output columns per workgroup (20 KiB of LDS)
constexpr int RG_WAVES = DP_THREADS / 64;     // output rows in flight per workgroup
constexpr int RG_VEC = STORE_VEC;             // output voxels per lane and pass

struct RgPlan {  // the reoriented volume, axis k: length, reversal, source stride (elements); the sampling step / start
  int len[3], rev[3];
  long long stride[3];
  double step[3], start[3];
};

// taps of output index o on one axis, as source indices: the coordinate step * o + start under scipy's own "nearest"
// (NEAREST_UNCLAMPED), then the reversal folded into the tap indices
__device__ __forceinline__ AxisTaps rg_axis(int o, double step, double start, int len, int rev) {
  double c = 0.0;
  c = c + (double)o * step;
  c = c + start;
  AxisTaps t = axis_taps(c, len, boundary::NEAREST_UNCLAMPED);
  if (rev) {
    t.i1[0] = len - 1 - t.i1[0];
    t.i1[1] = len - 1 - t.i1[1];
    t.i0 = len - 1 - t.i0;
  }
  return t;
}

template <int C, bool FAST, bool VEC>
__global__ __launch_bounds__(DP_THREADS) void regrid_kernel(const float* __restrict__ src_img,
                                                            const short* __restrict__ src_seg, long long SV, RgPlan p,
                                                            int m0, int m1, int m2, float* __restrict__ dst_img,
                                                            short* __restrict__ dst_seg) {
  __shared__ int t_ia[RG_TW], t_ib[RG_TW], t_in[RG_TW];
  __shared__ double t_w[RG_TW];
  const int x_base = blockIdx.y * RG_TW;
  const int x_cnt = (m2 - x_base) < RG_TW ? (m2 - x_base) : RG_TW;
  for (int i = threadIdx.x; i < x_cnt; i += DP_THREADS) {
    const AxisTaps t = rg_axis(x_base + i, p.step[2], p.start[2], p.len[2], p.rev[2]);
    t_ia[i] = t.i1[0];
    t_ib[i] = t.i1[1];
    t_in[i] = t.i0;
    t_w[i] = t.w[0];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long rows = (long long)m0 * m1;
  const long long MV = rows * m2;
  const long long st2 = FAST ? 1LL : p.stride[2];
  for (long long r = (long long)blockIdx.x * RG_WAVES + wave; r < rows; r += (long long)gridDim.x * RG_WAVES) {
    const AxisTaps a0 = rg_axis((int)(r / m1), p.step[0], p.start[0], p.len[0], p.rev[0]);
    const AxisTaps a1 = rg_axis((int)(r % m1), p.step[1], p.start[1], p.len[1], p.rev[1]);
    long long rr[2][2];  // the four tap rows of the image, the one of the mask
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) rr[a][b] = a0.i1[a] * p.stride[0] + a1.i1[b] * p.stride[1];
    const long long rq = a0.i0 * p.stride[0] + a1.i0 * p.stride[1];
    for (int x = lane * RG_VEC; x < x_cnt; x += 64 * RG_VEC) {
      const int cnt = VEC ? RG_VEC : ((x_cnt - x) < RG_VEC ? (x_cnt - x) : RG_VEC);
      float vi[C][RG_VEC];
      short vs[RG_VEC];
#pragma unroll
      for (int j = 0; j < RG_VEC; ++j) {
#pragma unroll
        for (int c = 0; c < C; ++c) vi[c][j] = 0.0f;
        vs[j] = 0;
        if (j < cnt) {
          if (src_img) {
            const long long col[2] = {t_ia[x + j] * st2, t_ib[x + j] * st2};
            const double w2[2] = {t_w[x + j], 1.0 - t_w[x + j]};
            double acc[C];
            trilinear<C>(src_img, SV, rr, col, a0.w, a1.w, w2, acc);
#pragma unroll
            for (int c = 0; c < C; ++c) vi[c][j] = (float)acc[c];
          }
          if (src_seg) vs[j] = src_seg[rq + t_in[x + j] * st2];
        }
      }
      // VEC: m2 % 4 == 0, so every group is whole
      const long long out = r * m2 + x_base + x;
      store_group<C, VEC>(vi, vs, cnt, dst_img ? dst_img + out : nullptr, MV, dst_seg ? dst_seg + out : nullptr);
    }
  }
}

template <int C>
void launch_regrid(bool fast, bool vec, dim3 grid, hipStream_t st, const float* src_img, const short* src_seg, long long SV,
                   const RgPlan& p, int m0, int m1, int m2, float* dst_img, short* dst_seg) {
  if (fast && vec)
    MSL_LAUNCH(regrid_kernel<C, true, true>, grid, dim3(DP_THREADS), 0, st, src_img, src_seg, SV, p, m0, m1, m2, dst_img, dst_seg);
  else if (fast)
    MSL_LAUNCH(regrid_kernel<C, true, false>, grid, dim3(DP_THREADS), 0, st, src_img, src_seg, SV, p, m0, m1, m2, dst_img, dst_seg);
  else if (vec)
    MSL_LAUNCH(regrid_kernel<C, false, true>, grid, dim3(DP_THREADS), 0, st, src_img, src_seg, SV, p, m0, m1, m2, dst_img, dst_seg);
  else
    MSL_LAUNCH(regrid_kernel<C, false, false>, grid, dim3(DP_THREADS), 0, st, src_img, src_seg, SV, p, m0, m1, m2, dst_img, dst_seg);
}

}  // namespace

extern "C" {

int msl_regrid(const float* src_img, const short* src_seg, int C, int n0, int n1, int n2, const double* plan, int m0,
               int m1, int m2, float* dst_img, short* dst_seg, void* stream) {
  if (!plan || (!src_img && !src_seg) || (src_img == nullptr) != (dst_img == nullptr) ||
      (src_seg == nullptr) != (dst_seg == nullptr))
    return MSL_ERR_ARG;
  if (C < 1 || C > FIT_MAX_CH || n0 < 1 || n1 < 1 || n2 < 1 || m0 < 1 || m1 < 1 || m2 < 1) return MSL_ERR_ARG;
  const int n[3] = {n0, n1, n2};
  const long long sstride[3] = {(long long)n1 * n2, (long long)n2, 1LL};
  RgPlan p;
  bool seen[3] = {false, false, false};
  for (int k = 0; k < 3; ++k) {  // the plan is read here, on the host: it need not outlive the call
    const double a = plan[k], r = plan[3 + k], step = plan[6 + k], start = plan[9 + k];
    if (!(a == 0.0 || a == 1.0 || a == 2.0) || !(r == 0.0 || r == 1.0)) return MSL_ERR_ARG;
    if (seen[(int)a]) return MSL_ERR_ARG;
    seen[(int)a] = true;
    if (!(step > 0.0) || step - step != 0.0 || start - start != 0.0) return MSL_ERR_ARG;  // x - x != 0: inf or NaN
    p.len[k] = n[(int)a];
    p.rev[k] = (int)r;
    p.stride[k] = sstride[(int)a];
    p.step[k] = step;
    p.start[k] = start;
  }
  const long long rows = (long long)m0 * m1;
  const int gy = (m2 + RG_TW - 1) / RG_TW;
  if (gy > 65535) return MSL_ERR_UNSUPPORTED;
  long long gx = (rows + RG_WAVES - 1) / RG_WAVES;
  const long long cap = 2048 / gy > 0 ? 2048 / gy : 1;  // enough workgroups to fill the chip; each amortises its table
  if (gx > cap) gx = cap;
  const bool fast = p.stride[2] == 1;
  const bool vec = m2 % RG_VEC == 0 && ((uintptr_t)dst_img & 15) == 0 && ((uintptr_t)dst_seg & 7) == 0;
  const dim3 grid((unsigned)gx, (unsigned)gy);
  const long long SV = (long long)n0 * n1 * n2;
  hipStream_t st = (hipStream_t)stream;
  return msl::dispatch_int<1, 2, 3, 4>(C, [&](auto ch) {
    launch_regrid<decltype(ch)::value>(fast, vec, grid, st, src_img, src_seg, SV, p, m0, m1, m2, dst_img, dst_seg);
    MSL_LAUNCH_CHECK();
    return MSL_OK;
  });
}

}  // extern "C"
