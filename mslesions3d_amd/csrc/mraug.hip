// The MR acquisition stage of the training batch: Gaussian blur, multiplicative bias field and
// additive noise on a built (N, C, D, H, W) f32 batch, out of place.  Host mirror: datasets.gaussian_smooth / bias_field /
// gaussian_noise, operation by operation, so this file is built with FMA contraction off.
//
//   msl_augment_mr = two launches.
//     mr_axis0_kernel : the blur pass over axis 0 (D) of every blurred sample, src -> workspace.  A thread owns one (h, w)
//                       column and AX0_RUN consecutive planes: it reads each of the AX0_RUN + 2R input planes once.
//     mr_tile_kernel  : one workgroup per TH x TW tile of one (n, c, d) plane.  A blurred sample: the tile and its halo of
//                       (R_1, R_2) voxels workspace -> LDS, the pass over axis 1 (H) LDS -> LDS, the pass over axis 2 (W)
//                       LDS -> registers.  A sample without blur: src -> registers.  Then the epilogue on the registers:
//                       bias field (the sample's L^3 lattice in LDS, sampled through resample.hpp's taps and corner sum)
//                       and noise (one Philox4x32-10 block per voxel and channel), and the one store.
// Every branch on what a sample drew is uniform within a workgroup.  Every blur pass: acc = 0.0 (f64), acc += f64(w[k]) *
// f64(v[i + k - R]) for k ascending - the product of two f32 is exact in f64, so the order of the adds is the whole
// contract - and one rounding to f32.  A tap outside the axis contributes nothing; the tile passes add its exact +0.0
// product instead, which changes no partial sum (the sums start at +0.0 and never become -0.0).  No exponential is
// computed here: the taps and the lattice are the host's tables.  No atomics; every output voxel is written exactly once.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {
#include "resample.hpp"

constexpr int MR_STRIDE = 8;      // doubles per sample: flags, R_0, R_1, R_2, std, k0, k1, -
constexpr int MR_RMAX = 8;        // the largest blur radius
constexpr int MR_TAPS = 2 * MR_RMAX + 1;
constexpr int MR_LMAX = 9;        // lattice points per axis the LDS copy holds
constexpr int MR_BLUR = 1, MR_BIAS = 2, MR_NOISE = 4;
constexpr int MR_THREADS = 256;
constexpr int AX0_RUN = 8;        // output planes per thread of the axis-0 pass
constexpr int TH = 32, TW = 64;   // output tile of the fused pass
constexpr int TROWS = TH + 2 * MR_RMAX, TCOLS = TW + 2 * MR_RMAX;
constexpr int TPT = TH * TW / MR_THREADS;  // outputs per thread: rows ty, ty + 4, ...
static_assert(TW == 64 && MR_THREADS % TW == 0 && TH % (MR_THREADS / TW) == 0, "a wave owns a tile row");

struct MrRow {
  int flags, R[3];
  float std;
  unsigned k0, k1;
};

// The radii are clamped into the taps table whatever the row holds: nothing is read out of bounds.
__device__ __forceinline__ MrRow mr_row(const double* __restrict__ p) {
  MrRow r;
  r.flags = (int)p[0];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int R = (int)p[1 + a];
    r.R[a] = R < 0 ? 0 : (R > MR_RMAX ? MR_RMAX : R);
  }
  r.std = (float)p[4];  // an f32 value stored exactly
  r.k0 = (unsigned)p[5];
  r.k1 = (unsigned)p[6];
  return r;
}

// ---- blur over axis 0 ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MR_THREADS) void mr_axis0_kernel(const float* __restrict__ src,
                                                              const double* __restrict__ params,
                                                              const float* __restrict__ taps, int C, int D, long long HW,
                                                              int chunks, float* __restrict__ tmp) {
  __shared__ double s_w[MR_TAPS];
  const int nc = blockIdx.y, n = nc / C;
  const MrRow r = mr_row(params + (long long)n * MR_STRIDE);
  if (!(r.flags & MR_BLUR)) return;  // (uniform: the tile kernel reads such a sample from src)
  const int R = r.R[0];
  if (threadIdx.x <= 2 * R) s_w[threadIdx.x] = (double)taps[((long long)n * 3 + 0) * MR_TAPS + threadIdx.x];
  __syncthreads();
  const int d0 = (int)(blockIdx.x / chunks) * AX0_RUN;
  const long long col = (long long)(blockIdx.x % chunks) * MR_THREADS + threadIdx.x;
  if (col >= HW) return;
  const float* __restrict__ in = src + (long long)nc * D * HW + col;
  float* __restrict__ out = tmp + (long long)nc * D * HW + col;
  double acc[AX0_RUN];
#pragma unroll
  for (int j = 0; j < AX0_RUN; ++j) acc[j] = 0.0;
  const int lo = d0 - R > 0 ? d0 - R : 0;
  const int hi = d0 + AX0_RUN - 1 + R < D - 1 ? d0 + AX0_RUN - 1 + R : D - 1;
  for (int i = lo; i <= hi; ++i) {  // ascending input plane = ascending tap of every output plane
    const double v = (double)in[(long long)i * HW];
#pragma unroll
    for (int j = 0; j < AX0_RUN; ++j) {
      const int k = i - (d0 + j) + R;
      if (k >= 0 && k <= 2 * R) acc[j] = acc[j] + s_w[k] * v;
    }
  }
#pragma unroll
  for (int j = 0; j < AX0_RUN; ++j)
    if (d0 + j < D) out[(long long)(d0 + j) * HW] = (float)acc[j];
}

// ---- Philox4x32-10 and the eight-half normal --------------------------------------------------------------------------------
__device__ __forceinline__ float mr_normal(unsigned index, unsigned channel, unsigned k0, unsigned k1) {
  unsigned c0 = index, c1 = channel, c2 = 0u, c3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
  }
  const int S = (int)((c0 & 0xFFFFu) + (c0 >> 16) + (c1 & 0xFFFFu) + (c1 >> 16) + (c2 & 0xFFFFu) + (c2 >> 16) +
                      (c3 & 0xFFFFu) + (c3 >> 16));
  // f32(1 / sqrt(8 (2^32 - 1) / 12)), datasets.NOISE_SCALE; S - 262140 is exact in f32
  return __fmul_rn((float)(S - 262140), __uint_as_float(0x379CC471u));
}

// ---- fused passes over axes 1 and 2, bias and noise ------------------------------------------------------------------------
__global__ __launch_bounds__(MR_THREADS) void mr_tile_kernel(const float* __restrict__ src, const float* __restrict__ tmp,
                                                             const double* __restrict__ params,
                                                             const float* __restrict__ taps,
                                                             const float* __restrict__ lattice, int C, int D, int H, int W,
                                                             int L, int tiles_h, int tiles_w, float* __restrict__ dst) {
  __shared__ float s_in[TROWS][TCOLS];
  __shared__ float s_mid[TH][TCOLS];
  __shared__ double s_w[2][MR_TAPS];
  __shared__ float s_lat[MR_LMAX * MR_LMAX * MR_LMAX];
  __shared__ int s_i1[2][TH], s_i2[2][TW];
  __shared__ double s_w1[2][TH], s_w2[2][TW];

  const int nc = blockIdx.y, n = nc / C, c = nc % C;
  const MrRow r = mr_row(params + (long long)n * MR_STRIDE);
  unsigned bx = blockIdx.x;
  const int w0 = (int)(bx % tiles_w) * TW;
  bx /= tiles_w;
  const int h0 = (int)(bx % tiles_h) * TH;
  const int d = (int)(bx / tiles_h);
  const long long plane = ((long long)nc * D + d) * H * W;
  const int tx = threadIdx.x % TW, ty = threadIdx.x / TW;
  constexpr int TYS = MR_THREADS / TW;
  float v[TPT];

  if (r.flags & MR_BLUR) {
    const int R1 = r.R[1], R2 = r.R[2];
    if (threadIdx.x < 2 * MR_TAPS) {
      const int a = threadIdx.x / MR_TAPS, k = threadIdx.x % MR_TAPS;
      s_w[a][k] = k <= 2 * r.R[1 + a] ? (double)taps[((long long)n * 3 + 1 + a) * MR_TAPS + k] : 0.0;
    }
    const int rows = TH + 2 * R1, cols = TW + 2 * R2;
    const float* __restrict__ in = tmp + plane;
    for (int y = ty; y < rows; y += TYS) {
      const int gh = h0 - R1 + y;
      for (int q = tx; q < cols; q += TW) {
        const int gw = w0 - R2 + q;
        const bool inside = gh >= 0 && gh < H && gw >= 0 && gw < W;
        s_in[y][q] = inside ? in[(long long)gh * W + gw] : 0.0f;
      }
    }
    __syncthreads();
    for (int y = ty; y < TH; y += TYS) {  // axis 1: every column of the tile and its halo along axis 2
      for (int q = tx; q < cols; q += TW) {
        double acc = 0.0;
        for (int k = 0; k <= 2 * R1; ++k) acc = acc + s_w[0][k] * (double)s_in[y + k][q];
        s_mid[y][q] = (float)acc;
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TPT; ++j) {  // axis 2
      const int y = ty + j * TYS;
      double acc = 0.0;
      for (int k = 0; k <= 2 * R2; ++k) acc = acc + s_w[1][k] * (double)s_mid[y][tx + k];
      v[j] = (float)acc;
    }
  } else {
    const float* __restrict__ in = src + plane;
#pragma unroll
    for (int j = 0; j < TPT; ++j) {
      const int gh = h0 + ty + j * TYS, gw = w0 + tx;
      v[j] = (gh < H && gw < W) ? in[(long long)gh * W + gw] : 0.0f;
    }
  }

  if (r.flags & MR_BIAS) {  // voxel o of an axis of n voxels samples the lattice at o (L - 1) / (n - 1)
    const int LLL = L * L * L;
    for (int i = threadIdx.x; i < LLL; i += MR_THREADS) s_lat[i] = lattice[(long long)n * LLL + i];
    if (threadIdx.x < TH + TW) {
      const bool row = threadIdx.x < TH;
      const int t = row ? threadIdx.x : threadIdx.x - TH;
      const int o = row ? h0 + t : w0 + t, len = row ? H : W;
      const double x = len > 1 ? (double)((long long)o * (L - 1)) / (double)(len - 1) : 0.0;
      const AxisTaps at = axis_taps(x, L, boundary::NEAREST);  // (a voxel past the axis clamps: it is never stored)
      if (row) {
        s_i1[0][t] = at.i1[0]; s_i1[1][t] = at.i1[1];
        s_w1[0][t] = at.w[0]; s_w1[1][t] = at.w[1];
      } else {
        s_i2[0][t] = at.i1[0]; s_i2[1][t] = at.i1[1];
        s_w2[0][t] = at.w[0]; s_w2[1][t] = at.w[1];
      }
    }
    __syncthreads();
    const double x0 = D > 1 ? (double)((long long)d * (L - 1)) / (double)(D - 1) : 0.0;
    const AxisTaps a0 = axis_taps(x0, L, boundary::NEAREST);
    const long long col[2] = {s_i2[0][tx], s_i2[1][tx]};
    const double wc[2] = {s_w2[0][tx], s_w2[1][tx]};
#pragma unroll
    for (int j = 0; j < TPT; ++j) {
      const int y = ty + j * TYS;
      long long rows[2][2];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) rows[a][b] = (long long)(a0.i1[a] * L + s_i1[b][y]) * L;
      const double wr[2] = {s_w1[0][y], s_w1[1][y]};
      double t[1];
      trilinear<1>(s_lat, 0, rows, col, a0.w, wr, wc, t);
      v[j] = __fmul_rn(v[j], (float)t[0]);
    }
  }

  const bool noise = (r.flags & MR_NOISE) != 0;
  float* __restrict__ out = dst + plane;
#pragma unroll
  for (int j = 0; j < TPT; ++j) {
    const int gh = h0 + ty + j * TYS, gw = w0 + tx;
    if (gh < H && gw < W) {
      float o = v[j];
      if (noise) {  // D H W < 2^32: the spatial index fits the counter word
        const unsigned index = (unsigned)(((long long)d * H + gh) * W + gw);
        o = __fadd_rn(o, __fmul_rn(mr_normal(index, (unsigned)c, r.k0, r.k1), r.std));
      }
      out[(long long)gh * W + gw] = o;
    }
  }
}

// sizes the entry point takes: positive, D H W below 2^32 (the counter word), grids within the launch limits
bool mr_sizes_ok(int N, int C, int D, int H, int W, int& rc) {
  rc = MSL_ERR_ARG;
  if (N < 1 || C < 1 || D < 1 || H < 1 || W < 1) return false;
  rc = MSL_ERR_UNSUPPORTED;
  const unsigned long long V = (unsigned long long)D * (unsigned long long)H * (unsigned long long)W;
  if (V >= (1ULL << 32)) return false;
  if ((long long)N * C > 65535) return false;
  if (V * (unsigned long long)N * (unsigned long long)C >= (1ULL << 60)) return false;
  const unsigned long long tiles = (unsigned long long)msl::cdiv(H, TH) * msl::cdiv(W, TW) * D;
  const unsigned long long hw = (unsigned long long)H * W;
  const unsigned long long cols = ((hw + MR_THREADS - 1) / MR_THREADS) * (unsigned long long)msl::cdiv(D, AX0_RUN);
  if (tiles > 0x7FFFFFFFULL || cols > 0x7FFFFFFFULL) return false;
  rc = MSL_OK;
  return true;
}

}  // namespace

extern "C" {

size_t msl_augment_mr_workspace_bytes(int N, int C, int D, int H, int W) {
  int rc;
  if (!mr_sizes_ok(N, C, D, H, W, rc)) return 0;
  return (size_t)N * C * D * H * W * sizeof(float);
}

int msl_augment_mr(const float* src, const double* params, const float* taps, const float* lattice, int N, int C, int D,
                   int H, int W, int L, float* dst, void* workspace, size_t workspace_bytes, void* stream) {
  int rc;
  if (!mr_sizes_ok(N, C, D, H, W, rc)) return rc;
  if (!src || !params || !taps || !lattice || !dst || !workspace || src == dst) return MSL_ERR_ARG;
  if (L < 2 || L > MR_LMAX) return MSL_ERR_ARG;
  if (workspace_bytes < msl_augment_mr_workspace_bytes(N, C, D, H, W)) return MSL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  float* tmp = (float*)workspace;
  const long long HW = (long long)H * W;
  const int chunks = (int)((HW + MR_THREADS - 1) / MR_THREADS);
  const dim3 grid0((unsigned)chunks * (unsigned)msl::cdiv(D, AX0_RUN), (unsigned)(N * C));
  MSL_LAUNCH(mr_axis0_kernel, grid0, dim3(MR_THREADS), 0, st, src, params, taps, C, D, HW, chunks, tmp);
  MSL_LAUNCH_CHECK();
  const int tiles_h = msl::cdiv(H, TH), tiles_w = msl::cdiv(W, TW);
  const dim3 grid1((unsigned)tiles_h * (unsigned)tiles_w * (unsigned)D, (unsigned)(N * C));
  MSL_LAUNCH(mr_tile_kernel, grid1, dim3(MR_THREADS), 0, st, src, (const float*)tmp, params, taps, lattice, C, D, H, W, L,
             tiles_h, tiles_w, dst);
  MSL_LAUNCH_CHECK();
  return MSL_OK;
}

}  // extern "C"
