// Per-tensor histograms and moments of the flat parameter arena and its twins (gradient, Adam's first moment).
// Reference: LSSD3D.on_after_backward (lesions3d/ssd3d.py:729-738), add_histogram("epoch/" + name, grads) every 25 steps.
//
// One pass over up to four flat fp32 arrays ("sources") that share one segment table: segment s = elements
// [seg_off[s], seg_off[s] + seg_len[s]) of every source = one parameter tensor.  Per (source, segment):
//   hist    128 int32 bins keyed on the fp32 BIT PATTERN (integer operations only: the counts are exact)
//             0        non-finite (NaN, +-Inf)
//             1        +-0
//             2 + c    negative finite non-zero values of magnitude class c
//             65 + c   positive finite non-zero values of magnitude class c
//           c = clamp(E - 127, -42, 20) + 42 for a normal number with biased exponent field E (floor(log2|x|) clamped to
//           [-42, 20]); a subnormal has class 0
//   moments 5 doubles over the FINITE values: sum, sum of squares, sum of magnitudes, min, max (+inf / -inf if there is none)
//
// Work split: a segment is cut into chunks of TS_CHUNK elements; a workgroup takes ONE (segment, chunk) named by a device
// table (no search) for the source blockIdx.y.  Three launches, run-to-run bit-identical:
//   1. zero the histograms                                 (the caller never clears anything)
//   2. per chunk: per-wave bin counts in LDS -> one global integer add per non-empty bin (integer adds commute);
//      fp64 moment partials of the chunk, combined in a fixed order -> workspace slot of (source, workgroup)
//   3. per (source, segment): its chunks' partials folded in a fixed order -> moments            (no floating-point atomics)
#include "common.hpp"
#include "../../include/mslesions3d_hip.h"

namespace {

constexpr int TS_BINS = MSL_TENSOR_STATS_BINS;
constexpr int TS_CHUNK = MSL_TENSOR_STATS_CHUNK;
constexpr int TS_THREADS = 256;
constexpr int TS_WAVES = TS_THREADS / 64;

struct TsSources {
  const float* p[MSL_TENSOR_STATS_MAX_SOURCES];
};

__device__ __forceinline__ int ts_bin(unsigned u) {
  const unsigned mag = u & 0x7FFFFFFFu;
  if (mag >= 0x7F800000u) return 0;  // exponent field all ones: Inf, NaN
  if (mag == 0u) return 1;
  const int e = (int)(mag >> 23);    // 0: subnormal
  const int c = e == 0 ? 0 : min(max(e - 127, -42), 20) + 42;
  return ((u >> 31) ? 2 : 65) + c;
}

struct TsAcc {
  double sum, sq, abs, lo, hi;
};

__device__ __forceinline__ void ts_take(float v, unsigned* bins, TsAcc& a) {
  const int b = ts_bin(__float_as_uint(v));
  atomicAdd(bins + b, 1u);  // LDS integer add
  if (b != 0) {
    const double d = (double)v;
    a.sum += d;
    a.sq += d * d;  // exact product of two fp32 values
    a.abs += fabs(d);
    a.lo = fmin(a.lo, d);
    a.hi = fmax(a.hi, d);
  }
}

__device__ __forceinline__ double ts_wave_min(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmin(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ double ts_wave_max(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m));
  return v;
}

__global__ __launch_bounds__(256) void tensor_stats_zero_kernel(int* __restrict__ hist, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) hist[i] = 0;
}

// table: [n_seg + 1] first workgroup of every segment (prefix sums), then per workgroup (segment, chunk)
__global__ __launch_bounds__(TS_THREADS) void tensor_stats_chunk_kernel(TsSources srcs, const long long* __restrict__ seg_off,
                                                                        const int* __restrict__ seg_len, int n_seg,
                                                                        const int* __restrict__ table, int n_blocks,
                                                                        double* __restrict__ partials, int* __restrict__ hist) {
  __shared__ unsigned bins[TS_WAVES][TS_BINS];
  __shared__ double red[TS_WAVES][5];
  const int tid = threadIdx.x, wave = tid >> 6, src = blockIdx.y;
  const int seg = table[n_seg + 1 + 2 * blockIdx.x], chunk = table[n_seg + 2 + 2 * blockIdx.x];
  const long long start = (long long)chunk * TS_CHUNK;
  const int n = (int)min((long long)TS_CHUNK, (long long)seg_len[seg] - start);
  const float* p = srcs.p[src] + seg_off[seg] + start;
  for (int i = tid; i < TS_WAVES * TS_BINS; i += TS_THREADS) (&bins[0][0])[i] = 0u;
  __syncthreads();

  TsAcc a = {0.0, 0.0, 0.0, __longlong_as_double(0x7FF0000000000000ll), __longlong_as_double(0xFFF0000000000000ull)};
  unsigned* wb = bins[wave];
  // elements in front of the first 16-byte boundary, then 16-byte loads, then what is left
  const int head = min(n, (int)((4u - (unsigned)(((uintptr_t)p >> 2) & 3u)) & 3u));
  const int nv = (n - head) >> 2, tail0 = head + 4 * nv;
  if (tid < head) ts_take(p[tid], wb, a);
  const float4* pv = reinterpret_cast<const float4*>(p + head);
  for (int i = tid; i < nv; i += TS_THREADS) {
    const float4 v = pv[i];
    ts_take(v.x, wb, a);
    ts_take(v.y, wb, a);
    ts_take(v.z, wb, a);
    ts_take(v.w, wb, a);
  }
  if (tid < n - tail0) ts_take(p[tail0 + tid], wb, a);

  // moments: lanes -> wave (fixed tree) -> workgroup (waves in index order)
  a.sum = msl::wave_sum(a.sum);
  a.sq = msl::wave_sum(a.sq);
  a.abs = msl::wave_sum(a.abs);
  a.lo = ts_wave_min(a.lo);
  a.hi = ts_wave_max(a.hi);
  if ((tid & 63) == 0) {
    red[wave][0] = a.sum; red[wave][1] = a.sq; red[wave][2] = a.abs; red[wave][3] = a.lo; red[wave][4] = a.hi;
  }
  __syncthreads();
  if (tid == 0) {
    double s = red[0][0], q = red[0][1], m = red[0][2], lo = red[0][3], hi = red[0][4];
#pragma unroll
    for (int w = 1; w < TS_WAVES; ++w) {
      s += red[w][0]; q += red[w][1]; m += red[w][2];
      lo = fmin(lo, red[w][3]);
      hi = fmax(hi, red[w][4]);
    }
    double* o = partials + ((size_t)src * n_blocks + blockIdx.x) * 5;
    o[0] = s; o[1] = q; o[2] = m; o[3] = lo; o[4] = hi;
  }
  if (tid < TS_BINS) {
    unsigned t = 0;
#pragma unroll
    for (int w = 0; w < TS_WAVES; ++w) t += bins[w][tid];
    if (t) atomicAdd(hist + ((size_t)src * n_seg + seg) * TS_BINS + tid, (int)t);
  }
}

// one wave per (segment, source): lane l adds the partials of chunks l, l + 64, ... in that order, then the wave tree
__global__ __launch_bounds__(64) void tensor_stats_fold_kernel(const int* __restrict__ table, int n_seg, int n_blocks,
                                                               const double* __restrict__ partials, double* __restrict__ moments) {
  const int seg = blockIdx.x, src = blockIdx.y, lane = threadIdx.x;
  const int b0 = table[seg], b1 = table[seg + 1];
  double s = 0.0, q = 0.0, m = 0.0, lo = __longlong_as_double(0x7FF0000000000000ll), hi = __longlong_as_double(0xFFF0000000000000ull);
  for (int b = b0 + lane; b < b1; b += 64) {
    const double* pp = partials + ((size_t)src * n_blocks + b) * 5;
    s += pp[0]; q += pp[1]; m += pp[2];
    lo = fmin(lo, pp[3]);
    hi = fmax(hi, pp[4]);
  }
  s = msl::wave_sum(s);
  q = msl::wave_sum(q);
  m = msl::wave_sum(m);
  lo = ts_wave_min(lo);
  hi = ts_wave_max(hi);
  if (lane == 0) {
    double* o = moments + ((size_t)src * n_seg + seg) * 5;
    o[0] = s; o[1] = q; o[2] = m; o[3] = lo; o[4] = hi;
  }
}

}  // namespace

extern "C" {

size_t msl_tensor_stats_chunk(void) { return (size_t)TS_CHUNK; }

// HOST arithmetic.  Number of workgroups for these segment lengths (0: a null pointer, n_seg < 1, a length < 1, or more
// than 2^24 workgroups); with host_table != NULL and capacity_ints >= n_seg + 1 + 2 * that number, also fills the table.
size_t msl_tensor_stats_block_table(const int* seg_len, int n_seg, int* host_table, size_t capacity_ints) {
  if (!seg_len || n_seg < 1) return 0;
  size_t total = 0;
  for (int s = 0; s < n_seg; ++s) {
    if (seg_len[s] < 1) return 0;
    total += ((size_t)seg_len[s] + TS_CHUNK - 1) / TS_CHUNK;
  }
  if (total > ((size_t)1 << 24)) return 0;
  if (host_table) {
    if (capacity_ints < (size_t)n_seg + 1 + 2 * total) return 0;
    int* pairs = host_table + n_seg + 1;
    int b = 0;
    for (int s = 0; s < n_seg; ++s) {
      host_table[s] = b;
      const int chunks = (int)(((size_t)seg_len[s] + TS_CHUNK - 1) / TS_CHUNK);
      for (int c = 0; c < chunks; ++c, ++b) {
        pairs[2 * b] = s;
        pairs[2 * b + 1] = c;
      }
    }
    host_table[n_seg] = b;
  }
  return total;
}

size_t msl_tensor_stats_workspace_bytes(int n_src, int n_blocks) {
  if (n_src < 1 || n_src > MSL_TENSOR_STATS_MAX_SOURCES || n_blocks < 1) return 0;
  return (size_t)n_src * n_blocks * 5 * sizeof(double);
}

int msl_tensor_stats(const float* src0, const float* src1, const float* src2, const float* src3, int n_src,
                     const long long* seg_off, const int* seg_len, int n_seg, const int* block_table, int n_blocks,
                     double* partials, int* hist, double* moments, void* stream) {
  const float* srcs[MSL_TENSOR_STATS_MAX_SOURCES] = {src0, src1, src2, src3};
  if (n_src < 1 || n_src > MSL_TENSOR_STATS_MAX_SOURCES || !seg_off || !seg_len || n_seg < 1 || n_seg > 65535 || !block_table ||
      n_blocks < n_seg || n_blocks > (1 << 24) || !partials || !hist || !moments)
    return MSL_ERR_ARG;
  if ((size_t)n_src * n_seg * TS_BINS > 0x7FFFFFFFu) return MSL_ERR_UNSUPPORTED;
  TsSources s;
  for (int k = 0; k < MSL_TENSOR_STATS_MAX_SOURCES; ++k) {
    if (k < n_src && (!srcs[k] || (uintptr_t)srcs[k] % 4 != 0)) return MSL_ERR_ARG;
    s.p[k] = k < n_src ? srcs[k] : nullptr;
  }
  if ((uintptr_t)partials % 8 != 0 || (uintptr_t)moments % 8 != 0 || (uintptr_t)hist % 4 != 0) return MSL_ERR_ARG;
  const int nh = n_src * n_seg * TS_BINS;
  hipStream_t st = (hipStream_t)stream;
  MSL_LAUNCH(tensor_stats_zero_kernel, dim3(msl::cdiv(nh, 256)), dim3(256), 0, st, hist, nh);
  MSL_LAUNCH(tensor_stats_chunk_kernel, dim3(n_blocks, n_src), dim3(TS_THREADS), 0, st, s, seg_off, seg_len, n_seg, block_table,
             n_blocks, partials, hist);
  MSL_LAUNCH(tensor_stats_fold_kernel, dim3(n_seg, n_src), dim3(64), 0, st, block_table, n_seg, n_blocks,
             (const double*)partials, moments);
  MSL_LAUNCH_CHECK();
  return MSL_OK;
}

}  // extern "C"
