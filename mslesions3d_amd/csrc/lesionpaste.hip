// lesionpaste: copy-paste of cached lesions on to a built training batch, in place.  Host mirror:
// datasets.paste_lesions, decision by decision.  Everything is integer arithmetic apart from the rim blend, which is two
// rounded f32 products and one rounded sum (this file is built with FMA contraction off), so both routes give the same bits.
//
//   msl_paste_lesions = one launch, one workgroup per sample.  The K pastes of a sample depend on each other (each tests
//   the mask the earlier ones left), so the workgroup walks them in order; the samples are independent.  Per paste:
//     validate : every thread checks the row (the same scalar reads in every thread, so the outcome is uniform); a refused
//                row reports -2 and writes nothing.
//     tests    : per candidate, (b) the C image voxels at the centre's destination (one broadcast read), then (a) an
//                or-reduction over the dilated destination box (at most 34^3 mask voxels, lanes consecutive along the last
//                axis) through __syncthreads_or; the walk stops at the first candidate that passes both.
//     copy     : the donor mask inside its box becomes a bit per voxel in LDS (32 x 32 words, a wave ballot per two rows,
//                already mirrored), then one thread per voxel of the dilated box decides written / rim / untouched from
//                the bits alone and writes its own voxel: no voxel is written twice, and a rim voxel reads only itself.
//     a block-scope fence and a barrier separate a paste's writes from the next paste's tests.
// No atomics.  A row can only address voxels inside its donor case and inside its sample: both are checked before any access.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int PL_THREADS = 1024;
constexpr int PL_HEAD = 13;   // ints of a row in front of its candidates
constexpr int PL_EMAX = 32;   // voxels per axis of a donor box: one LDS word per (p0, p1) row
constexpr int PL_KMAX = 8, PL_CANDMAX = 16, PL_CMAX = 4;
constexpr int PL_VALUEMAX = 32767;
static_assert(PL_EMAX == 32 && MSL_WAVE == 64, "a wave ballots two rows of 32 voxels");

__global__ __launch_bounds__(PL_THREADS) void paste_kernel(const float* __restrict__ arena_img,
                                                           const short* __restrict__ arena_seg, long long seg_elems, int C,
                                                           const long long* __restrict__ table, int n_cases,
                                                           const int* __restrict__ rows, int K, int n_cand, int T0, int T1,
                                                           int T2, float* img, short* seg, int* __restrict__ report) {
  __shared__ unsigned s_bits[PL_EMAX][PL_EMAX];
  const int n = blockIdx.x, tid = threadIdx.x;
  const long long T = (long long)T0 * T1 * T2;
  float* simg = img + (long long)n * C * T;  // (read and written here: no __restrict__, no read-only cache)
  short* sseg = seg + (long long)n * T;
  const int stride = PL_HEAD + 3 * n_cand;
  const int Ts[3] = {T0, T1, T2};

  for (int k = 0; k < K; ++k) {
    const int* __restrict__ r = rows + ((long long)n * K + k) * stride;
    // ---- validate (uniform) -------------------------------------------------------------------------------------------
    const int cs = r[1], value = r[9];
    int mn[3], e[3], cen[3], nn[3] = {1, 1, 1};
    long long off = 0;
    bool ok = r[0] != 0 && cs >= 0 && cs < n_cases && value >= 1 && value <= PL_VALUEMAX;
    if (ok) {
      off = table[4LL * cs];
      long long V = 1;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const long long v = table[4LL * cs + 1 + a];
        ok = ok && v >= 1 && v <= 0x7FFFFFFFLL && v <= seg_elems / V;  // (per factor: the product never overflows)
        nn[a] = ok ? (int)v : 1;
        V *= nn[a];
      }
      ok = ok && off >= 0 && off <= seg_elems - V;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      mn[a] = r[2 + a];
      e[a] = r[5 + a];
      cen[a] = r[10 + a];
      ok = ok && e[a] >= 1 && e[a] <= PL_EMAX && mn[a] >= 0 && mn[a] <= nn[a] - e[a] && cen[a] >= 0 && cen[a] < e[a];
    }
    if (ok)
      for (int j = 0; j < n_cand; ++j)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const int lo = r[PL_HEAD + 3 * j + a];
          ok = ok && lo >= 0 && lo <= Ts[a] - e[a];
        }
    if (!ok) {
      if (tid == 0) report[(long long)n * K + k] = -2;
      continue;
    }
    const int flips = r[8] & 7;

    // ---- the first candidate that passes (b) and (a) -----------------------------------------------------------------------
    int acc = -1, lo[3] = {0, 0, 0};
    for (int j = 0; j < n_cand && acc < 0; ++j) {
      int c[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) c[a] = r[PL_HEAD + 3 * j + a];
      const long long cv = ((long long)(c[0] + cen[0]) * T1 + (c[1] + cen[1])) * T2 + (c[2] + cen[2]);
      bool fg = true;
      for (int ch = 0; ch < C; ++ch) fg = fg && simg[ch * T + cv] != 0.0f;
      if (!fg) continue;  // (every thread read the same voxels)
      int a0[3], w[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        a0[a] = c[a] > 0 ? c[a] - 1 : 0;
        const int hi = c[a] + e[a] < Ts[a] ? c[a] + e[a] : Ts[a] - 1;
        w[a] = hi - a0[a] + 1;
      }
      const int total = w[0] * w[1] * w[2];
      int found = 0;
      for (int i = tid; i < total; i += PL_THREADS) {
        const int i2 = i % w[2], t = i / w[2], i1 = t % w[1], i0 = t / w[1];
        found |= sseg[((long long)(a0[0] + i0) * T1 + (a0[1] + i1)) * T2 + (a0[2] + i2)] != 0;
      }
      if (__syncthreads_or(found)) continue;
      acc = j;
#pragma unroll
      for (int a = 0; a < 3; ++a) lo[a] = c[a];
    }
    if (tid == 0) report[(long long)n * K + k] = acc;
    if (acc < 0) continue;

    // ---- the donor mask inside its box, mirrored, one bit per voxel -----------------------------------------------------------
    const short* __restrict__ dseg = arena_seg + off;
    const long long V = (long long)nn[0] * nn[1] * nn[2];
    const float* __restrict__ dimg = arena_img + (long long)C * off;
    const int lane = tid & 63, n_rows = e[0] * e[1];
    for (int row2 = (tid >> 6) * 2; row2 < n_rows; row2 += 2 * (PL_THREADS / 64)) {
      const int rr = row2 + (lane >> 5), p2 = lane & 31;
      const int p0 = rr / e[1], p1 = rr % e[1];
      bool b = false;
      if (rr < n_rows && p2 < e[2]) {
        const int d0 = mn[0] + ((flips & 1) ? e[0] - 1 - p0 : p0);
        const int d1 = mn[1] + ((flips & 2) ? e[1] - 1 - p1 : p1);
        const int d2 = mn[2] + ((flips & 4) ? e[2] - 1 - p2 : p2);
        b = dseg[((long long)d0 * nn[1] + d1) * nn[2] + d2] != 0;
      }
      const unsigned long long m = __ballot(b);
      if (p2 == 0 && rr < n_rows) s_bits[p0][p1] = (lane >> 5) ? (unsigned)(m >> 32) : (unsigned)m;
    }
    __syncthreads();

    // ---- one thread per voxel of the dilated box ------------------------------------------------------------------------------
    const int w0 = e[0] + 2, w1 = e[1] + 2, w2 = e[2] + 2;
    const int total = w0 * w1 * w2;
    auto bit = [&](int b0, int b1, int b2) -> bool {
      return (unsigned)b0 < (unsigned)e[0] && (unsigned)b1 < (unsigned)e[1] && (unsigned)b2 < (unsigned)e[2] &&
             ((s_bits[b0][b1] >> b2) & 1u);
    };
    for (int i = tid; i < total; i += PL_THREADS) {
      const int p2 = i % w2 - 1, t = i / w2, p1 = t % w1 - 1, p0 = t / w1 - 1;
      const int q0 = lo[0] + p0, q1 = lo[1] + p1, q2 = lo[2] + p2;
      if (q0 < 0 || q0 >= T0 || q1 < 0 || q1 >= T1 || q2 < 0 || q2 >= T2) continue;
      const long long qv = ((long long)q0 * T1 + q1) * T2 + q2;
      const int d0 = mn[0] + ((flips & 1) ? e[0] - 1 - p0 : p0);
      const int d1 = mn[1] + ((flips & 2) ? e[1] - 1 - p1 : p1);
      const int d2 = mn[2] + ((flips & 4) ? e[2] - 1 - p2 : p2);
      const long long dv = ((long long)d0 * nn[1] + d1) * nn[2] + d2;
      if (bit(p0, p1, p2)) {  // (inside the box, so inside the donor case)
        for (int ch = 0; ch < C; ++ch) simg[ch * T + qv] = dimg[ch * V + dv];
        sseg[qv] = (short)value;
      } else if (bit(p0 - 1, p1, p2) || bit(p0 + 1, p1, p2) || bit(p0, p1 - 1, p2) || bit(p0, p1 + 1, p2) ||
                 bit(p0, p1, p2 - 1) || bit(p0, p1, p2 + 1)) {
        if (d0 >= 0 && d0 < nn[0] && d1 >= 0 && d1 < nn[1] && d2 >= 0 && d2 < nn[2])
          for (int ch = 0; ch < C; ++ch)
            simg[ch * T + qv] = __fadd_rn(__fmul_rn(0.5f, simg[ch * T + qv]), __fmul_rn(0.5f, dimg[ch * V + dv]));
      }
    }
    __threadfence_block();  // this paste's voxels, before the next paste's tests read them
    __syncthreads();
  }
}

}  // namespace

extern "C" {

int msl_paste_lesions(const float* arena_img, const short* arena_seg, long long seg_elems, int C, const long long* table,
                      int n_cases, const int* rows, int N, int K, int n_cand, int T0, int T1, int T2, float* img,
                      short* seg, int* report, void* stream) {
  if (!arena_img || !arena_seg || !table || !rows || !img || !seg || !report) return MSL_ERR_ARG;
  if (seg_elems < 1 || C < 1 || n_cases < 1 || N < 1 || K < 1 || n_cand < 1 || T0 < 1 || T1 < 1 || T2 < 1) return MSL_ERR_ARG;
  if (C > PL_CMAX || K > PL_KMAX || n_cand > PL_CANDMAX) return MSL_ERR_UNSUPPORTED;
  MSL_LAUNCH(paste_kernel, dim3((unsigned)N), dim3(PL_THREADS), 0, (hipStream_t)stream, arena_img, arena_seg, seg_elems, C,
             table, n_cases, rows, K, n_cand, T0, T1, T2, img, seg, report);
  MSL_LAUNCH_CHECK();
  return MSL_OK;
}

}  // extern "C"
