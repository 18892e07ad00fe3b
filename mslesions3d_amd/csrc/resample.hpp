// The sampling core of datapipe.hip's six resampling kernels (resample, affine, fit / window, warp, deform, regrid): a parameter
// row's decode, the permuted view of its source, one axis coordinate's taps, the eight-corner sum, the intensity
// operations and the four-wide store, once each.  Everything follows scipy's NI_GeometricTransform for order 1 (image) /
// order 0 (mask) operation by operation in f64, so the including file is built with FMA contraction off; the host mirror
// is devicedata._sample_numpy.  A kernel decodes its row, forms coordinates in its own way (diagonal, dense matrix,
// table lookup, step / start), calls axis_taps and trilinear, applies the operations and stores.
// Device-only; include inside the including file's own namespace, after its `#pragma clang fp contract(off)`.
#pragma once

constexpr int PARAM_STRIDE = 16;   // doubles per sample of msl_augment_resample
constexpr int AFFINE_STRIDE = 32;  // doubles per sample of msl_augment_affine
constexpr int AFFINE_MAX_OPS = 4;  // intensity operations per sample
constexpr int STORE_VEC = 4;       // output voxels along the last axis that one thread stores (store_group)

// Boundary rules, devicedata.BOUNDARY's codes and devicedata.NEAREST_UNCLAMPED.  The first three map the coordinate
// (map_boundary).  The fourth is "nearest" as scipy computes it: the taps are clamped into the axis, but the weights come
// from the coordinate as it is, so past either end both taps are the end voxel with weights (1 - x, x), not (1, 0).
// That is the clamped form's sum up to its last f64 bit, which is another f32 where the sum is a tie - and a zoom's
// tables or a regrid step of 0.5 or 2.5 are full of half-integer coordinates, which a rotation's never are.  No row
// carries it: msl_regrid always samples by it, and msl_augment_warp_mc where the row says NEAREST.
namespace boundary {
constexpr int REFLECT = 0, NEAREST = 1, CONSTANT = 2, NEAREST_UNCLAMPED = 3;
}

// ---- boundary map and taps ------------------------------------------------------------------------------------------
// scipy's map_coordinate for NI_EXTEND_REFLECT (half-sample symmetric)
__device__ __forceinline__ double map_reflect(double in, int len) {
  if (in < 0.0) {
    if (len <= 1) return 0.0;
    const long long sz2 = 2LL * len;
    if (in < (double)-sz2) in = (double)(sz2 * (long long)(-in / (double)sz2)) + in;
    in = (in < (double)-len) ? in + (double)sz2 : (in > -1e-15 ? 1e-15 : -in) - 1.0;
  } else if (in > (double)(len - 1)) {
    if (len <= 1) return 0.0;
    const long long sz2 = 2LL * len;
    in -= (double)(sz2 * (long long)(in / (double)sz2));
    if (in >= (double)len) in = ((double)sz2 - in) - 1.0;
  }
  return in;
}

// scipy's map_coordinate for the three boundaries of datasets._aug_affine: reflect, nearest ("border"), constant
// ("zeros": -1 = outside, the caller writes cval 0; a coordinate exactly on the last voxel is inside)
__device__ __forceinline__ double map_boundary(double in, int len, int mode) {
  if (mode == boundary::REFLECT) return map_reflect(in, len);
  if (mode == boundary::NEAREST) return in < 0.0 ? 0.0 : (in > (double)(len - 1) ? (double)(len - 1) : in);
  return (in < 0.0 || in > (double)(len - 1)) ? -1.0 : in;
}

// Filter taps beyond the edge: reflect maps them as the coordinate; with the other rules a tap carries weight 0 where it
// leaves the volume by one voxel at the far edge (scipy reads an in-range voxel too) or is the end voxel by the rule: clamped.
// Every source index ends inside [0, len): axis_taps hands over i in [-2, len + 1], which reflect maps into the axis.
__device__ __forceinline__ int map_tap(int i, int len, int mode) {
  if ((unsigned)i < (unsigned)len) return i;
  if (mode == boundary::REFLECT) return (int)map_reflect((double)i, len);
  return i < 0 ? 0 : len - 1;
}

struct AxisTaps {  // one axis of one coordinate: order-1 taps and weights, the order-0 tap, outside under CONSTANT
  int i1[2], i0;
  double w[2];
  bool outside;
};

// The weights come from the mapped coordinate cc as it is.  The taps floor(cc), floor(cc) + 1 and floor(cc + 0.5) come
// from cc clamped to [-2, len] as a double first (a NaN becomes -2), so the conversions are defined for every double and
// need 32 bits only (one instruction each, where a 64-bit conversion is a sequence); the upper bound stops one short of
// INT_MAX so that + 1 cannot overflow.  The bounds are integers, so that is the clamp of the floors themselves, and it
// changes no finite result: the three mapped rules leave cc in [-1, len - 1], inside the clamp; under NEAREST_UNCLAMPED
// map_tap sends every index below 0 to 0 and every index above len - 1 to len - 1, as it sends -2, -1 and len, len + 1.
__device__ __forceinline__ AxisTaps axis_taps(double c, int len, int mode) {
  AxisTaps r;
  const double cc = mode == boundary::NEAREST_UNCLAMPED ? c : map_boundary(c, len, mode);
  r.outside = mode == boundary::CONSTANT && !(cc > -1.0);
  const double x = cc - floor(cc);
  r.w[0] = 1.0 - x;
  r.w[1] = 1.0 - r.w[0];
  const double hi = (double)(len < 0x7FFFFFFE ? len : 0x7FFFFFFE);
  const double ct = !(cc >= -2.0) ? -2.0 : (cc > hi ? hi : cc);
  const int st = (int)floor(ct);
  r.i1[0] = map_tap(st, len, mode);
  r.i1[1] = map_tap(st + 1, len, mode);
  r.i0 = map_tap((int)floor(ct + 0.5), len, mode);
  return r;
}

// ---- corner sum -------------------------------------------------------------------------------------------------------
// Order-1 value of C planes (plane c at si + c * V) in f64: the eight corners in scipy's order (axis 0 slowest), each
// ((v * w0) * w1) * w2, summed in that order - bit equality with scipy rests on it.  Corner (a, b, d) lies at element
// rows[a][b] + col[d]: the tap rows of axes 0 and 1, which a wave can share, and the tap offsets along axis 2.
template <int C>
__device__ __forceinline__ void trilinear(const float* __restrict__ si, long long V, const long long (&rows)[2][2],
                                          const long long (&col)[2], const double (&w0)[2], const double (&w1)[2],
                                          const double (&w2)[2], double (&t)[C]) {
#pragma unroll
  for (int c = 0; c < C; ++c) t[c] = 0.0;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const long long s = rows[a][b] + col[d];
#pragma unroll
        for (int c = 0; c < C; ++c) {  // a channel is bit-identical to a C = 1 call on its plane
          double coeff = (double)si[c * V + s];
          coeff = coeff * w0[a];
          coeff = coeff * w1[b];
          coeff = coeff * w2[d];
          t[c] = t[c] + coeff;
        }
      }
}

// ---- row decode -------------------------------------------------------------------------------------------------------
// Every row (PARAM_STRIDE or AFFINE_STRIDE doubles) starts alike: [0] source volume / case, [1..3] source axis of output
// axes 0..2, [4..6] reversal of output axes 0..2, [7] what to sample (0: the permuted copy).  An output voxel q of the
// permutation reads source voxel s with s[axis[a]] = rev[a] ? n_a - 1 - q[a] : q[a].  msl_augment_affine's rows go on:
// [8..16] matrix M row-major, [17..19] offset, [20] boundary, [21] number of intensity operations (<= 4), [22 + 2k] kind
// (1 add, 2 multiply), [23 + 2k] f32 operand.
struct RowAxes {
  int ax[3], rev[3];
  bool ok;  // the axes are a permutation of 0, 1, 2
};

__device__ __forceinline__ RowAxes row_axes(const double* __restrict__ p) {
  RowAxes r;
  r.ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    r.ax[a] = (int)p[1 + a];
    r.rev[a] = (int)p[4 + a];
    r.ok = r.ok && r.ax[a] >= 0 && r.ax[a] < 3;
  }
  r.ok = r.ok && r.ax[0] != r.ax[1] && r.ax[0] != r.ax[2] && r.ax[1] != r.ax[2];
  return r;
}

// The source of a row seen through its permutation: planes and mask, voxels per plane, and per output axis a the length,
// the source stride (signed by the reversal) and the base they start from.  !ok: the row was rejected on the host, the
// other members are zero and the kernel writes zeros - nothing is ever read out of bounds.
template <typename Seg>
struct SrcView {
  const float* si;
  const Seg* ss;
  long long V;
  int dims[3];
  long long pst[3], base;
  bool ok;
};

template <typename Seg, typename Len>  // Len: int for a launch's own shape, long long for a table entry
__device__ __forceinline__ void view_permute(SrcView<Seg>& v, const RowAxes& r, const Len (&sn)[3]) {
  const long long sstride[3] = {(long long)sn[1] * sn[2], (long long)sn[2], 1LL};
  v.V = (long long)sn[0] * sn[1] * sn[2];
  v.base = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    v.dims[a] = (int)sn[r.ax[a]];
    v.pst[a] = r.rev[a] ? -sstride[r.ax[a]] : sstride[r.ax[a]];
    if (r.rev[a]) v.base += (long long)(v.dims[a] - 1) * sstride[r.ax[a]];
  }
}

// n_src volumes of one shape (D, H, W), which the permutation must keep
__device__ __forceinline__ SrcView<unsigned char> view_fixed(const float* __restrict__ src_img,
                                                             const unsigned char* __restrict__ src_seg, int n_src,
                                                             const double* __restrict__ p, int D, int H, int W) {
  SrcView<unsigned char> v = {};
  const RowAxes r = row_axes(p);
  const int sv = (int)p[0];
  const int sn[3] = {D, H, W};
  v.ok = r.ok && sv >= 0 && sv < n_src;
  if (v.ok) v.ok = sn[r.ax[0]] == D && sn[r.ax[1]] == H && sn[r.ax[2]] == W;
  if (v.ok) {
    view_permute(v, r, sn);
    v.si = src_img + (long long)sv * v.V;
    v.ss = src_seg + (long long)sv * v.V;
  }
  return v;
}

// Ragged cases in two arenas.  table (n_cases, 4) i64 per case: element offset into the mask arena (times C into the
// image arena, which holds the C planes of a case contiguously), shape n0, n1, n2.
template <int C>
__device__ __forceinline__ SrcView<short> view_arena(const float* __restrict__ src_img, const short* __restrict__ src_seg,
                                                     long long seg_elems, const long long* __restrict__ table,
                                                     int n_cases, const double* __restrict__ p) {
  SrcView<short> v = {};
  const RowAxes r = row_axes(p);
  const int cs = (int)p[0];
  v.ok = r.ok && cs >= 0 && cs < n_cases;
  if (v.ok) {
    const long long coff = table[(long long)cs * 4];
    long long sn[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) sn[a] = table[(long long)cs * 4 + 1 + a];
    v.ok = coff >= 0 && sn[0] > 0 && sn[1] > 0 && sn[2] > 0 && sn[0] < (1 << 20) && sn[1] < (1 << 20) && sn[2] < (1 << 20);
    // the mask ends inside its arena; the image arena holds C * seg_elems floats, so the C planes end inside theirs
    v.ok = v.ok && coff + sn[0] * sn[1] * sn[2] <= seg_elems;
    if (v.ok) {
      view_permute(v, r, sn);
      v.si = src_img + (long long)C * coff;
      v.ss = src_seg + coff;
    }
  }
  return v;
}

// The shift d of the ragged kernels on one axis: output index o of a target of t voxels reads index clamp(o + d, 0,
// dim - 1) of the permuted case.  win: the sample's window origin on that axis; null: the centred fit (pad or crop).
__device__ __forceinline__ int fit_shift(const int* __restrict__ win, int dim, int t) {
  return win ? *win : (dim < t ? -((t - dim) / 2) : dim / 2 - t / 2);
}

// A row's boundary.  Only the three mapped rules are a row's to ask for: any other value keeps map_boundary's last branch
// and is never taken for NEAREST_UNCLAMPED.
__device__ __forceinline__ int row_boundary(const double* __restrict__ p) {
  const int mode = (int)p[20];
  return mode == boundary::NEAREST_UNCLAMPED ? -1 : mode;
}

// Coordinate on axis h of voxel q under the row's dense matrix, exactly as NI_GeometricTransform forms it: cc = 0,
// cc += q[k] * M[h][k] for k = 0, 1, 2, cc += offset[h]
__device__ __forceinline__ double affine_coord(const double* __restrict__ p, const int (&q)[3], int h) {
  double c = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) c = c + (double)q[k] * p[8 + 3 * h + k];
  return c + p[17 + h];
}

// trilinear's corner offsets and the order-0 (mask) offset of three axes' taps in a view
template <typename Seg>
__device__ __forceinline__ void tap_offsets(const SrcView<Seg>& v, const AxisTaps (&t)[3], long long (&rows)[2][2],
                                            long long (&col)[2], long long& nearest) {
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int b = 0; b < 2; ++b) rows[a][b] = v.base + t[0].i1[a] * v.pst[0] + t[1].i1[b] * v.pst[1];
    col[a] = t[2].i1[a] * v.pst[2];
  }
  nearest = v.base + t[0].i0 * v.pst[0] + t[1].i0 * v.pst[1] + t[2].i0 * v.pst[2];
}

// ---- intensity operations ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float apply_ops(float v, const double* __restrict__ p) {
  const int n_ops = (int)p[21];
#pragma unroll
  for (int k = 0; k < AFFINE_MAX_OPS; ++k) {
    if (k < n_ops) {
      const float x = (float)p[23 + 2 * k];  // an f32 value stored exactly
      v = p[22 + 2 * k] == 1.0 ? __fadd_rn(v, x) : __fmul_rn(v, x);
    }
  }
  return v;
}

// ---- four-wide store ----------------------------------------------------------------------------------------------------
// The first cnt of a thread's STORE_VEC consecutive voxels: C image planes (plane c at di + c * plane) and the mask; a
// null pointer skips that output.  VEC: the group is whole and 16-byte (image, every plane) / 8-byte (mask) aligned.
template <int C, bool VEC>
__device__ __forceinline__ void store_group(const float (&vi)[C][STORE_VEC], const short (&vs)[STORE_VEC], int cnt,
                                            float* __restrict__ di, long long plane, short* __restrict__ dsg) {
  if (VEC) {
    if (di) {
#pragma unroll
      for (int c = 0; c < C; ++c)
        *reinterpret_cast<float4*>(di + c * plane) = make_float4(vi[c][0], vi[c][1], vi[c][2], vi[c][3]);
    }
    if (dsg) {
      typedef short short4v __attribute__((ext_vector_type(4)));
      short4v o;
      o[0] = vs[0]; o[1] = vs[1]; o[2] = vs[2]; o[3] = vs[3];
      *reinterpret_cast<short4v*>(dsg) = o;
    }
  } else {
#pragma unroll
    for (int j = 0; j < STORE_VEC; ++j) {  // unrolled: vi / vs stay in registers
      if (j < cnt) {
        if (di) {
#pragma unroll
          for (int c = 0; c < C; ++c) di[c * plane + j] = vi[c][j];
        }
        if (dsg) dsg[j] = vs[j];
      }
    }
  }
}
