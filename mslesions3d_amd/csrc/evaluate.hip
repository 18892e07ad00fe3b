// Dataset-scale detection metrics: the (IoU threshold x score threshold) sweep of the reference's eval.py (every grid
// point is calculate_mAP, utils.py:242-396, on the detections with score >= min_score), with no cap on detections or
// ground truth.  Host mirror: mslesions3d_amd/utils.py::calculate_mAP; Python entry: utils.evaluate_detections.
//
// The greedy matching visits detections in ONE global stable descending score order and a detection's TP / FP decision
// depends only on earlier detections of its own image.  The detections kept at a score threshold c are a prefix of that
// order (length K_c), so their TP / FP flags are the prefix of the flags of the full run, and a ground-truth box is
// "found" at c iff the rank of the detection that claimed it is < K_c.  One sort and one matching pass per IoU threshold
// therefore give every score threshold.  Stages (launch boundaries on one stream are the only hand-offs):
//   key     : 32-bit key per detection whose ascending order is descending score (-0.0 == +0.0, NaN last); detections
//             whose label is not 1 get the largest key, so the class-1 detections sort to a prefix of length K
//   rank    : stable LSD radix sort of (key, concatenated index): histogram -> scan -> stable scatter, 4 passes of 8 bits
//             -> np.lexsort((arange, -score)) of compute_metrics_per_class
//   per img : a second stable radix sort of the ranked sequence keyed by image id: each image's detections in rank order
//   match   : one wave per (image, IoU threshold) walks them; lanes cover the image's class-1 ground truth in chunks of
//             64 with the NaN-aware first max; TP iff IoU > thr (strict, f32) and the box is not claimed yet.  Per
//             ground-truth box: rank of the detection that claimed it; TP flag at the detection's rank
//   curve   : exclusive scan of the TP flags over rank (multi-block across launches); cprec with the host's f32 expression
//   sweep   : one workgroup per (IoU, score threshold): K_c by an f64 compare (retrieve_boxes compares Python floats), the
//             11-point table as range maxima of cprec over [first rank with crec >= r, K_c), AP / precision / recall / F1
// Integer counts are exact in f32 while they stay below 2^24.
//
// Ignored ground truth (msl_evaluate_detections_ign): a class-1 box with its gt_ignore byte set
// takes part in the best-IoU pick like any other, but a detection that hits it (IoU > thr) is "absorbed": neither TP nor
// FP, and the box is not claimed.  Absorbed flags live in a plane of their own beside the TP flags (abf, scanned into cab
// the way tpf is scanned into cum), so the TP scan and everything that reads it keep their arithmetic; every kernel takes
// the plane as a pointer that is null without flags and then runs the statements it has always run.  hdr[2] records
// whether the workspace carries the plane, which is how the FROC and strata consumers learn of it.
#include "detmetrics.hpp"
#pragma clang fp contract(off)

namespace {

using msl::Best;
using msl::MT_NREC;

constexpr int EV_THREADS = 256;  // 4 waves
constexpr int EV_WAVES = EV_THREADS / 64;
constexpr int EV_TILE = 4096;    // elements per workgroup of the radix passes, the scans and the curve
constexpr int EV_SUMMARY = 8;    // AP, mAP, precision, recall, f1, n_true_boxes, K_c, TP count
constexpr int EV_SCAN_ONE = 16384;     // scans up to this length run in one workgroup
constexpr int EV_MATCH_LDS_G = 16384;  // claim flags of an image with up to this many ground-truth boxes live in LDS
constexpr int NEVER = 0x7FFFFFFF;      // claim rank of an unclaimed class-1 ground-truth box
constexpr int IGNORED = -2;            // claim entry of an ignored class-1 box (-1: a box of another label)
constexpr unsigned KEY_NAN = 0xFFFFFFFEu, KEY_SKIP = 0xFFFFFFFFu;

// first index in [0, n) whose key is >= v (keys ascending)
__device__ __forceinline__ int lower_bound_u32(const unsigned* k, int n, unsigned v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (k[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int block_sum_int(int v, int* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  int s = 0;
  for (int k = 0; k < EV_WAVES; ++k) s += red[k];
  return s;
}

// max of values that are all >= 0 and finite: any combination order gives the same bits
__device__ __forceinline__ float block_max(float v, float* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float m = red[0];
  for (int k = 1; k < EV_WAVES; ++k) m = fmaxf(m, red[k]);
  return m;
}

// ---- stage 1: keys, ground-truth bookkeeping, cleared TP flags.  grid cdiv(max(D, G), EV_THREADS)
// det_rows (D,8): box(6), score, label (as f32; 1.0f iff the label is 1).  det_off (N+1): detections of image n are
// [det_off[n], det_off[n+1]).
__global__ __launch_bounds__(EV_THREADS) void ev_key_kernel(
    const float* __restrict__ det_rows, const int* __restrict__ det_off, int D, int N, const float* __restrict__ gt_boxes,
    const long long* __restrict__ gt_labels, int G, int n_iou, unsigned* __restrict__ key, int* __restrict__ val,
    int* __restrict__ img_of, int* __restrict__ tpf, int* __restrict__ claim, float* __restrict__ gt_vol,
    int* __restrict__ hdr, const unsigned char* __restrict__ gt_ignore, int* __restrict__ abf) {
  __shared__ int red[EV_WAVES];
  const int i = blockIdx.x * EV_THREADS + threadIdx.x;
  if (gt_ignore && i == 0) hdr[2] = 1;  // the workspace carries absorbed flags
  if (i < D) {
    const float s = det_rows[(size_t)i * 8 + 6];
    unsigned k;
    if (det_rows[(size_t)i * 8 + 7] != 1.0f) {
      k = KEY_SKIP;
    } else if (isnan(s)) {
      k = KEY_NAN;
    } else {
      unsigned u = __float_as_uint(s);
      if (u == 0x80000000u) u = 0u;  // -0.0 == +0.0 (the host sorts on -score)
      const unsigned asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // ascending-order bits of the float
      k = ~asc;                                                         // <= 0xFF800000 (-inf): below KEY_NAN
    }
    key[i] = k;
    val[i] = i;
    int lo = 0, hi = N;  // the image n with det_off[n] <= i < det_off[n + 1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (det_off[mid] <= i) lo = mid;
      else hi = mid;
    }
    img_of[i] = lo;
    for (int t = 0; t < n_iou; ++t) tpf[(size_t)t * D + i] = 0;
    if (gt_ignore)
      for (int t = 0; t < n_iou; ++t) abf[(size_t)t * D + i] = 0;
  }
  int easy = 0;
  if (i < G) {
    const float* b = gt_boxes + (size_t)i * 6;
    gt_vol[i] = (b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2]);  // utils.py:152-154
    const bool c1 = gt_labels[i] == 1;
    const bool ign = gt_ignore && c1 && gt_ignore[i] != 0;  // a flag on a box of another label has no effect
    easy = c1 && !ign;
    const int unclaimed = ign ? IGNORED : c1 ? NEVER : -1;
    for (int t = 0; t < n_iou; ++t) claim[(size_t)t * G + i] = unclaimed;
  }
  const int cnt = block_sum_int(easy, red);
  if (threadIdx.x == 0 && cnt) atomicAdd(&hdr[0], cnt);  // integer count: order-independent
}

// ---- radix sort: per-tile digit histogram, digit-major (hist[d * nblk + b]) so that one exclusive scan gives every
// (digit, tile) its output offset
__global__ __launch_bounds__(EV_THREADS) void ev_radix_hist_kernel(const unsigned* __restrict__ keys, int n, int shift,
                                                                   int nblk, int* __restrict__ hist) {
  __shared__ int h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int base = blockIdx.x * EV_TILE;
  for (int k = 0; k < EV_TILE / EV_THREADS; ++k) {
    const int i = base + k * EV_THREADS + threadIdx.x;
    if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255u], 1);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];
}

// stable scatter of one tile: 256 elements per step in order; a lane's rank among the lanes of its wave with the same
// digit comes from eight ballots, the waves of the step are ordered through LDS counts, steps through a running offset
__global__ __launch_bounds__(EV_THREADS) void ev_radix_scatter_kernel(
    const unsigned* __restrict__ kin, const int* __restrict__ vin, unsigned* __restrict__ kout, int* __restrict__ vout,
    int n, int shift, int nblk, const int* __restrict__ off) {
  __shared__ int cnt[EV_WAVES][256];
  __shared__ int run[256];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  run[tid] = off[(size_t)tid * nblk + blockIdx.x];
#pragma unroll
  for (int q = 0; q < EV_WAVES; ++q) cnt[q][tid] = 0;
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  const int base = blockIdx.x * EV_TILE;
  for (int k = 0; k < EV_TILE / EV_THREADS; ++k) {
    const int i0 = base + k * EV_THREADS;
    if (i0 >= n) break;  // workgroup-uniform
    const int i = i0 + tid;
    const bool valid = i < n;
    unsigned key = 0u;
    int v = 0, d = 0;
    if (valid) {
      key = kin[i];
      v = vin[i];
      d = (int)((key >> shift) & 255u);
    }
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1;
      const unsigned long long m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    const int rank = __popcll(peers & below);
    if (valid && rank == 0) cnt[w][d] = __popcll(peers);
    __syncthreads();
    {
      int o = run[tid];  // digit `tid`: offsets of the waves of this step
#pragma unroll
      for (int q = 0; q < EV_WAVES; ++q) {
        const int c = cnt[q][tid];
        cnt[q][tid] = o;
        o += c;
      }
      run[tid] = o;
    }
    __syncthreads();
    if (valid) {
      const int dst = cnt[w][d] + rank;
      kout[dst] = key;
      vout[dst] = v;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < EV_WAVES; ++q) cnt[q][tid] = 0;
    __syncthreads();
  }
}

// ---- exclusive scan of ints: per-tile sums -> one-workgroup scan of the sums -> per-tile scan with its offset
__global__ __launch_bounds__(EV_THREADS) void ev_scan_reduce_kernel(const int* __restrict__ in, int n,
                                                                    int* __restrict__ sums) {
  __shared__ int red[EV_WAVES];
  const int base = blockIdx.x * EV_TILE;
  int s = 0;
  for (int k = 0; k < EV_TILE / EV_THREADS; ++k) {
    const int i = base + k * EV_THREADS + threadIdx.x;
    if (i < n) s += in[i];
  }
  s = block_sum_int(s, red);
  if (threadIdx.x == 0) sums[blockIdx.x] = s;
}

// one workgroup of 1024 threads, any length; in == out is fine (a thread reads its element before it writes it)
__global__ __launch_bounds__(1024) void ev_scan_one_kernel(const int* in, int n, int* out) {
  __shared__ int scratch[16];
  int carry = 0;
  for (int base = 0; base < n; base += 1024) {
    const int i = base + threadIdx.x;
    const int v = i < n ? in[i] : 0;
    int tot;
    const int ex = msl::block_excl_scan<16>(v, scratch, tot);
    if (i < n) out[i] = carry + ex;
    carry += tot;
  }
}

// each thread scans 16 consecutive elements; in place is fine (a thread reads its elements before it writes them)
__global__ __launch_bounds__(EV_THREADS) void ev_scan_down_kernel(const int* in, int n, const int* __restrict__ sums,
                                                                  int* out) {
  __shared__ int scratch[EV_WAVES];
  constexpr int PER = EV_TILE / EV_THREADS;
  const int i0 = blockIdx.x * EV_TILE + threadIdx.x * PER;
  int v[PER];
  int s = 0;
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    v[q] = i0 + q < n ? in[i0 + q] : 0;
    s += v[q];
  }
  int tot;
  int run = sums[blockIdx.x] + msl::block_excl_scan<EV_WAVES>(s, scratch, tot);
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    if (i0 + q < n) out[i0 + q] = run;
    run += v[q];
  }
}

// ---- after the global sort: K, per-image keys of the ranked sequence, sorted scores (the original f32 bits)
__global__ __launch_bounds__(EV_THREADS) void ev_rank_kernel(const unsigned* __restrict__ key1, const int* __restrict__ order,
                                                             const int* __restrict__ img_of, const float* __restrict__ det_rows,
                                                             int D, int N, unsigned* __restrict__ key2, int* __restrict__ val2,
                                                             float* __restrict__ sorted_scores, int* __restrict__ hdr) {
  __shared__ int Ks;
  if (threadIdx.x == 0) {
    Ks = lower_bound_u32(key1, D, KEY_SKIP);  // class-1 detections form the prefix
    if (blockIdx.x == 0) hdr[1] = Ks;
  }
  __syncthreads();
  const int K = Ks;
  const int r = blockIdx.x * EV_THREADS + threadIdx.x;
  if (r >= D) return;
  if (r < K) {
    const int j = order[r];
    key2[r] = (unsigned)img_of[j];
    sorted_scores[r] = det_rows[(size_t)j * 8 + 6];
  } else {
    key2[r] = (unsigned)N;  // after every image
    sorted_scores[r] = 0.f;
  }
  val2[r] = r;
}

// ---- greedy matching (compute_metrics_per_class, utils.py:157-239): one wave per (image, IoU threshold).
// grid N * n_iou, 64 threads.  Detections of the image are fetched 64 at a time (one per lane) and walked serially.
__global__ __launch_bounds__(64) void ev_match_kernel(
    const float* __restrict__ det_rows, const int* __restrict__ order, const unsigned* __restrict__ img_key,
    const int* __restrict__ img_rank, int D, int N, const float* __restrict__ gt_boxes,
    const long long* __restrict__ gt_labels, const int* __restrict__ obj_off, int G, const float* __restrict__ iou_thr,
    int* __restrict__ tpf, int* __restrict__ claim, const unsigned char* __restrict__ gt_ignore, int* __restrict__ abf) {
  __shared__ unsigned char cl[EV_MATCH_LDS_G];
  const int n = blockIdx.x % N, t = blockIdx.x / N, lane = threadIdx.x;
  const int Gtot = min(max(obj_off[N], 0), G);
  const int lo = min(max(obj_off[n], 0), Gtot);
  const int hi = min(max(obj_off[n + 1], lo), Gtot);
  if (hi <= lo) return;  // no ground truth: every detection is a FP and the flags are already 0
  const int p0 = lower_bound_u32(img_key, D, (unsigned)n), p1 = lower_bound_u32(img_key, D, (unsigned)n + 1u);
  if (p0 >= p1) return;
  const float thr = iou_thr[t];
  const bool in_lds = hi - lo <= EV_MATCH_LDS_G;
  if (in_lds)
    for (int g = lane; g < hi - lo; g += 64) cl[g] = 0;
  __syncthreads();
  // the first 64 ground-truth boxes stay in registers for the whole walk
  float g0[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  bool ok0 = false;
  if (lo + lane < hi) {
    ok0 = gt_labels[lo + lane] == 1;
#pragma unroll
    for (int q = 0; q < 6; ++q) g0[q] = gt_boxes[(size_t)(lo + lane) * 6 + q];
  }
  int* clg = claim + (size_t)t * G;
  int* tp = tpf + (size_t)t * D;
  int* ab = gt_ignore ? abf + (size_t)t * D : nullptr;
  for (int pb = p0; pb < p1; pb += 64) {
    const int nb = min(64, p1 - pb);
    int r_l = 0;
    float b_l[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (lane < nb) {
      r_l = img_rank[pb + lane];
      const int j = order[r_l];
#pragma unroll
      for (int q = 0; q < 6; ++q) b_l[q] = det_rows[(size_t)j * 8 + q];
    }
    for (int k = 0; k < nb; ++k) {
      float b[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) b[q] = msl::lane_value(b_l[q], k);
      const int r = __builtin_amdgcn_readlane(r_l, k);
      Best best = {0.f, -1};
      if (ok0) best = Best{msl::det_gt_iou(b, g0), lo + lane};
      for (int g = lo + 64 + lane; g < hi; g += 64) {
        if (gt_labels[g] != 1) continue;
        const Best c = {msl::det_gt_iou(b, gt_boxes + (size_t)g * 6), g};
        best = msl::pick(best, c);
      }
      best = msl::wave_pick(best);
      // no class-1 GT in the image -> FP; NaN > thr is false -> FP; a claimed GT -> FP; an ignored GT (it took part in
      // the pick like every class-1 box) -> absorbed: flagged at the rank, nothing claimed
      if (lane == 0 && best.g >= 0 && best.v > thr) {
        const bool taken = in_lds ? cl[best.g - lo] != 0 : clg[best.g] != NEVER;
        if (ab && gt_ignore[best.g] != 0) {
          ab[r] = 1;
        } else if (!taken) {
          if (in_lds) cl[best.g - lo] = 1;
          clg[best.g] = r;
          tp[r] = 1;
        }
      }
    }
  }
}

// ---- precision curve: cprec at every rank < K, and the maximum of every tile.  grid (cdiv(D, EV_TILE), n_iou)
__global__ __launch_bounds__(EV_THREADS) void ev_curve_kernel(const int* __restrict__ tpf, const int* __restrict__ cum,
                                                              int D, const int* __restrict__ hdr, float* __restrict__ cprec,
                                                              float* __restrict__ tp_out, float* __restrict__ tile_max,
                                                              int ntile, const int* __restrict__ abf,
                                                              const int* __restrict__ cab, int* __restrict__ ab_out) {
  __shared__ float red[EV_WAVES];
  const int K = hdr[1], t = blockIdx.y;
  const size_t row = (size_t)t * D;
  const int base = cum[row];  // the scan runs over all thresholds' flags at once
  const int base_ab = abf ? cab[row] : 0;
  float m = 0.f;
  for (int k = 0; k < EV_TILE / EV_THREADS; ++k) {
    const int r = blockIdx.x * EV_TILE + k * EV_THREADS + threadIdx.x;
    if (r >= D) break;
    const int f = tpf[row + r];
    tp_out[row + r] = (float)f;
    float cp = 0.f;
    if (r < K) {
      const int ctp = cum[row + r] - base + f;
      int cfp = r + 1 - ctp;
      if (abf) cfp -= cab[row + r] - base_ab + abf[row + r];  // cfp = ranked, not TP, not absorbed
      const float ctpf = (float)ctp, cfpf = (float)cfp;
      cp = ctpf / ((ctpf + cfpf) + 1e-10f);  // utils.py: ctp / (ctp + cfp + 1e-10)
      m = fmaxf(m, cp);
    }
    cprec[row + r] = cp;
    if (abf) ab_out[row + r] = abf[row + r];
  }
  m = block_max(m, red);
  if (threadIdx.x == 0) tile_max[(size_t)t * ntile + blockIdx.x] = m;
}

// max of cprec over [a, b) (0 if empty); whole workgroup
__device__ float range_max(const float* cp, const float* tmax, int a, int b, float* red) {
  float m = 0.f;
  if (a < b) {
    const int ta = (a + EV_TILE - 1) / EV_TILE, tb = b / EV_TILE;  // whole tiles [ta, tb)
    if (ta >= tb) {
      for (int r = a + threadIdx.x; r < b; r += EV_THREADS) m = fmaxf(m, cp[r]);
    } else {
      for (int r = a + threadIdx.x; r < ta * EV_TILE; r += EV_THREADS) m = fmaxf(m, cp[r]);
      for (int q = ta + threadIdx.x; q < tb; q += EV_THREADS) m = fmaxf(m, tmax[q]);
      for (int r = tb * EV_TILE + threadIdx.x; r < b; r += EV_THREADS) m = fmaxf(m, cp[r]);
    }
  }
  return block_max(m, red);
}

// ---- one workgroup per (score threshold, IoU threshold): grid (n_sc, n_iou)
__global__ __launch_bounds__(EV_THREADS) void ev_sweep_kernel(
    const float* __restrict__ sorted_scores, const int* __restrict__ tpf, const int* __restrict__ cum,
    const float* __restrict__ cprec, const float* __restrict__ tile_max, int ntile, int D, const int* __restrict__ hdr,
    const double* __restrict__ score_thr, int n_sc, const float* __restrict__ recall_thr, float* __restrict__ summary,
    const int* __restrict__ abf, const int* __restrict__ cab, int* __restrict__ abs_out) {
  __shared__ int Kc_s, start_s[MT_NREC];
  __shared__ float red[EV_WAVES];
  const int c = blockIdx.x, t = blockIdx.y;
  const int n_easy = hdr[0], K = hdr[1];
  const size_t row = (size_t)t * D;
  const int base = cum[row];
  const float fe = (float)n_easy;
  if (threadIdx.x == 0) {
    // retrieve_boxes: keep iff score >= min_score, both as Python floats (f64).  NaN scores fail; the ranked scores
    // descend (NaN last), so the kept class-1 detections are the prefix [0, K_c)
    const double thr = score_thr[c];
    int a = 0, b = K;
    while (a < b) {
      const int mid = a + ((b - a) >> 1);
      if ((double)sorted_scores[mid] >= thr) a = mid + 1;
      else b = mid;
    }
    Kc_s = a;
  } else if (threadIdx.x <= MT_NREC) {
    // first rank with crec >= recall threshold (crec = ctp / n_easy never decreases; NaN when n_easy == 0: never)
    const float rt = recall_thr[threadIdx.x - 1];
    int a = 0, b = K;
    while (a < b) {
      const int mid = a + ((b - a) >> 1);
      const float crec = (float)(cum[row + mid] - base + tpf[row + mid]) / fe;
      if (crec >= rt) b = mid;
      else a = mid + 1;
    }
    start_s[threadIdx.x - 1] = a;
  }
  __syncthreads();
  const int Kc = Kc_s;
  float p[MT_NREC];
  for (int i = 0; i < MT_NREC; ++i) p[i] = range_max(cprec + row, tile_max + (size_t)t * ntile, start_s[i], Kc, red);
  if (threadIdx.x != 0) return;
  float ap = 0.f, precision = 0.f, recall = 0.f, f1 = 0.f;
  int tpc = 0, absc = 0;
  if (Kc > 0) {
    tpc = cum[row + Kc - 1] - base + tpf[row + Kc - 1];
    if (abf) absc = cab[row + Kc - 1] - cab[row] + abf[row + Kc - 1];
    ap = msl::mean11_pairwise(p);
    // every TP claims one ground-truth box and every claimed box has one TP: found = TP count.  Ignored boxes are not in
    // n_easy and are never claimed; an absorbed detection is no false positive
    const float tps = (float)tpc, fps = (float)(Kc - tpc - absc), fn = (float)(n_easy - tpc);
    recall = tps / (tps + fn);
    precision = tps / (tps + fps);
    f1 = (2.0f * precision * recall) / (precision + recall);
  }  // else utils.py:370-380: nothing detected, every value 0
  float* out = summary + ((size_t)t * n_sc + c) * EV_SUMMARY;
  out[0] = ap;
  out[1] = ap;  // mean over the one foreground class
  out[2] = precision;
  out[3] = recall;
  out[4] = f1;
  out[5] = (float)n_easy;
  out[6] = (float)Kc;
  out[7] = (float)tpc;
  if (abs_out) abs_out[(size_t)t * n_sc + c] = absc;
}

// ---- FROC: sensitivity at fixed numbers of false positives per image, for (R1 weight rows) x (IoU thresholds), from the
// rank order and the TP flags msl_evaluate_detections left in its workspace ("FROC").  One workgroup per
// (weights row, IoU threshold) walks the K ranked detections in tiles of EV_FROC_TILE: a thread takes EV_FROC_PER
// consecutive ranks, gathers the weight of each detection's image (the row is a few hundred bytes and stays in cache; it is
// read from global memory, so any N takes the same path), and a 64-bit workgroup scan of the (TP, FP) pair with running
// carries gives TPw(k), FPw(k) at every prefix.  FPw(k) * den <= num * Nw is tested as FPw(k) <= floor(num * Nw / den),
// computed once per rate without leaving 64 bits.  Everything is integer: the result does not depend on any order.
constexpr int EV_FROC_PER = 4;
constexpr int EV_FROC_TILE = EV_THREADS * EV_FROC_PER;  // utils.FROC_TILE
constexpr int EV_FROC_MAX_RATES = 16;                   // utils.FROC_MAX_RATES
constexpr long long EV_FROC_RATE_MAX = 1LL << 20;       // numerator and denominator of a rate
constexpr long long I64_MAX = 0x7FFFFFFFFFFFFFFFLL;

__device__ __forceinline__ long long shfl_up_i64(long long v, int o) {
  const int lo = __shfl_up((int)(v & 0xFFFFFFFFLL), o, 64), hi = __shfl_up((int)(v >> 32), o, 64);
  return ((long long)hi << 32) | (long long)(unsigned)lo;
}

__device__ __forceinline__ long long shfl_xor_i64(long long v, int o) {
  const int lo = __shfl_xor((int)(v & 0xFFFFFFFFLL), o, 64), hi = __shfl_xor((int)(v >> 32), o, 64);
  return ((long long)hi << 32) | (long long)(unsigned)lo;
}

// grid (R1, n_iou).  out: (R1, n_iou, n_rates, 2) [k*, TPw(k*)] | (R1, 2) [Gw, Nw]
__global__ __launch_bounds__(EV_THREADS) void ev_froc_kernel(
    const int* __restrict__ order, const int* __restrict__ img_of, const int* __restrict__ tpf,
    const float* __restrict__ sorted_scores, const int* __restrict__ hdr, int D, int N, const int* __restrict__ gt_count,
    const int* __restrict__ weights, const long long* __restrict__ rates, int n_rates, long long* __restrict__ out,
    const int* __restrict__ abf) {
  __shared__ long long scan_a[EV_WAVES], scan_b[EV_WAVES];
  __shared__ long long lim_s[EV_FROC_MAX_RATES];
  __shared__ long long best_tp_s[EV_WAVES][EV_FROC_MAX_RATES];
  __shared__ int best_k_s[EV_WAVES][EV_FROC_MAX_RATES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int row = blockIdx.x, t = blockIdx.y, n_iou = gridDim.y, R1 = gridDim.x;
  const int K = min(max(hdr[1], 0), D);
  const int* __restrict__ w = weights + (size_t)row * N;
  const int* __restrict__ tp = tpf + (size_t)t * D;
  const int* __restrict__ ab = (abf && hdr[2] != 0) ? abf + (size_t)t * D : nullptr;  // absorbed: no false positives

  // Gw = sum w[n] * g[n], Nw = sum w[n]
  long long gw = 0, nw = 0;
  for (int n = tid; n < N; n += EV_THREADS) {
    const long long wn = w[n];
    nw += wn;
    gw += wn * (long long)gt_count[n];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    gw += shfl_xor_i64(gw, o);
    nw += shfl_xor_i64(nw, o);
  }
  if (lane == 0) {
    scan_a[wv] = gw;
    scan_b[wv] = nw;
  }
  __syncthreads();
  gw = 0;
  nw = 0;
  for (int q = 0; q < EV_WAVES; ++q) {
    gw += scan_a[q];
    nw += scan_b[q];
  }
  if (tid < EV_FROC_MAX_RATES) {
    // floor(num * Nw / den) = num * (Nw / den) + floor(num * (Nw % den) / den); the second term stays below 2^40
    long long lim = 0;
    if (tid < n_rates) {
      const long long num = min(max(rates[2 * tid], 0LL), EV_FROC_RATE_MAX);
      const long long den = min(max(rates[2 * tid + 1], 1LL), EV_FROC_RATE_MAX);
      const long long nwp = max(nw, 0LL), qd = nwp / den, rd = nwp % den;
      lim = (num > 0 && qd > (I64_MAX - EV_FROC_RATE_MAX * EV_FROC_RATE_MAX) / num) ? I64_MAX : num * qd + (num * rd) / den;
    }
    lim_s[tid] = lim;
  }
  __syncthreads();  // lim_s written; scan_a / scan_b free again
  long long lim[EV_FROC_MAX_RATES], best_tp[EV_FROC_MAX_RATES];
  int best_k[EV_FROC_MAX_RATES];
#pragma unroll
  for (int c = 0; c < EV_FROC_MAX_RATES; ++c) {
    lim[c] = lim_s[c];
    best_tp[c] = 0;  // k = 0 always qualifies
    best_k[c] = 0;
  }

  long long carry_a = 0, carry_b = 0;
  for (int base = 0; base < K; base += EV_FROC_TILE) {  // workgroup-uniform trip count
    const int r0 = base + tid * EV_FROC_PER;
    long long a[EV_FROC_PER], b[EV_FROC_PER];
    float s[EV_FROC_PER + 1];
    long long sa = 0, sb = 0;
#pragma unroll
    for (int q = 0; q < EV_FROC_PER; ++q) {
      const int r = r0 + q;
      a[q] = 0;
      b[q] = 0;
      s[q] = 0.f;
      if (r < K) {
        const long long wi = w[img_of[order[r]]];
        if (tp[r] != 0) a[q] = wi;
        else if (ab == nullptr || ab[r] == 0) b[q] = wi;
        s[q] = sorted_scores[r];
      }
      sa += a[q];
      sb += b[q];
    }
    s[EV_FROC_PER] = r0 + EV_FROC_PER < K ? sorted_scores[r0 + EV_FROC_PER] : 0.f;
    // exclusive workgroup scan of (sa, sb)
    long long ia = sa, ib = sb;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long ua = shfl_up_i64(ia, o), ub = shfl_up_i64(ib, o);
      if (lane >= o) {
        ia += ua;
        ib += ub;
      }
    }
    __syncthreads();  // the previous tile's totals have been read
    if (lane == 63) {
      scan_a[wv] = ia;
      scan_b[wv] = ib;
    }
    __syncthreads();
    long long run_a = carry_a + ia - sa, run_b = carry_b + ib - sb;
    for (int q = 0; q < EV_WAVES; ++q) {
      const long long ta = scan_a[q], tb = scan_b[q];
      if (q < wv) {
        run_a += ta;
        run_b += tb;
      }
      carry_a += ta;
      carry_b += tb;
    }
#pragma unroll
    for (int q = 0; q < EV_FROC_PER; ++q) {
      const int k = r0 + q + 1;  // prefix length
      if (k > K) break;
      run_a += a[q];
      run_b += b[q];
      if (k == K || s[q] != s[q + 1]) {  // admissible: not inside a run of tied scores
#pragma unroll
        for (int c = 0; c < EV_FROC_MAX_RATES; ++c)
          if (c < n_rates && run_b <= lim[c]) {
            best_k[c] = k;  // ranks ascend within a thread and from tile to tile
            best_tp[c] = run_a;
          }
      }
    }
  }

  // TPw never decreases with k: TPw(k*) is the maximum over the qualifying admissible prefixes
#pragma unroll
  for (int c = 0; c < EV_FROC_MAX_RATES; ++c) {
    int k = best_k[c];
    long long v = best_tp[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      k = max(k, __shfl_xor(k, o, 64));
      v = max(v, shfl_xor_i64(v, o));
    }
    if (lane == 0) {
      best_k_s[wv][c] = k;
      best_tp_s[wv][c] = v;
    }
  }
  __syncthreads();
  if (tid < n_rates) {
    int k = 0;
    long long v = 0;
    for (int q = 0; q < EV_WAVES; ++q) {
      k = max(k, best_k_s[q][tid]);
      v = max(v, best_tp_s[q][tid]);
    }
    long long* o = out + (((size_t)row * n_iou + t) * n_rates + tid) * 2;
    o[0] = k;
    o[1] = v;
  }
  if (t == 0 && tid == 0) {
    long long* o = out + (size_t)R1 * n_iou * n_rates * 2 + (size_t)row * 2;
    o[0] = gw;
    o[1] = nw;
  }
}

// ---- strata: TPw / FPw per lesion-size bin at given cuts of the rank order ("Eval by lesion size"), the second
// read-only consumer of a completed sweep.  Two launches on the caller's stream:
//   stratify : one thread per rank and per ground-truth box: the bounding-box volume in f32 (utils.volume, this file is
//              compiled without contraction), times the voxel count of its image's frame in f64, counted against the edges
//   count    : one workgroup per (weights row, IoU threshold): the cuts are sorted in LDS; an element (a ground-truth box
//              with its claim rank, a false positive with its rank) adds its weight to the accumulator of (number of cuts
//              <= its rank, stratum); a running sum over the sorted cuts then gives every cut.  64-bit integer LDS
//              atomics: exact and order-free.
constexpr int EV_STRATA_MAX_EDGES = 15;  // utils.STRATA_MAX_EDGES
constexpr int EV_STRATA_MAX_CUTS = 32;   // utils.STRATA_MAX_CUTS
constexpr int EV_STRATA_SLOTS = EV_STRATA_MAX_EDGES + 2;  // up to 16 strata and the unbinned slot
constexpr int STRATUM_NAN = -1, STRATUM_SKIP = -2;        // NaN volume: unbinned; not class 1 / not of any image: ignored

__device__ __forceinline__ float box_volume(const float* b) {  // utils.py:152-154
  return (b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2]);
}

// number of edges <= v; NaN -> STRATUM_NAN
__device__ __forceinline__ int stratum_of(float vol, double voxels, const double* __restrict__ edges, int m) {
  const double v = (double)vol * voxels;
  if (v != v) return STRATUM_NAN;
  int s = 0;
  for (int j = 0; j < m; ++j) s += edges[j] <= v ? 1 : 0;
  return s;
}

// grid cdiv(max(D, G), EV_THREADS).  rk_img / rk_str: image and stratum of the detection at every rank < K (0 /
// STRATUM_SKIP behind K); gt_img / gt_str: the same per ground-truth box
__global__ __launch_bounds__(EV_THREADS) void ev_stratify_kernel(
    const float* __restrict__ det_rows, const int* __restrict__ order, const int* __restrict__ img_of,
    const int* __restrict__ hdr, int D, int N, const int* __restrict__ obj_off, const int* __restrict__ claim0,
    const float* __restrict__ gt_vol, int G, const double* __restrict__ voxels, const double* __restrict__ edges, int m,
    int* __restrict__ rk_img, signed char* __restrict__ rk_str, int* __restrict__ gt_img, signed char* __restrict__ gt_str) {
  const int i = blockIdx.x * EV_THREADS + threadIdx.x;
  const int K = min(max(hdr[1], 0), D);
  if (i < D) {
    int n = 0, s = STRATUM_SKIP;
    if (i < K) {
      const int d = min(max(order[i], 0), D - 1);
      n = min(max(img_of[d], 0), N - 1);
      s = stratum_of(box_volume(det_rows + (size_t)d * 8), voxels[n], edges, m);
    }
    rk_img[i] = n;
    rk_str[i] = (signed char)s;
  }
  if (i < G) {
    int lo = 0, hi = N;  // the image n with obj_off[n] <= i < obj_off[n + 1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (obj_off[mid] <= i) lo = mid;
      else hi = mid;
    }
    // class 1, not ignored (IGNORED < 0) and inside its image
    const bool counts = claim0[i] >= 0 && i >= obj_off[lo] && i < obj_off[lo + 1];
    gt_img[i] = lo;
    gt_str[i] = (signed char)(counts ? stratum_of(gt_vol[i], voxels[lo], edges, m) : STRATUM_SKIP);
  }
}

__device__ __forceinline__ void lds_add_i64(long long* p, long long v) {
  atomicAdd((unsigned long long*)p, (unsigned long long)v);
}

// number of sorted cuts <= r: an element of rank r lies inside exactly the cuts from that position on
__device__ __forceinline__ int cuts_upto(const int* sc, int n, int r) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sc[mid] <= r) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// grid (R1, n_iou).  S1 = strata + 1 (the last slot is the unbinned one).
// out: (R1, n_iou, n_cuts, S1, 2) [TPw, FPw] | (R1, S1) Gw_s | (R1, 2) [unbinned detections, Nw]
__global__ __launch_bounds__(EV_THREADS) void ev_strata_count_kernel(
    const int* __restrict__ tpf, const int* __restrict__ claim, const int* __restrict__ hdr, int D, int N, int G,
    const int* __restrict__ rk_img, const signed char* __restrict__ rk_str, const int* __restrict__ gt_img,
    const signed char* __restrict__ gt_str, const int* __restrict__ weights, const long long* __restrict__ cuts, int n_cuts,
    int S1, long long* __restrict__ out, const int* __restrict__ abf) {
  __shared__ long long acc[EV_STRATA_MAX_CUTS * EV_STRATA_SLOTS * 2];
  __shared__ long long gws[EV_STRATA_SLOTS], tail[2];
  __shared__ int raw[EV_STRATA_MAX_CUTS], sc[EV_STRATA_MAX_CUTS], pos[EV_STRATA_MAX_CUTS];
  const int tid = threadIdx.x;
  const int row = blockIdx.x, t = blockIdx.y, n_iou = gridDim.y, R1 = gridDim.x;
  const int K = min(max(hdr[1], 0), D);
  const int* __restrict__ w = weights + (size_t)row * N;
  const int cell = S1 * 2;  // accumulators of one cut interval
  for (int q = tid; q < n_cuts * cell; q += EV_THREADS) acc[q] = 0;
  if (tid < EV_STRATA_SLOTS) gws[tid] = 0;
  if (tid < 2) tail[tid] = 0;
  if (tid < n_cuts) {
    const long long c = cuts[((size_t)row * n_iou + t) * n_cuts + tid];
    raw[tid] = (int)min(max(c, 0LL), (long long)K);
  }
  __syncthreads();
  if (tid < n_cuts) {  // stable counting sort of at most 32 cuts
    const int c = raw[tid];
    int p = 0;
    for (int q = 0; q < n_cuts; ++q) p += (raw[q] < c || (raw[q] == c && q < tid)) ? 1 : 0;
    pos[tid] = p;
    sc[p] = c;
  }
  __syncthreads();
  const int top = sc[n_cuts - 1];  // the longest prefix any cut asks for
  const bool first = t == 0;       // the per-row results are written by the workgroup of the first threshold

  // ground truth: Gw_s, and TPw through the claim rank
  const int* __restrict__ cl = claim + (size_t)t * G;
  for (int g = tid; g < G; g += EV_THREADS) {
    const int s = gt_str[g];
    if (s == STRATUM_SKIP) continue;
    const long long wi = w[min(max(gt_img[g], 0), N - 1)];
    if (wi == 0) continue;
    const int slot = s < 0 ? S1 - 1 : min(s, S1 - 2);
    if (first) lds_add_i64(&gws[slot], wi);
    const int c = cl[g];
    if (c < 0) continue;
    const int i = cuts_upto(sc, n_cuts, c);  // NEVER lies behind every cut
    if (i < n_cuts) lds_add_i64(&acc[i * cell + slot * 2], wi);
  }
  // detections: FPw over the ranks below the longest cut; the first threshold also counts the unbinned ones of all K
  const int* __restrict__ tp = tpf + (size_t)t * D;
  const int* __restrict__ ab = (abf && hdr[2] != 0) ? abf + (size_t)t * D : nullptr;
  long long unb = 0, nw = 0;
  const int end = first ? K : top;
  for (int j = tid; j < end; j += EV_THREADS) {
    const int s = rk_str[j];
    const long long wi = w[min(max(rk_img[j], 0), N - 1)];
    if (wi == 0 || s == STRATUM_SKIP) continue;
    if (first && s < 0) unb += wi;
    if (j < top && tp[j] == 0 && (ab == nullptr || ab[j] == 0)) {
      const int slot = s < 0 ? S1 - 1 : min(s, S1 - 2);
      lds_add_i64(&acc[cuts_upto(sc, n_cuts, j) * cell + slot * 2 + 1], wi);
    }
  }
  if (first) {
    for (int n = tid; n < N; n += EV_THREADS) nw += w[n];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      unb += shfl_xor_i64(unb, o);
      nw += shfl_xor_i64(nw, o);
    }
    if ((tid & 63) == 0) {
      lds_add_i64(&tail[0], unb);
      lds_add_i64(&tail[1], nw);
    }
  }
  __syncthreads();
  if (tid < cell)  // running sum over the sorted cuts, one thread per (slot, TP / FP)
    for (int i = 1; i < n_cuts; ++i) acc[i * cell + tid] += acc[(i - 1) * cell + tid];
  __syncthreads();
  long long* o = out + ((size_t)row * n_iou + t) * n_cuts * cell;
  for (int q = tid; q < n_cuts * cell; q += EV_THREADS) o[q] = acc[pos[q / cell] * cell + q % cell];
  if (first) {
    long long* og = out + (size_t)R1 * n_iou * n_cuts * cell;
    if (tid < S1) og[(size_t)row * S1 + tid] = gws[tid];
    if (tid < 2) og[(size_t)R1 * S1 + (size_t)row * 2 + tid] = tail[tid];
  }
}

// ---- host planning ------------------------------------------------------------------------------------------
// Workspace hand-off (msl_evaluate_froc, msl_evaluate_strata): after a completed msl_evaluate_detections call the workspace keeps, for the
// same (D, N, G, n_iou), hdr[1] = K (class-1 detections), valA = the rank -> detection index order (the global sort ends
// in (keyA, valA) after its four passes), img_of = image of every detection index, tpf = the TP flag per (IoU threshold,
// rank).  The sorted scores, the claim ranks and the ground-truth volumes live in the caller's result buffer, not here.
// Nothing reads these after the sweep, so a consumer on the same stream may; the layout below is part of that contract.
// A call with ignore flags (msl_evaluate_detections_ign, gt_ignore not null) sets hdr[2] = 1 and keeps the absorbed flag
// per (IoU threshold, rank) in abf and its exclusive scan in cab, both BEHIND the layout of a call without flags
// (total_ign bytes in all): the consumers compute abf's address from the sizes and read it only when hdr[2] says so.
struct EvPlan {
  int nblk, ntile, radix2_passes;
  size_t hdr, keyA, keyB, keyC, valA, valB, valC, img_of, hist, sums, tpf, cum, cprec, tile_max, total;
  size_t abf, cab, total_ign;
};

inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// the sizes the pipeline may take (int32 indexing everywhere)
bool ev_supported(int D, int N, int G, int n_iou, int n_sc) {
  if (D < 0 || N <= 0 || G < 0 || n_iou <= 0 || n_sc <= 0) return false;
  const long long lim = 0x7FFFFFFFLL - EV_TILE;
  return (long long)D * 8 <= lim && (long long)n_iou * D <= lim && (long long)n_iou * G <= lim &&
         (long long)N * n_iou <= lim && N < 0x7FFFFFFF && n_iou <= 65535 && n_sc <= 0x7FFFFFFF / 8 / n_iou;
}

EvPlan ev_plan(int D, int N, int G, int n_iou) {
  EvPlan p;
  const size_t Dz = (size_t)(D > 0 ? D : 1);
  p.nblk = msl::cdiv((int)Dz, EV_TILE);
  p.ntile = p.nblk;
  int bits = 0;
  while (bits < 32 && ((unsigned)N >> bits) != 0u) ++bits;  // image keys take values 0..N
  p.radix2_passes = (bits + 7) / 8;
  const size_t scan_n = (size_t)n_iou * Dz > (size_t)256 * p.nblk ? (size_t)n_iou * Dz : (size_t)256 * p.nblk;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o = align_up(o + bytes);
    return at;
  };
  p.hdr = take(64 * sizeof(int));
  p.keyA = take(Dz * 4);
  p.keyB = take(Dz * 4);
  p.keyC = take(Dz * 4);
  p.valA = take(Dz * 4);
  p.valB = take(Dz * 4);
  p.valC = take(Dz * 4);
  p.img_of = take(Dz * 4);
  p.hist = take((size_t)256 * p.nblk * 4);
  p.sums = take(((scan_n + EV_TILE - 1) / EV_TILE) * 4);
  p.tpf = take((size_t)n_iou * Dz * 4);
  p.cum = take((size_t)n_iou * Dz * 4);
  p.cprec = take((size_t)n_iou * Dz * 4);
  p.tile_max = take((size_t)n_iou * p.ntile * 4);
  p.total = o;
  p.abf = take((size_t)n_iou * Dz * 4);
  p.cab = take((size_t)n_iou * Dz * 4);
  p.total_ign = o;
  return p;
}

// exclusive scan in -> out (in == out allowed); `sums` holds cdiv(n, EV_TILE) ints
void ev_scan(const int* in, int* out, int n, int* sums, hipStream_t st) {
  if (n <= EV_SCAN_ONE) {
    MSL_LAUNCH(ev_scan_one_kernel, dim3(1), dim3(1024), 0, st, in, n, out);
    return;
  }
  const int nb = msl::cdiv(n, EV_TILE);
  MSL_LAUNCH(ev_scan_reduce_kernel, dim3(nb), dim3(EV_THREADS), 0, st, in, n, sums);
  MSL_LAUNCH(ev_scan_one_kernel, dim3(1), dim3(1024), 0, st, (const int*)sums, nb, sums);
  MSL_LAUNCH(ev_scan_down_kernel, dim3(nb), dim3(EV_THREADS), 0, st, in, n, (const int*)sums, out);
}

// `passes` stable passes of 8 bits from bit 0 up; the result ends in (k0, v0) for an even number of passes, else (k1, v1)
void ev_radix_sort(unsigned* k0, int* v0, unsigned* k1, int* v1, int n, int passes, int nblk, int* hist, int* sums,
                   hipStream_t st) {
  for (int p = 0; p < passes; ++p) {
    MSL_LAUNCH(ev_radix_hist_kernel, dim3(nblk), dim3(EV_THREADS), 0, st, (const unsigned*)k0, n, 8 * p, nblk, hist);
    ev_scan(hist, hist, 256 * nblk, sums, st);
    MSL_LAUNCH(ev_radix_scatter_kernel, dim3(nblk), dim3(EV_THREADS), 0, st, (const unsigned*)k0, (const int*)v0, k1, v1,
               n, 8 * p, nblk, (const int*)hist);
    unsigned* tk = k0;
    k0 = k1;
    k1 = tk;
    int* tv = v0;
    v0 = v1;
    v1 = tv;
  }
}

// the sweep; gt_ignore null: the launches and the statements of a run without flags.  absorbed (i32): (n_iou, n_sc)
// absorbed detections among the first K_c ranks | (n_iou, D) absorbed flags in rank order
int ev_run(const float* det_rows, const int* det_off, int D, int N, const float* gt_boxes, const long long* gt_labels,
           const int* obj_off, int G, const float* iou_thr, int n_iou, const double* score_thr, int n_sc,
           const float* recall_thr, void* workspace, size_t workspace_bytes, float* out, const unsigned char* gt_ignore,
           int* absorbed, void* stream) {
  if (N <= 0 || D < 0 || G < 0 || n_iou <= 0 || n_sc <= 0 || !det_off || !obj_off || !iou_thr || !score_thr ||
      !recall_thr || !workspace || !out || (D > 0 && !det_rows) || (G > 0 && (!gt_boxes || !gt_labels)) ||
      (gt_ignore && !absorbed))
    return MSL_ERR_ARG;
  if (!ev_supported(D, N, G, n_iou, n_sc)) return MSL_ERR_UNSUPPORTED;
  const EvPlan p = ev_plan(D, N, G, n_iou);
  if (workspace_bytes < (gt_ignore ? p.total_ign : p.total)) return MSL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int* hdr = (int*)(ws + p.hdr);
  unsigned *kA = (unsigned*)(ws + p.keyA), *kB = (unsigned*)(ws + p.keyB), *kC = (unsigned*)(ws + p.keyC);
  int *vA = (int*)(ws + p.valA), *vB = (int*)(ws + p.valB), *vC = (int*)(ws + p.valC);
  int* img_of = (int*)(ws + p.img_of);
  int* hist = (int*)(ws + p.hist);
  int* sums = (int*)(ws + p.sums);
  int* tpf = (int*)(ws + p.tpf);
  int* cum = (int*)(ws + p.cum);
  float* cprec = (float*)(ws + p.cprec);
  float* tile_max = (float*)(ws + p.tile_max);
  // output: summary (n_iou, n_sc, 8) | sorted scores (D) | TP flags (n_iou, D) | claim rank (n_iou, G) i32 | volumes (G)
  float* summary = out;
  float* sorted_scores = summary + (size_t)n_iou * n_sc * EV_SUMMARY;
  float* tp_out = sorted_scores + D;
  int* claim = (int*)(tp_out + (size_t)n_iou * D);
  float* gt_vol = (float*)(claim + (size_t)n_iou * G);
  // without flags every one of these is null, and a kernel that sees null runs what it ran before flags existed
  int* abf = gt_ignore ? (int*)(ws + p.abf) : nullptr;
  int* cab = gt_ignore ? (int*)(ws + p.cab) : nullptr;
  int* abs_cnt = gt_ignore ? absorbed : nullptr;
  int* ab_out = gt_ignore ? absorbed + (size_t)n_iou * n_sc : nullptr;

  if (hipMemsetAsync(hdr, 0, 64 * sizeof(int), st) != hipSuccess) return (int)hipGetLastError();
  if (!gt_ignore && absorbed &&
      hipMemsetAsync(absorbed, 0, ((size_t)n_iou * n_sc + (size_t)n_iou * D) * sizeof(int), st) != hipSuccess)
    return (int)hipGetLastError();
  if (D == 0) {  // nothing detected anywhere: only the ground-truth bookkeeping and the K_c == 0 summaries
    MSL_LAUNCH(ev_key_kernel, dim3(msl::cdiv(G > 0 ? G : 1, EV_THREADS)), dim3(EV_THREADS), 0, st, det_rows, det_off, 0,
               N, gt_boxes, gt_labels, G, n_iou, kA, vA, img_of, tpf, claim, gt_vol, hdr, gt_ignore, abf);
    const float* zs = cprec;  // never read: K = 0
    MSL_LAUNCH(ev_sweep_kernel, dim3(n_sc, n_iou), dim3(EV_THREADS), 0, st, (const float*)sorted_scores, (const int*)tpf,
               (const int*)cum, zs, (const float*)tile_max, p.ntile, 1, (const int*)hdr, score_thr, n_sc, recall_thr,
               summary, (const int*)abf, (const int*)cab, abs_cnt);
    MSL_LAUNCH_CHECK();
    return MSL_OK;
  }
  const int nthreads = D > G ? D : G;
  MSL_LAUNCH(ev_key_kernel, dim3(msl::cdiv(nthreads, EV_THREADS)), dim3(EV_THREADS), 0, st, det_rows, det_off, D, N,
             gt_boxes, gt_labels, G, n_iou, kA, vA, img_of, tpf, claim, gt_vol, hdr, gt_ignore, abf);
  // global rank: 4 passes, the order ends in (kA, vA)
  ev_radix_sort(kA, vA, kB, vB, D, 4, p.nblk, hist, sums, st);
  MSL_LAUNCH(ev_rank_kernel, dim3(msl::cdiv(D, EV_THREADS)), dim3(EV_THREADS), 0, st, (const unsigned*)kA,
             (const int*)vA, (const int*)img_of, det_rows, D, N, kB, vB, sorted_scores, hdr);
  // per-image order of the ranked sequence
  ev_radix_sort(kB, vB, kC, vC, D, p.radix2_passes, p.nblk, hist, sums, st);
  const unsigned* img_key = (p.radix2_passes % 2) ? kC : kB;
  const int* img_rank = (p.radix2_passes % 2) ? vC : vB;
  MSL_LAUNCH(ev_match_kernel, dim3(N * n_iou), dim3(64), 0, st, det_rows, (const int*)vA, img_key, img_rank, D, N,
             gt_boxes, gt_labels, obj_off, G, iou_thr, tpf, claim, gt_ignore, abf);
  // cumulative TP counts of every threshold (one scan over all of them: each row subtracts its first entry)
  ev_scan(tpf, cum, n_iou * D, sums, st);
  if (gt_ignore) ev_scan(abf, cab, n_iou * D, sums, st);  // the same for the absorbed flags: the only added launches
  MSL_LAUNCH(ev_curve_kernel, dim3(p.ntile, n_iou), dim3(EV_THREADS), 0, st, (const int*)tpf, (const int*)cum, D,
             (const int*)hdr, cprec, tp_out, tile_max, p.ntile, (const int*)abf, (const int*)cab, ab_out);
  MSL_LAUNCH(ev_sweep_kernel, dim3(n_sc, n_iou), dim3(EV_THREADS), 0, st, (const float*)sorted_scores, (const int*)tpf,
             (const int*)cum, (const float*)cprec, (const float*)tile_max, p.ntile, D, (const int*)hdr, score_thr, n_sc,
             recall_thr, summary, (const int*)abf, (const int*)cab, abs_cnt);
  MSL_LAUNCH_CHECK();
  return MSL_OK;
}

}  // namespace

extern "C" {

size_t msl_evaluate_workspace_bytes(int D, int N, int G, int n_iou, int n_sc) {
  if (!ev_supported(D, N, G, n_iou, n_sc)) return 0;
  return ev_plan(D, N, G, n_iou).total;
}

size_t msl_evaluate_workspace_bytes_ign(int D, int N, int G, int n_iou, int n_sc) {
  if (!ev_supported(D, N, G, n_iou, n_sc)) return 0;
  return ev_plan(D, N, G, n_iou).total_ign;
}

int msl_evaluate_detections(const float* det_rows, const int* det_off, int D, int N, const float* gt_boxes,
                            const long long* gt_labels, const int* obj_off, int G, const float* iou_thr, int n_iou,
                            const double* score_thr, int n_sc, const float* recall_thr, void* workspace,
                            size_t workspace_bytes, float* out, void* stream) {
  return ev_run(det_rows, det_off, D, N, gt_boxes, gt_labels, obj_off, G, iou_thr, n_iou, score_thr, n_sc, recall_thr,
                workspace, workspace_bytes, out, nullptr, nullptr, stream);
}

int msl_evaluate_detections_ign(const float* det_rows, const int* det_off, int D, int N, const float* gt_boxes,
                                const long long* gt_labels, const int* obj_off, int G, const float* iou_thr, int n_iou,
                                const double* score_thr, int n_sc, const float* recall_thr, void* workspace,
                                size_t workspace_bytes, float* out, const unsigned char* gt_ignore, int* absorbed,
                                void* stream) {
  return ev_run(det_rows, det_off, D, N, gt_boxes, gt_labels, obj_off, G, iou_thr, n_iou, score_thr, n_sc, recall_thr,
                workspace, workspace_bytes, out, gt_ignore, absorbed, stream);
}

int msl_evaluate_froc(const void* eval_workspace, size_t eval_workspace_bytes, const float* sorted_scores, int D, int N,
                      int G, int n_iou, const int* gt_count, const int* weights, int R1, const long long* rates,
                      int n_rates, long long* out, void* stream) {
  if (N <= 0 || D < 0 || G < 0 || n_iou <= 0 || R1 <= 0 || n_rates <= 0 || !eval_workspace || !gt_count || !weights ||
      !rates || !out || (D > 0 && !sorted_scores))
    return MSL_ERR_ARG;
  if (n_rates > EV_FROC_MAX_RATES || !ev_supported(D, N, G, n_iou, 1)) return MSL_ERR_UNSUPPORTED;
  const EvPlan p = ev_plan(D, N, G, n_iou);
  if (eval_workspace_bytes < p.total) return MSL_ERR_ARG;
  const char* ws = (const char*)eval_workspace;
  MSL_LAUNCH(ev_froc_kernel, dim3(R1, n_iou), dim3(EV_THREADS), 0, (hipStream_t)stream, (const int*)(ws + p.valA),
             (const int*)(ws + p.img_of), (const int*)(ws + p.tpf), sorted_scores, (const int*)(ws + p.hdr), D, N, gt_count,
             weights, rates, n_rates, out, eval_workspace_bytes >= p.total_ign ? (const int*)(ws + p.abf) : nullptr);
  MSL_LAUNCH_CHECK();
  return MSL_OK;
}

int msl_evaluate_strata(const void* eval_workspace, size_t eval_workspace_bytes, const float* eval_out, int D, int N, int G,
                        int n_iou, int n_sc, const float* det_rows, const int* obj_off, const double* voxels,
                        const double* edges, int n_edges, const int* weights, int R1, const long long* cuts, int n_cuts,
                        void* strata_workspace, size_t strata_workspace_bytes, long long* out, void* stream) {
  if (N <= 0 || D < 0 || G < 0 || n_iou <= 0 || n_sc <= 0 || R1 <= 0 || n_edges <= 0 || n_cuts <= 0 || !eval_workspace ||
      !eval_out || !obj_off || !voxels || !edges || !weights || !cuts || !out || (D > 0 && !det_rows) ||
      (D + (long long)G > 0 && !strata_workspace))
    return MSL_ERR_ARG;
  if (n_edges > EV_STRATA_MAX_EDGES || n_cuts > EV_STRATA_MAX_CUTS || !ev_supported(D, N, G, n_iou, n_sc))
    return MSL_ERR_UNSUPPORTED;
  const EvPlan p = ev_plan(D, N, G, n_iou);
  if (eval_workspace_bytes < p.total || strata_workspace_bytes < 5 * ((size_t)D + (size_t)G)) return MSL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const char* ws = (const char*)eval_workspace;
  const int* hdr = (const int*)(ws + p.hdr);
  // the sweep's result buffer: summary | sorted scores (D) | TP flags (n_iou, D) | claim rank (n_iou, G) | volumes (G)
  const int* claim = (const int*)(eval_out + (size_t)n_iou * n_sc * EV_SUMMARY + D + (size_t)n_iou * D);
  const float* gt_vol = (const float*)(claim + (size_t)n_iou * G);
  // own workspace: image per rank (D) i32 | image per box (G) i32 | stratum per rank (D) i8 | stratum per box (G) i8
  int* rk_img = (int*)strata_workspace;
  int* gt_img = rk_img + D;
  signed char* rk_str = (signed char*)(gt_img + G);
  signed char* gt_str = rk_str + D;
  if (D > 0 || G > 0)
    MSL_LAUNCH(ev_stratify_kernel, dim3(msl::cdiv(D > G ? D : G, EV_THREADS)), dim3(EV_THREADS), 0, st, det_rows,
               (const int*)(ws + p.valA), (const int*)(ws + p.img_of), hdr, D, N, obj_off, claim, gt_vol, G, voxels, edges,
               n_edges, rk_img, rk_str, gt_img, gt_str);
  MSL_LAUNCH(ev_strata_count_kernel, dim3(R1, n_iou), dim3(EV_THREADS), 0, st, (const int*)(ws + p.tpf), claim, hdr, D, N, G,
             (const int*)rk_img, (const signed char*)rk_str, (const int*)gt_img, (const signed char*)gt_str, weights, cuts,
             n_cuts, n_edges + 2, out, eval_workspace_bytes >= p.total_ign ? (const int*)(ws + p.abf) : nullptr);
  MSL_LAUNCH_CHECK();
  return MSL_OK;
}

}  // extern "C"
