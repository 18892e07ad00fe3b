// Detection metrics on the device: calculate_mAP / compute_metrics_per_class (reference lesions3d/utils.py:157-396,
// host mirror mslesions3d_amd/utils.py) for the one foreground class of the reference's task (n_classes = 2 is
// hard-coded there, utils.py:27-29, :260), on the padded detection layout that msl_detect_objects leaves behind.
//
// One workgroup (16 waves) per IoU threshold; the work is at most N * top_k detections and mostly serial:
//   compact : the class-1 detections (slot < count, label == 1) in concatenated (image, slot) order, into LDS
//   rank    : stable descending score order by counting (NaN last, ties by concatenated index) = np.lexsort's order
//   match   : one wave per image walks that image's detections in rank order; lanes cover the image's class-1 ground
//             truth in chunks of 64 with a NaN-aware first-max reduction (numpy argmax: the first NaN wins, else the
//             first maximum); TP iff IoU > thr (strict, f32) and the GT is not claimed yet
//   curve   : prefix counts of TP / FP (integers in f32: exact in any order), precision / recall curve, the 11-point
//             table, numpy's pairwise f32 mean of it, precision / recall / F1 with the host's f32 expressions
// The IoU keeps _iou_one_to_many's operation order (the one of msl_iou_matrix, multibox.hip) with FMA contraction
// off, so every output is bit-identical to the host code, NaNs included.
#include "detmetrics.hpp"
#pragma clang fp contract(off)

namespace {

constexpr int MT_THREADS = 1024;  // 16 waves
constexpr int MT_WAVES = MT_THREADS / 64;
constexpr int MT_MAXD = 4096;     // detections per batch (N * top_k)
constexpr int MT_MAXG = 4096;     // ground-truth boxes per batch
constexpr int MT_SUMMARY = 8;     // AP, mAP, precision, recall, f1, n_true_boxes, detections, TP count

using msl::Best;
using msl::block_excl_scan;
using msl::det_gt_iou;
using msl::MT_NREC;
using msl::pick;

// grid (n_thr), MT_THREADS threads
__global__ __launch_bounds__(MT_THREADS) void detection_metrics_kernel(
    const float* __restrict__ det_boxes, const float* __restrict__ det_scores, const long long* __restrict__ det_labels,
    const int* __restrict__ det_count, int N, int top_k, const float* __restrict__ gt_boxes,
    const long long* __restrict__ gt_labels, const int* __restrict__ obj_off, int G, const float* __restrict__ iou_thr,
    int n_thr, const float* __restrict__ recall_thr, float* __restrict__ summary, float* __restrict__ tp_out,
    float* __restrict__ fp_out, float* __restrict__ sorted_scores, float* __restrict__ gt_status,
    float* __restrict__ gt_vol, double* __restrict__ accum) {
  __shared__ int c_j[MT_MAXD];            // compacted detection -> concatenated slot n * top_k + s
  __shared__ float c_s[MT_MAXD];          // its score
  __shared__ int order[MT_MAXD];          // rank -> concatenated slot
  __shared__ unsigned char tpf[MT_MAXD];  // rank -> 1 = TP, 0 = FP
  __shared__ unsigned char claim[MT_MAXG];
  __shared__ int scratch[MT_WAVES];
  __shared__ float pmax[MT_WAVES][MT_NREC];
  __shared__ int n_easy_s;

  const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int D = N * top_k;
  const float thr = iou_thr[t];
  const int Gtot = min(max(obj_off[N], 0), G);

  // ---- ground truth: claims cleared, class-1 count, volumes (utils.py:152-154)
  if (tid == 0) n_easy_s = 0;
  __syncthreads();
  int easy = 0;
  for (int g = tid; g < Gtot; g += MT_THREADS) {
    claim[g] = 0;
    easy += gt_labels[g] == 1;
    if (t == 0) {
      const float* b = gt_boxes + (size_t)g * 6;
      gt_vol[g] = (b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2]);
    }
  }
  if (easy) atomicAdd(&n_easy_s, easy);  // integer count: order-independent

  // ---- compact the class-1 detections, in concatenated order
  int K = 0;
  for (int base = 0; base < D; base += MT_THREADS) {
    const int j = base + tid;
    bool valid = false;
    if (j < D) {
      const int n = j / top_k, s = j - n * top_k;
      const int cnt = min(max(det_count[n], 0), top_k);
      valid = s < cnt && det_labels[j] == 1;
    }
    int tot;
    const int pos = K + block_excl_scan<MT_WAVES>(valid ? 1 : 0, scratch, tot);
    if (valid) {
      c_j[pos] = j;
      c_s[pos] = det_scores[j];
    }
    K += tot;
  }
  __syncthreads();
  const int n_easy = n_easy_s;

  // ---- stable descending rank (np.lexsort((arange, -score)): NaN last, ties by concatenated index)
  for (int k = tid; k < K; k += MT_THREADS) {
    const float sk = c_s[k];
    int rank = 0;
    if (isnan(sk)) {
      for (int m = 0; m < K; ++m) rank += !isnan(c_s[m]) || m < k;
    } else {
      for (int m = 0; m < K; ++m) {
        const float sm = c_s[m];
        rank += (sm > sk) || (sm == sk && m < k);
      }
    }
    order[rank] = c_j[k];
    if (t == 0) sorted_scores[rank] = sk;
  }
  __syncthreads();

  // ---- greedy matching, one wave per image (compute_metrics_per_class, utils.py:157-239)
  for (int n = w; n < N; n += MT_WAVES) {
    const int lo = min(max(obj_off[n], 0), Gtot);
    const int hi = min(max(obj_off[n + 1], lo), Gtot);
    const int j0 = n * top_k, j1 = j0 + top_k;
    for (int r = 0; r < K; ++r) {
      const int j = order[r];
      if (j < j0 || j >= j1) continue;  // another image's detection (wave-uniform)
      float b[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) b[q] = det_boxes[(size_t)j * 6 + q];
      Best best = {0.f, -1};
      for (int g = lo + lane; g < hi; g += 64) {
        if (gt_labels[g] != 1) continue;
        const Best c = {det_gt_iou(b, gt_boxes + (size_t)g * 6), g};
        best = pick(best, c);
      }
      best = msl::wave_pick(best);
      if (lane == 0) {
        // no class-1 GT in the image -> FP; NaN > thr is false -> FP; a claimed GT -> FP (difficult flags are all False)
        const bool tp = best.g >= 0 && best.v > thr && claim[best.g] == 0;
        if (tp) claim[best.g] = 1;
        tpf[r] = tp ? 1 : 0;
      }
    }
  }
  __syncthreads();

  for (int g = tid; g < Gtot; g += MT_THREADS)
    gt_status[(size_t)t * G + g] = gt_labels[g] == 1 ? (claim[g] ? 1.f : 0.f) : 2.f;

  // ---- cumulative counts, precision / recall curve, 11-point table
  const int chunk = (K + MT_THREADS - 1) / MT_THREADS;
  const int r0 = min(tid * chunk, K), r1 = min(r0 + chunk, K);
  int own = 0;
  for (int r = r0; r < r1; ++r) own += tpf[r];
  int total_tp;
  int ctp = block_excl_scan<MT_WAVES>(own, scratch, total_tp);
  float pm[MT_NREC], rt[MT_NREC];
#pragma unroll
  for (int i = 0; i < MT_NREC; ++i) {
    pm[i] = 0.f;
    rt[i] = recall_thr[i];
  }  // every cprec is >= 0 and finite; "nothing above" -> 0
  float* tpo = tp_out + (size_t)t * D;
  float* fpo = fp_out + (size_t)t * D;
  for (int r = r0; r < r1; ++r) {
    const int f = tpf[r];
    ctp += f;
    tpo[r] = (float)f;
    fpo[r] = (float)(1 - f);
    const float ctpf = (float)ctp, cfpf = (float)(r + 1 - ctp);
    const float cprec = ctpf / ((ctpf + cfpf) + 1e-10f);
    const float crec = ctpf / (float)n_easy;
#pragma unroll
    for (int i = 0; i < MT_NREC; ++i)
      if (crec >= rt[i]) pm[i] = fmaxf(pm[i], cprec);
  }
#pragma unroll
  for (int i = 0; i < MT_NREC; ++i) {
    float v = pm[i];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    if (lane == 0) pmax[w][i] = v;
  }
  __syncthreads();
  if (tid != 0) return;
  float p[MT_NREC];
#pragma unroll
  for (int i = 0; i < MT_NREC; ++i) {
    float v = pmax[0][i];
    for (int k = 1; k < MT_WAVES; ++k) v = fmaxf(v, pmax[k][i]);
    p[i] = v;
  }
  float* out = summary + (size_t)t * MT_SUMMARY;
  float ap = 0.f, precision = 0.f, recall = 0.f, f1 = 0.f;
  if (K > 0) {
    ap = msl::mean11_pairwise(p);  // precs.mean(dtype=float32)
    const float tps = (float)total_tp, fps = (float)(K - total_tp), fn = (float)(n_easy - total_tp);
    recall = tps / (tps + fn);
    precision = tps / (tps + fps);
    f1 = (2.0f * precision * recall) / (precision + recall);
  }  // else utils.py:370-380: nothing detected, every value 0
  out[0] = ap;
  out[1] = ap;  // mean over the one foreground class
  out[2] = precision;
  out[3] = recall;
  out[4] = f1;
  out[5] = (float)n_easy;
  out[6] = (float)K;
  out[7] = (float)total_tp;
  if (accum) {  // per-step sums of a training epoch: [thr][mAP, precision, recall, f1] ..., steps
    double* a = accum + (size_t)t * 4;
    a[0] += (double)ap;
    a[1] += (double)precision;
    a[2] += (double)recall;
    a[3] += (double)f1;
    if (t == 0) accum[(size_t)n_thr * 4] += 1.0;
  }
}

}  // namespace

extern "C" {

// which = 0: detections per batch (N * top_k), 1: ground-truth boxes per batch, 2: IoU thresholds per launch
size_t msl_detection_metrics_max(int which) {
  return which == 0 ? (size_t)MT_MAXD : which == 1 ? (size_t)MT_MAXG : which == 2 ? (size_t)65535 : 0;
}

int msl_detection_metrics(const float* det_boxes, const float* det_scores, const long long* det_labels,
                          const int* det_count, int N, int top_k, const float* gt_boxes, const long long* gt_labels,
                          const int* obj_off, int G, const float* iou_thr, int n_thr, const float* recall_thr,
                          float* summary, float* tp, float* fp, float* sorted_scores, float* gt_status, float* gt_vol,
                          double* accum, void* stream) {
  if (N <= 0 || top_k <= 0 || G < 0 || n_thr <= 0 || !det_boxes || !det_scores || !det_labels || !det_count ||
      !obj_off || !iou_thr || !recall_thr || !summary || !tp || !fp || !sorted_scores)
    return MSL_ERR_ARG;
  if (G > 0 && (!gt_boxes || !gt_labels || !gt_status || !gt_vol)) return MSL_ERR_ARG;
  if ((long long)N * top_k > MT_MAXD || G > MT_MAXG || (size_t)n_thr > msl_detection_metrics_max(2))
    return MSL_ERR_UNSUPPORTED;
  MSL_LAUNCH(detection_metrics_kernel, dim3(n_thr), dim3(MT_THREADS), 0, (hipStream_t)stream, det_boxes, det_scores,
             det_labels, det_count, N, top_k, gt_boxes, gt_labels, obj_off, G, iou_thr, n_thr, recall_thr, summary, tp,
             fp, sorted_scores, gt_status, gt_vol, accum);
  MSL_LAUNCH_CHECK();
  return MSL_OK;
}

}  // extern "C"
