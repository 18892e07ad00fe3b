// Multi-view prediction on the device (LSSD3D.predict_views, predict.py --views tiles / --flip_views; DESIGN.md section
// 4.11).  Host mirrors: datasets.gather_views (msl_view_gather) and utils.merge_views (msl_views_merge); both are
// bit-identical to them.
//
//   gather : a view is a window of the network's input size at some origin of a ragged case, optionally mirrored along
//            some axes; outside the case it repeats the border voxel.  One thread per 16 bytes of one output row.  The
//            four-voxel chunks of a row are laid from the row's first 16-byte boundary (overlay.hip's rule), so a row of
//            any T2 at any 4-byte aligned address takes the wide store on all but its first and last chunk.  A chunk
//            whose four sources lie inside the case row reads them with one 16-byte load where that address is aligned
//            (four 4-byte loads where not: an odd origin) and, for a view flipped along W, reverses them in registers.
//            Chunks that touch the case border, the head and the tail go voxel by voxel through the clamped index.  Every
//            output voxel is written exactly once: no memset, no atomics.
//   merge  : the detections of V <= 64 views (N = V * top_k <= 8192 slots) become one list in the case frame in seven
//            launches and no host synchronisation:
//              prepare : per slot the case-frame box, its centre in case voxels, candidate or not (label, count, ownership)
//              rank    : position of every candidate in (class ascending, score descending, (view, slot) ascending) by
//                        counting from LDS tiles - exact, deterministic, no sort network (detect.hip's rule); scatter
//              mask    : 64-bit words  same class && iou6(i, j) > max_overlap  of the ranked candidates, a wave per row
//              scan    : detect.hip's greedy walk - one wave, 64 candidates per round, the rounds of a block repeated
//                        until the keep word stops changing
//              assign  : a suppressed candidate goes to the first kept one of its own mask row
//              cluster : a wave per kept candidate.  The members are found 64 at a time with a ballot and walked in rank
//                        order; lane v holds view v's best member score (V <= 64 is what makes a view a lane), so support
//                        and cover are popcounts of ballots and the score sum walks the lanes in ascending view order
//              output  : position by counting the kept candidates with a larger final score (ties: rank); top out_top_k
#include "common.hpp"
#include "../../include/mslesions3d_hip.h"
#pragma clang fp contract(off)

namespace {

#include "iou6.hpp"

constexpr int MAX_VIEWS = MSL_VIEWS_MAX;              // a view is a lane of the cluster kernel
constexpr int MAX_SLOTS = MSL_VIEWS_MAX_DETECTIONS;   // V * top_k
static_assert(MAX_VIEWS == MSL_WAVE, "cluster kernel: one lane per view");

struct ViewTab {
  int o[MAX_VIEWS][3];
  int f[MAX_VIEWS];  // bit k: mirrored along axis k
};

__device__ __forceinline__ int clampi(int x, int hi) { return min(max(x, 0), hi); }

// grid (ceil(T1 * NC / 256), C * T0, views of this launch); NC = chunks per row = ceil(T2 / 4) + 1
__global__ __launch_bounds__(256) void view_gather_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                          ViewTab tab, int C, int n0, int n1, int n2, int T0, int T1,
                                                          int T2, int NC) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T1 * NC) return;
  const int v = blockIdx.z, c = blockIdx.y / T0, p0 = blockIdx.y % T0;
  const int p1 = t / NC, ch = t % NC;
  const int fl = tab.f[v], o2 = tab.o[v][2];
  const int s0 = clampi(tab.o[v][0] + ((fl & 1) ? T0 - 1 - p0 : p0), n0 - 1);
  const int s1 = clampi(tab.o[v][1] + ((fl & 2) ? T1 - 1 - p1 : p1), n1 - 1);
  const float* srow = src + (((size_t)c * n0 + s0) * n1 + s1) * n2;
  float* drow = dst + ((((size_t)v * C + c) * T0 + p0) * T1 + p1) * T2;
  // chunk 0 is the part of the row before its first 16-byte boundary, chunk ch >= 1 covers [head + 4 (ch - 1), head + 4 ch)
  const int head = (int)(((16u - (unsigned)((uintptr_t)drow & 15u)) & 15u) >> 2);
  const int wb = ch == 0 ? 0 : head + 4 * (ch - 1);
  const int we = min(ch == 0 ? head : wb + 4, T2);
  if (wb >= we) return;
  const bool fw = (fl & 4) != 0;
  if (we - wb == 4) {  // a whole aligned chunk of the output row
    const int sl = fw ? o2 + T2 - 1 - (wb + 3) : o2 + wb;  // the lowest of its four source indices
    if (sl >= 0 && sl + 3 <= n2 - 1) {
      const float* sp = srow + sl;
      float4 x;
      if (((uintptr_t)sp & 15u) == 0) {
        x = *reinterpret_cast<const float4*>(sp);
      } else {
        x = make_float4(sp[0], sp[1], sp[2], sp[3]);
      }
      if (fw) x = make_float4(x.w, x.z, x.y, x.x);
      *reinterpret_cast<float4*>(drow + wb) = x;
      return;
    }
  }
  for (int w = wb; w < we; ++w) drow[w] = srow[clampi(o2 + (fw ? T2 - 1 - w : w), n2 - 1)];
}

// ---- merge ------------------------------------------------------------------------------------------------------------
struct MergeParams {
  ViewTab tab;
  int T[3], n[3], m[3];
  int V, K, out_top_k, mode;
  float max_overlap;
};

// the workspace: every array has one entry per slot (N = V * K); `s*` arrays are in rank order
struct MergeWs {
  unsigned long long* mask;  // N x Wn
  unsigned long long* keep;  // Wn
  long long* slabel;
  float *cbox, *ccen, *sbox, *scen, *sscore, *fbox, *fscore;
  int *ccand, *sview, *assign, *fsupport, *meta;  // meta: [candidates M, kept]
};

size_t merge_ws_carve(void* base, int N, MergeWs* w) {
  const size_t Wn = (size_t)(N + 63) / 64, n = (size_t)N;
  char* p = (char*)base;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* q = p + off;
    off += (bytes + 15) & ~(size_t)15;
    return q;
  };
  MergeWs t;
  t.mask = (unsigned long long*)take(n * Wn * 8);
  t.keep = (unsigned long long*)take(Wn * 8);
  t.slabel = (long long*)take(n * 8);
  t.cbox = (float*)take(n * 24);
  t.ccen = (float*)take(n * 12);
  t.sbox = (float*)take(n * 24);
  t.scen = (float*)take(n * 12);
  t.sscore = (float*)take(n * 4);
  t.fbox = (float*)take(n * 24);
  t.fscore = (float*)take(n * 4);
  t.ccand = (int*)take(n * 4);
  t.sview = (int*)take(n * 4);
  t.assign = (int*)take(n * 4);
  t.fsupport = (int*)take(n * 4);
  t.meta = (int*)take(16);
  if (w) *w = t;
  return off;
}

// the ownership test of a centre in case voxels by the view at origin o: a tile owns its core [o + m, o + T - m), out to the
// case border on a side where it touches it
__device__ __forceinline__ bool owns(const float* c, const int* o, const MergeParams& g) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int lo = o[k] + g.m[k], hi = o[k] + g.T[k] - g.m[k];
    ok = ok && (o[k] <= 0 || c[k] >= (float)lo) && (o[k] + g.T[k] >= g.n[k] || c[k] < (float)hi);
  }
  return ok;
}

__global__ __launch_bounds__(256) void merge_prepare_kernel(const float* __restrict__ boxes,
                                                            const float* __restrict__ scores,
                                                            const long long* __restrict__ labels,
                                                            const int* __restrict__ counts, MergeParams g, MergeWs ws) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= g.V * g.K) return;
  const int v = i / g.K, j = i % g.K;
  const float* b = boxes + (size_t)i * 6;
  float cen[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float lo = b[k], hi = b[3 + k];
    if ((g.tab.f[v] >> k) & 1) {
      const float t = lo;
      lo = 1.0f - hi;
      hi = 1.0f - t;
    }
    const float T = (float)g.T[k], o = (float)g.tab.o[v][k], n = (float)g.n[k];
    const float xl = __fadd_rn(__fmul_rn(lo, T), o), xh = __fadd_rn(__fmul_rn(hi, T), o);
    cen[k] = __fmul_rn(__fadd_rn(xl, xh), 0.5f);
    ws.cbox[(size_t)i * 6 + k] = __fdiv_rn(xl, n);
    ws.cbox[(size_t)i * 6 + 3 + k] = __fdiv_rn(xh, n);
    ws.ccen[(size_t)i * 3 + k] = cen[k];
  }
  const float s = scores[i];
  ws.ccand[i] = j < counts[v] && labels[i] >= 1 && s == s && owns(cen, g.tab.o[v], g);
}

// rank_i = #{j : j sorts in front of i} in (class ascending, score descending, slot index ascending); then scatter
__global__ __launch_bounds__(256) void merge_rank_kernel(const float* __restrict__ scores,
                                                         const long long* __restrict__ labels, int N, int K, MergeWs ws) {
  __shared__ float ts[256];
  __shared__ long long tl[256];
  __shared__ int tc[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool live = i < N;
  const bool ci = live && ws.ccand[i] != 0;
  const float si = live ? scores[i] : 0.f;
  const long long li = live ? labels[i] : 0;
  int rank = 0, total = 0;
  for (int j0 = 0; j0 < N; j0 += 256) {
    const int j = j0 + threadIdx.x;
    ts[threadIdx.x] = j < N ? scores[j] : 0.f;
    tl[threadIdx.x] = j < N ? labels[j] : 0;
    tc[threadIdx.x] = j < N ? ws.ccand[j] : 0;
    __syncthreads();
    const int lim = min(256, N - j0);
    for (int t = 0; t < lim; ++t) {
      if (!tc[t]) continue;  // wave-uniform
      ++total;
      const float sj = ts[t];
      const long long lj = tl[t];
      rank += lj < li || (lj == li && (sj > si || (sj == si && j0 + t < i)));
    }
    __syncthreads();
  }
  if (i == 0) ws.meta[0] = total;
  if (!ci) return;
#pragma unroll
  for (int k = 0; k < 6; ++k) ws.sbox[(size_t)rank * 6 + k] = ws.cbox[(size_t)i * 6 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) ws.scen[(size_t)rank * 3 + k] = ws.ccen[(size_t)i * 3 + k];
  ws.sscore[rank] = si;
  ws.slabel[rank] = li;
  ws.sview[rank] = i / K;
}

// mask[i][w] bit b: candidates i and 64 w + b are of one class and overlap.  grid ceil(N / 4), a wave per row
__global__ __launch_bounds__(256) void merge_mask_kernel(float max_overlap, int Wn, MergeWs ws) {
  const int M = ws.meta[0];
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= M) return;
  float bi[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) bi[k] = ws.sbox[(size_t)i * 6 + k];
  const long long li = ws.slabel[i];
  const int nw = (M + 63) >> 6;
  for (int w = 0; w < nw; ++w) {
    const int j = w * 64 + lane;
    bool over = false;
    if (j < M && ws.slabel[j] == li) {
      float bj[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) bj[k] = ws.sbox[(size_t)j * 6 + k];
      over = iou6(bi, bj) > max_overlap;  // strict; NaN -> false
    }
    const unsigned long long bits = __ballot(over);
    if (lane == 0) ws.mask[(size_t)i * Wn + w] = bits;
  }
}

// one wave: keep_i = !any_{j < i}(keep_j && mask[i][j]) (detect.hip's scan; the mask is bitwise symmetric)
__global__ __launch_bounds__(64) void merge_scan_kernel(int Wn, MergeWs ws) {
  __shared__ unsigned long long kf[MAX_SLOTS / 64];
  const int lane = threadIdx.x;
  const int M = ws.meta[0];
  const int nblk = (M + 63) >> 6;
  const unsigned long long lower = (1ull << lane) - 1ull;
  int cnt = 0;
  for (int blk = 0; blk < nblk; ++blk) {
    const int i = (blk << 6) + lane;
    const bool valid = i < M;
    const unsigned long long* row = ws.mask + (size_t)(valid ? i : 0) * Wn;
    bool free_ = valid;
    for (int w = 0; w < blk; ++w) free_ = free_ && (row[w] & kf[w]) == 0ull;
    const unsigned long long rb = row[blk];
    unsigned long long cur = __ballot(free_);
    for (int round = 0; round < 64; ++round) {  // wave-uniform exit
      const unsigned long long nw = __ballot(free_ && (rb & cur & lower) == 0ull);
      if (nw == cur) break;
      cur = nw;
    }
    if (lane == 0) kf[blk] = cur;  // (a wave's LDS operations execute in order: the next block's reads see it)
    if (lane == 0) ws.keep[blk] = cur;
    cnt += __popcll(cur);
  }
  if (lane == 0) ws.meta[1] = cnt;
}

__global__ __launch_bounds__(256) void merge_assign_kernel(int Wn, MergeWs ws) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int M = ws.meta[0];
  if (i >= M) return;
  int a = i;
  if (!((ws.keep[i >> 6] >> (i & 63)) & 1ull)) {
    const unsigned long long* row = ws.mask + (size_t)i * Wn;
    for (int w = 0; w <= (i >> 6); ++w) {  // a suppressed candidate has a kept one in front of it
      const unsigned long long x = row[w] & ws.keep[w];
      if (x) {
        a = w * 64 + __builtin_ctzll(x);
        break;
      }
    }
  }
  ws.assign[i] = a;
}

// grid ceil(N / 4), a wave per kept candidate k
__global__ __launch_bounds__(256) void merge_cluster_kernel(MergeParams g, MergeWs ws) {
  const int M = ws.meta[0];
  const int lane = threadIdx.x & 63, k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= M || !((ws.keep[k >> 6] >> (k & 63)) & 1ull)) return;
  const long long lab = ws.slabel[k];
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, wsum = 0.0;
  float best = 0.f;
  bool has = false;
  for (int i0 = k & ~63; i0 < M; i0 += 64) {
    if (ws.slabel[i0 > k ? i0 : k] != lab) break;  // ranked class-major: the class of k has ended
    const int i = i0 + lane;
    unsigned long long m = __ballot(i < M && i >= k && ws.assign[i] == k);
    while (m) {  // members in rank order, wave-uniform
      const int q = i0 + __builtin_ctzll(m);
      m &= m - 1ull;
      const float s = ws.sscore[q];
      if (lane == ws.sview[q]) {
        best = has ? fmaxf(best, s) : s;
        has = true;
      }
      if (g.mode == 1) {
        const double w = (double)s;
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[c] = acc[c] + w * (double)ws.sbox[(size_t)q * 6 + c];
        wsum = wsum + w;
      }
    }
  }
  const int support = __popcll(__ballot(has));
  float box[6], score;
  if (g.mode == 1) {
    float cen[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) cen[c] = ws.scen[(size_t)k * 3 + c];
    const int cover = __popcll(__ballot(lane < g.V && owns(cen, g.tab.o[lane < g.V ? lane : 0], g)));
    double total = 0.0;
    for (int v = 0; v < g.V; ++v) {
      const float bv = __shfl(best, v, 64);
      if (__shfl((int)has, v, 64)) total = total + (double)bv;
    }
    score = (float)(total / (double)max(cover, support));
#pragma unroll
    for (int c = 0; c < 6; ++c) box[c] = (float)(acc[c] / wsum);
  } else {
    score = ws.sscore[k];
#pragma unroll
    for (int c = 0; c < 6; ++c) box[c] = ws.sbox[(size_t)k * 6 + c];
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 6; ++c) ws.fbox[(size_t)k * 6 + c] = box[c];
    ws.fscore[k] = score;
    ws.fsupport[k] = support;
  }
}

__global__ __launch_bounds__(256) void merge_output_kernel(int out_top_k, MergeWs ws, float* __restrict__ out_boxes,
                                                           float* __restrict__ out_scores,
                                                           long long* __restrict__ out_labels,
                                                           int* __restrict__ out_support, int* __restrict__ out_count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int M = ws.meta[0];
  if (i == 0) out_count[0] = min(ws.meta[1], out_top_k);
  if (i >= M || !((ws.keep[i >> 6] >> (i & 63)) & 1ull)) return;
  const float si = ws.fscore[i];
  int pos = 0;
  const int nw = (M + 63) >> 6;
  for (int w = 0; w < nw; ++w) {
    unsigned long long word = ws.keep[w];
    while (word) {
      const int j = w * 64 + __builtin_ctzll(word);
      word &= word - 1ull;
      const float sj = ws.fscore[j];
      pos += sj > si || (sj == si && j < i);
    }
  }
  if (pos >= out_top_k) return;
#pragma unroll
  for (int c = 0; c < 6; ++c) out_boxes[(size_t)pos * 6 + c] = ws.fbox[(size_t)i * 6 + c];
  out_scores[pos] = si;
  out_labels[pos] = ws.slabel[i];
  out_support[pos] = ws.fsupport[i];
}

bool fill_tab(const int* views, int V, ViewTab* tab) {
  for (int v = 0; v < V; ++v) {
    int f = 0;
    for (int k = 0; k < 3; ++k) {
      const int fk = views[6 * v + 3 + k];
      if (fk != 0 && fk != 1) return false;
      f |= fk << k;
      tab->o[v][k] = views[6 * v + k];
    }
    tab->f[v] = f;
  }
  return true;
}

}  // namespace

extern "C" {

int msl_view_gather(const float* src, int C, int n0, int n1, int n2, const int* views, int V, int T0, int T1, int T2,
                    float* dst, void* stream) {
  if (!src || !views || !dst || V < 1 || C < 1 || C > 4 || n0 < 1 || n1 < 1 || n2 < 1 || T0 < 1 || T1 < 1 || T2 < 1)
    return MSL_ERR_ARG;
  if (((uintptr_t)src & 3u) || ((uintptr_t)dst & 3u)) return MSL_ERR_ARG;
  for (int v = 0; v < V; ++v)
    for (int k = 3; k < 6; ++k)
      if (views[6 * v + k] != 0 && views[6 * v + k] != 1) return MSL_ERR_ARG;
  const int NC = (T2 + 3) / 4 + 1;
  const long long per_plane = (long long)T1 * NC;
  if ((long long)C * T0 > 65535 || per_plane > 0x7FFFFFFFLL - 256) return MSL_ERR_UNSUPPORTED;
  // |origin| + tile must stay an int
  for (int v = 0; v < V; ++v)
    for (int k = 0; k < 3; ++k)
      if (views[6 * v + k] > (1 << 30) || views[6 * v + k] < -(1 << 30)) return MSL_ERR_UNSUPPORTED;
  if (T0 > (1 << 29) || T1 > (1 << 29) || T2 > (1 << 29)) return MSL_ERR_UNSUPPORTED;
  const size_t view_elems = (size_t)C * T0 * T1 * T2;
  for (int v0 = 0; v0 < V; v0 += MAX_VIEWS) {
    const int nv = V - v0 < MAX_VIEWS ? V - v0 : MAX_VIEWS;
    ViewTab tab = {};
    fill_tab(views + 6 * v0, nv, &tab);
    MSL_LAUNCH(view_gather_kernel, dim3((unsigned)((per_plane + 255) / 256), (unsigned)(C * T0), (unsigned)nv), dim3(256), 0,
               (hipStream_t)stream, src, dst + (size_t)v0 * view_elems, tab, C, n0, n1, n2, T0, T1, T2, NC);
  }
  MSL_LAUNCH_CHECK();
  return MSL_OK;
}

size_t msl_views_merge_workspace_bytes(int V, int top_k) {
  if (V < 1 || top_k < 1 || V > MAX_VIEWS || (long long)V * top_k > MAX_SLOTS) return 0;
  return merge_ws_carve(nullptr, V * top_k, nullptr);
}

int msl_views_merge(const float* boxes, const float* scores, const long long* labels, const int* counts, const int* views,
                    const int* geometry, float max_overlap, int mode, void* workspace, size_t workspace_bytes,
                    float* out_boxes, float* out_scores, long long* out_labels, int* out_support, int* out_count,
                    void* stream) {
  if (!boxes || !scores || !labels || !counts || !views || !geometry || !workspace || !out_boxes || !out_scores ||
      !out_labels || !out_support || !out_count)
    return MSL_ERR_ARG;
  MergeParams g = {};
  for (int k = 0; k < 3; ++k) {
    g.T[k] = geometry[k];
    g.n[k] = geometry[3 + k];
    g.m[k] = geometry[6 + k];
    if (g.T[k] < 1 || g.n[k] < 1 || g.m[k] < 0) return MSL_ERR_ARG;
    if (g.T[k] > (1 << 24) || g.n[k] > (1 << 24) || g.m[k] > (1 << 24)) return MSL_ERR_UNSUPPORTED;  // exact as f32
  }
  g.V = geometry[9];
  g.K = geometry[10];
  g.out_top_k = geometry[11];
  g.mode = mode;
  g.max_overlap = max_overlap;
  if (g.V < 1 || g.K < 1 || g.out_top_k < 1 || (mode != 0 && mode != 1) || ((uintptr_t)workspace & 15u)) return MSL_ERR_ARG;
  if (g.V > MAX_VIEWS || (long long)g.V * g.K > MAX_SLOTS) return MSL_ERR_UNSUPPORTED;
  if (!fill_tab(views, g.V, &g.tab)) return MSL_ERR_ARG;
  for (int v = 0; v < g.V; ++v)
    for (int k = 0; k < 3; ++k)
      if (g.tab.o[v][k] > (1 << 24) || g.tab.o[v][k] < -(1 << 24)) return MSL_ERR_UNSUPPORTED;
  const int N = g.V * g.K, Wn = (N + 63) / 64;
  MergeWs ws;
  if (workspace_bytes < merge_ws_carve(workspace, N, &ws)) return MSL_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const dim3 per_slot(msl::cdiv(N, 256)), per_row(msl::cdiv(N, 4));
  MSL_LAUNCH(merge_prepare_kernel, per_slot, dim3(256), 0, st, boxes, scores, labels, counts, g, ws);
  MSL_LAUNCH(merge_rank_kernel, per_slot, dim3(256), 0, st, scores, labels, N, g.K, ws);
  MSL_LAUNCH(merge_mask_kernel, per_row, dim3(256), 0, st, max_overlap, Wn, ws);
  MSL_LAUNCH(merge_scan_kernel, dim3(1), dim3(64), 0, st, Wn, ws);
  MSL_LAUNCH(merge_assign_kernel, per_slot, dim3(256), 0, st, Wn, ws);
  MSL_LAUNCH(merge_cluster_kernel, per_row, dim3(256), 0, st, g, ws);
  MSL_LAUNCH(merge_output_kernel, per_slot, dim3(256), 0, st, g.out_top_k, ws, out_boxes, out_scores, out_labels,
             out_support, out_count);
  MSL_LAUNCH_CHECK();
  return MSL_OK;
}

}  // extern "C"
