// Depthwise convolution, host side: which kernel a call runs and how many fp64 partials per channel it writes.
// dw_route() is the one place that decides; every *_num_partials / _variant / _rows_ok query and every launch of dwconv.hip,
// dwconv_bwd.hip and bf16.hip reads its answer from the DwRoute it returns, so a count cannot disagree with its launch.
// Host-only arithmetic: no kernel lives here, only the limits and tile sizes the kernels are compiled for.
#pragma once
#include "common.hpp"
#include <algorithm>

namespace msl {
namespace dw {

constexpr int DW_SMALL_VOX = 512, DW_SMALL_IMG = 1024;  // small-map kernel: voxels of a map, cells of its zero-haloed LDS image
constexpr int STATS_CHUNK = 4096;                       // outputs per statistics partial of the generic forward
constexpr int BW_CHUNK = 1024;                          // outputs per work item of the generic weight gradient
constexpr int DW_TD = 2, DW_TH = 8, DW_TW = 32;         // output tile of the bf16 LDS-tiled forward / weight gradient
constexpr int DB_TD = 4, DB_TH = 8, DB_TW = 64;         // input tile of the bf16 LDS-tiled stride-2 bwd-data

enum class DwOp {
  Fwd,
  BwdDataS1,  // stride-1 bwd-data as the forward with reversed taps (w[26-k]): Wave / Resident, or None
  BwdData,    // stride 1: BwdDataS1 where a kernel takes it, else (and for stride 2) the transposed-convolution kernels
  BwdWeight,
};

enum class DwKind {
  None,
  Wave,       // planes in registers: dw_s1_wave_kernel / dw_s2_wave_kernel (+ _bww), fp32 and bf16 storage
  RowsEval,   // statistics-free forward on dw_s1_rows_eval_kernel / dw_s2_rows_eval_kernel
  SmallEval,  // statistics-free forward of a small map on dw_small_eval_kernel
  Stream,     // fp32 dw_fwd_stream_kernel (MODE 0 forward, MODE 1 weight gradient)
  Resident,   // fp32 dw_fwd_resident_kernel (MODE 0 forward / flipped forward, MODE 1 weight gradient)
  Naive,      // fp32 dw_fwd_naive_kernel (+ channel_stats_kernel)
  Tiled,      // bf16 dw_fwd_bf16_kernel (forward / flipped forward) / dw_bww_bf16_kernel
  TiledS2,    // bf16 dw_bwd_data_s2_bf16_kernel
  S2Patch,    // dw_bwd_data_s2_patch_kernel (W % 4 == 0), fp32 and bf16 storage
  DataVec,    // fp32 dw_bwd_data_kernel<1> (W % 4 == 0)
  DataNaive,  // fp32 dw_bwd_data_naive_kernel
  Chunks,     // fp32 dw_bwd_weight_kernel
};

struct DwRoute {
  DwKind kind;
  int OD, OH, OW;                    // output map of the convolution
  int logw4, logh, cpw, wpp;         // Wave: log2(W/4), log2(rows per plane), channels per wave, waves per plane (stride 2)
  int G, SLAB, nslabs;               // channels per workgroup (Stream / Resident); output planes per slab, slabs (also Wave, RowsEval)
  int ipt, lpt;                      // Stream: items and prefetch registers per thread, (1, 4) or (4, 12)
  size_t lds_bytes;                  // Stream / Resident: dynamic LDS of the launch
  int tiles_d, tiles_h, tiles_w;     // Tiled / TiledS2
  int chunks;                        // Naive (statistics) / Chunks: partials per image
  int num_partials;                  // fp64 partials per channel (statistics) or per (channel, tap) (weight gradient)
};

inline bool dw_args_ok(int N, int C, int D, int H, int W, int stride) {
  return N > 0 && C > 0 && D > 0 && H > 0 && W > 0 && (stride == 1 || stride == 2);
}

inline int pow2_floor(int v) {
  int p = 1;
  while (p * 2 <= v) p *= 2;
  return p;
}

// Register-marching wave kernels: square planes of 4 / 8 / 16 (stride 1) or 8 / 16 / 32 / 64 (stride 2; block 1's 64^2 planes
// are slower on the streamed kernel).  Two depth slabs per cube of the network's tail (NP = 2N partials per channel).
inline bool wave_plan(DwRoute& r, int N, int C, int D, int H, int W, int stride) {
  if (H != W) return false;
  if (stride == 2) {
    if (W != 8 && W != 16 && W != 32 && W != 64) return false;
    r.logw4 = W == 8 ? 1 : W == 16 ? 2 : W == 32 ? 3 : 4;
    r.logh = r.logw4 + 1;  // log2(OH)
    const int cells = (H / 2) * (W / 4), OD = (D - 1) / 2 + 1;
    r.cpw = cells >= 64 ? 1 : 64 / cells;
    r.wpp = cells >= 64 ? cells / 64 : 1;
    if (C % r.cpw != 0) return false;
    r.SLAB = OD >= 8 ? 4 : OD >= 4 ? 2 : 1;
    r.nslabs = cdiv(OD, r.SLAB);
    return (long long)N * (C / r.cpw) * r.nslabs * r.wpp <= (1ll << 30);
  }
  r.wpp = 1;
  if (stride != 1 || (W != 4 && W != 8 && W != 16)) return false;
  r.logw4 = W == 4 ? 0 : W == 8 ? 1 : 2;
  r.logh = r.logw4 + 2;
  r.cpw = 64 / (H * W / 4);
  if (C % r.cpw != 0) return false;
  r.SLAB = D >= 16 ? 8 : D >= 8 ? 4 : D >= 4 ? 2 : 1;
  r.nslabs = cdiv(D, r.SLAB);
  return (long long)N * (C / r.cpw) * r.nslabs <= (1ll << 30);
}

// eval-mode forward on the rows kernels: no statistics, planes the power-of-two wave kernels do not take
inline bool rows_eval_plan(DwRoute& r, int N, int C, int D, int H, int W, int stride) {
  if (W % 4 != 0 || W < 8 || W > 256 || D < 2) return false;
  if (stride == 2 && H % 2 != 0) return false;
  const int OD = (D - 1) / stride + 1, RPW = 64 / (W / 4);
  r.SLAB = OD >= 8 ? 4 : OD >= 4 ? 2 : 1;
  r.nslabs = cdiv(OD, r.SLAB);
  return (long long)N * C * r.nslabs * cdiv(stride == 2 ? H / 2 : H, RPW) < (1ll << 30);
}

// fp32 LDS kernels: Stream for large planes, Resident for small ones, Naive where neither fits
inline DwKind lds_plan(DwRoute& r, int N, int C, int D, int H, int W, int stride) {
  const int OD = r.OD, OH = r.OH, OW = r.OW;
  const bool fast = (W % 4 == 0) && (OW % 4 == 0) && (stride == 1 || (H % 2 == 0 && W % 2 == 0));
  if (!fast) return DwKind::Naive;
  const int RS = stride == 1 ? W + 8 : ((OW + 3) & ~3) + ((OW + 4) & ~3);
  const int PS = (H + 2) * RS;
  const int OWV = OW / 4, Lp = OH * OWV;
  constexpr int stream_min_hw = 1024;
  if (H * W >= stream_min_hw) {  // stream
    const int ipt = cdiv(Lp, 256), lpt = cdiv(H * (W / 4), 256);
    const size_t lds = std::max((size_t)PS * 4, (size_t)2 * Lp * 4);  // the plane tile, reused for the per-item statistics
    if (ipt > 4 || lpt > 12 || lds > 160 * 1024) return DwKind::Naive;
    r.G = 1;
    r.ipt = (ipt <= 1 && lpt <= 4) ? 1 : 4;  // the two instantiations: (1, 4) and (4, 12)
    r.lpt = r.ipt == 1 ? 4 : 12;
    const int slabs = std::max(1, std::min(OD, 1024 / std::max(1, N * C)));
    int SLAB = cdiv(OD, slabs);
    if (SLAB < 4) SLAB = std::min(4, OD);
    r.SLAB = SLAB;
    r.nslabs = cdiv(OD, SLAB);
    r.lds_bytes = lds;
    return DwKind::Stream;
  }
  // resident: choose SLAB (power of two dividing work) and G so that ~256..1024 items and <= 60 KB of LDS
  int SLAB = OD;
  while (SLAB > 2 && (N * C * cdiv(OD, SLAB) < 1024 || (size_t)(stride * SLAB + 2) * PS * 4 > 40 * 1024) && SLAB % 2 == 0 &&
         SLAB / 2 >= 2)
    SLAB /= 2;
  const int NPL = stride * SLAB + (stride == 2 ? 1 : 2);
  const size_t per_ch = (size_t)NPL * PS * 4 + (size_t)2 * SLAB * Lp * 4;
  if (per_ch > 150 * 1024) return DwKind::Naive;  // + 7.5 KB of static LDS
  int G = std::max(1, 256 / std::max(1, SLAB * Lp));
  G = std::min(pow2_floor(G), 64);
  while (G > 1 && (C % G != 0 || per_ch * G > 60 * 1024)) G /= 2;
  r.G = G;
  r.SLAB = SLAB;
  r.nslabs = cdiv(OD, SLAB);
  r.lds_bytes = per_ch * G;
  return DwKind::Resident;
}

inline void set_tiles(DwRoute& r, int d, int h, int w, int td, int th, int tw) {
  r.tiles_d = cdiv(d, td);
  r.tiles_h = cdiv(h, th);
  r.tiles_w = cdiv(w, tw);
}

// The route of one call.  bf16: activations stored as bf16 (bf16.hip), else fp32.  stats: the forward writes statistics
// partials (a BatchNorm fold of the input counts as training mode too).  force_naive: fp32 forward on the generic kernel.
// The caller has checked dw_args_ok where its entry point refuses bad arguments; the count queries that never did still get
// the planners' arithmetic.
inline DwRoute dw_route(DwOp op, bool bf16, int N, int C, int D, int H, int W, int stride, bool stats, bool force_naive) {
  DwRoute r{};
  if (stride <= 0 || (op == DwOp::BwdDataS1 && stride != 1)) return r;
  r.OD = (D - 1) / stride + 1;
  r.OH = (H - 1) / stride + 1;
  r.OW = (W - 1) / stride + 1;
  if (op == DwOp::BwdData) {
    if (stride == 1) {
      const DwRoute s1 = dw_route(DwOp::BwdDataS1, bf16, N, C, D, H, W, 1, false, false);
      if (s1.kind != DwKind::None) return s1;
    }
    if (!bf16) {
      r.kind = W % 4 != 0 ? DwKind::DataNaive : stride == 2 ? DwKind::S2Patch : DwKind::DataVec;
    } else if (stride == 2 && W % 4 == 0) {
      r.kind = DwKind::S2Patch;
    } else if (stride == 1) {
      r.kind = DwKind::Tiled;
      set_tiles(r, D, H, W, DW_TD, DW_TH, DW_TW);
    } else {
      r.kind = DwKind::TiledS2;
      set_tiles(r, D, H, W, DB_TD, DB_TH, DB_TW);
    }
    return r;
  }
  // (the bf16 count query has always refused bad arguments before asking for a wave plan)
  if (!force_naive && (!bf16 || dw_args_ok(N, C, D, H, W, stride)) && wave_plan(r, N, C, D, H, W, stride)) {
    r.kind = DwKind::Wave;
    r.num_partials = N * r.nslabs * (r.wpp > 4 ? r.wpp / 4 : 1);  // a split plane: one partial per workgroup of four waves
    return r;
  }
  if (op == DwOp::BwdDataS1) {
    if (!bf16 && lds_plan(r, N, C, D, H, W, 1) == DwKind::Resident) r.kind = DwKind::Resident;
    return r;
  }
  if (op == DwOp::Fwd && !force_naive && !stats) {
    if (rows_eval_plan(r, N, C, D, H, W, stride)) {
      r.kind = DwKind::RowsEval;
      return r;
    }
    if (D * H * W <= DW_SMALL_VOX && (D + 2) * (H + 2) * (W + 2) <= DW_SMALL_IMG) {
      r.kind = DwKind::SmallEval;
      return r;
    }
  }
  if (bf16) {
    r.kind = DwKind::Tiled;
    set_tiles(r, r.OD, r.OH, r.OW, DW_TD, DW_TH, DW_TW);
    r.num_partials = N * r.tiles_d * r.tiles_h * r.tiles_w;
    return r;
  }
  r.kind = force_naive ? DwKind::Naive : lds_plan(r, N, C, D, H, W, stride);
  if (op == DwOp::BwdWeight) {
    // many channels per workgroup (tiny tail volumes): the per-channel epilogue reduction dominates and the barrier-free
    // wave-per-item kernel is faster
    if (r.kind == DwKind::Naive || r.G > 4) {
      r.kind = DwKind::Chunks;
      r.chunks = cdiv(r.OD * r.OH * r.OW, BW_CHUNK);
      r.num_partials = N * r.chunks;
    } else {
      r.lds_bytes = std::max(r.lds_bytes, (size_t)27 * 256 * sizeof(float));  // the tile doubles as the [27][256] reduction buffer
      r.num_partials = N * r.nslabs;
    }
    return r;
  }
  if (r.kind == DwKind::Naive) {
    r.chunks = cdiv(r.OD * r.OH * r.OW, STATS_CHUNK);
    r.num_partials = N * r.chunks;
  } else {
    r.num_partials = N * r.nslabs;
  }
  return r;
}

}  // namespace dw
}  // namespace msl

// ---- launchers of dwconv.hip that dwconv_bwd.hip reaches (C++ linkage: not part of the C ABI); the caller owns the route --------
// fp32 weight gradient of a Wave / Stream / Resident route: partials fp64 [C*27][r.num_partials]
int dwconv_launch_bwd_weight(const msl::dw::DwRoute& r, const float* dy, const float* x, const float* in_scale,
                             const float* in_shift, double* partials, int N, int C, int D, int H, int W, int stride,
                             hipStream_t st);
// fp32 stride-1 bwd-data of a Wave / Resident route: the forward kernels on dy with the taps reversed (w[26-k])
int dwconv_launch_s1_bwd_data(const msl::dw::DwRoute& r, const float* dy, const float* w, float* g_in, int N, int C, int D, int H,
                              int W, int accumulate, hipStream_t st);
