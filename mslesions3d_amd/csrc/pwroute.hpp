// Pointwise (1x1x1) convolution, host side: which kernel a call runs, with which template arguments and grid, and how many
// statistics partials or weight-gradient slabs it writes.  pw_route() is the one place that decides; every *_num_partials /
// _nslabs / _workspace_bytes / _batchable query and every launch of pwconv.hip, pwfused.hip and the pointwise half of bf16.hip
// reads its answer from the PwRoute it returns, so a count cannot disagree with its launch.
// Host-only arithmetic: no kernel lives here, only the tile sizes and limits the kernels are compiled for.
#pragma once
#include "common.hpp"
#include <algorithm>

namespace msl {
namespace pw {

constexpr int BM = 64, BN = 128, BK = 32;   // fp32 LDS-staged GEMM: output tile, K chunk
constexpr int WS_LD = BK + 1;               // its weight tile's LDS pitch
constexpr int FOLD_MAXK = 512;              // fp32: input channels whose (scale, shift) are kept in LDS
constexpr int KS_BM = 32, KS_BN = 64;       // fp32 K-split GEMM: output tile
constexpr int KS_WAVE_LDS = BK * KS_BN + KS_BM * WS_LD;  // its floats of LDS per wave
constexpr int SPLIT_MAX_TILES = 256;        // fewer plain 64 x 128 tiles than this: the K-split GEMM fills the chip better
constexpr int STRIP_MIN_WGS = 128;          // the strip kernels want at least this many strips
constexpr int WAVE_NT2_MIN_WAVES = 4096;    // two column tiles per wave once that still leaves >= 2 waves per SIMD
constexpr int PC = 64;                      // fp32 tile weight gradient: positions per chunk
constexpr int BWW_WAVE_WGS = 256, BWW_TILE_WGS = 512;  // workgroups the position splits of the two fp32 weight gradients aim at
constexpr int PW_BWW_BATCH_MAX = 4;         // layers of one msl_pwconv_bwd_weight_slabs_batch launch
constexpr int PB_BM = 64, PB_BN = 64, PB_BK = 32, PB_MAXK = 1024;  // bf16 plain GEMM tile; channels whose affine is kept in LDS
constexpr int PT_BM = 64, PT_BN = 64;       // bf16 transposed-read GEMM tile
constexpr int PT_WGS = 512;                 // ... several position tiles per workgroup above this many workgroups
constexpr int BF_BWW_WGS = 256;             // workgroups the bf16 MFMA weight gradient's position split aims at
constexpr int FUSED_K = 64, FUSED_M = 32, FUSED_COLS = 128;  // one-pass backward of block 1: Cout, Cin, positions per strip
constexpr int FUSED_MIN_STRIPS = 512, FUSED_WGS = 256;       // smaller layers are latency-bound; workgroups = partials = slabs

// (K, COLS, MT) of the five pw_strip_kernel instantiations (M = 32 MT) and (KW, MT, NWK, NT) of the eleven pw_wave_kernel ones:
// closed lists, a launcher dispatches over PwRoute::form
constexpr int STRIP_FORMS[5][3] = {{32, 256, 2}, {64, 128, 1}, {64, 64, 4}, {128, 64, 4}, {128, 64, 2}};
constexpr int WAVE_FORMS[11][4] = {{32, 1, 1, 1}, {32, 1, 1, 2}, {32, 2, 1, 1}, {32, 2, 1, 2}, {64, 1, 1, 1}, {64, 1, 1, 2},
                                   {64, 2, 1, 1}, {64, 2, 1, 2}, {64, 1, 2, 1}, {64, 1, 4, 1}, {64, 1, 8, 1}};

enum class PwOp { Fwd, BwdData, BwdWeight, BwdFused };

enum class PwKind {
  None,
  Strip,        // fp32 pw_strip_kernel: forward / bwd-data GEMMs of blocks 1-3
  Wave,         // fp32 pw_wave_kernel: K = 32 | 64 (one or two column tiles per wave) or K = 128 | 256 | 512 split over K / 64 waves
  KSplit,       // fp32 pw_gemm_ksplit_kernel: 4 or 8 waves split K, tail layers
  Gemm,         // fp32 pw_gemm_kernel: every other shape
  BwwWave,      // fp32 pw_bww_wave_kernel (the batched launch runs the same body)
  BwwTile,      // fp32 pw_bwd_weight_kernel
  Bf16Tr,       // pw_bf16_tr_kernel: whole 8-position groups, K in whole chunks
  Bf16Plain,    // pw_fwd_bf16_kernel
  Bf16BwwMfma,  // pw_bww_bf16_kernel
  Bf16BwwAny,   // pw_bww_bf16_any_kernel: one slab
  Fused,        // pw_bwd_fused_kernel (pwfused.hip)
};

struct PwRoute {
  PwKind kind;
  int M, K;            // Fwd / BwdData: rows and depth of the GEMM - (Cout, Cin) forward, (Cin, Cout) on transposed weights backward
  int form;            // Strip: index into STRIP_FORMS; Wave: into WAVE_FORMS
  int cols;            // Strip: positions per strip
  int nw;              // KSplit: waves (4 | 8)
  int bk, tpw;         // Bf16Tr: K chunk (32 | 64 | 128), position tiles per workgroup
  int mt, bnn, tiles;  // weight gradients: 32-row tiles per wave (1 | 2); BwwTile: tile width (32 | 64); output tiles
  int chunks_per_img, total_chunks, chunks_per_block;  // weight gradients: the position split
  dim3 grid;
  int threads;
  size_t lds_bytes;    // dynamic LDS of the launch (KSplit, Fused)
  int num_partials;    // Fwd: fp64 statistics partials per channel; Fused: per channel of z
  int nslabs;          // BwdWeight / Fused: [Cout][Cin] fp32 slabs (1: the result itself)
};

// which (K, M, S) take the column-strip kernel (-1: none): the forward and bwd-data GEMMs of blocks 1-3
inline int strip_form(int N, int K, int M, int S) {
  for (int f = 0; f < 5; ++f) {
    // (32-column strips - two workgroups per CU - measured equal or slower: 8.2 -> 9.4 us and 11.1 -> 12.4 us on blocks 2 / 3)
    const int cols = STRIP_FORMS[f][1];
    if (K == STRIP_FORMS[f][0] && M == 32 * STRIP_FORMS[f][2])
      return (S % cols != 0 || (long long)N * (S / cols) < STRIP_MIN_WGS) ? -1 : f;
  }
  return -1;
}

// which form of the wave kernel runs a (K, M) GEMM (-1: the LDS-staged kernels).  Unsplit (K <= 64): two column tiles per wave
// where statistics are written and that still leaves >= 2 waves per SIMD - the weight rows, the input affine and the statistics
// reduction are then paid once per 64 columns (measured: tools/bench_pw.py)
inline int wave_form(int N, int K, int M, int S, bool stats) {
  if (M % 32 != 0) return -1;
  if (K == 128 || K == 256 || K == 512) return K == 128 ? 8 : K == 256 ? 9 : 10;
  if (K != 32 && K != 64) return -1;
  const int mt = (M % 64 == 0) ? 2 : 1;
  const long long waves = (long long)N * cdiv(S, 32) * (M / (32 * mt));
  const int nt = (stats && waves >= WAVE_NT2_MIN_WAVES) ? 2 : 1;
  return (K == 32 ? 0 : 4) + (mt - 1) * 2 + (nt - 1);
}

// K-split pays when the plain 64 x 128 tiling cannot fill the chip (tail layers); with >= 256 plain tiles the serial-K kernel
// wins (no cross-wave reduction).
inline bool use_ksplit(int N, int K, int M, int S) {
  return K >= 128 && K % 128 == 0 && cdiv(S, BN) * cdiv(M, BM) * N < SPLIT_MAX_TILES;
}

// the position split of a weight gradient: ks workgroups of chunks_per_block chunks each, nslabs of them non-empty
inline void split_chunks(PwRoute& r, int ks) {
  r.chunks_per_block = cdiv(r.total_chunks, ks);
  r.nslabs = cdiv(r.total_chunks, r.chunks_per_block);
}

inline void bww_route(PwRoute& r, bool bf16, int N, int Cin, int Cout, int S) {
  const int chunk = bf16 ? 64 : 32;  // positions per chunk of the two wave-autonomous kernels
  if (S % chunk == 0 && Cin % 32 == 0 && Cout % 32 == 0) {  // whole chunks and 32-channel tiles
    r.kind = bf16 ? PwKind::Bf16BwwMfma : PwKind::BwwWave;
    r.mt = (Cout % 64 == 0) ? 2 : 1;
    r.tiles = (Cout / (32 * r.mt)) * (Cin / 32);
    r.chunks_per_img = S / chunk;
    r.total_chunks = N * r.chunks_per_img;
    // position split: about one workgroup per CU in total, at least 8 (fp32: 2 per wave) / 4 (bf16) chunks each - every split
    // costs a Cout x Cin slab written and read back
    split_chunks(r, std::max(1, std::min((bf16 ? BF_BWW_WGS : BWW_WAVE_WGS) / std::max(1, r.tiles), r.total_chunks / (bf16 ? 4 : 8))));
    r.grid = dim3(r.nslabs, r.tiles);
    return;
  }
  if (bf16) {
    r.kind = PwKind::Bf16BwwAny;
    r.nslabs = 1;
    r.grid = dim3(cdiv(Cin, 16), cdiv(Cout, 16));
    return;
  }
  r.kind = PwKind::BwwTile;
  r.bnn = (Cin % 64 == 0) ? 64 : 32;
  r.chunks_per_img = cdiv(S, PC);
  r.total_chunks = N * r.chunks_per_img;
  r.tiles = (Cout / 64) * (Cin / r.bnn);
  // K split: enough workgroups to matter - every split costs a Cout x Cin slab written and read back (a 256-way split of
  // block 2 moved 8 MB of slabs for 12 MB of operands), and this kernel runs on the weight-gradient stream beside the dependency
  // chain, where fewer, longer workgroups interfere less
  split_chunks(r, std::max(1, std::min(r.total_chunks, BWW_TILE_WGS / std::max(1, r.tiles))));
  r.grid = dim3(r.nslabs, r.tiles);
}

// The route of one call.  bf16: activations stored as bf16 (bf16.hip), else fp32.  stats: the forward writes statistics
// partials (the count queries assume it does).  The caller has checked what its entry point refuses; the count queries that
// never checked their arguments still get the planners' arithmetic (sizes must be positive: the splits divide by them).
inline PwRoute pw_route(PwOp op, bool bf16, int N, int Cin, int Cout, int S, bool stats) {
  PwRoute r{};
  r.threads = 256;
  if (op == PwOp::BwdWeight) {
    bww_route(r, bf16, N, Cin, Cout, S);
    return r;
  }
  if (op == PwOp::BwdFused) {
    // workgroups (= statistics partials per channel = weight-gradient slabs): <= 256, so that the BatchNorm backward of z can
    // fold them in its own prologue (msl_bn_relu_bwd_finalize_apply)
    if (bf16 || N <= 0 || Cin != FUSED_M || Cout != FUSED_K || S % FUSED_COLS != 0) return r;
    if ((long long)N * (S / FUSED_COLS) < FUSED_MIN_STRIPS) return r;
    r.kind = PwKind::Fused;
    r.grid = dim3(FUSED_WGS);
    r.threads = 512;
    r.lds_bytes = ((size_t)(FUSED_K + 2 * FUSED_M) * (FUSED_COLS + 1) + 4 * FUSED_K + 4 * FUSED_M) * sizeof(float);
    r.num_partials = r.nslabs = FUSED_WGS;
    return r;
  }
  const int M = r.M = op == PwOp::Fwd ? Cout : Cin, K = r.K = op == PwOp::Fwd ? Cin : Cout;
  if (bf16) {
    // the pipelined transposed-read kernel takes maps of whole 8-position groups and K in whole chunks
    if (S % 8 == 0 && K % 32 == 0 && K <= PB_MAXK && M % 8 == 0) {
      r.kind = PwKind::Bf16Tr;
      r.bk = K % 128 == 0 ? 128 : K % 64 == 0 ? 64 : 32;
      const int tiles_img = cdiv(S, PT_BN), mtiles = cdiv(M, PT_BM);
      // several position tiles per workgroup once the launch has more than ~2 workgroups per CU (block 1: 2048 tiles)
      r.tpw = std::max(1, std::min(std::min(4, tiles_img), (tiles_img * mtiles * N) / PT_WGS));
      r.grid = dim3(cdiv(tiles_img, r.tpw), mtiles, N);
    } else {
      r.kind = PwKind::Bf16Plain;
      r.grid = dim3(cdiv(S, PB_BN), cdiv(M, PB_BM), N);
    }
    r.num_partials = N * cdiv(S, PB_BN) * 2;  // both kernels: one per 64-position tile and wave column
    return r;
  }
  if ((r.form = strip_form(N, K, M, S)) >= 0) {
    r.kind = PwKind::Strip;
    r.cols = STRIP_FORMS[r.form][1];
    r.grid = dim3(S / r.cols, N);
    r.num_partials = N * (S / r.cols);
  } else if ((r.form = wave_form(N, K, M, S, stats)) >= 0) {
    r.kind = PwKind::Wave;
    const int mt = WAVE_FORMS[r.form][1], nwk = WAVE_FORMS[r.form][2], nt = WAVE_FORMS[r.form][3];
    r.grid = dim3(cdiv(S, nwk == 1 ? 128 * nt : 32), M / (32 * mt), N);
    r.threads = nwk == 1 ? 256 : nwk * 64;
    r.num_partials = N * (int)r.grid.x;
  } else if (use_ksplit(N, K, M, S)) {
    r.kind = PwKind::KSplit;
    r.nw = K % 256 == 0 ? 8 : 4;
    r.grid = dim3(cdiv(S, KS_BN), cdiv(M, KS_BM), N);
    r.threads = r.nw * 64;
    r.lds_bytes = (size_t)r.nw * KS_WAVE_LDS * sizeof(float);
    r.num_partials = N * cdiv(S, KS_BN);
  } else {
    r.kind = PwKind::Gemm;
    r.grid = dim3(cdiv(S, BN), cdiv(M, BM), N);
    r.num_partials = N * cdiv(S, BN);
  }
  return r;
}

}  // namespace pw
}  // namespace msl
