/* mslesions3d_hip.h — C ABI of libmsl3d_hip.so: the MI355X (gfx950) kernels behind the 3D-SSD hot path.
 *
 * The reference (Medical-Image-Analysis-Laboratory/MSLesions3D) has no FFI: its hot path is Python calling
 * stock torch ops.  The entry points below are what a maintainer of the reference would bind
 * (ctypes) to replace those op sequences; each one names the reference lines it replaces.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (HBM) unless the comment says "host"; tensors are dense fp32, NCDHW,
 *    W fastest; `stream` is a hipStream_t passed as void* (NULL = default stream); nothing here synchronises.
 *  - return value: 0 on success, >0 a hipError_t from the launch, -1 bad argument, -2 unsupported shape.
 *  - "raw" = convolution output BEFORE BatchNorm; an (in_scale, in_shift) pair is the folded BatchNorm of the
 *    producer (scale = gamma/sqrt(var+eps), shift = beta - mean*scale); consumers apply relu(x*scale+shift)
 *    while loading.  in_scale == NULL means "input is already an activation / a plain tensor".
 *  - stat partials: fp64 [2][C][NP] (sum, then sum of squares) written by a conv kernel, NP from the matching
 *    *_num_partials(); msl_bn_finalize folds them in a fixed order (bit-reproducible, no float atomics).
 */
#ifndef MSLESIONS3D_HIP_H
#define MSLESIONS3D_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

int msl_abi_version(void);

/* ---- BatchNorm3d (train-mode batch statistics) + ReLU : mobilenet.py:29-30, :39, :41, :44-45 ------------- */
int msl_bn_finalize(const double* partials, int num_partials, double count, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, long long* num_batches_tracked, float momentum,
                    float eps, float* scale, float* shift, float* save_mean, float* save_invstd, int C,
                    void* stream);
/* every BatchNorm of the network in one launch: fill a host table entry per layer, copy it to the device once */
size_t msl_bn_finalize_entry_bytes(void);
int msl_bn_finalize_table_set(void* host_table, int index, int first_block, const double* partials, int num_partials,
                              double count, const float* gamma, const float* beta, float* running_mean,
                              float* running_var, long long* num_batches_tracked, float momentum, float eps,
                              float* scale, float* shift, float* save_mean, float* save_invstd, int C);
int msl_bn_finalize_batch(const void* device_table, int n_entries, int total_channels, void* stream);
/* eval mode: scale/shift from the running statistics */
/* eval-mode (scale, shift) of every BatchNorm in a table built with msl_bn_finalize_table_set, one launch */
int msl_bn_eval_affine_batch(const void* device_table, int n_entries, int total_channels, void* stream);
int msl_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                       float eps, float* scale, float* shift, int C, void* stream);
/* relu(y*scale+shift) into a plain (N,C,D,H,W) tensor and/or a zero-haloed (N,C,D+2,H+2,W+2) one (either may be NULL) */
int msl_bn_relu_materialize(const float* y, const float* scale, const float* shift, float* out_plain,
                            float* out_pad, int N, int C, int D, int H, int W, void* stream);
int msl_bn_relu_materialize_fold(const float* y, const double* partials, int num_partials, double count,
                                 const float* gamma, const float* beta, float eps, float* out_plain, float* out_pad,
                                 int N, int C, int D, int H, int W, void* stream);
/* backward of a = relu(bn(y)):  reduce -> finalize -> apply (dy may alias g) */
int msl_bn_relu_bwd_num_partials(int N, int S);
int msl_bn_relu_bwd_reduce(const float* g, const float* y, const float* scale, const float* shift,
                           const float* mean, const float* invstd, double* partials, int N, int C, int S,
                           void* stream);
int msl_bn_bwd_finalize(const double* partials, int num_partials, double count, float* dgamma, float* dbeta,
                        float* c1, float* c2, int C, void* stream);
/* same on an (8, C) vector block [scale, shift, mean, invstd | c1, c2, cC, cE]: writes rows 4-7, where
 * dL/dy = scale * gm + (cC * y + cE) is the folded form used by msl_stem_conv_bwd_weight_fused */
int msl_bn_bwd_finalize_coef(const double* partials, int num_partials, double count, float* dgamma, float* dbeta,
                             float* bn_vec, int C, void* stream);
int msl_bn_relu_bwd_apply(const float* g, const float* y, const float* scale, const float* shift,
                          const float* mean, const float* invstd, const float* c1, const float* c2, float* dy,
                          int N, int C, int S, void* stream);
/* msl_bn_bwd_finalize + msl_bn_relu_bwd_apply in one launch (for <= 256 partials per channel): bn_vec = the (>= 6, C)
 * block [scale, shift, mean, invstd, c1, c2, ...], rows 4-5 are written */
int msl_bn_relu_bwd_finalize_apply(const double* partials, int num_partials, double count, const float* g, const float* y,
                                   float* bn_vec, float* dgamma, float* dbeta, float* dy, int N, int C, int S,
                                   void* stream);

/* the three steps above in one launch (one workgroup per channel); for N*S <= 65536 elements per channel */
int msl_bn_relu_bwd_fused(const float* g, const float* y, const float* scale, const float* shift, const float* mean,
                          const float* invstd, float* dgamma, float* dbeta, float* dy, int N, int C, int S,
                          void* stream);

/* Per-channel backward link of a Block (autograd of mobilenet.py:43-47 between two pointwise GEMMs), one launch instead of
 * msl_bn_relu_bwd_fused (bn1) + msl_dwconv_bwd_data + msl_bn_relu_bwd_fused (previous block's bn2):
 *   g_z (N,C,OD,OH,OW): in dL/d relu(bn1(z)), out dL/dz (in place; the depthwise weight gradient reads it)
 *   g_y (N,C,D,H,W):    out dL/dy_prev; with accumulate != 0 its content (the heads' share, ssd3d.py:143-169 backward) is
 *                       added to the depthwise bwd-data result before the BatchNorm backward
 *   vec_z / vec_y: (>= 4, C) BatchNorm vector blocks [scale, shift, mean, invstd] of bn1 (on z) / of the previous bn2 (on y_prev)
 *   dw_dw (C,27) or NULL: if given, the depthwise weight gradient dL/dw_dw (mobilenet.py:38 backward) is produced as well
 *                       (same operand pairs as the transposed convolution) - msl_dwconv_bwd_weight is then not needed
 *   (D,H,W) = input extents of the depthwise layer (powers of two, W >= 4, OW >= 4), stride 1 or 2 (k3, p1).  A channel's
 *   whole population lives in one workgroup: supported while N*D*H*W <= 16384 per channel; else MSL_ERR_UNSUPPORTED (-2).
 *   _supported returns the number of waves per channel the launch would use (1, 4, 8 or 16), 0 if unsupported: with
 *   many waves per channel the kernel is bound by instruction issue and dw_dw is better left to its own launch. */
int msl_block_bwd_channel_link_supported(int N, int D, int H, int W, int stride);
int msl_block_bwd_channel_link(float* g_z, const float* z, const float* vec_z, const float* w_dw, const float* y_prev,
                               const float* vec_y, float* g_y, float* dgamma_z, float* dbeta_z, float* dgamma_y,
                               float* dbeta_y, float* dw_dw, int N, int C, int D, int H, int W, int stride, int accumulate,
                               void* stream);

/* Pointwise backward of a big early block in one pass (autograd of mobilenet.py:45-47 for Block.conv2 / bn2 / bn1):
 *   g_y (N,Cout,S) = dL/d relu(bn2(y)) (raw), y (N,Cout,S) raw conv2 output, bn_y_vec (>= 4, Cout) [scale, shift, mean, invstd],
 *   y_partials fp64 [2][Cout][y_np] = the BatchNorm2-backward sums the producer of g_y emitted (msl_dwconv_bwd_data_bnreduce),
 *   y_count = N*S  ->  dgamma_y / dbeta_y, and dL/dy applied on the fly (never stored);
 *   g_z (N,Cin,S) = W^T . dL/dy (= dL/d relu(bn1(z)), raw), z_partials fp64 [2][Cin][NP] = BatchNorm1-backward sums of z
 *   (for msl_bn_relu_bwd_finalize_apply), dw_slabs [NP][Cout][Cin] = partial sums of dL/dW (msl_grad_reduce kind 0);
 *   NP = msl_pwconv_bwd_fused_num_partials (0: shape not taken - Cin = 32, Cout = 64, S % 128 == 0, >= 512 strips of 128
 *   positions - use msl_bn_relu_bwd_* + msl_pwconv_bwd_data + msl_pwconv_bwd_weight_slabs; the entry returns -2). */
int msl_pwconv_bwd_fused_num_partials(int N, int Cin, int Cout, int S);
int msl_pwconv_bwd_fused(const float* g_y, const float* y, const float* bn_y_vec, const double* y_partials, int y_np,
                         double y_count, float* dgamma_y, float* dbeta_y, const float* w, const float* z,
                         const float* bn_z_vec, float* g_z, double* z_partials, float* dw_slabs, int N, int Cin, int Cout, int S,
                         void* stream);

/* ---- stem: Conv3d(Cin->32,k3,stride (sd,sh,sw),p1,no bias) : mobilenet.py:26-31 via ssd3d.py:60-61 -------
 * Every stem entry point takes Cin 1..4 and strides 1..2 and refuses before any launch: Cin < 1, a stride outside 1..2 or
 * N, D, H, W <= 0 with MSL_ERR_ARG, Cin > 4 with MSL_ERR_UNSUPPORTED. */
int msl_stem_conv_fwd_num_partials(int N, int OD, int OH, int OW);
int msl_stem_conv_fwd(const float* x, const float* w, float* y, double* partials, int N, int Cin, int D, int H,
                      int W, int sd, int sh, int sw, void* stream);
size_t msl_stem_conv_bwd_weight_workspace_bytes(int Cin);
/* slabs ([32][32*ceil(Cin*27/32)] floats each) the three stem weight-gradient forms leave in `workspace`; with dw == NULL they
 * skip their own reduction (deferred: msl_grad_reduce_batch kind 2) */
int msl_stem_conv_bwd_weight_nslabs(int N, int D, int H, int W, int sd, int sh, int sw);
int msl_stem_conv_bwd_weight(const float* dy, const float* x, float* dw, float* workspace, int N, int Cin, int D,
                             int H, int W, int sd, int sh, int sw, void* stream);

/* same, with the BatchNorm+ReLU backward of the stem applied while loading: g = dL/d relu(bn(y)), bn_vec (6,32) */
int msl_stem_conv_bwd_weight_bnapply(const float* g, const float* yraw, const float* bn_vec, const float* x, float* dw,
                                     float* workspace, int N, int Cin, int D, int H, int W, int sd, int sh, int sw,
                                     void* stream);

/* same again for a stem that feeds a stride-2 depthwise layer with taps w1_t (27,32), tap-major: dz is THAT layer's dL/dz
 * (N,32,ceil(OD/2),ceil(OH/2),ceil(OW/2)) and the gradient of the stem activation (autograd's grad of ssd3d.py:81's
 * first feature) is rebuilt from it inside the kernel, never stored.  Pair: msl_dwconv_s2_bwd_bnreduce_bww. */
int msl_stem_conv_bwd_weight_fused(const float* dz, const float* w1_t, const float* yraw, const float* bn_vec,
                                   const float* x, float* dw, float* workspace, int N, int Cin, int D, int H, int W,
                                   int sd, int sh, int sw, void* stream);

/* ---- depthwise Conv3d(C,C,k3,stride s,p1,groups=C) : Block.conv1, mobilenet.py:38,44 ---------------------- */
int msl_dwconv_fwd_num_partials(int N, int C, int D, int H, int W, int stride);
int msl_dwconv_fwd_variant(int N, int C, int D, int H, int W, int stride); /* 0 naive, 1 stream, 2 resident, 3 wave */
int msl_dwconv_fwd(const float* x, const float* in_scale, const float* in_shift, const float* w, float* y,
                   double* partials, int N, int C, int D, int H, int W, int stride, int force_naive, void* stream);
/* forward with the input's BatchNorm folded in-kernel from the producer's partials (no finalize launch on the chain) */
int msl_dwconv_fwd_fold(const float* x, const double* in_partials, int in_np, double in_count, const float* gamma,
                        const float* beta, float eps, const float* w, float* y, double* partials, int N, int C, int D,
                        int H, int W, int stride, void* stream);
int msl_dwconv_bwd_data(const float* dy, const float* w, float* g_in, int N, int C, int D, int H, int W,
                        int stride, int accumulate, void* stream);
/* stride-2 bwd-data that also emits the BatchNorm-backward partials of the layer it feeds (fp64 [2][C][NP]) */
int msl_dwconv_bwd_data_bnreduce_num_partials(int N, int C, int D, int H, int W);
int msl_dwconv_bwd_data_bnreduce(const float* dy, const float* w, float* g_in, const float* y_prev,
                                 const float* bn_scale, const float* bn_shift, const float* bn_mean,
                                 const float* bn_invstd, double* partials, int N, int C, int D, int H, int W, int stride,
                                 int accumulate, void* stream);
/* stride-2 backward in ONE pass over (dy = dL/dz, y_prev) that does NOT write the input gradient: emits the
 * BatchNorm-backward partials of the producer layer (fp64 [2][C][NP]) and this layer's weight-gradient partials
 * (fp64 [C*27][NP]); msl_dwconv_bwd_weight_finalize sums the latter into dw (C,27).  NP from ..._num_partials (-1 =
 * shape unsupported).  w_taps_t (may be NULL) receives the (27,C) transpose of w. */
int msl_dwconv_s2_bwd_bnreduce_bww_num_partials(int N, int C, int D, int H, int W);
int msl_dwconv_s2_bwd_bnreduce_bww(const float* dy, const float* w, const float* y_prev, const float* bn_scale,
                                   const float* bn_shift, const float* bn_mean, const float* bn_invstd,
                                   double* bn_partials, double* w_partials, float* w_taps_t, int N, int C, int D, int H,
                                   int W, void* stream);
/* the same pass when the input gradient is a tensor of its own (every stride-2 block but the one behind a fused stem): also
 * writes g_in (N,C,D,H,W) = dL/d relu(bn(y_prev)) (accumulate != 0: on top of the heads' share already there) - one launch
 * instead of msl_dwconv_bwd_data_bnreduce + msl_dwconv_bwd_weight; partial counts as msl_dwconv_s2_bwd_bnreduce_bww_num_partials */
int msl_dwconv_s2_bwd_data_bnreduce_bww(const float* dy, const float* w, float* g_in, const float* y_prev,
                                        const float* bn_scale, const float* bn_shift, const float* bn_mean,
                                        const float* bn_invstd, double* bn_partials, double* w_partials, int N, int C, int D,
                                        int H, int W, int accumulate, void* stream);
int msl_dwconv_bwd_weight_finalize(const double* w_partials, int num_partials, float* dw, int C, void* stream);
int msl_dwconv_bwd_weight_num_partials(int N, int C, int D, int H, int W, int stride);
int msl_dwconv_bwd_weight(const float* dy, const float* x, const float* in_scale, const float* in_shift, float* dw,
                          double* partials, int N, int C, int D, int H, int W, int stride, void* stream);
/* Which kernel family a depthwise call of this shape runs (host arithmetic only, nothing is launched) - for tests / DESIGN.md.
 * op: 0 statistics-free forward, 1 stride-1 bwd-data as the flipped forward, 2 bwd-data, 3 bwd-weight; bf16 != 0: bf16 storage.
 * Returns 0 none, 1 wave, 2 rows-eval, 3 small-eval, 4 stream, 5 resident, 6 naive, 7 tiled (bf16), 8 tiled stride-2 bwd-data
 * (bf16), 9 stride-2 patch, 10 vectorised bwd-data, 11 generic bwd-data, 12 wave-per-chunk bwd-weight; MSL_ERR_ARG for an unknown
 * op, a bf16 flag other than 0 / 1, or a shape the entry points refuse. */
int msl_dwconv_route_kind(int op, int bf16, int N, int C, int D, int H, int W, int stride);

/* ---- pointwise Conv3d(Cin,Cout,k1) = per-image GEMM on MFMA : Block.conv2, mobilenet.py:40,45 ------------- */
/* Which kernel family a pointwise call of this shape runs (host arithmetic only, nothing is launched) - for tests / DESIGN.md.
 * op: 0 forward, 1 bwd-data, 2 bwd-weight, 3 the one-pass backward of msl_pwconv_bwd_fused; bf16 != 0: bf16 storage; stats != 0:
 * the forward writes statistics partials (as every *_num_partials query assumes).
 * Returns 0 none, 1 strip, 2 wave, 3 K-split GEMM, 4 GEMM, 5 wave-autonomous weight gradient, 6 tiled weight gradient, 7 bf16
 * transposed-read GEMM, 8 bf16 plain GEMM, 9 bf16 MFMA weight gradient, 10 bf16 one-slab weight gradient, 11 fused one-pass
 * backward; MSL_ERR_ARG for an unknown op, a bf16 flag other than 0 / 1, or a size <= 0.  Channel counts an entry point refuses
 * still get the planners' answer. */
int msl_pwconv_route_kind(int op, int bf16, int N, int Cin, int Cout, int S, int stats);
int msl_pwconv_fwd_num_partials(int N, int Cin, int Cout, int S);
int msl_pwconv_fwd(const float* z, const float* in_scale, const float* in_shift, const float* w, float* y,
                   double* partials, int N, int Cin, int Cout, int S, void* stream);
int msl_pwconv_fwd_fold(const float* z, const double* in_partials, int in_np, double in_count, const float* gamma,
                        const float* beta, float eps, const float* w, float* y, double* partials, int N, int Cin,
                        int Cout, int S, void* stream);
int msl_pwconv_bwd_data(const float* dy, const float* w, float* g_in, int N, int Cin, int Cout, int S,
                        void* stream);
size_t msl_pwconv_bwd_weight_workspace_bytes(int N, int Cin, int Cout, int S);
int msl_pwconv_bwd_weight(const float* dy, const float* z, const float* in_scale, const float* in_shift, float* dw,
                          float* workspace, int N, int Cin, int Cout, int S, void* stream);
/* the same as partial results: `out` = [nslabs][Cout][Cin] slabs whose sum (slab order) is dW; nslabs == 1: dW itself.
 * The training step folds the slabs of every layer in one msl_grad_reduce_batch (kind 0). */
int msl_pwconv_bwd_weight_nslabs(int N, int Cin, int Cout, int S);
int msl_pwconv_bwd_weight_slabs(const float* dy, const float* z, const float* in_scale, const float* in_shift,
                                float* out, int N, int Cin, int Cout, int S, void* stream);
/* the same for n <= 4 layers in ONE launch (the tail blocks, whose launches are pure latency): the eight arrays have n
 * entries and live on the host; every layer must be batchable (msl_pwconv_bwd_weight_batchable == 1) and carries its
 * input affine.  out[k] as `out` above for layer k.  Same arithmetic and slabs as n single calls: mobilenet.py:40 */
int msl_pwconv_bwd_weight_batchable(int N, int Cin, int Cout, int S);
int msl_pwconv_bwd_weight_slabs_batch(const float* const* dy, const float* const* z, const float* const* in_scale,
                                      const float* const* in_shift, float* const* out, const int* Cin, const int* Cout,
                                      const int* S, int n, int N, void* stream);

/* ---- detection heads: loc (C->12) + cls (C->2*ncls) k3 p1 convs, permute/view/cat fused : ssd3d.py:113-169 - */
size_t msl_head_packed_weight_elems(int C, int ncls);
int msl_head_pack_weights(const float* loc_w, const float* cl_w, float* Wf, float* Wb, int C, int ncls,
                          void* stream);
/* the same for all (<= 4) scales of the model in one launch; the five arrays have n entries and live on the host */
int msl_head_pack_weights_batch(const float* const* loc_w, const float* const* cl_w, float* const* Wf, float* const* Wb,
                                const int* C, int n, int ncls, void* stream);
size_t msl_head_fwd_workspace_bytes(int N, int C, int D, int H, int W, int ncls);
int msl_head_conv_fwd(const float* a_pad, const float* Wf, const float* loc_b, const float* cl_b, float* locs,
                      float* scores, float* workspace, int N, int C, int D, int H, int W, int Ptot, int prior_off,
                      int ncls, void* stream);
int msl_head_grad_pack(const float* dlocs, const float* dscores, float* dO_pad, int N, int D, int H, int W,
                       int Ptot, int prior_off, int ncls, void* stream);
/* the same for all (n <= 4) scales in one launch; dO_pad / D / H / W / prior_off are host arrays of n entries */
int msl_head_grad_pack_batch(const float* dlocs, const float* dscores, float* const* dO_pad, const int* D, const int* H,
                             const int* W, const int* prior_off, int n, int N, int Ptot, int ncls, void* stream);
int msl_head_conv_bwd_data(const float* dO_pad, const float* Wb, float* g_a, int N, int C, int D, int H, int W,
                           int ncls, void* stream);
size_t msl_head_bwd_weight_workspace_bytes(int N, int C, int D, int H, int W, int ncls);
/* slabs msl_head_conv_bwd_weight leaves in `workspace`; dloc_w == NULL skips its own reduction (deferred: kind 3) */
int msl_head_conv_bwd_weight_nslabs(int N, int C, int D, int H, int W, int ncls);
int msl_head_conv_bwd_weight(const float* dO_pad, const float* a_pad, float* dloc_w, float* dcl_w, float* dloc_b,
                             float* dcl_b, float* workspace, int N, int C, int D, int H, int W, int ncls,
                             void* stream);

/* ---- bf16 activation path (BASELINE configs[2]/[3]; the reference is fp32: a build-side extension) ------
 * Activations are bf16 in HBM (raw conv outputs, NCDHW; `void*` = bf16 storage); weights, BatchNorm vectors and statistics
 * and all accumulators stay fp32.  The forward kernels of the backbone + heads (mobilenet.py:26-49, ssd3d.py:113-169): */
int msl_stem_conv_fwd_bf16(const float* x, const float* w, void* y_bf16, double* partials, int N, int Cin, int D,
                           int H, int W, int sd, int sh, int sw, void* stream);

/* Eval-mode stem + block-1 depthwise convolution in one pass (inference; mobilenet.py:26-31 followed by the depthwise half of
 * mobilenet.py:34-49): z1 (N,32,D/4,H/4,W/4) = dw3x3x3 s2 (wdw [32][27]) of relu(bn_scale * stem(x) + bn_shift), the stem
 * activation never reaching HBM (in eval mode the BatchNorm between the two is a constant affine).  Values are those of
 * msl_stem_conv_fwd followed by msl_dwconv_fwd, bit for bit.  _supported: 1 if the shape is taken (Cin <= 2, D, H, W multiples
 * of 4, W/2 a multiple of 32 and <= 96), else callers use the two separate entry points. */
int msl_stem_dw_fwd_eval_supported(int N, int Cin, int D, int H, int W);
int msl_stem_dw_fwd_eval(const float* x, const float* w, const float* bn_scale, const float* bn_shift, const float* wdw,
                         float* z, int N, int Cin, int D, int H, int W, void* stream);
int msl_stem_dw_fwd_eval_bf16(const float* x, const float* w, const float* bn_scale, const float* bn_shift, const float* wdw,
                              void* z_bf16, int N, int Cin, int D, int H, int W, void* stream);
int msl_dwconv_fwd_bf16_num_partials(int N, int C, int D, int H, int W, int stride);
/* the register-marching wave kernels of the fp32 path on bf16 storage (square power-of-two planes; MSL_ERR_UNSUPPORTED
 * otherwise - msl_dwconv_*_bf16 try these first and fall back to the LDS-tiled any-shape kernels) */
int msl_dwconv_wave_num_partials(int N, int C, int D, int H, int W, int stride);
/* 1 when a statistics-free (eval-mode) forward of this shape runs on the register-marching rows kernels (W % 4 == 0 planes that
 * are not powers of two, e.g. the 96^2 ... 12^2 planes of a 192^3 volume): fp32 inside msl_dwconv_fwd, bf16 inside
 * msl_dwconv_fwd_wave_bf16 / msl_dwconv_fwd_bf16 when partials == NULL.  mobilenet.py:37-39 */
int msl_dwconv_fwd_eval_rows_ok(int N, int C, int D, int H, int W, int stride);
/* bf16 storage, statistics-free forward of a map of at most 512 voxels (one wave per (image, channel), volume in LDS);
 * msl_dwconv_fwd_bf16 takes this route by itself in eval mode */
int msl_dwconv_fwd_small_eval_bf16(const void* x, const float* in_scale, const float* in_shift, const float* w, void* y, int N,
                                   int C, int D, int H, int W, int stride, void* stream);
int msl_dwconv_fwd_wave_bf16(const void* x, const float* in_scale, const float* in_shift, const float* w, void* y,
                             double* partials, int N, int C, int D, int H, int W, int stride, int flip, int accumulate,
                             void* stream);
/* stride-2 bwd-data on bf16 gradients (one thread per 2x2x4 input patch; W % 4 == 0); y_prev != NULL: also the
 * BatchNorm-backward partials [2][C][NP] of the layer written, NP = msl_dwconv_bwd_data_bnreduce_num_partials */
int msl_dwconv_bwd_data_s2_patch_bf16(const void* dy, const float* w, void* g_in, const void* y_prev, const float* bn_vec,
                                      double* partials, int N, int C, int D, int H, int W, int accumulate, void* stream);
int msl_dwconv_fwd_wave_bf16_fold(const void* x, const double* in_partials, int in_np, double in_count, const float* gamma,
                                  const float* beta, float eps, const float* w, void* y, double* partials, int N, int C, int D,
                                  int H, int W, int stride, void* stream);
int msl_dwconv_bwd_weight_wave_bf16(const void* dz, const void* x, const float* in_scale, const float* in_shift,
                                    double* partials, int N, int C, int D, int H, int W, int stride, void* stream);
int msl_dwconv_fwd_bf16(const void* x, const float* in_scale, const float* in_shift, const float* w, void* y,
                        double* partials, int N, int C, int D, int H, int W, int stride, void* stream);
int msl_pwconv_fwd_bf16_num_partials(int N, int S);
/* pointwise GEMM on v_mfma_f32_32x32x16_bf16 (fp32 accumulate) */
/* input BatchNorm folded from the producer's partials (in_np <= 64, Cin <= 1024; MSL_ERR_UNSUPPORTED otherwise) */
int msl_pwconv_fwd_bf16_fold(const void* z, const double* in_partials, int in_np, double in_count, const float* gamma,
                             const float* beta, float eps, const float* w, void* y, double* partials, int N, int Cin, int Cout,
                             int S, void* stream);
int msl_pwconv_fwd_bf16(const void* z, const float* in_scale, const float* in_shift, const float* w, void* y,
                        double* partials, int N, int Cin, int Cout, int S, void* stream);
/* relu(bn(y)) of a head feature map -> bf16 CHANNELS-LAST zero-haloed copy (N,D+2,H+2,W+2,C), halo zeroed by the caller */
int msl_bn_relu_materialize_bf16(const void* y, const float* scale, const float* shift, float* plain, void* pad_cl, int N,
                                 int C, int D, int H, int W, void* stream);
/* ... fp32 zero-haloed NCDHW copy (N,C,D+2,H+2,W+2) instead: the bf16 TRAINING step runs its heads on the fp32 kernels */
int msl_bn_relu_materialize_bf16_pad32(const void* y, const float* scale, const float* shift, float* pad, int N, int C, int D,
                                       int H, int W, void* stream);
/* the same in training mode with the affine folded from the producer's statistics partials ([2][C][in_np]) */
int msl_bn_relu_materialize_bf16_pad32_fold(const void* y, const double* in_partials, int in_np, double in_count,
                                            const float* gamma, const float* beta, float eps, float* pad, int N, int C, int D,
                                            int H, int W, void* stream);
size_t msl_head_packed_weight_bf16_elems(int C);
int msl_head_pack_weights_bf16(const float* loc_w, const float* cl_w, void* Wp, int C, int ncls, void* stream);
/* both head convolutions of a scale on v_mfma_f32_16x16x32_bf16, fp32 rows out */
int msl_head_conv_fwd_bf16(const void* a_cl, const void* Wp, const float* loc_b, const float* cl_b, float* locs,
                           float* scores, int N, int C, int D, int H, int W, int Ptot, int prior_off, int ncls,
                           void* stream);
/* ... and the backward kernels of the bf16 training step (BASELINE configs[2]); gradients of activations are bf16 too,
 * weight gradients and all reductions fp32 / fp64 (same partial-sum layouts as the fp32 kernels, folded by
 * msl_grad_reduce_batch / msl_bn_bwd_finalize): */
int msl_pwconv_bwd_data_bf16(const void* dy, const float* w, void* g_in, int N, int Cin, int Cout, int S, void* stream);
int msl_pwconv_bwd_weight_bf16_nslabs(int N, int Cin, int Cout, int S);
int msl_pwconv_bwd_weight_slabs_bf16(const void* dy, const void* z, const float* in_scale, const float* in_shift, float* out,
                                     int N, int Cin, int Cout, int S, void* stream);
int msl_dwconv_bwd_data_bf16(const void* dy, const float* w, void* g_in, int N, int C, int D, int H, int W, int stride,
                             int accumulate, void* stream);
int msl_dwconv_bwd_weight_bf16(const void* dz, const void* x, const float* in_scale, const float* in_shift, double* partials,
                               int N, int C, int D, int H, int W, int stride, void* stream);
int msl_bn_relu_bwd_bf16_num_partials(int N, int S);
int msl_bn_relu_bwd_reduce_bf16(const void* g, const void* y, const float* scale, const float* shift, const float* mean,
                                const float* invstd, double* partials, int N, int C, int S, void* stream);
int msl_bn_relu_bwd_apply_bf16(const void* g, const void* y, const float* vec, void* dy, int N, int C, int S, void* stream);
int msl_bn_relu_bwd_fused_bf16(const void* g, const void* y, const float* vec, float* dgamma, float* dbeta, void* dy, int N,
                               int C, int S, void* stream);
/* msl_block_bwd_channel_link on bf16 activation / activation-gradient tensors (g_z, z, y_prev, g_y); vectors, taps, sums fp32 */
int msl_block_bwd_channel_link_bf16(void* g_z, const void* z, const float* vec_z, const float* w_dw, const void* y_prev,
                                    const float* vec_y, void* g_y, float* dgamma_z, float* dbeta_z, float* dgamma_y,
                                    float* dbeta_y, float* dw_dw, int N, int C, int D, int H, int W, int stride, int accumulate,
                                    void* stream);
int msl_head_conv_bwd_data_bf16(const float* dO_pad, const float* Wb, void* g_a_bf16, int N, int C, int D, int H, int W,
                                int ncls, void* stream);
int msl_head_conv_bwd_weight_bf16(const float* dO_pad, const void* a_cl, float* dloc_w, float* dcl_w, float* dloc_b,
                                  float* dcl_b, float* workspace, int N, int C, int D, int H, int W, int ncls,
                                  void* stream);
/* the fused stem backward (msl_dwconv_s2_bwd_bnreduce_bww -> msl_bn_bwd_finalize_coef -> msl_stem_conv_bwd_weight_fused) on
 * bf16 dL/dz and raw stem output: dL/d(stem activation) is never stored */
int msl_dwconv_s2_bwd_bnreduce_bww_bf16(const void* dy, const float* w, const void* y_prev, const float* bn_vec,
                                        double* bn_partials, double* w_partials, float* w_taps_t, int N, int C, int D, int H,
                                        int W, void* stream);
int msl_stem_conv_bwd_weight_fused_bf16(const void* dz, const float* w1_t, const void* yraw, const float* bn_vec, const float* x,
                                        float* dw, float* workspace, int N, int Cin, int D, int H, int W, int sd, int sh, int sw,
                                        void* stream);
int msl_stem_conv_bwd_weight_bnapply_bf16(const void* g, const void* yraw, const float* bn_vec, const float* x, float* dw,
                                          float* workspace, int N, int Cin, int D, int H, int W, int sd, int sh, int sw,
                                          void* stream);

/* ---- priors, box math, matching, MultiBox loss : ssd3d.py:286-342, utils.py:42-149, ssd3d.py:741-941 ------- */
int msl_make_priors(float* out, int row_off, int D0, int D1, int D2, double scale, int boxes_per_location,
                    void* stream);
/* op 0 cxcycz_to_xyz (utils.py:42) 1 xyz_to_cxcycz (:92) 2 cxcycz_to_gcxgcygcz (:71) 3 gcxgcygcz_to_cxcycz (:54) */
int msl_box_transform(const float* boxes, const float* priors, float* out, int n, int op, void* stream);
/* find_jaccard_overlap3d (utils.py:125) / find_intersection3d (utils.py:105) */
int msl_iou_matrix(const float* set1, const float* set2, float* out, int n1, int n2, int intersection_only,
                   void* stream);
/* MultiBoxLoss.forward matching part (ssd3d.py:786-887) for the whole batch.  gt_* are the per-image lists
 * concatenated; obj_off (N+1) int32 prefix offsets.  scratch: overlap (N,P) f32, obj (N,P) i32,
 * prior_for_obj (T) i32.  Outputs: true_classes (N,P) i64 in {-1,0,label}, true_locs (N,P,6), matched (N,P) i64
 * (may be NULL).  soft != 0 selects the two-threshold band of ssd3d.py:878-881. */
int msl_multibox_match(const float* gt_boxes, const long long* gt_labels, const int* obj_off, int total_objects,
                       const float* priors_c, int N, int P, float thr_lo, float thr_hi, int soft, float* overlap,
                       int* obj, int* prior_for_obj, long long* true_classes, float* true_locs, long long* matched,
                       void* stream);
/* the same; additionally *npos = number of positive priors of the batch (ssd3d.py:890-893), for msl_multibox_loss_pack */
int msl_multibox_match_count(const float* gt_boxes, const long long* gt_labels, const int* obj_off, int total_objects,
                             const float* priors_c, int N, int P, float thr_lo, float thr_hi, int soft, float* overlap,
                             int* obj, int* prior_for_obj, long long* true_classes, float* true_locs, long long* matched,
                             int* npos, void* stream);
size_t msl_multibox_loss_workspace_bytes(void);
/* loss part (ssd3d.py:890-941): loss_out[0] = conf_loss, [1] = loc_loss, [2] = number of positives */
int msl_multibox_loss_fwd(const float* locs, const float* scores, const long long* true_classes,
                          const float* true_locs, double* workspace, float* loss_out, int N, int P, int ncls,
                          void* stream);
int msl_multibox_loss_bwd(const float* locs, const float* scores, const long long* true_classes,
                          const float* true_locs, const float* loss_out, const float* upstream, float* dlocs,
                          float* dscores, int N, int P, int ncls, void* stream);

/* loss forward + backward for the training loop (2 launches; publishes loss_out as above).  nan_flag (may be NULL):
 * |= 1 if locs holds a NaN, |= 2 if scores does (the guards of ssd3d.py:258-261 without a pass of their own) */
int msl_multibox_loss_fwd_bwd(const float* locs, const float* scores, const long long* true_classes,
                              const float* true_locs, double* workspace, float* loss_out, const float* upstream,
                              float* dlocs, float* dscores, int* nan_flag, int N, int P, int ncls, void* stream);

/* Training hot loop, ONE launch: the loss terms of ssd3d.py:890-941, their gradients (the number of positives comes from
 * msl_multibox_match_count, so no thread waits for the loss sums) and the scatter of those gradients into the zero-haloed
 * head-gradient images of msl_head_grad_pack (dO_pad / D / H / W / prior_off: host arrays of n <= 4 scales; rows
 * a*6+q = box regressions of anchor a, 12 + a*ncls + c = class scores; padding rows are not written and must be zero).
 * partials: 2 * msl_multibox_loss_pack_num_partials(N, P) doubles; a kind-4 entry of msl_grad_reduce_batch folds them into
 * loss_out = [conf_loss, loc_loss, n_positives].  upstream / nan_flag as msl_multibox_loss_fwd_bwd. */
int msl_multibox_loss_pack_num_partials(int N, int P);
int msl_multibox_loss_pack(const float* locs, const float* scores, const long long* true_classes, const float* true_locs,
                           const int* npos, const float* upstream, double* partials, int* nan_flag, float* const* dO_pad,
                           const int* D, const int* H, const int* W, const int* prior_off, int n, int N, int P, int ncls,
                           void* stream);

/* Optional loss variants the reference keeps as commented code (ssd3d.py:758-760 loss choices, :926-932 hard-negative
 * mining); flags: 1 = hard-negative mining (keep the neg_pos_ratio * n_positives largest negative losses per image),
 * 2 = smooth-L1 (nn.SmoothL1Loss, beta 1) for the localisation loss, 4 = focal confidence loss (MONAI FocalLoss gamma 2,
 * weight 0.25, background excluded: two classes only, else MSL_ERR_UNSUPPORTED); 0 = the live path.  Forward, and
 * backward too when dlocs / dscores are given (upstream as above).  var_ws: ..._var_workspace_bytes(N, P) bytes. */
size_t msl_multibox_loss_var_workspace_bytes(int N, int P);
int msl_multibox_loss_var(const float* locs, const float* scores, const long long* true_classes, const float* true_locs,
                          double* workspace, void* var_ws, float* loss_out, const float* upstream, float* dlocs,
                          float* dscores, int* nan_flag, int N, int P, int ncls, int flags, int neg_pos_ratio,
                          void* stream);

/* The same call with an IoU-family localisation loss on the DECODED boxes of the positive priors (not in the reference):
 * kind 1 = IoU (1 - iou), 2 = GIoU (+ (enclosure - union) / enclosure), 3 = DIoU (+ centre distance^2 / sum of squared
 * enclosure extents); loc_loss = sum / n_positives.  Predicted box: centre g p_size / 10 + p_centre, size
 * exp(clamp(g / 5, -4, 4)) p_size; target box: the same decode of true_locs without the clamp.  priors_c: the (P, 6)
 * centre-size priors of the matcher.  flags: the confidence bits of msl_multibox_loss_var only (0, 1, 4, 5; bit 2 ->
 * MSL_ERR_ARG); confidence loss, mined mask and dscores have the bits msl_multibox_loss_var(flags) gives.  workspace,
 * var_ws, loss_out, upstream, dlocs / dscores (both or neither) and nan_flag as there.  Without a positive loc_loss is NaN. */
int msl_multibox_loss_iou(const float* locs, const float* scores, const long long* true_classes, const float* true_locs,
                          const float* priors_c, double* workspace, void* var_ws, float* loss_out, const float* upstream,
                          float* dlocs, float* dscores, int* nan_flag, int N, int P, int ncls, int flags, int neg_pos_ratio,
                          int kind, void* stream);

/* ---- LSSD3D.detect_objects (ssd3d.py:344-460): softmax, decode, filter, sort, 3D NMS, top-k ---------------
 * cap = 10*top_k (<= 4096), Wn = ceil(cap/64), K1 = ncls-1.  Caller-allocated scratch:
 *   probs (N,K1,P) f32; boxes (N,P,6) f32; sorted_idx (N,K1,cap) i32; ncand (N*K1) i32;
 *   mask (N,K1,cap,Wn) u64; keep_bits (N,K1,Wn) u64; nkept (N*K1) i32; tmp_scores (N,K1*cap) f32; tmp_ref same i32;
 *   select_ws: msl_detect_select_ws_ints(N,P,ncls) i32 (score histogram + shortlist of the candidates that can reach the
 *   best cap: the stable order is then found among ~cap candidates instead of all P); per (image, foreground class)
 *   2048 + 4 + P ints: [histogram 2048 | threshold bin | shortlist length | pad 2 | shortlist P]
 * The scratch needs no initialisation: every call sets what it reads (tests/test_gpu_detect.py hands it over poisoned).
 * After a call: ncand = candidates per (image, class); sorted_idx[.., :min(ncand, cap)] = their stable descending order;
 * keep_bits = bit r set if rank r is kept, words beyond the last block of 64 zero; nkept = their popcount.
 * Outputs: out_boxes (N,top_k,6), out_scores (N,top_k), out_labels / out_prior (N,top_k) i64, out_count (N) i32. */
size_t msl_detect_select_ws_ints(int N, int P, int ncls);
int msl_detect_objects(const float* locs, const float* scores, const float* priors_c, int N, int P, int ncls,
                       float min_score, float max_overlap, int top_k, float* probs, float* boxes, int* sorted_idx,
                       int* ncand, unsigned long long* mask, unsigned long long* keep_bits, int* nkept,
                       float* tmp_scores, int* tmp_ref, int* select_ws, float* out_boxes, float* out_scores,
                       long long* out_labels, long long* out_prior, int* out_count, void* stream);

/* ---- detection metrics: calculate_mAP / compute_metrics_per_class (utils.py:157-396), class 1 only ------------
 * Detections in msl_detect_objects' output layout: det_boxes (N,top_k,6) f32, det_scores (N,top_k) f32, det_labels
 * (N,top_k) i64, det_count (N) i32 (slots >= count and labels != 1 are ignored).  Ground truth packed
 * (MultiBoxLoss.pack_targets): gt_boxes (G,6) f32, gt_labels (G) i64, obj_off (N+1) i32 (boxes of image n are
 * [obj_off[n], obj_off[n+1]); labels != 1 ignored).  iou_thr (n_thr) f32: one workgroup per threshold, strict `>`;
 * recall_thr (11) f32: torch.arange(0, 1.1, .1).  D = N*top_k.  Outputs, per threshold t:
 *   summary (n_thr,8): AP, mAP, precision, recall, f1, n_true_boxes, K = class-1 detections, TP count
 *   tp / fp (n_thr,D): first K entries, in sorted order;  gt_status (n_thr,G): 1 detected, 0 not, 2 not class 1
 * and once: sorted_scores (D) (first K), gt_vol (G) (utils.py:152-154).  accum (NULL or n_thr*4+1 f64): += mAP,
 * precision, recall, f1 per threshold, then += 1 (per-step sums of a training epoch).  Bit-identical to the host code.
 * Capacity: msl_detection_metrics_max(0) detections (D), (1) ground-truth boxes (G), (2) thresholds; beyond -> -2. */
size_t msl_detection_metrics_max(int which);
int msl_detection_metrics(const float* det_boxes, const float* det_scores, const long long* det_labels,
                          const int* det_count, int N, int top_k, const float* gt_boxes, const long long* gt_labels,
                          const int* obj_off, int G, const float* iou_thr, int n_thr, const float* recall_thr,
                          float* summary, float* tp, float* fp, float* sorted_scores, float* gt_status, float* gt_vol,
                          double* accum, void* stream);

/* ---- dataset-scale evaluation: the (IoU x score threshold) grid of eval.py, each point calculate_mAP (utils.py:242-396)
 * on the detections with score >= min_score, class 1 only, no cap on detections or ground truth (csrc/evaluate.hip).
 * det_rows (D,8) f32: box(6), score, label (as f32); det_off (N+1) i32: detections of image n are [det_off[n],
 * det_off[n+1]).  Ground truth packed as for msl_detection_metrics.  iou_thr (n_iou) f32 (strict `>`), score_thr (n_sc)
 * f64 (kept iff (double)score >= thr), recall_thr (11) f32.  workspace: _workspace_bytes(...) bytes (0 = unsupported
 * sizes).  out (f32 words): summary (n_iou,n_sc,8) [AP, mAP, precision, recall, f1, n_true_boxes, K_c, TP count] |
 * sorted scores (D) | TP flags in rank order (n_iou,D) | claim rank (n_iou,G) i32: rank of the detection that claimed
 * the box, 0x7fffffff = never, -1 = not class 1 | volumes (G).  Values at (t, c) are those of the first K_c ranks.
 * Bit-identical to the host code while the counts stay below 2^24.  Sizes beyond int32 indexing -> -2. */
size_t msl_evaluate_workspace_bytes(int D, int N, int G, int n_iou, int n_sc);
int msl_evaluate_detections(const float* det_rows, const int* det_off, int D, int N, const float* gt_boxes,
                            const long long* gt_labels, const int* obj_off, int G, const float* iou_thr, int n_iou,
                            const double* score_thr, int n_sc, const float* recall_thr, void* workspace,
                            size_t workspace_bytes, float* out, void* stream);

/* ---- the same with ignored ground truth.  gt_ignore (G) u8 on the device, or NULL: a non-zero
 * byte on a class-1 box makes it "ignored" (a byte on a box of another label has no effect).  An ignored box takes part
 * in a detection's first-maximum-IoU pick like every class-1 box; a detection whose pick is ignored and has IoU > thr is
 * ABSORBED: neither true nor false positive, and it claims nothing (any number may be absorbed by one box).  n_true_boxes
 * counts the class-1 boxes that are not ignored, false negatives are the unclaimed ones among them, and at a score cut
 * FP = K_c - TP - absorbed.  The claim entry of an ignored box is -2.  absorbed (i32, required with gt_ignore):
 * (n_iou, n_sc) absorbed detections among the first K_c ranks | (n_iou, D) absorbed flag per rank.  workspace:
 * _workspace_bytes_ign(...) bytes with gt_ignore (0 for exactly the sizes _workspace_bytes refuses), _workspace_bytes(...)
 * suffice without.  gt_ignore NULL: the launches and results of msl_evaluate_detections, bit for bit; absorbed, when
 * given, is zeroed.  The workspace records whether it carries absorbed flags: msl_evaluate_froc and msl_evaluate_strata,
 * given that workspace WITH ITS FULL SIZE, then leave absorbed detections out of their false positives, and
 * msl_evaluate_strata leaves ignored boxes out of every bin; the caller passes msl_evaluate_froc the per-image counts of
 * class-1 boxes that are not ignored. */
size_t msl_evaluate_workspace_bytes_ign(int D, int N, int G, int n_iou, int n_sc);
int msl_evaluate_detections_ign(const float* det_rows, const int* det_off, int D, int N, const float* gt_boxes,
                                const long long* gt_labels, const int* obj_off, int G, const float* iou_thr, int n_iou,
                                const double* score_thr, int n_sc, const float* recall_thr, void* workspace,
                                size_t workspace_bytes, float* out, const unsigned char* gt_ignore, int* absorbed,
                                void* stream);

/* ---- FROC from a completed msl_evaluate_detections call ("FROC"): eval_workspace is that call's workspace,
 * sorted_scores the sorted-scores part of its result buffer, and D, N, G, n_iou its sizes, on the same stream.  The
 * workspace keeps the rank order, the image of every detection, the TP flag per (IoU threshold, rank) and K.
 * gt_count (N) i32: class-1 ground-truth boxes per image.  weights (R1, N) i32 >= 0: one multiplicity per image and row
 * (row 0 all ones = the plain curve, further rows = bootstrap resamples).  rates (n_rates, 2) i64: numerator and
 * denominator, 1 .. 2^20 each, n_rates <= 16 (more -> -2).  Per (row, IoU threshold, rate): k* = the largest admissible
 * prefix length (0, K, or a cut between two different scores) with FPw(k) * den <= num * Nw, and TPw(k*).
 * out (i64): (R1, n_iou, n_rates, 2) [k*, TPw(k*)] | (R1, 2) [Gw, Nw].  Integer arithmetic only. */
int msl_evaluate_froc(const void* eval_workspace, size_t eval_workspace_bytes, const float* sorted_scores, int D, int N,
                      int G, int n_iou, const int* gt_count, const int* weights, int R1, const long long* rates,
                      int n_rates, long long* out, void* stream);

/* ---- sensitivity and false positives by lesion size from a completed msl_evaluate_detections call ("Eval by
 * lesion size"): eval_workspace / eval_out are that call's workspace and result buffer, D, N, G, n_iou, n_sc its sizes and
 * det_rows, obj_off its inputs, on the same stream; all of them are only read.  The size of a box is its bounding-box
 * volume in f32 (utils.volume: the volumes (G) of eval_out for ground truth, the same expression on det_rows for a
 * detection) times voxels[image] in f64, one rounded multiply; voxels (N) f64 > 0.  edges (n_edges) f64, finite, strictly
 * ascending, n_edges <= 15 (more -> -2): stratum = number of edges <= size, n_edges + 1 strata; a NaN size is unbinned.
 * weights (R1, N) i32 >= 0 as for msl_evaluate_froc.  cuts (R1, n_iou, n_cuts) i64: prefix lengths of the rank order
 * (clamped to 0 .. K), in any order, repeats allowed, n_cuts <= 32 (more -> -2).  strata_workspace: 5 * (D + G) bytes,
 * 4-byte aligned, overwritten.  With S1 = n_edges + 2 slots per cut (the strata, then the unbinned slot), out (i64):
 * (R1, n_iou, n_cuts, S1, 2) [TPw, FPw] | (R1, S1) Gw_s | (R1, 2) [unbinned class-1 detections, Nw], where per slot s
 * TPw = sum over class-1 boxes g of w[img(g)] [claim rank of g < cut], FPw = sum over ranks j < cut of w[img(j)] (1 - tp[j]),
 * Gw_s = sum over class-1 boxes of w[img(g)].  Integer arithmetic only.  Null or inconsistent arguments -> -1. */
int msl_evaluate_strata(const void* eval_workspace, size_t eval_workspace_bytes, const float* eval_out, int D, int N, int G,
                        int n_iou, int n_sc, const float* det_rows, const int* obj_off, const double* voxels,
                        const double* edges, int n_edges, const int* weights, int R1, const long long* cuts, int n_cuts,
                        void* strata_workspace, size_t strata_workspace_bytes, long long* out, void* stream);

/* ---- prior fit report (csrc/priorfit.hip): what the matching of MultiBoxLoss (ssd3d.py:786-887)
 * gives every ground-truth box, for n_thr thresholds at once, without an (N,P) buffer.  gt_boxes (G,6) f32 fractional corner
 * boxes, finite with max >= min per axis, and obj_off (N+1) i32 on the device (msl_multibox_match's layout, any number of
 * boxes per image); priors_c (P,6) f32 centre-size on the device; scale_off (S+1) i32 HOST array of ascending prior-row
 * offsets, scale_off[0] = 0, scale_off[S] = P (one range per feature map); thr (n_thr) f32 HOST array.  S <= 8 and
 * n_thr <= 8 (more -> -2).  workspace: _workspace_bytes(G) bytes, 8-byte aligned, initialised by the call.  Outputs, exactly
 * what the matching implies for the image of box g (oracle/multibox.py:match_image with every label 1):
 *   best_iou (G) f32 / best_prior (G) i32: the maximum IoU of g over all priors and the FIRST prior attaining it (before
 *     the force-match);
 *   held (G) i32: 1 if g is the last box of its image with that best_prior (it keeps the prior the force-match gives it);
 *   pos (G, n_thr, S) i32: the priors p of range s with obj[p] == g and overlap[p] >= thr[t], obj / overlap taken AFTER the
 *     force-match (a forced prior has overlap 1 and belongs to the last claimant, every other prior to the first box with
 *     the maximum IoU).  sum_s pos[g,t,s] = positive priors of g in training; 0 = a box that trains nothing.
 * Two streaming passes over (image, tile of MSL_PRIOR_FIT_TILE priors), the image's boxes staged through LDS
 * MSL_PRIOR_FIT_CHUNK at a time; integer / max-of-keys atomics only: the result does not depend on scheduling.  G = 0
 * launches nothing.  Null or inconsistent arguments -> -1. */
#define MSL_PRIOR_FIT_TILE 1024 /* priors per workgroup */
#define MSL_PRIOR_FIT_CHUNK 64  /* boxes of one image staged in LDS at a time */
#define MSL_PRIOR_FIT_MAX_SCALES 8
#define MSL_PRIOR_FIT_MAX_THRESHOLDS 8
size_t msl_prior_fit_workspace_bytes(int G);
int msl_prior_fit(const float* gt_boxes, const int* obj_off, int N, int G, const float* priors_c, int P, const int* scale_off,
                  int S, const float* thr, int n_thr, void* workspace, size_t workspace_bytes, float* best_iou,
                  int* best_prior, int* held, int* pos, void* stream);

/* ---- device-resident training data (csrc/datapipe.hip, devicedata.py): the host pipeline of datasets._Cases ----------
 * msl_normalize_nonzero: NormalizeIntensity(nonzero=True) in place on n_volumes contiguous f32 volumes of `voxels` each:
 * population mean / std of the non-zero voxels (f64, fixed order), std 0 -> 1, zeros stay zero, all-zero unchanged.
 * msl_augment_resample: dst (N,D,H,W) f32 image / u8 mask from src volumes [0, n_src).  params (N,16) f64 per sample:
 * source volume, source axis of output axes 0..2, reversal of output axes 0..2 (flip / rot90 as one signed axis
 * permutation), affine on (1) / off (0), zoom 0..2, offset 0..2.  With the affine on, output voxel o samples the permuted
 * volume at c = zoom*o + offset as scipy.ndimage.affine_transform(mode="reflect") does: order 1 (image), order 0 (mask).
 * msl_augment_affine: the same with a dense matrix, a boundary mode and intensity arithmetic (datasets._aug_affine with a
 * rotate_range, _aug_shiftintensity, _aug_scaleintensity).  params (N,32) f64 per sample: [0] source volume, [1..3] source
 * axis of output axes 0..2, [4..6] reversal of output axes 0..2, [7] affine on (1) / off (0), [8..16] matrix M row-major,
 * [17..19] offset, both as the host computed them in f64, [20] boundary: 0 reflect, 1 nearest ("border"), 2 constant 0
 * ("zeros"), [21] number of intensity operations (<= 4), [22+2k] kind: 1 add, 2 multiply, [23+2k] its f32 operand,
 * [30..31] unused.  With the affine on, output voxel o samples the permuted volume at M o + offset as
 * scipy.ndimage.affine_transform does (order 1 image, order 0 mask; bit-identical for the three boundaries); the
 * operations then apply to the image value in list order, one rounded f32 operation each.  Affine off: a permuted copy
 * with that arithmetic.  A row whose source volume or axes are invalid writes zeros.
 * msl_seg_boxes: BoundingBoxesGeneratord "classes" mode (datasets.boxes_from_segmentation) on seg (N,D,H,W) u8: per image,
 * classes 1..n_classes (<= 8), 6-connected components in scipy.ndimage.label order, inclusive extents / size, flat ones
 * dropped -> boxes (capacity,6) f32, labels (capacity) i64, obj_off (N+1) i32 (msl_multibox_match's layout).  comp_cap
 * bounds the components before the flat ones are dropped.  *overflow (device): 0, |1 more boxes than capacity, |2 more
 * components than comp_cap; obj_off stays <= capacity.  workspace: _workspace_bytes(...) bytes (0 = unsupported). */
int msl_normalize_nonzero(float* img, int n_volumes, long long voxels, void* stream);
int msl_augment_resample(const float* src_img, const unsigned char* src_seg, int n_src, const double* params, int N,
                         int D, int H, int W, float* dst_img, unsigned char* dst_seg, void* stream);
int msl_augment_affine(const float* src_img, const unsigned char* src_seg, int n_src, const double* params, int N,
                       int D, int H, int W, float* dst_img, unsigned char* dst_seg, void* stream);
size_t msl_seg_boxes_workspace_bytes(int N, int D, int H, int W, int n_classes, int comp_cap);
int msl_seg_boxes(const unsigned char* seg, int N, int D, int H, int W, int n_classes, int capacity, int comp_cap,
                  void* workspace, size_t workspace_bytes, float* boxes, long long* labels, int* obj_off,
                  int* overflow, void* stream);

/* ---- clinical cases (csrc/datapipe.hip, devicedata.LesionCache): the host pipeline of datasets._LesionCases --------
 * msl_foreground_box: box (device, 6 ints) = lo0, lo1, lo2, hi0, hi1, hi2 of datasets.foreground_box on one (D,H,W) f32
 * volume: F = {v : vol[v] > 0}, lo = max(min F - margin, 0), hi = min(max F + margin + 1, n); empty F: the whole volume.
 * msl_augment_fit: dst (N,T0,T1,T2) f32 image / i16 mask from ragged cases kept in two flat arenas of arena_elems
 * elements each (f32 image, i16 mask).  table (device, n_cases x 4 i64): element offset and shape n0, n1, n2 of a case.
 * params: msl_augment_affine's (N,32) f64 rows with [0] = case.  Output voxel o reads voxel q of the permuted case (shape
 * n'), q = clamp(o + d, 0, n' - 1) per axis with d = -((t - n') / 2) where n' < t and n' / 2 - t / 2 otherwise
 * (resize_with_pad_or_crop, edge replication); with the affine on the permuted case is sampled at M q + offset as
 * msl_augment_affine samples it; then the intensity operations.  A row whose case, axes or table entry are invalid
 * writes zeros.
 * msl_instance_boxes: BoundingBoxesGeneratord "instances" mode (datasets.boxes_from_instances) on seg (N,D,H,W) i16, ids in
 * [1, 32767].  thresholds (HOST, n_pairs x 2 ints, n_pairs <= 8, read during the call; inf = INT_MAX): per image, per pair
 * (lo, hi) in order, the ids with lo <= id < hi in ascending order give inclusive extents / size with label = position + 1;
 * the first unique value of an image is discarded (the smallest id where there is no background); flat boxes dropped.
 * Outputs in msl_seg_boxes's layout.  *overflow (device): 0, |1 more boxes than capacity, |4 a negative value in seg;
 * obj_off stays <= capacity.  workspace: _workspace_bytes(N) bytes (0 = unsupported).
 * msl_binary_boxes: BoundingBoxesGeneratord "binary" mode (datasets.boxes_from_instances(seg, [(1, inf)], "binary")) on seg
 * (N,D,H,W) i16: per image, the 6-connected components of the non-zero voxels (negative values count, as for
 * scipy.ndimage.label) in scipy's order - by a component's first voxel in C raster order - give inclusive extents / size
 * with label 1; an image without a background voxel yields no box (its one component is the first unique value, which
 * is discarded); flat boxes - a one-voxel component among them - are dropped, by msl_instance_boxes's arithmetic.
 * Outputs in msl_seg_boxes's layout; rows past obj_off[N] are not touched.  Run-based: the unit of the union-find is a
 * run of consecutive non-zero voxels of a row, the mask is read twice (the second time only its rows with a run) and no
 * per-voxel array is kept.  run_cap bounds the runs of the call (all images together).  *overflow (device): 0, |1 more
 * boxes than capacity, |8 more runs than run_cap (the runs behind it are left out: the rows are then not the mask's);
 * obj_off stays <= capacity and nothing is written outside the buffers.  Integer min / max atomics and order-free links
 * only: the result does not depend on scheduling.  workspace: _workspace_bytes(N, D, H, W, run_cap) bytes =
 * up(4 (N D H + 1)) + 4 up(4 run_cap) + up(20 run_cap) + up(4 N) + 256 with up() rounding to 256 (0 = unsupported).
 * Returns -1 for null pointers, sizes <= 0, capacity < 0 or a workspace too small, -2 for N > 65535, N D H >= 2^31 - 2^16
 * or run_cap > 2^31 / 5, nothing launched in either case. */
int msl_foreground_box(const float* vol, int D, int H, int W, int margin, int* box, void* stream);
int msl_augment_fit(const float* arena_img, const short* arena_seg, long long arena_elems, const long long* table,
                    int n_cases, const double* params, int N, int T0, int T1, int T2, float* dst_img, short* dst_seg,
                    void* stream);
size_t msl_instance_boxes_workspace_bytes(int N);
int msl_instance_boxes(const short* seg, int N, int D, int H, int W, const int* thresholds, int n_pairs, int capacity,
                       void* workspace, size_t workspace_bytes, float* boxes, long long* labels, int* obj_off,
                       int* overflow, void* stream);
size_t msl_binary_boxes_workspace_bytes(int N, int D, int H, int W, int run_cap);
int msl_binary_boxes(const short* seg, int N, int D, int H, int W, int capacity, int run_cap, void* workspace,
                     size_t workspace_bytes, float* boxes, long long* labels, int* obj_off, int* overflow,
                     void* stream);
/* The same for cases of C sequences (1 <= C <= 4, the stem's limit; datasets.LesionsDataModule(input_images=...)).
 * msl_foreground_box_mc: msl_foreground_box on a channel-first (C,D,H,W) volume: F = {v : vol[c][v] > 0 for any c}, the
 * union of the channels' supports; one box for all channels.  C = 1 is msl_foreground_box.
 * msl_augment_fit_mc: msl_augment_fit for C channels in one launch.  arena_seg and table are msl_augment_fit's (seg_elems
 * i16 elements; table: element offset off_k and shape of case k).  arena_img holds C * seg_elems floats: case k is C
 * contiguous planes of n0*n1*n2 voxels starting at element C * off_k.  dst_img (N,C,T0,T1,T2) f32, dst_seg (N,T0,T1,T2)
 * i16.  One set of params per sample: the geometry and the mask are computed once and every channel is resampled with
 * it, then given the same intensity operations; each plane is bit-identical to a C = 1 launch on that plane alone, which
 * is what msl_augment_fit is (the same kernel with seg_elems = arena_elems, C = 1).  A row whose case, axes or table entry
 * are invalid (the case must end at or before seg_elems) writes zeros to all C planes. */
int msl_foreground_box_mc(const float* vol, int C, int D, int H, int W, int margin, int* box, void* stream);
int msl_augment_fit_mc(const float* arena_img, const short* arena_seg, long long seg_elems, int C, const long long* table,
                       int n_cases, const double* params, int N, int T0, int T1, int T2, float* dst_img, short* dst_seg,
                       void* stream);
/* Patch training (datasets.window / patch_origin, devicedata.LesionCache with a patch size).
 * msl_augment_window_mc: msl_augment_fit_mc in every respect (1 <= C <= 4, the same arenas, table, params, outputs and
 * zero rows) except the shift: windows (device, N x 3 i32) gives sample n its own d_k = windows[3n + k] in place of the
 * centred value, so output voxel o reads voxel q = clamp(o + d, 0, n' - 1) of the permuted case: the window of
 * T0 x T1 x T2 voxels at origin d, edge-replicated outside the case.  Any int is an origin (o + d is formed in 64 bits).
 * windows = the fit's shifts gives msl_augment_fit_mc's output bit for bit.  Every output voxel is written exactly once:
 * no memset, no atomics.  -1 (nothing launched, nothing written): windows null, or what msl_augment_fit_mc refuses. */
int msl_augment_window_mc(const float* arena_img, const short* arena_seg, long long seg_elems, int C,
                          const long long* table, int n_cases, const double* params, const int* windows, int N, int T0,
                          int T1, int T2, float* dst_img, short* dst_seg, void* stream);
/* Separable warps (datasets.zoom_table / grid_table, devicedata.WarpStage / warp_numpy).
 * msl_augment_warp_mc: msl_augment_window_mc's arenas, table, (N,32) f64 rows, outputs and zero rows (1 <= C <= 4), with
 * windows null meaning the centred fit of msl_augment_fit_mc.  A row with [7] = 0 is the permuted copy of those two entry
 * points, bit for bit (intensity operations included).  A row with [7] = 2 is a warp: [8] is the element offset of the
 * sample's three coordinate tables in coords (device, coords_len doubles): n'0 + n'1 + n'2 doubles for the permuted case
 * shape n', axis 0 first; [20] the boundary (0 reflect, 1 nearest, 2 constant) and [21..] the intensity operations as in
 * msl_augment_affine's rows.  Output voxel o maps to q = clamp(o + d, 0, n' - 1) and samples the permuted case at the
 * coordinate (t_0[q_0], t_1[q_1], t_2[q_2]): scipy's boundary map, taps and weights as msl_augment_affine forms them
 * from a coordinate (scipy.ndimage.map_coordinates), order 1 for every image plane and order 0 for the mask, then the
 * intensity operations.  One difference: under boundary 1 the weights come from the coordinate as it is and only the
 * taps are clamped, which is scipy's "nearest" to the bit (msl_regrid's rule); msl_augment_affine clamps the coordinate,
 * which rounds to another f32 at half-integer coordinates past an end - a zoom's tables hold those.  Any other [7] (an affine's 1 among them), an invalid case or axis list, or tables that do
 * not lie inside [0, coords_len) write zeros to the row.  Taps are clamped into the axis whatever the coordinate is: a
 * non-finite table value is outside the contract but reads inside the case.  Every output voxel is written exactly
 * once: no memset, no atomics.  -1 (nothing launched, nothing written): a null pointer other than windows, a size or
 * coords_len < 1, C outside 1..4.  -2: N > 65535 or T0 * T1 >= 2^31 - 4. */
int msl_augment_warp_mc(const float* arena_img, const short* arena_seg, long long seg_elems, int C,
                        const long long* table, int n_cases, const double* params, const double* coords,
                        long long coords_len, const int* windows, int N, int T0, int T1, int T2, float* dst_img,
                        short* dst_seg, void* stream);
/* Free-form deformation (datasets.deform_lattice / deform_coords, devicedata.DeformStage / deform_numpy; DESIGN.md
 * section 4.15).  msl_augment_deform_mc: msl_augment_warp_mc's arenas, table, (N,32) f64 rows, windows, outputs, zero
 * rows and return codes.  A row with [7] = 0 is the permuted copy of msl_augment_fit_mc / msl_augment_window_mc, bit for
 * bit (intensity operations included).  A row with [7] = 3 is a deformation: [8] is the element offset of the sample's
 * lattice P in lattices (device, lattices_len doubles): 3 L^3 doubles [m][i0][i1][i2], component m displacing along axis
 * m of the permuted case; [9] is L, the control points per axis (4 .. 16); [20] the boundary (1 is sampled as scipy's
 * "nearest", as msl_augment_warp_mc samples it) and [21..] the intensity operations.  Output voxel o maps to q =
 * clamp(o + d, 0, n' - 1) and samples the permuted case at q + d(q), d the cubic B-spline of P, every operation one
 * rounded f64 operation in a fixed order: per axis a, u = q_a (L - 3) / (n'_a - 1) (0 where n'_a = 1), cell =
 * min(floor(u), L - 4), t = u - cell, b0 = (1 - t)^3 / 6, b1 = (3 t^3 - 6 t^2 + 4) / 6, b2 = (-3 t^3 + 3 t^2 + 3 t + 1) / 6,
 * b3 = t^3 / 6; d_m = sum_k b[2][k] * (sum_j b[1][j] * (sum_i b[0][i] * P[m][cell_0 + i][cell_1 + j][cell_2 + k])), each
 * sum from 0.0 upwards.  Any other [7] (an affine's 1 and a warp's 2 among them), an invalid case or axis list, an L
 * outside 4 .. 16 or a lattice that does not lie inside [0, lattices_len) write zeros to the row.  cell is clamped into
 * [0, L - 4] and the taps into the axis, so a non-finite lattice value is outside the contract but reads inside the
 * lattice and the case.  Every output voxel is written exactly once: no memset, no atomics.  -1 (nothing launched,
 * nothing written): a null pointer other than windows, a size or lattices_len < 1, C outside 1..4.  -2: N > 65535 or
 * T0 * T1 >= 2^31 - 4. */
int msl_augment_deform_mc(const float* arena_img, const short* arena_seg, long long seg_elems, int C,
                          const long long* table, int n_cases, const double* params, const double* lattices,
                          long long lattices_len, const int* windows, int N, int T0, int T1, int T2, float* dst_img,
                          short* dst_seg, void* stream);

/* ---- native grid -> LPI at 1 mm (csrc/datapipe.hip, devicedata.LesionCache / LesionPredictFeed)
 * msl_regrid: datasets.regrid of one case, bit for bit.  src_img (C,n0,n1,n2) f32 with 1 <= C <= 4, src_seg (n0,n1,n2)
 * i16 -> dst_img (C,m0,m1,m2) f32, dst_seg (m0,m1,m2) i16.  plan (HOST, 12 doubles, read during the call): ax[3],
 * rev[3], step[3], start[3] of datasets.regrid_plan.  The reoriented volume has source axis ax[k] as its axis k,
 * reversed where rev[k] = 1; output voxel o samples it at c_k = step_k * o_k + start_k (one rounded f64 multiply, one
 * rounded add, no contraction) as scipy.ndimage.affine_transform(mode="nearest") does: order 1 for every image plane,
 * order 0 for the mask.  Either the image pair or the mask pair may be null.  Every output voxel is written exactly once:
 * no memset, no atomics.  -1 (nothing launched, nothing written): plan null, both pairs null or a pair half null, ax not
 * a permutation of 0..2, rev not 0 / 1, a size < 1, C outside 1..4, a step not finite or <= 0, a start not finite.
 * -2: m2 > 65535 * 1024. */
int msl_regrid(const float* src_img, const short* src_seg, int C, int n0, int n1, int n2, const double* plan, int m0,
               int m1, int m2, float* dst_img, short* dst_seg, void* stream);

/* ---- MR acquisition stage (csrc/mraug.hip, devicedata.MRStageRunner / mr_tables) ----
 * msl_augment_mr: Gaussian blur, multiplicative bias field and additive noise on a built batch, out of place: src and
 * dst (N,C,D,H,W) f32, bit-identical to datasets.gaussian_smooth / bias_field / gaussian_noise.  All device tables:
 * params (N,8) f64 per sample: [0] flags (1 blur + 2 bias + 4 noise), [1..3] the blur radii R_0..R_2 (clamped to 0..8),
 * [4] the noise deviation (an f32 value), [5] [6] the Philox key words k0, k1 (32-bit values); taps (N,3,17) f32, axis a
 * of sample n in [n][a][0 .. 2 R_a]; lattice (N,L,L,L) f32 with 2 <= L <= 9.  The host computes the taps and the lattice
 * (datasets.gaussian_taps / bias_lattice): the device evaluates no exponential.
 *   blur: three passes over axis 0, 1, 2 of every channel; each acc = 0.0 (f64), acc += (double)w[k] * (double)v[i+k-R]
 *     for k ascending, a tap outside the axis contributing nothing, and one rounding to f32.  Axis 0 is a launch of its
 *     own into the workspace; axes 1 and 2 are fused through an LDS tile with a halo of R.
 *   bias: voxel o samples the lattice at x_a = o_a (L-1) / (n_a-1) in f64 (0 where n_a = 1) with the taps, weights and
 *     eight-corner sum of msl_augment_affine (csrc/resample.hpp); field = (float)sum; v * field, one f32 multiply.
 *   noise: Philox4x32-10 under key (k0,k1) of counter (d H W + h W + w, channel, 0, 0); S = the sum of the eight 16-bit
 *     halves of the four output words; z = (float)(S - 262140) * f32(1 / sqrt(8 (2^32 - 1) / 12)); v + z * std: three
 *     rounded f32 operations.
 * Bias and noise are the epilogue of the last blur pass, or of the copy for a sample without blur; a sample that drew
 * nothing is copied.  Every output voxel is written exactly once: no memset, no atomics.  Two launches on `stream`, no
 * synchronisation.  workspace: msl_augment_mr_workspace_bytes(N,C,D,H,W) bytes (0 for sizes the entry point refuses).
 * -1 (nothing launched): a null pointer, src == dst, a size < 1, L outside 2..9, a workspace too small.  -2 (nothing
 * launched): D H W >= 2^32 (the counter's index word), N C > 65535. */
size_t msl_augment_mr_workspace_bytes(int N, int C, int D, int H, int W);
int msl_augment_mr(const float* src, const double* params, const float* taps, const float* lattice, int N, int C, int D,
                   int H, int W, int L, float* dst, void* workspace, size_t workspace_bytes, void* stream);

/* ---- lesionpaste (csrc/lesionpaste.hip, devicedata.LesionCache) ----
 * msl_paste_lesions: copy-paste of cached lesions on to a built batch, in place, bit-identical to datasets.paste_lesions.
 * arena_img, arena_seg, seg_elems, C, table, n_cases: the arenas of msl_augment_fit_mc (1 <= C <= 4).  img (N,C,T0,T1,T2)
 * f32 and seg (N,T0,T1,T2) i16 are the built batch; report (N,K) i32.  rows (device): N x K rows of 13 + 3 n_cand ints,
 *   [0] active (0: the row is skipped), [1] donor case, [2..4] min_0..2 and [5..7] e_0..2: the donor box, e voxels from
 *   min on, in the donor case, [8] flips (bit a: axis a of the box is mirrored), [9] the mask value written (1 .. 32767),
 *   [10..12] the destination of the donor box's centre voxel relative to the destination corner (in [0, e)), then per
 *   candidate j the destination corner lo_0..2 at [13 + 3 j].
 * One workgroup per sample applies its K rows in order, each on the mask the earlier ones left.  The first candidate is
 * taken whose (a) box [lo - 1, lo + e] clamped to the sample holds no non-zero voxel of seg and (b) image voxel at
 * lo + [10..12] is != 0 in every channel.  With p in [-1, e] per axis, destination voxel lo + p has the donor coordinate
 * d_a = min_a + (flip_a ? e_a - 1 - p_a : p_a).  Written voxels - p inside the box, donor mask at d non-zero: img = the donor's
 * value in every channel, seg = [9].  Rim voxels - inside the sample, not written, a 6-neighbour of a written voxel, d inside
 * the donor case: img = 0.5f * img + 0.5f * donor (two rounded products, one rounded sum; no contraction), seg unchanged.
 * report: the accepted candidate's index, -1 when none passed, -2 for a refused row, which writes nothing: [0] = 0, a case
 * outside [0, n_cases) or a table entry outside the arena, a donor box not inside the case's table shape, an extent > 32 or
 * < 1, [9] outside 1 .. 32767, [10..12] outside the box, or any candidate that would put the box outside the sample.  One
 * launch on `stream`, no synchronisation, no atomics.  -1 (nothing launched): a null pointer, a size < 1.  -2 (nothing
 * launched): C > 4, K > 8 or n_cand > 16. */
int msl_paste_lesions(const float* arena_img, const short* arena_seg, long long seg_elems, int C, const long long* table,
                      int n_cases, const int* rows, int N, int K, int n_cand, int T0, int T1, int T2, float* img,
                      short* seg, int* report, void* stream);

/* ---- prediction overlays (csrc/overlay.hip, devicedata.LesionPredictFeed, predict.py -si 1) ----
 * Packed detections of N images: boxes (K,6) f32 corner boxes, labels (K) i64, scores (K) f32 on the device; offsets
 * (HOST, N + 1 ints, read during the call): image n owns rows offsets[n] .. offsets[n+1].  Both launch on `stream` and
 * do not synchronise.
 * msl_boxes_to_case: datasets.fit_to_case_frame, bit for bit.  geometry (HOST, N x 12 ints, read during the call): per
 * image the fitted size t[3], the cropped size n[3], the crop origin lo[3] and the case's size s[3].  Per axis
 * d = -((t - n) / 2) where n < t and n / 2 - t / 2 otherwise; every coordinate c of that axis becomes
 * (c * t + (d + lo)) / s: one f32 multiply, one add, one divide, each rounded, no contraction.  Not clamped.
 * -1: N < 1, a negative or decreasing offset, a size < 1 or an origin < 0.  out may be boxes.
 * msl_draw_boxes: utils.draw_boxes, bit for bit.  instances / classes (N,D,H,W) i16 (classes may be null); style 0
 * "edges" (the reference's make_segmentation_from_bboxes), 1 "preds" (its save_predictions_example, which also skips
 * scores < min_score).  Voxel box = trunc(clip(box, 0, 1) * size) as an f32 product, max = min(max + style, size - 1).
 * Every voxel of both planes is written exactly once (no memset needed): j + 1 and the label of the last box of the
 * image, counting skipped ones, whose assignments cover it, else 0.  -1 (nothing written): style not 0 / 1, a size
 * < 1, N < 1, a negative or decreasing offset, more than 32766 boxes in one image (j + 1 is an int16). */
#define MSL_DRAW_BOXES_CHUNK 256 /* boxes a workgroup stages in LDS at a time */
int msl_boxes_to_case(const float* boxes, const int* offsets, const int* geometry, int N, float* out, void* stream);
int msl_draw_boxes(const float* boxes, const long long* labels, const float* scores, const int* offsets, int N, int D,
                   int H, int W, int style, double min_score, short* instances, short* classes, void* stream);

/* ---- multi-view prediction (csrc/views.hip, LSSD3D.predict_views, predict.py --views tiles) ----
 * A view is a window of T0 x T1 x T2 voxels at origin o of a case, optionally mirrored along some axes.  views (HOST,
 * V x 6 ints, read during the call): rows o0, o1, o2, f0, f1, f2 (datasets.view_plan).  Both launch on `stream` and do
 * not synchronise.
 * msl_view_gather: datasets.gather_views, bit for bit.  src (C,n0,n1,n2) f32, dst (V,C,T0,T1,T2) f32.  Output voxel p of
 * view v reads src[c][s] with q_k = f_k ? T_k - 1 - p_k : p_k and s_k = clamp(o_k + q_k, 0, n_k - 1).  Every output
 * voxel is written exactly once: no memset, no atomics.  -1 (nothing launched, nothing written): a null or misaligned
 * pointer, V < 1, a size < 1, C outside 1..4, a flip flag not 0 / 1.  -2: C * T0 > 65535 or T1 * (T2 / 4 + 2) >= 2^31.
 * msl_views_merge: utils.merge_views, bit for bit.  boxes (V,top_k,6) f32, scores (V,top_k) f32, labels (V,top_k) i64,
 * counts (V) i32 on the device: the detections of the V views in msl_detect_objects' output layout (corner boxes as
 * fractions of the view).  geometry (HOST, 12 ints, read during the call): tile[3], case[3], margin[3], V, top_k,
 * out_top_k.  All f32 arithmetic is single rounded operations, no contraction.  Map, per axis k: a corner pair (a, b) of a
 * view with f_k becomes (1 - b, 1 - a); voxel x = a * T_k + o_k; case fraction x / n_k; not clamped.  Candidates: slots
 * j < counts[v] with label >= 1 and a score that is not NaN whose centre (x_lo + x_hi) * 0.5f passes the ownership test of
 * their view: on every axis c >= o_k + m_k unless o_k <= 0, and c < o_k + T_k - m_k unless o_k + T_k >= n_k.  Per class,
 * ascending: rank by descending score, ties by ascending (view, slot); greedy NMS with iou > max_overlap (detect.hip's
 * iou6) on the case-frame boxes; a suppressed candidate is assigned to the earliest-ranked kept one that overlaps it;
 * support = distinct views among a kept candidate and its members.  mode 0 "nms": the kept candidate's box and score.
 * mode 1 "fuse": box = sum(s_i * B_i) / sum(s_i) over the cluster in rank order (f64: one rounded multiply and add per
 * term, one divide, rounded to f32); score = sum over views, ascending, of the view's best member score (f64) over
 * max(cover, support), cover = views whose ownership test the kept centre passes, rounded to f32.  Output: every class, by
 * descending final score, ties by (class, rank of the kept candidate), the first out_top_k: out_boxes (out_top_k,6),
 * out_scores, out_labels i64, out_support i32, out_count (1), possibly 0; rows past the count are not written.
 * workspace: msl_views_merge_workspace_bytes(V, top_k) bytes, 16-byte aligned; 0 = beyond capacity (V > 64 or
 * V * top_k > 8192: 2 x 2 x 2 tiles x 8 flips x top_k 100 = 6400).  -1 (nothing launched): a null pointer, V, top_k or
 * out_top_k < 1, a size < 1, a margin < 0, a flip flag or mode not 0 / 1, a workspace too small.  -2: beyond capacity. */
#define MSL_VIEWS_MAX 64
#define MSL_VIEWS_MAX_DETECTIONS 8192
int msl_view_gather(const float* src, int C, int n0, int n1, int n2, const int* views, int V, int T0, int T1, int T2,
                    float* dst, void* stream);
size_t msl_views_merge_workspace_bytes(int V, int top_k);
int msl_views_merge(const float* boxes, const float* scores, const long long* labels, const int* counts, const int* views,
                    const int* geometry, float max_overlap, int mode, void* workspace, size_t workspace_bytes,
                    float* out_boxes, float* out_scores, long long* out_labels, int* out_support, int* out_count,
                    void* stream);

/* ---- optimiser + NaN guard : ssd3d.py:704-722, :258-261 ---------------------------------------------------- */
/* hp (device, 8 floats): step_size(bias), step_size(other), sqrt(bias_correction2), beta1, beta2, eps,
 * weight_decay, gradient scale.  is_bias (n bytes): 1 for elements of '.bias' parameters (2*lr group). */
int msl_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const float* hp,
                  const unsigned char* is_bias, int n, void* stream);
int msl_nan_flag(const float* x, size_t n, int* flag, int bit, void* stream);
/* the same for two tensors in one launch: *flag |= bit_a if a holds a NaN, |= bit_b if b does */
int msl_nan_flag2(const float* a, size_t na, int bit_a, const float* b, size_t nb, int bit_b, int* flag, void* stream);
/* Batched gradient reduction (autograd's accumulation of the conv weight gradients, ssd3d.py:467-531 backward): the
 * weight-gradient kernels leave partial sums (fp32 slabs / fp64 partials) in their workspaces; ONE launch folds the
 * listed ones into the flat gradient arena in a fixed order.  The table is built on the host with _table_set (which
 * returns the number of workgroups of the entry; first_block = running sum) and uploaded by the caller.
 * kind 0: fp32 slabs [nslabs][stride] -> dst[i];  1: fp64 partials [count][nslabs] -> dst[i];  2: stem slabs, padded
 * [32][32*p1] image -> dst[co*p0 + k];  3: head slabs -> dst = dloc_w, dst2 = dcl_w (p0 = C, p1 = MT, p2 = 12 + 2*ncls);
 * 4: the loss partials of msl_multibox_loss_pack (src fp64 [nslabs][2], dst2 = its int positives counter, count = 1)
 * -> dst = loss_out [conf_loss, loc_loss, n_positives]. */
size_t msl_grad_reduce_entry_bytes(void);
int msl_grad_reduce_table_set(void* host_table, int index, int first_block, int kind, const void* src, float* dst,
                              float* dst2, int nslabs, int count, long long stride, int p0, int p1, int p2);
int msl_grad_reduce_batch(const void* table, int n_entries, int total_blocks, void* stream);
/* the same; block_entry[total_blocks] (device) names every workgroup's table entry, so no workgroup searches the table */
int msl_grad_reduce_batch_indexed(const void* table, int n_entries, const int* block_entry, int total_blocks, void* stream);
/* ---- per-tensor histograms and moments : ssd3d.py:729-738 (on_after_backward, add_histogram) ------------------- */
/* One pass over n_src (1 .. 4) flat fp32 device arrays that share one segment table: segment s is elements
 * [seg_off[s], seg_off[s] + seg_len[s]) of every source (seg_off (n_seg) i64, seg_len (n_seg) i32, device).  Outputs, per
 * (source k, segment s), at index k * n_seg + s:
 * hist (x 128 i32), keyed on the fp32 bit pattern with integer operations only: bin 0 non-finite (NaN, +-Inf), 1 +-0,
 * 2 + c negative and 65 + c positive finite non-zero values of magnitude class c = clamp(E - 127, -42, 20) + 42 for a
 * normal number with biased exponent field E (floor(log2|x|) clamped to [-42, 20]), c = 0 for a subnormal;
 * moments (x 5 f64) over the finite values: sum, sum of squares, sum of magnitudes, min, max (+inf / -inf if none).
 * Every output word is (re)written by each call - the caller clears nothing - and results are run-to-run bit-identical
 * (integer adds for the bins; the f64 sums go through per-workgroup partials folded in a fixed order, no float atomics).
 * A workgroup takes one chunk of msl_tensor_stats_chunk() elements of one segment, named by block_table (device copy of
 * what msl_tensor_stats_block_table fills on the HOST: n_seg + 1 prefix sums "first workgroup of segment s", then
 * (segment, chunk) per workgroup); that helper returns n_blocks (0: a null pointer, n_seg < 1, a length < 1, a table
 * capacity below n_seg + 1 + 2 * n_blocks ints) and only counts when host_table is NULL.  partials: workspace of
 * msl_tensor_stats_workspace_bytes(n_src, n_blocks) bytes, 8-byte aligned (0: bad argument).
 * -1 (nothing launched): a null or misaligned pointer, n_src outside 1 .. 4, n_seg outside 1 .. 65535, n_blocks < n_seg. */
#define MSL_TENSOR_STATS_BINS 128
#define MSL_TENSOR_STATS_CHUNK 4096
#define MSL_TENSOR_STATS_MAX_SOURCES 4
size_t msl_tensor_stats_chunk(void);
size_t msl_tensor_stats_block_table(const int* seg_len, int n_seg, int* host_table, size_t capacity_ints);
size_t msl_tensor_stats_workspace_bytes(int n_src, int n_blocks);
int msl_tensor_stats(const float* src0, const float* src1, const float* src2, const float* src3, int n_src,
                     const long long* seg_off, const int* seg_len, int n_seg, const int* block_table, int n_blocks,
                     double* partials, int* hist, double* moments, void* stream);
/* stream fork/join (hipEvent with timing disabled): record on the producer stream, wait on the consumer stream */
int msl_event_create(void** out);
int msl_event_create_device(void** out);                      /* orders streams of ONE device only (hipEventDisableSystemFence): never for host waits or other devices */
/* Fork without a record packet: the (skip + 1)-th kernel launch the calling THREAD issues from now on completes `ev`
 * (stopEvent of hipExtLaunchKernel) exactly as if msl_event_record(ev, <that launch's stream>) followed it.
 * msl_thread_launch_count(): kernel launches issued by the calling thread so far (launches per entry point = difference
 * around a call); msl_stop_event_pending(): 1 while an armed event has not met its launch. */
int msl_arm_stop_event(void* ev, int skip);
int msl_stop_event_pending(void);
int msl_thread_launch_count(void);      /* not an error code: the count, modulo 2^31 */
int msl_event_create_timed(void** out);                       /* timing-enabled event (launch-duration measurements) */
int msl_event_elapsed_ms(void* start, void* stop, float* out_ms);
int msl_event_destroy(void* ev);
int msl_event_record(void* ev, void* stream);
int msl_stream_wait_event(void* stream, void* ev);
/* native replay of a recorded launch sequence (generated trampolines, csrc/gen_runner.py): fn_ids from
 * msl_program_fn_id(); slots = n x stride raw 64-bit argument values; *failed_at = index of the failing call */
int msl_program_fn_id(const char* name);
int msl_run_program(const int* fn_ids, const unsigned long long* slots, int stride, int n, int* failed_at);
/* the same issued by two host threads: calls with lane[i] == 1 (the side streams' work) go to a persistent worker thread,
 * lane 0 (the dependency chain's stream) stays with the caller; wait_for[i] >= 0 names the msl_event_record entry that
 * must have been issued before the msl_stream_wait_event of entry i.  Every stream must belong to one lane.  Callers are
 * serialised internally (one worker thread, one posted program at a time): safe from several host threads. */
int msl_run_program_mt(const int* fn_ids, const unsigned long long* slots, int stride, int n, const int* lane,
                       const int* wait_for, int device, int* failed_at);
/* asynchronous 32-bit fill (used to clear flags / counters inside a launch sequence) */
int msl_fill_u32(void* dst, unsigned int value, size_t count, void* stream);

#ifdef __cplusplus
}
#endif
#endif
