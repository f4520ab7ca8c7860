/* eegldm.h -- C ABI of libeegldm.so: MI355X (gfx950) kernels and model executors for
 * the latent-diffusion hot path of the reference repository
 * (AutoencoderKL + PatchDiscriminator train step, UNet denoiser train step, DDIM sampling).
 *
 * The reference has no FFI layer: its boundary is the PyTorch nn.Module / callable
 * protocol of its entry scripts.  Each group below names the reference interface it
 * stands behind (file:line under /root/reference).  A Python binding mirroring those
 * classes lives in the package (`eegldm/`); INTEGRATION.md shows the ctypes stub a
 * reference maintainer would add.
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer unless the name ends in _host.  The caller owns
 *    all tensors, parameters, gradients and optimizer state; the library owns only the
 *    context workspace and the opaque handles.  No hidden host copies.
 *  - All calls enqueue on the context's HIP stream and return; a context is not
 *    thread-safe; one context + one process per GPU.
 *  - Return value 0 = ok, negative = error code; eegldm_last_error() gives the
 *    thread-local message.  No C++ exception crosses this ABI.  Shapes / dtypes are
 *    validated before any launch.
 *  - "NCL" = the reference's contiguous (batch, channel, length) tensors.
 *    "NLC" = the engine's internal layout: rows = (sample, position), channels
 *    contiguous, explicit leading dimension `ld` in elements (so channel-concats are
 *    views).  Model-level entry points take/return NCL fp32 like the reference;
 *    primitive entry points work on NLC.
 *  - Convolution weights are held packed as [K][Cout][Cin] (tap-major); eegldm_pack_*
 *    converts from/to the reference (Cout, Cin, K) layout.
 *  - Random draws (noise, eps, timesteps) are inputs, so device and oracle runs see
 *    identical values; eegldm_randn / eegldm_randint fill them on-device for perf runs.
 */
#ifndef EEGLDM_H
#define EEGLDM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* 4: + eegldm_ctx_stream, eegldm_linear_bwd, eegldm_disc_feature, eegldm_usleep_*, eegldm_feature_moments (additive).
 * 6 (round 5): + EEGLDM_F16, eegldm_conv1d_skip_fwd, eegldm_conv1d_fwd_qstats, eegldm_groupnorm_fwd_qstats, eegldm_batchnorm_lrelu_*,
 *    eegldm_kl_reparam_*, eegldm_conv1d_pack_kblocked_k, eegldm_avgpool2_*, eegldm_nearest2_* (additive).
 * 7 (round 6): + eegldm_resblock_create / eegldm_attnblock_create / eegldm_block_*, eegldm_timestep_embedding (primitive-granular UNet blocks),
 *    eegldm_conv1d_fwd_gn (GroupNorm + SiLU on the conv's operand load), eegldm_conv1d_pack_stride2; REMOVED: eegldm_conv1d_fwd_qstats and
 *    eegldm_groupnorm_fwd_qstats (round 5's GroupNorm-from-producer-moments path measured no gain and was taken out, HISTORY.md).
 * 8 (round 6): eegldm_unet_cfg grows by num_head_channels, num_heads_upsample, use_scale_shift_norm, resample_layers, resample_pool_only
 *    (zero = the config_ldm.yaml behaviour); eegldm_resblock_create gains use_scale_shift_norm, eegldm_attnblock_create gains num_heads;
 *    + eegldm_ddim_step_eta, eegldm_ddpm_step_var, eegldm_unet_set_dropout, eegldm_dropout.
 *    Added since without a version change (new symbols only): the class-conditional entry points, the weight EMA (eegldm_adam_step_ema,
 *    eegldm_ema_update, eegldm_swap), the multistep sampler (eegldm_multistep_step, eegldm_sample_multistep) and editing (eegldm_edit_step,
 *    eegldm_edit_start, eegldm_edit_window, eegldm_sample_edit) and the weighted diffusion loss (eegldm_diffusion_loss, eegldm_loss_bins,
 *    eegldm_ldm_train_step_weighted) and global gradient-norm clipping (eegldm_grad_norm, eegldm_adam_step_clip, eegldm_grad_scale_by)
 *    and long recordings (eegldm_canvas_gather, eegldm_canvas_step, eegldm_canvas_compose, eegldm_sample_long) and their editing
 *    (eegldm_canvas_edit_step, eegldm_sample_long_edit) and resampled repair (eegldm_edit_jump, eegldm_sample_edit_resample,
 *    eegldm_sample_long_edit_resample) and context conditioning (eegldm_unet_create_ctx, eegldm_unet_set_context, eegldm_context_mask,
 *    eegldm_add_noise_context, eegldm_context_window, eegldm_ldm_train_step_ctx, eegldm_sample_edit_ctx, eegldm_sample_long_edit_ctx)
 *    and the developer entries of the fused frozen encoder (eegldm_debug_pre_conv3, eegldm_debug_sample_stats, eegldm_debug_aekl_encode_route)
 *    and the sampling loop by descriptor (eegldm_sample_desc, eegldm_sample_run), of which every eegldm_sample_* export is a shorthand. */
#define EEGLDM_ABI_VERSION 8

/* Storage / operand type of activations and compute-copy weights (accumulation, statistics, master weights and optimizer state are
 * always fp32).  EEGLDM_F16 = IEEE half: the type the reference trains in under `autocast` (src/training/training.py:423) with its
 * GradScaler (:334,441-443); every kernel family is instantiated for it (general, big-tile, fused attention, weight-stationary and
 * few-row convs, fused frozen encoder, pipelined GroupNorm backward) and it runs at bf16 speed. */
enum { EEGLDM_F32 = 0, EEGLDM_BF16 = 1, EEGLDM_F16 = 2 };
enum {
  EEGLDM_OK = 0,
  EEGLDM_ERR_INVALID = -1,
  EEGLDM_ERR_HIP = -2,
  EEGLDM_ERR_UNSUPPORTED = -3,
  EEGLDM_ERR_NOMEM = -4
};
enum { EEGLDM_PRED_EPSILON = 0, EEGLDM_PRED_V = 1, EEGLDM_PRED_SAMPLE = 2 };

typedef struct eegldm_ctx eegldm_ctx;
typedef struct eegldm_unet eegldm_unet;
typedef struct eegldm_aekl eegldm_aekl;
typedef struct eegldm_disc eegldm_disc;
typedef struct eegldm_block eegldm_block;

/* ------------------------------------------------------------------ library / context */
int eegldm_abi_version(void);
const char* eegldm_last_error(void);
/* hip_stream: the hipStream_t to enqueue on (e.g. torch's current stream; NULL = the
 * device's default stream, which is what torch uses unless told otherwise).
 * own_stream != 0: ignore hip_stream and create a private non-blocking stream. */
int eegldm_ctx_create(int hip_device, void* hip_stream, int own_stream, eegldm_ctx** out);
/* The stream the context enqueues on: `hip_stream` as given, or the library's own non-blocking stream when own_stream != 0. */
void* eegldm_ctx_stream(const eegldm_ctx*);
int eegldm_ctx_destroy(eegldm_ctx* ctx);
int eegldm_ctx_sync(eegldm_ctx* ctx);
/* HIP-event timing on the context's stream (bench.py measures kernels with these, since
 * torch.cuda.Event only sees torch's current stream). */
int eegldm_timer_start(eegldm_ctx* ctx);
int eegldm_timer_stop_ms(eegldm_ctx* ctx, float* ms_host);
/* Per-launch profiling of the MFMA GEMM / implicit-conv family: while enabled, every launch
 * is bracketed by HIP events on the context's stream.  eegldm_prof_summary returns, for one
 * kernel class (0 conv fwd, 1 conv dgrad, 2 conv wgrad, 3 gemm NT, 4 gemm NN, 5 gemm TN),
 * the summed algorithmic FLOPs (2*M*N*K*taps), summed kernel time and launch count since
 * eegldm_prof_enable(ctx, 1).  Host outputs.  Enabling also measures the elapsed time of an EMPTY
 * event pair on the stream (median of 33); the summary subtracts it once per launch so that the
 * durations are the kernels' own (they then agree with a rocprofv3 kernel trace of the same run);
 * eegldm_prof_bracket_overhead_ms reports that calibration value. */
int eegldm_prof_enable(eegldm_ctx* ctx, int on);
int eegldm_prof_summary(eegldm_ctx* ctx, int kernel_class, double* flops_host, double* ms_host, int* launches_host);
int eegldm_prof_bracket_overhead_ms(eegldm_ctx* ctx, double* ms_host);
/* developer aid: CSV of every profiled launch (class,M,N,K,taps,splitk,ms,gflop) */
int eegldm_prof_dump(eegldm_ctx* ctx, const char* path_host);
/* Developer switches (EEGLDM_* environment variables, README "Developer switches") are cached on first use;
 * eegldm_debug_reload_env() makes every one of them be read again on its next use (returns the new epoch).  Tests use it to
 * A/B an execution path against its predecessor inside one process.  Models / contexts created BEFORE the call keep whatever
 * they built from the old values (weight copies, streams).  No reference counterpart. */
int eegldm_debug_reload_env(void);
/* developer aid: the kernel that served the calling thread's last eegldm_groupnorm_fwd (backward = 0) / _bwd (1) launch, as six ints:
 * family (1 split kernels, 2 register-resident, 3 pipelined persistent backward, 4 flat G = 1, 5 wide flat forward), 4-wide loads (1 / 0),
 * threads per block, rows- (flat: chunks-) per-thread instantiation, chunk width in channels, XCD-aware block order (1 / 0).
 * The route-aware tests confirm from it that a case ran on the kernel it names.  No reference counterpart. */
int eegldm_debug_gn_last_route(int backward, int* out6_host);
/* developer aid: what the calling thread's last ResBlock forward and backward (eegldm_block_forward / _backward, or the last ResBlock of a
 * model's step) decided, as twelve ints:
 *   [0]     forward form: 1 GroupNorm -> conv -> GroupNorm -> conv, 2 the same with use_scale_shift_norm, 3 the few-row eval form
 *   [1..3]  backward of the second GroupNorm: family (as eegldm_debug_gn_last_route), chunk width in channels, body (1 the straight-line
 *           full-slab kernel, 2 the predicated one, 0 outside the register-resident family);   [4..6] the same for the first GroupNorm
 *   [7]     who wrote the per-sample column sums behind the embedding gradient: 0 nobody, 1 the GroupNorm backward, 2 the column-sum
 *           kernel over the stored gradient, 3 the FiLM backward (use_scale_shift_norm)
 *   [8..10] who added the gradient of out_layers.3.bias, skip_connection.bias, in_layers.2.bias: 0 no such parameter (or no parameter
 *           gradients), 1 a column-sum kernel straight into it, 2 the weight-gradient GEMM, 3 the total of the per-sample sums, 4 the
 *           staged vector both output-side biases can share
 *   [11]    1 when the column-sum kernels were the ordered ones of EEGLDM_DETERMINISTIC=1
 * It records decisions only; no launch depends on it.  No reference counterpart. */
int eegldm_debug_res_last_route(int* out12_host);
/* developer aids of the time-embedding MLP kernels (EEGLDM_NO_EMB_MLP=1 runs the general GEMM path instead).  No reference
 * counterparts.
 * _launches: kernels of the purpose-built path launched by this process so far (reset != 0: and start again from zero).
 * _plan (no device needed): the launch arithmetic for n rows, as twelve ints: tiles of the three forward products, tiles of the weight
 *   gradients of emb_layers / time_embed.2 / time_embed.0, tiles of dsemb, its split-K count, the reduction length of one split, tiles of
 *   dh1, and the floats of backward work space (low 31 bits, high bits).
 * _embed: the embedding chain as every forward and the sampler's table run it: table [n][E] (E = every ResBlock's projection width),
 *   work = the tape [e0 (n x mc) | h1 | a1 | emb | semb (n x 4 mc each)].  labels_dev: class-conditional models only.
 * _embed_backward: the chain's backward from demb_all [n][E] and the tape that _embed left in `work`; adds into the bound gradient
 *   buffer.  dsemb_out (optional): [n][4 mc]. */
int eegldm_debug_emb_mlp_launches(long* out_host, int reset);
int eegldm_debug_emb_mlp_plan(int n, int mc, int te, int E, int* out12_host);
int eegldm_debug_unet_embed(eegldm_unet* u, const int64_t* tsteps_dev, const int64_t* labels_dev, int n, float* table, float* work);
int eegldm_debug_unet_embed_backward(eegldm_unet* u, const int64_t* labels_dev, int n, const float* demb_all, const float* work,
                                     float* dsemb_out);
/* developer aid: the kernels that served the calling thread's last eegldm_batchnorm_lrelu_fwd (backward = 0) / _bwd (1), as eight ints:
 * statistics family (0 none: plain LeakyReLU, 1 eval, 2 scalar kernel + fp64 atomics, 3 4-wide partials + fold_finalize, 4 4-wide partials +
 * fold into a sum area (forward: the ordered fold of the deterministic mode; backward: always), 5 from a producing conv's partials), apply family
 * (0 scalar, 1 4-wide), blocks, rows per block, TX, TY of the statistics / reduce launch, deterministic mode (1 / 0), rows per block of the
 * apply launch.  No reference counterpart. */
int eegldm_debug_bn_last_route(int backward, int* out8_host);
/* developer aid: the thin-channel direct kernel (csrc/direct_conv.hip) that served the calling thread's last forward / data-gradient launch
 * (which = 0) or weight-gradient launch (which = 1), as eight ints: family (which = 0: 1 row, 2 in1_seg, 3 thin_in_reg, 4 thin_in with LDS
 * weights, 5 thin_out_run, 6 thin_out, 7 rowdot, 8 point; which = 1: 1 tinyv + fold, 2 tiny, 3 in1out, 4 wt, 5 generic; 0: none yet), the
 * template channel counts CI and CO (row, tinyv: both; thin_in_reg: CI; wt: CI = 1 for the wide-Cout instantiation, 0 for wide Cin; else 0),
 * data-gradient mode (1 / 0), grid blocks, rows per block and grid-stride pass (rounded up, so blocks * rows_per_block < rows proves that the
 * grid-stride loop wrapped), block partials written for a fold (0: the blocks add atomically), deterministic mode (1 / 0).  Convs that the
 * MFMA GEMM family serves leave the record untouched.  No reference counterpart. */
int eegldm_debug_dconv_last_route(int which, int* out8_host);
/* developer aid: what served the last eegldm_aekl_forward (ints 0-4) and the last eegldm_aekl_backward / _backward_ex (ints 5-9) on this handle,
 * five ints each: whole-network program ran (1: csrc/aekl_thin.hip, one workgroup per window; 0: the layer-by-layer path), micro-ops of its
 * forward and of its backward program, floats per LDS tensor (`maxt`) -- all three 0 on the layer-by-layer path --, and 1 when the
 * configuration was accepted for the whole-network route but its program did not fit the LDS, so that the layer-by-layer path was taken
 * instead.  All zero before the first call.  The route-aware tests confirm from it that a case ran on the kernels it names.
 * No reference counterpart. */
int eegldm_debug_aekl_last_route(const eegldm_aekl*, int* out10_host);
/* developer aid: what served the last eegldm_aekl_encode on this handle, as three ints: fused frozen-encoder path taken (1: csrc/enc_fused.hip;
 * 0: the layer-by-layer path, which is also what a shape or dtype that the fused kernels do not cover and EEGLDM_AEKL_NO_FUSED_ENC give),
 * pre_conv3 launches, sample_stats launches (both 0 on the layer-by-layer path).  All zero before the first call.  Host-side bookkeeping
 * only.  No reference counterpart. */
int eegldm_debug_aekl_encode_route(const eegldm_aekl*, int* out3_host);
/* developer aids: the two kernels of the fused frozen encoder (csrc/enc_fused.hip) alone, as eegldm_aekl_encode chains them.  bf16 / fp16.
 *   eegldm_debug_pre_conv3     y [B * L][Cout] = bias + conv3(silu(GroupNorm_{G = 1}(x [B * L][Cin]))) (+ resid [B * L][Cout], nullable); zero
 *                              padding of the ACTIVATED tensor at the sample edges.  in_stats: fp64 [B][2] = (sum, sum of squares) of each
 *                              sample of x; out_stats (nullable): fp64 [B][2], the same sums of the ROUNDED y are ADDED to it.  w packed
 *                              [3][Cout][Cin] in `dtype`; gamma, beta, bias fp32.  EEGLDM_ERR_UNSUPPORTED where the eligibility check says no
 *                              (channel counts other than 32 / 64, L not a multiple of 256, fp32).
 *   eegldm_debug_sample_stats  stats [B][2] (fp64) += (sum, sum of squares) of each sample of x [B][n_per_sample]; n_per_sample % 8 != 0
 *                              (samples that are not whole 16-byte chunks) is refused.
 * No reference counterpart. */
int eegldm_debug_pre_conv3(eegldm_ctx*, int dtype, const void* x, const double* in_stats, const float* gamma, const float* beta, const void* w,
                           const float* bias, const void* resid, void* y, double* out_stats, int B, int L, int Cin, int Cout, float eps);
int eegldm_debug_sample_stats(eegldm_ctx*, int dtype, const void* x, long n_per_sample, int B, double* stats);
/* developer aid: BatchNorm statistics (and the running-statistics update) from per-block column partials parts_dev [nb][2 C] fp32 (interleaved
 * sum, sum of squares) -- the fold that follows a conv whose epilogue left them.  No reference counterpart. */
int eegldm_debug_bn_stats_from_parts(eegldm_ctx*, const float* parts_dev, int nb, float* stats, float* running_mean, float* running_var,
                                     float* num_batches_tracked, long rows, int C);
/* developer aids: the fused PatchDiscriminator tail (BatchNorm + LeakyReLU + final 3-tap conv to one channel; logits / dlogits fp32 [B][L], w3
 * fp32 [3][C], gradients ACCUMULATED, dgamma = dbeta = dw3 = dbias = NULL: data gradient only) and the fused head backward (LeakyReLU + the
 * 1 -> C0 conv; x [B * L] and w [3][C0] in the engine dtype, dw / db ACCUMULATED, dx fp32 [B][L] WRITTEN), as eegldm_disc_forward / _backward
 * run them.  EEGLDM_ERR_UNSUPPORTED where the eligibility check of the executor says no (channel count, leading dimension, odd length).
 * No reference counterpart. */
int eegldm_debug_disc_tail_fwd(eegldm_ctx*, int dtype, const void* y, long ldy, const float* gamma, const float* beta, const float* stats,
                               const float* w3, const float* bias, float slope, float* logits, int B, int L, int C);
int eegldm_debug_disc_tail_bwd(eegldm_ctx*, int dtype, const void* y, long ldy, const float* gamma, const float* beta, const float* stats,
                               const float* w3, float slope, const float* dlogits, void* dy, long lddy, float* dgamma, float* dbeta,
                               float* dw3, float* dbias, int B, int L, int C);
int eegldm_debug_disc_head_bwd(eegldm_ctx*, int dtype, const void* da, long ldda, const void* x, const void* w, const float* bias, float slope,
                               float* dw, float* db, float* dx, int B, int L, int Lo, int C0, int stride);
/* developer aid: eegldm_conv1d_fwd that also asks for the per-block column statistics of the UNROUNDED outputs (col_parts_dev [nparts][2 Cout]
 * fp32, at most 16 MiB; *col_nparts_host = 0: the kernel that ran does not provide them).  No reference counterpart. */
int eegldm_debug_conv1d_fwd_colstats(eegldm_ctx*, const void* x, long ldx, const void* w, const float* bias, void* y, long ldy,
                                     int B, int Lin, int Cin, int Cout, int K, int stride, int pad_l, int pad_r,
                                     const float* rowvec, long ld_rowvec, const void* resid, long ld_resid, int dtype,
                                     float* col_parts_dev, int* col_nparts_host);
/* EEGLDM_DETERMINISTIC=1 (environment variable, read like the developer switches; eegldm.set_deterministic() in the Python mirror):
 * bit-reproducible losses, parameter gradients and optimiser steps run to run.  Every order-dependent reduction -- fp32 atomics of
 * the bias / GroupNorm / thin-conv gradients and of the loss sums, fused column sums inside the weight-gradient GEMM, split-K without
 * a workspace -- takes a written-partials + fixed-order-fold route; forward results are unchanged, except that eegldm_aekl_encode takes
 * its layer-by-layer path (the fused frozen encoder adds its per-sample statistics with fp64 atomics across tiles).  Reference counterpart:
 * torch.use_deterministic_algorithms(True) around src/train_ldm.py / src/train_autoencoderkl.py (the reference itself does not set it). */

/* ------------------------------------------------------------------ layout / packing */
int eegldm_ncl_to_nlc(eegldm_ctx*, const float* src_ncl, void* dst_nlc, long ld_dst, int B, int C, int L, int dst_dtype);
int eegldm_nlc_to_ncl(eegldm_ctx*, const void* src_nlc, long ld_src, float* dst_ncl, int B, int C, int L, int src_dtype);
/* (Cout,Cin,K) fp32  <->  [K][Cout][Cin] fp32 */
int eegldm_pack_conv_weight(eegldm_ctx*, const float* w_ref, float* w_packed, int Cout, int Cin, int K);
int eegldm_unpack_conv_weight(eegldm_ctx*, const float* w_packed, float* w_ref, int Cout, int Cin, int K);
/* fp32 -> compute dtype copy (n elements) */
int eegldm_cast(eegldm_ctx*, const float* src, void* dst, long n, int dst_dtype);

/* K-blocked copy of a 3-tap conv weight, [3][Cin/32][Cout][32] (16-bit dtypes, Cin % 32 == 0): writes it to w_kblocked
 * (same size as w) and registers it with the context, after which eegldm_conv1d_fwd(.., w, ..) reads its weight tiles from
 * the copy (one contiguous run per K stage; results are bit-identical).  The model executors do this for their own weights;
 * a caller of the primitives who updates w must pack again.  eegldm_conv1d_forget_kblocked removes the registration
 * (before freeing either buffer).  No reference counterpart: layout plumbing behind nn.Conv1d (unet.py:263). */
int eegldm_conv1d_pack_kblocked(eegldm_ctx*, const void* w, void* w_kblocked, int Cout, int Cin, int dtype);
/* the same for a weight of K taps (K = 1: [1][Cin/32][Cout][32], the copy eegldm_conv1d_skip_fwd reads its 1 x 1 weight from) */
int eegldm_conv1d_pack_kblocked_k(eegldm_ctx*, const void* w, void* w_kblocked, int Cout, int Cin, int K, int dtype);
int eegldm_conv1d_forget_kblocked(eegldm_ctx*, const void* w);
/* Stride-2 Conv1d(64 -> 128, k 3, padding 1) -- the PatchDiscriminator's second layer (config/config_aekl_eeg.yaml:30-40) -- as a stride-1
 * conv of the weight-stationary kernel over PAIRS of rows: fills w_fwd / w_dgrad ([3][128][128] elements each, caller-owned) from the packed
 * weight w ([3][128][64]) and registers them; eegldm_conv1d_fwd / _bwd_data then take that route for contiguous operands (ld = channels),
 * whole 64-row tiles per sample and >= 16 384 output rows.  eegldm_conv1d_forget_kblocked drops the registration. */
int eegldm_conv1d_pack_stride2(eegldm_ctx*, const void* w, void* w_fwd, void* w_dgrad, int Cout, int Cin, int dtype);
/* Data-gradient copy of a 3-tap conv weight, [3][Cout/32][Cin][32] (16-bit dtypes, Cout % 32 == 0): written to w_dgrad (same size as w)
 * and registered with the context, after which eegldm_conv1d_bwd_data(.., w, ..) may run the input gradient as a plain NT product on
 * the 192 x 256 tile (shapes with Cin % 256 == 0, Cout % 64 == 0, L % 192 == 0; other shapes are unaffected).  The model executors do
 * this for their own weights; eegldm_conv1d_forget_kblocked removes this registration too.  No reference counterpart: layout
 * plumbing behind the backward of nn.Conv1d (unet.py:263). */
int eegldm_conv1d_pack_dgrad(eegldm_ctx*, const void* w, void* w_dgrad, int Cout, int Cin, int dtype);
/* the same for a weight of K taps, [K][Cout][Cin] -> [K][Cout/32][Cin][32] (K = 1: 1 x 1 convs; K = 3 is eegldm_conv1d_pack_dgrad) */
int eegldm_conv1d_pack_dgrad_k(eegldm_ctx*, const void* w, void* w_dgrad, int Cout, int Cin, int K, int dtype);

/* ------------------------------------------------------------------ primitives (NLC)
 * nn.Conv1d as used at unet.py:263,291,302,385,504 and inside MONAI AutoencoderKL /
 * PatchDiscriminator.  w: packed [K][Cout][Cin] in `dtype`;
 * bias / rowvec / dw / dbias: fp32.  Output length Lout = (Lin + pad_l + pad_r - K)/stride + 1.
 * rowvec (optional): per-sample vector [B][ld_rowvec] added to every position (the
 * timestep-embedding add, unet.py:316-325).  resid (optional): tensor added in the
 * epilogue (residual / skip, unet.py:327). */
int eegldm_conv1d_fwd(eegldm_ctx*, const void* x, long ldx, const void* w, const float* bias,
                      void* y, long ldy, int B, int Lin, int Cin, int Cout, int K, int stride,
                      int pad_l, int pad_r, const float* rowvec, long ld_rowvec,
                      const void* resid, long ld_resid, int dtype);
/* The ResBlock tail `self.skip_connection(x) + h` with h = out_layers' conv (unet.py:302,327) as one operator:
 *   y = conv1d(x; w [3][Cout][Cin], pad 1) + bias + conv1d(x2; w2 [1][Cout][Cin2]) + bias2 (+ rowvec per sample)
 * With 16-bit operands, Cout % 256 == 0, B*L and L multiples of 192 and K-blocked copies of BOTH weights registered
 * (eegldm_conv1d_pack_kblocked / _k) it is ONE launch -- the 1 x 1 conv runs as further reduction stages of the 3-tap kernel: one
 * fp32 accumulator, one rounding, no intermediate tensor; otherwise the two convs are launched one after the other (y is then
 * rounded twice in 16-bit storage).  y must not alias x or x2. */
int eegldm_conv1d_skip_fwd(eegldm_ctx*, const void* x, long ldx, const void* w, const float* bias,
                           const void* x2, long ldx2, const void* w2, const float* bias2, void* y, long ldy,
                           int B, int L, int Cin, int Cin2, int Cout, const float* rowvec, long ld_rowvec, int dtype);
int eegldm_conv1d_bwd_data(eegldm_ctx*, const void* dy, long lddy, const void* w, void* dx, long lddx,
                           int B, int Lin, int Cin, int Cout, int K, int stride, int pad_l, int pad_r,
                           const void* resid, long ld_resid, int dtype);
/* dw += ..., dbias += ... (fp32 accumulators; dbias may be NULL) */
int eegldm_conv1d_bwd_weight(eegldm_ctx*, const void* x, long ldx, const void* dy, long lddy,
                             float* dw, float* dbias, int B, int Lin, int Cin, int Cout, int K,
                             int stride, int pad_l, int pad_r, int dtype);
/* nn.Linear (unet.py:373-377, 277-285): y[M][N] = x[M][K] w[N][K]^T + bias; y is fp32 when out_f32.  M is free; N must be a
 * multiple of 4 (vector epilogue) and K a whole number of 16-byte chunks (8 bf16 / 4 fp32 elements): anything else is refused. */
int eegldm_linear_fwd(eegldm_ctx*, const void* x, long ldx, const void* w, const float* bias, void* y, long ldy,
                      int M, int N, int K, int dtype, int out_f32);
/* its backward (what autograd derives for nn.Linear): dx[M][K] = dy[M][N] w[N][K] (skipped when dx is NULL; fp32 when dx_f32),
 * dw[N][K] += dy^T x and dbias[N] += column sums of dy (fp32 accumulators; either may be NULL) */
int eegldm_linear_bwd(eegldm_ctx*, const void* x, long ldx, const void* w, const void* dy, long lddy, void* dx, long lddx,
                      float* dw, float* dbias, int M, int N, int K, int dtype, int dx_f32);

/* nn.GroupNorm(G, C, eps) [+ SiLU] (unet.py:71-74; MONAI norm_num_groups, eps 1e-6).
 * stats: [B][G][2] fp32 (mean, rstd), written by fwd and consumed by bwd.
 * resample: 0 none, 1 = AvgPool1d(2,2) after the activation, 2 = nearest x2 after the
 * activation (the up/down ResBlock, unet.py:308-313); then y has L/2 or 2L rows and
 * xr (optional) receives the equally resampled raw x. */
int eegldm_groupnorm_fwd(eegldm_ctx*, const void* x, long ldx, const float* gamma, const float* beta,
                         void* y, long ldy, float* stats, int B, int L, int C, int G, float eps,
                         int fuse_silu, int resample, void* xr, long ldxr, int dtype);
int eegldm_groupnorm_bwd(eegldm_ctx*, const void* x, long ldx, const float* gamma, const float* beta,
                         const float* stats, const void* dy, long lddy, void* dx, long lddx,
                         float* dgamma, float* dbeta, int B, int L, int C, int G, int fuse_silu,
                         int resample, const void* dxr, long lddxr, int dtype);

/* single-head QKV attention (unet.py:107-125): qkv [B*T][3C] (q|k|v), out [B*T][C].
 * probs: caller-provided [B][T][T] `dtype` buffer (kept for backward);
 * scratch_*: caller-provided work buffers, [B][T][T] fp32 (logits / dprobs) and
 * [B][T][T] `dtype` (dlogits). */
int eegldm_attention_fwd(eegldm_ctx*, const void* qkv, long ldqkv, void* out, long ldo, void* probs,
                         float* scratch_logits, int B, int T, int C, int dtype);
int eegldm_attention_bwd(eegldm_ctx*, const void* qkv, long ldqkv, const void* probs, const void* dout, long lddo,
                         void* dqkv, long lddqkv, float* scratch_dprobs, void* scratch_dlogits,
                         int B, int T, int C, int dtype);

/* ------------------------------------------------------------------ schedulers / losses / optimizer
 * DDPMScheduler.add_noise / get_velocity (training.py:429-436), DDIMScheduler.step
 * (sample_trials.py:163), F.mse_loss (training.py:437), torch.optim.Adam (train_ldm.py:208). */
int eegldm_add_noise(eegldm_ctx*, const float* x, const float* noise, const int64_t* t, const float* acp,
                     float* out, int B, long n_per_sample);
int eegldm_get_velocity(eegldm_ctx*, const float* x, const float* noise, const int64_t* t, const float* acp,
                        float* out, int B, long n_per_sample);
int eegldm_ddim_step(eegldm_ctx*, const float* model_out, const float* sample, float a_t, float a_prev,
                     int pred_type, int clip_sample, float* prev_sample, float* pred_x0, long n);
/* DDIMScheduler.step with eta >= 0 (the reference samples with eta = 0, sample_trials.py:163; eta > 0 is the scheduler's stochastic form):
 * sigma = eta sqrt((1 - a_prev) / (1 - a_t) (1 - a_t / a_prev)), prev = sqrt(a_prev) x0 + sqrt(1 - a_prev - sigma^2) eps + sigma noise.
 * eta == 0 is eegldm_ddim_step (noise may be NULL); eta == 1 over consecutive timesteps is the ancestral DDPM step (tests). (ABI 8) */
int eegldm_ddim_step_eta(eegldm_ctx*, const float* model_out, const float* sample, const float* noise, float a_t, float a_prev, float eta,
                         int pred_type, int clip_sample, float* prev_sample, float* pred_x0, long n);
/* DDPMScheduler.step (variance_type "fixed_small"; the ancestral sampler of util.py:241-243,261-285 and sample_trials_ddpm.py:99-102;
 * arithmetic pinned against DDPM.p_sample, /root/reference/src/models/ldm.py:311-357): x0 from the prediction type, optional clamp
 * to [-1,1], prev = c0*x0 + ct*sample + sqrt(max(var,1e-20))*noise with the posterior coefficients of (a_t, a_prev, beta_t);
 * a_prev == 1 (t == 0) adds no noise and `noise` may be NULL there.  pred_x0 nullable. */
int eegldm_ddpm_step(eegldm_ctx*, const float* model_out, const float* sample, const float* noise, float a_t, float a_prev,
                     float beta_t, int pred_type, int clip_sample, float* prev_sample, float* pred_x0, long n);
/* the same step with variance_type "fixed_large" when variance_large != 0: sigma^2 = beta_t instead of the posterior variance (ABI 8) */
int eegldm_ddpm_step_var(eegldm_ctx*, const float* model_out, const float* sample, const float* noise, float a_t, float a_prev,
                         float beta_t, int variance_large, int pred_type, int clip_sample, float* prev_sample, float* pred_x0, long n);
/* loss = mean((pred-target)^2); dpred = 2 (pred-target) / n * grad_scale (nullable) */
int eegldm_mse_loss(eegldm_ctx*, const float* pred, const float* target, float* loss, float* dpred, long n, float grad_scale);
/* Weighted diffusion loss with per-sample losses (the reference trains on the plain F.mse_loss; Min-SNR-gamma, Hang et al. 2023, is a
 * table here).  pred / x0 / noise / dpred: (B, n_per_sample) fp32; N = n_per_sample.  The target is noise (epsilon), x0 (sample), or
 * sqrt(acp[t_b]) noise - sqrt(1 - acp[t_b]) x0 (v_prediction) formed in registers with the rounding of eegldm_get_velocity; the buffer a
 * prediction type does not read may be NULL (x0 for epsilon, noise for sample; acp is read for v_prediction only).
 *   m_b = (1 / N) sum_i (pred - target)^2,   w_b = wtab[t_b] (wtab NULL: 1),   loss = (1 / B) sum_b w_b m_b,
 *   per_sample[b] (NULL ok) = m_b, unweighted,   dpred (NULL ok) = 2 (pred - target) / (B N) * grad_scale * w_b
 * (with w_b = 1 the bytes of eegldm_mse_loss's dpred).  wtab is a device table indexed by timestep (schedulers.loss_weights); all knowledge
 * of the weighting lives there.  Reductions: a written partial per (sample, 1024-element chunk), folded per sample in chunk order, the B
 * weighted values then added in sample order -- no float atomics, bit-reproducible with or without EEGLDM_DETERMINISTIC.  16-byte accesses
 * when the buffers in use share one offset inside a 16-byte line (scalar head / tail per sample), any 4-byte alignment otherwise.
 * Timesteps must lie inside the tables. */
int eegldm_diffusion_loss(eegldm_ctx*, const float* pred, const float* x0, const float* noise, const int64_t* t, const float* acp,
                          const float* wtab, int pred_type, int B, long n_per_sample, float grad_scale, float* loss, float* per_sample,
                          float* dpred);
/* Loss by noise level: bin_sum[k] += per_sample[b] and bin_cnt[k] += 1 for k = t_b K / T (integer division), samples in ascending order
 * (one workgroup: order-fixed).  bin_sum: K floats, bin_cnt: K int64, both accumulated into; timesteps outside [0, T) are not counted. */
int eegldm_loss_bins(eegldm_ctx*, const float* per_sample, const int64_t* t, int B, int T, int K, float* bin_sum, int64_t* bin_cnt);
int eegldm_adam_step(eegldm_ctx*, float* p, const float* g, float* m, float* v, long n, float lr, float beta1,
                     float beta2, float eps, int step, float grad_inv_scale);
/* Weight EMA (exponential moving average of the parameters; the reference has none, diffusion code bases sample from one).
 * The shadow is one more flat fp32 buffer beside the parameters.  All three are single streaming passes with 16-byte accesses on the part of
 * the buffers that is 16-byte aligned (any n, any 4-byte-aligned address).  NULL buffers, n < 0 and overlapping buffers are rejected
 * before the device is touched.
 *   eegldm_adam_step_ema  eegldm_adam_step, then in the same pass ema = fma(one_minus_decay, p_new - ema, ema): p, m, v come out
 *                         bit-identical to eegldm_adam_step and ema bit-identical to eegldm_adam_step + eegldm_ema_update
 *   eegldm_ema_update     ema = fma(one_minus_decay, p - ema, ema) on its own (parameters updated by another optimizer)
 *   eegldm_swap           exchanges a[0..n) and b[0..n) in place
 * one_minus_decay = 1 - decay, rounded once from double by the caller.  A NaN / inf parameter gives a NaN / inf shadow value. */
int eegldm_adam_step_ema(eegldm_ctx*, float* p, const float* g, float* m, float* v, float* ema, long n, float lr, float beta1,
                         float beta2, float eps, int step, float grad_inv_scale, float one_minus_decay);
int eegldm_ema_update(eegldm_ctx*, float* ema, const float* p, long n, float one_minus_decay);
int eegldm_swap(eegldm_ctx*, float* a, float* b, long n);
/* Global gradient-norm clipping (torch.nn.utils.clip_grad_norm_, L2 norm over the whole flat gradient) without a host read.
 * state: 8 device floats owned by the caller, zeroed once; eegldm_grad_norm leaves
 *   state[0]  sqrt(sum_i (g[i] * pre_scale)^2): the norm of the un-scaled gradient (pre_scale = 1 / loss scale)
 *   state[1]  coef = min(1, max_norm / (state[0] + 1e-6f)) in fp32, exactly that expression (torch's clip_coef_clamped; max_norm = +inf gives
 *             1 for a finite norm; a NaN norm gives NaN, an infinite one 0 or, with max_norm = +inf, NaN -- as in torch; nothing is skipped)
 *   state[2]  1 if any g[i] is inf / NaN, else 0 (the answer of eegldm_grad_check_finite)
 *   state[3]  += 1 when coef < 1 (steps clipped)     state[4]  += 1 (calls)     state[5]  = max(state[5], state[0])     state[6..7]  untouched
 * Reduction: one fp32 partial per chunk of 16384 elements (a constant: no dependence on the device or the grid), inside a chunk a fixed
 * per-thread order of fused multiply-adds (16-byte loads on the aligned body, scalar head and tail; any n >= 0, any 4-byte alignment), a
 * wave butterfly and a pairwise sum of the waves; a one-block kernel then folds the partials in index order in double.  No float atomics, no
 * memset: the same bits on every run, with or without EEGLDM_DETERMINISTIC.  The partials live in the context's written-partials buffer
 * (as eegldm_diffusion_loss's): the first call on a context that has not used that buffer allocates it (32 MiB, once), and a call that
 * needs more than it holds (n above 6.8e10) synchronises the stream to regrow it; every other call is launches only.  A finite |g[i] * pre_scale| above 1.8e19 overflows the fp32 sum of squares (as torch's fp32 norm does).
 * NULL buffers, n < 0, max_norm <= 0 and a NaN max_norm are rejected before the device is touched (state stays as it was).
 *   eegldm_adam_step_clip  eegldm_adam_step (ema NULL) / eegldm_adam_step_ema with grad_inv_scale * state[1] -- ONE fp32 product, read from
 *                          the device -- in place of grad_inv_scale: with state[1] == 1 the bytes of those exports, with state[1] = c the bytes
 *                          they give for the host float grad_inv_scale * c.  g is not modified.  Refusals as eegldm_adam_step_ema.
 *   eegldm_grad_scale_by   g[i] *= state[1] in place: the second half of a stand-alone clip_grad_norm_ (parameters stepped by another optimizer) */
int eegldm_grad_norm(eegldm_ctx*, const float* g, long n, float pre_scale, float max_norm, float* state);
int eegldm_adam_step_clip(eegldm_ctx*, float* p, const float* g, float* m, float* v, float* ema /* nullable */, long n, float lr, float beta1,
                          float beta2, float eps, int step, float grad_inv_scale, float one_minus_decay, const float* state);
int eegldm_grad_scale_by(eegldm_ctx*, float* g, long n, const float* state);
/* found_inf[0] (device float) = 1 if any of g[0..n) is inf/nan, else 0 -- the check behind GradScaler.unscale_/step
 * (torch.cuda.amp.GradScaler at /root/reference/src/training/training.py:334,441-443). g must be 16-byte aligned. */
int eegldm_grad_check_finite(eegldm_ctx*, const float* g, long n, float* found_inf);
int eegldm_randn(eegldm_ctx*, float* out, long n, uint64_t seed, uint64_t offset);
int eegldm_randint(eegldm_ctx*, int64_t* out, long n, int64_t high, uint64_t seed, uint64_t offset);

/* ------------------------------------------------------------------ UNet denoiser
 * UNetModel(image_size, in_channels, model_channels, out_channels, num_res_blocks,
 * attention_resolutions, dropout=0, channel_mult, num_heads=1, use_scale_shift_norm=False,
 * resblock_updown=True) -- /root/reference/src/models/unet.py:330-563, config_ldm.yaml:30-43. */
typedef struct {
  int in_channels, out_channels, model_channels, num_res_blocks;
  int n_mult; int channel_mult[8];
  int n_attn; int attention_resolutions[8];
  int num_heads;           /* attention heads of the input / middle blocks (unet.py:344,146-153; 0 = 1).  QKVAttentionLegacy layout:
                            * the qkv projection's channels are [q_0 | k_0 | v_0 | q_1 | ...] (unet.py:107-125) */
  int dtype;               /* storage/compute dtype of activations: EEGLDM_F32, EEGLDM_BF16 or EEGLDM_F16 */
  /* ABI 8: the constructor branches every reference yaml leaves at the values of config_ldm.yaml; 0 = that default */
  int num_head_channels;   /* > 0: heads = channels / num_head_channels in every attention block (unet.py:149-153); <= 0: num_heads */
  int num_heads_upsample;  /* heads of the output blocks' attention (unet.py:354-355,481-487); <= 0: num_heads */
  int use_scale_shift_norm;/* != 0: h = GroupNorm(h) * (1 + scale) + shift, emb_layers 2 x out_channels wide (unet.py:279-284,318-322) */
  int resample_layers;     /* != 0: resblock_updown = False -- Downsample / Upsample layers instead of down / up ResBlocks (unet.py:462-470,493-498) */
  int resample_pool_only;  /* with resample_layers: != 0 = conv_resample False (AvgPool1d(2,2) / nearest x 2 only, unet.py:192-195,221);
                            * 0 = Conv1d(k 3, stride 2, padding 1) / nearest x 2 + Conv1d(k 3, padding 1) (unet.py:188-190,211-224) */
} eegldm_unet_cfg;

int eegldm_unet_create(eegldm_ctx*, const eegldm_unet_cfg* cfg, eegldm_unet** out);
int eegldm_unet_destroy(eegldm_unet*);
/* nn.Dropout(p) of ResBlock.out_layers (unet.py:289; every reference yaml sets 0.0): active in forwards with training != 0 only; masks come
 * from the on-device Philox stream (seed, running counter), are regenerated by the backward and never stored.  Calling it restarts the
 * counter: the same seed reproduces the same masks for the same sequence of forwards.  (ABI 8) */
int eegldm_unet_set_dropout(eegldm_unet*, float p, uint64_t seed);
/* The mask kernel itself, in place on a [rows][C] tensor (leading dimension ld, elements): x <- keep ? x / (1 - p) : 0 with keep drawn from
 * Philox(seed, offset + e / 4), e = row * C + column.  The same (seed, offset) gives the same mask: the backward applies it to the gradient. */
int eegldm_dropout(eegldm_ctx*, void* x, long ld, long rows, int C, float p, uint64_t seed, uint64_t offset, int dtype);
/* Parameter table: entry i <-> one reference state_dict key, stored at [offset, offset+numel)
 * of the flat fp32 parameter / gradient buffers.  Conv weights (ndim 3) are stored packed
 * [K][Cout][Cin]; `shape` reports the reference shape (Cout, Cin, K). */
int eegldm_unet_num_entries(const eegldm_unet*);
long eegldm_unet_num_params(const eegldm_unet*);
int eegldm_unet_entry(const eegldm_unet*, int i, char* name, int name_cap, long* offset, long* numel,
                      int* ndim, int shape[3]);
/* Bind caller-owned flat fp32 buffers (grads may be NULL for inference). */
int eegldm_unet_bind(eegldm_unet*, float* params, float* grads);
/* Optional host callback fired from eegldm_unet_backward / eegldm_ldm_train_step once the gradients in
 * [offset, offset + numel) of the flat gradient buffer (out, output_blocks, middle_block -- the tail of the layout) are
 * complete in stream order, while the input blocks' backward is still to be enqueued.  Data-parallel hosts start the
 * all-reduce of that slice there (replaces torch.nn.DataParallel's gather, train_ldm.py:190-192).  NULL disables. */
typedef void (*eegldm_grad_hook)(void* user, long offset, long numel);
int eegldm_unet_set_grad_hook(eegldm_unet*, eegldm_grad_hook fn, void* user);
/* Refresh the compute-dtype weight copies after `params` changed (no-op for fp32). */
int eegldm_unet_sync_weights(eegldm_unet*);
/* forward(x, timesteps): x, y are NCL fp32 (B, C, L); t int64 (B).  training != 0 keeps
 * activations for eegldm_unet_backward.  training == 0 (model.eval(): sampling) MAY skip them: for launches of a few hundred rows
 * (one window per call, sample_trials.py:149-163) the second GroupNorm of each ResBlock is applied inside the next conv and neither
 * its output nor its statistics are stored -- eegldm_unet_backward then fails with an error instead of using a partial tape.  The
 * reference has the same contract in another form: its sampling runs under torch.no_grad() (sample_trials.py:147). */
int eegldm_unet_forward(eegldm_unet*, const float* x, const int64_t* t, float* y, int B, int L, int training);
/* grads += d loss / d params; dx (nullable) = d loss / d x.  Gradients accumulate: zero the
 * flat gradient buffer (eegldm_fill) between steps, as optimizer.zero_grad does. */
int eegldm_unet_backward(eegldm_unet*, const float* dy, float* dx);
int eegldm_fill(eegldm_ctx*, float* p, long n, float value);

/* The body of train_epoch_ldm (training.py:419-443) after the frozen encoder: add_noise,
 * UNet forward, MSE vs noise / velocity, backward.  loss: device scalar. */
int eegldm_ldm_train_step(eegldm_unet*, const float* latents, const float* noise, const int64_t* t,
                          const float* acp, int pred_type, int B, int L, float grad_scale, float* loss);

/* ------------------------------------------------------------------ class-conditional UNet (additive; ABI 8)
 * UNetModel(num_classes=K) (unet.py:342,366,379-380,531-533): one more parameter, label_emb.weight [K][4 * model_channels] (fp32, entry
 * right after time_embed.2.bias -- the reference's parameter order -- and outside the tail slice the grad hook reports), and
 * emb = time_embed(t_emb) + label_emb[y] ahead of the SiLU and the ResBlocks' projections.  Labels are device int64 [B] and must lie in
 * [0, K); a label outside the range adds nothing (no read outside the table) -- the host checks them before the call.  The forward copies
 * them into the executor, so eegldm_unet_backward after eegldm_unet_forward_cond does not read the caller's buffer; the backward adds
 * d label_emb[c] = sum over samples with y_b == c of d emb[b], folded in sample order (no atomics; classes absent from the batch get
 * exactly nothing).  The unconditional entry points (eegldm_unet_forward, eegldm_ldm_train_step, eegldm_sample) return an error on a
 * conditional UNet and vice versa. */
int eegldm_unet_create_cond(eegldm_ctx*, const eegldm_unet_cfg* cfg, int num_classes, eegldm_unet** out);
int eegldm_unet_forward_cond(eegldm_unet*, const float* x, const int64_t* t, const int64_t* labels, float* y, int B, int L, int training);
/* eegldm_ldm_train_step with labels and classifier-free guidance training: each sample's label is replaced by null_class (in [0, K)) with
 * probability p_uncond, drawn from Philox(seed, offset + b) (eegldm_label_dropout); the backward uses the replaced labels.  p_uncond == 0 is
 * the plain conditional step. */
int eegldm_ldm_train_step_cond(eegldm_unet*, const float* latents, const float* noise, const int64_t* t, const float* acp, int pred_type,
                               int B, int L, float grad_scale, float* loss, const int64_t* labels, float p_uncond, int64_t null_class,
                               uint64_t seed, uint64_t offset);
/* eegldm_ldm_train_step / eegldm_ldm_train_step_cond with eegldm_diffusion_loss in place of get_velocity + mse_loss (two kernels instead of memset + mse_loss [+ get_velocity]), no
 * target buffer, no float atomics in the loss.  wtab (NULL: all ones) weights sample b by wtab[t_b]; per_sample (NULL ok) receives the
 * unweighted per-sample losses.  labels == NULL for an unconditional UNet (the four label arguments are then ignored); the checks of the
 * two steps above apply. */
int eegldm_ldm_train_step_weighted(eegldm_unet*, const float* latents, const float* noise, const int64_t* t, const float* acp, int pred_type,
                                   int B, int L, float grad_scale, float* loss, const float* wtab, float* per_sample,
                                   const int64_t* labels, float p_uncond, int64_t null_class, uint64_t seed, uint64_t offset);
/* The label dropout on its own: out[b] = labels[b], or null_class when word 0 of Philox(seed, offset + b) / 2^32 < p_uncond. */
int eegldm_label_dropout(eegldm_ctx*, const int64_t* labels, int64_t* out, int B, float p_uncond, int64_t null_class, uint64_t seed,
                         uint64_t offset);

/* Round-6 prototype: nn.Conv1d(k 3, padding 1) over SiLU(GroupNorm(x)) -- the in_layers / out_layers pair of
 * /root/reference/src/models/unet.py:261-263,287-291 -- with the normalisation applied to the conv's operand tile inside LDS, so the
 * normalised tensor is never written (no-grad forward only: nothing is kept for a backward).  gn_stats: fp32 [B][G][2] = (mean, rstd) of x, as
 * eegldm_groupnorm_fwd leaves them.  bf16, silu = 1, B * L and L multiples of 192, Cout a multiple of 256, Cin of 64 (<= 1024), weight
 * registered with eegldm_conv1d_pack_kblocked; anything else is an error (there is no fallback inside this entry). */
int eegldm_conv1d_fwd_gn(eegldm_ctx*, const void* x, long ldx, const void* w, const float* bias, const float* gn_gamma, const float* gn_beta,
                         const float* gn_stats, int G, int silu, void* y, long ldy, int B, int L, int Cin, int Cout,
                         const float* rowvec, long ld_rowvec, const void* resid, long ld_resid, int dtype);

/* ------------------------------------------------------------------ UNet building blocks at primitive granularity (ABI 7)
 * ONE ResBlock(channels, emb_channels, dropout=0, out_channels, up / down) -- /root/reference/src/models/unet.py:227-327 -- or ONE
 * AttentionBlock(channels, num_heads=1) -- unet.py:132-174 -- run through exactly the kernel sequences the UNet executor runs per block
 * (csrc/net.hip res_forward / res_backward / attn_forward / attn_backward), plus timestep_embedding(t, dim) -- unet.py:12-36.
 * They exist so that the reference's per-primitive goldens are checked against the kernels, not only whole models
 * (tests/test_gpu_primitive_goldens.py).  Entry names are the reference module's state_dict keys; parameters / gradients are flat fp32
 * buffers as for the models; conv weights packed [K][Cout][Cin].  updown: 0 none, 1 down (AvgPool1d(2)), 2 up (nearest x2).
 * forward: x (B, channels, L) and y (B, out_channels, L') fp32 NCL; emb (B, emb_channels) fp32 -- the ResBlock's `emb` argument
 * (emb_layers = SiLU -> Linear runs inside); NULL for an AttentionBlock.  backward: grads += d<dy, y>/dparams; dx and demb are
 * WRITTEN (both nullable). */
/* use_scale_shift_norm != 0: ResBlock(use_scale_shift_norm=True) -- emb_layers.1 is 2 x out_channels wide (unet.py:279-284,318-322).
 * num_heads: AttentionBlock(channels, num_heads) (unet.py:132-166; pass channels / num_head_channels for the other spelling). */
int eegldm_resblock_create(eegldm_ctx*, int channels, int out_channels, int emb_channels, int groups, int updown, int use_scale_shift_norm,
                           int dtype, eegldm_block** out);
int eegldm_attnblock_create(eegldm_ctx*, int channels, int num_heads, int dtype, eegldm_block** out);
int eegldm_block_destroy(eegldm_block*);
int eegldm_block_num_entries(const eegldm_block*);
long eegldm_block_num_params(const eegldm_block*);
int eegldm_block_entry(const eegldm_block*, int i, char* name, int name_cap, long* offset, long* numel, int* ndim, int shape[3]);
int eegldm_block_bind(eegldm_block*, float* params, float* grads);
int eegldm_block_forward(eegldm_block*, const float* x, const float* emb, float* y, int B, int L);
int eegldm_block_backward(eegldm_block*, const float* dy, float* dx, float* demb);
/* out (B, dim) fp32 = [cos(t f_0) .. cos(t f_{h-1}), sin(t f_0) .. sin(t f_{h-1})], f_i = exp(-ln(10000) i / h), h = dim / 2; t int64 on the device */
int eegldm_timestep_embedding(eegldm_ctx*, const int64_t* t, float* out, int B, int dim);

/* ------------------------------------------------------------------ AutoencoderKL / PatchDiscriminator primitives
 * MONAI PatchDiscriminator layer `Convolution(.., norm=BATCH, act=LEAKYRELU(0.2))` (config/config_aekl_eeg.yaml:30-40; twin
 * src/models/discriminator.py:47-66): y = LeakyReLU_slope(BatchNorm1d(x)) on NLC rows [rows][C].  training != 0: batch statistics
 * (biased variance, eps 1e-5) and, when running_mean is given, the running-statistics update (momentum 0.1, unbiased variance,
 * num_batches_tracked += 1 -- a float count); training == 0: running statistics.  stats [C][2] fp32 receives (mean, rstd) -- the
 * tape of the backward.  gamma == NULL: plain LeakyReLU (no statistics).
 * Backward: dx, and dgamma / dbeta ACCUMULATED (fp32 [C]); the statistics of the forward. */
int eegldm_batchnorm_lrelu_fwd(eegldm_ctx*, const void* x, long ldx, const float* gamma, const float* beta, float* stats,
                               float* running_mean, float* running_var, float* num_batches_tracked, void* y, long ldy,
                               long rows, int C, float slope, int training, int dtype);
int eegldm_batchnorm_lrelu_bwd(eegldm_ctx*, const void* x, long ldx, const float* gamma, const float* beta, const float* stats,
                               const void* dy, long lddy, void* dx, long lddx, float* dgamma, float* dbeta, long rows, int C,
                               float slope, int dtype);
/* AutoencoderKL.sampling + the KL term of train_autoencoderkl.py:210-211 in one pass over n = B * latent * L' elements:
 * sigma = exp(clamp(log_var, -30, 20) / 2) (fp32 out), z = mu + eps * sigma (eps NULL: z = mu), and
 * *kl += (1 / B) * sum 0.5 * (mu^2 + sigma^2 - log sigma^2 - 1) when kl != NULL (zero it first).
 * Backward of  <dz, z> + kl_weight * KL : dmu = dz + (kl_weight / B) mu;
 * dlog_var = [-30 < log_var < 20] * (dz eps + (kl_weight / B)(sigma - 1 / sigma)) * sigma / 2.  dz NULL: the KL part alone. */
int eegldm_kl_reparam_fwd(eegldm_ctx*, const void* mu, const void* log_var, const float* eps, void* z, float* sigma, float* kl,
                          long n, int B, int dtype);
int eegldm_kl_reparam_bwd(eegldm_ctx*, const void* mu, const void* log_var, const float* eps, const float* sigma, const void* dz,
                          void* dmu, void* dlog_var, long n, float kl_weight_over_B, int dtype);

/* Stand-alone resampling in the NLC layout (rows = B * L, leading dimensions in elements): Downsample / Upsample with use_conv = False
 * (src/models/unet.py:177-224: nn.AvgPool1d(2, 2) / F.interpolate(scale_factor = 2, mode = "nearest")), the ops a ResBlock applies to h
 * and x when up / down is set (unet.py:308-313).  The executors fuse them into the GroupNorm kernels (`resample` above); these four are
 * the same arithmetic at primitive granularity.  L is the length of the op's INPUT (x for _fwd, the op's input for _bwd as well:
 * avgpool2_bwd takes dy [B][L/2][C] -> dx [B][L][C]; nearest2_bwd takes dy [B][2L][C] -> dx [B][L][C]). */
int eegldm_avgpool2_fwd(eegldm_ctx*, const void* x, long ldx, void* y, long ldy, int B, int L, int C, int dtype);
int eegldm_avgpool2_bwd(eegldm_ctx*, const void* dy, long lddy, void* dx, long lddx, int B, int L, int C, int dtype);
int eegldm_nearest2_fwd(eegldm_ctx*, const void* x, long ldx, void* y, long ldy, int B, int L, int C, int dtype);
int eegldm_nearest2_bwd(eegldm_ctx*, const void* dy, long lddy, void* dx, long lddx, int B, int L, int C, int dtype);

/* ------------------------------------------------------------------ losses of the AEKL step (fp32 NCL tensors)
 * L1Loss (train_autoencoderkl.py:155,206): *loss = mean|a-b|; da_accum (nullable) += grad_weight * d/da.
 * PatchAdversarialLoss("least_squares") (:156,214,226,228): LeakyReLU(0.05) on the logits, MSE against 1 / 0;
 *   dlogits (nullable) = grad_weight * d/dlogits.
 * JukeboxLoss(spatial_dims=1, reduction="sum") (:158,208): sum over windows and bins of (|FFT_ortho(recon)| -
 *   |FFT_ortho(target)|)^2; d_recon_accum (nullable) += grad_weight * d/d recon.  C must be 1; L in {3072, 768, 256, 96}. */
int eegldm_l1_loss(eegldm_ctx*, const float* a, const float* b, float* loss, float* da_accum, long n, float grad_weight);
int eegldm_lsgan_loss(eegldm_ctx*, const float* logits, int target_is_real, float* loss, float* dlogits, long n, float grad_weight);
int eegldm_spectral_loss(eegldm_ctx*, const float* recon, const float* target, float* loss, float* d_recon_accum,
                         int B, int C, int L, float grad_weight);
int eegldm_axpy(eegldm_ctx*, float* y, const float* x, float a, long n);

/* ------------------------------------------------------------------ AutoencoderKL
 * AutoencoderKL(spatial_dims=1, in_channels, out_channels, num_channels, latent_channels, num_res_blocks,
 * norm_num_groups, attention_levels=all False, with_*_nonlocal_attn=False) -- monai-generative, as configured by
 * config/config_aekl_eeg.yaml:19-28 and train_autoencoderkl.py:129-133.  Parameter table / bind / sync as for the UNet;
 * keys follow monai-generative's state_dict naming (encoder.blocks.N..., quant_conv_mu.conv..., ...). */
typedef struct {
  int in_channels, out_channels;
  int n_levels; int num_channels[8];
  int latent_channels, num_res_blocks, norm_num_groups;
  int dtype;
} eegldm_aekl_cfg;
int eegldm_aekl_create(eegldm_ctx*, const eegldm_aekl_cfg* cfg, eegldm_aekl** out);
int eegldm_aekl_destroy(eegldm_aekl*);
int eegldm_aekl_num_entries(const eegldm_aekl*);
long eegldm_aekl_num_params(const eegldm_aekl*);
int eegldm_aekl_entry(const eegldm_aekl*, int i, char* name, int name_cap, long* offset, long* numel, int* ndim, int shape[3]);
int eegldm_aekl_bind(eegldm_aekl*, float* params, float* grads);
int eegldm_aekl_sync_weights(eegldm_aekl*);
/* encode + sampling (encode_stage_2_inputs, train_ldm.py:148; Stage1Wrapper, training.py:15-26):
 * x (B,in,L) -> z = mu + eps*sigma (B,lat,L/2^(levels-1)); eps NULL -> z = mu.  z / z_mu / z_sigma nullable. */
int eegldm_aekl_encode(eegldm_aekl*, const float* x, const float* eps, float* z, float* z_mu, float* z_sigma, int B, int L);
/* decode_stage_2_outputs (sample_trials.py:166): z (B,lat,Ll) -> (B,out,Ll*2^(levels-1)) */
int eegldm_aekl_decode(eegldm_aekl*, const float* z, float* recon, int B, int Ll);
/* forward(x) -> (reconstruction, z_mu, z_sigma) with the reparameterisation noise eps supplied by the caller;
 * kl (nullable device scalar) receives 0.5*sum(mu^2+sigma^2-log sigma^2-1)/B.  Keeps the tape for backward. */
int eegldm_aekl_forward(eegldm_aekl*, const float* x, const float* eps, float* recon, float* z_mu, float* z_sigma,
                        float* kl, int B, int L);
/* grads += d/dparams [ <d_recon, recon> + kl_weight * KL ]; dx nullable */
int eegldm_aekl_backward(eegldm_aekl*, const float* d_recon, float kl_weight, float* dx);
/* The same plus <d_mu, z_mu> + <d_sigma, z_sigma>: gradients a caller's own loss put on the z_mu / z_sigma tensors eegldm_aekl_forward
 * returned (fp32 (B, lat, L/2^(levels-1)), each nullable) -- what an autograd engine hands back when the KL term is written with tensor
 * ops on those outputs, as train_autoencoderkl.py:210-211 does (eegldm.autograd). */
int eegldm_aekl_backward_ex(eegldm_aekl*, const float* d_recon, const float* d_mu, const float* d_sigma, float kl_weight, float* dx);

/* ------------------------------------------------------------------ quality metrics (fp32 NCL tensors, results on the device)
 * 1-D multi-scale SSIM -- the reference's local adaptation of MONAI's MultiScaleSSIMMetric (compute_mmds.py:214-408; used with
 * spatial_dims=1, data_range=1.0, kernel_size=7 at :487): per scale a `ksize`-tap (gaussian) valid convolution gives the local
 * moments, cs / ssim maps are averaged over channels and positions, avg_pool1d(2) between scales, out[b] = prod_s relu(.)^w_s
 * with the last scale using ssim.  kernel_host [ksize], weights_host [n_scales] are HOST arrays.  L <= 4096. */
int eegldm_ms_ssim_1d(eegldm_ctx*, const float* a, const float* b, float* out, int B, int C, int L, const float* kernel_host,
                      int ksize, const float* weights_host, int n_scales, float data_range, float k1, float k2);
/* Multitaper PSD of single-channel windows x (B, L), one-sided bins 0..n_bins-1 (bin k = k*sfreq/L Hz) -- what
 * mne's Epochs.compute_psd(fmax=18) computes per epoch at sample_trials.py:172-181 (method "multitaper", normalization "length"):
 * tapers (device, [n_tapers][L]) and weights_host ([n_tapers], sqrt of the DPSS concentrations) come from the host. */
int eegldm_psd_multitaper(eegldm_ctx*, const float* x, const float* tapers, const float* weights_host, int n_tapers, float sfreq,
                          int n_bins, float* psd, int B, int L);

/* ------------------------------------------------------------------ sampler
 * The whole sampling loop of sample_trials.py:149-170 (DDIM, eta 0) or util.py:261-285 / sample_trials_ddpm.py:99-104 (ancestral
 * DDPM, `ancestral` != 0) as one call: x <- noise (B,C,L); for i < n_steps: out = UNet(x, timesteps_host[i]);
 * x = step(out, x; a_t_host[i], a_prev_host[i] [, beta_t_host[i]]); then latents_out (nullable) <- x and windows_out (nullable) <-
 * decode(x * inv_scale_factor) when `ae` is given, else x itself (pixel-space model).  The three schedule arrays are HOST arrays
 * of n_steps entries (a_prev = 1 for the final step).  Ancestral noise is drawn on-device (Philox, noise_seed).
 * use_graph != 0: the UNet forward is captured once per (B, L) into a hipGraph and replayed (launch-bound at small B -- the
 * reference samples one window per call); *graph_used_host (nullable) reports whether the replay path ran. */
int eegldm_sample(eegldm_unet*, eegldm_aekl* ae, const float* noise, const int64_t* timesteps_host, const float* a_t_host,
                  const float* a_prev_host, const float* beta_t_host, int n_steps, int ancestral, int pred_type, int clip_sample,
                  float inv_scale_factor, uint64_t noise_seed, float* latents_out, float* windows_out, int B, int L, int use_graph,
                  int* graph_used_host);
/* Class-conditional sampling (a UNet from eegldm_unet_create_cond): labels_host is a HOST array of B classes in [0, num_classes).
 * guidance_scale w != 1: classifier-free guidance -- every forward runs 2B rows (the B samples with their labels, then the same latents
 * with null_class, which must lie in [0, num_classes) too) and ONE kernel forms out = out_u + w (out_c - out_u) in fp32 on the raw model
 * output and applies the DDIM / DDPM step (eegldm_guided_step).  w == 1 does not run the null-class half: it is the plain conditional
 * sampler.  The embedding rows of all (timestep, class) pairs are computed once per call.  eegldm_sample on a conditional UNet is an error. */
int eegldm_sample_cond(eegldm_unet*, eegldm_aekl* ae, const float* noise, const int64_t* timesteps_host, const float* a_t_host,
                       const float* a_prev_host, const float* beta_t_host, int n_steps, int ancestral, int pred_type, int clip_sample,
                       float inv_scale_factor, uint64_t noise_seed, float* latents_out, float* windows_out, int B, int L, int use_graph,
                       int* graph_used_host, const int64_t* labels_host, float guidance_scale, int64_t null_class);
/* The guided step itself: model_out holds 2n values, the conditional outputs then the null-class outputs; o = o_u + w (o_c - o_u), then
 * eegldm_ddim_step (ancestral == 0) or eegldm_ddpm_step (ancestral != 0; noise may be NULL when a_prev == 1) on `sample` (n values).
 * prev2 (nullable) receives a second copy of the result. */
int eegldm_guided_step(eegldm_ctx*, const float* model_out, float guidance_scale, const float* sample, const float* noise, float a_t,
                       float a_prev, float beta_t, int ancestral, int pred_type, int clip_sample, float* prev, float* prev2, long n);

/* Linear multistep sampling (DPM-Solver++ 2M, Lu et al. 2022; new symbols, ABI 8).  One step as ONE launch, solver-agnostic: everything the
 * solver knows is in the three host-computed coefficients (schedulers.py multistep_coefficients).  Per element, in one pass:
 *   o    = model_out                                   (guided != 0: model_out holds 2n values, the conditional outputs then the null-class
 *                                                       outputs, and o = o_u + w (o_c - o_u) in fp32, as eegldm_guided_step forms it)
 *   x0   = the data prediction from o, sample and a_t   (epsilon / v_prediction / sample, optional clamp to [-1, 1]: the arithmetic of
 *                                                       eegldm_ddim_step)
 *   prev = fma(cx, sample, fma(c0, x0, c1 * hist))      (c1 == 0: fma(cx, sample, c0 * x0), hist is not read)
 *   hist = x0
 * prev2 (a second copy of prev) and pred_x0 are nullable; hist may be NULL only when c1 == 0, and then nothing is read or written there;
 * prev may be `sample` itself; no other two buffers may overlap.  First order (c1 = 0) with c0 = sqrt(a_prev) - cx sqrt(a_t),
 * cx = sqrt((1 - a_prev) / (1 - a_t)) is the DDIM step. */
int eegldm_multistep_step(eegldm_ctx*, const float* model_out, float guidance_scale, int guided, const float* sample, float* hist, float a_t,
                          int pred_type, int clip_sample, float cx, float c0, float c1, float* prev, float* prev2, float* pred_x0, long n);
/* The sampling loop of eegldm_sample / eegldm_sample_cond with eegldm_multistep_step as the step: cx_host / c0_host / c1_host (HOST arrays of
 * n_steps entries) take the place of a_prev / beta_t, the history buffer belongs to the library, and c1_host[0] must be 0 (step 0 has no
 * history).  labels_host NULL: an unconditional UNet; otherwise a class-conditional one with guidance as in eegldm_sample_cond.  Everything
 * else -- embedding table, 2B-row guided forward, eager launches or graph replay, z * inv_scale_factor, decode -- is shared with them. */
int eegldm_sample_multistep(eegldm_unet*, eegldm_aekl* ae, const float* noise, const int64_t* timesteps_host, const float* a_t_host,
                            const float* cx_host, const float* c0_host, const float* c1_host, int n_steps, int pred_type, int clip_sample,
                            float inv_scale_factor, float* latents_out, float* windows_out, int B, int L, int use_graph, int* graph_used_host,
                            const int64_t* labels_host, float guidance_scale, int64_t null_class);

/* Editing: sampling that starts from an input (SDEdit) and keeps a masked region of it (inpainting); new symbols, ABI 8.
 * `known` is the clean signal z0 in the sampler's space, `noise` the caller's ONE noise tensor (used for the start and for every
 * re-noising; nothing is drawn), `mask` in [0, 1] per element, 1 = keep.  With k(a) = fma(sqrt(a), z0, sqrt(1 - a) * noise) (a == 1: z0):
 *   start   x = k(a_t of the first executed step)
 *   blend   after a step has produced x' at the noise level a_next:  x' <- mask == 0 ? x' : mask == 1 ? k(a_next)
 *                                                                           : fma(mask, k(a_next), (1 - mask) * x')
 * so an all-zero mask leaves the step's bytes and an all-one mask returns k(a_next) bit for bit.
 *
 * eegldm_edit_step: one sampling step and the blend in ONE launch.  coef_host == NULL: the DDIM (eta 0) step of eegldm_ddim_step /
 * eegldm_guided_step onto a_prev = a_next; coef_host = HOST {cx, c0, c1}: the step of eegldm_multistep_step (a_next then only sets the
 * blend's noise level).  guided / guidance_scale / hist / prev2 / pred_x0 and the aliasing rules are eegldm_multistep_step's (hist is
 * optional in the DDIM form); hist and pred_x0 receive the model's own data prediction, not a blended one.  mask == NULL: no blend,
 * known / noise are not read and the result is eegldm_ddim_step's / eegldm_multistep_step's, bit for bit (the guided DDIM form agrees
 * with eegldm_guided_step to rounding: that kernel shares its update with the ancestral step and is contracted differently).
 * known / noise / mask may not overlap an output. */
int eegldm_edit_step(eegldm_ctx*, const float* model_out, float guidance_scale, int guided, const float* sample, float* hist, float a_t,
                     float a_next, int pred_type, int clip_sample, const float* coef_host, const float* known, const float* noise,
                     const float* mask, float* prev, float* prev2, float* pred_x0, long n);
/* z0 (nullable) = scale_factor * z_mu and x_start (nullable) = k(a_start) of that z0, one launch; noise / a_start are read only for x_start. */
int eegldm_edit_start(eegldm_ctx*, const float* z_mu, float scale_factor, const float* noise, float a_start, float* z0, float* x_start, long n);
/* The window side.  mask_win (B, 1, Lw).  mask_lat (nullable; (B, C, Lw / down)): every channel's row is the min over the `down` window
 * samples a latent position covers -- a position is kept only if all of them are.  out (nullable; (B, Co, Lw), may be `decoded` itself):
 * the composite mask_win * input + (1 - mask_win) * decoded with the blend's exactness at 0 and 1 (kept samples are the input's bytes). */
int eegldm_edit_window(eegldm_ctx*, const float* mask_win, int B, int Lw, int down, int C, float* mask_lat, const float* input,
                       const float* decoded, int Co, float* out);
/* The sampling loop of eegldm_sample_cond / eegldm_sample_multistep (deterministic steps only) with the edit block: timesteps_host /
 * a_t_host / ... hold the n_steps EXECUTED steps (the tail of the scheduler's grid).  cx_host == NULL: DDIM with a_prev_host; otherwise the
 * multistep form with cx_host / c0_host / c1_host (c1_host[0] == 0: the first executed step has no history) and a_next_host, the noise
 * level each step lands on.  known == NULL: x starts from `noise` (plain sampling); else x = k(a_t_host[0]).
 * With `known` every step is one eegldm_edit_step launch; mask (nullable, needs known): the blend runs inside it, and the null-class
 * half of a guided run receives the blended latents.  labels_host NULL: an unconditional UNet.  known / noise / mask are device buffers of B * C * L floats that stay valid and
 * unwritten during the call. */
int eegldm_sample_edit(eegldm_unet*, eegldm_aekl* ae, const float* noise, const float* known, const float* mask, const int64_t* timesteps_host,
                       const float* a_t_host, const float* a_prev_host, const float* cx_host, const float* c0_host, const float* c1_host,
                       const float* a_next_host, int n_steps, int pred_type, int clip_sample, float inv_scale_factor, float* latents_out,
                       float* windows_out, int B, int L, int use_graph, int* graph_used_host, const int64_t* labels_host, float guidance_scale,
                       int64_t null_class);

/* Long recordings: overlapped-window sampling on one latent canvas (MultiDiffusion, Bar-Tal et al. 2023); new symbols, ABI 8.
 * A recording is ONE noisy canvas (R, C, Lc) longer than the window the UNet was trained on.  Window k covers canvas positions
 * [k S, k S + L) with the stride S = L - (2 m + r), so Lc = (W - 1) S + L; all R * W windows are rows of one forward batch (recording-major:
 * row rec * W + k).  Inside a window the first and last m positions that have a neighbour carry weight 0 (`margin`: where the network sees
 * a conv boundary and its trained-in padding), the next r positions ramp linearly (`ramp`), the interior has weight 1; a recording's free
 * start and end keep weight 1.  In the overlap of windows k and k + 1, with j' = p - (k + 1) S, window k + 1 has the weight
 *   u = 0 (j' < m),   u = (j' - m + 0.5) / r (m <= j' < m + r),   u = 1 (afterwards)        and window k has 1 - u.
 * L >= 3 m + 2 r is required: then S >= 1 and at most two windows carry weight anywhere.  m = r = 0: independent windows side by side.
 * fp32 throughout, any 4-byte alignment of every pointer (16-byte accesses wherever an address allows), no atomics, no memset: every
 * output element has exactly one writer, so results repeat bit for bit.
 *
 * eegldm_canvas_gather: win[rec * W + k][c][l] = canvas[rec][c][k S + l]; win2 (nullable) receives a second copy (the null-class half of
 * a guided forward's input).  Any 1 <= S <= L. */
int eegldm_canvas_gather(eegldm_ctx*, const float* canvas, int R, int C, int W, int L, int S, float* win, float* win2);
/* eegldm_canvas_step: one sampling step of the whole canvas, ONE launch.  model_out holds the forward's output for the R * W window
 * rows ((R W, C, L); guided != 0: twice that, the conditional rows then the null-class rows).  For each canvas element xc:
 *   o    = model_out at that position of each window with non-zero weight there (guided: o_u + w (o_c - o_u), as eegldm_multistep_step)
 *   x0_k = the data prediction from o, xc and a_t, the arithmetic of eegldm_multistep_step (epsilon / v_prediction / sample, optional clamp)
 *   x0   = u == 0 ? x0_k : u == 1 ? x0_{k+1} : fma(u, x0_{k+1}, (1 - u) * x0_k)        (a window with weight 0 is not read)
 *   prev = fma(cx, xc, fma(c0, x0, c1 * hist))      (c1 == 0: fma(cx, xc, c0 * x0), hist is not read);    hist = x0
 * prev goes to canvas_out (may be `canvas` itself) and to EVERY window row that covers the position, weight-0 windows included, in win
 * and win2 (both nullable; (R W, C, L)): the next forward's input is complete without a gather.  hist (canvas-shaped; NULL only when
 * c1 == 0) and pred_x0 (nullable, canvas-shaped) receive the fused prediction.  The update is linear in (x, x0), so fusing the x0 of two
 * windows that share xc equals fusing their updated samples (MultiDiffusion's average).  W == 1 and m == r == 0 are
 * eegldm_multistep_step on the same values, bit for bit.  No two buffers may overlap except canvas_out == canvas. */
int eegldm_canvas_step(eegldm_ctx*, const float* model_out, float guidance_scale, int guided, const float* canvas, float* hist, float a_t,
                       int pred_type, int clip_sample, float cx, float c0, float c1, int R, int C, int W, int L, int m, int r, float* canvas_out,
                       float* win, float* win2, float* pred_x0);
/* eegldm_canvas_compose: the decoded windows (R W, Co, Lw) cross-faded onto the recording (R, Co, (W - 1) Sw + Lw) with the layout at
 * window resolution (Sw == Lw - (2 mw + rw): the latent layout times the autoencoder's downsampling factor): the bytes of the owning
 * window where u is 0 or 1, fma(u, b, (1 - u) * a) inside a ramp. */
int eegldm_canvas_compose(eegldm_ctx*, const float* decoded, int R, int Co, int W, int Lw, int Sw, int mw, int rw, float* out);
/* The loop of eegldm_sample_multistep on R canvases of W windows each: canvas = noise ((R, C, Lc), device), gather, then per step one
 * forward on the R * W rows (2 R W when guided) and ONE eegldm_canvas_step launch; canvas_out (nullable, (R, C, Lc)) receives the final
 * canvas; recording_out (nullable, (R, Co, down * Lc)) the cross-fade (eegldm_canvas_compose) of the R * W windows decoded from the
 * gathered canvas times inv_scale_factor -- with ae == NULL (pixel-space model) the canvas itself (down = 1).  labels_host: R * W classes,
 * recording-major, or NULL for an unconditional UNet; guidance as in eegldm_sample_cond.  cx_host / c0_host / c1_host as in
 * eegldm_sample_multistep (c1_host[0] == 0); solver_order = 1 in schedulers.py is DDIM on the same grid.  Embedding table, eager launches
 * or graph replay are shared with the other loops (the forward state is the one of B = R * W rows). */
int eegldm_sample_long(eegldm_unet*, eegldm_aekl* ae, const float* noise, const int64_t* timesteps_host, const float* a_t_host,
                       const float* cx_host, const float* c0_host, const float* c1_host, int n_steps, int pred_type, int clip_sample,
                       float inv_scale_factor, float* canvas_out, float* recording_out, int R, int W, int L, int m, int r, int use_graph,
                       int* graph_used_host, const int64_t* labels_host, float guidance_scale, int64_t null_class);

/* Repairing and extending real recordings: init and keep-mask on the canvas; new symbols, ABI 8.
 * eegldm_canvas_edit_step: eegldm_canvas_step and the blend of eegldm_edit_step in ONE launch.  known / noise / mask are canvas-shaped
 * ((R, C, Lc) fp32, any 4-byte alignment each, 16-byte accesses where an address allows), read at the canvas index.  Per canvas element
 * the fused data prediction x0 and prev = fma(cx, xc, fma(c0, x0, c1 * hist)) are eegldm_canvas_step's, then
 *   prev <- mask == 0 ? prev : mask == 1 ? k(a_next) : fma(mask, k(a_next), (1 - mask) * prev),
 *   k(a) = fma(sqrt(a), known, sqrt(1 - a) * noise)  (a == 1: known)
 * with the device functions of eegldm_edit_step / eegldm_edit_start, so all three round alike.  The blended value goes to canvas_out and
 * to every covering window row of win / win2, weight-0 windows included (under guidance the null-class half receives the blended
 * latents); hist and pred_x0 receive the model's own fused x0, not a blended one.  mask == NULL: known / noise are not read and the call
 * IS eegldm_canvas_step (the same kernel).  An all-zero mask returns eegldm_canvas_step's bytes, an all-one mask k(a_next).  known / noise
 * / mask may not overlap an output; the aliasing rules are otherwise eegldm_canvas_step's.  No atomics, no memset, one writer per
 * output element. */
int eegldm_canvas_edit_step(eegldm_ctx*, const float* model_out, float guidance_scale, int guided, const float* canvas, float* hist, float a_t,
                            float a_next, int pred_type, int clip_sample, float cx, float c0, float c1, int R, int C, int W, int L, int m, int r,
                            const float* known, const float* noise, const float* mask, float* canvas_out, float* win, float* win2,
                            float* pred_x0);
/* The loop of eegldm_sample_long from a real recording: known / mask (both nullable; device, (R, C, Lc), valid and unwritten during the
 * call) and a_next_host.  All host arrays hold the n_steps EXECUTED steps (the tail of the grid, as in eegldm_sample_edit); a_next_host[i]
 * is the noise level step i lands on; c1_host[0] == 0.  known == NULL: eegldm_sample_long (mask must be NULL too).  Otherwise the canvas
 * starts as k(a_t_host[0]) (eegldm_edit_start on the R C Lc canvas elements), is gathered, and every step is one forward and ONE
 * eegldm_canvas_edit_step launch (mask NULL: without the blend).  Everything else -- embedding table, 2 R W-row guided forward, eager
 * launches or graph replay, the final gather, the window-by-window decode and the compose -- is eegldm_sample_long's. */
int eegldm_sample_long_edit(eegldm_unet*, eegldm_aekl* ae, const float* noise, const float* known, const float* mask,
                            const int64_t* timesteps_host, const float* a_t_host, const float* cx_host, const float* c0_host,
                            const float* c1_host, const float* a_next_host, int n_steps, int pred_type, int clip_sample, float inv_scale_factor,
                            float* canvas_out, float* recording_out, int R, int W, int L, int m, int r, int use_graph, int* graph_used_host,
                            const int64_t* labels_host, float guidance_scale, int64_t null_class);

/* Resampled repair (RePaint, Lugmayr et al. 2022): jumps back up the noise schedule with fresh noise; new symbols, ABI 8.
 * eegldm_edit_jump: ONE launch that takes x from the noise level a step landed on back up to a_level,
 *   p   = fma(jump_x, x, jump_n * eps)        jump_x = sqrt(rho), jump_n = sqrt(1 - rho), rho = a_level / a_landed (from the host)
 *   out = mask == 0 ? p : mask == 1 ? k(a_level) : fma(mask, k(a_level), (1 - mask) * p)
 * with k and the blend of eegldm_edit_step (the same device functions): the kept positions hold k(a_level) bit for bit after a jump as
 * after a step.  fresh != NULL: eps = fresh (device, n floats).  fresh == NULL: eps[e] is DRAWN IN REGISTERS, word e & 3 of the Box-Muller
 * quad of Philox(seed, offset + (e >> 2)) -- the value eegldm_randn(out, n, seed, offset) writes to out[e], bit for bit, a function of
 * (seed, offset, e) alone: not of any pointer's alignment, of the 16-byte body / scalar edge split or of the grid.  mask == NULL: no blend,
 * known / noise are not read.  out may be x itself; out2 (nullable) receives the same values (the null-class half of a guided batch).
 * fp32, any 4-byte alignment per buffer (16-byte accesses where all buffers in use share an offset inside a 16-byte line), no atomics, no
 * memset, one writer per element.  fresh / known / noise / mask may not overlap an output. */
int eegldm_edit_jump(eegldm_ctx*, const float* x, float jump_x, float jump_n, const float* fresh, uint64_t seed, uint64_t offset,
                     const float* known, const float* noise, const float* mask, float a_level, float* out, float* out2, long n);
/* eegldm_sample_edit / eegldm_sample_long_edit with the resampling block.  All host arrays hold ONE ENTRY PER FORWARD (n_steps forwards:
 * schedulers.resample_tables); jump_x_host / jump_n_host describe the jump in front of each forward, (0, 0) = none.  At the top of
 * iteration i with jump_n_host[i] != 0 the loop makes one eegldm_edit_jump launch (x in place, out2 = the null-class half when guided,
 * a_level = a_t_host[i], fresh = NULL, seed = noise_seed, offset = jump_index * ((n + 3) / 4), jump_index counting the call's jumps from
 * 0); on the canvas the jump runs on the n = R C Lc canvas elements and an eegldm_canvas_gather rewrites the window rows.  The step
 * behind a jump must not read the history: c1_host[i] == 0 there, and jump_n_host[0] == 0.  Needs known and mask.  jump_x_host ==
 * jump_n_host == NULL: the predecessor export itself.  Everything else -- embedding table (one row per forward), eager launches or graph
 * replay, decode -- is the predecessor's. */
int eegldm_sample_edit_resample(eegldm_unet*, eegldm_aekl* ae, const float* noise, const float* known, const float* mask,
                                const int64_t* timesteps_host, const float* a_t_host, const float* a_prev_host, const float* cx_host,
                                const float* c0_host, const float* c1_host, const float* a_next_host, int n_steps, int pred_type, int clip_sample,
                                float inv_scale_factor, const float* jump_x_host, const float* jump_n_host, uint64_t noise_seed,
                                float* latents_out, float* windows_out, int B, int L, int use_graph, int* graph_used_host,
                                const int64_t* labels_host, float guidance_scale, int64_t null_class);
int eegldm_sample_long_edit_resample(eegldm_unet*, eegldm_aekl* ae, const float* noise, const float* known, const float* mask,
                                     const int64_t* timesteps_host, const float* a_t_host, const float* cx_host, const float* c0_host,
                                     const float* c1_host, const float* a_next_host, int n_steps, int pred_type, int clip_sample,
                                     float inv_scale_factor, const float* jump_x_host, const float* jump_n_host, uint64_t noise_seed,
                                     float* canvas_out, float* recording_out, int R, int W, int L, int m, int r, int use_graph,
                                     int* graph_used_host, const int64_t* labels_host, float guidance_scale, int64_t null_class);

/* ------------------------------------------------------------------ context conditioning: learned repair and continuation (additive; ABI 8)
 * The Palette / inpainting-LDM form: the denoiser reads the kept signal and the keep-mask as extra input channels and is trained with
 * masks drawn at random, so repair, continuation and plain generation are one model at one forward per step.  Masks: 1 = keep, 0 =
 * regenerate (the convention of the edit entry points), one (L,) row per sample at the sampler's resolution.
 *
 * eegldm_unet_create_ctx: cfg->in_channels is the TOTAL input width; x has Cx = in_channels - context_channels channels, Cx == out_channels
 * and context_channels >= 1 are required (num_classes 0: no classes).  Parameter layout and state-dict keys are those of a plain UNet with
 * that in_channels (input_blocks.0.0.weight is [model_channels][in_channels][3]): the model is the reference UNetModel(in_channels) applied
 * to cat([x, context], 1).
 * eegldm_unet_set_context: context is device fp32 (rows, context_channels, L); the handle keeps the POINTER until it is cleared with NULL.
 * A forward of B rows requires B % rows == 0 and row b reads context row b % rows (both halves of a guided 2B batch share one copy); with
 * no context set a forward reads zeros.  The forward writes x into columns [0, Cx) and the context into columns [Cx, in_channels) of the
 * first conv's channels-last input in one launch; everything behind the first conv is unchanged.
 * THE CONTEXT GETS NO GRADIENT: eegldm_unet_backward on a context UNet accumulates every parameter gradient (the first conv's context
 * columns included) and writes dx (nullable) for the Cx columns of x only.
 * The unconditional / plain train steps (eegldm_ldm_train_step, _cond, _weighted) refuse a context UNet. */
int eegldm_unet_create_ctx(eegldm_ctx*, const eegldm_unet_cfg* cfg, int num_classes, int context_channels, eegldm_unet** out);
int eegldm_unet_set_context(eegldm_unet*, const float* context, int rows);
/* The training masks.  Sample b takes the four words w0..w3 of Philox(seed, offset + b) -- advance offset by B per step, as for
 * eegldm_label_dropout -- and u0 = (float)w0 * 2^-32 compared in fp32 as eegldm_label_dropout compares its word:
 *   u0 < p_none                        the mask is all 0: no context (the unconditional case, and what classifier-free training needs)
 *   else u0 < p_none + p_prefix        continuation: keep [0, s), regenerate [s, L), s = 1 + ((w1 * (L - 1)) >> 32); L == 1: all 0
 *   else                               one span: len = span_min + ((w1 * (span_max - span_min + 1)) >> 32),
 *                                      start = (w2 * (L - len + 1)) >> 32; regenerate [start, start + len), keep the rest
 * (p_none + p_prefix is the fp32 sum; the ranges are 64-bit products of 32-bit words, so a numpy uint64 restatement is bit-exact).
 * Refused before any launch: span_min < 1, span_max < span_min, span_max > L, a probability outside [0, 1], p_none + p_prefix > 1.
 * mask: device fp32 (B, L), one launch, vector stores. */
int eegldm_context_mask(eegldm_ctx*, float* mask, int B, int L, float p_none, float p_prefix, int span_min, int span_max, uint64_t seed,
                        uint64_t offset);
/* What a context train step feeds the UNet, in ONE launch: noisy = sqrt(a_t) x0 + sqrt(1 - a_t) noise (the bytes of eegldm_add_noise: one
 * device function), context[:, :C] = m * ctx_src (ctx_src NULL: x0), context[:, C] = m; context is (B, C + 1, L), the others (B, C, L).
 * mask (B, L) given: m is read from it and the draw's parameters are ignored.  mask == NULL: row b's mask is derived in registers from
 * (seed, offset + b) exactly as eegldm_context_mask derives it -- no mask buffer is written or re-read, unless mask_out (nullable, (B, L))
 * asks for a copy.  fp32, any 4-byte alignment per buffer: 16-byte accesses with a scalar head and tail wherever the buffers of a row
 * share an offset inside a 16-byte line (always, when L % 4 == 0 and the bases do), else element by element.  No atomics, no memset, one
 * writer per element.  No output may overlap an input or another output. */
int eegldm_add_noise_context(eegldm_ctx*, const float* x0, const float* ctx_src, const float* noise, const int64_t* t, const float* acp,
                             const float* mask, float p_none, float p_prefix, int span_min, int span_max, uint64_t seed, uint64_t offset,
                             float* noisy, float* context, float* mask_out, int B, int C, int L);
/* out = windows * upsample_nearest(mask, down): windows / out (B, Co, Lw), mask (B, Lw / down).  The masked input of the context encode: a
 * latent next to a hole is computed by the encoder from the hole's true content, which is absent at repair time, so the LDM context is
 * scale_factor * encode_mean(windows * upsample(mask)) in training and in sampling alike.  Exact (a multiply by the mask value). */
int eegldm_context_window(eegldm_ctx*, const float* windows, const float* mask, int down, float* out, int B, int Co, int Lw);
/* eegldm_ldm_train_step_weighted on a context UNet whose context_channels == out_channels + 1: eegldm_add_noise_context (ctx_latents
 * nullable: the latents themselves; mask nullable: drawn from (mask_seed, mask_offset + b) with the draw's parameters; mask_out nullable),
 * eegldm_unet_set_context, forward, eegldm_diffusion_loss over the WHOLE sample (the kept positions too), backward.  The context is
 * cleared before returning.  Refuses a UNet built without context channels. */
int eegldm_ldm_train_step_ctx(eegldm_unet*, const float* latents, const float* noise, const int64_t* t, const float* acp, int pred_type,
                              int B, int L, float grad_scale, float* loss, const float* wtab, float* per_sample, const int64_t* labels,
                              float p_uncond, int64_t null_class, uint64_t seed, uint64_t offset, const float* ctx_latents, const float* mask,
                              float p_none, float p_prefix, int span_min, int span_max, uint64_t mask_seed, uint64_t mask_offset,
                              float* mask_out);
/* eegldm_sample_edit_resample / eegldm_sample_long_edit_resample with the context every forward reads: device (context_rows,
 * context_channels, L) with B % context_rows == 0, or -- canvas form -- canvas-shaped (R, context_channels, Lc), gathered ONCE per call into
 * window rows with eegldm_canvas_gather.  The loop copies the context into a buffer of its own, one row per forward row, and points the
 * handle there: a captured graph outlives the call and never reads the caller's pointer.  context == NULL: the predecessor itself; every
 * sampling export accepts a context UNet and then runs it on a zero context.  known == NULL with a context: the learned conditioning
 * alone, without the replacement blend. */
int eegldm_sample_edit_ctx(eegldm_unet*, eegldm_aekl* ae, const float* noise, const float* known, const float* mask,
                           const int64_t* timesteps_host, const float* a_t_host, const float* a_prev_host, const float* cx_host,
                           const float* c0_host, const float* c1_host, const float* a_next_host, int n_steps, int pred_type, int clip_sample,
                           float inv_scale_factor, const float* jump_x_host, const float* jump_n_host, uint64_t noise_seed,
                           float* latents_out, float* windows_out, int B, int L, int use_graph, int* graph_used_host,
                           const int64_t* labels_host, float guidance_scale, int64_t null_class, const float* context, int context_rows);
int eegldm_sample_long_edit_ctx(eegldm_unet*, eegldm_aekl* ae, const float* noise, const float* known, const float* mask,
                                const int64_t* timesteps_host, const float* a_t_host, const float* cx_host, const float* c0_host,
                                const float* c1_host, const float* a_next_host, int n_steps, int pred_type, int clip_sample,
                                float inv_scale_factor, const float* jump_x_host, const float* jump_n_host, uint64_t noise_seed,
                                float* canvas_out, float* recording_out, int R, int W, int L, int m, int r, int use_graph,
                                int* graph_used_host, const int64_t* labels_host, float guidance_scale, int64_t null_class,
                                const float* context, int context_rows);

/* ------------------------------------------------------------------ the sampling loop by descriptor (additive; ABI 8)
 * ONE loop serves every eegldm_sample_* export above: each of them fills this descriptor from its argument list and calls
 * eegldm_sample_run, so they are its fixed-form shorthands and a caller may fill the descriptor itself.  Zero-initialise it, set `size`
 * and what the call uses: a NULL pointer or a zero count means "this part is not used".  HOST arrays hold n_steps entries, one per forward;
 * everything else is a device buffer of fp32 that stays valid and unwritten during the call.  Every rule below is checked before the first
 * launch or allocation, and a refused call leaves no state behind.  Group by group:
 *   size              sizeof(eegldm_sample_desc); anything else is refused before another member is read.
 *   unet, ae, noise   the denoiser; the autoencoder that decodes the result (NULL: pixel-space model, x IS the window; else it shares the
 *                     UNet's context); the caller's ONE noise tensor -- x starts as `noise`, and every re-noising of `known` uses it.
 *   B, L              window form: x is (B, C, L), C the UNet's x channels (== its out_channels).
 *   R, W, m, r,       canvas form, selected by R > 0 (B is then not read; needs the multistep step): the R * W <= 0x3fffffff forward rows
 *   canvas_out,       are the overlapping slices of R canvases (window length L, margin m, ramp r >= 0, L >= 3 m + 2 r: "Long recordings"
 *   recording_out     above).  noise / known / mask / context are canvas-shaped (R, ., Lc); x starts as the gathered canvas, and every step
 *                     is ONE eegldm_canvas_step (with `known`: eegldm_canvas_edit_step) launch that updates the canvas AND rewrites the
 *                     slices the next forward reads.  canvas_out (R, C, Lc) receives the final canvas; recording_out (R, Co, down * Lc)
 *                     the cross-fade (eegldm_canvas_compose) of the R * W windows decoded from the gathered canvas times inv_scale_factor,
 *                     without `ae` the canvas itself.  One of the two is required; latents_out / windows_out are not read.
 *   n_steps,          HOST: per forward the timestep the UNet sees and alphas_cumprod there.  The embedding rows of all (timestep, class)
 *   timesteps, a_t    pairs are computed once per call.
 *   a_prev, beta_t,   the DDIM step (eta 0; eegldm_ddim_step, guided: eegldm_guided_step) onto a_prev[i] (HOST; 1 for the final step), or
 *   ancestral,        with ancestral != 0 the DDPM step (eegldm_ddpm_step), which also needs beta_t (HOST) and draws its noise on the device:
 *   noise_seed        Philox key noise_seed, step i at offset i * ceil(n / 4), n = B C L.  noise_seed is also the key of the jumps below;
 *                     the two never occur together (the ancestral step is refused with `known`).
 *   cx, c0, c1,       HOST.  cx != NULL selects the linear multistep step (eegldm_multistep_step, one launch behind every forward; the
 *   a_next            history buffer belongs to the library): a_prev is then not read and ancestral must be 0.  c1[0] must be 0: the first
 *                     executed step has no history.  a_next[i], the noise level step i lands on, is needed with `known` (the DDIM form
 *                     lands on a_prev[i]).
 *   pred_type,        EEGLDM_PRED_*; clamp the data prediction to [-1, 1]; windows_out / recording_out decode x * inv_scale_factor
 *   clip_sample,      (1 / scale_factor; read only with `ae`, and a zeroed value there is a factor of 0, not "off").
 *   inv_scale_factor
 *   labels,           HOST, one class in [0, num_classes) per forward row (canvas form: recording-major).  Required for a UNet built with
 *   guidance_scale,   classes, refused for one without.  guidance_scale and null_class are read only when labels are given, and a zeroed
 *   null_class        guidance_scale there means w = 0 (the null class alone), NOT "off": w = 1 is the plain conditional sampler.  w != 1
 *                     runs every forward on twice the rows -- the samples with their labels, then the same latents with null_class, which
 *                     must lie in [0, num_classes) -- and the step forms out_u + w (out_c - out_u) on the raw model output.  NaN is refused.
 *   known, mask       the edit start and the blend ("Editing" above).  known != NULL: x starts as k(a_t[0]) of `known` and `noise`
 *                     (eegldm_edit_start) and every step is ONE eegldm_edit_step launch; deterministic steps only.  mask != NULL (needs
 *                     known): that launch also blends towards k(level the step lands on); without a mask the same launch runs without
 *                     the blend, so an all-zero mask and no mask give the same bytes.  The null-class half receives the blended latents.
 *   jump_x, jump_n    HOST, both or neither; need known and mask ("Resampled repair" above).  In front of forward i with jump_n[i] != 0
 *                     ONE eegldm_edit_jump launch takes x in place (out2 = the null-class half when guided) back up to the level a_t[i]:
 *                     fresh = NULL, seed = noise_seed, offset = jump_index * ((n + 3) / 4), jump_index counting the call's jumps from 0;
 *                     on the canvas the jump runs on the n = R C Lc canvas elements and an eegldm_canvas_gather rewrites the window rows.
 *                     jump_n[0] must be 0, no entry may be NaN, and c1[i] must be 0 behind a jump: the history is not cleared, only unread.
 *   context,          on a UNet from eegldm_unet_create_ctx only: device (context_rows, context_channels, L) with B % context_rows == 0 --
 *   context_rows      sample b reads row b % context_rows -- or, canvas form, (R, context_channels, Lc) with context_rows == R, gathered
 *                     ONCE per call into window rows.  The loop copies it into a buffer of its own (one row per forward row, both halves
 *                     of a guided batch) and points the handle there: a captured graph outlives the call and never reads the caller's
 *                     pointer.  A context UNet without a context runs on zeros.
 *   latents_out,      window form, one of them required: the final x (B, C, L), and its decode (B, Co, down * L) -- without `ae` x itself.
 *   windows_out
 *   use_graph,        use_graph != 0: the UNet forward is captured once per (forward rows, L) into a hipGraph and replayed (launch-bound at
 *   graph_used        small B); *graph_used (HOST, nullable) reports whether the replay path ran.  Eager launches are the default.
 * One context = one thread: the call swaps the context's stream for its duration. */
typedef struct eegldm_sample_desc {
  uint32_t size;
  eegldm_unet* unet; eegldm_aekl* ae; const float* noise;
  int B, L;
  int R, W, m, r; float *canvas_out, *recording_out;
  int n_steps; const int64_t* timesteps; const float* a_t;
  const float *a_prev, *beta_t; int ancestral; uint64_t noise_seed;
  const float *cx, *c0, *c1, *a_next;
  int pred_type, clip_sample; float inv_scale_factor;
  const int64_t* labels; float guidance_scale; int64_t null_class;
  const float *known, *mask;
  const float *jump_x, *jump_n;
  const float* context; int context_rows;
  float *latents_out, *windows_out;
  int use_graph; int* graph_used;
} eegldm_sample_desc;
int eegldm_sample_run(const eegldm_sample_desc* desc);

/* ------------------------------------------------------------------ data-parallel collectives (RCCL over xGMI)
 * One communicator per process / GPU.  Stands where the reference gathers gradients with single-process nn.DataParallel
 * (train_ldm.py:190-192, train_autoencoderkl.py:230-233): every rank means the model's flat fp32 gradient buffer across ranks, the
 * parameters of rank 0 are broadcast once at start (BASELINE configs[3]: 8 ranks, global batch 2048).  Collectives run on the
 * communicator's own stream, ordered after the work enqueued on the context's stream at the time of the call; eegldm_comm_wait makes
 * the context's stream wait for them.  RCCL is loaded with dlopen when the first communicator is created (no link-time dependency).
 * id128: the 128-byte ncclUniqueId made by ONE rank with eegldm_comm_unique_id and handed to the others by the launcher
 * (eegldm.distributed passes it through the torch.distributed store). */
typedef struct eegldm_comm eegldm_comm;
int eegldm_comm_unique_id(char* out128);
int eegldm_comm_create(eegldm_ctx*, const char* id128, int rank, int world, eegldm_comm** out);
int eegldm_comm_destroy(eegldm_comm*);
int eegldm_comm_rank(const eegldm_comm*);
int eegldm_comm_world(const eegldm_comm*);
/* buf[0..n) <- mean over ranks, in place, as ceil(n / bucket_elems) collectives in one group (bucket_elems <= 0: one) */
int eegldm_comm_allreduce_mean_f32(eegldm_comm*, float* buf, long n, long bucket_elems);
int eegldm_comm_broadcast_f32(eegldm_comm*, float* buf, long n, int root);
int eegldm_comm_wait(eegldm_comm*);

/* ------------------------------------------------------------------ PatchDiscriminator
 * PatchDiscriminator(spatial_dims=1, num_layers_d, num_channels, in_channels, out_channels, kernel_size=3,
 * norm="BATCH", bias, padding=1) -- monai-generative, config/config_aekl_eeg.yaml:30-40.  forward returns the
 * last feature map (the reference indexes [-1], train_autoencoderkl.py:213).  BatchNorm running statistics live
 * in a separate caller-owned flat fp32 `buffers` array (num_batches_tracked stored as a float count). */
typedef struct {
  int in_channels, out_channels, num_channels, num_layers_d, kernel_size, padding, bias;
  int dtype;
} eegldm_disc_cfg;
int eegldm_disc_create(eegldm_ctx*, const eegldm_disc_cfg* cfg, eegldm_disc** out);
int eegldm_disc_destroy(eegldm_disc*);
int eegldm_disc_num_entries(const eegldm_disc*);
long eegldm_disc_num_params(const eegldm_disc*);
int eegldm_disc_entry(const eegldm_disc*, int i, char* name, int name_cap, long* offset, long* numel, int* ndim, int shape[3]);
int eegldm_disc_num_buffer_entries(const eegldm_disc*);
long eegldm_disc_num_buffers(const eegldm_disc*);
int eegldm_disc_buffer_entry(const eegldm_disc*, int i, char* name, int name_cap, long* offset, long* numel, int* ndim, int shape[3]);
int eegldm_disc_bind(eegldm_disc*, float* params, float* grads, float* buffers);
int eegldm_disc_sync_weights(eegldm_disc*);
/* training == 1: batch statistics + running-stat update (momentum 0.1); training == 2: batch statistics, running statistics left
 * untouched (a re-forward of an earlier input for its backward); 0: running statistics */
int eegldm_disc_forward(eegldm_disc*, const float* x, float* logits, int B, int L, int training);
/* MONAI PatchDiscriminator.forward returns the list of per-block feature maps (callers index [-1] = the logits,
 * train_autoencoderkl.py:213).  Feature `index` (0 = initial conv + LeakyReLU, then one per conv + BatchNorm + LeakyReLU layer)
 * of the most recent forward, copied out as fp32 (B, C, L); out == NULL only reports *C / *L. */
int eegldm_disc_feature(eegldm_disc*, int index, float* out, int* C, int* L);
/* param_grads != 0: grads += d/dparams; dx (nullable) = d/dx */
int eegldm_disc_backward(eegldm_disc*, const float* dlogits, float* dx, int param_grads);

/* The AEKL/GAN step body (train_autoencoderkl.py:203-234) for one batch: generator forward, L1 + KL + adversarial
 * (+ spectral when use_spectral) backward into the autoencoder's gradient buffer, then the two discriminator
 * passes (fake -> 0, real -> 1, 0.5*adv_weight each) into the discriminator's gradient buffer; BatchNorm running
 * statistics are updated three times, as in the reference.  Both gradient buffers must be zeroed by the caller
 * (optimizer.zero_grad) and both Adam steps run after the call; the result equals the reference order because the
 * discriminator passes only consume `reconstruction.detach()`.
 * losses: device float[6] = recons L1, spectral, KL, generator adversarial, D fake, D real.  recon_out nullable. */
int eegldm_aekl_train_step(eegldm_aekl*, eegldm_disc*, const float* x, const float* eps, float adv_weight, float kl_weight,
                           float spectral_weight, int use_spectral, float* losses, float* recon_out, int B, int L);

/* ------------------------------------------------------------------ FID on U-Sleep features
 * The feature extractor of /root/reference/src/compute_fid.py:357-386: USleep(in_chans=2, sfreq=100, depth=12, ...) of
 * /root/reference/src/models/usleep.py:101-287, forward only, fp32, reference (B, C, T) layout.  kernel_size = round(time_conv_size_s *
 * sfreq) (7 at 100 Hz), input_size = ceil(input_size_s * sfreq) (the classifier's AvgPool1d window).  Parameters live in ONE flat
 * fp32 buffer (conv weights in the reference's (Cout, Cin, K) layout), BatchNorm running statistics + num_batches_tracked (as floats)
 * in a second one; eegldm_usleep_entry lists both in the reference's state_dict order (kind 0 = parameter, 1 = buffer). */
typedef struct eegldm_usleep eegldm_usleep;
typedef struct {
  int in_chans, depth, n_time_filters, n_classes, kernel_size, input_size, with_skip_connection;
  float complexity_factor;
} eegldm_usleep_cfg;
int eegldm_usleep_create(eegldm_ctx*, const eegldm_usleep_cfg*, eegldm_usleep** out);
int eegldm_usleep_destroy(eegldm_usleep*);
long eegldm_usleep_num_params(const eegldm_usleep*);
long eegldm_usleep_num_buffers(const eegldm_usleep*);
int eegldm_usleep_num_entries(const eegldm_usleep*);
int eegldm_usleep_channel(const eegldm_usleep*, int i);      /* c_i of usleep.py:165-172, i = 0 .. depth + 1; -1 out of range */
int eegldm_usleep_entry(const eegldm_usleep*, int i, char* name, int name_cap, int* kind, long* offset, long* numel, int* ndim, int shape[3]);
int eegldm_usleep_bind(eegldm_usleep*, float* params, float* buffers);
/* USleep.forward (usleep.py:249-287): x (B, in_chans, T) -> y_pred (B, n_classes, T / input_size), decoder output (B, c_1, T) and the
 * bottleneck (B, c_{depth+1}, Lb); each output is optional, and without y_pred and decoder_out the decoder is skipped (the FID feature
 * of compute_fid.py:380-381 is the bottleneck).  training != 0: BatchNorm on batch statistics + running-statistics update -- what the
 * reference script runs, since it never calls model.eval(). */
int eegldm_usleep_forward(eegldm_usleep*, const float* x, float* y_pred, float* decoder_out, float* bottom, int B, int T, int training);
/* ---- U-Sleep training (csrc/usleep_train.hip): fp32, additive (EEGLDM_ABI_VERSION stays 8).  Every reduction is written partials folded
 * in a fixed order (no float atomics): a step repeats bit for bit.  Gradients ACCUMULATE (+=) into the flat buffer bound here, laid out as
 * the parameter buffer of eegldm_usleep_bind. */
int eegldm_usleep_bind_grads(eegldm_usleep*, float* grads);
/* Training forward: BatchNorm on batch statistics (fp64 partial sums, ordered fold) + the running-statistics update of
 * eegldm_usleep_forward(training = 1); writes y_pred (B, n_classes, T / input_size) and keeps the tape in the object's arena (per layer the
 * ELU output z, mean / rstd, the normalised output; NOT x, which the first conv's weight gradient reads: keep it until the backward has run).
 * Refused before any launch: unbound gradients, T < input_size, B * bottleneck length < 2
 * (batch statistics over one value do not exist; torch raises too). */
int eegldm_usleep_forward_train(eegldm_usleep*, const float* x, float* y_pred, int B, int T);
/* Backward of the taped forward from dy_pred (B, n_classes, S): parameter gradients +=, dx (B, in_chans, T) written when not NULL.
 * EEGLDM_ERR_INVALID, and nothing launched, when there is no tape or it is stale: ANY other forward on this object (eegldm_usleep_forward in
 * either mode) reuses the arena and invalidates it. */
int eegldm_usleep_backward(eegldm_usleep*, const float* dy_pred, float* dx /* nullable */);
/* forward_train + weighted stage cross-entropy + backward.  labels (B, S) int64 on the device, any negative label is ignored; class_weight
 * [n_classes] or NULL; loss = sum_i w[l_i] nll_i / sum_i w[l_i] (F.cross_entropy(weight=, ignore_index=-1), mean reduction; all ignored: loss
 * and gradients 0).  Gradients are scaled by grad_scale, *loss_out (device) is not.  A label >= n_classes takes no part, and sets a device
 * flag that eegldm_usleep_label_error reads (labels are device memory: the host cannot look at them without a synchronisation). */
int eegldm_usleep_train_step(eegldm_usleep*, const float* x, const int64_t* labels, const float* class_weight /* nullable */, int B, int T,
                             float grad_scale, float* loss_out, float* y_pred /* nullable */);
/* Waits for the context's stream, *out = 1 when a train step since the last call met a label >= n_classes (the flag is cleared). */
int eegldm_usleep_label_error(eegldm_usleep*, int* out);
/* kernels launched by the last eegldm_usleep_train_step / _forward_train / _backward on this object */
long eegldm_usleep_last_launches(const eegldm_usleep*);
/* The loss alone: logits (B, n_classes, S) -> *loss_out, dlogits (nullable; scaled by grad_scale), label_flag (nullable device int). */
int eegldm_usleep_stage_loss(eegldm_ctx*, const float* logits, const int64_t* labels, const float* class_weight /* nullable */, int B, int n_classes,
                             int S, float grad_scale, float* loss_out, float* dlogits, int* label_flag);
/* Primitives of the backward, exported for the tests (in the manner of eegldm_batchnorm_lrelu_*).
 * conv_bwd: one conv1d 'same' layer (left pad (K - 1) / 2: an even K pads the extra zero on the right) over the forward's virtual input
 * [a (B, Ca, La), nearest x2 when ups | b2 (B, Cb, Lb)], both cropped to L; dz (B, Cout, L).  dA (B, Ca, La) and dB2 (B, Cb, Lb) are WRITTEN
 * (cropped-off positions 0; ups: dA[q] = dv[2q] + dv[2q + 1]), dw (Cout, Ca + Cb, K) and db += .  nsplit: splits of the B * L rows of the
 * weight gradient (written partials + ordered fold when > 1), 0 = chosen from the shape.  Any output may be NULL (dw and db together). */
int eegldm_usleep_conv_bwd(eegldm_ctx*, const float* a, int Ca, int La, int ups, const float* b2, int Cb, int Lb, int L, const float* w,
                           const float* dz, int B, int Cout, int K, int nsplit, float* dA, float* dB2, float* dw, float* db);
/* ELU + train-mode BatchNorm backward from the ELU output z (B, C, L) and the batch's mean / rstd [C]:
 * dz = ELU'(z) * gamma * rstd * (dy - mean(dy) - zhat * mean(dy * zhat)), ELU'(z) = z > 0 ? 1 : z + 1; dgamma += sum dy * zhat, dbeta += sum dy
 * (sums in fp64).  dz may alias dy. */
int eegldm_usleep_elu_bn_bwd(eegldm_ctx*, const float* dy, const float* z, const float* mean, const float* rstd, const float* gamma, float* dz,
                             float* dgamma, float* dbeta, int B, int C, int L);
/* MaxPool1d(2) over ConstantPad1d(1, 0) at odd L, backward: x (nrows, L), dpool (nrows, Lo), dx = (dskip ? dskip : 0) + gradient at the
 * arg-max (the first NaN of a pair, else the larger value; equal values: the lower padded index; the pad's zero wins: dropped).  Exact. */
int eegldm_usleep_maxpool_bwd(eegldm_ctx*, const float* x, const float* dpool, const float* dskip /* nullable */, float* dx, long nrows, int L);
/* Classifier head + loss, forward and backward: x (B, C1, L) decoder output; weights / grads: {clf.0.weight, clf.0.bias, clf.3.weight, clf.3.bias,
 * clf.5.weight, clf.5.bias} (grads +=); writes *loss_out, logits (B, n_classes, L / input_size) and dx (B, C1, L; 0 past S * input_size). */
int eegldm_usleep_clf_loss(eegldm_ctx*, const float* x, const float* const* weights, float* const* grads, const int64_t* labels,
                           const float* class_weight /* nullable */, int B, int C1, int L, int input_size, int n_classes, float grad_scale,
                           float* loss_out, float* logits, float* dx, int* label_flag /* nullable */);
/* Primitives of the forward, exported for the tests (additive, ABI 8); they add no launch to any model path.
 * layer_fwd: one conv1d 'same' -> + bias -> ELU -> BatchNorm [-> ConstantPad1d(1, 0) at odd L + MaxPool1d(2)] layer over the virtual input
 * [a (B, Ca, La), nearest x2 when ups | b2 (B, Cb, Lb)], both cropped to L, through the launch helpers the model runs.
 *   mode 0: the inference path in eval mode (BatchNorm folded from the running statistics into the conv's epilogue);
 *   mode 1: the inference path on batch statistics (fp64 atomics, finalize, affine pass), running statistics and counter updated;
 *   mode 2: the training path (written fp64 partials folded in order, stats, apply or the fused apply + pool), the same update; left must be
 *           (K - 1) / 2.
 * y (B, Cout, L) is written; pooled (B, Cout, Lo), Lo = (L + (L odd ? 2 : 0)) / 2, z (the ELU output before BatchNorm; modes 1 and 2) and
 * stat (mean [Cout] | rstd [Cout]; mode 2) are optional.  A NaN in either position of a pooled pair is the pair's maximum, as in torch.
 * Modes 1 and 2 need B * L >= 2.  The call returns after the stream has drained. */
int eegldm_usleep_layer_fwd(eegldm_ctx*, int mode, const float* a, int Ca, int La, int ups, const float* b2 /* nullable */, int Cb, int Lb, int L,
                            const float* w, const float* bias, const float* gamma, const float* beta, float* running_mean, float* running_var,
                            float* num_batches_tracked, int B, int Cout, int K, int left, float* y, float* pooled /* nullable */,
                            float* z /* nullable */, float* stat /* nullable */);
/* ConstantPad1d(1, 0) at odd L + MaxPool1d(2) alone: x (nrows, L) -> y (nrows, Lo); the zeros take part in the max, a NaN wins its pair. */
int eegldm_usleep_maxpool_fwd(eegldm_ctx*, const float* x, float* y, long nrows, int L);
/* The inference classifier head: x (B, C1, L) -> y (B, ncls, L / win); weights as in eegldm_usleep_clf_loss; positions past (L / win) * win
 * are not read. */
int eegldm_usleep_clf_fwd(eegldm_ctx*, const float* x, const float* const* weights, int B, int C1, int L, int win, int ncls, float* y);
/* First and second moments of a feature batch (N, D), accumulated in fp64 device buffers the caller zeroed: sum[D] += sum_n f[n],
 * outer[D][D] += sum_n f[n] f[n]^T.  mean = sum / N, covariance = (outer - N mean mean^T) / (N - 1) are the inputs of the Frechet
 * distance (compute_fid.py:412-414 = monai-generative FIDMetric: torch.mean, unbiased _cov, trace of the matrix square root). */
int eegldm_feature_moments(eegldm_ctx*, const float* feats, long N, int D, double* sum, double* outer);

/* ---- nearest-neighbour search (memorisation audit, precision / recall / coverage; csrc/knn.hip).  fp32 in and out; additive, ABI 8.
 * Score s(i, j) = xbias[j] - 2 <q_i, x_j>, smaller is nearer: xbias = |x_j|^2 orders by squared Euclidean distance (d^2 = max(0, |q_i|^2 + s)),
 * xbias = NULL (= 0) on rows of zero mean and unit norm orders by Pearson correlation (r = -s / 2), xbias = |x_j|^2 - radius_j^2 finds the
 * nearest corpus BALL (|q_i|^2 + s <= 0: query i lies inside some ball).
 * eegldm_knn_update merges one corpus chunk x (Nc rows, row j carries index index_base + j) into the running state best_s [Nq][k] fp32 /
 * best_i [Nq][k] int64, sorted ascending by (score, index), which the caller initialises to +inf / -1.  self_base >= 0 skips the pair with
 * index_base + j == self_base + i (neighbours inside one set); < 0: no pair is skipped.  ldq / ldx are row strides in floats (>= D), so a
 * crop of a window is a view.  1 <= k <= 32, D >= 1; q, x, xbias, best_s need 4-byte alignment only (best_i 8).  A NaN score never enters a
 * list; with fewer than k rows seen the tail stays +inf / -1.  The dot product of a pair is one fmaf chain in ascending k on the f32-input
 * MFMA whatever the pair's place in a tile, slab or chunk, and nothing is accumulated across workgroups: the state after a sequence of calls
 * depends only on the set of rows seen, bit for bit.  Workspace O(Nq * slabs * k) (the context's split-K buffer, main stream). */
int eegldm_knn_update(eegldm_ctx*, const float* q, long ldq, const float* x, long ldx, const float* xbias, int Nq, int Nc, int D, int k,
                      long index_base, long self_base, float* best_s, int64_t* best_i);
/* out[n] = sum_d x[n][d]^2: one wave per row, lane l chains elements l, l + 64, ... with fmaf, then a fixed butterfly -- the value of a row
 * does not depend on N or on the grid. */
int eegldm_rows_sqnorm(eegldm_ctx*, const float* x, long ldx, long N, int D, float* out);
/* out[n] = (x[n] - mean(x[n])) / |x[n] - mean(x[n])|_2, statistics in fp32 in the same fixed order; a constant row becomes all zeros. */
int eegldm_rows_standardize(eegldm_ctx*, const float* x, long ldx, long N, int D, float* out, long ldout);
/* out_d2[i][r] = sum_d (q[i][d] - x[j][d])^2 in direct form (no cancellation) for every slot whose index best_i[i][r] = index_base + j lies
 * in this chunk (0 <= j < Nc); other slots are left as they are. */
int eegldm_knn_rescore(eegldm_ctx*, const float* q, long ldq, const float* x, long ldx, int Nq, int D, int k, long index_base, long Nc,
                       const int64_t* best_i, float* out_d2);

/* ---- kernel matrix times a thin matrix (MMD^2, KID, permutation two-sample test, MMD witness; csrc/kmm.hip).  fp32 in, float64 out;
 * additive, ABI 8.
 *   R[i][p] = sum_j k(a_i, b_j) V[j][p]     0 <= i < Na, 0 <= j < Nb, 0 <= p < P;  pairs with j - i == diag_off are left out
 *   kind 0 (poly): k = (gamma <a, b> + coef0)^degree, degree 1..4 by repeated multiplication (KID: degree 3, gamma 1 / D, coef0 1)
 *   kind 1 (rbf):  k = (1 / S) sum_s exp(-betas_host[s] d2), d2 = max(0, asq[i] + bsq[j] - 2 <a, b>), S = n_betas in 1..8, beta = 1 / (2 sigma^2);
 *                  asq / bsq are the caller's eegldm_rows_sqnorm outputs and are taken as given (poly ignores them: NULL is fine).
 * The Na x Nb kernel matrix never exists: a workgroup evaluates it in 128 x 128 tiles (f32-input MFMA: the dot product of a pair is one fmaf
 * chain in ascending k whatever the pair's place), applies k in fp32, and multiplies each tile at once by its 128 x P slice of V (fmaf chains
 * of 32 rows of B, each from zero in ascending j); the chains' results are added in float64.  out [Na][ldo] float64 is stored, or added onto when accumulate != 0, so B
 * can be streamed in chunks (diag_off then counts from the chunk's first row).  EEGLDM_KMM_NO_DIAG leaves no pair out; left-out pairs and
 * rows past Nb are removed by selection, so a NaN or inf there never reaches a sum.  Elsewhere non-finite values propagate as in K @ V under
 * IEEE rules: a NaN row of B makes every R[i][p] NaN, also where V[j][p] == 0.
 * lda / ldb / ldv / ldo are row strides in elements (>= D, D, P, P).  1 <= P <= 64, D >= 1, Na >= 1, Nb >= 0 (Nb == 0: zeros, or out left as
 * it is when accumulating); a, asq, b, bsq, v need 4-byte alignment only, out 8.  Every refusal leaves out untouched.  B's tiles are cut into
 * at most 32 slabs by a rule that depends on Nb alone; slab partials are summed from zero in index order, then stored or added onto out: no
 * atomics, no memset, a result repeats bit for bit, a row of R does not depend on Na and a column not on P.  Workspace: slabs x rows x P
 * float64 in the context's split-K buffer (main stream), at most 64 MiB: row blocks run in groups beyond that, which changes no bit. */
#define EEGLDM_KMM_NO_DIAG  (-0x7fffffffffffffffL - 1)
int eegldm_kernel_matmul(eegldm_ctx*, const float* a, long lda, const float* asq, const float* b, long ldb, const float* bsq,
                         const float* v, long ldv, int Na, int Nb, int D, int P,
                         int kind /* 0 poly, 1 rbf */, int degree, float gamma, float coef0, const float* betas_host, int n_betas,
                         long diag_off, int accumulate, double* out, long ldo);

/* ---- sleep micro-structure primitives (spindle and slow-wave detectors of eegldm.metrics; csrc/events.hip).  fp32; additive, ABI 8.
 * eegldm_fir_same: zero-phase FIR over B rows of L samples, y[b][n] = sum_{k = 0..M-1} taps[k] xe[b][n + k - c], c = (M - 1) / 2, M odd in
 * 1..2049, L in 1..4096; taps is a DEVICE array of M floats.  xe is the row extended by zeros (edge 0) or by whole-sample reflection that does
 * not repeat the end sample (edge 1: xe[-i] = x[i], xe[L-1+i] = x[L-1-i]; needs c <= L - 1).  mode 1 is the RMS envelope: every sample
 * enters as x * x (one fp32 rounding) and sqrtf(max(sum, 0)) is stored; a NaN or infinite sum stays non-finite.  Every output is ONE fmaf chain in ascending k
 * from +0 over its own support: its bits do not depend on B, on the launch geometry or on where in a row the same samples sit, and a
 * non-finite sample makes non-finite exactly the outputs whose support [n - c, n + c] holds it.  ldx / ldy are row strides in floats (>= L);
 * x, taps, y need 4-byte alignment only; x == y is refused; B == 0 is a no-op.  A refusal leaves y untouched. */
int eegldm_fir_same(eegldm_ctx*, const float* x, long ldx, const float* taps, int M, float* y, long ldy, long B, int L,
                    int edge /* 0 zeros, 1 reflect */, int mode /* 0 plain, 1 rms */);
/* eegldm_threshold_events: per row, the runs of s above thr[b] after closing, with features.  All comparisons are exact fp32 comparisons.
 *  1. active[n] = s[b][n] > thr[b] (a NaN on either side and a tie are inactive);
 *  2. a maximal inactive stretch strictly between two active samples and at most merge_gap long becomes active (never one that touches a row end);
 *  3. events are the maximal runs [start, stop) of the closed set with min_len <= stop - start <= max_len, without those that touch a row end
 *     when drop_edge != 0; they are numbered by start, the first max_events (E, 1..64) are stored, the others only counted;
 *  counts [B][2] = (events kept, raw runs before closing and gating); ev_i [B][E][6] = (start, length, argmax, n_up, n_raw, flags): argmax the
 *  first index of the maximum of s over the run under `>` from s[start], n_up the number of n in [start + 1, stop) with aux[n-1] < 0 &&
 *  aux[n] >= 0, n_raw the raw runs merged, flags bit 0 / 1 = the run touches the left / right end; ev_f [B][E][4] = (peak, sum, aux_max, aux_min):
 *  sum the fp32 sum of s over the run in ascending order from +0 (a NaN inside a closed gap makes it NaN), aux_max / aux_min by `>` / `<`
 *  from aux[start].  aux == NULL: n_up, aux_max, aux_min are 0.  Unused table slots are left untouched.  L in 1..4096, lds_ / ldaux >= L.
 *  One wave per row; no atomics, no memset, one writer per element: a result repeats bit for bit. */
int eegldm_threshold_events(eegldm_ctx*, const float* s, long lds_, const float* aux, long ldaux, const float* thr, long B, int L,
                            int min_len, int max_len, int merge_gap, int drop_edge, int max_events, int* counts, int* ev_i, float* ev_f);

/* ---- preparing raw recordings (eegldm.recordings: EDF in, low-passed 100 Hz rows out; csrc/resample.hip).  Additive, ABI 8.
 * eegldm_resample_fir: zero-phase rational-rate FIR resampler over B rows of L samples, L in 1..2^30.  taps is a DEVICE array of M floats,
 * M odd in 1..16383, c = (M - 1) / 2; U in 1..64, D in 1..4096; Lout = ceil(L U / D) in 64 bits.
 *   v[i] = xe[b][i / U] where U divides i, else 0;      y[b][m] = sum_{k = 0..M-1} taps[k] v[m D + k - c],  m in [0, Lout).
 * xe is the row extended by zeros (edge 0) or by the whole-sample reflection of eegldm_fir_same (edge 1: xe[-i] = x[i], xe[L-1+i] =
 * x[L-1-i]; needs ceil(c / U) <= L - 1).  Only the taps with (m D + k - c) % U == 0 meet a sample, at most ceil(M / U) per output.  Every
 * output is ONE fmaf chain over its own terms in ascending k from +0; under edge 0 the terms outside the row are skipped, not multiplied.
 * So an output's bits do not depend on B, on the launch geometry or on where in a row the same samples sit, a non-finite sample makes
 * non-finite exactly the outputs whose terms hold it, and with U = D = 1 the result is that of eegldm_fir_same(mode 0) bit for bit.
 * xtype 0: x is fp32 rows.  xtype 1: x is int16 rows (EDF's digital samples) and gain / offset are fp32 DEVICE arrays of B values: the sample
 * that enters the chain is fmaf((float)d, gain[b], offset[b]), one fp32 rounding (gain / offset are ignored for xtype 0 and may be NULL).
 * ldx / ldy are row strides in elements (>= L, >= Lout); fp32 pointers need 4-byte alignment, an int16 x 2-byte alignment; x == y is
 * refused; B == 0 is a no-op; B times the number of output segments (Lout / 2048 or Lout / 1024 by default) beyond 65535 * 2^20 workgroups is refused.
 * No atomics, no memset, one writer per element.  Every refusal leaves y untouched. */
int eegldm_resample_fir(eegldm_ctx*, const void* x, long ldx, int xtype /* 0 fp32, 1 int16 */, const float* gain, const float* offset,
                        const float* taps, int M, int U, int D, float* y, long ldy, long B, long L, int edge /* 0 zeros, 1 reflect */);
/* eegldm_epoch_stats: for B rows of L fp32 samples (row stride ldx >= L) and epochs of E samples, E in 1..12288, only the L / E whole epochs
 * counted: out [B][L / E][4] = (min, max, mean, sd), contiguous fp32.  min / max by < / > from the epoch's first sample; the mean is a float64
 * sum over the epoch divided by E, sd the root of the float64 mean squared deviation ABOUT THAT MEAN (two passes over the epoch held on
 * chip), each rounded to fp32 once.  A NaN anywhere in the epoch makes all four NaN.  One workgroup per epoch, fixed reduction order: a result
 * repeats bit for bit.  L < E or B == 0 is a no-op; B (L / E) beyond 65535 * 2^20 is refused. */
int eegldm_epoch_stats(eegldm_ctx*, const float* x, long ldx, long B, long L, int E, float* out);

/* ---- time-frequency primitives (spectrograms, band courses and phase-amplitude coupling of eegldm.metrics; csrc/tfr.hip).  Additive, ABI 8.
 * eegldm_stft_num_frames (host only): frames of a row of L samples.  centre 0: frame f covers [f hop, f hop + n_win), F = L >= n_win ?
 * (L - n_win) / hop + 1 : 0.  centre 1: with h = n_win / 2 frame f covers [f hop - h, f hop - h + n_win), F = (L - 1) / hop + 1 (0 for L == 0).
 * Returns -1 for L < 0, n_win < 1, hop < 1 or centre outside {0, 1}.
 * eegldm_stft_power: short-time multitaper power of B rows of L fp32 samples (row stride ldx >= L floats).  n_fft in {64, 128, ..., 4096},
 * 1 <= n_win <= n_fft (the frame is zero-padded behind its n_win samples), hop >= 1, K in 1..8; tapers is a DEVICE array [K][n_win], w2_host [K]
 * the squared taper weights (finite, >= 0).  With centre 1 samples outside [0, L) are zeros (edge 0) or the whole-sample reflection of
 * eegldm_fir_same (edge 1: xe[-i] = x[i], xe[L-1+i] = x[L-1-i]; needs h <= L - 1); with centre 0 edge is ignored.
 *   v_t[n] = taper_t[n] (xe[s_f + n] - m), m the fp32 mean of the frame's n_win extended samples (detrend 1) or 0 (detrend 0);
 *   X_t[k] = sum_n v_t[n] e^{-2 pi i k n / n_fft};   P[b][f][k] = scale c_k sum_t w2[t] |X_t[k]|^2,
 *   c_k = 2 when onesided and 0 < k < n_fft / 2, else 1.  All physical normalisation is the host's (scale).
 * Outputs, both optional but not both NULL, contiguous fp32: power [B][F][k1 - k0], the bins 0 <= k0 < k1 <= n_fft / 2 + 1 (ignored when
 * power is NULL); bands [B][F][NB], NB in 1..16 host bin ranges bands_host [NB][2] = [lo, hi) with 0 <= lo < hi <= n_fft / 2 + 1, independent
 * of k0 / k1: the fp32 sum of P[b][f][k] over the range in ascending k from +0, of the same fp32 values a full call stores.  A bands-only
 * call never writes the spectrogram and equals the fold of a full call bit for bit.
 * Every sequence is transformed on its own (radix-2 in LDS, roots of unity by sincospif): a frame's bits depend only on its own n_win
 * samples, the tapers, the weights and scale; not on B, F, the frame index, the row, the other frames of its workgroup or the launch
 * geometry.  A non-finite sample makes non-finite exactly the frames whose support [s_f, s_f + n_win) holds it (reflected copies included,
 * also under a zero taper value).  No atomics, no memset, one writer per element: a result repeats bit for bit.  x, tapers, power, bands
 * need 4-byte alignment only.  F == 0 or B == 0 is a successful no-op; every refusal is made before the device is touched and leaves both
 * outputs untouched. */
long eegldm_stft_num_frames(long L, int n_win, int hop, int centre);
int eegldm_stft_power(eegldm_ctx*, const float* x, long ldx, long B, long L, const float* tapers, const float* w2_host, int K, int n_win,
                      int n_fft, int hop, int centre, int edge /* 0 zeros, 1 reflect */, int detrend, int onesided, float scale, int k0, int k1,
                      float* power, const int* bands_host, int NB, float* bands);
/* eegldm_pac_intervals: phase-amplitude sums over intervals.  pr, pi, amp are fp32 rows (B, L) with their own strides (>= L); iv is a DEVICE
 * int32 [NI][3] of (row, start, length), or NULL with NI == B for one interval per whole row.  out is a DEVICE double [NI][4] =
 * (n, sum a, sum a pr / h, sum a pi / h), h = sqrt(pr^2 + pi^2), every term in float64 from the fp32 inputs.  A sample takes part iff a, pr, pi
 * are finite and h > 0; n counts those.  An interval with a row outside [0, B), start < 0, length < 1 or start + length > L is no fault: it
 * writes (-1, 0, 0, 0).  One wave per interval: a lane's chain runs over samples start + lane, + 64, ... in ascending order from +0, a fixed
 * xor butterfly (offsets 32 .. 1) follows: an interval's bits do not depend on NI or on the other intervals.  out needs 8-byte alignment,
 * everything else 4.  The mean vector length hypot(c, s) / sum a and the preferred phase atan2(s, c) are host float64 algebra on out. */
int eegldm_pac_intervals(eegldm_ctx*, const float* pr, long ldr, const float* pi, long ldi, const float* amp, long lda, long B, long L,
                         const int* iv, long NI, double* out);

/* ---- signal-complexity primitives (Hjorth parameters, permutation entropy, sample entropy of eegldm.metrics; csrc/complexity.hip).  fp32
 * rows of L samples in 1..4096 with row stride ldx >= L floats; additive, ABI 8.  Float pointers need 4-byte alignment only, the int64 and
 * double outputs 8.  B == 0 is a no-op.  Every refusal returns its code, sets eegldm_last_error, launches nothing and leaves the outputs
 * untouched; no output has to be zeroed by the caller.  A row's result does not depend on B, on the other rows or on the launch geometry, and
 * a result repeats bit for bit: the integer results make every summation order exact, the float64 ones use a fixed order.
 * eegldm_row_moments: out [B][8] = (mean, m2_x, m2_d1, m2_d2, line_length, sign_changes, min, max), every term float64 formed from the fp32
 * samples.  d1[n] = x[n+1] - x[n], d2[n] = d1[n+1] - d1[n]; mean_v = (sum v) / count; m2_v = sum (v - mean_v)^2 about that mean, in a second pass
 * over the LDS-resident row (0 for an empty and for a finite one-element v); line_length = sum |d1|; sign_changes = #{n in [1, L) : (c[n-1] < 0)
 * != (c[n] < 0)}, c = x - mean; min / max by exact fp32 comparison, both NaN when the row holds a NaN.  A non-finite sample propagates by IEEE
 * rules into the moments it enters; other rows keep their bits.  Hjorth activity, mobility and complexity are host algebra on this table:
 * var = m2 / count, mobility = sqrt(var_d1 / var_x), complexity = sqrt(var_d2 / var_d1) / mobility. */
int eegldm_row_moments(eegldm_ctx*, const float* x, long ldx, long B, int L, double* out /* [B][8] */);
/* eegldm_ordinal_counts: ordinal-pattern histogram.  order in 2..6, delay >= 1, (order - 1) * delay < L.  For every position p in
 * [0, L - (order - 1) delay) with v_k = x[p + k delay], k < order: the pattern index is the Lehmer code sum_k c_k (order - 1 - k)!, c_k =
 * #{l > k : v_l < v_k}, by exact fp32 `<` (ties rank by position, -0 == +0); counts [B][order!] holds the positions per index.  A position
 * whose vector holds a NaN or an infinity is counted in skipped [B] and in no bin.  Permutation entropy -sum p ln p (optionally / ln(order!))
 * is host float64 algebra on the counts. */
int eegldm_ordinal_counts(eegldm_ctx*, const float* x, long ldx, long B, int L, int order, int delay, int* counts /* [B][order!] */,
                          int* skipped /* [B] */);
/* eegldm_template_matches: the pair counts of (multiscale) sample entropy.  m in 1..4, scale in 1..64, N = L / scale with N - m >= 2; r is a
 * DEVICE array [B] of tolerances.  y[j] = (x[j s] + ... + x[j s + s - 1]) / (float)s, the sum in fp32 in ascending order from +0, one IEEE
 * divide (scale 1: y compares as x; samples past N s are not read).  Templates are i in [0, N - m), the same set for both lengths (Richman
 * and Moorman 2000).  counts [B][2]:
 *   counts[b][0] = #{i < j : |y[i+k] - y[j+k]| <= r[b] for all k < m},   counts[b][1] = the same for all k <= m.
 * The test is fabsf(a - b) <= r with one fp32 rounding of the difference: anything with a NaN in y or r, and inf - inf, is no match; r = inf
 * matches every pair that produces no NaN; a negative r matches nothing.  SampEn = -ln(counts[b][1] / counts[b][0]) is host algebra. */
int eegldm_template_matches(eegldm_ctx*, const float* x, long ldx, long B, int L, int m, int scale, const float* r /* device [B] */,
                            long long* counts /* [B][2] */);

/* ---- device-resident window bank (eegldm.data; csrc/window_bank.hip).  Additive, ABI 8.  A bank is ONE flat fp32 device buffer holding every
 * recording of a loader, one channel each, row r at [row_off[r], row_off[r + 1]); rows start at any 4-byte offset and the bank may pass
 * 2^31 elements (64-bit indices).  Every refusal returns its code, sets eegldm_last_error, launches nothing and leaves the outputs untouched.
 *
 * eegldm_bank_normalise: the deterministic head of the window transform, in place, row by row -- a = x * fl32(1 + 1e6), lo = min a, hi = max a,
 * row = hi == lo ? +0 : (a - lo) / (hi - lo), every operation a separately rounded fp32 operation (no fma), so a row's bytes are those of the
 * same three numpy expressions; lohi [n_rec][2] receives (lo, hi).  A NaN in a row makes its lo, hi and every element NaN (numpy's min / max
 * keep a NaN) and touches no other row.  Only the sign of a zero minimum is unspecified (min(+0, -0)).  row_off is the DEVICE array of
 * n_rec + 1 ascending int64 offsets, row_off_host the same values in host memory (the checks and the launch shape are taken from it);
 * rows hold 1 .. 2^30 samples.  ws: 2 * (row_off[n_rec] / EEGLDM_BANK_CHUNK + n_rec + 1) floats of device workspace (contents irrelevant).
 * Three launches -- a min / max partial per fixed chunk of EEGLDM_BANK_CHUNK samples, one fold per row, the apply pass -- without atomics or
 * memsets; min and max are exact, so no value depends on the launch geometry and two runs agree bit for bit. */
#define EEGLDM_BANK_CHUNK 16384
int eegldm_bank_normalise(eegldm_ctx*, float* bank, const int64_t* row_off /* device [n_rec + 1] */, const int64_t* row_off_host, int n_rec,
                          float* lohi /* device [n_rec][2] */, float* ws, long ws_floats);
/* eegldm_window_batch: one launch crops, pads and labels a batch of B windows.  The sampling policy lives in the SEGMENT TABLE the caller
 * built (eegldm.data.segment_tables): segment j is a run of consecutive valid crop starts that share a label -- seg_first[j] the bank
 * index of its first start, seg_cum [n_seg + 1] the running count of starts (strictly ascending from 0), seg_label[j] int32 -- and a group
 * g is the contiguous segment range [group_bounds[g], group_bounds[g + 1]) (group_bounds [n_group + 1]).  All arrays are device memory.
 * Window b:  [lo, hi) = (seg_cum[group_bounds[g]], seg_cum[group_bounds[g + 1]]) for g = group[b], or (0, seg_cum[n_seg]) when group is
 * NULL;  idx = idx_in[b] when idx_in is given, else lo + v % (hi - lo) with v the 64-bit word (r0 << 32) | r1 of Philox4x32-10(key seed,
 * counter offset + b) -- lo plus what eegldm_randint(high = hi - lo, seed, offset) writes to element b;  j: seg_cum[j] <= idx <
 * seg_cum[j + 1] (binary search);  src = seg_first[j] + idx - seg_cum[j];  out[b * ld ..] = border exact +0, bank[src .. src + window),
 * border +0;  labels_out[b] = seg_label[j] and src_out[b] = src (int64, each nullable).  ld >= window + 2 border; the floats of a row past
 * window + 2 border are not written.  Nothing outside [src, src + window) is read; rows whose address is a multiple of 16 bytes are stored
 * 16 bytes at a time, others element by element, the source may have any 4-byte alignment.  One block per window: no value depends on the
 * launch geometry.  Refused: NULL bank / tables / out, group without group_bounds, window < 1, border < 0, ld too small, B < 1, n_seg < 1,
 * bank_len < window.  What only the device can see -- idx_in[b] outside [lo, hi), an empty range, a group outside [0, n_group), a src with
 * [src, src + window) outside [0, bank_len) -- gives row b = NaN (all window + 2 border floats), labels_out[b] = INT64_MIN, src_out[b] = -1,
 * reads nothing from the bank and leaves the other rows alone. */
int eegldm_window_batch(eegldm_ctx*, const float* bank, long bank_len, const int64_t* seg_first, const int64_t* seg_cum,
                        const int32_t* seg_label, long n_seg, const int64_t* group_bounds /* nullable */, int n_group,
                        const int64_t* group /* nullable [B] */, const int64_t* idx_in /* nullable [B] */, uint64_t seed, uint64_t offset,
                        int window, int border, float* out, long ld, int64_t* labels_out /* nullable */, int64_t* src_out /* nullable */, int B);

#ifdef __cplusplus
}
#endif
#endif /* EEGLDM_H */
