/* cpc_hip.h — C ABI of the MI355X-native CPC-audio train-step library (libcpc_hip.so).
 *
 * The reference (vincentherrmann/constrastive-predictive-coding-audio) is pure Python/PyTorch and has no FFI of its
 * own; the seam this library sits behind is the ATen call each reference line makes.  Every entry point below names
 * the reference statement(s) it replaces (paths relative to the reference repository root).
 *
 * Conventions
 *   - plain C: raw DEVICE pointers, sizes, a hipStream_t passed as void*; no torch types.
 *   - every call is stream-ordered and asynchronous, never allocates, never synchronises, never throws;
 *     returns 0 on success, -22 (EINVAL) for unsupported shapes/arguments, -5 (EIO) if the launch failed.
 *   - dtype: CPC_F32 (0) = exact-f32 parity mode (v_mfma_f32_16x16x4_f32), CPC_BF16 (1) = bf16 storage with f32
 *     accumulation (v_mfma_f32_16x16x32_bf16).  "T" below means that storage type.
 *   - activations are channels-last: act[item][position][channel], positions padded per item to L_alloc rows
 *     (pad rows hold zeros); see DESIGN.md "Data layout in HBM".
 */
#ifndef CPC_HIP_H
#define CPC_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define CPC_F32 0
#define CPC_BF16 1

#define CPC_GEMM_RELU 1      /* NT epilogue: relu */
#define CPC_GEMM_OUT_F32 2   /* store the result as f32 even when dtype is bf16 */
#define CPC_GEMM_TN_NO_TR 4  /* TN/bf16 only: scalar LDS reads instead of ds_read_b64_tr_b16 (A/B check) */
#define CPC_GEMM_FORCE_GENERIC 8 /* use the generic (any-shape) kernel even where the double-buffered fast path applies */
#define CPC_GEMM_NARROW_EPI 32   /* NT/bf16: per-lane 8-byte stores instead of the LDS-staged full-row epilogue (A/B check) */
#define CPC_GEMM_NO_DMA 64       /* NT fast path: register-staged global->LDS copies instead of LDS-DMA (A/B check) */
#define CPC_GEMM_SKIP_PAD_ROWS 128 /* NT: rows with (m % c_rpi) >= c_valid are left untouched instead of zeroed */
#define CPC_GEMM_LINEAR_K 256     /* NT: visit K in storage order even for overlapped-row A operands (A/B check; default for lda < K,
                                    K % lda == 0 is tap-innermost: identical sums in a different order, each input byte fetched once) */
#define CPC_GEMM_NO_PERS 512      /* NT/bf16: LDS-staged epilogue instead of the register epilogue (A/B check) */
#define CPC_GEMM_DIRECT_MASK 1024 /* NT/bf16: register epilogue also for launches with a mask (A/B check; default: LDS-staged there) */
#define CPC_GEMM_KRANGE_EXACT 2048 /* with k_ranges: the ranges cut out pieces that are NOT zero, so no tile may straddle two range indices — the
                                    * launch returns CPC_EINVAL unless a_rpi * max(a_rpi2, 1) is a multiple of the tile height (128 / 256) the
                                    * launcher picks.  Without the flag a tile runs the union of its rows' ranges (correct for known-zero cuts only). */
#define CPC_GEMM_SMALL_TILE 16   /* keep the 128x128 tile where the 256x256 one would be chosen (A/B check) */
#define CPC_GEMM_BIG_TILE 0x100000 /* NT/bf16: the 256x256 tile also where fewer than 200 of them exist (M >= 256): a launch that is ONE nearly
                                    * full round of such tiles (layer 2's target rows at the headline size: 196) runs 0.11 instead of 0.135 ms */
#define CPC_GEMM_GENERIC_EPI 0x200000 /* NT/bf16 256x256: the generic epilogue body also for the masked data-gradient launches that have a
                                       * compile-time epilogue form (A/B check: bit-identical results) */
#define CPC_GEMM_QUERY_EPI 0x800000   /* NT: launch nothing; a call that passes every argument check returns 100 + the epilogue form its launch would
                                       * run (0 generic, 1 masked data gradient with the sign-bit mask, 2 the same fused with layer 1's weight gradient, 3 masked data gradient
                                       * with the full-size mask) instead of 0.  For tests only. */

/* 9: the tuning-knob entry point (stagger, store policy, timing probes of the NT GEMM) is gone; cpc_gru_set_streaming is on / off only.
 *    Added later under 9 (backward compatible, no entry point changed): the difference scores cpc_diff_scores, cpc_diff_scores_bwd,
 *    cpc_diff_scores_rank1.
 *    Added later under 9 (backward compatible, no entry point changed): the attention core for up to 128 steps cpc_attn128_fwd,
 *    cpc_attn128_bwd, cpc_attn128_tangent, cpc_attn128_gp.
 *    Added later under 9 (backward compatible, no entry point added or changed): cpc_gru_tape_elems, cpc_gru_fwd, cpc_gru_fwd_h0,
 *    cpc_gru_bwd, cpc_gru_gp_fwd and cpc_gru_gp_bwd accept hidden sizes up to 512 (were 256).
 *    Added later under 9 (backward compatible, no entry point changed): the loss over sampled negatives
 *    cpc_nce_sampled_workspace_floats, cpc_nce_loss_sampled, cpc_nce_sample_mask.
 *    Added later under 9 (backward compatible, no entry point changed): the loss over grouped negatives
 *    cpc_nce_grouped_workspace_floats, cpc_nce_loss_grouped, cpc_nce_group_mask.
 *    Added later under 9 (backward compatible, no entry point changed): LAMB trust ratios cpc_lamb_workspace_floats, cpc_lamb.
 *    Added later under 9 (backward compatible, no entry point changed): row normalisation for the cosine-similarity scores
 *    cpc_norm_rows, cpc_norm_rows_bwd.
 *    Added later under 9 (backward compatible, no entry point changed): the exponential moving average of the weights cpc_ema,
 *    cpc_ema_swap; the temperature in device memory cpc_norm_rows_dev, cpc_norm_rows_bwd_dev, cpc_temperature_step, cpc_temperature_set.
 *    Added later under 9 (backward compatible, no entry point changed): cpc_gemm_nt_bits, cpc_gemm_nt_debug_flags.
 *    Added later under 9 (backward compatible, no entry point changed): the loss over a bank of earlier predictions
 *    cpc_nce_banked_workspace_floats, cpc_nce_loss_banked.
 *    Added later under 9 (backward compatible, no entry point changed): waveform augmentation cpc_wave_power_chunks, cpc_wave_power,
 *    cpc_wave_augment.
 *    Added later under 9 (backward compatible, one entry point added, none changed): cpc_gru_bwd_steps, the backward sweep of a GRU layer that
 *    receives a gradient at every hidden state (a lower layer of AudioGRUModel(num_layers > 1)).
 *    Added later under 9 (backward compatible, one entry point added, none changed): cpc_mel_pointwise, the log-mel front end behind the
 *    framed DFT GEMM.
 *    Added later under 9 (backward compatible, entry points added, none changed): masking augmentation on the input grid
 *    cpc_grid_sum_chunks, cpc_grid_sum, cpc_grid_mask.
 *    Added later under 9 (backward compatible, one entry point added, none changed): cpc_window_gather, the batch of a device-resident
 *    audio dataset.
 *    Added later under 9 (backward compatible, entry points added, none changed): the LSTM recurrence cpc_lstm_tape_elems, cpc_lstm_fwd,
 *    cpc_lstm_bwd (AudioLSTMModel).
 *    Added later under 9 (backward compatible, one entry point added, none changed): cpc_resample, downmix and rational resampling of
 *    audio files when a device-resident dataset is loaded.
 *    Added later under 9 (backward compatible, entry points added, none changed): prediction anchors — cpc_lstm_bwd_steps, the LSTM
 *    backward sweep with a gradient at every hidden state, and cpc_anchor_target_grad, the anchors' target-gradient windows summed
 *    into the top-layer gradient.
 *    Added later under 9 (backward compatible, entry points added, none changed): whole-recording feature extraction —
 *    cpc_stream_gather, cpc_feature_emit, cpc_stream_carry.
 * 8 (round 4): the fused all-timesteps score path (cpc_score_lse, cpc_nce_lse_merge, cpc_nce_fused_grad(_blocks), cpc_nce_fused_finalize); cpc_reduce_conv_w2d; cpc_accumulate; the row-range launches cpc_conv1_fwd_rows, cpc_conv_dgrad_rows, cpc_conv_dgrad_conv1_rows, cpc_conv1_fused_reduce_tiles.
 * 7 (round 3, second half): cpc_gemm_nt_args grew the second row level (a_rpi2 / c_rpi2), k_ranges and the gathered-row taps (k_taps,
 * k_tap_stride, k_tap_stride_a); new entry points cpc_conv_w_prep_group / _plan / _batch, cpc_bn_apply_residual, cpc_bn_bwd_reduce_res / _apply_res, cpc_stem_residual_bn_add,
 * cpc_stem_residual_wgrad_bits; cpc_gemm_tn_args grew a_rpi2 / a_item2.
 * 6: the stem kernels (cpc_stem_*), sign-bit BatchNorm passes (cpc_bn_*_bits), cpc_gru_fwd_h0.
 * 5 since the gradient-penalty entry points (cpc_gru_gp_*, cpc_ln_tangent / cpc_ln_gp, cpc_attn_tangent / cpc_attn_gp,
 * cpc_gp_score_coeff) were added; 4: per-tile column sums of the data gradients; 3: sign-bit masks; 2: over-read contract. */
int cpc_abi_version(void);

/* Row addressing used by both GEMMs: row m of an operand starts at element
 *   rpi == 0 :  m * ld
 *   rpi  > 0 :  (m / rpi) * item + (m % rpi) * ld        ("items" of rpi rows, e.g. a window of frames per clip)   */

/* C[m][n] = epi( sum_k A[m][k] * Bt[n][k] ), epi = (+bias[n]) -> (relu) -> (mask[m][n] > 0 ? . : 0) -> (pad row -> 0).
 * Replaces, in channels-last layout: F.conv1d forward of AudioEncoder layers 2..5 (audio_model.py:38-41, A rows
 * overlap: lda = stride*C_in, K = kernel*C_in), their data gradient (autograd of the same lines), nn.GRUCell's
 * input projection for all steps at once (audio_model.py:72), prediction_model (audio_model.py:208) and the
 * tensordot of the score functions restricted to equal steps (contrastive_estimation_training.py:13-14, :20-21).
 * PAD COLUMNS.  N % 4 != 0 is accepted without bias and mask only, and the rows of C must have room for round-up(N, 4) columns: every
 * kernel then stores ZEROS into columns N .. round-up(N, 4) - 1 of each row it writes; nothing beyond them is touched. */
typedef struct cpc_gemm_nt_args {
    const void* A;  const void* Bt;  void* C;
    const float* bias;            /* [N] f32 or NULL */
    const void* mask;             /* T, addressed like C, or NULL */
    int M, N, K;
    long long lda, ldb, ldc;
    int a_rpi; long long a_item;
    int b_rpi; long long b_item;
    int c_rpi; long long c_item; int c_valid;   /* rows with (m % c_rpi) >= c_valid are stored as zeros */
    long long a_batch, b_batch, c_batch; int batch;
    int flags; int dtype;
    /* OVER-READ CONTRACT.  Row m of A is read as the K elements starting at its row address, whatever lda is: with
     * overlapped rows (lda < K, the strided-convolution view) the last row therefore reads (K - lda) elements beyond the end
     * of an [M][lda] array, and rows are clamped to M - 1 but never shortened.  ALL of [A, A + last_row_offset + K) (and the
     * same for Bt) must be readable device memory: an allocation that ends exactly at M*lda elements may end at the end of a
     * mapped segment, and the over-read then faults (this happened once).  a_extent / b_extent:
     * number of elements readable from A / Bt (all batches); when > 0 the call returns CPC_EINVAL if any row would end beyond
     * it; 0 = not checked, the caller vouches. */
    long long a_extent, b_extent;
    /* Second row level and K ranges (LDS-DMA kernels, K a multiple of 64 bf16 / 32 f32 elements; CPC_EINVAL elsewhere): with
     * a_rpi2 != 0 row m of A sits at (m / (a_rpi a_rpi2)) a_item2 + ((m / a_rpi) % a_rpi2) a_item + (m % a_rpi) lda, likewise C and the
     * mask with c_rpi2 / c_item2: the rows of a grid ordered (band of rows, column, row within the band).  k_ranges: device int
     * pairs [lo, hi), hi > lo, in stages of 64 bf16 / 32 f32 elements: the part of the K axis that is not known to be zero for the
     * rows of band i = m / (a_rpi a_rpi2) (a_rpi2 == 0: of item m / a_rpi); a tile runs the union of the ranges of its rows.  The
     * extent check above does not know the second level: pass a_extent = 0 with a_rpi2.  All zero = off. */
    int a_rpi2; long long a_item2;
    int c_rpi2; long long c_item2;
    const int* k_ranges;
    /* Gathered rows (same kernels): with k_taps > 1 the K axis is k_taps pieces of k_tap_stride = K / k_taps elements (a multiple of 64 bf16 /
     * 32 f32), dense in Bt, while piece j of a row of A starts j * k_tap_stride_a elements after the row address — the window of an nn.Conv2d
     * read straight from a channels-last grid (piece = kh rows x C channels of one kernel column; k_tap_stride_a = one grid column), no
     * im2col matrix.  The over-read contract applies to every piece.  k_taps = 0: off (overlapped rows with lda < K are detected by the launcher
     * and visited tap-innermost on their own); k_tap_stride_a must be 0 then (CPC_EINVAL otherwise). */
    int k_taps; long long k_tap_stride; long long k_tap_stride_a;
} cpc_gemm_nt_args;
int cpc_gemm_nt(const cpc_gemm_nt_args* args, void* stream);
/* FOR TESTS AND A/B TIMING ONLY (this entry point and cpc_gemm_nt_debug_flags below; no production caller, not part of the supported
 * interface).  The same launch with the ReLU-backward mask as sign bits (cpc_sign_bits of the array `mask` would name; one byte per 8 elements, addressed
 * by the C element offset / 8; NULL only where args->mask is given) and, optionally, the per-tile column sums of what it stores (colsum_slabs[ceil(M / 256)][N] f32 or
 * NULL): what cpc_conv_dgrad builds, with every field of the argument block in the caller's hands.  bf16 launches that take the 256 x 256
 * tile with the LDS-staged epilogue only (N % 256 == 0, ldc % 32 == 0, c_item % 32 == 0); CPC_EINVAL otherwise. */
int cpc_gemm_nt_bits(const cpc_gemm_nt_args* args, const void* mask_bits, float* colsum_slabs, void* stream);
/* Tests and A/B timing only: flags OR-ed into every NT launch of the process from now on, whichever entry point builds it: CPC_GEMM_GENERIC_EPI,
 * CPC_GEMM_QUERY_EPI or 0; returns the previous value, -1 for anything else.  Not for use while another thread launches. */
int cpc_gemm_nt_debug_flags(int flags);

/* C[i][j] = sum_m A[m][i] * B[m][j]  (reduction over the row index of both operands), optionally split over m into
 * nsplit f32 slabs C + s*slab_stride that cpc_reduce_slabs sums deterministically.
 * Replaces the weight gradients autograd computes for conv1d / GRUCell / Linear (loss.backward(),
 * contrastive_estimation_training.py:161) and the two score-gradient contractions. */
typedef struct cpc_gemm_tn_args {
    const void* A;  const void* B;  void* C;
    int M, I, J;
    long long lda, ldb, ldc;
    int a_rpi; long long a_item;
    int b_rpi; long long b_item;
    long long a_batch, b_batch, c_batch; int batch;
    int nsplit; int m_chunk; long long slab_stride;
    int flags; int dtype;
    int c_rpi; long long c_item;          /* output row i at the item address (nsplit == 1 only); 0 = plain i*ldc */
    /* second row level of A (bf16 LDS-DMA kernel; CPC_EINVAL elsewhere): row m at (m / (a_rpi a_rpi2)) a_item2 + ((m / a_rpi) % a_rpi2) a_item
     * + (m % a_rpi) lda — with a_batch stepping over the kernel columns, the windows of a strided nn.Conv2d read straight from a channels-last grid
     * (rows = clip, output column, output row): the weight gradient without an im2col matrix.  0 = one level. */
    int a_rpi2; long long a_item2;
} cpc_gemm_tn_args;
int cpc_gemm_tn(const cpc_gemm_tn_args* args, void* stream);

/* out[j*s_j + (i / cdiv)*s_hi + (i % cdiv)*s_lo] = sum_z slabs[z*slab_stride + i*J + j]  (f32; fixed summation order). */
int cpc_reduce_slabs(const float* slabs, float* out, int I, int J, int nslab, long long slab_stride, int cdiv,
                     long long s_j, long long s_hi, long long s_lo, void* stream);

/* Conv weight gradient slabs (cpc_conv_wgrad) -> reference layout: out[co][c][j] = sum_z slabs[z][j*cin + c][co]. */
int cpc_reduce_conv_w(const float* slabs, float* out, int cin, int cout, int kw, int nslab, long long slab_stride,
                      void* stream);

/* Weight gradient of an nn.Conv2d in the reference's [cout][cin][kh][kw] layout from split-K slabs of the grid GEMMs (ABI 8):
 *   out[((co cin + c) kh + dh) kw + dw] = sum_z sum_{g < G} slabs[z slab_stride + dw s_dw + (dh + g) s_dh + c s_c + g s_g + co]
 * G = 1: slabs [kw][kh][cin][cout] (windows gathered from the grid, one GEMM batch entry per kernel column); G > 1: the row-grouped tall (k,1)
 * kernels, slab [(r, c)][(g, co)], whose G diagonals r = dh + g make up dW (scalogram_model.py:392-417's nn.Conv2d autograd). */
int cpc_reduce_conv_w2d(const float* slabs, float* out, int nslab, long long slab_stride, int cout, int cin, int kh, int kw, long long s_dw,
                        long long s_dh, long long s_c, int G, long long s_g, void* stream);

/* slabs[blk][n] = partial column sums of X[M][N] (T) — bias gradients; reduce with cpc_reduce_slabs(I=1). */
int cpc_colsum(const void* X, float* slabs, int M, int N, long long ldx, int nblocks, int dtype, void* stream);

/* AudioEncoder layer 1 (C_in = 1): y[b][t][co] = act(bias[co] + sum_j x[b][t*stride+j] * w[co][j]), act = relu when
 * relu != 0 (audio_model.py:38-41 for l == 0: the last layer of the stack has no activation, so a one-layer encoder passes
 * relu = 0).  x: f32 [B][ldx]; w: f32 [C][kw] (reference layout); y: T [B][L_alloc][C]. */
/* y_bits (may be NULL; C = 512 only, 16-byte aligned): the sign-bit mask of y, see cpc_sign_bits — written from the f32 values
 * before they are rounded to the storage type (what the reference's ReLU mask is taken from). */
int cpc_conv1_fwd(const float* x, const float* w, const float* bias, void* y, int B, int C, int stride, int kw,
                  long long ldx, int L_valid, int L_alloc, int relu, int dtype, void* y_bits, void* stream);
/* The same for positions [row_lo, row_hi) of every item only (0 <= row_lo < row_hi <= L_alloc; ABI 8): the train step computes the rows
 * the context network needs first and the rows only the targets need beside the GRU recurrence (engine.CPCEngine.encoder_forward). */
int cpc_conv1_fwd_rows(const float* x, const float* w, const float* bias, void* y, int B, int C, int stride, int kw, long long ldx,
                       int L_valid, int L_alloc, int relu, int dtype, void* y_bits, int row_lo, int row_hi, void* stream);
/* SIGN-BIT MASKS: bits[i] bit e = x[8 i + e] > 0 (for bf16: of the stored value), n elements (a multiple of 32; x 16-byte, bits
 * 4-byte aligned).  The ReLU-backward mask of a data gradient at 1/16 of the bytes of the activation it is taken from:
 * cpc_conv_dgrad / cpc_conv_dgrad_conv1 take it as x_act_bits in place of x_act — the same decision per element, identical
 * results — addressed by the element offset / 8, so a bits buffer mirrors its activation buffer (guard rows included). */
int cpc_sign_bits(const void* x, void* bits, long long n, int dtype, void* stream);
/* Weight/bias gradient of layer 1: slabs[nblk_b*nblk_t][(kw+1)][C] partials (row kw = bias); reduce with
 * cpc_reduce_slabs.  nblk_t blocks split the positions, nblk_b (<= B) blocks stride over the items. */
int cpc_conv1_bwd(const float* x, const void* dy, float* slabs, int B, int C, int stride, int kw, long long ldx,
                  int L_valid, int L_alloc, int nblk_t, int nblk_b, int dtype, void* stream);

/* Data gradient of encoder layer 2 FUSED with the weight/bias gradient of layer 1 (audio_model.py:38-39 differentiated, l = 1
 * and l = 0): the masked gradient tile of layer 1's output never goes to memory; each 256 x 256 tile leaves
 * slabs[tile][j][c] = sum_rows G[row][c] * x[b][t*stride1 + j] (j < kw1) and [kw1][c] = sum_rows G[row][c].
 * bf16 only, Cin % 256 == 0, kw1 <= 15; CPC_EINVAL otherwise (callers then use cpc_conv_dgrad + cpc_conv1_bwd).
 * x: f32 waveform (first sample the encoder reads), ldx samples per item.  Sizes of slabs / tmp (floats):
 * cpc_conv_dgrad_conv1_floats(..., what = 0 / 1).  cpc_conv1_fused_reduce sums the slabs in a fixed order into
 * dw [Cin][1][kw1] (reference layout) and db [Cin] (may be NULL). */
long long cpc_conv_dgrad_conv1_floats(int B, int Cin, int stride, int Lout_alloc, int kw1, int what);
int cpc_conv_dgrad_conv1(const void* dy, const void* w_dgrad, const void* x_act, const float* x, float* slabs, int B, int Cin,
                         int Cout, int kw, int stride, int Lout_alloc, long long ldx, int kw1, int stride1, int L1_valid,
                         long long dy_head, int dtype, const void* x_act_bits, void* stream);
int cpc_conv1_fused_reduce(const float* slabs, float* tmp, float* dw, float* db, int B, int Cin, int stride, int Lout_alloc,
                           int kw1, void* stream);

/* Conv1d (layers >= 2) in channels-last layout, expressed through the GEMMs above.
 *   fwd  : y[(b,t)][co] = relu?(bias + sum_{j,c} x[(b, t*stride + j)][c] * w[co][c][j])       audio_model.py:38-41
 *   dgrad: dx[(b,p)][c]  = (x_act > 0 ?) sum_{t,co: t*stride + j = p} dy[(b,t)][co] * w[co][c][j]
 *   wgrad: slabs of dw[(j,c)][co] = sum_{b,t} x[(b, t*stride+j)][c] * dy[(b,t)][co]
 * w_fwd / w_dgrad are the operand layouts cpc_conv_w_prep produces (either output pointer may be NULL: that layout is then
 * not written).  Lout_alloc * stride == Lin_alloc is required.
 * GUARD CONTRACT (the over-read contract of cpc_gemm_nt_args for these views): the forward and the weight gradient read
 * max(0, kw - stride) * Cin elements BEYOND the B * Lin_alloc * Cin elements of x (the window of the last row); the data
 * gradient reads (ceil(kw / stride) - 1) * Cout elements BEFORE dy.  The caller states how many elements are readable there
 * (x_tail after the end of x, dy_head in front of dy; zeros expected in dy_head, values in x_tail only ever meet pad rows);
 * CPC_EINVAL when that is less than the call needs.
 * The data gradient also requires every item of dy to END in at least D - 1 = ceil(kw / stride) - 1 zero pad rows (Lout_alloc >=
 * Lout_valid + D - 1): row 0 of item b reads the last D - 1 rows of item b - 1 as its preceding rows, exactly as row 0 of item 0 reads
 * dy_head.  Lin_valid is not used to zero anything: dx is zero beyond it, and at valid positions no window covers, only because those
 * pad rows (and dy_head) are zero.
 * x_act_bits: the sign-bit mask cpc_sign_bits makes of x_act (NULL: the mask is read from x_act).  Only the bf16 256 x 256-tile
 * kernel knows the format (>= 200 such tiles, stride * Cin a multiple of 256): CPC_EINVAL where the launch would take another
 * kernel, never a silent fall-back.  With x_act_bits, x_act may be NULL. */
int cpc_conv_fwd(const void* x, const void* w_fwd, const float* bias, void* y, int B, int Cin, int Cout, int kw,
                 int stride, int Lout_alloc, int Lout_valid, int relu, long long x_tail, int dtype, void* stream);
/* dx_colsum_slabs (may be NULL): f32 [ceil(B * Lout_alloc / 256)][stride * Cin] = per 256-row tile of the launch the column sums
 * of the dx it stores (cpc_conv_dgrad_colsum_floats floats); read as [tiles * stride][Cin] and summed by cpc_reduce_slabs this is the
 * bias gradient of the layer below — d loss / d bias = sum over (b, t) of dx — without another pass over dx.  bf16, 256 x 256-tile
 * kernel with a mask only (as x_act_bits: CPC_EINVAL elsewhere). */
long long cpc_conv_dgrad_colsum_floats(int B, int Cin, int stride, int Lout_alloc);
int cpc_conv_dgrad(const void* dy, const void* w_dgrad, const void* x_act, void* dx, int B, int Cin, int Cout, int kw,
                   int stride, int Lout_alloc, int Lin_valid, long long dy_head, int dtype, const void* x_act_bits,
                   float* dx_colsum_slabs, void* stream);
int cpc_conv_wgrad(const void* x, const void* dy, float* slabs, int B, int Cin, int Cout, int kw, int stride,
                   int Lout_alloc, int nsplit, long long x_tail, int dtype, void* stream);

/* The data-gradient launches above on rows [row_lo, row_hi) of every item only (ABI 8).  A data-gradient row q produces the input positions
 * q stride .. q stride + stride - 1 from the output-gradient rows q - D + 1 .. q (D = ceil(kw / stride)).  With kw = 2 stride the rows
 * [n_l + 1, L_alloc) of a data gradient need output-gradient rows >= n_l only: the part of the backward pass behind the TARGET frames runs
 * beside the GRU's backward recurrence (engine.CPCEngine._bwd_lane), the rest afterwards.  dx_colsum_slabs / the fused launch's slabs are
 * indexed by the launch's own 256-row tiles (ceil(B rows / 256) of them: pass an offset pointer to a second launch;
 * cpc_conv1_fused_reduce_tiles sums num_row_tiles of them). */
int cpc_conv_dgrad_rows(const void* dy, const void* w_dgrad, const void* x_act, void* dx, int B, int Cin, int Cout, int kw, int stride,
                        int Lout_alloc, long long dy_head, int dtype, const void* x_act_bits, float* dx_colsum_slabs, int row_lo, int row_hi,
                        void* stream);
int cpc_conv_dgrad_conv1_rows(const void* dy, const void* w_dgrad, const void* x_act, const float* x, float* slabs, int B, int Cin,
                              int Cout, int kw, int stride, int Lout_alloc, long long ldx, int kw1, int stride1, int L1_valid,
                              long long dy_head, int dtype, const void* x_act_bits, int row_lo, int row_hi, void* stream);
int cpc_conv1_fused_reduce_tiles(const float* slabs, float* tmp, float* dw, float* db, int num_row_tiles, int Cin, int stride, int kw1,
                                 void* stream);
int cpc_conv_w_prep(const float* w, void* w_fwd, void* w_dgrad, int Cout, int Cin, int kw, int stride, int dtype,
                    void* stream);
/* cpc_conv_w_prep for a LIST of convolutions in one launch (a context network's eleven 5 x 512 x 512 kernels: eleven launches of 20 us in
 * front of every step otherwise).  The caller fills w / w_fwd / w_dgrad (either output may be NULL) / Cout / Cin / kw / stride of every job in
 * HOST memory; cpc_conv_w_prep_plan fills the launch geometry (D, tco, gx, first) and returns the grid size and dynamic LDS bytes; the table is
 * then copied to device memory once (the operand addresses are stable) and cpc_conv_w_prep_batch launched with it whenever the weights changed. */
typedef struct cpc_conv_prep_job {
    const float* w; void* w_fwd; void* w_dgrad;
    int Cout, Cin, kw, stride;
    int D, tco, gx, first;        /* filled by cpc_conv_w_prep_plan */
} cpc_conv_prep_job;
int cpc_conv_w_prep_plan(cpc_conv_prep_job* jobs, int njobs, int* total_blocks, int* lds_bytes);
int cpc_conv_w_prep_batch(const cpc_conv_prep_job* jobs_dev, int njobs, int total_blocks, int lds_bytes, int dtype, void* stream);
/* Operands of a tall (kh,1) nn.Conv2d (scalogram_model.py:393-412, the (64,1) / (30,1) / (15,1) second kernels of the residual blocks)
 * when G output rows are computed per GEMM row (C_out < 256: G = 256 / C_out rows side by side fill the 256-wide tile): G shifted copies
 * of the kernel in a window of Rw / Rd >= kh + G - 1 rows, zeros elsewhere.  w f32 [Cout][Cin][kh] (reference layout);
 *   w_fwd  T [G][Cout][Rw][Cin]: [dh][co][r][c] = w[co][c][r - dh];     w_dgrad T [G][Cin][Rd][Cout]: [dr][c][q][co] = w[co][c][kh-1-(q-dr)];
 *   bias_g f32 [G][Cout] = bias repeated (bias, bias_g may both be NULL). */
int cpc_conv_w_prep_group(const float* w, const float* bias, void* w_fwd, void* w_dgrad, float* bias_g, int Cout, int Cin, int kh, int G,
                          int Rw, int Rd, int dtype, void* stream);

/* ConvolutionalArBlock's MaxPool1d(pool, ceil_mode=True) over positions (audio_model.py:98-99) on channels-last
 * activations [B][L_alloc][C], forward and backward (gradient to the first maximal element of each window). */
int cpc_maxpool_fwd(const void* in, void* out, int B, int C, int pool, int Lin_valid, int Lin_alloc, int Lout_valid,
                    int Lout_alloc, int dtype, void* stream);
int cpc_maxpool_bwd(const void* in, const void* dout, void* din, int B, int C, int pool, int Lin_valid, int Lin_alloc,
                    int Lout_alloc, int dtype, void* stream);
/* dy[b*item_stride + row_off + c] = y[...] > 0 ? dc[b][c] : 0 — the gradient entering the last ReLU of
 * ConvolutionalArModel at the single position its forward returns (audio_model.py:161). */
int cpc_relu_row_bwd(const float* dc, const void* y, void* dy, int B, int C, long long item_stride, long long row_off,
                     int dtype, void* stream);

/* ---- AttentionModel as the context network (attention_model.py:38-82; layers: transformer.py:223-272) ----
 * Everything works on channels-last rows x[(b,t)][C], t < S.  The linear maps are cpc_gemm_nt / cpc_gemm_tn calls.
 *
 * PositionalEncoder.forward (attention_model.py:28-35): x0[(b,t)] = top[b*item_stride + t*C ...] * scale + pe[t]
 * (pe f32 [S][C]); its backward writes scale * (g1 + g2) (g2 may be NULL) into the same rows of dtop. */
int cpc_pe_scale_fwd(const void* top, const float* pe, void* x0, int B, int S, int C, long long item_stride, float scale,
                     int dtype, void* stream);
int cpc_pe_scale_bwd(const void* g1, const void* g2, void* dtop, int B, int S, int C, long long item_stride, float scale,
                     int dtype, void* stream);
/* Dropout (transformer.py:243-252 modules, active in train mode): every mask is a pure function of (seed, site, element
 * index) — factor 1/(1-p) where a 64-bit mix of the three is >= p*2^32, else 0 — so the backward entry points regenerate
 * it from the same (drop_p, seed, site) instead of reading a stored mask.  drop_p = 0 disables it.  The reference draws
 * its masks from torch's generator stream; only the distribution can be shared, so dropout parity is statistical.
 * cpc_dropout: x[i] *= factor(i) in place (the feed-forward dropout);  cpc_dropout_mask: mask[i] = factor(i) as f32. */
int cpc_dropout(void* x, long long n, float drop_p, unsigned long long seed, unsigned site, int dtype, void* stream);
int cpc_dropout_mask(float* mask, long long n, float drop_p, unsigned long long seed, unsigned site, void* stream);
/* nn.MultiheadAttention core with the causal mask of attention_model.py:61-63, one (item, head) per workgroup:
 *   qkv T [(b,t)][3C] (q | k | v, head h at columns h*C/heads);  out T [(b,t)][C];  P T [B*heads][S][S] softmax rows (saved,
 *   before dropout; element index of the dropout mask = its offset in P).
 * Limits: S <= 64, C/heads <= 64 (-EINVAL otherwise).  The backward gives dqkv in the layout of qkv.
 * bf16 with C/heads == 64 (the reference's attention architectures) runs on the matrix pipe: scores, P V, dP, dq, dk, dv as 16x16x32
 * MFMAs with P / ds rounded to bf16 for the second products; other head sizes and f32 use vector kernels (f32 accumulation throughout). */
int cpc_attn_fwd(const void* qkv, void* out, void* P, int B, int S, int C, int heads, float drop_p, unsigned long long seed,
                 unsigned site, int dtype, void* stream);
int cpc_attn_bwd(const void* qkv, const void* P, const void* dout, void* dqkv, int B, int S, int C, int heads, float drop_p,
                 unsigned long long seed, unsigned site, int dtype, void* stream);
/* The same core for longer sequences (AudioPredictiveCodingModel's default visible_steps = 100; the reference's PositionalEncoder
 * max_seq_len = 128, attention_model.py:9-27): same layouts, P and dropout element index as cpc_attn_fwd / cpc_attn_bwd.
 * Limits: 1 <= S <= 128, C/heads <= 64 (-EINVAL otherwise).  bf16 with C/heads == 64 on the matrix pipe (one 8-wave workgroup per
 * (item, head), a 16-row query band per wave; key tiles above a band's diagonal are skipped); f32 and other head sizes on vector
 * kernels that keep the S x S matrices as packed lower triangles in LDS. */
int cpc_attn128_fwd(const void* qkv, void* out, void* P, int B, int S, int C, int heads, float drop_p, unsigned long long seed,
                    unsigned site, int dtype, void* stream);
int cpc_attn128_bwd(const void* qkv, const void* P, const void* dout, void* dqkv, int B, int S, int C, int heads, float drop_p,
                    unsigned long long seed, unsigned site, int dtype, void* stream);
/* r = a + dropout(b) (b may be NULL; r_out may be NULL), y = LayerNorm(r) * w + bias (transformer.py:262-271, eps inside
 * the sqrt); stats f32 [M][2] = (mean, rstd) saved for the backward; dropout element index = m*C + c.
 * Any C % 4 == 0 (rows of C <= 1024 stay in registers, wider rows are read three times) — wider than cpc_ln_bwd below, which stops at
 * C = 1024: a forward at C > 1024 has no backward here. */
int cpc_add_ln_fwd(const void* a, const void* b, const float* w, const float* bias, void* r_out, void* y, float* stats, int M,
                   int C, float eps, float drop_p, unsigned long long seed, unsigned site, int dtype, void* stream);
/* LayerNorm backward: dy = g1 * gscale (+ g2); with bcast > 0 row m reads g1 row m / bcast (the mean over time of
 * attention_model.py:79 folded in, gscale = 1/S).  dr = gradient of r; dr_b (may be NULL) = dr * dropout factor = gradient of
 * the summand b; slabs f32 [nblocks][2][C] hold per-block partial sums of (dw, dbias), to be summed by cpc_reduce_slabs.
 * C % 4 == 0 and C <= 1024 (a lane keeps at most four column groups; C*32 bytes of LDS): -EINVAL above, with nothing written, although
 * cpc_add_ln_fwd accepts such rows.  Blocks beyond ceil(M/4) write zero slabs. */
int cpc_ln_bwd(const void* g1, const void* g2, const void* r, const float* stats, const float* w, void* dr, float* slabs, int M,
               int C, int bcast, float gscale, int nblocks, void* dr_b, float drop_p, unsigned long long seed, unsigned site,
               int dtype, void* stream);
/* The Wasserstein gradient penalty through AttentionModel (contrastive_estimation_training.py:144-158: loss.backward() through
 * torch.autograd.grad(..., create_graph=True), here for attention_model.py:72-82 / transformer.py:262-271).  f32 only.  "Tangent":
 * the directional derivative along the penalty's direction; "delta": the adjoint of the SUMMED SCORES (pass 1 of DESIGN.md section 8).
 * cpc_ln_tangent: rt = at + dropout(bt) (bt, rt_out may be NULL), yt = w * rstd * (rt - <rt> - xh <xh rt>), xh = (r - mean) * rstd with
 *   (mean, rstd) = stats of the primal cpc_add_ln_fwd.
 * cpc_ln_gp: the second-order terms of LayerNorm.  dy = g1 * gscale (+ g2) is delta at the output (bcast as in cpc_ln_bwd), rt the
 *   tangent of the input: dr += -rstd^2 (xh <p P rt> + <xh rt> P p + <p xh> P rt), p = dy * w, P u = u - <u> - xh <xh u> (what the
 *   input's adjoint of the LAST pass gains; dr_b, may be NULL, gains the same times the dropout factor); slabs f32 [nblocks][C] hold
 *   per-block partial sums of the penalty part of the weight gradient, sum dy * rstd * P rt.  C <= 1024.
 * cpc_attn_tangent: out_t = (pt m) v + (P m) vt, pt = P (u - <P,u>), u = scale (qt k^T + q kt^T), m the dropout factors; qkvt in
 *   the layout of qkv.
 * cpc_attn_gp: dqkv += the second-order terms of the attention core, dout = delta at its output (formulas in csrc/attn.hip).
 * Preconditions, each refused with CPC_EINVAL before any launch unless stated as the caller's duty
 * (tests/test_penalty_reference_host.py pins the refusals without a GPU, tests/test_penalty_kernels_gpu.py that nothing is written):
 *   cpc_ln_tangent  at, r, stats, w, yt not NULL (bt and rt_out may be NULL: no second summand / rt not stored); M >= 1; C >= 1 with
 *                   no upper limit and no multiple required (one wave per row, lanes stride over the columns); 0 <= drop_p < 1.
 *   cpc_ln_gp       g1, rt, r, stats, w, dr, slabs not NULL (g2 and dr_b may be NULL); M >= 1; 1 <= C <= 1024 (cpc_ln_tangent
 *                   accepts wider rows, this entry point does not); nblocks >= 1; 0 <= drop_p < 1.  dr and dr_b ACCUMULATE (+=);
 *                   every one of the nblocks slabs is written, blocks beyond ceil(M/4) write zeros.  bcast > 0 must divide M and
 *                   g1 must hold M / bcast rows (caller's duty).
 *   cpc_attn_tangent / cpc_attn_gp (and the cpc_attn128 pair)
 *                   every pointer not NULL; B >= 1; 1 <= S <= 64 (128 for cpc_attn128_*); heads >= 1 dividing C; head size C / heads a
 *                   multiple of 4 and <= 64; 0 <= drop_p < 1.  qkv, qkvt, dout, dqkv and out_t are read and written as 16-byte
 *                   vectors: each must be 16-byte aligned (caller's duty; with the head size a multiple of 4 every row and head
 *                   offset then is).  P is the f32 weights cpc_attn_fwd / cpc_attn128_fwd saved, [B * heads][S][S].  dqkv ACCUMULATES.
 *                   The dropout factor of weight (bh, i, j) has element index bh S S + i S + j in both families. */
int cpc_ln_tangent(const float* at, const float* bt, const float* r, const float* stats, const float* w, float* rt_out, float* yt,
                   int M, int C, float drop_p, unsigned long long seed, unsigned site, void* stream);
int cpc_ln_gp(const float* g1, const float* g2, const float* rt, const float* r, const float* stats, const float* w, float* dr,
              float* dr_b, float* slabs, int M, int C, int bcast, float gscale, int nblocks, float drop_p, unsigned long long seed,
              unsigned site, void* stream);
int cpc_attn_tangent(const float* qkv, const float* qkvt, const float* P, float* out_t, int B, int S, int C, int heads, float drop_p,
                     unsigned long long seed, unsigned site, void* stream);
int cpc_attn_gp(const float* qkv, const float* qkvt, const float* P, const float* dout, float* dqkv, int B, int S, int C, int heads,
                float drop_p, unsigned long long seed, unsigned site, void* stream);
/* cpc_attn128_tangent / cpc_attn128_gp: cpc_attn_tangent / cpc_attn_gp for 1 <= S <= 128 (limits as cpc_attn128_fwd). */
int cpc_attn128_tangent(const float* qkv, const float* qkvt, const float* P, float* out_t, int B, int S, int C, int heads, float drop_p,
                        unsigned long long seed, unsigned site, void* stream);
int cpc_attn128_gp(const float* qkv, const float* qkvt, const float* P, const float* dout, float* dqkv, int B, int S, int C, int heads,
                   float drop_p, unsigned long long seed, unsigned site, void* stream);
/* out[b][c] = mean_t x[(b,t)][c]  (attention_model.py:79) */
int cpc_mean_time(const void* x, void* out, int B, int S, int C, int dtype, void* stream);

/* ---- scalogram front end (constant_q_transform.py, scalogram_model.py:34-102) ----
 * CQT.forward (constant_q_transform.py:161-172) is one f32 cpc_gemm_nt per octave group over overlapped waveform rows
 * (lda = hop) into cq f32 [B][Tn][ldq] with (re, im) interleaved per bin.  This call is the rest of
 * PreprocessingModule.forward: |z|^2 -> log(. + offset) + log_offset, and with phase != 0 the wrapped phase advance
 * (atan2 difference along time + fixed_pd[bin], single wrap into (-pi, pi], * pd_scale[bin]); then * norm and ** power.
 * out f32 channels-last [B][W/pw][bins/ph][Cc]: phase: W = Tn-1, Cc = 2 (amp of frame w+1, phase difference); else W = Tn,
 * Cc = 1.  ph, pw: F.max_pool2d(x, [ph, pw]) of scalogram_model.py:90-91 (floor mode), taken before the scaling; 1, 1 = none. */
int cpc_scalogram_pointwise(const float* cq, const float* fixed_pd, const float* pd_scale, float* out, int B, int Tn, int bins,
                            long long ldq, int phase, float offset, float log_offset, float norm, float power, int ph, int pw,
                            void* stream);

/* ---- 2-D residual encoder on channels-last "grids" (ScalogramEncoderBlock / ScalogramResidualEncoder,
 * scalogram_model.py:372-529) ----
 * A grid is described by int[6] = {B, W, H, Ha, top, C}: element (b, w, h, c) at ((b*W + w)*Ha + top + h)*C + c, with
 * h the frequency axis, w the time axis; Ha >= top + H rows are allocated per (b, w) column and rows outside
 * [top, top+H) are zero (ZeroPad2d top padding, scalogram_model.py:388-389, is a non-zero `top`).
 * Convolutions: tall (k,1) stride-1 kernels are cpc_gemm_nt / cpc_gemm_tn over overlapped rows of a grid; every other
 * kernel shape goes through cpc_im2col2d + plain GEMMs + cpc_col2im2d.
 *
 * col T [B*Wo*Ho][Kp], column (dh*kw + dw)*C + c = in(b, wo*sw + dw - pw, ho*sh + dh - ph, c) (zero outside the grid and
 * for columns >= kh*kw*C); in_f32: the input grid is f32 (the scalogram itself), else T. */
int cpc_im2col2d(const void* in, void* col, const int* grid, int kh, int kw, int sh, int sw, int ph, int pw, int Ho, int Wo, int Kp,
                 int in_f32, int dtype, void* stream);
/* The adjoint: din(b,w,h,c) (+= if accumulate) sum of the dcol entries that read it. */
int cpc_col2im2d(const void* dcol, void* din, const int* grid, int kh, int kw, int sh, int sw, int ph, int pw, int Ho, int Wo, int Kp,
                 int accumulate, int dtype, void* stream);
/* Depthwise (groups = channels) convolution of Conv2dSeparable (scalogram_model.py:532-544) on the im2col matrix of its input
 * (cpc_im2col2d: tap t of channel c of output row m at col[m][t*C + c]); w f32 [C][taps] is the reference's [C][1][kh][kw].
 * Output / gradient rows m live at (m / rpi) * item + (m % rpi) * C (rpi == 0: m * C), i.e. inside a grid.
 *   cpc_dw_fwd     : y[m][c] = sum_t col[m][t*C + c] * w[c][t]
 *   cpc_dw_bwd_col : dcol[m][t*C + c] = dy[m][c] * w[c][t]      (cpc_col2im2d then gives the input gradient)
 *   cpc_dw_bwd_w   : slabs[blk][c][t] = partial sums over rows of col[m][t*C + c] * dy[m][c]  (reduce with cpc_reduce_slabs) */
int cpc_dw_fwd(const void* col, const float* w, void* y, long long M, int C, int taps, int Kp, int rpi, long long item, int dtype,
               void* stream);
int cpc_dw_bwd_col(const void* dy, const float* w, void* dcol, long long M, int C, int taps, int Kp, int rpi, long long item, int dtype,
                   void* stream);
int cpc_dw_bwd_w(const void* col, const void* dy, float* slabs, long long M, int C, int taps, int Kp, int rpi, long long item,
                 int nblocks, int dtype, void* stream);
/* nn.BatchNorm2d / BatchNorm1d with batch statistics (scalogram_model.py:398-399, audio_model.py:102-103):
 * cpc_bn_stats: slabs f32 [nblocks][2][C] partial (sum, sum of squares) over the rows of x T [rows][C] (pad rows are zero);
 * cpc_bn_finalize: stats f32 [2][C] = (mean, 1/sqrt(biased var + eps)) over `count` elements per channel, and, when
 *   run_mean / run_var are given, torch's running update (momentum, unbiased variance);
 * cpc_bn_apply: out = act((x - mean) * rstd * gamma + beta) on the valid rows of two grids of equal shape. C a multiple of 4, at most 1024.
 * x_f32 (here and in the backward): x / dx are float32 grids although dtype is bf16 — the first convolution of the
 * encoder reads the float32 scalogram and keeps its pre-normalisation output in float32 (log-amplitudes have a large
 * common offset that bf16 storage would quantise away before the normalisation removes it). */
int cpc_bn_stats(const void* x, float* slabs, long long rows, int C, int nblocks, int dtype, void* stream);
int cpc_bn_finalize(const float* slabs, int nslab, int C, double count, float eps, float momentum, float* stats, float* run_mean,
                    float* run_var, void* stream);
/* cpc_bn_apply_residual (bf16, C a multiple of 8): out = act_out(act_in(BatchNorm(x)) + res(w + ow, h + oh)) — the block's second BatchNorm + ReLU,
 * the cropped residual add (scalogram_model.py:447-472) and the ReLU between blocks (:525-526) in one pass; the normalised branch is not stored,
 * only its sign bits (bits, may be NULL; addressed by the element offsets of the activation grid ga it stands for, as cpc_bn_apply_bits writes them)
 * for the BatchNorm's backward pass; obits (may be NULL): the sign bits of out, addressed like out, for cpc_bn_bwd_*_res.  Same results as cpc_bn_apply followed
 * by cpc_residual_add, bit for bit.  r_f32: res is a float32 grid. */
int cpc_bn_apply_residual(const void* x, const int* gx, const void* res, const int* gr, void* out, const int* go, const float* stats,
                          const float* gamma, const float* beta, int oh, int ow, int relu_in, int relu_out, int r_f32, unsigned char* bits,
                          const int* ga, unsigned char* obits, int dtype, void* stream);
/* ... and its backward: the cropped residual add's backward (scalogram_model.py:462-472 under autograd) folded into the second BatchNorm's two
 * backward passes.  dout: gradient of the block output on grid gd; obits (may be NULL: no ReLU behind the add): sign bits of the block output,
 * written by cpc_bn_apply_residual, addressed like dout; abits: sign bits of the normalised branch addressed like its activation grid ga.
 * g = dout [out > 0] [bn_out > 0].  cpc_bn_bwd_reduce_res: slabs as cpc_bn_bwd_reduce.  cpc_bn_bwd_apply_res: dx as cpc_bn_bwd_apply, and
 * dres (may be NULL) = dout [out > 0] at (w + ow, h + oh) of grid gr: the residual operand's gradient.  Neither the masked gradient of the main
 * branch nor a separate residual-add backward pass exists.  bf16, C a multiple of 8. */
int cpc_bn_bwd_reduce_res(const void* dout, const int* gd, const unsigned char* obits, const unsigned char* abits, const int* ga, const void* x,
                          const int* gx, const float* stats, float* slabs, int nblocks, int dtype, void* stream);
int cpc_bn_bwd_apply_res(const void* dout, const int* gd, const unsigned char* obits, const unsigned char* abits, const int* ga, const void* x,
                         void* dx, const int* gx, const float* stats, const float* gamma, const float* dgamma, const float* dbeta, double count,
                         int train, void* dres, const int* gr, int oh, int ow, int dtype, void* stream);
int cpc_bn_apply(const void* x, const int* gx, void* out, const int* go, const float* stats, const float* gamma, const float* beta,
                 int relu, int x_f32, int dtype, void* stream);
/* Backward: g = dy * (y > 0) if relu.  cpc_bn_bwd_reduce: slabs [nblocks][2][C] partials of (sum g*xhat, sum g) = (dgamma,
 * dbeta) to be summed by cpc_reduce_slabs; cpc_bn_bwd_apply: dx = gamma*rstd*(g - dbeta/count - xhat*dgamma/count) with
 * train != 0, g*gamma*rstd otherwise (running statistics).  With relu = 0 the activation is not read: both calls accept y = NULL
 * (the tangent pass of the gradient penalty calls them so); with relu != 0 a NULL y is CPC_EINVAL.  The reductions take C a multiple
 * of 4 up to 1024 (their shared-memory layout); the two apply passes take any multiple of 4. */
int cpc_bn_bwd_reduce(const void* dy, const void* y, const int* gy, const void* x, const int* gx, const float* stats, float* slabs,
                      int relu, int nblocks, int x_f32, int dtype, void* stream);
int cpc_bn_bwd_apply(const void* dy, const void* y, const int* gy, const void* x, void* dx, const int* gx, const float* stats,
                     const float* gamma, const float* dgamma, const float* dbeta, double count, int relu, int train, int x_f32,
                     int dtype, void* stream);
/* The same three passes with the activation's ReLU mask as SIGN BITS (one byte per 8 channels of a position, bit e = channel 8 i + e
 * is > 0, indexed by the element offset in the activation grid / 8): cpc_bn_apply_bits also writes them, the two backward passes read
 * them INSTEAD of the activation (2 bytes per element less in each; a ReLU's backward needs nothing else of it).  bf16 grids with C a
 * multiple of 8 only (CPC_EINVAL otherwise); relu is implied in the backward passes. */
int cpc_bn_apply_bits(const void* x, const int* gx, void* out, const int* go, const float* stats, const float* gamma, const float* beta,
                      int relu, void* out_bits, int dtype, void* stream);
int cpc_bn_bwd_reduce_bits(const void* dy, const void* y_bits, const int* gy, const void* x, const int* gx, const float* stats,
                           float* slabs, int nblocks, int dtype, void* stream);
int cpc_bn_bwd_apply_bits(const void* dy, const void* y_bits, const int* gy, const void* x, void* dx, const int* gx, const float* stats,
                          const float* gamma, const float* dgamma, const float* dbeta, double count, int train, int dtype, void* stream);
/* nn.MaxPool2d(kernel = stride = p): ceil mode (residual branches, scalogram_model.py:434-436; window clipped at the border)
 * or floor mode (main-branch pooling, :401-403; remainder dropped) according to the extents of the output grid; the backward
 * routes dout to the first maximum of each window in (dh outer, dw inner) scan order (+= if accumulate).
 * Contract of accumulate = 0: the call writes EXACTLY the positions covered by a window — the gradient at the first maximum, 0 at
 * the window's other positions.  In ceil mode that is every valid position; in floor mode the dropped remainder rows / columns are
 * not written and keep whatever din held: the caller owns them (clear din first, or never write them).  Pad and guard rows are
 * never written. */
int cpc_maxpool2d_fwd(const void* in, const int* gi, void* out, const int* go, int p, int in_f32, int dtype, void* stream);
int cpc_maxpool2d_bwd(const void* in, void* din, const int* gi, const void* dout, const int* go, int p, int accumulate, int dtype,
                      void* stream);
/* out = act(a + r(w + ow, h + oh)) — the cropped residual add (scalogram_model.py:453-472) with the inter-block ReLU
 * (:525-526) folded in; backward: da = g, dr(w + ow, h + oh) = g with g = dout * (out > 0) if relu.  Contract: the backward writes dr
 * only inside the crop window and leaves every position outside it untouched — a caller that wants zeros there clears dr once (the
 * engine relies on its allocation's zeros: every step overwrites the same interior).  With relu = 0, out is not read and may be NULL.
 * r_f32: the residual grid r / dr is float32 although dtype is bf16 (first block, see x_f32 above). */
int cpc_residual_add(const void* a, const int* ga, const void* r, const int* gr, void* out, const int* go, int oh, int ow, int relu,
                     int r_f32, int dtype, void* stream);
int cpc_residual_add_bwd(const void* dout, const void* out, const int* go, void* da, const int* ga, void* dr, const int* gr, int oh,
                         int ow, int relu, int r_f32, int dtype, void* stream);

/* dst bf16 [3n]: (hi, lo, hi) per f32 sample, hi = bf16(x), lo = bf16(x - hi).  With filter rows laid out (wh, wh, wl) the CQT
 * filter bank runs as bf16 MFMA GEMMs with f32-grade accuracy (xh wh + xl wh + xh wl; the dropped lo*lo term is ~2^-16
 * relative) — the "bf16x3" precision of constant_q_transform.CQT. */
int cpc_split3_bf16(const float* src, void* dst, long long n, void* stream);

/* FIRST BLOCK OF THE SCALOGRAM ENCODER ("stem", ABI version 6): nn.Conv2d on the float32 scalogram (1-4 input channels) + train-mode
 * nn.BatchNorm2d + ReLU (scalogram_model.py:392-406 of the first ScalogramEncoderBlock) WITHOUT storing the convolution's output:
 * every pass recomputes it from the input columns (bit-identically), so the 32-wide float32 tensor of 5 M positions that im2col + GEMM
 * moved three times per direction never exists.  x f32 grid gx = {B, W, H, Ha, top = 0, Cin}; w f32 [Cout][Cin][kh][kw] and bias
 * f32 [Cout] (or NULL) are the reference's parameters; conv = {Cout, kh, kw, sh, sw, ph, pw, Ho, Wo} (int[9]).
 *   cpc_stem_supported : 1 when the window shape / channel counts have kernels (Cout a multiple of 4 up to 64 dividing 1024;
 *                        (Cin, kh, kw, sh) one of (1|2, 3,3, 1|2), (1|2, 5,1, 1), (1|2, 2,2, 1): compile-time shapes, the weights and a
 *                        lane's input window live in registers), else 0 (callers take the im2col route)
 *   cpc_stem_stats     : slabs f32 [nblocks][2][Cout] partial (sum y, sum y^2)                       -> cpc_bn_finalize
 *   cpc_stem_apply     : out (T grid go, any row geometry) = relu((y - mean) rstd gamma + beta)
 *   cpc_stem_bwd_reduce: slabs f32 [nblocks][2][Cout] partial (sum g xhat, sum g), g = da * (a > 0) -> cpc_reduce_slabs (dgamma, dbeta)
 *   cpc_stem_bwd_wgrad : slabs f32 [nblocks][Cout][Cin*kh*kw] partial sums of dy (x) window, dy = gamma rstd (g - dbeta/n - xhat dgamma/n)
 *                        formed per position and never stored -> cpc_reduce_slabs gives d loss / d w in the reference's layout.
 *                        (The bias gradient of a convolution in front of a train-mode BatchNorm is exactly zero.)
 * Residual branch of the same block (scalogram_model.py:434-446, :462-472): xp f32 grid gp = the max-pooled input (cpc_maxpool2d_fwd),
 * wr f32 [Cout][Cin] the 1x1 projection (no bias, padding 0; Cin 1 or 2, Cout a multiple of 8 (bf16) / 4 (f32) dividing 2048 / 1024):
 *   cpc_stem_residual_add: out = act(main + wr xp(w + ow, h + oh))
 *   cpc_stem_residual_bwd: g = dout * (out > 0 if relu); dmain = g; slabs f32 [nblocks][Cout][Cin] partial sums of g (x) xp. */
int cpc_stem_supported(int cin, int cout, int kh, int kw, int sh, int hin, int ph);
int cpc_stem_stats(const float* x, const int* gx, const float* w, const float* bias, const int* conv, float* slabs, int nblocks,
                   void* stream);
int cpc_stem_apply(const float* x, const int* gx, const float* w, const float* bias, const int* conv, const float* stats,
                   const float* gamma, const float* beta, void* out, const int* go, int nblocks, int dtype, void* stream);
int cpc_stem_bwd_reduce(const float* x, const int* gx, const float* w, const float* bias, const int* conv, const float* stats,
                        const void* da, const void* a, const int* ga, float* slabs, int nblocks, int dtype, void* stream);
int cpc_stem_bwd_wgrad(const float* x, const int* gx, const float* w, const float* bias, const int* conv, const float* stats,
                       const float* gamma, const float* dgamma, const float* dbeta, double count, const void* da, const void* a,
                       const int* ga, float* slabs, int nblocks, int dtype, void* stream);
/* cpc_stem_residual_bn_add (bf16): cpc_bn_apply (+ReLU) of the block's second BatchNorm and cpc_stem_residual_add in one pass — y is the
 * BatchNorm's INPUT grid; out = act(bf16(relu(BatchNorm(y))) + wr xp(w + ow, h + oh)); bits (may be NULL): the sign bits of the normalised branch,
 * addressed like its activation grid ga (what the BatchNorm's backward pass reads); obits (may be NULL): the sign bits of out, addressed like out.
 * Bit-identical to the two passes. */
int cpc_stem_residual_bn_add(const void* y, const int* gy, const float* xp, const int* gp, const float* wr, void* out, const int* go, int oh, int ow,
                             int relu, const float* stats, const float* gamma, const float* beta, unsigned char* bits, const int* ga,
                             unsigned char* obits, int dtype, void* stream);
/* cpc_stem_residual_wgrad_bits (bf16): the projection's weight-gradient slabs of cpc_stem_residual_bwd with the ReLU mask taken from obits (the
 * sign bits of out that cpc_stem_residual_bn_add wrote, addressed like out) and WITHOUT storing the masked gradient: cpc_bn_bwd_*_res read dout
 * and the same bits.  gm: the main branch's grid (geometry only). */
int cpc_stem_residual_wgrad_bits(const void* dout, const unsigned char* obits, const int* go, const int* gm, const float* xp, const int* gp,
                                 float* slabs, int oh, int ow, int nblocks, int dtype, void* stream);
int cpc_stem_residual_add(const void* main_, const int* gm, const float* xp, const int* gp, const float* wr, void* out, const int* go,
                          int oh, int ow, int relu, int dtype, void* stream);
int cpc_stem_residual_bwd(const void* dout, const void* out, const int* go, void* dmain, const int* gm, const float* xp, const int* gp,
                          float* slabs, int oh, int ow, int relu, int nblocks, int dtype, void* stream);

/* ---- Wasserstein gradient penalty (contrastive_estimation_training.py:144-155: the gradient of the summed scores with respect
 * to the preprocessed batch, its 2-norm over the channel axis pushed towards 1, differentiated again by loss.backward()) ----
 * The penalty's parameter gradient is the parameter gradient of the directional derivative of the summed scores along
 * v = d penalty / d (input gradient); it is computed as a tangent (forward-mode) pass of v through the network plus extra
 * weight-gradient GEMMs and, at every train-mode BatchNorm, the second-order terms below.  The tangent
 * pass reuses the forward entry points with bias-free operands and the PRIMAL activations as ReLU masks; these three calls are
 * what it needs beyond them:
 * cpc_maxpool2d_select: out = element of `sel` at the first maximum of `in` in every p x p window (a max pooling applied to a
 *   tangent, selecting where the primal pooling selected); grids as for cpc_maxpool2d_fwd, `in` and `sel` share gi.
 * cpc_gp_direction: g f32 [npix][C] = gradient of the summed scores w.r.t. the channels-last scalogram; writes
 *   v = factor * 2 (|g| - 1) / |g| * g / npix (norm over the C channels of a pixel, :153) and per-block partial sums of
 *   (|g| - 1)^2 (penalty = factor * sum / npix).
 * cpc_bn_gp_cross: out = coef[c] * xhat + coef[C + c] * yt + coef[2C + c] * delta on the valid positions of grid gx, with
 *   xhat = (x - stats[c]) * stats[C + c]: the terms a train-mode BatchNorm adds to the adjoint of its input under the penalty. */
int cpc_maxpool2d_select(const void* in, const void* sel, const int* gi, void* out, const int* go, int p, int in_f32, int dtype,
                         void* stream);
int cpc_gp_direction(const float* g, float* v, long long npix, int C, float factor, float* partial, int nblocks, void* stream);
int cpc_bn_gp_cross(const void* x, const void* yt, const void* delta, void* out, const int* gx, const float* stats, const float* coef,
                    int x_f32, int dtype, void* stream);

/* g[i] = y[i] > 0 ? g[i] : 0 for i < n (n % 4 == 0): ReLU backward on whole buffers where no fused epilogue applies. */
int cpc_relu_mask(void* g, const void* y, long long n, int dtype, void* stream);

/* a[i] += b[i] for i < n (n % 4 == 0; ABI 8): the sum in f32, rounded once to the storage type.  Where two branches' data gradients meet
 * and the GEMM that produces the second cannot write into the first's grid (scalogram_model.py:462-476 under autograd). */
int cpc_accumulate(void* a, const void* b, long long n, int dtype, void* stream);

/* dst[r][c] = (T) src[r*sr + c*sc] — cast / transpose of a master weight into an operand layout. */
int cpc_cast2d(const float* src, void* dst, int R, int C, long long sr, long long sc, int dtype, void* stream);

/* Many cpc_cast2d jobs in one launch: jobs is a DEVICE array of njobs records {const float* src; void* dst; int64 R, C, sr, sc}
 * (six 64-bit fields each) with dst[r][c] = (T) src[r*sr + c*sc] — the per-step operand-layout copies of a context network's
 * nn.Linear weights (attention_model.py:59-66 keeps them f32; the GEMMs read storage-dtype copies). */
int cpc_cast2d_batch(const void* jobs, int njobs, int dtype, void* stream);
/* MFMA fragment order of a [R][Kd] operand (transpose: logical[n][k] = src[k*ld + n]) for the GRU kernels. */
int cpc_prep_frag(const float* src, void* dst, int R, int Kd, long long ld, int transpose, int dtype, void* stream);

/* AudioGRUModel.forward's python loop over nn.GRUCell (audio_model.py:66-77) as one persistent launch.
 * H: a multiple of 32 (bf16) or 16 (f32), at most 512 (weight-resident bf16 kernels for H in {32, 64, 128, 256}, weight-streaming
 * kernels otherwise: 4 waves per workgroup up to H = 256, 8 above).
 *   Gi    T   [B][V][3H]  = x_t W_ih^T + b_ih for all steps (cpc_gemm_nt), gate order r, z, n
 *   Wfrag T   cpc_prep_frag(weight_hh [3H][H]);  bhh f32 [3H]
 *   Hall  T   [B][V+1][H] hidden states (Hall[:,0] = 0)
 *   tape  T   cpc_gru_tape_elems(B,V,H,dtype) elements: saved activations (r, z, n, W_hn h + b_hn, h_{t-1}) in a layout
 *             private to the fwd/bwd kernel pair (lane-fragment order for the weight-resident bf16 kernels)
 *   c_out f32 [B][H] last hidden state (what AudioGRUModel.forward returns). */
long long cpc_gru_tape_elems(int B, int V, int H, int dtype);
int cpc_gru_fwd(const void* Gi, const void* Wfrag, const float* bhh, void* Hall, void* tape, float* c_out, int B, int V,
                int H, int dtype, void* stream);
/* The same with an initial hidden state h0 f32 [B][H] (NULL = zeros): AudioGRUModel(reset_hidden=False) carries the last hidden state
 * of one call into the next (audio_model.py:69, :75).  Forward only: the reference's autograd cannot differentiate a second call
 * through the first one's graph either. */
int cpc_gru_fwd_h0(const void* Gi, const void* Wfrag, const float* bhh, const float* h0, void* Hall, void* tape, float* c_out, int B,
                   int V, int H, int dtype, void* stream);
/* Backward through time: dc f32 [B][H] -> dG T [B][V][4H] = [d r_pre | d z_pre | d n_pre | d n_pre * r]: columns [0,3H) are
 * the gradient w.r.t. the input-projection term, columns [0,2H) and [3H,4H) the gradient w.r.t. h W_hh^T + b_hh.
 * WTfrag = cpc_prep_frag(weight_hh, transpose=1) ([H][3H] logical). */
int cpc_gru_bwd(const float* dc, const void* tape, const void* WTfrag, void* dG, int B, int V, int H, int dtype,
                void* stream);
/* The same sweep for a layer that is not the top of a stack (AudioGRUModel(num_layers > 1)): a gradient arrives at EVERY hidden state.
 *   dHs   T   rows of H elements, row (b, t) at element (b V + t) ld_h: the gradient that reaches h_{t+1} = Hall[b][t+1] from outside
 *             the recurrence (for a stack: dG_above[:, :3H] W_ih_above, which cpc_gemm_nt writes in exactly this layout, ld_h = H).
 *             ld_h >= H and a multiple of 8 (bf16) / 4 (f32) elements, the base 16-byte aligned; columns [H, ld_h) and the rows of
 *             items >= B are never read.  NULL: the call IS cpc_gru_bwd (same kernels, same bits; dc is then required).
 *   dc    f32 [B][H] the gradient at the last hidden state, or NULL = zeros (a lower layer has none); the last state receives
 *             dc + dHs[:, V-1].
 * Step t starts from d = dh + dHs[b][t]; both the gate derivatives and the dh u term that goes on to step t - 1 use this d.
 * tape, WTfrag, dG, the supported H / dtype and the kernel choice (cpc_gru_set_streaming included) are cpc_gru_bwd's.
 * CPC_EINVAL before any launch: NULL tape / WTfrag / dG, dc and dHs both NULL, B < 1, V < 1, an H or dtype cpc_gru_bwd refuses,
 * a bad ld_h with dHs given.  (Added under ABI 9: no existing entry point changed.) */
int cpc_gru_bwd_steps(const float* dc, const void* dHs, long long ld_h, const void* tape, const void* WTfrag, void* dG, int B, int V,
                      int H, int dtype, void* stream);

/* AudioLSTMModel's recurrence (torch.nn.LSTMCell stepped over the V frames; not in the reference) as one persistent launch per
 * direction.  Gate order i, f, g, o.  With a = Gi[:, t] + h_{t-1} W_hh^T + b_hh:
 *   i = sigmoid(a_i), f = sigmoid(a_f), g = tanh(a_g), o = sigmoid(a_o), cell_t = f cell_{t-1} + i g, h_t = o tanh(cell_t).
 * H: a multiple of 32 (bf16) or 16 (f32), at most 512 (weight-streaming kernels: 4 waves per workgroup up to H = 256, 8 above).
 *   Gi       T   [B][V][4H]  = x_t W_ih^T + b_ih for all steps (cpc_gemm_nt)
 *   Wfrag    T   cpc_prep_frag(weight_hh [4H][H], R = 4H, Kd = H);  bhh f32 [4H] or NULL (zeros)
 *   h0, c0   f32 [B][H] initial hidden and cell state, each NULL = zeros (AudioLSTMModel(reset_hidden=False) carries the pair)
 *   Hall     T   [B][V+1][H] hidden states, Hall[:,0] = h0 (rounded to T)
 *   tape     T   cpc_lstm_tape_elems(B,V,H,dtype) elements, [B][V][6][H]: i, f, g, o, cell_{t-1}, tanh(cell_t), each rounded to T;
 *                private to the fwd/bwd kernel pair
 *   h_out, cell_out f32 [B][H] the last hidden and cell state (the f32 masters; h_out is what AudioLSTMModel.forward returns).
 * The masters of h and cell are f32 for the whole sequence; what is rounded to T is the copy of h the matrix product reads, Hall
 * and the tape.  A run of V steps therefore equals, bit for bit, the same data run in pieces with (h_out, cell_out) handed on as (h0, c0).
 * cpc_lstm_bwd: dh_last f32 [B][H], the gradient at h_V -> dG T [B][V][4H] = [d a_i | d a_f | d a_g | d a_o], the gradient with respect
 * to Gi and to h W_hh^T + b_hh alike.  WTfrag = cpc_prep_frag(weight_hh, R = H, Kd = 4H, ld = H, transpose = 1).  Per step, with
 * tc = tanh(cell_t):  d a_o = dh tc o(1-o);  dct = dcell + dh o (1 - tc^2);  d a_i = dct g i(1-i);  d a_f = dct cell_{t-1} f(1-f);
 * d a_g = dct i (1 - g^2);  dcell <- dct f;  dh <- dG[:, t] W_hh (from the values as rounded to T).
 * Rows of items >= B are neither read nor written.  cpc_lstm_tape_elems returns CPC_EINVAL for arguments the kernels refuse.
 * CPC_EINVAL before any launch: a NULL pointer other than bhh / h0 / c0, B < 1, V < 1, an H outside the rule above, a dtype other
 * than f32 / bf16.  (Added under ABI 9: no existing entry point changed.) */
long long cpc_lstm_tape_elems(int B, int V, int H, int dtype);
int cpc_lstm_fwd(const void* Gi, const void* Wfrag, const float* bhh, const float* h0, const float* c0, void* Hall, void* tape,
                 float* h_out, float* cell_out, int B, int V, int H, int dtype, void* stream);
int cpc_lstm_bwd(const float* dh_last, const void* tape, const void* WTfrag, void* dG, int B, int V, int H, int dtype, void* stream);
/* The same sweep with a gradient at EVERY hidden state (predictions from several context steps, "prediction anchors"): the LSTM
 * counterpart of cpc_gru_bwd_steps, with its contract.
 *   dHs      T   rows of H elements, row (b, t) at element (b V + t) ld_h: the gradient that reaches h_{t+1} = Hall[b][t+1] from
 *                outside the recurrence.  ld_h >= H and a multiple of 8 (bf16) / 4 (f32) elements, the base 16-byte aligned; columns
 *                [H, ld_h) and the rows of items >= B are never read.  NULL: the call IS cpc_lstm_bwd (same kernels, same bits;
 *                dh_last is then required).
 *   dh_last  f32 [B][H] the gradient at the last hidden state, or NULL = zeros; the last state receives dh_last + dHs[:, V-1].
 * Step t starts from d = dh + dHs[b][t].  tape, WTfrag, dG and the supported H / dtype are cpc_lstm_bwd's.
 * CPC_EINVAL before any launch: NULL tape / WTfrag / dG, dh_last and dHs both NULL, B < 1, V < 1, an H or dtype cpc_lstm_bwd refuses,
 * a bad ld_h with dHs given.  (Added under ABI 9: no existing entry point changed.) */
int cpc_lstm_bwd_steps(const float* dh_last, const void* dHs, long long ld_h, const void* tape, const void* WTfrag, void* dG, int B,
                       int V, int H, int dtype, void* stream);

/* Prediction anchors: the target-gradient windows of A anchors summed into the top-layer gradient.
 *   dT    f32 [A][B][K][E]: d loss / d targets of every anchor; the window of anchor a covers top rows
 *         [first_row + a stride, first_row + a stride + K)
 *   dtop  T   row r of item b at element b item_stride + r E (item_stride a multiple of 8 (bf16) / 4 (f32) and >= row_hi E, the base
 *         16-byte aligned)
 * For every item and every row r in [row_lo, row_hi): dtop[b][r][:] = sum over the anchors a with 0 <= r - first_row - a stride < K of
 * dT[a][b][r - first_row - a stride][:], in f32 with a ascending, plus the stored row when accumulate != 0, rounded once.  A row of the
 * range that no window covers is written as zeros (accumulate == 0) or left alone (accumulate != 0).  Nothing outside [row_lo, row_hi)
 * of the B items is touched.  A gather per output row: no atomics, the order of every sum fixed by the arguments.
 * CPC_EINVAL before any launch: a NULL pointer; A, B or K < 1; stride < 1; E not a positive multiple of 8 (bf16) / 4 (f32); row_lo < 0,
 * row_hi <= row_lo or first_row < 0; a bad item_stride; a dtype other than f32 / bf16.  (Added under ABI 9: no existing entry point
 * changed.) */
int cpc_anchor_target_grad(const float* dT, void* dtop, long long item_stride, int A, int B, int K, int E, int first_row, int stride,
                           int row_lo, int row_hi, int accumulate, int dtype, void* stream);

/* The Wasserstein gradient penalty through AudioGRUModel (contrastive_estimation_training.py:144-158: loss.backward() through
 * torch.autograd.grad(..., create_graph=True), here for the GRUCell loop of audio_model.py:66-77).  f32 only, H <= 512.
 * cpc_gru_gp_fwd: primal and tangent recurrence together.  Gi as for cpc_gru_fwd (f32); GiT [B][V][3H] = (tangent of x_t) W_ih^T
 * (no bias); WT [H][3H] = weight_hh transposed; bhh [3H]; tape f32 [B][V][10][H] (r, z, n, W_hn h + b_hn, h_{t-1}, then the
 * tangents of the pre-activations of r and z, of W_hn h, of the pre-activation of n, and of h_{t-1}); ct_out [B][H] = tangent of
 * the last hidden state.
 * cpc_gru_gp_bwd: reverse sweep of the joint program seeded with dc [B][H], the adjoint of the SUMMED SCORES at the last hidden
 * state; W = weight_hh [3H][H].  dA f32 [B][V][8][H]: columns [0,4H) = [d r_pre | d z_pre | d n_pre | d n_pre * r] of the summed
 * scores (to be contracted with the TANGENT inputs / hidden states for the weight gradients), columns [4H,8H) the same four of
 * the second-order adjoint (contracted with the primal inputs / hidden states; [4H,7H) W_ih is what the encoder's top-layer
 * gradient gains).
 * Preconditions, each refused with CPC_EINVAL before any launch: every pointer not NULL (bhh included: a GRU without biases is not
 * supported here); B >= 1, V >= 1, 1 <= H <= 512.  H need NOT be a multiple of 16 or of the wave size (one thread per hidden unit,
 * the last wave partly idle).  Both kernels write every element of tape, ct_out and dA (no accumulation); the tangent slots of
 * h_{t-1} and W_hn h at t = 0 are exact zeros.  (Pinned by tests/test_penalty_reference_host.py and tests/test_penalty_kernels_gpu.py.) */
int cpc_gru_gp_fwd(const float* Gi, const float* GiT, const float* WT, const float* bhh, float* tape, float* ct_out, int B,
                   int V, int H, void* stream);
int cpc_gru_gp_bwd(const float* dc, const float* tape, const float* W, float* dA, int B, int V, int H, void* stream);

/* A/B switch: on != 0 forces the weight-streaming GRU kernels where the weight-resident bf16 ones would be used
 * (H in {32,64,128,256}), on == 0 restores the default; returns the previous setting (0 or 1).  Not stream-ordered (host-side flag). */
int cpc_gru_set_streaming(int on);

/* InfoNCE loss of ContrastiveEstimationTrainer.train, default branch score_over_all_timesteps=False
 * (contrastive_estimation_training.py:116-122, :141) on the equal-step scores S[k][b][b'] (f32, rows of ld >= B
 * floats; dS / dST use the same ld and get zeros in the pad columns), with the score
 * function folded in (softplus != 0: softplus_score_function :12-16, else linear_score_function :19-22).
 *   out f32[8]: out[0] = loss (incl. regulariser), out[1] = max score (logger value, :166), out[2..4] = -mean valid, mean lse,
 *   reg; out[5] = 1 if the loss before the regulariser (out[2] + out[3]) is NaN — the value the reference's NaN guard tests
 *   (:124) — else 0; out[6] = sticky NaN flag: set to 1 together with out[5], never cleared by the library (the caller zeroes it
 *   when a run starts; cpc_adam's `skip` argument).  cpc_nce_loss_all writes the same eight values.
 *   dS[k][b][b'], dST[k][b'][b] (T): d loss / d linear score.  workspace: cpc_nce_workspace_floats(B,K) f32.
 * CPC_EINVAL for B <= 0, K <= 0, ld < B, ld > B + 7 (cpc_nce_loss_all: ld < B K), a dtype other than f32 / bf16 and a null pointer.
 * A refused call of cpc_nce_loss, cpc_nce_loss_all or cpc_nce_loss_sampled launches nothing: every buffer, the workspace included,
 * keeps its bytes.  One +inf among a column's linear scores gives lse = +inf for that column (loss +inf, out[5] stays 0). */
long long cpc_nce_workspace_floats(int B, int K);
int cpc_nce_loss(const float* S, void* dS, void* dST, float* out, float* workspace, int B, int K, int ld, int softplus,
                 float regularization, int dtype, void* stream);

/* The same loss over N SAMPLED negatives per target (not in the reference; DESIGN.md, "Sampled negatives"): column (k, b') runs its
 * log-sum-exp over C(k,b') = {b'} + Neg(k,b') instead of all B rows, Neg the n_neg rows b != b' with the smallest (key, b),
 *   s = seed + 0x632BE59BD9B4E019 draw;  z = s + 0x9E3779B97F4A7C15 (k + 1) + (b' B + b) 0xD1B54A32D192ED03;
 *   z = (z ^ z >> 30) 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) 0x94D049BB133111EB;  z ^= z >> 31;  key = z >> 32      (all mod 2^64)
 * — a pure function of its arguments: the same (seed, draw) selects the same rows on every device and launch geometry.
 *   loss = -mean valid + mean_{k,b'} logsumexp_{b in C} sp + reg mean_{b,b'} (mean_k sp)^2        (regulariser over ALL scores)
 *   dsp[k][b][b'] = ([b in C(k,b')] exp(sp - lse[k][b']) - [b == b']) / (B K) + 2 reg / (B^2 K) mean_k sp[k][b][b']
 * S, dS, dST, out[8], ld, softplus, dtype and the pad-column zeros exactly as cpc_nce_loss (out[1] stays the max over all scores);
 * n_neg == B - 1 is cpc_nce_loss's loss (its column pass skips the search).  workspace: cpc_nce_sampled_workspace_floats(B,K) f32, 8-byte aligned.
 * Limits: 2 <= B <= 1024, 1 <= n_neg <= B - 1; CPC_EINVAL otherwise, for a null pointer and for a dtype other than f32 / bf16.
 * cpc_nce_sample_mask writes the candidate sets themselves, by the same device selection routine: mask[k][b][b'] (bytes, no padding)
 * = 1 where b is in C(k,b') (the diagonal included), else 0. */
long long cpc_nce_sampled_workspace_floats(int B, int K);
int cpc_nce_loss_sampled(const float* S, void* dS, void* dST, float* out, float* workspace, int B, int K, int ld, int softplus,
                         float regularization, int n_neg, unsigned long long seed, unsigned long long draw, int dtype, void* stream);
int cpc_nce_sample_mask(unsigned char* mask, int B, int K, int n_neg, unsigned long long seed, unsigned long long draw, void* stream);

/* cpc_nce_loss_sampled with the candidates restricted by a per-item group id (not in the reference; DESIGN.md, "Grouped negatives").
 * groups: B int32 on the device, any values (only equality matters); mode 0 = same, 1 = other; n_neg 0 = every eligible row, else 1 .. B - 1.
 *   Elig(b')  = { b != b' : (groups[b] == groups[b']) == (mode == 0) }                               (does not depend on k)
 *   n(b')     = |Elig(b')| if n_neg == 0, else min(n_neg, |Elig(b')|)
 *   C(k,b')   = {b'} + the n(b') rows of Elig(b') with the smallest (key, b), key the hash of cpc_nce_loss_sampled with the same
 *               (seed, draw) and B the batch size
 * Loss, dsp, out[8], the layouts, ld, softplus, dtype and the pad-column zeros are cpc_nce_loss_sampled's with this C (regulariser, max
 * score and valid scores over ALL scores).  A target whose eligible set is empty has lse = sp[k][b'][b']: it contributes 0 and stays in
 * the mean.  A column that keeps its whole eligible set (always with n_neg == 0) computes no hash.  One group for the whole batch with
 * mode 0: n_neg = N selects cpc_nce_sample_mask's sets and gives cpc_nce_loss_sampled's outputs bit for bit (both entry points run
 * one kernel template), n_neg = 0 is cpc_nce_loss's loss.
 * workspace: cpc_nce_grouped_workspace_floats(B,K) f32, 8-byte aligned.
 * Limits: 2 <= B <= 1024, B <= ld <= B + 7, mode in {0, 1}, 0 <= n_neg <= B - 1; CPC_EINVAL otherwise, for a null pointer (groups
 * included), for a dtype other than f32 / bf16 and for a workspace that is not 8-byte aligned — before any launch: a refused call
 * writes nothing.
 * cpc_nce_group_mask writes the candidate sets by the same device selection routine: mask[k][b][b'] (bytes, no padding) = 1 where b is
 * in C(k,b') (the diagonal included), else 0. */
long long cpc_nce_grouped_workspace_floats(int B, int K);
int cpc_nce_loss_grouped(const float* S, void* dS, void* dST, float* out, float* workspace, int B, int K, int ld, int softplus,
                         float regularization, const int* groups, int mode, int n_neg, unsigned long long seed, unsigned long long draw,
                         int dtype, void* stream);
int cpc_nce_group_mask(unsigned char* mask, const int* groups, int B, int K, int mode, int n_neg, unsigned long long seed,
                       unsigned long long draw, void* stream);

/* cpc_nce_loss with the predictions of earlier steps as further candidates (not in the reference; DESIGN.md, "Negative bank").
 * 2 <= slots <= 64 ring slots of B prediction rows each, N = slots B; sp = f(S), f the identity or softplus; V the rows of the slots
 * whose bit is set in valid_mask (bit cur always; no bit at or above slots):
 *   S[k][r][b'] = < R[r][k][:], targets[b'][:, k] >,  r in [0, N)          (f32, [K][N][ld], B <= ld <= B + 7, formed by the caller)
 *   loss = -mean_{b',k} sp[k][cur B + b'][b'] + mean_{k,b'} logsumexp_{r in V} sp[k][r][b']
 *          + reg mean_{b,b'} (mean_k sp[k][cur B + b][b'])^2                                         (current slot only, as cpc_nce_loss)
 *   dsp[k][r][b'] = [r in V] exp(sp - lse[k][b']) / (B K) - [r == cur B + b'] / (B K) + [r in slot cur] 2 reg / (B^2 K) mean_k sp[k][r][b']
 *   dS[k][r][b'] = dsp f'(S)  (T, [K][N][ld]);  dST_cur[k][b'][b] = dS[k][cur B + b][b']  (T, [K][B][ld], cpc_nce_loss's dST)
 * The rows of invalid slots are WRITTEN as zero coefficients by every call, and the pad columns [B, ld) of dS and dST_cur get zeros, so
 * that GEMMs may run over all N rows and ld columns; the scores of invalid slots are never read.  out[8] as cpc_nce_loss: the max
 * score, the valid scores and the pair means run over slot cur; a NaN among the scores of any valid slot reaches out[0] and raises
 * out[5] / out[6].  With valid_mask == 1 << cur the loss, out[] and the coefficients of slot cur are cpc_nce_loss's (other summation
 * order of the log-sum-exp).  No atomics; the summation order is fixed by B and slots alone.
 * workspace: cpc_nce_banked_workspace_floats(B, K, slots) f32, 8-byte aligned (it starts with 8-byte pairs).
 * Limits: 2 <= B <= 1024, 1 <= K <= 1024; CPC_EINVAL otherwise and for slots outside [2, 64], cur outside [0, slots), a valid_mask without
 * bit cur or with a bit at or above slots, ld outside [B, B + 7], a null pointer, a dtype other than f32 / bf16 and a workspace that
 * is not 8-byte aligned — before any launch: a refused call writes nothing. */
long long cpc_nce_banked_workspace_floats(int B, int K, int slots);
int cpc_nce_loss_banked(const float* S, void* dS, void* dST_cur, float* out, float* workspace, int B, int K, int ld, int slots, int cur,
                        unsigned long long valid_mask, int softplus, float regularization, int dtype, void* stream);

/* Wasserstein gradient penalty with softplus_score_function (contrastive_estimation_training.py:12-16 under :144-158): the
 * coefficients the penalty's seeds carry.  S (and the tangent scores St1 + St2, St2 may be NULL): nmat f32 matrices [rows][ld].
 * mode 0: w = softplus'(s) = sigmoid(s) (1 beyond torch's threshold 20); mode 1: w = softplus''(s) * (St1 + St2).
 * W [nmat][rows][ld] and its transpose WT [nmat][cols][ldT], both f32. */
int cpc_gp_score_coeff(const float* S, const float* St1, const float* St2, float* W, float* WT, int nmat, int rows, int cols, int ld,
                       int ldT, int mode, void* stream);

/* Same loss with score_over_all_timesteps=True (contrastive_estimation_training.py:108-114, :141): S is the full
 * (B*K) x (B*K) score matrix, row (b,k) = prediction, column (b',k') = target, ST its transpose (both f32, rows of ld
 * floats, produced by two cpc_gemm_nt calls); dS / dST (T, same ld) receive d loss / d linear score and its transpose. */
long long cpc_nce_all_workspace_floats(int B, int K);
int cpc_nce_loss_all(const float* S, const float* ST, void* dS, void* dST, float* out, float* workspace, int B, int K, int ld,
                     int softplus, float regularization, int dtype, void* stream);

/* score_over_all_timesteps=True with the column pass FUSED into the score contraction (bf16 storage; ABI 8).  The reference forms the
 * (B K) x (B K) score tensor (contrastive_estimation_training.py:12-22) and takes logsumexp over its first two axes (:109-110); here the
 * f32 score matrix is never written:
 *   cpc_score_lse      scores s[r][c] = <P[r][:], T[c][:]> (P [M][ldp], T [N][ldt] bf16, E a multiple of 64 and >= 128, M and N multiples of
 *                      256) on 256 x 256 tiles of a persistent MFMA kernel whose epilogue leaves, per M tile and column, the online pair
 *                      pm / ps [M / 256][N] = (max, sum exp(s - max)) over the tile's rows, taken from the f32 accumulators; valid[r] =
 *                      s[r][r + diag_off] where that column exists (a prediction's own target; may be NULL); S [M][lds] f32 = the scores,
 *                      for cpc_nce_fused_grad (NULL: not stored) — f32 because that pass takes exp(score - lse): a bf16 copy of a
 *                      score of 100 is off by up to 0.4, its softmax weight by half (measured: gradient cosine 0.48).
 *   cpc_nce_lse_merge  lse[c] = log( sum over ALL rows of exp(score(s[r][c])) ) from the pairs: for softplus scores exp(softplus(s)) =
 *                      1 + exp(s), so lse = log(nrows_total + sum ps exp(pm)) — no softplus is evaluated; colp [ceil(ncols / 256)][2] =
 *                      {sum of the block's lse, max of its pm}.
 *   cpc_nce_fused_grad d loss / d linear score (bf16, dS [items K][ld]; and its transpose, dST [ncols][ldT], or NULL) from S and lse, as cpc_nce_loss_all forms it:
 *                      (exp(sp - lse[c]) - [c == r + diag_off]) / n_rows_total + 2 reg / (n_items_total^2 K^2) mean_k sp[(b,k)][c], times the score
 *                      function's derivative; rows r = (item, k), items K of them, K even and <= 24, ncols a multiple of 4; gradp
 *                      [cpc_nce_fused_grad_blocks(items, ncols)] = partial sums of (mean_k sp)^2 (the regulariser :141).
 *   cpc_nce_fused_finalize   the eight values cpc_nce_loss_all writes to `out`.  mode 0: from the partials (colp, valid, gradp); mode 1:
 *                      the partials reduced to sums[4] = {sum valid, sum lse, sum m^2, max s} only — a rank that holds a strip of the
 *                      global score matrix all-reduces them (SUM, SUM, SUM, MAX) — and mode 2: out from sums.  n_rows_total /
 *                      n_items_total: rows (predictions) and items of the WHOLE score matrix.
 * Rectangular problems (M != N, diag_off != 0) are the strips of engine.GlobalNegatives: a rank computes all predictions x its own
 * targets and its own predictions x all targets instead of the whole global matrix.
 * Preconditions (CPC_EINVAL otherwise, before any launch: a refused call writes nothing):
 *   cpc_score_lse      P, T, pm, ps not NULL; M, N > 0 and multiples of 256; E >= 128 and a multiple of 64; ldp, ldt >= E and multiples of 8;
 *                      P and T 16-byte aligned; with S: lds >= N, a multiple of 4, S 16-byte aligned (lds is ignored when S is NULL).
 *                      Reads E elements of every row of P and T, nothing of the ldp - E / ldt - E padding; writes columns [0, N) of S.
 *                      valid[r] is written only where 0 <= r + diag_off < N: every other element of valid keeps what it held (any
 *                      diag_off is accepted; with diag_off >= N or <= -M nothing of valid is touched).  S = NULL changes no other output.
 *   cpc_nce_lse_merge  pm, ps, lse, colp not NULL; nparts, ncols > 0 (ncols need not be a multiple of 256: the last block of colp covers
 *                      the columns that exist).  nrows_total is used by softplus scores only and need not be 256 nparts.
 *   cpc_nce_fused_grad S, lse, dS not NULL and, with dST, 16-byte aligned; items > 0; K even, 2 <= K <= 24; ncols > 0 and a multiple
 *                      of 4; ld >= ncols and a multiple of 8 (the bf16 rows of dS are stored in 8-byte groups from 16-byte loads of S: the
 *                      same ld serves both); with dST: ldT >= items K and a multiple of 8.  Columns [ncols, ld) of S are not read, those
 *                      of dS and columns [items K, ldT) of dST not written.  dST = NULL and gradp = NULL leave dS as it is with them.
 *   cpc_nce_fused_finalize   mode in {0, 1, 2}; colp, valid, gradp not NULL and ncolp, nvalid, ngrad >= 0 unless mode == 2; sums not NULL
 *                      unless mode == 0; out not NULL unless mode == 1.  Writes out[0..5] and, only when out[5] is raised, out[6] = 1
 *                      (sticky: the caller clears it); out[7] and sums[4..] are never touched; mode 1 writes sums[0..3] only.
 * Non-finite scores: a NaN score reaches ps of its tile and column (the maxima are taken with fmaxf, which drops it, so pm stays
 * finite), from there lse, colp, out[0] and the flags out[5] / out[6].  An infinite score does NOT give lse = +inf as in the dense
 * kernels: the epilogue forms exp(s - max) = exp(inf - inf), so a +inf score (and a column that is -inf throughout the 128 rows of a half tile) gives ps = NaN
 * and lse = NaN, i.e. the step is flagged like a NaN; a -inf score beside finite ones contributes exp(-inf) = 0. */
int cpc_score_lse(const void* P, const void* T, float* S, float* pm, float* ps, float* valid, int M, int N, int E, long long ldp,
                  long long ldt, long long lds, int diag_off, void* stream);
int cpc_nce_lse_merge(const float* pm, const float* ps, int nparts, int ncols, int softplus, float nrows_total, float* lse, float* colp,
                      void* stream);
long long cpc_nce_fused_grad_blocks(int items, int ncols);
int cpc_nce_fused_grad(const float* S, const float* lse, void* dS, void* dST, float* gradp, int items, int K, int ncols, long long ld,
                       long long ldT, int diag_off, int softplus, float regularization, float n_rows_total, float n_items_total, void* stream);
int cpc_nce_fused_finalize(const float* colp, int ncolp, const float* valid, int nvalid, const float* gradp, int ngrad, float* sums, int mode,
                           float n_rows_total, float n_items_total, int K, float regularization, int softplus, float* out, void* stream);

/* The per-batch quantities of ContrastiveEstimationTrainer.validate (contrastive_estimation_training.py:227-247) from the same
 * score matrices the train step uses (S of cpc_nce_loss when all_timesteps == 0, S of cpc_nce_loss_all otherwise; softplus as
 * there): out[0..K) = prediction_losses per step (:237-241, including the reference's reading of the (k, b') log-sum-exps as a
 * (B, K) matrix in flat order in the default branch), out[K..2K) = prediction_accuracy per step (:245-247: arg max over the
 * targets of every prediction equal to its own target; first maximum on ties, first NaN if the row holds one, as torch.argmax), out[2K] = mean score (:249).  accumulate != 0
 * adds to out instead of overwriting it (validate sums over batches and divides once).  workspace:
 * cpc_nce_eval_workspace_floats(B, K) f32. */
long long cpc_nce_eval_workspace_floats(int B, int K);
int cpc_nce_eval(const float* S, float* out, float* workspace, int B, int K, int ld, int softplus, int all_timesteps, int accumulate,
                 void* stream);

/* Difference scores, difference_score_function (contrastive_estimation_training.py:25-33): s[r][c] = 1 / sum_e (p[r][e] - t[c][e])^2,
 * f32 accumulation of the squared DIFFERENCES (the reference subtracts first; |p|^2 + |t|^2 - 2 p.t would cancel exactly where the
 * score is largest).  Inputs P, T: storage type T; outputs f32, rows of lds floats (lds >= N for S, >= M for ST).
 *   cpc_diff_scores   S[z][m][n] = s(P row m of batch z, T row n of batch z) for m < M, n < N, z < batch, and, when ST != NULL, its
 *                     transpose ST[z][n][m] from the same pass.  P row m of batch z at z * p_batch + m * ldp; T row n at
 *                     z * t_batch + row address (n, t_rpi, t_item, ldt) (row addressing above); S / ST matrix z at z * s_batch.
 *                     Default branch: M = N = B, batch = K (S[k][b][b'] as cpc_nce_loss reads it); score_over_all_timesteps: M = N =
 *                     B K, batch = 1 (S and ST as cpc_nce_loss_all reads them).  Pad columns are left untouched.
 *   cpc_diff_scores_bwd   with g = d loss / d s (dS / dST of the loss kernels, T, same layouts), overwrites G[z][m][n] with
 *                     2 g s^2 = -(d loss / d squared distance), rounded to T, and writes its row sums (of the rounded values) to
 *                     sums[m * batch + z], f32; when GT != NULL the same for (GT, ST) -> sumsT[n * batch + z] in the same launch.
 *                     Then d predicted_z[r] = sum_c G[r][c] t[c] - sums[r] p[r] and d targets[c] = sum_r G[r][c] p[r] - sumsT[c] t[c]:
 *                     the two contractions of the linear score's gradient, followed by cpc_diff_scores_rank1 for the last terms.
 *   cpc_diff_scores_rank1 out[row][e] -= mu[row] * X[row][e] for row < rows, e < E; out and X rows at the row address
 *                     (row, rpi, item, ld); f32 arithmetic, one rounding to T. */
int cpc_diff_scores(const void* P, const void* T, float* S, float* ST, int M, int N, int E, long long ldp, long long ldt, int t_rpi,
                    long long t_item, long long p_batch, long long t_batch, long long s_batch, int batch, int lds, int dtype, void* stream);
int cpc_diff_scores_bwd(void* G, const float* S, float* sums, void* GT, const float* ST, float* sumsT, int M, int N, int lds,
                        long long s_batch, int batch, int dtype, void* stream);
int cpc_diff_scores_rank1(const float* mu, const void* X, void* out, int rows, int E, int rpi, long long item, long long ld, int dtype,
                          void* stream);

/* Row normalisation behind the cosine-similarity scores with a temperature (score kind "normalized"; no counterpart in the reference,
 * whose scores are the dot product, its softplus and the inverse squared distance):
 *   scores[b,k,b',k'] = < predicted_z[b,k,:] / max(|predicted_z[b,k,:]|, eps), targets[b',:,k'] / max(|targets[b',:,k']|, eps) > / tau,
 * i.e. linear scores of F.normalize(predicted_z, dim=2, eps) / tau and F.normalize(targets, dim=1, eps).  Row `row` of X, Y and G starts
 * at the row address (row, rpi, item, ld) (row addressing above): rpi = 0, ld = E for predicted_z; rpi = K, item = L_top * E, ld = E from
 * row T - K of the top layer for the K target rows of every item.  Elements the map does not name are never touched.  T: storage type.
 *   cpc_norm_rows      inv[row] = 1 / max(|X[row]|, eps) (f32 sum of the squares of the stored values, not rescaled) and
 *                      Y[row] = X[row] * (scale * inv[row]), one rounding to T.  scale = 1 / tau for predictions, 1 for targets.
 *                      A row of zeros gives zeros; a NaN in a row makes the whole row NaN (torch's clamp_min keeps it too).
 *   cpc_norm_rows_bwd  overwrites G, d loss / d Y in T, with d loss / d X = scale inv G - (inv / scale) <Y, G> Y per row (autograd's
 *                      gradient of the expression above: exact for the stored Y and G, f32 dot product, one rounding to T); rows with
 *                      inv >= 1 / eps (norm at or below eps) take the first term only.
 * One wave per row, the row in registers between the sum and the scaling (each row read once), 16-byte loads where the rows start
 * 16-byte aligned (X / Y / G, ld and item in 16-byte units; an E that is no multiple of that width leaves a scalar tail), else scalar
 * ones; sums in one fixed order (lane chain + xor butterfly): bit-identical from run to run and for any
 * rows.  CPC_EINVAL before any launch: a NULL pointer, rows < 1, E outside [1, 4096], rpi < 0, scale or eps not finite and > 0, an
 * unknown dtype. */
int cpc_norm_rows(const void* X, void* Y, float* inv, int rows, int E, int rpi, long long item, long long ld, float scale, float eps,
                  int dtype, void* stream);
int cpc_norm_rows_bwd(const void* Y, const float* inv, void* G, int rows, int E, int rpi, long long item, long long ld, float scale,
                      float eps, int dtype, void* stream);

/* A learnable or scheduled temperature ("Learnable and scheduled temperature"): the scale of the prediction rows lives in
 * device memory, so that a captured step can change it.  tstate f32[8] (device):
 *   [0] s = log(scale)   [1] scale = exp(s), what the two _dev kernels read   [2], [3] Adam's m and v of s
 *   [4] the latest g = d loss / d s, after grad_scale   [5] tau = 1 / scale   [6], [7] zero.
 *   cpc_norm_rows_dev      cpc_norm_rows with the scale read from scale[0] (device pointer, pass tstate + 1): for the same value it
 *                          writes cpc_norm_rows' bits.
 *   cpc_norm_rows_bwd_dev  cpc_norm_rows_bwd with the scale read from scale[0]; it also writes dots[row] = <Y[row], G[row]> (f32, over the
 *                          stored values, in the order of the kernel's own dot product, before G is overwritten), for every row: a row
 *                          whose norm was clamped still carries the scale.  dX has cpc_norm_rows_bwd's bits.  With pn = scale * p^ and
 *                          s = log(scale), d loss / d s = sum over the rows of <pn[row], d loss / d pn[row]> = the sum of dots.
 *   CPC_EINVAL as for cpc_norm_rows (the scale's value is not inspected), and for scale or dots NULL.
 *   cpc_temperature_step   g = grad_scale * sum(dots[0 .. rows)), one workgroup of 256 threads (thread i adds dots[i], dots[i + 256], ...
 *                          in that order, then a fixed tree in LDS: no atomics, the same data give the same bits); then
 *                          torch.optim.Adam's update of s without decay (cpc_adam's expressions in float32), s <- clamp(s, s_min, s_max),
 *                          scale = exp(s) and tau = exp(-s), each formed in double and rounded once.  tstate[0 .. 5] are written.
 *                          adam_state NULL: lr is the step's rate and the bias corrections of ``step`` (>= 1) are formed on the host in
 *                          double and rounded once, as in cpc_adam.  adam_state given (the f32[4] of cpc_adam_dev / cpc_adamw_dev, which
 *                          that call has already advanced; ``step`` is ignored): the step size is adam_state[1] * lr — lr then carries
 *                          only the scalar's own multiplier — and the second-moment correction adam_state[2]; no argument changes from
 *                          step to step, so the launch can be captured.  skip as in cpc_adam: while *skip != 0 nothing is written.
 *                          CPC_EINVAL before any launch: tstate or dots NULL, rows < 1, s_min > s_max, lr, beta1, beta2, eps, grad_scale,
 *                          s_min or s_max not finite, step < 1 without adam_state.
 *   cpc_temperature_set    a one-thread tick: tau of the 0-based step, in double (as cpc_lr_factors evaluates its factor), with
 *                          q = min(step / total_steps, 1):  kind 0 (linear) tau = start + (end - start) q;  kind 1 (cosine)
 *                          tau = end + (start - end) * 0.5 (1 + cos(pi q)).  Writes tstate[1] = (float)(1.0 / tau), tstate[0] = the log of
 *                          that float and tstate[5] = (float)tau.  adam_state given: step = step_offset + the device's step count (the
 *                          steps finished so far; ``step`` is ignored), so the launch can be captured in front of a step.
 *                          CPC_EINVAL: tstate NULL, kind outside {0, 1}, total_steps < 1, start or end not finite and > 0, a negative
 *                          step (step_offset with adam_state). */
int cpc_norm_rows_dev(const void* X, void* Y, float* inv, int rows, int E, int rpi, long long item, long long ld, const float* scale,
                      float eps, int dtype, void* stream);
int cpc_norm_rows_bwd_dev(const void* Y, const float* inv, void* G, float* dots, int rows, int E, int rpi, long long item, long long ld,
                          const float* scale, float eps, int dtype, void* stream);
int cpc_temperature_step(float* tstate, const float* dots, int rows, float lr, float beta1, float beta2, float eps, int step,
                         const float* adam_state, float grad_scale, float s_min, float s_max, const float* skip, void* stream);
int cpc_temperature_set(float* tstate, int kind, double start, double end, long long total_steps, long long step, const float* adam_state,
                        long long step_offset, void* stream);

/* torch.optim.Adam.step with default betas/eps semantics over one flat f32 buffer
 * (contrastive_estimation_training.py:83, :162).  step counts from 1; g is multiplied by grad_scale first.
 * skip (device pointer to one float, or NULL): the reference's NaN guard returns BEFORE backward() / optimizer.step()
 * (contrastive_estimation_training.py:124-133), so a NaN loss leaves the parameters at their last good values.  Here the update
 * is issued without waiting for the host to read the loss: while *skip != 0 — pass out + 6 of cpc_nce_loss / cpc_nce_loss_all,
 * the sticky NaN flag — the call changes nothing (p, m, v and the device-side step count keep their values).
 * p, g, m and v must be 16-byte aligned, here and in cpc_adam_dev, cpc_adam_clip, cpc_adamw and cpc_adamw_dev (the five run one
 * kernel, which moves them as float4; whole torch buffers, and ranges of them that start at a multiple of four floats, are).
 * CPC_EINVAL before any launch: p, g, m or v NULL, n <= 0, step < 1; cpc_adam_clip: the same and coef NULL; cpc_adam_dev: p, g, m, v
 * or state NULL, n <= 0. */
int cpc_adam(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
             int step, float grad_scale, const float* skip, void* stream);
/* The same update with the step count kept on the device: state f32[4] = {step count (int bits), lr/(1-b1^t), 1/sqrt(1-b2^t), -},
 * zero-initialised by the caller; every call advances the count first.  Nothing in the argument list changes from step to
 * step, so a train step captured in a hipGraph can be replayed. */
int cpc_adam_dev(float* p, const float* g, float* m, float* v, long long n, float lr, float b1, float b2, float eps, float* state,
                 float grad_scale, const float* skip, void* stream);


/* Gradient clipping by global norm: torch.nn.utils.clip_grad_norm_(parameters, max_norm) over one flat f32 gradient buffer (not in
 * the reference's train step; DESIGN.md, "Gradient clipping").  cpc_grad_norm replaces its norm and coefficient:
 *   state f32[4] (device): state[0] = || grad_scale * g ||_2, state[1] = min(1, max_norm / (state[0] + 1e-6)) — the factor
 *   clip_grad_norm_ multiplies every gradient by —, state[2] = 1 if the norm is NaN or inf, else 0 (then state[1] = 0),
 *   state[3] = max_norm.
 * Squares and sums are float32, in a fixed order without atomics: the same data give the same bits, and an element above about
 * 1e19 overflows its square and makes the norm inf — non-finite, as torch's float32 norm of it is.
 * nan_pair (two floats, or NULL): both are set to 1 when the norm is not finite and left alone otherwise; pass out + 5 of
 * cpc_nce_loss (step indicator and sticky flag) and a non-finite gradient ends the run the way a NaN loss does.
 * g must be 16-byte aligned; workspace: cpc_grad_norm_workspace_floats(n) floats; max_norm finite and > 0. */
long long cpc_grad_norm_workspace_floats(long long n);
int cpc_grad_norm(const float* g, long long n, float grad_scale, float max_norm, float* workspace, float* state, float* nan_pair,
                  void* stream);
/* cpc_adam on the clipped gradient, the optimizer.step() behind torch.nn.utils.clip_grad_norm_: the gradient is
 * (g * grad_scale) * coef[0], multiplied in that order (coef: device pointer to one float, state + 1 of cpc_grad_norm), so
 * that coef[0] == 1 gives cpc_adam's bits wherever g * grad_scale is itself exact (grad_scale 1 or a power of two; cpc_adam
 * contracts that product into its first-moment update, so for other scales the two differ by its rounding).  skip as in
 * cpc_adam (wire nan_pair of cpc_grad_norm to it: a coefficient of 0 alone does not stop inf * 0 from reaching the parameters). */
int cpc_adam_clip(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
                  int step, float grad_scale, const float* coef, const float* skip, void* stream);


/* AdamW and the learning-rate schedule: torch.optim.AdamW's decoupled weight decay in cpc_adam's update, and the factor of a
 * torch.optim.lr_scheduler.LambdaLR (not in the reference's train step, which runs Adam at one constant lr without decay;
 * DESIGN.md, "AdamW and the learning-rate schedule").
 * cpc_adamw: cpc_adam (coef == NULL) or cpc_adam_clip (coef given: the gradient is (g * grad_scale) * coef[0], in that order)
 * with the decay in front: a decayed element does p <- p * decay first, decay = (float)(1 - (double)lr * weight_decay), then
 * the Adam update with the new moments; gradient and moments do not see the decay.  lr is the step's learning rate (the
 * caller has multiplied the schedule's factor in).
 *   decay_bits: device pointer, one bit per 64-float block of the WHOLE flat buffer (parameters start at 64-float boundaries):
 *   bit j % 32 of word j / 32 covers floats [64 j, 64 j + 64); a set bit decays.  p, g, m, v point at the start of block
 *   first_block (a range that begins at float lo passes first_block = lo / 64, lo a multiple of 64); the words up to block
 *   first_block + (n - 1) / 64 are read.  decay_bits may be NULL when weight_decay == 0 (it is not read then).
 * With weight_decay == 0, or on an undecayed block, the results are cpc_adam's bits without coef and cpc_adam_clip's with
 * coef wherever g * grad_scale is exact (grad_scale 1 or a power of two).  skip as in cpc_adam.
 * CPC_EINVAL before any launch: n <= 0, step < 1, weight_decay negative or not finite, weight_decay > 0 with decay_bits NULL,
 * first_block < 0, p, g, m or v NULL. */
int cpc_adamw(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps, int step,
              float grad_scale, float weight_decay, const unsigned* decay_bits, long long first_block, const float* coef,
              const float* skip, void* stream);
/* The same update over the whole buffer (first_block 0) with the step count on the device, as cpc_adam_dev: the argument list
 * never changes from step to step, so the launch can be captured.  A one-thread kernel advances state[0] (unless skip is
 * raised) to the count t and writes, in double, with f = the schedule's factor at step index step_offset + t - 1:
 *   state[1] = lr f / (1 - beta1^t), state[2] = 1 / sqrt(1 - beta2^t), state[3] = 1 - lr f weight_decay;
 * the streaming kernel is cpc_adamw's and reads the three from state.  kind: 0 constant, 1 linear, 2 cosine (see
 * cpc_lr_factors; kind 0 with warmup_steps 0 is a constant lr).  coef must be NULL (clipped steps are not captured).
 * CPC_EINVAL: cpc_adamw's cases, state NULL, coef given, step_offset < 0, an invalid schedule. */
int cpc_adamw_dev(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
                  float* state, float grad_scale, float weight_decay, const unsigned* decay_bits, int kind, long long warmup_steps,
                  long long total_steps, float min_ratio, long long step_offset, const float* coef, const float* skip, void* stream);
/* out[i] = (float) factor(step0 + i), i < count (out: device pointer) — the function cpc_adamw_dev's tick evaluates, in double:
 *   s < warmup_steps: (s + 1) / warmup_steps;  kind 0: 1;  q = min((s - warmup_steps) / (total_steps - warmup_steps), 1);
 *   kind 1: r + (1 - r)(1 - q);  kind 2: r + (1 - r) * 0.5 * (1 + cos(pi q)),  r = min_ratio.
 * CPC_EINVAL: kind outside 0..2, warmup_steps < 0, total_steps <= warmup_steps unless kind 0, min_ratio outside [0, 1] or NaN,
 * step0 < 0, count <= 0, out NULL. */
int cpc_lr_factors(int kind, long long warmup_steps, long long total_steps, float min_ratio, long long step0, int count,
                   float* out, void* stream);


/* LAMB: a layer-wise trust ratio on Adam's direction (You et al., "Large Batch Optimization for Deep Learning"; not in the
 * reference's train step; DESIGN.md, "LAMB trust ratios").  Per step t, for every parameter tensor P of the range, with the gradient
 * g' = g * grad_scale, or (g * grad_scale) * coef[0] when coef is given, in that order as in cpc_adamw:
 *   m  = m + (g' - m)(1 - b1);   v = b2 v + (1 - b2) g'^2                 cpc_adam's moments, unchanged
 *   r  = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps)                          Adam's direction; bc1 = 1 - b1^t, bc2 = 1 - b2^t
 *   u  = r + weight_decay * p   if P is selected, else  u = r             the decay is part of the direction (not AdamW's multiply)
 *   w_norm = ||p||_2, u_norm = ||u||_2 over P's blocks (its alignment padding is zero and stays zero)
 *   trust  = w_norm / u_norm    if P is selected and both norms are finite and > 0, else 1
 *   trust  = min(trust, trust_clip)                                       if trust_clip >= 0 (a negative value: no clip)
 *   p  <- p - lr * trust * u                                              lr: the step's rate, schedule factor multiplied in
 * select_bits: cpc_adamw's bitmap (one bit per 64-float block of the whole buffer); it selects decay AND trust ratio and is required
 * also with weight_decay == 0.  The range [p, p + n) is a run of whole parameters, which start at 64-float boundaries:
 *   param_block      HOST pointer, int32[total_params + 1], ascending: parameter q covers blocks [param_block[q], param_block[q + 1])
 *                    of the whole buffer, its padding included (0 ... total blocks); read during the call, to check the range;
 *   param_block_dev  the same table in device memory;
 *   block_param      device int32[total blocks]: the parameter a block belongs to (the inverse of the table);
 *   first_param, n_params: the range is parameters first_param ... first_param + n_params - 1, first_block = param_block[first_param],
 *                    n = 64 * (param_block[first_param + n_params] - first_block);
 *   workspace        device, 8-byte aligned, cpc_lamb_workspace_floats(total blocks) floats: the sums of p^2 and u^2 of block j at
 *                    [2 j], [2 j + 1], written and read as one 8-byte pair;
 *   trust            device f32[3][total_params]: w_norm, u_norm and the ratio applied, written for the range's parameters.
 * Three launches: moments and block sums; one workgroup per parameter for the ratios; the update (u is formed again from the new
 * m, v and the old p — nothing is parked in g).  All sums are float32 in a fixed order without atomics: the same data give the same
 * bits for any split of the buffer into ranges.  skip as in cpc_adam: while *skip != 0, p, m, v, workspace and trust keep their bits.
 * CPC_EINVAL before any launch: cpc_adamw's cases; select_bits, param_block, param_block_dev, block_param, workspace or trust NULL;
 * a workspace that is not 8-byte aligned;
 * n_params <= 0, first_param < 0 or first_param + n_params > total_params; a table that descends inside the range, whose
 * param_block[first_param] is not first_block, or that gives the range another size than n; trust_clip >= 0 (given) but not finite
 * and > 0. */
long long cpc_lamb_workspace_floats(long long total_blocks);
int cpc_lamb(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps, int step,
             float grad_scale, float weight_decay, const unsigned* select_bits, long long first_block, const float* coef,
             const int* param_block, const int* param_block_dev, const int* block_param, int first_param, int n_params,
             int total_params, float trust_clip, float* workspace, float* trust, const float* skip, void* stream);


/* Exponential moving average (EMA) of the weights behind an optimizer update (not in the reference's train step; DESIGN.md, "EMA of
 * the weights").  For every i in [0, n):
 *   ema[i] = ema[i] + (p[i] - ema[i]) * w,   w = 1 - d
 *   d = decay                                 when warmup == 0
 *   d = min(decay, (1 + t) / (10 + t))        otherwise; t is the 1-based number of the update being averaged.
 * One float32 rounding for the difference and one for the fused product and sum; w == 1 (decay 0) stores p[i] itself.  The same data
 * give the same bits for any split of the buffer into ranges that start at multiples of four floats.
 *   state == NULL (host route): t = step, step >= 1; w is formed in double and rounded once to float.
 *   state != NULL (device route): state is the f32[4] of cpc_adam_dev / cpc_adamw_dev, t the int whose bits are in state[0], which
 *     that call has already advanced; step is ignored.  Every thread forms w = max(1 - decay, 9 / (10 + t)) in float (the same
 *     number, at most one unit in the last place of w from the host route's).  No argument changes from step to step, so the launch
 *     can be captured behind cpc_adam_dev.
 *   skip as in cpc_adam: while *skip != 0 the call changes nothing.
 * p is read with plain loads, ema is read and written non-temporally (it is touched once per step).  One launch, no scratch memory,
 * no atomics.  CPC_EINVAL before any launch: p or ema NULL, n <= 0, p or ema not 16-byte aligned, decay outside [0, 1) or not
 * finite, step < 1 on the host route.
 * cpc_ema_swap exchanges p[i] and ema[i] for every i in [0, n) in one pass (the averaged weights go into the model and the raw ones
 * are parked in ema; a second call restores both).  CPC_EINVAL: p or ema NULL, n <= 0, p or ema not 16-byte aligned.  p and ema must
 * not overlap, in either call. */
int cpc_ema(const float* p, float* ema, long long n, float decay, int warmup, int step, const float* state, const float* skip,
            void* stream);
int cpc_ema_swap(float* p, float* ema, long long n, void* stream);


/* Waveform augmentation in the time domain (not in the reference; DESIGN.md, "Waveform augmentation"): speed change, time drop,
 * additive noise, gain and polarity on the first protect_from samples of every clip of an f32 batch x[B][ldx] (L valid samples per
 * row), written to a separate buffer y[B][ldy]; x and y must not overlap.
 *
 * Randomness is counter-based, with the arithmetic of the sampled negatives (modulo 2^64):
 *   mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31)
 *   kb   = mix(seed + 0x632BE59BD9B4E019 * step + 0x9E3779B97F4A7C15 * (clip + 1)),  clip = clip_offset + b
 *   u_f  = mix(kb + 0xD1B54A32D192ED03 * f) >> 32                        field f of a clip, a u32
 *   integer draw in [lo, hi]:  lo + ((u_f * (hi - lo + 1)) >> 32)        (64-bit product)
 *   real draw in [lo, hi]:     fma(hi - lo, float(u_f) * 2^-32, lo)      (f32)
 * a = protect_from.  Samples n >= a are copied bit for bit; every stage acts on n < a, in this order, and a stage that is off
 * performs no arithmetic on the samples (all off: y == x bitwise).  With a == 0 nothing is drawn: q = 65536, no span, sigma = 0.
 *   speed     (field 1)  q in [q_lo, q_hi], Q16; q_lo == q_hi == 65536 is off.  pos = a * 65536 - (a - n) * q (64-bit integers),
 *             i = pos >> 16 (floor), t = (pos & 0xFFFF) * 2^-16, v = sum_j w_j(t) x[i + j], j = -1 .. 2, x = 0 outside [0, L), with
 *             the Catmull-Rom weights w_-1 = ((-t + 2) t - 1) t / 2, w_0 = ((3 t - 5) t^2 + 2) / 2, w_1 = ((-3 t + 4) t + 1) t / 2,
 *             w_2 = (t - 1) t^2 / 2, evaluated in the factored forms -t u^2 / 2, u (2 + t (2 - 3 t)) / 2, t (1 + t (4 - 3 t)) / 2,
 *             -u t^2 / 2 with u = 1 - t (no cancellation: every weight carries at most two roundings), and summed as one
 *             multiply and three fmas, j ascending.  No low-pass filter in front of a speed-up: meant for |q / 65536 - 1| <= 0.25.
 *   time drop (fields 8 + 2 d and 9 + 2 d, d < drop_count <= 8)  len_d in [1, min(drop_max_len, a)] from field 8 + 2 d, start_d in
 *             [0, a - len_d] from field 9 + 2 d; v = 0.0f for n in [start_d, start_d + len_d).  Spans may overlap.
 *   noise     (field 2)  snr_db in [snr_lo, snr_hi], sigma = sqrtf(P) * exp2f(-snr_db * (log2(10) / 20)), P = (sum of partial[b][.]
 *             in index order) / float(a): the mean square of the ORIGINAL x[b][0 .. a) as cpc_wave_power left it.
 *             v = fma(sigma, g(n), v), g(n) = float(s - 131070) * float(sqrt(3) / 65536), s = the sum of the four 16-bit fields of
 *             mix(kb + 0xD1B54A32D192ED03 * (32 + n)): mean 0, variance 1, |g| <= 3.47.  Dropped spans hold noise only.
 *   gain      (field 3)  db in [gain_lo_db, gain_hi_db], gain = exp2f(db * (log2(10) / 20)); v = v * gain.
 *   polarity  (field 4)  the sign flips when u_4 < polarity_threshold (probability * 2^32; 0 = off, 2^32 = always): with the gain
 *             on, v = v * (-gain); with it off, v = -v.
 * cpc_wave_power: partial[b][c] = the sum of squares of x[b][4096 c .. min(4096 (c + 1), n)), c < cpc_wave_power_chunks(n) =
 *   ceil(n / 4096) (0 for n < 1), rows of partial that many floats apart.  One workgroup per (b, c); thread t of 256 runs one fma
 *   chain over elements 4 (256 p + t) + j, p = 0 .. 3 outer, j = 0 .. 3 inner, then an xor-shuffle butterfly over the wave and
 *   (w0 + w1) + (w2 + w3) over the four waves: one fixed order whatever the alignment of the rows, no atomics.
 *   CPC_EINVAL: x or partial NULL, B outside [1, 65535], L outside [1, 2^24], ldx < L, n outside [1, L].
 * cpc_wave_augment: one launch (after cpc_wave_power(x, partial, B, L, ldx, protect_from) where the noise is on and
 *   protect_from >= 1).  params_out NULL or f32 [B][8]: per clip q, sigma, the signed gain, P, start_0, len_0, start_1, len_1 as the
 *   device drew them (0 for what is off or not drawn, gain +-1 with the gain off; integers up to 2^24 are exact in f32).  16-byte
 *   loads / stores where the row starts and leading dimensions allow, scalar ones otherwise; the same bits either way.
 *   CPC_EINVAL before any launch: x, y or cfg NULL, partial NULL with noise_on, B outside [1, 65535], L outside [1, 2^24], ldx < L or
 *   ldy < L, protect_from outside [0, L], not 32768 <= q_lo <= q_hi <= 131072, drop_count outside [0, 8], drop_max_len < 1 with
 *   drop_count > 0, snr_lo > snr_hi or either not finite with noise_on, gain_lo_db > gain_hi_db or either not finite with gain_on,
 *   polarity_threshold > 2^32.
 * Neither call throws, allocates or synchronises. */
typedef struct cpc_wave_augment_cfg {
    unsigned long long seed, step, clip_offset;
    int protect_from;
    int q_lo, q_hi;
    int drop_count, drop_max_len;
    int noise_on; float snr_lo, snr_hi;
    int gain_on; float gain_lo_db, gain_hi_db;
    unsigned long long polarity_threshold;
} CpcWaveAugment;
int cpc_wave_power_chunks(int n);
int cpc_wave_power(const float* x, float* partial, int B, int L, long long ldx, int n, void* stream);
int cpc_wave_augment(const float* x, float* y, const float* partial, float* params_out, int B, int L, long long ldx, long long ldy,
                     const CpcWaveAugment* cfg, void* stream);


/* Log-mel front end (not in the reference; DESIGN.md, "Log-mel front end"): what follows the framed, windowed DFT, which is one
 * cpc_gemm_nt over overlapped waveform rows.
 *   spec  f32 [B][Tn][lds], (re, im) interleaved per bin k < n_freq; elements at or beyond 2 n_freq of a row are never read.
 *   out   f32 [B][W][n_mels][Cc], (W, Cc) = (Tn - 1, 2) with delta, (Tn, 1) without (channels-last; the scalogram engine's input grid).
 *   p[t][k] = fl(fl(re^2) + fl(im^2)); band m: M[t][m] = the f32 fma chain acc = fmaf(band_w[band_off[m] + j], p[t][band_lo[m] + j], acc)
 *   from acc = 0 over j = 0 .. band_n[m] - 1 ascending, the range clamped to bins [0, n_freq) (a wrong table reads no other part of
 *   spec; band_w must hold band_off[m] + band_n[m] floats).  No atomics; the same bits from run to run, whatever the grid.
 *   take_log = 0: out = M (delta must be 0).  take_log = 1: l = logf(M + log_offset);
 *     delta = 0: out[b][t][m] = scaling * l[t][m];
 *     delta = 1: out[b][w][m] = (scaling * l[w + 1][m], delta_scaling * (l[w + 1][m] - l[w][m])).
 *   A spectrum row is read once, plus one row per run of 31 / 15 / 7 output frames with delta (n_freq <= 1025 / <= 2049 / above).
 *   A weight table of at most 2 n_freq floats (every bank of triangles) is kept in LDS; a longer one is read from global memory.
 *   CPC_EINVAL before any launch: a NULL pointer; B, Tn or n_mels < 1; Tn < 2 with delta; n_freq outside [2, 4097]; n_mels > 1024;
 *   lds < 2 n_freq or odd; delta or take_log outside {0, 1}; take_log = 0 with delta = 1; log_offset not finite or <= 0 with take_log;
 *   scaling or delta_scaling not finite; spec not 8-byte aligned, or out not 8-byte aligned with delta.  stream is a hipStream_t.
 *   Does not throw, allocate or synchronise. */
int cpc_mel_pointwise(const float* spec, long long lds, const int* band_lo, const int* band_n, const int* band_off, const float* band_w,
                      float* out, int B, int Tn, int n_freq, int n_mels, int delta, int take_log, float log_offset, float scaling,
                      float delta_scaling, void* stream);


/* Masking augmentation on the input grid of the scalogram engine (not in the reference; DESIGN.md, "Grid masking"; after SpecAugment,
 * Park et al. 2019): frequency bands and time spans of every clip are filled with zero, a constant or the clip's own mean.
 *   Grid: x is f32; clip b starts at x + b ldb, ldb >= W H Cc; element (t, h, c) of a clip (frame t < W, bin h < H, channel c < Cc) is at
 *   (t H + h) Cc + c — the channels-last buffer the scalogram and the log-mel front end write.  Cc is 1, 2 or 4.
 *   Wa = W - protect_last: frames t >= Wa are never changed.  With Wa == 0 nothing is drawn and cpc_grid_mask is the identity.
 * Randomness: mix, kb = kb(seed, step, clip_offset + b), the integer draw and u_f are those of cpc_wave_augment above; the mask fields are
 *   f = 0x4D41534B + j.  No field of the waveform augmentation (f < 32) and no noise index (32 + n, n < 2^24) reaches that value, so a
 *   waveform augmentation and a mask with the same seed are independent.
 *   frequency mask d < freq_count <= 8:  w_d in [0, min(freq_max, H)] from j = 2 d, f0_d in [0, H - w_d] from j = 2 d + 1; the cells
 *             h in [f0_d, f0_d + w_d) of every frame t < Wa are masked.
 *   time mask d < time_count <= 8:  w_d in [0, time_cap] from j = 16 + 2 d, t0_d in [0, Wa - w_d] from j = 17 + 2 d; all H Cc values of
 *             the frames [t0_d, t0_d + w_d) are masked.  time_cap = min(time_max, floor(time_fraction Wa), Wa) is formed by the caller.
 *   Masks may overlap.  A masked value of channel c becomes fill[c]: 0.0f (fill_mode 0), fill_value (1), or mean[b][c] (2), the mean of
 *   channel c over all W H cells of the ORIGINAL clip: (sum over chunk of partial[b][chunk][c], in index order) / float(W H), formed in
 *   the kernel from what cpc_grid_sum left.
 * cpc_grid_sum: partial[b][k][c] (f32 [B][cpc_grid_sum_chunks(n)][Cc]) = the sum of channel c over the elements [4096 k,
 *   min(4096 (k + 1), n)) of clip b, n = W H Cc, cpc_grid_sum_chunks(n) = ceil(n / 4096) (0 for n < 1).  Element e holds channel e % Cc,
 *   and 4 % Cc == 0, so position j of every aligned piece of four holds channel j % Cc.  One workgroup per (b, k).  Thread t of 256:
 *   a_j = the chain ((x[e_0j] + x[e_1j]) + x[e_2j]) + x[e_3j] over e_pj = 4096 k + 4 (256 p + t) + j, p = 0 .. 3 (elements at or behind n
 *   count as 0), for j = 0 .. 3; then the positions of one channel: Cc = 4: s_c = a_c; Cc = 2: s_c = a_c + a_(c + 2); Cc = 1:
 *   s_0 = (a_0 + a_1) + (a_2 + a_3); then an xor-shuffle butterfly over the wave (offsets 32, 16, .. 1) and (w0 + w1) + (w2 + w3) over
 *   the four waves.  One fixed order whatever the alignment of the clips, no atomics.  A partial carries at most 3 + log2(4 / Cc) + 6 +
 *   2 = 13 / 12 / 11 roundings (Cc = 1 / 2 / 4) along any path from an element to the result.
 *   CPC_EINVAL: x or partial NULL, B outside [1, 65535], Cc not in {1, 2, 4}, n < 1 or not a multiple of Cc, ldb < n.
 * cpc_grid_mask: one launch (after cpc_grid_sum(x, partial, B, W H Cc, ldbx, Cc) with fill_mode 2).
 *   y != x: y receives the masked copy in one sweep, x is never written and elements that are not masked are copied bit for bit;
 *     16-byte loads / stores where x / y and ldbx / ldby allow (16-byte aligned, a multiple of 4), scalar ones otherwise.
 *   y == x (ldby == ldbx), in place: the kernel is LAUNCHED OVER THE MASK RECTANGLES (one grid row of workgroups per drawn mask and
 *     clip, sized by the widest mask the configuration can draw; there is no sweep over the grid): only masked cells are written and
 *     no grid element is read.  A run of masked elements is stored in the pieces of four elements that start at multiples of 4 from
 *     the clip's start: 16-byte stores for pieces inside the run where y and ldby allow, scalar stores for the run's ends and otherwise.
 *     With no mask to draw and spans_out == fill_out == NULL nothing is launched.
 *   The bits are the same whichever loads and stores are used.
 *   spans_out NULL or int32 [B][32]: eight (f0, w) pairs, then eight (t0, w) pairs, 0 where not drawn.  fill_out NULL or f32 [B][4]: the
 *   fill value per channel as used (0 for c >= Cc).
 *   CPC_EINVAL before any launch: x, y or cfg NULL, partial NULL with fill_mode 2, B outside [1, 65535], W or H < 1, Cc not in
 *   {1, 2, 4}, W H Cc > 2^31 - 1, ldbx or ldby < W H Cc, protect_last outside [0, W], freq_count or time_count outside [0, 8],
 *   freq_max < 0, time_cap outside [0, Wa], fill_mode outside {0, 1, 2}, fill_value not finite with fill_mode 1, x != y with
 *   overlapping clip ranges [x, x + (B - 1) ldbx + W H Cc) and [y, ..), x == y with ldbx != ldby.
 * The calls never throw, allocate or synchronise.  stream is a hipStream_t. */
typedef struct cpc_grid_mask_cfg {
    unsigned long long seed, step, clip_offset;
    int protect_last;
    int freq_count, freq_max;
    int time_count, time_cap;
    int fill_mode; float fill_value;
} CpcGridMask;
int cpc_grid_sum_chunks(int n);
int cpc_grid_sum(const float* x, float* partial, int B, int n, long long ldb, int Cc, void* stream);
int cpc_grid_mask(const float* x, float* y, const float* partial, int* spans_out, float* fill_out, int B, int W, int H, int Cc,
                  long long ldbx, long long ldby, const CpcGridMask* cfg, void* stream);

/* ---- Device-resident audio dataset: a batch of windows cut from the concatenated samples (csrc/dataset.hip; DESIGN.md,
 * "Device-resident audio dataset").
 * cpc_window_gather: out[b ldo + t] = scale * float(store[starts[idx[b]] + t]) for b < B, t < L, in one launch.
 *   store: the samples of every file, one after the other, store_len of them; store_code 0: f32, 1: int16.
 *   starts: int64 [n_items], the first sample of example i (a device table the dataset builds once).  idx: int64 [B], the example of
 *   row b; an example may stand in several rows.  out: f32, rows ldo >= L apart; nothing is written between the rows or behind
 *   the last one.
 *   A f32 store with scale == 1.0f is copied bit for bit.  An int16 sample times scale = 1 / 32768 is exact in f32.
 *   Guard: the kernel forms no address outside [store, store + store_len).  A row whose idx[b] is outside [0, n_items), or whose
 *   window [starts[idx[b]], + L) is not inside [0, store_len], is written as L zeros; callers rule such rows out on the host, the
 *   guard keeps a wrong index from becoming a fault.
 *   Access: grid row b is output row b, a lane moves pieces of four consecutive samples; 16-byte stores where out is 16-byte aligned
 *   and ldo a multiple of 4, scalar stores otherwise and for the last piece of a row whose L is no multiple of 4.  The source of a
 *   piece is aligned to one sample only (the window starts anywhere).  The grid is sized from B L: workgroups of 4096, 1024 or 256
 *   outputs, the largest that still gives 1024 workgroups.  The bits do not depend on any of this.
 *   CPC_EINVAL before any launch: store, starts, idx or out NULL, B outside [1, 65535], L outside [1, 2^24], ldo < L, store_len < L,
 *   n_items < 1, store_code outside {0, 1}, scale not finite, store not aligned to its element size, out not 4-byte aligned.
 * The call never throws, allocates or synchronises.  stream is a hipStream_t. */
int cpc_window_gather(const void* store, int store_code, long long store_len, const long long* starts, long long n_items,
                      const long long* idx, float* out, int B, int L, long long ldo, float scale, void* stream);

/* ---- Load-time conversion: channel downmix, rational resampling and the f32 / int16 store for a list of segments (files) in one
 * launch (csrc/resample.hip; DESIGN.md, "Resampling and downmix at load").
 * cpc_resample: for every segment s with N = segs[4 s + 1] source frames and every n < segs[4 s + 3],
 *     x[i]  = in_scale * (mix == 0 ? f[i][0] : (f[i][0] + ... + f[i][C - 1]) / C)   for 0 <= i < N, 0 otherwise
 *     y[n]  = sum_{t = 0 .. 2 W} taps[t L + p] * x[i0 + t - W],   i0 = (n M) div L,  p = (n M) mod L
 *     dst[segs[4 s + 2] + n] = out_scale * y[n]
 *   where f[i][c] = src[(segs[4 s] + i) C + c].  The channel sum runs in channel order in f32; the sum over t runs in t order in f32.
 *   Frames outside [0, N) of the segment count as zero: no sample of a neighbouring segment enters.
 *   src: interleaved frames of C channels, src_frames_total of them, the segments back to back or apart; src_code 0: f32, 1: int16.
 *   dst: dst_total elements; dst_code 0: f32, 1: int16.  The int16 store writes the same f32 value out_scale * y[n], rounded half to
 *   even and saturated to [-32768, 32767]; both stores form that value by the same operations.
 *   taps: f32 [2 W + 1][L], the TRANSPOSE of the L x (2 W + 1) polyphase table the caller designs (taps[t L + p] is the table's
 *   [p][t]); the kernel knows nothing of windows or cut-offs.  W = 0, L = M = 1, taps = {1} is the identity: downmix and convert only.
 *   segs: int64 [nseg][4] on the device: first source frame, source frames, first output, output count (ceil(N L / M) for a whole
 *   file; any count is served, outputs whose taps lie behind the segment read zeros).  tile_first: int64 [nseg] on the device, the
 *   first tile of segment s when every segment is cut into tiles of CPC_RESAMPLE_TILE outputs, tile_first[0] = 0, non-decreasing;
 *   ntiles: their total, the grid.  A workgroup finds its segment by a uniform search in tile_first.
 *   Guard: the kernel forms no address outside [src, src + src_frames_total C) or [dst, dst + dst_total).  A segment whose entries
 *   leave [0, src_frames_total] or [0, dst_total], or are negative, is skipped: nothing of it is read or written; a tile that a wrong
 *   tile_first places outside its segment is skipped too.  Callers build right tables; the guard keeps a wrong one from becoming a
 *   fault.
 *   Access: a workgroup of 256 lanes stages the downmixed span of its tile, at most (CPC_RESAMPLE_TILE - 1) M div L + 2 W + 2 floats,
 *   in LDS once; a lane makes four outputs 256 apart; stores are one element per lane, consecutive lanes consecutive outputs.
 *   CPC_EINVAL before any launch: src, taps, segs, tile_first or dst NULL, C outside [1, 8], mix, src_code or dst_code outside {0, 1},
 *   L or M outside [1, 2^20], W < 0, L (2 W + 1) > 2^24, the span above > 16384 floats (64 KiB of LDS), nseg < 1, ntiles outside
 *   [1, 2^23], src_frames_total or dst_total outside [1, 2^40], in_scale or out_scale not finite, src or dst not aligned to its
 *   element size, taps not 4-byte aligned, segs or tile_first not 8-byte aligned.
 * The call never throws, allocates or synchronises.  stream is a hipStream_t. */
#define CPC_RESAMPLE_TILE 1024
int cpc_resample(const void* src, int src_code, long long src_frames_total, int C, int mix, float in_scale, const float* taps, int L,
                 int M, int W, const long long* segs, const long long* tile_first, int nseg, long long ntiles, void* dst, int dst_code,
                 long long dst_total, float out_scale, void* stream);

/* ---- Whole-recording feature extraction: z and c of every frame of every recording, in chunks (csrc/stream.hip; DESIGN.md,
 * "Whole-recording feature extraction").  R recordings ("streams") advance side by side, Tc frames per step.  The host lays out every
 * step up front as an int64 table [n_steps][R][6] on the device; each of the three calls of step j is given block j, `table`, whose
 * row r says what stream r does in that step:
 *     [0] first_sample   first sample of the step's window in the store
 *     [1] n_samples      samples of the window, (n_frames - 1) downsampling + receptive field, or 0
 *     [2] n_frames       frames the step makes for the recording, at most Tc
 *     [3] out_row        row of the feature stores that takes the first of them
 *     [4] rec            the recording, 0 <= rec < n_rec, or -1: an idle row
 *     [5] keep           1: the stream's next step continues this recording
 * GUARD (all three calls; the extents are arguments of each): a row with rec outside [0, n_rec), n_samples outside [0, L], a window
 * [first_sample, + n_samples) that is not inside [0, store_len], n_frames outside [0, Tc] or rows [out_row, + n_frames) that are not
 * inside [0, total_frames] is treated as idle: nothing of it is read, nothing is written for it beyond what an idle row gets (zeros
 * from cpc_stream_gather and cpc_stream_carry, nothing from cpc_feature_emit).  No address outside the stated extents is formed.
 * Callers build right tables; the guard keeps a wrong one from becoming a fault.  One thing the guard cannot see is left to the
 * caller: within one block no two rows name the same recording (cpc_feature_emit's accumulators are added to without atomics).
 *
 * cpc_stream_gather: out[r ldo + t] = scale * float(store[first_sample + t]) for t < n_samples, exact zeros for n_samples <= t < L;
 *   an idle row is L zeros.  store, store_code, scale, the unaligned source / aligned destination access and the bit-exactness rules
 *   (an f32 store with scale == 1.0f is copied bit for bit; int16 times 1 / 32768 is exact) are cpc_window_gather's.  Nothing is
 *   written between the rows or behind the last one.
 *   CPC_EINVAL before any launch: store, table or out NULL, R outside [1, 65535], L outside [1, 2^24], ldo < L, store_len < 1,
 *   Tc < 1, total_frames < 0, n_rec < 1, store_code outside {0, 1}, scale not finite, store not aligned to its element size, out
 *   not 4-byte aligned, table not 8-byte aligned.
 *
 * cpc_feature_emit: for every row that is not idle and every t < n_frames
 *     z_out[(out_row + t) E + e] = (U) top [r top_item  + t E + e]          e < E   (the encoder's top rows of the stream)
 *     c_out[(out_row + t) H + h] = (U) hall[r hall_item + (t + 1) H + h]    h < H   (row 0 of a stream's hidden states is the state
 *                                                                                    the step started from, row t + 1 the one after frame t)
 *   top, hall: the storage type src_dtype; z_out, c_out: out_dtype (CPC_F32 / CPC_BF16).  Equal types are copied bit for bit, f32 to
 *   bf16 rounds to nearest even, bf16 to f32 is exact.  z_out or c_out may be NULL: that kind is then neither read nor written (top /
 *   hall may be NULL with it).  Nothing but those rows is written.
 *   Pooling (partial != NULL): acc_z f64 [n_rec][2][E] and acc_c f64 [n_rec][2][H] (required for the kinds given) gain, for the row's
 *   recording and every channel, the sum (row 0) and the sum of squares (row 1) over the step's frames of the source values widened
 *   to f32.  partial: f64 scratch of R ceil(Tc / CPC_EMIT_FRAMES) 2 (E + H) elements, rewritten by every call.  A first launch leaves
 *   per (stream, block of CPC_EMIT_FRAMES frames, channel) the sums taken in frame order; a second adds the blocks of a stream to
 *   the accumulators in block order.  Every addition is in f64 and every square is exact (an f32 value squared has 48 bits): squares
 *   rounded to f32 would cost sqrt(E[x^2] - mean^2) half its digits.  No atomics: the order of every sum is fixed by the arguments, so a call sequence gives
 *   the same bits every time.  The caller zeroes the accumulators before the first step and turns them into mean and deviation after
 *   the last.
 *   Access: grid row r is stream r; a lane moves 16 bytes of a source row (4 f32 / 8 bf16 channels), neighbouring lanes neighbouring
 *   pieces, and walks the CPC_EMIT_FRAMES frames of its block.
 *   CPC_EINVAL before any launch: table NULL, z_out and c_out both NULL, z_out without top or c_out without hall, src_dtype or
 *   out_dtype outside {CPC_F32, CPC_BF16}, R outside [1, 65535], Tc outside [1, 2^20], E (with z_out) or H (with c_out) outside
 *   [ch, 65536] or, given at all, negative or no multiple of ch = 4 (f32) / 8 (bf16) source elements, top_item < Tc E or hall_item <
 *   (Tc + 1) H or either no multiple of ch, L outside [1, 2^24], store_len < 1, total_frames < 0, n_rec < 1, a pointer of top, hall,
 *   z_out, c_out or partial that is not 16-byte aligned, an accumulator that is missing with partial or not 8-byte aligned, table
 *   not 8-byte aligned.
 *
 * cpc_stream_carry: dst[i][r H + h] = keep(r) ? src[i][r H + h] : 0 for i < nstate state arrays f32 [R][H] (a GRU's c_out of every
 *   layer; an LSTM's h_out and cell_out), keep(r) = row r is not idle and its entry [5] is 1.  src, dst: HOST arrays of nstate device
 *   pointers, read by the call.  dst is the next step's h0 / c0 and never a buffer the recurrence writes; this is the only place
 *   where a stream's state is reset: the state a recording's last, short chunk leaves behind, computed on zero-filled samples, goes
 *   no further.
 *   CPC_EINVAL before any launch: table, src or dst NULL, nstate outside [1, CPC_STREAM_MAX_STATES], an array pointer NULL or not
 *   16-byte aligned, a dst that is also a src, R outside [1, 65535], H outside [4, 65536] or no multiple of 4, L outside [1, 2^24],
 *   store_len < 1, Tc < 1, total_frames < 0, n_rec < 1, table not 8-byte aligned.
 * The calls never throw, allocate or synchronise.  stream is a hipStream_t.  (Added under ABI 9: no existing entry point changed.) */
#define CPC_EMIT_FRAMES 32
#define CPC_STREAM_MAX_STATES 8
int cpc_stream_gather(const void* store, int store_code, long long store_len, const long long* table, float* out, int R, int L,
                      long long ldo, float scale, int Tc, long long total_frames, int n_rec, void* stream);
int cpc_feature_emit(const long long* table, const void* top, long long top_item, const void* hall, long long hall_item, int src_dtype,
                     void* z_out, void* c_out, int out_dtype, int R, int Tc, int E, int H, long long store_len, int L,
                     long long total_frames, int n_rec, double* partial, double* acc_z, double* acc_c, void* stream);
int cpc_stream_carry(const long long* table, const float* const* src, float* const* dst, int nstate, int R, int H, long long store_len,
                     int L, int Tc, long long total_frames, int n_rec, void* stream);

/* ---- K-means units over feature rows (csrc/kmeans.hip; DESIGN.md, "K-means units").  x: N rows of D values of the storage type
 * dtype (CPC_F32 / CPC_BF16) at a row stride of ldx >= D elements; centers f32 [K][D]; cnorm f32 [K], the squared norms of the centres.
 * Shared limits, CPC_EINVAL before any launch otherwise: x NULL or not 16-byte aligned, dtype outside {CPC_F32, CPC_BF16}, N outside
 * [1, 2^31 - 1], D outside [16, 512] or no multiple of 16, K outside [2, 1024], ldx < D or no multiple of 4 (f32) / 8 (bf16) elements
 * (rows are read 16 bytes at a time).  Offsets that grow with N ldx are 64-bit.
 *
 * cpc_kmeans_assign: labels[n] = the k with the smallest v(n, k) = cnorm[k] - 2 x_n . c_k, the lowest such k where several compare
 *   equal as the kernel computes them; dist[n] = max(v(n, labels[n]) + |x_n|^2, 0) with |x_n|^2 computed by the kernel; dist may be
 *   NULL and is then not written.  All arithmetic is f32: bf16 rows are widened (exact), centres are never rounded, x_n . c_k is an
 *   f32-input MFMA chain (one rounding per product, as an fmaf chain in a fixed order of the columns), v one more fmaf.  A row
 *   holding a NaN or an infinity gets the label -1 and the distance NaN; no other row is touched by it.  The N x K values v exist in
 *   registers only: the call writes the N labels and, if asked, the N distances, nothing else.
 *   CPC_EINVAL also for centers, cnorm or labels NULL, centers not 16-byte aligned, cnorm, labels or dist not 4-byte aligned.
 *
 * cpc_kmeans_update: from x, labels int32 [N] and the old centres,
 *     counts[k]        int32, the rows with label k
 *     centers_new[k]   f32 [D], their mean (an f64 sum rounded once), or centers_old[k] bit for bit where counts[k] == 0
 *     cnorm[k]         f32, |centers_new[k]|^2 (an f64 sum of exact squares, rounded once; cpc_kmeans_cnorm gives the same bits)
 *     *inertia         f64, the sum of dist[n] over the rows with a label in [0, K)      (dist and inertia: both given or both NULL)
 *   A label outside [0, K), -1 included, is skipped: no address is formed from it.  centers_new may be centers_old itself.
 *   Determinism: the rows are sorted by label with a stable counting sort (integer atomics in LDS for the histograms only), each
 *   cluster's rows are summed in pieces of a fixed length and the pieces are added in order; every floating-point sum is f64 and its
 *   order is fixed by (N, K, D) and the labels.  Two calls on the same inputs give the same bits.
 *   scratch: cpc_kmeans_scratch_bytes(N, K, D) bytes, 16-byte aligned, rewritten by every call.
 *   CPC_EINVAL also for labels, centers_old, scratch, centers_new, cnorm or counts NULL, one of dist / inertia without the other,
 *   scratch_bytes below cpc_kmeans_scratch_bytes(N, K, D), scratch not 16-byte aligned, inertia not 8-byte aligned, another pointer
 *   not 4-byte aligned.
 *
 * cpc_kmeans_scratch_bytes: the scratch size for (N, K, D), or CPC_EINVAL for a shape outside the limits above.
 * cpc_kmeans_cnorm: cnorm[k] = |centers[k]|^2 as cpc_kmeans_update computes it (for an initial codebook).  CPC_EINVAL for a NULL or
 *   misaligned pointer, D or K outside the limits.
 * The calls never throw, allocate or synchronise.  stream is a hipStream_t.  (Added under ABI 9: no existing entry point changed.) */
int cpc_kmeans_assign(const void* x, int dtype, long long N, int D, long long ldx, const float* centers, const float* cnorm, int K,
                      int* labels, float* dist, void* stream);
long long cpc_kmeans_scratch_bytes(long long N, int K, int D);
int cpc_kmeans_update(const void* x, int dtype, long long N, int D, long long ldx, const int* labels, const float* dist,
                      const float* centers_old, int K, void* scratch, long long scratch_bytes, float* centers_new, float* cnorm,
                      int* counts, double* inertia, void* stream);
int cpc_kmeans_cnorm(const float* centers, float* cnorm, int K, int D, void* stream);

/* ---- ABX discriminability: frame distances, batched DTW and the triple count (csrc/dtw.hip; DESIGN.md, "ABX discriminability").
 * x is the feature store as the k-means calls take it: N rows of D values of the storage type dtype at a row stride of ldx >= D
 * elements.  Shared limits, CPC_EINVAL before any launch otherwise: x NULL or not 16-byte aligned, dtype outside {CPC_F32, CPC_BF16},
 * N outside [1, 2^31 - 1], D outside [16, 512] or no multiple of 16, ldx < D or no multiple of 4 (f32) / 8 (bf16) elements, metric
 * outside {0, 1, 2}.  Offsets that grow with N ldx or with P are 64-bit.
 *
 * The frame distance of two rows a, b.  All arithmetic is f32, bf16 rows are widened (exact).  dot = a . b is an f32-input MFMA chain:
 * an fmaf chain, one rounding per product, over the columns in the order (8 s + e, 8 s + 4 + e) for s = 0 .. D/8 - 1, e = 0 .. 3.
 * |a|^2 (and |b|^2) = S0 + S1, S0 the fmaf chain over the columns 8 s + e and S1 the one over the columns 8 s + 4 + e, in ascending
 * order each.  None of these orders depends on where the rows sit in a tile, on La, Lb or P.
 *     metric 0 (angular)            acosf(cos) / (float)pi          cos = clamp(dot / (sqrtf(|a|^2) sqrtf(|b|^2)), -1, 1)
 *     metric 1 (cosine)             1 - cos
 *     metric 2 (squared Euclidean)  max(fmaf(-2, dot, |a|^2 + |b|^2), 0)
 * cpc_dtw uses, for every cell, exactly the bits cpc_frame_distance writes for the same two rows: one device function forms both.
 *
 * cpc_frame_distance: out[i * ldo + j] (f32) = the distance of row a_first + i to row b_first + j, 0 <= i < La, 0 <= j < Lb.
 *   It is there for inspection and applies no rule for bad rows: where a row holds a NaN or an infinity, overflows its squared norm or
 *   (metrics 0 and 1) has the norm 0, the cells of that row hold whatever the f32 arithmetic above gives (a NaN from 0 / 0, a clamped
 *   value), and cpc_dtw does not use them.  CPC_EINVAL also for La or Lb outside [1, 128], a segment outside [0, N), out NULL or not
 *   4-byte aligned, ldo < Lb.
 *
 * cpc_dtw: pairs int64 [P][4] = (a_first, La, b_first, Lb) on the device; with d[i][j] the frame distance of row a_first + i to row
 *   b_first + j,
 *     C[0][0] = d[0][0],  C[i][0] = d[i][0] + C[i-1][0],  C[0][j] = d[0][j] + C[0][j-1],
 *     C[i][j] = d[i][j] + min(C[i-1][j], C[i-1][j-1], C[i][j-1])                              every + one f32 addition;
 *   the predecessor of an inner cell is the diagonal one if it is <= both others, else the left one (i, j-1) if it is <= the upper
 *   one, else the upper one; len[0][j] = j + 1, len[i][0] = i + 1, len[i][j] = len[predecessor] + 1 (the length of the path a
 *   backtrack from the last cell with the same preference walks).  Per pair p: cost[p] = C[La-1][Lb-1], path_len[p] = len[La-1][Lb-1]
 *   (int32), dist[p] = cost / (float)path_len, one correctly rounded f32 division.  cost and path_len may be NULL and are then not
 *   written.  A pair one of whose rows holds a NaN or an infinity, or (metrics 0 and 1) has the squared norm 0 as computed, gets
 *   dist = cost = NaN and path_len = -1.  A finite row whose squared norm as computed is above 2^116 (an infinity included) counts
 *   as non-finite: below that every distance and every sum along a path of 255 cells is finite.  The same result goes to a pair whose
 *   table row is out of range (a length outside [1, 128], a segment outside [0, N)): no address is formed from such a row.  No other
 *   pair is touched.  The La x Lb distances and costs exist in LDS and registers only.  One call takes any P in the range: the
 *   runtime refuses a grid of 2^32 threads or more, so the call goes out as ceil(P / 2^25) launches of at most 2^25 one-wave
 *   workgroups (cpc_abx_count: ceil(T / 2^23) launches of 256 threads per task), in order on the stream.  CPC_EINVAL also for pairs
 *   NULL or not 8-byte aligned, P outside [1, 2^31 - 1], dist NULL, dist, cost or path_len not 4-byte aligned.
 *
 * cpc_abx_count: tasks int64 [T][6] = (cell_off, n_c, s_p, n_p, s_q, n_q) on the device.  A cell's n_c x n_c block of DTW distances
 *   starts at dist[cell_off] (row item = A or B, column item = X); group p is the items [s_p, s_p + n_p) of the cell, group q the
 *   items [s_q, s_q + n_q).  out[t] (int64) = sum over x, a != x in p and b in q of 2 [d(a,x) < d(b,x)] + [d(a,x) == d(b,x)], with
 *   d(a,x) = dist[cell_off + (s_p + a) n_c + s_p + x] and d(b,x) = dist[cell_off + (s_q + b) n_c + s_p + x]; d(x,x) is never read.
 *   out[t] = -1 if a distance the task reads is NaN; out[t] = -2, and nothing read, unless 2 <= n_p <= 1024, 1 <= n_q <= 1024, both
 *   groups lie inside [0, n_c) and the block inside [0, n_dist).  Integer arithmetic only: the result does not depend on the order.
 *   CPC_EINVAL for dist, tasks or out NULL, dist not 4-byte aligned, tasks or out not 8-byte aligned, n_dist < 1, T outside
 *   [1, 2^31 - 1].
 * The calls never throw, allocate or synchronise.  stream is a hipStream_t.  (Added under ABI 9: no existing entry point changed.) */
int cpc_frame_distance(const void* x, int dtype, long long N, int D, long long ldx, long long a_first, int La, long long b_first, int Lb,
                       int metric, float* out, long long ldo, void* stream);
int cpc_dtw(const void* x, int dtype, long long N, int D, long long ldx, const long long* pairs, long long P, int metric, float* dist,
            float* cost, int* path_len, void* stream);
int cpc_abx_count(const float* dist, long long n_dist, const long long* tasks, long long T, long long* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CPC_HIP_H */
