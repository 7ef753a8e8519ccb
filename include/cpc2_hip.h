/*
 * cpc2_hip.h -- C ABI of the MI355X-native CPC training hot path (libcpc2_hip.so).
 *
 * The reference (MarvinLvn/CPC2) has no FFI/operator registry on this path: its boundary is
 * the Python nn.Module API of cpc/model.py and cpc/criterion/criterion.py, under which it
 * dispatches PyTorch ATen ops.  This library is what sits UNDER that boundary here: each entry
 * point replaces the ATen call sequence of one reference function (cited per function as
 * file:line relative to /root/reference).  The Python modules under cpc2_amd/ keep the
 * reference's class names,
 * constructor/forward signatures and state-dict keys and call these through ctypes.
 *
 * Conventions
 *   - plain C, no torch types; all pointers are DEVICE pointers unless named *_host.
 *   - the caller allocates every buffer (inputs, outputs, saved-for-backward workspace,
 *     scratch); sizes come from the *_bytes() queries; the library never frees or retains.
 *   - all work is enqueued on `stream` (a hipStream_t); no host synchronisation.  One exception to
 *     "on `stream`": cpc_infonce_backward* build their reference lists on a stream owned by the
 *     library (one per device), forked from and joined to `stream` with events inside the call.
 *   - every function returns 0 on success, a negative cpc_status otherwise;
 *     cpc_last_error() gives a thread-local message.
 *   - fp32 everywhere (the reference's arithmetic); activations are CHANNEL-LAST
 *     ([windows][frames][channels]) inside the library.
 *   - hidden sizes supported by the fused row kernels: 32, 64, 128, 256, 512.
 */
#ifndef CPC2_HIP_H
#define CPC2_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *cpc_stream_t; /* hipStream_t */

enum cpc_status {
    CPC_OK = 0,
    CPC_ERR_INVALID = -1, /* bad argument / unsupported shape */
    CPC_ERR_HIP = -2,     /* a HIP runtime call or kernel launch failed */
    CPC_ERR_WORKSPACE = -3 /* workspace / scratch too small */
};

int cpc_version(void);          /* 100 x major + minor; 105 = the entry points of round 5 (cpc_coop_set_policy,
                                  * cpc_recurrent_backward_calls, cpc_side_tail_wait); 107 = cpc_abx_dtw / cpc_abx_counts;
                                  * 108 = cpc_kmeans_scratch_bytes / cpc_kmeans_assign / cpc_kmeans_distances / cpc_kmeans_accumulate;
                                  * 109 = cpc_probe_xent / cpc_probe_head_backward / cpc_probe_ctc / cpc_probe_collapse (+ scratch queries);
                                  * 110 = cpc_abx_dtw_units (+ scratch query); 111 = cpc_augment_*; 112 = cpc_resample_*;
                                  * 113 = cpc_text_*;
                                  * 114 = one forward and one backward entry point per op: x_rest / n_first, c_frames, `deferred`;
                                  * 115 = the library owns the sampler's draw ahead: cpc_negidx_draw_ahead / cpc_negidx_take;
                                  * 116 = cpc_ctc_beam_search (+ scratch query) / cpc_align_score;
                                  * 117 = cpc_ctc_loss (+ scratch query) / cpc_seqnorm_len_* / cpc_conv_head_forward (+ scratch query) / cpc_conv_head_backward_data /
                                  * cpc_gather_utterances;
                                  * 118 = cpc_moments_scratch_bytes / cpc_moments_accumulate;
                                  * 119 = cpc_mfcc_tables_doubles / cpc_mfcc_tables_host / cpc_mfcc_frame_tile / cpc_melspec_scratch_bytes /
                                  * cpc_melspec_db / cpc_mfcc_finish / cpc_deltas;
                                  * 120 = cpc_ctc_align (+ scratch query) / cpc_ctc_align_segments;
                                  * 121 = cpc_seq_moments_scratch_bytes / cpc_seq_moments_accumulate / cpc_center_scale_rows;
                                  * 122 = cpc_probe_ctc runs on cpc_ctc_loss's kernels: cpc_probe_ctc_scratch_bytes returns
                                  * cpc_ctc_loss_scratch_bytes of the same sizes, and cpc_probe_ctc needs b <= 65535;
                                  * 123 = cpc_augment_pitch;
                                  * 124 = cpc_seg_dissimilarity / cpc_seg_boundaries / cpc_seg_lds_entries;
                                  * 125 = cpc_augment_freeverb;
                                  * 126 = cpc_unit_counts / cpc_unit_boundaries (+ scratch queries) / cpc_unit_counts_lds_cells /
                                  * cpc_unit_counts_chunk;
                                  * 127 = cpc_bandreject_tile / cpc_bandreject_max_half / cpc_bandreject_taps /
                                  * cpc_augment_bandreject;
                                  * 128 = cpc_sdtw (+ scratch query);
                                  * 129 = cpc_segment_units (+ scratch query) / cpc_segment_units_wave_k;
                                  * 130 = cpc_local_align (+ scratch query);
                                  * 131 = cpc_sdtw_units / cpc_local_align_units (+ scratch queries) */
const char *cpc_last_error(void);

/* In-situ kernel timing for bench.py: when enabled, the launchers bracket each launch of the named
 * kernel class with hipEvents on the launch stream.  cpc_prof_read sums and releases the finished
 * records of one class: "gemm_planes_nt", "gemm_planes_tn" (the plane-fed products of the encoder), "gemm_nt", "gemm_tn"
 * (the split-in-kernel products), "infonce_fwd", "infonce_bwd", "gru_fwd", "gru_bwd", "conv0_fwd", "conv0_bwd" ("gru_*"
 * times whichever recurrent kernel runs: GRU, LSTM or RNN).  on = 1: every class; on = 2: "gemm_planes_nt" only, on = 3:
 * "gemm_nt" only (the events cost about 0.1 ms per step when every class is timed); 0 (default): off. */
/* Asynchronous errors of the cooperative recurrent kernels (GRU / LSTM at hidden 256 / 512: workgroups that exchange
 * the hidden state through L2 and need to be resident all at once).  Every wait inside them is bounded; a wave whose wait
 * runs out poisons its outputs with NaN AND records a code in a host-visible word.  cpc_gru_* / cpc_lstm_* / cpc_rnn_*
 * return CPC_ERR_HIP (message in cpc_last_error) at their NEXT call when the word is set; cpc_async_error_check
 * synchronises `stream`, then reports and clears it.  Reporting a time-out also switches the process to the streaming
 * recurrent kernels (cpc_coop_set_policy(1)): the step that timed out is lost (NaN loss; cpc_adam_step skips non-finite gradient
 * elements, so the parameters are intact), the following ones do not depend on co-residency.  CPC_COOP_FAULT=1 in the environment
 * (tests) makes one member withhold one publish so that its group times out. */
int cpc_async_error_check(cpc_stream_t stream);

/* Streams that run BESIDE a given stream.  A HIP stream is served by one of a few hardware queues (4 by default per priority) that
 * the runtime assigns by use count at creation, and two streams on one queue run one after the other.  cpc_stream_create_apart
 * returns a non-blocking stream of default priority whose kernels were OBSERVED to run beside those of every avoid[i] (the
 * caller's stream(s); NULL = the null stream is a valid entry): a 200 us spin kernel on the one, a one-wave kernel on the
 * candidate, who finishes first.  (With four queues at most three streams can be apart from a given one AND from each other.)  Blocks the host until avoid[i] has
 * drained (once).  The library's own side stream and the sampler's worker stream are made this way; cpc2_amd.train's
 * data-parallel helper stream too.  cpc_streams_overlap(a, b): the same test on two given streams, 1 = beside, 0 = behind, < 0
 * error.  cpc_stream_apart_failures: streams handed out although every candidate failed the test (a saturated device). */
int cpc_stream_create_apart(const cpc_stream_t *avoid, int n_avoid, cpc_stream_t *out);
int cpc_streams_overlap(cpc_stream_t a, cpc_stream_t b);
long cpc_stream_apart_failures(void);
int cpc_stream_spin(cpc_stream_t stream, long ticks);      /* one wave of `stream` busy for `ticks` of the 100 MHz clock (diagnostics) */
/* the library's side stream on the current device (created on first use, apart from `caller`), for diagnostics */
int cpc_side_stream(cpc_stream_t caller, cpc_stream_t *out);
/* Cooperative recurrent launches (the GRU / LSTM kernels at hidden 256 / 512 that need every workgroup resident at once)
 * issued by this process so far.  The data-parallel glue (train.py:523-527's role) checks with it that a gradient all-reduce
 * is never issued between a step's forward and backward recurrent launches. */
long cpc_coop_launches(void);
/* Granule buffers the cooperative kernels' launches hold right now: one per (device, stream) that launched one lately, at most
 * eight -- the one unused for longest is freed when a ninth stream comes (diagnostics / tests). */
int cpc_coop_comm_buffers(void);
/* Calls of the recurrent backward entry points (cpc_gru_backward, cpc_lstm_backward, cpc_rnn_backward; cooperative or streaming
 * kernels alike) by this process so far: what "the recurrent backward of this step has been issued" is decided by. */
long cpc_recurrent_backward_calls(void);
/* Process-wide policy for those kernels: 0 (default) = cooperative wherever they fit, 1 = the streaming (non-cooperative) kernels
 * only; returns the previous policy, policy < 0 only queries.  The cooperative kernels assume that nothing else holds CUs while
 * they run.  One rank per GPU with the library's own gradient exchange keeps that by stream order (cpc2_amd/train.py,
 * DataParallelContext); the reference's arrangement -- DistributedDataParallel around model and criterion on an RCCL process
 * group, cpc/train.py:523-527 -- does not: its criterion bucket is all-reduced (an RCCL kernel on the same CUs) while the
 * recurrent backward runs.  cpcStep selects policy 1 when it is handed such a wrapper (sticky for the process). */
int cpc_coop_set_policy(int policy);
int cpc_prof_enable(int on);
int cpc_prof_read(const char *name, double *total_ms, long *count);

/* ------------------------------------------------------------------------------------------
 * Dense fp32 GEMMs.  Replace the ATen addmm/linear calls behind nn.Linear / nn.GRU input
 * projections (criterion.py:144-146,163; model.py:196) and, through the encoder entry points,
 * the cuDNN convolutions of model.py:81-107.
 *   nt:  C[M,N] = A[M,K] . B[N,K]^T (+ bias[N])          (lda/ldb/ldc in elements)
 *   tn:  C[M,N] = sum_r A[r,M]^T . B[r,N], r < R   (split over R; scratch from the query)
 * f32 in, f32 out, f32 accumulation.  Mode 0 (default) multiplies on the bf16 matrix pipe after an
 * exact three-term bf16 split of every operand (six partial products, error <= that of the f32
 * MFMA path, tests/test_gpu_parity.py::test_gemm_split_accuracy); mode 1 uses the f32 MFMA
 * (v_mfma_f32_32x32x2_f32); mode 2 (opt-in, never the default) makes the encoder's plane-fed convolution products at
 * hidden 256 / 512 multiply only a0 b0 + a0 b1 + a1 b0 of the split (16 bits of product mantissa, f32 accumulation: half the
 * matrix work; TF32 -- what cuDNN gives the reference's convolutions on its own GPUs by default -- keeps 10 bits), everything
 * else as mode 0.  Domain of modes 0 and 2: |x| < (2 - 2^-8) 2^127 = 3.3962e38 for every operand element -- from there to FLT_MAX
 * the first bf16 term rounds to infinity and every output the element feeds is inf or NaN (never a finite wrong value; mode 1
 * multiplies such values as f32); and bf16's smallest subnormal being 2^-133, an element below 2^-110 in magnitude is held to
 * within 2^-134 absolute, not relative -- which shows only where it multiplies one of 2^100 or more.  cpc_gemm_set_mode returns the previous mode; other values only query.  The mode is PROCESS-WIDE (atomic, default
 * 0) and the only setting the library keeps between calls: it selects the arithmetic of a whole run (the tests' yardstick, the
 * benchmark's labelled entry) and has to reach the backward pass, which autograd runs on a thread of its own -- a per-thread mode
 * does not (tried in round 4).  Select it before the first call of a run, not concurrently with one.
 * cpc_gemm_nt splits K over workgroups when the output has few tiles and then adds the partial sums with
 * fp32 atomics (C is zeroed first); the module entry points below lend scratch for an ordered reduction instead.
 * ------------------------------------------------------------------------------------------ */
int cpc_gemm_set_mode(int mode);
int cpc_gemm_nt(const float *A, long lda, const float *B, long ldb, float *C, long ldc,
                const float *bias, int M, int N, int K, cpc_stream_t stream);
size_t cpc_gemm_tn_scratch_bytes(int M, int N, long R);
int cpc_gemm_tn(const float *A, long lda, const float *B, long ldb, float *C, long ldc,
                int M, int N, long R, void *scratch, size_t scratch_bytes, cpc_stream_t stream);

/* The same products with operands stored as their three bf16 terms ("planes": x = p0 + p1 + p2, p0 = bf16(x),
 * p1 = bf16(x - p0), p2 = bf16(x - p0 - p1); bf16 stored as 16-bit words, planes `plane_stride` elements apart).
 * The encoder's kernels write activations and weights in this form so that the GEMM tiles go global -> LDS by
 * LDS-DMA with no arithmetic besides the MFMAs; these two entries expose the format for tests and probes.
 * Layout of a plane: 16-element chunks; columns 16c .. 16c+15 of row R at chunk (c * s + R % s) * rows_per_phase + R / s,
 * s = 1 << stride_log2 (the stride of the Conv1d that will read the rows; 0 for a plain matrix).
 *   cpc_split_planes:   x[rows][ld] (f32, `cols` columns, cols % 16 == 0) -> planes[3][plane_stride]
 *   cpc_gemm_nt_planes: C[M,N] = A . B^T (+ bias).  K step ks (16 elements) of A is chunk c = ks >> a_taps_log2 of tap
 *                       j = (jj >> 1) + (jj & 1) * s, jj = ks & (k - 1) -- a Conv1d with k = 2 s taps over a C-channel signal:
 *                       K = k * C in the order (chunk, tap 0, s, 1, s + 1, ...); a plain matrix: a_taps_log2 = 0 --;
 *                       GEMM row m starts at signal row s * ((m / a_seg_rows) * a_seg_q + m % a_seg_rows)
 *                       (a_seg_rows <= 0: one segment).
 *                       B: planes of a plain [N][K] matrix in the same K order (stride_log2 0, rows_per_phase N).
 *                       N % 256 == 0, K % 32 == 0, K >= 64. */
int cpc_split_planes(const float *x, long ld, long rows, int cols, void *planes, long plane_stride, int stride_log2,
                     long rows_per_phase, cpc_stream_t stream);
int cpc_gemm_nt_planes(const void *a_planes, long a_plane_stride, int a_taps_log2, int a_stride_log2,
                       long a_rows_per_phase, int a_seg_rows, long a_seg_q, const void *b_planes, long b_plane_stride,
                       float *C, long ldc, const float *bias, long M, int N, int K, cpc_stream_t stream);
/*   cpc_gemm_tn_planes: C[M,N] = sum_{r<R} X(r, .)^T Y(r, .)  (weight gradients).  Column x of an operand is channel
 *                       x % channels of signal row r * s + tap + x / channels (s = 1 << stride_log2) of its planes.
 *                       M % 256 == 0, N % 256 == 0, R >= 64; rows R .. round_up(R, 32) - 1 of A must be zero, of B finite.
 *                       The partial sums of the row slabs are added in a fixed order (bitwise reproducible). */
size_t cpc_gemm_tn_planes_scratch_bytes(int M, int N, long R);
int cpc_gemm_tn_planes(const void *a_planes, long a_plane_stride, int a_stride_log2, long a_rows_per_phase, int a_tap,
                       int a_channels, const void *b_planes, long b_plane_stride, int b_stride_log2,
                       long b_rows_per_phase, int b_tap, int b_channels, float *C, long ldc, int M, int N, long R,
                       void *scratch, size_t scratch_bytes, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * ChannelNorm on a channel-FIRST tensor x[N,C,L] (standalone module API, model.py:27-60):
 * per (n,l) statistics over C, UNBIASED variance, y = (x-mean)*rsqrt(var+eps)*w[c]+b[c].
 * w/b may be NULL (affine=False).  rstd_save[N*L] is written by forward, read by backward.
 * ------------------------------------------------------------------------------------------ */
int cpc_channelnorm_forward(const float *x, const float *w, const float *b, float *y,
                            float *rstd_save, int N, int C, int L, float eps, cpc_stream_t stream);
int cpc_channelnorm_backward(const float *x, const float *w, const float *dy, const float *rstd_save,
                             float *dx, float *dw, float *db, int N, int C, int L, float eps,
                             cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * CPCEncoder (model.py:63-108): five strided Conv1d (k,s,p) = (10,5,3),(8,4,2),(4,2,1)x3, each
 * followed by ChannelNorm (model.py:52-60) and ReLU.
 *   x_first  [n_first, 1, length]                       raw waveform: windows 0 .. n_first - 1
 *   x_rest   [n_windows - n_first, 1, length] or NULL   windows n_first .. n_windows - 1 -- TWO input batches without concatenating
 *            them: train.py:99's cat([past, future]) as two pointers (only the first layer reads the waveform), 1 <= n_first <
 *            n_windows.  NULL: one input batch, and then n_first must equal n_windows
 *   params   20 pointers in state-dict order: for i in 0..4:
 *              conv{i}.weight [H, Cin, k], conv{i}.bias [H],
 *              batchNorm{i}.weight [1,H,1], batchNorm{i}.bias [1,H,1]
 *   z        [n_windows, frames, H] channel-last output (== reference output.permute(0,2,1),
 *            i.e. exactly what CPCModel.forward hands on, model.py:382)
 *   saved    activations kept for backward (cpc_encoder_saved_bytes)
 *   scratch  temporaries (cpc_encoder_scratch_bytes; same query serves forward and backward)
 *   grads    20 pointers, same order/shapes as params; overwritten (not accumulated)
 * Lengths: the forward pass takes every length that leaves a frame, i.e. 159 samples on (cpc_encoder_frames(158) == 0, and the
 * size queries return 0 below 159); the backward pass takes 400 samples on and refuses shorter inputs (CPC_ERR_INVALID) before
 * anything is launched.  Both take any n_windows >= 1 at every length they take and hidden 32, 64, 128, 256, 512 (at 256 / 512
 * few windows of a short input give the weight-gradient products fewer than the 64 reduction rows they want: the driver pads them
 * with zero rows).
 * The contents of saved and scratch are unspecified on entry: forward writes all of saved that backward reads, every row a
 * product reads as padding (halo, slack) included; nothing is kept in scratch between the passes, so the caller may reuse or
 * overwrite it in between (with deferred != 0: after cpc_side_tail_join); neither pass writes outside the sizes the queries
 * report, or to x, params or dz.  grads are overwritten, not accumulated.  tests/test_encoder_abi_gpu.py holds the two entry
 * points to this, and to the fp64 oracle, over the domain stated here.
 * ------------------------------------------------------------------------------------------ */
int cpc_encoder_frames(int length);
size_t cpc_encoder_saved_bytes(int n_windows, int length, int hidden);
size_t cpc_encoder_scratch_bytes(int n_windows, int length, int hidden);
int cpc_encoder_forward(const float *x_first, const float *x_rest, int n_first, const float *const *params, float *z, void *saved,
                        void *scratch, int n_windows, int length, int hidden, float eps, cpc_stream_t stream);
/* deferred != 0: the small passes of conv1-4 that only finish parameter gradients (the column sums of dgamma / dbeta / dbias, the
 * sum of each weight-gradient product's K-split slabs) run on a stream of the library's; the gradients of conv1-4 and their norms
 * may then not be read (nor x, saved, scratch reused) until cpc_side_tail_join(stream') -- see cpc_gru_backward.  conv0's
 * gradients are complete on `stream` as before. */
int cpc_encoder_backward(const float *x_first, const float *x_rest, int n_first, const float *const *params, const float *dz,
                         void *saved, void *scratch, float *const *grads, int n_windows, int length, int hidden, float eps,
                         int deferred, cpc_stream_t stream);
/* Inspection (tests only; the layout of `saved` is otherwise private): what the forward pass keeps of layer 0..4 --
 * the ChannelNorm of model.py:52-60 as (xhat, rstd) (layers 1..4) and, at hidden 256 / 512, the layer's ReLU'd output as the
 * next layer's input planes (layers 0..3).  out[10]:
 *   [0] byte offset of xhat [n_windows * out[2]][hidden] f32 (row n * out[2] + t, t < out[3] valid frames; -1: layer 0),
 *   [1] byte offset of rstd [n_windows * out[2]] f32 (-1: layer 0), [2] rows per window, [3] frames per window,
 *   [4] byte offset of the three bf16 planes of the layer's output (-1: stored as f32, or layer 4), [5] elements per plane,
 *   [6] rows per phase, [7] log2 of the reading stride s; channel ch of frame t of window n is element
 *   ((((ch / 16) << [7]) + (R & (s - 1))) * [6] + (R >> [7])) * 16 + ch % 16 with R = n * [8] + [9] + t.
 * hidden 32 / 64 / 128, layers 0..3 ([4] == -1: the output is kept as f32 rows): [5] byte offset of those rows, [hidden] f32 each,
 * [8] rows per window, [9] halo rows in front of a window's frames -- channel ch of frame t of window n is element
 * (n * [8] + [9] + t) * hidden + ch; [6] and [7] are 0. */
int cpc_encoder_saved_layout(int n_windows, int length, int hidden, int layer, long *out);

/* ------------------------------------------------------------------------------------------
 * CPCAR with mode="GRU" (model.py:158-207 -> torch.nn.GRU, batch_first, gate order r,z,n).
 *   x       [n, t, dim_in]
 *   params  4 pointers per layer: weight_ih_l{k} [3H, in], weight_hh_l{k} [3H, H],
 *           bias_ih_l{k} [3H], bias_hh_l{k} [3H]
 *   h0      [layers, n, H] or NULL (zeros)          (model.py:196, keepHidden :197-201)
 *   out     [n, t, H];  h_last [layers, n, H] or NULL
 *   backward: dout [n,t,H] -> dx [n,t,dim_in] (may be NULL), grads (4 per layer, overwritten)
 * ------------------------------------------------------------------------------------------ */
size_t cpc_gru_saved_bytes(int n, int t, int dim_in, int hidden, int layers);
size_t cpc_gru_scratch_bytes(int n, int t, int dim_in, int hidden, int layers);
int cpc_gru_forward(const float *x, const float *const *params, const float *h0, float *out,
                    float *h_last, void *saved, void *scratch, int n, int t, int dim_in, int hidden,
                    int layers, cpc_stream_t stream);
/* deferred != 0: on return `dx` is ordered on `stream`; the parameter gradients of every layer (weight_ih, weight_hh and the two
 * biases: two weight-gradient products and two column sums per layer that nothing in a backward pass needs before the optimiser)
 * are produced on a stream of the library's, beside the next layer's recurrent kernel and what the caller enqueues on `stream`
 * next, and NOTHING may read them (nor reuse x, saved, scratch, dout) until cpc_side_tail_join(stream') has been called for the
 * stream' that will -- it makes stream' wait for them (a no-op when nothing is pending; one such tail per device).  For callers
 * that write gradients in place and read them only at the end of the backward pass (cpc2_amd: FlatAdam's flat buffer). */
int cpc_gru_backward(const float *x, const float *const *params, const float *dout, void *saved,
                     void *scratch, float *dx, float *const *grads, int n, int t, int dim_in,
                     int hidden, int layers, int deferred, cpc_stream_t stream);
int cpc_side_tail_join(cpc_stream_t stream);
/* `stream` waits for the same work, which STAYS pending: for a stream that only consumes the finished gradients (the data-parallel
 * exchange's helper stream) while the caller's stream goes on; the buffers of the deferred calls are released by cpc_side_tail_join. */
int cpc_side_tail_wait(cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * CPCAR with mode="LSTM" (model.py:171-173 -> torch.nn.LSTM, batch_first, gate order i,f,g,o;
 * the default arMode of this fork, cpc/cpc_default_config.py).  Same conventions as the GRU:
 *   params  4 pointers per layer: weight_ih_l{k} [4H, in], weight_hh_l{k} [4H, H],
 *           bias_ih_l{k} [4H], bias_hh_l{k} [4H]
 *   h0, c0  [layers, n, H] or NULL (zeros);  h_last, c_last [layers, n, H] or NULL
 *           (keepHidden keeps the (h, c) tuple, model.py:197-199)
 * ------------------------------------------------------------------------------------------ */
size_t cpc_lstm_saved_bytes(int n, int t, int dim_in, int hidden, int layers);
size_t cpc_lstm_scratch_bytes(int n, int t, int dim_in, int hidden, int layers);
int cpc_lstm_forward(const float *x, const float *const *params, const float *h0, const float *c0,
                     float *out, float *h_last, float *c_last, void *saved, void *scratch, int n,
                     int t, int dim_in, int hidden, int layers, cpc_stream_t stream);
/* deferred != 0: as for cpc_gru_backward (the layers' weight gradients on the library's stream until cpc_side_tail_join). */
int cpc_lstm_backward(const float *x, const float *const *params, const float *dout, void *saved,
                      void *scratch, float *dx, float *const *grads, int n, int t, int dim_in,
                      int hidden, int layers, int deferred, cpc_stream_t stream);

/* CPCAR with mode="RNN" (model.py:174-176 -> torch.nn.RNN, tanh): weight_ih [H, in], weight_hh [H, H],
 * bias_ih [H], bias_hh [H]; arguments as for the GRU, except that this cell has no deferred backward: `deferred` must be 0
 * (CPC_ERR_INVALID otherwise). */
size_t cpc_rnn_saved_bytes(int n, int t, int dim_in, int hidden, int layers);
size_t cpc_rnn_scratch_bytes(int n, int t, int dim_in, int hidden, int layers);
int cpc_rnn_forward(const float *x, const float *const *params, const float *h0, float *out,
                    float *h_last, void *saved, void *scratch, int n, int t, int dim_in, int hidden,
                    int layers, cpc_stream_t stream);
int cpc_rnn_backward(const float *x, const float *const *params, const float *dout, void *saved,
                     void *scratch, float *dx, float *const *grads, int n, int t, int dim_in,
                     int hidden, int layers, int deferred, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Transformer autoregressive network (arMode="transformer", cpc/transformers.py:10-134,176-187):
 * `layers` TransformerLayers, each   y = LN1(x + Wo.MHA(x)),  out = LN2(Wl (y + FFN(y)) + bl),
 * 8 heads, causal mask, relative-position bias q_i.Krelpos[:, S-1-(i-j)], dff = 2048, ReLU.
 *   x       [n, s, d_model];  out [n, s, d_out];  s must be a multiple of size_seq (<= 128): longer
 *           inputs are attended in independent blocks of size_seq (transformers.py:38-50)
 *   params  cpc_transformer_param_count() = 15 pointers per layer, in THIS order:
 *           Wq, Wk, Wv, Wo [d,d]; Krelpos [d/8, size_seq] (NULL: no relative positions);
 *           ln_multihead.weight, .bias [d]; lin1.weight [2048,d], lin1.bias [2048];
 *           lin2.weight [d,2048], lin2.bias [d]; last_linear.weight [d_out,d], .bias [d_out];
 *           ln_ffnetwork.weight, .bias [d_out]
 *   dropout_p  0 in eval mode; in training the masks come from a counter-based hash of (seed, index):
 *           pass the same (dropout_p, seed) to backward.
 *   n_classifiers  1: plain TransformerLayers.  k > 1: the LAST layer is the multi-classifier head of
 *           the multi-head predictor (MultiClassifierTransformerHead, transformers.py:137-158):
 *           lin2.weight is [k*d, 2048], lin2.bias [k*d], and
 *           out[n, s, c, :] = LN2(Wl (y + FFN(y)[c*d : (c+1)*d]) + bl), out is [n, s, k, d_out].
 *   backward: dout -> dx (may be NULL), grads (same order/shapes as params, overwritten; NULL where the parameter is NULL).
 *   domain  d_model and d_out each one of 32, 64, 128, 256, 512 (independently; 8 heads of d_model / 8); 1 <= size_seq <= 128;
 *           1 <= layers <= 4, and layers > 1 needs d_out == d_model; 1 <= n_classifiers <= 64.  Anything else: the size
 *           queries return 0 and the entry points CPC_ERR_INVALID with the reason in cpc_last_error, nothing is launched.
 *   saved, scratch  exactly cpc_transformer_saved_bytes / _scratch_bytes are used.  Their contents are unspecified on entry:
 *           forward writes every part of `saved` that backward reads, and neither call reads scratch it has not written
 *           (scratch may be reused or overwritten between the two calls).
 *   (tests/test_transformer_abi_gpu.py holds the entry points to all of this in poisoned buffers against fp64.)
 * ------------------------------------------------------------------------------------------ */
int cpc_transformer_param_count(void);
size_t cpc_transformer_saved_bytes(int n, int s, int d_model, int d_out, int size_seq, int layers, int n_classifiers);
size_t cpc_transformer_scratch_bytes(int n, int s, int d_model, int d_out, int size_seq, int layers, int n_classifiers);
int cpc_transformer_forward(const float *x, const float *const *params, float *out, void *saved,
                            void *scratch, int n, int s, int d_model, int d_out, int size_seq, int layers,
                            int n_classifiers, float dropout_p, unsigned long long seed, cpc_stream_t stream);
/* deferred != 0 (see cpc_gru_backward): with one classifier, every parameter gradient of layer 0 -- seven weight-gradient
 * products with their bias sums, the LayerNorms' and Krelpos' column sums -- is produced on the library's stream after this call
 * has returned; `dx` and the gradients of layers 1.. are ordered on `stream`.  cpc_side_tail_join before anything reads them. */
int cpc_transformer_backward(const float *x, const float *const *params, const float *dout, void *saved,
                             void *scratch, float *dx, float *const *grads, int n, int s, int d_model,
                             int d_out, int size_seq, int layers, int n_classifiers, float dropout_p,
                             unsigned long long seed, int deferred, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Negative-index sampler of CPCUnsupersivedCriterion.sampleClean (criterion.py:247-266), HOST
 * side, bit-exact with torch's CPU generator: 32-bit MT19937, one draw per element,
 * batchIdx = draw % batch (all n first), then seqIdx = draw % (T-1) + 1;
 * extIdx[(bb*n_neg + nn)*W + t] = (seqIdx + t) % T + batchIdx*T   (draw / reference order).
 * time_major != 0 stores the SAME values as [b][W][n_neg] (the negatives of one (b,t) contiguous):
 * the layout cpc_infonce_* consume.  batch_idx/seq_idx outputs (optional) stay in draw order.
 * State interop: mt[624], left, next as in torch's CPUGeneratorImpl legacy state.
 * ------------------------------------------------------------------------------------------ */
typedef struct cpc_mt19937 cpc_mt19937;
cpc_mt19937 *cpc_mt_create(uint32_t seed);
void cpc_mt_destroy(cpc_mt19937 *g);
int cpc_mt_seed(cpc_mt19937 *g, uint32_t seed);
int cpc_mt_get_state(const cpc_mt19937 *g, uint32_t *mt624, int *left, int *next);
int cpc_mt_set_state(cpc_mt19937 *g, const uint32_t *mt624, int left, int next);
int cpc_negidx_sample_host(cpc_mt19937 *g, int batch, int seq_len, int window, int n_neg,
                           int time_major, int32_t *ext_idx_host, int64_t *batch_idx_host_opt,
                           int64_t *seq_idx_host_opt);
/* The same draw on a worker thread (at most one in flight per generator): returns at once;
 * ext_idx_host is valid after cpc_negidx_wait(g).  Every other cpc_mt_* / cpc_negidx_* call on g
 * waits for it first, so the stream stays sequential. */
int cpc_negidx_sample_host_async(cpc_mt19937 *g, int batch, int seq_len, int window, int n_neg,
                                 int time_major, int32_t *ext_idx_host);
int cpc_negidx_wait(cpc_mt19937 *g);
/* Split form used by the training loop: the host only produces the raw generator words (the sequential,
 * torch-bit-exact part; 2*n of them, n = batch*n_neg*window: batchIdx stream then seqIdx stream), the
 * device reduces them (% batch, % (T-1) + 1), applies the time offset and writes the time-major extIdx.
 * Integer-exact: cpc_negidx_expand(raw) == cpc_negidx_sample_host(time_major = 1). */
int cpc_mt_draw_host(cpc_mt19937 *g, uint32_t *raw_host, size_t n);
/* The draw AHEAD: the next call's 2*n words, drawn by the worker while the caller goes on.  The library keeps where the generator
 * stood in front of that draw, how many words it drew and how many of them callers took, so that
 *     SEEN THROUGH ANY SYNCHRONOUS ENTRY POINT, THE GENERATOR STANDS BEHIND EXACTLY THE WORDS CALLERS HAVE TAKEN:
 * cpc_mt_draw_host, cpc_negidx_sample_host(_async) and cpc_mt_get_state first wait for the worker as cpc_negidx_wait does (that
 * blocks the host on a device draw nobody took) and, unless every word drawn ahead was taken, go back to the state in front of
 * the draw and generate the taken words again; cpc_mt_set_state and cpc_mt_seed wait and forget the draw.  A draw ahead that is
 * not taken, or taken in part, is thereby undone without anyone asking for it; one that is taken whole costs nothing.
 * cpc_negidx_draw_ahead: the worker (ONE thread per generator with ONE stream, made on its first device job apart from
 *   `caller_stream`'s hardware queue: cpc_stream_create_apart) settles the draw ahead before this one in the same way, draws
 *   2 * batch * n_neg * window words into raw_host (pinned), copies them to raw_dev and expands them into ext_dev
 *   [batch * window * n_neg] on its stream -- the two torch.randint calls AND the index arithmetic of criterion.py:247-266 for
 *   step i + 1, done while step i runs -- and records an event behind them.  raw_dev == ext_dev == NULL: words into raw_host
 *   only, no HIP call.
 * cpc_negidx_take: the caller uses the next `words` of the words drawn ahead (at most those left of them, else CPC_ERR_INVALID):
 *   waits for the worker's HOST part and makes `stream` (may be NULL after a host-only draw) wait for the event, so that
 *   everything enqueued on it afterwards may read raw_dev / ext_dev; the host is not blocked on the device. */
int cpc_negidx_draw_ahead(cpc_mt19937 *g, uint32_t *raw_host, uint32_t *raw_dev, int32_t *ext_dev, int device,
                          int batch, int seq_len, int window, int n_neg, cpc_stream_t caller_stream);
int cpc_negidx_take(cpc_mt19937 *g, size_t words, cpc_stream_t stream);
int cpc_negidx_stream(cpc_mt19937 *g, cpc_stream_t *out);      /* the worker's stream (NULL before its first device job) */
int cpc_negidx_expand(const uint32_t *raw, int32_t *ext_idx, int batch, int seq_len, int window, int n_neg,
                      cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * CPCUnsupersivedCriterion.forward with linear predictors (criterion.py:329-363, 291-302,
 * 237-286, PredictionNetwork.forward :152-173): K predictions W_k c_t, scored by dot product / H
 * against 1 positive z[b, t+k] + n_neg gathered negatives, cross-entropy vs class 0.
 * The gathered candidate tensors of the reference are never materialised.
 *   c        [b, c_frames, dim_ar]   context.  c_frames = T: the whole sequence (only t < W = T-K is used; criterion.py:296
 *            slices `cFeature[:, :windowSize]` itself), or c_frames = W when the caller hands over ONLY the W frames it uses: a
 *            causal context network that keeps no state across calls need not compute the k frames behind them
 *            (cpc2_amd.train.cpcStep runs it on W steps).  Any other c_frames: CPC_ERR_INVALID.  z stays [b, T, dim_enc]
 *   z        [b, T, dim_enc]  encoder targets
 *   wpred    [K, dim_enc, dim_ar] packed nn.Linear weights (predictors.k.weight)
 *   ext_idx  [b, W, n_neg] int32 rows of z.view(b*T, dim_enc): cpc_negidx_sample_host with
 *            time_major = 1 (same values as the reference's [b, n_neg, W] order, transposed)
 *   weights  [b*W] per-sample loss weights or NULL (ones)        (criterion.py:334-340)
 *   losses   [K]  mean_i(w_i * CE_i);  acc [K] = #(argmax == 0) / (b*W)
 * backward: dlosses [K] upstream gradient -> dc [b,c_frames,dim_ar], dz [b,T,dim_enc],
 *           dwpred [K,dim_enc,dim_ar]  (all overwritten; dz is summed per row in a fixed order, so it
 *           is identical from run to run)
 * ------------------------------------------------------------------------------------------ */
size_t cpc_infonce_saved_bytes(int b, int t, int k, int dim_ar, int dim_enc, int n_neg);
/* scratch: dim_ar > 0 gives what ANY entry point of the criterion may use (the module-predictor entries below keep one
 * contribution row per candidate, 1.06 GB at the benchmark shape).  dim_ar < 0 (context width -dim_ar) gives what
 * cpc_infonce_forward / cpc_infonce_backward ALONE need: where their dz comes from per-row context sums (the environment's
 * CPC_NCE_DZ=q, read at every call; linear predictors, dim_enc and dim_ar 256 or 512) the contribution rows are not part of it. */
size_t cpc_infonce_scratch_bytes(int b, int t, int k, int dim_ar, int dim_enc, int n_neg);
/* byte offset, inside `saved`, of the logits the forward pass leaves there: float [b, W, K, 1 + n_neg], candidate 0 = the
 * positive, the negatives in slot order (cpc_infonce_perm_offset) -- what getPrediction (criterion.py:291-302) returns once
 * brought back to the caller's order and permuted to K tensors [b, 1 + n_neg, W] */
size_t cpc_infonce_logits_offset(int b, int t, int k, int dim_ar, int dim_enc, int n_neg);
/* The forward pass visits a (b, t)'s negatives sorted by z-row block and leaves the logits in THAT order (element 1 + g of a
 * row = the negative in slot g: a tile's columns are then consecutive floats).  byte offset, inside `saved`, of the
 * permutation: uint16 [b, W, n_neg], perm[g] = the caller's number (its position in ext_idx) of the negative in slot g */
size_t cpc_infonce_perm_offset(int b, int t, int k, int dim_ar, int dim_enc, int n_neg);
/* (ext_idx is range-checked on the device before anything gathers with it: an index outside [0, b * t) is replaced by 0 and
 *  reported by the next cpc_async_error_check(stream) -- criterion.py:264-268's gather has no such check.) */
int cpc_infonce_forward(const float *c, const float *z, const float *wpred, const int32_t *ext_idx,
                        const float *weights, float *losses, float *acc, void *saved, void *scratch,
                        int b, int t, int c_frames, int k, int dim_ar, int dim_enc, int n_neg, cpc_stream_t stream);
/* deferred != 0: on return only `dc` -- what the context network's backward (cpc/model.py:158-207 under autograd) needs next -- is
 * ordered on `stream`; `dz` and `dwpred` are produced on a stream of the library's, beside whatever the caller enqueues on `stream`
 * afterwards, and NOTHING may read them (nor reuse c, z, ext_idx, saved, scratch) until cpc_infonce_join(stream') has been called
 * for the stream' that will: it makes stream' wait for them (a no-op when nothing is pending; one deferred backward may be pending
 * per device).  The context network's backward is latency-bound and leaves the chip idle; the criterion's dz is a memory-bound sum
 * over ~1 GB -- together they take the time of the longer one. */
int cpc_infonce_backward(const float *c, const float *z, const float *wpred, const int32_t *ext_idx,
                         const float *weights, const float *dlosses, void *saved, void *scratch,
                         float *dc, float *dz, float *dwpred, int b, int t, int c_frames, int k, int dim_ar,
                         int dim_enc, int n_neg, int deferred, cpc_stream_t stream);
int cpc_infonce_join(cpc_stream_t stream);

/* The same criterion when the K predictions come from predictor MODULES instead of linear maps
 * (rnnMode="transformer": criterion.py:136-143; the predictions are produced by cpc_transformer_*):
 *   pred   K pointers, each [b, W, dim_enc] (W = t - k): output of predictor k on c[:, :W]
 *   dpred  K pointers, same shapes (overwritten);  saved/scratch sizes: cpc_infonce_*_bytes with dim_ar = dim_enc */
int cpc_infonce_forward_pred(const float *const *pred, const float *z, const int32_t *ext_idx, const float *weights,
                             float *losses, float *acc, void *saved, void *scratch, int b, int t, int k,
                             int dim_enc, int n_neg, cpc_stream_t stream);
int cpc_infonce_backward_pred(const float *const *pred, const float *z, const int32_t *ext_idx,
                              const float *weights, const float *dlosses, void *saved, void *scratch,
                              float *const *dpred, float *dz, int b, int t, int k, int dim_enc, int n_neg,
                              cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Native FLAC reader for the window feeder (replaces torchaudio.load at cpc/dataset.py:411-437 and
 * cpc/feature_loader.py:343; the image ships no audio library).  HOST side.  Output is float32
 * [channels][total_samples] scaled to [-1, 1) like torchaudio.load; every decode is checked against
 * the MD5 of the unencoded audio stored in STREAMINFO (md5_ok, and an error if it differs).
 * ------------------------------------------------------------------------------------------ */
int cpc_flac_info(const char *path, int *sample_rate, int *channels, int *bits_per_sample,
                  long *total_samples);
int cpc_flac_decode_f32(const char *path, float *out_host, long capacity_floats, int *md5_ok);

/* Window feeder (cpc/dataset.py:308-321 __getitem__ slicing): out[i][0..window) =
 * audio[offsets[i] .. offsets[i]+window) from one flat device-resident audio buffer (zeros outside it).
 * audio, offsets (int64) and out are DEVICE pointers. */
int cpc_window_gather(const float *audio, long total_samples, const long *offsets, float *out, int batch,
                      int window, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Adam on one flat fp32 buffer (torch.optim.Adam as built at train.py:477-479: no weight decay,
 * no amsgrad).  g is multiplied by grad_scale first (1/world_size after an all-reduce SUM).
 *   m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ;
 *   p -= lr/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps)
 * An element whose gradient is not finite is left alone (p, m, v unchanged) and the asynchronous error word is set: the
 * next cpc_async_error_check(stream) returns CPC_ERR_HIP.  A cooperative recurrent kernel that timed out therefore cannot
 * poison the weights.  This is a PARTIAL update when only some elements are non-finite (the finite ones are applied, the step
 * count advances) and a deviation from the reference, whose torch.optim.Adam (train.py:477-479) propagates the NaN into the
 * weights; recovery = reload the last checkpoint, or continue knowingly.
 * ------------------------------------------------------------------------------------------ */
int cpc_adam_step(float *p, const float *g, float *m, float *v, long n, int step, float lr,
                  float beta1, float beta2, float eps, float grad_scale, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SGD with momentum on one flat fp32 buffer (torch.optim.SGD as built at train.py:480-482: momentum 0.9,
 * no dampening, no weight decay, no nesterov).  g is multiplied by grad_scale first.
 *   step == 1: buf = g ; step > 1: buf = momentum buf + g ;   p -= lr buf
 * One launch.  Non-finite gradient elements: the rule of cpc_adam_step (p and buf of that element unchanged,
 * asynchronous error word set, the finite elements applied).
 * ------------------------------------------------------------------------------------------ */
int cpc_sgd_step(float *p, const float *g, float *buf, long n, int step, float lr, float momentum,
                 float grad_scale, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * ABX phone discriminability (cpc/eval/ABX/abx_group_computation.py, dtw.pyx of the reference).
 *
 * Items are spans of frames in one fp32 buffer `frames` [total_frames][dp] (dp a multiple of 4; padding columns zero);
 * item i is frames item_off[i] .. item_off[i] + item_len[i] - 1.  The work list is in CSR form over "segments": segment s
 * compares x item seg_x[s] with the y items pair_y[seg_start[s] .. seg_start[s+1]-1]; pair p's result goes to out[p].
 *
 * cpc_abx_dtw: out[p] = DTW(x, y) / path length, as dtw.pyx:_dtw(normalized=True): frame distance
 *   distance = CPC_ABX_COSINE     acos(clamp(<x_r, y_c>, -1, 1)) / pi       (inputs normalised by the caller)
 *   distance = CPC_ABX_EUCLIDIAN  sqrt(sum_k (x_rk - y_ck)^2)
 * in f32 (k-ordered fma chain); cost[i][j] = d[i][j] + min(up, diag, left); the path length follows the reference's
 * backtrack (ties: diag, then left, then up).  Any item length >= 1.  path_len (optional, may be NULL) receives the length.
 * max_len_x / max_len_y bound the x / y item lengths; scratch: cpc_abx_dtw_scratch_bytes (0 when every x item has <= 64
 * frames).  A pair whose item index or length is out of range gets NaN (path length -1).
 *
 * cpc_abx_counts: triplet t has shape[5t .. 5t+4] = (nx, na, nb, a_off, b_off).  idx_a[a_off + i*na + j] is the pair index
 * of dxa[i][j] (-1: excluded, the diagonal of a symmetric group), idx_b[b_off + i*nb + k] that of dxb[i][k].
 *   lt[t] = #{(i,j,k): dxa[i][j] < dxb[i][k]},  eq[t] = #{(i,j,k): dxa[i][j] == dxb[i][k]}   (integers; nx*na*nb < 2^31)
 * ------------------------------------------------------------------------------------------ */
enum cpc_abx_distance { CPC_ABX_COSINE = 0, CPC_ABX_EUCLIDIAN = 1 };
size_t cpc_abx_dtw_scratch_bytes(int n_seg, int max_len_x, int max_len_y);
int cpc_abx_dtw(const float *frames, int dp, const int *item_off, const int *item_len, int n_items,
                const int *seg_x, const int *seg_start, const int *pair_y, int n_seg, int max_len_x, int max_len_y,
                int distance, float *out, int *path_len, void *scratch, size_t scratch_bytes, cpc_stream_t stream);
int cpc_abx_counts(const float *dist, int n_pairs, const int *idx_a, const int *idx_b, const int *shape, int n_trip,
                   int *lt, int *eq, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * ABX on quantized units (cpc/eval/eval_ABX_clustering.py of the reference): the DTW of cpc_abx_dtw between items whose
 * frames are unit ids.  `units` [total_frames] int32; item i is units item_off[i] .. item_off[i] + item_len[i] - 1.  The
 * frame distance is d_same where the two units are equal and d_diff where they differ: the two values the reference's
 * distance takes on one-hot rows, computed by the caller.  Segment / pair lists, outputs, path-length rule, limits and the
 * not-computable convention (NaN, path length -1) are those of cpc_abx_dtw; cost = d + predecessor in f32, one f32 division
 * by the path length at the end.  scratch: cpc_abx_dtw_units_scratch_bytes (0 when every x item has <= 64 frames; 0 and a
 * "negative size" message in cpc_last_error for a negative argument, as the other queries on units).
 * ------------------------------------------------------------------------------------------ */
size_t cpc_abx_dtw_units_scratch_bytes(int n_seg, int max_len_x, int max_len_y);
int cpc_abx_dtw_units(const int *units, const int *item_off, const int *item_len, int n_items,
                      const int *seg_x, const int *seg_start, const int *pair_y, int n_seg,
                      int max_len_x, int max_len_y, float d_same, float d_diff,
                      float *out, int *path_len, void *scratch, size_t scratch_bytes, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Query-by-example term detection: subsequence DTW of a query inside a document (csrc/sdtw.hip, version 128; DESIGN.md
 * section 26).  The reference has no such task.  Items and the work list are laid out as for cpc_abx_dtw: segment s compares
 * QUERY item seg_q[s] with the DOCUMENT items pair_doc[seg_start[s] .. seg_start[s+1]-1]; a query's document list may be split
 * over several segments.  Pair p's results go to score[p] and span[3p .. 3p+2] = (start, end, length).
 *
 * Cells.  For a query of n >= 1 frames and a document of m >= 1 frames, d[i][j] is the frame distance of cpc_abx_dtw
 * (CPC_ABX_COSINE or CPC_ABX_EUCLIDIAN, f32, k-ordered fma chain, inputs normalised by the caller).  Every cell carries
 * (cost, length, start).
 * Recurrence.  Row 0: cost = d[0][j], length = 1, start = j (the start is free: no left predecessor on row 0).
 *   i > 0, j = 0: the predecessor is up (i-1, 0).  Otherwise the predecessor is the one of smallest cost among diag (i-1, j-1),
 *   left (i, j-1) and up (i-1, j); ties go to diag, then left, then up.  cost = d[i][j] + pred.cost (one f32 addition),
 *   length = pred.length + 1, start = pred.start.
 * Detection.  v[j] = cost[n-1][j] / length[n-1][j] (one f32 division); score = min_j v[j], the first j among equals;
 *   start = start[n-1][j], end = j, length = length[n-1][j].  m < n is allowed: the path may go straight up.
 *   No slope or band constraint is applied, and one detection is returned per pair.
 * Not computable.  A pair whose item index or length is out of range (an index outside [0, n_items), a length < 1, or a query
 *   longer than 64 frames against a document longer than max_len_doc) gets score NaN and span (-1, -1, -1).
 *
 * Any query length >= 1; max_len_q / max_len_doc bound the query / document lengths and size the scratch:
 * cpc_sdtw_scratch_bytes = 0 when max_len_q <= 64, else 2 * 12 * max_len_doc bytes per workgroup (the boundary row of a 64-row
 * strip of the query, double-buffered); negative sizes give 0 and a cpc_last_error text.  Frames beyond an item are never read;
 * the scratch's contents before the launch are never read; no atomics: two launches give the same bits.  A bad argument
 * returns CPC_ERR_INVALID with a message and launches nothing.
 * ------------------------------------------------------------------------------------------ */
size_t cpc_sdtw_scratch_bytes(int n_seg, int max_len_q, int max_len_doc);
int cpc_sdtw(const float *frames, int dp, const int *item_off, const int *item_len, int n_items, const int *seg_q,
             const int *seg_start, const int *pair_doc, int n_seg, int max_len_q, int max_len_doc, int distance,
             float *score, int *span /* [pairs][3] int32: start, end, length */, void *scratch, size_t scratch_bytes,
             cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Spoken term discovery: LOCAL alignment of two items, both ends free on both sides (csrc/lalign.hip, version 130; DESIGN.md
 * section 28).  The reference has no such task.  Items and the work list are laid out as for cpc_sdtw: segment s compares ROW
 * item seg_a[s] (n frames) with the COLUMN items pair_b[seg_start[s] .. seg_start[s+1]-1] (m frames each); a row item's list may
 * be split over several segments.  Pair p's results go to score[p] and span[5p .. 5p+4].
 *
 * Cells.  d[i][j] is the frame distance of cpc_abx_dtw, bit for bit (CPC_ABX_COSINE or CPC_ABX_EUCLIDIAN, f32, k-ordered fma
 *   chain, inputs normalised by the caller).  Two f32 parameters: a threshold theta > 0 and a step penalty gamma >= 0.
 * Gain.  g = theta - d[i][j] (one f32 subtraction).
 * Candidates of cell (i, j).  diag: H[i-1][j-1], when i > 0 and j > 0; left: H[i][j-1] - gamma, when j > 0; up: H[i-1][j] - gamma,
 *   when i > 0 (each of left and up is one f32 subtraction).  The best candidate is the largest; ties go to diag, then left,
 *   then up.
 * Open or continue.  No candidate exists, or the best is <= 0: the cell opens a path, h = g, length = 1, start = (i, j).
 *   Otherwise h = g + best (one f32 addition), length = pred.length + 1, start = pred.start.
 * Clamp.  h > 0: the cell holds (H = h, length, start).  Otherwise H = 0 and the cell carries nothing.  A NaN distance closes
 *   the cell.
 * Result of a pair.  The cell of largest H; among equals the smallest i, then the smallest j, whatever the order in which the
 *   matrix is walked.  score[p] = H, span[5p .. 5p+4] = (start_i, end_i, start_j, end_j, length).  No positive cell: score 0.0f,
 *   span all -1.
 * Not computable.  A pair with an item index outside [0, n_items), a length < 1, a row item longer than max_len_a or a column
 *   item longer than max_len_b gets score NaN and span all -1.
 * Limits.  Items have at most 32767 frames (the two start indices of a cell share one word): max_len_a, max_len_b <= 32767.  One
 *   match is returned per pair, and no band or slope constraint is applied other than gamma.
 *
 * cpc_local_align_scratch_bytes = 0 when max_len_a <= 64, else 2 * 12 * max_len_b bytes per workgroup (the boundary row of a
 * 64-row strip of the row item, one cell per column, double-buffered); negative sizes give 0 and a cpc_last_error text.  Frames
 * beyond an item are never read; the scratch's contents before the launch are never read; no atomics: two launches give the same
 * bytes.  Bad arguments (a null buffer, dp not a positive multiple of 4, an unknown distance, theta not finite or <= 0, gamma not
 * finite or < 0, negative or zero sizes, a maximum above 32767) return CPC_ERR_INVALID, a scratch that is too small
 * CPC_ERR_WORKSPACE, each with a cpc_last_error text; nothing is launched.
 * ------------------------------------------------------------------------------------------ */
size_t cpc_local_align_scratch_bytes(int n_seg, int max_len_a, int max_len_b);
int cpc_local_align(const float *frames, int dp, const int *item_off, const int *item_len, int n_items, const int *seg_a,
                    const int *seg_start, const int *pair_b, int n_seg, int max_len_a, int max_len_b, int distance, float theta,
                    float gamma, float *score, int *span /* [pairs][5] int32: start_i, end_i, start_j, end_j, length */,
                    void *scratch, size_t scratch_bytes, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Term detection and term discovery on quantized units (csrc/sdtw_units.hip, csrc/lalign_units.hip, version 131; DESIGN.md
 * section 29).  `units` [total_frames] int32 as for cpc_abx_dtw_units: item i is units item_off[i] .. item_off[i] + item_len[i] - 1.
 * Any int32 is a unit id: only equality is looked at.  The frame distance takes two values, given by the caller:
 *     d[i][j] = d_same where the two units are equal, d_diff where they differ.
 * With that d[i][j], cpc_sdtw_units is cpc_sdtw and cpc_local_align_units is cpc_local_align, word for word: the work list, the
 * cell contents, the tie order diag, left, up, the free start on row 0, one f32 addition per cell and one f32 division per end
 * column (subsequence); one f32 subtraction per gain and per candidate, open / continue / clamp, the best cell by (largest H,
 * smallest i, smallest j) (alignment); the outputs, and NaN and -1 for a pair that is not computable.  The kernels run the same
 * copy of each recurrence as the dense ones (csrc/sdtw_rule.h, csrc/lalign_rule.h).
 *
 * Not computable, both entry points: an item index outside [0, n_items), a length < 1, a row item (query) longer than
 * max_len_q / max_len_a or a column item (document) longer than max_len_doc / max_len_b.
 * Limits.  Alignment items have at most 32767 frames (max_len_a, max_len_b <= 32767); otherwise those of the dense entry points.
 *
 * Scratch, both queries: 0 when the row maximum is <= 64, else min(n_seg, 2048) workgroups x 4 waves x 2 buffers x 12 bytes x
 * the column maximum (one wave serves one pair, so every wave keeps the boundary row of a 64-row strip, double-buffered; the
 * launch has at most 2048 workgroups); negative sizes give 0 and a cpc_last_error text.  Units beyond an item are never read; the
 * scratch's contents before the launch are never read; no atomics and no LDS: two launches give the same bytes.
 * Bad arguments (a null buffer, a NaN d_same or d_diff, negative or zero sizes; for the alignment theta not finite or <= 0, gamma
 * not finite or < 0, a maximum above 32767) return CPC_ERR_INVALID; a scratch that is too small returns CPC_ERR_INVALID from
 * cpc_sdtw_units and CPC_ERR_WORKSPACE from cpc_local_align_units, as their dense siblings do; each with a cpc_last_error text
 * that names the entry point (sdtw_units / local_align_units); nothing is launched and no output is written.
 * ------------------------------------------------------------------------------------------ */
size_t cpc_sdtw_units_scratch_bytes(int n_seg, int max_len_q, int max_len_doc);
int cpc_sdtw_units(const int *units, const int *item_off, const int *item_len, int n_items, const int *seg_q,
                   const int *seg_start, const int *pair_doc, int n_seg, int max_len_q, int max_len_doc, float d_same,
                   float d_diff, float *score, int *span /* [pairs][3] int32: start, end, length */, void *scratch,
                   size_t scratch_bytes, cpc_stream_t stream);
size_t cpc_local_align_units_scratch_bytes(int n_seg, int max_len_a, int max_len_b);
int cpc_local_align_units(const int *units, const int *item_off, const int *item_len, int n_items, const int *seg_a,
                          const int *seg_start, const int *pair_b, int n_seg, int max_len_a, int max_len_b, float d_same,
                          float d_diff, float theta, float gamma, float *score,
                          int *span /* [pairs][5] int32: start_i, end_i, start_j, end_j, length */, void *scratch,
                          size_t scratch_bytes, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * k-means on features (cpc/clustering/clustering.py of the reference).  x [n][d] rows, ck [k][d] centroids, all fp32 DEVICE
 * pointers, row-major and contiguous.  Limits: 0 <= n < 2^31, 1 <= d <= 4096, 1 <= k <= 2^20; a call outside them returns
 * CPC_ERR_INVALID with a message.
 *
 * Every distance is the f32 chain over ascending feature index f:  t = x[f] - c[f]; acc = fmaf(t, t, acc)  (acc from 0),
 * never the |x|^2 - 2 x.c + |c|^2 expansion.  cpc_kmeans_assign and cpc_kmeans_distances compute it identically, so
 * index[i] == argmin_j dist[i][j] exactly.
 *
 * cpc_kmeans_assign: index[i] (int32) = the centroid of least distance, the LOWEST index among equal minima (torch.argmin);
 *   min_sq[i] = that distance (min_sq may be NULL).  The [n][k] matrix is never formed.
 * cpc_kmeans_distances: dist[i][j] = the distance of row i to centroid j ([n][k], long offsets).
 * cpc_kmeans_accumulate: running per-cluster sums and counts:  sums[c][:] += sum of the rows with index == c,
 *   counts[c] += their number (int64).  A row whose index is outside [0, k) is skipped and counted nowhere; a cluster with
 *   no row is left untouched.  No float atomic: rows are bucketed stably (ascending row order in each cluster), summed in
 *   chunks of 256 rows, and the chunks added in order, so the result is bitwise reproducible.  scratch:
 *   cpc_kmeans_scratch_bytes(n, d, k) bytes (0 for sizes outside the limits).
 * ------------------------------------------------------------------------------------------ */
size_t cpc_kmeans_scratch_bytes(long n, int d, int k);
int cpc_kmeans_assign(const float *x, long n, int d, const float *ck, int k, int *index, float *min_sq, cpc_stream_t stream);
int cpc_kmeans_distances(const float *x, long n, int d, const float *ck, int k, float *dist, cpc_stream_t stream);
int cpc_kmeans_accumulate(const float *x, long n, int d, const int *index, int k, float *sums, int64_t *counts,
                          void *scratch, size_t scratch_bytes, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Streaming second moments of one or two feature streams in f64 (the CCA of cpc2_amd/cca; a PCA needs the one-stream form).
 * x [n][dx] and y [n][dy] are fp32 DEVICE rows with row strides ldx >= dx and ldy >= dy (elements); x and y may alias.
 * y == NULL with dy == 0 is the one-stream form.  With D = dx + dy and row z = [x row, y row], the running totals are
 *   sums[D] += sum z,   gram[D][D] += sum z z^T     (f64 DEVICE buffers; gram row-major and FULL: both triangles are written and
 * are equal bit for bit).  The caller zeroes sums and gram once and keeps the row count itself.
 * Limits: 1 <= dx <= 512, 0 <= dy <= 512, 1 <= n < 2^31; a call outside them (or with ld below the width, or dy > 0 without y)
 * returns CPC_ERR_INVALID with a message before any launch, and the size query returns 0.
 *
 * Every product of two f32 values is exact in f64; the products are accumulated in f64 on v_mfma_f64_16x16x4_f64, so the only
 * rounding is that of an f64 sum.  One workgroup per (64 x 64 tile of the upper block triangle, one of S row ranges) leaves a
 * partial tile in scratch; a second kernel adds the S partials in range order and mirrors the triangle.  S depends on
 * (n, dx + dy) alone and there is no float atomic: the same call gives the same bits.  Columns beyond D and rows beyond n are
 * zero-filled in the kernel; no padded copy and no f64 copy of the inputs is made.
 * scratch: cpc_moments_scratch_bytes(n, dx, dy) bytes.
 * ------------------------------------------------------------------------------------------ */
size_t cpc_moments_scratch_bytes(long n, int dx, int dy);
int cpc_moments_accumulate(const float *x, long ldx, int dx, const float *y, long ldy, int dy, long n,
                           double *sums, double *gram, void *scratch, size_t scratch_bytes, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Second moments of windows of frames and of their frame-to-frame differences in f64 (the PCA / SFA projections of
 * cpc2_amd/dim_reduction.py; csrc/seqmoments.hip).  version 121.
 * x is [b][s][d] fp32 on the DEVICE with row stride ld >= d and sequence stride seq_stride >= s * ld (both in elements).  Of each
 * sequence the frames t = skip .. s-1 are kept, and in ONE pass over x the running f64 DEVICE totals become
 *   sums[d]     += sum x_t                                    over the kept frames,
 *   gram[d][d]  += sum x_t x_t^T                              over the kept frames,
 *   dgram[d][d] += sum (x_{t+1} - x_t) (x_{t+1} - x_t)^T      over t = skip .. s-2 of each sequence.
 * gram and dgram are row-major and FULL: both triangles are written and are equal bit for bit.  The caller zeroes the three once and
 * keeps the counts itself (b * (s - skip) rows, b * (s - skip - 1) differences).  With s - skip == 1 there is no difference and dgram
 * is left as it was.
 * The difference is taken in f64 from the two f32 values (exact) and never across a sequence boundary; products are accumulated
 * in f64 on v_mfma_f64_16x16x4_f64 as cpc_moments_accumulate does, a fresh chain per slab of 32 rows added to the running tile in
 * plain f64.  The split of the rows depends on (b, s, skip, d) alone and there is no float atomic: the same call gives the same bits.
 * Skipped frames, the columns beyond d and the gap between sequences are never read, so nothing in them (a NaN included) reaches
 * a result; no padded copy, no f64 copy and no difference tensor is made.
 * Limits: 1 <= d <= 512, b >= 1, 0 <= skip < s, b * s < 2^31.  A call outside them, a stride below the width, a null buffer or a
 * scratch below cpc_seq_moments_scratch_bytes(b, s, skip, d) returns CPC_ERR_INVALID with a message before any launch, and the
 * size query returns 0 outside the limits.
 *
 * cpc_center_scale_rows: y[r][c] = (x[r][c] - mean[c]) / (scale[c] + 1e-8f) for r < n, c < d, in f32 with each of the three
 * operations rounded once (a correctly rounded division): what the reference's SFALinear.forward does in two in-place passes.
 * scale == NULL leaves the division out (its PCA.forward).  x, y are fp32 DEVICE rows with strides ldx, ldy >= d; y is apart from x,
 * or y == x with ldy == ldx.  Limits: n >= 1, 1 <= d <= 512; anything else is CPC_ERR_INVALID with a message before any launch.
 * ------------------------------------------------------------------------------------------ */
size_t cpc_seq_moments_scratch_bytes(int b, int s, int skip, int d);
int cpc_seq_moments_accumulate(const float *x, long ld, long seq_stride, int b, int s, int skip, int d,
                               double *sums, double *gram, double *dgram,
                               void *scratch, size_t scratch_bytes, cpc_stream_t stream);
int cpc_center_scale_rows(const float *x, long ldx, const float *mean, const float *scale,
                          float *y, long ldy, long n, int d, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Log-mel and MFCC baseline features (cpc2_amd/spectral.py; csrc/mfcc.hip).  version 119.
 * The definition restates torchaudio's documented Spectrogram / MelScale / AmplitudeToDB / create_dct / compute_deltas; it has
 * never been compared with a torchaudio binary.  For a signal x[0 .. L) and n_freqs = n_fft / 2 + 1:
 *   frame t is centred on c_t = t * hop + offset and reads xr[c_t - n_fft / 2 + n], n < n_fft, xr = x reflected without
 *     repeating the edge sample (i < 0 -> -i, i >= L -> 2 (L - 1) - i; needs L > n_fft / 2);
 *   w[n] = 0.5 - 0.5 cos(2 pi n / n_fft);   P[t][k] = | sum_n w[n] xr_t[n] e^(-2 pi i ((n k) mod n_fft) / n_fft) |^2, k < n_freqs;
 *   fb[k][m] = max(0, min(-(f[m] - a[k]) / (f[m+1] - f[m]), (f[m+2] - a[k]) / (f[m+2] - f[m+1]))), a = linspace(0, sample_rate / 2
 *     (integer division), n_freqs), f = the inverse of mel(.) = 2595 log10(1 + . / 700) on linspace(mel(f_min), mel(f_max), n_mels + 2);
 *   D = 10 log10(max(P fb, 1e-10)), then D = max(D, max(D) - top_db) with the outer maximum over one signal (floor_mode 1), over
 *     every signal of the call (2), or no clamp (0);
 *   mel output: D [frames][n_mels];   mfcc output: C[t][k] = sum_m D[t][m] dct[k][m], k < n_out,
 *     dct[k][m] = cos(pi / n_mels (m + 0.5) k) sqrt(2 / n_mels), row 0 times 1 / sqrt(2);
 *   deltas: d[t] = ((c[t+1] - c[t-1]) + 2 (c[t+2] - c[t-2])) / 10, t +- j clamped to the signal's frames.
 * Samples are converted exactly, every table is built on the host in double, every sum and the log10 are f64, and one rounding
 * to f32 happens at the store.  No float atomic; a frame's order of summation depends on (n_fft, n_freqs, n_mels) alone: the
 * same call gives the same bits and, with floor_mode 0 or 1, a signal in a pack gives the bits it gives alone.
 *
 * Limits: 32 <= n_fft <= 512, 1 <= hop <= n_fft, 0 <= offset <= hop, 1 <= n_mels <= 512, 1 <= n_out <= n_mels, count >= 1.
 * Anything else, and a shortest signal (min_len, the caller's host value) of n_fft / 2 samples or fewer, returns CPC_ERR_INVALID
 * with a message before any launch; the size queries return 0.
 *
 * mfcc_tables_doubles / mfcc_tables_host: the one table buffer the kernels read, in HOST memory, `capacity` doubles:
 *   window [Wp] | cos [Hp][Fp] | sin [Hp][Fp] | fb [Fp][Mp] | dct transposed [n_mels][n_out], one behind the other, with
 *   Wp = n_fft rounded up to 4, Hp = n_freqs rounded up to 4, Fp = n_freqs rounded up to 16, Mp = n_mels rounded up to 16, the
 *   padding zero.  Only the twiddle rows n <= n_fft / 2 exist: cos is even and sin odd about n_fft / 2, and the kernel folds the
 *   windowed sample n_fft - n onto n before the product.  The caller copies the buffer to the device.
 * mfcc_frame_tile: frames per workgroup (16).  Signal i owns the tiles tile_start[i] .. tile_start[i + 1), ceil(n_frames[i] / tile)
 *   of them; total_tiles = tile_start[count].
 * melspec_db: `count` signals in one launch, signal i = x[in_off[i] .. in_off[i] + in_len[i]) of a flat DEVICE vector of x_total
 *   floats; in_off, in_len, n_frames [count] and tile_start [count + 1] are int64 DEVICE tables.  Leaves the unrounded dB rows, the
 *   tile maxima and the floors in scratch (cpc_melspec_scratch_bytes(total_tiles, count, n_mels) bytes) for mfcc_finish.  A table
 *   entry that leaves x is read as silence; nothing outside x is read.
 * mfcc_finish: out[(row_off[i] + t) * ldo + k] for t < n_frames[i], k < n_out (want_dct != 0: the MFCCs; 0: the dB rows,
 *   n_out == n_mels); rows outside [0, out_rows) are not written, nor is anything else of out.  Same scratch, tables and floor_mode.
 * deltas: out[(row_off[i] + t) * ldo + c] = d[t] of in[(row_off[i] + t) * ldi + c], c < cols; in and out may be column ranges of
 *   one buffer that do not overlap.  max_frames: the largest n_frames (host value: it sizes the grid); count <= 65535.
 * ------------------------------------------------------------------------------------------ */
long cpc_mfcc_tables_doubles(int n_fft, int n_mels, int n_out);
int cpc_mfcc_tables_host(int n_fft, int n_mels, int n_out, int sample_rate, double f_min, double f_max, double *tables_host,
                         long capacity);
int cpc_mfcc_frame_tile(void);
size_t cpc_melspec_scratch_bytes(long total_tiles, int count, int n_mels);
int cpc_melspec_db(const float *x, long x_total, const long *in_off, const long *in_len, const long *n_frames,
                   const long *tile_start, int count, long total_tiles, long min_len, int n_fft, int hop, int offset, int n_mels,
                   const double *tables, int floor_mode, double top_db, void *scratch, size_t scratch_bytes, cpc_stream_t stream);
int cpc_mfcc_finish(const void *scratch, size_t scratch_bytes, const long *n_frames, const long *row_off, const long *tile_start,
                    int count, long total_tiles, int n_fft, int n_mels, int n_out, int want_dct, const double *tables,
                    int floor_mode, float *out, long ldo, long out_rows, cpc_stream_t stream);
int cpc_deltas(const float *in, long ldi, float *out, long ldo, int cols, const long *n_frames, const long *row_off, int count,
               long max_frames, long rows_total, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Loss heads of the linear-separability probe (cpc/eval/linear_separability.py and the supervised criteria of
 * cpc/criterion/criterion.py of the reference).  All pointers are DEVICE pointers, row-major and contiguous; labels, targets and
 * lengths are int64 (torch.long).  No float atomic: every result is bitwise reproducible.  The logits come from cpc_gemm_nt
 * (with its bias), the weight and feature gradients from cpc_gemm_tn / cpc_gemm_nt.
 *
 * cpc_probe_xent: softmax cross-entropy of logits [n][c] (1 <= c <= 2^20) against labels [n]:  nll[i] = lse_i - x[i][label_i],
 *   correct[i] = (argmax_i == label_i) with the LOWEST index among equal maxima (predictions.max(1)[1]),
 *   loss[0] = sum_i nll[i] / n (fixed-order f32 sum), acc[0] = (number correct) / n in double.  want_grad != 0: the logits
 *   are overwritten by dlogits = (softmax - onehot) / n.  A label outside [0, c) gives nll NaN and counts as wrong.
 * cpc_probe_head_backward: dlogits [n][c] *= dloss[0] when dloss is not NULL (the loss's incoming gradient, read on the
 *   device), then db[j] = sum_i dlogits[i][j] (fixed order) when db is not NULL.  scratch: cpc_probe_xent_backward_scratch_bytes(c).
 * cpc_probe_ctc: nn.CTCLoss(blank = k - 1, reduction = 'mean', zero_infinity = True) of log_softmax(logits) for logits
 *   [b][t][k] (b <= 65535, t <= 1024, 2 <= k <= 65536), every input length t, targets [b][max_l] (max_l <= t, padding ignored)
 *   and lengths [b]:  nll[i] = -log p_i (0 when no alignment exists), loss[0] = (sum_i nll[i] / max(L_i, 1)) / b.  dlogits (may
 *   be NULL, may alias logits) = (softmax - occupancy) / (b * max(L_i, 1)), 0 for an infeasible sequence.  A length outside
 *   [0, max_l] or a label outside [0, k - 1) gives that sequence NaN loss and gradient.  alpha and beta are computed in f64.
 *   It is cpc_ctc_loss (below) without input lengths and with the mean: the same kernels (since version 122; b <= 65535 because
 *   their gradient grid has the sequence on its second axis).
 *   scratch: cpc_probe_ctc_scratch_bytes(b, t, max_l) = cpc_ctc_loss_scratch_bytes(b, t, max_l) since version 122 (before: f64
 *   [b][t][2 max_l + 1] alone); 0, without a message, for sizes outside the limits above.
 * cpc_probe_collapse: collapseLabelChain (cpc/criterion/seq_alignment.py) of labels [b][t]: consecutive repeats removed,
 *   out [b][ldo] (ldo >= t) zero padded, lengths [b].
 * ------------------------------------------------------------------------------------------ */
int cpc_probe_xent(float *logits, const int64_t *labels, long n, int c, int want_grad, float *nll, int *correct, float *loss,
                   double *acc, cpc_stream_t stream);
size_t cpc_probe_xent_backward_scratch_bytes(int c);
int cpc_probe_head_backward(float *dlogits, long n, int c, const float *dloss, float *db, void *scratch, size_t scratch_bytes,
                            cpc_stream_t stream);
size_t cpc_probe_ctc_scratch_bytes(int b, int t, int max_l);
int cpc_probe_ctc(const float *logits, int b, int t, int k, const int64_t *targets, int max_l, const int64_t *lengths, float *nll,
                  float *loss, float *dlogits, void *scratch, size_t scratch_bytes, cpc_stream_t stream);
int cpc_probe_collapse(const int64_t *labels, int b, int t, int64_t *out, long ldo, int64_t *lengths, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Audio augmentation on device batches (cpc/data_augmentation.py; cpc2_amd/data_augmentation.py).  Every pointer is a DEVICE
 * pointer.  An operand given as (vector, total, offsets) is read straight out of a flat vector: window i is
 * vector[offsets[i] .. offsets[i] + window), zeros outside [0, total); with offsets == NULL the operand already is a
 * [batch][window] buffer (total is then ignored).  No float atomics: two launches on the same inputs give the same bits.
 * version 111.
 * augment_additive: out[i] = peak(e(speech_i) + gain[i] * e(n_i)), e(w) = w / (sqrt(mean(w^2)) + 1e-8),
 *   peak(m) = m / (max|m| + 1e-8); n_i = noise_i / (max|noise_i| + 1e-8) when noise_peak_norm (the noise data set's
 *   PeakNorm), else noise_i.  One launch per batch; windows of up to 32768 samples are read from global memory once.
 * augment_peak_norm: out[i] = w_i / (max|w_i| + 1e-8); out may be the source buffer.
 * augment_fir: y_i[t] = sum_{k <= t, k < ir_len[i]} ir[ir_off[i] + k] * x_i[t - k] for t < window (the causal convolution cut
 *   to the input length), then out[i] = y_i / (max|y_i| + 1e-8).  ir_len[i] == 0 leaves window i as it is apart from that
 *   normalisation; taps beyond `window` or beyond ir_total are never read.  x is a [batch][window] buffer and must not be out.
 *   scratch: cpc_augment_fir_scratch_bytes(batch, window).
 * augment_time_dropout: x[i][start[i] .. start[i] + length[i]) = 0 (clipped to the window), in place; nothing else is written.
 * ------------------------------------------------------------------------------------------ */
int cpc_augment_additive(const float *speech, long speech_total, const long *speech_off, const float *noise, long noise_total,
                         const long *noise_off, int noise_peak_norm, const float *gain, float *out, int batch, int window,
                         cpc_stream_t stream);
int cpc_augment_peak_norm(const float *src, long src_total, const long *src_off, float *out, int batch, int window,
                          cpc_stream_t stream);
size_t cpc_augment_fir_scratch_bytes(int batch, int window);
int cpc_augment_fir(const float *x, const float *ir, long ir_total, const long *ir_off, const int *ir_len, float *out,
                    void *scratch, size_t scratch_bytes, int batch, int window, cpc_stream_t stream);
int cpc_augment_time_dropout(float *x, const long *start, const long *length, int batch, int window, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Pitch shift of windows by a whole number of cents (the `pitch_wsola` augmentation; cpc2_amd/data_augmentation.py
 * PitchShiftAugment, csrc/pitch.hip).  version 123.  The reference's PitchAugment is a sox effect chain (pitch + rate + dither)
 * that cannot be pinned to anything here; this is THIS LIBRARY'S definition of a pitch shift.  It is not sox's algorithm, it adds no
 * dither, and its agreement with sox is unmeasured.  The constants are in samples and mean what they say at 16 kHz only; the three
 * times are this library's choice.
 *   S = 1312 (segment, 82 ms)  O = 192 (overlap, 12 ms)  R = 234 (search candidates, 14.68 ms)  Ho = S - O = 1120 (output hop)
 *   L = 6 (sinc half-width in zero crossings)  rolloff 0.99
 * Window i is x[0 .. W) of the source (f32), read as ZERO outside [0, W) -- whatever lies beside it in the vector -- and outside
 * the vector.  r = ratio[i] (the caller's 2 ** (cents[i] / 1200), in double), c = cutoff[i] (0.99 min(1, 1 / r)).
 * cents[i] == 0: out[i] = the window, bit for bit.  Otherwise:
 *   Stage 1, a time stretch by r (WSOLA) stated as a function s(m), m >= 0; segment j = m / Ho, k = m - j Ho.
 *     q_0 = 0.  For j >= 1: p_j = nominal[i][j] (the caller's floor(j Ho / r + 0.5), in double -- no division on the device); the
 *     template is t[k] = x[q_{j-1} + Ho + k], k < O (raw input, the tail of the previous segment); the candidates are
 *     p_j - R / 2 + d, d = 0 .. R - 1; the cost D(d) = sum_{k < O} (x[cand + k] - t[k])^2 is taken in double: both values
 *     converted, subtracted, squared, added with k ascending, nothing contracted.  q_j = the candidate of the smallest D, the
 *     lowest d on a tie.
 *     s(m) = x[q_j + k] for k >= O or j == 0, else a + (k / O) (b - a) with a = x[q_{j-1} + Ho + k], b = x[q_j + k].
 *   Stage 2, resampling by r: out[i][n] = sum_{m >= 0} h(n r - m) s(m), n in [0, W), h(t) = c sinc(c t) cos(pi c t / (2 L))^2 for
 *     |c t| < L and 0 elsewhere (sinc(u) = sin(pi u) / (pi u)).
 * q[i][j] receives q_j for every j < segments and equals the statement's, exactly.  The weights are evaluated in double and
 * rounded once to f32 (sin and cos at an output's first tap, turned tap by tap in double from there; the tap nearest the centre
 * evaluates its sine directly), the cross-fade is taken in double and rounded once, and the sum is ONE f32 fmaf chain with m
 * ascending: an output's bits do not depend on the launch geometry, on the other windows or on what surrounds the window.
 * `segments` (the row length of nominal and q) must cover every tap: ceil((ceil(W r) + 16) / Ho) for the largest r of the batch;
 * segments nobody reads cost time only.  cents_bound is the HOST's bound on |cents[i]| (the device array is not read back).
 * Refused with CPC_ERR_INVALID, nothing launched and nothing written: window <= 0, segments <= 0, cents_bound > 1200 (or < 0),
 * batch < 0 or > 65535, a null pointer with batch > 0, out == src.  batch == 0 is a no-op.  The source is given as the other
 * augment entries take it: (vector, total, offsets), or a [batch][window] buffer with offsets == NULL.
 * ------------------------------------------------------------------------------------------ */
int cpc_augment_pitch(const float *src, long src_total, const long *src_off, const double *ratio, const double *cutoff,
                      const int *cents, int cents_bound, const int *nominal, int segments, float *out, int *q, int batch,
                      int window, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Artificial reverberation of windows (the `freeverb` augmentation; cpc2_amd/data_augmentation.py FreeverbAugment,
 * csrc/freeverb.hip).  version 125.  The reference's ReverbAugment is a sox effect chain (`reverb`) that is not available; the
 * algorithm behind it is the public-domain Freeverb network, and this is THIS LIBRARY'S statement of it: eight parallel feedback
 * comb filters with a one-pole low-pass in the loop, then four all-pass filters in series.  Its agreement with sox's output is
 * unmeasured.  The effect is defined at 16 kHz only.  The caller's tables (data_augmentation.freeverb_tables, in double):
 *   COMB = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)  ALLPASS = (225, 341, 441, 556)  (samples at 44.1 kHz)
 *   rho = 16000 / 44100;  per window a room size rs in [0, 100):  scale = rs / 100 * 0.9 + 0.1
 *   comb_len[i][c] = D[c] = int(scale * rho * COMB[c] + 0.5)      allpass_len[a] = A[a] = int(rho * ALLPASS[a] + 0.5) = (82, 124, 160, 202)
 *   a = -1 / ln(0.7);  b = 100 / (ln(0.02) * a + 1);  feedback fb = 1 - exp((reverberance - b) / (a * b))
 *   damping dmp = hf_damping / 100 * 0.3 + 0.2;  gain g = 0.015 * 10 ** (wet_gain_dB / 20);  fb, dmp, g rounded once to f32
 *   (reverberance = hf_damping = 100, the reference's reverb(100, 100, room): fb = 0.98, dmp = 0.5)
 * Window i is x[0 .. W) of the source (f32); nothing outside it is read, whatever lies beside it in the vector.  All state is
 * zero at n = 0.  For n = 0 .. W - 1, every operation in f32 and in this order, nothing contracted:
 *   u = g * x[n];  acc = 0
 *   for c in 0..7:  o = line_c[p_c];  s_c = o + (s_c - o) * dmp;  line_c[p_c] = u + s_c * fb;  p_c = (p_c + 1) % D[c];  acc = acc + o
 *   v = acc
 *   for a in 0..3:  o = line_a[p_a];  line_a[p_a] = v + o * 0.5;  v = o - v;  p_a = (p_a + 1) % A[a]
 *   out[i][n] = x[n] + v
 * No pre-delay, no tone filters, no stereo spread (one mono bank), no dither, no clipping, no peak normalisation; the tail beyond
 * W is cut off.  The kernel performs exactly these operations (one workgroup per window, the twelve lines in LDS), so out equals a
 * float32 evaluation of the statement and a window's bits depend on nothing else in the batch, the vector or the launch.
 * comb_len is a DEVICE table [batch][8]; len_bound is the HOST's bound on its entries (the table is not read back) and sizes the
 * lines: the kernel clamps every entry into [1, len_bound].  allpass_len[4] is a HOST array.
 * Refused with CPC_ERR_INVALID, nothing launched and nothing written: window <= 0, batch < 0 or > 65535, len_bound or an all-pass
 * length outside [1, 1024], feedback outside [0, 1), damping outside [0, 1], a scalar that is not finite, a null pointer with
 * batch > 0 (allpass_len always), out == src.  batch == 0 is a no-op.  The source is given as the other augment entries take it:
 * (vector, total, offsets) with zeros outside [0, total), or a [batch][window] buffer with offsets == NULL.
 * ------------------------------------------------------------------------------------------ */
int cpc_augment_freeverb(const float *src, long src_total, const long *src_off, const int *comb_len, int len_bound,
                         const int *allpass_len, float feedback, float damping, float gain, float *out, int batch, int window,
                         cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Band-reject filtering of windows (the `bandreject_sinc` augmentation; cpc2_amd/data_augmentation.py BandrejectSincAugment,
 * csrc/bandreject.hip).  version 127.  The reference's BandrejectAugment is a sox effect chain (`sinc -a 120 high-low`, then
 * `dither`) that is not available; the textbook filter behind it is a Kaiser-windowed sinc band-reject FIR, and this is THIS
 * LIBRARY'S statement of one.  Its agreement with sox's output is unmeasured, and there is no dither.  The caller's scalars
 * (data_augmentation.bandreject_tables, in double), from an attenuation A in dB and a transition width tbw in Hz:
 *   beta = 0.1102 (A - 8.7);  dw = 2 pi tbw / sr;  M = ceil((A - 7.95) / (2.285 dw));  half = H = (M + 1) / 2 (integer division)
 *   (A = 120, tbw = 400, sr = 16000: beta = 12.26526, M = 313, H = 157, 2 H + 1 = 315 taps)
 * band is a DEVICE table [batch][2] of doubles, (low, high) in Hz per window, 0 <= low <= high <= sr / 2.  For j = -H .. H, in f64:
 *   w[j]    = I0(beta sqrt(1 - (j / H)^2)) / I0(beta)
 *   lp_f[j] = (2 f / sr) sinc(2 f j / sr)          sinc(u) = sin(pi u) / (pi u), sinc(0) = 1
 *   h[j]    = [j == 0] - w[j] (lp_high[j] - lp_low[j])                          (no renormalisation)
 *   out[i][t] = round_f32( sum_{j = -H .. H} h[j] x[t - j] ),  t = 0 .. window - 1
 * Window i is x[0 .. W) of the source (f32) and reads as ZERO outside its own [0, W), whatever lies beside it in the vector.
 * Every product and sum is in f64 in one fixed order -- h[0] x[t], then fma(h[j], x[t - j] + x[t + j], .) for j = 1 .. H, the sum
 * of two f32 values being exact in f64 -- and the result is rounded once, at the store.  On the device I0 is its power series, summed
 * until a term falls below 2^-60 of the sum, and the sine takes the argument reduced exactly (u - 2 rint(u / 2)): a tap is within
 * 2^-40 of its value.  No dither, no clipping, no peak normalisation; the output has the input's length.  A row with low == high
 * is the identity and is COPIED with no arithmetic, and so is a row whose pair is no band (low < 0, low > high, high > sr / 2, a
 * NaN): the table lives on the device and is not read back.  A row's bits depend on nothing else in the batch, the vector or the
 * launch.
 *   cpc_bandreject_tile      outputs per workgroup (the seams of the filter kernel, for tests)
 *   cpc_bandreject_max_half  the largest half length, 1024
 *   cpc_bandreject_taps      taps [batch][half + 1] (DEVICE, doubles) receives h[0 .. half] of every row, from the same device
 *                            function the filter kernel designs its taps with; a copied row reads 1, 0, 0, ...
 * Both entries refuse with CPC_ERR_INVALID, nothing launched and nothing written: window <= 0, batch < 0 or > 65535, half outside
 * [1, 1024], beta not finite or outside [0, 50], sample_rate not finite or <= 0, a null pointer with batch > 0, out == src, offsets
 * without the vector's length.  batch == 0 is a no-op.  The source is given as the other augment entries take it: (vector, total,
 * offsets) with zeros outside [0, total), or a [batch][window] buffer with offsets == NULL.
 * ------------------------------------------------------------------------------------------ */
int cpc_bandreject_tile(void);
int cpc_bandreject_max_half(void);
int cpc_bandreject_taps(const double *band, int batch, int half, double beta, double sample_rate, double *taps,
                        cpc_stream_t stream);
int cpc_augment_bandreject(const float *src, long src_total, const long *src_off, const double *band, int half, double beta,
                           double sample_rate, float *out, int batch, int window, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Sample-rate conversion (torchaudio's sinc_interp_hann resampler, the transform of the reference's
 * cpc/eval/utils/adjust_sample_rate.py; cpc2_amd/audio.py: resample, resample_pack, save_wav).  version 112.
 *   g = gcd(orig_freq, new_freq), o = orig_freq / g, n = new_freq / g, base = min(o, n) * rolloff,
 *   w = ceil(lowpass_filter_width * o / base), taps = 2 w + o,
 *   h[p][j] = sinc(t) * cos(t pi / (2 width))^2 * base / o with t = clamp((-p / n + (j - w) / o) * base, -width, +width),
 *   y[f n + p] = sum_j h[p][j] * xp[f o + j], xp = x with w zeros in front and w + o zeros behind; a signal of L samples
 *   gives ceil(n L / o).
 * resample_plan: o, n, w, taps of a pair of rates (host; nothing is launched).
 * resample_table_host: fills table_host[p * taps + j] (HOST memory, n * taps floats; capacity = the floats it holds), computed
 *   in double and rounded once to f32.  The caller copies it to the device and passes it to cpc_resample.
 * resample: `count` signals in one launch.  Signal i is x[in_off[i] .. in_off[i] + in_len[i]) of a flat device vector of
 *   x_total floats and leaves y[out_off[i] .. out_off[i] + ceil(n in_len[i] / o)); nothing else of y is written and a signal never
 *   reads outside its own samples (zeros there).  in_off, in_len, out_off: int64 DEVICE tables; max_len: the largest in_len
 *   (host value: it sizes the grid; longer signals would be cut).  A signal whose table entry leaves x is skipped.  All sample
 *   indices are 64-bit.  Each output is one f32 fmaf chain over j ascending: the bits do not depend on the pack or the tiling.
 *   Refused (CPC_ERR_INVALID): a reduced ratio whose 2 w + 2 o exceeds a workgroup's 8192-float signal segment.
 * resample_to_pcm16: q[i] = (int16) clamp(rint(32768 * y[i]), -32768, 32767), ties to even; *clamped (a device counter the
 *   caller zeroes) is increased by the number of samples the clamp changed.
 * ------------------------------------------------------------------------------------------ */
int cpc_resample_plan(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, int *o, int *n, int *w, int *taps);
int cpc_resample_table_host(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, float *table_host, long capacity);
int cpc_resample(const float *x, long x_total, const long *in_off, const long *in_len, int count, long max_len, const float *table,
                 int o, int n, int w, float *y, long y_total, const long *out_off, cpc_stream_t stream);
int cpc_resample_to_pcm16(const float *y, long count, int16_t *q, unsigned long long *clamped, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Decimal text of a device matrix (the `fea` lines of the reference's cpc/eval/build_zeroSpeech_features.py;
 * cpc2_amd/text.py: format_rows).  version 113.
 *   row r of the text = prefix[r] ' ' v(r, 0) ' ' v(r, 1) ... v(r, cols - 1) '\n'; without prefixes a row starts at its first value.
 * text_format_f32: value i of `count` floats -> slots[3 i .. 3 i + 3) (24 bytes, the text from byte 0 on, zeros behind it) and
 *   len[i] (1 .. 23).  The text is CPython's repr(float(v)) byte for byte: the shortest decimal string that reads back as the
 *   double equal to v, the closest among the shortest, an exact tie to the even digit; positional with the first digit's decimal
 *   exponent in [-4, 16) ("0.0001", "1.0", "1000000000000000.0"), else d[.ddd]e+XX / e-XX; "-0.0", "inf", "-inf", "nan".
 *   Integer arithmetic throughout (csrc/text_digits.h).
 * text_format_i64: the same slots for int64 values as plain decimal integers (at most 20 bytes).
 * text_row_bytes: row_bytes[r] = the bytes of row r: its texts, a blank or the newline behind each, and with prefixes
 *   (prefix_off: int64 DEVICE table of rows + 1 offsets into `prefix`; NULL: none) the prefix and the blank behind it.  The caller's
 *   exclusive scan of row_bytes is row_off; its total out_total.
 * text_pack: writes the rows to out[row_off[r] ..).  A row whose offsets do not fit out_total is not written.  All offsets are
 *   64-bit; 1 <= cols < 2^26.
 * ------------------------------------------------------------------------------------------ */
int cpc_text_format_f32(const float *x, long count, unsigned long long *slots, unsigned char *len, cpc_stream_t stream);
int cpc_text_format_i64(const long *x, long count, unsigned long long *slots, unsigned char *len, cpc_stream_t stream);
int cpc_text_row_bytes(const unsigned char *len, long rows, int cols, const long *prefix_off, long *row_bytes, cpc_stream_t stream);
int cpc_text_pack(const unsigned long long *slots, const unsigned char *len, long rows, int cols, const unsigned char *prefix,
                  const long *prefix_off, const long *row_off, unsigned char *out, long out_total, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Phone error rate of a CTC probe (cpc/criterion/seq_alignment.py of the reference; cpc2_amd/seq_alignment.py).  version 116.
 * Every pointer is a DEVICE pointer, row-major and contiguous; labels and lengths are int32.
 *
 * cpc_ctc_beam_search: beam_search (seq_alignment.py:11-61) of n sequences.  probs [n][t_max][p] are probabilities (not logs),
 *   lengths[i] the frames of sequence i to decode (clamped to [0, t_max]; rows beyond it are never read), blank any class in
 *   [0, p).  Limits: 1 <= n_keep <= 128, 2 <= p <= 128 (a frame's n_keep * p candidates are held in LDS), t_max <= 8192;
 *   anything else is CPC_ERR_INVALID.  With R = n_keep (best_only == 0) or R = 1 (best_only != 0, the best prefix only):
 *     scores [n][R]        pb + pnb of the kept prefixes, best first; 0 behind the last one
 *     out_lengths [n][R]   their label counts; 0 behind the last one
 *     labels [n][R][t_max] their labels, -1 behind each prefix's last label
 *     counts [n]           how many of the R rows hold a prefix (fewer than n_keep exist only in the first frames)
 *     ties [n]             1 when some frame met two equal scores among its first n_keep + 1 candidates, else 0
 *   The arithmetic is the reference's, operation for operation, in f32 with subnormals kept and no fused multiply-add:
 *   pb' = (pnb + pb) p[blank]; pnb' = pnb p[last] for the prefix itself, plus pb p[c] when c repeats the last label of the
 *   prefix it extends and (pb + pnb) p[c] otherwise; score = pb + pnb.  Without ties the output equals the reference's bit for
 *   bit.  EQUAL scores are ordered by (rank of the extended prefix in the previous frame's beam, symbol), an unextended prefix
 *   counting as its own rank with symbol = blank; the reference orders them by the prefixes' decimal strings, which is not
 *   reproduced.  The order is a function of the inputs alone: two launches give the same bytes.
 *   scratch: cpc_ctc_beam_search_scratch_bytes(n, t_max, p, n_keep) (per sequence a trie of at most 1 + t_max * n_keep prefixes
 *   and its (parent, symbol) table; 0 with a message for sizes outside the limits); too little gives CPC_ERR_WORKSPACE.
 * cpc_align_score: NeedlemanWunschAlignScore (seq_alignment.py:89-112) of n pairs without its normalisation:
 *   score[i] = -H[len1[i]][len2[i]] with H[a][0] = a d, H[0][b] = b d and
 *   H[a+1][b+1] = max(H[a][b] + (seq1[i][a] == seq2[i][b] ? r : m), H[a+1][b] + d, H[a][b+1] + d): integers, exact.
 *   seq1 [n][ld1], seq2 [n][ld2] (1 <= ld <= 4096; lengths clamped to [0, ld]; padding is not read), |d|, |m|, |r| <= 32768.
 *   get_seq_PER of the reference is d = m = -1, r = 0 and score / len1.
 * ------------------------------------------------------------------------------------------ */
size_t cpc_ctc_beam_search_scratch_bytes(int n, int t_max, int p, int n_keep);
int cpc_ctc_beam_search(const float *probs, const int *lengths, int n, int t_max, int p, int n_keep, int blank, int best_only,
                        float *scores, int *out_lengths, int *labels, int *counts, int *ties, void *scratch, size_t scratch_bytes,
                        cpc_stream_t stream);
int cpc_align_score(const int *seq1, long ld1, const int *len1, const int *seq2, long ld2, const int *len2, int n, int d, int m,
                    int r, int *score, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The whole-utterance CTC phone recogniser (CTCphone_criterion of the reference's cpc/eval/common_voices_eval.py;
 * cpc2_amd/eval/common_voices_eval.py).  version 117.  Every pointer is a DEVICE pointer, row-major and contiguous; lengths,
 * offsets and targets are int64 (torch.long).  No float atomic in these kernels: two launches give the same bits.
 *
 * cpc_ctc_loss: nn.CTCLoss(blank = k - 1, reduction, zero_infinity = True) of log_softmax(logits) for logits [b][t_max][k] with
 *   an input length per sequence: in_lengths [b], targets [b][max_l] (padding ignored: the padded width does not matter) and
 *   tgt_lengths [b].  reduction: 0 = sum, 1 = mean.  nll[i] = -log p_i; loss[0] = sum_i nll[i], or for the mean
 *   (sum_i nll[i] / max(L_i, 1)) / b.  dlogits (may be NULL, may alias logits) = (softmax - occupancy) on the frames
 *   < in_lengths[i], divided by b max(L_i, 1) for the mean.  Frames at or beyond in_lengths[i] are never read and get gradient
 *   exactly 0.  A sequence without an alignment (an input length of 0 included) has nll 0 and gradient 0.  An input length
 *   outside [0, t_max], a target length outside [0, max_l] or a label outside [0, k - 1) gives that sequence NaN nll and NaN
 *   in all of its dlogits, as cpc_probe_ctc does.  alpha and beta are f64 in log space, fused with the log-softmax (one workgroup
 *   per sequence); the gradient is a second launch over (sequence, 1024 elements) workgroups; b <= 65535.  cpc_probe_ctc is
 *   these kernels with every input length = t_max and the mean, so the two give the same bits there.
 *   Limits: 1 <= t_max <= 4096 (164 s of audio behind a stride-4 head), 2 <= k <= 65536, 0 <= max_l <= min(t_max, 1024): the
 *   2 max_l + 1 extended states of a sequence are held in LDS at 20 bytes each, 40 KB at 1024 labels.
 *   scratch: cpc_ctc_loss_scratch_bytes(b, t_max, max_l) (f64 [b][t_max] + [b][t_max][2 max_l + 1] + [b], int [b]; 0 with a message in
 *   cpc_last_error for sizes outside the limits).
 * cpc_seqnorm_len_forward: the seqNorm branch of getPrediction.  x [b][s][h], lengths [b]: m = the mean and v = the unbiased
 *   variance of the frames < lengths[i] per (i, channel), then y = (x - m) / sqrt(v + eps) on ALL s frames; mean [b][h] and rstd
 *   [b][h] = 1 / sqrt(v + eps) are saved.  The statistics are summed in f64 in a fixed order.  lengths[i] = 1 gives NaN (0 / 0,
 *   as torch.var); a length outside [1, s] is invalid and gives that utterance NaN.
 * cpc_seqnorm_len_backward: the exact gradient from dy, the forward's y and rstd:
 *   dx[f] = rstd (dy[f] - [f < len] (A / len + B y[f] / (len - 1))), A = sum_f dy[f], B = sum_f dy[f] y[f] over ALL s frames
 *   (every frame's dy feeds dm and dv; only the frames < len receive those terms).
 * cpc_conv_head_backward_data: dx of Conv1d(h, c, ks, stride = ks / 2) on channel-last data.  dout [b][P][c] with
 *   P = (s - ks) / stride + 1, wp [c][ks][h] (the weight repacked, taps before channels), dx [b][s][h]:
 *   dx[i][stride j + u] = dout[i][j] . wp[:, u] + dout[i][j - 1] . wp[:, stride + u] for u < stride (a term whose output frame
 *   does not exist is 0); every element of dx is written once.  Supported: every even ks >= 2 (the reference's default is 8),
 *   ks <= s <= 262140.  The weight gradient takes no entry of its own: it is cpc_gemm_tn over the overlapping rows of the features
 *   (row j of an utterance = the ks h floats from frame stride j on: ldb = stride h), whose K split is summed from slabs in order.
 * cpc_conv_head_forward: out [b][P][c] = the same layer's outputs.  No kernel of its own: it is the product of cpc_gemm_nt, once
 *   per utterance (its rows end where the utterance ends), reading x [b][s][h] in place with lda = stride h against wp [c][ks][h]
 *   (bias [c] may be NULL); the unfolded [b][P][ks h] matrix never exists.  What it adds to cpc_gemm_nt is the lent scratch: with
 *   ks h >= 2048 and few output tiles that product splits K, and the public entry then adds the parts with fp32 atomics; here they
 *   go to slabs that are summed in a fixed order, so two launches give the same bits.
 *   scratch: cpc_conv_head_forward_scratch_bytes(b, s, h, c, ks) (0 with a message for sizes outside the limits).
 * cpc_gather_utterances: out [n][max_len] = the zero-padded batch of whole utterances:
 *   out[i][p] = pack[offsets[i] + roffset[i] + p] for p < lengths[i] - roffset[i], 0 behind it (roffset NULL: 0 everywhere).
 *   `pack` holds `total` floats; an item that leaves it, or whose roffset is outside [0, lengths[i]], becomes a row of zeros.
 * ------------------------------------------------------------------------------------------ */
size_t cpc_ctc_loss_scratch_bytes(int b, int t_max, int max_l);
int cpc_ctc_loss(const float *logits, int b, int t_max, int k, const int64_t *in_lengths, const int64_t *targets, int max_l,
                 const int64_t *tgt_lengths, int reduction, float *nll, float *loss, float *dlogits, void *scratch,
                 size_t scratch_bytes, cpc_stream_t stream);
int cpc_seqnorm_len_forward(const float *x, const int64_t *lengths, int b, int s, int h, float eps, float *y, float *mean,
                            float *rstd, cpc_stream_t stream);
int cpc_seqnorm_len_backward(const float *dy, const float *y, const float *rstd, const int64_t *lengths, int b, int s, int h,
                             float *dx, cpc_stream_t stream);
size_t cpc_conv_head_forward_scratch_bytes(int b, int s, int h, int c, int ks);
int cpc_conv_head_forward(const float *x, const float *wp, const float *bias, float *out, int b, int s, int h, int c, int ks,
                          void *scratch, size_t scratch_bytes, cpc_stream_t stream);
int cpc_conv_head_backward_data(const float *dout, const float *wp, int b, int s, int h, int c, int ks, float *dx,
                                cpc_stream_t stream);
int cpc_gather_utterances(const float *pack, long total, const int64_t *offsets, const int64_t *lengths, const int64_t *roffset,
                          float *out, int n, long max_len, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * CTC forced alignment of whole utterances (csrc/ctc_align.hip; cpc2_amd/seq_alignment.py: ctc_forced_align; DESIGN.md section
 * 19).  version 120.  Every pointer is a DEVICE pointer, row-major and contiguous; lengths and targets are int64 (torch.long).
 * The reference has no aligner: the definition below is the specification.  Agreement with torchaudio.functional.forced_align
 * is UNMEASURED.
 *
 * One sequence has logits x [T][k] (f32, T = its input length), targets y[0..L) and blank = k - 1 (the convention of cpc_ctc_loss
 * and cpc_probe_ctc).  Extended states are s in [0, 2 L + 1): sym(s) = blank for even s and y[s / 2] for odd s.  Every alignment
 * emits exactly one symbol per frame, so sum_t lse_t is the same for all paths: the maximisation runs on the raw logits and the
 * normaliser enters only the reported score.  No exp or log occurs inside the recurrence.
 *   Start.  v[0][0] = (double) x[0][blank]; v[0][1] = (double) x[0][y0] when L >= 1; every other state is -inf.
 *   Step.   v[t][s] = max(v[t-1][s], v[t-1][s-1] when s >= 1, v[t-1][s-2] when s is odd, s >= 3 and y[s/2] != y[s/2 - 1])
 *           + (double) x[t][sym(s)].  All values are f64; the max first, then ONE addition (the file is built with
 *           -ffp-contract=off): a host program with the same operation order gives the same bits.
 *   Ties inside a step (equal finite candidates): staying in s wins over s - 1, which wins over s - 2.
 *   End.    State 2 L wins over 2 L - 1 unless v[T-1][2L-1] is strictly larger.  With L = 0 there is only state 0.
 *   ties [b]     1 when a maximum ON THE RETURNED PATH had an equal finite competitor, the choice at the end included; else 0
 *                (0 with status 1 or 2).
 *   status [b]   0 = aligned; 1 = no alignment exists: T < L + #{i : y[i] == y[i-1]}, and T = 0 whatever L (there is no frame to
 *                start from); 2 = an argument of that sequence is invalid: input length outside [0, t_max], target length
 *                outside [0, max_l], or a label outside [0, k - 1).  With status 1 or 2 path is -1 on all t_max frames, both
 *                scores and all of lse are NaN, and first / last / conf are -1 / -1 / NaN.
 *   path [b][t_max]   the state index for t < T, -1 for T <= t < t_max
 *   score [b][2]      score[0] = the path's logit sum v[T-1][end]; score[1] = score[0] - sum_t lse_t, lse_t the f64
 *                     log-sum-exp of frame t, max-shifted as in cpc_ctc_loss (the sum over t in a fixed order)
 *   lse [b][t_max]    optional (may be NULL): lse_t for t < T, NaN behind; cpc_ctc_align_segments needs it
 * cpc_ctc_align_segments: for each token i < L of an aligned sequence first[i] and last[i] = the first and last frame whose state
 *   is 2 i + 1, and conf[i] = the mean over those frames of x[t][y[i]] - lse_t, summed in f64 in frame order and stored as f32.
 *   first, last, conf are [b][max_l]; tokens at or beyond L get -1 / -1 / NaN.  max_l = 0 writes nothing.
 * Limits (those of cpc_ctc_loss): 1 <= t_max <= 4096, 2 <= k <= 65536, 0 <= max_l <= min(t_max, 1024), 1 <= b <= 65535; anything
 *   else is CPC_ERR_INVALID with a message in cpc_last_error, and the scratch query returns 0 with a message.
 *   scratch: cpc_ctc_align_scratch_bytes(b, t_max, max_l) (f64 [b][t_max] + one byte of back-pointer per (frame, state):
 *   [b][t_max][2 max_l + 1], 8.4 MB per sequence at the limit); too little gives CPC_ERR_WORKSPACE.
 * No float atomic: two launches give the same bytes.  Rows of logits at or beyond in_lengths[i] and target padding are never read.
 * ------------------------------------------------------------------------------------------ */
size_t cpc_ctc_align_scratch_bytes(int b, int t_max, int max_l);
int cpc_ctc_align(const float *logits, int b, int t_max, int k, const int64_t *in_lengths, const int64_t *targets, int max_l,
                  const int64_t *tgt_lengths, int *path, double *score, int *status, int *ties, double *lse /* may be NULL */,
                  void *scratch, size_t scratch_bytes, cpc_stream_t stream);
int cpc_ctc_align_segments(const float *logits, int b, int t_max, int k, const int64_t *targets, int max_l, const int64_t *tgt_lengths,
                           const int *path, const int *status, const double *lse, int *first, int *last, float *conf,
                           cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Unsupervised phone segmentation and its counts (csrc/segment.hip; cpc2_amd/segmentation.py).  version 124.
 * Every pointer is a DEVICE pointer.  The reference has no such tool: the definition below is the specification (the recipe of
 * Kreuk et al. 2020 with the R-value of Rasanen et al. 2009; peaks and prominences are those of scipy.signal.find_peaks /
 * peak_prominences with wlen = None).
 *
 * Utterance i has L = lengths[i] frames (int32) of `dim` float32 columns: the rows offsets[i] .. offsets[i] + L - 1 (int64) of
 * x [total_rows][ld], ld >= dim -- the layout of a packed feature buffer.  d, peak_pos and peak_prom are arrays of total_rows entries
 * addressed by the same offsets.
 * cpc_seg_dissimilarity: d[offsets[i] + t] = 1 - dot(x_t, x_t+1) / sqrt(|x_t|^2 |x_t+1|^2) for t < L - 1, and 1 when the product of
 *   the squared norms is 0.  The three sums are f64 sums of exact products: lane j of a wave adds the columns j, j + 64, ... in
 *   order and the 64 partial sums meet in a fixed butterfly; then ONE product, square root, division and subtraction, all f64.
 *   d[t] is a function of the two rows alone and symmetric in them: equal pairs of rows give equal bits wherever they stand.
 *   Slot offsets[i] + L - 1 and slots of no utterance are not written.
 *   status [n_utt]: 0; 2 when the utterance holds a non-finite value (the pairs of that row are NaN, every other pair keeps its
 *   value) or when its rows leave the buffer (length outside [0, max_len], offset < 0, offset + L > total_rows: nothing of it is
 *   read or written).  Other utterances are unaffected.  max_len: no length exceeds it (it sizes the grid), at most 2^20.
 * cpc_seg_boundaries: for each utterance, on the n = max(L - 1, 0) entries of d at its offset:
 *   peaks    index i in [1, n - 2] starts a peak when d[i-1] < d[i] and the run of entries equal to d[i] ends before n with a
 *            smaller entry behind it; the peak's position is (first + last) / 2 of the run (integer division).
 *   prom     of a peak at q: walk left from q while d[i] <= d[q] keeping the minimum, the same to the right;
 *            prom = d[q] - max(left minimum, right minimum): one subtraction of two stored values.
 *   n_peaks [n_utt]; peak_pos / peak_prom: the peaks in increasing order in the first n_peaks slots at the utterance's offset (the
 *            other slots are not written); range [n_utt] = max d - min d (0 when n = 0).
 *   counts [n_utt][k][4] (int32) for threshold thresholds[j] (f64, 1 <= k <= 64): a peak is kept when prom >= thresholds[j] * range
 *            (ONE product; the file is built with -ffp-contract=off) and its boundary frame h = q + 1 is < hyp_limit[i] (NULL: L).
 *            [0] n_hyp = the kept boundaries; [1] hits = the one-to-one matching by two pointers over the two sorted lists (a pair
 *            within tol is a hit and advances both, otherwise the smaller frame advances); [2] hyp_near = kept boundaries with a
 *            reference within tol; [3] ref_near = references with a kept boundary within tol.  The references of utterance i are
 *            ref[ref_offsets[i] .. + ref_counts[i]) (int32 frames in strictly increasing order, ref holds total_ref of them).
 *            ref == NULL: no scoring, [1] .. [3] are 0.
 *   status [n_utt]: 0; 2 when d holds a non-finite value there or an argument of the utterance is invalid (length outside
 *            [0, 2^20], rows or references that leave their buffers): n_peaks 0, range NaN, counts 0, no peak slot written.
 *   Up to cpc_seg_lds_entries() entries of d are staged in LDS; a longer utterance is read in place.  No workspace is needed.
 * Limits: dim >= 1, ld >= dim, 1 <= n_utt <= 2^20, 0 <= tol <= 2^30; anything else is CPC_ERR_INVALID with a message naming the
 *   entry point, before any launch.  No float atomic: two launches give the same bytes.
 * ------------------------------------------------------------------------------------------ */
int cpc_seg_lds_entries(void);
int cpc_seg_dissimilarity(const float *x, long total_rows, long ld, int dim, const int64_t *offsets, const int *lengths, int n_utt,
                          int max_len, double *d, int *status, cpc_stream_t stream);
int cpc_seg_boundaries(const double *d, long total_rows, const int64_t *offsets, const int *lengths, int n_utt,
                       const double *thresholds, int k, const int *ref /* may be NULL */, long total_ref, const int64_t *ref_offsets,
                       const int *ref_counts, const int *hyp_limit /* may be NULL */, int tol, int *n_peaks, int *peak_pos,
                       double *peak_prom, double *range, int *counts, int *status, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Quantized units against frame-level phone labels (csrc/unit_scores.hip; cpc2_amd/unit_scores.py).
 * version 126.  Every pointer is a DEVICE pointer.  The reference has no counterpart: the definition below is the specification.
 * All inputs and outputs are integers and integer sums do not depend on their order: every output EQUALS the definition, bit
 * for bit, on every launch.
 *
 * Utterance i compares L = lengths[i] frames (int32; a value <= 0 compares nothing): the unit of frame f is
 * units[unit_off[i] + f] and its label labels[label_off[i] + f] (int32 packs of n_unit_words and n_label_words words, int64
 * offsets).  The packs are separate because a unit line and a label line of one utterance may differ by a frame or two: the caller
 * passes the common length.  The packs may have gaps and the utterances any order; words outside [off, off + L) are never read.
 * labels == NULL: every frame has label 0 and n_phones must be 1.  An utterance whose frames leave a pack (offset < 0 or
 * offset + L beyond the pack) is not read at all: cpc_unit_counts adds its L frames to `invalid`, cpc_unit_boundaries writes five
 * times -1 for it.
 * cpc_unit_counts ADDS into caller-zeroed tables, so that a corpus goes through in batches:
 *   joint [n_units][n_phones] (int64)  frames with that (unit, phone)
 *   unit_runs [n_units] (int64)        frames f with f == 0 or units[f] != units[f-1], by units[f]: a run never continues across
 *                                      an utterance boundary
 *   phone_runs [n_phones] (int64)      the same for the labels
 *   invalid [1] (int64)                frames whose unit is outside [0, n_units) or whose label is outside [0, n_phones): such a
 *                                      frame is counted nowhere else and never used as an index (the frame behind it still
 *                                      compares itself with it)
 *   form: 0 = chosen from the shape alone: 1 (the whole table in LDS as 32-bit words, flushed once per workgroup) when
 *   n_units * n_phones <= cpc_unit_counts_lds_cells() = 16384, else 2 (64-bit atomics on the table in global memory); 1 or 2 force
 *   a form (1 is refused for a table that does not fit).  Equal cells on adjacent lanes can be folded into one add of their
 *   number: the global form does that and the LDS form does not, which is what was measured to be faster;
 *   + 4 forces no folding, + 8 forces folding (for measurements; same outputs).  The run-start tables live in LDS in both forms.  The table and the run words are dynamic LDS
 *   sized by the shape, at most 132 KiB of the 160 KiB a gfx950 workgroup may take.  The work is cut into chunks of
 *   cpc_unit_counts_chunk() = 4096 compared frames of the concatenated utterances, whatever their lengths.
 *   scratch: cpc_unit_counts_scratch_bytes(n_utt) (the prefix of the lengths; 0 with a message for n_utt outside the limits);
 *   too little gives CPC_ERR_WORKSPACE.
 * cpc_unit_boundaries OVERWRITES out [n_utt][5] (int32) = (n_ref, n_hyp, hits, hyp_near, ref_near) at one tolerance tol in frames:
 *   hypotheses are the frames f in [1, L - 1] with units[f] != units[f-1], references the same for the labels (none when labels ==
 *   NULL); hits = the one-to-one matching by two pointers over the two sorted lists (a pair within tol is a hit and advances both,
 *   otherwise the smaller frame advances); hyp_near = hypotheses with a reference within tol, ref_near = references with a
 *   hypothesis within tol.  L <= 1: five zeros.  One wave per utterance; the matching is cpc_seg_boundaries', kept as a second copy
 *   so that segment.hip's code does not move.  total_frames: at least the sum of the lengths (it sizes the two lists in scratch;
 *   an utterance whose lists would not fit gets five times -1).  scratch: cpc_unit_boundaries_scratch_bytes(n_utt, total_frames).
 * Limits: 0 <= n_utt <= 2^20 (n_utt == 0: nothing is done, CPC_OK), 1 <= n_units <= 16384, 1 <= n_phones <= 1024, 0 <= tol <= 2^30,
 *   pack sizes and total_frames >= 0; those, labels == NULL with n_phones != 1 and a NULL pointer where one is required are
 *   CPC_ERR_INVALID with a message naming the entry point, before any launch, nothing written.
 *   No float atomic, no floating point at all.
 * ------------------------------------------------------------------------------------------ */
int cpc_unit_counts_lds_cells(void);
int cpc_unit_counts_chunk(void);
size_t cpc_unit_counts_scratch_bytes(int n_utt);
int cpc_unit_counts(const int *units, long n_unit_words, const int64_t *unit_off, const int *labels /* may be NULL */,
                    long n_label_words, const int64_t *label_off, const int *lengths, int n_utt, int n_units, int n_phones, int form,
                    int64_t *joint, int64_t *unit_runs, int64_t *phone_runs, int64_t *invalid, void *scratch, size_t scratch_bytes,
                    cpc_stream_t stream);
size_t cpc_unit_boundaries_scratch_bytes(int n_utt, long total_frames);
int cpc_unit_boundaries(const int *units, long n_unit_words, const int64_t *unit_off, const int *labels /* may be NULL */,
                        long n_label_words, const int64_t *label_off, const int *lengths, int n_utt, long total_frames, int tol,
                        int *out, void *scratch, size_t scratch_bytes, cpc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Duration-penalized unit segmentation (csrc/unit_dp.hip; cpc2_amd/unit_segmentation.py).  version 129.
 * Every pointer but penalties_host is a DEVICE pointer.  The reference has no counterpart: the definition below is the
 * specification.  It is the dynamic programme of Kamper & van Niekerk (Interspeech 2021) with their linear penalty
 * pen(l) = -(l - 1) weighted by lambda, which sums over T frames and S segments to lambda S - lambda T: a constant charge lambda
 * per segment, so the minimiser is a Viterbi pass over the K codes with a switch cost.
 *
 * Inputs for one utterance: costs c[t][k], f32, t in [0, T), k in [0, K); one penalty lambda >= 0, f64.  State values are f64:
 *
 *   V[0][k] = (double) c[0][k]
 *   m[t]    = min_k V[t][k]          a[t] = the LOWEST k with V[t][k] == m[t]
 *   sw      = m[t-1] + lambda                                  (one f64 add)
 *   stay[t][k] = (V[t-1][k] <= sw)                             (a tie stays)
 *   V[t][k] = (double) c[t][k] + (stay[t][k] ? V[t-1][k] : sw) (one f64 add)
 *
 * Backtrace:
 *
 *   u[T-1] = a[T-1]
 *   u[t-1] = stay[t][u[t]] ? u[t] : a[t-1]
 *
 * (m[t] is carried as V[t][a[t]]: where -0.0 and +0.0 are both minima, the one at the lowest index.)
 * Outputs per (utterance i, penalty p): u[0..T) (int32) at units[p * n_rows + offsets[i] + t]; energy[p * n_utt + i] = m[T-1]
 * (f64); n_segments[p * n_utt + i] = 1 + #{t >= 1 : u[t] != u[t-1]}; status[p * n_utt + i]:
 *   0  done
 *   1  empty utterance, T <= 0: nothing is written for its frames; energy 0, segments 0
 *   2  a cost of the utterance is NaN or +/-inf: its units are all -1, its energy is NaN, segments 0
 *   3  the utterance leaves the pack (offset < 0 or offset + T > n_rows), has more than 2^24 frames, or its back-pointers do not
 *      fit the scratch (below): it is never read, nothing is written for its frames; energy NaN, segments 0
 * Every step is a single IEEE operation and a min is exact; the file is built with -ffp-contract=off.  The device output
 * therefore EQUALS a numpy float64 statement of the lines above on every finite input, ties included, on every launch.
 *
 * cost is a pack of n_rows rows with stride ld >= k; utterance i owns rows [offsets[i], offsets[i] + lengths[i]) (int64 offsets,
 * int32 lengths).  Gaps and any order are allowed; rows outside an utterance and columns >= k are never read; units rows outside
 * an utterance are never written.  penalties_host: n_pen doubles on the HOST, read before the call returns.
 * Two forms, chosen from K alone: K <= cpc_segment_units_wave_k() = 256 runs one wave64 per (utterance, penalty) with the states in
 * registers (several waves per workgroup, no barrier); larger K one workgroup of 512 threads with one barrier per frame.  The
 * back-pointers are one bit per (frame, state) in 32-bit words plus a[t] as one int32 per frame, in scratch; the backtrace runs in
 * the same launch.  The scan for non-finite costs rides on the row reads.  No atomics, no f32 accumulation.
 * scratch: cpc_segment_units_scratch_bytes(n_utt, total_frames, k, n_pen), total_frames >= the summed lengths of the utterances that run
 * (0 with a message for sizes outside the limits).  The lengths live on the device, so cpc_segment_units cannot compare them with
 * scratch_bytes: fewer bytes than cpc_segment_units_scratch_bytes(n_utt, 0, k, n_pen) give CPC_ERR_WORKSPACE, and an utterance whose
 * back-pointers would leave what the scratch holds beyond that gets status 3.
 * Limits: 1 <= k <= 16384, 0 <= n_utt <= 2^20 (0: nothing is done, CPC_OK), 1 <= n_pen <= 16, every penalty finite and >= 0,
 *   n_rows >= 0, ld >= k; those and a NULL pointer where one is required are CPC_ERR_INVALID with a message naming the entry
 *   point, before any launch, nothing written.
 * ------------------------------------------------------------------------------------------ */
int cpc_segment_units_wave_k(void);
size_t cpc_segment_units_scratch_bytes(int n_utt, long total_frames, int k, int n_pen);
int cpc_segment_units(const float *cost, long n_rows, long ld, int k, const int64_t *offsets, const int *lengths, int n_utt,
                const double *penalties_host, int n_pen, int *units /* [n_pen][n_rows] */, double *energy /* [n_pen][n_utt] */,
                int *n_segments, int *status, void *scratch, size_t scratch_bytes, cpc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CPC2_HIP_H */
