/*
 * ms_hotpath.h -- C ABI of the MI355X-native myrtlespeech hot path.
 *
 * libms_hotpath.so is the drop-in boundary: plain pointers, sizes and a HIP
 * stream, no torch types.  The reference (MyrtleSoftware/myrtlespeech) has no
 * FFI of its own -- every FLOP on its hot path is a stock PyTorch op called
 * from a torch.nn.Module -- so each entry point below cites the reference
 * call site (file:line under src/myrtlespeech/) whose arithmetic it replaces.
 * The host-side mirror of those modules lives in myrtlespeech_amd/ (Python,
 * as the reference is Python); INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host;
 *   - tensors are dense, row-major, float32 unless stated; lengths are int32;
 *   - `stream` is a hipStream_t (NULL = default stream); calls only enqueue
 *     work, they never synchronise (exceptions: ms_rnn_status, ms_prof_read, the greedy ms_rnnt_decode and
 *     ms_rnnt_greedy_stream_step);
 *   - return value: MS_OK or an MS_ERR_* code; ms_last_error() describes the
 *     last failure on the calling thread;
 *   - outputs are caller-allocated; nothing is freed or retained.
 *
 * Operand precision (environment variable MS_PRECISION, read once per process
 * at the first launch; it selects kernels inside ms_rnn_pack / ms_rnn_layer_forward,
 * ms_linear_split_forward and ms_maskconv_cl_*; packed weights are only valid for
 * the mode they were packed in)
 *   unset / "bf16x3"  every float32 operand of the large contractions is split into
 *                     bf16 hi + lo and multiplied as hi*hi + lo*hi + hi*lo with float32
 *                     accumulation (relative error ~2^-17 per product; full-size DS2
 *                     logits within 2.5e-7 of the reference);
 *   "f32"             float32 MFMA everywhere (3.9e-8); the two-stream LSTM hands h to the
 *                     other workgroups with its mantissa LSB used as an epoch tag;
 *   "fp16"            one fp16 pass (1.1e-5 on that network; relative, not a parity mode).
 * Convolutions with few input channels, small GEMMs, CTC loss / gradient and the
 * decoders are float32 in every mode.
 */
#ifndef MS_HOTPATH_H
#define MS_HOTPATH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4 (round 6): MS_PRECISION's default is "f16x3" (fp16 hi + lo operand planes, three fp16 MFMAs; "bf16x3" selects the bf16
 * pairs of versions 1-3): packed weights made by an older library are in another plane format; ms_maskconv_cl_packed_bytes /
 * ms_maskconv_fwin_packed_bytes grew by 256 bytes (the weights' power-of-two scale word); MS_RNN_TIMING_SKIP_PROJECTION,
 * ms_rnn_stack_overlap_ok and ms_rnn_stack_forward are new; ms_rnn_workspace_bytes grew (four projection buffers for K-halves layers).
 * 3 (round 5): ms_ctc_status, ms_rnn_padded_hidden and ms_rnn_hx_preinit (+ MS_RNN_HX_PREINIT, exchange regions) are new; the CTC workspaces start with a 256-byte status region;
 * ms_linear_splitk_workspace_bytes / ms_linear_splitk_forward take `flags` (MS_LINEAR_FEW_ROWS): the K-slice count
 * no longer depends on M.
 * 2 (round 4): ms_prof_read writes MS_PROF_KINDS = 9 entries (was 4 in version 1); the `zero_infinity` argument of the CTC
 * entry points is a bit field {1 = zero_infinity, MS_CTC_LOG_PROBS_IN} and values above 3 are rejected;
 * ms_ctc_loss_backward takes the same bit field; ms_log_softmax_axis_backward is new.  The Python binding refuses a
 * library whose ms_abi_version() differs (myrtlespeech_amd/_lib.py). */
#define MS_ABI_VERSION 4

enum {
  MS_OK = 0,
  MS_ERR_INVALID = 1,     /* bad argument (shape, NULL pointer, unsupported value) */
  MS_ERR_HIP = 2,         /* a HIP runtime call failed */
  MS_ERR_WORKSPACE = 3,   /* workspace too small */
  MS_ERR_TIMEOUT = 4,     /* a persistent kernel gave up waiting for its peers */
  MS_ERR_UNSUPPORTED = 5
};

/* recurrent cell kinds: model/rnn.py:9-12 RNNType (+ model/hard_lstm.py) */
enum { MS_CELL_LSTM = 0, MS_CELL_GRU = 1, MS_CELL_RNN_TANH = 2, MS_CELL_HARD_LSTM = 3 };

/* activation fused into an epilogue: builders/activation.py:31-42 */
enum { MS_ACT_NONE = 0, MS_ACT_CLAMP = 1 /* Hardtanh(lo,hi); ReLU = clamp(0,+inf) */ };

int ms_abi_version(void);
const char* ms_last_error(void);

/* ---- model/cnn.py ------------------------------------------------------- */

/* MaskConv{1,2}d._mask_ (cnn.py:280-293, 425-443): x[n, :, t] = 0 for t >= lens[n],
 * in place.  x is [N, inner, T].  A negative length counts as 0, a length of T or more leaves the utterance alone; the
 * zeros written are +0.0 whatever the element held (NaN and Inf included), every other element keeps its bits. */
int ms_mask_time_(float* x, const int32_t* lens, int N, int inner, int T, void* stream);

/* Bytes of the packed filter bank ms_maskconv_pack writes (Cout = all groups). */
size_t ms_maskconv_packed_bytes(int Cout, int Cin_g, int KF, int KT, int groups);

/* Re-lays torch's Conv weight [Cout, Cin_g, KF, KT] (cnn.py:238-246, 377-385)
 * into the [group][cout-tile][cin*KF+kf][kt (padded even)][32] bank the kernel stages. */
int ms_maskconv_pack(const float* w, void* packed, int Cout, int Cin_g, int KF, int KT, int groups, void* stream);

/* MaskConv2d.forward (cnn.py:445-483) = mask + F.pad + Conv2d (+ the following
 * SeqLenWrapper activation, seq_len_wrapper.py:28-32), fused: frames t >= lens[n]
 * of the input read as 0, SAME padding is index arithmetic (pad_f_l / pad_t_l are
 * the LEFT pads of cnn.py:148-163), bias and clamp in the epilogue.
 * x [N, Cin, Fin, Tin] -> y [N, Cout, Fout, Tout].  MaskConv1d (cnn.py:295-333)
 * is the Fin = KF = SF = 1 case.  lens may be NULL (no masking).  groups >= 1. */
int ms_maskconv_forward(const float* x, const int32_t* lens, const void* packed_w, const float* bias, float* y,
                        int N, int Cin, int Fin, int Tin, int Cout, int Fout, int Tout, int KF, int KT, int SF,
                        int ST, int DF, int DT, int pad_f_l, int pad_t_l, int groups, int act, float act_lo,
                        float act_hi, void* stream);

/* Same contract as ms_maskconv_forward for groups == 1 and Cin % 16 == 0 (e.g. the second DS2
 * convolution), computed as a split-bf16 implicit GEMM over channels (x.w ~= x_hi.w_hi +
 * x_lo.w_hi + x_hi.w_lo, f32 accumulate).  The workspace receives the channels-last bf16
 * planes of the input. */
size_t ms_maskconv_cl_packed_bytes(int Cout, int Cin, int KF, int KT);
int ms_maskconv_cl_pack(const float* w, void* packed, int Cout, int Cin, int KF, int KT, void* stream);
size_t ms_maskconv_cl_workspace_bytes(int N, int Cin, int Fin, int Tin);
int ms_maskconv_cl_forward(const float* x, const int32_t* lens, const void* packed_w, const float* bias, float* y,
                           int N, int Cin, int Fin, int Tin, int Cout, int Fout, int Tout, int KF, int KT, int SF,
                           int ST, int DF, int DT, int pad_f_l, int pad_t_l, int act, float act_lo, float act_hi,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Single-channel MaskConv2d (Cin = 1, groups = 1, feature dilation 1, even feature stride; DS2's first convolution,
 * cnn.py:445-483 with builders/deep_speech_2.py:198-203 kernel [41, 11] stride [2, 2]) as the same split-bf16 implicit
 * GEMM: the KF input feature rows under an output feature row take the place of the input channels (padded to a
 * multiple of 16), the KT time taps stay taps.  x is [N, 1, Fin, Tin]; the workspace holds its feature-contiguous bf16
 * hi / lo planes [N, Tin, FP] with the SAME feature padding materialised; mask (t >= lens[n]) and time padding are load
 * predicates; bias + clamp in the epilogue; y is [N, Cout, Fout, Tout] float32.  MS_ERR_UNSUPPORTED when the staged
 * rows do not fit LDS (the caller then uses ms_maskconv_forward).  The window's KF rows are padded to whole 16-row k-steps
 * with zero filters, which multiply the input rows under the window: in the two-plane modes the planes therefore hold the
 * input clamped to the finite range of their format (f16x3: +-65504, as everywhere; bf16x3: +-3.39e38), so that a non-finite
 * input value reaches only the outputs whose window holds it (the one-plane fp16 mode does not clamp). */
size_t ms_maskconv_fwin_packed_bytes(int Cout, int KF, int KT);
int ms_maskconv_fwin_pack(const float* w, void* packed, int Cout, int KF, int KT, void* stream);
size_t ms_maskconv_fwin_workspace_bytes(int N, int Tin, int KF, int SF, int Fout);
int ms_maskconv_fwin_forward(const float* x, const int32_t* lens, const void* packed_w, const float* bias, float* y, int N,
                             int Fin, int Tin, int Cout, int Fout, int Tout, int KF, int KT, int SF, int ST, int DT,
                             int pad_f_l, int pad_t_l, int act, float act_lo, float act_hi, void* workspace,
                             size_t workspace_bytes, void* stream);

/* The pair single-channel convolution -> channels-last convolution without the float32 tensor between them:
 * ms_maskconv_fwin_planes_forward is ms_maskconv_fwin_forward whose epilogue writes, instead of y, the hi / lo planes
 * [N, Fout, Tout, Cout] that ms_maskconv_cl_forward's layout pass would make of y (same bias, clamp and split, so the
 * same bits; Cout % 16 == 0) into `planes` (at least ms_maskconv_cl_workspace_bytes(N, Cout, Fout, Tout) bytes);
 * ms_maskconv_cl_planes_forward is ms_maskconv_cl_forward on such planes, its layout pass skipped.  The first returns
 * MS_ERR_UNSUPPORTED, with nothing launched, for shapes that only the kernels without a planes epilogue serve (short
 * inputs, ms_conv_set_variant(1)): the caller then runs the two plain entry points.  The two *_supported queries say, without
 * launching anything, whether the producer would write planes and whether the channels-last kernel takes the consumer's
 * shape (it has no tile for e.g. 96 input channels at 11 taps: ms_maskconv_cl_forward then answers MS_ERR_UNSUPPORTED and
 * its caller uses ms_maskconv_forward, which needs the float32 tensor): hand planes over only when both answer 1. */
int ms_maskconv_fwin_planes_supported(int N, int Tin, int Cout, int Fout, int Tout, int KF, int KT, int SF, int ST, int DT);
int ms_maskconv_cl_supported(int N, int Cin, int Fin, int Cout, int Fout, int Tout, int KT, int ST, int DT);
int ms_maskconv_fwin_planes_forward(const float* x, const int32_t* lens, const void* packed_w, const float* bias, void* planes,
                                    size_t planes_bytes, int N, int Fin, int Tin, int Cout, int Fout, int Tout, int KF, int KT,
                                    int SF, int ST, int DT, int pad_f_l, int pad_t_l, int act, float act_lo, float act_hi,
                                    void* workspace, size_t workspace_bytes, void* stream);
int ms_maskconv_cl_planes_forward(const int32_t* lens, const void* packed_w, const float* bias, float* y, int N, int Cin,
                                  int Fin, int Tin, int Cout, int Fout, int Tout, int KF, int KT, int SF, int ST, int DF,
                                  int DT, int pad_f_l, int pad_t_l, int act, float act_lo, float act_hi, void* planes,
                                  size_t planes_bytes, void* stream);

/* Tuning switch for same-process A/B runs of the convolution front end: 0 = the shipped dispatch, 1 = every shape on the
 * tiled kernel and layout passes that served it before the shared-window kernel (bit-identical results).  Not part of
 * the reference surface. */
int ms_conv_set_variant(int variant);

/* MaskConv1d with many input channels as im2col + split-bf16 GEMM (model/cnn.py:295-333, the conv1d flavour of the DS2
 * builder): x [N, Cin, Tin] -> y [N, Cout, Tout]; frames t >= lens[n] read as zero (cnn.py:280-293), pad_l zero
 * frames on the left (cnn.py:252-278); packed = ms_maskconv1d_gemm_pack of weight [Cout, Cin, KT]; bias may be NULL;
 * groups = 1; MS_ERR_WORKSPACE for a workspace below ms_maskconv1d_gemm_workspace_bytes.  Products carry the split-bf16 error
 * (~2^-17 relative, like ms_linear_split_forward). */
size_t ms_maskconv1d_gemm_packed_bytes(int Cout, int Cin, int KT);
int ms_maskconv1d_gemm_pack(const float* w, void* packed, int Cout, int Cin, int KT, void* stream);
size_t ms_maskconv1d_gemm_workspace_bytes(int N, int Cin, int Tout, int Cout, int KT);
int ms_maskconv1d_gemm_forward(const float* x, const int32_t* lens, const void* packed, const float* bias, float* y, int N,
                               int Cin, int Tin, int Cout, int Tout, int KT, int ST, int DT, int pad_l, int act,
                               float act_lo, float act_hi, void* workspace, size_t workspace_bytes, void* stream);

/* DeepSpeech2._conv_to_rnn_size (deep_speech_2.py:114-117): [N, CF, T] -> [T, N, CF]. */
int ms_nct_to_tnc(const float* x, float* y, int N, int CF, int T, void* stream);

/* Elementwise clamp (SeqLenWrapper(Hardtanh/ReLU) on its own); y may alias x.  min(max(x, lo), hi) for every x that is a
 * number; a NaN stays a NaN (torch.clamp, F.hardtanh), as in every fused clamp of this library (MS_ACT_CLAMP epilogues, the
 * hard sigmoid and hard tanh of MS_CELL_HARD_LSTM).  n == 0 is valid and touches no pointer. */
int ms_clamp(const float* x, float* y, size_t n, float lo, float hi, void* stream);

/* ---- model/fully_connected.py ------------------------------------------ */

/* torch.nn.Linear (+ hidden activation) (fully_connected.py:107-131, 164; also
 * deep_speech_1.py:124-136): y[M,N] = act(x[M,K] . w[N,K]^T + bias[N]). bias may be NULL. */
int ms_linear_forward(const float* x, const float* w, const float* bias, float* y, int M, int K, int N, int act,
                      float act_lo, float act_hi, void* stream);

/* Same contract as ms_linear_forward (exact float32 MFMA) for layers with few output COLUMNS (N <= 64, K >= 512: the
 * 29-symbol output layer, fully_connected.py:164 / deep_speech_1.py:118-120): one 32-column tile per 128 rows leaves a
 * streaming chunk's 1 024 rows on eight workgroups that each walk all of K, so the contraction is cut into min(8, K / 128)
 * slices whose partial sums land in the workspace and are added in slice order (deterministic; the slice count depends on
 * (K, N, flags) only -- never on M -- so a row's result does not depend on the batch or chunk it is in; the rounding differs
 * from ms_linear_forward's single k-ordered chain by a few ulp).  flags: 0, or MS_LINEAR_FEW_ROWS = the caller states that
 * the layer serves a handful of rows (one clip's hidden layers, deep_speech_1.py:124-136) and takes K slices for N <= 4096
 * too; a caller that sets it for some batches and not for others gives up bit-reproducibility between them.
 * ms_linear_splitk_workspace_bytes() == 0 means the shape is not such a layer: the call then IS ms_linear_forward and needs
 * no workspace; a NULL workspace selects ms_linear_forward for any shape. */
#define MS_LINEAR_FEW_ROWS 1
size_t ms_linear_splitk_workspace_bytes(int M, int K, int N, int flags);
int ms_linear_splitk_forward(const float* x, const float* w, const float* bias, float* y, int M, int K, int N, int act,
                             float act_lo, float act_hi, int flags, void* workspace, size_t workspace_bytes, void* stream);

/* Same contract as ms_linear_forward for K % 32 == 0, computed with float32 operands split into 16-bit planes in the
 * process's MS_PRECISION mode, hi = rn(v), lo = rn(v - hi):
 *   "f16x3" (default)  fp16 hi + lo, 22 significant bits of every operand;
 *   "bf16x3"           bf16 hi + lo, 16 significant bits;
 *   "fp16"             one fp16 plane, 11 significant bits, one product;
 * y = act(sum_k (x_hi.w_hi + x_lo.w_hi + x_hi.w_lo) + bias) with float32 products and sums (x_lo.w_lo is left out; "fp16":
 * sum_k x_hi.w_hi).  The fp16 formats hold +-65504: a finite operand is clamped to that range before each rounding, so values
 * up to 2 x 65504 still come out through the lo plane and larger ones read as +-131008 ("fp16": +-65504); bf16 planes have
 * float32's range.  Non-finite values are kept: a NaN in x[m, k] makes row m of y NaN, a NaN in w[n, k] column n, in every
 * mode and through MS_ACT_CLAMP (which is torch.nn.Hardtanh: NaN stays NaN, +-Inf becomes a bound); a +-Inf operand makes
 * its row / column non-finite before the activation (NaN in the two-plane modes, whose lo plane is Inf - Inf).  Other rows and
 * columns are not affected.  This holds for the operands that ms_linear_split_* and the LSTM input projection split; the
 * convolution entry points (ms_maskconv1d_gemm_forward's im2col planes among them) still saturate a non-finite input to
 * +-65504 (NaN: -65504) before it reaches these kernels.  The workspace holds the four planes (ms_linear_split_workspace_bytes: M K 4 and N K 4 bytes, each
 * rounded up to 256); x and w must be 16-byte aligned. */
size_t ms_linear_split_workspace_bytes(int M, int K, int N);
int ms_linear_split_forward(const float* x, const float* w, const float* bias, float* y, int M, int K, int N, int act,
                            float act_lo, float act_hi, void* workspace, size_t workspace_bytes, void* stream);

/* The same layer with its weight planes made once instead of per call (fully_connected.py:107-131 builds the Linear once and
 * calls it per batch): ms_linear_split_pack writes [hi | lo] planes of w [N, K] (ms_linear_split_packed_bytes(K, N) bytes, in
 * the precision mode of the process); ms_linear_split_forward_packed takes them, its workspace holds the x planes only
 * (M * K * 4 bytes, 256-byte aligned size).  Same kernels, same plane values, same bits as ms_linear_split_forward. */
size_t ms_linear_split_packed_bytes(int K, int N);
int ms_linear_split_pack(const float* w, void* packed, int K, int N, void* stream);
int ms_linear_split_forward_packed(const float* x, const void* packed_w, const float* bias, float* y, int M, int K, int N, int act,
                                   float act_lo, float act_hi, void* workspace, size_t workspace_bytes, void* stream);

/* ---- model/lookahead.py ------------------------------------------------- */

/* Lookahead.forward (lookahead.py:65-69): y[n,f,t] = sum_k w[f,k] * x[n,f,t+k]
 * (zero beyond T).  Element strides let the caller pass the [T,N,F] RNN output
 * directly (deep_speech_2.py:119-121, 161-164).  w is [F, ctx]. */
int ms_lookahead_forward(const float* x, const float* w, float* y, int N, int F, int T, int ctx, long xs_n,
                         long xs_f, long xs_t, long ys_n, long ys_f, long ys_t, int act, float act_lo,
                         float act_hi, void* stream);

/* The same on a WINDOW of a stream (streaming with carried context, myrtlespeech_amd/streaming.py): x holds T_in frames,
 * only the first T_out <= T_in output frames are computed and written (taps beyond T_in read as zero, which a caller
 * allows only at the true end of the utterance); y has room for T_out frames. */
int ms_lookahead_window_forward(const float* x, const float* w, float* y, int N, int F, int T_in, int T_out, int ctx,
                                long xs_n, long xs_f, long xs_t, long ys_n, long ys_f, long ys_t, int act, float act_lo,
                                float act_hi, void* stream);

/* ---- model/rnn.py / model/hard_lstm.py ---------------------------------- */

/* One layer (all directions) of torch.nn.LSTM/GRU/RNN as RNN.forward drives it
 * (rnn.py:170-183: pack_padded_sequence -> rnn -> pad_packed_sequence) or of
 * HardLSTM (hard_lstm.py:346-379, 416-456, 513-561).
 *
 * Packing: weights in torch layout, per direction d (0 fwd, 1 reverse):
 * w_ih[d] [G*H, In], w_hh[d] [G*H, H], b_ih[d]/b_hh[d] [G*H] or NULL (bias=False);
 * G = 4 (LSTM, gate order i,f,g,o), 3 (GRU: r,z,n), 1 (RNN).  The pointer arrays
 * themselves are HOST arrays of device pointers. */
/* rnn.py:112-120 accepts any hidden_size (protos/rnn.proto:20); the persistent recurrence kernels exist for LSTM widths that
 * are multiples of 64 (<= 1024) / 1280 / 1536 / 2048 and GRU widths 512 .. 2560 in steps of 256 (+ 1280).  Returns the width a
 * caller should PAD a layer of hidden size H to (zero weight rows / columns, zero biases, zero initial state for the padded
 * units: they stay exactly 0, so out[..., :H], h_n[..., :H], c_n[..., :H] are the unpadded layer's values with exact zeros
 * added to their sums) so that it runs on a persistent kernel instead of one launch per step; H itself when no padding is
 * needed or none helps.  Round 6: in the two-plane modes an LSTM width of 129 .. 1024 that is not 256 / 512 / 768 / 1024 is sent
 * to the NEXT of those (the two-stream kernel is about twice as fast as the one that serves the other multiples of 64), and a
 * width beyond every persistent kernel to the next multiple of 64 (the MFMA step kernel instead of the scalar one).
 * MS_RNN_PAD_HIDDEN=0 always returns H. */
int ms_rnn_padded_hidden(int cell, int H, int ndir);
size_t ms_rnn_packed_bytes(int cell, int In, int H, int ndir);
int ms_rnn_pack(int cell, int In, int H, int ndir, const float* const* w_ih_host, const float* const* w_hh_host,
                const float* const* b_ih_host, const float* const* b_hh_host, void* packed, void* stream);

size_t ms_rnn_workspace_bytes(int cell, int T, int N, int In, int H, int ndir);

/* x [T, N, In] time-major; lens [N] sorted descending (enforce_sorted=True,
 * rnn.py:174) or NULL = all T (HardLSTM ignores lengths, hard_lstm.py:36);
 * max_len = lens[0] (host copy; T if lens is NULL); h0/c0 [ndir, N, H] (c0 only
 * for LSTM cells; NULL = zeros, rnn.py:187-205); out [T, N, ndir*H] (rows
 * t >= lens[n] are written as 0); hn/cn [ndir, N, H] = state at each sequence's
 * last valid step. */
int ms_rnn_layer_forward(int cell, const void* packed, const float* x, const int32_t* lens, int max_len,
                         const float* h0, const float* c0, float* out, float* hn, float* cn, int T, int N, int In,
                         int H, int ndir, void* workspace, size_t workspace_bytes, void* stream);

/* Layer stacks (rnn.py:112-120 num_layers > 1): the same call with two optional hand-offs through the shared workspace,
 * for layer kinds where ms_rnn_layer_chains_planes() returns 1 (the two-stream LSTM with split-bf16 / fp16 operands, the persistent GRU):
 *   MS_RNN_OUT_PLANES_TO_WS  the layer output is left in the workspace as the NEXT layer's GEMM operand planes
 *                            ([max_len*N][ndir*H] bf16 hi + lo, or one fp16 plane) instead of float32 `out` (which may
 *                            then be NULL and is not written); the workspace must also hold
 *                            ms_rnn_workspace_bytes(cell, T, N, ndir*H, H, ndir);
 *   MS_RNN_X_PLANES_IN_WS    the input is taken from those planes (left there by the previous layer's call with the
 *                            same T, N, max_len and workspace); `x` may be NULL.
 * Same arithmetic as splitting the float32 output afterwards, one pass over the activations less per layer. */
enum { MS_RNN_X_PLANES_IN_WS = 1, MS_RNN_OUT_PLANES_TO_WS = 2, MS_RNN_PACKED_ROWS = 4, MS_RNN_HX_PREINIT = 4096,
       /* A layer call in two halves, for callers that interleave two batches' layers on two streams (model/rnn.py: the
        * half-batch pipeline of short sequences): MS_RNN_PROJECTION_ONLY = the input projection into the workspace, nothing
        * else; MS_RNN_RECURRENCE_ONLY = the recurrence on the projection an earlier MS_RNN_PROJECTION_ONLY call with the same
        * arguments left in the SAME workspace (stream-ordered behind it).  Together they do what the plain call does. */
       MS_RNN_RECURRENCE_ONLY = 8192, MS_RNN_TIMING_SKIP_PROJECTION = 8192 /* (tools/overlap_emulation.py's name for it) */,
       MS_RNN_PROJECTION_ONLY = 16384 };
int ms_rnn_layer_chains_planes(int cell, int H, int ndir);
/* One initialisation of the cross-workgroup exchange for a whole stack (rnn.py:112-120 num_layers > 1): every layer call
 * of the persistent kernels starts with a small launch that sets its exchange buffer's epoch tags and zeroes the per-call
 * status words -- five of them on a streaming chunk's critical path.  A workspace holds 8 exchange regions; a layer call
 * selects one with `flags` bits 8 .. 11 (0 by default).  ms_rnn_hx_preinit initialises regions 0 .. nregions - 1 for layers
 * that all run with this (cell, T, N, H, ndir, max_len) in ONE launch; the layer calls that follow on the same stream then
 * carry MS_RNN_HX_PREINIT | (region << 8), region = the layer's index.  MS_ERR_UNSUPPORTED (nothing launched, no error text)
 * for layer kinds it does not serve: the caller then simply leaves the flag out. */
int ms_rnn_hx_preinit(int cell, int T, int N, int In, int H, int ndir, int max_len, int nregions, void* workspace,
                      size_t workspace_bytes, void* stream);
/* MS_RNN_PACKED_ROWS (a permission, for batches whose lengths differ): torch's packed sequences (rnn.py:174-181) hold only
 * the frames t < lens[n]; with this flag the layer does the same where it can -- the input projection runs over sum(lens)
 * rows instead of max_len * N and the chained planes hold only those rows, frame after frame -- and ignores it where it
 * cannot.  Outputs are the same bits either way.  Whether a layer can depends on (cell, max_len, N, H, ndir), not on In:
 * ms_rnn_layer_packs_rows() says; every layer of a chained stack must be given the same flag. */
int ms_rnn_layer_packs_rows(int cell, int T, int N, int In, int H, int ndir);
int ms_rnn_layer_forward_ex(int cell, const void* packed, const float* x, const int32_t* lens, int max_len,
                            const float* h0, const float* c0, float* out, float* hn, float* cn, int T, int N, int In,
                            int H, int ndir, int flags, void* workspace, size_t workspace_bytes, void* stream);

/* Synchronises `stream` and reports whether every ms_rnn_layer_forward that used
 * `workspace` since the previous call of this function completed (MS_OK) or a
 * persistent kernel timed out (MS_ERR_TIMEOUT, reported once).  The time-out word is
 * sticky across layer calls -- one check after a whole stack of layers is enough --
 * and lives in the first 256 bytes of the workspace, which must therefore be ZERO
 * when a freshly allocated workspace is used for the first time. */
/* 1 when a recurrent layer of this kind and batch size runs as the wide-workgroup persistent LSTM kernel, which occupies
 * at most half of the CUs per batch group of 32 rows (H = 1024, split-bf16 operands, up to 64 sequences): the two-in-flight
 * pipeline then runs the OTHER batch's projection as the regular GEMM on the free CUs instead of the co-tenant form. */
int ms_rnn_layer_is_wide(int cell, int H, int ndir, int N);
/* A whole stack in one call with layer l+1's input projection computed BESIDE layer l's recurrence (rnn.py:112-120 with
 * num_layers > 1, bidirectional; deep_speech_2.py:159): a bidirectional stack of wide-workgroup LSTM layers (H = 1024, up to 32
 * sequences) leaves half of the CUs idle during every recurrence; here a layer's recurrence runs as `segments` launches over
 * consecutive time segments and, after each, a second (library-owned) stream computes the next layer's two K-half projections
 * of the rows that segment produced.  Same kernels on the same operands as nl calls of ms_rnn_layer_forward_ex with the planes
 * chained -- the same bits -- for rows that all exist (not MS_RNN_PACKED_ROWS).  packed_host: HOST array of the nl layers'
 * packed weights (device pointers, layer 0 first; layer 0 packed for In, the others for ndir * H); h0 / c0 / hn / cn:
 * [nl * ndir, N, H]; out: [T, N, ndir * H] float32 of the last layer.  ms_rnn_stack_overlap_ok says whether a stack qualifies
 * (MS_RNN_OVERLAP=0: never); its T is the number of steps the call will RUN -- the max_len handed to ms_rnn_stack_forward, not
 * the length T of the buffers: a segment must be shorter than the steps that run, so a long buffer holding short sequences
 * does not qualify (ms_rnn_stack_forward checks with max_len and refuses such a call).  A stack it accepts runs with any
 * `segments` >= 2: where no cut of about max_len / segments steps qualifies, the forward uses the one the predicate found.
 * Not for use inside a stream capture or beside another stream's persistent launches. */
int ms_rnn_stack_overlap_ok(int cell, int T, int N, int In, int H, int ndir, int nl);
int ms_rnn_stack_forward(int cell, const void* const* packed_host, const float* x, const int32_t* lens, int max_len,
                         const float* h0, const float* c0, float* out, float* hn, float* cn, int T, int N, int In, int H, int ndir,
                         int nl, int segments, void* workspace, size_t workspace_bytes, void* stream);

int ms_rnn_status(const void* workspace, void* stream);

/* Diagnostic: byte offset inside the RNN workspace of the per-workgroup stamp sums
 * [ndir*H/8][8] (u64 wall-clock ticks, 100 MHz: wait, MFMA loop, reduce+cell, publish)
 * that the persistent LSTM kernel fills when MS_LSTM_STAMPS=1 is set in the environment. */
size_t ms_rnn_debug_offset(int cell, int T, int N, int In, int H, int ndir);

/* Tuning switch for same-process A/B runs of the split-operand GEMM (tools/gemm_probe.py): 0 = the shipped choice,
 * 2 = the register-staged kernel (the round-1 kernel), 7 .. 11 = the four-wave 256 x 128 LDS-DMA forms (with bf16 planes they
 * differ in how a wave issues its DMA pieces); bit-identical results.  Not part of the reference surface. */
int ms_gemm_set_variant(int variant);

/* Optional launch timing for bench.py's roofline line and its per-stage breakdown (not part of the reference
 * surface).  While enabled, the entry points on a DeepSpeech step bracket their launches with HIP events on the
 * caller's stream.  ms_prof_read synchronises those events and returns the summed milliseconds and launch counts
 * since the last read, MS_PROF_KINDS entries each, indexed by MS_PROF_*:
 * PROJECTION = input projection of one recurrent layer (operand split, where the producer did not hand planes
 * over, + GEMM), RECURRENCE = recurrent kernel(s) of one layer, GEMM_K_LARGE = the split-operand projection GEMM
 * kernel alone at In >= 1024, GEMM_K_SMALL = the same at In < 1024 (the first layer of a stack) -- both nested
 * inside PROJECTION --, CONV = one masked convolution call (mask, layout pass and kernel), LAYOUT = ms_nct_to_tnc,
 * LINEAR = one ms_linear(_split)_forward call, GREEDY = ms_ctc_greedy_decode, OTHER = clamp / mask / lookahead. */
enum {
  MS_PROF_PROJECTION = 0, MS_PROF_RECURRENCE = 1, MS_PROF_GEMM_K_LARGE = 2, MS_PROF_GEMM_K_SMALL = 3, MS_PROF_CONV = 4,
  MS_PROF_LAYOUT = 5, MS_PROF_LINEAR = 6, MS_PROF_GREEDY = 7, MS_PROF_OTHER = 8
};
#define MS_PROF_KINDS 9
int ms_prof_enable(int on);
int ms_prof_read(float* out_ms_host, int* out_n_host);

/* Diagnostic (tools/clock_probe.py; not part of the reference surface): ONE wave that samples the shader clock counter
 * and the 100 MHz wall clock `samples` times, about `spacing_us` apart, into out_dev[2 * samples] (u64 pairs
 * {wall ticks, shader cycles}).  Launched on a stream of its own beside other kernels it shows the clock the chip holds
 * under their load (MI355X_MICROARCH.md, DVFS give-back item 6).  samples * spacing_us is capped at 50 ms. */
int ms_clock_probe(unsigned long long* out_dev, int samples, int spacing_us, void* stream);

/* Diagnostic (bench.py's floors for the scan kernels; not part of the reference surface): one workgroup of `threads`
 * runs `steps` rounds of {LDS write, barrier, neighbour read, barrier}; out_dev[0] = elapsed ticks of the 100 MHz wall
 * clock (2 * steps barrier-separated phases), out_dev[1] = a checksum. */
int ms_barrier_chain_probe(unsigned long long* out_dev, int steps, int threads, void* stream);

/* ---- loss/ctc_loss.py ---------------------------------------------------- */

size_t ms_ctc_loss_workspace_bytes(int T, int N, int V, int S_max);

/* The first 256 bytes of a CTC workspace (forward or backward) hold a sticky time-out word; the caller provides it zeroed
 * before the first call and leaves it alone afterwards.  The four-wave alpha pipeline hands two values per frame from wave
 * to wave through an LDS mailbox with a bounded (0.5 s) spin; should an entry never arrive -- it cannot while every wave of
 * the workgroup runs -- the utterance's loss (and its gradient) is NaN AND the word is set.  ms_ctc_status synchronises
 * `stream`, returns MS_ERR_TIMEOUT once if the word was set and clears it (the CTC twin of ms_rnn_status; ctc_loss.py has
 * no such state: torch's kernel cannot time out).  A NaN loss WITHOUT the status is data: a frame (t < in_lens[n]) whose
 * log-softmax normaliser is not finite (a NaN or +inf logit, a row of -inf) or, under MS_CTC_LOG_PROBS_IN, a NaN among its
 * values gives NaN as torch.nn.CTCLoss does, also under zero_infinity and whichever kernel runs; ms_ctc_loss_backward
 * then writes NaN to every element of that utterance's existing frames and zeros behind them. */
int ms_ctc_status(const void* workspace, void* stream);

/* CTCLoss.forward (ctc_loss.py:95-101) = LogSoftmax(dim=-1) + torch.nn.CTCLoss:
 * log-space alpha recursion per utterance.  logits [T,N,V] unnormalised;
 * targets int32, utterance n's labels start at tgt_offsets[n] (covers both the
 * padded [N,S] and the concatenated 1-D form, ctc_loss.py:74-83).
 * nll [N] = -log p(target | input) (reduction='none');
 * reduced [1] = 'sum' (reduction=2) or 'mean' (reduction=1: nll/clamp(len,1),
 * batch mean, ctc_loss.py:17-19); zero_infinity replaces inf by 0. */
#define MS_CTC_LOG_PROBS_IN 2 /* OR-ed into `zero_infinity`: `logits` already hold the values torch.nn.CTCLoss is to take as
                              * log-probabilities -- CTCLoss(dim != -1), ctc_loss.py:37-45, normalises over another axis
                              * (ms_log_softmax_axis) -- so no log-softmax over the symbols is applied */
int ms_ctc_loss_forward(const float* logits, const int32_t* in_lens, const int32_t* targets,
                        const int32_t* tgt_offsets, const int32_t* tgt_lens, float* nll, float* reduced, int T,
                        int N, int V, int S_max, int blank, int reduction, int zero_infinity, void* workspace,
                        size_t workspace_bytes, void* stream);

/* LogSoftmax over an axis other than the last one (ctc_loss.py:45 passes the constructor's `dim` through): x, y are
 * contiguous [outer, axis, inner]; y = x - logsumexp over `axis`. */
int ms_log_softmax_axis(const float* x, float* y, int outer, int axis, int inner, void* stream);
/* Its backward (autograd through LogSoftmax(dim), ctc_loss.py:45): y = the log-probabilities ms_log_softmax_axis wrote,
 * g = the gradient with respect to them; gx = g - exp(y) * sum over `axis` of g.  gx may alias g. */
int ms_log_softmax_axis_backward(const float* y, const float* g, float* gx, int outer, int axis, int inner, void* stream);

/* Gradient of ms_ctc_loss_forward's per-utterance losses with respect to the logits (what autograd gives the
 * reference through LogSoftmax + torch.nn.CTCLoss, loss/ctc_loss.py:95-101): alpha rows forward, beta rows backward,
 * grad_logits[t,n,k] = grad_nll[n] * (softmax(x)[t,k] - exp(logsumexp_{s: l'_s=k}(alpha_t(s)+beta_t(s)) + nll[n] - lp[t,k]))
 * for t < in_lens[n], 0 on padding frames and, with zero_infinity, for utterances whose loss is infinite.  grad_nll
 * [N] is the upstream gradient of each nll[n] (the host folds the reduction in: 1 for 'sum', 1/(N*max(len,1)) for
 * 'mean').  grad_logits [T,N,V] is fully written.  `zero_infinity` is the same bit field as in ms_ctc_loss_forward: with
 * MS_CTC_LOG_PROBS_IN the `logits` are taken as log-probabilities (no softmax over the symbols: lp = logits) and the result
 * is what torch.nn.CTCLoss's backward hands to the LogSoftmax(dim) in front of it, exp(lp) - exp(... - lp) (the caller
 * chains ms_log_softmax_axis_backward); values above 3 are rejected. */
size_t ms_ctc_loss_backward_workspace_bytes(int T, int N, int V, int S_max);
int ms_ctc_loss_backward(const float* logits, const int32_t* in_lens, const int32_t* targets, const int32_t* tgt_offsets,
                         const int32_t* tgt_lens, const float* grad_nll, float* grad_logits, int T, int N, int V,
                         int S_max, int blank, int zero_infinity, void* workspace, size_t workspace_bytes, void* stream);

/* ---- post_process/ctc_greedy_decoder.py ---------------------------------- */

/* CTCGreedyDecoder.forward (ctc_greedy_decoder.py:74-92): argmax over symbols
 * (ties -> lowest index), drop repeats and blanks.  x [T,N,V] (any real scores);
 * out_idx [N, T] int32, out_len [N]; row n's entries past out_len[n] are unspecified (alphabets beyond 64 symbols keep
 * the frames' arg maxes there before the in-place compaction).  lens[n] is clamped to [0, T].  The arg max of a frame: a NaN
 * counts as the maximum and the first NaN wins (torch.argmax); a frame of all -inf decodes to symbol 0. */
int ms_ctc_greedy_decode(const float* x, const int32_t* lens, int32_t* out_idx, int32_t* out_len, int T, int N,
                         int V, int blank, void* stream);

/* The same decode advanced one chunk of logit rows at a time (ctc_greedy_decoder.py:74-92, its frame loop cut between
 * frames; the reference has no streaming decoder).  Everything a stream carries between two steps -- the symbol of its
 * last existing row, its label count, its rows seen, one sticky overflow word for the batch -- lives in `state`
 * (ms_ctc_greedy_stream_state_bytes(N) bytes of device memory; host arithmetic, 0 for N <= 0), as int32 words:
 * [0] the overflow word, [1 .. 15] reserved, then four per stream i at [16 + 4 i]: previous symbol (-1: none), label
 * count, frames seen, reserved.  _begin: no previous symbol, 0 labels, 0 frames seen, overflow word cleared.
 * _step: x [rows, n, V] are the next `rows` logit rows of the first n <= N streams (streams leave a sorted batch as a
 * suffix).  Any real scores; arg max as ms_ctc_greedy_decode has it: first maximum wins, NaN counts as the maximum,
 * first NaN wins.  Rows that exist for stream i: chunk_lens[i] (clamped to [0, rows]) if chunk_lens is given,
 * otherwise clamp(total_lens[i] - frames_seen[i], 0, rows); exactly one of the two is non-NULL.  frames_seen[i]
 * advances by the rows that existed.  A row's symbol is kept iff it is not `blank` and differs from the symbol of the
 * stream's previous existing row -- for a chunk's first row the one carried in `state`, none at the start of the clip.
 * Kept symbols are appended to labels [N, cap] at the stream's running label count; label_frames [N, cap] (may be NULL)
 * gets the 0-based index, counted over the stream's existing rows since _begin, of the row that emitted the label (where
 * its run began).  A stream that would exceed `cap` labels stops appending, keeps counting and sets the overflow word.
 * fresh [N, 1 + rows] (may be NULL): column 0 = labels this call appended for the stream (0 for streams n .. N-1),
 * columns 1.. = those labels: one small device-to-host copy per step delivers the news.
 * No host synchronisation, no host-read counter, no allocation: steps with a fixed `rows` can be captured into a HIP
 * graph on one stream and replayed. */
size_t ms_ctc_greedy_stream_state_bytes(int N);
int ms_ctc_greedy_stream_begin(void* state, int N, void* stream);
int ms_ctc_greedy_stream_step(const float* x, int rows, int n, int V, int blank, const int32_t* total_lens,
                              const int32_t* chunk_lens, int32_t* labels, int32_t* label_frames, int cap, int32_t* fresh,
                              void* state, int N, void* stream);

/* ---- post_process/ctc_aligner.py ----------------------------------------- */

/* CTC forced alignment (no counterpart in the reference): the best path of a GIVEN transcript through the scores, i.e. the
 * Viterbi (max-plus) form of the recursion ms_ctc_loss_forward sums, its back-trace and the frame span of every label.
 *
 * Per utterance n: T_n = in_lens[n] rows x[t, n, :] of V scores; a target y_0 .. y_{L-1}, L = tgt_lens[n] (<= L_max), whose
 * labels start at targets[tgt_offsets[n]] (the padded [N, S] and the concatenated 1-D form alike, as in
 * ms_ctc_loss_forward) and differ from `blank`; the extended sequence e_s, s = 0 .. S-1, S = 2L+1: e_s = blank for even s,
 * y_{(s-1)/2} for odd s.
 * flags = 0 (logits in): lp[t, v] = x[t, n, v] - logsumexp_v x[t, n, :] in float32, by the device's own log-softmax.
 * flags = MS_CTC_LOG_PROBS_IN: lp[t, v] = x[t, n, v] exactly as given; -inf is allowed and means "impossible".
 * Recursion in natural-log float32, one rounding per addition and no other arithmetic:
 *   d_0(0) = lp[0, e_0], d_0(1) = lp[0, e_1] (if S > 1), every other d_0(s) = -inf;
 *   t >= 1: best = d_{t-1}(s), k = 0;
 *           if s >= 1 and d_{t-1}(s-1) > best (strictly): best = d_{t-1}(s-1), k = 1;
 *           if s >= 2, e_s != blank, e_s != e_{s-2} and d_{t-1}(s-2) > best (strictly): best = d_{t-1}(s-2), k = 2;
 *           d_t(s) = best + lp[t, e_s], back-pointer k -- ties prefer staying, then one step, then the skip;
 *   end: the final state is S-1 unless S >= 2 and d_{T_n-1}(S-2) > d_{T_n-1}(S-1) strictly; score = d of that state;
 *        state[t], t = T_n-1 .. 0, by walking the back-pointers.
 * No alignment: score = -inf when no path exists (T_n < L + #{i: y_i == y_{i-1}}; T_n = 0 with L > 0; impossible symbols);
 * T_n = 0 with L = 0 gives score 0 and an empty path.  Non-finite input -- a NaN or +inf anywhere in an existing row
 * (log-probabilities in), a non-finite normaliser of an existing row (logits in) -- gives score = NaN.  In both cases the
 * utterance has no path: every per-frame output is -1, every span (-1, -1), every token log-probability -inf (NaN when the
 * score is NaN).  A target label outside [0, V) or equal to `blank`, or tgt_lens[n] outside [0, L_max], is the caller's
 * error: nothing is read out of bounds for it and the utterance is treated as having no alignment.
 * Outputs: score [N]; frame_state [N, T] int32 = state[t] for t < T_n, -1 beyond (always fully written);
 * token_start / token_end [N, L_max] int32 = the first frame with state 2i+1 / one past the last; token_logp [N, L_max] =
 * the float32 sum of lp[t, y_i] over the token's frames in ascending t; entries i >= L are -1 / -1 / 0 (the three may be
 * NULL when L_max = 0).
 * Two launches on `stream` (the normalisers: a wave per frame; the alignment: a workgroup per utterance), no host
 * synchronisation, no allocation, no bounded spin (hence no status word).  The 2-bit back-pointers of a frame are kept as two
 * 64-bit planes per 64 states, 16 ceil(S_max / 64) bytes per frame with S_max = 2 L_max + 1: in LDS while T such rows fit
 * MS_CTC_ALIGN_BP_LDS_BYTES, else in the workspace (ms_ctc_align_workspace_bytes: host arithmetic; 0 for N <= 0; it grows
 * by N T rows exactly when they leave the LDS).  Supported: T <= 8192, L_max <= 1023, any V; beyond that
 * MS_ERR_UNSUPPORTED and nothing is launched. */
#define MS_CTC_ALIGN_BP_LDS_BYTES 98304
size_t ms_ctc_align_workspace_bytes(int T, int N, int V, int S_max);
int ms_ctc_align(const float* x, const int32_t* in_lens, const int32_t* targets, const int32_t* tgt_offsets,
                 const int32_t* tgt_lens, float* score, int32_t* frame_state, int32_t* token_start, int32_t* token_end,
                 float* token_logp, int T, int N, int V, int L_max, int blank, int flags, void* workspace,
                 size_t workspace_bytes, void* stream);

/* ---- post_process/ctc_beam_decoder.py ------------------------------------ */

size_t ms_ctc_beam_workspace_bytes(int T, int N, int V, int beam_width);

/* CTCBeamDecoder.forward (ctc_beam_decoder.py:175-258): prefix beam search in
 * linear float32 arithmetic in the reference's visiting order, bit-exact beam.
 * probs [T,N,V] normalised.  separator < 0 = None; word_factor [T+2] (or NULL
 * when separator < 0) holds float32((1 + n_words) ** word_weight) for
 * n_words = 0..T+1, evaluated by the host exactly as ctc_beam_decoder.py:248-253.  One call advances every
 * utterance over time steps [t_begin, t_end); state persists in `workspace`
 * (t_begin = 0 initialises it), so a host language model can be consulted
 * between steps: lm_factor [N, beam_width] float32 (or NULL) multiplies the
 * separator extension of beam entry w (= float32(lm(l+sep) ** lm_weight),
 * ctc_beam_decoder.py:222-228).  When finish != 0 the best prefix of each
 * utterance is written to out_idx [N, T] / out_len [N]; beam_len [N] and
 * beam_idx [N, beam_width, T] / beam_plen [N, beam_width] (may be NULL) expose
 * the current beam for the LM callback. */
int ms_ctc_beam_decode(const float* probs, const int32_t* lens, int32_t* out_idx, int32_t* out_len, int T, int N,
                       int V, int blank, int beam_width, float prune_threshold, int separator, const float* word_factor,
                       int t_begin, int t_end, const float* lm_factor, int finish, int32_t* beam_len,
                       int32_t* beam_idx, int32_t* beam_plen, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ms_ctc_beam_decode over a WINDOW of the clip's rows (a streaming caller holds only the rows of the current chunk):
 * probs [rows_held, N, V] holds rows [row0, row0 + rows_held) of the clip and frame t is read at row t - row0;
 * row0 <= t_begin and t_end - row0 <= rows_held.  T stays the clip's total number of frames (it sizes the trie in the
 * workspace and out_idx / beam_idx), every stream is present in every window (ended ones are skipped through lens), and
 * everything else is ms_ctc_beam_decode, which is the row0 = 0, rows_held = T case of the same code.  finish != 0 with
 * t_begin == t_end writes the current best prefix without disturbing the search. */
int ms_ctc_beam_decode_rows(const float* probs, const int32_t* lens, int32_t* out_idx, int32_t* out_len, int T, int N,
                            int V, int blank, int beam_width, float prune_threshold, int separator,
                            const float* word_factor, int t_begin, int t_end, int row0, int rows_held,
                            const float* lm_factor, int finish, int32_t* beam_len, int32_t* beam_idx, int32_t* beam_plen,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---- n-gram language model (myrtlespeech_amd/language_model.py) ----------- */

/* A word-level back-off n-gram model as ONE contiguous little-endian blob, packed for one lm_weight by
 * NGramLanguageModel.packed and walked identically by NGramLanguageModel.factor (host) and csrc/ngram_lm.h (device):
 *
 *   header, 16 uint32 words (64 bytes):
 *     0 magic 0x4D4C534D ("MSLM")   1 order (1 .. MS_NGRAM_MAX_ORDER)   2 log2(vocabulary slots)   3 log2(n-gram slots)
 *     4, 5 vocabulary hash seed (lo, hi)   6, 7 n-gram hash seed (lo, hi)   8 id of <s> (int32, -1: none)   9 id of <unk>
 *     10 longest probe run of the vocabulary table   11 ... of the n-gram table (slots examined to reach any stored key)
 *     12 byte offset of the vocabulary table   13 ... of the n-gram table (multiples of 16)   14 size of the blob   15 words
 *   vocabulary table, 16 bytes per slot: {uint64 key, int32 word id, 0}; key = fin(h), h = step(...step(seed, s1)..., sk)
 *     over the word's symbols s1 .. sk
 *   n-gram table, 16 bytes per slot: {uint64 key, float32 p ** lm_weight, float32 backoff ** lm_weight} (1.0 where the
 *     file gives no back-off); key = fin(step(h, n)), h = step(...step(seed, id1)..., idn) over the n word ids
 *   step(h, x) = (h ^ (x + 1)) * 0x100000001B3 mod 2^64;  fin = the 64-bit murmur3 finaliser, 0 mapped to 1.
 *
 * Open addressing, power-of-two slot counts, load <= 0.5, linear probing from key & (slots - 1); key 0 = empty slot.  A
 * look-up examines at most the recorded number of slots, so a damaged table cannot keep a kernel from ending.  Keys are
 * compared in full and no two stored keys are equal (the packer re-seeds until so); a spelling outside the vocabulary
 * that hashes onto a stored key (probability ~ words / 2^64) is scored as that word, on the host and the device alike.
 *
 * The factor of a prefix: drop one trailing separator, split on runs of the separator; the scored word w is what follows
 * the last separator (none: the factor is 1.0), the context the up-to-(order - 1) words before it, preceded by <s> when
 * fewer exist and the model has <s>; unknown spellings are <unk>.  Then, starting from float32 1 and rounding after every
 * multiply: for k = context length down to 0, if (last k context words, w) is stored multiply by its p-factor and stop;
 * else if k > 0 and (last k context words) is stored multiply by its backoff-factor. */
#define MS_NGRAM_MAX_ORDER 5

/* Host-only validation of a packed blob (magic, order, slot counts, offsets and sizes inside `bytes`, probe bounds <=
 * slots, special ids < words); runs without a GPU.  MS_OK or MS_ERR_INVALID (ms_last_error says what). */
int ms_ngram_lm_table_check(const void* blob_host, size_t bytes);

/* Scores P prefixes against a table: prefixes [P, L] int32 padded, prefix_lens [P], out [P] float32 = the factor defined
 * above.  table: the blob in device memory; header_host: its first 64 bytes in HOST memory (re-validated here against
 * table_bytes; the device copy is never read by the host). */
int ms_ngram_lm_score(const void* table, const void* header_host, size_t table_bytes, const int32_t* prefixes,
                      const int32_t* prefix_lens, float* out, int P, int L, int separator, void* stream);

/* ms_ctc_beam_decode_rows with the language model in device memory: the separator extension of beam entry l is
 * multiplied by the factor of l + (separator,) looked up inside the frame loop (computed at most once per prefix), so a
 * decode with a model is one launch.  lm_table / lm_header_host / lm_table_bytes as for ms_ngram_lm_score; separator >= 0.
 * The workspace (ms_ctc_beam_lm_workspace_bytes; t_begin = 0 initialises it) additionally carries every prefix's model
 * state, so a decode advanced in pieces equals the decode in one call.  Everything else as ms_ctc_beam_decode_rows. */
size_t ms_ctc_beam_lm_workspace_bytes(int T, int N, int V, int beam_width, int order);
int ms_ctc_beam_decode_lm(const float* probs, const int32_t* lens, int32_t* out_idx, int32_t* out_len, int T, int N,
                          int V, int blank, int beam_width, float prune_threshold, int separator,
                          const float* word_factor, int t_begin, int t_end, int row0, int rows_held, const void* lm_table,
                          const void* lm_header_host, size_t lm_table_bytes, int finish, int32_t* beam_len,
                          int32_t* beam_idx, int32_t* beam_plen, void* workspace, size_t workspace_bytes, void* stream);

/* The three entry points above in one, plus the range-safe search and the scored beam.  The arguments of
 * ms_ctc_beam_decode_rows, then the optional device model of ms_ctc_beam_decode_lm (lm_table = lm_header_host = NULL:
 * none; with one, lm_factor must be NULL and the workspace is sized by ms_ctc_beam_lm_workspace_bytes, otherwise by
 * ms_ctc_beam_workspace_bytes), then:
 *   range_safe != 0: after every frame whose new best beam entry has a stored Pb + Pnb (float32, without the word-count
 *     factor) below 2^-32, every stored probability of that frame -- the beam's and the frame's candidate tables -- is
 *     multiplied by 2^-e, e = that sum's unbiased exponent (floor(log2), -126 for a subnormal), and e is added to the
 *     utterance's int32 scale_log2, kept in the workspace: true value = stored value * 2^scale_log2.  The multiplication
 *     is exact and the same for every entry, so pruning, model and word factors, the `> 0` test, tie order and every later
 *     rounding are those of ms_ctc_beam_decode: the transcripts are the same wherever that search stays in float32's normal
 *     range, and the beam does not run empty where it underflows.  range_safe == 0 runs the kernels of the entry points
 *     above.  A workspace begun in one mode (t_begin = 0) continues in that mode.
 *   beam_score [N, beam_width] float32 and scale_log2 [N] int32 (both or neither NULL; they need beam_len / beam_idx /
 *     beam_plen): the stored Pb + Pnb of beam entries 0 .. beam_len[n] - 1 in beam order and the utterance's scale (0
 *     with range_safe == 0); ln P(entry) = ln(beam_score) + scale_log2 * ln 2.  Entries past beam_len[n] are not written. */
int ms_ctc_beam_decode_ex(const float* probs, const int32_t* lens, int32_t* out_idx, int32_t* out_len, int T, int N,
                          int V, int blank, int beam_width, float prune_threshold, int separator,
                          const float* word_factor, int t_begin, int t_end, int row0, int rows_held,
                          const float* lm_factor, int finish, int32_t* beam_len, int32_t* beam_idx, int32_t* beam_plen,
                          void* workspace, size_t workspace_bytes, void* stream, const void* lm_table,
                          const void* lm_header_host, size_t lm_table_bytes, int range_safe, float* beam_score,
                          int32_t* scale_log2);

/* ---- feature front-end: data/preprocess.py + builders/pre_process_step.py ---- */

/* torchaudio.transforms.MFCC as built by builders/pre_process_step.py:33-43 (torchaudio==0.4.0,
 * environment.yml:171; absent here, so the pipeline is restated from its published algorithm):
 * centred, reflect-padded STFT with `window` [n_fft] -> power -> mel_fb [n_mels, n_fft/2+1] ->
 * 10*log10(max(.,1e-10)) floored at (per-utterance max - top_db) -> dct [n_mfcc, n_mels].
 * wave [N, max_samples] zero-padded, wave_lens [N] (each > n_fft/2); dft [2*(n_fft/2+1), n_fft] holds
 * the cos rows then the -sin rows.  out [N, n_mfcc, T], T = 1 + max_samples/hop; utterance n has
 * 1 + wave_lens[n]/hop frames, later frames are zero (what data/batch.py:7-42 pads with); a
 * wave_lens[n] above max_samples counts as max_samples.  top_db < 0 disables the floor.
 * The dB step and its floor select like torch.clamp and torch.max, so a NaN, an Inf or an overflowing
 * sample makes every feature of its own utterance NaN (as in torchaudio) and touches no other utterance.
 * MS_ERR_WORKSPACE for a workspace below ms_mfcc_workspace_bytes. */
size_t ms_mfcc_workspace_bytes(int N, int T, int n_fft, int n_mels, int n_mfcc);
int ms_mfcc_forward(const float* wave, const int32_t* wave_lens, const float* window, const float* dft,
                    const float* mel_fb, const float* dct, float* out, int N, int max_samples, int T, int n_fft,
                    int hop, int n_mels, int n_mfcc, float top_db, void* workspace, size_t workspace_bytes,
                    void* stream);

/* MFCCLegacy.__call__ (data/preprocess.py:262-319) = python_speech_features==0.6 `mfcc`
 * (environment.yml:169; absent here, restated from its published algorithm) in float64: samples
 * scaled to the int16 range and truncated, pre-emphasis, rectangular frames of frame_len every
 * frame_step samples (zero-padded tail), |DFT_nfft|^2/nfft, fbank [nfilt, nfft/2+1], log,
 * dct [numcep, nfilt], lifter [numcep], coefficient 0 := log(frame energy).  twiddle [nfft, 2] holds
 * (cos, sin)(2 pi j / nfft).  out [N, numcep, T] float32, T = frame count of max_samples; frames
 * past an utterance's own count are zero; a wave_lens[n] above max_samples counts as max_samples. */
int ms_mfcc_legacy_forward(const float* wave, const int32_t* wave_lens, const double* twiddle, const double* fbank,
                           const double* dct, const double* lifter, float* out, int N, int max_samples, int T,
                           int frame_len, int frame_step, int nfft, int nfilt, int numcep, double preemph,
                           void* stream);

/* Standardize.__call__ (data/preprocess.py:57-63) per utterance: y = (x - mean) / std (unbiased)
 * over x[n, :, t < lens[n]]; x, y [N, inner, T]; frames t >= lens[n] are written as 0.  lens may be
 * NULL (every utterance is T frames long).  y may alias x.  MS_ERR_WORKSPACE for a workspace below
 * ms_standardize_workspace_bytes. */
size_t ms_standardize_workspace_bytes(int N);
int ms_standardize_forward(const float* x, const int32_t* lens, float* y, int N, int inner, int T, void* workspace,
                           size_t workspace_bytes, void* stream);

/* AddContextFrames.__call__ (data/preprocess.py:117-141): x [N, F, T] -> y [N, 2c+1, F, T],
 * y[n,w,f,t] = x[n,f,t+w-c] when both t and t+w-c lie inside utterance n, else 0. */
int ms_context_frames_forward(const float* x, const int32_t* lens, float* y, int N, int F, int T, int n_context,
                              void* stream);

/* SpecAugment.__call__ (data/preprocess.py:193-218), the zeroing half: the host draws the bands in
 * the reference's order; f_bands [N, n_f, 2] / t_bands [N, n_t, 2] hold (start, width) int32 pairs
 * on the device.  x [N, C, F, T] is modified in place. */
int ms_spec_augment_(float* x, const int32_t* f_bands, const int32_t* t_bands, int N, int C, int F, int T, int n_f,
                     int n_t, void* stream);

/* ---- RNN-T decode step (own specification: the reference snapshot has no transducer,
 *      SURVEY 0.3 / 8 a15; see myrtlespeech_amd/model/rnnt.py) ------------------------------ */

/* out[r,:] = table[idx[r],:]  (prediction-network embedding; idx clamped to [0, V1)). */
int ms_embedding_forward(const float* table, const int32_t* idx, float* out, int R, int D, int V1, void* stream);

/* logp[r,:] = log_softmax(w_out . tanh(enc_p[enc_row[r],:] + pred_p[r,:]) + b_out) for R hypothesis rows;
 * enc_p [*, J] are the projected encoder frames, pred_p [R, J] the projected predictor outputs. */
int ms_rnnt_joint_forward(const float* enc_p, const int32_t* enc_row, const float* pred_p, const float* w_out,
                          const float* b_out, float* logp, int R, int J, int V1, void* stream);

/* Per row b of scores [B, C]: the k largest entries in descending order (ties -> lowest index); k may exceed C.
 * -inf entries are never selected, and neither is a NaN (no comparison with it holds: a row's NaN scores are passed over as
 * if they were -inf); the places left when fewer than k entries lie above -inf hold (index -1, value -inf). */
int ms_rnnt_topk(const float* scores, int32_t* out_idx, float* out_val, int B, int C, int k, void* stream);

/* Whole-batch RNN-T decode on the device (own specification, oracle/rnnt_oracle.py): one call enqueues the
 * complete frame loop; nothing is read back until the caller synchronises.  enc_p [T*N, J] are the encoder frames
 * after RNNTJoint.enc_proj (row t*N + n); the prediction network is Embedding(V+1, D) + L LSTM layers given in
 * torch layout (w_ih[l] [4H, In_l], w_hh[l] [4H, H], b_ih[l] / b_hh[l] [4H] or NULL, gate order i,f,g,o), w_pred
 * [J, H] (no bias), w_out [V+1, J], b_out [V+1]; blank = V.
 * greedy != 0: per frame, emit argmax labels until blank, at most max_symbols per frame; out_idx [N, T*max_symbols].
 * greedy == 0: time-synchronous beam search of width beam_width (<= 32) with max_symbols rounds per frame (blank
 * transitions of equal prefixes merged by float32 logaddexp evaluated in float64; the beam_width best label
 * extensions, ties to the lowest (hypothesis, label) index, stay live); out_idx [N, T*(max_symbols-1) + 1].
 * out_len [N]; out_score [N] (beam only, may be NULL) is the log-probability of the returned hypothesis.
 * The greedy decode is the one entry point besides ms_rnn_status that BLOCKS the host: the number of iterations depends on
 * the labels emitted, so the host polls a device counter a few iterations behind the launch queue and returns once the last
 * poll's copy has landed (the beam decode only enqueues).  MS_ERR_HIP if the pinned counter ring cannot be created. */
size_t ms_rnnt_decode_workspace_bytes(int T, int N, int V, int D, int H, int L, int J, int beam_width, int max_symbols,
                                      int greedy);
int ms_rnnt_decode(const float* enc_p, const int32_t* lens, const float* embedding, const float* const* w_ih,
                   const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, const float* w_pred,
                   const float* w_out, const float* b_out, int32_t* out_idx, int32_t* out_len, float* out_score, int T,
                   int N, int V, int D, int H, int L, int J, int beam_width, int max_symbols, int greedy, void* workspace,
                   size_t workspace_bytes, void* stream);
/* Greedy iterations (joint of 32 frames per utterance, scan, predictor step) that the calling thread's last ms_rnnt_decode
 * enqueued; 0 after a beam call, a refused call or no call at all.  A record for tools and tests, like word [1] of the
 * streaming state below: an utterance is finished once its frame reaches its length (one of length <= 0 from the start), and
 * the host, which looks every second iteration at a counter fetched two looks earlier, stops within six iterations of that. */
long long ms_rnnt_decode_last_iterations(void);

/* The greedy decode advanced one chunk of encoder rows at a time (own specification: oracle/rnnt_oracle.py::greedy_decode
 * with its frame loop cut BETWEEN frames; restated in numpy by tests/rnnt_stream_ref.py).  The predictor's LSTM state and the
 * prefix it encodes survive the cut: everything a stream carries lives in `state`
 * (ms_rnnt_greedy_stream_state_bytes(N, H, L, J) bytes of device memory, 16-byte aligned; host arithmetic, 0 for a
 * non-positive shape): int32 words [0] the sticky overflow word, [1] iterations launched since _begin (a record for tools),
 * [2 .. 15] reserved, then four per stream i at [16 + 4 i]: label count, frames seen, two reserved; then, each aligned to 256
 * bytes, float32 h [N, L, H], c [N, L, H] (the predictor after the stream's prefix) and pred_p [N, J] = w_pred . h_top.
 * Network arguments as ms_rnnt_decode takes them (blank = V); they must be the same in _begin and in every _step.
 * `workspace`: ms_rnnt_greedy_stream_workspace_bytes(N, V, D, H, L, J) bytes, 16-byte aligned; nothing in it outlives a call,
 * so _begin and the steps of several decoders may share one.
 * _begin: clears the overflow word, sets every stream to zero labels, zero frames seen and zero h and c in every layer, takes
 * the predictor step on the start symbol and stores the resulting state and its pred_p.  The start step is the same for every
 * stream: it is computed once and broadcast.  Only enqueues.
 * _step: enc_p [rows * n, J], row r n + i, are the next `rows` projected encoder frames of the first n <= N streams (streams
 * leave a sorted batch as a suffix, as in ms_ctc_greedy_stream_step).  Rows that exist for stream i: chunk_lens[i] (clamped to
 * [0, rows]) if chunk_lens is given, otherwise clamp(total_lens[i] - frames_seen[i], 0, rows); exactly one of the two is
 * non-NULL.  frames_seen[i] advances by the rows that existed.  Per existing frame, in order: x = w_out . tanh(enc_p[row] +
 * pred_p_i) + b_out; the symbol is the arg max over the LOGITS x (first maximum wins; a row without a number counts as blank);
 * blank moves to the next frame; a label is appended, the stream's predictor takes one step on it (a new pred_p_i) and the same
 * frame is scored again; after max_symbols labels on one frame the frame advances.  A frame never spans two steps, so nothing
 * about the quota is carried.
 * labels [N, cap]: appended at the stream's running label count; label_frames [N, cap] (may be NULL): the 0-based index,
 * counted over the stream's existing rows since _begin, of the frame that emitted the label.  A stream that would exceed `cap`
 * labels stops appending, keeps counting, sets the overflow word and keeps advancing its predictor, so later labels are still
 * the right ones.  fresh [N, 1 + rows * max_symbols] (may be NULL): column 0 = labels this call appended for the stream (0 for
 * streams n .. N-1), columns 1.. = those labels.
 * Arithmetic: the joint's output layer as three fp16 MFMA products of hi + lo planes (f16x3, as ms_rnnt_score; MS_PRECISION is
 * not consulted), the predictor in float32 FMA.  DETERMINISM is part of the contract: the logit row of a (frame, prefix) pair
 * and the predictor state after a prefix are computed by the same sequence of operations wherever the rows are cut, wherever
 * the frame sits among the 32 a stream has scored at once, and whichever other streams are in the batch; transcripts and
 * label_frames of a clip are the same for every way of cutting it.
 * Non-finite input: a NaN or infinity in an existing row of one stream leaves that stream's labels unspecified (they stay
 * inside [0, V)); nothing is read or written out of bounds, the call ends within its bound, every other stream is unchanged.
 * Like the greedy ms_rnnt_decode, _step BLOCKS the host: the number of iterations (score 32 pending frames per stream, step the
 * predictor of the streams that emitted) depends on the labels, so the host polls a device counter of finished streams a few
 * iterations behind the launch queue and returns once the last poll's copy has landed.  It runs at most rows * max_symbols +
 * ceil(rows / 32) + 1 iterations whatever the device reports; no kernel waits on another workgroup (no spin, no status word).
 * For the same reason a step CANNOT be captured into a HIP graph.  MS_ERR_HIP if the pinned counter ring cannot be created.
 * Shapes: those of the greedy ms_rnnt_decode (at most 8 predictor layers) and any V and J; beyond them MS_ERR_UNSUPPORTED, and
 * nothing is launched. */
size_t ms_rnnt_greedy_stream_state_bytes(int N, int H, int L, int J);
size_t ms_rnnt_greedy_stream_workspace_bytes(int N, int V, int D, int H, int L, int J);
int ms_rnnt_greedy_stream_begin(void* state, int N, const float* embedding, const float* const* w_ih, const float* const* w_hh,
                                const float* const* b_ih, const float* const* b_hh, const float* w_pred, const float* w_out,
                                const float* b_out, int V, int D, int H, int L, int J, void* workspace, size_t workspace_bytes,
                                void* stream);
int ms_rnnt_greedy_stream_step(const float* enc_p, int rows, int n, const int32_t* total_lens, const int32_t* chunk_lens,
                               const float* embedding, const float* const* w_ih, const float* const* w_hh,
                               const float* const* b_ih, const float* const* b_hh, const float* w_pred, const float* w_out,
                               const float* b_out, int32_t* labels, int32_t* label_frames, int cap, int32_t* fresh, void* state,
                               int N, int V, int D, int H, int L, int J, int max_symbols, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ---- RNN-T (transducer) loss: forward, and the gradient with respect to the joint's logits.  OWN specification, like
 *      everything under the RNN-T label (the reference snapshot has no transducer; parity unpinned); restated in numpy by
 *      tests/rnnt_loss_ref.py.  Graves 2012, "Sequence Transduction with Recurrent Neural Networks", section 2.4.
 *
 * Inputs.  logits [N, T, U1, V1] float32, contiguous: joint-network outputs, not necessarily normalised.  U1 = U_max + 1,
 * V1 = number of symbols, blank any index in [0, V1).  Per utterance n: T_n = in_lens[n] in [1, T], U_n = tgt_lens[n] in
 * [0, U1 - 1]; labels y_0 .. y_{U_n - 1} = targets[n (U1 - 1) + u] (padded, int32), each in [0, V1) and != blank.  targets
 * may be NULL when U1 == 1.  All indexing is size_t (N T U1 V1 passes 2^31 at realistic sizes).
 *
 * Recursion, for the EXISTING cells t < T_n, u <= U_n, in natural-log float32:
 *   Z(t,u)     = logsumexp_v logits[n,t,u,:]   (max-subtracted)
 *   lp(t,u,v)  = logits[n,t,u,v] - Z(t,u);   b(t,u) = lp(t,u,blank);   e(t,u) = lp(t,u,y_u) for u < U_n
 *   alpha(0,0) = 0
 *   alpha(t,u) = logaddexp(alpha(t-1,u) + b(t-1,u), alpha(t,u-1) + e(t,u-1))     (a term whose predecessor lies outside the
 *                                                                                 lattice is absent)
 *   ll         = alpha(T_n-1, U_n) + b(T_n-1, U_n);   nll[n] = -ll
 *   beta(T_n-1, U_n) = b(T_n-1, U_n)
 *   beta(t,u)  = logaddexp(beta(t+1,u) + b(t,u), beta(t,u+1) + e(t,u))
 *   logaddexp(-inf, -inf) = -inf, never NaN; a -inf logit is allowed and means "impossible".
 *
 * Gradient of sum_n grad_nll[n] nll[n] with respect to the logits (log-softmax included), for an existing cell:
 *   grad[n,t,u,v] = grad_nll[n] ( exp(lp(t,u,v) + alpha(t,u) + beta(t,u) - ll)
 *                                 - [v == blank] exp(alpha(t,u) + b(t,u) + beta(t+1,u) - ll)
 *                                 - [u < U_n and v == y_u] exp(alpha(t,u) + e(t,u) + beta(t,u+1) - ll) )
 *   at (T_n-1, U_n) the blank term is exp(alpha + b - ll); for every other (T_n-1, u) it is 0.
 *   grad is always fully written: every element of a cell that does not exist is 0.
 *
 * Edge cases.
 *   ll = -inf (the transcript is impossible under the given -inf's): nll = +inf, the utterance's gradient all 0.
 *   a non-finite Z in an existing cell (a NaN or +inf logit, a row of -inf only): nll = NaN, the gradient NaN in the
 *     utterance's existing cells and 0 outside them.
 *   what lies in cells that do not exist (NaN included) and in targets past U_n changes no output bit.
 *   T_n outside [1, T], U_n outside [0, U1 - 1], a label outside [0, V1) or equal to blank: the caller's error; nothing is read
 *     out of bounds for it; nll = +inf and a zero gradient.
 *
 * Memory.  lattice is caller-owned float32 [3][N][T][U1] = Z, alpha, beta (ms_rnnt_loss_lattice_bytes = 12 N T U1); only its
 * existing cells are defined.  The forward writes it, the backward reads it (an autograd node saves it): the workspace is
 * transient and nothing is kept between the calls.  ms_rnnt_loss_workspace_bytes = 2 planes of N (T + U1 - 1) U1 floats,
 * each rounded up to 256 bytes: b and e, gathered by the normaliser pass and stored skewed by anti-diagonal, [n][t + u][u].
 * Both size queries are host arithmetic and return 0 for non-positive shapes.
 * Supported: U1 <= 1024, any T, any V1 >= 1 (and N T U1 < 2^33 cells); MS_ERR_UNSUPPORTED beyond, nothing launched.
 * Neither call synchronises the host or allocates.  Three passes -- normalisers (forward), lattice (forward; 2 N workgroups,
 * alpha and beta side by side), gradient (backward); no kernel waits on another workgroup, so there is no bounded spin and
 * no status word.  Results are deterministic: the same inputs give the same bits. */
size_t ms_rnnt_loss_lattice_bytes(int N, int T, int U1);
size_t ms_rnnt_loss_workspace_bytes(int N, int T, int U1, int V1);
int ms_rnnt_loss_forward(const float* logits, const int32_t* in_lens, const int32_t* targets, const int32_t* tgt_lens,
                         float* nll, float* lattice, int N, int T, int U1, int V1, int blank, void* workspace,
                         size_t workspace_bytes, void* stream);
int ms_rnnt_loss_backward(const float* logits, const int32_t* in_lens, const int32_t* targets, const int32_t* tgt_lens,
                          const float* nll, const float* lattice, const float* grad_nll, float* grad, int N, int T, int U1,
                          int V1, int blank, void* stream);

/* ---- RNN-T scoring without the logit lattice: the joint network fused into the loss's normaliser pass.  OWN specification;
 *      restated in numpy by tests/rnnt_score_ref.py on top of tests/rnnt_loss_ref.py.
 *
 * nll[n] = -log P(y_n | audio_n) of ms_rnnt_loss_forward for the logits
 *   x(n,t,u)[v] = sum_j w_out[v, j] tanh(enc_p[t N + n, j] + pred_p[u N + n, j]) + b_out[v]
 * without ever storing them: for every EXISTING cell (t < T_n, u <= U_n) one MFMA kernel forms the row, its log-sum-exp Z
 * (online over column tiles), and keeps b(t,u) = x[blank] - Z and e(t,u) = x[y_u] - Z (u < U_n) in the two skewed planes of
 * the workspace; the loss's own lattice pass then gives alpha, beta and nll.  The recursion and EVERY edge case are those of
 * ms_rnnt_loss_forward above: lengths out of range, a label out of range or equal to blank: nll = +inf; an impossible
 * transcript (ll = -inf): +inf; a non-finite Z in an existing cell (a NaN anywhere in the cell's inputs, a +inf logit, a row
 * of -inf only): NaN for that utterance alone.  A -inf in b_out is allowed and means "impossible symbol".  What lies in rows
 * t >= T_n of enc_p, in rows u > U_n of pred_p and in targets past U_n changes no output bit.
 *
 * Inputs.  enc_p [T*N, J], row t N + n: the projected encoder frames, as ms_rnnt_decode takes them.  pred_p [U1*N, J], row
 * u N + n: the projected predictor output after y_n[:u] (u = 0: after the start symbol).  w_out [V1, J], b_out [V1] or NULL
 * (zeros).  in_lens, targets [N, U1 - 1] (NULL iff U1 == 1), tgt_lens, blank as for the loss.  J >= 1 and V1 >= 1 arbitrary.
 * Arithmetic: the products are f16x3 (both operands split into fp16 hi + lo, three fp16 MFMAs, float32 accumulation),
 * whatever MS_PRECISION says; error bound in tests/test_rnnt_score_gpu.py, stated for |w_out| within [2^-10, 2^10].
 *
 * Memory.  lattice is caller-owned float32 [2][N][T][U1] = alpha, beta (ms_rnnt_score_lattice_bytes = 8 N T U1; there is no
 * Z plane: this call has no backward); only existing cells are defined.  ms_rnnt_score_workspace_bytes = the two skewed
 * planes of the loss plus w_out split and packed in MFMA operand order (4 bytes per element of w_out padded to 128 symbols
 * x 64 features); the workspace must be 16-byte aligned, is transient, and is rewritten by every call (the packing is one
 * small launch of the call).  Both size queries are host arithmetic and return 0 for non-positive shapes.
 * Supported: U1 <= 1024 (and N T U1 < 2^33 cells), as the loss; MS_ERR_UNSUPPORTED beyond, nothing launched.
 * The call neither synchronises nor allocates.  Three launches (pack, cells, lattice); no workgroup waits on another, no
 * atomics: the same inputs give the same bits. */
size_t ms_rnnt_score_lattice_bytes(int N, int T, int U1);
size_t ms_rnnt_score_workspace_bytes(int N, int T, int U1, int J, int V1);
int ms_rnnt_score(const float* enc_p, const float* pred_p, const float* w_out, const float* b_out, const int32_t* in_lens,
                  const int32_t* targets, const int32_t* tgt_lens, float* nll, float* lattice, int N, int T, int U1, int J,
                  int V1, int blank, void* workspace, size_t workspace_bytes, void* stream);

/* ---- The fused transducer loss WITH its gradient: ms_rnnt_score's forward plus a Z plane, and a backward with respect to
 *      enc_p, pred_p, w_out and b_out that never holds a V1-wide row per cell for the whole lattice.  OWN specification;
 *      restated in numpy by tests/rnnt_joint_loss_ref.py on top of tests/rnnt_loss_ref.py and tests/rnnt_score_ref.py.
 *
 * Forward.  ms_rnnt_joint_loss_forward takes ms_rnnt_score's arguments (its workspace is ms_rnnt_score_workspace_bytes) and
 * runs the same three launches; lattice is float32 [3][N][T][U1] = Z, alpha, beta as for ms_rnnt_loss_forward
 * (ms_rnnt_joint_loss_lattice_bytes = 12 N T U1), Z = NaN in a cell whose Z is not finite.  nll, alpha and beta are
 * ms_rnnt_score's bit for bit.
 *
 * Backward.  For an existing cell c = (n, t, u), t < T_n, u <= U_n:
 *   h_c = tanh(enc_p[t, n] + pred_p[u, n]);   x_c = w_out h_c + b_out;   Z, b, e, alpha, beta, ll as for ms_rnnt_loss_forward
 * and the gradient of sum_n grad_nll[n] nll[n] is
 *   g_c[v]  = grad_nll[n] ( exp(x_c[v] - Z_c + alpha_c + beta_c - ll_n)
 *                           - [v == blank] exp(alpha_c + b_c + beta(t+1, u) - ll_n)     (at (T_n-1, U_n): exp(alpha + b - ll);
 *                                                                                        at every other (T_n-1, u): 0)
 *                           - [u < U_n, v == y_u] exp(alpha_c + e_c + beta(t, u+1) - ll_n) )
 *   d_b_out[v]      = sum_c g_c[v]
 *   d_w_out[v, j]   = sum_c g_c[v] h_c[j]
 *   da_c[j]         = (sum_v g_c[v] w_out[v, j]) (1 - h_c[j]^2)
 *   d_enc_p[t, n]   = sum_{u <= U_n} da_(n,t,u)
 *   d_pred_p[u, n]  = sum_{t < T_n} da_(n,t,u)
 * Edge cases mirror the loss.  An utterance with nll = +inf (an impossible transcript, the caller's errors in lengths or
 * labels) contributes nothing to any gradient.  A NaN utterance: its own existing rows of d_enc_p and d_pred_p are NaN, and
 * so are d_w_out and d_b_out (they are shared across utterances); every other utterance's rows stay clean.  Rows t >= T_n of
 * d_enc_p[:, n] and rows u > U_n of d_pred_p[:, n] are written as 0; what lies in those INPUT rows and in targets past U_n
 * changes no output bit.  All four gradients are always fully written.  d_b_out may be NULL (not wanted); b_out NULL: zeros.
 *
 * Arithmetic.  The three products -- the recomputed x = H w_out^T, dH = G w_out and d_w_out = G^T H -- are f16x3 on MFMA
 * (both operands split into fp16 hi + lo, three products, float32 accumulation), whatever MS_PRECISION says.  The logits are
 * recomputed with the forward's planes and K order: they are the forward's bit for bit.  G is split as 2^12 g and the scale
 * undone in the epilogues; the error bound (tests/test_rnnt_joint_loss_gpu.py) is stated for |w_out| within [2^-10, 2^10]
 * and |grad_nll| within [2^-10, 8].
 *
 * Memory.  The backward walks the cells in BANDS of units (8 frames of one utterance, every prediction row): per band row
 * it holds g twice (row-major and transposed) and h once as fp16 hi + lo, and da as float32 -- 8 (V1p + Jp) bytes, V1p and
 * Jp = V1 and J rounded up to 128 -- plus w_out packed twice and the partial sums of the d_w_out product, whose K extent is
 * split over workgroups (up to 64 x V1p x Jp floats).  ms_rnnt_joint_loss_backward_workspace_min_bytes is one unit,
 * ms_rnnt_joint_loss_backward_workspace_bytes the preferred size (as many units as fit in 500e6 bytes, at least one);
 * any 16-byte aligned workspace of at least the minimum is accepted, MS_ERR_WORKSPACE below it.  A larger one only buys
 * larger bands.  The size queries are host arithmetic in size_t and return 0 for non-positive shapes.
 * Supported: U1 <= 1024 (and N T U1 < 2^33 cells), as the scorer; MS_ERR_UNSUPPORTED beyond, nothing launched.
 * Neither call synchronises or allocates.  Sums across bands are stream-ordered launches, sums inside a band run in a fixed
 * order; no atomics, no workgroup waits on another: the same inputs and the same workspace size give the same bits
 * (different workspace sizes may differ in rounding). */
size_t ms_rnnt_joint_loss_lattice_bytes(int N, int T, int U1);
int ms_rnnt_joint_loss_forward(const float* enc_p, const float* pred_p, const float* w_out, const float* b_out,
                               const int32_t* in_lens, const int32_t* targets, const int32_t* tgt_lens, float* nll,
                               float* lattice, int N, int T, int U1, int J, int V1, int blank, void* workspace,
                               size_t workspace_bytes, void* stream);
size_t ms_rnnt_joint_loss_backward_workspace_min_bytes(int N, int T, int U1, int J, int V1);
size_t ms_rnnt_joint_loss_backward_workspace_bytes(int N, int T, int U1, int J, int V1);
int ms_rnnt_joint_loss_backward(const float* enc_p, const float* pred_p, const float* w_out, const float* b_out,
                                const int32_t* in_lens, const int32_t* targets, const int32_t* tgt_lens, const float* nll,
                                const float* lattice, const float* grad_nll, float* d_enc_p, float* d_pred_p, float* d_w_out,
                                float* d_b_out, int N, int T, int U1, int J, int V1, int blank, void* workspace,
                                size_t workspace_bytes, void* stream);

/* ---- Transducer forced alignment: the best path of a GIVEN transcript through the lattice, i.e. the Viterbi (max-plus)
 *      form of the recursion ms_rnnt_loss_forward sums, its back-trace, and where every label is emitted.  OWN
 *      specification; restated in numpy by tests/rnnt_align_ref.py.
 *
 * Per utterance n the existing cells are t < T_n, u <= U_n; b(t,u) = lp(t,u,blank) and e(t,u) = lp(t,u,y_u) (u < U_n) exactly
 * as in the comment on ms_rnnt_loss_forward.  Recursion in natural-log float32, one rounding per addition and no other
 * arithmetic:
 *   d(0,0) = 0
 *   d(t,u): best = d(t-1,u) + b(t-1,u), k = 0                          (absent when t == 0)
 *           if u >= 1 and d(t,u-1) + e(t,u-1) > best (strictly, or when the blank predecessor is absent):
 *               best = that value, k = 1
 *           d(t,u) = best, back-pointer k        -- a tie takes the blank predecessor
 *   score = d(T_n-1, U_n) + b(T_n-1, U_n)
 * and the path is found by walking the back-pointers from (T_n-1, U_n) to (0,0).
 *
 * Edge cases.
 *   an impossible transcript (a -inf makes score = -inf): no path; every per-frame and per-token integer output is -1, every
 *     log-probability output of the utterance's own frames and labels -inf.
 *   a NaN or +inf b or e in an existing cell, or a non-finite normaliser of one: score = NaN for that utterance only; no path;
 *     the integer outputs are -1, the log-probability outputs NaN.
 *   T_n outside [1, T], U_n outside [0, U1 - 1], a label outside [0, V1) or equal to blank: the caller's error; nothing is read
 *     out of bounds for it; score = -inf and no path (frames and labels counted with the lengths clamped to the shapes).
 *   what lies in cells that do not exist and in targets past U_n changes no output bit.
 *
 * Outputs, always fully written:
 *   score       [N] float32           the score of the best path
 *   token_frame [N, U1 - 1] int32     the frame t at which label u is emitted (the step (t,u) -> (t,u+1)); -1 for u >= U_n
 *   token_logp  [N, U1 - 1] float32   e(token_frame[u], u); 0 for u >= U_n
 *   frame_u     [N, T] int32          the u at which the path takes the blank of frame t = the number of labels emitted through
 *                                     frame t; -1 for t >= T_n
 *   frame_logp  [N, T] float32        b(t, frame_u[t]); 0 for t >= T_n
 * (targets and the two token outputs may be NULL when U1 == 1).  score is, bit for bit, the float32 sum of those
 * log-probabilities in path order starting from 0: for each frame its emitted labels in order of u, then its blank.
 *
 * ms_rnnt_align takes logits [N, T, U1, V1] as the loss does.  flags = 0: logits in, the device runs the loss's own
 * normaliser pass (its Z goes to workspace scratch).  flags = MS_RNNT_LOG_PROBS_IN: b and e are x[n,t,u,blank] and
 * x[n,t,u,y_u] exactly as given (-inf is allowed and means "impossible").
 * ms_rnnt_align_joint takes ms_rnnt_score's inputs (enc_p, pred_p, w_out, b_out; see there) and runs its pack and cells
 * launches: there is no [N, T, U1, V1] tensor, and b, e carry the error bound of ms_rnnt_score.
 *
 * Memory.  d lives in registers: there is no alpha / beta lattice.  The back-pointer of a cell is one bit; a diagonal t + u of
 * an utterance is ceil(U1 / 64) 64-bit words, an utterance (T + U1 - 1) such rows: in LDS while they fit
 * MS_RNNT_ALIGN_BP_LDS_BYTES, else in the workspace.  ms_rnnt_align_workspace_bytes = the two skewed planes of the loss + Z
 * scratch of N T U1 floats; ms_rnnt_align_joint_workspace_bytes = ms_rnnt_score_workspace_bytes; each rounded up to 256
 * bytes and grown by the N utterances' back-pointer rows exactly when they leave the LDS.  The workspace must be 16-byte
 * aligned and is transient.  The size queries are host arithmetic and return 0 for non-positive shapes.
 * Supported: the shapes of ms_rnnt_loss_forward / ms_rnnt_score (U1 <= 1024); MS_ERR_UNSUPPORTED beyond, nothing launched.
 * Neither call synchronises nor allocates.  Two launches (planes; walk, back-trace and read-out: a workgroup per utterance),
 * three for the joint form; no workgroup waits on another, no atomics, no status word: the same inputs give the same bits. */
#define MS_RNNT_LOG_PROBS_IN 2
#define MS_RNNT_ALIGN_BP_LDS_BYTES 98304
size_t ms_rnnt_align_workspace_bytes(int N, int T, int U1, int V1);
int ms_rnnt_align(const float* logits, const int32_t* in_lens, const int32_t* targets, const int32_t* tgt_lens, float* score,
                  int32_t* token_frame, float* token_logp, int32_t* frame_u, float* frame_logp, int N, int T, int U1, int V1,
                  int blank, int flags, void* workspace, size_t workspace_bytes, void* stream);
size_t ms_rnnt_align_joint_workspace_bytes(int N, int T, int U1, int J, int V1);
int ms_rnnt_align_joint(const float* enc_p, const float* pred_p, const float* w_out, const float* b_out, const int32_t* in_lens,
                        const int32_t* targets, const int32_t* tgt_lens, float* score, int32_t* token_frame, float* token_logp,
                        int32_t* frame_u, float* frame_logp, int N, int T, int U1, int J, int V1, int blank, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- LSTM backward through time, and the embedding backward: what lets the transducer loss reach the prediction network.
 *      OWN specification; restated in float64 numpy by tests/lstm_backward_ref.py.
 *
 * One layer of a unidirectional torch.nn.LSTM, float32 throughout, weights in torch layout and read as stored (no packed
 * copy): w_ih [4H, In], w_hh [4H, H], b_ih / b_hh [4H] or NULL (zeros), gate order i, f, g, o:
 *   a_t = x_t w_ih^T + b_ih + h_{t-1} w_hh^T + b_hh;   i, f, o = sigmoid(a_i, a_f, a_o);   g = tanh(a_g)
 *   c_t = f c_{t-1} + i g;   h_t = o tanh(c_t)
 * Any H, In, N, T >= 1.  lens [N] int32 on the device, sorted descending, or NULL (every sequence has T steps), with the
 * forward's meaning: rows t >= lens[n] of the output are 0 and carry no gradient, h_n / c_n is the state at lens[n] - 1.
 * lens is read on the device only; max_len = lens[0] (T without lens) is the number of steps the backward runs.
 *
 * ms_lstm_recompute.  The forward saves no gates; this call rebuilds them from x [T,N,In] and the forward's output
 * h [T,N,H] (h0 / c0 [N,H], NULL = zeros).  Every h_{t-1} is known, so the pre-activations of all steps are two batch
 * products over T N rows (the exact float32 MFMA GEMM behind ms_linear_forward) into the workspace
 * (ms_lstm_recompute_workspace_bytes: two [T N, 4H] planes, each rounded up to 256 bytes; 0 for non-positive shapes), and
 * a scan with exact expf / tanhf writes gates [T,N,4H] (activated: i, f, g, o) and c [T,N,H] for t < lens[n].  Rows past a
 * length are not written, and nothing in them is read by ms_lstm_backward_steps.
 *
 * ms_lstm_backward_steps.  From gates, c, c0 (NULL = zeros), w_hh, d_out [T,N,H] (the gradient of the layer's output) and
 * d_hn / d_cn [N,H] (the gradients of the final states; either may be NULL), for t = lens[n] - 1 down to 0:
 *   dh_t = d_out[t] + dG_{t+1} w_hh  (+ d_hn at t == lens[n] - 1; no recurrent term there)
 *   dc_t = dh_t o (1 - tanh(c_t)^2) + f_{t+1} dc_{t+1}  (d_cn in place of the last term at t == lens[n] - 1)
 *   dG_t = [dc_t g i (1 - i), dc_t c_{t-1} f (1 - f), dc_t i (1 - g^2), dh_t tanh(c_t) o (1 - o)]
 * Outputs, always fully written: dG [T,N,4H] = the gradient of the pre-activations, rows t >= lens[n] exact zeros;
 * d_h0 = dG_0 w_hh and d_c0 = f_0 dc_0 [N,H] (d_c0 also carries dc between the steps); d_b [4H] = the column sums of dG.
 * The batch products that finish the layer -- dx = dG w_ih, d_w_ih = dG^T x, d_w_hh = dG^T h_prev -- are ordinary GEMMs
 * over T N rows and are left to ms_linear_forward.
 * Launches: one per step from t = max_len - 1 down to 0, and one for d_h0; stream order is the only dependency between
 * them -- no grid barrier, no spin wait, no persistent kernel.  A workgroup owns 32 hidden units for every n at every step,
 * so d_b and dc are plain read-modify-writes: no atomics, the same inputs give the same bits.  The product is float32 MFMA
 * (K = 4H), never split planes.  dG must be 16-byte aligned.  Neither call synchronises or allocates.
 *
 * ms_embedding_backward.  d_table[v, :] = the sum of d_out[r, :] over the rows r with clamp(idx[r], 0, V1 - 1) == v
 * (ms_embedding_forward's clamping rule), added in the order of r by one workgroup per table row: deterministic bits,
 * rows never looked up are written as zeros.  d_out [R, D], idx [R] int32, d_table [V1, D].
 *
 * Bidirectional layers (OWN specification; restated by tests/bilstm_backward_ref.py).  One layer of a bidirectional
 * torch.nn.LSTM is two such cells on the same x with their own weights.  Direction 0 is the recurrence above.  Direction 1
 * (reverse) is, for sequence n, the same cell run from t = lens[n] - 1 down to 0: h_prev(t) = h[t + 1] for t + 1 < lens[n]
 * and h0[1][n] at t = lens[n] - 1 (c_prev alike); its h_n / c_n is the state at t = 0.  Its backward therefore runs t = 0 up
 * to lens[n] - 1: d_hn / d_cn enter at t = 0 with no recurrent term there, dh_t = d_out[t] + dG_{t-1} w_hh,
 * d_h0[n] = dG[lens[n] - 1, n] w_hh (the row differs per sequence) and d_c0[n] = f dc at lens[n] - 1.  lens as above; rows
 * t >= lens[n] of dG are exact zeros in both directions.
 *
 * ms_lstm_recompute_dir is ms_lstm_recompute with `reverse`: h is that direction's [T,N,H] output, contiguous; reverse = 0
 * gives ms_lstm_recompute's bits (it is the same call).  With reverse = 1 the recurrent plane is the product of h[t + 1]
 * into rows 0 .. T - 2 and of h0 into row T - 1, the one row that product leaves free, so the workspace is
 * ms_lstm_recompute_workspace_bytes; the scan walks t downward with c in a register and takes the h0 row at
 * t = lens[n] - 1 (without h0 the bias alone, as at step 0 of direction 0).
 *
 * ms_lstm_backward_steps_bidir runs both recurrences in the same launches.  gates [2,T,N,4H], c [2,T,N,H] (direction
 * major: the two ms_lstm_recompute_dir results), c0 / d_hn / d_cn [2,N,H] or NULL, d_out [T,N,2H] as autograd hands the
 * layer's output gradient over -- direction d is read at column d H + j, no slicing pass.  Outputs dG [2,T,N,4H], d_h0 and
 * d_c0 [2,N,H], d_b [2,4H], all fully written.  max_len + 1 launches of grid (ceil(H / 32), 2): launch s serves
 * t = max_len - 1 - s of direction 0 and t = s of direction 1, the last one the two d_h0 products (direction 1 reads the A
 * row of sequence n at lens[n] - 1).  It is the step kernel of ms_lstm_backward_steps with a direction index, and keeps
 * every promise above: stream order only, no atomics, float32 MFMA over K = 4H, the same bits on every run; direction 0's
 * outputs are ms_lstm_backward_steps' bits.
 *
 * Errors: NULL pointers (other than the optional ones above) and non-positive shapes MS_ERR_INVALID, a short workspace
 * MS_ERR_WORKSPACE.  Out of scope: a single-launch recurrence, mixed precision (GRU / tanh cells: the next block). */
size_t ms_lstm_recompute_workspace_bytes(int T, int N, int H);
int ms_lstm_recompute(const float* x, const float* h, const float* h0, const float* c0, const int32_t* lens,
                      const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* gates, float* c,
                      int T, int N, int In, int H, void* workspace, size_t workspace_bytes, void* stream);
int ms_lstm_backward_steps(const float* gates, const float* c, const float* c0, const float* w_hh, const float* d_out,
                           const float* d_hn, const float* d_cn, const int32_t* lens, int max_len, float* dG, float* d_h0,
                           float* d_c0, float* d_b, int T, int N, int H, void* stream);
int ms_lstm_recompute_dir(const float* x, const float* h, const float* h0, const float* c0, const int32_t* lens,
                          const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* gates, float* c,
                          int T, int N, int In, int H, int reverse, void* workspace, size_t workspace_bytes, void* stream);
int ms_lstm_backward_steps_bidir(const float* gates, const float* c, const float* c0, const float* w_hh_fwd,
                                 const float* w_hh_rev, const float* d_out, const float* d_hn, const float* d_cn,
                                 const int32_t* lens, int max_len, float* dG, float* d_h0, float* d_c0, float* d_b, int T,
                                 int N, int H, void* stream);
int ms_embedding_backward(const float* d_out, const int32_t* idx, float* d_table, int R, int D, int V1, void* stream);

/* ---- GRU backward through time (csrc/rnn_backward.hip): what lets a loss reach the shipped DeepSpeech2's recurrent stack.
 *      OWN specification; restated in float64 numpy by tests/gru_backward_ref.py.
 *
 * One layer of torch.nn.GRU, float32 throughout, weights in torch layout and read as stored (no packed copy):
 * w_ih [3H, In], w_hh [3H, H], b_ih / b_hh [3H] or NULL (zeros), gate order r, z, n:
 *   r = sigmoid(x w_ir^T + b_ir + h_prev w_hr^T + b_hr)
 *   z = sigmoid(x w_iz^T + b_iz + h_prev w_hz^T + b_hz)
 *   q = h_prev w_hn^T + b_hn
 *   n = tanh(x w_in^T + b_in + r q)
 *   h_t = (1 - z) n + z h_prev
 * Any H, In, N, T >= 1.  lens [N] int32 on the device, sorted descending, or NULL (every sequence has T steps), with the
 * LSTM entries' meaning: rows t >= lens[n] of the output are 0 and carry no gradient, h_n is the state at lens[n] - 1 for
 * direction 0 and at t = 0 for the reverse direction.  The reverse direction is the same cell walked from lens[n] - 1 down
 * to 0: h_prev(t) = h[t + 1], and h0[1][n] at t = lens[n] - 1.
 *
 * Backward, direction 0, for t = lens[n] - 1 down to 0 (the reverse direction mirrors it from t = 0 up to lens[n] - 1):
 *   dh_t  = d_out[t] + z_{t+1} dh_{t+1} + dGh_{t+1} w_hh     (at t == lens[n] - 1: d_out[t] + d_hn, nothing carried in)
 *   da_n  = dh_t (1 - z)(1 - n^2)
 *   da_z  = dh_t (h_prev - n) z (1 - z)
 *   da_r  = da_n q r (1 - r)
 *   dGi_t = [da_r, da_z, da_n]        (the gradient of the input-side pre-activations)
 *   dGh_t = [da_r, da_z, da_n r]      (the gradient of the hidden-side ones)
 *   d_h0  = z_0 dh_0 + dGh_0 w_hh
 * d_b_ih / d_b_hh are the column sums of dGi / dGh.  The batch products that finish the layer -- dx = dGi w_ih,
 * d_w_ih = dGi^T x, d_w_hh = dGh^T h_prev -- are ordinary GEMMs over T N rows and are left to ms_linear_forward.
 *
 * ms_gru_recompute.  The forward saves no gates; this call rebuilds one direction's from x [T,N,In] and that direction's
 * contiguous output h [T,N,H] (h0 [N,H], NULL = zeros).  Every h_prev is known, so the pre-activations of all steps are two
 * batch products over T N rows (the exact float32 MFMA GEMM behind ms_linear_forward) into the workspace
 * (ms_gru_recompute_workspace_bytes: two [T N, 3H] planes, each rounded up to 256 bytes; 0 for non-positive shapes).  With
 * reverse = 1 the recurrent plane is the product of h[t + 1] into rows 0 .. T - 2 and of h0 into row T - 1, the one row that
 * product leaves free; without h0 the step a direction starts on takes the bias alone.  Then ONE elementwise kernel over
 * (t, n, j) with t < lens[n], exact expf / tanhf, writes gates [T,N,3H] (activated r, z, n) and q [T,N,H]: nothing is carried,
 * so unlike the LSTM recompute there is no scan.  Rows past a length are not written, and nothing in them is read by
 * ms_gru_backward_steps.
 *
 * ms_gru_backward_steps.  ndir is 1 or 2.  gates [ndir,T,N,3H]; q and h [ndir,T,N,H], direction major (for ndir == 1 h is the
 * layer's output itself); h0 and d_hn [ndir,N,H] or NULL; w_hh_rev NULL when ndir == 1; d_out [T,N,ndir H] as autograd hands
 * the layer's output gradient over -- direction d is read at column d H + j, no slicing pass.  Outputs, always fully written:
 * dGi and dGh [ndir,T,N,3H], rows t >= lens[n] exact zeros; d_h0 [ndir,N,H] (it also carries z dh between the launches);
 * d_b_ih and d_b_hh [ndir,3H].  max_len = lens[0] (T without lens) is the number of steps the backward runs.
 * Launches: max_len + 1 on a (ceil(H / 32), ndir) grid; launch s serves t = max_len - 1 - s of direction 0 and t = s of
 * direction 1, the last one the d_h0 products (direction 1 reads each sequence's OWN row lens[n] - 1 of dGh).  Stream order is
 * the only dependency between them -- no grid barrier, no spin wait, no persistent kernel.  A workgroup owns 32 hidden units
 * for every n at every step, so the bias sums and the carried z dh are plain read-modify-writes: no atomics, the same inputs
 * give the same bits, and direction 0's outputs of an ndir == 2 call are the ndir == 1 call's bits on the same direction-0
 * inputs.  The product is float32 MFMA over K = 3H (never split planes); rows of dGh are read in 16-byte quads where H % 4 == 0
 * and dGh is 16-byte aligned, element by element otherwise -- the same bits either way.  Neither call synchronises or allocates.
 *
 * Errors: NULL pointers (other than the optional ones above), non-positive shapes, reverse outside {0, 1}, ndir outside
 * {1, 2}, max_len outside [1, T] (or != T without lens) MS_ERR_INVALID; a short workspace MS_ERR_WORKSPACE.  Out of scope: a
 * single-launch recurrence, a K-split of the step product across workgroups, mixed precision. */
size_t ms_gru_recompute_workspace_bytes(int T, int N, int H);
int ms_gru_recompute(const float* x, const float* h, const float* h0, const int32_t* lens, const float* w_ih,
                     const float* w_hh, const float* b_ih, const float* b_hh, float* gates, float* q, int T, int N, int In,
                     int H, int reverse, void* workspace, size_t workspace_bytes, void* stream);
int ms_gru_backward_steps(const float* gates, const float* q, const float* h, const float* h0, const float* w_hh_fwd,
                          const float* w_hh_rev, const float* d_out, const float* d_hn, const int32_t* lens, int max_len,
                          float* dGi, float* dGh, float* d_h0, float* d_b_ih, float* d_b_hh, int T, int N, int H, int ndir,
                          void* stream);

/* ---- HardLSTM backward through time (csrc/rnn_backward.hip): what lets a loss reach DeepSpeech1(hard_lstm=True).
 *      OWN specification; restated in float64 numpy by tests/hard_lstm_backward_ref.py.
 *
 * One direction of one HardLSTM layer (model/hard_lstm.py: hard sigmoid, hard tanh), float32 throughout, weights in torch
 * layout and read as stored: w_ih [4H, In], w_hh [4H, H], b_ih / b_hh [4H] or NULL (zeros), gate order i, f, g, o.  HardLSTM
 * ignores sequence lengths: every sequence has T steps and neither call takes lens.
 *   a   = x_t w_ih^T + b_ih + h_prev w_hh^T + b_hh
 *   z_k = fl(fl(0.2f a_k) + 0.5f)   k in {i, f, o}      TWO roundings, never a fused multiply-add
 *   i, f, o = min(max(z_k, 0), 1);   g = min(max(a_g, -1), 1)
 *   c_t = f c_prev + i g;   h_t = o min(max(c_t, -1), 1)
 * The two-rounding clause: the forward kernels form 0.2f a + 0.5f fused, which gives the same value AFTER the clamp, but the
 * derivative is discontinuous in z and its gate is decided on z itself.  At a = -2.5 the fused form is -7.45e-9 (outside) where
 * the reference's two torch ops give exactly 0 (inside: torch.clamp passes the gradient on the closed interval).  The
 * backward follows the reference, so the recompute rounds twice.
 * Gradient gates, the reference's ops under torch autograd, both selects (never a multiply by 0 or 1; a NaN compares false):
 *   P(z) = 1 iff 0 <= z <= 1      torch.clamp: closed
 *   Q(v) = 1 iff -1 < v < 1       torch.nn.Hardtanh: open
 * Backward, direction 0, for t = T - 1 down to 0 (the reverse direction mirrors it from t = 0 up to T - 1, as in the LSTM block):
 *   dh_t = d_out[t] + dA_{t+1} w_hh                 (+ d_hn at the last step; no recurrent term there)
 *   dc_t = dh_t o Q(c_t) + f_{t+1} dc_{t+1}         (d_cn in place of the carried term at the last step)
 *   dA_t = [0.2 dc_t g P(z_i),  0.2 dc_t c_prev P(z_f),  dc_t i Q(a_g),  0.2 dh_t clamp11(c_t) P(z_o)]
 *   d_h0 = dA_first w_hh;   d_c0 = f_first dc_first;   d_b = the column sums of dA
 * each product rounded on its own in autograd's order ((dc g), the select, then the 0.2), so that on inputs whose forward
 * values are exact dA, d_c0 and d_b are torch float32 autograd's bits.
 *
 * ms_hard_lstm_recompute.  ms_lstm_recompute_dir's two batch products (the same workspace:
 * ms_lstm_recompute_workspace_bytes) and a scan that writes gates [T,N,4H] = the PRE-CLAMP values z_i, z_f, a_g, z_o -- not the
 * activated gates: a gate of exactly 0 may come from z == 0, which passes a gradient, or from z < 0, which does not, so the
 * backward derives both the value and the gate from z; the memory is the soft entry's -- and c [T,N,H], unclamped.
 *
 * ms_hard_lstm_backward_steps.  ndir is 1 or 2.  gates [ndir,T,N,4H] and c [ndir,T,N,H] direction major (the recompute's
 * results), c0 / d_hn / d_cn [ndir,N,H] or NULL, w_hh_rev NULL when ndir == 1, d_out [T,N,ndir H] read in place (direction d at
 * column d H + j).  Outputs, always fully written: dA [ndir,T,N,4H] (16-byte aligned), d_h0 and d_c0 [ndir,N,H] (d_c0 also
 * carries dc between the launches), d_b [ndir,4H].  T + 1 launches of the step kernel of ms_lstm_backward_steps on a
 * (ceil(H / 32), ndir) grid with a third cell policy, and every promise of that block: stream order only, no atomics, float32
 * MFMA over K = 4H, the same bits on every run; direction 0 of an ndir == 2 call is the ndir == 1 call's bits.
 *
 * Errors: NULL pointers (other than the optional ones above), non-positive shapes, reverse outside {0, 1}, ndir outside
 * {1, 2} MS_ERR_INVALID; a short workspace MS_ERR_WORKSPACE.  Out of scope: a single-launch recurrence, a K-split of the step
 * product, mixed precision, dropout inside HardLSTM (the reference asserts there is none). */
int ms_hard_lstm_recompute(const float* x, const float* h, const float* h0, const float* c0, const float* w_ih,
                           const float* w_hh, const float* b_ih, const float* b_hh, float* gates, float* c, int T, int N, int In,
                           int H, int reverse, void* workspace, size_t workspace_bytes, void* stream);
int ms_hard_lstm_backward_steps(const float* gates, const float* c, const float* c0, const float* w_hh_fwd,
                                const float* w_hh_rev, const float* d_out, const float* d_hn, const float* d_cn, float* dA,
                                float* d_h0, float* d_c0, float* d_b, int T, int N, int H, int ndir, void* stream);

/* ---- training: convolution and lookahead backward (csrc/conv_backward.hip) -- OWN specification ---------------------
 *
 * The forward is ms_maskconv_forward's contract with groups == 1:
 *   y = act(b[co] + sum_{ci,kf,kt} w[co,ci,kf,kt] xm[n, ci, fo SF - pad_f + kf DF, to ST - pad_t + kt DT])
 * where xm is x with frames t >= min(lens[n], Tin) read as 0 and everything outside [0, Fin) x [0, Tin) read as 0.  w is
 * torch's [Cout, Cin, KF, KT] (no packed bank), x [N, Cin, Fin, Tin], y and dy [N, Cout, Fout, Tout], lens [N] or NULL.
 *
 * Gate: g = dy where act == MS_ACT_NONE or act_lo < y < act_hi strictly, +0 elsewhere: the saved OUTPUT decides, no
 * pre-activation is kept (y may be NULL when act == MS_ACT_NONE).
 *
 * ms_maskconv_backward_data:   dx[n,ci,fi,ti] = sum w[co,ci,kf,kt] g[n,co,fo,to] over every (co,kf,kt,fo,to) with
 *   fi = fo SF - pad_f + kf DF, ti = to ST - pad_t + kt DT, 0 <= fo < Fout, 0 <= to < Tout.  dx[n,:,:,t] = +0.0 for
 *   t >= lens[n] (a select: whatever g holds), and an input position that no window reads gets +0.0.  dx is fully written.
 * ms_maskconv_backward_weight: dw[co,ci,kf,kt] = sum_{n,fo,to} g[n,co,fo,to] xm[...] over in-range positions,
 *   db[co] = sum_{n,fo,to} g (db may be NULL).  A masked or padded position is a load predicate, never a product with what
 *   memory holds there.  The reduction over K = N Fout Tout is cut into ceil(K / 8192) slices -- a function of the arguments
 *   only -- whose partials [slices][Cout][Cin KF KT + 1] go to the workspace (ms_maskconv_backward_workspace_bytes) and are
 *   added in ascending slice order by a second launch.
 *
 * Arithmetic: v_mfma_f32_32x32x2_f32, float32 accumulation, no atomics: the same bits on every run and every device.  One
 * route per gradient serves every geometry (the file's header comment): the data gradient tiles 32 input channels x 128
 * frames of one time-stride residue class, the weight gradient 32 output channels x 128 flattened (ci,kf,kt) columns.
 *
 * Errors: NULL operands and bad geometry (a non-positive extent, stride or dilation, a negative pad, an unknown act, an
 * output row or frame that starts past the input) MS_ERR_INVALID with nothing launched; a short workspace MS_ERR_WORKSPACE.
 * Out of scope: groups > 1.
 *
 * ms_lookahead_backward: forward z[n,f,t] = sum_{k<ctx} w[f,k] x[n,f,t+k] (zero beyond T), y = act(z); with the same gate
 *   dx[n,f,t] = sum_{k <= min(t, ctx-1)} w[f,k] g[n,f,t-k]   and   dw[f,k] = sum_n sum_{t: t+k<T} g[n,f,t] x[n,f,t+k]
 * (n, then t, ascending).  x / dx share the element strides xs_*, y / dy the strides ys_*, as in ms_lookahead_forward; w and
 * dw are [F, ctx].  Taps are guarded by k < ctx and t + k < T, never padded with zero weights.  dx or dw may be NULL (that
 * gradient is not wanted; x may then be NULL with dw). */
size_t ms_maskconv_backward_workspace_bytes(int N, int Cin, int Cout, int Fout, int Tout, int KF, int KT);
int ms_maskconv_backward_data(const float* w, const float* y, const float* dy, const int32_t* lens, float* dx, int N, int Cin,
                              int Fin, int Tin, int Cout, int Fout, int Tout, int KF, int KT, int SF, int ST, int DF, int DT,
                              int pad_f_l, int pad_t_l, int act, float act_lo, float act_hi, void* stream);
int ms_maskconv_backward_weight(const float* x, const float* y, const float* dy, const int32_t* lens, float* dw, float* db,
                                int N, int Cin, int Fin, int Tin, int Cout, int Fout, int Tout, int KF, int KT, int SF, int ST,
                                int DF, int DT, int pad_f_l, int pad_t_l, int act, float act_lo, float act_hi, void* workspace,
                                size_t workspace_bytes, void* stream);
int ms_lookahead_backward(const float* x, const float* w, const float* y, const float* dy, float* dx, float* dw, int N, int F,
                          int T, int ctx, long xs_n, long xs_f, long xs_t, long ys_n, long ys_f, long ys_t, int act,
                          float act_lo, float act_hi, void* stream);

/* ---- training: gradient norm, clip and the fused optimizer steps (csrc/optim.hip) -- OWN specification -----------------
 *
 * A tensor LIST is a host array of n device pointers (one array per role: parameters, gradients, each state) plus the host
 * array numels_host of n element counts.  Every tensor is float32, contiguous and 4-byte aligned -- NOT necessarily 16-byte
 * aligned: parameters may be views at odd offsets; the kernels move 16-byte quads where an array's body is so aligned and
 * single elements elsewhere, with the same bits either way.  A count may be 0 (the tensor is skipped; its pointers are not
 * read) and must be below 2^40.  The lists travel to the kernels by value, 48 tensors per launch; there is no device table.
 * Nothing synchronises, allocates or reads back.  Every multiply and add below is ONE rounded float32 operation (the file is
 * built with -ffp-contract=off), square root and division are correctly rounded (plain sqrtf and /, not __fsqrt_rn): tests/optim_ref.py restates the arithmetic
 * in numpy and the device is held to it bit for bit.
 *
 * ms_grad_norm: norm_out[0] = sqrtf(S), S the float32 sum of g*g over every element of every tensor; norm_out[1] = 1.0f where
 *   norm_out[0] is NaN or infinite, else 0.0f.  n == 0 or all-empty lists give {0, 0}.  Order of the additions -- a function of
 *   numels_host alone, so the same list gives the same bits on every run and at every alignment: a tensor is cut into chunks
 *   of 4096 elements by element index; in a chunk thread u of 256 adds the quads u, u + 256, .. (a quad is
 *   ((g0 g0 + g1 g1) + g2 g2) + g3 g3, the 1..3 elements after the last whole quad are summed on their own and added on the
 *   thread that the next quad would fall to); the 64 lanes of a wave meet in a butterfly (xor 32, 16, .. 1), the four waves
 *   are added in ascending order: one partial per chunk in the workspace, in list order.  A second launch of one workgroup
 *   adds the partials the same way (thread u takes partials u, u + 256, ..) and takes the root.
 *   ms_grad_norm_workspace_bytes is host arithmetic on the counts.
 *
 * The clip coefficient of the device word norm[0], in float32:  q = max_norm / (norm[0] + 1e-6f);  c = q where q < 1 or q is
 *   NaN, else 1.  A NaN norm therefore poisons what it scales (torch.nn.utils.clip_grad_norm_ does the same; fminf(1, q) would
 *   drop the NaN), an infinite norm gives c = 0.
 *
 * ms_grad_clip: g = g * c in place.
 *
 * ms_sgd_step, per element (torch.optim.SGD without dampening):
 *     g' = g * c                      only when norm != NULL; g itself is NOT written
 *     d  = g' + weight_decay * p      skipped when weight_decay == 0
 *     b  = momentum * b + d           skipped when momentum == 0 (bufs_host NULL; u = d)
 *     u  = nesterov ? d + momentum * b : b
 *     p  = p - lr * u
 *   Momentum buffers start as zeros (momentum * 0 + d == d: the first step is no special case).
 *
 * ms_adam_step, per element (torch.optim.Adam; the caller forms step_size = float32(lr / (1 - beta1^t)) and
 *   rsqrt_bc2 = float32(sqrt(1 - beta2^t)) in float64, from the FLOAT32 values of the betas -- there is no pow on the device; (1 - beta1) and (1 - beta2) are formed
 *   in float64 from the float32 arguments, rounded once to float32 on the host and passed to the kernel as scalars):
 *     g', d as above
 *     m  = beta1 * m + (1 - beta1) * d
 *     v  = beta2 * v + ((1 - beta2) * d) * d
 *     w  = amsgrad ? (vmax = (v > vmax or v is NaN) ? v : vmax) : v       max_exp_avg_sq_host NULL: no amsgrad
 *     den = sqrt(w) / rsqrt_bc2 + eps
 *     p  = p - step_size * (m / den)
 *
 * Both steps: with skip_nonfinite != 0 and norm[1] != 0 the kernels write NOTHING, neither p nor the state.
 *
 * Errors (MS_ERR_INVALID, nothing launched): n < 0, a NULL list that is not optional, a NULL or misaligned pointer of a
 * non-empty tensor, a count out of range, bufs_host without momentum or momentum without bufs_host, nesterov without momentum,
 * skip_nonfinite without norm; a short workspace MS_ERR_WORKSPACE.  Out of scope: other dtypes, dampening, decoupled weight
 * decay, capture of a step into a HIP graph across changing lists, multi-device reduction. */
size_t ms_grad_norm_workspace_bytes(const int64_t* numels_host, int n);
int ms_grad_norm(void* const* grads_host, const int64_t* numels_host, int n, float* norm_out, void* workspace,
                 size_t workspace_bytes, void* stream);
int ms_grad_clip(void* const* grads_host, const int64_t* numels_host, int n, const float* norm, float max_norm, void* stream);
int ms_sgd_step(void* const* params_host, void* const* grads_host, void* const* bufs_host, const int64_t* numels_host, int n,
                float lr, float momentum, float weight_decay, int nesterov, const float* norm, float max_norm,
                int skip_nonfinite, void* stream);
int ms_adam_step(void* const* params_host, void* const* grads_host, void* const* exp_avg_host, void* const* exp_avg_sq_host,
                 void* const* max_exp_avg_sq_host, const int64_t* numels_host, int n, float beta1, float beta2, float eps,
                 float weight_decay, float step_size, float rsqrt_bc2, const float* norm, float max_norm, int skip_nonfinite,
                 void* stream);

/* ---- training: dropout (csrc/dropout.hip) -- OWN specification ------------------------------------------------------------
 *
 * Every result is a pure function of its arguments: no generator state on the device, no stored mask, the same bits on every
 * run and every device, and a backward that RECOMPUTES the mask from the same four numbers.
 *
 * Generator: Philox4x32-10 -- multipliers 0xD2511F53 (on word 0) and 0xCD9E8D57 (on word 2), Weyl constants 0x9E3779B9 and
 *   0xBB67AE85 added to the key words after every round.  Known answers (counter, key -> output, words 0..3):
 *     0 0 0 0, 0 0                                              -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *     ffffffff x 4, ffffffff x 2                                -> 408f276d 41c83b0e a20bc7c6 6d5451fd
 *     243f6a88 85a308d3 13198a2e 03707344, a4093822 299f31d0    -> d16cfe09 94fdcceb 5001e420 24126ea1
 * Key and counter: a dropout CALL is (seed: u64, offset: u64).  For the flat element index e of the contiguous array the call
 *   covers, q = e >> 2 and lane = e & 3; counter = (q_lo, q_hi, offset_lo, offset_hi), key = (seed_lo, seed_hi),
 *   r = philox(counter, key)[lane].  e is relative to the ARRAY, not to its address: a view at an odd element offset gets the
 *   same mask.  One offset per call, so calls never overlap whatever their size.
 * Keep rule: the element is kept iff r >= thr, thr = ceil(p * 2^32) formed on the host in exact integer arithmetic from the
 *   double p, 0 < p <= 1; thr may be 2^32 (nothing is kept).  The uniform is never converted to float: the mask is exact.
 * Value: out[e] = x[e] * m[e], m[e] = scale where kept and +0.0f otherwise; scale = float32(1.0 / (1.0 - p)) formed in double
 *   on the host and rounded once, 0 for p == 1.  ONE float32 multiply, not a select: a NaN or an infinity in a dropped element
 *   stays visible, as in torch.nn.Dropout.  tests/dropout_ref.py restates all of this in numpy and the device is held to it
 *   bit for bit.
 *
 * ms_dropout_forward: out = x * m over n elements.  out may alias x.  Applied to a gradient with the forward's (thr, scale,
 *   seed, offset) it IS the backward of dropout: dx = dy * m.
 * ms_clamp_dropout_backward: dx[e] = (lo < y[e] && y[e] < hi) ? dy[e] * m[e] : 0, y the saved clamped PRE-dropout output of a
 *   linear layer with a fused clamp: the clamp's gate (a NaN y closes it) and the mask in one pass.
 *
 * Every array is float32, contiguous and 4-byte aligned; it moves as 16-byte quads where its base is 16-byte aligned and
 * element by element otherwise.  One lane owns one Philox quad; the grid is capped at 2048 workgroups of 256 and strides.
 * Errors (MS_ERR_INVALID, nothing launched): n < 0, a NULL or misaligned pointer with n > 0, thr == 0, thr > 2^32, a negative
 * or non-finite scale.  n == 0 is MS_OK with no launch.  Out of scope: dropout in a GEMM epilogue, other dtypes, torch's own
 * mask stream. */
int ms_dropout_forward(const float* x, float* out, int64_t n, uint64_t thr, float scale, uint64_t seed, uint64_t offset,
                       void* stream);
int ms_clamp_dropout_backward(const float* dy, const float* y, float* dx, int64_t n, float lo, float hi, uint64_t thr,
                              float scale, uint64_t seed, uint64_t offset, void* stream);

/* ---- post_process/edit_distance.py, wer.py (DeviceWordErrorRate) ---------- */

/* Batched edit distance with operation counts: what the reference's ReportCTCDecoder (run/run.py:50-109) computes on the host
 * with post_process/utils.py's levenshtein, per utterance, on the device.  tests/edit_distance_ref.py restates this comment.
 *
 * Rows: hyp [n, hyp_stride] and ref [n, ref_stride] int32 labels, of which row u holds hyp_lens[u] / ref_lens[u] (clamped to
 * [0, stride]); what lies past a row's length is never read.  A length of 0 is legal anywhere.
 * Units.  mode = MS_EDIT_TOKENS: a row's units are its labels, as they are (separator and n_symbols are ignored).
 *   mode = MS_EDIT_WORDS: first the labels outside [0, n_symbols) are dropped (Alphabet.get_symbols skips an index without a
 *   symbol; the CTC blank is one); the rest is cut at every label equal to `separator`; empty words are dropped (WordSegmentor).
 *   Two words are equal iff their label sequences are equal -- a hash only pre-filters.  separator = -1 (any value no kept
 *   label takes): no separator, the row is one word, or none if nothing was kept.
 * Distance and counts.  For hypothesis units a[0..m) and reference units b[0..n): D[i][0] = i insertions, D[0][j] = j deletions;
 *   cell (i, j) takes the cheapest of, in this order, (1) (i-1, j-1) + (a[i-1] != b[j-1]): a match or a substitution,
 *   (2) (i, j-1) + 1: a deletion (a reference unit the hypothesis lacks), (3) (i-1, j) + 1: an insertion; on equal cost the
 *   first in that order wins.  The counts (S, D, I) of the chosen predecessor travel with the cost and the cell adds its own
 *   operation.  out [n, 6] int32 = distance, S, D, I, m, n per utterance; distance is the reference's levenshtein(a, b);
 *   S + D + I == distance and m - I == n - D by construction.
 * totals: NULL, or int64 [6] (8-byte aligned) to which the six columns of this call are ADDED with integer atomics (any order
 *   gives the same bits); the caller zeroes it, e.g. once per epoch.
 * Launches on `stream`, no host read-back, no allocation: in word mode one workgroup per utterance turns both rows into unit
 * ids (the index of the first equal word among the utterance's hypothesis and reference words) in the workspace; then the
 * recurrence over anti-diagonals, a wave per utterance with the cells in registers when either side holds at most 63 units
 * by its row width (stride in token mode, (stride + 1) / 2 words), else a workgroup per utterance with three rolling
 * anti-diagonals in LDS.  LDS is sized by the strides, so a caller with short rows passes narrow matrices.
 * Supported: 4096 units a side by the row widths -- hyp_stride, ref_stride <= MS_EDIT_MAX_LEN in token mode and
 * <= 2 MS_EDIT_MAX_LEN - 1 in word mode (4096 one-letter words and their separators) -- beyond that MS_ERR_UNSUPPORTED and
 * nothing is launched; a workspace below ms_edit_distance_workspace_bytes(n, hyp_stride, ref_stride)
 * (host arithmetic; 0 for n <= 0) is MS_ERR_WORKSPACE; n = 0 is MS_OK with no launch.  Out of scope: the back-trace (which
 * unit was substituted for which), weighted costs. */
#define MS_EDIT_TOKENS 0
#define MS_EDIT_WORDS 1
#define MS_EDIT_MAX_LEN 4096
size_t ms_edit_distance_workspace_bytes(int n, int max_hyp, int max_ref);
int ms_edit_distance(const int32_t* hyp, int hyp_stride, const int32_t* hyp_lens, const int32_t* ref, int ref_stride,
                     const int32_t* ref_lens, int n, int mode, int separator, int n_symbols, int32_t* out, int64_t* totals,
                     void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MS_HOTPATH_H */
