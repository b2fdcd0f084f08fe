/*
 * include/edison_hip.h -- C-ABI of libedison_hip.so: edison's keyword-spotting hot path on MI355X (gfx950).
 *
 * This is the drop-in boundary. Plain C, plain pointers and sizes, int return codes; no torch types.
 * Every entry point names the reference interface it replaces (paths relative to the reference repo):
 *
 *   per-frame MFCC   audio/edison/mfcc/mfcc_utils.py:134 `mfcc` (variant A), :255 `mfcc_mcu` (variant B),
 *                    :75 `batch_mfcc`; C call surface firmware/src/audioprocessing.h:21-22
 *                    (`audioInit`, `audioCalcMFCCs`) and firmware/src/audio/mfcc.h:64-67 (`mfcc_compute`)
 *   net-input glue   firmware/src/app.c:675-695 `mfccToNetInput`, :706-719 `mfccToNetInputPush`
 *   int8 CNN         firmware/src/ai/ai.h:74-80 (`aiInitialize`, `aiGetInputShape`, `aiRunInference`,
 *                    `aiGetKeywordFromIndex`, `aiGetKeywordCount`), firmware/src/ai/ai_nnom.c:64-132
 *                    (`aiNnomInit`, `aiNnomRunInference`, `aiNnomPredict`, `aiNnomGet{Input,Output}Buffer`),
 *                    model = firmware/src/ai/nnom/kws_nnom/weights.h
 *
 * The reference processes ONE frame / ONE utterance per call on a Cortex-M4 (or in a Python loop). The
 * batched `edison_*_batch*` calls are the MI355X-native form of the same computation; the legacy names at
 * the bottom are batch=1 wrappers with the reference's own signatures and ownership rules.
 *
 * Conventions
 *   - return 0 (EDISON_OK == NNoM's NN_SUCCESS) or a negative code; edison_last_error() gives text.
 *   - `_dev` calls take DEVICE pointers (hipMalloc / torch CUDA tensors) and enqueue on the context's
 *     stream without synchronising; the others take HOST pointers and are synchronous.
 *   - one context per process per GPU; calls on one context are serialised by the caller.
 *   - there is NO CPU fallback: without a gfx950 device edison_init fails.
 */
#ifndef EDISON_HIP_H
#define EDISON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- constants of the hot path (audio/config.py:11-32, firmware/src/ai/ai.h:55-60) ------------------ */
#define EDISON_FS 16000
#define EDISON_FRAME_LEN 1024          /* frame_length = fft_len = frame_step                            */
#define EDISON_NUM_MEL 32              /* num_mel_bins                                                   */
#define EDISON_NUM_MFCC 13             /* num_mfcc (first_mfcc = 0)                                      */
#define EDISON_UTT_FRAMES 31           /* n_frames of a 2 s / 32000-sample utterance                     */
#define EDISON_NET_IN (EDISON_UTT_FRAMES * EDISON_NUM_MFCC) /* 403 int8, HWC [31][13][1]                 */
#define EDISON_NET_OUT 10

/* ---- status codes: 0 and the negatives mirror nnom_status_t (firmware/src/ai/nnom/inc/nnom.h:34-45) -- */
#define EDISON_OK 0                     /* NN_SUCCESS                                                    */
#define EDISON_E_ARGUMENT (-1)          /* NN_ARGUMENT_ERROR                                             */
#define EDISON_E_LENGTH (-2)            /* NN_LENGTH_ERROR                                               */
#define EDISON_E_SIZE (-3)              /* NN_SIZE_MISMATCH: model blob does not have the kws_conv shape  */
#define EDISON_E_NO_MEMORY (-7)         /* NN_NO_MEMORY (host or HBM allocation failed)                  */
#define EDISON_E_MORE_TODO (-8)         /* NN_MORE_TODO                                                  */
/* codes below have no NNoM counterpart */
#define EDISON_E_RUNTIME (-16)          /* HIP error, text in edison_last_error()                        */
#define EDISON_E_NO_IMPL (-17)          /* valid for the reference, not built on this path yet           */
#define EDISON_E_NO_DEVICE (-18)        /* no gfx950 GPU visible: the product has no CPU path            */
#define EDISON_E_NO_MODEL (-19)         /* CNN call before edison_model_load                             */

/* ---- MFCC variants ----------------------------------------------------------- */
#define EDISON_MFCC_A 0 /* mfcc_utils.mfcc    : fft[:512] -> |.| -> mel(512x32) -> ln(x+1e-6) -> dct2/sqrt(64) */
#define EDISON_MFCC_B 1 /* mfcc_utils.mfcc_mcu: fft/1024 -> |.|/sqrt2 -> mel(513x32) -> [ln] -> dct2/64        */
#define EDISON_MFCC_C 2 /* audioCalcMFCCs, the firmware's Q15 pipeline (firmware/src/audioprocessing.c:116-215):
                         * arm_cfft_q15(1024) -> arm_sqrt_q31 magnitude -> compact int16 mel / 128 -> RFFT-based dct2_q15.
                         * Integer-exact. Through the fp32 entry points below the outputs are the int16 values as
                         * floats (Cube branch of mfccToNetInput, app.c:680-683) and feat is the NNoM branch
                         * (app.c:686-694); feat_scale must be 1, no log. Native int16 interface: edison_mfcc_q15_*.  */
#define EDISON_MFCC_TF 3 /* mfcc_utils.mfcc_tf (mfcc_utils.py:201-253), the TensorFlow curve of `main.py mfcc host`:
                          * periodic Hann window (tf.signal.stft's default) -> rfft -> |.| -> mel(513x32) -> ln(x+1e-6) ->
                          * dct2/sqrt(64). Batch and stage entry points only (edison_mfcc_batch / _rows / _stages and
                          * their _dev forms); TensorFlow is not in this image, so this variant's parity is UNPINNED:
                          * it is checked against a float64 restatement of tf.signal's published definitions only.     */
#define EDISON_MFCC_USE_LOG 0x100 /* OR into variant: mfcc_mcu(..., use_log=True)                       */

typedef struct edison_ctx edison_ctx;

/* ---- lifecycle ---------------------------------------------------------------------------------------- */
int edison_init(int device, edison_ctx **out);
void edison_shutdown(edison_ctx *ctx);
const char *edison_last_error(const edison_ctx *ctx); /* ctx may be NULL: last init error                */
/* Enqueue on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream). The handle is used as
 * given: NULL is HIP's default (null) stream, NOT "no stream". edison_reset_stream returns to the context's own
 * private non-blocking stream (the state after edison_init). */
int edison_set_stream(edison_ctx *ctx, void *hip_stream);
int edison_reset_stream(edison_ctx *ctx);
int edison_sync(edison_ctx *ctx);
int edison_device_info(edison_ctx *ctx, char *name, int name_cap, int *n_cu, int64_t *hbm_bytes);

/* Mel filterbank parameters (defaults = audio/config.py). Rebuilds the device tables of both variants.
 * num_mel_bins must be 32 and the frame length 1024 on this path (EDISON_E_NO_IMPL otherwise). An upper edge above
 * sample_rate / 2 is accepted, as gen_mel_weight_matrix accepts it: the top bands end at the last spectrum bin.  */
int edison_mfcc_configure(edison_ctx *ctx, double sample_rate, double lower_edge_hertz, double upper_edge_hertz,
                          double mel_mtx_scale);

/* gen_mel_weight_matrix (mfcc_utils.py:36-73), host-side, float64: W[num_spectrogram_bins][num_mel_bins]. */
int edison_gen_mel_weight_matrix(int num_mel_bins, int num_spectrogram_bins, double sample_rate,
                                 double lower_edge_hertz, double upper_edge_hertz, double *W);

/* Load the int8 CNN (an .ednn blob written by tools/import_weights_h.py from an NNoM weights.h): the GPU's
 * nnom_model_create() + model_compile() (weights.h:138-161, nnom.c:758-900). Accepted: any chain
 * Input -> {Conv2D valid|same [+ReLU] | DW_Conv2D valid|same [+ReLU] (depth multiplier 1, even channel count) | MaxPool valid|same |
 * AvgPool valid|same | Dense [+ReLU] | Flatten | Softmax (last)}* -> Output whose
 * activations fit 2 x 32 KB. The shipped kws_conv graph (and any retrained model of that shape) runs on the matrix
 * cores; every other graph runs on the general layer-by-layer kernel. EDISON_E_SIZE: malformed graph or one the
 * reference itself would reject; EDISON_E_NO_IMPL: a layer/shape the reference runs but this path does not.  */
int edison_model_load(edison_ctx *ctx, const char *ednn_path);
int edison_model_load_mem(edison_ctx *ctx, const void *blob, size_t blob_bytes);

/* ---- any NNoM graph: shapes come from the loaded model ---------------------------------------------------
 * edison_net_batch = model_run() (nnom.c:975-1040) + nnom_predict()'s first-maximum argmax (nnom_utils.c:258-305)
 * for n inputs; edison_net_layers = the outputs of every layer, as a layer callback installed with
 * model_set_callback() (nnom.c:1043) would see them.
 *   in      [n][in_h*in_w*in_c] int8, HWC                  logits  [n][n_out] int8: output of the layer before a final
 *   softmax [n][n_out] int8 (NULL if the graph has none)            Softmax, or of the last layer if there is none
 *   argmax  [n] int32 first maximum of the LAST layer's output      acts    [n][acts_bytes]: layer outputs back to back
 * The fixed-shape entry points below (edison_cnn_*, edison_kws_*, edison_stream_*) accept any loaded model that maps
 * 31x13x1 features to 10 softmax classes. */
typedef struct edison_net_info {
	int32_t in_h, in_w, in_c; /* Input(shape(h, w, c))                                                          */
	int32_t n_out;            /* elements of the last layer's output                                            */
	int32_t n_layers;         /* compute layers (Input/Output/Flatten are not counted)                          */
	int32_t acts_bytes;       /* bytes per input of edison_net_layers                                           */
	int32_t has_softmax;
	int32_t accelerated;      /* 1: the kws_conv graph, served by its specialised matrix-core kernel; 2: another graph,
	                           * served by the general matrix-core kernel; 0: layer-by-layer VALU kernel only      */
} edison_net_info;
typedef struct edison_net_layer_info_t {
	int32_t type;             /* 1 Conv2D, 2 MaxPool, 3 Dense, 4 Softmax, 5 DW_Conv2D, 6 AvgPool                 */
	int32_t out_h, out_w, out_c;
	int32_t acts_offset;      /* where this layer's output starts inside one input's acts record                */
	int32_t relu;
} edison_net_layer_info_t;
int edison_net_get_info(edison_ctx *ctx, edison_net_info *out);
int edison_net_layer_info(edison_ctx *ctx, int layer, edison_net_layer_info_t *out);
int edison_net_batch_dev(edison_ctx *ctx, const int8_t *in, int64_t n, int8_t *logits, int8_t *softmax, int32_t *argmax);
int edison_net_layers_dev(edison_ctx *ctx, const int8_t *in, int64_t n, int8_t *acts);
int edison_net_batch(edison_ctx *ctx, const int8_t *in, int64_t n, int8_t *logits, int8_t *softmax, int32_t *argmax);
int edison_net_layers(edison_ctx *ctx, const int8_t *in, int64_t n, int8_t *acts);
/* The loaded graph's OWN kernel. NNoM fixes shapes, buffers and per-layer kernels once, in model_compile()
 * (nnom.c:758-900); edison_net_specialize() goes one step further and compiles the general matrix-core kernel's source with
 * this graph's plan as constants (0.8-1.8 s with the installed hipcc as a child process -- $EDISON_HIPCC, else $ROCM_PATH/bin/hipcc,
 * else /opt/rocm/bin/hipcc, never $PATH -- or hipRTC in this process). Code objects are cached on disk: $EDISON_JIT_CACHE, else
 * $XDG_CACHE_HOME/edison_amd, else $HOME/.cache/edison_amd ("off" disables the cache); the directory is created 0700 and used only
 * if it belongs to this user and nobody else can write it; an entry is keyed by graph, kernel text, compiler options and the
 * compiler's identity. From then on every entry point that runs the general kernel for this load (edison_net_batch*, and
 * edison_cnn_* / edison_kws_* / edison_stream_* for graphs other than kws_conv) runs the graph's own: same arithmetic,
 * bit-identical outputs, 1.7-3 x the general kernel on the fixture graphs (profiles/r03_net_own_kernel_all_graphs.txt).
 * EDISON_E_NO_IMPL: the graph has no matrix-core plan, or it holds a DW_Conv2D / AvgPool layer (such graphs are not specialised: their
 * VALU layers run inside the general kernel's one launch), or neither hipcc nor libhiprtc.so is installed -- the graph stays on the general
 * kernel. A model load by itself does NONE of this (no compiler, no file, no cached code object): it is this call, or the
 * caller's wish in the environment, read at every load -- EDISON_NET_SPECIALIZE=1: every load ends with this call (a failure
 * there never fails the load), =cache: a load takes the own kernel if an earlier call left it in the cache.
 * edison_net_specialized: 0 general kernel; own kernel: 1 compiled just now by a hipcc child process (the installed ROCm's
 * compiler, tried first), 2 taken from the cache, 3 compiled just now by hipRTC in this process (EDISON_JIT_COMPILER=hipcc|hiprtc
 * picks one).
 * edison_net_spec_source (host only, no context): the generated constants of an .ednn blob, for inspection / offline builds;
 * EDISON_E_SIZE with *need = bytes wanted when cap is too small. */
int edison_net_specialize(edison_ctx *ctx);
int edison_net_specialized(edison_ctx *ctx);
int edison_net_spec_source(const void *ednn_blob, size_t blob_bytes, char *out, size_t cap, size_t *need);
/* Host only, for tests and inspection: the plans of an .ednn blob as the matrix-core kernels get them (raw structs of
 * csrc/edison_internal.h: ed_net_plan_t, ed_mm_plan_t), the packed weight fragments and the accumulator seeds; any out pointer
 * may be NULL, *_need report the bytes wanted. edison_net_plan_layout(i): struct sizes / field offsets (see net_spec.c) so that a
 * reader outside C need not restate the layout -- tests/plan_emulator.py walks a plan in numpy exactly as the kernel does. */
int edison_net_plan_dump(const void *ednn_blob, size_t blob_bytes, void *plan_out, size_t plan_cap, void *mm_out, size_t mm_cap,
                         void *frag_out, size_t frag_cap, size_t *frag_need, void *seeds_out, size_t seeds_cap, size_t *seeds_need);
size_t edison_net_plan_layout(int which);

/* ---- device memory helpers (so a C caller needs nothing but this library) ---------------------------- */
int edison_dev_alloc(edison_ctx *ctx, size_t bytes, void **dptr);
int edison_dev_free(edison_ctx *ctx, void *dptr);
int edison_dev_upload(edison_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int edison_dev_download(edison_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);

/* ---- multi-GPU: one process (one context) per GPU, one RCCL all-gather of the logits ---------------------------
 * The reference has no counterpart (single MCU, UART host link: hostinterface.c:96-112). Utterances are
 * sharded contiguously over the ranks (edison_dist_shard_range); frames and utterances are independent, so the data
 * path has no collective; the only exchange is the all-gather of the per-class int8 logits (10 B per utterance) over
 * xGMI. Protocol: rank 0 calls edison_dist_unique_id and hands the 128 bytes to every rank by whatever means the host
 * program has (MPI, a file, a socket, torch.distributed); every rank then calls edison_dist_init on its context.
 * RCCL is bound at run time (librccl.so.1, or EDISON_RCCL_LIB); EDISON_E_NO_IMPL when it cannot be found. */
#define EDISON_DIST_ID_BYTES 128
int edison_dist_available(void); /* EDISON_OK when RCCL can be bound in this process (binds it, creates nothing) */
int edison_dist_unique_id(void *id128);
int edison_dist_init(edison_ctx *ctx, const void *id128, int rank, int world_size);
int edison_dist_info(const edison_ctx *ctx, int *rank, int *world_size);
int edison_dist_shutdown(edison_ctx *ctx); /* also done by edison_shutdown */
int edison_dist_shard_range(int64_t n_items, int rank, int world_size, int64_t *lo, int64_t *hi);
/* device pointers; every rank passes the same n_local_utt; rank r's rows land at all_logits + r * n_local_utt * 10.
 * Asynchronous on the context's stream. A context outside any communicator is a world of one (plain copy). */
int edison_dist_allgather_logits(edison_ctx *ctx, const int8_t *local_logits, int64_t n_local_utt, int8_t *all_logits);
/* a batch the world size does not divide: every rank passes the TOTAL n_total_utt, holds the shard
 * edison_dist_shard_range(n_total_utt, rank, world) in local_logits, and receives all n_total_utt rows in rank order
 * (shards padded to the largest one inside, still one ncclAllGather). The equal-shard call above must NOT be used with
 * different n_local_utt on different ranks (it cannot tell; ncclAllGather would mis-place or overrun the rows). */
int edison_dist_allgather_logits_total(edison_ctx *ctx, const int8_t *local_logits, int64_t n_total_utt, int8_t *all_logits);
/* edison_kws_batch_dev on this rank's shard followed by the all-gather: BASELINE config 4 in one call per rank */
int edison_kws_batch_sharded_dev(edison_ctx *ctx, const int16_t *audio, int64_t n_local_utt, int64_t utt_stride,
                                 int8_t *feat, int8_t *logits_local, int8_t *softmax, int32_t *argmax, int8_t *logits_all);
/* ... with shards cut by edison_dist_shard_range from n_total_utt (audio = this rank's shard only) */
int edison_kws_batch_sharded_total_dev(edison_ctx *ctx, const int16_t *audio, int64_t n_total_utt, int64_t utt_stride,
                                       int8_t *feat, int8_t *logits_local, int8_t *softmax, int32_t *argmax, int8_t *logits_all);

/* ---- the hot path, batched, device pointers ----------------------------------------------------------- */

/*
 * n_frames frames of 1024 int16 samples; frame i starts at audio + i*frame_step (samples; 1024 = the
 * reference's hop, 512 = 50 % overlap). Writes the first n_coef (1..32) coefficients of every frame:
 *   mfcc  [n_frames][n_coef] fp32            (may be NULL)
 *   feat  [n_frames][n_coef] int8 net input  (may be NULL) = round_half_even(clip(mfcc*feat_scale,-128,127)),
 *         the reference's np.clip(x*scale,-128,127).round().astype(int8) (kws_nnom.py:359-361)
 * Replaces the per-frame loops mfcc_utils.py:160-197 (A) and :287-322 (B).
 */
int edison_mfcc_batch_dev(edison_ctx *ctx, const int16_t *audio, int64_t n_frames, int64_t frame_step,
                          int variant, int n_coef, float *mfcc, int8_t *feat, float feat_scale);

/*
 * The same over n_rows independent rows of samples (the reference's batch_mfcc, mfcc_utils.py:75-131: one utterance per
 * row of data[n, samples]): row r starts at audio + r*row_stride (samples), its frame i at + i*frame_step; every row
 * yields frames_per_row frames. Outputs are [n_rows * frames_per_row][n_coef], row-major over (row, frame). ONE kernel
 * launch for the whole array (the kernel's grouped addressing), not one call per row.
 */
int edison_mfcc_rows_dev(edison_ctx *ctx, const int16_t *audio, int64_t n_rows, int64_t row_stride, int64_t frames_per_row,
                         int64_t frame_step, int variant, int n_coef, float *mfcc, int8_t *feat, float feat_scale);

/*
 * The same over n_batches INDEPENDENT batches -- batch b's samples at audio[b] (any address), its outputs at mfcc[b] / feat[b] (either
 * ARRAY may be NULL: that output is not written; an array that is given holds no NULL entries) -- of n_frames_each frames each, in ONE
 * launch per 16 batches (`audio`, `mfcc`, `feat` are HOST arrays of DEVICE pointers, read during the call). Rows of batch_mfcc that
 * do not share an allocation (mfcc_utils.py:75-131: rows are independent), or batches arriving from different producers. Why it
 * exists: a 65 536-frame launch idles ~15 % of its window (start-up, drain), a launch that runs on does not (0.41-0.42 of 8 TB/s
 * against 0.37-0.40), and keeping the NEXT launch in flight on a second HIP queue (below) recovers a quarter of it at best
 * (profiles/r05_mfcc_two_queues_notes.txt). Variants A and B (EDISON_E_NO_IMPL otherwise). Results are bit-identical to one
 * edison_mfcc_batch_dev call per batch.
 */
int edison_mfcc_batches_dev(edison_ctx *ctx, int n_batches, const int16_t *const *audio, int64_t n_frames_each, int64_t frame_step,
                            int variant, int n_coef, float *const *mfcc, int8_t *const *feat, float feat_scale);

/*
 * One call per batch with the NEXT launch already in flight: two library-owned HIP queues per context (created with different
 * priorities by default: HIP shares a pool of hardware queues among the streams of ONE priority, two such streams may serialise).
 *   edison_queues_fork(ctx)                  both queues wait for what the context's stream holds so far (the batches' producers)
 *   edison_mfcc_batch_queue_dev(ctx, q, ...) edison_mfcc_batch_dev on queue q = 0 / 1; batches in flight together must be independent
 *                                            (own input, own outputs); alternate q from call to call
 *   edison_queues_join(ctx)                  the context's stream waits for both queues; outputs are ordered as usual after it
 * Between fork and join the context's stream must not be changed (edison_set_stream) and only the queue call may be used. Results
 * are bit-identical to the plain calls. From a host that keeps both queues fed (a C host, ~5 us per call) a 65 536-frame batch
 * takes 45.7 us instead of 47.7 (+4.5 %; +1 ... +2.6 % on boards that sit at their power cap); a host that needs as long per call as the
 * GPU per batch gains nothing
 * (profiles/r05_mfcc_two_queues_notes.txt). A fork / join pair itself costs ~25-30 us of cross-queue signalling: keep MANY batches between
 * them -- at 65 536 frames per batch the two queues break even near 25 batches per fork (profiles/r05_two_queues_region_length.txt).
 * The list call above is the faster way whenever the batches are known together.
 * Which two streams: whether the next launch really backfills the CUs this one leaves depends on where runtime and driver put the two
 * streams' hardware queues, which HIP does not let a program choose -- of all pairs of nine streams in one process a third gained, a
 * third changed nothing, a third LOST 8-10 %. edison_queues_calibrate measures it: every pair of the context's five candidate streams
 * (three of the least, two of the greatest priority) and the serial sequence, interleaved, on the caller's own batch (`audio`: device
 * pointer, n_frames frames, read only), the winner once more against the serial sequence; the pair is kept only if it is at least 1 %
 * faster, otherwise both queue indices mean one stream and the queue calls ARE the serial sequence (never slower than it). ~0.17 s for a
 * 65 536-frame batch; call it once, after edison_init / edison_mfcc_configure, with a batch of the size that will be used. Outputs (each
 * may be NULL): microseconds per batch of the serial sequence and of what was kept, pair_kept = 10 * i + j (candidate indices) or 0.
 * A batch whose launch takes more than a millisecond keeps one queue without further measurement (its fixed cost is microseconds).
 * Without a calibration the queues are one stream of each priority.
 */
int edison_queues_calibrate(edison_ctx *ctx, const int16_t *audio, int64_t n_frames, int64_t frame_step, int variant, double *serial_us,
                            double *best_us, int *pair_kept);
int edison_queues_fork(edison_ctx *ctx);
int edison_queues_join(edison_ctx *ctx);
int edison_mfcc_batch_queue_dev(edison_ctx *ctx, int queue, const int16_t *audio, int64_t n_frames, int64_t frame_step, int variant,
                                int n_coef, float *mfcc, int8_t *feat, float feat_scale);

/*
 * Same, plus every intermediate the reference returns in its per-frame dict (mfcc_utils.py:161-197):
 *   fft   [n][513][2] fp32  un-normalised X[k], k=0..512 (re,im)      spec   [n][513] fp32 |X[k]| (A) or |X[k]|/1024/sqrt2 (B)
 *   mel   [n][32] fp32 mel_spectrogram                                 logmel [n][32] fp32 log_mel_spectrogram
 * Any of them may be NULL. This is the diagnostic path (parity tests, `main.py mfcc host`), not the fast one.
 */
int edison_mfcc_stages_dev(edison_ctx *ctx, const int16_t *audio, int64_t n_frames, int64_t frame_step,
                           int variant, float *fft, float *spec, float *mel, float *logmel, float *mfcc32);

/*
 * The generality path: variants A, B and TF for ANY geometry the reference's Python functions accept -- frame_len (4 .. 4096, also no power
 * of two: the reference calls numpy.fft.fft), mel_nbins (1 .. 256), sample rate, filterbank edges, mel_mtx_scale (mfcc_utils.py:134-199,
 * 255-323; every caller in the reference passes audio/config.py's 1024 / 32, which the entry points above serve). Float64 on the GPU
 * (direct DFT against a host-built table, dense mel product, ln, DCT-II with the variant's constants -- for B the literal 1/1024 and
 * 1/64 of mfcc_utils.py:297,318 whatever the frame length): the outputs are the reference's to ~1e-12. One workgroup per frame; not a
 * throughput path. Outputs, float64, each may be NULL: fft [n][F][2] (re, im), spec [n][F] with F = frame_len/2 (A) or frame_len (B) as
 * in the reference's per-frame dict; mel, logmel, mfcc [n][mel_nbins]; feat [n][n_coef] int8 = the net-input rounding of the first
 * n_coef coefficients (kws_nnom.py:359-361). EDISON_E_NO_IMPL outside the limits above or for other variants.
 * Variant TF (mfcc_utils.py:201-253 with fft_len == frame_len): the samples as float32 times tf.signal's periodic Hann window in float32,
 * then float64 -- rfft, |.|, the (frame_len/2+1)-bin mel matrix, ln(x + 1e-6), DCT-II / sqrt(2 mel_nbins); F = frame_len/2 + 1 (the caller cuts the
 * DC bin as the reference does); mel_mtx_scale is ignored. PARITY UNPINNED like the fast path's variant TF: no TensorFlow in this image.
 */
int edison_mfcc_generic_dev(edison_ctx *ctx, const int16_t *audio, int64_t n_frames, int frame_len, int64_t frame_step, int variant, int mel_nbins,
                            double sample_rate, double lower_edge_hertz, double upper_edge_hertz, double mel_mtx_scale, double *fft, double *spec,
                            double *mel, double *logmel, double *mfcc, int n_coef, int8_t *feat, float feat_scale);
int edison_mfcc_generic(edison_ctx *ctx, const int16_t *audio, int64_t n_frames, int frame_len, int64_t frame_step, int variant, int mel_nbins,
                        double sample_rate, double lower_edge_hertz, double upper_edge_hertz, double mel_mtx_scale, double *fft, double *spec,
                        double *mel, double *logmel, double *mfcc, int n_coef, int8_t *feat, float feat_scale);

/*
 * n_utt feature maps [31][13] int8 (403 B each, HWC, as aiRunInference's in_data) ->
 *   logits  [n_utt][10] int8 dense output      softmax [n_utt][10] int8 (= aiRunInference's out_data)
 *   argmax  [n_utt] int32 first maximum of the softmax output (nnom_predict, nnom_utils.c:275-284)
 * Each output may be NULL. Replaces model_run() (nnom.c:1037) over the graph of weights.h:138-161.
 */
int edison_cnn_batch_dev(edison_ctx *ctx, const int8_t *feat, int64_t n_utt, int8_t *logits, int8_t *softmax,
                         int32_t *argmax);

/* Per-layer activations of the CNN for parity tests: acts[n_utt][6496] = conv1+relu(3888) | pool1(1872) is
 * not kept separately on the fast path, so this diagnostic entry runs the unfused kernels:
 * conv1 3888 | pool1 1872 | conv2 2464 | pool2 1120 | conv3 960 | conv4 96 | dense 10 | softmax 10 = 10420 B. */
#define EDISON_CNN_ACT_BYTES 10420
int edison_cnn_layers_dev(edison_ctx *ctx, const int8_t *feat, int64_t n_utt, int8_t *acts);

/*
 * Full keyword spotting: utterance u = 31 frames of 1024 samples starting at audio + u*utt_stride (samples;
 * the reference's utterances are 32000 samples of which 31*1024 are used, audio/config.py:12,25,31).
 * Variant B features (the ones the net was trained on, kws_keras.py:47) -> int8 -> CNN.
 * feat [n_utt][403] (may be NULL) receives the int8 net input.
 */
int edison_kws_batch_dev(edison_ctx *ctx, const int16_t *audio, int64_t n_utt, int64_t utt_stride,
                         int8_t *feat, int8_t *logits, int8_t *softmax, int32_t *argmax);

/*
 * Keyword spotting for a graph trained at ANY MFCC geometry: the general audio -> class path. The fixed-shape entry points above and
 * below (edison_kws_batch*, the sharded and streaming calls) stay as they are: 1024-sample frames, 32 mel bins, 31x13x1 -> 10 graphs.
 * The geometry is what the reference's training flow reads from audio/config.py (kws_keras.py:443-468, kws_nnom.py:352-361):
 *   variant        EDISON_MFCC_A or EDISON_MFCC_B, B optionally | EDISON_MFCC_USE_LOG (TF and C: EDISON_E_NO_IMPL)
 *   frame_len      4 .. 4096 (EDISON_E_NO_IMPL outside); frame_step >= 1; n_samples >= frame_len per utterance
 *   frame_count    frames per utterance; 0: 1 + (n_samples - frame_len) / frame_step
 *   mel_nbins      1 .. 256 (EDISON_E_NO_IMPL outside), with the filterbank sample_rate, lower / upper_edge_hertz, mel_mtx_scale
 *   first_mfcc, num_mfcc  the coefficients handed to the network (first_mfcc + num_mfcc <= mel_nbins)
 *   net_input_scale       feature = int8(round half even(clip((float)mfcc * scale, -128, 127)))
 * Utterance u's frame f starts at audio + u * utt_stride + f * frame_step; its feature (f, c - first_mfcc) is element
 * u * in_n + f * num_mfcc + (c - first_mfcc) of the network input (the reference's flat reshape, whatever the graph's h, w, c).
 * frame_count * num_mfcc must equal the loaded graph's in_h * in_w * in_c (EDISON_E_SIZE otherwise). The MFCC runs in float64 like
 * the reference (FFT radix 2/3/4/5 for frame_len = 2^a 3^b 5^c, a direct DFT for other lengths), so the features, logits, softmax
 * and argmax are the reference host flow's; the graph runs on the network kernel edison_net_batch_dev picks for it. feat may be NULL
 * (context scratch); softmax may be NULL and is not written for a graph without Softmax. The filterbank, twiddle and DCT tables are
 * cached in the context for the last geometry: a call at that geometry allocates nothing and does not synchronise, a call at another
 * one synchronises the stream once. edison_mfcc_configure and the exact KWS mode neither affect this call nor are affected by it.
 */
typedef struct edison_kws_geom {
	int32_t variant;
	int32_t frame_len, frame_step, n_samples, frame_count;
	int32_t mel_nbins, first_mfcc, num_mfcc;
	double sample_rate, lower_edge_hertz, upper_edge_hertz, mel_mtx_scale, net_input_scale;
} edison_kws_geom;
/* audio/config.py's values: variant B without log, 1024 / 1024, 32000 samples, 32 mel bins 80 .. 7600 Hz, scale 128, first 13, 1.0 */
void edison_kws_geom_default(edison_kws_geom *g);
int edison_kws_geom_batch_dev(edison_ctx *ctx, const edison_kws_geom *g, const int16_t *audio, int64_t n_utt, int64_t utt_stride,
                              int8_t *feat, int8_t *logits, int8_t *softmax, int32_t *argmax);
/*
 * Float64 MFCC at the same geometry, without a model: the training-side features of a graph trained at g (the reference's load_data,
 * kws_keras.py:443-468, before its net_input_scale and clip). Frame addressing, coefficient window and arithmetic are those of
 * edison_kws_geom_batch*: mfcc [n_utt][frame_count][num_mfcc] (device pointer; edison_mfcc_geom_batch below takes host pointers)
 * receives the unscaled coefficient first_mfcc + c of frame f of utterance u at [u][f][c] -- the very float64 value that
 * edison_kws_geom_batch* and edison_stream_geom round to their int8 feature. net_input_scale is not used; first_mfcc = 0,
 * num_mfcc = mel_nbins gives whole MFCC rows. No model is needed. Errors: the geometry checks and codes of edison_kws_geom,
 * EDISON_E_ARGUMENT for more than 2^31 frames in one call or mfcc == NULL with n_utt > 0; n_utt == 0 does nothing. The call
 * shares the context's table cache with edison_kws_geom_batch* (same key): at the cached geometry it allocates nothing and does not
 * synchronise, at another one it synchronises the stream once. Tables owned by an edison_stream_geom are not touched.
 */
int edison_mfcc_geom_batch_dev(edison_ctx *ctx, const edison_kws_geom *g, const int16_t *audio, int64_t n_utt, int64_t utt_stride,
                               double *mfcc);

/*
 * Float32 X-CUBE-AI networks: the reference's default network type (firmware/src/ai/ai.h NET_TYPE_CUBE), imported from the generated
 * <net>.c + <net>_data.c by edison_amd/cube_import.py into an .ednf blob. Accepted: conv2d / conv2d_nl_pool (groups 1, any stride,
 * ReLU or none, max pool of 1, 2 or 4 elements with stride = size), dense, ReLU, a final softmax; activations HWC. An .ednf is version
 * 1 (records of int32[16], no pads) or version 2 (records of int32[24]: [16..19] the conv's pads top, left, bottom, right, [20..23]
 * the pool's): out = (in + before + after - k) / stride + 1, a tap outside the image is the operand +0.0f of the chain below, an
 * element of a pool window outside the conv's map takes no part in the max; a pad as large as its window on that axis is
 * EDISON_E_NO_IMPL. The blob's layer list,
 * shapes and weights are checked at load (EDISON_E_SIZE: malformed; EDISON_E_NO_IMPL: a network this path does not run, e.g. one whose
 * activations and largest layer do not fit the LDS). A load replaces the context's previous float network (synchronising the stream
 * once); a refused load leaves the previous network loaded and answering as before. The int8 NNoM model (edison_model_load) is
 * separate: a context may hold both.
 *   edison_fnet_batch  = the Cube aiRunInference for n inputs: in [n][in_h*in_w*in_c] float32 HWC -> logits [n][n_out] (the last
 *                        layer's output before softmax), probs [n][n_out] = exp(z - max) / sum, argmax [n] the first maximum of probs;
 *                        any output may be NULL
 *   edison_fnet_layers = every conv / dense layer's output (after bias, ReLU and pool), back to back: acts [n][acts_floats]
 * Arithmetic: each conv / dense output is the k-ordered f32 fmaf chain from +0.0f over k = (ky kw + kx) in_c + ci, then one f32 bias
 * add, fmaxf ReLU and fmaxf pool, subnormals kept: bit for bit what tests/fnet_exact.py computes.
 * EDISON_E_NO_MODEL when no float network is loaded.
 */
typedef struct edison_fnet_info_t {
	int32_t in_h, in_w, in_c; /* network input (rows = frames, columns = coefficients, channels)            */
	int32_t n_out;
	int32_t n_layers;         /* conv / dense layers (ReLU folded in, softmax not counted)                  */
	int32_t acts_floats;      /* floats per input of edison_fnet_layers                                    */
	int32_t batch;            /* utterances per workgroup of the kernel; 0: a layered network (below)      */
	int32_t lds_bytes;        /* LDS per workgroup                                                         */
} edison_fnet_info_t;
int edison_fnet_load(edison_ctx *ctx, const char *ednf_path);
int edison_fnet_load_mem(edison_ctx *ctx, const void *blob, size_t blob_bytes);
int edison_fnet_info(edison_ctx *ctx, edison_fnet_info_t *out);
/*
 * Networks the one-launch kernel cannot hold. edison_fnet_load* stage a whole record's weights and a tile of
 * utterances' activations in LDS and refuse a network that does not fit; the _ex loads take flags:
 *   EDISON_FNET_LARGE    such a network loads and runs on the layer road: one launch per conv / dense record and one softmax launch per
 *                        chunk of utterances, activations in a device workspace the context owns. The flag lifts only the two LDS
 *                        refusals and the 4096 bound on a record's in_c (a dense record's input is (1, 1, n)), up to what
 *                        kh kw in_c <= 65536 allows; every other check keeps its code and order. A network that fits gets the same plan
 *                        and kernel as without the flag.
 *   EDISON_FNET_LAYERED  the layer road even for a network that fits (A/B and tests).
 * Flags 0 is the plain call; any other bit is EDISON_E_ARGUMENT. The layer road computes the same k-ordered fmaf chains: its outputs are
 * bit for bit those of the one-launch kernel. edison_fnet_info reports batch = 0 for a layered network, and the layer kernel's LDS.
 * edison_fnet_batch*, edison_fnet_layers* and edison_kws_float_batch* take a layered network; the calibrator, the trainer, the float
 * stream and the float bank answer EDISON_E_NO_IMPL ("... layer road ...") at create.
 *   edison_fnet_set_workspace  the cap in bytes of the layer road's workspace (0: the default, 256 MiB). n utterances run in
 *                        ceil(n / chunk) chunks on the context's stream without synchronising between them, chunk = what the cap holds
 *                        of one utterance's activations (two buffers); the workspace grows on demand (synchronising once) up to the
 *                        cap. EDISON_E_NO_MEMORY, naming the cap, when one utterance of the loaded layered network exceeds it (the cap
 *                        stays as it was), and from a load under a cap one utterance of the new network exceeds (the previous network
 *                        stays).
 *   edison_fnet_profile_dev    a measurement aid (tools/bench_fnet_large.py): the layer road for n device inputs, no outputs kept;
 *                        ms [n_layers + 1] receives each record's and the softmax's kernel time in milliseconds between hipEvents,
 *                        summed over the chunks; it synchronises after every chunk. EDISON_E_NO_IMPL for a network that is not layered.
 */
#define EDISON_FNET_LARGE 1u   /* a network the one-launch kernel cannot hold runs layer by layer instead of being refused */
#define EDISON_FNET_LAYERED 2u /* take the layer road even when the network fits (A/B and tests) */
int edison_fnet_load_ex(edison_ctx *ctx, const char *ednf_path, unsigned flags);
int edison_fnet_load_mem_ex(edison_ctx *ctx, const void *blob, size_t blob_bytes, unsigned flags);
int edison_fnet_set_workspace(edison_ctx *ctx, size_t max_bytes);
int edison_fnet_profile_dev(edison_ctx *ctx, const float *in, int64_t n, float *ms);
int edison_fnet_batch_dev(edison_ctx *ctx, const float *in, int64_t n, float *logits, float *probs, int32_t *argmax);
int edison_fnet_layers_dev(edison_ctx *ctx, const float *in, int64_t n, float *acts);
int edison_fnet_batch(edison_ctx *ctx, const float *in, int64_t n, float *logits, float *probs, int32_t *argmax);
int edison_fnet_layers(edison_ctx *ctx, const float *in, int64_t n, float *acts);
/*
 * Audio -> class with the float network in one call (the Cube flow), utterances addressed as in edison_kws_geom_batch*:
 *   q15 = 0  the reference's host flow (kws_on_mcu.py:343-348): the float64 MFCC of edison_mfcc_geom_batch at g (any geometry) ->
 *            float32 -> x (float)net_input_scale -> clip to [clip_lo, clip_hi] (audio/config.py: -32768, 32767), never rounded
 *   q15 = 1  the firmware's flow (app.c:675-683): variant C int16 coefficients 0 .. num_mfcc - 1 -> (float), no scale, no clip; the
 *            shipped framing only (frame_len = frame_step = 1024, mel_nbins 32, first_mfcc 0; EDISON_E_NO_IMPL otherwise), on the
 *            context's configured filterbank (edison_mfcc_configure); clip_lo / clip_hi and net_input_scale are not used
 * feat [n_utt][frame_count * num_mfcc] float32 receives the network input (may be NULL: context scratch); logits / probs / argmax as
 * edison_fnet_batch. frame_count * num_mfcc must equal the float network's input size (EDISON_E_SIZE otherwise); EDISON_E_NO_MODEL
 * without a float network. Errors of the geometry as edison_kws_geom.
 */
int edison_kws_float_batch_dev(edison_ctx *ctx, const edison_kws_geom *g, int q15, float clip_lo, float clip_hi, const int16_t *audio,
                               int64_t n_utt, int64_t utt_stride, float *feat, float *logits, float *probs, int32_t *argmax);
int edison_kws_float_batch(edison_ctx *ctx, const edison_kws_geom *g, int q15, float clip_lo, float clip_hi, const int16_t *audio,
                           int64_t n_utt, int64_t utt_stride, float *feat, float *logits, float *probs, int32_t *argmax);

/*
 * Calibrating the loaded float network for quantisation to an int8 NNoM graph (the rule that turns the statistic
 * into formats and shifts is edison_amd/quantize.py). A calibrator is bound to the float network loaded when it is created and
 * accumulates, over every utterance added, one statistic for the network input (index 0) and one per conv / dense layer (index i =
 * layer i - 1), n_stats = n_layers + 1 in all:
 *   absmax  the largest bit pattern of fabsf(v) as uint32: v runs over the in_n floats of each input, or over acc + bias in f32 of a
 *           layer -- edison_fnet_batch's value before ReLU and before the pool, at the positions the network uses (those a truncating
 *           pool drops are not computed). An Inf or NaN anywhere gives a pattern >= 0x7f800000.
 *   hist    [256] uint64: how many v have biased exponent field (bits >> 23) & 0xff
 *   count   uint64: how many v
 * All counting is in integer atomics: the result does not depend on launch shape, on arrival order or on how the data set is split
 * into adds, and equals tests/fcal_ref.py's bit for bit.
 *   edison_fcal_add_dev  one kernel launch on the context's stream: it follows a feature stage on that stream with no synchronisation
 *   edison_fcal_add      the host form: stages its array and synchronises
 *   edison_fcal_result   synchronises and copies out absmax [n_stats], hist [n_stats][256], count [n_stats]; each may be NULL; the
 *                        counters go on
 *   edison_fcal_reset    zeroes the counters, stream-ordered
 * EDISON_E_NO_MODEL: no float network loaded at create; or, from every call but destroy, another float network was loaded since
 * (create a new calibrator). EDISON_E_NO_IMPL at create: the network fills the LDS so far that the statistic's 1028 bytes do not fit
 * beside one utterance. The calibrator runs the network at its own batch (edison_fcal_info), at most the network's.
 */
typedef struct edison_fcal edison_fcal;
typedef struct edison_fcal_info_t {
	int32_t n_stats;   /* n_layers + 1 */
	int32_t in_n;      /* floats per input */
	int32_t batch;     /* utterances per workgroup of the calibration kernel */
	int32_t lds_bytes; /* LDS per workgroup */
} edison_fcal_info_t;
int edison_fcal_create(edison_ctx *ctx, edison_fcal **out);
void edison_fcal_destroy(edison_fcal *c);
int edison_fcal_info(edison_fcal *c, edison_fcal_info_t *out);
int edison_fcal_reset(edison_fcal *c);
int edison_fcal_add_dev(edison_fcal *c, const float *in, int64_t n);
int edison_fcal_add(edison_fcal *c, const float *in, int64_t n);
int edison_fcal_result(edison_fcal *c, uint32_t *absmax, uint64_t *hist, uint64_t *count);

/*
 * Training the loaded float network (the epochs, callbacks and the model dict are edison_amd/train.py). A trainer is
 * bound to the float network loaded when it is created and updates that network's device weights in place: after a step the next
 * edison_fnet_batch, stream push or calibration on the context runs the new weights.
 *   edison_ftrain_create    a trainer for networks whose records have no conv or pool pad: a padded record is EDISON_E_NO_IMPL
 *   edison_ftrain_create_ex the same with flags: EDISON_FTRAIN_PADDED also takes networks with 'same' convs and pools (DESIGN.md section
 *                           14b), every network edison_fnet_load* loads; on a network without pads it makes edison_ftrain_create's
 *                           trainer exactly. flags = 0 is edison_ftrain_create; any other bit is EDISON_E_ARGUMENT. Use this call with
 *                           the flag unless a caller relies on the refusal.
 *   edison_ftrain_grad_dev  n inputs [n][in_n] and int32 labels [n] in device memory -> loss [n] (log sum exp(z) - z[y] per row) and
 *                           argmax [n] (edison_fnet_batch's), each NULL for not written, and, kept in the trainer, the logits [n][n_out]
 *                           (edison_fnet_batch's bit for bit) and the gradient of the batch loss (1 / n) sum loss with respect to every
 *                           weight and bias, in the packed layout below. Two launches on the context's stream, no synchronisation. A
 *                           label outside [0, n_out) contributes nothing (loss 0) and is counted (edison_ftrain_info). The same call
 *                           repeated gives the same bits. The weights are not changed.
 *   edison_ftrain_grad      the host form: stages its arrays and synchronises; a label outside [0, n_out) is EDISON_E_ARGUMENT before
 *                           any launch
 *   edison_ftrain_grad_get / _logits_get  synchronise and copy out the last call's gradient [w_floats] / logits [n][n_out]
 *   edison_ftrain_step      one optimiser step with the last gradient at learning rate lr, one launch. Adam as Keras states it, t from 1:
 *                           m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g g, w -= lr sqrt(1 - b2^t) / (1 - b1^t) m / (sqrt(v) + eps); the
 *                           scalar factor is computed in double. Or, kind EDISON_FTRAIN_SGD, w -= lr g.
 *   edison_ftrain_set_opt   kind and Adam's constants (at create: Adam, 0.9, 0.999, 1e-7); edison_ftrain_reset zeroes m, v, t and the
 *                           counter of ignored rows. Kind EDISON_FTRAIN_ADADELTA: b1 carries rho in [0, 1), b2 is ignored, eps > 0
 *                           (Keras's 'adadelta' is remembered as rho 0.95, eps 1e-7 at lr 1.0: unpinned); its step, a kernel of its own
 *                           on the two moment arrays, is a = rho a + (1 - rho) g g, u = g sqrt(d + eps) / sqrt(a + eps), w -= lr u,
 *                           d = rho d + (1 - rho) u u (Keras's and torch.optim.Adadelta's). A refused setting leaves the previous one.
 *   edison_ftrain_weights_get / _set  copy the packed weights [w_floats] out / in (synchronising)
 * Dropout, off at create:
 *   edison_ftrain_set_dropout  rate [n_records] in [0, 1) behind each conv / dense record's output (n_records = n_layers; the last
 *                           record's is 0: its output is the logits) and before_pool [n_records] (NULL: all 0): 1 puts the mask between
 *                           ReLU and the pool (Keras's Conv -> Dropout -> MaxPool), 0 behind the pool; with no pool they coincide.
 *                           All rates 0 turns dropout off. Sets the call counter to 0. Anything else is EDISON_E_ARGUMENT and leaves
 *                           the previous setting. Synchronises.
 *                           Whether element e of record l is kept for row u of a call is a pure function of (seed, call counter, u,
 *                           l, e) -- Philox4x32-10 keys per (row, record), two MurmurHash3 finalisers per element, csrc/fnet_dropout.h
 *                           -- and does not depend on the tile, the grid or the batch the trainer runs at. A kept value is multiplied
 *                           by (float)(1 / (1 - rate)), a dropped one is +0.0f. The masks are this library's, not TensorFlow's.
 *   edison_ftrain_set_dropout_call  position the call counter (< 2^60): resuming, or repeating a call
 *   edison_ftrain_dropout_get  read the setting back: rate and before_pool [n_layers], seed, counter (each NULL for not wanted)
 *   edison_ftrain_grad_dev_ex / edison_ftrain_grad_ex  the gradient calls with flags. EDISON_FTRAIN_EVAL: no dropout, the counter not
 *                           advanced; the outputs are bit for bit those of a trainer on which dropout was never set (validation).
 *                           flags = 0 is the plain call; any other bit is EDISON_E_ARGUMENT.
 * With dropout set, edison_ftrain_grad_dev / edison_ftrain_grad (and flags 0) are training calls: they apply the mask of the current
 * counter (n < 2^32 rows), then advance it by one; the logits and the loss they give are those of the masked network. Repeating a
 * call at the same counter gives the same bits. edison_ftrain_reset also sets the counter to 0. With dropout never set nothing changes.
 * The packed layout is the .ednf blob's and the kernels': per conv / dense record, at float offset w_at, B[k_pad][n_pad] with
 * k = (ky kw + kx) in_c + ci, then bias[n_pad] (edison_ftrain_layout; K = the real k rows). Padding k rows and padding channels of the
 * gradient are exactly +0.0f whatever the blob holds there, so a step leaves the weights' padding as it was.
 * EDISON_E_NO_MODEL: no float network loaded at create; or, from every call but destroy, another float network was loaded since (create
 * a new trainer). EDISON_E_NO_IMPL at create, the message naming the cause: a record with a pad (without EDISON_FTRAIN_PADDED), or a
 * training workgroup (the network at batch 1 beside one utterance's dY) that does not fit the LDS.
 */
#define EDISON_FTRAIN_ADAM 0
#define EDISON_FTRAIN_SGD 1
#define EDISON_FTRAIN_ADADELTA 2
#define EDISON_FTRAIN_PADDED 1u
#define EDISON_FTRAIN_EVAL 1u /* edison_ftrain_grad_dev_ex / edison_ftrain_grad_ex */
typedef struct edison_ftrain edison_ftrain;
typedef struct edison_ftrain_info_t {
	int32_t n_layers;  /* conv / dense records */
	int32_t in_n;      /* floats per input */
	int32_t n_out;     /* logits */
	int32_t batch;     /* utterances per workgroup tile of the gradient kernel */
	int32_t lds_bytes; /* LDS per workgroup */
	int32_t grid;      /* workgroups of the gradient kernel, at most: one gradient slab each */
	int64_t w_floats;  /* the packed weight array */
	int64_t steps;     /* optimiser steps since create / reset: Adam's t */
	int64_t ignored;   /* rows with a label outside [0, n_out) since create / reset (synchronises) */
} edison_ftrain_info_t;
int edison_ftrain_create(edison_ctx *ctx, edison_ftrain **out);
int edison_ftrain_create_ex(edison_ctx *ctx, uint32_t flags, edison_ftrain **out);
void edison_ftrain_destroy(edison_ftrain *t);
int edison_ftrain_info(edison_ftrain *t, edison_ftrain_info_t *out);
int edison_ftrain_layout(edison_ftrain *t, int record, int64_t *w_at, int32_t *K, int32_t *k_pad, int32_t *out_c, int32_t *n_pad);
int edison_ftrain_grad_dev(edison_ftrain *t, const float *in, const int32_t *labels, int64_t n, float *loss, int32_t *argmax);
int edison_ftrain_grad(edison_ftrain *t, const float *in, const int32_t *labels, int64_t n, float *loss, int32_t *argmax);
int edison_ftrain_grad_get(edison_ftrain *t, float *packed);
int edison_ftrain_logits_get(edison_ftrain *t, float *logits);
int edison_ftrain_step(edison_ftrain *t, double lr);
int edison_ftrain_set_opt(edison_ftrain *t, int kind, double b1, double b2, double eps);
int edison_ftrain_weights_get(edison_ftrain *t, float *packed);
int edison_ftrain_weights_set(edison_ftrain *t, const float *packed);
int edison_ftrain_reset(edison_ftrain *t);
int edison_ftrain_set_dropout(edison_ftrain *t, const double *rate, const uint8_t *before_pool, int n_records, uint64_t seed);
int edison_ftrain_set_dropout_call(edison_ftrain *t, uint64_t call);
int edison_ftrain_dropout_get(edison_ftrain *t, double *rate, uint8_t *before_pool, uint64_t *seed, uint64_t *call);
int edison_ftrain_grad_dev_ex(edison_ftrain *t, const float *in, const int32_t *labels, int64_t n, float *loss, int32_t *argmax, uint32_t flags);
int edison_ftrain_grad_ex(edison_ftrain *t, const float *in, const int32_t *labels, int64_t n, float *loss, int32_t *argmax, uint32_t flags);
/*
 * BatchNorm in the trainer: conv + bias = z -> BatchNorm -> ReLU -> dropout -> max pool, as the reference trains
 * kws_conv. Batch statistics are taken over every row of a training call and the whole conv map, the positions a floor-mode pool drops
 * included; mean and the population variance from centred values; y = gamma (z - mean) / sqrt(var + eps) + beta.
 *   edison_ftrain_set_batchnorm  has_bn [n_records = n_layers]: which records normalise (never the last; no record of the network may
 *                           have a pad: EDISON_E_NO_IMPL). momentum in [0, 1) and eps > 0 (Keras: 0.99, 1e-3); max_rows: the most rows
 *                           a training call may have (<= 0: 1024), the trainer's stores are sized for it; flags:
 *                           EDISON_FTRAIN_BN_UNBIASED moves the moving variance by var N / (N - 1) (torch's rule) instead of the
 *                           population variance. Starts at gamma 1, beta 0, moving mean 0, moving variance 1. From here on the trainer
 *                           trains a master copy of the weights with gamma and beta, and after every step, edison_ftrain_bn_set and
 *                           edison_ftrain_weights_set folds them into the loaded network's device buffer (W s, (b - mean) s + beta,
 *                           s = gamma / sqrt(var + eps) of the moving statistics), which every other entry point runs.
 *                           edison_ftrain_weights_get / _set are the master weights, edison_ftrain_folded_get the folded ones. An
 *                           EDISON_FTRAIN_EVAL call runs the folded network, moves no statistic, and leaves no gradient:
 *                           edison_ftrain_grad_get and edison_ftrain_step are EDISON_E_ARGUMENT until the next training call. A
 *                           second call on one trainer is EDISON_E_ARGUMENT. A BatchNorm record's bias gradient is +0.0f.
 *   edison_ftrain_batchnorm_get  read the setting back (each NULL for not wanted); batch: utterances per tile of a training call
 *   edison_ftrain_bn_get / _set  gamma, beta, moving mean and variance [out_c] of a BatchNorm record (NULL: not wanted / unchanged);
 *                           _set refolds; a variance <= -eps is EDISON_E_ARGUMENT
 *   edison_ftrain_bn_batch_get   the last training call's batch mean and variance [out_c]
 *   edison_ftrain_bn_grad_get    the last training call's dgamma, dbeta [out_c]
 */
#define EDISON_FTRAIN_BN_UNBIASED 1u
int edison_ftrain_set_batchnorm(edison_ftrain *t, const uint8_t *has_bn, int n_records, double momentum, double eps, int64_t max_rows, uint32_t flags);
int edison_ftrain_batchnorm_get(edison_ftrain *t, uint8_t *has_bn, double *momentum, double *eps, int64_t *max_rows, uint32_t *flags, int32_t *batch);
int edison_ftrain_bn_get(edison_ftrain *t, int record, float *gamma, float *beta, float *mean, float *var);
int edison_ftrain_bn_set(edison_ftrain *t, int record, const float *gamma, const float *beta, const float *mean, const float *var);
int edison_ftrain_bn_batch_get(edison_ftrain *t, int record, float *mean, float *var);
int edison_ftrain_bn_grad_get(edison_ftrain *t, int record, float *dgamma, float *dbeta);
int edison_ftrain_folded_get(edison_ftrain *t, float *packed);
/*
 * Training from a data set that lives on the device: whole epochs with one synchronisation each.
 *   edison_ftrain_data_create / _destroy  a store of rows [n][in_n] float32 and labels [n] int32 in device memory. It belongs to the
 *                           context, not to a trainer: it outlives trainers and network loads. Destroy it before edison_shutdown.
 *   edison_ftrain_data_set  host arrays, uploaded once; replaces the contents, regrows when needed. A negative label is
 *                           EDISON_E_ARGUMENT naming the row; labels are checked against the network's n_out where it is known, at
 *                           the epoch call. edison_ftrain_data_set_dev takes device pointers (it reads the labels back, synchronising).
 *   edison_ftrain_data_audio  host int16 audio, n_utt utterances utt_stride samples apart, uploaded `chunk` utterances at a time; each
 *                           chunk's features are written straight into the store by the feature launches of edison_kws_float_batch_dev
 *                           (g, q15, clip_lo, clip_hi as there; no network need be loaded): the rows are bit for bit that call's feat.
 *                           frame_count x num_mfcc != in_n is EDISON_E_SIZE; the geometry's errors are edison_kws_geom's.
 *   edison_ftrain_data_info / _get  n and in_n / copy the rows and labels back (each NULL for not wanted)
 *   edison_ftrain_epoch     one epoch over rows order[0 .. n_order) of d (any values in [0, n), repeats allowed), in batches of `batch`
 *                           rows, the last one short: one launch gathers the rows and labels in that order into the trainer's epoch
 *                           store, then per batch edison_ftrain_grad_dev_ex on its slice and edison_ftrain_step(lr), in stream order
 *                           with nothing between them, then one launch sums the per-row losses (in double, in an order n alone fixes,
 *                           no atomics: the same call gives the same bits) and counts the rows whose argmax is their label; one copy
 *                           back, one synchronisation. max_steps >= 0 ends the epoch after that many batches (< 0: no limit). Dropout's
 *                           counter and Adam's t advance as the same grad / step calls advance them. Before any launch: an order index
 *                           outside [0, n), a label of such a row >= n_out, batch < 1, or with BatchNorm batch > max_rows, are
 *                           EDISON_E_ARGUMENT; a data set of another in_n is EDISON_E_SIZE. n_order = 0 is zero steps and a zero result.
 *   edison_ftrain_data_eval the whole store through EDISON_FTRAIN_EVAL calls of 4096 rows, then the same reduction: no weight, statistic
 *                           or counter changes (with BatchNorm the next step needs a training call first, as after any EVAL call)
 *   edison_ftrain_epoch_rows  the per-row loss and argmax of the last epoch or eval call, in the order the rows were run (*n: how many)
 */
typedef struct edison_ftrain_data edison_ftrain_data;
typedef struct edison_ftrain_epoch_t {
	double loss_sum; /* sum of the per-row losses of the rows run */
	int64_t hits;    /* rows whose argmax equals their label      */
	int64_t seen;    /* rows run                                   */
	int64_t steps;   /* optimiser steps taken (an eval call: 0)    */
} edison_ftrain_epoch_t;
int edison_ftrain_data_create(edison_ctx *ctx, int32_t in_n, edison_ftrain_data **out);
void edison_ftrain_data_destroy(edison_ftrain_data *d);
int edison_ftrain_data_info(edison_ftrain_data *d, int64_t *n, int32_t *in_n);
int edison_ftrain_data_set(edison_ftrain_data *d, const float *x, const int32_t *y, int64_t n);
int edison_ftrain_data_set_dev(edison_ftrain_data *d, const float *x, const int32_t *y, int64_t n);
int edison_ftrain_data_get(edison_ftrain_data *d, float *x, int32_t *y);
int edison_ftrain_data_audio(edison_ftrain_data *d, const edison_kws_geom *g, int q15, float clip_lo, float clip_hi, const int16_t *audio, int64_t n_utt,
                             int64_t utt_stride, const int32_t *labels, int64_t chunk);
int edison_ftrain_epoch(edison_ftrain *t, edison_ftrain_data *d, const int32_t *order, int64_t n_order, int64_t batch, double lr, int64_t max_steps,
                        edison_ftrain_epoch_t *out);
int edison_ftrain_data_eval(edison_ftrain *t, edison_ftrain_data *d, edison_ftrain_epoch_t *out);
int edison_ftrain_epoch_rows(edison_ftrain *t, float *loss, int32_t *argmax, int64_t *n);

/*
 * Exact KWS mode (off by default; EDISON_KWS_EXACT=1 in the environment at edison_init turns it on for that context).
 * While it is on, every variant-B KWS call of the context -- edison_kws_batch, edison_kws_batch_dev and the sharded entry points --
 * aims at features, logits and argmax identical to the host flow's float64 arithmetic (mfcc_mcu, then float32 * scale, clip,
 * round half to even: kws_nnom.py:354-361) instead of the fp32 kernel's, which lands one int8 step off where a coefficient lies
 * within its rounding error of x.5. On ctx's stream, asynchronously, the call runs: the fp32 MFCC kernel, which also lists every
 * frame with an in-range feature within delta = K 2^-24 rms(frame) of x.5; a float64 kernel that recomputes the listed frames
 * (FFT, mel, DCT as the host flow) and overwrites their features; the CNN. Variant C (edison_kws_batch_q15*) and the continuous
 * streams are not affected.
 * Limits of the guarantee:
 *   - K is calibrated on the fp32 kernel's measured error with a margin, not proven: a frame whose fp32 error
 *     exceeds the bound would keep the fp32 feature.
 *   - the float64 recompute differs from numpy's pocketfft at about 1e-13 relative; that changes a feature only if float32(v64)
 *     falls on the other side of a float32 rounding boundary lying exactly at an x.5.
 * edison_kws_exact_stats covers the last exact call on the context: frames listed for the recompute and frames computed
 * (31 per utterance). It synchronises ctx's stream; both are 0 before the first exact call.
 */
int edison_kws_set_exact(edison_ctx *ctx, int on);
int edison_kws_get_exact(const edison_ctx *ctx, int *on);
int edison_kws_exact_stats(edison_ctx *ctx, int64_t *frames_flagged, int64_t *frames_total);

/*
 * Variant C with its native types: what the firmware keeps in bufDctInline / sends with audioDumpToHost
 * (audioprocessing.c:221-231). mfcc [n_frames][n_coef] int16; feat [n_frames][n_coef] int8 = mfccToNetInput's NNoM
 * branch (C division by NNOM_INPUT_SCALE = 1, clip to [-128,127], app.c:686-694). Stage dumps, all int16:
 *   fft [n][513][2] X[k] (re,im), k = 0..512, natural order     spec [n][513] bufSpect     mel [n][32] bufMelSpect
 * EDISON_E_NO_IMPL when the configured filterbank cannot be expressed as the firmware's compact tables.
 */
int edison_mfcc_q15_batch_dev(edison_ctx *ctx, const int16_t *audio, int64_t n_frames, int64_t frame_step, int n_coef,
                              int16_t *mfcc, int8_t *feat);
int edison_mfcc_q15_stages_dev(edison_ctx *ctx, const int16_t *audio, int64_t n_frames, int64_t frame_step,
                               int16_t *fft, int16_t *spec, int16_t *mel, int16_t *mfcc32);
/* edison_kws_batch_dev with the firmware's own features: variant C -> NNoM clip -> CNN, i.e. what the board
 * answers for the same samples (appHifMfccAndInference, app.c:167-221). */
int edison_kws_batch_q15_dev(edison_ctx *ctx, const int16_t *audio, int64_t n_utt, int64_t utt_stride, int8_t *feat,
                             int8_t *logits, int8_t *softmax, int32_t *argmax);

/* ---- the same with HOST pointers (upload, run, download, synchronise) -------------------------------- */
int edison_mfcc_q15_batch(edison_ctx *ctx, const int16_t *audio, int64_t n_frames, int64_t frame_step, int n_coef,
                          int16_t *mfcc, int8_t *feat);
int edison_mfcc_q15_stages(edison_ctx *ctx, const int16_t *audio, int64_t n_frames, int64_t frame_step, int16_t *fft,
                           int16_t *spec, int16_t *mel, int16_t *mfcc32);
int edison_kws_batch_q15(edison_ctx *ctx, const int16_t *audio, int64_t n_utt, int64_t utt_stride, int8_t *feat,
                         int8_t *logits, int8_t *softmax, int32_t *argmax);
int edison_mfcc_batch(edison_ctx *ctx, const int16_t *audio, int64_t n_frames, int64_t frame_step, int variant,
                      int n_coef, float *mfcc, int8_t *feat, float feat_scale);
int edison_mfcc_stages(edison_ctx *ctx, const int16_t *audio, int64_t n_frames, int64_t frame_step, int variant,
                       float *fft, float *spec, float *mel, float *logmel, float *mfcc32);
int edison_mfcc_rows(edison_ctx *ctx, const int16_t *audio, int64_t n_rows, int64_t row_stride, int64_t frames_per_row,
                     int64_t frame_step, int variant, int n_coef, float *mfcc, int8_t *feat, float feat_scale);
int edison_cnn_batch(edison_ctx *ctx, const int8_t *feat, int64_t n_utt, int8_t *logits, int8_t *softmax,
                     int32_t *argmax);
int edison_cnn_layers(edison_ctx *ctx, const int8_t *feat, int64_t n_utt, int8_t *acts);
int edison_kws_batch(edison_ctx *ctx, const int16_t *audio, int64_t n_utt, int64_t utt_stride, int8_t *feat,
                     int8_t *logits, int8_t *softmax, int32_t *argmax);
int edison_kws_geom_batch(edison_ctx *ctx, const edison_kws_geom *g, const int16_t *audio, int64_t n_utt, int64_t utt_stride,
                          int8_t *feat, int8_t *logits, int8_t *softmax, int32_t *argmax);
int edison_mfcc_geom_batch(edison_ctx *ctx, const edison_kws_geom *g, const int16_t *audio, int64_t n_utt, int64_t utt_stride,
                           double *mfcc);

/* ---- continuous-microphone mode ------------------------------------------------------------------------
 * The firmware's appMicMfccInfereContinuous / appAudioEvent loop (firmware/src/app.c:288-371, 635-663): every new
 * frame -> MFCC -> mfccToNetInputPush (31-row sliding window, app.c:706-719) -> inference. A push delivers
 * chunk_frames hops of `hop` NEW samples (hop 1024 = firmware cadence, 512 = 50 % overlap); the stream keeps the
 * last 1024-hop samples and the last 30 feature rows on the device and starts from silence / a zero window like
 * the firmware's static buffers. Output i of a push belongs to the window ending with its i-th new frame.
 * One push = one hipGraph launch (MFCC kernel, CNN kernel over sliding windows, history shift).            */
typedef struct edison_stream edison_stream;
int edison_stream_create(edison_ctx *ctx, int hop, int chunk_frames, edison_stream **out);
void edison_stream_destroy(edison_stream *s);
int edison_stream_reset(edison_stream *s);
int edison_stream_push_dev(edison_stream *s, const int16_t *samples /* device, chunk*hop */, int8_t *logits,
                           int8_t *softmax, int32_t *argmax /* device, may be NULL */);
/* n_frames <= chunk_frames new frames (n_frames * hop samples, outputs [n_frames][..]): the ragged last push of a recording that the
 * chunk does not divide (the firmware has no counterpart: its microphone never ends, app.c:288-371). Either launch mode (under
 * EDISON_STREAM_LAUNCH_GRAPH a short push runs the same kernels launched directly: the captured graph holds the chunk). The filtered
 * outputs of such a push: its n_frames entries. */
int edison_stream_push_n_dev(edison_stream *s, const int16_t *samples /* device, n_frames*hop */, int n_frames, int8_t *logits,
                             int8_t *softmax, int32_t *argmax /* device, may be NULL */);
int edison_stream_push(edison_stream *s, const int16_t *samples /* host */, int8_t *logits, int8_t *softmax,
                       int32_t *argmax);
int64_t edison_stream_frames_seen(const edison_stream *s);

/* Stream options beyond hop / chunk. mfcc_variant: EDISON_MFCC_B (host float model, default) or EDISON_MFCC_C (the
 * firmware's own Q15 features). filter = 1 adds the firmware's output post-processing to every inference of a push
 * (app.c:332-356): netOutFilt[c] = (float)(alpha*netOutFilt[c] + (1.0-alpha)*(float)netOutput[c]) in double
 * arithmetic, arm_max_f32 (first maximum) over the ten filtered outputs, "spotted" if that maximum exceeds
 * true_threshold. Defaults (edison_stream_default_opts): alpha 0.9 = NET_OUT_MOVING_AVG_ALPHA for NNoM (app.c:38),
 * threshold 0.5 = TRUE_THRESHOLD (app.c:34); the filter state starts at zero (app.c:299-300) and survives pushes. */
typedef struct edison_stream_opts
{
	int hop, chunk_frames;
	int mfcc_variant;
	int filter;
	double filter_alpha;
	double true_threshold;
	int launch_mode;  /* EDISON_STREAM_LAUNCH_DIRECT (default): the kernels of a push are launched one by one;
	                   * EDISON_STREAM_LAUNCH_GRAPH: every push replays the hipGraph captured at creation (device pushes: the
	                   * MFCC / CNN / filter / shift nodes; host pushes: upload + those + download). Same results; on this
	                   * platform the replay measures slower. Default from EDISON_STREAM_GRAPH=1. */
	int fsm;          /* 1 (needs filter = 1): the firmware's state machine (edisonFSM, app.c:727-928; edison_fsm below) as the last
	                   * stage of every push, on the GPU: the inferences of the push walk through it in order, the time between
	                   * two of them being the hop (dt = hop / 16 kHz, the cadence of appAudioEvent); state per inference and
	                   * the machine itself: edison_stream_fsm*. The machine starts in RESET and survives pushes. */
} edison_stream_opts;
#define EDISON_STREAM_LAUNCH_DIRECT 0
#define EDISON_STREAM_LAUNCH_GRAPH 1
void edison_stream_default_opts(edison_stream_opts *o);
int edison_stream_create_ex(edison_ctx *ctx, const edison_stream_opts *o, edison_stream **out);
/* Filtered outputs of the LAST push: filt [n][10] fp32 (netOutFilt after each inference), likely [n] int32 (predMaxIdx), spotted [n]
 * int32 (predMaxIdx where predMax > threshold, else -1); n = the frames of that push (chunk_frames, or the n_frames of
 * edison_stream_push_n_dev: exactly n entries are written). Each may be NULL. */
int edison_stream_filtered(edison_stream *s, float *filt /* host */, int32_t *likely, int32_t *spotted);
int edison_stream_filtered_dev(edison_stream *s, float *filt /* device */, int32_t *likely, int32_t *spotted);
/* The state machine of a stream created with fsm = 1, after the LAST push: *fsm = the machine (may be NULL), states [n] int32 =
 * the state it was in after each of the n inferences of that push (may be NULL; n as for edison_stream_filtered).
 * Before the first push after edison_stream_create* or edison_stream_reset these four answer chunk_frames entries of zeros and the
 * machine as edison_fsm_init leaves it. */
struct edison_fsm;
int edison_stream_fsm(edison_stream *s, struct edison_fsm *fsm /* host */, int32_t *states /* host */);
int edison_stream_fsm_dev(edison_stream *s, int32_t *states /* device */);

/* ---- continuous mode for a graph trained at ANY MFCC geometry ------------------------------------------
 * The continuous counterpart of edison_kws_geom_batch*: the firmware's continuous loop (app.c:288-371, 706-719) for the loaded graph at
 * the geometry g (variants A / B, float64 MFCC: the features, logits, softmax and argmax are the reference host flow's, at every
 * geometry, the shipped one included). The fixed-shape edison_stream_* above is a separate object and stays as it is.
 *   hop and window  the hop is g->frame_step: a push carries chunk_frames * frame_step new samples. The window is F = frame_count rows of
 *                   num_mfcc int8 features (as edison_kws_geom); F * num_mfcc must equal the graph's in_h * in_w * in_c.
 *   start state     T = max(0, frame_len - frame_step) samples of silence and F - 1 rows of int8 zeros (the firmware's static buffers).
 *   frames          with z = the recording behind T zeros, global frame k is the MFCC of z[k * frame_step .. k * frame_step + frame_len);
 *                   when frame_step > frame_len the rest of each hop is skipped.
 *   outputs         output i of a push is the graph on rows k - F + 1 .. k, oldest first (the firmware's order and the batch call's
 *                   flat reshape), k = the push's i-th new frame. For k >= F - 1 it is bit-identical to edison_kws_geom_batch on z at
 *                   offset (k - F + 1) * frame_step. logits / softmax [n][n_out] int8, argmax [n] int32, each may be NULL; softmax is
 *                   not written for a graph without Softmax.
 *   filter          (opts.filter) the firmware's post-processing (app.c:332-356) over the graph's n_out outputs: float32 state starting at
 *                   zero, state = (float)(alpha * state + (1 - alpha) * (float)x) with product and sum rounded separately in double,
 *                   first maximum, spotted if that maximum > true_threshold. x = the softmax output, or the last layer's output for a
 *                   graph without Softmax. n_out above 256 (one workgroup): EDISON_E_NO_IMPL.
 *   fsm             (opts.fsm, needs filter) edisonFSM behind the filter (as edison_stream_opts.fsm) with dt_us = floor(frame_step *
 *                   1e6 / sample_rate); only for a graph with 10 outputs, the keyword list its roles index (EDISON_E_NO_IMPL otherwise).
 * Errors of create: the geometry checks and codes of edison_kws_geom; EDISON_E_NO_MODEL without a model; EDISON_E_SIZE when F * num_mfcc
 * != in_n or chunk_frames * frame_step >= 2^30; EDISON_E_ARGUMENT for chunk_frames < 1, fsm without filter or alpha outside [0, 1].
 * A push after a model reload fails with EDISON_E_ARGUMENT (create a new stream).
 * A device push is asynchronous on the context's stream: it allocates nothing and does not synchronise (MFCC kernel on the sliding
 * sample buffer, the network over the n overlapping windows at an input stride of num_mfcc bytes, the filter, and -- only when the next
 * push would not fit -- the history shift). A host push stages through pinned memory on a private stream and synchronises it. Host and
 * device pushes may alternate: they share one history. The stream owns its own tables: edison_kws_geom_batch* at another geometry on
 * the same context neither frees them nor makes a push synchronise. */
typedef struct edison_stream_geom edison_stream_geom;
typedef struct edison_stream_geom_opts {
	int32_t chunk_frames;          /* new frames per push, >= 1 */
	int32_t filter;                /* 1: moving average, first maximum and threshold over the graph's n_out outputs */
	int32_t fsm;                   /* 1 (needs filter): edisonFSM behind the filter; only for a graph with 10 outputs */
	double filter_alpha, true_threshold;
} edison_stream_geom_opts;
/* chunk_frames 1, filter 0, fsm 0, alpha 0.9, threshold 0.5: the fixed stream's defaults */
void edison_stream_geom_default_opts(edison_stream_geom_opts *o);
int edison_stream_geom_create(edison_ctx *ctx, const edison_kws_geom *g, const edison_stream_geom_opts *o, edison_stream_geom **out);
void edison_stream_geom_destroy(edison_stream_geom *s);
int edison_stream_geom_reset(edison_stream_geom *s);
/* chunk_frames * frame_step new samples; outputs [chunk_frames][..] */
int edison_stream_geom_push(edison_stream_geom *s, const int16_t *samples /* host */, int8_t *logits, int8_t *softmax, int32_t *argmax);
int edison_stream_geom_push_dev(edison_stream_geom *s, const int16_t *samples /* device */, int8_t *logits, int8_t *softmax, int32_t *argmax);
/* 1 <= n_frames <= chunk_frames new frames (n_frames * frame_step samples, outputs [n_frames][..]): the ragged last push of a recording */
int edison_stream_geom_push_n_dev(edison_stream_geom *s, const int16_t *samples /* device */, int n_frames, int8_t *logits, int8_t *softmax,
                                  int32_t *argmax);
int64_t edison_stream_geom_frames_seen(const edison_stream_geom *s);
/* Filtered outputs of the LAST push (n = its frames): filt [n][n_out] fp32, likely [n], spotted [n] (-1 below the threshold); each
 * may be NULL. Host form synchronous, device form ordered on the context's stream. */
int edison_stream_geom_filtered(edison_stream_geom *s, float *filt, int32_t *likely, int32_t *spotted);
int edison_stream_geom_filtered_dev(edison_stream_geom *s, float *filt, int32_t *likely, int32_t *spotted);
/* The state machine after the LAST push (*fsm, host, may be NULL) and the state after each of its n inferences (states [n]) */
int edison_stream_geom_fsm(edison_stream_geom *s, struct edison_fsm *fsm, int32_t *states);
int edison_stream_geom_fsm_dev(edison_stream_geom *s, int32_t *states);

/* ---- a bank of continuous streams: one push advances many microphones through one graph ----------------------------------
 * n_mics independent continuous streams at ONE geometry on the loaded graph, advancing in lockstep: microphone m behaves exactly as an
 * edison_stream_geom of its own, created with the same geometry, options and model and fed microphone m's samples -- logits, softmax,
 * argmax, filtered outputs, likely, spotted, the state machine and frames_seen, byte for byte. One push carries n frames for every
 * microphone and costs a number of launches that does not depend on n_mics (one MFCC launch, n network launches, one filter launch).
 *   samples         [n_mics][n * frame_step] int16: each microphone's new samples contiguous, microphone after microphone.
 *   outputs         time-major: logits / softmax [n][n_mics][n_out] int8, argmax [n][n_mics] int32; filt [n][n_mics][n_out] fp32,
 *                   likely / spotted / states [n][n_mics] int32; the state machines fsm [n_mics]. For the usual n = 1 that is simply
 *                   [n_mics][..]. Each may be NULL; softmax is not written for a graph without Softmax.
 *   reset_mic       microphone `mic` alone back to a new stream's state (silent history, zero filter state, edisonFSM in RESET): from
 *                   the next push on it equals a freshly created stream; the other microphones do not notice. Ordered like a push: it
 *                   waits for device pushes still in flight and has taken effect when it returns. frames_seen is the bank's and stays.
 * Errors of create: those of edison_stream_geom_create, and EDISON_E_ARGUMENT for n_mics outside 1 .. 4096; EDISON_E_NO_MEMORY when the
 * buffers (n_mics times a stream's) cannot be allocated. A push after a model reload fails with EDISON_E_ARGUMENT; so does n_frames
 * outside 1 .. chunk_frames and a microphone index outside 0 .. n_mics - 1. NULL handles: EDISON_E_ARGUMENT. Messages name stream_bank.
 * Host and device pushes may alternate, as edison_stream_geom's; the getters copy the LAST push's outputs (n = its frames). */
typedef struct edison_stream_bank edison_stream_bank;
typedef struct edison_stream_bank_opts {
	int n_mics;                      /* microphones, 1 .. 4096 */
	edison_stream_geom_opts stream;  /* every microphone's options */
} edison_stream_bank_opts;
/* n_mics 1, stream = edison_stream_geom_default_opts */
void edison_stream_bank_default_opts(edison_stream_bank_opts *o);
int edison_stream_bank_create(edison_ctx *ctx, const edison_kws_geom *g, const edison_stream_bank_opts *o, edison_stream_bank **out);
void edison_stream_bank_destroy(edison_stream_bank *b);
int edison_stream_bank_reset(edison_stream_bank *b);
int edison_stream_bank_reset_mic(edison_stream_bank *b, int mic);
/* chunk_frames frames per microphone: samples [n_mics][chunk_frames * frame_step] */
int edison_stream_bank_push(edison_stream_bank *b, const int16_t *samples /* host */, int8_t *logits, int8_t *softmax, int32_t *argmax);
int edison_stream_bank_push_dev(edison_stream_bank *b, const int16_t *samples /* device */, int8_t *logits, int8_t *softmax, int32_t *argmax);
/* 1 <= n_frames <= chunk_frames frames per microphone: samples [n_mics][n_frames * frame_step], outputs [n_frames][n_mics][..] */
int edison_stream_bank_push_n_dev(edison_stream_bank *b, const int16_t *samples /* device */, int n_frames, int8_t *logits, int8_t *softmax,
                                  int32_t *argmax);
int edison_stream_bank_filtered(edison_stream_bank *b, float *filt, int32_t *likely, int32_t *spotted);
int edison_stream_bank_filtered_dev(edison_stream_bank *b, float *filt, int32_t *likely, int32_t *spotted);
/* the state machines after the LAST push (fsm [n_mics], may be NULL) and every microphone's state after each of its n inferences */
int edison_stream_bank_fsm(edison_stream_bank *b, struct edison_fsm *fsm /* host */, int32_t *states);
int edison_stream_bank_fsm_dev(edison_stream_bank *b, struct edison_fsm *fsm /* device */, int32_t *states);
/* frames pushed per microphone since create or reset */
int edison_stream_bank_frames_seen(edison_stream_bank *b, int64_t *out);

/* ---- a bank push may leave microphones out: their streams stay untouched --------------------------------------------------
 * A late or lost packet, a muted device, a recording that has ended: the push carries a mask, present [n_mics] uint8, nonzero = this
 * microphone's samples count, NULL = every microphone (then the call IS the push above). Push k carries the set P_k of present
 * microphones and n_k frames; microphone m behaves exactly as an edison_stream_geom of its own that was pushed only the pushes k with m
 * in P_k -- its rows of those pushes, its state machine and its frame count, byte for byte. For m outside P_k nothing of m changes:
 * sample history, feature rows, filter state, state machine, frame count. Its samples in the push buffer are ignored and may hold
 * anything (they must be readable). Its rows of the push's outputs hold a defined fill: zero bytes in logits, softmax and filt, -1 in
 * argmax, likely and spotted, the machine's unchanged state in states, the unchanged machine in fsm [m]. The bank-wide frames_seen
 * advances by n_k as before, also when nobody is present.
 *   present         host memory for the host push, device memory for the device push, which reads it on the context's stream: it
 *                   stays valid and unchanged until the push has run.
 *   frames_seen_mics  counts [n_mics] int64 (host): the frames each microphone was present for since create or reset. Synchronous and
 *                   ordered after pushes in flight, as reset_mic. reset zeroes the counts; reset_mic does not, as frames_seen.
 * A push with a mask costs one launch more than without, whatever n_mics, and the host push one upload of n_mics bytes; an absent
 * microphone still takes its share of the feature and network launches. Errors as the pushes above: EDISON_E_ARGUMENT for a NULL bank,
 * NULL samples or counts and for n_frames outside 1 .. chunk_frames. Messages name stream_bank. */
int edison_bank_push_present(edison_stream_bank *b, const int16_t *samples /* host */, const uint8_t *present /* host */, int8_t *logits,
                             int8_t *softmax, int32_t *argmax);
int edison_bank_push_present_n_dev(edison_stream_bank *b, const int16_t *samples /* device */, const uint8_t *present /* device */, int n_frames,
                                   int8_t *logits, int8_t *softmax, int32_t *argmax);
int edison_bank_frames_seen_mics(edison_stream_bank *b, int64_t *counts);

/* ---- continuous mode for the float32 X-CUBE-AI network ------------------------------------------------------------------
 * The continuous counterpart of edison_kws_float_batch*: the firmware's continuous loop for its default network type, NET_TYPE_CUBE
 * (app.c:288-371, 630-719), on the float network loaded on the context (edison_fnet_load). A separate object: edison_stream_geom_* and
 * edison_stream_* stay as they are.
 *   features      q15 = 0: the host flow of edison_kws_float_batch -- the float64 MFCC at any geometry that call accepts ->
 *                 (float)y * (float)net_input_scale -> clip to [clip_lo, clip_hi], never rounded. q15 = 1: the firmware flow --
 *                 variant-C int16 coefficients -> (float), the shipped framing only (frame_len = frame_step = 1024, mel_nbins 32,
 *                 first_mfcc 0), on the context's Q15 tables: exactly what edison_kws_float_batch(q15 = 1) does.
 *   hop and window  the hop is g->frame_step: a push carries chunk_frames * frame_step new samples. The window is F = frame_count rows of
 *                 num_mfcc float32 features; F * num_mfcc must equal the network's input size.
 *   start state   T = max(0, frame_len - frame_step) samples of silence and F - 1 rows of float zeros (the firmware's static netInput).
 *   frames        with z = the recording behind T zeros, global frame k is the MFCC of z[k * frame_step ..); when frame_step > frame_len
 *                 the rest of each hop is skipped.
 *   outputs       output i of a push is the network on rows k - F + 1 .. k, oldest first (the firmware's append order, not kws_live.py's
 *                 prepend), k = the push's i-th new frame. logits / probs [n][n_out] float32 and argmax [n] int32 (the first maximum of
 *                 probs), each may be NULL. For k >= F - 1 they are bit-identical to edison_kws_float_batch on z at offset
 *                 (k - F + 1) * frame_step.
 *   filter        (opts.filter) app.c:332-356 over the n_out probabilities p: float32 state starting at zero,
 *                 state = (float)(alpha * (double)state + (1 - alpha) * (double)p) with the product and the sum rounded separately;
 *                 then the first maximum, spotted if it is > true_threshold.
 *   fsm           (opts.fsm, needs filter) edisonFSM behind the filter with dt_us = floor(frame_step * 1e6 / sample_rate); only for a
 *                 network with 10 outputs.
 * Errors of create: EDISON_E_NO_MODEL without a float network; EDISON_E_SIZE when F * num_mfcc != its input size or chunk_frames *
 * frame_step >= 2^30; EDISON_E_NO_IMPL for q15 = 1 off the shipped framing (or without variant-C tables), a filter over more than 256
 * classes, or fsm on a network without 10 outputs; EDISON_E_ARGUMENT for chunk_frames < 1, fsm without filter, filter_alpha outside
 * [0, 1], clip_lo > clip_hi; the geometry checks and codes of edison_kws_float_batch otherwise. A push after edison_fnet_load has
 * replaced the network fails with EDISON_E_ARGUMENT (create a new stream).
 * A device push is asynchronous on the context's stream: it allocates nothing and does not synchronise. It enqueues one sample copy,
 * the feature kernel writing the new rows behind the history, the network over the n overlapping windows read in place (an input stride
 * of num_mfcc floats), the filter, and -- only when the next push would not fit -- the history shift. A host push stages through pinned
 * memory on a private stream: one upload, one download of one output block, one synchronise. Host and device pushes may alternate: they
 * share one history. The stream owns its own tables: batch calls at other geometries neither free them nor make a push synchronise. */
typedef struct edison_stream_float edison_stream_float;
typedef struct edison_stream_float_opts {
	int32_t chunk_frames;          /* new frames per push, >= 1 */
	int32_t q15;                   /* 0: host flow at any geometry; 1: the firmware's variant C, shipped framing */
	float clip_lo, clip_hi;        /* host flow: the network input's clip range */
	int32_t filter;                /* 1: moving average, first maximum and threshold over the network's n_out probabilities */
	int32_t fsm;                   /* 1 (needs filter): edisonFSM behind the filter; only for a network with 10 outputs */
	double filter_alpha, true_threshold;
} edison_stream_float_opts;
/* chunk_frames 1, q15 0, clip -32768 / 32767, filter 0, fsm 0, alpha 0.5 (the Cube build's NET_OUT_MOVING_AVG_ALPHA), threshold 0.5 */
void edison_stream_float_default_opts(edison_stream_float_opts *o);
int edison_stream_float_create(edison_ctx *ctx, const edison_kws_geom *g, const edison_stream_float_opts *o, edison_stream_float **out);
void edison_stream_float_destroy(edison_stream_float *s);
int edison_stream_float_reset(edison_stream_float *s);
/* chunk_frames * frame_step new samples; outputs [chunk_frames][..] */
int edison_stream_float_push(edison_stream_float *s, const int16_t *samples /* host */, float *logits, float *probs, int32_t *argmax);
int edison_stream_float_push_dev(edison_stream_float *s, const int16_t *samples /* device */, float *logits, float *probs, int32_t *argmax);
/* 1 <= n_frames <= chunk_frames new frames (n_frames * frame_step samples, outputs [n_frames][..]): the ragged last push of a recording */
int edison_stream_float_push_n_dev(edison_stream_float *s, const int16_t *samples /* device */, int n_frames, float *logits, float *probs,
                                   int32_t *argmax);
int64_t edison_stream_float_frames_seen(const edison_stream_float *s);
/* Filtered outputs of the LAST push (n = its frames): filt [n][n_out] fp32, likely [n], spotted [n] (-1 below the threshold); each
 * may be NULL. Host form synchronous, device form ordered on the context's stream. */
int edison_stream_float_filtered(edison_stream_float *s, float *filt, int32_t *likely, int32_t *spotted);
int edison_stream_float_filtered_dev(edison_stream_float *s, float *filt, int32_t *likely, int32_t *spotted);
/* The state machine after the LAST push (*fsm, host, may be NULL) and the state after each of its n inferences (states [n]) */
int edison_stream_float_fsm(edison_stream_float *s, struct edison_fsm *fsm, int32_t *states);
int edison_stream_float_fsm_dev(edison_stream_float *s, int32_t *states);

/* ---- a bank of continuous streams on the float32 X-CUBE-AI network: one push advances many microphones ----------------------
 * n_mics independent continuous streams at ONE geometry on the float network loaded on the context (edison_fnet_load), advancing in
 * lockstep: microphone m behaves exactly as an edison_stream_float of its own, created with the same geometry, options and network and
 * fed microphone m's samples -- logits, probs, argmax, filtered outputs, likely, spotted, the filter state, the state machine and
 * frames_seen, bit for bit. One push carries n frames for every microphone and costs a number of launches that depends neither on n_mics
 * nor on n: one feature launch over the n_mics * n frames (q15 = 1: plus one strided device copy), ONE network launch over the n * n_mics
 * windows, one filter launch.
 *   samples         [n_mics][n * frame_step] int16: each microphone's new samples contiguous, microphone after microphone.
 *   outputs         time-major: logits / probs [n][n_mics][n_out] float32, argmax [n][n_mics] int32; filt [n][n_mics][n_out] fp32,
 *                   likely / spotted / states [n][n_mics] int32; the state machines fsm [n_mics]. For the usual n = 1 that is simply
 *                   [n_mics][..]. Each may be NULL.
 *   reset_mic       microphone `mic` alone back to a new stream's state (silent history, float zero rows, zero filter state, edisonFSM in
 *                   RESET): from the next push on it equals a freshly created stream; the other microphones do not notice. Ordered like a
 *                   push: it waits for device pushes still in flight and has taken effect when it returns. frames_seen is the bank's and
 *                   stays.
 * Errors of create: those of edison_stream_float_create, EDISON_E_ARGUMENT for n_mics outside 1 .. 4096, EDISON_E_SIZE when n_mics *
 * chunk_frames >= 2^31; EDISON_E_NO_MEMORY when the buffers (n_mics times a stream's) cannot be allocated. A push after edison_fnet_load
 * has replaced the network fails with EDISON_E_ARGUMENT; so does n_frames outside 1 .. chunk_frames and a microphone index outside
 * 0 .. n_mics - 1. NULL handles: EDISON_E_ARGUMENT. Messages name float_bank. Host and device pushes may alternate, as
 * edison_stream_float's; the getters copy the LAST push's outputs (n = its frames). A bank of one microphone issues exactly
 * edison_stream_float's copies and kernels. */
typedef struct edison_float_bank edison_float_bank;
typedef struct edison_float_bank_opts {
	int32_t n_mics;                   /* microphones, 1 .. 4096 */
	edison_stream_float_opts stream;  /* every microphone's options */
} edison_float_bank_opts;
/* n_mics 1, stream = edison_stream_float_default_opts */
void edison_float_bank_default_opts(edison_float_bank_opts *o);
int edison_float_bank_create(edison_ctx *ctx, const edison_kws_geom *g, const edison_float_bank_opts *o, edison_float_bank **out);
void edison_float_bank_destroy(edison_float_bank *b);
int edison_float_bank_reset(edison_float_bank *b);
int edison_float_bank_reset_mic(edison_float_bank *b, int mic);
/* chunk_frames frames per microphone: samples [n_mics][chunk_frames * frame_step] */
int edison_float_bank_push(edison_float_bank *b, const int16_t *samples /* host */, float *logits, float *probs, int32_t *argmax);
int edison_float_bank_push_dev(edison_float_bank *b, const int16_t *samples /* device */, float *logits, float *probs, int32_t *argmax);
/* 1 <= n_frames <= chunk_frames frames per microphone: samples [n_mics][n_frames * frame_step], outputs [n_frames][n_mics][..] */
int edison_float_bank_push_n_dev(edison_float_bank *b, const int16_t *samples /* device */, int n_frames, float *logits, float *probs,
                                 int32_t *argmax);
int edison_float_bank_filtered(edison_float_bank *b, float *filt, int32_t *likely, int32_t *spotted);
int edison_float_bank_filtered_dev(edison_float_bank *b, float *filt, int32_t *likely, int32_t *spotted);
/* the state machines after the LAST push (fsm [n_mics], may be NULL) and every microphone's state after each of its n inferences */
int edison_float_bank_fsm(edison_float_bank *b, struct edison_fsm *fsm /* host */, int32_t *states);
int edison_float_bank_fsm_dev(edison_float_bank *b, struct edison_fsm *fsm /* device */, int32_t *states);
/* frames pushed per microphone since create or reset */
int edison_float_bank_frames_seen(edison_float_bank *b, int64_t *out);

/* A float bank push may leave microphones out, as edison_bank_push_present*: the same mask, the same defining property with an
 * edison_stream_float per microphone, the same fill (zero bytes in logits, probs and filt; -1 in argmax, likely and spotted; the
 * unchanged state and machine), the same counts and the same cost of one launch more. Messages name float_bank. */
int edison_fbank_push_present(edison_float_bank *b, const int16_t *samples /* host */, const uint8_t *present /* host */, float *logits,
                              float *probs, int32_t *argmax);
int edison_fbank_push_present_n_dev(edison_float_bank *b, const int16_t *samples /* device */, const uint8_t *present /* device */, int n_frames,
                                    float *logits, float *probs, int32_t *argmax);
int edison_fbank_frames_seen_mics(edison_float_bank *b, int64_t *counts);

/* ---- the firmware's home-automation state machine (edisonFSM, app.c:727-928), host side, without the LEDs -------
 * RESET -> IDLE -(wake word "edison" spotted)-> HOT -(a location spotted)-> LOC -(a value spotted)-> SET -> IDLE;
 * HOT and LOC fall back to IDLE after EDI_LOC_TIMEOUT = 5000 ms (app.c:48). Time advances by dt_us per call exactly
 * like the firmware's `hotTimeout += dt/1000` (integer milliseconds per call). One step per inference. */
#define EDISON_FSM_RESET 0
#define EDISON_FSM_IDLE 1
#define EDISON_FSM_HOT 2
#define EDISON_FSM_LOC 3
#define EDISON_FSM_SET 4
typedef struct edison_fsm
{
	int state;
	uint32_t hot_timeout_ms;
	int wake_idx;
	int loc_idx, val_idx;       /* keyword indices of the pending location / value */
	int last_loc, last_val;     /* the last executed command (keyword indices), -1 before the first */
	uint32_t commands;          /* how many "location value" commands were executed */
} edison_fsm;
void edison_fsm_init(edison_fsm *f);
/* pred_max / pred_idx: arm_max_f32 of the filtered outputs; returns the new state. */
int edison_fsm_step(edison_fsm *f, float pred_max, uint32_t pred_idx, uint32_t dt_us, double true_threshold);
/* The whole post-processing chain of the firmware (app.c:332-371) on n network outputs in time order, as one GPU stage and without a
 * stream: moving average -> first maximum -> threshold -> state machine. softmax [n][10] int8 (host); filt_state [10] fp32 in/out
 * (netOutFilt, zeros at the start), fsm in/out (edison_fsm_init at the start; NULL: no state machine), dt_us = time between two
 * inferences; outputs (host, each may be NULL): filt [n][10], likely [n], spotted [n], states [n]. n < 2^30. The recurrence rounds at every
 * step, so the chain is sequential in time by definition: ONE workgroup (ten lanes filter, one walks the machine), cost linear in n -- a
 * post-processing stage for the outputs of a stream, not a batch kernel. EDISON_E_ARGUMENT: alpha outside [0, 1], a threshold that is
 * not a number, an fsm->state that is not a state of the machine (what edison_fsm_step answers for it). */
int edison_postproc(edison_ctx *ctx, const int8_t *softmax, int64_t n, double alpha, double true_threshold, uint32_t dt_us,
                    float *filt_state, edison_fsm *fsm, float *filt, int32_t *likely, int32_t *spotted, int32_t *states);
/* roles of the ten classes in the state machine: the wake word's class index (-1: none), bit masks of the locations and values */
void edison_fsm_roles(int32_t *wake_idx, uint32_t *loc_mask, uint32_t *val_mask);

/* ---- legacy call surface of the reference firmware (batch = 1, process-global context) --------------- */
/* firmware/src/ai/ai.h:74-80. aiInitialize() creates the global context on device $EDISON_DEVICE (default 0)
 * and loads $EDISON_MODEL (default: kws_nnom.ednn next to the library). in_data: 403 int8, out_data: 10 int8. */
int aiInitialize(void);
void aiPrintInfo(void);
void aiGetInputShape(uint16_t *x, uint16_t *y);
int aiRunInference(void *in_data, void *out_data);
const char *aiGetKeywordFromIndex(uint32_t idx);
uint32_t aiGetKeywordCount(void);
/* firmware/src/ai/ai_nnom.c:64-132 */
void aiNnomTest(void);
void aiNnomInit(void);
void aiNnomPrintInfo(void);
int aiNnomRunInference(void *in_data, void *out_data);
int aiNnomPredict(uint32_t *label, float *prob);
/* nnom_predict's result rule (nnom_utils.c:272-302) alone, on the host (no GPU, no context, like edison_fsm_step): out [n][n_out] int8,
 * the graph's last output (the softmax if it ends in one, else the logits). n_out > 1: label = first strict maximum, prob = (float)max /
 * (float)(int32 sum of all n_out values), 0 when the sum is 0 (a negative sum keeps the C quotient); n_out == 1: prob = out / 127.f,
 * label = prob >= 0.5f. prob may be NULL. aiNnomPredict is this on the shipped graph's softmax. */
int edison_nnom_predict(const int8_t *out, int64_t n, int n_out, uint32_t *label, float *prob);
int8_t *aiNnomGetInputBuffer(void);
int8_t *aiNnomGetOutputBuffer(void);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Scoring a labelled data set: NNoM's evaluation API -- prediction_create / prediction_run / prediction_matrix /
 * prediction_top_k (nnom_utils.c:20-254) -- and the float model's predictWithConfMatrix (kws_keras.py:503-517), with the counters in
 * device memory. The data set goes in chunk by chunk behind the batch calls that produce the outputs; only the counts come back.
 *
 * rule  EDISON_EVAL_NNOM    int8 outputs (the softmax if the graph ends in one, else the logits): prediction_run. Predicted label =
 *                           first strict maximum; prob = (float)max / (float)(uint32 sum of out[1 .. n_out - 1], element 0 left out,
 *                           modulo 2^32), 0 when that sum is 0 -- the reference's quirk, kept; one output: prob = out / 127.f, label =
 *                           prob >= 0.5f, only `count` moves.
 *       EDISON_EVAL_KERAS   float32 probabilities: first class with p > 0.5f, class 0 when there is none; prob = p[label].
 *       EDISON_EVAL_ARGMAX  float32: first maximum (edison_fnet_batch's argmax); prob = p[label].
 * rank  of the true label t: the number of j != t with out[t] < out[j] plus the number of j < t with out[j] == out[t]; top_k[rank]
 *       counts it when rank < top_k (top-k accuracy = (top_k[0] + ... + top_k[k - 1]) / count). For the float rules this is the
 *       project's own extension.
 * labels int32; one outside 0 .. n_classes - 1 (-1: unlabelled) adds to `skipped` only; its pred / prob are still written, its rank
 *       is -1 (as is every rank of a one-output NNOM evaluation).
 * The matrix is always n_classes x n_classes uint64, rows = actual label, columns = predicted (NNoM's cells are uint16 and wrap at
 * 65 536; sklearn drops classes that never occur). All counting is in integers: the result does not depend on launch shape or order. */
#define EDISON_EVAL_NNOM 0
#define EDISON_EVAL_KERAS 1
#define EDISON_EVAL_ARGMAX 2
typedef struct edison_eval edison_eval;
typedef struct edison_eval_opts {
	int rule;       /* EDISON_EVAL_*; default EDISON_EVAL_NNOM */
	int n_classes;  /* 1 .. 256: outputs per utterance; default 10 */
	int top_k;      /* >= 0: entries of the top-k histogram (entries at n_classes and above stay 0); default 2 */
	int max_blocks; /* workgroups of one add: min(ceil(n / 256), max_blocks); 0 (default): twice the compute units */
} edison_eval_opts;
typedef struct edison_eval_totals {
	uint64_t count;   /* outputs counted (label in range) */
	uint64_t skipped; /* outputs whose label was out of range */
	uint64_t correct; /* the trace of the matrix */
} edison_eval_totals;
void edison_eval_default_opts(edison_eval_opts *o);
/* EDISON_E_ARGUMENT (message in edison_last_error) for n_classes outside 1 .. 256, a negative top_k or max_blocks, an unknown rule. */
int edison_eval_create(edison_ctx *ctx, const edison_eval_opts *o, edison_eval **out);
void edison_eval_destroy(edison_eval *e);
int edison_eval_reset(edison_eval *e); /* zero the counters, stream-ordered */
/* Count n outputs [n][n_classes] against labels [n], stream-ordered on the context's stream: an add follows a *_batch_dev call on the
 * same context with no synchronisation in between. pred [n] uint32, prob [n] float and rank [n] int32 are optional per-utterance
 * outputs (NULL: not written). The element type must match the rule (i8: NNOM; f32: KERAS, ARGMAX), else EDISON_E_ARGUMENT. n == 0
 * does nothing. The host forms stage their arrays and synchronise. */
int edison_eval_add_i8_dev(edison_eval *e, const int8_t *out, const int32_t *labels, int64_t n, uint32_t *pred, float *prob, int32_t *rank);
int edison_eval_add_f32_dev(edison_eval *e, const float *probs, const int32_t *labels, int64_t n, uint32_t *pred, float *prob, int32_t *rank);
int edison_eval_add_i8(edison_eval *e, const int8_t *out, const int32_t *labels, int64_t n, uint32_t *pred, float *prob, int32_t *rank);
int edison_eval_add_f32(edison_eval *e, const float *probs, const int32_t *labels, int64_t n, uint32_t *pred, float *prob, int32_t *rank);
/* Synchronise and copy the counters out: confusion [n_classes * n_classes], top_k [opts.top_k]; each of the three may be NULL. May be
 * called between adds: the counters go on. */
int edison_eval_result(edison_eval *e, edison_eval_totals *t, uint64_t *confusion, uint64_t *top_k);
/* The same rules on the host alone (no GPU, no context, like edison_nnom_predict): they ADD to confusion [n_out * n_out], topk_hist
 * [top_k] and *totals, which the caller zeroes first; every output pointer may be NULL. EDISON_E_ARGUMENT: n_out outside 1 .. 256, a
 * negative n or top_k, NULL out / labels with n > 0, a rule that is not a float one. */
int edison_nnom_prediction_run(const int8_t *out, const int32_t *labels, int64_t n, int n_out, int top_k, uint64_t *confusion,
                               uint64_t *topk_hist, uint32_t *pred, float *prob, int32_t *rank, edison_eval_totals *totals);
int edison_eval_f32_host(int rule, const float *probs, const int32_t *labels, int64_t n, int n_out, int top_k, uint64_t *confusion,
                         uint64_t *topk_hist, uint32_t *pred, float *prob, int32_t *rank, edison_eval_totals *totals);
/* firmware/src/app.c:152-153: write / push one frame's MFCCs into the process-global 403-byte net input
 * (clip to [-128,127] after integer division by NNOM_INPUT_SCALE = 1, app.c:685-693).                    */
void mfccToNetInput(int16_t *mfcc, uint16_t in_x, uint16_t in_y, uint32_t xoffset);
void mfccToNetInputPush(int16_t *mfcc, uint16_t in_x, uint16_t in_y);
/* firmware/src/audioprocessing.h:21-22: one 1024-sample frame -> pointer to a callee-owned static buffer of 32
 * int16 (valid until the next call): MFCC variant C, the firmware's own Q15 arithmetic. */
void audioInit(void);
void audioCalcMFCCs(int16_t *inp, int16_t **oup);
/* firmware/src/audio/mfcc.h:64-67 -- MFCC variant D, the float32 ML-KWS extractor of the firmware's NNoM example
 * (app.c:540,583: mfcc_create(13, 1, 512, 8, 0.97f), hop 256): pre-emphasis, Hann window, FFT of the frame padded to a
 * power of two, 26 mel bands 20..4000 Hz, logf, DCT rows feature_offset..num_mfcc_features-1, * 2^mfcc_dec_bits,
 * round, saturate to q7. The handle is opaque (the firmware's struct fields are private scratch); `mfcc_out` receives
 * num_mfcc_features - feature_offset int8. mfcc_create returns NULL on failure (bad arguments, padded length outside
 * 128..1024, no GPU). Same struct tag as the firmware's header, so both headers can be included together. */
#ifndef __KWS_MFCC_H__
typedef struct _mfcc_t mfcc_t;
#endif
mfcc_t *mfcc_create(int num_mfcc_features, int feature_offset, int frame_len, int mfcc_dec_bits, float preemph);
void mfcc_delete(mfcc_t *mfcc);
void mfcc_compute(mfcc_t *mfcc, const int16_t *audio_data, int8_t *mfcc_out);
/* mfcc.h:61, mfcc.c:101-115: the DCT-II matrix of that extractor, float32, [coefficient][input], malloc'd (host) */
float *create_dct_matrix(int32_t input_length, int32_t coefficient_count);
/* the same on an explicit context, and batched: frame i starts at audio + i*frame_step; out [n][n_out] q7,
 * out_f32 [n][n_out] (the scaled sums before round/saturate) and logmel [n][26] may be NULL */
mfcc_t *edison_mfcc_f32_create(edison_ctx *ctx, int num_mfcc_features, int feature_offset, int frame_len,
                               int mfcc_dec_bits, float preemph);
int edison_mfcc_f32_n_out(const mfcc_t *mfcc);
int edison_mfcc_f32_batch_dev(mfcc_t *mfcc, const int16_t *audio, int64_t n_frames, int64_t frame_step, int8_t *out,
                              float *out_f32, float *logmel);
int edison_mfcc_f32_batch(mfcc_t *mfcc, const int16_t *audio, int64_t n_frames, int64_t frame_step, int8_t *out,
                          float *out_f32, float *logmel);
/* Variant D over rows, mirroring edison_mfcc_rows: frame f belongs to row u = f / frames_per_row and starts at
 * audio + u * row_stride + (f % frames_per_row) * frame_step; out [n_rows * frames_per_row][n_out] back to back (out_f32, logmel
 * likewise, may be NULL). One launch; rows may overlap or leave gaps. The host form stages (n_rows - 1) * row_stride +
 * (frames_per_row - 1) * frame_step + frame_len samples. EDISON_E_SIZE: 2^31 frames or more. */
int edison_mfcc_f32_rows_dev(mfcc_t *mfcc, const int16_t *audio, int64_t n_rows, int64_t row_stride, int64_t frames_per_row,
                             int64_t frame_step, int8_t *out, float *out_f32, float *logmel);
int edison_mfcc_f32_rows(mfcc_t *mfcc, const int16_t *audio, int64_t n_rows, int64_t row_stride, int64_t frames_per_row,
                         int64_t frame_step, int8_t *out, float *out_f32, float *logmel);
/* Audio to label in one call with the loaded int8 graph (edison_model_load*: any graph the general path runs) and a variant D
 * extractor: what the firmware's NNoM example does per audio event (mfcc_compute per row, aiNnomPredict: app.c:583,613), batched.
 * The graph's input rows x n_out x 1 gives the window: n_out must be edison_mfcc_f32_n_out(mfcc); utterance u starts at
 * audio + u * utt_stride and holds `rows` frames `hop` samples apart (hop = 0: frame_len / 2, the firmware's overlap), i.e.
 * (rows - 1) * hop + frame_len samples. Three launches: the rows form above -> feat [n_utt][rows][n_out], the graph -> logits, softmax
 * [n_utt][graph outputs] (softmax is left alone for a graph without Softmax), edison_nnom_predict's rule on the graph's last output ->
 * label [n_utt] uint32, prob [n_utt] float. Every output but label may be NULL (a NULL feat goes to the context's scratch buffer).
 * EDISON_E_ARGUMENT: no graph loaded, or an extractor of another context; EDISON_E_SIZE: another input shape (the message names
 * both); both before anything is launched. The _dev form is asynchronous on the context's stream. */
int edison_kws_f32_batch_dev(edison_ctx *ctx, mfcc_t *mfcc, const int16_t *audio, int64_t n_utt, int64_t utt_stride, int64_t hop,
                             int8_t *feat, int8_t *logits, int8_t *softmax, uint32_t *label, float *prob);
int edison_kws_f32_batch(edison_ctx *ctx, mfcc_t *mfcc, const int16_t *audio, int64_t n_utt, int64_t utt_stride, int64_t hop,
                         int8_t *feat, int8_t *logits, int8_t *softmax, uint32_t *label, float *prob);

/* The front end of the firmware's NNoM keyword-spotting example around mfcc_compute (appNnomKwsRun, app.c:545-623): every
 * audio event delivers 512 new samples behind the last 256 old ones (app.c:567-575), two frames are extracted at offsets 0
 * and 256 (app.c:583) into a ring of window_rows (MFCC_LEN = 63) feature rows, and the network input is that ring oldest
 * row first (mfcc_features_seq, app.c:600-604). A push takes n_events <= max_events events (one kernel launch for all
 * their frames) and returns the window after every event: windows [n_events][window_rows][n_out] int8. State (samples and
 * rows) starts as zeros, like the firmware's static buffers. The extractor must be a 512-sample one on the same context and
 * must outlive the stream (edison_f32_stream_destroy before mfcc_delete). */
typedef struct edison_f32_stream edison_f32_stream;
int edison_f32_stream_create(edison_ctx *ctx, mfcc_t *mfcc, int window_rows, int max_events, edison_f32_stream **out);
void edison_f32_stream_destroy(edison_f32_stream *s);
int edison_f32_stream_reset(edison_f32_stream *s);
int64_t edison_f32_stream_events_seen(const edison_f32_stream *s);
int edison_f32_stream_push_dev(edison_f32_stream *s, const int16_t *samples, int n_events, int8_t *windows);
int edison_f32_stream_push(edison_f32_stream *s, const int16_t *samples, int n_events, int8_t *windows);
/* The example's whole loop: a push that also runs the loaded int8 graph on the window after every event and nnom_predict's rule on
 * its output: logits, softmax [n_events][graph outputs], label [n_events] uint32, prob [n_events] float; every output but label may
 * be NULL. The graph reads the overlapping windows in place (no window copy). Its input must be window_rows x n_out x 1 (checked
 * per call as in edison_kws_f32_batch). State, reset and events_seen as for push; push and predict may be mixed on one stream. */
int edison_f32_stream_predict_dev(edison_f32_stream *s, const int16_t *samples, int n_events, int8_t *logits, int8_t *softmax,
                                  uint32_t *label, float *prob);
int edison_f32_stream_predict(edison_f32_stream *s, const int16_t *samples, int n_events, int8_t *logits, int8_t *softmax,
                              uint32_t *label, float *prob);
/* One 1024-sample frame through the GPU MFCC, any variant; out32 fp32. */
int edison_mfcc_frame(const int16_t *frame1024, int variant, float *out32);
edison_ctx *edison_global_ctx(void);

#ifdef __cplusplus
}
#endif
#endif
