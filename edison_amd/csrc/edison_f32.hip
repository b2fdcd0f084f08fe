/*
 * edison_f32.hip -- C-ABI entry points of MFCC variant D, the firmware's float32 ML-KWS extractor, under the
 * firmware's own names (firmware/src/audio/mfcc.h:64-67: mfcc_create / mfcc_compute / mfcc_delete) plus the batched
 * forms. The kernel is mfcc_f32_kernels.hip, the tables tables_f32.c. No CPU path.
 */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "edison_ctx.h"
#include "nnom_predict_core.h"

extern "C" int ed_launch_mfcc_f32(const ed_mfcc_f32_args_t *args, const ed_f32_tables_t *dev_tab, int padded, int n_cu, hipStream_t stream);
extern "C" int ed_launch_mfcc_f32_fast(const ed_mfcc_f32_args_t *args, const ed_f32_tables_t *dev_tab, const ed_mfcc_tables_t *dev_fft_tab,
                                       int n_cu, hipStream_t stream);

/* the handle: opaque to callers (the firmware's struct fields are its private scratch) */
struct _mfcc_t
{
	edison_ctx *ctx;
	ed_f32_tables_t *d_tab;
	int n_out, frame_len, padded;
};

extern "C" mfcc_t *edison_mfcc_f32_create(edison_ctx *ctx, int num_mfcc_features, int feature_offset, int frame_len,
                                          int mfcc_dec_bits, float preemph)
{
	if (!ctx) return NULL;
	ed_f32_tables_t *h = (ed_f32_tables_t *)malloc(sizeof(ed_f32_tables_t));
	mfcc_t *m = (mfcc_t *)calloc(1, sizeof(mfcc_t));
	if (!h || !m) { free(h); free(m); ed_set_err(ctx, EDISON_E_NO_MEMORY, "host allocation failed"); return NULL; }
	int r = ed_build_f32_tables(num_mfcc_features, feature_offset, frame_len, mfcc_dec_bits, preemph, h, ctx->err, sizeof(ctx->err));
	hipError_t e = hipSuccess;
	const int padded = r == EDISON_OK ? h->padded : 0; /* the kernel's per-wave LDS buffer is sized by it */
	if (r == EDISON_OK)
	{
		e = hipSetDevice(ctx->device);
		if (e == hipSuccess) e = hipMalloc((void **)&m->d_tab, sizeof(ed_f32_tables_t));
		if (e == hipSuccess) e = hipMemcpy(m->d_tab, h, sizeof(ed_f32_tables_t), hipMemcpyHostToDevice);
		if (e != hipSuccess) snprintf(ctx->err, sizeof(ctx->err), "mfcc_create: %s", hipGetErrorString(e));
	}
	free(h);
	if (r != EDISON_OK || e != hipSuccess)
	{
		if (m->d_tab) (void)hipFree(m->d_tab);
		free(m);
		return NULL;
	}
	m->ctx = ctx;
	m->n_out = num_mfcc_features - feature_offset;
	m->frame_len = frame_len;
	m->padded = padded;
	return m;
}

extern "C" void mfcc_delete(mfcc_t *mfcc)
{
	if (!mfcc) return;
	if (mfcc->d_tab) { (void)hipSetDevice(mfcc->ctx->device); (void)hipStreamSynchronize(mfcc->ctx->stream); (void)hipFree(mfcc->d_tab); }
	free(mfcc);
}

extern "C" int edison_mfcc_f32_n_out(const mfcc_t *mfcc) { return mfcc ? mfcc->n_out : EDISON_E_ARGUMENT; }

/* both forms of the frame addressing (ed_mfcc_f32_args_t) on the kernel that serves the extractor's padded length */
static int f32_launch(mfcc_t *mfcc, const ed_mfcc_f32_args_t &a)
{
	edison_ctx *ctx = mfcc->ctx;
	/* frames padded to 512 points (the firmware's configuration) take the register-FFT kernel; its FFT twiddles are those
	 * of the variant A / B tables (a property of the 512-point transform, not of the filterbank). EDISON_F32_GENERIC=1
	 * keeps the generic radix-2 kernel, for A/B measurements */
	static const int generic = getenv("EDISON_F32_GENERIC") ? atoi(getenv("EDISON_F32_GENERIC")) : 0;
	int e = (mfcc->padded == 512 && ctx->d_tab[0] && !generic)
	            ? ed_launch_mfcc_f32_fast(&a, mfcc->d_tab, ctx->d_tab[0], ctx->n_cu, ctx->stream)
	            : ed_launch_mfcc_f32(&a, mfcc->d_tab, mfcc->padded, ctx->n_cu, ctx->stream);
	return ed_launch_result(ctx, e, "float32 MFCC kernel");
}

extern "C" int edison_mfcc_f32_batch_dev(mfcc_t *mfcc, const int16_t *audio, int64_t n_frames, int64_t frame_step,
                                         int8_t *out, float *out_f32, float *logmel)
{
	if (!mfcc || n_frames < 0 || frame_step < 0 || ((!audio || !out) && n_frames > 0)) return EDISON_E_ARGUMENT;
	if (n_frames == 0) return EDISON_OK;
	ed_mfcc_f32_args_t a;
	a.audio = audio; a.n_frames = n_frames; a.frame_step = frame_step; a.out = out; a.out_f32 = out_f32; a.logmel = logmel;
	a.frames_per_row = 0; a.row_stride = 0;
	return f32_launch(mfcc, a);
}

/* ---- variant D over rows (as edison_mfcc_rows for variants A / B): frame f of row u = f / frames_per_row starts at
 * audio + u * row_stride + (f % frames_per_row) * frame_step; outputs [n_rows * frames_per_row][..] back to back */
static int f32_rows_check(mfcc_t *mfcc, const int16_t *audio, int64_t n_rows, int64_t row_stride, int64_t frames_per_row, int64_t frame_step,
                          const int8_t *out)
{
	if (!mfcc || n_rows < 0 || row_stride < 0 || frames_per_row < 0 || frame_step < 0) return EDISON_E_ARGUMENT;
	if (n_rows == 0 || frames_per_row == 0) return EDISON_OK;
	if (!audio || !out) return EDISON_E_ARGUMENT;
	if (n_rows > INT32_MAX / frames_per_row) return ed_set_err(mfcc->ctx, EDISON_E_SIZE, "edison_mfcc_f32_rows: more than 2^31 frames in one call");
	return EDISON_OK;
}

extern "C" int edison_mfcc_f32_rows_dev(mfcc_t *mfcc, const int16_t *audio, int64_t n_rows, int64_t row_stride, int64_t frames_per_row,
                                        int64_t frame_step, int8_t *out, float *out_f32, float *logmel)
{
	{ const int r = f32_rows_check(mfcc, audio, n_rows, row_stride, frames_per_row, frame_step, out); if (r != EDISON_OK) return r; }
	if (n_rows == 0 || frames_per_row == 0) return EDISON_OK;
	ed_mfcc_f32_args_t a;
	a.audio = audio; a.n_frames = n_rows * frames_per_row; a.frame_step = frame_step; a.out = out; a.out_f32 = out_f32; a.logmel = logmel;
	a.frames_per_row = frames_per_row; a.row_stride = row_stride;
	return f32_launch(mfcc, a);
}

/* samples a host call stages: (n_rows - 1) * row_stride + (frames_per_row - 1) * frame_step + frame_len, in 128 bits, refused beyond
 * 2^46 samples (as edison_mfcc_rows) */
static int f32_rows_samples(mfcc_t *mfcc, int64_t n_rows, int64_t row_stride, int64_t frames_per_row, int64_t frame_step, const char *who, size_t *n)
{
	const unsigned __int128 na = (unsigned __int128)(n_rows - 1) * (unsigned __int128)row_stride +
	                             (unsigned __int128)(frames_per_row - 1) * (unsigned __int128)frame_step + (unsigned __int128)mfcc->frame_len;
	if (na * sizeof(int16_t) > ((unsigned __int128)1 << 47))
	{
		snprintf(mfcc->ctx->err, sizeof(mfcc->ctx->err), "%s: row_stride x n_rows too large", who);
		return EDISON_E_SIZE;
	}
	*n = (size_t)na;
	return EDISON_OK;
}

extern "C" int edison_mfcc_f32_rows(mfcc_t *mfcc, const int16_t *audio, int64_t n_rows, int64_t row_stride, int64_t frames_per_row,
                                    int64_t frame_step, int8_t *out, float *out_f32, float *logmel)
{
	{ const int r = f32_rows_check(mfcc, audio, n_rows, row_stride, frames_per_row, frame_step, out); if (r != EDISON_OK) return r; }
	if (n_rows == 0 || frames_per_row == 0) return EDISON_OK;
	size_t na = 0;
	{ const int r = f32_rows_samples(mfcc, n_rows, row_stride, frames_per_row, frame_step, "edison_mfcc_f32_rows", &na); if (r != EDISON_OK) return r; }
	ed_staging st(mfcc->ctx);
	const size_t n = (size_t)(n_rows * frames_per_row), no = (size_t)mfcc->n_out;
	const int16_t *a = st.in(audio, na);
	int8_t *o = st.out(out, n * no);
	float *f = st.out(out_f32, n * no), *l = st.out(logmel, n * ED_F32_NUM_FBANK);
	return st.finish(st.ok() ? edison_mfcc_f32_rows_dev(mfcc, a, n_rows, row_stride, frames_per_row, frame_step, o, f, l) : EDISON_OK);
}

extern "C" int edison_mfcc_f32_batch(mfcc_t *mfcc, const int16_t *audio, int64_t n_frames, int64_t frame_step, int8_t *out,
                                     float *out_f32, float *logmel)
{
	if (!mfcc || n_frames < 0 || frame_step < 0 || ((!audio || !out) && n_frames > 0)) return EDISON_E_ARGUMENT;
	if (n_frames == 0) return EDISON_OK;
	edison_ctx *ctx = mfcc->ctx;
	ed_staging st(ctx);
	const size_t n = (size_t)n_frames, no = (size_t)mfcc->n_out;
	const int16_t *a = st.in(audio, (size_t)(n_frames - 1) * (size_t)frame_step + (size_t)mfcc->frame_len);
	int8_t *o = st.out(out, n * no);
	float *f = st.out(out_f32, n * no), *l = st.out(logmel, n * ED_F32_NUM_FBANK);
	return st.finish(st.ok() ? edison_mfcc_f32_batch_dev(mfcc, a, n_frames, frame_step, o, f, l) : EDISON_OK);
}

/* ---- the firmware's own names, on the process-global context (created like aiInitialize does) ---- */
extern "C" mfcc_t *mfcc_create(int num_mfcc_features, int feature_offset, int frame_len, int mfcc_dec_bits, float preemph)
{
	edison_ctx *ctx = edison_global_ctx();
	if (!ctx)
	{
		if (aiInitialize() != EDISON_OK) return NULL;
		ctx = edison_global_ctx();
	}
	return edison_mfcc_f32_create(ctx, num_mfcc_features, feature_offset, frame_len, mfcc_dec_bits, preemph);
}

extern "C" void mfcc_compute(mfcc_t *mfcc, const int16_t *audio_data, int8_t *mfcc_out)
{
	if (!mfcc || !audio_data || !mfcc_out) return;
	if (edison_mfcc_f32_batch(mfcc, audio_data, 1, mfcc->frame_len, mfcc_out, NULL, NULL) != EDISON_OK)
	{
		fprintf(stderr, "mfcc_compute: GPU MFCC failed: %s\n", edison_last_error(mfcc->ctx));
		memset(mfcc_out, 0, (size_t)mfcc->n_out);
	}
}

/* ================================================================================================================
 * Audio to label in one call: variant D over rows -> the loaded int8 graph -> nnom_predict's result rule.
 * The firmware's NNoM example does the three steps per audio event (mfcc_compute x 2, aiNnomPredict: app.c:583,613).
 */

/* one lane per input: nnom_predict's rule (nnom_predict_core.h) on the graph's last output, n_out int8 values per input */
__global__ __launch_bounds__(256) void ed_nnom_predict_kernel(const int8_t *__restrict__ out, int64_t n, int n_out, uint32_t *__restrict__ label,
                                                              float *__restrict__ prob)
{
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
	{
		uint32_t l;
		float p;
		ed_nnom_predict_one(out + i * n_out, n_out, &l, &p);
		label[i] = l;
		if (prob) prob[i] = p;
	}
}

static int f32_predict_launch(edison_ctx *ctx, const int8_t *last, int64_t n, uint32_t *label, float *prob)
{
	int64_t blocks = (n + 255) / 256;
	if (blocks > 4096) blocks = 4096;
	hipLaunchKernelGGL(ed_nnom_predict_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, last, n, ctx->net.out_n, label, prob);
	return ed_launch_result(ctx, (int)hipGetLastError(), "nnom_predict kernel");
}

/* The loaded int8 graph must read windows of this extractor's rows: in_h x n_out x 1, in_h = rows (rows = 0: the graph decides).
 * Refused before anything is launched, naming both shapes. */
static int f32_window_check(edison_ctx *ctx, const mfcc_t *mfcc, int rows, const char *who)
{
	if (mfcc->ctx != ctx)
	{
		snprintf(ctx->err, sizeof(ctx->err), "%s: the extractor belongs to another context", who);
		return EDISON_E_ARGUMENT;
	}
	if (!ctx->have_model)
	{
		snprintf(ctx->err, sizeof(ctx->err), "%s: no int8 graph loaded (edison_model_load)", who);
		return EDISON_E_ARGUMENT;
	}
	const ed_net_plan_t *p = &ctx->net;
	if (p->in_w != mfcc->n_out || p->in_c != 1 || (rows && p->in_h != rows))
	{
		char want[32];
		if (rows) snprintf(want, sizeof(want), "%d", rows); else snprintf(want, sizeof(want), "rows");
		snprintf(ctx->err, sizeof(ctx->err), "%s: the loaded graph's input is %d x %d x %d, the extractor's windows are %s x %d x 1", who, p->in_h,
		         p->in_w, p->in_c, want, mfcc->n_out);
		return EDISON_E_SIZE;
	}
	return EDISON_OK;
}

/* The graph's last output where the caller gave no buffer for it: behind `front` bytes of the context's scratch. */
static int f32_last_output(edison_ctx *ctx, size_t front, int64_t n, int8_t *logits, int8_t *softmax, int8_t **lg, int8_t **sm, int8_t **front_out)
{
	const int has_sm = ctx->net.has_softmax;
	const bool need = has_sm ? !softmax : !logits;
	front = (front + 15) & ~(size_t)15;
	const size_t total = front + (need ? (size_t)n * (size_t)ctx->net.out_n : 0);
	if (total)
	{
		const int r = ed_ctx_ensure_scratch(ctx, total);
		if (r != EDISON_OK) return r;
	}
	int8_t *own = need ? (int8_t *)ctx->scratch + front : NULL;
	*lg = has_sm ? logits : (logits ? logits : own);
	*sm = has_sm ? (softmax ? softmax : own) : NULL; /* a graph without Softmax leaves `softmax` alone */
	if (front_out) *front_out = front ? (int8_t *)ctx->scratch : NULL;
	return EDISON_OK;
}

static int kws_f32_check(edison_ctx *ctx, mfcc_t *mfcc, int64_t n_utt, int64_t utt_stride, int64_t *hop)
{
	if (!ctx || !mfcc || n_utt < 0 || utt_stride < 0 || *hop < 0) return EDISON_E_ARGUMENT;
	{ const int r = f32_window_check(ctx, mfcc, 0, "edison_kws_f32_batch"); if (r != EDISON_OK) return r; }
	if (*hop == 0) *hop = mfcc->frame_len / 2; /* the firmware's 50 % overlap (app.c:583) */
	if (n_utt > INT32_MAX / ctx->net.in_h) return ed_set_err(ctx, EDISON_E_SIZE, "edison_kws_f32_batch: more than 2^31 frames in one call");
	return EDISON_OK;
}

extern "C" int edison_kws_f32_batch_dev(edison_ctx *ctx, mfcc_t *mfcc, const int16_t *audio, int64_t n_utt, int64_t utt_stride, int64_t hop,
                                        int8_t *feat, int8_t *logits, int8_t *softmax, uint32_t *label, float *prob)
{
	{ const int r = kws_f32_check(ctx, mfcc, n_utt, utt_stride, &hop); if (r != EDISON_OK) return r; }
	if (n_utt == 0) return EDISON_OK;
	if (!audio || !label) return EDISON_E_ARGUMENT;
	ED_HIP(ctx, hipSetDevice(ctx->device));
	int8_t *lg = NULL, *sm = NULL, *f = feat;
	{
		int8_t *own = NULL;
		const int r = f32_last_output(ctx, feat ? 0 : (size_t)n_utt * (size_t)ctx->net.in_n, n_utt, logits, softmax, &lg, &sm, &own);
		if (r != EDISON_OK) return r;
		if (!f) f = own;
	}
	{ const int r = edison_mfcc_f32_rows_dev(mfcc, audio, n_utt, utt_stride, ctx->net.in_h, hop, f, NULL, NULL); if (r != EDISON_OK) return r; }
	{
		const int e = ed_ctx_net_launch(ctx, f, n_utt, ctx->net.in_n, lg, sm, NULL);
		if (e != 0) return ed_launch_result(ctx, e, "network kernel");
	}
	return f32_predict_launch(ctx, ctx->net.has_softmax ? sm : lg, n_utt, label, prob);
}

extern "C" int edison_kws_f32_batch(edison_ctx *ctx, mfcc_t *mfcc, const int16_t *audio, int64_t n_utt, int64_t utt_stride, int64_t hop,
                                    int8_t *feat, int8_t *logits, int8_t *softmax, uint32_t *label, float *prob)
{
	{ const int r = kws_f32_check(ctx, mfcc, n_utt, utt_stride, &hop); if (r != EDISON_OK) return r; }
	if (n_utt == 0) return EDISON_OK;
	if (!audio || !label) return EDISON_E_ARGUMENT;
	size_t na = 0;
	{ const int r = f32_rows_samples(mfcc, n_utt, utt_stride, ctx->net.in_h, hop, "edison_kws_f32_batch", &na); if (r != EDISON_OK) return r; }
	const size_t n = (size_t)n_utt, out_n = (size_t)ctx->net.out_n;
	ed_staging st(ctx);
	const int16_t *au = st.in(audio, na);
	int8_t *f = st.out(feat, n * (size_t)ctx->net.in_n), *l = st.out(logits, n * out_n);
	int8_t *s = st.out(ctx->net.has_softmax ? softmax : (int8_t *)NULL, n * out_n);
	uint32_t *lb = st.out(label, n);
	float *pr = st.out(prob, n);
	return st.finish(st.ok() ? edison_kws_f32_batch_dev(ctx, mfcc, au, n_utt, utt_stride, hop, f, l, s, lb, pr) : EDISON_OK);
}

/* ================================================================================================================
 * The front end of the firmware's NNoM keyword-spotting example around mfcc_compute (appNnomKwsRun, app.c:545-623):
 * every audio event brings AUDIO_FRAME_LEN = 512 new samples; they are appended behind the last 256 old ones
 * (audio_buffer_16bit, app.c:507,567-575), TWO frames are extracted at offsets 0 and 256 (50 % overlap, app.c:583) and
 * go into a ring of MFCC_LEN = 63 feature rows (app.c:508,594-596); the network input is the ring unrolled oldest row
 * first (mfcc_features_seq, app.c:600-604). Here the state (256 samples, window_rows feature rows, both starting as
 * zeros like the firmware's static buffers) lives in HBM, a push takes any number of events, runs ONE launch of the
 * variant D kernel over all 2 * n_events frames and returns the window after EVERY event.
 */
struct edison_f32_stream
{
	edison_ctx *ctx;
	mfcc_t *mfcc;
	int rows, n_out, max_events;
	int16_t *d_audio; /* [256 + max_events * 512] */
	int8_t *d_feat;   /* [rows + 2 * max_events][n_out]: the last `rows` rows, then the rows of the running push */
	int64_t events_seen;
};

/* window e (after event e of this push) = feature rows 2e+2 .. 2e+1+rows of d_feat; then the state moves up */
__global__ void ed_f32_windows_kernel(const int8_t *__restrict__ feat, int rows, int n_out, int n_events, int8_t *__restrict__ win)
{
	const int64_t per = (int64_t)rows * n_out, total = per * n_events;
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
	{
		const int64_t e = i / per, r = i - e * per;
		win[i] = feat[(2 * e + 2) * n_out + r];
	}
}

/* one workgroup: the last `rows` feature rows and the last 256 samples become the state of the next push (read
 * everything, barrier, write: the ranges may overlap) */
__global__ __launch_bounds__(256) void ed_f32_shift_kernel(int8_t *feat, int rows, int n_out, int n_events, int16_t *audio)
{
	extern __shared__ int8_t sh[];
	const int nf = rows * n_out;
	int16_t *sa = reinterpret_cast<int16_t *>(sh + ((nf + 15) & ~15));
	for (int i = threadIdx.x; i < nf; i += 256) sh[i] = feat[(int64_t)2 * n_events * n_out + i];
	for (int i = threadIdx.x; i < 256; i += 256) sa[i] = audio[(int64_t)n_events * 512 + i];
	__syncthreads();
	for (int i = threadIdx.x; i < nf; i += 256) feat[i] = sh[i];
	for (int i = threadIdx.x; i < 256; i += 256) audio[i] = sa[i];
}

extern "C" int edison_f32_stream_create(edison_ctx *ctx, mfcc_t *mfcc, int window_rows, int max_events, edison_f32_stream **out)
{
	if (!ctx || !mfcc || !out) return EDISON_E_ARGUMENT;
	*out = NULL;
	if (mfcc->ctx != ctx) return ed_set_err(ctx, EDISON_E_ARGUMENT, "f32 stream: the extractor belongs to another context");
	if (mfcc->frame_len != 512) return ed_set_err(ctx, EDISON_E_NO_IMPL, "f32 stream: the firmware's front end is defined for 512-sample frames (AUDIO_FRAME_LEN, app.c:497)");
	if (window_rows < 2 || window_rows > 1024 || max_events < 1 || max_events > (1 << 20)) return ed_set_err(ctx, EDISON_E_ARGUMENT, "f32 stream: bad window_rows / max_events");
	edison_f32_stream *s = (edison_f32_stream *)calloc(1, sizeof(edison_f32_stream));
	if (!s) return ed_set_err(ctx, EDISON_E_NO_MEMORY, "host allocation failed");
	s->ctx = ctx; s->mfcc = mfcc; s->rows = window_rows; s->n_out = mfcc->n_out; s->max_events = max_events;
	const size_t na = (256 + (size_t)max_events * 512) * sizeof(int16_t), nf = ((size_t)window_rows + 2 * (size_t)max_events) * mfcc->n_out;
	hipError_t e = hipSetDevice(ctx->device);
	if (e == hipSuccess) e = hipMalloc((void **)&s->d_audio, na);
	if (e == hipSuccess) e = hipMalloc((void **)&s->d_feat, nf);
	if (e == hipSuccess) e = hipMemsetAsync(s->d_audio, 0, na, ctx->stream);
	if (e == hipSuccess) e = hipMemsetAsync(s->d_feat, 0, nf, ctx->stream);
	if (e != hipSuccess)
	{
		snprintf(ctx->err, sizeof(ctx->err), "f32 stream: %s", hipGetErrorString(e));
		if (s->d_audio) (void)hipFree(s->d_audio);
		if (s->d_feat) (void)hipFree(s->d_feat);
		free(s);
		return EDISON_E_RUNTIME;
	}
	*out = s;
	return EDISON_OK;
}

extern "C" void edison_f32_stream_destroy(edison_f32_stream *s)
{
	if (!s) return;
	(void)hipSetDevice(s->ctx->device);
	(void)hipStreamSynchronize(s->ctx->stream);
	(void)hipFree(s->d_audio);
	(void)hipFree(s->d_feat);
	free(s);
}

extern "C" int edison_f32_stream_reset(edison_f32_stream *s)
{
	if (!s) return EDISON_E_ARGUMENT;
	edison_ctx *ctx = s->ctx;
	ED_HIP(ctx, hipMemsetAsync(s->d_audio, 0, 256 * sizeof(int16_t), ctx->stream));
	ED_HIP(ctx, hipMemsetAsync(s->d_feat, 0, (size_t)s->rows * s->n_out, ctx->stream));
	s->events_seen = 0;
	return EDISON_OK;
}

extern "C" int64_t edison_f32_stream_events_seen(const edison_f32_stream *s) { return s ? s->events_seen : 0; }

/* the first half of a push: the new samples behind the 256 old ones, ONE variant D launch over the 2 * n_events new frames */
static int f32_stream_rows(edison_f32_stream *s, const int16_t *samples, int n_events)
{
	edison_ctx *ctx = s->ctx;
	ED_HIP(ctx, hipMemcpyAsync(s->d_audio + 256, samples, (size_t)n_events * 512 * sizeof(int16_t), hipMemcpyDeviceToDevice, ctx->stream));
	return edison_mfcc_f32_batch_dev(s->mfcc, s->d_audio, 2 * (int64_t)n_events, 256, s->d_feat + (size_t)s->rows * s->n_out, NULL, NULL);
}

/* the last half: the state moves up */
static int f32_stream_shift(edison_f32_stream *s, int n_events)
{
	edison_ctx *ctx = s->ctx;
	const size_t lds = (((size_t)s->rows * s->n_out + 15) & ~(size_t)15) + 512;
	hipLaunchKernelGGL(ed_f32_shift_kernel, dim3(1), dim3(256), lds, ctx->stream, s->d_feat, s->rows, s->n_out, n_events, s->d_audio);
	ED_HIP(ctx, hipGetLastError());
	s->events_seen += n_events;
	return EDISON_OK;
}

/* samples: n_events x 512 new int16 samples (device); windows: [n_events][window_rows][n_out] int8 (device), window e =
 * what mfcc_features_seq holds after event e. Asynchronous on the context's stream. */
extern "C" int edison_f32_stream_push_dev(edison_f32_stream *s, const int16_t *samples, int n_events, int8_t *windows)
{
	if (!s || n_events < 0 || (n_events > 0 && (!samples || !windows))) return EDISON_E_ARGUMENT;
	if (n_events == 0) return EDISON_OK;
	edison_ctx *ctx = s->ctx;
	if (n_events > s->max_events) return ed_set_err(ctx, EDISON_E_SIZE, "f32 stream: more events than the stream was created for");
	{ const int r = f32_stream_rows(s, samples, n_events); if (r != EDISON_OK) return r; }
	const int64_t total = (int64_t)n_events * s->rows * s->n_out;
	int blocks = (int)((total + 255) / 256);
	if (blocks > 4096) blocks = 4096;
	hipLaunchKernelGGL(ed_f32_windows_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, s->d_feat, s->rows, s->n_out, n_events, windows);
	return f32_stream_shift(s, n_events);
}

/* the same with host pointers; synchronous */
extern "C" int edison_f32_stream_push(edison_f32_stream *s, const int16_t *samples, int n_events, int8_t *windows)
{
	if (!s || n_events < 0 || (n_events > 0 && (!samples || !windows))) return EDISON_E_ARGUMENT;
	if (n_events == 0) return EDISON_OK;
	edison_ctx *ctx = s->ctx;
	if (n_events > s->max_events) return ed_set_err(ctx, EDISON_E_SIZE, "f32 stream: more events than the stream was created for");
	ed_staging st(ctx);
	const int16_t *a = st.in(samples, (size_t)n_events * 512);
	int8_t *w = st.out(windows, (size_t)n_events * s->rows * s->n_out);
	return st.finish(st.ok() ? edison_f32_stream_push_dev(s, a, n_events, w) : EDISON_OK);
}


/* ---- the example's whole loop (app.c:545-623): per event two frames, the window, aiNnomPredict. One variant D launch over the new
 * frames, the loaded graph over the n_events overlapping windows read IN PLACE from d_feat (window e starts at row 2e + 2: an input
 * stride of 2 * n_out bytes, nothing is copied), nnom_predict's rule, the shift. May be mixed with edison_f32_stream_push* on one
 * stream: both leave the same state. */
static int f32_predict_check(edison_f32_stream *s, const int16_t *samples, int n_events, const uint32_t *label)
{
	if (!s || n_events < 0 || (n_events > 0 && (!samples || !label))) return EDISON_E_ARGUMENT;
	if (n_events == 0) return EDISON_OK;
	{ const int r = f32_window_check(s->ctx, s->mfcc, s->rows, "edison_f32_stream_predict"); if (r != EDISON_OK) return r; }
	if (n_events > s->max_events) return ed_set_err(s->ctx, EDISON_E_SIZE, "f32 stream: more events than the stream was created for");
	return EDISON_OK;
}

extern "C" int edison_f32_stream_predict_dev(edison_f32_stream *s, const int16_t *samples, int n_events, int8_t *logits, int8_t *softmax,
                                             uint32_t *label, float *prob)
{
	{ const int r = f32_predict_check(s, samples, n_events, label); if (r != EDISON_OK) return r; }
	if (n_events == 0) return EDISON_OK;
	edison_ctx *ctx = s->ctx;
	int8_t *lg = NULL, *sm = NULL;
	{ const int r = f32_last_output(ctx, 0, n_events, logits, softmax, &lg, &sm, NULL); if (r != EDISON_OK) return r; }
	{ const int r = f32_stream_rows(s, samples, n_events); if (r != EDISON_OK) return r; }
	{
		const int e = ed_ctx_net_launch(ctx, s->d_feat + 2 * (size_t)s->n_out, n_events, 2 * (int64_t)s->n_out, lg, sm, NULL);
		if (e != 0) return ed_launch_result(ctx, e, "network kernel");
	}
	{ const int r = f32_predict_launch(ctx, ctx->net.has_softmax ? sm : lg, n_events, label, prob); if (r != EDISON_OK) return r; }
	return f32_stream_shift(s, n_events);
}

/* the same with host pointers; synchronous */
extern "C" int edison_f32_stream_predict(edison_f32_stream *s, const int16_t *samples, int n_events, int8_t *logits, int8_t *softmax,
                                         uint32_t *label, float *prob)
{
	{ const int r = f32_predict_check(s, samples, n_events, label); if (r != EDISON_OK) return r; }
	if (n_events == 0) return EDISON_OK;
	edison_ctx *ctx = s->ctx;
	const size_t n = (size_t)n_events, out_n = (size_t)ctx->net.out_n;
	ed_staging st(ctx);
	const int16_t *a = st.in(samples, n * 512);
	int8_t *l = st.out(logits, n * out_n), *sm = st.out(ctx->net.has_softmax ? softmax : (int8_t *)NULL, n * out_n);
	uint32_t *lb = st.out(label, n);
	float *pr = st.out(prob, n);
	return st.finish(st.ok() ? edison_f32_stream_predict_dev(s, a, n_events, l, sm, lb, pr) : EDISON_OK);
}
