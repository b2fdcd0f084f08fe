/*
 * edison_stream_geom.hip -- continuous mode for a graph trained at ANY MFCC geometry (include/edison_hip.h, edison_stream_geom_*): the
 * continuous counterpart of edison_kws_geom_batch*, as edison_stream.hip is the one of edison_kws_batch*. A push of n new frames runs
 *
 *     [shift, only when the push would not fit] -> MFCC (ed_mfcc_geom_kernel, float64) -> network over the n overlapping windows
 *     -> [n_out-class output filter (+ edisonFSM)]
 *
 * Device state: two sliding buffers `slots` pushes long,
 *     d_audio  [T + slots * chunk * hop] int16     T = max(0, frame_len - hop) samples of history, then the new samples
 *     d_feat   [F - 1 + slots * chunk][num_mfcc]   F - 1 rows of history, then the new rows
 * whose history starts at frame `pos` (samples pos * hop, rows pos): a push appends behind it and advances pos by its frames; window i
 * of the push is rows pos + i .. pos + i + F - 1, read by the network kernel at a stride of num_mfcc bytes, nothing copied. When the
 * next push would run past the end, the shift kernel first moves the history back to the front. The stream owns its own tables, so
 * batch calls at other geometries on the same context never touch it.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "edison_ctx.h"
#include "edison_fsm_core.h"
#include "edison_stream_kernels.h"
#include "mfcc_geom.h"

struct edison_stream_geom
{
	edison_ctx *ctx;
	int F, nm, hop, tail, chunk;   /* frames per window, coefficients per row, frame_step, T history samples, frames per push */
	int n_out, has_softmax, in_n;
	int filter, fsm;
	double alpha, one_minus_alpha, threshold;
	ed_geom_cache tab;             /* this stream's own tables (edison_kws_geom.hip builds them) */
	ed_geom_args_t margs;          /* tab.tmpl with the per-geometry fields; audio, feat and the frame counts are set per push */
	int slots, pos;                /* buffers of `slots` pushes; the history starts at frame pos */
	int16_t *d_audio;
	int8_t *d_feat;
	/* every output of a push in one block (device d_out, pinned h_out), so that a host push downloads once */
	unsigned char *d_out, *h_out;
	size_t off_soft, off_argmax, off_filt, off_likely, off_spotted, off_states, off_fsm, out_bytes;
	int16_t *h_in;                 /* pinned [chunk * hop]: the host push's upload */
	float *d_state;                /* [n_out] the filter state */
	edison_fsm *d_fsm;
	ed_fsm_roles_t roles;
	uint32_t dt_us;
	hipStream_t own;               /* host pushes run here */
	hipEvent_t ev;
	hipStream_t q_last;            /* where the last unsynchronised work on the stream's state went (device pushes: the caller's stream) */
	int q_pending;
	int last_n, last_staged;       /* frames of the last push; 1: its outputs are in h_out already (host push) */
	int64_t frames_seen;
	int model_epoch;
};

/* The newest `tail` samples from audio + a_src and `feat_bytes` history bytes from feat + f_src to the front of their buffers. The
 * destination lies BELOW the source and may overlap it: in rounds of 256 elements every lane reads, the workgroup waits, every lane
 * writes. A write to element j clobbers source element j - src < j, which this round or an earlier one has already read. */
__global__ __launch_bounds__(256) void ed_stream_geom_shift_kernel(int16_t *audio, int64_t a_src, int tail, int8_t *feat, int64_t f_src,
                                                                   int feat_bytes)
{
	const int t = threadIdx.x;
	for (int base = 0; base < tail; base += 256)
	{
		const int j = base + t;
		const int16_t v = j < tail ? audio[a_src + j] : (int16_t)0;
		__syncthreads();
		if (j < tail) audio[j] = v;
		__syncthreads();
	}
	for (int base = 0; base < feat_bytes; base += 256)
	{
		const int j = base + t;
		const int8_t v = j < feat_bytes ? feat[f_src + j] : (int8_t)0;
		__syncthreads();
		if (j < feat_bytes) feat[j] = v;
		__syncthreads();
	}
}

/*
 * The firmware's post-processing (app.c:332-356) over n_out classes, for the n inferences of a push:
 *   state[c] = (float)(alpha * (double)state[c] + (1 - alpha) * (double)x[c])   product and sum rounded separately, no contraction
 *   likely = first maximum of the state row, spotted = likely if that maximum > threshold, else -1
 * The recurrence is sequential in time; classes run on lanes, the per-frame maximum afterwards on frames. One workgroup.
 * T = int8_t: the int8 graph's softmax / logits (this file); T = float: the float network's probabilities (edison_stream_float.hip).
 * (double)x is exact for both.
 */
template <class T>
__global__ __launch_bounds__(256) void ed_stream_geom_filter_kernel(const T *x, int n, int n_out, double alpha, double one_minus_alpha,
                                                                    double threshold, float *state, float *filt, int32_t *likely,
                                                                    int32_t *spotted, edsg_fsm_stage_t fs)
{
	const int t = threadIdx.x;
	if (t < n_out)
	{
		float y = state[t];
		for (int i = 0; i < n; i++)
		{
			/* as ed_stream_filter_kernel: the compiler's default contraction would fuse these into one v_fma_f64, a different double in
			 * the last place (the Cortex-M4 rounds each operation) */
#pragma clang fp contract(off)
			const double a = alpha * (double)y;
			const double b = one_minus_alpha * (double)x[(size_t)i * n_out + t];
			y = (float)(a + b);
			filt[(size_t)i * n_out + t] = y;
		}
		state[t] = y;
	}
	__syncthreads();
	for (int i = t; i < n; i += 256)
	{
		const float *row = filt + (size_t)i * n_out;
		float best = row[0];
		int idx = 0;
		for (int c = 1; c < n_out; c++)
			if (best < row[c]) { best = row[c]; idx = c; }
		likely[i] = idx;
		spotted[i] = ((double)best > threshold) ? idx : -1;
	}
	if (!fs.fsm) return;
	__syncthreads();
	if (t == 0)
	{
		edison_fsm m = *fs.fsm;
		for (int i = 0; i < n; i++)
			fs.states[i] = ed_fsm_step_core(&m, spotted[i] >= 0, (uint32_t)likely[i], fs.dt_us, &fs.roles);
		*fs.fsm = m;
		if (fs.copy) *fs.copy = m;
	}
}

int ed_launch_stream_shift(hipStream_t q, int16_t *audio, int64_t a_src, int tail, void *feat, int64_t f_src, int feat_bytes)
{
	hipLaunchKernelGGL(ed_stream_geom_shift_kernel, dim3(1), dim3(256), 0, q, audio, a_src, tail, (int8_t *)feat, f_src, feat_bytes);
	return (int)hipGetLastError();
}

int ed_launch_stream_filter_f32(hipStream_t q, const float *x, int n, int n_out, double alpha, double one_minus_alpha, double threshold,
                                float *state, float *filt, int32_t *likely, int32_t *spotted, edsg_fsm_stage_t fs)
{
	hipLaunchKernelGGL(ed_stream_geom_filter_kernel<float>, dim3(1), dim3(256), 0, q, x, n, n_out, alpha, one_minus_alpha, threshold, state,
	                   filt, likely, spotted, fs);
	return (int)hipGetLastError();
}

/* Work the stream left unsynchronised on another HIP stream must be behind us before q touches the stream's state. */
static int order_after(edison_stream_geom *s, hipStream_t q)
{
	if (!s->q_pending || s->q_last == q) return EDISON_OK;
	if (hipEventRecord(s->ev, s->q_last) == hipSuccess) ED_HIP(s->ctx, hipStreamWaitEvent(q, s->ev, 0));
	else (void)hipGetLastError(); /* the caller destroyed that stream (which drains it) */
	s->q_pending = 0;
	return EDISON_OK;
}

/* the network on the kernel edison_net_batch_dev picks for the loaded graph, on hipStream q */
static int net_on(edison_ctx *ctx, hipStream_t q, const int8_t *in, int n, int64_t stride, int8_t *logits, int8_t *softmax, int32_t *argmax)
{
	const char *fg_ = getenv("EDISON_NET_FORCE_GENERAL"); /* read per call, as edison_net_batch_dev does */
	const int force_general = fg_ ? atoi(fg_) : 0;
	if (ctx->fast_model && !force_general) return ed_ctx_kws_cnn_launch_on(ctx, q, in, n, stride, logits, softmax, argmax);
	return ed_launch_result(ctx, ed_ctx_net_launch_on(ctx, q, in, n, stride, logits, softmax, argmax), "network kernel");
}

/* Enqueue the device work of a push of n frames whose samples are already at d_audio + pos * hop + tail: MFCC, network, filter.
 * The outputs go where they are told (NULL: not written); the filter reads its input from `fin` and writes the stream's block. */
static int enqueue_push(edison_stream_geom *s, hipStream_t q, int n, int8_t *logits, int8_t *softmax, int32_t *argmax, const int8_t *fin,
                        unsigned char *fout)
{
	edison_ctx *ctx = s->ctx;
	int8_t *win = s->d_feat + (size_t)s->pos * s->nm; /* F - 1 rows of history, then the n new rows */
	ed_geom_args_t a = s->margs;
	a.audio = s->d_audio + (size_t)s->pos * s->hop;
	a.frames_per_utt = n;
	a.n_frames = n;
	a.feat = win + (size_t)(s->F - 1) * s->nm;
	{ const int e = ed_launch_mfcc_geom(&a, ctx->n_cu, q); if (e != 0) return ed_launch_result(ctx, e, "MFCC geometry kernel"); }
	{ const int r = net_on(ctx, q, win, n, s->nm, logits, softmax, argmax); if (r != EDISON_OK) return r; }
	if (s->filter)
	{
		edsg_fsm_stage_t fs;
		memset(&fs, 0, sizeof(fs));
		if (s->fsm)
		{
			fs.fsm = s->d_fsm; fs.states = (int32_t *)(fout + s->off_states); fs.copy = (edison_fsm *)(fout + s->off_fsm);
			fs.dt_us = s->dt_us; fs.roles = s->roles;
		}
		hipLaunchKernelGGL(ed_stream_geom_filter_kernel<int8_t>, dim3(1), dim3(256), 0, q, fin, n, s->n_out, s->alpha, s->one_minus_alpha, s->threshold,
		                   s->d_state, (float *)(fout + s->off_filt), (int32_t *)(fout + s->off_likely), (int32_t *)(fout + s->off_spotted), fs);
		if (hipGetLastError() != hipSuccess) return ed_set_err(ctx, EDISON_E_RUNTIME, "stream_geom: filter launch failed");
	}
	s->pos += n;
	return EDISON_OK;
}

/* Before a push of n frames: the history to the front when the push would run past the end of the buffers. */
static int make_room(edison_stream_geom *s, hipStream_t q, int n)
{
	if (s->pos + n <= s->slots * s->chunk || s->pos == 0) return EDISON_OK;
	const int e = ed_launch_stream_shift(q, s->d_audio, (int64_t)s->pos * s->hop, s->tail, s->d_feat, (int64_t)s->pos * s->nm, (s->F - 1) * s->nm);
	s->pos = 0;
	return e == 0 ? EDISON_OK : ed_set_err(s->ctx, EDISON_E_RUNTIME, "stream_geom: shift launch failed");
}

static int check_push(edison_stream_geom *s, const int16_t *samples)
{
	if (!s || !samples) return EDISON_E_ARGUMENT;
	if (s->model_epoch != s->ctx->model_epoch)
		return ed_set_err(s->ctx, EDISON_E_ARGUMENT, "stream_geom: the model was reloaded after this stream was created; create a new stream");
	return EDISON_OK;
}

extern "C" void edison_stream_geom_default_opts(edison_stream_geom_opts *o)
{
	if (!o) return;
	memset(o, 0, sizeof(*o));
	o->chunk_frames = 1;
	o->filter = 0;
	o->fsm = 0;
	o->filter_alpha = 0.9;   /* edison_stream_default_opts' values: NET_OUT_MOVING_AVG_ALPHA (app.c:38) */
	o->true_threshold = 0.5; /* TRUE_THRESHOLD (app.c:34) */
}

extern "C" void edison_stream_geom_destroy(edison_stream_geom *s)
{
	if (!s) return;
	if (s->own && s->ev) (void)order_after(s, s->own);
	if (s->own) (void)hipStreamSynchronize(s->own);
	if (s->tab.d) (void)hipFree(s->tab.d);
	if (s->d_audio) (void)hipFree(s->d_audio);
	if (s->d_feat) (void)hipFree(s->d_feat);
	if (s->d_out) (void)hipFree(s->d_out);
	if (s->d_state) (void)hipFree(s->d_state);
	if (s->d_fsm) (void)hipFree(s->d_fsm);
	if (s->h_in) (void)hipHostFree(s->h_in);
	if (s->h_out) (void)hipHostFree(s->h_out);
	if (s->ev) (void)hipEventDestroy(s->ev);
	if (s->own) (void)hipStreamDestroy(s->own);
	delete s;
}

extern "C" int edison_stream_geom_reset(edison_stream_geom *s)
{
	if (!s) return EDISON_E_ARGUMENT;
	edison_ctx *ctx = s->ctx;
	{ const int r = order_after(s, s->own); if (r != EDISON_OK) return r; }
	s->pos = 0;
	if (s->tail) ED_HIP(ctx, hipMemsetAsync(s->d_audio, 0, sizeof(int16_t) * (size_t)s->tail, s->own));
	if (s->F > 1) ED_HIP(ctx, hipMemsetAsync(s->d_feat, 0, (size_t)(s->F - 1) * s->nm, s->own));
	ED_HIP(ctx, hipMemsetAsync(s->d_out, 0, s->out_bytes, s->own));
	if (s->filter) ED_HIP(ctx, hipMemsetAsync(s->d_state, 0, sizeof(float) * (size_t)s->n_out, s->own));
	if (s->fsm)
	{
		edison_fsm start;
		edison_fsm_init(&start); /* EDI_RESET, as the firmware enters its continuous loop (app.c:288-300) */
		ED_HIP(ctx, hipMemcpyAsync(s->d_fsm, &start, sizeof(start), hipMemcpyHostToDevice, s->own));
	}
	ED_HIP(ctx, hipStreamSynchronize(s->own));
	memset(s->h_out, 0, s->out_bytes);
	s->q_pending = 0;
	s->last_n = s->chunk;
	s->last_staged = 0;
	s->frames_seen = 0;
	return EDISON_OK;
}

extern "C" int edison_stream_geom_create(edison_ctx *ctx, const edison_kws_geom *g, const edison_stream_geom_opts *o, edison_stream_geom **out)
{
	if (!ctx || !g || !o || !out) return EDISON_E_ARGUMENT;
	*out = NULL;
	int F = 0;
	{ const int r = ed_kws_geom_check(ctx, g, &F); if (r != EDISON_OK) return r; }
	if (!ctx->have_model) return ed_set_err(ctx, EDISON_E_NO_MODEL, "no CNN model loaded (edison_model_load)");
	if ((int64_t)F * g->num_mfcc != ctx->net.in_n)
	{
		snprintf(ctx->err, sizeof(ctx->err), "stream_geom: frame_count x num_mfcc = %lld features, the graph's input in_h x in_w x in_c = %d",
		         (long long)F * g->num_mfcc, ctx->net.in_n);
		return EDISON_E_SIZE;
	}
	if (o->chunk_frames < 1) return ed_set_err(ctx, EDISON_E_ARGUMENT, "stream_geom: chunk_frames >= 1");
	/* positions and sample counts are ints in places (pos * hop, kernel arguments): as edison_stream_create_ex */
	if ((int64_t)o->chunk_frames * g->frame_step >= ((int64_t)1 << 30))
		return ed_set_err(ctx, EDISON_E_SIZE, "stream_geom: chunk_frames x frame_step must stay below 2^30 samples per push");
	if (o->fsm && !o->filter) return ed_set_err(ctx, EDISON_E_ARGUMENT, "stream_geom: the state machine (fsm) works on the filtered outputs: filter = 1 too");
	if (o->filter && !(o->filter_alpha >= 0.0 && o->filter_alpha <= 1.0))
		return ed_set_err(ctx, EDISON_E_ARGUMENT, "stream_geom: filter_alpha must be within [0, 1]");
	if (o->filter && ctx->net.out_n > EDSG_FILTER_MAX_OUT)
		return ed_set_err(ctx, EDISON_E_NO_IMPL, "stream_geom: the output filter serves graphs of at most 256 outputs");
	if (o->fsm && ctx->net.out_n != EDISON_NET_OUT)
		return ed_set_err(ctx, EDISON_E_NO_IMPL, "stream_geom: the state machine needs a graph with 10 outputs (the keyword list its roles index)");

	edison_stream_geom *s = new (std::nothrow) edison_stream_geom();
	if (!s) return ed_set_err(ctx, EDISON_E_NO_MEMORY, "host allocation failed");
	s->ctx = ctx;
	s->F = F; s->nm = g->num_mfcc; s->hop = g->frame_step; s->chunk = o->chunk_frames;
	s->tail = g->frame_len > g->frame_step ? g->frame_len - g->frame_step : 0;
	s->n_out = ctx->net.out_n; s->has_softmax = ctx->net.has_softmax; s->in_n = ctx->net.in_n;
	s->filter = o->filter ? 1 : 0;
	s->fsm = o->fsm ? 1 : 0;
	s->alpha = o->filter_alpha;
	s->one_minus_alpha = 1.0 - o->filter_alpha; /* folded in double, as the firmware's (1.0-NET_OUT_MOVING_AVG_ALPHA) */
	s->threshold = o->true_threshold;
	s->dt_us = (uint32_t)floor((double)g->frame_step * 1e6 / g->sample_rate);
	edison_fsm_roles(&s->roles.wake_idx, &s->roles.loc_mask, &s->roles.val_mask);
	s->model_epoch = ctx->model_epoch;
	s->last_n = s->chunk;

	hipError_t e = hipSetDevice(ctx->device);
	if (e != hipSuccess) { delete s; ED_HIP(ctx, e); }
	{ const int r = ed_geom_tables_build(ctx, g, &s->tab); if (r != EDISON_OK) { edison_stream_geom_destroy(s); return r; } }
	s->margs = s->tab.tmpl;
	s->margs.utt_stride = 0;
	s->margs.frame_step = g->frame_step;
	s->margs.take_log = (g->variant & 0xff) == EDISON_MFCC_A || (g->variant & EDISON_MFCC_USE_LOG);
	s->margs.feat_scale = (float)g->net_input_scale;

	e = hipStreamCreateWithFlags(&s->own, hipStreamNonBlocking);
	if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev, hipEventDisableTiming);
	/* eight pushes of room while that stays below 64 MB of samples, else one (then every push after the first shifts) */
	const size_t c = (size_t)s->chunk, push_samples = c * (size_t)s->hop;
	s->slots = push_samples * sizeof(int16_t) * 8 <= ((size_t)64 << 20) ? 8 : 1;
	if (e == hipSuccess) e = hipMalloc((void **)&s->d_audio, sizeof(int16_t) * ((size_t)s->tail + (size_t)s->slots * push_samples) + 64);
	if (e == hipSuccess) e = hipMalloc((void **)&s->d_feat, ((size_t)(s->F - 1) + (size_t)s->slots * c) * s->nm + 64);
	{
		const size_t no = (size_t)s->n_out;
		size_t off = c * no;                                                   /* logits at 0 */
		s->off_soft = off; off += s->has_softmax ? c * no : 0;
		off = (off + 15) & ~(size_t)15; s->off_argmax = off; off += c * sizeof(int32_t);
		off = (off + 15) & ~(size_t)15; s->off_filt = off; off += s->filter ? c * no * sizeof(float) : 0;
		s->off_likely = off; off += s->filter ? c * sizeof(int32_t) : 0;
		s->off_spotted = off; off += s->filter ? c * sizeof(int32_t) : 0;
		s->off_states = off; off += s->fsm ? c * sizeof(int32_t) : 0;
		off = (off + 15) & ~(size_t)15; s->off_fsm = off; off += s->fsm ? sizeof(edison_fsm) : 0;
		s->out_bytes = off;
	}
	if (e == hipSuccess) e = hipMalloc((void **)&s->d_out, s->out_bytes);
	if (e == hipSuccess) e = hipHostMalloc((void **)&s->h_out, s->out_bytes, hipHostMallocDefault);
	if (e == hipSuccess) e = hipHostMalloc((void **)&s->h_in, sizeof(int16_t) * push_samples, hipHostMallocDefault);
	if (e == hipSuccess && s->filter) e = hipMalloc((void **)&s->d_state, sizeof(float) * (size_t)s->n_out);
	if (e == hipSuccess && s->fsm) e = hipMalloc((void **)&s->d_fsm, sizeof(edison_fsm));
	if (e != hipSuccess)
	{
		edison_stream_geom_destroy(s);
		return ed_set_err(ctx, e == hipErrorOutOfMemory ? EDISON_E_NO_MEMORY : EDISON_E_RUNTIME, "stream_geom: allocation failed");
	}
	const int r = edison_stream_geom_reset(s);
	if (r != EDISON_OK) { edison_stream_geom_destroy(s); return r; }
	*out = s;
	return EDISON_OK;
}

extern "C" int edison_stream_geom_push_n_dev(edison_stream_geom *s, const int16_t *samples, int n_frames, int8_t *logits, int8_t *softmax,
                                             int32_t *argmax)
{
	{ const int r = check_push(s, samples); if (r != EDISON_OK) return r; }
	edison_ctx *ctx = s->ctx;
	if (n_frames < 1 || n_frames > s->chunk) return ed_set_err(ctx, EDISON_E_ARGUMENT, "stream_geom: n_frames must be 1 .. chunk_frames");
	hipStream_t q = ctx->stream;
	{ const int r = order_after(s, q); if (r != EDISON_OK) return r; }
	{ const int r = make_room(s, q, n_frames); if (r != EDISON_OK) return r; }
	ED_HIP(ctx, hipMemcpyAsync(s->d_audio + (size_t)s->pos * s->hop + s->tail, samples, sizeof(int16_t) * (size_t)n_frames * s->hop,
	                           hipMemcpyDeviceToDevice, q));
	int8_t *so = s->has_softmax ? softmax : NULL;
	/* the filter's input: the caller's softmax (or logits for a graph without Softmax) where given, else the stream's block */
	const int8_t *fin = NULL;
	if (s->filter)
	{
		int8_t *&src = s->has_softmax ? so : logits;
		if (!src) src = (int8_t *)(s->d_out + (s->has_softmax ? s->off_soft : 0));
		fin = src;
	}
	{ const int r = enqueue_push(s, q, n_frames, logits, so, argmax, fin, s->d_out); if (r != EDISON_OK) return r; }
	s->q_last = q;
	s->q_pending = 1;
	s->last_n = n_frames;
	s->last_staged = 0;
	s->frames_seen += n_frames;
	return EDISON_OK;
}

extern "C" int edison_stream_geom_push_dev(edison_stream_geom *s, const int16_t *samples, int8_t *logits, int8_t *softmax, int32_t *argmax)
{
	return edison_stream_geom_push_n_dev(s, samples, s ? s->chunk : 0, logits, softmax, argmax);
}

/* host pointers: one upload from pinned memory, the same launches on the private stream, one download of the output block, one wait */
extern "C" int edison_stream_geom_push(edison_stream_geom *s, const int16_t *samples, int8_t *logits, int8_t *softmax, int32_t *argmax)
{
	{ const int r = check_push(s, samples); if (r != EDISON_OK) return r; }
	edison_ctx *ctx = s->ctx;
	const size_t c = (size_t)s->chunk, no = (size_t)s->n_out, nnew = c * (size_t)s->hop;
	hipStream_t q = s->own;
	{ const int r = order_after(s, q); if (r != EDISON_OK) return r; }
	{ const int r = make_room(s, q, s->chunk); if (r != EDISON_OK) return r; }
	memcpy(s->h_in, samples, sizeof(int16_t) * nnew);
	ED_HIP(ctx, hipMemcpyAsync(s->d_audio + (size_t)s->pos * s->hop + s->tail, s->h_in, sizeof(int16_t) * nnew, hipMemcpyHostToDevice, q));
	int8_t *dl = (int8_t *)s->d_out, *ds = s->has_softmax ? (int8_t *)(s->d_out + s->off_soft) : NULL;
	{
		const int r = enqueue_push(s, q, s->chunk, dl, ds, (int32_t *)(s->d_out + s->off_argmax), s->has_softmax ? ds : dl, s->d_out);
		if (r != EDISON_OK) return r;
	}
	ED_HIP(ctx, hipMemcpyAsync(s->h_out, s->d_out, s->out_bytes, hipMemcpyDeviceToHost, q));
	ED_HIP(ctx, hipStreamSynchronize(q));
	if (logits) memcpy(logits, s->h_out, c * no);
	if (softmax && s->has_softmax) memcpy(softmax, s->h_out + s->off_soft, c * no);
	if (argmax) memcpy(argmax, s->h_out + s->off_argmax, c * sizeof(int32_t));
	s->q_pending = 0;
	s->last_n = s->chunk;
	s->last_staged = 1;
	s->frames_seen += s->chunk;
	return EDISON_OK;
}

extern "C" int64_t edison_stream_geom_frames_seen(const edison_stream_geom *s) { return s ? s->frames_seen : -1; }

/* Copy `count` pieces of the last push's output block to the caller: from h_out after a host push, else from d_out on the stream the
 * work went to (host = 1: synchronously; host = 0: ordered on the context's stream). */
struct edsg_piece { void *dst; size_t off, bytes; };
static int copy_out(edison_stream_geom *s, const edsg_piece *p, int count, int host)
{
	edison_ctx *ctx = s->ctx;
	if (host && s->last_staged)
	{
		for (int i = 0; i < count; i++)
			if (p[i].dst) memcpy(p[i].dst, s->h_out + p[i].off, p[i].bytes);
		return EDISON_OK;
	}
	hipStream_t q = host ? s->own : ctx->stream;
	{ const int r = order_after(s, q); if (r != EDISON_OK) return r; }
	for (int i = 0; i < count; i++)
		if (p[i].dst)
			ED_HIP(ctx, hipMemcpyAsync(p[i].dst, s->d_out + p[i].off, p[i].bytes, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, q));
	if (host)
	{
		ED_HIP(ctx, hipStreamSynchronize(q));
		s->q_pending = 0;
	}
	else
	{
		s->q_last = q;
		s->q_pending = 1;
	}
	return EDISON_OK;
}

static int filtered_out(edison_stream_geom *s, float *filt, int32_t *likely, int32_t *spotted, int host)
{
	if (!s) return EDISON_E_ARGUMENT;
	if (!s->filter) return ed_set_err(s->ctx, EDISON_E_ARGUMENT, "stream_geom: created without the output filter");
	const size_t n = (size_t)s->last_n;
	const edsg_piece p[3] = {{filt, s->off_filt, n * (size_t)s->n_out * sizeof(float)}, {likely, s->off_likely, n * sizeof(int32_t)},
	                         {spotted, s->off_spotted, n * sizeof(int32_t)}};
	return copy_out(s, p, 3, host);
}

static int fsm_out(edison_stream_geom *s, edison_fsm *fsm, int32_t *states, int host)
{
	if (!s) return EDISON_E_ARGUMENT;
	if (!s->fsm) return ed_set_err(s->ctx, EDISON_E_ARGUMENT, "stream_geom: created without the state machine (opts.fsm)");
	const edsg_piece p[2] = {{states, s->off_states, (size_t)s->last_n * sizeof(int32_t)}, {fsm, s->off_fsm, sizeof(edison_fsm)}};
	return copy_out(s, p, host ? 2 : 1, host);
}

extern "C" int edison_stream_geom_filtered(edison_stream_geom *s, float *filt, int32_t *likely, int32_t *spotted)
{
	return filtered_out(s, filt, likely, spotted, 1);
}

extern "C" int edison_stream_geom_filtered_dev(edison_stream_geom *s, float *filt, int32_t *likely, int32_t *spotted)
{
	return filtered_out(s, filt, likely, spotted, 0);
}

extern "C" int edison_stream_geom_fsm(edison_stream_geom *s, edison_fsm *fsm, int32_t *states) { return fsm_out(s, fsm, states, 1); }
extern "C" int edison_stream_geom_fsm_dev(edison_stream_geom *s, int32_t *states) { return fsm_out(s, NULL, states, 0); }
