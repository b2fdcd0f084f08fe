/*
 * edison_stream_float.hip -- continuous mode for the float32 X-CUBE-AI network (include/edison_hip.h, edison_stream_float_*): the
 * continuous counterpart of edison_kws_float_batch*, as edison_stream_geom.hip is the one of edison_kws_geom_batch*. It is the
 * firmware's loop for NET_TYPE_CUBE (app.c:288-371, 630-719). A push of n new frames runs
 *
 *     [shift, only when the push would not fit] -> feature rows -> network over the n overlapping windows -> [filter (+ edisonFSM)]
 *
 * The feature rows come from ed_mfcc_geom_fnet_kernel in the host flow (q15 = 0): float64 MFCC -> (float)y * net_input_scale -> clip,
 * in one launch. In the firmware flow (q15 = 1) they come from the variant-C kernel's float output.
 *
 * Device state: two sliding buffers `slots` pushes long,
 *     d_audio  [T + slots * chunk * hop] int16             T = max(0, frame_len - hop) samples of history, then the new samples
 *     d_feat   [F - 1 + slots * chunk][num_mfcc] float32   F - 1 rows of history, then the new rows
 * whose history starts at frame `pos`. Window i of a push is rows pos + i .. pos + i + F - 1. The network kernel reads it in place at
 * an input stride of num_mfcc floats, so nothing is copied. When the next push would run past the end, the shift kernel of
 * edison_stream_geom.hip first moves the history back to the front (a byte move: 4 (F - 1) num_mfcc bytes of rows). The filter is that
 * file's kernel too, instantiated for float inputs. The stream owns its own geometry tables.
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
#include "fnet.h"
#include "mfcc_geom.h"

struct edison_stream_float
{
	edison_ctx *ctx;
	int F, nm, hop, tail, chunk;   /* frames per window, coefficients per row, frame_step, T history samples, frames per push */
	int n_out;
	int q15;
	float scale, lo, hi;           /* the host flow's (float)net_input_scale and clip range */
	int filter, fsm;
	double alpha, one_minus_alpha, threshold;
	ed_geom_cache tab;             /* this stream's own tables (host flow only; edison_kws_geom.hip builds them) */
	ed_geom_args_t margs;          /* tab.tmpl with the per-geometry fields; audio and the frame counts are set per push */
	int slots, pos;                /* buffers of `slots` pushes; the history starts at frame pos */
	int16_t *d_audio;
	float *d_feat;
	/* every output of a push in one block (device d_out, pinned h_out), so that a host push downloads once */
	unsigned char *d_out, *h_out;
	size_t off_probs, off_argmax, off_filt, off_likely, off_spotted, off_states, off_fsm, out_bytes;
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
	int fnet_epoch;
};

/* Work the stream left unsynchronised on another HIP stream must be behind us before q touches the stream's state. */
static int order_after(edison_stream_float *s, hipStream_t q)
{
	if (!s->q_pending || s->q_last == q) return EDISON_OK;
	if (hipEventRecord(s->ev, s->q_last) == hipSuccess) ED_HIP(s->ctx, hipStreamWaitEvent(q, s->ev, 0));
	else (void)hipGetLastError(); /* the caller destroyed that stream (which drains it) */
	s->q_pending = 0;
	return EDISON_OK;
}

/* Enqueue the device work of a push of n frames whose samples are already at d_audio + pos * hop + tail: feature rows, network, filter.
 * The outputs go where they are told (NULL: not written); the filter reads its input from `fin` and writes the stream's block. */
static int enqueue_push(edison_stream_float *s, hipStream_t q, int n, float *logits, float *probs, int32_t *argmax, const float *fin,
                        unsigned char *fout)
{
	edison_ctx *ctx = s->ctx;
	float *win = s->d_feat + (size_t)s->pos * s->nm; /* F - 1 rows of history, then the n new rows */
	float *rows = win + (size_t)(s->F - 1) * s->nm;
	const int16_t *au = s->d_audio + (size_t)s->pos * s->hop;
	if (s->q15)
	{
		/* variant C int16 -> (float), no scale, no clip (app.c:675-683): the Q15 kernel's float output, frames hop samples apart */
		const int r = ed_ctx_mfcc_q15_launch_on(ctx, q, au, n, n, 0, s->hop, s->nm, NULL, rows, NULL, 0, NULL, NULL, NULL);
		if (r != EDISON_OK) return r;
	}
	else
	{
		ed_geom_args_t a = s->margs;
		a.audio = au;
		a.frames_per_utt = n;
		a.n_frames = n;
		const int e = ed_launch_mfcc_geom_fnet(&a, rows, s->scale, s->lo, s->hi, ctx->n_cu, q);
		if (e != 0) return ed_launch_result(ctx, e, "MFCC geometry kernel (float network input)");
	}
	{
		const int e = ed_launch_fnet(ed_ctx_fnet_plan(ctx), win, s->nm, n, logits, probs, argmax, NULL, q);
		if (e != 0) return ed_launch_result(ctx, e, "float network kernel");
	}
	if (s->filter)
	{
		edsg_fsm_stage_t fs;
		memset(&fs, 0, sizeof(fs));
		if (s->fsm)
		{
			fs.fsm = s->d_fsm; fs.states = (int32_t *)(fout + s->off_states); fs.copy = (edison_fsm *)(fout + s->off_fsm);
			fs.dt_us = s->dt_us; fs.roles = s->roles;
		}
		const int e = ed_launch_stream_filter_f32(q, fin, n, s->n_out, s->alpha, s->one_minus_alpha, s->threshold, s->d_state,
		                                          (float *)(fout + s->off_filt), (int32_t *)(fout + s->off_likely),
		                                          (int32_t *)(fout + s->off_spotted), fs);
		if (e != 0) return ed_set_err(ctx, EDISON_E_RUNTIME, "stream_float: filter launch failed");
	}
	s->pos += n;
	return EDISON_OK;
}

/* Before a push of n frames: the history to the front when the push would run past the end of the buffers. */
static int make_room(edison_stream_float *s, hipStream_t q, int n)
{
	if (s->pos + n <= s->slots * s->chunk || s->pos == 0) return EDISON_OK;
	const int e = ed_launch_stream_shift(q, s->d_audio, (int64_t)s->pos * s->hop, s->tail, s->d_feat, (int64_t)s->pos * s->nm * (int64_t)sizeof(float),
	                                     (int)sizeof(float) * (s->F - 1) * s->nm);
	s->pos = 0;
	return e == 0 ? EDISON_OK : ed_set_err(s->ctx, EDISON_E_RUNTIME, "stream_float: shift launch failed");
}

static int check_push(edison_stream_float *s, const int16_t *samples)
{
	if (!s || !samples) return EDISON_E_ARGUMENT;
	if (s->fnet_epoch != s->ctx->fnet_epoch || !s->ctx->fnet)
		return ed_set_err(s->ctx, EDISON_E_ARGUMENT, "stream_float: the float network was reloaded after this stream was created; create a new stream");
	return EDISON_OK;
}

extern "C" void edison_stream_float_default_opts(edison_stream_float_opts *o)
{
	if (!o) return;
	memset(o, 0, sizeof(*o));
	o->chunk_frames = 1;
	o->q15 = 0;
	o->clip_lo = -32768.0f; /* audio/config.py's net_input_clip_min / _max, as Context.kws_float */
	o->clip_hi = 32767.0f;
	o->filter = 0;
	o->fsm = 0;
	o->filter_alpha = 0.5;   /* NET_OUT_MOVING_AVG_ALPHA of the Cube build (app.c:35-36) */
	o->true_threshold = 0.5; /* TRUE_THRESHOLD (app.c:34) */
}

extern "C" void edison_stream_float_destroy(edison_stream_float *s)
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

extern "C" int edison_stream_float_reset(edison_stream_float *s)
{
	if (!s) return EDISON_E_ARGUMENT;
	edison_ctx *ctx = s->ctx;
	{ const int r = order_after(s, s->own); if (r != EDISON_OK) return r; }
	s->pos = 0;
	if (s->tail) ED_HIP(ctx, hipMemsetAsync(s->d_audio, 0, sizeof(int16_t) * (size_t)s->tail, s->own));
	if (s->F > 1) ED_HIP(ctx, hipMemsetAsync(s->d_feat, 0, sizeof(float) * (size_t)(s->F - 1) * s->nm, s->own)); /* +0.0f rows */
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

extern "C" int edison_stream_float_create(edison_ctx *ctx, const edison_kws_geom *g, const edison_stream_float_opts *o, edison_stream_float **out)
{
	if (!ctx || !g || !o || !out) return EDISON_E_ARGUMENT;
	*out = NULL;
	if (o->q15 != 0 && o->q15 != 1) return ed_set_err(ctx, EDISON_E_ARGUMENT, "stream_float: q15 is 0 or 1");
	int F = 0;
	/* the batch call's checks: clip range, geometry (q15 = 1: the shipped framing), a float network loaded, F * num_mfcc = its input */
	{ const int r = ed_kws_float_geom_check(ctx, g, o->q15, o->clip_lo, o->clip_hi, &F); if (r != EDISON_OK) return r; }
	if (o->q15 && !ctx->d_q15)
	{
		snprintf(ctx->err, sizeof(ctx->err), "stream_float: MFCC variant C is not available for the configured filterbank: %s",
		         ctx->q15_err[0] ? ctx->q15_err : "tables not built");
		return EDISON_E_NO_IMPL;
	}
	const int n_out = ed_ctx_fnet_plan(ctx)->n_out;
	if (o->chunk_frames < 1) return ed_set_err(ctx, EDISON_E_ARGUMENT, "stream_float: chunk_frames >= 1");
	/* positions and sample counts are ints in places (pos * hop, kernel arguments): as edison_stream_geom_create */
	if ((int64_t)o->chunk_frames * g->frame_step >= ((int64_t)1 << 30))
		return ed_set_err(ctx, EDISON_E_SIZE, "stream_float: chunk_frames x frame_step must stay below 2^30 samples per push");
	if (o->fsm && !o->filter) return ed_set_err(ctx, EDISON_E_ARGUMENT, "stream_float: the state machine (fsm) works on the filtered outputs: filter = 1 too");
	if (o->filter && !(o->filter_alpha >= 0.0 && o->filter_alpha <= 1.0))
		return ed_set_err(ctx, EDISON_E_ARGUMENT, "stream_float: filter_alpha must be within [0, 1]");
	if (o->filter && n_out > EDSG_FILTER_MAX_OUT)
		return ed_set_err(ctx, EDISON_E_NO_IMPL, "stream_float: the output filter serves networks of at most 256 outputs");
	if (o->fsm && n_out != EDISON_NET_OUT)
		return ed_set_err(ctx, EDISON_E_NO_IMPL, "stream_float: the state machine needs a network with 10 outputs (the keyword list its roles index)");

	edison_stream_float *s = new (std::nothrow) edison_stream_float();
	if (!s) return ed_set_err(ctx, EDISON_E_NO_MEMORY, "host allocation failed");
	s->ctx = ctx;
	s->F = F; s->nm = g->num_mfcc; s->hop = g->frame_step; s->chunk = o->chunk_frames;
	s->tail = g->frame_len > g->frame_step ? g->frame_len - g->frame_step : 0;
	s->n_out = n_out;
	s->q15 = o->q15;
	s->scale = (float)g->net_input_scale;
	s->lo = o->clip_lo;
	s->hi = o->clip_hi;
	s->filter = o->filter ? 1 : 0;
	s->fsm = o->fsm ? 1 : 0;
	s->alpha = o->filter_alpha;
	s->one_minus_alpha = 1.0 - o->filter_alpha; /* folded in double, as the firmware's (1.0-NET_OUT_MOVING_AVG_ALPHA) */
	s->threshold = o->true_threshold;
	s->dt_us = (uint32_t)floor((double)g->frame_step * 1e6 / g->sample_rate);
	edison_fsm_roles(&s->roles.wake_idx, &s->roles.loc_mask, &s->roles.val_mask);
	s->fnet_epoch = ctx->fnet_epoch;
	s->last_n = s->chunk;

	hipError_t e = hipSetDevice(ctx->device);
	if (e != hipSuccess) { delete s; ED_HIP(ctx, e); }
	if (!s->q15)
	{
		{ const int r = ed_geom_tables_build(ctx, g, &s->tab); if (r != EDISON_OK) { edison_stream_float_destroy(s); return r; } }
		s->margs = s->tab.tmpl;
		s->margs.utt_stride = 0;
		s->margs.frame_step = g->frame_step;
		s->margs.take_log = (g->variant & 0xff) == EDISON_MFCC_A || (g->variant & EDISON_MFCC_USE_LOG);
		s->margs.feat = NULL;
	}

	e = hipStreamCreateWithFlags(&s->own, hipStreamNonBlocking);
	if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev, hipEventDisableTiming);
	/* eight pushes of room while that stays below 64 MB of samples, else one (then every push after the first shifts) */
	const size_t c = (size_t)s->chunk, push_samples = c * (size_t)s->hop;
	s->slots = push_samples * sizeof(int16_t) * 8 <= ((size_t)64 << 20) ? 8 : 1;
	if (e == hipSuccess) e = hipMalloc((void **)&s->d_audio, sizeof(int16_t) * ((size_t)s->tail + (size_t)s->slots * push_samples) + 64);
	if (e == hipSuccess) e = hipMalloc((void **)&s->d_feat, sizeof(float) * ((size_t)(s->F - 1) + (size_t)s->slots * c) * s->nm + 64);
	{
		const size_t no = (size_t)s->n_out, fb = c * no * sizeof(float);
		size_t off = fb;                                                       /* logits at 0 */
		s->off_probs = off; off += fb;
		s->off_argmax = off; off += c * sizeof(int32_t);
		off = (off + 15) & ~(size_t)15; s->off_filt = off; off += s->filter ? fb : 0;
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
		edison_stream_float_destroy(s);
		return ed_set_err(ctx, e == hipErrorOutOfMemory ? EDISON_E_NO_MEMORY : EDISON_E_RUNTIME, "stream_float: allocation failed");
	}
	const int r = edison_stream_float_reset(s);
	if (r != EDISON_OK) { edison_stream_float_destroy(s); return r; }
	*out = s;
	return EDISON_OK;
}

extern "C" int edison_stream_float_push_n_dev(edison_stream_float *s, const int16_t *samples, int n_frames, float *logits, float *probs,
                                              int32_t *argmax)
{
	{ const int r = check_push(s, samples); if (r != EDISON_OK) return r; }
	edison_ctx *ctx = s->ctx;
	if (n_frames < 1 || n_frames > s->chunk) return ed_set_err(ctx, EDISON_E_ARGUMENT, "stream_float: n_frames must be 1 .. chunk_frames");
	hipStream_t q = ctx->stream;
	{ const int r = order_after(s, q); if (r != EDISON_OK) return r; }
	{ const int r = make_room(s, q, n_frames); if (r != EDISON_OK) return r; }
	ED_HIP(ctx, hipMemcpyAsync(s->d_audio + (size_t)s->pos * s->hop + s->tail, samples, sizeof(int16_t) * (size_t)n_frames * s->hop,
	                           hipMemcpyDeviceToDevice, q));
	/* the filter's input: the caller's probs where given, else the stream's block */
	if (s->filter && !probs) probs = (float *)(s->d_out + s->off_probs);
	{ const int r = enqueue_push(s, q, n_frames, logits, probs, argmax, probs, s->d_out); if (r != EDISON_OK) return r; }
	s->q_last = q;
	s->q_pending = 1;
	s->last_n = n_frames;
	s->last_staged = 0;
	s->frames_seen += n_frames;
	return EDISON_OK;
}

extern "C" int edison_stream_float_push_dev(edison_stream_float *s, const int16_t *samples, float *logits, float *probs, int32_t *argmax)
{
	return edison_stream_float_push_n_dev(s, samples, s ? s->chunk : 0, logits, probs, argmax);
}

/* host pointers: one upload from pinned memory, the same launches on the private stream, one download of the output block, one wait */
extern "C" int edison_stream_float_push(edison_stream_float *s, const int16_t *samples, float *logits, float *probs, int32_t *argmax)
{
	{ const int r = check_push(s, samples); if (r != EDISON_OK) return r; }
	edison_ctx *ctx = s->ctx;
	const size_t c = (size_t)s->chunk, fb = c * (size_t)s->n_out * sizeof(float), nnew = c * (size_t)s->hop;
	hipStream_t q = s->own;
	{ const int r = order_after(s, q); if (r != EDISON_OK) return r; }
	{ const int r = make_room(s, q, s->chunk); if (r != EDISON_OK) return r; }
	memcpy(s->h_in, samples, sizeof(int16_t) * nnew);
	ED_HIP(ctx, hipMemcpyAsync(s->d_audio + (size_t)s->pos * s->hop + s->tail, s->h_in, sizeof(int16_t) * nnew, hipMemcpyHostToDevice, q));
	float *dl = (float *)s->d_out, *dp = (float *)(s->d_out + s->off_probs);
	{ const int r = enqueue_push(s, q, s->chunk, dl, dp, (int32_t *)(s->d_out + s->off_argmax), dp, s->d_out); if (r != EDISON_OK) return r; }
	ED_HIP(ctx, hipMemcpyAsync(s->h_out, s->d_out, s->out_bytes, hipMemcpyDeviceToHost, q));
	ED_HIP(ctx, hipStreamSynchronize(q));
	if (logits) memcpy(logits, s->h_out, fb);
	if (probs) memcpy(probs, s->h_out + s->off_probs, fb);
	if (argmax) memcpy(argmax, s->h_out + s->off_argmax, c * sizeof(int32_t));
	s->q_pending = 0;
	s->last_n = s->chunk;
	s->last_staged = 1;
	s->frames_seen += s->chunk;
	return EDISON_OK;
}

extern "C" int64_t edison_stream_float_frames_seen(const edison_stream_float *s) { return s ? s->frames_seen : -1; }

/* Copy `count` pieces of the last push's output block to the caller: from h_out after a host push, else from d_out on the stream the
 * work went to (host = 1: synchronously; host = 0: ordered on the context's stream). */
struct edsf_piece { void *dst; size_t off, bytes; };
static int copy_out(edison_stream_float *s, const edsf_piece *p, int count, int host)
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

static int filtered_out(edison_stream_float *s, float *filt, int32_t *likely, int32_t *spotted, int host)
{
	if (!s) return EDISON_E_ARGUMENT;
	if (!s->filter) return ed_set_err(s->ctx, EDISON_E_ARGUMENT, "stream_float: created without the output filter");
	const size_t n = (size_t)s->last_n;
	const edsf_piece p[3] = {{filt, s->off_filt, n * (size_t)s->n_out * sizeof(float)}, {likely, s->off_likely, n * sizeof(int32_t)},
	                         {spotted, s->off_spotted, n * sizeof(int32_t)}};
	return copy_out(s, p, 3, host);
}

static int fsm_out(edison_stream_float *s, edison_fsm *fsm, int32_t *states, int host)
{
	if (!s) return EDISON_E_ARGUMENT;
	if (!s->fsm) return ed_set_err(s->ctx, EDISON_E_ARGUMENT, "stream_float: created without the state machine (opts.fsm)");
	const edsf_piece p[2] = {{states, s->off_states, (size_t)s->last_n * sizeof(int32_t)}, {fsm, s->off_fsm, sizeof(edison_fsm)}};
	return copy_out(s, p, host ? 2 : 1, host);
}

extern "C" int edison_stream_float_filtered(edison_stream_float *s, float *filt, int32_t *likely, int32_t *spotted)
{
	return filtered_out(s, filt, likely, spotted, 1);
}

extern "C" int edison_stream_float_filtered_dev(edison_stream_float *s, float *filt, int32_t *likely, int32_t *spotted)
{
	return filtered_out(s, filt, likely, spotted, 0);
}

extern "C" int edison_stream_float_fsm(edison_stream_float *s, edison_fsm *fsm, int32_t *states) { return fsm_out(s, fsm, states, 1); }
extern "C" int edison_stream_float_fsm_dev(edison_stream_float *s, int32_t *states) { return fsm_out(s, NULL, states, 0); }
