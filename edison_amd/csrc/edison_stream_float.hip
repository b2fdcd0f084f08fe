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
 * It runs on the sliding-window core (edison_stream_core.h) with float32 feature rows and float32 outputs: the
 * network kernel reads window i of a push in place at an input stride of num_mfcc floats. This file keeps the feature and network
 * launches and the front of the output block. The stream owns its own geometry tables.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <new>

#include "edison_ctx.h"
#include "edison_stream_core.h"
#include "fnet.h"
#include "mfcc_geom.h"

struct edison_stream_float
{
	ed_stream_core core;           /* float32 rows, float32 outputs */
	int q15;
	float scale, lo, hi;           /* the host flow's (float)net_input_scale and clip range */
	ed_geom_cache tab;             /* this stream's own tables (host flow only; edison_kws_geom.hip builds them) */
	ed_geom_args_t margs;          /* tab.tmpl with the per-geometry fields; audio and the frame counts are set per push */
	size_t off_probs, off_argmax;  /* the front of the core's output block: logits at 0, probs, argmax */
	int fnet_epoch;
};

static ed_stream_core *core_of(edison_stream_float *s) { return s ? &s->core : NULL; }

/* The device work of a push of n frames whose samples the core has uploaded: feature rows, network, the core's end of the push. The
 * outputs go where they are told (NULL: not written); the filter reads `probs`. */
static int enqueue_push(edison_stream_float *s, hipStream_t q, int n, float *logits, float *probs, int32_t *argmax, int host)
{
	ed_stream_core *c = &s->core;
	edison_ctx *ctx = c->ctx;
	float *win = (float *)c->d_feat + (size_t)c->pos * c->nm; /* F - 1 rows of history, then the n new rows */
	float *rows = win + (size_t)(c->F - 1) * c->nm;
	const int16_t *au = c->d_audio + (size_t)c->pos * c->hop;
	if (s->q15)
	{
		/* variant C int16 -> (float), no scale, no clip (app.c:675-683): the Q15 kernel's float output, frames hop samples apart */
		const int r = ed_ctx_mfcc_q15_launch_on(ctx, q, au, n, n, 0, c->hop, c->nm, NULL, rows, NULL, 0, NULL, NULL, NULL);
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
		const int e = ed_launch_fnet(ed_ctx_fnet_plan(ctx), win, c->nm, n, logits, probs, argmax, NULL, q);
		if (e != 0) return ed_launch_result(ctx, e, "float network kernel");
	}
	return ed_stream_core_finish_push(c, q, probs, n, host);
}

static int check_push(edison_stream_float *s, const int16_t *samples)
{
	if (!s || !samples) return EDISON_E_ARGUMENT;
	edison_ctx *ctx = s->core.ctx;
	if (s->fnet_epoch != ctx->fnet_epoch || !ctx->fnet)
		return ed_set_err(ctx, EDISON_E_ARGUMENT, "stream_float: the float network was reloaded after this stream was created; create a new stream");
	return EDISON_OK;
}

extern "C" void edison_stream_float_default_opts(edison_stream_float_opts *o)
{
	if (!o) return;
	memset(o, 0, sizeof(*o));
	o->chunk_frames = 1;     /* q15, filter and fsm stay 0 */
	o->clip_lo = -32768.0f; /* audio/config.py's net_input_clip_min / _max, as Context.kws_float */
	o->clip_hi = 32767.0f;
	o->filter_alpha = 0.5;   /* NET_OUT_MOVING_AVG_ALPHA of the Cube build (app.c:35-36) */
	o->true_threshold = 0.5; /* TRUE_THRESHOLD (app.c:34) */
}

extern "C" void edison_stream_float_destroy(edison_stream_float *s)
{
	if (!s) return;
	ed_stream_core_free(&s->core);
	if (s->tab.d) (void)hipFree(s->tab.d);
	delete s;
}

extern "C" int edison_stream_float_reset(edison_stream_float *s) { return ed_stream_core_reset(core_of(s)); }

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
	const ed_stream_core_opts co = {o->chunk_frames, o->filter, o->fsm, o->filter_alpha, o->true_threshold};
	{ const int r = ed_stream_core_check_opts(ctx, "stream_float", g, &co); if (r != EDISON_OK) return r; }
	if (o->filter && n_out > EDSG_FILTER_MAX_OUT)
		return ed_set_err(ctx, EDISON_E_NO_IMPL, "stream_float: the output filter serves networks of at most 256 outputs");
	if (o->fsm && n_out != EDISON_NET_OUT)
		return ed_set_err(ctx, EDISON_E_NO_IMPL, "stream_float: the state machine needs a network with 10 outputs (the keyword list its roles index)");

	edison_stream_float *s = new (std::nothrow) edison_stream_float();
	if (!s) return ed_set_err(ctx, EDISON_E_NO_MEMORY, "host allocation failed");
	s->q15 = o->q15;
	s->scale = (float)g->net_input_scale; s->lo = o->clip_lo; s->hi = o->clip_hi;
	s->fnet_epoch = ctx->fnet_epoch;
	s->off_probs = (size_t)o->chunk_frames * n_out * sizeof(float);          /* logits at 0 */
	s->off_argmax = 2 * s->off_probs;
	int r = ed_stream_core_create(&s->core, ctx, "stream_float", sizeof(float), sizeof(float), g, F, n_out, 1, &co,
	                              s->off_argmax + (size_t)o->chunk_frames * sizeof(int32_t));
	if (r == EDISON_OK && !s->q15) r = ed_geom_tables_build(ctx, g, &s->tab);
	if (r != EDISON_OK) { edison_stream_float_destroy(s); return r; }
	if (!s->q15)
	{
		s->margs = s->tab.tmpl;
		s->margs.utt_stride = 0;
		s->margs.frame_step = g->frame_step;
		s->margs.take_log = (g->variant & 0xff) == EDISON_MFCC_A || (g->variant & EDISON_MFCC_USE_LOG);
		s->margs.feat = NULL;
	}
	*out = s;
	return EDISON_OK;
}

extern "C" int edison_stream_float_push_n_dev(edison_stream_float *s, const int16_t *samples, int n_frames, float *logits, float *probs,
                                              int32_t *argmax)
{
	{ const int r = check_push(s, samples); if (r != EDISON_OK) return r; }
	ed_stream_core *c = &s->core;
	hipStream_t q = c->ctx->stream;
	{ const int r = ed_stream_core_begin_push(c, q, samples, n_frames, 0); if (r != EDISON_OK) return r; }
	/* the filter's input: the caller's probs where given, else the stream's block */
	if (c->filter && !probs) probs = (float *)(c->d_out + s->off_probs);
	return enqueue_push(s, q, n_frames, logits, probs, argmax, 0);
}

extern "C" int edison_stream_float_push_dev(edison_stream_float *s, const int16_t *samples, float *logits, float *probs, int32_t *argmax)
{
	return edison_stream_float_push_n_dev(s, samples, s ? s->core.chunk : 0, logits, probs, argmax);
}

/* host pointers: one upload from pinned memory, the same launches on the private stream, one download of the output block, one wait */
extern "C" int edison_stream_float_push(edison_stream_float *s, const int16_t *samples, float *logits, float *probs, int32_t *argmax)
{
	{ const int r = check_push(s, samples); if (r != EDISON_OK) return r; }
	ed_stream_core *c = &s->core;
	hipStream_t q = c->own;
	{ const int r = ed_stream_core_begin_push(c, q, samples, c->chunk, 1); if (r != EDISON_OK) return r; }
	{
		const int r = enqueue_push(s, q, c->chunk, (float *)c->d_out, (float *)(c->d_out + s->off_probs), (int32_t *)(c->d_out + s->off_argmax), 1);
		if (r != EDISON_OK) return r;
	}
	const size_t fb = s->off_probs; /* chunk * n_out floats */
	if (logits) memcpy(logits, c->h_out, fb);
	if (probs) memcpy(probs, c->h_out + fb, fb);
	if (argmax) memcpy(argmax, c->h_out + s->off_argmax, (size_t)c->chunk * sizeof(int32_t));
	return EDISON_OK;
}

extern "C" int64_t edison_stream_float_frames_seen(const edison_stream_float *s) { return s ? s->core.frames_seen : -1; }

extern "C" int edison_stream_float_filtered(edison_stream_float *s, float *filt, int32_t *likely, int32_t *spotted)
{
	return ed_stream_core_filtered(core_of(s), filt, likely, spotted, 1);
}

extern "C" int edison_stream_float_filtered_dev(edison_stream_float *s, float *filt, int32_t *likely, int32_t *spotted)
{
	return ed_stream_core_filtered(core_of(s), filt, likely, spotted, 0);
}

extern "C" int edison_stream_float_fsm(edison_stream_float *s, edison_fsm *fsm, int32_t *states) { return ed_stream_core_fsm(core_of(s), fsm, states, 1); }
extern "C" int edison_stream_float_fsm_dev(edison_stream_float *s, int32_t *states) { return ed_stream_core_fsm(core_of(s), NULL, states, 0); }
