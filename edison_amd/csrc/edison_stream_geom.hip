/*
 * edison_stream_geom.hip -- continuous mode for a graph trained at ANY MFCC geometry (include/edison_hip.h, edison_stream_geom_*): the
 * continuous counterpart of edison_kws_geom_batch*, as edison_stream.hip is the one of edison_kws_batch*. A push of n new frames runs
 *
 *     [shift, only when the push would not fit] -> MFCC (ed_mfcc_geom_kernel, float64) -> network over the n overlapping windows
 *     -> [n_out-class output filter (+ edisonFSM)]
 *
 * on the sliding-window core (edison_stream_core.h) with int8 feature rows and int8 outputs: the network kernel
 * reads window i of a push in place at a stride of num_mfcc bytes. This file keeps the MFCC and network launches and the front of the
 * output block. The stream owns its own tables, so batch calls at other geometries on the same context never touch it.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "edison_ctx.h"
#include "edison_stream_geom.h"

struct edison_stream_geom : ed_stream_geom_part
{
	ed_stream_core core;           /* int8 rows, int8 outputs */
	size_t off_soft, off_argmax;   /* the front of the core's output block: logits at 0, softmax (graphs that have one), argmax */
};

static ed_stream_core *core_of(edison_stream_geom *s) { return s ? &s->core : NULL; }

int ed_stream_geom_net_on(edison_ctx *ctx, hipStream_t q, const int8_t *in, int n, int64_t stride, int8_t *logits, int8_t *softmax, int32_t *argmax)
{
	const char *fg_ = getenv("EDISON_NET_FORCE_GENERAL"); /* read per call, as edison_net_batch_dev does */
	const int force_general = fg_ ? atoi(fg_) : 0;
	if (ctx->fast_model && !force_general) return ed_ctx_kws_cnn_launch_on(ctx, q, in, n, stride, logits, softmax, argmax);
	return ed_launch_result(ctx, ed_ctx_net_launch_on(ctx, q, in, n, stride, logits, softmax, argmax), "network kernel");
}

/* The device work of a push of n frames whose samples the core has uploaded: MFCC, network, the core's end of the push. The outputs go
 * where they are told (NULL: not written); the filter reads its input from `fin`. */
static int enqueue_push(edison_stream_geom *s, hipStream_t q, int n, int8_t *logits, int8_t *softmax, int32_t *argmax, const int8_t *fin,
                        int host)
{
	ed_stream_core *c = &s->core;
	edison_ctx *ctx = c->ctx;
	int8_t *win = (int8_t *)c->d_feat + (size_t)c->pos * c->nm; /* F - 1 rows of history, then the n new rows */
	ed_geom_args_t a = s->margs;
	a.audio = c->d_audio + (size_t)c->pos * c->hop;
	a.frames_per_utt = n;
	a.n_frames = n;
	a.feat = win + (size_t)(c->F - 1) * c->nm;
	{ const int e = ed_launch_mfcc_geom(&a, ctx->n_cu, q); if (e != 0) return ed_launch_result(ctx, e, "MFCC geometry kernel"); }
	{ const int r = ed_stream_geom_net_on(ctx, q, win, n, c->nm, logits, softmax, argmax); if (r != EDISON_OK) return r; }
	return ed_stream_core_finish_push(c, q, fin, n, host);
}

static int check_push(edison_stream_geom *s, const int16_t *samples)
{
	if (!s || !samples) return EDISON_E_ARGUMENT;
	return ed_stream_geom_part_check(s->core.ctx, "stream_geom", s);
}

int ed_stream_geom_part_check(edison_ctx *ctx, const char *who, const ed_stream_geom_part *p)
{
	if (p->model_epoch == ctx->model_epoch) return EDISON_OK;
	snprintf(ctx->err, sizeof(ctx->err), "%s: the model was reloaded after this stream was created; create a new stream", who);
	return EDISON_E_ARGUMENT;
}

extern "C" void edison_stream_geom_default_opts(edison_stream_geom_opts *o)
{
	if (!o) return;
	memset(o, 0, sizeof(*o));
	o->chunk_frames = 1;     /* filter and fsm stay 0 */
	o->filter_alpha = 0.9;   /* edison_stream_default_opts' values: NET_OUT_MOVING_AVG_ALPHA (app.c:38) */
	o->true_threshold = 0.5; /* TRUE_THRESHOLD (app.c:34) */
}

extern "C" void edison_stream_geom_destroy(edison_stream_geom *s)
{
	if (!s) return;
	ed_stream_core_free(&s->core);
	ed_stream_geom_part_free(s);
	delete s;
}

extern "C" int edison_stream_geom_reset(edison_stream_geom *s) { return ed_stream_core_reset(core_of(s)); }

static int part_err(edison_ctx *ctx, const char *who, int code, const char *what)
{
	snprintf(ctx->err, sizeof(ctx->err), "%s: %s", who, what);
	return code;
}

int ed_stream_geom_check_create(edison_ctx *ctx, const char *who, const edison_kws_geom *g, const edison_stream_geom_opts *o, int *F,
                                ed_stream_core_opts *co)
{
	{ const int r = ed_kws_geom_check(ctx, g, F); if (r != EDISON_OK) return r; }
	if (!ctx->have_model) return ed_set_err(ctx, EDISON_E_NO_MODEL, "no CNN model loaded (edison_model_load)");
	if ((int64_t)*F * g->num_mfcc != ctx->net.in_n)
	{
		snprintf(ctx->err, sizeof(ctx->err), "%s: frame_count x num_mfcc = %lld features, the graph's input in_h x in_w x in_c = %d", who,
		         (long long)*F * g->num_mfcc, ctx->net.in_n);
		return EDISON_E_SIZE;
	}
	*co = {o->chunk_frames, o->filter, o->fsm, o->filter_alpha, o->true_threshold};
	{ const int r = ed_stream_core_check_opts(ctx, who, g, co); if (r != EDISON_OK) return r; }
	if (o->filter && ctx->net.out_n > EDSG_FILTER_MAX_OUT)
		return part_err(ctx, who, EDISON_E_NO_IMPL, "the output filter serves graphs of at most 256 outputs");
	if (o->fsm && ctx->net.out_n != EDISON_NET_OUT)
		return part_err(ctx, who, EDISON_E_NO_IMPL, "the state machine needs a graph with 10 outputs (the keyword list its roles index)");
	return EDISON_OK;
}

int ed_stream_geom_part_init(edison_ctx *ctx, const edison_kws_geom *g, ed_stream_geom_part *p)
{
	p->has_softmax = ctx->net.has_softmax;
	p->model_epoch = ctx->model_epoch;
	{ const int r = ed_geom_tables_build(ctx, g, &p->tab); if (r != EDISON_OK) return r; }
	p->margs = p->tab.tmpl;
	p->margs.utt_stride = 0;
	p->margs.frame_step = g->frame_step;
	p->margs.take_log = (g->variant & 0xff) == EDISON_MFCC_A || (g->variant & EDISON_MFCC_USE_LOG);
	p->margs.feat_scale = (float)g->net_input_scale;
	return EDISON_OK;
}

void ed_stream_geom_part_free(ed_stream_geom_part *p)
{
	if (p->tab.d) (void)hipFree(p->tab.d);
	p->tab.d = NULL;
}

extern "C" int edison_stream_geom_create(edison_ctx *ctx, const edison_kws_geom *g, const edison_stream_geom_opts *o, edison_stream_geom **out)
{
	if (!ctx || !g || !o || !out) return EDISON_E_ARGUMENT;
	*out = NULL;
	int F = 0;
	ed_stream_core_opts co;
	{ const int r = ed_stream_geom_check_create(ctx, "stream_geom", g, o, &F, &co); if (r != EDISON_OK) return r; }

	edison_stream_geom *s = new (std::nothrow) edison_stream_geom();
	if (!s) return ed_set_err(ctx, EDISON_E_NO_MEMORY, "host allocation failed");
	const size_t cn = (size_t)o->chunk_frames * ctx->net.out_n;               /* logits at 0 */
	s->off_soft = cn;
	s->off_argmax = ed_stream_core_align(cn + (ctx->net.has_softmax ? cn : 0));
	int r = ed_stream_core_create(&s->core, ctx, "stream_geom", 1, 1, g, F, ctx->net.out_n, 1, &co, s->off_argmax + (size_t)o->chunk_frames * sizeof(int32_t));
	if (r == EDISON_OK) r = ed_stream_geom_part_init(ctx, g, s);
	if (r != EDISON_OK) { edison_stream_geom_destroy(s); return r; }
	*out = s;
	return EDISON_OK;
}

extern "C" int edison_stream_geom_push_n_dev(edison_stream_geom *s, const int16_t *samples, int n_frames, int8_t *logits, int8_t *softmax,
                                             int32_t *argmax)
{
	{ const int r = check_push(s, samples); if (r != EDISON_OK) return r; }
	ed_stream_core *c = &s->core;
	hipStream_t q = c->ctx->stream;
	{ const int r = ed_stream_core_begin_push(c, q, samples, n_frames, 0); if (r != EDISON_OK) return r; }
	int8_t *so = s->has_softmax ? softmax : NULL;
	/* the filter's input: the caller's softmax (or logits for a graph without Softmax) where given, else the stream's block */
	const int8_t *fin = NULL;
	if (c->filter)
	{
		int8_t *&src = s->has_softmax ? so : logits;
		if (!src) src = (int8_t *)(c->d_out + (s->has_softmax ? s->off_soft : 0));
		fin = src;
	}
	return enqueue_push(s, q, n_frames, logits, so, argmax, fin, 0);
}

extern "C" int edison_stream_geom_push_dev(edison_stream_geom *s, const int16_t *samples, int8_t *logits, int8_t *softmax, int32_t *argmax)
{
	return edison_stream_geom_push_n_dev(s, samples, s ? s->core.chunk : 0, logits, softmax, argmax);
}

/* host pointers: one upload from pinned memory, the same launches on the private stream, one download of the output block, one wait */
extern "C" int edison_stream_geom_push(edison_stream_geom *s, const int16_t *samples, int8_t *logits, int8_t *softmax, int32_t *argmax)
{
	{ const int r = check_push(s, samples); if (r != EDISON_OK) return r; }
	ed_stream_core *c = &s->core;
	const size_t cn = (size_t)c->chunk * c->n_out;
	hipStream_t q = c->own;
	{ const int r = ed_stream_core_begin_push(c, q, samples, c->chunk, 1); if (r != EDISON_OK) return r; }
	int8_t *dl = (int8_t *)c->d_out, *ds = s->has_softmax ? (int8_t *)(c->d_out + s->off_soft) : NULL;
	{
		const int r = enqueue_push(s, q, c->chunk, dl, ds, (int32_t *)(c->d_out + s->off_argmax), s->has_softmax ? ds : dl, 1);
		if (r != EDISON_OK) return r;
	}
	if (logits) memcpy(logits, c->h_out, cn);
	if (softmax && s->has_softmax) memcpy(softmax, c->h_out + s->off_soft, cn);
	if (argmax) memcpy(argmax, c->h_out + s->off_argmax, (size_t)c->chunk * sizeof(int32_t));
	return EDISON_OK;
}

extern "C" int64_t edison_stream_geom_frames_seen(const edison_stream_geom *s) { return s ? s->core.frames_seen : -1; }

extern "C" int edison_stream_geom_filtered(edison_stream_geom *s, float *filt, int32_t *likely, int32_t *spotted)
{
	return ed_stream_core_filtered(core_of(s), filt, likely, spotted, 1);
}

extern "C" int edison_stream_geom_filtered_dev(edison_stream_geom *s, float *filt, int32_t *likely, int32_t *spotted)
{
	return ed_stream_core_filtered(core_of(s), filt, likely, spotted, 0);
}

extern "C" int edison_stream_geom_fsm(edison_stream_geom *s, edison_fsm *fsm, int32_t *states) { return ed_stream_core_fsm(core_of(s), fsm, states, 1); }
extern "C" int edison_stream_geom_fsm_dev(edison_stream_geom *s, int32_t *states) { return ed_stream_core_fsm(core_of(s), NULL, states, 0); }
