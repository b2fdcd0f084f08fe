/*
 * edison_stream_bank.hip -- continuous mode for a graph trained at ANY MFCC geometry, for one microphone (include/edison_hip.h,
 * edison_stream_geom_*) and for a bank of them (edison_stream_bank_*; DESIGN.md sections 12 and 12b): n_mics microphones at one MFCC
 * geometry on the int8 graph loaded on the context, advancing in lockstep, each a stream of its own fed its own samples. A stream is a
 * bank of one microphone under its public name: every edison_stream_geom_* entry point forwards to the bank's. A push of n frames runs
 *
 *     [the shift, only when the push would not fit] -> one upload (strided for several microphones) -> ONE MFCC launch
 *     (ed_mfcc_geom_kernel, float64) over the n_mics * n frames -> the network -> [ONE n_out-class output filter (+ edisonFSM)]
 *
 * on the sliding-window core (edison_stream_core.h) with int8 feature rows and int8 outputs, whose shift and
 * filter run a workgroup per microphone: a number of launches that does not depend on n_mics. This file is a host object with no kernel
 * of its own. The network kernels take one base and one stride. One microphone: ONE launch over the push's n overlapping windows, read in
 * place at a stride of num_mfcc bytes. More: n launches, one per frame of the push, each over the n_mics windows of that frame, which lie
 * at d_feat + (pos + i) * nm + m * mic_feat; launch i writes slab i of the time-major outputs. The bank owns its own tables, so batch
 * calls at other geometries on the same context never touch it.
 *
 * A push with a mask (edison_bank_push_present*) runs the same upload and launches over all microphones; the core
 * then holds the absent ones (edison_bank_hold.hip): one launch more, whatever n_mics.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "edison_ctx.h"
#include "edison_stream_core.h"
#include "mfcc_geom.h"

#define ED_STREAM_BANK_MAX_MICS 4096

struct edison_stream_bank
{
	ed_stream_core core;           /* int8 rows, int8 outputs, n_mics microphones; core.who leads every message */
	int has_softmax;
	ed_geom_cache tab;             /* tables of its own (edison_kws_geom.hip builds them) */
	ed_geom_args_t margs;          /* tab.tmpl with the per-geometry fields; audio, feat, the strides and the frame counts are set per push */
	int model_epoch;
	size_t off_soft, off_argmax;   /* the front of the core's output block: logits [chunk][n_mics][n_out] at 0, softmax, argmax [chunk][n_mics] */
};

static ed_stream_core *core_of(edison_stream_bank *b) { return b ? &b->core : NULL; }
/* a stream is a bank of one microphone under the public opaque name */
static edison_stream_bank *bank_of(const edison_stream_geom *s) { return (edison_stream_bank *)s; }

static int bank_err(edison_ctx *ctx, const char *who, int code, const char *what)
{
	snprintf(ctx->err, sizeof(ctx->err), "%s: %s", who, what);
	return code;
}

/* the network on the kernel edison_net_batch_dev picks for the loaded graph, on hipStream q: n inputs, `stride` bytes apart */
static int ed_stream_geom_net_on(edison_ctx *ctx, hipStream_t q, const int8_t *in, int n, int64_t stride, int8_t *logits, int8_t *softmax, int32_t *argmax)
{
	const char *fg_ = getenv("EDISON_NET_FORCE_GENERAL"); /* read per call, as edison_net_batch_dev does */
	const int force_general = fg_ ? atoi(fg_) : 0;
	if (ctx->fast_model && !force_general) return ed_ctx_kws_cnn_launch_on(ctx, q, in, n, stride, logits, softmax, argmax);
	return ed_launch_result(ctx, ed_ctx_net_launch_on(ctx, q, in, n, stride, logits, softmax, argmax), "network kernel");
}

/* The device work of a push of n frames whose samples the core has uploaded: MFCC, network, the core's end of the push. The outputs go
 * where they are told (NULL: not written), time-major; the filter reads its input from `fin`. present: the push's mask (host = 1: host
 * memory), NULL: every microphone. */
static int enqueue_push(edison_stream_bank *b, hipStream_t q, int n, int8_t *logits, int8_t *softmax, int32_t *argmax, const int8_t *fin, int host,
                        const uint8_t *present)
{
	ed_stream_core *c = &b->core;
	edison_ctx *ctx = c->ctx;
	int8_t *win = (int8_t *)c->d_feat + (size_t)c->pos * c->nm; /* microphone 0: F - 1 rows of history, then the n new rows */
	ed_geom_args_t a = b->margs;
	a.audio = c->d_audio + (size_t)c->pos * c->hop;
	a.utt_stride = c->n_mics == 1 ? 0 : (int64_t)c->mic_audio;  /* an utterance of the launch = a microphone */
	a.frames_per_utt = n;
	a.n_frames = c->n_mics * n;
	a.feat = win + (size_t)(c->F - 1) * c->nm;
	a.feat_utt_stride = c->n_mics == 1 ? 0 : (int64_t)c->mic_feat;
	{ const int e = ed_launch_mfcc_geom(&a, ctx->n_cu, q); if (e != 0) return ed_launch_result(ctx, e, "MFCC geometry kernel"); }
	if (c->n_mics == 1)
	{
		const int r = ed_stream_geom_net_on(ctx, q, win, n, c->nm, logits, softmax, argmax); /* window i: num_mfcc bytes behind window i - 1 */
		if (r != EDISON_OK) return r;
	}
	else
	{
		const size_t slab = (size_t)c->n_mics * c->n_out;
		for (int i = 0; i < n; i++)
		{
			const int r = ed_stream_geom_net_on(ctx, q, win + (size_t)i * c->nm, c->n_mics, (int64_t)c->mic_feat, logits ? logits + i * slab : NULL,
			                                    softmax ? softmax + i * slab : NULL, argmax ? argmax + (size_t)i * c->n_mics : NULL);
			if (r != EDISON_OK) return r;
		}
	}
	if (present) return ed_stream_core_finish_push_present(c, q, fin, n, host, present, logits, softmax, argmax);
	return ed_stream_core_finish_push(c, q, fin, n, host);
}

static int check_push(edison_stream_bank *b, const int16_t *samples)
{
	if (!b || !samples) return EDISON_E_ARGUMENT;
	edison_ctx *ctx = b->core.ctx;
	if (b->model_epoch == ctx->model_epoch) return EDISON_OK;
	snprintf(ctx->err, sizeof(ctx->err), "%s: the model was reloaded after this stream was created; create a new stream", b->core.who);
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

extern "C" void edison_stream_bank_default_opts(edison_stream_bank_opts *o)
{
	if (!o) return;
	o->n_mics = 1;
	edison_stream_geom_default_opts(&o->stream);
}

extern "C" void edison_stream_bank_destroy(edison_stream_bank *b)
{
	if (!b) return;
	ed_stream_core_free(&b->core);
	if (b->tab.d) (void)hipFree(b->tab.d);
	delete b;
}

extern "C" int edison_stream_bank_reset(edison_stream_bank *b) { return ed_stream_core_reset(core_of(b)); }
extern "C" int edison_stream_bank_reset_mic(edison_stream_bank *b, int mic) { return ed_stream_core_reset_mic(core_of(b), mic); }

/* both creates; o: every microphone's options, messages led by `who` */
static int create(edison_ctx *ctx, const char *who, const edison_kws_geom *g, const edison_stream_geom_opts *o, int n_mics, edison_stream_bank **out)
{
	if (!ctx || !g || !o || !out) return EDISON_E_ARGUMENT;
	*out = NULL;
	if (n_mics < 1 || n_mics > ED_STREAM_BANK_MAX_MICS) return bank_err(ctx, who, EDISON_E_ARGUMENT, "n_mics must be 1 .. 4096");
	int F = 0;
	{ const int r = ed_kws_geom_check(ctx, g, &F); if (r != EDISON_OK) return r; }
	if (!ctx->have_model) return ed_set_err(ctx, EDISON_E_NO_MODEL, "no CNN model loaded (edison_model_load)");
	if ((int64_t)F * g->num_mfcc != ctx->net.in_n)
	{
		snprintf(ctx->err, sizeof(ctx->err), "%s: frame_count x num_mfcc = %lld features, the graph's input in_h x in_w x in_c = %d", who,
		         (long long)F * g->num_mfcc, ctx->net.in_n);
		return EDISON_E_SIZE;
	}
	const ed_stream_core_opts co = {o->chunk_frames, o->filter, o->fsm, o->filter_alpha, o->true_threshold};
	{ const int r = ed_stream_core_check_opts(ctx, who, g, &co); if (r != EDISON_OK) return r; }
	if (o->filter && ctx->net.out_n > EDSG_FILTER_MAX_OUT)
		return bank_err(ctx, who, EDISON_E_NO_IMPL, "the output filter serves graphs of at most 256 outputs");
	if (o->fsm && ctx->net.out_n != EDISON_NET_OUT)
		return bank_err(ctx, who, EDISON_E_NO_IMPL, "the state machine needs a graph with 10 outputs (the keyword list its roles index)");
	/* the MFCC launch counts n_mics * chunk_frames frames in an int32 */
	if ((int64_t)n_mics * o->chunk_frames >= ((int64_t)1 << 31))
		return bank_err(ctx, who, EDISON_E_SIZE, "n_mics x chunk_frames must stay below 2^31 frames per push");

	edison_stream_bank *b = new (std::nothrow) edison_stream_bank();
	if (!b) return bank_err(ctx, who, EDISON_E_NO_MEMORY, "host allocation failed");
	const size_t entries = (size_t)o->chunk_frames * n_mics, cn = entries * ctx->net.out_n; /* logits at 0 */
	b->off_soft = cn;
	b->off_argmax = ed_stream_core_align(cn + (ctx->net.has_softmax ? cn : 0));
	b->has_softmax = ctx->net.has_softmax;
	b->model_epoch = ctx->model_epoch;
	int r = ed_stream_core_create(&b->core, ctx, who, 1, 1, g, F, ctx->net.out_n, n_mics, &co, b->off_argmax + entries * sizeof(int32_t));
	if (r == EDISON_OK) r = ed_geom_tables_build(ctx, g, &b->tab);
	if (r != EDISON_OK) { edison_stream_bank_destroy(b); return r; }
	b->margs = b->tab.tmpl;
	b->margs.frame_step = g->frame_step;
	b->margs.take_log = (g->variant & 0xff) == EDISON_MFCC_A || (g->variant & EDISON_MFCC_USE_LOG);
	b->margs.feat_scale = (float)g->net_input_scale;
	*out = b;
	return EDISON_OK;
}

extern "C" int edison_stream_bank_create(edison_ctx *ctx, const edison_kws_geom *g, const edison_stream_bank_opts *o, edison_stream_bank **out)
{
	return create(ctx, "stream_bank", g, o ? &o->stream : NULL, o ? o->n_mics : 0, out);
}

extern "C" int edison_bank_push_present_n_dev(edison_stream_bank *b, const int16_t *samples, const uint8_t *present, int n_frames, int8_t *logits,
                                              int8_t *softmax, int32_t *argmax)
{
	{ const int r = check_push(b, samples); if (r != EDISON_OK) return r; }
	ed_stream_core *c = &b->core;
	hipStream_t q = c->ctx->stream;
	{ const int r = ed_stream_core_begin_push(c, q, samples, n_frames, 0); if (r != EDISON_OK) return r; }
	int8_t *so = b->has_softmax ? softmax : NULL;
	/* the filter's input: the caller's softmax (or logits for a graph without Softmax) where given, else the bank's block */
	const int8_t *fin = NULL;
	if (c->filter)
	{
		int8_t *&src = b->has_softmax ? so : logits;
		if (!src) src = (int8_t *)(c->d_out + (b->has_softmax ? b->off_soft : 0));
		fin = src;
	}
	return enqueue_push(b, q, n_frames, logits, so, argmax, fin, 0, present);
}

extern "C" int edison_stream_bank_push_n_dev(edison_stream_bank *b, const int16_t *samples, int n_frames, int8_t *logits, int8_t *softmax,
                                             int32_t *argmax)
{
	return edison_bank_push_present_n_dev(b, samples, NULL, n_frames, logits, softmax, argmax);
}

extern "C" int edison_stream_bank_push_dev(edison_stream_bank *b, const int16_t *samples, int8_t *logits, int8_t *softmax, int32_t *argmax)
{
	return edison_stream_bank_push_n_dev(b, samples, b ? b->core.chunk : 0, logits, softmax, argmax);
}

/* host pointers: one upload from pinned memory (strided for several microphones), the same launches on the private stream, one download of the
 * output block, one wait */
extern "C" int edison_bank_push_present(edison_stream_bank *b, const int16_t *samples, const uint8_t *present, int8_t *logits, int8_t *softmax,
                                        int32_t *argmax)
{
	{ const int r = check_push(b, samples); if (r != EDISON_OK) return r; }
	ed_stream_core *c = &b->core;
	const size_t entries = (size_t)c->chunk * c->n_mics, cn = entries * c->n_out;
	hipStream_t q = c->own;
	{ const int r = ed_stream_core_begin_push(c, q, samples, c->chunk, 1); if (r != EDISON_OK) return r; }
	int8_t *dl = (int8_t *)c->d_out, *ds = b->has_softmax ? (int8_t *)(c->d_out + b->off_soft) : NULL;
	{
		const int r = enqueue_push(b, q, c->chunk, dl, ds, (int32_t *)(c->d_out + b->off_argmax), b->has_softmax ? ds : dl, 1, present);
		if (r != EDISON_OK) return r;
	}
	if (logits) memcpy(logits, c->h_out, cn);
	if (softmax && b->has_softmax) memcpy(softmax, c->h_out + b->off_soft, cn);
	if (argmax) memcpy(argmax, c->h_out + b->off_argmax, entries * sizeof(int32_t));
	return EDISON_OK;
}

extern "C" int edison_stream_bank_push(edison_stream_bank *b, const int16_t *samples, int8_t *logits, int8_t *softmax, int32_t *argmax)
{
	return edison_bank_push_present(b, samples, NULL, logits, softmax, argmax);
}

extern "C" int edison_bank_frames_seen_mics(edison_stream_bank *b, int64_t *counts) { return ed_stream_core_frames_seen_mics(core_of(b), counts); }

extern "C" int edison_stream_bank_frames_seen(edison_stream_bank *b, int64_t *out)
{
	if (!b || !out) return EDISON_E_ARGUMENT;
	*out = b->core.frames_seen;
	return EDISON_OK;
}

extern "C" int edison_stream_bank_filtered(edison_stream_bank *b, float *filt, int32_t *likely, int32_t *spotted)
{
	return ed_stream_core_filtered(core_of(b), filt, likely, spotted, 1);
}

extern "C" int edison_stream_bank_filtered_dev(edison_stream_bank *b, float *filt, int32_t *likely, int32_t *spotted)
{
	return ed_stream_core_filtered(core_of(b), filt, likely, spotted, 0);
}

extern "C" int edison_stream_bank_fsm(edison_stream_bank *b, edison_fsm *fsm, int32_t *states) { return ed_stream_core_fsm(core_of(b), fsm, states, 1); }
extern "C" int edison_stream_bank_fsm_dev(edison_stream_bank *b, edison_fsm *fsm, int32_t *states) { return ed_stream_core_fsm(core_of(b), fsm, states, 0); }

/* ---- edison_stream_geom_*: the bank of one microphone, created with the prefix "stream_geom" */
extern "C" int edison_stream_geom_create(edison_ctx *ctx, const edison_kws_geom *g, const edison_stream_geom_opts *o, edison_stream_geom **out)
{
	return create(ctx, "stream_geom", g, o, 1, (edison_stream_bank **)out);
}

extern "C" void edison_stream_geom_destroy(edison_stream_geom *s) { edison_stream_bank_destroy(bank_of(s)); }
extern "C" int edison_stream_geom_reset(edison_stream_geom *s) { return edison_stream_bank_reset(bank_of(s)); }

extern "C" int edison_stream_geom_push(edison_stream_geom *s, const int16_t *samples, int8_t *logits, int8_t *softmax, int32_t *argmax)
{
	return edison_bank_push_present(bank_of(s), samples, NULL, logits, softmax, argmax);
}

extern "C" int edison_stream_geom_push_dev(edison_stream_geom *s, const int16_t *samples, int8_t *logits, int8_t *softmax, int32_t *argmax)
{
	return edison_stream_bank_push_dev(bank_of(s), samples, logits, softmax, argmax);
}

extern "C" int edison_stream_geom_push_n_dev(edison_stream_geom *s, const int16_t *samples, int n_frames, int8_t *logits, int8_t *softmax,
                                             int32_t *argmax)
{
	return edison_bank_push_present_n_dev(bank_of(s), samples, NULL, n_frames, logits, softmax, argmax);
}

extern "C" int64_t edison_stream_geom_frames_seen(const edison_stream_geom *s) { return s ? bank_of(s)->core.frames_seen : -1; }

extern "C" int edison_stream_geom_filtered(edison_stream_geom *s, float *filt, int32_t *likely, int32_t *spotted)
{
	return edison_stream_bank_filtered(bank_of(s), filt, likely, spotted);
}

extern "C" int edison_stream_geom_filtered_dev(edison_stream_geom *s, float *filt, int32_t *likely, int32_t *spotted)
{
	return edison_stream_bank_filtered_dev(bank_of(s), filt, likely, spotted);
}

extern "C" int edison_stream_geom_fsm(edison_stream_geom *s, edison_fsm *fsm, int32_t *states) { return edison_stream_bank_fsm(bank_of(s), fsm, states); }
extern "C" int edison_stream_geom_fsm_dev(edison_stream_geom *s, int32_t *states) { return edison_stream_bank_fsm_dev(bank_of(s), NULL, states); }
