/*
 * edison_stream_bank.hip -- a bank of continuous streams (include/edison_hip.h, edison_stream_bank_*): n_mics
 * microphones at one MFCC geometry on the graph loaded on the context, advancing in lockstep. Microphone m behaves as an
 * edison_stream_geom of its own fed microphone m's samples; a push of n frames for all of them runs
 *
 *     [the shift, only when the push would not fit] -> one strided upload -> ONE MFCC launch over n_mics * n frames
 *     -> n network launches (one per frame of the push, each over the n_mics windows of that frame) -> [ONE filter (+ edisonFSM)]
 *
 * on the sliding-window core with n_mics microphones (edison_stream_core.h), whose shift and filter run a workgroup per microphone: a
 * number of launches that does not depend on n_mics. This file is a host object with no kernel of its own. The
 * network kernels are the ones edison_stream_geom runs, unchanged: for frame i of the push the windows of all microphones lie at
 * d_feat + (pos + i) * nm + m * mic_feat, one base and one stride, which is what they take. Launch i writes slab i of the time-major
 * outputs. The checks, the tables and the choice of the network kernel are edison_stream_geom.hip's (edison_stream_geom.h).
 *
 * A push with a mask (edison_bank_push_present*) runs the same upload and launches over all microphones; the core
 * then holds the absent ones (edison_bank_hold.hip): one launch more, whatever n_mics.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <new>

#include "edison_ctx.h"
#include "edison_stream_geom.h"

#define ED_STREAM_BANK_MAX_MICS 4096

struct edison_stream_bank : ed_stream_geom_part
{
	ed_stream_core core;           /* int8 rows, int8 outputs, n_mics microphones */
	size_t off_soft, off_argmax;   /* the front of the core's output block: logits [chunk][n_mics][n_out] at 0, softmax, argmax [chunk][n_mics] */
};

static ed_stream_core *core_of(edison_stream_bank *b) { return b ? &b->core : NULL; }

static int bank_err(edison_ctx *ctx, int code, const char *what)
{
	snprintf(ctx->err, sizeof(ctx->err), "stream_bank: %s", what);
	return code;
}

/* The device work of a push of n frames whose samples the core has uploaded. The outputs go where they are told (NULL: not written),
 * time-major; the filter reads its input from `fin`. present: the push's mask (host = 1: host memory), NULL: every microphone. */
static int enqueue_push(edison_stream_bank *b, hipStream_t q, int n, int8_t *logits, int8_t *softmax, int32_t *argmax, const int8_t *fin, int host,
                        const uint8_t *present)
{
	ed_stream_core *c = &b->core;
	edison_ctx *ctx = c->ctx;
	int8_t *win = (int8_t *)c->d_feat + (size_t)c->pos * c->nm; /* microphone 0: F - 1 rows of history, then the n new rows */
	ed_geom_args_t a = b->margs;
	a.audio = c->d_audio + (size_t)c->pos * c->hop;
	a.utt_stride = (int64_t)c->mic_audio;                       /* an utterance of the launch = a microphone */
	a.frames_per_utt = n;
	a.n_frames = c->n_mics * n;
	a.feat = win + (size_t)(c->F - 1) * c->nm;
	a.feat_utt_stride = (int64_t)c->mic_feat;
	{ const int e = ed_launch_mfcc_geom(&a, ctx->n_cu, q); if (e != 0) return ed_launch_result(ctx, e, "MFCC geometry kernel"); }
	const size_t slab = (size_t)c->n_mics * c->n_out;
	for (int i = 0; i < n; i++)
	{
		const int r = ed_stream_geom_net_on(ctx, q, win + (size_t)i * c->nm, c->n_mics, (int64_t)c->mic_feat, logits ? logits + i * slab : NULL,
		                                    softmax ? softmax + i * slab : NULL, argmax ? argmax + (size_t)i * c->n_mics : NULL);
		if (r != EDISON_OK) return r;
	}
	if (present) return ed_stream_core_finish_push_present(c, q, fin, n, host, present, logits, softmax, argmax);
	return ed_stream_core_finish_push(c, q, fin, n, host);
}

static int check_push(edison_stream_bank *b, const int16_t *samples)
{
	if (!b || !samples) return EDISON_E_ARGUMENT;
	return ed_stream_geom_part_check(b->core.ctx, "stream_bank", b);
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
	ed_stream_geom_part_free(b);
	delete b;
}

extern "C" int edison_stream_bank_reset(edison_stream_bank *b) { return ed_stream_core_reset(core_of(b)); }
extern "C" int edison_stream_bank_reset_mic(edison_stream_bank *b, int mic) { return ed_stream_core_reset_mic(core_of(b), mic); }

extern "C" int edison_stream_bank_create(edison_ctx *ctx, const edison_kws_geom *g, const edison_stream_bank_opts *o, edison_stream_bank **out)
{
	if (!ctx || !g || !o || !out) return EDISON_E_ARGUMENT;
	*out = NULL;
	if (o->n_mics < 1 || o->n_mics > ED_STREAM_BANK_MAX_MICS) return bank_err(ctx, EDISON_E_ARGUMENT, "n_mics must be 1 .. 4096");
	int F = 0;
	ed_stream_core_opts co;
	{ const int r = ed_stream_geom_check_create(ctx, "stream_bank", g, &o->stream, &F, &co); if (r != EDISON_OK) return r; }
	/* the MFCC launch counts n_mics * chunk_frames frames in an int32 */
	if ((int64_t)o->n_mics * o->stream.chunk_frames >= ((int64_t)1 << 31))
		return bank_err(ctx, EDISON_E_SIZE, "n_mics x chunk_frames must stay below 2^31 frames per push");

	edison_stream_bank *b = new (std::nothrow) edison_stream_bank();
	if (!b) return bank_err(ctx, EDISON_E_NO_MEMORY, "host allocation failed");
	const size_t entries = (size_t)o->stream.chunk_frames * o->n_mics, cn = entries * ctx->net.out_n;
	b->off_soft = cn;
	b->off_argmax = ed_stream_core_align(cn + (ctx->net.has_softmax ? cn : 0));
	int r = ed_stream_core_create(&b->core, ctx, "stream_bank", 1, 1, g, F, ctx->net.out_n, o->n_mics, &co, b->off_argmax + entries * sizeof(int32_t));
	if (r == EDISON_OK) r = ed_stream_geom_part_init(ctx, g, b);
	if (r != EDISON_OK) { edison_stream_bank_destroy(b); return r; }
	*out = b;
	return EDISON_OK;
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

/* host pointers: one strided upload from pinned memory, the same launches on the private stream, one download of the output block, one wait */
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
