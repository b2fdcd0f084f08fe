/*
 * edison_float_bank.hip -- continuous mode for the float32 X-CUBE-AI network, the firmware's loop for NET_TYPE_CUBE (app.c:288-371,
 * 630-719), for one microphone (include/edison_hip.h, edison_stream_float_*) and for a bank of them (edison_float_bank_*; DESIGN.md
 * sections 15 and 15a): n_mics microphones at one MFCC geometry on the float network loaded on the context, advancing in lockstep, each a
 * stream of its own fed its own samples. A stream is a bank of one microphone under its public name: every edison_stream_float_* entry
 * point forwards to the bank's. A push of n frames for all microphones runs
 *
 *     [banked shift, only when the push would not fit] -> one strided upload -> feature rows of all n_mics * n frames
 *     -> ONE network launch over the n * n_mics windows -> [ONE banked filter (+ edisonFSM)]
 *
 * on the sliding-window core with n_mics microphones, float32 rows and float32 outputs (edison_stream_core.h): a number of launches that
 * does not depend on n_mics, nor on n. The feature rows come from ONE ed_mfcc_geom_fnet_kernel launch in the host flow (q15 = 0), an
 * utterance of the launch being a microphone and feat_utt_stride carrying its rows behind its own history. In the firmware flow (q15 = 1)
 * ONE launch of the variant C kernel, which has no such stride, writes the rows compactly [n_mics][n][num_mfcc] into a scratch of the
 * bank's and one strided device-to-device copy places them. The network reads window i of microphone m in place at
 * d_feat + m * mic_feat + (pos + i) * num_mfcc floats: two strides, ed_fnet_windows_kernel (fnet_windows_kernels.hip). Where one stride
 * describes the windows -- one frame (mic_feat / 4 floats apart) or one microphone (num_mfcc apart) -- the launch is ed_fnet_kernel's, and
 * one microphone needs no strided copy and no scratch: the rows of either flow land behind its history in place.
 *
 * A push with a mask (edison_fbank_push_present*) runs the same upload and launches over all microphones; the
 * core then holds the absent ones (edison_bank_hold.hip): one launch more, whatever n_mics.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <new>

#include "edison_ctx.h"
#include "edison_stream_core.h"
#include "fnet.h"
#include "mfcc_geom.h"

#define ED_FLOAT_BANK_MAX_MICS 4096

struct edison_float_bank
{
	ed_stream_core core;           /* float32 rows, float32 outputs, n_mics microphones; core.who leads every message */
	const char *noun;              /* what the reload message calls the object: "stream" or "bank" */
	int q15;
	float scale, lo, hi;           /* the host flow's (float)net_input_scale and clip range */
	ed_geom_cache tab;             /* this bank's own tables (host flow only; edison_kws_geom.hip builds them) */
	ed_geom_args_t margs;          /* tab.tmpl with the per-geometry fields; audio and the frame counts are set per push */
	float *d_rows;                 /* firmware flow, n_mics > 1: [n_mics][chunk][num_mfcc] the variant C kernel's compact rows */
	size_t off_probs, off_argmax;  /* the front of the core's output block: logits [chunk][n_mics][n_out] at 0, probs, argmax [chunk][n_mics] */
	int fnet_epoch;
	int per_frame;                 /* tools/bench_float_bank.py only: one network launch per frame of the push (ed_float_bank_tool_per_frame) */
};

static ed_stream_core *core_of(edison_float_bank *b) { return b ? &b->core : NULL; }
/* a stream is a bank of one microphone under the public opaque name */
static edison_float_bank *bank_of(const edison_stream_float *s) { return (edison_float_bank *)s; }

static int bank_err(edison_ctx *ctx, const char *who, int code, const char *what)
{
	snprintf(ctx->err, sizeof(ctx->err), "%s: %s", who, what);
	return code;
}

/* The device work of a push of n frames whose samples the core has uploaded: feature rows, network, the core's end of the push. The
 * outputs go where they are told (NULL: not written), time-major; the filter reads `probs`. present: the push's mask (host = 1: host
 * memory), NULL: every microphone. */
static int enqueue_push(edison_float_bank *b, hipStream_t q, int n, float *logits, float *probs, int32_t *argmax, int host, const uint8_t *present)
{
	ed_stream_core *c = &b->core;
	edison_ctx *ctx = c->ctx;
	const int64_t mic_rows = (int64_t)(c->mic_feat / sizeof(float));  /* floats from one microphone's rows to the next's */
	float *win = (float *)c->d_feat + (size_t)c->pos * c->nm;         /* microphone 0: F - 1 rows of history, then the n new rows */
	float *rows = win + (size_t)(c->F - 1) * c->nm;
	const int16_t *au = c->d_audio + (size_t)c->pos * c->hop;
	if (b->q15)
	{
		/* variant C int16 -> (float), no scale, no clip (app.c:675-683): a group of the launch = a microphone, its frames hop samples apart */
		float *dst = c->n_mics == 1 ? rows : b->d_rows;
		const int64_t group_stride = c->n_mics == 1 ? 0 : (int64_t)c->mic_audio;
		const int r = ed_ctx_mfcc_q15_launch_on(ctx, q, au, (int64_t)c->n_mics * n, n, group_stride, c->hop, c->nm, NULL, dst, NULL, 0, NULL, NULL, NULL);
		if (r != EDISON_OK) return r;
		if (c->n_mics > 1)
		{
			const size_t bytes = sizeof(float) * (size_t)n * c->nm; /* a row of the copy = a microphone's n new rows */
			ED_HIP(ctx, hipMemcpy2DAsync(rows, c->mic_feat, dst, bytes, bytes, (size_t)c->n_mics, hipMemcpyDeviceToDevice, q));
		}
	}
	else
	{
		ed_geom_args_t a = b->margs;
		a.audio = au;
		a.utt_stride = c->n_mics == 1 ? 0 : (int64_t)c->mic_audio;    /* an utterance of the launch = a microphone */
		a.frames_per_utt = n;
		a.n_frames = c->n_mics * n;
		a.feat_utt_stride = c->n_mics == 1 ? 0 : mic_rows;
		const int e = ed_launch_mfcc_geom_fnet(&a, rows, b->scale, b->lo, b->hi, ctx->n_cu, q);
		if (e != 0) return ed_launch_result(ctx, e, "MFCC geometry kernel (float network input)");
	}
	{
		const ed_fnet_plan_t *p = ed_ctx_fnet_plan(ctx);
		int e;
		if (c->n_mics == 1) e = ed_launch_fnet(p, win, c->nm, n, logits, probs, argmax, NULL, q);
		else if (n == 1) e = ed_launch_fnet(p, win, mic_rows, c->n_mics, logits, probs, argmax, NULL, q);
		else e = ed_launch_fnet_windows(p, win, mic_rows, c->n_mics, c->nm, n, logits, probs, argmax, b->per_frame, q);
		if (e != 0) return ed_launch_result(ctx, e, "float network kernel");
	}
	if (present) return ed_stream_core_finish_push_present(c, q, probs, n, host, present, logits, probs, argmax);
	return ed_stream_core_finish_push(c, q, probs, n, host);
}

static int check_push(edison_float_bank *b, const int16_t *samples)
{
	if (!b || !samples) return EDISON_E_ARGUMENT;
	edison_ctx *ctx = b->core.ctx;
	if (b->fnet_epoch == ctx->fnet_epoch && ctx->fnet) return EDISON_OK;
	snprintf(ctx->err, sizeof(ctx->err), "%s: the float network was reloaded after this %s was created; create a new %s", b->core.who, b->noun, b->noun);
	return EDISON_E_ARGUMENT;
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

extern "C" void edison_float_bank_default_opts(edison_float_bank_opts *o)
{
	if (!o) return;
	o->n_mics = 1;
	edison_stream_float_default_opts(&o->stream);
}

extern "C" void edison_float_bank_destroy(edison_float_bank *b)
{
	if (!b) return;
	ed_stream_core_free(&b->core);
	if (b->d_rows) (void)hipFree(b->d_rows);
	if (b->tab.d) (void)hipFree(b->tab.d);
	delete b;
}

extern "C" int edison_float_bank_reset(edison_float_bank *b) { return ed_stream_core_reset(core_of(b)); }
extern "C" int edison_float_bank_reset_mic(edison_float_bank *b, int mic) { return ed_stream_core_reset_mic(core_of(b), mic); }

/* both creates; o: every microphone's options, messages led by `who`, the object called `noun` */
static int create(edison_ctx *ctx, const char *who, const char *noun, const edison_kws_geom *g, const edison_stream_float_opts *o, int n_mics,
                  edison_float_bank **out)
{
	if (!ctx || !g || !o || !out) return EDISON_E_ARGUMENT;
	*out = NULL;
	if (n_mics < 1 || n_mics > ED_FLOAT_BANK_MAX_MICS) return bank_err(ctx, who, EDISON_E_ARGUMENT, "n_mics must be 1 .. 4096");
	if (o->q15 != 0 && o->q15 != 1) return bank_err(ctx, who, EDISON_E_ARGUMENT, "q15 is 0 or 1");
	if (ed_ctx_fnet_layered(ctx)) return ed_fnet_refuse_layered(ctx, who); /* the window launches are the in-LDS kernels' */
	int F = 0;
	/* the batch call's checks: clip range, geometry (q15 = 1: the shipped framing), a float network loaded, F * num_mfcc = its input */
	{ const int r = ed_kws_float_geom_check(ctx, g, o->q15, o->clip_lo, o->clip_hi, &F); if (r != EDISON_OK) return r; }
	if (o->q15 && !ctx->d_q15)
	{
		snprintf(ctx->err, sizeof(ctx->err), "%s: MFCC variant C is not available for the configured filterbank: %s", who,
		         ctx->q15_err[0] ? ctx->q15_err : "tables not built");
		return EDISON_E_NO_IMPL;
	}
	const int n_out = ed_ctx_fnet_plan(ctx)->n_out;
	const ed_stream_core_opts co = {o->chunk_frames, o->filter, o->fsm, o->filter_alpha, o->true_threshold};
	{ const int r = ed_stream_core_check_opts(ctx, who, g, &co); if (r != EDISON_OK) return r; }
	if (o->filter && n_out > EDSG_FILTER_MAX_OUT) return bank_err(ctx, who, EDISON_E_NO_IMPL, "the output filter serves networks of at most 256 outputs");
	if (o->fsm && n_out != EDISON_NET_OUT)
		return bank_err(ctx, who, EDISON_E_NO_IMPL, "the state machine needs a network with 10 outputs (the keyword list its roles index)");
	/* the feature and network launches count n_mics * chunk_frames frames in an int32 */
	if ((int64_t)n_mics * o->chunk_frames >= ((int64_t)1 << 31))
		return bank_err(ctx, who, EDISON_E_SIZE, "n_mics x chunk_frames must stay below 2^31 frames per push");

	edison_float_bank *b = new (std::nothrow) edison_float_bank();
	if (!b) return bank_err(ctx, who, EDISON_E_NO_MEMORY, "host allocation failed");
	b->noun = noun;
	b->q15 = o->q15;
	b->scale = (float)g->net_input_scale; b->lo = o->clip_lo; b->hi = o->clip_hi;
	b->fnet_epoch = ctx->fnet_epoch;
	const size_t entries = (size_t)o->chunk_frames * n_mics;
	b->off_probs = entries * n_out * sizeof(float);                           /* logits at 0 */
	b->off_argmax = 2 * b->off_probs;
	int r = ed_stream_core_create(&b->core, ctx, who, sizeof(float), sizeof(float), g, F, n_out, n_mics, &co,
	                              b->off_argmax + entries * sizeof(int32_t));
	if (r == EDISON_OK && !b->q15) r = ed_geom_tables_build(ctx, g, &b->tab);
	if (r == EDISON_OK && b->q15 && n_mics > 1 && hipMalloc((void **)&b->d_rows, sizeof(float) * entries * g->num_mfcc) != hipSuccess)
	{
		(void)hipGetLastError();
		r = bank_err(ctx, who, EDISON_E_NO_MEMORY, "allocation failed");
	}
	if (r != EDISON_OK) { edison_float_bank_destroy(b); return r; }
	if (!b->q15)
	{
		b->margs = b->tab.tmpl;
		b->margs.utt_stride = 0;
		b->margs.frame_step = g->frame_step;
		b->margs.take_log = (g->variant & 0xff) == EDISON_MFCC_A || (g->variant & EDISON_MFCC_USE_LOG);
		b->margs.feat = NULL;
	}
	*out = b;
	return EDISON_OK;
}

extern "C" int edison_float_bank_create(edison_ctx *ctx, const edison_kws_geom *g, const edison_float_bank_opts *o, edison_float_bank **out)
{
	return create(ctx, "float_bank", "bank", g, o ? &o->stream : NULL, o ? o->n_mics : 0, out);
}

extern "C" int edison_fbank_push_present_n_dev(edison_float_bank *b, const int16_t *samples, const uint8_t *present, int n_frames, float *logits,
                                               float *probs, int32_t *argmax)
{
	{ const int r = check_push(b, samples); if (r != EDISON_OK) return r; }
	ed_stream_core *c = &b->core;
	hipStream_t q = c->ctx->stream;
	{ const int r = ed_stream_core_begin_push(c, q, samples, n_frames, 0); if (r != EDISON_OK) return r; }
	/* the filter's input: the caller's probs where given, else the bank's block */
	if (c->filter && !probs) probs = (float *)(c->d_out + b->off_probs);
	return enqueue_push(b, q, n_frames, logits, probs, argmax, 0, present);
}

extern "C" int edison_float_bank_push_n_dev(edison_float_bank *b, const int16_t *samples, int n_frames, float *logits, float *probs, int32_t *argmax)
{
	return edison_fbank_push_present_n_dev(b, samples, NULL, n_frames, logits, probs, argmax);
}

extern "C" int edison_float_bank_push_dev(edison_float_bank *b, const int16_t *samples, float *logits, float *probs, int32_t *argmax)
{
	return edison_float_bank_push_n_dev(b, samples, b ? b->core.chunk : 0, logits, probs, argmax);
}

/* host pointers: one upload from pinned memory (strided for several microphones), the same launches on the private stream, one download of the output block, one wait */
extern "C" int edison_fbank_push_present(edison_float_bank *b, const int16_t *samples, const uint8_t *present, float *logits, float *probs,
                                         int32_t *argmax)
{
	{ const int r = check_push(b, samples); if (r != EDISON_OK) return r; }
	ed_stream_core *c = &b->core;
	hipStream_t q = c->own;
	{ const int r = ed_stream_core_begin_push(c, q, samples, c->chunk, 1); if (r != EDISON_OK) return r; }
	{
		const int r = enqueue_push(b, q, c->chunk, (float *)c->d_out, (float *)(c->d_out + b->off_probs), (int32_t *)(c->d_out + b->off_argmax), 1, present);
		if (r != EDISON_OK) return r;
	}
	const size_t fb = b->off_probs; /* chunk * n_mics * n_out floats */
	if (logits) memcpy(logits, c->h_out, fb);
	if (probs) memcpy(probs, c->h_out + fb, fb);
	if (argmax) memcpy(argmax, c->h_out + b->off_argmax, (size_t)c->chunk * c->n_mics * sizeof(int32_t));
	return EDISON_OK;
}

extern "C" int edison_float_bank_push(edison_float_bank *b, const int16_t *samples, float *logits, float *probs, int32_t *argmax)
{
	return edison_fbank_push_present(b, samples, NULL, logits, probs, argmax);
}

extern "C" int edison_fbank_frames_seen_mics(edison_float_bank *b, int64_t *counts) { return ed_stream_core_frames_seen_mics(core_of(b), counts); }

extern "C" int edison_float_bank_frames_seen(edison_float_bank *b, int64_t *out)
{
	if (!b || !out) return EDISON_E_ARGUMENT;
	*out = b->core.frames_seen;
	return EDISON_OK;
}

extern "C" int edison_float_bank_filtered(edison_float_bank *b, float *filt, int32_t *likely, int32_t *spotted)
{
	return ed_stream_core_filtered(core_of(b), filt, likely, spotted, 1);
}

extern "C" int edison_float_bank_filtered_dev(edison_float_bank *b, float *filt, int32_t *likely, int32_t *spotted)
{
	return ed_stream_core_filtered(core_of(b), filt, likely, spotted, 0);
}

extern "C" int edison_float_bank_fsm(edison_float_bank *b, edison_fsm *fsm, int32_t *states) { return ed_stream_core_fsm(core_of(b), fsm, states, 1); }
extern "C" int edison_float_bank_fsm_dev(edison_float_bank *b, edison_fsm *fsm, int32_t *states) { return ed_stream_core_fsm(core_of(b), fsm, states, 0); }

/* Not in the public header: tools/bench_float_bank.py's switch between the bank's one network launch per push (0, what the library
 * does) and one ed_launch_fnet per frame of the push (1), the same outputs by n launches. */
extern "C" int ed_float_bank_tool_per_frame(edison_float_bank *b, int on)
{
	if (!b) return EDISON_E_ARGUMENT;
	b->per_frame = on ? 1 : 0;
	return EDISON_OK;
}

/* ---- edison_stream_float_*: the bank of one microphone, created with the prefix "stream_float" and the noun "stream" */
extern "C" int edison_stream_float_create(edison_ctx *ctx, const edison_kws_geom *g, const edison_stream_float_opts *o, edison_stream_float **out)
{
	return create(ctx, "stream_float", "stream", g, o, 1, (edison_float_bank **)out);
}

extern "C" void edison_stream_float_destroy(edison_stream_float *s) { edison_float_bank_destroy(bank_of(s)); }
extern "C" int edison_stream_float_reset(edison_stream_float *s) { return edison_float_bank_reset(bank_of(s)); }

extern "C" int edison_stream_float_push(edison_stream_float *s, const int16_t *samples, float *logits, float *probs, int32_t *argmax)
{
	return edison_fbank_push_present(bank_of(s), samples, NULL, logits, probs, argmax);
}

extern "C" int edison_stream_float_push_dev(edison_stream_float *s, const int16_t *samples, float *logits, float *probs, int32_t *argmax)
{
	return edison_float_bank_push_dev(bank_of(s), samples, logits, probs, argmax);
}

extern "C" int edison_stream_float_push_n_dev(edison_stream_float *s, const int16_t *samples, int n_frames, float *logits, float *probs,
                                              int32_t *argmax)
{
	return edison_fbank_push_present_n_dev(bank_of(s), samples, NULL, n_frames, logits, probs, argmax);
}

extern "C" int64_t edison_stream_float_frames_seen(const edison_stream_float *s) { return s ? bank_of(s)->core.frames_seen : -1; }

extern "C" int edison_stream_float_filtered(edison_stream_float *s, float *filt, int32_t *likely, int32_t *spotted)
{
	return edison_float_bank_filtered(bank_of(s), filt, likely, spotted);
}

extern "C" int edison_stream_float_filtered_dev(edison_stream_float *s, float *filt, int32_t *likely, int32_t *spotted)
{
	return edison_float_bank_filtered_dev(bank_of(s), filt, likely, spotted);
}

extern "C" int edison_stream_float_fsm(edison_stream_float *s, edison_fsm *fsm, int32_t *states) { return edison_float_bank_fsm(bank_of(s), fsm, states); }
extern "C" int edison_stream_float_fsm_dev(edison_stream_float *s, int32_t *states) { return edison_float_bank_fsm_dev(bank_of(s), NULL, states); }
