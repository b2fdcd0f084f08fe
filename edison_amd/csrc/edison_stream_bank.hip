/*
 * edison_stream_bank.hip -- a bank of continuous streams (include/edison_hip.h, edison_stream_bank_*): n_mics
 * microphones at one MFCC geometry on the graph loaded on the context, advancing in lockstep. Microphone m behaves as an
 * edison_stream_geom of its own fed microphone m's samples; a push of n frames for all of them runs
 *
 *     [banked shift, only when the push would not fit] -> one strided upload -> ONE MFCC launch over n_mics * n frames
 *     -> n network launches (one per frame of the push, each over the n_mics windows of that frame) -> [ONE banked filter (+ edisonFSM)]
 *
 * on the sliding-window core with n_mics microphones (edison_stream_core.h): a number of launches that does not depend on n_mics. The
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

/* The banked shift: workgroup m moves microphone m's history -- the newest `tail` samples from a_src and feat_bytes bytes from f_src --
 * to the front of its buffers, a_stride samples and f_stride bytes behind microphone m - 1's. The rounds are those of
 * ed_stream_geom_shift_kernel (edison_stream_core.hip): the destination lies below the source and may overlap it, so in rounds of 256
 * elements every lane reads, the workgroup waits, every lane writes. */
__global__ __launch_bounds__(256) void ed_stream_bank_shift_kernel(int16_t *audio, int64_t a_stride, int64_t a_src, int tail, int8_t *feat,
                                                                   int64_t f_stride, int64_t f_src, int feat_bytes)
{
	const int t = threadIdx.x;
	audio += (int64_t)blockIdx.x * a_stride;
	feat += (int64_t)blockIdx.x * f_stride;
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

/* The banked filter: workgroup m runs the firmware's post-processing for microphone m with the arithmetic of
 * ed_stream_geom_filter_kernel (edison_stream_core.hip) -- product and sum rounded separately in double, no contraction, first maximum,
 * edisonFSM on lane 0. Entry i of microphone m is row i * n_mics + m of the time-major arrays x / filt [n][n_mics][n_out] and likely /
 * spotted / fs.states [n][n_mics]; between pushes it keeps state [n_mics][n_out] and fs.fsm [n_mics]. T = int8_t: the int8 graph's softmax
 * / logits (this file's bank); T = float: the float network's probabilities (edison_float_bank.hip). (double)x is exact for both. */
template <class T>
__global__ __launch_bounds__(256) void ed_stream_bank_filter_kernel(const T *x, int n, int n_out, double alpha, double one_minus_alpha,
                                                                    double threshold, float *state, float *filt, int32_t *likely,
                                                                    int32_t *spotted, edsg_fsm_stage_t fs)
{
	const int t = threadIdx.x;
	const size_t m = blockIdx.x, n_mics = gridDim.x;
	if (t < n_out)
	{
		float y = state[m * n_out + t];
		for (int i = 0; i < n; i++)
		{
			/* the compiler's default contraction would fuse these into one v_fma_f64 (the Cortex-M4 rounds each operation) */
#pragma clang fp contract(off)
			const size_t at = (i * n_mics + m) * n_out + t;
			const double a = alpha * (double)y;
			const double b = one_minus_alpha * (double)x[at];
			y = (float)(a + b);
			filt[at] = y;
		}
		state[m * n_out + t] = y;
	}
	__syncthreads();
	for (int i = t; i < n; i += 256)
	{
		const size_t im = i * n_mics + m;
		const float *row = filt + im * n_out;
		float best = row[0];
		int idx = 0;
		for (int c = 1; c < n_out; c++)
			if (best < row[c]) { best = row[c]; idx = c; }
		likely[im] = idx;
		spotted[im] = ((double)best > threshold) ? idx : -1;
	}
	if (!fs.fsm) return;
	__syncthreads();
	if (t == 0)
	{
		edison_fsm mach = fs.fsm[m];
		for (int i = 0; i < n; i++)
		{
			const size_t im = i * n_mics + m;
			fs.states[im] = ed_fsm_step_core(&mach, spotted[im] >= 0, (uint32_t)likely[im], fs.dt_us, &fs.roles);
		}
		fs.fsm[m] = mach;
		if (fs.copy) fs.copy[m] = mach;
	}
}

void ed_stream_bank_launch_shift(hipStream_t q, int n_mics, int16_t *audio, int64_t a_stride, int64_t a_src, int tail, int8_t *feat, int64_t f_stride,
                                 int64_t f_src, int feat_bytes)
{
	hipLaunchKernelGGL(ed_stream_bank_shift_kernel, dim3(n_mics), dim3(256), 0, q, audio, a_stride, a_src, tail, feat, f_stride, f_src, feat_bytes);
}

void ed_stream_bank_launch_filter(hipStream_t q, int n_mics, int out_elem, const void *x, int n, int n_out, double alpha, double one_minus_alpha,
                                  double threshold, float *state, float *filt, int32_t *likely, int32_t *spotted, edsg_fsm_stage_t fs)
{
	if (out_elem == 1)
		hipLaunchKernelGGL(ed_stream_bank_filter_kernel<int8_t>, dim3(n_mics), dim3(256), 0, q, (const int8_t *)x, n, n_out, alpha, one_minus_alpha,
		                   threshold, state, filt, likely, spotted, fs);
	else
		hipLaunchKernelGGL(ed_stream_bank_filter_kernel<float>, dim3(n_mics), dim3(256), 0, q, (const float *)x, n, n_out, alpha, one_minus_alpha,
		                   threshold, state, filt, likely, spotted, fs);
}

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
