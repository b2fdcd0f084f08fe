/*
 * edison_q15.hip -- C-ABI entry points of MFCC variant C, the firmware's fixed-point audioCalcMFCCs
 * (firmware/src/audioprocessing.c:116-215), with its native int16 outputs. See include/edison_hip.h.
 * The kernel is mfcc_q15_kernels.hip; the tables are tables_q15.c. No CPU path.
 */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "edison_ctx.h"

int ed_ctx_mfcc_q15_launch(edison_ctx *ctx, const int16_t *audio, int64_t n_frames, int64_t fpg, int64_t group_stride,
                           int64_t frame_step, int n_coef, int16_t *mfcc_i16, float *mfcc_f32, int8_t *feat, int stages,
                           int16_t *fft, int16_t *spec, int16_t *mel)
{
	if (!ctx) return EDISON_E_ARGUMENT;
	return ed_ctx_mfcc_q15_launch_on(ctx, ctx->stream, audio, n_frames, fpg, group_stride, frame_step, n_coef, mfcc_i16, mfcc_f32, feat,
	                                 stages, fft, spec, mel);
}

int ed_ctx_mfcc_q15_launch_on(edison_ctx *ctx, hipStream_t stream, const int16_t *audio, int64_t n_frames, int64_t fpg, int64_t group_stride,
                              int64_t frame_step, int n_coef, int16_t *mfcc_i16, float *mfcc_f32, int8_t *feat, int stages,
                              int16_t *fft, int16_t *spec, int16_t *mel)
{
	if (!ctx || (!audio && n_frames > 0)) return EDISON_E_ARGUMENT;
	if (n_coef < 1 || n_coef > EDISON_NUM_MEL) return ed_set_err(ctx, EDISON_E_ARGUMENT, "n_coef must be 1..32");
	if (n_frames < 0 || n_frames >= ((int64_t)1 << 31) || frame_step < 0 || fpg < 1)
		return ed_set_err(ctx, EDISON_E_ARGUMENT, "bad frame count / step");
	if (!ctx->d_q15)
	{
		snprintf(ctx->err, sizeof(ctx->err), "MFCC variant C is not available for the configured filterbank: %s",
		         ctx->q15_err[0] ? ctx->q15_err : "tables not built");
		return EDISON_E_NO_IMPL;
	}
	if (n_frames == 0) return EDISON_OK;
	ed_mfcc_q15_args_t a;
	memset(&a, 0, sizeof(a));
	a.audio = audio; a.n_frames = n_frames; a.frames_per_group = fpg; a.group_stride = group_stride;
	a.frame_step = frame_step; a.n_coef = n_coef;
	a.mfcc_i16 = mfcc_i16; a.mfcc_f32 = mfcc_f32; a.feat = feat;
	a.fft = fft; a.spec = spec; a.mel = mel;
	int e = ed_launch_mfcc_q15(&a, ctx->d_q15, ctx->q15_nlo, ctx->q15_nhi, stages, ctx->n_cu, stream);
	return ed_launch_result(ctx, e, "Q15 MFCC kernel");
}

extern "C" int edison_mfcc_q15_batch_dev(edison_ctx *ctx, const int16_t *audio, int64_t n_frames, int64_t frame_step,
                                         int n_coef, int16_t *mfcc, int8_t *feat)
{
	return ed_ctx_mfcc_q15_launch(ctx, audio, n_frames, n_frames > 0 ? n_frames : 1, 0, frame_step, n_coef, mfcc, NULL,
	                              feat, 0, NULL, NULL, NULL);
}

extern "C" int edison_mfcc_q15_stages_dev(edison_ctx *ctx, const int16_t *audio, int64_t n_frames, int64_t frame_step,
                                          int16_t *fft, int16_t *spec, int16_t *mel, int16_t *mfcc32)
{
	return ed_ctx_mfcc_q15_launch(ctx, audio, n_frames, n_frames > 0 ? n_frames : 1, 0, frame_step, EDISON_NUM_MEL,
	                              mfcc32, NULL, NULL, 1, fft, spec, mel);
}

/* ------------------------------------------------------------------------------------------ host pointers */
static int q15_host(edison_ctx *ctx, const int16_t *audio, int64_t n_frames, int64_t frame_step, int n_coef, int stages,
                    int16_t *mfcc, int8_t *feat, int16_t *fft, int16_t *spec, int16_t *mel)
{
	if (!ctx || n_frames < 0 || (!audio && n_frames > 0) || frame_step < 0) return EDISON_E_ARGUMENT;
	if (n_frames == 0) return EDISON_OK;
	if (n_coef < 1 || n_coef > EDISON_NUM_MEL) return ed_set_err(ctx, EDISON_E_ARGUMENT, "n_coef must be 1..32");
	ed_staging st(ctx);
	const size_t n = (size_t)n_frames;
	const int16_t *a = st.in(audio, (size_t)(n_frames - 1) * (size_t)frame_step + EDISON_FRAME_LEN);
	int16_t *m = st.out(mfcc, n * n_coef), *f = st.out(fft, n * 513 * 2), *s = st.out(spec, n * 513), *l = st.out(mel, n * 32);
	int8_t *q = st.out(feat, n * n_coef);
	return st.finish(st.ok() ? ed_ctx_mfcc_q15_launch(ctx, a, n_frames, n_frames, 0, frame_step, n_coef, m, NULL, q, stages, f, s, l) : EDISON_OK);
}

extern "C" int edison_mfcc_q15_batch(edison_ctx *ctx, const int16_t *audio, int64_t n_frames, int64_t frame_step,
                                     int n_coef, int16_t *mfcc, int8_t *feat)
{
	return q15_host(ctx, audio, n_frames, frame_step, n_coef, 0, mfcc, feat, NULL, NULL, NULL);
}

extern "C" int edison_mfcc_q15_stages(edison_ctx *ctx, const int16_t *audio, int64_t n_frames, int64_t frame_step,
                                      int16_t *fft, int16_t *spec, int16_t *mel, int16_t *mfcc32)
{
	return q15_host(ctx, audio, n_frames, frame_step, EDISON_NUM_MEL, 1, mfcc32, NULL, fft, spec, mel);
}
