/*
 * edison_kws_geom.hip -- keyword spotting for a graph trained at any MFCC geometry: audio -> int8 features (mfcc_geom_kernels.hip,
 * float64) -> the loaded graph on the network kernel that serves it today (edison_net_batch_dev), in one call
 * (include/edison_hip.h, edison_kws_geom_batch*). The filterbank, twiddle and DCT tables of one geometry are cached in the context:
 * a call at the cached geometry allocates nothing and does not synchronise; a call at another geometry synchronises the stream once,
 * frees the old tables and uploads the new ones. Independent of edison_mfcc_configure (the geometry carries its own filterbank).
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "edison_ctx.h"
#include "mfcc_geom.h"

#define EDG_WAVE_TEAM_BYTES 20480 /* a frame's LDS slice that still runs on one wavefront (mfcc_geom_kernels.hip) */

extern "C" void edison_kws_geom_default(edison_kws_geom *g)
{
	if (!g) return;
	memset(g, 0, sizeof(*g));
	/* audio/config.py:11-43: 2 s at 16 kHz, frame = hop = 1024, 32 mel bins 80 .. 7600 Hz, first 13 coefficients, scale 1 */
	g->variant = EDISON_MFCC_B;
	g->frame_len = EDISON_FRAME_LEN;
	g->frame_step = EDISON_FRAME_LEN;
	g->n_samples = 2 * EDISON_FS;
	g->frame_count = 0;
	g->mel_nbins = EDISON_NUM_MEL;
	g->first_mfcc = 0;
	g->num_mfcc = EDISON_NUM_MFCC;
	g->sample_rate = EDISON_FS;
	g->lower_edge_hertz = 80.0;
	g->upper_edge_hertz = 7600.0;
	g->mel_mtx_scale = 128.0;
	g->net_input_scale = 1.0;
}

void ed_ctx_geom_free(edison_ctx *ctx)
{
	if (!ctx || !ctx->geom) return;
	if (ctx->geom->d) (void)hipFree(ctx->geom->d);
	delete ctx->geom;
	ctx->geom = NULL;
}

/* Checks everything but the model; *frames = frames per utterance. */
int ed_kws_geom_check(edison_ctx *ctx, const edison_kws_geom *g, int *frames)
{
	const int v = g->variant & 0xff;
	if (v != EDISON_MFCC_A && v != EDISON_MFCC_B) return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_kws_geom: variants A and B (TF and C are not on this path)");
	if (g->variant & ~(0xff | EDISON_MFCC_USE_LOG)) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_kws_geom: unknown variant flags");
	if (v == EDISON_MFCC_A && (g->variant & EDISON_MFCC_USE_LOG)) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_kws_geom: variant A always takes the logarithm");
	if (g->frame_len < 4 || g->frame_len > ED_GEN_MAX_FRAME) return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_kws_geom: frame_len 4 .. 4096");
	if (g->mel_nbins < 1 || g->mel_nbins > ED_GEN_MAX_MEL) return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_kws_geom: mel_nbins 1 .. 256");
	if (g->frame_step < 1) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_kws_geom: frame_step >= 1");
	if (g->n_samples < g->frame_len) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_kws_geom: n_samples < frame_len");
	if (g->frame_count < 0) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_kws_geom: negative frame_count");
	const int64_t F = g->frame_count ? g->frame_count : 1 + (g->n_samples - g->frame_len) / g->frame_step;
	if ((F - 1) * (int64_t)g->frame_step + g->frame_len > g->n_samples)
		return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_kws_geom: frame_count frames do not fit in n_samples");
	if (g->first_mfcc < 0 || g->num_mfcc < 1 || g->first_mfcc + g->num_mfcc > g->mel_nbins)
		return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_kws_geom: needs 0 <= first_mfcc, 1 <= num_mfcc, first_mfcc + num_mfcc <= mel_nbins");
	if (!(g->sample_rate > 0) || !(g->lower_edge_hertz >= 0) || !(g->upper_edge_hertz > g->lower_edge_hertz) || !(g->mel_mtx_scale > 0) ||
	    !isfinite(g->sample_rate) || !isfinite(g->upper_edge_hertz) || !isfinite(g->mel_mtx_scale) || !isfinite(g->net_input_scale))
		return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_kws_geom: bad filterbank edges / scales");
	*frames = (int)F;
	return EDISON_OK;
}

/* Radices 4, then 2, 3, 5 whose product is M; 0 when M has another prime factor. */
static int plan_radices(int M, int32_t *radix)
{
	int n = 0;
	while (M % 4 == 0) { radix[n++] = 4; M /= 4; }
	while (M % 2 == 0) { radix[n++] = 2; M /= 2; }
	while (M % 3 == 0) { radix[n++] = 3; M /= 3; }
	while (M % 5 == 0) { radix[n++] = 5; M /= 5; }
	return M == 1 ? n : 0;
}

static bool geom_key_matches(const ed_geom_cache *c, const edison_kws_geom *g)
{
	return c->variant == (g->variant & 0xff) && c->N == g->frame_len && c->n_mel == g->mel_nbins && c->first == g->first_mfcc &&
	       c->num == g->num_mfcc && c->fs == g->sample_rate && c->lo == g->lower_edge_hertz && c->hi == g->upper_edge_hertz &&
	       c->scale == g->mel_mtx_scale;
}

/* Builds the tables of g's geometry into *c (key, device block, launch template); c->d must be NULL on entry. On failure c->d stays
 * NULL. Synchronous (one upload from pageable memory). */
int ed_geom_tables_build(edison_ctx *ctx, const edison_kws_geom *g, ed_geom_cache *c)
{
	const int v = g->variant & 0xff, N = g->frame_len, nm = g->mel_nbins, first = g->first_mfcc, num = g->num_mfcc;
	const int nb = v == EDISON_MFCC_A ? N / 2 : N / 2 + 1;
	double *W = (double *)malloc(sizeof(double) * (size_t)nb * nm);
	if (!W) return ed_set_err(ctx, EDISON_E_NO_MEMORY, "host allocation failed");
	int r = ed_gen_mel_weight_matrix(nm, nb, g->sample_rate, g->lower_edge_hertz, g->upper_edge_hertz, W);
	if (r != EDISON_OK) { free(W); return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_kws_geom: mel matrix (needs >= 2 spectrum bins, >= 1 mel bin)"); }
	/* each band's nonzero run (triangular filters: one run; an interior zero would only add 0) */
	int32_t *band = (int32_t *)malloc(sizeof(int32_t) * 3 * (size_t)nm);
	if (!band) { free(W); return ed_set_err(ctx, EDISON_E_NO_MEMORY, "host allocation failed"); }
	size_t n_taps = 0;
	for (int j = 0; j < nm; j++)
	{
		int k0 = -1, k1 = -1;
		for (int k = 0; k < nb; k++)
			if (W[(size_t)k * nm + j] != 0.0) { if (k0 < 0) k0 = k; k1 = k; }
		band[3 * j] = k0 < 0 ? 0 : k0;
		band[3 * j + 1] = k0 < 0 ? 0 : k1 - k0 + 1;
		band[3 * j + 2] = (int32_t)n_taps;
		n_taps += (size_t)band[3 * j + 1];
	}
	const size_t n_tw = 2 * (size_t)N, n_dct = (size_t)num * nm;
	const size_t bytes = sizeof(double) * (n_tw + n_taps + n_dct) + sizeof(int32_t) * 3 * (size_t)nm;
	double *h = (double *)malloc(bytes);
	if (!h) { free(W); free(band); return ed_set_err(ctx, EDISON_E_NO_MEMORY, "host allocation failed"); }
	for (int j = 0; j < N; j++)
	{
		const double ang = 2.0 * M_PI * (double)j / (double)N;
		h[2 * j] = cos(ang);
		h[2 * j + 1] = -sin(ang);
	}
	double *taps = h + n_tw;
	for (int j = 0; j < nm; j++)
		for (int t = 0; t < band[3 * j + 1]; t++)
		{
			const double w = W[(size_t)(band[3 * j] + t) * nm + j];
			taps[band[3 * j + 2] + t] = v == EDISON_MFCC_B ? g->mel_mtx_scale * w : w; /* mfcc_utils.py:281-284 */
		}
	double *dct = taps + n_taps;
	for (int c2 = 0; c2 < num; c2++)
		for (int n = 0; n < nm; n++)
			dct[(size_t)c2 * nm + n] = 2.0 * cos(M_PI * (double)(first + c2) * (double)(2 * n + 1) / (double)(2 * nm));
	memcpy(dct + n_dct, band, sizeof(int32_t) * 3 * (size_t)nm);
	free(W);
	free(band);

	hipError_t e = hipMalloc(&c->d, bytes);
	if (e == hipSuccess) e = hipMemcpy(c->d, h, bytes, hipMemcpyHostToDevice);
	free(h);
	if (e != hipSuccess)
	{
		if (c->d) (void)hipFree(c->d);
		c->d = NULL;
		if (e == hipErrorOutOfMemory) return ed_set_err(ctx, EDISON_E_NO_MEMORY, "edison_kws_geom: table hipMalloc: out of HBM");
		ED_HIP(ctx, e);
	}
	c->variant = v; c->N = N; c->n_mel = nm; c->first = first; c->num = num;
	c->fs = g->sample_rate; c->lo = g->lower_edge_hertz; c->hi = g->upper_edge_hertz; c->scale = g->mel_mtx_scale;

	ed_geom_args_t &a = c->tmpl;
	memset(&a, 0, sizeof(a));
	a.N = N;
	a.packed = N % 2 == 0;
	const int M = a.packed ? N / 2 : N;
	a.n_stages = plan_radices(M, a.radix);
	a.M = a.n_stages > 0 ? M : 0; /* a prime factor above 5: the direct DFT */
	a.n_bins = nb;
	a.n_mel = nm;
	a.n_coef = num;
	if (a.M > 0) a.r0 = a.r1 = 2 * M;                              /* two FFT buffers of M complex points   */
	else { a.r0 = (N + 1) & ~1; a.r1 = (nb + 1) & ~1; }            /* the samples, the spectrum            */
	a.r2 = (nm + 1) & ~1;                                           /* the mel bands                        */
	a.team = sizeof(double) * (size_t)(a.r0 + a.r1 + a.r2) <= EDG_WAVE_TEAM_BYTES ? 64 : 256;
	const bool b = v == EDISON_MFCC_B; /* mfcc_utils.py:170-196 (A), :296-319 (B); the generic kernel's constants */
	a.fft_scale = b ? 1.0 / 1024.0 : 1.0;
	a.spec_scale = b ? 1.0 / sqrt(2.0) : 1.0;
	a.mel_div = b ? g->mel_mtx_scale : 1.0;
	a.dct_div = b ? 64.0 : sqrt(2.0 * (double)nm);
	double *d = (double *)c->d;
	a.tw = d;
	a.taps = d + n_tw;
	a.dct = d + n_tw + n_taps;
	a.band = (const int32_t *)(d + n_tw + n_taps + n_dct);
	return EDISON_OK;
}

/* The context's cached tables of g's geometry: kept when the key matches, else rebuilt (after one synchronisation, so no queued launch
 * still reads the old block). */
static int geom_tables(edison_ctx *ctx, const edison_kws_geom *g, const ed_geom_cache **out)
{
	ed_geom_cache *c = ctx->geom;
	if (c && geom_key_matches(c, g))
	{
		*out = c;
		return EDISON_OK;
	}
	ed_geom_cache *nc = new (std::nothrow) ed_geom_cache();
	if (!nc) return ed_set_err(ctx, EDISON_E_NO_MEMORY, "host allocation failed");
	{ const int r = ed_geom_tables_build(ctx, g, nc); if (r != EDISON_OK) { delete nc; return r; } }
	/* the old block may still be read by queued launches */
	if (c)
	{
		const hipError_t e = hipStreamSynchronize(ctx->stream);
		if (e != hipSuccess) { (void)hipFree(nc->d); delete nc; ED_HIP(ctx, e); }
		ed_ctx_geom_free(ctx);
	}
	ctx->geom = nc;
	*out = nc;
	return EDISON_OK;
}

/* Argument and geometry checks shared by every form; *frames = frames per utterance. */
static int check_audio(edison_ctx *ctx, const edison_kws_geom *g, const int16_t *audio, int64_t n_utt, int64_t utt_stride, int *frames)
{
	if (!ctx || !g || n_utt < 0 || (!audio && n_utt > 0)) return EDISON_E_ARGUMENT;
	if (utt_stride < 0) return ed_set_err(ctx, EDISON_E_ARGUMENT, "negative utterance stride");
	return ed_kws_geom_check(ctx, g, frames);
}

static int check_n_frames(edison_ctx *ctx, int64_t n_utt, int frames)
{
	if (n_utt * (int64_t)frames >= ((int64_t)1 << 31)) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_kws_geom: more than 2^31 frames in one call");
	return EDISON_OK;
}

/* Argument, geometry and model checks shared by both forms of edison_kws_geom_batch; *frames = frames per utterance. */
static int check_call(edison_ctx *ctx, const edison_kws_geom *g, const int16_t *audio, int64_t n_utt, int64_t utt_stride, int *frames)
{
	{ const int r = check_audio(ctx, g, audio, n_utt, utt_stride, frames); if (r != EDISON_OK) return r; }
	if (!ctx->have_model) return ed_set_err(ctx, EDISON_E_NO_MODEL, "no CNN model loaded (edison_model_load)");
	const int64_t n_feat = (int64_t)*frames * g->num_mfcc;
	if (n_feat != ctx->net.in_n)
	{
		snprintf(ctx->err, sizeof(ctx->err), "edison_kws_geom: frame_count x num_mfcc = %lld features, the graph's input in_h x in_w x in_c = %d",
		         (long long)n_feat, ctx->net.in_n);
		return EDISON_E_SIZE;
	}
	return check_n_frames(ctx, n_utt, *frames);
}

/* edison_mfcc_geom_batch*: no model; mfcc must be given when there is anything to compute. */
static int check_mfcc_call(edison_ctx *ctx, const edison_kws_geom *g, const int16_t *audio, int64_t n_utt, int64_t utt_stride, const double *mfcc,
                           int *frames)
{
	{ const int r = check_audio(ctx, g, audio, n_utt, utt_stride, frames); if (r != EDISON_OK) return r; }
	if (!mfcc && n_utt > 0) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_mfcc_geom_batch: mfcc is NULL");
	return check_n_frames(ctx, n_utt, *frames);
}

/* The kernel's arguments for n_utt utterances of F frames at g, on the cached tables c (feat / feat_scale left to the caller). */
static ed_geom_args_t launch_args(const ed_geom_cache *c, const edison_kws_geom *g, const int16_t *audio, int64_t n_utt, int64_t utt_stride, int F)
{
	ed_geom_args_t a = c->tmpl;
	a.audio = audio;
	a.utt_stride = utt_stride;
	a.frame_step = g->frame_step;
	a.frames_per_utt = F;
	a.n_frames = (int32_t)(n_utt * F);
	a.take_log = (g->variant & 0xff) == EDISON_MFCC_A || (g->variant & EDISON_MFCC_USE_LOG);
	return a;
}

/* Samples a host-pointer call stages: (n_utt - 1) * utt_stride + the frames of one utterance, computed in 128 bits, refused beyond 2^46
 * samples (as edison_mfcc_rows). */
static int staged_samples(edison_ctx *ctx, const edison_kws_geom *g, int64_t n_utt, int64_t utt_stride, int F, const char *who, size_t *n)
{
	const unsigned __int128 na128 = (unsigned __int128)(n_utt - 1) * (unsigned __int128)utt_stride +
	                                (unsigned __int128)((int64_t)(F - 1) * g->frame_step + g->frame_len);
	if (na128 * sizeof(int16_t) > ((unsigned __int128)1 << 47))
	{
		snprintf(ctx->err, sizeof(ctx->err), "%s: utt_stride x n_utt too large", who);
		return EDISON_E_SIZE;
	}
	*n = (size_t)na128;
	return EDISON_OK;
}

extern "C" int edison_kws_geom_batch_dev(edison_ctx *ctx, const edison_kws_geom *g, const int16_t *audio, int64_t n_utt, int64_t utt_stride,
                                         int8_t *feat, int8_t *logits, int8_t *softmax, int32_t *argmax)
{
	int F = 0;
	{ const int r = check_call(ctx, g, audio, n_utt, utt_stride, &F); if (r != EDISON_OK) return r; }
	if (n_utt == 0) return EDISON_OK;
	ED_HIP(ctx, hipSetDevice(ctx->device));
	const ed_geom_cache *c = NULL;
	{ const int r = geom_tables(ctx, g, &c); if (r != EDISON_OK) return r; }
	int8_t *f = feat;
	if (!f)
	{
		const int r = ed_ctx_ensure_scratch(ctx, (size_t)n_utt * (size_t)ctx->net.in_n);
		if (r != EDISON_OK) return r;
		f = (int8_t *)ctx->scratch;
	}
	ed_geom_args_t a = launch_args(c, g, audio, n_utt, utt_stride, F);
	a.feat = f;
	a.feat_scale = (float)g->net_input_scale;
	const int e = ed_launch_mfcc_geom(&a, ctx->n_cu, ctx->stream);
	if (e != 0) return ed_launch_result(ctx, e, "MFCC geometry kernel");
	/* the graph on the kernel that serves it (edison_net_batch_dev); a graph without Softmax leaves `softmax` alone */
	return edison_net_batch_dev(ctx, f, n_utt, logits, ctx->net.has_softmax ? softmax : NULL, argmax);
}

extern "C" int edison_kws_geom_batch(edison_ctx *ctx, const edison_kws_geom *g, const int16_t *audio, int64_t n_utt, int64_t utt_stride,
                                     int8_t *feat, int8_t *logits, int8_t *softmax, int32_t *argmax)
{
	int F = 0;
	{ const int r = check_call(ctx, g, audio, n_utt, utt_stride, &F); if (r != EDISON_OK) return r; }
	if (n_utt == 0) return EDISON_OK;
	size_t na = 0;
	{ const int r = staged_samples(ctx, g, n_utt, utt_stride, F, "edison_kws_geom_batch", &na); if (r != EDISON_OK) return r; }
	const size_t n = (size_t)n_utt, out_n = (size_t)ctx->net.out_n;
	ed_staging st(ctx);
	const int16_t *au = st.in(audio, na);
	int8_t *f = st.scratch(feat, n * (size_t)ctx->net.in_n), *l = st.out(logits, n * out_n);
	int8_t *s = st.out(ctx->net.has_softmax ? softmax : (int8_t *)NULL, n * out_n);
	int32_t *am = st.out(argmax, n);
	return st.finish(st.ok() ? edison_kws_geom_batch_dev(ctx, g, au, n_utt, utt_stride, f, l, s, am) : EDISON_OK);
}

/* ---- float64 MFCC at any geometry: ed_mfcc_geom_kernel's frames and stages, y itself stored */
extern "C" int edison_mfcc_geom_batch_dev(edison_ctx *ctx, const edison_kws_geom *g, const int16_t *audio, int64_t n_utt, int64_t utt_stride,
                                          double *mfcc)
{
	int F = 0;
	{ const int r = check_mfcc_call(ctx, g, audio, n_utt, utt_stride, mfcc, &F); if (r != EDISON_OK) return r; }
	if (n_utt == 0) return EDISON_OK;
	ED_HIP(ctx, hipSetDevice(ctx->device));
	const ed_geom_cache *c = NULL;
	{ const int r = geom_tables(ctx, g, &c); if (r != EDISON_OK) return r; }
	const ed_geom_args_t a = launch_args(c, g, audio, n_utt, utt_stride, F);
	const int e = ed_launch_mfcc_geom_f64(&a, mfcc, ctx->n_cu, ctx->stream);
	return e != 0 ? ed_launch_result(ctx, e, "float64 MFCC geometry kernel") : EDISON_OK;
}

extern "C" int edison_mfcc_geom_batch(edison_ctx *ctx, const edison_kws_geom *g, const int16_t *audio, int64_t n_utt, int64_t utt_stride,
                                      double *mfcc)
{
	int F = 0;
	{ const int r = check_mfcc_call(ctx, g, audio, n_utt, utt_stride, mfcc, &F); if (r != EDISON_OK) return r; }
	if (n_utt == 0) return EDISON_OK;
	size_t na = 0;
	{ const int r = staged_samples(ctx, g, n_utt, utt_stride, F, "edison_mfcc_geom_batch", &na); if (r != EDISON_OK) return r; }
	ed_staging st(ctx);
	const int16_t *au = st.in(audio, na);
	double *m = st.out(mfcc, (size_t)n_utt * (size_t)F * (size_t)g->num_mfcc);
	return st.finish(st.ok() ? edison_mfcc_geom_batch_dev(ctx, g, au, n_utt, utt_stride, m) : EDISON_OK);
}
