/*
 * edison_fcal.hip -- the C-ABI of calibrating the loaded float32 network for quantisation (include/edison_hip.h, edison_fcal_*;
 * DESIGN.md section 18): a calibrator owns 64-bit counters in device memory (layout: fnet_calib.h) and its own copy of the network's
 * plan, sized with the statistic's LDS held back; every add is one launch of ed_fnet_calib_kernel on the context's stream, behind
 * whatever produced the inputs. Only edison_fcal_result synchronises. The calibrator serves the network of one load: after another
 * edison_fnet_load* its calls fail with EDISON_E_NO_MODEL.
 */
#include <stdlib.h>

#include <vector>

#include "edison_ctx.h"
#include "fnet_calib.h"

struct edison_fcal
{
	edison_ctx *ctx;
	int epoch;          /* the float network load (ctx->fnet_epoch) the plan belongs to */
	ed_fnet_plan_t plan; /* the network's plan at the calibrator's batch */
	size_t words;       /* (n_layers + 1) * EDFC_WORDS */
	unsigned long long *d_counters;
};

static int fcal_live(edison_fcal *c, const char *who)
{
	if (!c) return EDISON_E_ARGUMENT;
	if (c->epoch != c->ctx->fnet_epoch || !c->ctx->fnet)
	{
		snprintf(c->ctx->err, sizeof(c->ctx->err), "%s: another float network was loaded after this calibrator was created; create a new one", who);
		return EDISON_E_NO_MODEL;
	}
	return EDISON_OK;
}

extern "C" int edison_fcal_create(edison_ctx *ctx, edison_fcal **out)
{
	if (!ctx || !out) return EDISON_E_ARGUMENT;
	*out = NULL;
	const ed_fnet_plan_t *net = ed_ctx_fnet_plan(ctx);
	if (!net) return ed_set_err(ctx, EDISON_E_NO_MODEL, "no float network loaded (edison_fnet_load)");
	if (ed_ctx_fnet_layered(ctx)) return ed_fnet_refuse_layered(ctx, "edison_fcal_create");
	edison_fcal *c = (edison_fcal *)calloc(1, sizeof(*c));
	if (!c) return ed_set_err(ctx, EDISON_E_NO_MEMORY, "edison_fcal_create: out of host memory");
	c->ctx = ctx;
	c->epoch = ctx->fnet_epoch;
	c->plan = *net;
	/* utterances per workgroup: the network's own rule (edison_fnet.hip) with the histogram's bytes held back */
	const int64_t fixed = 4 * ((int64_t)net->w_lds + net->k_lds) + (int64_t)sizeof(uint32_t) * EDFC_LDS_WORDS;
	const int64_t per = 4 * ((int64_t)net->buf_n[0] + net->buf_n[1]);
	int64_t batch = (ED_FNET_LDS_BYTES - fixed) / per;
	if (batch > ED_FNET_MAX_BATCH) batch = ED_FNET_MAX_BATCH;
	if (batch < 1)
	{
		free(c);
		return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_fcal_create: one utterance, the largest layer and the histogram do not fit the LDS");
	}
	c->plan.batch = (int32_t)batch;
	c->words = (size_t)(net->n_layers + 1) * EDFC_WORDS;
	if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc((void **)&c->d_counters, c->words * sizeof(unsigned long long)) != hipSuccess)
	{
		free(c);
		return ed_set_err(ctx, EDISON_E_NO_MEMORY, "edison_fcal_create: cannot allocate the device counters");
	}
	/* zeroed before create returns: the caller may move the context to another stream before the first add */
	const int r = edison_fcal_reset(c) == EDISON_OK && hipStreamSynchronize(ctx->stream) == hipSuccess
	                  ? EDISON_OK
	                  : ed_set_err(ctx, EDISON_E_RUNTIME, "edison_fcal_create: cannot zero the device counters");
	if (r != EDISON_OK)
	{
		edison_fcal_destroy(c);
		return r;
	}
	*out = c;
	return EDISON_OK;
}

extern "C" void edison_fcal_destroy(edison_fcal *c)
{
	if (!c) return;
	(void)hipSetDevice(c->ctx->device);
	(void)hipStreamSynchronize(c->ctx->stream); /* an add may still be queued */
	if (c->d_counters) (void)hipFree(c->d_counters);
	free(c);
}

extern "C" int edison_fcal_info(edison_fcal *c, edison_fcal_info_t *out)
{
	if (!c || !out) return EDISON_E_ARGUMENT;
	{ const int r = fcal_live(c, "edison_fcal_info"); if (r != EDISON_OK) return r; }
	out->n_stats = c->plan.n_layers + 1;
	out->in_n = c->plan.in_n;
	out->batch = c->plan.batch;
	out->lds_bytes = (int32_t)ed_fnet_calib_lds_bytes(&c->plan);
	return EDISON_OK;
}

extern "C" int edison_fcal_reset(edison_fcal *c)
{
	if (!c) return EDISON_E_ARGUMENT;
	edison_ctx *ctx = c->ctx;
	ED_HIP(ctx, hipSetDevice(ctx->device));
	ED_HIP(ctx, hipMemsetAsync(c->d_counters, 0, c->words * sizeof(unsigned long long), ctx->stream));
	return EDISON_OK;
}

extern "C" int edison_fcal_add_dev(edison_fcal *c, const float *in, int64_t n)
{
	{ const int r = fcal_live(c, "edison_fcal_add"); if (r != EDISON_OK) return r; }
	edison_ctx *ctx = c->ctx;
	if (n < 0 || (n > 0 && !in)) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_fcal_add: negative n, or NULL inputs");
	if (n == 0) return EDISON_OK;
	ED_HIP(ctx, hipSetDevice(ctx->device));
	/* the plan's w / tab are the loaded network's device buffers: the epoch check above says they are still those */
	return ed_launch_result(ctx, ed_launch_fnet_calib(&c->plan, in, n, c->d_counters, ctx->stream), "calibration kernel");
}

extern "C" int edison_fcal_add(edison_fcal *c, const float *in, int64_t n)
{
	{ const int r = fcal_live(c, "edison_fcal_add"); if (r != EDISON_OK) return r; }
	if (n < 0 || (n > 0 && !in)) return ed_set_err(c->ctx, EDISON_E_ARGUMENT, "edison_fcal_add: negative n, or NULL inputs");
	if (n == 0) return EDISON_OK;
	ed_staging st(c->ctx);
	const float *x = st.in(in, (size_t)n * (size_t)c->plan.in_n);
	return st.finish(st.ok() ? edison_fcal_add_dev(c, x, n) : EDISON_OK);
}

extern "C" int edison_fcal_result(edison_fcal *c, uint32_t *absmax, uint64_t *hist, uint64_t *count)
{
	{ const int r = fcal_live(c, "edison_fcal_result"); if (r != EDISON_OK) return r; }
	edison_ctx *ctx = c->ctx;
	ED_HIP(ctx, hipSetDevice(ctx->device));
	std::vector<unsigned long long> h(c->words);
	ED_HIP(ctx, hipMemcpyAsync(h.data(), c->d_counters, c->words * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
	ED_HIP(ctx, hipStreamSynchronize(ctx->stream));
	const int n_stats = c->plan.n_layers + 1;
	for (int i = 0; i < n_stats; i++)
	{
		const unsigned long long *w = h.data() + (size_t)i * EDFC_WORDS;
		if (absmax) absmax[i] = (uint32_t)w[0];
		if (count) count[i] = w[1];
		if (hist)
			for (int e = 0; e < EDFC_HIST; e++) hist[(size_t)i * EDFC_HIST + e] = w[2 + e];
	}
	return EDISON_OK;
}
