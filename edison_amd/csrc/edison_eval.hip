/*
 * edison_eval.hip -- the C-ABI of scoring a labelled data set on the device (include/edison_hip.h): an evaluator
 * owns its 64-bit counters in device memory (layout: eval_kernels.hip) and every add is one launch of ed_eval_kernel on the
 * context's stream, behind whatever produced the outputs. Only edison_eval_result synchronises.
 */
#include <stdlib.h>

#include <vector>

#include "edison_ctx.h"

extern "C" int ed_launch_eval_i8(const int8_t *out, const int32_t *labels, int64_t n, int n_out, int top_k, int max_blocks, unsigned long long *counters,
                                 uint32_t *pred, float *prob, int32_t *rank, hipStream_t stream);
extern "C" int ed_launch_eval_f32(int rule, const float *out, const int32_t *labels, int64_t n, int n_out, int top_k, int max_blocks,
                                  unsigned long long *counters, uint32_t *pred, float *prob, int32_t *rank, hipStream_t stream);

struct edison_eval
{
	edison_ctx *ctx;
	edison_eval_opts o;
	int k_dev;    /* top-k entries kept on the device: min(top_k, n_classes) */
	size_t words; /* 2 + n_classes^2 + k_dev */
	unsigned long long *d_counters;
};

extern "C" void edison_eval_default_opts(edison_eval_opts *o)
{
	if (!o) return;
	o->rule = EDISON_EVAL_NNOM;
	o->n_classes = EDISON_NET_OUT;
	o->top_k = 2;
	o->max_blocks = 0;
}

extern "C" int edison_eval_create(edison_ctx *ctx, const edison_eval_opts *opts, edison_eval **out)
{
	if (!ctx || !out) return EDISON_E_ARGUMENT;
	*out = NULL;
	edison_eval_opts o;
	if (opts) o = *opts; else edison_eval_default_opts(&o);
	if (o.rule != EDISON_EVAL_NNOM && o.rule != EDISON_EVAL_KERAS && o.rule != EDISON_EVAL_ARGMAX)
		return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_eval_create: rule is not one of EDISON_EVAL_NNOM, _KERAS, _ARGMAX");
	if (o.n_classes < 1 || o.n_classes > 256) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_eval_create: n_classes must be 1 .. 256");
	if (o.top_k < 0) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_eval_create: top_k must not be negative");
	if (o.max_blocks < 0) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_eval_create: max_blocks must not be negative (0: twice the compute units)");
	if (o.max_blocks == 0) o.max_blocks = 2 * (ctx->n_cu > 0 ? ctx->n_cu : 1);
	edison_eval *e = (edison_eval *)calloc(1, sizeof(*e));
	if (!e) return ed_set_err(ctx, EDISON_E_NO_MEMORY, "edison_eval_create: out of host memory");
	e->ctx = ctx;
	e->o = o;
	e->k_dev = o.top_k < o.n_classes ? o.top_k : o.n_classes;
	e->words = 2 + (size_t)o.n_classes * (size_t)o.n_classes + (size_t)e->k_dev;
	if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc((void **)&e->d_counters, e->words * sizeof(unsigned long long)) != hipSuccess)
	{
		free(e);
		return ed_set_err(ctx, EDISON_E_NO_MEMORY, "edison_eval_create: cannot allocate the device counters");
	}
	/* zeroed before create returns: the caller may move the context to another stream before the first add */
	const int r = edison_eval_reset(e) == EDISON_OK && hipStreamSynchronize(ctx->stream) == hipSuccess
	                  ? EDISON_OK
	                  : ed_set_err(ctx, EDISON_E_RUNTIME, "edison_eval_create: cannot zero the device counters");
	if (r != EDISON_OK)
	{
		edison_eval_destroy(e);
		return r;
	}
	*out = e;
	return EDISON_OK;
}

extern "C" void edison_eval_destroy(edison_eval *e)
{
	if (!e) return;
	(void)hipSetDevice(e->ctx->device);
	(void)hipStreamSynchronize(e->ctx->stream); /* an add may still be queued */
	if (e->d_counters) (void)hipFree(e->d_counters);
	free(e);
}

extern "C" int edison_eval_reset(edison_eval *e)
{
	if (!e) return EDISON_E_ARGUMENT;
	edison_ctx *ctx = e->ctx;
	ED_HIP(ctx, hipSetDevice(ctx->device));
	ED_HIP(ctx, hipMemsetAsync(e->d_counters, 0, e->words * sizeof(unsigned long long), ctx->stream));
	return EDISON_OK;
}

static int eval_add_check(edison_eval *e, bool is_f32, const void *out, const int32_t *labels, int64_t n, const char *who)
{
	if (!e) return EDISON_E_ARGUMENT;
	edison_ctx *ctx = e->ctx;
	if ((e->o.rule != EDISON_EVAL_NNOM) != is_f32)
	{
		snprintf(ctx->err, sizeof(ctx->err), "%s: the evaluator's rule takes %s outputs", who, is_f32 ? "int8" : "float32");
		return EDISON_E_ARGUMENT;
	}
	if (n < 0 || (n > 0 && (!out || !labels)))
	{
		snprintf(ctx->err, sizeof(ctx->err), "%s: negative n, or NULL outputs / labels", who);
		return EDISON_E_ARGUMENT;
	}
	return EDISON_OK;
}

extern "C" int edison_eval_add_i8_dev(edison_eval *e, const int8_t *out, const int32_t *labels, int64_t n, uint32_t *pred, float *prob, int32_t *rank)
{
	{ const int r = eval_add_check(e, false, out, labels, n, "edison_eval_add_i8"); if (r != EDISON_OK) return r; }
	if (n == 0) return EDISON_OK;
	edison_ctx *ctx = e->ctx;
	ED_HIP(ctx, hipSetDevice(ctx->device));
	return ed_launch_result(ctx, ed_launch_eval_i8(out, labels, n, e->o.n_classes, e->o.top_k, e->o.max_blocks, e->d_counters, pred, prob, rank, ctx->stream),
	                        "evaluation kernel");
}

extern "C" int edison_eval_add_f32_dev(edison_eval *e, const float *probs, const int32_t *labels, int64_t n, uint32_t *pred, float *prob, int32_t *rank)
{
	{ const int r = eval_add_check(e, true, probs, labels, n, "edison_eval_add_f32"); if (r != EDISON_OK) return r; }
	if (n == 0) return EDISON_OK;
	edison_ctx *ctx = e->ctx;
	ED_HIP(ctx, hipSetDevice(ctx->device));
	return ed_launch_result(ctx, ed_launch_eval_f32(e->o.rule, probs, labels, n, e->o.n_classes, e->o.top_k, e->o.max_blocks, e->d_counters, pred, prob,
	                                                rank, ctx->stream),
	                        "evaluation kernel");
}

template <class T>
static int eval_add_host(edison_eval *e, int (*dev)(edison_eval *, const T *, const int32_t *, int64_t, uint32_t *, float *, int32_t *), bool is_f32,
                         const T *out, const int32_t *labels, int64_t n, uint32_t *pred, float *prob, int32_t *rank, const char *who)
{
	{ const int r = eval_add_check(e, is_f32, out, labels, n, who); if (r != EDISON_OK) return r; }
	if (n == 0) return EDISON_OK;
	ed_staging st(e->ctx);
	const T *o = st.in(out, (size_t)n * (size_t)e->o.n_classes);
	const int32_t *l = st.in(labels, (size_t)n);
	uint32_t *pd = st.out(pred, (size_t)n);
	float *pb = st.out(prob, (size_t)n);
	int32_t *rk = st.out(rank, (size_t)n);
	return st.finish(st.ok() ? dev(e, o, l, n, pd, pb, rk) : EDISON_OK);
}

extern "C" int edison_eval_add_i8(edison_eval *e, const int8_t *out, const int32_t *labels, int64_t n, uint32_t *pred, float *prob, int32_t *rank)
{
	return eval_add_host<int8_t>(e, edison_eval_add_i8_dev, false, out, labels, n, pred, prob, rank, "edison_eval_add_i8");
}

extern "C" int edison_eval_add_f32(edison_eval *e, const float *probs, const int32_t *labels, int64_t n, uint32_t *pred, float *prob, int32_t *rank)
{
	return eval_add_host<float>(e, edison_eval_add_f32_dev, true, probs, labels, n, pred, prob, rank, "edison_eval_add_f32");
}

extern "C" int edison_eval_result(edison_eval *e, edison_eval_totals *t, uint64_t *confusion, uint64_t *top_k)
{
	if (!e) return EDISON_E_ARGUMENT;
	edison_ctx *ctx = e->ctx;
	ED_HIP(ctx, hipSetDevice(ctx->device));
	std::vector<unsigned long long> h(e->words);
	ED_HIP(ctx, hipMemcpyAsync(h.data(), e->d_counters, e->words * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
	ED_HIP(ctx, hipStreamSynchronize(ctx->stream));
	const size_t nc = (size_t)e->o.n_classes, cells = nc * nc;
	if (t)
	{
		t->count = h[0];
		t->skipped = h[1];
		t->correct = 0;
		for (size_t c = 0; c < nc; c++) t->correct += h[2 + c * nc + c];
	}
	if (confusion)
		for (size_t c = 0; c < cells; c++) confusion[c] = h[2 + c];
	if (top_k)
		for (int k = 0; k < e->o.top_k; k++) top_k[k] = k < e->k_dev ? h[2 + cells + (size_t)k] : 0;
	return EDISON_OK;
}
