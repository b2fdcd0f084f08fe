/*
 * edison_ftrain.hip -- the C-ABI of training the loaded float32 network (include/edison_hip.h, edison_ftrain_*): a
 * trainer owns its copy of the network's plan at the training batch, the inverse origin tables of the backward half, one gradient slab
 * and one activation store per workgroup of the grid, the reduced gradient and Adam's moments. The weights it trains are the loaded
 * network's own device buffer. A gradient call is two launches on the context's stream (fnet_grad_kernels.hip), a step one. The trainer
 * serves the network of one load: after another edison_fnet_load* its calls fail with EDISON_E_NO_MODEL. edison_ftrain_create refuses a
 * network with a conv or pool pad; edison_ftrain_create_ex with EDISON_FTRAIN_PADDED takes it (two ints per row base, the inverse
 * origin table from the padded tables). Dropout (edison_ftrain_set_dropout) is a setting of the trainer: per
 * record a rate and a position in the plan's device copy, a seed and a call counter here; a training call with a non-zero rate runs the
 * kernel's instantiation with the mask of fnet_dropout.h and advances the counter.
 */
#include <math.h>
#include <stdlib.h>

#include <new>
#include <vector>

#include "edison_ctx.h"
#include "fnet_dropout.h"
#include "fnet_train.h"

#define EDFT_MAX_INV (1 << 24) /* ints of inverse origin tables, all records */

struct edison_ftrain
{
	edison_ctx *ctx;
	int epoch; /* the float network load (ctx->fnet_epoch) the plan belongs to */
	ed_ftrain_plan_t plan, *d_plan; /* and its copy in device memory, which the gradient kernel reads */
	int grid;
	int32_t *d_inv;
	float *d_grad, *d_m, *d_v, *d_logits;
	unsigned long long *d_ignored;
	int64_t logits_cap, n_last; /* rows d_logits holds / the last gradient call's n */
	int kind;
	double b1, b2, eps;
	int64_t steps;
	/* dropout: the rates as set (all zero: off), the positions are the plan's drop_before; the mask of a training call is a function of
	 * (drop_seed, drop_call) and the counter advances by one per such call */
	double drop_rate[ED_FNET_MAX_LAYERS];
	bool drop_on;
	uint64_t drop_seed, drop_call;
};

static int ftrain_live(edison_ftrain *t, const char *who)
{
	if (!t) return EDISON_E_ARGUMENT;
	if (t->epoch != t->ctx->fnet_epoch || !t->ctx->fnet)
	{
		snprintf(t->ctx->err, sizeof(t->ctx->err), "%s: another float network was loaded after this trainer was created; create a new one", who);
		return EDISON_E_NO_MODEL;
	}
	return EDISON_OK;
}

static float *ftrain_w(edison_ftrain *t) { return const_cast<float *>(t->plan.net.w); } /* the loaded network's device weights */

/* dY and the row bases of the largest record at the plan's batch; a padded record's row has two ints: its utterance's base and its origin */
static void ftrain_size_lds(ed_ftrain_plan_t *tp)
{
	int64_t dy = 0, rb = 0;
	for (int l = 0; l < tp->net.n_layers; l++)
	{
		const ed_fnet_layer_t &L = tp->net.L[l];
		const int64_t mp = ((int64_t)tp->net.batch * L.rows + 15) & ~(int64_t)15;
		if (mp * L.n_pad > dy) dy = mp * L.n_pad;
		if (mp * (L.pad ? 2 : 1) > rb) rb = mp * (L.pad ? 2 : 1);
	}
	tp->dy_lds = (int32_t)(dy < INT32_MAX ? dy : INT32_MAX);
	tp->rb_lds = (int32_t)(rb < INT32_MAX ? rb : INT32_MAX);
}

extern "C" int edison_ftrain_create(edison_ctx *ctx, edison_ftrain **out) { return edison_ftrain_create_ex(ctx, 0, out); }

extern "C" int edison_ftrain_create_ex(edison_ctx *ctx, uint32_t flags, edison_ftrain **out)
{
	if (!ctx || !out) return EDISON_E_ARGUMENT;
	*out = NULL;
	if (flags & ~EDISON_FTRAIN_PADDED) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_create_ex: flags has a bit other than EDISON_FTRAIN_PADDED");
	const ed_fnet_plan_t *net = ed_ctx_fnet_plan(ctx);
	if (!net) return ed_set_err(ctx, EDISON_E_NO_MODEL, "no float network loaded (edison_fnet_load)");
	for (int l = 0; l < net->n_layers; l++)
		if (net->L[l].pad && !(flags & EDISON_FTRAIN_PADDED))
		{
			snprintf(ctx->err, sizeof(ctx->err), "edison_ftrain_create: record %d has a conv or pool pad; training runs networks without pads", l);
			return EDISON_E_NO_IMPL;
		}
	edison_ftrain *t = new (std::nothrow) edison_ftrain();
	if (!t) return ed_set_err(ctx, EDISON_E_NO_MEMORY, "edison_ftrain_create: out of host memory");
	t->ctx = ctx;
	t->epoch = ctx->fnet_epoch;
	t->kind = EDISON_FTRAIN_ADAM;
	t->b1 = 0.9; t->b2 = 0.999; t->eps = 1e-7;
	ed_ftrain_plan_t &tp = t->plan;
	tp.net = *net;
	const ed_fnet_layer_t &last = net->L[net->n_layers - 1];
	tp.w_floats = last.w_at + (int64_t)last.k_pad * last.n_pad + last.n_pad;
	/* utterances per workgroup: the network's, fewer while the backward half's dY does not fit */
	for (ftrain_size_lds(&tp); tp.net.batch > 1 && ed_ftrain_lds_bytes(&tp) > ED_FNET_LDS_BYTES; ftrain_size_lds(&tp)) tp.net.batch--;
	if (ed_ftrain_lds_bytes(&tp) > ED_FNET_LDS_BYTES)
	{
		delete t;
		return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_ftrain_create: the training workgroup does not fit the LDS (one utterance's dY of the largest record)");
	}
	if (hipSetDevice(ctx->device) != hipSuccess) { delete t; return ed_set_err(ctx, EDISON_E_RUNTIME, "edison_ftrain_create: hipSetDevice failed"); }

	/* the inverse origin tables, from the plan's own koff / rowin: row r reads position (rowin[r] + koff[k]) / in_c through tap k / in_c;
	 * a padded record's row that is not absent reads (y0 + ky, x0 + kx) through tap (ky, kx) where that lies inside the image */
	const size_t tabn = (size_t)last.rowin_at + (size_t)last.rows;
	std::vector<int32_t> tab(tabn), inv;
	if (hipMemcpy(tab.data(), net->tab, tabn * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
	{
		delete t;
		return ed_set_err(ctx, EDISON_E_RUNTIME, "edison_ftrain_create: cannot read the network's tables");
	}
	for (int l = 0; l < ED_FNET_MAX_LAYERS; l++) tp.drop_s[l] = 1.0f; /* dropout off: T 0, s 1 */
	for (int l = 0; l < net->n_layers; l++)
	{
		const ed_fnet_layer_t &L = net->L[l];
		ed_ftrain_layer_t &G = tp.G[l];
		const int32_t *koff = tab.data() + L.koff_at, *rowin = tab.data() + L.rowin_at;
		G.K = 0;
		for (int k = 0; k < L.k_pad; k++) G.K += koff[k] >= 0;
		G.T = G.K / L.in_c;
		G.np = L.in_h * L.in_w;
		G.inv_at = (int32_t)inv.size();
		if (l == 0) continue; /* the network input's gradient is not computed */
		if ((int64_t)G.np * G.T + (int64_t)inv.size() > EDFT_MAX_INV)
		{
			delete t;
			snprintf(ctx->err, sizeof(ctx->err), "edison_ftrain_create: record %d's inverse origin table is too large", l);
			return EDISON_E_NO_IMPL;
		}
		inv.resize(inv.size() + (size_t)G.np * G.T, -1);
		int32_t *iv = inv.data() + G.inv_at;
		for (int r = 0; r < L.rows; r++)
		{
			if (!L.pad)
			{
				for (int tap = 0; tap < G.T; tap++) iv[(size_t)((rowin[r] + koff[tap * L.in_c]) / L.in_c) * G.T + tap] = r;
				continue;
			}
			if (rowin[r] < 0) continue; /* absent */
			const int y0 = (rowin[r] >> 16) - ED_FNET_ORIGIN_BIAS, x0 = (rowin[r] & 0xffff) - ED_FNET_ORIGIN_BIAS;
			for (int tap = 0; tap < G.T; tap++)
			{
				const int32_t kyx = koff[L.k_pad + tap * L.in_c];
				const int y = y0 + (kyx >> 16), x = x0 + (kyx & 0xffff);
				if (y >= 0 && y < L.in_h && x >= 0 && x < L.in_w) iv[(size_t)(y * L.in_w + x) * G.T + tap] = r;
			}
		}
	}

	const int64_t store = (int64_t)tp.net.batch * tp.net.acts_n;
	t->grid = ctx->n_cu > 0 ? ctx->n_cu : 1;
	const size_t wb = sizeof(float) * (size_t)tp.w_floats;
	hipError_t e = hipMalloc((void **)&t->d_inv, sizeof(int32_t) * (inv.size() ? inv.size() : 1));
	if (e == hipSuccess && inv.size()) e = hipMemcpy(t->d_inv, inv.data(), sizeof(int32_t) * inv.size(), hipMemcpyHostToDevice);
	if (e == hipSuccess) e = hipMalloc((void **)&tp.slabs, wb * (size_t)t->grid);
	if (e == hipSuccess) e = hipMemset(tp.slabs, 0, wb * (size_t)t->grid); /* the padding entries: never written afterwards */
	if (e == hipSuccess) e = hipMalloc((void **)&tp.acts, sizeof(float) * (size_t)store * (size_t)t->grid);
	if (e == hipSuccess) e = hipMalloc((void **)&tp.dacts, sizeof(float) * (size_t)store * (size_t)t->grid);
	if (e == hipSuccess) e = hipMalloc((void **)&tp.mask, (size_t)store * (size_t)t->grid);
	if (e == hipSuccess) e = hipMalloc((void **)&tp.keys, sizeof(uint32_t) * 2 * (size_t)tp.net.batch * (size_t)tp.net.n_layers * (size_t)t->grid);
	tp.inv = t->d_inv;
	if (e == hipSuccess) e = hipMalloc((void **)&t->d_plan, sizeof(tp));
	if (e == hipSuccess) e = hipMemcpy(t->d_plan, &tp, sizeof(tp), hipMemcpyHostToDevice);
	if (e == hipSuccess) e = hipMalloc((void **)&t->d_grad, wb);
	if (e == hipSuccess) e = hipMalloc((void **)&t->d_m, wb);
	if (e == hipSuccess) e = hipMalloc((void **)&t->d_v, wb);
	if (e == hipSuccess) e = hipMalloc((void **)&t->d_ignored, sizeof(unsigned long long));
	if (e == hipSuccess) e = hipMemset(t->d_grad, 0, wb);
	if (e == hipSuccess) e = hipMemset(t->d_m, 0, wb);
	if (e == hipSuccess) e = hipMemset(t->d_v, 0, wb);
	if (e == hipSuccess) e = hipMemset(t->d_ignored, 0, sizeof(unsigned long long));
	if (e == hipSuccess) e = hipDeviceSynchronize(); /* zeroed before create returns, whatever stream the context moves to */
	if (e != hipSuccess)
	{
		edison_ftrain_destroy(t);
		return ed_set_err(ctx, e == hipErrorOutOfMemory ? EDISON_E_NO_MEMORY : EDISON_E_RUNTIME, "edison_ftrain_create: cannot allocate the trainer's device buffers");
	}
	*out = t;
	return EDISON_OK;
}

extern "C" void edison_ftrain_destroy(edison_ftrain *t)
{
	if (!t) return;
	(void)hipSetDevice(t->ctx->device);
	(void)hipStreamSynchronize(t->ctx->stream); /* a gradient call or a step may still be queued */
	void *bufs[] = {t->d_plan, t->d_inv, t->plan.slabs, t->plan.acts, t->plan.dacts, t->plan.mask, t->plan.keys, t->d_grad, t->d_m, t->d_v, t->d_logits, t->d_ignored};
	for (void *b : bufs)
		if (b) (void)hipFree(b);
	delete t;
}

extern "C" int edison_ftrain_info(edison_ftrain *t, edison_ftrain_info_t *out)
{
	if (!t || !out) return EDISON_E_ARGUMENT;
	{ const int r = ftrain_live(t, "edison_ftrain_info"); if (r != EDISON_OK) return r; }
	edison_ctx *ctx = t->ctx;
	unsigned long long ignored = 0;
	ED_HIP(ctx, hipSetDevice(ctx->device));
	ED_HIP(ctx, hipMemcpyAsync(&ignored, t->d_ignored, sizeof(ignored), hipMemcpyDeviceToHost, ctx->stream));
	ED_HIP(ctx, hipStreamSynchronize(ctx->stream));
	out->n_layers = t->plan.net.n_layers;
	out->in_n = t->plan.net.in_n;
	out->n_out = t->plan.net.n_out;
	out->batch = t->plan.net.batch;
	out->lds_bytes = (int32_t)ed_ftrain_lds_bytes(&t->plan);
	out->grid = t->grid;
	out->w_floats = t->plan.w_floats;
	out->steps = t->steps;
	out->ignored = (int64_t)ignored;
	return EDISON_OK;
}

extern "C" int edison_ftrain_layout(edison_ftrain *t, int record, int64_t *w_at, int32_t *K, int32_t *k_pad, int32_t *out_c, int32_t *n_pad)
{
	{ const int r = ftrain_live(t, "edison_ftrain_layout"); if (r != EDISON_OK) return r; }
	if (record < 0 || record >= t->plan.net.n_layers) return ed_set_err(t->ctx, EDISON_E_ARGUMENT, "edison_ftrain_layout: no such record");
	const ed_fnet_layer_t &L = t->plan.net.L[record];
	if (w_at) *w_at = L.w_at;
	if (K) *K = t->plan.G[record].K;
	if (k_pad) *k_pad = L.k_pad;
	if (out_c) *out_c = L.out_c;
	if (n_pad) *n_pad = L.n_pad;
	return EDISON_OK;
}

extern "C" int edison_ftrain_set_dropout(edison_ftrain *t, const double *rate, const uint8_t *before_pool, int n_records, uint64_t seed)
{
	{ const int r = ftrain_live(t, "edison_ftrain_set_dropout"); if (r != EDISON_OK) return r; }
	edison_ctx *ctx = t->ctx;
	const int nl = t->plan.net.n_layers;
	if (!rate || n_records != nl) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_set_dropout: NULL rates, or n_records is not the network's conv / dense records");
	bool on = false;
	for (int l = 0; l < nl; l++)
	{
		if (!(rate[l] >= 0.0 && rate[l] < 1.0)) /* NaN fails both */
		{
			snprintf(ctx->err, sizeof(ctx->err), "edison_ftrain_set_dropout: record %d's rate is not in [0, 1)", l);
			return EDISON_E_ARGUMENT;
		}
		on = on || rate[l] > 0.0;
	}
	if (rate[nl - 1] != 0.0) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_set_dropout: the last record's output is the logits; its rate must be 0");
	ED_HIP(ctx, hipSetDevice(ctx->device));
	ED_HIP(ctx, hipStreamSynchronize(ctx->stream)); /* a queued gradient call reads the plan's device copy */
	ed_ftrain_plan_t &tp = t->plan;
	for (int l = 0; l < nl; l++)
	{
		t->drop_rate[l] = rate[l];
		tp.drop_T[l] = rate[l] > 0.0 ? edd_threshold(rate[l]) : 0;
		tp.drop_s[l] = rate[l] > 0.0 ? edd_scale(rate[l]) : 1.0f;
		tp.drop_before[l] = before_pool && before_pool[l] ? 1 : 0;
	}
	t->drop_on = on;
	t->drop_seed = seed;
	t->drop_call = 0;
	ED_HIP(ctx, hipMemcpy(t->d_plan, &tp, sizeof(tp), hipMemcpyHostToDevice));
	return EDISON_OK;
}

extern "C" int edison_ftrain_set_dropout_call(edison_ftrain *t, uint64_t call)
{
	{ const int r = ftrain_live(t, "edison_ftrain_set_dropout_call"); if (r != EDISON_OK) return r; }
	if (call >= (1ull << 60)) return ed_set_err(t->ctx, EDISON_E_ARGUMENT, "edison_ftrain_set_dropout_call: the counter is below 2^60");
	t->drop_call = call;
	return EDISON_OK;
}

extern "C" int edison_ftrain_dropout_get(edison_ftrain *t, double *rate, uint8_t *before_pool, uint64_t *seed, uint64_t *call)
{
	{ const int r = ftrain_live(t, "edison_ftrain_dropout_get"); if (r != EDISON_OK) return r; }
	for (int l = 0; l < t->plan.net.n_layers; l++)
	{
		if (rate) rate[l] = t->drop_rate[l];
		if (before_pool) before_pool[l] = t->plan.drop_before[l];
	}
	if (seed) *seed = t->drop_seed;
	if (call) *call = t->drop_call;
	return EDISON_OK;
}

extern "C" int edison_ftrain_grad_dev(edison_ftrain *t, const float *in, const int32_t *labels, int64_t n, float *loss, int32_t *argmax)
{
	return edison_ftrain_grad_dev_ex(t, in, labels, n, loss, argmax, 0);
}

extern "C" int edison_ftrain_grad_dev_ex(edison_ftrain *t, const float *in, const int32_t *labels, int64_t n, float *loss, int32_t *argmax, uint32_t flags)
{
	{ const int r = ftrain_live(t, "edison_ftrain_grad"); if (r != EDISON_OK) return r; }
	edison_ctx *ctx = t->ctx;
	if (flags & ~EDISON_FTRAIN_EVAL) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_grad_ex: flags has a bit other than EDISON_FTRAIN_EVAL");
	const bool drop = t->drop_on && !(flags & EDISON_FTRAIN_EVAL);
	if (drop && n > 0xffffffffll) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_grad: a training call with dropout takes fewer than 2^32 rows");
	if (n < 0 || (n > 0 && (!in || !labels))) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_grad: negative n, or NULL inputs or labels");
	ED_HIP(ctx, hipSetDevice(ctx->device));
	t->n_last = n;
	if (n == 0)
	{
		ED_HIP(ctx, hipMemsetAsync(t->d_grad, 0, sizeof(float) * (size_t)t->plan.w_floats, ctx->stream));
		return EDISON_OK;
	}
	if (n > t->logits_cap)
	{
		/* a queued call may still write the old buffer */
		ED_HIP(ctx, hipStreamSynchronize(ctx->stream));
		if (t->d_logits) (void)hipFree(t->d_logits);
		t->d_logits = NULL;
		t->logits_cap = 0;
		if (hipMalloc((void **)&t->d_logits, sizeof(float) * (size_t)n * (size_t)t->plan.net.n_out) != hipSuccess)
			return ed_set_err(ctx, EDISON_E_NO_MEMORY, "edison_ftrain_grad: cannot allocate the logits");
		t->logits_cap = n;
	}
	/* the plan's w / tab are the loaded network's device buffers: the epoch check above says they are still those */
	const int r = ed_launch_result(ctx, ed_launch_ftrain_grad(&t->plan, t->d_plan, in, labels, n, loss, argmax, t->d_logits, t->d_grad, t->d_ignored, t->grid,
	                                                          drop, t->drop_seed, t->drop_call, ctx->stream),
	                               "gradient kernel");
	if (r == EDISON_OK && drop) t->drop_call++; /* the next training call draws another mask */
	return r;
}

extern "C" int edison_ftrain_grad(edison_ftrain *t, const float *in, const int32_t *labels, int64_t n, float *loss, int32_t *argmax)
{
	return edison_ftrain_grad_ex(t, in, labels, n, loss, argmax, 0);
}

extern "C" int edison_ftrain_grad_ex(edison_ftrain *t, const float *in, const int32_t *labels, int64_t n, float *loss, int32_t *argmax, uint32_t flags)
{
	{ const int r = ftrain_live(t, "edison_ftrain_grad"); if (r != EDISON_OK) return r; }
	edison_ctx *ctx = t->ctx;
	if (flags & ~EDISON_FTRAIN_EVAL) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_grad_ex: flags has a bit other than EDISON_FTRAIN_EVAL");
	if (n < 0 || (n > 0 && (!in || !labels))) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_grad: negative n, or NULL inputs or labels");
	for (int64_t i = 0; i < n; i++)
		if (labels[i] < 0 || labels[i] >= t->plan.net.n_out)
		{
			snprintf(ctx->err, sizeof(ctx->err), "edison_ftrain_grad: label %d of row %lld is outside 0 .. %d", labels[i], (long long)i, t->plan.net.n_out - 1);
			return EDISON_E_ARGUMENT;
		}
	if (n == 0) return edison_ftrain_grad_dev_ex(t, NULL, NULL, 0, NULL, NULL, flags);
	ed_staging st(ctx);
	const float *x = st.in(in, (size_t)n * (size_t)t->plan.net.in_n);
	const int32_t *y = st.in(labels, (size_t)n);
	float *l = st.out(loss, (size_t)n);
	int32_t *a = st.out(argmax, (size_t)n);
	return st.finish(st.ok() ? edison_ftrain_grad_dev_ex(t, x, y, n, l, a, flags) : EDISON_OK);
}

/* synchronising copies between the host and one of the trainer's device arrays */
static int ftrain_copy(edison_ftrain *t, const char *who, void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
	{ const int r = ftrain_live(t, who); if (r != EDISON_OK) return r; }
	edison_ctx *ctx = t->ctx;
	if (!dst || !src) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain: NULL array");
	ED_HIP(ctx, hipSetDevice(ctx->device));
	if (bytes) ED_HIP(ctx, hipMemcpyAsync(dst, src, bytes, kind, ctx->stream));
	ED_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return EDISON_OK;
}

extern "C" int edison_ftrain_grad_get(edison_ftrain *t, float *packed)
{
	if (!t) return EDISON_E_ARGUMENT;
	return ftrain_copy(t, "edison_ftrain_grad_get", packed, t->d_grad, sizeof(float) * (size_t)t->plan.w_floats, hipMemcpyDeviceToHost);
}

extern "C" int edison_ftrain_logits_get(edison_ftrain *t, float *logits)
{
	if (!t) return EDISON_E_ARGUMENT;
	if (t->n_last == 0) return ftrain_live(t, "edison_ftrain_logits_get");
	return ftrain_copy(t, "edison_ftrain_logits_get", logits, t->d_logits, sizeof(float) * (size_t)t->n_last * (size_t)t->plan.net.n_out, hipMemcpyDeviceToHost);
}

extern "C" int edison_ftrain_weights_get(edison_ftrain *t, float *packed)
{
	if (!t) return EDISON_E_ARGUMENT;
	return ftrain_copy(t, "edison_ftrain_weights_get", packed, t->plan.net.w, sizeof(float) * (size_t)t->plan.w_floats, hipMemcpyDeviceToHost);
}

extern "C" int edison_ftrain_weights_set(edison_ftrain *t, const float *packed)
{
	if (!t) return EDISON_E_ARGUMENT;
	return ftrain_copy(t, "edison_ftrain_weights_set", ftrain_w(t), packed, sizeof(float) * (size_t)t->plan.w_floats, hipMemcpyHostToDevice);
}

extern "C" int edison_ftrain_set_opt(edison_ftrain *t, int kind, double b1, double b2, double eps)
{
	{ const int r = ftrain_live(t, "edison_ftrain_set_opt"); if (r != EDISON_OK) return r; }
	if (kind != EDISON_FTRAIN_ADAM && kind != EDISON_FTRAIN_SGD) return ed_set_err(t->ctx, EDISON_E_ARGUMENT, "edison_ftrain_set_opt: kind is not Adam or SGD");
	if (kind == EDISON_FTRAIN_ADAM && !(b1 >= 0.0 && b1 < 1.0 && b2 >= 0.0 && b2 < 1.0 && eps > 0.0))
		return ed_set_err(t->ctx, EDISON_E_ARGUMENT, "edison_ftrain_set_opt: Adam takes b1 and b2 in [0, 1) and eps > 0");
	t->kind = kind;
	if (kind == EDISON_FTRAIN_ADAM) { t->b1 = b1; t->b2 = b2; t->eps = eps; }
	return EDISON_OK;
}

extern "C" int edison_ftrain_step(edison_ftrain *t, double lr)
{
	{ const int r = ftrain_live(t, "edison_ftrain_step"); if (r != EDISON_OK) return r; }
	edison_ctx *ctx = t->ctx;
	if (!(lr >= 0.0) || !isfinite(lr)) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_step: the learning rate is negative or not finite");
	ED_HIP(ctx, hipSetDevice(ctx->device));
	const double tt = (double)(t->steps + 1);
	const double factor = t->kind == EDISON_FTRAIN_SGD ? lr : lr * sqrt(1.0 - pow(t->b2, tt)) / (1.0 - pow(t->b1, tt));
	const int e = ed_launch_ftrain_step(t->kind, ftrain_w(t), t->d_grad, t->d_m, t->d_v, t->plan.w_floats, (float)factor, (float)t->b1, (float)(1.0 - t->b1),
	                                    (float)t->b2, (float)(1.0 - t->b2), (float)t->eps, ctx->n_cu, ctx->stream);
	if (e == 0) t->steps++;
	return ed_launch_result(ctx, e, "optimiser step kernel");
}

extern "C" int edison_ftrain_reset(edison_ftrain *t)
{
	{ const int r = ftrain_live(t, "edison_ftrain_reset"); if (r != EDISON_OK) return r; }
	edison_ctx *ctx = t->ctx;
	ED_HIP(ctx, hipSetDevice(ctx->device));
	ED_HIP(ctx, hipMemsetAsync(t->d_m, 0, sizeof(float) * (size_t)t->plan.w_floats, ctx->stream));
	ED_HIP(ctx, hipMemsetAsync(t->d_v, 0, sizeof(float) * (size_t)t->plan.w_floats, ctx->stream));
	ED_HIP(ctx, hipMemsetAsync(t->d_ignored, 0, sizeof(unsigned long long), ctx->stream));
	t->steps = 0;
	t->drop_call = 0;
	return EDISON_OK;
}
