/*
 * edison_ftrain.hip -- the C-ABI of training the loaded float32 network (include/edison_hip.h, edison_ftrain_*): a
 * trainer owns its copy of the network's plan at the training batch, the inverse origin tables of the backward half, one gradient slab
 * and one activation store per workgroup of the grid, the reduced gradient and Adam's moments. The weights it trains are the loaded
 * network's own device buffer. A gradient call is two launches on the context's stream (fnet_grad_kernels.hip), a step one. The trainer
 * serves the network of one load: after another edison_fnet_load* its calls fail with EDISON_E_NO_MODEL. edison_ftrain_create refuses a
 * network with a conv or pool pad; edison_ftrain_create_ex with EDISON_FTRAIN_PADDED takes it (two ints per row base, the inverse
 * origin table from the padded tables). Dropout (edison_ftrain_set_dropout) is a setting of the trainer: per
 * record a rate and a position in the plan's device copy, a seed and a call counter here; a training call with a non-zero rate runs the
 * kernel's instantiation with the mask of fnet_dropout.h and advances the counter. BatchNorm (edison_ftrain_set_batchnorm; DESIGN.md
 * section 19c) turns the trainer into one that owns master weights, gamma, beta and moving statistics: a training call is the chain of
 * launches of fnet_bn_kernels.hip over stores sized for max_rows rows, and after every change a fold kernel rewrites the loaded
 * network's device buffer with the inference-mode network, which is what every other entry point, an EVAL call included, runs.
 * Data sets on the device (edison_ftrain_data_*) belong to the context; edison_ftrain_epoch gathers an epoch's rows
 * out of one into the trainer's epoch store and queues the gradient call and the step of every batch behind it, edison_ftrain_data_eval
 * runs one through EVAL calls; both end in one reduction (fnet_data_kernels.hip), one copy back and one synchronisation.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <vector>

#include "edison_ctx.h"
#include "fnet_bn.h"
#include "fnet_data.h"
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
	/* BatchNorm: off until edison_ftrain_set_batchnorm. d_master [w_floats] is what step and weights_get / _set see; d_bn holds every
	 * per-channel array of the plan, d_bn_m / d_bn_v Adam's moments of gamma and beta. grad_stale: the last gradient call was an EVAL
	 * call on the folded weights, whose gradient is not one of the master weights. */
	bool bn_on, grad_stale;
	uint8_t has_bn[ED_FNET_MAX_LAYERS];
	double bn_momentum, bn_eps;
	uint32_t bn_flags;
	ed_fbn_plan_t bplan, *d_bplan;
	float *d_master, *d_bn, *d_bn_m, *d_bn_v;
	int32_t *d_rtab, *d_binv;
	/* Adadelta's constants (EDISON_FTRAIN_ADADELTA): d_m is its average of g g, d_v its average of u u */
	double rho, ad_eps;
	/* the epoch store (edison_ftrain_epoch / edison_ftrain_data_eval): per row of the last such call its loss and argmax, and for an epoch
	 * the order, the gathered labels (all [e_cap]) and the gathered rows [ex_cap][in_n]; e_n rows of the last call */
	float *d_ex, *d_eloss;
	int32_t *d_ey, *d_eam, *d_eorder;
	ed_fdata_sums_t *d_esums;
	int64_t e_cap, ex_cap, e_n;
};

struct edison_ftrain_data
{
	edison_ctx *ctx;
	int32_t in_n;
	int64_t n, cap;
	float *d_x;    /* [cap][in_n] */
	int32_t *d_y;  /* [cap]       */
	std::vector<int32_t> y; /* the labels on the host: an epoch call checks them against the network's n_out before any launch */
};

#define EDBN_DEFAULT_ROWS 1024

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
	if (ed_ctx_fnet_layered(ctx)) return ed_fnet_refuse_layered(ctx, "edison_ftrain_create");
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
	t->rho = 0.95; t->ad_eps = 1e-7;
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
	void *bufs[] = {t->d_plan, t->d_inv, t->plan.slabs, t->plan.acts, t->plan.dacts, t->plan.mask, t->plan.keys, t->d_grad, t->d_m, t->d_v, t->d_logits, t->d_ignored,
	                t->d_bplan, t->d_master, t->d_bn, t->d_bn_m, t->d_bn_v, t->d_rtab, t->d_binv, t->bplan.zs, t->bplan.outs, t->bplan.douts, t->bplan.mask,
	                t->bplan.part, t->bplan.keys, t->d_ex, t->d_eloss, t->d_ey, t->d_eam, t->d_eorder, t->d_esums};
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
	const bool bn = t->bn_on && !(flags & EDISON_FTRAIN_EVAL);
	if (bn && n > t->bplan.max_rows)
	{
		snprintf(ctx->err, sizeof(ctx->err), "edison_ftrain_grad: a training call with BatchNorm takes at most max_rows = %lld rows (edison_ftrain_set_batchnorm)",
		         (long long)t->bplan.max_rows);
		return EDISON_E_ARGUMENT;
	}
	if (bn && (t->bn_flags & EDISON_FTRAIN_BN_UNBIASED) && n > 0)
		for (int l = 0; l < t->bplan.n_layers; l++)
			if (t->has_bn[l] && n * t->bplan.R[l].R < 2)
			{
				snprintf(ctx->err, sizeof(ctx->err), "edison_ftrain_grad: record %d's statistics have N < 2 values; the unbiased variance needs two", l);
				return EDISON_E_ARGUMENT;
			}
	if (drop && n > 0xffffffffll) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_grad: a training call with dropout takes fewer than 2^32 rows");
	if (n < 0 || (n > 0 && (!in || !labels))) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_grad: negative n, or NULL inputs or labels");
	ED_HIP(ctx, hipSetDevice(ctx->device));
	t->n_last = n;
	t->grad_stale = t->bn_on && !bn; /* an EVAL call runs the folded weights: what it leaves is no gradient of the master weights */
	if (n == 0)
	{
		ED_HIP(ctx, hipMemsetAsync(t->d_grad, 0, sizeof(float) * (size_t)t->plan.w_floats, ctx->stream));
		if (bn) ED_HIP(ctx, hipMemsetAsync(t->bplan.bng, 0, sizeof(float) * 2 * (size_t)t->bplan.bn_n, ctx->stream));
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
	if (bn)
	{
		ed_fbn_drop_t dr[ED_FNET_MAX_LAYERS];
		for (int l = 0; l < t->bplan.n_layers; l++) dr[l] = (ed_fbn_drop_t){drop ? t->plan.drop_T[l] : 0, t->plan.drop_s[l], t->plan.drop_before[l]};
		const int r = ed_launch_result(ctx, ed_launch_fbn_train(&t->bplan, t->d_bplan, in, labels, n, loss, argmax, t->d_logits, t->d_grad, t->d_ignored, dr,
		                                                         t->drop_seed, t->drop_call, t->bn_momentum, t->bn_eps, t->bn_flags, ctx->stream),
		                               "BatchNorm training kernels");
		if (r == EDISON_OK && drop) t->drop_call++;
		return r;
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

/* BatchNorm: rewrite the loaded network's device buffer with the inference-mode network of the master weights and the moving statistics */
static int ftrain_fold(edison_ftrain *t)
{
	edison_ctx *ctx = t->ctx;
	return ed_launch_result(ctx, ed_launch_fbn_fold(&t->bplan, t->d_bplan, ftrain_w(t), t->bn_eps, ctx->stream), "BatchNorm fold kernel");
}

static int ftrain_stale(edison_ftrain *t, const char *who)
{
	snprintf(t->ctx->err, sizeof(t->ctx->err),
	         "%s: the last gradient call was an EDISON_FTRAIN_EVAL call on the folded BatchNorm network; its gradient is not one of the trained weights (make a training call first)", who);
	return EDISON_E_ARGUMENT;
}

extern "C" int edison_ftrain_grad_get(edison_ftrain *t, float *packed)
{
	if (!t) return EDISON_E_ARGUMENT;
	if (t->grad_stale) return ftrain_stale(t, "edison_ftrain_grad_get");
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
	return ftrain_copy(t, "edison_ftrain_weights_get", packed, t->bn_on ? t->d_master : t->plan.net.w, sizeof(float) * (size_t)t->plan.w_floats, hipMemcpyDeviceToHost);
}

extern "C" int edison_ftrain_weights_set(edison_ftrain *t, const float *packed)
{
	if (!t) return EDISON_E_ARGUMENT;
	const int r = ftrain_copy(t, "edison_ftrain_weights_set", t->bn_on ? t->d_master : ftrain_w(t), packed, sizeof(float) * (size_t)t->plan.w_floats, hipMemcpyHostToDevice);
	return r == EDISON_OK && t->bn_on ? ftrain_fold(t) : r;
}

extern "C" int edison_ftrain_set_opt(edison_ftrain *t, int kind, double b1, double b2, double eps)
{
	{ const int r = ftrain_live(t, "edison_ftrain_set_opt"); if (r != EDISON_OK) return r; }
	if (kind != EDISON_FTRAIN_ADAM && kind != EDISON_FTRAIN_SGD && kind != EDISON_FTRAIN_ADADELTA)
		return ed_set_err(t->ctx, EDISON_E_ARGUMENT, "edison_ftrain_set_opt: kind is not Adam, SGD or Adadelta");
	if (kind == EDISON_FTRAIN_ADADELTA && !(b1 >= 0.0 && b1 < 1.0 && eps > 0.0 && isfinite(eps)))
		return ed_set_err(t->ctx, EDISON_E_ARGUMENT, "edison_ftrain_set_opt: Adadelta takes rho (b1) in [0, 1) and a finite eps > 0");
	if (kind == EDISON_FTRAIN_ADAM && !(b1 >= 0.0 && b1 < 1.0 && b2 >= 0.0 && b2 < 1.0 && eps > 0.0))
		return ed_set_err(t->ctx, EDISON_E_ARGUMENT, "edison_ftrain_set_opt: Adam takes b1 and b2 in [0, 1) and eps > 0");
	t->kind = kind;
	if (kind == EDISON_FTRAIN_ADAM) { t->b1 = b1; t->b2 = b2; t->eps = eps; }
	if (kind == EDISON_FTRAIN_ADADELTA) { t->rho = b1; t->ad_eps = eps; }
	return EDISON_OK;
}

extern "C" int edison_ftrain_step(edison_ftrain *t, double lr)
{
	{ const int r = ftrain_live(t, "edison_ftrain_step"); if (r != EDISON_OK) return r; }
	edison_ctx *ctx = t->ctx;
	if (!(lr >= 0.0) || !isfinite(lr)) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_step: the learning rate is negative or not finite");
	if (t->grad_stale) return ftrain_stale(t, "edison_ftrain_step");
	ED_HIP(ctx, hipSetDevice(ctx->device));
	int e;
	if (t->kind == EDISON_FTRAIN_ADADELTA)
	{
		/* a kernel of its own (fnet_data_kernels.hip) on the same two moment arrays; gamma and beta as the other kinds step them */
		const float rho = (float)t->rho, omr = (float)(1.0 - t->rho), eps = (float)t->ad_eps;
		e = ed_launch_ftrain_adadelta(t->bn_on ? t->d_master : ftrain_w(t), t->d_grad, t->d_m, t->d_v, t->plan.w_floats, (float)lr, rho, omr, eps, ctx->n_cu, ctx->stream);
		if (e == 0 && t->bn_on)
			e = ed_launch_ftrain_adadelta(t->bplan.bnp, t->bplan.bng, t->d_bn_m, t->d_bn_v, 2 * (int64_t)t->bplan.bn_n, (float)lr, rho, omr, eps, ctx->n_cu, ctx->stream);
	}
	else
	{
		const double tt = (double)(t->steps + 1);
		const double factor = t->kind == EDISON_FTRAIN_SGD ? lr : lr * sqrt(1.0 - pow(t->b2, tt)) / (1.0 - pow(t->b1, tt));
		e = ed_launch_ftrain_step(t->kind, t->bn_on ? t->d_master : ftrain_w(t), t->d_grad, t->d_m, t->d_v, t->plan.w_floats, (float)factor, (float)t->b1,
		                              (float)(1.0 - t->b1), (float)t->b2, (float)(1.0 - t->b2), (float)t->eps, ctx->n_cu, ctx->stream);
		if (e == 0 && t->bn_on) /* gamma and beta: the same optimiser, moments of their own; channels of records without BatchNorm have gradient 0 */
			e = ed_launch_ftrain_step(t->kind, t->bplan.bnp, t->bplan.bng, t->d_bn_m, t->d_bn_v, 2 * (int64_t)t->bplan.bn_n, (float)factor, (float)t->b1,
			                          (float)(1.0 - t->b1), (float)t->b2, (float)(1.0 - t->b2), (float)t->eps, ctx->n_cu, ctx->stream);
	}
	if (e == 0) t->steps++;
	{ const int r = ed_launch_result(ctx, e, "optimiser step kernel"); if (r != EDISON_OK || !t->bn_on) return r; }
	return ftrain_fold(t);
}

extern "C" int edison_ftrain_reset(edison_ftrain *t)
{
	{ const int r = ftrain_live(t, "edison_ftrain_reset"); if (r != EDISON_OK) return r; }
	edison_ctx *ctx = t->ctx;
	ED_HIP(ctx, hipSetDevice(ctx->device));
	ED_HIP(ctx, hipMemsetAsync(t->d_m, 0, sizeof(float) * (size_t)t->plan.w_floats, ctx->stream));
	ED_HIP(ctx, hipMemsetAsync(t->d_v, 0, sizeof(float) * (size_t)t->plan.w_floats, ctx->stream));
	ED_HIP(ctx, hipMemsetAsync(t->d_ignored, 0, sizeof(unsigned long long), ctx->stream));
	if (t->bn_on)
	{
		ED_HIP(ctx, hipMemsetAsync(t->d_bn_m, 0, sizeof(float) * 2 * (size_t)t->bplan.bn_n, ctx->stream));
		ED_HIP(ctx, hipMemsetAsync(t->d_bn_v, 0, sizeof(float) * 2 * (size_t)t->bplan.bn_n, ctx->stream));
	}
	t->steps = 0;
	t->drop_call = 0;
	return EDISON_OK;
}

/* ---- BatchNorm ---- */
extern "C" int edison_ftrain_set_batchnorm(edison_ftrain *t, const uint8_t *has_bn, int n_records, double momentum, double eps, int64_t max_rows, uint32_t flags)
{
	{ const int r = ftrain_live(t, "edison_ftrain_set_batchnorm"); if (r != EDISON_OK) return r; }
	edison_ctx *ctx = t->ctx;
	const ed_fnet_plan_t &net = t->plan.net;
	const int nl = net.n_layers;
	if (t->bn_on) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_set_batchnorm: BatchNorm is already on for this trainer; create a new trainer");
	if (!has_bn || n_records != nl) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_set_batchnorm: NULL has_bn, or n_records is not the network's conv / dense records");
	if (flags & ~EDISON_FTRAIN_BN_UNBIASED) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_set_batchnorm: flags has a bit other than EDISON_FTRAIN_BN_UNBIASED");
	if (!(momentum >= 0.0 && momentum < 1.0)) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_set_batchnorm: momentum is not in [0, 1)");
	if (!(eps > 0.0) || !isfinite(eps)) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_set_batchnorm: eps is not a finite value above 0");
	if (has_bn[nl - 1]) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_set_batchnorm: the last record's output is the logits; it takes no BatchNorm");
	for (int l = 0; l < nl; l++)
		if (net.L[l].pad)
		{
			snprintf(ctx->err, sizeof(ctx->err), "edison_ftrain_set_batchnorm: record %d has a conv or pool pad; BatchNorm trains networks without pads", l);
			return EDISON_E_NO_IMPL;
		}
	if (max_rows <= 0) max_rows = EDBN_DEFAULT_ROWS;
	if (max_rows > (1 << 22)) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_set_batchnorm: max_rows is above 2^22");
	const ed_fnet_geom_t *geom = ed_ctx_fnet_geom(ctx);
	if (!geom) return ed_set_err(ctx, EDISON_E_NO_MODEL, "no float network loaded (edison_fnet_load)");

	ed_fbn_plan_t bp = {};
	bp.n_layers = nl;
	bp.in_n = net.in_n;
	bp.n_out = net.n_out;
	bp.grid = t->grid;
	bp.max_rows = max_rows;
	bp.w_floats = t->plan.w_floats;
	bp.tab = net.tab;
	bp.slabs = t->plan.slabs;
	const ed_fnet_layer_t &last = net.L[nl - 1];
	const size_t tabn = (size_t)last.rowin_at + (size_t)last.rows;
	std::vector<int32_t> tab(tabn), rtab, inv;
	ED_HIP(ctx, hipSetDevice(ctx->device));
	ED_HIP(ctx, hipStreamSynchronize(ctx->stream));
	ED_HIP(ctx, hipMemcpy(tab.data(), net.tab, tabn * sizeof(int32_t), hipMemcpyDeviceToHost));
	int64_t z_at = 0, out_at = 0;
	int bn_n = 0;
	for (int l = 0; l < nl; l++)
	{
		const ed_fnet_layer_t &L = net.L[l];
		const ed_fnet_geom_t &g = geom[l];
		ed_fbn_layer_t &Q = bp.R[l];
		Q.L = L;
		Q.G = t->plan.G[l];
		Q.rows = L.rows; Q.P = L.P; Q.relu = L.relu;
		Q.R = g.ch * g.cw;
		Q.L.rows = Q.R; Q.L.P = 1; Q.L.relu = 0; Q.L.live = Q.R;
		Q.has_bn = has_bn[l] ? 1 : 0;
		Q.rowin_at = (int32_t)rtab.size();
		Q.bn_at = bn_n;
		Q.in_n = L.in_n; Q.out_n = L.out_n;
		Q.z_at = z_at; Q.out_at = out_at;
		z_at += max_rows * (int64_t)Q.R * L.out_c;
		out_at += max_rows * (int64_t)L.out_n;
		bn_n += L.n_pad;
		/* the row table: the plan's rows r = q P + e first, then the conv positions the pool's floor drops, which have no window */
		const int32_t *rowin = tab.data() + L.rowin_at, *koff = tab.data() + L.koff_at;
		for (int r = 0; r < L.rows; r++) rtab.push_back(rowin[r]);
		for (int cy = 0; cy < g.ch; cy++)
			for (int cx = 0; cx < g.cw; cx++)
				if (cy >= g.oh * g.ph || cx >= g.ow * g.pw) rtab.push_back((cy * g.sh * L.in_w + cx * g.sw) * L.in_c);
		if ((int)(rtab.size() - (size_t)Q.rowin_at) != Q.R) return ed_set_err(ctx, EDISON_E_RUNTIME, "edison_ftrain_set_batchnorm: a record's rows do not cover its conv map");
		/* dX's inverse origin table over these rows: a truncated position reads its window too */
		Q.G.inv_at = (int32_t)inv.size();
		if (l == 0) continue;
		if ((int64_t)Q.G.np * Q.G.T + (int64_t)inv.size() > EDFT_MAX_INV) return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_ftrain_set_batchnorm: the inverse origin tables are too large");
		inv.resize(inv.size() + (size_t)Q.G.np * Q.G.T, -1);
		int32_t *iv = inv.data() + Q.G.inv_at;
		const int32_t *rt = rtab.data() + Q.rowin_at;
		for (int r = 0; r < Q.R; r++)
			for (int tap = 0; tap < Q.G.T; tap++) iv[(size_t)((rt[r] + koff[tap * L.in_c]) / L.in_c) * Q.G.T + tap] = r;
	}
	bp.bn_n = bn_n;
	/* utterances a tile: the trainer's, fewer while dZ over the whole conv map does not fit */
	bp.batch = net.batch;
	while (bp.batch > 1 && ed_fbn_lds_bytes(&bp, bp.batch) > ED_FNET_LDS_BYTES) bp.batch--;
	if (ed_fbn_lds_bytes(&bp, bp.batch) > ED_FNET_LDS_BYTES)
		return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_ftrain_set_batchnorm: one utterance's dZ of the largest record does not fit the LDS");
	if ((int64_t)bp.batch * bp.R[0].R > INT32_MAX / 1024 || z_at > ((int64_t)1 << 33) || out_at > ((int64_t)1 << 33))
		return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_ftrain_set_batchnorm: the stores of max_rows rows are too large");

	const size_t wb = sizeof(float) * (size_t)bp.w_floats, cb = sizeof(float) * (size_t)bn_n;
	float *d_bn = NULL;
	hipError_t e = hipMalloc((void **)&t->d_master, wb);
	if (e == hipSuccess) e = hipMemcpy(t->d_master, net.w, wb, hipMemcpyDeviceToDevice);
	if (e == hipSuccess) e = hipMalloc((void **)&d_bn, 9 * cb);
	t->d_bn = d_bn;
	if (e == hipSuccess) e = hipMalloc((void **)&t->d_bn_m, 2 * cb);
	if (e == hipSuccess) e = hipMalloc((void **)&t->d_bn_v, 2 * cb);
	if (e == hipSuccess) e = hipMemset(t->d_bn_m, 0, 2 * cb);
	if (e == hipSuccess) e = hipMemset(t->d_bn_v, 0, 2 * cb);
	if (e == hipSuccess)
	{
		/* gamma 1, beta 0, gradients 0, moving mean 0, moving variance 1, batch statistics 0 / 0 / 1 */
		std::vector<float> init(9 * (size_t)bn_n, 0.0f);
		for (int i = 0; i < bn_n; i++) init[i] = init[5 * (size_t)bn_n + i] = init[8 * (size_t)bn_n + i] = 1.0f;
		e = hipMemcpy(d_bn, init.data(), 9 * cb, hipMemcpyHostToDevice);
	}
	if (e == hipSuccess) e = hipMalloc((void **)&t->d_rtab, sizeof(int32_t) * rtab.size());
	if (e == hipSuccess) e = hipMemcpy(t->d_rtab, rtab.data(), sizeof(int32_t) * rtab.size(), hipMemcpyHostToDevice);
	if (e == hipSuccess) e = hipMalloc((void **)&t->d_binv, sizeof(int32_t) * (inv.size() ? inv.size() : 1));
	if (e == hipSuccess && inv.size()) e = hipMemcpy(t->d_binv, inv.data(), sizeof(int32_t) * inv.size(), hipMemcpyHostToDevice);
	if (e == hipSuccess) e = hipMalloc((void **)&bp.zs, sizeof(float) * (size_t)z_at);
	if (e == hipSuccess) e = hipMalloc((void **)&bp.outs, sizeof(float) * (size_t)out_at);
	if (e == hipSuccess) e = hipMalloc((void **)&bp.douts, sizeof(float) * (size_t)out_at);
	if (e == hipSuccess) e = hipMalloc((void **)&bp.mask, (size_t)out_at);
	if (e == hipSuccess) e = hipMalloc((void **)&bp.part, sizeof(double) * 2 * (size_t)bn_n * (size_t)t->grid);
	if (e == hipSuccess) e = hipMalloc((void **)&bp.keys, sizeof(uint32_t) * 2 * (size_t)max_rows * (size_t)nl);
	if (e == hipSuccess) e = hipMalloc((void **)&t->d_bplan, sizeof(bp));
	if (e == hipSuccess)
	{
		bp.w = t->d_master;
		bp.rtab = t->d_rtab;
		bp.inv = t->d_binv;
		bp.bnp = d_bn;
		bp.bng = d_bn + 2 * (size_t)bn_n;
		bp.mm = d_bn + 4 * (size_t)bn_n;
		bp.mv = d_bn + 5 * (size_t)bn_n;
		bp.mean = d_bn + 6 * (size_t)bn_n;
		bp.var = d_bn + 7 * (size_t)bn_n;
		bp.rstd = d_bn + 8 * (size_t)bn_n;
		e = hipMemcpy(t->d_bplan, &bp, sizeof(bp), hipMemcpyHostToDevice);
	}
	t->bplan = bp; /* destroy frees whatever was allocated */
	if (e != hipSuccess)
	{
		void **bufs[] = {(void **)&t->d_master, (void **)&t->d_bn, (void **)&t->d_bn_m, (void **)&t->d_bn_v, (void **)&t->d_rtab, (void **)&t->d_binv, (void **)&t->bplan.zs,
		                 (void **)&t->bplan.outs, (void **)&t->bplan.douts, (void **)&t->bplan.mask, (void **)&t->bplan.part, (void **)&t->bplan.keys, (void **)&t->d_bplan};
		for (void **b : bufs)
		{
			if (*b) (void)hipFree(*b);
			*b = NULL;
		}
		return ed_set_err(ctx, e == hipErrorOutOfMemory ? EDISON_E_NO_MEMORY : EDISON_E_RUNTIME, "edison_ftrain_set_batchnorm: cannot allocate the stores of max_rows rows");
	}
	for (int l = 0; l < nl; l++) t->has_bn[l] = bp.R[l].has_bn;
	t->bn_momentum = momentum;
	t->bn_eps = eps;
	t->bn_flags = flags;
	t->bn_on = true;
	t->grad_stale = false;
	/* the copies and memsets above ran on the null stream and the context's stream does not wait for it: done before the fold reads them */
	ED_HIP(ctx, hipDeviceSynchronize());
	return ftrain_fold(t); /* gamma 1, beta 0, mean 0, variance 1: the loaded weights over sqrt(1 + eps) */
}

extern "C" int edison_ftrain_batchnorm_get(edison_ftrain *t, uint8_t *has_bn, double *momentum, double *eps, int64_t *max_rows, uint32_t *flags, int32_t *batch)
{
	{ const int r = ftrain_live(t, "edison_ftrain_batchnorm_get"); if (r != EDISON_OK) return r; }
	if (has_bn)
		for (int l = 0; l < t->plan.net.n_layers; l++) has_bn[l] = t->bn_on ? t->has_bn[l] : 0;
	if (momentum) *momentum = t->bn_on ? t->bn_momentum : 0.0;
	if (eps) *eps = t->bn_on ? t->bn_eps : 0.0;
	if (max_rows) *max_rows = t->bn_on ? t->bplan.max_rows : 0;
	if (flags) *flags = t->bn_on ? t->bn_flags : 0;
	if (batch) *batch = t->bn_on ? t->bplan.batch : 0;
	return EDISON_OK;
}

/* the BatchNorm record `record` of a trainer with BatchNorm on, or an error */
static int ftrain_bn_record(edison_ftrain *t, const char *who, int record)
{
	{ const int r = ftrain_live(t, who); if (r != EDISON_OK) return r; }
	if (!t->bn_on || record < 0 || record >= t->plan.net.n_layers || !t->has_bn[record])
	{
		snprintf(t->ctx->err, sizeof(t->ctx->err), "%s: record %d is not a BatchNorm record of this trainer", who, record);
		return EDISON_E_ARGUMENT;
	}
	return EDISON_OK;
}

static int ftrain_bn_copy(edison_ftrain *t, int record, float *const host[], float *const dev[], int count, bool to_host)
{
	edison_ctx *ctx = t->ctx;
	const ed_fbn_layer_t &Q = t->bplan.R[record];
	ED_HIP(ctx, hipSetDevice(ctx->device));
	for (int i = 0; i < count; i++)
	{
		if (!host[i]) continue;
		if (to_host) ED_HIP(ctx, hipMemcpyAsync(host[i], dev[i] + Q.bn_at, sizeof(float) * (size_t)Q.L.out_c, hipMemcpyDeviceToHost, ctx->stream));
		else ED_HIP(ctx, hipMemcpyAsync(dev[i] + Q.bn_at, host[i], sizeof(float) * (size_t)Q.L.out_c, hipMemcpyHostToDevice, ctx->stream));
	}
	ED_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return EDISON_OK;
}

extern "C" int edison_ftrain_bn_get(edison_ftrain *t, int record, float *gamma, float *beta, float *mean, float *var)
{
	{ const int r = ftrain_bn_record(t, "edison_ftrain_bn_get", record); if (r != EDISON_OK) return r; }
	float *const host[] = {gamma, beta, mean, var};
	float *const dev[] = {t->bplan.bnp, t->bplan.bnp + t->bplan.bn_n, t->bplan.mm, t->bplan.mv};
	return ftrain_bn_copy(t, record, host, dev, 4, true);
}

extern "C" int edison_ftrain_bn_batch_get(edison_ftrain *t, int record, float *mean, float *var)
{
	{ const int r = ftrain_bn_record(t, "edison_ftrain_bn_batch_get", record); if (r != EDISON_OK) return r; }
	float *const host[] = {mean, var};
	float *const dev[] = {t->bplan.mean, t->bplan.var};
	return ftrain_bn_copy(t, record, host, dev, 2, true);
}

extern "C" int edison_ftrain_bn_set(edison_ftrain *t, int record, const float *gamma, const float *beta, const float *mean, const float *var)
{
	{ const int r = ftrain_bn_record(t, "edison_ftrain_bn_set", record); if (r != EDISON_OK) return r; }
	const int oc = t->bplan.R[record].L.out_c;
	const float *all[] = {gamma, beta, mean, var};
	for (const float *a : all)
		for (int c = 0; a && c < oc; c++)
			if (!isfinite(a[c])) return ed_set_err(t->ctx, EDISON_E_ARGUMENT, "edison_ftrain_bn_set: a value is not finite");
	/* in the fold kernel's own arithmetic, float32: what passes here has a finite 1 / sqrtf(var + eps) there */
	for (int c = 0; var && c < oc; c++)
		if (!(var[c] + (float)t->bn_eps > 0.0f)) return ed_set_err(t->ctx, EDISON_E_ARGUMENT, "edison_ftrain_bn_set: a variance is not above -eps");
	float *const host[] = {const_cast<float *>(gamma), const_cast<float *>(beta), const_cast<float *>(mean), const_cast<float *>(var)};
	float *const dev[] = {t->bplan.bnp, t->bplan.bnp + t->bplan.bn_n, t->bplan.mm, t->bplan.mv};
	{ const int r = ftrain_bn_copy(t, record, host, dev, 4, false); if (r != EDISON_OK) return r; }
	return ftrain_fold(t);
}

extern "C" int edison_ftrain_bn_grad_get(edison_ftrain *t, int record, float *dgamma, float *dbeta)
{
	{ const int r = ftrain_bn_record(t, "edison_ftrain_bn_grad_get", record); if (r != EDISON_OK) return r; }
	if (t->grad_stale) return ftrain_stale(t, "edison_ftrain_bn_grad_get");
	float *const host[] = {dgamma, dbeta};
	float *const dev[] = {t->bplan.bng, t->bplan.bng + t->bplan.bn_n};
	return ftrain_bn_copy(t, record, host, dev, 2, true);
}

extern "C" int edison_ftrain_folded_get(edison_ftrain *t, float *packed)
{
	if (!t) return EDISON_E_ARGUMENT;
	return ftrain_copy(t, "edison_ftrain_folded_get", packed, t->plan.net.w, sizeof(float) * (size_t)t->plan.w_floats, hipMemcpyDeviceToHost);
}

/* ---- data sets on the device and whole epochs ---- */
extern "C" int edison_ftrain_data_create(edison_ctx *ctx, int32_t in_n, edison_ftrain_data **out)
{
	if (!ctx || !out) return EDISON_E_ARGUMENT;
	*out = NULL;
	if (in_n < 1) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_data_create: in_n is below 1");
	edison_ftrain_data *d = new (std::nothrow) edison_ftrain_data();
	if (!d) return ed_set_err(ctx, EDISON_E_NO_MEMORY, "edison_ftrain_data_create: out of host memory");
	d->ctx = ctx;
	d->in_n = in_n;
	*out = d;
	return EDISON_OK;
}

extern "C" void edison_ftrain_data_destroy(edison_ftrain_data *d)
{
	if (!d) return;
	(void)hipSetDevice(d->ctx->device);
	(void)hipStreamSynchronize(d->ctx->stream); /* an epoch's gather may still be queued */
	if (d->d_x) (void)hipFree(d->d_x);
	if (d->d_y) (void)hipFree(d->d_y);
	delete d;
}

extern "C" int edison_ftrain_data_info(edison_ftrain_data *d, int64_t *n, int32_t *in_n)
{
	if (!d) return EDISON_E_ARGUMENT;
	if (n) *n = d->n;
	if (in_n) *in_n = d->in_n;
	return EDISON_OK;
}

/* room for n rows; the contents are lost when it grows */
static int fdata_reserve(edison_ftrain_data *d, const char *who, int64_t n)
{
	edison_ctx *ctx = d->ctx;
	if (n > ((int64_t)1 << 31) - 1)
	{
		snprintf(ctx->err, sizeof(ctx->err), "%s: more than 2^31 - 1 rows", who);
		return EDISON_E_SIZE;
	}
	ED_HIP(ctx, hipSetDevice(ctx->device));
	if (n <= d->cap) return EDISON_OK;
	ED_HIP(ctx, hipStreamSynchronize(ctx->stream)); /* a queued launch may still read the old arrays */
	if (d->d_x) (void)hipFree(d->d_x);
	if (d->d_y) (void)hipFree(d->d_y);
	d->d_x = NULL; d->d_y = NULL;
	d->cap = 0; d->n = 0;
	hipError_t e = hipMalloc((void **)&d->d_x, sizeof(float) * (size_t)n * (size_t)d->in_n);
	if (e == hipSuccess) e = hipMalloc((void **)&d->d_y, sizeof(int32_t) * (size_t)n);
	if (e != hipSuccess)
	{
		if (d->d_x) (void)hipFree(d->d_x);
		d->d_x = NULL;
		snprintf(ctx->err, sizeof(ctx->err), "%s: cannot allocate %lld rows of %d floats", who, (long long)n, d->in_n);
		return e == hipErrorOutOfMemory ? EDISON_E_NO_MEMORY : EDISON_E_RUNTIME;
	}
	d->cap = n;
	return EDISON_OK;
}

static int fdata_labels_ok(edison_ctx *ctx, const char *who, const int32_t *y, int64_t n)
{
	for (int64_t i = 0; i < n; i++)
		if (y[i] < 0)
		{
			snprintf(ctx->err, sizeof(ctx->err), "%s: label %d of row %lld is negative", who, y[i], (long long)i);
			return EDISON_E_ARGUMENT;
		}
	return EDISON_OK;
}

static int fdata_set(edison_ftrain_data *d, const char *who, const float *x, const int32_t *y, int64_t n, bool dev)
{
	if (!d) return EDISON_E_ARGUMENT;
	edison_ctx *ctx = d->ctx;
	if (n < 0 || (n > 0 && (!x || !y))) { snprintf(ctx->err, sizeof(ctx->err), "%s: negative n, or NULL rows or labels", who); return EDISON_E_ARGUMENT; }
	ED_HIP(ctx, hipSetDevice(ctx->device));
	std::vector<int32_t> lab;
	try { lab.resize((size_t)n); } catch (...) { return ed_set_err(ctx, EDISON_E_NO_MEMORY, "edison_ftrain_data_set: out of host memory"); }
	if (n && dev)
	{
		ED_HIP(ctx, hipMemcpyAsync(lab.data(), y, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
		ED_HIP(ctx, hipStreamSynchronize(ctx->stream));
	}
	else if (n) memcpy(lab.data(), y, sizeof(int32_t) * (size_t)n);
	{ const int r = fdata_labels_ok(ctx, who, lab.data(), n); if (r != EDISON_OK) return r; }
	{ const int r = fdata_reserve(d, who, n); if (r != EDISON_OK) return r; }
	d->n = 0;
	if (n)
	{
		const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
		ED_HIP(ctx, hipMemcpyAsync(d->d_x, x, sizeof(float) * (size_t)n * (size_t)d->in_n, kind, ctx->stream));
		ED_HIP(ctx, hipMemcpyAsync(d->d_y, lab.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
		ED_HIP(ctx, hipStreamSynchronize(ctx->stream));
	}
	d->y.swap(lab);
	d->n = n;
	return EDISON_OK;
}

extern "C" int edison_ftrain_data_set(edison_ftrain_data *d, const float *x, const int32_t *y, int64_t n) { return fdata_set(d, "edison_ftrain_data_set", x, y, n, false); }

extern "C" int edison_ftrain_data_set_dev(edison_ftrain_data *d, const float *x, const int32_t *y, int64_t n)
{
	return fdata_set(d, "edison_ftrain_data_set_dev", x, y, n, true);
}

extern "C" int edison_ftrain_data_get(edison_ftrain_data *d, float *x, int32_t *y)
{
	if (!d) return EDISON_E_ARGUMENT;
	edison_ctx *ctx = d->ctx;
	ED_HIP(ctx, hipSetDevice(ctx->device));
	if (x && d->n) ED_HIP(ctx, hipMemcpyAsync(x, d->d_x, sizeof(float) * (size_t)d->n * (size_t)d->in_n, hipMemcpyDeviceToHost, ctx->stream));
	if (y && d->n) ED_HIP(ctx, hipMemcpyAsync(y, d->d_y, sizeof(int32_t) * (size_t)d->n, hipMemcpyDeviceToHost, ctx->stream));
	ED_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return EDISON_OK;
}

extern "C" int edison_ftrain_data_audio(edison_ftrain_data *d, const edison_kws_geom *g, int q15, float clip_lo, float clip_hi, const int16_t *audio, int64_t n_utt,
                                        int64_t utt_stride, const int32_t *labels, int64_t chunk)
{
	if (!d) return EDISON_E_ARGUMENT;
	edison_ctx *ctx = d->ctx;
	const char *who = "edison_ftrain_data_audio";
	if (!g) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_data_audio: NULL geometry");
	if (chunk < 1) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_data_audio: chunk is below 1");
	if (n_utt > 0 && !labels) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_data_audio: NULL labels");
	int F = 0;
	/* the checks of edison_kws_float_batch without its network, and the row size; audio is only looked at for NULL here */
	{ const int r = ed_kws_float_features_dev(ctx, g, q15, clip_lo, clip_hi, audio, n_utt, utt_stride, d->in_n, NULL, &F); if (r != EDISON_OK) return r; }
	{ const int r = fdata_labels_ok(ctx, who, labels, n_utt); if (r != EDISON_OK) return r; }
	std::vector<int32_t> lab;
	try { lab.assign(labels, labels + (n_utt > 0 ? n_utt : 0)); } catch (...) { return ed_set_err(ctx, EDISON_E_NO_MEMORY, "edison_ftrain_data_audio: out of host memory"); }
	{ const int r = fdata_reserve(d, who, n_utt); if (r != EDISON_OK) return r; }
	d->n = 0;
	if (n_utt == 0) { d->y.clear(); return EDISON_OK; }
	const int64_t per = chunk < n_utt ? chunk : n_utt, used = (int64_t)(F - 1) * g->frame_step + g->frame_len;
	const unsigned __int128 na = (unsigned __int128)(per - 1) * (unsigned __int128)utt_stride + (unsigned __int128)used;
	if (na * sizeof(int16_t) > ((unsigned __int128)1 << 47)) return ed_set_err(ctx, EDISON_E_SIZE, "edison_ftrain_data_audio: utt_stride x chunk too large");
	ed_dev_buf au;
	if (au.alloc((size_t)na * sizeof(int16_t)) != hipSuccess) return ed_set_err(ctx, EDISON_E_NO_MEMORY, "edison_ftrain_data_audio: cannot allocate a chunk of audio");
	int r = EDISON_OK;
	for (int64_t u0 = 0; u0 < n_utt && r == EDISON_OK; u0 += per)
	{
		const int64_t m = n_utt - u0 < per ? n_utt - u0 : per;
		/* the copy waits in stream order for the feature launch of the chunk before it, which reads the same buffer */
		const hipError_t e = hipMemcpyAsync(au.p, audio + u0 * utt_stride, sizeof(int16_t) * (size_t)((m - 1) * utt_stride + used), hipMemcpyHostToDevice, ctx->stream);
		if (e != hipSuccess) { r = ed_set_err(ctx, EDISON_E_RUNTIME, "edison_ftrain_data_audio: the audio upload failed"); break; }
		r = ed_kws_float_features_dev(ctx, g, q15, clip_lo, clip_hi, (const int16_t *)au.p, m, utt_stride, d->in_n, d->d_x + u0 * (int64_t)d->in_n, NULL);
	}
	if (r == EDISON_OK && hipMemcpyAsync(d->d_y, lab.data(), sizeof(int32_t) * (size_t)n_utt, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
		r = ed_set_err(ctx, EDISON_E_RUNTIME, "edison_ftrain_data_audio: the label upload failed");
	if (hipStreamSynchronize(ctx->stream) != hipSuccess && r == EDISON_OK) r = ed_set_err(ctx, EDISON_E_RUNTIME, "edison_ftrain_data_audio: hipStreamSynchronize failed");
	if (r != EDISON_OK) return r; /* the set stays empty */
	d->y.swap(lab);
	d->n = n_utt;
	return EDISON_OK;
}

/* room for `rows` rows of loss, argmax, order and labels, and for `xrows` gathered rows */
static int ftrain_epoch_reserve(edison_ftrain *t, int64_t rows, int64_t xrows)
{
	edison_ctx *ctx = t->ctx;
	if (!t->d_esums && hipMalloc((void **)&t->d_esums, sizeof(ed_fdata_sums_t)) != hipSuccess)
		return ed_set_err(ctx, EDISON_E_NO_MEMORY, "edison_ftrain_epoch: cannot allocate the epoch store");
	if (rows > t->e_cap || xrows > t->ex_cap) ED_HIP(ctx, hipStreamSynchronize(ctx->stream)); /* a queued call may still use the old arrays */
	if (rows > t->e_cap)
	{
		void **bufs[] = {(void **)&t->d_eloss, (void **)&t->d_eam, (void **)&t->d_eorder, (void **)&t->d_ey};
		t->e_cap = 0; t->e_n = 0;
		hipError_t e = hipSuccess;
		for (void **b : bufs)
		{
			if (*b) (void)hipFree(*b);
			*b = NULL;
			if (e == hipSuccess) e = hipMalloc(b, 4 * (size_t)rows);
		}
		if (e != hipSuccess) return ed_set_err(ctx, EDISON_E_NO_MEMORY, "edison_ftrain_epoch: cannot allocate the epoch store");
		t->e_cap = rows;
	}
	if (xrows > t->ex_cap)
	{
		if (t->d_ex) (void)hipFree(t->d_ex);
		t->d_ex = NULL;
		t->ex_cap = 0;
		if (hipMalloc((void **)&t->d_ex, sizeof(float) * (size_t)xrows * (size_t)t->plan.net.in_n) != hipSuccess)
			return ed_set_err(ctx, EDISON_E_NO_MEMORY, "edison_ftrain_epoch: cannot allocate the epoch's copy of the rows");
		t->ex_cap = xrows;
	}
	return EDISON_OK;
}

/* the checks an epoch and an eval share: a live trainer, a data set of this context and of the network's input size */
static int ftrain_data_ok(edison_ftrain *t, edison_ftrain_data *d, const char *who)
{
	{ const int r = ftrain_live(t, who); if (r != EDISON_OK) return r; }
	edison_ctx *ctx = t->ctx;
	if (!d || d->ctx != ctx) { snprintf(ctx->err, sizeof(ctx->err), "%s: NULL data set, or one of another context", who); return EDISON_E_ARGUMENT; }
	if (d->in_n != t->plan.net.in_n)
	{
		snprintf(ctx->err, sizeof(ctx->err), "%s: the data set's rows have %d floats, the network's input %d", who, d->in_n, t->plan.net.in_n);
		return EDISON_E_SIZE;
	}
	return EDISON_OK;
}

static int ftrain_label_refused(edison_ftrain *t, const char *who, int32_t label, int64_t row)
{
	snprintf(t->ctx->err, sizeof(t->ctx->err), "%s: label %d of the data set's row %lld is outside 0 .. %d", who, label, (long long)row, t->plan.net.n_out - 1);
	return EDISON_E_ARGUMENT;
}

/* the reduction over the first n rows of the epoch store against `labels`, one copy back, one synchronisation */
static int ftrain_epoch_finish(edison_ftrain *t, const int32_t *labels, int64_t n, int64_t steps, edison_ftrain_epoch_t *out)
{
	edison_ctx *ctx = t->ctx;
	ed_fdata_sums_t sums = {0.0, 0};
	{ const int r = ed_launch_result(ctx, ed_launch_fdata_reduce(t->d_eloss, t->d_eam, labels, n, t->d_esums, ctx->stream), "epoch reduction kernel"); if (r != EDISON_OK) return r; }
	ED_HIP(ctx, hipMemcpyAsync(&sums, t->d_esums, sizeof(sums), hipMemcpyDeviceToHost, ctx->stream));
	ED_HIP(ctx, hipStreamSynchronize(ctx->stream));
	out->loss_sum = sums.loss_sum;
	out->hits = sums.hits;
	out->seen = n;
	out->steps = steps;
	return EDISON_OK;
}

extern "C" int edison_ftrain_epoch(edison_ftrain *t, edison_ftrain_data *d, const int32_t *order, int64_t n_order, int64_t batch, double lr, int64_t max_steps,
                                   edison_ftrain_epoch_t *out)
{
	const char *who = "edison_ftrain_epoch";
	{ const int r = ftrain_data_ok(t, d, who); if (r != EDISON_OK) return r; }
	edison_ctx *ctx = t->ctx;
	if (!out || n_order < 0 || (n_order > 0 && !order)) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_epoch: NULL out or order, or negative n_order");
	if (batch < 1) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_epoch: batch is below 1");
	if (!(lr >= 0.0) || !isfinite(lr)) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_epoch: the learning rate is negative or not finite");
	if (n_order > ((int64_t)1 << 31) - 1) return ed_set_err(ctx, EDISON_E_SIZE, "edison_ftrain_epoch: more than 2^31 - 1 rows in one epoch");
	if (t->bn_on && batch > t->bplan.max_rows)
	{
		snprintf(ctx->err, sizeof(ctx->err), "edison_ftrain_epoch: a training call with BatchNorm takes at most max_rows = %lld rows (edison_ftrain_set_batchnorm), batch is %lld",
		         (long long)t->bplan.max_rows, (long long)batch);
		return EDISON_E_ARGUMENT;
	}
	int64_t steps = (n_order + batch - 1) / batch; /* the last batch may be short */
	if (max_steps >= 0 && steps > max_steps) steps = max_steps;
	const int64_t rows = steps * batch < n_order ? steps * batch : n_order;
	for (int64_t i = 0; i < rows; i++)
	{
		if (order[i] < 0 || order[i] >= d->n)
		{
			snprintf(ctx->err, sizeof(ctx->err), "edison_ftrain_epoch: order[%lld] = %d is no row of the data set (%lld rows)", (long long)i, order[i], (long long)d->n);
			return EDISON_E_ARGUMENT;
		}
		const int32_t y = d->y[(size_t)order[i]];
		if (y >= t->plan.net.n_out) return ftrain_label_refused(t, who, y, order[i]);
	}
	if (t->bn_on && (t->bn_flags & EDISON_FTRAIN_BN_UNBIASED) && rows > 0) /* what the last, shortest batch's gradient call would refuse */
		for (int l = 0; l < t->bplan.n_layers; l++)
			if (t->has_bn[l] && (rows - (steps - 1) * batch) * t->bplan.R[l].R < 2)
				return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_epoch: the last batch gives a BatchNorm record N < 2 values; the unbiased variance needs two");
	ED_HIP(ctx, hipSetDevice(ctx->device));
	{ const int r = ftrain_epoch_reserve(t, rows, rows); if (r != EDISON_OK) return r; }
	t->e_n = 0;
	if (rows == 0) { *out = (edison_ftrain_epoch_t){0.0, 0, 0, 0}; return EDISON_OK; }
	/* pageable host memory: the copy has left `order` when the call returns */
	ED_HIP(ctx, hipMemcpyAsync(t->d_eorder, order, sizeof(int32_t) * (size_t)rows, hipMemcpyHostToDevice, ctx->stream));
	{
		const int r = ed_launch_result(ctx, ed_launch_fdata_gather(d->d_x, d->d_y, t->d_eorder, rows, d->in_n, t->d_ex, t->d_ey, ctx->n_cu, ctx->stream), "epoch gather kernel");
		if (r != EDISON_OK) return r;
	}
	const int64_t in_n = d->in_n;
	for (int64_t s = 0; s < steps; s++)
	{
		const int64_t b0 = s * batch, m = rows - b0 < batch ? rows - b0 : batch;
		int r = edison_ftrain_grad_dev_ex(t, t->d_ex + b0 * in_n, t->d_ey + b0, m, t->d_eloss + b0, t->d_eam + b0, 0);
		if (r == EDISON_OK) r = edison_ftrain_step(t, lr);
		if (r != EDISON_OK)
		{
			(void)hipStreamSynchronize(ctx->stream);
			return r;
		}
	}
	t->e_n = rows;
	return ftrain_epoch_finish(t, t->d_ey, rows, steps, out);
}

#define EDFT_EVAL_ROWS 4096 /* rows an EVAL call of edison_ftrain_data_eval takes */

extern "C" int edison_ftrain_data_eval(edison_ftrain *t, edison_ftrain_data *d, edison_ftrain_epoch_t *out)
{
	const char *who = "edison_ftrain_data_eval";
	{ const int r = ftrain_data_ok(t, d, who); if (r != EDISON_OK) return r; }
	edison_ctx *ctx = t->ctx;
	if (!out) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_ftrain_data_eval: NULL out");
	for (int64_t i = 0; i < d->n; i++)
		if (d->y[(size_t)i] >= t->plan.net.n_out) return ftrain_label_refused(t, who, d->y[(size_t)i], i);
	ED_HIP(ctx, hipSetDevice(ctx->device));
	{ const int r = ftrain_epoch_reserve(t, d->n, 0); if (r != EDISON_OK) return r; }
	t->e_n = 0;
	if (d->n == 0) { *out = (edison_ftrain_epoch_t){0.0, 0, 0, 0}; return EDISON_OK; }
	for (int64_t b0 = 0; b0 < d->n; b0 += EDFT_EVAL_ROWS)
	{
		const int64_t m = d->n - b0 < EDFT_EVAL_ROWS ? d->n - b0 : EDFT_EVAL_ROWS;
		const int r = edison_ftrain_grad_dev_ex(t, d->d_x + b0 * (int64_t)d->in_n, d->d_y + b0, m, t->d_eloss + b0, t->d_eam + b0, EDISON_FTRAIN_EVAL);
		if (r != EDISON_OK)
		{
			(void)hipStreamSynchronize(ctx->stream);
			return r;
		}
	}
	t->e_n = d->n;
	return ftrain_epoch_finish(t, d->d_y, d->n, 0, out);
}

extern "C" int edison_ftrain_epoch_rows(edison_ftrain *t, float *loss, int32_t *argmax, int64_t *n)
{
	{ const int r = ftrain_live(t, "edison_ftrain_epoch_rows"); if (r != EDISON_OK) return r; }
	edison_ctx *ctx = t->ctx;
	ED_HIP(ctx, hipSetDevice(ctx->device));
	if (n) *n = t->e_n;
	if (loss && t->e_n) ED_HIP(ctx, hipMemcpyAsync(loss, t->d_eloss, sizeof(float) * (size_t)t->e_n, hipMemcpyDeviceToHost, ctx->stream));
	if (argmax && t->e_n) ED_HIP(ctx, hipMemcpyAsync(argmax, t->d_eam, sizeof(int32_t) * (size_t)t->e_n, hipMemcpyDeviceToHost, ctx->stream));
	ED_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return EDISON_OK;
}
