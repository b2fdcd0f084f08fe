/*
 * edison_fnet.hip -- C-ABI of the float32 X-CUBE-AI network path (include/edison_hip.h, edison_fnet_* and edison_kws_float_batch*;
 * DESIGN.md sections 14 and 14b): the .ednf blob (edison_amd/cube_import.py; version 1, or version 2 with conv and pool pads) is checked and turned into the kernel's plan (fnet.h), and the
 * network runs on fnet_kernels.hip. edison_kws_float_batch* puts a feature stage in front of it: the float64 MFCC at any geometry
 * (mfcc_geom_kernels.hip) -> float32 x net_input_scale -> clip (the reference's host flow), or variant C -> (float) (the firmware's).
 * The int8 NNoM model of the context is not touched: a context may hold both.
 * A network the one-launch kernel cannot hold (edison_fnet_load_ex, EDISON_FNET_LARGE) is a layered one: plan.batch 0, run record by
 * record on fnet_layer_kernels.hip between two buffers of the context's workspace (run_layered).
 */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "edison_ctx.h"
#include "fnet.h"

#define EDF_T_CONV 1
#define EDF_T_SOFTMAX 2
#define EDF_REC_INTS 24 /* version 2; version 1 has the first 16 and no pads */
#define EDF_HDR_BYTES 32
#define EDF_MAX_DIM 4096

struct ed_fnet
{
	ed_fnet_plan_t plan; /* w / tab point into d */
	int32_t in_h, in_w, in_c;
	ed_fnet_geom_t geom[ED_FNET_MAX_LAYERS];
	void *d;
	bool layered; /* runs on the layer road (fnet_layer_kernels.hip): plan.batch is 0 */
};

void ed_ctx_fnet_free(edison_ctx *ctx)
{
	if (!ctx || !ctx->fnet) return;
	if (ctx->fnet->d) (void)hipFree(ctx->fnet->d);
	delete ctx->fnet;
	ctx->fnet = NULL;
}

const ed_fnet_plan_t *ed_ctx_fnet_plan(const edison_ctx *ctx) { return ctx && ctx->fnet ? &ctx->fnet->plan : NULL; }
const ed_fnet_geom_t *ed_ctx_fnet_geom(const edison_ctx *ctx) { return ctx && ctx->fnet ? ctx->fnet->geom : NULL; }
int ed_ctx_fnet_layered(const edison_ctx *ctx) { return ctx && ctx->fnet && ctx->fnet->layered; }

int ed_fnet_refuse_layered(edison_ctx *ctx, const char *who)
{
	snprintf(ctx->err, sizeof(ctx->err), "%s: the loaded float network runs on the layer road (edison_fnet_load_ex), which this does not serve", who);
	return EDISON_E_NO_IMPL;
}

static size_t ws_cap(const edison_ctx *ctx) { return ctx->fnet_ws_cap ? ctx->fnet_ws_cap : ED_FNET_WORKSPACE_DEFAULT; }

/* Bytes of the layer road's scratch per utterance: one row of each of its two buffers. */
static size_t ws_per_utt(const ed_fnet_plan_t &p) { return sizeof(float) * ((size_t)p.buf_n[0] + (size_t)p.buf_n[1]); }

/* Utterances per chunk of a layered plan under a cap of `cap` bytes (0: one utterance does not fit): as many as the cap holds and the
 * kernel's int indices allow, whole M blocks of a dense record where there are that many. */
static int64_t ws_chunk(const ed_fnet_plan_t &p, size_t cap)
{
	int64_t chunk = (int64_t)(cap / ws_per_utt(p));
	int64_t most = INT32_MAX / (p.buf_n[0] > p.buf_n[1] ? p.buf_n[0] : p.buf_n[1]);
	for (int l = 0; l < p.n_layers; l++)
		if (INT32_MAX / 16 / p.L[l].rows < most) most = INT32_MAX / 16 / p.L[l].rows;
	if (chunk > most) chunk = most;
	if (chunk > ED_FNET_LAYER_MB) chunk -= chunk % ED_FNET_LAYER_MB;
	return chunk;
}

static int ws_too_small(edison_ctx *ctx, const char *who, const ed_fnet_plan_t &p, size_t cap)
{
	snprintf(ctx->err, sizeof(ctx->err), "%s: one utterance's activations (%zu bytes) exceed the workspace cap of %zu bytes (edison_fnet_set_workspace)",
	         who, ws_per_utt(p), cap);
	return EDISON_E_NO_MEMORY;
}

static int32_t rd32(const uint8_t *p)
{
	int32_t v;
	memcpy(&v, p, 4);
	return v;
}

static int bad(edison_ctx *ctx, const char *msg)
{
	snprintf(ctx->err, sizeof(ctx->err), "edison_fnet_load: %s", msg);
	return EDISON_E_SIZE;
}

/* Checks the blob and fills *f (plan with offsets, not yet device pointers) and the host images of the weights and the tables. */
static int parse(edison_ctx *ctx, const uint8_t *b, size_t nb, unsigned flags, ed_fnet *f, float **w_out, size_t *nw_out, int32_t **tab_out, size_t *nt_out)
{
	/* EDISON_FNET_LARGE lifts the two LDS refusals and the EDF_MAX_DIM bound on a record's in_c (a dense record is inp = (1, 1, n)) up
	 * to what kh kw ic <= 1 << 16 allows; a network it lets through, and any network under EDISON_FNET_LAYERED, is a layered one */
	const bool large = (flags & EDISON_FNET_LARGE) != 0;
	bool layered = (flags & EDISON_FNET_LAYERED) != 0;
	if (nb < EDF_HDR_BYTES || memcmp(b, "EDNF", 4) != 0) return bad(ctx, "not an .ednf blob (magic)");
	const int ver = rd32(b + 4);
	if (ver != 1 && ver != 2) return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_fnet_load: .ednf version is not 1 or 2");
	const int ri = ver == 1 ? 16 : EDF_REC_INTS; /* ints per record */
	const int nl = rd32(b + 8), in_h = rd32(b + 12), in_w = rd32(b + 16), in_c = rd32(b + 20), n_out = rd32(b + 24), kwb = rd32(b + 28);
	if (nl < 2 || nl > ED_FNET_MAX_LAYERS + 1) return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_fnet_load: 2 .. 17 layer records");
	if (in_h < 1 || in_w < 1 || in_c < 1 || in_h > EDF_MAX_DIM || in_w > EDF_MAX_DIM || in_c > EDF_MAX_DIM || kwb < 0 || kwb % 4)
		return bad(ctx, "bad header");
	if ((int64_t)in_h * in_w * in_c > (1 << 20)) return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_fnet_load: input too large");
	size_t off = EDF_HDR_BYTES + (size_t)nl * ri * 4;
	if (off + (size_t)kwb > nb) return bad(ctx, "truncated records");
	const uint8_t *rec0 = b + EDF_HDR_BYTES;
	off += (size_t)kwb;
	memset(f, 0, sizeof(*f));
	ed_fnet_plan_t &p = f->plan;
	f->in_h = in_h; f->in_w = in_w; f->in_c = in_c;
	int h = in_h, w = in_w, c = in_c;
	int64_t wfl = 0, tabn = 0, acts = 0;
	int buf[2] = {h * w * c, 0};
	int n_conv = 0;
	/* pass 1: shapes, sizes */
	for (int i = 0; i < nl; i++)
	{
		const uint8_t *r = rec0 + (size_t)i * ri * 4;
		int v[EDF_REC_INTS] = {0};
		for (int j = 0; j < ri; j++) v[j] = rd32(r + 4 * j);
		if (v[0] != EDF_T_CONV && v[0] != EDF_T_SOFTMAX) return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_fnet_load: unknown layer type");
		for (int j = 1; j <= (v[0] == EDF_T_CONV ? 15 : 6); j++)
			if (v[j] < (j == 11 ? 0 : 1) || v[j] > EDF_MAX_DIM * (j >= 14 || (j == 3 && large) ? 16 : 1)) return bad(ctx, "layer field out of range");
		if (v[0] == EDF_T_CONV)
			for (int j = 16; j < EDF_REC_INTS; j++)
				if (v[j] < 0 || v[j] > EDF_MAX_DIM) return bad(ctx, "a pad is negative or out of range");
		const int64_t cur = (int64_t)h * w * c;
		if ((int64_t)v[1] * v[2] * v[3] != cur) return bad(ctx, "a layer's input size differs from the previous layer's output");
		if (v[0] == EDF_T_SOFTMAX)
		{
			if (i != nl - 1) return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_fnet_load: softmax only as the last layer");
			if ((int64_t)v[4] * v[5] * v[6] != cur) return bad(ctx, "softmax changes the size");
			continue;
		}
		if (i == nl - 1) return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_fnet_load: the network must end in a softmax");
		const int ih = v[1], iw = v[2], ic = v[3], kh = v[7], kw = v[8], sh = v[9], sw = v[10], ph = v[12], pw = v[13];
		const int pt = v[16], pl = v[17], pb = v[18], pr = v[19], qt = v[20], ql = v[21], qb = v[22], qr = v[23];
		/* a pad as large as its window's extent would give windows wholly in padding: refused, so every window has a real element */
		if (pt >= kh || pb >= kh || pl >= kw || pr >= kw)
			return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_fnet_load: a conv pad must be smaller than the kernel on its axis");
		if (qt >= ph || qb >= ph || ql >= pw || qr >= pw)
			return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_fnet_load: a pool pad must be smaller than the pool window on its axis");
		if (kh > ih + pt + pb || kw > iw + pl + pr) return bad(ctx, "kernel larger than its padded input");
		const int oh = (ih + pt + pb - kh) / sh + 1, ow = (iw + pl + pr - kw) / sw + 1;
		const int Ph = oh + qt + qb >= ph ? (oh + qt + qb - ph) / ph + 1 : 0, Pw = ow + ql + qr >= pw ? (ow + ql + qr - pw) / pw + 1 : 0;
		if (v[4] != Ph || v[5] != Pw) return bad(ctx, "output shape does not follow from the conv and pool");
		if ((int64_t)v[4] * v[5] * v[6] * ph * pw > (1 << 20) || (int64_t)kh * kw * ic > (1 << 16))
			return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_fnet_load: layer too large");
		const int P = ph * pw;
		if (P != 1 && P != 2 && P != 4) return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_fnet_load: pool windows of 1, 2 or 4 elements");
		if (v[11] > 1) return bad(ctx, "relu flag");
		const int K = kh * kw * ic, oc = v[6];
		if (v[14] != (K + 3) / 4 * 4 || v[15] != (oc + 15) / 16 * 16) return bad(ctx, "k_pad / n_pad");
		/* not reachable while nl <= ED_FNET_MAX_LAYERS + 1 and the last record must be the softmax; kept beside p.L's bound */
		if (n_conv == ED_FNET_MAX_LAYERS) return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_fnet_load: at most 16 conv / dense layers");
		ed_fnet_layer_t &L = p.L[n_conv];
		f->geom[n_conv] = (ed_fnet_geom_t){sh, sw, ph, pw, oh, ow, v[4], v[5]};
		L.in_n = ih * iw * ic;
		L.out_c = oc;
		L.out_n = v[4] * v[5] * oc;
		L.P = P;
		L.rows = v[4] * v[5] * P;
		L.k_pad = v[14];
		L.n_pad = v[15];
		L.relu = v[11];
		L.src = n_conv & 1;
		L.dst = L.src ^ 1;
		L.w_at = wfl;
		L.koff_at = (int32_t)tabn;
		L.pad = (pt | pl | pb | pr | qt | ql | qb | qr) != 0;
		L.in_h = ih; L.in_w = iw; L.in_c = ic;
		const int kn = L.pad ? 2 * L.k_pad : L.k_pad; /* koff, and behind it a padded record's kyx */
		L.rowin_at = (int32_t)(tabn + kn);
		{
			/* rows of the pool windows that lie on the conv's map: the others are absent */
			int lh = 0, lw = 0;
			for (int y = 0; y < Ph * ph; y++) lh += y >= qt && y - qt < oh;
			for (int x = 0; x < Pw * pw; x++) lw += x >= ql && x - ql < ow;
			L.live = lh * lw;
		}
		L.acts_at = (int32_t)acts;
		const int64_t wl = (int64_t)L.k_pad * L.n_pad;
		if (wl > ED_FNET_LDS_BYTES / 4)
		{
			if (!large) return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_fnet_load: a layer's weights exceed the LDS");
			layered = true;
		}
		wfl += wl + L.n_pad;
		tabn += kn + L.rows;
		acts += L.out_n;
		if ((int64_t)L.out_n > (1 << 20) || tabn > (1 << 26) || acts > (1 << 26)) return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_fnet_load: network too large");
		if (L.out_n > buf[L.dst]) buf[L.dst] = L.out_n;
		if (wl > p.w_lds) p.w_lds = (int32_t)wl;
		if (kn > p.k_lds) p.k_lds = kn;
		h = v[4]; w = v[5]; c = oc;
		n_conv++;
	}
	if (n_conv < 1 || (int64_t)h * w * c != n_out) return bad(ctx, "n_out differs from the last layer's output");
	if (off + (size_t)wfl * 4 != nb) return bad(ctx, "blob size does not match its records");
	p.n_layers = n_conv;
	p.in_n = in_h * in_w * in_c;
	p.n_out = n_out;
	p.buf_n[0] = (buf[0] + 3) & ~3;
	p.buf_n[1] = (buf[1] + 3) & ~3;
	p.acts_n = (int32_t)acts;
	/* utterances per workgroup: as many as the LDS holds beside the largest layer's weights, at most ED_FNET_MAX_BATCH */
	const int64_t fixed = 4 * ((int64_t)p.w_lds + p.k_lds), per = 4 * ((int64_t)p.buf_n[0] + p.buf_n[1]);
	int64_t batch = (ED_FNET_LDS_BYTES - fixed) / per;
	if (batch > ED_FNET_MAX_BATCH) batch = ED_FNET_MAX_BATCH;
	if (batch < 1)
	{
		if (!large) return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_fnet_load: one utterance's activations and the largest layer do not fit the LDS");
		layered = true;
	}
	p.batch = layered ? 0 : (int32_t)batch; /* 0: ed_fnet_plan_launchable keeps every in-LDS launcher off a layered plan */
	f->layered = layered;
	if ((int64_t)p.batch * p.L[n_conv - 1].rows > INT32_MAX / 16) return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_fnet_load: network too large");
	if (layered && ws_chunk(p, ws_cap(ctx)) < 1) return ws_too_small(ctx, "edison_fnet_load", p, ws_cap(ctx));

	/* pass 2: weights (already in the kernel's layout) and the koff / rowin tables */
	float *wh = (float *)malloc(sizeof(float) * (size_t)(wfl ? wfl : 1));
	int32_t *th = (int32_t *)malloc(sizeof(int32_t) * (size_t)(tabn ? tabn : 1));
	if (!wh || !th) { free(wh); free(th); return ed_set_err(ctx, EDISON_E_NO_MEMORY, "host allocation failed"); }
	memcpy(wh, b + off, (size_t)wfl * 4);
	for (int i = 0, l = 0; i < nl; i++)
	{
		const uint8_t *r = rec0 + (size_t)i * ri * 4;
		if (rd32(r) != EDF_T_CONV) continue;
		int v[EDF_REC_INTS] = {0};
		for (int j = 0; j < ri; j++) v[j] = rd32(r + 4 * j);
		const ed_fnet_layer_t &L = p.L[l++];
		const int ih = v[1], iw = v[2], ic = v[3], kh = v[7], kw = v[8], sh = v[9], sw = v[10], ph = v[12], pw = v[13], ow = v[5];
		int32_t *koff = th + L.koff_at, *rowin = th + L.rowin_at;
		for (int k = 0; k < L.k_pad; k++)
		{
			if (k >= kh * kw * ic) { koff[k] = -1; if (L.pad) koff[L.k_pad + k] = 0; continue; }
			const int ci = k % ic, t = k / ic, kx = t % kw, ky = t / kw;
			koff[k] = (ky * iw + kx) * ic + ci;
			if (L.pad) koff[L.k_pad + k] = ky << 16 | kx;
		}
		/* the conv's map, before the pool */
		const int ch = (ih + v[16] + v[18] - kh) / sh + 1, cw = (iw + v[17] + v[19] - kw) / sw + 1;
		for (int rr = 0; rr < L.rows; rr++)
		{
			const int q = rr / L.P, e = rr % L.P, py = q / ow, px = q % ow, ey = e / pw, ex = e % pw;
			if (!L.pad) { rowin[rr] = ((py * ph + ey) * sh * iw + (px * pw + ex) * sw) * ic; continue; }
			const int cy = py * ph + ey - v[20], cx = px * pw + ex - v[21];
			if (cy < 0 || cy >= ch || cx < 0 || cx >= cw) { rowin[rr] = -1; continue; } /* absent: in the pool's padding */
			rowin[rr] = (cy * sh - v[16] + ED_FNET_ORIGIN_BIAS) << 16 | (cx * sw - v[17] + ED_FNET_ORIGIN_BIAS);
		}
	}
	*w_out = wh; *nw_out = (size_t)wfl; *tab_out = th; *nt_out = (size_t)tabn;
	return EDISON_OK;
}

static int bad_flags(edison_ctx *ctx, unsigned flags)
{
	if (!(flags & ~(EDISON_FNET_LARGE | EDISON_FNET_LAYERED))) return EDISON_OK;
	return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_fnet_load_ex: flags has a bit other than EDISON_FNET_LARGE and EDISON_FNET_LAYERED");
}

extern "C" int edison_fnet_load_mem(edison_ctx *ctx, const void *blob, size_t blob_bytes) { return edison_fnet_load_mem_ex(ctx, blob, blob_bytes, 0); }

extern "C" int edison_fnet_load_mem_ex(edison_ctx *ctx, const void *blob, size_t blob_bytes, unsigned flags)
{
	if (!ctx || !blob) return EDISON_E_ARGUMENT;
	{ const int r = bad_flags(ctx, flags); if (r != EDISON_OK) return r; }
	ed_fnet *f = new (std::nothrow) ed_fnet();
	if (!f) return ed_set_err(ctx, EDISON_E_NO_MEMORY, "host allocation failed");
	float *wh = NULL;
	int32_t *th = NULL;
	size_t nw = 0, nt = 0;
	{ const int r = parse(ctx, (const uint8_t *)blob, blob_bytes, flags, f, &wh, &nw, &th, &nt); if (r != EDISON_OK) { delete f; return r; } }
	const size_t wbytes = (sizeof(float) * nw + 255) & ~(size_t)255, bytes = wbytes + sizeof(int32_t) * nt;
	hipError_t e = hipSetDevice(ctx->device);
	if (e == hipSuccess) e = hipMalloc(&f->d, bytes);
	if (e == hipSuccess) e = hipMemcpy(f->d, wh, sizeof(float) * nw, hipMemcpyHostToDevice);
	if (e == hipSuccess) e = hipMemcpy((char *)f->d + wbytes, th, sizeof(int32_t) * nt, hipMemcpyHostToDevice);
	free(wh);
	free(th);
	if (e != hipSuccess)
	{
		if (f->d) (void)hipFree(f->d);
		delete f;
		if (e == hipErrorOutOfMemory) return ed_set_err(ctx, EDISON_E_NO_MEMORY, "edison_fnet_load: hipMalloc: out of HBM");
		ED_HIP(ctx, e);
	}
	f->plan.w = (const float *)f->d;
	f->plan.tab = (const int32_t *)((char *)f->d + wbytes);
	/* queued launches may still read the old network */
	if (ctx->fnet)
	{
		e = hipStreamSynchronize(ctx->stream);
		if (e != hipSuccess) { (void)hipFree(f->d); delete f; ED_HIP(ctx, e); }
		ed_ctx_fnet_free(ctx);
	}
	ctx->fnet = f;
	ctx->fnet_epoch++;
	return EDISON_OK;
}

extern "C" int edison_fnet_load(edison_ctx *ctx, const char *ednf_path) { return edison_fnet_load_ex(ctx, ednf_path, 0); }

extern "C" int edison_fnet_load_ex(edison_ctx *ctx, const char *ednf_path, unsigned flags)
{
	if (!ctx || !ednf_path) return EDISON_E_ARGUMENT;
	{ const int r = bad_flags(ctx, flags); if (r != EDISON_OK) return r; }
	FILE *fp = fopen(ednf_path, "rb");
	if (!fp) { snprintf(ctx->err, sizeof(ctx->err), "edison_fnet_load: cannot open %s", ednf_path); return EDISON_E_ARGUMENT; }
	fseek(fp, 0, SEEK_END);
	const long n = ftell(fp);
	fseek(fp, 0, SEEK_SET);
	if (n <= 0 || n > (1L << 30)) { fclose(fp); return bad(ctx, "empty or oversized file"); }
	void *buf = malloc((size_t)n);
	if (!buf) { fclose(fp); return ed_set_err(ctx, EDISON_E_NO_MEMORY, "host allocation failed"); }
	const size_t got = fread(buf, 1, (size_t)n, fp);
	fclose(fp);
	const int r = got == (size_t)n ? edison_fnet_load_mem_ex(ctx, buf, (size_t)n, flags) : bad(ctx, "short read");
	free(buf);
	return r;
}

extern "C" int edison_fnet_info(edison_ctx *ctx, edison_fnet_info_t *out)
{
	if (!ctx || !out) return EDISON_E_ARGUMENT;
	if (!ctx->fnet) return ed_set_err(ctx, EDISON_E_NO_MODEL, "no float network loaded (edison_fnet_load)");
	const ed_fnet *f = ctx->fnet;
	out->in_h = f->in_h; out->in_w = f->in_w; out->in_c = f->in_c;
	out->n_out = f->plan.n_out;
	out->n_layers = f->plan.n_layers;
	out->acts_floats = f->plan.acts_n;
	out->batch = f->plan.batch;
	out->lds_bytes = f->layered ? ED_FNET_LAYER_LDS_BYTES : (int32_t)ed_fnet_lds_bytes(&f->plan);
	return EDISON_OK;
}

extern "C" int edison_fnet_set_workspace(edison_ctx *ctx, size_t max_bytes)
{
	if (!ctx) return EDISON_E_ARGUMENT;
	const size_t cap = max_bytes ? max_bytes : ED_FNET_WORKSPACE_DEFAULT;
	if (ctx->fnet && ctx->fnet->layered && ws_chunk(ctx->fnet->plan, cap) < 1) return ws_too_small(ctx, "edison_fnet_set_workspace", ctx->fnet->plan, cap);
	ctx->fnet_ws_cap = max_bytes;
	return EDISON_OK;
}

/* The layer road for n utterances: the chunk the cap allows, the scratch grown to it (a growth synchronises the stream once). */
static int run_layered(edison_ctx *ctx, const float *in, int64_t n, float *logits, float *probs, int32_t *argmax, float *acts, float *ms)
{
	const ed_fnet_plan_t &p = ctx->fnet->plan;
	int64_t chunk = ws_chunk(p, ws_cap(ctx));
	if (chunk < 1) return ws_too_small(ctx, "edison_fnet_batch", p, ws_cap(ctx));
	if (chunk > n) chunk = n;
	const size_t b0 = (sizeof(float) * (size_t)chunk * (size_t)p.buf_n[0] + 255) & ~(size_t)255, need = b0 + sizeof(float) * (size_t)chunk * (size_t)p.buf_n[1];
	if (need > ctx->fnet_ws_bytes)
	{
		ED_HIP(ctx, hipStreamSynchronize(ctx->stream));
		if (ctx->fnet_ws) (void)hipFree(ctx->fnet_ws);
		ctx->fnet_ws = NULL;
		ctx->fnet_ws_bytes = 0;
		const hipError_t e = hipMalloc(&ctx->fnet_ws, need);
		if (e == hipErrorOutOfMemory) { ctx->fnet_ws = NULL; return ed_set_err(ctx, EDISON_E_NO_MEMORY, "edison_fnet_batch: hipMalloc of the layer road's workspace: out of HBM"); }
		ED_HIP(ctx, e);
		ctx->fnet_ws_bytes = need;
	}
	float *const ws[2] = {(float *)ctx->fnet_ws, (float *)((char *)ctx->fnet_ws + b0)};
	const int e = ed_launch_fnet_layered(&p, in, n, chunk, ws, logits, probs, argmax, acts, ms, ctx->stream);
	return ed_launch_result(ctx, e, "float network layer kernel");
}

static int need_net(edison_ctx *ctx, const void *in, int64_t n)
{
	if (!ctx || n < 0 || (!in && n > 0)) return EDISON_E_ARGUMENT;
	if (!ctx->fnet) return ed_set_err(ctx, EDISON_E_NO_MODEL, "no float network loaded (edison_fnet_load)");
	return EDISON_OK;
}

static int run_on(edison_ctx *ctx, const float *in, int64_t n, float *logits, float *probs, int32_t *argmax, float *acts)
{
	if (n == 0) return EDISON_OK;
	ED_HIP(ctx, hipSetDevice(ctx->device));
	if (ctx->fnet->layered) return run_layered(ctx, in, n, logits, probs, argmax, acts, NULL);
	const int e = ed_launch_fnet(&ctx->fnet->plan, in, ctx->fnet->plan.in_n, n, logits, probs, argmax, acts, ctx->stream);
	return ed_launch_result(ctx, e, "float network kernel");
}

extern "C" int edison_fnet_batch_dev(edison_ctx *ctx, const float *in, int64_t n, float *logits, float *probs, int32_t *argmax)
{
	{ const int r = need_net(ctx, in, n); if (r != EDISON_OK) return r; }
	return run_on(ctx, in, n, logits, probs, argmax, NULL);
}

extern "C" int edison_fnet_profile_dev(edison_ctx *ctx, const float *in, int64_t n, float *ms)
{
	{ const int r = need_net(ctx, in, n); if (r != EDISON_OK) return r; }
	if (!ms) return EDISON_E_ARGUMENT;
	if (!ctx->fnet->layered) return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_fnet_profile_dev: the loaded float network is not a layered one");
	if (n == 0) return EDISON_OK;
	ED_HIP(ctx, hipSetDevice(ctx->device));
	return run_layered(ctx, in, n, NULL, NULL, NULL, NULL, ms);
}

extern "C" int edison_fnet_layers_dev(edison_ctx *ctx, const float *in, int64_t n, float *acts)
{
	{ const int r = need_net(ctx, in, n); if (r != EDISON_OK) return r; }
	if (!acts && n > 0) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_fnet_layers: acts is NULL");
	return run_on(ctx, in, n, NULL, NULL, NULL, acts);
}

extern "C" int edison_fnet_batch(edison_ctx *ctx, const float *in, int64_t n, float *logits, float *probs, int32_t *argmax)
{
	{ const int r = need_net(ctx, in, n); if (r != EDISON_OK) return r; }
	if (n == 0) return EDISON_OK;
	const ed_fnet_plan_t &p = ctx->fnet->plan;
	ed_staging st(ctx);
	const float *x = st.in(in, (size_t)n * p.in_n);
	float *l = st.out(logits, (size_t)n * p.n_out), *s = st.out(probs, (size_t)n * p.n_out);
	int32_t *a = st.out(argmax, (size_t)n);
	return st.finish(st.ok() ? edison_fnet_batch_dev(ctx, x, n, l, s, a) : EDISON_OK);
}

extern "C" int edison_fnet_layers(edison_ctx *ctx, const float *in, int64_t n, float *acts)
{
	{ const int r = need_net(ctx, in, n); if (r != EDISON_OK) return r; }
	if (n == 0) return EDISON_OK;
	if (!acts) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_fnet_layers: acts is NULL");
	const ed_fnet_plan_t &p = ctx->fnet->plan;
	ed_staging st(ctx);
	const float *x = st.in(in, (size_t)n * p.in_n);
	float *a = st.out(acts, (size_t)n * p.acts_n);
	return st.finish(st.ok() ? edison_fnet_layers_dev(ctx, x, n, a) : EDISON_OK);
}

/* ---- audio -> class with the float network (edison_kws_float_batch*) ---------------------------------------------------------- */
/* everything of kws_float_check that does not need the loaded network: the arguments, the flow and the geometry (*frames = frames per utterance) */
static int kws_float_geom(edison_ctx *ctx, const edison_kws_geom *g, int q15, float lo, float hi, const int16_t *audio, int64_t n_utt,
                          int64_t utt_stride, int *frames)
{
	if (!ctx || !g || n_utt < 0 || (!audio && n_utt > 0) || (q15 != 0 && q15 != 1)) return EDISON_E_ARGUMENT;
	if (utt_stride < 0) return ed_set_err(ctx, EDISON_E_ARGUMENT, "negative utterance stride");
	if (!(lo <= hi)) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_kws_float: clip_lo > clip_hi");
	if (q15)
	{
		/* the firmware's variant C: 1024-sample frames and hops, the context's 32-band filterbank, DCT rows 0 .. num_mfcc - 1 */
		if (g->frame_len != EDISON_FRAME_LEN || g->frame_step != EDISON_FRAME_LEN || g->mel_nbins != EDISON_NUM_MEL || g->first_mfcc != 0 ||
		    g->num_mfcc < 1 || g->num_mfcc > EDISON_NUM_MEL)
			return ed_set_err(ctx, EDISON_E_NO_IMPL, "edison_kws_float: q15 = 1 takes the shipped geometry only (1024 / 1024, 32 mel bins, first_mfcc 0)");
		if (g->n_samples < g->frame_len || g->frame_count < 0) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_kws_float: bad n_samples / frame_count");
		const int64_t F = g->frame_count ? g->frame_count : 1 + (g->n_samples - g->frame_len) / g->frame_step;
		if ((F - 1) * (int64_t)g->frame_step + g->frame_len > g->n_samples)
			return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_kws_float: frame_count frames do not fit in n_samples");
		*frames = (int)F;
	}
	else
	{
		const int r = ed_kws_geom_check(ctx, g, frames);
		if (r != EDISON_OK) return r;
	}
	return EDISON_OK;
}

static int kws_float_check(edison_ctx *ctx, const edison_kws_geom *g, int q15, float lo, float hi, const int16_t *audio, int64_t n_utt,
                           int64_t utt_stride, int *frames)
{
	{ const int r = kws_float_geom(ctx, g, q15, lo, hi, audio, n_utt, utt_stride, frames); if (r != EDISON_OK) return r; }
	if (!ctx->fnet) return ed_set_err(ctx, EDISON_E_NO_MODEL, "no float network loaded (edison_fnet_load)");
	const int64_t n_feat = (int64_t)*frames * g->num_mfcc;
	if (n_feat != ctx->fnet->plan.in_n)
	{
		snprintf(ctx->err, sizeof(ctx->err), "edison_kws_float: frame_count x num_mfcc = %lld features, the float network's input = %d",
		         (long long)n_feat, ctx->fnet->plan.in_n);
		return EDISON_E_SIZE;
	}
	if (n_utt * (int64_t)*frames >= ((int64_t)1 << 31)) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_kws_float: more than 2^31 frames in one call");
	return EDISON_OK;
}

int ed_kws_float_geom_check(edison_ctx *ctx, const edison_kws_geom *g, int q15, float clip_lo, float clip_hi, int *frames)
{
	return kws_float_check(ctx, g, q15, clip_lo, clip_hi, NULL, 0, 0, frames);
}

/* The feature launches of edison_kws_float_batch*: n_utt utterances (F frames each, checked) -> in_n = F x num_mfcc floats a row in feat, or in
 * the context's scratch when feat is NULL; *out = where they are. */
static int kws_float_features(edison_ctx *ctx, const edison_kws_geom *g, int q15, float clip_lo, float clip_hi, const int16_t *audio, int64_t n_utt,
                              int64_t utt_stride, int F, int in_n, float *feat, float **out)
{
	ED_HIP(ctx, hipSetDevice(ctx->device));
	const size_t n_feat = (size_t)n_utt * (size_t)in_n;
	/* scratch: [the float64 MFCC (host flow)] then [the float features when the caller passes none] */
	const size_t y_bytes = q15 ? 0 : sizeof(double) * n_feat, f_bytes = feat ? 0 : sizeof(float) * n_feat;
	if (y_bytes + f_bytes)
	{
		const int r = ed_ctx_ensure_scratch(ctx, y_bytes + f_bytes);
		if (r != EDISON_OK) return r;
	}
	float *const f = feat ? feat : (float *)((char *)ctx->scratch + y_bytes);
	if (q15)
	{
		/* variant C int16 -> (float), no scale, no clip (app.c:675-683): the Q15 kernel's float output */
		const int r = ed_ctx_mfcc_q15_launch(ctx, audio, n_utt * F, F, utt_stride, g->frame_step, g->num_mfcc, NULL, f, NULL, 0, NULL, NULL, NULL);
		if (r != EDISON_OK) return r;
	}
	else
	{
		double *y = (double *)ctx->scratch;
		const int r = edison_mfcc_geom_batch_dev(ctx, g, audio, n_utt, utt_stride, y);
		if (r != EDISON_OK) return r;
		const int e = ed_launch_fnet_input(y, (int64_t)n_feat, (float)g->net_input_scale, clip_lo, clip_hi, f, ctx->n_cu, ctx->stream);
		if (e != 0) return ed_launch_result(ctx, e, "float network input");
	}
	*out = f;
	return EDISON_OK;
}

/* edison_ftrain.hip's edison_ftrain_data_audio: kws_float's checks without the loaded network, then its feature launches into feat [n_utt][in_n] */
int ed_kws_float_features_dev(edison_ctx *ctx, const edison_kws_geom *g, int q15, float clip_lo, float clip_hi, const int16_t *audio, int64_t n_utt,
                              int64_t utt_stride, int in_n, float *feat, int *frames)
{
	int F = 0;
	{ const int r = kws_float_geom(ctx, g, q15, clip_lo, clip_hi, audio, n_utt, utt_stride, &F); if (r != EDISON_OK) return r; }
	if (frames) *frames = F;
	if ((int64_t)F * g->num_mfcc != in_n)
	{
		snprintf(ctx->err, sizeof(ctx->err), "edison_ftrain_data_audio: frame_count x num_mfcc = %lld features, the data set's rows have %d",
		         (long long)F * g->num_mfcc, in_n);
		return EDISON_E_SIZE;
	}
	if (n_utt * (int64_t)F >= ((int64_t)1 << 31)) return ed_set_err(ctx, EDISON_E_ARGUMENT, "edison_kws_float: more than 2^31 frames in one call");
	if (n_utt == 0 || !feat) return EDISON_OK;
	float *f = NULL;
	return kws_float_features(ctx, g, q15, clip_lo, clip_hi, audio, n_utt, utt_stride, F, in_n, feat, &f);
}

extern "C" int edison_kws_float_batch_dev(edison_ctx *ctx, const edison_kws_geom *g, int q15, float clip_lo, float clip_hi, const int16_t *audio,
                                          int64_t n_utt, int64_t utt_stride, float *feat, float *logits, float *probs, int32_t *argmax)
{
	int F = 0;
	{ const int r = kws_float_check(ctx, g, q15, clip_lo, clip_hi, audio, n_utt, utt_stride, &F); if (r != EDISON_OK) return r; }
	if (n_utt == 0) return EDISON_OK;
	float *f = NULL;
	{ const int r = kws_float_features(ctx, g, q15, clip_lo, clip_hi, audio, n_utt, utt_stride, F, ctx->fnet->plan.in_n, feat, &f); if (r != EDISON_OK) return r; }
	return run_on(ctx, f, n_utt, logits, probs, argmax, NULL);
}

extern "C" int edison_kws_float_batch(edison_ctx *ctx, const edison_kws_geom *g, int q15, float clip_lo, float clip_hi, const int16_t *audio,
                                      int64_t n_utt, int64_t utt_stride, float *feat, float *logits, float *probs, int32_t *argmax)
{
	int F = 0;
	{ const int r = kws_float_check(ctx, g, q15, clip_lo, clip_hi, audio, n_utt, utt_stride, &F); if (r != EDISON_OK) return r; }
	if (n_utt == 0) return EDISON_OK;
	const unsigned __int128 na128 = (unsigned __int128)(n_utt - 1) * (unsigned __int128)utt_stride +
	                                (unsigned __int128)((int64_t)(F - 1) * g->frame_step + g->frame_len);
	if (na128 * sizeof(int16_t) > ((unsigned __int128)1 << 47)) return ed_set_err(ctx, EDISON_E_SIZE, "edison_kws_float_batch: utt_stride x n_utt too large");
	const size_t n = (size_t)n_utt, in_n = (size_t)ctx->fnet->plan.in_n, n_out = (size_t)ctx->fnet->plan.n_out;
	ed_staging st(ctx);
	const int16_t *au = st.in(audio, (size_t)na128);
	float *f = st.scratch(feat, n * in_n), *l = st.out(logits, n * n_out), *s = st.out(probs, n * n_out);
	int32_t *am = st.out(argmax, n);
	return st.finish(st.ok() ? edison_kws_float_batch_dev(ctx, g, q15, clip_lo, clip_hi, au, n_utt, utt_stride, f, l, s, am) : EDISON_OK);
}
