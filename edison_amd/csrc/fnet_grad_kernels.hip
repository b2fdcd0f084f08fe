/*
 * fnet_grad_kernels.hip -- training the loaded float32 network (edison_ftrain.hip, edison_amd/train.py): the
 * gradient of the batch-mean cross entropy with respect to every weight and bias, and the optimiser step. ed_ftrain_grad_kernel<PADS, DROP>:
 * PADS = false is the kernel of a plan without padded records; true also holds the padded path of the forward tile
 * and of the dW gather, taken by the records that have pad; dX reads the inverse origin table only and is the same for both. DROP = true
 * is a training call on a trainer with dropout: the mask of fnet_dropout.h in the forward epilogue and again
 * where dY is built; every other call runs DROP = false, whose instructions are those of the kernel before dropout existed.
 *
 * ed_ftrain_grad_kernel. A fixed grid of workgroups; workgroup g takes the tiles of utterances g, g + grid, g + 2 grid, ... in that
 * order, each through a forward half and a backward half, and adds what the tile gives into its own gradient slab (the first tile
 * stores, so a slab needs no zeroing; its padding entries are never written and stay the +0.0f they were allocated with).
 * ed_ftrain_reduce_kernel then sums the slabs in index order. No float atomic anywhere: every slab element has one owner lane, and
 * the order of every sum is fixed by (n, batch, grid), so a call repeated gives the same bits.
 *
 *   forward   ed_fnet_kernel's own LDS plan and layer walk (fnet_device.h: EDF_LDS_PLAN, EDF_LAYER_WALK) over the work item edg_tile:
 *             edf_tile's k-ordered MFMA loop and epilogue order, so the logits are edison_fnet_batch's bit for bit, with an epilogue
 *             specialised by P that also writes every pooled output to the workgroup's activation store in global memory (the A
 *             operand of dW) and beside it one mask byte: which element of the pool window was the first maximum, and whether its
 *             gradient passes (no ReLU, or a pre-activation > 0). The shared tile with these stores in a sink was measured 3 to 6 %
 *             slower, so this one copy of the tile stays.
 *   loss      one thread per utterance on the network's EDF_SOFTMAX: loss = log sum exp(z - max) + max - z[y], dz = (softmax(z) - onehot(y)) / n.
 *   backward  per record, last to first, with LDS reused (the forward half is done with it):
 *     dY   [rows of the tile][n_pad] in LDS, from the gradient of the pooled outputs and the mask bytes: the window's winner gets it,
 *          every other element, every padding channel and every row beyond the tile is +0.0f. No second comparison.
 *     dW   [k][c] = sum_r A[r][k] dY[r][c]: 16 k x 16 c tiles on v_mfma_f32_16x16x4_f32, four rows r per instruction in ascending
 *          order; A is gathered through the plan's own rowin / koff. One more tile row with A = 1 gives the bias gradient.
 *     dX   of the record's input (not for record 0) in gather form: [position][ci] = sum_t sum_c dY[inv[position][t]][c] W[t in_c + ci][c]
 *          on the same instruction, through the inverse origin table of fnet_train.h; a position nothing reads gets +0.0f.
 *
 * ed_ftrain_step_kernel: Adam as Keras states it, or plain SGD, elementwise over the packed array.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edison_launch.h"
#include "fnet.h"
#include "fnet_device.h"
#include "fnet_dropout.h"
#include "fnet_grad_device.h"
#include "fnet_train.h"

/* edf_tile (fnet_device.h) with the training epilogue: the MFMA loop and the order bias, ReLU, pool are edf_tile's; every pooled output
 * also goes to acts (this workgroup's store, utterance-major) with its mask byte. PAD = true takes edf_tile<NT, true>'s three
 * differences: edf_pad_row, edf_pad_tap on the kyx behind koff, and edf_pad_live, an absent row being -inf before the window's max. */
/* What the training epilogue stores beside dst: the workgroup's activation store and mask bytes; with DROP (a training call on a trainer
 * with dropout) also the record's threshold T, scale s and position, and its keys of the tile's utterances:
 * utterance u's (kA, kB) at keys[2 u key_n]. */
template <bool DROP>
struct edg_stores;
template <>
struct edg_stores<false>
{
	float *__restrict__ acts;
	uint8_t *__restrict__ mask;
	int acts_n;
};
template <>
struct edg_stores<true>
{
	float *__restrict__ acts;
	uint8_t *__restrict__ mask;
	int acts_n;
	const uint32_t *__restrict__ keys;
	int key_n;
	uint32_t T;
	float s;
	bool before;
};

/* DROP: the mask of fnet_dropout.h in the epilogue. Before the pool (and P > 1) every present element after bias and ReLU becomes
 * keep ? v s : +0.0f, then the max and the first-maximum chain run as without; after the pool, or P = 1, the pooled x does. The stored
 * value is the dropped one; EDFT_DROPPED in the mask byte says the window's winner, or the pooled output, was dropped. T = 0 (rate 0)
 * skips the hash. */
template <int NT, bool PAD, bool DROP>
__device__ __forceinline__ void edg_tile(const ed_fnet_layer_t &L, const float *__restrict__ src, int src_n, float *__restrict__ dst, int dst_n,
                                         const float *__restrict__ wl, const int32_t *__restrict__ kl, const int32_t *__restrict__ rowin,
                                         const float *__restrict__ bias, int M, int mt, int n0, int lane, float *__restrict__ acts,
                                         uint8_t *__restrict__ mask, int acts_n, [[maybe_unused]] const edg_stores<DROP> &st)
{
	const int r = lane & 15, kq = lane >> 4;
	const int m = mt * 16 + r;
	int base = 0;
	[[maybe_unused]] int y0 = 0, x0 = 0;
	if constexpr (PAD) edf_pad_row(L, rowin, src_n, M, m, base, y0, x0);
	else if (m < M)
	{
		const int u = m / L.rows;
		base = u * src_n + rowin[m - u * L.rows];
	}
	ed_f4 acc[NT];
#pragma unroll
	for (int j = 0; j < NT; j++) acc[j] = (ed_f4){0.0f, 0.0f, 0.0f, 0.0f};
	const float *wp = wl + kq * L.n_pad + n0 + r;
#pragma unroll 4
	for (int k0 = 0; k0 < L.k_pad; k0 += 4)
	{
		const int ko = kl[k0 + kq];
		float a;
		if constexpr (PAD) a = edf_pad_tap(L, src, base, y0, x0, ko, kl[L.k_pad + k0 + kq]);
		else a = ko >= 0 ? src[base + ko] : 0.0f;
#pragma unroll
		for (int j = 0; j < NT; j++) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wp[j * 16], acc[j], 0, 0, 0);
		wp += 4 * L.n_pad;
	}
	/* D: lane holds rows 4 kq + i (i = 0..3) of channel n0 + 16 j + r */
	const int P = L.P;
	const int m0 = mt * 16 + 4 * kq;
	[[maybe_unused]] bool live[4];
	if constexpr (PAD) edf_pad_live(L, rowin, M, m0, live);
#pragma unroll
	for (int j = 0; j < NT; j++)
	{
		const int n = n0 + 16 * j + r;
		if (n >= L.out_c) continue;
		const float b = bias[n];
		float v[4];
#pragma unroll
		for (int i = 0; i < 4; i++)
		{
			v[i] = acc[j][i] + b;
			if (L.relu) v[i] = fmaxf(v[i], 0.0f);
			if constexpr (PAD) { if (!live[i]) v[i] = -INFINITY; } /* absent: the max's identity; its window has a real element */
		}
		[[maybe_unused]] bool kept[4] = {true, true, true, true};
		if constexpr (DROP)
		{
			if (st.T != 0 && st.before && P > 1)
			{
#pragma unroll
				for (int i = 0; i < 4; i++)
				{
					const int mi = m0 + i;
					bool real = mi < M;
					if constexpr (PAD) real = live[i];
					if (!real) continue; /* absent stays -inf; a row beyond M is not emitted */
					const int u = mi / L.rows, row = mi - u * L.rows;
					const uint32_t *k = st.keys + 2 * u * st.key_n;
					kept[i] = edd_hash((uint32_t)(row * L.out_c + n), k[0], k[1]) >= st.T;
					v[i] = kept[i] ? v[i] * st.s : 0.0f;
				}
			}
		}
		/* one pooled output: the window's maximum x at rows mg .., its first maximum e in element order; under ReLU a maximum of 0 is a
		 * pre-activation <= 0 and passes nothing. A padded record's absent elements are -inf and x is a present element's finite value
		 * (a pad is smaller than its window), so the v[g] == x chains below pick the first maximum among the present elements. */
		auto emit = [&](int mg, float x, int e, [[maybe_unused]] bool winner_kept) {
			if (mg >= M) return;
			int pass = !L.relu || x > 0.0f ? EDFT_PASS : 0;
			const int u = mg / L.rows, q = (mg - u * L.rows) / P;
			if constexpr (DROP)
			{
				if (st.T != 0)
				{
					if (!st.before || P == 1)
					{
						const uint32_t *k = st.keys + 2 * u * st.key_n;
						winner_kept = edd_hash((uint32_t)(q * L.out_c + n), k[0], k[1]) >= st.T;
						x = winner_kept ? x * st.s : 0.0f;
					}
					if (!winner_kept) pass |= EDFT_DROPPED;
				}
			}
			dst[u * dst_n + q * L.out_c + n] = x;
			const int o = u * acts_n + L.acts_at + q * L.out_c + n;
			acts[o] = x;
			mask[o] = (uint8_t)(e | pass);
		};
		if (P == 1)
		{
#pragma unroll
			for (int i = 0; i < 4; i++) emit(m0 + i, v[i], 0, true);
		}
		else if (P == 2)
		{
#pragma unroll
			for (int g = 0; g < 4; g += 2)
			{
				const float x = fmaxf(v[g], v[g + 1]);
				const int e = v[g] == x ? 0 : 1;
				emit(m0 + g, x, e, e ? kept[g + 1] : kept[g]);
			}
		}
		else
		{
			const float x = fmaxf(fmaxf(fmaxf(v[0], v[1]), v[2]), v[3]);
			const int e = v[0] == x ? 0 : v[1] == x ? 1 : v[2] == x ? 2 : 3;
			emit(m0, x, e, e == 0 ? kept[0] : e == 1 ? kept[1] : e == 2 ? kept[2] : kept[3]);
		}
	}
}

/* The walk's work item for training (EDF_LAYER_WALK of fnet_device.h): edg_tile by the item's nt <= 4 channel tiles. */
template <bool PAD, bool DROP>
__device__ __forceinline__ void edg_item(int nt, const ed_fnet_layer_t &L, const float *__restrict__ src, int src_n, float *__restrict__ dst, int dst_n,
                                         const float *__restrict__ wl, const int32_t *__restrict__ kl, const int32_t *__restrict__ rowin,
                                         const float *__restrict__ bias, int M, int mt, int n0, int lane, float *, int64_t, int64_t, const edg_stores<DROP> &st)
{
	if (nt == 4) edg_tile<4, PAD, DROP>(L, src, src_n, dst, dst_n, wl, kl, rowin, bias, M, mt, n0, lane, st.acts, st.mask, st.acts_n, st);
	else if (nt == 3) edg_tile<3, PAD, DROP>(L, src, src_n, dst, dst_n, wl, kl, rowin, bias, M, mt, n0, lane, st.acts, st.mask, st.acts_n, st);
	else if (nt == 2) edg_tile<2, PAD, DROP>(L, src, src_n, dst, dst_n, wl, kl, rowin, bias, M, mt, n0, lane, st.acts, st.mask, st.acts_n, st);
	else edg_tile<1, PAD, DROP>(L, src, src_n, dst, dst_n, wl, kl, rowin, bias, M, mt, n0, lane, st.acts, st.mask, st.acts_n, st);
}

/* DROP: a training call on a trainer with dropout. seed and call are read by that instantiation only. */
template <bool PADS, bool DROP>
__global__ __launch_bounds__(ED_FNET_THREADS) void ed_ftrain_grad_kernel(const ed_ftrain_plan_t *tp, const float *__restrict__ in,
                                                                           const int32_t *__restrict__ labels, int64_t n, float *__restrict__ loss,
                                                                           int32_t *__restrict__ argmax, float *__restrict__ logits,
                                                                           unsigned long long *__restrict__ ignored, uint64_t seed, uint64_t call)
{
	const ed_ftrain_plan_t &t = *tp; /* in device memory, read where it is used: by value its fields stay live in SGPRs and spill */
	const ed_fnet_plan_t &p = t.net;
	EDF_LDS_PLAN /* the forward half: ed_fnet_kernel's plan */
	/* backward half, over it */
	float *dy = lds;
	int32_t *rb = (int32_t *)(lds + t.dy_lds);
	const int acts_n = p.acts_n;
	float *slab = t.slabs + (int64_t)blockIdx.x * t.w_floats;
	float *acts = t.acts + (int64_t)blockIdx.x * B * acts_n;
	float *dacts = t.dacts + (int64_t)blockIdx.x * B * acts_n;
	uint8_t *mask = t.mask + (int64_t)blockIdx.x * B * acts_n;
	[[maybe_unused]] uint32_t *keys = NULL;
	if constexpr (DROP) keys = t.keys + (int64_t)blockIdx.x * B * p.n_layers * 2;
	const int64_t n_tiles = (n + B - 1) / B;
	bool first = true;

	for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x, first = false)
	{
		const int64_t u0 = tile * B;
		const int nu = (int)(n - u0 < B ? n - u0 : B);
		const float *x0 = in + u0 * (int64_t)p.in_n;
		__syncthreads(); /* the previous tile's backward half no longer reads the LDS */
		for (int i = tid; i < nu * p.in_n; i += ED_FNET_THREADS)
		{
			const int u = i / p.in_n, e = i - u * p.in_n;
			buf[0][u * p.buf_n[0] + e] = x0[i];
		}

		/* the dropout keys of (utterance of the tile, record): Philox once each, read by every element's hash after the walk's first sync */
		if constexpr (DROP)
			for (int i = tid; i < nu * p.n_layers; i += ED_FNET_THREADS)
			{
				const int u = i / p.n_layers;
				edd_keys(seed, call, (uint32_t)(u0 + u), (uint32_t)(i - u * p.n_layers), keys + 2 * i, keys + 2 * i + 1);
			}

		/* ---- forward: the network's own walk over edg_tile (PADS = false: the launcher starts it for plans without padded records) ---- */
		if constexpr (DROP)
		{
			for (int l = 0; l < p.n_layers; l++)
			{
				const edg_stores<true> stores = {acts, mask, acts_n, keys + 2 * l, p.n_layers, t.drop_T[l], t.drop_s[l], t.drop_before[l] != 0};
				EDF_LAYER_WALK(PADS, edg_item, p.L[l], (float *)NULL, 0, 0, stores)
			}
		}
		else
		{
			const edg_stores<false> stores = {acts, mask, acts_n};
			for (int l = 0; l < p.n_layers; l++) EDF_LAYER_WALK(PADS, edg_item, p.L[l], (float *)NULL, 0, 0, stores)
		}
		__syncthreads();

		/* ---- loss and dL/dz, one thread per utterance (the softmax and the argmax are ed_fnet_kernel's) ---- */
		if (tid < nu)
		{
			const ed_fnet_layer_t &L = p.L[p.n_layers - 1];
			const float *z = buf[L.dst] + tid * p.buf_n[L.dst];
			float *dz = dacts + tid * acts_n + L.acts_at;
			const int64_t u = u0 + tid;
			const int y = labels[u];
			const bool labelled = (unsigned)y < (unsigned)p.n_out;
			const float nf = (float)n;
			EDF_SOFTMAX(z, p.n_out, logits[u * p.n_out + j] = z[j]; dz[j] = labelled ? (pj - (j == y ? 1.0f : 0.0f)) / nf : 0.0f;)
			if (argmax) argmax[u] = best;
			if (loss) loss[u] = labelled ? logf(s) + mx - z[y] : 0.0f;
			if (!labelled) atomicAdd(ignored, 1ull);
		}

		/* ---- backward ---- */
		for (int l = p.n_layers - 1; l >= 0; l--)
		{
			const ed_fnet_layer_t &L = p.L[l];
			const ed_ftrain_layer_t &G = t.G[l];
			const int M = nu * L.rows, Mp = (M + 15) & ~15;
			const int src_n = l ? acts_n : p.in_n;
			const float *src = l ? acts + p.L[l - 1].acts_at : x0;
			const int32_t *rowin = p.tab + L.rowin_at;
			[[maybe_unused]] float ds = 1.0f;
			if constexpr (DROP) ds = t.drop_s[l];
			__syncthreads(); /* dz, or the next record's dX, is written; its dY no longer read */
			for (int i = tid; i < Mp * L.n_pad; i += ED_FNET_THREADS)
			{
				const int m = i / L.n_pad, c = i - m * L.n_pad;
				float v = 0.0f;
				if (m < M && c < L.out_c)
				{
					const int u = m / L.rows, r = m - u * L.rows, q = r / L.P, e = r - q * L.P;
					const int o = u * acts_n + L.acts_at + q * L.out_c + c;
					const int mk = mask[o];
					if constexpr (DROP)
					{
						if ((mk & (EDFT_PASS | EDFT_DROPPED)) == EDFT_PASS && (mk & EDFT_WIN_MASK) == e) v = dacts[o] * ds;
					}
					else if ((mk & EDFT_PASS) && (mk & EDFT_WIN_MASK) == e) v = dacts[o];
				}
				dy[i] = v;
			}
			const bool padded = PADS && L.pad;
			for (int m = tid; m < Mp; m += ED_FNET_THREADS)
			{
				const int u = m / L.rows;
				if (padded)
				{
					rb[2 * m] = m < M ? u * src_n : 0;
					rb[2 * m + 1] = m < M ? rowin[m - u * L.rows] : -1;
				}
				else rb[m] = m < M ? u * src_n + rowin[m - u * L.rows] : 0;
			}
			__syncthreads();
			{
				const int KT = (G.K + 15) / 16, NT = L.n_pad / 16, NG = (NT + 3) / 4;
				const int32_t *koff = p.tab + L.koff_at;
				for (int item = wave; item < (KT + 1) * NG; item += n_waves)
				{
					const int kt = item / NG, g = item - kt * NG;
					const int n0 = g * 64, nt = NT - 4 * g < 4 ? NT - 4 * g : 4;
					if (padded)
					{
						if constexpr (PADS)
						{
							if (nt == 4) edg_dw_tile<4, true>(L, G.K, src, koff, dy, rb, M, kt, KT, n0, lane, slab, first);
							else if (nt == 3) edg_dw_tile<3, true>(L, G.K, src, koff, dy, rb, M, kt, KT, n0, lane, slab, first);
							else if (nt == 2) edg_dw_tile<2, true>(L, G.K, src, koff, dy, rb, M, kt, KT, n0, lane, slab, first);
							else edg_dw_tile<1, true>(L, G.K, src, koff, dy, rb, M, kt, KT, n0, lane, slab, first);
						}
					}
					else if (nt == 4) edg_dw_tile<4, false>(L, G.K, src, koff, dy, rb, M, kt, KT, n0, lane, slab, first);
					else if (nt == 3) edg_dw_tile<3, false>(L, G.K, src, koff, dy, rb, M, kt, KT, n0, lane, slab, first);
					else if (nt == 2) edg_dw_tile<2, false>(L, G.K, src, koff, dy, rb, M, kt, KT, n0, lane, slab, first);
					else edg_dw_tile<1, false>(L, G.K, src, koff, dy, rb, M, kt, KT, n0, lane, slab, first);
				}
			}
			if (l)
			{
				const int MX = nu * G.np, MT = (MX + 15) / 16, CT = (L.in_c + 15) / 16;
				for (int item = wave; item < MT * CT; item += n_waves)
				{
					const int mt = item / CT, ct = item - mt * CT;
					edg_dx_tile(L, G, t.inv + G.inv_at, p.w + L.w_at, dy, MX, mt, ct * 16, lane, dacts + p.L[l - 1].acts_at, acts_n);
				}
			}
		}
	}
}

/* grad[i] = slab 0's [i] + slab 1's [i] + ... in that order */
__global__ __launch_bounds__(256) void ed_ftrain_reduce_kernel(const float *__restrict__ slabs, int n_slabs, int64_t w_floats, float *__restrict__ grad)
{
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= w_floats) return;
	float s = slabs[i];
	for (int g = 1; g < n_slabs; g++) s += slabs[g * w_floats + i];
	grad[i] = s;
}

__global__ __launch_bounds__(256) void ed_ftrain_step_kernel(int kind, float *__restrict__ w, const float *__restrict__ g, float *__restrict__ m,
                                                              float *__restrict__ v, int64_t count, float factor, float b1, float omb1, float b2,
                                                              float omb2, float eps)
{
	const int64_t stride = (int64_t)gridDim.x * 256;
	for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += stride)
	{
		const float gi = g[i];
		if (kind == EDFT_SGD)
		{
			w[i] -= factor * gi;
			continue;
		}
		const float mi = b1 * m[i] + omb1 * gi;
		const float vi = b2 * v[i] + omb2 * gi * gi;
		m[i] = mi;
		v[i] = vi;
		w[i] -= factor * mi / (sqrtf(vi) + eps);
	}
}

extern "C" int ed_launch_ftrain_grad(const ed_ftrain_plan_t *t, const ed_ftrain_plan_t *d_plan, const float *in, const int32_t *labels, int64_t n, float *loss, int32_t *argmax,
                                     float *logits, float *grad, unsigned long long *ignored, int grid, int drop, uint64_t seed, uint64_t call, hipStream_t stream)
{
	if (n <= 0) return 0;
	const ed_fnet_plan_t *p = &t->net;
	const size_t lds = ed_ftrain_lds_bytes(t);
	if (!ed_fnet_plan_launchable(p, lds) || grid < 1) return (int)hipErrorInvalidValue;
	bool pads = false; /* a plan with a padded record runs the instantiation that holds the padded path, any other plan the one without */
	for (int l = 0; l < p->n_layers; l++) pads = pads || p->L[l].pad;
	/* drop: a training call with a non-zero rate; every other call runs the instantiations without the mask */
	if (drop && (n > 0xffffffffll || !t->keys)) return (int)hipErrorInvalidValue;
	const auto kernel = drop ? (pads ? ed_ftrain_grad_kernel<true, true> : ed_ftrain_grad_kernel<false, true>)
	                         : (pads ? ed_ftrain_grad_kernel<true, false> : ed_ftrain_grad_kernel<false, false>);
	{ const int e = ed_kernel_prepare((const void *)kernel, ED_FNET_THREADS, lds, NULL, NULL); if (e) return e; }
	const int64_t n_tiles = (n + p->batch - 1) / p->batch;
	const int used = (int)(n_tiles < grid ? n_tiles : grid); /* a workgroup without a tile would leave its slab stale */
	hipLaunchKernelGGL(kernel, dim3((unsigned)used), dim3(ED_FNET_THREADS), lds, stream, d_plan, in, labels, n, loss, argmax, logits, ignored, seed, call);
	{ const int e = (int)hipGetLastError(); if (e) return e; }
	hipLaunchKernelGGL(ed_ftrain_reduce_kernel, dim3((unsigned)((t->w_floats + 255) / 256)), dim3(256), 0, stream, t->slabs, used, t->w_floats, grad);
	return (int)hipGetLastError();
}

extern "C" int ed_launch_ftrain_step(int kind, float *w, const float *g, float *m, float *v, int64_t count, float factor, float b1, float omb1, float b2,
                                     float omb2, float eps, int n_cu, hipStream_t stream)
{
	if (count <= 0) return 0;
	int64_t blocks = (count + 255) / 256;
	const int64_t cap = (int64_t)(n_cu > 0 ? n_cu : 1) * 8;
	if (blocks > cap) blocks = cap;
	hipLaunchKernelGGL(ed_ftrain_step_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, kind, w, g, m, v, count, factor, b1, omb1, b2, omb2, eps);
	return (int)hipGetLastError();
}
