/*
 * fnet_bn_kernels.hip -- a training call of the float32 trainer with BatchNorm (edison_ftrain_set_batchnorm, edison_ftrain.hip;
 * DESIGN.md section 19c). Batch statistics couple every sample of the call, in the forward pass and again in the backward pass, so the
 * call is not one persistent launch as ed_ftrain_grad_kernel is: every batch-wide dependency is a kernel boundary on the stream, and no
 * kernel waits for another workgroup. The launches of a call, their number fixed by the records and not by n:
 *
 *   edb_keys_kernel     (a call with dropout) the Philox keys of fnet_dropout.h per (sample, record)
 *   per record, first to last:
 *     edb_conv_kernel   workgroup g takes the tiles g, g + grid, ... of `batch` utterances: z = conv + bias over the whole conv map on
 *                       v_mfma_f32_16x16x4_f32 (edf_tile's tiling and k order, operands read through global pointers, float32 chains
 *                       of 16 k summed in double: edb_conv_tile), stored to zs; then, for a BatchNorm record, the moments of its own
 *                       rows per channel: count, mean, and M2 from values centred on that mean
 *     edb_stats_kernel  (BatchNorm records) one workgroup, one thread a channel: Chan's merge of the workgroups' moments in index order
 *                       -> mean, variance, rstd; the moving statistics. The only writer of all of them
 *     edb_apply_kernel  per pooled output: normalise, ReLU, dropout, the pool's first maximum -> outs and the mask byte
 *   edb_loss_kernel     per sample the network's EDF_SOFTMAX: logits, loss, argmax, dL/dz
 *   per record, last to first:
 *     edb_dysum_kernel / edb_dyreduce_kernel  (BatchNorm records) partial sums of dy and dy zhat per workgroup, then in index order
 *     edb_back_kernel   per tile dZ [rows][n_pad] in LDS (dz of DESIGN.md section 19c from dy, or dy itself), then edg_dw_tile into
 *                       the workgroup's slab and edg_dx_tile into the previous record's douts: the trainer's own two work items
 *   edb_reduce_kernel   the slabs in index order; the bias gradient of a BatchNorm record +0.0f
 *
 * Determinism: no float atomic; a workgroup's tiles, a thread's rows and every merge have an order fixed by (n, batch, grid). The
 * statistics and the sums of dy are accumulated in double: they are elementwise passes over z, far from any limit of the FP64 pipe.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edison_launch.h"
#include "fnet.h"
#include "fnet_bn.h"
#include "fnet_device.h"
#include "fnet_dropout.h"
#include "fnet_grad_device.h"
#include "fnet_train.h"

#define EDB_THREADS ED_FNET_THREADS

__global__ __launch_bounds__(256) void edb_keys_kernel(int64_t n, int n_layers, uint64_t seed, uint64_t call, uint32_t *__restrict__ keys)
{
	const int64_t stride = (int64_t)gridDim.x * 256;
	for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n * n_layers; i += stride)
	{
		const int64_t u = i / n_layers;
		edd_keys(seed, call, (uint32_t)u, (uint32_t)(i - u * n_layers), keys + 2 * i, keys + 2 * i + 1);
	}
}

/* The sum over the workgroup's rows of f(row of the call, channel) for each channel of the record, in double: thread (s, c) takes the
 * rows s, s + S, ... of every tile the workgroup owns in tile order, then thread (0, c) adds the S slices in index order. Result in
 * tot[c - c0] for the CW channels from c0, valid after the closing sync. rows_per: rows an utterance has in f's numbering. */
template <class F>
__device__ __forceinline__ void edb_wg_sum(int64_t n, int B, int rows_per, int c0, int CW, int S, int out_c, double *red, double *tot, F f)
{
	const int tid = threadIdx.x, c = c0 + tid % CW, s = tid / CW;
	const int64_t n_tiles = (n + B - 1) / B;
	double sum = 0.0;
	if (s < S && c < out_c)
		for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
		{
			const int64_t u0 = tile * B;
			const int nu = (int)(n - u0 < B ? n - u0 : B);
			for (int m = s; m < nu * rows_per; m += S) sum += f(u0, m, c);
		}
	__syncthreads(); /* red and tot of the previous sum are read */
	red[tid] = sum;
	__syncthreads();
	if (s == 0 && c < out_c)
	{
		double a = red[tid];
		for (int j = 1; j < S; j++) a += red[j * CW + tid];
		tot[tid] = a;
	}
	__syncthreads();
}

/* rows of z the workgroup g owns in a call of n utterances */
__device__ __forceinline__ int64_t edb_wg_rows(int64_t n, int B, int grid, int g, int R)
{
	const int64_t n_tiles = (n + B - 1) / B;
	int64_t rows = 0;
	for (int64_t tile = g; tile < n_tiles; tile += grid)
	{
		const int64_t u0 = tile * B;
		rows += (n - u0 < B ? n - u0 : B) * R;
	}
	return rows;
}

/* z of 16 rows (M tile mt) x NT tiles of 16 channels from n0: edf_tile's tiling, operands and k order on v_mfma_f32_16x16x4_f32, without
 * its epilogue (z is stored before BatchNorm, ReLU and the pool) and with the chain cut every EDB_CHAIN k: four MFMA steps run in a
 * float32 accumulator from zero, which is then added to a double one. A float32 chain over the whole of K = 576 rounds after each of its
 * products, and that error, carried through three normalised records, alone put the shipped network's deepest batch variance
 * 5e-07 of its maximum from the float64 restatement; chains of 16 leave 1e-07. One rounding to float32 at the store. */
#define EDB_CHAIN 16
template <int NT>
__device__ __forceinline__ void edb_conv_tile(const ed_fnet_layer_t &L, const float *__restrict__ src, int src_n, float *__restrict__ dst, int dst_n,
                                              const float *__restrict__ w, const int32_t *__restrict__ koff, const int32_t *__restrict__ rowin,
                                              const float *__restrict__ bias, int M, int mt, int n0, int lane)
{
	const int r = lane & 15, kq = lane >> 4;
	const int m = mt * 16 + r;
	int base = 0;
	if (m < M)
	{
		const int u = m / L.rows;
		base = u * src_n + rowin[m - u * L.rows];
	}
	double tot[NT][4];
#pragma unroll
	for (int j = 0; j < NT; j++)
#pragma unroll
		for (int i = 0; i < 4; i++) tot[j][i] = 0.0;
	const float *wp = w + kq * L.n_pad + n0 + r;
	for (int k0 = 0; k0 < L.k_pad; k0 += EDB_CHAIN)
	{
		ed_f4 acc[NT];
#pragma unroll
		for (int j = 0; j < NT; j++) acc[j] = (ed_f4){0.0f, 0.0f, 0.0f, 0.0f};
		const int k1 = k0 + EDB_CHAIN < L.k_pad ? k0 + EDB_CHAIN : L.k_pad; /* k_pad is a multiple of 4 */
		for (int k = k0; k < k1; k += 4)
		{
			const int ko = koff[k + kq];
			const float a = ko >= 0 ? src[base + ko] : 0.0f;
#pragma unroll
			for (int j = 0; j < NT; j++) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wp[j * 16], acc[j], 0, 0, 0);
			wp += 4 * L.n_pad;
		}
#pragma unroll
		for (int j = 0; j < NT; j++)
#pragma unroll
			for (int i = 0; i < 4; i++) tot[j][i] += (double)acc[j][i];
	}
	/* D: lane holds rows 4 kq + i (i = 0..3) of channel n0 + 16 j + r */
#pragma unroll
	for (int j = 0; j < NT; j++)
	{
		const int n = n0 + 16 * j + r;
		if (n >= L.out_c) continue; /* a padding channel: not written */
		const double b = (double)bias[n];
#pragma unroll
		for (int i = 0; i < 4; i++)
		{
			const int mi = mt * 16 + 4 * kq + i;
			if (mi >= M) break;
			const int u = mi / L.rows;
			dst[u * dst_n + (mi - u * L.rows) * L.out_c + n] = (float)(tot[j][i] + b);
		}
	}
}

__global__ __launch_bounds__(EDB_THREADS) void edb_conv_kernel(const ed_fbn_plan_t *bp, int l, const float *__restrict__ in, int64_t n)
{
	const ed_fbn_plan_t &b = *bp;
	const ed_fbn_layer_t &Q = b.R[l];
	const ed_fnet_layer_t &L = Q.L;
	const int B = b.batch;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = EDB_THREADS / 64;
	const float *src0 = l ? b.outs + b.R[l - 1].out_at : in;
	const int src_n = Q.in_n, dst_n = Q.R * L.out_c;
	float *z0 = b.zs + Q.z_at;
	const float *gw = b.w + L.w_at;
	const float *bias = gw + (int64_t)L.k_pad * L.n_pad;
	const int32_t *koff = b.tab + L.koff_at, *rowin = b.rtab + Q.rowin_at;
	const int64_t n_tiles = (n + B - 1) / B;
	for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
	{
		const int64_t u0 = tile * B;
		const int nu = (int)(n - u0 < B ? n - u0 : B);
		const int M = nu * Q.R;
		const float *src = src0 + u0 * src_n;
		float *dst = z0 + u0 * dst_n;
		const int MT = (M + 15) / 16, NT = L.n_pad / 16, NG = (NT + 3) / 4;
		for (int item = wave; item < MT * NG; item += n_waves)
		{
			const int mt = item / NG, g = item - mt * NG;
			const int n0 = g * 64, nt = NT - 4 * g < 4 ? NT - 4 * g : 4;
			if (nt == 4) edb_conv_tile<4>(L, src, src_n, dst, dst_n, gw, koff, rowin, bias, M, mt, n0, lane);
			else if (nt == 3) edb_conv_tile<3>(L, src, src_n, dst, dst_n, gw, koff, rowin, bias, M, mt, n0, lane);
			else if (nt == 2) edb_conv_tile<2>(L, src, src_n, dst, dst_n, gw, koff, rowin, bias, M, mt, n0, lane);
			else edb_conv_tile<1>(L, src, src_n, dst, dst_n, gw, koff, rowin, bias, M, mt, n0, lane);
		}
	}
	if (!Q.has_bn) return;

	/* the workgroup's own moments: mean, then M2 from values centred on it */
	__shared__ double red[EDB_THREADS], tot[EDB_THREADS], mean_s[EDB_THREADS];
	__syncthreads(); /* every wave's z is stored */
	const int CW = L.n_pad < EDB_THREADS ? L.n_pad : EDB_THREADS, S = EDB_THREADS / CW;
	const int64_t cnt = edb_wg_rows(n, B, gridDim.x, blockIdx.x, Q.R);
	double *part = b.part + (int64_t)blockIdx.x * 2 * b.bn_n + Q.bn_at;
	const int oc = L.out_c;
	for (int c0 = 0; c0 < oc; c0 += CW)
	{
		edb_wg_sum(n, B, Q.R, c0, CW, S, oc, red, tot, [&](int64_t u0, int m, int c) { return (double)z0[(u0 * Q.R + m) * oc + c]; });
		if (tid < CW) mean_s[tid] = tot[tid] / (double)cnt;
		__syncthreads();
		const double mc = mean_s[tid % CW];
		edb_wg_sum(n, B, Q.R, c0, CW, S, oc, red, tot, [&](int64_t u0, int m, int c) {
			const double d = (double)z0[(u0 * Q.R + m) * oc + c] - mc;
			return d * d;
		});
		if (tid < CW && c0 + tid < oc)
		{
			part[c0 + tid] = mean_s[tid];
			part[b.bn_n + c0 + tid] = tot[tid];
		}
		__syncthreads(); /* mean_s is read before the next channels' replace it */
	}
}

__global__ __launch_bounds__(256) void edb_stats_kernel(const ed_fbn_plan_t *bp, int l, int64_t n, int used, double momentum, double eps, int unbiased)
{
	const ed_fbn_plan_t &b = *bp;
	const ed_fbn_layer_t &Q = b.R[l];
	for (int c = threadIdx.x; c < Q.L.out_c; c += 256)
	{
		double na = 0.0, mean = 0.0, M2 = 0.0;
		for (int g = 0; g < used; g++)
		{
			const double nb = (double)edb_wg_rows(n, b.batch, used, g, Q.R);
			const double *part = b.part + (int64_t)g * 2 * b.bn_n + Q.bn_at;
			const double d = part[c] - mean, tot = na + nb;
			mean += d * nb / tot;
			M2 += part[b.bn_n + c] + d * d * na * nb / tot;
			na = tot;
		}
		const double var = M2 / na;
		const int i = Q.bn_at + c;
		b.mean[i] = (float)mean;
		b.var[i] = (float)var;
		b.rstd[i] = (float)(1.0 / sqrt(var + eps));
		b.mm[i] = (float)(momentum * (double)b.mm[i] + (1.0 - momentum) * mean);
		b.mv[i] = (float)(momentum * (double)b.mv[i] + (1.0 - momentum) * (unbiased ? var * na / (na - 1.0) : var));
	}
}

/* Per pooled output: the window's P elements of z through BatchNorm, ReLU and dropout before the pool, their maximum and its first
 * element, dropout behind the pool; the order and the mask bits are edg_tile's (fnet_grad_kernels.hip). */
__global__ __launch_bounds__(256) void edb_apply_kernel(const ed_fbn_plan_t *bp, int l, int64_t n, ed_fbn_drop_t dr)
{
	const ed_fbn_plan_t &b = *bp;
	const ed_fbn_layer_t &Q = b.R[l];
	const int oc = Q.L.out_c, P = Q.P;
	const float *z0 = b.zs + Q.z_at;
	float *out = b.outs + Q.out_at;
	uint8_t *mask = b.mask + Q.out_at;
	const int64_t stride = (int64_t)gridDim.x * 256;
	for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n * Q.out_n; i += stride)
	{
		const int64_t u = i / Q.out_n;
		const int o = (int)(i - u * Q.out_n), q = o / oc, c = o - q * oc;
		float ga = 1.0f, be = 0.0f, mean = 0.0f, rstd = 1.0f;
		if (Q.has_bn)
		{
			ga = b.bnp[Q.bn_at + c];
			be = b.bnp[b.bn_n + Q.bn_at + c];
			mean = b.mean[Q.bn_at + c];
			rstd = b.rstd[Q.bn_at + c];
		}
		uint32_t kA = 0, kB = 0;
		if (dr.T != 0)
		{
			const uint32_t *k = b.keys + 2 * (u * b.n_layers + l);
			kA = k[0];
			kB = k[1];
		}
		const bool before = dr.T != 0 && dr.before && P > 1;
		float x = 0.0f;
		int e = 0;
		bool kept = true;
		for (int j = 0; j < P; j++)
		{
			const int row = q * P + j;
			float v = z0[(u * Q.R + row) * oc + c];
			if (Q.has_bn) v = ga * ((v - mean) * rstd) + be;
			if (Q.relu) v = fmaxf(v, 0.0f);
			bool kj = true;
			if (before)
			{
				kj = edd_hash((uint32_t)(row * oc + c), kA, kB) >= dr.T;
				v = kj ? v * dr.s : 0.0f;
			}
			if (j == 0 || v > x) /* the first maximum in element order */
			{
				x = v;
				e = j;
				kept = kj;
			}
		}
		int pass = !Q.relu || x > 0.0f ? EDFT_PASS : 0;
		if (dr.T != 0)
		{
			if (!before)
			{
				kept = edd_hash((uint32_t)(q * oc + c), kA, kB) >= dr.T;
				x = kept ? x * dr.s : 0.0f;
			}
			if (!kept) pass |= EDFT_DROPPED;
		}
		out[i] = x;
		mask[i] = (uint8_t)(e | pass);
	}
}

__global__ __launch_bounds__(256) void edb_loss_kernel(const ed_fbn_plan_t *bp, const int32_t *__restrict__ labels, int64_t n, float *__restrict__ loss,
                                                       int32_t *__restrict__ argmax, float *__restrict__ logits, unsigned long long *__restrict__ ignored)
{
	const ed_fbn_plan_t &b = *bp;
	const ed_fbn_layer_t &Q = b.R[b.n_layers - 1];
	const int n_out = b.n_out;
	const float nf = (float)n;
	const int64_t stride = (int64_t)gridDim.x * 256;
	for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < n; u += stride)
	{
		const float *z = b.outs + Q.out_at + u * n_out;
		float *dz = b.douts + Q.out_at + u * n_out;
		const int y = labels[u];
		const bool labelled = (unsigned)y < (unsigned)n_out;
		EDF_SOFTMAX(z, n_out, logits[u * n_out + j] = z[j]; dz[j] = labelled ? (pj - (j == y ? 1.0f : 0.0f)) / nf : 0.0f;)
		if (argmax) argmax[u] = best;
		if (loss) loss[u] = labelled ? logf(s) + mx - z[y] : 0.0f;
		if (!labelled) atomicAdd(ignored, 1ull);
	}
}

/* dy of (row u of the call, the plan's output row r < rows, channel c) from the gradient of the pooled outputs and the mask bytes, as
 * ed_ftrain_grad_kernel builds it: the window's winner gets it if it passes and was not dropped, times the dropout scale. */
__device__ __forceinline__ float edb_dy(const ed_fbn_layer_t &Q, const float *__restrict__ dout, const uint8_t *__restrict__ mask, int64_t u, int r, int c, float ds)
{
	const int q = r / Q.P, e = r - q * Q.P;
	const int64_t o = u * Q.out_n + q * Q.L.out_c + c;
	const int mk = mask[o];
	return (mk & (EDFT_PASS | EDFT_DROPPED)) == EDFT_PASS && (mk & EDFT_WIN_MASK) == e ? dout[o] * ds : 0.0f;
}

__global__ __launch_bounds__(EDB_THREADS) void edb_dysum_kernel(const ed_fbn_plan_t *bp, int l, int64_t n, float ds)
{
	const ed_fbn_plan_t &b = *bp;
	const ed_fbn_layer_t &Q = b.R[l];
	__shared__ double red[EDB_THREADS], tot[EDB_THREADS];
	const int tid = threadIdx.x, oc = Q.L.out_c;
	const int CW = Q.L.n_pad < EDB_THREADS ? Q.L.n_pad : EDB_THREADS, S = EDB_THREADS / CW;
	const float *z0 = b.zs + Q.z_at, *dout = b.douts + Q.out_at;
	const uint8_t *mask = b.mask + Q.out_at;
	double *part = b.part + (int64_t)blockIdx.x * 2 * b.bn_n + Q.bn_at;
	for (int c0 = 0; c0 < oc; c0 += CW)
	{
		edb_wg_sum(n, b.batch, Q.rows, c0, CW, S, oc, red, tot, [&](int64_t u0, int m, int c) {
			const int u = m / Q.rows;
			return (double)edb_dy(Q, dout, mask, u0 + u, m - u * Q.rows, c, ds);
		});
		if (tid < CW && c0 + tid < oc) part[c0 + tid] = tot[tid];
		edb_wg_sum(n, b.batch, Q.rows, c0, CW, S, oc, red, tot, [&](int64_t u0, int m, int c) {
			const int u = m / Q.rows, r = m - u * Q.rows;
			const float zhat = (z0[((u0 + u) * Q.R + r) * oc + c] - b.mean[Q.bn_at + c]) * b.rstd[Q.bn_at + c];
			return (double)edb_dy(Q, dout, mask, u0 + u, r, c, ds) * (double)zhat;
		});
		if (tid < CW && c0 + tid < oc) part[b.bn_n + c0 + tid] = tot[tid];
	}
}

/* dbeta = sum dy, dgamma = sum dy zhat: the workgroups' partial sums in index order */
__global__ __launch_bounds__(256) void edb_dyreduce_kernel(const ed_fbn_plan_t *bp, int l, int used)
{
	const ed_fbn_plan_t &b = *bp;
	const ed_fbn_layer_t &Q = b.R[l];
	for (int c = threadIdx.x; c < Q.L.out_c; c += 256)
	{
		double db = 0.0, dg = 0.0;
		for (int g = 0; g < used; g++)
		{
			const double *part = b.part + (int64_t)g * 2 * b.bn_n + Q.bn_at;
			db += part[c];
			dg += part[b.bn_n + c];
		}
		b.bng[Q.bn_at + c] = (float)dg;
		b.bng[b.bn_n + Q.bn_at + c] = (float)db;
	}
}

__global__ __launch_bounds__(EDB_THREADS) void edb_back_kernel(const ed_fbn_plan_t *bp, int l, const float *__restrict__ in, int64_t n, float ds)
{
	const ed_fbn_plan_t &b = *bp;
	const ed_fbn_layer_t &Q = b.R[l];
	const ed_fnet_layer_t &L = Q.L;
	const ed_ftrain_layer_t &G = Q.G;
	extern __shared__ float lds[];
	const int B = b.batch, oc = L.out_c;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = EDB_THREADS / 64;
	float *dy = lds;
	int32_t *rb = (int32_t *)(lds + (((int64_t)B * Q.R + 15) & ~(int64_t)15) * L.n_pad);
	const float *src0 = l ? b.outs + b.R[l - 1].out_at : in;
	const int src_n = Q.in_n;
	const float *z0 = b.zs + Q.z_at, *dout = b.douts + Q.out_at;
	const uint8_t *mask = b.mask + Q.out_at;
	const int32_t *rowin = b.rtab + Q.rowin_at, *koff = b.tab + L.koff_at;
	float *slab = b.slabs + (int64_t)blockIdx.x * b.w_floats;
	const int64_t n_tiles = (n + B - 1) / B;
	const float Nf = (float)(n * Q.R);
	bool first = true;
	for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x, first = false)
	{
		const int64_t u0 = tile * B;
		const int nu = (int)(n - u0 < B ? n - u0 : B);
		const int M = nu * Q.R, Mp = (M + 15) & ~15;
		__syncthreads(); /* the previous tile's dZ is no longer read */
		for (int i = tid; i < Mp * L.n_pad; i += EDB_THREADS)
		{
			const int m = i / L.n_pad, c = i - m * L.n_pad;
			float v = 0.0f;
			if (m < M && c < oc)
			{
				const int u = m / Q.R, r = m - u * Q.R;
				if (r < Q.rows) v = edb_dy(Q, dout, mask, u0 + u, r, c, ds); /* a truncated position: dy = 0 */
				if (Q.has_bn)
				{
					const int ch = Q.bn_at + c;
					const float rstd = b.rstd[ch];
					const float zhat = (z0[((u0 + u) * Q.R + r) * oc + c] - b.mean[ch]) * rstd;
					v = b.bnp[ch] * rstd * (v - b.bng[b.bn_n + ch] / Nf - zhat * (b.bng[ch] / Nf));
				}
			}
			dy[i] = v;
		}
		for (int m = tid; m < Mp; m += EDB_THREADS)
		{
			const int u = m / Q.R;
			rb[m] = m < M ? u * src_n + rowin[m - u * Q.R] : 0;
		}
		__syncthreads();
		const float *src = src0 + u0 * src_n;
		{
			const int KT = (G.K + 15) / 16, NT = L.n_pad / 16, NG = (NT + 3) / 4;
			for (int item = wave; item < (KT + 1) * NG; item += n_waves)
			{
				const int kt = item / NG, g = item - kt * NG;
				const int n0 = g * 64, nt = NT - 4 * g < 4 ? NT - 4 * g : 4;
				if (nt == 4) edg_dw_tile<4, false>(L, G.K, src, koff, dy, rb, M, kt, KT, n0, lane, slab, first);
				else if (nt == 3) edg_dw_tile<3, false>(L, G.K, src, koff, dy, rb, M, kt, KT, n0, lane, slab, first);
				else if (nt == 2) edg_dw_tile<2, false>(L, G.K, src, koff, dy, rb, M, kt, KT, n0, lane, slab, first);
				else edg_dw_tile<1, false>(L, G.K, src, koff, dy, rb, M, kt, KT, n0, lane, slab, first);
			}
		}
		if (l)
		{
			const int MX = nu * G.np, MT = (MX + 15) / 16, CT = (L.in_c + 15) / 16;
			float *dprev = b.douts + b.R[l - 1].out_at + u0 * src_n;
			for (int item = wave; item < MT * CT; item += n_waves)
			{
				const int mt = item / CT, ct = item - mt * CT;
				edg_dx_tile(L, G, b.inv + G.inv_at, b.w + L.w_at, dy, MX, mt, ct * 16, lane, dprev, src_n);
			}
		}
	}
}

/* grad[i] = slab 0's [i] + slab 1's [i] + ... in that order. A BatchNorm record's bias gradient is zero in exact arithmetic (sum dz = 0):
 * it is written as +0.0f, not as that sum's rounding noise (its padding entries are +0.0f in every slab already). */
__global__ __launch_bounds__(256) void edb_reduce_kernel(const ed_fbn_plan_t *bp, int n_slabs, float *__restrict__ grad)
{
	const ed_fbn_plan_t &b = *bp;
	const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, w_floats = b.w_floats;
	if (i >= w_floats) return;
	int l = 0;
	while (l + 1 < b.n_layers && i >= b.R[l + 1].L.w_at) l++;
	const ed_fbn_layer_t &Q = b.R[l];
	float s = b.slabs[i];
	for (int g = 1; g < n_slabs; g++) s += b.slabs[g * w_floats + i];
	grad[i] = Q.has_bn && i - Q.L.w_at >= (int64_t)Q.L.k_pad * Q.L.n_pad ? 0.0f : s;
}

__global__ __launch_bounds__(256) void edb_fold_kernel(const ed_fbn_plan_t *bp, float *__restrict__ dst, float eps)
{
	const ed_fbn_plan_t &b = *bp;
	const int64_t stride = (int64_t)gridDim.x * 256;
	for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < b.w_floats; i += stride)
	{
		int l = 0;
		while (l + 1 < b.n_layers && i >= b.R[l + 1].L.w_at) l++;
		const ed_fbn_layer_t &Q = b.R[l];
		const int64_t off = i - Q.L.w_at, nw = (int64_t)Q.L.k_pad * Q.L.n_pad;
		const bool is_bias = off >= nw;
		const int c = (int)(is_bias ? off - nw : off % Q.L.n_pad), k = (int)(is_bias ? 0 : off / Q.L.n_pad);
		float v = b.w[i];
		if (Q.has_bn && c < Q.L.out_c && k < Q.G.K) /* the padding is copied */
		{
			const int ch = Q.bn_at + c;
			const float s = b.bnp[ch] / sqrtf(b.mv[ch] + eps);
			v = is_bias ? (v - b.mm[ch]) * s + b.bnp[b.bn_n + ch] : v * s;
		}
		dst[i] = v;
	}
}

static unsigned edb_blocks(int64_t count, int grid)
{
	int64_t blocks = (count + 255) / 256;
	const int64_t cap = (int64_t)(grid > 0 ? grid : 1) * 8;
	if (blocks > cap) blocks = cap;
	return (unsigned)(blocks < 1 ? 1 : blocks);
}

#define EDB_LAUNCHED { const int e_ = (int)hipGetLastError(); if (e_) return e_; }

extern "C" int ed_launch_fbn_train(const ed_fbn_plan_t *b, const ed_fbn_plan_t *d_b, const float *in, const int32_t *labels, int64_t n, float *loss,
                                   int32_t *argmax, float *logits, float *grad, unsigned long long *ignored, const ed_fbn_drop_t *drop, uint64_t seed,
                                   uint64_t call, double momentum, double eps, uint32_t flags, hipStream_t stream)
{
	if (n <= 0) return 0;
	const int nl = b->n_layers;
	const size_t lds = ed_fbn_lds_bytes(b, b->batch);
	if (n > b->max_rows || n > 0xffffffffll || nl < 1 || nl > ED_FNET_MAX_LAYERS || b->batch < 1 || b->grid < 1 || lds > ED_FNET_LDS_BYTES) return (int)hipErrorInvalidValue;
	{ const int e = ed_kernel_prepare((const void *)edb_back_kernel, EDB_THREADS, lds, NULL, NULL); if (e) return e; }
	const int64_t n_tiles = (n + b->batch - 1) / b->batch;
	const unsigned used = (unsigned)(n_tiles < b->grid ? n_tiles : b->grid); /* a workgroup without a tile would leave its slab and its moments stale */
	bool any_drop = false;
	for (int l = 0; l < nl; l++) any_drop = any_drop || drop[l].T != 0;
	if (any_drop)
	{
		hipLaunchKernelGGL(edb_keys_kernel, dim3(edb_blocks(n * nl, b->grid)), dim3(256), 0, stream, n, nl, seed, call, b->keys);
		EDB_LAUNCHED
	}
	for (int l = 0; l < nl; l++)
	{
		hipLaunchKernelGGL(edb_conv_kernel, dim3(used), dim3(EDB_THREADS), 0, stream, d_b, l, in, n);
		EDB_LAUNCHED
		if (b->R[l].has_bn)
		{
			hipLaunchKernelGGL(edb_stats_kernel, dim3(1), dim3(256), 0, stream, d_b, l, n, (int)used, momentum, eps, (int)(flags & EDBN_UNBIASED));
			EDB_LAUNCHED
		}
		hipLaunchKernelGGL(edb_apply_kernel, dim3(edb_blocks(n * b->R[l].out_n, b->grid)), dim3(256), 0, stream, d_b, l, n, drop[l]);
		EDB_LAUNCHED
	}
	hipLaunchKernelGGL(edb_loss_kernel, dim3(edb_blocks(n, b->grid)), dim3(256), 0, stream, d_b, labels, n, loss, argmax, logits, ignored);
	EDB_LAUNCHED
	for (int l = nl - 1; l >= 0; l--)
	{
		const float ds = drop[l].T != 0 ? drop[l].s : 1.0f;
		if (b->R[l].has_bn)
		{
			hipLaunchKernelGGL(edb_dysum_kernel, dim3(used), dim3(EDB_THREADS), 0, stream, d_b, l, n, ds);
			EDB_LAUNCHED
			hipLaunchKernelGGL(edb_dyreduce_kernel, dim3(1), dim3(256), 0, stream, d_b, l, (int)used);
			EDB_LAUNCHED
		}
		hipLaunchKernelGGL(edb_back_kernel, dim3(used), dim3(EDB_THREADS), lds, stream, d_b, l, in, n, ds);
		EDB_LAUNCHED
	}
	hipLaunchKernelGGL(edb_reduce_kernel, dim3((unsigned)((b->w_floats + 255) / 256)), dim3(256), 0, stream, d_b, (int)used, grad);
	return (int)hipGetLastError();
}

extern "C" int ed_launch_fbn_fold(const ed_fbn_plan_t *b, const ed_fbn_plan_t *d_b, float *dst, double eps, hipStream_t stream)
{
	hipLaunchKernelGGL(edb_fold_kernel, dim3(edb_blocks(b->w_floats, b->grid)), dim3(256), 0, stream, d_b, dst, (float)eps);
	return (int)hipGetLastError();
}
