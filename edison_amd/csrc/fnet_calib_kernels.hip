/*
 * fnet_calib_kernels.hip -- the calibration pass of quantising a float32 network (edison_fcal.hip, edison_amd/quantize.py; DESIGN.md
 * section 18): ed_fnet_calib_kernel takes a tile of utterances through the network exactly as ed_fnet_kernel does (fnet_device.h: the
 * same tiling, the same k-ordered MFMA loop, the same epilogue order) and, instead of writing logits, reduces the network input and
 * every conv / dense record to three integers each:
 *
 *   absmax  the largest bit pattern of fabsf(v) as uint32 (for non-negative floats the integer order is the float order; an Inf or a
 *           NaN anywhere wins and the quantiser refuses it)
 *   hist    how many v have biased exponent field e = (bits >> 23) & 0xff, 256 uint64 counters
 *   count   how many v
 *
 * v runs over the in_n input floats of every utterance, and for a record over acc + bias in f32 -- the kernel's value before ReLU and
 * before the pool -- at rows < M and channels < out_c: the padding of the last M tile and of the last channel tile is not counted.
 * Rows a truncating pool drops are never computed (fnet.h: the rows of a layer are those of its pool windows), so they are not
 * counted either. In a padded record the absent elements of a pool window -- those in the pool's padding -- are
 * not counted: the count is the record's live rows x out_c.
 *
 * Per work item every lane keeps a running maximum in a register and bumps a workgroup histogram in LDS (an LDS add without return).
 * Per layer and workgroup: the waves reduce their maxima (shuffles, then one LDS atomicMax per wave), then one global atomicMax, one
 * global add of the count -- the tile's real rows x out_c, known without counting -- and a flush of the non-zero histogram cells into the 64-bit
 * device counters. Integer atomics only, as eval_kernels.hip and for its reason: the counters do not depend on the launch shape or on
 * the order the atomics arrive in. No scratch memory; no logits, no softmax.
 *
 * Device counters, uint64 words, EDFC_WORDS per index (0 = the input, i = record i - 1): [0] absmax in its low 32 bits (the atomicMax
 * is a 32-bit one on the word's first half), [1] count, [2 .. 258) hist.
 *
 * LDS: ed_fnet_kernel's plan (two activation buffers, the layer's weights, its k offsets) and behind it EDFC_LDS_WORDS uint32: the
 * histogram and the maximum. The calibrator's plan holds those bytes back when it sizes its batch (edison_fcal.hip).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edison_launch.h"
#include "fnet.h"
#include "fnet_calib.h"
#include "fnet_device.h"

/* one value into the lane's maximum and the workgroup's histogram */
__device__ __forceinline__ void edfc_see(float v, uint32_t &amax, uint32_t *__restrict__ s_hist)
{
	const uint32_t b = __float_as_uint(fabsf(v));
	amax = b > amax ? b : amax;
	atomicAdd(&s_hist[b >> 23], 1u);
}

/* edf_tile with the statistic in its epilogue: 16 output rows (M tile mt) x NT tiles of 16 channels starting at n0. The MFMA loop and
 * the order bias, ReLU, pool are edf_tile's; nothing is dumped. PAD = true is a padded record (fnet.h): edf_tile's gather, and an absent
 * row -- an element of a pool window in the pool's padding -- is not counted and is -inf in the window's max. */
template <int NT, bool PAD = false>
__device__ __forceinline__ void edfc_tile(const ed_fnet_layer_t &L, const float *__restrict__ src, int src_n, float *__restrict__ dst, int dst_n,
                                          const float *__restrict__ wl, const int32_t *__restrict__ kl, const int32_t *__restrict__ rowin,
                                          const float *__restrict__ bias, int M, int mt, int n0, int lane, uint32_t &amax, uint32_t *__restrict__ s_hist)
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
		if (n >= L.out_c) continue; /* a padding channel: not counted, not written */
		const float b = bias[n];
		float v[4];
#pragma unroll
		for (int i = 0; i < 4; i++)
		{
			v[i] = acc[j][i] + b;
			if constexpr (PAD)
			{
				if (live[i]) edfc_see(v[i], amax, s_hist); /* neither a padding row nor an absent one */
			}
			else if (m0 + i < M) edfc_see(v[i], amax, s_hist); /* before ReLU, before the pool; a padding row is not counted */
			if (L.relu) v[i] = fmaxf(v[i], 0.0f);
			if constexpr (PAD) { if (!live[i]) v[i] = -INFINITY; }
		}
		for (int g = 0; g < 4; g += P)
		{
			const int mg = m0 + g;
			if (mg >= M) break;
			float x = v[g];
			if (P >= 2) x = fmaxf(x, v[g + 1]);
			if (P == 4) x = fmaxf(fmaxf(x, v[g + 2]), v[g + 3]);
			const int u = mg / L.rows, q = (mg - u * L.rows) / P;
			dst[u * dst_n + q * L.out_c + n] = x;
		}
	}
}

/* the wave's maximum into the workgroup's (s_stat[EDFC_HIST] is the maximum) */
__device__ __forceinline__ void edfc_wave_max(uint32_t amax, int lane, uint32_t *__restrict__ s_stat)
{
	for (int d = 32; d > 0; d >>= 1)
	{
		const uint32_t o = (uint32_t)__shfl_xor((int)amax, d);
		amax = o > amax ? o : amax;
	}
	if (lane == 0 && amax) atomicMax(&s_stat[EDFC_HIST], amax);
}

/* After a __syncthreads behind the last bump: the workgroup's statistic of index idx into the device counters, and the LDS cells back
 * to zero (the caller's next __syncthreads comes before the next bump). */
__device__ __forceinline__ void edfc_flush(int idx, unsigned long long values, uint32_t *__restrict__ s_stat, unsigned long long *__restrict__ counters, int tid)
{
	unsigned long long *c = counters + (size_t)idx * EDFC_WORDS;
	if (tid < EDFC_HIST)
	{
		const uint32_t h = s_stat[tid];
		if (h)
		{
			atomicAdd(&c[2 + tid], (unsigned long long)h);
			s_stat[tid] = 0;
		}
	}
	else if (tid == EDFC_HIST)
	{
		const uint32_t a = s_stat[EDFC_HIST];
		if (a)
		{
			atomicMax((uint32_t *)&c[0], a); /* little endian: the word's low half */
			s_stat[EDFC_HIST] = 0;
		}
		if (values) atomicAdd(&c[1], values);
	}
}

__global__ __launch_bounds__(ED_FNET_THREADS) void ed_fnet_calib_kernel(ed_fnet_plan_t p, const float *__restrict__ in, int64_t n,
                                                                          unsigned long long *__restrict__ counters)
{
	extern __shared__ float lds[];
	const int B = p.batch;
	float *buf[2] = {lds, lds + B * p.buf_n[0]};
	float *wl = lds + B * (p.buf_n[0] + p.buf_n[1]);
	int32_t *kl = (int32_t *)(wl + p.w_lds);
	uint32_t *s_stat = (uint32_t *)(kl + p.k_lds); /* EDFC_LDS_WORDS: hist[256], then the maximum */
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = ED_FNET_THREADS / 64;
	const int64_t u0 = (int64_t)blockIdx.x * B;
	const int nu = (int)(n - u0 < B ? n - u0 : B);

	if (tid < EDFC_LDS_WORDS) s_stat[tid] = 0;
	__syncthreads();

	/* the network input of the tile's utterances into buffer 0, and its statistic (index 0) */
	{
		uint32_t amax = 0;
		for (int i = tid; i < nu * p.in_n; i += ED_FNET_THREADS)
		{
			const int u = i / p.in_n, e = i - u * p.in_n;
			const float x = in[(u0 + u) * (int64_t)p.in_n + e];
			buf[0][u * p.buf_n[0] + e] = x;
			edfc_see(x, amax, s_stat);
		}
		edfc_wave_max(amax, lane, s_stat);
		__syncthreads();
		edfc_flush(0, (unsigned long long)nu * (unsigned long long)p.in_n, s_stat, counters, tid);
	}

	for (int l = 0; l < p.n_layers; l++)
	{
		const ed_fnet_layer_t &L = p.L[l];
		const float *gw = p.w + L.w_at;
		__syncthreads(); /* the previous layer's outputs are written, its weights no longer read, its statistic flushed */
		{
			const int nw = L.k_pad * L.n_pad; /* a multiple of 64: float4 copies */
			const float4 *g4 = (const float4 *)gw;
			float4 *l4 = (float4 *)wl;
			for (int i = tid; i < nw / 4; i += ED_FNET_THREADS) l4[i] = g4[i];
			const int nk = L.pad ? 2 * L.k_pad : L.k_pad; /* a padded record: kyx behind koff */
			for (int i = tid; i < nk; i += ED_FNET_THREADS) kl[i] = p.tab[L.koff_at + i];
		}
		__syncthreads();
		const float *src = buf[L.src];
		float *dst = buf[L.dst];
		const int src_n = p.buf_n[L.src], dst_n = p.buf_n[L.dst];
		const int32_t *rowin = p.tab + L.rowin_at;
		const float *bias = gw + (int64_t)L.k_pad * L.n_pad;
		const int M = nu * L.rows;
		const int MT = (M + 15) / 16, NT = L.n_pad / 16, NG = (NT + 3) / 4;
		uint32_t amax = 0;
		for (int item = wave; item < MT * NG; item += n_waves)
		{
			const int mt = item / NG, g = item - mt * NG;
			const int n0 = g * 64, nt = NT - 4 * g < 4 ? NT - 4 * g : 4;
			if (L.pad)
			{
				if (nt == 4) edfc_tile<4, true>(L, src, src_n, dst, dst_n, wl, kl, rowin, bias, M, mt, n0, lane, amax, s_stat);
				else if (nt == 3) edfc_tile<3, true>(L, src, src_n, dst, dst_n, wl, kl, rowin, bias, M, mt, n0, lane, amax, s_stat);
				else if (nt == 2) edfc_tile<2, true>(L, src, src_n, dst, dst_n, wl, kl, rowin, bias, M, mt, n0, lane, amax, s_stat);
				else edfc_tile<1, true>(L, src, src_n, dst, dst_n, wl, kl, rowin, bias, M, mt, n0, lane, amax, s_stat);
			}
			else if (nt == 4) edfc_tile<4>(L, src, src_n, dst, dst_n, wl, kl, rowin, bias, M, mt, n0, lane, amax, s_stat);
			else if (nt == 3) edfc_tile<3>(L, src, src_n, dst, dst_n, wl, kl, rowin, bias, M, mt, n0, lane, amax, s_stat);
			else if (nt == 2) edfc_tile<2>(L, src, src_n, dst, dst_n, wl, kl, rowin, bias, M, mt, n0, lane, amax, s_stat);
			else edfc_tile<1>(L, src, src_n, dst, dst_n, wl, kl, rowin, bias, M, mt, n0, lane, amax, s_stat);
		}
		edfc_wave_max(amax, lane, s_stat);
		__syncthreads();
		edfc_flush(l + 1, (unsigned long long)nu * (unsigned long long)L.live * (unsigned long long)L.out_c, s_stat, counters, tid);
	}
}

extern "C" int ed_launch_fnet_calib(const ed_fnet_plan_t *p, const float *in, int64_t n, unsigned long long *counters, hipStream_t stream)
{
	if (n <= 0) return 0;
	const size_t lds = ed_fnet_calib_lds_bytes(p);
	if (lds > ED_FNET_LDS_BYTES || p->batch < 1 || p->n_layers < 1 || p->n_layers > ED_FNET_MAX_LAYERS) return (int)hipErrorInvalidValue;
	{ const int e = ed_kernel_prepare((const void *)ed_fnet_calib_kernel, ED_FNET_THREADS, lds, NULL, NULL); if (e) return e; }
	const int64_t blocks = (n + p->batch - 1) / p->batch;
	if (blocks > INT32_MAX) return (int)hipErrorInvalidValue;
	hipLaunchKernelGGL(ed_fnet_calib_kernel, dim3((unsigned)blocks), dim3(ED_FNET_THREADS), lds, stream, *p, in, n, counters);
	return (int)hipGetLastError();
}
