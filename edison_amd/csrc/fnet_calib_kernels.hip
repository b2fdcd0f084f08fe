/*
 * fnet_calib_kernels.hip -- the calibration pass of quantising a float32 network (edison_fcal.hip, edison_amd/quantize.py; DESIGN.md
 * section 18): ed_fnet_calib_kernel takes a tile of utterances through the network with ed_fnet_kernel's own code (fnet_device.h: the
 * LDS plan, the walk EDF_LAYER_WALK and the work item edf_tile, with the sink edfc_sink) and, instead of writing logits, reduces the network
 * input and every conv / dense record to three integers each:
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

/* edf_tile's sink: every real value acc + bias, before ReLU and before the pool, into the lane's maximum and the workgroup's histogram.
 * A padding row of the last M tile is not counted, nor is an absent row of a padded record (an element of a pool window in the pool's
 * padding); a padding channel never reaches the sink. */
struct edfc_sink
{
	uint32_t amax;
	uint32_t *__restrict__ s_hist;
	__device__ __forceinline__ void pre(float v, bool real) { if (real) edfc_see(v, amax, s_hist); }
	__device__ __forceinline__ void out(const ed_fnet_layer_t &, int, int, int, float, const float *) {}
};

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
	EDF_LDS_PLAN
	uint32_t *s_stat = (uint32_t *)(kl + p.k_lds); /* EDFC_LDS_WORDS: hist[256], then the maximum */
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

	/* the walk's first __syncthreads also stands behind the previous statistic's flush */
	for (int l = 0; l < p.n_layers; l++)
	{
		const ed_fnet_layer_t &L = p.L[l];
		edfc_sink sink = {0, s_stat};
		EDF_LAYER_WALK(true, edf_item, L, (float *)NULL, 0, 0, sink)
		edfc_wave_max(sink.amax, lane, s_stat);
		__syncthreads();
		edfc_flush(l + 1, (unsigned long long)nu * (unsigned long long)L.live * (unsigned long long)L.out_c, s_stat, counters, tid);
	}
}

extern "C" int ed_launch_fnet_calib(const ed_fnet_plan_t *p, const float *in, int64_t n, unsigned long long *counters, hipStream_t stream)
{
	if (n <= 0) return 0;
	const size_t lds = ed_fnet_calib_lds_bytes(p);
	if (!ed_fnet_plan_launchable(p, lds)) return (int)hipErrorInvalidValue;
	{ const int e = ed_kernel_prepare((const void *)ed_fnet_calib_kernel, ED_FNET_THREADS, lds, NULL, NULL); if (e) return e; }
	const int64_t blocks = (n + p->batch - 1) / p->batch;
	if (blocks > INT32_MAX) return (int)hipErrorInvalidValue;
	hipLaunchKernelGGL(ed_fnet_calib_kernel, dim3((unsigned)blocks), dim3(ED_FNET_THREADS), lds, stream, *p, in, n, counters);
	return (int)hipGetLastError();
}
