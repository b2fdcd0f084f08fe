/*
 * mfcc_exact_kernels.hip -- the float64 recompute of the exact KWS mode (edison_kws_set_exact), hand-written HIP for gfx950.
 *
 * The fast MFCC kernel works in fp32; its flagging instance (ed_mfcc2_flag_kernel, mfcc_kernels.hip) lists the frames whose int8
 * feature lies so close to a rounding boundary that the fp32 error could move it. This kernel takes that list
 * and recomputes each listed frame the way the host flow does, in float64 (variant B, mfcc_utils.py:287-322; oracle/mfcc_ref.c
 * restates it):
 *   1. z[n] = x[2n] + i x[2n+1], n < 512, to LDS in bit-reversed order
 *   2. FFT512: radix-2 decimation in time in place, stages fused in pairs (four radix-2^2 passes + one radix-2 pass), float64
 *      twiddles from the context's table
 *   3. split X[k] = E[k] + W1024^k O[k], k = 0..512, and the spectrum |X[k]| / 1024 / sqrt(2)
 *   4. mel: band j = sum over its nonzero weights (mel_mtx_scale W[k][j]) in ascending k, then / mel_mtx_scale
 *   5. [ln(x + 1e-6)], DCT-II: y[c] = (1/64) sum_n L[n] 2 cos(pi c (2n+1) / 64), c < n_coef
 *   6. feature = (int8) rintf(clip((float)y * scale, -128, 127)): kws_nnom.py:359-361 (oracle/mfcc_ref.c:219-231)
 * and overwrites the frame's row of the features.
 *
 * Persistent and list-driven: the grid is what is resident, every wavefront reads the list length the flagging kernel left on the
 * device (no host round trip) and takes listed frames one at a time (wave w of the grid: entries w, w + W, ...). A wavefront owns one
 * frame at a time and its own LDS, so there is no workgroup barrier.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edison_internal.h"
#include "edison_launch.h"
#include "mfcc_fft.h"

#define EDX_WPB 4 /* wavefronts per workgroup */

struct edx_wave_lds
{
	double2 z[512];   /* the packed frame / its FFT, in place       */
	double spec[520]; /* |X[k]| / 1024 / sqrt 2, k = 0..512         */
	double lm[32];    /* mel bands (ln taken when use_log)          */
};

__device__ __forceinline__ double2 edx_cmul(double2 a, double2 w)
{
	return make_double2(fma(a.x, w.x, -a.y * w.y), fma(a.x, w.y, a.y * w.x));
}

/* a = a + w b, b = a - w b */
__device__ __forceinline__ void edx_bfly(double2 &a, double2 &b, double2 w)
{
	const double2 t = edx_cmul(b, w);
	b = make_double2(a.x - t.x, a.y - t.y);
	a = make_double2(a.x + t.x, a.y + t.y);
}

__global__ __launch_bounds__(64 * EDX_WPB) void ed_mfcc_exact_kernel(ed_exact_args_t args, const ed_exact_tables_t *__restrict__ tab)
{
	__shared__ edx_wave_lds lds[EDX_WPB];
	const int lane = threadIdx.x & 63;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	edx_wave_lds &L = lds[wave];
	const double2 *__restrict__ tw = reinterpret_cast<const double2 *>(&tab->tw[0][0]);
	/* the flagging kernel ran before this one on the same stream: its count is complete */
	const uint32_t n_listed = __builtin_amdgcn_readfirstlane(__hip_atomic_load(args.count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
	const uint32_t fpg = (uint32_t)args.frames_per_group;

	for (uint32_t e = blockIdx.x * EDX_WPB + wave; e < n_listed; e += gridDim.x * EDX_WPB)
	{
		const uint32_t f = __builtin_amdgcn_readfirstlane(args.list[e]);
		const uint32_t g = f / fpg, i = f - g * fpg;
		const int16_t *x = args.audio + ((int64_t)g * args.group_stride + (int64_t)i * args.frame_step);

		/* ---- 1. load, bit-reversed */
#pragma unroll
		for (int t = 0; t < 8; t++)
		{
			const uint32_t n = lane + 64 * t;
			L.z[__brev(n) >> 23] = make_double2((double)x[2 * n], (double)x[2 * n + 1]);
		}
		ed_wave_sync();

		/* ---- 2. FFT512: stages h and 2h (half-widths) of the radix-2 DIT in one pass over groups {b, b+h, b+2h, b+3h} */
#pragma unroll
		for (int h = 1; h <= 64; h *= 4)
		{
#pragma unroll
			for (int t = 0; t < 2; t++)
			{
				const int gq = lane + 64 * t; /* 128 groups */
				const int r = gq & (h - 1);
				const int b = (gq - r) * 4 + r;
				double2 x0 = L.z[b], x1 = L.z[b + h], x2 = L.z[b + 2 * h], x3 = L.z[b + 3 * h];
				const double2 w1 = tw[r * (512 / h)];        /* W_{2h}^r  */
				const double2 w2a = tw[r * (256 / h)];       /* W_{4h}^r  */
				const double2 w2b = tw[(r + h) * (256 / h)]; /* W_{4h}^{r+h} */
				edx_bfly(x0, x1, w1);
				edx_bfly(x2, x3, w1);
				edx_bfly(x0, x2, w2a);
				edx_bfly(x1, x3, w2b);
				L.z[b] = x0; L.z[b + h] = x1; L.z[b + 2 * h] = x2; L.z[b + 3 * h] = x3;
			}
			ed_wave_sync();
		}
#pragma unroll
		for (int t = 0; t < 4; t++) /* last stage, h = 256 */
		{
			const int r = lane + 64 * t;
			double2 x0 = L.z[r], x1 = L.z[r + 256];
			edx_bfly(x0, x1, tw[2 * r]);
			L.z[r] = x0; L.z[r + 256] = x1;
		}
		ed_wave_sync();

		/* ---- 3. real-FFT split and spectrum: X[k] = (Z[k] + conj Z[-k]) / 2 - i W1024^k (Z[k] - conj Z[-k]) / 2 */
#pragma unroll
		for (int t = 0; t < 9; t++)
		{
			const int k = lane + 64 * t;
			if (k > 512) break;
			const double2 a = L.z[k & 511], p = L.z[(512 - k) & 511];
			const double er = 0.5 * (a.x + p.x), ei = 0.5 * (a.y - p.y);  /* E = (A + conj P) / 2 */
			const double orr = 0.5 * (a.y + p.y), oi = -0.5 * (a.x - p.x); /* O = (A - conj P) / 2i */
			const double2 w = k < 512 ? tw[k] : make_double2(-1.0, 0.0);
			const double xr = er + (orr * w.x - oi * w.y), xi = ei + (orr * w.y + oi * w.x);
			/* mfcc_utils.py:297-300: |X / 1024| / sqrt 2 */
			L.spec[k] = 0.70710678118654752440 * sqrt(fma(xr, xr, xi * xi)) * (1.0 / 1024.0);
		}
		ed_wave_sync();

		/* ---- 4. mel: lane j and lane j + 32 each sum half of band j's run, in ascending order */
		{
			const int j = lane & 31, half = lane >> 5;
			const int len = tab->mel_len[j], k0 = tab->mel_k0[j], off = tab->mel_off[j];
			const int mid = len / 2;
			const int t0 = half ? mid : 0, t1 = half ? len : mid;
			double acc = 0.0;
			for (int t = t0; t < t1; t++) acc = fma(L.spec[k0 + t], tab->mel_w[off + t], acc);
			acc += __shfl_down(acc, 32);
			if (lane < 32)
			{
				double m = acc / tab->mel_div; /* mfcc_utils.py:309 */
				if (args.use_log) m = log(m + 1e-6);
				L.lm[j] = m;
			}
		}
		ed_wave_sync();

		/* ---- 5./6. DCT-II / 64 and the int8 feature */
		if (lane < args.n_coef)
		{
			double acc = 0.0;
#pragma unroll 8
			for (int n = 0; n < 32; n++) acc = fma(L.lm[n], tab->dct[lane][n], acc);
			const double y = (1.0 / 64.0) * acc;
			const float v = fminf(fmaxf((float)y * args.feat_scale, -128.0f), 127.0f);
			args.feat[(int64_t)f * args.n_coef + lane] = (int8_t)rintf(v);
		}
		ed_wave_sync(); /* the next frame rewrites this wave's LDS */
	}
}

/* Persistent grid: every resident workgroup, each ends at once when the list is short. */
extern "C" int ed_launch_mfcc_exact(const ed_exact_args_t *args, const ed_exact_tables_t *dev_tab, int n_cu, hipStream_t stream)
{
	const void *fn = (const void *)ed_mfcc_exact_kernel;
	int bpc = 1;
	{ const int e = ed_kernel_prepare(fn, 64 * EDX_WPB, 0, NULL, &bpc); if (e) return e; }
	void *kargs[] = {(void *)args, (void *)&dev_tab};
	return (int)hipLaunchKernel(fn, dim3((unsigned)(n_cu * bpc)), dim3(64 * EDX_WPB), kargs, 0, stream);
}
