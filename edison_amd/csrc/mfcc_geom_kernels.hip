/*
 * mfcc_geom_kernels.hip -- audio -> int8 network input for MFCC variants A and B at ANY geometry the generality path accepts (frame_len
 * 4 .. 4096, mel_nbins 1 .. 256), batched over all frames of all utterances of a call: the feature stage of edison_kws_geom_batch*
 * (edison_kws_geom.hip). Float64 throughout, as the reference computes (mfcc_utils.py:134-199 `mfcc`, :255-323 `mfcc_mcu`), so the int8
 * features are the reference host flow's. Per frame:
 *   1. load: N even -- z[n] = x[2n] + i x[2n+1], n < M = N/2 (the real frame packed into complex pairs); N odd -- z[n] = x[n], M = N
 *   2. Stockham FFT over M points in LDS, radix 4 / 2 / 3 / 5 stages ping-ponging between two buffers (self-sorting: natural order in
 *      and out); twiddles W_M^j = W_N^(j N / M) from the host-built table of W_N^j
 *      -- or, when M has a prime factor above 5 (441, 882, ...), a direct DFT of the real frame against the same table (N^2/2 fma)
 *   3. N even: real split X[k] = (Z[k] + conj Z[M-k]) / 2 - i W_N^k (Z[k] - conj Z[M-k]) / 2, k = 0 .. N/2
 *   4. spectrum s[k] = |X[k] * fft_scale| * spec_scale for the variant's n_bins bins (A: N/2 bins, 1, 1; B: N/2 + 1 bins, 1/1024, 1/sqrt 2)
 *   5. mel: band j = sum of its nonzero run of the filterbank in ascending k, / mel_div; ln(x + 1e-6) for A and B with use_log
 *   6. DCT-II rows first_mfcc .. first_mfcc + num_mfcc - 1 over dct_div (A sqrt(2 mel_nbins), B 64); feature = int8 of
 *      rint(clip((float)y * feat_scale, -128, 127)) (kws_nnom.py:359-361), written to feat + g * num_mfcc + row
 *      -- or, in the float64 instance (ed_mfcc_geom_f64_kernel, edison_mfcc_geom_batch*), y itself to mfcc + g * num_mfcc + row
 *
 * Work split: a TEAM of threads owns one frame at a time and a private LDS slice of r0 + r1 + r2 doubles (two FFT buffers -- the
 * spectrum goes to the one the FFT's result is not in -- and the mel bands); teams take frames g = team, team + n_teams, ... of the
 * whole call. TEAM = 64 (a wavefront; four per workgroup, no workgroup barrier) where the slice is at most 20 KiB, which covers every
 * even N <= 1024 and mel_nbins <= 256; TEAM = 256 (the workgroup) for the longer frames.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edison_launch.h"
#include "mfcc_fft.h"
#include "mfcc_geom.h"

#define EDG_BLOCK 256
#define EDG_WAVE_LDS_MAX 20480 /* bytes of a wavefront team's slice: 4 per workgroup <= 80 KiB, two workgroups per CU */

__device__ __forceinline__ double2 edg_cmul(double2 a, double2 w) { return make_double2(fma(a.x, w.x, -a.y * w.y), fma(a.x, w.y, a.y * w.x)); }
__device__ __forceinline__ double2 edg_add(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 edg_sub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }

template <int TEAM> __device__ __forceinline__ void edg_sync()
{
	if (TEAM == 64) ed_wave_sync();
	else __syncthreads();
}

/* V[q] = sum_r v[r] W_R^(r q) */
template <int R> __device__ __forceinline__ void edg_dft(double2 *v)
{
	if (R == 2)
	{
		const double2 a = v[0], b = v[1];
		v[0] = edg_add(a, b);
		v[1] = edg_sub(a, b);
	}
	else if (R == 4)
	{
		const double2 s02 = edg_add(v[0], v[2]), d02 = edg_sub(v[0], v[2]), s13 = edg_add(v[1], v[3]), d13 = edg_sub(v[1], v[3]);
		v[0] = edg_add(s02, s13);
		v[2] = edg_sub(s02, s13);
		v[1] = make_double2(d02.x + d13.y, d02.y - d13.x); /* d02 - i d13 */
		v[3] = make_double2(d02.x - d13.y, d02.y + d13.x); /* d02 + i d13 */
	}
	else
	{
		/* R = 3, 5: W_R^m = cos(2 pi m / R) - i sin(2 pi m / R) */
		const double c3[3] = {1.0, -0.5, -0.5}, s3[3] = {0.0, -0.86602540378443864676, 0.86602540378443864676};
		const double c5[5] = {1.0, 0.30901699437494742410, -0.80901699437494742410, -0.80901699437494742410, 0.30901699437494742410};
		const double s5[5] = {0.0, -0.95105651629515357212, -0.58778525229247312917, 0.58778525229247312917, 0.95105651629515357212};
		double2 o[R];
#pragma unroll
		for (int q = 0; q < R; q++)
		{
			double2 acc = v[0];
#pragma unroll
			for (int r = 1; r < R; r++)
			{
				const int m = (r * q) % R;
				const double2 w = R == 3 ? make_double2(c3[m], s3[m]) : make_double2(c5[m], s5[m]);
				acc = edg_add(acc, edg_cmul(v[r], w));
			}
			o[q] = acc;
		}
#pragma unroll
		for (int q = 0; q < R; q++) v[q] = o[q];
	}
}

/* One Stockham stage of radix R: sub-transforms of length ns become length ns R (Govindaraju et al., SC'08, "High performance discrete
 * Fourier transforms on graphics processors"): butterfly j takes src[j + r M/R], twiddles by W_{ns R}^{(j mod ns) r}, writes
 * dst[(j - j mod ns) R + j mod ns + q ns]. */
template <int R, int TEAM>
__device__ __forceinline__ void edg_stage(const double2 *src, double2 *dst, int M, int ns, int tws, const double2 *__restrict__ tw, int tid)
{
	const int mr = M / R, tstep = (M / (ns * R)) * tws; /* W_{ns R}^m = W_N^(m tstep) */
	for (int j = tid; j < mr; j += TEAM)
	{
		const int k = j % ns;
		double2 v[R];
#pragma unroll
		for (int r = 0; r < R; r++) v[r] = src[j + r * mr];
		if (ns > 1)
		{
#pragma unroll
			for (int r = 1; r < R; r++) v[r] = edg_cmul(v[r], tw[k * r * tstep]);
		}
		edg_dft<R>(v);
		const int base = (j - k) * R + k;
#pragma unroll
		for (int q = 0; q < R; q++) dst[base + q * ns] = v[q];
	}
}

template <int TEAM> __global__ __launch_bounds__(EDG_BLOCK) void ed_mfcc_geom_kernel(ed_geom_args_t a)
{
#define EDG_STORE(i, y)                                                                        \
	{                                                                                          \
		const float v = fminf(fmaxf((float)(y) * a.feat_scale, -128.0f), 127.0f);            \
		a.feat[i] = (int8_t)rintf(v);                                                          \
	}
#include "mfcc_geom_frames.inc"
#undef EDG_STORE
}

/* The float64 instance (edison_mfcc_geom_batch*): the same frames and stages; stage 6 stores y itself, unscaled
 * and unrounded, to mfcc [n_frames][n_coef]. a.feat and a.feat_scale are not read. */
template <int TEAM> __global__ __launch_bounds__(EDG_BLOCK) void ed_mfcc_geom_f64_kernel(ed_geom_args_t a, double *mfcc)
{
#define EDG_STORE(i, y) mfcc[i] = (y);
#include "mfcc_geom_frames.inc"
#undef EDG_STORE
}

/* mfcc == NULL: ed_mfcc_geom_kernel (int8 features to a->feat); else ed_mfcc_geom_f64_kernel (y to mfcc) */
static int edg_launch(const ed_geom_args_t *a, double *mfcc, int n_cu, hipStream_t stream)
{
	if (a->n_frames <= 0) return 0;
	if (a->team != 64 && a->team != EDG_BLOCK) return (int)hipErrorInvalidValue;
	const int teams = EDG_BLOCK / a->team;
	const size_t lds = sizeof(double) * (size_t)teams * (size_t)(a->r0 + a->r1 + a->r2);
	if (a->team == 64 && lds > 4 * (size_t)EDG_WAVE_LDS_MAX) return (int)hipErrorInvalidValue;
	if (lds > 160 * 1024) return (int)hipErrorInvalidValue;
	const void *fn = !mfcc ? (a->team == 64 ? (const void *)ed_mfcc_geom_kernel<64> : (const void *)ed_mfcc_geom_kernel<EDG_BLOCK>)
	                       : (a->team == 64 ? (const void *)ed_mfcc_geom_f64_kernel<64> : (const void *)ed_mfcc_geom_f64_kernel<EDG_BLOCK>);
	{ const int e = ed_kernel_prepare(fn, EDG_BLOCK, lds, NULL, NULL); if (e) return e; }
	/* resident workgroups: as many as the LDS admits, at most 4 per CU (16 waves); the frames are grid-strided */
	int64_t per_cu = (int64_t)(160 * 1024) / (int64_t)lds;
	if (per_cu > 4) per_cu = 4;
	if (per_cu < 1) per_cu = 1;
	int64_t blocks = ((int64_t)a->n_frames + teams - 1) / teams;
	if (blocks > per_cu * n_cu) blocks = per_cu * n_cu;
	const dim3 grid((unsigned)blocks), block(EDG_BLOCK);
	if (mfcc)
	{
		if (a->team == 64) hipLaunchKernelGGL(ed_mfcc_geom_f64_kernel<64>, grid, block, lds, stream, *a, mfcc);
		else hipLaunchKernelGGL(ed_mfcc_geom_f64_kernel<EDG_BLOCK>, grid, block, lds, stream, *a, mfcc);
	}
	else if (a->team == 64) hipLaunchKernelGGL(ed_mfcc_geom_kernel<64>, grid, block, lds, stream, *a);
	else hipLaunchKernelGGL(ed_mfcc_geom_kernel<EDG_BLOCK>, grid, block, lds, stream, *a);
	return (int)hipGetLastError();
}

extern "C" int ed_launch_mfcc_geom(const ed_geom_args_t *a, int n_cu, hipStream_t stream) { return edg_launch(a, NULL, n_cu, stream); }

extern "C" int ed_launch_mfcc_geom_f64(const ed_geom_args_t *a, double *mfcc, int n_cu, hipStream_t stream)
{
	if (!mfcc) return (int)hipErrorInvalidValue;
	return edg_launch(a, mfcc, n_cu, stream);
}
