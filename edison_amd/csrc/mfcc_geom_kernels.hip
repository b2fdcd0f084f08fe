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
	extern __shared__ __attribute__((aligned(16))) double edg_lds[];
	constexpr int TEAMS = EDG_BLOCK / TEAM;
	const int tid = TEAM == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
	const int team = TEAM == 64 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : 0;
	double *r0 = edg_lds + (size_t)team * (a.r0 + a.r1 + a.r2);
	double *r1 = r0 + a.r0, *mel = r1 + a.r1;
	const double2 *__restrict__ tw = reinterpret_cast<const double2 *>(a.tw);
	const int N = a.N, M = a.M, tws = a.packed ? 2 : 1;

	for (int g = blockIdx.x * TEAMS + team; g < a.n_frames; g += gridDim.x * TEAMS)
	{
		const int u = g / a.frames_per_utt, f = g - u * a.frames_per_utt;
		const int16_t *x = a.audio + (int64_t)u * a.utt_stride + (int64_t)f * a.frame_step;
		edg_sync<TEAM>(); /* the previous frame's DCT has read the mel bands */
		double *spec;
		if (M > 0)
		{
			/* ---- 1. load, 2. FFT */
			double2 *src = reinterpret_cast<double2 *>(r0), *dst = reinterpret_cast<double2 *>(r1);
			if (a.packed)
				for (int n = tid; n < M; n += TEAM) src[n] = make_double2((double)x[2 * n], (double)x[2 * n + 1]);
			else
				for (int n = tid; n < M; n += TEAM) src[n] = make_double2((double)x[n], 0.0);
			edg_sync<TEAM>();
			int ns = 1;
			for (int s = 0; s < a.n_stages; s++)
			{
				const int R = a.radix[s];
				if (R == 4) edg_stage<4, TEAM>(src, dst, M, ns, tws, tw, tid);
				else if (R == 2) edg_stage<2, TEAM>(src, dst, M, ns, tws, tw, tid);
				else if (R == 3) edg_stage<3, TEAM>(src, dst, M, ns, tws, tw, tid);
				else edg_stage<5, TEAM>(src, dst, M, ns, tws, tw, tid);
				edg_sync<TEAM>();
				double2 *t = src; src = dst; dst = t;
				ns *= R;
			}
			/* ---- 3. split, 4. spectrum: into the buffer the result is not in */
			spec = reinterpret_cast<double *>(dst);
			for (int k = tid; k < a.n_bins; k += TEAM)
			{
				double xr, xi;
				if (a.packed)
				{
					const double2 p = src[k < M ? k : k - M], q = src[k == 0 ? 0 : M - k]; /* Z[k mod M], Z[-k mod M] */
					const double er = 0.5 * (p.x + q.x), ei = 0.5 * (p.y - q.y);      /* E = (Z[k] + conj Z[-k]) / 2  */
					const double orr = 0.5 * (p.y + q.y), oi = -0.5 * (p.x - q.x);    /* O = (Z[k] - conj Z[-k]) / 2i */
					const double2 w = tw[k];
					xr = er + (orr * w.x - oi * w.y);
					xi = ei + (orr * w.y + oi * w.x);
				}
				else
				{
					xr = src[k].x;
					xi = src[k].y;
				}
				xr *= a.fft_scale;
				xi *= a.fft_scale;
				spec[k] = sqrt(xr * xr + xi * xi) * a.spec_scale;
			}
		}
		else
		{
			/* ---- 1. load, 2. direct DFT of the real frame: X[k] = sum_n x[n] W_N^(k n mod N), the index kept by addition */
			double *xs = r0;
			spec = r1;
			for (int n = tid; n < N; n += TEAM) xs[n] = (double)x[n];
			edg_sync<TEAM>();
			for (int k = tid; k < a.n_bins; k += TEAM)
			{
				double sr = 0.0, si = 0.0;
				int j = 0;
				for (int n = 0; n < N; n++)
				{
					const double v = xs[n];
					const double2 w = tw[j];
					sr = fma(v, w.x, sr);
					si = fma(v, w.y, si);
					j += k;
					if (j >= N) j -= N;
				}
				sr *= a.fft_scale;
				si *= a.fft_scale;
				spec[k] = sqrt(sr * sr + si * si) * a.spec_scale;
			}
		}
		edg_sync<TEAM>();

		/* ---- 5. mel bands over their nonzero taps, [ln] */
		for (int j = tid; j < a.n_mel; j += TEAM)
		{
			const int k0 = a.band[3 * j], len = a.band[3 * j + 1], off = a.band[3 * j + 2];
			double acc = 0.0;
			for (int t = 0; t < len; t++) acc = fma(spec[k0 + t], a.taps[off + t], acc);
			const double e = acc / a.mel_div;
			mel[j] = a.take_log ? log(e + 1e-6) : e;
		}
		edg_sync<TEAM>();

		/* ---- 6. DCT-II rows, the int8 feature */
		for (int c = tid; c < a.n_coef; c += TEAM)
		{
			const double *d = a.dct + (size_t)c * a.n_mel;
			double y = 0.0;
			for (int n = 0; n < a.n_mel; n++) y = fma(mel[n], d[n], y);
			y = y / a.dct_div;
			const float v = fminf(fmaxf((float)y * a.feat_scale, -128.0f), 127.0f);
			a.feat[(int64_t)g * a.n_coef + c] = (int8_t)rintf(v);
		}
	}
}

extern "C" int ed_launch_mfcc_geom(const ed_geom_args_t *a, int n_cu, hipStream_t stream)
{
	if (a->n_frames <= 0) return 0;
	if (a->team != 64 && a->team != EDG_BLOCK) return (int)hipErrorInvalidValue;
	const int teams = EDG_BLOCK / a->team;
	const size_t lds = sizeof(double) * (size_t)teams * (size_t)(a->r0 + a->r1 + a->r2);
	if (a->team == 64 && lds > 4 * (size_t)EDG_WAVE_LDS_MAX) return (int)hipErrorInvalidValue;
	if (lds > 160 * 1024) return (int)hipErrorInvalidValue;
	const void *fn = a->team == 64 ? (const void *)ed_mfcc_geom_kernel<64> : (const void *)ed_mfcc_geom_kernel<EDG_BLOCK>;
	{ const int e = ed_kernel_prepare(fn, EDG_BLOCK, lds, NULL, NULL); if (e) return e; }
	/* resident workgroups: as many as the LDS admits, at most 4 per CU (16 waves); the frames are grid-strided */
	int64_t per_cu = (int64_t)(160 * 1024) / (int64_t)lds;
	if (per_cu > 4) per_cu = 4;
	if (per_cu < 1) per_cu = 1;
	int64_t blocks = ((int64_t)a->n_frames + teams - 1) / teams;
	if (blocks > per_cu * n_cu) blocks = per_cu * n_cu;
	if (a->team == 64) hipLaunchKernelGGL(ed_mfcc_geom_kernel<64>, dim3((unsigned)blocks), dim3(EDG_BLOCK), lds, stream, *a);
	else hipLaunchKernelGGL(ed_mfcc_geom_kernel<EDG_BLOCK>, dim3((unsigned)blocks), dim3(EDG_BLOCK), lds, stream, *a);
	return (int)hipGetLastError();
}
