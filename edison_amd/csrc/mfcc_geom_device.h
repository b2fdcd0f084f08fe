/*
 * mfcc_geom_device.h -- the device helpers of the any-geometry MFCC frame body (mfcc_geom_frames.inc) and the launch shape every
 * instance of it shares: included by mfcc_geom_kernels.hip (the int8 and float64 instances) and mfcc_geom_fnet_kernels.hip (the
 * float network-input instance). Not part of the public ABI.
 */
#ifndef EDISON_MFCC_GEOM_DEVICE_H
#define EDISON_MFCC_GEOM_DEVICE_H

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

/* The launch of an instance for the frames of *a: workgroups of EDG_BLOCK threads, EDG_BLOCK / a->team teams each, *lds dynamic bytes;
 * as many resident workgroups as the LDS admits, at most 4 per CU (16 waves); the frames are grid-strided. Returns a hipError_t. */
static inline int edg_launch_shape(const ed_geom_args_t *a, int n_cu, size_t *lds, dim3 *grid)
{
	if (a->team != 64 && a->team != EDG_BLOCK) return (int)hipErrorInvalidValue;
	const int teams = EDG_BLOCK / a->team;
	*lds = sizeof(double) * (size_t)teams * (size_t)(a->r0 + a->r1 + a->r2);
	if (a->team == 64 && *lds > 4 * (size_t)EDG_WAVE_LDS_MAX) return (int)hipErrorInvalidValue;
	if (*lds > 160 * 1024) return (int)hipErrorInvalidValue;
	int64_t per_cu = (int64_t)(160 * 1024) / (int64_t)*lds;
	if (per_cu > 4) per_cu = 4;
	if (per_cu < 1) per_cu = 1;
	int64_t blocks = ((int64_t)a->n_frames + teams - 1) / teams;
	if (blocks > per_cu * n_cu) blocks = per_cu * n_cu;
	*grid = dim3((unsigned)blocks);
	return 0;
}

#endif
