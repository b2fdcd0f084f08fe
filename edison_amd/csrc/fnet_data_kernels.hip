/*
 * fnet_data_kernels.hip -- the kernels of training from a device-resident data set (edison_ftrain_data_*, edison_ftrain_epoch; DESIGN.md
 * section 19d), and the Adadelta step. None of them is hot beside the gradient kernel: an epoch launches the gather once, the
 * reduction once and the step once a batch.
 *
 * ed_fdata_gather_kernel<V>: a workgroup copies one row of in_n floats at a time, V floats a lane and pass; its first lane copies the
 *   label. V = 4 needs in_n % 4 == 0, V = 2 in_n % 2 == 0: then every row of both arrays starts on a multiple of V floats (hipMalloc's
 *   base is aligned far beyond that). A row of 403 floats starts on no such multiple, so it moves float by float, which is still one
 *   coalesced 256-byte line a wave and instruction.
 * ed_fdata_reduce_kernel: one workgroup. Thread t sums rows t, t + 256, ... in double and counts its hits, then the 256 partial sums
 *   are added pairwise in LDS, (s[t] + s[t + 128]), (.. + 64), ...: the order of every addition is fixed by n alone. No atomics.
 * ed_ftrain_adadelta_kernel: elementwise over the packed array, float32, as ed_ftrain_step_kernel's Adam is.
 */
#include "fnet_data.h"

template <int V> struct ed_fdata_vec;
template <> struct ed_fdata_vec<1> { typedef float type; };
template <> struct ed_fdata_vec<2> { typedef float2 type; };
template <> struct ed_fdata_vec<4> { typedef float4 type; };

template <int V>
__global__ __launch_bounds__(256) void ed_fdata_gather_kernel(const float *__restrict__ src_x, const int32_t *__restrict__ src_y, const int32_t *__restrict__ order,
                                                               int64_t n, int32_t in_n, float *__restrict__ dst_x, int32_t *__restrict__ dst_y)
{
	typedef typename ed_fdata_vec<V>::type vec_t;
	const int nv = in_n / V; /* V divides in_n */
	for (int64_t i = blockIdx.x; i < n; i += gridDim.x)
	{
		const int64_t r = order[i];
		const vec_t *s = (const vec_t *)(src_x + r * in_n);
		vec_t *d = (vec_t *)(dst_x + i * in_n);
		for (int e = threadIdx.x; e < nv; e += 256) d[e] = s[e];
		if (threadIdx.x == 0) dst_y[i] = src_y[r];
	}
}

__global__ __launch_bounds__(256) void ed_fdata_reduce_kernel(const float *__restrict__ loss, const int32_t *__restrict__ argmax, const int32_t *__restrict__ labels,
                                                               int64_t n, ed_fdata_sums_t *__restrict__ out)
{
	__shared__ double s_sum[256];
	__shared__ long long s_hit[256];
	const int t = threadIdx.x;
	double sum = 0.0;
	long long hit = 0;
	for (int64_t i = t; i < n; i += 256)
	{
		sum += (double)loss[i];
		hit += argmax[i] == labels[i];
	}
	s_sum[t] = sum;
	s_hit[t] = hit;
	__syncthreads();
	for (int h = 128; h > 0; h >>= 1)
	{
		if (t < h)
		{
			s_sum[t] += s_sum[t + h];
			s_hit[t] += s_hit[t + h];
		}
		__syncthreads();
	}
	if (t == 0)
	{
		out->loss_sum = s_sum[0];
		out->hits = s_hit[0];
	}
}

__global__ __launch_bounds__(256) void ed_ftrain_adadelta_kernel(float *__restrict__ w, const float *__restrict__ g, float *__restrict__ a, float *__restrict__ d,
                                                                  int64_t count, float lr, float rho, float omr, float eps)
{
	const int64_t stride = (int64_t)gridDim.x * 256;
	for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += stride)
	{
		const float gi = g[i];
		const float ai = rho * a[i] + omr * gi * gi;
		const float ui = gi * sqrtf(d[i] + eps) / sqrtf(ai + eps);
		a[i] = ai;
		w[i] -= lr * ui;
		d[i] = rho * d[i] + omr * ui * ui;
	}
}

extern "C" int ed_launch_fdata_gather(const float *src_x, const int32_t *src_y, const int32_t *order, int64_t n, int32_t in_n, float *dst_x, int32_t *dst_y,
                                      int n_cu, hipStream_t stream)
{
	if (n <= 0) return 0;
	if (in_n < 1) return (int)hipErrorInvalidValue;
	const int64_t cap = (int64_t)(n_cu > 0 ? n_cu : 1) * 8;
	const dim3 grid((unsigned)(n < cap ? n : cap)), block(256);
	if (in_n % 4 == 0) hipLaunchKernelGGL(ed_fdata_gather_kernel<4>, grid, block, 0, stream, src_x, src_y, order, n, in_n, dst_x, dst_y);
	else if (in_n % 2 == 0) hipLaunchKernelGGL(ed_fdata_gather_kernel<2>, grid, block, 0, stream, src_x, src_y, order, n, in_n, dst_x, dst_y);
	else hipLaunchKernelGGL(ed_fdata_gather_kernel<1>, grid, block, 0, stream, src_x, src_y, order, n, in_n, dst_x, dst_y);
	return (int)hipGetLastError();
}

extern "C" int ed_launch_fdata_reduce(const float *loss, const int32_t *argmax, const int32_t *labels, int64_t n, ed_fdata_sums_t *out, hipStream_t stream)
{
	if (n < 0) return (int)hipErrorInvalidValue;
	hipLaunchKernelGGL(ed_fdata_reduce_kernel, dim3(1), dim3(256), 0, stream, loss, argmax, labels, n, out);
	return (int)hipGetLastError();
}

extern "C" int ed_launch_ftrain_adadelta(float *w, const float *g, float *a, float *d, int64_t count, float lr, float rho, float omr, float eps, int n_cu,
                                         hipStream_t stream)
{
	if (count <= 0) return 0;
	int64_t blocks = (count + 255) / 256;
	const int64_t cap = (int64_t)(n_cu > 0 ? n_cu : 1) * 8;
	if (blocks > cap) blocks = cap;
	hipLaunchKernelGGL(ed_ftrain_adadelta_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, w, g, a, d, count, lr, rho, omr, eps);
	return (int)hipGetLastError();
}
