/*
 * fnet_windows_kernels.hip -- the float32 X-CUBE-AI network over the windows of a bank of microphones (edison_float_bank.hip, DESIGN.md
 * section 15a): ed_fnet_kernel's workgroup (fnet_device.h's EDF_NETWORK_BODY: the one tile, walk, softmax and LDS plan) whose
 * utterances find their input by TWO strides. Utterance U of the launch is frame i = U / n_mics of microphone m = U % n_mics: its in_n
 * input floats start at in + m * mic_stride + i * frame_stride -- window i of the push in microphone m's sliding buffer, read in place --
 * and its outputs go to row U, the time-major order [n][n_mics] of every output of a bank. A tile of `batch` utterances may straddle
 * frames: the division is resolved once, for the tile's first utterance, and stepped from there.
 * No scratch memory, f32 subnormals kept, as fnet_kernels.hip.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edison_launch.h"
#include "fnet.h"
#include "fnet_device.h"

__global__ __launch_bounds__(ED_FNET_THREADS) void ed_fnet_windows_kernel(ed_fnet_plan_t p, const float *__restrict__ in, int64_t mic_stride,
                                                                            int32_t n_mics, int64_t frame_stride, int64_t n,
                                                                            float *__restrict__ logits, float *__restrict__ probs,
                                                                            int32_t *__restrict__ argmax)
{
	float *const acts = NULL; /* no per-layer dump: the bank has none */
	/* n < 2^31 (the launcher checks): the tile's first utterance in 32 bits, the others one step on */
	EDF_NETWORK_BODY(int32_t fi = (int32_t)u0 / n_mics, mi = (int32_t)u0 - fi * n_mics;
	for (int u = 0; u < nu; u++)
	{
		const float *__restrict__ w = in + mi * mic_stride + fi * frame_stride;
		for (int e = tid; e < p.in_n; e += ED_FNET_THREADS) buf[0][u * p.buf_n[0] + e] = w[e];
		if (++mi == n_mics) { mi = 0; fi++; }
	})
}

extern "C" int ed_launch_fnet_windows(const ed_fnet_plan_t *p, const float *in, int64_t mic_stride, int32_t n_mics, int64_t frame_stride, int32_t n,
                                      float *logits, float *probs, int32_t *argmax, int per_frame, hipStream_t stream)
{
	if (n <= 0 || n_mics <= 0) return 0;
	if (mic_stride < 0 || frame_stride < 0) return (int)hipErrorInvalidValue;
	const int64_t total = (int64_t)n * n_mics;
	if (total > INT32_MAX) return (int)hipErrorInvalidValue;
	if (per_frame)
	{
		/* tools/bench_float_bank.py's other leg: frame i's n_mics windows lie one stride apart, one ed_launch_fnet each */
		const size_t slab = (size_t)n_mics * (size_t)p->n_out;
		for (int i = 0; i < n; i++)
		{
			const int e = ed_launch_fnet(p, in + i * frame_stride, mic_stride, n_mics, logits ? logits + i * slab : NULL, probs ? probs + i * slab : NULL,
			                             argmax ? argmax + (size_t)i * n_mics : NULL, NULL, stream);
			if (e) return e;
		}
		return 0;
	}
	const size_t lds = ed_fnet_lds_bytes(p);
	if (!ed_fnet_plan_launchable(p, lds)) return (int)hipErrorInvalidValue;
	{ const int e = ed_kernel_prepare((const void *)ed_fnet_windows_kernel, ED_FNET_THREADS, lds, NULL, NULL); if (e) return e; }
	const int64_t blocks = (total + p->batch - 1) / p->batch;
	hipLaunchKernelGGL(ed_fnet_windows_kernel, dim3((unsigned)blocks), dim3(ED_FNET_THREADS), lds, stream, *p, in, mic_stride, n_mics, frame_stride,
	                   total, logits, probs, argmax);
	return (int)hipGetLastError();
}
