/*
 * edison_bank_hold.hip -- the two kernels of a bank push that leaves microphones out (edison_stream_core.h, finish_push_present;
 * DESIGN.md section 15b), for both banks: edison_stream_bank.hip's int8 graph and edison_float_bank.hip's float32 network.
 *
 * The push has run the upload, the feature launch and the network over ALL microphones, so an absent microphone's buffers hold garbage
 * behind its history and the network's outputs hold garbage rows for it; pos is about to advance by n for everyone. The hold kernel
 * carries the absent microphone's history forward to the new pos and overwrites its rows; the masked filter gives a present microphone
 * the banked filter's path and an absent one the fill. One workgroup per microphone, as the banked kernels of edison_stream_bank.hip.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edison_stream_core.h"

/* `count` elements from p up by `by` elements. The destination lies ABOVE the source and overlaps it when by < count, so the rounds of
 * 256 run from the top down -- the mirror image of ed_stream_bank_shift_kernel: every lane reads, the workgroup waits, every lane
 * writes. A write to element j + by clobbers source element j + by > j, which this round or an earlier one has already read. Called by
 * the whole workgroup. */
template <class E>
static __device__ void hold_up(E *p, int count, int64_t by, int t)
{
	for (int top = count; top > 0; top -= 256)
	{
		const int j = top - 1 - t;
		const E v = j >= 0 ? p[j] : (E)0;
		__syncthreads();
		if (j >= 0) p[by + j] = v;
		__syncthreads();
	}
}

/* Workgroup m, for a microphone with present[m] == 0 (the others return at once): its `tail` history samples and feat_bytes bytes of
 * history rows up by the push's advance, zero bytes into its rows of the network outputs, -1 into its argmax, n more frames missed. */
__global__ __launch_bounds__(256) void ed_bank_hold_kernel(ed_bank_hold_t h)
{
	const int t = threadIdx.x;
	const size_t m = blockIdx.x, n_mics = gridDim.x;
	if (h.present[m]) return;
	hold_up(h.audio + (int64_t)m * h.a_stride + h.a_src, h.tail, h.a_by, t);
	hold_up(h.feat + (int64_t)m * h.f_stride + h.f_src, h.feat_bytes, h.f_by, t);
	const size_t row = (size_t)h.row_bytes;
	for (size_t k = t; k < (size_t)h.n * row; k += 256)
	{
		const size_t at = (k / row * n_mics + m) * row + k % row;
		if (h.out0) h.out0[at] = 0;
		if (h.out1) h.out1[at] = 0;
	}
	if (h.argmax)
		for (int i = t; i < h.n; i += 256) h.argmax[i * n_mics + m] = -1;
	if (t == 0) h.missed[m] += h.n;
}

/* ed_stream_bank_filter_kernel (edison_stream_bank.hip) with a mask. A present microphone runs that kernel's body: product and sum
 * rounded separately in double, no contraction, first maximum, edisonFSM on lane 0. An absent one writes the fill -- zero bytes in its
 * rows of filt, -1 in likely and spotted, its machine's unchanged state in fs.states, the unchanged machine in fs.copy -- and leaves
 * state[m] and fs.fsm[m] alone. The body is repeated here, not shared: that file keeps its two kernels and its one pragma. */
template <class T>
__global__ __launch_bounds__(256) void ed_bank_filter_present_kernel(const unsigned char *present, const T *x, int n, int n_out, double alpha,
                                                                     double one_minus_alpha, double threshold, float *state, float *filt,
                                                                     int32_t *likely, int32_t *spotted, edsg_fsm_stage_t fs)
{
	const int t = threadIdx.x;
	const size_t m = blockIdx.x, n_mics = gridDim.x;
	if (!present[m])
	{
		for (size_t k = t; k < (size_t)n * n_out; k += 256) filt[(k / n_out * n_mics + m) * n_out + k % n_out] = 0.0f;
		for (int i = t; i < n; i += 256)
		{
			likely[i * n_mics + m] = -1;
			spotted[i * n_mics + m] = -1;
		}
		if (fs.fsm && t == 0)
		{
			const edison_fsm mach = fs.fsm[m];
			for (int i = 0; i < n; i++) fs.states[i * n_mics + m] = mach.state;
			if (fs.copy) fs.copy[m] = mach;
		}
		return;
	}
	if (t < n_out)
	{
		float y = state[m * n_out + t];
		for (int i = 0; i < n; i++)
		{
			/* the compiler's default contraction would fuse these into one v_fma_f64 (the Cortex-M4 rounds each operation) */
#pragma clang fp contract(off)
			const size_t at = (i * n_mics + m) * n_out + t;
			const double a = alpha * (double)y;
			const double b = one_minus_alpha * (double)x[at];
			y = (float)(a + b);
			filt[at] = y;
		}
		state[m * n_out + t] = y;
	}
	__syncthreads();
	for (int i = t; i < n; i += 256)
	{
		const size_t im = i * n_mics + m;
		const float *row = filt + im * n_out;
		float best = row[0];
		int idx = 0;
		for (int c = 1; c < n_out; c++)
			if (best < row[c]) { best = row[c]; idx = c; }
		likely[im] = idx;
		spotted[im] = ((double)best > threshold) ? idx : -1;
	}
	if (!fs.fsm) return;
	__syncthreads();
	if (t == 0)
	{
		edison_fsm mach = fs.fsm[m];
		for (int i = 0; i < n; i++)
		{
			const size_t im = i * n_mics + m;
			fs.states[im] = ed_fsm_step_core(&mach, spotted[im] >= 0, (uint32_t)likely[im], fs.dt_us, &fs.roles);
		}
		fs.fsm[m] = mach;
		if (fs.copy) fs.copy[m] = mach;
	}
}

void ed_bank_launch_hold(hipStream_t q, int n_mics, const ed_bank_hold_t *h)
{
	hipLaunchKernelGGL(ed_bank_hold_kernel, dim3(n_mics), dim3(256), 0, q, *h);
}

void ed_bank_launch_filter_present(hipStream_t q, int n_mics, const unsigned char *present, int out_elem, const void *x, int n, int n_out,
                                   double alpha, double one_minus_alpha, double threshold, float *state, float *filt, int32_t *likely,
                                   int32_t *spotted, edsg_fsm_stage_t fs)
{
	if (out_elem == 1)
		hipLaunchKernelGGL(ed_bank_filter_present_kernel<int8_t>, dim3(n_mics), dim3(256), 0, q, present, (const int8_t *)x, n, n_out, alpha,
		                   one_minus_alpha, threshold, state, filt, likely, spotted, fs);
	else
		hipLaunchKernelGGL(ed_bank_filter_present_kernel<float>, dim3(n_mics), dim3(256), 0, q, present, (const float *)x, n, n_out, alpha,
		                   one_minus_alpha, threshold, state, filt, likely, spotted, fs);
}
