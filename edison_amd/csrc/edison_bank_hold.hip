/*
 * edison_bank_hold.hip -- the hold kernel of a bank push that leaves microphones out (edison_stream_core.h, finish_push_present;
 * DESIGN.md section 15b), for both banks: edison_stream_bank.hip's int8 graph and edison_float_bank.hip's float32 network.
 *
 * The push has run the upload, the feature launch and the network over ALL microphones, so an absent microphone's buffers hold garbage
 * behind its history and the network's outputs hold garbage rows for it; pos is about to advance by n for everyone. The hold kernel
 * carries the absent microphone's history forward to the new pos and overwrites its rows; the core's filter kernel, given the mask,
 * writes an absent microphone's fill (edison_stream_core.hip). One workgroup per microphone, as the core's two kernels.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edison_stream_core.h"

/* `count` elements from p up by `by` elements. The destination lies ABOVE the source and overlaps it when by < count, so the rounds of
 * 256 run from the top down -- the mirror image of ed_stream_core_shift_kernel: every lane reads, the workgroup waits, every lane
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

void ed_bank_launch_hold(hipStream_t q, int n_mics, const ed_bank_hold_t *h)
{
	hipLaunchKernelGGL(ed_bank_hold_kernel, dim3(n_mics), dim3(256), 0, q, *h);
}
