/*
 * fnet_kernels.hip -- a float32 X-CUBE-AI network (edison_amd/cube_import.py, .ednf) on the f32-input matrix cores: the Cube runtime's
 * forward_conv2d_nl_pool / forward_conv2d / forward_dense / forward_sm for a batch of utterances (edison_fnet.hip).
 *
 * A workgroup (512 threads, 8 waves) owns a tile of `batch` utterances. Their activations live in LDS, in two buffers the layers
 * ping-pong between; the network input is loaded into buffer 0. Per layer the workgroup streams that layer's weights into LDS (the
 * largest layers are 72 KB: all of them would not fit beside the activations) and runs it as an implicit GEMM on
 * v_mfma_f32_16x16x4_f32: M = output rows of all utterances of the tile, N = output channels, K = kh * kw * in_c. Lane l of a wave
 * holds A[row l & 15][k l >> 4] -- the input element at the row's window origin (rowin, per row) plus the k-th window offset (koff,
 * per k, -1 in the padding) -- and B[k l >> 4][channel l & 15] from the layer's [k_pad][n_pad] weights. Exact f32: each output is the
 * k-ordered fmaf chain acc = fmaf(a_k, w_k, acc) from acc = +0.0f over k = 0 .. K - 1, subnormals kept; then one f32 bias add, fmaxf
 * ReLU and fmaxf pool. tests/fnet_exact.py models exactly that and the tests hold every layer to it bit for bit (DESIGN.md section 14,
 * tests/fnet_sweep.py). The epilogue adds the bias, applies ReLU and max-pools over the
 * P adjacent rows of each window (all in one lane's accumulator registers), then writes the pooled value to the other buffer. After
 * the last layer, one thread per utterance computes softmax = exp(z - max) / sum and the first maximum.
 * A record with a conv or a pool pad ('same' layers, .ednf version 2) takes the tile function's PAD = true
 * instantiation: rowin holds the window's origin, a second k table (ky, kx), and a tap outside the image is the operand +0.0f of the
 * same chain; an element of a pool window outside the conv's map is -inf in the max. Records without pads run PAD = false.
 * No scratch memory: everything is registers and LDS.
 * All of that is fnet_device.h's text (the LDS plan, the tile, the walk, the softmax), which the bank's, the calibrator's and the
 * trainer's kernels expand too; this kernel's own is the statement that loads a tile's inputs.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edison_launch.h"
#include "fnet.h"
#include "fnet_device.h"

__global__ __launch_bounds__(ED_FNET_THREADS) void ed_fnet_kernel(ed_fnet_plan_t p, const float *__restrict__ in, int64_t in_stride, int64_t n,
                                                                    float *__restrict__ logits,
                                                                    float *__restrict__ probs, int32_t *__restrict__ argmax, float *__restrict__ acts)
{
	/* utterance u starts in_stride floats after u - 1 (in_n: back to back; less: overlapping windows, edison_stream_float) */
	EDF_NETWORK_BODY(for (int i = tid; i < nu * p.in_n; i += ED_FNET_THREADS) {
		const int u = i / p.in_n, e = i - u * p.in_n;
		buf[0][u * p.buf_n[0] + e] = in[(u0 + u) * in_stride + e];
	})
}

extern "C" int ed_launch_fnet(const ed_fnet_plan_t *p, const float *in, int64_t in_stride, int64_t n, float *logits, float *probs, int32_t *argmax,
                              float *acts, hipStream_t stream)
{
	if (n <= 0) return 0;
	if (in_stride < 0) return (int)hipErrorInvalidValue;
	const size_t lds = ed_fnet_lds_bytes(p);
	if (!ed_fnet_plan_launchable(p, lds)) return (int)hipErrorInvalidValue;
	{ const int e = ed_kernel_prepare((const void *)ed_fnet_kernel, ED_FNET_THREADS, lds, NULL, NULL); if (e) return e; }
	const int64_t blocks = (n + p->batch - 1) / p->batch;
	if (blocks > INT32_MAX) return (int)hipErrorInvalidValue;
	hipLaunchKernelGGL(ed_fnet_kernel, dim3((unsigned)blocks), dim3(ED_FNET_THREADS), lds, stream, *p, in, in_stride, n, logits, probs, argmax, acts);
	return (int)hipGetLastError();
}

__global__ __launch_bounds__(256) void ed_fnet_input_kernel(const double *__restrict__ y, int64_t count, float scale, float lo, float hi, float *__restrict__ out)
{
	for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256)
		out[i] = fminf(fmaxf((float)y[i] * scale, lo), hi);
}

extern "C" int ed_launch_fnet_input(const double *y, int64_t count, float scale, float lo, float hi, float *out, int n_cu, hipStream_t stream)
{
	if (count <= 0) return 0;
	int64_t blocks = (count + 255) / 256;
	if (blocks > 8 * (int64_t)n_cu) blocks = 8 * (int64_t)n_cu;
	if (blocks < 1) blocks = 1;
	hipLaunchKernelGGL(ed_fnet_input_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, y, count, scale, lo, hi, out);
	return (int)hipGetLastError();
}
