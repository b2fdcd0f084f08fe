/*
 * fnet_layer_kernels.hip -- the layer road of the float32 network: a network whose weights or activations do
 * not fit the LDS beside each other (edison_fnet_load_ex, EDISON_FNET_LARGE) runs one launch per conv / dense record and one softmax
 * launch, chunk by chunk of utterances, between two activation buffers in device memory.
 *
 * ed_fnet_layer_kernel<PAD>: a workgroup (512 threads, 8 waves) owns MB = 128 rows x up to NB = 64 channels of the record's implicit
 * GEMM, M = all rows of the chunk's utterances (tiles straddle utterances; a dense record's M is the utterances themselves, so its
 * weights are read once per 128 utterances and not once per utterance). The grid is M blocks x channel groups; K is never split.
 * The workgroup walks K in chunks of KC = 64: B[KC][NB] and the gathered A[MB][KC] -- through the plan's koff / kyx / rowin tables,
 * +0.0f for K padding, taps outside the image and absent rows, exactly edf_pad_tap's operand -- go through registers into LDS while
 * the previous chunk's MFMAs run, and wave w feeds the accumulators of its 16 rows, which stay in registers across the chunks, the
 * same v_mfma_f32_16x16x4_f32 steps in the same k order as edf_tile (fnet_device.h). So every output is the same k-ordered fmaf
 * chain, then the same epilogue: bit for bit what ed_fnet_kernel gives, and what tests/fnet_exact.py and tests/fnet_pad.py compute.
 * LDS row strides: A KC + 2 (bank (2 r + kq) mod 32), B NB + 16 (bank (16 kq + r) mod 32): ds_read_b32 serves lanes 0 .. 31 and
 * 32 .. 63 in one cycle each from 32 banks, and both maps are one-to-one on either half.
 * ed_fnet_softmax_kernel: EDF_SOFTMAX, one thread per utterance, as the in-LDS kernels end.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fnet.h"
#include "fnet_device.h"

template <bool PAD>
__global__ __launch_bounds__(ED_FNET_THREADS) void ed_fnet_layer_kernel(ed_fnet_layer_t L, const float *__restrict__ w, const int32_t *__restrict__ tab,
                                                                          const float *__restrict__ src, int src_n, float *__restrict__ dst, int dst_n,
                                                                          int nu, float *__restrict__ acts, int64_t acts_n, int64_t u0)
{
	__shared__ edf_layer_lds S;
	const float *gw = w + L.w_at;
	const int M = nu * L.rows;
	const int n0 = blockIdx.y * ED_FNET_LAYER_NB;
	const int nt = L.n_pad / 16 - 4 * (int)blockIdx.y; /* channel tiles from n0 on; this group takes at most 4 */
	if (nt >= 4) edf_layer_tile<4, PAD>(L, gw, tab, src, src_n, dst, dst_n, M, n0, acts, acts_n, u0, S);
	else if (nt == 3) edf_layer_tile<3, PAD>(L, gw, tab, src, src_n, dst, dst_n, M, n0, acts, acts_n, u0, S);
	else if (nt == 2) edf_layer_tile<2, PAD>(L, gw, tab, src, src_n, dst, dst_n, M, n0, acts, acts_n, u0, S);
	else edf_layer_tile<1, PAD>(L, gw, tab, src, src_n, dst, dst_n, M, n0, acts, acts_n, u0, S);
}

__global__ __launch_bounds__(256) void ed_fnet_softmax_kernel(const float *__restrict__ zs, int z_n, int n_out, int nu, int64_t u0,
                                                               float *__restrict__ logits, float *__restrict__ probs, int32_t *__restrict__ argmax)
{
	const int t = blockIdx.x * 256 + threadIdx.x;
	if (t >= nu) return;
	const float *z = zs + (int64_t)t * z_n;
	const int64_t u = u0 + t;
	EDF_SOFTMAX(z, n_out, if (logits) logits[u * n_out + j] = z[j]; if (probs) probs[u * n_out + j] = pj;)
	if (argmax) argmax[u] = best;
}

extern "C" int ed_launch_fnet_layered(const ed_fnet_plan_t *p, const float *in, int64_t n, int64_t chunk, float *const ws[2], float *logits, float *probs,
                                      int32_t *argmax, float *acts, float *ms, hipStream_t stream)
{
	if (n <= 0) return 0;
	if (p->batch != 0 || p->n_layers < 1 || p->n_layers > ED_FNET_MAX_LAYERS || chunk < 1) return (int)hipErrorInvalidValue;
	hipEvent_t ev[ED_FNET_MAX_LAYERS + 2];
	const int n_ev = ms ? p->n_layers + 2 : 0;
	for (int i = 0; i < n_ev; i++)
	{
		const hipError_t e = hipEventCreate(&ev[i]);
		if (e != hipSuccess) { while (i--) (void)hipEventDestroy(ev[i]); return (int)e; }
	}
	if (ms) for (int l = 0; l <= p->n_layers; l++) ms[l] = 0.0f;
	hipError_t e = hipSuccess;
	for (int64_t u0 = 0; u0 < n && e == hipSuccess; u0 += chunk)
	{
		const int nu = (int)(n - u0 < chunk ? n - u0 : chunk);
		for (int l = 0; l < p->n_layers && e == hipSuccess; l++)
		{
			const ed_fnet_layer_t &L = p->L[l];
			/* the bounds the kernel's int indices rely on: the host side (edison_fnet.hip) sizes chunk so that they hold */
			if ((int64_t)nu * L.rows > INT32_MAX / 16 || (int64_t)nu * p->buf_n[0] > INT32_MAX || (int64_t)nu * p->buf_n[1] > INT32_MAX)
			{
				e = hipErrorInvalidValue;
				break;
			}
			const float *src = l == 0 ? in + u0 * p->in_n : ws[L.src];
			const int src_n = l == 0 ? p->in_n : p->buf_n[L.src];
			const int M = nu * L.rows;
			const dim3 grid((unsigned)((M + ED_FNET_LAYER_MB - 1) / ED_FNET_LAYER_MB), (unsigned)((L.n_pad + ED_FNET_LAYER_NB - 1) / ED_FNET_LAYER_NB));
			if (ms) (void)hipEventRecord(ev[l], stream);
			if (L.pad)
				hipLaunchKernelGGL(ed_fnet_layer_kernel<true>, grid, dim3(ED_FNET_THREADS), 0, stream, L, p->w, p->tab, src, src_n, ws[L.dst], p->buf_n[L.dst], nu,
				                   acts, (int64_t)p->acts_n, u0);
			else
				hipLaunchKernelGGL(ed_fnet_layer_kernel<false>, grid, dim3(ED_FNET_THREADS), 0, stream, L, p->w, p->tab, src, src_n, ws[L.dst], p->buf_n[L.dst], nu,
				                   acts, (int64_t)p->acts_n, u0);
			e = hipGetLastError();
		}
		if (e != hipSuccess) break;
		const ed_fnet_layer_t &Z = p->L[p->n_layers - 1];
		if (ms) (void)hipEventRecord(ev[p->n_layers], stream);
		hipLaunchKernelGGL(ed_fnet_softmax_kernel, dim3((unsigned)((nu + 255) / 256)), dim3(256), 0, stream, ws[Z.dst], p->buf_n[Z.dst], p->n_out, nu, u0, logits,
		                   probs, argmax);
		e = hipGetLastError();
		if (ms && e == hipSuccess)
		{
			(void)hipEventRecord(ev[p->n_layers + 1], stream);
			e = hipEventSynchronize(ev[p->n_layers + 1]);
			for (int l = 0; l <= p->n_layers && e == hipSuccess; l++)
			{
				float t = 0.0f;
				e = hipEventElapsedTime(&t, ev[l], ev[l + 1]);
				ms[l] += t;
			}
		}
	}
	for (int i = 0; i < n_ev; i++) (void)hipEventDestroy(ev[i]);
	return (int)e;
}
