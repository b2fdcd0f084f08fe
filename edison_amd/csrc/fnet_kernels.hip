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
 * No scratch memory: everything is registers and LDS.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edison_launch.h"
#include "fnet.h"

typedef float ed_f4 __attribute__((ext_vector_type(4)));

/* One work item: 16 output rows (M tile mt) x NT tiles of 16 channels starting at n0. */
template <int NT>
__device__ __forceinline__ void edf_tile(const ed_fnet_layer_t &L, const float *__restrict__ src, int src_n, float *__restrict__ dst, int dst_n,
                                         const float *__restrict__ wl, const int32_t *__restrict__ kl, const int32_t *__restrict__ rowin,
                                         const float *__restrict__ bias, int M, int mt, int n0, int lane, float *__restrict__ acts,
                                         int64_t acts_n, int64_t u0)
{
	const int r = lane & 15, kq = lane >> 4;
	const int m = mt * 16 + r;
	int base = 0;
	if (m < M)
	{
		const int u = m / L.rows;
		base = u * src_n + rowin[m - u * L.rows];
	}
	ed_f4 acc[NT];
#pragma unroll
	for (int j = 0; j < NT; j++) acc[j] = (ed_f4){0.0f, 0.0f, 0.0f, 0.0f};
	const float *wp = wl + kq * L.n_pad + n0 + r;
#pragma unroll 4
	for (int k0 = 0; k0 < L.k_pad; k0 += 4)
	{
		const int ko = kl[k0 + kq];
		const float a = ko >= 0 ? src[base + ko] : 0.0f;
#pragma unroll
		for (int j = 0; j < NT; j++) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wp[j * 16], acc[j], 0, 0, 0);
		wp += 4 * L.n_pad;
	}
	/* D: lane holds rows 4 kq + i (i = 0..3) of channel n0 + 16 j + r */
	const int P = L.P;
	const int m0 = mt * 16 + 4 * kq;
#pragma unroll
	for (int j = 0; j < NT; j++)
	{
		const int n = n0 + 16 * j + r;
		if (n >= L.out_c) continue;
		const float b = bias[n];
		float v[4];
#pragma unroll
		for (int i = 0; i < 4; i++)
		{
			v[i] = acc[j][i] + b;
			if (L.relu) v[i] = fmaxf(v[i], 0.0f);
		}
		for (int g = 0; g < 4; g += P)
		{
			const int mg = m0 + g;
			if (mg >= M) break;
			float x = v[g];
			if (P >= 2) x = fmaxf(x, v[g + 1]);
			if (P == 4) x = fmaxf(fmaxf(x, v[g + 2]), v[g + 3]);
			const int u = mg / L.rows, q = (mg - u * L.rows) / P;
			dst[u * dst_n + q * L.out_c + n] = x;
			if (acts) acts[(u0 + u) * acts_n + L.acts_at + q * L.out_c + n] = x;
		}
	}
}

__global__ __launch_bounds__(ED_FNET_THREADS) void ed_fnet_kernel(ed_fnet_plan_t p, const float *__restrict__ in, int64_t in_stride, int64_t n,
                                                                    float *__restrict__ logits,
                                                                    float *__restrict__ probs, int32_t *__restrict__ argmax, float *__restrict__ acts)
{
	extern __shared__ float lds[];
	const int B = p.batch;
	float *buf[2] = {lds, lds + B * p.buf_n[0]};
	float *wl = lds + B * (p.buf_n[0] + p.buf_n[1]);
	int32_t *kl = (int32_t *)(wl + p.w_lds);
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = ED_FNET_THREADS / 64;
	const int64_t u0 = (int64_t)blockIdx.x * B;
	const int nu = (int)(n - u0 < B ? n - u0 : B);

	/* the network input of the tile's utterances into buffer 0; utterance u starts in_stride floats after u - 1 (in_n: back to back;
	 * less: overlapping windows, edison_stream_float) */
	for (int i = tid; i < nu * p.in_n; i += ED_FNET_THREADS)
	{
		const int u = i / p.in_n, e = i - u * p.in_n;
		buf[0][u * p.buf_n[0] + e] = in[(u0 + u) * in_stride + e];
	}

	for (int l = 0; l < p.n_layers; l++)
	{
		const ed_fnet_layer_t &L = p.L[l];
		const float *gw = p.w + L.w_at;
		__syncthreads(); /* the previous layer's outputs are written and its weights no longer read */
		{
			const int nw = L.k_pad * L.n_pad; /* a multiple of 64: float4 copies */
			const float4 *g4 = (const float4 *)gw;
			float4 *l4 = (float4 *)wl;
			for (int i = tid; i < nw / 4; i += ED_FNET_THREADS) l4[i] = g4[i];
			for (int i = tid; i < L.k_pad; i += ED_FNET_THREADS) kl[i] = p.tab[L.koff_at + i];
		}
		__syncthreads();
		const float *src = buf[L.src];
		float *dst = buf[L.dst];
		const int src_n = p.buf_n[L.src], dst_n = p.buf_n[L.dst];
		const int32_t *rowin = p.tab + L.rowin_at;
		const float *bias = gw + (int64_t)L.k_pad * L.n_pad;
		const int M = nu * L.rows;
		const int MT = (M + 15) / 16, NT = L.n_pad / 16, NG = (NT + 3) / 4;
		for (int item = wave; item < MT * NG; item += n_waves)
		{
			const int mt = item / NG, g = item - mt * NG;
			const int n0 = g * 64, nt = NT - 4 * g < 4 ? NT - 4 * g : 4;
			if (nt == 4) edf_tile<4>(L, src, src_n, dst, dst_n, wl, kl, rowin, bias, M, mt, n0, lane, acts, p.acts_n, u0);
			else if (nt == 3) edf_tile<3>(L, src, src_n, dst, dst_n, wl, kl, rowin, bias, M, mt, n0, lane, acts, p.acts_n, u0);
			else if (nt == 2) edf_tile<2>(L, src, src_n, dst, dst_n, wl, kl, rowin, bias, M, mt, n0, lane, acts, p.acts_n, u0);
			else edf_tile<1>(L, src, src_n, dst, dst_n, wl, kl, rowin, bias, M, mt, n0, lane, acts, p.acts_n, u0);
		}
	}
	__syncthreads();

	/* softmax (forward_sm: exp(z - max) / sum) and the first maximum of the probabilities, one thread per utterance */
	if (tid < nu)
	{
		const ed_fnet_layer_t &L = p.L[p.n_layers - 1];
		const float *z = buf[L.dst] + tid * p.buf_n[L.dst];
		const int64_t u = u0 + tid;
		float mx = z[0];
		for (int j = 1; j < p.n_out; j++) mx = fmaxf(mx, z[j]);
		float s = 0.0f;
		for (int j = 0; j < p.n_out; j++) s += expf(z[j] - mx);
		int best = 0;
		float bp = -1.0f;
		for (int j = 0; j < p.n_out; j++)
		{
			const float pj = expf(z[j] - mx) / s;
			if (logits) logits[u * p.n_out + j] = z[j];
			if (probs) probs[u * p.n_out + j] = pj;
			if (pj > bp) { bp = pj; best = j; }
		}
		if (argmax) argmax[u] = best;
	}
}

extern "C" int ed_launch_fnet(const ed_fnet_plan_t *p, const float *in, int64_t in_stride, int64_t n, float *logits, float *probs, int32_t *argmax,
                              float *acts, hipStream_t stream)
{
	if (n <= 0) return 0;
	if (in_stride < 0) return (int)hipErrorInvalidValue;
	const size_t lds = ed_fnet_lds_bytes(p);
	if (lds > ED_FNET_LDS_BYTES || p->batch < 1 || p->n_layers < 1 || p->n_layers > ED_FNET_MAX_LAYERS) return (int)hipErrorInvalidValue;
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
