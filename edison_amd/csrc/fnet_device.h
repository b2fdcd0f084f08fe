/*
 * fnet_device.h -- the device code of every kernel that takes a tile of utterances through the float32 network in LDS. It exists once,
 * here, in named pieces:
 *   EDF_LDS_PLAN      the LDS pointers of a plan p
 *   edf_tile          the work item: the tiling, the k-ordered fmaf chain, the epilogue of bias, ReLU and pool, the per-layer dump;
 *                     its sink sees every value before ReLU (pre) and every pooled output (out)
 *   EDF_LAYER_WALK    one record by the whole workgroup: staging into LDS, the two syncs, the item loop, the nt and pad dispatch
 *   EDF_SOFTMAX       the softmax of one utterance and its first maximum
 *   EDF_NETWORK_BODY  the body of a forward kernel on those pieces
 * and, for networks that LDS cannot hold (the layer road, fnet_layer_kernels.hip), one record per launch:
 *   edf_layer_lds / edf_layer_fetch / edf_layer_tile   a workgroup's tile with its operands streamed through LDS in K chunks
 *   edf_layer_epilogue                                  edf_tile's epilogue restated (why: at the function)
 * ed_fnet_kernel and ed_fnet_windows_kernel (EDF_NETWORK_BODY, edf_no_sink) differ in how the utterances of a tile find their input;
 * ed_fnet_calib_kernel (fnet_calib_kernels.hip) walks with edfc_sink, its statistic in pre; ed_ftrain_grad_kernel
 * (fnet_grad_kernels.hip) expands the plan, the walk and the softmax over a work item of its own. The plan, the walk and the softmax are
 * textual and the tile is a function: DESIGN.md section 14 says why, and why the trainer keeps its work item.
 * DESIGN.md sections 14, 14b (padded records: PAD = true), 15a, 18 and 19. Not part of the public ABI.
 */
#ifndef EDISON_FNET_DEVICE_H
#define EDISON_FNET_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fnet.h"

typedef float ed_f4 __attribute__((ext_vector_type(4)));

/* A padded record's row m of the tile (fnet.h): its window origin and the offset of that origin in src. A row beyond M and an absent
 * row get y0 = in_h, which puts every tap outside the image: the lane reads nothing and multiplies zeros. */
__device__ __forceinline__ void edf_pad_row(const ed_fnet_layer_t &L, const int32_t *__restrict__ rowin, int src_n, int M, int m, int &base, int &y0, int &x0)
{
	base = 0; y0 = L.in_h; x0 = 0;
	if (m >= M) return;
	const int u = m / L.rows;
	const int32_t o = rowin[m - u * L.rows];
	if (o < 0) return;
	y0 = (o >> 16) - ED_FNET_ORIGIN_BIAS;
	x0 = (o & 0xffff) - ED_FNET_ORIGIN_BIAS;
	base = u * src_n + (y0 * L.in_w + x0) * L.in_c;
}

/* A padded record's A operand at k: the tap (y0 + ky, x0 + kx) where it lies inside the image, else +0.0f (the K padding has ko < 0). */
__device__ __forceinline__ float edf_pad_tap(const ed_fnet_layer_t &L, const float *__restrict__ src, int base, int y0, int x0, int32_t ko, int32_t kyx)
{
	const bool in = ko >= 0 && (unsigned)(y0 + (kyx >> 16)) < (unsigned)L.in_h && (unsigned)(x0 + (kyx & 0xffff)) < (unsigned)L.in_w;
	return in ? src[base + ko] : 0.0f;
}

/* Which of the lane's four output rows m0 .. m0 + 3 of a padded record are real: below M and not absent. */
__device__ __forceinline__ void edf_pad_live(const ed_fnet_layer_t &L, const int32_t *__restrict__ rowin, int M, int m0, bool live[4])
{
#pragma unroll
	for (int i = 0; i < 4; i++)
	{
		const int m = m0 + i;
		live[i] = m < M && rowin[m - m / L.rows * L.rows] >= 0;
	}
}

/* One work item: 16 output rows (M tile mt) x NT tiles of 16 channels starting at n0. PAD = false is a record without pads; PAD = true
 * reads the record's origins and kyx (kl + k_pad), gathers through edf_pad_tap and leaves absent rows out of the pool's max.
 * acts != NULL: every pooled output also goes to the per-layer dump of utterance u0 + u, acts_n floats per utterance. The dump is a
 * __restrict__ parameter and not a sink's member on purpose: as a member the forward kernels compile to other instructions and measured
 * 1.7 % slower.
 * The sink sees what a kernel wants beside that: sink.pre(v, real) every accumulator element after the bias add and before ReLU (real:
 * neither a padding row of the last M tile nor an absent one), sink.out(L, u, q, n, x, v) every pooled output x after its stores, with
 * the window's P elements v[0 .. P - 1] as the max saw them. */
template <int NT, bool PAD, class SINK>
__device__ __forceinline__ void edf_tile(const ed_fnet_layer_t &L, const float *__restrict__ src, int src_n, float *__restrict__ dst, int dst_n,
                                         const float *__restrict__ wl, const int32_t *__restrict__ kl, const int32_t *__restrict__ rowin,
                                         const float *__restrict__ bias, int M, int mt, int n0, int lane, float *__restrict__ acts,
                                         int64_t acts_n, int64_t u0, SINK &sink)
{
	const int r = lane & 15, kq = lane >> 4;
	const int m = mt * 16 + r;
	int base = 0;
	[[maybe_unused]] int y0 = 0, x0 = 0;
	if constexpr (PAD) edf_pad_row(L, rowin, src_n, M, m, base, y0, x0);
	else if (m < M)
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
		float a;
		if constexpr (PAD) a = edf_pad_tap(L, src, base, y0, x0, ko, kl[L.k_pad + k0 + kq]);
		else a = ko >= 0 ? src[base + ko] : 0.0f;
#pragma unroll
		for (int j = 0; j < NT; j++) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wp[j * 16], acc[j], 0, 0, 0);
		wp += 4 * L.n_pad;
	}
	/* D: lane holds rows 4 kq + i (i = 0..3) of channel n0 + 16 j + r */
	const int P = L.P;
	const int m0 = mt * 16 + 4 * kq;
	[[maybe_unused]] bool live[4];
	if constexpr (PAD) edf_pad_live(L, rowin, M, m0, live);
#pragma unroll
	for (int j = 0; j < NT; j++)
	{
		const int n = n0 + 16 * j + r;
		if (n >= L.out_c) continue; /* a padding channel: not seen, not written */
		const float b = bias[n];
		float v[4];
#pragma unroll
		for (int i = 0; i < 4; i++)
		{
			v[i] = acc[j][i] + b;
			if constexpr (PAD) sink.pre(v[i], live[i]);
			else sink.pre(v[i], m0 + i < M);
			if (L.relu) v[i] = fmaxf(v[i], 0.0f);
			if constexpr (PAD) { if (!live[i]) v[i] = -INFINITY; } /* absent: the max's identity; its window has a real element */
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
			sink.out(L, u, q, n, x, v + g);
		}
	}
}

/* The sink of a kernel that wants nothing beside the tile's outputs: the forward kernels'. */
struct edf_no_sink
{
	__device__ __forceinline__ void pre(float, bool) {}
	__device__ __forceinline__ void out(const ed_fnet_layer_t &, int, int, int, float, const float *) {}
};

/* The plan's LDS, declared in a kernel whose plan is p (by value, or a reference into device memory): two activation buffers of
 * p.batch utterances each, the record's weights wl, its k tables kl; and the thread's place in the workgroup. */
#define EDF_LDS_PLAN                                                                                                                       \
	extern __shared__ float lds[];                                                                                                         \
	const int B = p.batch;                                                                                                                 \
	float *buf[2] = {lds, lds + B * p.buf_n[0]};                                                                                           \
	float *wl = lds + B * (p.buf_n[0] + p.buf_n[1]);                                                                                       \
	int32_t *kl = (int32_t *)(wl + p.w_lds);                                                                                               \
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = ED_FNET_THREADS / 64;

/* One work item of a walk: its nt <= 4 channel tiles pick the instantiation. */
template <bool PAD, class SINK>
__device__ __forceinline__ void edf_item(int nt, const ed_fnet_layer_t &L, const float *__restrict__ src, int src_n, float *__restrict__ dst, int dst_n,
                                         const float *__restrict__ wl, const int32_t *__restrict__ kl, const int32_t *__restrict__ rowin,
                                         const float *__restrict__ bias, int M, int mt, int n0, int lane, float *__restrict__ acts,
                                         int64_t acts_n, int64_t u0, SINK &sink)
{
	if (nt == 4) edf_tile<4, PAD>(L, src, src_n, dst, dst_n, wl, kl, rowin, bias, M, mt, n0, lane, acts, acts_n, u0, sink);
	else if (nt == 3) edf_tile<3, PAD>(L, src, src_n, dst, dst_n, wl, kl, rowin, bias, M, mt, n0, lane, acts, acts_n, u0, sink);
	else if (nt == 2) edf_tile<2, PAD>(L, src, src_n, dst, dst_n, wl, kl, rowin, bias, M, mt, n0, lane, acts, acts_n, u0, sink);
	else edf_tile<1, PAD>(L, src, src_n, dst, dst_n, wl, kl, rowin, bias, M, mt, n0, lane, acts, acts_n, u0, sink);
}

/* The walk of one record L by the whole workgroup: nu utterances from buf[L.src] to buf[L.dst], every work item through
 * ITEM<pad>(nt, ..., acts, acts_n, u0, sink): edf_item, or a kernel's own with that signature. Expanded behind EDF_LDS_PLAN where nu is in
 * scope. PADS is a constant: false leaves the padded instantiations out of a kernel that refuses padded records. The first __syncthreads
 * stands behind everything the kernel did since its last walk. */
#define EDF_LAYER_WALK(PADS, ITEM, L, acts, acts_n, u0, sink)                                                                              \
	{                                                                                                                                      \
		const float *gw = p.w + (L).w_at;                                                                                                  \
		__syncthreads(); /* the previous layer's outputs are written and its weights no longer read */                                     \
		{                                                                                                                                  \
			const int nw = (L).k_pad * (L).n_pad; /* a multiple of 64: float4 copies */                                                    \
			const float4 *g4 = (const float4 *)gw;                                                                                         \
			float4 *l4 = (float4 *)wl;                                                                                                     \
			for (int i = tid; i < nw / 4; i += ED_FNET_THREADS) l4[i] = g4[i];                                                             \
			const int nk = (PADS) && (L).pad ? 2 * (L).k_pad : (L).k_pad; /* a padded record: kyx behind koff */                           \
			for (int i = tid; i < nk; i += ED_FNET_THREADS) kl[i] = p.tab[(L).koff_at + i];                                                \
		}                                                                                                                                  \
		__syncthreads();                                                                                                                   \
		const float *src = buf[(L).src];                                                                                                   \
		float *dst = buf[(L).dst];                                                                                                         \
		const int src_n = p.buf_n[(L).src], dst_n = p.buf_n[(L).dst];                                                                      \
		const int32_t *rowin = p.tab + (L).rowin_at;                                                                                       \
		const float *bias = gw + (int64_t)(L).k_pad * (L).n_pad;                                                                           \
		const int M = nu * (L).rows;                                                                                                       \
		const int MT = (M + 15) / 16, NT = (L).n_pad / 16, NG = (NT + 3) / 4;                                                              \
		for (int item = wave; item < MT * NG; item += n_waves)                                                                             \
		{                                                                                                                                  \
			const int mt = item / NG, g = item - mt * NG;                                                                                  \
			const int n0 = g * 64, nt = NT - 4 * g < 4 ? NT - 4 * g : 4;                                                                   \
			if ((PADS) && (L).pad)                                                                                                         \
			{                                                                                                                              \
				if constexpr (PADS) ITEM<true>(nt, L, src, src_n, dst, dst_n, wl, kl, rowin, bias, M, mt, n0, lane, acts, acts_n, u0, sink); \
			}                                                                                                                              \
			else ITEM<false>(nt, L, src, src_n, dst, dst_n, wl, kl, rowin, bias, M, mt, n0, lane, acts, acts_n, u0, sink);                 \
		}                                                                                                                                  \
	}

/* One utterance's softmax (forward_sm: exp(z - max) / sum) over the n_out logits at z: declares mx (the maximum), s (the sum of
 * exp(z - mx)) and best (the first maximum of the probabilities); the argument is the statement that takes probability pj of class j. */
#define EDF_SOFTMAX(z, n_out, ...)                                                                                                         \
	float mx = (z)[0];                                                                                                                     \
	for (int j = 1; j < (n_out); j++) mx = fmaxf(mx, (z)[j]);                                                                              \
	float s = 0.0f;                                                                                                                        \
	for (int j = 0; j < (n_out); j++) s += expf((z)[j] - mx);                                                                              \
	int best = 0;                                                                                                                          \
	float bp = -1.0f;                                                                                                                      \
	for (int j = 0; j < (n_out); j++)                                                                                                      \
	{                                                                                                                                      \
		const float pj = expf((z)[j] - mx) / s;                                                                                            \
		__VA_ARGS__                                                                                                                        \
		if (pj > bp) { bp = pj; best = j; }                                                                                                \
	}

/* The body of a kernel `(ed_fnet_plan_t p, ..., int64_t n, float *logits, float *probs, int32_t *argmax, float *acts)`: the workgroup of
 * blockIdx.x takes the tile of utterances u0 = blockIdx.x * batch .. u0 + nu - 1 of the launch's n through the network. The argument is
 * the kernel's own statement that puts utterance u0 + u's p.in_n input floats at buf[0] + u * p.buf_n[0] for u < nu (it sees p, buf, u0,
 * nu and tid); outputs go to rows u0 .. of logits / probs / argmax (NULL: not written) and, with acts, of the per-layer dump. */
#define EDF_NETWORK_BODY(...)                                                                                                              \
	EDF_LDS_PLAN                                                                                                                           \
	const int64_t u0 = (int64_t)blockIdx.x * B;                                                                                            \
	const int nu = (int)(n - u0 < B ? n - u0 : B);                                                                                         \
                                                                                                                                           \
	/* the network input of the tile's utterances into buffer 0 */                                                                         \
	__VA_ARGS__                                                                                                                            \
                                                                                                                                           \
	edf_no_sink sink;                                                                                                                      \
	for (int l = 0; l < p.n_layers; l++) EDF_LAYER_WALK(true, edf_item, p.L[l], acts, p.acts_n, u0, sink)                                  \
	__syncthreads();                                                                                                                       \
                                                                                                                                           \
	/* one thread per utterance */                                                                                                         \
	if (tid < nu)                                                                                                                          \
	{                                                                                                                                      \
		const ed_fnet_layer_t &L = p.L[p.n_layers - 1];                                                                                    \
		const float *z = buf[L.dst] + tid * p.buf_n[L.dst];                                                                                \
		const int64_t u = u0 + tid;                                                                                                        \
		EDF_SOFTMAX(z, p.n_out, if (logits) logits[u * p.n_out + j] = z[j]; if (probs) probs[u * p.n_out + j] = pj;)                       \
		if (argmax) argmax[u] = best;                                                                                                      \
	}

/* ---- the layer road (fnet_layer_kernels.hip): one record per launch, its operands streamed through LDS ------- */

/* A workgroup's LDS: the gathered A[MB][KC] and B[KC][NB] of one K chunk (row strides SA, SB), and per row of the M block what
 * edf_pad_row gives (a record without pads: its base, -1 for a row beyond M). */
struct edf_layer_lds
{
	float A[ED_FNET_LAYER_MB * ED_FNET_LAYER_SA];
	float B[ED_FNET_LAYER_KC * ED_FNET_LAYER_SB];
	int32_t rb[ED_FNET_LAYER_MB], ry[ED_FNET_LAYER_MB], rx[ED_FNET_LAYER_MB];
};
static_assert(sizeof(edf_layer_lds) == ED_FNET_LAYER_LDS_BYTES, "fnet.h's ED_FNET_LAYER_LDS_BYTES");
static_assert(ED_FNET_LAYER_MB == 16 * (ED_FNET_THREADS / 64) && ED_FNET_LAYER_KC == 64 && ED_FNET_LAYER_NB == 64, "the thread maps of edf_layer_fetch");

/* The thread's share of the K chunk at kc0, from global memory into registers: A[wave + 8 i][lane] for i < 16 -- the operand edf_tile
 * reads, +0.0f for K padding, for a tap outside the image and for a row that is absent or beyond M -- and B[(tid >> 4) + 32 i][4 (tid &
 * 15) ..] for i < 2, of the NT tiles at n0. */
template <int NT, bool PAD>
__device__ __forceinline__ void edf_layer_fetch(const ed_fnet_layer_t &L, const float *__restrict__ gw, const int32_t *__restrict__ koff,
                                                const float *__restrict__ src, const edf_layer_lds &S, int kc0, int n0, int tid, float (&pa)[16],
                                                float4 (&pb)[2])
{
	const int lane = tid & 63, wave = tid >> 6, k = kc0 + lane;
	int32_t ko = -1;
	[[maybe_unused]] int32_t kyx = 0;
	if (k < L.k_pad)
	{
		ko = koff[k];
		if constexpr (PAD) kyx = koff[L.k_pad + k];
	}
#pragma unroll
	for (int i = 0; i < 16; i++)
	{
		const int m = wave + 8 * i;
		if constexpr (PAD) pa[i] = edf_pad_tap(L, src, S.rb[m], S.ry[m], S.rx[m], ko, kyx);
		else
		{
			const int base = S.rb[m];
			pa[i] = ko >= 0 && base >= 0 ? src[base + ko] : 0.0f;
		}
	}
	const int c = 4 * (tid & 15);
#pragma unroll
	for (int i = 0; i < 2; i++)
	{
		const int kb = kc0 + (tid >> 4) + 32 * i;
		pb[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		if (kb < L.k_pad && c < 16 * NT) pb[i] = *(const float4 *)(gw + (int64_t)kb * L.n_pad + n0 + c);
	}
}

/* edf_tile's epilogue (above, "D: lane holds rows ..."), restated for the layer road without a sink: factored into one function that
 * both tiles call, the in-LDS kernels compiled to other instructions, so edf_tile keeps its text and this
 * follows it line by line. Keep the two alike. */
template <int NT, bool PAD>
__device__ __forceinline__ void edf_layer_epilogue(const ed_fnet_layer_t &L, const ed_f4 (&acc)[NT], float *__restrict__ dst, int dst_n,
                                                   const int32_t *__restrict__ rowin, const float *__restrict__ bias, int M, int mt, int n0, int r,
                                                   int kq, float *__restrict__ acts, int64_t acts_n, int64_t u0)
{
	const int P = L.P;
	const int m0 = mt * 16 + 4 * kq;
	[[maybe_unused]] bool live[4];
	if constexpr (PAD) edf_pad_live(L, rowin, M, m0, live);
#pragma unroll
	for (int j = 0; j < NT; j++)
	{
		const int n = n0 + 16 * j + r;
		if (n >= L.out_c) continue; /* a padding channel: not written */
		const float b = bias[n];
		float v[4];
#pragma unroll
		for (int i = 0; i < 4; i++)
		{
			v[i] = acc[j][i] + b;
			if (L.relu) v[i] = fmaxf(v[i], 0.0f);
			if constexpr (PAD) { if (!live[i]) v[i] = -INFINITY; } /* absent: the max's identity; its window has a real element */
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

/* One workgroup's tile of record L: the MB rows from blockIdx.x * MB of the launch's M = nu * rows (tiles straddle utterances; a dense
 * record's rows are the utterances), the NT tiles of 16 channels from n0. K is walked in chunks of KC by the whole workgroup and never
 * split: wave w holds the accumulators of rows 16 w .. 16 w + 15 in registers across the chunks and feeds them the same
 * mfma_f32_16x16x4f32 steps in the same k order as edf_tile, so every output is the same fmaf chain. The next chunk's operands are
 * fetched into registers before the current chunk's MFMAs and stored to LDS behind them. */
template <int NT, bool PAD>
__device__ __forceinline__ void edf_layer_tile(const ed_fnet_layer_t &L, const float *__restrict__ gw, const int32_t *__restrict__ tab,
                                               const float *__restrict__ src, int src_n, float *__restrict__ dst, int dst_n, int M, int n0,
                                               float *__restrict__ acts, int64_t acts_n, int64_t u0, edf_layer_lds &S)
{
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int r = lane & 15, kq = lane >> 4;
	const int mb0 = blockIdx.x * ED_FNET_LAYER_MB;
	const int32_t *koff = tab + L.koff_at, *rowin = tab + L.rowin_at;
	if (tid < ED_FNET_LAYER_MB)
	{
		const int m = mb0 + tid;
		int base = -1, y0 = 0, x0 = 0;
		if constexpr (PAD) edf_pad_row(L, rowin, src_n, M, m, base, y0, x0);
		else if (m < M)
		{
			const int u = m / L.rows;
			base = u * src_n + rowin[m - u * L.rows];
		}
		S.rb[tid] = base; S.ry[tid] = y0; S.rx[tid] = x0;
	}
	__syncthreads();
	ed_f4 acc[NT];
#pragma unroll
	for (int j = 0; j < NT; j++) acc[j] = (ed_f4){0.0f, 0.0f, 0.0f, 0.0f};
	const int mt = blockIdx.x * (ED_FNET_LAYER_MB / 16) + wave;
	const bool active = mt * 16 < M; /* a wave whose 16 rows lie beyond M stages and syncs, and computes nothing */
	const float *ap = S.A + (16 * wave + r) * ED_FNET_LAYER_SA + kq;
	const float *bp = S.B + kq * ED_FNET_LAYER_SB + r;
	float pa[16];
	float4 pb[2];
	edf_layer_fetch<NT, PAD>(L, gw, koff, src, S, 0, n0, tid, pa, pb);
	for (int kc0 = 0; kc0 < L.k_pad; kc0 += ED_FNET_LAYER_KC)
	{
		const int kc = L.k_pad - kc0 < ED_FNET_LAYER_KC ? L.k_pad - kc0 : ED_FNET_LAYER_KC; /* a multiple of 4 */
		__syncthreads(); /* the previous chunk's operands are no longer read */
#pragma unroll
		for (int i = 0; i < 16; i++) S.A[(wave + 8 * i) * ED_FNET_LAYER_SA + lane] = pa[i];
#pragma unroll
		for (int i = 0; i < 2; i++) *(float4 *)(S.B + ((tid >> 4) + 32 * i) * ED_FNET_LAYER_SB + 4 * (tid & 15)) = pb[i];
		__syncthreads();
		if (kc0 + ED_FNET_LAYER_KC < L.k_pad) edf_layer_fetch<NT, PAD>(L, gw, koff, src, S, kc0 + ED_FNET_LAYER_KC, n0, tid, pa, pb);
		if (active && kc == ED_FNET_LAYER_KC)
		{
#pragma unroll 4
			for (int kk = 0; kk < ED_FNET_LAYER_KC; kk += 4)
			{
				const float a = ap[kk];
#pragma unroll
				for (int j = 0; j < NT; j++)
					acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[kk * ED_FNET_LAYER_SB + 16 * j], acc[j], 0, 0, 0);
			}
		}
		else if (active) /* the last chunk of a k_pad that is no multiple of KC: the same steps, a run-time count */
		{
			for (int kk = 0; kk < kc; kk += 4)
			{
				const float a = ap[kk];
#pragma unroll
				for (int j = 0; j < NT; j++)
					acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[kk * ED_FNET_LAYER_SB + 16 * j], acc[j], 0, 0, 0);
			}
		}
	}
	if (active)
		edf_layer_epilogue<NT, PAD>(L, acc, dst, dst_n, rowin, gw + (int64_t)L.k_pad * L.n_pad, M, mt, n0, r, kq, acts, acts_n, u0);
}

#endif
