/*
 * fnet_grad_device.h -- the two MFMA work items of the float32 trainer's backward half, written once for the kernels that use them:
 * ed_ftrain_grad_kernel (fnet_grad_kernels.hip), which takes a tile through every record in one launch, and the
 * BatchNorm trainer's per-record backward launch (fnet_bn_kernels.hip). Both take every operand through a
 * pointer: dY and the row bases in LDS, the record's input, its weights and the gradient slab in global memory.
 * Not part of the public ABI.
 */
#ifndef EDISON_FNET_GRAD_DEVICE_H
#define EDISON_FNET_GRAD_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fnet.h"
#include "fnet_device.h"
#include "fnet_train.h"

/* dW of 16 k rows (k tile kt; kt == KT is the bias row: A = 1 in row 0) x NT tiles of 16 channels from n0, summed over the tile's M rows
 * four at a time in ascending order (rows beyond M multiply zeros), into the workgroup's slab. src: the record's input, utterance u at src + u * src_n.
 * PAD = false: rb[m] is row m's base in src. PAD = true: rb[2 m] is its utterance's base and rb[2 m + 1] its packed origin (fnet.h), -1
 * for an absent row and for a row beyond M; the lane's k is one tap (ky, kx) for the whole tile (kyx behind koff), read where
 * edf_pad_tap reads it: inside the image. The bias row needs neither: dY is +0.0f on absent rows. */
template <int NT, bool PAD>
__device__ __forceinline__ void edg_dw_tile(const ed_fnet_layer_t &L, int K, const float *__restrict__ src, const int32_t *__restrict__ koff,
                                            const float *__restrict__ dy, const int32_t *__restrict__ rb, int M, int kt, int KT, int n0, int lane,
                                            float *__restrict__ slab, bool first)
{
	const int r = lane & 15, kq = lane >> 4;
	const bool is_bias = kt == KT;
	const int k = kt * 16 + r;
	const int ko = !is_bias && k < K ? koff[k] : -1;
	[[maybe_unused]] int ky = 0, kx = 0;
	if constexpr (PAD)
	{
		const int32_t kyx = ko >= 0 ? koff[L.k_pad + k] : 0;
		ky = kyx >> 16;
		kx = kyx & 0xffff;
	}
	ed_f4 acc[NT];
#pragma unroll
	for (int j = 0; j < NT; j++) acc[j] = (ed_f4){0.0f, 0.0f, 0.0f, 0.0f};
	const float *dp = dy + kq * L.n_pad + n0 + r;
	/* 16 rows a turn, their operands loaded before the four MFMA steps that take them in order: dY is +0.0f up to the next multiple of 16 */
	for (int m0 = 0; m0 < M; m0 += 16)
	{
		float a[4], b[4][NT];
#pragma unroll
		for (int s = 0; s < 4; s++)
		{
			const int m = m0 + 4 * s + kq;
			if (is_bias) a[s] = r == 0 ? 1.0f : 0.0f;
			else if constexpr (PAD)
			{
				const int32_t o = rb[2 * m + 1]; /* m < the 16-padded M: the row-base array has it */
				const int y0 = (o >> 16) - ED_FNET_ORIGIN_BIAS, x0 = (o & 0xffff) - ED_FNET_ORIGIN_BIAS;
				const bool in = ko >= 0 && o >= 0 && (unsigned)(y0 + ky) < (unsigned)L.in_h && (unsigned)(x0 + kx) < (unsigned)L.in_w;
				a[s] = in ? src[rb[2 * m] + (y0 * L.in_w + x0) * L.in_c + ko] : 0.0f;
			}
			else a[s] = ko >= 0 && m < M ? src[rb[m] + ko] : 0.0f;
#pragma unroll
			for (int j = 0; j < NT; j++) b[s][j] = dp[4 * s * L.n_pad + j * 16];
		}
#pragma unroll
		for (int s = 0; s < 4; s++)
#pragma unroll
			for (int j = 0; j < NT; j++) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s][j], acc[j], 0, 0, 0);
		dp += 16 * L.n_pad;
	}
	/* D: lane holds k rows kt * 16 + 4 kq + i of channel n0 + 16 j + r */
	float *gw = slab + L.w_at;
#pragma unroll
	for (int j = 0; j < NT; j++)
	{
		const int n = n0 + 16 * j + r;
		if (n >= L.out_c) continue; /* a padding channel stays +0.0f */
		if (is_bias)
		{
			if (kq == 0)
			{
				float *o = gw + (int64_t)L.k_pad * L.n_pad + n;
				*o = first ? acc[j][0] : *o + acc[j][0];
			}
			continue;
		}
#pragma unroll
		for (int i = 0; i < 4; i++)
		{
			const int kk = kt * 16 + 4 * kq + i;
			if (kk >= K) continue; /* a padding k row stays +0.0f */
			float *o = gw + (int64_t)kk * L.n_pad + n;
			*o = first ? acc[j][i] : *o + acc[j][i];
		}
	}
}

/* dX of 16 (utterance, position) rows (tile mt of MX = nu * np) x 16 input channels from c0, into dprev: utterance u's gradient of the
 * record's input at dprev + u * acts_n, HWC. Taps in ascending order, channels four at a time; a tap no row of the tile has is skipped
 * (it would add +0.0f to every sum). w: the record's B[k_pad][n_pad] in global memory. */
__device__ __forceinline__ void edg_dx_tile(const ed_fnet_layer_t &L, const ed_ftrain_layer_t &G, const int32_t *__restrict__ inv,
                                            const float *__restrict__ w, const float *__restrict__ dy, int MX, int mt, int c0, int lane,
                                            float *__restrict__ dprev, int acts_n)
{
	const int r = lane & 15, kq = lane >> 4;
	const int m = mt * 16 + r;
	const bool real = m < MX;
	const int u = real ? m / G.np : 0, pos = real ? m - u * G.np : 0;
	const int ci = c0 + r;
	const int oc4 = (L.out_c + 3) & ~3;
	ed_f4 acc = (ed_f4){0.0f, 0.0f, 0.0f, 0.0f};
	for (int t = 0; t < G.T; t++)
	{
		const int row = real ? inv[pos * G.T + t] : -1;
		if (__ballot(row >= 0) == 0) continue;
		const float *dr = dy + (row >= 0 ? (u * L.rows + row) * L.n_pad : 0);
		const float *wr = w + (int64_t)(t * L.in_c + (ci < L.in_c ? ci : 0)) * L.n_pad;
		for (int n0 = 0; n0 < oc4; n0 += 4)
		{
			const int n = n0 + kq;
			const float a = row >= 0 ? dr[n] : 0.0f;
			const float b = ci < L.in_c && n < L.out_c ? wr[n] : 0.0f; /* the blob's padding channels are never read */
			acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
		}
	}
	if (ci >= L.in_c) return;
#pragma unroll
	for (int i = 0; i < 4; i++)
	{
		const int mm = mt * 16 + 4 * kq + i;
		if (mm >= MX) break;
		const int uu = mm / G.np, pp = mm - uu * G.np;
		dprev[uu * acts_n + pp * L.in_c + ci] = acc[i];
	}
}

#endif
