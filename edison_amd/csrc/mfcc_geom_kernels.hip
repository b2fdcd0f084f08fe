/*
 * mfcc_geom_kernels.hip -- audio -> int8 network input for MFCC variants A and B at ANY geometry the generality path accepts (frame_len
 * 4 .. 4096, mel_nbins 1 .. 256), batched over all frames of all utterances of a call: the feature stage of edison_kws_geom_batch*
 * (edison_kws_geom.hip). Float64 throughout, as the reference computes (mfcc_utils.py:134-199 `mfcc`, :255-323 `mfcc_mcu`), so the int8
 * features are the reference host flow's. Per frame:
 *   1. load: N even -- z[n] = x[2n] + i x[2n+1], n < M = N/2 (the real frame packed into complex pairs); N odd -- z[n] = x[n], M = N
 *   2. Stockham FFT over M points in LDS, radix 4 / 2 / 3 / 5 stages ping-ponging between two buffers (self-sorting: natural order in
 *      and out); twiddles W_M^j = W_N^(j N / M) from the host-built table of W_N^j
 *      -- or, when M has a prime factor above 5 (441, 882, ...), a direct DFT of the real frame against the same table (N^2/2 fma)
 *   3. N even: real split X[k] = (Z[k] + conj Z[M-k]) / 2 - i W_N^k (Z[k] - conj Z[M-k]) / 2, k = 0 .. N/2
 *   4. spectrum s[k] = |X[k] * fft_scale| * spec_scale for the variant's n_bins bins (A: N/2 bins, 1, 1; B: N/2 + 1 bins, 1/1024, 1/sqrt 2)
 *   5. mel: band j = sum of its nonzero run of the filterbank in ascending k, / mel_div; ln(x + 1e-6) for A and B with use_log
 *   6. DCT-II rows first_mfcc .. first_mfcc + num_mfcc - 1 over dct_div (A sqrt(2 mel_nbins), B 64); feature = int8 of
 *      rint(clip((float)y * feat_scale, -128, 127)) (kws_nnom.py:359-361), written to feat + g * num_mfcc + row (utterance u's rows
 *      to feat + u * feat_utt_stride where that stride is given)
 *      -- or, in the float64 instance (ed_mfcc_geom_f64_kernel, edison_mfcc_geom_batch*), y itself to mfcc + g * num_mfcc + row
 *      -- or, in the float network-input instance (mfcc_geom_fnet_kernels.hip, edison_stream_float), min(max((float)y * scale, lo), hi)
 *
 * Work split: a TEAM of threads owns one frame at a time and a private LDS slice of r0 + r1 + r2 doubles (two FFT buffers -- the
 * spectrum goes to the one the FFT's result is not in -- and the mel bands); teams take frames g = team, team + n_teams, ... of the
 * whole call. TEAM = 64 (a wavefront; four per workgroup, no workgroup barrier) where the slice is at most 20 KiB, which covers every
 * even N <= 1024 and mel_nbins <= 256; TEAM = 256 (the workgroup) for the longer frames.
 */
#include "mfcc_geom_device.h"

template <int TEAM> __global__ __launch_bounds__(EDG_BLOCK) void ed_mfcc_geom_kernel(ed_geom_args_t a)
{
	/* what utterance u's rows lie behind their contiguous place (u = the frame loop's utterance index); 0 for feat_utt_stride = 0 */
	const int64_t feat_skip = a.feat_utt_stride ? a.feat_utt_stride - (int64_t)a.frames_per_utt * a.n_coef : 0;
#define EDG_STORE(i, y)                                                                        \
	{                                                                                          \
		const float v = fminf(fmaxf((float)(y) * a.feat_scale, -128.0f), 127.0f);            \
		a.feat[(i) + feat_skip * u] = (int8_t)rintf(v);                                        \
	}
#include "mfcc_geom_frames.inc"
#undef EDG_STORE
}

/* The float64 instance (edison_mfcc_geom_batch*): the same frames and stages; stage 6 stores y itself, unscaled
 * and unrounded, to mfcc [n_frames][n_coef]. a.feat and a.feat_scale are not read. */
template <int TEAM> __global__ __launch_bounds__(EDG_BLOCK) void ed_mfcc_geom_f64_kernel(ed_geom_args_t a, double *mfcc)
{
#define EDG_STORE(i, y) mfcc[i] = (y);
#include "mfcc_geom_frames.inc"
#undef EDG_STORE
}

/* mfcc == NULL: ed_mfcc_geom_kernel (int8 features to a->feat); else ed_mfcc_geom_f64_kernel (y to mfcc) */
static int edg_launch(const ed_geom_args_t *a, double *mfcc, int n_cu, hipStream_t stream)
{
	if (a->n_frames <= 0) return 0;
	size_t lds = 0;
	dim3 grid;
	{ const int e = edg_launch_shape(a, n_cu, &lds, &grid); if (e) return e; }
	const void *fn = !mfcc ? (a->team == 64 ? (const void *)ed_mfcc_geom_kernel<64> : (const void *)ed_mfcc_geom_kernel<EDG_BLOCK>)
	                       : (a->team == 64 ? (const void *)ed_mfcc_geom_f64_kernel<64> : (const void *)ed_mfcc_geom_f64_kernel<EDG_BLOCK>);
	{ const int e = ed_kernel_prepare(fn, EDG_BLOCK, lds, NULL, NULL); if (e) return e; }
	const dim3 block(EDG_BLOCK);
	if (mfcc)
	{
		if (a->team == 64) hipLaunchKernelGGL(ed_mfcc_geom_f64_kernel<64>, grid, block, lds, stream, *a, mfcc);
		else hipLaunchKernelGGL(ed_mfcc_geom_f64_kernel<EDG_BLOCK>, grid, block, lds, stream, *a, mfcc);
	}
	else if (a->team == 64) hipLaunchKernelGGL(ed_mfcc_geom_kernel<64>, grid, block, lds, stream, *a);
	else hipLaunchKernelGGL(ed_mfcc_geom_kernel<EDG_BLOCK>, grid, block, lds, stream, *a);
	return (int)hipGetLastError();
}

extern "C" int ed_launch_mfcc_geom(const ed_geom_args_t *a, int n_cu, hipStream_t stream) { return edg_launch(a, NULL, n_cu, stream); }

extern "C" int ed_launch_mfcc_geom_f64(const ed_geom_args_t *a, double *mfcc, int n_cu, hipStream_t stream)
{
	if (!mfcc) return (int)hipErrorInvalidValue;
	return edg_launch(a, mfcc, n_cu, stream);
}
