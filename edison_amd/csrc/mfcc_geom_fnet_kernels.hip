/*
 * mfcc_geom_fnet_kernels.hip -- audio -> float32 network-input rows at ANY MFCC geometry: the feature stage of edison_stream_float's host
 * flow (edison_float_bank.hip). The third instance of the any-geometry frame body (mfcc_geom_frames.inc), beside
 * the int8 (ed_mfcc_geom_kernel) and float64 (ed_mfcc_geom_f64_kernel) instances of mfcc_geom_kernels.hip: the same frames, stages and
 * launch; stage 6 stores
 *     out[g * n_coef + row] = fminf(fmaxf((float)y * scale, lo), hi)
 * (with a.feat_utt_stride != 0: out[u * feat_utt_stride + f * n_coef + row], the stride in floats -- every utterance's rows in a buffer
 * of its own, the microphones of edison_float_bank.hip)
 * which is ed_mfcc_geom_f64_kernel followed by ed_fnet_input_kernel (fnet_kernels.hip) bit for bit, with no float64 scratch and one
 * launch fewer. a.feat and a.feat_scale are not read.
 */
#include "mfcc_geom_device.h"

template <int TEAM>
__global__ __launch_bounds__(EDG_BLOCK) void ed_mfcc_geom_fnet_kernel(ed_geom_args_t a, float *out, float scale, float lo, float hi)
{
	/* what utterance u's rows lie behind their contiguous place, in floats (u = the frame loop's utterance index); 0 for feat_utt_stride = 0 */
	const int64_t feat_skip = a.feat_utt_stride ? a.feat_utt_stride - (int64_t)a.frames_per_utt * a.n_coef : 0;
#define EDG_STORE(i, y) out[(i) + feat_skip * u] = fminf(fmaxf((float)(y) * scale, lo), hi);
#include "mfcc_geom_frames.inc"
#undef EDG_STORE
}

extern "C" int ed_launch_mfcc_geom_fnet(const ed_geom_args_t *a, float *out, float scale, float lo, float hi, int n_cu, hipStream_t stream)
{
	if (a->n_frames <= 0) return 0;
	if (!out) return (int)hipErrorInvalidValue;
	size_t lds = 0;
	dim3 grid;
	{ const int e = edg_launch_shape(a, n_cu, &lds, &grid); if (e) return e; }
	const void *fn = a->team == 64 ? (const void *)ed_mfcc_geom_fnet_kernel<64> : (const void *)ed_mfcc_geom_fnet_kernel<EDG_BLOCK>;
	{ const int e = ed_kernel_prepare(fn, EDG_BLOCK, lds, NULL, NULL); if (e) return e; }
	if (a->team == 64) hipLaunchKernelGGL(ed_mfcc_geom_fnet_kernel<64>, grid, dim3(EDG_BLOCK), lds, stream, *a, out, scale, lo, hi);
	else hipLaunchKernelGGL(ed_mfcc_geom_fnet_kernel<EDG_BLOCK>, grid, dim3(EDG_BLOCK), lds, stream, *a, out, scale, lo, hi);
	return (int)hipGetLastError();
}
