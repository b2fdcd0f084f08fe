/*
 * mfcc_geom.h -- launch arguments of the audio -> network-input kernel for any MFCC geometry (mfcc_geom_kernels.hip), shared with
 * its host side (edison_kws_geom.hip). Not part of the public ABI.
 */
#ifndef EDISON_MFCC_GEOM_H
#define EDISON_MFCC_GEOM_H

#include <hip/hip_runtime.h>
#include <stdint.h>

/* ---- audio -> network input at any MFCC geometry (mfcc_geom_kernels.hip, edison_kws_geom.hip) ------------
 * Variants A / B, float64 throughout. Frame g of the call is frame f = g % frames_per_utt of utterance u = g / frames_per_utt: its
 * samples start at audio + u * utt_stride + f * frame_step, its int8 features land at feat + g * n_coef (the flat [frames][num_mfcc]
 * vector the reference reshapes to the graph's input) -- or, with feat_utt_stride != 0, at feat + u * feat_utt_stride + f * n_coef:
 * every utterance's rows in a buffer of its own (the microphones of edison_stream_bank.hip and edison_float_bank.hip; the unit is the
 * instance's output element: bytes for the int8 features, floats for ed_launch_mfcc_geom_fnet's rows). The transform is a Stockham FFT over M complex points with the radices in
 * `radix` (M = N/2 with the real frame packed into complex pairs when N is even, M = N when N is odd), or a direct DFT when M has a
 * prime factor above 5 (M = 0). */
#define ED_GEOM_MAX_STAGES 16
typedef struct {
	const int16_t *audio;
	int64_t utt_stride, frame_step;
	int32_t frames_per_utt, n_frames;  /* n_frames = n_utt * frames_per_utt < 2^31 */
	int32_t N, M, packed, n_stages;
	int32_t radix[ED_GEOM_MAX_STAGES];
	int32_t n_bins;                    /* spectrum bins under the filterbank: A N/2, B N/2 + 1 */
	int32_t n_mel, n_coef, take_log;   /* n_coef = num_mfcc: DCT rows first_mfcc .. first_mfcc + num_mfcc - 1 */
	int32_t team;                      /* threads per frame: 64 (a wavefront, four per workgroup) or 256 (the workgroup) */
	int32_t r0, r1, r2;                /* doubles of a team's three LDS regions (each even: 16-byte aligned) */
	double fft_scale, spec_scale, mel_div, dct_div;
	const double *tw;                  /* [N][2] cos(2 pi j / N), -sin(2 pi j / N) = W_N^j */
	const int32_t *band;               /* [n_mel][3] first bin, taps, offset into taps: the band's nonzero run of the filterbank */
	const double *taps;                /* for B already multiplied by mel_mtx_scale (mel_div divides it out again, as the reference does) */
	const double *dct;                 /* [n_coef][n_mel] 2 cos(pi c (2 n + 1) / (2 n_mel)), c = first_mfcc + row */
	int8_t *feat;
	float feat_scale;
	int64_t feat_utt_stride;           /* int8 and float-network instances: output elements (bytes / floats) from one utterance's rows to the next's; 0: contiguous, frames_per_utt * n_coef */
} ed_geom_args_t;

/* The filterbank / twiddle / DCT tables of one geometry on the device and the kernel's launch template (edison_kws_geom.hip builds
 * them): the context's one-entry cache of edison_kws_geom_batch*, and a table set of its own in every stream and bank. */
struct ed_geom_cache
{
	/* the key: everything the tables depend on */
	int variant, N, n_mel, first, num;
	double fs, lo, hi, scale;
	void *d;            /* one device block: tw | taps | dct | band */
	ed_geom_args_t tmpl; /* plan, LDS regions, scales and table pointers; the per-call fields are filled at launch */
};

/* Enqueue the kernel on `stream` (mfcc_geom_kernels.hip). Returns a hipError_t. */
extern "C" int ed_launch_mfcc_geom(const ed_geom_args_t *a, int n_cu, hipStream_t stream);
/* The same frames, stages and launch; stage 6 stores the float64 DCT row value y (unscaled, unrounded) to mfcc + g * n_coef + row
 * instead of the int8 feature (a->feat and a->feat_scale are not read). */
extern "C" int ed_launch_mfcc_geom_f64(const ed_geom_args_t *a, double *mfcc, int n_cu, hipStream_t stream);
/* The same frames, stages and launch (mfcc_geom_fnet_kernels.hip); stage 6 stores the float network input
 * fminf(fmaxf((float)y * scale, lo), hi) to out + g * n_coef + row, or with a->feat_utt_stride != 0 (in floats) to out + u * feat_utt_stride
 * + f * n_coef + row (a->feat and a->feat_scale are not read). */
extern "C" int ed_launch_mfcc_geom_fnet(const ed_geom_args_t *a, float *out, float scale, float lo, float hi, int n_cu, hipStream_t stream);

#endif
