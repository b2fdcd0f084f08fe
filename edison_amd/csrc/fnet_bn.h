/*
 * fnet_bn.h -- the launch plan of the BatchNorm trainer's kernels (fnet_bn_kernels.hip), built by edison_ftrain_set_batchnorm
 * (edison_ftrain.hip) from the loaded network's plan (fnet.h). DESIGN.md section 19c. Not part of the public ABI.
 *
 * A training call with BatchNorm couples every sample of the call through per-channel batch statistics, forward and backward, so the
 * call is a chain of launches on one stream and what passes from one to the next lies in stores sized for max_rows rows:
 *   zs     per record the conv output z = conv + bias over the WHOLE conv map: [row of the call][R][out_c], R = ch * cw. The plan's
 *          rows r = q P + e come first, the positions a floor-mode pool drops are appended behind them
 *   outs   per record its pooled output after BatchNorm, ReLU and dropout [row][out_n] (the next record's input; the last: the logits)
 *   douts  the loss gradient of outs; mask: one byte per element of outs, the bits of fnet_train.h
 */
#ifndef EDISON_FNET_BN_H
#define EDISON_FNET_BN_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fnet.h"
#include "fnet_train.h"

#define EDBN_UNBIASED 1u /* EDISON_FTRAIN_BN_UNBIASED */

typedef struct {
	ed_fnet_layer_t L;    /* the record as the conv tile, dW and dX see it: rows = R, P = 1, relu = 0 (z is stored before both) */
	ed_ftrain_layer_t G;  /* inv_at into the plan's inv, whose rows are this table's                                           */
	int32_t rows, P, relu; /* the loaded plan's: output rows that reach a pool window, window elements, ReLU                   */
	int32_t R;            /* conv positions per utterance: the rows of z                                                       */
	int32_t has_bn;
	int32_t rowin_at;     /* int32 offset into rtab of rowin[R]                                                                */
	int32_t bn_at;        /* offset of the record's channels in every per-channel array                                        */
	int32_t in_n, out_n;  /* floats per utterance of its input and of its pooled output                                        */
	int64_t z_at, out_at; /* float offsets into zs and into outs / douts / mask                                                */
} ed_fbn_layer_t;

typedef struct {
	int32_t n_layers, batch; /* utterances per tile: the trainer's, fewer while dZ of the largest record does not fit the LDS */
	int32_t in_n, n_out;
	int32_t bn_n;            /* channels of all records: the per-channel arrays' length */
	int32_t grid;
	int64_t max_rows, w_floats;
	const float *w;          /* the master weights */
	const int32_t *tab;      /* the loaded network's tables: koff */
	const int32_t *rtab, *inv;
	float *zs, *outs, *douts, *slabs;
	uint8_t *mask;
	float *bnp;              /* gamma [bn_n], beta [bn_n]: one array, stepped as one */
	float *bng;              /* dgamma [bn_n], dbeta [bn_n] */
	float *mm, *mv;          /* moving mean and variance */
	float *mean, *var, *rstd; /* the last training call's batch statistics */
	double *part;            /* per workgroup two rows of [bn_n] partial results */
	uint32_t *keys;          /* dropout: [max_rows][n_layers][2] */
	ed_fbn_layer_t R[ED_FNET_MAX_LAYERS];
} ed_fbn_plan_t;

/* Dynamic LDS of the backward launch at `batch` utterances a tile: dZ [16-padded batch R][n_pad] and the row bases, the largest record's. */
static inline size_t ed_fbn_lds_bytes(const ed_fbn_plan_t *b, int batch)
{
	size_t most = 0;
	for (int l = 0; l < b->n_layers; l++)
	{
		const size_t mp = ((size_t)batch * (size_t)b->R[l].R + 15) & ~(size_t)15;
		const size_t need = mp * ((size_t)b->R[l].L.n_pad + 1) * 4;
		if (need > most) most = need;
	}
	return most;
}

/* what one record's dropout needs in a launch (fnet_dropout.h): T = 0 is rate 0 */
typedef struct {
	uint32_t T;
	float s;
	int32_t before;
} ed_fbn_drop_t;

/* One training call of n <= max_rows rows: every launch of it, on `stream`. b is the host copy, d_b the device copy the kernels read.
 * drop [n_layers]: the records' dropout (all T = 0: none; then no keys are drawn). Leaves loss / argmax (NULL: not written), logits
 * [n][n_out], the weight gradient in grad [w_floats] (a BatchNorm record's bias gradient +0.0f), dgamma / dbeta in bng, the batch
 * statistics, and the moving statistics moved by `momentum`. Returns a hipError_t. */
extern "C" int ed_launch_fbn_train(const ed_fbn_plan_t *b, const ed_fbn_plan_t *d_b, const float *in, const int32_t *labels, int64_t n, float *loss,
                                   int32_t *argmax, float *logits, float *grad, unsigned long long *ignored, const ed_fbn_drop_t *drop, uint64_t seed,
                                   uint64_t call, double momentum, double eps, uint32_t flags, hipStream_t stream);
/* dst [w_floats] = the inference-mode network of the master weights and the moving statistics: a BatchNorm record's W s and
 * (b - mm) s + beta, s = gamma / sqrt(mv + eps); every other record and all padding copied. */
extern "C" int ed_launch_fbn_fold(const ed_fbn_plan_t *b, const ed_fbn_plan_t *d_b, float *dst, double eps, hipStream_t stream);

#endif
