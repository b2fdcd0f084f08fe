/*
 * fnet_train.h -- the launch plan of the float32 network's gradient kernels (fnet_grad_kernels.hip), built by edison_ftrain.hip from the
 * loaded network's plan (fnet.h). DESIGN.md section 19. Not part of the public ABI.
 */
#ifndef EDISON_FNET_TRAIN_H
#define EDISON_FNET_TRAIN_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fnet.h"

#define EDFT_WIN_MASK 3 /* a mask byte: the pool window's first maximum, element e = r % P ... */
#define EDFT_PASS 4     /* ... and whether its gradient passes: no ReLU, or a pre-activation > 0 */
#define EDFT_DROPPED 8  /* ... unless the winner, or the pooled output, was dropped (dropout): it passes nothing */
#define EDFT_SGD 1      /* edison_ftrain_set_opt's kind; 0 is Adam */

/* What the backward half needs of record l beside ed_fnet_layer_t. inv is the inverse of the record's gather, row-at-offset: the input
 * element at position pos = y * in_w + x (any channel) is read by output row inv[pos * T + t] through tap t = ky * kw + kx, or by none
 * (-1: a stride skips it, the pool's floor drops the row, or the window would start outside the image). */
typedef struct {
	int32_t K;      /* real k rows: kh * kw * in_c                                  */
	int32_t T;      /* taps: kh * kw                                                */
	int32_t np;     /* input positions: in_h * in_w                                 */
	int32_t inv_at; /* int32 offset into inv of inv[np][T]; unused by record 0      */
} ed_ftrain_layer_t;

typedef struct {
	ed_fnet_plan_t net; /* the loaded network's plan at the trainer's batch */
	ed_ftrain_layer_t G[ED_FNET_MAX_LAYERS];
	const int32_t *inv;
	int32_t dy_lds;     /* floats of the backward half's dY[16-padded batch * rows][n_pad], the largest record's */
	int32_t rb_lds;     /* ints of its row bases, the largest record's 16-padded batch * rows, two a row of a padded record */
	int64_t w_floats;   /* the packed weight array: every record's B[k_pad][n_pad], then bias[n_pad]           */
	/* per workgroup of the grid: a gradient slab [w_floats], and per utterance of its batch the records' outputs, their gradients
	 * (both [acts_n] floats) and the mask bytes [acts_n] */
	float *slabs, *acts, *dacts;
	uint8_t *mask;
	/* dropout (fnet_dropout.h), behind everything else so that no other field moves: per record the threshold (0: rate 0, no hash), the
	 * scale 1 / (1 - rate) and whether the mask stands before the pool; per workgroup the keys [batch][n_layers][2] of its tile */
	uint32_t drop_T[ED_FNET_MAX_LAYERS];
	float drop_s[ED_FNET_MAX_LAYERS];
	uint8_t drop_before[ED_FNET_MAX_LAYERS];
	uint32_t *keys;
} ed_ftrain_plan_t;

/* Dynamic LDS bytes of the training workgroup: the forward half's plan, and over it (the forward half is done with it) dY and the row
 * bases of the record the backward half is at. */
static inline size_t ed_ftrain_lds_bytes(const ed_ftrain_plan_t *t)
{
	const size_t fwd = ed_fnet_lds_bytes(&t->net), bwd = sizeof(float) * (size_t)t->dy_lds + sizeof(int32_t) * (size_t)t->rb_lds;
	return fwd > bwd ? fwd : bwd;
}

/* n inputs and labels -> loss [n], argmax [n] (NULL: not written), logits [n][n_out], and the batch-mean gradient of the cross entropy in
 * grad [w_floats]: `grid` workgroups (at most the plan's slabs) walk the batches, then the slabs of those that had one are summed in
 * index order. d_plan: *t in device memory, which the kernel reads. A label outside [0, n_out) bumps *ignored and contributes nothing.
 * drop != 0: the instantiation with the dropout mask of (seed, call), n < 2^32. Returns a hipError_t. */
extern "C" int ed_launch_ftrain_grad(const ed_ftrain_plan_t *t, const ed_ftrain_plan_t *d_plan, const float *in, const int32_t *labels, int64_t n, float *loss, int32_t *argmax,
                                     float *logits, float *grad, unsigned long long *ignored, int grid, int drop, uint64_t seed, uint64_t call, hipStream_t stream);
/* One optimiser step over w [count], in place. Adam: m, v and `factor` = lr sqrt(1 - b2^t) / (1 - b1^t); SGD: w -= factor g. */
extern "C" int ed_launch_ftrain_step(int kind, float *w, const float *g, float *m, float *v, int64_t count, float factor, float b1, float omb1, float b2,
                                     float omb2, float eps, int n_cu, hipStream_t stream);

#endif
