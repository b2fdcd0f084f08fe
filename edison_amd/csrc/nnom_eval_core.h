/*
 * nnom_eval_core.h -- what one labelled network output adds to an evaluation: the predicted label, its "probability" and the rank of
 * the true label. Written once for the host (legacy.c: edison_nnom_prediction_run, edison_eval_f32_host) and for the device
 * (eval_kernels.hip: ed_eval_kernel behind edison_eval_add_*). The callers do the counting: confusion[t * n_out + pred]++,
 * top_k[rank]++ when rank < top_k, count++. This header neither calls nor changes ed_nnom_predict_one (nnom_predict_core.h), whose prob
 * divides by the sum of ALL outputs and is deliberately different.
 *
 * EDISON_EVAL_NNOM -- prediction_run (nnom_utils.c:88-164) on n_out int8 values, the softmax if the graph ends in one, else the logits.
 *   n_out > 1:
 *     rank  (:112-121) the number of j != t with out[t] < out[j], plus the number of j < t with out[j] == out[t].
 *     pred  (:128-136) the index of the first strict maximum, starting from out[0].
 *     prob  (:137-143) a quirk of the reference, kept: `sum` is a uint32 that starts at 0 and adds out[j] for j = 1 .. n_out - 1 only
 *           (element 0 is left out), each int8 sign-extended and added modulo 2^32; prob = (float)max / (float)sum with max converted
 *           int -> float and sum uint32 -> float, the correctly rounded division (`/` on the host, __fdiv_rn on the device), 0 when
 *           sum == 0. A sum that wraps gives a tiny quotient, a row like [5, 5, 0, ..., 5] gives 0.5.
 *   n_out == 1 (:150-157): prob = out[0] / 127.f, pred = prob >= 0.5f; no rank (-1), no matrix and no top-k: only count moves.
 *   NNoM's matrix cells are uint16_t and wrap at 65 536; the counters here are 64-bit and do not. The two agree while every cell is
 *   below 65 536.
 *
 * EDISON_EVAL_KERAS -- predictWithConfMatrix (kws_keras.py:503-517, kws_nnom.py:150-165) on n_out float32 probabilities:
 *     pred = the first c with p[c] > 0.5f, class 0 when there is none: argmax of 1.0 * (y_pred > 0.5).
 *   sklearn's confusion_matrix drops classes that occur neither as a label nor as a prediction; the matrix here is always
 *   n_out x n_out.
 * EDISON_EVAL_ARGMAX -- float32: pred = the first maximum, edison_fnet_batch's argmax.
 * Both float rules: prob = p[pred]; rank follows the tie rule above with float comparisons. The reference has no float top-k: that
 * part is this project's own. A NaN compares false, as in C.
 *
 * Labels are int32. One outside 0 .. n_out - 1 (-1 stands for "unlabelled") still gets pred and prob; its rank is -1 and the caller
 * counts it as skipped, leaving count, the matrix and top_k alone. With one output that makes 0 the only label that counts (the
 * reference never looks at the label there).
 *
 * In C++ a row is anything with operator[] (the kernel hands over short rows in registers); in C it is a pointer.
 */
#ifndef NNOM_EVAL_CORE_H
#define NNOM_EVAL_CORE_H
#include <stdint.h>

#include "../../include/edison_hip.h"

#if defined(__HIPCC__) && defined(__HIP_DEVICE_COMPILE__)
#define ED_EVAL_DIV(a, b) __fdiv_rn((a), (b))
#else
#define ED_EVAL_DIV(a, b) ((a) / (b))
#endif
#ifdef __HIPCC__
#define ED_EVAL_FN __host__ __device__ static inline
#else
#define ED_EVAL_FN static inline
#endif
#ifdef __cplusplus
#define ED_EVAL_ROW(name) template <class name>
#else
#define ED_EVAL_ROW(name)
typedef const int8_t *ed_eval_row_i8;
typedef const float *ed_eval_row_f32;
#endif

typedef struct ed_eval_one_t
{
	uint32_t pred;
	float prob;
	int32_t rank; /* -1: none taken (label out of range, or a single output) */
	int counted;  /* the label is in range: the caller counts this output */
} ed_eval_one_t;

ED_EVAL_ROW(ed_eval_row_i8)
ED_EVAL_FN ed_eval_one_t ed_eval_i8_one(ed_eval_row_i8 out, int n_out, int32_t t)
{
	ed_eval_one_t r;
	r.counted = t >= 0 && t < n_out;
	r.rank = -1;
	if (n_out > 1)
	{
		int32_t max_val = out[0], max_index = 0;
		uint32_t sum = 0;
		for (int j = 1; j < n_out; j++)
		{
			const int32_t v = out[j];
			if (v > max_val) { max_val = v; max_index = j; }
			sum += (uint32_t)v;
		}
		r.pred = (uint32_t)max_index;
		r.prob = sum != 0 ? ED_EVAL_DIV((float)max_val, (float)sum) : 0.0f;
		if (r.counted)
		{
			const int32_t vt = out[t];
			int32_t rank = 0;
			for (int j = 0; j < n_out; j++)
			{
				const int32_t v = out[j];
				rank += (j != t) & ((vt < v) | ((vt == v) & (j < t)));
			}
			r.rank = rank;
		}
	}
	else
	{
		r.prob = ED_EVAL_DIV((float)out[0], 127.f);
		r.pred = r.prob >= 0.5f ? 1u : 0u;
	}
	return r;
}

ED_EVAL_ROW(ed_eval_row_f32)
ED_EVAL_FN ed_eval_one_t ed_eval_f32_one(ed_eval_row_f32 p, int n_out, int32_t t, int rule)
{
	ed_eval_one_t r;
	int pred = 0;
	if (rule == EDISON_EVAL_KERAS)
	{
		for (int c = 0; c < n_out; c++)
			if (p[c] > 0.5f) { pred = c; break; }
	}
	else
	{
		float max_val = p[0];
		for (int c = 1; c < n_out; c++)
		{
			const float v = p[c];
			if (v > max_val) { max_val = v; pred = c; }
		}
	}
	r.pred = (uint32_t)pred;
	r.prob = p[pred];
	r.counted = t >= 0 && t < n_out;
	r.rank = -1;
	if (r.counted)
	{
		const float vt = p[t];
		int32_t rank = 0;
		for (int j = 0; j < n_out; j++)
		{
			const float v = p[j];
			rank += (j != t) & ((vt < v) | ((vt == v) & (j < t)));
		}
		r.rank = rank;
	}
	return r;
}

#endif
