/*
 * nnom_predict_core.h -- the result rule of nnom_predict (nnom_utils.c:258-305) on one network output, written once for the host
 * (legacy.c: edison_nnom_predict, aiNnomPredict) and for the device (edison_f32.hip: ed_nnom_predict_kernel, the last stage of
 * edison_kws_f32_batch* and edison_f32_stream_predict*). `out` is the graph's last output -- the softmax if it ends in one, the logits
 * otherwise -- n_out int8 values.
 *
 *   n_out > 1  (nnom_utils.c:272-293): label = index of the first strict maximum, sum = int32 sum of ALL values,
 *              prob = (float)max / (float)sum, 0 when the sum is 0. A graph without Softmax can give a negative sum: the C quotient
 *              (a negative or > 1 "probability") is kept as it is.
 *   n_out == 1 (nnom_utils.c:295-302): prob = out / 127.f, label = prob >= 0.5f.
 *
 * Both divisions are the correctly rounded IEEE one: `/` in host C (no fast-math flag anywhere in the build), __fdiv_rn on the device
 * (a plain `/` in device code is correctly rounded too under the build's flags; the intrinsic says so in the source).
 */
#ifndef NNOM_PREDICT_CORE_H
#define NNOM_PREDICT_CORE_H
#include <stdint.h>

#if defined(__HIPCC__) && defined(__HIP_DEVICE_COMPILE__)
#define ED_PREDICT_DIV(a, b) __fdiv_rn((a), (b))
#else
#define ED_PREDICT_DIV(a, b) ((a) / (b))
#endif
#ifdef __HIPCC__
#define ED_PREDICT_FN __host__ __device__ static inline
#else
#define ED_PREDICT_FN static inline
#endif

ED_PREDICT_FN void ed_nnom_predict_one(const int8_t *out, int n_out, uint32_t *label, float *prob)
{
	if (n_out > 1)
	{
		int32_t max_val = out[0], max_index = 0, sum = out[0];
		for (int i = 1; i < n_out; i++)
		{
			if (out[i] > max_val) { max_val = out[i]; max_index = i; }
			sum += out[i];
		}
		*label = (uint32_t)max_index;
		*prob = sum != 0 ? ED_PREDICT_DIV((float)max_val, (float)sum) : 0.0f;
	}
	else
	{
		const float p = ED_PREDICT_DIV((float)out[0], 127.f);
		*prob = p;
		*label = p >= 0.5f ? 1u : 0u;
	}
}

#endif
