/*
 * edison_stream_kernels.h -- the two state kernels of the any-geometry streams, defined once in edison_stream_geom.hip and launched from
 * there and from edison_stream_float.hip: the output filter (+ edisonFSM) over n_out classes, and the history shift of the two sliding
 * buffers. Not part of the public ABI.
 */
#ifndef EDISON_STREAM_KERNELS_H
#define EDISON_STREAM_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edison_fsm_core.h"

#define EDSG_FILTER_MAX_OUT 256 /* classes the filter kernel serves: one lane each in one workgroup */

/* the state machine behind the filter; fsm = NULL: none */
struct edsg_fsm_stage_t
{
	edison_fsm *fsm;      /* device memory, read and written                       */
	int32_t *states;      /* [n] out: the state after each inference               */
	edison_fsm *copy;     /* out: the machine after the push (the host's view)     */
	uint32_t dt_us;
	ed_fsm_roles_t roles;
};

/* The history to the front of the two sliding buffers: the newest `tail` samples from audio + a_src, and `feat_bytes` bytes from
 * feat + f_src (rows of any element type: the move is a byte move). One workgroup on q. Returns a hipError_t. */
int ed_launch_stream_shift(hipStream_t q, int16_t *audio, int64_t a_src, int tail, void *feat, int64_t f_src, int feat_bytes);
/* The filter over n inferences x[n][n_out] float32 (the float network's probabilities) with the arithmetic of the int8 instance
 * (edison_stream_geom.hip). One workgroup on q. Returns a hipError_t. */
int ed_launch_stream_filter_f32(hipStream_t q, const float *x, int n, int n_out, double alpha, double one_minus_alpha, double threshold,
                                float *state, float *filt, int32_t *likely, int32_t *spotted, edsg_fsm_stage_t fs);

#endif
