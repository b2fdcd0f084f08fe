/*
 * edison_postproc_core.h -- the firmware's output filter (firmware/src/app.c:341-356), written once for every kernel that runs it:
 * the any-geometry streams and banks (edison_stream_core.hip), the fixed stream (edison_stream.hip: ed_stream_filter_kernel) and the
 * one-launch microphone push (cnn_mfma_kernels.hip: the filtering lane of ed_kws1_kernel).
 *
 *     netOutFilt[c] = (float)(ALPHA * netOutFilt[c] + (1.0 - ALPHA) * netOutFloat[c])     double arithmetic, rounded to float on the store
 *     arm_max_f32: the first maximum;   spotted = that maximum > TRUE_THRESHOLD;   then one step of edisonFSM (edison_fsm_core.h)
 */
#ifndef EDISON_POSTPROC_CORE_H
#define EDISON_POSTPROC_CORE_H
#include "edison_fsm_core.h"

#ifdef __HIPCC__
#define ED_PP_FN __host__ __device__ static inline
#else
#define ED_PP_FN static inline
#endif

/* The rounding rule. The product and the sum are rounded SEPARATELY: the Cortex-M4 computes doubles in software, nothing is fused. The
 * compiler's default contraction turns a plain * and + into one v_fma_f64 -- a different double in the last place, and a different
 * float wherever that sum sits next to a float rounding boundary (found by scripted softmax streams: one value in ~4 000; network
 * outputs of 0 and 127 never showed it). HIP's __dmul_rn / __dadd_rn do not help: they are plain * and + whose bodies are compiled with
 * their header's own contraction. So the two operations are written here, under the library's one contract(off), and nowhere else.
 * Behind the pair the header hands contraction back as hipcc sets it for every file of the library (-ffp-contract=fast-honor-pragmas marks
 * each operation exactly as contract(fast) does; amdgcn has no float_control(push / pop) to restore it with), so the code of a file
 * that includes this header compiles as it did without it. build.py refuses an ED_CFLAGS with -ffp-contract for that reason. */
#pragma clang fp contract(off)
/* (1 - alpha) * x as the firmware rounds it; x: the network output as a double (exact for an int8 and for a float) */
ED_PP_FN double ed_filter_term(double one_minus_alpha, double x) { return one_minus_alpha * x; }
/* one step of the moving average: the state y and ed_filter_term's product for the new output */
ED_PP_FN float ed_filter_step(double alpha, float y, double term) { return (float)(alpha * (double)y + term); }
#pragma clang fp contract(fast)

/* the state machine behind a filter kernel, for the n inferences of a push over n_mics microphones (the fixed stream: 1); fsm = NULL:
 * none */
struct ed_fsm_stage_t
{
	edison_fsm *fsm;      /* [n_mics] device memory, read and written                             */
	int32_t *states;      /* [n][n_mics] out: the state after each inference                      */
	edison_fsm *copy;     /* [n_mics] out: the machines after the push (the host's view), or NULL */
	uint32_t dt_us;
	ed_fsm_roles_t roles;
};

#endif
