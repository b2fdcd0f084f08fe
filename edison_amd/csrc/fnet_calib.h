/*
 * fnet_calib.h -- what the calibration kernel (fnet_calib_kernels.hip) and its host side (edison_fcal.hip) share: the layout of the
 * device counters and of the statistic's LDS behind the float network's plan (fnet.h). Not part of the public ABI.
 */
#ifndef EDISON_FNET_CALIB_H
#define EDISON_FNET_CALIB_H

#include "fnet.h"

#define EDFC_HIST 256                 /* exponent cells                                                          */
#define EDFC_LDS_WORDS (EDFC_HIST + 1) /* uint32 in LDS: the histogram, then the maximum                          */
#define EDFC_WORDS (EDFC_HIST + 2)    /* uint64 per index in device memory: absmax (low half), count, the histogram */

/* Dynamic LDS bytes of the calibration kernel's workgroup at plan p. */
static inline size_t ed_fnet_calib_lds_bytes(const ed_fnet_plan_t *p) { return ed_fnet_lds_bytes(p) + sizeof(uint32_t) * EDFC_LDS_WORDS; }

/* n utterances back to back (in_n floats each) through the network of plan p, their statistic added to counters
 * [(n_layers + 1) * EDFC_WORDS]. Returns a hipError_t. */
extern "C" int ed_launch_fnet_calib(const ed_fnet_plan_t *p, const float *in, int64_t n, unsigned long long *counters, hipStream_t stream);

#endif
