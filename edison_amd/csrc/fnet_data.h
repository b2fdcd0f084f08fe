/*
 * fnet_data.h -- the launchers of fnet_data_kernels.hip: the gather of an epoch's rows out of a device-resident data set, the reduction
 * of an epoch's per-row losses and hits, and the Adadelta step (edison_ftrain.hip). Not part of the public ABI.
 */
#ifndef EDISON_FNET_DATA_H
#define EDISON_FNET_DATA_H

#include <hip/hip_runtime.h>
#include <stdint.h>

/* what the reduction leaves in device memory */
typedef struct {
	double loss_sum; /* sum of loss [n] in double, in a fixed order */
	int64_t hits;    /* rows with argmax == label                   */
} ed_fdata_sums_t;

/* dst_x [n][in_n], dst_y [n] <- row order[i] of src_x [.][in_n], src_y [.]; every order[i] is a row of the source (the caller checked).
 * Rows move in float4 where in_n % 4 == 0, in float2 where in_n % 2 == 0 (every row is aligned to that), else float by float.
 * Returns a hipError_t. */
extern "C" int ed_launch_fdata_gather(const float *src_x, const int32_t *src_y, const int32_t *order, int64_t n, int32_t in_n, float *dst_x, int32_t *dst_y,
                                      int n_cu, hipStream_t stream);
/* *out <- the sums over loss [n], argmax [n], labels [n]: one workgroup, thread t adds rows t, t + 256, ... in that order, then a tree over
 * the threads: the same n gives the same order of additions. n = 0 gives zeros. */
extern "C" int ed_launch_fdata_reduce(const float *loss, const int32_t *argmax, const int32_t *labels, int64_t n, ed_fdata_sums_t *out, hipStream_t stream);
/* One Adadelta step over w [count], in place: a = rho a + omr g g, u = g sqrt(d + eps) / sqrt(a + eps), w -= lr u, d = rho d + omr u u. */
extern "C" int ed_launch_ftrain_adadelta(float *w, const float *g, float *a, float *d, int64_t count, float lr, float rho, float omr, float eps, int n_cu,
                                         hipStream_t stream);

#endif
