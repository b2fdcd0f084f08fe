/*
 * eval_kernels.hip -- scoring labelled network outputs where they lie (edison_eval.hip): one lane per utterance,
 * grid-stride, the rules of nnom_eval_core.h. Counting is integer only, so the counters do not depend on the launch shape or on the
 * order the atomics arrive in; there is no float atomic here.
 *
 *   n_out <= 64   every workgroup keeps its own matrix (n_out^2 uint32, at most 16 KB) and top-k histogram in LDS and counts there with
 *                 LDS atomics (a workgroup sees far fewer than 2^32 utterances in a launch); after the loop it adds its non-zero cells
 *                 to the evaluator's 64-bit device counters.
 *   n_out <= 256  the matrix is too large for that: cells are added in global memory directly, the top-k histogram stays in LDS.
 *   count and skipped are summed per lane, reduced per wave, then per workgroup: one global atomic each per workgroup.
 *
 * A row of at most 16 bytes (the shipped 10 int8 outputs) is fetched with loads of 8, 4, 2 and 1 bytes -- exactly its bytes, rows are
 * not padded -- into registers; longer rows are read in place.
 *
 * Device counters, uint64: [0] count, [1] skipped, [2 .. 2 + n_out^2) the matrix, then min(top_k, n_out) top-k entries (a rank is
 * below n_out, the entries above stay 0 on the host).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nnom_eval_core.h"

#define EDE_THREADS 256
#define EDE_LDS_CLASSES 64

/* a row of up to 16 int8 in two registers pairs */
struct ede_row_i8
{
	uint64_t lo, hi;
	__device__ int32_t operator[](int j) const { return (int8_t)((j < 8 ? lo : hi) >> (8 * (j & 7))); }
};

/* a row of up to 4 float32 */
struct ede_row_f32
{
	float v0, v1, v2, v3;
	__device__ float operator[](int j) const { return j == 0 ? v0 : j == 1 ? v1 : j == 2 ? v2 : v3; }
};

template <class W> __device__ static inline uint64_t ede_load(const int8_t *p)
{
	W w;
	__builtin_memcpy(&w, p, sizeof(W)); /* rows of int8 start at any byte */
	return (uint64_t)w;
}

__device__ static inline ede_row_i8 ede_fetch_i8(const int8_t *p, int n_out)
{
	ede_row_i8 r = {0, 0};
	int off = 0;
	if (n_out & 16) { r.lo = ede_load<uint64_t>(p); r.hi = ede_load<uint64_t>(p + 8); return r; }
	if (n_out & 8) { r.lo = ede_load<uint64_t>(p); off = 8; }
	uint64_t tail = 0; /* the up to 7 bytes behind `off`, lowest first */
	int tb = 0;
	if (n_out & 4) { tail = ede_load<uint32_t>(p + off); tb = 4; }
	if (n_out & 2) { tail |= ede_load<uint16_t>(p + off + tb) << (8 * tb); tb += 2; }
	if (n_out & 1) { tail |= ede_load<uint8_t>(p + off + tb) << (8 * tb); }
	if (off) r.hi = tail; else r.lo = tail;
	return r;
}

__device__ static inline ede_row_f32 ede_fetch_f32(const float *p, int n_out)
{
	ede_row_f32 r = {0.f, 0.f, 0.f, 0.f};
	r.v0 = p[0];
	if (n_out > 1) r.v1 = p[1];
	if (n_out > 2) r.v2 = p[2];
	if (n_out > 3) r.v3 = p[3];
	return r;
}

__device__ static inline ed_eval_one_t ede_one(const int8_t *out, int64_t i, int n_out, int32_t t, int rule)
{
	const int8_t *p = out + i * n_out;
	return n_out <= 16 ? ed_eval_i8_one(ede_fetch_i8(p, n_out), n_out, t) : ed_eval_i8_one(p, n_out, t);
}

__device__ static inline ed_eval_one_t ede_one(const float *out, int64_t i, int n_out, int32_t t, int rule)
{
	const float *p = out + i * n_out;
	return n_out <= 4 ? ed_eval_f32_one(ede_fetch_f32(p, n_out), n_out, t, rule) : ed_eval_f32_one(p, n_out, t, rule);
}

template <class T, int RULE>
__global__ __launch_bounds__(EDE_THREADS) void ed_eval_kernel(const T *__restrict__ out, const int32_t *__restrict__ labels, int64_t n, int n_out,
                                                              int top_k, unsigned long long *__restrict__ counters, uint32_t *__restrict__ pred,
                                                              float *__restrict__ prob, int32_t *__restrict__ rank)
{
	__shared__ uint32_t s_mat[EDE_LDS_CLASSES * EDE_LDS_CLASSES];
	__shared__ uint32_t s_top[256];
	__shared__ uint32_t s_cnt[2];
	const int tid = threadIdx.x;
	const bool lds_mat = n_out <= EDE_LDS_CLASSES;
	const int cells = n_out * n_out;
	const int k_top = top_k < n_out ? top_k : n_out; /* <= 256 */
	unsigned long long *const g_mat = counters + 2, *const g_top = counters + 2 + cells;

	if (lds_mat)
		for (int c = tid; c < cells; c += EDE_THREADS) s_mat[c] = 0;
	for (int c = tid; c < k_top; c += EDE_THREADS) s_top[c] = 0;
	if (tid < 2) s_cnt[tid] = 0;
	__syncthreads();

	uint32_t my_count = 0, my_skipped = 0;
	for (int64_t i = (int64_t)blockIdx.x * EDE_THREADS + tid; i < n; i += (int64_t)gridDim.x * EDE_THREADS)
	{
		const int32_t t = labels[i];
		const ed_eval_one_t r = ede_one(out, i, n_out, t, RULE);
		if (pred) pred[i] = r.pred;
		if (prob) prob[i] = r.prob;
		if (rank) rank[i] = r.rank;
		if (!r.counted) { my_skipped++; continue; }
		my_count++;
		if (r.rank < 0) continue;                     /* a single NNoM output: no matrix, no top-k */
		const int cell = t * n_out + (int)r.pred;     /* 0 <= t, pred < n_out */
		if (lds_mat) atomicAdd(&s_mat[cell], 1u); else atomicAdd(&g_mat[cell], 1ull);
		if (r.rank < k_top) atomicAdd(&s_top[r.rank], 1u);
	}

	/* count and skipped: per wave, then per workgroup, then one global atomic each */
	for (int d = warpSize / 2; d > 0; d >>= 1)
	{
		my_count += __shfl_down(my_count, d);
		my_skipped += __shfl_down(my_skipped, d);
	}
	if ((tid & (warpSize - 1)) == 0)
	{
		if (my_count) atomicAdd(&s_cnt[0], my_count);
		if (my_skipped) atomicAdd(&s_cnt[1], my_skipped);
	}
	__syncthreads();

	if (lds_mat)
		for (int c = tid; c < cells; c += EDE_THREADS)
		{
			const uint32_t v = s_mat[c];
			if (v) atomicAdd(&g_mat[c], (unsigned long long)v);
		}
	for (int c = tid; c < k_top; c += EDE_THREADS)
	{
		const uint32_t v = s_top[c];
		if (v) atomicAdd(&g_top[c], (unsigned long long)v);
	}
	if (tid < 2 && s_cnt[tid]) atomicAdd(&counters[tid], (unsigned long long)s_cnt[tid]);
}

template <class T, int RULE>
static int ede_launch(const T *out, const int32_t *labels, int64_t n, int n_out, int top_k, int max_blocks, unsigned long long *counters, uint32_t *pred,
                      float *prob, int32_t *rank, hipStream_t stream)
{
	int64_t blocks = (n + EDE_THREADS - 1) / EDE_THREADS;
	if (blocks > max_blocks) blocks = max_blocks;
	hipLaunchKernelGGL((ed_eval_kernel<T, RULE>), dim3((unsigned)blocks), dim3(EDE_THREADS), 0, stream, out, labels, n, n_out, top_k, counters, pred, prob,
	                   rank);
	return (int)hipGetLastError();
}

/* n > 0, 1 <= n_out <= 256, top_k >= 0, max_blocks >= 1: checked by the caller (edison_eval.hip). Returns a hipError_t. */
extern "C" int ed_launch_eval_i8(const int8_t *out, const int32_t *labels, int64_t n, int n_out, int top_k, int max_blocks, unsigned long long *counters,
                                 uint32_t *pred, float *prob, int32_t *rank, hipStream_t stream)
{
	if (n <= 0 || n_out < 1 || n_out > 256 || top_k < 0 || max_blocks < 1) return (int)hipErrorInvalidValue;
	return ede_launch<int8_t, EDISON_EVAL_NNOM>(out, labels, n, n_out, top_k, max_blocks, counters, pred, prob, rank, stream);
}

extern "C" int ed_launch_eval_f32(int rule, const float *out, const int32_t *labels, int64_t n, int n_out, int top_k, int max_blocks,
                                  unsigned long long *counters, uint32_t *pred, float *prob, int32_t *rank, hipStream_t stream)
{
	if (n <= 0 || n_out < 1 || n_out > 256 || top_k < 0 || max_blocks < 1) return (int)hipErrorInvalidValue;
	if (rule == EDISON_EVAL_KERAS)
		return ede_launch<float, EDISON_EVAL_KERAS>(out, labels, n, n_out, top_k, max_blocks, counters, pred, prob, rank, stream);
	if (rule == EDISON_EVAL_ARGMAX)
		return ede_launch<float, EDISON_EVAL_ARGMAX>(out, labels, n, n_out, top_k, max_blocks, counters, pred, prob, rank, stream);
	return (int)hipErrorInvalidValue;
}
