/*
 * fnet_dropout.h -- the dropout mask of the float32 trainer (fnet_grad_kernels.hip, edison_ftrain.hip), written
 * once: plain C that also compiles as HIP device code, so the kernel, the library's host code and a stand-alone host program state the
 * same function. Whether element e of record l is kept, for sample u of a training call, depends on (seed, call, u, l, e) only: not on
 * the training batch, the grid, the tile or the lane that computes it.
 *
 *   keys    per (sample, record): (kA, kB) = words 0 and 1 of Philox4x32-10 at counter (u, call & 0xffffffff, call >> 32, l) under key
 *           (seed & 0xffffffff, seed >> 32); a training call has n < 2^32 samples
 *   hash    per element: h = fmix32(fmix32(e ^ kA) + kB), fmix32 MurmurHash3's finaliser
 *   keep    iff h >= T, T = (uint32) floor(rate 2^32 + 0.5) in double; a kept value is multiplied by s = (float)(1 / (1 - rate)), a
 *           dropped one is +0.0f
 *   e       after the pool q out_c + c (pooled position q, channel c); before the pool r out_c + c, r = q P + element the plan's
 *           output row, absent rows counted
 * Not part of the public ABI.
 */
#ifndef EDISON_FNET_DROPOUT_H
#define EDISON_FNET_DROPOUT_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EDD_FN static __host__ __device__ __forceinline__
#else
#define EDD_FN static inline
#endif

#define EDD_PHILOX_M0 0xD2511F53u
#define EDD_PHILOX_M1 0xCD9E8D57u
#define EDD_PHILOX_W0 0x9E3779B9u
#define EDD_PHILOX_W1 0xBB67AE85u

/* Philox4x32-10 of counter c[4] under key k[2], in place */
EDD_FN void edd_philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1)
{
	for (int round = 0; round < 10; round++)
	{
		const uint64_t p0 = (uint64_t)EDD_PHILOX_M0 * c[0], p1 = (uint64_t)EDD_PHILOX_M1 * c[2];
		const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
		c[1] = (uint32_t)p1;
		c[3] = (uint32_t)p0;
		c[0] = n0;
		c[2] = n2;
		k0 += EDD_PHILOX_W0;
		k1 += EDD_PHILOX_W1;
	}
}

/* the keys of (sample u, record l) in training call `call` under `seed` */
EDD_FN void edd_keys(uint64_t seed, uint64_t call, uint32_t u, uint32_t l, uint32_t *kA, uint32_t *kB)
{
	uint32_t c[4] = {u, (uint32_t)call, (uint32_t)(call >> 32), l};
	edd_philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
	*kA = c[0];
	*kB = c[1];
}

EDD_FN uint32_t edd_fmix32(uint32_t x)
{
	x ^= x >> 16;
	x *= 0x85ebca6bu;
	x ^= x >> 13;
	x *= 0xc2b2ae35u;
	x ^= x >> 16;
	return x;
}

EDD_FN uint32_t edd_hash(uint32_t e, uint32_t kA, uint32_t kB) { return edd_fmix32(edd_fmix32(e ^ kA) + kB); }

/* the threshold of a rate in [0, 1): kept iff hash >= T; T = 0 keeps everything */
EDD_FN uint32_t edd_threshold(double rate)
{
	const uint64_t t = (uint64_t)(rate * 4294967296.0 + 0.5);
	return t > 0xffffffffu ? 0xffffffffu : (uint32_t)t; /* a rate within 2^-33 of 1 */
}

EDD_FN float edd_scale(double rate) { return (float)(1.0 / (1.0 - rate)); }

/* the whole function, for host code: is element e of record l kept for sample u */
EDD_FN int edd_keep(uint64_t seed, uint64_t call, uint32_t u, uint32_t l, uint32_t e, double rate)
{
	uint32_t kA, kB;
	edd_keys(seed, call, u, l, &kA, &kB);
	return edd_hash(e, kA, kB) >= edd_threshold(rate);
}

#endif
