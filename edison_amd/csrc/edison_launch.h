/*
 * edison_launch.h -- preparing a kernel for launch on the current device (host only; defined in edison_hip.hip). Not part of
 * the public ABI, and not included from edison_internal.h: that header is also handed to hipRTC as source text.
 */
#ifndef EDISON_LAUNCH_H
#define EDISON_LAUNCH_H

#include <stddef.h>

/* Raise fn's dynamic-LDS limit on the current device to at least lds_bytes (once per fn, device and size: more than 64 KB has
 * to be asked for, and the attribute belongs to the function on a device). With blocks_per_cu != NULL, also return the
 * resident workgroups per CU at (threads, lds_bytes) -- at least 1 -- computed once per fn and device, capped by the integer in
 * getenv(cap_env) when cap_env is given and the value is in 1 .. computed. A cache hit takes no lock and makes no HIP call
 * beyond hipGetDevice. Returns a hipError_t. Not for hipModule functions: a reloaded module may reuse an address. */
int ed_kernel_prepare(const void *fn, int threads, size_t lds_bytes, const char *cap_env, int *blocks_per_cu);

#endif
