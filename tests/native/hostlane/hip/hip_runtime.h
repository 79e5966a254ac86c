// Stand-in for <hip/hip_runtime.h> (tests/native/hostlane): the device headers of fray_amd/csrc compiled for the host as ONE lane of a wave.
// Found before the real header because the harness puts this directory first on the include path.  __HIP_DEVICE_COMPILE__ stays undefined:
// dev_math.hpp and dev_rng.hpp then take their portable arithmetic, and FRAY_RO (dev_scene.hpp) is no address space.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#define __device__
#define __host__
#define __global__
#define __constant__
#define __shared__ static          // the KD walk's LDS stack (dev_trace.hpp kd_stack_slot) returns a pointer into it: it must outlive the call
#define __forceinline__ inline __attribute__((always_inline))
#define __launch_bounds__(...)

struct hostlane_dim3 { unsigned x, y, z; };
static const hostlane_dim3 threadIdx = {0, 0, 0}, blockIdx = {0, 0, 0}, blockDim = {1, 1, 1}, gridDim = {1, 1, 1};

// wave votes of a wave of one
static inline int __any(int p) { return p != 0; }
static inline int __all(int p) { return p != 0; }
static inline unsigned long long __ballot(int p) { return p ? 1ull : 0ull; }
static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
#define __builtin_amdgcn_readlane(v, l) (v)
#define __builtin_amdgcn_sched_barrier(m) ((void)0)

static inline unsigned __float_as_uint(float f) { unsigned u; memcpy(&u, &f, sizeof u); return u; }
