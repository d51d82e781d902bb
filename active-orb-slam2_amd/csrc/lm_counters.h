// The per-keyframe counters of the kernels that count over the resident graph (k_lm_keyframes of csrc/local_map.hip, k_conn of
// csrc/connections.hip): they live in the workgroup's LDS while the graph has at most kLmLdsKfs keyframes (csrc/local_map.h, the
// switch of aos2_local_map_debug_limits), and in zeroed global scratch otherwise.  Kernels are instantiated on kLds.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace aos2 {

// counters and marks: LDS, or global memory through the L2 (they are written by atomics and read back in the same launch)
template <bool kLds>
__device__ __forceinline__ int lm_load(const int32_t *p)
{
    if constexpr (kLds) return *p;
    else return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool kLds>
__device__ __forceinline__ void lm_store(int32_t *p, int v)
{
    if constexpr (kLds) *p = v;
    else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace aos2
