#pragma once
// qnet_trace.h — the policy kernels' phase stamps (SHIPENV_X3_TRACE, a diagnostic build): X3STAMP,
// X3STAMP_ANY and their buffer g_ptrace, read back by se_policy_trace_read (qpolicy.h) for
// tools/time_policy.py --trace. Empty statements in the product build.
//
// A fragment of shipenv.hip's translation unit, included inside qpolicy.h's anonymous
// namespace before the policy kernels: not a stand-alone header. X3STAMP reads the kernel's own
// tile_iter.

#ifndef SHIPENV_X3_TRACE
#define SHIPENV_X3_TRACE 0  // 1 = diagnostic build: per-wave s_memtime phase stamps of the fp32 policy
#endif                      // kernels' 4th tile (se_policy_trace_read, tools/time_policy.py --trace)
#if SHIPENV_X3_TRACE
__device__ uint64_t g_ptrace[4096 * 16];
#define X3STAMP(k)                                                                                          \
    do {                                                                                                    \
        if (tile_iter == 3 && (threadIdx.x & 63) == 0)                                                      \
            g_ptrace[(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) % 4096 * 16 + (k)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#define X3STAMP_ANY(k)                                                                                      \
    do {                                                                                                    \
        if ((threadIdx.x & 63) == 0) {                                                                      \
            uint64_t* p_ = g_ptrace + (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) % 4096 * 16;       \
            p_[(k)] = __builtin_amdgcn_s_memrealtime();                                                     \
            p_[(k) + 3] = __builtin_amdgcn_s_memtime();                                                     \
        }                                                                                                   \
    } while (0)
#else
#define X3STAMP(k) \
    do {           \
    } while (0)
#define X3STAMP_ANY(k) X3STAMP(k)
#endif
