// hs_flow.h -- the exchange primitives of the dataflow sweeps (kernels_solve_wide.hip, kernels_solve_t.hip): values are published with an
// agent-scope atomic store into vectors that hold the SENTINEL (all bits set) until then, and polled with agent-scope atomic loads; every poll
// is bounded by HS_FLOW_SPIN rounds of s_sleep.
#pragma once
#include "hs_common.h"

#define HS_FLOW_SPIN (1 << 22)
static constexpr unsigned long long HS_SENT = ~0ull;
__device__ __forceinline__ unsigned long long flow_ldbits(const double* p) {
  return __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void flow_publish(double* p, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void flow_publish(cplx* p, cplx v) {
  flow_publish(reinterpret_cast<double*>(p), v.re);
  flow_publish(reinterpret_cast<double*>(p) + 1, v.im);
}
