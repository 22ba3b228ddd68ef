// hs_flow.h -- the skeleton of the dataflow sweeps (flow_sweep_kernel in kernels_solve_wide.hip, t_flow_kernel in kernels_solve_t.hip; DESIGN.md
// section 4a').  The exchange: values are published with an agent-scope atomic store into vectors that hold the SENTINEL (all bits set) until
// then, and polled with agent-scope atomic loads; every poll is bounded by HS_FLOW_SPIN rounds of s_sleep, and a workgroup whose wait ran out
// raises *err and leaves.  Around it: the claim of a workgroup id in start order, the decode of an interior sub-block, the uniform buffer
// descriptor of a tile, and the round loop over two register tiles.  The tile layouts, loads, reductions, the diagonal-block stage and the
// boundary branches are the kernels' own.
#pragma once
#include "hs_common.h"

#define HS_FLOW_SPIN (1 << 22)
#define HS_FLOW_W 256  // columns of a diagonal block (HS_SW, HS_TW)
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
// thread t's element of a published vector (cnt entries; zero beyond); false when the wait ran out
__device__ __forceinline__ bool flow_poll(const double* src, int cnt, int t, double& v) {
  v = 0.0;
  if (t >= cnt) return true;
  for (int it = 0; it < HS_FLOW_SPIN; ++it) {
    const unsigned long long x = flow_ldbits(src + t);
    if (x != HS_SENT) {
      v = __longlong_as_double((long long)x);
      return true;
    }
    __builtin_amdgcn_s_sleep(1);
  }
  return false;
}
__device__ __forceinline__ bool flow_poll(const cplx* src, int cnt, int t, cplx& v) {
  v = cplx{0.0, 0.0};
  if (t >= cnt) return true;
  const double* p = reinterpret_cast<const double*>(src + t);
  for (int it = 0; it < HS_FLOW_SPIN; ++it) {
    const unsigned long long a = flow_ldbits(p), b = flow_ldbits(p + 1);
    if (a != HS_SENT && b != HS_SENT) {
      v = cplx{__longlong_as_double((long long)a), __longlong_as_double((long long)b)};
      return true;
    }
    __builtin_amdgcn_s_sleep(1);
  }
  return false;
}
// a wait ran out: the host reports it at its next call (pinned host memory: a plain store)
__device__ __forceinline__ void flow_raise(int* err, int t) {
  if (t == 0) *(volatile int*)err = 1;
}

// Workgroup ids are handed out by an atomic counter in the order the workgroups actually start (block-major, front-minor: all fronts of a
// level advance together), so everything a workgroup waits for has started.  (scalar: the front's descriptor and every tile base stay in SGPRs)
struct FlowId {
  int f, sb;  // front of the batch, sub-block of the sweep
};
__device__ __forceinline__ FlowId flow_claim(int* counter, int nbatch) {
  __shared__ int s_id;
  if (threadIdx.x == 0) s_id = atomicAdd(counter, 1);
  __syncthreads();
  const int id = __builtin_amdgcn_readfirstlane(s_id);
  return {id % nbatch, id / nbatch};
}
// interior sub-block sb of a front with ncb column blocks, FB rows (columns) each: column block jb, position q inside it, first row rs and
// row count rl; `reversed`: the sweep starts at the last sub-block
template <int FB>
__device__ __forceinline__ void flow_interior(int sb, int ncb, int ni, bool reversed, int& jb, int& q, int& rs, int& rl) {
  constexpr int Q = HS_FLOW_W / FB;
  jb = reversed ? ncb - 1 - sb / Q : sb / Q;
  q = reversed ? Q - 1 - sb % Q : sb % Q;
  rs = jb * HS_FLOW_W + q * FB;
  rl = min(FB, ni - rs);
}
// the buffer descriptor of a tile at `base` (256 columns of a front: < 2^31 bytes).  It must be PROVABLY uniform or every load becomes a
// waterfall loop: its inputs, and the leading dimension and column count the loads' scalar offsets are made of, go through readfirstlane
template <class T>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t flow_rsrc(const T* base, unsigned& ld, int& ncol) {
  const unsigned long long pb = (unsigned long long)base;
  const unsigned plo = __builtin_amdgcn_readfirstlane((unsigned)pb), phi = __builtin_amdgcn_readfirstlane((unsigned)(pb >> 32));
  ld = __builtin_amdgcn_readfirstlane(ld);
  ncol = __builtin_amdgcn_readfirstlane(ncol);
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<T*>(((unsigned long long)phi << 32) | plo), 0, 0x7FFFFFFF, 0x00020000);
}

// The n rounds of a sub-block over two register tiles.  request(v, c) issues the loads of the tile of round c into v -- for c >= n those of
// what comes after the rounds (the slab of the stored inverse), or nothing -- and round(v, c) waits for the vector of round c and accumulates;
// it returns false when the wait ran out (uniform).  The tiles do not depend on what is waited for, so the tile of the NEXT round is
// requested before this round's vector is polled.  An odd count runs one round on its own first, so that the pairs always end with the tile
// requested last in `va`.  Returns false as soon as a round did.
// (request is one straight run of loads whatever c is: branches there made the compiler keep four tiles alive and spill)
template <class V, int N, class Request, class Round>
__device__ __forceinline__ bool flow_rounds(int n, V (&va)[N], V (&vb)[N], Request&& request, Round&& round) {
  bool alive = true;
  int c = 0;
  if (n & 1) {
    request(va, 0);
    alive = round(va, 0);
    c = 1;
  }
  request(va, c);
  while (c < n && alive) {
    request(vb, c + 1);
    alive = round(va, c);
    request(va, c + 2);  // (c + 2 == n: what follows the rounds, requested before the last vector is waited for)
    if (alive) alive = round(vb, c + 1);
    c += 2;
  }
  return alive;
}
