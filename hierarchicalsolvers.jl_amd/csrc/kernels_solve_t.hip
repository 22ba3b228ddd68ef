// kernels_solve_t.hip -- ldiv!(transpose(F), B) and ldiv!(adjoint(F), B): the sweeps of kernels_solve.hip for op(A) = A^T / A^H.
//
// The same stored blocks (P*Aii = L11*U11, Lbi = Abi*U11^-1 in rows ni.. of LF, Uib = L11^-1*P*Aib in UR, rperm = P) give
//   A = [P' L11, 0; Lbi, I] [U11, Uib; 0, S]   =>   A^T = [U11^T, 0; Uib^T, I] [L11^T P, Lbi^T; 0, S^T]
// so the transposed per-front sweeps are
//   forward  (leaves -> root):  z = U11^-T * rhs[int]              (natural order: no permutation)
//                               rhs[bnd] -= Uib^T * z
//   backward (root -> leaves):  v = z - Lbi^T * rhs[bnd]
//                               rhs[int[rperm[i]]] = (L11^-T * v)[i]
// and A^H conjugates every factor entry that is read (CONJ; Float64 ignores it).  The stored inverses of the diagonal blocks serve
// transposed: (inv256U)^T = (U11_blk^T)^-1, the same for L, so no factor memory is added.
//
// Every product here reads a factor block along its COLUMNS (a row of op(A) is a column of the stored block, contiguous over the
// reduction index): the lanes walk the contiguous reduction index, keep partial sums, and meet in a fixed xor butterfly once per output
// (the dataflow sweep: once per owned column after its last round).  No atomics on values, fixed order: bitwise reproducible results.
// The triangular sweeps of a tree level run as ONE dataflow launch (t_flow_kernel, the transposed counterpart of flow_sweep_kernel);
// HS_SOLVE_FLOW=0 selects one pair of launches per 256-column diagonal block instead (t_diag_kernel + t_update_kernel: the yardstick).
#include "hs_common.h"
#include "hs_flow.h"

#define HS_TW 256  // columns per sweep step (the stored inverses of the 256 x 256 diagonal blocks)
static_assert(HS_TW == HS_FLOW_W, "flow_interior decodes sub-blocks of HS_FLOW_W columns");
#define HS_TCPW 8  // output columns per wavefront and pass of a workgroup (4 wavefronts: 32 columns per workgroup)
#define HS_TCH 1024  // reduction entries staged in LDS per chunk

template <bool CONJ>
__device__ __forceinline__ double cj(double v) {
  return v;
}
template <bool CONJ>
__device__ __forceinline__ cplx cj(cplx v) {
  return CONJ ? cplx{v.re, -v.im} : v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ cplx wave_sum(cplx v) { return {wave_sum(v.re), wave_sum(v.im)}; }

// (gather and scatter: sweep_gather_kernel / sweep_scatter_kernel of kernels_solve.hip, with the row permutation on the scatter)

// ---- diagonal block: dst[c0 + c] = sum_k cj(inv[k + c * 256]) * src[c0 + k] ------------------------------
// UPPER: inv = inv256U of block blk (upper triangular: k <= c), else inv256L (lower: k >= c).  grid.x = 8 (32 output columns each).
template <class T, bool CONJ, bool UPPER>
__global__ __launch_bounds__(256) void t_diag_kernel(const SolveNode<T>* __restrict__ nodes, int blk, const T* __restrict__ src, T* __restrict__ dst) {
  const SolveNode<T> nd = nodes[blockIdx.y];
  const int c0 = blk * HS_TW;
  if (c0 >= nd.ni) return;
  const int wl = min(HS_TW, nd.ni - c0);
  __shared__ T s_x[HS_TW];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  s_x[t] = t < wl ? src[nd.woff + c0 + t] : Scal<T>::zero();
  __syncthreads();
  const T* inv = (UPPER ? nd.inv256U : nd.inv256L) + (size_t)blk * HS_TW * HS_TW;
  for (int q = 0; q < HS_TCPW; ++q) {
    const int c = blockIdx.x * (4 * HS_TCPW) + wv * HS_TCPW + q;
    if (c >= wl) break;  // uniform over the wavefront
    const int klo = UPPER ? 0 : c, khi = UPPER ? c + 1 : wl;  // the triangle only: the other one is not stored inside the 32-blocks
    const T* col = inv + (size_t)c * HS_TW;
    T acc = Scal<T>::zero();
    for (int k = klo + lane; k < khi; k += 64) acc = Scal<T>::fma(cj<CONJ>(gld(col + k)), s_x[k], acc);
    acc = wave_sum(acc);
    if (lane == 0) dst[nd.woff + c0 + c] = acc;
  }
}

// ---- panel update of one sweep step: for every column j of the range, out_j -= sum_{k < wl} cj(A[c0 + k, j]) * x[k] ------------
// UPPER (forward): j in [c0 + wl, mrows): j < ni: A = U11 (LF), out = w[j];  j >= ni: A = Uib (UR, column j - ni), out = b[fidx[j]].
// !UPPER (backward): j in [0, c0): A = L11 (LF), out = w[j].   x = the block's solved values (xs[c0 ..]).  grid.x covers 32 columns.
template <class T, bool CONJ, bool UPPER>
__global__ __launch_bounds__(256) void t_update_kernel(const SolveNode<T>* __restrict__ nodes, int blk, const T* __restrict__ xs, T* __restrict__ w,
                                                       T* __restrict__ b) {
  const SolveNode<T> nd = nodes[blockIdx.y];
  const int c0 = blk * HS_TW;
  if (c0 >= nd.ni) return;
  const int wl = min(HS_TW, nd.ni - c0);
  const int jlo = UPPER ? c0 + wl : 0, jhi = UPPER ? nd.mrows : c0;
  const int jw = jlo + (int)blockIdx.x * (4 * HS_TCPW);
  if (jw >= jhi) return;
  __shared__ T s_x[HS_TW];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  s_x[t] = t < wl ? xs[nd.woff + c0 + t] : Scal<T>::zero();
  __syncthreads();
  T acc[HS_TCPW];
#pragma unroll
  for (int q = 0; q < HS_TCPW; ++q) {
    acc[q] = Scal<T>::zero();
    const int j = jw + wv * HS_TCPW + q;
    if (j >= jhi) continue;
    const T* a = (UPPER && j >= nd.ni) ? nd.UR + (size_t)c0 + (size_t)(j - nd.ni) * nd.ldu : nd.LF + (size_t)c0 + (size_t)j * nd.ldl;
#pragma unroll
    for (int u = 0; u < HS_TW / 64; ++u) {
      const int k = lane + 64 * u;
      if (k < wl) acc[q] = Scal<T>::fma(cj<CONJ>(gld(a + k)), s_x[k], acc[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < HS_TCPW; ++q) {
    const int j = jw + wv * HS_TCPW + q;
    const T s = wave_sum(acc[q]);
    if (j >= jhi || lane != 0) continue;
    if (!UPPER || j < nd.ni) {
      w[nd.woff + j] = w[nd.woff + j] - s;
    } else {
      const int g = gld(nd.fidx + j);
      b[g] = b[g] - s;
    }
  }
}

// ---- v = z - Lbi^T * rhs[bnd] (dense fronts; compressed fronts: v = z, the low-rank kernels below take the rest) -------------
// Column i of Lbi is nb consecutive entries of LF (rows ni..m-1); rhs[bnd] is staged in LDS HS_TCH entries at a time.  grid.x covers 32
// columns.
template <class T, bool CONJ>
__global__ __launch_bounds__(256) void t_int_update_kernel(const SolveNode<T>* __restrict__ nodes, const T* __restrict__ b, const T* __restrict__ z,
                                                           T* __restrict__ v) {
  const SolveNode<T> nd = nodes[blockIdx.y];
  const int iw = (int)blockIdx.x * (4 * HS_TCPW);
  if (iw >= nd.ni) return;
  const int nb = nd.compressed ? 0 : nd.nb;
  __shared__ T s_x[HS_TCH];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  T acc[HS_TCPW];
#pragma unroll
  for (int q = 0; q < HS_TCPW; ++q) acc[q] = Scal<T>::zero();
  for (int j0 = 0; j0 < nb; j0 += HS_TCH) {
    const int jn = min(HS_TCH, nb - j0);
    __syncthreads();
    for (int j = t; j < jn; j += 256) s_x[j] = b[gld(nd.fidx + nd.ni + j0 + j)];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < HS_TCPW; ++q) {
      const int i = iw + wv * HS_TCPW + q;
      if (i >= nd.ni) continue;
      const T* a = nd.LF + (size_t)nd.ni + (size_t)j0 + (size_t)i * nd.ldl;
      for (int j = lane; j < jn; j += 64) acc[q] = Scal<T>::fma(cj<CONJ>(gld(a + j)), s_x[j], acc[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < HS_TCPW; ++q) {
    const int i = iw + wv * HS_TCPW + q;
    const T s = wave_sum(acc[q]);
    if (i < nd.ni && lane == 0) v[nd.woff + i] = z[nd.woff + i] - s;
  }
}

// ---- low-rank Gauss transforms, transposed ------------------------------------------------------------------------------
// C (rows x r) is the dense C in original row order (every compressed front keeps it: lowrank_expand, hs_lrdense.hip; the host refuses one
// without it).  part[s * r + c] = sum over the rows of chunk s of cj(C[row, c]) * x[xidx ? xidx[row] : row]   (grid: (ceil(r / 32), chunks of HS_TCH))
template <class T, bool CONJ>
__global__ __launch_bounds__(256) void t_lr_ct_partial_kernel(const T* __restrict__ Cd, int ldc, int rows, int r, const T* __restrict__ x,
                                                              const int* __restrict__ xidx, T* __restrict__ part) {
  const int p0 = blockIdx.y * HS_TCH, pn = min(HS_TCH, rows - p0);
  __shared__ T s_x[HS_TCH];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  for (int p = t; p < pn; p += 256) s_x[p] = x[xidx ? xidx[p0 + p] : p0 + p];
  __syncthreads();
  T acc[HS_TCPW];
#pragma unroll
  for (int q = 0; q < HS_TCPW; ++q) {
    acc[q] = Scal<T>::zero();
    const int c = blockIdx.x * (4 * HS_TCPW) + wv * HS_TCPW + q;
    if (c >= r) continue;
    const T* a = Cd + (size_t)p0 + (size_t)c * ldc;
    for (int p = lane; p < pn; p += 64) acc[q] = Scal<T>::fma(cj<CONJ>(a[p]), s_x[p], acc[q]);
  }
#pragma unroll
  for (int q = 0; q < HS_TCPW; ++q) {
    const int c = blockIdx.x * (4 * HS_TCPW) + wv * HS_TCPW + q;
    const T s = wave_sum(acc[q]);
    if (c < r && lane == 0) part[(size_t)blockIdx.y * r + c] = s;
  }
}
template <class T>
__global__ __launch_bounds__(256) void t_lr_reduce_kernel(const T* __restrict__ part, int r, int ns, T* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= r) return;
  T acc = Scal<T>::zero();
  for (int s = 0; s < ns; ++s) acc = acc + part[(size_t)s * r + c];
  out[c] = acc;
}
// dst[didx ? didx[j] : j] -= sum_c cj(Z[c + j * ldz]) * t[c],  j < cols   (column j of Z is r consecutive entries; grid.x covers 32 columns)
template <class T, bool CONJ>
__global__ __launch_bounds__(256) void t_lr_zt_kernel(const T* __restrict__ Z, int ldz, int r, int cols, const T* __restrict__ tv, T* __restrict__ dst,
                                                      const int* __restrict__ didx) {
  const int jw = (int)blockIdx.x * (4 * HS_TCPW);
  __shared__ T s_t[HS_TCH];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  T acc[HS_TCPW];
#pragma unroll
  for (int q = 0; q < HS_TCPW; ++q) acc[q] = Scal<T>::zero();
  for (int c0 = 0; c0 < r; c0 += HS_TCH) {
    const int cn = min(HS_TCH, r - c0);
    __syncthreads();
    for (int c = t; c < cn; c += 256) s_t[c] = tv[c0 + c];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < HS_TCPW; ++q) {
      const int j = jw + wv * HS_TCPW + q;
      if (j >= cols) continue;
      const T* a = Z + (size_t)c0 + (size_t)j * ldz;
      for (int c = lane; c < cn; c += 64) acc[q] = Scal<T>::fma(cj<CONJ>(a[c]), s_t[c], acc[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < HS_TCPW; ++q) {
    const int j = jw + wv * HS_TCPW + q;
    const T s = wave_sum(acc[q]);
    if (j >= cols || lane != 0) continue;
    const int g = didx ? didx[j] : j;
    dst[g] = dst[g] - s;
  }
}

// ---- the dataflow sweep of one level (HS_SOLVE_FLOW=1, the default) ------------------------------------------------------------
// FWD: z = U11^-T w (w = rhs[int] gathered) and rhs[bnd] -= Uib^T z;  !FWD: x = L11^-T v (v = z - Lbi^T rhs[bnd]).  The skeleton of
// flow_sweep_kernel, shared through hs_flow.h (flow_claim, flow_interior, flow_poll, flow_rounds, flow_raise, flow_publish): workgroup ids from an atomic counter in start order (block-major, front-minor), values published into the sentinel-armed
// exchange vectors (E1: z / x, E2: the finished w of a diagonal block) and polled with bounded waits (*err on run-out), the tile of the next
// round requested before this round's vector is waited for.  What changes is the tile: a workgroup OWNS FB output columns [rs, rs + FB) --
// columns of U11 (Uib, L11) -- and reads them over the rows of one 256-block per round, so the 256 threads run along the rows (the contiguous,
// reduction dimension: coalesced, one scalar column base per load) and every thread keeps FB partial sums, one per column, across all rounds.
// They meet once, after the last round, in a fixed butterfly per wavefront and a fixed-order sum over the four wavefronts.  The diagonal block
// multiplies by columns [q FB, q FB + FB) of the stored inverse -- the transposed slab of inv256U (inv256L) -- with the same tile shape.
template <class T>
struct TFlowCfg {
  static constexpr int NT = 256;                       // threads: thread t owns row t of every 256-row tile
  static constexpr int FB = sizeof(T) == 8 ? 32 : 16;  // output columns a workgroup owns: 32 data registers per thread and tile either way
  static constexpr int Q = HS_TW / FB;                 // sub-blocks per 256-column block
};
// the thread's row of a tile: element (row t, column c) of base (ld), rows clamped to nrow, columns to ncol (what a clamped load brings in is
// multiplied by a zero of the vector or lands in a column nobody stores).  `base` and `ld` are workgroup-uniform: scalar column offsets.
template <class T, int FB>
__device__ __forceinline__ void t_load(T (&v)[FB], const T* base, size_t ld, int ncol, int nrow, int t) {
  const T* p = base + min(t, nrow - 1);
#pragma unroll
  for (int c = 0; c < FB; ++c) v[c] = gld(p + (size_t)min(c, ncol - 1) * ld);
}
// sum over the workgroup of the FB partial sums; the result for column t is returned to thread t < FB (fixed order)
template <class T, int FB>
__device__ __forceinline__ T t_reduce(const T (&acc)[FB], T* s_red, int t) {
  const int lane = t & 63, wv = t >> 6;
#pragma unroll
  for (int c = 0; c < FB; ++c) {
    const T s = wave_sum(acc[c]);
    if (lane == 0) s_red[wv * FB + c] = s;
  }
  __syncthreads();
  T v = Scal<T>::zero();
  if (t < FB) v = ((s_red[t] + s_red[FB + t]) + s_red[2 * FB + t]) + s_red[3 * FB + t];
  __syncthreads();  // s_red is used again
  return v;
}
template <class T, bool CONJ, bool FWD>
__global__ __launch_bounds__(256) void t_flow_kernel(const SolveNode<T>* __restrict__ nodes, int nbatch, const T* __restrict__ w, T* __restrict__ out,
                                                     T* __restrict__ b, T* __restrict__ E1, T* __restrict__ E2, int* __restrict__ counter, int* __restrict__ err) {
  constexpr int FB = TFlowCfg<T>::FB, Q = TFlowCfg<T>::Q;
  __shared__ T s_red[4 * FB];
  __shared__ T s_own[FB];
  const int t = threadIdx.x;
  const FlowId id = flow_claim(counter, nbatch);
  const int sb = id.sb;
  const SolveNode<T> nd = nodes[id.f];
  if (nd.ni <= 0) return;
  const int ncb = (nd.ni + HS_TW - 1) / HS_TW;
  const bool interior = sb < Q * ncb;
  if (!FWD && !interior) return;
  int jb, q, rs, rl;
  if (interior) {
    flow_interior<FB>(sb, ncb, nd.ni, !FWD, jb, q, rs, rl);
  } else {  // boundary columns [rs, rs + FB) of Uib: every interior block feeds them
    jb = ncb;
    q = 0;
    rs = (sb - Q * ncb) * FB;
    rl = min(FB, nd.mrows - nd.ni - rs);
  }
  if (rl <= 0) return;
  // the tile of round c: rows of block kb(c) of the owned columns (FWD: U11 / Uib above the block, !FWD: L11 below it)
  const int nr = FWD ? jb : ncb - 1 - jb;
  const T* cbase = interior ? nd.LF + (size_t)rs * nd.ldl : nd.UR + (size_t)rs * nd.ldu;
  const size_t cld = interior ? (size_t)nd.ldl : (size_t)nd.ldu;
  T acc[FB], va[FB], vb[FB];
#pragma unroll
  for (int c = 0; c < FB; ++c) acc[c] = Scal<T>::zero();
  auto request = [&](T(&v)[FB], int c) {
    if (c >= nr) return;
    const int kb = FWD ? c : ncb - 1 - c;
    t_load<T, FB>(v, cbase + (size_t)kb * HS_TW, cld, rl, min(HS_TW, nd.ni - kb * HS_TW), t);
  };
  auto round = [&](const T(&v)[FB], int c) -> bool {
    const int kb = FWD ? c : ncb - 1 - c;
    T x;
    const bool ok = flow_poll(E1 + nd.woff + (size_t)kb * HS_TW, min(HS_TW, nd.ni - kb * HS_TW), t, x);
    if (__builtin_amdgcn_readfirstlane(__syncthreads_or(ok ? 0 : 1))) return false;
#pragma unroll
    for (int cc = 0; cc < FB; ++cc) acc[cc] = Scal<T>::fma(cj<CONJ>(v[cc]), x, acc[cc]);
    return true;
  };
  if (!flow_rounds(nr, va, vb, request, round)) return flow_raise(err, t);
  const int wlj = interior ? min(HS_TW, nd.ni - jb * HS_TW) : 1;
  const T* inv = (FWD ? nd.inv256U : nd.inv256L) + (size_t)jb * HS_TW * HS_TW + (size_t)(q * FB) * HS_TW;
  if (interior) t_load<T, FB>(va, inv, HS_TW, rl, wlj, t);  // the slab of the inverse, in flight during the reduction
  const T s = t_reduce<T, FB>(acc, s_red, t);
  if (!interior) {
    if (t < rl) {
      const int g = gld(nd.fidx + nd.ni + rs + t);
      b[g] = b[g] - s;
    }
    return;
  }
  if (t < rl) {
    const T wfin = w[nd.woff + rs + t] - s;
    flow_publish(E2 + nd.woff + rs + t, wfin);
    s_own[t] = wfin;
  }
  __syncthreads();
  // element t of the block's finished w, for the triangle of the slab: FWD rows <= the columns (sub-blocks <= q), !FWD rows >= them (>= q)
  const int own_lo = q * FB, lo = FWD ? 0 : own_lo, hi = FWD ? own_lo + rl : wlj;
  T x = Scal<T>::zero();
  bool ok = true;
  if (t >= own_lo && t < own_lo + rl)
    x = s_own[t - own_lo];
  else if (t >= lo && t < hi)
    ok = flow_poll(E2 + nd.woff + (size_t)jb * HS_TW, hi, t, x);
  if (__builtin_amdgcn_readfirstlane(__syncthreads_or(ok ? 0 : 1))) return flow_raise(err, t);
#pragma unroll
  for (int cc = 0; cc < FB; ++cc) {
    const int col = own_lo + cc;
    const bool in = t < wlj && (FWD ? t <= col : t >= col);  // (the other triangle of the diagonal 32-blocks is not stored)
    acc[cc] = Scal<T>::fma(in ? cj<CONJ>(va[cc]) : Scal<T>::zero(), x, Scal<T>::zero());
  }
  const T z = t_reduce<T, FB>(acc, s_red, t);
  if (t < rl) {
    flow_publish(E1 + nd.woff + rs + t, z);
    out[nd.woff + rs + t] = z;
  }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
static inline int t_groups(int cols) { return (cols + 4 * HS_TCPW - 1) / (4 * HS_TCPW); }

int hs_solve_t_cols() { return HS_TW; }
template <class T, bool CONJ>
void launch_t_fwd_step(const SolveNode<T>* dn, int nbatch, int blk, int maxm, T* w, T* z, T* b, hipStream_t s) {
  if (nbatch <= 0) return;
  hipLaunchKernelGGL((t_diag_kernel<T, CONJ, true>), dim3(HS_TW / (4 * HS_TCPW), nbatch), dim3(256), 0, s, dn, blk, (const T*)w, z);
  const int cols = maxm - blk * HS_TW;
  if (cols > 0) hipLaunchKernelGGL((t_update_kernel<T, CONJ, true>), dim3(t_groups(cols), nbatch), dim3(256), 0, s, dn, blk, (const T*)z, w, b);
}
template <class T, bool CONJ>
void launch_t_bwd_step(const SolveNode<T>* dn, int nbatch, int blk, T* v, T* x, hipStream_t s) {
  if (nbatch <= 0) return;
  hipLaunchKernelGGL((t_diag_kernel<T, CONJ, false>), dim3(HS_TW / (4 * HS_TCPW), nbatch), dim3(256), 0, s, dn, blk, (const T*)v, x);
  const int cols = blk * HS_TW;
  if (cols > 0) hipLaunchKernelGGL((t_update_kernel<T, CONJ, false>), dim3(t_groups(cols), nbatch), dim3(256), 0, s, dn, blk, (const T*)x, v, (T*)nullptr);
}
template <class T, bool CONJ>
void launch_t_fwd_flow(const SolveNode<T>* dn, int nbatch, int maxni, int maxnb, const T* w, T* z, T* b, T* E1, T* E2, int* counter, int* err, hipStream_t s) {
  if (nbatch <= 0 || maxni <= 0) return;
  constexpr int FB = TFlowCfg<T>::FB;
  const int nsb = TFlowCfg<T>::Q * ((maxni + HS_TW - 1) / HS_TW) + (std::max(maxnb, 0) + FB - 1) / FB;
  hipLaunchKernelGGL((t_flow_kernel<T, CONJ, true>), dim3((unsigned)nsb * (unsigned)nbatch), dim3(TFlowCfg<T>::NT), 0, s, dn, nbatch, w, z, b, E1, E2, counter, err);
}
template <class T, bool CONJ>
void launch_t_bwd_flow(const SolveNode<T>* dn, int nbatch, int maxni, const T* v, T* x, T* E1, T* E2, int* counter, int* err, hipStream_t s) {
  if (nbatch <= 0 || maxni <= 0) return;
  const int nsb = TFlowCfg<T>::Q * ((maxni + HS_TW - 1) / HS_TW);
  hipLaunchKernelGGL((t_flow_kernel<T, CONJ, false>), dim3((unsigned)nsb * (unsigned)nbatch), dim3(TFlowCfg<T>::NT), 0, s, dn, nbatch, v, x, (T*)nullptr, E1, E2, counter, err);
}
template <class T, bool CONJ>
void launch_t_int_update(const SolveNode<T>* dn, int nbatch, int maxni, const T* b, const T* z, T* v, hipStream_t s) {
  if (nbatch <= 0 || maxni <= 0) return;
  hipLaunchKernelGGL((t_int_update_kernel<T, CONJ>), dim3(t_groups(maxni), nbatch), dim3(256), 0, s, dn, b, z, v);
}
// t = C^T x (two passes, fixed order); `part` holds ceil(rows / HS_TCH) * r entries
template <class T, bool CONJ>
void launch_t_lr_ct(const T* Cd, int ldc, int rows, int r, const T* x, const int* xidx, T* part, T* t, hipStream_t s) {
  if (r <= 0) return;
  const int ns = (rows + HS_TCH - 1) / HS_TCH;
  if (ns > 0) hipLaunchKernelGGL((t_lr_ct_partial_kernel<T, CONJ>), dim3(t_groups(r), ns), dim3(256), 0, s, Cd, ldc, rows, r, x, xidx, part);
  hipLaunchKernelGGL(t_lr_reduce_kernel<T>, dim3((r + 255) / 256), dim3(256), 0, s, (const T*)part, r, ns, t);
}
int hs_lr_ct_part_elems(int rows, int r) { return ((rows + HS_TCH - 1) / HS_TCH) * r; }
template <class T, bool CONJ>
void launch_t_lr_zt(const T* Z, int ldz, int r, int cols, const T* t, T* dst, const int* didx, hipStream_t s) {
  if (r <= 0 || cols <= 0) return;
  hipLaunchKernelGGL((t_lr_zt_kernel<T, CONJ>), dim3(t_groups(cols)), dim3(256), 0, s, Z, ldz, r, cols, t, dst, didx);
}

#define INST_TC(T, C)                                                                                                                   \
  template void launch_t_fwd_step<T, C>(const SolveNode<T>*, int, int, int, T*, T*, T*, hipStream_t);                                  \
  template void launch_t_bwd_step<T, C>(const SolveNode<T>*, int, int, T*, T*, hipStream_t);                                           \
  template void launch_t_fwd_flow<T, C>(const SolveNode<T>*, int, int, int, const T*, T*, T*, T*, T*, int*, int*, hipStream_t);        \
  template void launch_t_bwd_flow<T, C>(const SolveNode<T>*, int, int, const T*, T*, T*, T*, int*, int*, hipStream_t);                 \
  template void launch_t_int_update<T, C>(const SolveNode<T>*, int, int, const T*, const T*, T*, hipStream_t);                        \
  template void launch_t_lr_ct<T, C>(const T*, int, int, int, const T*, const int*, T*, T*, hipStream_t);                            \
  template void launch_t_lr_zt<T, C>(const T*, int, int, int, const T*, T*, const int*, hipStream_t);
INST_TC(double, false)
INST_TC(cplx, false)
INST_TC(cplx, true)
