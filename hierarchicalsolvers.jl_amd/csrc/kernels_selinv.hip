// kernels_selinv.hip -- the kernels of hs_logabsdet and hs_selinv (hs_selinv.hip) that are not matrix products:
//
//   logdet_kernel        per front: sum log|u_kk|, the phase of prod u_kk, the parity of the row permutation   (one launch per handle)
//   zinit_kernel         Vi = I                                  (the right-hand side of U X = I; the rest of the work blocks is cleared by a memset)
//   zload_lr_kernel      Vg = G, Tm[nit.., :] = Z_L'             (hs_selinv_lr: the stored low-rank factors are copied, the substitutions overwrite the copies)
//   zgather_kernel       child Z[bnd, bnd] = parent Z[cmap, cmap]   (the reverse of scatter_kernel's extend-add)
//   zpermute_cols_kernel Z[:, rperm[i]] = X2[:, i]                  (the trailing P of (T L^-1) P, fused with the write into the Z block)
//   zextract_kernel      diag[fidx[i]] = Z[i, i];  zval[e] = Z[pr, pc] (or its transpose) for the entries of A the front owns
//
// All of them are grouped over the fronts of a batch (blockIdx.y or .z = front, descriptors read from memory) and move data column-major with
// the row index on the lanes, so loads and stores of a wave are contiguous; ComplexF64 moves as 16-byte accesses through gld / gst.
#include <algorithm>

#include "hs_selinv.h"

// ------------------------------------------------------------------------------------------------
// log-determinant
// ------------------------------------------------------------------------------------------------
// One workgroup per front.  Every thread walks the diagonal with stride 256 (a fixed order), the 256 partial results meet in a fixed
// tree: two calls return the same bits.  The parity of P comes from the cycles of rperm (maintained by every pivoting path, it is what
// ldiv! reads): a permutation of ni elements with c cycles is odd iff ni - c is.  Element i is counted as the head of its cycle when
// the walk from i comes back without meeting a smaller index; the walk stops at the first smaller index, which keeps it short for the
// permutations pivoting produces (few displaced rows; an identity costs one load per element).
template <class T>
__device__ inline void logdet_term(T u, double& la, double& ang, int& neg, int& zero);
template <>
__device__ inline void logdet_term<double>(double u, double& la, double& ang, int& neg, int& zero) {
  if (u == 0.0) { zero = 1; return; }
  la += log(fabs(u));
  neg += u < 0.0 ? 1 : 0;
  (void)ang;
}
template <>
__device__ inline void logdet_term<cplx>(cplx u, double& la, double& ang, int& neg, int& zero) {
  if (u.re == 0.0 && u.im == 0.0) { zero = 1; return; }
  la += log(hypot(u.re, u.im));
  ang += atan2(u.im, u.re);  // a sum of angles never under- or overflows; the host reduces it modulo 2 pi
  (void)neg;
}

template <class T>
__global__ __launch_bounds__(256) void logdet_kernel(const LogdetFront* __restrict__ fronts, LogdetOut* __restrict__ out) {
  __shared__ double s_la[256], s_ang[256];
  __shared__ int s_neg[256], s_cyc[256], s_zero[256];
  const LogdetFront f = fronts[blockIdx.x];
  const T* LU = (const T*)f.LU;
  const int t = threadIdx.x;
  double la = 0.0, ang = 0.0;
  int neg = 0, cyc = 0, zero = 0;
  for (int i = t; i < f.ni; i += 256) {
    logdet_term<T>(gld(LU + (size_t)i * f.ld + i), la, ang, neg, zero);
    int j = f.rperm[i], steps = 0;
    while (j > i && steps < f.ni) {  // (bounded: a corrupt list cannot hang the kernel)
      j = f.rperm[j];
      ++steps;
    }
    cyc += (j == i) ? 1 : 0;
  }
  s_la[t] = la; s_ang[t] = ang; s_neg[t] = neg; s_cyc[t] = cyc; s_zero[t] = zero;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (t < w) {
      s_la[t] += s_la[t + w]; s_ang[t] += s_ang[t + w];
      s_neg[t] += s_neg[t + w]; s_cyc[t] += s_cyc[t + w]; s_zero[t] |= s_zero[t + w];
    }
    __syncthreads();
  }
  if (t == 0) {
    LogdetOut o;
    o.logabs = s_la[0]; o.angle = s_ang[0]; o.neg = s_neg[0]; o.odd = (f.ni - s_cyc[0]) & 1; o.zero = s_zero[0]; o.pad = 0;
    out[blockIdx.x] = o;
  }
}

template <class T>
void launch_logdet(const LogdetFront* df, int nfronts, LogdetOut* out, hipStream_t s) {
  if (nfronts <= 0) return;
  hipLaunchKernelGGL(logdet_kernel<T>, dim3(nfronts), dim3(256), 0, s, df, out);
}
template void launch_logdet<double>(const LogdetFront*, int, LogdetOut*, hipStream_t);
template void launch_logdet<cplx>(const LogdetFront*, int, LogdetOut*, hipStream_t);

// The determinant of a ULV-eliminated HSS matrix (hs_hss_logabsdet): det H = det(root LU) * prod over the eliminated nodes of det(X_RR),
// every factor read from the diagonal of a node's pivoted LU and the parity of its rperm, as above.  The nodes of an HSS tree are many and
// small (at most a leaf size of eliminated rows each, the root a few ranks), so a node is one wave: lane l walks the diagonal entries
// l, l + 64, ... in order, and the 64 partial results meet in the fixed shuffle tree below -- no LDS, no barrier, no atomics, and two
// calls return the same bits.  ni = 0 writes the neutral element.
template <class T>
__global__ __launch_bounds__(64) void ulv_det_kernel(const LogdetFront* __restrict__ nodes, LogdetOut* __restrict__ out) {
  const LogdetFront f = nodes[blockIdx.x];
  const T* LU = (const T*)f.LU;
  const int l = threadIdx.x;
  double la = 0.0, ang = 0.0;
  int neg = 0, cyc = 0, zero = 0;
  for (int i = l; i < f.ni; i += 64) {
    logdet_term<T>(gld(LU + (size_t)i * f.ld + i), la, ang, neg, zero);
    int j = f.rperm[i], steps = 0;
    while (j > i && j < f.ni && steps < f.ni) {  // (bounded, and an entry outside 0:ni-1 ends the walk: a corrupt list can neither hang nor stray)
      j = f.rperm[j];
      ++steps;
    }
    cyc += (j == i) ? 1 : 0;
  }
  for (int w = 32; w >= 1; w >>= 1) {
    la += __shfl_down(la, w, 64);
    ang += __shfl_down(ang, w, 64);
    neg += __shfl_down(neg, w, 64);
    cyc += __shfl_down(cyc, w, 64);
    zero |= __shfl_down(zero, w, 64);
  }
  if (l == 0) {
    LogdetOut o;
    o.logabs = la; o.angle = ang; o.neg = neg; o.odd = (f.ni - cyc) & 1; o.zero = zero; o.pad = 0;
    out[blockIdx.x] = o;
  }
}

template <class T>
void launch_ulv_det(const LogdetFront* dn, int nnodes, LogdetOut* out, hipStream_t s) {
  if (nnodes <= 0) return;
  hipLaunchKernelGGL(ulv_det_kernel<T>, dim3(nnodes), dim3(64), 0, s, dn, out);
}
template void launch_ulv_det<double>(const LogdetFront*, int, LogdetOut*, hipStream_t);
template void launch_ulv_det<cplx>(const LogdetFront*, int, LogdetOut*, hipStream_t);

// ------------------------------------------------------------------------------------------------
// selected inversion
// ------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void zinit_kernel(const SelDesc<T>* __restrict__ descs) {
  const SelDesc<T> d = descs[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < d.ni) gst(d.Vi + (size_t)i * d.ldv + i, Scal<T>::one());
}
template <class T>
void launch_zinit(const SelDesc<T>* d, int nbatch, int maxni, hipStream_t s) {
  if (nbatch <= 0 || maxni <= 0) return;
  hipLaunchKernelGGL(zinit_kernel<T>, dim3((maxni + 255) / 256, nbatch), dim3(256), 0, s, d);
}

// hs_selinv_lr: the right-hand sides of a low-rank front's substitutions are COPIES of its stored factors (the substitutions overwrite
// them): part 0 (blockIdx.z) copies G (ni x rR) into Vg = Vi + ni ldv, part 1 copies Z_L' (rL x ni) into rows nit.. of Tm.  A wave owns a
// column at a time, its lanes run along the leading dimension.  Float64 moves two rows per lane as one 16-byte access when source and
// destination column share their 16-byte phase (every ld is even, so all columns of a block have the phase of the first one): a scalar
// head element up to the boundary, the pairs, a scalar tail; with different phases every access is 8 bytes.  ComplexF64 elements are
// 16 bytes each.  A dense front of a mixed batch has rR = rL = 0 and leaves at once.
template <class T>
__device__ inline void zload_col(const T* __restrict__ src, T* __restrict__ dst, int rows, int lane) {
  for (int r = lane; r < rows; r += 64) gst(dst + r, gld(src + r));
}
template <>
__device__ inline void zload_col<double>(const double* __restrict__ src, double* __restrict__ dst, int rows, int lane) {
  const unsigned ps = (unsigned)((uintptr_t)src & 15), pd = (unsigned)((uintptr_t)dst & 15);
  if (ps != pd) {
    for (int r = lane; r < rows; r += 64) gst(dst + r, gld(src + r));
    return;
  }
  const int head = ps ? 1 : 0;  // (elements are 8-byte aligned: the phase is 0 or 8)
  if (head && lane == 0 && rows > 0) gst(dst, gld(src));
  const int pairs = (rows - head) / 2;
  for (int q = lane; q < pairs; q += 64) {
    const hs_d2u v = gld2(src + head + 2 * q);
    *(hs_d2u HS_AS_GLOBAL*)(dst + head + 2 * q) = v;
  }
  const int done = head + 2 * pairs;
  if (done < rows && lane == 0) gst(dst + done, gld(src + done));
}
template <class T>
__global__ __launch_bounds__(256) void zload_lr_kernel(const SelDesc<T>* __restrict__ descs) {
  const SelDesc<T> d = descs[blockIdx.y];
  const T* src;
  T* dst;
  int rows, cols, lds, ldd;
  if (blockIdx.z == 0) {
    src = d.G; lds = d.ldg; dst = d.Vi + (size_t)d.ldv * d.ni; ldd = d.ldv; rows = d.ni; cols = d.rR;
  } else {
    src = d.ZL; lds = d.ldzl; dst = d.Tm + d.nit; ldd = d.ldt; rows = d.rL; cols = d.ni;
  }
  if (!src || rows <= 0 || cols <= 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = blockIdx.x * 4 + wave; c < cols; c += gridDim.x * 4) zload_col<T>(src + (size_t)c * lds, dst + (size_t)c * ldd, rows, lane);
}
template <class T>
void launch_zload_lr(const SelDesc<T>* d, int nbatch, int maxni, int maxr, hipStream_t s) {
  if (nbatch <= 0 || maxni <= 0 || maxr <= 0) return;
  const int gx = std::min((std::max(maxni, maxr) + 3) / 4, 256);
  hipLaunchKernelGGL(zload_lr_kernel<T>, dim3(gx, nbatch, 2), dim3(256), 0, s, d);
}

// A workgroup owns 256 destination rows a and ZG_COLS destination columns b: cmap of both ranges is staged in LDS once, then every
// column is one contiguous store of 256 elements (the loads follow cmap, which is piecewise contiguous: the child's boundary keeps its
// order inside the parent's interior and boundary parts).
#define ZG_COLS 32
template <class T>
__global__ __launch_bounds__(256) void zgather_kernel(const SelDesc<T>* __restrict__ descs) {
  __shared__ int s_row[256], s_col[ZG_COLS];
  const SelDesc<T> d = descs[blockIdx.z];
  if (!d.Zp || d.nb <= 0) return;
  const int a0 = blockIdx.x * 256, b0 = blockIdx.y * ZG_COLS;
  if (a0 >= d.nb || b0 >= d.nb) return;
  const int t = threadIdx.x, a = a0 + t;
  s_row[t] = a < d.nb ? d.cmap[a] : 0;
  if (t < ZG_COLS) s_col[t] = (b0 + t < d.nb) ? d.cmap[b0 + t] : 0;
  __syncthreads();
  if (a >= d.nb) return;
  const int nc = min(ZG_COLS, d.nb - b0);
  const T* src = d.Zp + s_row[t];
  T* dst = d.Z + (size_t)(d.ni + a) + (size_t)(d.ni + b0) * d.ldz;
#pragma unroll 4
  for (int b = 0; b < nc; ++b) gst(dst + (size_t)b * d.ldz, gld(src + (size_t)s_col[b] * d.ldzp));
}
template <class T>
void launch_zgather(const SelDesc<T>* d, int nbatch, int maxnb, hipStream_t s) {
  if (nbatch <= 0 || maxnb <= 0) return;
  hipLaunchKernelGGL(zgather_kernel<T>, dim3((maxnb + 255) / 256, (maxnb + ZG_COLS - 1) / ZG_COLS, nbatch), dim3(256), 0, s, d);
}

// Z[r, rperm[i]] = X2[r, i] for every row r of the front and every interior column i: 256 rows x ZG_COLS columns per workgroup, the
// targets of the columns staged in LDS.  rperm is a permutation of 0:ni-1, so every interior column of Z is written exactly once.
template <class T>
__global__ __launch_bounds__(256) void zpermute_cols_kernel(const SelDesc<T>* __restrict__ descs) {
  __shared__ int s_to[ZG_COLS];
  const SelDesc<T> d = descs[blockIdx.z];
  const int r0 = blockIdx.x * 256, c0 = blockIdx.y * ZG_COLS;
  if (r0 >= d.m || c0 >= d.ni) return;
  const int t = threadIdx.x, r = r0 + t;
  if (t < ZG_COLS) {
    int to = (c0 + t < d.ni) ? d.rperm[c0 + t] : 0;
    s_to[t] = min(max(to, 0), d.ni - 1);  // (a permutation entry is always in range; the clamp keeps a corrupt list inside the block)
  }
  __syncthreads();
  if (r >= d.m) return;
  const int nc = min(ZG_COLS, d.ni - c0);
  const T* src = d.X2 + (size_t)r + (size_t)c0 * d.ldz;
#pragma unroll 4
  for (int c = 0; c < nc; ++c) gst(d.Z + (size_t)r + (size_t)s_to[c] * d.ldz, gld(src + (size_t)c * d.ldz));
}
template <class T>
void launch_zpermute_cols(const SelDesc<T>* d, int nbatch, int maxm, int maxni, hipStream_t s) {
  if (nbatch <= 0 || maxm <= 0 || maxni <= 0) return;
  hipLaunchKernelGGL(zpermute_cols_kernel<T>, dim3((maxm + 255) / 256, (maxni + ZG_COLS - 1) / ZG_COLS, nbatch), dim3(256), 0, s, d);
}

// grid.x covers max(ni, entries) of the front: thread k writes the k-th diagonal entry and the k-th owned entry of A's pattern
template <class T>
__global__ __launch_bounds__(256) void zextract_kernel(const SelDesc<T>* __restrict__ descs, int trans, T* __restrict__ diag, T* __restrict__ zval) {
  const SelDesc<T> d = descs[blockIdx.y];
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (diag && k < d.ni) gst(diag + d.fidx[k], gld(d.Z + (size_t)k * d.ldz + k));
  if (zval && k < d.ecnt) {
    int pr = d.epr[k], pc = d.epc[k];
    if (trans) { const int x = pr; pr = pc; pc = x; }
    gst(zval + d.ee[k], gld(d.Z + (size_t)pr + (size_t)pc * d.ldz));
  }
}
template <class T>
void launch_zextract(const SelDesc<T>* d, int nbatch, int maxni, int maxe, int trans, T* diag, T* zval, hipStream_t s) {
  const int cnt = std::max(diag ? maxni : 0, zval ? maxe : 0);
  if (nbatch <= 0 || cnt <= 0) return;
  hipLaunchKernelGGL(zextract_kernel<T>, dim3((cnt + 255) / 256, nbatch), dim3(256), 0, s, d, trans, diag, zval);
}

#define HS_SEL_INST(T)                                                                          \
  template void launch_zinit<T>(const SelDesc<T>*, int, int, hipStream_t);                      \
  template void launch_zload_lr<T>(const SelDesc<T>*, int, int, int, hipStream_t);              \
  template void launch_zgather<T>(const SelDesc<T>*, int, int, hipStream_t);                    \
  template void launch_zpermute_cols<T>(const SelDesc<T>*, int, int, int, hipStream_t);         \
  template void launch_zextract<T>(const SelDesc<T>*, int, int, int, int, T*, T*, hipStream_t);
HS_SEL_INST(double)
HS_SEL_INST(cplx)
