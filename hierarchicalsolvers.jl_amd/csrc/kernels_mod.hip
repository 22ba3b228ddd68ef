// kernels_mod.hip -- the device pieces of hs_mod_* (hs_mod.hip): solves with A1 = A + U V^H from the stored factors of A.
//
//   mod_inner     T = op(P)^H Y      tall-skinny inner product over n, row slabs + an ordered second pass
//   mod_apply     Y -= op(Z) T       rank-k correction of a block
//   mod_gather    T = Y[J, :]        the inner product with V = I[:, J]
//   mod_cap_lu / mod_cap_solve       LU and solves with the k x k capacitance matrix (off the hot path: one workgroup / one per column)
//
// Lane maps of v_mfma_f64_16x16x4_f64 (as kernels_solve_multi_t.hip): A operand lane (row = lane & 15, k = lane >> 4), B operand lane
// (k = lane >> 4, col = lane & 15), C/D col = lane & 15, row = (lane >> 4) + 4 reg.  hsk_mod_inner_* / hsk_mod_apply_* check them with exact
// integer data (tests/test_mod_gpu.py).
//
// mod_inner: both operands have the reduction index (rows) contiguous, so a lane owns PAIRS of consecutive rows of its column (one 16-byte
// load), the first of the pair feeding one MFMA and the second the next; the sum does not care which row a (group, MFMA) pair holds as long as
// both operands agree.  A wave owns 16 columns of P and every column tile of Y; the four waves of a workgroup take 64 columns of P and share Y
// through L1.  mod_apply computes the TRANSPOSED tile (Y^T -= T^T op(Z)^T): the rows of Y and Z then sit on lane & 15 in the B operand and in
// C/D, so the loads of Z and the loads and stores of Y are 128 contiguous bytes per lane group, and -T is the A operand, read from LDS.
#include "hs_mod.h"

typedef double v4d __attribute__((ext_vector_type(4)));
#define MFMA64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

// ---- mod_inner ------------------------------------------------------------------------------------------------------------------------
// rows [rb, rb + 8) (Float64) of one column: the pair (rb + 2 g, rb + 2 g + 1), zeros past r1
__device__ __forceinline__ hs_d2u mod_pair(const double* col, long long rb, int g, long long r1, bool full) {
  const long long r = rb + 2 * g;
  if (full) return gld2(col + r);
  hs_d2u v;
  v.x = r < r1 ? gld(col + r) : 0.0;
  v.y = r + 1 < r1 ? gld(col + r + 1) : 0.0;
  return v;
}
// row rb + g (ComplexF64) of one column as (re, im), zeros past r1
__device__ __forceinline__ hs_d2u mod_elem(const cplx* col, long long rb, int g, long long r1) {
  const long long r = rb + g;
  hs_d2u v = gld2(col + (r < r1 ? r : r1 - 1));
  if (r >= r1) { v.x = 0.0; v.y = 0.0; }
  return v;
}

template <class T, int NT>
__global__ __launch_bounds__(256) void mod_inner_kernel(const T* P, long long ldp, const T* Y, long long ldy, long long n, int k, int m, int conj, T* part) {
  constexpr bool CX = sizeof(T) == 16;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int i0 = (blockIdx.y * 4 + wv) * 16;
  if (i0 >= k) return;  // (no barrier in this kernel)
  const long long r0 = (long long)blockIdx.x * HS_MOD_SLAB, r1 = min(n, r0 + (long long)HS_MOD_SLAB);
  const T* pp = P + (size_t)min(i0 + l15, k - 1) * ldp;
  const T* yp[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) yp[ct] = Y + (size_t)min(ct * 16 + l15, m - 1) * ldy;
  v4d acc[NT], aci[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    acc[ct] = v4d{0.0, 0.0, 0.0, 0.0};
    aci[ct] = v4d{0.0, 0.0, 0.0, 0.0};
  }
  if constexpr (CX) {
    const int nsteps = (int)((r1 - r0 + 3) / 4);
    for (int st = 0; st < nsteps; ++st) {
      const long long rb = r0 + 4 * st;
      hs_d2u a = mod_elem(pp, rb, l4, r1);
      if (!conj) a.y = -a.y;  // op = identity: conj(P)^T Y
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        const hs_d2u y = mod_elem(yp[ct], rb, l4, r1);
        acc[ct] = MFMA64(a.x, y.x, acc[ct]);
        acc[ct] = MFMA64(-a.y, y.y, acc[ct]);
        aci[ct] = MFMA64(a.x, y.y, aci[ct]);
        aci[ct] = MFMA64(a.y, y.x, aci[ct]);
      }
    }
  } else {
    const int nsteps = (int)((r1 - r0 + 7) / 8);
    for (int st = 0; st < nsteps; ++st) {
      const long long rb = r0 + 8 * st;
      const bool full = rb + 8 <= r1;
      const hs_d2u a = mod_pair(pp, rb, l4, r1, full);
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        const hs_d2u y = mod_pair(yp[ct], rb, l4, r1, full);
        acc[ct] = MFMA64(a.x, y.x, acc[ct]);
        acc[ct] = MFMA64(a.y, y.y, acc[ct]);
      }
    }
  }
  T* ps = part + (size_t)blockIdx.x * k * m;  // part[slab]: k x m column-major, ld k
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    const int c = ct * 16 + l15;
    if (c >= m) continue;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int i = i0 + l4 + 4 * g;
      if (i >= k) continue;
      if constexpr (CX)
        gst(ps + (size_t)c * k + i, cplx{acc[ct][g], aci[ct][g]});
      else
        gst(ps + (size_t)c * k + i, acc[ct][g]);
    }
  }
}

// T[i, c] = part[0][i, c] + part[1][i, c] + ... in slab order
template <class T>
__global__ __launch_bounds__(256) void mod_inner_sum_kernel(const T* part, long long nslab, int k, int m, T* Tout, long long ldt) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)k * m) return;
  T acc = gld(part + e);
  for (long long s = 1; s < nslab; ++s) acc = acc + gld(part + s * k * m + e);
  gst(Tout + (e / k) * ldt + (e % k), acc);
}

template <class T>
void launch_mod_inner(const T* P, int64_t ldp, const T* Y, int64_t ldy, int64_t n, int k, int m, int conj, T* part, T* Tout, int64_t ldt, hipStream_t s) {
  if (k <= 0 || m <= 0 || n <= 0) return;
  const dim3 grid((unsigned)hs_mod_slabs(n), (unsigned)((k + 63) / 64));
  const int cj = (conj && sizeof(T) == 16) ? 1 : 0;
  switch ((m + 15) / 16) {
    case 1: hipLaunchKernelGGL((mod_inner_kernel<T, 1>), grid, dim3(256), 0, s, P, (long long)ldp, Y, (long long)ldy, (long long)n, k, m, cj, part); break;
    case 2: hipLaunchKernelGGL((mod_inner_kernel<T, 2>), grid, dim3(256), 0, s, P, (long long)ldp, Y, (long long)ldy, (long long)n, k, m, cj, part); break;
    case 3: hipLaunchKernelGGL((mod_inner_kernel<T, 3>), grid, dim3(256), 0, s, P, (long long)ldp, Y, (long long)ldy, (long long)n, k, m, cj, part); break;
    default: hipLaunchKernelGGL((mod_inner_kernel<T, 4>), grid, dim3(256), 0, s, P, (long long)ldp, Y, (long long)ldy, (long long)n, k, m, cj, part); break;
  }
  hipLaunchKernelGGL(mod_inner_sum_kernel<T>, dim3((unsigned)(((long long)k * m + 255) / 256)), dim3(256), 0, s, (const T*)part, (long long)hs_mod_slabs(n), k, m, Tout,
                     (long long)ldt);
}
template void launch_mod_inner<double>(const double*, int64_t, const double*, int64_t, int64_t, int, int, int, double*, double*, int64_t, hipStream_t);
template void launch_mod_inner<cplx>(const cplx*, int64_t, const cplx*, int64_t, int64_t, int, int, int, cplx*, cplx*, int64_t, hipStream_t);

// ---- mod_apply ------------------------------------------------------------------------------------------------------------------------
#define MOD_APPLY_ROWS 512  // rows of Y per workgroup: 8 tiles of 16 rows per wave
template <class T>
__global__ __launch_bounds__(256) void mod_apply_kernel(T* Y, long long ldy, const T* Z, long long ldz, const T* Tm, long long ldt, long long n, int k, int m, int conj) {
  constexpr bool CX = sizeof(T) == 16;
  __shared__ double tl[(CX ? 2 : 1) * HS_MOD_MAXRANK * 16];  // -T[j, c0 + c] at [j * 16 + c]; ComplexF64: the imaginary parts behind the real ones
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int c0 = blockIdx.y * 16;
  const int kp = (k + 3) & ~3;
  for (int e = threadIdx.x; e < kp * 16; e += 256) {
    const int j = e >> 4, c = c0 + (e & 15);
    const bool in = j < k && c < m;
    if constexpr (CX) {
      const cplx v = in ? gld(Tm + (size_t)c * ldt + j) : cplx{0.0, 0.0};
      tl[e] = -v.re;
      tl[HS_MOD_MAXRANK * 16 + e] = -v.im;
    } else {
      tl[e] = in ? -gld(Tm + (size_t)c * ldt + j) : 0.0;
    }
  }
  __syncthreads();
  const long long rbase = (long long)blockIdx.x * MOD_APPLY_ROWS;
  for (int tile = wv; tile < MOD_APPLY_ROWS / 16; tile += 4) {
    const long long rt = rbase + tile * 16;
    if (rt >= n) break;
    const long long r = rt + l15, rc = min(r, n - 1);
    v4d acc = v4d{0.0, 0.0, 0.0, 0.0}, aci = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c = c0 + l4 + 4 * g;
      if (r < n && c < m) {
        if constexpr (CX) {
          const cplx v = gld(Y + (size_t)c * ldy + r);
          acc[g] = v.re;
          aci[g] = v.im;
        } else {
          acc[g] = gld(Y + (size_t)c * ldy + r);
        }
      }
    }
    for (int j0 = 0; j0 < kp; j0 += 4) {
      const int j = j0 + l4;
      const T* zp = Z + (size_t)min(j, k - 1) * ldz + rc;
      if constexpr (CX) {
        hs_d2u z = gld2(zp);
        if (j >= k) { z.x = 0.0; z.y = 0.0; }
        if (conj) z.y = -z.y;
        const double ntr = tl[j * 16 + l15], nti = tl[HS_MOD_MAXRANK * 16 + j * 16 + l15];
        acc = MFMA64(ntr, z.x, acc);
        acc = MFMA64(-nti, z.y, acc);
        aci = MFMA64(nti, z.x, aci);
        aci = MFMA64(ntr, z.y, aci);
      } else {
        double z = gld(zp);
        if (j >= k) z = 0.0;
        acc = MFMA64(tl[j * 16 + l15], z, acc);
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c = c0 + l4 + 4 * g;
      if (r < n && c < m) {
        if constexpr (CX)
          gst(Y + (size_t)c * ldy + r, cplx{acc[g], aci[g]});
        else
          gst(Y + (size_t)c * ldy + r, acc[g]);
      }
    }
  }
}
template <class T>
void launch_mod_apply(T* Y, int64_t ldy, const T* Z, int64_t ldz, const T* Tm, int64_t ldt, int64_t n, int k, int m, int conj, hipStream_t s) {
  if (k <= 0 || m <= 0 || n <= 0) return;
  const dim3 grid((unsigned)((n + MOD_APPLY_ROWS - 1) / MOD_APPLY_ROWS), (unsigned)((m + 15) / 16));  // rows on x (no 65535 limit), at most 4 column tiles on y
  hipLaunchKernelGGL(mod_apply_kernel<T>, grid, dim3(256), 0, s, Y, (long long)ldy, Z, (long long)ldz, Tm, (long long)ldt, (long long)n, k, m,
                     (conj && sizeof(T) == 16) ? 1 : 0);
}
template void launch_mod_apply<double>(double*, int64_t, const double*, int64_t, const double*, int64_t, int64_t, int, int, int, hipStream_t);
template void launch_mod_apply<cplx>(cplx*, int64_t, const cplx*, int64_t, const cplx*, int64_t, int64_t, int, int, int, hipStream_t);

// ---- mod_gather, mod_add_eye, mod_scatter -------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void mod_gather_kernel(T* Tout, long long ldt, const T* Y, long long ldy, const int64_t* J, int k, int m) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)k * m) return;
  const int j = (int)(e % k);
  const long long c = e / k;
  gst(Tout + c * ldt + j, gld(Y + c * ldy + gld(J + j)));
}
template <class T>
void launch_mod_gather(T* Tout, int64_t ldt, const T* Y, int64_t ldy, const int64_t* J, int k, int m, hipStream_t s) {
  if (k <= 0 || m <= 0) return;
  hipLaunchKernelGGL(mod_gather_kernel<T>, dim3((unsigned)(((long long)k * m + 255) / 256)), dim3(256), 0, s, Tout, (long long)ldt, Y, (long long)ldy, J, k, m);
}
template void launch_mod_gather<double>(double*, int64_t, const double*, int64_t, const int64_t*, int, int, hipStream_t);
template void launch_mod_gather<cplx>(cplx*, int64_t, const cplx*, int64_t, const int64_t*, int, int, hipStream_t);

template <class T>
__global__ __launch_bounds__(256) void mod_add_eye_kernel(T* C, int ldc, int k) {
  const int j = threadIdx.x;
  if (j < k) gst(C + (size_t)j * ldc + j, gld(C + (size_t)j * ldc + j) + Scal<T>::one());
}
template <class T>
void launch_mod_add_eye(T* C, int ldc, int k, hipStream_t s) {
  if (k <= 0) return;
  hipLaunchKernelGGL(mod_add_eye_kernel<T>, dim3(1), dim3(256), 0, s, C, ldc, k);
}
template void launch_mod_add_eye<double>(double*, int, int, hipStream_t);
template void launch_mod_add_eye<cplx>(cplx*, int, int, hipStream_t);

template <class T>
__global__ __launch_bounds__(256) void mod_scatter_kernel(T* out, long long ld, const int32_t* row, const int32_t* col, const T* val, long long cnt) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= cnt) return;
  gst(out + (long long)gld(col + e) * ld + gld(row + e), gld(val + e));
}
template <class T>
void launch_mod_scatter(T* out, int64_t ld, const int32_t* row, const int32_t* col, const T* val, int64_t cnt, hipStream_t s) {
  if (cnt <= 0) return;
  hipLaunchKernelGGL(mod_scatter_kernel<T>, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, out, (long long)ld, row, col, val, (long long)cnt);
}
template void launch_mod_scatter<double>(double*, int64_t, const int32_t*, const int32_t*, const double*, int64_t, hipStream_t);
template void launch_mod_scatter<cplx>(cplx*, int64_t, const int32_t*, const int32_t*, const cplx*, int64_t, hipStream_t);

// ---- mod_cap_lu -----------------------------------------------------------------------------------------------------------------------
// Right-looking, unblocked, one workgroup of 256 threads on C in global memory (k <= 256: thread t owns row j + t of the pivot search and
// row j + 1 + t of the update, column t of the row exchange).
template <class T>
__global__ __launch_bounds__(256) void mod_cap_lu_kernel(T* C, int ldc, int k, int* piv, int* info) {
  __shared__ double smax[256];
  __shared__ int sidx[256];
  const int t = threadIdx.x;
  if (t == 0) *info = 0;
  for (int j = 0; j < k; ++j) {
    const int i = j + t;
    smax[t] = i < k ? Scal<T>::abs1(gld(C + (size_t)j * ldc + i)) : -1.0;
    sidx[t] = i;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (t < s && smax[t + s] > smax[t]) {
        smax[t] = smax[t + s];
        sidx[t] = sidx[t + s];
      }
      __syncthreads();
    }
    const int p = sidx[0];
    const double pm = smax[0];
    __syncthreads();
    if (!(pm > 0.0)) {  // an exactly zero (or NaN) pivot column: the same branch in every thread
      if (t == 0) *info = j + 1;
      return;
    }
    if (t == 0) piv[j] = p;
    if (p != j && t < k) {
      T* cj = C + (size_t)t * ldc;
      const T a = gld(cj + j), b = gld(cj + p);
      gst(cj + j, b);
      gst(cj + p, a);
    }
    __syncthreads();
    const T d = gld(C + (size_t)j * ldc + j);
    if (i > j && i < k) gst(C + (size_t)j * ldc + i, gld(C + (size_t)j * ldc + i) / d);
    __syncthreads();
    const int iu = j + 1 + t;
    if (iu < k) {
      const T l = gld(C + (size_t)j * ldc + iu);
      for (int jj = j + 1; jj < k; ++jj) {
        T* cc = C + (size_t)jj * ldc;
        gst(cc + iu, Scal<T>::fnma(l, gld(cc + j), gld(cc + iu)));
      }
    }
    __syncthreads();
  }
}
template <class T>
void launch_mod_cap_lu(T* C, int ldc, int k, int* piv, int* info, hipStream_t s) {
  hipLaunchKernelGGL(mod_cap_lu_kernel<T>, dim3(1), dim3(256), 0, s, C, ldc, k, piv, info);
}
template void launch_mod_cap_lu<double>(double*, int, int, int*, int*, hipStream_t);
template void launch_mod_cap_lu<cplx>(cplx*, int, int, int*, int*, hipStream_t);

// ---- mod_cap_solve --------------------------------------------------------------------------------------------------------------------
// One workgroup per column, thread t owns row t of it (in LDS).  P C = L U, so
//   op 0:     x = U^-1 L^-1 P b
//   op 1, 2:  o(C)^T = o(U)^T o(L)^T P  (o = identity / conj):  x = P^T o(L)^-T o(U)^-T b
// Every triangular sweep is column-oriented: step j finishes x_j, then every other thread takes its own update.
__device__ __forceinline__ double mod_cj(double a, bool) { return a; }
__device__ __forceinline__ cplx mod_cj(cplx a, bool cj) { return cj ? cplx{a.re, -a.im} : a; }

template <class T>
__global__ __launch_bounds__(256) void mod_cap_solve_kernel(const T* LU, int ldc, int k, const int* piv, int op, T* Tm, long long ldt) {
  __shared__ T xs[256];
  const int t = threadIdx.x;
  T* col = Tm + (size_t)blockIdx.x * ldt;
  const bool cj = op == 2;
  if (t < k) xs[t] = gld(col + t);
  __syncthreads();
  T mine = Scal<T>::zero();
  if (op == 0) {
    if (t == 0)
      for (int j = 0; j < k; ++j) {
        const int p = gld(piv + j);
        const T a = xs[j];
        xs[j] = xs[p];
        xs[p] = a;
      }
    for (int j = 0; j < k; ++j) {  // L y = P b (unit diagonal)
      __syncthreads();
      const T xj = xs[j];
      if (t > j && t < k) xs[t] = xs[t] - gld(LU + (size_t)j * ldc + t) * xj;
    }
    for (int j = k - 1; j >= 0; --j) {  // U x = y
      __syncthreads();
      const T xj = xs[j] / gld(LU + (size_t)j * ldc + j);
      if (t == j) mine = xj;
      if (t < j) xs[t] = xs[t] - gld(LU + (size_t)j * ldc + t) * xj;
    }
    if (t < k) gst(col + t, mine);
    return;
  }
  for (int j = 0; j < k; ++j) {  // o(U)^T y = b
    __syncthreads();
    const T yj = xs[j] / mod_cj(gld(LU + (size_t)j * ldc + j), cj);
    if (t == j) mine = yj;
    if (t > j && t < k) xs[t] = xs[t] - mod_cj(gld(LU + (size_t)t * ldc + j), cj) * yj;
  }
  __syncthreads();
  if (t < k) xs[t] = mine;
  for (int j = k - 1; j >= 0; --j) {  // o(L)^T z = y (unit diagonal)
    __syncthreads();
    const T zj = xs[j];
    if (t < j) xs[t] = xs[t] - mod_cj(gld(LU + (size_t)t * ldc + j), cj) * zj;
  }
  __syncthreads();
  if (t == 0)
    for (int j = k - 1; j >= 0; --j) {
      const int p = gld(piv + j);
      const T a = xs[j];
      xs[j] = xs[p];
      xs[p] = a;
    }
  __syncthreads();
  if (t < k) gst(col + t, xs[t]);
}
template <class T>
void launch_mod_cap_solve(const T* LU, int ldc, int k, const int* piv, int op, T* Tm, int64_t ldt, int m, hipStream_t s) {
  if (k <= 0 || m <= 0) return;
  hipLaunchKernelGGL(mod_cap_solve_kernel<T>, dim3((unsigned)m), dim3(256), 0, s, LU, ldc, k, piv, (op == 2 && sizeof(T) == 8) ? 1 : op, Tm, (long long)ldt);
}
template void launch_mod_cap_solve<double>(const double*, int, int, const int*, int, double*, int64_t, int, hipStream_t);
template void launch_mod_cap_solve<cplx>(const cplx*, int, int, const int*, int, cplx*, int64_t, int, hipStream_t);
