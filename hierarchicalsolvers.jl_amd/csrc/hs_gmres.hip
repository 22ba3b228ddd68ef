// hs_gmres.hip -- right-preconditioned restarted GMRES with every vector on the device, behind the C ABI (include/hs_solver.h).
//
// Reference scenario (test/rungmres.jl:47-48):  x, ch = gmres(A, b; Pr=F, reltol=1e-9, restart=30, log=true, maxiter=30)
// IterativeSolvers.jl (0.9.0) is not part of the reference tree: the algorithm is the textbook one (Saad & Schultz 1986; Arnoldi with
// classical Gram-Schmidt + one re-orthogonalisation pass, Givens rotations on the Hessenberg matrix, right preconditioning
// x = x0 + Pr^-1 V y) and matches the Python mirror hierarchicalsolvers.jl_amd/gmres.py step for step (same iteration counts).
// PARITY UNPINNED against the Julia package.
//
// Kernels (all HBM-bound, n-vectors): CSR SpMV (one thread per row; a stencil row has <= 27 entries), the (k+1) simultaneous dot
// products V^H w of an Arnoldi step (per-workgroup partial sums, then one small reduction), the update w -= V h, norm and scale;
// the Hessenberg / Givens recurrences and the final triangular solve run in one single-thread kernel each on device-resident H, c, s,
// g -- the host reads ONE double (the residual estimate) per iteration to decide whether to go on: a preconditioner application costs
// three orders of magnitude more than that read, and an iteration that is not needed costs a whole `ldiv!`.
//
// hs_gmres_t_* runs the same iteration on op(A) x = b, op(A) = A, transpose(A) or adjoint(A), right-preconditioned by op(Pr): gmres_device is a
// template on the operator (the CSR SpMV above, or the SpMV over "entry ranges as rows" of hs_gmres_common.h, which reads the CSC columns of A
// as the rows of op(A)) and on the preconditioner call (hs_ldiv_dev_* / hs_ldiv_dev_t_*).  A is passed as host CSC arrays or is the handle's
// own (hs_gmres_op.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "hs_gmres_common.h"

namespace {

// y = A x (CSR, 0-based), or y = b - A x with b, is spmv_op_kernel<T, false> (hs_gmres_common.h): a CSR is the plain case of its "entry
// ranges as rows".

// part[blockIdx.x * (k+1) + j] = sum over the block's rows of conj(V[j][i]) * w[i],  j = 0..k
template <class T>
__global__ __launch_bounds__(256) void multi_dot_kernel(const T* __restrict__ V, int64_t ldv, int k1, const T* __restrict__ w, T* __restrict__ part, int64_t n) {
  __shared__ T sh[256];
  const int64_t i0 = (int64_t)blockIdx.x * 1024;
  T wv[4];
  for (int t = 0; t < 4; ++t) {
    const int64_t i = i0 + t * 256 + threadIdx.x;
    wv[t] = i < n ? w[i] : Scal<T>::zero();
  }
  for (int j = 0; j < k1; ++j) {
    T acc = Scal<T>::zero();
    for (int t = 0; t < 4; ++t) {
      const int64_t i = i0 + t * 256 + threadIdx.x;
      if (i < n) acc = Scal<T>::fma(conj_(V[(size_t)j * ldv + i]), wv[t], acc);
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if ((int)threadIdx.x < st) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + st];
      __syncthreads();
    }
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * k1 + j] = sh[0];
    __syncthreads();
  }
}
// h[j] (+)= sum over blocks of part[b * k1 + j]   (one workgroup; deterministic order)
template <class T>
__global__ __launch_bounds__(256) void reduce_parts_kernel(const T* __restrict__ part, int nblk, int k1, T* __restrict__ h, T* __restrict__ hacc) {
  __shared__ T sh[256];
  for (int j = 0; j < k1; ++j) {
    T acc = Scal<T>::zero();
    for (int b = threadIdx.x; b < nblk; b += 256) acc = acc + part[(size_t)b * k1 + j];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if ((int)threadIdx.x < st) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + st];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      h[j] = sh[0];
      if (hacc) hacc[j] = hacc[j] + sh[0];
    }
    __syncthreads();
  }
}
// w[i] -= sum_j h[j] * V[j][i]
template <class T>
__global__ __launch_bounds__(256) void multi_axpy_kernel(const T* __restrict__ V, int64_t ldv, int k1, const T* __restrict__ h, T* __restrict__ w, int64_t n) {
  __shared__ T sh[GM_MAXK + 1];
  if ((int)threadIdx.x < k1) sh[threadIdx.x] = h[threadIdx.x];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  T acc = w[i];
  for (int j = 0; j < k1; ++j) acc = Scal<T>::fnma(sh[j], V[(size_t)j * ldv + i], acc);
  w[i] = acc;
}
// out[i] = x[i] + sum_j y[j] * V[j][i]  (x may be null: out = V^T y)
template <class T>
__global__ __launch_bounds__(256) void combine_kernel(const T* __restrict__ V, int64_t ldv, int k, const T* __restrict__ y, const T* __restrict__ x, T* __restrict__ out,
                                                      int64_t n) {
  __shared__ T sh[GM_MAXK + 1];
  if ((int)threadIdx.x < k) sh[threadIdx.x] = y[threadIdx.x];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  T acc = x ? x[i] : Scal<T>::zero();
  for (int j = 0; j < k; ++j) acc = Scal<T>::fma(sh[j], V[(size_t)j * ldv + i], acc);
  out[i] = acc;
}
template <class T>
__global__ __launch_bounds__(256) void norm2_part_kernel(const T* __restrict__ w, double* __restrict__ part, int64_t n) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (int t = 0; t < 4; ++t) {
    const int64_t i = (int64_t)blockIdx.x * 1024 + t * 256 + threadIdx.x;
    if (i < n) acc += abs2_(w[i]);
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}
__global__ __launch_bounds__(256) void norm2_final_kernel(const double* __restrict__ part, int nblk, double* __restrict__ out) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) acc += part[b];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = sqrt(sh[0]);
}
// v[i] = w[i] / *nrm  (nothing when the norm is zero: breakdown is handled by the caller through the residual estimate)
template <class T>
__global__ __launch_bounds__(256) void scale_into_kernel(const T* __restrict__ w, const double* __restrict__ nrm, T* __restrict__ v, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double a = *nrm;
  v[i] = a > 0.0 ? scale_(w[i], 1.0 / a) : w[i];
}

// Device-resident small state of one restart cycle: H ((m+1) x m, column-major, ld m+1), c, s, g, the new column h (+ its norm)
template <class T>
struct GmSmall {
  T* H;
  T* cs;  // real cosines stored as T
  T* sn;
  T* g;
  T* h;         // column k of the Hessenberg matrix before the rotations: h[0..k] = (h1 + h2), h[k+1] = ||w||
  double* hn;   // ||w||
  double* res;  // |g[k+1]| after the rotation
  T* y;
  int ld;
};

// applies the previous rotations to column k, creates the rotation that annihilates H[k+1, k], updates g (gmres.py lines "apply the
// previous rotations ...")
template <class T>
__global__ void givens_kernel(GmSmall<T> S, int k) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  T* Hc = S.H + (size_t)k * S.ld;
  for (int i = 0; i <= k; ++i) Hc[i] = S.h[i];
  T hk1 = Scal<T>::zero();
  *((double*)&hk1) = *S.hn;  // real part = ||w||
  Hc[k + 1] = hk1;
  for (int i = 0; i < k; ++i) {
    const T t = S.cs[i] * Hc[i] + S.sn[i] * Hc[i + 1];
    Hc[i + 1] = Scal<T>::zero() - conj_(S.sn[i]) * Hc[i] + S.cs[i] * Hc[i + 1];
    Hc[i] = t;
  }
  const T a = Hc[k], b = Hc[k + 1];
  const double aa = absT(a), den = sqrt(aa * aa + absT(b) * absT(b));
  T c = Scal<T>::one(), s = Scal<T>::zero();
  if (den != 0.0) {
    c = Scal<T>::zero();
    *((double*)&c) = aa / den;
    const T ph = aa > 0.0 ? scale_(a, 1.0 / aa) : Scal<T>::one();
    s = scale_(ph * conj_(b), 1.0 / den);
  }
  S.cs[k] = c;
  S.sn[k] = s;
  Hc[k] = c * a + s * b;
  Hc[k + 1] = Scal<T>::zero();
  S.g[k + 1] = Scal<T>::zero() - conj_(s) * S.g[k];
  S.g[k] = c * S.g[k];
  *S.res = absT(S.g[k + 1]);
}
// y = triu(H[:k, :k]) \ g[:k]
template <class T>
__global__ void hess_solve_kernel(GmSmall<T> S, int k) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int i = k - 1; i >= 0; --i) {
    T acc = S.g[i];
    for (int j = i + 1; j < k; ++j) acc = Scal<T>::fnma(S.H[(size_t)i + (size_t)j * S.ld], S.y[j], acc);
    S.y[i] = acc / S.H[(size_t)i + (size_t)i * S.ld];
  }
}
template <class T>
__global__ void gm_reset_kernel(GmSmall<T> S, int m, const double* beta) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int i = 0; i <= m; ++i) S.g[i] = Scal<T>::zero();
  T b = Scal<T>::zero();
  *((double*)&b) = *beta;
  S.g[0] = b;
}

template <class T>
int prec_apply(hs_handle* F, T* out, const T* in, int64_t n, hipStream_t s);
template <>
int prec_apply<double>(hs_handle* F, double* out, const double* in, int64_t n, hipStream_t s) {
  return hs_ldiv_dev_d(F, out, n, in, n, n, 1, (void*)s);
}
template <>
int prec_apply<cplx>(hs_handle* F, cplx* out, const cplx* in, int64_t n, hipStream_t s) {
  return hs_ldiv_dev_z(F, (double*)out, n, (const double*)in, n, n, 1, (void*)s);
}

template <class T>
int prec_apply_t(hs_handle* F, int trans, T* out, const T* in, int64_t n, hipStream_t s);
template <>
int prec_apply_t<double>(hs_handle* F, int trans, double* out, const double* in, int64_t n, hipStream_t s) {
  return hs_ldiv_dev_t_d(F, trans, out, n, in, n, n, 1, (void*)s);
}
template <>
int prec_apply_t<cplx>(hs_handle* F, int trans, cplx* out, const cplx* in, int64_t n, hipStream_t s) {
  return hs_ldiv_dev_t_z(F, trans, (double*)out, n, (const double*)in, n, n, 1, (void*)s);
}

template <class T>
int prec_apply_probe(hs_handle* F, int trans, int64_t n) {
  return sizeof(T) == 16 ? hs_ldiv_dev_t_z(F, trans, nullptr, n, nullptr, n, n, 0, nullptr) : hs_ldiv_dev_t_d(F, trans, nullptr, n, nullptr, n, n, 0, nullptr);
}

// What gmres_device is instantiated on.  The operator: y = A x, or y = b - A x with b.  The preconditioner: out = Pr^-1 in; F == nullptr: none.
template <class T>
struct CsrSpmv {  // hs_gmres_*: the CSR upload of A
  const int64_t* rowptr;
  const int32_t* colind;
  const T* val;
  void operator()(const T* x, T* y, const T* b, int64_t n, hipStream_t s) const {
    hipLaunchKernelGGL((spmv_op_kernel<T, false>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rowptr, colind, val, x, y, b, n);
  }
};
template <class T>
struct RowsSpmv {  // hs_gmres_t_*: op(A) over entry ranges
  RowsOf<T> A;
  void operator()(const T* x, T* y, const T* b, int64_t n, hipStream_t s) const { launch_spmv_op<T>(A, x, y, b, n, s); }
};
template <class T>
struct PrecFwd {  // hs_ldiv_dev_*
  hs_handle* F;
  int operator()(T* out, const T* in, int64_t n, hipStream_t s) const { return prec_apply<T>(F, out, in, n, s); }
};
template <class T>
struct PrecOp {  // hs_ldiv_dev_t_*: op(F)
  hs_handle* F;
  int trans;
  int operator()(T* out, const T* in, int64_t n, hipStream_t s) const { return prec_apply_t<T>(F, trans, out, in, n, s); }
};

template <class T, class Op, class Prec>
void gmres_device(const Op& A, const Prec& Pr, int64_t n, const T* b, T* x, int use_x0, double reltol, double abstol, int restart, int64_t maxiter, double* hist,
                  int64_t* iters_out, int* conv_out, hipStream_t s) {
  hs_handle* const F = Pr.F;
  DevBuf buf;
  const int m = restart;
  const int64_t ldv = (n + 1) / 2 * 2;
  T* V = buf.get<T>((size_t)(m + 1) * ldv);
  T* w = buf.get<T>((size_t)ldv);
  T* z = buf.get<T>((size_t)ldv);
  T* r = buf.get<T>((size_t)ldv);
  const int nblk = (int)((n + 1023) / 1024);
  T* part = buf.get<T>((size_t)nblk * (m + 2));
  double* dpart = buf.get<double>((size_t)nblk);
  double* dscal = buf.get<double>(8);  // [0] beta, [1] hn, [2] res
  GmSmall<T> S;
  S.ld = m + 1;
  S.H = buf.get<T>((size_t)(m + 1) * m);
  S.cs = buf.get<T>(m + 1);
  S.sn = buf.get<T>(m + 1);
  S.g = buf.get<T>(m + 2);
  S.h = buf.get<T>(m + 2);
  S.y = buf.get<T>(m + 1);
  S.hn = dscal + 1;
  S.res = dscal + 2;
  T* h2 = buf.get<T>(m + 2);
  const unsigned gn = (unsigned)((n + 255) / 256);
  auto norm = [&](const T* v, double* dout) {
    hipLaunchKernelGGL(norm2_part_kernel<T>, dim3(nblk), dim3(256), 0, s, v, dpart, n);
    hipLaunchKernelGGL(norm2_final_kernel, dim3(1), dim3(256), 0, s, (const double*)dpart, nblk, dout);
  };
  auto read = [&](const double* d) {
    double v = 0.0;
    GM_HIP(hipMemcpyAsync(&v, d, sizeof(double), hipMemcpyDeviceToHost, s));
    GM_HIP(hipStreamSynchronize(s));
    return v;
  };
  if (!use_x0) GM_HIP(hipMemsetAsync(x, 0, sizeof(T) * (size_t)n, s));
  // r = b - A x
  if (use_x0)
    A((const T*)x, r, b, n, s);
  else
    GM_HIP(hipMemcpyAsync(r, b, sizeof(T) * (size_t)n, hipMemcpyDeviceToDevice, s));
  norm(r, dscal);
  double beta = read(dscal);
  const double tol = std::max(reltol * beta, abstol);
  int64_t it = 0;
  size_t nh = 0;
  hist[nh++] = beta;
  bool converged = beta <= tol;
  while (!converged && it < maxiter) {
    hipLaunchKernelGGL(scale_into_kernel<T>, dim3(gn), dim3(256), 0, s, (const T*)r, (const double*)dscal, V, n);
    hipLaunchKernelGGL(gm_reset_kernel<T>, dim3(1), dim3(1), 0, s, S, m, (const double*)dscal);
    int k_used = 0;
    for (int k = 0; k < m && it < maxiter; ++k) {
      const T* vk = V + (size_t)k * ldv;
      const T* zz = vk;
      if (F) {
        const int st = Pr(z, vk, n, s);
        if (st != 0) throw st;
        zz = z;
      }
      A(zz, w, (const T*)nullptr, n, s);
      // classical Gram-Schmidt with one re-orthogonalisation pass: h = V^H w; w -= V h; h2 = V^H w; w -= V h2; H[:, k] = h + h2
      const int k1 = k + 1;
      hipLaunchKernelGGL(multi_dot_kernel<T>, dim3(nblk), dim3(256), 0, s, (const T*)V, ldv, k1, (const T*)w, part, n);
      hipLaunchKernelGGL(reduce_parts_kernel<T>, dim3(1), dim3(256), 0, s, (const T*)part, nblk, k1, S.h, (T*)nullptr);
      hipLaunchKernelGGL(multi_axpy_kernel<T>, dim3(gn), dim3(256), 0, s, (const T*)V, ldv, k1, (const T*)S.h, w, n);
      hipLaunchKernelGGL(multi_dot_kernel<T>, dim3(nblk), dim3(256), 0, s, (const T*)V, ldv, k1, (const T*)w, part, n);
      hipLaunchKernelGGL(reduce_parts_kernel<T>, dim3(1), dim3(256), 0, s, (const T*)part, nblk, k1, h2, S.h);
      hipLaunchKernelGGL(multi_axpy_kernel<T>, dim3(gn), dim3(256), 0, s, (const T*)V, ldv, k1, (const T*)h2, w, n);
      norm(w, S.hn);
      hipLaunchKernelGGL(scale_into_kernel<T>, dim3(gn), dim3(256), 0, s, (const T*)w, (const double*)S.hn, V + (size_t)(k + 1) * ldv, n);
      hipLaunchKernelGGL(givens_kernel<T>, dim3(1), dim3(1), 0, s, S, k);
      double two[2];  // hn, res (adjacent)
      GM_HIP(hipMemcpyAsync(two, S.hn, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
      GM_HIP(hipStreamSynchronize(s));
      ++it;
      k_used = k + 1;
      hist[nh++] = two[1];
      if (two[1] <= tol || two[0] == 0.0) {
        converged = two[1] <= tol;
        break;
      }
    }
    if (k_used > 0) {  // x += Pr^-1 (V_k y),  H y = g
      hipLaunchKernelGGL(hess_solve_kernel<T>, dim3(1), dim3(1), 0, s, S, k_used);
      if (F) {
        hipLaunchKernelGGL(combine_kernel<T>, dim3(gn), dim3(256), 0, s, (const T*)V, ldv, k_used, (const T*)S.y, (const T*)nullptr, w, n);
        const int st = Pr(z, w, n, s);
        if (st != 0) throw st;
        T one = Scal<T>::one();
        GM_HIP(hipMemcpyAsync(S.y, &one, sizeof(T), hipMemcpyHostToDevice, s));
        GM_HIP(hipStreamSynchronize(s));
        hipLaunchKernelGGL(combine_kernel<T>, dim3(gn), dim3(256), 0, s, (const T*)z, ldv, 1, (const T*)S.y, (const T*)x, x, n);
      } else {
        hipLaunchKernelGGL(combine_kernel<T>, dim3(gn), dim3(256), 0, s, (const T*)V, ldv, k_used, (const T*)S.y, (const T*)x, x, n);
      }
    }
    A((const T*)x, r, b, n, s);
    norm(r, dscal);
    beta = read(dscal);
    converged = converged || beta <= tol;
    if (k_used == 0) break;
  }
  GM_HIP(hipStreamSynchronize(s));
  *iters_out = it;
  *conv_out = converged ? 1 : 0;
}


// the checks and defaults hs_gmres_* and hs_gmres_t_* share (A apart)
template <class T>
int gmres_check(hs_handle* F, int64_t n, int64_t* restart, int64_t* maxiter, double* reltol) {
  if (F && (hs_size(F) != n || (hs_is_complex(F) != 0) != (sizeof(T) == 16))) {
    hs_set_error(HS_ERR_DIMENSION, 0, "DimensionMismatch: the preconditioner is %lld x %lld %s, A is %lld x %lld", (long long)hs_size(F), (long long)hs_size(F),
                 hs_is_complex(F) ? "ComplexF64" : "Float64", (long long)n, (long long)n);
    return HS_ERR_DIMENSION;
  }
  // defaults of IterativeSolvers 0.9: restart = min(20, n), maxiter = n, reltol = sqrt(eps)
  if (*restart <= 0) *restart = std::min<int64_t>(20, n);
  if (*restart > GM_MAXK) {
    hs_set_error(HS_ERR_ARGUMENT, *restart, "ArgumentError: restart = %lld exceeds the limit of %d", (long long)*restart, GM_MAXK);
    return HS_ERR_ARGUMENT;
  }
  if (*maxiter < 0) *maxiter = n;
  if (!(*reltol >= 0.0)) *reltol = 1.4901161193847656e-08;
  return HS_OK;
}
// from the device check to the results; make_op(buf, s) puts A on the device (or finds it there) and returns the operator
template <class T, class MakeOp, class Prec>
int gmres_run(MakeOp make_op, const Prec& Pr, int64_t n, const T* b, T* x, int where, int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter,
              double* resnorm, int64_t* iters, int* converged, void* stream) {
  try {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) {
      hs_set_error(HS_ERR_DEVICE, 0, "no HIP device available: this library has no CPU fallback");
      return HS_ERR_DEVICE;
    }
    DevBuf buf;
    hipStream_t s = (hipStream_t)stream;
    const auto A = make_op(buf, s);
    std::vector<double> hist((size_t)maxiter + 2, 0.0);
    const T* db = b;
    T* dx = x;
    if (where == 0) {
      T* tb = buf.get<T>((size_t)n);
      T* tx = buf.get<T>((size_t)n);
      GM_HIP(hipMemcpy(tb, b, sizeof(T) * (size_t)n, hipMemcpyHostToDevice));
      if (use_x0) GM_HIP(hipMemcpy(tx, x, sizeof(T) * (size_t)n, hipMemcpyHostToDevice));
      db = tb;
      dx = tx;
    }
    gmres_device<T>(A, Pr, n, db, dx, use_x0, reltol, abstol, (int)restart, maxiter, hist.data(), iters, converged, s);
    if (where == 0) GM_HIP(hipMemcpy(x, dx, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost));
    if (resnorm)
      for (int64_t i = 0; i <= *iters; ++i) resnorm[i] = hist[(size_t)i];
    return HS_OK;
  } catch (int code) {
    return code;
  } catch (const std::bad_alloc&) {
    hs_set_error(HS_ERR_NOMEM, 0, "host allocation failed");
    return HS_ERR_NOMEM;
  }
}

template <class T>
int gmres_entry(hs_handle* F, int64_t n, const int64_t* colptr, const int64_t* rowval, const T* nz, const T* b, T* x, int where, int use_x0, double reltol, double abstol,
                int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged, void* stream) {
  if (n <= 0 || !colptr || !rowval || !nz || !b || !x || !iters || !converged) {
    hs_set_error(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_gmres needs A (CSC), b, x and the two result slots");
    return HS_ERR_ARGUMENT;
  }
  if (const int st = gmres_check<T>(F, n, &restart, &maxiter, &reltol)) return st;
  auto make_op = [&](DevBuf& buf, hipStream_t) {
    int64_t* d_rp;
    int32_t* d_ci;
    T* d_v;
    upload_csr<T>(buf, n, colptr, rowval, nz, &d_rp, &d_ci, &d_v);
    return CsrSpmv<T>{d_rp, d_ci, d_v};
  };
  return gmres_run<T>(make_op, PrecFwd<T>{F}, n, b, x, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters, converged, stream);
}

// hs_gmres_t_*: op(A) x = b right-preconditioned by op(Pr); A explicit or the handle's own
template <class T>
int gmres_t_entry(hs_handle* F, int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const T* nz, const T* b, T* x, int where, int use_x0, double reltol,
                  double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged, void* stream) {
  bool own = false;
  if (const int st = gm_check_op_args("hs_gmres_t_*", F, trans, colptr, rowval, nz, &own)) return st;
  if (trans == 0 && !own) return gmres_entry<T>(F, n, colptr, rowval, nz, b, x, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters, converged, stream);
  if (n <= 0 || !b || !x || !iters || !converged) {
    hs_set_error(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_gmres_t needs n >= 1, b, x and the two result slots");
    return HS_ERR_ARGUMENT;
  }
  if (const int st = gmres_check<T>(F, n, &restart, &maxiter, &reltol)) return st;
  if (own)
    if (const int st = hs_gmres_own_check(F, "hs_gmres_t_*", 1)) return st;
  if (F)  // what hs_ldiv_t_* refuses (or an unfactored handle) is refused here, before any device work: zero columns are solved
    if (const int st = prec_apply_probe<T>(F, trans, n)) return st;
  if (own)
    if (const int st = hs_gmres_own_check(F, "hs_gmres_t_*", 0)) return st;
  auto make_op = [&](DevBuf& buf, hipStream_t s) { return RowsSpmv<T>{gm_rows_of_op<T>(buf, F, trans, own, n, colptr, rowval, nz, s)}; };
  return gmres_run<T>(make_op, PrecOp<T>{F, trans}, n, b, x, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters, converged, stream);
}

}  // namespace

extern "C" int hs_gmres_d(hs_handle* Pr, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double* x, int where, int use_x0,
                          double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged, void* stream) {
  return gmres_entry<double>(Pr, n, colptr, rowval, nzval, b, x, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters, converged, stream);
}
extern "C" int hs_gmres_z(hs_handle* Pr, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double* x, int where, int use_x0,
                          double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged, void* stream) {
  return gmres_entry<cplx>(Pr, n, colptr, rowval, (const cplx*)nzval, (const cplx*)b, (cplx*)x, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters, converged,
                           stream);
}
extern "C" int hs_gmres_t_d(hs_handle* Pr, int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double* x, int where,
                            int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged, void* stream) {
  return gmres_t_entry<double>(Pr, trans, n, colptr, rowval, nzval, b, x, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters, converged, stream);
}
extern "C" int hs_gmres_t_z(hs_handle* Pr, int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval, const double* b, double* x, int where,
                            int use_x0, double reltol, double abstol, int64_t restart, int64_t maxiter, double* resnorm, int64_t* iters, int* converged, void* stream) {
  return gmres_t_entry<cplx>(Pr, trans, n, colptr, rowval, (const cplx*)nzval, (const cplx*)b, (cplx*)x, where, use_x0, reltol, abstol, restart, maxiter, resnorm, iters,
                             converged, stream);
}
