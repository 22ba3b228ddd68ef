// kernels_eigs.hip -- the device pieces of hs_eigs_* (hs_eigs.hip) that kernels_mod.hip does not already have (hs_eigs.h states each contract):
//
//   eigs_rotate     Out[:, :N] = V[:, :K] Q     the basis rotation of a restart, W <- W R^-1 of CholQR and the Ritz vectors; in place or not
//   eigs_chol_inv   G = R^H R, R^-1             the p x p Cholesky factor of a Gram matrix and its inverse, with the first dependent column
//   eigs_colsq      Y -= X diag(mu), ||.||_2    the residual of the Ritz pairs and column norms, row slabs + an ordered second pass
//   eigs_coldot     Re x_c^H y_c                the x^H op(M) x of the generalized problem (hs_eigs_gen_*), the same slabs and order
//   eigs_scale, eigs_init                    column normalisation, the seeded start block
//
// eigs_rotate computes the TRANSPOSED tile like mod_apply (kernels_mod.hip gives the lane maps of v_mfma_f64_16x16x4_f64): Q^T is the A operand
// (lane: column c0 + (lane & 15) of Q, row j0 + (lane >> 4)), the rows of V sit on lane & 15 of the B operand and of C/D, so the stores of Out
// are 128 contiguous bytes per lane group.  A workgroup owns 32 rows (ComplexF64: 16, real and imaginary parts in two planes) and holds ALL K
// entries of them in LDS, [tile][j][16 rows]: the four lane groups of a B-operand read are 64 consecutive doubles, and once the barrier behind
// the copy has passed nothing of V in these rows is read again -- which is what lets Out be V.  The four waves share the slab and split the
// (row tile, column tile) pairs; hsk_eigs_rotate_* checks the maps with exact integer data (tests/test_eigs_gpu.py).
#include "hs_eigs.h"

typedef double v4d __attribute__((ext_vector_type(4)));
#define MFMA64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

// ---- eigs_rotate ----------------------------------------------------------------------------------------------------------------------------
#define ER_PLANE (HS_EIGS_MAXBASIS * 16)  // doubles of one [j][16] plane
template <class T>
__global__ __launch_bounds__(256) void eigs_rotate_kernel(T* Out, long long ldo, const T* V, long long ldv, const T* Q, long long ldq, long long n, int K, int N) {
  constexpr bool CX = sizeof(T) == 16;
  constexpr int RT = CX ? 1 : 2;  // row tiles of 16 per workgroup
  __shared__ double vl[2 * ER_PLANE];  // Float64: plane = row tile; ComplexF64: plane 0 real parts, plane 1 imaginary parts
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
  const long long rbase = (long long)blockIdx.x * (16 * RT);
  const int kp = (K + 3) & ~3;
  for (int e = threadIdx.x; e < kp * 16 * RT; e += 256) {
    const int rt = e / (kp * 16), rem = e - rt * kp * 16, j = rem >> 4;
    const long long r = rbase + rt * 16 + (rem & 15);
    const bool in = j < K && r < n;
    if constexpr (CX) {
      const cplx v = in ? gld(V + (size_t)j * ldv + r) : cplx{0.0, 0.0};
      vl[rem] = v.re;
      vl[ER_PLANE + rem] = v.im;
    } else {
      vl[rt * ER_PLANE + rem] = in ? gld(V + (size_t)j * ldv + r) : 0.0;
    }
  }
  __syncthreads();  // from here on the workgroup reads its rows of V from LDS alone
  const int nct = (N + 15) / 16;
  for (int t = wv; t < nct * RT; t += 4) {
    const int rt = t % RT, c0 = (t / RT) * 16;
    const int cq = c0 + l15;
    const T* qp = Q + (size_t)min(cq, N - 1) * ldq;
    v4d acc = v4d{0.0, 0.0, 0.0, 0.0}, aci = v4d{0.0, 0.0, 0.0, 0.0};
    for (int j0 = 0; j0 < kp; j0 += 4) {
      const int j = j0 + l4;
      const bool in = cq < N && j < K;
      if constexpr (CX) {
        hs_d2u q = gld2(qp + min(j, K - 1));
        if (!in) { q.x = 0.0; q.y = 0.0; }
        const double vr = vl[j * 16 + l15], vi = vl[ER_PLANE + j * 16 + l15];
        acc = MFMA64(q.x, vr, acc);
        acc = MFMA64(-q.y, vi, acc);
        aci = MFMA64(q.x, vi, aci);
        aci = MFMA64(q.y, vr, aci);
      } else {
        double q = gld(qp + min(j, K - 1));
        if (!in) q = 0.0;
        acc = MFMA64(q, vl[rt * ER_PLANE + j * 16 + l15], acc);
      }
    }
    const long long r = rbase + rt * 16 + l15;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c = c0 + l4 + 4 * g;
      if (r < n && c < N) {
        if constexpr (CX)
          gst(Out + (size_t)c * ldo + r, cplx{acc[g], aci[g]});
        else
          gst(Out + (size_t)c * ldo + r, acc[g]);
      }
    }
  }
}
template <class T>
void launch_eigs_rotate(T* Out, int64_t ldo, const T* V, int64_t ldv, const T* Q, int64_t ldq, int64_t n, int K, int N, hipStream_t s) {
  if (n <= 0 || K <= 0 || N <= 0) return;
  const int rows = sizeof(T) == 16 ? 16 : 32;
  hipLaunchKernelGGL(eigs_rotate_kernel<T>, dim3((unsigned)((n + rows - 1) / rows)), dim3(256), 0, s, Out, (long long)ldo, V, (long long)ldv, Q, (long long)ldq, (long long)n, K,
                     N);
}
template void launch_eigs_rotate<double>(double*, int64_t, const double*, int64_t, const double*, int64_t, int64_t, int, int, hipStream_t);
template void launch_eigs_rotate<cplx>(cplx*, int64_t, const cplx*, int64_t, const cplx*, int64_t, int64_t, int, int, hipStream_t);

// ---- eigs_chol_inv --------------------------------------------------------------------------------------------------------------------------
// Row c of R per step: thread t >= c owns R[c, t] = (G[c, t] - sum_{i < c} conj(R[i, c]) R[i, t]) / R[c, c], the sum in the order of i.  Then
// thread t solves R x = e_t upwards for column t of the inverse.  R and Rinv live in global memory (one workgroup: the barrier orders them).
#define EIGS_DEF_TOL 5.048709793414476e-29  // (64 * 2^-53)^2
__device__ __forceinline__ double eg_re(double a) { return a; }
__device__ __forceinline__ double eg_re(cplx a) { return a.re; }
__device__ __forceinline__ double eg_cj(double a) { return a; }
__device__ __forceinline__ cplx eg_cj(cplx a) { return cplx{a.re, -a.im}; }
__device__ __forceinline__ double eg_real(double a, double) { return a; }
__device__ __forceinline__ cplx eg_real(double a, cplx) { return cplx{a, 0.0}; }
__device__ __forceinline__ double eg_div(double a, double d) { return a / d; }
__device__ __forceinline__ cplx eg_div(cplx a, double d) { return cplx{a.re / d, a.im / d}; }
__device__ __forceinline__ double eg_abs2(double a) { return a * a; }
__device__ __forceinline__ double eg_abs2(cplx a) { return a.re * a.re + a.im * a.im; }

template <class T>
__global__ __launch_bounds__(64) void eigs_chol_inv_kernel(const T* G, int ldg, int p, T* R, T* Ri, int* info) {
  __shared__ double sroot, sdmax;
  __shared__ int sbad;
  const int t = threadIdx.x;
  if (t < p)
    for (int i = 0; i < p; ++i) {
      gst(R + (size_t)t * p + i, Scal<T>::zero());
      gst(Ri + (size_t)t * p + i, Scal<T>::zero());
    }
  if (t == 0) {
    double d = 0.0;
    for (int i = 0; i < p; ++i) d = fmax(d, eg_re(gld(G + (size_t)i * ldg + i)));
    sdmax = d;
    sbad = -1;
  }
  __syncthreads();
  for (int c = 0; c < p; ++c) {
    T sum = Scal<T>::zero();
    if (t >= c && t < p) {
      sum = gld(G + (size_t)t * ldg + c);
      for (int i = 0; i < c; ++i) sum = Scal<T>::fnma(eg_cj(gld(R + (size_t)c * p + i)), gld(R + (size_t)t * p + i), sum);
    }
    if (t == c) {
      const double piv = eg_re(sum);
      if (!(piv > EIGS_DEF_TOL * sdmax))
        sbad = c;
      else
        sroot = sqrt(piv);
    }
    __syncthreads();
    if (sbad >= 0) {  // the same branch in every thread
      if (t == 0) *info = sbad;
      return;
    }
    if (t >= c && t < p) gst(R + (size_t)t * p + c, t == c ? eg_real(sroot, sum) : eg_div(sum, sroot));
    __syncthreads();
  }
  if (t < p) {
    T* x = Ri + (size_t)t * p;
    gst(x + t, eg_real(1.0 / eg_re(gld(R + (size_t)t * p + t)), Scal<T>::zero()));
    for (int i = t - 1; i >= 0; --i) {
      T sum = Scal<T>::zero();
      for (int l = i + 1; l <= t; ++l) sum = Scal<T>::fma(gld(R + (size_t)l * p + i), gld(x + l), sum);
      gst(x + i, eg_div(-sum, eg_re(gld(R + (size_t)i * p + i))));
    }
  }
  if (t == 0) *info = -1;
}
template <class T>
void launch_eigs_chol_inv(const T* G, int ldg, int p, T* R, T* Rinv, int* info, hipStream_t s) {
  hipLaunchKernelGGL(eigs_chol_inv_kernel<T>, dim3(1), dim3(64), 0, s, G, ldg, p, R, Rinv, info);
}
template void launch_eigs_chol_inv<double>(const double*, int, int, double*, double*, int*, hipStream_t);
template void launch_eigs_chol_inv<cplx>(const cplx*, int, int, cplx*, cplx*, int*, hipStream_t);

// ---- eigs_colsq, eigs_norm ------------------------------------------------------------------------------------------------------------------
// Workgroup (slab, c): thread t adds rows r0 + t, r0 + t + 256, ... of its slab in that order, then the 256 partial sums fold by halves.
template <class T>
__global__ __launch_bounds__(256) void eigs_colsq_kernel(T* Y, long long ldy, const T* X, long long ldx, const double* mu, const int* pair, long long n, int nc, double* part) {
  __shared__ double red[256];
  const int t = threadIdx.x, c = blockIdx.y;
  const int pc = pair ? gld(pair + c) : 0;
  const long long r0 = (long long)blockIdx.x * HS_EIGS_SLAB, r1 = min(n, r0 + (long long)HS_EIGS_SLAB);
  double acc = 0.0;
  if (pc >= 0) {
    const double mr = X ? gld(mu + 2 * c) : 0.0, mi = X ? gld(mu + 2 * c + 1) : 0.0;
    for (long long r = r0 + t; r < r1; r += 256) {
      T* y = Y + (size_t)c * ldy + r;
      if constexpr (sizeof(T) == 16) {
        cplx v = gld(y);
        if (X) {
          v = Scal<cplx>::fnma(cplx{mr, mi}, gld(X + (size_t)c * ldx + r), v);
          gst(y, v);
        }
        acc += eg_abs2(v);
      } else {
        double v = gld(y);
        if (pc == 0) {
          if (X) {
            v = fma(-mr, gld(X + (size_t)c * ldx + r), v);
            gst(y, v);
          }
          acc += v * v;
        } else {  // the pair (c, c + 1): (yr + i yi) -= (mr + i mi) (xr + i xi)
          double w = gld(y + ldy);
          if (X) {
            const double xr = gld(X + (size_t)c * ldx + r), xi = gld(X + (size_t)(c + 1) * ldx + r);
            v = fma(-mr, xr, fma(mi, xi, v));
            w = fma(-mi, xr, fma(-mr, xi, w));
            gst(y, v);
            gst(y + ldy, w);
          }
          acc += v * v + w * w;
        }
      }
    }
  }
  red[t] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  if (t == 0) gst(part + (size_t)blockIdx.x * nc + c, red[0]);
}
__global__ __launch_bounds__(256) void eigs_norm_kernel(const double* part, long long nslab, int nc, const int* pair, double* nrm) {
  const int c = threadIdx.x;
  if (c >= nc) return;
  const int cc = (pair && gld(pair + c) < 0) ? c - 1 : c;  // the second of a pair takes the figure of the first
  double acc = gld(part + cc);
  for (long long s = 1; s < nslab; ++s) acc += gld(part + s * nc + cc);
  gst(nrm + c, sqrt(acc));
}
template <class T>
void launch_eigs_resid(T* Y, int64_t ldy, const T* X, int64_t ldx, const double* mu, const int* pair, int64_t n, int nc, double* part, double* nrm, hipStream_t s) {
  if (n <= 0 || nc <= 0) return;
  hipLaunchKernelGGL(eigs_colsq_kernel<T>, dim3((unsigned)hs_eigs_slabs(n), (unsigned)nc), dim3(256), 0, s, Y, (long long)ldy, X, (long long)ldx, mu, pair, (long long)n, nc,
                     part);
  hipLaunchKernelGGL(eigs_norm_kernel, dim3(1), dim3(256), 0, s, (const double*)part, (long long)hs_eigs_slabs(n), nc, pair, nrm);
}
template void launch_eigs_resid<double>(double*, int64_t, const double*, int64_t, const double*, const int*, int64_t, int, double*, double*, hipStream_t);
template void launch_eigs_resid<cplx>(cplx*, int64_t, const cplx*, int64_t, const double*, const int*, int64_t, int, double*, double*, hipStream_t);

// ---- eigs_coldot ----------------------------------------------------------------------------------------------------------------------------
// The workgroup (slab, c) of eigs_colsq on two blocks: Re conj(x) y per row (ComplexF64: re*re then im*im), the second column of a Float64
// pair added in the same row step; the workgroup of the second member of a pair writes a zero that nothing reads.
template <class T>
__global__ __launch_bounds__(256) void eigs_coldot_kernel(const T* X, long long ldx, const T* Y, long long ldy, const int* pair, long long n, int nc, double* part) {
  __shared__ double red[256];
  const int t = threadIdx.x, c = blockIdx.y;
  const int pc = pair ? gld(pair + c) : 0;
  const long long r0 = (long long)blockIdx.x * HS_EIGS_SLAB, r1 = min(n, r0 + (long long)HS_EIGS_SLAB);
  double acc = 0.0;
  if (pc >= 0) {
    const T* x = X + (size_t)c * ldx;
    const T* y = Y + (size_t)c * ldy;
    for (long long r = r0 + t; r < r1; r += 256) {
      if constexpr (sizeof(T) == 16) {
        const cplx a = gld(x + r), b = gld(y + r);
        acc += a.re * b.re + a.im * b.im;
      } else {  // the expressions of eigs_colsq with its two equal factors apart: Y == X gives the bits of its squared norm
        const double a = gld(x + r), b = gld(y + r);
        if (pc == 0) {
          acc += a * b;
        } else {
          const double a2 = gld(x + ldx + r), b2 = gld(y + ldy + r);
          acc += a * b + a2 * b2;
        }
      }
    }
  }
  red[t] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  if (t == 0) gst(part + (size_t)blockIdx.x * nc + c, red[0]);
}
__global__ __launch_bounds__(256) void eigs_slabsum_kernel(const double* part, long long nslab, int nc, const int* pair, double* d) {
  const int c = threadIdx.x;
  if (c >= nc) return;
  const int cc = (pair && gld(pair + c) < 0) ? c - 1 : c;  // the second of a pair takes the figure of the first
  double acc = gld(part + cc);
  for (long long s = 1; s < nslab; ++s) acc += gld(part + s * nc + cc);
  gst(d + c, acc);
}
template <class T>
void launch_eigs_coldot(const T* X, int64_t ldx, const T* Y, int64_t ldy, const int* pair, int64_t n, int nc, double* part, double* d, hipStream_t s) {
  if (n <= 0 || nc <= 0) return;
  hipLaunchKernelGGL(eigs_coldot_kernel<T>, dim3((unsigned)hs_eigs_slabs(n), (unsigned)nc), dim3(256), 0, s, X, (long long)ldx, Y, (long long)ldy, pair, (long long)n, nc, part);
  hipLaunchKernelGGL(eigs_slabsum_kernel, dim3(1), dim3(256), 0, s, (const double*)part, (long long)hs_eigs_slabs(n), nc, pair, d);
}
template void launch_eigs_coldot<double>(const double*, int64_t, const double*, int64_t, const int*, int64_t, int, double*, double*, hipStream_t);
template void launch_eigs_coldot<cplx>(const cplx*, int64_t, const cplx*, int64_t, const int*, int64_t, int, double*, double*, hipStream_t);
__global__ __launch_bounds__(256) void eigs_sqrt_kernel(double* d, int nc) {
  const int c = threadIdx.x;
  if (c >= nc) return;
  const double v = gld(d + c);
  gst(d + c, v > 0.0 ? sqrt(v) : 0.0);
}
void launch_eigs_sqrt(double* d, int nc, hipStream_t s) {
  if (nc > 0) hipLaunchKernelGGL(eigs_sqrt_kernel, dim3(1), dim3(256), 0, s, d, nc);
}

// ---- eigs_scale, eigs_init ------------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void eigs_scale_kernel(T* X, long long ldx, const double* nrm, long long n) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  const double d = gld(nrm + blockIdx.y);
  if (r >= n || !(d > 0.0)) return;
  T* x = X + (size_t)blockIdx.y * ldx + r;
  gst(x, eg_div(gld(x), d));
}
template <class T>
void launch_eigs_scale(T* X, int64_t ldx, const double* nrm, int64_t n, int nc, hipStream_t s) {
  if (n <= 0 || nc <= 0) return;
  hipLaunchKernelGGL(eigs_scale_kernel<T>, dim3((unsigned)((n + 255) / 256), (unsigned)nc), dim3(256), 0, s, X, (long long)ldx, nrm, (long long)n);
}
template void launch_eigs_scale<double>(double*, int64_t, const double*, int64_t, int, hipStream_t);
template void launch_eigs_scale<cplx>(cplx*, int64_t, const double*, int64_t, int, hipStream_t);

// the counter-based generator of the norm estimator's start block (est_init_kernel, hs_normest.h): splitmix64 of (column key ^ row)
__device__ __forceinline__ uint64_t eg_sm64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ double eg_unif(uint64_t key, uint64_t i) { return (double)(eg_sm64(key ^ i) >> 11) * 0x1.0p-52 - 1.0; }  // in [-1, 1)
template <class T>
__global__ __launch_bounds__(256) void eigs_init_kernel(T* X, long long ldx, long long n, long long seed, int col0, int salt) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int c = blockIdx.y;
  const uint64_t key = eg_sm64(eg_sm64((uint64_t)seed) ^ ((uint64_t)salt << 8) ^ (uint64_t)(col0 + c));
  T* x = X + (size_t)c * ldx + r;
  if constexpr (sizeof(T) == 16)
    gst(x, cplx{eg_unif(key, 2 * (uint64_t)r), eg_unif(key, 2 * (uint64_t)r + 1)});
  else
    gst(x, eg_unif(key, (uint64_t)r));
}
template <class T>
void launch_eigs_init(T* X, int64_t ldx, int64_t n, int nc, int64_t seed, int col0, int salt, hipStream_t s) {
  if (n <= 0 || nc <= 0) return;
  hipLaunchKernelGGL(eigs_init_kernel<T>, dim3((unsigned)((n + 255) / 256), (unsigned)nc), dim3(256), 0, s, X, (long long)ldx, (long long)n, (long long)seed, col0, salt);
}
template void launch_eigs_init<double>(double*, int64_t, int64_t, int, int64_t, int, int, hipStream_t);
template void launch_eigs_init<cplx>(cplx*, int64_t, int64_t, int, int64_t, int, int, hipStream_t);
