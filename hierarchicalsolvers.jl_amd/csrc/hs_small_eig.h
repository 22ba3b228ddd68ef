// hs_small_eig.h -- the dense eigenproblem of the projected matrix of hs_eigs_* (hs_eigs.hip), on the host and without LAPACK: the library
// links none.  m <= 256, once per restart, so plain loops:
//
//   small_eig   H (m x m, any) -> eigenvalues w and unit eigenvectors Y: Householder reduction to Hessenberg form, single-shift QR with
//               deflation and accumulated transformations to the Schur form T = Z^H H Z, eigenvectors of T by back substitution, Y = Z y.
//               A real H is promoted by the caller.
//   house_q     an orthonormal basis Q (m x k) of the columns of Z (m x k) by Householder QR; real or complex.  Q is a product of
//               reflectors applied to the identity, so it is orthonormal to rounding whatever the rank of Z.
//
// Everything is column-major.  hsk_small_eig_z (include/hs_kernels.h) exposes small_eig to the tests.
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <vector>

namespace hs_se {

typedef std::complex<double> zc;
constexpr double SE_EPS = 2.220446049250313e-16;

inline double abs1(zc a) { return std::fabs(a.real()) + std::fabs(a.imag()); }
inline double conj_s(double a) { return a; }
inline zc conj_s(zc a) { return std::conj(a); }
inline double abs_s(double a) { return std::fabs(a); }
inline double abs_s(zc a) { return std::abs(a); }

// the rotation G = [c s; -conj(s) c] with G [x; y] = [r; 0]
inline void givens(zc x, zc y, double* c, zc* s) {
  const double ay = std::abs(y);
  if (ay == 0.0) {
    *c = 1.0;
    *s = 0.0;
    return;
  }
  const double ax = std::abs(x);
  if (ax == 0.0) {
    *c = 0.0;
    *s = std::conj(y) / ay;
    return;
  }
  const double nrm = std::hypot(ax, ay);
  *c = ax / nrm;
  *s = (x / ax) * std::conj(y) / nrm;
}

// H (m x m, ldh; overwritten by its Schur form T) -> w, Y (m x m, ldy; unit 2-norm columns, H Y = Y diag(w)).  Returns 0, or 1 + the index of
// an eigenvalue the QR iteration did not isolate in 60 sweeps (w and Y are then not to be used).
inline int small_eig(int m, zc* H, int ldh, zc* w, zc* Y, int ldy) {
  if (m <= 0) return 0;
#define SE_H(i, j) H[(size_t)(j) * ldh + (i)]
  std::vector<zc> Zs((size_t)m * m, zc(0.0)), v((size_t)m);
#define SE_Z(i, j) Zs[(size_t)(j) * m + (i)]
  for (int i = 0; i < m; ++i) SE_Z(i, i) = 1.0;
  // ---- Hessenberg form: reflector k zeroes H[k + 2 .., k]; Z accumulates them
  for (int k = 0; k + 2 < m; ++k) {
    double nrm = 0.0;
    for (int i = k + 1; i < m; ++i) nrm = std::hypot(nrm, std::abs(SE_H(i, k)));
    if (nrm == 0.0) continue;
    const zc x0 = SE_H(k + 1, k);
    const zc ph = std::abs(x0) == 0.0 ? zc(1.0) : x0 / std::abs(x0);
    for (int i = k + 1; i < m; ++i) v[i] = SE_H(i, k);
    v[k + 1] += ph * nrm;
    double vn = 0.0;
    for (int i = k + 1; i < m; ++i) vn = std::hypot(vn, std::abs(v[i]));
    if (vn == 0.0) continue;
    for (int i = k + 1; i < m; ++i) v[i] /= vn;
    for (int j = k; j < m; ++j) {  // H <- (I - 2 v v^H) H
      zc s = 0.0;
      for (int i = k + 1; i < m; ++i) s += std::conj(v[i]) * SE_H(i, j);
      s *= 2.0;
      for (int i = k + 1; i < m; ++i) SE_H(i, j) -= v[i] * s;
    }
    for (int i = 0; i < m; ++i) {  // H <- H (I - 2 v v^H), Z likewise
      zc s = 0.0, t = 0.0;
      for (int j = k + 1; j < m; ++j) {
        s += SE_H(i, j) * v[j];
        t += SE_Z(i, j) * v[j];
      }
      s *= 2.0;
      t *= 2.0;
      for (int j = k + 1; j < m; ++j) {
        SE_H(i, j) -= s * std::conj(v[j]);
        SE_Z(i, j) -= t * std::conj(v[j]);
      }
    }
    for (int i = k + 2; i < m; ++i) SE_H(i, k) = 0.0;
  }
  double hnorm = 0.0;
  for (int j = 0; j < m; ++j)
    for (int i = 0; i <= std::min(j + 1, m - 1); ++i) hnorm = std::max(hnorm, abs1(SE_H(i, j)));
  // ---- single-shift QR on the active block [l, hi], deflating at the bottom
  int hi = m - 1, iter = 0;
  while (hi > 0) {
    int l = hi;
    while (l > 0) {
      double sdiag = abs1(SE_H(l - 1, l - 1)) + abs1(SE_H(l, l));
      if (sdiag == 0.0) sdiag = hnorm;
      if (abs1(SE_H(l, l - 1)) <= SE_EPS * sdiag) break;
      --l;
    }
    if (l > 0) SE_H(l, l - 1) = 0.0;
    if (l == hi) {
      --hi;
      iter = 0;
      continue;
    }
    if (++iter > 60) return 1 + hi;
    zc shift;
    if (iter % 10 == 0) {  // an exceptional shift against a cycle
      shift = SE_H(hi, hi) + zc(0.75 * abs1(SE_H(hi, hi - 1)), 0.0);
    } else {  // Wilkinson: the eigenvalue of the trailing 2 x 2 block nearer its last entry
      const zc a = SE_H(hi - 1, hi - 1), b = SE_H(hi - 1, hi), c = SE_H(hi, hi - 1), d = SE_H(hi, hi);
      const zc t = 0.5 * (a - d), disc = std::sqrt(t * t + b * c);
      const zc den = std::abs(t + disc) >= std::abs(t - disc) ? t + disc : t - disc;
      shift = std::abs(den) == 0.0 ? d : d - b * c / den;
    }
    zc x = SE_H(l, l) - shift, y = SE_H(l + 1, l);
    for (int k = l; k < hi; ++k) {
      double c;
      zc s;
      givens(x, y, &c, &s);
      for (int j = std::max(k - 1, l); j < m; ++j) {  // rows k, k + 1
        const zc a = SE_H(k, j), b = SE_H(k + 1, j);
        SE_H(k, j) = c * a + s * b;
        SE_H(k + 1, j) = -std::conj(s) * a + c * b;
      }
      const int rmax = std::min(k + 2, hi);
      for (int i = 0; i <= rmax; ++i) {  // columns k, k + 1
        const zc a = SE_H(i, k), b = SE_H(i, k + 1);
        SE_H(i, k) = a * c + b * std::conj(s);
        SE_H(i, k + 1) = -a * s + b * c;
      }
      for (int i = 0; i < m; ++i) {
        const zc a = SE_Z(i, k), b = SE_Z(i, k + 1);
        SE_Z(i, k) = a * c + b * std::conj(s);
        SE_Z(i, k + 1) = -a * s + b * c;
      }
      if (k > l) SE_H(k + 1, k - 1) = 0.0;
      if (k + 1 < hi) {
        x = SE_H(k + 1, k);
        y = SE_H(k + 2, k);
      }
    }
  }
  // ---- eigenvectors of T by back substitution (a difference of diagonal entries below eps ||T|| is replaced by it), Y = Z y, unit norm
  double tnorm = 0.0;
  for (int j = 0; j < m; ++j)
    for (int i = 0; i <= j; ++i) tnorm = std::max(tnorm, abs1(SE_H(i, j)));
  const double small = std::max(SE_EPS * tnorm, 1e-300);
  for (int k = 0; k < m; ++k) {
    const zc tk = SE_H(k, k);
    w[k] = tk;
    v[k] = 1.0;
    for (int i = k - 1; i >= 0; --i) {
      zc s = 0.0;
      for (int j = i + 1; j <= k; ++j) s += SE_H(i, j) * v[j];
      zc den = SE_H(i, i) - tk;
      if (abs1(den) < small) den = small;
      v[i] = -s / den;
    }
    double nrm = 0.0;
    for (int i = 0; i < m; ++i) {
      zc s = 0.0;
      for (int j = 0; j <= k; ++j) s += SE_Z(i, j) * v[j];
      Y[(size_t)k * ldy + i] = s;
      nrm = std::hypot(nrm, std::abs(s));
    }
    if (nrm > 0.0)
      for (int i = 0; i < m; ++i) Y[(size_t)k * ldy + i] /= nrm;
  }
#undef SE_H
#undef SE_Z
  return 0;
}

// Q (m x k, ldq) = an orthonormal basis of the columns of Z (m x k, ldz; destroyed), k <= m
template <class S>
inline void house_q(int m, int k, S* Z, int ldz, S* Q, int ldq) {
  std::vector<S> vs((size_t)m * k, S(0.0));  // reflector j in column j, rows j .. m - 1, unit 2-norm (or zero)
  for (int j = 0; j < k; ++j) {
    S* z = Z + (size_t)j * ldz;
    S* v = vs.data() + (size_t)j * m;
    double nrm = 0.0;
    for (int i = j; i < m; ++i) nrm = std::hypot(nrm, abs_s(z[i]));
    if (nrm == 0.0) continue;
    const S ph = abs_s(z[j]) == 0.0 ? S(1.0) : z[j] / abs_s(z[j]);
    for (int i = j; i < m; ++i) v[i] = z[i];
    v[j] += ph * nrm;
    double vn = 0.0;
    for (int i = j; i < m; ++i) vn = std::hypot(vn, abs_s(v[i]));
    if (vn == 0.0) continue;
    for (int i = j; i < m; ++i) v[i] /= vn;
    for (int c = j; c < k; ++c) {
      S* zc_ = Z + (size_t)c * ldz;
      S s = S(0.0);
      for (int i = j; i < m; ++i) s += conj_s(v[i]) * zc_[i];
      s *= 2.0;
      for (int i = j; i < m; ++i) zc_[i] -= v[i] * s;
    }
  }
  for (int c = 0; c < k; ++c) {
    S* q = Q + (size_t)c * ldq;
    for (int i = 0; i < m; ++i) q[i] = S(i == c ? 1.0 : 0.0);
    for (int j = k - 1; j >= 0; --j) {
      const S* v = vs.data() + (size_t)j * m;
      S s = S(0.0);
      for (int i = j; i < m; ++i) s += conj_s(v[i]) * q[i];
      s *= 2.0;
      for (int i = j; i < m; ++i) q[i] -= v[i] * s;
    }
  }
}

}  // namespace hs_se
