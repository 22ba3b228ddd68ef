// hs_eigs.hip -- eigenpairs of A nearest a shift from the stored factorization of A_s = A - sigma I (hs_eigs_*; include/hs_solver.h): block
// Arnoldi on op(F)^-1 with thick restart, in Krylov-decomposition form.  hs_eigs_gen_* is the same loop for the pencil (A, M) with
// A_s = A - sigma M: the operator is C = op(F)^-1 op(M) (see "generalized" below); hs_eigs_* is that body with M = NULL.
//
// State: an orthonormal basis V (n x (m + p), on the device) and the host matrix G ((m + p) x m) with  op(F)^-1 V[:, :m] = V G.
//
//   expansion   W = op(F)^-1 V[:, m:m+p] (one hs_ldiv_block_dev_t_* call) lands in V[:, m+p:m+2p]; two passes of classical Gram-Schmidt
//               against V[:, :m+p] (launch_mod_inner, launch_mod_apply), CholQR twice (launch_mod_inner(W, W), launch_eigs_chol_inv,
//               launch_eigs_rotate in place); the coefficients h and R become columns m .. m+p-1 of G.  A dependent column (chol_inv names
//               it) is replaced by a seeded random vector and the block is orthogonalised again; the row of R that carried the dropped
//               remainder is zero.
//   restart     when no further block fits into ncv columns: eigenpairs (theta, y) of H = G[:m] on the host (hs_small_eig.h), sorted by
//               |theta| descending, est_c = ||G[m:] y_c||_2 / |theta_c|; stop when the first nout are at or below tol; else an orthonormal
//               basis Q of the kept eigenvectors (Float64: of their real and imaginary parts, pairs kept whole), G <- [Q^H H Q; B Q],
//               V[:, :keep] <- V[:, :m] Q in place (launch_eigs_rotate), the last block moves down behind them.
//   finish      X = V[:, :m] Y normalised, mu = 1 / theta, lambda = sigma + mu, true residuals ||op(A_s) X - X diag(mu)|| with the handle's
//               own A_s (hs_gmres_own_rows, spmm_op_kernel, launch_eigs_resid).
//
//   generalized an expansion first forms T = op(M) V[:, m:m+p] (launch_spmm_op over the rows of op(M): a CSR of M for trans = 0, the CSC arrays
//               of M read in place otherwise, conjugated on load for trans = 2) and solves from T.  inner = 1: every inner product of
//               orth_block is taken against MW = op(M) W, recomputed by SpMM after every change of W, so V is op(M)-orthonormal; the Ritz
//               vectors are scaled to x^H op(M) x = 1 (launch_eigs_coldot).  The residual is op(A_s) X - (op(M) X) diag(mu).
//
// Everything the device computes has one summation order per element and the host part is sequential, so two calls return the same bits.
#include <chrono>
#include <complex>
#include <new>
#include <string>

#include "hs_gmres_common.h"  // RowsOf, launch_spmm_op; includes hs_solver.h, hs_common.h, hs_host.h, hs_gmres_op.h
#include "hs_eigs.h"
#include "hs_small_eig.h"
#include "../../include/hs_kernels.h"

namespace {

using hs_se::zc;

enum { EI_SECONDS = 0, EI_SOLVES, EI_COLAPPS, EI_RESTARTS, EI_ORTH, EI_REPLACED, EI_WORK_BYTES, EI_NCV };
thread_local double g_einfo[8] = {0, 0, 0, 0, 0, 0, 0, 0};
enum { GI_PRODUCTS = 0, GI_COLUMNS, GI_BYTES, GI_INNER };  // hs_eigs_gen_info
thread_local double g_ginfo[4] = {0, 0, 0, 0};
thread_local double g_mprod_seconds = 0.0;  // host-clock seconds of the products with op(M), taken only while hsk_eigs_phase_timing is on
// host-clock seconds of the last call by phase (hsk_eigs_phases): block solves, orthogonalisation, restarts (host eigenproblem and rotation),
// Ritz vectors and residuals.  Every phase ends in a synchronisation of its own except the block solve, which gets one only while
// hsk_eigs_phase_timing is on (off: its time is counted with the orthogonalisation that follows).
enum { EP_SOLVE = 0, EP_ORTH, EP_RESTART, EP_FINISH };
thread_local double g_ephase[4] = {0, 0, 0, 0};
bool g_phase_sync = false;
struct PhaseClock {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void lap(int phase) {
    const auto t1 = std::chrono::steady_clock::now();
    g_ephase[phase] += std::chrono::duration<double>(t1 - t0).count();
    t0 = t1;
  }
};

template <class T>
struct HostOf;
template <>
struct HostOf<double> {
  typedef double type;
};
template <>
struct HostOf<cplx> {
  typedef zc type;
};

inline double cj(double a) { return a; }
inline zc cj(zc a) { return std::conj(a); }

template <class T>
int block_solve(hs_handle* F, int t, T* C, int64_t ldc, const T* B, int64_t ldb, int64_t n, int64_t nc, hipStream_t s) {
  if (sizeof(T) == 16) return hs_ldiv_block_dev_t_z(F, t, (double*)C, ldc, (const double*)B, ldb, n, nc, (void*)s);
  return hs_ldiv_block_dev_t_d(F, t, (double*)C, ldc, (const double*)B, ldb, n, nc, (void*)s);
}

template <class T>
struct Eigs {
  typedef typename HostOf<T>::type S;
  hs_handle* F = nullptr;
  int trans = 0, p = 0, ncv = 0, mcap = 0;  // mcap = ncv + 1: the columns of G (a restart may keep one more vector than planned)
  int64_t n = 0, ldv = 0, seed = 0;
  hipStream_t s = nullptr;
  T *V = nullptr, *part = nullptr, *dh = nullptr, *dG = nullptr, *dR = nullptr, *dRi = nullptr, *dQ = nullptr;
  double *dpart = nullptr, *dnrm = nullptr;
  int* dInfo = nullptr;
  std::vector<S> G;  // (mcap + p) x mcap, ld = mcap + p
  int ldg = 0, draws = 0;
  // the generalized problem: the rows of op(M) (has_m), the op(M) inner product (minner, only with has_m) and its block MW = op(M) W
  RowsOf<T> M;
  bool has_m = false, minner = false;
  T* MW = nullptr;

  S& g(int i, int j) { return G[(size_t)j * ldg + i]; }

  // Y (n x nc, ld n) = op(M) X
  void mult_m(const T* X, int64_t ldx, T* Y, int nc) {
    if (g_phase_sync) {  // a synchronisation before and behind each product, so that the clock sees the product alone
      HS_HIP(hipStreamSynchronize(s));
      const auto t0 = std::chrono::steady_clock::now();
      launch_spmm_op<T>(M, X, ldx, nullptr, Y, n, nullptr, 0, nullptr, n, nc, s);
      HS_HIP(hipStreamSynchronize(s));
      g_mprod_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    } else {
      launch_spmm_op<T>(M, X, ldx, nullptr, Y, n, nullptr, 0, nullptr, n, nc, s);
    }
    g_ginfo[GI_PRODUCTS] += 1;
    g_ginfo[GI_COLUMNS] += nc;
  }
  // the right-hand block of an inner product with W: W itself, or op(M) W computed now (never updated: one summation order per element)
  const T* metric(const T* W) {
    if (!minner) return W;
    mult_m(W, ldv, MW, p);
    return MW;
  }

  // Orthonormalise W = V[:, k:k+p] against V[:, :k] and in itself, in place: W_in = V[:, :k] h + W_out R; h (k x p) and R (p x p) go to
  // G[0:k, col0:col0+p] and G[k:k+p, col0:col0+p] (col0 < 0: the start block, nothing is recorded).  With minner "orthonormal" is meant in
  // the op(M) inner product, and the deficiency rule of chol_inv applies to the M-Gram matrix.
  void orth_block(int k, int col0) {
    T* W = V + (size_t)k * ldv;
    std::vector<S> Racc((size_t)p * p, S(0.0)), Hacc((size_t)k * p, S(0.0)), h((size_t)k * p), R((size_t)p * p), tmp((size_t)p * p);
    for (int i = 0; i < p; ++i) Racc[(size_t)i * p + i] = S(1.0);
    for (int attempt = 0; attempt <= p; ++attempt) {
      for (int pass = 0; pass < 2 && k > 0; ++pass) {
        const T* mw = metric(W);
        launch_mod_inner<T>(V, ldv, mw, minner ? n : ldv, n, k, p, 0, part, dh, k, s);
        launch_mod_apply<T>(W, ldv, V, ldv, dh, k, n, k, p, 0, s);
        HS_HIP(hipMemcpyAsync(h.data(), dh, sizeof(T) * (size_t)k * p, hipMemcpyDeviceToHost, s));
        HS_HIP(hipStreamSynchronize(s));
        for (int c = 0; c < p; ++c)  // Hacc += h Racc (Racc upper)
          for (int l = 0; l <= c; ++l) {
            const S r = Racc[(size_t)c * p + l];
            if (r == S(0.0)) continue;
            for (int i = 0; i < k; ++i) Hacc[(size_t)c * k + i] += h[(size_t)l * k + i] * r;
          }
        g_einfo[EI_ORTH] += 1;
      }
      int bad = -1;
      for (int round = 0; round < 2; ++round) {
        const T* mw = metric(W);
        launch_mod_inner<T>(W, ldv, mw, minner ? n : ldv, n, p, p, 0, part, dG, p, s);
        if (minner && col0 < 0 && attempt == 0 && round == 0) {  // the start block as given: a diagonal entry v^H op(M) v that is not positive
          HS_HIP(hipMemcpyAsync(tmp.data(), dG, sizeof(T) * (size_t)p * p, hipMemcpyDeviceToHost, s));
          HS_HIP(hipStreamSynchronize(s));
          for (int c = 0; c < p; ++c)
            if (!(std::real(tmp[(size_t)c * p + c]) > 0.0))
              HS_FAIL(HS_ERR_ARGUMENT, c, "ArgumentError: hs_eigs_gen_*: inner = 1 needs a Hermitian positive definite M: v^H op(M) v = %g for column %d of the start block",
                      std::real(tmp[(size_t)c * p + c]), c + 1);
        }
        launch_eigs_chol_inv<T>(dG, p, p, dR, dRi, dInfo, s);
        HS_HIP(hipMemcpyAsync(&bad, dInfo, sizeof(int), hipMemcpyDeviceToHost, s));
        HS_HIP(hipMemcpyAsync(R.data(), dR, sizeof(T) * (size_t)p * p, hipMemcpyDeviceToHost, s));
        HS_HIP(hipStreamSynchronize(s));
        if (bad >= 0) break;
        launch_eigs_rotate<T>(W, ldv, W, ldv, dRi, p, n, p, p, s);
        for (int c = 0; c < p; ++c)  // Racc <- R Racc
          for (int i = 0; i < p; ++i) {
            S acc = S(0.0);
            for (int l = i; l <= c; ++l) acc += R[(size_t)l * p + i] * Racc[(size_t)c * p + l];
            tmp[(size_t)c * p + i] = acc;
          }
        Racc = tmp;
      }
      if (bad < 0) {
        if (col0 >= 0)
          for (int c = 0; c < p; ++c) {
            for (int i = 0; i < k; ++i) g(i, col0 + c) = Hacc[(size_t)c * k + i];
            for (int i = 0; i < p; ++i) g(k + i, col0 + c) = Racc[(size_t)c * p + i];
          }
        return;
      }
      // column `bad` depends on the basis: a seeded random unit vector takes its place, and no original column keeps a component through it
      T* wb = W + (size_t)bad * ldv;
      launch_eigs_init<T>(wb, ldv, n, 1, seed, draws++, 1, s);
      launch_eigs_resid<T>(wb, ldv, nullptr, 0, nullptr, nullptr, n, 1, dpart, dnrm, s);
      launch_eigs_scale<T>(wb, ldv, dnrm, n, 1, s);
      for (int c = 0; c < p; ++c) Racc[(size_t)c * p + bad] = S(0.0);
      g_einfo[EI_REPLACED] += 1;
    }
    HS_FAIL(HS_ERR_SINGULAR, k, "hs_eigs_*: the block at column %d stays rank deficient after %d replaced columns", k, p + 1);
  }
};

// |theta| descending (stable); Float64: the members of a conjugate pair adjacent, the one with the negative imaginary part first -- it gives
// the lambda with the positive one.  pair[c]: 0 a column of its own, +1 / -1 the first / second of a pair.
void sort_ritz(int m, bool real_h, const std::vector<zc>& w, std::vector<int>& order, std::vector<int>& pair) {
  std::vector<int> ord((size_t)m);
  for (int i = 0; i < m; ++i) ord[(size_t)i] = i;
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return std::abs(w[(size_t)a]) > std::abs(w[(size_t)b]); });
  order.clear();
  pair.assign((size_t)m, 0);
  if (!real_h) {
    order = ord;
    return;
  }
  double scale = 1e-300;
  for (int i = 0; i < m; ++i) scale = std::max(scale, std::abs(w[(size_t)i]));
  const double cut = 64.0 * 1.1102230246251565e-16 * scale;
  std::vector<char> used((size_t)m, 0);
  for (int a = 0; a < m; ++a) {
    const int i = ord[(size_t)a];
    if (used[(size_t)i]) continue;
    used[(size_t)i] = 1;
    int j = -1;
    if (std::fabs(w[(size_t)i].imag()) > cut) {
      double best = 0.0;
      for (int b = 0; b < m; ++b) {
        const int q = ord[(size_t)b];
        if (used[(size_t)q]) continue;
        const double d = std::abs(w[(size_t)q] - std::conj(w[(size_t)i]));
        if (j < 0 || d < best) {
          j = q;
          best = d;
        }
      }
    }
    if (j < 0) {
      order.push_back(i);
      continue;
    }
    used[(size_t)j] = 1;
    const bool ifirst = w[(size_t)i].imag() < 0.0;
    pair[order.size()] = 1;
    order.push_back(ifirst ? i : j);
    pair[order.size()] = -1;
    order.push_back(ifirst ? j : i);
  }
}

// column c of the kept / returned vectors in the element type of the handle
void ritz_column(int m, const zc* Y, int ldy, const std::vector<int>& order, const std::vector<int>& pair, int c, zc* out) {
  const zc* y = Y + (size_t)order[(size_t)c] * ldy;
  for (int i = 0; i < m; ++i) out[i] = y[i];
}
void ritz_column(int m, const zc* Y, int ldy, const std::vector<int>& order, const std::vector<int>& pair, int c, double* out) {
  if (pair[(size_t)c] == 0) {  // a real eigenvalue: the phase that makes the largest entry real
    const zc* y = Y + (size_t)order[(size_t)c] * ldy;
    int big = 0;
    for (int i = 1; i < m; ++i)
      if (std::abs(y[i]) > std::abs(y[big])) big = i;
    const double ab = std::abs(y[big]);
    const zc ph = ab > 0.0 ? std::conj(y[big]) / ab : zc(1.0);
    for (int i = 0; i < m; ++i) out[i] = (y[i] * ph).real();
    return;
  }
  const zc* y = Y + (size_t)order[(size_t)(pair[(size_t)c] > 0 ? c : c - 1)] * ldy;
  for (int i = 0; i < m; ++i) out[i] = pair[(size_t)c] > 0 ? y[i].real() : y[i].imag();
}

template <class T>
int refused_by_block_solve(hs_handle* F, int trans, int64_t n) {
  return block_solve<T>(F, trans, nullptr, n, nullptr, n, n, 0, nullptr);
}

// The CSC arrays of M as the caller passed them (1-based SparseMatrixCSC fields); all null: M = I
template <class T>
struct HostCsc {
  const int64_t* colptr = nullptr;
  const int64_t* rowval = nullptr;
  const T* nzval = nullptr;
};

// What upload_csr / upload_csc would find, found on the host before anything else is touched -- and what they do not look at (a colptr that
// is not monotone).  Returns whether M is given.
template <class T>
bool check_m_args(const char* fn, const HostCsc<T>& M, int inner, int64_t n) {
  if (inner < 0 || inner > 1) HS_FAIL(HS_ERR_ARGUMENT, inner, "ArgumentError: %s: inner = %d (0: Euclidean, 1: the op(M) inner product)", fn, inner);
  const int given = (M.colptr ? 1 : 0) + (M.rowval ? 1 : 0) + (M.nzval ? 1 : 0);
  if (given != 0 && given != 3) HS_FAIL(HS_ERR_ARGUMENT, given, "ArgumentError: %s: mcolptr, mrowval and mnzval must all be given, or all be NULL (M = I)", fn);
  if (given == 0) return false;
  if (n > (int64_t)INT32_MAX)
    HS_FAIL(HS_ERR_ARGUMENT, n, "ArgumentError: %s: n = %lld exceeds the 32-bit indices of the device matrix (limit %d)", fn, (long long)n, INT32_MAX);
  if (M.colptr[0] != 1) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: mcolptr must be 1-based (SparseMatrixCSC)", fn);
  for (int64_t c = 0; c < n; ++c)
    if (M.colptr[c + 1] < M.colptr[c])
      HS_FAIL(HS_ERR_ARGUMENT, c + 1, "ArgumentError: %s: mcolptr[%lld] = %lld is below mcolptr[%lld] = %lld", fn, (long long)c + 2, (long long)M.colptr[c + 1], (long long)c + 1,
              (long long)M.colptr[c]);
  const int64_t nnz = M.colptr[n] - 1;
  for (int64_t e = 0; e < nnz; ++e)
    if (M.rowval[e] < 1 || M.rowval[e] > n)
      HS_FAIL(HS_ERR_ARGUMENT, e, "ArgumentError: %s: mrowval[%lld] = %lld outside 1:%lld", fn, (long long)e + 1, (long long)M.rowval[e], (long long)n);
  return true;
}

template <class T>
void eigs_run(hs_handle* F, int trans, int64_t n, const HostCsc<T>& Mh, int inner, int64_t nev, int64_t ncv, int64_t block, double sigma_re, double sigma_im, double tol, int64_t maxrestart, const T* V0,
              int64_t ldv0, int64_t seed, int where, double* lam, T* X, int64_t ldx, double* resid, double* est, int64_t* nout_, int64_t* nconv_, void* stream, HsDevBuf& buf,
              hipEvent_t* e0, hipEvent_t* e1) {
  typedef typename HostOf<T>::type S;
  const char* fn = "hs_eigs_*";
  const bool real_h = sizeof(T) == 8;
  // ---- arguments: nothing is written before all of them (and the handle) have passed
  const HsHandleView v = hs_view_of(F, fn);
  hs_check_trans(fn, trans);
  if ((v.is_complex != 0) != !real_h || n != v.n)
    HS_FAIL(HS_ERR_DIMENSION, 0, "DimensionMismatch: %s: called for %s with n = %lld, F is %lld x %lld %s", fn, real_h ? "Float64" : "ComplexF64", (long long)n, (long long)v.n,
            (long long)v.n, v.is_complex ? "ComplexF64" : "Float64");
  if (nev < 1) HS_FAIL(HS_ERR_ARGUMENT, nev, "ArgumentError: %s: nev = %lld < 1", fn, (long long)nev);
  if (block < 0 || ncv < 0) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: ncv = %lld, block = %lld (0 selects the default)", fn, (long long)ncv, (long long)block);
  if (block == 0) block = 16;
  if (block > HS_EIGS_MAXBLOCK) HS_FAIL(HS_ERR_ARGUMENT, block, "ArgumentError: %s: block = %lld exceeds the limit of %d", fn, (long long)block, HS_EIGS_MAXBLOCK);
  if (ncv == 0) {  // the multiple of block >= max(2 nev + block, 4 block), capped by ncv + block <= 256
    const int64_t want = std::max<int64_t>(2 * nev + block, 4 * block);
    ncv = (want + block - 1) / block * block;
    const int64_t cap = std::min<int64_t>(HS_EIGS_MAXBASIS - block, n - block);
    if (ncv > cap) ncv = cap;
  }
  if (ncv + block > HS_EIGS_MAXBASIS)
    HS_FAIL(HS_ERR_ARGUMENT, ncv, "ArgumentError: %s: ncv + block = %lld + %lld exceeds the limit of %d basis columns", fn, (long long)ncv, (long long)block, HS_EIGS_MAXBASIS);
  if (ncv < nev + block) HS_FAIL(HS_ERR_ARGUMENT, ncv, "ArgumentError: %s: ncv = %lld < nev + block = %lld + %lld", fn, (long long)ncv, (long long)nev, (long long)block);
  if (n < ncv + block) HS_FAIL(HS_ERR_ARGUMENT, n, "ArgumentError: %s: n = %lld < ncv + block = %lld + %lld", fn, (long long)n, (long long)ncv, (long long)block);
  if (!lam || !resid || !est || !nout_ || !nconv_) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: lam, resid, est, nout and nconv must not be NULL", fn);
  if (where != 0 && where != 1) HS_FAIL(HS_ERR_ARGUMENT, where, "ArgumentError: %s: where = %d (0: host pointers, 1: device pointers)", fn, where);
  if ((V0 && ldv0 < n) || (X && ldx < n)) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: ldv0 = %lld, ldx = %lld below n = %lld", fn, (long long)ldv0, (long long)ldx, (long long)n);
  if (real_h && sigma_im != 0.0) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: a complex shift on a Float64 factorization (factor A - sigma I as ComplexF64)", fn);
  if (!(tol >= 0.0) || maxrestart < 0 || !std::isfinite(sigma_re) || !std::isfinite(sigma_im))
    HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: tol = %g, maxrestart = %lld, sigma = (%g, %g)", fn, tol, (long long)maxrestart, sigma_re, sigma_im);
  const bool has_m = check_m_args<T>(fn, Mh, inner, n);
  if (const int st = hs_gmres_own_check(F, fn, 1)) throw st;  // more than one rank: neither the block solve nor the handle's own A
  {  // what hs_ldiv_block_dev_t_* refuses is refused here, with its words
    const int st = refused_by_block_solve<T>(F, trans, n);
    if (st == HS_ERR_UNSUPPORTED) {
      const std::string why = hs_last_error();
      HS_FAIL(HS_ERR_UNSUPPORTED, hs_last_error_info(), "%s: the block solve does not serve this handle (%s)", fn, why.c_str());
    }
    if (st != HS_OK) throw st;
  }
  if (const int st = hs_gmres_own_check(F, fn, 0)) throw st;
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) HS_FAIL(HS_ERR_DEVICE, 0, "no HIP device available: this library has no CPU fallback");

  // ---- workspace
  Eigs<T> E;
  const int p = (int)block, mcap = (int)ncv + 1;
  const int ncols = (int)std::min<int64_t>(ncv + 1 + p, n);  // the basis may grow to ncv + 1 + p columns when n allows
  hipStream_t s = (hipStream_t)stream;
  E.F = F;
  E.trans = trans;
  E.p = p;
  E.ncv = (int)ncv;
  E.mcap = mcap;
  E.n = n;
  E.ldv = n;
  E.seed = seed;
  E.s = s;
  E.ldg = mcap + p;
  E.G.assign((size_t)E.ldg * mcap, S(0.0));
  const int64_t ldv = n;
  const int nx = (int)nev + 1;
  size_t bytes = 0;
  auto take = [&](size_t cnt_, size_t size) {
    bytes += std::max<size_t>(cnt_ * size, 256);
    return cnt_;
  };
  E.V = buf.get<T>(take((size_t)n * ncols, sizeof(T)));
  E.part = buf.get<T>(take((size_t)hs_mod_slabs(n) * HS_EIGS_MAXBASIS * p, sizeof(T)));
  E.dh = buf.get<T>(take((size_t)HS_EIGS_MAXBASIS * p, sizeof(T)));
  E.dG = buf.get<T>(take((size_t)p * p, sizeof(T)));
  E.dR = buf.get<T>(take((size_t)p * p, sizeof(T)));
  E.dRi = buf.get<T>(take((size_t)p * p, sizeof(T)));
  E.dQ = buf.get<T>(take((size_t)HS_EIGS_MAXBASIS * HS_EIGS_MAXBASIS, sizeof(T)));
  E.dpart = buf.get<double>(take((size_t)hs_eigs_slabs(n) * nx, sizeof(double)));
  E.dnrm = buf.get<double>(take((size_t)nx, sizeof(double)));
  E.dInfo = buf.get<int>(take(1, sizeof(int)));
  T* dX = buf.get<T>(take((size_t)n * nx, sizeof(T)));
  T* dAX = buf.get<T>(take((size_t)n * nx, sizeof(T)));
  double* dmu = buf.get<double>(take((size_t)2 * nx, sizeof(double)));
  int* dpair = buf.get<int>(take((size_t)nx, sizeof(int)));
  for (double& q : g_einfo) q = 0.0;
  for (double& q : g_ephase) q = 0.0;
  for (double& q : g_ginfo) q = 0.0;
  g_mprod_seconds = 0.0;
  // ---- M on the device, once per call, and the blocks only the generalized problem needs: T = op(M) V[:, m:m+p], MX = op(M) X, MW
  T *dT = nullptr, *dMX = nullptr;
  if (has_m) {
    E.has_m = true;
    E.minner = inner == 1;
    dT = buf.get<T>(take((size_t)n * p, sizeof(T)));
    dMX = buf.get<T>(take((size_t)n * nx, sizeof(T)));
    if (E.minner) E.MW = buf.get<T>(take((size_t)n * p, sizeof(T)));
    int64_t* mp = nullptr;
    int32_t* mi = nullptr;
    T* mv = nullptr;
    if (trans == 0)
      upload_csr<T>(buf, n, Mh.colptr, Mh.rowval, Mh.nzval, &mp, &mi, &mv);
    else
      upload_csc<T>(buf, n, Mh.colptr, Mh.rowval, Mh.nzval, &mp, &mi, &mv);
    E.M.ptr = mp;
    E.M.idx = mi;
    E.M.val = mv;
    E.M.conj = trans == 2;
    const size_t nnz = (size_t)(Mh.colptr[n] - 1);
    g_ginfo[GI_BYTES] = (double)(std::max<size_t>(sizeof(int64_t) * ((size_t)n + 1), 256) + std::max<size_t>(sizeof(int32_t) * nnz, 256) + std::max<size_t>(sizeof(T) * nnz, 256));
    g_ginfo[GI_INNER] = E.minner ? 1.0 : 0.0;
  }
  g_einfo[EI_WORK_BYTES] = (double)bytes;
  g_einfo[EI_NCV] = (double)ncv;
  HS_HIP(hipEventCreate(e0));
  HS_HIP(hipEventCreate(e1));
  HS_HIP(hipEventRecord(*e0, s));

  // ---- the start block
  if (V0)
    HS_HIP(hipMemcpy2DAsync(E.V, ldv * sizeof(T), V0, ldv0 * sizeof(T), n * sizeof(T), p, where ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
  else
    launch_eigs_init<T>(E.V, ldv, n, p, seed, 0, 0, s);
  PhaseClock clk;
  E.orth_block(0, -1);
  clk.lap(EP_ORTH);

  // ---- expansions and restarts
  int m = 0, nout = 0, nconv = 0, restarts = 0;
  int64_t lim = ncv;  // ncv, or ncv + 1 after a restart that kept one more vector to keep a conjugate pair whole
  std::vector<zc> Hc, w, Y;
  std::vector<int> order, pair;
  std::vector<double> estv;
  for (;;) {
    while (m + p <= lim && m + 2 * p <= ncols) {
      const T* rhs = E.V + (size_t)m * ldv;
      if (has_m) {
        E.mult_m(rhs, ldv, dT, p);
        rhs = dT;
      }
      const int st = block_solve<T>(F, trans, E.V + (size_t)(m + p) * ldv, ldv, rhs, has_m ? n : ldv, n, p, s);
      if (st != HS_OK) throw st;
      g_einfo[EI_SOLVES] += 1;
      g_einfo[EI_COLAPPS] += p;
      if (g_phase_sync) {
        HS_HIP(hipStreamSynchronize(s));
        clk.lap(EP_SOLVE);
      }
      E.orth_block(m + p, m);
      clk.lap(EP_ORTH);
      m += p;
    }
    Hc.assign((size_t)m * m, zc(0.0));
    w.assign((size_t)m, zc(0.0));
    Y.assign((size_t)m * m, zc(0.0));
    for (int j = 0; j < m; ++j)
      for (int i = 0; i < m; ++i) Hc[(size_t)j * m + i] = zc(E.g(i, j));
    const int bad = hs_se::small_eig(m, Hc.data(), m, w.data(), Y.data(), m);
    if (bad) HS_FAIL(HS_ERR_SINGULAR, bad - 1, "%s: the QR iteration on the %d x %d projected matrix did not converge", fn, m, m);
    sort_ritz(m, real_h, w, order, pair);
    estv.assign((size_t)m, 0.0);
    for (int c = 0; c < m; ++c) {
      const zc* y = Y.data() + (size_t)order[(size_t)c] * m;
      double nb = 0.0;
      for (int i = 0; i < p; ++i) {
        zc acc = 0.0;
        for (int j = 0; j < m; ++j) acc += zc(E.g(m + i, j)) * y[j];
        nb = std::hypot(nb, std::abs(acc));
      }
      estv[(size_t)c] = nb / std::abs(w[(size_t)order[(size_t)c]]);
    }
    nout = (int)nev + (pair[(size_t)nev - 1] == 1 ? 1 : 0);
    nconv = 0;
    for (int c = 0; c < nout; ++c)
      if (estv[(size_t)c] <= tol) ++nconv;
    if (nconv == nout || restarts >= maxrestart) break;
    // ---- contraction to `keep` vectors
    const int t = (int)std::max<int64_t>(1, (ncv - nev - p) / p);
    int keep = std::max(m - t * p, 1);
    lim = ncv;
    if (pair[(size_t)keep - 1] == 1) {
      const bool more = ncv + 1 + p <= ncols && keep + 1 < m;
      keep += more ? 1 : -1;
      if (more) lim = ncv + 1;
    }
    if (keep < 1) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: ncv = %lld leaves no room to restart", fn, (long long)ncv);
    std::vector<S> Z((size_t)m * keep), Q((size_t)m * keep), HQ((size_t)m * keep), Gn((size_t)(keep + p) * keep, S(0.0));
    for (int c = 0; c < keep; ++c) ritz_column(m, Y.data(), m, order, pair, c, Z.data() + (size_t)c * m);
    hs_se::house_q<S>(m, keep, Z.data(), m, Q.data(), m);
    for (int c = 0; c < keep; ++c)
      for (int i = 0; i < m; ++i) {
        S acc = S(0.0);
        for (int j = 0; j < m; ++j) acc += E.g(i, j) * Q[(size_t)c * m + j];
        HQ[(size_t)c * m + i] = acc;
      }
    const int ldn = keep + p;
    for (int c = 0; c < keep; ++c) {
      for (int i = 0; i < keep; ++i) {
        S acc = S(0.0);
        for (int j = 0; j < m; ++j) acc += cj(Q[(size_t)i * m + j]) * HQ[(size_t)c * m + j];
        Gn[(size_t)c * ldn + i] = acc;
      }
      for (int i = 0; i < p; ++i) {
        S acc = S(0.0);
        for (int j = 0; j < m; ++j) acc += E.g(m + i, j) * Q[(size_t)c * m + j];
        Gn[(size_t)c * ldn + keep + i] = acc;
      }
    }
    HS_HIP(hipMemcpyAsync(E.dQ, Q.data(), sizeof(T) * (size_t)m * keep, hipMemcpyHostToDevice, s));
    launch_eigs_rotate<T>(E.V, ldv, E.V, ldv, E.dQ, m, n, m, keep, s);
    for (int c = 0; c < p; ++c)  // ascending: a destination column never lies behind a source column still to be read
      HS_HIP(hipMemcpyAsync(E.V + (size_t)(keep + c) * ldv, E.V + (size_t)(m + c) * ldv, sizeof(T) * (size_t)n, hipMemcpyDeviceToDevice, s));
    HS_HIP(hipStreamSynchronize(s));
    std::fill(E.G.begin(), E.G.end(), S(0.0));
    for (int c = 0; c < keep; ++c)
      for (int i = 0; i < keep + p; ++i) E.g(i, c) = Gn[(size_t)c * ldn + i];
    m = keep;
    ++restarts;
    clk.lap(EP_RESTART);
  }
  clk.lap(EP_RESTART);
  g_einfo[EI_RESTARTS] = restarts;

  // ---- the Ritz pairs
  std::vector<S> Yo((size_t)m * nout);
  std::vector<double> mu((size_t)2 * nx, 0.0), lamv((size_t)2 * nx, 0.0), nrm((size_t)nx, 0.0);
  std::vector<int> pr((size_t)nx, 0);
  const double sg_im = trans == 2 ? -sigma_im : sigma_im;
  for (int c = 0; c < nout; ++c) {
    ritz_column(m, Y.data(), m, order, pair, c, Yo.data() + (size_t)c * m);
    const zc muc = pair[(size_t)c] < 0 ? std::conj(1.0 / w[(size_t)order[(size_t)c - 1]]) : 1.0 / w[(size_t)order[(size_t)c]];  // a pair: exact conjugates
    pr[(size_t)c] = pair[(size_t)c];
    mu[(size_t)2 * c] = muc.real();
    mu[(size_t)2 * c + 1] = (real_h && pair[(size_t)c] == 0) ? 0.0 : muc.imag();
    lamv[(size_t)2 * c] = sigma_re + mu[(size_t)2 * c];
    lamv[(size_t)2 * c + 1] = sg_im + mu[(size_t)2 * c + 1];
  }
  HS_HIP(hipMemcpyAsync(E.dQ, Yo.data(), sizeof(T) * (size_t)m * nout, hipMemcpyHostToDevice, s));
  HS_HIP(hipMemcpyAsync(dmu, mu.data(), sizeof(double) * 2 * (size_t)nx, hipMemcpyHostToDevice, s));
  HS_HIP(hipMemcpyAsync(dpair, pr.data(), sizeof(int) * (size_t)nx, hipMemcpyHostToDevice, s));
  launch_eigs_rotate<T>(dX, n, E.V, ldv, E.dQ, m, n, m, nout, s);
  if (E.minner) {  // x^H op(M) x = 1
    E.mult_m(dX, n, dMX, nout);
    launch_eigs_coldot<T>(dX, n, dMX, n, dpair, n, nout, E.dpart, E.dnrm, s);
    launch_eigs_sqrt(E.dnrm, nout, s);
  } else {
    launch_eigs_resid<T>(dX, n, nullptr, 0, nullptr, dpair, n, nout, E.dpart, E.dnrm, s);
  }
  launch_eigs_scale<T>(dX, n, E.dnrm, n, nout, s);
  if (has_m) E.mult_m(dX, n, dMX, nout);
  HsGmresRows rows;
  if (const int st = hs_gmres_own_rows(F, trans, s, &rows)) throw st;
  RowsOf<T> A;
  A.ptr = rows.ptr;
  A.idx = rows.idx;
  A.val = (const T*)rows.val;
  A.conj = trans == 2;
  launch_spmm_op<T>(A, dX, n, nullptr, dAX, n, nullptr, 0, nullptr, n, nout, s);
  launch_eigs_resid<T>(dAX, n, has_m ? dMX : dX, n, dmu, dpair, n, nout, E.dpart, E.dnrm, s);
  HS_HIP(hipMemcpyAsync(nrm.data(), E.dnrm, sizeof(double) * (size_t)nout, hipMemcpyDeviceToHost, s));
  HS_HIP(hipEventRecord(*e1, s));
  HS_HIP(hipStreamSynchronize(s));
  HS_HIP(hipGetLastError());
  if (const int st = hs_handle_flow_check(F)) throw st;
  float ms = 0.f;
  HS_HIP(hipEventElapsedTime(&ms, *e0, *e1));
  g_einfo[EI_SECONDS] = ms * 1e-3;
  clk.lap(EP_FINISH);
  // ---- results
  if (X) HS_HIP(hipMemcpy2D(X, ldx * sizeof(T), dX, n * sizeof(T), n * sizeof(T), nout, where ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
  for (int c = 0; c < nx; ++c) {
    lam[2 * c] = c < nout ? lamv[(size_t)2 * c] : 0.0;
    lam[2 * c + 1] = c < nout ? lamv[(size_t)2 * c + 1] : 0.0;
    resid[c] = c < nout ? nrm[(size_t)c] : 0.0;
    est[c] = c < nout ? estv[(size_t)c] : 0.0;
  }
  *nout_ = nout;
  *nconv_ = nconv;
}

template <class T>
int eigs_entry(hs_handle* F, int trans, int64_t n, const HostCsc<T>& M, int inner, int64_t nev, int64_t ncv, int64_t block, double sigma_re, double sigma_im, double tol, int64_t maxrestart, const T* V0,
               int64_t ldv0, int64_t seed, int where, double* lam, T* X, int64_t ldx, double* resid, double* est, int64_t* nout, int64_t* nconv, void* stream) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = HS_OK;
  HsDevBuf buf("GMRES workspace");  // outlives the try block: after a throw the stream is drained below before the workspace is freed
  try {
    eigs_run<T>(F, trans, n, M, inner, nev, ncv, block, sigma_re, sigma_im, tol, maxrestart, V0, ldv0, seed, where, lam, X, ldx, resid, est, nout, nconv, stream, buf, &e0, &e1);
  } catch (int code) {
    rc = code;
  } catch (const std::bad_alloc&) {
    hs_set_error(HS_ERR_NOMEM, 0, "host allocation failed");
    rc = HS_ERR_NOMEM;
  }
  if (rc != HS_OK && e0) (void)hipStreamSynchronize((hipStream_t)stream);  // nothing in flight may outlive the workspace
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  return rc;
}

}  // namespace

extern "C" int hs_eigs_d(hs_handle* F, int trans, int64_t n, int64_t nev, int64_t ncv, int64_t block, double sigma_re, double sigma_im, double tol, int64_t maxrestart,
                         const double* V0, int64_t ldv0, int64_t seed, int where, double* lam, double* X, int64_t ldx, double* resid, double* est, int64_t* nout, int64_t* nconv,
                         void* stream) {
  return eigs_entry<double>(F, trans, n, HostCsc<double>(), 0, nev, ncv, block, sigma_re, sigma_im, tol, maxrestart, V0, ldv0, seed, where, lam, X, ldx, resid, est, nout, nconv,
                            stream);
}
extern "C" int hs_eigs_z(hs_handle* F, int trans, int64_t n, int64_t nev, int64_t ncv, int64_t block, double sigma_re, double sigma_im, double tol, int64_t maxrestart,
                         const double* V0, int64_t ldv0, int64_t seed, int where, double* lam, double* X, int64_t ldx, double* resid, double* est, int64_t* nout, int64_t* nconv,
                         void* stream) {
  return eigs_entry<cplx>(F, trans, n, HostCsc<cplx>(), 0, nev, ncv, block, sigma_re, sigma_im, tol, maxrestart, (const cplx*)V0, ldv0, seed, where, lam, (cplx*)X, ldx, resid, est,
                          nout, nconv, stream);
}
extern "C" int hs_eigs_gen_d(hs_handle* F, int trans, int64_t n, const int64_t* mcolptr, const int64_t* mrowval, const double* mnzval, int inner, int64_t nev, int64_t ncv,
                             int64_t block, double sigma_re, double sigma_im, double tol, int64_t maxrestart, const double* V0, int64_t ldv0, int64_t seed, int where, double* lam,
                             double* X, int64_t ldx, double* resid, double* est, int64_t* nout, int64_t* nconv, void* stream) {
  HostCsc<double> M;
  M.colptr = mcolptr;
  M.rowval = mrowval;
  M.nzval = mnzval;
  return eigs_entry<double>(F, trans, n, M, inner, nev, ncv, block, sigma_re, sigma_im, tol, maxrestart, V0, ldv0, seed, where, lam, X, ldx, resid, est, nout, nconv, stream);
}
extern "C" int hs_eigs_gen_z(hs_handle* F, int trans, int64_t n, const int64_t* mcolptr, const int64_t* mrowval, const double* mnzval, int inner, int64_t nev, int64_t ncv,
                             int64_t block, double sigma_re, double sigma_im, double tol, int64_t maxrestart, const double* V0, int64_t ldv0, int64_t seed, int where, double* lam,
                             double* X, int64_t ldx, double* resid, double* est, int64_t* nout, int64_t* nconv, void* stream) {
  HostCsc<cplx> M;
  M.colptr = mcolptr;
  M.rowval = mrowval;
  M.nzval = (const cplx*)mnzval;
  return eigs_entry<cplx>(F, trans, n, M, inner, nev, ncv, block, sigma_re, sigma_im, tol, maxrestart, (const cplx*)V0, ldv0, seed, where, lam, (cplx*)X, ldx, resid, est, nout,
                          nconv, stream);
}
extern "C" int hs_eigs_gen_info(double* out4) {
  if (!out4) {
    hs_set_error(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_eigs_gen_info: out4 == NULL");
    return HS_ERR_ARGUMENT;
  }
  for (int k = 0; k < 4; ++k) out4[k] = g_ginfo[k];
  return HS_OK;
}
extern "C" int hs_eigs_info(double* out8) {
  if (!out8) {
    hs_set_error(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_eigs_info: out8 == NULL");
    return HS_ERR_ARGUMENT;
  }
  for (int k = 0; k < 8; ++k) out8[k] = g_einfo[k];
  return HS_OK;
}
extern "C" int hsk_eigs_phase_timing(int on) {
  const int was = g_phase_sync ? 1 : 0;
  g_phase_sync = on != 0;
  return was;
}
extern "C" double hsk_eigs_gen_mprod_seconds(void) { return g_mprod_seconds; }
extern "C" int hsk_eigs_phases(double* out4) {
  if (!out4) {
    hs_set_error(HS_ERR_ARGUMENT, 0, "ArgumentError: hsk_eigs_phases: out4 == NULL");
    return HS_ERR_ARGUMENT;
  }
  for (int k = 0; k < 4; ++k) out4[k] = g_ephase[k];
  return HS_OK;
}
