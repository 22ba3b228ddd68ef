// hs_selinv.h -- what hs_selinv.hip (log-determinant, selected inversion) reads from a factorization handle, and the launch API of
// kernels_selinv.hip.  hs_api.hip owns the handle; hs_selinv_view and the two scratch calls are the whole interface between the files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include <limits>
#include <vector>

#include "hs_common.h"

struct hs_handle;
struct hs_hss;

enum {
  HS_SEL_NOLU = 1,     // D = Aii is kept as an HSS matrix (hss_d, mf = 2, 3): there is no pivoted LU to read
  HS_SEL_LOWRANK = 2,  // Lbi / Uib live in low-rank objects (compressed front)
  HS_SEL_SLICE = 4,    // the front is one slice of a split front (hs_options.split)
};

struct HsSelFront {          // one owned front, every pointer a device pointer
  int parent = -1;           // index into HsSelView::fronts, -1: root (or pseudo-root)
  int level = 0, ni = 0, nb = 0;
  int flags = 0;
  const void* LU = nullptr;  // pivoted L\U of Aii (ni x ni, ld ldlu); with a dense front Lbi = Abi U^-1 follows below it (rows ni..m)
  const void* UR = nullptr;  // Uib = L^-1 P Aib (ni x nb, ld ldu); null unless the front is dense
  int ldlu = 0, ldu = 0;
  const void* inv256L = nullptr;  // inverses of the 256 x 256 diagonal blocks (ld 256); the factorization leaves them behind for ldiv!
  const void* inv256U = nullptr;
  const int* rperm = nullptr;
  const int* fidx = nullptr;  // m global ids, front order [int; bnd]
  size_t off_fidx_host = 0;   // the same ids in HsSelView::fidx_host
  // hs_selinv_lr only (hs_selinv never reads them): the LowRank<T> objects of a compressed front that keeps a dense pivoted LU of Aii,
  // Lbi ~= C_L Z_L' (lrL: Cd nb x rL, Z rL x ni) and Uib ~= G Z_R (lrR: Cd ni x rR, Z rR x nb); null: dense front, or a front the call refuses
  const void* lrL = nullptr;
  const void* lrR = nullptr;
  // HS_SEL_NOLU only (hs_logabsdet with hs_ulv_mode 1): D as an eliminated HSS matrix; mfb: the 2 x 2 block form of mf = 3, D = [A11 A12; A21 A22]
  // with hss = A11 and hss2 = S22 (null while the factorization is incomplete)
  const hs_hss* hss = nullptr;
  const hs_hss* hss2 = nullptr;
  int mfb = 0;
};

struct HsSelView {
  int64_t n = 0, nnz = 0;
  int is_complex = 0, factored = 0, device = 0, nranks = 1;
  int ulv_mode = 0;                // hs_ulv_mode
  std::vector<HsSelFront> fronts;  // tree nodes in post-order (children before parents), the pseudo-root last
  const int* fidx_host = nullptr;
  const int64_t* colptr = nullptr;  // A's pattern on the device, 0-based
  const int32_t* rowval = nullptr;
  void* sb = nullptr;               // the Schur scratch when it is idle (not kept, no buffer of another rank inside), else null
  size_t sb_bytes = 0;
  hipStream_t stream = nullptr;
  void** sx = nullptr;              // cache slot of hs_selinv.hip (entry lists of A's pattern, the last call's figures), freed by hs_free through *sx_free
  void (**sx_free)(void*) = nullptr;
};

void hs_selinv_view(hs_handle* h, HsSelView* v);

// ---- kernels_selinv.hip ---------------------------------------------------------------------------------------------------------------
struct LogdetFront {  // input of the log-determinant reduction
  const void* LU;
  const int* rperm;
  int ni, ld;
};
struct LogdetOut {  // per front: sum log|u_kk|, sum arg(u_kk) (Float64: pi per negative entry is NOT used -- `neg` counts them), flags
  double logabs, angle;
  int neg, odd, zero, pad;  // negative diagonal entries (Float64), parity of the row permutation, exactly zero pivots
};
template <class T>
void launch_logdet(const LogdetFront* df, int nfronts, LogdetOut* out, hipStream_t s);
// the same per-node figures for the fronts of a ULV elimination (hs_hss_logabsdet): the nodes of an HSS tree are small and many, so a
// workgroup is one wave-reduced pass; ni = 0 (a node that eliminates nothing) gives the neutral element
template <class T>
void launch_ulv_det(const LogdetFront* df, int nnodes, LogdetOut* out, hipStream_t s);
// the host side of both launches: the per-front results are added in the order they are given, always the same
struct LogdetAcc {
  double la = 0.0, ang = 0.0;
  long long flips = 0;
  bool zero = false;
  void add(const LogdetOut& o) {
    const double twopi = 6.283185307179586476925286766559;
    la += o.logabs;
    ang = std::remainder(ang + std::remainder(o.angle, twopi), twopi);
    flips += o.neg + o.odd;
    zero = zero || o.zero != 0;
  }
  void add(double logabs, double sign_re, double sign_im) {  // a finished factor: (log|d|, d / |d|)
    if (sign_re == 0.0 && sign_im == 0.0) { zero = true; return; }
    LogdetOut o{logabs, 0.0, 0, 0, 0, 0};
    if (sign_im == 0.0) o.neg = sign_re < 0.0 ? 1 : 0;
    else o.angle = std::atan2(sign_im, sign_re);
    add(o);
  }
  void finish(bool is_complex, double* logabs, double* sign_re, double* sign_im) const {
    if (zero) {
      *logabs = -std::numeric_limits<double>::infinity();
      *sign_re = *sign_im = 0.0;
      return;
    }
    *logabs = la;
    if (!is_complex) {
      *sign_re = (flips & 1) ? -1.0 : 1.0;
      *sign_im = 0.0;
    } else {
      const double a = (flips & 1) ? ang + 3.14159265358979323846264338327950288 : ang;
      *sign_re = std::cos(a);
      *sign_im = std::sin(a);
    }
  }
};

template <class T>
struct SelDesc {  // one front of a selected-inversion batch
  T* Z;           // its m x m block of A^-1, front order [int; bnd]
  const T* Zp;    // the parent's finished block (null: no boundary to gather)
  const int* cmap;
  const int* rperm;
  const int* fidx;
  T* Vi;          // ni x ni work block (starts as the identity), ld ldv
  T* Tm;          // m x ni work block (starts as zero), ld ldz
  T* X2;          // m x ni: Z[:, int] before the column permutation, ld ldz
  const int* epr;  // entries of A this front owns: row / column position in the front, index into A's nzval
  const int* epc;
  const int64_t* ee;
  int ecnt;
  int ni, nb, m, ldz, ldzp, ldv;
  // a low-rank front of hs_selinv_lr (rR = rL = 0 and null pointers: dense front).  The stored factors are only read: zload_lr copies G
  // into Vg = Vi + ni ldv and Z_L' into rows nit.. of Tm, the right-hand sides the substitutions overwrite
  int rR, rL;      // ranks of Uib ~= G Z_R and Lbi ~= C_L Z_L'
  int ldg, ldzr, ldcl, ldzl;
  const T* G;      // ni x rR
  const T* ZR;     // rR x nb
  const T* CL;     // nb x rL
  const T* ZL;     // rL x ni (Z_L' = Z_L U^-1)
  int ldt, nit;    // Tm of a low-rank front: (nit + rL) x ni, ld ldt, nit = ni rounded up to even (the tail starts 16-byte aligned)
  int ld1, ld2;    // ld of T1 / T3 (rR rows) and of T2 (nb rows); Wg and WT3 use ldv, Yp uses ldy
  int ldy, pad;
  T* Wg;           // W = U^-1 G (ni x rR)
  T* Yp;           // Y' = Z_L' L^-1 (rL x ni)
  T* T1;           // -Z_R Zbb (rR x nb)
  T* T2;           // -Zbb C_L (nb x rL)
  T* T3;           // T1 C_L (rR x rL)
  T* WT3;          // W T3 (ni x rL)
};
template <class T>
void launch_zinit(const SelDesc<T>* d, int nbatch, int maxni, hipStream_t s);                 // Vi = I
template <class T>
void launch_zload_lr(const SelDesc<T>* d, int nbatch, int maxni, int maxr, hipStream_t s);   // Vg = G, Tm[nit.., :] = Z_L' for the low-rank fronts
template <class T>
void launch_zgather(const SelDesc<T>* d, int nbatch, int maxnb, hipStream_t s);               // Z[bnd, bnd] = Zp[cmap, cmap]
template <class T>
void launch_zpermute_cols(const SelDesc<T>* d, int nbatch, int maxm, int maxni, hipStream_t s);  // Z[:, rperm[i]] = X2[:, i]
template <class T>
void launch_zextract(const SelDesc<T>* d, int nbatch, int maxni, int maxe, int trans, T* diag, T* zval, hipStream_t s);
