// hs_testhooks.hip -- kernel-level entry points used only by tests/ (declared in include/hs_kernels.h).
// They drive exactly the kernels hs_factor_* uses, on caller-supplied dense data, so every kernel
// can be checked against the oracle in isolation.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <chrono>
#include <vector>

#include "../../include/hs_kernels.h"
#include "hs_host.h"
#include "hs_sched.h"
#include "hs_envelope.h"
#include "hs_lowrank.h"
#include "hs_solve_multi.h"
#include "hs_sweep.h"

// Every hook below is a void template that refuses through HS_FAIL / HS_HIP / HS_CHECK, in the order arguments, device, allocation; its
// hsk_* entry points are HS_GUARD(hook<T>(...)).  Device memory belongs to an HsDevBuf, so it is freed on every path.
namespace {
void need_device() {
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) HS_FAIL(HS_ERR_DEVICE, 0, "no HIP device available");
}
size_t rup32(size_t e) { return (e + 31) / 32 * 32; }
// A rows x cols host block (leading dimension ld; null: nothing is copied) goes up with leading dimension max(rows, 1) ...
template <class T>
T* put_block(HsDevBuf& buf, const T* src, int64_t ld, int64_t rows, int64_t cols) {
  const int64_t r = std::max<int64_t>(rows, 1);
  T* d = buf.get<T>((size_t)(r * std::max<int64_t>(cols, 1)));
  if (src && rows > 0 && cols > 0) HS_HIP(hipMemcpy2D(d, r * sizeof(T), src, ld * sizeof(T), rows * sizeof(T), cols, hipMemcpyHostToDevice));
  return d;
}
// ... and a rows x cols device block (leading dimension dld) comes down into dst (leading dimension ld).
template <class T>
void bring_block(T* dst, int64_t ld, const T* d, int64_t dld, int64_t rows, int64_t cols) {
  HS_HIP(hipMemcpy2D(dst, ld * sizeof(T), d, dld * sizeof(T), rows * sizeof(T), cols, hipMemcpyDeviceToHost));
}
// the mean time of `repeat` runs on the null stream (repeat <= 0: none)
template <class Run>
void time_repeats(int repeat, double* ms_out, Run run) {
  if (repeat <= 0) return;
  HsEvents<2> ev;
  HS_HIP(hipEventRecord(ev[0], 0));
  for (int r = 0; r < repeat; ++r) run();
  HS_HIP(hipEventRecord(ev[1], 0));
  HS_HIP(hipEventSynchronize(ev[1]));
  float ms = 0.f;
  HS_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
  if (ms_out) *ms_out = ms / repeat;
}
}  // namespace

template <class T>
static void gemm_hook(int64_t M, int64_t N, int64_t K, const T* A, int64_t lda, const T* B, int64_t ldb, T* C, int64_t ldc, int minus,
                      int repeat, double* ms_out) {
  need_device();
  HsDevBuf buf("hsk_gemm");
  T* dA = (T*)buf.get<char>(sizeof(T) * (size_t)lda * K + 16);
  T* dB = (T*)buf.get<char>(sizeof(T) * (size_t)ldb * N + 16);
  T* dC = (T*)buf.get<char>(sizeof(T) * (size_t)ldc * N + 16);
  GemmProb<T>* dp = buf.get<GemmProb<T>>(1);
  HS_HIP(hipMemcpy(dA, A, sizeof(T) * (size_t)lda * K, hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(dB, B, sizeof(T) * (size_t)ldb * N, hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(dC, C, sizeof(T) * (size_t)ldc * N, hipMemcpyHostToDevice));
  GemmProb<T> p{dA, dB, dC, (int)M, (int)N, (int)K, (int)lda, (int)ldb, (int)ldc};
  HS_HIP(hipMemcpy(dp, &p, sizeof p, hipMemcpyHostToDevice));
  launch_gemm_probs<T>(dp, 1, (int)M, (int)N, minus, 0);
  HS_HIP(hipDeviceSynchronize());
  HS_HIP(hipMemcpy(C, dC, sizeof(T) * (size_t)ldc * N, hipMemcpyDeviceToHost));
  time_repeats(repeat, ms_out, [&] { launch_gemm_probs<T>(dp, 1, (int)M, (int)N, minus, 0); });
}

extern "C" int hsk_gemm_d(int64_t M, int64_t N, int64_t K, const double* A, int64_t lda, const double* B, int64_t ldb, double* C,
                          int64_t ldc, int minus, int repeat, double* ms_out) {
  HS_GUARD(gemm_hook<double>(M, N, K, A, lda, B, ldb, C, ldc, minus, repeat, ms_out));
}
extern "C" int hsk_gemm_z(int64_t M, int64_t N, int64_t K, const double* A, int64_t lda, const double* B, int64_t ldb, double* C,
                          int64_t ldc, int minus, int repeat, double* ms_out) {
  HS_GUARD(gemm_hook<cplx>(M, N, K, (const cplx*)A, lda, (const cplx*)B, ldb, (cplx*)C, ldc, minus, repeat, ms_out));
}

// The plain update of a level, C -= A * B for a batch of `count` fronts, the way Sched::gemm issues the U12 update UR[r0.., :] -= LF[r0.., k0:k1) *
// UR[k0:k1, :]: front f has K + M[f] (+ koff + roff) interior and N[f] boundary DOFs, A sits in LF at row r0 = koff + K + roff and column
// k0 = koff, B in the rows k0.. of UR and C in its rows r0...  The schedule decides per launch between gemm_op_kernel and gemm_op_lds_kernel
// exactly as in a factorization (hs_gemm_lds_route, HS_GEMM_LDS / hsk_gemm_lds_enable); *routed says how many launches took the latter (the
// launches of the edge kernels have a counter of their own, hsk_gemm_lds_edge_launches).
// koff / roff = 1 shift B / A by one double (an operand the direct load may not take).
static void gemm_op_hook(int64_t count, const int64_t* M, const int64_t* N, int64_t K, int64_t koff, int64_t roff, const double* A, const double* B,
                         double* C, int64_t* routed, int repeat, double* ms_out) {
  typedef double T;
  if (count <= 0 || count > 65535 || !M || !N || !A || !B || !C || K <= 0 || koff < 0 || roff < 0)
    HS_FAIL(HS_ERR_ARGUMENT, count, "hsk_gemm_op_d: count in [1, 65535], positive K, non-negative offsets and non-null arrays required");
  for (int64_t f = 0; f < count; ++f)
    if (M[f] <= 0 || N[f] <= 0 || koff + K + roff + M[f] > (1 << 20) || N[f] > (1 << 20))
      HS_FAIL(HS_ERR_ARGUMENT, f, "hsk_gemm_op_d: front %lld has M = %lld, N = %lld", (long long)f, (long long)M[f], (long long)N[f]);
  need_device();
  const int k0 = (int)koff, k1 = (int)(koff + K), r0 = (int)(koff + K + roff);
  std::vector<NodeDesc<T>> hn(count);
  std::vector<int> h_ni(count), h_nb(count);
  std::vector<size_t> olf(count), our(count);
  size_t nT = 0;
  int maxni = 0, maxnb = 0;
  for (int64_t f = 0; f < count; ++f) {
    const int ni = r0 + (int)M[f], nb = (int)N[f], ld = (ni + 1) / 2 * 2;
    h_ni[f] = ni; h_nb[f] = nb;
    maxni = std::max(maxni, ni); maxnb = std::max(maxnb, nb);
    olf[f] = nT; nT += rup32((size_t)ld * k1);  // only the columns [0, k1) of LF are read
    our[f] = nT; nT += rup32((size_t)ld * nb);
  }
  HsDevBuf buf("hsk_gemm_op_d");
  T* dbuf = buf.get<T>(nT);
  NodeDesc<T>* dn = buf.get<NodeDesc<T>>((size_t)count);
  HS_HIP(hipMemset(dbuf, 0, sizeof(T) * nT));
  bool aligned = true;
  const T *Af = A, *Bf = B;
  T* Cf = C;
  for (int64_t f = 0; f < count; ++f) {
    NodeDesc<T>& d = hn[f];
    memset(&d, 0, sizeof d);
    d.ni = h_ni[f]; d.nb = h_nb[f]; d.m = d.ni + d.nb;
    d.ldl = d.ldu = (d.ni + 1) / 2 * 2;
    d.lds = (d.nb + 1) / 2 * 2;
    d.LF = dbuf + olf[f]; d.UR = dbuf + our[f];
    d.SB = nullptr;  // (never addressed: C and B are UR)
    d.ni1 = d.ni; d.nb1 = d.nb; d.node = (int)f;
    d.finalize();
    d.mrows[HS_MAT_SB] = d.mcols[HS_MAT_SB] = 0;
    aligned = aligned && !((((uintptr_t)d.LF | (uintptr_t)d.UR) & 15) || ((d.ldl | d.ldu) & 1));
    const int Mf = (int)M[f];
    HS_HIP(hipMemcpy2D(d.LF + r0 + (size_t)k0 * d.ldl, sizeof(T) * d.ldl, Af, sizeof(T) * Mf, sizeof(T) * Mf, K, hipMemcpyHostToDevice));
    HS_HIP(hipMemcpy2D(d.UR + k0, sizeof(T) * d.ldu, Bf, sizeof(T) * K, sizeof(T) * K, d.nb, hipMemcpyHostToDevice));
    HS_HIP(hipMemcpy2D(d.UR + r0, sizeof(T) * d.ldu, Cf, sizeof(T) * Mf, sizeof(T) * Mf, d.nb, hipMemcpyHostToDevice));
    Af += (size_t)Mf * K; Bf += (size_t)K * d.nb; Cf += (size_t)Mf * d.nb;
  }
  HS_HIP(hipMemcpy(dn, hn.data(), sizeof(NodeDesc<T>) * count, hipMemcpyHostToDevice));
  Profiler prof;
  Sched<T> sch{dn, (int)count, maxni, maxnb, maxni + maxnb, (hipStream_t) nullptr, &prof, h_ni.data(), h_nb.data()};
  sch.aligned16 = aligned;
  const long long before = hsk_gemm_lds_launches(0);
  sch.gemm(HS_MAT_UR, HS_MAT_UR, r0, HS_BIG, 0, HS_BIG, k0, k1);
  HS_HIP(hipDeviceSynchronize());
  if (routed) *routed = (int64_t)(hsk_gemm_lds_launches(0) - before);
  Cf = C;
  for (int64_t f = 0; f < count; ++f) {
    const NodeDesc<T>& d = hn[f];
    const int Mf = (int)M[f];
    bring_block(Cf, Mf, d.UR + r0, d.ldu, Mf, d.nb);
    Cf += (size_t)Mf * d.nb;
  }
  time_repeats(repeat, ms_out, [&] { sch.gemm(HS_MAT_UR, HS_MAT_UR, r0, HS_BIG, 0, HS_BIG, k0, k1); });
  prof.collect();
}
extern "C" int hsk_gemm_op_d(int64_t count, const int64_t* M, const int64_t* N, int64_t K, int64_t koff, int64_t roff, const double* A,
                             const double* B, double* C, int64_t* routed, int repeat, double* ms_out) {
  HS_GUARD(gemm_op_hook(count, M, N, K, koff, roff, A, B, C, routed, repeat, ms_out));
}

// The Schur update of a level, SB -= LF[ni.., 0:ni) * UR, for a batch of `count` fronts with their own ni[f] and nb[f] -- what hsk_gemm_op_d
// cannot pose: there every front has the same K and the same row offset, here K = ni[f] and A's row offset is ni[f].  LF, UR and SB are laid
// out as hs_analyze lays them out (even leading dimensions, every matrix at a multiple of 32 elements) and the launch is
// Sched::gemm(HS_MAT_SB, HS_MAT_UR, 0, HS_BIG, 0, HS_BIG, 0, HS_BIG).  A (nb x ni), B (ni x nb) and C (nb x nb, overwritten) are packed
// column-major, front after front; everything else of the fronts -- the interior rows of LF, the padding rows, the gaps -- holds a finite
// non-zero value, so a load that should have been a zero fill shows in the result.  A == B == C == null: no host data, the operands hold
// that value too (timing only).  env != 0: the launch is enveloped and every front carries the block envelope of the zeros its A and B
// really have (firstL of a 32-row block of A: the first column, rounded down to 32, with a non-zero entry in one of its rows; firstU of
// a 32-column block of B likewise by rows; the interior blocks, which this product does not address, get their diagonal).
static void gemm_schur_hook(int64_t count, const int64_t* ni_, const int64_t* nb_, const double* A, const double* B, double* C, int env,
                            int64_t* routed_lds, int64_t* routed_edge, int repeat, double* ms_out) {
  typedef double T;
  const bool data = A && B && C;
  if (count <= 0 || count > 65535 || !ni_ || !nb_ || (!data && (A || B || C)) || (env && !data))
    HS_FAIL(HS_ERR_ARGUMENT, count, "hsk_gemm_schur_d: count in [1, 65535], ni and nb non-null, A, B, C all given or all null (env needs them) required");
  for (int64_t f = 0; f < count; ++f)
    if (ni_[f] <= 0 || nb_[f] <= 0 || ni_[f] + nb_[f] > (1 << 20))
      HS_FAIL(HS_ERR_ARGUMENT, f, "hsk_gemm_schur_d: front %lld has ni = %lld, nb = %lld", (long long)f, (long long)ni_[f], (long long)nb_[f]);
  need_device();
  auto even = [](int v) { return (v + 1) / 2 * 2; };
  std::vector<NodeDesc<T>> hn(count);
  std::vector<int> h_ni(count), h_nb(count);
  std::vector<size_t> olf(count), our(count), osb(count), oenv(count);
  size_t nT = 0, nE = 0;
  int maxni = 0, maxnb = 0, maxm = 0;
  for (int64_t f = 0; f < count; ++f) {
    const int ni = (int)ni_[f], nb = (int)nb_[f];
    h_ni[f] = ni; h_nb[f] = nb;
    maxni = std::max(maxni, ni); maxnb = std::max(maxnb, nb); maxm = std::max(maxm, ni + nb);
    olf[f] = nT; nT += rup32((size_t)even(ni + nb) * ni);
    our[f] = nT; nT += rup32((size_t)even(ni) * nb);
    osb[f] = nT; nT += rup32((size_t)even(nb) * nb);
    oenv[f] = nE; nE += 2 * (size_t)hs_env_nblocks(ni, nb);
  }
  HsDevBuf buf("hsk_gemm_schur_d");
  T* dbuf = buf.get<T>(nT);
  NodeDesc<T>* dn = buf.get<NodeDesc<T>>((size_t)count);
  HS_HIP(hipMemsetD32(dbuf, 0x3F800000, 2 * nT));  // every double 0x3F8000003F800000 = 0.0078125...: finite, non-zero
  std::vector<int> henv(env ? nE : 0);
  std::vector<const int*> h_envp(count, nullptr);
  int* denv = env ? buf.get<int>(nE) : nullptr;
  bool aligned = true;
  const T *Af = A, *Bf = B;
  T* Cf = C;
  for (int64_t f = 0; f < count; ++f) {
    NodeDesc<T>& d = hn[f];
    memset(&d, 0, sizeof d);
    d.ni = h_ni[f]; d.nb = h_nb[f]; d.m = d.ni + d.nb;
    d.ldl = even(d.m); d.ldu = even(d.ni); d.lds = even(d.nb);
    d.LF = dbuf + olf[f]; d.UR = dbuf + our[f]; d.SB = dbuf + osb[f];
    d.ni1 = d.ni; d.nb1 = d.nb; d.node = (int)f;
    const int ni = d.ni, nb = d.nb;
    if (env) {
      const int nI = (ni + 31) / 32, nblk = hs_env_nblocks(ni, nb);
      int* fL = henv.data() + oenv[f];
      int* fU = fL + nblk;
      for (int b = 0; b < nblk; ++b) fL[b] = fU[b] = b < nI ? 32 * b : HS_ENV_NONE;
      for (int k = 0; k < ni; ++k)
        for (int r = 0; r < nb; ++r)
          if (Af[(size_t)r + (size_t)k * nb] != 0.0) { int& v = fL[nI + r / 32]; v = std::min(v, k & ~31); }
      for (int c = 0; c < nb; ++c)
        for (int k = 0; k < ni; ++k)
          if (Bf[(size_t)k + (size_t)c * ni] != 0.0) { int& v = fU[nI + c / 32]; v = std::min(v, k & ~31); break; }
      d.env = denv + oenv[f];
      h_envp[f] = fL;
    }
    d.finalize();
    aligned = aligned && !((((uintptr_t)d.LF | (uintptr_t)d.UR | (uintptr_t)d.SB) & 15) || ((d.ldl | d.ldu | d.lds) & 1));
    if (data) {
      HS_HIP(hipMemcpy2D(d.LF + ni, sizeof(T) * d.ldl, Af, sizeof(T) * nb, sizeof(T) * nb, ni, hipMemcpyHostToDevice));
      HS_HIP(hipMemcpy2D(d.UR, sizeof(T) * d.ldu, Bf, sizeof(T) * ni, sizeof(T) * ni, nb, hipMemcpyHostToDevice));
      HS_HIP(hipMemcpy2D(d.SB, sizeof(T) * d.lds, Cf, sizeof(T) * nb, sizeof(T) * nb, nb, hipMemcpyHostToDevice));
      Af += (size_t)nb * ni; Bf += (size_t)ni * nb; Cf += (size_t)nb * nb;
    }
  }
  if (env) HS_HIP(hipMemcpy(denv, henv.data(), sizeof(int) * nE, hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(dn, hn.data(), sizeof(NodeDesc<T>) * count, hipMemcpyHostToDevice));
  Profiler prof;
  Sched<T> sch{dn, (int)count, maxni, maxnb, maxm, (hipStream_t) nullptr, &prof, h_ni.data(), h_nb.data()};
  sch.aligned16 = aligned;
  if (env) {
    sch.optimistic = true;
    sch.env = true;
    sch.h_env = h_envp.data();
    sch.perm_cap = (size_t)count * hs_env_perm_stride(hs_env_perm_slot(maxm));
    sch.perm = buf.get<uint16_t>(sch.perm_cap);
  }
  const long long lds0 = hsk_gemm_lds_launches(0), edge0 = hsk_gemm_lds_edge_launches(0);
  sch.gemm(HS_MAT_SB, HS_MAT_UR, 0, HS_BIG, 0, HS_BIG, 0, HS_BIG);
  HS_HIP(hipDeviceSynchronize());
  if (routed_lds) *routed_lds = (int64_t)(hsk_gemm_lds_launches(0) - lds0);
  if (routed_edge) *routed_edge = (int64_t)(hsk_gemm_lds_edge_launches(0) - edge0);
  if (data) {
    Cf = C;
    for (int64_t f = 0; f < count; ++f) {
      const NodeDesc<T>& d = hn[f];
      bring_block(Cf, d.nb, d.SB, d.lds, d.nb, d.nb);
      Cf += (size_t)d.nb * d.nb;
    }
  }
  time_repeats(repeat, ms_out, [&] { sch.gemm(HS_MAT_SB, HS_MAT_UR, 0, HS_BIG, 0, HS_BIG, 0, HS_BIG); });
  prof.collect();
}
extern "C" int hsk_gemm_schur_d(int64_t count, const int64_t* ni, const int64_t* nb, const double* A, const double* B, double* C, int env,
                                int64_t* routed_lds, int64_t* routed_edge, int repeat, double* ms_out) {
  HS_GUARD(gemm_schur_hook(count, ni, nb, A, B, C, env, routed_lds, routed_edge, repeat, ms_out));
}

// The 256-row TRSM base case of a level, UR[r0 : r0 + wl, c0 : c1) <- inv256L[r0 / 256] * UR, for a batch of `count` fronts with their own
// ni[f] and nb[f], issued as a factorization issues it: Sched::trsm_rec(HS_MAT_UR, r0, r0 + 256, c0, c1) with the descriptors' inverses
// valid -- ONE launch of trsm_strip_kernel while the strip kernel is on, the two half products (GemmOp::ainv 3, 4) otherwise.  X holds the
// whole ni[f] x nb[f] matrix UR of every front (column-major, leading dimension ni[f], front after front; overwritten with what the device
// holds afterwards, so the caller sees everything outside the block too), inv one 256 x 256 block per front (the one the launch reads).
// On the device UR has the leading dimension ni[f] + ldpad and starts `shift` doubles past a 16-byte boundary (ldpad making it odd,
// shift = 1: operands the 16-byte loads meet unaligned).  env != 0: an enveloped launch, every front with the firstU of the zeros X really
// has.  *strips (may be null): launches that took the strip kernel.
static void trsm_inv_hook(int64_t count, const int64_t* ni_, const int64_t* nb_, int64_t r0, int64_t c0, int64_t c1, int64_t ldpad, int64_t shift,
                          const double* inv, double* X, int env, int64_t* strips) {
  typedef double T;
  if (count <= 0 || count > 65535 || !ni_ || !nb_ || !inv || !X || r0 < 0 || (r0 & 255) || c0 < 0 || c1 <= c0 || ldpad < 0 || shift < 0 || shift > 1)
    HS_FAIL(HS_ERR_ARGUMENT, count, "hsk_trsm_inv_d: count in [1, 65535], r0 a multiple of 256, 0 <= c0 < c1, ldpad >= 0, shift 0 or 1 and non-null arrays required");
  for (int64_t f = 0; f < count; ++f)
    if (ni_[f] <= 0 || nb_[f] <= 0 || ni_[f] + nb_[f] > (1 << 20))
      HS_FAIL(HS_ERR_ARGUMENT, f, "hsk_trsm_inv_d: front %lld has ni = %lld, nb = %lld", (long long)f, (long long)ni_[f], (long long)nb_[f]);
  need_device();
  std::vector<NodeDesc<T>> hn(count);
  std::vector<SolveNode<T>> hs(count);
  std::vector<int> h_ni(count), h_nb(count);
  std::vector<size_t> our(count), oenv(count);
  size_t nT = 0, nE = 0;
  int maxni = 0, maxnb = 0, maxm = 0;
  const size_t nblk = (size_t)(r0 / 256) + 1;
  for (int64_t f = 0; f < count; ++f) {
    const int ni = (int)ni_[f], nb = (int)nb_[f];
    h_ni[f] = ni; h_nb[f] = nb;
    maxni = std::max(maxni, ni); maxnb = std::max(maxnb, nb); maxm = std::max(maxm, ni + nb);
    our[f] = nT + (size_t)shift; nT += rup32((size_t)(ni + ldpad) * nb + 2);
    oenv[f] = nE; nE += 2 * (size_t)hs_env_nblocks(ni, nb);
  }
  HsDevBuf buf("hsk_trsm_inv_d");
  T* dbuf = buf.get<T>(nT);
  T* dinv = buf.get<T>((size_t)count * nblk * 65536);
  NodeDesc<T>* dn = buf.get<NodeDesc<T>>((size_t)count);
  SolveNode<T>* dsn = buf.get<SolveNode<T>>((size_t)count);
  HS_HIP(hipMemsetD32(dbuf, 0x3F800000, 2 * nT));  // the padding rows and the gaps: finite, non-zero
  HS_HIP(hipMemsetD32(dinv, 0x3F800000, 2 * (size_t)count * nblk * 65536));
  std::vector<int> henv(env ? nE : 0);
  std::vector<const int*> h_envp(count, nullptr);
  int* denv = env ? buf.get<int>(nE) : nullptr;
  const T* Xf = X;
  for (int64_t f = 0; f < count; ++f) {
    NodeDesc<T>& d = hn[f];
    memset(&d, 0, sizeof d);
    memset(&hs[f], 0, sizeof hs[f]);
    const int ni = h_ni[f], nb = h_nb[f];
    d.ni = ni; d.nb = nb; d.m = ni + nb;
    d.ldl = d.m; d.ldu = ni + (int)ldpad; d.lds = nb;
    d.UR = dbuf + our[f];  // (LF and SB are never addressed)
    d.inv256L = dinv + (size_t)f * nblk * 65536;
    d.ni1 = ni; d.nb1 = nb; d.node = (int)f;
    if (env) {
      const int nI = (ni + 31) / 32, nb_all = hs_env_nblocks(ni, nb);
      int* fL = henv.data() + oenv[f];
      int* fU = fL + nb_all;
      for (int b = 0; b < nb_all; ++b) fL[b] = fU[b] = b < nI ? 32 * b : HS_ENV_NONE;
      for (int c = 0; c < nb; ++c)
        for (int k = 0; k < ni; ++k)
          if (Xf[(size_t)k + (size_t)c * ni] != 0.0) { int& v = fU[nI + c / 32]; v = std::min(v, k & ~31); break; }
      d.env = denv + oenv[f];
      h_envp[f] = fL;
    }
    d.finalize();
    d.mrows[HS_MAT_LF] = d.mcols[HS_MAT_LF] = d.mrows[HS_MAT_SB] = d.mcols[HS_MAT_SB] = 0;
    HS_HIP(hipMemcpy2D(d.UR, sizeof(T) * d.ldu, Xf, sizeof(T) * ni, sizeof(T) * ni, nb, hipMemcpyHostToDevice));
    HS_HIP(hipMemcpy(d.inv256L + (nblk - 1) * 65536, inv + (size_t)f * 65536, sizeof(T) * 65536, hipMemcpyHostToDevice));
    Xf += (size_t)ni * nb;
  }
  if (env) HS_HIP(hipMemcpy(denv, henv.data(), sizeof(int) * nE, hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(dn, hn.data(), sizeof(NodeDesc<T>) * count, hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(dsn, hs.data(), sizeof(SolveNode<T>) * count, hipMemcpyHostToDevice));
  Profiler prof;
  Sched<T> sch{dn, (int)count, maxni, maxnb, maxm, (hipStream_t) nullptr, &prof, h_ni.data(), h_nb.data()};
  sch.sn = dsn;  // (never read by the solve: it only says that the descriptors carry inv256L)
  sch.wide = true;
  if (env) {
    sch.optimistic = true;
    sch.env = true;
    sch.h_env = h_envp.data();
  }
  const long long before = hsk_trsm_strip_launches(0);
  sch.trsm_rec(HS_MAT_UR, (int)r0, (int)r0 + 256, (int)c0, (int)std::min<int64_t>(c1, HS_BIG));
  HS_HIP(hipDeviceSynchronize());
  if (strips) *strips = (int64_t)(hsk_trsm_strip_launches(0) - before);
  T* Xo = X;
  for (int64_t f = 0; f < count; ++f) {
    const NodeDesc<T>& d = hn[f];
    bring_block(Xo, d.ni, d.UR, d.ldu, d.ni, d.nb);
    Xo += (size_t)d.ni * d.nb;
  }
  prof.collect();
}
extern "C" int hsk_trsm_inv_d(int64_t count, const int64_t* ni, const int64_t* nb, int64_t r0, int64_t c0, int64_t c1, int64_t ldpad, int64_t shift,
                              const double* inv, double* X, int env, int64_t* strips) {
  HS_GUARD(trsm_inv_hook(count, ni, nb, r0, c0, c1, ldpad, shift, inv, X, env, strips));
}

// Factor a batch of `count` dense fronts F[k] ((ni[k]+nb[k])^2, column-major, front order [int;bnd], packed one after another) the way
// hs_numeric factors a level: one Sched over the batch (batch maxima, per-front sizes on the host, the look-ahead streams).
//   mode 0: tournament pivoting, no solve descriptors   1: optimistic, no descriptors (32-row TRSM base case, full-height panels)
//        2: optimistic WITH descriptors -- the production default: diagonal-block-first 256-column groups, inv256, ainv 3..8 / 16..19
//        3: tournament with descriptors -- what a redone level runs
//   + 4 (bit 2): the batch runs with Sched::aligned16 = true, as hs_numeric sets it for the dense batch of a level: Float64 plain updates take
//        gemm_op_lds_kernel or the edge kernels where hs_gemm_lds_route lets them (ComplexF64 accepts the bit; the route needs sizeof(T) == 8)
// Outputs (any may be null) are packed per front in the same order: LF m x ni, UR ni x nb, SB nb x nb, rperm ni, info, growth;
// invL / invU ceil(ni/32) blocks of 32 x 32, inv256L / inv256U ceil(ni/256) blocks of 256 x 256 (column-major; modes 2, 3 only).
// The batch itself -- device buffers, descriptors, copy-in, factorization, copy-out -- is FrontBatch, shared with hsk_sweep_level_* below.
template <class T>
struct FrontBatch {
  // per-front layout of one device buffer of T and one of int, laid out as hs_analyze lays out the factor arenas
  struct Off {
    int ni, nb, m, ldl, ldu, lds, nblk, nb256, ncand;
    size_t lf, ur, sb, inv, inv256, ip, cand;
  };
  int64_t count = 0;
  std::vector<Off> o;
  std::vector<int> h_ni, h_nb;
  int maxni = 0, maxnb = 0, maxm = 0;
  HsDevBuf buf{"front batch"};  // owns the four device blocks below
  T* dbuf = nullptr;
  int* dint = nullptr;
  NodeDesc<T>* dn = nullptr;
  SolveNode<T>* dsn = nullptr;
  std::vector<NodeDesc<T>> hn;
  std::vector<SolveNode<T>> hs;  // filled by setup, reaches the device with upload_solve (a caller may complete it in between)
  std::vector<int> env_host;     // caller-made block envelopes (set_env): firstL then firstU of every front, packed in batch order
  std::vector<const int*> h_env; // ... one pointer per front, for Sched::h_env; empty: the batch is dense
  // the argument checks both hooks share; nothing on the device yet
  static void check(const char* name, int64_t count, const int64_t* ni_, const int64_t* nb_, const T* F, int mode, int mode_lo, int mode_hi = 3) {
    if (count <= 0 || count > 65535 || !ni_ || !nb_ || !F || mode < mode_lo || mode > mode_hi)
      HS_FAIL(HS_ERR_ARGUMENT, count, "%s: count in [1, 65535], ni, nb and F non-null and mode in %d..%d required", name, mode_lo, mode_hi);
    for (int64_t k = 0; k < count; ++k)
      if (ni_[k] < 0 || nb_[k] < 0 || ni_[k] + nb_[k] > (1 << 16))
        HS_FAIL(HS_ERR_ARGUMENT, k, "%s: front %lld has ni = %lld, nb = %lld (need 0 <= ni, nb and ni + nb <= 65536)", name, (long long)k,
                (long long)ni_[k], (long long)nb_[k]);
  }
  void setup(int64_t count_, const int64_t* ni_, const int64_t* nb_, const T* F);
  void upload_solve() { HS_HIP(hipMemcpy(dsn, hs.data(), sizeof(SolveNode<T>) * count, hipMemcpyHostToDevice)); }
  void set_env(const int32_t* env);
  int aligned16_status() const;
  void factor(int mode, double* ms_out, bool sym = false);
  void copy_out(T* outLF, T* outUR, T* outSB, int64_t* out_rperm, int64_t* info, int64_t* growth, T* outInvL, T* outInvU, T* outInv256L, T* outInv256U);
};

template <class T>
void FrontBatch<T>::setup(int64_t count_, const int64_t* ni_, const int64_t* nb_, const T* F) {
  count = count_;
  need_device();
  o.resize(count);
  h_ni.resize(count);
  h_nb.resize(count);
  size_t nT = 0, nI = 0;
  for (int64_t k = 0; k < count; ++k) {
    Off& x = o[k];
    x.ni = (int)ni_[k]; x.nb = (int)nb_[k]; x.m = x.ni + x.nb;
    x.ldl = std::max((x.m + 1) / 2 * 2, 2); x.ldu = std::max((x.ni + 1) / 2 * 2, 2); x.lds = std::max((x.nb + 1) / 2 * 2, 2);
    x.nblk = (x.ni + HS_PB - 1) / HS_PB;
    x.nb256 = (x.ni + 255) / 256;
    x.ncand = ((x.ni + HS_CHUNK - 1) / HS_CHUNK + 1) * HS_PB;
    x.lf = nT; nT += rup32((size_t)x.ldl * x.ni) + 32;
    x.ur = nT; nT += rup32((size_t)x.ldu * x.nb) + 32;
    x.sb = nT; nT += rup32((size_t)x.lds * x.nb) + 32;
    x.inv = nT; nT += (size_t)2 * x.nblk * HS_PB * HS_PB + 32;
    x.inv256 = nT; nT += (size_t)2 * x.nb256 * 65536 + 32;
    x.ip = nI; nI += (size_t)2 * x.ni + 2;  // ipiv, rperm, info, growth
    x.cand = nI; nI += (size_t)2 * x.ncand + HS_PB + 32;
    h_ni[k] = x.ni; h_nb[k] = x.nb;
    maxni = std::max(maxni, x.ni); maxnb = std::max(maxnb, x.nb); maxm = std::max(maxm, x.m);
  }
  dbuf = buf.get<T>(nT);
  dint = buf.get<int>(nI);
  dn = buf.get<NodeDesc<T>>((size_t)count);
  dsn = buf.get<SolveNode<T>>((size_t)count);
  HS_HIP(hipMemset(dbuf, 0, sizeof(T) * nT));
  HS_HIP(hipMemset(dint, 0, sizeof(int) * nI));
  hn.resize(count);
  hs.resize(count);
  const T* Fk = F;
  for (int64_t k = 0; k < count; ++k) {
    const Off& x = o[k];
    NodeDesc<T>& d = hn[k];
    memset(&d, 0, sizeof d);
    d.LF = dbuf + x.lf; d.UR = dbuf + x.ur; d.SB = dbuf + x.sb;
    d.invL = dbuf + x.inv;
    d.invU = d.invL + (size_t)x.nblk * HS_PB * HS_PB;
    d.inv256L = dbuf + x.inv256;
    d.inv256U = d.inv256L + (size_t)x.nb256 * 65536;
    d.ipiv = dint + x.ip;
    d.rperm = d.ipiv + x.ni;
    d.info = d.rperm + x.ni;
    d.growth = d.info + 1;
    d.cand0 = dint + x.cand;
    d.cand1 = d.cand0 + x.ncand;
    d.pivlist = d.cand1 + x.ncand;
    d.ni = x.ni; d.nb = x.nb; d.m = x.m;
    d.ldl = x.ldl; d.ldu = x.ldu; d.lds = x.lds;
    d.ni1 = x.ni; d.nb1 = x.nb; d.isleaf = 1; d.node = (int)k;
    d.pivrows = x.ni;
    d.finalize();
    SolveNode<T>& q = hs[k];
    memset(&q, 0, sizeof q);
    q.LF = d.LF; q.UR = d.UR; q.invL = d.invL; q.invU = d.invU;
    q.inv256L = d.inv256L; q.inv256U = d.inv256U;
    q.rperm = d.rperm;
    q.ni = x.ni; q.nb = x.nb; q.m = x.m; q.ldl = x.ldl; q.ldu = x.ldu;
    q.mrows = x.m;
    const int m = x.m;
    if (x.ni > 0) HS_HIP(hipMemcpy2D(d.LF, sizeof(T) * x.ldl, Fk, sizeof(T) * m, sizeof(T) * m, x.ni, hipMemcpyHostToDevice));
    if (x.ni > 0 && x.nb > 0) HS_HIP(hipMemcpy2D(d.UR, sizeof(T) * x.ldu, Fk + (size_t)m * x.ni, sizeof(T) * m, sizeof(T) * x.ni, x.nb, hipMemcpyHostToDevice));
    if (x.nb > 0) HS_HIP(hipMemcpy2D(d.SB, sizeof(T) * x.lds, Fk + (size_t)m * x.ni + x.ni, sizeof(T) * m, sizeof(T) * x.nb, x.nb, hipMemcpyHostToDevice));
    Fk += (size_t)m * m;
  }
  HS_HIP(hipMemcpy(dn, hn.data(), sizeof(NodeDesc<T>) * count, hipMemcpyHostToDevice));
}

// Block envelopes made by the caller (hs_envelope.h: 2 * hs_env_nblocks(ni, nb) entries per front, firstL then firstU, packed in batch order):
// every front gets its table, and the optimistic modes then run the batch as hs_numeric runs a level whose fronts carry tables (Sched::env).
template <class T>
void FrontBatch<T>::set_env(const int32_t* env) {
  size_t nE = 0;
  for (int64_t k = 0; k < count; ++k) nE += 2 * (size_t)hs_env_nblocks(o[k].ni, o[k].nb);
  env_host.assign(env, env + nE);
  int* denv = buf.get<int>(nE);
  HS_HIP(hipMemcpy(denv, env_host.data(), sizeof(int) * nE, hipMemcpyHostToDevice));
  h_env.resize(count);
  size_t off = 0;
  for (int64_t k = 0; k < count; ++k) {
    hn[k].env = denv + off;
    h_env[k] = env_host.data() + off;
    off += 2 * (size_t)hs_env_nblocks(o[k].ni, o[k].nb);
  }
  HS_HIP(hipMemcpy(dn, hn.data(), sizeof(NodeDesc<T>) * count, hipMemcpyHostToDevice));
}

// The premise of Sched::aligned16, which hs_numeric sets for the dense batch of a level: setup lays LF / UR / SB of every front out at multiples
// of 32 elements of a hipMalloc block (so 16-byte aligned) with even ldl / ldu / lds.  HS_OK when that holds for the whole batch.
template <class T>
int FrontBatch<T>::aligned16_status() const {
  for (int64_t k = 0; k < count; ++k) {
    const NodeDesc<T>& d = hn[k];
    if ((((uintptr_t)d.LF | (uintptr_t)d.UR | (uintptr_t)d.SB) & 15) || ((d.ldl | d.ldu | d.lds) & 1)) {
      hs_set_error(HS_ERR_UNSUPPORTED, k, "front batch: LF / UR / SB of front %lld are not 16-byte aligned with even leading dimensions", (long long)k);
      return HS_ERR_UNSUPPORTED;
    }
  }
  return HS_OK;
}

// mode & 3: the pivoting and the descriptors (hsk_front_batch_*); mode & 4: Sched::aligned16, the routing of the plain updates hs_numeric runs with
template <class T>
void FrontBatch<T>::factor(int mode, double* ms_out, bool sym) {
  const bool aligned = (mode & 4) != 0;
  mode &= 3;
  if (aligned) HS_CHECK(aligned16_status());
  Profiler prof;
  // same stream set-up as hs_analyze: a main stream and a high-priority side stream for look-ahead panels
  struct Streams {
    hipStream_t main = nullptr, side = nullptr, la = nullptr, sidem = nullptr;
    ~Streams() {
      for (hipStream_t s : {main, side, la, sidem})
        if (s) (void)hipStreamDestroy(s);
    }
  } st;
  HsEvents<2> ev;
  HS_HIP(hipStreamCreate(&st.main));
  hs_create_lookahead_streams(&st.la, &st.sidem, &st.side);
  HS_HIP(hipEventRecord(ev[0], st.main));
  launch_init_fronts<T>(dn, (int)count, maxni, st.main);
  Sched<T> sch{dn, (int)count, maxni, maxnb, maxm, st.main, &prof, h_ni.data(), h_nb.data(), st.side, 0, st.la, st.sidem};
  if (mode >= 2) sch.sn = dsn;
  sch.optimistic = (mode == 1 || mode == 2);
  sch.aligned16 = aligned;
  sch.sym = sym && sch.optimistic;  // (hsk_front_batch_sym_*: the caller vouches that every front equals its transpose)
  if (sch.optimistic && !h_env.empty()) {
    sch.env = true;
    sch.h_env = h_env.data();
    if (sizeof(T) == 8) {  // the K-sorted tile order (Float64): main and side stream
      sch.perm_cap = (size_t)count * hs_env_perm_stride(hs_env_perm_slot(maxm));
      sch.perm = buf.template get<uint16_t>(2 * sch.perm_cap);
      sch.perm_side = sch.perm + sch.perm_cap;
    }
  }
  const auto h0 = std::chrono::steady_clock::now();
  sch.factor_fronts();
  HS_HIP(hipEventRecord(ev[1], st.main));
  if (getenv("HS_HOOK_VERBOSE"))
    fprintf(stderr, "[hook] host enqueue time %.2f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count());
  HS_HIP(hipEventSynchronize(ev[1]));
  float ms = 0.f;
  HS_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
  if (ms_out) *ms_out = ms;
  HS_HIP(hipDeviceSynchronize());
}

template <class T>
void FrontBatch<T>::copy_out(T* outLF, T* outUR, T* outSB, int64_t* out_rperm, int64_t* info, int64_t* growth, T* outInvL, T* outInvU, T* outInv256L,
                             T* outInv256U) {
  std::vector<int> ip;
  size_t pLF = 0, pUR = 0, pSB = 0, pR = 0, pInv = 0, pInv256 = 0;
  for (int64_t k = 0; k < count; ++k) {
    const Off& x = o[k];
    const NodeDesc<T>& d = hn[k];
    const int ni = x.ni, nb = x.nb, m = x.m;
    if (ni > 0 && outLF) bring_block(outLF + pLF, m, d.LF, x.ldl, m, ni);
    if (ni > 0 && nb > 0 && outUR) bring_block(outUR + pUR, ni, d.UR, x.ldu, ni, nb);
    if (nb > 0 && outSB) bring_block(outSB + pSB, nb, d.SB, x.lds, nb, nb);
    ip.resize((size_t)ni + 2);
    HS_HIP(hipMemcpy(ip.data(), d.rperm, sizeof(int) * ((size_t)ni + 2), hipMemcpyDeviceToHost));  // rperm, info, growth
    if (out_rperm)
      for (int i = 0; i < ni; ++i) out_rperm[pR + i] = ip[i];
    if (info) info[k] = ip[ni];
    if (growth) growth[k] = ip[ni + 1];
    const size_t n32 = (size_t)x.nblk * HS_PB * HS_PB, n256 = (size_t)x.nb256 * 65536;
    if (outInvL && n32) HS_HIP(hipMemcpy(outInvL + pInv, d.invL, sizeof(T) * n32, hipMemcpyDeviceToHost));
    if (outInvU && n32) HS_HIP(hipMemcpy(outInvU + pInv, d.invU, sizeof(T) * n32, hipMemcpyDeviceToHost));
    if (outInv256L && n256) HS_HIP(hipMemcpy(outInv256L + pInv256, d.inv256L, sizeof(T) * n256, hipMemcpyDeviceToHost));
    if (outInv256U && n256) HS_HIP(hipMemcpy(outInv256U + pInv256, d.inv256U, sizeof(T) * n256, hipMemcpyDeviceToHost));
    pLF += (size_t)m * ni; pUR += (size_t)ni * nb; pSB += (size_t)nb * nb; pR += ni; pInv += n32; pInv256 += n256;
  }
}

template <class T>
static void front_batch_hook(int64_t count, const int64_t* ni_, const int64_t* nb_, int mode, const T* F, T* outLF, T* outUR, T* outSB,
                             int64_t* out_rperm, int64_t* info, int64_t* growth, T* outInvL, T* outInvU, T* outInv256L, T* outInv256U,
                             double* ms_out, const int32_t* env = nullptr, bool sym = false) {
  FrontBatch<T>::check(sym ? "hsk_front_batch_sym" : "hsk_front_batch", count, ni_, nb_, F, mode, 0, 7);
  if (sym && mode != 1 && mode != 2 && mode != (2 | 4))
    HS_FAIL(HS_ERR_ARGUMENT, mode, "hsk_front_batch_sym: the symmetric schedule runs under optimistic pivoting only (modes 1, 2 and 2 | 4)");
  if (env && (mode & 3) != 1 && (mode & 3) != 2) HS_FAIL(HS_ERR_ARGUMENT, mode, "hsk_front_batch_env: block envelopes hold under optimistic pivoting only (modes 1, 2)");
  if ((outInvL || outInvU || outInv256L || outInv256U) && (mode & 3) < 2)
    HS_FAIL(HS_ERR_ARGUMENT, mode, "hsk_front_batch: the stored inverses are returned by modes 2 and 3 only");
  FrontBatch<T> fb;
  fb.setup(count, ni_, nb_, F);
  if (env) fb.set_env(env);
  fb.upload_solve();
  fb.factor(mode, ms_out, sym);
  fb.copy_out(outLF, outUR, outSB, out_rperm, info, growth, outInvL, outInvU, outInv256L, outInv256U);
}

// One tree level of ldiv!: the batch above, factored in mode 2 or 3, then the level's forward and backward sweeps on a global vector (the
// contract is in include/hs_kernels.h).  The sweeps are sweep_level_fwd / sweep_level_bwd (hs_sweep.h), the functions the level loops of
// hs_api.hip call for every level -- here without the low-rank and HSS calls around and between them, and with `path` given instead of read
// from HS_SOLVE_FLOW / HS_SOLVE_WIDE (hs_sweep_path).
template <class T>
static void sweep_level_hook(int64_t count, const int64_t* ni_, const int64_t* nb_, int mode, const T* F, const int64_t* flags, int64_t n,
                             const int64_t* fidx, const T* b, int path, int trans, int tall, T* outLF, T* outUR, int64_t* out_rperm, int64_t* info,
                             int64_t* growth, T* outInvL, T* outInvU, T* outInv256L, T* outInv256U, T* out_y, T* out_bfwd, T* out_x, T* out_bbwd,
                             int* tall_used) {
  const char* name = "hsk_sweep_level";
  FrontBatch<T>::check(name, count, ni_, nb_, F, mode, 2);
  if (!fidx || !b || n <= 0 || n > 0x7fffffff || path < 0 || path > 2 || trans < 0 || trans > 2 || tall < -1 || tall > 1)
    HS_FAIL(HS_ERR_ARGUMENT, 0, "%s: fidx and b non-null, n in [1, 2^31), path in 0..2, trans in 0..2 and tall in -1..1 required", name);
  if (path == 2 && trans != 0) HS_FAIL(HS_ERR_ARGUMENT, trans, "%s: the 32-column sweeps (path 2) exist for trans = 0 only", name);
  if (trans == 2 && sizeof(T) == 8) HS_FAIL(HS_ERR_ARGUMENT, trans, "%s: trans = 2 (adjoint) is for ComplexF64; Float64 has trans = 1", name);
  size_t nidx = 0;
  for (int64_t k = 0; k < count; ++k) nidx += (size_t)(ni_[k] + nb_[k]);
  std::vector<int> hidx(nidx + 1, 0);
  {
    std::vector<char> seen((size_t)n, 0);
    for (size_t p = 0; p < nidx; ++p) {
      if (fidx[p] < 0 || fidx[p] >= n || seen[(size_t)fidx[p]])
        HS_FAIL(HS_ERR_ARGUMENT, (int64_t)p, "%s: fidx[%lld] = %lld is outside 0:%lld or occurs twice (the fronts of a level are disjoint)", name,
                (long long)p, (long long)fidx[p], (long long)n - 1);
      seen[(size_t)fidx[p]] = 1;
      hidx[p] = (int)fidx[p];
    }
  }
  FrontBatch<T> fb;
  fb.setup(count, ni_, nb_, F);
  struct MappedWord {  // the error word the sweep kernels write: host memory the device sees (freed after the device buffers, as before)
    int* p = nullptr;
    ~MappedWord() {
      if (p) (void)hipHostFree(p);
    }
  } err;
  HsDevBuf buf(name);
  int* dfidx = buf.get<int>(nidx + 1);
  HS_HIP(hipMemcpy(dfidx, hidx.data(), sizeof(int) * (nidx + 1), hipMemcpyHostToDevice));
  // woff / poff as hs_analyze lays them out: packed, one entry of slack at the end of the buffers
  long long woff = 0, poff = 0;
  size_t ioff = 0;
  for (int64_t k = 0; k < count; ++k) {
    SolveNode<T>& q = fb.hs[k];
    q.fidx = dfidx + ioff;
    q.woff = woff;
    q.poff = poff;
    if (flags && (flags[k] & 1)) {
      q.compressed = 1;
      q.mrows = q.ni;
    }
    ioff += (size_t)q.m;
    woff += q.ni;
    poff += (long long)((q.nb + 511) / 512) * q.ni;
  }
  fb.upload_solve();
  fb.factor(mode, nullptr);
  fb.copy_out(outLF, outUR, nullptr, out_rperm, info, growth, outInvL, outInvU, outInv256L, outInv256U);
  bool blanked = false;
  for (int64_t k = 0; k < count; ++k)
    if (flags && (flags[k] & 2)) {  // as hs_analyze blanks the descriptor of a front whose interior block is an HSS matrix
      SolveNode<T>& q = fb.hs[k];
      q.ni = q.nb = q.m = q.mrows = 0;
      blanked = true;
    }
  if (blanked) fb.upload_solve();
  const size_t nw = (size_t)(woff + 1), wbytes = sizeof(T) * nw;
  T* w1 = buf.get<T>(nw);
  T* w2 = buf.get<T>(nw);
  T* e1 = buf.get<T>(nw);
  T* e2 = buf.get<T>(nw);
  T* part = buf.get<T>((size_t)(poff + 1));
  T* db = buf.get<T>((size_t)n);
  int* counter = buf.get<int>(1);
  HS_HIP(hipHostMalloc((void**)&err.p, sizeof(int), hipHostMallocMapped));
  *err.p = 0;
  HS_HIP(hipMemset(w1, 0, wbytes));
  HS_HIP(hipMemset(w2, 0, wbytes));
  HS_HIP(hipMemset(part, 0, sizeof(T) * (size_t)(poff + 1)));
  HS_HIP(hipMemcpy(db, b, sizeof(T) * (size_t)n, hipMemcpyHostToDevice));
  const SweepLevel<T> lvl = {fb.dsn, (int)count, fb.maxni, fb.maxnb, fb.maxm, w1, w2, part, db, e1, e2, err.p};
  const hipStream_t s = nullptr;
  const int tall_rule = hs_fwd_flow_tall<T>(lvl.nfronts, lvl.maxnb);
  if (tall_used) *tall_used = (path == 0 && trans == 0) ? (tall >= 0 ? tall : tall_rule) : 0;
  auto arm = [&] {  // flow_arm and a fresh workgroup-id counter
    HS_HIP(hipMemsetAsync(e1, 0xFF, wbytes, s));
    HS_HIP(hipMemsetAsync(e2, 0xFF, wbytes, s));
    HS_HIP(hipMemsetAsync(counter, 0, sizeof(int), s));
  };
  auto finish = [&](const char* dir) {  // flow_check
    HS_HIP(hipDeviceSynchronize());
    if (*err.p) HS_FAIL(HS_ERR_DEVICE, 0, "%s: a workgroup of the %s sweep waited for a block that never arrived", name, dir);
  };
  auto copy_w = [&](T* out) {  // the level's w2, packed per front (ni entries each)
    if (out && woff > 0) HS_HIP(hipMemcpy(out, w2, sizeof(T) * (size_t)woff, hipMemcpyDeviceToHost));
  };
  auto copy_b = [&](T* out) {
    if (out) HS_HIP(hipMemcpy(out, db, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost));
  };
  const bool level_on = lvl.maxni > 0;  // (solve_fwd / solve_bwd skip a level without interior DOFs)
  // forward
  if (level_on) {
    arm();
    sweep_level_fwd<T>(lvl, path, trans, counter, s, tall);
    finish("forward");
  }
  copy_w(out_y);
  copy_b(out_bfwd);
  // backward, on the b and y the forward sweep left
  if (level_on) {
    arm();
    sweep_level_bwd<T>(lvl, path, trans, counter, s);
    finish("backward");
  }
  copy_w(out_x);
  copy_b(out_bbwd);
}
extern "C" int hsk_sweep_level_d(int64_t count, const int64_t* ni, const int64_t* nb, int mode, const double* F, const int64_t* flags, int64_t n,
                                 const int64_t* fidx, const double* b, int path, int trans, int tall, double* outLF, double* outUR,
                                 int64_t* out_rperm, int64_t* info, int64_t* growth, double* outInvL, double* outInvU, double* outInv256L,
                                 double* outInv256U, double* y, double* b_fwd, double* x, double* b_bwd, int* tall_used) {
  HS_GUARD(sweep_level_hook<double>(count, ni, nb, mode, F, flags, n, fidx, b, path, trans, tall, outLF, outUR, out_rperm, info, growth, outInvL,
                                    outInvU, outInv256L, outInv256U, y, b_fwd, x, b_bwd, tall_used));
}
extern "C" int hsk_sweep_level_z(int64_t count, const int64_t* ni, const int64_t* nb, int mode, const double* F, const int64_t* flags, int64_t n,
                                 const int64_t* fidx, const double* b, int path, int trans, int tall, double* outLF, double* outUR,
                                 int64_t* out_rperm, int64_t* info, int64_t* growth, double* outInvL, double* outInvU, double* outInv256L,
                                 double* outInv256U, double* y, double* b_fwd, double* x, double* b_bwd, int* tall_used) {
  HS_GUARD(sweep_level_hook<cplx>(count, ni, nb, mode, (const cplx*)F, flags, n, fidx, (const cplx*)b, path, trans, tall, (cplx*)outLF, (cplx*)outUR,
                                  out_rperm, info, growth, (cplx*)outInvL, (cplx*)outInvU, (cplx*)outInv256L, (cplx*)outInv256U, (cplx*)y,
                                  (cplx*)b_fwd, (cplx*)x, (cplx*)b_bwd, tall_used));
}
extern "C" int hsk_sweep_path() { return hs_sweep_path(); }
extern "C" int hsk_flow_tall_rule(int is_complex, int64_t nbatch, int64_t maxnb) {
  if (nbatch < 0 || nbatch > 0x7fffffff || maxnb < 0 || maxnb > 0x7fffffff) return -1;
  return is_complex ? hs_fwd_flow_tall<cplx>((int)nbatch, (int)maxnb) : hs_fwd_flow_tall<double>((int)nbatch, (int)maxnb);
}

extern "C" int hsk_front_batch_d(int64_t count, const int64_t* ni, const int64_t* nb, int mode, const double* F, double* outLF, double* outUR,
                                 double* outSB, int64_t* out_rperm, int64_t* info, int64_t* growth, double* outInvL, double* outInvU,
                                 double* outInv256L, double* outInv256U, double* ms_out) {
  HS_GUARD(front_batch_hook<double>(count, ni, nb, mode, F, outLF, outUR, outSB, out_rperm, info, growth, outInvL, outInvU, outInv256L, outInv256U, ms_out));
}
extern "C" int hsk_front_batch_env_d(int64_t count, const int64_t* ni, const int64_t* nb, int mode, const double* F, const int32_t* env, double* outLF,
                                     double* outUR, double* outSB, int64_t* out_rperm, int64_t* info, int64_t* growth) {
  HS_GUARD(front_batch_hook<double>(count, ni, nb, mode, F, outLF, outUR, outSB, out_rperm, info, growth, nullptr, nullptr, nullptr, nullptr, nullptr, env));
}
extern "C" int hsk_front_batch_z(int64_t count, const int64_t* ni, const int64_t* nb, int mode, const double* F, double* outLF, double* outUR,
                                 double* outSB, int64_t* out_rperm, int64_t* info, int64_t* growth, double* outInvL, double* outInvU,
                                 double* outInv256L, double* outInv256U, double* ms_out) {
  HS_GUARD(front_batch_hook<cplx>(count, ni, nb, mode, (const cplx*)F, (cplx*)outLF, (cplx*)outUR, (cplx*)outSB, out_rperm, info, growth,
                                  (cplx*)outInvL, (cplx*)outInvU, (cplx*)outInv256L, (cplx*)outInv256U, ms_out));
}
// hsk_front_batch_{d,z} with Sched::sym = true: every front must equal its transpose (plain, not conjugated); modes 1, 2 and 2 | 4 only.
extern "C" int hsk_front_batch_sym_d(int64_t count, const int64_t* ni, const int64_t* nb, int mode, const double* F, double* outLF, double* outUR,
                                     double* outSB, int64_t* out_rperm, int64_t* info, int64_t* growth, double* outInvL, double* outInvU,
                                     double* outInv256L, double* outInv256U, double* ms_out) {
  HS_GUARD(front_batch_hook<double>(count, ni, nb, mode, F, outLF, outUR, outSB, out_rperm, info, growth, outInvL, outInvU, outInv256L, outInv256U, ms_out,
                                    nullptr, true));
}
extern "C" int hsk_front_batch_sym_z(int64_t count, const int64_t* ni, const int64_t* nb, int mode, const double* F, double* outLF, double* outUR,
                                     double* outSB, int64_t* out_rperm, int64_t* info, int64_t* growth, double* outInvL, double* outInvU,
                                     double* outInv256L, double* outInv256U, double* ms_out) {
  HS_GUARD(front_batch_hook<cplx>(count, ni, nb, mode, (const cplx*)F, (cplx*)outLF, (cplx*)outUR, (cplx*)outSB, out_rperm, info, growth,
                                  (cplx*)outInvL, (cplx*)outInvU, (cplx*)outInv256L, (cplx*)outInv256U, ms_out, nullptr, true));
}

// Batches Sched::factor_fronts has sent to factor_fronts_lookahead since the last reset (process-wide, host only): one note per batch.
namespace {
std::atomic<long long> g_lookahead_runs{0};
}
void hs_lookahead_note() { g_lookahead_runs.fetch_add(1, std::memory_order_relaxed); }
extern "C" long long hsk_lookahead_runs(int reset) { return reset ? g_lookahead_runs.exchange(0) : g_lookahead_runs.load(); }

// `count` fronts of one shape, tournament pivoting without solve descriptors (mode 0); HS_HOOK_OPTIMISTIC=1: mode 1, and a raised growth
// flag comes back through `info` as -1
template <class T>
static void front_hook(int64_t count, int64_t ni, int64_t nb, const T* F, T* outLF, T* outUR, T* outSB, int64_t* out_rperm, int64_t* info,
                       double* ms_out) {
  if (count <= 0) HS_FAIL(HS_ERR_ARGUMENT, count, "hsk_front_factor: count must be positive");
  const bool hook_opt = getenv("HS_HOOK_OPTIMISTIC") != nullptr;
  std::vector<int64_t> vni(count, ni), vnb(count, nb), inf(count), gr(count);
  front_batch_hook<T>(count, vni.data(), vnb.data(), hook_opt ? 1 : 0, F, outLF, outUR, outSB, out_rperm, inf.data(), gr.data(), nullptr, nullptr,
                      nullptr, nullptr, ms_out);
  if (info)
    for (int64_t k = 0; k < count; ++k) info[k] = hook_opt ? ((inf[k] != 0 || gr[k] != 0) ? -1 : 0) : inf[k];
}

extern "C" int hsk_front_factor_d(int64_t count, int64_t ni, int64_t nb, const double* F, double* outLF, double* outUR, double* outSB,
                                  int64_t* out_rperm, int64_t* info, double* ms_out) {
  HS_GUARD(front_hook<double>(count, ni, nb, F, outLF, outUR, outSB, out_rperm, info, ms_out));
}
extern "C" int hsk_front_factor_z(int64_t count, int64_t ni, int64_t nb, const double* F, double* outLF, double* outUR, double* outSB,
                                  int64_t* out_rperm, int64_t* info, double* ms_out) {
  HS_GUARD(front_hook<cplx>(count, ni, nb, (const cplx*)F, (cplx*)outLF, (cplx*)outUR, (cplx*)outSB, out_rperm, info, ms_out));
}

// Low-rank compression of a dense rows x cols block (column-major host array): returns the rank r and
// the dense factors C (rows x r) and Z (r x cols), X ~= C * Z, built from the device representation.
template <class T>
static void lowrank_hook(int64_t rows, int64_t cols, const T* X, double atol, double rtol, int64_t kinit, int64_t seed, int64_t* r_out, T* Cout,
                         T* Zout, int64_t cap) {
  need_device();
  HsDevBuf buf("hsk_lowrank");
  const int ldx = ((int)rows + 1) / 2 * 2;
  T* dX = buf.get<T>((size_t)ldx * cols + 32);
  HS_HIP(hipMemcpy2D(dX, sizeof(T) * ldx, X, sizeof(T) * rows, sizeof(T) * rows, cols, hipMemcpyHostToDevice));
  // the primitive the compressed fronts use (hs_compress.h): interpolative form, rank and interpolation from the orthogonalisation of
  // the sketch rows in tournament-pivot order (lowrank_id_batch); HS_LR_QR=0: the LU-based factors of hs_lowrank.hip
  static const bool lr_qr = !(getenv("HS_LR_QR") && getenv("HS_LR_QR")[0] == '0');
  LowRank<T> lr;
  struct Release {  // whatever the compression has allocated by the time this scope is left
    LowRank<T>& lr;
    ~Release() { lowrank_free(lr); }
  } release{lr};
  if (lr_qr) {
    LowRankJob<T> job{dX, ldx, (int)rows, (int)cols, (int)kinit, (uint64_t)seed, &lr, 0};
    HS_CHECK(lowrank_id_batch<T>(&job, 1, atol, rtol, 0));
  } else {
    HS_CHECK(lowrank_compress<T>(dX, ldx, (int)rows, (int)cols, atol, rtol, (int)kinit, (uint64_t)seed, 0, &lr));
  }
  *r_out = lr.r;
  if (lr.r > cap) HS_FAIL(HS_ERR_ARGUMENT, lr.r, "rank %d exceeds the output capacity %lld", lr.r, (long long)cap);
  if (lr.Cd) {
    if (lr.r > 0) bring_block(Cout, rows, lr.Cd, lr.ldc, rows, lr.r);
  } else {
    std::vector<T> hL((size_t)lr.ldp * lr.k);
    std::vector<int> rp(rows);
    HS_HIP(hipMemcpy(hL.data(), lr.Lp, sizeof(T) * hL.size(), hipMemcpyDeviceToHost));
    HS_HIP(hipMemcpy(rp.data(), lr.rperm, sizeof(int) * rows, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < rows; ++i)
      for (int64_t j = 0; j < lr.r; ++j) {
        T v = (i == j) ? Scal<T>::one() : (i > j ? hL[(size_t)i + (size_t)j * lr.ldp] : Scal<T>::zero());
        Cout[(size_t)rp[i] + (size_t)j * rows] = v;
      }
  }
  if (lr.r > 0) bring_block(Zout, lr.r, lr.Z, lr.ldz, lr.r, cols);
}
extern "C" int hsk_lowrank_d(int64_t rows, int64_t cols, const double* X, double atol, double rtol, int64_t kinit, int64_t seed, int64_t* r_out,
                             double* Cout, double* Zout, int64_t cap) {
  HS_GUARD(lowrank_hook<double>(rows, cols, X, atol, rtol, kinit, seed, r_out, Cout, Zout, cap));
}
extern "C" int hsk_lowrank_z(int64_t rows, int64_t cols, const double* X, double atol, double rtol, int64_t kinit, int64_t seed, int64_t* r_out,
                             double* Cout, double* Zout, int64_t cap) {
  HS_GUARD(lowrank_hook<cplx>(rows, cols, (const cplx*)X, atol, rtol, kinit, seed, r_out, (cplx*)Cout, (cplx*)Zout, cap));
}

// The panel products of the block solves (kernels_solve_multi.hip, kernels_solve_multi_t.hip) on host data, staged by one helper: X and C
// reach the kernel row-major with a pitch of 64, as the work blocks of the driver do.  A is lda x acols with arows rows in use (forward
// M x K, transposed K x M); map (null: none) has nmap entries in 0..nmap-1; launch(dA, dX, dC, dmap, pitch) fills the problem struct.
template <class T, class Launch>
static void multi_prob_stage(const char* name, int64_t M, int64_t K, int64_t kc, const T* A, int64_t lda, int64_t arows, int64_t acols, const T* X, int64_t ldx,
                             T* C, int64_t ldc, const int32_t* map, int64_t nmap, Launch launch) {
  bool ok = M >= 1 && K >= 0 && kc >= 1 && kc <= 64 && lda >= std::max<int64_t>(arows, 1) && ldx >= std::max<int64_t>(K, 1) && ldc >= M && A && X && C;
  for (int64_t i = 0; ok && map && i < nmap; ++i) ok = map[i] >= 0 && map[i] < nmap;
  if (!ok) HS_FAIL(HS_ERR_ARGUMENT, 0, "%s: M >= 1, K >= 0, kc in 1..64, leading dimensions, non-null arrays and map entries inside their range required", name);
  need_device();
  const int64_t P = 64;
  std::vector<T> hx((size_t)std::max<int64_t>(K, 1) * P), hc((size_t)M * P);
  for (int64_t c = 0; c < kc; ++c) {
    for (int64_t k = 0; k < K; ++k) hx[k * P + c] = X[k + c * ldx];
    for (int64_t i = 0; i < M; ++i) hc[i * P + c] = C[i + c * ldc];
  }
  HsDevBuf buf(name);
  T* dA = buf.get<T>((size_t)lda * std::max<int64_t>(acols, 1));
  T* dX = buf.get<T>(hx.size());
  T* dC = buf.get<T>(hc.size());
  if (K > 0) HS_HIP(hipMemcpy(dA, A, sizeof(T) * ((size_t)lda * (acols - 1) + arows), hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(dX, hx.data(), sizeof(T) * hx.size(), hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(dC, hc.data(), sizeof(T) * hc.size(), hipMemcpyHostToDevice));
  int* dmap = nullptr;
  if (map && nmap > 0) {
    dmap = buf.get<int>((size_t)nmap);
    HS_HIP(hipMemcpy(dmap, map, sizeof(int) * (size_t)nmap, hipMemcpyHostToDevice));
  }
  launch(dA, dX, dC, dmap, P);
  HS_HIP(hipDeviceSynchronize());
  HS_HIP(hipMemcpy(hc.data(), dC, sizeof(T) * hc.size(), hipMemcpyDeviceToHost));
  for (int64_t c = 0; c < kc; ++c)
    for (int64_t i = 0; i < M; ++i) C[i + c * ldc] = hc[i * P + c];
}
// The same staging for the two products over a Float32 panel (kernels_solve_multi_f32.hip): A arrives in Float64, is demoted on the device
// by the library's demotion kernel (kernels_f32.hip) into a copy with the leading dimension hs_f32_create would give it, and the product
// reads the copy.
#include "hs_f32.h"
template <class T, class Launch>
static void multi_prob_f32_stage(const char* name, int64_t M, int64_t K, int64_t kc, const T* A, int64_t lda, int64_t arows, int64_t acols, const T* X, int64_t ldx, T* C,
                                 int64_t ldc, const int32_t* map, int64_t nmap, Launch launch) {
  typedef typename F32Of<T>::type S;
  constexpr int RE = sizeof(T) / 8;
  const long long ldd = RE == 2 ? std::max<long long>(arows, 1) : hs_f32_ld(arows);
  HsDevBuf buf(name);
  multi_prob_stage<T>(name, M, K, kc, A, lda, arows, acols, X, ldx, C, ldc, map, nmap, [&](const T* dA, const T* dX, T* dC, const int* dmap, int64_t P) {
    S* dS = nullptr;
    if (arows >= 1) {  // (a transposed product with K = 0 has no panel)
      dS = buf.get<S>((size_t)ldd * std::max<int64_t>(acols, 1));
      unsigned long long* dcnt = buf.get<unsigned long long>(2);
      F32Job* djob = buf.get<F32Job>(1);
      HS_HIP(hipMemset(dcnt, 0, 2 * sizeof(unsigned long long)));
      if (K > 0) {
        const F32Job job{(const double*)dA, (void*)dS, (long long)lda * RE, ldd * RE, (int)arows * RE, (int)acols};
        HS_HIP(hipMemcpy(djob, &job, sizeof job, hipMemcpyHostToDevice));
        launch_f32_demote(djob, 1, job.rows, job.cols, false, dcnt, 0);
      }
    }
    launch(dS, (int)ldd, dX, dC, dmap, P);
  });
}
// the staging of a hook whose panel is stored as S: launch(dA as S, its leading dimension, dX, dC, dmap, pitch)
template <class T, class S, class Launch>
static void multi_prob_stage_as(const char* name, int64_t M, int64_t K, int64_t kc, const T* A, int64_t lda, int64_t arows, int64_t acols, const T* X, int64_t ldx, T* C,
                                int64_t ldc, const int32_t* map, int64_t nmap, Launch launch) {
  if constexpr (std::is_same<T, S>::value)
    multi_prob_stage<T>(name, M, K, kc, A, lda, arows, acols, X, ldx, C, ldc, map, nmap,
                        [&](const T* dA, const T* dX, T* dC, const int* dmap, int64_t P) { launch(dA, (int)lda, dX, dC, dmap, P); });
  else
    multi_prob_f32_stage<T>(name, M, K, kc, A, lda, arows, acols, X, ldx, C, ldc, map, nmap, launch);
}
// C = A X or C - A X, A M x K; map: cmap, row i of the product goes to row map[i] of C
template <class T, class S>
static void multi_prob_hook(int64_t M, int64_t K, int64_t kc, const T* A, int64_t lda, const T* X, int64_t ldx, T* C, int64_t ldc, int minus, int trap, const int32_t* map) {
  const char* name = std::is_same<T, S>::value ? "hsk_multi_prob" : "hsk_multi_prob_f32";
  multi_prob_stage_as<T, S>(name, M, K, kc, A, lda, M, K, X, ldx, C, ldc, map, M, [&](const S* dA, int ld, const T* dX, T* dC, const int* dmap, int64_t P) {
    MultiProb<T, S> p;
    memset(&p, 0, sizeof p);
    p.A = dA; p.lda = ld; p.M = (int)M; p.K = (int)K; p.trap = trap ? 1 : 0;
    p.X = dX; p.xrs = P;
    p.Cin = minus ? dC : nullptr;
    p.C = dC; p.crs = P; p.cmap = dmap;
    launch_multi_prob<T, S>(p, (int)kc, 0);
  });
}
// C = op(A)^T X or C - op(A)^T X, A K x M; map: xmap, row k of A meets row map[k] of X
template <class T, class S>
static void multi_prob_t_hook(int64_t M, int64_t K, int64_t kc, const T* A, int64_t lda, const T* X, int64_t ldx, T* C, int64_t ldc, int minus, int trap, int conj,
                              const int32_t* map) {
  const char* name = std::is_same<T, S>::value ? "hsk_multi_prob_t" : "hsk_multi_prob_t_f32";
  multi_prob_stage_as<T, S>(name, M, K, kc, A, lda, K, M, X, ldx, C, ldc, map, K, [&](const S* dA, int ld, const T* dX, T* dC, const int* dmap, int64_t P) {
    MultiProbT<T, S> p;
    memset(&p, 0, sizeof p);
    p.A = dA; p.lda = ld; p.M = (int)M; p.K = (int)K; p.trap = trap ? 1 : 0; p.conj = (conj && sizeof(T) == 16) ? 1 : 0;
    p.X = dX; p.xrs = P; p.xmap = dmap;
    p.Cin = minus ? dC : nullptr;
    p.C = dC; p.crs = P;
    launch_multi_prob_t<T, S>(p, (int)kc, 0);
  });
}
// one triangular product of hs_mul_* (kernels_solve_multi_mul.hip): C = tri(A) X or C + tri(A) X, and the transposed counterpart
template <class T>
static void multi_tri_hook(int64_t M, int64_t K, int64_t kc, const T* A, int64_t lda, const T* X, int64_t ldx, T* C, int64_t ldc, int plus, int tri, const int32_t* map) {
  if (tri != 1 && tri != 2) HS_FAIL(HS_ERR_ARGUMENT, tri, "hsk_multi_tri: tri = %d (1: unit lower trapezoid, 2: upper triangle with the diagonal)", tri);
  multi_prob_stage<T>("hsk_multi_tri", M, K, kc, A, lda, M, K, X, ldx, C, ldc, map, M, [&](const T* dA, const T* dX, T* dC, const int* dmap, int64_t P) {
    MultiProbMul<T, T> p;
    memset(&p, 0, sizeof p);
    p.A = dA; p.lda = (int)lda; p.M = (int)M; p.K = (int)K; p.trap = tri;
    p.X = dX; p.xrs = P;
    p.Cin = plus ? dC : nullptr;
    p.C = dC; p.crs = P; p.cmap = dmap;
    launch_mul_prob<T>(p, (int)kc, 0);
  });
}
template <class T>
static void multi_tri_t_hook(int64_t M, int64_t K, int64_t kc, const T* A, int64_t lda, const T* X, int64_t ldx, T* C, int64_t ldc, int plus, int tri, int conj,
                             const int32_t* map) {
  if (tri != 1 && tri != 2) HS_FAIL(HS_ERR_ARGUMENT, tri, "hsk_multi_tri_t: tri = %d (1: unit lower trapezoid, 2: upper triangle with the diagonal)", tri);
  multi_prob_stage<T>("hsk_multi_tri_t", M, K, kc, A, lda, K, M, X, ldx, C, ldc, map, K, [&](const T* dA, const T* dX, T* dC, const int* dmap, int64_t P) {
    MultiProbMulT<T, T> p;
    memset(&p, 0, sizeof p);
    p.A = dA; p.lda = (int)lda; p.M = (int)M; p.K = (int)K; p.trap = tri; p.conj = (conj && sizeof(T) == 16) ? 1 : 0;
    p.X = dX; p.xrs = P; p.xmap = dmap;
    p.Cin = plus ? dC : nullptr;
    p.C = dC; p.crs = P;
    launch_mul_prob_t<T>(p, (int)kc, 0);
  });
}
extern "C" int hsk_multi_tri_d(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C, int64_t ldc, int plus, int tri,
                               const int32_t* map) {
  HS_GUARD(multi_tri_hook<double>(M, K, kc, A, lda, X, ldx, C, ldc, plus, tri, map));
}
extern "C" int hsk_multi_tri_z(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C, int64_t ldc, int plus, int tri,
                               const int32_t* map) {
  HS_GUARD(multi_tri_hook<cplx>(M, K, kc, (const cplx*)A, lda, (const cplx*)X, ldx, (cplx*)C, ldc, plus, tri, map));
}
extern "C" int hsk_multi_tri_t_d(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C, int64_t ldc, int plus, int tri,
                                 int conj, const int32_t* map) {
  HS_GUARD(multi_tri_t_hook<double>(M, K, kc, A, lda, X, ldx, C, ldc, plus, tri, conj, map));
}
extern "C" int hsk_multi_tri_t_z(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C, int64_t ldc, int plus, int tri,
                                 int conj, const int32_t* map) {
  HS_GUARD(multi_tri_t_hook<cplx>(M, K, kc, (const cplx*)A, lda, (const cplx*)X, ldx, (cplx*)C, ldc, plus, tri, conj, map));
}
extern "C" int hsk_multi_prob_d(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C,
                                int64_t ldc, int minus, int trap, const int32_t* map) {
  HS_GUARD(multi_prob_hook<double, double>(M, K, kc, A, lda, X, ldx, C, ldc, minus, trap, map));
}
extern "C" int hsk_multi_prob_z(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C,
                                int64_t ldc, int minus, int trap, const int32_t* map) {
  HS_GUARD(multi_prob_hook<cplx, cplx>(M, K, kc, (const cplx*)A, lda, (const cplx*)X, ldx, (cplx*)C, ldc, minus, trap, map));
}
extern "C" int hsk_multi_prob_t_d(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C,
                                  int64_t ldc, int minus, int trap, int conj, const int32_t* map) {
  HS_GUARD(multi_prob_t_hook<double, double>(M, K, kc, A, lda, X, ldx, C, ldc, minus, trap, conj, map));
}
extern "C" int hsk_multi_prob_t_z(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C,
                                  int64_t ldc, int minus, int trap, int conj, const int32_t* map) {
  HS_GUARD(multi_prob_t_hook<cplx, cplx>(M, K, kc, (const cplx*)A, lda, (const cplx*)X, ldx, (cplx*)C, ldc, minus, trap, conj, map));
}
extern "C" int hsk_multi_prob_f32_d(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C,
                                    int64_t ldc, int minus, int trap, const int32_t* map) {
  HS_GUARD(multi_prob_hook<double, float>(M, K, kc, A, lda, X, ldx, C, ldc, minus, trap, map));
}
extern "C" int hsk_multi_prob_f32_z(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C,
                                    int64_t ldc, int minus, int trap, const int32_t* map) {
  HS_GUARD(multi_prob_hook<cplx, cplxf>(M, K, kc, (const cplx*)A, lda, (const cplx*)X, ldx, (cplx*)C, ldc, minus, trap, map));
}
extern "C" int hsk_multi_prob_t_f32_d(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C,
                                      int64_t ldc, int minus, int trap, int conj, const int32_t* map) {
  HS_GUARD(multi_prob_t_hook<double, float>(M, K, kc, A, lda, X, ldx, C, ldc, minus, trap, conj, map));
}
extern "C" int hsk_multi_prob_t_f32_z(int64_t M, int64_t K, int64_t kc, const double* A, int64_t lda, const double* X, int64_t ldx, double* C,
                                      int64_t ldc, int minus, int trap, int conj, const int32_t* map) {
  HS_GUARD(multi_prob_t_hook<cplx, cplxf>(M, K, kc, (const cplx*)A, lda, (const cplx*)X, ldx, (cplx*)C, ldc, minus, trap, conj, map));
}
// x <- (double)(float)x for every stored element hs_f32_create would demote, in place in the handle (hs_f32.hip)
extern "C" int hsk_round_factors_f32(hs_handle* F, int64_t* counts2) { HS_GUARD(hs_f32_round_in_place(F, counts2)); }

// one grouped launch of the transposed ULV product (kernels_ulv_t.hip) on caller-supplied jobs (include/hs_kernels.h)
#include "hs_ulv_t.h"
template <class T>
static void ulv_t_group_hook(int64_t njobs, const int64_t* desc, const T* Abuf, int64_t na, const T* Xbuf, int64_t nx, T* Cbuf, int64_t nc, int conj) {
  if (njobs < 1 || njobs > 65535 || !desc || !Abuf || !Xbuf || !Cbuf || na < 1 || nx < 1 || nc < 1)
    HS_FAIL(HS_ERR_ARGUMENT, 0, "hsk_ulv_t_group: 1..65535 jobs, their descriptions and non-empty buffers required");
  std::vector<UlvTJob<T>> jobs((size_t)njobs);
  int maxM = 0, maxN = 0;
  for (int64_t i = 0; i < njobs; ++i) {
    const int64_t* d = desc + 10 * i;
    const int64_t M = d[0], K = d[1], N = d[2], lda = d[3], ldx = d[4], ldc = d[5], ao = d[6], xo = d[7], co = d[8], fl = d[9];
    const bool empty = M == 0 || K == 0 || N == 0;
    bool ok = M >= 0 && K >= 0 && N >= 0 && M < (1 << 30) && K < (1 << 30) && N < (1 << 30) && ao >= 0 && xo >= 0 && co >= 0 && fl >= 0 && fl < 6;
    if (ok && !empty)
      ok = lda >= K && ldx >= K && ldc >= M && lda < (1 << 30) && ldx < (1 << 30) && ldc < (1 << 30) && ao + lda * (M - 1) + K <= na &&
           xo + ldx * (N - 1) + K <= nx && co + ldc * (N - 1) + M <= nc;
    if (!ok) HS_FAIL(HS_ERR_ARGUMENT, i, "hsk_ulv_t_group: job %lld reaches outside its buffers", (long long)i);
    UlvTJob<T>& j = jobs[(size_t)i];
    memset(&j, 0, sizeof j);
    if (empty) continue;  // (stays in the launch with M = K = N = 0: the kernel skips it)
    j.M = (int)M; j.K = (int)K; j.N = (int)N;
    j.lda = (int)lda; j.ldx = (int)ldx; j.ldc = j.ldcin = (int)ldc;
    j.conj = (conj && sizeof(T) == 16) ? 1 : 0;
    j.tri = (int)(fl >> 1);
    maxM = std::max(maxM, j.M);
    maxN = std::max(maxN, j.N);
  }
  need_device();
  HsDevBuf buf("hsk_ulv_t_group");
  T* dA = buf.get<T>((size_t)na);
  T* dX = buf.get<T>((size_t)nx);
  T* dC = buf.get<T>((size_t)nc);
  UlvTJob<T>* dJ = buf.get<UlvTJob<T>>(jobs.size());
  for (int64_t i = 0; i < njobs; ++i) {
    UlvTJob<T>& j = jobs[(size_t)i];
    if (j.M == 0) continue;
    const int64_t* d = desc + 10 * i;
    j.A = dA + d[6];
    j.X = dX + d[7];
    j.C = dC + d[8];
    j.Cin = (d[9] & 1) ? j.C : nullptr;
  }
  HS_HIP(hipMemcpy(dA, Abuf, sizeof(T) * (size_t)na, hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(dX, Xbuf, sizeof(T) * (size_t)nx, hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(dC, Cbuf, sizeof(T) * (size_t)nc, hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(dJ, jobs.data(), sizeof(UlvTJob<T>) * jobs.size(), hipMemcpyHostToDevice));
  launch_ulv_t<T>(dJ, (int)njobs, maxM, maxN, 0);
  HS_HIP(hipDeviceSynchronize());
  HS_HIP(hipMemcpy(Cbuf, dC, sizeof(T) * (size_t)nc, hipMemcpyDeviceToHost));
}
extern "C" int hsk_ulv_t_group_d(int64_t njobs, const int64_t* desc, const double* Abuf, int64_t na, const double* Xbuf, int64_t nx, double* Cbuf, int64_t nc, int conj) {
  HS_GUARD(ulv_t_group_hook<double>(njobs, desc, Abuf, na, Xbuf, nx, Cbuf, nc, conj));
}
extern "C" int hsk_ulv_t_group_z(int64_t njobs, const int64_t* desc, const double* Abuf, int64_t na, const double* Xbuf, int64_t nx, double* Cbuf, int64_t nc, int conj) {
  HS_GUARD(ulv_t_group_hook<cplx>(njobs, desc, (const cplx*)Abuf, na, (const cplx*)Xbuf, nx, (cplx*)Cbuf, nc, conj));
}

// The leaf-envelope builder of the analysis (hs_envelope.h), host only: tests compare it with a NumPy computation from A[idx][:, idx]
// hsk_sddmm_*: the reduction kernel of hs_sens_* (kernels_sens.hip) alone on host data
#include "hs_sens.h"
template <class T>
static void sddmm_hook(int64_t n, const int64_t* colptr, const int64_t* rowval, int64_t kc, const T* L, int64_t ldl, const T* R, int64_t ldr, int swap, int conjl, int conjr,
                       int diag, int form, T* G, double* seconds) {
  if (n < 1 || n > 0x7fffffff || kc < 1 || kc > 4096 || !colptr || !L || !R || !G || ldl < n || ldr < n || form < 0 || form > 1 || colptr[0] != 1)
    HS_FAIL(HS_ERR_ARGUMENT, 0, "hsk_sddmm: n >= 1, kc in 1..4096, 1-based colptr, leading dimensions >= n, form in 0:1 and non-null arrays required");
  const int64_t nnz = colptr[n] - 1;
  std::vector<int64_t> cp((size_t)n + 1);
  std::vector<int32_t> rv((size_t)std::max<int64_t>(nnz, 0));
  bool ok = nnz >= 0 && (nnz == 0 || rowval);
  for (int64_t j = 0; ok && j <= n; ++j) {
    cp[(size_t)j] = colptr[j] - 1;
    ok = j == 0 || cp[(size_t)j] >= cp[(size_t)j - 1];
  }
  for (int64_t e = 0; ok && e < nnz; ++e) {
    ok = rowval[e] >= 1 && rowval[e] <= n;
    rv[(size_t)e] = (int32_t)(rowval[e] - 1);
  }
  if (!ok) HS_FAIL(HS_ERR_ARGUMENT, 0, "hsk_sddmm: colptr decreases or rowval is outside 1:n");
  need_device();
  const int64_t glen = diag ? n : nnz, stride = hs_sens_row_stride((int)kc, sizeof(T) == 16);
  const bool staged = form == 1 && !diag;
  HsDevBuf b("hsk_sddmm");
  int64_t* dcp = b.get<int64_t>((size_t)(n + 1));
  int32_t* drv = b.get<int32_t>((size_t)nnz);
  int32_t* dec = b.get<int32_t>((size_t)nnz);
  T* dL = b.get<T>((size_t)ldl * kc);
  T* dR = b.get<T>((size_t)ldr * kc);
  T* dG = b.get<T>((size_t)glen);
  T* dG2 = seconds ? b.get<T>((size_t)glen) : dG;
  T* dLt = staged ? b.get<T>((size_t)n * stride) : dL;
  T* dRt = staged ? b.get<T>((size_t)n * stride) : dR;
  HS_HIP(hipMemcpy(dcp, cp.data(), sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice));
  if (nnz > 0) HS_HIP(hipMemcpy(drv, rv.data(), sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(dL, L, sizeof(T) * (size_t)ldl * kc, hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(dR, R, sizeof(T) * (size_t)ldr * kc, hipMemcpyHostToDevice));
  if (glen > 0) HS_HIP(hipMemcpy(dG, G, sizeof(T) * (size_t)glen, hipMemcpyHostToDevice));
  const HsSddmmFlags f{swap ? 1 : 0, conjl ? 1 : 0, conjr ? 1 : 0};
  launch_sens_entry_cols(dcp, n, nnz, dec, 0);
  auto run = [&](T* g) {
    if (diag) {
      launch_sddmm_diag<T>(dcp, drv, n, dL, ldl, dR, ldr, (int)kc, f, g, 0);
    } else if (staged) {
      launch_sens_rowstage<T>(dL, ldl, n, (int)kc, dLt, stride, 0);
      launch_sens_rowstage<T>(dR, ldr, n, (int)kc, dRt, stride, 0);
      launch_sddmm_rows<T>(drv, dec, nnz, dLt, dRt, stride, (int)kc, f, g, 0);
    } else {
      launch_sddmm<T>(drv, dec, nnz, dL, ldl, dR, ldr, (int)kc, f, g, 0);
    }
  };
  if (seconds) {  // one warm-up and three timed runs on a copy of G; the median
    HsEvents<2> ev;
    float ms[4] = {0.f, 0.f, 0.f, 0.f};
    if (glen > 0) HS_HIP(hipMemcpy(dG2, dG, sizeof(T) * (size_t)glen, hipMemcpyDeviceToDevice));
    for (int k = 0; k < 4; ++k) {
      HS_HIP(hipEventRecord(ev[0], 0));
      run(dG2);
      HS_HIP(hipEventRecord(ev[1], 0));
      HS_HIP(hipEventSynchronize(ev[1]));
      HS_HIP(hipEventElapsedTime(&ms[k], ev[0], ev[1]));
    }
    std::sort(ms + 1, ms + 4);
    *seconds = ms[2] * 1e-3;
  }
  run(dG);
  HS_HIP(hipDeviceSynchronize());
  if (glen > 0) HS_HIP(hipMemcpy(G, dG, sizeof(T) * (size_t)glen, hipMemcpyDeviceToHost));
}
extern "C" int hsk_sddmm_d(int64_t n, const int64_t* colptr, const int64_t* rowval, int64_t kc, const double* L, int64_t ldl, const double* R, int64_t ldr, int swap,
                           int conjl, int conjr, int diag, int form, double* G, double* seconds) {
  HS_GUARD(sddmm_hook<double>(n, colptr, rowval, kc, L, ldl, R, ldr, swap, conjl, conjr, diag, form, G, seconds));
}
extern "C" int hsk_sddmm_z(int64_t n, const int64_t* colptr, const int64_t* rowval, int64_t kc, const double* L, int64_t ldl, const double* R, int64_t ldr, int swap,
                           int conjl, int conjr, int diag, int form, double* G, double* seconds) {
  HS_GUARD(sddmm_hook<cplx>(n, colptr, rowval, kc, (const cplx*)L, ldl, (const cplx*)R, ldr, swap, conjl, conjr, diag, form, (cplx*)G, seconds));
}

// hsk_gn_rhs_*, hsk_gn_rowsq_*: the right-hand side and row square sum kernels of hs_tangent_* / hs_gn_* (kernels_gn.hip) alone on host data
#include "hs_gn.h"
template <class T>
static void gn_rhs_hook(int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const T* E, int pattern, const T* X, int64_t ldx, int64_t kc, T* P, int64_t ldp) {
  if (trans < 0 || trans > 2 || pattern < 0 || pattern > 1 || n < 1 || n > 0x7fffffff || kc < 1 || kc > 4096 || !colptr || !E || !X || !P || ldx < n || ldp < n ||
      colptr[0] != 1)
    HS_FAIL(HS_ERR_ARGUMENT, 0, "hsk_gn_rhs: trans in 0:2, pattern in 0:1, n >= 1, kc in 1..4096, 1-based colptr, leading dimensions >= n and non-null arrays required");
  const int64_t nnz = colptr[n] - 1;
  std::vector<int64_t> cp((size_t)n + 1), rp((size_t)n + 1, 0), tp((size_t)std::max<int64_t>(nnz, 0));
  std::vector<int32_t> rv((size_t)std::max<int64_t>(nnz, 0)), ci((size_t)std::max<int64_t>(nnz, 0));
  bool ok = nnz >= 0 && (nnz == 0 || rowval);
  for (int64_t j = 0; ok && j <= n; ++j) {
    cp[(size_t)j] = colptr[j] - 1;
    ok = j == 0 || cp[(size_t)j] >= cp[(size_t)j - 1];
  }
  for (int64_t j = 0; ok && j < n; ++j)
    for (int64_t e = cp[(size_t)j]; ok && e < cp[(size_t)j + 1]; ++e) {
      ok = rowval[e] >= 1 && rowval[e] <= n && (e == cp[(size_t)j] || rowval[e] > rowval[e - 1]);
      rv[(size_t)e] = (int32_t)(rowval[e] - 1);
    }
  if (!ok) HS_FAIL(HS_ERR_ARGUMENT, 0, "hsk_gn_rhs: colptr decreases, rowval is outside 1:n or the rows of a column do not ascend");
  // the CSR map: rows in column order, CSR entry -> CSC entry
  for (int64_t e = 0; e < nnz; ++e) ++rp[(size_t)rv[(size_t)e] + 1];
  for (int64_t i = 0; i < n; ++i) rp[(size_t)i + 1] += rp[(size_t)i];
  {
    std::vector<int64_t> cur(rp.begin(), rp.end() - 1);
    for (int64_t j = 0; j < n; ++j)
      for (int64_t e = cp[(size_t)j]; e < cp[(size_t)j + 1]; ++e) {
        const int64_t at = cur[(size_t)rv[(size_t)e]]++;
        ci[(size_t)at] = (int32_t)j;
        tp[(size_t)at] = e;
      }
  }
  need_device();
  const int64_t elen = pattern == 0 ? nnz : n;
  HsDevBuf b("hsk_gn_rhs");
  int64_t* dcp = b.get<int64_t>((size_t)(n + 1));
  int64_t* drp = b.get<int64_t>((size_t)(n + 1));
  int64_t* dtp = b.get<int64_t>((size_t)nnz);
  int32_t* drv = b.get<int32_t>((size_t)nnz);
  int32_t* dci = b.get<int32_t>((size_t)nnz);
  T* dE = b.get<T>((size_t)elen);
  T* dX = b.get<T>((size_t)ldx * kc);
  T* dP = b.get<T>((size_t)ldp * kc);
  HS_HIP(hipMemcpy(dcp, cp.data(), sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(drp, rp.data(), sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice));
  if (nnz > 0) {
    HS_HIP(hipMemcpy(dtp, tp.data(), sizeof(int64_t) * (size_t)nnz, hipMemcpyHostToDevice));
    HS_HIP(hipMemcpy(drv, rv.data(), sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice));
    HS_HIP(hipMemcpy(dci, ci.data(), sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice));
  }
  if (elen > 0) HS_HIP(hipMemcpy(dE, E, sizeof(T) * (size_t)elen, hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(dX, X, sizeof(T) * (size_t)ldx * kc, hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(dP, P, sizeof(T) * (size_t)ldp * kc, hipMemcpyHostToDevice));
  const int cjE = (sizeof(T) == 16 && trans == 2) ? 1 : 0;
  if (pattern == 1)
    launch_gn_rhs_diag<T>(dcp, drv, dE, cjE, n, dX, ldx, (int)kc, dP, ldp, 0);
  else if (trans == 0)
    launch_gn_rhs<T>(HsGnRows{drp, dci, dtp, 0}, dE, n, dX, ldx, (int)kc, dP, ldp, 0);
  else
    launch_gn_rhs<T>(HsGnRows{dcp, drv, nullptr, cjE}, dE, n, dX, ldx, (int)kc, dP, ldp, 0);
  HS_HIP(hipDeviceSynchronize());
  HS_HIP(hipMemcpy(P, dP, sizeof(T) * (size_t)ldp * kc, hipMemcpyDeviceToHost));
}
extern "C" int hsk_gn_rhs_d(int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* E, int pattern, const double* X, int64_t ldx, int64_t kc,
                            double* P, int64_t ldp) {
  HS_GUARD(gn_rhs_hook<double>(trans, n, colptr, rowval, E, pattern, X, ldx, kc, P, ldp));
}
extern "C" int hsk_gn_rhs_z(int trans, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* E, int pattern, const double* X, int64_t ldx, int64_t kc,
                            double* P, int64_t ldp) {
  HS_GUARD(gn_rhs_hook<cplx>(trans, n, colptr, rowval, (const cplx*)E, pattern, (const cplx*)X, ldx, kc, (cplx*)P, ldp));
}
template <class T>
static void gn_rowsq_hook(int64_t n, int64_t kc, const T* X, int64_t ldx, double* acc) {
  if (n < 1 || kc < 1 || kc > 4096 || !X || !acc || ldx < n) HS_FAIL(HS_ERR_ARGUMENT, 0, "hsk_gn_rowsq: n >= 1, kc in 1..4096, ldx >= n and non-null arrays required");
  need_device();
  HsDevBuf b("hsk_gn_rowsq");
  T* dX = b.get<T>((size_t)ldx * kc);
  double* da = b.get<double>((size_t)n);
  HS_HIP(hipMemcpy(dX, X, sizeof(T) * (size_t)ldx * kc, hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(da, acc, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  launch_gn_rowsq<T>(dX, ldx, n, (int)kc, da, 0);
  HS_HIP(hipDeviceSynchronize());
  HS_HIP(hipMemcpy(acc, da, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
}
extern "C" int hsk_gn_rowsq_d(int64_t n, int64_t kc, const double* X, int64_t ldx, double* acc) { HS_GUARD(gn_rowsq_hook<double>(n, kc, X, ldx, acc)); }
extern "C" int hsk_gn_rowsq_z(int64_t n, int64_t kc, const double* X, int64_t ldx, double* acc) { HS_GUARD(gn_rowsq_hook<cplx>(n, kc, (const cplx*)X, ldx, acc)); }

#include "hs_envelope.h"
static bool envelope_args_ok(int64_t n, const int64_t* colptr, const int64_t* rowval, const int32_t* fidx, int64_t ni, int64_t nb, const int32_t* firstL,
                             const int32_t* firstU) {
  if (n <= 0 || !colptr || !rowval || !fidx || ni < 0 || nb < 0 || ni + nb <= 0 || !firstL || !firstU) return false;
  for (int64_t p = 0; p < ni + nb; ++p)
    if (fidx[p] < 0 || fidx[p] >= n) return false;
  if (colptr[0] != 1) return false;
  for (int64_t j = 0; j < n; ++j)
    if (colptr[j + 1] < colptr[j]) return false;
  for (int64_t e = 0; e < colptr[n] - 1; ++e)
    if (rowval[e] < 1 || rowval[e] > n) return false;
  return true;
}
extern "C" int hsk_leaf_envelope(int64_t n, const int64_t* colptr, const int64_t* rowval, const int32_t* fidx, int64_t ni, int64_t nb, int32_t* firstL,
                                 int32_t* firstU) {
  if (!envelope_args_ok(n, colptr, rowval, fidx, ni, nb, firstL, firstU)) return -1;
  std::vector<int> where((size_t)n, -1);
  hs_leaf_envelope(colptr, rowval, fidx, (int)ni, (int)nb, where.data(), firstL, firstU);
  return 0;
}
extern "C" int hsk_branch_envelope(int64_t n, const int64_t* colptr, const int64_t* rowval, const int32_t* fidx, int64_t ni, int64_t nb, int64_t ni1,
                                   int64_t nb1, int32_t* firstL, int32_t* firstU) {
  if (!envelope_args_ok(n, colptr, rowval, fidx, ni, nb, firstL, firstU) || ni1 < 0 || ni1 > ni || nb1 < 0 || nb1 > nb) return -1;
  std::vector<int> where((size_t)n, -1);
  hs_branch_envelope(colptr, rowval, fidx, (int)ni, (int)nb, (int)ni1, (int)nb1, where.data(), firstL, firstU);
  return 0;
}

// the kernels of hs_mod_* (kernels_mod.hip) on host data (include/hs_kernels.h)
#include "hs_mod.h"

template <class T>
static void mod_inner_hook(int64_t n, int64_t k, int64_t m, const T* P, int64_t ldp, const T* Y, int64_t ldy, int conj, T* Tm, int64_t ldt) {
  if (n < 1 || k < 1 || k > HS_MOD_MAXRANK || m < 1 || m > HS_MOD_MAXCOLS || ldp < n || ldy < n || ldt < k || !P || !Y || !Tm)
    HS_FAIL(HS_ERR_ARGUMENT, 0, "hsk_mod_inner: n >= 1, k in 1..256, m in 1..64, leading dimensions and non-null arrays required");
  need_device();
  HsDevBuf b("hsk_mod_inner");
  T* dP = put_block<T>(b, P, ldp, n, k);
  T* dY = put_block<T>(b, Y, ldy, n, m);
  T* dT = put_block<T>(b, nullptr, k, k, m);
  T* dPart = put_block<T>(b, nullptr, 1, hs_mod_slabs(n) * k * m, 1);
  launch_mod_inner<T>(dP, n, dY, n, n, (int)k, (int)m, conj, dPart, dT, k, 0);
  HS_HIP(hipDeviceSynchronize());
  bring_block(Tm, ldt, dT, k, k, m);
}
extern "C" int hsk_mod_inner_d(int64_t n, int64_t k, int64_t m, const double* P, int64_t ldp, const double* Y, int64_t ldy, int conj, double* T, int64_t ldt) {
  HS_GUARD(mod_inner_hook<double>(n, k, m, P, ldp, Y, ldy, conj, T, ldt));
}
extern "C" int hsk_mod_inner_z(int64_t n, int64_t k, int64_t m, const double* P, int64_t ldp, const double* Y, int64_t ldy, int conj, double* T, int64_t ldt) {
  HS_GUARD(mod_inner_hook<cplx>(n, k, m, (const cplx*)P, ldp, (const cplx*)Y, ldy, conj, (cplx*)T, ldt));
}

template <class T>
static void mod_apply_hook(int64_t n, int64_t k, int64_t m, T* Y, int64_t ldy, const T* Z, int64_t ldz, const T* Tm, int64_t ldt, int conj) {
  if (n < 1 || k < 1 || k > HS_MOD_MAXRANK || m < 1 || m > HS_MOD_MAXCOLS || ldy < n || ldz < n || ldt < k || !Y || !Z || !Tm)
    HS_FAIL(HS_ERR_ARGUMENT, 0, "hsk_mod_apply: n >= 1, k in 1..256, m in 1..64, leading dimensions and non-null arrays required");
  need_device();
  HsDevBuf b("hsk_mod_apply");
  T* dY = put_block<T>(b, Y, ldy, n, m);
  T* dZ = put_block<T>(b, Z, ldz, n, k);
  T* dT = put_block<T>(b, Tm, ldt, k, m);
  launch_mod_apply<T>(dY, n, dZ, n, dT, k, n, (int)k, (int)m, conj, 0);
  HS_HIP(hipDeviceSynchronize());
  bring_block(Y, ldy, dY, n, n, m);
}
extern "C" int hsk_mod_apply_d(int64_t n, int64_t k, int64_t m, double* Y, int64_t ldy, const double* Z, int64_t ldz, const double* T, int64_t ldt, int conj) {
  HS_GUARD(mod_apply_hook<double>(n, k, m, Y, ldy, Z, ldz, T, ldt, conj));
}
extern "C" int hsk_mod_apply_z(int64_t n, int64_t k, int64_t m, double* Y, int64_t ldy, const double* Z, int64_t ldz, const double* T, int64_t ldt, int conj) {
  HS_GUARD(mod_apply_hook<cplx>(n, k, m, (cplx*)Y, ldy, (const cplx*)Z, ldz, (const cplx*)T, ldt, conj));
}

template <class T>
static void mod_gather_hook(int64_t n, int64_t k, int64_t m, const T* Y, int64_t ldy, const int64_t* J, T* Tm, int64_t ldt) {
  if (n < 1 || k < 1 || m < 1 || ldy < n || ldt < k || !Y || !J || !Tm)
    HS_FAIL(HS_ERR_ARGUMENT, 0, "hsk_mod_gather: n, k, m >= 1, leading dimensions and non-null arrays required");
  for (int64_t j = 0; j < k; ++j)
    if (J[j] < 0 || J[j] >= n) HS_FAIL(HS_ERR_DIMENSION, j, "hsk_mod_gather: J[%lld] = %lld outside 0:%lld", (long long)j, (long long)J[j], (long long)n - 1);
  need_device();
  HsDevBuf b("hsk_mod_gather");
  T* dY = put_block<T>(b, Y, ldy, n, m);
  int64_t* dJ = put_block<int64_t>(b, J, k, k, 1);
  T* dT = put_block<T>(b, nullptr, k, k, m);
  launch_mod_gather<T>(dT, k, dY, n, dJ, (int)k, (int)m, 0);
  HS_HIP(hipDeviceSynchronize());
  bring_block(Tm, ldt, dT, k, k, m);
}
extern "C" int hsk_mod_gather_d(int64_t n, int64_t k, int64_t m, const double* Y, int64_t ldy, const int64_t* J, double* T, int64_t ldt) {
  HS_GUARD(mod_gather_hook<double>(n, k, m, Y, ldy, J, T, ldt));
}
extern "C" int hsk_mod_gather_z(int64_t n, int64_t k, int64_t m, const double* Y, int64_t ldy, const int64_t* J, double* T, int64_t ldt) {
  HS_GUARD(mod_gather_hook<cplx>(n, k, m, (const cplx*)Y, ldy, J, (cplx*)T, ldt));
}

template <class T>
static void mod_cap_hook(int64_t k, int64_t m, const T* C, int64_t ldc, int op, T* Tm, int64_t ldt) {
  if (k < 1 || k > HS_MOD_MAXRANK || m < 1 || ldc < k || ldt < k || op < 0 || op > 2 || !C || !Tm)
    HS_FAIL(HS_ERR_ARGUMENT, 0, "hsk_mod_cap: k in 1..256, m >= 1, op in 0..2, leading dimensions and non-null arrays required");
  need_device();
  HsDevBuf b("hsk_mod_cap");
  T* dC = put_block<T>(b, C, ldc, k, k);
  T* dT = put_block<T>(b, Tm, ldt, k, m);
  int* dPiv = put_block<int>(b, nullptr, k + 1, k + 1, 1);
  launch_mod_cap_lu<T>(dC, (int)k, (int)k, dPiv, dPiv + k, 0);
  int info = 0;
  HS_HIP(hipMemcpy(&info, dPiv + k, sizeof(int), hipMemcpyDeviceToHost));
  if (info != 0) HS_FAIL(HS_ERR_SINGULAR, info, "SingularException(%d): hsk_mod_cap: zero pivot", info);
  launch_mod_cap_solve<T>(dC, (int)k, (int)k, dPiv, op, dT, k, (int)m, 0);
  HS_HIP(hipDeviceSynchronize());
  bring_block(Tm, ldt, dT, k, k, m);
}
extern "C" int hsk_mod_cap_d(int64_t k, int64_t m, const double* C, int64_t ldc, int op, double* T, int64_t ldt) {
  HS_GUARD(mod_cap_hook<double>(k, m, C, ldc, op, T, ldt));
}
extern "C" int hsk_mod_cap_z(int64_t k, int64_t m, const double* C, int64_t ldc, int op, double* T, int64_t ldt) {
  HS_GUARD(mod_cap_hook<cplx>(k, m, (const cplx*)C, ldc, op, (cplx*)T, ldt));
}

// ---- the pieces of hs_eigs_* (kernels_eigs.hip, hs_small_eig.h) on host data (tests/test_eigs_gpu.py, tests/test_eigs_host.py) ---------------
#include "hs_eigs.h"
#include "hs_small_eig.h"

template <class T>
static void eigs_rotate_hook(int64_t n, int64_t K, int64_t N, const T* V, int64_t ldv, const T* Q, int64_t ldq, int inplace, T* Out, int64_t ldo) {
  if (n < 1 || K < 1 || K > HS_EIGS_MAXBASIS || N < 1 || N > K || ldv < n || ldq < K || ldo < n || !V || !Q || !Out)
    HS_FAIL(HS_ERR_ARGUMENT, 0, "hsk_eigs_rotate: n >= 1, K in 1..256, N in 1..K, leading dimensions and non-null arrays required");
  need_device();
  HsDevBuf b("hsk_eigs_rotate");
  T* dV = put_block<T>(b, V, ldv, n, K);
  T* dQ = put_block<T>(b, Q, ldq, K, N);
  T* dO = inplace ? dV : put_block<T>(b, nullptr, n, n, N);
  launch_eigs_rotate<T>(dO, n, dV, n, dQ, K, n, (int)K, (int)N, 0);
  HS_HIP(hipDeviceSynchronize());
  bring_block(Out, ldo, dO, n, n, N);
}
extern "C" int hsk_eigs_rotate_d(int64_t n, int64_t K, int64_t N, const double* V, int64_t ldv, const double* Q, int64_t ldq, int inplace, double* Out, int64_t ldo) {
  HS_GUARD(eigs_rotate_hook<double>(n, K, N, V, ldv, Q, ldq, inplace, Out, ldo));
}
extern "C" int hsk_eigs_rotate_z(int64_t n, int64_t K, int64_t N, const double* V, int64_t ldv, const double* Q, int64_t ldq, int inplace, double* Out, int64_t ldo) {
  HS_GUARD(eigs_rotate_hook<cplx>(n, K, N, (const cplx*)V, ldv, (const cplx*)Q, ldq, inplace, (cplx*)Out, ldo));
}

template <class T>
static void eigs_chol_inv_hook(int64_t p, const T* G, int64_t ldg, T* R, T* Rinv, int* info) {
  if (p < 1 || p > HS_EIGS_MAXBLOCK || ldg < p || !G || !R || !Rinv || !info)
    HS_FAIL(HS_ERR_ARGUMENT, 0, "hsk_eigs_chol_inv: p in 1..64, ldg >= p and non-null arrays required");
  need_device();
  HsDevBuf b("hsk_eigs_chol_inv");
  T* dG = put_block<T>(b, G, ldg, p, p);
  T* dR = put_block<T>(b, nullptr, p, p, p);
  T* dRi = put_block<T>(b, nullptr, p, p, p);
  int* dInfo = put_block<int>(b, nullptr, 1, 1, 1);
  launch_eigs_chol_inv<T>(dG, (int)p, (int)p, dR, dRi, dInfo, 0);
  HS_HIP(hipDeviceSynchronize());
  HS_HIP(hipMemcpy(info, dInfo, sizeof(int), hipMemcpyDeviceToHost));
  HS_HIP(hipMemcpy(R, dR, sizeof(T) * (size_t)(p * p), hipMemcpyDeviceToHost));
  HS_HIP(hipMemcpy(Rinv, dRi, sizeof(T) * (size_t)(p * p), hipMemcpyDeviceToHost));
}
extern "C" int hsk_eigs_chol_inv_d(int64_t p, const double* G, int64_t ldg, double* R, double* Rinv, int* info) {
  HS_GUARD(eigs_chol_inv_hook<double>(p, G, ldg, R, Rinv, info));
}
extern "C" int hsk_eigs_chol_inv_z(int64_t p, const double* G, int64_t ldg, double* R, double* Rinv, int* info) {
  HS_GUARD(eigs_chol_inv_hook<cplx>(p, (const cplx*)G, ldg, (cplx*)R, (cplx*)Rinv, info));
}

template <class T>
static void eigs_coldot_hook(int64_t n, int64_t nc, const T* X, int64_t ldx, const T* Y, int64_t ldy, const int* pair, double* d) {
  bool ok = n >= 1 && nc >= 1 && nc <= HS_EIGS_MAXBASIS && ldx >= n && ldy >= n && X && Y && d;
  for (int64_t c = 0; ok && pair && c < nc; ++c)  // a pair is two adjacent columns of a Float64 block
    ok = pair[c] == 0 || (sizeof(T) == 8 && ((pair[c] == 1 && c + 1 < nc && pair[c + 1] == -1) || (pair[c] == -1 && c > 0 && pair[c - 1] == 1)));
  if (!ok) HS_FAIL(HS_ERR_ARGUMENT, 0, "hsk_eigs_coldot: n >= 1, nc in 1..256, leading dimensions >= n, non-null arrays and whole Float64 pairs required");
  need_device();
  HsDevBuf b("hsk_eigs_coldot");
  T* dX = put_block<T>(b, X, ldx, n, nc);
  T* dY = put_block<T>(b, Y, ldy, n, nc);
  int* dPair = pair ? put_block<int>(b, pair, nc, nc, 1) : nullptr;
  double* dPart = put_block<double>(b, nullptr, 1, hs_eigs_slabs(n) * nc, 1);
  double* dD = put_block<double>(b, nullptr, nc, nc, 1);
  launch_eigs_coldot<T>(dX, n, dY, n, dPair, n, (int)nc, dPart, dD, 0);
  HS_HIP(hipDeviceSynchronize());
  HS_HIP(hipMemcpy(d, dD, sizeof(double) * (size_t)nc, hipMemcpyDeviceToHost));
}
extern "C" int hsk_eigs_coldot_d(int64_t n, int64_t nc, const double* X, int64_t ldx, const double* Y, int64_t ldy, const int* pair, double* d) {
  HS_GUARD(eigs_coldot_hook<double>(n, nc, X, ldx, Y, ldy, pair, d));
}
extern "C" int hsk_eigs_coldot_z(int64_t n, int64_t nc, const double* X, int64_t ldx, const double* Y, int64_t ldy, const int* pair, double* d) {
  HS_GUARD(eigs_coldot_hook<cplx>(n, nc, (const cplx*)X, ldx, (const cplx*)Y, ldy, pair, d));
}

static void small_eig_hook(int64_t m, const double* H, int64_t ldh, double* w, double* Y, int64_t ldy) {
  if (m < 1 || m > HS_EIGS_MAXBASIS || ldh < m || ldy < m || !H || !w || !Y)
    HS_FAIL(HS_ERR_ARGUMENT, 0, "hsk_small_eig_z: m in 1..256, leading dimensions >= m and non-null arrays required");
  std::vector<hs_se::zc> Hc((size_t)(m * m));
  for (int64_t j = 0; j < m; ++j)
    for (int64_t i = 0; i < m; ++i) Hc[(size_t)(j * m + i)] = hs_se::zc(H[2 * (j * ldh + i)], H[2 * (j * ldh + i) + 1]);
  const int bad = hs_se::small_eig((int)m, Hc.data(), (int)m, (hs_se::zc*)w, (hs_se::zc*)Y, (int)ldy);
  if (bad) HS_FAIL(HS_ERR_SINGULAR, bad - 1, "hsk_small_eig_z: the QR iteration did not isolate eigenvalue %d", bad - 1);
}
extern "C" int hsk_small_eig_z(int64_t m, const double* H, int64_t ldh, double* w, double* Y, int64_t ldy) { HS_GUARD(small_eig_hook(m, H, ldh, w, Y, ldy)); }

// ---- hs_interface_matrix_*: the product S = P^T (L U) of a packed LU (kernels_interface.hip) on host data ------------------------------------
#include "hs_interface.h"
template <class T>
static void lu_product_hook(int64_t nb, const T* LF, int64_t ldl, const int32_t* rperm, T* S, int64_t lds, double* flops_out) {
  bool ok = nb >= 1 && nb <= (1 << 20) && LF && rperm && S && ldl >= nb && lds >= nb;
  if (ok) {
    std::vector<char> seen((size_t)nb, 0);
    for (int64_t i = 0; ok && i < nb; ++i) {
      ok = rperm[i] >= 0 && rperm[i] < nb && !seen[(size_t)rperm[i]];
      if (ok) seen[(size_t)rperm[i]] = 1;
    }
  }
  if (!ok) HS_FAIL(HS_ERR_ARGUMENT, 0, "hsk_lu_product: nb >= 1, non-null arrays, ldl >= nb, lds >= nb and rperm a permutation of 0..nb-1 required");
  need_device();
  const size_t nl = (size_t)ldl * (nb - 1) + nb, ns = (size_t)lds * (nb - 1) + nb;
  HsDevBuf b("hsk_lu_product");
  T* dL = b.get<T>(nl);
  T* dS = b.get<T>(ns);
  int* dp = b.get<int>((size_t)nb);
  HS_HIP(hipMemcpy(dL, LF, sizeof(T) * nl, hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(dS, S, sizeof(T) * ns, hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(dp, rperm, sizeof(int) * (size_t)nb, hipMemcpyHostToDevice));
  const double fl = launch_lu_product<T>((int)nb, dL, ldl, dp, dS, lds, 0);
  HS_HIP(hipDeviceSynchronize());
  HS_HIP(hipMemcpy(S, dS, sizeof(T) * ns, hipMemcpyDeviceToHost));
  if (flops_out) *flops_out = fl;
}
extern "C" int hsk_lu_product_d(int64_t nb, const double* LF, int64_t ldl, const int32_t* rperm, double* S, int64_t lds, double* flops_out) {
  HS_GUARD(lu_product_hook<double>(nb, LF, ldl, rperm, S, lds, flops_out));
}
extern "C" int hsk_lu_product_z(int64_t nb, const double* LF, int64_t ldl, const int32_t* rperm, double* S, int64_t lds, double* flops_out) {
  HS_GUARD(lu_product_hook<cplx>(nb, (const cplx*)LF, ldl, (const int32_t*)rperm, (cplx*)S, lds, flops_out));
}

// ---- hs_hss_logabsdet: the per-node determinant reduction of the ULV factors (kernels_selinv.hip: ulv_det_kernel) on host data ----------------
#include "hs_selinv.h"
template <class T>
static void ulv_det_hook(int64_t nnodes, const int64_t* ni, const int64_t* ld, const T* LU, const int32_t* rperm, double* out2, int32_t* flags3, double* res3) {
  bool ok = nnodes >= 1 && nnodes <= 65535 && ni && ld && out2 && flags3 && res3;
  size_t nlu = 0, np = 0;
  for (int64_t k = 0; ok && k < nnodes; ++k) {
    ok = ni[k] >= 0 && ni[k] <= (1 << 20) && ld[k] >= std::max<int64_t>(ni[k], 1);
    if (!ok) break;
    std::vector<char> seen((size_t)ni[k], 0);
    for (int64_t i = 0; ok && i < ni[k]; ++i) {
      const int32_t q = rperm[np + (size_t)i];
      ok = q >= 0 && q < ni[k] && !seen[(size_t)q];
      if (ok) seen[(size_t)q] = 1;
    }
    nlu += (size_t)ld[k] * (size_t)ni[k];
    np += (size_t)ni[k];
  }
  if (!ok || (nlu > 0 && (!LU || !rperm)))
    HS_FAIL(HS_ERR_ARGUMENT, 0, "hsk_ulv_det: 1..65535 nodes, ni >= 0, ld >= max(ni, 1), non-null arrays and every rperm a permutation of 0..ni-1 required");
  need_device();
  HsDevBuf b("hsk_ulv_det");
  T* dL = b.get<T>(std::max<size_t>(nlu, 1));
  int* dp = b.get<int>(std::max<size_t>(np, 1));
  LogdetFront* dn = b.get<LogdetFront>((size_t)nnodes);
  LogdetOut* dout = b.get<LogdetOut>((size_t)nnodes);
  if (nlu > 0) HS_HIP(hipMemcpy(dL, LU, sizeof(T) * nlu, hipMemcpyHostToDevice));
  if (np > 0) HS_HIP(hipMemcpy(dp, rperm, sizeof(int) * np, hipMemcpyHostToDevice));
  std::vector<LogdetFront> hn((size_t)nnodes);
  size_t ol = 0, op = 0;
  for (int64_t k = 0; k < nnodes; ++k) {
    hn[(size_t)k] = LogdetFront{dL + ol, dp + op, (int)ni[k], (int)ld[k]};
    ol += (size_t)ld[k] * (size_t)ni[k];
    op += (size_t)ni[k];
  }
  HS_HIP(hipMemcpy(dn, hn.data(), sizeof(LogdetFront) * (size_t)nnodes, hipMemcpyHostToDevice));
  HS_HIP(hipMemset(dout, 0xff, sizeof(LogdetOut) * (size_t)nnodes));  // an unwritten result shows
  launch_ulv_det<T>(dn, (int)nnodes, dout, 0);
  HS_HIP(hipGetLastError());
  HS_HIP(hipDeviceSynchronize());
  std::vector<LogdetOut> out((size_t)nnodes);
  HS_HIP(hipMemcpy(out.data(), dout, sizeof(LogdetOut) * (size_t)nnodes, hipMemcpyDeviceToHost));
  LogdetAcc acc;
  for (int64_t k = 0; k < nnodes; ++k) {
    const LogdetOut& o = out[(size_t)k];
    out2[2 * k] = o.logabs; out2[2 * k + 1] = o.angle;
    flags3[3 * k] = o.neg; flags3[3 * k + 1] = o.odd; flags3[3 * k + 2] = o.zero;
    acc.add(o);
  }
  acc.finish(sizeof(T) != sizeof(double), &res3[0], &res3[1], &res3[2]);
}
extern "C" int hsk_ulv_det_d(int64_t nnodes, const int64_t* ni, const int64_t* ld, const double* LU, const int32_t* rperm, double* out2, int32_t* flags3, double* res3) {
  HS_GUARD(ulv_det_hook<double>(nnodes, ni, ld, LU, rperm, out2, flags3, res3));
}
extern "C" int hsk_ulv_det_z(int64_t nnodes, const int64_t* ni, const int64_t* ld, const double* LU, const int32_t* rperm, double* out2, int32_t* flags3, double* res3) {
  HS_GUARD(ulv_det_hook<cplx>(nnodes, ni, ld, (const cplx*)LU, rperm, out2, flags3, res3));
}
