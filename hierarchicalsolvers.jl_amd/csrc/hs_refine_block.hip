// hs_refine_block.hip -- refined solves with error bounds for a block of right-hand sides in lockstep (hs_ldiv_refine_block_*,
// include/hs_solver.h).
//
// Column c gets the xGERFS iteration hs_ldiv_refine_* (hs_condest.hip) runs for B[:, c] alone -- the same start, residual, weights, guarded
// ratio, continuation rule and forward error bound -- but every application of op(F)^-1 is ONE hs_ldiv_block_dev_t_* call on all columns that
// are still active, so the factors are read once per chunk of columns and not once per column.
//
// Refinement: a correction is a gather of the residuals of the columns that go on into the leading slots of the correction block, one block
// solve, one axpy through the slot -> column map, one fused residual pass over op(A) for all active columns and one host synchronisation that
// reads nact ratios.  A column whose test ends is frozen: its x, berr and steps are no longer written.  X and B are never repacked.
//
// Forward error bound: after the refinement every column runs its own Higham-Tisseur Algorithm 2.4 on diag(v) op(F)^-H, t = min(2, n)
// columns and 5 iterations.  The estimator is est_run of hs_normest.h -- the kernels and the host loop hs_ldiv_refine_* runs with a single
// estimator -- with one estimator per column of the group and the block solve as its application of op(F)^-1: the active estimators share
// one block application of op_fwd(F)^-1 and one of op_adj(F)^-1 per iteration, and finished ones cost nothing.
//
// Determinism: no floating-point atomics; every reduction is per (workgroup, column) partials and one ordered final pass per column, so a
// column's results depend on neither its slot, the other columns, the group width nor compaction.
//
// Shared with hs_condest.hip through hs_condest.h: the op(F)^-1 code table, the rows of op(A) (op_rows) and the argument checks common to
// both entry points.  Not shared: the residual kernels -- the single path sums long rows by a wave butterfly, one order serves all rows here.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/hs_solver.h"
#include "hs_common.h"
#define HS_CONDEST_KERNELS
#include "hs_condest.h"  // switches fma contraction off for the rest of this file
#include "hs_normest.h"
#include "hs_block_apply.h"
#include "hs_solve_multi.h"

#define RB_T 2      // estimator columns per right-hand side: t = min(2, n)
#define RB_ITMAX 5  // estimator iterations

using namespace hs_ce;

namespace {

// ---- the fused block residual -----------------------------------------------------------------------------------------------------------
// For the nc active slots: R[:, s] = B[:, col[s]] - op(A) X[:, col[s]], W[:, s] = |B[:, col[s]]| + |op(A)| |X[:, col[s]]| (cabs1), with V:
// V[:, vcol[s]] = |r| + nz eps w (+ safe1 where w is tiny), and part[s * gridDim.x + blockIdx.x] = the workgroup's max of the guarded ratio.
// Row i of op(A) is row i of the CSR map (op = N) or column i of the CSC arrays (op = T, H: CJ conjugates on load).  A workgroup owns 256
// rows, lanes along rows, and walks the slots CB at a time: ptr / idx / val of the row tile are read once per CB columns; B, R, W, V are read
// and written contiguously per column; the gathers of x through idx are the uncoalesced part.  Per (row, column) the sum runs over the stored
// entries in order, without contraction: given the same x these are the bits of resid_kernel (hs_condest.hip).  One summation order serves
// every row length.
template <class T, bool CJ, int CB>
__global__ __launch_bounds__(256) void resid_block_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, const T* __restrict__ val,
                                                          const T* __restrict__ X, int64_t ldx, const T* __restrict__ B, int64_t ldb,
                                                          const int64_t* __restrict__ col, T* __restrict__ R, double* __restrict__ W, int64_t ldr,
                                                          double* __restrict__ V, const int* __restrict__ vcol, double* __restrict__ part, int64_t n,
                                                          int nc, ResidArgs g, double nzeps) {
  __shared__ double sh[CB][256];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  const bool live = i < n;
  int64_t e0 = 0, e1 = 0;
  if (live) {
    e0 = ptr[i];
    e1 = ptr[i + 1];
  }
  for (int c0 = 0; c0 < nc; c0 += CB) {
    T acc[CB];
    double wa[CB];
    const T* xp[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      const int cc = min(c0 + c, nc - 1);  // a ragged chunk recomputes its last column and does not store it
      xp[c] = X + (size_t)col[cc] * ldx;
      acc[c] = Scal<T>::zero();
      wa[c] = 0.0;
    }
    for (int64_t e = e0; e < e1; ++e) {
      const T a = cj_<CJ>(val[e]);
      const int32_t j = idx[e];
      const double aa = abs1_(a);
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        const T xv = xp[c][j];
        acc[c] = add_(acc[c], mul_(a, xv));
        wa[c] += aa * abs1_(xv);
      }
    }
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      const int cc = c0 + c;
      double ratio = 0.0;
      if (live && cc < nc) {
        const T bi = B[(size_t)col[cc] * ldb + i];
        const T ri = sub_(bi, acc[c]);
        const double wi = wa[c] + abs1_(bi);
        R[(size_t)cc * ldr + i] = ri;
        W[(size_t)cc * ldr + i] = wi;
        const double ra = abs1_(ri);
        ratio = berr_ratio(ra, wi, g);
        if (V) V[(size_t)vcol[cc] * ldr + i] = wi > g.safe2 ? ra + nzeps * wi : ra + nzeps * wi + g.safe1;
      }
      sh[c][tid] = ratio;
    }
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if (tid < st) {
#pragma unroll
        for (int c = 0; c < CB; ++c) sh[c][tid] = fmax(sh[c][tid], sh[c][tid + st]);
      }
      __syncthreads();
    }
    if (tid < CB && c0 + tid < nc) part[(size_t)(c0 + tid) * gridDim.x + blockIdx.x] = sh[tid][0];
    __syncthreads();
  }
}
// out[c] = max of part[c * cnt .. (c + 1) * cnt)   (one workgroup per column, fixed order)
__global__ __launch_bounds__(256) void colmax_final_kernel(const double* __restrict__ part, int64_t cnt, double* __restrict__ out) {
  __shared__ double sh[256];
  const double* p = part + (size_t)blockIdx.x * cnt;
  double m = 0.0;
  for (int64_t b = threadIdx.x; b < cnt; b += 256) m = fmax(m, p[b]);
  sh[threadIdx.x] = m;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + st]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}
// D[:, s] = R[:, src[s]]: the residuals of the columns that go on, compacted into the leading slots of the correction block
template <class T>
__global__ __launch_bounds__(256) void gather_kernel(const T* __restrict__ R, T* __restrict__ D, int64_t ld, const int* __restrict__ src, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) D[(size_t)blockIdx.y * ld + i] = R[(size_t)src[blockIdx.y] * ld + i];
}
// X[:, col[s]] += D[:, s]
template <class T>
__global__ __launch_bounds__(256) void axpy_map_kernel(T* __restrict__ X, int64_t ldx, const int64_t* __restrict__ col, const T* __restrict__ D, int64_t ld, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  T* x = X + (size_t)col[blockIdx.y] * ldx;
  x[i] = add_(x[i], D[(size_t)blockIdx.y * ld + i]);
}
// part[c * gridDim.x + b] = max over the workgroup's rows of cabs1(X[i, c])   (grid: nblk x columns)
template <class T>
__global__ __launch_bounds__(256) void absmax_cols_kernel(const T* __restrict__ X, int64_t ldx, int64_t n, double* __restrict__ part) {
  __shared__ double sh[256];
  const T* x = X + (size_t)blockIdx.y * ldx;
  double m = 0.0;
  for (int q = 0; q < CE_ROWS / 256; ++q) {
    const int64_t i = (int64_t)blockIdx.x * CE_ROWS + q * 256 + threadIdx.x;
    if (i < n) m = fmax(m, abs1_(x[i]));
  }
  sh[threadIdx.x] = m;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + st]);
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sh[0];
}

// ---- the driver ------------------------------------------------------------------------------------------------------------------------
enum { RI_SECONDS = 0, RI_SOLVES, RI_COL_APPS, RI_RESID, RI_MAX_ACTIVE, RI_GROUPS, RI_WORK_BYTES, RI_EST_COL_APPS };
thread_local double g_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};

template <class T>
struct Work {
  int64_t n = 0, G = 0;
  int nwg = 0;
  T *R = nullptr, *D = nullptr;
  double *W = nullptr, *V = nullptr, *part = nullptr, *ratio = nullptr;
  int64_t* col = nullptr;
  int *src = nullptr, *vcol = nullptr;
  EstWork<T, RB_T> est;  // one estimator per column of the group (ferr)
};
template <class T>
size_t bytes_per_column(int64_t n, bool ferr) {
  const size_t nwg = (size_t)nb256(n);
  size_t b = (size_t)n * (2 * sizeof(T) + 2 * sizeof(double)) + (nwg + 1) * sizeof(double) + sizeof(int64_t) + 2 * sizeof(int);
  if (ferr) b += EstWork<T, RB_T>::bytes_per_estimator(n);
  return b;
}

template <class T>
struct Driver {
  hs_handle* F;
  HsHandleView v;
  hipStream_t s;
  int trans;
  Work<T> ws;
  OpRows<T> A;  // the rows of op(A)
  HostIo io{F, s};

  void bsolve(int tr, T* X, int64_t ld, int64_t nc) {
    HS_CHECK(hs_block_apply_dev<T>(F, HS_VIA_BLOCK_T, tr, X, ld, (const T*)X, ld, v.n, nc, s));
    g_info[RI_SOLVES] += 1;
    g_info[RI_COL_APPS] += (double)nc;
  }
  void residual(const T* X, int64_t ldx, const T* B, int64_t ldb, int nact, bool weights) {
    constexpr int CB = sizeof(T) == 16 ? 4 : 8;
    auto k = A.cj ? resid_block_kernel<T, true, CB> : resid_block_kernel<T, false, CB>;
    hipLaunchKernelGGL(k, dim3((unsigned)ws.nwg), dim3(256), 0, s, A.ptr, A.idx, A.val, X, ldx, B, ldb, (const int64_t*)ws.col, ws.R, ws.W, ws.n,
                       weights ? ws.V : (double*)nullptr, (const int*)ws.vcol, ws.part, ws.n, nact, A.g, A.nz * CE_EPS);
    hipLaunchKernelGGL(colmax_final_kernel, dim3(nact), dim3(256), 0, s, (const double*)ws.part, (int64_t)ws.nwg, ws.ratio);
    g_info[RI_RESID] += 1;
  }

  // the columns g0 .. g0 + gc of the caller's block from start to finish
  void group(T* X, int64_t ldx, const T* B, int64_t ldb, int64_t g0, int gc, int64_t itmax, double* berr, double* ferr, int64_t* steps) {
    const int64_t n = ws.n;
    const unsigned gn = nb256(n);
    struct Col {
      int id;  // column within the group
      double lst = 3.0;
      int64_t cnt = 0;
    };
    std::vector<Col> cur((size_t)gc);
    std::vector<int64_t> hcol((size_t)gc);
    std::vector<int> hsrc((size_t)gc), hv((size_t)gc);
    for (int c = 0; c < gc; ++c) {
      cur[(size_t)c].id = c;
      hcol[(size_t)c] = g0 + c;
      hv[(size_t)c] = c;
    }
    io.upload(ws.col, hcol.data(), sizeof(int64_t) * (size_t)gc);
    io.upload(ws.vcol, hv.data(), sizeof(int) * (size_t)gc);
    // x = op(F) \ b
    HS_HIP(hipMemcpy2DAsync(X + (size_t)g0 * ldx, sizeof(T) * (size_t)ldx, B + (size_t)g0 * ldb, sizeof(T) * (size_t)ldb, sizeof(T) * (size_t)n, (size_t)gc,
                            hipMemcpyDeviceToDevice, s));
    bsolve(trans, X + (size_t)g0 * ldx, ldx, gc);
    for (;;) {
      const int nact = (int)cur.size();
      g_info[RI_MAX_ACTIVE] = std::max(g_info[RI_MAX_ACTIVE], (double)nact);
      residual(X, ldx, B, ldb, nact, ferr != nullptr);
      io.read(ws.ratio, (size_t)nact);
      std::vector<Col> next;
      for (int c = 0; c < nact; ++c) {
        Col q = cur[(size_t)c];
        const double be = io.hd[(size_t)c];
        if (be > CE_EPS && 2.0 * be <= q.lst && q.cnt < itmax) {
          q.lst = be;
          ++q.cnt;
          hsrc[next.size()] = c;
          hcol[next.size()] = g0 + q.id;
          hv[next.size()] = q.id;
          next.push_back(q);
        } else {  // frozen: its x, berr and steps are final
          berr[g0 + q.id] = be;
          steps[g0 + q.id] = q.cnt;
        }
      }
      if (next.empty()) break;
      const int nn = (int)next.size();
      io.upload(ws.src, hsrc.data(), sizeof(int) * (size_t)nn);
      io.upload(ws.col, hcol.data(), sizeof(int64_t) * (size_t)nn);
      io.upload(ws.vcol, hv.data(), sizeof(int) * (size_t)nn);
      // d = op(F) \ r for the columns that go on, in the leading slots; x += d
      hipLaunchKernelGGL(gather_kernel<T>, dim3(gn, nn), dim3(256), 0, s, (const T*)ws.R, ws.D, n, (const int*)ws.src, n);
      bsolve(trans, ws.D, n, nn);
      hipLaunchKernelGGL(axpy_map_kernel<T>, dim3(gn, nn), dim3(256), 0, s, X, ldx, (const int64_t*)ws.col, (const T*)ws.D, n, n);
      cur.swap(next);
    }
    if (ferr) estimate(X, ldx, g0, gc, ferr);
  }

  // ferr of the group's columns: || |op(A)^-1| v ||_Inf = || diag(v) op(A)^-H ||_1, estimated on B = diag(v) op(F)^-H, B^H = op(F)^-1 diag(v),
  // one estimator per column (t = min(2, n), 5 iterations) and one block solve per half-step for all of them, then / ||x||_Inf
  void estimate(const T* X, int64_t ldx, int64_t g0, int gc, double* ferr) {
    const int64_t n = ws.n;
    const int nblk = ws.est.nblk;
    std::vector<double> est((size_t)gc);
    est_run(io, ws.est, v.seed, adj(trans), ws.V, gc, RB_ITMAX, [&](int tr, T* blk, int64_t nc) {
      bsolve(tr, blk, n, nc);
      g_info[RI_EST_COL_APPS] += (double)nc;
    }, est.data());
    // ||x||_Inf of every column of the group
    hipLaunchKernelGGL(absmax_cols_kernel<T>, dim3(nblk, gc), dim3(256), 0, s, X + (size_t)g0 * ldx, ldx, n, ws.est.part);
    hipLaunchKernelGGL(colmax_final_kernel, dim3(gc), dim3(256), 0, s, (const double*)ws.est.part, (int64_t)nblk, ws.est.res);
    io.read(ws.est.res, (size_t)gc);
    for (int c = 0; c < gc; ++c) {
      const double xn = io.hd[(size_t)c];
      ferr[g0 + c] = xn != 0.0 ? est[(size_t)c] / xn : est[(size_t)c];
    }
  }
};

// G: the widest group (a multiple of the block solve's chunk width) whose workspace fits half of the free memory; HS_REFINE_BLOCK_GROUP overrides
int64_t group_width(size_t per_col, int64_t nrhs) {
  const int64_t KC = hs_ldiv_block_cols();
  const int64_t all = std::min<int64_t>((nrhs + KC - 1) / KC * KC, 4096);  // blockIdx.y carries up to 2 t^2 = 8 entries per column
  if (const char* e = getenv("HS_REFINE_BLOCK_GROUP")) {
    const long long w = atoll(e);
    if (w > 0) return std::min<int64_t>(all, (w + KC - 1) / KC * KC);
  }
  size_t fr = 0, tot = 0;
  HS_HIP(hipMemGetInfo(&fr, &tot));
  const int64_t fit = (int64_t)(fr / 2 / per_col);
  if (fit >= all) return all;
  const int64_t least = std::min<int64_t>(KC, nrhs);
  if (fit < least)
    HS_FAIL(HS_ERR_NOMEM, 0, "OutOfMemoryError: hs_ldiv_refine_block_* needs %zu bytes for one group of %lld columns, half of the free device memory is %zu bytes",
            per_col * (size_t)least, (long long)least, fr / 2);
  return std::max<int64_t>(fit / KC * KC, least);
}

template <class T>
void refine_block_dev(hs_handle* F, const HsHandleView& v, int trans, T* dX, int64_t ldx, const T* dB, int64_t ldb, int64_t nrhs, int64_t itmax, double* berr,
                      double* ferr, int64_t* steps, hipStream_t s, HsDevBuf& buf) {
  const int64_t n = v.n;
  Driver<T> d{F, v, s, trans};
  d.A = op_rows<T>(v, trans, s);
  Work<T>& ws = d.ws;
  const size_t per_col = bytes_per_column<T>(n, ferr != nullptr);
  ws.n = n;
  ws.G = std::min<int64_t>(group_width(per_col, nrhs), nrhs);
  ws.nwg = (int)nb256(n);
  const size_t G = (size_t)ws.G, blk = G * (size_t)n;
  ws.R = buf.get<T>(blk);
  ws.D = buf.get<T>(blk);
  ws.W = buf.get<double>(blk);
  ws.V = buf.get<double>(blk);
  ws.part = buf.get<double>(G * ws.nwg);
  ws.ratio = buf.get<double>(G);
  ws.col = buf.get<int64_t>(G);
  ws.src = buf.get<int>(G);
  ws.vcol = buf.get<int>(G);
  if (ferr) ws.est.alloc(buf, n, (int)std::min<int64_t>(RB_T, n), G);
  g_info[RI_WORK_BYTES] = (double)(per_col * G);
  HsEvents<2> ev;
  HsDrain drain{s};  // nothing in flight may outlive the workspace or the host sides of the uploads
  HS_HIP(hipEventRecord(ev[0], s));
  for (int64_t g0 = 0; g0 < nrhs; g0 += ws.G) {
    d.group(dX, ldx, dB, ldb, g0, (int)std::min<int64_t>(ws.G, nrhs - g0), itmax, berr, ferr, steps);
    g_info[RI_GROUPS] += 1;
  }
  HS_HIP(hipEventRecord(ev[1], s));
  HS_HIP(hipEventSynchronize(ev[1]));
  HS_CHECK(hs_handle_flow_check(F));
  float ms = 0.f;
  HS_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
  g_info[RI_SECONDS] = ms * 1e-3;
}

template <class T>
void refine_block_entry(hs_handle* F, int trans, T* X, int64_t ldx, const T* B, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax, double* berr, double* ferr,
                        int64_t* steps, bool on_device, void* stream) {
  const char* fn = on_device ? "hs_ldiv_refine_block_dev_*" : "hs_ldiv_refine_block_*";
  // refusals: before any device work, X untouched
  const HsHandleView v = hs_view_of(F, fn);
  check_refine_args<T>(fn, v, trans, X, ldx, B, ldb, n, nrhs, itmax, berr, steps);
  check_no_alias<T>(fn, X, ldx, B, ldb, nrhs);
  // what hs_ldiv_block_t_* refuses, whatever trans and ferr are (a host-side plan names these too)
  if (v.nranks > 1)
    HS_FAIL(HS_ERR_UNSUPPORTED, v.nranks, "%s: a factorization over %d ranks is not supported (single-rank factorizations only)", fn, v.nranks);
  if (v.t_refused_node >= 0 && !v.ulv)  // (hs_ulv_mode 1: the router below serves these fronts)
    HS_FAIL(HS_ERR_UNSUPPORTED, v.t_refused_node,
            "%s: node %d keeps its interior block D as an HSS matrix (hs_options.hss_d / mf = 2, 3): block solves and transposed ULV solves are not implemented; "
            "hs_ldiv_refine_* serves this handle with trans = 0 and without ferr",
            fn, v.t_refused_node);
  if (!v.device) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: handle holds a host-side plan only (hs_plan)", fn);
  if (!v.factored) HS_FAIL(HS_ERR_ARGUMENT, 0, "ArgumentError: %s: factorization is not complete", fn);
  // whatever else the block solve refuses is refused here: nothing is silently looped
  hs_block_probe_or_fail<T>(F, HS_VIA_BLOCK_T, trans, fn, "handle", "", false);
  for (double& x : g_info) x = 0.0;
  if (nrhs == 0) return;
  HsDevBuf buf("condest workspace");  // freed after the stream is drained, on every path
  if (on_device) return refine_block_dev<T>(F, v, trans, X, ldx, B, ldb, nrhs, itmax, berr, ferr, steps, (hipStream_t)stream, buf);
  hipStream_t s = v.stream;
  T* dX = buf.get<T>((size_t)n * nrhs);
  T* dB = buf.get<T>((size_t)n * nrhs);
  HsDrain drain{s};
  HS_HIP(hipMemcpy2DAsync(dB, sizeof(T) * n, B, sizeof(T) * ldb, sizeof(T) * n, nrhs, hipMemcpyHostToDevice, s));
  // results go to the caller's arrays only when the whole call succeeded
  std::vector<double> be((size_t)nrhs), fe((size_t)nrhs);
  std::vector<int64_t> st((size_t)nrhs);
  refine_block_dev<T>(F, v, trans, dX, n, dB, n, nrhs, itmax, be.data(), ferr ? fe.data() : nullptr, st.data(), s, buf);
  HS_HIP(hipMemcpy2DAsync(X, sizeof(T) * ldx, dX, sizeof(T) * n, sizeof(T) * n, nrhs, hipMemcpyDeviceToHost, s));
  HS_HIP(hipStreamSynchronize(s));
  std::copy(be.begin(), be.end(), berr);
  if (ferr) std::copy(fe.begin(), fe.end(), ferr);
  std::copy(st.begin(), st.end(), steps);
}

}  // namespace

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------------
extern "C" int hs_ldiv_refine_block_d(hs_handle* F, int trans, double* X, int64_t ldx, const double* B, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                                      double* berr, double* ferr, int64_t* steps) {
  HS_GUARD(refine_block_entry<double>(F, trans, X, ldx, B, ldb, n, nrhs, itmax, berr, ferr, steps, false, nullptr));
}
extern "C" int hs_ldiv_refine_block_z(hs_handle* F, int trans, double* X, int64_t ldx, const double* B, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                                      double* berr, double* ferr, int64_t* steps) {
  HS_GUARD(refine_block_entry<cplx>(F, trans, (cplx*)X, ldx, (const cplx*)B, ldb, n, nrhs, itmax, berr, ferr, steps, false, nullptr));
}
extern "C" int hs_ldiv_refine_block_dev_d(hs_handle* F, int trans, double* dX, int64_t ldx, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                                          double* berr, double* ferr, int64_t* steps, void* stream) {
  HS_GUARD(refine_block_entry<double>(F, trans, dX, ldx, dB, ldb, n, nrhs, itmax, berr, ferr, steps, true, stream));
}
extern "C" int hs_ldiv_refine_block_dev_z(hs_handle* F, int trans, double* dX, int64_t ldx, const double* dB, int64_t ldb, int64_t n, int64_t nrhs, int64_t itmax,
                                          double* berr, double* ferr, int64_t* steps, void* stream) {
  HS_GUARD(refine_block_entry<cplx>(F, trans, (cplx*)dX, ldx, (const cplx*)dB, ldb, n, nrhs, itmax, berr, ferr, steps, true, stream));
}
extern "C" int hs_ldiv_refine_block_info(double* out8) {
  if (!out8) {
    hs_set_error(HS_ERR_ARGUMENT, 0, "ArgumentError: hs_ldiv_refine_block_info: null argument");
    return HS_ERR_ARGUMENT;
  }
  for (int i = 0; i < 8; ++i) out8[i] = g_info[i];
  return HS_OK;
}
