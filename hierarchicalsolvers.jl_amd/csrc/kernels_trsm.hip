// kernels_trsm.hip -- the 256-row TRSM base case of the recursive LU as ONE in-place pass (Float64, gfx950).
//
//   X[r0 : r0 + wl, c0 : c1) <- inv256L[r0 / 256] * X,   wl = min(256, ni - r0),   for every front of a batch
//
// Sched::trsm256 used to issue this as two half products on the 128 x 128 GEMM tile (GemmOp::ainv 3: rows 128.. from all wl rows, then 4:
// rows 0..127 from the first min(128, wl)): one tile row per launch, X read 1.5 times, N / 128 workgroups per front and launch.  Here a
// workgroup owns a STRIP of NS = 32 columns of one front:
//   - it brings its wl x 32 piece of X into LDS once (image [n][LDX], the layout X has in memory; 64.5 KiB, two workgroups per CU),
//   - forms both halves from it -- rows 0..127 over k < min(128, wl), rows 128.. over all wl -- and
//   - stores the wl x 32 results.
// In place is safe in one launch: every load of X is complete before the barrier in front of the first MFMA, hence before the first store,
// and no other workgroup touches these columns (the argument resolve_op makes per tile row, kernels_gemm.hip).
// The inverse block (512 KiB, shared by the workgroups of a front, L2-resident) goes straight into the operand registers: a lane's 8 bytes
// per MFMA are inv[16 mt + (lane & 15), k + (lane >> 4)], a wave-load touches four 128-byte row segments, the next K-step's values are in
// flight while the MFMAs of the current one run.
//
// The stored values keep their bits: every output element takes one v_mfma_f64_16x16x4_f64 chain from a zero accumulator over the k range
// the half products give it, in ascending k and in the same groups of four (k - r0 = 4 q .. 4 q + 3 per instruction); the operands sit on
// the same sides (X on the MFMA's A side, the inverse on its B side).  Past the end of a ragged block (k >= wl) both operands are zero, as
// the tile kernels fill them.  Enveloped launches (GemmOp::env, leaf fronts): column c of X is zero above firstU[c], so a strip starts its K
// loop at the smallest firstU of ITS 32 columns (a multiple of 32 past r0) -- the K-steps it leaves out multiply exact zeros of X, the rule
// of gemm_dispatch_env per 128-column tile, applied per strip; a strip with nothing left is not run, and one whose first 128 rows are all
// structural zeros does not store them.
//
// MFMA layout as in kernels_gemm.hip ("transposed" issue): D[n][m], m = lane & 15 runs along the rows of X (contiguous in memory),
// n = (lane >> 4) + 4 reg.  The 16 m-tiles of a strip are dealt to the four waves as {w, w + 4} (rows 0..127, K <= 128) and
// {8 + w, 12 + w} (rows 128.., K <= 256), so every wave carries the same number of MFMAs.
#include <atomic>
#include <mutex>
#include <cstdlib>
#include "hs_common.h"

typedef double double4_t __attribute__((ext_vector_type(4)));

namespace {
constexpr int NS = 32;            // columns of a strip
constexpr int LDX = 258;          // doubles per column of the LDS image: 256 + 2, so that the 16 columns x 2 k of a half-wave's operand
                                  // ds_read_b64 fall on 32 different 8-byte bank pairs (258 n mod 32 = 2 n), and a column stays 16-byte aligned
constexpr int LDS_BYTES = NS * LDX * 8;
}  // namespace

// The m-tiles I0 .. I0 + NT - 1 of a wave (rows 16 mt[i] .. + 15 of the block) x the two 16-column halves of the strip over the K-steps
// [kb, ke) of 16: acc[i][j] += inv[rows of tile i, k] * X[k, columns of half j].  invl = inv + (lane & 15) + (lane >> 4) * 256, xl = xs + (lane & 15) * LDX + (lane >> 4).
template <int I0, int NT>
__device__ __forceinline__ void strip_ksteps(const double* __restrict__ invl, const double* xl, int kb, int ke, int wl, int l4, const int (&mt)[4],
                                             double4_t (&acc)[4][2]) {
  double af[NT][4], afn[NT][4];
  auto load_inv = [&](double (&a)[NT][4], int k0) {
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int k = k0 + 4 * ks;  // (+ l4 inside invl)
        const double v = gld(invl + 16 * mt[I0 + i] + (size_t)k * 256);  // always inside the 256 x 256 block
        a[i][ks] = (k + l4 < wl) ? v : 0.0;
      }
  };
  if (kb >= ke) return;
  load_inv(af, kb);
  for (int k0 = kb; k0 < ke; k0 += 16) {
    if (k0 + 16 < ke) load_inv(afn, k0 + 16);
    double bf[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) bf[j][ks] = xl[(16 * j) * LDX + k0 + 4 * ks];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) acc[I0 + i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(bf[j][ks], af[i][ks], acc[I0 + i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);  // one accumulator takes its four k-steps back to back (kernels_gemm.hip, "chained issue")
      }
    if (k0 + 16 < ke) {
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) af[i][ks] = afn[i][ks];
    }
  }
}

__global__ __launch_bounds__(256, 2) void trsm_strip_kernel(const NodeDesc<double>* __restrict__ nodes, GemmOp op) {
  extern __shared__ __attribute__((aligned(16))) double xs[];  // [NS][LDX]
  __builtin_amdgcn_s_setprio(2);
  const NodeDesc<double>* pn = nodes + blockIdx.y;
  double* cp;
  int ldc, crows, ccols;
  mat_of(pn, op.cmat, cp, ldc, crows, ccols);
  const int ni = pn->ni;
  const int wl = min(256, ni - op.r0);
  const int N = min(op.c1, ccols) - op.c0;
  const int n0 = blockIdx.x * NS;
  if (wl <= 0 || n0 >= N) return;  // (a front with ni <= r0 or fewer columns than the batch's widest: nothing of it is touched)
  const int ns = min(NS, N - n0);
  int dk = 0;
  if (op.env && pn->env) {
    const int* fU = pn->env + hs_env_block(pn->m - 1, ni) + 1;  // firstU follows the firstL entries of all blocks
    const int col0 = op.c0 + (op.cmat == HS_MAT_LF ? 0 : ni) + n0;
    const int kstart = hs_env_min(fU, ni, col0, col0 + ns);
    if (kstart - op.r0 >= wl) return;  // only exact zeros in these columns: zeros stay zeros
    dk = max(0, kstart - op.r0) & ~31;
  }
  const double* __restrict__ inv = pn->inv256L + (size_t)(op.r0 / 256) * 65536;
  double* X = cp + (size_t)op.r0 + (size_t)(op.c0 + n0) * ldc;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int kend = (wl + 15) & ~15;  // the K-steps run over [dk, kend): rows wl.. of the image are zero

  // X -> LDS.  A thread brings 16 row pairs: pair kp = tid & 127 of the columns (tid >> 7) + 2 i; a wave reads 1 KiB of one column.  Clamped
  // addresses and selects, no per-lane branches (a guarded load costs a memory round trip at every join).  All loads are issued before the
  // first LDS store.  An even wl: a pair is inside or outside as a whole, 16-byte loads; an odd one (the last block of a front with an odd
  // ni): two 8-byte loads per pair.
  {
    const int kp = tid & 127, nb = tid >> 7;
    const int k = 2 * kp;
    hs_d2u v[16];
    if (k >= dk && k < kend) {
      if (!(wl & 1)) {
        const double* src = X + min(k, wl - 2);
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = gld2(src + (size_t)min(nb + 2 * i, ns - 1) * ldc);
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const double* col = X + (size_t)min(nb + 2 * i, ns - 1) * ldc;
          v[i].x = gld(col + min(k, wl - 1));
          v[i].y = gld(col + min(k + 1, wl - 1));
        }
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const bool nok = nb + 2 * i < ns;
        hs_d2u w;
        w.x = (nok && k < wl) ? v[i].x : 0.0;
        w.y = (nok && k + 1 < wl) ? v[i].y : 0.0;
        *(hs_d2u*)(xs + (nb + 2 * i) * LDX + k) = w;
      }
    }
  }
  __syncthreads();

  // rows 0..127 (tiles w, w + 4) take k < min(128, wl); rows 128.. (tiles 8 + w, 12 + w) all of wl
  const double* invl = inv + l15 + (size_t)l4 * 256;
  const double* xl = xs + l15 * LDX + l4;
  const int mt4[4] = {wave, wave + 4, wave + 8, wave + 12};
  double4_t acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};
  const int k1 = min(128, kend);
  if (wl > 128) {
    strip_ksteps<0, 4>(invl, xl, dk, k1, wl, l4, mt4, acc);
    strip_ksteps<2, 2>(invl, xl, max(dk, 128), kend, wl, l4, mt4, acc);
  } else {
    strip_ksteps<0, 2>(invl, xl, dk, k1, wl, l4, mt4, acc);
  }

  // acc[i][j][r] -> X[16 mt4[i] + l15, 16 j + l4 + 4 r]: a half-wave stores 128 contiguous bytes of four columns
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int mm = 16 * mt4[i] + l15;
    if (mm >= wl || (i < 2 && dk >= 128)) continue;  // (rows 0..127 of a strip clipped past them: structural zeros, left alone)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int nn = 16 * j + l4 + 4 * r;
        if (nn < ns) gst(X + (size_t)mm + (size_t)nn * ldc, acc[i][j][r]);
      }
  }
}

// ------------------------------------------------------------------------------------------------
namespace {
std::atomic<int> g_strip_on{-1};  // -1: not read yet (HS_TRSM_STRIP, default on)
std::atomic<long long> g_strip_launches{0};
std::atomic<long long> g_half_launches{0};
}  // namespace
bool hs_trsm_strip_enabled() {
  int v = g_strip_on.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("HS_TRSM_STRIP");
    v = (e && e[0] == '0') ? 0 : 1;
    g_strip_on.store(v);
  }
  return v != 0;
}
extern "C" int hsk_trsm_strip_enable(int on) {  // returns the previous setting
  const int prev = hs_trsm_strip_enabled() ? 1 : 0;
  g_strip_on.store(on ? 1 : 0);
  return prev;
}
extern "C" long long hsk_trsm_strip_launches(int reset) {  // launches of trsm_strip_kernel since the last reset (each stands for an ainv 3 + 4 pair)
  return reset ? g_strip_launches.exchange(0) : g_strip_launches.load();
}

// the half products the schedule issues instead (Float64, lower: GemmOp::ainv 3 and 4), counted by Sched::trsm256
void hs_trsm_half_note() { g_half_launches.fetch_add(1, std::memory_order_relaxed); }
extern "C" long long hsk_trsm_half_launches(int reset) { return reset ? g_half_launches.exchange(0) : g_half_launches.load(); }

void launch_trsm_strip(const NodeDesc<double>* dnodes, int nbatch, int maxN, const GemmOp& op, hipStream_t s) {
  if (nbatch <= 0 || maxN <= 0) return;
  static std::once_flag once;  // > 64 KiB of LDS per workgroup needs the opt-in, once per process
  std::call_once(once, [] { (void)hipFuncSetAttribute((const void*)trsm_strip_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES); });
  g_strip_launches.fetch_add(1, std::memory_order_relaxed);
  hipLaunchKernelGGL(trsm_strip_kernel, dim3((maxN + NS - 1) / NS, nbatch), dim3(256), LDS_BYTES, s, dnodes, op);
}
