// kernels_gemm.hip -- FP64 / complex-FP64 MFMA GEMM for gfx950 (v_mfma_f64_16x16x4_f64).
//
// C (M x N) -= A (M x K) * B (K x N)   or   C = A * B, all column-major (Julia Matrix{T}).
// This is the dense contraction of the elimination: the Schur-complement update
// S = Abb - Abi*R (reference src/factorization.jl:40,72), the products inside blockfactor /
// blockldiv / blockrdiv (src/blockmatrix.jl:118,163-170,178-185) and every trailing update of the
// blocked interior LU that replaces the reference's `\` and `/`.
//
// Tiling (real): 128x128 output tile per 256-thread workgroup, 4 waves as 2(M) x 2(N), each wave
// 64x64 = 4x4 MFMA tiles of 16x16 (64 f64 accumulators = 128 VGPRs/lane, 2 workgroups per CU).
// K is consumed in steps of BK=16 staged through LDS ([k][m] / [k][n] images, row stride 144 so the
// two 16-lane halves of a ds_read_b64 land on disjoint bank halves); the next K-step's global
// loads are issued into registers before the MFMAs of the current one.
//
// The MFMA is issued "transposed": its A operand carries B's column index and its B operand A's
// row index, so that lane&15 runs along C's rows -- contiguous in column-major memory -- and every
// C load/store instruction touches four 128-byte row segments instead of sixteen 32-byte ones.
// f64 C/D map (cdna guide section 3): col = lane&15, row = (lane>>4) + 4*reg.
//
// Complex: planar split when staging (re / im images in LDS), 4 real MFMAs per k-step
// (re += ar*br - ai*bi, im += ar*bi + ai*br); 128x64 tile, wave tile 64x32.
#include <atomic>
#include <mutex>
#include <vector>
#include <algorithm>
#include <initializer_list>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hs_common.h"
#include "hs_envelope.h"

typedef double double4_t __attribute__((ext_vector_type(4)));
typedef hs_d2u double2_u;

// Tile geometry, one struct per element type: everything that sizes an LDS image, a stage or a launch is derived from these values.
// A K-step is BK = 16 wide; a stage holds the A image [k][LDA] followed by the B image(s).
template <class T>
struct TileCfg;
template <>
struct TileCfg<double> {
  static constexpr int BM = 128, BN = 128;  // output tile of the dense kernels (the skinny tiles cut 64 x 64 / 64 x 128 out of the same images)
  static constexpr int BK = 16;
  static constexpr int LDA = 144;  // 128 + 16: stride == 16 (mod 32) doubles => conflict-free ds_read_b64 across the two k rows of a half-wave
  static constexpr int LDB = 18;   // B image is [n][k] with 16 + 2 padding: ds_write_b128 of a k-pair row segment and the MFMA-operand ds_read_b64 are both conflict-free
  static constexpr int A_IMG = BK * LDA;                // doubles: the B image follows the A image of its stage
  static constexpr int STAGE = A_IMG + BN * LDB;        // register-staged tiles: As [BK][LDA] then Bs [BN][LDB]
  static constexpr int STAGE_LDS = A_IMG + BN * BK;     // direct-to-LDS tile: the B image is [n][BK], unpadded -- 18,432 + 16,384 bytes
  static constexpr int smem_doubles = 2 * STAGE;        // two stages
  static constexpr int smem_doubles_lds = 2 * STAGE_LDS;
};
template <>
struct TileCfg<cplx> {
  static constexpr int BM = 128, BN = 64;
  static constexpr int BK = 16;
  static constexpr int LDA = 144;  // planar A images [k][LDA], re then im
  static constexpr int LDB = 18;   // planar B images [n][k], 16 + 2 padding as for the real tile
  static constexpr int smem_doubles = 2 * BK * LDA + 2 * BN * LDB;  // one stage
};

// bijective XCD-aware remap of a 1-D block id (cdna guide section 5, "XCD swizzle must be bijective"):
// blocks b and b+8 share an XCD; give each XCD a contiguous chunk of tile ids so neighbouring tiles
// (which share A row-panels / B column-panels) hit the same L2.
__host__ __device__ inline int xcd_remap(int bid, int nwg) {
  int q = nwg >> 3, r = nwg & 7, x = bid & 7, o = bid >> 3;
  int base = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
  return base + o;
}
// The same for a front of a BATCHED launch (grid = tiles x fronts): the hardware deals workgroups to the XCDs round-robin over the LINEAR
// workgroup id blockIdx.x + gridDim.x * blockIdx.y, so block `bid` of front y sits on XCD (bid + shift) & 7 with shift = (gridDim.x * y) & 7.
// Round 2 assumed bid & 7 for every front: with gridDim.x not a multiple of 8 the chunks of every front but the first grouped tiles of
// DIFFERENT L2s.  Bijective on [0, nwg): XCD x owns the bids first_x, first_x + 8, ... and gets a contiguous chunk.
__host__ __device__ inline int xcd_remap_shift(int bid, int nwg, int shift) {
  if (shift == 0) return xcd_remap(bid, nwg);
  const int x = (bid + shift) & 7;
  int base = 0;
#pragma unroll
  for (int xx = 0; xx < 8; ++xx) {
    const int first = (xx - shift) & 7;                       // smallest bid on XCD xx
    const int cnt = first < nwg ? (nwg - first + 7) >> 3 : 0;  // bids of this front on XCD xx
    base += (xx < x) ? cnt : 0;
  }
  return base + ((bid - ((x - shift) & 7)) >> 3);
}

// tile id -> (tile_m, tile_n): walk column-panels of GROUP_M tiles so a group shares B panels and re-uses A panels
__host__ __device__ inline void tile_coords(int t, int tiles_m, int tiles_n, int& tm, int& tn) {
  const int GROUP_M = 8;
  int per_group = GROUP_M * tiles_n;
  int g = t / per_group;
  int first_m = g * GROUP_M;
  int gm = min(tiles_m - first_m, GROUP_M);
  int in_g = t - g * per_group;
  tm = first_m + in_g % gm;
  tn = in_g / gm;
}

// Balanced tile order of an enveloped plain update (GemmOp::order; HS_ENV_ORDER, DESIGN.md section 4 "Branch fronts").  The remap above hands
// every XCD the same NUMBER of tiles, a contiguous run of tile rows; under an envelope the K length of a tile depends on where it lies -- in a
// branch front [int1; int2 | bnd1; bnd2] the tiles of bnd1 x bnd1 run all of K, every other tile starts at ni1 -- so the XCDs that own the
// upper rows finish last.  The order sends tile row i to (i * s) mod T with s the integer nearest 0.618 T that is coprime to T (a bijection
// of [0, T)): any window of consecutive i lands spread over the whole row range, so every chunk holds about the same mix of long and short
// tiles.  The columns go through the same map: a chunk boundary that cuts a group of 8 tile rows cuts it by COLUMNS (tile_coords runs down
// the group column after column), and left alone one chunk would get the group's left, long columns and the next its right, short ones.
// The 8 tile rows of a group are still 8 rows and its columns still columns: co-resident workgroups share A row panels and B column panels
// in L2 as before.  T <= 8 (one group: nothing to deal) keeps s = 1.  Plain updates only: their tiles are independent of one another.
__host__ __device__ inline int env_order_stride(int T) {
  if (T <= 8) return 1;
  const int s0 = (T * 40503 + 32768) >> 16;  // 40503 / 65536 = 0.61803; T is a tile count, at most 2^15 (a front of 4 M rows) in all int products here
  for (int d = 0;; ++d)                      // ends at s = 1 at the latest (s0 - d >= 1 > 0 up to there)
    for (int s = s0 - d; s <= s0 + d; s += (d ? 2 * d : 1)) {
      int a = s, b = T;
      while (b) { const int r = a % b; a = b; b = r; }
      if (a == 1) return s;
    }
}
__host__ __device__ inline void env_order_apply(int& tm, int& tn, int tiles_m, int tiles_n, int sm, int sn) {
  if (sm > 1) tm = tm * sm % tiles_m;
  if (sn > 1) tn = tn * sn % tiles_n;
}

// K-sorted tile order of an enveloped plain update (GemmOp::order == 2; HS_ENV_ORDER=2, DESIGN.md section 4 "K-sorted order").  The balanced
// order above mixes long and short tiles among the 64 workgroups an XCD holds at a time on purpose; this one keeps tiles of one K start
// together.  Per front and launch env_perm_kernel sorts the tile rows by kr[i] = max(k0, min firstL over the rows of tile row i) and the tile
// columns by kc[j] likewise (stable, ascending; a row or column with nothing left counts as kend), so that the tile at sorted position
// (a, b) starts at max(kr, kc), monotone in a and in b.  The sorted grid is cut into UNITS of 8 sorted rows x 8 sorted columns; the whole
// units come first in the sequence of positions, heaviest first (unitperm: stable by the summed K starts of their 64 tiles), 64 positions
// each, column after column -- what tile_coords does inside a group; the right strip (fewer than 8 columns left) and the bottom strip (fewer
// than 8 rows) follow.  Block ids reach positions through env_phase_pos: whole rounds of 8 units are dealt one unit per XCD, back and forth
// (x, then 7 - x: under weights that fall along the sequence the XCD that got the heaviest unit of one round gets the lightest of the
// next), what is left -- fewer than 8 units and the strips -- position by position the same way (8 consecutive positions are one column
// of a unit: an XCD gets one sorted row of it in the even columns and the mirrored row in the odd ones, so its tiles of a unit still share
// an A row panel), and the last < 8 block ids one per XCD.  A rest of at most 256 positions -- a launch, or the end of one, that gives every
// CU at most one tile -- goes to the XCDs in contiguous chunks like a dense launch.
// Every step is a bijection, so the map is one for every tile count and shift.  A static map: no atomics, nothing shared between workgroups.
__host__ __device__ inline int env_rank(const int* keys, int n, int i) {  // position of element i in a stable ascending sort of keys[0, n)
  const int k = keys[i];
  int r = 0;
  for (int j = 0; j < n; ++j) r += (keys[j] < k || (keys[j] == k && j < i)) ? 1 : 0;
  return r;
}
// summed K starts of the 64 tiles of the unit (g, c), from the SORTED keys (each at most kend <= ni: the sum stays far below 2^31)
__host__ __device__ inline int env_unit_key(const int* skr, const int* skc, int g, int c) {
  int sum = 0;
  for (int a = 8 * g; a < 8 * g + 8; ++a)
    for (int b = 8 * c; b < 8 * c + 8; ++b) sum += skr[a] > skc[b] ? skr[a] : skc[b];
  return sum;
}
// block id -> position in the sequence; nfull = whole units of the tiling, shift as for xcd_remap_shift
__host__ __device__ inline int env_phase_pos(int bid, int ntiles, int nfull, int shift) {
  const int head = (nfull >> 3) << 9;  // whole rounds of 8 units; block ids [0, head) are exactly those whose rank on their XCD is below head / 8
  int b = bid, base = 0, lg = 6;
  if (bid >= head) {
    b = bid - head;  // (head is a multiple of 8: the XCD of b is still (b + shift) & 7)
    base = head;
    lg = 0;
    // (at most 256 positions left: a tile per CU, nothing to balance -- contiguous chunks, which keep tiles of one K start on one XCD)
    const int sub = ntiles - head <= 256 ? 0 : ((ntiles - head) >> 3) << 3;  // whole rounds of 8 positions
    if (b >= sub) return head + sub + xcd_remap_shift(b - sub, ntiles - head - sub, shift);
  }
  const int x = (b + shift) & 7, o = (b - ((x - shift) & 7)) >> 3;  // XCD and rank of the block id among those of its XCD
  const int r = o >> lg;
  return base + (((r << 3) + ((r & 1) ? 7 - x : x)) << lg) + (o & ((1 << lg) - 1));
}
// position -> sorted tile coordinates (a, b)
__host__ __device__ inline void env_phase_coords(int p, int tiles_m, int tiles_n, const uint16_t* unitperm, int& a, int& b) {
  const int gm = tiles_m >> 3, gn = tiles_n >> 3;
  if (p < 64 * gm * gn) {
    const int u = unitperm[p >> 6], q = p & 63;
    a = 8 * (u / gn) + (q & 7);
    b = 8 * (u % gn) + (q >> 3);
    return;
  }
  p -= 64 * gm * gn;
  const int wr = tiles_n - 8 * gn;  // right strip: sorted rows [0, 8 gm) x the last wr columns, a group of 8 rows at a time
  if (p < 8 * gm * wr) {
    const int g = p / (8 * wr), q = p - g * 8 * wr;
    a = 8 * g + (q & 7);
    b = 8 * gn + (q >> 3);
    return;
  }
  p -= 8 * gm * wr;
  const int hb = tiles_m - 8 * gm;  // bottom strip: the last hb sorted rows x every column
  a = 8 * gm + p % hb;
  b = p / hb;
}

// The block envelope of a leaf front (GemmOp::env, NodeDesc::env; hs_envelope.h) comes back in `e`: which of firstL / firstU says something
// about this product, and where C and the K index sit in the front.  gemm_dispatch_env clips every tile with it (the enveloped launches run
// in kernels of their own, gemm_op_env_kernel / trsm_inv_env_kernel; the dense kernels instantiate resolve_op<T, false>, which holds none of
// this).  What each form may skip:
//   plain update C -= L[rows, k] * U[k, cols]: L[r, k] = 0 for k < firstL[r] and U[k, c] = 0 for k < firstU[c], so the K loop of a tile starts
//     at the larger of the two minima over its rows / columns; a tile with nothing left subtracts an exact +0 from C and is not run at all.
//   ainv 1, 3, 4 (X <- inv(L block) * X, in place; X is a piece of U or U12): column c of X is zero above firstU[c], so the same clip by the
//     columns alone.  A tile with nothing left reads only zeros of X -- its own rows among them, as its K range covers the rows it writes --
//     and would store zeros over zeros; the tiles that do run read what they read before (nobody has written anything else), so the
//     read-all-of-K-before-the-stores ordering argument below is untouched.
//   ainv 7, 8, 16 + q (L_below <- A_below * inv(U_group), in place): row r of A_below is zero left of firstL[r], so the clip by the rows alone;
//     an empty tile has zero rows over the whole group, the product with the triangular inverse is zero, zeros stay (and raise no growth flag).
//   ainv 2, 5, 6 (X <- inv(U block) * X, backward substitution) fill upwards: no clip.
template <class T, bool ENV>
__device__ inline bool resolve_op(const NodeDesc<T>* pn, const GemmOp& op, GemmProb<T>& p, EnvClip* ep) {
  EnvClip e_unused;  // (ENV == false: every use below is compiled out)
  EnvClip& e = ENV ? *ep : e_unused;
  T *cp, *bp;
  int ldc, ldb, crows, ccols, brows, bcols;
  mat_of(pn, op.cmat, cp, ldc, crows, ccols);
  mat_of(pn, op.bmat, bp, ldb, brows, bcols);
  const int ni = pn->ni, ldl = pn->ldl;
  T* const LF = pn->LF;
  const int* env = nullptr;
  const int* envU = nullptr;
  if constexpr (ENV) {
    env = op.env ? pn->env : nullptr;
    envU = env ? env + hs_env_block(pn->m - 1, ni) + 1 : nullptr;  // firstU follows the firstL entries of all blocks
    e.fL = e.fU = nullptr;
    e.ni = ni;
    e.row0 = op.r0 + (op.cmat == HS_MAT_SB ? ni : 0);
    e.col0 = op.c0 + (op.cmat == HS_MAT_LF ? 0 : ni);
    e.kbase = op.k0;
  }
  if (op.ainv >= 16) {
    // The same product for tiles that are 64 columns wide (ComplexF64): column block q = ainv - 16 of the group, from the right (3, 2, 1, 0):
    //   L[r0.., k0+64q : k0+64q+64) <- A[r0.., k0 : k0+64(q+1)) * V[0 : 64(q+1), 64q : 64q+64)      (V = inv(U_group) is upper triangular)
    // One tile column per launch: a workgroup has read all of its K before it stores, no other workgroup touches its rows, and the blocks to the
    // LEFT of q -- the only columns block q reads besides its own -- are still the original A when block q runs.
    const int q = op.ainv - 16;
    const int wl = min(256, ni - op.k0);
    const int M = min(op.r1, crows) - op.r0;
    const int N = min(64, wl - 64 * q);
    if (wl <= 0 || M <= 0 || N <= 0 || q > 3) return false;
    const T* V = pn->inv256U + (size_t)(op.k0 / 256) * 65536;
    T* X = LF + (size_t)op.r0 + (size_t)op.k0 * ldl;
    p.A = X; p.B = V + (size_t)(64 * q) * 256; p.C = X + (size_t)(64 * q) * ldl;
    p.M = M; p.N = N; p.K = min(wl, 64 * (q + 1));
    p.lda = ldl; p.ldb = 256; p.ldc = ldl;
    p.flag = pn->growth;
    p.flag_rows = pn->pivrows - op.r0;
    if constexpr (ENV) e.fL = env;
    return true;
  }
  if (op.ainv >= 7) {
    // L[r0.., k0 : k0+wl) <- A[r0.., k0 : k0+wl) * inv(U[k0 : k0+wl, k0 : k0+wl)), in place as two products that read every column they
    // overwrite before their stores (one tile column each: N <= 128): 7 = columns 128.. from all wl columns (first), 8 = columns 0..127
    const int wl = min(256, ni - op.k0);
    const int M = min(op.r1, crows) - op.r0;
    if (wl <= 0 || M <= 0) return false;
    const T* V = pn->inv256U + (size_t)(op.k0 / 256) * 65536;
    T* X = LF + (size_t)op.r0 + (size_t)op.k0 * ldl;
    if (op.ainv == 7) {
      if (wl <= 128) return false;
      p.A = X; p.B = V + (size_t)128 * 256; p.C = X + (size_t)128 * ldl;
      p.M = M; p.N = wl - 128; p.K = wl;
    } else {
      p.A = X; p.B = V; p.C = X;
      p.M = M; p.N = min(128, wl); p.K = min(128, wl);
    }
    p.lda = ldl; p.ldb = 256; p.ldc = ldl;
    p.flag = pn->growth;
    p.flag_rows = pn->pivrows - op.r0;
    if constexpr (ENV) e.fL = env;
    return true;
  }
  if (op.ainv >= 3) {
    // 256-row TRSM base case X[r0:r0+256, c0:c1) <- inv256 * X, in place, as two half products that never read a row
    // another workgroup may already have overwritten (each has one tile row and reads all of K before its stores):
    //   lower (L): 3 = rows 128.. <- inv[128:256, 0:256] * X[0:256]   (first),  4 = rows 0..127 <- inv[0:128, 0:128] * X[0:128]
    //   upper (U): 5 = rows 0..127 <- inv[0:128, 0:256] * X[0:256]    (first),  6 = rows 128.. <- inv[128:256, 128:256] * X[128:256]
    const int wl = min(256, ni - op.r0);
    const int N = min(op.c1, ccols) - op.c0;
    if (wl <= 0 || N <= 0) return false;
    const bool up = op.ainv >= 5;
    const T* inv = (up ? pn->inv256U : pn->inv256L) + (size_t)(op.r0 / 256) * 65536;
    const bool second_half_rows = (op.ainv == 3 || op.ainv == 6);  // output rows 128..
    const bool full_k = (op.ainv == 3 || op.ainv == 5);
    const int ro = second_half_rows ? 128 : 0;
    const int M = min(128, wl - ro);
    if (M <= 0) return false;
    const int ko = (op.ainv == 6) ? 128 : 0;
    const int K = full_k ? wl : (op.ainv == 4 ? min(128, wl) : wl - 128);
    if (K <= 0) return false;
    p.A = inv + ro + (size_t)ko * 256;
    p.B = cp + (size_t)(op.r0 + ko) + (size_t)op.c0 * ldc;
    p.C = cp + (size_t)(op.r0 + ro) + (size_t)op.c0 * ldc;
    p.M = M; p.N = N; p.K = K;
    p.lda = 256; p.ldb = ldc; p.ldc = ldc;
    if constexpr (ENV)
      if (!up) { e.fU = envU; e.kbase = op.r0; }  // (ko == 0 for the lower forms)
    return true;
  }
  if (op.ainv) {  // X[r0:r0+w, c0:c1) <- inv(L11[r0/32]) * X, in place (one tile row, all of K is read before the stores)
    const int w = min(HS_PB, ni - op.r0);
    const int N = min(op.c1, ccols) - op.c0;
    if (w <= 0 || N <= 0) return false;
    p.A = (op.ainv == 2 ? pn->invU : pn->invL) + (size_t)(op.r0 / HS_PB) * HS_PB * HS_PB;  // 2: inverse of the UPPER diagonal block
    p.B = cp + (size_t)op.r0 + (size_t)op.c0 * ldc;
    p.C = cp + (size_t)op.r0 + (size_t)op.c0 * ldc;
    p.M = w; p.N = N; p.K = w;
    p.lda = HS_PB; p.ldb = ldc; p.ldc = ldc;
    if constexpr (ENV)
      if (op.ainv == 1) { e.fU = envU; e.kbase = op.r0; }
    return true;
  }
  int r1 = min(op.r1, crows), c1 = min(op.c1, ccols), k1 = min(op.k1, ni);
  int M = r1 - op.r0, N = c1 - op.c0, K = k1 - op.k0;
  if (M <= 0 || N <= 0 || K <= 0) return false;
  int aoff = (op.cmat == HS_MAT_SB) ? ni : 0;
  p.A = LF + (size_t)(op.r0 + aoff) + (size_t)op.k0 * ldl;
  p.B = bp + (size_t)op.k0 + (size_t)op.c0 * ldb;
  p.C = cp + (size_t)op.r0 + (size_t)op.c0 * ldc;
  p.M = M; p.N = N; p.K = K;
  p.lda = ldl; p.ldb = ldb; p.ldc = ldc;
  if constexpr (ENV) {
    e.fL = env;
    e.fU = envU;
  }
  return true;
}

// ------------------------------------------------------------------------------------------------
// real double
// ------------------------------------------------------------------------------------------------
// The pieces the real tiles share come first.  Left in copies ON PURPOSE, because the kernels sit at the register limit and the shared form
// made some kernel worse (figures: profiles/r17_gemm_refactor.txt): gemm_tile_d_lds keeps its own epilogue (with real_epilogue its kernels go
// from 195 / 198 to 211 / 222 VGPRs and run the Schur updates of Poisson 128^3 3-9 % slower, measured); the two 128 x 128 tiles keep their
// own MFMA chain (one chain function: 108 -> 112 and 92 -> 108 bytes of scratch in the enveloped kernels); the edge loads are written out
// in each load_tile (as a function they change the code of all five dense kernels).

// Register staging of one K-step, shared by the register-staged real tiles: a thread holds PA row pairs of A (k rows KA apart) and PB k-pairs
// of B (columns 32 apart); store() writes them into the LDS images As [k][LDA] / Bs [n][LDB] of a stage.
template <int PA, int KA, int PB>
struct RegStage {
  double2_u ra[PA], rb[PB];
  __device__ __forceinline__ void store(double* As, int a_k, int a_pair, int b_n, int b_kp) const {
    using G = TileCfg<double>;
    double* Bs = As + G::A_IMG;
#pragma unroll
    for (int i = 0; i < PA; ++i) {
      double* dst = As + (a_k + KA * i) * G::LDA + 2 * a_pair;
      dst[0] = ra[i].x;
      dst[1] = ra[i].y;
    }
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      double* dst = Bs + (b_n + 32 * i) * G::LDB + 2 * b_kp;  // 16-byte aligned: 144 n + 16 kp bytes
      dst[0] = rb[i].x;
      dst[1] = rb[i].y;
    }
  }
};

// C epilogue of the register-staged real tiles: acc[i][j][r] <-> C[mw + i*16 + l15][nw + j*16 + l4 + 4r], (mw, nw) the wave's corner of the tile.
// All loads of a row block are issued before the first store (the compiler cannot prove the C addresses distinct and would otherwise
// serialise load -> store -> load ...).  FLAG: the stored values may be multipliers (GemmProb::flag) and raise the growth flag.
template <int MI, int NJ, bool FLAG>
__device__ __forceinline__ void real_epilogue(const GemmProb<double>& p, const double4_t (&acc)[MI][NJ], int mw, int nw, int l15, int l4, bool minus) {
  const int M = p.M, N = p.N;
  double* __restrict__ C = p.C;
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int mm = mw + i * 16 + l15;
    const bool rok = mm < M;
    double cv[NJ][4];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int nn = nw + j * 16 + l4 + 4 * r;
        cv[j][r] = (minus && rok && nn < N) ? gld(C + (size_t)mm + (size_t)nn * p.ldc) : 0.0;
      }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int nn = nw + j * 16 + l4 + 4 * r;
        if (rok && nn < N) {
          // (value before address with the flag, address before value without: the order in which the tiles had it written out, which
          // the compiler's schedule follows -- every kernel keeps its code)
          if constexpr (FLAG) {
            const double v = minus ? (cv[j][r] - acc[i][j][r]) : acc[i][j][r];
            gst(C + (size_t)mm + (size_t)nn * p.ldc, v);
            if (p.flag && mm < p.flag_rows && !(fabs(v) <= HS_GROWTH_MAX)) *p.flag = 1;  // uniform null test; NaN counts
          } else {
            gst(C + (size_t)mm + (size_t)nn * p.ldc, minus ? (cv[j][r] - acc[i][j][r]) : acc[i][j][r]);
          }
        }
      }
  }
}

__device__ inline void gemm_tile_d(const GemmProb<double>& p, int tile_m, int tile_n, bool minus, double* smem) {
  using G = TileCfg<double>;
  constexpr int BM = G::BM, BN = G::BN, BK = G::BK, LDA = G::LDA, LDB = G::LDB, STAGE = G::STAGE;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int M = p.M, N = p.N, K = p.K;
  const double* __restrict__ A = p.A;
  const double* __restrict__ B = p.B;

  // staging coordinates
  const int a_pair = tid & 63;  // rows 2*a_pair, 2*a_pair+1
  const int a_k = tid >> 6;     // + 4*i
  const int b_kp = tid & 7;     // k = 2*b_kp, 2*b_kp+1
  const int b_n = tid >> 3;     // + 32*i

  RegStage<4, 4, 4> st;

  // Global -> register staging.  Interior tiles take 16-byte loads with no guards.  Edge tiles use
  // clamped 8-byte loads + selects: a per-lane `if (in range) load` compiles to a branch with an
  // s_waitcnt vmcnt(0) at every join, i.e. eight fully serialised memory round trips per K-step
  // (that cost 33 % of every wave's life in SQ_WAIT_ANY before this was restructured).
  // Ragged batches (fronts of one level differ in ni / nb) give EVERY front an edge tile in n: at the leaf level of Poisson 128^3 9-17 %
  // of all tiles, which the clamped 8-byte path made 4-5x slower than interior ones (the level ran at the rate of its bounding box).
  // The operands are independent: a tile whose rows are all inside takes the 16-byte A loads whatever its columns do, and for a full
  // K-step the B loads stay 16 bytes wide with the COLUMN clamped -- what lands in columns >= N only feeds accumulators that are
  // never stored (C[:, n] depends on B[:, n] alone).  Only a partial K-step (the last one of a tile) needs the zero-filling path.
  const bool rows_in = (m0 + BM <= M), rows_even = (M & 1) == 0;  // M >= 2 when even (M > 0)
  auto load_tile = [&](int k0) {
    const bool kfull = k0 + BK <= K;
    if ((rows_in || rows_even) && kfull) {  // an even row count: a row pair is inside or outside as a whole, outside pairs re-read the last one
#pragma unroll
      for (int i = 0; i < 4; ++i)
        st.ra[i] = gld2(A + (size_t)min(m0 + 2 * a_pair, M - 2) + (size_t)(k0 + a_k + 4 * i) * p.lda);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int kk = k0 + a_k + 4 * i, mm = m0 + 2 * a_pair;
        const double* col = A + (size_t)min(kk, K - 1) * p.lda;
        double x = gld(col + min(mm, M - 1)), y = gld(col + min(mm + 1, M - 1));
        const bool kok = kk < K;
        st.ra[i].x = (kok && mm < M) ? x : 0.0;
        st.ra[i].y = (kok && mm + 1 < M) ? y : 0.0;
      }
    }
    if (kfull) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        st.rb[i] = gld2(B + (size_t)(k0 + 2 * b_kp) + (size_t)min(n0 + b_n + 32 * i, N - 1) * p.ldb);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int nn = n0 + b_n + 32 * i, kk = k0 + 2 * b_kp;
        const double* col = B + (size_t)min(nn, N - 1) * p.ldb;
        double x = gld(col + min(kk, K - 1)), y = gld(col + min(kk + 1, K - 1));
        const bool nok = nn < N;
        st.rb[i].x = (nok && kk < K) ? x : 0.0;
        st.rb[i].y = (nok && kk + 1 < K) ? y : 0.0;
      }
    }
  };
  auto store_tile = [&](int stage) { st.store(smem + stage * STAGE, a_k, a_pair, b_n, b_kp); };

  double4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};

  const int l15 = lane & 15, l4 = lane >> 4;
  const int a_off = l4 * LDA + wm * 64 + l15;
  const int b_off = G::A_IMG + (wn * 64 + l15) * LDB + l4;

  // Two LDS stages, ONE barrier per K-step: while the MFMAs of stage `cur` run, the next tile's global
  // loads are in flight; they are written to the other stage right after the MFMAs (every wave finished
  // reading that stage before the previous barrier).
  load_tile(0);
  store_tile(0);
  __syncthreads();
  int cur = 0;
  for (int k0 = 0; k0 < K; k0 += BK) {
    const bool more = (k0 + BK) < K;
    if (more) load_tile(k0 + BK);
    const double* a_rd = smem + cur * STAGE + a_off;
    const double* b_rd = smem + cur * STAGE + b_off;
    // Chained issue: v_mfma_f64_16x16x4_f64 pays ~40 extra cycles whenever consecutive MFMAs use a
    // different accumulator (C read + D write through the register file); back-to-back MFMAs on the
    // SAME accumulator forward it inside the pipe (measured: 105 -> 74 cycles/MFMA at chain 4,
    // tools/mfma_f64_probe.hip).  So every accumulator takes all BK/4 k-steps of the tile in a row.
    // (Round 2: visiting all 16 accumulators per k-step instead measured the same -- 63.6 vs 64.4 TFLOP/s at 8192^3.)
    {
      double bf[4][BK / 4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int ks = 0; ks < BK / 4; ++ks) bf[j][ks] = b_rd[(j * 16) * LDB + ks * 4];
      double af[BK / 4];
#pragma unroll
      for (int ks = 0; ks < BK / 4; ++ks) af[ks] = a_rd[(ks * 4) * LDA];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        double afn[BK / 4];
        if (i < 3) {
#pragma unroll
          for (int ks = 0; ks < BK / 4; ++ks) afn[ks] = a_rd[(ks * 4) * LDA + (i + 1) * 16];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int ks = 0; ks < BK / 4; ++ks)
            // transposed issue: MFMA-A <- B data (n on the register/row axis), MFMA-B <- A data (m on lane&15)
            acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(bf[j][ks], af[ks], acc[i][j], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);  // keep the chain together: the scheduler must not interleave accumulators
        }
        if (i < 3) {
#pragma unroll
          for (int ks = 0; ks < BK / 4; ++ks) af[ks] = afn[ks];
        }
      }
    }
    if (more) store_tile(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

  real_epilogue<4, 4, true>(p, acc, m0 + wm * 64, n0 + wn * 64, l15, l4, minus);
}

// ------------------------------------------------------------------------------------------------
// real double, operands loaded STRAIGHT INTO LDS (global_load_lds, 16 bytes per lane): gemm_op_lds_kernel.  Tile, wave layout, BK, the two
// stages, the transposed MFMA issue, the order in which every accumulator takes its k-steps and the epilogue are those of gemm_tile_d, so
// every stored value keeps its bits; what is gone are the staging registers ra / rb and the LDS store pass behind the MFMAs.
// A wave-instruction writes 64 lanes x 16 B = 1 KiB at a wave-uniform LDS base, lane-linear; only the SOURCE address is per lane:
//   A image [k][LDA], as before: one instruction fills one k-row of 128 doubles (the 16 padding doubles of a row are never written or
//     read).  Wave w issues the k-rows w, w + 4, w + 8, w + 12; lane l brings the row pair 2l, 2l + 1, clamped to the last pair of A.
//   B image [n][BK], 128 B per column, no padding (a lane-linear write cannot skip any): the eight 16-byte k-pair chunks of column n sit at
//     chunk index c ^ ((n >> 1) & 7).  One instruction fills eight columns; the lane whose slot is (n, c') fetches chunk c' ^ ((n >> 1) & 7)
//     of column min(n0 + n, N - 1).  The operand ds_read_b64 of a half-wave (16 columns n, two k of one pair) then meets every chunk index
//     twice, at an even and an odd n (32 banks apart), with the two k in the two halves of the chunk: all 64 banks once.
// The launch must qualify (launch_gemm_op): K a multiple of BK, A and B 16-byte aligned with even leading dimensions -- the row pair
// (M - 1, M) of an odd M then lies inside A's column, and what it brings for row M feeds accumulators that are never stored.
// ------------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void* hs_lds_ptr;
// EDGE (gemm_op_lds_edge_kernel, gemm_op_env_lds_kernel): the same tile for a K that is no multiple of BK and for a problem that was
// shifted one row up to make A 16-byte aligned (edge_shift_rows).  Only the last, partial K-step differs: its k-rows of the A image and
// k-pair chunks of the B image with k >= K are filled with zeros by ordinary LDS stores, as gemm_tile_d fills them, and all four MFMA
// k-steps run -- every stored value keeps the bits gemm_op_kernel gives.  For A the choice is wave-uniform per k-row; for B it is per
// lane: a chunk below K takes the direct load, a chunk at or above K the zeros, and with an odd K the chunk (K - 1, K) an 8-byte load of
// B[K - 1] and a stored (v, 0).  Nothing is read at k >= K.  mlo = 1: row 0 of the shifted problem is not C's; it is neither loaded
// nor stored.
template <bool EDGE>
__device__ inline void gemm_tile_d_lds(const GemmProb<double>& p, int tile_m, int tile_n, bool minus, double* smem, int mlo) {
  using G = TileCfg<double>;
  constexpr int BM = G::BM, BN = G::BN, BK = G::BK, LDA = G::LDA, STAGE = G::STAGE_LDS;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int M = p.M, N = p.N, K = p.K;

  // per-lane sources of the first K-step; a K-step further is BK columns of A / BK doubles down B
  const double* a_src = p.A + (size_t)min(m0 + 2 * lane, (M - 1) & ~1) + (size_t)wave * p.lda;  // + 4 i lda
  const double* b_src[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = 8 * (wave + 4 * i) + (lane >> 3);
    b_src[i] = p.B + (size_t)(2 * ((lane & 7) ^ ((n >> 1) & 7))) + (size_t)min(n0 + n, N - 1) * p.ldb;
  }
  const size_t a_row4 = (size_t)4 * p.lda;
  auto issue_tile = [&](int k0, int stage) {
    double* As = smem + stage * STAGE;
    double* Bs = As + G::A_IMG;
    const double* a = a_src + (size_t)k0 * p.lda;
    if constexpr (EDGE) {
      if (k0 + BK > K) {  // the partial K-step (uniform over the workgroup)
        const double2_u zero2 = {0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          double* row = As + (wave + 4 * i) * LDA;
          if (k0 + wave + 4 * i < K)
            __builtin_amdgcn_global_load_lds((const void HS_AS_GLOBAL*)(a + i * a_row4), (hs_lds_ptr)row, 16, 0, 0);
          else
            *(double2_u*)(row + 2 * lane) = zero2;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int n = 8 * (wave + 4 * i) + (lane >> 3);
          const int kk = k0 + 2 * ((lane & 7) ^ ((n >> 1) & 7));  // this lane's slot holds k = kk, kk + 1
          double* blk = Bs + (wave + 4 * i) * (8 * BK);
          if (kk + 1 < K) {
            __builtin_amdgcn_global_load_lds((const void HS_AS_GLOBAL*)(b_src[i] + k0), (hs_lds_ptr)blk, 16, 0, 0);
          } else {
            double2_u v = zero2;
            if (kk < K) v.x = gld(b_src[i] + k0);  // kk == K - 1
            *(double2_u*)(blk + 2 * lane) = v;
          }
        }
        return;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_global_load_lds((const void HS_AS_GLOBAL*)(a + i * a_row4), (hs_lds_ptr)(As + (wave + 4 * i) * LDA), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_global_load_lds((const void HS_AS_GLOBAL*)(b_src[i] + k0), (hs_lds_ptr)(Bs + (wave + 4 * i) * (8 * BK)), 16, 0, 0);
  };

  double4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};

  const int l15 = lane & 15, l4 = lane >> 4;
  const int a_off = l4 * LDA + wm * 64 + l15;
  // B operand of k-step ks: k = l4 + 4 ks, chunk (k >> 1) ^ ((n >> 1) & 7) with (n >> 1) & 7 == l15 >> 1 for every j (n = wn 64 + j 16 + l15)
  int b_off[BK / 4];
#pragma unroll
  for (int ks = 0; ks < BK / 4; ++ks)
    b_off[ks] = G::A_IMG + (wn * 64 + l15) * BK + 2 * ((2 * ks + (l4 >> 1)) ^ (l15 >> 1)) + (l4 & 1);

  // Two LDS stages, ONE barrier per K-step: the loads of the next tile go into the other stage before the MFMAs of this one (every wave
  // finished reading that stage before the previous barrier) and are waited for by the barrier that ends the step.
  issue_tile(0, 0);
  __syncthreads();
  int cur = 0;
  for (int k0 = 0; k0 < K; k0 += BK) {
    if (k0 + BK < K) issue_tile(k0 + BK, cur ^ 1);
    const double* s_rd = smem + cur * STAGE;
    const double* a_rd = s_rd + a_off;
    {
      double bf[4][BK / 4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int ks = 0; ks < BK / 4; ++ks) bf[j][ks] = s_rd[b_off[ks] + (j * 16) * BK];
      double af[BK / 4];
#pragma unroll
      for (int ks = 0; ks < BK / 4; ++ks) af[ks] = a_rd[(ks * 4) * LDA];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        double afn[BK / 4];
        if (i < 3) {
#pragma unroll
          for (int ks = 0; ks < BK / 4; ++ks) afn[ks] = a_rd[(ks * 4) * LDA + (i + 1) * 16];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int ks = 0; ks < BK / 4; ++ks)
            // transposed issue, as in gemm_tile_d.  No sched_barrier behind the chain here: the source order already gives every accumulator
            // its k-steps in a row (and whatever the scheduler does, each accumulator still takes them in the same order: same bits), and
            // unpinned the compiler spreads the operand reads of the next row block under the MFMAs -- 195 instead of 214 VGPRs and
            // 3-6 % more TFLOP/s at every K
            acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(bf[j][ks], af[ks], acc[i][j], 0, 0, 0);
        }
        if (i < 3) {
#pragma unroll
          for (int ks = 0; ks < BK / 4; ++ks) af[ks] = afn[ks];
        }
      }
    }
    __syncthreads();
    cur ^= 1;
  }

  // epilogue: real_epilogue<4, 4, true> written out, plus the lower row bound of a shifted problem (see the top of this section)
  double* __restrict__ C = p.C;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int mm = m0 + wm * 64 + i * 16 + l15;
    const bool rok = EDGE ? (mm < M && mm >= mlo) : (mm < M);
    double cv[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int nn = n0 + wn * 64 + j * 16 + l4 + 4 * r;
        cv[j][r] = (minus && rok && nn < N) ? gld(C + (size_t)mm + (size_t)nn * p.ldc) : 0.0;
      }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int nn = n0 + wn * 64 + j * 16 + l4 + 4 * r;
        if (rok && nn < N) {
          const double v = minus ? (cv[j][r] - acc[i][j][r]) : acc[i][j][r];
          gst(C + (size_t)mm + (size_t)nn * p.ldc, v);
          if (p.flag && mm < p.flag_rows && !(fabs(v) <= HS_GROWTH_MAX)) *p.flag = 1;
        }
      }
  }
}

// ------------------------------------------------------------------------------------------------
// real double, SKINNY problems (the grouped products of the HSS module: a 64-row window against 2,048 sample columns, 64 x 64 Gram
// matrices over a long inner dimension, ...).  The same pipeline with a 64 x 128 or 64 x 64 tile: a lone workgroup pays 64 MFMAs per wave and
// K-step of the 128 x 128 tile (1.7 us) whether its rows exist or not -- half or three quarters of them multiply padding when M, N <= 64 --
// and these launches are latency chains of K/16 such steps, not throughput.  2 x 2 waves, wave tile (BMs/2) x (BNs/2).
// ------------------------------------------------------------------------------------------------
template <int BMs, int BNs>
__device__ inline void gemm_tile_s_d(const GemmProb<double>& p, int tile_m, int tile_n, bool minus, double* smem) {
  using G = TileCfg<double>;
  constexpr int BK = G::BK, LDA = G::LDA, LDB = G::LDB, STAGE = G::STAGE;
  constexpr int WM = BMs / 2, WN = BNs / 2, MI = WM / 16, NJ = WN / 16;
  constexpr int NP = BMs / 2, KA = 256 / NP, PA = BK / KA;  // A staging: row pairs, k rows per pass, passes
  constexpr int PB = BNs / 32;                               // B staging passes
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int m0 = tile_m * BMs, n0 = tile_n * BNs;
  const int M = p.M, N = p.N, K = p.K;
  const double* __restrict__ A = p.A;
  const double* __restrict__ B = p.B;
  const int a_pair = tid % NP, a_k = tid / NP;
  const int b_kp = tid & 7, b_n = tid >> 3;
  RegStage<PA, KA, PB> st;
  const bool interior = (m0 + BMs <= M) && (n0 + BNs <= N);
  auto load_tile = [&](int k0) {
    if (interior && k0 + BK <= K) {
#pragma unroll
      for (int i = 0; i < PA; ++i) st.ra[i] = gld2(A + (size_t)(m0 + 2 * a_pair) + (size_t)(k0 + a_k + KA * i) * p.lda);
#pragma unroll
      for (int i = 0; i < PB; ++i) st.rb[i] = gld2(B + (size_t)(k0 + 2 * b_kp) + (size_t)(n0 + b_n + 32 * i) * p.ldb);
    } else {
#pragma unroll
      for (int i = 0; i < PA; ++i) {
        const int kk = k0 + a_k + KA * i, mm = m0 + 2 * a_pair;
        const double* col = A + (size_t)min(kk, K - 1) * p.lda;
        double x = gld(col + min(mm, M - 1)), y = gld(col + min(mm + 1, M - 1));
        const bool kok = kk < K;
        st.ra[i].x = (kok && mm < M) ? x : 0.0;
        st.ra[i].y = (kok && mm + 1 < M) ? y : 0.0;
      }
#pragma unroll
      for (int i = 0; i < PB; ++i) {
        const int nn = n0 + b_n + 32 * i, kk = k0 + 2 * b_kp;
        const double* col = B + (size_t)min(nn, N - 1) * p.ldb;
        double x = gld(col + min(kk, K - 1)), y = gld(col + min(kk + 1, K - 1));
        const bool nok = nn < N;
        st.rb[i].x = (nok && kk < K) ? x : 0.0;
        st.rb[i].y = (nok && kk + 1 < K) ? y : 0.0;
      }
    }
  };
  auto store_tile = [&](int stage) { st.store(smem + stage * STAGE, a_k, a_pair, b_n, b_kp); };
  double4_t acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};
  const int l15 = lane & 15, l4 = lane >> 4;
  const int a_off = l4 * LDA + wm * WM + l15;
  const int b_off = G::A_IMG + (wn * WN + l15) * LDB + l4;
  load_tile(0);
  store_tile(0);
  __syncthreads();
  int cur = 0;
  for (int k0 = 0; k0 < K; k0 += BK) {
    const bool more = (k0 + BK) < K;
    if (more) load_tile(k0 + BK);
    const double* a_rd = smem + cur * STAGE + a_off;
    const double* b_rd = smem + cur * STAGE + b_off;
    {
      double bf[NJ][BK / 4], af[MI][BK / 4];
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int ks = 0; ks < BK / 4; ++ks) bf[j][ks] = b_rd[(j * 16) * LDB + ks * 4];
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int ks = 0; ks < BK / 4; ++ks) af[i][ks] = a_rd[(ks * 4) * LDA + i * 16];
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
#pragma unroll
          for (int ks = 0; ks < BK / 4; ++ks) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(bf[j][ks], af[i][ks], acc[i][j], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (more) store_tile(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }
  real_epilogue<MI, NJ, false>(p, acc, m0 + wm * WM, n0 + wn * WN, l15, l4, minus);
}

// ------------------------------------------------------------------------------------------------
// complex double (planar split in LDS)
// ------------------------------------------------------------------------------------------------
__device__ inline void gemm_tile_z(const GemmProb<cplx>& p, int tile_m, int tile_n, bool minus, double* smem) {
  using G = TileCfg<cplx>;
  constexpr int BM = G::BM, BN = G::BN, BK = G::BK, LDA = G::LDA, LDB = G::LDB;
  double* Ar = smem;
  double* Ai = Ar + BK * LDA;
  double* Br = Ai + BK * LDA;
  double* Bi = Br + BN * LDB;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int M = p.M, N = p.N, K = p.K;
  const cplx* __restrict__ A = p.A;
  const cplx* __restrict__ B = p.B;

  // A tile 128 x 16 complex: thread -> row (tid&127), k = (tid>>7) + 2*i, i<8
  const int a_m = tid & 127, a_k = tid >> 7;
  // B tile 16 x 64 complex: thread -> k = tid&15, n = (tid>>4) + 16*i, i<4
  const int b_k = tid & 15, b_n = tid >> 4;
  double2_u ra[8], rb[4];

  // branch-free staging (clamped address + select), see gemm_tile_d
  auto load_tile = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int kk = k0 + a_k + 2 * i, mm = m0 + a_m;
      double2_u v = gld2(A + (size_t)min(mm, M - 1) + (size_t)min(kk, K - 1) * p.lda);
      const bool ok = kk < K && mm < M;
      ra[i].x = ok ? v.x : 0.0;
      ra[i].y = ok ? v.y : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int kk = k0 + b_k, nn = n0 + b_n + 16 * i;
      double2_u v = gld2(B + (size_t)min(kk, K - 1) + (size_t)min(nn, N - 1) * p.ldb);
      const bool ok = kk < K && nn < N;
      rb[i].x = ok ? v.x : 0.0;
      rb[i].y = ok ? v.y : 0.0;
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      int o = (a_k + 2 * i) * LDA + a_m;
      Ar[o] = ra[i].x;
      Ai[o] = ra[i].y;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int o = (b_n + 16 * i) * LDB + b_k;
      Br[o] = rb[i].x;
      Bi[o] = rb[i].y;
    }
  };

  double4_t accr[4][2], acci[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      accr[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};
      acci[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};
    }
  const int l15 = lane & 15, l4 = lane >> 4;
  const int a_off = l4 * LDA + wm * 64 + l15;
  const int b_off = (wn * 32 + l15) * LDB + l4;

  load_tile(0);
  store_tile();
  __syncthreads();
  for (int k0 = 0; k0 < K; k0 += BK) {
    const bool more = (k0 + BK) < K;
    if (more) load_tile(k0 + BK);
    {  // chained issue, see gemm_tile_d: each accumulator takes its 2 * BK/4 MFMAs back to back
      double bfr[2][BK / 4], bfi[2][BK / 4];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int ks = 0; ks < BK / 4; ++ks) {
          bfr[j][ks] = Br[b_off + (j * 16) * LDB + ks * 4];
          bfi[j][ks] = Bi[b_off + (j * 16) * LDB + ks * 4];
        }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        double afr[BK / 4], afi[BK / 4];
#pragma unroll
        for (int ks = 0; ks < BK / 4; ++ks) {
          afr[ks] = Ar[a_off + (ks * 4) * LDA + i * 16];
          afi[ks] = Ai[a_off + (ks * 4) * LDA + i * 16];
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
          for (int ks = 0; ks < BK / 4; ++ks) {
            accr[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(bfr[j][ks], afr[ks], accr[i][j], 0, 0, 0);
            accr[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(bfi[j][ks], afi[ks], accr[i][j], 0, 0, 1);  // blgp bit 0 = NEG(src A) on f64 MFMA: re -= bi*ai
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int ks = 0; ks < BK / 4; ++ks) {
            acci[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(bfi[j][ks], afr[ks], acci[i][j], 0, 0, 0);
            acci[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(bfr[j][ks], afi[ks], acci[i][j], 0, 0, 0);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    __syncthreads();
    if (more) {
      store_tile();
      __syncthreads();
    }
  }
  cplx* __restrict__ C = p.C;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int mm = m0 + wm * 64 + i * 16 + l15;
    const bool rok = mm < M;
    double2_u cv[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int nn = n0 + wn * 32 + j * 16 + l4 + 4 * r;
        double2_u o = {0.0, 0.0};
        if (minus && rok && nn < N) o = gld2(C + (size_t)mm + (size_t)nn * p.ldc);
        cv[j][r] = o;
      }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int nn = n0 + wn * 32 + j * 16 + l4 + 4 * r;
        if (rok && nn < N) {
          double2_u v = {accr[i][j][r], acci[i][j][r]};
          if (minus) {
            v.x = cv[j][r].x - v.x;
            v.y = cv[j][r].y - v.y;
          }
          gst2(C + (size_t)mm + (size_t)nn * p.ldc, v);
          if (p.flag && mm < p.flag_rows && !(fabs(v.x) + fabs(v.y) <= HS_GROWTH_MAX)) *p.flag = 1;  // uniform null test; NaN counts (GemmOp::ainv 16..19: the values ARE multipliers)
        }
      }
  }
}

// Device-side flop count of the plain updates (hsk_op_flops): the K-steps the tiles really ran, added up by gemm_op_env_kernel while
// GemmOp::count is set -- launch_gemm_op then sends EVERY plain update there, dense ones included; gemm_op_kernel itself never counts
__device__ double g_op_flops;

// Which real tile a dispatch runs (ComplexF64 has one tile, gemm_tile_z, whatever the tag)
enum class Tile {
  Reg,      // operands staged through registers: gemm_tile_d
  Lds,      // operands loaded straight into LDS: gemm_tile_d_lds<false> (gemm_op_lds_kernel)
  LdsEdge,  // the same for a ragged K and a problem shifted one row up: gemm_tile_d_lds<true> (gemm_op_lds_edge_kernel, gemm_op_env_lds_kernel)
};
// The tile walk of a workgroup over the tiles of an M x N problem: tile counts, the XCD remap and the tile order.  A launch may have fewer
// workgroups than tiles (GemmOp::cap, enveloped launches): each workgroup then walks the tiles bid, bid + gridDim.x, ... -- with gridDim.x a
// multiple of 8 they all stay in the same XCD chunk of the remap.
template <class T>
struct TileWalk {
  int tiles_m, tiles_n, ntiles, shift;
  __device__ __forceinline__ TileWalk(int M, int N) {
    tiles_m = (M + TileCfg<T>::BM - 1) / TileCfg<T>::BM, tiles_n = (N + TileCfg<T>::BN - 1) / TileCfg<T>::BN;
    ntiles = tiles_m * tiles_n;
    shift = (int)((gridDim.x * blockIdx.y) & 7u);
  }
  __device__ __forceinline__ void coords(int bid, int& tm, int& tn) const {
    int t = xcd_remap_shift(bid, ntiles, (gridDim.x & 7u) ? shift : 0);  // (a walking workgroup keeps its XCD only when gridDim.x is a multiple of 8: then shift == 0)
    tile_coords(t, tiles_m, tiles_n, tm, tn);
  }
  __device__ __forceinline__ bool more(int bid) const { return bid + (int)gridDim.x < ntiles; }  // this workgroup has a tile after `bid`
};
template <class T, Tile TILE = Tile::Reg>
__device__ inline void gemm_dispatch(const GemmProb<T>& p, bool minus, double* smem, int mlo = 0) {
  const TileWalk<T> w(p.M, p.N);
  for (int bid = blockIdx.x; bid < w.ntiles; bid += gridDim.x) {
    int tm, tn;
    w.coords(bid, tm, tn);
    if constexpr (sizeof(T) == 16)
      gemm_tile_z(p, tm, tn, minus, smem);
    else if constexpr (TILE == Tile::Reg)
      gemm_tile_d(p, tm, tn, minus, smem);
    else
      gemm_tile_d_lds<TILE == Tile::LdsEdge>(p, tm, tn, minus, smem, mlo);
    if (w.more(bid)) __syncthreads();  // the next tile re-uses the LDS stages
  }
}

// The same loop for a launch whose fronts may carry a block envelope (gemm_op_env_kernel, trsm_inv_env_kernel below)
template <class T, Tile TILE = Tile::Reg>  // (enveloped launches have no Tile::Lds twin: launch_gemm_op sends them to the edge tile)
__device__ inline void gemm_dispatch_env(GemmProb<T>& p, bool minus, double* smem, const EnvClip* e, int count, int order, int mlo = 0,
                                         const uint32_t* pm = nullptr) {
  const TileWalk<T> w(p.M, p.N);
  // (GemmOp::order: the strides of the balanced order, once per front and uniform over the workgroup; 1, 1 is the order of the dense launches)
  const int sm = (order && !pm) ? env_order_stride(w.tiles_m) : 1, sn = (order && !pm) ? env_order_stride(w.tiles_n) : 1;
  bool ran = false;
  for (int bid = blockIdx.x; bid < w.ntiles; bid += gridDim.x) {
    int tm, tn;
    if (pm) {  // the K-sorted order: the front's table (env_perm_slot), one read per tile
      const uint32_t t = pm[bid];
      tm = (int)(t & 0xffffu);
      tn = (int)(t >> 16);
    } else {
      w.coords(bid, tm, tn);
      env_order_apply(tm, tn, w.tiles_m, w.tiles_n, sm, sn);
    }
    int dk = 0;
    {
      // Leaf front with a block envelope: everything here is uniform over the workgroup and done once per tile; the tile code is handed a
      // problem whose A, B and K are already shifted.  dk is a multiple of 32: the 16-byte operand loads keep their alignment and the
      // remaining BK-steps hold the same k as before, in the same order -- every stored value keeps its bits.
      const int m_lo = tm * TileCfg<T>::BM, n_lo = tn * TileCfg<T>::BN;
      const int m_hi = min(m_lo + TileCfg<T>::BM, p.M), n_hi = min(n_lo + TileCfg<T>::BN, p.N);
      if (e->fL || e->fU) {
        dk = hs_env_kstart(*e, m_lo, m_hi, n_lo, n_hi) - e->kbase;
        if (dk >= p.K) continue;  // only exact zeros left: nothing to subtract / zeros stay zeros (no LDS touched, so no barrier either)
      }
      if (count && threadIdx.x == 0)  // (test hook: one atomic per tile, i.e. per workgroup unless the launch walks)
        atomicAdd(&g_op_flops, (sizeof(T) == 16 ? 8.0 : 2.0) * (double)(m_hi - m_lo) * (double)(n_hi - n_lo) * (double)(p.K - dk));
    }
    const size_t da = (size_t)dk * p.lda;  // the problem is shifted in place and put back after the tile (a shifted copy next to the original
    p.A += da;                             // keeps both alive in scalar registers through the tile code)
    p.B += dk;
    p.K -= dk;
    if (ran) __syncthreads();  // this tile re-uses the LDS stages of the last one that ran
    ran = true;
    if constexpr (sizeof(T) == 16)
      gemm_tile_z(p, tm, tn, minus, smem);
    else if constexpr (TILE == Tile::Reg)
      gemm_tile_d(p, tm, tn, minus, smem);
    else
      gemm_tile_d_lds<true>(p, tm, tn, minus, smem, mlo);
    p.A -= da;
    p.B -= dk;
    p.K += dk;
  }
}

// What a kernel of launch_gemm_op does before its tiles: raise the wave priority (always for the 32-row solves; for a plain update when
// GemmOp::prio asks -- look-ahead panel work sharing CUs with the big trailing update) and resolve the op for this front.  (The enveloped
// kernels write the two steps out: their form filter sits between them, and wherever else it was put their code changed.)
template <class T, bool TRSM>
__device__ __forceinline__ bool op_prologue(const NodeDesc<T>* __restrict__ nodes, const GemmOp& op, GemmProb<T>& p) {
  if (TRSM || op.prio) __builtin_amdgcn_s_setprio(2);
  return resolve_op<T, false>(nodes + blockIdx.y, op, p, nullptr);
}
template <class T>
__global__ __launch_bounds__(256, 2) void gemm_op_kernel(const NodeDesc<T>* __restrict__ nodes, GemmOp op) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  GemmProb<T> p;
  if (!op_prologue<T, false>(nodes, op, p)) return;
  gemm_dispatch<T>(p, true, smem);
}
// The plain dense update again with its operands loaded straight into LDS (gemm_tile_d_lds): launch_gemm_op sends a launch here when
// every front of the batch qualifies (K a multiple of 16, 16-byte aligned A and B) and HS_GEMM_LDS is on.  A kernel of its own: the
// register-staged kernels keep their code and with it their register allocation.
template <class T>
__global__ __launch_bounds__(256, 2) void gemm_op_lds_kernel(const NodeDesc<T>* __restrict__ nodes, GemmOp op) {
  static_assert(sizeof(T) == 8, "real double only");
  extern __shared__ __attribute__((aligned(16))) double smem[];
  GemmProb<T> p;
  if (!op_prologue<T, false>(nodes, op, p)) return;
  gemm_dispatch<T, Tile::Lds>(p, true, smem);
}
// A plain update whose A sits at an odd row (r0, plus ni when C is SB) has an A that is 8 but not 16 bytes off a 16-byte boundary.  The
// edge kernels then run the problem one row higher: A' = A - 1 row, C' = C - 1 row, M' = M + 1 -- the extra row lies inside LF's column
// (arow - 1 >= 0), its accumulators are never stored and C' row 0 is never touched (mlo = 1 in the tile).  Every entry of C still takes
// its k-steps in the same order.  Decided per front from the resolved pointer, so a batch may mix odd and even ni.
__device__ inline int edge_shift_rows(GemmProb<double>& p) {
  if (!((uintptr_t)p.A & 15)) return 0;
  p.A -= 1;
  p.C -= 1;
  p.M += 1;
  p.flag_rows += 1;
  return 1;
}
// The plain dense update with direct-to-LDS loads for the launches gemm_op_lds_kernel does not take: a K that is no multiple of 16
// and / or an odd row offset of A (hs_gemm_lds_route: HS_GEMM_ROUTE_EDGE).  Again a kernel of its own, with its own instantiation of the tile.
template <class T>
__global__ __launch_bounds__(256, 2) void gemm_op_lds_edge_kernel(const NodeDesc<T>* __restrict__ nodes, GemmOp op) {
  static_assert(sizeof(T) == 8, "real double only");
  extern __shared__ __attribute__((aligned(16))) double smem[];
  GemmProb<T> p;
  if (!op_prologue<T, false>(nodes, op, p)) return;
  const int mlo = edge_shift_rows(p);
  gemm_dispatch<T, Tile::LdsEdge>(p, true, smem, mlo);
}
// The TRSM base case (X <- inv(diagonal block) * X, in place) runs the same tile code under its own name, so that
// profiles separate the trailing updates (gemm_op_kernel: the flops) from the 32-row solves (latency).
template <class T>
__global__ __launch_bounds__(256, 2) void trsm_inv_kernel(const NodeDesc<T>* __restrict__ nodes, GemmOp op) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  GemmProb<T> p;
  if (!op_prologue<T, true>(nodes, op, p)) return;
  gemm_dispatch<T>(p, false, smem);
}
// The table of this front for the K-sorted order (GemmOp::order == 2): block id -> tile, tile row in the low and tile column in the high
// half of a word.  Null: the launch runs another order, or the front did not fit its slot and takes the balanced order (the flag
// env_perm_kernel left).
__device__ __forceinline__ const uint32_t* env_perm_slot(const GemmOp& op) {
  if (op.order != 2) return nullptr;
  const uint16_t* pm = op.perm + (size_t)blockIdx.y * hs_env_perm_stride(op.perm_slot);
  return pm[0] ? (const uint32_t*)(pm + 2) : nullptr;
}
// The tables themselves, written on the stream of the update in front of it (launch_gemm_op): grid (workgroups, fronts).  The op is resolved
// as the update resolves it (edge: the update runs gemm_op_env_lds_kernel, which tiles a front whose A sits at an odd row from one row
// higher), the keys are those hs_env_kstart gives the tiles, split into their row and column part.  A front without tables has constant
// keys and gets the identity.  Every workgroup of a front does the sorts for itself in LDS (rank sorts: tile counts are at most
// HS_ENV_PERM_MAX, a few hundred at the root of the benchmark) and fills its share of the block id -> tile table; the first also leaves the
// permutations behind the table.  A front whose tables are not written -- more tile rows or columns than the slot holds, or fewer tiles than
// min_tiles -- gets the flag 0 and runs the balanced order.  gridx: gridDim.x of the update, which decides the XCD a front's first block id sits on (TileWalk).
template <class T>
__global__ __launch_bounds__(256) void env_perm_kernel(const NodeDesc<T>* __restrict__ nodes, GemmOp op, int edge, int gridx, int min_tiles) {
  constexpr int MAXT = HS_ENV_PERM_MAX, MAXG = MAXT / 8;
  __shared__ int key[2 * MAXT], skey[2 * MAXT], ukey[MAXG * MAXG];
  __shared__ uint16_t rowperm[MAXT], colperm[MAXT], unitperm[MAXG * MAXG];
  const int slot = op.perm_slot;
  uint16_t* const pm = op.perm + (size_t)blockIdx.y * hs_env_perm_stride(slot);
  GemmProb<T> p;
  EnvClip e;
  const bool ok = resolve_op<T, true>(nodes + blockIdx.y, op, p, &e);
  if constexpr (sizeof(T) == 8)
    if (ok && edge) e.row0 -= edge_shift_rows(p);
  const int tiles_m = ok ? (p.M + TileCfg<T>::BM - 1) / TileCfg<T>::BM : 0, tiles_n = ok ? (p.N + TileCfg<T>::BN - 1) / TileCfg<T>::BN : 0;
  // (min_tiles: a front with fewer tiles keeps the balanced order -- hs_env_perm_min_tiles)
  if (!ok || tiles_m > slot || tiles_n > slot || slot > MAXT || tiles_m * tiles_n < min_tiles) {
    if (threadIdx.x == 0 && blockIdx.x == 0) pm[0] = 0;
    return;
  }
  const int kend = e.kbase + p.K;
  for (int i = threadIdx.x; i < tiles_m; i += blockDim.x) {
    const int lo = i * TileCfg<T>::BM, hi = min(lo + TileCfg<T>::BM, p.M);
    const int v = e.fL ? hs_env_min(e.fL, e.ni, e.row0 + lo, e.row0 + hi) : e.kbase;
    key[i] = min(max(v, e.kbase), kend);
  }
  for (int j = threadIdx.x; j < tiles_n; j += blockDim.x) {
    const int lo = j * TileCfg<T>::BN, hi = min(lo + TileCfg<T>::BN, p.N);
    const int v = e.fU ? hs_env_min(e.fU, e.ni, e.col0 + lo, e.col0 + hi) : e.kbase;
    key[MAXT + j] = min(max(v, e.kbase), kend);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < tiles_m; i += blockDim.x) {
    const int r = env_rank(key, tiles_m, i);
    rowperm[r] = (uint16_t)i;
    skey[r] = key[i];
  }
  for (int j = threadIdx.x; j < tiles_n; j += blockDim.x) {
    const int r = env_rank(key + MAXT, tiles_n, j);
    colperm[r] = (uint16_t)j;
    skey[MAXT + r] = key[MAXT + j];
  }
  __syncthreads();
  const int gn = tiles_n >> 3, nfull = (tiles_m >> 3) * gn, ntiles = tiles_m * tiles_n;
  for (int u = threadIdx.x; u < nfull; u += blockDim.x) ukey[u] = env_unit_key(skey, skey + MAXT, u / gn, u % gn);
  __syncthreads();
  for (int u = threadIdx.x; u < nfull; u += blockDim.x) unitperm[env_rank(ukey, nfull, u)] = (uint16_t)u;
  __syncthreads();
  const int shift = (gridx & 7) ? (int)(((unsigned)gridx * blockIdx.y) & 7u) : 0;  // as TileWalk has it
  uint32_t* const tab = (uint32_t*)(pm + 2);
  for (int bid = blockIdx.x * blockDim.x + threadIdx.x; bid < ntiles; bid += gridDim.x * blockDim.x) {
    int a, b;
    env_phase_coords(env_phase_pos(bid, ntiles, nfull, shift), tiles_m, tiles_n, unitperm, a, b);
    tab[bid] = (uint32_t)rowperm[a] | ((uint32_t)colperm[b] << 16);
  }
  if (blockIdx.x == 0) {
    uint16_t* const out = pm + 2 + 2 * slot * slot;
    for (int i = threadIdx.x; i < tiles_m; i += blockDim.x) out[i] = rowperm[i];
    for (int j = threadIdx.x; j < tiles_n; j += blockDim.x) out[slot + j] = colperm[j];
    for (int u = threadIdx.x; u < nfull; u += blockDim.x) out[2 * slot + u] = unitperm[u];
    if (threadIdx.x == 0) pm[0] = 1;
  }
}

// The two kernels again for launches with GemmOp::env (batches of leaf fronts under optimistic pivoting) or GemmOp::count: kernels of their
// own, so that the dense launches above -- every level but the leaves, 87 % of the factorization -- keep the code they had: with the
// clip inside gemm_op_kernel<double> its register allocation moved and the dense levels of Poisson 128^3 ran 10-14 % slower.
template <class T>
__global__ __launch_bounds__(256, 2) void gemm_op_env_kernel(const NodeDesc<T>* __restrict__ nodes, GemmOp op) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  GemmProb<T> p;
  EnvClip e;
  if (op.prio) __builtin_amdgcn_s_setprio(2);
  if (op.ainv) return;  // (launch_gemm_op sends those to trsm_inv_env_kernel: lets the compiler drop the in-place forms and their growth check here)
  if (!resolve_op<T, true>(nodes + blockIdx.y, op, p, &e)) return;
  // (no K-sorted order here: launch_gemm_op gives the launches of this kernel -- ComplexF64, and Float64 with an odd k0 or counted -- the
  // balanced order, so that the register-staged tiles keep the code they had.  With the table read in it the Float64 kernel went from 26 to
  // 27 spilled VGPRs, the ComplexF64 one from 13 to 18 spilled SGPRs and helmholtz3d_64 ran 8 % slower on the balanced order itself.)
  gemm_dispatch_env<T>(p, true, smem, &e, op.count, op.order);
}
// The enveloped plain update on the edge tile (batches of leaf fronts whose k0 is even): the clip moves A and B by a multiple of 32
// columns / rows, which keeps their alignment and the K tail.  A shifted front looks its rows up one position higher (row0 - 1): the
// clip of a tile can only start earlier, over exact zeros of L.  The price of the shift: tile row 0 of a shifted front with C in SB begins
// at front row ni - 1, the last interior block, whose firstL is its own diagonal -- the clip of those tiles starts no later than
// 32 (ceil(ni / 32) - 1) and they are never skipped, where the unshifted tiling may skip them or start later.  Not measured on its own (at
// Poisson 128^3 8 of the 512 leaves have an odd ni); the host accounting (Sched::gemm) keeps describing the unshifted tiling.
// Counted launches (GemmOp::count) stay on gemm_op_env_kernel.
template <class T>
__global__ __launch_bounds__(256, 2) void gemm_op_env_lds_kernel(const NodeDesc<T>* __restrict__ nodes, GemmOp op) {
  static_assert(sizeof(T) == 8, "real double only");
  extern __shared__ __attribute__((aligned(16))) double smem[];
  GemmProb<T> p;
  EnvClip e;
  if (op.prio) __builtin_amdgcn_s_setprio(2);
  if (op.ainv) return;
  if (!resolve_op<T, true>(nodes + blockIdx.y, op, p, &e)) return;
  const int mlo = edge_shift_rows(p);
  e.row0 -= mlo;
  gemm_dispatch_env<T, Tile::LdsEdge>(p, true, smem, &e, 0, op.order, mlo, env_perm_slot(op));
}
template <class T>
__global__ __launch_bounds__(256, 2) void trsm_inv_env_kernel(const NodeDesc<T>* __restrict__ nodes, GemmOp op) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  GemmProb<T> p;
  EnvClip e;
  __builtin_amdgcn_s_setprio(2);
  if (!op.ainv) return;  // (plain updates run as gemm_op_env_kernel)
  if (!resolve_op<T, true>(nodes + blockIdx.y, op, p, &e)) return;
  gemm_dispatch_env<T>(p, false, smem, &e, 0, 0);  // (in place, one tile row or column per launch: the order of the dense launches)
}

// Accounting of the grouped products (hs_probs_stats, include/hs_kernels.h): the descriptors live on the device, so the kernel itself adds
// the real flops of every problem (one atomic per problem and launch, only while the accounting is on: bit 1 of `minus`)
__device__ double g_probs_flops;
template <class T>
__global__ __launch_bounds__(256, 2) void gemm_probs_kernel(const GemmProb<T>* __restrict__ probs, int minus) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  GemmProb<T> p = probs[blockIdx.y];
  if (p.M <= 0 || p.N <= 0) return;
  if ((minus & 2) && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&g_probs_flops, (sizeof(T) == 16 ? 8.0 : 2.0) * p.M * (double)p.N * p.K);
  gemm_dispatch<T>(p, (minus & 1) != 0, smem);
}
// Problem lists that cannot fill the chip with 128 x 128 tiles (launch_gemm_probs decides): what such a launch costs is the LENGTH of a
// tile's K loop (1.7 us per 16 columns for a lone workgroup), so the work is cut into 64 x 64 tiles -- a quarter of the MFMAs per K-step,
// four times the workgroups -- and 64 x 128 for a problem with M <= 64 < N.
__global__ __launch_bounds__(256, 2) void gemm_probs_skinny_kernel(const GemmProb<double>* __restrict__ probs, int minus) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  GemmProb<double> p = probs[blockIdx.y];
  if (p.M <= 0 || p.N <= 0) return;
  if ((minus & 2) && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&g_probs_flops, 2.0 * p.M * (double)p.N * p.K);
  minus &= 1;
  if (p.M <= 64 && p.N > 64) {
    const int tn_ = (p.N + 127) / 128;
    for (int bid = blockIdx.x; bid < tn_; bid += gridDim.x) {
      gemm_tile_s_d<64, 128>(p, 0, bid, minus != 0, smem);
      if (bid + (int)gridDim.x < tn_) __syncthreads();
    }
    return;
  }
  const int tm_ = (p.M + 63) / 64, tn_ = (p.N + 63) / 64, nt = tm_ * tn_;
  for (int bid = blockIdx.x; bid < nt; bid += gridDim.x) {
    gemm_tile_s_d<64, 64>(p, bid % tm_, bid / tm_, minus != 0, smem);
    if (bid + (int)gridDim.x < nt) __syncthreads();
  }
}

template <class T>
__global__ void resolve_dump_kernel(const NodeDesc<T>* __restrict__ nodes, GemmOp op, GemmProb<T>* out, int* ok) {
  GemmProb<T> p;
  memset(&p, 0, sizeof p);
  ok[blockIdx.x] = resolve_op<T, false>(nodes + blockIdx.x, op, p, nullptr) ? 1 : 0;
  out[blockIdx.x] = p;
}

// Switches of the leaf envelope and of the device-side flop count (test hooks, include/hs_kernels.h)
namespace {
std::atomic<int> g_env_on{-1};      // -1: not read yet (HS_LEAF_ENVELOPE, default on)
std::atomic<int> g_benv_on{-1};     // -1: not read yet (HS_BRANCH_ENVELOPE, default on)
std::atomic<int> g_env_order_on{-1};  // -1: not read yet (HS_ENV_ORDER, default 2)
std::atomic<int> g_op_count_on{0};
std::atomic<int> g_lds_on{-1};      // -1: not read yet (HS_GEMM_LDS, default on)
std::atomic<long long> g_lds_launches{0};
std::atomic<long long> g_lds_edge_launches{0};
std::atomic<long long> g_reg_launches{0};
}  // namespace
// HS_GEMM_LDS=0 / hsk_gemm_lds_enable(0): every plain update runs the register-staged gemm_op_kernel / gemm_op_env_kernel
static bool gemm_lds_enabled() {
  int v = g_lds_on.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("HS_GEMM_LDS");
    v = (e && e[0] == '0') ? 0 : 1;
    g_lds_on.store(v);
  }
  return v != 0;
}
extern "C" int hsk_gemm_lds_enable(int on) {  // returns the previous setting
  const int prev = gemm_lds_enabled() ? 1 : 0;
  g_lds_on.store(on ? 1 : 0);
  return prev;
}
extern "C" long long hsk_gemm_lds_launches(int reset) {  // launches sent to gemm_op_lds_kernel since the last reset
  return reset ? g_lds_launches.exchange(0) : g_lds_launches.load();
}
extern "C" long long hsk_gemm_lds_edge_launches(int reset) {  // launches sent to gemm_op_lds_edge_kernel / gemm_op_env_lds_kernel
  return reset ? g_lds_edge_launches.exchange(0) : g_lds_edge_launches.load();
}
extern "C" long long hsk_gemm_reg_launches(int reset) {  // plain, uncounted Float64 updates sent to gemm_op_kernel / gemm_op_env_kernel
  return reset ? g_reg_launches.exchange(0) : g_reg_launches.load();
}
extern "C" int hsk_gemm_lds_route(int cmat, int r0, int k0, int k1, int ni) { return hs_gemm_lds_route(cmat, r0, k0, k1, ni); }
bool hs_envelope_enabled() {
  int v = g_env_on.load();
  if (v < 0) {
    const char* e = getenv("HS_LEAF_ENVELOPE");
    v = (e && e[0] == '0') ? 0 : 1;
    g_env_on.store(v);
  }
  return v != 0;
}
extern "C" int hsk_envelope_enable(int on) {  // returns the previous setting
  const int prev = hs_envelope_enabled() ? 1 : 0;
  g_env_on.store(on ? 1 : 0);
  return prev;
}
// the branch fronts' tables alone; effective only while the envelope as a whole is on
bool hs_branch_envelope_enabled() {
  int v = g_benv_on.load();
  if (v < 0) {
    const char* e = getenv("HS_BRANCH_ENVELOPE");
    v = (e && e[0] == '0') ? 0 : 1;
    g_benv_on.store(v);
  }
  return v != 0;
}
extern "C" int hsk_branch_envelope_enable(int on) {  // returns the previous setting
  const int prev = hs_branch_envelope_enabled() ? 1 : 0;
  g_benv_on.store(on ? 1 : 0);
  return prev;
}
// HS_ENV_ORDER / hsk_env_order_enable: 0 = enveloped plain updates walk their tiles in the order of the dense launches, 1 = the balanced
// order, 2 = the K-sorted order (default; launches whose Sched carries no scratch for the tables run 1)
static int env_order_setting() {
  int v = g_env_order_on.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("HS_ENV_ORDER");
    v = (e && e[0] == '0') ? 0 : ((e && e[0] == '1') ? 1 : 2);
    g_env_order_on.store(v);
  }
  return v;
}
extern "C" int hsk_env_order_enable(int on) {  // returns the previous setting
  const int prev = env_order_setting();
  g_env_order_on.store(on < 0 ? 0 : (on > 2 ? 2 : on));
  return prev;
}
// Tile rows / columns a scratch slot of the K-sorted order holds for a batch whose fronts have at most maxm rows; hs_env_perm_wanted: whether
// a front of that size can reach the lower tile limit at all (analysis: levels that cannot get no scratch).  hsk_env_perm_slot_limit
// (tests) lowers the cap, so that small fronts take the fallback of fronts that do not fit; returns the previous cap.
namespace {
std::atomic<int> g_perm_slot_limit{HS_ENV_PERM_MAX};
std::atomic<int> g_perm_min_tiles{-1};  // -1: not read yet
std::atomic<long long> g_perm_launches{0};
}
int hs_env_perm_slot(int maxm) {
  const int need = ((maxm + 1 + 127) / 128 + 7) / 8 * 8;  // (128 x 128 Float64 tiles: the only ones that take the order; + 1: the shifted edge tile)
  return std::max(8, std::min(need, g_perm_slot_limit.load(std::memory_order_relaxed)));
}
// Fronts with fewer tiles than this keep the balanced order under HS_ENV_ORDER=2 (HS_ENV_ORDER_MIN_TILES; default 2048 = four rounds of 8
// units).  The K-sorted order evens the XCDs out over whole rounds, heaviest unit to another XCD in each; a front of a few hundred tiles has
// one round or none, and in a batched launch every front leans the same way.  A heuristic fitted on ONE problem, Poisson 128^3
// (profiles/r27_env_phase_order.txt): the level-wide Schur launches of 2116 tiles per front and more gain 3-9 %, those of 121, 361 and 900
// tiles lose 7-70 % without the limit.  The reason given suggests a criterion in rounds of units per XCD over the whole batch; not tried.
static int hs_env_perm_min_tiles() {
  int v = g_perm_min_tiles.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("HS_ENV_ORDER_MIN_TILES");
    v = e ? std::max(0, atoi(e)) : HS_ENV_PERM_MIN_TILES;
    g_perm_min_tiles.store(v);
  }
  return v;
}
extern "C" int hsk_env_perm_min_tiles(int min_tiles) {  // tests; < 0: back to the default.  Returns the previous limit
  const int prev = hs_env_perm_min_tiles();
  g_perm_min_tiles.store(min_tiles < 0 ? HS_ENV_PERM_MIN_TILES : min_tiles);
  return prev;
}
// launches of env_perm_kernel from launch_gemm_op since the last reset: the enveloped updates that really ran the K-sorted order
extern "C" long long hsk_env_perm_launches(int reset) { return reset ? g_perm_launches.exchange(0) : g_perm_launches.load(); }
bool hs_env_perm_wanted(int maxm) {
  const long long t = (maxm + 1 + 127) / 128;
  return t * t >= hs_env_perm_min_tiles();
}
extern "C" int hsk_env_perm_slot_limit(int limit) {
  const int prev = g_perm_slot_limit.load();
  g_perm_slot_limit.store(std::max(8, std::min(limit / 8 * 8, HS_ENV_PERM_MAX)));
  return prev;
}
// The tile every block id of a launch with one workgroup per tile gets (first front of a batch: shift 0), by the functions
// gemm_dispatch_env calls.  Host only.
extern "C" int hsk_env_tile_order(int tiles_m, int tiles_n, int order, int32_t* tm, int32_t* tn) {
  if (tiles_m <= 0 || tiles_n <= 0 || tiles_m > 32768 || tiles_n > 32768 || !tm || !tn || (long long)tiles_m * tiles_n > (1 << 24)) return -1;
  const int ntiles = tiles_m * tiles_n;
  const int sm = order ? env_order_stride(tiles_m) : 1, sn = order ? env_order_stride(tiles_n) : 1;
  for (int bid = 0; bid < ntiles; ++bid) {
    int m, n;
    tile_coords(xcd_remap_shift(bid, ntiles, 0), tiles_m, tiles_n, m, n);
    env_order_apply(m, n, tiles_m, tiles_n, sm, sn);
    tm[bid] = m;
    tn[bid] = n;
  }
  return 0;
}
// The same for the K-sorted order, from caller-made keys (kr: tiles_m, kc: tiles_n entries, what env_perm_kernel computes from a front's
// tables) and the shift of the front in its batch.  Host only; the sorts, the unit keys and the map are the functions the kernels call.
extern "C" int hsk_env_phase_order(int tiles_m, int tiles_n, const int32_t* kr, const int32_t* kc, int shift, int32_t* tm, int32_t* tn, int32_t* pos) {
  if (tiles_m <= 0 || tiles_n <= 0 || tiles_m > HS_ENV_PERM_MAX || tiles_n > HS_ENV_PERM_MAX || !kr || !kc || !tm || !tn || shift < 0 || shift > 7) return -1;
  for (int i = 0; i < tiles_m; ++i)
    if (kr[i] < 0 || kr[i] > (1 << 24)) return -1;
  for (int j = 0; j < tiles_n; ++j)
    if (kc[j] < 0 || kc[j] > (1 << 24)) return -1;
  std::vector<uint16_t> rowperm(tiles_m), colperm(tiles_n);
  std::vector<int> skr(tiles_m), skc(tiles_n);
  for (int i = 0; i < tiles_m; ++i) { const int r = env_rank(kr, tiles_m, i); rowperm[r] = (uint16_t)i; skr[r] = kr[i]; }
  for (int j = 0; j < tiles_n; ++j) { const int r = env_rank(kc, tiles_n, j); colperm[r] = (uint16_t)j; skc[r] = kc[j]; }
  const int gn = tiles_n >> 3, nfull = (tiles_m >> 3) * gn, ntiles = tiles_m * tiles_n;
  std::vector<int> ukey(nfull);
  std::vector<uint16_t> unitperm(nfull + 1);
  for (int u = 0; u < nfull; ++u) ukey[u] = env_unit_key(skr.data(), skc.data(), u / gn, u % gn);
  for (int u = 0; u < nfull; ++u) unitperm[env_rank(ukey.data(), nfull, u)] = (uint16_t)u;
  for (int bid = 0; bid < ntiles; ++bid) {
    int a, b;
    const int p = env_phase_pos(bid, ntiles, nfull, shift);
    env_phase_coords(p, tiles_m, tiles_n, unitperm.data(), a, b);
    if (pos) pos[bid] = p;
    tm[bid] = rowperm[a];
    tn[bid] = colperm[b];
  }
  return 0;
}
// env_perm_kernel on one front, as launch_gemm_op launches it in front of the plain update (cmat, bmat, r0 .. k1) of a front with ni / nb
// rows and the block envelope `env` (2 * hs_env_nblocks entries, firstL then firstU; null: none).  No matrix is touched: the descriptor
// carries 16-byte aligned addresses that are never read.  out: hs_env_perm_stride(slot) entries, the slot as the kernel leaves it for the
// first front of a launch (XCD shift 0).
template <class T>
static int env_perm_hook(int ni, int nb, const int32_t* env, const GemmOp& op_in, int edge, int slot, uint16_t* out) {
  if (ni <= 0 || nb < 0 || ni + nb > (1 << 20) || slot < 8 || (slot & 7) || slot > HS_ENV_PERM_MAX || !out) return -1;
  const int m = ni + nb, nblk = hs_env_nblocks(ni, nb), stride = hs_env_perm_stride(slot);
  NodeDesc<T> d;
  memset(&d, 0, sizeof d);
  d.ni = ni; d.nb = nb; d.m = m;
  d.ldl = (m + 1) / 2 * 2; d.ldu = (ni + 1) / 2 * 2; d.lds = std::max((nb + 1) / 2 * 2, 2);
  d.LF = (T*)(uintptr_t)0x10000000; d.UR = (T*)(uintptr_t)0x20000000; d.SB = (T*)(uintptr_t)0x30000000;
  d.ni1 = ni; d.nb1 = nb;
  int* denv = nullptr;
  NodeDesc<T>* dn = nullptr;
  uint16_t* dpm = nullptr;
  int rc = 0;
  if (env && hipMalloc((void**)&denv, sizeof(int) * 2 * nblk) != hipSuccess) rc = -6;
  if (!rc && hipMalloc((void**)&dn, sizeof d) != hipSuccess) rc = -6;
  if (!rc && hipMalloc((void**)&dpm, sizeof(uint16_t) * stride) != hipSuccess) rc = -6;
  if (!rc && env && hipMemcpy(denv, env, sizeof(int) * 2 * nblk, hipMemcpyHostToDevice) != hipSuccess) rc = -6;
  if (!rc) {
    d.env = denv;
    d.finalize();
    GemmOp op = op_in;
    op.ainv = 0; op.env = env ? 1 : 0; op.order = 2; op.perm = dpm; op.perm_slot = slot;
    if (hipMemcpy(dn, &d, sizeof d, hipMemcpyHostToDevice) != hipSuccess || hipMemset(dpm, 0xFF, sizeof(uint16_t) * stride) != hipSuccess) rc = -6;
    if (!rc) {
      hipLaunchKernelGGL(env_perm_kernel<T>, dim3(2), dim3(256), 0, nullptr, dn, op, edge, 8, 0);  // (two workgroups share the table; shift 0; no lower limit)
      if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, dpm, sizeof(uint16_t) * stride, hipMemcpyDeviceToHost) != hipSuccess) rc = -6;
    }
  }
  if (denv) (void)hipFree(denv);
  if (dn) (void)hipFree(dn);
  if (dpm) (void)hipFree(dpm);
  return rc;
}
extern "C" int hsk_env_perm(int is_complex, int ni, int nb, const int32_t* env, int cmat, int bmat, int r0, int r1, int c0, int c1, int k0, int k1,
                            int edge, int slot, uint16_t* out) {
  if (cmat < 0 || cmat > 2 || bmat < 0 || bmat > 2 || r0 < 0 || c0 < 0 || k0 < 0) return -1;
  GemmOp op{cmat, bmat, r0, r1, c0, c1, k0, k1};
  return is_complex ? env_perm_hook<cplx>(ni, nb, env, op, 0, slot, out) : env_perm_hook<double>(ni, nb, env, op, edge ? 1 : 0, slot, out);
}
extern "C" int hsk_op_flops_mode(int on) {  // resets the counter
  (void)hipDeviceSynchronize();
  g_op_count_on.store(on ? 1 : 0);
  const double z = 0.0;
  return hipMemcpyToSymbol(HIP_SYMBOL(g_op_flops), &z, sizeof z) == hipSuccess ? 0 : -6;
}
extern "C" int hsk_op_flops(double* out) {
  if (!out) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -6;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_op_flops), sizeof *out) == hipSuccess ? 0 : -6;
}

// HS_DEBUG_SYNC=2: print what the first fronts of a batch resolve this op to (diagnostics, no arithmetic)
template <class T>
static void dump_resolved_op(const NodeDesc<T>* dnodes, int nbatch, int maxM, int maxN, const GemmOp& op, hipStream_t s) {
  GemmProb<T>* dp;
  int* dok;
  (void)hipMalloc((void**)&dp, sizeof(GemmProb<T>) * nbatch);
  (void)hipMalloc((void**)&dok, sizeof(int) * nbatch);
  hipLaunchKernelGGL(resolve_dump_kernel<T>, dim3(nbatch), dim3(1), 0, s, dnodes, op, dp, dok);
  (void)hipStreamSynchronize(s);
  GemmProb<T> hp;
  int hok;
  NodeDesc<T> hn;
  for (int i = 0; i < nbatch && i < 4; ++i) {
    (void)hipMemcpy(&hp, dp + i, sizeof hp, hipMemcpyDeviceToHost);
    (void)hipMemcpy(&hok, dok + i, sizeof hok, hipMemcpyDeviceToHost);
    (void)hipMemcpy(&hn, dnodes + i, sizeof hn, hipMemcpyDeviceToHost);
    fprintf(stderr, "[hs debug] gemm op c%d b%d r[%d,%d) c[%d,%d) k[%d,%d) node%d: ok=%d A=%p B=%p C=%p M=%d N=%d K=%d ld=%d,%d,%d | LF=%p UR=%p SB=%p ni=%d nb=%d m=%d ld=%d,%d,%d maxM=%d maxN=%d\n",
            op.cmat, op.bmat, op.r0, op.r1, op.c0, op.c1, op.k0, op.k1, i, hok, (void*)hp.A, (void*)hp.B, (void*)hp.C, hp.M, hp.N, hp.K, hp.lda,
            hp.ldb, hp.ldc, (void*)hn.LF, (void*)hn.UR, (void*)hn.SB, hn.ni, hn.nb, hn.m, hn.ldl, hn.ldu, hn.lds, maxM, maxN);
  }
  (void)hipFree(dp);
  (void)hipFree(dok);
}

// > 64 KiB of LDS per workgroup needs the opt-in, once per kernel and process (launches come from several streams and threads)
template <class K>
static void opt_in_lds(std::once_flag& once, std::initializer_list<K> kernels, int lds_bytes) {
  std::call_once(once, [&] {
    for (K k : kernels) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  });
}

// The kernel a launch of launch_gemm_op gets, with its LDS size and the launch counter it feeds (nullptr: none)
template <class T>
struct OpKernel {
  void (*fn)(const NodeDesc<T>*, GemmOp);
  int lds_bytes;
  std::atomic<long long>* launches;
};
template <class T>
static OpKernel<T> pick_op_kernel(const GemmOp& op, int route) {
  constexpr int lds_reg = TileCfg<T>::smem_doubles * 8;
  if constexpr (sizeof(T) == 8) {
    constexpr int lds_direct = TileCfg<T>::smem_doubles_lds * 8;
    if (route == HS_GEMM_ROUTE_LDS) return {gemm_op_lds_kernel<T>, lds_direct, &g_lds_launches};
    if (route != HS_GEMM_ROUTE_REG) return {op.env ? gemm_op_env_lds_kernel<T> : gemm_op_lds_edge_kernel<T>, lds_direct, &g_lds_edge_launches};
  }
  std::atomic<long long>* const reg = (sizeof(T) == 8 && !op.ainv && !op.count) ? &g_reg_launches : nullptr;
  if (op.env || op.count) return {op.ainv ? trsm_inv_env_kernel<T> : gemm_op_env_kernel<T>, lds_reg, reg};
  return {op.ainv ? trsm_inv_kernel<T> : gemm_op_kernel<T>, lds_reg, reg};
}

template <class T>
void launch_gemm_op(const NodeDesc<T>* dnodes, int nbatch, int maxM, int maxN, const GemmOp& op_in, hipStream_t s, int route, bool shifted,
                    long long live_tiles, uint16_t* perm, int perm_slot) {
  if (nbatch <= 0 || maxM <= 0 || maxN <= 0) return;
  GemmOp op = op_in;
  op.count = (!op.ainv && g_op_count_on.load(std::memory_order_relaxed)) ? 1 : 0;
  op.order = (op.env && !op.ainv) ? env_order_setting() : 0;
  if (op.order == 2 && (!perm || perm_slot < 8 || perm_slot > HS_ENV_PERM_MAX)) op.order = 1;  // no scratch for the tables on this path
  static const bool dump = getenv("HS_DEBUG_SYNC") && getenv("HS_DEBUG_SYNC")[0] == '2';
  if (dump) dump_resolved_op(dnodes, nbatch, maxM, maxN, op, s);
  // (the caller vouches for K and the alignment of every front: hs_gemm_lds_route)
  if (sizeof(T) != 8 || op.ainv || op.count || !gemm_lds_enabled()) route = HS_GEMM_ROUTE_REG;
  if (op.env && route == HS_GEMM_ROUTE_LDS) route = HS_GEMM_ROUTE_EDGE;  // one enveloped twin: the edge tile
  if (op.order == 2 && route == HS_GEMM_ROUTE_REG) op.order = 1;  // (gemm_op_env_kernel holds no K-sorted order: ComplexF64, odd k0, counted launches)
  op.perm = op.order == 2 ? perm : nullptr;
  op.perm_slot = op.order == 2 ? perm_slot : 0;
  if (route == HS_GEMM_ROUTE_EDGE && shifted) maxM += 1;  // a front whose A sits at an odd row runs one row higher (edge_shift_rows)
  int tiles = ((maxM + TileCfg<T>::BM - 1) / TileCfg<T>::BM) * ((maxN + TileCfg<T>::BN - 1) / TileCfg<T>::BN);
  const int all_tiles = tiles;
  if (op.order == 2 && all_tiles < hs_env_perm_min_tiles()) op.order = 1, op.perm = nullptr, op.perm_slot = 0;  // (no front of the launch is large enough)
  if (op.cap > 0 && tiles > op.cap) tiles = std::max(8, op.cap / 8 * 8);
  // Enveloped launch of a batch of leaf fronts: most tiles of the bounding box are empty.  A workgroup per tile would start, read its
  // descriptor and leave; instead a quarter as many workgroups (HS_ENV_WALK, 1: off) walk the tiles, so that an empty tile costs a table
  // look-up inside a running workgroup.  The batch itself keeps the chip full (hundreds of fronts).  A branch front is the other case: most
  // of its tiles run, and a workgroup that walks four of them in a row loses the second resident workgroup of its CU that hides the C
  // traffic of the first.  So the walk is no longer than the grid's share of empty tiles, which the caller counted (live_tiles; -1: unknown).
  if (op.env && !(op.cap > 0)) {
    static const int walk_max = getenv("HS_ENV_WALK") ? atoi(getenv("HS_ENV_WALK")) : 4;
    int walk = walk_max;
    if (live_tiles >= 0) walk = (int)std::min<long long>(walk, (long long)tiles * nbatch / std::max(1LL, live_tiles));
    if (walk > 1 && tiles >= 32 && (long long)tiles * nbatch >= 4096) tiles = std::max(8, tiles / walk / 8 * 8);
  }
  static std::once_flag once_reg;
  opt_in_lds(once_reg, {gemm_op_kernel<T>, trsm_inv_kernel<T>, gemm_op_env_kernel<T>, trsm_inv_env_kernel<T>}, TileCfg<T>::smem_doubles * 8);
  if constexpr (sizeof(T) == 8) {
    if (route != HS_GEMM_ROUTE_REG) {
      static std::once_flag once_direct;
      opt_in_lds(once_direct, {gemm_op_lds_kernel<T>, gemm_op_lds_edge_kernel<T>, gemm_op_env_lds_kernel<T>}, TileCfg<T>::smem_doubles_lds * 8);
    }
  }
  const OpKernel<T> k = pick_op_kernel<T>(op, route);
  if (k.launches) k.launches->fetch_add(1, std::memory_order_relaxed);
  if (op.order == 2) {  // the tables of the K-sorted order, per front, for the tiling and the grid of the kernel below (the edge tile)
    g_perm_launches.fetch_add(1, std::memory_order_relaxed);
    hipLaunchKernelGGL(env_perm_kernel<T>, dim3(std::max(1, std::min(32, all_tiles / 2048)), nbatch), dim3(256), 0, s, dnodes, op, 1, tiles,
                       hs_env_perm_min_tiles());
  }
  hipLaunchKernelGGL(k.fn, dim3(tiles, nbatch), dim3(256), k.lds_bytes, s, dnodes, op);
}

// hs_probs_stats: flops (counted by the kernels), launches and -- with timing on -- the summed launch durations of the grouped products,
// process-wide (they are issued from the HSS module, the low-rank compressions and the matrix-free fronts, on several streams)
namespace {
struct ProbsAcc {
  std::mutex mu;
  int mode = 0;  // 0: off, 1: flops + launches, 2: + a HIP event pair around every launch
  long long launches = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
};
ProbsAcc& probs_acc() {
  static ProbsAcc* a = new ProbsAcc();
  return *a;
}
}  // namespace
extern "C" int hs_probs_stats_mode(int mode) {  // resets the counters
  ProbsAcc& a = probs_acc();
  std::lock_guard<std::mutex> lk(a.mu);
  (void)hipDeviceSynchronize();
  for (auto& e : a.ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  a.ev.clear();
  a.launches = 0;
  a.mode = mode;
  const double z = 0.0;
  return hipMemcpyToSymbol(HIP_SYMBOL(g_probs_flops), &z, sizeof z) == hipSuccess ? 0 : -6;
}
extern "C" int hs_probs_stats(double* out3) {  // {real flops executed, launches, summed launch seconds (0 without timing)}
  if (!out3) return -1;
  ProbsAcc& a = probs_acc();
  std::lock_guard<std::mutex> lk(a.mu);
  if (hipDeviceSynchronize() != hipSuccess) return -6;
  double fl = 0.0, ms = 0.0;
  if (hipMemcpyFromSymbol(&fl, HIP_SYMBOL(g_probs_flops), sizeof fl) != hipSuccess) return -6;
  for (auto& e : a.ev) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, e.first, e.second) == hipSuccess) ms += t;
  }
  out3[0] = fl; out3[1] = (double)a.launches; out3[2] = ms * 1e-3;
  return 0;
}

template <class T>
void launch_gemm_probs(const GemmProb<T>* dprobs, int nprob, int maxM, int maxN, int minus, hipStream_t s) {
  if (nprob <= 0 || maxM <= 0 || maxN <= 0) return;
  minus = minus ? 1 : 0;
  hipEvent_t pe0 = nullptr, pe1 = nullptr;
  {
    ProbsAcc& a = probs_acc();
    if (a.mode) {  // (read without the lock: switched only between factorizations)
      std::lock_guard<std::mutex> lk(a.mu);
      a.launches++;
      minus |= 2;
      if (a.mode >= 2 && hipEventCreate(&pe0) == hipSuccess && hipEventCreate(&pe1) == hipSuccess) {
        (void)hipEventRecord(pe0, s);
        a.ev.push_back({pe0, pe1});
      } else {
        pe1 = nullptr;
      }
    }
  }
  struct Rec {  // the closing event is recorded on every exit path
    hipEvent_t e; hipStream_t s;
    ~Rec() { if (e) (void)hipEventRecord(e, s); }
  } rec{pe1, s};
  int tiles = ((maxM + TileCfg<T>::BM - 1) / TileCfg<T>::BM) * ((maxN + TileCfg<T>::BN - 1) / TileCfg<T>::BN);
  constexpr int lds_bytes = TileCfg<T>::smem_doubles * 8;
  static std::once_flag once;
  opt_in_lds(once, {gemm_probs_kernel<T>}, lds_bytes);
  if constexpr (sizeof(T) == 8) {
    static const bool skinny = !(getenv("HS_GEMM_SKINNY") && getenv("HS_GEMM_SKINNY")[0] == '0');
    static const int small_tiles = getenv("HS_GEMM_SMALL_TILES") ? atoi(getenv("HS_GEMM_SMALL_TILES")) : 128;  // lists of at most this many 128 x 128 tiles
    if (skinny && (maxM <= 64 || (long long)tiles * nprob <= small_tiles)) {
      if (maxM > 64) tiles = ((maxM + 63) / 64) * ((maxN + 63) / 64);
      static std::once_flag once_skinny;
      opt_in_lds(once_skinny, {gemm_probs_skinny_kernel}, lds_bytes);
      hipLaunchKernelGGL(gemm_probs_skinny_kernel, dim3(tiles, nprob), dim3(256), lds_bytes, s, (const GemmProb<double>*)dprobs, minus);
      return;
    }
  }
  hipLaunchKernelGGL(gemm_probs_kernel<T>, dim3(tiles, nprob), dim3(256), lds_bytes, s, dprobs, minus);
}

template void launch_gemm_op<double>(const NodeDesc<double>*, int, int, int, const GemmOp&, hipStream_t, int, bool, long long, uint16_t*, int);
template void launch_gemm_op<cplx>(const NodeDesc<cplx>*, int, int, int, const GemmOp&, hipStream_t, int, bool, long long, uint16_t*, int);
template void launch_gemm_probs<double>(const GemmProb<double>*, int, int, int, int, hipStream_t);
template void launch_gemm_probs<cplx>(const GemmProb<cplx>*, int, int, int, int, hipStream_t);
