// PCA truncation-error curve: the residual sums of every requested rank in one pass
// (plot_PC_RMSE.py:25-46,84-108 compute_truncation_error per rank; include_trunc_error.py:41-49).
//
//   e_r[i,j] = (Y[i,j] - mu[j]) - sd[j] sum_{k < ranks[r]} C[i,k] V[k,j],   C = U diag(S), V = Vh,
//   tot[2r] = sum_ij e_r^2,  tot[2r+1] = sum_ij e_r,  node[r, j] = sum_i e_r[i,j]^2.
//
// The rank-p_r product is the rank-p_{r-1} product plus C[:, p_{r-1}:p_r] V[p_{r-1}:p_r, :], so ONE
// k-ordered v_mfma_f64_16x16x4_f64 chain over the PCs passes through every level; the squared
// residual of a level is accumulated when the chain crosses it.  Y and V are read once, C comes
// from L2, and no (n x ncols) array is stored: the reference builds R rank-k fields (R GEMMs with
// an (n, ncols) output) and takes R residual passes over them.
//
// Level boundaries: each segment [ranks[r-1], ranks[r]) of the inner dimension is padded to a
// multiple of 4 with ZERO operands (both the C and the V element), so a level always ends on a
// whole MFMA step and the chain needs no partial-step correction.  The padded-k -> k table
// (<= 224 entries) and the step at which every level ends are built on the host at enqueue and
// travel by value in the kernel's argument block: a captured graph keeps them, and nothing is
// copied from the caller's host array after the call returns.  A padding step adds exact zeros
// (0 x 0 into the accumulator), so a level's sums do not depend on which other levels were asked
// for: every element is the k-ordered chain over k < ranks[r], and a list split over several
// calls gives the bits of one call.
//
// Layout: block = 4 waves = one panel of 64 columns, 16 per wave; a block walks all rows of Y in
// tiles of 16 RS rows (RS = 2 row sub-tiles: two independent accumulators per wave; RS = 1 when
// n <= 16 or the padded inner dimension is so long that the LDS would not hold two).
//   LDS   the block's V panel, padded-k major per wave ([wave][kpad][16]: a k-step's B operands
//         are one conflict-free 64-bit read), read from HBM once; the current C row tile
//         ([16 RS][kpad + 2]: pitch = 2 mod 4 doubles, conflict-free A reads), single-buffered,
//         the next tile's loads (C from L2, Y from HBM) in flight in registers under the chain.
//   regs  per level and lane one sum of e^2 (its column, its rows) and one of e: 2 x 32 doubles,
//         indexed at compile time (the level loop is unrolled, a level's k-steps are a run-time
//         loop); e0 = Y - mu of the tile; two accumulator sets, used in turn by the levels.
// The epilogue of level r (e = e0 - sd D, e^2 and e added up: 3 fp64 VALU operations per element)
// is issued behind the first MFMA step of level r + 1, which does not depend on it.
//
// Measured (MI355X, n = 512, ncols = 1,347,945, float32 Y, the reference's 26 ranks up to 100,
// padded inner dimension 156): 13.3 ms, 0.21 of the fp64 MFMA floor; ~3.5 ms of it is the row
// loop with no chain at all (ranks = {0}), ~0.16 ms per k-step and ~0.14 ms per level come on top
// (DESIGN.md 4.6d).  One wave per SIMD (registers: the 64 per-level sums; LDS: the V panel)
// leaves each k-step waiting for its own LDS operands.
//
// Determinism: no atomics.  A panel reduces its lanes in a fixed shuffle / LDS order and writes
// its nlev x 2 partial sums to slot `panel` of the workspace; a second launch adds the panels up
// in an order that depends on their number only.  node is written from the same registers, so
// tot has the same bits with and without it.
#include "gpfit_common.h"
#include "../../include/gpfit.h"

namespace {

constexpr int kPcaMaxRank = 128;
constexpr int kPcaMaxLev = 32;
constexpr int kPcaMaxKpad = kPcaMaxRank + 3 * kPcaMaxLev;     // 224: every segment padded by <= 3
constexpr int kPcaThreads = 256;
constexpr int kPcaCols = 64;                                  // columns per panel (block)
constexpr int kPcaRed = 4 * kPcaMaxLev * 2;                   // per-wave partials (doubles)
constexpr int kPcaSlack = 8;                                  // the operand prefetch reads one step on
constexpr int kPcaNone = 255;                                 // table entry of a zero operand
constexpr long long kPcaLdsMax = 160 * 1024;

struct PcaArgs {
  const void* Y;
  long long ldy;
  int n, ncols;
  const double* mu;
  const double* sd;
  const double* C;
  long long ldc;
  const double* V;
  long long ldv;
  int nlev, kpad;                        // kpad: padded inner dimension, a multiple of 4, >= 4
  double* part;                          // npanels x nlev x 2
  double* node;
  long long ldn;
  unsigned char send[kPcaMaxLev];        // MFMA steps (of 4 padded k) done when level r ends
  unsigned char ktab[kPcaMaxKpad];       // padded k -> k, kPcaNone = zero operand
};

constexpr long long pca_lds_doubles(int rs, int kpad) {
  return (long long)kPcaCols * kpad + 16LL * rs * (kpad + 2) + kPcaSlack + kPcaRed;
}

GP_DEV double shfl_xor_f64(double x, int m) { return __shfl_xor(x, m, 64); }

template <int RS, bool F32>
__global__ __launch_bounds__(kPcaThreads, 1) void pca_trunc_kernel(const PcaArgs a) {
  using YT = std::conditional_t<F32, float, double>;
  extern __shared__ double pca_lds[];
  const int kpad = a.kpad, cp = kpad + 2;
  double* Vs = pca_lds;                                  // [4][kpad][16]
  double* Cs = Vs + kPcaCols * kpad;                     // [16 RS][cp] + slack
  double* red = Cs + 16 * RS * cp + kPcaSlack;           // [4][32][2]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int n = a.n, ncols = a.ncols, nlev = a.nlev;
  const long long panel = blockIdx.x;
  const long long c0 = panel * kPcaCols;
  const long long col = c0 + 16 * wv + li;
  const bool colok = col < ncols;
  const double mu_c = (a.mu && colok) ? a.mu[col] : 0.0;
  const double sd_c = (a.sd && colok) ? a.sd[col] : 1.0;
  const YT* Yp = static_cast<const YT*>(a.Y);

  // the C tile's loads: thread -> padded k = (tid & 63) + 64 j, rows (tid >> 6) + 4 i
  int kk[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int kp = (tid & 63) + 64 * j;
    kk[j] = kp < kpad ? a.ktab[kp] : kPcaNone;
  }
  double pre[4 * RS][4];
  auto load_c = [&](int t) __attribute__((always_inline)) {
    const int r0 = 16 * RS * t + (tid >> 6);
#pragma unroll
    for (int i = 0; i < 4 * RS; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = r0 + 4 * i;
        pre[i][j] = (kk[j] != kPcaNone && row < n) ? a.C[(long long)row * a.ldc + kk[j]] : 0.0;
      }
  };
  auto store_c = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4 * RS; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kp = (tid & 63) + 64 * j;
        if (kp < kpad) Cs[((tid >> 6) + 4 * i) * cp + kp] = pre[i][j];
      }
  };
  // Y of the tile in the MFMA C layout: row 16 rs + lk + 4 q, the lane's column
  YT yraw[RS][4];
  auto load_y = [&](int t) __attribute__((always_inline)) {
#pragma unroll
    for (int rs = 0; rs < RS; ++rs)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = 16 * RS * t + 16 * rs + lk + 4 * q;
        yraw[rs][q] = (colok && row < n) ? Yp[(long long)row * a.ldy + col] : YT(0);
      }
  };

  load_c(0);
  load_y(0);
  // the V panel, zero where the table says so and beyond the last column: wave w takes padded
  // rows w, w + 4, ... (the table entry is wave-uniform, a row is 512 contiguous bytes), eight
  // rows in flight at a time
  {
    const int wu = __builtin_amdgcn_readfirstlane(wv);
    const long long c = c0 + lane;
    double* dst = Vs + ((lane >> 4) * kpad) * 16 + (lane & 15);
    for (int kp0 = wu; kp0 < kpad; kp0 += 32) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int kp = kp0 + 4 * u;
        const int k = kp < kpad ? a.ktab[kp] : kPcaNone;
        v[u] = (k != kPcaNone && c < ncols) ? a.V[(long long)k * a.ldv + c] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int kp = kp0 + 4 * u;
        if (kp < kpad) dst[kp * 16] = v[u];
      }
    }
  }
  store_c();
  __syncthreads();

  double sq[kPcaMaxLev], sm[kPcaMaxLev];
#pragma unroll
  for (int r = 0; r < kPcaMaxLev; ++r) sq[r] = sm[r] = 0.0;

  const double* Vw = Vs + wv * kpad * 16 + lk * 16 + li;   // + 64 s: the B operand of step s
  const double* Cw = Cs + li * cp + lk;                    // + 16 rs cp + 4 s: the A operands
  const int ntile = (n + 16 * RS - 1) / (16 * RS);
  for (int t = 0; t < ntile; ++t) {
    double e0[RS][4];
#pragma unroll
    for (int rs = 0; rs < RS; ++rs)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = 16 * RS * t + 16 * rs + lk + 4 * q;
        e0[rs][q] = (colok && row < n) ? static_cast<double>(yraw[rs][q]) - mu_c : 0.0;
      }
    const bool more = t + 1 < ntile;
    if (more) {                                          // in flight under the chain
      load_c(t + 1);
      load_y(t + 1);
    }
    // two accumulator sets: level r accumulates in X[r & 1], starting from the products of level
    // r - 1 in X[(r - 1) & 1], which stay there until that level's epilogue has read them
    f64x4 X[2][RS];
#pragma unroll
    for (int rs = 0; rs < RS; ++rs) X[0][rs] = X[1][rs] = zero4();
    // operands of the step to come, read one step ahead of their MFMAs
    int s = 0;
    double bc = Vw[0], ac[RS];
#pragma unroll
    for (int rs = 0; rs < RS; ++rs) ac[rs] = Cw[16 * rs * cp];
    auto step = [&](f64x4(&dst)[RS], const f64x4(&src)[RS]) __attribute__((always_inline)) {
      const double bn = Vw[64 * (s + 1)];
      double an[RS];
#pragma unroll
      for (int rs = 0; rs < RS; ++rs) an[rs] = Cw[16 * rs * cp + 4 * (s + 1)];
#pragma unroll
      for (int rs = 0; rs < RS; ++rs) dst[rs] = mfma16x16x4(ac[rs], bc, src[rs]);
      bc = bn;
#pragma unroll
      for (int rs = 0; rs < RS; ++rs) ac[rs] = an[rs];
      ++s;
    };
    // a level's epilogue: the residuals of the tile first (independent), then the two sums in
    // row order, their dependent chains interleaved
    auto level_sums = [&](const f64x4(&D)[RS], double& q2, double& q1)
                          __attribute__((always_inline)) {
      double e[RS][4];
#pragma unroll
      for (int rs = 0; rs < RS; ++rs)
#pragma unroll
        for (int q = 0; q < 4; ++q) e[rs][q] = fma(-sd_c, D[rs][q], e0[rs][q]);
#pragma unroll
      for (int rs = 0; rs < RS; ++rs)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          q2 = fma(e[rs][q], e[rs][q], q2);
          q1 += e[rs][q];
        }
    };
    // the level loop is unrolled: sq / sm and the accumulator sets are indexed at compile time
#pragma unroll
    for (int r = 0; r < kPcaMaxLev; ++r) {
      if (r < nlev) {
        const int se = a.send[r];
        if (r > 0) {
          step(X[r & 1], X[(r - 1) & 1]);                // ranks increase: a level has a step
          // the level before, behind the MFMAs just issued
          level_sums(X[(r - 1) & 1], sq[r > 0 ? r - 1 : 0], sm[r > 0 ? r - 1 : 0]);
        }
        while (s < se) step(X[r & 1], X[r & 1]);
        if (r + 1 == nlev) {                             // the last level
          level_sums(X[r & 1], sq[r], sm[r]);
        }
      }
    }
    __syncthreads();                                     // every wave is done with the C tile
    if (more) {
      store_c();
      __syncthreads();
    }
  }

  // lanes -> columns (node) -> wave -> block, in a fixed order
#pragma unroll
  for (int r = 0; r < kPcaMaxLev; ++r) {
    if (r < nlev) {
      double v = sq[r];
      v += shfl_xor_f64(v, 16);
      v += shfl_xor_f64(v, 32);
      if (a.node && lk == 0 && colok) a.node[(long long)r * a.ldn + col] = v;
      double u = sm[r];
      u += shfl_xor_f64(u, 16);
      u += shfl_xor_f64(u, 32);
#pragma unroll
      for (int m = 8; m >= 1; m >>= 1) {
        v += shfl_xor_f64(v, m);
        u += shfl_xor_f64(u, m);
      }
      if (lane == 0) {
        red[(wv * kPcaMaxLev + r) * 2] = v;
        red[(wv * kPcaMaxLev + r) * 2 + 1] = u;
      }
    }
  }
  __syncthreads();
  if (tid < 2 * nlev) {
    const int r = tid >> 1, c = tid & 1;
    double v = red[r * 2 + c];
#pragma unroll
    for (int w = 1; w < 4; ++w) v += red[(w * kPcaMaxLev + r) * 2 + c];
    a.part[(panel * nlev + r) * 2 + c] = v;
  }
}

// tot[i] = sum over the panels of part[panel][i], i = 2 r + c: one block per sum, every thread a
// strided run of panels in order, then a fixed tree
__global__ __launch_bounds__(256) void pca_trunc_reduce_kernel(const double* __restrict__ part,
                                                               long long npanels, int nsum,
                                                               double* __restrict__ tot) {
  __shared__ double red[256];
  const int i = blockIdx.x, tid = threadIdx.x;
  double v = 0.0;
  for (long long p = tid; p < npanels; p += 256) v += part[p * nsum + i];
  red[tid] = v;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) tot[i] = red[0];
}

template <int RS, bool F32>
hipError_t launch_pca(const PcaArgs& a, long long npanels, hipStream_t stream) {
  const size_t lds = (size_t)pca_lds_doubles(RS, a.kpad) * sizeof(double);
  static const hipError_t attr = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&pca_trunc_kernel<RS, F32>),
      hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPcaLdsMax);
  if (attr != hipSuccess) return attr;
  hipLaunchKernelGGL((pca_trunc_kernel<RS, F32>), dim3((unsigned)npanels), dim3(kPcaThreads), lds,
                     stream, a);
  return hipGetLastError();
}

long long pca_ws_bytes(int ncols, int nlev) {
  const long long npanels = ((long long)ncols + kPcaCols - 1) / kPcaCols;
  return align256(npanels * nlev * 2 * (long long)sizeof(double));
}

}  // namespace

extern "C" int gp_pca_trunc_max_rank(void) { return kPcaMaxRank; }
extern "C" int gp_pca_trunc_max_levels(void) { return kPcaMaxLev; }

extern "C" long long gp_pca_trunc_ws_bytes(int n, int ncols, int nlev) {
  if (n < 0 || ncols < 0 || nlev < 0 || nlev > kPcaMaxLev) return -1;
  if (n == 0 || ncols == 0 || nlev == 0) return 0;
  return pca_ws_bytes(ncols, nlev);
}

extern "C" int gp_pca_trunc(const void* Y, long long ldy, int y_f32, int n, int ncols,
                            const double* mu, const double* sd, const double* C, long long ldc,
                            const double* V, long long ldv, const int* ranks, int nlev,
                            double* tot, double* node, long long ldn, void* ws,
                            long long ws_bytes, hipStream_t stream) {
  // the dimensions and the rank list first (the strides are checked against them), then the
  // operands in the order they are listed
  if (n < 0) return -4;
  if (ncols < 0) return -5;
  if (nlev < 0 || nlev > kPcaMaxLev) return -13;
  if (nlev > 0 && !ranks) return -12;
  for (int r = 0; r < nlev; ++r)
    if (ranks[r] < 0 || ranks[r] > kPcaMaxRank || (r > 0 && ranks[r] <= ranks[r - 1])) return -12;
  const int pmax = nlev > 0 ? ranks[nlev - 1] : 0;
  if (!Y) return -1;
  if (ldy < ncols || ldy < 1) return -2;
  if (y_f32 != 0 && y_f32 != 1) return -3;
  if ((mu == nullptr) != (sd == nullptr)) return -6;
  if (!C) return -8;
  if (ldc < pmax || ldc < 1) return -9;
  if (!V) return -10;
  if (ldv < ncols || ldv < 1) return -11;
  if (!tot) return -14;
  if (node && (ldn < ncols || ldn < 1)) return -16;
  if (n == 0 || ncols == 0 || nlev == 0) return 0;
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255)) return -17;
  if (ws_bytes < pca_ws_bytes(ncols, nlev)) return -18;

  PcaArgs a = {};
  a.Y = Y; a.ldy = ldy; a.n = n; a.ncols = ncols; a.mu = mu; a.sd = sd; a.C = C; a.ldc = ldc;
  a.V = V; a.ldv = ldv; a.nlev = nlev; a.part = static_cast<double*>(ws); a.node = node;
  a.ldn = ldn;
  int kp = 0, prev = 0;
  for (int r = 0; r < nlev; ++r) {
    for (int k = prev; k < ranks[r]; ++k) a.ktab[kp++] = (unsigned char)k;
    while (kp & 3) a.ktab[kp++] = kPcaNone;
    a.send[r] = (unsigned char)(kp / 4);
    prev = ranks[r];
  }
  while (kp < 4) a.ktab[kp++] = kPcaNone;               // ranks = {0}: one step of zeros, never run
  a.kpad = kp;

  const long long npanels = ((long long)ncols + kPcaCols - 1) / kPcaCols;
  const bool two = n > 16 && pca_lds_doubles(2, kp) * (long long)sizeof(double) <= kPcaLdsMax;
  hipError_t e;
  if (two)
    e = y_f32 ? launch_pca<2, true>(a, npanels, stream) : launch_pca<2, false>(a, npanels, stream);
  else
    e = y_f32 ? launch_pca<1, true>(a, npanels, stream) : launch_pca<1, false>(a, npanels, stream);
  if (e != hipSuccess) return GPFIT_ERR_HIP - (int)e;
  hipLaunchKernelGGL(pca_trunc_reduce_kernel, dim3((unsigned)(2 * nlev)), dim3(256), 0, stream,
                     a.part, npanels, 2 * nlev, tot);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : GPFIT_ERR_HIP - (int)e;
}
