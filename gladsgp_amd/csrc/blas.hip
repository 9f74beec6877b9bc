// Fit-side dense kernels (fp64): general MFMA GEMM with split-K, column statistics and
// elementwise standardisation.  They implement the non-GP arithmetic of the drop-in surface:
//   src/svd.py:52-64   Y = X Omega, (X X^T) Y, Q^T X, U = Q U_B      (randomized SVD, A2)
//   src/model.py:60-72 mu = mean(Y, 0), sd = std(Y, ddof=1, 0) floored, Y_std      (A1)
//   src/model.py:101, 219-223  K = diag(S) Vh / sqrt(n), w = Y_std pinv(K)           (A3, A4)
//   SepiaEmulatorPrediction.get_y(): y = (w K) sd + mu                              (A9)
// GEMM: 64x64 output tiles, 256 threads = 4 waves (2x2 of 32x32, v_mfma_f64_16x16x4_f64),
// K staged through LDS 64 at a time with operand transposition folded into the staging;
// split-K over grid.z writes partial slabs that a second kernel reduces deterministically
// (no atomics), so X X^T with K = 1.35M still fills all 256 CUs.
#include "gpfit_common.h"
#include "../../include/gpfit.h"

namespace {

constexpr int TB = 64;
constexpr int TP = TB + 1;

// Operand staging of one 64 x 64 K-step: S[k][x] = op(M)(x, k) for the block at (x0, k0);
// NAT: M[x + k*ld], TRN: M[k + x*ld].  Thread slot q reads element (fast, slow) = (g & 63,
// g >> 6), g = tid + 256 q, so a wave reads 64 consecutive elements of memory; the element type
// E (double, or float widened exactly on load -- the fit's float32 ensembles are read as
// stored, without an fp64 copy) only changes the load.  Split in two phases so the next
// K-step's loads are in flight while the current one's MFMAs run.
template <bool TRN, typename E>
GP_DEV void stage_load(double (&r)[16], const E* __restrict__ M, int ld, int x0, int xmax,
                       int k0, int kmax) {
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int g = threadIdx.x + 256 * q;
    const int fast = g & (TB - 1), slow = g >> 6;
    int x, k;
    if (!TRN) { x = fast; k = slow; } else { k = fast; x = slow; }
    const int gx = x0 + x, gk = k0 + k;
    r[q] = (gx < xmax && gk < kmax)
               ? static_cast<double>(TRN ? M[gk + (long long)gx * ld] : M[gx + (long long)gk * ld])
               : 0.0;
  }
}

template <bool TRN>
GP_DEV void stage_store(double* S, const double (&r)[16]) {
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int g = threadIdx.x + 256 * q;
    const int fast = g & (TB - 1), slow = g >> 6;
    const int x = TRN ? slow : fast, k = TRN ? fast : slow;
    S[k * TP + x] = r[q];
  }
}

// The C update of the general kernel and of both split-K reductions: alpha v + beta c with
// beta c rounded first, and c not read at beta = 0 (it may hold NaN).
GP_DEV void gemm_store(double* c, double v, double alpha, double beta) {
  *c = (beta == 0.0) ? alpha * v : fma(alpha, v, beta * *c);
}

// opA(i,k): transa=0 -> A[i + k*lda] (NAT staging), 1 -> A[k + i*lda] (TRN staging)
// opB(k,j): transb=0 -> B[k + j*ldb] (TRN staging), 1 -> B[j + k*ldb] (NAT staging)
template <int TA, int TBT, typename EA, typename EB>
__global__ __launch_bounds__(256) void gemm_kernel(int M, int N, int K, int kchunk,
                                                   const EA* __restrict__ A, int lda,
                                                   const EB* __restrict__ B, int ldb,
                                                   double alpha, double beta,
                                                   double* __restrict__ C, int ldc,
                                                   double* __restrict__ part) {
  __shared__ double As[TB * TP];
  __shared__ double Bs[TB * TP];
  const int tilesM = gp_ceil_div(M, TB);
  const int ti = blockIdx.x % tilesM, tj = blockIdx.x / tilesM;
  const int i0 = ti * TB, j0 = tj * TB;
  const int kb = blockIdx.z * kchunk, ke = min(K, kb + kchunk);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wr = w >> 1, wc = w & 1, li = lane & 15, lk = lane >> 4;
  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = zero4();
  double ra[16], rb[16];
  if (kb < ke) {
    stage_load<TA != 0>(ra, A, lda, i0, M, kb, ke);
    stage_load<TBT == 0>(rb, B, ldb, j0, N, kb, ke);
  }
  for (int k0 = kb; k0 < ke; k0 += TB) {
    stage_store<TA != 0>(As, ra);
    stage_store<TBT == 0>(Bs, rb);
    __syncthreads();
    if (k0 + TB < ke) {          // the next K-step's operands, in flight under the MFMAs
      stage_load<TA != 0>(ra, A, lda, i0, M, k0 + TB, ke);
      stage_load<TBT == 0>(rb, B, ldb, j0, N, k0 + TB, ke);
    }
#pragma unroll 4
    for (int k4 = 0; k4 < TB / 4; ++k4) {
      const int k = k4 * 4 + lk;
      const double a0 = As[k * TP + wr * 32 + li], a1 = As[k * TP + wr * 32 + 16 + li];
      const double b0 = Bs[k * TP + wc * 32 + li], b1 = Bs[k * TP + wc * 32 + 16 + li];
      acc[0][0] = mfma16x16x4(a0, b0, acc[0][0]);
      acc[0][1] = mfma16x16x4(a0, b1, acc[0][1]);
      acc[1][0] = mfma16x16x4(a1, b0, acc[1][0]);
      acc[1][1] = mfma16x16x4(a1, b1, acc[1][1]);
    }
    __syncthreads();
  }
  // transpose through LDS for coalesced column-major stores
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 2; ++nj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wr * 32 + mi * 16 + lk + 4 * r, col = wc * 32 + nj * 16 + li;
        As[col * TP + row] = acc[mi][nj][r];
      }
  __syncthreads();
  for (int g = threadIdx.x; g < TB * TB; g += 256) {
    const int row = g & (TB - 1), col = g >> 6;
    const int gi = i0 + row, gj = j0 + col;
    if (gi >= M || gj >= N) continue;
    const double v = As[col * TP + row];
    if (part) {
      part[(long long)blockIdx.z * M * N + gi + (long long)gj * M] = v;
    } else {
      gemm_store(C + gi + (long long)gj * ldc, v, alpha, beta);
    }
  }
}

__global__ void splitk_reduce_kernel(const double* __restrict__ part, int splits, int M, int N,
                                     double alpha, double beta, double* __restrict__ C,
                                     int ldc) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)M * N) return;
  const int gi = (int)(idx % M), gj = (int)(idx / M);
  double s = 0.0;
  for (int p = 0; p < splits; ++p) s += part[(long long)p * M * N + idx];
  gemm_store(C + gi + (long long)gj * ldc, s, alpha, beta);
}

// The tsk products' reduction (hundreds of slices over a small C: 256 x 512 x 25 at the fit):
// 32 outputs x 8 slice groups per block, group h summing its contiguous run of slices in order
// with eight loads in flight, then the eight group sums added in group order (a fixed order:
// deterministic).  splitk_reduce_kernel's thread per output summed 256 slices one load at a
// time on 50 CUs: 74 us per product (profiles/r05/r05_pmc_ts.txt).
constexpr int kRedGroups = 8;
__global__ __launch_bounds__(256) void splitk_reduce_wide_kernel(
    const double* __restrict__ part, int splits, int M, int N, double alpha, double beta,
    double* __restrict__ C, int ldc) {
  __shared__ double red[kRedGroups][33];
  const int o = threadIdx.x & 31, h = threadIdx.x >> 5;
  const long long MN = (long long)M * N;
  const long long idx = (long long)blockIdx.x * 32 + o;
  const int per = (splits + kRedGroups - 1) / kRedGroups;
  const int p0 = min(splits, h * per), p1 = min(splits, p0 + per);
  double s = 0.0;
  if (idx < MN) {
    const double* q = part + idx;
#pragma unroll 8
    for (int p = p0; p < p1; ++p) s += q[(long long)p * MN];
  }
  red[h][o] = s;
  __syncthreads();
  if (h == 0 && idx < MN) {
    double t = red[0][o];
#pragma unroll
    for (int g = 1; g < kRedGroups; ++g) t += red[g][o];
    const int gi = (int)(idx % M), gj = (int)(idx / M);
    gemm_store(C + gi + (long long)gj * ldc, t, alpha, beta);
  }
}

int choose_splits(int M, int N, int K) {
  const int tiles = gp_ceil_div(M, TB) * gp_ceil_div(N, TB);
  int s = 1;
  while (tiles * s < 512 && K / (s * 2) >= 256) s *= 2;
  return s;
}

// Per-location statistics over simulations of a C-order ensemble Y (n sims x ny locations,
// row stride ldy) — src/model.py:60-64: mu = mean(Y, 0), sd = std(Y, ddof=1, 0) floored at
// sd_floor.  Thread per location: each sweep over the n rows reads 256 consecutive locations
// per block row (coalesced); two passes (mean, then centred sum of squares) as numpy does.
__global__ __launch_bounds__(256) void simstats_kernel(const double* __restrict__ Y, int n,
                                                       int ny, long long ldy, double sd_floor,
                                                       double* __restrict__ mu,
                                                       double* __restrict__ sd) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ny) return;
  double s = 0.0;
  for (int r = 0; r < n; ++r) s += Y[(long long)r * ldy + c];
  const double mean = s / n;
  double q = 0.0;
  for (int r = 0; r < n; ++r) {
    const double t = Y[(long long)r * ldy + c] - mean;
    q = fma(t, t, q);
  }
  double v = sqrt(q / (n > 1 ? n - 1 : 1));
  if (v < sd_floor) v = sd_floor;
  mu[c] = mean;
  sd[c] = v;
}

// The same statistics for a short field (ny below kSimStatsSplitNy: a thread per location would
// leave most CUs idle -- 40 blocks at C5's 10k nodes took 252 us, profiles/r06/
// r06b_c5_kernel_stats.csv): 64 locations per block, the rows in four consecutive quarters
// summed by four thread groups, the quarter sums added in quarter order (a fixed order:
// deterministic), for the mean and then the centred sum of squares.
constexpr int kSimStatsSplitNy = 1 << 16;
__global__ __launch_bounds__(256) void simstats_split_kernel(const double* __restrict__ Y, int n,
                                                             int ny, long long ldy,
                                                             double sd_floor,
                                                             double* __restrict__ mu,
                                                             double* __restrict__ sd) {
  __shared__ double part[4][64];
  const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  const int q = (n + 3) / 4, r0 = min(n, g * q), r1 = min(n, r0 + q);
  const double* y = Y + (c < ny ? c : 0);
  double s = 0.0;
  if (c < ny)
    for (int r = r0; r < r1; ++r) s += y[(long long)r * ldy];
  part[g][cl] = s;
  __syncthreads();
  const double mean = (((part[0][cl] + part[1][cl]) + part[2][cl]) + part[3][cl]) / n;
  __syncthreads();
  double t2 = 0.0;
  if (c < ny)
    for (int r = r0; r < r1; ++r) {
      const double t = y[(long long)r * ldy] - mean;
      t2 = fma(t, t, t2);
    }
  part[g][cl] = t2;
  __syncthreads();
  if (g == 0 && c < ny) {
    const double qs = ((part[0][cl] + part[1][cl]) + part[2][cl]) + part[3][cl];
    double v = sqrt(qs / (n > 1 ? n - 1 : 1));
    if (v < sd_floor) v = sd_floor;
    mu[c] = mean;
    sd[c] = v;
  }
}

// out[r*ldo + c] = (Y[r*ldy + c] - mu[c]) / sd[c]   (inverse = 0, src/model.py:72)
// out[r*ldo + c] =  Y[r*ldy + c] * sd[c] + mu[c]    (inverse = 1, get_y's back-transform)
__global__ void standardize_kernel(const double* __restrict__ Y, int n, int ny, long long ldy,
                                   const double* __restrict__ mu, const double* __restrict__ sd,
                                   double* __restrict__ out, long long ldo, int inverse) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)n * ny) return;
  const int r = (int)(idx / ny), c = (int)(idx % ny);
  const double y = Y[(long long)r * ldy + c];
  out[(long long)r * ldo + c] = inverse ? fma(y, sd[c], mu[c]) : (y - mu[c]) / sd[c];
}

// A[i][i] += factor * trace(A) — the shift of shifted CholeskyQR (one block).
__global__ __launch_bounds__(256) void shift_diag_kernel(double* __restrict__ A, int r, int lda,
                                                         double factor) {
  __shared__ double red[4];
  double t = 0.0;
  for (int i = threadIdx.x; i < r; i += 256) t += A[i + (long long)i * lda];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  const double tr = (red[0] + red[1]) + (red[2] + red[3]);
  for (int i = threadIdx.x; i < r; i += 256) A[i + (long long)i * lda] += factor * tr;
}

// scale row i of a column-major (rows x cols) matrix by f[i] (or 1/f[i] when inv=1, 0 if f=0)
__global__ void rowscale_kernel(double* __restrict__ M, int rows, int cols, int ld,
                                const double* __restrict__ f, int inv) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)rows * cols) return;
  const int i = (int)(idx % rows), j = (int)(idx / rows);
  const double fi = f[i];
  const double g = inv ? (fi != 0.0 ? 1.0 / fi : 0.0) : fi;
  M[i + (long long)j * ld] *= g;
}

// Two-pass mean / variance of a long vector: grid-stride partial sums into work[blocks], one
// block reduces them; the second pass is centred (as numpy's var).
constexpr int kMVBlocks = 1024;
__global__ __launch_bounds__(256) void partial_sum_kernel(const double* __restrict__ x,
                                                          long long N,
                                                          const double* __restrict__ center,
                                                          double* __restrict__ work) {
  __shared__ double red[4];
  const double c = center ? center[0] : 0.0;
  double s = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N;
       i += (long long)gridDim.x * 256) {
    const double t = x[i] - c;
    s += center ? t * t : t;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) work[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void finish_sum_kernel(const double* __restrict__ work,
                                                         int nb, double scale,
                                                         double* __restrict__ out) {
  __shared__ double red[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) s += work[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = ((red[0] + red[1]) + (red[2] + red[3])) * scale;
}

}  // namespace

extern "C" int gp_mean_var(const double* x, long long N, int ddof, double* out, double* work,
                           hipStream_t stream) {
  if (!x) return -1;
  if (N < 1) return -2;
  if (ddof < 0 || ddof >= N) return -3;
  if (!out) return -4;
  if (!work) return -5;
  const int nb = (int)((N + 255) / 256 < kMVBlocks ? (N + 255) / 256 : kMVBlocks);
  hipLaunchKernelGGL(partial_sum_kernel, dim3(nb), dim3(256), 0, stream, x, N, nullptr, work);
  hipLaunchKernelGGL(finish_sum_kernel, dim3(1), dim3(256), 0, stream, work, nb, 1.0 / N, out);
  hipLaunchKernelGGL(partial_sum_kernel, dim3(nb), dim3(256), 0, stream, x, N, out, work);
  hipLaunchKernelGGL(finish_sum_kernel, dim3(1), dim3(256), 0, stream, work, nb,
                     1.0 / (double)(N - ddof), out + 1);
  GP_CK(hipGetLastError());
  return 0;
}

extern "C" int gp_shift_diag(double* A, int r, int lda, double factor, hipStream_t stream) {
  if (!A) return -1;
  if (r < 0) return -2;
  if (lda < r || lda < 1) return -3;
  if (r == 0) return 0;
  hipLaunchKernelGGL(shift_diag_kernel, dim3(1), dim3(256), 0, stream, A, r, lda, factor);
  GP_CK(hipGetLastError());
  return 0;
}

extern "C" int gp_rowscale(double* M, int rows, int cols, int ld, const double* f, int inv,
                           hipStream_t stream) {
  if (!M) return -1;
  if (rows < 0) return -2;
  if (cols < 0) return -3;
  if (ld < rows || ld < 1) return -4;
  if (!f) return -5;
  if (rows == 0 || cols == 0) return 0;
  const long long tot = (long long)rows * cols;
  hipLaunchKernelGGL(rowscale_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream,
                     M, rows, cols, ld, f, inv);
  GP_CK(hipGetLastError());
  return 0;
}

namespace {

// ---- Tall-skinny products of the randomized SVD (src/svd.py:52-64 at the fit's shapes) ------
// The four products that stream the ensemble X (n_sims x ny, C-order: ny = 1,347,945 at the
// fit's 512 runs) against r = p + k <= 32 test vectors read X once each and are HBM-bound
// (5.5 GB in fp64; their fp64 MFMA time at r padded to 32 is ~0.6 ms, the read ~0.9 ms at
// 6 TB/s).  The 64 x 64-tile GEMM above reached 0.20-0.35 of HBM on them (r = 25 of 64 tile
// columns, one K-step of staging in flight: profiles/r04/r04k_prof_pca.log).  Two kernels keep
// the narrow side in registers / L2 and stream X with many loads in flight:
//   tsk (C = X W, K = ny long, C small): every block owns one K-slice of kTskRows rows, each
//       wave 64 rows (4 row tiles x 2 column tiles of 16 in MFMA accumulators).  X is loaded
//       row-contiguous (8 lanes read one row's K-group, 8 rows per load), groups ahead in a
//       register ring, and transposed into the MFMA A layout through a wave-private LDS tile;
//       partial C per slice, then splitk_reduce_wide_kernel (fixed order: deterministic).
//       gemm_tsk_kernel<EP, EW, V16> is the one kernel, in two forms that sum the same products
//       in the same order (same bits):
//         8-B form  (V16 = 0, any operand types): a lane loads one element, groups of 8 k (64 B
//                   per row), X and W both three groups ahead;
//         16-B form (V16 = 1, an fp64 X whose rows start 16-B aligned -- ts_vec_ok; the fit's
//                   y_std is allocated with a padded row stride, emulator.py standardize_y): a
//                   lane loads a pair, groups of 16 k (128 B per row), X two groups ahead, W one.
//       (Round 5's first tsk loaded X straight into the A layout -- 16 rows x 32 B per load --
//       and reached 0.19-0.25 of HBM: profiles/r05/r05g_prof_pca.log.)
//   tsm (C = X^T Y or Q^T X, the big side is the output): every block owns kTsmRows rows of the
//       big dimension and the whole K <= kTsmMaxK (the narrow operand read through L1 / L2),
//       two blocks per CU; the accumulators go through LDS so the output is written as
//       contiguous runs.
// The operands' element types are template parameters (float32 X read as stored and widened
// exactly, as the general kernel does), so float32 and fp64 operands give the same bits.
constexpr int kTskWaves = 4;                   // waves per tsk block, 64 rows each
constexpr int kTskRows = 64 * kTskWaves;       // rows of C per tsk block
constexpr int kTskMinK = 1 << 16;
// 256 rows (4 waves x 64) at two blocks per CU: 0.53-0.56 of HBM on the fit's products, against
// 0.42-0.47 at 128 x 3, 0.29-0.31 at 64 x 4, 0.48-0.49 at 512 x 1 (profiles/r05/r05w_tsm*.log)
constexpr int kTsmRows = 256;    // rows of the big dimension per tsm block
constexpr int kTsmOcc = 2;       // blocks per CU (launch_bounds' waves per SIMD at 4 waves)
constexpr int kTsmMaxK = 1024;   // K of a tsm product (the number of runs)
constexpr int kTsMaxN = 32;          // narrow side (two 16-wide MFMA column tiles)

// K-groups (16 k each) in flight ahead of the one being multiplied (a ring of kTsRing register
// buffers, indexed at compile time: the loops below are unrolled over the ring)
constexpr int kTsRing = 3;    // tsm

// The narrow operand W(k, j) = W[k*wk + j*wj] as one lane reads it: columns li and 16 + li of
// the two MFMA column tiles.  c0 / c1 point at those columns clamped to N - 1 (N < 16 too): the
// unmasked form then multiplies a finite column into C columns >= N that are never stored, and
// every stored element sums the same products in the same order as the masked form (same bits).
template <typename E>
struct TsNarrow {
  const E *c0, *c1;
  long long wk;
  bool ok0, ok1;     // the column itself is < N
};

template <typename E>
GP_DEV TsNarrow<E> ts_narrow(const E* __restrict__ W, long long wk, long long wj, int li, int N) {
  const int j0 = li, j1 = 16 + li;
  return {W + (j0 < N ? j0 : N - 1) * wj, W + (j1 < N ? j1 : N - 1) * wj, wk, j0 < N, j1 < N};
}

// bb[u][0..1] = the lane's two columns of W at k + 4u, u < U.  FULL: no masks and one 64-bit
// offset per group; otherwise zero at k + 4u >= ke and in columns >= N.
template <bool FULL, int U, typename E>
GP_DEV void ts_load_narrow(double (&bb)[U][2], const TsNarrow<E>& w, int k, int ke) {
  if constexpr (FULL) {
    const long long wo = (long long)k * w.wk, wk4 = 4LL * w.wk;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      bb[u][0] = static_cast<double>(w.c0[wo + u * wk4]);
      bb[u][1] = static_cast<double>(w.c1[wo + u * wk4]);
    }
  } else {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ku = k + 4 * u;
      const bool ok = ku < ke;
      bb[u][0] = (ok && w.ok0) ? static_cast<double>(w.c0[ku * w.wk]) : 0.0;
      bb[u][1] = (ok && w.ok1) ? static_cast<double>(w.c1[ku * w.wk]) : 0.0;
    }
  }
}

// C(i, j) = sum_k P(i, k) W(k, j) for i < M (P(i,k) = P[k + i*ldp], contiguous in k), j < N <= 32,
// W(k, j) = W[k*wk + j*wj], k in this block's slice; partial C to part[slice][j*M + i].
// A lane's load slot is (k offset EL c, row offset rr) = (lane & 7, lane >> 3): 8 lanes read
// one row's G = 8 EL consecutive k, a load covers 8 rows, eight loads a wave's 64.
template <typename EP, typename EW, bool V16>
__global__ __launch_bounds__(64 * kTskWaves, 8 / kTskWaves) void gemm_tsk_kernel(
    int M, int N, int K, int kslice, const EP* __restrict__ P, int ldp,
    const EW* __restrict__ W, long long wk, long long wj, double* __restrict__ part) {
  static_assert(!V16 || std::is_same<EP, double>::value, "the 16-B form loads fp64 pairs");
  constexpr int EL = V16 ? 2 : 1;               // elements per lane and load
  constexpr int G = 8 * EL;                     // k per group
  constexpr int RX = V16 ? 3 : 4;               // X ring: loaded RX - 1 groups ahead
  constexpr int RW = V16 ? 2 : 4;               // W ring: loaded RW - 1 groups ahead
  constexpr int UN = V16 ? 6 : 4;               // lcm(RX, RW): the unrolled ring
  constexpr int PITCH = V16 ? 68 : 72;          // LDS transpose: doubles per k row of a wave's tile
  using XV = std::conditional_t<V16, double2, double>;
  __shared__ double xs[kTskWaves * G * PITCH];
  const int slice = blockIdx.x, rg = blockIdx.y;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int li = lane & 15, ks = lane >> 4;
  const int c = lane & 7, rr = lane >> 3;
  const int kb = slice * kslice, ke = min(K, kb + kslice);
  const int row0 = rg * kTskRows + w * 64;
  double* xw = xs + w * G * PITCH;
  f64x4 acc[4][2];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t][0] = acc[t][1] = zero4();
  // load q of a group: row row0 + 8 q + rr, k = k0 + EL c (+ 1); rows >= M masked (never read)
  const EP* lrow = P + (long long)(row0 + rr) * ldp + EL * c;
  const long long qstep = 8LL * ldp;
  const TsNarrow<EW> wn = ts_narrow(W, wk, wj, li, N);
  XV xr[RX][8];
  double bv[RW][G / 4][2];
  // FULL (the block's rows < M and its k range whole groups: all but a product's last slice):
  // loads without per-lane masks and one 64-bit multiply per W group, as in tsm (the masked
  // form spent more instructions on exec-mask branches and 64-bit address arithmetic than on
  // MFMAs: profiles/r05/r05_pmc_ts.txt, MFMA busy 0.49).
  auto run = [&](auto fullc) {
    constexpr bool FULL = decltype(fullc)::value;
    auto load_x = [&](XV (&xb)[8], int k0) {
      const EP* lk = lrow + k0;
      const int k = k0 + EL * c;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const bool ok = FULL || (k < ke && row0 + 8 * q + rr < M);
        if constexpr (V16) {
          // (k even < ke: the pair's second element is inside the padded row; zeroed past ke)
          double2 v = make_double2(0.0, 0.0);
          if (ok) v = *reinterpret_cast<const double2*>(lk + q * qstep);
          if (!FULL && k + 1 >= ke) v.y = 0.0;
          xb[q] = v;
        } else {
          xb[q] = ok ? static_cast<double>(lk[q * qstep]) : 0.0;
        }
      }
    };
    auto load_w = [&](double (&bb)[G / 4][2], int k0) {
      ts_load_narrow<FULL>(bb, wn, k0 + ks, ke);
    };
    // prologue: only groups inside the slice (FULL loads are unmasked: a group at or past ke
    // would read up to 16 k past the slice, i.e. past X's last row and W's last k)
    static_for<0, (RX > RW ? RX : RW) - 1, 1>([&](auto Q) {
      constexpr int q = decltype(Q)::value;
      if (kb + G * q < ke) {
        if constexpr (q < RX - 1) load_x(xr[q], kb + G * q);
        if constexpr (q < RW - 1) load_w(bv[q], kb + G * q);
      }
    });
    for (int k0 = kb; k0 < ke; k0 += G * UN) {
      static_for<0, UN, 1>([&](auto Q) {
        constexpr int q = decltype(Q)::value;
        const int kq = k0 + G * q;
        if (kq >= ke) return;
        if (kq + G * (RX - 1) < ke) load_x(xr[(q + RX - 1) % RX], kq + G * (RX - 1));
        if (kq + G * (RW - 1) < ke) load_w(bv[(q + RW - 1) % RW], kq + G * (RW - 1));
        // transpose: xw[k][row] (one wave's LDS: its own DS instructions run in order)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          if constexpr (V16) {
            xw[(2 * c) * PITCH + 8 * i + rr] = xr[q % RX][i].x;
            xw[(2 * c + 1) * PITCH + 8 * i + rr] = xr[q % RX][i].y;
          } else {
            xw[c * PITCH + 8 * i + rr] = xr[q % RX][i];
          }
        }
#pragma unroll
        for (int u = 0; u < G / 4; ++u) {
          double a[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) a[t] = xw[(4 * u + ks) * PITCH + 16 * t + li];
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            acc[t][0] = mfma16x16x4(a[t], bv[q % RW][u][0], acc[t][0]);
            acc[t][1] = mfma16x16x4(a[t], bv[q % RW][u][1], acc[t][1]);
          }
        }
      });
    }
  };
  if (rg * kTskRows + kTskRows <= M && (ke - kb) % G == 0) run(std::true_type{});
  else run(std::false_type{});
  // C layout: lane l, reg q holds C[(l >> 4) + 4q][l & 15] of each 16 x 16 tile
  double* pp = part + (long long)slice * M * N;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = row0 + 16 * t + ks + 4 * q, j = 16 * jt + li;
        if (r < M && j < N) pp[(long long)j * M + r] = acc[t][jt][q];
      }
}

// C(i, j) = alpha sum_k P(i, k) Q(k, j) + beta C(i, j) for i < M (P(i,k) = P[i + k*ldp],
// contiguous in i), j < N <= 32, k < K <= kTsmMaxK, Q(k, j) = Q[k*qk + j*qj] (read through L1 /
// L2: 100 KB at the fit's 512 x 25), C(i, j) = C[i*ci + j*cj].  The block's rows are written
// through LDS as runs along whichever of i / j is contiguous in C.
template <typename EP, typename EQ>
__global__ __launch_bounds__(256, kTsmOcc) void gemm_tsm_kernel(int M, int N, int K,
                                                          const EP* __restrict__ P, int ldp,
                                                          const EQ* __restrict__ Q, long long qk,
                                                          long long qj, double alpha,
                                                          double beta, double* __restrict__ C,
                                                          long long ci, long long cj) {
  __shared__ double cs[kTsmRows * 33];            // the block's C rows, pitch 33
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int li = lane & 15, ks = lane >> 4;
  const long long i0 = (long long)blockIdx.x * kTsmRows;
  constexpr int T = kTsmRows / 64;                // row tiles of 16 per wave
  f64x4 acc[T][2];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t][0] = acc[t][1] = zero4();
  const long long rbase = i0 + w * 16 * T;
  const EP* pcol[T];
  bool rok[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const long long r = rbase + 16 * t + li;
    rok[t] = r < M;
    pcol[t] = P + (rok[t] ? r : 0);
  }
  // K-group of 16: lane (row li, slot ks) holds k = k0 + 4u + ks of its 4 row tiles.
  // FULL (every block row < M and K % 16 == 0, i.e. all but a product's last block): no
  // per-load masks and one 64-bit address per (group, u) -- the masked form's per-load
  // exec-mask branches and 64-bit multiplies outnumbered its MFMAs (r05_pmc_ts.txt: MFMA busy
  // 0.46 with waves waiting only 19% of their cycles).
  const long long ldp4 = 4LL * ldp;
  const TsNarrow<EQ> qn = ts_narrow(Q, qk, qj, li, N);
  double a[kTsRing][T][4], bv[kTsRing][4][2];
  auto run = [&](auto fullc) {
    constexpr bool FULL = decltype(fullc)::value;
    auto load = [&](double (&ab)[T][4], double (&bb)[4][2], int k0) {
      if constexpr (FULL) {
        const EP* pk = P + rbase + li + (long long)(k0 + ks) * ldp;
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int t = 0; t < T; ++t) ab[t][u] = static_cast<double>(pk[u * ldp4 + 16 * t]);
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = k0 + 4 * u + ks;
#pragma unroll
          for (int t = 0; t < T; ++t)
            ab[t][u] = (k < K && rok[t]) ? static_cast<double>(pcol[t][(long long)k * ldp]) : 0.0;
        }
      }
      ts_load_narrow<FULL>(bb, qn, k0 + ks, K);
    };
    // prologue: only groups < K (FULL loads are unmasked; K = 16 would otherwise read P's
    // columns and Q's rows 16..31, past both operands)
#pragma unroll
    for (int q = 0; q < kTsRing - 1; ++q)
      if (16 * q < K) load(a[q], bv[q], 16 * q);
    for (int k0 = 0; k0 < K; k0 += 16 * kTsRing) {
#pragma unroll
      for (int q = 0; q < kTsRing; ++q) {
        const int kq = k0 + 16 * q;
        if (kq >= K) break;
        const int kn = kq + 16 * (kTsRing - 1);
        if (kn < K) load(a[(q + kTsRing - 1) % kTsRing], bv[(q + kTsRing - 1) % kTsRing], kn);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int t = 0; t < T; ++t) {
            acc[t][0] = mfma16x16x4(a[q][t][u], bv[q][u][0], acc[t][0]);
            acc[t][1] = mfma16x16x4(a[q][t][u], bv[q][u][1], acc[t][1]);
          }
      }
    }
  };
  if (i0 + kTsmRows <= M && K % 16 == 0) run(std::true_type{});
  else run(std::false_type{});
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        cs[(w * 16 * T + 16 * t + ks + 4 * q) * 33 + 16 * jt + li] = acc[t][jt][q];
  __syncthreads();
  // not gemm_store: this kernel has always rounded alpha v first and then fused beta c into it;
  // the general kernel rounds beta c first.  Merging the two would change the bits of one.
  const int rows = (int)min((long long)kTsmRows, M - i0);
  if (cj == 1) {                                // C(i, j) runs along j: rows of N doubles
    for (int e = threadIdx.x; e < rows * N; e += 256) {
      const int r = e / N, j = e - r * N;
      double* c = C + (i0 + r) * ci + j;
      const double v = alpha * cs[r * 33 + j];
      *c = (beta == 0.0) ? v : fma(beta, *c, v);
    }
  } else {                                      // runs along i: one column at a time
    for (int e = threadIdx.x; e < rows * N; e += 256) {
      const int j = e / rows, r = e - j * rows;
      double* c = C + (i0 + r) * ci + j * cj;
      const double v = alpha * cs[r * 33 + j];
      *c = (beta == 0.0) ? v : fma(beta, *c, v);
    }
  }
}

// The 16-B form applies to an fp64 big operand with a 16-B aligned base and an even leading
// dimension (a pair never reads past the row: an even ldp >= len rounds len up inside it).
// (A 16-B tsm, each lane reading rows 2i, 2i + 1 of a column, ran 2.4 vs 1.6 ms on the fit's
// products at its occupancy of 2 blocks per CU instead of 3: profiles/r05/r05j_prof_pca.log.)
template <typename E>
bool ts_vec_ok(const E* p, int ld, int len) {
  return sizeof(E) == 8 && (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld & 1) == 0 &&
         ld >= ((len + 1) & ~1);
}

// How one product runs: which kernel, over how many K ranges, and the workspace that takes.
// Filled from (transa, transb, m, n, k) alone, so the size query and the launch cannot differ.
enum GemmKind {
  kGeneral,   // gemm_kernel, split-K over `splits` chunks of kchunk (one chunk: no workspace)
  kTsk,       // transa = 1 (A's columns are C's rows), n <= 32, k >= kTskMinK: `splits` slices
  kTsm,       // transa = 0, n <= 32, k <= kTsmMaxK, m >= 8192 (the big side is C's rows)
  kTsmT,      // tsm on the transpose: transb = 1, m <= 32, k <= kTsmMaxK, n >= 8192 (C^T's rows)
};
struct GemmPlan {
  GemmKind kind;
  int splits, kchunk;   // K ranges (grid.z chunks or tsk slices) and the length of one
  int groups;           // tsk: row groups of kTskRows
  long long ws_bytes;   // partial slabs; 0: the product needs no workspace
};

GemmPlan plan_general(int m, int n, int k, bool split) {
  GemmPlan p = {kGeneral, 1, TB, 0, 0};
  if (k <= 0) return p;
  const int s = split ? choose_splits(m, n, k) : 1;
  p.kchunk = gp_ceil_div(gp_ceil_div(k, s), TB) * TB;
  p.splits = gp_ceil_div(k, p.kchunk);
  if (s > 1) p.ws_bytes = (long long)s * m * n * 8;
  return p;
}

GemmPlan gemm_plan(int transa, int transb, int m, int n, int k) {
  if (transa == 1 && n <= kTsMaxN && k >= kTskMinK) {
    // K slices: eight waves per CU over all row groups, each slice a multiple of 16
    GemmPlan p = {kTsk, 0, 0, gp_ceil_div(m, kTskRows), 0};
    p.kchunk = gp_ceil_div(gp_ceil_div(k, max(1, (2048 / kTskWaves) / p.groups)), 16) * 16;
    p.splits = gp_ceil_div(k, p.kchunk);
    p.ws_bytes = (long long)p.splits * m * n * 8;
    return p;
  }
  if (k > 0 && k <= kTsmMaxK) {
    if (transa == 0 && n <= kTsMaxN && m >= 8192) return {kTsm, 1, k, 0, 0};
    if (transb == 1 && m <= kTsMaxN && n >= 8192) return {kTsmT, 1, k, 0, 0};
  }
  return plan_general(m, n, k, true);
}

// f(EA{}, EB{}) with the element types that (a_f32, b_f32) name
template <class F>
void with_elem_types(int a_f32, int b_f32, F&& f) {
  if (a_f32 && b_f32) f(float{}, float{});
  else if (a_f32) f(float{}, double{});
  else if (b_f32) f(double{}, float{});
  else f(double{}, double{});
}

struct GemmArgs {
  int transa, transb, m, n, k;
  double alpha;
  const void* A;
  int lda;
  const void* B;
  int ldb;
  double beta;
  double* C;
  int ldc;
  double* part;
  hipStream_t stream;
};

template <typename EA, typename EB>
hipError_t launch_gemm(const GemmPlan& p, const GemmArgs& g) {
  const EA* a = static_cast<const EA*>(g.A);
  const EB* b = static_cast<const EB*>(g.B);
  const int m = g.m, n = g.n, k = g.k;
  const long long tot = (long long)m * n;
  if (p.kind == kTsk) {
    // W(k, j) = opB(k, j): transb 0 -> B[k + j*ldb], 1 -> B[j + k*ldb]
    const long long wk = g.transb ? g.ldb : 1, wj = g.transb ? 1 : g.ldb;
    constexpr bool can16 = sizeof(EA) == 8;
    auto kern = (can16 && ts_vec_ok(a, g.lda, k)) ? gemm_tsk_kernel<EA, EB, can16>
                                                  : gemm_tsk_kernel<EA, EB, false>;
    hipLaunchKernelGGL(kern, dim3(p.splits, p.groups), dim3(64 * kTskWaves), 0, g.stream, m, n, k,
                       p.kchunk, a, g.lda, b, wk, wj, g.part);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(splitk_reduce_wide_kernel, dim3((unsigned)((tot + 31) / 32)), dim3(256), 0,
                       g.stream, g.part, p.splits, m, n, g.alpha, g.beta, g.C, g.ldc);
  } else if (p.kind == kTsm) {
    // C(i, j) = sum_k A[i + k*lda] opB(k, j), C[i + j*ldc]
    const long long qk = g.transb ? g.ldb : 1, qj = g.transb ? 1 : g.ldb;
    hipLaunchKernelGGL((gemm_tsm_kernel<EA, EB>), dim3(gp_ceil_div(m, kTsmRows)), dim3(256), 0,
                       g.stream, m, n, k, a, g.lda, b, qk, qj, g.alpha, g.beta, g.C, 1LL,
                       (long long)g.ldc);
  } else if (p.kind == kTsmT) {
    // C^T(j, i) = sum_k B[j + k*ldb] opA(i, k), C[i + j*ldc]: the big operand is B
    const long long qk = g.transa ? 1 : g.lda, qj = g.transa ? g.lda : 1;
    hipLaunchKernelGGL((gemm_tsm_kernel<EB, EA>), dim3(gp_ceil_div(n, kTsmRows)), dim3(256), 0,
                       g.stream, n, m, k, b, g.ldb, a, qk, qj, g.alpha, g.beta, g.C,
                       (long long)g.ldc, 1LL);
  } else {
    double* part = p.splits > 1 ? g.part : nullptr;
    const dim3 grid(gp_ceil_div(m, TB) * gp_ceil_div(n, TB), 1, p.splits);
#define GP_GEMM(TA_, TB_)                                                                     \
  hipLaunchKernelGGL((gemm_kernel<TA_, TB_, EA, EB>), grid, dim3(256), 0, g.stream, m, n, k,   \
                     p.kchunk, a, g.lda, b, g.ldb, g.alpha, g.beta, g.C, g.ldc, part)
    if (g.transa == 0 && g.transb == 0) GP_GEMM(0, 0);
    else if (g.transa == 0 && g.transb == 1) GP_GEMM(0, 1);
    else if (g.transa == 1 && g.transb == 0) GP_GEMM(1, 0);
    else GP_GEMM(1, 1);
#undef GP_GEMM
    if (!part) return hipGetLastError();
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0,
                       g.stream, part, p.splits, m, n, g.alpha, g.beta, g.C, g.ldc);
  }
  return hipGetLastError();
}

}  // namespace

// The largest need over the plans a product of this size can be given: the general kernel's
// split-K (any trans pair, and what a tsk product falls back to) and tsk's slices (transa = 1).
extern "C" long long gp_dgemm_ws_bytes(int m, int n, int k) {
  if (m <= 0 || n <= 0 || k <= 0) return 0;
  return max(plan_general(m, n, k, true).ws_bytes, gemm_plan(1, 0, m, n, k).ws_bytes);
}

extern "C" int gp_gemm_ex(int transa, int transb, int m, int n, int k, double alpha,
                          const void* A, int a_f32, int lda, const void* B, int b_f32, int ldb,
                          double beta, double* C, int ldc, void* ws, long long ws_bytes,
                          hipStream_t stream) {
  if (transa != 0 && transa != 1) return -1;
  if (transb != 0 && transb != 1) return -2;
  if (m < 0) return -3;
  if (n < 0) return -4;
  if (k < 0) return -5;
  if (!A && k > 0) return -7;
  if (a_f32 != 0 && a_f32 != 1) return -8;
  if (lda < (transa ? k : m) || lda < 1) return -9;
  if (!B && k > 0) return -10;
  if (b_f32 != 0 && b_f32 != 1) return -11;
  if (ldb < (transb ? n : k) || ldb < 1) return -12;
  if (!C) return -14;
  if (ldc < m || ldc < 1) return -15;
  if (m == 0 || n == 0) return 0;
  // without the workspace its plan needs, a tsk product runs as general GEMM and split-K unsplit
  auto fits = [&](const GemmPlan& p) { return p.ws_bytes == 0 || (ws && ws_bytes >= p.ws_bytes); };
  GemmPlan p = gemm_plan(transa, transb, m, n, k);
  if (p.kind == kTsk && !fits(p)) p = plan_general(m, n, k, true);
  if (!fits(p)) p = plan_general(m, n, k, false);
  const GemmArgs g = {transa, transb, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc,
                      static_cast<double*>(ws), stream};
  hipError_t e = hipSuccess;
  with_elem_types(a_f32, b_f32, [&](auto ea, auto eb) {
    e = launch_gemm<decltype(ea), decltype(eb)>(p, g);
  });
  GP_CK(e);
  return 0;
}

extern "C" int gp_dgemm(int transa, int transb, int m, int n, int k, double alpha,
                        const double* A, int lda, const double* B, int ldb, double beta,
                        double* C, int ldc, void* ws, long long ws_bytes, hipStream_t stream) {
  const int rc = gp_gemm_ex(transa, transb, m, n, k, alpha, A, 0, lda, B, 0, ldb, beta, C, ldc,
                            ws, ws_bytes, stream);
  // keep gp_dgemm's documented argument numbers (A, lda = 7, 8; B, ldb = 9, 10; C, ldc = 12, 13)
  static const int remap[16] = {0, -1, -2, -3, -4, -5, 0, -7, 0, -8, -9, 0, -10, 0, -12, -13};
  return (rc < 0 && rc > -16) ? remap[-rc] : rc;
}

extern "C" int gp_sim_stats(const double* Y, int n, int ny, long long ldy, double sd_floor,
                            double* mu, double* sd, hipStream_t stream) {
  if (!Y) return -1;
  if (n < 1) return -2;
  if (ny < 0) return -3;
  if (ldy < ny) return -4;
  if (!mu) return -6;
  if (!sd) return -7;
  if (ny == 0) return 0;
  if (ny < kSimStatsSplitNy)
    hipLaunchKernelGGL(simstats_split_kernel, dim3(gp_ceil_div(ny, 64)), dim3(256), 0, stream, Y,
                       n, ny, ldy, sd_floor, mu, sd);
  else
    hipLaunchKernelGGL(simstats_kernel, dim3(gp_ceil_div(ny, 256)), dim3(256), 0, stream, Y, n,
                       ny, ldy, sd_floor, mu, sd);
  GP_CK(hipGetLastError());
  return 0;
}

extern "C" int gp_standardize(const double* Y, int n, int ny, long long ldy, const double* mu,
                              const double* sd, double* out, long long ldo, int inverse,
                              hipStream_t stream) {
  if (!Y) return -1;
  if (n < 0) return -2;
  if (ny < 0) return -3;
  if (ldy < ny) return -4;
  if (!mu) return -5;
  if (!sd) return -6;
  if (!out) return -7;
  if (ldo < ny) return -8;
  if (n == 0 || ny == 0) return 0;
  const long long tot = (long long)n * ny;
  hipLaunchKernelGGL(standardize_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0,
                     stream, Y, n, ny, ldy, mu, sd, out, ldo, inverse);
  GP_CK(hipGetLastError());
  return 0;
}
