// Analytic gradient of the GP negative log-likelihood from the L^-1 of gp_potrf_inv.
//
// Reference replaced: GPmodule.GP.fit hands scipy's BFGS a bare objective, so scipy takes every
// gradient by forward differences of it (examples/02_univariate_GP_regression.ipynb:80-85): d + 1
// further Gram -> factorisation -> nll chains per gradient, each only cond(K) eps accurate.
//
// With NLL = 1/2 w^T K^-1 w + 1/2 log|K| (gp_nll), K = s R + delta I, R_ij = exp(-sum_k beta_k
// D_ijk^2), D_ijk = X[i,k] - X[j,k], alpha = K^-1 w (gp_alpha) and W = K^-1 - alpha alpha^T:
//   dNLL/ds      =  1/2 sum_ij W_ij R_ij
//   dNLL/ddelta  =  1/2 sum_i  W_ii
//   dNLL/dbeta_k = -1/2 s sum_ij W_ij R_ij D_ijk^2
//
// Per call of gp_nll_grad, no n x n matrix is stored:
//   1. ng_tile   one lower 64 x 64 tile (I, J <= I) of one problem per block: acc = the tile of
//                K^-1 = L^-T L^-1 = sum_{k >= I0} L^-1[k, I0 + i] L^-1[k, J0 + j] on
//                v_mfma_f64_16x16x4_f64 (the k-range is triangular: n^3 / 3 flop for the whole
//                product), columns of L^-1 masked to c <= k < n while they are staged; epilogue:
//                W = acc - alpha_i alpha_j, R recomputed from X and beta in the scaled-difference
//                form (ard_dist), the d + 2 sums over the tile (an off-diagonal element counts
//                twice, inside a diagonal tile only j <= i) into the workspace
//   2. ng_sum    the tiles' partial sums added in ascending tile order, scaled, into grad
// One block per tile with k ascending, a fixed reduction tree inside the block and a serial sum
// over the tiles: no atomics, so equal inputs give equal bits whatever the layout and whatever
// the problem's position in the batch.
#include "gpfit_common.h"
#include "gpfit_internal.h"
#include "../../include/gpfit.h"

namespace {

// 64 x 64 tiles per 256-thread block, 4 waves as 2 x 2, each wave NT x NT MFMA tiles (the small
// tile of jointcov.hip: n = 512 gives 36 tiles per problem, a 128-edge only 10).
constexpr int NT = 2;
constexpr int T = 32 * NT;
constexpr int JK = 16;            // k per staged step
// LDS pitch of a staged column in doubles: the operands are columns of L^-1 (k contiguous), kept
// column-major in LDS; even, so a thread's 4 k go in as two 16-B stores
constexpr int PK = JK + 2;
constexpr long long kMaxBlocks = 1LL << 30;

GP_DEV int round_up(int a, int b) { return (a + b - 1) / b * b; }

struct NgArgs {
  const double* Linv;   // padded L^-1, column c at c * ld
  int ld;
  long long sL;
  const double* X;
  int ldx, n, d;
  const double* beta;
  int ldbeta;
  const double* alpha;
  int lda;
  double* part;         // partial sums: part[(b (d + 2) + e) per + t]
  int per, nb;          // lower tiles per problem, problems of this launch
  int vec;              // L^-1 16-B aligned with even ld / stride: 16-B loads
};

// Lower tile t = I (I + 1) / 2 + J of problem b.  Blocks are numbered tile-major (t = block / nb):
// a tile's k-range is n - I0, so the longest tiles of every problem are dispatched first.
// D: compile-time bound of d; D <= 8 unrolls the loops over dimensions, above that they are
// rolled (unrolling D steps for each of the 16 elements would leave the sums dynamically indexed).
template <int D>
__global__ __launch_bounds__(256) void ng_tile_kernel(const NgArgs a) {
  constexpr int XP = D + 1;
  constexpr int kStage = 2 * T * PK, kEpi = 2 * T * XP + D + 2 * T;
  __shared__ __attribute__((aligned(16))) double smem[kStage > kEpi ? kStage : kEpi];
  __shared__ double red[4][D + 2];
  double* As = smem;
  double* Bs = smem + T * PK;
  const int t = blockIdx.x / a.nb, b = blockIdx.x - t * a.nb;
  int I = (int)((__builtin_sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  while (I * (I + 1) / 2 > t) --I;
  const int J = t - I * (I + 1) / 2;
  const int I0 = I * T, J0 = J * T;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = w >> 1, wc = w & 1, li = lane & 15, lk = lane >> 4;
  const int sc = tid >> 2, sk = (tid & 3) * 4;      // staged column, first of its 4 k
  const int n = a.n, d = a.d;
  const int nsteps = (round_up(n, JK) - I0) / JK;   // k from I0: L^-1[k, I0 + i] = 0 above it
  const double* Li = a.Linv + b * a.sL + (long long)(I0 + sc) * a.ld;
  const double* Lj = a.Linv + b * a.sL + (long long)(J0 + sc) * a.ld;

  // Rows k .. k + 3 of the two staged columns.  Every address lies inside the padded buffer
  // (column < T ceil(n / T), row < 16 ceil(n / 16), both <= gp_padded_n(n)); what the buffer
  // holds above the diagonal or from row n on never reaches a product.
  double ra[4], rb[4];
  auto load = [&](int s) {
    const int k = I0 + s * JK + sk;
    const f64x2 a0 = load2(Li + k, a.vec), a1 = load2(Li + k + 2, a.vec);
    const f64x2 b0 = load2(Lj + k, a.vec), b1 = load2(Lj + k + 2, a.vec);
    const double va[4] = {a0.x, a0.y, a1.x, a1.y}, vb[4] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      ra[q] = (k + q >= I0 + sc && k + q < n) ? va[q] : 0.0;
      rb[q] = (k + q >= J0 + sc && k + q < n) ? vb[q] : 0.0;
    }
  };

  f64x4 acc[NT][NT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = zero4();

  load(0);
  for (int s = 0; s < nsteps; ++s) {
    __syncthreads();
    f64x2 v;
    v.x = ra[0]; v.y = ra[1];
    *reinterpret_cast<f64x2*>(As + sc * PK + sk) = v;
    v.x = ra[2]; v.y = ra[3];
    *reinterpret_cast<f64x2*>(As + sc * PK + sk + 2) = v;
    v.x = rb[0]; v.y = rb[1];
    *reinterpret_cast<f64x2*>(Bs + sc * PK + sk) = v;
    v.x = rb[2]; v.y = rb[3];
    *reinterpret_cast<f64x2*>(Bs + sc * PK + sk + 2) = v;
    __syncthreads();
    if (s + 1 < nsteps) load(s + 1);
#pragma unroll
    for (int k4 = 0; k4 < JK / 4; ++k4) {
      const int k = k4 * 4 + lk;
      double fa[NT], fb[NT];
#pragma unroll
      for (int mi = 0; mi < NT; ++mi) fa[mi] = As[((wr * NT + mi) * 16 + li) * PK + k];
#pragma unroll
      for (int nj = 0; nj < NT; ++nj) fb[nj] = Bs[((wc * NT + nj) * 16 + li) * PK + k];
#pragma unroll
      for (int mi = 0; mi < NT; ++mi) {
        // rows I0 + 16 (NT wr + mi) .. lie wholly below this step's k: only zeros (wave-uniform)
        if (wr * NT + mi > s) continue;
#pragma unroll
        for (int nj = 0; nj < NT; ++nj) acc[mi][nj] = mfma16x16x4(fa[mi], fb[nj], acc[mi][nj]);
      }
    }
  }

  __syncthreads();
  double* xi = smem;
  double* xj = smem + T * XP;
  double* bs = smem + 2 * T * XP;
  double* ai = bs + D;
  double* aj = ai + T;
  for (int e = tid; e < T * D; e += 256) {
    const int p = e / D, k = e - p * D;
    const bool ki = k < d && I0 + p < n, kj = k < d && J0 + p < n;
    xi[p * XP + k] = ki ? a.X[(long long)(I0 + p) * a.ldx + k] : 0.0;
    xj[p * XP + k] = kj ? a.X[(long long)(J0 + p) * a.ldx + k] : 0.0;
  }
  if (tid < D) bs[tid] = tid < d ? a.beta[(long long)b * a.ldbeta + tid] : 0.0;
  if (tid < T) {
    ai[tid] = I0 + tid < n ? a.alpha[(long long)b * a.lda + I0 + tid] : 0.0;
  } else if (tid < 2 * T) {
    const int p = tid - T;
    aj[p] = J0 + p < n ? a.alpha[(long long)b * a.lda + J0 + p] : 0.0;
  }
  __syncthreads();

  // wv: the element's weight (1 on the diagonal, 2 below it, 0 elsewhere) times W_ij R_ij
  double wv[NT * NT * 4];
  double ss = 0.0, sd = 0.0;
#pragma unroll
  for (int mi = 0; mi < NT; ++mi)
#pragma unroll
    for (int nj = 0; nj < NT; ++nj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int pi = (wr * NT + mi) * 16 + lk + 4 * r, pj = (wc * NT + nj) * 16 + li;
        const int i = I0 + pi, j = J0 + pj;
        double dist;
        if constexpr (D <= 8) {
          dist = ard_dist<D>(xi + pi * XP, xj + pj * XP, bs, d);
        } else {
          dist = 0.0;
#pragma unroll 1
          for (int k = 0; k < d; ++k) {
            const double tk = xi[pi * XP + k] - xj[pj * XP + k];
            dist = fma(bs[k] * tk, tk, dist);
          }
        }
        const double wij = acc[mi][nj][r] - ai[pi] * aj[pj];
        const double wr_ij = wij * exp_neg(dist);
        const bool on = i < n && j <= i;
        const double v = on ? (i == j ? wr_ij : 2.0 * wr_ij) : 0.0;
        wv[(mi * NT + nj) * 4 + r] = v;
        ss += v;
        sd += (on && i == j) ? wij : 0.0;
      }

  // sum over the tile of wv D_ijk^2: the thread's 16 elements, then the wave
  auto dim_sum = [&](int k) {
    double p = 0.0;
#pragma unroll
    for (int mi = 0; mi < NT; ++mi)
#pragma unroll
      for (int nj = 0; nj < NT; ++nj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int pi = (wr * NT + mi) * 16 + lk + 4 * r, pj = (wc * NT + nj) * 16 + li;
          const double tk = xi[pi * XP + k] - xj[pj * XP + k];
          p = fma(wv[(mi * NT + nj) * 4 + r], tk * tk, p);
        }
    p = wave_sum(p);
    if (lane == 0) red[w][2 + k] = p;
  };
  if constexpr (D <= 8) {
#pragma unroll
    for (int k = 0; k < D; ++k) dim_sum(k);     // k >= d: both points hold 0 there
  } else {
#pragma unroll 1
    for (int k = 0; k < d; ++k) dim_sum(k);
  }
  ss = wave_sum(ss);
  sd = wave_sum(sd);
  if (lane == 0) {
    red[w][0] = ss;
    red[w][1] = sd;
  }
  __syncthreads();
  if (tid < d + 2)
    a.part[((long long)b * (d + 2) + tid) * a.per + t] =
        ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// grad_b[e] = scale_e sum_t part[(b (d + 2) + e) per + t], t ascending: one thread per entry.
__global__ __launch_bounds__(64) void ng_sum_kernel(const double* __restrict__ part, int per, int d,
                                                    const double* __restrict__ s,
                                                    double* __restrict__ grad, int ldg) {
  const int b = blockIdx.x, e = threadIdx.x;
  if (e >= d + 2) return;
  const double* p = part + ((long long)b * (d + 2) + e) * per;
  double acc = 0.0;
  for (int t = 0; t < per; ++t) acc += p[t];
  grad[(long long)b * ldg + e] = e < 2 ? 0.5 * acc : -0.5 * s[b] * acc;
}

long long tiles_per_problem(int n) {
  const long long nt = gp_ceil_div(n, T);
  return nt * (nt + 1) / 2;
}

}  // namespace

extern "C" long long gp_nll_grad_ws_bytes(int n, int d, int batch) {
  if (n < 0 || d < 0 || batch < 0) return -1;
  if (n == 0 || batch == 0) return 0;
  return align256(8LL * batch * (d + 2) * tiles_per_problem(n));
}

extern "C" int gp_nll_grad(const double* Linv, int ldinv, long long strideInv, const double* X,
                           int ldx, int n, int d, const double* beta, int ldbeta,
                           const double* s, const double* alpha, int lda, double* grad, int ldg,
                           int batch, void* ws, long long ws_bytes, hipStream_t stream) {
  if (!Linv) return -1;
  if (n < 0) return -6;
  if (d < 1 || d > GPFIT_MAX_DIM) return -7;
  if (batch < 0) return -15;
  const int npad = gp_padded_n(n);
  if (ldinv < npad || ldinv < 1) return -2;
  if (batch > 1 && strideInv < (long long)ldinv * npad) return -3;
  if (!X) return -4;
  if (ldx < d) return -5;
  if (!beta) return -8;
  if (ldbeta < d && batch > 1) return -9;
  if (!s) return -10;
  if (!alpha) return -11;
  if (lda < n && batch > 1) return -12;
  if (!grad) return -13;
  if (ldg < d + 2) return -14;
  if (n == 0 || batch == 0) return 0;
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255)) return -16;
  if (ws_bytes < gp_nll_grad_ws_bytes(n, d, batch)) return -17;

  const long long per = tiles_per_problem(n);
  if (per > kMaxBlocks) return -6;
  const long long sL = batch > 1 ? strideInv : 0;
  const int ldb = batch > 1 ? ldbeta : 0, lda_ = batch > 1 ? lda : 0;
  const int chunk = (int)(kMaxBlocks / per < kMaxGridY ? kMaxBlocks / per : kMaxGridY);
  double* part = static_cast<double*>(ws);
  for (int b0 = 0; b0 < batch; b0 += chunk) {
    const int nb = batch - b0 < chunk ? batch - b0 : chunk;
    NgArgs a;
    a.Linv = Linv + b0 * sL;
    a.ld = ldinv;
    a.sL = sL;
    a.X = X;
    a.ldx = ldx;
    a.n = n;
    a.d = d;
    a.beta = beta + (long long)b0 * ldb;
    a.ldbeta = ldb;
    a.alpha = alpha + (long long)b0 * lda_;
    a.lda = lda_;
    a.part = part + (long long)b0 * (d + 2) * per;
    a.per = (int)per;
    a.nb = nb;
    a.vec = !(reinterpret_cast<uintptr_t>(Linv) & 15) && !(ldinv & 1) && !(sL & 1);
    hipLaunchKernelGGL(d <= 8 ? ng_tile_kernel<8> : ng_tile_kernel<GPFIT_MAX_DIM>,
                       dim3((unsigned)(per * nb)), dim3(256), 0, stream, a);
    GP_CK(hipGetLastError());
    hipLaunchKernelGGL(ng_sum_kernel, dim3(nb), dim3(64), 0, stream, a.part, (int)per, d, s + b0,
                       grad + (long long)b0 * ldg, ldg);
    GP_CK(hipGetLastError());
  }
  return 0;
}
