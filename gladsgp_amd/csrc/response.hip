// gp_mean_response: mean-response surfaces (main effects and input pairs) of the posterior mean
// in closed form.  With A = G + delta I, alpha = A^-1 w (gp_alpha, linalg.hip) and the
// ARD kernel a product over dimensions, the posterior mean at x_d1 = t1[a1], x_d2 = t2[a2],
// averaged over I integration points in the other dimensions, is
//   R[a2, a1] = s sum_n alpha_n M_n exp(-beta_d1 (x_n,d1 - t1[a1])^2) exp(-beta_d2 (x_n,d2 - t2[a2])^2)
//   M_n       = (1/I) sum_i exp(-sum_{k not free} beta_k (x_n,k - Xint[i, col(k)])^2)
// so no test point is ever materialised: O(n I d + n T) per main effect, a rank-n product per
// pair.  The reference (mean_response.py:82-138, 159-208) predicts at every (target,
// integration point) and averages: 8 SepiaEmulatorPrediction calls of 220 points for the main
// effects, 121 calls of 10 points per pair, each refactorising every (sample, PC) GP.
//
//   response     : one 256-thread workgroup per (problem, effect).  Xint, t1, t2 and the
//                  problem's beta are staged in LDS.  The training rows go by in chunks of 256,
//                  one row per thread: M_n with one exp per integration point on the summed
//                  exponent (eight points' exponents in registers per pass over the row), then
//                  g_n = s alpha_n M_n.  The chunk is contracted 32 rows at a time from LDS
//                  panels whose entries (one exp each) the 256 threads share:
//                    main effects  g_n E1[n,a] in the panel, lane a of wave v sums rows 8v..8v+7
//                                  in order into its own partial; the four partials are added in
//                                  wave order at the end;
//                    pairs         out += (g E2)^T E1 on v_mfma_f64_16x16x4_f64, T padded to 16
//                                  with zero columns, the <= 16 output tiles dealt over the four
//                                  waves, accumulators carried across all rows.
// No atomics, one summation order fixed by (n, I, T) alone: equal inputs give equal bits, and a
// (problem, effect) value does not depend on the batch or on the other effects.  Every load is an
// 8-B load, so the bits do not depend on the layout either.
// Rates assumed, not measured: a workgroup's work is n (I + T1 + T2) exps of ~19 fp64 VALU ops
// (exp_neg) plus n I (d - nfree) fmas; the pair MFMAs (n / 4 per tile) are a few per cent of
// that, and the global traffic (n d + n doubles) is negligible, so the kernel is bound by the
// fp64 VALU rate.  Measured on one MI355X (HIP events): 4096 GPs x 8 main effects
// at n = 512, T = 11, I = 20 in 0.96 ms, about a third of the data-sheet fp64 vector rate by the
// operation count above; 16 GPs x 8 main effects 0.043 ms and x 1 pair of 11 x 11 0.049 ms
// (launch-bound).
#include "gpfit_common.h"
#include "../../include/gpfit.h"

namespace {

constexpr int kMaxGrid = 64;                  // T1, T2 <= 64: at most 4 x 4 output tiles
constexpr int kMaxIntElems = 2048;            // I (d - nfree) doubles of Xint kept in LDS
constexpr int kMaxEffects = GPFIT_RESP_MAX_EFFECTS;
constexpr int kRows = 256;                    // training rows per chunk, one per thread
constexpr int kSub = 32;                      // rows contracted per panel
constexpr int kRS = kSub + 2;                 // doubles between two panel columns: the MFMA
                                              // operand reads (16 columns x 2 rows per 32 lanes)
                                              // hit 32 different 8-B banks
constexpr int kIB = 8;                        // integration points per pass over a row

struct RespArgs {
  const double* X;
  int n, d, ldx;
  const double* alpha;
  int lda;
  const double* beta;
  int ldbeta;
  const double* s;
  int nfree, order;
  const double* t1;
  int T1;
  const double* t2;
  int T2;
  const double* Xint;
  int I, ldi;
  double* out;
  long long lde, ldb;
  int b0;
  int eff[2 * kMaxEffects];
};

// One (problem, effect): PAIR = false the T1 values of a main effect, true the T2 x T1 surface.
template <bool PAIR>
__global__ __launch_bounds__(256) void response_kernel(RespArgs a) {
  __shared__ double xint[kMaxIntElems];
  __shared__ __attribute__((aligned(16))) double p1[kMaxGrid * kRS];   // E1 (main: g E1)
  __shared__ __attribute__((aligned(16))) double p2[kMaxGrid * kRS];   // g E2 (pairs)
  __shared__ double gs[kRows], x1s[kRows], x2s[kRows];
  __shared__ double t1s[kMaxGrid], t2s[kMaxGrid], betas[GPFIT_MAX_DIM];
  __shared__ int dimc[GPFIT_MAX_DIM];
  static_assert(4 * 64 <= kMaxGrid * kRS, "the main effect's partials alias the panel");
  const int e = blockIdx.x, b = a.b0 + blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = a.n, d = a.d, T1 = a.T1, T2 = PAIR ? a.T2 : 1, I = a.I;
  const int d1 = a.eff[e * a.nfree];
  const int d2 = PAIR ? a.eff[e * 2 + 1] : -1;
  const int nc = d - a.nfree;

  if (tid < d) betas[tid] = a.beta[(long long)b * a.ldbeta + tid];
  if (tid < T1) t1s[tid] = a.t1[tid];
  if (PAIR && tid < T2) t2s[tid] = a.t2[tid];
  if (tid == 0) {
    if (a.order == GPFIT_RESP_CYCLIC) {
      for (int c = 0; c < nc; ++c) dimc[c] = (d1 + 1 + c) % d;
    } else {
      for (int k = 0, c = 0; k < d; ++k)
        if (k != d1 && k != d2) dimc[c++] = k;
    }
  }
  for (int q = tid; q < I * nc; q += 256) xint[q] = a.Xint[(long long)(q / nc) * a.ldi + q % nc];
  __syncthreads();

  const double sb = a.s[b];
  const double b1 = betas[d1];
  const double b2 = PAIR ? betas[d2] : 0.0;
  const int T1p = (T1 + 15) & ~15, T2p = (T2 + 15) & ~15;
  const int nt1 = T1p >> 4, ntiles = nt1 * (T2p >> 4);
  const double* ab = a.alpha + (long long)b * a.lda;
  f64x4 acc[4] = {zero4(), zero4(), zero4(), zero4()};
  double accm = 0.0;

  for (int k0 = 0; k0 < n; k0 += kRows) {
    const int row = k0 + tid;
    const bool valid = row < n;
    const double* xr = a.X + (long long)(valid ? row : 0) * a.ldx;
    double M = 1.0;
    if (nc > 0) {
      double msum = 0.0;
      for (int i0 = 0; i0 < I; i0 += kIB) {
        double ex[kIB];
#pragma unroll
        for (int j = 0; j < kIB; ++j) ex[j] = 0.0;
        for (int c = 0; c < nc; ++c) {
          const int k = dimc[c];
          const double xv = xr[k], bk = betas[k];
#pragma unroll
          for (int j = 0; j < kIB; ++j) {
            const int i = min(i0 + j, I - 1);
            const double t = xv - xint[i * nc + c];
            ex[j] = fma(bk * t, t, ex[j]);
          }
        }
#pragma unroll
        for (int j = 0; j < kIB; ++j)
          if (i0 + j < I) msum += exp_neg(ex[j]);
      }
      M = msum / (double)I;
    }
    gs[tid] = valid ? (sb * ab[row]) * M : 0.0;
    x1s[tid] = xr[d1];
    if (PAIR) x2s[tid] = xr[d2];
    __syncthreads();

    for (int r0 = 0; r0 < kRows && k0 + r0 < n; r0 += kSub) {
      // the panels of rows k0 + r0 .. + 31: zero past n and in the columns T .. 16 ceil(T / 16)
      for (int q = tid; q < T1p * kSub; q += 256) {
        const int c = q / kSub, r = q % kSub;
        double v = 0.0;
        if (c < T1 && k0 + r0 + r < n) {
          const double t = x1s[r0 + r] - t1s[c];
          v = exp_neg((b1 * t) * t);
          if (!PAIR) v *= gs[r0 + r];
        }
        p1[c * kRS + r] = v;
      }
      if (PAIR) {
        for (int q = tid; q < T2p * kSub; q += 256) {
          const int c = q / kSub, r = q % kSub;
          double v = 0.0;
          if (c < T2 && k0 + r0 + r < n) {
            const double t = x2s[r0 + r] - t2s[c];
            v = gs[r0 + r] * exp_neg((b2 * t) * t);
          }
          p2[c * kRS + r] = v;
        }
      }
      __syncthreads();
      if (PAIR) {
        // A[i][k] = (g E2)[row k][column 16 ta + i], B[k][j] = E1[row k][column 16 tb + j]
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int p = wv + 4 * q;
          if (p < ntiles) {
            const double* pa = p2 + ((p / nt1) * 16 + (lane & 15)) * kRS + (lane >> 4);
            const double* pb = p1 + ((p % nt1) * 16 + (lane & 15)) * kRS + (lane >> 4);
#pragma unroll
            for (int ks = 0; ks < kSub; ks += 4) acc[q] = mfma16x16x4(pa[ks], pb[ks], acc[q]);
          }
        }
      } else if (lane < T1) {
        const double* pc = p1 + lane * kRS + wv * 8;
#pragma unroll
        for (int r = 0; r < 8; ++r) accm += pc[r];
      }
      __syncthreads();
    }
  }

  double* ob = a.out + (long long)b * a.ldb + (long long)e * a.lde;
  if (PAIR) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p = wv + 4 * q;
      if (p < ntiles) {
        const int a1 = (p % nt1) * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int a2 = (p / nt1) * 16 + (lane >> 4) + 4 * r;
          if (a1 < T1 && a2 < T2) ob[a2 * T1 + a1] = acc[q][r];
        }
      }
    }
  } else {
    // the four waves' partial sums, added in wave order (the panel is free now)
    p1[wv * 64 + lane] = accm;
    __syncthreads();
    if (tid < T1) ob[tid] = ((p1[tid] + p1[64 + tid]) + p1[128 + tid]) + p1[192 + tid];
  }
}

}  // namespace

extern "C" int gp_mean_response_max_grid(void) { return kMaxGrid; }
extern "C" int gp_mean_response_max_int_elems(void) { return kMaxIntElems; }

extern "C" int gp_mean_response(const double* X, int n, int d, int ldx, const double* alpha,
                                int lda, const double* beta, int ldbeta, const double* s,
                                int batch, const int* effects, int nfree, int E, int order,
                                const double* t1, int T1, const double* t2, int T2,
                                const double* Xint, int I, int ldi, double* out, long long lde,
                                long long ldb, hipStream_t stream) {
  if (!X) return -1;
  if (n < 0) return -2;
  if (d < 1 || d > GPFIT_MAX_DIM) return -3;
  if (ldx < d) return -4;
  if (!alpha) return -5;
  if (batch < 0) return -10;
  if (lda < n && batch > 1) return -6;
  if (!beta) return -7;
  if (ldbeta < d && batch > 1) return -8;
  if (!s) return -9;
  if (nfree < 1 || nfree > 2 || nfree > d) return -12;
  if (E < 0 || E > kMaxEffects) return -13;
  if (!effects && E > 0) return -11;
  if (order != GPFIT_RESP_CYCLIC && order != GPFIT_RESP_ASCENDING) return -14;
  if (order == GPFIT_RESP_CYCLIC && nfree == 2) return -14;
  for (int e = 0; e < E; ++e) {
    const int d1 = effects[e * nfree], d2 = nfree == 2 ? effects[e * 2 + 1] : -1;
    if (d1 < 0 || d1 >= d) return -11;
    if (nfree == 2 && (d2 < 0 || d2 >= d || d2 == d1)) return -11;
  }
  if (!t1) return -15;
  if (T1 < 1 || T1 > kMaxGrid) return -16;
  if (nfree == 2) {
    if (!t2) return -17;
    if (T2 < 1 || T2 > kMaxGrid) return -18;
  } else {
    T2 = 1;
  }
  const int nc = d - nfree;
  if (nc > 0) {
    if (!Xint) return -19;
    if (I < 1 || (long long)I * nc > kMaxIntElems) return -20;
    if (ldi < nc) return -21;
  } else {
    I = 0;
  }
  if (!out) return -22;
  if (lde < (long long)T1 * T2) return -23;
  if (E > 0 && ldb < (E - 1) * lde + (long long)T1 * T2) return -24;
  if (n == 0 || batch == 0 || E == 0) return 0;

  RespArgs a;
  a.X = X;
  a.n = n;
  a.d = d;
  a.ldx = ldx;
  a.alpha = alpha;
  a.lda = batch > 1 ? lda : 0;
  a.beta = beta;
  a.ldbeta = batch > 1 ? ldbeta : 0;
  a.s = s;
  a.nfree = nfree;
  a.order = order;
  a.t1 = t1;
  a.T1 = T1;
  a.t2 = t2;
  a.T2 = T2;
  a.Xint = Xint;
  a.I = I;
  a.ldi = ldi;
  a.out = out;
  a.lde = lde;
  a.ldb = batch > 1 ? ldb : 0;
  for (int i = 0; i < 2 * kMaxEffects; ++i) a.eff[i] = i < E * nfree ? effects[i] : 0;

  hipError_t e = hipSuccess;
  for (int b0 = 0; b0 < batch && e == hipSuccess; b0 += kMaxGridY) {
    const int nb = batch - b0 < kMaxGridY ? batch - b0 : kMaxGridY;
    a.b0 = b0;
    if (nfree == 2)
      hipLaunchKernelGGL(response_kernel<true>, dim3(E, nb), dim3(256), 0, stream, a);
    else
      hipLaunchKernelGGL(response_kernel<false>, dim3(E, nb), dim3(256), 0, stream, a);
    e = hipGetLastError();
  }
  return e == hipSuccess ? 0 : GPFIT_ERR_HIP - (int)e;
}
