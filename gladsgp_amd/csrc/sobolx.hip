// gp_sobol_exact: closed-form Sobol' ingredients of the emulator's posterior mean under uniform
// inputs on a box.  A unit u is one (sample, PC) GP with beta_u (d values), s_u
// and alpha_u = A^-1 w (gp_alpha); its mean is f_u(x) = s_u sum_n alpha_un prod_k
// exp(-beta_uk (x_k - X_nk)^2).  With w_k = hi_k - lo_k and erfd(p, q) = erf(p) - erf(q):
//   I_k(u,n)         = sqrt(pi) / (2 r w_k) erfd(r (hi_k - X_nk), r (lo_k - X_nk)),  r = sqrt(beta_uk)
//   J_k(u,n; v,n')   = exp(-(b b'/B) (a - a')^2) sqrt(pi) / (2 sqrt(B) w_k)
//                      erfd(sqrt(B) (hi_k - c), sqrt(B) (lo_k - c))
//                      b = beta_uk, b' = beta_vk, B = b + b', a = X_nk, a' = X_n'k,
//                      c = (b / B) a + (b' / B) a'
//   E_u              = s_u sum_n alpha_un prod_k I_k(u,n)
//   Q_tot(u,v)       = s_u s_v sum_nn' alpha_un alpha_vn' prod_k J_k
//   Q_main_i(u,v)    = s_u s_v sum_nn' alpha_un alpha_vn' J_i prod_{k != i} I_k(u,n) I_k(v,n')
//   Q_not_i(u,v)     = s_u s_v sum_nn' alpha_un alpha_vn' I_i(u,n) I_i(v,n') prod_{k != i} J_k
// The reference (src/utils.py:27-256) estimates the same quantities by Saltelli sampling of the
// mean with 2^8 base points and describes the estimate's noise with 4 x 9,999 bootstrap resamples.
//
//   sx_unit   one 256-thread workgroup per unit: I_k(u,n) for every point (d erf pairs each), its
//             leave-one-out products L_i = prod_{k != i} I_k by exclusive prefix / suffix products
//             (never a division: an I_k may underflow), alpha I_k and alpha L_k into the
//             workspace, and E_u (one partial per thread over n = tid, tid + 256, .., the wave
//             tree, the four waves in order).
//   sx_pair   one workgroup per (unit pair a <= b of a group, 64 x 64 tile of the (n, n') plane),
//             16 point pairs per thread, the dimensions in chunks of 8: the chunk's J_k in
//             registers, prod_{k != i} J_k by prefix / suffix products inside the chunk times the
//             product over the other chunks' dimensions (none for d <= 8; recomputed per chunk
//             above: 4 x the transcendentals at 8 < d <= 32, nothing indexed dynamically).  The
//             2 d + 1 sums of the tile go to the workspace.  a == b: the summand is the same
//             function of (n, n') and (n', n), so only tiles I >= J are computed, those with I > J
//             doubled (exact), the others written as 0.
//   sx_sum    per pair and quantity the tiles' partial sums in ascending tile order, times
//             s_u s_v, written to Q[g, a, b] and Q[g, b, a].
// No atomics; the order of every sum is fixed by (n, d) alone and every load is an 8-B load:
// equal inputs give equal bits whatever G, M, the unit's place in the batch or the strides, and
// the (a, a) entry of a grouped call is the M = 1 call's.
// erfd with both arguments of one sign (a point, or the centre c, outside the box) is evaluated
// as erfc(|near|) - erfc(|far|), which keeps the bracket's relative accuracy; inside the box the
// two erf terms have opposite signs and add.
// Work: per point pair and dimension one exp_neg (~19 fp64 VALU ops), two erf / erfc (ocml) and
// ~15 multiplies; n^2 d of them per unit pair.  The kernel is bound by the fp64 VALU rate
// (measured: DESIGN.md §4.6h).
#include "gpfit_common.h"
#include "../../include/gpfit.h"

namespace {

constexpr int T = 64;                 // tile edge of the (n, n') plane
constexpr int CH = 8;                 // dimensions per chunk
constexpr int EPT = T * T / 256;      // point pairs per thread
constexpr int NQ = 2 * CH + 1;        // sums per chunk: tot, main, not
constexpr double kHalfSqrtPi = 0x1.c5bf891b4ef6bp-1;     // sqrt(pi) / 2
constexpr long long kMaxBlocks = 1LL << 30;

struct SxArgs {
  const double* X;
  int n, d, ldx, M;
  const double* alpha;
  long long lda;
  const double* beta;
  long long ldbeta;
  const double* s;
  const double* lo;
  const double* hi;
  double* E;
  long long incE;
  double* Q;
  long long ldq, ldqa, ldqg;
  double* wA;             // alpha_un L_k(u,n) at (u d + k) n + point
  double* wB;             // alpha_un I_k(u,n), same layout
  double* part;           // part[(pair (2 d + 1) + q) nt2 + tile]
  int nt;                 // tiles per edge
  long long p0;           // first pair (sx_pair, sx_sum) or unit (sx_unit) of this launch
};

// erf(p) - erf(q), p > q
GP_DEV double erf_diff(double p, double q) {
  if (p <= 0.0) {         // both below the point: mirror
    const double t = -q;
    q = -p;
    p = t;
  }
  if (q >= 0.0) return erfc(q) - erfc(p);
  return erf(p) - erf(q);
}

GP_DEV double block_sum(double v, double* red, int tid) {
  v = wave_sum(v);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void sx_unit_kernel(const SxArgs a) {
  __shared__ double rs[GPFIT_MAX_DIM], cf[GPFIT_MAX_DIM], los[GPFIT_MAX_DIM], his[GPFIT_MAX_DIM];
  __shared__ double red[4];
  const long long u = a.p0 + blockIdx.x;
  const int tid = threadIdx.x, n = a.n, d = a.d;
  if (tid < d) {
    const double b = a.beta[u * a.ldbeta + tid];
    const double l = a.lo ? a.lo[tid] : 0.0, h = a.hi ? a.hi[tid] : 1.0;
    const double r = sqrt(b);
    rs[tid] = r;
    los[tid] = l;
    his[tid] = h;
    cf[tid] = kHalfSqrtPi / (r * (h - l));
  }
  __syncthreads();
  double* wA = a.wA + u * d * (long long)n;
  double* wB = a.wB + u * d * (long long)n;
  double acc = 0.0;
  for (int row = tid; row < n; row += 256) {
    const double al = a.alpha[u * a.lda + row];
    const double* xr = a.X + (long long)row * a.ldx;
    double pre = 1.0;
    for (int k = 0; k < d; ++k) {
      const double x = xr[k];
      const double v = cf[k] * erf_diff(rs[k] * (his[k] - x), rs[k] * (los[k] - x));
      wB[(long long)k * n + row] = v;
      pre *= v;
    }
    acc = fma(al, pre, acc);
    double suf = 1.0;                                   // prod_{k' > k} I_k'
    for (int k = d - 1; k >= 0; --k) {
      wA[(long long)k * n + row] = suf;
      suf *= wB[(long long)k * n + row];
    }
    pre = 1.0;                                          // prod_{k' < k} I_k'
    for (int k = 0; k < d; ++k) {
      const double v = wB[(long long)k * n + row];
      wA[(long long)k * n + row] = al * (pre * wA[(long long)k * n + row]);
      wB[(long long)k * n + row] = al * v;
      pre *= v;
    }
  }
  const double tot = block_sum(acc, red, tid);
  if (tid == 0) a.E[u * a.incE] = a.s[u] * tot;
}

// NC: chunks of 8 dimensions (1: d <= 8, 4: d <= 32)
template <int NC>
__global__ __launch_bounds__(256) void sx_pair_kernel(const SxArgs a) {
  constexpr int DM = NC * CH;
  __shared__ double xr[DM * T], xc[DM * T];
  __shared__ double Ar[CH * T], Ac[CH * T], Br[CH * T], Bc[CH * T];
  __shared__ double alr[T], alc[T];
  __shared__ double kk[DM], rB[DM], cf[DM], wa[DM], wb[DM], los[DM], his[DM];
  __shared__ double red[4][NQ];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = a.n, d = a.d, nt = a.nt, nt2 = nt * nt;
  const long long blk = blockIdx.x;
  const int t = (int)(blk % nt2);
  const long long pr = a.p0 + blk / nt2;
  const long long npg = (long long)a.M * (a.M + 1) / 2;
  const long long g = pr / npg;
  const long long p = pr - g * npg;
  // p = ub (ub + 1) / 2 + ua, ua <= ub
  long long ub = (long long)((__builtin_sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
  while ((ub + 1) * (ub + 2) / 2 <= p) ++ub;
  while (ub * (ub + 1) / 2 > p) --ub;
  const long long ua = p - ub * (ub + 1) / 2;
  const long long u = g * a.M + ua, v = g * a.M + ub;
  const int I = t / nt, J = t - I * nt;
  const int I0 = I * T, J0 = J * T;
  double* part = a.part + pr * (2 * d + 1) * nt2 + t;
  const bool diag = ua == ub;
  if (diag && J > I) {
    if (tid < 2 * d + 1) part[(long long)tid * nt2] = 0.0;
    return;
  }
  const double weight = (diag && I > J) ? 2.0 : 1.0;

  if (tid < DM) {
    double b = 1.0, b2 = 1.0, l = 0.0, h = 1.0;
    if (tid < d) {
      b = a.beta[u * a.ldbeta + tid];
      b2 = a.beta[v * a.ldbeta + tid];
      l = a.lo ? a.lo[tid] : 0.0;
      h = a.hi ? a.hi[tid] : 1.0;
    }
    const double B = b + b2;
    const double r = sqrt(B);
    kk[tid] = b * b2 / B;
    rB[tid] = r;
    cf[tid] = kHalfSqrtPi / (r * (h - l));
    wa[tid] = b / B;
    wb[tid] = b2 / B;
    los[tid] = l;
    his[tid] = h;
  }
  for (int e = tid; e < T * d; e += 256) {
    const int q = e / d, k = e - q * d;
    xr[k * T + q] = I0 + q < n ? a.X[(long long)(I0 + q) * a.ldx + k] : 0.0;
    xc[k * T + q] = J0 + q < n ? a.X[(long long)(J0 + q) * a.ldx + k] : 0.0;
  }
  if (tid < T) {
    alr[tid] = I0 + tid < n ? a.alpha[u * a.lda + I0 + tid] : 0.0;
  } else if (tid < 2 * T) {
    const int q = tid - T;
    alc[q] = J0 + q < n ? a.alpha[v * a.lda + J0 + q] : 0.0;
  }
  const double* wAu = a.wA + u * d * (long long)n;
  const double* wAv = a.wA + v * d * (long long)n;
  const double* wBu = a.wB + u * d * (long long)n;
  const double* wBv = a.wB + v * d * (long long)n;

  auto Jk = [&](int k, int i, int j) {
    const double x = xr[k * T + i], y = xc[k * T + j];
    const double dl = x - y;
    const double ex = exp_neg((kk[k] * dl) * dl);
    const double c = wa[k] * x + wb[k] * y;
    const double br = erf_diff(rB[k] * (his[k] - c), rB[k] * (los[k] - c));
    return (ex * cf[k]) * br;
  };

#pragma unroll 1
  for (int c = 0; c < NC; ++c) {
    const int k0 = c * CH;
    if (NC > 1 && k0 >= d) break;
    __syncthreads();
    for (int e = tid; e < CH * T; e += 256) {
      const int j = e / T, q = e - j * T, k = k0 + j;
      const bool okr = k < d && I0 + q < n, okc = k < d && J0 + q < n;
      Ar[e] = okr ? wAu[(long long)k * n + I0 + q] : 0.0;
      Br[e] = okr ? wBu[(long long)k * n + I0 + q] : 0.0;
      Ac[e] = okc ? wAv[(long long)k * n + J0 + q] : 0.0;
      Bc[e] = okc ? wBv[(long long)k * n + J0 + q] : 0.0;
    }
    __syncthreads();
    double tot = 0.0, mn[CH], nn[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) mn[j] = nn[j] = 0.0;
#pragma unroll 1
    for (int e = 0; e < EPT; ++e) {
      const int i = wv + 4 * e, jc = lane;
      double other = 1.0;
      if (NC > 1) {
#pragma unroll 1
        for (int k = 0; k < d; ++k)
          if ((k >> 3) != c) other *= Jk(k, i, jc);
      }
      double Jv[CH], suf[CH];
#pragma unroll
      for (int j = 0; j < CH; ++j) Jv[j] = k0 + j < d ? Jk(k0 + j, i, jc) : 1.0;
      suf[CH - 1] = 1.0;
#pragma unroll
      for (int j = CH - 2; j >= 0; --j) suf[j] = suf[j + 1] * Jv[j + 1];
      double pre = other;
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const double loo = pre * suf[j];
        mn[j] = fma(Ar[j * T + i] * Ac[j * T + jc], Jv[j], mn[j]);
        nn[j] = fma(Br[j * T + i] * Bc[j * T + jc], loo, nn[j]);
        pre *= Jv[j];
      }
      if (c == 0) tot = fma(alr[i] * alc[jc], pre, tot);
    }
    // the chunk's 17 sums over the tile: the wave tree, then the four waves in order
    tot = wave_sum(tot);
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      mn[j] = wave_sum(mn[j]);
      nn[j] = wave_sum(nn[j]);
    }
    __syncthreads();
    if (lane == 0) {
      red[wv][0] = tot;
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        red[wv][1 + j] = mn[j];
        red[wv][1 + CH + j] = nn[j];
      }
    }
    __syncthreads();
    if (tid < NQ) {
      const double s4 = weight * (((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid]);
      if (tid == 0) {
        if (c == 0) part[0] = s4;
      } else {
        const int j = (tid - 1) % CH, k = k0 + j;
        const int q = tid <= CH ? 1 + k : 1 + d + k;
        if (k < d) part[(long long)q * nt2] = s4;
      }
    }
  }
}

// Q[g, a, b, q] = Q[g, b, a, q] = s_u s_v sum_t part[(pair (2 d + 1) + q) nt2 + t], t ascending
__global__ __launch_bounds__(128) void sx_sum_kernel(const SxArgs a) {
  const int q = threadIdx.x, d = a.d, nt2 = a.nt * a.nt;
  if (q >= 2 * d + 1) return;
  const long long pr = a.p0 + blockIdx.x;
  const long long npg = (long long)a.M * (a.M + 1) / 2;
  const long long g = pr / npg;
  const long long p = pr - g * npg;
  long long ub = (long long)((__builtin_sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
  while ((ub + 1) * (ub + 2) / 2 <= p) ++ub;
  while (ub * (ub + 1) / 2 > p) --ub;
  const long long ua = p - ub * (ub + 1) / 2;
  const double* pp = a.part + (pr * (2 * d + 1) + q) * nt2;
  double acc = 0.0;
  for (int t = 0; t < nt2; ++t) acc += pp[t];
  const double val = (a.s[g * a.M + ua] * a.s[g * a.M + ub]) * acc;
  double* Qg = a.Q + g * a.ldqg;
  Qg[ua * a.ldqa + ub * a.ldq + q] = val;
  if (ua != ub) Qg[ub * a.ldqa + ua * a.ldq + q] = val;
}

// n = 0: every sum is empty
__global__ __launch_bounds__(256) void sx_zero_kernel(const SxArgs a, long long G) {
  const long long U = G * a.M, nq = 2 * a.d + 1;
  const long long total = U + U * a.M * nq;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += 256LL * gridDim.x) {
    if (e < U) {
      a.E[e * a.incE] = 0.0;
    } else {
      long long r = e - U;
      const long long q = r % nq;
      r /= nq;
      const long long b = r % a.M;
      r /= a.M;
      const long long ua = r % a.M, g = r / a.M;
      a.Q[g * a.ldqg + ua * a.ldqa + b * a.ldq + q] = 0.0;
    }
  }
}

long long sx_tiles(int n) { return gp_ceil_div(n, T); }

}  // namespace

extern "C" long long gp_sobol_exact_ws_bytes(int n, int d, int G, int M) {
  if (n < 0 || d < 0 || G < 0 || M < 0) return -1;
  if (n == 0 || d == 0 || G == 0 || M == 0) return 0;
  const long long U = (long long)G * M, nt = sx_tiles(n);
  const long long pairs = (long long)G * ((long long)M * (M + 1) / 2);
  return align256(8 * (2 * U * d * n + pairs * (2 * d + 1) * nt * nt));
}

extern "C" int gp_sobol_exact(const double* X, int n, int d, int ldx, int G, int M,
                              const double* alpha, int lda, const double* beta, int ldbeta,
                              const double* s, const double* lo, const double* hi, double* E,
                              long long incE, double* Q, long long ldq, long long ldqa,
                              long long ldqg, void* ws, long long ws_bytes, hipStream_t stream) {
  if (!X) return -1;
  if (n < 0) return -2;
  if (d < 1 || d > GPFIT_MAX_DIM) return -3;
  if (ldx < d) return -4;
  if (G < 0) return -5;
  if (M < 1 || (long long)G * M > 0x7fffffffLL) return -6;
  const long long U = (long long)G * M, nq = 2 * d + 1;
  if (!alpha) return -7;
  if (lda < n && U > 1) return -8;
  if (!beta) return -9;
  if (ldbeta < d && U > 1) return -10;
  if (!s) return -11;
  if (!lo != !hi) return lo ? -13 : -12;
  if (!E) return -14;
  if (incE < 1 && U > 1) return -15;
  if (!Q) return -16;
  if (ldq < nq && M > 1) return -17;
  if (M > 1 && ldqa < (M - 1) * ldq + nq) return -18;
  if (G > 1 && ldqg < (M - 1) * (M > 1 ? ldqa + ldq : 0) + nq) return -19;
  if (G == 0) return 0;

  SxArgs a;
  a.X = X;
  a.n = n;
  a.d = d;
  a.ldx = ldx;
  a.M = M;
  a.alpha = alpha;
  a.lda = U > 1 ? lda : 0;
  a.beta = beta;
  a.ldbeta = U > 1 ? ldbeta : 0;
  a.s = s;
  a.lo = lo;
  a.hi = hi;
  a.E = E;
  a.incE = U > 1 ? incE : 0;
  a.Q = Q;
  a.ldq = M > 1 ? ldq : 0;
  a.ldqa = M > 1 ? ldqa : 0;
  a.ldqg = G > 1 ? ldqg : 0;
  a.wA = a.wB = a.part = nullptr;
  a.nt = 0;
  a.p0 = 0;
  if (n == 0) {
    const long long total = U + U * M * nq;
    const long long nb = (total + 255) / 256;
    hipLaunchKernelGGL(sx_zero_kernel, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0,
                       stream, a, (long long)G);
    GP_CK(hipGetLastError());
    return 0;
  }
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255)) return -20;
  if (ws_bytes < gp_sobol_exact_ws_bytes(n, d, G, M)) return -21;

  const long long nt = sx_tiles(n), nt2 = nt * nt;
  if (nt2 > kMaxBlocks) return -2;
  const long long pairs = (long long)G * ((long long)M * (M + 1) / 2);
  a.wA = static_cast<double*>(ws);
  a.wB = a.wA + U * d * n;
  a.part = a.wB + U * d * n;
  a.nt = (int)nt;
  for (long long u0 = 0; u0 < U; u0 += kMaxBlocks) {
    const long long nu = U - u0 < kMaxBlocks ? U - u0 : kMaxBlocks;
    a.p0 = u0;
    hipLaunchKernelGGL(sx_unit_kernel, dim3((unsigned)nu), dim3(256), 0, stream, a);
    GP_CK(hipGetLastError());
  }
  const long long chunk = kMaxBlocks / nt2;
  for (long long p0 = 0; p0 < pairs; p0 += chunk) {
    const long long np = pairs - p0 < chunk ? pairs - p0 : chunk;
    a.p0 = p0;
    if (d <= CH)
      hipLaunchKernelGGL(sx_pair_kernel<1>, dim3((unsigned)(np * nt2)), dim3(256), 0, stream, a);
    else
      hipLaunchKernelGGL(sx_pair_kernel<GPFIT_MAX_DIM / CH>, dim3((unsigned)(np * nt2)),
                         dim3(256), 0, stream, a);
    GP_CK(hipGetLastError());
    hipLaunchKernelGGL(sx_sum_kernel, dim3((unsigned)np), dim3(128), 0, stream, a);
    GP_CK(hipGetLastError());
  }
  return 0;
}
