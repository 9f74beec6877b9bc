// gp_xval: cross-validated predictions (leave-one-out / K-fold) from the L^-1 of gp_potrf_inv,
// with no refit.  For one problem, A = G + delta I, Q = A^-1 = L^-T L^-1, z = L^-1 w,
// alpha = L^-T z, and for a fold F (f indices) with the column panel P_F = L^-1[:, F]:
//   Q_FF = P_F^T P_F,  alpha_F = P_F^T z,
//   mean_F = w_F - Q_FF^-1 alpha_F = E[w_F | w_rest],  var_F = diag(Q_FF^-1) - shift.
// SEPIA's SepiaXvalEmulatorPrediction refits a sub-model per fold (assess_all_models.py:32,
// include_trunc_error.py:15 import it); here every fold is one pass over its panel.
//
//   z            : the triangular gemv of linalg.hip (masked form) into the workspace, chunked
//                  and launched by linv_vec.h's driver
//   xval_loo     : singleton folds, one wave per column: sum L^-1[k,i]^2 and sum L^-1[k,i] z_k
//                  over k >= i by linv_vec.h's column pass (the one gp_alpha runs), 16-B loads
//                  from the column's 16-row tile on; bound by the 4 n^2 bytes of the lower triangle
//   xval_fold    : 2 <= f <= 64, one workgroup per (problem, fold): the panel rows from
//                  min(F) down are staged 64 at a time in LDS (16-B loads down each gathered
//                  column), Q_FF accumulates on v_mfma_f64_16x16x4_f64 (the lower 16 x 16 tiles,
//                  the four waves splitting the 64 rows), alpha_F on the VALU; then in LDS
//                  Q_FF = R R^T, M = R^-1 in place, Q_FF^-1 alpha_F = M^T (M alpha_F) and
//                  diag(Q_FF^-1) = column sums of M^2; bound by 8 sum_F (n - min F) f bytes.
// Every kernel takes column c as zero above row c by masking (and rows >= n as zero), so the
// strict upper triangle and the padding of the caller's buffer never reach a result.  MFMA and
// not VALU for Q_FF: both have the same fp64 rate on gfx950, but a VALU contraction of the LDS
// panel needs two LDS operand reads per fma where the MFMA needs one per 16 (not measured
// against each other).
#include "linv_vec.h"

namespace {

constexpr int kMaxFold = GPFIT_XVAL_MAX_FOLD;
constexpr int kChunk = 64;            // panel rows staged per step
constexpr int kRS = kChunk + 2;       // doubles between two panel columns in LDS: the MFMA
                                      // operand reads (16 columns x 2 rows per 32 lanes) hit 32
                                      // different 8-B banks, and every column stays 16-B aligned
constexpr int kQS = kMaxFold + 1;     // row stride of Q_FF / R / M in LDS

struct XvalArgs {
  LinvVec v;              // L^-1, z and the launch's first problem
  const double* w;
  int ldw;
  const int* fold_ptr;
  const int* fold_idx;
  int nfolds, nidx;
  const double* shift;
  double* mean;
  double* var;
  int ldo;
  int* info;
};

// info[b]: -2 (an invalid fold) wins, otherwise the smallest failing fold + 1.
GP_DEV void report(int* info, int b, int v) {
  if (!info) return;
  int* p = info + b;
  int old = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (;;) {
    const int nw = (old == -2 || v == -2) ? -2 : (old == 0 ? v : min(old, v));
    if (nw == old) return;
    if (__hip_atomic_compare_exchange_strong(p, &old, nw, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      return;
  }
}

// Singleton folds (fold_ptr == NULL: fold i = {i} for every i < n), one wave per fold.
__global__ __launch_bounds__(256) void xval_loo_kernel(XvalArgs a) {
  const int b = a.v.b0 + blockIdx.y;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int n = a.v.n;
  int col;
  if (a.fold_ptr) {
    if (j >= a.nfolds) return;
    const int p0 = a.fold_ptr[j], p1 = a.fold_ptr[j + 1];
    if (p1 - p0 != 1) return;                  // xval_fold_kernel's (or empty)
    if (p0 < 0 || p0 >= a.nidx) {
      if (lane == 0) report(a.info, b, -2);
      return;
    }
    col = a.fold_idx[p0];
    if (col < 0 || col >= n) {
      if (lane == 0) report(a.info, b, -2);
      return;
    }
  } else {
    if (j >= n) return;
    col = j;
  }
  const LinvColSums cs = linv_col_sums<true>(a.v, b, col, lane);
  const double q = cs.sq, al = cs.zdot;
  if (lane == 0) {
    const double sh = a.shift ? a.shift[b] : 0.0;
    double m, v;
    if (q > 0.0) {
      m = a.w[(long long)b * a.ldw + col] - al / q;
      v = 1.0 / q - sh;
    } else {
      m = v = __builtin_nan("");
      report(a.info, b, j + 1);
    }
    a.mean[(long long)b * a.ldo + col] = m;
    a.var[(long long)b * a.ldo + col] = v;
  }
}

// Q_FF (lower 16 x 16 tiles) and alpha_F of one fold with T = ceil(f / 16) column tiles; on
// return Qm (aliasing the panel) holds Q_FF's lower triangle and apart the four waves' alpha.
template <int T>
GP_DEV void fold_accumulate(const XvalArgs& a, const double* Lb, const double* zb, const int* idx,
                            int f, int r0, double* panel, double* zs, double* apart) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = a.v.n;
  f64x4 acc[T * (T + 1) / 2];
#pragma unroll
  for (int p = 0; p < T * (T + 1) / 2; ++p) acc[p] = zero4();
  double al = 0.0;
  for (int k0 = r0; k0 < n; k0 += kChunk) {
    // stage rows k0 .. k0 + 63 of the gathered columns (zero above the diagonal, past n and in
    // the columns f .. 16 T - 1); a pair wholly above its column's diagonal is not loaded
    for (int e = tid; e < 16 * T * 32; e += 256) {
      const int c = e >> 5, rr = 2 * (e & 31), row = k0 + rr;
      f64x2 v = {0.0, 0.0};
      if (c < f && row < n) {
        const int ci = idx[c];
        if (row + 1 >= ci) {
          v = load2(Lb + (long long)ci * a.v.ld + row, a.v.vec);
          if (row < ci) v.x = 0.0;
          if (row + 1 >= n) v.y = 0.0;
        }
      }
      *reinterpret_cast<f64x2*>(panel + c * kRS + rr) = v;
    }
    if (tid < kChunk) zs[tid] = (k0 + tid < n) ? zb[k0 + tid] : 0.0;
    __syncthreads();
    if (lane < f) {
      const double* pc = panel + lane * kRS + wv * 16;
#pragma unroll
      for (int r = 0; r < 16; ++r) al = fma(pc[r], zs[wv * 16 + r], al);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      // A[i][k] = P[row k][column 16 ta + i] and B[k][j] = P[row k][column 16 tb + j]: one
      // value per lane and tile serves as both operands
      const int row = wv * 16 + s * 4 + (lane >> 4);
      double pv[T];
#pragma unroll
      for (int t = 0; t < T; ++t) pv[t] = panel[(t * 16 + (lane & 15)) * kRS + row];
      int p = 0;
#pragma unroll
      for (int ta = 0; ta < T; ++ta)
#pragma unroll
        for (int tb = 0; tb <= ta; ++tb, ++p) acc[p] = mfma16x16x4(pv[ta], pv[tb], acc[p]);
    }
    __syncthreads();
  }
  // the four waves' partial tiles, summed in wave order into Qm (the panel is free now)
  double* Qm = panel;
  for (int w = 0; w < 4; ++w) {
    if (wv == w) {
      int p = 0;
#pragma unroll
      for (int ta = 0; ta < T; ++ta)
#pragma unroll
        for (int tb = 0; tb <= ta; ++tb, ++p)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double* q = Qm + (ta * 16 + (lane >> 4) + 4 * r) * kQS + tb * 16 + (lane & 15);
            *q = w ? *q + acc[p][r] : acc[p][r];
          }
    }
    __syncthreads();
  }
  apart[wv * 64 + lane] = al;
  __syncthreads();
}

// Folds of 2 .. 64 indices: one workgroup per (problem, fold).
__global__ __launch_bounds__(256) void xval_fold_kernel(XvalArgs a) {
  __shared__ __attribute__((aligned(16))) double panel[kMaxFold * kRS];
  __shared__ double zs[kChunk];
  __shared__ double apart[4 * 64];
  __shared__ int idx[kMaxFold];
  __shared__ int meta[2];
  static_assert(kMaxFold * kQS <= kMaxFold * kRS, "Q_FF aliases the panel");
  const int fold = blockIdx.x, b = a.v.b0 + blockIdx.y;
  const int tid = threadIdx.x;
  const int n = a.v.n;
  const int p0 = a.fold_ptr[fold], p1 = a.fold_ptr[fold + 1];
  const int f = p1 - p0;
  if (f == 0 || f == 1) return;                // empty, or xval_loo_kernel's
  if (p0 < 0 || p1 > a.nidx || f < 0 || f > kMaxFold) {
    if (tid == 0) report(a.info, b, -2);
    return;
  }
  if (tid < f) idx[tid] = a.fold_idx[p0 + tid];
  __syncthreads();
  if (tid == 0) {
    int bad = 0, lo = n;
    for (int c = 0; c < f; ++c) {
      bad |= (idx[c] < 0 || idx[c] >= n);
      lo = min(lo, idx[c]);
    }
    meta[0] = bad;
    meta[1] = lo;
  }
  __syncthreads();
  if (meta[0]) {
    if (tid == 0) report(a.info, b, -2);
    return;
  }
  const int r0 = meta[1] & ~15;
  const double* Lb = a.v.Linv + b * a.v.sL;
  const double* zb = a.v.z + (long long)b * a.v.ldz;
  switch ((f + 15) >> 4) {
    case 1: fold_accumulate<1>(a, Lb, zb, idx, f, r0, panel, zs, apart); break;
    case 2: fold_accumulate<2>(a, Lb, zb, idx, f, r0, panel, zs, apart); break;
    case 3: fold_accumulate<3>(a, Lb, zb, idx, f, r0, panel, zs, apart); break;
    default: fold_accumulate<4>(a, Lb, zb, idx, f, r0, panel, zs, apart); break;
  }
  if (tid >= 64) return;
  // Wave 0, lane i = row i of R (factor) and column i of M (inverse); the wave runs in lockstep,
  // so a lane's LDS store is visible to every lane's later load.
  double* Qm = panel;
  const int i = tid;
  bool ok = true;
  for (int j = 0; j < f; ++j) {                // Q_FF = R R^T, left-looking, column j
    double s = 0.0;
    if (i >= j && i < f) {
      s = Qm[i * kQS + j];
      for (int k = 0; k < j; ++k) s = fma(-Qm[i * kQS + k], Qm[j * kQS + k], s);
    }
    const double d = readlane_f64(s, j);
    if (!(d > 0.0)) {
      ok = false;
      break;
    }
    const double r = sqrt(d);
    if (i >= j && i < f) Qm[i * kQS + j] = (i == j) ? r : s / r;
    __builtin_amdgcn_wave_barrier();
  }
  double x = 0.0, v = 0.0;
  if (ok) {
    const double alc =
        i < f ? ((apart[i] + apart[64 + i]) + apart[128 + i]) + apart[192 + i] : 0.0;
    for (int r = 0; r < f; ++r) {              // row r of M = R^-1, in place over row r of R
      const double rinv = 1.0 / Qm[r * kQS + r];
      double s = 0.0;
      for (int k = 0; k < r; ++k) {
        const double rk = Qm[r * kQS + k], mk = Qm[k * kQS + i];
        s = (k >= i) ? fma(rk, mk, s) : s;
      }
      const double m = i > r ? 0.0 : (i == r ? rinv : -s * rinv);
      __builtin_amdgcn_wave_barrier();
      if (i <= r) Qm[r * kQS + i] = m;
      const double y = wave_sum(m * alc);      // y_r = (M alpha_F)_r
      x = fma(m, y, x);                        // (M^T y)_i = (Q_FF^-1 alpha_F)_i
      v = fma(m, m, v);                        // diag(Q_FF^-1)_i
      __builtin_amdgcn_wave_barrier();
    }
  }
  if (i < f) {
    const int col = idx[i];
    const double sh = a.shift ? a.shift[b] : 0.0;
    const double nan = __builtin_nan("");
    a.mean[(long long)b * a.ldo + col] = ok ? a.w[(long long)b * a.ldw + col] - x : nan;
    a.var[(long long)b * a.ldo + col] = ok ? v - sh : nan;
  }
  if (!ok && i == 0) report(a.info, b, fold + 1);
}

}  // namespace

extern "C" int gp_xval_max_fold(void) { return kMaxFold; }

extern "C" long long gp_xval_ws_bytes(int n, int nfolds, int nidx, int batch) {
  if (n < 0 || nfolds < 0 || nidx < 0 || batch < 0) return -1;
  if (n == 0 || batch == 0) return 0;
  return linv_vec_ws_bytes(n, batch);
}

extern "C" int gp_xval(const double* Linv, int ldinv, long long strideInv, int n,
                       const double* w_hat, int ldw, const int* fold_ptr, const int* fold_idx,
                       int nfolds, int nidx, const double* shift, double* mean, double* var,
                       int ldo, int* info, int batch, void* ws, long long ws_bytes,
                       hipStream_t stream) {
  if (!Linv) return -1;
  if (n < 0) return -4;
  if (batch < 0) return -16;
  const int npad = gp_padded_n(n);
  if (ldinv < npad || ldinv < 1) return -2;
  if (batch > 1 && strideInv < (long long)ldinv * npad) return -3;
  if (!w_hat) return -5;
  if (ldw < n && batch > 1) return -6;
  if (nfolds < 0) return -9;
  if (nidx < 0 || nidx > n) return -10;
  if (!fold_ptr && fold_idx) return -7;
  if (fold_ptr && !fold_idx) return -8;
  if (!fold_ptr && nfolds != 0) return -9;
  if (!fold_ptr && nidx != 0) return -10;
  if (!mean) return -12;
  if (!var) return -13;
  if (ldo < n && batch > 1) return -14;
  if (n == 0 || batch == 0) return 0;
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255)) return -17;
  if (ws_bytes < gp_xval_ws_bytes(n, nfolds, nidx, batch)) return -18;
  if (fold_ptr && nfolds == 0) return 0;

  XvalArgs a;
  a.v = linv_vec_operands(Linv, ldinv, strideInv, n, batch, ws);
  a.w = w_hat;
  a.ldw = batch > 1 ? ldw : 0;
  a.fold_ptr = fold_ptr;
  a.fold_idx = fold_idx;
  a.nfolds = nfolds;
  a.nidx = nidx;
  a.shift = shift;
  a.mean = mean;
  a.var = var;
  a.ldo = batch > 1 ? ldo : 0;
  a.info = info;

  hipError_t e = hipSuccess;
  if (info) e = hipMemsetAsync(info, 0, sizeof(int) * (size_t)batch, stream);
  if (e == hipSuccess)
    e = linv_vec_run(a.v, w_hat, ldw, batch, stream, [&](int nb) {
      const int jobs = fold_ptr ? nfolds : n;
      hipLaunchKernelGGL(xval_loo_kernel, dim3(gp_ceil_div(jobs, 4), nb), dim3(256), 0, stream, a);
      const hipError_t el = hipGetLastError();
      if (el != hipSuccess || !fold_ptr) return el;
      hipLaunchKernelGGL(xval_fold_kernel, dim3(nfolds, nb), dim3(256), 0, stream, a);
      return hipGetLastError();
    });
  return e == hipSuccess ? 0 : GPFIT_ERR_HIP - (int)e;
}
