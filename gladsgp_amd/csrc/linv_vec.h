// L^-1 vector passes: what the post-fit consumers of the padded L^-1 of gp_potrf_inv share
// (gp_xval in xval.hip, gp_alpha in linalg.hip).  Both first form z = L^-1 w in the workspace by
// the masked triangular gemv of linalg.hip and then walk columns of L^-1 against z.
#pragma once
#include "gpfit_common.h"
#include "gpfit_internal.h"
#include "../../include/gpfit.h"

// The operands of a column pass.
struct LinvVec {
  const double* Linv;
  int ld;
  long long sL;
  int n;
  double* z;              // workspace: z_b = L_b^-1 w_b at z + b * ldz
  int ldz;
  int b0;                 // first problem of this launch (grid.y is limited)
  int vec;                // L^-1 16-B aligned with even ld / stride: 16-B loads
};

struct LinvColSums {
  double zdot;            // sum_{k >= col} L^-1[k,col] z_k
  double sq;              // sum_{k >= col} L^-1[k,col]^2 (kSq), otherwise 0
};

// Column `col` of problem `b`, one wave: 16-B loads from the column's 16-row tile on, the rows
// above the diagonal and past n taken as zero; every lane returns the wave's sums.
template <bool kSq>
GP_DEV LinvColSums linv_col_sums(LinvVec a, int b, int col, int lane) {
  const int n = a.n;
  const double* Lc = a.Linv + b * a.sL + (long long)col * a.ld;
  const double* zb = a.z + (long long)b * a.ldz;
  double q0 = 0.0, q1 = 0.0, al0 = 0.0, al1 = 0.0;
  // rows r, r + 1 with r even: r + 1 <= n - 1, or n is odd and r + 1 = n < gp_padded_n(n)
  for (int r = (col & ~15) + 2 * lane; r < n; r += 128) {
    const f64x2 v = load2(Lc + r, a.vec);
    const f64x2 zz = *reinterpret_cast<const f64x2*>(zb + r);
    const bool in1 = r + 1 < n;
    const double x0 = r >= col ? v.x : 0.0;
    const double x1 = (in1 && r + 1 >= col) ? v.y : 0.0;
    const double z1 = in1 ? zz.y : 0.0;
    if constexpr (kSq) {
      q0 = fma(x0, x0, q0);
      q1 = fma(x1, x1, q1);
    }
    al0 = fma(x0, zz.x, al0);
    al1 = fma(x1, z1, al1);
  }
  LinvColSums s;
  s.sq = kSq ? wave_sum(q0 + q1) : 0.0;
  s.zdot = wave_sum(al0 + al1);
  return s;
}

// z = L^-1 w of every problem: gp_padded_n(n) doubles each.
inline long long linv_vec_ws_bytes(int n, int batch) {
  return align256(8LL * batch * gp_padded_n(n));
}

// A lone problem takes stride 0 (the caller's value is not read); 16-B loads need a 16-B aligned
// base with even ld and stride.
inline LinvVec linv_vec_operands(const double* Linv, int ldinv, long long strideInv, int n,
                                 int batch, void* ws) {
  LinvVec a;
  a.Linv = Linv;
  a.ld = ldinv;
  a.sL = batch > 1 ? strideInv : 0;
  a.n = n;
  a.z = static_cast<double*>(ws);
  a.ldz = gp_padded_n(n);
  a.b0 = 0;
  a.vec = !(reinterpret_cast<uintptr_t>(Linv) & 15) && !(ldinv & 1) && !(a.sL & 1);
  return a;
}

// Per chunk of at most kMaxGridY problems: z by the masked triangular gemv, then launch(nb) with
// a.b0 set (the caller's kernels read `a` through the struct that embeds it).
template <class Launch>
hipError_t linv_vec_run(LinvVec& a, const double* w, int ldw, int batch, hipStream_t stream,
                        Launch launch) {
  const int sw = batch > 1 ? ldw : 0;
  hipError_t e = hipSuccess;
  for (int b0 = 0; b0 < batch && e == hipSuccess; b0 += kMaxGridY) {
    const int nb = batch - b0 < kMaxGridY ? batch - b0 : kMaxGridY;
    a.b0 = b0;
    e = gpfit_trmv_launch(true, a.Linv + b0 * a.sL, a.ld, a.sL, w + (long long)b0 * sw, sw,
                          a.z + (long long)b0 * a.ldz, a.ldz, a.n, nb, stream);
    if (e == hipSuccess) e = launch(nb);
  }
  return e;
}
