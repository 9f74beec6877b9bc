// The per-column 16 x 16 leaf that leaf16_blocked (gladsgp_amd/csrc/chol.hip) replaced in the
// library, kept for the micro-benchmarks that compare the two (leaf_micro.hip,
// leaf2_micro.hip, leafonly_micro.hip).  Include after chol.hip.
#pragma once

// One wave: factor + invert the 16 x 16 block at (o, o).  Writes L_bb into T's block and
// Dinv_b into U's block (lower, zero upper) and the 16 pivots p_c (L_cc = sqrt(p_c)) into
// piv[o + c]; the caller checks them.
//
// The block lives in MFMA C layout (lane l, reg q = element [(l >> 4) + 4q][l & 15]), so row j
// of the block is register j / 4 of lanes 16 (j % 4) .. + 15, which is at once the A operand's
// column k = j % 4 (A[i][k] from lane 16k + i) and the B operand's row k (B[k][c] from lane
// 16k + c).  Elimination step j is therefore ONE v_mfma_f64_16x16x4 on the whole block,
//   A[i][c] -= A[j][i] (A[j][c] / p_j)    (i, c > j; the other three k lanes zero),
// and one more applies the same row operation to W (= I at the start): W[i][c] -= m_i W[j][c],
// m_i = A[j][i] / p_j.  Both factors come from row j only, the same copy for every row (the
// rounding asymmetry of the trailing block never feeds back; see diag_factor_inv).  At the end
// A's lower triangle holds Lt[r][c] p_c and W = Lt^-1:  L = A D^-1/2 (columns), L^-1 = D^-1/2 W
// (rows).  Per step the dependent chain is readlane -> rcp + 2 Newton -> select -> MFMA; the
// register-resident form with one readlane pair per row and step (and the SGPR traffic that
// came with it) measured 8.5k cycles per leaf (tools/dbg/leaf_micro.hip).  Splitting the W
// row operations onto a second wave (multipliers handed over through LDS, a step counter)
// measured slower inside the chain: 14.6 vs 12.4 us per 64 x 64 factor
// (profiles/r03/pp_trace_pp4_pairs_splitleaf.txt).
GP_DEV void leaf16(lds_double* T, lds_double* U, int o, lds_double* piv) {
  const int lane = threadIdx.x & 63;
  const int r0 = lane >> 4, c = lane & 15;
  f64x4 A = ld16(T + o * LP + o);
  f64x4 W;
#pragma unroll
  for (int q = 0; q < 4; ++q) W[q] = (r0 + 4 * q == c) ? 1.0 : 0.0;
  double colpiv = 1.0;          // p_c of this lane's column
  double rowpiv[4];             // p_r of rows r0 + 4q
#pragma unroll
  for (int q = 0; q < 4; ++q) rowpiv[q] = 1.0;
  static_for<0, 16, 1>([&](auto J) {
    constexpr int j = decltype(J)::value;
    constexpr int q = j >> 2, k = j & 3;
    const double p = readlane_f64(A[q], 16 * k + j);
    colpiv = (c == j) ? p : colpiv;
    rowpiv[q] = (r0 == k) ? p : rowpiv[q];
    if constexpr (j < 15) {
      const double rp = rcp_nr(p);
      const bool sel = r0 == k && c > j;
      const double rowj = A[q];
      const double a = sel ? -rowj : 0.0;
      const double m = sel ? rowj * rp : 0.0;
      const double wj = W[q];
      A = mfma16x16x4(a, m, A);
      W = mfma16x16x4(-m, wj, W);
    }
  });
  const double rsc = rsqrt_nr(colpiv);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = r0 + 4 * q;
    const double rsr = rsqrt_nr(rowpiv[q]);
    T[(o + r) * LP + o + c] = r >= c ? A[q] * rsc : 0.0;
    U[(o + r) * LP + o + c] = r >= c ? W[q] * rsr : 0.0;
  }
  if (lane < 16) piv[o + c] = colpiv;
}
