// Fused predictive summary (A9 + its reduction): mean and quantile band of the reconstructed
// field over the posterior samples -- np.mean(preds.get_y(), 0) and np.quantile(preds.get_y() +
// error, [q, 1 - q], 0) of assess_all_models.py:489-500 / 510-521, plot_test_error.py:77-87,
// include_trunc_error.py:84-90 -- in one pass over w and K.  The (S, m, ny) field the reference
// builds only to reduce it (four test points at a time, because it does not fit otherwise) is
// never stored: 3 m ny outputs instead of S m ny.
//
// Layout (field_core.h, shared with field.hip): block = 4 waves; every wave owns 32 consecutive
// columns (two 16-column MFMA tiles), the block 128.  A work unit is (column panel, test point);
// block i takes a contiguous range of the panel-major unit list and keeps its K panel in
// registers while the panel lasts.  The point's S rows of w (one per sample, stride lds) stream
// through LDS in 32-sample tiles (16 at P > 32), double-buffered across unit boundaries; the
// tile's error scalars ride in a spare column of the LDS rows.
//
// After a tile's MFMAs every lane folds its 2 x 8 accumulator values (MFMA C layout: lane l,
// register r holds row (l >> 4) + 4 r, column l & 15 of a 16 x 16 tile) into running state per
// owned column: one fp64 sum of y, the KT smallest z (ascending) and the KT smallest -z, i.e. the
// KT largest z, both kept by min/max insertion in registers (2 KT - 1 operations per value and
// list; rows past S in the last tile are branched around and enter nothing).  The
// state is 2 KT + 1 doubles per column whatever S is.  At the end of a unit the four lanes that
// share a column (l >> 4 = 0..3) merge by two cross-lane exchanges that also split the work:
// lanes 16 apart trade tiles (one keeps column tile 0, the other tile 1), lanes 32 apart trade
// tails (one keeps the lower list, the other the upper), so each of the 64 lanes ends with one
// complete list of one column and does one interpolation.  No LDS is needed for the merge.
//
// Bits: a_s is field_kernel's k-ordered MFMA chain (same operands, same order: tested directly by
// tests/test_gpu_summary.py::test_one_sample_is_the_field), y and z are the same fma / add as
// field_kernel's epilogue, so every sample value equals gp_field's bit for bit; the order
// statistics are selections of those values (exact), the interpolation is numpy's _lerp with its
// three roundings (no contraction), the mean is a fixed-order fp64 sum divided by S.
//
// gp_field_score is the same body with the reduction against a truth in the store's place
// (summary_body<KS, KT, SCORE>, see there): row and column partial sums into a workspace, added in
// a fixed order by score_reduce_kernel.  summary_kernel<KS, KT> is the SCORE = false instance and
// compiles to the registers, LDS and scratch it had as a kernel of its own.
#include "field_core.h"
#include "../../include/gpfit.h"

#include <math.h>

namespace {

using namespace field_core;

// waves per SIMD the register allocator is asked to keep: 2 (256 registers per lane; the small
// instantiations end below that and fit 3-4); the deepest lists (2 x 2 x 8 doubles of state
// beside the K panel) get the whole file instead of spilling to scratch
template <int KS, int KT> constexpr int sum_occ() { return KT > 4 || (KT == 4 && KS > 12) ? 1 : 2; }
constexpr int kSumErrCol = kMaxP;             // the row's error scalar (k < kMaxP: the weights)
static_assert(kSumErrCol < kPitch, "the error scalar rides inside the LDS row");
constexpr int kSumMaxTail = 8;

// one tail of the band: the two list positions numpy's linear rule reads and its weight
struct SumTail {
  int ia, ib;
  double t;
};

// sorted insertion: l ascending keeps the KT smallest of what it has seen; NEG inserts -v (the
// source modifier is free).  v_min_f64 / v_max_f64 are written out because fmin / fmax add a
// canonicalising v_max_f64 x, x, x per operand whose producer the compiler cannot see (every list
// entry at every basic-block entry: +40 % fp64 operations in the fold), which values that all come
// out of v_fma_f64 or of these two instructions do not need.
template <int KT, bool NEG = false>
GP_DEV void sum_insert(double (&l)[KT], double v) {
#pragma unroll
  for (int i = 0; i < KT; ++i) {
    double w;                                  // the larger moves on, the smaller stays in place
    if (NEG && i == 0) {
      asm("v_max_f64 %0, %1, -%2" : "=v"(w) : "v"(l[i]), "v"(v));
      asm("v_min_f64 %0, %0, -%1" : "+v"(l[i]) : "v"(v));
    } else {
      asm("v_max_f64 %0, %1, %2" : "=v"(w) : "v"(l[i]), "v"(v));
      asm("v_min_f64 %0, %0, %1" : "+v"(l[i]) : "v"(v));
    }
    v = w;
  }
}

// numpy's _lerp(a, b, t): every product and sum rounded on its own
GP_DEV double sum_lerp(double a, double b, double t) {
#pragma clang fp contract(off)
  const double d = b - a;
  const double up = a + d * t;
  const double dn = b - d * (1.0 - t);
  return t >= 0.5 ? dn : up;
}

// gp_field_score's operands beside the summary's: the truth, the MAPE floor, the partials
struct ScoreK {
  const void* Y;
  long long ldy;
  int y_f32;
  double floor;
  double* rowp;   // 8 doubles per unit (GPFIT_SCORE_ROW_* order)
  double* colp;   // per segment 4 x kCols doubles (GPFIT_SCORE_COL_* order); may be null
};

// the lower lane's terms of one element: (mu - y)^2 and |(mu - y) / y|, every operation rounded
// on its own (numpy's terms bit for bit)
GP_DEV void score_resid(double mv, double y, double* sq, double* ape) {
#pragma clang fp contract(off)
  const double r = mv - y;
  *sq = r * r;
  *ape = fabs(r / y);
}

// KS = k-steps of 4 (P <= 4 KS), KT = list depth per tail.  Work units are (column panel, test
// point) pairs, panel-major; block i takes units [i U / B, (i + 1) U / B) of the U = npanels x m.
//
// SCORE (gp_field_score): the same chain, fold and merge, and instead of (or beside) the three
// stores the unit's terms against the truth Y.  After the merge the lane pair of a column (lanes
// 32 apart: lower tail, upper tail) trades l and h as stored; the lower lane forms the residual
// terms, the upper one the band terms.  Row sums: an xor-shuffle reduction over each 32-lane half,
// the four waves' results through LDS (two slots, alternating per unit, read after the tile loop's
// own barrier), one partial of 8 doubles per unit at rowp + 8 u.  Column sums: one double and one
// count per lane, kept while the block stays on a panel and stored per (block, panel) segment
// blockIdx + panel at colp.  Every partial has one writer and a fixed order: no atomics.
template <int KS, int KT, bool SCORE>
GP_DEV void summary_body(
    const double* __restrict__ W, long long ldw, long long lds, int S, int m, int P,
    const double* __restrict__ K, long long ldk, int ncols, const double* __restrict__ sd,
    const double* __restrict__ mu, const double* __restrict__ err, SumTail tlo, SumTail thi,
    void* __restrict__ mean, void* __restrict__ lo, void* __restrict__ hi, long long ldo,
    int out_f32, int nts, const ScoreK& sc) {
  constexpr int kRows = tile_rows<KS>(), RS = kRows / 16;
  __shared__ double ws[2][kRows * kPitch];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  // SCORE: the lane's column accumulator (lower lane: sum of squared residuals and valid count,
  // upper lane: sum of widths and covered count), the row slot in use
  [[maybe_unused]] double col_s = 0.0;
  [[maybe_unused]] int col_n = 0, rp = 0;
  [[maybe_unused]] double* rsh = nullptr;
  if constexpr (SCORE) {
    __shared__ double row_sh[2][kWaves][8];
    rsh = &row_sh[0][0][0];
  }
  // the finished unit's row partial: the four waves' sums in wave order
  [[maybe_unused]] auto flush_row = [&](long long unit) {
    if (threadIdx.x < 8) {
      const double* r = rsh + rp * (kWaves * 8) + threadIdx.x;
      sc.rowp[unit * 8 + threadIdx.x] = ((r[0] + r[8]) + r[16]) + r[24];
    }
    rp ^= 1;
  };
  [[maybe_unused]] auto flush_cols = [&](long long pan) {
    if (sc.colp) {
      const int idx = wv * kWaveCols + 16 * (lk & 1) + li;
      double* seg = sc.colp + ((long long)blockIdx.x + pan) * (4 * kCols) + idx;
      const bool upl = lk >> 1;
      seg[(upl ? 3 : 0) * kCols] = col_s;
      seg[(upl ? 2 : 1) * kCols] = (double)col_n;
    }
    col_s = 0.0;
    col_n = 0;
  };
  const long long npanels = (ncols + kCols - 1) / kCols;
  const long long units = npanels * m;
  const long long u0 = units * blockIdx.x / gridDim.x;
  const long long u1 = units * (blockIdx.x + 1) / gridDim.x;
  if (u0 >= u1) return;                                    // block-uniform
  const double inf = __builtin_inf();

  double b[KS][kJT];
  long long cur = -1;                                      // the panel held in b
  // (panel load, tile load / store and chain are field.hip's, written out: see the note there)
  auto load_panel = [&](long long panel) {
    const int c0 = (int)panel * kCols + wv * kWaveCols;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int jt = 0; jt < kJT; ++jt) {
        const int k = 4 * ks + lk, c = c0 + 16 * jt + li;
        b[ks][jt] = (k < P && c < ncols) ? K[(long long)k * ldk + c] : 0.0;
      }
    cur = panel;
  };

  // tile ts of point i (sample rows, stride lds) -> registers; the first kRows threads also
  // fetch their row's error scalar
  constexpr int KP = 4 * KS, NLD = tile_loads<KS>();        // padded inner dimension
  double pre[NLD], pre_e = -0.0;
  auto fetch_tile = [&](int i, int ts) {
    const int s0 = ts * kRows;
    const double* wp = W + (long long)i * ldw;
#pragma unroll
    for (int q = 0; q < NLD; ++q) {
      const int e = threadIdx.x + kThreads * q;
      const int r = e / KP, k = e % KP;
      pre[q] = (e < kRows * KP && k < P && s0 + r < S) ? wp[(long long)(s0 + r) * lds + k]
                                                     : 0.0;
    }
    if (err && threadIdx.x < kRows)
      pre_e = s0 + (int)threadIdx.x < S ? err[(long long)(s0 + (int)threadIdx.x) * m + i] : -0.0;
  };
  auto stage_tile = [&](int buf) {
#pragma unroll
    for (int q = 0; q < NLD; ++q) {
      const int e = threadIdx.x + kThreads * q;
      if (e < kRows * KP) ws[buf][(e / KP) * kPitch + e % KP] = pre[q];
    }
    if (threadIdx.x < kRows) ws[buf][threadIdx.x * kPitch + kSumErrCol] = pre_e;
  };

  // running state of the lane's two columns (tile jt, column li): rows lk + 4 q of every tile
  double sum[kJT], lo_l[kJT][KT], nh_l[kJT][KT], s_c[kJT], m_c[kJT];
  auto reset = [&](long long panel) {
    const int c0 = (int)panel * kCols + wv * kWaveCols;
#pragma unroll
    for (int jt = 0; jt < kJT; ++jt) {
      sum[jt] = 0.0;
#pragma unroll
      for (int i = 0; i < KT; ++i) lo_l[jt][i] = nh_l[jt][i] = inf;
      const int c = c0 + 16 * jt + li;
      // without sd / mu: fma(a, 1, -0) = a for every a, signed zeros included
      const bool ok = sd != nullptr && c < ncols;
      s_c[jt] = ok ? sd[c] : 1.0;
      m_c[jt] = ok ? mu[c] : -0.0;
    }
  };

  long long u = u0, panel = u0 / m;                        // unit u = panel * m + i
  int i = (int)(u0 - panel * m), ts = 0, buf = 0;
  fetch_tile(i, 0);
  stage_tile(0);
  __syncthreads();
  reset(panel);
  for (;;) {
    if (panel != cur) load_panel(panel);
    int tsn = ts + 1, in = i;
    long long un = u;
    if (tsn == nts) {
      tsn = 0;
      ++un;
      in = i + 1 == m ? 0 : i + 1;
    }
    const bool more = un < u1;
    if (more) fetch_tile(in, tsn);                         // in flight under the MFMAs
    f64x4 acc[RS][kJT];
#pragma unroll
    for (int rs = 0; rs < RS; ++rs)
#pragma unroll
      for (int jt = 0; jt < kJT; ++jt) acc[rs][jt] = zero4();
    const double* wt = ws[buf];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int rs = 0; rs < RS; ++rs) {
        const double a = wt[(16 * rs + li) * kPitch + 4 * ks + lk];
#pragma unroll
        for (int jt = 0; jt < kJT; ++jt)
          acc[rs][jt] = mfma16x16x4(a, b[ks][jt], acc[rs][jt]);
      }
    }
    // fold: sample row 16 rs + lk + 4 q of the tile, column 16 jt + li of the wave's panel
    const int s0 = ts * kRows;
    // (without err the scalar is -0: a + -0 = a for every a, as fma(a, 1, -0) = a without sd --
    // one code path for all four operand combinations keeps the register budget).
    // Rows past S are masked by the branch: their lanes execute none of the fold.
#pragma unroll
    for (int rs = 0; rs < RS; ++rs)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = 16 * rs + lk + 4 * q;
        if (s0 + r < S) {
          const double e = wt[r * kPitch + kSumErrCol];
#pragma unroll
          for (int jt = 0; jt < kJT; ++jt) {
            const double a = acc[rs][jt][q];
            const double y = fma(a, s_c[jt], m_c[jt]);
            const double z = fma(a + e, s_c[jt], m_c[jt]);
            sum[jt] += y;
            sum_insert<KT>(lo_l[jt], z);
            sum_insert<KT, true>(nh_l[jt], z);
          }
        }
      }

    if (tsn == 0) {
      // the unit is complete.  Exchange 1 (lanes 16 apart): the even lk keeps column tile 0 and
      // takes its partner's tile-0 state, the odd one tile 1.
      const bool odd = lk & 1, up = lk >> 1;
      [[maybe_unused]] double yv = __builtin_nan("");      // stays NaN: no truth for this element
      if constexpr (SCORE) {
        const int c = (int)panel * kCols + wv * kWaveCols + 16 * (int)odd + li;
        if (sc.Y && c < ncols) {                           // in flight under the merge
          const long long o = (long long)i * sc.ldy + c;
          yv = sc.y_f32 ? (double)static_cast<const float*>(sc.Y)[o]
                        : static_cast<const double*>(sc.Y)[o];
        }
      }
      double L[KT], N[KT], R[KT];
#pragma unroll
      for (int j = 0; j < KT; ++j) {
        L[j] = odd ? lo_l[1][j] : lo_l[0][j];
        R[j] = __shfl_xor(odd ? lo_l[0][j] : lo_l[1][j], 16);
      }
#pragma unroll
      for (int j = 0; j < KT; ++j) sum_insert<KT>(L, R[j]);
#pragma unroll
      for (int j = 0; j < KT; ++j) {
        N[j] = odd ? nh_l[1][j] : nh_l[0][j];
        R[j] = __shfl_xor(odd ? nh_l[0][j] : nh_l[1][j], 16);
      }
#pragma unroll
      for (int j = 0; j < KT; ++j) sum_insert<KT>(N, R[j]);
      double sm = (odd ? sum[1] : sum[0]) + __shfl_xor(odd ? sum[0] : sum[1], 16);
      // exchange 2 (lanes 32 apart): lk < 2 keeps the lower list, lk >= 2 the (negated) upper
      double F[KT];
#pragma unroll
      for (int j = 0; j < KT; ++j) {
        F[j] = up ? N[j] : L[j];
        R[j] = __shfl_xor(up ? L[j] : N[j], 32);
      }
#pragma unroll
      for (int j = 0; j < KT; ++j) sum_insert<KT>(F, R[j]);
      sm = sm + __shfl_xor(sm, 32);
      // the two order statistics of this lane's tail, its interpolation, the stores
      const int ia = up ? thi.ia : tlo.ia, ib = up ? thi.ib : tlo.ib;
      const double t = up ? thi.t : tlo.t;
      double va = F[0], vb = F[0];
#pragma unroll
      for (int j = 1; j < KT; ++j) {
        va = ia == j ? F[j] : va;
        vb = ib == j ? F[j] : vb;
      }
      if (up) {
        va = -va;
        vb = -vb;
      }
      const double qv = sum_lerp(va, vb, t);
      const int c = (int)panel * kCols + wv * kWaveCols + 16 * (int)odd + li;
      if constexpr (!SCORE) {
        if (c < ncols) {
          const long long o = (long long)i * ldo + c;
          void* qp = up ? hi : lo;
          if (out_f32) {
            static_cast<float*>(qp)[o] = static_cast<float>(qv);
            if (!up) static_cast<float*>(mean)[o] = static_cast<float>(sm / (double)S);
          } else {
            static_cast<double*>(qp)[o] = qv;
            if (!up) static_cast<double*>(mean)[o] = sm / (double)S;
          }
        }
      } else {
        const bool in_c = c < ncols;
        const double mv = sm / (double)S;
        // the values as stored (each output is optional), widened again
        const double qs = out_f32 ? (double)static_cast<float>(qv) : qv;
        const double ms = out_f32 ? (double)static_cast<float>(mv) : mv;
        if (in_c) {
          const long long o = (long long)i * ldo + c;
          void* qp = up ? hi : lo;
          if (out_f32) {
            if (qp) static_cast<float*>(qp)[o] = static_cast<float>(qv);
            if (!up && mean) static_cast<float*>(mean)[o] = static_cast<float>(mv);
          } else {
            if (qp) static_cast<double*>(qp)[o] = qv;
            if (!up && mean) static_cast<double*>(mean)[o] = mv;
          }
        }
        const double qo = __shfl_xor(qs, 32);              // the pair's other quantile
        const double lv = up ? qo : qs, hv = up ? qs : qo;
        const bool valid = yv == yv;                       // implies in_c and Y given
        double ta, tb, tc = 0.0;                           // this lane's three row terms
        int tn;                                            // and its counts, 8 bits each
        if (up) {
          const bool cov = valid && lv <= yv && yv <= hv;
          ta = in_c ? lv : 0.0;
          tb = in_c ? hv : 0.0;
          tn = cov;
          col_s += in_c ? hv - lv : 0.0;
          col_n += cov;
        } else {
          double sq = 0.0, ape = 0.0;
          if (valid) score_resid(ms, yv, &sq, &ape);
          const bool cnt = valid && !(yv < sc.floor);
          ta = sq;
          tb = cnt ? ape : 0.0;
          tc = in_c ? ms : 0.0;
          tn = (int)valid | ((int)cnt << 8);
          col_s += sq;
          col_n += valid;
        }
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) {                // within the 32-lane half
          ta += __shfl_xor(ta, d);
          tb += __shfl_xor(tb, d);
          tc += __shfl_xor(tc, d);
          tn += __shfl_xor(tn, d);
        }
        double* r = rsh + (rp * kWaves + wv) * 8;
        if (lane == 0) {
          r[0] = ta;
          r[1] = (double)(tn & 255);
          r[2] = tb;
          r[3] = (double)(tn >> 8);
          r[7] = tc;
        } else if (lane == 32) {
          r[4] = ta;
          r[5] = tb;
          r[6] = (double)tn;
        }
      }
    }
    if (!more) {
      if constexpr (SCORE) {
        __syncthreads();
        flush_row(u);
        flush_cols(panel);
      }
      break;
    }
    stage_tile(buf ^ 1);                                   // the other buffer: last read a tile ago
    __syncthreads();
    buf ^= 1;
    if (tsn == 0) {
      if constexpr (SCORE) {
        flush_row(u);
        if (in == 0) flush_cols(panel);
      }
      if (in == 0) ++panel;
      reset(panel);
    }
    ts = tsn;
    i = in;
    u = un;
  }
}

template <int KS, int KT>
__global__ __launch_bounds__(kThreads, (sum_occ<KS, KT>())) void summary_kernel(
    const double* __restrict__ W, long long ldw, long long lds, int S, int m, int P,
    const double* __restrict__ K, long long ldk, int ncols, const double* __restrict__ sd,
    const double* __restrict__ mu, const double* __restrict__ err, SumTail tlo, SumTail thi,
    void* __restrict__ mean, void* __restrict__ lo, void* __restrict__ hi, long long ldo,
    int out_f32, int nts) {
  summary_body<KS, KT, false>(W, ldw, lds, S, m, P, K, ldk, ncols, sd, mu, err, tlo, thi, mean,
                              lo, hi, ldo, out_f32, nts, ScoreK{});
}

template <int KS, int KT>
__global__ __launch_bounds__(kThreads, (sum_occ<KS, KT>())) void score_kernel(
    const double* __restrict__ W, long long ldw, long long lds, int S, int m, int P,
    const double* __restrict__ K, long long ldk, int ncols, const double* __restrict__ sd,
    const double* __restrict__ mu, const double* __restrict__ err, SumTail tlo, SumTail thi,
    void* __restrict__ mean, void* __restrict__ lo, void* __restrict__ hi, long long ldo,
    int out_f32, int nts, ScoreK sc) {
  summary_body<KS, KT, true>(W, ldw, lds, S, m, P, K, ldk, ncols, sd, mu, err, tlo, thi, mean,
                             lo, hi, ldo, out_f32, nts, sc);
}

// first block of a `grid`-block launch whose unit range [units b / grid, units (b + 1) / grid)
// holds unit u
GP_DEV long long score_block_of(long long u, long long units, long long grid) {
  long long b = u * grid / units;
  while (b + 1 < grid && units * (b + 1) / grid <= u) ++b;
  while (b > 0 && units * b / grid > u) --b;
  return b;
}

// The partials of score_kernel -> rows and cols, every sum in a fixed order.  Block i < m: row i,
// thread t adds the partials of panels t / 8 + 32 j for value t % 8, then thread k < 8 the 32
// strands in order.  The blocks after those: one thread per column, the segments of the blocks
// (of the `grid` that ran) whose unit range meets the column's panel, in block order.
__global__ __launch_bounds__(256) void score_reduce_kernel(
    const double* __restrict__ rowp, const double* __restrict__ colp, int m, int ncols,
    long long npanels, long long grid, double* __restrict__ rows, double* __restrict__ cols) {
  __shared__ double sh[256];
  if ((int)blockIdx.x < m) {
    const int i = blockIdx.x, k = threadIdx.x & 7;
    double s = 0.0;
    for (long long p = threadIdx.x >> 3; p < npanels; p += 32) s += rowp[(p * m + i) * 8 + k];
    sh[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < 8) {
      double t = 0.0;
      for (int g = 0; g < 32; ++g) t += sh[8 * g + threadIdx.x];
      rows[(long long)i * 8 + threadIdx.x] = t;
    }
    return;
  }
  const long long c = (long long)(blockIdx.x - m) * 256 + threadIdx.x;
  if (c >= ncols) return;
  const long long p = c / kCols, units = npanels * m;
  const int idx = (int)(c % kCols);
  const long long b0 = score_block_of(p * m, units, grid);
  const long long b1 = score_block_of(p * m + m - 1, units, grid);
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (long long b = b0; b <= b1; ++b) {
    const double* seg = colp + (b + p) * (4 * kCols) + idx;
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] += seg[j * kCols];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) cols[c * 4 + j] = a[j];
}

struct SumArgs {
  const double* W;
  long long ldw, lds;
  int S, m, P;
  const double* K;
  long long ldk;
  int ncols;
  const double *sd, *mu, *err;
  SumTail tlo, thi;
  void *mean, *lo, *hi;
  long long ldo;
  int out_f32;
  hipStream_t stream;
  ScoreK sc;      // gp_field_score only
  double *rows, *cols;
};

// blocks of the score launch: one residency round as the summary's, and never more than the
// workspace has segments for
constexpr long long kScoreMaxBlocks = 2048;

// the summary (SCORE = false) or the score kernel and its reduction, on the grid of one residency
// round of that instantiation
template <int KS, int KT, bool SCORE>
hipError_t launch_summary(const SumArgs& a) {
  const long long npanels = gp_ceil_div(a.ncols, kCols), units = npanels * a.m;
  const int nts = (a.S + tile_rows<KS>() - 1) / tile_rows<KS>();
  if constexpr (!SCORE) {
    constexpr auto kernel = summary_kernel<KS, KT>;
    const long long blocks = round_blocks(blocks_per_cu<kernel>(sum_occ<KS, KT>()), units);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kThreads), 0, a.stream, a.W, a.ldw,
                       a.lds, a.S, a.m, a.P, a.K, a.ldk, a.ncols, a.sd, a.mu, a.err, a.tlo, a.thi,
                       a.mean, a.lo, a.hi, a.ldo, a.out_f32, nts);
    return hipGetLastError();
  } else {
    constexpr auto kernel = score_kernel<KS, KT>;
    long long blocks = round_blocks(blocks_per_cu<kernel>(sum_occ<KS, KT>()), units);
    if (blocks > kScoreMaxBlocks) blocks = kScoreMaxBlocks;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kThreads), 0, a.stream, a.W, a.ldw,
                       a.lds, a.S, a.m, a.P, a.K, a.ldk, a.ncols, a.sd, a.mu, a.err, a.tlo, a.thi,
                       a.mean, a.lo, a.hi, a.ldo, a.out_f32, nts, a.sc);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const unsigned rblocks = (unsigned)a.m + (a.cols ? (unsigned)gp_ceil_div(a.ncols, 256) : 0u);
    hipLaunchKernelGGL(score_reduce_kernel, dim3(rblocks), dim3(256), 0, a.stream, a.sc.rowp,
                       a.sc.colp, a.m, a.ncols, npanels, blocks, a.rows, a.cols);
    return hipGetLastError();
  }
}

// numpy's "linear" rule: pos = q (S - 1), j = floor(pos), t = pos - j
void summary_position(double q, int S, int* j, double* t) {
  const double pos = q * (double)(S - 1);
  const double f = floor(pos);
  *j = (int)f;
  *t = pos - f;
}

// the checks gp_field_summary and gp_field_score share (arguments 1-14, the same numbers in
// both), and the two tails of a valid request
int summary_check(const double* W, long long ldw, long long lds, int S, int m, int P,
                  const double* K, long long ldk, int ncols, const double* sd, const double* mu,
                  double q_lo, double q_hi, SumTail* a_lo, SumTail* a_hi, int* depth) {
  if (!W) return -1;
  if (ldw < P || ldw < 1) return -2;
  if (lds < 1 || lds < (m > 0 ? m - 1 : 0) * ldw + P) return -3;
  if (S < 1) return -4;
  if (m < 0) return -5;
  if (P < 1 || P > kMaxP) return -6;
  if (!K) return -7;
  if (ldk < ncols || ldk < 1) return -8;
  if (ncols < 0) return -9;
  if ((sd == nullptr) != (mu == nullptr)) return -10;
  if (!(q_lo >= 0.0 && q_lo <= 1.0)) return -13;
  if (!(q_hi >= 0.0 && q_hi <= 1.0) || q_lo > q_hi) return -14;
  // selection depth: the lower tail reads z_(j), z_(j+1) of the ascending order, the upper one
  // the same two counted from the top
  int jl, jh;
  double tl, th;
  summary_position(q_lo, S, &jl, &tl);
  summary_position(q_hi, S, &jh, &th);
  const int dlo = jl + 2 < S ? jl + 2 : S, dhi = S - jh;
  if (dlo > kSumMaxTail) return -13;
  if (dhi > kSumMaxTail) return -14;
  const int jl1 = jl + 1 < S ? jl + 1 : jl, jh1 = jh + 1 < S ? jh + 1 : jh;
  // the upper list holds -z ascending: z_(j) is its entry S - 1 - j
  *a_lo = {jl, jl1, jl1 == jl ? 0.0 : tl};
  *a_hi = {S - 1 - jh, S - 1 - jh1, jh1 == jh ? 0.0 : th};
  *depth = dlo > dhi ? dlo : dhi;
  return 0;
}

// KT = the instantiated list depth 2 / 4 / 8 that holds `depth`
template <bool SCORE>
hipError_t dispatch_summary(const SumArgs& a, int depth) {
  return dispatch_ks(a.P, [&](auto ks) {
    constexpr int KS = decltype(ks)::value;
    return depth <= 2   ? launch_summary<KS, 2, SCORE>(a)
           : depth <= 4 ? launch_summary<KS, 4, SCORE>(a)
                        : launch_summary<KS, 8, SCORE>(a);
  });
}

// workspace of gp_field_score: the row partials (8 doubles per unit), then the column segments
long long score_ws_layout(long long m, long long ncols, long long* col_off) {
  const long long npanels = (ncols + kCols - 1) / kCols, units = npanels * m;
  const long long nb = units < kScoreMaxBlocks ? units : kScoreMaxBlocks;
  const long long rows_b = align256(units * 8 * (long long)sizeof(double));
  if (col_off) *col_off = rows_b;
  return rows_b + align256((npanels + nb - 1) * 4 * kCols * (long long)sizeof(double));
}

}  // namespace

extern "C" int gp_field_summary_max_tail(void) { return kSumMaxTail; }

extern "C" int gp_field_summary(const double* W, long long ldw, long long lds, int S, int m, int P,
                                const double* K, long long ldk, int ncols, const double* sd,
                                const double* mu, const double* err, double q_lo, double q_hi,
                                void* mean, void* lo, void* hi, long long ldo, int out_f32,
                                hipStream_t stream) {
  SumTail a_lo, a_hi;
  int depth;
  const int rc = summary_check(W, ldw, lds, S, m, P, K, ldk, ncols, sd, mu, q_lo, q_hi, &a_lo,
                               &a_hi, &depth);
  if (rc) return rc;
  if (!mean) return -15;
  if (!lo) return -16;
  if (!hi) return -17;
  if (ldo < ncols || ldo < 1) return -18;
  if (m == 0 || ncols == 0) return 0;
  const SumArgs a = {W, ldw, lds, S, m, P, K, ldk, ncols, sd, mu, err, a_lo, a_hi,
                     mean, lo, hi, ldo, out_f32, stream, ScoreK{}, nullptr, nullptr};
  const hipError_t e = dispatch_summary<false>(a, depth);
  return e == hipSuccess ? 0 : GPFIT_ERR_HIP - (int)e;
}

extern "C" long long gp_field_score_ws_bytes(int S, int m, int P, int ncols) {
  if (S < 1 || m < 0 || P < 1 || ncols < 0) return -1;
  if (m == 0 || ncols == 0) return 0;
  return score_ws_layout(m, ncols, nullptr);
}

extern "C" int gp_field_score(const double* W, long long ldw, long long lds, int S, int m, int P,
                              const double* K, long long ldk, int ncols, const double* sd,
                              const double* mu, const double* err, double q_lo, double q_hi,
                              const void* Y, long long ldy, int y_f32, double mape_floor,
                              void* mean, void* lo, void* hi, long long ldo, int out_f32,
                              double* rows, double* cols, void* ws, long long ws_bytes,
                              hipStream_t stream) {
  SumTail a_lo, a_hi;
  int depth;
  const int rc = summary_check(W, ldw, lds, S, m, P, K, ldk, ncols, sd, mu, q_lo, q_hi, &a_lo,
                               &a_hi, &depth);
  if (rc) return rc;
  if (Y && (ldy < ncols || ldy < 1)) return -16;
  if (y_f32 != 0 && y_f32 != 1) return -17;
  if ((mean || lo || hi) && (ldo < ncols || ldo < 1)) return -22;
  if (out_f32 != 0 && out_f32 != 1) return -23;
  if (!rows) return -24;
  if (m == 0 || ncols == 0) return 0;
  long long col_off;
  const long long need = score_ws_layout(m, ncols, &col_off);
  if (!ws || ((size_t)ws & 255)) return -26;
  if (ws_bytes < need) return -27;
  const ScoreK sc = {Y, ldy, y_f32, mape_floor, static_cast<double*>(ws),
                     cols ? reinterpret_cast<double*>(static_cast<char*>(ws) + col_off)
                          : nullptr};
  const SumArgs a = {W, ldw, lds, S, m, P, K, ldk, ncols, sd, mu, err, a_lo, a_hi,
                     mean, lo, hi, ldo, out_f32, stream, sc, rows, cols};
  const hipError_t e = dispatch_summary<true>(a, depth);
  return e == hipSuccess ? 0 : GPFIT_ERR_HIP - (int)e;
}
