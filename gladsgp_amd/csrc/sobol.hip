// Saltelli estimators of the Sobol' sensitivity indices over R replicates of the design rows:
// the statistic the reference's bootstrap evaluates 4 x 9,999 (+ 4 N jackknife) times in
// interpreted numpy on fancy-indexed (d, N, p) arrays (src/utils.py:27-256, called from
// sensitivity_indices.py:96,214).  One launch computes first-order and total indices of every
// output and input for every replicate; a second small one forms the pcvar-weighted general
// indices.  The formulas are in include/gpfit.h.
//
// Mapping: one 256-thread block per (output j, block of 64 replicates).  The block stages the
// (d + 2) N doubles of output j -- fA, fB and fAB_0 .. fAB_{d-1}, each contiguous in the
// output-major operand layout -- into LDS once, row-interleaved: row k holds a, b, c_0 .. c_{d-1}
// at pitch d + 2 rounded up to even, so a gathered row is read as 16-byte pairs (ds_read_b128;
// the row index is random, so is the bank, whatever the pitch).  A group of 16 lanes owns one
// replicate (16 replicates in flight per block, 4 rounds per block): lane s of the group takes
// the 4-row chunks q = s, s + 16, ... (rows k = 4 q .. 4 q + 3, one Philox block per chunk),
// accumulates them in order and the group reduces by a fixed xor tree (8, 4, 2, 1).  The order
// of every sum depends on (M, k) alone, never on the mode, so modes that select the same rows
// give the same bits.  The variance is two-pass: the second pass needs the rows again, so the
// first 4 chunks per lane (256 rows per replicate: all of the reference's N = 256) stay in
// registers and later ones are drawn again.  Inputs are handled 8 at a time (d <= 8: one pass).
// N > gp_sobol_lds_points(d) (the working set above 64 KiB): the same kernel gathers from global
// memory, which stays L2-resident.  No atomics; nothing is allocated; all arithmetic is fp64.
#include "gpfit_common.h"
#include "philox.h"
#include "../../include/gpfit.h"

namespace {

constexpr int kSobThreads = 256;
constexpr int kSobGroup = 16;                          // lanes per replicate
constexpr int kSobGroups = kSobThreads / kSobGroup;    // replicates in flight per block
constexpr int kSobRepBlock = 64;                       // replicates per block
constexpr int kSobTile = 8;                            // inputs per pass over the rows
constexpr int kSobCache = 4;                           // 4-row chunks per lane kept in registers
constexpr long long kSobLdsBytes = 65536;              // LDS working set limit per block
constexpr int kSobMaxN = 1 << 20;

struct SobArgs {
  const double *fA, *fB, *fAB;
  long long ldf, strideAB;
  int N, p, d, mode;
  const int* idx;
  long long ldi;
  int M, R;
  uint64_t seed, offset;
  int clamp;
  double *first, *total;
  long long ldr;
};

__host__ __device__ inline int sob_pitch(int d) { return (d + 3) & ~1; }   // d + 2, even

// rows i_k of replicate r for k = 4 q .. 4 q + 3; entries with k >= M are in range and unused
GP_DEV void sob_rows(const SobArgs& a, long long r, long long q, int (&row)[4]) {
  const long long k0 = 4 * q;
  const int last = a.N - 1;
  if (a.mode == GPFIT_SOBOL_PHILOX) {
    uint32_t c[4] = {(uint32_t)q, (uint32_t)r, (uint32_t)a.offset, (uint32_t)(a.offset >> 32)};
    philox4x32_10(c, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
#pragma unroll
    for (int e = 0; e < 4; ++e) row[e] = (int)(((uint64_t)c[e] * (uint32_t)a.N) >> 32);
  } else if (a.mode == GPFIT_SOBOL_INDEX) {
    const int* ip = a.idx + r * a.ldi;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int v = k0 + e < a.M ? ip[k0 + e] : 0;
      row[e] = v < 0 ? 0 : (v > last ? last : v);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long long k = k0 + e + (a.mode == GPFIT_SOBOL_JACKKNIFE && k0 + e >= r ? 1 : 0);
      row[e] = k > last ? last : (int)k;
    }
  }
}

// a, b and (WITH_C) the 8 inputs i0 .. i0 + 7 of one design row; inputs >= d read 0 or padding
template <bool LDS, bool WITH_C>
GP_DEV void sob_load(const SobArgs& a, const double* S, int pitch, const double* A,
                     const double* B, const double* AB, int row, int i0, double& av, double& bv,
                     double (&c)[kSobTile]) {
  if (LDS) {
    const double2* p = reinterpret_cast<const double2*>(S + (size_t)row * pitch);
    const double2 ab = p[0];
    av = ab.x;
    bv = ab.y;
    if (WITH_C) {
#pragma unroll
      for (int t = 0; t < kSobTile / 2; ++t) {
        double2 v = {0.0, 0.0};
        if (i0 + 2 * t < a.d) v = p[1 + (i0 >> 1) + t];
        c[2 * t] = v.x;
        c[2 * t + 1] = v.y;
      }
    }
  } else {
    av = A[row];
    bv = B[row];
    if (WITH_C) {
#pragma unroll
      for (int i = 0; i < kSobTile; ++i)
        c[i] = i0 + i < a.d ? AB[(long long)(i0 + i) * a.strideAB + row] : 0.0;
    }
  }
}

// sum over the 16 lanes of a replicate's group, the same tree in every lane
GP_DEV double sob_sum16(double x) {
#pragma unroll
  for (int o = kSobGroup / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, kSobGroup);
  return x;
}

template <bool LDS>
__global__ __launch_bounds__(kSobThreads) void sobol_kernel(SobArgs a) {
  extern __shared__ double2 sob_lds[];
  double* S = reinterpret_cast<double*>(sob_lds);
  const int j = (int)(blockIdx.x % (unsigned)a.p);
  const long long rb = blockIdx.x / (unsigned)a.p;
  const double* A = a.fA + (long long)j * a.ldf;
  const double* B = a.fB + (long long)j * a.ldf;
  const double* AB = a.fAB + (long long)j * a.ldf;       // input i: + i strideAB
  const int pitch = sob_pitch(a.d);
  if (LDS) {
    for (int v = 0; v < pitch; ++v) {
      const double* src = v == 0 ? A : v == 1 ? B : AB + (long long)(v - 2) * a.strideAB;
      const bool pad = v >= a.d + 2;
      for (int k = threadIdx.x; k < a.N; k += kSobThreads)
        S[(size_t)k * pitch + v] = pad ? 0.0 : src[k];
    }
    __syncthreads();
  }
  const int sub = threadIdx.x % kSobGroup, grp = threadIdx.x / kSobGroup;
  const long long r0 = rb * kSobRepBlock;
  const long long r1 = r0 + kSobRepBlock < a.R ? r0 + kSobRepBlock : a.R;
  const long long M = a.M;
  const double Md = (double)a.M, M2 = 2.0 * (double)a.M;

  // no barrier below: every group runs its own replicates
  for (long long r = r0 + grp; r < r1; r += kSobGroups) {
    int cache[kSobCache][4];
    // f(row) for the rows of this lane's chunks, in k order; FILL draws the cached chunks
    auto for_rows = [&](auto fill, auto&& f) {
#pragma unroll
      for (int t = 0; t < kSobCache; ++t) {
        const long long q = sub + kSobGroup * t;
        if (4 * q < M) {
          if (decltype(fill)::value) sob_rows(a, r, q, cache[t]);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (4 * q + e < M) f(cache[t][e]);
        }
      }
      for (long long q = sub + kSobGroup * kSobCache; 4 * q < M; q += kSobGroup) {
        int row[4];
        sob_rows(a, r, q, row);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (4 * q + e < M) f(row[e]);
      }
    };

    double var = 0.0;
    for (int i0 = 0; i0 < a.d; i0 += kSobTile) {
      double sa = 0.0, sb = 0.0, V[kSobTile], E[kSobTile];
#pragma unroll
      for (int i = 0; i < kSobTile; ++i) V[i] = E[i] = 0.0;
      auto body = [&](int row) {
        double av, bv, c[kSobTile];
        sob_load<LDS, true>(a, S, pitch, A, B, AB, row, i0, av, bv, c);
        sa += av;
        sb += bv;
#pragma unroll
        for (int i = 0; i < kSobTile; ++i) {
          const double df = c[i] - bv;
          V[i] = fma(av, df, V[i]);
          E[i] = fma(df, df, E[i]);
        }
      };
      if (i0 == 0) {
        for_rows(std::true_type{}, body);
        const double mu = (sob_sum16(sa) + sob_sum16(sb)) / M2;
        double qa = 0.0, qb = 0.0;
        for_rows(std::false_type{}, [&](int row) {
          double av, bv, c[kSobTile];
          sob_load<LDS, false>(a, S, pitch, A, B, AB, row, 0, av, bv, c);
          const double da = av - mu, db = bv - mu;
          qa = fma(da, da, qa);
          qb = fma(db, db, qb);
        });
        var = (sob_sum16(qa) + sob_sum16(qb)) / M2;
      } else {
        for_rows(std::false_type{}, body);
      }
      // lane s < 8 of the group stores input i0 + s
      double v = 0.0, e = 0.0;
#pragma unroll
      for (int i = 0; i < kSobTile; ++i) {
        const double vi = sob_sum16(V[i]), ei = sob_sum16(E[i]);
        if (sub == i) {
          v = vi;
          e = ei;
        }
      }
      if (sub < kSobTile && i0 + sub < a.d) {
        v = v / Md;
        if (a.clamp && v < 0.0) v = 0.0;
        const long long o = r * a.ldr + (long long)j * a.d + i0 + sub;
        a.first[o] = v / var;
        a.total[o] = (e / M2) / var;
      }
    }
  }
}

// general indices: thread (r, i) sums pcvar[j] x[r, j, i] in increasing j
__global__ __launch_bounds__(256) void sobol_general_kernel(
    const double* __restrict__ first, const double* __restrict__ total, long long ldr,
    const double* __restrict__ pcvar, int p, int d, int R, double* __restrict__ gfirst,
    double* __restrict__ gtotal, long long ldg) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)R * d) return;
  const long long r = t / d;
  const int i = (int)(t % d);
  double gf = 0.0, gt = 0.0;
  for (int j = 0; j < p; ++j) {
    const long long o = r * ldr + (long long)j * d + i;
    gf = fma(pcvar[j], first[o], gf);
    gt = fma(pcvar[j], total[o], gt);
  }
  gfirst[r * ldg + i] = gf;
  gtotal[r * ldg + i] = gt;
}

}  // namespace

extern "C" long long gp_sobol_lds_points(int d) {
  if (d < 1 || d > GPFIT_MAX_DIM) return 0;
  const long long n = kSobLdsBytes / (8LL * sob_pitch(d));
  return n < kSobMaxN ? n : kSobMaxN;
}

extern "C" int gp_sobol_replicates(const double* fA, const double* fB, const double* fAB,
                                   long long ldf, long long strideAB, int N, int p, int d,
                                   int mode, const int* idx, long long ldi, int n_draw, int R,
                                   unsigned long long seed, unsigned long long offset,
                                   const double* pcvar, int clamp, double* first, double* total,
                                   long long ldr, double* gfirst, double* gtotal, long long ldg,
                                   hipStream_t stream) {
  if (!fA) return -1;
  if (!fB) return -2;
  if (!fAB) return -3;
  if (N < 2 || N > kSobMaxN) return -6;
  if (p < 1) return -7;
  if (d < 1 || d > GPFIT_MAX_DIM) return -8;
  if (ldf < N) return -4;
  if (strideAB < (long long)(p - 1) * ldf + N) return -5;
  if (mode < GPFIT_SOBOL_IDENTITY || mode > GPFIT_SOBOL_JACKKNIFE) return -9;
  if (mode == GPFIT_SOBOL_INDEX && !idx) return -10;
  if (n_draw < 1) return -12;
  if (mode == GPFIT_SOBOL_IDENTITY && n_draw != N) return -12;
  if (mode == GPFIT_SOBOL_JACKKNIFE && n_draw != N - 1) return -12;
  if (mode == GPFIT_SOBOL_INDEX && ldi < n_draw) return -11;
  if (R < 0) return -13;
  if (mode == GPFIT_SOBOL_IDENTITY && R != 1) return -13;
  if (mode == GPFIT_SOBOL_JACKKNIFE && R != N) return -13;
  if (!pcvar && (gfirst || gtotal)) return -16;
  if (!first) return -18;
  if (!total) return -19;
  if (ldr < (long long)p * d) return -20;
  if (pcvar && !gfirst) return -21;
  if (pcvar && !gtotal) return -22;
  if (pcvar && ldg < d) return -23;
  const long long blocks = (long long)p * gp_ceil_div(R, kSobRepBlock);
  if (blocks > 0x7fffffffLL) return -13;
  if (R == 0) return 0;

  const SobArgs a = {fA, fB, fAB, ldf, strideAB, N, p, d, mode, idx, ldi, n_draw, R,
                     (uint64_t)seed, (uint64_t)offset, clamp, first, total, ldr};
  if (N <= gp_sobol_lds_points(d)) {
    const size_t lds = (size_t)N * sob_pitch(d) * sizeof(double);
    hipLaunchKernelGGL(sobol_kernel<true>, dim3((unsigned)blocks), dim3(kSobThreads), lds, stream,
                       a);
  } else {
    hipLaunchKernelGGL(sobol_kernel<false>, dim3((unsigned)blocks), dim3(kSobThreads), 0, stream,
                       a);
  }
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && pcvar) {
    const long long th = (long long)R * d;
    hipLaunchKernelGGL(sobol_general_kernel, dim3((unsigned)gp_ceil_div(th, 256)), dim3(256), 0,
                       stream, first, total, ldr, pcvar, p, d, R, gfirst, gtotal, ldg);
    e = hipGetLastError();
  }
  return e == hipSuccess ? 0 : GPFIT_ERR_HIP - (int)e;
}
