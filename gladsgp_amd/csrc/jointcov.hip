// Joint predictive covariance of a block of test points and joint posterior draws.
//
// Reference replaced: SepiaEmulatorPrediction forms the full m x m predictive covariance of every
// (sample, PC) GP over the test points of a call and draws the PC weights from it jointly
// (SURVEY §8a A8).  predict.hip gives the mean and the covariance's diagonal; here, with
// V = L^-1 K* (n x m) from the L^-1 of gp_potrf_inv,
//   C = K** + (s_pred + jitter - s) I - V^T V            (gp_predict_cov)
//   out = mean + tril(R) xi,  R = chol(C)                (gp_mvn_draw, after gp_potrf)
//
// Per call of gp_predict_cov, with T = 128 for m > 64 and 64 otherwise:
//   1. cross_kp (predict.hip)  Kt = K*, npad x mp k-major rows of mp = T ceil(m / T) test
//                              points: the very values gp_predict multiplies
//   2. jc_trmm                 V = L^-1 Kt, one T x T tile per block, k < T (R + 1) only; L^-1
//                              masked to k <= r < n while it is staged; V stored k-major
//   3. jc_syrk                 one lower T x T tile (I, J <= I) of C per block: acc = sum_k
//                              V[k, I] V[k, J] with both operands k-major rows of V, then the
//                              prior term from Xs, the subtraction, the tile and its mirror
// Both products run on v_mfma_f64_16x16x4_f64 with k ascending in one block per tile: no
// atomics, no split-K, so equal inputs give equal bits and a problem's result does not depend on
// its neighbours in the batch.
#include "gpfit_common.h"
#include "philox.h"
#include "gpfit_internal.h"
#include "../../include/gpfit.h"

namespace {

// Square tiles of T = 32 NT rows and columns per 256-thread block, 4 waves as 2 x 2, each wave
// NT x NT MFMA tiles: NT = 4 (128 x 128, 16 flop per byte staged: what keeps the products off
// the L2's bandwidth, as predict.hip's pair kernel) when m > 64, NT = 2 (64 x 64) for the
// reference's small blocks of test points, where a 128-column tile would be mostly padding.
constexpr int JK = 16;        // k per staged step
constexpr int kMaxGridZ = 32768;

template <int NT>
struct Tile {
  static constexpr int T = 32 * NT;
  // LDS row pitch in doubles: T + 16 (640 B / 1152 B), so the k rows lk and lk + 1 of a
  // fragment read sit 32 banks apart
  static constexpr int P = T + 16;
  static constexpr int V2 = NT;       // double2 per thread and operand of one staged step
};

// 128 x 128 tiles hold 128 accumulator registers per lane: two waves per SIMD (256 registers
// each), the occupancy predict.hip's pair kernel runs at; the 64 x 64 tiles are left to the
// compiler.
#define JC_WAVES(NT) __attribute__((amdgpu_waves_per_eu((NT) == 4 ? 2 : 1, (NT) == 4 ? 2 : 8)))

GP_DEV int round_up(int a, int b) { return (a + b - 1) / b * b; }

// One staged step: 16 k of a wave's NT x NT MFMA tiles.  skip: the wave's first `skip` row tiles
// lie wholly above the diagonal of L^-1 at this step (wave-uniform).
template <int NT>
GP_DEV void jc_stage(const double* __restrict__ As, const double* __restrict__ Bs,
                     f64x4 (&acc)[NT][NT], int wr, int wc, int li, int lk, int skip) {
  constexpr int P = Tile<NT>::P;
#pragma unroll
  for (int k4 = 0; k4 < JK / 4; ++k4) {
    const int k = k4 * 4 + lk;
    double a[NT], bb[NT];
#pragma unroll
    for (int mi = 0; mi < NT; ++mi) a[mi] = As[k * P + (wr * NT + mi) * 16 + li];
#pragma unroll
    for (int nj = 0; nj < NT; ++nj) bb[nj] = Bs[k * P + (wc * NT + nj) * 16 + li];
#pragma unroll
    for (int mi = 0; mi < NT; ++mi) {
      if (mi < skip) continue;
#pragma unroll
      for (int nj = 0; nj < NT; ++nj) acc[mi][nj] = mfma16x16x4(a[mi], bb[nj], acc[mi][nj]);
    }
  }
}

// Stage registers -> LDS (row skk, columns sc ..) of both operands.
template <int NT>
GP_DEV void jc_put(double* As, double* Bs, const double (&ra)[2 * NT], const double (&rb)[2 * NT],
                   int skk, int sc) {
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    double2 va, vb;
    va.x = ra[2 * q];
    va.y = ra[2 * q + 1];
    vb.x = rb[2 * q];
    vb.y = rb[2 * q + 1];
    *reinterpret_cast<double2*>(As + skk * Tile<NT>::P + sc + 2 * q) = va;
    *reinterpret_cast<double2*>(Bs + skk * Tile<NT>::P + sc + 2 * q) = vb;
  }
}

struct JcTrmmArgs {
  const double* Linv;   // padded L^-1, column k at k * ld
  int ld;
  long long sL;
  const double* Kt;     // npad x mp, k-major
  double* V;            // nr x mp, k-major (nr = T ceil(n / T))
  long long sK, sV;
  int mp, n, nrt, nct;  // row and column tiles per problem
};

// V tile (R, Cc) = sum_{k < min(T (R + 1), 16 ceil(n / 16))} Linv[R, k] Kt[k, Cc].  Operands pass
// through registers into LDS one step ahead; the mask k <= r < n is applied on the way, so
// nothing above the diagonal or in the padding rows of the buffer reaches a product.  Blocks
// are numbered problem-major through xcd_remap (a problem's tiles share an XCD's L2: its L^-1
// rows and K* panels are read by several of them), row tiles longest first.
template <int NT>
__global__ __launch_bounds__(256) JC_WAVES(NT) void jc_trmm_kernel(const JcTrmmArgs a) {
  constexpr int T = Tile<NT>::T, P = Tile<NT>::P, V2 = Tile<NT>::V2;
  __shared__ __attribute__((aligned(16))) double As[JK * P];
  __shared__ __attribute__((aligned(16))) double Bs[JK * P];
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int per = a.nrt * a.nct;
  const int b = lid / per, t = lid - b * per;
  const int R0 = (a.nrt - 1 - t / a.nct) * T, C0 = (t % a.nct) * T;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = w >> 1, wc = w & 1, li = lane & 15, lk = lane >> 4;
  const int skk = tid >> 4, sc = (tid & 15) * (2 * V2);   // staged row k, first of 2 V2 columns
  const double* L = a.Linv + b * a.sL + R0 + sc;
  const double* K = a.Kt + b * a.sK + C0 + sc;
  const int n = a.n;
  const int nsteps = min(R0 + T, round_up(n, JK)) / JK;

  double ra[2 * V2], rb[2 * V2];
  auto load = [&](int s) {
    const int k = s * JK + skk;
    const double2* lp = reinterpret_cast<const double2*>(L + (long long)k * a.ld);
    const double2* kp = reinterpret_cast<const double2*>(K + (long long)k * a.mp);
#pragma unroll
    for (int q = 0; q < V2; ++q) {
      const double2 va = lp[q], vb = kp[q];
      const int r = R0 + sc + 2 * q;
      ra[2 * q] = (k <= r && r < n) ? va.x : 0.0;
      ra[2 * q + 1] = (k <= r + 1 && r + 1 < n) ? va.y : 0.0;
      rb[2 * q] = vb.x;
      rb[2 * q + 1] = vb.y;
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
    jc_put<NT>(As, Bs, ra, rb, skk, sc);
    __syncthreads();
    if (s + 1 < nsteps) load(s + 1);
    // inside the diagonal block the wave's row tile mi (rows R0 + 16 (NT wr + mi) ...) meets
    // only zeros from step k0 >= its last row + 1 on
    const int over = s * JK - (R0 + wr * NT * 16);
    const int skip = over < 16 ? 0 : over / 16;
    if (skip < NT) jc_stage<NT>(As, Bs, acc, wr, wc, li, lk, skip);
  }

  double* Vb = a.V + b * a.sV + C0;
#pragma unroll
  for (int mi = 0; mi < NT; ++mi)
#pragma unroll
    for (int nj = 0; nj < NT; ++nj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = R0 + (wr * NT + mi) * 16 + lk + 4 * r;
        Vb[(long long)row * a.mp + (wc * NT + nj) * 16 + li] = acc[mi][nj][r];
      }
}

struct JcSyrkArgs {
  const double* V;      // nr x mp, k-major
  long long sV;
  const double* Xs;
  int ldxs, d;
  const double* beta;
  int ldbeta;
  const double *s, *s_pred, *jitter;
  double* C;
  int ldc;
  long long sC;
  int mp, m, n, nt;     // nt: tiles per side, nt (nt + 1) / 2 lower tiles per problem
};

// Lower tile (I, J <= I) of C.  Both MFMA operands are k-major rows of V: A[i][k] = V[k, I0 + i],
// B[k][j] = V[k, J0 + j].  Epilogue: the tiles' test points and beta into LDS, the prior term
// s exp(-sum beta (xs_i - xs_j)^2) (s_pred + jitter on the diagonal) minus the product, written
// for j <= i at (i, j) and (j, i): both triangles from one value.  Blocks problem-major through
// xcd_remap, as jc_trmm_kernel's.
template <int NT, int D>
__global__ __launch_bounds__(256) JC_WAVES(NT) void jc_syrk_kernel(const JcSyrkArgs a) {
  constexpr int T = Tile<NT>::T, P = Tile<NT>::P, V2 = Tile<NT>::V2;
  constexpr int XP = D + 1;
  constexpr int kStage = 2 * JK * P, kEpi = 2 * T * XP + D;
  __shared__ __attribute__((aligned(16))) double smem[kStage > kEpi ? kStage : kEpi];
  double* As = smem;
  double* Bs = smem + JK * P;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int per = a.nt * (a.nt + 1) / 2;
  const int b = lid / per, t = lid - b * per;           // t = I (I + 1) / 2 + J
  int I = (int)((__builtin_sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  while (I * (I + 1) / 2 > t) --I;
  const int J = t - I * (I + 1) / 2;
  const int I0 = I * T, J0 = J * T;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = w >> 1, wc = w & 1, li = lane & 15, lk = lane >> 4;
  const int skk = tid >> 4, sc = (tid & 15) * (2 * V2);
  const int nsteps = round_up(a.n, JK) / JK;
  const double* Vi = a.V + b * a.sV + I0 + sc;
  const double* Vj = a.V + b * a.sV + J0 + sc;

  double ra[2 * V2], rb[2 * V2];
  auto load = [&](int s) {
    const long long off = (long long)(s * JK + skk) * a.mp;
    const double2* ip = reinterpret_cast<const double2*>(Vi + off);
    const double2* jp = reinterpret_cast<const double2*>(Vj + off);
#pragma unroll
    for (int q = 0; q < V2; ++q) {
      const double2 va = ip[q], vb = jp[q];
      ra[2 * q] = va.x;
      ra[2 * q + 1] = va.y;
      rb[2 * q] = vb.x;
      rb[2 * q + 1] = vb.y;
    }
  };

  f64x4 acc[NT][NT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = zero4();

  if (nsteps > 0) load(0);
  for (int s = 0; s < nsteps; ++s) {
    __syncthreads();
    jc_put<NT>(As, Bs, ra, rb, skk, sc);
    __syncthreads();
    if (s + 1 < nsteps) load(s + 1);
    jc_stage<NT>(As, Bs, acc, wr, wc, li, lk, 0);
  }

  __syncthreads();
  double* xi = smem;
  double* xj = smem + T * XP;
  double* bs = smem + 2 * T * XP;
  const int d = a.d, m = a.m;
  for (int e = tid; e < T * D; e += 256) {
    const int p = e / D, k = e - p * D;
    const bool ki = k < d && I0 + p < m, kj = k < d && J0 + p < m;
    xi[p * XP + k] = ki ? a.Xs[(long long)(I0 + p) * a.ldxs + k] : 0.0;
    xj[p * XP + k] = kj ? a.Xs[(long long)(J0 + p) * a.ldxs + k] : 0.0;
  }
  if (tid < D) bs[tid] = tid < d ? a.beta[(long long)b * a.ldbeta + tid] : 0.0;
  __syncthreads();

  const double sb = a.s[b];
  const double diag = a.s_pred[b] + (a.jitter ? a.jitter[b] : 0.0);
  double* Cb = a.C + b * a.sC;
#pragma unroll
  for (int mi = 0; mi < NT; ++mi)
#pragma unroll
    for (int nj = 0; nj < NT; ++nj) {
      // (tile pairs wholly above the diagonal of a diagonal block, or past m: nothing to write)
      if (I0 + (wr * NT + mi) * 16 + 15 < J0 + (wc * NT + nj) * 16) continue;
      if (I0 + (wr * NT + mi) * 16 >= m) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int pi = (wr * NT + mi) * 16 + lk + 4 * r, pj = (wc * NT + nj) * 16 + li;
        const int i = I0 + pi, j = J0 + pj;
        double dist;
        if constexpr (D <= 8) {
          dist = ard_dist<D>(xi + pi * XP, xj + pj * XP, bs, d);
        } else {
          // a rolled loop: unrolling D steps for each of the 16 NT^2 elements would leave the
          // accumulators dynamically indexed (scratch)
          dist = 0.0;
#pragma unroll 1
          for (int k = 0; k < d; ++k) {
            const double tk = xi[pi * XP + k] - xj[pj * XP + k];
            dist = fma(bs[k] * tk, tk, dist);
          }
        }
        const double prior = (i == j) ? diag : exp_neg_scaled(dist, sb);
        const double v = prior - acc[mi][nj][r];
        if (i < m && j <= i) {
          Cb[(long long)j * a.ldc + i] = v;
          if (i != j) Cb[(long long)i * a.ldc + j] = v;
        }
      }
    }
}

// Element e of gp_realize's normal stream for (seed, offset): Philox4x32-10 at counter
// (e / 2, offset), Box-Muller, cos for even e and sin for odd e (rng.hip).
GP_DEV double stream_normal(uint64_t e, uint64_t seed, uint64_t offset) {
  const uint64_t j = e >> 1;
  uint32_t c[4] = {(uint32_t)j, (uint32_t)(j >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const double scale = 1.0 / 9007199254740992.0;   // 2^-53
  const double u1 = (double)((((uint64_t)c[0] << 32) | c[1]) >> 11) * scale;
  const double u2 = (double)((((uint64_t)c[2] << 32) | c[3]) >> 11) * scale;
  const double r = sqrt(-2.0 * log(1.0 - u1));
  double sn, cs;
  sincospi(2.0 * u2, &sn, &cs);
  return (e & 1) ? r * sn : r * cs;
}

constexpr int kDrawGroup = 8;    // draws that share one pass over R
constexpr int kDrawK = 64;       // columns of R per LDS round of normals

// out[b][r][i] = mean_b[i] + sum_{k <= i} R_b[i, k] xi_e, e = ((unit0 + b) nsamp + r) m + k.
// One thread per row i (a wave reads 512 contiguous bytes of a column of R), kDrawGroup draws per
// block so R is read once per group; the group's normals of 64 columns are generated by the
// block into LDS.  The test k <= i guards the load itself: nothing above the diagonal is read.
__global__ __launch_bounds__(256) void mvn_draw_kernel(
    const double* __restrict__ R, int ldr, long long sR, int m, const double* __restrict__ mean,
    int ldm, int nsamp, uint64_t seed, uint64_t offset, long long unit, double* __restrict__ out,
    long long ldo) {
  __shared__ double xi[kDrawK][kDrawGroup];
  const int b = blockIdx.z, r0 = blockIdx.y * kDrawGroup, tid = threadIdx.x;
  const int i = blockIdx.x * 256 + tid;
  const int kmax = min(m, (int)blockIdx.x * 256 + 256);
  const double* Rb = R + b * sR;
  const uint64_t e0 = ((uint64_t)(unit + b) * (uint64_t)nsamp + (uint64_t)r0) * (uint64_t)m;
  double acc[kDrawGroup];
#pragma unroll
  for (int g = 0; g < kDrawGroup; ++g) acc[g] = 0.0;
  for (int k0 = 0; k0 < kmax; k0 += kDrawK) {
    __syncthreads();
    for (int e = tid; e < kDrawK * kDrawGroup; e += 256) {
      const int g = e / kDrawK, kk = e - g * kDrawK, k = k0 + kk;
      xi[kk][g] = (k < m && r0 + g < nsamp)
                      ? stream_normal(e0 + (uint64_t)g * (uint64_t)m + (uint64_t)k, seed, offset)
                      : 0.0;
    }
    __syncthreads();
    if (i < m) {
      const int kk1 = min(kDrawK, i - k0 + 1);
      for (int kk = 0; kk < kk1; ++kk) {
        const double rv = Rb[(long long)(k0 + kk) * ldr + i];
#pragma unroll
        for (int g = 0; g < kDrawGroup; ++g) acc[g] = fma(rv, xi[kk][g], acc[g]);
      }
    }
  }
  if (i >= m) return;
  const double mu = mean ? mean[(long long)b * ldm + i] : 0.0;
#pragma unroll
  for (int g = 0; g < kDrawGroup; ++g)
    if (r0 + g < nsamp) out[((long long)b * nsamp + r0 + g) * ldo + i] = mu + acc[g];
}

// tile edge for m test points, and the padded extents of the k-major images
int tile_edge(int m) { return m > 64 ? 128 : 64; }
int pad_cols(int m) { return gp_ceil_div(m, tile_edge(m)) * tile_edge(m); }
int pad_rows(int n, int m) { return gp_ceil_div(n, tile_edge(m)) * tile_edge(m); }

template <int NT>
hipError_t syrk_launch(const JcSyrkArgs& y, int nb, hipStream_t stream) {
  auto kern = jc_syrk_kernel<NT, 8>;
  if (y.d > 8) kern = y.d <= 16 ? jc_syrk_kernel<NT, 16> : jc_syrk_kernel<NT, 32>;
  hipLaunchKernelGGL(kern, dim3(y.nt * (y.nt + 1) / 2 * nb), dim3(256), 0, stream, y);
  return hipGetLastError();
}

}  // namespace

extern "C" long long gp_predict_cov_ws_bytes(int n, int m, int batch) {
  if (n < 0 || m < 0 || batch < 0) return -1;
  if (n == 0 || m == 0 || batch == 0) return 0;
  const long long mp = pad_cols(m);
  return align256(8LL * batch * gp_padded_n(n) * mp) + align256(8LL * batch * pad_rows(n, m) * mp);
}

extern "C" int gp_predict_cov(const double* Linv, int ldinv, long long strideInv,
                              const double* X, int ldx, const double* Xs, int ldxs, int n, int m,
                              int d, const double* beta, int ldbeta, const double* s,
                              const double* s_pred, const double* jitter, double* C, int ldc,
                              long long strideC, int batch, void* ws, long long ws_bytes,
                              hipStream_t stream) {
  const int npad = gp_padded_n(n);
  if (!Linv || (reinterpret_cast<uintptr_t>(Linv) & 15)) return -1;
  if (n > 0 && (ldinv < npad || (ldinv & 1))) return -2;
  if (n > 0 && ((batch > 1 && strideInv < (long long)ldinv * npad) || (strideInv & 1))) return -3;
  if (!X) return -4;
  if (ldx < d) return -5;
  if (!Xs) return -6;
  if (ldxs < d) return -7;
  if (n < 0) return -8;
  if (m < 0) return -9;
  if (d < 1 || d > GPFIT_MAX_DIM) return -10;
  if (!beta) return -11;
  if (ldbeta < d && batch > 1) return -12;
  if (!s) return -13;
  if (!s_pred) return -14;
  if (!C) return -16;
  if (ldc < m || ldc < 1) return -17;
  if (batch > 1 && strideC < (long long)ldc * m) return -18;
  if (batch < 0) return -19;
  if (m == 0 || batch == 0) return 0;
  const long long need = gp_predict_cov_ws_bytes(n, m, batch);
  if (need > 0) {
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255)) return -21;
    if (ws_bytes < need) return -22;
  }

  const int T = tile_edge(m), mp = pad_cols(m), nr = pad_rows(n, m), nt = mp / T;
  const long long sK = (long long)npad * mp, sV = (long long)nr * mp;
  double* Kt = static_cast<double*>(ws);
  double* V = n > 0 ? reinterpret_cast<double*>(static_cast<char*>(ws) + align256(8LL * batch * sK))
                    : nullptr;
  const long long sL = batch > 1 ? strideInv : 0, sC = batch > 1 ? strideC : 0;
  const int ldb = batch > 1 ? ldbeta : 0;

  for (int b0 = 0; b0 < batch; b0 += kMaxGridZ) {
    const int nb = min(batch - b0, kMaxGridZ);
    if (n > 0) {
      GP_CK(gpfit_cross_kp_launch(X, ldx, Xs, ldxs, n, m, d, beta + (long long)b0 * ldb, ldb,
                                  s + b0, Kt + b0 * sK, mp, sK, nb, stream));
      JcTrmmArgs t;
      t.Linv = Linv + b0 * sL;
      t.ld = ldinv;
      t.sL = sL;
      t.Kt = Kt + b0 * sK;
      t.V = V + b0 * sV;
      t.sK = sK;
      t.sV = sV;
      t.mp = mp;
      t.n = n;
      t.nrt = nr / T;
      t.nct = nt;
      hipLaunchKernelGGL(T == 128 ? jc_trmm_kernel<4> : jc_trmm_kernel<2>,
                         dim3(t.nrt * t.nct * nb), dim3(256), 0, stream, t);
      GP_CK(hipGetLastError());
    }
    JcSyrkArgs y;
    y.V = n > 0 ? V + b0 * sV : nullptr;
    y.sV = sV;
    y.Xs = Xs;
    y.ldxs = ldxs;
    y.d = d;
    y.beta = beta + (long long)b0 * ldb;
    y.ldbeta = ldb;
    y.s = s + b0;
    y.s_pred = s_pred + b0;
    y.jitter = jitter ? jitter + b0 : nullptr;
    y.C = C + b0 * sC;
    y.ldc = ldc;
    y.sC = sC;
    y.mp = mp;
    y.m = m;
    y.n = n;
    y.nt = nt;
    GP_CK(T == 128 ? syrk_launch<4>(y, nb, stream) : syrk_launch<2>(y, nb, stream));
  }
  return 0;
}

extern "C" int gp_mvn_draw(const double* R, int ldr, long long strideR, int m, const double* mean,
                           int ldm, int nsamp, unsigned long long seed,
                           unsigned long long offset, long long unit0, double* out,
                           long long ldo, int batch, hipStream_t stream) {
  if (!R) return -1;
  if (ldr < m || ldr < 1) return -2;
  if (batch > 1 && strideR < (long long)ldr * m) return -3;
  if (m < 0) return -4;
  if (mean && ldm < m && batch > 1) return -6;
  if (nsamp < 0 || nsamp > kDrawGroup * kMaxGridZ) return -7;
  if (unit0 < 0) return -10;
  if (!out) return -11;
  if (ldo < m) return -12;
  if (batch < 0) return -13;
  if (m == 0 || nsamp == 0 || batch == 0) return 0;
  const long long sR = batch > 1 ? strideR : 0;
  const int ldm_ = batch > 1 ? ldm : 0;
  const int groups = gp_ceil_div(nsamp, kDrawGroup);
  for (int b0 = 0; b0 < batch; b0 += kMaxGridZ) {
    const int nb = min(batch - b0, kMaxGridZ);
    hipLaunchKernelGGL(mvn_draw_kernel, dim3(gp_ceil_div(m, 256), groups, nb), dim3(256), 0,
                       stream, R + b0 * sR, ldr, sR, m,
                       mean ? mean + (long long)b0 * ldm_ : nullptr, ldm_, nsamp, (uint64_t)seed,
                       (uint64_t)offset, unit0 + b0, out + (long long)b0 * nsamp * ldo, ldo);
    GP_CK(hipGetLastError());
  }
  return 0;
}
