// Field reconstruction (A9): SepiaEmulatorPrediction.get_y() -- y = (w K + e) sd + mu
// (time_predictions.py:79-90, assess_all_models.py:489-500) in one kernel.
//
// w (rows x P, rows = samples x test points) times the PC basis K (P x ncols, ncols = field
// nodes) is a GEMM with a short inner dimension (P <= 64 PCs) and a huge output (C5: 100k
// points x 10k nodes = 1e9 elements): the product is fp64-MFMA-bound (2 P flop per element,
// 1.28e11 flop at C5 = 1.6 ms at peak) against a 4-8 GB output write (0.5-1.0 ms at 8 TB/s).
// The generic path wrote the fp64 product (8 B per element), re-read it for the back-transform
// and again for the float32 narrowing -- ~4.5x the output's bytes.  Here the back-transform
// (fma(v, sd, mu), the same operation as gp_standardize's inverse), the optional error term
// (one scalar per row) and the narrowing run in the MFMA epilogue: every output element is
// written once, in its final dtype.
//
// Layout (field_core.h, shared with summary.hip): block = 4 waves; every wave owns 32
// consecutive output columns, the block 128.  A wave keeps its K panel in registers while the
// block stays on the panel; the block streams 32-row tiles of w (16 at P > 32) through LDS,
// double-buffered, so w is read once per 128 columns (from L2 / MALL: w is 51 MB at C5).
//
// Bits: every element is the k-ordered MFMA chain over k = 0, 4, 8, ... (k >= P contributes
// exact zeros), then v + e, then fma(v, sd, mu) -- the sums gp_dgemm's 64x64-tile kernel forms
// for K <= 64 (one accumulator, k in order, no split) followed by gp_standardize's inverse, so
// the fused path equals the generic one bit for bit (tests/test_gpu_emulator.py).
#include "field_core.h"
#include "../../include/gpfit.h"

namespace {

using namespace field_core;

// waves per SIMD asked of the register allocator, and the blocks per CU the grid is sized by:
// 3 blocks of 32-column wave panels against 2 of 64-column ones, 3.02 vs 3.13 ms at C5
// (profiles/r06/r06i_field_ab.log)
constexpr int kFieldOcc = 3;
typedef float f32x4_t __attribute__((ext_vector_type(4)));

// KS = k-steps of 4 (P <= 4 KS), F32 = narrow the output to float32.  Work units are (column
// panel, row tile) pairs, panel-major; block i takes units [i U / B, (i + 1) U / B) of the
// U = npanels x ntiles (one residency round of B blocks: no tail round), reloading its K panel
// when its range crosses into the next panel.
//
// Every store is non-temporal (the field is written once and not re-read by this kernel): 3.26
// vs 3.78 ms at C5 (profiles/r06/r06c_field_ab.log), same bits.
template <int KS, bool F32>
__global__ __launch_bounds__(kThreads, kFieldOcc) void field_kernel(const double* __restrict__ W,
                                                       long long ldw, int rows, int P,
                                                       const double* __restrict__ K,
                                                       long long ldk, int ncols,
                                                       const double* __restrict__ sd,
                                                       const double* __restrict__ mu,
                                                       const double* __restrict__ err,
                                                       void* __restrict__ Y, long long ldy,
                                                       long long ntiles, bool vec16) {
  constexpr int kRows = tile_rows<KS>(), RS = kRows / 16;
  __shared__ double ws[2][kRows * kPitch];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const long long npanels = (ncols + kCols - 1) / kCols;
  const long long units = npanels * ntiles;
  const long long u0 = units * blockIdx.x / gridDim.x;
  const long long u1 = units * (blockIdx.x + 1) / gridDim.x;
  if (u0 >= u1) return;                                  // block-uniform

  // The K-panel load, the tile load / store and the MFMA chain below are written out here and in
  // summary.hip, not shared through field_core.h: every shared form tried (free functions, a
  // struct of references) kept registers, LDS and occupancy but moved some kernel of the two
  // files 0.4-1.4 % outside the parent's timing spread.  That the two files form
  // the same elements is tested (tests/test_gpu_summary.py::test_one_sample_is_the_field).
  constexpr int KP = 4 * KS, NLD = tile_loads<KS>();      // padded inner dimension
  double b[KS][kJT];
  long long cur = -1;                                    // the panel held in b
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

  // w tile t -> registers: element e = tid + 256 q is (row e / KP, k e % KP)
  double pre[NLD];
  auto load_tile = [&](long long t) {
    const long long r0 = t * kRows;
#pragma unroll
    for (int q = 0; q < NLD; ++q) {
      const int e = threadIdx.x + kThreads * q;
      const int r = e / KP, k = e % KP;
      pre[q] = (e < kRows * KP && k < P && r0 + r < rows) ? W[(r0 + r) * ldw + k] : 0.0;
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int q = 0; q < NLD; ++q) {
      const int e = threadIdx.x + kThreads * q;
      if (e < kRows * KP) ws[buf][(e / KP) * kPitch + e % KP] = pre[q];
    }
  };

  long long panel = u0 / ntiles, t = u0 - panel * ntiles;  // unit u = panel * ntiles + t
  load_tile(t);
  store_tile(0);
  __syncthreads();
  int buf = 0;
  for (long long u = u0; u < u1; ++u) {
    if (panel != cur) load_panel(panel);
    const bool more = u + 1 < u1;
    const long long tn = t + 1 == ntiles ? 0 : t + 1;
    if (more) load_tile(tn);                             // in flight under the MFMAs
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
    // epilogue: row 16 rs + lk + 4 q, column 16 jt + li of the tile
    const long long r0 = t * kRows;
    const int c0 = (int)panel * kCols + wv * kWaveCols;
    // the back-transform's sd / mu of the lane's 2 columns: read per tile (L1 hits), not held
    // in 8 more registers across the loop beside the K panel (64 at P = 64)
    double s_c[kJT], m_c[kJT];
#pragma unroll
    for (int jt = 0; jt < kJT; ++jt) {
      const int c = c0 + 16 * jt + li;
      const bool ok = sd != nullptr && c < ncols;
      s_c[jt] = ok ? sd[c] : 1.0;
      m_c[jt] = ok ? mu[c] : 0.0;
    }
    if constexpr (F32) {
      // float32: the wave's kRows x kWaveCols tile into its LDS slice, then back as 16-B row
      // pieces, 8 lanes per 128-B row segment: a wave's row segments are written by one
      // instruction each instead of 4 B per lane from the MFMA C layout (2.763 vs 3.030 ms at
      // C5, profiles/r06/r06ap_field_st16_ab.log)
      constexpr int kYP = kWaveCols + 4;                 // staged row pitch (floats, 16-B rows)
      __shared__ __attribute__((aligned(16))) float ys[kWaves * kRows * kYP];
      float* yw = ys + wv * (kRows * kYP);
#pragma unroll
      for (int rs = 0; rs < RS; ++rs)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int rr = 16 * rs + lk + 4 * q;
          const long long r = r0 + rr;
          const double e = (err && r < rows) ? err[r] : 0.0;
#pragma unroll
          for (int jt = 0; jt < kJT; ++jt) {
            double v = acc[rs][jt][q];
            if (err) v = v + e;
            if (sd) v = fma(v, s_c[jt], m_c[jt]);
            yw[rr * kYP + 16 * jt + li] = static_cast<float>(v);
          }
        }
      constexpr int kPieces = kWaveCols / 4;             // 16-B pieces per row
#pragma unroll
      for (int h = 0; h < kRows * kPieces / 64; ++h) {
        const int idx = lane + 64 * h, rr = idx / kPieces, cc = 4 * (idx % kPieces);
        const f32x4_t v4 = *reinterpret_cast<const f32x4_t*>(yw + rr * kYP + cc);
        const long long r = r0 + rr;
        const int c = c0 + cc;
        if (r >= rows) continue;
        float* yp = static_cast<float*>(Y) + r * ldy + c;
        if (vec16 && c + 3 < ncols) {
          __builtin_nontemporal_store(v4, reinterpret_cast<f32x4_t*>(yp));
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (c + i < ncols) __builtin_nontemporal_store(v4[i], yp + i);
        }
      }
    } else {
      // fp64: 8 B per lane straight from the MFMA C layout
#pragma unroll
      for (int rs = 0; rs < RS; ++rs)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const long long r = r0 + 16 * rs + lk + 4 * q;
          if (r >= rows) continue;
          const double e = err ? err[r] : 0.0;
#pragma unroll
          for (int jt = 0; jt < kJT; ++jt) {
            const int c = c0 + 16 * jt + li;
            if (c >= ncols) continue;
            double v = acc[rs][jt][q];
            if (err) v = v + e;
            if (sd) v = fma(v, s_c[jt], m_c[jt]);
            __builtin_nontemporal_store(v, static_cast<double*>(Y) + r * ldy + c);
          }
        }
    }
    if (more) {
      store_tile(buf ^ 1);                               // the other buffer: last read a tile ago
      __syncthreads();
      buf ^= 1;
    }
    if (tn == 0) ++panel;
    t = tn;
  }
}

struct FieldArgs {
  const double* W;
  long long ldw;
  int rows, P;
  const double* K;
  long long ldk;
  int ncols;
  const double *sd, *mu, *err;
  void* Y;
  long long ldy;
  hipStream_t stream;
};

template <int KS, bool F32>
hipError_t launch_field(const FieldArgs& a) {
  const long long ntiles = ((long long)a.rows + tile_rows<KS>() - 1) / tile_rows<KS>();
  const long long blocks = round_blocks(kFieldOcc, gp_ceil_div(a.ncols, kCols) * ntiles);
  // 16-B stores need 16-B aligned rows
  const bool vec16 = ((reinterpret_cast<uintptr_t>(a.Y) & 15) == 0) && (a.ldy % 4 == 0);
  hipLaunchKernelGGL((field_kernel<KS, F32>), dim3((unsigned)blocks), dim3(kThreads), 0, a.stream,
                     a.W, a.ldw, a.rows, a.P, a.K, a.ldk, a.ncols, a.sd, a.mu, a.err, a.Y, a.ldy,
                     ntiles, vec16);
  return hipGetLastError();
}

}  // namespace

extern "C" int gp_field_max_pcs(void) { return kMaxP; }

extern "C" int gp_field(const double* W, long long ldw, int rows, int P, const double* K,
                        long long ldk, int ncols, const double* sd, const double* mu,
                        const double* err, void* Y, long long ldy, int out_f32,
                        hipStream_t stream) {
  if (!W) return -1;
  if (ldw < P || ldw < 1) return -2;
  if (rows < 0) return -3;
  if (P < 1 || P > kMaxP) return -4;
  if (!K) return -5;
  if (ldk < ncols || ldk < 1) return -6;
  if (ncols < 0) return -7;
  if ((sd == nullptr) != (mu == nullptr)) return -8;
  if (!Y) return -11;
  if (ldy < ncols || ldy < 1) return -12;
  if (rows == 0 || ncols == 0) return 0;
  const FieldArgs a = {W, ldw, rows, P, K, ldk, ncols, sd, mu, err, Y, ldy, stream};
  const hipError_t e = dispatch_ks(P, [&](auto ks) {
    return out_f32 ? launch_field<decltype(ks)::value, true>(a)
                   : launch_field<decltype(ks)::value, false>(a);
  });
  return e == hipSuccess ? 0 : GPFIT_ERR_HIP - (int)e;
}
