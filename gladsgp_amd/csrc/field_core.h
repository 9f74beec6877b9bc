// What field.hip (gp_field) and summary.hip (gp_field_summary, gp_field_score) have in common
// outside their kernels' tile loops: the geometry, and the host's choice of instantiation and
// grid.
//
// Geometry: block = 4 waves; every wave owns 32 consecutive output columns (two 16-column MFMA
// tiles), the block 128.  A wave keeps its K panel (P x 32 doubles, the B operands of all its
// k-steps: 64 VGPRs at P = 64) in registers while the block stays on the panel; row tiles of w
// stream through double-buffered LDS (the next tile's global loads in flight under the current
// tile's MFMAs).  Per tile and wave: 1-2 row sub-tiles x 2 column tiles x ceil(P/4) k-steps of
// v_mfma_f64_16x16x4_f64.
//
// The tile loop's four steps (K-panel load, tile load, LDS store, MFMA chain) are not here: they
// stay written out in both kernels for code generation (see the note in field_kernel).
#pragma once
#include "gpfit_common.h"

namespace field_core {

constexpr int kWaves = 4;                    // waves per block
constexpr int kJT = 2;                       // 16-column MFMA tiles per wave
constexpr int kThreads = 64 * kWaves;
constexpr int kWaveCols = 16 * kJT;
constexpr int kCols = kWaves * kWaveCols;    // output columns per block
constexpr int kPitch = 68;                   // LDS row pitch of a w tile (doubles)
constexpr int kMaxP = 64;

// KS = k-steps of 4 (P <= 4 KS) everywhere below.
// rows of w per tile: 32 (two 16-row MFMA sub-tiles), 16 at P > 32 where the K panel leaves no
// room for the second sub-tile's accumulators and staging
template <int KS> constexpr int tile_rows() { return KS <= 8 ? 32 : 16; }
// elements of a tile (tile_rows x 4 KS, the inner dimension padded) per thread
template <int KS> constexpr int tile_loads() {
  return (tile_rows<KS>() * 4 * KS + kThreads - 1) / kThreads;
}

// ---- host ---------------------------------------------------------------------------------------

// f(std::integral_constant<int, KS>) for the instantiated KS that holds P
template <class F>
auto dispatch_ks(int P, F&& f) {
  const int ks = (P + 3) / 4;
  if (ks <= 2) return f(std::integral_constant<int, 2>{});
  if (ks <= 4) return f(std::integral_constant<int, 4>{});
  if (ks <= 8) return f(std::integral_constant<int, 8>{});
  if (ks <= 12) return f(std::integral_constant<int, 12>{});
  return f(std::integral_constant<int, 16>{});
}

// blocks of one residency round (no tail round of blocks), never more than the work units
inline long long round_blocks(int blocks_per_cu, long long units) {
  const long long blocks = (long long)gp_num_cus() * blocks_per_cu;
  return blocks < units ? blocks : units;
}

// blocks of `Kernel` that fit a CU at once (registers and LDS, from the runtime; `fallback` if
// it does not say), asked once per kernel
template <auto Kernel>
int blocks_per_cu(int fallback) {
  static const int nb = [fallback] {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, Kernel, kThreads, 0) != hipSuccess ||
        n < 1)
      n = fallback;
    return n;
  }();
  return nb;
}

}  // namespace field_core
