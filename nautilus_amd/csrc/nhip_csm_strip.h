// nhip_csm_strip.h -- K2 + K3, every add: the skeleton of the strip kernels, once for both cell widths.
//
// Replaces CorrelativeScanMatcher::GetTransformation (call site src/optimization/solver.cc:633-638), batched over
// candidate pairs.
//
// Formulation (accumulator-stationary, LDS-tiled): a wave owns one 21-row strip of the (nx x ny) score plane of one
// rotation k of one pair and keeps its integer accumulators in registers -- three lanes per y-shift, 28 consecutive
// x-shifts each.  A point's contribution to the strip is the (81 x 21) window of the target grid anchored at its rotated
// cell.  Per lane-chunk of 64 points the wave computes the rotated cells (one point per lane) and looks up the target's
// skip map (nhip_grid_tables.hip): points whose window strip holds only zeros are dropped -- they would add nothing, so the sums
// are unchanged.  The others are visited in beam order; consecutive beams hit neighbouring cells, so a run of points
// shares one grid tile: the workgroup stages a tile of the grid in LDS (16-byte reads of HBM/L2, once per run), then
// every point of the run is a wave-uniform LDS offset (v_readlane) from which each lane reads its 28 cells as seven
// aligned words and accumulates them.  LDS pitch 53 words makes the 32-lane read groups conflict-free (bank = 7 * lane
// mod 32).  All arithmetic is integer: sums are order-independent, hence bit-exact against the oracle.
//
// No bounds checks: grids carry a zero border of pad = 2*max_shift+16 cells and rotated cells are clamped to one cell
// outside the window-overlap range (a clamped point only sees border).
//
// What a cell width changes is its policy class (Cells8 of nhip_csm.hip, Cells16 of nhip_csm16.hip):
//   CB                      bytes per cell; the tile's geometry follows from it (Strip<C> below)
//   WG_WAVES, TILE_ROWS, FILL_INFLIGHT, WAVES_PER_SIMD
//                           strips (waves) that share one tile, the tile's rows, 16-byte tile-fill loads a lane keeps in
//                           flight, the launch bound
//   Word                    the tile's element: the unit of the aligned LDS reads (4 * CB bytes)
//   Acc, clear / segment / finish
//                           a lane's accumulators; the grouped add of a run segment's points from the tile; the lane's 28
//                           sums from the accumulators (named as references to the unit's functions: through a wrapper
//                           the kernels compile to other code)
//   UNPACKS, FLUSH_START_MAX
//                           whether the accumulators' fields overflow: finish then adds into the sums and clears the
//                           accumulators whenever an alignment class has had more than FLUSH_START_MAX points, and not
//                           only once at the end
//   tile_base               what segment takes as the tile (a pointer, an LDS address)
//   store_head / store_tail a 16-byte chunk of a grid row into the tile: its first word, the others
// The skip map's bit and a window's byte column follow from CB and are in the body.
//
// The skeleton itself is nhip_csm_strip_body.h, text that the two __global__ templates include (see there for why it is
// no function): each kernel declares its static LDS tile, names its policy C and includes the body.
#pragma once
#include "nhip_csm_shared.h"

namespace nhip {
namespace csm {

constexpr int SEGS = 3;                     // lanes per plane row: 84 aligned cells >= 81 + 3
constexpr int SEG_COLS = 28;                // x-shifts per lane: seven aligned words of four cells
constexpr int WAVE_ROWS = 63 / SEGS;        // 21 plane rows per wave (lane 63 idles: rows never straddle waves)
constexpr int PB_NX = SEGS * SEG_COLS - 3;  // 81 x-shifts per plane block (84 cells minus alignment slack)
constexpr int LP_W = 53;                    // LDS tile pitch in words (conflict-free: 53 = 21 mod 32)

template <class C>
struct Strip {
  static constexpr int THREADS = 64 * C::WG_WAVES;
  static constexpr int PB_NY = C::WG_WAVES * WAVE_ROWS;          // y-shifts per plane block (21 per wave)
  static constexpr int LP = LP_W * 4 * C::CB;                    // tile pitch in bytes (212, 424)
  static constexpr int ROW_BYTES = SEGS * SEG_COLS * C::CB;      // bytes of a tile row one point touches from its aligned start
  static constexpr int COL_SPAN = LP - ROW_BYTES;                // max byte offset (CB * pcol - tile_col0) of a covered point
  static constexpr int ROW_CH = (LP + 15) / 16;                  // 16-byte chunks per tile row (14, 27); the last holds one word
  static constexpr int FILL_ROWS = 64 / ROW_CH;                  // tile rows a wave fills per step (4, 2)
  static constexpr int STEP_ROWS = FILL_ROWS * C::WG_WAVES;      // rows one step of the whole workgroup covers
  static constexpr int CHUNK_W = 16 / (int)sizeof(typename C::Word);
  static_assert(sizeof(typename C::Word) == 4 * C::CB, "an aligned read is four cells");
  static_assert(WAVE_ROWS == CSM_WAVE_ROWS && ROW_BYTES == 4 * C::CB * CSM_ROW_DW,
                "the skip map (nhip_grid_tables.hip) is built for this wave footprint");
  static_assert(C::TILE_ROWS % STEP_ROWS == 0, "tile rows must be a whole number of fill steps");
};

}  // namespace csm
}  // namespace nhip
