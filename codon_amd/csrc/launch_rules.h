// The host launch rules of the stem / head stencils, the one-channel weight gradient and the CAC gate passes, each stated
// ONCE, with the constants their kernels share with them.  The launchers of stencil.hip, ew_c8.hip, cac.hip
// and cac_bwd.hip switch on these functions; codon_launch_form (codon_abi.hip) is the same functions called without a
// launch, which is what the tests ask (tests/forms.py).  Host arithmetic only; no launcher compares a pixel count with a
// number of its own.
#pragma once
#include "px8.h"

namespace codon {

// ---- stem and head ----------------------------------------------------------------------------------------------------
// pixels = B H W of the launch.  aligned16: what the launcher finds for its own pointers and slices.
constexpr long TINY_PIXELS = 65536;       // up to here (one 128 x 128 pair per call, BASELINE configs[0]): the one-pixel forms
constexpr long BIG_PIXELS = 1L << 22;     // from here on: the tall head bands

// fp32 stem, pixels per thread.  Images of a few thousand pixels: the four-pixel form is 16 workgroups on 256 CUs, each
// thread 64 dependent row stores long -- the one-pixel form has four times the threads.  Same fma chain per output either
// way: same bits.
inline int stem_vec_f32(long pixels, int W, bool aligned16) { return pixels > TINY_PIXELS && W % 4 == 0 && aligned16 ? 4 : 1; }

// 16-bit stem: a wave owns 64 x STEM_C8_VEC columns of one row
constexpr int STEM_C8_VEC = 2;

// fp32 head: f(HeadF32<VEC, R, DEPTH>{}) with the template arguments of head_kernel.
//   tiny (one 128 x 128 image: 32 waves of the 4-pixel form, each 16 memory round trips long): one row and 64 pixels per wave,
//   16 channels' rows in flight -- 256 waves, 4 round trips.  Same accumulation order: same bits.
//   band height R: an input row is fetched (R + 2) / R times.  Measured at 32 x 64 x 480 x 640 (tools/time_head.py, one box):
//   fp32 R = 4 / 8 / 16: 0.531 / 0.468 / 0.462 ms; bf16: 0.429 / 0.393 / 0.345 ms (round 1: 1.11 / 1.30 ms).  Small images
//   keep R = 4 (more waves).
template <int VEC, int R, int DEPTH>
struct HeadF32 { static constexpr int vec = VEC, rows = R, depth = DEPTH; };
template <typename F>
inline int head_form_f32(long pixels, int W, bool aligned16, F&& f) {
  if (pixels <= TINY_PIXELS) return f(HeadF32<1, 1, 16>{});
  const bool big = pixels >= BIG_PIXELS;
  if (W % 4 == 0 && aligned16) return big ? f(HeadF32<4, 16, 1>{}) : f(HeadF32<4, 4, 4>{});
  return big ? f(HeadF32<1, 4, 1>{}) : f(HeadF32<1, 4, 8>{});
}

// 16-bit head: rows per band; a wave owns 64 input columns = HEAD_C8_COLS output columns + one halo column each side
inline int head_rows_c8(long pixels) { return pixels >= BIG_PIXELS ? 8 : 4; }
constexpr int HEAD_C8_COLS = 62;

// ---- conv1ch_wgrad, fp32 and 16-bit: workgroup = (image, band of W1_ROWS rows), walked in chunks of W1_CHUNK pixels ------
constexpr int W1_ROWS = 8;
constexpr int W1_CHUNK = 64;
inline int w1_bands(int H) { return (H + W1_ROWS - 1) / W1_ROWS; }

// ---- CAC statistics -----------------------------------------------------------------------------------------------------
// SMALL IMAGES (one 128 x 128 pair per call, BASELINE configs[0]): 2048-pixel tiles make 8 workgroups that walk 128 planes in
// 16 dependent trips -- 57 us of a 2.9 ms forward on a chip with 256 CUs (profiles/r05_b1_fp32_128x128_timeline.txt).  Up to
// STATS_SMALL_HW pixels a tile is 256 pixels (one per thread, 64 workgroups for 128 x 128) and a trip holds 32 planes.  The
// choice depends on H * W only, never on the batch: an image's statistics do not depend on what else is in the batch.
constexpr long STATS_SMALL_HW = 32768;
constexpr int STATS_SMALL_TILE = 256;
inline bool stats_small(long HW) { return HW <= STATS_SMALL_HW; }
inline int stats_tile(long HW) { return stats_small(HW) ? STATS_SMALL_TILE : PX_TILE; }

// ---- CAC backward gate: GATE_SLICES slices of the tile range, each a contiguous share of gate_slice_tiles tiles ----------
constexpr int GATE_SLICES = 8;
__host__ __device__ inline int gate_slice_tiles(int ntiles) { return (ntiles + GATE_SLICES - 1) / GATE_SLICES; }

// ---- spatial gate: tile edge of the forward and of the backward kernel (two kernels' constants) --------------------------
constexpr int SPF_T = 32;
constexpr int SPB_T = 32;

// ---- temporal filter (temporal.hip): frames per time chunk, and the window registers of the kernel -----------
// A workgroup owns TEMPORAL_TILE pixels (temporal_tile.h's TP_TILE) through one chunk of frames and re-reads back + ahead frames
// at the chunk's seams.  One chunk is the fewest bytes; a small plane under a long sequence is then a handful of workgroups on
// 256 CUs.  So: as many chunks as bring the launch to TEMPORAL_WORKGROUPS workgroups (four of 34 KiB of LDS per CU), but no
// chunk shorter than TEMPORAL_MIN_CHUNK frames or than twice the seam (at most a third of the frames read twice).  A function of
// (T, h, w, back, ahead) alone; codon_temporal_chunk_frames is this function called without a launch.
constexpr int TEMPORAL_TILE = 1024;
constexpr int TEMPORAL_WORKGROUPS = 1024;
constexpr int TEMPORAL_MIN_CHUNK = 8;
inline int temporal_chunk_frames(int T, int h, int w, int back, int ahead) {
  const long groups = ((long)h * w + TEMPORAL_TILE - 1) / TEMPORAL_TILE;
  const long want = (TEMPORAL_WORKGROUPS + groups - 1) / groups;
  const long even = (T + want - 1) / want;
  const long least = 2 * (back + ahead) > TEMPORAL_MIN_CHUNK ? 2 * (back + ahead) : TEMPORAL_MIN_CHUNK;
  const long len = even > least ? even : least;
  return (int)(len < T ? len : T);
}
// the window registers: the smallest of 3, 5, 9, 15 that holds back + ahead + 1 frames
inline int temporal_cap(int back, int ahead) {
  const int n = back + ahead + 1;
  return n <= 3 ? 3 : n <= 5 ? 5 : n <= 9 ? 9 : 15;
}
// ---- temporal stream (temporal_push.hip): a step is one workgroup (the counters, the statistics row to 0) and
// then one workgroup per TEMPORAL_TILE pixels of the plane -- a function of (h, w) alone, the same for a push and a flush, for
// every frame index and with or without statistics.  The window registers are temporal_cap's.
inline long temporal_push_groups(int h, int w) { return ((long)h * w + TEMPORAL_TILE - 1) / TEMPORAL_TILE; }

// ---- spatial smoothing (smooth.hip): tile, passes fused per launch, launches -- one rule of (R, P) --------------
// A workgroup owns a SMOOTH_TILE x SMOOTH_TILE tile.  A launch that runs k passes loads the tile plus a halo of R k and computes
// pass j on the tile plus a halo of R (k - j): (T + 2 R (k - j))^2 / T^2 times the work of a launch of its own, against one launch,
// one read and one write of the plane saved per fused pass.  smooth_fuse_bound(R) is the largest k at which that pays, MEASURED
// (tools/time_smooth.py; DESIGN 12.25 holds the numbers); a call of P passes is ceil(P / min(P, bound)) launches of the one kernel,
// the first ones of the full bound.  codon_smooth_plan is these functions called without a launch.
// CODON_SMOOTH_FUSE_ALL: every pass of a call in one launch, whatever R -- the other side of that measurement, never the default.
constexpr int SMOOTH_TILE = 32;
constexpr int SMOOTH_MAX_RADIUS = 4, SMOOTH_MAX_PASSES = 3;
inline int smooth_fuse_bound(int radius) {
#ifdef CODON_SMOOTH_FUSE_ALL
  return SMOOTH_MAX_PASSES;
#else
  return radius == 1 ? SMOOTH_MAX_PASSES : 1;
#endif
}
inline int smooth_fused(int radius, int passes) { return passes < smooth_fuse_bound(radius) ? passes : smooth_fuse_bound(radius); }
inline int smooth_launches(int radius, int passes) { return (passes + smooth_fused(radius, passes) - 1) / smooth_fused(radius, passes); }

}  // namespace codon
