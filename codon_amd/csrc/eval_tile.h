// The workgroup body of the depth evaluation kernel (eval.hip; wg_eval_tile, over wg.h's group type: DESIGN 12.13)
// and the per-thread phases it runs, written so that the SAME text compiles for the device and for a plain host compiler: the
// kernel and tools/eval_host_check.cpp, under the address and undefined-behaviour sanitizers, call the same body.  Integers
// only.  A workgroup of EV_THREADS threads owns one EV_TILE x EV_TILE tile of one image's (H, W) output window and runs four
// phases with a workgroup barrier between them:
//   1 load    the label tile plus a halo of h = r + 1 codes (edge evaluation off: h = 0, no neighbour is read) into `lab`;
//             a position outside the H x W window is stored as code 0 -- a hole is never a neighbour and never a discontinuity,
//             which is exactly the rule "a valid 4-neighbour INSIDE the window" -- and the label beyond the window is not read
//   2 flags   over tile + r:  flag = valid and some valid 4-neighbour differs by more than T   (sensor_pixel.h's edge rule)
//   3 row OR  over (tile + r rows) x (tile columns):  rowor[y][x] = OR of flag[y][x .. x + 2r]
//   4 pixel   near = OR of rowor[y .. y + 2r][x]  (the two ORs are the (2r+1)^2 Chebyshev dilation, separably), then the
//             pixel's error, counts and maps, accumulated into the THREAD's sixteen words
// LDS coordinates: lab[ly][lx] is window position (i0 - h + ly, j0 - h + lx); flag[fy][fx] is (i0 - r + fy, j0 - r + fx),
// i.e. lab[fy + 1][fx + 1]; rowor[fy][x] is (i0 - r + fy, j0 + x).
#pragma once

#include "wg.h"

#if defined(__HIPCC__)
#define CODON_EV_HD __host__ __device__ __forceinline__
#else
#define CODON_EV_HD inline
#endif

namespace codon {

constexpr int EV_TILE = 32;
constexpr int EV_THREADS = 256;
constexpr int EV_RMAX = 8;                                   // largest dilation radius
constexpr int EV_SIDE = EV_TILE + 2 * (EV_RMAX + 1);         // 50: label tile + halo
constexpr int EV_FSIDE = EV_TILE + 2 * EV_RMAX;              // 48: flags
constexpr int EV_WORDS = 16;
constexpr int EV_MAX_THRESHOLDS = 4;

struct EvalArgs {
  int H, W;                       // the output's size = the evaluation window
  long label_row, label_image;    // the label's row stride and image stride, in elements
  int nthr;                       // thresholds in use (0..4)
  int thr[EV_MAX_THRESHOLDS];     // bad-pixel thresholds, codes
  int edge;                       // 0: edge evaluation off
  int edge_thr;                   // T, codes
  int r;                          // dilation radius, 0..EV_RMAX
};

CODON_EV_HD int ev_halo(const EvalArgs& a) { return a.edge ? a.r + 1 : 0; }
CODON_EV_HD int ev_tiles(int n) { return (n + EV_TILE - 1) / EV_TILE; }      // the grid is (ev_tiles(W), ev_tiles(H), B)

// phase 1
template <typename T>
CODON_EV_HD void ev_load(const EvalArgs& a, int tid, int i0, int j0, const T* label, T (*lab)[EV_SIDE]) {
  const int h = ev_halo(a), side = EV_TILE + 2 * h;
  for (int idx = tid; idx < side * side; idx += EV_THREADS) {
    const int ly = idx / side, lx = idx - ly * side;
    const int y = i0 - h + ly, x = j0 - h + lx;
    T v = 0;
    if (y >= 0 && y < a.H && x >= 0 && x < a.W) v = label[(long)y * a.label_row + x];
    lab[ly][lx] = v;
  }
}

// phase 2 (edge evaluation on only)
template <typename T>
CODON_EV_HD void ev_flags(const EvalArgs& a, int tid, const T (*lab)[EV_SIDE], unsigned char (*flag)[EV_FSIDE]) {
  const int side = EV_TILE + 2 * a.r;
  for (int idx = tid; idx < side * side; idx += EV_THREADS) {
    const int fy = idx / side, fx = idx - fy * side;
    const int v = lab[fy + 1][fx + 1];
    int f = 0;
    if (v != 0) {
      const int n[4] = {lab[fy][fx + 1], lab[fy + 2][fx + 1], lab[fy + 1][fx], lab[fy + 1][fx + 2]};
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int k = 0; k < 4; ++k) {
        const int d = v > n[k] ? v - n[k] : n[k] - v;
        f |= (n[k] != 0 && d > a.edge_thr) ? 1 : 0;
      }
    }
    flag[fy][fx] = (unsigned char)f;
  }
}

// phase 3 (edge evaluation on only)
CODON_EV_HD void ev_row_or(const EvalArgs& a, int tid, const unsigned char (*flag)[EV_FSIDE], unsigned char (*rowor)[EV_TILE]) {
  const int rows = EV_TILE + 2 * a.r;
  for (int idx = tid; idx < rows * EV_TILE; idx += EV_THREADS) {
    const int fy = idx / EV_TILE, x = idx - fy * EV_TILE;
    int f = 0;
    for (int d = 0; d <= 2 * a.r; ++d) f |= flag[fy][x + d];
    rowor[fy][x] = (unsigned char)f;
  }
}

// phase 4: the thread's pixels of the tile, w[] += this thread's share of the sixteen words (w[3] is a maximum).
// out / err / region: this image's (H, W) planes; err and region may be null.
template <typename T>
CODON_EV_HD void ev_pixels(const EvalArgs& a, int tid, int i0, int j0, const T (*lab)[EV_SIDE],
                           const unsigned char (*rowor)[EV_TILE], const T* out, T* err, unsigned char* region,
                           unsigned long long* w) {
  const int h = ev_halo(a);
  const int tx = tid % EV_TILE, ty = tid / EV_TILE;
  const int x = j0 + tx;
  for (int yy = ty; yy < EV_TILE; yy += EV_THREADS / EV_TILE) {
    const int y = i0 + yy;
    if (y >= a.H || x >= a.W) continue;
    const long at = (long)y * a.W + x;
    const int l = lab[yy + h][tx + h];
    int e = 0, reg = 0;
    if (l != 0) {
      const int o = out[at];
      e = l > o ? l - o : o - l;
      const int mx = l > o ? l : o, mn = l > o ? o : l;
      const unsigned long long e64 = (unsigned long long)e;
      w[0] += 1;
      w[1] += e64;
      w[2] += e64 * e64;
      w[3] = e64 > w[3] ? e64 : w[3];
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int k = 0; k < EV_MAX_THRESHOLDS; ++k) w[4 + k] += (k < a.nthr && e > a.thr[k]) ? 1 : 0;
      w[8] += 4 * mx < 5 * mn ? 1 : 0;            // 125 * 65535 < 2^31: int holds every product
      w[9] += 16 * mx < 25 * mn ? 1 : 0;
      w[10] += 64 * mx < 125 * mn ? 1 : 0;
      reg = 1;
      if (a.edge) {
        int near = 0;
        for (int d = 0; d <= 2 * a.r; ++d) near |= rowor[yy + d][tx];
        if (near) {
          w[11] += 1;
          w[12] += e64;
          w[13] += e64 * e64;
          reg = 2;
        }
      }
    }
    if (err) err[at] = (T)e;
    if (region) region[at] = (unsigned char)reg;
  }
}

// workgroup (bx, by, b) of grid (ev_tiles(W), ev_tiles(H), B): one tile of image b.  label / out / err / region: the batches; err
// and region may be null.  LDS: lab, flag, rowor.  w: the threads' sixteen words of this tile, for the caller to fold
template <typename T, class G>
CODON_EV_HD void wg_eval_tile(G wg, int bx, int by, int b, const EvalArgs& a, const T* label, const T* out, T* err,
                              unsigned char* region, T (*lab)[EV_SIDE], unsigned char (*flag)[EV_FSIDE],
                              unsigned char (*rowor)[EV_TILE], typename G::template Regs<unsigned long long, EV_WORDS>& w) {
  const int i0 = by * EV_TILE, j0 = bx * EV_TILE;
  const long hw = (long)a.H * a.W;
  WG_EACH(wg, tid) ev_load<T>(a, tid, i0, j0, label + b * a.label_image, lab);
  wg.sync();
  if (a.edge) {                                                    // uniform
    WG_EACH(wg, tid) ev_flags<T>(a, tid, lab, flag);
    wg.sync();
    WG_EACH(wg, tid) ev_row_or(a, tid, flag, rowor);
    wg.sync();
  }
  WG_EACH(wg, tid) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < EV_WORDS; ++k) w[tid][k] = 0;
    ev_pixels<T>(a, tid, i0, j0, lab, rowor, out + b * hw, err ? err + b * hw : nullptr, region ? region + b * hw : nullptr, w[tid]);
  }
}

}  // namespace codon
