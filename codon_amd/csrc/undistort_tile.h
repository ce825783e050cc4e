// The undistortion of colour images (undistort.hip): its launch plan (ud_plan), the host's tile table (ud_tiles),
// its workgroup body (wg_undistort_tile, over wg.h's group type: DESIGN 12.13) and the per-pixel function it runs (ud_pixel),
// written like register_tile.h so that the SAME text compiles for the device and for a plain host compiler: the kernel and
// tools/undistort_host_check.cpp, under the address and undefined-behaviour sanitizers, call the same body.  Integers only.
//
// The definition (tests/undistort_ref.py): images are u8 (B, H, W, C) interleaved, C 1 or 3.  map: int32 (ho, wo, 2), the source
// position (U, V) of a target pixel in Q5 source pixels, or (UD_OUTSIDE, UD_OUTSIDE); weights: int16 (32, 4), the Catmull-Rom taps
// -1 .. 2 of the 32 phases in Q11, every row summing to 2048.  A pixel that is not outside: xi = U >> 5, px = U & 31, yi, py
// likewise; tap (r, c) = src[clamp(yi - 1 + r)][clamp(xi - 1 + c)]; row_r = sum_c K[px][c] tap, acc = sum_r K[py][r] row_r,
// out = clamp((acc + 2^21) >> 22, 0, 255) per channel: with sum |K[p]| <= 2560 every intermediate is below 255 2560^2 + 2^21 < 2^31.
// An outside pixel is 0.
//
// One launch, a function of the sizes alone: workgroup (tx, ty, b) of grid (ud_plan, B) is one UD_TW x UD_TH tile of target pixels
// of image b, one pixel per thread.  tiles: int32 (ty, tx, 4) = kind, x0, y0, 0, made on the host by ud_tiles from the host's copy
// of the map; the kind is uniform over the workgroup:
//   UD_EMPTY    no pixel of the tile is inside: zeros
//   UD_STAGED   the box of every tap of the tile's inside pixels fits UD_WW x UD_WH cells from (y0, x0): the window goes to LDS
//               with the clamp applied while staging, one word a cell (the grey byte, or RGBX: a tap is one 4-byte LDS read
//               either way; a byte a cell for grey measured 2.3 times slower), one barrier, and the tap loop
//               indexes the window without a clamp
//   UD_DIRECT   everything else: the taps come from global memory, clamped one by one
// CODON_UD_STAGE=0 compiles the staging out of ud_tiles (every tile that is not empty is UD_DIRECT): the build DESIGN 12.16 times
// the window against.
#pragma once

#include "fill_tile.h"

#ifndef CODON_UD_STAGE
#define CODON_UD_STAGE 1
#endif

namespace codon {

constexpr int UD_TW = 32, UD_TH = 8, UD_THREADS = UD_TW * UD_TH;    // 256: one target pixel per thread
constexpr int UD_WW = 48, UD_WH = 24, UD_WIN = UD_WW * UD_WH;       // the staged window: 1152 cells
constexpr int UD_WEIGHTS = 32 * 4;
constexpr int UD_EMPTY = 0, UD_STAGED = 1, UD_DIRECT = 2;
constexpr int UD_N_STAGED = 0, UD_N_DIRECT = 1, UD_N_EMPTY = 2, UD_N_OUTSIDE = 3, UD_COUNTS = 4;
constexpr int UD_OUTSIDE = -(1 << 20);
constexpr int UD_MAX_SIDE = FL_MAX_SIDE;

// The launch of B images onto ho x wo: grid (tx, ty, B), and the tile table's (ty, tx, 4) words
struct UdPlan {
  int tx, ty;
};
CODON_FL_HD UdPlan ud_plan(int ho, int wo) {
  UdPlan p;
  p.tx = (wo + UD_TW - 1) / UD_TW;
  p.ty = (ho + UD_TH - 1) / UD_TH;
  return p;
}

struct alignas(8) UdEntry {
  int u, v;
};

// HOST: the tile table and the counts (staged, direct, empty tiles, outside pixels) of a map.  Returns -1, or the index of the
// first entry that is neither the outside pair nor within -16 <= U < 32 ws - 16 and -16 <= V < 32 hs - 16 -- after which nothing
// written is of use.  A table that passes cannot make a tile read past its window.
inline long ud_tiles(int hs, int ws, int ho, int wo, const int* map, int* tiles, unsigned* counts) {
  const UdPlan p = ud_plan(ho, wo);
  for (int q = 0; q < UD_COUNTS; ++q) counts[q] = 0;
  for (int ty = 0; ty < p.ty; ++ty)
    for (int tx = 0; tx < p.tx; ++tx) {
      int xlo = 0, xhi = 0, ylo = 0, yhi = 0;
      bool any = false;
      for (int i = ty * UD_TH; i < (ty + 1) * UD_TH && i < ho; ++i)
        for (int j = tx * UD_TW; j < (tx + 1) * UD_TW && j < wo; ++j) {
          const long at = (long)i * wo + j;
          const int U = map[2 * at], V = map[2 * at + 1];
          if (U == UD_OUTSIDE && V == UD_OUTSIDE) {
            ++counts[UD_N_OUTSIDE];
            continue;
          }
          if (U < -16 || U >= 32 * ws - 16 || V < -16 || V >= 32 * hs - 16) return at;
          const int xi = U >> 5, yi = V >> 5;
          xlo = !any || xi < xlo ? xi : xlo;
          xhi = !any || xi > xhi ? xi : xhi;
          ylo = !any || yi < ylo ? yi : ylo;
          yhi = !any || yi > yhi ? yi : yhi;
          any = true;
        }
      int* t = tiles + ((long)ty * p.tx + tx) * 4;
      t[0] = UD_DIRECT, t[1] = t[2] = t[3] = 0;
      if (!any) {
        t[0] = UD_EMPTY;
        ++counts[UD_N_EMPTY];
      } else if (CODON_UD_STAGE && xhi + 2 - (xlo - 1) + 1 <= UD_WW && yhi + 2 - (ylo - 1) + 1 <= UD_WH) {
        t[0] = UD_STAGED, t[1] = xlo - 1, t[2] = ylo - 1;
        ++counts[UD_N_STAGED];
      } else {
        ++counts[UD_N_DIRECT];
      }
    }
  return -1;
}

// a cell of the window and a fetched tap are one word: the byte for grey, R | G << 8 | B << 16 for RGB

CODON_FL_HD int ud_clamp(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// the pixel (y, x) of an image, both clamped to it; bytes: right for any base and any row length
template <int C>
CODON_FL_HD unsigned ud_texel(const unsigned char* src, int hs, int ws, int y, int x) {
  const unsigned char* p = src + ((long)ud_clamp(y, hs - 1) * ws + ud_clamp(x, ws - 1)) * C;
  if (C == 1) return p[0];
  return (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16;
}

// the two fetches ud_pixel is called with
template <int C>
struct UdGlobal {
  const unsigned char* src;
  int hs, ws;
  CODON_FL_HD unsigned operator()(int y, int x) const { return ud_texel<C>(src, hs, ws, y, x); }
};
template <int C>
struct UdWindow {
  const unsigned* win;
  int x0, y0;
  CODON_FL_HD unsigned operator()(int y, int x) const { return win[(y - y0) * UD_WW + (x - x0)]; }
};

// one pixel that is not outside: the arithmetic of the definition, once, whatever fetches the taps
template <int C, class F>
CODON_FL_HD void ud_pixel(int U, int V, const short* lk, const F& fetch, unsigned char* o) {
  const int xi = U >> 5, yi = V >> 5;
  const short* kx = lk + (U & 31) * 4;
  const short* ky = lk + (V & 31) * 4;
  int acc[C];
  for (int ch = 0; ch < C; ++ch) acc[ch] = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int r = 0; r < 4; ++r) {
    int row[C];
    for (int ch = 0; ch < C; ++ch) row[ch] = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int c = 0; c < 4; ++c) {
      const unsigned tap = fetch(yi - 1 + r, xi - 1 + c);
      for (int ch = 0; ch < C; ++ch) row[ch] += (int)kx[c] * (int)((tap >> (8 * ch)) & 255u);
    }
    for (int ch = 0; ch < C; ++ch) acc[ch] += (int)ky[r] * row[ch];
  }
  for (int ch = 0; ch < C; ++ch) o[ch] = (unsigned char)ud_clamp((acc[ch] + (1 << 21)) >> 22, 255);
}

// ---- the workgroup body -----------------------------------------------------------------------------------------------------------

// workgroup (tx, ty, b) of grid (ud_plan, B).  LDS: lk UD_WEIGHTS shorts, win UD_WIN cells
template <int C, class G>
CODON_FL_HD void wg_undistort_tile(G wg, int tx, int ty, long b, const unsigned char* in, int hs, int ws, int ho, int wo,
                                   const int* map, const int* tiles, const short* weights, unsigned char* out, short* lk,
                                   unsigned* win) {
  const int* t = tiles + ((long)ty * ud_plan(ho, wo).tx + tx) * 4;
  const int kind = t[0], x0 = t[1], y0 = t[2];
  const unsigned char* src = in + b * hs * ws * C;
  unsigned char* dst = out + b * ho * wo * C;
  if (kind == UD_EMPTY) {
    WG_EACH(wg, tid) {
      const int i = ty * UD_TH + tid / UD_TW, j = tx * UD_TW + tid % UD_TW;
      if (i < ho && j < wo)
        for (int ch = 0; ch < C; ++ch) dst[((long)i * wo + j) * C + ch] = 0;
    }
    return;
  }
  typename G::template Regs<int, 2> uv(wg);
  WG_EACH(wg, tid) {
    const int i = ty * UD_TH + tid / UD_TW, j = tx * UD_TW + tid % UD_TW;
    UdEntry e = {UD_OUTSIDE, UD_OUTSIDE};
    if (i < ho && j < wo) e = *(const UdEntry*)(map + 2 * ((long)i * wo + j));          // one 8-byte load
    uv[tid][0] = e.u, uv[tid][1] = e.v;
    if (tid < UD_WEIGHTS) lk[tid] = weights[tid];
    if (kind == UD_STAGED)
      for (int idx = tid; idx < UD_WIN; idx += UD_THREADS) {
        const int r = idx / UD_WW, c = idx - r * UD_WW;
        win[idx] = ud_texel<C>(src, hs, ws, y0 + r, x0 + c);
      }
  }
  wg.sync();
  WG_EACH(wg, tid) {
    const int i = ty * UD_TH + tid / UD_TW, j = tx * UD_TW + tid % UD_TW;
    if (i < ho && j < wo) {
      const int U = uv[tid][0], V = uv[tid][1];
      unsigned char o[C];
      for (int ch = 0; ch < C; ++ch) o[ch] = 0;
      if (U != UD_OUTSIDE) {
        if (kind == UD_STAGED)
          ud_pixel<C>(U, V, lk, UdWindow<C>{win, x0, y0}, o);
        else
          ud_pixel<C>(U, V, lk, UdGlobal<C>{src, hs, ws}, o);
      }
      for (int ch = 0; ch < C; ++ch) dst[((long)i * wo + j) * C + ch] = o[ch];
    }
  }
}

}  // namespace codon
