// The joint bilateral upsampler (jbu.hip): its launch plan (jb_plan), its two workgroup bodies (wg_jbu_g0, wg_jbu,
// over wg.h's group type: DESIGN 12.13) and the per-thread phases they run, written like fill_guided_tile.h so that the SAME text
// compiles for the device and for a plain host compiler: the kernels and tools/jbu_host_check.cpp, under the address and
// undefined-behaviour sanitizers, call the same bodies.  Integers only, except the estimate of the quotient, which is corrected
// in integers (jb_quot).
//
// The definition (tests/jbu_ref.py): the high-resolution pixel (Y, X) of a plane at scale S reads the bicubic's own 4 x 4
// footprint of low-resolution cells, rows y0 - 1 .. y0 + 2 with y0 = (2 Y + 1 - S) // (2 S); tap q weighs
//   w_q = max(1, (sy[Y mod S][ky] sx[X mod S][kx] + 128) >> 8) T[|g(Y, X) - G_0(q)|]      (at most 2^16)
// and 0 outside the plane or at a hole, and out = (2 sum w c + sum w) // (2 sum w), 0 where no tap is valid.
//
// Two launches, a function of the shape alone:
//   wg_jbu_g0   G_0, the S x S box means of the guidance, of one 64 x 64 tile of cells into the workspace plane (h x w, u8):
//               the guided filler's own reduction (fg_g0_tile)
//   wg_jbu      one JB_TW x JB_TH tile of high-resolution pixels: the codes (u16) and G_0 (u8) of the tile's footprint,
//               (JB_TH / S + 4) x (JB_TW / S + 4) cells -- a cell outside the plane a hole -- and the two tables into LDS; then
//               every thread one run of JB_RUN = 16 adjacent pixels of one row: its 4 x (16 / S + 4) window of cells from LDS
//               into registers, 16 bytes of guidance in one load where the address allows (else bytes), the 16 quotients, and
//               stores of four pixels (4 or 8 bytes).
#pragma once

#include <type_traits>

#include "fill_guided_tile.h"

namespace codon {

constexpr int JB_TW = 128, JB_TH = 32, JB_RUN = 16;
constexpr int JB_THREADS = (JB_TW / JB_RUN) * JB_TH;                 // 256: eight runs across, thirty-two rows
static_assert(JB_THREADS == FL_THREADS, "the G_0 body runs with the filler's workgroup");

template <int S>
struct JbShape {
  static constexpr int ROWS = JB_TH / S + 4, COLS = JB_TW / S + 4, CELLS = ROWS * COLS;   // x4: 12 x 36, x8: 8 x 20, x16: 6 x 12
  static constexpr int off(int j) { return (j + S / 2) / S; }        // the window column of pixel j's first tap
  static constexpr int NW = 4 + off(JB_RUN - 1);                     // 8, 6, 5
};
constexpr int JB_CELLS_MAX = JbShape<4>::CELLS;                      // 432
constexpr int JB_STAB_MAX = 16 * 4;

// The launches of B planes of h x w at scale s: the G_0 body over g0x x g0y tiles of cells per image, the upsampling body over
// gx x gy tiles of pixels; the workspace holds G_0 alone, images `stride` bytes apart
struct JbPlan {
  int g0x, g0y, gx, gy;
  long stride;
};
CODON_FL_HD JbPlan jb_plan(int h, int w, int s) {
  JbPlan p;
  p.g0x = fl_size(w, FL_LOG);
  p.g0y = fl_size(h, FL_LOG);
  p.gx = (w * s + JB_TW - 1) / JB_TW;
  p.gy = (h * s + JB_TH - 1) / JB_TH;
  p.stride = ((long)h * w + 15) / 16 * 16;
  return p;
}

// floor(num / den) for 0 < den <= 2^21 and a quotient below 2^17: the fp32 estimate is off by less than 2^17 (2^-24 + 2^-22),
// so at most one step either way sets it right; the steps are in integers
template <typename ACC>
CODON_FL_HD int jb_quot(ACC num, unsigned den) {
  typedef typename std::conditional<sizeof(ACC) == 4, int, long long>::type I;      // the u8 numerator stays below 2^30
  I q = (I)((float)num / (float)den);
  I r = (I)num - q * (I)den;
  if (r < 0) {
    --q;
    r += (I)den;
  }
  if (r < 0) --q;
  if (r >= (I)den) {
    ++q;
    r -= (I)den;
  }
  if (r >= (I)den) ++q;
  return (int)q;
}

// the footprint of tile (tx, ty) of image `in` (h x w codes) and of its G_0 plane into LDS; the tables too
template <int S, int FMT>
CODON_FL_HD void jb_tile_load(int tid, const void* in, const unsigned char* g0, int h, int w, int ty, int tx,
                              const unsigned short* rtab, const unsigned short* stab, unsigned short* lc, unsigned char* lg,
                              unsigned short* t, unsigned short* st) {
  using Sh = JbShape<S>;
  fg_tab_load(tid, rtab, t);
  if (tid < S * 4) st[tid] = stab[tid];
  const int cy0 = ty * (JB_TH / S) - 2, cx0 = tx * (JB_TW / S) - 2;
  for (int idx = tid; idx < Sh::CELLS; idx += JB_THREADS) {
    const int i = idx / Sh::COLS, j = idx - i * Sh::COLS;
    const int y = cy0 + i, x = cx0 + j;
    const bool ok = y >= 0 && y < h && x >= 0 && x < w;
    const long at = (long)(y < 0 ? 0 : y < h ? y : h - 1) * w + (x < 0 ? 0 : x < w ? x : w - 1);
    const int c = fl_load<FMT>(in, at, 0), g = g0[at];               // no branch around the loads
    lc[idx] = (unsigned short)(ok ? c : 0);
    lg[idx] = (unsigned char)(ok ? g : 0);
  }
}

// one thread's run: row `row` and run `run` of the tile; gimg the image's guidance, out its H x W plane of codes
template <int S, int FMT, typename ACC>
CODON_FL_HD void jb_run(int tid, const unsigned char* gimg, long row_bytes, int H, int W, int ty, int tx, const unsigned short* lc,
                        const unsigned char* lg, const unsigned short* t, const unsigned short* st, void* out) {
  using Sh = JbShape<S>;
  constexpr int NW = Sh::NW;
  const int row = tid / (JB_TW / JB_RUN), run = tid - row * (JB_TW / JB_RUN);
  const int Y = ty * JB_TH + row, X0 = tx * JB_TW + run * JB_RUN;
  if (Y >= H || X0 >= W) return;
  const int n = W - X0 < JB_RUN ? W - X0 : JB_RUN;                   // a multiple of 4: W is one
  unsigned gq[JB_RUN / 4];
  const unsigned char* gp = gimg + (long)Y * row_bytes + X0;
  if (n == JB_RUN && (((uintptr_t)gp) & 15) == 0) {
    fg_load16(gp, gq);
  } else {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int e = 0; e < JB_RUN / 4; ++e) {
      unsigned q = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int b = 0; b < 4; ++b) q |= (unsigned)gp[4 * e + b < n ? 4 * e + b : 0] << (8 * b);
      gq[e] = q;
    }
  }
  // the window: rows (row + S / 2) / S .. + 3 of the footprint, columns run * (16 / S) .. + NW - 1
  const int base = ((row + S / 2) / S) * Sh::COLS + run * JB_RUN / S;
  int wc[4][NW], wg[4][NW], sy[4];
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 4; ++k) {
    sy[k] = st[(Y % S) * 4 + k];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int c = 0; c < NW; ++c) {
      wc[k][c] = lc[base + k * Sh::COLS + c];
      wg[k][c] = lg[base + k * Sh::COLS + c];
    }
  }
  unsigned res[JB_RUN];
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int j = 0; j < JB_RUN; ++j) {
    const int o = Sh::off(j);
    const int g = (int)((gq[j >> 2] >> (8 * (j & 3))) & 255u);
    const unsigned short* sx = st + (j % S) * 4;                     // X0 is a multiple of 16, hence of S
    ACC num = 0;
    unsigned den = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int ky = 0; ky < 4; ++ky) {
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int kx = 0; kx < 4; ++kx) {
        const int c = wc[ky][o + kx], d = g - wg[ky][o + kx];
        const unsigned sp = ((unsigned)sy[ky] * sx[kx] + 128u) >> 8;
        const unsigned tv = t[d < 0 ? -d : d];                       // read for a hole too: no branch around the sixteen reads
        const unsigned wq = (c ? (sp ? sp : 1u) : 0u) * tv;
        num += (ACC)(wq * (unsigned)c);                              // at most 2^16 * 65535: 32 bits
        den += wq;
      }
    }
    res[j] = den ? (unsigned)jb_quot<ACC>((ACC)(2 * num + den), 2u * den) : 0u;
  }
  // stores of four pixels, 4 bytes (u8) or 8 (u16): the plane is 16-byte aligned and X0, W and n are multiples of 4
  unsigned char* op = (unsigned char*)out + ((long)Y * W + X0) * fl_elem_bytes(FMT);
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int e = 0; e < JB_RUN / 4; ++e) {
    if (4 * e >= n) continue;
    if (FMT == FL_U8) {
      const unsigned q = res[4 * e] | (res[4 * e + 1] << 8) | (res[4 * e + 2] << 16) | (res[4 * e + 3] << 24);
      memcpy(__builtin_assume_aligned(op + 4 * e, 4), &q, 4);
    } else {
      const unsigned q[2] = {res[4 * e] | (res[4 * e + 1] << 16), res[4 * e + 2] | (res[4 * e + 3] << 16)};
      memcpy(__builtin_assume_aligned(op + 8 * e, 8), q, 8);
    }
  }
}

// ---- the workgroup bodies -------------------------------------------------------------------------------------------------------

// workgroup (tx, ty, b) of grid (g0x, g0y, B): G_0 of one 64 x 64 tile of cells to the workspace.  g: FL_TILE * FL_TILE bytes of LDS
template <class G>
CODON_FL_HD void wg_jbu_g0(G wg, int tx, int ty, long b, const unsigned char* guide, long row_bytes, long image_bytes, int scale,
                           int h, int w, unsigned char* ws, long ws_stride, unsigned char* g) {
  wg_fillg_g0(wg, scale, guide + b * image_bytes, row_bytes, h, w, ty * FL_TILE, tx * FL_TILE, g, (unsigned char*)nullptr,
              ws + b * ws_stride);
}

// workgroup (tx, ty, b) of grid (gx, gy, B): one tile of high-resolution pixels.  LDS: lc JbShape<S>::CELLS u16, lg as many u8,
// t FG_TAB u16, st S * 4 u16
template <int S, int FMT, class G>
CODON_FL_HD void wg_jbu(G wg, int tx, int ty, long b, const void* in, int h, int w, const unsigned char* guide, long row_bytes,
                        long image_bytes, const unsigned short* rtab, const unsigned short* stab, const unsigned char* ws,
                        long ws_stride, void* out, unsigned short* lc, unsigned char* lg, unsigned short* t, unsigned short* st) {
  typedef typename std::conditional<FMT == FL_U8, unsigned, unsigned long long>::type ACC;
  const long plane = (long)h * w * fl_elem_bytes(FMT);
  WG_EACH(wg, tid)
    jb_tile_load<S, FMT>(tid, (const char*)in + b * plane, ws + b * ws_stride, h, w, ty, tx, rtab, stab, lc, lg, t, st);
  wg.sync();
  WG_EACH(wg, tid)
    jb_run<S, FMT, ACC>(tid, guide + b * image_bytes, row_bytes, h * S, w * S, ty, tx, lc, lg, t, st,
                        (char*)out + b * plane * S * S);
}

}  // namespace codon
