// The pull-push hole filler (fill_holes.hip): its launch plan (fl_plan), its three workgroup bodies (wg_fill_*,
// over wg.h's group type: DESIGN 12.13) and the per-thread phases they run, written so that the SAME text compiles for the
// device and for a plain host compiler: the kernels and tools/fill_host_check.cpp, under the address and undefined-behaviour
// sanitizers, call the same bodies.  Integers only past the load: a plane of codes (0 a hole) is pulled up a pyramid of means
// over the valid children, level k+1 of size ceil(h_k / 2) x ceil(w_k / 2) up to 1 x 1, and pushed back down, a hole taking the
// 9/3/3/1 mix of the filled level above.  Levels are u16 cells, 0 a hole.
//
// A workgroup of FL_THREADS threads works on an aligned FL_TILE x FL_TILE tile of level 0 (a plane up to FL_TILE x FL_TILE is
// its own tile) and runs phases with a workgroup barrier between them.
//   tile pyramid `pyr`: level k of the tile is (FL_TILE >> k)^2 cells at fl_pyr_off(k), row stride FL_TILE >> k; a cell outside
//                       the plane is 0 -- a hole is never a child, which is the rule "children that lie inside level k"
//   fl_tile_load        level 0 of the tile from the plane
//   fl_tile_pull        level k -> k + 1 of the tile, and (ws != null) the in-plane cells out to the workspace
//   fl_tile_push        level k's holes from level k + 1       (a plane that is its own tile: the whole pyramid is in `pyr`)
//   fl_tile_store       level 0 of the tile to the output plane
// and, for a plane of more than one tile, the push of one tile with a halo of ONE cell per level (the parents of the cells
// a - 1 and b + 1 beside an even-aligned run [a, b] are a / 2 - 1 and (b + 1) / 2: halo cells one level up):
//   fl_halo_load        the halo pyramid: F at level FL_LOG of the tile's cell and its neighbours (3 x 3) and V at levels
//                       FL_LOG - 1 .. 1 over the tile's (FL_TILE >> k)^2 cells + halo, all from the workspace in one sweep
//   fl_halo_in          the thread's level-0 codes of the tile, from the input plane into registers
//   fl_halo_push        the holes of halo level k (FL_LOG - 1 .. 1) from halo level k + 1, in place
//   fl_halo_out         F at level 0 over the tile's cells, to the output plane
// Halo level k has side (FL_TILE >> k) + 2; its cell (i, j) is level-k cell (ty * (FL_TILE >> k) - 1 + i, ...); cells outside
// the plane hold 0 and are never read.
// Workspace of one image: levels 1 .. K back to back, level k as h_k x w_k cells (fl_level_offset).
#pragma once

#include <math.h>

#include "wg.h"

#if defined(__HIPCC__)
#define CODON_FL_HD __host__ __device__ __forceinline__
#else
#define CODON_FL_HD inline
#endif

namespace codon {

constexpr int FL_LOG = 6;
constexpr int FL_TILE = 1 << FL_LOG;                         // 64
constexpr int FL_THREADS = 256;
constexpr int FL_PYR_CELLS = 5464;                           // 4096 + 1024 + ... + 1 = 5461, rounded up to 8
constexpr int FL_HALO_CELLS = 9 + 16 + 36 + 100 + 324 + 1156;  // 1641: the halo pyramid of one tile, levels 6 .. 1
constexpr int FL_MAX_SIDE = 4096;
constexpr int FL_U8 = 0, FL_U16 = 1, FL_F32 = 2;             // CODON_FILL_U8 / _U16 / _F32

CODON_FL_HD int fl_size(int n, int k) { return (n + (1 << k) - 1) >> k; }                  // ceil(n / 2^k)
CODON_FL_HD int fl_top_level(int h, int w) {                                               // K: the first level of 1 x 1
  int k = 0;
  while (fl_size(h, k) > 1 || fl_size(w, k) > 1) ++k;
  return k;
}
CODON_FL_HD long fl_level_offset(int h, int w, int k) {                                    // cells of levels 1 .. k - 1
  long o = 0;
  for (int j = 1; j < k; ++j) o += (long)fl_size(h, j) * fl_size(w, j);
  return o;
}
CODON_FL_HD long fl_workspace_cells(int h, int w) { return fl_level_offset(h, w, fl_top_level(h, w) + 1); }
CODON_FL_HD int fl_pyr_off(int k) { return (16384 - (16384 >> (2 * k))) / 3; }             // 0, 4096, 5120, 5376, ...
CODON_FL_HD int fl_elem_bytes(int fmt) { return fmt == FL_U8 ? 1 : fmt == FL_U16 ? 2 : 4; }

// The launches of an h x w plane, a function of the shape alone.  single: one launch of the plane body, one workgroup per
// image.  Else three: the pull body over gx x gy tiles per image, the plane body on level 6 of the workspace (h6 x w6 u16 cells
// at cell l6 of each image, in place), the push body over the same tiles.
struct FlPlan {
  int single, gx, gy, h6, w6;
  long l6;
  long stride;                    // workspace cells (u16) per image: never 0, and images 16 bytes apart
};
CODON_FL_HD FlPlan fl_plan(int h, int w) {
  FlPlan p;
  p.single = h <= FL_TILE && w <= FL_TILE;
  p.gx = fl_size(w, FL_LOG);
  p.gy = fl_size(h, FL_LOG);
  p.h6 = p.gy;                    // a level-6 cell is a tile
  p.w6 = p.gx;
  p.l6 = fl_level_offset(h, w, FL_LOG);
  const long cells = fl_workspace_cells(h, w);
  p.stride = cells < 8 ? 8 : (cells + 7) / 8 * 8;
  return p;
}

// the code of element i.  fp32 on the code grid: rintf(v * top) is exact for v = tab[c]; a value off the grid is rounded
// onto it and clamped to top, and anything that is not positive (0.0f, a negative, a NaN) is a hole
template <int FMT>
CODON_FL_HD int fl_load(const void* p, long i, int top) {
  if (FMT == FL_U8) return ((const unsigned char*)p)[i];
  if (FMT == FL_U16) return ((const unsigned short*)p)[i];
  const float v = ((const float*)p)[i];
  if (!(v > 0.0f)) return 0;
  const float s = v * (float)top;
  return s < (float)top ? (int)rintf(s) : top;
}

template <int FMT>
CODON_FL_HD void fl_store(void* p, long i, int c, const float* tab) {
  if (FMT == FL_U8) ((unsigned char*)p)[i] = (unsigned char)c;
  else if (FMT == FL_U16) ((unsigned short*)p)[i] = (unsigned short)c;
  else ((float*)p)[i] = c ? tab[c] : 0.0f;
}

// the mean of the valid children, half rounded up; 2 * 4 * 65535 + 4 < 2^31
CODON_FL_HD int fl_pull4(int a, int b, int c, int d) {
  const int n = (a != 0) + (b != 0) + (c != 0) + (d != 0);
  return n ? (2 * (a + b + c + d) + n) / (2 * n) : 0;
}
// 16 * 65535 + 8 < 2^31
CODON_FL_HD int fl_mix(int near, int qx, int qy, int far) { return (9 * near + 3 * qx + 3 * qy + far + 8) >> 4; }
// the second parent of cell y beside py = y >> 1: the one on y's side, clamped into the level above (n_up cells)
CODON_FL_HD int fl_other(int y, int n_up) {
  const int q = (y >> 1) + ((y & 1) ? 1 : -1);
  return q < 0 ? 0 : q > n_up - 1 ? n_up - 1 : q;
}

// ---- the tile pyramid ---------------------------------------------------------------------------------------------------------

// level 0 of the tile at (y0, x0) of the h x w plane `in`
template <int FMT>
CODON_FL_HD void fl_tile_load(int tid, const void* in, int h, int w, int y0, int x0, int top, unsigned short* pyr) {
  constexpr int PER = FL_TILE * FL_TILE / FL_THREADS;            // 16: every thread issues all of its loads, then stores them
  int v[PER];
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int q = 0; q < PER; ++q) {
    const int idx = tid + q * FL_THREADS;
    const int y = y0 + (idx >> FL_LOG), x = x0 + (idx & (FL_TILE - 1));
    const int c = fl_load<FMT>(in, (long)(y < h ? y : h - 1) * w + (x < w ? x : w - 1), top);      // no branch around the load:
    v[q] = (y < h && x < w) ? c : 0;                                                               // the loads go out together
  }
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int q = 0; q < PER; ++q) pyr[tid + q * FL_THREADS] = (unsigned short)v[q];
}

// level k -> k + 1 of the tile (k = 0 .. FL_LOG - 1).  ws != null: the in-plane cells of level k + 1 also go to `ws`, this
// image's level k + 1 in the workspace (h_{k+1} x w_{k+1} cells); the tile is (ty, tx) of the h x w plane
CODON_FL_HD void fl_tile_pull(int tid, int k, unsigned short* pyr, unsigned short* ws, int h, int w, int ty, int tx) {
  const int n = FL_TILE >> (k + 1), lg = FL_LOG - (k + 1);
  const unsigned short* src = pyr + fl_pyr_off(k);
  unsigned short* dst = pyr + fl_pyr_off(k + 1);
  const int hk = fl_size(h, k + 1), wk = fl_size(w, k + 1);
  for (int idx = tid; idx < n * n; idx += FL_THREADS) {
    const int i = idx >> lg, j = idx & (n - 1);
    const unsigned short* c = src + (2 * i) * (2 * n) + 2 * j;
    const int v = fl_pull4(c[0], c[1], c[2 * n], c[2 * n + 1]);
    dst[idx] = (unsigned short)v;
    if (ws) {
      const int gy = ty * n + i, gx = tx * n + j;
      if (gy < hk && gx < wk) ws[(long)gy * wk + gx] = (unsigned short)v;
    }
  }
}

// level k's holes from level k + 1 (k = K - 1 .. 0, K <= FL_LOG): the plane h x w is its own tile
CODON_FL_HD void fl_tile_push(int tid, int k, int h, int w, unsigned short* pyr) {
  const int n = FL_TILE >> k, lg = FL_LOG - k, nu = n >> 1;
  unsigned short* cur = pyr + fl_pyr_off(k);
  const unsigned short* up = pyr + fl_pyr_off(k + 1);
  const int hk = fl_size(h, k), wk = fl_size(w, k), hu = fl_size(h, k + 1), wu = fl_size(w, k + 1);
  for (int idx = tid; idx < hk * n; idx += FL_THREADS) {
    const int y = idx >> lg, x = idx & (n - 1);
    if (x >= wk || cur[idx] != 0) continue;
    const int py = y >> 1, px = x >> 1, qy = fl_other(y, hu), qx = fl_other(x, wu);
    cur[idx] = (unsigned short)fl_mix(up[py * nu + px], up[py * nu + qx], up[qy * nu + px], up[qy * nu + qx]);
  }
}

// level 0 of the tile at (0, 0) to the h x w plane `out`
template <int FMT>
CODON_FL_HD void fl_tile_store(int tid, void* out, int h, int w, const float* tab, const unsigned short* pyr) {
  for (int idx = tid; idx < h * FL_TILE; idx += FL_THREADS) {
    const int y = idx >> FL_LOG, x = idx & (FL_TILE - 1);
    if (x < w) fl_store<FMT>(out, (long)y * w + x, pyr[idx], tab);
  }
}

// ---- the push of one tile of a larger plane -----------------------------------------------------------------------------------
// The halo pyramid `hp` of one tile: level k = FL_LOG .. 1 as (n_k + 2)^2 cells at fl_halo_off(k), n_k = FL_TILE >> k, sides
// 3, 4, 6, 10, 18, 34 -- FL_HALO_CELLS = 1641 cells in all.

CODON_FL_HD int fl_halo_off(int k) {                                                       // level 6 first, level 1 last
  return k == 6 ? 0 : k == 5 ? 9 : k == 4 ? 25 : k == 3 ? 61 : k == 2 ? 161 : 485;
}

// phase 1: the whole halo pyramid from this image's workspace `img` in ONE sweep -- F at level FL_LOG (already filled), V at
// levels FL_LOG - 1 .. 1.  Every thread first issues all of its loads, then stores them: one trip to memory, not one per level.
// `img` is this image's level 1 of one pyramid in the workspace.  HOLES: the cells are codes, 0 a hole (V, u16), and a cell
// outside the plane is stored as 0; else (the guided filler's A^ and G, u8) as its nearest cell inside.  Never read, either way.
template <bool HOLES, typename T>
CODON_FL_HD void fl_halo_load(int tid, int h, int w, int ty, int tx, const T* img, T* hp) {
  constexpr int PER = (FL_HALO_CELLS + FL_THREADS - 1) / FL_THREADS;                       // 7
  long base[FL_LOG + 1];
  base[0] = 0;
  base[1] = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 1; k < FL_LOG; ++k) base[k + 1] = base[k] + (long)fl_size(h, k) * fl_size(w, k);
  T v[PER];
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int q = 0; q < PER; ++q) {
    const int at = tid + q * FL_THREADS, idx = at < FL_HALO_CELLS ? at : FL_HALO_CELLS - 1;      // (the last sweep's tail re-reads a cell)
    const int k = idx < 9 ? 6 : idx < 25 ? 5 : idx < 61 ? 4 : idx < 161 ? 3 : idx < 485 ? 2 : 1;
    const long lb = k == 6 ? base[6] : k == 5 ? base[5] : k == 4 ? base[4] : k == 3 ? base[3] : k == 2 ? base[2] : base[1];
    const int n = FL_TILE >> k, s = n + 2, r = idx - fl_halo_off(k);
    const int i = r / s, j = r - i * s;
    const int gy = ty * n - 1 + i, gx = tx * n - 1 + j;
    const int hk = fl_size(h, k), wk = fl_size(w, k);
    const int cy = gy < 0 ? 0 : gy < hk ? gy : hk - 1, cx = gx < 0 ? 0 : gx < wk ? gx : wk - 1;
    const T c = img[lb + (long)cy * wk + cx];                    // no branch around the load: the loads go out together
    v[q] = (!HOLES || (cy == gy && cx == gx)) ? c : (T)0;
  }
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int q = 0; q < PER; ++q) {
    const int idx = tid + q * FL_THREADS;
    if (idx < FL_HALO_CELLS) hp[idx] = v[q];
  }
}

// F of the level-k cell (gy, gx), a hole there: the mix of `up`, the halo level k + 1 (side su, origin (uy0, ux0))
CODON_FL_HD int fl_halo_mix(int gy, int gx, int hu, int wu, const unsigned short* up, int su, int uy0, int ux0) {
  const int py = (gy >> 1) - uy0, px = (gx >> 1) - ux0, qy = fl_other(gy, hu) - uy0, qx = fl_other(gx, wu) - ux0;
  return fl_mix(up[py * su + px], up[py * su + qx], up[qy * su + px], up[qy * su + qx]);
}

// phase 2, k = FL_LOG - 1 .. 1: the holes of halo level k inside the plane, in place, from halo level k + 1
CODON_FL_HD void fl_halo_push(int tid, int k, int h, int w, int ty, int tx, unsigned short* hp) {
  const int n = FL_TILE >> k, s = n + 2, nu = n >> 1, su = nu + 2;
  const int hk = fl_size(h, k), wk = fl_size(w, k), hu = fl_size(h, k + 1), wu = fl_size(w, k + 1);
  const int gy0 = ty * n - 1, gx0 = tx * n - 1, uy0 = ty * nu - 1, ux0 = tx * nu - 1;
  unsigned short* cur = hp + fl_halo_off(k);
  const unsigned short* up = hp + fl_halo_off(k + 1);
  for (int idx = tid; idx < s * s; idx += FL_THREADS) {
    const int i = idx / s, j = idx - i * s;
    const int gy = gy0 + i, gx = gx0 + j;
    if (gy < 0 || gy >= hk || gx < 0 || gx >= wk || cur[idx] != 0) continue;
    cur[idx] = (unsigned short)fl_halo_mix(gy, gx, hu, wu, up, su, uy0, ux0);
  }
}

constexpr int FL_PER_THREAD = FL_TILE * FL_TILE / FL_THREADS;                              // 16 level-0 cells per thread

// the thread's level-0 codes of the tile, read before the pushes so that the trip to memory runs beside them; 0 outside the plane
template <int FMT>
CODON_FL_HD void fl_halo_in(int tid, int h, int w, int ty, int tx, const void* in, int top, int* v0) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int q = 0; q < FL_PER_THREAD; ++q) {
    const int idx = tid + q * FL_THREADS;
    const int gy = ty * FL_TILE + (idx >> FL_LOG), gx = tx * FL_TILE + (idx & (FL_TILE - 1));
    const int c = fl_load<FMT>(in, (long)(gy < h ? gy : h - 1) * w + (gx < w ? gx : w - 1), top);
    v0[q] = (gy < h && gx < w) ? c : 0;
  }
}

// phase 3, level 0: the tile's cells to the h x w plane `out`, a hole from halo level 1
template <int FMT>
CODON_FL_HD void fl_halo_out(int tid, int h, int w, int ty, int tx, const int* v0, const unsigned short* hp, void* out,
                             const float* tab) {
  const int nu = FL_TILE >> 1, su = nu + 2;
  const int hu = fl_size(h, 1), wu = fl_size(w, 1);
  const int uy0 = ty * nu - 1, ux0 = tx * nu - 1;
  const unsigned short* up = hp + fl_halo_off(1);
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int q = 0; q < FL_PER_THREAD; ++q) {
    const int idx = tid + q * FL_THREADS;
    const int gy = ty * FL_TILE + (idx >> FL_LOG), gx = tx * FL_TILE + (idx & (FL_TILE - 1));
    if (gy >= h || gx >= w) continue;
    int v = v0[q];
    if (v == 0) v = fl_halo_mix(gy, gx, hu, wu, up, su, uy0, ux0);
    fl_store<FMT>(out, (long)gy * w + gx, v, tab);
  }
}

// ---- the workgroup bodies -------------------------------------------------------------------------------------------------------
// LDS: pyr is FL_PYR_CELLS cells, hp is FL_HALO_CELLS cells.

// workgroup b of grid (B): the h x w plane that is its own tile.  in / out: image b at + b * stride elements; they may be the
// same buffer (level 6 of the workspace): the whole plane is in LDS before any of it is written
template <int FMT, class G>
CODON_FL_HD void wg_fill_plane(G wg, long b, const void* in, long in_stride, void* out, long out_stride, int h, int w,
                               const float* tab, int top, unsigned short* pyr) {
  const int K = fl_top_level(h, w);                                // uniform, <= FL_LOG
  WG_EACH(wg, tid) fl_tile_load<FMT>(tid, (const char*)in + b * in_stride * fl_elem_bytes(FMT), h, w, 0, 0, top, pyr);
  wg.sync();
  for (int k = 0; k < K; ++k) {
    WG_EACH(wg, tid) fl_tile_pull(tid, k, pyr, nullptr, h, w, 0, 0);
    wg.sync();
  }
  for (int k = K - 1; k >= 0; --k) {
    WG_EACH(wg, tid) fl_tile_push(tid, k, h, w, pyr);
    wg.sync();
  }
  WG_EACH(wg, tid) fl_tile_store<FMT>(tid, (char*)out + b * out_stride * fl_elem_bytes(FMT), h, w, tab, pyr);
}

// workgroup (tx, ty, b) of grid (gx, gy, B): levels 1 .. 6 of one tile, to the workspace
template <int FMT, class G>
CODON_FL_HD void wg_fill_pull(G wg, int tx, int ty, long b, const void* in, int h, int w, int top, unsigned short* ws,
                              long ws_stride, unsigned short* pyr) {
  WG_EACH(wg, tid)
    fl_tile_load<FMT>(tid, (const char*)in + b * h * w * fl_elem_bytes(FMT), h, w, ty * FL_TILE, tx * FL_TILE, top, pyr);
  wg.sync();
  unsigned short* lvl = ws + b * ws_stride;                         // level k + 1 of this image
  for (int k = 0; k < FL_LOG; ++k) {
    WG_EACH(wg, tid) fl_tile_pull(tid, k, pyr, lvl, h, w, ty, tx);
    lvl += (long)fl_size(h, k + 1) * fl_size(w, k + 1);
    wg.sync();
  }
}

// workgroup (tx, ty, b) of grid (gx, gy, B): one tile's holes from the workspace's filled level 6 down, to the output
template <int FMT, class G>
CODON_FL_HD void wg_fill_push(G wg, int tx, int ty, long b, const void* in, void* out, int h, int w, const float* tab, int top,
                              const unsigned short* ws, long ws_stride, unsigned short* hp) {
  const long at = b * h * w * fl_elem_bytes(FMT);
  typename G::template Regs<int, FL_PER_THREAD> v0(wg);
  WG_EACH(wg, tid) {
    fl_halo_load<true>(tid, h, w, ty, tx, ws + b * ws_stride, hp);
    fl_halo_in<FMT>(tid, h, w, ty, tx, (const char*)in + at, top, v0[tid]);
  }
  wg.sync();
  for (int k = FL_LOG - 1; k >= 1; --k) {
    WG_EACH(wg, tid) fl_halo_push(tid, k, h, w, ty, tx, hp);
    wg.sync();
  }
  WG_EACH(wg, tid) fl_halo_out<FMT>(tid, h, w, ty, tx, v0[tid], hp, (char*)out + at, tab);
}

}  // namespace codon
