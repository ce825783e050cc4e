// The guidance-aware (joint) pull-push hole filler (fill_guided.hip): its launch plan (fg_plan), its three
// workgroup bodies (wg_fillg_*, over wg.h's group type: DESIGN 12.13) and the per-thread phases they run, written like fill_tile.h
// so that the SAME text compiles for the device and for a plain host compiler: the kernels and tools/guided_fill_host_check.cpp,
// under the address and undefined-behaviour sanitizers, call the same bodies.  Integers only.
//
// Three pyramids ride together, all with fill_tile.h's geometry (tile pyramid: level k at fl_pyr_off(k), row stride FL_TILE >> k;
// halo pyramid: level k at fl_halo_off(k), side (FL_TILE >> k) + 2):
//   v  u16  the depth pyramid: the plain filler's V, 0 a hole, then F in place
//   g  u8   the guidance pyramid: G_0 the s x s box mean of the high-resolution guidance, G_{k+1} the mean over the children
//           inside level k, halves rounded up
//   a  u8   the attached guidance A^: at a valid cell the mean of A over the valid children that entered V (A_0 = G_0), at a
//           hole G itself -- the rule "A where V is valid, else G" is applied once, when the level is pulled, so that the push
//           never needs to know which cells of the level above were holes
// A hole at (y, x) of level k weighs the plain filler's four parents p by w_p = B_p T[|G_k(y, x) - A^_{k+1}(p)|], B = 9, 3, 3, 1,
// and takes (2 sum w_p F_{k+1}(p) + sum w_p) / (2 sum w_p);  16 <= sum w_p <= 4096 and 2 * 4096 * 65535 + 4096 < 2^31.
//   fg_tab_load     the range table T (256 u16) into LDS
//   fg_g0_tile<S>   G_0 (and A_0 = G_0) of the tile from the guidance image, row segments of 16 bytes read as one load where the
//                   image and its row stride are 16-byte aligned, as 4-byte words where they are 4-byte aligned, else bytes
//   fg_plane_load8  A^ and G of a plane that is its own tile from two u8 planes (level 6 of a larger plane, from the workspace)
//   fg_pull         level k -> k + 1 of v, a and g, and (ws != null) the in-plane cells out to the workspace
//   fg_push         level k's holes from level k + 1 (a plane that is its own tile)
//   fl_halo_load    (fill_tile.h's, over u8 cells) the halo pyramids of A^ and G from the workspace, one sweep each
//   fg_halo_g0      the thread's level-0 G of the tile from the workspace into registers
//   fg_halo_push    the holes of halo level k from halo level k + 1, in place
//   fg_halo_out     F at level 0 over the tile's cells, to the output plane
// Workspace of one image, fg_workspace_bytes(h, w) bytes with C = fl_workspace_cells(h, w): V of levels 1 .. K (u16) at 0, A^ at
// fg_a_at(C), G at fg_g_at(C) (u8, the same level offsets in cells), G_0 (h x w, u8) at fg_g0_at(C).
#pragma once

#include <stdint.h>
#include <string.h>

#include "fill_tile.h"

namespace codon {

constexpr int FG_TAB = 256;

// byte offsets of the planes in one image's workspace of C = fl_workspace_cells(h, w) cells per pyramid
CODON_FL_HD long fg_a_at(long cells) { return 2 * cells; }
CODON_FL_HD long fg_g_at(long cells) { return 3 * cells; }
CODON_FL_HD long fg_g0_at(long cells) { return 4 * cells; }
CODON_FL_HD long fg_workspace_bytes(int h, int w) { return fg_g0_at(fl_workspace_cells(h, w)) + (long)h * w; }

// The launches of an h x w plane: the plain filler's (FlPlan), with the workspace in bytes.  Level 6 of each image: V (u16) at
// byte v6, A^ and G (u8) at bytes a6 and g6
struct FgPlan {
  int single, gx, gy, h6, w6;
  long v6, a6, g6;
  long stride;                    // workspace bytes per image: never 0, and images 16 bytes apart
};
CODON_FL_HD FgPlan fg_plan(int h, int w) {
  const FlPlan f = fl_plan(h, w);
  const long cells = fl_workspace_cells(h, w);
  FgPlan p;
  p.single = f.single;
  p.gx = f.gx;
  p.gy = f.gy;
  p.h6 = f.h6;
  p.w6 = f.w6;
  p.v6 = 2 * f.l6;
  p.a6 = fg_a_at(cells) + f.l6;
  p.g6 = fg_g_at(cells) + f.l6;
  p.stride = (fg_workspace_bytes(h, w) + 15) / 16 * 16;
  return p;
}
CODON_FL_HD int fg_log2(int s) { return s == 4 ? 2 : s == 8 ? 3 : 4; }

CODON_FL_HD void fg_tab_load(int tid, const unsigned short* tab, unsigned short* t) {
  if (tid < FG_TAB) t[tid] = tab[tid];
}

// acc + the four bytes of q; on the device one v_sad_u8 (the sum of absolute differences against 0), which also keeps the
// compiler from spreading sixteen loads into 256 separate byte registers before it adds them
CODON_FL_HD int fg_bytes_add(unsigned q, int acc) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (int)__builtin_amdgcn_sad_u8(q, 0u, (unsigned)acc);
#else
  return acc + (int)((q & 255u) + ((q >> 8) & 255u) + ((q >> 16) & 255u) + (q >> 24));
#endif
}
CODON_FL_HD void fg_load16(const unsigned char* p, unsigned* q) { memcpy(q, __builtin_assume_aligned(p, 16), 16); }
CODON_FL_HD unsigned fg_load4(const unsigned char* p) {
  unsigned q;
  memcpy(&q, __builtin_assume_aligned(p, 4), 4);
  return q;
}

// G_0 of the tile at (y0, x0) of the h x w plane from its guidance image `gimg` (rows row_bytes apart, at least w * S bytes
// each): g, a (when not null) and ws_g0 (when not null: the h x w plane of the workspace) get the box means of the in-plane
// cells.  A work item is one 16-byte segment of the tile's high-resolution rows over the S rows of a cell row: neighbouring
// threads read neighbouring segments.  Where the image and its row stride are 16-byte aligned, the segments that lie whole
// inside the plane go in batches of 16 / S items per thread: sixteen 16-byte loads are issued, without a branch around
// them, before the first is used -- one trip to memory per batch.  What is left (the last, partial segment of a row, or
// everything of an image that is not aligned) is read as 4-byte words where those are aligned, else as bytes.
CODON_FL_HD void fg_g0_put(int i, int c, int mean, int w, int y0, int x0, unsigned char* g, unsigned char* a, unsigned char* ws_g0) {
  g[i * FL_TILE + c] = (unsigned char)mean;
  if (a) a[i * FL_TILE + c] = (unsigned char)mean;
  if (ws_g0) ws_g0[(long)(y0 + i) * w + x0 + c] = (unsigned char)mean;
}

template <int S>
CODON_FL_HD void fg_g0_tile(int tid, const unsigned char* gimg, long row_bytes, int h, int w, int y0, int x0, unsigned char* g,
                            unsigned char* a, unsigned char* ws_g0) {
  constexpr int LGS = S == 4 ? 2 : S == 8 ? 3 : 4;
  constexpr int CPS = 16 / S;                                    // cells per segment, and items per batch: 4, 2, 1
  constexpr int NSEG = FL_TILE / CPS, LGSEG = FL_LOG - (4 - LGS);  // segments per row of the tile: 16, 32, 64
  const int th = h - y0 < FL_TILE ? h - y0 : FL_TILE, tw = w - x0 < FL_TILE ? w - x0 : FL_TILE;
  const bool al16 = ((((uintptr_t)gimg) | (uintptr_t)row_bytes) & 15) == 0;
  const bool al4 = ((((uintptr_t)gimg) | (uintptr_t)row_bytes) & 3) == 0;
  const int nfull = al16 ? (tw * S) >> 4 : 0;                    // a row's segments that lie whole inside the plane
  const unsigned char* p00 = gimg + (long)y0 * S * row_bytes + (long)x0 * S;
  if (nfull > 0) {
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int idx0 = tid; idx0 < th * NSEG; idx0 += CPS * FL_THREADS) {
      unsigned q[CPS][S][4];
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int u = 0; u < CPS; ++u) {
        const int idx = idx0 + u * FL_THREADS, i = idx >> LGSEG, j = idx & (NSEG - 1);
        const bool ok = idx < th * NSEG && j < nfull;
        const unsigned char* p = ok ? p00 + (long)i * S * row_bytes + j * 16 : p00;     // (an item out of range re-reads the first)
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int r = 0; r < S; ++r) fg_load16(p + r * row_bytes, q[u][r]);
      }
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int u = 0; u < CPS; ++u) {
        const int idx = idx0 + u * FL_THREADS, i = idx >> LGSEG, j = idx & (NSEG - 1);
        if (idx >= th * NSEG || j >= nfull) continue;
        int sum[CPS];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int c = 0; c < CPS; ++c) sum[c] = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int r = 0; r < S; ++r) {
#if defined(__HIPCC__)
#pragma unroll
#endif
          for (int e = 0; e < 4; ++e) sum[e >> (LGS - 2)] = fg_bytes_add(q[u][r][e], sum[e >> (LGS - 2)]);
        }
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int c = 0; c < CPS; ++c)                            // the box mean, half rounded up
          fg_g0_put(i, j * CPS + c, (2 * sum[c] + S * S) >> (2 * LGS + 1), w, y0, x0, g, a, ws_g0);
      }
    }
  }
#if defined(__HIPCC__)
#pragma unroll 1
#endif
  for (int idx = tid; idx < th * NSEG; idx += FL_THREADS) {      // the rest, one item at a time
    const int i = idx >> LGSEG, j = idx & (NSEG - 1);
    const int c0 = j * CPS;
    if (j < nfull || c0 >= tw) continue;
    const int nc = tw - c0 < CPS ? tw - c0 : CPS;
    const unsigned char* p = p00 + (long)i * S * row_bytes + (long)c0 * S;
    int sum[CPS];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int c = 0; c < CPS; ++c) sum[c] = 0;
    if (al4) {
#if defined(__HIPCC__)
#pragma unroll 4
#endif
      for (int r = 0; r < S; ++r) {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int e = 0; e < 4; ++e)
          if ((e >> (LGS - 2)) < nc) sum[e >> (LGS - 2)] = fg_bytes_add(fg_load4(p + r * row_bytes + 4 * e), sum[e >> (LGS - 2)]);
      }
    } else {
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int c = 0; c < CPS; ++c) {
        if (c >= nc) continue;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
        for (int r = 0; r < S; ++r)
          for (int e = 0; e < S; ++e) sum[c] += p[r * row_bytes + c * S + e];
      }
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int c = 0; c < CPS; ++c) {
      if (c >= nc) continue;
      fg_g0_put(i, c0 + c, (2 * sum[c] + S * S) >> (2 * LGS + 1), w, y0, x0, g, a, ws_g0);
    }
  }
}

// level 0 of a and g of an h x w plane (h, w <= FL_TILE) from the dense u8 planes a0 and g0
CODON_FL_HD void fg_plane_load8(int tid, const unsigned char* a0, const unsigned char* g0, int h, int w, unsigned char* a,
                                unsigned char* g) {
  for (int idx = tid; idx < h * FL_TILE; idx += FL_THREADS) {
    const int y = idx >> FL_LOG, x = idx & (FL_TILE - 1);
    if (x >= w) continue;
    a[idx] = a0[y * w + x];
    g[idx] = g0[y * w + x];
  }
}

// level k -> k + 1 of the tile (ty, tx) of the h x w plane (k = 0 .. FL_LOG - 1).  ws_v != null: the in-plane cells of level
// k + 1 also go to this image's level k + 1 in the workspace (ws_v, ws_a, ws_g: h_{k+1} x w_{k+1} cells each)
CODON_FL_HD void fg_pull(int tid, int k, unsigned short* v, unsigned char* a, unsigned char* g, int h, int w, int ty, int tx,
                         unsigned short* ws_v, unsigned char* ws_a, unsigned char* ws_g) {
  const int n = FL_TILE >> (k + 1), lg = FL_LOG - (k + 1);
  const int so = fl_pyr_off(k), d = fl_pyr_off(k + 1);
  const int hk = fl_size(h, k), wk = fl_size(w, k), hu = fl_size(h, k + 1), wu = fl_size(w, k + 1);
  for (int idx = tid; idx < n * n; idx += FL_THREADS) {
    const int i = idx >> lg, j = idx & (n - 1);
    const int gy = ty * n + i, gx = tx * n + j;
    if (gy >= hu || gx >= wu) {                                  // outside the plane: a hole, never a child
      v[d + idx] = 0;
      continue;
    }
    const int o = so + (2 * i) * (2 * n) + 2 * j;
    const bool in_x = 2 * gx + 1 < wk, in_y = 2 * gy + 1 < hk;  // the children (., +1) lie inside level k
    const int v00 = v[o], v01 = in_x ? v[o + 1] : 0, v10 = in_y ? v[o + 2 * n] : 0, v11 = (in_x && in_y) ? v[o + 2 * n + 1] : 0;
    const int g00 = g[o], g01 = in_x ? g[o + 1] : 0, g10 = in_y ? g[o + 2 * n] : 0, g11 = (in_x && in_y) ? g[o + 2 * n + 1] : 0;
    const int lgn = (int)in_x + (int)in_y;                       // n = 1, 2 or 4 children inside
    const int gm = (2 * (g00 + g01 + g10 + g11) + (1 << lgn)) >> (lgn + 1);
    const int nv = (v00 != 0) + (v01 != 0) + (v10 != 0) + (v11 != 0);
    const int sa = (v00 ? a[o] : 0) + (v01 ? a[o + 1] : 0) + (v10 ? a[o + 2 * n] : 0) + (v11 ? a[o + 2 * n + 1] : 0);
    const int vm = fl_pull4(v00, v01, v10, v11);
    const int am = nv ? (2 * sa + nv) / (2 * nv) : gm;           // a hole carries its own guidance
    v[d + idx] = (unsigned short)vm;
    a[d + idx] = (unsigned char)am;
    g[d + idx] = (unsigned char)gm;
    if (ws_v) {
      const long at = (long)gy * wu + gx;
      ws_v[at] = (unsigned short)vm;
      ws_a[at] = (unsigned char)am;
      ws_g[at] = (unsigned char)gm;
    }
  }
}

// the guidance-weighted mix of the four parents: gk the hole's own guidance, f / a the parents' filled values and attached
// guidance in the order near, qx, qy, far
CODON_FL_HD int fg_mix(int gk, int f0, int f1, int f2, int f3, int a0, int a1, int a2, int a3, const unsigned short* t) {
  const int d0 = gk - a0, d1 = gk - a1, d2 = gk - a2, d3 = gk - a3;
  const unsigned w0 = 9u * t[d0 < 0 ? -d0 : d0], w1 = 3u * t[d1 < 0 ? -d1 : d1], w2 = 3u * t[d2 < 0 ? -d2 : d2],
                 w3 = t[d3 < 0 ? -d3 : d3];
  const unsigned sw = w0 + w1 + w2 + w3;
  const unsigned sf = w0 * (unsigned)f0 + w1 * (unsigned)f1 + w2 * (unsigned)f2 + w3 * (unsigned)f3;
  return (int)((2u * sf + sw) / (2u * sw));
}

// level k's holes from level k + 1 (k = K - 1 .. 0, K <= FL_LOG): the plane h x w is its own tile
CODON_FL_HD void fg_push(int tid, int k, int h, int w, unsigned short* v, const unsigned char* a, const unsigned char* g,
                         const unsigned short* t) {
  const int n = FL_TILE >> k, lg = FL_LOG - k, nu = n >> 1;
  const int co = fl_pyr_off(k), uo = fl_pyr_off(k + 1);
  const int hk = fl_size(h, k), wk = fl_size(w, k), hu = fl_size(h, k + 1), wu = fl_size(w, k + 1);
  for (int idx = tid; idx < hk * n; idx += FL_THREADS) {
    const int y = idx >> lg, x = idx & (n - 1);
    if (x >= wk || v[co + idx] != 0) continue;
    const int py = y >> 1, px = x >> 1, qy = fl_other(y, hu), qx = fl_other(x, wu);
    const int p0 = uo + py * nu + px, p1 = uo + py * nu + qx, p2 = uo + qy * nu + px, p3 = uo + qy * nu + qx;
    v[co + idx] = (unsigned short)fg_mix(g[co + idx], v[p0], v[p1], v[p2], v[p3], a[p0], a[p1], a[p2], a[p3], t);
  }
}

// ---- the push of one tile of a larger plane -----------------------------------------------------------------------------------

// the thread's level-0 guidance of the tile from the workspace's G_0 plane (h x w); unused outside the plane
CODON_FL_HD void fg_halo_g0(int tid, int h, int w, int ty, int tx, const unsigned char* ws_g0, int* g0) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int q = 0; q < FL_PER_THREAD; ++q) {
    const int idx = tid + q * FL_THREADS;
    const int gy = ty * FL_TILE + (idx >> FL_LOG), gx = tx * FL_TILE + (idx & (FL_TILE - 1));
    g0[q] = ws_g0[(long)(gy < h ? gy : h - 1) * w + (gx < w ? gx : w - 1)];
  }
}

// F of the level-k cell (gy, gx) of guidance gk, a hole there: the weighted mix of halo level k + 1 (side su, origin (uy0, ux0))
CODON_FL_HD int fg_halo_mix(int gk, int gy, int gx, int hu, int wu, const unsigned short* uv, const unsigned char* ua, int su,
                            int uy0, int ux0, const unsigned short* t) {
  const int py = (gy >> 1) - uy0, px = (gx >> 1) - ux0, qy = fl_other(gy, hu) - uy0, qx = fl_other(gx, wu) - ux0;
  const int p0 = py * su + px, p1 = py * su + qx, p2 = qy * su + px, p3 = qy * su + qx;
  return fg_mix(gk, uv[p0], uv[p1], uv[p2], uv[p3], ua[p0], ua[p1], ua[p2], ua[p3], t);
}

// k = FL_LOG - 1 .. 1: the holes of halo level k inside the plane, in place, from halo level k + 1
CODON_FL_HD void fg_halo_push(int tid, int k, int h, int w, int ty, int tx, unsigned short* hv, const unsigned char* ha,
                              const unsigned char* hg, const unsigned short* t) {
  const int n = FL_TILE >> k, s = n + 2, nu = n >> 1, su = nu + 2;
  const int hk = fl_size(h, k), wk = fl_size(w, k), hu = fl_size(h, k + 1), wu = fl_size(w, k + 1);
  const int gy0 = ty * n - 1, gx0 = tx * n - 1, uy0 = ty * nu - 1, ux0 = tx * nu - 1;
  const int co = fl_halo_off(k), uo = fl_halo_off(k + 1);
  for (int idx = tid; idx < s * s; idx += FL_THREADS) {
    const int i = idx / s, j = idx - i * s;
    const int gy = gy0 + i, gx = gx0 + j;
    if (gy < 0 || gy >= hk || gx < 0 || gx >= wk || hv[co + idx] != 0) continue;
    hv[co + idx] = (unsigned short)fg_halo_mix(hg[co + idx], gy, gx, hu, wu, hv + uo, ha + uo, su, uy0, ux0, t);
  }
}

// level 0: the tile's cells to the h x w plane `out`, a hole from halo level 1.  The mix is worked out for every cell, valid or
// not, without a branch (a cell outside the plane stands in for its nearest one inside): with a hole anywhere in the wave the
// wave runs the mix anyway, and sixteen independent mixes hide each other's trips to LDS and their divisions
template <int FMT>
CODON_FL_HD void fg_halo_out(int tid, int h, int w, int ty, int tx, const int* v0, const int* g0, const unsigned short* hv,
                             const unsigned char* ha, const unsigned short* t, void* out) {
  const int nu = FL_TILE >> 1, su = nu + 2;
  const int hu = fl_size(h, 1), wu = fl_size(w, 1);
  const int uy0 = ty * nu - 1, ux0 = tx * nu - 1, uo = fl_halo_off(1);
  int f[FL_PER_THREAD];
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int q = 0; q < FL_PER_THREAD; ++q) {
    const int idx = tid + q * FL_THREADS;
    const int gy = ty * FL_TILE + (idx >> FL_LOG), gx = tx * FL_TILE + (idx & (FL_TILE - 1));
    const int m = fg_halo_mix(g0[q], gy < h ? gy : h - 1, gx < w ? gx : w - 1, hu, wu, hv + uo, ha + uo, su, uy0, ux0, t);
    f[q] = v0[q] ? v0[q] : m;
  }
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int q = 0; q < FL_PER_THREAD; ++q) {
    const int idx = tid + q * FL_THREADS;
    const int gy = ty * FL_TILE + (idx >> FL_LOG), gx = tx * FL_TILE + (idx & (FL_TILE - 1));
    if (gy < h && gx < w) fl_store<FMT>(out, (long)gy * w + gx, f[q], nullptr);
  }
}

// ---- the workgroup bodies -------------------------------------------------------------------------------------------------------
// LDS: v (u16), a and g (u8) are FL_PYR_CELLS cells each; hv (u16), ha and hg (u8) FL_HALO_CELLS cells each; t is FG_TAB u16.

// one phase: G_0 (and A_0) of the tile at (y0, x0) from the guidance image, by the scale
template <class G>
CODON_FL_HD void wg_fillg_g0(G wg, int scale, const unsigned char* gimg, long row_bytes, int h, int w, int y0, int x0,
                             unsigned char* g, unsigned char* a, unsigned char* ws_g0) {
  if (scale == 4) {
    WG_EACH(wg, tid) fg_g0_tile<4>(tid, gimg, row_bytes, h, w, y0, x0, g, a, ws_g0);
  } else if (scale == 8) {
    WG_EACH(wg, tid) fg_g0_tile<8>(tid, gimg, row_bytes, h, w, y0, x0, g, a, ws_g0);
  } else {
    WG_EACH(wg, tid) fg_g0_tile<16>(tid, gimg, row_bytes, h, w, y0, x0, g, a, ws_g0);
  }
}

// workgroup b of grid (B): the h x w plane that is its own tile.  in / out: image b at + b * stride elements; they may be the
// same buffer (level 6 of the workspace).  guide != null: G_0 from image b of the guidance; else A^ and G of the plane from
// a0 / g0 (image b at + b * ag_stride bytes)
template <int FMT, class G>
CODON_FL_HD void wg_fillg_plane(G wg, long b, const void* in, long in_stride, void* out, long out_stride, int h, int w, int top,
                                const unsigned char* guide, long row_bytes, long image_bytes, int scale, const unsigned char* a0,
                                const unsigned char* g0, long ag_stride, const unsigned short* tab, unsigned short* v,
                                unsigned char* a, unsigned char* g, unsigned short* t) {
  const int K = fl_top_level(h, w);                                // uniform, <= FL_LOG
  WG_EACH(wg, tid) {
    fg_tab_load(tid, tab, t);
    fl_tile_load<FMT>(tid, (const char*)in + b * in_stride * fl_elem_bytes(FMT), h, w, 0, 0, top, v);
  }
  if (guide) {
    wg_fillg_g0(wg, scale, guide + b * image_bytes, row_bytes, h, w, 0, 0, g, a, nullptr);
  } else {
    WG_EACH(wg, tid) fg_plane_load8(tid, a0 + b * ag_stride, g0 + b * ag_stride, h, w, a, g);
  }
  wg.sync();
  for (int k = 0; k < K; ++k) {
    WG_EACH(wg, tid) fg_pull(tid, k, v, a, g, h, w, 0, 0, nullptr, nullptr, nullptr);
    wg.sync();
  }
  for (int k = K - 1; k >= 0; --k) {
    WG_EACH(wg, tid) fg_push(tid, k, h, w, v, a, g, t);
    wg.sync();
  }
  WG_EACH(wg, tid) fl_tile_store<FMT>(tid, (char*)out + b * out_stride * fl_elem_bytes(FMT), h, w, nullptr, v);
}

// workgroup (tx, ty, b) of grid (gx, gy, B): V_0 and G_0 of one tile (G_0 also to the workspace), then levels 1 .. 6 of the
// three pyramids to the workspace.  ws: image b at + b * ws_stride bytes
template <int FMT, class G>
CODON_FL_HD void wg_fillg_pull(G wg, int tx, int ty, long b, const void* in, int h, int w, int top, const unsigned char* guide,
                               long row_bytes, long image_bytes, int scale, unsigned char* ws, long ws_stride, unsigned short* v,
                               unsigned char* a, unsigned char* g) {
  const long cells = fl_workspace_cells(h, w);
  unsigned char* img = ws + b * ws_stride;
  WG_EACH(wg, tid)
    fl_tile_load<FMT>(tid, (const char*)in + b * h * w * fl_elem_bytes(FMT), h, w, ty * FL_TILE, tx * FL_TILE, top, v);
  wg_fillg_g0(wg, scale, guide + b * image_bytes, row_bytes, h, w, ty * FL_TILE, tx * FL_TILE, g, a, img + fg_g0_at(cells));
  wg.sync();
  long at = 0;                                                      // level k + 1 of this image, in cells
  for (int k = 0; k < FL_LOG; ++k) {
    WG_EACH(wg, tid)
      fg_pull(tid, k, v, a, g, h, w, ty, tx, (unsigned short*)img + at, img + fg_a_at(cells) + at, img + fg_g_at(cells) + at);
    at += (long)fl_size(h, k + 1) * fl_size(w, k + 1);
    wg.sync();
  }
}

// workgroup (tx, ty, b) of grid (gx, gy, B): one tile's holes from the workspace's filled level 6 down, to the output
template <int FMT, class G>
CODON_FL_HD void wg_fillg_push(G wg, int tx, int ty, long b, const void* in, void* out, int h, int w, int top,
                               const unsigned short* tab, const unsigned char* ws, long ws_stride, unsigned short* hv,
                               unsigned char* ha, unsigned char* hg, unsigned short* t) {
  const long at = b * h * w * fl_elem_bytes(FMT);
  const long cells = fl_workspace_cells(h, w);
  const unsigned char* img = ws + b * ws_stride;
  typename G::template Regs<int, FL_PER_THREAD> v0(wg), g0(wg);
  WG_EACH(wg, tid) {
    fg_tab_load(tid, tab, t);
    fl_halo_load<true>(tid, h, w, ty, tx, (const unsigned short*)img, hv);
    fl_halo_load<false>(tid, h, w, ty, tx, img + fg_a_at(cells), ha);
    fl_halo_load<false>(tid, h, w, ty, tx, img + fg_g_at(cells), hg);
    fl_halo_in<FMT>(tid, h, w, ty, tx, (const char*)in + at, top, v0[tid]);
    fg_halo_g0(tid, h, w, ty, tx, img + fg_g0_at(cells), g0[tid]);
  }
  wg.sync();
  for (int k = FL_LOG - 1; k >= 1; --k) {
    WG_EACH(wg, tid) fg_halo_push(tid, k, h, w, ty, tx, hv, ha, hg, t);
    wg.sync();
  }
  WG_EACH(wg, tid) fg_halo_out<FMT>(tid, h, w, ty, tx, v0[tid], g0[tid], hv, ha, t, (char*)out + at);
}

}  // namespace codon
