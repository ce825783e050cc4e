// The outlier rejection of sensor depth maps (clean.hip): its launch plan (cl_plan), its workgroup bodies
// (wg_clean_zero, wg_clean_flying, wg_clean_link, wg_clean_count, wg_clean_apply, over wg.h's group type: DESIGN 12.13) and the
// per-thread phases they run, written like register_tile.h so that the SAME text compiles for the device and for a plain host
// compiler: the kernels and tools/clean_host_check.cpp, under the address and undefined-behaviour sanitizers, call the same
// bodies.  Integers only.
//
// The definition (tests/clean_ref.py): tau(v) = A + ((Rq v) >> 16), the product in UNSIGNED 32 bits (65535 * 65535 < 2^32); two
// pixels are linked iff both are non-zero and |c_p - c_q| <= tau(min(c_p, c_q)).  Rule 1: a valid pixel with fewer than K of its 8
// neighbours inside the plane linked to it becomes 0 (K = 0: off); it reads the input, never its own result.  Rule 2: the
// components of the result k under 4-connectivity, two 4-neighbours in one component iff linked; a component of fewer than N
// pixels becomes 0 (N <= 1: off).  Statistics per image: valid inputs, pixels rule 1 removed, pixels rule 2 removed, components
// rule 2 removed.
//
// The launches, a function of (B, h, w) and of whether rule 2 is on:
//   rule 2 off   wg_clean_zero     one workgroup: the statistics to 0
//                wg_clean_flying   one CL_TILE x CL_TILE tile of one image plus a halo of 1 in LDS, a word per cell: k to `out`,
//                                  the tile's valid and flying counts summed through LDS, one atomic add per count that is not 0
//   rule 2 on    wg_clean_flying   the same tile: k to `out`, the pixel's size word to 0; the tile's own links (right and down, inside
//                                  the tile) united on tile-local labels in LDS, and the pixel's label word to the index in the
//                                  image of its tile-local root (a hole: all ones); tile (0, 0) of an image zeroes its statistics
//                wg_clean_link     the last column and the last row of a tile unite themselves with their right and lower
//                                  neighbour in the next tile where linked: lock-free union-find on the label plane, a root's
//                                  label its own index (cl_find, cl_unite).  (CODON_CLEAN_LOCAL=0: labels start as the pixels'
//                                  own indices and every link is united here)
//                wg_clean_count    every non-zero pixel finds its root and writes it back as its label; the runs of equal roots
//                                  in a tile's rows, found through LDS, add their length to the root's size word -- unless the
//                                  word already reads N or more: only "size >= N" is ever asked, and a word that reached N stays
//                                  there, so the decision is exact though the word is not
//                wg_clean_apply    CL_RUN pixels of one image: out = 0 where size[label] < N, in place; the four counts
//
// Termination: a label only ever points from a larger index to a smaller one.  cl_find from x strictly descends, so
// it ends within x steps; a trip of cl_unite either finishes or strictly lowers its larger endpoint, so it ends within
// max(a, b) + 1 trips.  Both bounds are the loops' trip limits, and a label that points upwards (a broken invariant) is taken for a
// root: wrong bytes, never a hang and never an index outside the plane.
#pragma once

#include "fill_tile.h"

// 1: a tile's own links are united in LDS by the flying launch, which then writes every pixel's label as its tile-local root, and
// the link launch unites across tile borders alone; 0: every link is united on the label plane in global memory (the A/B of
// DESIGN 12.17)
#ifndef CODON_CLEAN_LOCAL
#define CODON_CLEAN_LOCAL 1
#endif

namespace codon {

constexpr bool CL_LOCAL = CODON_CLEAN_LOCAL != 0;
constexpr int CL_TILE = 16, CL_THREADS = CL_TILE * CL_TILE;         // 256: one pixel per thread
constexpr int CL_HALO = CL_TILE + 2, CL_CELLS = CL_HALO * CL_HALO;  // 18 x 18 = 324 words
constexpr int CL_PER = 4, CL_RUN = CL_THREADS * CL_PER;             // apply: four pixels per thread
constexpr int CL_MAX_SIDE = FL_MAX_SIDE;
constexpr int CL_MAX_SUPPORT = 8, CL_MAX_REGION = 1 << 24, CL_MAX_REL = 65535;
constexpr unsigned CL_EMPTY = 0xFFFFFFFFu;
constexpr int CL_VALID = 0, CL_FLYING = 1, CL_SPECKLE = 2, CL_REGIONS = 3, CL_STATS = 4;

struct ClArgs {
  int h, w;
  unsigned tol_abs, tol_rel;       // A, and Rq = rint(65536 rel)
  int support, region;             // K, N
};

// The launches of B planes of h x w: the tile bodies over sx x sy tiles per image, the apply body over rx runs per image; the
// label plane and the size plane of the workspace hold B images `stride` words apart each (16 bytes a multiple)
struct ClPlan {
  int sx, sy, rx, rule2;
  long stride;
};
CODON_FL_HD ClPlan cl_plan(int h, int w, int region) {
  ClPlan p;
  p.sx = (w + CL_TILE - 1) / CL_TILE;
  p.sy = (h + CL_TILE - 1) / CL_TILE;
  p.rx = (int)(((long)h * w + CL_RUN - 1) / CL_RUN);
  p.rule2 = region > 1;
  p.stride = ((long)h * w + 3) / 4 * 4;
  return p;
}
CODON_FL_HD long cl_workspace_words(int B, int h, int w) { return 2 * cl_plan(h, w, 2).stride * B; }

// tau in unsigned 32 bits: tol_rel <= 65535 and a code <= 65535, the product below 2^32; the sum below 2^17
CODON_FL_HD bool cl_linked(unsigned a, unsigned b, unsigned tol_abs, unsigned tol_rel) {
  const unsigned lo = a < b ? a : b, hi = a < b ? b : a;
  return lo != 0u && hi - lo <= tol_abs + ((tol_rel * lo) >> 16);
}

// the root of x: at most x steps, since every step strictly descends
template <class G>
CODON_FL_HD unsigned cl_find(G wg, const unsigned* label, unsigned x) {
  for (unsigned trip = x; trip != 0u; --trip) {
    const unsigned y = wg.load_relaxed(label + x);
    if (y >= x) break;             // y == x: a root; y > x never happens, and would end here as one
    x = y;
  }
  return x;
}

// a and b into one tree: at most max(a, b) + 1 trips, since a trip that does not finish strictly lowers the larger endpoint.  A
// stale read in cl_find gives an older ancestor, which the returning minimum then corrects
template <class G>
CODON_FL_HD void cl_unite(G wg, unsigned* label, unsigned a, unsigned b) {
  for (unsigned trip = (a > b ? a : b) + 1u; trip != 0u; --trip) {
    a = cl_find(wg, label, a);
    b = cl_find(wg, label, b);
    if (a == b) return;
    const unsigned lo = a < b ? a : b, hi = a < b ? b : a;
    const unsigned old = wg.atomic_min_old(label + hi, lo);
    if (old >= hi) return;         // hi was a root, and now points to lo
    a = lo;                        // hi pointed to old < hi already, and now to min(old, lo): lo and old remain to be united
    b = old;
  }
}

// the sums over the workgroup of two packed words per thread (cnt[tid] and cnt[CL_THREADS + tid], two fields of 16 bits each, a
// thread adding at most CL_PER to a field): phase 1 of 2 -- sixteen partial sums per word
CODON_FL_HD void cl_sum32(int tid, const unsigned* cnt, unsigned* part) {
  if (tid >= 32) return;
  unsigned s = 0;
  for (int q = 0; q < 16; ++q) s += cnt[tid * 16 + q];
  part[tid] = s;
}
// phase 2 of 2: thread `tid` < nfields adds field (tid & 1) of word (tid >> 1) to stats[tid]
template <class G>
CODON_FL_HD void cl_sum_add(G wg, int tid, int nfields, const unsigned* part, unsigned* stats) {
  if (tid >= nfields) return;
  unsigned s = 0;
  for (int q = 0; q < 16; ++q) s += (part[(tid >> 1) * 16 + q] >> (16 * (tid & 1))) & 0xFFFFu;
  if (s) wg.atomic_add(stats + tid, s);
}

// tile (ty, tx) of this image's plane `in` plus a halo of 1 into LDS; a cell outside the plane is 0, a hole, linked to nothing
template <int FMT>
CODON_FL_HD void cl_cells_load(int tid, const void* in, int h, int w, int ty, int tx, unsigned* cell) {
  for (int idx = tid; idx < CL_CELLS; idx += CL_THREADS) {
    const int i = idx / CL_HALO, j = idx - i * CL_HALO;
    const int y = ty * CL_TILE - 1 + i, x = tx * CL_TILE - 1 + j;
    cell[idx] = y >= 0 && y < h && x >= 0 && x < w ? (unsigned)fl_load<FMT>(in, (long)y * w + x, 0) : 0u;
  }
}

// one thread's pixel under rule 1: k to `out` (this image's plane), with rule 2 on its size word and its label word -- or, CL_LOCAL,
// k into kk[tid] and the tile-local label into loc[tid]; its packed counts (valid | flying << 16) into cnt[tid], 0 into
// cnt[CL_THREADS + tid]
template <int FMT>
CODON_FL_HD void cl_flying_pixel(int tid, const ClArgs& a, int ty, int tx, const unsigned* cell, void* out, unsigned* label,
                                 unsigned* size, unsigned* cnt, unsigned* kk, unsigned* loc) {
  const int li = tid / CL_TILE, lj = tid - li * CL_TILE;
  const int y = ty * CL_TILE + li, x = tx * CL_TILE + lj;
  unsigned word = 0;
  if (CL_LOCAL && label) {
    kk[tid] = 0u;                                  // a pixel outside the plane: a hole
    loc[tid] = CL_EMPTY;
  }
  if (y < a.h && x < a.w) {
    const int at = (li + 1) * CL_HALO + lj + 1;
    const unsigned c = cell[at];
    unsigned k = c;
    if (c != 0u && a.support > 0) {
      int n = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int q = 0; q < 9; ++q)
        if (q != 4) n += cl_linked(c, cell[at + (q / 3 - 1) * CL_HALO + q % 3 - 1], a.tol_abs, a.tol_rel);
      if (n < a.support) k = 0u;
    }
    const long p = (long)y * a.w + x;
    fl_store<FMT>(out, p, (int)k, nullptr);
    if (label) {
      if (CL_LOCAL) {
        kk[tid] = k;
        loc[tid] = k != 0u ? (unsigned)tid : CL_EMPTY;
      } else {
        label[p] = k != 0u ? (unsigned)p : CL_EMPTY;
      }
      size[p] = 0u;
    }
    word = (c != 0u) | ((unsigned)(c != 0u && k == 0u) << 16);
  }
  cnt[tid] = word;
  cnt[CL_THREADS + tid] = 0u;
}

// ---- the workgroup bodies -------------------------------------------------------------------------------------------------------

// one workgroup: the nstats statistics words to 0 (stats may be null)
template <class G>
CODON_FL_HD void wg_clean_zero(G wg, unsigned* stats, int nstats) {
  WG_EACH(wg, tid) {
    if (stats)
      for (int s = tid; s < nstats; s += CL_THREADS) stats[s] = 0u;
  }
}

// CL_LOCAL: one thread's links to the right and down INSIDE the tile, united on the tile-local labels in LDS
template <class G>
CODON_FL_HD void cl_local_link(G wg, int tid, const ClArgs& a, const unsigned* kk, unsigned* loc) {
  const int li = tid / CL_TILE, lj = tid - li * CL_TILE;
  const unsigned k = kk[tid];
  if (k == 0u) return;
  if (lj + 1 < CL_TILE && cl_linked(k, kk[tid + 1], a.tol_abs, a.tol_rel)) cl_unite(wg, loc, (unsigned)tid, (unsigned)tid + 1u);
  if (li + 1 < CL_TILE && cl_linked(k, kk[tid + CL_TILE], a.tol_abs, a.tol_rel))
    cl_unite(wg, loc, (unsigned)tid, (unsigned)(tid + CL_TILE));
}

// CL_LOCAL: one thread's label word: the index in the image of its tile-local root (row-major order inside a tile is the image's
// order, so the root's index is not above the pixel's own), all ones for a hole
template <class G>
CODON_FL_HD void cl_local_label(G wg, int tid, const ClArgs& a, int ty, int tx, const unsigned* kk, const unsigned* loc,
                                unsigned* label) {
  const int li = tid / CL_TILE, lj = tid - li * CL_TILE;
  const int y = ty * CL_TILE + li, x = tx * CL_TILE + lj;
  if (y >= a.h || x >= a.w) return;
  unsigned word = CL_EMPTY;
  if (kk[tid] != 0u) {
    const unsigned r = cl_find(wg, loc, (unsigned)tid);
    word = (unsigned)((long)(ty * CL_TILE + (int)(r / CL_TILE)) * a.w + tx * CL_TILE + (int)(r % CL_TILE));
  }
  label[(long)y * a.w + x] = word;
}

// workgroup (tx, ty, b) of grid (sx, sy, B).  ws: the workspace, read with rule 2 on alone.  LDS: cell CL_CELLS words, cnt
// 2 CL_THREADS, part 32, kk and loc CL_THREADS each (CL_LOCAL alone reads them).  stats (may be null): with rule 2 off the valid and flying counts are added here, to words an earlier
// launch zeroed; with rule 2 on tile (0, 0) zeroes the image's four, and wg_clean_apply adds them all
template <int FMT, class G>
CODON_FL_HD void wg_clean_flying(G wg, int tx, int ty, long b, int B, const void* in, const ClArgs& a, void* out, unsigned* ws,
                                 unsigned* stats, unsigned* cell, unsigned* cnt, unsigned* part, unsigned* kk, unsigned* loc) {
  const ClPlan p = cl_plan(a.h, a.w, a.region);
  const long plane = (long)a.h * a.w * fl_elem_bytes(FMT);
  unsigned* label = p.rule2 ? ws + b * p.stride : nullptr;
  unsigned* size = p.rule2 ? ws + (B + b) * p.stride : nullptr;
  WG_EACH(wg, tid) cl_cells_load<FMT>(tid, (const char*)in + b * plane, a.h, a.w, ty, tx, cell);
  wg.sync();
  WG_EACH(wg, tid) {
    cl_flying_pixel<FMT>(tid, a, ty, tx, cell, (char*)out + b * plane, label, size, cnt, kk, loc);
    if (p.rule2 && stats && tx == 0 && ty == 0 && tid < CL_STATS) stats[b * CL_STATS + tid] = 0u;
  }
  if (CL_LOCAL && p.rule2) {
    wg.sync();
    WG_EACH(wg, tid) cl_local_link(wg, tid, a, kk, loc);
    wg.sync();
    WG_EACH(wg, tid) cl_local_label(wg, tid, a, ty, tx, kk, loc, label);
  }
  if (p.rule2 || !stats) return;
  wg.sync();
  WG_EACH(wg, tid) cl_sum32(tid, cnt, part);
  wg.sync();
  WG_EACH(wg, tid) cl_sum_add(wg, tid, 2, part, stats + b * CL_STATS);      // CL_VALID, CL_FLYING
}

// workgroup (tx, ty, b) of grid (sx, sy, B), rule 2 on: k is read from `out`; no LDS.  CL_LOCAL: the links that leave the tile alone,
// those of its last column to the right and of its last row downwards
template <int FMT, class G>
CODON_FL_HD void wg_clean_link(G wg, int tx, int ty, long b, const void* out, const ClArgs& a, unsigned* ws) {
  const ClPlan p = cl_plan(a.h, a.w, a.region);
  const long n = (long)a.h * a.w;
  unsigned* label = ws + b * p.stride;
  WG_EACH(wg, tid) {
    const int li = tid / CL_TILE, lj = tid - li * CL_TILE;
    const int y = ty * CL_TILE + li, x = tx * CL_TILE + lj;
    const bool right = !CL_LOCAL || lj == CL_TILE - 1, down = !CL_LOCAL || li == CL_TILE - 1;
    if (y < a.h && x < a.w && (right || down)) {
      const long at = (long)y * a.w + x;
      const unsigned k = (unsigned)fl_load<FMT>(out, b * n + at, 0);
      if (k != 0u) {
        if (right && x + 1 < a.w && cl_linked(k, (unsigned)fl_load<FMT>(out, b * n + at + 1, 0), a.tol_abs, a.tol_rel))
          cl_unite(wg, label, (unsigned)at, (unsigned)(at + 1));
        if (down && y + 1 < a.h && cl_linked(k, (unsigned)fl_load<FMT>(out, b * n + at + a.w, 0), a.tol_abs, a.tol_rel))
          cl_unite(wg, label, (unsigned)at, (unsigned)(at + a.w));
      }
    }
  }
}

// workgroup (tx, ty, b) of grid (sx, sy, B), rule 2 on.  LDS: root CL_THREADS words
template <class G>
CODON_FL_HD void wg_clean_count(G wg, int tx, int ty, long b, int B, const ClArgs& a, unsigned* ws, unsigned* root) {
  const ClPlan p = cl_plan(a.h, a.w, a.region);
  unsigned* label = ws + b * p.stride;
  unsigned* size = ws + (B + b) * p.stride;
  WG_EACH(wg, tid) {
    const int li = tid / CL_TILE, lj = tid - li * CL_TILE;
    const int y = ty * CL_TILE + li, x = tx * CL_TILE + lj;
    unsigned r = CL_EMPTY;
    if (y < a.h && x < a.w) {
      const long at = (long)y * a.w + x;
      if (label[at] != CL_EMPTY) {                 // a non-zero pixel of k: its own index or an ancestor's
        r = cl_find(wg, label, (unsigned)at);
        label[at] = r;                             // the tree flattened: another thread's find through here sees either ancestor
      }
    }
    root[tid] = r;
  }
  wg.sync();
  WG_EACH(wg, tid) {
    const int lj = tid % CL_TILE;
    const unsigned r = root[tid];
    if (r != CL_EMPTY && (lj == 0 || root[tid - 1] != r)) {           // the head of a run of one root in this row of the tile
      unsigned run = 1;
      while (lj + (int)run < CL_TILE && root[tid + run] == r) ++run;
      if (wg.load_relaxed(size + r) < (unsigned)a.region) wg.atomic_add(size + r, run);
    }
  }
}

// workgroup (r, b) of grid (rx, B), rule 2 on: CL_RUN pixels of image b, in place in `out`.  LDS: cnt 2 CL_THREADS words, part 32
template <int FMT, class G>
CODON_FL_HD void wg_clean_apply(G wg, long r, long b, int B, const void* in, const ClArgs& a, void* out, const unsigned* ws,
                                unsigned* stats, unsigned* cnt, unsigned* part) {
  const ClPlan p = cl_plan(a.h, a.w, a.region);
  const long n = (long)a.h * a.w;
  const unsigned* label = ws + b * p.stride;
  const unsigned* size = ws + (B + b) * p.stride;
  WG_EACH(wg, tid) {
    unsigned first = 0, second = 0;                // valid | flying << 16, speckle | regions << 16
    for (int q = 0; q < CL_PER; ++q) {
      const long at = r * CL_RUN + q * CL_THREADS + tid;
      if (at < n) {
        const unsigned k = (unsigned)fl_load<FMT>(out, b * n + at, 0);
        if (k != 0u) {
          const unsigned root = label[at];
          if (root <= (unsigned)at && size[root] < (unsigned)a.region) {
            fl_store<FMT>(out, b * n + at, 0, nullptr);
            second += 1u + ((unsigned)(root == (unsigned)at) << 16);
          }
        }
        if (stats) {
          const unsigned c = (unsigned)fl_load<FMT>(in, b * n + at, 0);
          first += (c != 0u) + ((unsigned)(c != 0u && k == 0u) << 16);
        }
      }
    }
    cnt[tid] = first;
    cnt[CL_THREADS + tid] = second;
  }
  if (!stats) return;
  wg.sync();
  WG_EACH(wg, tid) cl_sum32(tid, cnt, part);
  wg.sync();
  WG_EACH(wg, tid) cl_sum_add(wg, tid, CL_STATS, part, stats + b * CL_STATS);
}

}  // namespace codon
