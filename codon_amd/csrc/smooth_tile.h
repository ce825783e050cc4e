// The spatial, edge-preserving smoothing of sensor depth maps (smooth.hip): its one workgroup body (wg_smooth, over
// wg.h's group type: DESIGN 12.13) and the per-thread phases it runs, written like clean_tile.h so that the SAME text compiles for
// the device and for a plain host compiler: the kernel and tools/smooth_host_check.cpp, under the address and undefined-behaviour
// sanitizers, call the same body.  Integers only.
//
// The definition (tests/smooth_ref.py).  One pass c -> c': a hole (0) stays 0.  For a valid pixel p the window is the (2R+1)^2
// positions around it, R = 1 .. 4; S is the set of positions q != p inside the plane that are LINKED to c_p (cl_linked of
// clean_tile.h, the one text: both non-zero, codes at most tol_abs + ((tol_rel min) >> 16) apart), every code read from the pass's
// input; with the PAIR RULE q stays in S only if its mirror 2p - q is in S too.  N = 256 c_p + sum_S W_q c_q, D = 256 + sum_S W_q,
// c' = (2N + D) / (2D) rounded down: the weighted mean, half rounded up.  W: the caller's (2R+1)^2 table, every entry 0 .. 256, the
// centre 256, symmetric under q -> 2p - q, so that a pair shares one entry.  P = 1 .. 3 passes compose; a pixel outside the plane is
// a hole in every pass.
//
// THE BOUND: N <= 256 * 65535 * 81 = 1358933760, so 2N + D <= 2717867520 + 20736 < 2^32: unsigned 32-bit arithmetic throughout.
// Consequences: c' >= 1 (a mean of codes >= 1, rounded), so the hole set never changes; every member of S is within
// tau(c_p) = tol_abs + ((tol_rel c_p) >> 16) of c_p, and so is c'; under the pair rule the members of a pair on a plane with an
// integer gradient sum to 2 c_p, N = c_p D, and c' = c_p exactly, however holes, an occluder or the border cut the window.
//
// Statistics per image: valid inputs; pixels whose final code differs from the input; valid pixels whose S is empty in the FIRST
// pass; the largest |final - input|.
//
// A launch runs `fused` passes (launch_rules.h's rule of (R, P)) on one SM_TILE x SM_TILE tile of one image: the tile plus a halo
// of R * fused goes into LDS as 16-bit cells, u8 and u16 codes alike, a cell outside the plane 0 -- a hole, linked to nothing,
// which is the rule "inside the plane"; pass j of the launch computes the tile plus a halo of R * (fused - j) from one LDS plane
// into the other, the last one the tile itself into `out`.  A pair is two link tests and one decision: half the window is walked.
#pragma once

#include "clean_tile.h"

namespace codon {

constexpr int SM_TILE = 32, SM_THREADS = 256, SM_PER = SM_TILE * SM_TILE / SM_THREADS;      // four pixels per thread
constexpr int SM_MAX_RADIUS = 4, SM_MAX_PASSES = 3;
constexpr int SM_MAX_TAPS = (2 * SM_MAX_RADIUS + 1) * (2 * SM_MAX_RADIUS + 1);              // 81
constexpr int SM_WEIGHT_ONE = 256;
constexpr int SM_MAX_SIDE = CL_MAX_SIDE, SM_MAX_REL = CL_MAX_REL;
constexpr int SM_VALID = 0, SM_CHANGED = 1, SM_ALONE = 2, SM_MAX = 3, SM_STATS = 4;
static_assert(SM_THREADS == CL_THREADS, "wg_smooth sums its counts with clean_tile.h's cl_sum32 and cl_sum_add");
static_assert(2ull * SM_WEIGHT_ONE * 65535 * SM_MAX_TAPS + (unsigned long long)SM_WEIGHT_ONE * SM_MAX_TAPS < (1ull << 32), "2N + D");

struct SmArgs {
  int h, w, radius, pairs;
  unsigned tol_abs, tol_rel;       // A, and Rq = rint(65536 rel)
  int fused;                       // the passes of THIS launch, 1 .. SM_MAX_PASSES
  int first, last;                 // this launch holds the first pass (the `alone` count) / the last (the other three)
};

// the row stride of the LDS planes at radius R: the span of the most passes a launch can run, a compile-time constant, so that
// every tap is the centre's address plus a constant
template <int R>
constexpr int sm_stride() { return SM_TILE + 2 * R * SM_MAX_PASSES; }

// one pixel of one pass: the cell at `at` of the LDS plane `src` (row stride sm_stride<R>()), every tap inside the plane's cells.
// *any: whether S holds a position.  The window is unrolled: 4, 12, 24 or 40 pairs
template <int R>
CODON_FL_HD unsigned sm_pixel(const SmArgs& a, const int* wtab, const unsigned short* src, int at, bool* any) {
  constexpr int side = 2 * R + 1, stride = sm_stride<R>();
  const unsigned c = src[at];
  *any = false;
  if (c == 0u) return 0u;
  unsigned N = (unsigned)SM_WEIGHT_ONE * c, D = (unsigned)SM_WEIGHT_ONE;
  bool some = false;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int t = 0; t < side * side / 2; ++t) {        // the taps before the centre in row-major order; their mirrors come after it
    const int dy = t / side - R, dx = t % side - R;
    const unsigned W = (unsigned)wtab[t];
    const int off = dy * stride + dx;
    const unsigned c1 = src[at + off], c2 = src[at - off];
    bool l1 = cl_linked(c, c1, a.tol_abs, a.tol_rel), l2 = cl_linked(c, c2, a.tol_abs, a.tol_rel);
    if (a.pairs) l1 = l2 = l1 && l2;
    if (l1) N += W * c1, D += W;
    if (l2) N += W * c2, D += W;
    some = some || l1 || l2;
  }
  *any = some;
  return (2u * N + D) / (2u * D);
}

// workgroup (tx, ty, b) of grid (ceil(w / SM_TILE), ceil(h / SM_TILE), B).  in: this launch's input planes; orig: the call's input
// planes (read where a.last and stats); out: this launch's output planes.  wtab: (2R+1)^2 weights.  stats (may be null): (B, 4)
// words an earlier launch zeroed.  R: a.radius.  LDS: pa and pb sm_stride<R>()^2 cells each (the rows a launch of fewer passes
// uses are shorter and fewer; the stride stays), cnt 2 SM_THREADS words, part 32, mx SM_THREADS, pmx 16
template <int FMT, int R, class G>
CODON_FL_HD void wg_smooth(G wg, int tx, int ty, long b, const void* in, const void* orig, const SmArgs& a, const int* wtab, void* out,
                           unsigned* stats, unsigned short* pa, unsigned short* pb, unsigned* cnt, unsigned* part, unsigned* mx,
                           unsigned* pmx) {
  constexpr int stride = sm_stride<R>();
  const int k = a.fused, span = SM_TILE + 2 * R * k;
  const int y0 = ty * SM_TILE - R * k, x0 = tx * SM_TILE - R * k;
  const long plane = (long)a.h * a.w;
  const char* src_plane = (const char*)in + b * plane * fl_elem_bytes(FMT);
  WG_EACH(wg, tid) {
    for (int idx = tid; idx < span * span; idx += SM_THREADS) {
      const int i = idx / span, j = idx - i * span;
      const int y = y0 + i, x = x0 + j;
      pa[i * stride + j] = y >= 0 && y < a.h && x >= 0 && x < a.w ? (unsigned short)fl_load<FMT>(src_plane, (long)y * a.w + x, 0) : (unsigned short)0;
    }
    cnt[tid] = 0u;
    cnt[SM_THREADS + tid] = 0u;
  }
  wg.sync();
  unsigned short* from = pa;
  unsigned short* to = pb;
  for (int pass = 1; pass < k; ++pass) {           // the tile plus a halo of R (k - pass), LDS to LDS
    const int lo = R * pass, m = span - 2 * lo;
    WG_EACH(wg, tid) {
      unsigned alone = 0;
      for (int idx = tid; idx < m * m; idx += SM_THREADS) {
        const int i = idx / m, j = idx - i * m;
        const int at = (lo + i) * stride + lo + j;
        bool any;
        const unsigned v = sm_pixel<R>(a, wtab, from, at, &any);
        to[at] = (unsigned short)v;
        const int li = lo + i - R * k, lj = lo + j - R * k;          // the cell's place in the tile proper
        if (pass == 1 && v != 0u && !any && li >= 0 && li < SM_TILE && lj >= 0 && lj < SM_TILE) ++alone;
      }
      if (pass == 1 && a.first && stats) cnt[SM_THREADS + tid] = alone;
    }
    wg.sync();
    unsigned short* t = from;
    from = to;
    to = t;
  }
  WG_EACH(wg, tid) {                               // the last pass of the launch: the tile itself, to `out`
    unsigned first = 0, second = cnt[SM_THREADS + tid], big = 0;
    for (int q = 0; q < SM_PER; ++q) {
      const int idx = q * SM_THREADS + tid;
      const int li = idx / SM_TILE, lj = idx - li * SM_TILE;
      const int y = ty * SM_TILE + li, x = tx * SM_TILE + lj;
      if (y >= a.h || x >= a.w) continue;
      bool any;
      const unsigned v = sm_pixel<R>(a, wtab, from, (R * k + li) * stride + R * k + lj, &any);
      const long p = b * plane + (long)y * a.w + x;
      fl_store<FMT>(out, p, (int)v, nullptr);
      if (!stats) continue;
      if (a.first && k == 1 && v != 0u && !any) ++second;
      if (a.last) {
        const unsigned c = (unsigned)fl_load<FMT>(orig, p, 0);
        const unsigned d = c < v ? v - c : c - v;
        first += (c != 0u) + ((unsigned)(d != 0u) << 16);
        big = d > big ? d : big;
      }
    }
    cnt[tid] = first;
    cnt[SM_THREADS + tid] = second;
    mx[tid] = big;
  }
  if (!stats) return;
  wg.sync();
  WG_EACH(wg, tid) {
    cl_sum32(tid, cnt, part);
    if (tid < 16) {
      unsigned m = 0;
      for (int q = 0; q < 16; ++q) m = mx[tid * 16 + q] > m ? mx[tid * 16 + q] : m;
      pmx[tid] = m;
    }
  }
  wg.sync();
  WG_EACH(wg, tid) {
    cl_sum_add(wg, tid, 3, part, stats + b * SM_STATS);              // SM_VALID, SM_CHANGED, SM_ALONE
    if (tid == SM_MAX) {
      unsigned m = 0;
      for (int q = 0; q < 16; ++q) m = pmx[q] > m ? pmx[q] : m;
      if (m) wg.atomic_max(stats + b * SM_STATS + SM_MAX, m);
    }
  }
}

}  // namespace codon
