// The workgroup body of the surface-normal angle error (normal_errors.hip; wg_normal_errors, over wg.h's group type:
// DESIGN 12.13) and the per-thread phases it runs, written like eval_tile.h so that the SAME text compiles for the device and for a
// plain host compiler: the kernel and tools/normal_errors_host_check.cpp, under the address and undefined-behaviour sanitizers,
// call the same body.  Integers only, but for the estimates of a root and of a reciprocal that cloud_tile.h corrects in integers.
//
// The definition (tests/normal_errors_ref.py).  Inside the H x W window the output counts as 0 wherever the label is 0, and both
// planes count as 0 outside the window: both normals see one hole set.  N_l = cd_normal of the label, N_o = cd_normal of the masked
// output (cloud_tile.h's text, Q14, facing the camera); a pixel is COMPARED when its label code is non-zero and both planes have a
// normal there.  For a compared pixel D = N_l . N_o (|D| < 2^29), X = |N_l x N_o|^2 (each component below 2^29, the sum below
// 2^60), A = cd_isqrt(X), and with C[m] = rint(2^30 cos t_m), S[m] = rint(2^30 sin t_m), t_m = (m - 1/2) / 8 degrees, m = 1 .. 1440,
// the index is a = #{ m : A C[m] - D S[m] > 0 } = rint(8 angle in degrees), 0 .. 1440: the predicate changes sign once in m, so
// ne_index bisects in 11 steps; every product stays below 2^61.
// Per image NE_WORDS u32 words: 0 .. 1440 the histogram of a over the compared pixels, 1441 valid label pixels in the window, 1442
// those whose label has a normal, 1443 compared pixels, 1444 pixels with label != 0 and output = 0, 1445 .. 1447 zero.  The angle
// map: a where the pixel is compared, 65535 elsewhere.
//
// A workgroup of NE_THREADS threads owns one NE_TILE x NE_TILE tile of one image's window and runs three phases with a workgroup
// barrier between them:
//   1 load    the label tile plus a halo of R = radius codes into `lab`, the output through the mask into `outm` (the mask is
//             applied once), the tile's slices of RX and RY, both angle tables, and the histogram's zeros
//   2 pixel   the label's normal; the output's, only if the label has one; the index; an LDS atomic add; the map's texel; the four
//             counts into the THREAD's words
//   3 flush   the non-zero bins to the image's row, one global u32 atomic add each: integer adds, so the row does not depend on
//             the order of arrival
// LDS coordinates: lab[ly side + lx], side = NE_TILE + 2 R, is window position (i0 - R + ly, j0 - R + lx); rxs[lx] and rys[ly] are
// the rays of those columns and rows.  cd_normal runs in THESE coordinates, on a side x side plane: a position outside the window
// is code 0 there, which links to nothing, exactly as a position outside the plane does for cloud.
#pragma once

#include "cloud_tile.h"

namespace codon {

constexpr int NE_TILE = 32;
constexpr int NE_THREADS = 256;
constexpr int NE_RMAX = CD_MAX_RADIUS;
constexpr int NE_SIDE = NE_TILE + 2 * NE_RMAX;                 // 48: a tile and its halo
constexpr int NE_ANGLES = 1440;                                // thresholds, an eighth of a degree apart
constexpr int NE_BINS = NE_ANGLES + 1;
constexpr int NE_WORDS = 1448;
constexpr int NE_COUNTS = 4;                                   // words NE_BINS .. NE_BINS + 3
constexpr int NE_MAX_SIDE = CD_MAX_SIDE;
constexpr unsigned short NE_NONE = 65535;                      // the map's texel of a pixel that is not compared

struct NeArgs {
  int H, W;                        // the output's size = the window
  long label_row, label_image;     // the label's row stride and image stride, in elements
  int radius;                      // R, 1 .. NE_RMAX
  unsigned tol_abs, tol_rel;       // R A, and Rq: cloud's link parameters
};

CODON_FL_HD int ne_tiles(int n) { return (n + NE_TILE - 1) / NE_TILE; }        // the grid is (ne_tiles(W), ne_tiles(H), B)

// the loader cd_normal reads a tile in LDS through
template <typename T>
struct NeTile {
  const T* t;
  CODON_FL_HD unsigned operator()(long at) const { return (unsigned)t[at]; }
};

// the angle index of two Q14 normals p and q (|p_c|, |q_c| <= 16384): rint(8 atan2(|p x q|, p . q) in degrees), 0 .. 1440.
// cosine and sine: the NE_ANGLES entries C[m - 1], S[m - 1] of threshold m.  The greedy descent finds the largest m whose
// predicate holds, given that it holds for every smaller m and for no larger one
CODON_FL_HD int ne_index(const int* p, const int* q, const int* cosine, const int* sine) {
  const long long D = (long long)(p[0] * q[0] + p[1] * q[1] + p[2] * q[2]);                  // three products of at most 2^28
  const long long x = p[1] * q[2] - p[2] * q[1], y = p[2] * q[0] - p[0] * q[2], z = p[0] * q[1] - p[1] * q[0];
  const long long A = cd_isqrt(x * x + y * y + z * z);
  int a = 0;
  for (int step = 1024; step >= 1; step >>= 1) {
    const int m = a + step;
    if (m <= NE_ANGLES && A * cosine[m - 1] - D * sine[m - 1] > 0) a = m;
  }
  return a;
}

// phase 1
template <typename T>
CODON_FL_HD void ne_load(const NeArgs& a, int tid, int i0, int j0, const T* label, const T* out, const int* rx, const int* ry,
                         const int* ctab, const int* stab, T* lab, T* outm, int* rxs, int* rys, int* cosine, int* sine,
                         unsigned* hist) {
  const int R = a.radius, side = NE_TILE + 2 * R;
  for (int idx = tid; idx < side * side; idx += NE_THREADS) {
    const int ly = idx / side, lx = idx - ly * side;
    const int y = i0 - R + ly, x = j0 - R + lx;
    T l = 0, o = 0;
    if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
      l = label[(long)y * a.label_row + x];
      o = l != 0 ? out[(long)y * a.W + x] : (T)0;
    }
    lab[idx] = l;
    outm[idx] = o;
  }
  for (int idx = tid; idx < side; idx += NE_THREADS) {
    const int y = i0 - R + idx, x = j0 - R + idx;
    rxs[idx] = x >= 0 && x < a.W ? rx[x] : 0;
    rys[idx] = y >= 0 && y < a.H ? ry[y] : 0;
  }
  for (int idx = tid; idx < NE_ANGLES; idx += NE_THREADS) cosine[idx] = ctab[idx], sine[idx] = stab[idx];
  for (int idx = tid; idx < NE_BINS; idx += NE_THREADS) hist[idx] = 0u;
}

// phase 2: the thread's pixels of the tile; c[] += its share of the four counts.  amap: this image's (H, W) map, or null
template <typename T, class G>
CODON_FL_HD void ne_pixels(G wg, const NeArgs& a, int tid, int i0, int j0, const T* lab, const T* outm, const int* rxs,
                           const int* rys, const int* cosine, const int* sine, unsigned* hist, unsigned short* amap, unsigned* c) {
  const int R = a.radius, side = NE_TILE + 2 * R;
  CdArgs ca;
  ca.h = side, ca.w = side, ca.radius = R, ca.tol_abs = a.tol_abs, ca.tol_rel = a.tol_rel, ca.channels = 0, ca.m = 0.0;
  const int tx = tid % NE_TILE, ty = tid / NE_TILE;
  const int x = j0 + tx;
  for (int yy = ty; yy < NE_TILE; yy += NE_THREADS / NE_TILE) {
    const int y = i0 + yy;
    if (y >= a.H || x >= a.W) continue;
    const int li = yy + R, lj = tx + R;
    const unsigned l = lab[li * side + lj];
    unsigned short texel = NE_NONE;
    if (l != 0u) {
      const unsigned o = outm[li * side + lj];
      int Nl[3], No[3];
      c[0] += 1u;
      c[3] += o == 0u ? 1u : 0u;
      if (cd_normal(NeTile<T>{lab}, ca, rxs, rys, li, lj, l, Nl)) {
        c[1] += 1u;
        if (o != 0u && cd_normal(NeTile<T>{outm}, ca, rxs, rys, li, lj, o, No)) {
          const int bin = ne_index(Nl, No, cosine, sine);
          c[2] += 1u;
          wg.lds_add(hist + bin, 1u);
          texel = (unsigned short)bin;
        }
      }
    }
    if (amap) amap[(long)y * a.W + x] = texel;
  }
}

// workgroup (bx, by, b) of grid (ne_tiles(W), ne_tiles(H), B): one tile of image b.  label / out / amap: the batches, amap may be
// null; rx (W), ry (H): the rays; ctab, stab: the NE_ANGLES entries of each table; words: (B, NE_WORDS), zeroed by the entry.  LDS:
// lab and outm NE_SIDE^2 codes each, rxs and rys NE_SIDE, cosine and sine NE_ANGLES, hist NE_BINS.  c: the threads' four counts of
// this tile, for the caller to fold into words NE_BINS .. NE_BINS + 3
template <typename T, class G>
CODON_FL_HD void wg_normal_errors(G wg, int bx, int by, int b, const NeArgs& a, const T* label, const T* out, const int* rx,
                                  const int* ry, const int* ctab, const int* stab, unsigned* words, unsigned short* amap, T* lab,
                                  T* outm, int* rxs, int* rys, int* cosine, int* sine, unsigned* hist,
                                  typename G::template Regs<unsigned, NE_COUNTS>& c) {
  const int i0 = by * NE_TILE, j0 = bx * NE_TILE;
  const long hw = (long)a.H * a.W;
  WG_EACH(wg, tid)
    ne_load<T>(a, tid, i0, j0, label + b * a.label_image, out + b * hw, rx, ry, ctab, stab, lab, outm, rxs, rys, cosine, sine, hist);
  wg.sync();
  WG_EACH(wg, tid) {
    for (int k = 0; k < NE_COUNTS; ++k) c[tid][k] = 0u;
    ne_pixels<T>(wg, a, tid, i0, j0, lab, outm, rxs, rys, cosine, sine, hist, amap ? amap + b * hw : nullptr, c[tid]);
  }
  wg.sync();
  WG_EACH(wg, tid) {
    for (int bin = tid; bin < NE_BINS; bin += NE_THREADS) {
      const unsigned v = hist[bin];
      if (v != 0u) wg.atomic_add(words + (long)b * NE_WORDS + bin, v);
    }
  }
}

}  // namespace codon
