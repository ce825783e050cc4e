// The depth registration (register.hip): its launch plan (rg_plan), its three workgroup bodies (wg_register_init,
// wg_register_splat, wg_register_resolve, over wg.h's group type: DESIGN 12.13) and the per-thread phases they run, written like
// jbu_tile.h so that the SAME text compiles for the device and for a plain host compiler: the kernels and
// tools/register_host_check.cpp, under the address and undefined-behaviour sanitizers, call the same bodies.  Integers only,
// except the estimate of a quotient, which is corrected in integers (rg_floor_div).
//
// The definition (tests/register_ref.py): a valid source pixel (i, j) with code k has the corners a = (i, j), b = (i + 1, j + 1),
// c = (i, j + 1), d = (i + 1, j) of the corner-ray table A (Q20, |A| < 2^22); P_q = k A[q] + T in Q20 codes (|T| < 2^38).  Any
// P_q.z < 2^20: dropped.  z' = (((P_a.z + P_b.z + 1) >> 1) + 2^19) >> 20, dropped unless 1 <= z' <= top.
// U_q = floor((FX P_q.x + CX P_q.z) / P_q.z) and V_q likewise, Q8 pixels (0 < FX, FY < 2^20, |CX|, |CY| < 2^21: every intermediate
// below 2^61, |U| < 2^41).  Footprint: x0 = (min U + 255) >> 8 .. x1 = ((max U + 255) >> 8) - 1, y likewise; wider or taller than
// RG_FOOT: dropped; empty: nothing; wholly outside the plane: counted; else clipped, and every pixel takes min(zbuf, z').
//
// Three launches, a function of the shapes alone:
//   wg_register_init      RG_RUN u32 words of the z-buffer planes to all ones per workgroup; workgroup 0 zeroes the statistics
//   wg_register_splat     one RG_TILE x RG_TILE tile of source pixels of one image: the tile's 17 x 17 x 3 corner rays into LDS, one
//                         barrier, one pixel per thread (eight exact floor divisions, the footprint loop of atomic minima), the
//                         three counts of the workgroup summed through LDS, one atomic add per count that is not 0
//   wg_register_resolve   RG_RUN target pixels of one image: z-buffer -> codes (all ones -> 0), the filled count likewise
#pragma once

#include "fill_tile.h"

namespace codon {

constexpr int RG_TILE = 16, RG_THREADS = RG_TILE * RG_TILE;         // 256: one source pixel per thread
constexpr int RG_CORNERS = (RG_TILE + 1) * (RG_TILE + 1);           // 289 corners of 3 words
constexpr int RG_FOOT = 8;
constexpr int RG_PER = 4, RG_RUN = RG_THREADS * RG_PER;             // init and resolve: four words per thread
constexpr int RG_MAX_SIDE = FL_MAX_SIDE;
constexpr unsigned RG_EMPTY = 0xFFFFFFFFu;
constexpr long long RG_ONE = 1ll << 20;
constexpr long long RG_T_LIMIT = 1ll << 38;
constexpr int RG_F_LIMIT = 1 << 20, RG_C_LIMIT = 1 << 21;
constexpr int RG_VALID = 0, RG_OUTSIDE = 1, RG_DROPPED = 2, RG_FILLED = 3, RG_STATS = 4;

// The launches of B planes of hs x ws onto ho x wo: the splat body over sx x sy tiles per image, the resolve body over rx runs per
// image, the init body over `init` runs of all B planes (images `stride` words apart in the workspace, 16 bytes a multiple)
struct RgPlan {
  int sx, sy, rx;
  long stride;
};
CODON_FL_HD RgPlan rg_plan(int hs, int ws, int ho, int wo) {
  RgPlan p;
  p.sx = (ws + RG_TILE - 1) / RG_TILE;
  p.sy = (hs + RG_TILE - 1) / RG_TILE;
  p.rx = (int)(((long)ho * wo + RG_RUN - 1) / RG_RUN);
  p.stride = ((long)ho * wo + 3) / 4 * 4;
  return p;
}
CODON_FL_HD long rg_init_runs(const RgPlan& p, int B) { return (p.stride * B + RG_RUN - 1) / RG_RUN; }

struct RgArgs {
  long long tx, ty, tz;            // T, Q20 codes
  int fx, fy, cx, cy;              // the projection, Q8 pixels
  int hs, ws, ho, wo, top;
};

// floor(num / den) for 2^20 <= den < 2^40 and |num| < 2^61, a quotient below 2^41 in magnitude: the fp64 estimate is off by less
// than 2^41 * 3 * 2^-53, its floor by at most one, which one step either way in integers sets right
CODON_FL_HD long long rg_floor_div(long long num, long long den) {
  long long q = (long long)floor((double)num / (double)den);
  long long r = num - q * den;
  if (r < 0) {
    --q;
    r += den;
  }
  if (r >= den) ++q;
  return q;
}

// the sum over the workgroup of one packed word per thread (three fields of 10 bits, each thread adding at most 1 to a field, or
// one count up to RG_PER): phase 1 of 2 -- sixteen partial sums
CODON_FL_HD void rg_sum16(int tid, const unsigned* cnt, unsigned* part) {
  if (tid >= 16) return;
  unsigned s = 0;
  for (int q = 0; q < 16; ++q) s += cnt[tid * 16 + q];
  part[tid] = s;
}

// the corner rays of source tile (ty, tx) into LDS; a corner beyond the table (a tile that overhangs the plane) reads the last
CODON_FL_HD void rg_rays_load(int tid, const int* rays, int hs, int ws, int ty, int tx, int* la) {
  for (int idx = tid; idx < RG_CORNERS; idx += RG_THREADS) {
    const int i = idx / (RG_TILE + 1), j = idx - i * (RG_TILE + 1);
    const int y = ty * RG_TILE + i, x = tx * RG_TILE + j;
    const long at = ((long)(y < hs ? y : hs) * (ws + 1) + (x < ws ? x : ws)) * 3;
    la[idx * 3 + 0] = rays[at + 0];
    la[idx * 3 + 1] = rays[at + 1];
    la[idx * 3 + 2] = rays[at + 2];
  }
}

// one thread's source pixel: its code from `in` (this image's hs x ws plane), the atomic minima into `zb` (this image's ho x wo
// words), its packed counts (valid | outside << 10 | dropped << 20) into cnt[tid]
template <int FMT, class G>
CODON_FL_HD void rg_pixel(G wg, int tid, const void* in, const RgArgs& a, int ty, int tx, const int* la, unsigned* zb, unsigned* cnt) {
  const int li = tid / RG_TILE, lj = tid - li * RG_TILE;
  const int i = ty * RG_TILE + li, j = tx * RG_TILE + lj;
  unsigned word = 0;
  if (i < a.hs && j < a.ws) {
    const long long k = fl_load<FMT>(in, (long)i * a.ws + j, 0);
    if (k != 0) {
      word = 1u;                                                     // valid
      const int corner[4] = {li * (RG_TILE + 1) + lj, (li + 1) * (RG_TILE + 1) + lj + 1, li * (RG_TILE + 1) + lj + 1,
                             (li + 1) * (RG_TILE + 1) + lj};          // a, b, c, d
      long long px[4], py[4], pz[4];
      bool front = true;
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int q = 0; q < 4; ++q) {
        px[q] = k * la[corner[q] * 3 + 0] + a.tx;
        py[q] = k * la[corner[q] * 3 + 1] + a.ty;
        pz[q] = k * la[corner[q] * 3 + 2] + a.tz;
        front = front && pz[q] >= RG_ONE;
      }
      const long long z = front ? (((pz[0] + pz[1] + 1) >> 1) + (RG_ONE >> 1)) >> 20 : 0;
      if (!front || z < 1 || z > a.top) {
        word = 1u | (1u << 20);                                      // dropped: behind the camera or off the grid
      } else {
        long long u0 = 0, u1 = 0, v0 = 0, v1 = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int q = 0; q < 4; ++q) {
          const long long u = rg_floor_div(a.fx * px[q] + a.cx * pz[q], pz[q]);
          const long long v = rg_floor_div(a.fy * py[q] + a.cy * pz[q], pz[q]);
          u0 = q == 0 || u < u0 ? u : u0;
          u1 = q == 0 || u > u1 ? u : u1;
          v0 = q == 0 || v < v0 ? v : v0;
          v1 = q == 0 || v > v1 ? v : v1;
        }
        long long x0 = (u0 + 255) >> 8, x1 = ((u1 + 255) >> 8) - 1;
        long long y0 = (v0 + 255) >> 8, y1 = ((v1 + 255) >> 8) - 1;
        if (x1 - x0 + 1 > RG_FOOT || y1 - y0 + 1 > RG_FOOT) {
          word = 1u | (1u << 20);                                    // dropped: an oversize footprint
        } else if (x1 >= x0 && y1 >= y0) {
          if (x1 < 0 || x0 >= a.wo || y1 < 0 || y0 >= a.ho) {
            word = 1u | (1u << 10);                                  // outside
          } else {
            x0 = x0 < 0 ? 0 : x0;
            y0 = y0 < 0 ? 0 : y0;
            x1 = x1 > a.wo - 1 ? a.wo - 1 : x1;
            y1 = y1 > a.ho - 1 ? a.ho - 1 : y1;
            for (int y = (int)y0; y <= (int)y1; ++y)
              for (int x = (int)x0; x <= (int)x1; ++x) wg.atomic_min(zb + (long)y * a.wo + x, (unsigned)z);
          }
        }
      }
    }
  }
  cnt[tid] = word;
}

// ---- the workgroup bodies -------------------------------------------------------------------------------------------------------

// workgroup r of grid (rg_init_runs): words [r RG_RUN, (r + 1) RG_RUN) of the `words` of the workspace to all ones; workgroup 0
// also zeroes the nstats statistics words (stats may be null)
template <class G>
CODON_FL_HD void wg_register_init(G wg, long r, unsigned* zb, long words, unsigned* stats, int nstats) {
  WG_EACH(wg, tid) {
    for (int q = 0; q < RG_PER; ++q) {
      const long at = r * RG_RUN + q * RG_THREADS + tid;
      if (at < words) zb[at] = RG_EMPTY;
    }
    if (r == 0 && stats)
      for (int s = tid; s < nstats; s += RG_THREADS) stats[s] = 0u;
  }
}

// workgroup (tx, ty, b) of grid (sx, sy, B): one tile of source pixels.  LDS: la 3 RG_CORNERS ints, cnt RG_THREADS words, part 16
template <int FMT, class G>
CODON_FL_HD void wg_register_splat(G wg, int tx, int ty, long b, const void* in, const int* rays, const RgArgs& a, unsigned* zb,
                                   long zb_stride, unsigned* stats, int* la, unsigned* cnt, unsigned* part) {
  const long plane = (long)a.hs * a.ws * fl_elem_bytes(FMT);
  WG_EACH(wg, tid) rg_rays_load(tid, rays, a.hs, a.ws, ty, tx, la);
  wg.sync();
  WG_EACH(wg, tid) rg_pixel<FMT>(wg, tid, (const char*)in + b * plane, a, ty, tx, la, zb + b * zb_stride, cnt);
  if (!stats) return;
  wg.sync();
  WG_EACH(wg, tid) rg_sum16(tid, cnt, part);
  wg.sync();
  WG_EACH(wg, tid) {
    if (tid < 3) {                                                   // RG_VALID, RG_OUTSIDE, RG_DROPPED
      unsigned s = 0;
      for (int q = 0; q < 16; ++q) s += (part[q] >> (10 * tid)) & 1023u;
      if (s) wg.atomic_add(stats + b * RG_STATS + tid, s);
    }
  }
}

// workgroup (r, b) of grid (rx, B): RG_RUN target pixels of image b.  LDS: cnt RG_THREADS words, part 16
template <int FMT, class G>
CODON_FL_HD void wg_register_resolve(G wg, long r, long b, const unsigned* zb, long zb_stride, int ho, int wo, void* out,
                                     unsigned* stats, unsigned* cnt, unsigned* part) {
  const long n = (long)ho * wo;
  WG_EACH(wg, tid) {
    unsigned filled = 0;
    for (int q = 0; q < RG_PER; ++q) {
      const long at = r * RG_RUN + q * RG_THREADS + tid;
      if (at < n) {
        const unsigned z = zb[b * zb_stride + at];
        filled += z != RG_EMPTY;
        fl_store<FMT>(out, b * n + at, z == RG_EMPTY ? 0 : (int)z, nullptr);
      }
    }
    cnt[tid] = filled;
  }
  if (!stats) return;
  wg.sync();
  WG_EACH(wg, tid) rg_sum16(tid, cnt, part);
  wg.sync();
  WG_EACH(wg, tid) {
    if (tid == 0) {
      unsigned s = 0;
      for (int q = 0; q < 16; ++q) s += part[q];
      if (s) wg.atomic_add(stats + b * RG_STATS + RG_FILLED, s);
    }
  }
}

}  // namespace codon
