// Depth maps as point clouds with normals (cloud.hip): the launch plan (cd_plan), the three workgroup bodies
// (wg_cloud_count, wg_cloud_scan, wg_cloud_emit, over wg.h's group type: DESIGN 12.13) and the per-thread phases they run, written
// like clean_tile.h so that the SAME text compiles for the device and for a plain host compiler: the kernels and
// tools/cloud_host_check.cpp, under the address and undefined-behaviour sanitizers, call the same bodies.
//
// The definition (tests/cloud_ref.py).  Tables RX (w), RY (h): Q20 rays, |RX|, |RY| < 2^22.  A valid pixel (i, j) has code k,
// 1 <= k <= 65535, and the point P = (k RX[j], k RY[i], k << 20), Q20 codes, |P| < 2^38; its record holds float32(float64(P_c) m)
// per component: one multiply in double on an exact input, one conversion, nothing a compiler can contract.
// Normal: P8 = (P + 2^11) >> 12, |P8| < 2^26.  Along each axis the pixels R steps ahead (j + R, i + R) and behind COUNT if inside
// the plane and cl_linked(k, k_far, R A, Rq) (clean_tile.h's link rule, the one text); the tangent is P8+ - P8- if both count,
// P8+ - P8 or P8 - P8- if one does, and with neither, on either axis, the pixel has no normal.  n = du x dv in int64 (products
// below 2^54); s = max(0, bitlength(max |n_c|) - 30) and n_c <- sign(n_c) (|n_c| >> s); L = isqrt(n . n) (the sum below 3 2^60),
// L = 0: no normal; n . P8 > 0: n negated (the normal faces the camera); N_c = floor((2 n_c 16384 + L) / (2 L)), |N_c| <= 16384;
// the record holds float32(N_c) 2^-14, exact, and three zeros without a normal.  The only floating point beside the positions is
// the estimate of the root and of the three quotients (one reciprocal), each corrected in integers.
// Records: x y z [nx ny nz] [r g b], 12, 24, 15 or 27 bytes, packed, little-endian, one per non-zero code, in row-major order of
// the pixels.  Normal map: (h, w, 3) u8, channel 128 + ((127 N_c + 8192) >> 14); a hole or a pixel without a normal: 0, 0, 0.
//
// Three launches, a function of (B, h, w) and the record form alone; no atomic decides a position and no workgroup waits for
// another -- only kernel boundaries:
//   wg_cloud_count   CD_RUN consecutive pixels of one image: the number of non-zero codes to the block's word of the workspace
//   wg_cloud_scan    one image: the exclusive scan of its block words in place, a thread taking cd_plan().per consecutive words,
//                    the threads' sums scanned through LDS; counts[b] = (points, 0)
//   wg_cloud_emit    the count launch's blocks: a thread ranks its CD_PER consecutive pixels through LDS, forms the records, and
//                    they go to (offset + rank) REC of the image's body.  The compaction is ordered, so a block writes ONE
//                    contiguous span of bytes: the records are staged in LDS (CODON_CLOUD_STAGED, 27 KB at most) at the span's
//                    own offset modulo 4, and the span is stored with 4-byte stores between its ragged ends; 0: every thread
//                    stores its own record in bytes (the A/B of DESIGN 12.18).  The normal map; counts[b][1] summed through LDS
#pragma once

#include <stdint.h>

#include "clean_tile.h"
#include "register_tile.h"

#ifndef CODON_CLOUD_STAGED
#define CODON_CLOUD_STAGED 1
#endif

namespace codon {

constexpr bool CD_STAGED = CODON_CLOUD_STAGED != 0;
// 4: 256 threads with four consecutive pixels each; 1: 1024 threads with one pixel each (the second A/B of DESIGN 12.18)
#ifndef CODON_CLOUD_PER
#define CODON_CLOUD_PER 4
#endif
static_assert(CODON_CLOUD_PER == 4 || CODON_CLOUD_PER == 1, "CODON_CLOUD_PER is 4 or 1");
constexpr int CD_PER = CODON_CLOUD_PER, CD_RUN = 1024, CD_THREADS = CD_RUN / CD_PER;   // 1024 consecutive pixels per workgroup
constexpr int CD_PARTS = CD_PER == 4 ? 16 : 32;                                   // CD_THREADS = CD_PARTS^2: the two levels of a sum
constexpr int CD_SCAN_THREADS = RG_THREADS;                                       // the scan body: 256 threads, rg_sum16's sixteen sums
constexpr int CD_MAX_SIDE = FL_MAX_SIDE, CD_MAX_RADIUS = 8, CD_MAX_REL = 65535;
constexpr int CD_RAY_LIMIT = 1 << 22;
constexpr int CD_ONE = 16384;                                                     // a unit normal's length, Q14
constexpr int CD_POINTS = 0, CD_NORMALS = 1, CD_COUNTS = 2;

CODON_FL_HD constexpr int cd_rec(bool normals, bool color) { return 12 + (normals ? 12 : 0) + (color ? 3 : 0); }
CODON_FL_HD constexpr bool cd_rec_normals(int rec) { return rec >= 24; }
CODON_FL_HD constexpr bool cd_rec_color(int rec) { return rec % 4 == 3; }
// the staging array of the emit body in u32 words: CD_RUN records, up to 3 bytes of skew in front, rounded up
CODON_FL_HD constexpr int cd_stage_words(int rec) { return CD_STAGED ? (CD_RUN * rec + 3 + 3) / 4 : 1; }

struct CdArgs {
  int h, w;
  int radius;                      // R; 0: no normals are formed (a record form without them)
  unsigned tol_abs, tol_rel;       // R A, and Rq = rint(65536 rel)
  int channels;                    // of `color`: 1 grey, 3 RGB (read only by a record form with colour)
  double m;                        // depth_unit / 2^20: metres per Q20 code
};

// The launches of B planes of h x w: the count and emit bodies over `blocks` runs per image, the scan body once per image, a
// thread of it over `per` consecutive block words; an image's block words are `stride` apart in the workspace (16 bytes a multiple)
struct CdPlan {
  int blocks, per;
  long stride;
};
CODON_FL_HD CdPlan cd_plan(int h, int w) {
  CdPlan p;
  p.blocks = (int)(((long)h * w + CD_RUN - 1) / CD_RUN);
  p.per = (p.blocks + CD_SCAN_THREADS - 1) / CD_SCAN_THREADS;
  p.stride = ((long)p.blocks + 3) / 4 * 4;
  return p;
}
CODON_FL_HD long cd_workspace_words(int B, int h, int w) { return cd_plan(h, w).stride * B; }

// floor(sqrt(s)) for 0 <= s < 2^62: the fp64 estimate is off by less than 2^31 * 3 * 2^-53, its floor by at most one, which one
// step either way in integers sets right (as rg_floor_div does for a quotient); the root is below 2^31, its square a 32 x 32 product
CODON_FL_HD long long cd_isqrt(long long s) {
  unsigned r = (unsigned)(long long)sqrt((double)s);
  if ((unsigned long long)r * r > (unsigned long long)s) --r;
  if ((unsigned long long)(r + 1u) * (r + 1u) <= (unsigned long long)s) ++r;
  return (long long)r;
}

// floor(num / den) with inv = 1.0 / den, for |num| < 2^46 and 2 <= den < 2^32: a quotient of at most 2^15 in magnitude, the estimate
// num inv off by less than 2^15 * 3 * 2^-53, its floor by at most one, which one step either way in integers sets right.  The three
// components of a normal share den: one division
CODON_FL_HD long long cd_floor_mul(long long num, long long den, double inv) {
  long long q = (long long)floor((double)num * inv);
  long long r = num - q * den;
  if (r < 0) {
    --q;
    r += den;
  }
  if (r >= den) ++q;
  return q;
}

// P8 of code k under the rays (x, y): (P + 2^11) >> 12, an arithmetic shift; |P8| < 2^26: an int
CODON_FL_HD void cd_p8(unsigned k, int x, int y, int* p) {
  p[0] = (int)(((long long)k * x + 2048) >> 12);
  p[1] = (int)(((long long)k * y + 2048) >> 12);
  p[2] = (int)(k << 8);
}

// A loader gives the code at element `at` = i a.w + j of the a.h x a.w plane the tangents are formed on: CdPlane reads a plane of
// codes in global memory (cloud's bodies); normal_tile.h passes a loader over a tile in LDS
template <int FMT>
struct CdPlane {
  const void* in;
  CODON_FL_HD unsigned operator()(long at) const { return (unsigned)fl_load<FMT>(in, at, 0); }
};

// the tangent at pixel (i, j), code k, P8 `own`, along (di, dj): false if neither the pixel ahead nor the one behind counts;
// |d| < 2^27
template <class LD>
CODON_FL_HD bool cd_tangent(const LD& ld, const CdArgs& a, const int* rx, const int* ry, int i, int j, int di, int dj, unsigned k,
                            const int* own, int* d) {
  const int ia = i + di, ja = j + dj, ib = i - di, jb = j - dj;
  const unsigned ka = ia < a.h && ja < a.w ? ld((long)ia * a.w + ja) : 0u;
  const unsigned kb = ib >= 0 && jb >= 0 ? ld((long)ib * a.w + jb) : 0u;
  const bool fa = cl_linked(k, ka, a.tol_abs, a.tol_rel), fb = cl_linked(k, kb, a.tol_abs, a.tol_rel);       // a hole links to nothing
  if (!fa && !fb) return false;
  int hi[3] = {own[0], own[1], own[2]}, lo[3] = {own[0], own[1], own[2]};
  if (fa) cd_p8(ka, rx[ja], ry[ia], hi);
  if (fb) cd_p8(kb, rx[jb], ry[ib], lo);
  for (int c = 0; c < 3; ++c) d[c] = hi[c] - lo[c];
  return true;
}

// the normal of pixel (i, j), code k: N in Q14; false: none, and N is three zeros.  Every product is of two ints, 32 x 32 -> 64
template <class LD>
CODON_FL_HD bool cd_normal(const LD& ld, const CdArgs& a, const int* rx, const int* ry, int i, int j, unsigned k, int* N) {
  N[0] = N[1] = N[2] = 0;
  int own[3], du[3], dv[3];
  cd_p8(k, rx[j], ry[i], own);
  if (!cd_tangent(ld, a, rx, ry, i, j, 0, a.radius, k, own, du)) return false;
  if (!cd_tangent(ld, a, rx, ry, i, j, a.radius, 0, k, own, dv)) return false;
  const long long n[3] = {(long long)du[1] * dv[2] - (long long)du[2] * dv[1], (long long)du[2] * dv[0] - (long long)du[0] * dv[2],
                          (long long)du[0] * dv[1] - (long long)du[1] * dv[0]};
  unsigned long long mx = 0;
  for (int c = 0; c < 3; ++c) {
    const unsigned long long v = (unsigned long long)(n[c] < 0 ? -n[c] : n[c]);
    mx = v > mx ? v : mx;
  }
  if (mx == 0) return false;
  const int bits = 64 - __builtin_clzll(mx), s = bits > 30 ? bits - 30 : 0;
  int r[3];                                                           // the reduced n: below 2^30 in magnitude
  long long sq = 0, dot = 0;
  for (int c = 0; c < 3; ++c) {
    const int v = (int)((n[c] < 0 ? -n[c] : n[c]) >> s);
    r[c] = n[c] < 0 ? -v : v;
    sq += (long long)v * v;
    dot += (long long)r[c] * own[c];
  }
  const long long L = cd_isqrt(sq);
  if (L == 0) return false;
  const double inv = 1.0 / (double)(2 * L);
  for (int c = 0; c < 3; ++c) N[c] = (int)cd_floor_mul(2 * (long long)(dot > 0 ? -r[c] : r[c]) * CD_ONE + L, 2 * L, inv);
  return true;
}

CODON_FL_HD unsigned cd_bits(float v) {
  unsigned u;
  __builtin_memcpy(&u, &v, 4);
  return u;
}

// four bytes, little-endian, at p: one store where p is 4-byte aligned and `words` allows, else bytes
CODON_FL_HD void cd_put32(unsigned char* p, unsigned v, bool word) {
  if (word) {
    *(unsigned*)p = v;
  } else {
    p[0] = (unsigned char)v, p[1] = (unsigned char)(v >> 8), p[2] = (unsigned char)(v >> 16), p[3] = (unsigned char)(v >> 24);
  }
}

// the record of pixel `at` = (i, j) of this image, code k != 0, to the REC bytes at p; its normal's texel to nmap (this image's
// map, or null); returns 1 if the pixel has a normal
template <int FMT, int REC>
CODON_FL_HD unsigned cd_record(const void* in, const CdArgs& a, const int* rx, const int* ry, const unsigned char* color, long at,
                               int i, int j, unsigned k, unsigned char* p, bool word, unsigned char* nmap) {
  const long long P[3] = {(long long)k * rx[j], (long long)k * ry[i], (long long)k << 20};
  for (int c = 0; c < 3; ++c) cd_put32(p + 4 * c, cd_bits((float)((double)P[c] * a.m)), word);
  unsigned has = 0;
  if (cd_rec_normals(REC)) {
    int N[3];
    has = cd_normal(CdPlane<FMT>{in}, a, rx, ry, i, j, k, N);
    for (int c = 0; c < 3; ++c) cd_put32(p + 12 + 4 * c, cd_bits((float)N[c] * (1.0f / CD_ONE)), word);
    if (nmap && has)
      for (int c = 0; c < 3; ++c) nmap[at * 3 + c] = (unsigned char)(128 + ((127 * N[c] + CD_ONE / 2) >> 14));
  }
  if (cd_rec_color(REC)) {
    unsigned char* q = p + (cd_rec_normals(REC) ? 24 : 12);
    for (int c = 0; c < 3; ++c) q[c] = a.channels == 3 ? color[at * 3 + c] : color[at];
  }
  return has;
}

// the number of non-zero codes among a thread's CD_PER pixels of run r
template <int FMT>
CODON_FL_HD unsigned cd_valid(const void* in, long n, long r, int tid) {
  unsigned c = 0;
  for (int q = 0; q < CD_PER; ++q) {
    const long at = r * CD_RUN + tid * CD_PER + q;
    if (at < n) c += fl_load<FMT>(in, at, 0) != 0;
  }
  return c;
}

// the sums over a workgroup of P^2 threads of one word per thread: phase 1 of 2 -- P partial sums of P words
template <int P>
CODON_FL_HD void cd_sum(int tid, const unsigned* cnt, unsigned* part) {
  if (tid >= P) return;
  unsigned s = 0;
  for (int q = 0; q < P; ++q) s += cnt[tid * P + q];
  part[tid] = s;
}
// the exclusive prefix of cnt[tid] over the workgroup, from cd_sum's partial sums
template <int P>
CODON_FL_HD unsigned cd_prefix(int tid, const unsigned* cnt, const unsigned* part) {
  unsigned s = 0;
  for (int q = 0; q < tid / P; ++q) s += part[q];
  for (int q = tid / P * P; q < tid; ++q) s += cnt[q];
  return s;
}
template <int P>
CODON_FL_HD unsigned cd_total(const unsigned* part) {
  unsigned s = 0;
  for (int q = 0; q < P; ++q) s += part[q];
  return s;
}

// ---- the workgroup bodies -------------------------------------------------------------------------------------------------------

// workgroup (r, b) of grid (blocks, B), CD_THREADS threads.  LDS: cnt CD_THREADS words, part CD_PARTS
template <int FMT, class G>
CODON_FL_HD void wg_cloud_count(G wg, long r, long b, const void* in, int h, int w, unsigned* ws, unsigned* cnt, unsigned* part) {
  const CdPlan p = cd_plan(h, w);
  const long n = (long)h * w;
  const void* plane = (const char*)in + b * n * fl_elem_bytes(FMT);
  WG_EACH(wg, tid) cnt[tid] = cd_valid<FMT>(plane, n, r, tid);
  wg.sync();
  WG_EACH(wg, tid) cd_sum<CD_PARTS>(tid, cnt, part);
  wg.sync();
  WG_EACH(wg, tid) {
    if (tid == 0) ws[b * p.stride + r] = cd_total<CD_PARTS>(part);
  }
}

// The scan body, one workgroup of CD_SCAN_THREADS threads: the `blocks` words at `word` to their exclusive scan in place, a thread
// taking `per` consecutive words (per CD_SCAN_THREADS >= blocks; blocks may be 0); *total = their sum, and *zero = 0 where zero is
// not null.  The cloud's block words and the mesh's run words (mesh_tile.h) both go through it.  LDS: cnt CD_SCAN_THREADS words,
// part 16
template <class G>
CODON_FL_HD void wg_scan_words(G wg, unsigned* word, int blocks, int per, unsigned* total, unsigned* zero, unsigned* cnt,
                               unsigned* part) {
  WG_EACH(wg, tid) {
    unsigned s = 0;
    for (int q = 0; q < per; ++q) {
      const int at = tid * per + q;
      if (at < blocks) s += word[at];
    }
    cnt[tid] = s;
  }
  wg.sync();
  WG_EACH(wg, tid) rg_sum16(tid, cnt, part);
  wg.sync();
  WG_EACH(wg, tid) {
    unsigned s = cd_prefix<16>(tid, cnt, part);
    for (int q = 0; q < per; ++q) {
      const int at = tid * per + q;
      if (at < blocks) {
        const unsigned c = word[at];
        word[at] = s;
        s += c;
      }
    }
    if (tid == 0) {
      *total = cd_total<16>(part);
      if (zero) *zero = 0u;
    }
  }
}

// workgroup b of grid (B), CD_SCAN_THREADS threads: the block words of image b to their exclusive scan, counts[b] = (their sum,
// 0).  LDS: cnt CD_SCAN_THREADS words, part 16
template <class G>
CODON_FL_HD void wg_cloud_scan(G wg, long b, int h, int w, unsigned* ws, unsigned* counts, unsigned* cnt, unsigned* part) {
  const CdPlan p = cd_plan(h, w);
  wg_scan_words(wg, ws + b * p.stride, p.blocks, p.per, counts + b * CD_COUNTS + CD_POINTS, counts + b * CD_COUNTS + CD_NORMALS, cnt,
                part);
}

// workgroup (r, b) of grid (blocks, B).  body: image b's records start at byte b h w REC; color (a form with colour): (B, h, w) or
// (B, h, w, 3) u8; nmap: (B, h, w, 3) u8 or null.  LDS: cnt and ncnt CD_THREADS words each, part and npart CD_PARTS each, stage
// cd_stage_words(REC) words (CD_STAGED alone reads it)
template <int FMT, int REC, class G>
CODON_FL_HD void wg_cloud_emit(G wg, long r, long b, const void* in, const CdArgs& a, const int* rx, const int* ry,
                               const unsigned char* color, unsigned char* body, unsigned* counts, unsigned char* nmap,
                               const unsigned* ws, unsigned* cnt, unsigned* ncnt, unsigned* part, unsigned* npart, unsigned* stage) {
  const CdPlan p = cd_plan(a.h, a.w);
  const long n = (long)a.h * a.w;
  const void* plane = (const char*)in + b * n * fl_elem_bytes(FMT);
  const unsigned char* tint = cd_rec_color(REC) ? color + b * n * a.channels : nullptr;
  unsigned char* texels = nmap ? nmap + b * n * 3 : nullptr;
  unsigned char* dst = body + (b * n + (long)ws[b * p.stride + r]) * REC;        // the block's span starts here
  const int skew = (int)((uintptr_t)dst & 3);
  unsigned char* staged = (unsigned char*)stage + skew;                           // staged[x] goes to dst[x]
  WG_EACH(wg, tid) cnt[tid] = cd_valid<FMT>(plane, n, r, tid);
  wg.sync();
  WG_EACH(wg, tid) cd_sum<CD_PARTS>(tid, cnt, part);
  wg.sync();
  WG_EACH(wg, tid) {
    long rank = cd_prefix<CD_PARTS>(tid, cnt, part);
    unsigned has = 0;
    long at = r * CD_RUN + tid * CD_PER;
    int i = (int)(at / a.w), j = (int)(at - (long)i * a.w);
    for (int q = 0; q < CD_PER && at < n; ++q, ++at) {
      const unsigned k = (unsigned)fl_load<FMT>(plane, at, 0);
      if (texels) texels[at * 3] = texels[at * 3 + 1] = texels[at * 3 + 2] = 0;
      if (k != 0u) {
        unsigned char* rec = (CD_STAGED ? staged : dst) + rank * REC;
        has += cd_record<FMT, REC>(plane, a, rx, ry, tint, at, i, j, k, rec, CD_STAGED && ((skew + rank * REC) & 3) == 0, texels);
        ++rank;
      }
      if (++j == a.w) j = 0, ++i;
    }
    ncnt[tid] = has;
  }
  if (!CD_STAGED && !cd_rec_normals(REC)) return;
  wg.sync();
  WG_EACH(wg, tid) {
    if (CD_STAGED) {
      // the span [0, bytes): bytes up to the first 4-byte boundary of its address, words, and bytes again
      const long bytes = (long)cd_total<CD_PARTS>(part) * REC;
      const long lead = (4 - skew) & 3, head = lead < bytes ? lead : bytes, words = (bytes - head) / 4;
      for (long x = tid; x < head; x += CD_THREADS) dst[x] = staged[x];
      for (long x = tid; x < words; x += CD_THREADS) *(unsigned*)(dst + head + 4 * x) = stage[(skew + head) / 4 + x];
      for (long x = head + 4 * words + tid; x < bytes; x += CD_THREADS) dst[x] = staged[x];
    }
    if (cd_rec_normals(REC)) cd_sum<CD_PARTS>(tid, ncnt, npart);
  }
  if (!cd_rec_normals(REC)) return;
  wg.sync();
  WG_EACH(wg, tid) {
    if (tid == 0) {
      const unsigned s = cd_total<CD_PARTS>(npart);
      if (s) wg.atomic_add(counts + b * CD_COUNTS + CD_NORMALS, s);
    }
  }
}

}  // namespace codon
