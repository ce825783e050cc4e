// Depth maps as triangle meshes (cloud.hip): the launch plan (ms_plan), the workgroup bodies (wg_mesh_index,
// wg_mesh_count, wg_mesh_scan, wg_mesh_emit, over wg.h's group type: DESIGN 12.13) and the per-thread phases they run, written like
// cloud_tile.h so that the SAME text compiles for the device and for a plain host compiler: the kernels and
// tools/mesh_host_check.cpp, under the address and undefined-behaviour sanitizers, call the same bodies.
//
// The definition (tests/mesh_ref.py).  Vertices are the cloud's own: the index of a non-zero code is its rank among the non-zero
// codes of the plane in row-major order.  Quad q = i (w - 1) + j, 0 <= i < h - 1, 0 <= j < w - 1, has the corners a = (i, j),
// b = (i, j + 1), c = (i + 1, j), d = (i + 1, j + 1).  Two corners are linked by cl_linked(k1, k2, A, Rq) (clean_tile.h's link rule,
// the one text), A for ONE step, sides and diagonals alike; a hole links to nothing.  A triangle is emitted when its three corners
// are pairwise linked.  Four non-zero corners: the diagonal is a-d if |k_a - k_d| <= |k_b - k_c| and b-c otherwise; a-d gives
// (a, c, d) then (a, d, b), b-c gives (a, c, b) then (b, c, d), each emitted on its own, the other diagonal never retried.  Three:
// the one triangle of those four without the missing corner.  Fewer: none.  Faces go in row-major order of the quads, the
// first-listed triangle first: 13 bytes each, packed, the byte 3 and three little-endian int32 vertex indices.
//
// Faces depend on the codes alone, so the entry ranks the vertices itself.  SIX launches, a function of (B, h, w) alone (ONE, the
// face scan, for a plane without a quad); no atomic decides a position and no workgroup waits for another -- only kernel boundaries:
//   wg_cloud_count   cloud_tile.h's, unchanged: the non-zero codes of CD_RUN consecutive pixels to the block's word
//   wg_cloud_scan    cloud_tile.h's, unchanged: the exclusive scan of an image's block words (its two counts go to the workspace)
//   wg_mesh_index    the count launch's blocks: a thread ranks its CD_PER consecutive pixels through LDS and writes offset + rank,
//                    or -1 for a hole, to the int32 index plane in the workspace
//   wg_mesh_count    MS_RUN consecutive quads of one image, MS_PER consecutive quads a thread: the number of faces to the run's word
//   wg_mesh_scan     one image: cloud_tile.h's scan body over the run words; counts[b] = faces
//   wg_mesh_emit     the count launch's runs: a thread ranks its quads' faces through LDS and forms the records at the run's own
//                    offset modulo 4 in LDS (MS_RUN * 2 * 13 bytes and the skew: 26 628 bytes); the run's ONE contiguous span is
//                    stored with 4-byte stores between its ragged ends, as wg_cloud_emit stores its records
// A thread's MS_PER quads are consecutive, so the lanes of a wave read one contiguous stretch of row i and one of row i + 1 (of
// the codes, and in the emit of the indices): every byte of a fetched line is used, the second to fifth read of a line are cache
// hits.
#pragma once

#include <stdint.h>

#include "cloud_tile.h"

namespace codon {

constexpr int MS_PER = 4, MS_THREADS = 256, MS_RUN = MS_THREADS * MS_PER;        // 1024 consecutive quads per workgroup
constexpr int MS_PARTS = 16;                                                      // MS_THREADS = MS_PARTS^2: the two levels of a sum
constexpr int MS_REC = 13, MS_QUAD_FACES = 2;
constexpr int MS_MAX_SIDE = CD_MAX_SIDE, MS_MAX_REL = CD_MAX_REL;
constexpr int MS_STAGE_WORDS = (MS_RUN * MS_QUAD_FACES * MS_REC + 3 + 3) / 4;     // the records of a run, 3 bytes of skew, rounded up
static_assert(MS_THREADS == MS_PARTS * MS_PARTS, "cd_sum and cd_prefix take a square");

struct MsArgs {
  int h, w;
  unsigned tol_abs, tol_rel;       // A, and Rq = rint(65536 rel)
};

// The face launches of B planes of h x w: the count and emit bodies over `runs` runs per image (0: no quad, they are not
// launched), the scan body once per image, a thread of it over `per` consecutive run words; an image's run words are `stride` apart
struct MsPlan {
  long quads;
  int runs, per;
  long stride;
};
CODON_FL_HD MsPlan ms_plan(int h, int w) {
  MsPlan p;
  p.quads = (long)(h - 1) * (w - 1);
  p.runs = (int)((p.quads + MS_RUN - 1) / MS_RUN);
  p.per = (p.runs + CD_SCAN_THREADS - 1) / CD_SCAN_THREADS;
  p.stride = p.runs ? ((long)p.runs + 3) / 4 * 4 : 4;
  return p;
}
CODON_FL_HD long ms_face_bytes(int h, int w) { return (long)(h - 1) * (w - 1) * MS_QUAD_FACES * MS_REC; }   // one image's row of `faces`

// The workspace in u32 words, every part a multiple of four words (16 bytes) from the start: the cloud's block words of the B
// images, the run words, the (B, 2) counts wg_cloud_scan writes, the (B, h, w) int32 index plane
struct MsSpace {
  long blocks, runs, counts, index, words;
};
CODON_FL_HD MsSpace ms_space(int B, int h, int w) {
  MsSpace s;
  s.blocks = 0;
  s.runs = s.blocks + cd_workspace_words(B, h, w);
  s.counts = s.runs + ms_plan(h, w).stride * B;
  s.index = s.counts + ((long)B * CD_COUNTS + 3) / 4 * 4;
  s.words = s.index + ((long)B * h * w + 3) / 4 * 4;
  return s;
}

// The faces of a quad with the codes ka .. kd: bits 0-1 their number n, bits 2-7 the first triangle and bits 8-13 the second, a
// triangle three corners of two bits each (0 a, 1 b, 2 c, 3 d) in the order of the definition.  With a corner missing the diagonal
// is the one that does not end in it, and the triangle that holds the hole fails its links; with two missing every triangle does
CODON_FL_HD unsigned ms_quad(unsigned ka, unsigned kb, unsigned kc, unsigned kd, const MsArgs& a) {
  const unsigned dad = ka < kd ? kd - ka : ka - kd, dbc = kb < kc ? kc - kb : kb - kc;
  const bool ad = ka != 0u && kd != 0u && (kb == 0u || kc == 0u || dad <= dbc);
  const bool ab = cl_linked(ka, kb, a.tol_abs, a.tol_rel), ac = cl_linked(ka, kc, a.tol_abs, a.tol_rel);
  const bool bd = cl_linked(kb, kd, a.tol_abs, a.tol_rel), cd = cl_linked(kc, kd, a.tol_abs, a.tol_rel);
  const bool dg = ad ? cl_linked(ka, kd, a.tol_abs, a.tol_rel) : cl_linked(kb, kc, a.tol_abs, a.tol_rel);
  // a-d: (a, c, d) = 0 | 2 << 2 | 3 << 4 and (a, d, b) = 0 | 3 << 2 | 1 << 4;  b-c: (a, c, b) = 0 | 2 << 2 | 1 << 4 and (b, c, d) = 1 | 2 << 2 | 3 << 4
  const unsigned t1 = ad ? 56u : 24u, t2 = ad ? 28u : 57u;
  const bool e1 = dg && ac && (ad ? cd : ab), e2 = dg && bd && (ad ? ab : cd);
  if (e1) return (e2 ? 2u : 1u) | t1 << 2 | t2 << 8;
  return e2 ? 1u | t2 << 2 : 0u;
}

// quad q of an h x w plane -> (i, j); q < 4095^2: an int
CODON_FL_HD void ms_at(int q, int w, int* i, int* j) {
  *i = q / (w - 1);
  *j = q - *i * (w - 1);
}

// the number of faces among a thread's MS_PER quads of run r (plane: one image's codes)
template <int FMT>
CODON_FL_HD unsigned ms_faces(const void* plane, const MsArgs& a, int quads, long r, int tid) {
  int q = (int)r * MS_RUN + tid * MS_PER;
  if (q >= quads) return 0u;
  int i, j;
  ms_at(q, a.w, &i, &j);
  unsigned n = 0;
  for (int s = 0; s < MS_PER && q < quads; ++s, ++q) {
    const long at = (long)i * a.w + j;
    n += ms_quad((unsigned)fl_load<FMT>(plane, at, 0), (unsigned)fl_load<FMT>(plane, at + 1, 0),
                 (unsigned)fl_load<FMT>(plane, at + a.w, 0), (unsigned)fl_load<FMT>(plane, at + a.w + 1, 0), a) & 3u;
    if (++j == a.w - 1) j = 0, ++i;
  }
  return n;
}

// one record to the 13 bytes at p: the int32s are 4-byte stores where they are aligned (`word`), else bytes
CODON_FL_HD void ms_record(unsigned char* p, bool word, int v0, int v1, int v2) {
  p[0] = 3;
  cd_put32(p + 1, (unsigned)v0, word);
  cd_put32(p + 5, (unsigned)v1, word);
  cd_put32(p + 9, (unsigned)v2, word);
}

// corner c (0 a, 1 b, 2 c, 3 d) of four values
CODON_FL_HD int ms_pick(unsigned c, int va, int vb, int vc, int vd) { return c == 0u ? va : c == 1u ? vb : c == 2u ? vc : vd; }

// ---- the workgroup bodies -------------------------------------------------------------------------------------------------------

// workgroup (r, b) of grid (cd_plan's blocks, B), CD_THREADS threads, after wg_cloud_scan: index[b h w + at] = the rank of pixel
// `at` among image b's non-zero codes, -1 for a hole.  LDS: cnt CD_THREADS words, part CD_PARTS
template <int FMT, class G>
CODON_FL_HD void wg_mesh_index(G wg, long r, long b, const void* in, int h, int w, const unsigned* ws, int* index, unsigned* cnt,
                               unsigned* part) {
  const CdPlan p = cd_plan(h, w);
  const long n = (long)h * w;
  const void* plane = (const char*)in + b * n * fl_elem_bytes(FMT);
  int* out = index + b * n;
  WG_EACH(wg, tid) cnt[tid] = cd_valid<FMT>(plane, n, r, tid);
  wg.sync();
  WG_EACH(wg, tid) cd_sum<CD_PARTS>(tid, cnt, part);
  wg.sync();
  WG_EACH(wg, tid) {
    unsigned rank = ws[b * p.stride + r] + cd_prefix<CD_PARTS>(tid, cnt, part);
    long at = r * CD_RUN + tid * CD_PER;
    for (int q = 0; q < CD_PER && at < n; ++q, ++at) out[at] = fl_load<FMT>(plane, at, 0) != 0 ? (int)rank++ : -1;
  }
}

// workgroup (r, b) of grid (runs, B), MS_THREADS threads: runs[b stride + r] = the faces of run r.  LDS: cnt MS_THREADS words,
// part MS_PARTS
template <int FMT, class G>
CODON_FL_HD void wg_mesh_count(G wg, long r, long b, const void* in, const MsArgs& a, unsigned* runs, unsigned* cnt, unsigned* part) {
  const MsPlan p = ms_plan(a.h, a.w);
  const void* plane = (const char*)in + b * ((long)a.h * a.w) * fl_elem_bytes(FMT);
  WG_EACH(wg, tid) cnt[tid] = ms_faces<FMT>(plane, a, (int)p.quads, r, tid);
  wg.sync();
  WG_EACH(wg, tid) cd_sum<MS_PARTS>(tid, cnt, part);
  wg.sync();
  WG_EACH(wg, tid) {
    if (tid == 0) runs[b * p.stride + r] = cd_total<MS_PARTS>(part);
  }
}

// workgroup b of grid (B), CD_SCAN_THREADS threads: the run words of image b to their exclusive scan, counts[b] = their sum (0 for
// a plane without a quad).  LDS: cnt CD_SCAN_THREADS words, part 16
template <class G>
CODON_FL_HD void wg_mesh_scan(G wg, long b, int h, int w, unsigned* runs, unsigned* counts, unsigned* cnt, unsigned* part) {
  const MsPlan p = ms_plan(h, w);
  wg_scan_words(wg, runs + b * p.stride, p.runs, p.per, counts + b, (unsigned*)nullptr, cnt, part);
}

// workgroup (r, b) of grid (runs, B), MS_THREADS threads, after wg_mesh_scan.  faces: image b's records start at byte
// b ms_face_bytes(h, w).  LDS: cnt MS_THREADS words, part MS_PARTS, stage MS_STAGE_WORDS words
template <int FMT, class G>
CODON_FL_HD void wg_mesh_emit(G wg, long r, long b, const void* in, const MsArgs& a, const int* index, const unsigned* runs,
                              unsigned char* faces, unsigned* cnt, unsigned* part, unsigned* stage) {
  const MsPlan p = ms_plan(a.h, a.w);
  const long n = (long)a.h * a.w;
  const void* plane = (const char*)in + b * n * fl_elem_bytes(FMT);
  const int* idx = index + b * n;
  unsigned char* dst = faces + b * ms_face_bytes(a.h, a.w) + (long)runs[b * p.stride + r] * MS_REC;      // the run's span starts here
  const int skew = (int)((uintptr_t)dst & 3);
  unsigned char* staged = (unsigned char*)stage + skew;                           // staged[x] goes to dst[x]
  WG_EACH(wg, tid) cnt[tid] = ms_faces<FMT>(plane, a, (int)p.quads, r, tid);
  wg.sync();
  WG_EACH(wg, tid) cd_sum<MS_PARTS>(tid, cnt, part);
  wg.sync();
  WG_EACH(wg, tid) {
    int q = (int)r * MS_RUN + tid * MS_PER;
    if (q < p.quads && cnt[tid] != 0u) {
      long rank = cd_prefix<MS_PARTS>(tid, cnt, part);
      int i, j;
      ms_at(q, a.w, &i, &j);
      for (int s = 0; s < MS_PER && q < p.quads; ++s, ++q) {
        const long at = (long)i * a.w + j;
        const unsigned f = ms_quad((unsigned)fl_load<FMT>(plane, at, 0), (unsigned)fl_load<FMT>(plane, at + 1, 0),
                                   (unsigned)fl_load<FMT>(plane, at + a.w, 0), (unsigned)fl_load<FMT>(plane, at + a.w + 1, 0), a);
        if ((f & 3u) != 0u) {
          const int va = idx[at], vb = idx[at + 1], vc = idx[at + a.w], vd = idx[at + a.w + 1];
          for (unsigned t = 0; t < (f & 3u); ++t, ++rank) {
            const unsigned tri = f >> (2 + 6 * t);
            unsigned char* rec = staged + rank * MS_REC;
            ms_record(rec, ((skew + rank * MS_REC + 1) & 3) == 0, ms_pick(tri & 3u, va, vb, vc, vd), ms_pick((tri >> 2) & 3u, va, vb, vc, vd),
                      ms_pick((tri >> 4) & 3u, va, vb, vc, vd));
          }
        }
        if (++j == a.w - 1) j = 0, ++i;
      }
    }
  }
  wg.sync();
  WG_EACH(wg, tid) {
    // the span [0, bytes): bytes up to the first 4-byte boundary of its address, words, and bytes again
    const long bytes = (long)cd_total<MS_PARTS>(part) * MS_REC;
    const long lead = (4 - skew) & 3, head = lead < bytes ? lead : bytes, words = (bytes - head) / 4;
    for (long x = tid; x < head; x += MS_THREADS) dst[x] = staged[x];
    for (long x = tid; x < words; x += MS_THREADS) *(unsigned*)(dst + head + 4 * x) = stage[(skew + head) / 4 + x];
    for (long x = head + 4 * words + tid; x < bytes; x += MS_THREADS) dst[x] = staged[x];
  }
}

}  // namespace codon
