// Host-side check of the spatial smoothing of sensor depth maps: the workgroup body of csrc/smooth_tile.h --
// the very text the device kernel of csrc/smooth.hip calls -- compiled for the host and run workgroup by workgroup of the launches
// over exactly-sized heap buffers (the two LDS planes, the weight table, the intermediate planes and the arrays of the sums too), so
// that the address and undefined-behaviour sanitizers see every access.  `in` and `out` stand ONE ELEMENT into larger buffers, and
// the elements before and behind must stay as they were; a second pass has both on a 16-byte boundary.  Every case runs with the
// passes split over the launches in every way the launcher's rule could choose (at most 1, 2 or 3 passes a launch), with the threads
// of a workgroup forwards and backwards, and with and without statistics, and all outputs must agree.  No GPU, no HIP, nothing
// loaded into Python.
// `python tools/host_check.py smooth` builds this, runs it over the GPU test's cases and compares what it writes with
// tests/smooth_ref.py, bit for bit.
//
//   smooth_host_check <fmt 0|1> B h w R P pairs A Rq in.bin weights.bin out.bin stats.bin
//     in.bin: (B, h, w) codes; weights.bin: (2R+1)^2 int32  ->  out.bin: (B, h, w) codes; stats.bin: (B, 4) uint32
#include "host_check.h"

#include "../codon_amd/csrc/smooth_tile.h"

using namespace codon;

// smooth_launch<FMT> of smooth.hip with at most `bound` passes a launch; ws: one plane set
template <int FMT, int R>
static void launches(WgHost wg, int B, const void* in, SmArgs a, int passes, int bound, const int* wtab, void* out, unsigned* stats, void* ws) {
  wg_clean_zero(wg, stats, B * SM_STATS);
  const int fused = passes < bound ? passes : bound, n = (passes + fused - 1) / fused;
  const void* src = in;
  for (int i = 0, done = 0; i < n; ++i) {
    void* dst = (n - 1 - i) % 2 == 0 ? out : ws;
    a.fused = passes - done < fused ? passes - done : fused;
    a.first = i == 0, a.last = i == n - 1;
    for (int b = 0; b < B; ++b)
      for (int ty = 0; ty < (a.h + SM_TILE - 1) / SM_TILE; ++ty)
        for (int tx = 0; tx < (a.w + SM_TILE - 1) / SM_TILE; ++tx) {
          const int span = SM_TILE + 2 * R * a.fused;                        // the launch's own need: less than the kernel declares,
          const size_t cells = (size_t)(span - 1) * sm_stride<R>() + span;   // up to the last cell of its last row
          unsigned short* pa = hc_alloc<unsigned short>(sizeof(unsigned short) * cells, 0xCD);
          unsigned short* pb = hc_alloc<unsigned short>(sizeof(unsigned short) * cells, 0xCD);
          unsigned* cnt = hc_alloc<unsigned>(sizeof(unsigned) * 2 * SM_THREADS, 0xCD);
          unsigned* part = hc_alloc<unsigned>(sizeof(unsigned) * 32, 0xCD);
          unsigned* mx = hc_alloc<unsigned>(sizeof(unsigned) * SM_THREADS, 0xCD);
          unsigned* pmx = hc_alloc<unsigned>(sizeof(unsigned) * 16, 0xCD);
          wg_smooth<FMT, R>(wg, tx, ty, (long)b, src, in, a, wtab, dst, stats, pa, pb, cnt, part, mx, pmx);
          free(pa), free(pb), free(cnt), free(part), free(mx), free(pmx);
        }
    done += a.fused;
    src = dst;
  }
}

// smooth_radii<FMT>
template <int FMT>
static void radii(WgHost wg, int B, const void* in, const SmArgs& a, int passes, int bound, const int* wtab, void* out, unsigned* stats, void* ws) {
  switch (a.radius) {
    case 1: return launches<FMT, 1>(wg, B, in, a, passes, bound, wtab, out, stats, ws);
    case 2: return launches<FMT, 2>(wg, B, in, a, passes, bound, wtab, out, stats, ws);
    case 3: return launches<FMT, 3>(wg, B, in, a, passes, bound, wtab, out, stats, ws);
    default: return launches<FMT, 4>(wg, B, in, a, passes, bound, wtab, out, stats, ws);
  }
}

template <int FMT>
static int run(int B, SmArgs a, int passes, char** path) {
  const size_t e = fl_elem_bytes(FMT), bytes = (size_t)B * a.h * a.w * e, stats_bytes = sizeof(unsigned) * B * SM_STATS;
  const int side = 2 * a.radius + 1;
  int* wtab = hc_read<int>(path[1], sizeof(int) * side * side);
  char* first = nullptr;
  unsigned* first_stats = nullptr;
  for (int bound = 1; bound <= (passes < SM_MAX_PASSES ? passes : SM_MAX_PASSES); ++bound)
    for (int skew = 1; skew >= 0; --skew) {          // one element into larger buffers, then on a 16-byte boundary
      const size_t lead = skew * e, whole = bytes + 2 * lead;
      char* src = (char*)memset(hc_aligned(whole), 0x77, whole);
      hc_read(path[0], bytes, lead, src);
      for (int rev = 0; rev < 2; ++rev)
        for (int with = 1; with >= 0; --with) {
          char* out = (char*)memset(hc_aligned(whole), 0xEE, whole);
          char* ws = (char*)memset(hc_aligned(whole), 0xEE, whole);
          unsigned* stats = with ? hc_alloc<unsigned>(stats_bytes, 0xEE) : nullptr;
          radii<FMT>(WgHost{SM_THREADS, rev != 0}, B, src + lead, a, passes, bound, wtab, out + lead, stats, ws + lead);
          for (size_t i = 0; i < lead; ++i)
            if ((unsigned char)out[i] != 0xEE || (unsigned char)out[lead + bytes + i] != 0xEE || (unsigned char)ws[i] != 0xEE ||
                (unsigned char)ws[lead + bytes + i] != 0xEE)
              hc_die("an element beside `out` or the workspace was written");
          free(ws);
          if (!first) {
            first = out, first_stats = stats;
            continue;
          }
          hc_same(first + e, out + lead, bytes, "the output depends on the split of the passes, the thread order, the statistics pointer or the alignment");
          if (with) hc_same(first_stats, stats, stats_bytes, "the statistics depend on the split of the passes, the thread order or the alignment");
          free(out), free(stats);
        }
      for (size_t i = 0; i < lead; ++i)
        if (src[i] != 0x77 || src[lead + bytes + i] != 0x77) hc_die("an element beside `in` was written");
      char* again = hc_read<char>(path[0], bytes);
      hc_same(again, src + lead, bytes, "`in` was modified");
      free(again), free(src);
    }
  hc_write(path[2], first + e, bytes);
  hc_write(path[3], first_stats, stats_bytes);
  free(first), free(first_stats), free(wtab);
  return 0;
}

int main(int argc, char** argv) {
  hc_name = "smooth_host_check";
  if (argc != 14) hc_die("usage: smooth_host_check <fmt 0|1> B h w R P pairs A Rq in.bin weights.bin out.bin stats.bin");
  const int fmt = atoi(argv[1]), B = atoi(argv[2]);
  SmArgs a;
  a.h = atoi(argv[3]), a.w = atoi(argv[4]), a.radius = atoi(argv[5]);
  const int passes = atoi(argv[6]);
  a.pairs = atoi(argv[7]);
  const int A = atoi(argv[8]), Rq = atoi(argv[9]);
  a.fused = 1, a.first = a.last = 1;
  if (B < 1 || B > 65535 || a.h < 1 || a.h > SM_MAX_SIDE || a.w < 1 || a.w > SM_MAX_SIDE || a.radius < 1 || a.radius > SM_MAX_RADIUS ||
      passes < 1 || passes > SM_MAX_PASSES || (a.pairs != 0 && a.pairs != 1) || A < 0 || A > 65535 || Rq < 0 || Rq > SM_MAX_REL)
    return 2;
  a.tol_abs = (unsigned)A, a.tol_rel = (unsigned)Rq;
  char* path[4] = {argv[10], argv[11], argv[12], argv[13]};
  if (fmt == FL_U8) return run<FL_U8>(B, a, passes, path);
  if (fmt == FL_U16) return run<FL_U16>(B, a, passes, path);
  return 2;
}
