// Host-side check of the temporal filter of a depth sequence: the workgroup body of csrc/temporal_tile.h --
// the very text the device kernel of csrc/temporal.hip calls -- compiled for the host and run workgroup by workgroup of the two
// launches over exactly-sized heap buffers (the LDS ring and the two arrays of the sums too), so that the address and
// undefined-behaviour sanitizers see every access.  `in` and `out` stand ONE ELEMENT into larger buffers: the four-pixel loads and
// stores are then off their alignment and the body must take the element path, and the elements before and behind stay as they
// were; a second pass with both on a 16-byte boundary takes the four-pixel path where the plane allows it.  Every case runs with
// the threads of a workgroup forwards and backwards, and with and without statistics, and the outputs must agree.  No GPU, no HIP,
// nothing loaded into Python.
// `python tools/host_check.py temporal` builds this, runs it over the GPU test's cases and compares what it writes with
// tests/temporal_ref.py, bit for bit.
//
//   temporal_host_check <fmt 0|1> T h w Bk Ah A Rq M F chunk in.bin out.bin stats.bin
//     in.bin: (T, h, w) codes  ->  out.bin: (T, h, w) codes; stats.bin: (T, 4) uint32.  chunk: the frames per time chunk, the
//     launcher's rule as tests/temporal_ref.py restates it
#include "host_check.h"

#include "../codon_amd/csrc/temporal_tile.h"

using namespace codon;

// temporal_caps<FMT> and temporal_launch<FMT, CAP>
template <int FMT, int CAP>
static void launches(WgHost wg, const void* in, const TpArgs& a, void* out, unsigned* stats) {
  wg_clean_zero(wg, stats, a.T * TP_STATS);
  const long groups = ((long)a.h * a.w + TP_TILE - 1) / TP_TILE;
  const int chunks = (a.T + a.chunk - 1) / a.chunk;
  for (int c = 0; c < chunks; ++c)
    for (long gx = 0; gx < groups; ++gx) {
      tp_quad* ring = hc_alloc<tp_quad>(sizeof(tp_quad) * TP_SLOTS * TP_THREADS, 0xCD);
      unsigned* cnt = hc_alloc<unsigned>(sizeof(unsigned) * 2 * TP_THREADS, 0xCD);
      unsigned* part = hc_alloc<unsigned>(sizeof(unsigned) * 32, 0xCD);
      wg_temporal<FMT, CAP>(wg, gx, c, in, a, out, stats, ring, cnt, part);
      free(ring), free(cnt), free(part);
    }
}

template <int FMT>
static void caps(WgHost wg, const void* in, const TpArgs& a, void* out, unsigned* stats) {
  const int n = a.back + a.ahead + 1;                // temporal_cap of launch_rules.h
  if (n <= 3) launches<FMT, 3>(wg, in, a, out, stats);
  else if (n <= 5) launches<FMT, 5>(wg, in, a, out, stats);
  else if (n <= 9) launches<FMT, 9>(wg, in, a, out, stats);
  else launches<FMT, TP_MAX_WINDOW>(wg, in, a, out, stats);
}

template <int FMT>
static int run(TpArgs a, char** path) {
  const size_t e = fl_elem_bytes(FMT), bytes = (size_t)a.T * a.h * a.w * e, stats_bytes = sizeof(unsigned) * a.T * TP_STATS;
  char* first = nullptr;
  unsigned* first_stats = nullptr;
  for (int skew = 1; skew >= 0; --skew) {            // one element into larger buffers, then on a 16-byte boundary
    const size_t lead = skew * e, whole = bytes + 2 * lead;
    char* src = (char*)memset(hc_aligned(whole), 0x77, whole);
    hc_read(path[0], bytes, lead, src);
    a.vec = ((long)a.h * a.w) % TP_PER == 0 && skew == 0;
    for (int rev = 0; rev < 2; ++rev)
      for (int with = 1; with >= 0; --with) {
        char* out = (char*)memset(hc_aligned(whole), 0xEE, whole);
        unsigned* stats = with ? hc_alloc<unsigned>(stats_bytes, 0xEE) : nullptr;
        caps<FMT>(WgHost{TP_THREADS, rev != 0}, src + lead, a, out + lead, stats);
        for (size_t i = 0; i < lead; ++i)
          if ((unsigned char)out[i] != 0xEE || (unsigned char)out[lead + bytes + i] != 0xEE) hc_die("an element beside `out` was written");
        if (!first) {
          first = out, first_stats = stats;
          continue;
        }
        hc_same(first + e, out + lead, bytes, "the output depends on the thread order, the statistics pointer or the alignment");
        if (with) hc_same(first_stats, stats, stats_bytes, "the statistics depend on the thread order or the alignment");
        free(out), free(stats);
      }
    for (size_t i = 0; i < lead; ++i)
      if (src[i] != 0x77 || src[lead + bytes + i] != 0x77) hc_die("an element beside `in` was written");
    free(src);
  }
  hc_write(path[1], first + e, bytes);
  hc_write(path[2], first_stats, stats_bytes);
  free(first), free(first_stats);
  return 0;
}

int main(int argc, char** argv) {
  hc_name = "temporal_host_check";
  if (argc != 15) hc_die("usage: temporal_host_check <fmt 0|1> T h w Bk Ah A Rq M F chunk in.bin out.bin stats.bin");
  const int fmt = atoi(argv[1]);
  TpArgs a;
  a.T = atoi(argv[2]), a.h = atoi(argv[3]), a.w = atoi(argv[4]), a.back = atoi(argv[5]), a.ahead = atoi(argv[6]);
  const int A = atoi(argv[7]), Rq = atoi(argv[8]);
  a.min_count = atoi(argv[9]), a.min_fill = atoi(argv[10]), a.chunk = atoi(argv[11]), a.vec = 0;
  if (a.T < 1 || a.T > TP_MAX_FRAMES || a.h < 1 || a.h > TP_MAX_SIDE || a.w < 1 || a.w > TP_MAX_SIDE || a.back < 0 || a.ahead < 0 ||
      a.back + a.ahead >= TP_MAX_WINDOW || A < 0 || A > 65535 || Rq < 0 || Rq > TP_MAX_REL || a.min_count < 1 ||
      a.min_count > TP_MAX_WINDOW || a.min_fill < 0 || a.min_fill > TP_MAX_WINDOW || a.chunk < 1 || a.chunk > a.T)
    return 2;
  a.tol_abs = (unsigned)A, a.tol_rel = (unsigned)Rq;
  char* path[3] = {argv[12], argv[13], argv[14]};
  if (fmt == FL_U8) return run<FL_U8>(a, path);
  if (fmt == FL_U16) return run<FL_U16>(a, path);
  return 2;
}
