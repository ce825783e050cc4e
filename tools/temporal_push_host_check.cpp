// Host-side check of the temporal filter of a depth stream: the workgroup bodies of csrc/temporal_tile.h --
// the very text the device kernels of csrc/temporal_push.hip call -- compiled for the host and run step by step, workgroup by
// workgroup of the two launches of a step, over exactly-sized heap buffers (the ring of 16 planes, the two state words, every
// frame's `in` and `out`, the statistics row and the two arrays of the sums), so that the address and undefined-behaviour
// sanitizers see every access.  A sequence is pushed frame by frame and flushed; one flush step more than the stream owes must
// write nothing.  `in` and `out` stand ONE ELEMENT into larger buffers: the four-pixel loads and stores are then off their
// alignment and the body must take the element path, and the elements before and behind stay as they were; a second pass with
// both on a 16-byte boundary takes the four-pixel path where the plane allows it.  Every case runs with the threads of a
// workgroup forwards and backwards, and with and without statistics, and the outputs must agree.  A step that emits nothing must
// leave `out` as it was and the row at 0.  No GPU, no HIP, nothing loaded into Python.
// `python tools/host_check.py temporal_push` builds this, runs it over the GPU test's cases (tests/temporal_stream_cases.py) and
// compares what it writes with tests/temporal_ref.py on the whole sequence, bit for bit.
//
//   temporal_push_host_check <fmt 0|1> T h w Bk Ah A Rq M F in.bin out.bin stats.bin
//     in.bin: (T, h, w) codes  ->  out.bin: (T, h, w) codes; stats.bin: (T, 4) uint32
#include "host_check.h"

#include "../codon_amd/csrc/temporal_tile.h"

using namespace codon;

// temporal_push_launch<FMT, CAP>: the two launches of one step
template <int FMT, int CAP>
static void step(WgHost wg, const void* in, const TpArgs& a, void* ring, unsigned* state, void* out, unsigned* stats) {
  wg_temporal_push_begin(wg, in ? 1 : 0, state, stats);
  const long groups = ((long)a.h * a.w + TP_TILE - 1) / TP_TILE;     // temporal_push_groups of launch_rules.h
  for (long gx = 0; gx < groups; ++gx) {
    unsigned* cnt = hc_alloc<unsigned>(sizeof(unsigned) * 2 * TP_THREADS, 0xCD);
    unsigned* part = hc_alloc<unsigned>(sizeof(unsigned) * 32, 0xCD);
    wg_temporal_push<FMT, CAP>(wg, gx, in, a, ring, state, out, stats, cnt, part);
    free(cnt), free(part);
  }
}

template <int FMT>
static void caps(WgHost wg, const void* in, const TpArgs& a, void* ring, unsigned* state, void* out, unsigned* stats) {
  const int n = a.back + a.ahead + 1;                // temporal_cap of launch_rules.h
  if (n <= 3) step<FMT, 3>(wg, in, a, ring, state, out, stats);
  else if (n <= 5) step<FMT, 5>(wg, in, a, ring, state, out, stats);
  else if (n <= 9) step<FMT, 9>(wg, in, a, ring, state, out, stats);
  else step<FMT, TP_MAX_WINDOW>(wg, in, a, ring, state, out, stats);
}

static bool all_bytes(const char* p, size_t n, int v) {
  for (size_t i = 0; i < n; ++i)
    if ((unsigned char)p[i] != (unsigned char)v) return false;
  return true;
}

// one stream of a.T frames from `seq`: frames to `res` (T planes) and rows to `rows` (T x 4, where with)
template <int FMT>
static void stream(WgHost wg, TpArgs a, const char* seq, size_t lead, bool with, char* res, unsigned* rows) {
  const size_t e = fl_elem_bytes(FMT), plane = (size_t)a.h * a.w * e, whole = plane + 2 * lead;
  char* ring = (char*)memset(hc_aligned(TP_SLOTS * plane), 0xCD, TP_SLOTS * plane);
  unsigned* state = hc_alloc<unsigned>(sizeof(unsigned) * TP_STATE, 0);            // a stream opens at (0, 0)
  const int T = a.T, owed = a.ahead < T ? a.ahead : T;
  int emitted = 0;
  for (int s = 0; s < T + owed + 1; ++s) {           // T pushes, the flush steps the stream owes, and one more
    const bool push = s < T, final = push ? s >= a.ahead : s < T + owed;
    char* src = nullptr;
    if (push) {
      src = (char*)memset(hc_aligned(whole), 0x77, whole);
      memcpy(src + lead, seq + (size_t)s * plane, plane);
    }
    char* out = (char*)memset(hc_aligned(whole), 0xEE, whole);
    unsigned* stats = with ? hc_alloc<unsigned>(sizeof(unsigned) * TP_STATS, 0xEE) : nullptr;
    caps<FMT>(wg, push ? src + lead : nullptr, a, ring, state, out + lead, stats);
    if (!all_bytes(out, lead, 0xEE) || !all_bytes(out + lead + plane, lead, 0xEE)) hc_die("an element beside `out` was written");
    if (push && (!all_bytes(src, lead, 0x77) || !all_bytes(src + lead + plane, lead, 0x77) ||
                 memcmp(src + lead, seq + (size_t)s * plane, plane) != 0))
      hc_die("`in` or an element beside it was written");
    if (final) {
      memcpy(res + (size_t)emitted * plane, out + lead, plane);
      if (with) memcpy(rows + (size_t)emitted * TP_STATS, stats, sizeof(unsigned) * TP_STATS);
      ++emitted;
    } else {
      if (!all_bytes(out + lead, plane, 0xEE)) hc_die("a step that emits no frame wrote `out`");
      if (with && !all_bytes((const char*)stats, sizeof(unsigned) * TP_STATS, 0)) hc_die("a step that emits no frame left counts");
    }
    if (state[TP_PUSHED] != (unsigned)(push ? s + 1 : T) || state[TP_FLUSHED] != (unsigned)(push ? 0 : s - T + 1))
      hc_die("the state words are not (frames pushed, flush steps since the last push)");
    free(src), free(out), free(stats);
  }
  if (emitted != T) hc_die("a stream of T frames did not emit T frames");
  free(ring), free(state);
}

template <int FMT>
static int run(TpArgs a, char** path) {
  const size_t e = fl_elem_bytes(FMT), bytes = (size_t)a.T * a.h * a.w * e, stats_bytes = sizeof(unsigned) * a.T * TP_STATS;
  char* seq = hc_read<char>(path[0], bytes);
  char* first = nullptr;
  unsigned* first_stats = nullptr;
  for (int skew = 1; skew >= 0; --skew) {            // one element into larger buffers, then on a 16-byte boundary
    a.vec = ((long)a.h * a.w) % TP_PER == 0 && skew == 0;
    for (int rev = 0; rev < 2; ++rev)
      for (int with = 1; with >= 0; --with) {
        char* res = hc_alloc<char>(bytes, 0xEE);
        unsigned* rows = with ? hc_alloc<unsigned>(stats_bytes, 0xEE) : nullptr;
        stream<FMT>(WgHost{TP_THREADS, rev != 0}, a, seq, skew * e, with != 0, res, rows);
        if (!first) {
          first = res, first_stats = rows;
          continue;
        }
        hc_same(first, res, bytes, "the output depends on the thread order, the statistics pointer or the alignment");
        if (with) hc_same(first_stats, rows, stats_bytes, "the statistics depend on the thread order or the alignment");
        free(res), free(rows);
      }
  }
  hc_write(path[1], first, bytes);
  hc_write(path[2], first_stats, stats_bytes);
  free(first), free(first_stats), free(seq);
  return 0;
}

int main(int argc, char** argv) {
  hc_name = "temporal_push_host_check";
  if (argc != 14) hc_die("usage: temporal_push_host_check <fmt 0|1> T h w Bk Ah A Rq M F in.bin out.bin stats.bin");
  const int fmt = atoi(argv[1]);
  TpArgs a;
  a.T = atoi(argv[2]), a.h = atoi(argv[3]), a.w = atoi(argv[4]), a.back = atoi(argv[5]), a.ahead = atoi(argv[6]);
  const int A = atoi(argv[7]), Rq = atoi(argv[8]);
  a.min_count = atoi(argv[9]), a.min_fill = atoi(argv[10]), a.chunk = 0, a.vec = 0;
  if (a.T < 1 || a.T > TP_MAX_FRAMES || a.h < 1 || a.h > TP_MAX_SIDE || a.w < 1 || a.w > TP_MAX_SIDE || a.back < 0 || a.ahead < 0 ||
      a.back + a.ahead >= TP_MAX_WINDOW || A < 0 || A > 65535 || Rq < 0 || Rq > TP_MAX_REL || a.min_count < 1 ||
      a.min_count > TP_MAX_WINDOW || a.min_fill < 0 || a.min_fill > TP_MAX_WINDOW)
    return 2;
  a.tol_abs = (unsigned)A, a.tol_rel = (unsigned)Rq;
  char* path[3] = {argv[11], argv[12], argv[13]};
  if (fmt == FL_U8) return run<FL_U8>(a, path);
  if (fmt == FL_U16) return run<FL_U16>(a, path);
  return 2;
}
