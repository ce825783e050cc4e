// Host-side check of the outlier rejection of sensor depth maps: the launch plan and the workgroup bodies of
// csrc/clean_tile.h -- the very text the device kernels of csrc/clean.hip call, the union-find's returning minimum and relaxed load
// spelled over the group type -- compiled for the host and run workgroup by workgroup of the two or four launches over
// exactly-sized heap buffers (the LDS arrays too), so that the address and undefined-behaviour sanitizers see every access.  Every
// case runs with the threads of a workgroup forwards and backwards, and with and without statistics, and the outputs must agree:
// counts and component sizes do not depend on the order.  No GPU, no HIP, nothing loaded into Python.
// `python tools/host_check.py clean` builds this, runs it over the GPU test's cases and compares what it writes with
// tests/clean_ref.py, bit for bit.
//
//   clean_host_check <fmt 0|1> B h w A Rq K N in.bin out.bin stats.bin
//     in.bin: (B, h, w) codes  ->  out.bin: (B, h, w) codes; stats.bin: (B, 4) uint32
#include "host_check.h"

#include "../codon_amd/csrc/clean_tile.h"

using namespace codon;

// clean_launch<FMT>
template <int FMT>
static void launches(WgHost wg, int B, const void* in, const ClArgs& a, void* out, unsigned* stats) {
  const ClPlan p = cl_plan(a.h, a.w, a.region);
  unsigned* ws = hc_alloc<unsigned>(sizeof(unsigned) * cl_workspace_words(B, a.h, a.w), 0xEE);
  if (!p.rule2) wg_clean_zero(wg, stats, B * CL_STATS);
  for (long b = 0; b < B; ++b)
    for (int ty = 0; ty < p.sy; ++ty)
      for (int tx = 0; tx < p.sx; ++tx) {
        unsigned* cell = hc_alloc<unsigned>(sizeof(unsigned) * CL_CELLS, 0xCD);
        unsigned* cnt = hc_alloc<unsigned>(sizeof(unsigned) * 2 * CL_THREADS, 0xCD);
        unsigned* part = hc_alloc<unsigned>(sizeof(unsigned) * 32, 0xCD);
        unsigned* kk = hc_alloc<unsigned>(sizeof(unsigned) * CL_THREADS, 0xCD);
        unsigned* loc = hc_alloc<unsigned>(sizeof(unsigned) * CL_THREADS, 0xCD);
        wg_clean_flying<FMT>(wg, tx, ty, b, B, in, a, out, ws, stats, cell, cnt, part, kk, loc);
        free(cell), free(cnt), free(part), free(kk), free(loc);
      }
  if (p.rule2) {
    for (long b = 0; b < B; ++b)
      for (int ty = 0; ty < p.sy; ++ty)
        for (int tx = 0; tx < p.sx; ++tx) wg_clean_link<FMT>(wg, tx, ty, b, out, a, ws);
    for (long b = 0; b < B; ++b)
      for (int ty = 0; ty < p.sy; ++ty)
        for (int tx = 0; tx < p.sx; ++tx) {
          unsigned* root = hc_alloc<unsigned>(sizeof(unsigned) * CL_THREADS, 0xCD);
          wg_clean_count(wg, tx, ty, b, B, a, ws, root);
          free(root);
        }
    for (long b = 0; b < B; ++b)
      for (long r = 0; r < p.rx; ++r) {
        unsigned* cnt = hc_alloc<unsigned>(sizeof(unsigned) * 2 * CL_THREADS, 0xCD);
        unsigned* part = hc_alloc<unsigned>(sizeof(unsigned) * 32, 0xCD);
        wg_clean_apply<FMT>(wg, r, b, B, in, a, out, ws, stats, cnt, part);
        free(cnt), free(part);
      }
  }
  free(ws);
}

template <int FMT>
static int run(int B, const ClArgs& a, char** path) {
  const size_t bytes = (size_t)B * a.h * a.w * fl_elem_bytes(FMT), stats_bytes = sizeof(unsigned) * B * CL_STATS;
  void* in = hc_read(path[0], bytes);
  void* out[2];
  unsigned* stats[2];
  for (int rev = 0; rev < 2; ++rev) {
    out[rev] = memset(hc_aligned(bytes), 0xEE, bytes);
    stats[rev] = hc_alloc<unsigned>(stats_bytes, 0xEE);
    launches<FMT>(WgHost{CL_THREADS, rev != 0}, B, in, a, out[rev], stats[rev]);
  }
  hc_same(out[0], out[1], bytes, "the output depends on the order of the threads within a phase");
  hc_same(stats[0], stats[1], stats_bytes, "the statistics depend on the order of the threads within a phase");
  // without statistics, in both orders: the same codes
  for (int rev = 0; rev < 2; ++rev) {
    void* bare = memset(hc_aligned(bytes), 0xEE, bytes);
    launches<FMT>(WgHost{CL_THREADS, rev != 0}, B, in, a, bare, nullptr);
    hc_same(out[0], bare, bytes, "the output differs when no statistics are asked for");
    free(bare);
  }
  hc_write(path[1], out[0], bytes);
  hc_write(path[2], stats[0], stats_bytes);
  free(in);
  for (int rev = 0; rev < 2; ++rev) free(out[rev]), free(stats[rev]);
  return 0;
}

int main(int argc, char** argv) {
  hc_name = "clean_host_check";
  if (argc != 12) hc_die("usage: clean_host_check <fmt 0|1> B h w A Rq K N in.bin out.bin stats.bin");
  const int fmt = atoi(argv[1]), B = atoi(argv[2]);
  ClArgs a;
  a.h = atoi(argv[3]), a.w = atoi(argv[4]);
  const int A = atoi(argv[5]), Rq = atoi(argv[6]);
  a.support = atoi(argv[7]), a.region = atoi(argv[8]);
  if (B < 1 || a.h < 1 || a.h > CL_MAX_SIDE || a.w < 1 || a.w > CL_MAX_SIDE || A < 0 || A > 65535 || Rq < 0 || Rq > CL_MAX_REL ||
      a.support < 0 || a.support > CL_MAX_SUPPORT || a.region < 0 || a.region > CL_MAX_REGION)
    return 2;
  a.tol_abs = (unsigned)A, a.tol_rel = (unsigned)Rq;
  char* path[3] = {argv[9], argv[10], argv[11]};
  if (fmt == FL_U8) return run<FL_U8>(B, a, path);
  if (fmt == FL_U16) return run<FL_U16>(B, a, path);
  return 2;
}
