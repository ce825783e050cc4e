// Host-side check of the depth registration: the launch plan and the workgroup bodies of
// csrc/register_tile.h -- the very text the device kernels of csrc/register.hip call -- compiled for the host and run workgroup by
// workgroup of the three launches over exactly-sized heap buffers (the LDS arrays too), so that the address and undefined-behaviour
// sanitizers see every access.  Every case runs with the threads of a workgroup forwards and backwards, and the two outputs must
// agree: the minimum and the counts do not depend on the order.  No GPU, no HIP, nothing loaded into Python.
// `python tools/host_check.py register` builds this, runs it over the GPU test's cases and compares what it writes with
// tests/register_ref.py, bit for bit.
//
//   register_host_check <fmt 0|1> B hs ws top ho wo in.bin rays.bin params.bin out.bin stats.bin
//     in.bin: (B, hs, ws) codes; rays.bin: (hs + 1, ws + 1, 3) int32; params.bin: 7 int64, T[3] and FX, FY, CX, CY
//     ->  out.bin: (B, ho, wo) codes; stats.bin: (B, 4) uint32
#include "host_check.h"

#include "../codon_amd/csrc/register_tile.h"

using namespace codon;

// register_launch<FMT>
template <int FMT>
static void launches(WgHost wg, int B, const void* in, const int* rays, const RgArgs& a, void* out, unsigned* stats) {
  const RgPlan p = rg_plan(a.hs, a.ws, a.ho, a.wo);
  unsigned* zb = hc_alloc<unsigned>(sizeof(unsigned) * p.stride * B, 0xEE);
  for (long r = 0; r < rg_init_runs(p, B); ++r) wg_register_init(wg, r, zb, p.stride * B, stats, B * RG_STATS);
  for (long b = 0; b < B; ++b)
    for (int ty = 0; ty < p.sy; ++ty)
      for (int tx = 0; tx < p.sx; ++tx) {
        int* la = hc_alloc<int>(sizeof(int) * RG_CORNERS * 3, 0xCD);
        unsigned* cnt = hc_alloc<unsigned>(sizeof(unsigned) * RG_THREADS, 0xCD);
        unsigned* part = hc_alloc<unsigned>(sizeof(unsigned) * 16, 0xCD);
        wg_register_splat<FMT>(wg, tx, ty, b, in, rays, a, zb, p.stride, stats, la, cnt, part);
        free(la), free(cnt), free(part);
      }
  for (long b = 0; b < B; ++b)
    for (long r = 0; r < p.rx; ++r) {
      unsigned* cnt = hc_alloc<unsigned>(sizeof(unsigned) * RG_THREADS, 0xCD);
      unsigned* part = hc_alloc<unsigned>(sizeof(unsigned) * 16, 0xCD);
      wg_register_resolve<FMT>(wg, r, b, zb, p.stride, a.ho, a.wo, out, stats, cnt, part);
      free(cnt), free(part);
    }
  free(zb);
}

template <int FMT>
static int run(int B, const RgArgs& a, char** path) {
  const size_t in_bytes = (size_t)B * a.hs * a.ws * fl_elem_bytes(FMT), out_bytes = (size_t)B * a.ho * a.wo * fl_elem_bytes(FMT);
  const size_t stats_bytes = sizeof(unsigned) * B * RG_STATS;
  void* in = hc_read(path[0], in_bytes);
  int* rays = hc_read<int>(path[1], sizeof(int) * (a.hs + 1) * (a.ws + 1) * 3);
  void* out[2];
  unsigned* stats[2];
  for (int rev = 0; rev < 2; ++rev) {
    out[rev] = memset(hc_aligned(out_bytes), 0xEE, out_bytes);
    stats[rev] = hc_alloc<unsigned>(stats_bytes, 0xEE);
    launches<FMT>(WgHost{RG_THREADS, rev != 0}, B, in, rays, a, out[rev], stats[rev]);
  }
  hc_same(out[0], out[1], out_bytes, "the output depends on the order of the threads within a phase");
  hc_same(stats[0], stats[1], stats_bytes, "the statistics depend on the order of the threads within a phase");
  // without statistics: the same codes
  void* bare = memset(hc_aligned(out_bytes), 0xEE, out_bytes);
  launches<FMT>(WgHost{RG_THREADS, false}, B, in, rays, a, bare, nullptr);
  hc_same(out[0], bare, out_bytes, "the output differs when no statistics are asked for");
  hc_write(path[3], out[0], out_bytes);
  hc_write(path[4], stats[0], stats_bytes);
  free(in);
  free(rays);
  free(bare);
  for (int rev = 0; rev < 2; ++rev) free(out[rev]), free(stats[rev]);
  return 0;
}

int main(int argc, char** argv) {
  hc_name = "register_host_check";
  if (argc != 13) hc_die("usage: register_host_check <fmt 0|1> B hs ws top ho wo in.bin rays.bin params.bin out.bin stats.bin");
  const int fmt = atoi(argv[1]), B = atoi(argv[2]);
  RgArgs a;
  a.hs = atoi(argv[3]), a.ws = atoi(argv[4]), a.top = atoi(argv[5]), a.ho = atoi(argv[6]), a.wo = atoi(argv[7]);
  if (B < 1 || a.hs < 1 || a.hs > RG_MAX_SIDE || a.ws < 1 || a.ws > RG_MAX_SIDE || a.ho < 1 || a.ho > RG_MAX_SIDE || a.wo < 1 ||
      a.wo > RG_MAX_SIDE || a.top < 1 || a.top > 65535)
    return 2;
  long long* par = hc_read<long long>(argv[10], sizeof(long long) * 7);
  a.tx = par[0], a.ty = par[1], a.tz = par[2];
  a.fx = (int)par[3], a.fy = (int)par[4], a.cx = (int)par[5], a.cy = (int)par[6];
  free(par);
  char* path[5] = {argv[8], argv[9], argv[10], argv[11], argv[12]};
  if (fmt == FL_U8) return run<FL_U8>(B, a, path);
  if (fmt == FL_U16) return run<FL_U16>(B, a, path);
  return 2;
}
