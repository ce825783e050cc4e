// Host-side check of the point clouds with normals: the launch plan and the three workgroup bodies of
// csrc/cloud_tile.h -- the very text the device kernels of csrc/cloud.hip call -- compiled for the host and run workgroup by
// workgroup of the three launches over exactly-sized heap buffers (the LDS arrays too), so that the address and
// undefined-behaviour sanitizers see every access.  The body and the normal map start ONE BYTE into their buffers, so the staged
// 4-byte stores run on an odd base address.  Every case runs with the threads of a workgroup forwards and backwards, and the
// outputs must agree.  No GPU, no HIP, nothing loaded into Python.
// `python tools/host_check.py cloud` builds this, runs it over the GPU test's cases and compares what it writes with
// tests/cloud_ref.py, byte for byte.
//
//   cloud_host_check <fmt 0|1> B h w <normals 0|1> <channels 0|1|3> R A Rq m <map 0|1> in.bin rx.bin ry.bin color.bin body.bin
//                    counts.bin map.bin
//     in.bin: (B, h, w) codes; rx.bin (w), ry.bin (h): int32; color.bin: (B, h, w, channels) u8 (not read for channels 0)
//     -> body.bin: (B, h w rec) bytes, 0xEE where nothing was written; counts.bin: (B, 2) uint32; map.bin: (B, h, w, 3) u8
#include "host_check.h"

#include "../codon_amd/csrc/cloud_tile.h"

using namespace codon;

struct Case {
  int B, map;
  CdArgs a;
  const void* in;
  const int *rx, *ry;
  const unsigned char* color;
};

// cloud_launch<FMT> and cloud_emit<FMT, REC>
template <int FMT, int REC>
static void launches(WgHost wg, const Case& c, unsigned char* body, unsigned* counts, unsigned char* nmap) {
  const CdPlan p = cd_plan(c.a.h, c.a.w);
  unsigned* ws = hc_alloc<unsigned>(sizeof(unsigned) * cd_workspace_words(c.B, c.a.h, c.a.w), 0xEE);
  for (long b = 0; b < c.B; ++b)
    for (long r = 0; r < p.blocks; ++r) {
      unsigned* cnt = hc_alloc<unsigned>(sizeof(unsigned) * CD_THREADS, 0xCD);
      unsigned* part = hc_alloc<unsigned>(sizeof(unsigned) * CD_PARTS, 0xCD);
      wg_cloud_count<FMT>(wg, r, b, c.in, c.a.h, c.a.w, ws, cnt, part);
      free(cnt), free(part);
    }
  for (long b = 0; b < c.B; ++b) {
    unsigned* cnt = hc_alloc<unsigned>(sizeof(unsigned) * CD_SCAN_THREADS, 0xCD);
    unsigned* part = hc_alloc<unsigned>(sizeof(unsigned) * 16, 0xCD);
    wg_cloud_scan(WgHost{CD_SCAN_THREADS, wg.reverse}, b, c.a.h, c.a.w, ws, counts, cnt, part);
    free(cnt), free(part);
  }
  for (long b = 0; b < c.B; ++b)
    for (long r = 0; r < p.blocks; ++r) {
      unsigned* cnt = hc_alloc<unsigned>(sizeof(unsigned) * CD_THREADS, 0xCD);
      unsigned* ncnt = hc_alloc<unsigned>(sizeof(unsigned) * CD_THREADS, 0xCD);
      unsigned* part = hc_alloc<unsigned>(sizeof(unsigned) * CD_PARTS, 0xCD);
      unsigned* npart = hc_alloc<unsigned>(sizeof(unsigned) * CD_PARTS, 0xCD);
      unsigned* stage = hc_alloc<unsigned>(sizeof(unsigned) * cd_stage_words(REC), 0xCD);
      wg_cloud_emit<FMT, REC>(wg, r, b, c.in, c.a, c.rx, c.ry, c.color, body, counts, nmap, ws, cnt, ncnt, part, npart, stage);
      free(cnt), free(ncnt), free(part), free(npart), free(stage);
    }
  free(ws);
}

template <int FMT, int REC>
static int run(Case c, char** path) {
  const size_t n = (size_t)c.a.h * c.a.w, bytes = (size_t)c.B * n * REC, map_bytes = (size_t)c.B * n * 3;
  const size_t counts_bytes = sizeof(unsigned) * c.B * CD_COUNTS;
  c.in = hc_read(path[0], (size_t)c.B * n * fl_elem_bytes(FMT));
  c.rx = hc_read<int>(path[1], sizeof(int) * c.a.w);
  c.ry = hc_read<int>(path[2], sizeof(int) * c.a.h);
  c.color = cd_rec_color(REC) ? hc_read<unsigned char>(path[3], (size_t)c.B * n * c.a.channels) : nullptr;
  unsigned char *body[2], *nmap[2] = {nullptr, nullptr};
  unsigned* counts[2];
  for (int rev = 0; rev < 2; ++rev) {
    body[rev] = hc_alloc<unsigned char>(1 + bytes, 0xEE);             // the records start one byte in
    counts[rev] = hc_alloc<unsigned>(counts_bytes, 0xEE);
    if (c.map) nmap[rev] = hc_alloc<unsigned char>(1 + map_bytes, 0xEE);
    launches<FMT, REC>(WgHost{CD_THREADS, rev != 0}, c, body[rev] + 1, counts[rev], c.map ? nmap[rev] + 1 : nullptr);
    if (body[rev][0] != 0xEE || (c.map && nmap[rev][0] != 0xEE)) hc_die("the byte before an output was written");
  }
  hc_same(body[0], body[1], 1 + bytes, "the records depend on the order of the threads within a phase");
  hc_same(counts[0], counts[1], counts_bytes, "the counts depend on the order of the threads within a phase");
  if (c.map) hc_same(nmap[0], nmap[1], 1 + map_bytes, "the normal map depends on the order of the threads within a phase");
  hc_write(path[4], body[0] + 1, bytes);
  hc_write(path[5], counts[0], counts_bytes);
  if (c.map) hc_write(path[6], nmap[0] + 1, map_bytes);
  free((void*)c.in), free((void*)c.rx), free((void*)c.ry), free((void*)c.color);
  for (int rev = 0; rev < 2; ++rev) free(body[rev]), free(counts[rev]), free(nmap[rev]);
  return 0;
}

template <int FMT>
static int run_form(const Case& c, int normals, char** path) {
  if (c.a.channels) return normals ? run<FMT, cd_rec(true, true)>(c, path) : run<FMT, cd_rec(false, true)>(c, path);
  return normals ? run<FMT, cd_rec(true, false)>(c, path) : run<FMT, cd_rec(false, false)>(c, path);
}

int main(int argc, char** argv) {
  hc_name = "cloud_host_check";
  if (argc != 19)
    hc_die("usage: cloud_host_check <fmt 0|1> B h w <normals 0|1> <channels 0|1|3> R A Rq m <map 0|1> in.bin rx.bin ry.bin color.bin "
           "body.bin counts.bin map.bin");
  const int fmt = atoi(argv[1]), normals = atoi(argv[5]), R = atoi(argv[7]), A = atoi(argv[8]), Rq = atoi(argv[9]);
  Case c;
  c.B = atoi(argv[2]), c.map = atoi(argv[11]);
  c.a.h = atoi(argv[3]), c.a.w = atoi(argv[4]), c.a.channels = atoi(argv[6]), c.a.m = atof(argv[10]);
  if (c.B < 1 || c.a.h < 1 || c.a.h > CD_MAX_SIDE || c.a.w < 1 || c.a.w > CD_MAX_SIDE || (normals != 0 && normals != 1) ||
      (c.a.channels != 0 && c.a.channels != 1 && c.a.channels != 3) || R < 1 || R > CD_MAX_RADIUS || A < 0 || A > 65535 || Rq < 0 ||
      Rq > CD_MAX_REL || !(c.a.m > 0.0) || (c.map && !normals))
    return 2;
  c.a.radius = normals ? R : 0, c.a.tol_abs = (unsigned)(R * A), c.a.tol_rel = (unsigned)Rq;
  if (fmt == FL_U8) return run_form<FL_U8>(c, normals, argv + 12);
  if (fmt == FL_U16) return run_form<FL_U16>(c, normals, argv + 12);
  return 2;
}
