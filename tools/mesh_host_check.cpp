// Host-side check of the triangle meshes: the launch plan and the workgroup bodies of csrc/mesh_tile.h, with
// the two of csrc/cloud_tile.h they follow -- the very text the device kernels of csrc/cloud.hip call -- compiled for the host and
// run workgroup by workgroup of the six launches over exactly-sized heap buffers (the LDS arrays too), so that the address and
// undefined-behaviour sanitizers see every access.  The face buffer starts ONE BYTE into its allocation, so the staged 4-byte stores
// run on an odd base address.  Every case runs with the threads of a workgroup forwards and backwards, and the outputs must agree.
// No GPU, no HIP, nothing loaded into Python.
// `python tools/host_check.py mesh` builds this, runs it over the GPU test's cases and compares what it writes with
// tests/mesh_ref.py, byte for byte.
//
//   mesh_host_check <fmt 0|1> B h w A Rq in.bin faces.bin counts.bin
//     in.bin: (B, h, w) codes -> faces.bin: (B, 2 (h - 1) (w - 1) 13) bytes, 0xEE where nothing was written; counts.bin: (B) uint32
#include "host_check.h"

#include "../codon_amd/csrc/mesh_tile.h"

using namespace codon;

// mesh_launch<FMT>
template <int FMT>
static void launches(bool reverse, int B, const MsArgs& a, const void* in, unsigned char* faces, unsigned* counts) {
  const CdPlan c = cd_plan(a.h, a.w);
  const MsPlan p = ms_plan(a.h, a.w);
  const MsSpace s = ms_space(B, a.h, a.w);
  unsigned* ws = hc_alloc<unsigned>(sizeof(unsigned) * s.words, 0xEE);
  unsigned *blocks = ws + s.blocks, *runs = ws + s.runs, *points = ws + s.counts;
  int* index = (int*)(ws + s.index);
  const WgHost pixels{CD_THREADS, reverse}, quads{MS_THREADS, reverse}, scan{CD_SCAN_THREADS, reverse};
  if (p.runs > 0) {
    for (long b = 0; b < B; ++b)
      for (long r = 0; r < c.blocks; ++r) {
        unsigned* cnt = hc_alloc<unsigned>(sizeof(unsigned) * CD_THREADS, 0xCD);
        unsigned* part = hc_alloc<unsigned>(sizeof(unsigned) * CD_PARTS, 0xCD);
        wg_cloud_count<FMT>(pixels, r, b, in, a.h, a.w, blocks, cnt, part);
        free(cnt), free(part);
      }
    for (long b = 0; b < B; ++b) {
      unsigned* cnt = hc_alloc<unsigned>(sizeof(unsigned) * CD_SCAN_THREADS, 0xCD);
      unsigned* part = hc_alloc<unsigned>(sizeof(unsigned) * 16, 0xCD);
      wg_cloud_scan(scan, b, a.h, a.w, blocks, points, cnt, part);
      free(cnt), free(part);
    }
    for (long b = 0; b < B; ++b)
      for (long r = 0; r < c.blocks; ++r) {
        unsigned* cnt = hc_alloc<unsigned>(sizeof(unsigned) * CD_THREADS, 0xCD);
        unsigned* part = hc_alloc<unsigned>(sizeof(unsigned) * CD_PARTS, 0xCD);
        wg_mesh_index<FMT>(pixels, r, b, in, a.h, a.w, blocks, index, cnt, part);
        free(cnt), free(part);
      }
    for (long b = 0; b < B; ++b)
      for (long r = 0; r < p.runs; ++r) {
        unsigned* cnt = hc_alloc<unsigned>(sizeof(unsigned) * MS_THREADS, 0xCD);
        unsigned* part = hc_alloc<unsigned>(sizeof(unsigned) * MS_PARTS, 0xCD);
        wg_mesh_count<FMT>(quads, r, b, in, a, runs, cnt, part);
        free(cnt), free(part);
      }
  }
  for (long b = 0; b < B; ++b) {
    unsigned* cnt = hc_alloc<unsigned>(sizeof(unsigned) * CD_SCAN_THREADS, 0xCD);
    unsigned* part = hc_alloc<unsigned>(sizeof(unsigned) * 16, 0xCD);
    wg_mesh_scan(scan, b, a.h, a.w, runs, counts, cnt, part);
    free(cnt), free(part);
  }
  for (long b = 0; b < B; ++b)
    for (long r = 0; r < p.runs; ++r) {
      unsigned* cnt = hc_alloc<unsigned>(sizeof(unsigned) * MS_THREADS, 0xCD);
      unsigned* part = hc_alloc<unsigned>(sizeof(unsigned) * MS_PARTS, 0xCD);
      unsigned* stage = hc_alloc<unsigned>(sizeof(unsigned) * MS_STAGE_WORDS, 0xCD);
      wg_mesh_emit<FMT>(quads, r, b, in, a, index, runs, faces, cnt, part, stage);
      free(cnt), free(part), free(stage);
    }
  free(ws);
}

template <int FMT>
static int run(int B, const MsArgs& a, char** path) {
  const size_t n = (size_t)a.h * a.w, bytes = (size_t)B * ms_face_bytes(a.h, a.w), counts_bytes = sizeof(unsigned) * B;
  const void* in = hc_read(path[0], (size_t)B * n * fl_elem_bytes(FMT));
  unsigned char* faces[2];
  unsigned* counts[2];
  for (int rev = 0; rev < 2; ++rev) {
    faces[rev] = hc_alloc<unsigned char>(1 + bytes, 0xEE);            // the records start one byte in
    counts[rev] = hc_alloc<unsigned>(counts_bytes, 0xEE);
    launches<FMT>(rev != 0, B, a, in, faces[rev] + 1, counts[rev]);
    if (faces[rev][0] != 0xEE) hc_die("the byte before the faces was written");
  }
  hc_same(faces[0], faces[1], 1 + bytes, "the faces depend on the order of the threads within a phase");
  hc_same(counts[0], counts[1], counts_bytes, "the counts depend on the order of the threads within a phase");
  hc_write(path[1], faces[0] + 1, bytes);
  hc_write(path[2], counts[0], counts_bytes);
  free((void*)in);
  for (int rev = 0; rev < 2; ++rev) free(faces[rev]), free(counts[rev]);
  return 0;
}

int main(int argc, char** argv) {
  hc_name = "mesh_host_check";
  if (argc != 10) hc_die("usage: mesh_host_check <fmt 0|1> B h w A Rq in.bin faces.bin counts.bin");
  const int fmt = atoi(argv[1]), B = atoi(argv[2]), A = atoi(argv[5]), Rq = atoi(argv[6]);
  MsArgs a;
  a.h = atoi(argv[3]), a.w = atoi(argv[4]);
  if (B < 1 || a.h < 1 || a.h > MS_MAX_SIDE || a.w < 1 || a.w > MS_MAX_SIDE || A < 0 || A > 65535 || Rq < 0 || Rq > MS_MAX_REL) return 2;
  a.tol_abs = (unsigned)A, a.tol_rel = (unsigned)Rq;
  if (fmt == FL_U8) return run<FL_U8>(B, a, argv + 7);
  if (fmt == FL_U16) return run<FL_U16>(B, a, argv + 7);
  return 2;
}
