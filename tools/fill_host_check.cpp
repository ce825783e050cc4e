// Host-side check of the pull-push hole filler: the launch plan and the workgroup bodies of csrc/fill_tile.h
// -- the very text the device kernels of csrc/fill_holes.hip call -- compiled for the host and run workgroup by workgroup of
// every launch over exactly-sized heap buffers (the LDS arrays too), so that the address and undefined-behaviour sanitizers see
// every access.  Every case runs with the threads of a workgroup forwards and backwards, and the two outputs must agree.  No GPU,
// no HIP, nothing loaded into Python.  `python tools/host_check.py fill` builds this, runs it over the GPU tests' shapes,
// patterns and formats and compares what it writes with tests/fill_ref.py, bit for bit.
//
//   fill_host_check <fmt 0|1|2> B h w top in.bin tab.bin|- out.bin
//     in.bin: (B, h, w) elements of the format; tab.bin: top + 1 fp32 (format 2 only)  ->  out.bin: (B, h, w) elements
#include "host_check.h"

#include "../codon_amd/csrc/fill_tile.h"

using namespace codon;

// fill_launch<FMT>
template <int FMT>
static void launches(WgHost wg, int B, int h, int w, int top, const void* in, const float* tab, void* out) {
  const FlPlan p = fl_plan(h, w);
  if (p.single) {
    for (long b = 0; b < B; ++b) {
      unsigned short* pyr = hc_alloc<unsigned short>(sizeof(unsigned short) * FL_PYR_CELLS, 0xCD);
      wg_fill_plane<FMT>(wg, b, in, (long)h * w, out, (long)h * w, h, w, tab, top, pyr);
      free(pyr);
    }
    return;
  }
  unsigned short* ws = hc_alloc<unsigned short>(sizeof(unsigned short) * B * p.stride, 0xEE);
  for (long b = 0; b < B; ++b)
    for (int ty = 0; ty < p.gy; ++ty)
      for (int tx = 0; tx < p.gx; ++tx) {
        unsigned short* pyr = hc_alloc<unsigned short>(sizeof(unsigned short) * FL_PYR_CELLS, 0xCD);
        wg_fill_pull<FMT>(wg, tx, ty, b, in, h, w, top, ws, p.stride, pyr);
        free(pyr);
      }
  unsigned short* l6 = ws + p.l6;
  for (long b = 0; b < B; ++b) {
    unsigned short* pyr = hc_alloc<unsigned short>(sizeof(unsigned short) * FL_PYR_CELLS, 0xCD);
    wg_fill_plane<FL_U16>(wg, b, l6, p.stride, l6, p.stride, p.h6, p.w6, nullptr, 65535, pyr);
    free(pyr);
  }
  for (long b = 0; b < B; ++b)
    for (int ty = 0; ty < p.gy; ++ty)
      for (int tx = 0; tx < p.gx; ++tx) {
        unsigned short* hp = hc_alloc<unsigned short>(sizeof(unsigned short) * FL_HALO_CELLS, 0xCD);
        wg_fill_push<FMT>(wg, tx, ty, b, in, out, h, w, tab, top, ws, p.stride, hp);
        free(hp);
      }
  free(ws);
}

template <int FMT>
static int run(int B, int h, int w, int top, const char* fin, const char* ftab, const char* fout) {
  const size_t bytes = (size_t)B * h * w * fl_elem_bytes(FMT);
  void* in = hc_read(fin, bytes);
  float* tab = FMT == FL_F32 ? hc_read<float>(ftab, ((size_t)top + 1) * sizeof(float)) : nullptr;
  void* out[2];
  for (int rev = 0; rev < 2; ++rev) {
    out[rev] = hc_alloc(bytes, 0xEE);
    launches<FMT>(WgHost{FL_THREADS, rev != 0}, B, h, w, top, in, tab, out[rev]);
  }
  hc_same(out[0], out[1], bytes, "the output depends on the order of the threads within a phase");
  hc_write(fout, out[0], bytes);
  free(in);
  free(tab);
  free(out[0]);
  free(out[1]);
  return 0;
}

int main(int argc, char** argv) {
  hc_name = "fill_host_check";
  if (argc != 9) hc_die("usage: fill_host_check <fmt 0|1|2> B h w top in.bin tab.bin|- out.bin");
  const int fmt = atoi(argv[1]), B = atoi(argv[2]), h = atoi(argv[3]), w = atoi(argv[4]), top = atoi(argv[5]);
  if (B < 1 || h < 1 || h > FL_MAX_SIDE || w < 1 || w > FL_MAX_SIDE || top < 1 || top > 65535) return 2;
  if (fmt == FL_U8) return run<FL_U8>(B, h, w, top, argv[6], argv[7], argv[8]);
  if (fmt == FL_U16) return run<FL_U16>(B, h, w, top, argv[6], argv[7], argv[8]);
  if (fmt == FL_F32) return run<FL_F32>(B, h, w, top, argv[6], argv[7], argv[8]);
  return 2;
}
