// Host-side check of the guidance-aware hole filler: the launch plan and the workgroup bodies of
// csrc/fill_guided_tile.h -- the very text the device kernels of csrc/fill_guided.hip call -- compiled for the host and run
// workgroup by workgroup of every launch over exactly-sized heap buffers (the LDS arrays too), so that the address and
// undefined-behaviour sanitizers see every access.  Every case runs with the threads of a workgroup forwards and backwards, and
// the two outputs must agree.  No GPU, no HIP, nothing loaded into Python.  `python tools/host_check.py guided_fill` builds this,
// runs it over the GPU tests' shapes, patterns and formats and compares what it writes with tests/guided_fill_ref.py, bit for bit.
//
//   guided_fill_host_check <fmt 0|1> B h w top scale skew pad in.bin guide.bin tab.bin out.bin
//     in.bin: (B, h, w) codes; guide.bin: (B, h * scale, w * scale) u8; tab.bin: 256 u16  ->  out.bin: (B, h, w) codes
//     The guidance is laid out with rows w * scale + pad bytes apart, starting skew bytes into a buffer that ends with the last
//     row's last byte: skew and pad choose the load path (16-byte segments with or without a partial last segment read as
//     4-byte words, 4-byte words throughout, bytes), and a read past a row's end in the last row is a sanitizer report.
#include "host_check.h"

#include "../codon_amd/csrc/fill_guided_tile.h"

using namespace codon;

struct Lds {                      // pointers only: every array is an allocation of its own
  unsigned short* v;
  unsigned char *a, *g;
  unsigned short* t;
  explicit Lds(int cells)
      : v(hc_alloc<unsigned short>(sizeof(unsigned short) * cells, 0xCD)), a(hc_alloc<unsigned char>(cells, 0xCD)),
        g(hc_alloc<unsigned char>(cells, 0xCD)), t(hc_alloc<unsigned short>(sizeof(unsigned short) * FG_TAB, 0xCD)) {}
  ~Lds() { free(v), free(a), free(g), free(t); }
};

// fillg_launch<FMT>
template <int FMT>
static void launches(WgHost wg, int B, int h, int w, int top, int scale, const void* in, const unsigned char* guide, long row_bytes,
                     long image_bytes, const unsigned short* tab, void* out) {
  const FgPlan p = fg_plan(h, w);
  if (p.single) {
    for (long b = 0; b < B; ++b) {
      Lds l(FL_PYR_CELLS);
      wg_fillg_plane<FMT>(wg, b, in, (long)h * w, out, (long)h * w, h, w, top, guide, row_bytes, image_bytes, scale, nullptr, nullptr,
                          0, tab, l.v, l.a, l.g, l.t);
    }
    return;
  }
  unsigned char* ws = hc_alloc<unsigned char>((size_t)B * p.stride, 0xEE);
  for (long b = 0; b < B; ++b)
    for (int ty = 0; ty < p.gy; ++ty)
      for (int tx = 0; tx < p.gx; ++tx) {
        Lds l(FL_PYR_CELLS);
        wg_fillg_pull<FMT>(wg, tx, ty, b, in, h, w, top, guide, row_bytes, image_bytes, scale, ws, p.stride, l.v, l.a, l.g);
      }
  for (long b = 0; b < B; ++b) {
    Lds l(FL_PYR_CELLS);
    wg_fillg_plane<FL_U16>(wg, b, ws + p.v6, p.stride / 2, ws + p.v6, p.stride / 2, p.h6, p.w6, 65535, nullptr, 0, 0, scale,
                           ws + p.a6, ws + p.g6, p.stride, tab, l.v, l.a, l.g, l.t);
  }
  for (long b = 0; b < B; ++b)
    for (int ty = 0; ty < p.gy; ++ty)
      for (int tx = 0; tx < p.gx; ++tx) {
        Lds l(FL_HALO_CELLS);
        wg_fillg_push<FMT>(wg, tx, ty, b, in, out, h, w, top, tab, ws, p.stride, l.v, l.a, l.g, l.t);
      }
  free(ws);
}

template <int FMT>
static int run(int B, int h, int w, int top, int scale, int skew, int pad, char** path) {
  const size_t bytes = (size_t)B * h * w * fl_elem_bytes(FMT);
  const long dense = (long)w * scale, rows = (long)h * scale;
  const long row_bytes = dense + pad, image_bytes = rows * row_bytes;
  void* in = hc_read(path[0], bytes);
  unsigned char* gfile = hc_read<unsigned char>(path[1], (size_t)(B * rows * dense));
  const size_t gbytes = (size_t)(skew + (B - 1) * image_bytes + (rows - 1) * row_bytes + dense);   // ends with the last byte used
  unsigned char* gbuf = hc_alloc<unsigned char>(gbytes, 0x5A);
  for (long r = 0; r < B * rows; ++r) memcpy(gbuf + skew + (r / rows) * image_bytes + (r % rows) * row_bytes, gfile + r * dense, dense);
  free(gfile);
  unsigned short* tab = hc_read<unsigned short>(path[2], FG_TAB * sizeof(unsigned short));
  void* out[2];
  for (int rev = 0; rev < 2; ++rev) {
    out[rev] = hc_alloc(bytes, 0xEE);
    launches<FMT>(WgHost{FL_THREADS, rev != 0}, B, h, w, top, scale, in, gbuf + skew, row_bytes, image_bytes, tab, out[rev]);
  }
  hc_same(out[0], out[1], bytes, "the output depends on the order of the threads within a phase");
  hc_write(path[3], out[0], bytes);
  free(in);
  free(gbuf);
  free(tab);
  free(out[0]);
  free(out[1]);
  return 0;
}

int main(int argc, char** argv) {
  hc_name = "guided_fill_host_check";
  if (argc != 13) hc_die("usage: guided_fill_host_check <fmt 0|1> B h w top scale skew pad in.bin guide.bin tab.bin out.bin");
  const int fmt = atoi(argv[1]), B = atoi(argv[2]), h = atoi(argv[3]), w = atoi(argv[4]), top = atoi(argv[5]);
  const int scale = atoi(argv[6]), skew = atoi(argv[7]), pad = atoi(argv[8]);
  if (B < 1 || h < 1 || h > FL_MAX_SIDE || w < 1 || w > FL_MAX_SIDE || top < 1 || top > 65535) return 2;
  if ((scale != 4 && scale != 8 && scale != 16) || skew < 0 || skew > 15 || pad < 0 || pad > 64) return 2;
  if (fmt == FL_U8) return run<FL_U8>(B, h, w, top, scale, skew, pad, argv + 9);
  if (fmt == FL_U16) return run<FL_U16>(B, h, w, top, scale, skew, pad, argv + 9);
  return 2;
}
