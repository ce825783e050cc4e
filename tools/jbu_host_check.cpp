// Host-side check of the joint bilateral upsampler: the launch plan and the workgroup bodies of
// csrc/jbu_tile.h -- the very text the device kernels of csrc/jbu.hip call -- compiled for the host and run workgroup by
// workgroup of both launches over exactly-sized heap buffers (the LDS arrays too), so that the address and undefined-behaviour
// sanitizers see every access.  Every case runs with the threads of a workgroup forwards and backwards, and the two outputs must
// agree.  No GPU, no HIP, nothing loaded into Python.  `python tools/host_check.py jbu` builds this, runs it over the GPU tests'
// shapes, patterns and formats and compares what it writes with tests/jbu_ref.py, bit for bit.
//
//   jbu_host_check <fmt 0|1> B h w scale skew pad in.bin guide.bin rtab.bin stab.bin out.bin
//     in.bin: (B, h, w) codes; guide.bin: (B, h * scale, w * scale) u8; rtab.bin: 256 u16; stab.bin: scale x 4 u16
//     ->  out.bin: (B, h * scale, w * scale) codes
//     The guidance is laid out as guided_fill_host_check lays it out: rows w * scale + pad bytes apart, starting skew bytes into
//     a buffer that ends with the last row's last byte, so that skew and pad choose the load path (16 bytes at once or bytes) and
//     a read past a row's end in the last row is a sanitizer report.
#include "host_check.h"

#include "../codon_amd/csrc/jbu_tile.h"

using namespace codon;

// jbu_launch<S, FMT>
template <int S, int FMT>
static void launches(WgHost wg, int B, int h, int w, const void* in, const unsigned char* guide, long row_bytes, long image_bytes,
                     const unsigned short* rtab, const unsigned short* stab, void* out) {
  const JbPlan p = jb_plan(h, w, S);
  unsigned char* ws = hc_alloc<unsigned char>((size_t)B * p.stride, 0xEE);
  for (long b = 0; b < B; ++b)
    for (int ty = 0; ty < p.g0y; ++ty)
      for (int tx = 0; tx < p.g0x; ++tx) {
        unsigned char* g = hc_alloc<unsigned char>(FL_TILE * FL_TILE, 0xCD);
        wg_jbu_g0(wg, tx, ty, b, guide, row_bytes, image_bytes, S, h, w, ws, p.stride, g);
        free(g);
      }
  for (long b = 0; b < B; ++b)
    for (int ty = 0; ty < p.gy; ++ty)
      for (int tx = 0; tx < p.gx; ++tx) {
        unsigned short* lc = hc_alloc<unsigned short>(sizeof(unsigned short) * JbShape<S>::CELLS, 0xCD);
        unsigned char* lg = hc_alloc<unsigned char>(JbShape<S>::CELLS, 0xCD);
        unsigned short* t = hc_alloc<unsigned short>(sizeof(unsigned short) * FG_TAB, 0xCD);
        unsigned short* st = hc_alloc<unsigned short>(sizeof(unsigned short) * S * 4, 0xCD);
        wg_jbu<S, FMT>(wg, tx, ty, b, in, h, w, guide, row_bytes, image_bytes, rtab, stab, ws, p.stride, out, lc, lg, t, st);
        free(lc), free(lg), free(t), free(st);
      }
  free(ws);
}

template <int S, int FMT>
static int run(int B, int h, int w, int skew, int pad, char** path) {
  const size_t in_bytes = (size_t)B * h * w * fl_elem_bytes(FMT), out_bytes = in_bytes * S * S;
  const long dense = (long)w * S, rows = (long)h * S;
  const long row_bytes = dense + pad, image_bytes = rows * row_bytes;
  void* in = hc_read(path[0], in_bytes);
  unsigned char* gfile = hc_read<unsigned char>(path[1], (size_t)(B * rows * dense));
  const size_t gbytes = (size_t)(skew + (B - 1) * image_bytes + (rows - 1) * row_bytes + dense);   // ends with the last byte used
  unsigned char* gbuf = (unsigned char*)memset(hc_aligned(gbytes), 0x5A, gbytes);
  for (long r = 0; r < B * rows; ++r) memcpy(gbuf + skew + (r / rows) * image_bytes + (r % rows) * row_bytes, gfile + r * dense, dense);
  free(gfile);
  unsigned short* rtab = hc_read<unsigned short>(path[2], FG_TAB * sizeof(unsigned short));
  unsigned short* stab = hc_read<unsigned short>(path[3], S * 4 * sizeof(unsigned short));
  void* out[2];
  for (int rev = 0; rev < 2; ++rev) {
    out[rev] = memset(hc_aligned(out_bytes), 0xEE, out_bytes);
    launches<S, FMT>(WgHost{JB_THREADS, rev != 0}, B, h, w, in, gbuf + skew, row_bytes, image_bytes, rtab, stab, out[rev]);
  }
  hc_same(out[0], out[1], out_bytes, "the output depends on the order of the threads within a phase");
  hc_write(path[4], out[0], out_bytes);
  free(in);
  free(gbuf);
  free(rtab);
  free(stab);
  free(out[0]);
  free(out[1]);
  return 0;
}

template <int FMT>
static int by_scale(int scale, int B, int h, int w, int skew, int pad, char** path) {
  if (scale == 4) return run<4, FMT>(B, h, w, skew, pad, path);
  if (scale == 8) return run<8, FMT>(B, h, w, skew, pad, path);
  return run<16, FMT>(B, h, w, skew, pad, path);
}

int main(int argc, char** argv) {
  hc_name = "jbu_host_check";
  if (argc != 13) hc_die("usage: jbu_host_check <fmt 0|1> B h w scale skew pad in.bin guide.bin rtab.bin stab.bin out.bin");
  const int fmt = atoi(argv[1]), B = atoi(argv[2]), h = atoi(argv[3]), w = atoi(argv[4]), scale = atoi(argv[5]);
  const int skew = atoi(argv[6]), pad = atoi(argv[7]);
  if (B < 1 || h < 1 || h > FL_MAX_SIDE || w < 1 || w > FL_MAX_SIDE) return 2;
  if ((scale != 4 && scale != 8 && scale != 16) || skew < 0 || skew > 15 || pad < 0 || pad > 64) return 2;
  if (fmt == FL_U8) return by_scale<FL_U8>(scale, B, h, w, skew, pad, argv + 8);
  if (fmt == FL_U16) return by_scale<FL_U16>(scale, B, h, w, skew, pad, argv + 8);
  return 2;
}
