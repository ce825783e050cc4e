// Host-side check of the guidance-aware hole filler's tile, level and halo arithmetic: the per-thread phase bodies
// of csrc/fill_guided_tile.h (and those of csrc/fill_tile.h it builds on) -- the very text the device kernels of
// csrc/fill_guided.hip call -- compiled for the host and driven launch by launch, workgroup by workgroup, thread by thread,
// phase by phase over exactly-sized heap buffers (the LDS arrays too), so that the address and undefined-behaviour sanitizers see
// every access.  The launch plan below is fillg_launch's.  No GPU, no HIP, nothing loaded into Python.
// tools/guided_fill_host_check.py builds this with
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
// runs it over the GPU tests' shapes, patterns and formats and compares what it writes with tests/guided_fill_ref.py, bit for bit.
//
//   guided_fill_host_check <fmt 0|1> B h w top scale skew pad in.bin guide.bin tab.bin out.bin
//     in.bin: (B, h, w) codes; guide.bin: (B, h * scale, w * scale) u8; tab.bin: 256 u16  ->  out.bin: (B, h, w) codes
//     The guidance is laid out with rows w * scale + pad bytes apart, starting skew bytes into a buffer that ends with the last
//     row's last byte: skew and pad choose the load path (16-byte segments with or without a partial last segment read as
//     4-byte words, 4-byte words throughout, bytes), and a read past a row's end in the last row is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../codon_amd/csrc/fill_guided_tile.h"

using namespace codon;

static void* slurp(const char* path, size_t bytes, size_t skew = 0) {
  char* p = (char*)malloc(bytes + skew);        // exactly `bytes` past the skew: one element past the end is a sanitizer report
  FILE* f = fopen(path, "rb");
  if (!p || !f || fread(p + skew, 1, bytes, f) != bytes || fgetc(f) != EOF) {
    fprintf(stderr, "guided_fill_host_check: %s does not hold exactly %zu bytes\n", path, bytes);
    exit(2);
  }
  fclose(f);
  return p;
}

template <typename T>
static T* lds(int cells) {
  T* p = (T*)malloc(cells * sizeof(T));
  memset(p, 0xCD, cells * sizeof(T));           // what a phase reads without an earlier phase having written it shows as this
  return p;
}

template <int S>
static void g0_all(const unsigned char* gimg, long row_bytes, int h, int w, int y0, int x0, unsigned char* g, unsigned char* a,
                   unsigned char* ws_g0) {
  for (int t = 0; t < FL_THREADS; ++t) fg_g0_tile<S>(t, gimg, row_bytes, h, w, y0, x0, g, a, ws_g0);
}

static void g0_tile(int scale, const unsigned char* gimg, long row_bytes, int h, int w, int y0, int x0, unsigned char* g,
                    unsigned char* a, unsigned char* ws_g0) {
  if (scale == 4) g0_all<4>(gimg, row_bytes, h, w, y0, x0, g, a, ws_g0);
  else if (scale == 8) g0_all<8>(gimg, row_bytes, h, w, y0, x0, g, a, ws_g0);
  else g0_all<16>(gimg, row_bytes, h, w, y0, x0, g, a, ws_g0);
}

// fillg_plane_kernel<FMT>, workgroup b
template <int FMT>
static void plane_block(long b, const void* in, long in_stride, void* out, long out_stride, int h, int w, int top,
                        const unsigned char* guide, long row_bytes, long image_bytes, int scale, const unsigned char* a0,
                        const unsigned char* g0, long ag_stride, const unsigned short* tab) {
  unsigned short* v = lds<unsigned short>(FL_PYR_CELLS);
  unsigned char* a = lds<unsigned char>(FL_PYR_CELLS);
  unsigned char* g = lds<unsigned char>(FL_PYR_CELLS);
  unsigned short* tt = lds<unsigned short>(FG_TAB);
  const int K = fl_top_level(h, w);
  for (int t = 0; t < FL_THREADS; ++t) {
    fg_tab_load(t, tab, tt);
    fl_tile_load<FMT>(t, (const char*)in + b * in_stride * fl_elem_bytes(FMT), h, w, 0, 0, top, v);
  }
  if (guide) g0_tile(scale, guide + b * image_bytes, row_bytes, h, w, 0, 0, g, a, nullptr);
  else
    for (int t = 0; t < FL_THREADS; ++t) fg_plane_load8(t, a0 + b * ag_stride, g0 + b * ag_stride, h, w, a, g);
  for (int k = 0; k < K; ++k)
    for (int t = 0; t < FL_THREADS; ++t) fg_pull(t, k, v, a, g, h, w, 0, 0, nullptr, nullptr, nullptr);
  for (int k = K - 1; k >= 0; --k)
    for (int t = 0; t < FL_THREADS; ++t) fg_push(t, k, h, w, v, a, g, tt);
  for (int t = 0; t < FL_THREADS; ++t) fl_tile_store<FMT>(t, (char*)out + b * out_stride * fl_elem_bytes(FMT), h, w, nullptr, v);
  free(v);
  free(a);
  free(g);
  free(tt);
}

template <int FMT>
static int run(int B, int h, int w, int top, int scale, int skew, int pad, const char* fin, const char* fguide, const char* ftab,
               const char* fout) {
  const size_t n = (size_t)B * h * w, eb = (size_t)fl_elem_bytes(FMT);
  const long dense = (long)w * scale, rows = (long)h * scale;
  const long row_bytes = dense + pad, image_bytes = rows * row_bytes;
  void* in = slurp(fin, n * eb);
  unsigned char* gfile = (unsigned char*)slurp(fguide, (size_t)(B * rows * dense));
  const size_t gbytes = (size_t)(skew + (B - 1) * image_bytes + (rows - 1) * row_bytes + dense);   // ends with the last byte used
  unsigned char* gbuf = (unsigned char*)malloc(gbytes);
  memset(gbuf, 0x5A, gbytes);
  for (long r = 0; r < B * rows; ++r) memcpy(gbuf + skew + (r / rows) * image_bytes + (r % rows) * row_bytes, gfile + r * dense, dense);
  free(gfile);
  const unsigned char* guide = gbuf + skew;
  unsigned short* tab = (unsigned short*)slurp(ftab, FG_TAB * sizeof(unsigned short));
  void* out = malloc(n * eb);
  memset(out, 0xEE, n * eb);                    // an element no thread writes stays this
  if (h <= FL_TILE && w <= FL_TILE) {
    for (long b = 0; b < B; ++b)
      plane_block<FMT>(b, in, (long)h * w, out, (long)h * w, h, w, top, guide, row_bytes, image_bytes, scale, nullptr, nullptr, 0,
                       tab);
  } else {
    const long cells = fl_workspace_cells(h, w), ws_stride = (fg_workspace_bytes(h, w) + 15) / 16 * 16;
    unsigned char* ws = (unsigned char*)malloc((size_t)B * ws_stride);             // codon_fill_guided_workspace_bytes, exactly
    memset(ws, 0xEE, (size_t)B * ws_stride);
    const int gy = (h + FL_TILE - 1) / FL_TILE, gx = (w + FL_TILE - 1) / FL_TILE;
    for (long b = 0; b < B; ++b)                // fillg_pull_kernel<FMT>
      for (int ty = 0; ty < gy; ++ty)
        for (int tx = 0; tx < gx; ++tx) {
          unsigned short* v = lds<unsigned short>(FL_PYR_CELLS);
          unsigned char* a = lds<unsigned char>(FL_PYR_CELLS);
          unsigned char* g = lds<unsigned char>(FL_PYR_CELLS);
          unsigned char* img = ws + b * ws_stride;
          for (int t = 0; t < FL_THREADS; ++t)
            fl_tile_load<FMT>(t, (const char*)in + b * h * w * (long)eb, h, w, ty * FL_TILE, tx * FL_TILE, top, v);
          g0_tile(scale, guide + b * image_bytes, row_bytes, h, w, ty * FL_TILE, tx * FL_TILE, g, a, img + 4 * cells);
          long at = 0;
          for (int k = 0; k < FL_LOG; ++k) {
            for (int t = 0; t < FL_THREADS; ++t)
              fg_pull(t, k, v, a, g, h, w, ty, tx, (unsigned short*)img + at, img + 2 * cells + at, img + 3 * cells + at);
            at += (long)fl_size(h, k + 1) * fl_size(w, k + 1);
          }
          free(v);
          free(a);
          free(g);
        }
    const long l6 = fl_level_offset(h, w, FL_LOG);                                 // fillg_plane_kernel<FL_U16>, V in place
    unsigned short* v6 = (unsigned short*)ws + l6;
    for (long b = 0; b < B; ++b)
      plane_block<FL_U16>(b, v6, ws_stride / 2, v6, ws_stride / 2, fl_size(h, FL_LOG), fl_size(w, FL_LOG), 65535, nullptr, 0, 0,
                          scale, ws + 2 * cells + l6, ws + 3 * cells + l6, ws_stride, tab);
    for (long b = 0; b < B; ++b)                // fillg_push_kernel<FMT>
      for (int ty = 0; ty < gy; ++ty)
        for (int tx = 0; tx < gx; ++tx) {
          unsigned short* hv = lds<unsigned short>(FL_HALO_CELLS);
          unsigned char* ha = lds<unsigned char>(FL_HALO_CELLS);
          unsigned char* hg = lds<unsigned char>(FL_HALO_CELLS);
          unsigned short* tt = lds<unsigned short>(FG_TAB);
          const long at = b * h * w * (long)eb;
          const unsigned char* img = ws + b * ws_stride;
          int(*v0)[FL_PER_THREAD] = (int(*)[FL_PER_THREAD])malloc(sizeof(int) * FL_PER_THREAD * FL_THREADS);   // the threads' registers
          int(*g0)[FL_PER_THREAD] = (int(*)[FL_PER_THREAD])malloc(sizeof(int) * FL_PER_THREAD * FL_THREADS);
          for (int t = 0; t < FL_THREADS; ++t) {
            fg_tab_load(t, tab, tt);
            fl_halo_load(t, h, w, ty, tx, (const unsigned short*)img, hv);
            fg_halo_load8(t, h, w, ty, tx, img + 2 * cells, ha);
            fg_halo_load8(t, h, w, ty, tx, img + 3 * cells, hg);
            fl_halo_in<FMT>(t, h, w, ty, tx, (const char*)in + at, top, v0[t]);
            fg_halo_g0(t, h, w, ty, tx, img + 4 * cells, g0[t]);
          }
          for (int k = FL_LOG - 1; k >= 1; --k)
            for (int t = 0; t < FL_THREADS; ++t) fg_halo_push(t, k, h, w, ty, tx, hv, ha, hg, tt);
          for (int t = 0; t < FL_THREADS; ++t) fg_halo_out<FMT>(t, h, w, ty, tx, v0[t], g0[t], hv, ha, tt, (char*)out + at);
          free(v0);
          free(g0);
          free(hv);
          free(ha);
          free(hg);
          free(tt);
        }
    free(ws);
  }
  FILE* f = fopen(fout, "wb");
  if (!f || fwrite(out, 1, n * eb, f) != n * eb || fclose(f) != 0) {
    fprintf(stderr, "guided_fill_host_check: cannot write %s\n", fout);
    return 2;
  }
  free(in);
  free(gbuf);
  free(tab);
  free(out);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 13) {
    fprintf(stderr, "usage: guided_fill_host_check <fmt 0|1> B h w top scale skew pad in.bin guide.bin tab.bin out.bin\n");
    return 2;
  }
  const int fmt = atoi(argv[1]), B = atoi(argv[2]), h = atoi(argv[3]), w = atoi(argv[4]), top = atoi(argv[5]);
  const int scale = atoi(argv[6]), skew = atoi(argv[7]), pad = atoi(argv[8]);
  if (B < 1 || h < 1 || h > FL_MAX_SIDE || w < 1 || w > FL_MAX_SIDE || top < 1 || top > 65535) return 2;
  if ((scale != 4 && scale != 8 && scale != 16) || skew < 0 || skew > 15 || pad < 0 || pad > 64) return 2;
  if (fmt == FL_U8) return run<FL_U8>(B, h, w, top, scale, skew, pad, argv[9], argv[10], argv[11], argv[12]);
  if (fmt == FL_U16) return run<FL_U16>(B, h, w, top, scale, skew, pad, argv[9], argv[10], argv[11], argv[12]);
  return 2;
}
