// Host-side check of the pull-push hole filler's tile, level and halo arithmetic: the per-thread phase bodies of
// csrc/fill_tile.h -- the very text the device kernels of csrc/fill_holes.hip call -- compiled for the host and driven launch by
// launch, workgroup by workgroup, thread by thread, phase by phase over exactly-sized heap buffers (the LDS arrays too), so that
// the address and undefined-behaviour sanitizers see every access.  The launch plan below is fill_launch's.  No GPU, no HIP,
// nothing loaded into Python.  tools/fill_host_check.py builds this with
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
// runs it over the GPU tests' shapes, patterns and formats and compares what it writes with tests/fill_ref.py, bit for bit.
//
//   fill_host_check <fmt 0|1|2> B h w top in.bin tab.bin|- out.bin
//     in.bin: (B, h, w) elements of the format; tab.bin: top + 1 fp32 (format 2 only)  ->  out.bin: (B, h, w) elements
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../codon_amd/csrc/fill_tile.h"

using namespace codon;

static void* slurp(const char* path, size_t bytes) {
  void* p = malloc(bytes);                      // exactly `bytes`: one element past either end is a sanitizer report
  FILE* f = fopen(path, "rb");
  if (!p || !f || fread(p, 1, bytes, f) != bytes || fgetc(f) != EOF) {
    fprintf(stderr, "fill_host_check: %s does not hold exactly %zu bytes\n", path, bytes);
    exit(2);
  }
  fclose(f);
  return p;
}

static unsigned short* lds(int cells) {
  unsigned short* p = (unsigned short*)malloc(cells * sizeof(unsigned short));
  memset(p, 0xCD, cells * sizeof(unsigned short));   // what a phase reads without an earlier phase having written it shows as this
  return p;
}

// fill_plane_kernel<FMT>, workgroup b
template <int FMT>
static void plane_block(long b, const void* in, long in_stride, void* out, long out_stride, int h, int w, const float* tab,
                        int top) {
  unsigned short* pyr = lds(FL_PYR_CELLS);
  const int K = fl_top_level(h, w);
  for (int t = 0; t < FL_THREADS; ++t)
    fl_tile_load<FMT>(t, (const char*)in + b * in_stride * fl_elem_bytes(FMT), h, w, 0, 0, top, pyr);
  for (int k = 0; k < K; ++k)
    for (int t = 0; t < FL_THREADS; ++t) fl_tile_pull(t, k, pyr, nullptr, h, w, 0, 0);
  for (int k = K - 1; k >= 0; --k)
    for (int t = 0; t < FL_THREADS; ++t) fl_tile_push(t, k, h, w, pyr);
  for (int t = 0; t < FL_THREADS; ++t) fl_tile_store<FMT>(t, (char*)out + b * out_stride * fl_elem_bytes(FMT), h, w, tab, pyr);
  free(pyr);
}

template <int FMT>
static int run(int B, int h, int w, int top, const char* fin, const char* ftab, const char* fout) {
  const size_t n = (size_t)B * h * w, eb = (size_t)fl_elem_bytes(FMT);
  void* in = slurp(fin, n * eb);
  float* tab = FMT == FL_F32 ? (float*)slurp(ftab, ((size_t)top + 1) * sizeof(float)) : nullptr;
  void* out = malloc(n * eb);
  memset(out, 0xEE, n * eb);                    // an element no thread writes stays this
  if (h <= FL_TILE && w <= FL_TILE) {
    for (long b = 0; b < B; ++b) plane_block<FMT>(b, in, (long)h * w, out, (long)h * w, h, w, tab, top);
  } else {
    const long cells = fl_workspace_cells(h, w), ws_stride = (2 * cells + 15) / 16 * 8;
    unsigned short* ws = (unsigned short*)malloc((size_t)B * ws_stride * 2);       // codon_fill_holes_workspace_bytes, exactly
    memset(ws, 0xEE, (size_t)B * ws_stride * 2);
    const int gy = (h + FL_TILE - 1) / FL_TILE, gx = (w + FL_TILE - 1) / FL_TILE;
    for (long b = 0; b < B; ++b)                // fill_pull_kernel<FMT>
      for (int ty = 0; ty < gy; ++ty)
        for (int tx = 0; tx < gx; ++tx) {
          unsigned short* pyr = lds(FL_PYR_CELLS);
          for (int t = 0; t < FL_THREADS; ++t)
            fl_tile_load<FMT>(t, (const char*)in + b * h * w * (long)eb, h, w, ty * FL_TILE, tx * FL_TILE, top, pyr);
          unsigned short* lvl = ws + b * ws_stride;
          for (int k = 0; k < FL_LOG; ++k) {
            for (int t = 0; t < FL_THREADS; ++t) fl_tile_pull(t, k, pyr, lvl, h, w, ty, tx);
            lvl += (long)fl_size(h, k + 1) * fl_size(w, k + 1);
          }
          free(pyr);
        }
    unsigned short* l6 = ws + fl_level_offset(h, w, FL_LOG);                       // fill_plane_kernel<FL_U16>, in place
    for (long b = 0; b < B; ++b)
      plane_block<FL_U16>(b, l6, ws_stride, l6, ws_stride, fl_size(h, FL_LOG), fl_size(w, FL_LOG), nullptr, 65535);
    for (long b = 0; b < B; ++b)                // fill_push_kernel<FMT>
      for (int ty = 0; ty < gy; ++ty)
        for (int tx = 0; tx < gx; ++tx) {
          unsigned short* hp = lds(FL_HALO_CELLS);
          const long at = b * h * w * (long)eb;
          int(*v0)[FL_PER_THREAD] = (int(*)[FL_PER_THREAD])malloc(sizeof(int) * FL_PER_THREAD * FL_THREADS);   // the threads' registers
          for (int t = 0; t < FL_THREADS; ++t) {
            fl_halo_load(t, h, w, ty, tx, ws + b * ws_stride, hp);
            fl_halo_in<FMT>(t, h, w, ty, tx, (const char*)in + at, top, v0[t]);
          }
          for (int k = FL_LOG - 1; k >= 1; --k)
            for (int t = 0; t < FL_THREADS; ++t) fl_halo_push(t, k, h, w, ty, tx, hp);
          for (int t = 0; t < FL_THREADS; ++t) fl_halo_out<FMT>(t, h, w, ty, tx, v0[t], hp, (char*)out + at, tab);
          free(v0);
          free(hp);
        }
    free(ws);
  }
  FILE* f = fopen(fout, "wb");
  if (!f || fwrite(out, 1, n * eb, f) != n * eb || fclose(f) != 0) {
    fprintf(stderr, "fill_host_check: cannot write %s\n", fout);
    return 2;
  }
  free(in);
  free(tab);
  free(out);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 9) {
    fprintf(stderr, "usage: fill_host_check <fmt 0|1|2> B h w top in.bin tab.bin|- out.bin\n");
    return 2;
  }
  const int fmt = atoi(argv[1]), B = atoi(argv[2]), h = atoi(argv[3]), w = atoi(argv[4]), top = atoi(argv[5]);
  if (B < 1 || h < 1 || h > FL_MAX_SIDE || w < 1 || w > FL_MAX_SIDE || top < 1 || top > 65535) return 2;
  if (fmt == FL_U8) return run<FL_U8>(B, h, w, top, argv[6], argv[7], argv[8]);
  if (fmt == FL_U16) return run<FL_U16>(B, h, w, top, argv[6], argv[7], argv[8]);
  if (fmt == FL_F32) return run<FL_F32>(B, h, w, top, argv[6], argv[7], argv[8]);
  return 2;
}
