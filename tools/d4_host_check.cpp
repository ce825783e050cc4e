// Host-side check of the D4 self-ensemble kernels' index arithmetic: the per-thread bodies of csrc/d4_tile.h --
// the very text the device kernels of csrc/d4.hip call -- compiled for the host and driven block by block, thread by thread,
// phase by phase over exactly-sized heap buffers, so that the address and undefined-behaviour sanitizers see every access.
// No GPU, no HIP, nothing loaded into Python.  tools/d4_host_check.py builds this with
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
// runs it over the GPU tests' shapes and compares what it writes with tests/d4_ref.py, bit for bit.
//
//   d4_host_check views <elem bytes 2|4> B H W src0.bin <src1.bin|-> out_prefix   -> out_prefix.{up0,tp0[,up1,tp1]}
//   d4_host_check merge <dtype 0|1|2>    B H W upright.bin transposed.bin out.bin
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../codon_amd/csrc/d4_tile.h"

using namespace codon;

static void* slurp(const char* path, size_t bytes) {
  void* p = malloc(bytes);                      // exactly `bytes`: one element past either end is a sanitizer report
  FILE* f = fopen(path, "rb");
  if (!p || !f || fread(p, 1, bytes, f) != bytes || fgetc(f) != EOF) {
    fprintf(stderr, "d4_host_check: %s does not hold exactly %zu bytes\n", path, bytes);
    exit(2);
  }
  fclose(f);
  return p;
}

static void dump(const std::string& path, const void* p, size_t bytes) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, 1, bytes, f) != bytes || fclose(f) != 0) {
    fprintf(stderr, "d4_host_check: cannot write %s\n", path.c_str());
    exit(2);
  }
}

// the launch of d4_views_kernel<T>: grid (ceil(W/32), ceil(H/32), B * planes)
template <typename T>
static void run_views(int B, int H, int W, const T* src0, const T* src1, T* up0, T* tp0, T* up1, T* tp1) {
  const int planes = src1 ? 2 : 1;
  const long hw = (long)H * W;
  for (int z = 0; z < B * planes; ++z)
    for (int by = 0; by < (H + D4_TILE - 1) / D4_TILE; ++by)
      for (int bx = 0; bx < (W + D4_TILE - 1) / D4_TILE; ++bx) {
        T tile[D4_TILE][D4Stride<T>::value];
        memset(tile, 0xCD, sizeof(tile));       // what the barrier does not order would show as this pattern
        const int b = z / planes, p = z - b * planes;
        const T* src = (p ? src1 : src0) + b * hw;
        T* up = (p ? up1 : up0) + 4 * b * hw;
        T* tp = (p ? tp1 : tp0) + 4 * b * hw;
        for (int t = 0; t < D4_THREADS; ++t) d4_views_phase1<T>(t, by * D4_TILE, bx * D4_TILE, H, W, src, up, tile);
        for (int t = 0; t < D4_THREADS; ++t) d4_views_phase2<T>(t, by * D4_TILE, bx * D4_TILE, H, W, tp, tile);
      }
}

template <typename T>
static int views(int B, int H, int W, const char* f0, const char* f1, const std::string& prefix) {
  const size_t n = (size_t)B * H * W;
  T* s0 = (T*)slurp(f0, n * sizeof(T));
  T* s1 = strcmp(f1, "-") ? (T*)slurp(f1, n * sizeof(T)) : nullptr;
  T* out[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int k = 0; k < (s1 ? 4 : 2); ++k) {
    out[k] = (T*)malloc(4 * n * sizeof(T));
    memset(out[k], 0xEE, 4 * n * sizeof(T));    // an element no thread writes stays this
  }
  run_views<T>(B, H, W, s0, s1, out[0], out[1], out[2], out[3]);
  const char* names[4] = {".up0", ".tp0", ".up1", ".tp1"};
  for (int k = 0; k < (s1 ? 4 : 2); ++k) {
    dump(prefix + names[k], out[k], 4 * n * sizeof(T));
    free(out[k]);
  }
  free(s0);
  free(s1);
  return 0;
}

// the launch of d4_merge_kernel<DT>: grid (ceil(W/32), ceil(H/32), B)
template <int DT>
static int merge(int B, int H, int W, const char* fu, const char* ft, const char* fo) {
  const size_t n = (size_t)B * H * W, e = DT == 0 ? 4 : 2;
  void* up = slurp(fu, 4 * n * e);
  void* tr = slurp(ft, 4 * n * e);
  float* out = (float*)malloc(n * sizeof(float));
  memset(out, 0xEE, n * sizeof(float));
  const long hw = (long)H * W;
  for (int z = 0; z < B; ++z)
    for (int by = 0; by < (H + D4_TILE - 1) / D4_TILE; ++by)
      for (int bx = 0; bx < (W + D4_TILE - 1) / D4_TILE; ++bx) {
        float lds[4][D4_TILE][D4_TILE + 1];
        memset(lds, 0xCD, sizeof(lds));
        for (int t = 0; t < D4_THREADS; ++t) d4_merge_phase1<DT>(t, by * D4_TILE, bx * D4_TILE, H, W, tr, 4 * z * hw, lds);
        for (int t = 0; t < D4_THREADS; ++t)
          d4_merge_phase2<DT>(t, by * D4_TILE, bx * D4_TILE, H, W, up, 4 * z * hw, lds, out + z * hw);
      }
  dump(fo, out, n * sizeof(float));
  free(up);
  free(tr);
  free(out);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 9 || (strcmp(argv[1], "views") && strcmp(argv[1], "merge"))) {
    fprintf(stderr, "usage: d4_host_check views <2|4> B H W src0 <src1|-> out_prefix\n"
                    "       d4_host_check merge <0|1|2> B H W upright transposed out\n");
    return 2;
  }
  const int k = atoi(argv[2]), B = atoi(argv[3]), H = atoi(argv[4]), W = atoi(argv[5]);
  if (B <= 0 || H <= 0 || W <= 0) return 2;
  if (!strcmp(argv[1], "views")) {
    if (k == 4) return views<unsigned int>(B, H, W, argv[6], argv[7], argv[8]);
    if (k == 2) return views<unsigned short>(B, H, W, argv[6], argv[7], argv[8]);
    return 2;
  }
  if (k == 0) return merge<0>(B, H, W, argv[6], argv[7], argv[8]);
  if (k == 1) return merge<1>(B, H, W, argv[6], argv[7], argv[8]);
  if (k == 2) return merge<2>(B, H, W, argv[6], argv[7], argv[8]);
  return 2;
}
