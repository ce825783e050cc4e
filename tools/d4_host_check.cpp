// Host-side check of the D4 self-ensemble kernels: the workgroup bodies of csrc/d4_tile.h -- the very text
// the device kernels of csrc/d4.hip call -- compiled for the host and run workgroup by workgroup over exactly-sized heap buffers
// (the LDS arrays too), so that the address and undefined-behaviour sanitizers see every access.  Every run is made with the
// threads of a workgroup forwards and backwards, and the two outputs must agree.  No GPU, no HIP, nothing loaded into Python.
// `python tools/host_check.py d4` builds this (with -ffp-contract=off), runs it over the GPU tests' shapes and compares what it
// writes with tests/d4_ref.py, bit for bit.
//
//   d4_host_check views <elem bytes 2|4> B H W src0.bin <src1.bin|-> out_prefix   -> out_prefix.{up0,tp0[,up1,tp1]}
//   d4_host_check merge <dtype 0|1|2>    B H W upright.bin transposed.bin out.bin
#include "host_check.h"

#include "../codon_amd/csrc/d4_tile.h"

using namespace codon;

static const char* kOrder = "the output depends on the order of the threads within a phase";

template <typename T>
static int views(int B, int H, int W, const char* f0, const char* f1, const std::string& prefix) {
  const size_t bytes = (size_t)B * H * W * sizeof(T);
  T* s0 = hc_read<T>(f0, bytes);
  T* s1 = strcmp(f1, "-") ? hc_read<T>(f1, bytes) : nullptr;
  const int planes = s1 ? 2 : 1;
  T* out[2][4] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};
  for (int rev = 0; rev < 2; ++rev) {
    const WgHost wg{D4_THREADS, rev != 0};
    T** o = out[rev];
    for (int k = 0; k < 2 * planes; ++k) o[k] = hc_alloc<T>(4 * bytes, 0xEE);
    for (int bz = 0; bz < B * planes; ++bz)       // the launch of d4_views_kernel<T>
      for (int by = 0; by < d4_tiles(H); ++by)
        for (int bx = 0; bx < d4_tiles(W); ++bx) {
          typedef T Row[D4Stride<T>::value];
          Row* tile = hc_alloc<Row>(sizeof(Row) * D4_TILE, 0xCD);
          wg_d4_views<T>(wg, bx, by, bz, s0, s1, o[0], o[1], o[2], o[3], H, W, planes, tile);
          free(tile);
        }
  }
  const char* names[4] = {".up0", ".tp0", ".up1", ".tp1"};
  for (int k = 0; k < 2 * planes; ++k) {
    hc_same(out[0][k], out[1][k], 4 * bytes, kOrder);
    hc_write(prefix + names[k], out[0][k], 4 * bytes);
    free(out[0][k]);
    free(out[1][k]);
  }
  free(s0);
  free(s1);
  return 0;
}

template <int DT>
static int merge(int B, int H, int W, const char* fu, const char* ft, const char* fo) {
  const size_t n = (size_t)B * H * W, e = DT == 0 ? 4 : 2;
  void* up = hc_read(fu, 4 * n * e);
  void* tr = hc_read(ft, 4 * n * e);
  float* out[2];
  for (int rev = 0; rev < 2; ++rev) {
    const WgHost wg{D4_THREADS, rev != 0};
    out[rev] = hc_alloc<float>(n * sizeof(float), 0xEE);
    for (int bz = 0; bz < B; ++bz)                // the launch of d4_merge_kernel<DT>
      for (int by = 0; by < d4_tiles(H); ++by)
        for (int bx = 0; bx < d4_tiles(W); ++bx) {
          typedef float Plane[D4_TILE][D4_TILE + 1];
          Plane* lds = hc_alloc<Plane>(sizeof(Plane) * 4, 0xCD);
          wg_d4_merge<DT>(wg, bx, by, bz, up, tr, out[rev], H, W, lds);
          free(lds);
        }
  }
  hc_same(out[0], out[1], n * sizeof(float), kOrder);
  hc_write(fo, out[0], n * sizeof(float));
  free(up);
  free(tr);
  free(out[0]);
  free(out[1]);
  return 0;
}

int main(int argc, char** argv) {
  hc_name = "d4_host_check";
  if (argc != 9 || (strcmp(argv[1], "views") && strcmp(argv[1], "merge")))
    hc_die("usage: d4_host_check views <2|4> B H W src0 <src1|-> out_prefix\n"
           "       d4_host_check merge <0|1|2> B H W upright transposed out");
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
