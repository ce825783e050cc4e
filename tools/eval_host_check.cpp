// Host-side check of the depth evaluation kernel's tile, halo and dilation arithmetic: the four per-thread phase
// bodies of csrc/eval_tile.h -- the very text the device kernel of csrc/eval.hip calls -- compiled for the host and driven block
// by block, thread by thread, phase by phase over exactly-sized heap buffers, so that the address and undefined-behaviour
// sanitizers see every access.  Only the wave / workgroup reduction is the device's own; here the threads' words are added up
// (word 3: the maximum) in plain C++.  No GPU, no HIP, nothing loaded into Python.  tools/eval_host_check.py builds this with
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
// runs it over the GPU tests' cases and compares what it writes with tests/eval_ref.py, bit for bit.
//
//   eval_host_check <bits 8|16> B H W Hl Wl <nthr> t0 t1 t2 t3 <edge 0|1> T r label.bin out.bin out_prefix
//     label.bin: (B, Hl, Wl) codes, out.bin: (B, H, W) codes  ->  out_prefix.{acc (B,16) u64, err (B,H,W) codes, reg (B,H,W) u8}
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../codon_amd/csrc/eval_tile.h"

using namespace codon;

static void* slurp(const char* path, size_t bytes) {
  void* p = malloc(bytes);                      // exactly `bytes`: one element past either end is a sanitizer report
  FILE* f = fopen(path, "rb");
  if (!p || !f || fread(p, 1, bytes, f) != bytes || fgetc(f) != EOF) {
    fprintf(stderr, "eval_host_check: %s does not hold exactly %zu bytes\n", path, bytes);
    exit(2);
  }
  fclose(f);
  return p;
}

static void dump(const std::string& path, const void* p, size_t bytes) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, 1, bytes, f) != bytes || fclose(f) != 0) {
    fprintf(stderr, "eval_host_check: cannot write %s\n", path.c_str());
    exit(2);
  }
}

// the launch of depth_errors_kernel<T>: grid (ceil(W/32), ceil(H/32), B)
template <typename T>
static int run(const EvalArgs& a, int B, int Hl, const char* fl, const char* fo, const std::string& prefix) {
  const size_t n = (size_t)B * a.H * a.W;
  T* label = (T*)slurp(fl, (size_t)B * Hl * a.label_row * sizeof(T));
  T* out = (T*)slurp(fo, n * sizeof(T));
  T* err = (T*)malloc(n * sizeof(T));
  unsigned char* reg = (unsigned char*)malloc(n);
  unsigned long long* acc = (unsigned long long*)calloc((size_t)B * EV_WORDS, sizeof(unsigned long long));   // the entry's memset
  memset(err, 0xEE, n * sizeof(T));             // an element no thread writes stays this
  memset(reg, 0xEE, n);
  const long hw = (long)a.H * a.W;
  for (int b = 0; b < B; ++b)
    for (int by = 0; by < (a.H + EV_TILE - 1) / EV_TILE; ++by)
      for (int bx = 0; bx < (a.W + EV_TILE - 1) / EV_TILE; ++bx) {
        T lab[EV_SIDE][EV_SIDE];
        unsigned char flag[EV_FSIDE][EV_FSIDE], rowor[EV_FSIDE][EV_TILE];
        memset(lab, 0xCD, sizeof(lab));         // what a phase reads without an earlier phase having written it shows as this
        memset(flag, 0xCD, sizeof(flag));
        memset(rowor, 0xCD, sizeof(rowor));
        const int i0 = by * EV_TILE, j0 = bx * EV_TILE;
        for (int t = 0; t < EV_THREADS; ++t) ev_load<T>(a, t, i0, j0, label + b * a.label_image, lab);
        if (a.edge) {
          for (int t = 0; t < EV_THREADS; ++t) ev_flags<T>(a, t, lab, flag);
          for (int t = 0; t < EV_THREADS; ++t) ev_row_or(a, t, flag, rowor);
        }
        for (int t = 0; t < EV_THREADS; ++t) {
          unsigned long long w[EV_WORDS] = {0};
          ev_pixels<T>(a, t, i0, j0, lab, rowor, out + b * hw, err + b * hw, reg + b * hw, w);
          for (int k = 0; k < EV_WORDS; ++k) {
            unsigned long long& d = acc[(size_t)b * EV_WORDS + k];
            d = k == 3 ? (w[k] > d ? w[k] : d) : d + w[k];
          }
        }
      }
  dump(prefix + ".acc", acc, (size_t)B * EV_WORDS * sizeof(unsigned long long));
  dump(prefix + ".err", err, n * sizeof(T));
  dump(prefix + ".reg", reg, n);
  free(label);
  free(out);
  free(err);
  free(reg);
  free(acc);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 18) {
    fprintf(stderr, "usage: eval_host_check <8|16> B H W Hl Wl nthr t0 t1 t2 t3 edge T r label.bin out.bin out_prefix\n");
    return 2;
  }
  int v[14];
  for (int k = 0; k < 14; ++k) v[k] = atoi(argv[1 + k]);
  const int bits = v[0], B = v[1], Hl = v[4], Wl = v[5];
  EvalArgs a;
  a.H = v[2];
  a.W = v[3];
  a.label_row = Wl;
  a.label_image = (long)Hl * Wl;
  a.nthr = v[6];
  for (int k = 0; k < EV_MAX_THRESHOLDS; ++k) a.thr[k] = v[7 + k];
  a.edge = v[11] != 0;
  a.edge_thr = v[12];
  a.r = v[13];
  if (B <= 0 || a.H <= 0 || a.W <= 0 || Hl < a.H || Wl < a.W || a.nthr < 0 || a.nthr > EV_MAX_THRESHOLDS || a.r < 0 ||
      a.r > EV_RMAX)
    return 2;
  if (bits == 8) return run<unsigned char>(a, B, Hl, argv[15], argv[16], argv[17]);
  if (bits == 16) return run<unsigned short>(a, B, Hl, argv[15], argv[16], argv[17]);
  return 2;
}
