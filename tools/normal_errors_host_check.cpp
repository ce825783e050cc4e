// Host-side check of the surface-normal angle error: the workgroup body of csrc/normal_tile.h -- the very
// text the device kernel of csrc/normal_errors.hip calls -- compiled for the host and run workgroup by workgroup over exactly-sized
// heap buffers (the LDS arrays too), so that the address and undefined-behaviour sanitizers see every access.  Only the wave /
// workgroup reduction of the four counts after the body is the device's own; here the threads' counts are added up in plain C++.
// Every case runs with the threads of a workgroup forwards and backwards, and the two outputs must agree.  No GPU, no HIP, nothing
// loaded into Python.  `python tools/host_check.py normal_errors` builds this, runs it over the GPU test's cases and compares what
// it writes with tests/normal_errors_ref.py, word for word.
//
//   normal_errors_host_check planes <fmt 0|1> B H W Hl Wl R A Rq label.bin out.bin rx.bin ry.bin cos.bin sin.bin out_prefix
//     label.bin: (B, Hl, Wl) codes, out.bin: (B, H, W) codes; rx.bin (Wl), ry.bin (Hl), cos.bin, sin.bin (1440 each): int32; A: the
//     tolerance per step  ->  out_prefix.{words (B, 1448) u32, map (B, H, W) u16}
//   normal_errors_host_check pairs n pairs.bin cos.bin sin.bin index.bin
//     pairs.bin: (n, 6) int32, two Q14 normals a row  ->  index.bin: (n) int32, ne_index of every row
#include "host_check.h"

#include "../codon_amd/csrc/normal_tile.h"

using namespace codon;

template <typename T>
static int planes(const NeArgs& a, int B, int Hl, int Wl, char** f, const std::string& prefix) {
  const size_t n = (size_t)B * a.H * a.W, words_bytes = (size_t)B * NE_WORDS * sizeof(unsigned);
  T* label = hc_read<T>(f[0], (size_t)B * Hl * Wl * sizeof(T));
  T* out = hc_read<T>(f[1], n * sizeof(T));
  int* rx = hc_read<int>(f[2], sizeof(int) * Wl);
  int* ry = hc_read<int>(f[3], sizeof(int) * Hl);
  int* ctab = hc_read<int>(f[4], sizeof(int) * NE_ANGLES);
  int* stab = hc_read<int>(f[5], sizeof(int) * NE_ANGLES);
  unsigned* words[2];
  unsigned short* amap[2];
  for (int rev = 0; rev < 2; ++rev) {
    const WgHost wg{NE_THREADS, rev != 0};
    words[rev] = hc_alloc<unsigned>(words_bytes, 0);                  // the entry's memset
    amap[rev] = hc_alloc<unsigned short>(n * sizeof(unsigned short), 0xEE);
    for (int b = 0; b < B; ++b)                                       // the launch of normal_errors_kernel<T>
      for (int by = 0; by < ne_tiles(a.H); ++by)
        for (int bx = 0; bx < ne_tiles(a.W); ++bx) {
          T* lab = hc_alloc<T>(sizeof(T) * NE_SIDE * NE_SIDE, 0xCD);
          T* outm = hc_alloc<T>(sizeof(T) * NE_SIDE * NE_SIDE, 0xCD);
          int* rxs = hc_alloc<int>(sizeof(int) * NE_SIDE, 0xCD);
          int* rys = hc_alloc<int>(sizeof(int) * NE_SIDE, 0xCD);
          int* cosine = hc_alloc<int>(sizeof(int) * NE_ANGLES, 0xCD);
          int* sine = hc_alloc<int>(sizeof(int) * NE_ANGLES, 0xCD);
          unsigned* hist = hc_alloc<unsigned>(sizeof(unsigned) * NE_BINS, 0xCD);
          WgHost::Regs<unsigned, NE_COUNTS> c(wg);
          wg_normal_errors<T>(wg, bx, by, b, a, label, out, rx, ry, ctab, stab, words[rev], amap[rev], lab, outm, rxs, rys, cosine,
                              sine, hist, c);
          for (int t = 0; t < NE_THREADS; ++t)
            for (int k = 0; k < NE_COUNTS; ++k) words[rev][(size_t)b * NE_WORDS + NE_BINS + k] += c[t][k];
          free(lab), free(outm), free(rxs), free(rys), free(cosine), free(sine), free(hist);
        }
  }
  const char* order = "the output depends on the order of the threads within a phase";
  hc_same(words[0], words[1], words_bytes, order);
  hc_same(amap[0], amap[1], n * sizeof(unsigned short), order);
  hc_write(prefix + ".words", words[0], words_bytes);
  hc_write(prefix + ".map", amap[0], n * sizeof(unsigned short));
  free(label), free(out), free(rx), free(ry), free(ctab), free(stab);
  for (int rev = 0; rev < 2; ++rev) free(words[rev]), free(amap[rev]);
  return 0;
}

static int pairs(int n, char** f) {
  int* pq = hc_read<int>(f[0], sizeof(int) * 6 * (size_t)n);
  int* ctab = hc_read<int>(f[1], sizeof(int) * NE_ANGLES);
  int* stab = hc_read<int>(f[2], sizeof(int) * NE_ANGLES);
  int* index = hc_alloc<int>(sizeof(int) * (size_t)n, 0xEE);
  for (int k = 0; k < n; ++k) index[k] = ne_index(pq + 6 * (size_t)k, pq + 6 * (size_t)k + 3, ctab, stab);
  hc_write(f[3], index, sizeof(int) * (size_t)n);
  free(pq), free(ctab), free(stab), free(index);
  return 0;
}

int main(int argc, char** argv) {
  hc_name = "normal_errors_host_check";
  const char* usage = "usage: normal_errors_host_check planes <0|1> B H W Hl Wl R A Rq label out rx ry cos sin out_prefix | "
                      "pairs n pairs cos sin index";
  if (argc == 7 && !strcmp(argv[1], "pairs")) {
    const int n = atoi(argv[2]);
    return n >= 1 ? pairs(n, argv + 3) : 2;
  }
  if (argc != 18 || strcmp(argv[1], "planes")) hc_die(usage);
  int v[9];
  for (int k = 0; k < 9; ++k) v[k] = atoi(argv[2 + k]);
  const int fmt = v[0], B = v[1], Hl = v[4], Wl = v[5], R = v[6], A = v[7], Rq = v[8];
  NeArgs a;
  a.H = v[2], a.W = v[3], a.label_row = Wl, a.label_image = (long)Hl * Wl;
  a.radius = R, a.tol_abs = (unsigned)(R * A), a.tol_rel = (unsigned)Rq;
  if (B <= 0 || a.H <= 0 || a.W <= 0 || Hl < a.H || Wl < a.W || R < 1 || R > NE_RMAX || A < 0 || A > 65535 || Rq < 0 || Rq > CD_MAX_REL)
    return 2;
  if (fmt == FL_U8) return planes<unsigned char>(a, B, Hl, Wl, argv + 11, argv[17]);
  if (fmt == FL_U16) return planes<unsigned short>(a, B, Hl, Wl, argv + 11, argv[17]);
  return 2;
}
