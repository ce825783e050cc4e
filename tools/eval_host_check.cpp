// Host-side check of the depth evaluation kernel: the workgroup body of csrc/eval_tile.h -- the very text the
// device kernel of csrc/eval.hip calls -- compiled for the host and run workgroup by workgroup over exactly-sized heap buffers
// (the LDS arrays too), so that the address and undefined-behaviour sanitizers see every access.  Only the wave / workgroup
// reduction after the body is the device's own; here the threads' words are added up (word 3: the maximum) in plain C++.  Every
// case runs with the threads of a workgroup forwards and backwards, and the two outputs must agree.  No GPU, no HIP, nothing
// loaded into Python.  `python tools/host_check.py eval` builds this, runs it over the GPU tests' cases and compares what it
// writes with tests/eval_ref.py, bit for bit.
//
//   eval_host_check <bits 8|16> B H W Hl Wl <nthr> t0 t1 t2 t3 <edge 0|1> T r label.bin out.bin out_prefix
//     label.bin: (B, Hl, Wl) codes, out.bin: (B, H, W) codes  ->  out_prefix.{acc (B,16) u64, err (B,H,W) codes, reg (B,H,W) u8}
#include "host_check.h"

#include "../codon_amd/csrc/eval_tile.h"

using namespace codon;

template <typename T>
static int run(const EvalArgs& a, int B, int Hl, const char* fl, const char* fo, const std::string& prefix) {
  const size_t n = (size_t)B * a.H * a.W, words = (size_t)B * EV_WORDS * sizeof(unsigned long long);
  T* label = hc_read<T>(fl, (size_t)B * Hl * a.label_row * sizeof(T));
  T* out = hc_read<T>(fo, n * sizeof(T));
  T* err[2];
  unsigned char* reg[2];
  unsigned long long* acc[2];
  for (int rev = 0; rev < 2; ++rev) {
    const WgHost wg{EV_THREADS, rev != 0};
    err[rev] = hc_alloc<T>(n * sizeof(T), 0xEE);
    reg[rev] = hc_alloc<unsigned char>(n, 0xEE);
    acc[rev] = hc_alloc<unsigned long long>(words, 0);              // the entry's memset
    for (int b = 0; b < B; ++b)                                     // the launch of depth_errors_kernel<T>
      for (int by = 0; by < ev_tiles(a.H); ++by)
        for (int bx = 0; bx < ev_tiles(a.W); ++bx) {
          typedef T LabRow[EV_SIDE];
          typedef unsigned char FlagRow[EV_FSIDE];
          typedef unsigned char OrRow[EV_TILE];
          LabRow* lab = hc_alloc<LabRow>(sizeof(LabRow) * EV_SIDE, 0xCD);
          FlagRow* flag = hc_alloc<FlagRow>(sizeof(FlagRow) * EV_FSIDE, 0xCD);
          OrRow* rowor = hc_alloc<OrRow>(sizeof(OrRow) * EV_FSIDE, 0xCD);
          WgHost::Regs<unsigned long long, EV_WORDS> w(wg);
          wg_eval_tile<T>(wg, bx, by, b, a, label, out, err[rev], reg[rev], lab, flag, rowor, w);
          for (int t = 0; t < EV_THREADS; ++t)
            for (int k = 0; k < EV_WORDS; ++k) {
              unsigned long long& d = acc[rev][(size_t)b * EV_WORDS + k];
              d = k == 3 ? (w[t][k] > d ? w[t][k] : d) : d + w[t][k];
            }
          free(lab);
          free(flag);
          free(rowor);
        }
  }
  const char* order = "the output depends on the order of the threads within a phase";
  hc_same(acc[0], acc[1], words, order);
  hc_same(err[0], err[1], n * sizeof(T), order);
  hc_same(reg[0], reg[1], n, order);
  hc_write(prefix + ".acc", acc[0], words);
  hc_write(prefix + ".err", err[0], n * sizeof(T));
  hc_write(prefix + ".reg", reg[0], n);
  free(label);
  free(out);
  for (int rev = 0; rev < 2; ++rev) free(err[rev]), free(reg[rev]), free(acc[rev]);
  return 0;
}

int main(int argc, char** argv) {
  hc_name = "eval_host_check";
  if (argc != 18) hc_die("usage: eval_host_check <8|16> B H W Hl Wl nthr t0 t1 t2 t3 edge T r label.bin out.bin out_prefix");
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
