// Host-side check of the range normalisation's run, tail and alignment arithmetic: the per-thread bodies of
// csrc/stretch_tile.h -- the very text the device kernels of csrc/stretch.hip call -- compiled for the host and driven launch by
// launch, workgroup by workgroup, thread by thread over exactly-sized heap buffers, so that the address and
// undefined-behaviour sanitizers see every access (a vector access off its alignment is an undefined-behaviour report).  The
// launch plans below are code_range's and map_launch's.  No GPU, no HIP, nothing loaded into Python.
// `python tools/host_check.py stretch` builds this, runs it over the GPU tests' shapes, patterns and formats and compares what it
// writes with tests/stretch_ref.py, bit for bit.
//
//   stretch_host_check <fmt 0|1> B n top skew in.bin range.bin stretched.bin back.bin
//     in.bin: (B, n) codes of the format; skew: the planes start that many ELEMENTS into a 16-byte aligned buffer (0: the first
//     image takes the vector path; 1: none does)  ->  range.bin: (B, 2) int32; stretched.bin, back.bin: (B, n) codes -- every
//     image stretched by its own range, and that unstretched again.  The stretch is also run in place and must agree.
#include "host_check.h"

#include "../codon_amd/csrc/stretch_tile.h"

using namespace codon;

// code_range_kernel<FMT>, workgroup b: the threads' partial ranges, folded as the shuffles and the LDS pass fold them
template <int FMT>
static void range_block(long b, const void* codes, long n, int* lo_hi) {
  const char* plane = (const char*)codes + b * n * st_elem_bytes(FMT);
  int mn = ST_NONE, mx = 0;
  for (int t = 0; t < ST_RANGE_THREADS; ++t) {
    int a, z;
    st_range_thread<FMT>(t, ST_RANGE_THREADS, plane, n, st_wide((uintptr_t)plane, FMT), &a, &z);
    mn = st_fold_lo(mn, a);
    mx = st_fold_hi(mx, z);
  }
  st_range_close(mn, mx, lo_hi + 2 * b);
}

// map_kernel<FMT, DIR>, the whole grid
template <int FMT, int DIR>
static void map_grid(int B, const void* in, void* out, long n, int top, const int* lo_hi) {
  const long runs = (n + ST_RUN - 1) / ST_RUN, gx = (runs + ST_MAP_THREADS - 1) / ST_MAP_THREADS;
  for (long b = 0; b < B; ++b)
    for (long bx = 0; bx < gx; ++bx)
      for (int t = 0; t < ST_MAP_THREADS; ++t) {
        const long r = bx * ST_MAP_THREADS + t;
        const char* src = (const char*)in + b * n * st_elem_bytes(FMT);
        char* dst = (char*)out + b * n * st_elem_bytes(FMT);
        if (r * ST_RUN < n)
          st_map_thread<FMT, DIR>(r, src, dst, n, st_wide((uintptr_t)src | (uintptr_t)dst, FMT), lo_hi[2 * b], lo_hi[2 * b + 1], top);
      }
}

template <int FMT>
static int run(int B, long n, int top, int skew, char** path) {
  const size_t eb = (size_t)st_elem_bytes(FMT), bytes = (size_t)B * n * eb, lead = (size_t)skew * eb;
  // exactly lead + bytes each: one element past the end is a sanitizer report
  char *in = hc_aligned(lead + bytes), *out = hc_aligned(lead + bytes), *back = hc_aligned(lead + bytes);
  char* place = hc_aligned(lead + bytes);
  int* lo_hi = hc_alloc<int>(sizeof(int) * 2 * B, 0xEE);        // code_range needs no initialisation
  hc_read(path[0], bytes, lead, in);
  memset(out, 0xEE, lead + bytes);                 // an element no thread writes stays this
  memset(back, 0xEE, lead + bytes);
  memcpy(place, in, lead + bytes);
  for (long b = 0; b < B; ++b) range_block<FMT>(b, in + lead, n, lo_hi);
  map_grid<FMT, ST_STRETCH>(B, in + lead, out + lead, n, top, lo_hi);
  map_grid<FMT, ST_STRETCH>(B, place + lead, place + lead, n, top, lo_hi);
  hc_same(place + lead, out + lead, bytes, "the stretch in place differs from the stretch into another buffer");
  map_grid<FMT, ST_UNSTRETCH>(B, out + lead, back + lead, n, top, lo_hi);
  hc_write(path[1], lo_hi, sizeof(int) * 2 * B);
  hc_write(path[2], out + lead, bytes);
  hc_write(path[3], back + lead, bytes);
  free(in);
  free(out);
  free(back);
  free(place);
  free(lo_hi);
  return 0;
}

int main(int argc, char** argv) {
  hc_name = "stretch_host_check";
  if (argc != 10) hc_die("usage: stretch_host_check <fmt 0|1> B n top skew in.bin range.bin stretched.bin back.bin");
  const int fmt = atoi(argv[1]), B = atoi(argv[2]), top = atoi(argv[4]), skew = atoi(argv[5]);
  const long n = atol(argv[3]);
  if (B < 1 || n < 1 || n > (long)ST_MAX_SIDE * ST_MAX_SIDE || top < 2 || top > 65535 || skew < 0 || skew > 15) return 2;
  if (fmt == ST_U8) return run<ST_U8>(B, n, top, skew, argv + 6);
  if (fmt == ST_U16) return run<ST_U16>(B, n, top, skew, argv + 6);
  return 2;
}
