// The per-element and per-thread bodies of the per-image range normalisation of depth codes (stretch.hip), written
// so that the SAME text compiles for the device and for a plain host compiler: tools/stretch_host_check.cpp drives them
// workgroup by workgroup, thread by thread, under the address and undefined-behaviour sanitizers.  Integers only.
//
// A plane of n codes on the grid 0 .. top, 0 a hole.  Its range (lo, hi) is the smallest non-zero and the largest code, (0, 0)
// without a valid code.  With T = top - 1 and n = hi - lo
//   stretch    c == 0 -> 0;  else 1 + (2 k T + n) / (2 n),  k = clamp(c, lo, hi) - lo     (n == 0 -> top)
//   unstretch  lo + (2 (max(o, 1) - 1) n + T) / (2 T)
// in 64-bit integer division (2 * 65534 * 65534 does not fit 32 bits).  A range that is not 1 <= lo <= hi <= top -- (0, 0)
// above all -- makes both the identity.  unstretch(stretch(c)) == c on [lo, hi] because n <= T.
//
// Work is cut into RUNS of ST_RUN = 8 consecutive codes, run r of a plane being its codes 8 r .. 8 r + 7; a thread owns whole
// runs.  THE ALIGNMENT RULE, stated here once: a plane may start at any element boundary (the training pool packs u8 planes
// at byte offsets and u16 planes at even ones), so a full run moves as ONE vector access -- 8 bytes of u8 codes, 16 bytes of
// u16 codes -- exactly when every plane pointer of the workgroup's image is a multiple of that width (st_wide: then every run
// is, since runs are 8 elements apart), and as 8 element accesses otherwise; the plane's last, partial run always moves by
// elements.  The choice is uniform over the workgroup and depends on the pointers and the size alone.
//   st_range_thread   the thread's partial range over its runs, as (smallest non-zero code or ST_NONE, largest code)
//   st_fold_lo/_hi    two partial ranges into one: what the wave shuffles and the LDS pass across waves apply
//   st_range_close    the partial range of the whole plane -> (lo, hi)
//   st_map_thread     the thread's one run, stretched (DIR 0) or unstretched (DIR 1), from `in` to `out` (which may be `in`)
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define CODON_ST_HD __host__ __device__ __forceinline__
#else
#define CODON_ST_HD inline
#endif

namespace codon {

constexpr int ST_RUN = 8;                                    // codes per run
constexpr int ST_RANGE_THREADS = 1024;                       // code_range: one workgroup of 16 waves per image
constexpr int ST_MAP_THREADS = 256;                          // stretch / unstretch: one run per thread
constexpr int ST_MAX_SIDE = 16384;                           // planes up to 16384 x 16384: run indices fit an int
constexpr int ST_U8 = 0, ST_U16 = 1;
constexpr int ST_STRETCH = 0, ST_UNSTRETCH = 1;
constexpr int ST_NONE = 0x7fffffff;                          // "no valid code yet" as a smallest code

CODON_ST_HD int st_elem_bytes(int fmt) { return fmt == ST_U8 ? 1 : 2; }
CODON_ST_HD bool st_range_ok(int lo, int hi, int top) { return lo >= 1 && lo <= hi && hi <= top; }
// every plane pointer that is OR-ed into `ptrs` is a multiple of the run's bytes
CODON_ST_HD bool st_wide(uintptr_t ptrs, int fmt) { return (ptrs & (uintptr_t)(ST_RUN * st_elem_bytes(fmt) - 1)) == 0; }

CODON_ST_HD int st_stretch(int c, int lo, int hi, int top) {
  if (c == 0 || !st_range_ok(lo, hi, top)) return c;
  const int n = hi - lo;
  if (n == 0) return top;
  const int k = (c < lo ? lo : c > hi ? hi : c) - lo;
  return 1 + (int)((2 * (int64_t)k * (top - 1) + n) / (2 * (int64_t)n));
}

CODON_ST_HD int st_unstretch(int o, int lo, int hi, int top) {
  if (!st_range_ok(lo, hi, top)) return o;
  const int64_t T = top - 1;
  const int q = (o < 1 ? 1 : o > top ? top : o) - 1;
  return lo + (int)((2 * (int64_t)q * (hi - lo) + T) / (2 * T));
}

template <int DIR>
CODON_ST_HD int st_map(int c, int lo, int hi, int top) {
  return DIR == ST_STRETCH ? st_stretch(c, lo, hi, top) : st_unstretch(c, lo, hi, top);
}

// one run of the plane `p` (element type of FMT) at element `at`: `count` codes (1 .. 8) into v; wide: count == 8 and aligned
template <int FMT>
CODON_ST_HD void st_run_load(const void* p, long at, int count, bool wide, int v[ST_RUN]) {
  if (FMT == ST_U8) {
    const unsigned char* s = (const unsigned char*)p + at;
    if (wide && count == ST_RUN) {
      unsigned char b[ST_RUN];
      memcpy(b, __builtin_assume_aligned(s, ST_RUN), ST_RUN);
      for (int j = 0; j < ST_RUN; ++j) v[j] = b[j];
    } else {
      for (int j = 0; j < ST_RUN; ++j) v[j] = j < count ? s[j] : 0;
    }
  } else {
    const unsigned short* s = (const unsigned short*)p + at;
    if (wide && count == ST_RUN) {
      unsigned short b[ST_RUN];
      memcpy(b, __builtin_assume_aligned(s, 2 * ST_RUN), 2 * ST_RUN);
      for (int j = 0; j < ST_RUN; ++j) v[j] = b[j];
    } else {
      for (int j = 0; j < ST_RUN; ++j) v[j] = j < count ? s[j] : 0;
    }
  }
}

template <int FMT>
CODON_ST_HD void st_run_store(void* p, long at, int count, bool wide, const int v[ST_RUN]) {
  if (FMT == ST_U8) {
    unsigned char* d = (unsigned char*)p + at;
    if (wide && count == ST_RUN) {
      unsigned char b[ST_RUN];
      for (int j = 0; j < ST_RUN; ++j) b[j] = (unsigned char)v[j];
      memcpy(__builtin_assume_aligned(d, ST_RUN), b, ST_RUN);
    } else {
      for (int j = 0; j < count; ++j) d[j] = (unsigned char)v[j];
    }
  } else {
    unsigned short* d = (unsigned short*)p + at;
    if (wide && count == ST_RUN) {
      unsigned short b[ST_RUN];
      for (int j = 0; j < ST_RUN; ++j) b[j] = (unsigned short)v[j];
      memcpy(__builtin_assume_aligned(d, 2 * ST_RUN), b, 2 * ST_RUN);
    } else {
      for (int j = 0; j < count; ++j) d[j] = (unsigned short)v[j];
    }
  }
}

CODON_ST_HD int st_fold_lo(int a, int b) { return a < b ? a : b; }
CODON_ST_HD int st_fold_hi(int a, int b) { return a > b ? a : b; }

// thread `tid` of `threads`: runs tid, tid + threads, ... of the n-element plane
template <int FMT>
CODON_ST_HD void st_range_thread(int tid, int threads, const void* plane, long n, bool wide, int* lo, int* hi) {
  int mn = ST_NONE, mx = 0;
  const long runs = (n + ST_RUN - 1) / ST_RUN;
  for (long r = tid; r < runs; r += threads) {
    const long at = r * ST_RUN;
    const int count = n - at < ST_RUN ? (int)(n - at) : ST_RUN;
    int v[ST_RUN];
    st_run_load<FMT>(plane, at, count, wide, v);
    for (int j = 0; j < ST_RUN; ++j) {                           // a code past the plane's end was loaded as 0: a hole
      mn = st_fold_lo(mn, v[j] ? v[j] : ST_NONE);
      mx = st_fold_hi(mx, v[j]);
    }
  }
  *lo = mn;
  *hi = mx;
}

CODON_ST_HD void st_range_close(int mn, int mx, int* lo_hi) {
  lo_hi[0] = mn == ST_NONE ? 0 : mn;
  lo_hi[1] = mx;
}

// run `r` (< ceil(n / 8)) of the n-element plane
template <int FMT, int DIR>
CODON_ST_HD void st_map_thread(long r, const void* in, void* out, long n, bool wide, int lo, int hi, int top) {
  const long at = r * ST_RUN;
  const int count = n - at < ST_RUN ? (int)(n - at) : ST_RUN;
  int v[ST_RUN];
  st_run_load<FMT>(in, at, count, wide, v);
  for (int j = 0; j < ST_RUN; ++j) v[j] = st_map<DIR>(v[j], lo, hi, top);
  st_run_store<FMT>(out, at, count, wide, v);
}

}  // namespace codon
