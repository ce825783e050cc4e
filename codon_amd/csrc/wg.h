// One text for a workgroup's whole body.  A body is a function template over a group type G, written with
// explicit phases and explicit barriers:
//     WG_EACH(wg, tid) phase_a(tid, ...);          // every thread of the workgroup
//     wg.sync();
//     WG_EACH(wg, tid) phase_b(tid, ...);
// The kernel calls it with WgDevice and the host-side sanitizer check (tools/*_host_check.cpp) with WgHost: phase order,
// arguments, uniform branches, per-thread registers and address arithmetic exist once.  LDS arrays are no part of the group:
// the kernel declares them __shared__ and the host allocates each one on its own, exactly sized, and both pass pointers.
//   WgDevice  WG_EACH is one trip with tid = threadIdx.x, spelled as an `if` with an initialiser and not as a one-trip `for`:
//             with a `for` around them the compiler schedules the phases' unrolled loads differently (fill_push_kernel: 54 -> 70
//             VGPRs), with the `if` the code is the hand-strung kernel's; sync() is __syncthreads(); Regs<T, N> is a plain local
//             array.  Hence: WG_EACH takes one statement or a braced block, and never stands before an `else`;
//             atomic_min / atomic_max / atomic_add are the device's atomics on global memory, results not returned; atomic_min_old is the
//             same minimum and RETURNS what the word held, load_relaxed a relaxed load at agent scope (served by L2, never a
//             stale L1 line): the pair a lock-free union-find needs (clean_tile.h); lds_add is the add on a word
//             of an LDS array (normal_tile.h's histogram)
//   WgHost    WG_EACH runs tid over all threads, forwards or (reverse) backwards, so that a phase that reads what another thread
//             of the SAME phase writes gives different bytes in the two orders; sync() does nothing; Regs<T, N> is one
//             separately allocated row of exactly N elements per thread: a thread that writes past its registers is a report;
//             atomic_min / atomic_max / atomic_add / lds_add / atomic_min_old are a plain minimum, maximum and add, load_relaxed a plain load
//             (one thread runs at a time)
#pragma once

#if defined(__HIPCC__)

#define WG_EACH(wg, tid) if (const int tid = (wg).first(); true)

namespace codon {

struct WgDevice {
  template <typename T, int N>
  struct Regs {
    T v[N];
    __device__ __forceinline__ explicit Regs(const WgDevice&) {}
    __device__ __forceinline__ T* operator[](int) { return v; }
  };
  __device__ __forceinline__ int first() const { return threadIdx.x; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
  __device__ __forceinline__ void atomic_min(unsigned* p, unsigned v) const { atomicMin(p, v); }
  __device__ __forceinline__ void atomic_max(unsigned* p, unsigned v) const { atomicMax(p, v); }
  __device__ __forceinline__ void atomic_add(unsigned* p, unsigned v) const { atomicAdd(p, v); }
  __device__ __forceinline__ void lds_add(unsigned* p, unsigned v) const { atomicAdd(p, v); }
  __device__ __forceinline__ unsigned atomic_min_old(unsigned* p, unsigned v) const { return atomicMin(p, v); }
  __device__ __forceinline__ unsigned load_relaxed(const unsigned* p) const {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

}  // namespace codon

#else

#define WG_EACH(wg, tid) for (int tid = (wg).first(), wg_left_ = (wg).count(); wg_left_ > 0; --wg_left_, tid += (wg).step())

#include <stdlib.h>
#include <string.h>

namespace codon {

struct WgHost {
  int threads;
  bool reverse;
  template <typename T, int N>
  struct Regs {
    int threads;
    T** row;
    explicit Regs(const WgHost& wg) : threads(wg.threads), row((T**)malloc(sizeof(T*) * wg.threads)) {
      for (int t = 0; t < threads; ++t) row[t] = (T*)memset(malloc(sizeof(T) * N), 0xCD, sizeof(T) * N);
    }
    Regs(const Regs&) = delete;
    ~Regs() {
      for (int t = 0; t < threads; ++t) free(row[t]);
      free(row);
    }
    T* operator[](int tid) { return row[tid]; }
  };
  int first() const { return reverse ? threads - 1 : 0; }
  int count() const { return threads; }
  int step() const { return reverse ? -1 : 1; }
  void sync() const {}
  void atomic_min(unsigned* p, unsigned v) const { *p = v < *p ? v : *p; }
  void atomic_max(unsigned* p, unsigned v) const { *p = v > *p ? v : *p; }
  void atomic_add(unsigned* p, unsigned v) const { *p += v; }
  void lds_add(unsigned* p, unsigned v) const { *p += v; }
  unsigned atomic_min_old(unsigned* p, unsigned v) const {
    const unsigned old = *p;
    *p = v < old ? v : old;
    return old;
  }
  unsigned load_relaxed(const unsigned* p) const { return *p; }
};

}  // namespace codon

#endif
