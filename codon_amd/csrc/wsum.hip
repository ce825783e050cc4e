// Stale-packed-weight guard: ONE launch per forward folds a position-dependent 64-bit checksum of the raw bytes of every
// MFMA conv weight (17 tensors, 7.4 MB in fp32) and compares it with the checksum taken when the packed images were
// built.  A write that the host-side cache key (data_ptr, Tensor._version) cannot see -- `w.data.normal_()`, the
// reference's own init idiom, /root/reference/CODON_X4/CODON_x4.py:50-53 -- sets a sticky flag in host-visible memory;
// codon_amd.model raises on the next call or synchronisation point instead of serving stale weights silently.
//
// The checksum is a sum of 64-bit terms (integer addition: any order gives the same value, so the grid may reduce in
// any shape): term(i, w) = (w + 0x9E3779B9) * (2 i + 1) * 0x9E3779B97F4A7C15 mod 2^64 for the 32-bit word w at global word
// index i.  Changing one word by d != 0 changes the sum by d * odd * odd != 0 mod 2^64: every single-word change is
// detected, and the odd position factor makes swaps visible.
#include "codon_common.h"
#include "kernels.h"

namespace codon {

// 64 workgroups x 1024 threads (one arrival atomic each: with 1024 workgroups the 1024 same-address atomics alone took
// ~40 us -- measured: the first version cost a 1 x 128 x 128 forward 50 us); a thread owns WS_U vectors per sweep, all
// requested before the first is used.  7.4 MB of fp32 weights = one sweep.
constexpr int WS_BLOCKS = 64, WS_THREADS = 1024, WS_U = 8;

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct WsumArgs {
  int n;
  unsigned nvec[CODON_WSUM_MAX + 1];      // prefix sums of 16-byte vectors per tensor
  const u32x4* data[CODON_WSUM_MAX];
};
static_assert(sizeof(WsumArgs) <= CODON_KERNARG_LIMIT, "passed by value as a kernel argument");

__device__ __forceinline__ unsigned long long wsum_term(unsigned w, unsigned long long i) {
  return ((unsigned long long)w + 0x9E3779B9ull) * (2ull * i + 1ull) * 0x9E3779B97F4A7C15ull;
}

__device__ __forceinline__ unsigned long long wsum_wave_sum(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o), hi = __shfl_xor((unsigned)(v >> 32), o);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

__global__ __launch_bounds__(WS_THREADS) void wsum_kernel(const WsumArgs a, unsigned long long* __restrict__ ws,
                                                           unsigned long long* __restrict__ ref, int mode,
                                                           int* __restrict__ flag, int* __restrict__ zero, int nzero) {
  __shared__ unsigned long long red[WS_THREADS / 64];
  __shared__ unsigned s_nvec[CODON_WSUM_MAX + 1];
  __shared__ const u32x4* s_data[CODON_WSUM_MAX];
  __shared__ bool last;
  const int tid = threadIdx.x;
  // this launch opens every forward on the forward's stream: it also clears the per-image words of the non-finite input
  // guard (stencil.hip) -- no launch of their own, and inside a captured graph with the rest
  if (zero && blockIdx.x == 0)
    for (int i = tid; i < nzero; i += WS_THREADS) zero[i] = 0;
  if (tid <= CODON_WSUM_MAX) s_nvec[tid] = a.nvec[tid];
  if (tid < CODON_WSUM_MAX) s_data[tid] = a.data[tid];
  __syncthreads();
  const unsigned total = s_nvec[CODON_WSUM_MAX];     // == nvec[n]: the host pads the prefix table
  unsigned long long acc = 0;
  for (unsigned base = blockIdx.x * (WS_THREADS * WS_U); base < total; base += WS_BLOCKS * WS_THREADS * WS_U) {
    u32x4 v[WS_U];
#pragma unroll
    for (int u = 0; u < WS_U; ++u) {
      const unsigned q = base + u * WS_THREADS + tid;
      int t = 0;                            // tensor of vector q: 5-step bisection of the 33-entry prefix table
#pragma unroll
      for (int step = CODON_WSUM_MAX / 2; step > 0; step >>= 1)
        if (q >= s_nvec[t + step]) t += step;
      v[u] = q < total ? __builtin_nontemporal_load(s_data[t] + (q - s_nvec[t])) : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int u = 0; u < WS_U; ++u) {
      const unsigned q = base + u * WS_THREADS + tid;
      if (q < total) {
        const unsigned long long i = 4ull * q;
        acc += wsum_term(v[u].x, i) + wsum_term(v[u].y, i + 1) + wsum_term(v[u].z, i + 2) + wsum_term(v[u].w, i + 3);
      }
    }
  }
  acc = wsum_wave_sum(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    unsigned long long s = 0;
    for (int k = 0; k < WS_THREADS / 64; ++k) s += red[k];
    ws[1 + blockIdx.x] = s;
    __threadfence();
    last = atomicAdd(&ws[0], 1ull) == WS_BLOCKS - 1;     // ws[0]: arrival counter, zero between launches
  }
  __syncthreads();
  if (!last) return;
  // the last workgroup to arrive folds the per-workgroup sums (all visible: release fence above, acquire fence below)
  __threadfence();
  if (tid < 64) {
    unsigned long long s = 0;
    for (int k = tid; k < WS_BLOCKS; k += 64) s += __atomic_load_n(&ws[1 + k], __ATOMIC_RELAXED);
    s = wsum_wave_sum(s);
    if (tid == 0) {
      ws[0] = 0;                                          // ready for the next launch on this workspace
      ws[1 + WS_BLOCKS] = s;                              // last value seen (diagnostics)
      if (mode == 0) {
        *ref = s;
      } else if (s != *ref) {
        __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // host-visible, sticky
      }
    }
  }
}

size_t weight_checksum_workspace_bytes() { return (size_t)(WS_BLOCKS + 2) * sizeof(unsigned long long); }

int weight_checksum(const codon_wsum_desc* d, void* ws, unsigned long long* ref, int mode, int* flag, int* zero, int nzero,
                    hipStream_t s) {
  WsumArgs a;
  a.n = d->n;
  a.nvec[0] = 0;
  for (int t = 0; t < d->n; ++t) {
    a.data[t] = (const u32x4*)d->data[t];
    a.nvec[t + 1] = a.nvec[t] + (unsigned)(d->bytes[t] / 16);
  }
  for (int t = d->n; t < CODON_WSUM_MAX; ++t) {
    a.data[t] = nullptr;
    a.nvec[t + 1] = a.nvec[d->n];
  }
  hipLaunchKernelGGL(wsum_kernel, dim3(WS_BLOCKS), dim3(WS_THREADS), 0, s, a, (unsigned long long*)ws, ref, mode, flag, zero, nzero);
  return check_launch("weight_checksum");
}

}  // namespace codon
