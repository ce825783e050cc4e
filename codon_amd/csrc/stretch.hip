// Per-image range normalisation of depth codes (codon_amd.upsample.code_range / stretch_codes /
// unstretch_codes): the valid codes [lo, hi] of a plane are stretched onto [1, top] of the data's own grid, code 0 -- a hole --
// stays 0, and the network's output codes are mapped back.  A DEFINITION of this project, in integers, restated in numpy in
// tests/stretch_ref.py; the kernels are held to its bits.  The per-element and per-thread bodies, and the alignment rule of
// the 8-code runs, are in stretch_tile.h, shared with the host-side sanitizer check.
//
//   code_range_kernel   grid (B), ST_RANGE_THREADS threads: every thread folds its runs, every wave folds its lanes by
//                       shuffles, LDS carries the 16 wave results to wave 0, which folds them and writes (lo, hi) of the image.
//                       No atomics, no initialisation launch; min and max are exact, so the order of folding is immaterial.
//   map_kernel<DIR>     grid (ceil(runs / ST_MAP_THREADS), B): one thread per run, the image's range read from device memory
//                       (a uniform load); out may be in.
// The launches depend on (B, h, w) alone.

#include "codon_common.h"
#include "kernels.h"
#include "stretch_tile.h"

namespace codon {

template <int FMT>
__global__ __launch_bounds__(ST_RANGE_THREADS) void code_range_kernel(const void* __restrict__ codes, long n,
                                                                      int* __restrict__ lo_hi) {
  __shared__ int part[2 * (ST_RANGE_THREADS / 64)];
  const int tid = threadIdx.x;
  const long b = blockIdx.x;
  const char* plane = (const char*)codes + b * n * st_elem_bytes(FMT);
  int mn, mx;
  st_range_thread<FMT>(tid, ST_RANGE_THREADS, plane, n, st_wide((uintptr_t)plane, FMT), &mn, &mx);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    mn = st_fold_lo(mn, __shfl_xor(mn, d));
    mx = st_fold_hi(mx, __shfl_xor(mx, d));
  }
  if ((tid & 63) == 0) {
    part[2 * (tid >> 6)] = mn;
    part[2 * (tid >> 6) + 1] = mx;
  }
  __syncthreads();
  if (tid < 64) {                                                  // wave 0: lanes 0 .. 15 hold a wave's result each
    constexpr int WAVES = ST_RANGE_THREADS / 64;
    mn = tid < WAVES ? part[2 * tid] : ST_NONE;
    mx = tid < WAVES ? part[2 * tid + 1] : 0;
#pragma unroll
    for (int d = WAVES / 2; d >= 1; d >>= 1) {
      mn = st_fold_lo(mn, __shfl_xor(mn, d));
      mx = st_fold_hi(mx, __shfl_xor(mx, d));
    }
    if (tid == 0) st_range_close(mn, mx, lo_hi + 2 * b);
  }
}

template <int FMT, int DIR>
__global__ __launch_bounds__(ST_MAP_THREADS) void map_kernel(const void* in, void* out, long n, int top,
                                                             const int* __restrict__ lo_hi) {
  const long b = blockIdx.y;
  const long r = (long)blockIdx.x * ST_MAP_THREADS + threadIdx.x;
  const char* src = (const char*)in + b * n * st_elem_bytes(FMT);
  char* dst = (char*)out + b * n * st_elem_bytes(FMT);
  const int lo = lo_hi[2 * b], hi = lo_hi[2 * b + 1];
  if (r * ST_RUN < n) st_map_thread<FMT, DIR>(r, src, dst, n, st_wide((uintptr_t)src | (uintptr_t)dst, FMT), lo, hi, top);
}

int code_range(int B, long n, const void* codes, int fmt, int* lo_hi, hipStream_t stream) {
  if (fmt == ST_U8)
    hipLaunchKernelGGL(code_range_kernel<ST_U8>, dim3((unsigned)B), dim3(ST_RANGE_THREADS), 0, stream, codes, n, lo_hi);
  else
    hipLaunchKernelGGL(code_range_kernel<ST_U16>, dim3((unsigned)B), dim3(ST_RANGE_THREADS), 0, stream, codes, n, lo_hi);
  return check_launch("code_range_kernel");
}

template <int FMT, int DIR>
static int map_launch(int B, long n, const void* in, int top, const int* lo_hi, void* out, hipStream_t stream) {
  const long runs = (n + ST_RUN - 1) / ST_RUN;
  const dim3 grid((unsigned)((runs + ST_MAP_THREADS - 1) / ST_MAP_THREADS), (unsigned)B);
  hipLaunchKernelGGL((map_kernel<FMT, DIR>), grid, dim3(ST_MAP_THREADS), 0, stream, in, out, n, top, lo_hi);
  return check_launch(DIR == ST_STRETCH ? "stretch_kernel" : "unstretch_kernel");
}

int map_codes(int dir, int B, long n, const void* in, int fmt, int top, const int* lo_hi, void* out, hipStream_t stream) {
  if (dir == ST_STRETCH)
    return fmt == ST_U8 ? map_launch<ST_U8, ST_STRETCH>(B, n, in, top, lo_hi, out, stream)
                        : map_launch<ST_U16, ST_STRETCH>(B, n, in, top, lo_hi, out, stream);
  return fmt == ST_U8 ? map_launch<ST_U8, ST_UNSTRETCH>(B, n, in, top, lo_hi, out, stream)
                      : map_launch<ST_U16, ST_UNSTRETCH>(B, n, in, top, lo_hi, out, stream);
}

}  // namespace codon
