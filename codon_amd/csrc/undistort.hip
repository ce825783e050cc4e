// Undistortion of colour images (codon_amd.undistort): the image of a camera with Brown distortion resampled to a
// pinhole camera, the step codon_amd.register asks for.  A DEFINITION of this project, in integers, restated in numpy in
// tests/undistort_ref.py; the kernel is held to its bits.  Grey and RGB u8 images, interleaved; the launch plan, the host's tile
// table, the workgroup body and the per-pixel arithmetic are in undistort_tile.h, and the host-side sanitizer check calls the same
// body.
//
// ONE launch, a function of (B, ho, wo) alone; no workspace, no atomics, no wait on another workgroup, no host synchronisation:
//   undistort_kernel<C>   per 32 x 8 tile of target pixels: the map entry of the thread's pixel (one 8-byte load), the 128 weights
//                         into LDS (256 bytes), for a STAGED tile the 48 x 24 window of the source into LDS (one word a cell, 4608
//                         bytes), one barrier, one pixel per thread: 16 taps from the window or, for a DIRECT tile, from
//                         global memory; an EMPTY tile writes zeros and loads nothing but its tile entry

#include "codon_common.h"
#include "kernels.h"
#include "undistort_tile.h"

namespace codon {

// grid (tx, ty, B) of ud_plan
template <int C>
__global__ __launch_bounds__(UD_THREADS) void undistort_kernel(const unsigned char* __restrict__ in, int hs, int ws, int ho, int wo,
                                                               const int* __restrict__ map, const int* __restrict__ tiles,
                                                               const short* __restrict__ weights, unsigned char* __restrict__ out) {
  __shared__ __attribute__((aligned(8))) short lk[UD_WEIGHTS];
  __shared__ unsigned win[UD_WIN];
  wg_undistort_tile<C>(WgDevice(), (int)blockIdx.x, (int)blockIdx.y, (long)blockIdx.z, in, hs, ws, ho, wo, map, tiles, weights, out,
                       lk, win);
}

size_t undistort_tiles_bytes(int ho, int wo) {
  if (ho < 1 || ho > UD_MAX_SIDE || wo < 1 || wo > UD_MAX_SIDE) return 0;
  const UdPlan p = ud_plan(ho, wo);
  return (size_t)p.tx * p.ty * 4 * sizeof(int);
}

// HOST: here, beside the kernel, so that one translation unit holds everything -DCODON_UD_STAGE=0 changes (tools/ab_build.sh)
long undistort_plan(int hs, int ws, int ho, int wo, const int* map, int* tiles, unsigned* counts) {
  return ud_tiles(hs, ws, ho, wo, map, tiles, counts);
}

int undistort(int B, int hs, int ws, int channels, const void* in, int ho, int wo, const void* map, const void* tiles,
              const void* weights, void* out, hipStream_t stream) {
  const UdPlan p = ud_plan(ho, wo);
  const dim3 grid((unsigned)p.tx, (unsigned)p.ty, (unsigned)B);
  if (channels == 1)
    hipLaunchKernelGGL((undistort_kernel<1>), grid, dim3(UD_THREADS), 0, stream, (const unsigned char*)in, hs, ws, ho, wo,
                       (const int*)map, (const int*)tiles, (const short*)weights, (unsigned char*)out);
  else
    hipLaunchKernelGGL((undistort_kernel<3>), grid, dim3(UD_THREADS), 0, stream, (const unsigned char*)in, hs, ws, ho, wo,
                       (const int*)map, (const int*)tiles, (const short*)weights, (unsigned char*)out);
  return check_launch("undistort_kernel");
}

}  // namespace codon
