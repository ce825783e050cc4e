// Geometric (D4) self-ensemble of codon_amd.ensemble.self_ensemble: the eight flips and rotations of the two
// input planes in ONE launch, and the mean of the eight un-flipped, un-rotated network outputs in ONE launch.  The reference
// ships no self-ensemble, so both are DEFINITIONS, restated in numpy in tests/d4_ref.py, and the kernels are held to its bits:
// the views only copy bits; the merge upcasts exactly to fp32 and adds in a fixed tree,
//   out = 0.125f * (((u0+u1)+(u2+u3)) + ((u4+u5)+(u6+u7))),   u_k the inverse of view k of the network output,
// every add rounded on its own (built with -ffp-contract=off, like upsample.hip), so that eight equal values average to
// themselves exactly.  The D4 code is train_record.h's (crop_pixel); the workgroup bodies, the index arithmetic and the layout of the two
// view batches are in d4_tile.h, and the host-side sanitizer check calls the same bodies.
//
// Both kernels are HBM-bound permutations.  One workgroup of 256 threads owns a 32 x 32 tile; the transposed half goes through
// a padded LDS tile, so that every global read and write of every view runs along that view's contiguous axis; the flipped
// views are reversed indices only.  Ragged edges are predicated; offsets are 64-bit; no atomics.

#include "codon_common.h"
#include "d4_tile.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace codon {

// grid (d4_tiles(W), d4_tiles(H), B * planes)
template <typename T>
__global__ __launch_bounds__(D4_THREADS) void d4_views_kernel(const T* __restrict__ src0, const T* __restrict__ src1,
                                                              T* __restrict__ up0, T* __restrict__ tp0, T* __restrict__ up1,
                                                              T* __restrict__ tp1, int H, int W, int planes) {
  __shared__ T tile[D4_TILE][D4Stride<T>::value];
  wg_d4_views<T>(WgDevice(), blockIdx.x, blockIdx.y, blockIdx.z, src0, src1, up0, tp0, up1, tp1, H, W, planes, tile);
}

// grid (d4_tiles(W), d4_tiles(H), B)
template <int DT>
__global__ __launch_bounds__(D4_THREADS) void d4_merge_kernel(const void* __restrict__ upright, const void* __restrict__ transposed,
                                                              float* __restrict__ out, int H, int W) {
  __shared__ float lds[4][D4_TILE][D4_TILE + 1];
  wg_d4_merge<DT>(WgDevice(), blockIdx.x, blockIdx.y, blockIdx.z, upright, transposed, out, H, W, lds);
}

static dim3 d4_grid(int z, int H, int W) { return dim3((unsigned)d4_tiles(W), (unsigned)d4_tiles(H), (unsigned)z); }

int d4_views(int B, int H, int W, const void* src0, const void* src1, int dtype, void* up0, void* tp0, void* up1, void* tp1,
             hipStream_t stream) {
  const int planes = src1 ? 2 : 1;
  const dim3 grid = d4_grid(B * planes, H, W);
  if (dtype == CODON_F32) {
    typedef unsigned int T;
    hipLaunchKernelGGL(d4_views_kernel<T>, grid, dim3(D4_THREADS), 0, stream, (const T*)src0, (const T*)src1, (T*)up0, (T*)tp0,
                       (T*)up1, (T*)tp1, H, W, planes);
  } else {
    typedef unsigned short T;
    hipLaunchKernelGGL(d4_views_kernel<T>, grid, dim3(D4_THREADS), 0, stream, (const T*)src0, (const T*)src1, (T*)up0, (T*)tp0,
                       (T*)up1, (T*)tp1, H, W, planes);
  }
  return check_launch("d4_views_kernel");
}

int d4_merge(int B, int H, int W, const void* upright, const void* transposed, int dtype, float* out, hipStream_t stream) {
  const dim3 grid = d4_grid(B, H, W);
  if (dtype == CODON_F32)
    hipLaunchKernelGGL(d4_merge_kernel<CODON_F32>, grid, dim3(D4_THREADS), 0, stream, upright, transposed, out, H, W);
  else if (dtype == CODON_BF16)
    hipLaunchKernelGGL(d4_merge_kernel<CODON_BF16>, grid, dim3(D4_THREADS), 0, stream, upright, transposed, out, H, W);
  else
    hipLaunchKernelGGL(d4_merge_kernel<CODON_F16>, grid, dim3(D4_THREADS), 0, stream, upright, transposed, out, H, W);
  return check_launch("d4_merge_kernel");
}

}  // namespace codon
