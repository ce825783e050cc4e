// Surface-normal angle error of codon_amd.metrics.normal_errors: per image a 1441-bin histogram of the angle between
// the label's normal and the output's, in eighths of a degree, and four counts, in ONE launch for a batch, plus an optional angle
// map.  The normals are cloud's (cloud_tile.h's cd_normal, the one text), the angle an integer atan2 by bisection over two tables.
// A DEFINITION of this project, restated in numpy in tests/normal_errors_ref.py, and the kernel is held to its words and maps:
// integers only, so the words do not depend on the order of summation.
//
// One workgroup of 256 threads owns a 32 x 32 tile of one image.  The label tile plus a halo of `radius`, the output tile behind
// the label's mask, the tile's rays, both angle tables and the histogram live in LDS (26 884 bytes with u16 codes); the workgroup
// body and its phases are in normal_tile.h, and the host-side sanitizer check calls the same body.  The four counts
// are reduced as eval.hip reduces its words: __shfl_xor over 64 lanes, the four waves through LDS, one global atomic per count.

#include "codon_common.h"
#include "kernels.h"
#include "normal_tile.h"

namespace codon {

// grid (ne_tiles(W), ne_tiles(H), B)
template <typename T>
__global__ __launch_bounds__(NE_THREADS) void normal_errors_kernel(NeArgs a, const T* __restrict__ label, const T* __restrict__ out,
                                                                   const int* __restrict__ rx, const int* __restrict__ ry,
                                                                   const int* __restrict__ ctab, const int* __restrict__ stab,
                                                                   unsigned* __restrict__ words /* (B, NE_WORDS) */,
                                                                   unsigned short* __restrict__ amap) {
  __shared__ T lab[NE_SIDE * NE_SIDE];
  __shared__ T outm[NE_SIDE * NE_SIDE];
  __shared__ int rxs[NE_SIDE];
  __shared__ int rys[NE_SIDE];
  __shared__ int cosine[NE_ANGLES];
  __shared__ int sine[NE_ANGLES];
  __shared__ unsigned hist[NE_BINS];
  __shared__ unsigned red[NE_THREADS / 64][NE_COUNTS];
  const int b = blockIdx.z, tid = threadIdx.x;
  WgDevice::Regs<unsigned, NE_COUNTS> regs{WgDevice()};
  wg_normal_errors<T>(WgDevice(), blockIdx.x, blockIdx.y, b, a, label, out, rx, ry, ctab, stab, words, amap, lab, outm, rxs, rys,
                      cosine, sine, hist, regs);
  unsigned* c = regs[tid];                                          // the reduction: the device's own
#pragma unroll
  for (int k = 0; k < NE_COUNTS; ++k) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c[k] += __shfl_xor(c[k], m, 64);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NE_COUNTS; ++k) red[tid >> 6][k] = c[k];
  }
  __syncthreads();
  if (tid < NE_COUNTS) {
    unsigned v = red[0][tid];
    for (int q = 1; q < NE_THREADS / 64; ++q) v += red[q][tid];
    if (v != 0u) atomicAdd(&words[(long)b * NE_WORDS + NE_BINS + tid], v);     // the entry zeroed the words
  }
}

int normal_errors(const NeArgs& a, int B, int fmt, const void* label, const void* out, const int* rx, const int* ry, const int* ctab,
                  const int* stab, unsigned* words, unsigned short* amap, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(words, 0, (size_t)B * NE_WORDS * sizeof(unsigned), stream);
  if (e != hipSuccess) { set_error("normal_errors: memset: %s", hipGetErrorString(e)); return CODON_ERR_LAUNCH; }
  const dim3 grid((unsigned)ne_tiles(a.W), (unsigned)ne_tiles(a.H), (unsigned)B);
  if (fmt == FL_U16) {
    typedef unsigned short T;
    hipLaunchKernelGGL(normal_errors_kernel<T>, grid, dim3(NE_THREADS), 0, stream, a, (const T*)label, (const T*)out, rx, ry, ctab,
                       stab, words, amap);
  } else {
    typedef unsigned char T;
    hipLaunchKernelGGL(normal_errors_kernel<T>, grid, dim3(NE_THREADS), 0, stream, a, (const T*)label, (const T*)out, rx, ry, ctab,
                       stab, words, amap);
  }
  return check_launch("normal_errors_kernel");
}

}  // namespace codon
