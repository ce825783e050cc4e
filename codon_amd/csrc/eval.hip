// Depth evaluation suite of codon_amd.metrics.depth_errors: per image sixteen exact u64 words -- count, sum |e|,
// sum e^2, max e, up to four bad-pixel counts, the three delta-inlier counts, and count / sum |e| / sum e^2 over the edge
// region -- plus an optional error map and region map, over u8 or u16 codes, in ONE launch for a batch.  The reference prints
// one masked RMSE and nothing else, so all of this is a DEFINITION, restated in numpy in tests/eval_ref.py, and the kernel is
// held to its bits: integers only (no floating point anywhere), so the words do not depend on the order of summation.
//
// One workgroup of 256 threads owns a 32 x 32 tile of one image.  The label tile plus a halo of r + 1 goes to LDS (50 x 50
// codes at r = 8); the discontinuity flags over tile + r are dilated separably there (a row OR, then a column OR); the workgroup
// body and its four phases are in eval_tile.h, and the host-side sanitizer check calls the same body.  Each
// thread accumulates its pixels in registers; the wave reduces by __shfl_xor over 64 lanes, the four waves through LDS, and the
// workgroup issues one u64 atomicAdd / atomicMax per accumulator it touched.  The label is read through its own row stride,
// top-left: no cropped copy.
// Bounds: |e| <= 65535, e^2 < 2^32, at most 2^26 pixels per image, so every sum stays below 2^58.

#include "codon_common.h"
#include "eval_tile.h"
#include "kernels.h"

namespace codon {

// grid (ev_tiles(W), ev_tiles(H), B)
template <typename T>
__global__ __launch_bounds__(EV_THREADS) void depth_errors_kernel(EvalArgs a, const T* __restrict__ label,
                                                                  const T* __restrict__ out, T* __restrict__ err,
                                                                  unsigned char* __restrict__ region,
                                                                  unsigned long long* __restrict__ acc /* (B, 16) */) {
  __shared__ T lab[EV_SIDE][EV_SIDE];
  __shared__ unsigned char flag[EV_FSIDE][EV_FSIDE];
  __shared__ unsigned char rowor[EV_FSIDE][EV_TILE];
  __shared__ unsigned long long red[EV_THREADS / 64][EV_WORDS];
  const int b = blockIdx.z, tid = threadIdx.x;
  WgDevice::Regs<unsigned long long, EV_WORDS> regs{WgDevice()};
  wg_eval_tile<T>(WgDevice(), blockIdx.x, blockIdx.y, b, a, label, out, err, region, lab, flag, rowor, regs);
  unsigned long long* w = regs[tid];                               // the reduction: the device's own
#pragma unroll
  for (int k = 0; k < 14; ++k) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const unsigned long long o = __shfl_xor(w[k], m, 64);
      w[k] = k == 3 ? (o > w[k] ? o : w[k]) : w[k] + o;
    }
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 14; ++k) red[tid >> 6][k] = w[k];
  }
  __syncthreads();
  if (tid < 14) {
    unsigned long long v = red[0][tid];
    for (int q = 1; q < EV_THREADS / 64; ++q) v = tid == 3 ? (red[q][tid] > v ? red[q][tid] : v) : v + red[q][tid];
    if (v != 0) {                                                  // the entry zeroed the words: adding 0 changes nothing
      if (tid == 3) atomicMax(&acc[(long)b * EV_WORDS + tid], v);
      else atomicAdd(&acc[(long)b * EV_WORDS + tid], v);
    }
  }
}

int depth_errors(const EvalArgs& a, int B, int bits, const void* label, const void* out, void* err, unsigned char* region,
                 unsigned long long* acc, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(acc, 0, (size_t)B * EV_WORDS * sizeof(unsigned long long), stream);
  if (e != hipSuccess) { set_error("depth_errors: memset: %s", hipGetErrorString(e)); return CODON_ERR_LAUNCH; }
  const dim3 grid((unsigned)ev_tiles(a.W), (unsigned)ev_tiles(a.H), (unsigned)B);
  if (bits == 16) {
    typedef unsigned short T;
    hipLaunchKernelGGL(depth_errors_kernel<T>, grid, dim3(EV_THREADS), 0, stream, a, (const T*)label, (const T*)out, (T*)err,
                       region, acc);
  } else {
    typedef unsigned char T;
    hipLaunchKernelGGL(depth_errors_kernel<T>, grid, dim3(EV_THREADS), 0, stream, a, (const T*)label, (const T*)out, (T*)err,
                       region, acc);
  }
  return check_launch("depth_errors_kernel");
}

}  // namespace codon
