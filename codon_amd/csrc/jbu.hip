// Joint bilateral upsampling of low-resolution code planes (codon_amd.upsample.joint_bilateral_upsample): the
// classical guided baseline beside the network (Kopf et al. 2007) on the bicubic's own 4 x 4 footprint, the range weight the
// guided hole filler's table, the spatial weight a per-phase table.  A DEFINITION of this project, in integers, restated in
// numpy in tests/jbu_ref.py; the kernels are held to its bits.  u8 and u16 codes; the launch plan, the workgroup bodies and their
// phases are in jbu_tile.h, and the host-side sanitizer check calls the same bodies.
//
// TWO launches, a function of (B, h, w, scale) alone; no atomics, no flag, no wait on another workgroup:
//   jbu_g0_kernel   per 64 x 64 tile of cells: G_0, the box means of the guidance, to the workspace plane (the guided filler's
//                   reduction; LDS 4096 bytes)
//   jbu_kernel      per 128 x 32 tile of high-resolution pixels: the footprint's codes and G_0 and the two tables in LDS (at x4
//                   864 + 432 + 512 + 32 = 1840 bytes), one run of 16 pixels per thread

#include "codon_common.h"
#include "jbu_tile.h"
#include "kernels.h"

namespace codon {

// grid (g0x, g0y, B) of jb_plan
__global__ __launch_bounds__(FL_THREADS) void jbu_g0_kernel(const unsigned char* __restrict__ guide, long row_bytes, long image_bytes,
                                                            int scale, int h, int w, unsigned char* __restrict__ ws, long ws_stride) {
  __shared__ unsigned char g[FL_TILE * FL_TILE];
  wg_jbu_g0(WgDevice(), blockIdx.x, blockIdx.y, blockIdx.z, guide, row_bytes, image_bytes, scale, h, w, ws, ws_stride, g);
}

// grid (gx, gy, B) of jb_plan
template <int S, int FMT>
__global__ __launch_bounds__(JB_THREADS) void jbu_kernel(const void* __restrict__ in, int h, int w,
                                                         const unsigned char* __restrict__ guide, long row_bytes, long image_bytes,
                                                         const unsigned short* __restrict__ rtab,
                                                         const unsigned short* __restrict__ stab,
                                                         const unsigned char* __restrict__ ws, long ws_stride,
                                                         void* __restrict__ out) {
  __shared__ unsigned short lc[JbShape<S>::CELLS];
  __shared__ unsigned char lg[JbShape<S>::CELLS];
  __shared__ unsigned short t[FG_TAB];
  __shared__ unsigned short st[S * 4];
  wg_jbu<S, FMT>(WgDevice(), blockIdx.x, blockIdx.y, blockIdx.z, in, h, w, guide, row_bytes, image_bytes, rtab, stab, ws, ws_stride,
                 out, lc, lg, t, st);
}

template <int S, int FMT>
static int jbu_launch(int B, int h, int w, const void* in, const unsigned char* guide, long row_bytes, long image_bytes,
                      const unsigned short* rtab, const unsigned short* stab, void* out, unsigned char* ws, hipStream_t stream) {
  const JbPlan p = jb_plan(h, w, S);
  hipLaunchKernelGGL(jbu_g0_kernel, dim3((unsigned)p.g0x, (unsigned)p.g0y, (unsigned)B), dim3(FL_THREADS), 0, stream, guide,
                     row_bytes, image_bytes, S, h, w, ws, p.stride);
  const int st = check_launch("jbu_g0_kernel");
  if (st != CODON_OK) return st;
  hipLaunchKernelGGL((jbu_kernel<S, FMT>), dim3((unsigned)p.gx, (unsigned)p.gy, (unsigned)B), dim3(JB_THREADS), 0, stream, in, h, w,
                     guide, row_bytes, image_bytes, rtab, stab, (const unsigned char*)ws, p.stride, out);
  return check_launch("jbu_kernel");
}

size_t jbu_workspace_bytes(int h, int w) {
  if (h < 1 || h > FL_MAX_SIDE || w < 1 || w > FL_MAX_SIDE) return 0;
  return (size_t)jb_plan(h, w, 4).stride;
}

int jbu_upsample(int B, int h, int w, const void* in, int fmt, const void* guide, long row_bytes, long image_bytes, int scale,
                 const void* range_tab, const void* spatial_tab, void* out, void* workspace, hipStream_t stream) {
#define CODON_JBU(S_)                                                                                                      \
  return fmt == FL_U8 ? jbu_launch<S_, FL_U8>(B, h, w, in, (const unsigned char*)guide, row_bytes, image_bytes,           \
                                               (const unsigned short*)range_tab, (const unsigned short*)spatial_tab, out, \
                                               (unsigned char*)workspace, stream)                                         \
                      : jbu_launch<S_, FL_U16>(B, h, w, in, (const unsigned char*)guide, row_bytes, image_bytes,          \
                                                (const unsigned short*)range_tab, (const unsigned short*)spatial_tab, out, \
                                                (unsigned char*)workspace, stream)
  if (scale == 4) { CODON_JBU(4); }
  if (scale == 8) { CODON_JBU(8); }
  CODON_JBU(16);
#undef CODON_JBU
}

}  // namespace codon
