// Pull-push hole filling of low-resolution code planes (codon_amd.upsample.fill_holes): code 0 is a hole, the
// plane is pulled up a pyramid of means over the valid children and pushed back down, a hole taking the 9/3/3/1 mix of the
// filled level above.  A DEFINITION of this project, in integers, restated in numpy in tests/fill_ref.py; the kernels are held
// to its bits.  u8 codes, u16 codes and fp32 on the code grid share the one integer core; the launch plan, the workgroup bodies and
// their phases are in fill_tile.h, and the host-side sanitizer check calls the same bodies.
//
// The launches depend on (B, h, w) alone, never on the hole pattern; no atomics, no flag, no wait on another workgroup: levels
// pass between workgroups only across kernel boundaries.
//   h, w <= 64 (every training crop):  ONE launch, fill_plane_kernel, one workgroup per image, the whole pyramid in LDS.
//   larger:                            THREE launches
//     fill_pull_kernel   one workgroup per aligned 64 x 64 tile: levels 1 .. 6 of the tile in LDS, each level's in-plane cells
//                        to the workspace (tiles are aligned to 2^6: a cell of levels 1 .. 6 has exactly one tile)
//     fill_plane_kernel  on level 6 of the workspace (at most 64 x 64 cells, u16), in place: one workgroup per image pulls it
//                        to the top and pushes back down -- it reads the whole level into LDS before it writes any of it
//     fill_push_kernel   one workgroup per tile: F of level 6 at its cell and the neighbours and V of levels 5 .. 1 with a halo
//                        of one cell from the workspace in one sweep, the pushes in LDS, level 0 from the input to the output
// Nothing writes the workspace in the third launch and nothing reads the output, so out only must not be the input's buffer
// because the entry says so (a caller's filled plane next to its holey one).

#include "codon_common.h"
#include "fill_tile.h"
#include "kernels.h"

namespace codon {

// grid (B)
template <int FMT>
__global__ __launch_bounds__(FL_THREADS) void fill_plane_kernel(const void* in, long in_stride, void* out, long out_stride, int h,
                                                                int w, const float* __restrict__ tab, int top) {
  __shared__ unsigned short pyr[FL_PYR_CELLS];
  wg_fill_plane<FMT>(WgDevice(), blockIdx.x, in, in_stride, out, out_stride, h, w, tab, top, pyr);
}

// grid (gx, gy, B) of fl_plan
template <int FMT>
__global__ __launch_bounds__(FL_THREADS) void fill_pull_kernel(const void* __restrict__ in, int h, int w, int top,
                                                               unsigned short* __restrict__ ws, long ws_stride) {
  __shared__ unsigned short pyr[FL_PYR_CELLS];
  wg_fill_pull<FMT>(WgDevice(), blockIdx.x, blockIdx.y, blockIdx.z, in, h, w, top, ws, ws_stride, pyr);
}

// grid (gx, gy, B) of fl_plan
template <int FMT>
__global__ __launch_bounds__(FL_THREADS) void fill_push_kernel(const void* __restrict__ in, void* __restrict__ out, int h, int w,
                                                               const float* __restrict__ tab, int top,
                                                               const unsigned short* __restrict__ ws, long ws_stride) {
  __shared__ unsigned short hp[FL_HALO_CELLS];
  wg_fill_push<FMT>(WgDevice(), blockIdx.x, blockIdx.y, blockIdx.z, in, out, h, w, tab, top, ws, ws_stride, hp);
}

template <int FMT>
static int fill_launch(int B, int h, int w, const void* in, const float* tab, int top, void* out, unsigned short* ws,
                       hipStream_t stream) {
  const FlPlan p = fl_plan(h, w);
  if (p.single) {
    hipLaunchKernelGGL(fill_plane_kernel<FMT>, dim3((unsigned)B), dim3(FL_THREADS), 0, stream, in, (long)h * w, out, (long)h * w,
                       h, w, tab, top);
    return check_launch("fill_plane_kernel");
  }
  const dim3 grid((unsigned)p.gx, (unsigned)p.gy, (unsigned)B);
  hipLaunchKernelGGL(fill_pull_kernel<FMT>, grid, dim3(FL_THREADS), 0, stream, in, h, w, top, ws, p.stride);
  int st = check_launch("fill_pull_kernel");
  if (st != CODON_OK) return st;
  unsigned short* l6 = ws + p.l6;
  hipLaunchKernelGGL(fill_plane_kernel<FL_U16>, dim3((unsigned)B), dim3(FL_THREADS), 0, stream, (const void*)l6, p.stride,
                     (void*)l6, p.stride, p.h6, p.w6, (const float*)nullptr, 65535);
  st = check_launch("fill_plane_kernel");
  if (st != CODON_OK) return st;
  hipLaunchKernelGGL(fill_push_kernel<FMT>, grid, dim3(FL_THREADS), 0, stream, in, out, h, w, tab, top,
                     (const unsigned short*)ws, p.stride);
  return check_launch("fill_push_kernel");
}

size_t fill_holes_workspace_bytes(int h, int w) {
  if (h < 1 || h > FL_MAX_SIDE || w < 1 || w > FL_MAX_SIDE) return 0;
  return sizeof(unsigned short) * (size_t)fl_plan(h, w).stride;
}

int fill_holes(int B, int h, int w, const void* in, int fmt, const float* tab, int top, void* out, void* workspace,
               hipStream_t stream) {
  unsigned short* ws = (unsigned short*)workspace;
  if (fmt == FL_U8) return fill_launch<FL_U8>(B, h, w, in, tab, top, out, ws, stream);
  if (fmt == FL_U16) return fill_launch<FL_U16>(B, h, w, in, tab, top, out, ws, stream);
  return fill_launch<FL_F32>(B, h, w, in, tab, top, out, ws, stream);
}

}  // namespace codon
