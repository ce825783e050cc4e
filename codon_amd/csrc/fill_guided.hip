// Guidance-aware (joint) pull-push hole filling of low-resolution code planes (DESIGN 12.11;
// codon_amd.upsample.fill_holes_guided): the plain filler's pyramid and parents (fill_holes.hip), but a hole weighs
// each parent by a range table of the difference between its own guidance and the guidance attached to that parent, so that a
// hole beside an occlusion edge is filled from its own side.  A DEFINITION of this project, in integers, restated in numpy in
// tests/guided_fill_ref.py; the kernels are held to its bits.  u8 and u16 codes; the launch plan, the workgroup bodies and their
// phases are in fill_guided_tile.h, and the host-side sanitizer check calls the same bodies.
//
// The launch plan is the plain filler's and depends on (B, h, w, scale) alone; no atomics, no flag, no wait on another
// workgroup: levels pass between workgroups only across kernel boundaries.
//   h, w <= 64:  ONE launch, fillg_plane_kernel, one workgroup per image: V (u16), A^ and G (u8) pyramids and the table in LDS
//                (22 368 bytes), G_0 reduced from the high-resolution guidance straight into LDS.
//   larger:      THREE launches over the plain filler's aligned 64 x 64 tiles
//     fillg_pull_kernel   per tile: V_0 and G_0 of the tile into LDS -- G_0 also to the workspace, where the push launch reads it
//                         back (2 bytes of traffic per cell instead of s^2 more bytes of guidance) -- then levels 1 .. 6 of V,
//                         A^ and G, each level's in-plane cells to the workspace
//     fillg_plane_kernel  on level 6 of the workspace (at most 64 x 64 cells), V in place: one workgroup per image pulls the
//                         three pyramids to the top and pushes V back down; it reads the whole level before it writes any of it
//     fillg_push_kernel   per tile: F of level 6 and V of levels 5 .. 1 with a halo of one cell, the same halo pyramids of A^
//                         and G, the pushes in LDS, level 0 from the input and the workspace's G_0 to the output

#include "codon_common.h"
#include "fill_guided_tile.h"
#include "kernels.h"

namespace codon {

// grid (B)
template <int FMT>
__global__ __launch_bounds__(FL_THREADS) void fillg_plane_kernel(const void* in, long in_stride, void* out, long out_stride, int h,
                                                                 int w, int top, const unsigned char* __restrict__ guide,
                                                                 long row_bytes, long image_bytes, int scale,
                                                                 const unsigned char* __restrict__ a0,
                                                                 const unsigned char* __restrict__ g0, long ag_stride,
                                                                 const unsigned short* __restrict__ tab) {
  __shared__ unsigned short v[FL_PYR_CELLS];
  __shared__ unsigned char a[FL_PYR_CELLS];
  __shared__ unsigned char g[FL_PYR_CELLS];
  __shared__ unsigned short t[FG_TAB];
  wg_fillg_plane<FMT>(WgDevice(), blockIdx.x, in, in_stride, out, out_stride, h, w, top, guide, row_bytes, image_bytes, scale, a0,
                      g0, ag_stride, tab, v, a, g, t);
}

// grid (gx, gy, B) of fg_plan
template <int FMT>
__global__ __launch_bounds__(FL_THREADS) void fillg_pull_kernel(const void* __restrict__ in, int h, int w, int top,
                                                                const unsigned char* __restrict__ guide, long row_bytes,
                                                                long image_bytes, int scale, unsigned char* __restrict__ ws,
                                                                long ws_stride) {
  __shared__ unsigned short v[FL_PYR_CELLS];
  __shared__ unsigned char a[FL_PYR_CELLS];
  __shared__ unsigned char g[FL_PYR_CELLS];
  wg_fillg_pull<FMT>(WgDevice(), blockIdx.x, blockIdx.y, blockIdx.z, in, h, w, top, guide, row_bytes, image_bytes, scale, ws,
                     ws_stride, v, a, g);
}

// grid (gx, gy, B) of fg_plan
template <int FMT>
__global__ __launch_bounds__(FL_THREADS) void fillg_push_kernel(const void* __restrict__ in, void* __restrict__ out, int h, int w,
                                                                int top, const unsigned short* __restrict__ tab,
                                                                const unsigned char* __restrict__ ws, long ws_stride) {
  __shared__ unsigned short hv[FL_HALO_CELLS];
  __shared__ unsigned char ha[FL_HALO_CELLS];
  __shared__ unsigned char hg[FL_HALO_CELLS];
  __shared__ unsigned short t[FG_TAB];
  wg_fillg_push<FMT>(WgDevice(), blockIdx.x, blockIdx.y, blockIdx.z, in, out, h, w, top, tab, ws, ws_stride, hv, ha, hg, t);
}

template <int FMT>
static int fillg_launch(int B, int h, int w, const void* in, int top, const unsigned char* guide, long row_bytes, long image_bytes,
                        int scale, const unsigned short* tab, void* out, unsigned char* ws, hipStream_t stream) {
  const unsigned char* none = nullptr;
  const FgPlan p = fg_plan(h, w);
  if (p.single) {
    hipLaunchKernelGGL(fillg_plane_kernel<FMT>, dim3((unsigned)B), dim3(FL_THREADS), 0, stream, in, (long)h * w, out, (long)h * w,
                       h, w, top, guide, row_bytes, image_bytes, scale, none, none, 0L, tab);
    return check_launch("fillg_plane_kernel");
  }
  const dim3 grid((unsigned)p.gx, (unsigned)p.gy, (unsigned)B);
  hipLaunchKernelGGL(fillg_pull_kernel<FMT>, grid, dim3(FL_THREADS), 0, stream, in, h, w, top, guide, row_bytes, image_bytes, scale,
                     ws, p.stride);
  int st = check_launch("fillg_pull_kernel");
  if (st != CODON_OK) return st;
  hipLaunchKernelGGL(fillg_plane_kernel<FL_U16>, dim3((unsigned)B), dim3(FL_THREADS), 0, stream, (const void*)(ws + p.v6),
                     p.stride / 2, (void*)(ws + p.v6), p.stride / 2, p.h6, p.w6, 65535, none, 0L, 0L, scale,
                     (const unsigned char*)ws + p.a6, (const unsigned char*)ws + p.g6, p.stride, tab);
  st = check_launch("fillg_plane_kernel");
  if (st != CODON_OK) return st;
  hipLaunchKernelGGL(fillg_push_kernel<FMT>, grid, dim3(FL_THREADS), 0, stream, in, out, h, w, top, tab, (const unsigned char*)ws,
                     p.stride);
  return check_launch("fillg_push_kernel");
}

size_t fill_guided_workspace_bytes(int h, int w) {
  if (h < 1 || h > FL_MAX_SIDE || w < 1 || w > FL_MAX_SIDE) return 0;
  return (size_t)fg_plan(h, w).stride;
}

int fill_holes_guided(int B, int h, int w, const void* in, int fmt, int top, const void* guide, long row_bytes, long image_bytes,
                      int scale, const void* range_tab, void* out, void* workspace, hipStream_t stream) {
  if (fmt == FL_U8)
    return fillg_launch<FL_U8>(B, h, w, in, top, (const unsigned char*)guide, row_bytes, image_bytes, scale,
                               (const unsigned short*)range_tab, out, (unsigned char*)workspace, stream);
  return fillg_launch<FL_U16>(B, h, w, in, top, (const unsigned char*)guide, row_bytes, image_bytes, scale,
                              (const unsigned short*)range_tab, out, (unsigned char*)workspace, stream);
}

}  // namespace codon
