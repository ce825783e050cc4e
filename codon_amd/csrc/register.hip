// Registration of a depth sensor's map to the colour camera (codon_amd.register): a z-buffered forward projection
// of every valid source pixel's four corners onto the colour camera's grid, the box of them splatted with an atomic minimum.  A
// DEFINITION of this project, in integers, restated in numpy in tests/register_ref.py; the kernels are held to its bits -- the
// minimum and the counts do not depend on the order of the threads.  u8 and u16 codes; the launch plan, the workgroup bodies and
// their phases are in register_tile.h, and the host-side sanitizer check calls the same bodies.
//
// THREE launches, a function of (B, hs, ws, ho, wo) alone; no flag, no wait on another workgroup, no host synchronisation:
//   register_init_kernel      the z-buffer planes (u32 per target pixel, the workspace) to all ones, the statistics to 0
//   register_splat_kernel     per 16 x 16 tile of source pixels: the tile's 17 x 17 x 3 corner rays in LDS (3468 bytes, and 1088 of
//                             counts), one pixel per thread, 32-bit vector atomic minima on global memory
//   register_resolve_kernel   per 1024 target pixels: z-buffer -> codes, all ones -> 0, and the filled count

#include "codon_common.h"
#include "kernels.h"
#include "register_tile.h"

namespace codon {

// grid (rg_init_runs)
__global__ __launch_bounds__(RG_THREADS) void register_init_kernel(unsigned* __restrict__ zb, long words, unsigned* __restrict__ stats,
                                                                   int nstats) {
  wg_register_init(WgDevice(), (long)blockIdx.x, zb, words, stats, nstats);
}

// grid (sx, sy, B) of rg_plan
template <int FMT>
__global__ __launch_bounds__(RG_THREADS) void register_splat_kernel(const void* __restrict__ in, const int* __restrict__ rays, RgArgs a,
                                                                    unsigned* __restrict__ zb, long zb_stride,
                                                                    unsigned* __restrict__ stats) {
  __shared__ int la[RG_CORNERS * 3];
  __shared__ unsigned cnt[RG_THREADS];
  __shared__ unsigned part[16];
  wg_register_splat<FMT>(WgDevice(), blockIdx.x, blockIdx.y, (long)blockIdx.z, in, rays, a, zb, zb_stride, stats, la, cnt, part);
}

// grid (rx, B) of rg_plan
template <int FMT>
__global__ __launch_bounds__(RG_THREADS) void register_resolve_kernel(const unsigned* __restrict__ zb, long zb_stride, int ho, int wo,
                                                                      void* __restrict__ out, unsigned* __restrict__ stats) {
  __shared__ unsigned cnt[RG_THREADS];
  __shared__ unsigned part[16];
  wg_register_resolve<FMT>(WgDevice(), (long)blockIdx.x, (long)blockIdx.y, zb, zb_stride, ho, wo, out, stats, cnt, part);
}

template <int FMT>
static int register_launch(int B, const void* in, const int* rays, const RgArgs& a, void* out, unsigned* stats, unsigned* zb,
                           hipStream_t stream) {
  const RgPlan p = rg_plan(a.hs, a.ws, a.ho, a.wo);
  hipLaunchKernelGGL(register_init_kernel, dim3((unsigned)rg_init_runs(p, B)), dim3(RG_THREADS), 0, stream, zb, p.stride * B, stats,
                     B * RG_STATS);
  int st = check_launch("register_init_kernel");
  if (st != CODON_OK) return st;
  hipLaunchKernelGGL((register_splat_kernel<FMT>), dim3((unsigned)p.sx, (unsigned)p.sy, (unsigned)B), dim3(RG_THREADS), 0, stream, in,
                     rays, a, zb, p.stride, stats);
  st = check_launch("register_splat_kernel");
  if (st != CODON_OK) return st;
  hipLaunchKernelGGL((register_resolve_kernel<FMT>), dim3((unsigned)p.rx, (unsigned)B), dim3(RG_THREADS), 0, stream,
                     (const unsigned*)zb, p.stride, a.ho, a.wo, out, stats);
  return check_launch("register_resolve_kernel");
}

size_t register_workspace_bytes(int ho, int wo) {
  if (ho < 1 || ho > RG_MAX_SIDE || wo < 1 || wo > RG_MAX_SIDE) return 0;
  return (size_t)rg_plan(1, 1, ho, wo).stride * sizeof(unsigned);
}

int register_depth(int B, int hs, int ws, const void* in, int fmt, int top, const void* rays, const long long* trans, const int* proj,
                   int ho, int wo, void* out, void* stats, void* workspace, hipStream_t stream) {
  RgArgs a;
  a.tx = trans[0], a.ty = trans[1], a.tz = trans[2];
  a.fx = proj[0], a.fy = proj[1], a.cx = proj[2], a.cy = proj[3];
  a.hs = hs, a.ws = ws, a.ho = ho, a.wo = wo, a.top = top;
  return fmt == FL_U8 ? register_launch<FL_U8>(B, in, (const int*)rays, a, out, (unsigned*)stats, (unsigned*)workspace, stream)
                      : register_launch<FL_U16>(B, in, (const int*)rays, a, out, (unsigned*)stats, (unsigned*)workspace, stream);
}

}  // namespace codon
