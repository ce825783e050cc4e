// Outlier rejection of a depth sensor's maps (codon_amd.clean): flying pixels, by the support a pixel has among its
// 8 neighbours, and speckles, by the size of its connected component -- labelled by a lock-free union-find on a u32 plane.  A
// DEFINITION of this project, in integers, restated in numpy in tests/clean_ref.py; the kernels are held to its bits -- counts
// and component sizes do not depend on the order of the threads.  u8 and u16 codes; the launch plan, the workgroup bodies and
// their phases are in clean_tile.h, and the host-side sanitizer check calls the same bodies.
//
// TWO launches with rule 2 off, FOUR with it on, a function of (B, h, w) and of that alone; no flag, no wait on another workgroup,
// no host synchronisation; every loop of the union-find carries its trip limit:
//   clean_zero_kernel     (rule 2 off) the statistics to 0
//   clean_flying_kernel   per 16 x 16 tile: the tile and a halo of 1 in LDS (1296 bytes, and 2176 of counts); rule 1 -> out, the
//                         tile's own links united in LDS (2048 bytes), the label words to the tile-local roots, the size words to 0
//   clean_link_kernel     per tile: its last column and row with the next tile's, 32-bit atomic minima that return the old word
//   clean_count_kernel    per tile: roots written back, the row runs of a root (1024 bytes of LDS) added to its size word
//   clean_apply_kernel    per 1024 pixels: rule 2 -> out in place, and the four counts

#include "codon_common.h"
#include "kernels.h"
#include "clean_tile.h"

namespace codon {

// grid (1)
__global__ __launch_bounds__(CL_THREADS) void clean_zero_kernel(unsigned* __restrict__ stats, int nstats) {
  wg_clean_zero(WgDevice(), stats, nstats);
}

// grid (sx, sy, B) of cl_plan
template <int FMT>
__global__ __launch_bounds__(CL_THREADS) void clean_flying_kernel(const void* __restrict__ in, ClArgs a, int B, void* __restrict__ out,
                                                                  unsigned* __restrict__ ws, unsigned* __restrict__ stats) {
  __shared__ unsigned cell[CL_CELLS];
  __shared__ unsigned cnt[2 * CL_THREADS];
  __shared__ unsigned part[32];
  __shared__ unsigned kk[CL_THREADS];
  __shared__ unsigned loc[CL_THREADS];
  wg_clean_flying<FMT>(WgDevice(), blockIdx.x, blockIdx.y, (long)blockIdx.z, B, in, a, out, ws, stats, cell, cnt, part, kk, loc);
}

// grid (sx, sy, B) of cl_plan
template <int FMT>
__global__ __launch_bounds__(CL_THREADS) void clean_link_kernel(const void* __restrict__ out, ClArgs a, unsigned* ws) {
  wg_clean_link<FMT>(WgDevice(), blockIdx.x, blockIdx.y, (long)blockIdx.z, out, a, ws);
}

// grid (sx, sy, B) of cl_plan
__global__ __launch_bounds__(CL_THREADS) void clean_count_kernel(ClArgs a, int B, unsigned* ws) {
  __shared__ unsigned root[CL_THREADS];
  wg_clean_count(WgDevice(), blockIdx.x, blockIdx.y, (long)blockIdx.z, B, a, ws, root);
}

// grid (rx, B) of cl_plan
template <int FMT>
__global__ __launch_bounds__(CL_THREADS) void clean_apply_kernel(const void* __restrict__ in, ClArgs a, int B, void* __restrict__ out,
                                                                 const unsigned* __restrict__ ws, unsigned* __restrict__ stats) {
  __shared__ unsigned cnt[2 * CL_THREADS];
  __shared__ unsigned part[32];
  wg_clean_apply<FMT>(WgDevice(), (long)blockIdx.x, (long)blockIdx.y, B, in, a, out, ws, stats, cnt, part);
}

template <int FMT>
static int clean_launch(int B, const void* in, const ClArgs& a, void* out, unsigned* stats, unsigned* ws, hipStream_t stream) {
  const ClPlan p = cl_plan(a.h, a.w, a.region);
  const dim3 tiles((unsigned)p.sx, (unsigned)p.sy, (unsigned)B), threads(CL_THREADS);
  int st;
  if (!p.rule2) {
    hipLaunchKernelGGL(clean_zero_kernel, dim3(1), threads, 0, stream, stats, B * CL_STATS);
    st = check_launch("clean_zero_kernel");
    if (st != CODON_OK) return st;
  }
  hipLaunchKernelGGL((clean_flying_kernel<FMT>), tiles, threads, 0, stream, in, a, B, out, ws, stats);
  st = check_launch("clean_flying_kernel");
  if (st != CODON_OK || !p.rule2) return st;
  hipLaunchKernelGGL((clean_link_kernel<FMT>), tiles, threads, 0, stream, (const void*)out, a, ws);
  st = check_launch("clean_link_kernel");
  if (st != CODON_OK) return st;
  hipLaunchKernelGGL(clean_count_kernel, tiles, threads, 0, stream, a, B, ws);
  st = check_launch("clean_count_kernel");
  if (st != CODON_OK) return st;
  hipLaunchKernelGGL((clean_apply_kernel<FMT>), dim3((unsigned)p.rx, (unsigned)B), threads, 0, stream, in, a, B, out,
                     (const unsigned*)ws, stats);
  return check_launch("clean_apply_kernel");
}

size_t clean_workspace_bytes(int B, int h, int w) {
  if (B < 1 || B > 65535 || h < 1 || h > CL_MAX_SIDE || w < 1 || w > CL_MAX_SIDE) return 0;
  return (size_t)cl_workspace_words(B, h, w) * sizeof(unsigned);
}

int clean_depth(int B, int h, int w, const void* in, int fmt, int tol_abs, int tol_rel_q16, int min_support, int min_region, void* out,
                void* stats, void* workspace, hipStream_t stream) {
  ClArgs a;
  a.h = h, a.w = w, a.tol_abs = (unsigned)tol_abs, a.tol_rel = (unsigned)tol_rel_q16, a.support = min_support, a.region = min_region;
  return fmt == FL_U8 ? clean_launch<FL_U8>(B, in, a, out, (unsigned*)stats, (unsigned*)workspace, stream)
                      : clean_launch<FL_U16>(B, in, a, out, (unsigned*)stats, (unsigned*)workspace, stream);
}

}  // namespace codon
