// Spatial, edge-preserving smoothing of a depth sensor's maps (codon_amd.smooth): every valid code becomes the
// weighted mean, rounded, of the codes of its (2R+1)^2 window that are linked to it under clean's rule -- and, with the pair rule,
// whose point mirror through the centre is linked too, which makes the mean exact on any plane however the window is cut.  A
// DEFINITION of this project, in integers, restated in numpy in tests/smooth_ref.py; the kernel is held to its bits.  u8 and u16
// codes; the workgroup body and its phases are in smooth_tile.h, and the host-side sanitizer check calls the same body (DESIGN
// 12.13).
//
// 1 + smooth_launches(R, P) launches (launch_rules.h), a function of (R, P) and of that alone -- not of the statistics pointer; no
// wait on another workgroup, no host synchronisation:
//   smooth_zero_kernel    the (B, 4) statistics to 0 (nothing where there are none): clean's wg_clean_zero
//   smooth_kernel<R>      per 32 x 32 tile of one image: up to smooth_fused(R, P) passes between two LDS planes of 16-bit cells
//                         (5776 bytes at radius 1 .. 12544 at radius 4, and 3264 of counts), the last of them to global memory;
//                         the radius is a template argument, so that the window unrolls and every tap is a constant offset
// With more than one smooth_kernel launch the planes between them go through the caller's workspace (one plane set) and `out` in
// turn, the last launch writing `out`.

#include "codon_common.h"
#include "kernels.h"
#include "launch_rules.h"
#include "smooth_tile.h"

namespace codon {

static_assert(SMOOTH_TILE == SM_TILE, "launch_rules.h states the tile of smooth_tile.h");
static_assert(SMOOTH_MAX_RADIUS == SM_MAX_RADIUS && SMOOTH_MAX_PASSES == SM_MAX_PASSES, "launch_rules.h states smooth_tile.h's limits");

// grid (1)
__global__ __launch_bounds__(SM_THREADS) void smooth_zero_kernel(unsigned* __restrict__ stats, int nstats) {
  wg_clean_zero(WgDevice(), stats, nstats);
}

// grid (ceil(w / SM_TILE), ceil(h / SM_TILE), B)
template <int FMT, int R>
__global__ __launch_bounds__(SM_THREADS) void smooth_kernel(const void* __restrict__ in, const void* __restrict__ orig, SmArgs a,
                                                            const int* __restrict__ wtab, void* __restrict__ out,
                                                            unsigned* __restrict__ stats) {
  __shared__ unsigned short pa[sm_stride<R>() * sm_stride<R>()];
  __shared__ unsigned short pb[sm_stride<R>() * sm_stride<R>()];
  __shared__ unsigned cnt[2 * SM_THREADS];
  __shared__ unsigned part[32];
  __shared__ unsigned mx[SM_THREADS];
  __shared__ unsigned pmx[16];
  wg_smooth<FMT, R>(WgDevice(), blockIdx.x, blockIdx.y, (long)blockIdx.z, in, orig, a, wtab, out, stats, pa, pb, cnt, part, mx, pmx);
}

template <int FMT, int R>
static int smooth_launch(int B, const void* in, SmArgs a, int passes, const int* wtab, void* out, unsigned* stats, void* ws,
                         hipStream_t stream) {
  const dim3 tiles((unsigned)((a.w + SM_TILE - 1) / SM_TILE), (unsigned)((a.h + SM_TILE - 1) / SM_TILE), (unsigned)B), threads(SM_THREADS);
  hipLaunchKernelGGL(smooth_zero_kernel, dim3(1), threads, 0, stream, stats, B * SM_STATS);
  int st = check_launch("smooth_zero_kernel");
  const int fused = smooth_fused(a.radius, passes), launches = smooth_launches(a.radius, passes);
  const void* src = in;
  for (int i = 0, done = 0; i < launches && st == CODON_OK; ++i) {
    void* dst = (launches - 1 - i) % 2 == 0 ? out : ws;              // the last launch writes `out`
    a.fused = passes - done < fused ? passes - done : fused;
    a.first = i == 0, a.last = i == launches - 1;
    hipLaunchKernelGGL((smooth_kernel<FMT, R>), tiles, threads, 0, stream, src, in, a, wtab, dst, stats);
    st = check_launch("smooth_kernel");
    done += a.fused;
    src = dst;
  }
  return st;
}

template <int FMT>
static int smooth_radii(int B, const void* in, const SmArgs& a, int passes, const int* wtab, void* out, unsigned* stats, void* ws,
                        hipStream_t stream) {
  switch (a.radius) {
    case 1: return smooth_launch<FMT, 1>(B, in, a, passes, wtab, out, stats, ws, stream);
    case 2: return smooth_launch<FMT, 2>(B, in, a, passes, wtab, out, stats, ws, stream);
    case 3: return smooth_launch<FMT, 3>(B, in, a, passes, wtab, out, stats, ws, stream);
    default: return smooth_launch<FMT, 4>(B, in, a, passes, wtab, out, stats, ws, stream);
  }
}

size_t smooth_workspace_bytes(int B, int h, int w) {
  if (B < 1 || B > 65535 || h < 1 || h > SM_MAX_SIDE || w < 1 || w > SM_MAX_SIDE) return 0;
  return ((size_t)B * h * w * sizeof(unsigned short) + 15) / 16 * 16;
}

int smooth_depth(int B, int h, int w, const void* in, int fmt, int radius, int passes, int tol_abs, int tol_rel_q16, int pairs,
                 const void* weights, void* out, void* stats, void* workspace, hipStream_t stream) {
  SmArgs a;
  a.h = h, a.w = w, a.radius = radius, a.pairs = pairs != 0, a.tol_abs = (unsigned)tol_abs, a.tol_rel = (unsigned)tol_rel_q16;
  a.fused = 1, a.first = a.last = 1;
  return fmt == FL_U8 ? smooth_radii<FL_U8>(B, in, a, passes, (const int*)weights, out, (unsigned*)stats, workspace, stream)
                      : smooth_radii<FL_U16>(B, in, a, passes, (const int*)weights, out, (unsigned*)stats, workspace, stream);
}

}  // namespace codon
