// Guidance-aware (joint) pull-push hole filling of low-resolution code planes (DESIGN 12.11;
// codon_amd.upsample.fill_holes_guided): the plain filler's pyramid and parents (fill_holes.hip), but a hole weighs
// each parent by a range table of the difference between its own guidance and the guidance attached to that parent, so that a
// hole beside an occlusion edge is filled from its own side.  A DEFINITION of this project, in integers, restated in numpy in
// tests/guided_fill_ref.py; the kernels are held to its bits.  u8 and u16 codes; the per-thread bodies are in
// fill_guided_tile.h, shared with the host-side sanitizer check.
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

// grid (B).  in / out: image b at + b * stride elements; they may be the same buffer (level 6 of the workspace).  guide != null:
// G_0 from image b of the guidance; else A^ and G of the plane from a0 / g0 (image b at + b * ag_stride bytes)
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
  const int tid = threadIdx.x;
  const long b = blockIdx.x;
  const int K = fl_top_level(h, w);                                // uniform, <= FL_LOG
  fg_tab_load(tid, tab, t);
  fl_tile_load<FMT>(tid, (const char*)in + b * in_stride * fl_elem_bytes(FMT), h, w, 0, 0, top, v);
  if (guide) {
    const unsigned char* gimg = guide + b * image_bytes;
    if (scale == 4) fg_g0_tile<4>(tid, gimg, row_bytes, h, w, 0, 0, g, a, nullptr);
    else if (scale == 8) fg_g0_tile<8>(tid, gimg, row_bytes, h, w, 0, 0, g, a, nullptr);
    else fg_g0_tile<16>(tid, gimg, row_bytes, h, w, 0, 0, g, a, nullptr);
  } else {
    fg_plane_load8(tid, a0 + b * ag_stride, g0 + b * ag_stride, h, w, a, g);
  }
  __syncthreads();
  for (int k = 0; k < K; ++k) {
    fg_pull(tid, k, v, a, g, h, w, 0, 0, nullptr, nullptr, nullptr);
    __syncthreads();
  }
  for (int k = K - 1; k >= 0; --k) {
    fg_push(tid, k, h, w, v, a, g, t);
    __syncthreads();
  }
  fl_tile_store<FMT>(tid, (char*)out + b * out_stride * fl_elem_bytes(FMT), h, w, nullptr, v);
}

// grid (ceil(w/64), ceil(h/64), B).  ws: image b at + b * ws_stride bytes
template <int FMT>
__global__ __launch_bounds__(FL_THREADS) void fillg_pull_kernel(const void* __restrict__ in, int h, int w, int top,
                                                                const unsigned char* __restrict__ guide, long row_bytes,
                                                                long image_bytes, int scale, unsigned char* __restrict__ ws,
                                                                long ws_stride) {
  __shared__ unsigned short v[FL_PYR_CELLS];
  __shared__ unsigned char a[FL_PYR_CELLS];
  __shared__ unsigned char g[FL_PYR_CELLS];
  const int tid = threadIdx.x, tx = blockIdx.x, ty = blockIdx.y;
  const long b = blockIdx.z;
  const long cells = fl_workspace_cells(h, w);
  unsigned char* img = ws + b * ws_stride;
  const unsigned char* gimg = guide + b * image_bytes;
  fl_tile_load<FMT>(tid, (const char*)in + b * h * w * fl_elem_bytes(FMT), h, w, ty * FL_TILE, tx * FL_TILE, top, v);
  if (scale == 4) fg_g0_tile<4>(tid, gimg, row_bytes, h, w, ty * FL_TILE, tx * FL_TILE, g, a, img + 4 * cells);
  else if (scale == 8) fg_g0_tile<8>(tid, gimg, row_bytes, h, w, ty * FL_TILE, tx * FL_TILE, g, a, img + 4 * cells);
  else fg_g0_tile<16>(tid, gimg, row_bytes, h, w, ty * FL_TILE, tx * FL_TILE, g, a, img + 4 * cells);
  __syncthreads();
  long at = 0;                                                      // level k + 1 of this image, in cells
  for (int k = 0; k < FL_LOG; ++k) {
    fg_pull(tid, k, v, a, g, h, w, ty, tx, (unsigned short*)img + at, img + 2 * cells + at, img + 3 * cells + at);
    at += (long)fl_size(h, k + 1) * fl_size(w, k + 1);
    __syncthreads();
  }
}

// grid (ceil(w/64), ceil(h/64), B)
template <int FMT>
__global__ __launch_bounds__(FL_THREADS) void fillg_push_kernel(const void* __restrict__ in, void* __restrict__ out, int h, int w,
                                                                int top, const unsigned short* __restrict__ tab,
                                                                const unsigned char* __restrict__ ws, long ws_stride) {
  __shared__ unsigned short hv[FL_HALO_CELLS];
  __shared__ unsigned char ha[FL_HALO_CELLS];
  __shared__ unsigned char hg[FL_HALO_CELLS];
  __shared__ unsigned short t[FG_TAB];
  const int tid = threadIdx.x, tx = blockIdx.x, ty = blockIdx.y;
  const long b = blockIdx.z;
  const long at = b * h * w * fl_elem_bytes(FMT);
  const long cells = fl_workspace_cells(h, w);
  const unsigned char* img = ws + b * ws_stride;
  int v0[FL_PER_THREAD], g0[FL_PER_THREAD];
  fg_tab_load(tid, tab, t);
  fl_halo_load(tid, h, w, ty, tx, (const unsigned short*)img, hv);
  fg_halo_load8(tid, h, w, ty, tx, img + 2 * cells, ha);
  fg_halo_load8(tid, h, w, ty, tx, img + 3 * cells, hg);
  fl_halo_in<FMT>(tid, h, w, ty, tx, (const char*)in + at, top, v0);
  fg_halo_g0(tid, h, w, ty, tx, img + 4 * cells, g0);
  __syncthreads();
  for (int k = FL_LOG - 1; k >= 1; --k) {
    fg_halo_push(tid, k, h, w, ty, tx, hv, ha, hg, t);
    __syncthreads();
  }
  fg_halo_out<FMT>(tid, h, w, ty, tx, v0, g0, hv, ha, t, (char*)out + at);
}

template <int FMT>
static int fillg_launch(int B, int h, int w, const void* in, int top, const unsigned char* guide, long row_bytes, long image_bytes,
                        int scale, const unsigned short* tab, void* out, unsigned char* ws, long ws_stride, hipStream_t stream) {
  const unsigned char* none = nullptr;
  if (h <= FL_TILE && w <= FL_TILE) {
    hipLaunchKernelGGL(fillg_plane_kernel<FMT>, dim3((unsigned)B), dim3(FL_THREADS), 0, stream, in, (long)h * w, out, (long)h * w,
                       h, w, top, guide, row_bytes, image_bytes, scale, none, none, 0L, tab);
    return check_launch("fillg_plane_kernel");
  }
  const dim3 grid((unsigned)((w + FL_TILE - 1) / FL_TILE), (unsigned)((h + FL_TILE - 1) / FL_TILE), (unsigned)B);
  hipLaunchKernelGGL(fillg_pull_kernel<FMT>, grid, dim3(FL_THREADS), 0, stream, in, h, w, top, guide, row_bytes, image_bytes, scale,
                     ws, ws_stride);
  int st = check_launch("fillg_pull_kernel");
  if (st != CODON_OK) return st;
  const long cells = fl_workspace_cells(h, w), l6 = fl_level_offset(h, w, FL_LOG);
  unsigned short* v6 = (unsigned short*)ws + l6;
  hipLaunchKernelGGL(fillg_plane_kernel<FL_U16>, dim3((unsigned)B), dim3(FL_THREADS), 0, stream, (const void*)v6, ws_stride / 2,
                     (void*)v6, ws_stride / 2, fl_size(h, FL_LOG), fl_size(w, FL_LOG), 65535, none, 0L, 0L, scale,
                     (const unsigned char*)ws + 2 * cells + l6, (const unsigned char*)ws + 3 * cells + l6, ws_stride, tab);
  st = check_launch("fillg_plane_kernel");
  if (st != CODON_OK) return st;
  hipLaunchKernelGGL(fillg_push_kernel<FMT>, grid, dim3(FL_THREADS), 0, stream, in, out, h, w, top, tab, (const unsigned char*)ws,
                     ws_stride);
  return check_launch("fillg_push_kernel");
}

size_t fill_guided_workspace_bytes(int h, int w) {
  if (h < 1 || h > FL_MAX_SIDE || w < 1 || w > FL_MAX_SIDE) return 0;
  return ((size_t)fg_workspace_bytes(h, w) + 15) / 16 * 16;        // never 0 for a shape that is taken; images 16 bytes apart
}

int fill_holes_guided(int B, int h, int w, const void* in, int fmt, int top, const void* guide, long row_bytes, long image_bytes,
                      int scale, const void* range_tab, void* out, void* workspace, hipStream_t stream) {
  const long ws_stride = (long)fill_guided_workspace_bytes(h, w);
  if (fmt == FL_U8)
    return fillg_launch<FL_U8>(B, h, w, in, top, (const unsigned char*)guide, row_bytes, image_bytes, scale,
                               (const unsigned short*)range_tab, out, (unsigned char*)workspace, ws_stride, stream);
  return fillg_launch<FL_U16>(B, h, w, in, top, (const unsigned char*)guide, row_bytes, image_bytes, scale,
                              (const unsigned short*)range_tab, out, (unsigned char*)workspace, ws_stride, stream);
}

}  // namespace codon
