// Depth maps as coloured point clouds with normals (codon_amd.cloud): every non-zero code of a plane becomes a packed
// record -- position in metres, a unit normal from integer tangents, the colour -- in row-major order of the pixels: an ORDERED
// stream compaction, count, scan, scatter.  A DEFINITION of this project, restated in numpy in tests/cloud_ref.py; the kernels are
// held to its bytes.  u8 and u16 codes; the launch plan, the workgroup bodies and their phases are in cloud_tile.h, and the
// host-side sanitizer check calls the same bodies.
//
// THREE launches, a function of (B, h, w) and the record form alone; no atomic decides a position, no workgroup waits for another,
// no host synchronisation:
//   cloud_count_kernel   per 1024 consecutive pixels: the number of non-zero codes to the block's word (1088 bytes of LDS)
//   cloud_scan_kernel    per image: the exclusive scan of its block words in place, and counts[b] = (points, 0)
//   cloud_emit_kernel    per 1024 consecutive pixels: ranks through LDS, the records staged in LDS (up to 27652 bytes) and the
//                        block's one contiguous span stored in 4-byte words; the normal map; counts[b][1], one atomic add per block

#include "codon_common.h"
#include "kernels.h"
#include "cloud_tile.h"
#include "mesh_tile.h"

namespace codon {

// grid (blocks, B) of cd_plan
template <int FMT>
__global__ __launch_bounds__(CD_THREADS) void cloud_count_kernel(const void* __restrict__ in, int h, int w, unsigned* __restrict__ ws) {
  __shared__ unsigned cnt[CD_THREADS];
  __shared__ unsigned part[CD_PARTS];
  wg_cloud_count<FMT>(WgDevice(), (long)blockIdx.x, (long)blockIdx.y, in, h, w, ws, cnt, part);
}

// grid (B)
__global__ __launch_bounds__(CD_SCAN_THREADS) void cloud_scan_kernel(int h, int w, unsigned* __restrict__ ws,
                                                                     unsigned* __restrict__ counts) {
  __shared__ unsigned cnt[CD_SCAN_THREADS];
  __shared__ unsigned part[16];
  wg_cloud_scan(WgDevice(), (long)blockIdx.x, h, w, ws, counts, cnt, part);
}

// grid (blocks, B) of cd_plan
template <int FMT, int REC>
__global__ __launch_bounds__(CD_THREADS) void cloud_emit_kernel(const void* __restrict__ in, CdArgs a, const int* __restrict__ rx,
                                                                const int* __restrict__ ry, const unsigned char* __restrict__ color,
                                                                unsigned char* __restrict__ body, unsigned* __restrict__ counts,
                                                                unsigned char* __restrict__ nmap, const unsigned* __restrict__ ws) {
  __shared__ unsigned cnt[CD_THREADS];
  __shared__ unsigned ncnt[CD_THREADS];
  __shared__ unsigned part[CD_PARTS];
  __shared__ unsigned npart[CD_PARTS];
  __shared__ unsigned stage[cd_stage_words(REC)];
  wg_cloud_emit<FMT, REC>(WgDevice(), (long)blockIdx.x, (long)blockIdx.y, in, a, rx, ry, color, body, counts, nmap, ws, cnt, ncnt, part,
                          npart, stage);
}

template <int FMT, int REC>
static int cloud_emit(int B, const void* in, const CdArgs& a, const int* rx, const int* ry, const unsigned char* color,
                      unsigned char* body, unsigned* counts, unsigned char* nmap, const unsigned* ws, hipStream_t stream) {
  const CdPlan p = cd_plan(a.h, a.w);
  hipLaunchKernelGGL((cloud_emit_kernel<FMT, REC>), dim3((unsigned)p.blocks, (unsigned)B), dim3(CD_THREADS), 0, stream, in, a, rx, ry,
                     color, body, counts, nmap, ws);
  return check_launch("cloud_emit_kernel");
}

template <int FMT>
static int cloud_launch(int B, const void* in, const CdArgs& a, const int* rx, const int* ry, const unsigned char* color,
                        unsigned char* body, unsigned* counts, unsigned char* nmap, unsigned* ws, hipStream_t stream) {
  const CdPlan p = cd_plan(a.h, a.w);
  hipLaunchKernelGGL((cloud_count_kernel<FMT>), dim3((unsigned)p.blocks, (unsigned)B), dim3(CD_THREADS), 0, stream, in, a.h, a.w, ws);
  int st = check_launch("cloud_count_kernel");
  if (st != CODON_OK) return st;
  hipLaunchKernelGGL(cloud_scan_kernel, dim3((unsigned)B), dim3(CD_SCAN_THREADS), 0, stream, a.h, a.w, ws, counts);
  st = check_launch("cloud_scan_kernel");
  if (st != CODON_OK) return st;
  const bool normals = a.radius > 0;
  if (color)
    return normals ? cloud_emit<FMT, cd_rec(true, true)>(B, in, a, rx, ry, color, body, counts, nmap, ws, stream)
                   : cloud_emit<FMT, cd_rec(false, true)>(B, in, a, rx, ry, color, body, counts, nmap, ws, stream);
  return normals ? cloud_emit<FMT, cd_rec(true, false)>(B, in, a, rx, ry, color, body, counts, nmap, ws, stream)
                 : cloud_emit<FMT, cd_rec(false, false)>(B, in, a, rx, ry, color, body, counts, nmap, ws, stream);
}

size_t cloud_workspace_bytes(int B, int h, int w) {
  if (B < 1 || B > 65535 || h < 1 || h > CD_MAX_SIDE || w < 1 || w > CD_MAX_SIDE) return 0;
  return (size_t)cd_workspace_words(B, h, w) * sizeof(unsigned);
}

int cloud_points(int B, int h, int w, const void* in, int fmt, const int* rx, const int* ry, double m, int radius, int tol_abs,
                 int tol_rel_q16, const void* color, int channels, void* body, void* counts, void* nmap, void* workspace,
                 hipStream_t stream) {
  CdArgs a;
  a.h = h, a.w = w, a.radius = radius, a.tol_abs = (unsigned)(radius * tol_abs), a.tol_rel = (unsigned)tol_rel_q16;
  a.channels = channels, a.m = m;
  return fmt == FL_U8 ? cloud_launch<FL_U8>(B, in, a, rx, ry, (const unsigned char*)color, (unsigned char*)body, (unsigned*)counts,
                                            (unsigned char*)nmap, (unsigned*)workspace, stream)
                      : cloud_launch<FL_U16>(B, in, a, rx, ry, (const unsigned char*)color, (unsigned char*)body, (unsigned*)counts,
                                             (unsigned char*)nmap, (unsigned*)workspace, stream);
}

// ---- depth maps as triangle meshes (codon_amd.cloud.triangulate) ----------------------------------------------------
// The pixel quads of a code plane whose corners are linked become triangles over the cloud's own vertices, packed in row-major order
// of the quads: a second ordered compaction.  A DEFINITION, restated in numpy in tests/mesh_ref.py; the bodies are in mesh_tile.h.
// SIX launches, a function of (B, h, w) alone (one, the face scan, for a plane without a quad); no atomic decides a position, no
// workgroup waits for another, no host synchronisation:
//   cloud_count_kernel   as above: the non-zero codes of 1024 consecutive pixels to the block's word
//   cloud_scan_kernel    as above: the exclusive scan of an image's block words (its two counts go to the workspace)
//   mesh_index_kernel    per 1024 consecutive pixels: the rank of every non-zero code to the int32 index plane (1088 bytes of LDS)
//   mesh_count_kernel    per 1024 consecutive quads: the number of faces to the run's word (1088 bytes of LDS)
//   mesh_scan_kernel     per image: the scan body over the run words, and counts[b] = faces
//   mesh_emit_kernel     per 1024 consecutive quads: ranks through LDS, the 13-byte records staged in LDS (26 628 bytes) and the
//                        run's one contiguous span stored in 4-byte words

// grid (blocks, B) of cd_plan
template <int FMT>
__global__ __launch_bounds__(CD_THREADS) void mesh_index_kernel(const void* __restrict__ in, int h, int w,
                                                                const unsigned* __restrict__ ws, int* __restrict__ index) {
  __shared__ unsigned cnt[CD_THREADS];
  __shared__ unsigned part[CD_PARTS];
  wg_mesh_index<FMT>(WgDevice(), (long)blockIdx.x, (long)blockIdx.y, in, h, w, ws, index, cnt, part);
}

// grid (runs, B) of ms_plan
template <int FMT>
__global__ __launch_bounds__(MS_THREADS) void mesh_count_kernel(const void* __restrict__ in, MsArgs a, unsigned* __restrict__ runs) {
  __shared__ unsigned cnt[MS_THREADS];
  __shared__ unsigned part[MS_PARTS];
  wg_mesh_count<FMT>(WgDevice(), (long)blockIdx.x, (long)blockIdx.y, in, a, runs, cnt, part);
}

// grid (B)
__global__ __launch_bounds__(CD_SCAN_THREADS) void mesh_scan_kernel(int h, int w, unsigned* __restrict__ runs,
                                                                    unsigned* __restrict__ counts) {
  __shared__ unsigned cnt[CD_SCAN_THREADS];
  __shared__ unsigned part[16];
  wg_mesh_scan(WgDevice(), (long)blockIdx.x, h, w, runs, counts, cnt, part);
}

// grid (runs, B) of ms_plan
template <int FMT>
__global__ __launch_bounds__(MS_THREADS) void mesh_emit_kernel(const void* __restrict__ in, MsArgs a, const int* __restrict__ index,
                                                               const unsigned* __restrict__ runs, unsigned char* __restrict__ faces) {
  __shared__ unsigned cnt[MS_THREADS];
  __shared__ unsigned part[MS_PARTS];
  __shared__ unsigned stage[MS_STAGE_WORDS];
  wg_mesh_emit<FMT>(WgDevice(), (long)blockIdx.x, (long)blockIdx.y, in, a, index, runs, faces, cnt, part, stage);
}

template <int FMT>
static int mesh_launch(int B, const void* in, const MsArgs& a, unsigned char* faces, unsigned* counts, unsigned* ws,
                       hipStream_t stream) {
  const CdPlan c = cd_plan(a.h, a.w);
  const MsPlan p = ms_plan(a.h, a.w);
  const MsSpace s = ms_space(B, a.h, a.w);
  unsigned *blocks = ws + s.blocks, *runs = ws + s.runs, *points = ws + s.counts;
  int* index = (int*)(ws + s.index);
  int st = CODON_OK;
  if (p.runs > 0) {
    const dim3 pixels((unsigned)c.blocks, (unsigned)B), quads((unsigned)p.runs, (unsigned)B);
    hipLaunchKernelGGL((cloud_count_kernel<FMT>), pixels, dim3(CD_THREADS), 0, stream, in, a.h, a.w, blocks);
    if ((st = check_launch("cloud_count_kernel")) != CODON_OK) return st;
    hipLaunchKernelGGL(cloud_scan_kernel, dim3((unsigned)B), dim3(CD_SCAN_THREADS), 0, stream, a.h, a.w, blocks, points);
    if ((st = check_launch("cloud_scan_kernel")) != CODON_OK) return st;
    hipLaunchKernelGGL((mesh_index_kernel<FMT>), pixels, dim3(CD_THREADS), 0, stream, in, a.h, a.w, blocks, index);
    if ((st = check_launch("mesh_index_kernel")) != CODON_OK) return st;
    hipLaunchKernelGGL((mesh_count_kernel<FMT>), quads, dim3(MS_THREADS), 0, stream, in, a, runs);
    if ((st = check_launch("mesh_count_kernel")) != CODON_OK) return st;
  }
  hipLaunchKernelGGL(mesh_scan_kernel, dim3((unsigned)B), dim3(CD_SCAN_THREADS), 0, stream, a.h, a.w, runs, counts);
  if ((st = check_launch("mesh_scan_kernel")) != CODON_OK) return st;
  if (p.runs > 0) {
    hipLaunchKernelGGL((mesh_emit_kernel<FMT>), dim3((unsigned)p.runs, (unsigned)B), dim3(MS_THREADS), 0, stream, in, a, index, runs,
                       faces);
    st = check_launch("mesh_emit_kernel");
  }
  return st;
}

size_t cloud_mesh_workspace_bytes(int B, int h, int w) {
  if (B < 1 || B > 65535 || h < 1 || h > MS_MAX_SIDE || w < 1 || w > MS_MAX_SIDE) return 0;
  return (size_t)ms_space(B, h, w).words * sizeof(unsigned);
}

int cloud_mesh(int B, int h, int w, const void* in, int fmt, int tol_abs, int tol_rel_q16, void* faces, void* counts, void* workspace,
               hipStream_t stream) {
  MsArgs a;
  a.h = h, a.w = w, a.tol_abs = (unsigned)tol_abs, a.tol_rel = (unsigned)tol_rel_q16;
  return fmt == FL_U8 ? mesh_launch<FL_U8>(B, in, a, (unsigned char*)faces, (unsigned*)counts, (unsigned*)workspace, stream)
                      : mesh_launch<FL_U16>(B, in, a, (unsigned char*)faces, (unsigned*)counts, (unsigned*)workspace, stream);
}

}  // namespace codon
