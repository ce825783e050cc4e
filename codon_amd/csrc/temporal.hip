// The temporal filter of a fixed camera's depth sequence (codon_amd.temporal): every pixel's code is replaced by the
// rounded mean of the samples of its window of frames that are linked to it (range noise), a sample with too few such partners is
// rejected (a one-frame spike), and a hole or a rejected sample takes the consensus around the window's lower median where enough
// of the window is valid (flicker).  A DEFINITION of this project, in integers, restated in numpy in tests/temporal_ref.py; the
// kernel is held to its bits.  u8 and u16 codes; the workgroup body and its phases are in temporal_tile.h, and the host-side
// sanitizer check calls the same body.
//
// TWO launches, a function of (T, h, w, back, ahead) and of that alone -- not of the statistics pointer; no workspace, no wait on
// another workgroup, no host synchronisation:
//   temporal_zero_kernel       the (T, 4) statistics to 0 (nothing where there are none): clean's wg_clean_zero
//   temporal_kernel            per 1024 pixels and time chunk (launch_rules.h): a thread walks four pixels through the chunk's
//                              frames with the last 16 frames in an LDS ring (32 KiB), every frame read once and written once

#include "codon_common.h"
#include "kernels.h"
#include "launch_rules.h"
#include "temporal_tile.h"

namespace codon {

static_assert(TEMPORAL_TILE == TP_TILE, "launch_rules.h counts the workgroups of temporal_tile.h's tile");

// grid (1)
__global__ __launch_bounds__(TP_THREADS) void temporal_zero_kernel(unsigned* __restrict__ stats, int nstats) {
  wg_clean_zero(WgDevice(), stats, nstats);
}

// grid (ceil(h w / TP_TILE), ceil(T / a.chunk))
template <int FMT, int CAP>
__global__ __launch_bounds__(TP_THREADS) void temporal_kernel(const void* __restrict__ in, TpArgs a, void* __restrict__ out,
                                                              unsigned* __restrict__ stats) {
  __shared__ tp_quad ring[TP_SLOTS * TP_THREADS];
  __shared__ unsigned cnt[2 * TP_THREADS];
  __shared__ unsigned part[32];
  wg_temporal<FMT, CAP>(WgDevice(), (long)blockIdx.x, (int)blockIdx.y, in, a, out, stats, ring, cnt, part);
}

template <int FMT, int CAP>
static int temporal_launch(const void* in, const TpArgs& a, void* out, unsigned* stats, hipStream_t stream) {
  const long hw = (long)a.h * a.w;
  const dim3 grid((unsigned)((hw + TP_TILE - 1) / TP_TILE), (unsigned)((a.T + a.chunk - 1) / a.chunk)), threads(TP_THREADS);
  hipLaunchKernelGGL(temporal_zero_kernel, dim3(1), threads, 0, stream, stats, a.T * TP_STATS);
  const int st = check_launch("temporal_zero_kernel");
  if (st != CODON_OK) return st;
  hipLaunchKernelGGL((temporal_kernel<FMT, CAP>), grid, threads, 0, stream, in, a, out, stats);
  return check_launch("temporal_kernel");
}

template <int FMT>
static int temporal_caps(const void* in, const TpArgs& a, void* out, unsigned* stats, hipStream_t stream) {
  switch (temporal_cap(a.back, a.ahead)) {
    case 3: return temporal_launch<FMT, 3>(in, a, out, stats, stream);
    case 5: return temporal_launch<FMT, 5>(in, a, out, stats, stream);
    case 9: return temporal_launch<FMT, 9>(in, a, out, stats, stream);
    default: return temporal_launch<FMT, TP_MAX_WINDOW>(in, a, out, stats, stream);
  }
}

int temporal_depth(int T, int h, int w, const void* in, int fmt, int back, int ahead, int tol_abs, int tol_rel_q16, int min_count,
                   int min_fill, void* out, void* stats, hipStream_t stream) {
  TpArgs a;
  a.T = T, a.h = h, a.w = w, a.back = back, a.ahead = ahead;
  a.tol_abs = (unsigned)tol_abs, a.tol_rel = (unsigned)tol_rel_q16, a.min_count = min_count, a.min_fill = min_fill;
  a.chunk = temporal_chunk_frames(T, h, w, back, ahead);
  const uintptr_t quad = (uintptr_t)(TP_PER * fl_elem_bytes(fmt)) - 1;
  a.vec = ((long)h * w) % TP_PER == 0 && (((uintptr_t)in | (uintptr_t)out) & quad) == 0;
  return fmt == FL_U8 ? temporal_caps<FL_U8>(in, a, out, (unsigned*)stats, stream)
                      : temporal_caps<FL_U16>(in, a, out, (unsigned*)stats, stream);
}

}  // namespace codon
