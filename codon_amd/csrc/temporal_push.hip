// The temporal filter of a fixed camera's depth stream, one frame per call (codon_amd.temporal.TemporalStream): the
// definition of temporal.hip with the window resident in device memory -- a ring of 16 planes and two counter words the caller
// owns -- so that a live stream, or a recording of any length, goes through frame by frame: frame t comes out with the push of
// frame t + ahead, the last `ahead` frames with flush steps.  Held to the bits of tests/temporal_ref.py on the whole sequence.
// The workgroup bodies are in temporal_tile.h, the per-quad arithmetic is the sequence kernel's own text (tp_filter4), and the
// host-side sanitizer check calls the same bodies.
//
// TWO launches per step, a function of (h, w, back, ahead, format, in null or not) and of that alone -- not of the frame index,
// which lives on the device, and not of the statistics pointer; no workspace, no wait on another workgroup, no host
// synchronisation:
//   temporal_push_begin_kernel   one workgroup: pushed += 1 and flushed = 0 (a push), or flushed += 1 (a flush); the statistics
//                                row to 0 -- an atomic add never shares a launch with the store that zeroes its word
//   temporal_push_kernel         per 1024 pixels (launch_rules.h): the new frame into its slot, the window gathered into
//                                registers, the final frame to `out`, its four counts added to the row

#include "codon_common.h"
#include "kernels.h"
#include "launch_rules.h"
#include "temporal_tile.h"

namespace codon {

static_assert(TEMPORAL_TILE == TP_TILE, "launch_rules.h counts the workgroups of temporal_tile.h's tile");

// grid (1)
__global__ __launch_bounds__(TP_THREADS) void temporal_push_begin_kernel(int push, unsigned* __restrict__ state,
                                                                         unsigned* __restrict__ stats) {
  wg_temporal_push_begin(WgDevice(), push, state, stats);
}

// grid (ceil(h w / TP_TILE)).  in, ring and out do not overlap (the entry refuses it)
template <int FMT, int CAP>
__global__ __launch_bounds__(TP_THREADS) void temporal_push_kernel(const void* __restrict__ in, TpArgs a, void* __restrict__ ring,
                                                                   const unsigned* __restrict__ state, void* __restrict__ out,
                                                                   unsigned* __restrict__ stats) {
  __shared__ unsigned cnt[2 * TP_THREADS];
  __shared__ unsigned part[32];
  wg_temporal_push<FMT, CAP>(WgDevice(), (long)blockIdx.x, in, a, ring, state, out, stats, cnt, part);
}

template <int FMT, int CAP>
static int temporal_push_launch(const void* in, const TpArgs& a, void* ring, unsigned* state, void* out, unsigned* stats,
                                hipStream_t stream) {
  const dim3 grid((unsigned)temporal_push_groups(a.h, a.w)), threads(TP_THREADS);
  hipLaunchKernelGGL(temporal_push_begin_kernel, dim3(1), threads, 0, stream, in ? 1 : 0, state, stats);
  const int st = check_launch("temporal_push_begin_kernel");
  if (st != CODON_OK) return st;
  hipLaunchKernelGGL((temporal_push_kernel<FMT, CAP>), grid, threads, 0, stream, in, a, ring, (const unsigned*)state, out, stats);
  return check_launch("temporal_push_kernel");
}

template <int FMT>
static int temporal_push_caps(const void* in, const TpArgs& a, void* ring, unsigned* state, void* out, unsigned* stats,
                              hipStream_t stream) {
  switch (temporal_cap(a.back, a.ahead)) {
    case 3: return temporal_push_launch<FMT, 3>(in, a, ring, state, out, stats, stream);
    case 5: return temporal_push_launch<FMT, 5>(in, a, ring, state, out, stats, stream);
    case 9: return temporal_push_launch<FMT, 9>(in, a, ring, state, out, stats, stream);
    default: return temporal_push_launch<FMT, TP_MAX_WINDOW>(in, a, ring, state, out, stats, stream);
  }
}

int temporal_push(int h, int w, const void* in, int fmt, int back, int ahead, int tol_abs, int tol_rel_q16, int min_count,
                  int min_fill, void* ring, void* state, void* out, void* stats, hipStream_t stream) {
  TpArgs a;
  a.T = 0, a.h = h, a.w = w, a.back = back, a.ahead = ahead;
  a.tol_abs = (unsigned)tol_abs, a.tol_rel = (unsigned)tol_rel_q16, a.min_count = min_count, a.min_fill = min_fill;
  a.chunk = 0;
  const uintptr_t quad = (uintptr_t)(TP_PER * fl_elem_bytes(fmt)) - 1;
  a.vec = ((long)h * w) % TP_PER == 0 && (((uintptr_t)in | (uintptr_t)out | (uintptr_t)ring) & quad) == 0;
  return fmt == FL_U8 ? temporal_push_caps<FL_U8>(in, a, ring, (unsigned*)state, out, (unsigned*)stats, stream)
                      : temporal_push_caps<FL_U16>(in, a, ring, (unsigned*)state, out, (unsigned*)stats, stream);
}

}  // namespace codon
