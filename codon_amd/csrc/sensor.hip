// The sensor model of the training degradation (codon_amd.train.synthesize(sensor=...)): range noise and
// dropout on the low-resolution map between the down and the up launch, so that a network fine-tuned on clean HR depth meets
// what `infer --lr-depth` will feed it from a sensor's file.  The reference ships no degradation at all, so this is a
// DEFINITION, restated in numpy in tests/sensor_ref.py, and the two agree BIT FOR BIT: the random words are Philox4x32-10 of
// (pixel, global sample, step; seed) -- sensor_rng.h, the same on any number of ranks and after --resume -- the Gaussian is a
// 65 536-entry table built on the host (no logf, no cosf), and the arithmetic is three fp32 operations rounded on their own
// (built with -ffp-contract=off, like train_data.hip).  The per-pixel rule is sensor_pixel.h's, shared with the host-side
// sanitizer check.
//
// One launch over (B,1,p,p), one thread per pixel, NOT in place (the edge term reads the input's neighbours): 8 bytes per
// pixel, one table gather, ten Philox rounds.  No atomics, no LDS.

#include "codon_common.h"
#include "kernels.h"
#include "sensor_pixel.h"

#pragma clang fp contract(off)

namespace codon {

// grid (ceil(p*p / 256), B)
__global__ __launch_bounds__(256) void lr_sensor_kernel(const SensorArgs a, const float* __restrict__ lr,
                                                        const float* __restrict__ gauss, const float* __restrict__ lut,
                                                        float* __restrict__ out) {
  const int idx = blockIdx.x * 256 + threadIdx.x, pp = a.p * a.p;
  if (idx >= pp) return;
  const int b = blockIdx.y, y = idx / a.p;
  const long base = (long)b * pp;
  out[base + idx] = sensor_pixel(a, lr + base, gauss, lut, b, y, idx - y * a.p);
}

int lr_sensor(const SensorArgs& a, int B, const float* lr, const float* gauss, const float* lut, float* out,
              hipStream_t stream) {
  const dim3 grid((unsigned)((a.p * a.p + 255) / 256), (unsigned)B);
  hipLaunchKernelGGL(lr_sensor_kernel, grid, dim3(256), 0, stream, a, lr, gauss, lut, out);
  return check_launch("lr_sensor_kernel");
}

}  // namespace codon
