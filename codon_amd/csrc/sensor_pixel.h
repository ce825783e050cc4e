// The per-pixel body of the sensor model (sensor.hip), written so that the SAME text compiles for the device and
// for a plain host compiler: tools/sensor_host_check.cpp drives it pixel by pixel under the address and undefined-behaviour
// sanitizers.  The including file switches floating-point contraction off: every fp32 operation is rounded on its own.
//
// One output pixel of sample b's own p x p low-resolution map `m` (values on [0, 1], in masked mode on the code grid with
// +0.0f a hole), with v = m[y][x] and the four words of philox4x32_10(y * p + x, first + b, step, 0; key):
//   hole    (masked)  v == 0.0f -> +0.0f, nothing else runs
//   edge              e = any 4-neighbour n INSIDE the map (masked: and n != 0.0f) with fabsf(v - n) > edge_thr
//   dropout (masked)  (uint64)w1 < t_drop + (e ? t_edge : 0) -> +0.0f        (t = floor(P * 2^32): P = 0 never, P = 1 always)
//   noise             g = gauss[w0 >> 16];  s = sigma + quad * (v * v);  v' = v + s * g
//   out     masked:   lut[min(max((int)rintf(clamp(v', 0, 1) * (float)levels), 1), levels)] -- the masked downsample's snap:
//                     noise never turns a valid pixel into code 0
//           unmasked: v', unclamped (the map is not snapped on that path; the final quantise clamps)
// w2 and w3 are reserved.
#pragma once

#include <math.h>

#include "sensor_rng.h"

namespace codon {

struct SensorArgs {
  int p, masked, levels;
  unsigned k0, k1, step, first;
  float sigma, quad, edge_thr;
  unsigned long long t_drop, t_edge;
};

CODON_SENSOR_HD float sensor_pixel(const SensorArgs& a, const float* m, const float* gauss, const float* lut, int b, int y,
                                   int x) {
  const int p = a.p;
  const float v = m[y * p + x];
  if (a.masked && v == 0.0f) return 0.0f;
  bool e = false;
  if (a.t_edge != 0) {                                   // (uniform; without an edge term no neighbour is read)
    const int ny[4] = {y - 1, y + 1, y, y};
    const int nx[4] = {x, x, x - 1, x + 1};
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) {
      if (ny[k] < 0 || ny[k] >= p || nx[k] < 0 || nx[k] >= p) continue;
      const float n = m[ny[k] * p + nx[k]];
      if (a.masked && n == 0.0f) continue;
      e = e || fabsf(v - n) > a.edge_thr;
    }
  }
  const Philox4 r = philox4x32_10((unsigned)(y * p + x), a.first + (unsigned)b, a.step, 0u, a.k0, a.k1);
  if (a.masked && (unsigned long long)r.w[1] < a.t_drop + (e ? a.t_edge : 0ull)) return 0.0f;
  const float g = gauss[r.w[0] >> 16];
  const float s = a.sigma + a.quad * (v * v);
  const float vn = v + s * g;
  if (!a.masked) return vn;
  const int levels = a.levels;
  const int code = (int)rintf(fminf(fmaxf(vn, 0.0f), 1.0f) * (float)levels);
  return lut[code < 1 ? 1 : (code > levels ? levels : code)];
}

}  // namespace codon
