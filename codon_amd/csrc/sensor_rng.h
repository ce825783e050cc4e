// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), the counter-based
// generator of the training degradation's sensor model (sensor.hip): plain C++ -- a 64-bit multiply for the two
// 32 x 32 -> 64 products of a round, no inline assembly -- so that the SAME text compiles for the device, for the host entry
// codon_philox4x32_10 (held to the published known-answer vectors by the CPU suite) and for a plain host compiler
// (tools/sensor_host_check.cpp).  Restated on numpy uint64 arrays in tests/sensor_ref.py.
//
// The four output words are a pure function of a 128-bit counter and a 64-bit key: no state, nothing to save or to ship --
// a resumed run, or rank r of N, regenerates exactly the words the uninterrupted single process drew.
#pragma once

#if defined(__HIPCC__)
#define CODON_SENSOR_HD __host__ __device__ __forceinline__
#else
#define CODON_SENSOR_HD inline
#endif

namespace codon {

struct Philox4 {
  unsigned w[4];
};

CODON_SENSOR_HD Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
  constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;       // the round multipliers
  constexpr unsigned W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;       // the key schedule's Weyl increments
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)M0 * c0, p1 = (unsigned long long)M1 * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1;
    c3 = (unsigned)p0;
    c0 = n0;
    c2 = n2;
    k0 += W0;                                                  // (the bump after the last round is unused)
    k1 += W1;
  }
  Philox4 o;
  o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
  return o;
}

}  // namespace codon
