// (w0*p0 + w1*p1) + (w2*p2 + w3*p3), every operation rounded on its own: the one 4-tap form of the bicubic kernels
// (upsample.hip, resample_masked.hip), restated in numpy by the oracles.  HIP's __fmul_rn / __fadd_rn are plain * and +
// and would be contracted into v_fma under the default -ffp-contract=fast, so the files that include this are built
// with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace codon {

__device__ __forceinline__ float dot4_rn(float w0, float w1, float w2, float w3, float p0, float p1, float p2,
                                         float p3) {
  return __fadd_rn(__fadd_rn(__fmul_rn(w0, p0), __fmul_rn(w1, p1)), __fadd_rn(__fmul_rn(w2, p2), __fmul_rn(w3, p3)));
}

}  // namespace codon
