// Training-batch synthesis on the device (codon_amd.train): crop + D4 augmentation + u8 -> fp32 of a whole batch, the
// antialiased bicubic reduction x4 / x8 / x16, and the 8-bit quantisation of the network's depth input.  The reference ships
// no training code and no degradation script (its depth inputs were made offline and saved as 8-bit PNGs,
// CODON_X4/test.py:70-79,116-123 of the reference), so this pipeline is a DEFINITION, unpinned against the reference; it is
// restated in numpy in tests/train_data_ref.py and the two must agree BIT FOR BIT (built with -ffp-contract=off, like
// upsample.hip).
//
// crops:      t[b][i][j] = lut[code of the depth plane at (y0 + i', x0 + j')],  y[b][i][j] the same from the guidance,
//             (i', j') = D4 op of (i, j); where the planes of a record sit is train_record.h's, for all its layouts
//             labeled: source from the depth map, target from the label plane
// downsample: PIL BICUBIC reduce (Keys a = -0.5 stretched by s, 4s taps per axis, out-of-image taps dropped and the rest
//             renormalised): weights from the host, one row of 4s per output index; a horizontal pass, then a vertical pass,
//             each a sequential fp32 sum over k = 0 .. 4s-1 of w[k] * v[clamp(o*s - 3s/2 + k)] (dropped taps have w = 0).
// quantize:   x = lut[rint(clamp(x, 0, 1) * 255f)]  (round half to even)
//
// 16-bit depth: code c is lut16[c] = float32(float64(c) / depth_max), a 65 536-entry table, and the degraded
// input goes back onto the data set's own grid: x = lut16[rint(clamp(x, 0, 1) * (float)depth_max)].

#include "kernels.h"
#include "train_record.h"

#pragma clang fp contract(off)

namespace codon {

// grid (ceil(P*P / 256), B): one thread per output pixel of one sample.  `lut` converts the depth (and label) codes of BITS
// bits, lut8 the guidance; LABEL: `source` from the depth plane and `target` from the label plane -- without one `source` is
// the HR target too and `target` is not written.
template <int BITS, bool LABEL>
__global__ __launch_bounds__(256) void train_crops_kernel(const CropArgs a, const unsigned char* __restrict__ pool,
                                                          const float* __restrict__ lut, const float* __restrict__ lut8,
                                                          float* __restrict__ source, float* __restrict__ guide,
                                                          float* __restrict__ target, int P) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= P * P) return;
  const codon_crop_sample d = a.s[blockIdx.y];
  const CropPixel c = crop_pixel(idx, d, P);
  const RecordLayout r = record_layout(BITS, LABEL, 0, d.height, d.width);
  const unsigned char* rec = pool + d.offset;                        // even for u16 records (ABI check)
  const long px = (long)c.gy * d.width + c.gx;
  source[c.out] = lut[record_code<BITS>(rec + r.depth, px)];
  guide[c.out] = lut8[rec[r.guide + px]];
  if (LABEL) target[c.out] = lut[record_code<BITS>(rec + r.label, px)];
}

// one workgroup per (output row oy, sample b): the horizontal pass of the 4s input rows that row reads goes to LDS, then
// each thread finishes output columns from it
__global__ __launch_bounds__(256) void bicubic_down_kernel(const float* __restrict__ hr, const float* __restrict__ wtab,
                                                           float* __restrict__ out, int P, int s) {
  extern __shared__ float hrow[];                        // [4s][P/s]
  const int p = P / s, taps = 4 * s, oy = blockIdx.x, b = blockIdx.y;
  const float* img = hr + (long)b * P * P;
  const int r0 = oy * s - 3 * s / 2;
  for (int e = threadIdx.x; e < taps * p; e += 256) {
    const int k = e / p, ox = e - k * p;
    const int r = min(max(r0 + k, 0), P - 1);
    const float* row = img + (long)r * P;
    const float* w = wtab + (long)ox * taps;
    const int c0 = ox * s - 3 * s / 2;
    float acc = 0.f;
    for (int q = 0; q < taps; ++q) acc = acc + w[q] * row[min(max(c0 + q, 0), P - 1)];
    hrow[e] = acc;
  }
  __syncthreads();
  const float* w = wtab + (long)oy * taps;
  for (int ox = threadIdx.x; ox < p; ox += 256) {
    float acc = 0.f;
    for (int k = 0; k < taps; ++k) acc = acc + w[k] * hrow[k * p + ox];
    out[((long)b * p + oy) * p + ox] = acc;
  }
}

__global__ __launch_bounds__(256) void quantize_levels_kernel(float* __restrict__ x, const float* __restrict__ lut,
                                                              float levels, long n) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = fminf(fmaxf(x[i], 0.f), 1.f) * levels;       // NaN: fmaxf gives 0
    x[i] = lut[(int)rintf(v)];
  }
}

// bits 8: lut8 is lut.  target == nullptr: records without a label plane.
int train_crops(const codon_crop_desc* d, const unsigned char* pool, int bits, const float* lut, const float* lut8,
                float* source, float* guide, float* target, hipStream_t stream) {
  const CropArgs a = pack_crop_args(d);
  const int P = d->crop;
  const dim3 grid((unsigned)((P * P + 255) / 256), (unsigned)d->n);
#define CODON_LAUNCH_CROPS(BITS_, LABEL_)                                                                          \
  hipLaunchKernelGGL((train_crops_kernel<BITS_, LABEL_>), grid, dim3(256), 0, stream, a, pool, lut, lut8, source, guide, \
                     target, P)
  if (bits == 16 && target) CODON_LAUNCH_CROPS(16, true);
  else if (bits == 16) CODON_LAUNCH_CROPS(16, false);
  else if (target) CODON_LAUNCH_CROPS(8, true);
  else CODON_LAUNCH_CROPS(8, false);
#undef CODON_LAUNCH_CROPS
  return check_launch("train_crops_kernel");
}

int bicubic_downsample(int B, int P, int s, const float* hr, const float* wtab, float* out, hipStream_t stream) {
  const size_t lds = (size_t)4 * P * sizeof(float);     // 4s rows of P/s values
  hipLaunchKernelGGL(bicubic_down_kernel, dim3((unsigned)(P / s), (unsigned)B), dim3(256), lds, stream, hr, wtab, out, P, s);
  return check_launch("bicubic_down_kernel");
}

// quantize_u8 is levels 255 with the 256-entry table
int quantize_levels(long n, float* x, const float* lut, int levels, hipStream_t stream) {
  const long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(quantize_levels_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, x, lut,
                     (float)levels, n);
  return check_launch("quantize_levels_kernel");
}

}  // namespace codon
