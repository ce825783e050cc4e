// Training-batch synthesis on the device (codon_amd.train): crop + D4 augmentation + u8 -> fp32 of a whole batch, the
// antialiased bicubic reduction x4 / x8 / x16, and the 8-bit quantisation of the network's depth input.  The reference ships
// no training code and no degradation script (its depth inputs were made offline and saved as 8-bit PNGs,
// CODON_X4/test.py:70-79,116-123 of the reference), so this pipeline is a DEFINITION, unpinned against the reference; it is
// restated in numpy in tests/train_data_ref.py and the two must agree BIT FOR BIT (built with -ffp-contract=off, like
// upsample.hip).
//
// crops:      t[b][i][j] = lut[pool[off + (y0 + i')*W + (x0 + j')]],  y[b][i][j] the same from the guidance (at off + H*W),
//             (i', j') = D4 op of (i, j) -- numpy: c = img[y0:y0+P, x0:x0+P]; op&1: c = c.T; op&2: c = c[::-1];
//             op&4: c = c[:, ::-1]
//             labeled: a third plane, the label, at off + 2*H*W -- source from the depth map, target from the label
// downsample: PIL BICUBIC reduce (Keys a = -0.5 stretched by s, 4s taps per axis, out-of-image taps dropped and the rest
//             renormalised): weights from the host, one row of 4s per output index; a horizontal pass, then a vertical pass,
//             each a sequential fp32 sum over k = 0 .. 4s-1 of w[k] * v[clamp(o*s - 3s/2 + k)] (dropped taps have w = 0).
// quantize:   x = lut[rint(clamp(x, 0, 1) * 255f)]  (round half to even)
//
// 16-bit depth: the same window and D4 op over records of little-endian u16 depth (and label) planes followed by
// the u8 guidance; code c is lut16[c] = float32(float64(c) / depth_max), a 65 536-entry table, and the degraded input goes back
// onto the data set's own grid: x = lut16[rint(clamp(x, 0, 1) * (float)depth_max)].

#include "codon_common.h"

#pragma clang fp contract(off)

namespace codon {

struct CropArgs {
  codon_crop_sample s[CODON_TRAIN_MAX_BATCH];
};
static_assert(sizeof(CropArgs) + 64 <= CODON_KERNARG_LIMIT, "passed by value as a kernel argument");

// grid (ceil(P*P / 256), B): one thread per output pixel of one sample
__global__ __launch_bounds__(256) void train_crops_kernel(const CropArgs a, const unsigned char* __restrict__ pool,
                                                          const float* __restrict__ lut, float* __restrict__ target,
                                                          float* __restrict__ guide, int P) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= P * P) return;
  const codon_crop_sample d = a.s[blockIdx.y];
  const int i = idx / P, j = idx - i * P;
  int si = i, sj = j;
  if (d.op & 4) sj = P - 1 - sj;
  if (d.op & 2) si = P - 1 - si;
  if (d.op & 1) { const int t = si; si = sj; sj = t; }
  const long hw = (long)d.height * d.width;
  const long src = d.offset + (long)(d.y0 + si) * d.width + (d.x0 + sj);
  const long o = (long)blockIdx.y * P * P + idx;
  target[o] = lut[pool[src]];
  guide[o] = lut[pool[src + hw]];
}

// the same window, op and table with a third plane: the degradation source from the depth map, the target from the label that
// follows the guidance (at off + 2*H*W)
__global__ __launch_bounds__(256) void train_crops_labeled_kernel(const CropArgs a, const unsigned char* __restrict__ pool,
                                                                  const float* __restrict__ lut, float* __restrict__ source,
                                                                  float* __restrict__ guide, float* __restrict__ target,
                                                                  int P) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= P * P) return;
  const codon_crop_sample d = a.s[blockIdx.y];
  const int i = idx / P, j = idx - i * P;
  int si = i, sj = j;
  if (d.op & 4) sj = P - 1 - sj;
  if (d.op & 2) si = P - 1 - si;
  if (d.op & 1) { const int t = si; si = sj; sj = t; }
  const long hw = (long)d.height * d.width;
  const long src = d.offset + (long)(d.y0 + si) * d.width + (d.x0 + sj);
  const long o = (long)blockIdx.y * P * P + idx;
  source[o] = lut[pool[src]];
  guide[o] = lut[pool[src + hw]];
  target[o] = lut[pool[src + 2 * hw]];
}

// 16-bit records: depth plane (H*W u16) at the even byte offset `offset`, then -- labeled -- the label plane (H*W u16), then
// the guidance (H*W u8).  target == nullptr: the unlabeled record, `source` is the HR target too.  Uniform branch.
__global__ __launch_bounds__(256) void train_crops_u16_kernel(const CropArgs a, const unsigned char* __restrict__ pool,
                                                              const float* __restrict__ lut16, const float* __restrict__ lut8,
                                                              float* __restrict__ source, float* __restrict__ guide,
                                                              float* __restrict__ target, int P) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= P * P) return;
  const codon_crop_sample d = a.s[blockIdx.y];
  const int i = idx / P, j = idx - i * P;
  int si = i, sj = j;
  if (d.op & 4) sj = P - 1 - sj;
  if (d.op & 2) si = P - 1 - si;
  if (d.op & 1) { const int t = si; si = sj; sj = t; }
  const long hw = (long)d.height * d.width;
  const long px = (long)(d.y0 + si) * d.width + (d.x0 + sj);
  const unsigned short* depth = reinterpret_cast<const unsigned short*>(pool + d.offset);      // offset is even (ABI check)
  const long o = (long)blockIdx.y * P * P + idx;
  source[o] = lut16[depth[px]];
  if (target != nullptr) {
    target[o] = lut16[depth[hw + px]];
    guide[o] = lut8[pool[d.offset + 4 * hw + px]];
  } else {
    guide[o] = lut8[pool[d.offset + 2 * hw + px]];
  }
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

__global__ __launch_bounds__(256) void quantize_u8_kernel(float* __restrict__ x, const float* __restrict__ lut, long n) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = fminf(fmaxf(x[i], 0.f), 1.f) * 255.f;
    x[i] = lut[(int)rintf(v)];
  }
}

__global__ __launch_bounds__(256) void quantize_levels_kernel(float* __restrict__ x, const float* __restrict__ lut16,
                                                              float levels, long n) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = fminf(fmaxf(x[i], 0.f), 1.f) * levels;       // NaN: fmaxf gives 0
    x[i] = lut16[(int)rintf(v)];
  }
}

int train_crops(const codon_crop_desc* d, const unsigned char* pool, const float* lut, float* target, float* guide,
                hipStream_t stream) {
  CropArgs a;
  for (int b = 0; b < d->n; ++b) a.s[b] = d->s[b];
  for (int b = d->n; b < CODON_TRAIN_MAX_BATCH; ++b) a.s[b] = codon_crop_sample{};
  const int P = d->crop;
  hipLaunchKernelGGL(train_crops_kernel, dim3((unsigned)((P * P + 255) / 256), (unsigned)d->n), dim3(256), 0, stream, a, pool,
                     lut, target, guide, P);
  return check_launch("train_crops_kernel");
}

int train_crops_labeled(const codon_crop_desc* d, const unsigned char* pool, const float* lut, float* source, float* guide,
                        float* target, hipStream_t stream) {
  CropArgs a;
  for (int b = 0; b < d->n; ++b) a.s[b] = d->s[b];
  for (int b = d->n; b < CODON_TRAIN_MAX_BATCH; ++b) a.s[b] = codon_crop_sample{};
  const int P = d->crop;
  hipLaunchKernelGGL(train_crops_labeled_kernel, dim3((unsigned)((P * P + 255) / 256), (unsigned)d->n), dim3(256), 0, stream, a,
                     pool, lut, source, guide, target, P);
  return check_launch("train_crops_labeled_kernel");
}

int train_crops_u16(const codon_crop_desc* d, const unsigned char* pool, const float* lut16, const float* lut8, float* source,
                    float* guide, float* target, hipStream_t stream) {
  CropArgs a;
  for (int b = 0; b < d->n; ++b) a.s[b] = d->s[b];
  for (int b = d->n; b < CODON_TRAIN_MAX_BATCH; ++b) a.s[b] = codon_crop_sample{};
  const int P = d->crop;
  hipLaunchKernelGGL(train_crops_u16_kernel, dim3((unsigned)((P * P + 255) / 256), (unsigned)d->n), dim3(256), 0, stream, a, pool,
                     lut16, lut8, source, guide, target, P);
  return check_launch("train_crops_u16_kernel");
}

int bicubic_downsample(int B, int P, int s, const float* hr, const float* wtab, float* out, hipStream_t stream) {
  const size_t lds = (size_t)4 * P * sizeof(float);     // 4s rows of P/s values
  hipLaunchKernelGGL(bicubic_down_kernel, dim3((unsigned)(P / s), (unsigned)B), dim3(256), lds, stream, hr, wtab, out, P, s);
  return check_launch("bicubic_down_kernel");
}

int quantize_u8(long n, float* x, const float* lut, hipStream_t stream) {
  const long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(quantize_u8_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, x, lut, n);
  return check_launch("quantize_u8_kernel");
}

int quantize_levels(long n, float* x, const float* lut16, int depth_max, hipStream_t stream) {
  const long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(quantize_levels_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, x, lut16,
                     (float)depth_max, n);
  return check_launch("quantize_levels_kernel");
}

}  // namespace codon
