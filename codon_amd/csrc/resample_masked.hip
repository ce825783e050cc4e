// Hole-aware (mask-normalised) bicubic resampling of depth maps in which 0.0 / code 0 marks a hole: the masked
// twins of bicubic_kernel (upsample.hip) and bicubic_down_kernel (train_data.hip), the fused inference kernel that turns a
// sensor's low-resolution code plane into the network's depth input in one launch, and its training twin (train_crops_lr,
// DESIGN 12.5).  No reference counterpart (the reference ships neither a degradation nor an upsampler): these are
// DEFINITIONS, restated in numpy in tests/resample_masked_ref.py (the training twin in tests/train_lr_ref.py), and
// the two agree BIT FOR BIT -- built with -ffp-contract=off, every multiply, add and divide rounded on its own (the fp32
// divide is hipcc's correctly rounded default; nothing here relaxes it).
//
// The rule, for a numerator N (the unmasked kernel's own arithmetic, holes entering as their 0.0), a denominator D (the same
// arithmetic over the validity m in {0.0f, 1.0f}) and the count of invalid taps:
//   0 invalid    -> N, valid              (the unmasked kernel's bits)
//   D >= 0.5f    -> N / D, valid
//   otherwise    -> +0.0f, a hole         (0.5 keeps D away from the cubic's negative lobes)
//
// upsample:   index arithmetic, phase table, border clamp and dot4_rn are bicubic_kernel's; a clamped tap is a real tap and
//             carries its clamped pixel's validity.  n_k = dot4_rn(wx, v), d_k = dot4_rn(wx, m) per tap row, then
//             N = dot4_rn(wy, n), D = dot4_rn(wy, d); the count runs over all 16 taps.
// downsample: weight table, tap range, clamping and the two sequential fp32 passes are bicubic_down_kernel's, carried for the
//             numerator and the denominator; the count runs over the taps INSIDE the image (a clamped out-of-image tap has
//             weight 0 and is not counted).  A valid value is snapped as a sensor's file would hold it:
//             code = min(max((int)rintf(clamp(v, 0, 1) * levels), 1), levels), out = lut[code] -- never code 0.
// fused:      codes (u8 / u16) -> lut -> upsample rule -> lut[(int)rintf(clamp(., 0, 1) * levels)] -> round to nearest even
//             into fp32 / fp16 / bf16: bicubic_masked_kernel, quantize_levels_kernel and a cast, fused.
// paired:     a training batch from records that carry a sensor's low-resolution code plane: t and y are the crop
//             kernels' look-ups, x is the fused kernel's fp32 value at the source pixel of the WHOLE plane -- the window, under
//             the D4 op, of what inference builds from the file.  Restated in numpy in tests/train_lr_ref.py.

#include <hip/hip_fp16.h>

#include "dot4_rn.h"
#include "kernels.h"
#include "train_record.h"

#pragma clang fp contract(off)

namespace codon {

__device__ __forceinline__ float masked_rule(float N, float D, int invalid, bool* ok) {
  if (invalid == 0) { *ok = true; return N; }
  if (D >= 0.5f) { *ok = true; return N / D; }
  *ok = false;
  return 0.f;
}

// The upsample rule for one output pixel whose taps are looked up already: v is a register window of 4 tap rows of which the
// pixel reads columns o .. o + 3 (o a constant once the caller's loop is unrolled, so the window is indexed by constants only
// and stays in registers), wx and wy the weight rows of its phases.  Rows then columns for the numerator; the denominator,
// the count and the rule only where one of the 16 taps is a hole -- with none the rule gives the numerator's bits.
template <int NW>
__device__ __forceinline__ float bicubic4x4_masked(const float (&v)[4][NW], int o, const float* __restrict__ wx,
                                                   const float* __restrict__ wy, bool* ok) {
  const float w0 = wx[0], w1 = wx[1], w2 = wx[2], w3 = wx[3];
  float nrow[4];
  bool anyhole = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    nrow[k] = dot4_rn(w0, w1, w2, w3, v[k][o], v[k][o + 1], v[k][o + 2], v[k][o + 3]);
#pragma unroll
    for (int c = 0; c < 4; ++c) anyhole = anyhole || !(v[k][o + c] != 0.f);
  }
  float r = dot4_rn(wy[0], wy[1], wy[2], wy[3], nrow[0], nrow[1], nrow[2], nrow[3]);
  *ok = true;
  if (anyhole) {
    float drow[4];
    int invalid = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float m[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        m[c] = v[k][o + c] != 0.f ? 1.f : 0.f;
        invalid += v[k][o + c] != 0.f ? 0 : 1;
      }
      drow[k] = dot4_rn(w0, w1, w2, w3, m[0], m[1], m[2], m[3]);
    }
    const float D = dot4_rn(wy[0], wy[1], wy[2], wy[3], drow[0], drow[1], drow[2], drow[3]);
    r = masked_rule(r, D, invalid, ok);
  }
  return r;
}

// one thread per output pixel, as bicubic_kernel
__global__ __launch_bounds__(256) void bicubic_masked_kernel(const float* __restrict__ lr, const float* __restrict__ wtab,
                                                             float* __restrict__ out, unsigned char* __restrict__ valid, int h,
                                                             int w, int s, long total) {
  const long idx = blockIdx.x * 256L + threadIdx.x;
  if (idx >= total) return;
  const int W = w * s, H = h * s;
  const int gx = (int)(idx % W);
  const long t = idx / W;
  const int gy = (int)(t % H);
  const int b = (int)(t / H);
  const int qx = gx / s, rx = gx - qx * s, qy = gy / s, ry = gy - qy * s;
  const int ix0 = qx - ((2 * rx + 1 < s) ? 1 : 0), iy0 = qy - ((2 * ry + 1 < s) ? 1 : 0);
  const float* wx = wtab + rx * 4;
  const float* wy = wtab + ry * 4;
  int xs[4], ys[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    xs[k] = min(max(ix0 - 1 + k, 0), w - 1);
    ys[k] = min(max(iy0 - 1 + k, 0), h - 1);
  }
  const float* p = lr + (long)b * h * w;
  float v[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float* r = p + (long)ys[k] * w;
#pragma unroll
    for (int c = 0; c < 4; ++c) v[k][c] = r[xs[c]];
  }
  bool ok;
  out[idx] = bicubic4x4_masked(v, 0, wx, wy, &ok);
  if (valid != nullptr) valid[idx] = ok ? 1 : 0;
}

// one workgroup per (output row oy, sample b), as bicubic_down_kernel: the horizontal pass of the 4s input rows goes to LDS as
// three planes [4s][P/s] -- numerator, denominator, invalid in-image taps -- then each thread finishes output columns
__global__ __launch_bounds__(256) void bicubic_down_masked_kernel(const float* __restrict__ hr, const float* __restrict__ wtab,
                                                                  const float* __restrict__ lut, float levels, int top,
                                                                  float* __restrict__ out, int P, int s) {
  extern __shared__ float hrow[];                        // [3][4s][P/s]
  const int p = P / s, taps = 4 * s, oy = blockIdx.x, b = blockIdx.y;
  float* hnum = hrow;
  float* hden = hrow + taps * p;
  int* hcnt = reinterpret_cast<int*>(hrow + 2 * taps * p);
  const float* img = hr + (long)b * P * P;
  const int r0 = oy * s - 3 * s / 2;
  for (int e = threadIdx.x; e < taps * p; e += 256) {
    const int k = e / p, ox = e - k * p;
    const int r = min(max(r0 + k, 0), P - 1);
    const float* row = img + (long)r * P;
    const float* w = wtab + (long)ox * taps;
    const int c0 = ox * s - 3 * s / 2;
    float acc = 0.f, den = 0.f;
    int cnt = 0;
    for (int q = 0; q < taps; ++q) {
      const int c = c0 + q;
      const float v = row[min(max(c, 0), P - 1)];
      const bool hole = !(v != 0.f);
      acc = acc + w[q] * v;
      den = den + w[q] * (hole ? 0.f : 1.f);
      cnt += (hole && c >= 0 && c < P) ? 1 : 0;
    }
    hnum[e] = acc;
    hden[e] = den;
    hcnt[e] = cnt;
  }
  __syncthreads();
  const float* w = wtab + (long)oy * taps;
  for (int ox = threadIdx.x; ox < p; ox += 256) {
    float acc = 0.f, den = 0.f;
    int cnt = 0;
    for (int k = 0; k < taps; ++k) {
      acc = acc + w[k] * hnum[k * p + ox];
      den = den + w[k] * hden[k * p + ox];
      cnt += (r0 + k >= 0 && r0 + k < P) ? hcnt[k * p + ox] : 0;
    }
    bool ok;
    const float v = masked_rule(acc, den, cnt, &ok);
    float res = 0.f;
    if (ok) {
      const int code = min(max((int)rintf(fminf(fmaxf(v, 0.f), 1.f) * levels), 1), top);
      res = lut[code];
    }
    out[((long)b * p + oy) * p + ox] = res;
  }
}

// ---- codes -> network input -------------------------------------------------------------------------------------------------
// One lane produces a run of R consecutive output pixels of one row and stores them at once (R = 4 fp32: 16 bytes; R = 8
// 16-bit values: 16 bytes; R = 4 16-bit values, 8 bytes, where the row length is no multiple of 8).  R divides the row length
// and S is a multiple of R or R of S, so with ix0 = (gx + S/2) / S - 1 (bicubic_kernel's qx - (2 rx + 1 < s), in one
// expression) pixel j of a run reads taps ix0(0) + OFF(j) - 1 .. + 2 with OFF(j) = R >= S ? (j + S/2) / S : 0, a compile-time
// number: the run's 4 x NW window of codes lives in registers and is indexed by constants only.
template <int S, int R>
struct RunShape {
  static constexpr int off(int j) { return R >= S ? (j + S / 2) / S : 0; }
  static constexpr int NW = 4 + off(R - 1);
};

__device__ __forceinline__ unsigned short to_bits16(float v, int dtype) {
  if (dtype == CODON_F16) return __half_as_ushort(__float2half_rn(v));
  const unsigned u = __float_as_uint(v);                 // bf16, round to nearest even (finite, non-negative values)
  return (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// CODES: the run is written as the INTEGERS the look-up takes, (int)rintf(clamp(., 0, 1) * levels), in the codes' own width (a
// hole stays 0) -- codon_lr_codes_upsample, the bicubic baseline; R = 4: 4 or 8 bytes per lane
template <int S, int R, bool CODES>
__global__ __launch_bounds__(256) void lr_codes_to_input_kernel(const void* __restrict__ codes, int code16,
                                                                const float* __restrict__ lut, float levels,
                                                                const float* __restrict__ wtab, void* __restrict__ out,
                                                                int dtype, int h, int w, long runs) {
  using Sh = RunShape<S, R>;
  constexpr int NW = Sh::NW;
  const long run = blockIdx.x * 256L + threadIdx.x;
  if (run >= runs) return;
  const int W = w * S, H = h * S, rpr = W / R;           // runs per row
  const int gx0 = (int)(run % rpr) * R;
  const long t = run / rpr;
  const int gy = (int)(t % H);
  const int b = (int)(t / H);
  const int qy = gy / S, ry = gy - qy * S;
  const int iy0 = qy - ((2 * ry + 1 < S) ? 1 : 0);
  const int ixf = (gx0 + S / 2) / S - 1;
  const float* wy = wtab + ry * 4;
  const long plane = (long)b * h * w;
  float v[4][NW];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long row = plane + (long)min(max(iy0 - 1 + k, 0), h - 1) * w;
#pragma unroll
    for (int c = 0; c < NW; ++c) {
      const long at = row + min(max(ixf - 1 + c, 0), w - 1);
      const int code = code16 ? (int)static_cast<const unsigned short*>(codes)[at]
                              : (int)static_cast<const unsigned char*>(codes)[at];
      v[k][c] = lut[code];
    }
  }
  float res[R];
  int code[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    bool ok;
    const float r = bicubic4x4_masked(v, Sh::off(j), wtab + (gx0 + j) % S * 4, wy, &ok);
    code[j] = (int)rintf(fminf(fmaxf(r, 0.f), 1.f) * levels);
    if constexpr (!CODES) res[j] = lut[code[j]];
  }
  const long at = run * R;
  if constexpr (CODES) {                                 // R == 4 (host rule)
    if (code16) {
      uint2 o2 = make_uint2((unsigned)code[0] | ((unsigned)code[1] << 16), (unsigned)code[2] | ((unsigned)code[3] << 16));
      *reinterpret_cast<uint2*>(static_cast<unsigned short*>(out) + at) = o2;
    } else {
      *reinterpret_cast<unsigned*>(static_cast<unsigned char*>(out) + at) =
          (unsigned)code[0] | ((unsigned)code[1] << 8) | ((unsigned)code[2] << 16) | ((unsigned)code[3] << 24);
    }
  } else if (dtype == CODON_F32) {                              // R == 4 (host rule)
    f32x4 o4;
    o4[0] = res[0]; o4[1] = res[1]; o4[2] = res[2]; o4[3] = res[3];
    *reinterpret_cast<f32x4*>(static_cast<float*>(out) + at) = o4;
  } else {
    unsigned pk[R / 2];
#pragma unroll
    for (int j = 0; j < R / 2; ++j)
      pk[j] = (unsigned)to_bits16(res[2 * j], dtype) | ((unsigned)to_bits16(res[2 * j + 1], dtype) << 16);
    unsigned short* dst = static_cast<unsigned short*>(out) + at;
    if constexpr (R == 8) {
      uint4 o4 = make_uint4(pk[0], pk[1], pk[2], pk[3]);
      *reinterpret_cast<uint4*>(dst) = o4;
    } else {
      uint2 o2 = make_uint2(pk[0], pk[1]);
      *reinterpret_cast<uint2*>(dst) = o2;
    }
  }
}

// ---- paired training: records with a low-resolution code plane -> x, y, t -------------------------------------
// grid (ceil(P*P / 256), B), one thread per output pixel of one sample; window, D4 op and record layout are train_record.h's
// ((h, w) = (H / S, W / S) is the LR plane's size).  t and y are the crop kernels' table look-ups at the source pixel
// (gy, gx); x is what lr_codes_to_input_kernel writes at (gy, gx) of the WHOLE plane in fp32: bicubic_masked_kernel's index
// arithmetic with the border clamp at the image's edge (the window's real neighbours are read), lut[code] for the 16 taps, the
// rule, back onto the code grid.
template <int S>
__global__ __launch_bounds__(256) void train_crops_lr_kernel(const CropArgs a, const unsigned char* __restrict__ pool,
                                                             int code16, const float* __restrict__ lut, float levels,
                                                             const float* __restrict__ lut8, const float* __restrict__ wtab,
                                                             float* __restrict__ x, float* __restrict__ guide,
                                                             float* __restrict__ target, int P) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= P * P) return;
  const codon_crop_sample d = a.s[blockIdx.y];
  const CropPixel cp = crop_pixel(idx, d, P);
  const int gy = cp.gy, gx = cp.gx;
  const int h = d.height / S, w = d.width / S;
  const RecordLayout rl = record_layout(code16 ? 16 : 8, false, S, d.height, d.width);
  const unsigned char* rec = pool + d.offset;            // even for u16 records (ABI check)
  const unsigned char* lrp = rec + rl.lr;
  const long px = (long)gy * d.width + gx;
  target[cp.out] = lut[code16 ? record_code<16>(rec + rl.depth, px) : record_code<8>(rec + rl.depth, px)];
  guide[cp.out] = lut8[rec[rl.guide + px]];
  const int qx = gx / S, rx = gx - qx * S, qy = gy / S, ry = gy - qy * S;
  const int ix0 = qx - ((2 * rx + 1 < S) ? 1 : 0), iy0 = qy - ((2 * ry + 1 < S) ? 1 : 0);
  int xs[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) xs[c] = min(max(ix0 - 1 + c, 0), w - 1);
  float v[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long row = (long)min(max(iy0 - 1 + k, 0), h - 1) * w;
#pragma unroll
    for (int c = 0; c < 4; ++c) v[k][c] = lut[code16 ? record_code<16>(lrp, row + xs[c]) : record_code<8>(lrp, row + xs[c])];
  }
  bool ok;
  const float r = bicubic4x4_masked(v, 0, wtab + rx * 4, wtab + ry * 4, &ok);
  x[cp.out] = lut[(int)rintf(fminf(fmaxf(r, 0.f), 1.f) * levels)];
}

int train_crops_lr(const codon_crop_desc* d, const unsigned char* pool, int s, int code_bits, const float* lut, int levels,
                   const float* lut8, const float* wtab, float* x, float* guide, float* target, hipStream_t stream) {
  const CropArgs a = pack_crop_args(d);
  const int P = d->crop, code16 = code_bits == 16 ? 1 : 0;
  const dim3 grid((unsigned)((P * P + 255) / 256), (unsigned)d->n);
#define CODON_LAUNCH_CROPS_LR(S_)                                                                                   \
  hipLaunchKernelGGL((train_crops_lr_kernel<S_>), grid, dim3(256), 0, stream, a, pool, code16, lut, (float)levels, lut8, wtab, \
                     x, guide, target, P)
  if (s == 4) CODON_LAUNCH_CROPS_LR(4);
  else if (s == 8) CODON_LAUNCH_CROPS_LR(8);
  else CODON_LAUNCH_CROPS_LR(16);
#undef CODON_LAUNCH_CROPS_LR
  return check_launch("train_crops_lr_kernel");
}

int bicubic_upsample_masked(int B, int h, int w, int s, const float* lr, const float* wtab, float* out, unsigned char* valid,
                            hipStream_t stream) {
  const long total = (long)B * h * s * w * s;
  const long blocks = (total + 255) / 256;
  CODON_REQUIRE(blocks < (1L << 31), CODON_ERR_UNSUPPORTED, "bicubic_upsample_masked: grid too large");
  hipLaunchKernelGGL(bicubic_masked_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, lr, wtab, out, valid, h, w, s, total);
  return check_launch("bicubic_masked_kernel");
}

int bicubic_downsample_masked(int B, int P, int s, const float* hr, const float* wtab, const float* lut, int levels, float* out,
                              hipStream_t stream) {
  const size_t lds = (size_t)3 * 4 * P * sizeof(float);  // three planes of 4s rows of P/s values: 48 KiB at P = 1024
  hipLaunchKernelGGL(bicubic_down_masked_kernel, dim3((unsigned)(P / s), (unsigned)B), dim3(256), lds, stream, hr, wtab, lut,
                     (float)levels, levels, out, P, s);
  return check_launch("bicubic_down_masked_kernel");
}

template <int S, int R, bool CODES = false>
static int launch_codes(int B, int h, int w, const void* codes, int code16, const float* lut, int levels, const float* wtab,
                        void* out, int dtype, hipStream_t stream) {
  const long runs = (long)B * h * S * w * S / R;
  const long blocks = (runs + 255) / 256;
  CODON_REQUIRE(blocks < (1L << 31), CODON_ERR_UNSUPPORTED, "lr_codes_to_input: grid too large");
  hipLaunchKernelGGL((lr_codes_to_input_kernel<S, R, CODES>), dim3((unsigned)blocks), dim3(256), 0, stream, codes, code16, lut,
                     (float)levels, wtab, out, dtype, h, w, runs);
  return check_launch("lr_codes_to_input_kernel");
}

int lr_codes_to_input(int B, int h, int w, int s, const void* codes, int code_bits, const float* lut, int levels,
                      const float* wtab, void* out, int dtype, hipStream_t stream) {
  const int code16 = code_bits == 16 ? 1 : 0;
  const bool wide = dtype != CODON_F32 && ((long)w * s) % 8 == 0;      // 8 16-bit values per lane: 16 bytes
#define CODON_LAUNCH_CODES(S_)                                                                                  \
  return wide ? launch_codes<S_, 8>(B, h, w, codes, code16, lut, levels, wtab, out, dtype, stream)             \
              : launch_codes<S_, 4>(B, h, w, codes, code16, lut, levels, wtab, out, dtype, stream)
  if (s == 4) { CODON_LAUNCH_CODES(4); }
  if (s == 8) { CODON_LAUNCH_CODES(8); }
  CODON_LAUNCH_CODES(16);
#undef CODON_LAUNCH_CODES
}

// out: codes of the input's width; dtype is not looked at
int lr_codes_upsample(int B, int h, int w, int s, const void* codes, int code_bits, const float* lut, int levels,
                      const float* wtab, void* out, hipStream_t stream) {
  const int code16 = code_bits == 16 ? 1 : 0;
  if (s == 4) return launch_codes<4, 4, true>(B, h, w, codes, code16, lut, levels, wtab, out, CODON_F32, stream);
  if (s == 8) return launch_codes<8, 4, true>(B, h, w, codes, code16, lut, levels, wtab, out, CODON_F32, stream);
  return launch_codes<16, 4, true>(B, h, w, codes, code16, lut, levels, wtab, out, CODON_F32, stream);
}

}  // namespace codon
