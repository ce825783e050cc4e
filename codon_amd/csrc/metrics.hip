// "Next" rows of SURVEY.md 8(f): what sits either side of the network in the reference's script.
//   postprocess : out = uint8(clip(x,0,1) * 255)   (truncating cast)        CODON_X4/test.py:127-132
//   masked RMSE : sqrt(sum_{label != 0} (label - out)^2 / #{label != 0})    CODON_X4/test.py:148-164
//   SSIM        : ssim_exact(img1, img2, sd=1.5)                             CODON_X4/ssim_2.py:36-52
//                 (scipy gaussian_filter: 13 taps, truncate 4.0, 'reflect' = half-sample symmetric boundary)
//   L1 + SSIM loss forward/backward for the fwd+bwd config (no loss exists in the reference, SURVEY D8: the
//   combination is this repo's definition; the SSIM VALUE is pinned to ssim_exact).
// All of it is 1-channel work (B,1,H,W): a few MB, HBM-trivial; byte/integer pieces are bit-exact.

#include <math.h>

#include "codon_common.h"
#include "kernels.h"

namespace codon {

// ---- post-processing ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void postprocess_u8_kernel(const float* __restrict__ x, unsigned char* __restrict__ o,
                                                             long n) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= n) return;
  float v = x[i];
  v = fminf(fmaxf(v, 0.f), 1.f);            // np.clip(out, 0, 1)
  // (out * 255).astype(np.uint8): the product is computed in the array's dtype, then truncated toward zero
  o[i] = (unsigned char)(int)(v * 255.f);
}

// fp16 network output (the reference script's default: model.cuda().half(), test.py:52): numpy keeps the array in
// float16, so `out * 255` is ROUNDED TO fp16 (spacing 0.125 in [128,256)) before the truncating cast -- 252.96 becomes
// 253.0 -> 253, where the fp32 product would give 252.  One fp32 multiply + one rounding to fp16 is exactly numpy's
// half * half (11-bit x 8-bit significands: the fp32 product is exact).
__global__ __launch_bounds__(256) void postprocess_u8_f16_kernel(const _Float16* __restrict__ x,
                                                                 unsigned char* __restrict__ o, long n) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= n) return;
  float v = (float)x[i];
  v = fminf(fmaxf(v, 0.f), 1.f);
  const _Float16 p = (_Float16)(v * 255.f);
  o[i] = (unsigned char)(int)(float)p;
}

// sum of squared integer differences and count of valid pixels over u8 or u16 codes: exact in 64-bit integers (|d| <= 65535,
// d * d < 2^32, formed in 64 bits), so the result is independent of summation order and equals the reference's float64 loop
// bit for bit.
template <typename T>
__global__ __launch_bounds__(256) void masked_sqerr_kernel(const T* __restrict__ label, const T* __restrict__ out, long n,
                                                           unsigned long long* __restrict__ acc /* [2] */) {
  unsigned long long s = 0, c = 0;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int l = label[i];
    if (l != 0) {
      const long long d = l - (int)out[i];
      s += (unsigned long long)(d * d);
      c += 1;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    s += __shfl_xor(s, m, 64);
    c += __shfl_xor(c, m, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&acc[0], s);
    atomicAdd(&acc[1], c);
  }
}

// ---- 16-bit depth codes ------------------------------------------------------------------
// code = rint(clamp(x, 0, 1) * float32(depth_max)), round half to even; the product in fp32 whatever the input's dtype (fp16
// and bf16 are upcast first, exactly); NaN -> 0 (fmaxf returns its other operand).  No reference counterpart: the
// reference's outputs are 8-bit.  One multiply, one rounding: nothing for the compiler to contract.
template <typename T> __device__ __forceinline__ float load_f32(const T* p, long i) { return (float)p[i]; }
struct bf16_bits { unsigned short u; };
template <> __device__ __forceinline__ float load_f32<bf16_bits>(const bf16_bits* p, long i) {
  return __uint_as_float((unsigned)p[i].u << 16);
}

template <typename T>
__global__ __launch_bounds__(256) void postprocess_u16_kernel(const T* __restrict__ x, unsigned short* __restrict__ o,
                                                              float levels, long n) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= n) return;
  const float v = fminf(fmaxf(load_f32<T>(x, i), 0.f), 1.f) * levels;
  o[i] = (unsigned short)(int)rintf(v);
}

// ---- SSIM ----------------------------------------------------------------------------------------------
constexpr int SS_R = 6, SS_T = 32, SS_P = SS_T + 2 * SS_R;  // radius, tile, padded tile

__device__ __forceinline__ int reflect_idx(int i, int n) {  // scipy 'reflect': (d c b a | a b c d | d c b a)
  while (i < 0 || i >= n) {
    if (i < 0) i = -1 - i;
    if (i >= n) i = 2 * n - 1 - i;
  }
  return i;
}

struct GaussW { float w[2 * SS_R + 1]; };

// ---- the SSIM tile, unmasked and hole-aware -------------------------------------------------------------
// Validity v: valid[idx] != 0, or (valid == null) t != 0 -- masked_rmse's rule.  Invalid pixels of BOTH images are loaded as 0
// (a select, so that no value there -- NaN and Inf included -- reaches anything).  E = pixels whose whole 13x13 window, under
// the same reflect indexing, is valid; there the SSIM value is the unmasked one.  The derivative maps are 0 outside E.
__device__ __forceinline__ bool px_valid(const unsigned char* __restrict__ valid, const float* __restrict__ t, long i) {
  return valid ? valid[i] != 0 : t[i] != 0.0f;
}

// what the masked instantiation alone keeps in LDS: validity; invalid pixels in the 13 horizontal taps; the integer partials
template <bool MASKED> struct MaskTile {};
template <> struct MaskTile<true> {
  unsigned char tv[SS_P][SS_P + 4], hv[SS_P][SS_T + 4];
  int redi[2][4];
};

// One 32x32 output tile per workgroup, written once for both losses.  Per tile: the sum of the SSIM map -> out[tile] and, if
// dmaps != null, the three derivative maps d(sum ssim)/d{mu1, s11, s12} (s11 = G(x^2), s12 = G(x*t)) for the backward.
// MASKED: the sum runs over E, and out is ws, 4 * ntiles words -- [0, nt) ssim sums, [nt, 2nt) sums of |a - b| over valid pixels
// (float), [2nt, 3nt) valid counts, [3nt, 4nt) |E| (int32).  Unmasked, valid and ntiles are unused and nothing of the validity
// planes, the invalid-tap counts, the L1 sum or the integer reductions is compiled in.
template <bool MASKED>
__global__ __launch_bounds__(256) void ssim_tile_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                        const unsigned char* __restrict__ valid, float* __restrict__ out,
                                                        float* __restrict__ dmaps, int H, int W, int tiles_x, int tiles_y,
                                                        int ntiles, GaussW g, float C1, float C2) {
  __shared__ float ta[SS_P][SS_P + 1], tb[SS_P][SS_P + 1];
  __shared__ float hz[5][SS_P][SS_T + 1];
  __shared__ float red[MASKED ? 2 : 1][4];
  __shared__ MaskTile<MASKED> mk;
  const int tid = threadIdx.x;
  const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, img = blockIdx.x / (tiles_x * tiles_y);
  const int x0 = tx * SS_T, y0 = ty * SS_T;
  const float* pa = a + (long)img * H * W;
  const float* pb = b + (long)img * H * W;
  for (int e = tid; e < SS_P * SS_P; e += 256) {
    const int r = e / SS_P, c = e % SS_P;
    const int yy = reflect_idx(y0 + r - SS_R, H), xx = reflect_idx(x0 + c - SS_R, W);
    const long i = (long)yy * W + xx;
    const float av = pa[i], bv = pb[i];
    bool v = true;
    if constexpr (MASKED) {
      v = valid ? valid[(long)img * H * W + i] != 0 : bv != 0.0f;
      mk.tv[r][c] = v ? 1 : 0;
    }
    ta[r][c] = v ? av : 0.f;
    tb[r][c] = v ? bv : 0.f;
  }
  __syncthreads();
  // variances / covariance are shift invariant: take the moments of (a - ca), (b - cb) with ca, cb the tile's
  // centre pixels, so that E[x^2] - E[x]^2 does not cancel 4+ digits in fp32 on flat image regions
  const float ca = ta[SS_P / 2][SS_P / 2], cb = tb[SS_P / 2][SS_P / 2];
  for (int e = tid; e < SS_P * SS_T; e += 256) {   // horizontal pass of the 5 moments (and of the invalid count)
    const int r = e / SS_T, c = e % SS_T;
    float s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
    [[maybe_unused]] int bad = 0;
#pragma unroll
    for (int k = 0; k <= 2 * SS_R; ++k) {
      const float u = ta[r][c + k] - ca, v = tb[r][c + k] - cb, w = g.w[k];
      s0 = fmaf(w, u, s0); s1 = fmaf(w, v, s1); s2 = fmaf(w, u * u, s2); s3 = fmaf(w, v * v, s3);
      s4 = fmaf(w, u * v, s4);
      if constexpr (MASKED) bad += 1 - (int)mk.tv[r][c + k];
    }
    hz[0][r][c] = s0; hz[1][r][c] = s1; hz[2][r][c] = s2; hz[3][r][c] = s3; hz[4][r][c] = s4;
    if constexpr (MASKED) mk.hv[r][c] = (unsigned char)bad;
  }
  __syncthreads();
  float lss = 0.f;
  [[maybe_unused]] float ll1 = 0.f;
  [[maybe_unused]] int nv = 0, ne = 0;
  for (int e = tid; e < SS_T * SS_T; e += 256) {
    const int r = e / SS_T, c = e % SS_T;
    const int gy = y0 + r, gx = x0 + c;
    float m[5] = {0, 0, 0, 0, 0};
    [[maybe_unused]] int bad = 0;
#pragma unroll
    for (int k = 0; k <= 2 * SS_R; ++k) {
      const float w = g.w[k];
#pragma unroll
      for (int q = 0; q < 5; ++q) m[q] = fmaf(w, hz[q][r + k][c], m[q]);
      if constexpr (MASKED) bad += mk.hv[r + k][c];
    }
    if (gy < H && gx < W) {
      bool in_e = true;
      if constexpr (MASKED) {
        if (mk.tv[r + SS_R][c + SS_R]) {
          ll1 += fabsf(ta[r + SS_R][c + SS_R] - tb[r + SS_R][c + SS_R]);
          nv += 1;
        }
        in_e = bad == 0;
      }
      const float mu1 = m[0] + ca, mu2 = m[1] + cb;
      const float s1 = m[2] - m[0] * m[0], s2 = m[3] - m[1] * m[1], s12 = m[4] - m[0] * m[1];
      const float A1 = 2.f * mu1 * mu2 + C1, A2 = 2.f * s12 + C2;
      const float B1 = mu1 * mu1 + mu2 * mu2 + C1, B2 = s1 + s2 + C2;
      const float ssim = (A1 * A2) / (B1 * B2);
      if (in_e) {
        lss += ssim;
        ne += 1;
      }
      if (dmaps) {
        // S = A1*A2/(B1*B2) with s1 = s11 - mu1^2, s12 = s12raw - mu1*mu2
        const float inv = 1.f / (B1 * B2);
        const float dA1 = A2 * inv, dA2 = A1 * inv, dB1 = -ssim / B1, dB2 = -ssim / B2;
        const float d_s11 = dB2;                       // via s1
        const float d_s12 = 2.f * dA2;                 // via A2
        const float d_mu1 = dA1 * 2.f * mu2 + dB1 * 2.f * mu1 + dA2 * (-2.f * mu2) + dB2 * (-2.f * mu1);
        const long o = (long)img * 3 * H * W + (long)gy * W + gx;
        dmaps[o] = in_e ? d_mu1 : 0.f;
        dmaps[o + (long)H * W] = in_e ? d_s11 : 0.f;
        dmaps[o + 2L * H * W] = in_e ? d_s12 : 0.f;
      }
    }
  }
#pragma unroll
  for (int mm = 32; mm >= 1; mm >>= 1) {
    lss += __shfl_xor(lss, mm, 64);
    if constexpr (MASKED) {
      ll1 += __shfl_xor(ll1, mm, 64);
      nv += __shfl_xor(nv, mm, 64);
      ne += __shfl_xor(ne, mm, 64);
    }
  }
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = lss;
    if constexpr (MASKED) {
      red[1][tid >> 6] = ll1;
      mk.redi[0][tid >> 6] = nv; mk.redi[1][tid >> 6] = ne;
    }
  }
  __syncthreads();
  if (tid == 0) {
    out[blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    if constexpr (MASKED) {
      out[ntiles + blockIdx.x] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
      int* wi = (int*)out;
      wi[2 * ntiles + blockIdx.x] = mk.redi[0][0] + mk.redi[0][1] + mk.redi[0][2] + mk.redi[0][3];
      wi[3 * ntiles + blockIdx.x] = mk.redi[1][0] + mk.redi[1][1] + mk.redi[1][2] + mk.redi[1][3];
    }
  }
}

// adjoint of the reflect-boundary separable Gaussian applied to the three derivative maps, combined into
// dL/da = scale * ( G^T(d_mu1) + 2 a G^T(d_s11) + b G^T(d_s12) ) [+ l1_scale * sign(a - b)]
// G^T along one axis: g[j] = C[j] + C[-1-j] (j <= R-1) + C[2n-1-j] (j >= n-R), C[m] = sum_k w[k] D0[m-k+R], D0 = 0 outside.
__device__ __forceinline__ float adj_tap(const float* __restrict__ d, int n, int stride, int m, const GaussW& g) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k <= 2 * SS_R; ++k) {
    const int i = m - k + SS_R;
    if (i >= 0 && i < n) s = fmaf(g.w[k], d[(long)i * stride], s);
  }
  return s;
}
__device__ __forceinline__ float adj_axis(const float* __restrict__ d, int n, int stride, int j, const GaussW& g) {
  float s = adj_tap(d, n, stride, j, g);
  if (j <= SS_R - 1) s += adj_tap(d, n, stride, -1 - j, g);
  if (j >= n - SS_R) s += adj_tap(d, n, stride, 2 * n - 1 - j, g);
  return s;
}

// pass 1: rows (along W) of each derivative map -> tmp; pass 2: columns + combine, written once for both losses.
__global__ __launch_bounds__(256) void gauss_adj_rows_kernel(const float* __restrict__ d, float* __restrict__ tmp, int H,
                                                             int W, long total, GaussW g) {
  const long idx = blockIdx.x * 256L + threadIdx.x;  // over (plane, y, x)
  if (idx >= total) return;
  const int x = (int)(idx % W);
  const long row = idx / W;
  tmp[idx] = adj_axis(d + row * W, W, 1, x, g);
}
// MASKED: the two scales are read per image from the device (scales[2 * img], unmasked: the arguments), the upstream gradient is
// applied here (gup[0]; unmasked: by the caller) and exactly +0.0f is SELECTED at every invalid pixel (a NaN there, or a
// negative upstream gradient, cannot leave a mark).
template <bool MASKED>
__global__ __launch_bounds__(256) void loss_bwd_kernel(const float* __restrict__ tmp, const float* __restrict__ a,
                                                       const float* __restrict__ b, const unsigned char* __restrict__ valid,
                                                       const float* __restrict__ scales, const float* __restrict__ gup,
                                                       float* __restrict__ ga, int H, int W, long total, GaussW g,
                                                       float ssim_scale, float l1_scale) {
  const long idx = blockIdx.x * 256L + threadIdx.x;  // over (img, y, x)
  if (idx >= total) return;
  if constexpr (MASKED) {
    if (!px_valid(valid, b, idx)) {
      ga[idx] = 0.f;
      return;
    }
  }
  const int x = (int)(idx % W);
  const long t = idx / W;
  const int y = (int)(t % H);
  const long img = t / H;
  const long HW = (long)H * W;
  if constexpr (MASKED) { ssim_scale = scales[2 * img]; l1_scale = scales[2 * img + 1]; }
  const float* base = tmp + img * 3 * HW + x;
  const float g_mu = adj_axis(base, H, W, y, g);
  const float g_s11 = adj_axis(base + HW, H, W, y, g);
  const float g_s12 = adj_axis(base + 2 * HW, H, W, y, g);
  const float av = a[idx], bv = b[idx];
  float r = ssim_scale * (g_mu + 2.f * av * g_s11 + bv * g_s12);
  const float df = av - bv;
  r += l1_scale * (df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f));
  if constexpr (MASKED) r = r * gup[0];
  ga[idx] = r;
}

__global__ __launch_bounds__(256) void l1_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                         float* __restrict__ partial, long n) {
  __shared__ float red[4];
  float s = 0.f;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) s += fabsf(a[i] - b[i]);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out[0] = sum_i partial[i] in double, fixed order: 256 contiguous chunks summed in parallel, then the 256 chunk sums in
// index order (one thread walking ~10^4 dependent loads took 0.43 ms of a training step)
__global__ __launch_bounds__(256) void sum_partials_f64_kernel(const float* __restrict__ partial, int n, double scale,
                                                              double* __restrict__ out) {
  __shared__ double red[256];
  const int per = (n + 255) / 256;
  const int i0 = threadIdx.x * per, i1 = min(i0 + per, n);
  double s = 0.0;
  for (int i = i0; i < i1; ++i) s += (double)partial[i];
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int k = 0; k < 256; ++k) t += red[k];
    out[0] = t * scale;
  }
}

static GaussW make_gauss(double sd) {
  GaussW g;
  double w[2 * SS_R + 1], sum = 0.0;
  for (int k = -SS_R; k <= SS_R; ++k) { w[k + SS_R] = exp(-0.5 * k * k / (sd * sd)); sum += w[k + SS_R]; }
  for (int k = 0; k <= 2 * SS_R; ++k) g.w[k] = (float)(w[k] / sum);
  return g;
}

int postprocess_u8(const float* x, unsigned char* o, long n, hipStream_t stream) {
  hipLaunchKernelGGL(postprocess_u8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, o, n);
  return check_launch("postprocess_u8_kernel");
}

int postprocess_u8_f16(const void* x, unsigned char* o, long n, hipStream_t stream) {
  hipLaunchKernelGGL(postprocess_u8_f16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                     (const _Float16*)x, o, n);
  return check_launch("postprocess_u8_f16_kernel");
}

template <typename T>
static int masked_sqerr_launch(const char* what, const T* label, const T* out, long n, unsigned long long* acc,
                               hipStream_t stream) {
  hipError_t e = hipMemsetAsync(acc, 0, 2 * sizeof(unsigned long long), stream);
  if (e != hipSuccess) { set_error("%s: memset: %s", what, hipGetErrorString(e)); return CODON_ERR_LAUNCH; }
  const unsigned blocks = (unsigned)((n + 255) / 256 > 1024 ? 1024 : (n + 255) / 256);
  hipLaunchKernelGGL(masked_sqerr_kernel<T>, dim3(blocks), dim3(256), 0, stream, label, out, n, acc);
  return check_launch("masked_sqerr_kernel");
}
int masked_sqerr(const unsigned char* label, const unsigned char* out, long n, unsigned long long* acc, hipStream_t stream) {
  return masked_sqerr_launch("masked_rmse", label, out, n, acc, stream);
}
int masked_sqerr_u16(const unsigned short* label, const unsigned short* out, long n, unsigned long long* acc,
                     hipStream_t stream) {
  return masked_sqerr_launch("masked_sqerr_u16", label, out, n, acc, stream);
}

int postprocess_u16(const void* x, int dtype, int depth_max, unsigned short* o, long n, hipStream_t stream) {
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  const float levels = (float)depth_max;
  if (dtype == CODON_F16)
    hipLaunchKernelGGL(postprocess_u16_kernel<_Float16>, grid, block, 0, stream, (const _Float16*)x, o, levels, n);
  else if (dtype == CODON_BF16)
    hipLaunchKernelGGL(postprocess_u16_kernel<bf16_bits>, grid, block, 0, stream, (const bf16_bits*)x, o, levels, n);
  else
    hipLaunchKernelGGL(postprocess_u16_kernel<float>, grid, block, 0, stream, (const float*)x, o, levels, n);
  return check_launch("postprocess_u16_kernel");
}

struct SsimGrid { int tx, ty, nt; };
static SsimGrid ssim_grid(int B, int H, int W) {
  const int tx = (W + SS_T - 1) / SS_T, ty = (H + SS_T - 1) / SS_T;
  return {tx, ty, B * tx * ty};
}
int ssim_tiles(int B, int H, int W) { return ssim_grid(B, H, W).nt; }

int ssim_fwd(int B, int H, int W, const float* a, const float* b, float* partial, float* dmaps, double* value,
             hipStream_t stream) {
  const SsimGrid t = ssim_grid(B, H, W);
  hipLaunchKernelGGL(ssim_tile_kernel<false>, dim3(t.nt), dim3(256), 0, stream, a, b, (const unsigned char*)nullptr, partial,
                     dmaps, H, W, t.tx, t.ty, t.nt, make_gauss(1.5), 0.01f * 0.01f, 0.03f * 0.03f);
  int st = check_launch("ssim_tile_kernel<false>");
  if (st != CODON_OK) return st;
  hipLaunchKernelGGL(sum_partials_f64_kernel, dim3(1), dim3(256), 0, stream, partial, t.nt, 1.0 / ((double)B * H * W),
                     value);
  return check_launch("sum_partials_f64_kernel");
}

int l1_fwd(long n, const float* a, const float* b, float* partial, int nparts, double* value, hipStream_t stream) {
  hipLaunchKernelGGL(l1_partial_kernel, dim3(nparts), dim3(256), 0, stream, a, b, partial, n);
  int st = check_launch("l1_partial_kernel");
  if (st != CODON_OK) return st;
  hipLaunchKernelGGL(sum_partials_f64_kernel, dim3(1), dim3(256), 0, stream, partial, nparts, 1.0 / (double)n, value);
  return check_launch("sum_partials_f64_kernel");
}

// gauss_adj_rows_kernel, then loss_bwd_kernel<MASKED>
template <bool MASKED>
static int loss_bwd(int B, int H, int W, const float* a, const float* b, const unsigned char* valid, const float* dmaps,
                    const float* scales, const float* gup, float* tmp, float* ga, float ssim_scale, float l1_scale,
                    hipStream_t stream) {
  const GaussW g = make_gauss(1.5);
  const long t3 = (long)B * 3 * H * W, t1 = (long)B * H * W;
  hipLaunchKernelGGL(gauss_adj_rows_kernel, dim3((unsigned)((t3 + 255) / 256)), dim3(256), 0, stream, dmaps, tmp, H, W,
                     t3, g);
  int st = check_launch("gauss_adj_rows_kernel");
  if (st != CODON_OK) return st;
  hipLaunchKernelGGL(loss_bwd_kernel<MASKED>, dim3((unsigned)((t1 + 255) / 256)), dim3(256), 0, stream, tmp, a, b, valid,
                     scales, gup, ga, H, W, t1, g, ssim_scale, l1_scale);
  return check_launch(MASKED ? "loss_bwd_kernel<true>" : "loss_bwd_kernel<false>");
}

int ssim_l1_bwd(int B, int H, int W, const float* a, const float* b, const float* dmaps, float* tmp, float* ga,
                float ssim_scale, float l1_scale, hipStream_t stream) {
  return loss_bwd<false>(B, H, W, a, b, nullptr, dmaps, nullptr, nullptr, tmp, ga, ssim_scale, l1_scale, stream);
}

// ---- hole-aware L1 + SSIM: the finishing kernel and the two entries ---------------------------------------
// One workgroup; image b is folded by wave b % 4: each lane sums a contiguous run of the image's tiles in index order, lane 0
// then adds the runs in order -- float64 sums, integer counts, an order that depends on the image's size alone (an image's
// partials are the same in any batch).  counts[b] = {n_b, e_b}; per_image[b] = {L1_b, SSIM_b} (SSIM_b = 1 when e_b = 0);
// scales[b] = {-w_ssim / (B e_b), w_l1 / (B n_b)} rounded once to fp32 (0 for an empty set) for the backward;
// value = (1/B) sum_b [w_l1 L1_b + w_ssim (1 - SSIM_b)], added in the order of b.
__global__ __launch_bounds__(256) void masked_loss_finish_kernel(const float* __restrict__ ws, int B, int tpi, int ntiles,
                                                                 double w_l1, double w_ssim, long long* __restrict__ counts,
                                                                 double* per_image, float* __restrict__ scales,
                                                                 double* __restrict__ value) {
  __shared__ double rs[4][64], rl[4][64];
  __shared__ long long rn[4][64], re[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int* wi = (const int*)ws;
  const int per = (tpi + 63) / 64, runs = (tpi + per - 1) / per;
  for (int b0 = 0; b0 < B; b0 += 4) {
    const int b = b0 + wave;
    if (b < B) {
      const int i0 = b * tpi + lane * per, i1 = b * tpi + min(lane * per + per, tpi);
      double ss = 0.0, sl = 0.0;
      long long n = 0, e = 0;
      for (int i = i0; i < i1; ++i) {
        ss += (double)ws[i];
        sl += (double)ws[ntiles + i];
        n += wi[2 * ntiles + i];
        e += wi[3 * ntiles + i];
      }
      rs[wave][lane] = ss; rl[wave][lane] = sl; rn[wave][lane] = n; re[wave][lane] = e;
    }
    __syncthreads();
    if (b < B && lane == 0) {
      double ss = 0.0, sl = 0.0;
      long long n = 0, e = 0;
      for (int k = 0; k < runs; ++k) { ss += rs[wave][k]; sl += rl[wave][k]; n += rn[wave][k]; e += re[wave][k]; }
      counts[2 * b] = n;
      counts[2 * b + 1] = e;
      per_image[2 * b] = sl / (double)(n > 0 ? n : 1);
      per_image[2 * b + 1] = e > 0 ? ss / (double)e : 1.0;
      scales[2 * b] = e > 0 ? (float)(-w_ssim / ((double)B * (double)e)) : 0.f;
      scales[2 * b + 1] = n > 0 ? (float)(w_l1 / ((double)B * (double)n)) : 0.f;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {            // this thread's own stores and, through the barriers above, the other waves'
    double t = 0.0;
    for (int b = 0; b < B; ++b) t += w_l1 * per_image[2 * b] + w_ssim * (1.0 - per_image[2 * b + 1]);
    value[0] = t / (double)B;
  }
}

int masked_l1_ssim_fwd(int B, int H, int W, const float* a, const float* b, const unsigned char* valid, float* ws,
                       float* dmaps, double w_l1, double w_ssim, long long* counts, double* per_image, float* scales,
                       double* value, hipStream_t stream) {
  const SsimGrid t = ssim_grid(B, H, W);
  hipLaunchKernelGGL(ssim_tile_kernel<true>, dim3(t.nt), dim3(256), 0, stream, a, b, valid, ws, dmaps, H, W, t.tx, t.ty, t.nt,
                     make_gauss(1.5), 0.01f * 0.01f, 0.03f * 0.03f);
  int st = check_launch("ssim_tile_kernel<true>");
  if (st != CODON_OK) return st;
  hipLaunchKernelGGL(masked_loss_finish_kernel, dim3(1), dim3(256), 0, stream, ws, B, t.tx * t.ty, t.nt, w_l1, w_ssim, counts,
                     per_image, scales, value);
  return check_launch("masked_loss_finish_kernel");
}

int masked_l1_ssim_bwd(int B, int H, int W, const float* a, const float* b, const unsigned char* valid, const float* dmaps,
                       const float* scales, const float* gup, float* tmp, float* ga, hipStream_t stream) {
  return loss_bwd<true>(B, H, W, a, b, valid, dmaps, scales, gup, tmp, ga, 0.f, 0.f, stream);
}

}  // namespace codon
