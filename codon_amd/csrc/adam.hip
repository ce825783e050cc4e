// One optimizer step of Adam over the 44 used parameter tensors in ONE launch (round 6).  The reference ships no training code
// (SURVEY.md D8); the bench's training step (BASELINE.json configs[2]) used torch.optim.Adam -- five ATen multi_tensor_apply
// launches inside the timed region.  The gradients already sit in codon_amd.dist.GradSync's flat all-reduce buffer, in the
// parameters' order; the two moment buffers are flat alike, so the step is elementwise over (tensor, offset):
//   g  = grad (+ weight_decay * p)
//   m  = m + (1 - beta1) * (g - m)                      (torch: exp_avg.lerp_(grad, 1 - beta1))
//   v  = beta2 * v + (1 - beta2) * g * g                (torch: exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2))
//   p -= (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
// -- torch.optim.Adam's arithmetic (amsgrad = False, maximize = False), to fp32 rounding (tests/test_gpu_reduce.py).
#include <math.h>

#include "codon_common.h"
#include "kernels.h"

namespace codon {

struct AdamArgs {
  float* p[CODON_ADAM_MAX];
  unsigned start[CODON_ADAM_MAX + 1];        // tensor t -> flat elements [start[t], start[t + 1])
  int first_block[CODON_ADAM_MAX + 1];       // ... -> workgroups [first_block[t], first_block[t + 1]), 1024 elements each
  int n;
  const float* g;
  float* m;
  float* v;
  float step_size, w1, beta2, one_minus_beta2, inv_sqrt_bc2, eps, wd;
};
static_assert(sizeof(AdamArgs) <= CODON_KERNARG_LIMIT, "passed by value as a kernel argument");

__global__ __launch_bounds__(256) void adam_step_kernel(const AdamArgs a) {
  int t = 0;
  while (t + 1 < a.n && (int)blockIdx.x >= a.first_block[t + 1]) ++t;        // block-uniform
  const unsigned cnt = a.start[t + 1] - a.start[t];
  const unsigned base = ((unsigned)blockIdx.x - (unsigned)a.first_block[t]) * 1024u;
  float* const p = a.p[t];
  const float* const g = a.g + a.start[t];
  float* const m = a.m + a.start[t];
  float* const v = a.v + a.start[t];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned i = base + k * 256u + threadIdx.x;
    if (i >= cnt) break;
    const float pi = p[i];
    const float gi = a.wd != 0.f ? fmaf(a.wd, pi, g[i]) : g[i];
    const float mi = m[i] + a.w1 * (gi - m[i]);
    const float vi = a.beta2 * v[i] + a.one_minus_beta2 * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] = pi - a.step_size * (mi / (sqrtf(vi) * a.inv_sqrt_bc2 + a.eps));
  }
}

// The descriptor and the hyper-parameters as kernel arguments, shared by the plain and the guarded step (`what` names the caller
// in the refusals).
static int adam_args(AdamArgs& a, const char* what, const codon_adam_desc* d, const float* grad, float* exp_avg, float* exp_avg_sq,
                     float lr, float beta1, float beta2, float eps, float weight_decay, int step) {
  CODON_REQUIRE(d->n >= 1 && d->n <= CODON_ADAM_MAX, CODON_ERR_BAD_ARG, "%s: %d tensors (1..%d)", what, d->n, CODON_ADAM_MAX);
  CODON_REQUIRE(step >= 1 && lr >= 0.f && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f,
                CODON_ERR_BAD_ARG, "%s: step %d lr %g betas (%g, %g) eps %g", what, step, lr, beta1, beta2, eps);
  a.n = d->n;
  a.start[0] = 0;
  a.first_block[0] = 0;
  for (int t = 0; t < d->n; ++t) {
    CODON_REQUIRE(d->param[t] && d->count[t] > 0 && ((uintptr_t)d->param[t] % 4) == 0, CODON_ERR_BAD_ARG,
                  "%s: tensor %d: null, empty or misaligned", what, t);
    const long nb = (d->count[t] + 1023) / 1024;
    CODON_REQUIRE((long)a.start[t] + d->count[t] < (1L << 32) && (long)a.first_block[t] + nb < (1L << 31), CODON_ERR_UNSUPPORTED,
                  "%s: too many elements", what);
    a.p[t] = (float*)d->param[t];
    a.start[t + 1] = a.start[t] + (unsigned)d->count[t];
    a.first_block[t + 1] = a.first_block[t] + (int)nb;
  }
  for (int t = d->n; t < CODON_ADAM_MAX; ++t) { a.p[t] = nullptr; a.start[t + 1] = a.start[d->n]; a.first_block[t + 1] = a.first_block[d->n]; }
  a.g = grad; a.m = exp_avg; a.v = exp_avg_sq;
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  a.step_size = (float)((double)lr / bc1);
  a.w1 = 1.f - beta1;
  a.beta2 = beta2;
  a.one_minus_beta2 = 1.f - beta2;
  a.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  a.eps = eps;
  a.wd = weight_decay;
  return CODON_OK;
}

int adam_step(const codon_adam_desc* d, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2,
              float eps, float weight_decay, int step, hipStream_t stream) {
  AdamArgs a;
  const int st = adam_args(a, "adam_step", d, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step);
  if (st != CODON_OK) return st;
  hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)a.first_block[d->n]), dim3(256), 0, stream, a);
  return check_launch("adam_step_kernel");
}

// ---- the guarded step: global-norm clipping, non-finite skipping, EMA ------------------------------------------------------
// Two launches on one stream and a small device state block (GN_STATE_WORDS 8-byte words, zeroed once by the caller):
//   [0] last_norm (double)   [1] applied   [2] skipped   [3] clipped (64-bit counts)
//   [4 .. 4 + GN_BLOCKS)             per-workgroup sum of g * g, accumulated in double (the product of two floats is exact there)
//   [4 + GN_BLOCKS .. 4 + 2 GN_BLOCKS)   per-workgroup count of non-finite elements
// grad_norm_kernel fills the partials: fixed grid, fixed element -> thread mapping, fixed fold order, no atomics.  Every wave of
// adam_step_guarded_kernel folds the GN_BLOCKS partials again for itself (2 KiB out of L2, the same order everywhere, so every
// workgroup -- and every rank, from identical all-reduced gradients -- reaches the same clip / skip decision); no arrival
// counter exists that a killed launch could leave stale.  The kernel boundary orders the two launches.
constexpr int GN_BLOCKS = 256, GN_THREADS = 256, GN_STATE_WORDS = 4 + 2 * GN_BLOCKS;

// xor butterfly: a + b == b + a bit for bit, so all 64 lanes end with the same value.
__device__ __forceinline__ double wave_sum_all(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ unsigned wave_sum_all(unsigned v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ void gn_take(float x, double& acc, unsigned& bad) {
  acc += (double)x * (double)x;
  bad += (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
}

__global__ __launch_bounds__(GN_THREADS) void grad_norm_kernel(const float* __restrict__ g, unsigned n, double* __restrict__ state) {
  __shared__ double s_acc[GN_THREADS / 64];
  __shared__ unsigned s_bad[GN_THREADS / 64];
  const unsigned tid = threadIdx.x, nvec = n / 4u;
  const f32x4* const g4 = (const f32x4*)g;
  double acc = 0.0;
  unsigned bad = 0;
  constexpr unsigned SWEEP = GN_BLOCKS * GN_THREADS;
  for (unsigned q = blockIdx.x * GN_THREADS + tid; q < nvec; q += 4u * SWEEP) {     // four 16-byte loads in flight
    f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const unsigned qu = q + u * SWEEP;
      v[u] = qu < nvec ? g4[qu] : f32x4{0.f, 0.f, 0.f, 0.f};      // plain loads: the step kernel reads g again, from L2
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      gn_take(v[u].x, acc, bad);
      gn_take(v[u].y, acc, bad);
      gn_take(v[u].z, acc, bad);
      gn_take(v[u].w, acc, bad);
    }
  }
  if (blockIdx.x == GN_BLOCKS - 1 && tid == GN_THREADS - 1)
    for (unsigned i = 4u * nvec; i < n; ++i) gn_take(g[i], acc, bad);                // the scalar tail (n % 4 elements)
  acc = wave_sum_all(acc);
  bad = wave_sum_all(bad);
  if ((tid & 63u) == 0) { s_acc[tid >> 6] = acc; s_bad[tid >> 6] = bad; }
  __syncthreads();
  if (tid == 0) {
    double s = s_acc[0];
    unsigned b = s_bad[0];
    for (int k = 1; k < GN_THREADS / 64; ++k) { s += s_acc[k]; b += s_bad[k]; }
    state[4 + blockIdx.x] = s;
    ((unsigned long long*)state)[4 + GN_BLOCKS + blockIdx.x] = b;
  }
}

struct GuardArgs {
  double* state;
  float* ema;                 // flat, the gradient's layout; null = no EMA
  double max_norm;            // +inf = no clipping
  float w_ema;                // 1 - decay
  int skip_nonfinite;
};
static_assert(sizeof(AdamArgs) + sizeof(GuardArgs) <= CODON_KERNARG_LIMIT, "both passed by value as kernel arguments");

__global__ __launch_bounds__(256) void adam_step_guarded_kernel(const AdamArgs a, const GuardArgs q) {
  // block-uniform head: fold the partials (every wave for itself, same order), decide skip and clip
  const unsigned lane = threadIdx.x & 63u;
  double sumsq = 0.0;
  unsigned bad = 0;
#pragma unroll
  for (int k = 0; k < GN_BLOCKS / 64; ++k) {
    sumsq += q.state[4 + k * 64 + lane];
    bad += (unsigned)((const unsigned long long*)q.state)[4 + GN_BLOCKS + k * 64 + lane];
  }
  sumsq = wave_sum_all(sumsq);
  bad = wave_sum_all(bad);
  const double norm = sqrt(sumsq);
  const bool skip = q.skip_nonfinite && bad != 0;
  // torch.nn.utils.clip_grad_norm_: coef = clamp(max_norm / (norm + 1e-6), max = 1), in double, rounded once.  A NaN quotient
  // stays NaN (the comparison is false): nothing is hidden when skipping is off.
  const double c = q.max_norm / (norm + 1e-6);
  const float coef = (isinf(q.max_norm) || c >= 1.0) ? 1.f : (float)c;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    unsigned long long* const ctr = (unsigned long long*)q.state;
    q.state[0] = norm;
    if (skip) {
      ctr[2] += 1;
    } else {
      ctr[1] += 1;
      if (coef < 1.f) ctr[3] += 1;
    }
  }
  if (skip) return;                                                              // p, m, v and the EMA keep their bits

  int t = 0;
  while (t + 1 < a.n && (int)blockIdx.x >= a.first_block[t + 1]) ++t;        // block-uniform
  const unsigned cnt = a.start[t + 1] - a.start[t];
  const unsigned base = ((unsigned)blockIdx.x - (unsigned)a.first_block[t]) * 1024u;
  float* const p = a.p[t];
  const float* const g = a.g + a.start[t];
  float* const m = a.m + a.start[t];
  float* const v = a.v + a.start[t];
  float* const ema = q.ema ? q.ema + a.start[t] : nullptr;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned i = base + k * 256u + threadIdx.x;
    if (i >= cnt) break;
    const float pi = p[i];
    float cg = coef * g[i];
    asm volatile("" : "+v"(cg));      // the product is rounded on its own: no contraction into the arithmetic below
    const float gi = a.wd != 0.f ? fmaf(a.wd, pi, cg) : cg;
    // adam_step_kernel's expressions with the contractions hipcc picks for them written out (left to itself it fuses `vi` the
    // other way round here): coef == 1 must give that kernel's bits (tests/test_gpu_guarded_step.py pins it)
    const float mi = fmaf(a.w1, gi - m[i], m[i]);
    const float b2v = a.beta2 * v[i], wg = a.one_minus_beta2 * gi;
    const float vi = fmaf(gi, wg, b2v);
    m[i] = mi;
    v[i] = vi;
    const float pn = fmaf(-a.step_size, mi / fmaf(sqrtf(vi), a.inv_sqrt_bc2, a.eps), pi);
    p[i] = pn;
    if (ema) ema[i] = fmaf(q.w_ema, pn - ema[i], ema[i]);
  }
}

size_t grad_norm_workspace_bytes() { return (size_t)GN_STATE_WORDS * sizeof(double); }

int grad_norm(const float* grad, long n, void* state, hipStream_t stream) {
  CODON_REQUIRE(n >= 1 && n < (1L << 32), CODON_ERR_BAD_ARG, "grad_norm: %ld elements (1..2^32 - 1)", n);
  CODON_REQUIRE(((uintptr_t)grad % 16) == 0 && ((uintptr_t)state % 8) == 0, CODON_ERR_BAD_ARG,
                "grad_norm: the gradient must be 16-byte aligned, the state block 8-byte aligned");
  hipLaunchKernelGGL(grad_norm_kernel, dim3(GN_BLOCKS), dim3(GN_THREADS), 0, stream, grad, (unsigned)n, (double*)state);
  return check_launch("grad_norm_kernel");
}

int adam_step_guarded(const codon_adam_desc* d, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, void* state,
                      float lr, float beta1, float beta2, float eps, float weight_decay, int step, double max_norm,
                      int skip_nonfinite, double ema_decay, hipStream_t stream) {
  CODON_REQUIRE(max_norm > 0.0, CODON_ERR_BAD_ARG, "adam_step_guarded: max_norm %g (> 0, +inf = no clipping)", max_norm);
  CODON_REQUIRE(!ema || (ema_decay >= 0.0 && ema_decay < 1.0), CODON_ERR_BAD_ARG, "adam_step_guarded: EMA decay %g (0 <= decay < 1)",
                ema_decay);
  CODON_REQUIRE(((uintptr_t)state % 8) == 0 && ((uintptr_t)ema % 4) == 0, CODON_ERR_BAD_ARG,
                "adam_step_guarded: misaligned state block or EMA buffer");
  AdamArgs a;
  const int st = adam_args(a, "adam_step_guarded", d, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step);
  if (st != CODON_OK) return st;
  GuardArgs q;
  q.state = (double*)state;
  q.ema = ema;
  q.max_norm = max_norm;
  q.w_ema = ema ? (float)(1.0 - ema_decay) : 0.f;
  q.skip_nonfinite = skip_nonfinite != 0;
  hipLaunchKernelGGL(adam_step_guarded_kernel, dim3((unsigned)a.first_block[d->n]), dim3(256), 0, stream, a, q);
  return check_launch("adam_step_guarded_kernel");
}

}  // namespace codon
