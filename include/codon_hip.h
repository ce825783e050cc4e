/* codon_hip.h -- C ABI of libcodon_hip.so: the MI355X (gfx950) kernels behind CODONNet.
 *
 * The reference (619862306/CODON) is eager PyTorch with no native layer; what it calls for
 * this path are stock ATen ops from nn.Module.forward.  Each entry point below replaces the
 * ATen op sequence at the cited reference lines.  All pointers are DEVICE pointers (descriptors and the three
 * arguments of the host-only known-answer entry of the sensor model's generator excepted); all work
 * is enqueued on the caller's stream; nothing allocates, synchronises or throws.  Every
 * function returns CODON_OK (0) or a negative codon_status; codon_last_error_string() gives
 * the detail for the calling thread.
 *
 * Activation layout of the 64/128-channel tensors:
 *   CODON_F32           : NCHW, contiguous                         element (b,c,h,w) at ((b*C + c)*H + h)*W + w
 *   CODON_BF16 / _F16   : channel-blocked [B][C/8][H][W][8]        element (b,c,h,w) at (((b*C/8 + c/8)*H + h)*W + w)*8 + c%8
 *                         (one 16-byte vector = 8 consecutive channels of a pixel: the MFMA B operand, codon_amd/csrc/c8.h)
 * 1-channel maps (x, y, the output, gates, pooled maps) are fp32 NCHW in every mode: what crosses the reference's
 * nn.Module boundary (CODON_x4.py:66-68,130-132) never changes layout.  A tensor argument may be a channel slice of a
 * wider buffer: (ctotal, coff) describe a buffer of ctotal channels of which channels [coff, coff+C) are read / written
 * (16-bit: coff, C and ctotal multiples of 8, i.e. whole 8-channel planes) -- this is how the torch.cat calls of the
 * reference (CODON_x4.py:79,80,85,119,125) disappear.
 */
#ifndef CODON_HIP_H
#define CODON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CODON_ABI_VERSION 1

typedef void* codon_stream_t; /* hipStream_t */

typedef enum codon_status {
  CODON_OK = 0,
  CODON_ERR_BAD_ARG = -1,     /* null pointer, non-positive size, misaligned buffer */
  CODON_ERR_UNSUPPORTED = -2, /* shape / dtype combination with no kernel */
  CODON_ERR_LAUNCH = -3       /* HIP reported a launch failure */
} codon_status;

/* dtype of the 64/128-channel activations (and of the packed conv weights): storage + MFMA operand type;
 * accumulation is always fp32.  CODON_F16 is the reference script's own inference precision
 * (model.cuda().half(), /root/reference/CODON_X4/test.py:52,122-123).  A 16-bit conv stores its fp32 result rounded once to
 * nearest even; fp16 subnormal operands and results are kept, as the reference's CPU .half() keeps them. */
typedef enum codon_dtype { CODON_F32 = 0, CODON_BF16 = 1, CODON_F16 = 2 } codon_dtype;

enum {
  CODON_CONV_RELU = 1,         /* y = max(conv, 0)          (self.relu(self.convN(..)))      */
  CODON_CONV_ADD_RESIDUAL = 2, /* y = conv + residual       (torch.add(out_fuse, fuse) :128) */
  CODON_CONV_ACCUM_OUT = 4,    /* y += conv                 (backward: grads that fan in)    */
  CODON_CONV_MASK_RELU = 8,    /* y = residual > 0 ? conv : 0   (backward through a ReLU whose OUTPUT is
                                  passed in the residual slot; applied before ACCUM_OUT's add)      */
  CODON_CONV_F16X3 = 16,       /* OPT-IN, fp32 tensors, k in {3,5}: split-precision evaluation -- operands split
                                  into fp16 hi+lo, three f16 MFMAs per product, fp32 accumulate (~2^-22 per
                                  product; |activations| < 65504).  w_packed must come from CODON_PACK_FWD_F16X3. */
  CODON_CONV_MASK_SUM = 32     /* with MASK_RELU | ACCUM_OUT: the mask applies to the SUM, y = residual > 0 ? conv + y : 0
                                  (the last gradient that fans into a ReLU output: no separate mask pass)          */
};

enum { CODON_PACK_FWD = 0, CODON_PACK_DGRAD = 1, CODON_PACK_FWD_F16X3 = 2, CODON_PACK_CHAIN1X1 = 3,
       CODON_PACK_CHAIN1X1_F16X3 = 4 };

/* One stride-1, "same"-padded, bias-free 2-D convolution (every nn.Conv2d of
 * CODON_X4/CODON_x4.py:24-47 has stride 1, padding k//2, bias=False). */
typedef struct codon_conv_desc {
  int32_t batch, height, width;
  int32_t cin, cout, ksize;   /* ksize in {1,3,5}; (cin,cout) in {64,128}x{64,128} */
  int32_t x_ctotal, x_coff;   /* input  buffer (B, x_ctotal, H, W), channels [x_coff, x_coff+cin)  */
  int32_t y_ctotal, y_coff;   /* output buffer (B, y_ctotal, H, W), channels [y_coff, y_coff+cout) */
  int32_t r_ctotal, r_coff;   /* residual buffer, used with CODON_CONV_ADD_RESIDUAL                */
  int32_t flags;              /* CODON_CONV_* */
  int32_t dtype;              /* codon_dtype of x, y, residual and the packed weights              */
} codon_conv_desc;

/* A 64-channel activation that may be a channel slice of a wider buffer.  fp32 (NCHW): element (b, c, h, w) lives at
 * data[((b*ctotal + coff + c)*H + h)*W + w]; 16-bit (channel-blocked): at
 * data[(((b*ctotal/8 + (coff + c)/8)*H + h)*W + w)*8 + (coff + c)%8]. */
typedef struct codon_tensor {
  void* data;
  int32_t ctotal, coff;
} codon_tensor;

int codon_abi_version(void);
const char* codon_last_error_string(void);
/* first 32 hex digits of sha256 over the sources this binary was built from (codon_amd/csrc/{*.hip,*.h} in byte-sorted
 * name order, then include/codon_hip.h, contents concatenated): lets a host detect a stale binary. */
const char* codon_build_source_hash(void);

/* ---- MFMA implicit-GEMM convolutions (99.9 % of the FLOPs) -------------------------------
 * replaces: self.relu(self.conv{1..11}(..)), self.conv_input(_c), self.confuse(_c/_fuse)
 *           /root/reference/CODON_X4/CODON_x4.py:69,72,75-78,81-84,120,123-129 */

/* bytes of the packed (K-major, stage-contiguous) weight image the conv kernels read */
size_t codon_conv_packed_weight_bytes(int32_t cout, int32_t cin, int32_t ksize, int32_t dtype);

/* w_oihw: (cout, cin, k, k) fp32 contiguous (the nn.Conv2d.weight layout).
 * mode CODON_PACK_FWD  : pack for y = conv(x, w)
 * mode CODON_PACK_DGRAD: pack the spatially flipped, in/out-transposed filter so that the SAME
 *                        forward kernel computes dL/dx = conv(dL/dy, w') (cin/cout swap roles).
 * mode CODON_PACK_CHAIN1X1: (64,128,1,1) only -- the register-chained 1x1 of codon_conv_chain1x1_fwd;
 *      CODON_PACK_CHAIN1X1_F16X3 the same for a CODON_CONV_F16X3 call (fp32 tensors). */
int codon_conv_pack_weight(const float* w_oihw, void* w_packed, int32_t cout, int32_t cin,
                           int32_t ksize, int32_t mode, int32_t dtype, codon_stream_t stream);

int codon_conv2d_fwd(const codon_conv_desc* d, const void* x, const void* w_packed, void* y,
                     const void* residual, codon_stream_t stream);

/* 16-bit tensors, conv5x5 64 -> 64 (training, round 4):  y (+)= conv(x)  exactly as codon_conv2d_fwd with flags 0 /
 * CODON_CONV_ACCUM_OUT, and in the same epilogue   sum += y   with y the value AS STORED (so the result equals a separate
 * pass that reads y back, bit for bit).  d->r_ctotal / r_coff describe `sum` (READ-WRITE).  Used for the LAST input
 * gradient that fans into a block's dL/d(out): the running dL/d(inputs) of the network's long skip connection
 * (`out*g + inputs`, /root/reference/CODON_X4/CODON_x4.py:90-91,117-118) takes it there instead of in a pass of its own
 * (codon_cac_bwd_reduce_acc with accumulate_in = 2). */
int codon_conv2d_sum_into_fwd(const codon_conv_desc* d, const void* x, const void* w_packed, void* y, void* sum,
                              codon_stream_t stream);

/* conv5x5(128 -> 128) + ReLU and the 1x1 conv (128 -> 64) [+ residual] that consumes it, in ONE launch:
 *   confuse(relu(conv3(.))) / confuse_c(relu(conv6(.))) / torch.add(confuse_fuse(relu(conv10(.))), fuse)
 *   /root/reference/CODON_X4/CODON_x4.py:81-84,125-128.
 * The MFMA accumulator layout of the 5x5 tile is already a B operand of the 1x1's MFMAs, so the 1x1 runs from
 * registers and the 128-channel intermediate need not reach HBM: y may be NULL (inference); when given (training
 * saves it) it receives relu(conv5x5) exactly as codon_conv2d_fwd would write it.
 * d: the 5x5 conv (flags: CODON_CONV_RELU [| CODON_CONV_F16X3]; r_* ignored).  w_chain: the (64,128,1,1) weight
 * packed with mode CODON_PACK_CHAIN1X1 (CODON_PACK_CHAIN1X1_F16X3 under CODON_CONV_F16X3; same dtype; 64*128 elements).  out / residual: 64-channel slices of
 * d->dtype; residual may be NULL. */
int codon_conv_chain1x1_fwd(const codon_conv_desc* d, const void* x, const void* w_packed, void* y,
                            const void* w_chain, const codon_tensor* out, const codon_tensor* residual,
                            codon_stream_t stream);

/* codon_conv_chain1x1_fwd that ALSO produces the CAC statistics of its 64 output channels from the
 * epilogue (the values as stored, i.e. 16-bit tensors: rounded to 16 bits), instead of a separate pass over the tensor
 * (codon_cac_stats_fwd; F.avg_pool2d / F.max_pool2d / ChannelPool, /root/reference/CODON_X4/CAC_module.py:43,47,81):
 *   stats_pool     (B,2,H,W) fp32 : per pixel { max, SUM } over THIS stream's 64 channels
 *   stats_partials (B, codon_cac_fused_tiles(H,W), 128, 2) fp32 : per 8 x 32 conv tile, per channel { sum, max } written at
 *                  channels [stats_choff, stats_choff + 64): 0 = colour stream (Fcat channels 0..63), 64 = depth.  Every
 *                  16-bit launch runs on 8 x 32 tiles whatever the batch, so the partials of an image do not depend on it.
 * Two launches (one per stream) fill one partials buffer.  Then
 *   codon_cac_fused_finish   : folds the tiles into CODON_CAC_FOLDS rows in fixed order (`folded`: (B, CODON_CAC_FOLDS, 128, 2)
 *                              scratch) and combines the two stream maps into pooled (B,2,H,W) = { max, mean over 128 }
 *   codon_cac_gate_folded_fwd: codon_cac_gate_fwd over the folded rows.
 * Max pools are exact; sums are added in a different (fixed) order than codon_cac_stats_fwd adds them. */
#define CODON_CAC_FOLDS 16
int codon_conv_chain1x1_stats_fwd(const codon_conv_desc* d, const void* x, const void* w_packed, void* y,
                                  const void* w_chain, const codon_tensor* out, const codon_tensor* residual,
                                  float* stats_pool, float* stats_partials, int32_t stats_choff, codon_stream_t stream);
int32_t codon_cac_fused_tiles(int32_t height, int32_t width);
/* Rows per image of stats_partials for tensors of `dtype`: 16-bit = codon_cac_fused_tiles; fp32 (round 6) = one row per STRIP
 * of 32 pixels of one image row, height * ceil(width / 32).  fp32 strips are summed by one fixed in-wave tree and folded in
 * index order by codon_cac_tail_fwd, so the statistics -- and with them the gates and the image -- do not depend on which
 * tiling (8 x 32, 4 x 32, 2 x 32 cout-split: codon_conv_tiling_f32) the launch took, i.e. not on the batch an image arrives in.
 * fp32: no residual; the model uses it for images of at most 32 768 pixels (by height x width only), where the separate
 * statistics pass cost 22 us of a 2.2 ms forward (BASELINE configs[0]). */
int32_t codon_cac_fused_parts(int32_t height, int32_t width, int32_t dtype);
int codon_cac_fused_finish(int32_t batch, int32_t height, int32_t width, const float* partials, const float* pool_c,
                           const float* pool_d, float* folded, float* pooled, codon_stream_t stream);
int codon_cac_gate_folded_fwd(int32_t batch, int32_t height, int32_t width, const float* folded, const float* w1,
                              const float* b1, const float* w2, const float* b2, float* ch, float* pools_out,
                              codon_stream_t stream);
/* The whole gate of a block in ONE launch (replaces codon_cac_fused_finish + codon_cac_gate_folded_fwd + codon_cac_spatial_fwd,
 * or codon_cac_gate_fwd + codon_cac_spatial_fwd behind codon_cac_stats_fwd): at one image per call -- the reference script's
 * own calling pattern, /root/reference/CODON_X4/test.py:116-125 -- these were 20 dependent few-microsecond launches per
 * forward.  partials: (B, ntiles, 128, 2) per-tile { sum, max }; ntiles = codon_cac_fused_tiles (pool_c / pool_d given: the
 * two per-stream maps of codon_conv_chain1x1_stats_fwd, combined on the fly; pooled (B,2,H,W) is WRITTEN when non-null) or
 * codon_cac_stats_tiles (pool_c = pool_d = NULL: pooled is READ, as codon_cac_stats_fwd left it).  folded: (B,
 * CODON_CAC_FOLDS, 128, 2) scratch; counters: B int32, zero on entry and on exit.  Outputs as the calls it replaces: ch
 * (B,64), sp (B,1,H,W), pools_out (B,2,128) or NULL.  16-bit path: bit for bit the results of the three calls; fp32 path:
 * the pools are folded before they are finished (codon_cac_gate_fwd adds the tiles serially), identical for <= CODON_CAC_FOLDS tiles. */
int codon_cac_tail_fwd(int32_t batch, int32_t height, int32_t width, int32_t ntiles, const float* partials,
                       const float* pool_c, const float* pool_d, float* pooled, float* folded, int32_t* counters,
                       const float* w1, const float* b1, const float* w2, const float* b2, const float* w_spatial, float* ch,
                       float* pools_out, float* sp, codon_stream_t stream);

/* Two independent convs of one shape as ONE launch.  The depth and the colour stream of a block do not meet before the CAC
 * gate (/root/reference/CODON_X4/CODON_x4.py:75-84: conv2 | conv4, conv1 | conv5, conv3 + confuse | conv6 + confuse_c), and
 * at one image per call (test.py:116-125) each of their launches covers the chip only about once: issued as one grid of
 * twice the tiles they fill each other's last round.  Between codon_conv_pair_begin() and codon_conv_pair_end(stream), on
 * the calling host thread, up to two calls of codon_conv2d_fwd / codon_conv_chain1x1[_stats]_fwd / codon_conv2d_gated[_emit]_fwd
 * are validated as usual but HELD BACK; pair_end issues them -- as one launch when both run the same kernel variant on the
 * same grid (same shapes, dtype and epilogue kind), else one after the other -- and returns the number of launches issued
 * (>= 0) or a negative codon_status.  The two calls must be independent (neither reads what the other writes).  Calls the
 * pair form does not cover (1x1 convs, the resident-filter conv3x3 of large grids, fp32 convs that are not small-grid)
 * launch at once, as without the bracket.  Same arithmetic per tile: results are bit-identical to separate launches.
 * Streams: a held call keeps the stream it was given.  The one-grid form is taken only when both held calls named the
 * stream pair_end is given; otherwise each is launched alone on ITS OWN stream (so work ordered against those streams stays
 * ordered).  A third call the pair form covers inside one bracket is refused with CODON_ERR_BAD_ARG (launching it at once
 * would put it ahead of the two held ones); the bracket stays open and pair_end still issues the first two. */
int codon_conv_pair_begin(void);
int codon_conv_pair_end(codon_stream_t stream);

/* Which tiling the fp32 conv entry points give a launch of this shape -- the launch rule itself, the one function the
 * launchers ask, called without a launch (host arithmetic, no GPU call): diagnostics, and the CPU tests that pin the rule.  `chained`: codon_conv_chain1x1_fwd
 * (conv5x5 128->128 + 1x1) instead of codon_conv2d_fwd; `in_pair`: as inside a codon_conv_pair_begin / _end bracket.
 * A launch of a few rounds of workgroups is priced by its rounds (256 CUs, two 4-wave workgroups per CU):
 * 8 x 32 pixel tiles two per CU, 4 x 32 two per CU, 4 x 32 one per CU, or (small launches) 2 x 32 with the couts split
 * over the waves.  Every tiling computes every output pixel with the same fma chain: results do not depend on it.
 * Replaces nothing in the reference (eager PyTorch leaves tiling to cuDNN: /root/reference/CODON_X4/CODON_x4.py:75-84). */
#define CODON_TILING_8X32 0
#define CODON_TILING_4X32 1
#define CODON_TILING_4X32_SOLO 2
#define CODON_TILING_2X32_COUT_SPLIT 3
int codon_conv_tiling_f32(const codon_conv_desc* desc, int chained, int in_pair);

/* Which form codon_conv2d_fwd gives a 16-bit (CODON_BF16 / CODON_F16) conv of this shape, asked of the same rule the launch
 * follows (nothing is launched): diagnostics, and the tests whose premise is the form.  The plain conv3x3 64->64 of a LARGE
 * launch runs as one resident generation of 16-wave workgroups, each holding the whole packed filter in LDS and walking
 * 32 x 32 pixel tiles: taken when the grid has at least 8 such tiles per resident workgroup, the number of resident
 * workgroups coming from the current device's occupancy query (no usable device: staged, as the launch would be).  Every
 * other shape, and every smaller launch, is staged: one 8 x 32 (5x5 64->64: 16 x 32) tile per workgroup.  Same MFMAs on
 * the same operands in the same order per pixel: results do not depend on the form.  The flags and slices of d are not
 * looked at.  Returns CODON_C8_FORM_STAGED / _RESIDENT, or CODON_ERR_UNSUPPORTED for an fp32 dtype or a (k, cin, cout)
 * with no 16-bit kernel.  Replaces nothing in the reference (eager PyTorch leaves the kernel choice to cuDNN,
 * CODON_x4.py:75-84). */
#define CODON_C8_FORM_STAGED 0
#define CODON_C8_FORM_RESIDENT 1
int codon_conv_form_c8(const codon_conv_desc* desc);

/* Which form the stem / head stencils, the one-channel weight gradient and the CAC gate passes give a launch of this size:
 * the host rules the launchers themselves switch on (csrc/launch_rules.h, px8.h, cac_stats_tiles), called without a launch
 * (host arithmetic, no GPU call): diagnostics, and the tests that place their probes on a form's seams (tests/forms.py).
 * `aligned`: every pointer and slice of the launch starts on 16 bytes (the launcher finds that out from its own arguments).
 * Fields an op does not have are 0.
 *   CODON_FORM_STEM          fp32: vec (pixels per thread, 1 or 4), cols 0 (a thread index walks the flattened rows: no
 *                            segments); 16-bit: vec 2, cols 128 (columns of one row per wave)
 *   CODON_FORM_HEAD          fp32: vec, rows, depth = VEC, R, DEPTH of the kernel, cols = 64 vec (output columns per wave);
 *                            16-bit: rows (4 or 8), cols 62
 *   CODON_FORM_CAC_STATS     tile (pixels per tile: 256 for small images, else 2048), tiles (per image, codon_cac_stats_tiles),
 *                            vector (fp32, 2048-pixel form: 1 = 16-byte accesses, 0 = scalar)
 *   CODON_FORM_CAC_BWD_GATE  tile (2048), tiles (per image, codon_cac_bwd_tiles), slices (of the tile range the gate kernel
 *                            walks), per (tiles per slice)
 *   CODON_FORM_CAC_SPATIAL_FWD / _BWD   tile (edge of the square pixel tile of the forward / the backward kernel)
 *   CODON_FORM_CONV1CH_WGRAD rows (per band), cols (pixels per chunk)
 * The CODON_TUNE lab override of the head's band height is not reported.  CODON_ERR_BAD_ARG for a NULL out, an unknown op
 * or dtype or a non-positive size.  Replaces nothing in the reference (eager PyTorch leaves the kernel choice to cuDNN,
 * CODON_x4.py:68-131). */
#define CODON_FORM_STEM 0
#define CODON_FORM_HEAD 1
#define CODON_FORM_CAC_STATS 2
#define CODON_FORM_CAC_BWD_GATE 3
#define CODON_FORM_CAC_SPATIAL_FWD 4
#define CODON_FORM_CAC_SPATIAL_BWD 5
#define CODON_FORM_CONV1CH_WGRAD 6
typedef struct codon_form {
  int32_t vec, rows, depth, cols, tile, tiles, slices, per, vector;
} codon_form;
int codon_launch_form(int32_t op, int32_t dtype, int32_t batch, int32_t height, int32_t width, int32_t aligned, codon_form* out);

/* A conv whose input is the CAC gate-apply of the producing block, formed while the input tile is staged instead of
 * being written to HBM and read back (inference):   x = pre * (ch * sp) + inputs ,  y = conv(x) [ReLU]
 *   out*ad_CAC + inputs  /  out_c*ad_CAC + inputs_c  feeding conv1, conv2 / conv4, conv5 / conv7
 *   /root/reference/CODON_X4/CODON_x4.py:89-91,117-120,75-78.
 * d->x_* describe `pre` (channels of the (B,128,H,W) [pre | pre_c] buffer); `inputs` = the same channels of
 * [inputs | inputs_c]; ch: (B,64) fp32 channel gate (channel c of the 128 uses ch[c & 63]); sp: (B,1,H,W) fp32 spatial
 * gate.  flags: CODON_CONV_RELU only.  Same arithmetic as codon_cac_apply_fwd followed by codon_conv2d_fwd, bit for
 * bit.  Any dtype, (k, cin, cout) in {(5,64,64), (3,64,64), (3,128,64)}. */
int codon_conv2d_gated_fwd(const codon_conv_desc* d, const void* pre, const codon_tensor* inputs, const float* ch,
                           const float* sp, const void* w_packed, void* y, codon_stream_t stream);
/* The same conv, which ALSO writes its gate-applied input x (the d->cin channels, each workgroup the pixels of its own
 * tile, the values it staged) to the `gated_out` slice: `out` / `out_c` feed TWO convs (conv1 + conv2, conv4 + conv5,
 * CODON_x4.py:75-78) -- the first one applies the gate and emits x, the second reads it as a plain conv (codon_conv2d_fwd)
 * instead of repeating the gate arithmetic in its own staging.  gated_out must not alias `pre` / `inputs` (other tiles
 * still read their halos from them).  Any dtype. */
int codon_conv2d_gated_emit_fwd(const codon_conv_desc* d, const void* pre, const codon_tensor* inputs, const float* ch,
                                const float* sp, const void* w_packed, void* y, const codon_tensor* gated_out,
                                codon_stream_t stream);

/* dL/dw (cout, cin, k, k) fp32 = sum over b,h,w of gy[b,co,h,w] * x[b,ci,h+dy-p,w+dx-p]: what autograd
 * computes for the nn.Conv2d weights (the reference has no explicit backward).
 * d describes the FORWARD conv: x = its input (x_* fields), gy = gradient of its output (y_* fields
 * describe gy's buffer).  workspace: codon_conv_wgrad_workspace_bytes(d) bytes of scratch (per-split
 * partials, summed in fixed order: deterministic).  accumulate: 0 = dw is overwritten; 1 = the result is ADDED into dw
 * (weights shared by the 5 / 3 loop iterations, CODON_x4.py:74,122); CODON_WGRAD_DEFER = the per-split partials
 * [nsplit][k*k][cout][cin] (nsplit = workspace bytes / (4 k k cout cin)) are LEFT in `workspace` for a later
 * codon_reduce_multi -- one launch for all the weight gradients of a backward pass -- and dw is not touched (may be NULL). */
#define CODON_WGRAD_DEFER 2
size_t codon_conv_wgrad_workspace_bytes(const codon_conv_desc* d);
int codon_conv2d_wgrad(const codon_conv_desc* d, const void* x, const void* gy, float* dw,
                       void* workspace, size_t workspace_bytes, int32_t accumulate,
                       codon_stream_t stream);
/* Both gradients of a 1x1 conv 128 -> 64 whose input is a ReLU output, in ONE pass over x and gy (16-bit dtypes):
 *   dw (+)= dL/dw as codon_conv2d_wgrad;   gx = (W^T gy) * [x > 0]   as codon_conv2d_fwd on the CODON_PACK_DGRAD image with
 *   CODON_CONV_MASK_RELU and x as the mask -- bit for bit the results of those two calls.
 * confuse / confuse_c / confuse_fuse and the ReLU in front of them: /root/reference/CODON_X4/CODON_x4.py:81-84,126-127
 * (autograd; the reference has no explicit backward).  d describes the FORWARD conv (k = 1, cin = 128,
 * cout = 64; x_* = its input, y_* = gy's buffer), gx = the (B,128,H,W) slice the input gradient is written to (must
 * not alias x or gy), workspace as codon_conv_wgrad_workspace_bytes(d). */
int codon_conv1x1_bwd(const codon_conv_desc* d, const void* x, const void* gy, const void* w_packed_dgrad,
                      const codon_tensor* gx, float* dw, void* workspace, size_t workspace_bytes, int32_t accumulate,
                      codon_stream_t stream);
/* Same pass with the CAC gate backward formed while the output-gradient tile is staged (16-bit tensors, training): g_out is
 * ONE stream's half of the block's dL/d(out) (the 64-channel slice d->y_*), and the 1x1 conv's output gradient is
 *   dL/d(pre)[c,p] = g_out[c,p] * ch[c] * sp[p] + g_pools[0][f]/HW + g_pooled[1][p]/128
 *                    + [p == argpix[f]] g_pools[1][f] + [f == argch[p]] g_pooled[0][p],   f = fcat_base + c
 * -- what codon_cac_bwd_apply would store as g_pre, bit for bit (autograd of CODON_x4.py:85-91, CAC_module.py:38-94).
 * argch: (B,H,W) int32 from codon_cac_bwd_reduce_acc; fcat_base: 0 = colour stream, 64 = depth stream. */
int codon_conv1x1_bwd_gated(const codon_conv_desc* d, const void* x, const void* g_out, const void* w_packed_dgrad,
                            const codon_tensor* gx, float* dw, void* workspace, size_t workspace_bytes, int32_t accumulate,
                            const float* ch, const float* sp, const float* g_pooled, const float* g_pools,
                            const int32_t* argpix, const int32_t* argch, int32_t fcat_base, codon_stream_t stream);

/* ---- stem / head stencils (HBM-bound) ----------------------------------------------------
 * stem: y[:, y_coff:y_coff+64] = relu(conv3x3_{1->64}(x))        CODON_x4.py:68,71
 * head: y = conv3x3_{64->1}(x) + residual                         CODON_x4.py:130-131 */
int codon_stem_fwd(int32_t batch, int32_t height, int32_t width, const float* x,
                   const float* w_oihw, void* y, int32_t y_ctotal, int32_t y_coff, int32_t dtype,
                   codon_stream_t stream);
/* both stems of a forward -- relu(input(x)) and relu(input_c(y)), CODON_x4.py:68,71 -- as ONE launch (at one image per call,
 * test.py:116-125, each is a launch of 10-17 us that covers a fraction of the chip): two codon_stem_fwd calls' arguments, the
 * results bit for bit.  The two output slices must not overlap. */
int codon_stem_pair_fwd(int32_t batch, int32_t height, int32_t width, const float* xa, const float* wa_oihw, void* ya,
                        int32_t ya_ctotal, int32_t ya_coff, const float* xb, const float* wb_oihw, void* yb,
                        int32_t yb_ctotal, int32_t yb_coff, int32_t dtype, codon_stream_t stream);
int codon_head_fwd(int32_t batch, int32_t height, int32_t width, const void* x, int32_t x_ctotal,
                   int32_t x_coff, const float* w_oihw, const float* residual, float* y,
                   int32_t dtype, codon_stream_t stream);
/* head with the output map stored in the activations' 16-bit type (dtype = CODON_BF16 / CODON_F16 only): what a module
 * cast as a whole returns -- `model.cuda().half()`, /root/reference/CODON_X4/test.py:52,125.  The fp32 sum conv + residual
 * rounded once: the bits of codon_head_fwd followed by a conversion pass, without the pass (one launch of ~40 at one image
 * per call).  residual stays fp32 (B,1,H,W). */
int codon_head_fwd_y16(int32_t batch, int32_t height, int32_t width, const void* x, int32_t x_ctotal,
                       int32_t x_coff, const float* w_oihw, const float* residual, void* y16,
                       int32_t dtype, codon_stream_t stream);

/* ---- non-finite input guard: the stems detect, the head poisons -------------------------------------------------------
 * The reference turns ONE NaN / +Inf / -Inf pixel of x or y into an all-NaN map for that image and leaves the other images
 * of the batch untouched (torch's ReLU keeps NaN; the global pools of the first CAC block, CAC_module.py:43,47, spread it
 * over every channel; the gate, CODON_x4.py:89-91, over every pixel).  The kernels' ReLUs and pools are IEEE maxNum and
 * would drop it.  The stems read every input pixel exactly once as a centre pixel, so they test it there ("exponent all
 * ones" on the fp32 word: denormals, zeros, +-FLT_MAX pass) and report to
 *   bad:        (batch) int32 words in DEVICE memory; bad[b] = 1 for the image the pixel belongs to.  ZERO on entry:
 *               cleared by the caller, or by codon_weight_checksum_clear, the launch that opens a forward;
 *   host_word*: ONE int32 word each in HOST-VISIBLE (pinned, device-mapped) memory -- a relaxed system-scope store of 1, as
 *               codon_weight_checksum's flag; polled by the caller without synchronising, never cleared by a kernel.
 * Either pointer may be NULL; with all of them NULL the guarded entry IS the plain one (which is defined that way).  The
 * stems' outputs are the plain entries' bit for bit in every case.
 * Heads: with bad != NULL and bad[b] != 0 every element of image b is stored as a quiet NaN of the output's type; images
 * with bad[b] == 0 are stored as by the plain entry.  Gradients are no inputs of the network: the backward's uses of these
 * kernels (codon_stencil_1to64, codon_head_fwd on dL/dy) go through the plain entries. */
int codon_stem_fwd_guarded(int32_t batch, int32_t height, int32_t width, const float* x, const float* w_oihw, void* y,
                           int32_t y_ctotal, int32_t y_coff, int32_t dtype, int32_t* bad, int32_t* host_word,
                           codon_stream_t stream);
int codon_stem_pair_fwd_guarded(int32_t batch, int32_t height, int32_t width, const float* xa, const float* wa_oihw, void* ya,
                                int32_t ya_ctotal, int32_t ya_coff, const float* xb, const float* wb_oihw, void* yb,
                                int32_t yb_ctotal, int32_t yb_coff, int32_t dtype, int32_t* bad, int32_t* host_word_a,
                                int32_t* host_word_b, codon_stream_t stream);
int codon_head_fwd_guarded(int32_t batch, int32_t height, int32_t width, const void* x, int32_t x_ctotal, int32_t x_coff,
                           const float* w_oihw, const float* residual, float* y, int32_t dtype, const int32_t* bad,
                           codon_stream_t stream);
int codon_head_fwd_y16_guarded(int32_t batch, int32_t height, int32_t width, const void* x, int32_t x_ctotal,
                               int32_t x_coff, const float* w_oihw, const float* residual, void* y16, int32_t dtype,
                               const int32_t* bad, codon_stream_t stream);

/* ---- CAC gate (HBM-bound) -----------------------------------------------------------------
 * Fcat = cat(out_c, out) is never materialised: pre_c (colour, channels 0..63 of Fcat) and pre
 * (depth, channels 64..127) are passed separately (CODON_x4.py:85).
 *
 * stats : one pass over Fcat producing
 *           pooled   (B,2,H,W) fp32 : channel max (plane 0) and channel mean (plane 1)
 *                                      ChannelPool, CAC_module.py:78-81
 *           partials (B,ntiles,128,2) fp32 : per-tile per-channel {sum, max}
 *                                      first stage of avg_pool2d / max_pool2d, CAC_module.py:43,47
 *         ntiles = codon_cac_stats_tiles(H, W).
 * gate  : finishes the pools (fixed-order second stage, run-to-run deterministic) and applies the
 *         shared MLP + sigmoid:  ch (B,64) = sigmoid(mlp(avg) + mlp(max))   CAC_module.py:30-35,58-62
 *         pools_out (B,2,128) receives {avg,max} when non-null (saved for backward).
 * spatial: sp (B,1,H,W) = sigmoid(conv5x5_{2->1,pad 2}(pooled))            CAC_module.py:88,92-93
 * apply : out = pre*ch*sp + inputs ; out_c = pre_c*ch*sp + inputs_c         CODON_x4.py:89-91,117-118 */
int32_t codon_cac_stats_tiles(int32_t height, int32_t width);
int codon_cac_stats_fwd(int32_t batch, int32_t height, int32_t width, const codon_tensor* pre_c,
                        const codon_tensor* pre, float* pooled, float* partials, int32_t dtype,
                        codon_stream_t stream);
/* Sequential-gate ablation (BaseNet_RMCR_fuseRMCR_cross, /root/reference/CODON_X4/base_net_withoutBN.py:2186-2317; SURVEY.md
 * 8f row f4): its spatial gate sees the CHANNEL-GATED features, and its trunk squares the 64-channel fuse tensor
 * through ChannelGate's `x * scale` return value.
 *   cac_stats_scaled_fwd: codon_cac_stats_fwd on Fcat[b][c] * ch[b][c & 63]  (ch: (B,64) fp32; only `pooled` is meaningful)
 *   ew_sq_scale         : y = x * x * ch[b][c] over a 64-channel slice */
int codon_cac_stats_scaled_fwd(int32_t batch, int32_t height, int32_t width, const codon_tensor* pre_c,
                               const codon_tensor* pre, const float* ch, float* pooled, float* partials,
                               int32_t dtype, codon_stream_t stream);
int codon_ew_sq_scale(int32_t batch, int32_t height, int32_t width, const codon_tensor* x, const float* ch,
                      const codon_tensor* y, int32_t dtype, codon_stream_t stream);
int codon_cac_gate_fwd(int32_t batch, int32_t height, int32_t width, const float* partials,
                       const float* w1, const float* b1, const float* w2, const float* b2,
                       float* ch, float* pools_out, codon_stream_t stream);
int codon_cac_spatial_fwd(int32_t batch, int32_t height, int32_t width, const float* pooled,
                          const float* w_spatial, float* sp, codon_stream_t stream);
int codon_cac_apply_fwd(int32_t batch, int32_t height, int32_t width, const codon_tensor* pre,
                        const codon_tensor* pre_c, const float* ch, const float* sp,
                        const codon_tensor* inputs, const codon_tensor* inputs_c,
                        const codon_tensor* out, const codon_tensor* out_c, int32_t dtype,
                        codon_stream_t stream);

/* ---- backward (what torch.autograd computes for the reference) ------------
 * dtype = codon_dtype of the 64/128-channel activation and gradient tensors (fp32 or bf16); 1-channel
 * maps, gates, pooled maps and every parameter gradient are fp32.
 * The MFMA convs back-propagate through codon_conv2d_fwd (CODON_PACK_DGRAD weights, MASK_RELU /
 * ACCUM_OUT epilogues) and codon_conv2d_wgrad above; the entry points below cover the rest. */

/* Generalised 1->64 3x3 stencil.  flags: 1 = ReLU, 2 = spatially flipped taps.
 * flags=1           : the stem forward (== codon_stem_fwd)
 * flags=2, w=output.weight, x=dL/dy, mask=t11 : dL/dt11 of the head conv, masked by conv11's ReLU
 *                     (backward of CODON_x4.py:129-130). mask may be NULL. */
int codon_stencil_1to64(int32_t batch, int32_t height, int32_t width, const float* x,
                        const float* w_64x9, const codon_tensor* y, int32_t flags,
                        const codon_tensor* mask, int32_t dtype, codon_stream_t stream);

/* dw[c*9 + t] = sum_{b,q} a[b,c,q] * s[b, q + (t/3-1, t%3-1)]   (flip: written at c*9 + 8-t)
 * stem: a = dL/d(stem output, ReLU-masked), s = x, flip=0  -> input.weight.grad (64,1,3,3)
 * head: a = t11, s = dL/dy, flip=1                         -> output.weight.grad (1,64,3,3) */
/* flip: bit 0 = flipped taps; bit 1 (CODON_W1_ACCUMULATE) = dw += ...; bit 2 (CODON_W1_DEFER) = the (nparts, 576) partial
 * rows, nparts = workspace bytes / 2304, stay in `workspace` for codon_reduce_multi (rows item: nchunk 16, FLIP9 for the
 * head) and dw is not touched (may be NULL). */
#define CODON_W1_FLIP 1
#define CODON_W1_ACCUMULATE 2
#define CODON_W1_DEFER 4
size_t codon_conv1ch_wgrad_workspace_bytes(int32_t batch, int32_t height, int32_t width);
int codon_conv1ch_wgrad(int32_t batch, int32_t height, int32_t width, const codon_tensor* a,
                        const float* s, float* dw, int32_t flip, void* workspace,
                        size_t workspace_bytes, int32_t dtype, codon_stream_t stream);

/* dst = [dst +] src (src may be NULL), then dst = mask > 0 ? dst : 0 (mask may be NULL); C channels. */
int codon_ew_add_mask(int32_t batch, int32_t height, int32_t width, int32_t channels,
                      const codon_tensor* dst, const codon_tensor* src, const codon_tensor* mask,
                      int32_t accumulate, int32_t dtype, codon_stream_t stream);
/* dst = mask > 0 ? src0 + ... + src{nsrc-1} : 0 (1 <= nsrc <= 4, summed left to right; dst aliases no source; mask may be
 * null).  16-bit tensors: ONE pass, fp32 sum rounded once; fp32: the same result as a copy + nsrc-1 accumulating
 * codon_ew_add_mask passes.  Collects dL/d(fuse) = sum of the trunk's dL/d(f_i) (autograd of CODON_x4.py:122-128). */
int codon_ew_sum_mask(int32_t batch, int32_t height, int32_t width, int32_t channels, const codon_tensor* dst,
                      int32_t nsrc, const codon_tensor* src0, const codon_tensor* src1, const codon_tensor* src2,
                      const codon_tensor* src3, const codon_tensor* mask, int32_t dtype, codon_stream_t stream);

/* CAC gate backward, four launches (see codon_amd/csrc/cac_bwd.hip for the math):
 * reduce : g_z (B,1,H,W) = dL/d(spatial logits); part_gch (B,nt,64), part_arg (B,nt,128) int32,
 *          nt = codon_cac_bwd_tiles(H,W).  pools = the (B,2,128) {avg,max} saved by cac_gate_fwd.
 * gate   : g_pools (B,2,128) = dL/d{avg,max}; argpix (B,128) int32 first arg-max pixel of each Fcat
 *          channel; part_param (B,1608) scratch; dw1 (8,128), db1 (8), dw2 (64,8), db2 (64) OVERWRITTEN -- or all four
 *          NULL: the per-image rows w1 | b1 | w2 | b2 (offsets 0, 1024, 1032, 1544) stay in part_param for codon_reduce_multi.
 * spatial: g_pooled (B,2,H,W) = dL/d{chmax,chmean}; part_w (codon_cac_bwd_spatial_blocks(B,H,W),50)
 *          scratch; dw (1,2,5,5) OVERWRITTEN -- or NULL: the rows stay in part_w for codon_reduce_multi (nchunk 64 when
 *          there are >= 64 rows, else 1: the order of the immediate form).
 * apply  : g_pre / g_pre_c = full dL/dpre, dL/dpre_c; g_in / g_in_c (+)= g_out / g_out_c
 *          (accumulate_in = 0 writes instead of adding). */
int32_t codon_cac_bwd_tiles(int32_t height, int32_t width);
int32_t codon_cac_bwd_spatial_blocks(int32_t batch, int32_t height, int32_t width);
int codon_cac_bwd_reduce(int32_t batch, int32_t height, int32_t width, const codon_tensor* g_out,
                         const codon_tensor* g_out_c, const codon_tensor* pre, const codon_tensor* pre_c,
                         const float* ch, const float* sp, const float* pools, float* g_z,
                         float* part_gch, int32_t* part_arg, int32_t dtype, codon_stream_t stream);
/* 16-bit tensors: pass A that ALSO writes argch (B,H,W) int32 = the first arg-max channel of every pixel's channel max-pool
 * in Fcat order (255 if none; pooled = the forward's (B,2,H,W) {max, mean} map) and folds dL/d(out) into the running
 * dL/d(inputs): g_in (+)= g_out, g_in_c (+)= g_out_c (accumulate_in = 1: add, 0: plain copy, 2: leave g_in alone -- the
 * convs that produced g_out already added it, codon_conv2d_sum_into_fwd).  With codon_conv1x1_bwd_gated this replaces
 * codon_cac_bwd_apply in a training step. */
int codon_cac_bwd_reduce_acc(int32_t batch, int32_t height, int32_t width, const codon_tensor* g_out,
                             const codon_tensor* g_out_c, const codon_tensor* pre, const codon_tensor* pre_c,
                             const float* ch, const float* sp, const float* pools, const float* pooled, float* g_z,
                             float* part_gch, int32_t* part_arg, int32_t* argch, const codon_tensor* g_in,
                             const codon_tensor* g_in_c, int32_t accumulate_in, int32_t dtype, codon_stream_t stream);
int codon_cac_bwd_gate(int32_t batch, int32_t height, int32_t width, const float* part_gch,
                       const int32_t* part_arg, const float* ch, const float* pools, const float* w1,
                       const float* b1, const float* w2, float* g_pools, int32_t* argpix,
                       float* part_param, float* dw1, float* db1, float* dw2, float* db2,
                       codon_stream_t stream);
int codon_cac_bwd_spatial(int32_t batch, int32_t height, int32_t width, const float* g_z,
                          const float* pooled, const float* w_spatial, float* g_pooled, float* part_w,
                          float* dw_spatial, codon_stream_t stream);
int codon_cac_bwd_apply(int32_t batch, int32_t height, int32_t width, const codon_tensor* g_out,
                        const codon_tensor* g_out_c, const codon_tensor* pre, const codon_tensor* pre_c,
                        const float* ch, const float* sp, const float* pooled, const float* g_pooled,
                        const float* g_pools, const int32_t* argpix, const codon_tensor* g_pre,
                        const codon_tensor* g_pre_c, const codon_tensor* g_in, const codon_tensor* g_in_c,
                        int32_t accumulate_in, int32_t dtype, codon_stream_t stream);

/* ---- every deferred fixed-order reduction of a backward pass in ONE launch ---------------------------------------
 * Parameter gradients of autograd through CODON_x4.py:66-132 (the reference has no explicit backward) leave
 * their kernels as partial sums; instead of one small reduce launch behind each producer (86 per training step) the caller
 * collects them as items and reduces them all at once, optionally ADDING into its own gradient storage (a slice of the flat
 * data-parallel all-reduce buffer: no per-tensor add afterwards).  Every sum runs in a fixed order.
 *   WGRAD item : out (cout,cin,k,k) (+)= r_0 + r_1 + ... + r_{nuse-1} (added in that order; the 5 / 3 uses of a shared weight),
 *                r_u = sum_s part[u][s][tap][co][ci] over nparts splits, serially from zero: the CODON_WGRAD_DEFER
 *                workspaces.  Bit for bit what nuse immediate calls (accumulate = 1 on all but the first) produce.
 *                cin % 4 == 0, workspaces 16-byte aligned; taps = k*k.
 *   rows item  : out[f(i)] (+)= sum_k part[0][k*stride + i], i < cin (= the row length; cout = taps = 1), nparts rows.
 *                nchunk 1: serial; 16 or 64: two-level -- chunk c = rows [c*per, (c+1)*per), per = ceil(nparts/nchunk),
 *                summed serially, then the chunk sums in order.  CODON_REDUCE_FLIP9: f(i) = (i/9)*9 + 8 - i%9.
 * flags: CODON_REDUCE_ACCUMULATE adds into out instead of overwriting.  The items of one call run CONCURRENTLY: no two of them
 * may share `out` (a weight with more than CODON_REDUCE_MAX_USES uses continues in a second call with ACCUMULATE). */
#define CODON_REDUCE_MAX_USES 5
#define CODON_REDUCE_MAX_ITEMS 44
enum { CODON_REDUCE_ACCUMULATE = 1, CODON_REDUCE_WGRAD = 2, CODON_REDUCE_FLIP9 = 4 };
typedef struct codon_reduce_item {
  float* out;
  const float* part[CODON_REDUCE_MAX_USES];
  int64_t stride;   /* rows item: floats between consecutive rows */
  int32_t nuse;     /* WGRAD item: workspaces in part[] (1..CODON_REDUCE_MAX_USES) */
  int32_t nparts;   /* splits per workspace / rows */
  int32_t cout, cin, taps;
  int32_t nchunk;   /* rows item: 1, 16 or 64 */
  int32_t flags;
  int32_t reserved;
} codon_reduce_item;
int codon_reduce_multi(const codon_reduce_item* items, int32_t n_items, codon_stream_t stream);

/* ---- either side of the network in the reference's script ----------------------------
 * postprocess_u8 : out[i] = (uint8)(clip(x[i],0,1) * 255)  (truncating)      CODON_X4/test.py:127-132
 * masked_sqerr   : acc[0] = sum_{label!=0} (label-out)^2, acc[1] = #{label!=0}, exact 64-bit integers;
 *                  RMSE = sqrt(acc[0]/acc[1])                                 CODON_X4/test.py:148-164
 * ssim_fwd       : value[0] (double) = mean SSIM map of (a, b), both (B,1,H,W) fp32; 13-tap Gaussian sd 1.5,
 *                  'reflect' boundary, C1 = 0.01^2, C2 = 0.03^2              CODON_X4/ssim_2.py:36-52
 *                  partial: codon_ssim_tiles(B,H,W) floats scratch; dmaps: NULL or (B,3,H,W) derivative maps
 * l1_fwd         : value[0] (double) = mean |a - b| ; partial: nparts floats scratch
 * ssim_l1_bwd    : ga = ssim_scale * d(sum SSIM)/da + l1_scale * sign(a - b); tmp: (B,3,H,W) scratch; H,W >= 7 */
int codon_postprocess_u8(int64_t n, const float* x, uint8_t* out, codon_stream_t stream);
/* same, with the product formed in the ARRAY'S dtype as numpy does: dtype CODON_F16 rounds clip(x)*255 to fp16
 * before truncating (the reference's default fp16 path, test.py:52,125-132); CODON_F32 == codon_postprocess_u8. */
int codon_postprocess_u8_dt(int64_t n, const void* x, int32_t dtype, uint8_t* out, codon_stream_t stream);
int codon_masked_sqerr(int64_t n, const uint8_t* label, const uint8_t* out, uint64_t* acc,
                       codon_stream_t stream);
/* 16-bit depth codes.  No reference counterpart -- the reference's outputs are 8-bit -- so these are
 * DEFINITIONS, restated in numpy in tests/train_data16_ref.py.
 * postprocess_u16_dt : out[i] = (uint16)rint(clamp(x[i], 0, 1) * (float)depth_max), round half to even; x of dtype CODON_F32 /
 *                      CODON_F16 / CODON_BF16 is upcast to fp32 (exactly) and the product is formed in fp32; NaN -> 0 (fmaxf);
 *                      depth_max in [1, 65535].
 * masked_sqerr_u16   : codon_masked_sqerr over u16 codes: acc[0] = sum_{label!=0} (label-out)^2, acc[1] = #{label!=0}, exact
 *                      64-bit integers.  Bound: one term is at most 65535^2 < 2^32, and n <= 2^26 pixels is required, so
 *                      acc[0] <= 65535^2 * 2^26 < 2^58 fits a uint64 with room to spare. */
int codon_postprocess_u16_dt(int64_t n, const void* x, int32_t dtype, int32_t depth_max, uint16_t* out, codon_stream_t stream);
int codon_masked_sqerr_u16(int64_t n, const uint16_t* label, const uint16_t* out, uint64_t* acc, codon_stream_t stream);
int32_t codon_ssim_tiles(int32_t batch, int32_t height, int32_t width);
int codon_ssim_fwd(int32_t batch, int32_t height, int32_t width, const float* a, const float* b,
                   float* partial, float* dmaps, double* value, codon_stream_t stream);
int codon_l1_fwd(int64_t n, const float* a, const float* b, float* partial, int32_t nparts,
                 double* value, codon_stream_t stream);
int codon_ssim_l1_bwd(int32_t batch, int32_t height, int32_t width, const float* a, const float* b,
                      const float* dmaps, float* tmp, float* ga, float ssim_scale, float l1_scale,
                      codon_stream_t stream);

/* ---- hole-aware L1 + SSIM loss (codon_amd.metrics.MaskedL1SSIMLoss) ----------------------------------------
 * No reference counterpart (it ships no loss); the validity rule is EvaluationResults' (CODON_X4/test.py:148-164:
 * label == 0 is a hole).  pred p, target t: (B,1,H,W) fp32.  valid: u8 (B,1,H,W), nonzero = valid, or NULL for v = (t != 0).
 *   n_b = #valid pixels of image b;  E_b = pixels whose whole 13x13 window is valid (reflect indexing), e_b = |E_b|
 *   L1_b = sum_v |p - t| / max(n_b, 1);  SSIM_b = sum_{E_b} ssim / max(e_b, 1), 1 when e_b = 0 (ssim: ssim_fwd's per-pixel value)
 *   value[0] (double) = (1/B) sum_b [ w_l1 L1_b + w_ssim (1 - SSIM_b) ]
 * Invalid pixels of p and t are read as 0, so nothing stored there (NaN, Inf) reaches any result.  Two launches, no float
 * atomics, every sum in a fixed order that depends on H and W alone, counts in integers, sums in float64.
 *   ws: 4 * codon_ssim_tiles(B,H,W) 4-byte words of scratch;  dmaps: NULL or (B,3,H,W) derivative maps (0 outside E_b)
 *   counts: int64 (B,2) {n_b, e_b};  per_image: double (B,2) {L1_b, SSIM_b};
 *   scales: float (B,2) {-w_ssim / (B e_b), w_l1 / (B n_b)} (0 for an empty set), read by the backward.
 * masked_l1_ssim_bwd: ga = upstream[0] * ( scales[b][0] d(sum_E ssim)/dp + scales[b][1] sign(p - t) ) at valid pixels and
 * exactly +0.0f (selected, not multiplied) at invalid ones; upstream: one float in device memory; tmp: (B,3,H,W) scratch;
 * H, W >= 7.  Two launches. */
int codon_masked_l1_ssim_fwd(int32_t batch, int32_t height, int32_t width, const float* pred, const float* target,
                             const uint8_t* valid, float* ws, float* dmaps, double w_l1, double w_ssim, int64_t* counts,
                             double* per_image, float* scales, double* value, codon_stream_t stream);
int codon_masked_l1_ssim_bwd(int32_t batch, int32_t height, int32_t width, const float* pred, const float* target,
                             const uint8_t* valid, const float* dmaps, const float* scales, const float* upstream, float* tmp,
                             float* ga, codon_stream_t stream);

/* ---- synthetic-input generator: x4 / x8 / x16 bicubic upsample ---------------------------------
 * No reference counterpart (the reference's depth inputs are upsampled offline,
 * CODON_X4/test.py:70-77); defined in codon_amd/csrc/upsample.hip, restated in
 * oracle/upsample_oracle.py, required to agree bit for bit.  lr: (B,1,h,w) fp32;
 * phase_weights: (scale,4) fp32 Keys a=-0.75 weights per output phase; out: (B,1,h*scale,w*scale). */
int codon_bicubic_upsample(int32_t batch, int32_t lr_height, int32_t lr_width, int32_t scale,
                           const float* lr, const float* phase_weights, float* out,
                           codon_stream_t stream);

/* ---- stale-packed-weight guard -------------------------------------------------------------------
 * The packed MFMA weight images are cached on the host side under (data_ptr, Tensor._version) of each weight; the
 * reference's own init idiom writes THROUGH `.data` (`m.weight.data.normal_()`, CODON_X4/CODON_x4.py:50-53), which
 * that key cannot see.  codon_weight_checksum is launched once per forward: it folds a position-dependent 64-bit
 * checksum over the raw bytes of the n listed tensors (bytes[t] % 16 == 0, 16-byte aligned) and
 *   mode 0: stores it in *ref (device memory; taken when the packed images are (re)built);
 *   mode 1: compares it with *ref and, on a mismatch, stores 1 to *flag -- host-visible (pinned, device-mapped)
 *           memory that the caller polls without synchronising; never cleared by the kernel.
 * ws: codon_weight_checksum_workspace_bytes() of device memory, ZEROED once by the caller, private to one stream
 * (the kernel leaves its arrival counter at zero).  Defined in codon_amd/csrc/wsum.hip. */
#define CODON_WSUM_MAX 32
typedef struct codon_wsum_desc {
  int32_t n;
  int32_t reserved;
  const void* data[CODON_WSUM_MAX];
  uint64_t bytes[CODON_WSUM_MAX];
} codon_wsum_desc;
size_t codon_weight_checksum_workspace_bytes(void);
int codon_weight_checksum(const codon_wsum_desc* desc, void* ws, uint64_t* ref, int32_t mode, int32_t* flag,
                          codon_stream_t stream);
/* the same launch, which also stores 0 to clear[0 .. nclear): the `bad` words of the non-finite input guard above are
 * zeroed by the launch that opens the forward anyway, not by one of their own.  clear may be NULL (nclear = 0). */
int codon_weight_checksum_clear(const codon_wsum_desc* desc, void* ws, uint64_t* ref, int32_t mode, int32_t* flag,
                                int32_t* clear, int32_t nclear, codon_stream_t stream);

/* ---- the small fp32-arithmetic parameters of a 16-bit model as one flat fp32 buffer ------------------------------------
 * `model.cuda().half()` (/root/reference/CODON_X4/test.py:52) keeps the stems, the head and the gate tensors in 16 bits;
 * the kernels that use them take fp32.  One launch converts up to CODON_CAST_MAX tensors (count[t] elements of dtype[t],
 * a codon_dtype) into dst, back to back in the order given; nothing is cached (the live parameters are read every time). */
#define CODON_CAST_MAX 32
typedef struct codon_cast_desc {
  int32_t n;
  int32_t reserved;
  const void* src[CODON_CAST_MAX];
  int64_t count[CODON_CAST_MAX];
  int32_t dtype[CODON_CAST_MAX];
} codon_cast_desc;
int codon_cast_multi(const codon_cast_desc* desc, float* dst, codon_stream_t stream);

/* ---- one Adam step over all parameter tensors in ONE launch (round 6) -----------------------------------------------------
 * The reference ships no optimizer; BASELINE.json configs[2] is a training step, and torch.optim.Adam costs five
 * ATen launches per step.  param[t] (count[t] fp32 elements, updated in place) in the order of the flat gradient buffer `grad`
 * (codon_amd.dist.GradSync); exp_avg / exp_avg_sq: flat fp32 moment buffers of the same layout (zero before the first step).
 * torch.optim.Adam's update (amsgrad = False, maximize = False; weight_decay is the L2 form: g += weight_decay * p), `step` = 1,
 * 2, ...:  m += (1 - beta1)(g - m);  v = beta2 v + (1 - beta2) g g;  p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps). */
#define CODON_ADAM_MAX 64
typedef struct codon_adam_desc {
  int32_t n;
  int32_t reserved;
  void* param[CODON_ADAM_MAX];
  int64_t count[CODON_ADAM_MAX];
} codon_adam_desc;
int codon_adam_step(const codon_adam_desc* desc, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                    float beta2, float eps, float weight_decay, int32_t step, codon_stream_t stream);

/* ---- the guarded Adam step: global-norm clipping, non-finite skipping, EMA (codon_amd.dist.FlatAdam's options) -------------
 * No reference counterpart: the reference ships no training code.  Two launches per step on the caller's stream, no host
 * synchronisation, no float atomics, every reduction in a fixed order (a resumed run continues bit for bit, and N ranks reach
 * the same decision from their identical all-reduced gradients).  `state`: codon_grad_norm_workspace_bytes() of device
 * memory, 8-byte aligned, ZEROED once by the caller and private to one stream; its first four 8-byte words are
 * last_norm (double), applied, skipped, clipped (uint64 counts), the rest is scratch.
 *
 * codon_grad_norm: reads the flat fp32 gradient (n elements, 16-byte aligned) once and leaves per-workgroup partial sums of
 * g * g, accumulated in float64 (the product of two fp32 values is exact there), and counts of non-finite elements in `state`.
 *
 * codon_adam_step_guarded: codon_adam_step's update after folding those partials, block-uniformly:
 *   norm = sqrt(sum g g);  coef = min(1, max_norm / (norm + 1e-6)) in float64, rounded once to fp32 (torch's clip_grad_norm_;
 *   max_norm = +inf: no clipping, coef = 1 exactly);  the gradient used is coef * g (then + weight_decay * p as in
 *   codon_adam_step); `grad` itself is left unscaled.
 *   skip_nonfinite != 0 and any non-finite element: the WHOLE step is a no-op -- param, exp_avg, exp_avg_sq and ema keep their
 *   bits, `skipped` goes up by one.  Otherwise `applied` goes up by one, and `clipped` when coef < 1.  With skip_nonfinite = 0
 *   nothing is hidden: a NaN norm gives a NaN coef, an Inf norm coef = 0 and 0 * Inf = NaN.
 *   ema (flat fp32 in the gradient's layout, or null):  ema += (1 - ema_decay) * (param_new - ema), in the same pass.
 * `step` is a host argument and counts ATTEMPTED steps: a skipped step consumes its number (no read-back decides the bias
 * correction), so the guarded step with nothing firing equals codon_adam_step bit for bit. */
size_t codon_grad_norm_workspace_bytes(void);
int codon_grad_norm(const float* grad, int64_t n, void* state, codon_stream_t stream);
int codon_adam_step_guarded(const codon_adam_desc* desc, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema,
                            void* state, float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                            double max_norm, int32_t skip_nonfinite, double ema_decay, codon_stream_t stream);

/* ---- training-batch synthesis (codon_amd.train) -------------------------------------------------------------------------
 * No reference counterpart: the reference ships no training code and its depth inputs were degraded offline (bicubic down,
 * bicubic up, 8-bit PNG: CODON_X4/test.py:70-79,116-123) by a script it does not ship -- this pipeline is a DEFINITION, not
 * pinned to the reference.  Defined in codon_amd/csrc/train_data.hip, restated in numpy in tests/train_data_ref.py, required
 * to agree bit for bit.
 *
 * codon_train_crops: one launch for a batch of n <= CODON_TRAIN_MAX_BATCH samples of one crop size P.  `pool` is a flat u8
 * buffer of pool_bytes bytes; sample b's HR depth map (height x width, row-major) starts at s[b].offset and its grey guidance
 * image of the same size follows at s[b].offset + height * width.  The P x P window at (y0, x0) of both is taken through the
 * D4 op s[b].op (numpy: c = img[y0:y0+P, x0:x0+P]; op&1: c = c.T; op&2: c = c[::-1]; op&4: c = c[:, ::-1]) and written as
 * lut[u8] (a 256-entry fp32 table, device memory) to target and guide, (n,1,P,P) fp32 each.  Every window must lie inside
 * its image and every image inside the pool. */
#define CODON_TRAIN_MAX_BATCH 64
typedef struct codon_crop_sample {
  int64_t offset;
  int32_t height, width, y0, x0, op, reserved;
} codon_crop_sample;
typedef struct codon_crop_desc {
  int32_t n;
  int32_t crop;
  codon_crop_sample s[CODON_TRAIN_MAX_BATCH];
} codon_crop_desc;
int codon_train_crops(const codon_crop_desc* desc, const uint8_t* pool, int64_t pool_bytes, const float* lut, float* target,
                      float* guide, codon_stream_t stream);
/* codon_train_crops_labeled: the same window, D4 op and table for records of THREE planes -- depth map, guidance, label (at
 * s[b].offset + 2 * height * width): `source` (what the degradation reads) comes from the depth map, `target` from the label,
 * which may carry holes (code 0) the hole-filled depth map does not.  Every record (3 * height * width bytes) inside the pool. */
int codon_train_crops_labeled(const codon_crop_desc* desc, const uint8_t* pool, int64_t pool_bytes, const float* lut,
                              float* source, float* guide, float* target, codon_stream_t stream);
/* codon_bicubic_downsample: antialiased integer-factor reduction (PIL BICUBIC reduce; F.interpolate(mode="bicubic",
 * antialias=True, align_corners=False)) of hr (batch,1,size,size) fp32 by scale 4 / 8 / 16 to out (batch,1,size/scale,
 * size/scale).  weights: (size/scale) x (4*scale) fp32 -- row o holds the weights of input taps o*scale - 3*scale/2 + k,
 * k = 0 .. 4*scale-1 (taps outside the image: weight 0).  A horizontal pass, then a vertical pass, each a sequential fp32 sum
 * over k with an fp32 intermediate.  size % scale == 0, size / scale >= 4, size <= 2048. */
int codon_bicubic_downsample(int32_t batch, int32_t size, int32_t scale, const float* hr, const float* weights, float* out,
                             codon_stream_t stream);
/* codon_quantize_u8: in place, x[i] = lut[rint(clamp(x[i], 0, 1) * 255f)] (round half to even): the 8-bit PNG the network's
 * depth input is read from at test time. */
int codon_quantize_u8(int64_t n, float* x, const float* lut, codon_stream_t stream);
/* codon_train_crops_u16: codon_train_crops / _labeled for 16-bit depth, same window, same D4 op, same
 * descriptor.  A record in the byte pool is the depth plane (height * width little-endian u16) at s[b].offset, which must be
 * EVEN, then -- when target != NULL -- the label plane (height * width u16), then the guidance plane (height * width u8):
 * 3 or 5 bytes per pixel, every record inside the pool, the pool itself 2-byte aligned.  Depth and label codes c go through
 * lut16 (65 536 fp32 entries, device memory: lut16[c] = float32(float64(c) / depth_max)), guidance codes through lut8 (the
 * 256-entry table of codon_train_crops).  source / guide / target: (n,1,P,P) fp32.  target == NULL: two-plane records, and
 * `source` is the HR target too, as in codon_train_crops.  Codes above depth_max are the caller's to refuse (the table has an
 * entry for every u16, so nothing is read out of bounds). */
int codon_train_crops_u16(const codon_crop_desc* desc, const uint8_t* pool, int64_t pool_bytes, const float* lut16,
                          const float* lut8, float* source, float* guide, float* target, codon_stream_t stream);
/* codon_quantize_levels: in place, x[i] = lut16[(int)rintf(clamp(x[i], 0, 1) * (float)depth_max)] (round half to even; NaN
 * -> lut16[0]): codon_quantize_u8's counterpart at the same point of the degradation, onto the data set's own code grid.
 * depth_max in [1, 65535]. */
int codon_quantize_levels(int64_t n, float* x, const float* lut16, int32_t depth_max, codon_stream_t stream);

/* ---- hole-aware (mask-normalised) bicubic resampling: depth maps in which 0.0 / code 0 marks a hole ----------
 * No reference counterpart (the reference ships neither a degradation nor an upsampler): DEFINITIONS, in
 * codon_amd/csrc/resample_masked.hip, restated in numpy in tests/resample_masked_ref.py, required to agree bit for bit.
 * With N the unmasked kernel's own arithmetic (holes entering as 0.0), D the same arithmetic over the validity (0.0f / 1.0f)
 * and the count of invalid taps:  0 invalid -> N, valid;  otherwise D >= 0.5f -> N / D (correctly rounded), valid;  otherwise
 * +0.0f, a hole.
 *
 * codon_bicubic_upsample_masked: codon_bicubic_upsample under that rule (the count over all 16 taps, a clamped border tap
 * carrying its clamped pixel's validity).  valid: (B,1,h*scale,w*scale) u8, 1 where the result is valid, or NULL. */
int codon_bicubic_upsample_masked(int32_t batch, int32_t lr_height, int32_t lr_width, int32_t scale, const float* lr,
                                  const float* phase_weights, float* out, uint8_t* valid, codon_stream_t stream);
/* codon_bicubic_downsample_masked: codon_bicubic_downsample under that rule (numerator and denominator through both passes,
 * the count over the taps inside the image), then every valid value v is snapped as a sensor's file would hold it:
 * out = lut[min(max((int)rintf(clamp(v, 0, 1) * (float)levels), 1), levels)] -- never code 0; a hole is +0.0f.  lut: levels + 1
 * fp32 entries (levels 255 with the 256-entry table of codon_train_crops, or depth_max with lut16).  size <= 1024. */
int codon_bicubic_downsample_masked(int32_t batch, int32_t size, int32_t scale, const float* hr, const float* weights,
                                    const float* lut, int32_t levels, float* out, codon_stream_t stream);
/* codon_lr_codes_to_input: a low-resolution code plane as the network's depth input, one launch:
 *   codes (B,h,w) u8 (code_bits 8, depth_max 255, lut of 256 entries) or u16 (code_bits 16, lut16 of 65 536 entries)
 *   -> lut -> codon_bicubic_upsample_masked's rule -> lut[(int)rintf(clamp(., 0, 1) * (float)depth_max)]
 *   -> round to nearest even into dtype (a codon_dtype), written to out (B,1,h*scale,w*scale), 16-byte aligned.
 * Bit for bit codon_bicubic_upsample_masked, then codon_quantize_u8 / codon_quantize_levels, then a cast. */
int codon_lr_codes_to_input(int32_t batch, int32_t lr_height, int32_t lr_width, int32_t scale, const void* codes,
                            int32_t code_bits, const float* lut, int32_t depth_max, const float* phase_weights, void* out,
                            int32_t dtype, codon_stream_t stream);
/* codon_lr_codes_upsample: codon_lr_codes_to_input's sibling, the BICUBIC BASELINE: the same per-pixel
 * arithmetic, but what is written is the INTEGER the look-up takes before the cast, (int)rintf(clamp(., 0, 1) * (float)depth_max),
 * as codes of the input's own width: out (B,h*scale,w*scale) u8 or u16, 16-byte aligned, not codes itself.  A hole of the
 * rule stays code 0.  (A baseline cannot go through the float input and back: float32(k / 255) * 255 truncates to k - 1 for
 * some k.)  One launch. */
int codon_lr_codes_upsample(int32_t batch, int32_t lr_height, int32_t lr_width, int32_t scale, const void* codes,
                            int32_t code_bits, const float* lut, int32_t depth_max, const float* phase_weights, void* out,
                            codon_stream_t stream);
/* codon_train_crops_lr: a whole training batch -- x, guide, target, (n,1,P,P) fp32 each -- from records that PAIR an HR depth
 * map with a sensor's low-resolution code plane, one launch in place of the synthetic path's four.  Descriptor,
 * window and D4 op are codon_train_crops'; height x width is the HR size (H, W), both multiples of scale (4 / 8 / 16), and the
 * LR plane is (h, w) = (H / scale, W / scale).  The record at s[b].offset:
 *   code_bits 8  (depth_max 255, lut = lut8 = the 256-entry table): depth H*W u8, guidance H*W u8, LR codes h*w u8;
 *   code_bits 16 (lut = lut16 of depth_max, 65 536 entries):        depth H*W little-endian u16 at an EVEN offset, LR codes
 *                h*w u16, guidance H*W u8; the pool 2-byte aligned.
 * With (gy, gx) the source pixel of an output pixel under the window and the op:  target = lut[depth[gy][gx]],
 * guide = lut8[guidance[gy][gx]], and x = the value codon_lr_codes_to_input (dtype fp32) gives at HR pixel (gy, gx) of the
 * WHOLE LR plane -- the border clamp is at the image's edge, not the window's, and y0 / x0 need not be multiples of the scale:
 * x is the window, under the D4 op, of what inference builds from the whole file.  Every window inside its image, every
 * record inside the pool. */
int codon_train_crops_lr(const codon_crop_desc* desc, const uint8_t* pool, int64_t pool_bytes, int32_t scale, int32_t code_bits,
                         const float* lut, int32_t depth_max, const float* lut8, const float* phase_weights, float* x,
                         float* guide, float* target, codon_stream_t stream);

/* ---- the sensor model of the training degradation: range noise and dropout on the low-resolution map -------
 * No reference counterpart (the reference ships no degradation): DEFINITIONS, in codon_amd/csrc/sensor.hip, sensor_pixel.h and
 * sensor_rng.h, restated in numpy in tests/sensor_ref.py, required to agree bit for bit.
 *
 * codon_philox4x32_10: HOST ONLY, no GPU needed -- out[0..3] = Philox4x32-10 of the counter ctr[0..3] under the key key[0..1]
 * (Salmon et al., SC'11), from the very function the kernel calls: the known-answer check of the generator.
 *
 * codon_lr_sensor: ONE launch over lr (batch,1,size,size) fp32 into out (same shape; NOT in place, the edge term reads lr's
 * neighbours), one thread per pixel.  With v = lr[b][y][x] and (w0, w1, w2, w3) the Philox words of the counter
 * (y * size + x, first_sample + b, step, 0) under the key (seed_lo, seed_hi):
 *   masked != 0 and v == 0.0f: a hole stays a hole, +0.0f, and nothing below runs;
 *   e = fabsf(v - n) > edge_thr for any 4-neighbour n of lr inside the map (masked: a neighbour n == 0.0f does not count);
 *   masked != 0 and (uint64)w1 < T(p_drop) + (e ? T(p_edge) : 0), T(P) = (uint64)floor(P * 2^32) in float64: +0.0f (dropout);
 *   v' = v + (sigma + quad * (v * v)) * gauss[w0 >> 16], every fp32 operation rounded on its own; sigma, quad, edge_thr in
 *   VALUE units;
 *   masked != 0: out = lut[min(max((int)rintf(clamp(v', 0, 1) * (float)levels), 1), levels)], the snap of
 *   the masked downsample (never code 0);  masked == 0: out = v', unclamped.
 * gauss: 65 536 fp32 entries, gauss[u] = float32(inverse normal CDF((u + 0.5) / 65536)); lut and levels: the masked
 * downsample's (levels + 1 entries).  w2 and w3 are reserved.  Refused on the host, before any HIP call: null pointers, lr == out,
 * batch outside 1 .. CODON_TRAIN_MAX_BATCH, size outside 4 .. 512, levels outside 1 .. 65535, step or first_sample (+ batch)
 * outside 32 bits, a negative or non-finite sigma / quad / edge_thr, a probability outside [0, 1], p_drop + p_edge > 1, and
 * a non-zero probability with masked == 0 (without the masked upsample a dropped pixel would ring, not be left out). */
typedef struct codon_sensor_desc {
  int32_t batch;         /* samples in this launch */
  int32_t size;          /* p: each sample's map is size x size */
  int32_t masked;        /* 0: plain path (noise only, unsnapped); else: 0.0f is a hole, dropout allowed, output snapped */
  int32_t reserved;
  uint32_t seed_lo, seed_hi; /* the key: the low and high 32 bits of the 64-bit sensor seed */
  int64_t step;          /* c2: the training step, 0 .. 2^32 - 1 */
  int64_t first_sample;  /* c1 of sample 0: its index in the GLOBAL batch (the shard start) */
  float sigma, quad, edge_thr, reserved_f;
  double p_drop, p_edge;
} codon_sensor_desc;
int codon_philox4x32_10(const uint32_t* ctr, const uint32_t* key, uint32_t* out);
int codon_lr_sensor(const codon_sensor_desc* desc, const float* lr, const float* gauss, const float* lut, int32_t levels,
                    float* out, codon_stream_t stream);

/* ---- D4 self-ensemble (codon_amd.ensemble.self_ensemble) ---------------------------------------------------
 * No reference counterpart: DEFINITIONS, in codon_amd/csrc/d4.hip, restated in numpy in tests/d4_ref.py, equal bits required.
 * The D4 code is codon_crop_sample.op's, on a whole (H, W) plane c:  op&1: c = c.T;  then op&2: c = c[::-1];  then op&4:
 * c = c[:, ::-1].  Codes 0, 2, 4, 6 stay H x W ("upright"), codes 1, 3, 5, 7 are W x H ("transposed"); view k of image b is
 * image 4*b + (k >> 1) of its batch.  dtype: a codon_dtype, the element type of every plane but out_f32.
 *
 * codon_d4_views: ONE launch copies the bits of src0 (batch,1,H,W) into upright0 (4*batch,1,H,W) and transposed0
 * (4*batch,1,W,H), and the same from src1 into upright1 / transposed1; src1, upright1 and transposed1 may all three be NULL
 * (one plane only).  No arithmetic: NaN payloads and -0.0 arrive as they left.
 *
 * codon_d4_merge: ONE launch, out_f32[b] = 0.125f * (((u0+u1)+(u2+u3)) + ((u4+u5)+(u6+u7))), u_k the inverse of view k (undo
 * op&4, then op&2, then transpose if op&1) of the network's output on that view, upcast exactly to fp32, every add rounded
 * on its own in this order -- eight equal values average to themselves.  out_f32: (batch,1,H,W), ALWAYS fp32.  No atomics. */
int codon_d4_views(int32_t batch, int32_t height, int32_t width, const void* src0, const void* src1, int32_t dtype,
                   void* upright0, void* transposed0, void* upright1, void* transposed1, codon_stream_t stream);
int codon_d4_merge(int32_t batch, int32_t height, int32_t width, const void* upright, const void* transposed, int32_t dtype,
                   float* out_f32, codon_stream_t stream);

/* ---- depth evaluation suite (codon_amd.metrics.depth_errors) ------------------------------------------------
 * No reference counterpart (the reference prints one masked RMSE): DEFINITIONS, in codon_amd/csrc/eval.hip and eval_tile.h,
 * restated in numpy in tests/eval_ref.py, equal bits required.  Integers only.
 *
 * codon_depth_errors: ONE launch over a batch of code planes, all u8 (bits 8) or all u16 (bits 16): the output out
 * (batch, height, width), contiguous, and the label, image b at label + b * label_image_stride, its rows label_row_stride
 * elements apart, label_height x label_width >= height x width and read top-left -- the window is the output's, and no label
 * pixel beyond it is read, not even as a neighbour.  Per pixel: valid v = (L != 0), e = |L - O|.  acc: (batch, 16) uint64,
 * zeroed by this entry on the stream, then per image
 *   word 0      n = #v
 *   word 1      sum_v e
 *   word 2      sum_v e^2 (each square formed in 64 bits)
 *   word 3      max_v e (0 when n = 0)
 *   words 4-7   #{v, e > thresholds[k]}, k < n_thresholds (unused thresholds: 0)
 *   words 8-10  delta inliers in integers: #{v, 4 max(L,O) < 5 min(L,O)}, then 16 max < 25 min, then 64 max < 125 min
 *               (O = 0 is never an inlier)
 *   word 11     n_E = #E
 *   word 12     sum_E e
 *   word 13     sum_E e^2
 *   words 14-15 reserved, written as 0
 * Edge region E (edge != 0): a pixel is a discontinuity when it is valid and some 4-neighbour inside the window is valid and
 * differs from it by more than edge_threshold codes (codon_lr_sensor's rule); E = the valid pixels within Chebyshev distance
 * edge_radius of a discontinuity.  edge == 0: words 11-13 are 0 and no neighbour is read.
 * error_map (NULL, or (batch, height, width) of the codes' type): e where valid, 0 elsewhere.  region_map (NULL, or (batch,
 * height, width) uint8): 0 hole, 1 valid outside E, 2 valid in E.
 * Bound: e <= 65535, e^2 < 2^32, height * width <= 2^26, so no word exceeds 2^58.  Refused on the host, before any HIP call:
 * null pointers, bits other than 8 or 16, an unaligned u16 plane, a bad shape, more than 2^26 pixels per image, more than 65535
 * images or tile rows, a label smaller than the output or a row stride below label_width, n_thresholds outside 0..4, a
 * negative threshold, a negative edge_threshold, edge_radius outside 0..8. */
typedef struct codon_depth_errors_desc {
  int32_t batch, height, width;        /* the output planes = the evaluation window */
  int32_t bits;                        /* 8: uint8 codes, 16: uint16 codes (label, out and error_map alike) */
  int32_t label_height, label_width;   /* the label planes, at least height x width */
  int64_t label_row_stride;            /* elements between label rows (>= label_width) */
  int64_t label_image_stride;          /* elements between label images */
  int32_t n_thresholds;                /* 0..4 */
  int32_t thresholds[4];               /* codes, >= 0 */
  int32_t edge;                        /* 0: no edge evaluation */
  int32_t edge_threshold;              /* T, codes, >= 0 */
  int32_t edge_radius;                 /* r, 0..8 */
} codon_depth_errors_desc;
int codon_depth_errors(const codon_depth_errors_desc* desc, const void* label, const void* out, uint64_t* acc,
                       void* error_map, uint8_t* region_map, codon_stream_t stream);

/* ---- surface-normal angle error (codon_amd.metrics.normal_errors, infer --report-normals) -----------------------
 * Nothing in the reference: it prints one masked RMSE per image.  A DEFINITION, in codon_amd/csrc/normal_errors.hip and
 * normal_tile.h, restated in numpy in tests/normal_errors_ref.py, equal words and equal maps required.  Integers only.
 *
 * label: (batch, label_height, label_width) codes, read top-left through label_row_stride / label_image_stride (elements), as
 * codon_depth_errors reads it; out: (batch, height, width) codes, dense; both u8 (CODON_FILL_U8) or both u16 (CODON_FILL_U16), 0 a
 * hole.  Inside the height x width window the output counts as 0 wherever the label is 0, and both planes count as 0 outside the
 * window.  rx (width), ry (height): int32 ON THE DEVICE, codon_cloud_points' Q20 rays (of the LABEL's camera: a top-left crop keeps
 * the principal point, so only the first width and height entries are read); ray_span: ON THE HOST, rx[0], rx[width - 1], ry[0],
 * ry[height - 1].  cos_table, sin_table: int32[1440] ON THE DEVICE, rint(2^30 cos t_m) and rint(2^30 sin t_m) at t_m = (m - 1/2) / 8
 * degrees, m = 1 .. 1440, at index m - 1; trusted to be those values, as the range and Gauss tables of other entries are.  N_l and
 * N_o: the integer normals of cloud_tile.h of the label and of the masked output under radius, tol_abs and tol_rel_q16
 * (codon_cloud_points' link parameters).  A pixel is compared when its label is non-zero and both planes have a normal there; its
 * index is a = #{ m : A cos_table[m] - D sin_table[m] > 0 } with D = N_l . N_o and A = isqrt(|N_l x N_o|^2): rint(8 angle in degrees).
 * words: (batch, 1448) uint32 ON THE DEVICE, needs no initialisation (the entry zeroes it on the stream): 0 .. 1440 the histogram of
 * a, 1441 valid label pixels in the window, 1442 those whose label has a normal, 1443 compared pixels, 1444 pixels with label != 0
 * and out == 0, 1445 .. 1447 zero.  angle_map: NULL, or (batch, height, width) uint16: a where compared, 65535 elsewhere.
 *
 * ONE launch; no workspace; no host synchronisation.  Refused on the host, before any HIP call: null pointers (angle_map may be
 * NULL), an fmt other than CODON_FILL_U8 / _U16, batch outside 1 .. 65535, a height or width outside 1 .. 4096, top outside
 * 1 .. 65535 or not 255 for u8 codes, a label smaller than the window or strides that do not hold it, radius outside 1 .. 8,
 * tol_abs outside 0 .. top, tol_rel_q16 outside 0 .. 65535, a ray of the span of 2^22 or more in magnitude, a u16 plane or map that
 * is not 2-byte aligned, tables or words not 4-byte aligned. */
int codon_normal_errors(int32_t batch, int32_t height, int32_t width, const void* label, int32_t label_height, int32_t label_width,
                        int64_t label_row_stride, int64_t label_image_stride, const void* out, int32_t fmt, int32_t top,
                        const int32_t* rx, const int32_t* ry, const int32_t* ray_span, const int32_t* cos_table,
                        const int32_t* sin_table, int32_t radius, int32_t tol_abs, int32_t tol_rel_q16, uint32_t* words,
                        uint16_t* angle_map, codon_stream_t stream);

/* ---- pull-push hole filling of low-resolution code planes (codon_amd.upsample.fill_holes) -------------------
 * No reference counterpart (its depth inputs were hole-filled offline by a tool it does not ship): a DEFINITION, in
 * codon_amd/csrc/fill_holes.hip and fill_tile.h, restated in numpy in tests/fill_ref.py, equal bits required.  Integers only.
 *
 * A plane of codes, 0 a hole.  Level 0 is the plane; level k+1 has ceil(h_k / 2) x ceil(w_k / 2) cells; the top level K is the
 * first of 1 x 1.  Pull: cell (i, j) of level k+1 is (2 S + n) / (2 n) in integer division over its n valid children
 * (2i+a, 2j+b) inside level k, S their sum -- the mean, half rounded up -- or a hole when n = 0; only values valid at level k
 * enter.  Push, from the top down: a valid cell keeps its value; a hole at (y, x) of level k takes
 *   (9 F(py, px) + 3 F(py, qx) + 3 F(qy, px) + F(qy, qx) + 8) >> 4  of the filled level k+1, py = y >> 1,
 *   qy = clamp(py + (y odd ? +1 : -1), 0, h_{k+1} - 1), px and qx likewise from x.
 * Valid codes come back as they were, a plane without holes or without a valid code comes back unchanged, and with one valid
 * code no output is 0 or above the largest valid code.
 *
 * fmt: CODON_FILL_U8 (u8 codes, top 255), CODON_FILL_U16 (u16 codes, 2-byte aligned) or CODON_FILL_F32 (fp32 on the code grid
 * of `top`, as the masked downsample and the sensor launch write it: v loads as code (int)rintf(v * (float)top), anything not
 * positive is a hole, code c stores as tab[c] and a hole as +0.0f; tab: top + 1 fp32 entries).  tab is read by the fp32 format
 * only and may be NULL otherwise.  in, out: (batch, height, width), contiguous; out must not be in.
 *
 * codon_fill_holes_workspace_bytes: HOST ONLY, no GPU needed -- the bytes ONE image takes, at least 2 bytes per cell of the
 * levels 1 .. K; 0 for a height or width outside 1 .. 4096.  workspace: batch times that, 2-byte aligned, private to the stream.
 * Planes up to 64 x 64: one launch; larger: three.  The launches depend on (batch, height, width) alone; no atomics, no host
 * synchronisation.  Refused on the host, before any HIP call: null pointers, an unknown fmt, batch outside 1 .. 65535, height
 * or width outside 1 .. 4096, top outside 1 .. 65535 or not 255 for u8 codes, out == in, an unaligned plane or workspace, a
 * workspace that is too small. */
#define CODON_FILL_U8 0
#define CODON_FILL_U16 1
#define CODON_FILL_F32 2
size_t codon_fill_holes_workspace_bytes(int32_t height, int32_t width);
int codon_fill_holes(int32_t batch, int32_t height, int32_t width, const void* in, int32_t fmt, const float* tab, int32_t top,
                     void* out, void* workspace, size_t workspace_bytes, codon_stream_t stream);

/* ---- guidance-aware (joint) pull-push hole filling (codon_amd.upsample.fill_holes_guided) -------------------
 * No reference counterpart: a DEFINITION on top of codon_fill_holes', in codon_amd/csrc/fill_guided.hip and
 * fill_guided_tile.h, restated in numpy in tests/guided_fill_ref.py, equal bits required.  Integers only.
 *
 * The levels, the pull of the codes (V) and the four parents of a hole with their base weights B = 9, 3, 3, 1 are
 * codon_fill_holes'.  guide: u8, image b at guide + b * guide_image_bytes, row r at + r * guide_row_bytes; its top-left
 * (height * scale) x (width * scale) is used.  Guidance pyramid: G_0 the scale x scale box mean (2 S + s^2) / (2 s^2),
 * G_{k+1} = (2 S + n) / (2 n) over the n children inside level k.  Attached guidance: A_0 = G_0 at valid pixels,
 * A_{k+1} = (2 S_A + n) / (2 n) over the n valid children that entered V_{k+1}.  Push: a hole at (y, x) of level k weighs
 * parent p by w_p = B_p * range_tab[|G_k(y, x) - A^(p)|], A^(p) = A_{k+1}(p) where V_{k+1}(p) is valid, else G_{k+1}(p), and
 * takes (2 sum w_p F_{k+1}(p) + sum w_p) / (2 sum w_p).  range_tab: 256 u16 ON THE DEVICE, each 1 .. 256 (the caller's
 * duty: 16 <= sum w_p <= 4096 keeps everything inside 32 bits); a constant table, or a constant guide, gives
 * codon_fill_holes' bits.  Valid codes come back as they were and no filled value exceeds the largest valid code.
 *
 * fmt: CODON_FILL_U8 or CODON_FILL_U16.  in, out: (batch, height, width), contiguous; out must not be in.
 * codon_fill_guided_workspace_bytes: HOST ONLY -- the bytes ONE image takes (V, A and G of levels 1 .. K and G_0), a
 * multiple of 16; 0 for a height or width outside 1 .. 4096.  workspace: batch times that, 16-byte aligned, private to the
 * stream.  Planes up to 64 x 64: one launch; larger: three.  The launches depend on (batch, height, width, scale) alone; no
 * atomics, no host synchronisation.  Refused on the host, before any HIP call: null pointers, an fmt other than the two,
 * batch outside 1 .. 65535, height or width outside 1 .. 4096, top outside 1 .. 65535 or not 255 for u8 codes, a scale other
 * than 4, 8, 16, guide_row_bytes < width * scale, guide_image_bytes < height * scale * guide_row_bytes with batch > 1,
 * out == in, a u16 plane or a table that is not 2-byte aligned, a workspace that is not 16-byte aligned, a workspace that is
 * too small. */
size_t codon_fill_guided_workspace_bytes(int32_t height, int32_t width);
int codon_fill_holes_guided(int32_t batch, int32_t height, int32_t width, const void* in, int32_t fmt, int32_t top,
                            const uint8_t* guide, int64_t guide_row_bytes, int64_t guide_image_bytes, int32_t scale,
                            const uint16_t* range_tab, void* out, void* workspace, size_t workspace_bytes, codon_stream_t stream);

/* ---- joint bilateral upsampling (codon_amd.upsample.joint_bilateral_upsample) ----------------------------------
 * The classical guided baseline (Kopf et al. 2007) in the network's place.  No reference counterpart: a DEFINITION, in
 * codon_amd/csrc/jbu.hip and jbu_tile.h, restated in numpy in tests/jbu_ref.py, equal bits required.  Integers only.
 *
 * in: (batch, height, width) codes, 0 a hole; guide as codon_fill_holes_guided's, with its box means G_0.  The pixel (Y, X) of
 * out, (batch, height * scale, width * scale) codes of the input's width, reads the bicubic's 4 x 4 footprint: rows
 * y0 - 1 .. y0 + 2, y0 = floor((2 Y + 1 - scale) / (2 scale)), columns likewise.  Tap q = (row ky, column kx) weighs
 *   w_q = max(1, (spatial_tab[Y % scale][ky] * spatial_tab[X % scale][kx] + 128) >> 8) * range_tab[|guide(Y, X) - G_0(q)|],
 * 0 where q lies outside the plane or in(q) is 0, and out = (2 sum w_q in(q) + sum w_q) / (2 sum w_q), 0 (a hole) exactly
 * where no tap is valid.  range_tab: 256 u16, spatial_tab: scale x 4 u16, both ON THE DEVICE and each entry 1 .. 256 (the
 * caller's duty: sum w_q <= 2^20; the sums are 32-bit for u8 codes and 64-bit for u16 codes).  top is checked, not used.
 *
 * codon_jbu_workspace_bytes: HOST ONLY -- the bytes ONE image takes (G_0), a multiple of 16; 0 for a height or width outside
 * 1 .. 4096.  workspace: batch times that, 16-byte aligned, private to the stream.  Two launches, which depend on (batch,
 * height, width, scale) alone; no atomics, no host synchronisation.  Refused on the host, before any HIP call:
 * codon_fill_holes_guided's list, a null spatial_tab, and an out that is not 16-byte aligned. */
size_t codon_jbu_workspace_bytes(int32_t height, int32_t width);
int codon_jbu_upsample(int32_t batch, int32_t height, int32_t width, const void* in, int32_t fmt, int32_t top, const uint8_t* guide,
                       int64_t guide_row_bytes, int64_t guide_image_bytes, int32_t scale, const uint16_t* range_tab,
                       const uint16_t* spatial_tab, void* out, void* workspace, size_t workspace_bytes, codon_stream_t stream);

/* ---- registration of depth maps to the colour camera (codon_amd.register) ---------------------------------------
 * Nothing in the reference: its inputs were registered and upsampled offline.  A DEFINITION, in codon_amd/csrc/register.hip and
 * register_tile.h, restated in numpy in tests/register_ref.py, equal bits required.  Integers only.
 *
 * A depth sensor's map, in its own camera, is projected forwards onto the colour camera's grid under a z-test.  in: (batch,
 * src_height, src_width) codes, 0 a hole.  rays: int32 (src_height + 1, src_width + 1, 3) ON THE DEVICE, shared by the batch:
 * rays[i][j] = rint(2^20 R r) with r the undistorted normalised ray of the source image point (j - 0.5, i - 0.5), the top-left
 * corner of pixel (i, j), and R the depth -> colour rotation; every entry below 2^22 in magnitude (the caller's duty: nothing
 * reads the device here).  trans: int64[3] ON THE HOST, rint(2^20 t / unit) in Q20 codes.  proj: int32[4] ON THE HOST, FX, FY,
 * CX, CY in Q8 pixels of the output grid.  A valid pixel (i, j) with code k has the corners a = (i, j), b = (i + 1, j + 1),
 * c = (i, j + 1), d = (i + 1, j); P_q = k rays[q] + trans.  Any P_q.z < 2^20: dropped.  z' = (((P_a.z + P_b.z + 1) >> 1) + 2^19)
 * >> 20; not 1 <= z' <= top: dropped.  U_q = floor((FX P_q.x + CX P_q.z) / P_q.z), V_q likewise with FY, CY and P_q.y.  The
 * footprint is x0 = (min U + 255) >> 8 .. x1 = ((max U + 255) >> 8) - 1 and y likewise: wider or taller than 8 pixels: dropped;
 * empty: nothing is written; wholly outside the out_height x out_width plane: counted as outside; else clipped to the plane, and
 * every pixel of it takes the minimum of what it holds and z'.  out: (batch, out_height, out_width) codes of the input's width,
 * the minimum where one was written, 0 elsewhere.  stats: NULL, or (batch, 4) uint32 ON THE DEVICE: valid source pixels,
 * outside, dropped, filled target pixels; it needs no initialisation.
 *
 * codon_register_workspace_bytes: HOST ONLY -- the bytes ONE image takes (a u32 per target pixel), a multiple of 16; 0 for a
 * height or width outside 1 .. 4096.  workspace: batch times that, 16-byte aligned, private to the stream; initialised by the
 * call itself, on the stream.  Three launches, which depend on the sizes alone; 32-bit atomic minima and adds on global memory,
 * whose result does not depend on their order; no host synchronisation.  Refused on the host, before any HIP call: null
 * pointers (stats may be NULL), an fmt other than CODON_FILL_U8 / _U16, batch outside 1 .. 65535, a source or target height or
 * width outside 1 .. 4096, top outside 1 .. 65535 or not 255 for u8 codes, |trans| >= 2^38, FX or FY outside 1 .. 2^20 - 1,
 * |CX| or |CY| >= 2^21, out == in, a u16 plane that is not 2-byte aligned, rays or stats not 4-byte aligned, a workspace that
 * is not 16-byte aligned or too small. */
size_t codon_register_workspace_bytes(int32_t out_height, int32_t out_width);
int codon_register_depth(int32_t batch, int32_t src_height, int32_t src_width, const void* in, int32_t fmt, int32_t top,
                         const int32_t* rays, const int64_t* trans, const int32_t* proj, int32_t out_height, int32_t out_width,
                         void* out, uint32_t* stats, void* workspace, size_t workspace_bytes, codon_stream_t stream);

/* ---- outlier rejection of sensor depth maps (codon_amd.clean) ----------------------------------------------------
 * Nothing in the reference: its inputs were cleaned offline, if at all.  A DEFINITION, in codon_amd/csrc/clean.hip and
 * clean_tile.h, restated in numpy in tests/clean_ref.py, equal bits required.  Integers only.
 *
 * in, out: (batch, height, width) codes, u8 or u16, 0 a hole; every output code is the input code or 0.  tau(v) = tol_abs +
 * ((tol_rel_q16 * v) >> 16), the product in unsigned 32 bits; two pixels are LINKED iff both are non-zero and their codes differ
 * by at most tau of the smaller.  Rule 1, flying pixels: a valid pixel with fewer than min_support of its 8 neighbours inside
 * the plane linked to it becomes 0; min_support 0 switches it off; it reads `in`, a single pass, not idempotent.  Rule 2,
 * speckles: the connected components of what rule 1 left, under 4-connectivity, two 4-neighbours in one component iff linked; a
 * component of fewer than min_region pixels becomes 0; min_region <= 1 switches it off.  counts: NULL, or (batch, 4) uint32 ON
 * THE DEVICE: valid inputs, pixels removed by rule 1, pixels removed by rule 2, components removed by rule 2; it needs no
 * initialisation.
 *
 * codon_clean_workspace_bytes: HOST ONLY -- the bytes the batch takes (a u32 label and a u32 size per pixel, each image rounded
 * up to 16 bytes), 0 for a batch outside 1 .. 65535 or a height or width outside 1 .. 4096.  workspace: 16-byte aligned, private
 * to the stream; initialised by the call itself, on the stream.  Two launches with rule 2 off, four with it on: they depend on
 * (batch, height, width) and on that alone; the components are labelled by a lock-free union-find, 32-bit atomic minima on
 * global memory, every loop of it with a trip limit; no host synchronisation.  Refused on the host, before any HIP call: null
 * pointers (counts may be NULL), an fmt other than CODON_FILL_U8 / _U16, batch outside 1 .. 65535, a height or width outside
 * 1 .. 4096, top outside 1 .. 65535 or not 255 for u8 codes, tol_abs outside 0 .. top, tol_rel_q16 outside 0 .. 65535,
 * min_support outside 0 .. 8, min_region outside 0 .. 2^24, out == in, a u16 plane that is not 2-byte aligned, counts not 4-byte
 * aligned, a workspace that is not 16-byte aligned or too small. */
size_t codon_clean_workspace_bytes(int32_t batch, int32_t height, int32_t width);
int codon_clean_depth(int32_t batch, int32_t height, int32_t width, const void* in, int32_t fmt, int32_t top, int32_t tol_abs,
                      int32_t tol_rel_q16, int32_t min_support, int32_t min_region, void* out, uint32_t* counts, void* workspace,
                      size_t workspace_bytes, codon_stream_t stream);

/* ---- spatial smoothing of sensor depth maps (codon_amd.smooth) ---------------------------------------------------
 * Nothing in the reference: its inputs were noise-free renderings.  A DEFINITION, in codon_amd/csrc/smooth.hip and smooth_tile.h,
 * restated in numpy in tests/smooth_ref.py, equal bits required.  Integers only.
 *
 * in, out: (batch, height, width) codes, u8 or u16, 0 a hole.  Two codes are LINKED under codon_clean_depth's rule with tol_abs
 * and tol_rel_q16.  One pass c -> c': a hole stays 0.  For a valid pixel p, S is the set of the positions q != p of the
 * (2 radius + 1)^2 window around p that lie inside the plane and are linked to c_p, every code read from the pass's input; with
 * pairs = 1, q stays in S only if its point mirror 2p - q is in S too.  N = 256 c_p + sum_S W_q c_q, D = 256 + sum_S W_q,
 * c' = floor((2N + D) / (2D)), in unsigned 32 bits (2N + D < 2^32 for radius <= 4 and weights <= 256).  `passes` passes compose.
 * weights: int32 (2 radius + 1)^2 ON THE DEVICE, row-major over (dy, dx): every entry 0 .. 256, symmetric under (dy, dx) ->
 * (-dy, -dx) -- the caller's duty, nothing reads the device here; the entry of the centre is not read.  The hole set of out is
 * that of in; a pass moves a code by at most tol_abs + ((tol_rel_q16 c_p) >> 16); with pairs = 1 a plane with an integer
 * gradient comes back bit for bit, however holes, an occluder or the border cut the windows.  counts: NULL, or (batch, 4) uint32
 * ON THE DEVICE: valid inputs, pixels whose output differs from the input, valid pixels whose S is empty in the first pass, the
 * largest |out - in|; it needs no initialisation.
 *
 * codon_smooth_plan: HOST ONLY -- the launcher's own rule of (radius, passes) (csrc/launch_rules.h) called without a launch:
 * returns the number of filter launches, 0 for a radius outside 1 .. 4 or passes outside 1 .. 3, and with plan != NULL writes
 * plan[0] = the tile's side, plan[1] = the most passes one launch runs at this radius (the fusion bound), plan[2] = the passes
 * of the call's first launch.  codon_smooth_workspace_bytes: HOST ONLY -- the bytes of one set of planes as u16 cells, a multiple
 * of 16; 0 for a batch outside 1 .. 65535 or a height or width outside 1 .. 4096.  workspace: read and written only where
 * codon_smooth_plan answers more than 1 (NULL otherwise is accepted): 16-byte aligned, private to the stream, no initialisation
 * needed.  1 + codon_smooth_plan launches (the statistics to 0; the filter), which depend on (radius, passes) and the sizes
 * alone and not on counts; no host synchronisation.  Refused on the host, before any HIP call: null pointers (counts may be
 * NULL), an fmt other than CODON_FILL_U8 / _U16, batch outside 1 .. 65535, a height or width outside 1 .. 4096, top outside
 * 1 .. 65535 or not 255 for u8 codes, radius outside 1 .. 4, passes outside 1 .. 3, tol_abs outside 0 .. top, tol_rel_q16
 * outside 0 .. 65535, pairs other than 0 or 1, out == in, a u16 plane that is not 2-byte aligned, weights or counts not 4-byte
 * aligned, and, where it is used, a workspace that is NULL, in or out, not 16-byte aligned or too small.  `out` is untouched on
 * a refusal. */
int32_t codon_smooth_plan(int32_t radius, int32_t passes, int32_t* plan);
size_t codon_smooth_workspace_bytes(int32_t batch, int32_t height, int32_t width);
int codon_smooth_depth(int32_t batch, int32_t height, int32_t width, const void* in, int32_t fmt, int32_t top, int32_t radius,
                       int32_t passes, int32_t tol_abs, int32_t tol_rel_q16, int32_t pairs, const int32_t* weights, void* out,
                       uint32_t* counts, void* workspace, size_t workspace_bytes, codon_stream_t stream);

/* ---- temporal filter of a fixed camera's depth sequence (codon_amd.temporal) -------------------------------------
 * Nothing in the reference: it reads single images.  A DEFINITION, in codon_amd/csrc/temporal.hip and temporal_tile.h, restated in
 * numpy in tests/temporal_ref.py, equal bits required.  Integers only.
 *
 * in, out: (frames, height, width) codes, u8 or u16, 0 a hole, frame order being time; frames height width < 2^31.  The window of
 * frame t is the frames s in [max(0, t - back), min(frames - 1, t + ahead)], n_w of them, at most 15.  Two codes are LINKED under
 * codon_clean_depth's rule with tol_abs and tol_rel_q16.  Per pixel and frame, v the input code, every read of `in` (a single
 * pass, not idempotent): 1. v != 0: Lk = the window's samples at that pixel linked to v, v among them, n = |Lk|; if n >=
 * min(min_count, n_w), out = (2 sum Lk + n) / (2 n), the mean rounded half up; otherwise the pixel is REJECTED and goes on with
 * 2.  min_count 1 switches rejection off.  2. v == 0, or rejected: min_fill 0: out = 0.  Otherwise S = the non-zero samples of
 * the window, k = |S|; k < min_fill: out = 0; else m = the lower median of S (rank (k - 1) >> 1 in sorted order), Lm = the samples
 * linked to m, out = the same rounded mean of Lm if |Lm| >= min_fill, else 0.  min_fill is not clamped by n_w.  counts: NULL, or
 * (frames, 4) uint32 ON THE DEVICE: valid inputs, rejected pixels, non-zero outputs where the input was 0 or rejected, accepted
 * pixels whose output differs from the input; it needs no initialisation.
 *
 * Two launches (the statistics to 0; the filter), which depend on (frames, height, width, back, ahead) alone and not on counts;
 * no workspace; no host synchronisation.  A workgroup walks 1024 pixels through one chunk of frames and reads back + ahead frames
 * beyond the chunk's ends.  codon_temporal_chunk_frames: HOST ONLY -- the frames per chunk, the launcher's own rule
 * (csrc/launch_rules.h) called without a launch; 0 for arguments codon_temporal_depth refuses.  Refused on the host, before any
 * HIP call, in this order: null pointers (counts may be NULL), frames outside 1 .. 4096, a height or width outside 1 .. 4096,
 * frames height width of 2^31 or more, an fmt other than CODON_FILL_U8 / _U16, top outside 1 .. 65535 or not 255 for u8 codes,
 * back or ahead below 0 or back + ahead above 14, tol_abs outside 0 .. top, tol_rel_q16 outside 0 .. 65535, min_count outside
 * 1 .. 15, min_fill outside 0 .. 15, out == in (the window reads frames the call would already have overwritten), a u16 plane
 * that is not 2-byte aligned, counts not 4-byte aligned.  `out` is untouched on a refusal. */
int32_t codon_temporal_chunk_frames(int32_t frames, int32_t height, int32_t width, int32_t back, int32_t ahead);
int codon_temporal_depth(int32_t frames, int32_t height, int32_t width, const void* in, int32_t fmt, int32_t top, int32_t back,
                         int32_t ahead, int32_t tol_abs, int32_t tol_rel_q16, int32_t min_count, int32_t min_fill, void* out,
                         uint32_t* counts, codon_stream_t stream);

/* ---- temporal filter of a depth stream, frame by frame (codon_amd.temporal.TemporalStream) ------------------------
 * codon_temporal_depth's definition with the window resident on the device: frames go in one per call and frame t comes out as
 * soon as it is final, with the push of frame t + ahead or, after the last push, with a flush step.  The outputs and counts of a
 * stream of T frames are those of codon_temporal_depth on the (T, height, width) sequence, bit for bit, for any T.
 *
 * The state is the caller's, ON THE DEVICE, private to one stream of frames: ring, codon_temporal_ring_frames() = 16 planes of
 * height x width codes in the stream's format (frame s lives in plane s & 15; no initialisation needed), and state, two uint32 --
 * the frames pushed so far and the flush steps taken since the last push -- which the caller sets to 0 to open a stream.  The
 * parameters must be the same in every call of one stream.
 * A PUSH step (in: height x width codes): pushed += 1, flushed = 0, the frame is stored; with t = pushed - 1 - ahead >= 0 frame t
 * goes to out and its four counts to counts; otherwise neither is written (counts is zeroed).
 * A FLUSH step (in NULL): flushed += 1; with t = max(0, pushed - ahead) + flushed - 1 <= pushed - 1 frame t goes to out, its
 * window cut at the last frame pushed; otherwise nothing is written.  A push after a flush continues the sequence behind the
 * frames already emitted, which is no sequence of the definition: the wrapper refuses it.
 * counts: NULL, or 4 uint32 ON THE DEVICE as in codon_temporal_depth; it needs no initialisation.
 *
 * Two launches per step (the counters and the zeroing; the filter), which depend on (height, width, back, ahead, fmt, in NULL or
 * not) alone -- not on the frame index, which is read from state on the device, and not on counts: a step recorded into a graph
 * replays for every later frame.  No workspace; no host synchronisation.  Refused on the host, before any HIP call, in this
 * order: a height or width outside 1 .. 4096, an fmt other than CODON_FILL_U8 / _U16, top outside 1 .. 65535 or not 255 for u8
 * codes, back or ahead below 0 or back + ahead above 14, tol_abs outside 0 .. top, tol_rel_q16 outside 0 .. 65535, min_count
 * outside 1 .. 15, min_fill outside 0 .. 15, a NULL ring, state or out, out == in, a ring that overlaps in or out, a u16 plane or
 * ring that is not 2-byte aligned, state or counts not 4-byte aligned.  On a refusal out, the ring, state and counts are
 * untouched. */
int32_t codon_temporal_ring_frames(void);
int codon_temporal_push(int32_t height, int32_t width, const void* in, int32_t fmt, int32_t top, int32_t back, int32_t ahead,
                        int32_t tol_abs, int32_t tol_rel_q16, int32_t min_count, int32_t min_fill, void* ring, uint32_t* state,
                        void* out, uint32_t* counts, codon_stream_t stream);

/* ---- depth maps as point clouds with normals (codon_amd.cloud) ---------------------------------------------------
 * Nothing in the reference: it stops at the depth map.  A DEFINITION, in codon_amd/csrc/cloud.hip and cloud_tile.h, restated in
 * numpy in tests/cloud_ref.py, equal bytes required.
 *
 * codes: (batch, height, width) codes, u8 or u16, 0 a hole.  rx (width), ry (height): int32 ON THE DEVICE, the Q20 rays
 * rint(2^20 (j - cx) / fx) and rint(2^20 (i - cy) / fy) of a pinhole camera without distortion; ray_span: ON THE HOST, their four
 * ends rx[0], rx[width - 1], ry[0], ry[height - 1] -- the tables are monotone, so the ends bound them, and the device tables are
 * trusted to be the ones the span describes.  A valid pixel (i, j) with code k has P = (k rx[j], k ry[i], k << 20); its record
 * holds float32(float64(P_c) m) for c = x, y, z (x right, y down, z forward; m = metres per code / 2^20); with normals three more
 * floats N_c 2^-14 of the integer normal of cloud_tile.h (tangents between the pixels `radius` steps away that are linked to k
 * under tol_abs radius + ((tol_rel_q16 min) >> 16), facing the camera, three zeros where there is none); with colour (color:
 * (batch, height, width) u8 for color_channels 1, (batch, height, width, 3) for 3) three more bytes r g b.  Records are 12, 24, 15
 * or 27 bytes, packed, in row-major order of the pixels: image b's start at byte b height width rec of body, which needs no
 * alignment.  counts: (batch, 2) uint32 ON THE DEVICE: records, records with a normal; it needs no initialisation.  normal_map:
 * NULL, or (batch, height, width, 3) u8: 128 + ((127 N_c + 8192) >> 14), and 0 0 0 for a hole or no normal.
 *
 * codon_cloud_workspace_bytes: HOST ONLY -- the bytes the batch takes (a u32 per 1024 pixels, each image rounded up to 16 bytes),
 * 0 for a batch outside 1 .. 65535 or a height or width outside 1 .. 4096.  workspace: 16-byte aligned, private to the stream;
 * initialised by the call itself, on the stream.  Three launches (count, scan, emit), which depend on (batch, height, width) and
 * the record form alone; no atomic decides a position, no workgroup waits for another; no host synchronisation.  Refused on the
 * host, before any HIP call: null pointers (color and normal_map may be NULL), an fmt other than CODON_FILL_U8 / _U16, batch
 * outside 1 .. 65535, a height or width outside 1 .. 4096, top outside 1 .. 65535 or not 255 for u8 codes, normals other than 0
 * or 1, radius outside 1 .. 8, tol_abs outside 0 .. top, tol_rel_q16 outside 0 .. 65535, a ray of the span of 2^22 or more in
 * magnitude, m not positive or not finite, color_channels other than 1 or 3 with colour or 0 without, a normal map without
 * normals, a u16 plane that is not 2-byte aligned, tables or counts not 4-byte aligned, a workspace that is not 16-byte aligned
 * or too small. */
size_t codon_cloud_workspace_bytes(int32_t batch, int32_t height, int32_t width);
int codon_cloud_points(int32_t batch, int32_t height, int32_t width, const void* codes, int32_t fmt, int32_t top, const int32_t* rx,
                       const int32_t* ry, const int32_t* ray_span, double m, int32_t normals, int32_t radius, int32_t tol_abs,
                       int32_t tol_rel_q16, const uint8_t* color, int32_t color_channels, uint8_t* body, uint32_t* counts,
                       uint8_t* normal_map, void* workspace, size_t workspace_bytes, codon_stream_t stream);

/* ---- depth maps as triangle meshes (codon_amd.cloud.triangulate) -------------------------------------------------
 * Nothing in the reference: it stops at the depth map.  A DEFINITION, in codon_amd/csrc/cloud.hip and mesh_tile.h, restated in
 * numpy in tests/mesh_ref.py, equal bytes required.
 *
 * codes: (batch, height, width) codes, u8 or u16, 0 a hole.  The vertices are codon_cloud_points' own: the index of a non-zero code
 * is its rank among the non-zero codes of its plane in row-major order.  Quad (i, j), i < height - 1, j < width - 1, has the corners
 * a = (i, j), b = (i, j + 1), c = (i + 1, j), d = (i + 1, j + 1); two corners are linked under codon_clean_depth's rule with tol_abs
 * for ONE step (sides and diagonals alike) and tol_rel_q16, and a hole links to nothing.  A triangle is emitted when its three
 * corners are pairwise linked.  Four non-zero corners: the diagonal is a-d if |k_a - k_d| <= |k_b - k_c|, else b-c; a-d gives
 * (a, c, d) then (a, d, b), b-c gives (a, c, b) then (b, c, d); each on its own, the other diagonal is not retried.  Three: the one
 * of those four triangles without the missing corner.  Fewer: none.  The orders face the camera (x right, y down, z forward).
 * faces: (batch, 2 (height - 1) (width - 1) 13) bytes, no alignment needed: image b's records are the first counts[b] 13 bytes of its
 * row, in row-major order of the quads, the first-listed triangle first; a record is the byte 3 and three little-endian int32
 * vertex indices, packed (PLY's `property list uchar int vertex_indices`); the bytes behind them are not written.  counts: (batch)
 * uint32 ON THE DEVICE, the faces of each image; it needs no initialisation.  A plane with height 1 or width 1 has no quad: zero
 * faces, and faces may be NULL.
 *
 * codon_cloud_mesh_workspace_bytes: HOST ONLY -- the bytes the batch takes (codon_cloud_workspace_bytes' block words, a u32 per
 * 1024 quads, 8 bytes per image and an int32 per pixel, each part rounded up to 16 bytes), 0 for a batch outside 1 .. 65535 or a
 * height or width outside 1 .. 4096.  workspace: 16-byte aligned, private to the stream; initialised by the call itself, on the
 * stream.  Six launches (vertex count, scan, index plane; face count, scan, emit; the face scan alone for a plane without a quad),
 * which depend on (batch, height, width) alone; no atomic decides a position, no workgroup waits for another; no host
 * synchronisation.  Refused on the host, before any HIP call: null pointers, an fmt other than CODON_FILL_U8 / _U16, batch outside
 * 1 .. 65535, a height or width outside 1 .. 4096, top outside 1 .. 65535 or not 255 for u8 codes, tol_abs outside 0 .. top,
 * tol_rel_q16 outside 0 .. 65535, a u16 plane that is not 2-byte aligned, counts not 4-byte aligned, a workspace that is not
 * 16-byte aligned or too small. */
size_t codon_cloud_mesh_workspace_bytes(int32_t batch, int32_t height, int32_t width);
int codon_cloud_mesh(int32_t batch, int32_t height, int32_t width, const void* codes, int32_t fmt, int32_t top, int32_t tol_abs,
                     int32_t tol_rel_q16, uint8_t* faces, uint32_t* counts, void* workspace, size_t workspace_bytes,
                     codon_stream_t stream);

/* ---- undistortion of colour images (codon_amd.undistort) ---------------------------------------------------------
 * Nothing in the reference: its colour images were rectified offline.  A DEFINITION, in codon_amd/csrc/undistort.hip and
 * undistort_tile.h, restated in numpy in tests/undistort_ref.py, equal bits required.  Integers only.
 *
 * The image of a camera with Brown distortion is resampled to a pinhole camera, the grid codon_register_depth projects onto.
 * in: (batch, src_height, src_width, channels) u8, interleaved, channels 1 (grey) or 3 (RGB); out: (batch, out_height,
 * out_width, channels) u8.  Neither needs any alignment.  map: int32 (out_height, out_width, 2) ON THE DEVICE, shared by the
 * batch: the source position (U, V) of a target pixel in Q5 source pixels, -16 <= U < 32 src_width - 16 and V likewise, or
 * the outside pair (-2^20, -2^20).  weights: int16 (32, 4) ON THE DEVICE: the taps -1, 0, 1, 2 of a cubic at the 32 phases,
 * Q11, sum |weights[p]| <= 2560 (the caller's duty: nothing reads the device here; then every intermediate fits 32 bits).  A
 * pixel that is not outside: xi = U >> 5, px = U & 31, yi and py likewise; tap (r, c) = in[clamp(yi - 1 + r)][clamp(xi - 1 +
 * c)]; row_r = sum_c weights[px][c] tap, acc = sum_r weights[py][r] row_r, out = clamp((acc + 2^21) >> 22, 0, 255) per
 * channel.  An outside pixel is 0 in every channel.
 *
 * tiles: int32 (ceil(out_height / 8), ceil(out_width / 32), 4) ON THE DEVICE = kind, x0, y0, 0 per 32 x 8 tile of target
 * pixels, as codon_undistort_plan wrote it: 0 EMPTY (no pixel inside: zeros), 1 STAGED (the box of every tap of the tile's
 * inside pixels fits the 48 x 24 window from (y0, x0), which the workgroup stages in LDS), 2 DIRECT (taps from global memory).
 * The kind changes how a tile is computed, never what.
 *
 * codon_undistort_tiles_bytes: HOST ONLY -- the bytes of the tile table; 0 for a height or width outside 1 .. 4096.
 * codon_undistort_plan: HOST ONLY, every pointer ON THE HOST -- writes the tile table of a map and counts_host[4]: staged,
 * direct and empty tiles, outside pixels.  Refused: null pointers, a height or width outside 1 .. 4096, and a map entry that is
 * neither the outside pair nor inside the bounds above: a table that passes cannot make a tile read past its window.
 * codon_undistort: one launch, which depends on (batch, out_height, out_width, channels) alone; no workspace, no atomics, no
 * host synchronisation.  Refused on the host, before any HIP call: null pointers, batch outside 1 .. 65535, a source or target
 * height or width outside 1 .. 4096, channels other than 1 or 3, out == in, a map that is not 8-byte aligned, tiles not
 * 16-byte aligned, weights not 2-byte aligned. */
size_t codon_undistort_tiles_bytes(int32_t out_height, int32_t out_width);
int codon_undistort_plan(int32_t src_height, int32_t src_width, int32_t out_height, int32_t out_width, const int32_t* map_host,
                         int32_t* tiles_host, uint32_t* counts_host);
int codon_undistort(int32_t batch, int32_t src_height, int32_t src_width, int32_t channels, const uint8_t* in, int32_t out_height,
                    int32_t out_width, const int32_t* map, const int32_t* tiles, const int16_t* weights, uint8_t* out,
                    codon_stream_t stream);

/* ---- per-image range normalisation of depth codes (codon_amd.upsample.code_range / stretch_codes /
 * unstretch_codes) ---------------------------------------------------------------------------------------------------------
 * No reference counterpart (its data was normalised offline, if at all): a DEFINITION, in codon_amd/csrc/stretch.hip and
 * stretch_tile.h, restated in numpy in tests/stretch_ref.py, equal bits required.  Integers only.
 *
 * A plane of codes on the grid 0 .. top, 0 a hole; T = top - 1.  The range of a plane is (lo, hi), its smallest non-zero and
 * its largest code, (0, 0) without a valid code.  With n = hi - lo, in 64-bit integer division:
 *   stretch:    0 -> 0;  c -> 1 + (2 k T + n) / (2 n),  k = clamp(c, lo, hi) - lo;  n == 0: c -> top
 *   unstretch:  o -> lo + (2 (clamp(o, 1, top) - 1) n + T) / (2 T)
 * A range that is not 1 <= lo <= hi <= top, (0, 0) above all, makes both the identity.  unstretch(stretch(c)) == c for every
 * c in [lo, hi]; a valid code never becomes 0; the range (1, top) makes stretch the identity.
 *
 * codes, in, out: (batch, height, width), contiguous, u8 codes (code_bits 8, top 255) or u16 codes (code_bits 16, 2-byte
 * aligned, top 2 .. 65535); no other alignment is asked of a plane.  lo_hi: (batch, 2) int32 ON THE DEVICE, written by
 * codon_code_range and read by the other two, never by the host; image b is mapped with its own pair.  out may be in.
 * codon_code_range: one launch, one workgroup per image, no atomics, lo_hi needs no initialisation.  codon_stretch_codes,
 * codon_unstretch_codes: one launch each.  The launches depend on (batch, height, width) alone; no host synchronisation.
 * Refused on the host, before any HIP call: null pointers, code_bits other than 8 or 16, batch outside 1 .. 65535, height or
 * width outside 1 .. 16384, top not 255 for u8 codes or outside 2 .. 65535 for u16 codes, an unaligned plane or range. */
int codon_code_range(int32_t batch, int32_t height, int32_t width, const void* codes, int32_t code_bits, int32_t* lo_hi,
                     codon_stream_t stream);
int codon_stretch_codes(int32_t batch, int32_t height, int32_t width, const void* in, int32_t code_bits, int32_t top,
                        const int32_t* lo_hi, void* out, codon_stream_t stream);
int codon_unstretch_codes(int32_t batch, int32_t height, int32_t width, const void* in, int32_t code_bits, int32_t top,
                          const int32_t* lo_hi, void* out, codon_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CODON_HIP_H */
