// Every function of libcodon_hip.so that one translation unit defines and another calls, declared once, grouped by the
// file that defines it.  Included by the definer and by every caller; there is no other prototype of these anywhere.  (A
// definition that drifts from its declaration here is still a LINK error, not a compile error: C++ takes it for an overload.)
#pragma once
#include "codon_common.h"

namespace codon {

struct SensorArgs;   // sensor_pixel.h
struct EvalArgs;     // eval_tile.h
struct NeArgs;       // normal_tile.h

// GB operands of conv1x1_bwd_16 (see WgradC8Params in conv_wgrad_c8.hip); a null pointer = plain codon_conv1x1_bwd
struct Conv1x1GateBwd {
  const float* ch; const float* sp; const float* g_pooled; const float* g_pools; const int* argpix; const int* argch;
  int fbase;
};

// ---- weight gradients: the host layer conv_wgrad_f32.hip, conv_wgrad_f32_t16.hip and conv_wgrad_c8.hip share ----
// Bands per image a planner asks for: enough workgroups to reach `target` per launch (blocks = channel-tile workgroups per
// split), at least one band, at most one per tile row (bounded workspace).  What a planner then makes of it is its own: it
// fixes the partition of the sums, hence the bits (wgrad_plan, wgrad16_plan).
inline int wgrad_band_count(int target, int blocks, int batch, int tiles_y) {
  const int want = (target + blocks * batch - 1) / (blocks * batch);
  return want < 1 ? 1 : want > tiles_y ? tiles_y : want;
}

// The fields WgradParams, WgradT16Params and WgradC8Params have in common, everything else zero.  unit = channels per stored
// element of a plane: 1 for fp32 NCHW floats, 8 for the 16-byte vectors of the channel-blocked 16-bit layout.
template <class P>
inline P wgrad_fill(const codon_conv_desc* d, const void* x, const void* gy, float* workspace, int unit, int nbands, int nsplit) {
  P p{};
  const long HW = (long)d->height * d->width;
  p.x = static_cast<decltype(p.x)>(x); p.gy = static_cast<decltype(p.gy)>(gy); p.ws = workspace;
  p.H = d->height; p.W = d->width; p.cin = d->cin; p.cout = d->cout;
  p.x_img = (d->x_ctotal / unit) * HW; p.g_img = (d->y_ctotal / unit) * HW;
  p.x_base = (d->x_coff / unit) * HW; p.g_base = (d->y_coff / unit) * HW;
  p.tiles_x = (d->width + 31) / 32;
  p.nbands = nbands; p.nsplit = nsplit;
  return p;
}

// adam.hip
int adam_step(const codon_adam_desc* d, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2,
              float eps, float weight_decay, int step, hipStream_t stream);
size_t grad_norm_workspace_bytes();
int grad_norm(const float* grad, long n, void* state, hipStream_t stream);
int adam_step_guarded(const codon_adam_desc* d, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, void* state,
                      float lr, float beta1, float beta2, float eps, float weight_decay, int step, double max_norm,
                      int skip_nonfinite, double ema_decay, hipStream_t stream);

// cac.hip
int cac_stats_tiles(int H, int W);
int cac_stats_fwd(int B, int H, int W, const codon_tensor* pc, const codon_tensor* pd, float* pooled,
                  float* partials, int dtype, hipStream_t stream, const float* chs);
int cac_gate_fwd(int B, int H, int W, const float* partials, const float* w1, const float* b1, const float* w2,
                 const float* b2, float* ch, float* pools_out, hipStream_t stream);
int cac_gate_fwd_n(int B, int ntiles, float inv_hw, const float* partials, const float* w1, const float* b1, const float* w2,
                   const float* b2, float* ch, float* pools_out, hipStream_t stream);
int cac_fused_finish(int B, int H, int W, int ntiles, const float* partials, const float* pool_c, const float* pool_d,
                     float* folded, float* pooled, hipStream_t stream);
int cac_tail_fwd(int B, int H, int W, int ntiles, const float* partials, const float* pool_c, const float* pool_d,
                 const float* pooled_in, float* pooled_out, float* folded, int* counters, const float* w1, const float* b1,
                 const float* w2, const float* b2, const float* ws, float* ch, float* pools_out, float* sp, hipStream_t stream);
int cac_spatial_fwd(int B, int H, int W, const float* pooled, const float* w, float* sp, hipStream_t stream);
int cac_apply_fwd(int B, int H, int W, const codon_tensor* pre, const codon_tensor* pre_c, const float* ch,
                  const float* sp, const codon_tensor* in, const codon_tensor* in_c, const codon_tensor* out,
                  const codon_tensor* out_c, int dtype, hipStream_t stream);
int ew_sq_scale(int B, int H, int W, const codon_tensor* x, const float* ch, const codon_tensor* y, int dtype,
                hipStream_t stream);

// cac_bwd.hip
int cac_bwd_tiles(int H, int W);
int cac_bwd_spatial_blocks(int B, int H, int W);
int cac_bwd_reduce(int B, int H, int W, const codon_tensor* g_out, const codon_tensor* g_outc,
                   const codon_tensor* pre, const codon_tensor* pre_c, const float* ch, const float* sp,
                   const float* pools, float* g_z, float* part_gch, int* part_arg, int dtype, hipStream_t stream);
int cac_bwd_reduce_acc(int B, int H, int W, const codon_tensor* g_out, const codon_tensor* g_outc, const codon_tensor* pre,
                       const codon_tensor* pre_c, const float* ch, const float* sp, const float* pools, const float* pooled,
                       float* g_z, float* part_gch, int* part_arg, int* argch, const codon_tensor* g_in,
                       const codon_tensor* g_in_c, int accumulate_in, int dtype, hipStream_t stream);
int cac_bwd_gate(int B, int H, int W, const float* part_gch, const int* part_arg, const float* ch,
                 const float* pools, const float* w1, const float* b1, const float* w2, float* g_pools, int* argpix,
                 float* part_param, float* dw1, float* db1, float* dw2, float* db2, hipStream_t stream);
int cac_bwd_spatial(int B, int H, int W, const float* g_z, const float* pooled, const float* w, float* g_pooled,
                    float* part_w, float* dw, hipStream_t stream);
int cac_bwd_apply(int B, int H, int W, const codon_tensor* g_out, const codon_tensor* g_outc,
                  const codon_tensor* pre, const codon_tensor* pre_c, const float* ch, const float* sp,
                  const float* pooled, const float* g_pooled, const float* g_pools, const int* argpix,
                  const codon_tensor* g_pre, const codon_tensor* g_pre_c, const codon_tensor* g_in,
                  const codon_tensor* g_in_c, int accumulate_in, int dtype, hipStream_t stream);
int ew_add_mask(int B, int H, int W, int C, const codon_tensor* dst, const codon_tensor* src,
                const codon_tensor* mask, int accumulate, int dtype, hipStream_t stream);
int ew_sum_mask(int B, int H, int W, int C, const codon_tensor* dst, int nsrc, const codon_tensor* const* srcs,
                const codon_tensor* mask, int dtype, hipStream_t stream);

// cast_multi.hip
int cast_multi(const codon_cast_desc* d, float* dst, hipStream_t stream);

// conv_c8.hip
int pack_chain1x1_16(const float* w, void* out, int dtype, hipStream_t stream);
int pack_weight_16(const float* w, void* out, int cout, int cin, int ks, int mode, int dtype, hipStream_t stream);
int conv_form_c8(const codon_conv_desc* d);
int conv2d_fwd_16(const codon_conv_desc* d, const void* x, const void* w, void* y, const void* res, hipStream_t stream);
int conv2d_sum_into_16(const codon_conv_desc* d, const void* x, const void* w, void* y, void* sum, hipStream_t stream);
int conv_chain1x1_fwd_16(const codon_conv_desc* d, const void* x, const void* w, void* y, const void* w_chain,
                         const codon_tensor* out, const codon_tensor* res, float* st_pool, float* st_part, int st_choff,
                         hipStream_t stream);
int conv2d_gated_fwd_16(const codon_conv_desc* d, const void* pre, const codon_tensor* inputs, const float* ch,
                        const float* sp, const void* w, void* y, const codon_tensor* gated_out, hipStream_t stream);
int cac_fused_tiles(int H, int W);

// conv_mfma_f32.hip
int pack_chain1x1_f32(const float* w, float* out, hipStream_t stream);
int conv_ck(int ks);
int conv_tiling_f32(const codon_conv_desc* d, int chained, int in_pair);
int conv2d_gated_fwd_f32(const codon_conv_desc* d, const float* pre, const codon_tensor* in2, const float* ch,
                         const float* sp, const float* w, float* y, const codon_tensor* gated_out, hipStream_t stream);
int conv_chain1x1_fwd_f32(const codon_conv_desc* d, const float* x, const float* w, float* y, const float* w_chain,
                          const codon_tensor* out, const codon_tensor* res, float* st_pool, float* st_part, int st_choff,
                          hipStream_t stream);
int conv2d_fwd_f32(const codon_conv_desc* d, const float* x, const float* w, float* y, const float* res,
                   hipStream_t stream);
int pack_weight_f32(const float* w, float* out, int cout, int cin, int ks, int mode, hipStream_t stream);

// conv_mfma_f32x3.hip
int pack_chain1x1_f32x3(const float* w, void* out, hipStream_t stream);
int conv_chain1x1_fwd_f32x3(const codon_conv_desc* d, const float* x, const void* w, float* y, const void* w_chain,
                            const codon_tensor* out, const codon_tensor* res, hipStream_t stream);
bool conv_f32x3_supported(const codon_conv_desc* d);
int conv2d_fwd_f32x3(const codon_conv_desc* d, const float* x, const void* w, float* y, const float* res,
                     hipStream_t stream);
int pack_weight_f32x3(const float* w, void* out, int cout, int cin, int ks, hipStream_t stream);

// conv_wgrad_c8.hip
size_t conv_wgrad_16_workspace_bytes(const codon_conv_desc* d);
int conv2d_wgrad_16(const codon_conv_desc* d, const void* x, const void* gy, float* dw, float* workspace,
                    size_t ws_bytes, int accumulate, hipStream_t stream);
int conv1x1_bwd_16(const codon_conv_desc* d, const void* x, const void* gy, const void* w_dgrad, const codon_tensor* gx,
                   float* dw, float* workspace, size_t ws_bytes, int accumulate, hipStream_t stream,
                   const Conv1x1GateBwd* gb);

// conv_wgrad_f32.hip
// dw[co][ci][tap] (+)= sum_s ws[s][tap][co][ci], fixed order over s
int launch_wgrad_reduce(const float* ws, float* dw, int cout, int cin, int taps, int nsplit, int accumulate,
                        hipStream_t stream);
size_t conv_wgrad_workspace_bytes(const codon_conv_desc* d);
int conv2d_wgrad_f32(const codon_conv_desc* d, const float* x, const float* gy, float* dw, float* workspace,
                     size_t ws_bytes, int accumulate, hipStream_t stream);

// conv_wgrad_f32_t16.hip: 16x16x4 tiles, 8 balanced waves, double-buffered (W % 4 == 0, 16-byte aligned slices, k in {1,3,5})
bool conv_wgrad_f32_t16_shape(const codon_conv_desc* d);
bool conv_wgrad_f32_t16_supported(const codon_conv_desc* d, const void* x, const void* gy);
int launch_wgrad_f32_t16(const codon_conv_desc* d, const float* x, const float* gy, float* workspace, int nbands,
                         int nsplit, hipStream_t stream);

// d4.hip
int d4_views(int B, int H, int W, const void* src0, const void* src1, int dtype, void* up0, void* tp0, void* up1, void* tp1,
             hipStream_t stream);
int d4_merge(int B, int H, int W, const void* upright, const void* transposed, int dtype, float* out, hipStream_t stream);

// eval.hip
int depth_errors(const EvalArgs& a, int B, int bits, const void* label, const void* out, void* err, unsigned char* region,
                 unsigned long long* acc, hipStream_t stream);

// normal_errors.hip; rx (W), ry (H), ctab and stab (1440 each): int32 on the device; words: (B, 1448) u32; amap: null or (B, H, W) u16
int normal_errors(const NeArgs& a, int B, int fmt, const void* label, const void* out, const int* rx, const int* ry, const int* ctab,
                  const int* stab, unsigned* words, unsigned short* amap, hipStream_t stream);

// fill_holes.hip
size_t fill_holes_workspace_bytes(int h, int w);
int fill_holes(int B, int h, int w, const void* in, int fmt, const float* tab, int top, void* out, void* workspace,
               hipStream_t stream);

// fill_guided.hip; guide: u8 rows row_bytes apart, images image_bytes apart; range_tab: 256 u16
size_t fill_guided_workspace_bytes(int h, int w);
int fill_holes_guided(int B, int h, int w, const void* in, int fmt, int top, const void* guide, long row_bytes, long image_bytes,
                      int scale, const void* range_tab, void* out, void* workspace, hipStream_t stream);

// jbu.hip; guide as fill_guided.hip's; range_tab: 256 u16, spatial_tab: scale x 4 u16; out: (B, h * scale, w * scale) codes
size_t jbu_workspace_bytes(int h, int w);
int jbu_upsample(int B, int h, int w, const void* in, int fmt, const void* guide, long row_bytes, long image_bytes, int scale,
                 const void* range_tab, const void* spatial_tab, void* out, void* workspace, hipStream_t stream);

// register.hip; rays: (hs + 1, ws + 1, 3) int32 on the device; trans (3) and proj (4) on the host; stats: (B, 4) u32 or null;
// workspace: B u32 planes of ho x wo
size_t register_workspace_bytes(int ho, int wo);
int register_depth(int B, int hs, int ws, const void* in, int fmt, int top, const void* rays, const long long* trans, const int* proj,
                   int ho, int wo, void* out, void* stats, void* workspace, hipStream_t stream);

// clean.hip; stats: (B, 4) u32 or null; workspace: a u32 label plane and a u32 size plane of B images
size_t clean_workspace_bytes(int B, int h, int w);
int clean_depth(int B, int h, int w, const void* in, int fmt, int tol_abs, int tol_rel_q16, int min_support, int min_region, void* out,
                void* stats, void* workspace, hipStream_t stream);

// cloud.hip; rx (w), ry (h): int32 on the device; radius 0: records without normals; color: null, or (B, h, w, channels) u8; body:
// (B, h w rec) bytes; counts: (B, 2) u32; nmap: null or (B, h, w, 3) u8; workspace: a u32 per 1024 pixels of every image
size_t cloud_workspace_bytes(int B, int h, int w);
int cloud_points(int B, int h, int w, const void* in, int fmt, const int* rx, const int* ry, double m, int radius, int tol_abs,
                 int tol_rel_q16, const void* color, int channels, void* body, void* counts, void* nmap, void* workspace,
                 hipStream_t stream);
// smooth.hip; weights: (2 radius + 1)^2 int32 on the device; stats: (B, 4) u32 or null; workspace: one plane set of u16 cells,
// read and written only where smooth_launches(radius, passes) > 1 (may be null otherwise)
size_t smooth_workspace_bytes(int B, int h, int w);
int smooth_depth(int B, int h, int w, const void* in, int fmt, int radius, int passes, int tol_abs, int tol_rel_q16, int pairs,
                 const void* weights, void* out, void* stats, void* workspace, hipStream_t stream);
// temporal.hip; in, out: (T, h, w) codes, T h w below 2^31; stats: (T, 4) u32 or null; no workspace
int temporal_depth(int T, int h, int w, const void* in, int fmt, int back, int ahead, int tol_abs, int tol_rel_q16, int min_count,
                   int min_fill, void* out, void* stats, hipStream_t stream);
// temporal_push.hip; in: (h, w) codes or null (a flush step); ring: 16 planes of (h, w) codes; state: 2 u32; out: (h, w) codes;
// stats: 4 u32 or null; no workspace
int temporal_push(int h, int w, const void* in, int fmt, int back, int ahead, int tol_abs, int tol_rel_q16, int min_count,
                  int min_fill, void* ring, void* state, void* out, void* stats, hipStream_t stream);

// cloud.hip, mesh_tile.h; faces: (B, 2 (h - 1) (w - 1) 13) bytes; counts: (B) u32; workspace: the cloud's block words, a u32 per
// 1024 quads of every image, (B, 2) u32 and the (B, h, w) int32 index plane
size_t cloud_mesh_workspace_bytes(int B, int h, int w);
int cloud_mesh(int B, int h, int w, const void* in, int fmt, int tol_abs, int tol_rel_q16, void* faces, void* counts, void* workspace,
               hipStream_t stream);

// undistort.hip; in: (B, hs, ws, channels) u8, out: (B, ho, wo, channels) u8; map (ho, wo, 2) int32, tiles (the words of
// undistort_tiles_bytes) and weights (32, 4) int16 on the device.  undistort_plan: HOST -- the tile table and the four counts of a
// host copy of the map; -1, or the index of the first entry it refuses
size_t undistort_tiles_bytes(int ho, int wo);
long undistort_plan(int hs, int ws, int ho, int wo, const int* map, int* tiles, unsigned* counts);
int undistort(int B, int hs, int ws, int channels, const void* in, int ho, int wo, const void* map, const void* tiles,
              const void* weights, void* out, hipStream_t stream);

// stretch.hip; fmt: ST_U8 / ST_U16, dir: ST_STRETCH / ST_UNSTRETCH (stretch_tile.h); n: codes per image
int code_range(int B, long n, const void* codes, int fmt, int* lo_hi, hipStream_t stream);
int map_codes(int dir, int B, long n, const void* in, int fmt, int top, const int* lo_hi, void* out, hipStream_t stream);

// ew_c8.hip: the stencils, CAC passes and elementwise helpers of stencil.hip, cac.hip and cac_bwd.hip over channel-blocked 16-bit tensors
int stem_pair_fwd_c8(int B, int H, int W, const float* xa, const float* wa, void* ya, int ya_ctotal, int ya_coff,
                     const float* xb, const float* wb, void* yb, int yb_ctotal, int yb_coff, int dtype, int* bad, int* host_a,
                     int* host_b, hipStream_t stream);
int stem_fwd_c8(int B, int H, int W, const float* x, const float* w, void* y, int y_ctotal, int y_coff, int flags,
                const void* mask, int m_ctotal, int m_coff, int dtype, int* bad, int* host, hipStream_t stream);
int head_fwd_c8(int B, int H, int W, const void* x, int x_ctotal, int x_coff, const float* w, const float* res, void* y,
                bool y16, int dtype, const int* bad, hipStream_t stream);
size_t conv1ch_wgrad_c8_workspace_bytes(int B, int H, int W);
int conv1ch_wgrad_c8(int B, int H, int W, const void* a, int a_ctotal, int a_coff, const float* s, float* dw, int flip,
                     float* ws, size_t ws_bytes, int dtype, hipStream_t stream);
int cac_stats_fwd_c8(int B, int H, int W, const codon_tensor* pc, const codon_tensor* pd, float* pooled, float* partials,
                     int dtype, hipStream_t stream, const float* chs);
int cac_apply_fwd_c8(int B, int H, int W, const codon_tensor* pre, const codon_tensor* pre_c, const float* ch,
                     const float* sp, const codon_tensor* in, const codon_tensor* in_c, const codon_tensor* out,
                     const codon_tensor* out_c, int dtype, hipStream_t stream);
int ew_sq_scale_c8(int B, int H, int W, const codon_tensor* x, const float* ch, const codon_tensor* y, int dtype,
                   hipStream_t stream);
int ew_add_mask_c8(int B, int H, int W, int C, const codon_tensor* dst, const codon_tensor* src, const codon_tensor* mask,
                   int accumulate, int dtype, hipStream_t stream);
int ew_sum_mask_c8(int B, int H, int W, int C, const codon_tensor* dst, int nsrc, const codon_tensor* const* srcs,
                   const codon_tensor* mask, int dtype, hipStream_t stream);
int cac_bwd_reduce_c8(int B, int H, int W, const codon_tensor* g_out, const codon_tensor* g_outc, const codon_tensor* pre,
                      const codon_tensor* pre_c, const float* ch, const float* sp, const float* pools, float* g_z,
                      float* part_gch, int* part_arg, int dtype, hipStream_t stream, const float* pooled, int* argch,
                      const codon_tensor* g_in, const codon_tensor* g_in_c, int accumulate_in);
int cac_bwd_apply_c8(int B, int H, int W, const codon_tensor* g_out, const codon_tensor* g_outc, const codon_tensor* pre,
                     const codon_tensor* pre_c, const float* ch, const float* sp, const float* pooled, const float* g_pooled,
                     const float* g_pools, const int* argpix, const codon_tensor* g_pre, const codon_tensor* g_pre_c,
                     const codon_tensor* g_in, const codon_tensor* g_in_c, int accumulate_in, int dtype, hipStream_t stream);

// metrics.hip
int postprocess_u8(const float* x, unsigned char* o, long n, hipStream_t stream);
int postprocess_u8_f16(const void* x, unsigned char* o, long n, hipStream_t stream);
int masked_sqerr(const unsigned char* label, const unsigned char* out, long n, unsigned long long* acc, hipStream_t stream);
int masked_sqerr_u16(const unsigned short* label, const unsigned short* out, long n, unsigned long long* acc,
                     hipStream_t stream);
int postprocess_u16(const void* x, int dtype, int depth_max, unsigned short* o, long n, hipStream_t stream);
int ssim_tiles(int B, int H, int W);
int ssim_fwd(int B, int H, int W, const float* a, const float* b, float* partial, float* dmaps, double* value,
             hipStream_t stream);
int l1_fwd(long n, const float* a, const float* b, float* partial, int nparts, double* value, hipStream_t stream);
int ssim_l1_bwd(int B, int H, int W, const float* a, const float* b, const float* dmaps, float* tmp, float* ga,
                float ssim_scale, float l1_scale, hipStream_t stream);
int masked_l1_ssim_fwd(int B, int H, int W, const float* a, const float* b, const unsigned char* valid, float* ws,
                       float* dmaps, double w_l1, double w_ssim, long long* counts, double* per_image, float* scales,
                       double* value, hipStream_t stream);
int masked_l1_ssim_bwd(int B, int H, int W, const float* a, const float* b, const unsigned char* valid, const float* dmaps,
                       const float* scales, const float* gup, float* tmp, float* ga, hipStream_t stream);

// reduce_multi.hip
int reduce_multi(const codon_reduce_item* items, int n_items, hipStream_t stream);

// resample_masked.hip
int train_crops_lr(const codon_crop_desc* d, const unsigned char* pool, int s, int code_bits, const float* lut, int levels,
                   const float* lut8, const float* wtab, float* x, float* guide, float* target, hipStream_t stream);
int bicubic_upsample_masked(int B, int h, int w, int s, const float* lr, const float* wtab, float* out, unsigned char* valid,
                            hipStream_t stream);
int bicubic_downsample_masked(int B, int P, int s, const float* hr, const float* wtab, const float* lut, int levels, float* out,
                              hipStream_t stream);
int lr_codes_to_input(int B, int h, int w, int s, const void* codes, int code_bits, const float* lut, int levels,
                      const float* wtab, void* out, int dtype, hipStream_t stream);
int lr_codes_upsample(int B, int h, int w, int s, const void* codes, int code_bits, const float* lut, int levels,
                      const float* wtab, void* out, hipStream_t stream);

// sensor.hip
int lr_sensor(const SensorArgs& a, int B, const float* lr, const float* gauss, const float* lut, float* out,
              hipStream_t stream);

// stencil.hip
int stem_fwd(int B, int H, int W, const float* x, const float* w, void* y, int y_ctotal, int y_coff, int flags,
             const void* mask, int m_ctotal, int m_coff, int dtype, int* bad, int* host, hipStream_t stream);
int stem_pair_fwd(int B, int H, int W, const float* xa, const float* wa, void* ya, int ya_ctotal, int ya_coff,
                  const float* xb, const float* wb, void* yb, int yb_ctotal, int yb_coff, int dtype, int* bad, int* host_a,
                  int* host_b, hipStream_t stream);
int head_fwd(int B, int H, int W, const void* x, int x_ctotal, int x_coff, const float* w, const float* res, void* y,
             bool y16, int dtype, const int* bad, hipStream_t stream);
// dw[576] = fixed-order sum of the (nparts, 576) partials
int conv1ch_wgrad_reduce(const float* part, float* dw, int nparts, int flip, hipStream_t stream);
size_t conv1ch_wgrad_workspace_bytes(int B, int H, int W);
int conv1ch_wgrad(int B, int H, int W, const void* a, int a_ctotal, int a_coff, const float* s, float* dw, int flip,
                  float* ws, size_t ws_bytes, int dtype, hipStream_t stream);

// train_data.hip
int train_crops(const codon_crop_desc* d, const unsigned char* pool, int bits, const float* lut, const float* lut8,
                float* source, float* guide, float* target, hipStream_t stream);
int bicubic_downsample(int B, int P, int s, const float* hr, const float* wtab, float* out, hipStream_t stream);
int quantize_levels(long n, float* x, const float* lut, int levels, hipStream_t stream);

// upsample.hip
int bicubic_upsample(int B, int h, int w, int s, const float* lr, const float* wtab, float* out, hipStream_t stream);

// wsum.hip
size_t weight_checksum_workspace_bytes();
int weight_checksum(const codon_wsum_desc* d, void* ws, unsigned long long* ref, int mode, int* flag, int* zero, int nzero,
                    hipStream_t s);

}  // namespace codon
