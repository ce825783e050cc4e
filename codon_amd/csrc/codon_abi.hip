// extern "C" surface of libcodon_hip.so (see include/codon_hip.h): argument validation, dtype
// dispatch, error strings.  Never throws, never allocates device memory, never synchronises.

#include <math.h>
#include <stdarg.h>
#include <string.h>

#include "codon_common.h"
#include "eval_tile.h"
#include "fill_tile.h"
#include "kernels.h"
#include "launch_rules.h"
#include "pair.h"
#include "register_tile.h"
#include "clean_tile.h"
#include "cloud_tile.h"
#include "mesh_tile.h"
#include "normal_tile.h"
#include "sensor_pixel.h"
#include "smooth_tile.h"
#include "stretch_tile.h"
#include "temporal_tile.h"
#include "train_record.h"
#include "undistort_tile.h"

namespace codon {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return CODON_ERR_LAUNCH;
  }
  return CODON_OK;
}

static thread_local PairRecorder g_pair;
PairRecorder* pair_recorder() { return g_pair.active ? &g_pair : nullptr; }

// channels [coff, coff + c) lie inside a buffer of ctotal channels (whole 8-channel planes are the 16-bit launchers' rule, c8.h)
static bool in_bounds(int coff, int c, int ctotal) { return coff >= 0 && coff + c <= ctotal; }
static bool slice_ok(const codon_tensor* t, int c = 64) { return t && t->data && in_bounds(t->coff, c, t->ctotal); }
// the slices of a conv descriptor: x always, y (cout channels of y_*) and the residual slot (cout channels of r_*) when used
static bool conv_slices_ok(const codon_conv_desc* d, bool with_y, bool with_res) {
  return in_bounds(d->x_coff, d->cin, d->x_ctotal) && (!with_y || in_bounds(d->y_coff, d->cout, d->y_ctotal)) &&
         (!with_res || in_bounds(d->r_coff, d->cout, d->r_ctotal));
}

static bool is16(int dtype) { return dtype == CODON_BF16 || dtype == CODON_F16; }
static bool dtype_known(int dtype) { return dtype == CODON_F32 || is16(dtype); }

static bool shape_ok(int b, int h, int w) { return b > 0 && h > 0 && w > 0 && (long)h * w < (1L << 31); }

// The descriptor of a codon_train_crops* entry `name` against a pool of records of one layout (train_record.h): the batch,
// the crop, and per sample the window inside its image and the whole record inside the pool.  lr_scale != 0: the image
// sizes are multiples of it.  Nothing is launched before every sample has passed.
static int check_crop_desc(const char* name, const codon_crop_desc* desc, int64_t pool_bytes, int bits, bool label,
                           int lr_scale) {
  CODON_REQUIRE(desc->n >= 1 && desc->n <= CODON_TRAIN_MAX_BATCH, CODON_ERR_BAD_ARG, "%s: batch %d (1..%d)", name, desc->n,
                CODON_TRAIN_MAX_BATCH);
  const int P = desc->crop;
  CODON_REQUIRE(P >= 1 && P <= 2048, CODON_ERR_BAD_ARG, "%s: crop %d (1..2048)", name, P);
  for (int b = 0; b < desc->n; ++b) {
    const codon_crop_sample& c = desc->s[b];
    CODON_REQUIRE(lr_scale == 0 || (c.height >= 1 && c.width >= 1 && c.height % lr_scale == 0 && c.width % lr_scale == 0),
                  CODON_ERR_BAD_ARG, "%s: sample %d: %dx%d is no multiple of the scale %d", name, b, c.height, c.width,
                  lr_scale);
    CODON_REQUIRE(c.height >= P && c.width >= P && c.y0 >= 0 && c.x0 >= 0 && c.y0 <= c.height - P && c.x0 <= c.width - P &&
                      c.op >= 0 && c.op <= 7,
                  CODON_ERR_BAD_ARG, "%s: sample %d: %dx%d crop at (%d, %d) op %d outside the image", name, b, c.height,
                  c.width, c.y0, c.x0, c.op);
    CODON_REQUIRE(c.offset >= 0 && (bits == 8 || c.offset % 2 == 0), CODON_ERR_BAD_ARG,
                  "%s: sample %d: offset %lld is negative, or odd (u16 planes start at even bytes)", name, b,
                  (long long)c.offset);
    CODON_REQUIRE(c.offset <= pool_bytes - record_layout(bits, label, lr_scale, c.height, c.width).size, CODON_ERR_BAD_ARG,
                  "%s: sample %d: the record at offset %lld runs past the %lld-byte pool", name, b, (long long)c.offset,
                  (long long)pool_bytes);
  }
  return CODON_OK;
}

// ---- the checks the code-plane entries share: `who` is the entry's name in the message.  An entry calls them in
// the order its refusals are documented in -- of two broken rules the first is reported -- so each is one rule, and
// check_planes is the run of four that most entries have unbroken.
static int check_fmt(const char* who, int fmt) {
  CODON_REQUIRE(fmt == FL_U8 || fmt == FL_U16, CODON_ERR_BAD_ARG, "%s: fmt %d (0: u8 codes, 1: u16 codes)", who, fmt);
  return CODON_OK;
}

static int check_batch(const char* who, int batch) {
  CODON_REQUIRE(batch >= 1 && batch <= 65535, CODON_ERR_BAD_ARG, "%s: batch %d (1..65535)", who, batch);
  return CODON_OK;
}

// noun: what the message calls the plane ("plane", "source", "target")
static int check_side(const char* who, int height, int width, const char* noun, int limit) {
  CODON_REQUIRE(height >= 1 && height <= limit && width >= 1 && width <= limit, CODON_ERR_BAD_ARG, "%s: a %dx%d %s (1..%d each way)",
                who, height, width, noun, limit);
  return CODON_OK;
}

static int check_top(const char* who, int fmt, int top) {
  CODON_REQUIRE(top >= 1 && top <= 65535 && (fmt != FL_U8 || top == 255), CODON_ERR_BAD_ARG,
                "%s: top %d (255 for u8 codes, 1..65535 otherwise)", who, top);
  return CODON_OK;
}

// format (codes only), batch, a "plane" of at most `limit` each way, top
static int check_planes(const char* who, int fmt, int batch, int height, int width, int limit, int top) {
  if (const int st = check_fmt(who, fmt)) return st;
  if (const int st = check_batch(who, batch)) return st;
  if (const int st = check_side(who, height, width, "plane", limit)) return st;
  return check_top(who, fmt, top);
}

// the strided guidance image of the guided filler and of the joint bilateral upsampler, and the scale it is at
static int check_guide(const char* who, int batch, int height, int width, int scale, int64_t row_bytes, int64_t image_bytes) {
  CODON_REQUIRE(scale == 4 || scale == 8 || scale == 16, CODON_ERR_BAD_ARG, "%s: scale %d (4, 8 or 16)", who, scale);
  CODON_REQUIRE(row_bytes >= (int64_t)width * scale, CODON_ERR_BAD_ARG,
                "%s: guide rows of %lld bytes (at least %lld: width times scale)", who, (long long)row_bytes, (long long)width * scale);
  CODON_REQUIRE(batch == 1 || image_bytes >= (int64_t)height * scale * row_bytes, CODON_ERR_BAD_ARG,
                "%s: guide images %lld bytes apart (at least %lld: height times scale rows)", who, (long long)image_bytes,
                (long long)height * scale * row_bytes);
  return CODON_OK;
}

// the link rule's two tolerances (clean_tile.h, cloud_tile.h): codes up to top, and a Q16 fraction up to max_rel
static int check_link_tolerances(const char* who, int tol_abs, int top, int tol_rel_q16, int max_rel) {
  CODON_REQUIRE(tol_abs >= 0 && tol_abs <= top, CODON_ERR_BAD_ARG, "%s: tolerance %d (codes, 0..top = %d)", who, tol_abs, top);
  CODON_REQUIRE(tol_rel_q16 >= 0 && tol_rel_q16 <= max_rel, CODON_ERR_BAD_ARG, "%s: tolerance_rel %d (Q16, 0..%d)", who, tol_rel_q16,
                max_rel);
  return CODON_OK;
}

// in_name: what the message calls the input ("in", "codes")
static int check_not_same(const char* who, const void* in, const void* out, const char* in_name = "in") {
  CODON_REQUIRE(in != out, CODON_ERR_BAD_ARG, "%s: %s and out are the same buffer", who, in_name);
  return CODON_OK;
}

static int check_workspace(const char* who, size_t workspace_bytes, size_t need) {
  CODON_REQUIRE(workspace_bytes >= need, CODON_ERR_BAD_ARG, "%s: a workspace of %zu bytes is too small (%zu needed)", who,
                workspace_bytes, need);
  return CODON_OK;
}

static int check_code_bits(const char* who, int code_bits) {
  CODON_REQUIRE(code_bits == 8 || code_bits == 16, CODON_ERR_BAD_ARG, "%s: code_bits %d (8 or 16)", who, code_bits);
  return CODON_OK;
}

// the low-resolution code planes of the lr_codes_* entries and their output at `scale`: grid, shape, alignment
static int check_lr_codes(const char* who, int batch, int lr_height, int lr_width, int scale, const void* codes, int code_bits,
                          int depth_max, const void* out) {
  if (const int st = check_code_bits(who, code_bits)) return st;
  CODON_REQUIRE(code_bits == 16 ? (depth_max >= 1 && depth_max <= 65535) : depth_max == 255, CODON_ERR_BAD_ARG,
                "%s: depth_max %d (255 for 8-bit codes, 1..65535 for 16-bit codes)", who, depth_max);
  CODON_REQUIRE(lr_height >= 1 && lr_width >= 1 && lr_height <= 65536 && lr_width <= 65536 &&
                    shape_ok(batch, lr_height * scale, lr_width * scale),
                CODON_ERR_BAD_ARG, "%s: bad shape", who);
  CODON_REQUIRE(((uintptr_t)out & 15) == 0 && (code_bits == 8 || ((uintptr_t)codes & 1) == 0), CODON_ERR_BAD_ARG,
                "%s: out must be 16-byte aligned and u16 codes 2-byte aligned", who);
  return CODON_OK;
}

}  // namespace codon

using namespace codon;

extern "C" {

int codon_abi_version(void) { return CODON_ABI_VERSION; }

const char* codon_last_error_string(void) { return g_err; }

#ifndef CODON_SOURCE_HASH
#define CODON_SOURCE_HASH "unknown"
#endif
const char* codon_build_source_hash(void) { return CODON_SOURCE_HASH; }

size_t codon_conv_packed_weight_bytes(int32_t cout, int32_t cin, int32_t ksize, int32_t dtype) {
  if (cout <= 0 || cin <= 0 || (ksize != 1 && ksize != 3 && ksize != 5)) return 0;
  return (size_t)cout * cin * ksize * ksize * (dtype == CODON_F32 ? 4 : 2);
}

int codon_conv_pack_weight(const float* w_oihw, void* w_packed, int32_t cout, int32_t cin, int32_t ksize,
                           int32_t mode, int32_t dtype, codon_stream_t stream) {
  CODON_REQUIRE(w_oihw && w_packed, CODON_ERR_BAD_ARG, "conv_pack_weight: null pointer");
  CODON_REQUIRE(ksize == 1 || ksize == 3 || ksize == 5, CODON_ERR_UNSUPPORTED, "conv_pack_weight: ksize %d", ksize);
  if (mode == CODON_PACK_FWD_F16X3) {
    CODON_REQUIRE(dtype == CODON_F32 && (ksize == 3 || ksize == 5) && cin % 16 == 0 && cout % 64 == 0,
                  CODON_ERR_UNSUPPORTED, "conv_pack_weight: f16x3 packing needs fp32, k in {3,5}, cin%%16==0, cout%%64==0");
    return pack_weight_f32x3(w_oihw, w_packed, cout, cin, ksize, (hipStream_t)stream);
  }
  if (mode == CODON_PACK_CHAIN1X1 || mode == CODON_PACK_CHAIN1X1_F16X3) {
    CODON_REQUIRE(ksize == 1 && cin == 128 && cout == 64, CODON_ERR_UNSUPPORTED,
                  "conv_pack_weight: CHAIN1X1 packs the (64,128,1,1) weights only");
    if (mode == CODON_PACK_CHAIN1X1_F16X3) {
      CODON_REQUIRE(dtype == CODON_F32, CODON_ERR_UNSUPPORTED, "conv_pack_weight: CHAIN1X1_F16X3 is for fp32 tensors");
      return pack_chain1x1_f32x3(w_oihw, w_packed, (hipStream_t)stream);
    }
    if (is16(dtype)) return pack_chain1x1_16(w_oihw, w_packed, dtype, (hipStream_t)stream);
    CODON_REQUIRE(dtype == CODON_F32, CODON_ERR_UNSUPPORTED, "conv_pack_weight: CHAIN1X1 dtype %d", dtype);
    return pack_chain1x1_f32(w_oihw, (float*)w_packed, (hipStream_t)stream);
  }
  CODON_REQUIRE(mode == CODON_PACK_FWD || mode == CODON_PACK_DGRAD, CODON_ERR_BAD_ARG, "conv_pack_weight: mode %d", mode);
  const int kin = mode == CODON_PACK_DGRAD ? cout : cin;
  CODON_REQUIRE(cout > 0 && cin > 0 && kin % conv_ck(ksize) == 0, CODON_ERR_UNSUPPORTED,
                "conv_pack_weight: cin=%d cout=%d not a multiple of the channel chunk", cin, cout);
  if (is16(dtype)) {
    CODON_REQUIRE(kin % 16 == 0, CODON_ERR_UNSUPPORTED, "conv_pack_weight: 16-bit packing needs cin %% 16 == 0");
    return pack_weight_16(w_oihw, w_packed, cout, cin, ksize, mode, dtype, (hipStream_t)stream);
  }
  CODON_REQUIRE(dtype == CODON_F32, CODON_ERR_UNSUPPORTED, "conv_pack_weight: dtype %d", dtype);
  return pack_weight_f32(w_oihw, (float*)w_packed, cout, cin, ksize, mode, (hipStream_t)stream);
}

int codon_conv2d_fwd(const codon_conv_desc* d, const void* x, const void* w_packed, void* y, const void* residual,
                     codon_stream_t stream) {
  CODON_REQUIRE(d && x && w_packed && y, CODON_ERR_BAD_ARG, "conv2d_fwd: null pointer");
  CODON_REQUIRE(shape_ok(d->batch, d->height, d->width), CODON_ERR_BAD_ARG, "conv2d_fwd: bad shape %dx%dx%d",
                d->batch, d->height, d->width);
  CODON_REQUIRE(in_bounds(d->x_coff, d->cin, d->x_ctotal), CODON_ERR_BAD_ARG,
                "conv2d_fwd: input slice [%d,%d) outside %d channels", d->x_coff, d->x_coff + d->cin, d->x_ctotal);
  CODON_REQUIRE(in_bounds(d->y_coff, d->cout, d->y_ctotal), CODON_ERR_BAD_ARG,
                "conv2d_fwd: output slice [%d,%d) outside %d channels", d->y_coff, d->y_coff + d->cout, d->y_ctotal);
  // only the public CODON_CONV_* bits: the kernels keep internal selector bits above them (conv_c8.hip: a read-write running
  // sum in the residual slot), which no caller of THIS entry point may reach -- `residual` is const here
  CODON_REQUIRE((d->flags & ~(CODON_CONV_RELU | CODON_CONV_ADD_RESIDUAL | CODON_CONV_ACCUM_OUT | CODON_CONV_MASK_RELU |
                              CODON_CONV_F16X3 | CODON_CONV_MASK_SUM)) == 0,
                CODON_ERR_BAD_ARG, "conv2d_fwd: unknown flag bits 0x%x", (unsigned)d->flags);
  CODON_REQUIRE(!((d->flags & CODON_CONV_ADD_RESIDUAL) && (d->flags & CODON_CONV_MASK_RELU)), CODON_ERR_BAD_ARG,
                "conv2d_fwd: ADD_RESIDUAL and MASK_RELU share the residual slot");
  if (d->flags & (CODON_CONV_ADD_RESIDUAL | CODON_CONV_MASK_RELU)) {
    CODON_REQUIRE(residual, CODON_ERR_BAD_ARG, "conv2d_fwd: ADD_RESIDUAL without a residual pointer");
    CODON_REQUIRE(in_bounds(d->r_coff, d->cout, d->r_ctotal), CODON_ERR_BAD_ARG,
                  "conv2d_fwd: residual slice outside its buffer");
  }
  CODON_REQUIRE(!(d->flags & CODON_CONV_MASK_SUM) ||
                    ((d->flags & CODON_CONV_MASK_RELU) && (d->flags & CODON_CONV_ACCUM_OUT) && !(d->flags & (CODON_CONV_RELU | CODON_CONV_F16X3))),
                CODON_ERR_BAD_ARG, "conv2d_fwd: MASK_SUM needs MASK_RELU | ACCUM_OUT (and neither RELU nor F16X3)");
  CODON_REQUIRE(((uintptr_t)w_packed % 16) == 0, CODON_ERR_BAD_ARG, "conv2d_fwd: packed weights not 16-byte aligned");
  if (is16(d->dtype))
    return conv2d_fwd_16(d, x, w_packed, y, residual, (hipStream_t)stream);
  CODON_REQUIRE(d->dtype == CODON_F32, CODON_ERR_UNSUPPORTED, "conv2d_fwd: dtype %d", d->dtype);
  if (d->flags & CODON_CONV_F16X3) {
    CODON_REQUIRE(conv_f32x3_supported(d), CODON_ERR_UNSUPPORTED, "conv2d_fwd: no f16x3 kernel for k=%d cin=%d cout=%d",
                  d->ksize, d->cin, d->cout);
    return conv2d_fwd_f32x3(d, (const float*)x, w_packed, (float*)y, (const float*)residual, (hipStream_t)stream);
  }
  return conv2d_fwd_f32(d, (const float*)x, (const float*)w_packed, (float*)y, (const float*)residual,
                        (hipStream_t)stream);
}

int codon_conv2d_sum_into_fwd(const codon_conv_desc* d, const void* x, const void* w_packed, void* y, void* sum,
                              codon_stream_t stream) {
  CODON_REQUIRE(d && x && w_packed && y && sum, CODON_ERR_BAD_ARG, "conv2d_sum_into_fwd: null pointer");
  CODON_REQUIRE(shape_ok(d->batch, d->height, d->width), CODON_ERR_BAD_ARG, "conv2d_sum_into_fwd: bad shape %dx%dx%d",
                d->batch, d->height, d->width);
  CODON_REQUIRE(conv_slices_ok(d, true, true), CODON_ERR_BAD_ARG, "conv2d_sum_into_fwd: channel slice outside its buffer");
  CODON_REQUIRE(((uintptr_t)w_packed % 16) == 0, CODON_ERR_BAD_ARG, "conv2d_sum_into_fwd: packed weights not 16-byte aligned");
  CODON_REQUIRE(is16(d->dtype), CODON_ERR_UNSUPPORTED, "conv2d_sum_into_fwd: 16-bit dtypes only (dtype %d)", d->dtype);
  // `sum` may be another channel slice of the buffer that holds y (or x), never an overlapping one
  auto disjoint = [](int a0, int an, int b0, int bn) { return a0 + an <= b0 || b0 + bn <= a0; };
  CODON_REQUIRE((sum != y || (d->r_ctotal == d->y_ctotal && disjoint(d->r_coff, d->cout, d->y_coff, d->cout))) &&
                    (sum != x || (d->r_ctotal == d->x_ctotal && disjoint(d->r_coff, d->cout, d->x_coff, d->cin))),
                CODON_ERR_BAD_ARG, "conv2d_sum_into_fwd: sum overlaps x or y");
  return conv2d_sum_into_16(d, x, w_packed, y, sum, (hipStream_t)stream);
}

int codon_conv_chain1x1_fwd(const codon_conv_desc* d, const void* x, const void* w_packed, void* y, const void* w_chain,
                            const codon_tensor* out, const codon_tensor* residual, codon_stream_t stream) {
  CODON_REQUIRE(d && x && w_packed && w_chain && out && out->data, CODON_ERR_BAD_ARG, "conv_chain1x1_fwd: null pointer");
  CODON_REQUIRE(shape_ok(d->batch, d->height, d->width), CODON_ERR_BAD_ARG, "conv_chain1x1_fwd: bad shape %dx%dx%d",
                d->batch, d->height, d->width);
  CODON_REQUIRE(in_bounds(d->x_coff, d->cin, d->x_ctotal), CODON_ERR_BAD_ARG,
                "conv_chain1x1_fwd: input slice outside its buffer");
  CODON_REQUIRE(!y || in_bounds(d->y_coff, d->cout, d->y_ctotal), CODON_ERR_BAD_ARG,
                "conv_chain1x1_fwd: intermediate slice outside its buffer");
  CODON_REQUIRE(slice_ok(out), CODON_ERR_BAD_ARG, "conv_chain1x1_fwd: output slice outside its buffer");
  CODON_REQUIRE(!residual || slice_ok(residual), CODON_ERR_BAD_ARG, "conv_chain1x1_fwd: residual slice outside its buffer");
  CODON_REQUIRE((d->flags & ~(CODON_CONV_RELU | CODON_CONV_F16X3)) == 0, CODON_ERR_BAD_ARG,
                "conv_chain1x1_fwd: only RELU / F16X3 flags apply to the 5x5 stage");
  CODON_REQUIRE(((uintptr_t)w_packed % 16) == 0 && ((uintptr_t)w_chain % 16) == 0, CODON_ERR_BAD_ARG,
                "conv_chain1x1_fwd: packed weights not 16-byte aligned");
  if (is16(d->dtype)) {
    CODON_REQUIRE(!(d->flags & CODON_CONV_F16X3), CODON_ERR_BAD_ARG, "conv_chain1x1_fwd: F16X3 applies to fp32 tensors");
    return conv_chain1x1_fwd_16(d, x, w_packed, y, w_chain, out, residual, nullptr, nullptr, 0, (hipStream_t)stream);
  }
  CODON_REQUIRE(d->dtype == CODON_F32, CODON_ERR_UNSUPPORTED, "conv_chain1x1_fwd: dtype %d", d->dtype);
  if (d->flags & CODON_CONV_F16X3)
    return conv_chain1x1_fwd_f32x3(d, (const float*)x, w_packed, (float*)y, w_chain, out, residual, (hipStream_t)stream);
  return conv_chain1x1_fwd_f32(d, (const float*)x, (const float*)w_packed, (float*)y, (const float*)w_chain, out,
                               residual, nullptr, nullptr, 0, (hipStream_t)stream);
}

int codon_conv_chain1x1_stats_fwd(const codon_conv_desc* d, const void* x, const void* w_packed, void* y,
                                  const void* w_chain, const codon_tensor* out, const codon_tensor* residual,
                                  float* stats_pool, float* stats_partials, int32_t stats_choff, codon_stream_t stream) {
  CODON_REQUIRE(d && x && w_packed && w_chain && out && out->data && stats_pool && stats_partials, CODON_ERR_BAD_ARG,
                "conv_chain1x1_stats_fwd: null pointer");
  CODON_REQUIRE(shape_ok(d->batch, d->height, d->width), CODON_ERR_BAD_ARG, "conv_chain1x1_stats_fwd: bad shape %dx%dx%d",
                d->batch, d->height, d->width);
  CODON_REQUIRE(stats_choff == 0 || stats_choff == 64, CODON_ERR_BAD_ARG,
                "conv_chain1x1_stats_fwd: stats_choff %d (0 = colour stream, 64 = depth stream)", stats_choff);
  CODON_REQUIRE((d->flags & ~CODON_CONV_RELU) == 0, CODON_ERR_BAD_ARG, "conv_chain1x1_stats_fwd: only the RELU flag applies");
  CODON_REQUIRE(((uintptr_t)w_packed % 16) == 0 && ((uintptr_t)w_chain % 16) == 0 && ((uintptr_t)stats_partials % 8) == 0,
                CODON_ERR_BAD_ARG, "conv_chain1x1_stats_fwd: misaligned buffer");
  CODON_REQUIRE(conv_slices_ok(d, y != nullptr, false) && slice_ok(out), CODON_ERR_BAD_ARG,
                "conv_chain1x1_stats_fwd: slice outside its buffer");
  if (d->dtype == CODON_F32) {
    // fp32 (round 6): per-row-strip partials, codon_cac_fused_parts(height, width, CODON_F32) rows per image
    CODON_REQUIRE(!residual, CODON_ERR_BAD_ARG, "conv_chain1x1_stats_fwd: fp32 statistics come without a residual");
    return conv_chain1x1_fwd_f32(d, (const float*)x, (const float*)w_packed, (float*)y, (const float*)w_chain, out, nullptr,
                                 stats_pool, stats_partials, stats_choff, (hipStream_t)stream);
  }
  CODON_REQUIRE(is16(d->dtype), CODON_ERR_UNSUPPORTED, "conv_chain1x1_stats_fwd: dtype %d", d->dtype);
  return conv_chain1x1_fwd_16(d, x, w_packed, y, w_chain, out, residual, stats_pool, stats_partials, stats_choff,
                              (hipStream_t)stream);
}

int32_t codon_cac_fused_tiles(int32_t height, int32_t width) {
  return (height > 0 && width > 0) ? cac_fused_tiles(height, width) : 0;
}

int32_t codon_cac_fused_parts(int32_t height, int32_t width, int32_t dtype) {
  if (height <= 0 || width <= 0) return 0;
  if (dtype == CODON_F32) return height * ((width + 31) / 32);         // one row strip of 32 pixels each
  if (is16(dtype)) return cac_fused_tiles(height, width);
  return 0;
}

int codon_cac_fused_finish(int32_t batch, int32_t height, int32_t width, const float* partials, const float* pool_c,
                           const float* pool_d, float* folded, float* pooled, codon_stream_t stream) {
  CODON_REQUIRE(partials && pool_c && pool_d && folded && pooled, CODON_ERR_BAD_ARG, "cac_fused_finish: null pointer");
  CODON_REQUIRE(shape_ok(batch, height, width) && batch <= 65535, CODON_ERR_BAD_ARG, "cac_fused_finish: bad shape");
  return cac_fused_finish(batch, height, width, cac_fused_tiles(height, width), partials, pool_c, pool_d, folded, pooled,
                          (hipStream_t)stream);
}

int codon_cac_tail_fwd(int32_t batch, int32_t height, int32_t width, int32_t ntiles, const float* partials,
                       const float* pool_c, const float* pool_d, float* pooled, float* folded, int32_t* counters,
                       const float* w1, const float* b1, const float* w2, const float* b2, const float* w_spatial, float* ch,
                       float* pools_out, float* sp, codon_stream_t stream) {
  CODON_REQUIRE(partials && folded && counters && w1 && b1 && w2 && b2 && w_spatial && ch && sp, CODON_ERR_BAD_ARG,
                "cac_tail_fwd: null pointer");
  CODON_REQUIRE((pool_c != nullptr) == (pool_d != nullptr) && (pool_c || pooled), CODON_ERR_BAD_ARG,
                "cac_tail_fwd: pool_c and pool_d together, or pooled to read");
  CODON_REQUIRE(shape_ok(batch, height, width) && batch <= 65535, CODON_ERR_BAD_ARG, "cac_tail_fwd: bad shape");
  CODON_REQUIRE(pool_c ? (ntiles == cac_fused_tiles(height, width) || ntiles == codon_cac_fused_parts(height, width, CODON_F32))
                       : ntiles == cac_stats_tiles(height, width), CODON_ERR_BAD_ARG,
                "cac_tail_fwd: ntiles %d does not match the producer of the partials", ntiles);
  return cac_tail_fwd(batch, height, width, ntiles, partials, pool_c, pool_d, pool_c ? nullptr : pooled, pool_c ? pooled : nullptr,
                      folded, counters, w1, b1, w2, b2, w_spatial, ch, pools_out, sp, (hipStream_t)stream);
}

int codon_cac_gate_folded_fwd(int32_t batch, int32_t height, int32_t width, const float* folded, const float* w1,
                              const float* b1, const float* w2, const float* b2, float* ch, float* pools_out,
                              codon_stream_t stream) {
  CODON_REQUIRE(folded && w1 && b1 && w2 && b2 && ch, CODON_ERR_BAD_ARG, "cac_gate_folded_fwd: null pointer");
  CODON_REQUIRE(shape_ok(batch, height, width), CODON_ERR_BAD_ARG, "cac_gate_folded_fwd: bad shape");
  return cac_gate_fwd_n(batch, CODON_CAC_FOLDS, (float)(1.0 / ((double)height * width)), folded, w1, b1, w2, b2, ch,
                        pools_out, (hipStream_t)stream);
}

static int gated_fwd(const codon_conv_desc* d, const void* pre, const codon_tensor* inputs, const float* ch,
                     const float* sp, const void* w_packed, void* y, const codon_tensor* gated_out, codon_stream_t stream) {
  CODON_REQUIRE(d && pre && inputs && inputs->data && ch && sp && w_packed && y, CODON_ERR_BAD_ARG,
                "conv2d_gated_fwd: null pointer");
  CODON_REQUIRE(shape_ok(d->batch, d->height, d->width), CODON_ERR_BAD_ARG, "conv2d_gated_fwd: bad shape %dx%dx%d",
                d->batch, d->height, d->width);
  CODON_REQUIRE(in_bounds(d->x_coff, d->cin, d->x_ctotal) && d->x_coff % 64 == 0, CODON_ERR_BAD_ARG,
                "conv2d_gated_fwd: input slice [%d,%d) of %d channels (must start at a multiple of 64)", d->x_coff,
                d->x_coff + d->cin, d->x_ctotal);
  CODON_REQUIRE(slice_ok(inputs, d->cin), CODON_ERR_BAD_ARG, "conv2d_gated_fwd: `inputs` slice outside its buffer");
  CODON_REQUIRE(in_bounds(d->y_coff, d->cout, d->y_ctotal), CODON_ERR_BAD_ARG,
                "conv2d_gated_fwd: output slice outside its buffer");
  CODON_REQUIRE((d->flags & ~CODON_CONV_RELU) == 0, CODON_ERR_BAD_ARG, "conv2d_gated_fwd: only the RELU flag applies");
  CODON_REQUIRE(((uintptr_t)w_packed % 16) == 0, CODON_ERR_BAD_ARG, "conv2d_gated_fwd: packed weights not 16-byte aligned");
  if (is16(d->dtype))
    return conv2d_gated_fwd_16(d, pre, inputs, ch, sp, w_packed, y, gated_out, (hipStream_t)stream);
  CODON_REQUIRE(d->dtype == CODON_F32, CODON_ERR_UNSUPPORTED, "conv2d_gated_fwd: dtype %d", d->dtype);
  CODON_REQUIRE(!gated_out || slice_ok(gated_out, d->cin), CODON_ERR_BAD_ARG,
                "conv2d_gated_emit_fwd: gated_out slice outside its buffer");
  return conv2d_gated_fwd_f32(d, (const float*)pre, inputs, ch, sp, (const float*)w_packed, (float*)y, gated_out, (hipStream_t)stream);
}

int codon_conv2d_gated_fwd(const codon_conv_desc* d, const void* pre, const codon_tensor* inputs, const float* ch,
                           const float* sp, const void* w_packed, void* y, codon_stream_t stream) {
  return gated_fwd(d, pre, inputs, ch, sp, w_packed, y, nullptr, stream);
}

int codon_conv2d_gated_emit_fwd(const codon_conv_desc* d, const void* pre, const codon_tensor* inputs, const float* ch,
                                const float* sp, const void* w_packed, void* y, const codon_tensor* gated_out,
                                codon_stream_t stream) {
  CODON_REQUIRE(gated_out && gated_out->data, CODON_ERR_BAD_ARG, "conv2d_gated_emit_fwd: null gated_out");
  return gated_fwd(d, pre, inputs, ch, sp, w_packed, y, gated_out, stream);
}

size_t codon_conv_wgrad_workspace_bytes(const codon_conv_desc* d) {
  if (!d || !shape_ok(d->batch, d->height, d->width)) return 0;
  if (is16(d->dtype)) return conv_wgrad_16_workspace_bytes(d);
  return conv_wgrad_workspace_bytes(d);
}

int codon_conv2d_wgrad(const codon_conv_desc* d, const void* x, const void* gy, float* dw, void* workspace,
                       size_t workspace_bytes, int32_t accumulate, codon_stream_t stream) {
  CODON_REQUIRE(d && x && gy && (dw || accumulate == CODON_WGRAD_DEFER) && workspace, CODON_ERR_BAD_ARG, "conv2d_wgrad: null pointer");
  CODON_REQUIRE(accumulate >= 0 && accumulate <= CODON_WGRAD_DEFER, CODON_ERR_BAD_ARG, "conv2d_wgrad: accumulate %d", accumulate);
  CODON_REQUIRE(shape_ok(d->batch, d->height, d->width), CODON_ERR_BAD_ARG, "conv2d_wgrad: bad shape");
  CODON_REQUIRE(conv_slices_ok(d, true, false), CODON_ERR_BAD_ARG, "conv2d_wgrad: channel slice outside its buffer");
  if (is16(d->dtype))
    return conv2d_wgrad_16(d, x, gy, dw, (float*)workspace, workspace_bytes, accumulate, (hipStream_t)stream);
  CODON_REQUIRE(d->dtype == CODON_F32, CODON_ERR_UNSUPPORTED, "conv2d_wgrad: dtype %d", d->dtype);
  return conv2d_wgrad_f32(d, (const float*)x, (const float*)gy, dw, (float*)workspace, workspace_bytes, accumulate,
                          (hipStream_t)stream);
}

int codon_conv1x1_bwd(const codon_conv_desc* d, const void* x, const void* gy, const void* w_packed_dgrad,
                      const codon_tensor* gx, float* dw, void* workspace, size_t workspace_bytes, int32_t accumulate,
                      codon_stream_t stream) {
  CODON_REQUIRE(d && x && gy && w_packed_dgrad && gx && gx->data && (dw || accumulate == CODON_WGRAD_DEFER) && workspace,
                CODON_ERR_BAD_ARG, "conv1x1_bwd: null pointer");
  CODON_REQUIRE(accumulate >= 0 && accumulate <= CODON_WGRAD_DEFER, CODON_ERR_BAD_ARG, "conv1x1_bwd: accumulate %d", accumulate);
  CODON_REQUIRE(shape_ok(d->batch, d->height, d->width), CODON_ERR_BAD_ARG, "conv1x1_bwd: bad shape");
  CODON_REQUIRE(conv_slices_ok(d, true, false) && slice_ok(gx, d->cin), CODON_ERR_BAD_ARG,
                "conv1x1_bwd: channel slice outside its buffer");
  CODON_REQUIRE(((uintptr_t)w_packed_dgrad % 16) == 0, CODON_ERR_BAD_ARG, "conv1x1_bwd: packed weights not 16-byte aligned");
  CODON_REQUIRE(is16(d->dtype), CODON_ERR_UNSUPPORTED,
                "conv1x1_bwd: 16-bit dtypes only (dtype %d): call codon_conv2d_wgrad + codon_conv2d_fwd", d->dtype);
  return conv1x1_bwd_16(d, x, gy, w_packed_dgrad, gx, dw, (float*)workspace, workspace_bytes, accumulate, (hipStream_t)stream,
                        nullptr);
}

int codon_conv1x1_bwd_gated(const codon_conv_desc* d, const void* x, const void* g_out, const void* w_packed_dgrad,
                            const codon_tensor* gx, float* dw, void* workspace, size_t workspace_bytes, int32_t accumulate,
                            const float* ch, const float* sp, const float* g_pooled, const float* g_pools,
                            const int32_t* argpix, const int32_t* argch, int32_t fcat_base, codon_stream_t stream) {
  CODON_REQUIRE(d && x && g_out && w_packed_dgrad && gx && gx->data && (dw || accumulate == CODON_WGRAD_DEFER) && workspace &&
                    ch && sp && g_pooled && g_pools && argpix && argch,
                CODON_ERR_BAD_ARG, "conv1x1_bwd_gated: null pointer");
  CODON_REQUIRE(accumulate >= 0 && accumulate <= CODON_WGRAD_DEFER, CODON_ERR_BAD_ARG, "conv1x1_bwd_gated: accumulate %d", accumulate);
  CODON_REQUIRE(shape_ok(d->batch, d->height, d->width), CODON_ERR_BAD_ARG, "conv1x1_bwd_gated: bad shape");
  CODON_REQUIRE(conv_slices_ok(d, true, false) && slice_ok(gx, d->cin), CODON_ERR_BAD_ARG,
                "conv1x1_bwd_gated: channel slice outside its buffer");
  CODON_REQUIRE(fcat_base == 0 || fcat_base == 64, CODON_ERR_BAD_ARG, "conv1x1_bwd_gated: fcat_base %d (0 colour, 64 depth)", fcat_base);
  CODON_REQUIRE(((uintptr_t)w_packed_dgrad % 16) == 0, CODON_ERR_BAD_ARG, "conv1x1_bwd_gated: packed weights not 16-byte aligned");
  CODON_REQUIRE(is16(d->dtype), CODON_ERR_UNSUPPORTED, "conv1x1_bwd_gated: 16-bit dtypes only (dtype %d)", d->dtype);
  const Conv1x1GateBwd gb{ch, sp, g_pooled, g_pools, argpix, argch, fcat_base};
  return conv1x1_bwd_16(d, x, g_out, w_packed_dgrad, gx, dw, (float*)workspace, workspace_bytes, accumulate, (hipStream_t)stream,
                        &gb);
}

int codon_stem_fwd(int32_t batch, int32_t height, int32_t width, const float* x, const float* w_oihw, void* y,
                   int32_t y_ctotal, int32_t y_coff, int32_t dtype, codon_stream_t stream) {
  return codon_stem_fwd_guarded(batch, height, width, x, w_oihw, y, y_ctotal, y_coff, dtype, nullptr, nullptr, stream);
}

int codon_stem_fwd_guarded(int32_t batch, int32_t height, int32_t width, const float* x, const float* w_oihw, void* y,
                           int32_t y_ctotal, int32_t y_coff, int32_t dtype, int32_t* bad, int32_t* host_word,
                           codon_stream_t stream) {
  CODON_REQUIRE(x && w_oihw && y, CODON_ERR_BAD_ARG, "stem_fwd: null pointer");
  CODON_REQUIRE(shape_ok(batch, height, width), CODON_ERR_BAD_ARG, "stem_fwd: bad shape");
  CODON_REQUIRE(in_bounds(y_coff, 64, y_ctotal), CODON_ERR_BAD_ARG, "stem_fwd: output slice outside buffer");
  CODON_REQUIRE(dtype_known(dtype), CODON_ERR_UNSUPPORTED, "stem_fwd: dtype %d", dtype);
  return stem_fwd(batch, height, width, x, w_oihw, y, y_ctotal, y_coff, 1, nullptr, 0, 0, dtype, bad, host_word,
                  (hipStream_t)stream);
}

int codon_stem_pair_fwd(int32_t batch, int32_t height, int32_t width, const float* xa, const float* wa_oihw, void* ya,
                        int32_t ya_ctotal, int32_t ya_coff, const float* xb, const float* wb_oihw, void* yb,
                        int32_t yb_ctotal, int32_t yb_coff, int32_t dtype, codon_stream_t stream) {
  return codon_stem_pair_fwd_guarded(batch, height, width, xa, wa_oihw, ya, ya_ctotal, ya_coff, xb, wb_oihw, yb, yb_ctotal,
                                     yb_coff, dtype, nullptr, nullptr, nullptr, stream);
}

int codon_stem_pair_fwd_guarded(int32_t batch, int32_t height, int32_t width, const float* xa, const float* wa_oihw, void* ya,
                                int32_t ya_ctotal, int32_t ya_coff, const float* xb, const float* wb_oihw, void* yb,
                                int32_t yb_ctotal, int32_t yb_coff, int32_t dtype, int32_t* bad, int32_t* host_word_a,
                                int32_t* host_word_b, codon_stream_t stream) {
  CODON_REQUIRE(xa && wa_oihw && ya && xb && wb_oihw && yb, CODON_ERR_BAD_ARG, "stem_pair_fwd: null pointer");
  CODON_REQUIRE(shape_ok(batch, height, width), CODON_ERR_BAD_ARG, "stem_pair_fwd: bad shape");
  CODON_REQUIRE(in_bounds(ya_coff, 64, ya_ctotal) && in_bounds(yb_coff, 64, yb_ctotal), CODON_ERR_BAD_ARG,
                "stem_pair_fwd: output slice outside buffer");
  CODON_REQUIRE(ya != yb || ya_coff + 64 <= yb_coff || yb_coff + 64 <= ya_coff, CODON_ERR_BAD_ARG,
                "stem_pair_fwd: the two output slices overlap");
  CODON_REQUIRE(dtype_known(dtype), CODON_ERR_UNSUPPORTED, "stem_pair_fwd: dtype %d", dtype);
  return stem_pair_fwd(batch, height, width, xa, wa_oihw, ya, ya_ctotal, ya_coff, xb, wb_oihw, yb, yb_ctotal, yb_coff, dtype,
                       bad, host_word_a, host_word_b, (hipStream_t)stream);
}

int codon_head_fwd(int32_t batch, int32_t height, int32_t width, const void* x, int32_t x_ctotal, int32_t x_coff,
                   const float* w_oihw, const float* residual, float* y, int32_t dtype, codon_stream_t stream) {
  return codon_head_fwd_guarded(batch, height, width, x, x_ctotal, x_coff, w_oihw, residual, y, dtype, nullptr, stream);
}

int codon_head_fwd_guarded(int32_t batch, int32_t height, int32_t width, const void* x, int32_t x_ctotal, int32_t x_coff,
                           const float* w_oihw, const float* residual, float* y, int32_t dtype, const int32_t* bad,
                           codon_stream_t stream) {
  CODON_REQUIRE(x && w_oihw && residual && y, CODON_ERR_BAD_ARG, "head_fwd: null pointer");
  CODON_REQUIRE(shape_ok(batch, height, width), CODON_ERR_BAD_ARG, "head_fwd: bad shape");
  CODON_REQUIRE(in_bounds(x_coff, 64, x_ctotal), CODON_ERR_BAD_ARG, "head_fwd: input slice outside buffer");
  CODON_REQUIRE(dtype_known(dtype), CODON_ERR_UNSUPPORTED, "head_fwd: dtype %d", dtype);
  return head_fwd(batch, height, width, x, x_ctotal, x_coff, w_oihw, residual, y, false, dtype, bad, (hipStream_t)stream);
}

int codon_head_fwd_y16(int32_t batch, int32_t height, int32_t width, const void* x, int32_t x_ctotal, int32_t x_coff,
                       const float* w_oihw, const float* residual, void* y16, int32_t dtype, codon_stream_t stream) {
  return codon_head_fwd_y16_guarded(batch, height, width, x, x_ctotal, x_coff, w_oihw, residual, y16, dtype, nullptr, stream);
}

int codon_head_fwd_y16_guarded(int32_t batch, int32_t height, int32_t width, const void* x, int32_t x_ctotal, int32_t x_coff,
                               const float* w_oihw, const float* residual, void* y16, int32_t dtype, const int32_t* bad,
                               codon_stream_t stream) {
  CODON_REQUIRE(x && w_oihw && residual && y16, CODON_ERR_BAD_ARG, "head_fwd_y16: null pointer");
  CODON_REQUIRE(shape_ok(batch, height, width), CODON_ERR_BAD_ARG, "head_fwd_y16: bad shape");
  CODON_REQUIRE(in_bounds(x_coff, 64, x_ctotal), CODON_ERR_BAD_ARG, "head_fwd_y16: input slice outside buffer");
  CODON_REQUIRE(is16(dtype), CODON_ERR_UNSUPPORTED,
                "head_fwd_y16: dtype %d (the 16-bit output exists for 16-bit activations)", dtype);
  CODON_REQUIRE(((uintptr_t)y16 % 2) == 0, CODON_ERR_BAD_ARG, "head_fwd_y16: output not 2-byte aligned");
  return head_fwd(batch, height, width, x, x_ctotal, x_coff, w_oihw, residual, y16, true, dtype, bad, (hipStream_t)stream);
}

int32_t codon_cac_stats_tiles(int32_t height, int32_t width) {
  if (height <= 0 || width <= 0) return 0;
  return cac_stats_tiles(height, width);
}

int codon_cac_stats_fwd(int32_t batch, int32_t height, int32_t width, const codon_tensor* pre_c,
                        const codon_tensor* pre, float* pooled, float* partials, int32_t dtype,
                        codon_stream_t stream) {
  CODON_REQUIRE(slice_ok(pre_c) && slice_ok(pre) && pooled && partials, CODON_ERR_BAD_ARG,
                "cac_stats_fwd: null pointer or bad channel slice");
  CODON_REQUIRE(shape_ok(batch, height, width), CODON_ERR_BAD_ARG, "cac_stats_fwd: bad shape");
  CODON_REQUIRE(((uintptr_t)partials % 8) == 0, CODON_ERR_BAD_ARG, "cac_stats_fwd: partials not 8-byte aligned");
  CODON_REQUIRE(dtype_known(dtype), CODON_ERR_UNSUPPORTED, "cac_stats_fwd: dtype %d", dtype);
  return cac_stats_fwd(batch, height, width, pre_c, pre, pooled, partials, dtype, (hipStream_t)stream, nullptr);
}

int codon_cac_stats_scaled_fwd(int32_t batch, int32_t height, int32_t width, const codon_tensor* pre_c,
                               const codon_tensor* pre, const float* ch, float* pooled, float* partials, int32_t dtype,
                               codon_stream_t stream) {
  CODON_REQUIRE(slice_ok(pre_c) && slice_ok(pre) && ch && pooled && partials, CODON_ERR_BAD_ARG,
                "cac_stats_scaled_fwd: null pointer or bad channel slice");
  CODON_REQUIRE(shape_ok(batch, height, width), CODON_ERR_BAD_ARG, "cac_stats_scaled_fwd: bad shape");
  CODON_REQUIRE(((uintptr_t)partials % 8) == 0, CODON_ERR_BAD_ARG, "cac_stats_scaled_fwd: partials not 8-byte aligned");
  CODON_REQUIRE(dtype_known(dtype), CODON_ERR_UNSUPPORTED, "cac_stats_scaled_fwd: dtype %d", dtype);
  return cac_stats_fwd(batch, height, width, pre_c, pre, pooled, partials, dtype, (hipStream_t)stream, ch);
}

int codon_ew_sq_scale(int32_t batch, int32_t height, int32_t width, const codon_tensor* x, const float* ch,
                      const codon_tensor* y, int32_t dtype, codon_stream_t stream) {
  CODON_REQUIRE(slice_ok(x) && slice_ok(y) && ch, CODON_ERR_BAD_ARG, "ew_sq_scale: null pointer or bad channel slice");
  CODON_REQUIRE(shape_ok(batch, height, width), CODON_ERR_BAD_ARG, "ew_sq_scale: bad shape");
  CODON_REQUIRE(dtype_known(dtype), CODON_ERR_UNSUPPORTED, "ew_sq_scale: dtype %d", dtype);
  return ew_sq_scale(batch, height, width, x, ch, y, dtype, (hipStream_t)stream);
}

int codon_cac_gate_fwd(int32_t batch, int32_t height, int32_t width, const float* partials, const float* w1,
                       const float* b1, const float* w2, const float* b2, float* ch, float* pools_out,
                       codon_stream_t stream) {
  CODON_REQUIRE(partials && w1 && b1 && w2 && b2 && ch, CODON_ERR_BAD_ARG, "cac_gate_fwd: null pointer");
  CODON_REQUIRE(shape_ok(batch, height, width), CODON_ERR_BAD_ARG, "cac_gate_fwd: bad shape");
  return cac_gate_fwd(batch, height, width, partials, w1, b1, w2, b2, ch, pools_out, (hipStream_t)stream);
}

int codon_cac_spatial_fwd(int32_t batch, int32_t height, int32_t width, const float* pooled, const float* w_spatial,
                          float* sp, codon_stream_t stream) {
  CODON_REQUIRE(pooled && w_spatial && sp, CODON_ERR_BAD_ARG, "cac_spatial_fwd: null pointer");
  CODON_REQUIRE(shape_ok(batch, height, width), CODON_ERR_BAD_ARG, "cac_spatial_fwd: bad shape");
  return cac_spatial_fwd(batch, height, width, pooled, w_spatial, sp, (hipStream_t)stream);
}

int codon_cac_apply_fwd(int32_t batch, int32_t height, int32_t width, const codon_tensor* pre,
                        const codon_tensor* pre_c, const float* ch, const float* sp, const codon_tensor* inputs,
                        const codon_tensor* inputs_c, const codon_tensor* out, const codon_tensor* out_c,
                        int32_t dtype, codon_stream_t stream) {
  CODON_REQUIRE(slice_ok(pre) && slice_ok(pre_c) && ch && sp && slice_ok(inputs) && slice_ok(inputs_c) &&
                    slice_ok(out) && slice_ok(out_c),
                CODON_ERR_BAD_ARG, "cac_apply_fwd: null pointer or bad channel slice");
  CODON_REQUIRE(shape_ok(batch, height, width), CODON_ERR_BAD_ARG, "cac_apply_fwd: bad shape");
  CODON_REQUIRE(dtype_known(dtype), CODON_ERR_UNSUPPORTED, "cac_apply_fwd: dtype %d", dtype);
  return cac_apply_fwd(batch, height, width, pre, pre_c, ch, sp, inputs, inputs_c, out, out_c, dtype,
                       (hipStream_t)stream);
}

int codon_stencil_1to64(int32_t batch, int32_t height, int32_t width, const float* x, const float* w_64x9,
                        const codon_tensor* y, int32_t flags, const codon_tensor* mask, int32_t dtype,
                        codon_stream_t stream) {
  CODON_REQUIRE(x && w_64x9 && slice_ok(y) && (!mask || slice_ok(mask)), CODON_ERR_BAD_ARG,
                "stencil_1to64: null pointer or bad channel slice");
  CODON_REQUIRE(shape_ok(batch, height, width), CODON_ERR_BAD_ARG, "stencil_1to64: bad shape");
  CODON_REQUIRE(dtype_known(dtype), CODON_ERR_UNSUPPORTED, "stencil_1to64: dtype %d", dtype);
  return stem_fwd(batch, height, width, x, w_64x9, y->data, y->ctotal, y->coff, flags, mask ? mask->data : nullptr,
                  mask ? mask->ctotal : 0, mask ? mask->coff : 0, dtype, nullptr, nullptr, (hipStream_t)stream);
}

size_t codon_conv1ch_wgrad_workspace_bytes(int32_t batch, int32_t height, int32_t width) {
  if (!shape_ok(batch, height, width)) return 0;
  return conv1ch_wgrad_workspace_bytes(batch, height, width);
}

int codon_conv1ch_wgrad(int32_t batch, int32_t height, int32_t width, const codon_tensor* a, const float* s,
                        float* dw, int32_t flip, void* workspace, size_t workspace_bytes, int32_t dtype,
                        codon_stream_t stream) {
  CODON_REQUIRE(dtype_known(dtype), CODON_ERR_UNSUPPORTED, "conv1ch_wgrad: dtype %d", dtype);
  CODON_REQUIRE(slice_ok(a) && s && (dw || (flip & CODON_W1_DEFER)) && workspace, CODON_ERR_BAD_ARG,
                "conv1ch_wgrad: null pointer or bad slice");
  CODON_REQUIRE((flip & ~(CODON_W1_FLIP | CODON_W1_ACCUMULATE | CODON_W1_DEFER)) == 0, CODON_ERR_BAD_ARG, "conv1ch_wgrad: flip 0x%x", (unsigned)flip);
  CODON_REQUIRE(shape_ok(batch, height, width), CODON_ERR_BAD_ARG, "conv1ch_wgrad: bad shape");
  return conv1ch_wgrad(batch, height, width, a->data, a->ctotal, a->coff, s, dw, flip, (float*)workspace,
                       workspace_bytes, dtype, (hipStream_t)stream);
}

int codon_conv_pair_begin(void) {
  CODON_REQUIRE(!g_pair.active, CODON_ERR_BAD_ARG, "conv_pair_begin: already inside a pair on this thread");
  g_pair.active = true;
  g_pair.n = 0;
  return CODON_OK;
}

int codon_conv_pair_end(codon_stream_t stream) {
  CODON_REQUIRE(g_pair.active, CODON_ERR_BAD_ARG, "conv_pair_end without conv_pair_begin on this thread");
  g_pair.active = false;
  const int n = g_pair.n;
  g_pair.n = 0;
  const PairCall& a = g_pair.call[0];
  const PairCall& b = g_pair.call[1];
  // one grid only for two calls that were given pair_end's own stream: a caller that issued them on different streams
  // ordered its other work against THOSE streams
  if (n == 2 && a.pair == b.pair && a.nblk == b.nblk && a.tiles_x == b.tiles_x && a.tiles_y == b.tiles_y &&
      a.stream == (hipStream_t)stream && b.stream == (hipStream_t)stream && (long)a.nblk * 2 < (1L << 31)) {
    const int st = a.pair(a.blob, b.blob, (hipStream_t)stream);
    return st == CODON_OK ? 1 : st;
  }
  // a conv5x5 64->64 and the conv3x3 64->64 of the same family (mix53): one grid of both kinds of workgroup
  if (n == 2 && a.stream == (hipStream_t)stream && b.stream == (hipStream_t)stream && a.mix_kind && b.mix_kind &&
      (long)a.nblk + b.nblk < (1L << 31)) {
    const PairCall* five = (a.mix_kind & 1) ? &a : &b;
    const PairCall* three = (a.mix_kind & 1) ? &b : &a;
    if ((five->mix_kind & 1) && three->mix_kind == five->mix_kind + 1 && five->mix) {
      const int st = five->mix(five->blob, three->blob, (hipStream_t)stream);
      return st == CODON_OK ? 1 : st;
    }
  }
  for (int k = 0; k < n; ++k) {          // one by one, each on the stream its call named
    const int st = g_pair.call[k].single(g_pair.call[k].blob, g_pair.call[k].stream);
    if (st != CODON_OK) return st;
  }
  return n;
}

int codon_conv_tiling_f32(const codon_conv_desc* d, int chained, int in_pair) {
  CODON_REQUIRE(d && shape_ok(d->batch, d->height, d->width), CODON_ERR_BAD_ARG, "conv_tiling_f32: null descriptor or bad shape");
  return conv_tiling_f32(d, chained, in_pair);
}

int codon_conv_form_c8(const codon_conv_desc* d) {
  CODON_REQUIRE(d && shape_ok(d->batch, d->height, d->width), CODON_ERR_BAD_ARG, "conv_form_c8: null descriptor or bad shape");
  CODON_REQUIRE(is16(d->dtype), CODON_ERR_UNSUPPORTED, "conv_form_c8: dtype %d is not a 16-bit dtype", d->dtype);
  return conv_form_c8(d);
}

// codon_launch_form (include/codon_hip.h): the rules of launch_rules.h / px8.h as the launchers ask them, without a launch
int codon_launch_form(int32_t op, int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t aligned, codon_form* out) {
  CODON_REQUIRE(out && op >= CODON_FORM_STEM && op <= CODON_FORM_CONV1CH_WGRAD && dtype_known(dtype) && shape_ok(B, H, W),
                CODON_ERR_BAD_ARG, "launch_form: null out, unknown op %d or dtype %d, or bad shape", op, dtype);
  const long HW = (long)H * W;
  codon_form f{};
  switch (op) {
    case CODON_FORM_STEM:
      f.vec = is16(dtype) ? STEM_C8_VEC : stem_vec_f32(B * HW, W, aligned != 0);
      f.cols = is16(dtype) ? 64 * STEM_C8_VEC : 0;
      break;
    case CODON_FORM_HEAD:
      if (is16(dtype)) {
        f.rows = head_rows_c8(B * HW); f.cols = HEAD_C8_COLS;
      } else {
        head_form_f32(B * HW, W, aligned != 0, [&](auto s) {
          f.vec = s.vec; f.rows = s.rows; f.depth = s.depth; f.cols = 64 * s.vec;
          return 0;
        });
      }
      break;
    case CODON_FORM_CAC_STATS:
      f.tile = stats_tile(HW); f.tiles = cac_stats_tiles(H, W);
      f.vector = !is16(dtype) && !stats_small(HW) && px_vector(HW, aligned != 0);
      break;
    case CODON_FORM_CAC_BWD_GATE:
      f.tile = PX_TILE; f.tiles = cac_bwd_tiles(H, W); f.slices = GATE_SLICES; f.per = gate_slice_tiles(f.tiles);
      break;
    case CODON_FORM_CAC_SPATIAL_FWD: f.tile = SPF_T; break;
    case CODON_FORM_CAC_SPATIAL_BWD: f.tile = SPB_T; break;
    default: f.rows = W1_ROWS; f.cols = W1_CHUNK; break;      // CODON_FORM_CONV1CH_WGRAD
  }
  *out = f;
  return CODON_OK;
}

int codon_cast_multi(const codon_cast_desc* desc, float* dst, codon_stream_t stream) {
  CODON_REQUIRE(desc && dst, CODON_ERR_BAD_ARG, "cast_multi: null pointer");
  return cast_multi(desc, dst, (hipStream_t)stream);
}

int codon_adam_step(const codon_adam_desc* desc, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                    float beta2, float eps, float weight_decay, int32_t step, codon_stream_t stream) {
  CODON_REQUIRE(desc && grad && exp_avg && exp_avg_sq, CODON_ERR_BAD_ARG, "adam_step: null pointer");
  return adam_step(desc, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream);
}

size_t codon_grad_norm_workspace_bytes(void) { return grad_norm_workspace_bytes(); }

int codon_grad_norm(const float* grad, int64_t n, void* state, codon_stream_t stream) {
  CODON_REQUIRE(grad && state, CODON_ERR_BAD_ARG, "grad_norm: null pointer");
  return grad_norm(grad, (long)n, state, (hipStream_t)stream);
}

int codon_adam_step_guarded(const codon_adam_desc* desc, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema,
                            void* state, float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                            double max_norm, int32_t skip_nonfinite, double ema_decay, codon_stream_t stream) {
  CODON_REQUIRE(desc && grad && exp_avg && exp_avg_sq && state, CODON_ERR_BAD_ARG, "adam_step_guarded: null pointer");
  return adam_step_guarded(desc, grad, exp_avg, exp_avg_sq, ema, state, lr, beta1, beta2, eps, weight_decay, step, max_norm,
                           skip_nonfinite, ema_decay, (hipStream_t)stream);
}

int codon_reduce_multi(const codon_reduce_item* items, int32_t n_items, codon_stream_t stream) {
  CODON_REQUIRE(items && n_items >= 1, CODON_ERR_BAD_ARG, "reduce_multi: no items");
  return reduce_multi(items, n_items, (hipStream_t)stream);
}

int codon_ew_add_mask(int32_t batch, int32_t height, int32_t width, int32_t channels, const codon_tensor* dst,
                      const codon_tensor* src, const codon_tensor* mask, int32_t accumulate, int32_t dtype,
                      codon_stream_t stream) {
  CODON_REQUIRE(dtype_known(dtype), CODON_ERR_UNSUPPORTED, "ew_add_mask: dtype %d", dtype);
  auto ok = [&](const codon_tensor* t) { return slice_ok(t, channels); };
  CODON_REQUIRE(channels > 0 && ok(dst) && (!src || ok(src)) && (!mask || ok(mask)), CODON_ERR_BAD_ARG,
                "ew_add_mask: null pointer or bad channel slice");
  CODON_REQUIRE(shape_ok(batch, height, width), CODON_ERR_BAD_ARG, "ew_add_mask: bad shape");
  return ew_add_mask(batch, height, width, channels, dst, src, mask, accumulate, dtype, (hipStream_t)stream);
}

int codon_ew_sum_mask(int32_t batch, int32_t height, int32_t width, int32_t channels, const codon_tensor* dst, int32_t nsrc,
                      const codon_tensor* src0, const codon_tensor* src1, const codon_tensor* src2, const codon_tensor* src3,
                      const codon_tensor* mask, int32_t dtype, codon_stream_t stream) {
  CODON_REQUIRE(dtype_known(dtype), CODON_ERR_UNSUPPORTED, "ew_sum_mask: dtype %d", dtype);
  auto ok = [&](const codon_tensor* t) { return slice_ok(t, channels); };
  const codon_tensor* srcs[4] = {src0, src1, src2, src3};
  CODON_REQUIRE(nsrc >= 1 && nsrc <= 4, CODON_ERR_BAD_ARG, "ew_sum_mask: %d sources (1..4)", nsrc);
  for (int i = 0; i < nsrc; ++i)
    CODON_REQUIRE(ok(srcs[i]) && srcs[i]->data != dst->data, CODON_ERR_BAD_ARG, "ew_sum_mask: source %d null, out of range or aliasing dst", i);
  CODON_REQUIRE(channels > 0 && ok(dst) && (!mask || ok(mask)), CODON_ERR_BAD_ARG, "ew_sum_mask: null pointer or bad channel slice");
  CODON_REQUIRE(shape_ok(batch, height, width), CODON_ERR_BAD_ARG, "ew_sum_mask: bad shape");
  return ew_sum_mask(batch, height, width, channels, dst, nsrc, srcs, mask, dtype, (hipStream_t)stream);
}

int32_t codon_cac_bwd_tiles(int32_t height, int32_t width) {
  return (height > 0 && width > 0) ? cac_bwd_tiles(height, width) : 0;
}
int32_t codon_cac_bwd_spatial_blocks(int32_t batch, int32_t height, int32_t width) {
  return shape_ok(batch, height, width) ? cac_bwd_spatial_blocks(batch, height, width) : 0;
}

int codon_cac_bwd_reduce(int32_t batch, int32_t height, int32_t width, const codon_tensor* g_out,
                         const codon_tensor* g_out_c, const codon_tensor* pre, const codon_tensor* pre_c,
                         const float* ch, const float* sp, const float* pools, float* g_z, float* part_gch,
                         int32_t* part_arg, int32_t dtype, codon_stream_t stream) {
  CODON_REQUIRE(dtype_known(dtype), CODON_ERR_UNSUPPORTED, "cac_bwd_reduce: dtype %d", dtype);
  CODON_REQUIRE(slice_ok(g_out) && slice_ok(g_out_c) && slice_ok(pre) && slice_ok(pre_c) && ch && sp && pools &&
                    g_z && part_gch && part_arg,
                CODON_ERR_BAD_ARG, "cac_bwd_reduce: null pointer or bad channel slice");
  CODON_REQUIRE(shape_ok(batch, height, width) && batch <= 65535, CODON_ERR_BAD_ARG, "cac_bwd_reduce: bad shape");
  return cac_bwd_reduce(batch, height, width, g_out, g_out_c, pre, pre_c, ch, sp, pools, g_z, part_gch, part_arg,
                        dtype, (hipStream_t)stream);
}

int codon_cac_bwd_reduce_acc(int32_t batch, int32_t height, int32_t width, const codon_tensor* g_out,
                             const codon_tensor* g_out_c, const codon_tensor* pre, const codon_tensor* pre_c,
                             const float* ch, const float* sp, const float* pools, const float* pooled, float* g_z,
                             float* part_gch, int32_t* part_arg, int32_t* argch, const codon_tensor* g_in,
                             const codon_tensor* g_in_c, int32_t accumulate_in, int32_t dtype, codon_stream_t stream) {
  CODON_REQUIRE(is16(dtype), CODON_ERR_UNSUPPORTED,
                "cac_bwd_reduce_acc: 16-bit dtypes only (dtype %d): fp32 takes codon_cac_bwd_reduce + codon_cac_bwd_apply", dtype);
  CODON_REQUIRE(slice_ok(g_out) && slice_ok(g_out_c) && slice_ok(pre) && slice_ok(pre_c) && slice_ok(g_in) && slice_ok(g_in_c) &&
                    ch && sp && pools && pooled && g_z && part_gch && part_arg && argch,
                CODON_ERR_BAD_ARG, "cac_bwd_reduce_acc: null pointer or bad channel slice");
  CODON_REQUIRE(shape_ok(batch, height, width) && batch <= 65535, CODON_ERR_BAD_ARG, "cac_bwd_reduce_acc: bad shape");
  return cac_bwd_reduce_acc(batch, height, width, g_out, g_out_c, pre, pre_c, ch, sp, pools, pooled, g_z, part_gch, part_arg,
                            argch, g_in, g_in_c, accumulate_in, dtype, (hipStream_t)stream);
}

int codon_cac_bwd_gate(int32_t batch, int32_t height, int32_t width, const float* part_gch, const int32_t* part_arg,
                       const float* ch, const float* pools, const float* w1, const float* b1, const float* w2,
                       float* g_pools, int32_t* argpix, float* part_param, float* dw1, float* db1, float* dw2,
                       float* db2, codon_stream_t stream) {
  CODON_REQUIRE(part_gch && part_arg && ch && pools && w1 && b1 && w2 && g_pools && argpix && part_param &&
                    ((dw1 && db1 && dw2 && db2) || (!dw1 && !db1 && !dw2 && !db2)),
                CODON_ERR_BAD_ARG, "cac_bwd_gate: null pointer (dw1 / db1 / dw2 / db2: all four or none)");
  CODON_REQUIRE(shape_ok(batch, height, width), CODON_ERR_BAD_ARG, "cac_bwd_gate: bad shape");
  return cac_bwd_gate(batch, height, width, part_gch, part_arg, ch, pools, w1, b1, w2, g_pools, argpix, part_param,
                      dw1, db1, dw2, db2, (hipStream_t)stream);
}

int codon_cac_bwd_spatial(int32_t batch, int32_t height, int32_t width, const float* g_z, const float* pooled,
                          const float* w_spatial, float* g_pooled, float* part_w, float* dw_spatial,
                          codon_stream_t stream) {
  CODON_REQUIRE(g_z && pooled && w_spatial && g_pooled && part_w, CODON_ERR_BAD_ARG, "cac_bwd_spatial: null pointer");
  CODON_REQUIRE(shape_ok(batch, height, width), CODON_ERR_BAD_ARG, "cac_bwd_spatial: bad shape");
  return cac_bwd_spatial(batch, height, width, g_z, pooled, w_spatial, g_pooled, part_w, dw_spatial,
                         (hipStream_t)stream);
}

int codon_cac_bwd_apply(int32_t batch, int32_t height, int32_t width, const codon_tensor* g_out,
                        const codon_tensor* g_out_c, const codon_tensor* pre, const codon_tensor* pre_c,
                        const float* ch, const float* sp, const float* pooled, const float* g_pooled,
                        const float* g_pools, const int32_t* argpix, const codon_tensor* g_pre,
                        const codon_tensor* g_pre_c, const codon_tensor* g_in, const codon_tensor* g_in_c,
                        int32_t accumulate_in, int32_t dtype, codon_stream_t stream) {
  CODON_REQUIRE(dtype_known(dtype), CODON_ERR_UNSUPPORTED, "cac_bwd_apply: dtype %d", dtype);
  CODON_REQUIRE(slice_ok(g_out) && slice_ok(g_out_c) && slice_ok(pre) && slice_ok(pre_c) && ch && sp && pooled &&
                    g_pooled && g_pools && argpix && slice_ok(g_pre) && slice_ok(g_pre_c) && slice_ok(g_in) &&
                    slice_ok(g_in_c),
                CODON_ERR_BAD_ARG, "cac_bwd_apply: null pointer or bad channel slice");
  CODON_REQUIRE(shape_ok(batch, height, width) && batch <= 65535, CODON_ERR_BAD_ARG, "cac_bwd_apply: bad shape");
  return cac_bwd_apply(batch, height, width, g_out, g_out_c, pre, pre_c, ch, sp, pooled, g_pooled, g_pools, argpix,
                       g_pre, g_pre_c, g_in, g_in_c, accumulate_in, dtype, (hipStream_t)stream);
}

int codon_postprocess_u8(int64_t n, const float* x, uint8_t* out, codon_stream_t stream) {
  CODON_REQUIRE(x && out && n > 0, CODON_ERR_BAD_ARG, "postprocess_u8: null pointer or n <= 0");
  return postprocess_u8(x, out, (long)n, (hipStream_t)stream);
}

int codon_postprocess_u8_dt(int64_t n, const void* x, int32_t dtype, uint8_t* out, codon_stream_t stream) {
  CODON_REQUIRE(x && out && n > 0, CODON_ERR_BAD_ARG, "postprocess_u8_dt: null pointer or n <= 0");
  CODON_REQUIRE(dtype == CODON_F32 || dtype == CODON_F16, CODON_ERR_UNSUPPORTED,
                "postprocess_u8_dt: dtype %d (fp32 or fp16; numpy has no bf16 -- upcast bf16 to fp32 first)", dtype);
  if (dtype == CODON_F16) return postprocess_u8_f16(x, out, (long)n, (hipStream_t)stream);
  return postprocess_u8((const float*)x, out, (long)n, (hipStream_t)stream);
}

int codon_masked_sqerr(int64_t n, const uint8_t* label, const uint8_t* out, uint64_t* acc, codon_stream_t stream) {
  CODON_REQUIRE(label && out && acc && n > 0, CODON_ERR_BAD_ARG, "masked_sqerr: null pointer or n <= 0");
  return masked_sqerr(label, out, (long)n, (unsigned long long*)acc, (hipStream_t)stream);
}

int codon_postprocess_u16_dt(int64_t n, const void* x, int32_t dtype, int32_t depth_max, uint16_t* out, codon_stream_t stream) {
  CODON_REQUIRE(x && out && n > 0, CODON_ERR_BAD_ARG, "postprocess_u16_dt: null pointer or n <= 0");
  CODON_REQUIRE(dtype_known(dtype), CODON_ERR_UNSUPPORTED, "postprocess_u16_dt: dtype %d (fp32, fp16 or bf16)", dtype);
  CODON_REQUIRE(depth_max >= 1 && depth_max <= 65535, CODON_ERR_BAD_ARG, "postprocess_u16_dt: depth_max %d (1..65535)",
                depth_max);
  CODON_REQUIRE(((uintptr_t)out & 1) == 0, CODON_ERR_BAD_ARG, "postprocess_u16_dt: out is not 2-byte aligned");
  return postprocess_u16(x, dtype, depth_max, out, (long)n, (hipStream_t)stream);
}

int codon_masked_sqerr_u16(int64_t n, const uint16_t* label, const uint16_t* out, uint64_t* acc, codon_stream_t stream) {
  CODON_REQUIRE(label && out && acc && n > 0, CODON_ERR_BAD_ARG, "masked_sqerr_u16: null pointer or n <= 0");
  CODON_REQUIRE(n <= ((int64_t)1 << 26), CODON_ERR_UNSUPPORTED, "masked_sqerr_u16: %lld pixels (at most 2^26)", (long long)n);
  CODON_REQUIRE((((uintptr_t)label | (uintptr_t)out) & 1) == 0, CODON_ERR_BAD_ARG, "masked_sqerr_u16: unaligned plane");
  return masked_sqerr_u16(label, out, (long)n, (unsigned long long*)acc, (hipStream_t)stream);
}

int32_t codon_ssim_tiles(int32_t batch, int32_t height, int32_t width) {
  return shape_ok(batch, height, width) ? ssim_tiles(batch, height, width) : 0;
}

int codon_ssim_fwd(int32_t batch, int32_t height, int32_t width, const float* a, const float* b, float* partial,
                   float* dmaps, double* value, codon_stream_t stream) {
  CODON_REQUIRE(a && b && partial && value, CODON_ERR_BAD_ARG, "ssim_fwd: null pointer");
  CODON_REQUIRE(shape_ok(batch, height, width), CODON_ERR_BAD_ARG, "ssim_fwd: bad shape");
  return ssim_fwd(batch, height, width, a, b, partial, dmaps, value, (hipStream_t)stream);
}

int codon_l1_fwd(int64_t n, const float* a, const float* b, float* partial, int32_t nparts, double* value,
                 codon_stream_t stream) {
  CODON_REQUIRE(a && b && partial && value && n > 0 && nparts > 0, CODON_ERR_BAD_ARG, "l1_fwd: bad argument");
  return l1_fwd((long)n, a, b, partial, nparts, value, (hipStream_t)stream);
}

int codon_ssim_l1_bwd(int32_t batch, int32_t height, int32_t width, const float* a, const float* b,
                      const float* dmaps, float* tmp, float* ga, float ssim_scale, float l1_scale,
                      codon_stream_t stream) {
  CODON_REQUIRE(a && b && dmaps && tmp && ga, CODON_ERR_BAD_ARG, "ssim_l1_bwd: null pointer");
  CODON_REQUIRE(shape_ok(batch, height, width) && height >= 7 && width >= 7, CODON_ERR_UNSUPPORTED,
                "ssim_l1_bwd: needs H, W >= 7 (got %dx%d)", height, width);
  return ssim_l1_bwd(batch, height, width, a, b, dmaps, tmp, ga, ssim_scale, l1_scale, (hipStream_t)stream);
}

int codon_masked_l1_ssim_fwd(int32_t batch, int32_t height, int32_t width, const float* pred, const float* target,
                             const uint8_t* valid, float* ws, float* dmaps, double w_l1, double w_ssim, int64_t* counts,
                             double* per_image, float* scales, double* value, codon_stream_t stream) {
  CODON_REQUIRE(pred && target && ws && counts && per_image && scales && value, CODON_ERR_BAD_ARG,
                "masked_l1_ssim_fwd: null pointer");
  CODON_REQUIRE(shape_ok(batch, height, width), CODON_ERR_BAD_ARG, "masked_l1_ssim_fwd: bad shape");
  return masked_l1_ssim_fwd(batch, height, width, pred, target, valid, ws, dmaps, w_l1, w_ssim, (long long*)counts, per_image,
                            scales, value, (hipStream_t)stream);
}

int codon_masked_l1_ssim_bwd(int32_t batch, int32_t height, int32_t width, const float* pred, const float* target,
                             const uint8_t* valid, const float* dmaps, const float* scales, const float* upstream, float* tmp,
                             float* ga, codon_stream_t stream) {
  CODON_REQUIRE(pred && target && dmaps && scales && upstream && tmp && ga, CODON_ERR_BAD_ARG,
                "masked_l1_ssim_bwd: null pointer");
  CODON_REQUIRE(shape_ok(batch, height, width) && height >= 7 && width >= 7, CODON_ERR_UNSUPPORTED,
                "masked_l1_ssim_bwd: needs H, W >= 7 (got %dx%d)", height, width);
  return masked_l1_ssim_bwd(batch, height, width, pred, target, valid, dmaps, scales, upstream, tmp, ga, (hipStream_t)stream);
}

int codon_bicubic_upsample(int32_t batch, int32_t lr_height, int32_t lr_width, int32_t scale, const float* lr,
                           const float* phase_weights, float* out, codon_stream_t stream) {
  CODON_REQUIRE(lr && phase_weights && out, CODON_ERR_BAD_ARG, "bicubic_upsample: null pointer");
  CODON_REQUIRE(scale == 4 || scale == 8 || scale == 16, CODON_ERR_UNSUPPORTED, "bicubic_upsample: scale %d", scale);
  CODON_REQUIRE(shape_ok(batch, lr_height * scale, lr_width * scale), CODON_ERR_BAD_ARG, "bicubic_upsample: bad shape");
  return bicubic_upsample(batch, lr_height, lr_width, scale, lr, phase_weights, out, (hipStream_t)stream);
}

int codon_train_crops(const codon_crop_desc* desc, const uint8_t* pool, int64_t pool_bytes, const float* lut, float* target,
                      float* guide, codon_stream_t stream) {
  CODON_REQUIRE(desc && pool && lut && target && guide, CODON_ERR_BAD_ARG, "train_crops: null pointer");
  if (const int st = check_crop_desc("train_crops", desc, pool_bytes, 8, false, 0)) return st;
  return train_crops(desc, pool, 8, lut, lut, target, guide, nullptr, (hipStream_t)stream);
}

int codon_train_crops_labeled(const codon_crop_desc* desc, const uint8_t* pool, int64_t pool_bytes, const float* lut,
                              float* source, float* guide, float* target, codon_stream_t stream) {
  CODON_REQUIRE(desc && pool && lut && source && guide && target, CODON_ERR_BAD_ARG, "train_crops_labeled: null pointer");
  if (const int st = check_crop_desc("train_crops_labeled", desc, pool_bytes, 8, true, 0)) return st;
  return train_crops(desc, pool, 8, lut, lut, source, guide, target, (hipStream_t)stream);
}

int codon_bicubic_downsample(int32_t batch, int32_t size, int32_t scale, const float* hr, const float* weights, float* out,
                             codon_stream_t stream) {
  CODON_REQUIRE(hr && weights && out, CODON_ERR_BAD_ARG, "bicubic_downsample: null pointer");
  CODON_REQUIRE(scale == 4 || scale == 8 || scale == 16, CODON_ERR_UNSUPPORTED, "bicubic_downsample: scale %d", scale);
  CODON_REQUIRE(batch >= 1 && batch < 65536 && size >= 4 * scale && size <= 2048 && size % scale == 0, CODON_ERR_BAD_ARG,
                "bicubic_downsample: batch %d, size %d at scale %d", batch, size, scale);
  return bicubic_downsample(batch, size, scale, hr, weights, out, (hipStream_t)stream);
}

int codon_quantize_u8(int64_t n, float* x, const float* lut, codon_stream_t stream) {
  CODON_REQUIRE(x && lut && n >= 1, CODON_ERR_BAD_ARG, "quantize_u8: null pointer or empty");
  return quantize_levels((long)n, x, lut, 255, (hipStream_t)stream);
}

int codon_train_crops_u16(const codon_crop_desc* desc, const uint8_t* pool, int64_t pool_bytes, const float* lut16,
                          const float* lut8, float* source, float* guide, float* target, codon_stream_t stream) {
  CODON_REQUIRE(desc && pool && lut16 && lut8 && source && guide, CODON_ERR_BAD_ARG, "train_crops_u16: null pointer");
  CODON_REQUIRE(((uintptr_t)pool & 1) == 0, CODON_ERR_BAD_ARG, "train_crops_u16: the pool is not 2-byte aligned");
  if (const int st = check_crop_desc("train_crops_u16", desc, pool_bytes, 16, target != nullptr, 0)) return st;
  return train_crops(desc, pool, 16, lut16, lut8, source, guide, target, (hipStream_t)stream);
}

int codon_quantize_levels(int64_t n, float* x, const float* lut16, int32_t depth_max, codon_stream_t stream) {
  CODON_REQUIRE(x && lut16 && n >= 1, CODON_ERR_BAD_ARG, "quantize_levels: null pointer or empty");
  CODON_REQUIRE(depth_max >= 1 && depth_max <= 65535, CODON_ERR_BAD_ARG, "quantize_levels: depth_max %d (1..65535)", depth_max);
  return quantize_levels((long)n, x, lut16, depth_max, (hipStream_t)stream);
}

int codon_bicubic_upsample_masked(int32_t batch, int32_t lr_height, int32_t lr_width, int32_t scale, const float* lr,
                                  const float* phase_weights, float* out, uint8_t* valid, codon_stream_t stream) {
  CODON_REQUIRE(lr && phase_weights && out, CODON_ERR_BAD_ARG, "bicubic_upsample_masked: null pointer");
  CODON_REQUIRE(scale == 4 || scale == 8 || scale == 16, CODON_ERR_UNSUPPORTED, "bicubic_upsample_masked: scale %d", scale);
  CODON_REQUIRE(lr_height >= 1 && lr_width >= 1 && lr_height <= 65536 && lr_width <= 65536 &&
                    shape_ok(batch, lr_height * scale, lr_width * scale),
                CODON_ERR_BAD_ARG, "bicubic_upsample_masked: bad shape");
  return bicubic_upsample_masked(batch, lr_height, lr_width, scale, lr, phase_weights, out, valid, (hipStream_t)stream);
}

int codon_bicubic_downsample_masked(int32_t batch, int32_t size, int32_t scale, const float* hr, const float* weights,
                                    const float* lut, int32_t levels, float* out, codon_stream_t stream) {
  CODON_REQUIRE(hr && weights && lut && out, CODON_ERR_BAD_ARG, "bicubic_downsample_masked: null pointer");
  CODON_REQUIRE(scale == 4 || scale == 8 || scale == 16, CODON_ERR_UNSUPPORTED, "bicubic_downsample_masked: scale %d", scale);
  CODON_REQUIRE(batch >= 1 && batch < 65536 && size >= 4 * scale && size <= 1024 && size % scale == 0, CODON_ERR_BAD_ARG,
                "bicubic_downsample_masked: batch %d, size %d at scale %d (size: a multiple of the scale, 4 * scale .. 1024)",
                batch, size, scale);
  CODON_REQUIRE(levels >= 1 && levels <= 65535, CODON_ERR_BAD_ARG, "bicubic_downsample_masked: levels %d (1..65535)", levels);
  return bicubic_downsample_masked(batch, size, scale, hr, weights, lut, levels, out, (hipStream_t)stream);
}

int codon_lr_codes_to_input(int32_t batch, int32_t lr_height, int32_t lr_width, int32_t scale, const void* codes,
                            int32_t code_bits, const float* lut, int32_t depth_max, const float* phase_weights, void* out,
                            int32_t dtype, codon_stream_t stream) {
  CODON_REQUIRE(codes && lut && phase_weights && out, CODON_ERR_BAD_ARG, "lr_codes_to_input: null pointer");
  CODON_REQUIRE(scale == 4 || scale == 8 || scale == 16, CODON_ERR_UNSUPPORTED, "lr_codes_to_input: scale %d", scale);
  CODON_REQUIRE(dtype_known(dtype), CODON_ERR_UNSUPPORTED, "lr_codes_to_input: dtype %d (fp32, fp16 or bf16)", dtype);
  if (const int st = check_lr_codes("lr_codes_to_input", batch, lr_height, lr_width, scale, codes, code_bits, depth_max, out)) return st;
  return lr_codes_to_input(batch, lr_height, lr_width, scale, codes, code_bits, lut, depth_max, phase_weights, out, dtype,
                           (hipStream_t)stream);
}

int codon_lr_codes_upsample(int32_t batch, int32_t lr_height, int32_t lr_width, int32_t scale, const void* codes,
                            int32_t code_bits, const float* lut, int32_t depth_max, const float* phase_weights, void* out,
                            codon_stream_t stream) {
  CODON_REQUIRE(codes && lut && phase_weights && out, CODON_ERR_BAD_ARG, "lr_codes_upsample: null pointer");
  CODON_REQUIRE(scale == 4 || scale == 8 || scale == 16, CODON_ERR_UNSUPPORTED, "lr_codes_upsample: scale %d", scale);
  if (const int st = check_lr_codes("lr_codes_upsample", batch, lr_height, lr_width, scale, codes, code_bits, depth_max, out)) return st;
  if (const int st = check_not_same("lr_codes_upsample", codes, out, "codes")) return st;
  return lr_codes_upsample(batch, lr_height, lr_width, scale, codes, code_bits, lut, depth_max, phase_weights, out,
                           (hipStream_t)stream);
}

int codon_train_crops_lr(const codon_crop_desc* desc, const uint8_t* pool, int64_t pool_bytes, int32_t scale, int32_t code_bits,
                         const float* lut, int32_t depth_max, const float* lut8, const float* phase_weights, float* x,
                         float* guide, float* target, codon_stream_t stream) {
  CODON_REQUIRE(desc && pool && lut && lut8 && phase_weights && x && guide && target, CODON_ERR_BAD_ARG,
                "train_crops_lr: null pointer");
  CODON_REQUIRE(scale == 4 || scale == 8 || scale == 16, CODON_ERR_UNSUPPORTED, "train_crops_lr: scale %d", scale);
  CODON_REQUIRE(code_bits == 8 || code_bits == 16, CODON_ERR_BAD_ARG, "train_crops_lr: code_bits %d (8 or 16)", code_bits);
  CODON_REQUIRE(code_bits == 16 ? (depth_max >= 1 && depth_max <= 65535) : depth_max == 255, CODON_ERR_BAD_ARG,
                "train_crops_lr: depth_max %d (255 for 8-bit codes, 1..65535 for 16-bit codes)", depth_max);
  CODON_REQUIRE(code_bits == 8 || ((uintptr_t)pool & 1) == 0, CODON_ERR_BAD_ARG, "train_crops_lr: the pool is not 2-byte aligned");
  if (const int st = check_crop_desc("train_crops_lr", desc, pool_bytes, code_bits, false, scale)) return st;
  return train_crops_lr(desc, pool, scale, code_bits, lut, depth_max, lut8, phase_weights, x, guide, target, (hipStream_t)stream);
}

int codon_d4_views(int32_t batch, int32_t height, int32_t width, const void* src0, const void* src1, int32_t dtype,
                   void* upright0, void* transposed0, void* upright1, void* transposed1, codon_stream_t stream) {
  CODON_REQUIRE(src0 && upright0 && transposed0, CODON_ERR_BAD_ARG, "d4_views: null pointer");
  CODON_REQUIRE(src1 ? (upright1 && transposed1) : (!upright1 && !transposed1), CODON_ERR_BAD_ARG,
                "d4_views: src1, upright1 and transposed1 go together (all three, or all three NULL)");
  CODON_REQUIRE(shape_ok(batch, height, width), CODON_ERR_BAD_ARG, "d4_views: bad shape %dx%dx%d", batch, height, width);
  CODON_REQUIRE(dtype_known(dtype), CODON_ERR_BAD_ARG, "d4_views: dtype %d", dtype);
  CODON_REQUIRE(batch <= 32767, CODON_ERR_UNSUPPORTED, "d4_views: batch %d (at most 32767 images per launch)", batch);
  return d4_views(batch, height, width, src0, src1, dtype, upright0, transposed0, upright1, transposed1, (hipStream_t)stream);
}

int codon_d4_merge(int32_t batch, int32_t height, int32_t width, const void* upright, const void* transposed, int32_t dtype,
                   float* out_f32, codon_stream_t stream) {
  CODON_REQUIRE(upright && transposed && out_f32, CODON_ERR_BAD_ARG, "d4_merge: null pointer");
  CODON_REQUIRE(shape_ok(batch, height, width), CODON_ERR_BAD_ARG, "d4_merge: bad shape %dx%dx%d", batch, height, width);
  CODON_REQUIRE(dtype_known(dtype), CODON_ERR_BAD_ARG, "d4_merge: dtype %d", dtype);
  CODON_REQUIRE(batch <= 32767, CODON_ERR_UNSUPPORTED, "d4_merge: batch %d (at most 32767 images per launch)", batch);
  return d4_merge(batch, height, width, upright, transposed, dtype, out_f32, (hipStream_t)stream);
}

int codon_philox4x32_10(const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
  CODON_REQUIRE(ctr && key && out, CODON_ERR_BAD_ARG, "philox4x32_10: null pointer");
  const Philox4 r = philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
  for (int k = 0; k < 4; ++k) out[k] = r.w[k];
  return CODON_OK;
}

int codon_lr_sensor(const codon_sensor_desc* desc, const float* lr, const float* gauss, const float* lut, int32_t levels,
                    float* out, codon_stream_t stream) {
  CODON_REQUIRE(desc && lr && gauss && lut && out, CODON_ERR_BAD_ARG, "lr_sensor: null pointer");
  CODON_REQUIRE(lr != out, CODON_ERR_BAD_ARG, "lr_sensor: lr and out are the same buffer (the edge term reads lr's neighbours)");
  CODON_REQUIRE(desc->batch >= 1 && desc->batch <= CODON_TRAIN_MAX_BATCH, CODON_ERR_BAD_ARG, "lr_sensor: batch %d (1..%d)",
                desc->batch, CODON_TRAIN_MAX_BATCH);
  CODON_REQUIRE(desc->size >= 4 && desc->size <= 512, CODON_ERR_BAD_ARG, "lr_sensor: size %d (4..512)", desc->size);
  CODON_REQUIRE(levels >= 1 && levels <= 65535, CODON_ERR_BAD_ARG, "lr_sensor: levels %d (1..65535)", levels);
  CODON_REQUIRE(desc->step >= 0 && desc->step <= 0xFFFFFFFFll, CODON_ERR_BAD_ARG, "lr_sensor: step %lld (0..2^32-1)",
                (long long)desc->step);
  CODON_REQUIRE(desc->first_sample >= 0 && desc->first_sample + desc->batch <= 0x100000000ll, CODON_ERR_BAD_ARG,
                "lr_sensor: first_sample %lld (with the batch: 0..2^32)", (long long)desc->first_sample);
  CODON_REQUIRE(isfinite(desc->sigma) && desc->sigma >= 0.f, CODON_ERR_BAD_ARG, "lr_sensor: sigma %g is negative or not finite",
                (double)desc->sigma);
  CODON_REQUIRE(isfinite(desc->quad) && desc->quad >= 0.f, CODON_ERR_BAD_ARG, "lr_sensor: quad %g is negative or not finite",
                (double)desc->quad);
  CODON_REQUIRE(isfinite(desc->edge_thr) && desc->edge_thr >= 0.f, CODON_ERR_BAD_ARG,
                "lr_sensor: edge_thr %g is negative or not finite", (double)desc->edge_thr);
  CODON_REQUIRE(desc->p_drop >= 0.0 && desc->p_drop <= 1.0, CODON_ERR_BAD_ARG, "lr_sensor: p_drop %g outside [0, 1]", desc->p_drop);
  CODON_REQUIRE(desc->p_edge >= 0.0 && desc->p_edge <= 1.0, CODON_ERR_BAD_ARG, "lr_sensor: p_edge %g outside [0, 1]", desc->p_edge);
  CODON_REQUIRE(desc->p_drop + desc->p_edge <= 1.0, CODON_ERR_BAD_ARG, "lr_sensor: p_drop + p_edge = %g exceeds 1",
                desc->p_drop + desc->p_edge);
  CODON_REQUIRE(desc->masked != 0 || (desc->p_drop == 0.0 && desc->p_edge == 0.0), CODON_ERR_BAD_ARG,
                "lr_sensor: masked 0 with p_drop %g, p_edge %g (without the masked upsample a dropped pixel would ring)",
                desc->p_drop, desc->p_edge);
  SensorArgs a;
  a.p = desc->size;
  a.masked = desc->masked != 0 ? 1 : 0;
  a.levels = levels;
  a.k0 = desc->seed_lo;
  a.k1 = desc->seed_hi;
  a.step = (unsigned)desc->step;
  a.first = (unsigned)desc->first_sample;
  a.sigma = desc->sigma;
  a.quad = desc->quad;
  a.edge_thr = desc->edge_thr;
  a.t_drop = (unsigned long long)floor(desc->p_drop * 4294967296.0);      // NaN fails the range checks above
  a.t_edge = (unsigned long long)floor(desc->p_edge * 4294967296.0);
  return lr_sensor(a, desc->batch, lr, gauss, lut, out, (hipStream_t)stream);
}

// ---- depth evaluation suite ---------------------------------------------------------------------------------
int codon_depth_errors(const codon_depth_errors_desc* desc, const void* label, const void* out, uint64_t* acc, void* error_map,
                       uint8_t* region_map, codon_stream_t stream) {
  CODON_REQUIRE(desc && label && out && acc, CODON_ERR_BAD_ARG, "depth_errors: null pointer");
  CODON_REQUIRE(desc->bits == 8 || desc->bits == 16, CODON_ERR_BAD_ARG, "depth_errors: bits %d (8 or 16)", desc->bits);
  CODON_REQUIRE(shape_ok(desc->batch, desc->height, desc->width), CODON_ERR_BAD_ARG, "depth_errors: bad shape %dx%dx%d",
                desc->batch, desc->height, desc->width);
  CODON_REQUIRE((int64_t)desc->height * desc->width <= ((int64_t)1 << 26), CODON_ERR_UNSUPPORTED,
                "depth_errors: %lld pixels per image (at most 2^26)", (long long)desc->height * desc->width);
  CODON_REQUIRE(desc->batch <= 65535 && (desc->height + EV_TILE - 1) / EV_TILE <= 65535, CODON_ERR_UNSUPPORTED,
                "depth_errors: %d images of %d rows (at most 65535 images and 65535 tile rows per launch)", desc->batch,
                desc->height);
  CODON_REQUIRE(desc->label_height >= desc->height && desc->label_width >= desc->width, CODON_ERR_BAD_ARG,
                "depth_errors: a %dx%d label is smaller than the %dx%d output", desc->label_height, desc->label_width,
                desc->height, desc->width);
  CODON_REQUIRE(desc->label_row_stride >= desc->label_width && desc->label_image_stride >= 0 &&
                    (desc->batch == 1 || desc->label_image_stride >= desc->label_row_stride * (desc->label_height - 1) + desc->label_width),
                CODON_ERR_BAD_ARG, "depth_errors: label strides %lld (row), %lld (image) for %dx%d planes",
                (long long)desc->label_row_stride, (long long)desc->label_image_stride, desc->label_height, desc->label_width);
  CODON_REQUIRE(desc->bits == 8 || (((uintptr_t)label | (uintptr_t)out | (uintptr_t)error_map) & 1) == 0, CODON_ERR_BAD_ARG,
                "depth_errors: unaligned u16 plane");
  CODON_REQUIRE(desc->n_thresholds >= 0 && desc->n_thresholds <= EV_MAX_THRESHOLDS, CODON_ERR_BAD_ARG,
                "depth_errors: %d thresholds (at most %d)", desc->n_thresholds, EV_MAX_THRESHOLDS);
  EvalArgs a;
  for (int k = 0; k < EV_MAX_THRESHOLDS; ++k) {
    a.thr[k] = k < desc->n_thresholds ? desc->thresholds[k] : 0;
    CODON_REQUIRE(a.thr[k] >= 0, CODON_ERR_BAD_ARG, "depth_errors: threshold %d is negative (%d)", k, a.thr[k]);
  }
  CODON_REQUIRE(desc->edge == 0 || desc->edge_threshold >= 0, CODON_ERR_BAD_ARG, "depth_errors: edge_threshold %d is negative",
                desc->edge_threshold);
  CODON_REQUIRE(desc->edge == 0 || (desc->edge_radius >= 0 && desc->edge_radius <= EV_RMAX), CODON_ERR_BAD_ARG,
                "depth_errors: edge_radius %d (0..%d)", desc->edge_radius, EV_RMAX);
  a.H = desc->height;
  a.W = desc->width;
  a.label_row = (long)desc->label_row_stride;
  a.label_image = (long)desc->label_image_stride;
  a.nthr = desc->n_thresholds;
  a.edge = desc->edge != 0 ? 1 : 0;
  a.edge_thr = a.edge ? desc->edge_threshold : 0;
  a.r = a.edge ? desc->edge_radius : 0;
  return depth_errors(a, desc->batch, desc->bits, label, out, error_map, region_map, (unsigned long long*)acc,
                      (hipStream_t)stream);
}

// ---- surface-normal angle error -----------------------------------------------------------------------------------
int codon_normal_errors(int32_t batch, int32_t height, int32_t width, const void* label, int32_t label_height, int32_t label_width,
                        int64_t label_row_stride, int64_t label_image_stride, const void* out, int32_t fmt, int32_t top,
                        const int32_t* rx, const int32_t* ry, const int32_t* ray_span, const int32_t* cos_table,
                        const int32_t* sin_table, int32_t radius, int32_t tol_abs, int32_t tol_rel_q16, uint32_t* words,
                        uint16_t* angle_map, codon_stream_t stream) {
  CODON_REQUIRE(label && out && rx && ry && ray_span && cos_table && sin_table && words, CODON_ERR_BAD_ARG,
                "normal_errors: null pointer");
  const char* who = "normal_errors";
  if (const int st = check_planes(who, fmt, batch, height, width, NE_MAX_SIDE, top)) return st;
  CODON_REQUIRE(label_height >= height && label_width >= width, CODON_ERR_BAD_ARG,
                "normal_errors: a %dx%d label is smaller than the %dx%d output", label_height, label_width, height, width);
  CODON_REQUIRE(label_row_stride >= label_width && label_image_stride >= 0 &&
                    (batch == 1 || label_image_stride >= label_row_stride * (label_height - 1) + label_width),
                CODON_ERR_BAD_ARG, "normal_errors: label strides %lld (row), %lld (image) for %dx%d planes",
                (long long)label_row_stride, (long long)label_image_stride, label_height, label_width);
  CODON_REQUIRE(radius >= 1 && radius <= NE_RMAX, CODON_ERR_BAD_ARG, "normal_errors: radius %d (1..%d)", radius, NE_RMAX);
  if (const int st = check_link_tolerances(who, tol_abs, top, tol_rel_q16, CD_MAX_REL)) return st;
  for (int q = 0; q < 4; ++q)
    CODON_REQUIRE(ray_span[q] > -CD_RAY_LIMIT && ray_span[q] < CD_RAY_LIMIT, CODON_ERR_BAD_ARG,
                  "normal_errors: ray %d of the span is %d (Q20, below 2^22 in magnitude)", q, ray_span[q]);
  const bool planes_ok = (((uintptr_t)label | (uintptr_t)out) & (uintptr_t)(fl_elem_bytes(fmt) - 1)) == 0;
  const bool words_ok = (((uintptr_t)rx | (uintptr_t)ry | (uintptr_t)cos_table | (uintptr_t)sin_table | (uintptr_t)words) & 3) == 0 &&
                        ((uintptr_t)angle_map & 1) == 0;
  CODON_REQUIRE(planes_ok && words_ok, CODON_ERR_BAD_ARG, "normal_errors: unaligned plane, table, words or map");
  NeArgs a;
  a.H = height, a.W = width, a.label_row = (long)label_row_stride, a.label_image = (long)label_image_stride;
  a.radius = radius, a.tol_abs = (unsigned)(radius * tol_abs), a.tol_rel = (unsigned)tol_rel_q16;
  return normal_errors(a, batch, fmt, label, out, rx, ry, cos_table, sin_table, words, angle_map, (hipStream_t)stream);
}

// ---- pull-push hole filling -----------------------------------------------------------------------------------
size_t codon_fill_holes_workspace_bytes(int32_t height, int32_t width) { return fill_holes_workspace_bytes(height, width); }

int codon_fill_holes(int32_t batch, int32_t height, int32_t width, const void* in, int32_t fmt, const float* tab, int32_t top,
                     void* out, void* workspace, size_t workspace_bytes, codon_stream_t stream) {
  CODON_REQUIRE(in && out && workspace, CODON_ERR_BAD_ARG, "fill_holes: null pointer");
  const char* who = "fill_holes";
  CODON_REQUIRE(fmt == FL_U8 || fmt == FL_U16 || fmt == FL_F32, CODON_ERR_BAD_ARG,
                "fill_holes: fmt %d (0: u8 codes, 1: u16 codes, 2: fp32 on the code grid)", fmt);
  CODON_REQUIRE(fmt != FL_F32 || tab, CODON_ERR_BAD_ARG, "fill_holes: null pointer (the fp32 format needs tab)");
  if (const int st = check_batch(who, batch)) return st;
  if (const int st = check_side(who, height, width, "plane", FL_MAX_SIDE)) return st;
  if (const int st = check_top(who, fmt, top)) return st;
  if (const int st = check_not_same(who, in, out)) return st;
  CODON_REQUIRE((((uintptr_t)in | (uintptr_t)out) & (uintptr_t)(fl_elem_bytes(fmt) - 1)) == 0 && ((uintptr_t)workspace & 1) == 0,
                CODON_ERR_BAD_ARG, "fill_holes: unaligned plane or workspace");
  if (const int st = check_workspace(who, workspace_bytes, (size_t)batch * fill_holes_workspace_bytes(height, width))) return st;
  return fill_holes(batch, height, width, in, fmt, tab, top, out, workspace, (hipStream_t)stream);
}

// ---- guidance-aware pull-push hole filling ---------------------------------------------------------------------
size_t codon_fill_guided_workspace_bytes(int32_t height, int32_t width) { return fill_guided_workspace_bytes(height, width); }

int codon_fill_holes_guided(int32_t batch, int32_t height, int32_t width, const void* in, int32_t fmt, int32_t top,
                            const uint8_t* guide, int64_t guide_row_bytes, int64_t guide_image_bytes, int32_t scale,
                            const uint16_t* range_tab, void* out, void* workspace, size_t workspace_bytes, codon_stream_t stream) {
  CODON_REQUIRE(in && out && workspace && guide && range_tab, CODON_ERR_BAD_ARG, "fill_holes_guided: null pointer");
  const char* who = "fill_holes_guided";
  if (const int st = check_planes(who, fmt, batch, height, width, FL_MAX_SIDE, top)) return st;
  if (const int st = check_guide(who, batch, height, width, scale, guide_row_bytes, guide_image_bytes)) return st;
  if (const int st = check_not_same(who, in, out)) return st;
  const bool planes_ok = (((uintptr_t)in | (uintptr_t)out) & (uintptr_t)(fl_elem_bytes(fmt) - 1)) == 0;      // u16 codes: 2 bytes
  const bool tab_ok = ((uintptr_t)range_tab & 1) == 0, ws_ok = ((uintptr_t)workspace & 15) == 0;             // u16 entries; 16 bytes
  CODON_REQUIRE(planes_ok && tab_ok && ws_ok, CODON_ERR_BAD_ARG, "fill_holes_guided: unaligned plane, table or workspace");
  if (const int st = check_workspace(who, workspace_bytes, (size_t)batch * fill_guided_workspace_bytes(height, width))) return st;
  return fill_holes_guided(batch, height, width, in, fmt, top, guide, (long)guide_row_bytes,
                           batch == 1 ? 0L : (long)guide_image_bytes, scale, range_tab, out, workspace, (hipStream_t)stream);
}

// ---- joint bilateral upsampling ----------------------------------------------------------------------------------
size_t codon_jbu_workspace_bytes(int32_t height, int32_t width) { return jbu_workspace_bytes(height, width); }

int codon_jbu_upsample(int32_t batch, int32_t height, int32_t width, const void* in, int32_t fmt, int32_t top, const uint8_t* guide,
                       int64_t guide_row_bytes, int64_t guide_image_bytes, int32_t scale, const uint16_t* range_tab,
                       const uint16_t* spatial_tab, void* out, void* workspace, size_t workspace_bytes, codon_stream_t stream) {
  CODON_REQUIRE(in && out && workspace && guide && range_tab && spatial_tab, CODON_ERR_BAD_ARG, "jbu_upsample: null pointer");
  const char* who = "jbu_upsample";
  if (const int st = check_planes(who, fmt, batch, height, width, FL_MAX_SIDE, top)) return st;
  if (const int st = check_guide(who, batch, height, width, scale, guide_row_bytes, guide_image_bytes)) return st;
  if (const int st = check_not_same(who, in, out)) return st;
  const bool planes_ok = ((uintptr_t)in & (uintptr_t)(fl_elem_bytes(fmt) - 1)) == 0 && ((uintptr_t)out & 15) == 0;
  const bool tab_ok = (((uintptr_t)range_tab | (uintptr_t)spatial_tab) & 1) == 0, ws_ok = ((uintptr_t)workspace & 15) == 0;
  CODON_REQUIRE(planes_ok && tab_ok && ws_ok, CODON_ERR_BAD_ARG, "jbu_upsample: unaligned plane, table or workspace");
  if (const int st = check_workspace(who, workspace_bytes, (size_t)batch * jbu_workspace_bytes(height, width))) return st;
  return jbu_upsample(batch, height, width, in, fmt, guide, (long)guide_row_bytes, batch == 1 ? 0L : (long)guide_image_bytes, scale,
                      range_tab, spatial_tab, out, workspace, (hipStream_t)stream);
}

// ---- registration of depth maps to the colour camera ---------------------------------------------------------------
size_t codon_register_workspace_bytes(int32_t out_height, int32_t out_width) { return register_workspace_bytes(out_height, out_width); }

int codon_register_depth(int32_t batch, int32_t src_height, int32_t src_width, const void* in, int32_t fmt, int32_t top,
                         const int32_t* rays, const int64_t* trans, const int32_t* proj, int32_t out_height, int32_t out_width,
                         void* out, uint32_t* stats, void* workspace, size_t workspace_bytes, codon_stream_t stream) {
  CODON_REQUIRE(in && out && workspace && rays && trans && proj, CODON_ERR_BAD_ARG, "register_depth: null pointer");
  const char* who = "register_depth";
  if (const int st = check_fmt(who, fmt)) return st;
  if (const int st = check_batch(who, batch)) return st;
  if (const int st = check_side(who, src_height, src_width, "source", RG_MAX_SIDE)) return st;
  if (const int st = check_side(who, out_height, out_width, "target", RG_MAX_SIDE)) return st;
  if (const int st = check_top(who, fmt, top)) return st;
  for (int q = 0; q < 3; ++q)
    CODON_REQUIRE(trans[q] > -RG_T_LIMIT && trans[q] < RG_T_LIMIT, CODON_ERR_BAD_ARG,
                  "register_depth: translation %d is %lld (Q20 codes, below 2^38 in magnitude)", q, (long long)trans[q]);
  CODON_REQUIRE(proj[0] >= 1 && proj[0] < RG_F_LIMIT && proj[1] >= 1 && proj[1] < RG_F_LIMIT, CODON_ERR_BAD_ARG,
                "register_depth: projection FX %d, FY %d (Q8 pixels, 1 .. 2^20 - 1)", proj[0], proj[1]);
  CODON_REQUIRE(proj[2] > -RG_C_LIMIT && proj[2] < RG_C_LIMIT && proj[3] > -RG_C_LIMIT && proj[3] < RG_C_LIMIT, CODON_ERR_BAD_ARG,
                "register_depth: projection CX %d, CY %d (Q8 pixels, below 2^21 in magnitude)", proj[2], proj[3]);
  if (const int st = check_not_same(who, in, out)) return st;
  const bool planes_ok = (((uintptr_t)in | (uintptr_t)out) & (uintptr_t)(fl_elem_bytes(fmt) - 1)) == 0;
  const bool words_ok = (((uintptr_t)rays | (uintptr_t)stats) & 3) == 0 && ((uintptr_t)workspace & 15) == 0;
  CODON_REQUIRE(planes_ok && words_ok, CODON_ERR_BAD_ARG, "register_depth: unaligned plane, table, statistics or workspace");
  if (const int st = check_workspace(who, workspace_bytes, (size_t)batch * register_workspace_bytes(out_height, out_width))) return st;
  return register_depth(batch, src_height, src_width, in, fmt, top, rays, (const long long*)trans, proj, out_height, out_width, out,
                        stats, workspace, (hipStream_t)stream);
}

// ---- outlier rejection of sensor depth maps -------------------------------------------------------------------------
size_t codon_clean_workspace_bytes(int32_t batch, int32_t height, int32_t width) { return clean_workspace_bytes(batch, height, width); }

int codon_clean_depth(int32_t batch, int32_t height, int32_t width, const void* in, int32_t fmt, int32_t top, int32_t tol_abs,
                      int32_t tol_rel_q16, int32_t min_support, int32_t min_region, void* out, uint32_t* counts, void* workspace,
                      size_t workspace_bytes, codon_stream_t stream) {
  CODON_REQUIRE(in && out && workspace, CODON_ERR_BAD_ARG, "clean_depth: null pointer");
  const char* who = "clean_depth";
  if (const int st = check_planes(who, fmt, batch, height, width, CL_MAX_SIDE, top)) return st;
  if (const int st = check_link_tolerances(who, tol_abs, top, tol_rel_q16, CL_MAX_REL)) return st;
  CODON_REQUIRE(min_support >= 0 && min_support <= CL_MAX_SUPPORT, CODON_ERR_BAD_ARG, "clean_depth: min_support %d (0..%d)",
                min_support, CL_MAX_SUPPORT);
  CODON_REQUIRE(min_region >= 0 && min_region <= CL_MAX_REGION, CODON_ERR_BAD_ARG, "clean_depth: min_region %d (0..%d)", min_region,
                CL_MAX_REGION);
  if (const int st = check_not_same(who, in, out)) return st;
  const bool planes_ok = (((uintptr_t)in | (uintptr_t)out) & (uintptr_t)(fl_elem_bytes(fmt) - 1)) == 0;
  const bool words_ok = ((uintptr_t)counts & 3) == 0 && ((uintptr_t)workspace & 15) == 0;
  CODON_REQUIRE(planes_ok && words_ok, CODON_ERR_BAD_ARG, "clean_depth: unaligned plane, statistics or workspace");
  if (const int st = check_workspace(who, workspace_bytes, clean_workspace_bytes(batch, height, width))) return st;
  return clean_depth(batch, height, width, in, fmt, tol_abs, tol_rel_q16, min_support, min_region, out, counts, workspace,
                     (hipStream_t)stream);
}

// ---- spatial smoothing of sensor depth maps -------------------------------------------------------------------------
static int check_smooth_window(const char* who, int radius, int passes) {
  CODON_REQUIRE(radius >= 1 && radius <= SM_MAX_RADIUS, CODON_ERR_BAD_ARG, "%s: radius %d (1..%d)", who, radius, SM_MAX_RADIUS);
  CODON_REQUIRE(passes >= 1 && passes <= SM_MAX_PASSES, CODON_ERR_BAD_ARG, "%s: passes %d (1..%d)", who, passes, SM_MAX_PASSES);
  return CODON_OK;
}

int32_t codon_smooth_plan(int32_t radius, int32_t passes, int32_t* plan) {
  if (check_smooth_window("smooth_plan", radius, passes)) return 0;
  if (plan) plan[0] = SMOOTH_TILE, plan[1] = smooth_fuse_bound(radius), plan[2] = smooth_fused(radius, passes);
  return smooth_launches(radius, passes);
}

size_t codon_smooth_workspace_bytes(int32_t batch, int32_t height, int32_t width) { return smooth_workspace_bytes(batch, height, width); }

int codon_smooth_depth(int32_t batch, int32_t height, int32_t width, const void* in, int32_t fmt, int32_t top, int32_t radius,
                       int32_t passes, int32_t tol_abs, int32_t tol_rel_q16, int32_t pairs, const int32_t* weights, void* out,
                       uint32_t* counts, void* workspace, size_t workspace_bytes, codon_stream_t stream) {
  const char* who = "smooth_depth";
  CODON_REQUIRE(in && out && weights, CODON_ERR_BAD_ARG, "smooth_depth: null pointer");
  if (const int st = check_planes(who, fmt, batch, height, width, SM_MAX_SIDE, top)) return st;
  if (const int st = check_smooth_window(who, radius, passes)) return st;
  if (const int st = check_link_tolerances(who, tol_abs, top, tol_rel_q16, SM_MAX_REL)) return st;
  CODON_REQUIRE(pairs == 0 || pairs == 1, CODON_ERR_BAD_ARG, "smooth_depth: pairs %d (0 or 1)", pairs);
  if (const int st = check_not_same(who, in, out)) return st;
  const bool planes_ok = (((uintptr_t)in | (uintptr_t)out) & (uintptr_t)(fl_elem_bytes(fmt) - 1)) == 0;
  const bool words_ok = (((uintptr_t)counts | (uintptr_t)weights) & 3) == 0 && ((uintptr_t)workspace & 15) == 0;
  CODON_REQUIRE(planes_ok && words_ok, CODON_ERR_BAD_ARG, "smooth_depth: unaligned plane, weights, statistics or workspace");
  if (smooth_launches(radius, passes) > 1) {
    CODON_REQUIRE(workspace, CODON_ERR_BAD_ARG, "smooth_depth: null workspace with %d launches", smooth_launches(radius, passes));
    CODON_REQUIRE(workspace != in && workspace != out, CODON_ERR_BAD_ARG, "smooth_depth: the workspace is in or out");
    if (const int st = check_workspace(who, workspace_bytes, smooth_workspace_bytes(batch, height, width))) return st;
  }
  return smooth_depth(batch, height, width, in, fmt, radius, passes, tol_abs, tol_rel_q16, pairs, weights, out, counts, workspace,
                      (hipStream_t)stream);
}

// ---- temporal filter of a fixed camera's depth sequence ------------------------------------------------------------
// the refusals a call and the chunk query share, in the order of the argument list
static int check_sequence(const char* who, int frames, int height, int width) {
  CODON_REQUIRE(frames >= 1 && frames <= TP_MAX_FRAMES, CODON_ERR_BAD_ARG, "%s: frames %d (1..%d)", who, frames, TP_MAX_FRAMES);
  if (const int st = check_side(who, height, width, "plane", TP_MAX_SIDE)) return st;
  CODON_REQUIRE((int64_t)frames * height * width < ((int64_t)1 << 31), CODON_ERR_BAD_ARG,
                "%s: a sequence of %lld codes (%d frames of %dx%d; below 2^31)", who, (long long)frames * height * width, frames, height,
                width);
  return CODON_OK;
}

static int check_window(const char* who, int back, int ahead) {
  CODON_REQUIRE(back >= 0 && ahead >= 0 && back + ahead < TP_MAX_WINDOW, CODON_ERR_BAD_ARG,
                "%s: window back %d ahead %d (each at least 0, back + ahead at most %d)", who, back, ahead, TP_MAX_WINDOW - 1);
  return CODON_OK;
}

int32_t codon_temporal_chunk_frames(int32_t frames, int32_t height, int32_t width, int32_t back, int32_t ahead) {
  const char* who = "temporal_chunk_frames";
  if (check_sequence(who, frames, height, width) || check_window(who, back, ahead)) return 0;
  return temporal_chunk_frames(frames, height, width, back, ahead);
}

int codon_temporal_depth(int32_t frames, int32_t height, int32_t width, const void* in, int32_t fmt, int32_t top, int32_t back,
                         int32_t ahead, int32_t tol_abs, int32_t tol_rel_q16, int32_t min_count, int32_t min_fill, void* out,
                         uint32_t* counts, codon_stream_t stream) {
  CODON_REQUIRE(in && out, CODON_ERR_BAD_ARG, "temporal_depth: null pointer");
  const char* who = "temporal_depth";
  if (const int st = check_sequence(who, frames, height, width)) return st;
  if (const int st = check_fmt(who, fmt)) return st;
  if (const int st = check_top(who, fmt, top)) return st;
  if (const int st = check_window(who, back, ahead)) return st;
  if (const int st = check_link_tolerances(who, tol_abs, top, tol_rel_q16, TP_MAX_REL)) return st;
  CODON_REQUIRE(min_count >= 1 && min_count <= TP_MAX_WINDOW, CODON_ERR_BAD_ARG, "temporal_depth: min_count %d (1..%d)", min_count,
                TP_MAX_WINDOW);
  CODON_REQUIRE(min_fill >= 0 && min_fill <= TP_MAX_WINDOW, CODON_ERR_BAD_ARG, "temporal_depth: min_fill %d (0..%d)", min_fill,
                TP_MAX_WINDOW);
  if (const int st = check_not_same(who, in, out)) return st;
  const bool planes_ok = (((uintptr_t)in | (uintptr_t)out) & (uintptr_t)(fl_elem_bytes(fmt) - 1)) == 0;
  CODON_REQUIRE(planes_ok && ((uintptr_t)counts & 3) == 0, CODON_ERR_BAD_ARG, "temporal_depth: unaligned plane or statistics");
  return temporal_depth(frames, height, width, in, fmt, back, ahead, tol_abs, tol_rel_q16, min_count, min_fill, out, counts,
                        (hipStream_t)stream);
}

// ---- temporal filter of a depth stream, frame by frame --------------------------------------------------------------
int32_t codon_temporal_ring_frames(void) { return TP_SLOTS; }

int codon_temporal_push(int32_t height, int32_t width, const void* in, int32_t fmt, int32_t top, int32_t back, int32_t ahead,
                        int32_t tol_abs, int32_t tol_rel_q16, int32_t min_count, int32_t min_fill, void* ring, uint32_t* state,
                        void* out, uint32_t* counts, codon_stream_t stream) {
  const char* who = "temporal_push";
  if (const int st = check_side(who, height, width, "plane", TP_MAX_SIDE)) return st;
  if (const int st = check_fmt(who, fmt)) return st;
  if (const int st = check_top(who, fmt, top)) return st;
  if (const int st = check_window(who, back, ahead)) return st;
  if (const int st = check_link_tolerances(who, tol_abs, top, tol_rel_q16, TP_MAX_REL)) return st;
  CODON_REQUIRE(min_count >= 1 && min_count <= TP_MAX_WINDOW, CODON_ERR_BAD_ARG, "temporal_push: min_count %d (1..%d)", min_count,
                TP_MAX_WINDOW);
  CODON_REQUIRE(min_fill >= 0 && min_fill <= TP_MAX_WINDOW, CODON_ERR_BAD_ARG, "temporal_push: min_fill %d (0..%d)", min_fill,
                TP_MAX_WINDOW);
  CODON_REQUIRE(ring && state && out, CODON_ERR_BAD_ARG, "temporal_push: null pointer");
  if (const int st = check_not_same(who, in, out)) return st;
  const uintptr_t plane = (uintptr_t)height * width * fl_elem_bytes(fmt), r0 = (uintptr_t)ring, r1 = r0 + TP_SLOTS * plane;
  const bool in_hit = in && (uintptr_t)in < r1 && (uintptr_t)in + plane > r0, out_hit = (uintptr_t)out < r1 && (uintptr_t)out + plane > r0;
  CODON_REQUIRE(!in_hit && !out_hit, CODON_ERR_BAD_ARG, "temporal_push: the ring overlaps %s", in_hit ? "in" : "out");
  const bool planes_ok = (((uintptr_t)in | (uintptr_t)out | r0) & (uintptr_t)(fl_elem_bytes(fmt) - 1)) == 0;
  CODON_REQUIRE(planes_ok && (((uintptr_t)state | (uintptr_t)counts) & 3) == 0, CODON_ERR_BAD_ARG,
                "temporal_push: unaligned plane, ring, state or statistics");
  return temporal_push(height, width, in, fmt, back, ahead, tol_abs, tol_rel_q16, min_count, min_fill, ring, state, out, counts,
                       (hipStream_t)stream);
}

// ---- depth maps as point clouds with normals -----------------------------------------------------------------------
size_t codon_cloud_workspace_bytes(int32_t batch, int32_t height, int32_t width) { return cloud_workspace_bytes(batch, height, width); }

int codon_cloud_points(int32_t batch, int32_t height, int32_t width, const void* codes, int32_t fmt, int32_t top, const int32_t* rx,
                       const int32_t* ry, const int32_t* ray_span, double m, int32_t normals, int32_t radius, int32_t tol_abs,
                       int32_t tol_rel_q16, const uint8_t* color, int32_t color_channels, uint8_t* body, uint32_t* counts,
                       uint8_t* normal_map, void* workspace, size_t workspace_bytes, codon_stream_t stream) {
  CODON_REQUIRE(codes && rx && ry && ray_span && body && counts && workspace, CODON_ERR_BAD_ARG, "cloud_points: null pointer");
  const char* who = "cloud_points";
  if (const int st = check_planes(who, fmt, batch, height, width, CD_MAX_SIDE, top)) return st;
  CODON_REQUIRE(normals == 0 || normals == 1, CODON_ERR_BAD_ARG, "cloud_points: normals %d (0 or 1)", normals);
  CODON_REQUIRE(radius >= 1 && radius <= CD_MAX_RADIUS, CODON_ERR_BAD_ARG, "cloud_points: radius %d (1..%d)", radius, CD_MAX_RADIUS);
  if (const int st = check_link_tolerances(who, tol_abs, top, tol_rel_q16, CD_MAX_REL)) return st;
  for (int q = 0; q < 4; ++q)
    CODON_REQUIRE(ray_span[q] > -CD_RAY_LIMIT && ray_span[q] < CD_RAY_LIMIT, CODON_ERR_BAD_ARG,
                  "cloud_points: ray %d of the span is %d (Q20, below 2^22 in magnitude)", q, ray_span[q]);
  CODON_REQUIRE(m > 0.0 && isfinite(m), CODON_ERR_BAD_ARG, "cloud_points: m %g (metres per Q20 code: positive and finite)", m);
  CODON_REQUIRE(color ? color_channels == 1 || color_channels == 3 : color_channels == 0, CODON_ERR_BAD_ARG,
                "cloud_points: color_channels %d (1: grey, 3: RGB; 0 without colour)", color_channels);
  CODON_REQUIRE(!normal_map || normals, CODON_ERR_BAD_ARG, "cloud_points: a normal map without normals");
  const bool planes_ok = ((uintptr_t)codes & (uintptr_t)(fl_elem_bytes(fmt) - 1)) == 0;
  const bool words_ok = (((uintptr_t)rx | (uintptr_t)ry | (uintptr_t)counts) & 3) == 0 && ((uintptr_t)workspace & 15) == 0;
  CODON_REQUIRE(planes_ok && words_ok, CODON_ERR_BAD_ARG, "cloud_points: unaligned plane, table, counts or workspace");
  if (const int st = check_workspace(who, workspace_bytes, cloud_workspace_bytes(batch, height, width))) return st;
  return cloud_points(batch, height, width, codes, fmt, rx, ry, m, normals ? radius : 0, tol_abs, tol_rel_q16, color, color_channels,
                      body, counts, normal_map, workspace, (hipStream_t)stream);
}

// ---- depth maps as triangle meshes ----------------------------------------------------------------------------------
size_t codon_cloud_mesh_workspace_bytes(int32_t batch, int32_t height, int32_t width) {
  return cloud_mesh_workspace_bytes(batch, height, width);
}

int codon_cloud_mesh(int32_t batch, int32_t height, int32_t width, const void* codes, int32_t fmt, int32_t top, int32_t tol_abs,
                     int32_t tol_rel_q16, uint8_t* faces, uint32_t* counts, void* workspace, size_t workspace_bytes,
                     codon_stream_t stream) {
  // a plane without a quad has no face: its `faces` holds no byte and may be NULL
  CODON_REQUIRE(codes && counts && workspace && (faces || height == 1 || width == 1), CODON_ERR_BAD_ARG, "cloud_mesh: null pointer");
  const char* who = "cloud_mesh";
  if (const int st = check_planes(who, fmt, batch, height, width, MS_MAX_SIDE, top)) return st;
  if (const int st = check_link_tolerances(who, tol_abs, top, tol_rel_q16, MS_MAX_REL)) return st;
  const bool planes_ok = ((uintptr_t)codes & (uintptr_t)(fl_elem_bytes(fmt) - 1)) == 0;
  const bool words_ok = ((uintptr_t)counts & 3) == 0 && ((uintptr_t)workspace & 15) == 0;
  CODON_REQUIRE(planes_ok && words_ok, CODON_ERR_BAD_ARG, "cloud_mesh: unaligned plane, counts or workspace");
  if (const int st = check_workspace(who, workspace_bytes, cloud_mesh_workspace_bytes(batch, height, width))) return st;
  return cloud_mesh(batch, height, width, codes, fmt, tol_abs, tol_rel_q16, faces, counts, workspace, (hipStream_t)stream);
}

// ---- undistortion of colour images ---------------------------------------------------------------------------------
size_t codon_undistort_tiles_bytes(int32_t out_height, int32_t out_width) { return undistort_tiles_bytes(out_height, out_width); }

int codon_undistort_plan(int32_t src_height, int32_t src_width, int32_t out_height, int32_t out_width, const int32_t* map_host,
                         int32_t* tiles_host, uint32_t* counts_host) {
  CODON_REQUIRE(map_host && tiles_host && counts_host, CODON_ERR_BAD_ARG, "undistort_plan: null pointer");
  CODON_REQUIRE(src_height >= 1 && src_height <= UD_MAX_SIDE && src_width >= 1 && src_width <= UD_MAX_SIDE, CODON_ERR_BAD_ARG,
                "undistort_plan: a %dx%d source (1..%d each way)", src_height, src_width, UD_MAX_SIDE);
  CODON_REQUIRE(out_height >= 1 && out_height <= UD_MAX_SIDE && out_width >= 1 && out_width <= UD_MAX_SIDE, CODON_ERR_BAD_ARG,
                "undistort_plan: a %dx%d target (1..%d each way)", out_height, out_width, UD_MAX_SIDE);
  const long bad = undistort_plan(src_height, src_width, out_height, out_width, map_host, tiles_host, counts_host);
  CODON_REQUIRE(bad < 0, CODON_ERR_BAD_ARG,
                "undistort_plan: map entry (%ld, %ld) is (%d, %d): neither the outside pair nor a Q5 position in the %dx%d source "
                "(-16 <= U < 32 width - 16, V likewise)", bad / out_width, bad % out_width, map_host[2 * bad], map_host[2 * bad + 1],
                src_height, src_width);
  return CODON_OK;
}

int codon_undistort(int32_t batch, int32_t src_height, int32_t src_width, int32_t channels, const uint8_t* in, int32_t out_height,
                    int32_t out_width, const int32_t* map, const int32_t* tiles, const int16_t* weights, uint8_t* out,
                    codon_stream_t stream) {
  CODON_REQUIRE(in && out && map && tiles && weights, CODON_ERR_BAD_ARG, "undistort: null pointer");
  CODON_REQUIRE(batch >= 1 && batch <= 65535, CODON_ERR_BAD_ARG, "undistort: batch %d (1..65535)", batch);
  CODON_REQUIRE(src_height >= 1 && src_height <= UD_MAX_SIDE && src_width >= 1 && src_width <= UD_MAX_SIDE, CODON_ERR_BAD_ARG,
                "undistort: a %dx%d source (1..%d each way)", src_height, src_width, UD_MAX_SIDE);
  CODON_REQUIRE(out_height >= 1 && out_height <= UD_MAX_SIDE && out_width >= 1 && out_width <= UD_MAX_SIDE, CODON_ERR_BAD_ARG,
                "undistort: a %dx%d target (1..%d each way)", out_height, out_width, UD_MAX_SIDE);
  CODON_REQUIRE(channels == 1 || channels == 3, CODON_ERR_BAD_ARG, "undistort: channels %d (1: grey, 3: RGB)", channels);
  CODON_REQUIRE(in != out, CODON_ERR_BAD_ARG, "undistort: in and out are the same buffer");
  CODON_REQUIRE(((uintptr_t)map & 7) == 0 && ((uintptr_t)tiles & 15) == 0 && ((uintptr_t)weights & 1) == 0, CODON_ERR_BAD_ARG,
                "undistort: unaligned table (map: 8 bytes, tiles: 16, weights: 2)");
  return undistort(batch, src_height, src_width, channels, in, out_height, out_width, map, tiles, weights, out,
                   (hipStream_t)stream);
}

// ---- per-image range normalisation of depth codes ---------------------------------------------------------------
int codon_code_range(int32_t batch, int32_t height, int32_t width, const void* codes, int32_t code_bits, int32_t* lo_hi,
                     codon_stream_t stream) {
  CODON_REQUIRE(codes && lo_hi, CODON_ERR_BAD_ARG, "code_range: null pointer");
  if (const int st = check_code_bits("code_range", code_bits)) return st;
  if (const int st = check_batch("code_range", batch)) return st;
  if (const int st = check_side("code_range", height, width, "plane", ST_MAX_SIDE)) return st;
  CODON_REQUIRE(((uintptr_t)codes & (uintptr_t)(code_bits / 8 - 1)) == 0 && ((uintptr_t)lo_hi & 3) == 0, CODON_ERR_BAD_ARG,
                "code_range: unaligned plane or range");
  return code_range(batch, (long)height * width, codes, code_bits == 8 ? ST_U8 : ST_U16, lo_hi, (hipStream_t)stream);
}

static int map_codes_checked(const char* who, int dir, int32_t batch, int32_t height, int32_t width, const void* in,
                             int32_t code_bits, int32_t top, const int32_t* lo_hi, void* out, codon_stream_t stream) {
  CODON_REQUIRE(in && lo_hi && out, CODON_ERR_BAD_ARG, "%s: null pointer", who);
  if (const int st = check_code_bits(who, code_bits)) return st;
  if (const int st = check_batch(who, batch)) return st;
  if (const int st = check_side(who, height, width, "plane", ST_MAX_SIDE)) return st;
  CODON_REQUIRE(code_bits == 16 ? (top >= 2 && top <= 65535) : top == 255, CODON_ERR_BAD_ARG,
                "%s: top %d (255 for 8-bit codes, 2..65535 for 16-bit codes)", who, top);
  CODON_REQUIRE((((uintptr_t)in | (uintptr_t)out) & (uintptr_t)(code_bits / 8 - 1)) == 0 && ((uintptr_t)lo_hi & 3) == 0,
                CODON_ERR_BAD_ARG, "%s: unaligned plane or range", who);
  return map_codes(dir, batch, (long)height * width, in, code_bits == 8 ? ST_U8 : ST_U16, top, lo_hi, out, (hipStream_t)stream);
}

int codon_stretch_codes(int32_t batch, int32_t height, int32_t width, const void* in, int32_t code_bits, int32_t top,
                        const int32_t* lo_hi, void* out, codon_stream_t stream) {
  return map_codes_checked("stretch_codes", ST_STRETCH, batch, height, width, in, code_bits, top, lo_hi, out, stream);
}

int codon_unstretch_codes(int32_t batch, int32_t height, int32_t width, const void* in, int32_t code_bits, int32_t top,
                          const int32_t* lo_hi, void* out, codon_stream_t stream) {
  return map_codes_checked("unstretch_codes", ST_UNSTRETCH, batch, height, width, in, code_bits, top, lo_hi, out, stream);
}

size_t codon_weight_checksum_workspace_bytes(void) { return weight_checksum_workspace_bytes(); }

int codon_weight_checksum(const codon_wsum_desc* desc, void* ws, uint64_t* ref, int32_t mode, int32_t* flag,
                          codon_stream_t stream) {
  return codon_weight_checksum_clear(desc, ws, ref, mode, flag, nullptr, 0, stream);
}

int codon_weight_checksum_clear(const codon_wsum_desc* desc, void* ws, uint64_t* ref, int32_t mode, int32_t* flag,
                                int32_t* clear, int32_t nclear, codon_stream_t stream) {
  CODON_REQUIRE(desc && ws && ref && flag, CODON_ERR_BAD_ARG, "weight_checksum: null pointer");
  CODON_REQUIRE(nclear >= 0 && (clear || nclear == 0), CODON_ERR_BAD_ARG, "weight_checksum: %d words to clear at a null pointer", nclear);
  CODON_REQUIRE(desc->n > 0 && desc->n <= CODON_WSUM_MAX && (mode == 0 || mode == 1), CODON_ERR_BAD_ARG,
                "weight_checksum: n %d (1..%d), mode %d (0, 1)", desc->n, CODON_WSUM_MAX, mode);
  uint64_t total = 0;
  for (int t = 0; t < desc->n; ++t) {
    CODON_REQUIRE(desc->data[t] && desc->bytes[t] % 16 == 0 && ((uintptr_t)desc->data[t] & 15) == 0, CODON_ERR_BAD_ARG,
                  "weight_checksum: tensor %d must be 16-byte aligned with a multiple of 16 bytes", t);
    total += desc->bytes[t];
  }
  CODON_REQUIRE(total / 16 < (1ull << 32), CODON_ERR_UNSUPPORTED, "weight_checksum: more than 64 GiB of weights");
  return weight_checksum(desc, ws, (unsigned long long*)ref, mode, flag, clear, nclear, (hipStream_t)stream);
}

}  // extern "C"
