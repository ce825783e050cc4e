// The training pool's record format, written once for the crop kernels (train_data.hip, resample_masked.hip)
// and the descriptor validator (codon_abi.hip); codon_amd/train.py's record_layout is its mirror on the host.
#pragma once
#include "codon_common.h"

namespace codon {

// A batch's descriptors, passed by value as a kernel argument; the other arguments of a crop kernel take up to 96 bytes.
struct CropArgs {
  codon_crop_sample s[CODON_TRAIN_MAX_BATCH];
};
static_assert(sizeof(CropArgs) + 96 <= CODON_KERNARG_LIMIT, "passed by value as a kernel argument");

inline CropArgs pack_crop_args(const codon_crop_desc* d) {
  CropArgs a;
  for (int b = 0; b < d->n; ++b) a.s[b] = d->s[b];
  for (int b = d->n; b < CODON_TRAIN_MAX_BATCH; ++b) a.s[b] = codon_crop_sample{};
  return a;
}

// Byte offsets of a record's planes from its start, and the bytes it holds.  The depth plane (H*W codes of `bits` bits)
// comes first; a record has a label plane (H*W codes) or a low-resolution plane ((H/s)*(W/s) codes), never both, and
// either starts at byte 2*H*W; the guidance is always H*W u8:
//    8-bit: depth | guide | label or lr           16-bit: depth16 | label16 or lr16 | guide
// Little-endian u16 planes start at even bytes: a 16-bit record starts at an even offset, and the pool pads one of odd
// size by a byte that `size` does not count.
struct RecordLayout {
  long depth, guide, label, lr, size;
};

__host__ __device__ inline RecordLayout record_layout(int bits, bool label, int lr_scale, int H, int W) {
  const long hw = (long)H * W;
  const long extra = (label ? hw : 0) + (lr_scale ? (long)(H / lr_scale) * (W / lr_scale) : 0);
  if (bits == 16) return {0, 2 * hw + 2 * extra, 2 * hw, 2 * hw, 3 * hw + 2 * extra};
  return {0, hw, 2 * hw, 2 * hw, 2 * hw + extra};
}

// Code `px` of the plane at `plane`: a u8, or a u16 at an even address.
template <int BITS>
__device__ __forceinline__ int record_code(const unsigned char* plane, long px) {
  if (BITS == 16) return reinterpret_cast<const unsigned short*>(plane)[px];
  return plane[px];
}

// Output pixel idx = i*P + j of sample blockIdx.y's crop -> its source pixel (gy, gx) in the (H, W) image, through the
// D4 op (numpy: c = img[y0:y0+P, x0:x0+P]; op&1: c = c.T; op&2: c = c[::-1]; op&4: c = c[:, ::-1]), and where it goes in
// the (n,1,P,P) outputs.
struct CropPixel {
  int gy, gx;
  long out;
};

__device__ __forceinline__ CropPixel crop_pixel(int idx, const codon_crop_sample& d, int P) {
  const int i = idx / P, j = idx - i * P;
  int si = i, sj = j;
  if (d.op & 4) sj = P - 1 - sj;
  if (d.op & 2) si = P - 1 - si;
  if (d.op & 1) { const int t = si; si = sj; sj = t; }
  return {d.y0 + si, d.x0 + sj, (long)blockIdx.y * P * P + idx};
}

}  // namespace codon
