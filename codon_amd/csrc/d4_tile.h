// The two workgroup bodies of the D4 self-ensemble kernels (d4.hip; wg_d4_*, over wg.h's group type: DESIGN 12.13)
// and the per-thread phases they run, written so that the SAME text compiles for the device and for a plain host compiler: the
// kernels and tools/d4_host_check.cpp, under the address and undefined-behaviour sanitizers, call the same bodies.  A workgroup
// of D4_THREADS threads owns one D4_TILE x D4_TILE tile of the (H, W) plane; each kernel is two phases with a workgroup barrier
// between them, and the tile in LDS is what turns the transposed views' column walk into row walks on both sides of the copy.
//
// The D4 code is train_record.h's (crop_pixel), on the whole plane c (H, W):  op&1: c = c.T; then op&2: c = c[::-1]; then op&4: c = c[:, ::-1].
// Codes 0, 2, 4, 6 ("upright", H x W) sit at slot s = op >> 1 of the upright batch, codes 1, 3, 5, 7 ("transposed", W x H) at
// slot s of the transposed batch; in both  fr = s & 1  flips rows and  fc = s & 2  flips columns:
//   upright    view s:  v[i][j] = c[fr ? H-1-i : i][fc ? W-1-j : j]
//   transposed view s:  v[a][b] = c[fc ? H-1-b : b][fr ? W-1-a : a]            (a < W, b < H)
// and, the flips being involutions, the inverse of a network output o of that view is
//   upright    : u[i][j] = o[fr ? H-1-i : i][fc ? W-1-j : j]
//   transposed : u[i][j] = o[fr ? W-1-j : j][fc ? H-1-i : i]
#pragma once

#include "wg.h"

#if defined(__HIPCC__)
#define CODON_D4_HD __host__ __device__ __forceinline__
#else
#define CODON_D4_HD inline
#endif

namespace codon {

constexpr int D4_TILE = 32;
constexpr int D4_THREADS = 256;
constexpr int D4_ROWS = D4_THREADS / D4_TILE;       // tile rows per pass of the workgroup

CODON_D4_HD int d4_tiles(int n) { return (n + D4_TILE - 1) / D4_TILE; }      // both grids are (d4_tiles(W), d4_tiles(H), .)

// LDS row stride in elements: an ODD number of dwords (33 for 4-byte, 17 for 2-byte elements), so that the 32 lanes that
// read one tile COLUMN land on 32 different banks
template <typename T>
struct D4Stride {
  static constexpr int value = D4_TILE + 4 / (int)sizeof(T);
};

// ---- views: bit copies ---------------------------------------------------------------------------------------------------
// src: this image's (H, W) plane; up / tp: this image's four upright / transposed views, hw elements apart.

// phase 1: the thread's tile elements, read along the row, go to LDS and to the four upright views (rows of W, walked
// forwards or backwards: contiguous either way)
template <typename T>
CODON_D4_HD void d4_views_phase1(int tid, int i0, int j0, int H, int W, const T* src, T* up, T (*tile)[D4Stride<T>::value]) {
  const int tx = tid % D4_TILE, ty = tid / D4_TILE;
  const long hw = (long)H * W;
  const int j = j0 + tx;
  for (int r = ty; r < D4_TILE; r += D4_ROWS) {
    const int i = i0 + r;
    if (i < H && j < W) {
      const T v = src[(long)i * W + j];
      tile[r][tx] = v;
      const int ri = H - 1 - i, rj = W - 1 - j;
      up[(long)i * W + j] = v;                        // code 0
      up[hw + (long)ri * W + j] = v;                  // code 2: rows flipped
      up[2 * hw + (long)i * W + rj] = v;              // code 4: columns flipped
      up[3 * hw + (long)ri * W + rj] = v;             // code 6: both
    }
  }
}

// phase 2 (after the barrier): the tile read by COLUMN -- thread (tx, r) takes c[i0 + tx][j0 + r] -- goes to the four
// transposed views, whose rows of H are walked by tx
template <typename T>
CODON_D4_HD void d4_views_phase2(int tid, int i0, int j0, int H, int W, T* tp, const T (*tile)[D4Stride<T>::value]) {
  const int tx = tid % D4_TILE, ty = tid / D4_TILE;
  const long hw = (long)H * W;
  const int b = i0 + tx;                              // column of the transposed plane = row of the source
  for (int r = ty; r < D4_TILE; r += D4_ROWS) {
    const int a = j0 + r;                             // row of the transposed plane = column of the source
    if (a < W && b < H) {
      const T v = tile[tx][r];
      const int ra = W - 1 - a, rb = H - 1 - b;
      tp[(long)a * H + b] = v;                        // code 1
      tp[hw + (long)ra * H + b] = v;                  // code 3: rows flipped
      tp[2 * hw + (long)a * H + rb] = v;              // code 5: columns flipped
      tp[3 * hw + (long)ra * H + rb] = v;             // code 7: both
    }
  }
}

// ---- merge: the mean of the eight inverses, fp32 ---------------------------------------------------------------------------
// DT is a codon_dtype: 0 fp32, 1 bf16, 2 fp16.  The upcast is exact.
template <int DT>
CODON_D4_HD float d4_load_f32(const void* p, long idx) {
  if (DT == 0) return static_cast<const float*>(p)[idx];
  const unsigned short h = static_cast<const unsigned short*>(p)[idx];
  if (DT == 1) return __builtin_bit_cast(float, (unsigned)h << 16);
  return (float)__builtin_bit_cast(_Float16, h);
}

// phase 1: the four transposed outputs' part of this tile, read along THEIR rows (tx walks i, the source row), into LDS as
// lds[s][j - j0][i - i0];  tr: this image's four (W, H) outputs, hw elements apart
template <int DT>
CODON_D4_HD void d4_merge_phase1(int tid, int i0, int j0, int H, int W, const void* tr, long tr_base,
                                 float (*lds)[D4_TILE][D4_TILE + 1]) {
  const int tx = tid % D4_TILE, ty = tid / D4_TILE;
  const long hw = (long)H * W;
  const int i = i0 + tx;
  for (int r = ty; r < D4_TILE; r += D4_ROWS) {
    const int j = j0 + r;
    if (i < H && j < W) {
      const int rj = W - 1 - j, ri = H - 1 - i;
      lds[0][r][tx] = d4_load_f32<DT>(tr, tr_base + (long)j * H + i);                 // code 1
      lds[1][r][tx] = d4_load_f32<DT>(tr, tr_base + hw + (long)rj * H + i);           // code 3
      lds[2][r][tx] = d4_load_f32<DT>(tr, tr_base + 2 * hw + (long)j * H + ri);       // code 5
      lds[3][r][tx] = d4_load_f32<DT>(tr, tr_base + 3 * hw + (long)rj * H + ri);      // code 7
    }
  }
}

// phase 2 (after the barrier): out[i][j] = 0.125f * (((u0+u1)+(u2+u3)) + ((u4+u5)+(u6+u7))), every add rounded on its own
// (the including file switches contraction off); the even codes straight from the upright outputs, the odd ones from LDS
template <int DT>
CODON_D4_HD void d4_merge_phase2(int tid, int i0, int j0, int H, int W, const void* upr, long up_base,
                                 const float (*lds)[D4_TILE][D4_TILE + 1], float* out) {
  const int tx = tid % D4_TILE, ty = tid / D4_TILE;
  const long hw = (long)H * W;
  const int j = j0 + tx;
  for (int r = ty; r < D4_TILE; r += D4_ROWS) {
    const int i = i0 + r;
    if (i < H && j < W) {
      const int ri = H - 1 - i, rj = W - 1 - j;
      const float u0 = d4_load_f32<DT>(upr, up_base + (long)i * W + j);
      const float u2 = d4_load_f32<DT>(upr, up_base + hw + (long)ri * W + j);
      const float u4 = d4_load_f32<DT>(upr, up_base + 2 * hw + (long)i * W + rj);
      const float u6 = d4_load_f32<DT>(upr, up_base + 3 * hw + (long)ri * W + rj);
      const float u1 = lds[0][tx][r], u3 = lds[1][tx][r], u5 = lds[2][tx][r], u7 = lds[3][tx][r];
      const float a = (u0 + u1) + (u2 + u3);
      const float b = (u4 + u5) + (u6 + u7);
      out[(long)i * W + j] = 0.125f * (a + b);
    }
  }
}

// ---- the workgroup bodies -----------------------------------------------------------------------------------------------------

// workgroup (bx, by, bz) of grid (d4_tiles(W), d4_tiles(H), B * planes): plane p of image b = bz.  LDS: tile
template <typename T, class G>
CODON_D4_HD void wg_d4_views(G wg, int bx, int by, unsigned bz, const T* src0, const T* src1, T* up0, T* tp0, T* up1, T* tp1, int H,
                             int W, int planes, T (*tile)[D4Stride<T>::value]) {
  const int b = bz / planes, p = bz - b * planes;                      // uniform (bz is unsigned: no signed division)
  const long hw = (long)H * W;
  const T* src = (p ? src1 : src0) + b * hw;
  T* up = (p ? up1 : up0) + 4 * b * hw;
  T* tp = (p ? tp1 : tp0) + 4 * b * hw;
  const int i0 = by * D4_TILE, j0 = bx * D4_TILE;
  WG_EACH(wg, tid) d4_views_phase1<T>(tid, i0, j0, H, W, src, up, tile);
  wg.sync();
  WG_EACH(wg, tid) d4_views_phase2<T>(tid, i0, j0, H, W, tp, tile);
}

// workgroup (bx, by, bz) of grid (d4_tiles(W), d4_tiles(H), B): image bz.  LDS: lds
template <int DT, class G>
CODON_D4_HD void wg_d4_merge(G wg, int bx, int by, unsigned bz, const void* upright, const void* transposed, float* out, int H, int W,
                             float (*lds)[D4_TILE][D4_TILE + 1]) {
  const long hw = (long)H * W;
  const long base = 4 * (long)bz * hw;
  const int i0 = by * D4_TILE, j0 = bx * D4_TILE;
  WG_EACH(wg, tid) d4_merge_phase1<DT>(tid, i0, j0, H, W, transposed, base, lds);
  wg.sync();
  WG_EACH(wg, tid) d4_merge_phase2<DT>(tid, i0, j0, H, W, upright, base, lds, out + (long)bz * hw);
}

}  // namespace codon
