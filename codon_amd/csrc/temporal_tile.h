// The temporal filter of a fixed camera's depth sequence (temporal.hip): its workgroup body (wg_temporal, over
// wg.h's group type: DESIGN 12.13) and the per-thread phases it runs, written like clean_tile.h so that the SAME text compiles for
// the device and for a plain host compiler: the kernel and tools/temporal_host_check.cpp, under the address and undefined-behaviour
// sanitizers, call the same body.  Integers only.
//
// The definition (tests/temporal_ref.py): c is T frames of h x w codes, 0 a hole.  The window of frame t is the frames
// s in [max(0, t - Bk), min(T - 1, t + Ah)], n_w of them, at most TP_MAX_WINDOW.  The link rule is clean's (cl_linked, clean_tile.h:
// the one text).  Per pixel and frame, v = c_t(p), every read of c:
//   1. v != 0: Lk = the window samples linked to v (v among them), n = |Lk|.  n >= min(M, n_w): out = (2 sum Lk + n) / (2 n).
//      Otherwise the pixel is REJECTED and goes on with 2.
//   2. v == 0 or rejected: F == 0: out = 0.  Otherwise S = the non-zero window samples, k = |S|; k < F: out = 0; else m = the lower
//      median of S (rank (k - 1) >> 1), Lm = the samples linked to m, out = the same rounded mean of Lm if |Lm| >= F, else 0.
// Statistics per frame, four u32: valid inputs, rejected pixels, non-zero outputs where the input was 0 or rejected, accepted
// pixels whose output differs from the input.
//
// One launch of wg_temporal over a grid (pixel groups, time chunks); wg_clean_zero before it zeroes the statistics.  A thread owns
// TP_PER consecutive pixels of the plane through the frames [t0, t1) of its chunk.  The last frames it has read stand in an LDS ring
// laid out [slot][thread], a 64-bit word of four u16 codes each: TP_SLOTS = 16 slots, frame s in slot s & 15, so the at most 15
// frames of a window and the frame read ahead never share one.  A thread reads and writes its own column alone: no barrier guards
// the ring, and 64 lanes x 8 bytes of one slot are 512 contiguous bytes, free of bank conflicts for 8-byte reads.  Every frame is
// read from memory once per chunk (the chunk's seams re-read Bk + Ah frames) and every output written once.  A step first issues
// the load of frame t + Ah + 1, then gathers the window from the ring into CAP 64-bit registers by a STATIC index (the slot is the
// dynamic one; a sample beyond the window is 0, a hole, which neither links nor counts), works on registers alone, stores the
// frame, and only then puts the frame read ahead into its slot: the load has the whole step to arrive.  CAP is the smallest of
// 3, 5, 9, 15 that holds Bk + Ah + 1 (temporal_cap, launch_rules.h), a template argument so that every loop over the window unrolls.
// The median's rank is counted: rank_i = #{j < i: y_j <= y_i} + #{j > i: y_j < y_i} with a hole's key above every code, one
// comparison per pair; the ranks are a permutation, so exactly one sample has rank (k - 1) >> 1.  Only holes and rejected pixels
// take that branch.
#pragma once

#include "clean_tile.h"

namespace codon {

constexpr int TP_THREADS = CL_THREADS;                               // 256: cl_sum32 and cl_sum_add are clean's
constexpr int TP_PER = 4, TP_TILE = TP_THREADS * TP_PER;             // four consecutive pixels per thread: 8 bytes of u16, 4 of u8
constexpr int TP_SLOTS = 16;                                         // ring slots: a power of two above TP_MAX_WINDOW
constexpr int TP_MAX_WINDOW = 15, TP_MAX_FRAMES = 4096, TP_MAX_SIDE = FL_MAX_SIDE, TP_MAX_REL = CL_MAX_REL;
constexpr int TP_VALID = 0, TP_REJECTED = 1, TP_FILLED = 2, TP_CHANGED = 3, TP_STATS = 4;
typedef unsigned long long tp_quad;                                  // four u16 codes, pixel q at bits 16 q

struct TpArgs {
  int T, h, w, back, ahead;
  unsigned tol_abs, tol_rel;       // A, and Rq = rint(65536 rel)
  int min_count, min_fill;         // M, F
  int chunk;                       // frames per time chunk (temporal_chunk_frames, launch_rules.h)
  int vec;                         // h w is a multiple of TP_PER and both planes stand on a multiple of TP_PER elements
};

CODON_FL_HD unsigned tp_code(tp_quad word, int q) { return (unsigned)(word >> (16 * q)) & 0xFFFFu; }

// the codes of pixels at .. at + 3 of `in` (an element index over all frames), `left` of them inside the plane, the rest 0
template <int FMT>
CODON_FL_HD tp_quad tp_load4(const void* in, long at, long left, int vec) {
  tp_quad word = 0;
  if (vec) {
    if (FMT == FL_U16) {
      __builtin_memcpy(&word, __builtin_assume_aligned((const unsigned short*)in + at, 8), 8);
    } else {
      unsigned b;
      __builtin_memcpy(&b, __builtin_assume_aligned((const unsigned char*)in + at, 4), 4);
      word = (tp_quad)(b & 0xFFu) | (tp_quad)(b >> 8 & 0xFFu) << 16 | (tp_quad)(b >> 16 & 0xFFu) << 32 | (tp_quad)(b >> 24) << 48;
    }
    return word;
  }
  for (int q = 0; q < TP_PER; ++q)
    if (q < left) word |= (tp_quad)(unsigned)fl_load<FMT>(in, at + q, 0) << (16 * q);
  return word;
}

template <int FMT>
CODON_FL_HD void tp_store4(void* out, long at, long left, tp_quad word, int vec) {
  if (vec) {
    if (FMT == FL_U16) {
      __builtin_memcpy(__builtin_assume_aligned((unsigned short*)out + at, 8), &word, 8);
    } else {
      const unsigned b = tp_code(word, 0) | tp_code(word, 1) << 8 | tp_code(word, 2) << 16 | tp_code(word, 3) << 24;
      __builtin_memcpy(__builtin_assume_aligned((unsigned char*)out + at, 4), &b, 4);
    }
    return;
  }
  for (int q = 0; q < TP_PER; ++q)
    if (q < left) fl_store<FMT>(out, at + q, (int)tp_code(word, q), nullptr);
}

// the mean of n >= 1 codes of sum `sum`, half rounded up: 2 * 15 * 65535 + 15 < 2^21
CODON_FL_HD unsigned tp_mean(unsigned sum, unsigned n) { return (2u * sum + n) / (2u * n); }

// step 2 for pixel q of the window: the rounded mean of the samples linked to the lower median of the non-zero ones, or 0
template <int CAP>
CODON_FL_HD unsigned tp_fill(const tp_quad* wnd, int q, const TpArgs& a) {
  unsigned y[CAP];
  int rank[CAP];
  int k = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < CAP; ++i) {
    const unsigned x = tp_code(wnd[i], q);
    k += x != 0u;
    y[i] = x != 0u ? x : 0xFFFFFFFFu;              // a hole: above every code, so it ranks behind the k samples
    rank[i] = i;                                   // the j < i, each taken off again where y_j > y_i
  }
  if (k < a.min_fill) return 0u;                   // min_fill >= 1 here: k >= 1
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < CAP; ++i) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = i + 1; j < CAP; ++j) {
      const int c = y[j] < y[i];
      rank[i] += c;
      rank[j] -= c;
    }
  }
  const int r = (k - 1) >> 1;
  const unsigned rel = a.tol_rel & 0xFFFFu;        // as in tp_step
  unsigned m = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < CAP; ++i) m = rank[i] == r ? y[i] : m;
  unsigned n = 0, sum = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < CAP; ++i) {
    const unsigned x = tp_code(wnd[i], q);
    const bool l = cl_linked(m & 0xFFFFu, x, a.tol_abs, rel);     // m is a sample (r < k): the mask says so to the compiler
    n += l;
    sum += l ? x : 0u;
  }
  return n >= (unsigned)a.min_fill ? tp_mean(sum, n) : 0u;
}

// steps 1 and 2 for a thread's four pixels -- THE one text of the arithmetic, for the sequence body (tp_step) and the stream body
// (tp_push_step): wnd the window's samples (a register beyond its nw frames is 0), cur the frame's own -> the four outputs; the
// packed counts (valid | rejected << 16, filled | changed << 16) are added to first and second
template <int CAP>
CODON_FL_HD tp_quad tp_filter4(const tp_quad* wnd, tp_quad cur, int nw, const TpArgs& a, unsigned& first, unsigned& second) {
  const unsigned need = (unsigned)(a.min_count < nw ? a.min_count : nw);
  // Rq <= 65535 (the entry refuses more) and a code is 16 bits: with both masks in sight the product of tau is the 24-bit
  // multiply, a full-rate instruction, where the 32-bit one runs at a quarter of it
  const unsigned rel = a.tol_rel & 0xFFFFu;
  tp_quad res = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int q = 0; q < TP_PER; ++q) {
    const unsigned v = tp_code(cur, q);
    unsigned n = 0, sum = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < CAP; ++i) {
      const unsigned x = tp_code(wnd[i], q);
      const bool l = cl_linked(v, x, a.tol_abs, rel);
      n += l;
      sum += l ? x : 0u;
    }
    const bool rejected = v != 0u && n < need, kept = v != 0u && !rejected;
    unsigned o = 0;
    if (kept) o = tp_mean(sum, n);
    else if (a.min_fill > 0) o = tp_fill<CAP>(wnd, q, a);
    res |= (tp_quad)o << (16 * q);
    first += (v != 0u) + ((unsigned)rejected << 16);
    second += (!kept && o != 0u) + ((unsigned)(kept && o != v) << 16);
  }
  return res;
}

// one thread's four pixels of frame t, group gx of the plane: the window from the ring, the frame to `out`, the frame read ahead
// (up to frame `last` of this chunk) into its slot; its packed counts (valid | rejected << 16, filled | changed << 16) into
// cnt[tid] and cnt[TP_THREADS + tid] where cnt is given
template <int FMT, int CAP>
CODON_FL_HD void tp_step(int tid, long gx, int t, int last, const void* in, const TpArgs& a, void* out, tp_quad* ring, unsigned* cnt) {
  const long hw = (long)a.h * a.w, p = (gx * TP_THREADS + tid) * TP_PER;
  unsigned first = 0, second = 0;
  if (p < hw) {
    const int lo = t - a.back > 0 ? t - a.back : 0, hi = t + a.ahead < a.T - 1 ? t + a.ahead : a.T - 1, nw = hi - lo + 1;
    const int nxt = t + a.ahead + 1;
    tp_quad pre = 0;
    if (nxt <= last) pre = tp_load4<FMT>(in, (long)nxt * hw + p, hw - p, a.vec);
    tp_quad wnd[CAP];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < CAP; ++i) wnd[i] = i < nw ? ring[((lo + i) & (TP_SLOTS - 1)) * TP_THREADS + tid] : (tp_quad)0;
    const tp_quad cur = ring[(t & (TP_SLOTS - 1)) * TP_THREADS + tid];
    const tp_quad res = tp_filter4<CAP>(wnd, cur, nw, a, first, second);
    tp_store4<FMT>(out, (long)t * hw + p, hw - p, res, a.vec);
    if (nxt <= last) ring[(nxt & (TP_SLOTS - 1)) * TP_THREADS + tid] = pre;
  }
  if (cnt) {
    cnt[tid] = first;
    cnt[TP_THREADS + tid] = second;
  }
}

// workgroup (gx, chunk) of grid (ceil(h w / TP_TILE), ceil(T / a.chunk)).  LDS: ring TP_SLOTS * TP_THREADS 64-bit words; cnt
// 2 TP_THREADS words and part 32, read with statistics alone.  stats (may be null): (T, 4) words an earlier launch zeroed; every
// frame's four sums go through LDS, one atomic add per count that is not 0.  The barriers stand in the loop over the frames, which
// every thread of the workgroup walks alike.
template <int FMT, int CAP, class G>
CODON_FL_HD void wg_temporal(G wg, long gx, int chunk, const void* in, const TpArgs& a, void* out, unsigned* stats, tp_quad* ring,
                             unsigned* cnt, unsigned* part) {
  const long hw = (long)a.h * a.w;
  const int t0 = chunk * a.chunk, t1 = t0 + a.chunk < a.T ? t0 + a.chunk : a.T;
  const int first = t0 - a.back > 0 ? t0 - a.back : 0, last = t1 - 1 + a.ahead < a.T - 1 ? t1 - 1 + a.ahead : a.T - 1;
  const int ready = t0 + a.ahead < last ? t0 + a.ahead : last;       // the frames of the first window
  WG_EACH(wg, tid) {
    const long p = (gx * TP_THREADS + tid) * TP_PER;
    if (p < hw)
      for (int s = first; s <= ready; ++s) ring[(s & (TP_SLOTS - 1)) * TP_THREADS + tid] = tp_load4<FMT>(in, (long)s * hw + p, hw - p, a.vec);
  }
  for (int t = t0; t < t1; ++t) {
    WG_EACH(wg, tid) tp_step<FMT, CAP>(tid, gx, t, last, in, a, out, ring, stats ? cnt : nullptr);
    if (stats) {
      wg.sync();
      WG_EACH(wg, tid) cl_sum32(tid, cnt, part);
      wg.sync();
      WG_EACH(wg, tid) cl_sum_add(wg, tid, TP_STATS, part, stats + (long)t * TP_STATS);
    }
  }
}

// ---- the stream: one frame per step, the window resident in device memory (temporal_push.hip) ----------------------
// The same definition, one frame at a time.  The state is the caller's: a ring of TP_SLOTS planes of h x w codes in the stream's
// format, frame s in plane s & 15, and two words, state[TP_PUSHED] = N, the frames pushed so far, and state[TP_FLUSHED] = F, the
// flush steps taken since the last push.  A step is wg_temporal_push_begin (one workgroup) and then wg_temporal_push over
// ceil(h w / TP_TILE) workgroups; N and F are read from the state words, never from an argument, so one recorded step serves
// every later frame.
//   a push step   (in given): begin makes N += 1, F = 0.  The frame goes into slot (N - 1) & 15; frame t = N - 1 - ahead, if there
//                 is one, is final -- its window [max(0, t - back), t + ahead] ends at the frame just pushed -- and goes to `out`
//   a flush step  (in null): begin makes F += 1.  Frame t = max(0, N - ahead) + F - 1 goes to `out` if t <= N - 1, its window cut
//                 at the sequence's end N - 1
// Where no frame is final `out` is not written and the statistics row stays at the zeros of begin.
// SIXTEEN SLOTS SUFFICE.  Storing frame N - 1 overwrites frame N - 17 and no other.  The frames not yet emitted when frame
// N - 1 arrives are t >= N - 1 - ahead; the oldest frame one of their windows reads is N - 1 - ahead - back >= N - 15 > N - 17.
// A flush stores nothing.  (tests/test_temporal_stream_cpu.py walks the rule for every window and length.)
// A thread reads and writes its own four pixels of every plane and nothing else: no barrier, no LDS but the statistics' sums, no
// dependency between workgroups.  The window is gathered into CAP registers by a static index (only the slot is dynamic); the
// frame just pushed comes from the register that holds it.  N stays below 2^31 (the wrapper counts).
constexpr int TP_PUSHED = 0, TP_FLUSHED = 1, TP_STATE = 2;

// one workgroup: the counters' step, and the four statistics words to 0 (stats may be null)
template <class G>
CODON_FL_HD void wg_temporal_push_begin(G wg, int push, unsigned* state, unsigned* stats) {
  WG_EACH(wg, tid) {
    if (tid == 0) {
      if (push) {
        state[TP_PUSHED] += 1u;
        state[TP_FLUSHED] = 0u;
      } else {
        state[TP_FLUSHED] += 1u;
      }
    }
    if (stats && tid < TP_STATS) stats[tid] = 0u;
  }
}

// one thread's four pixels of a step: N frames are in (the new one among them where `in` is given), frame t is the one to emit
template <int FMT, int CAP>
CODON_FL_HD void tp_push_step(int tid, long gx, int N, int t, const void* in, const TpArgs& a, void* ring, void* out, unsigned* cnt) {
  const long hw = (long)a.h * a.w, p = (gx * TP_THREADS + tid) * TP_PER;
  unsigned first = 0, second = 0;
  if (p < hw) {
    tp_quad fresh = 0;
    if (in) {
      fresh = tp_load4<FMT>(in, p, hw - p, a.vec);
      tp_store4<FMT>(ring, (long)((N - 1) & (TP_SLOTS - 1)) * hw + p, hw - p, fresh, a.vec);
    }
    if (t >= 0 && t <= N - 1) {
      const int lo = t - a.back > 0 ? t - a.back : 0, nw = N - lo;     // hi = min(N - 1, t + ahead) = N - 1 in either step
      tp_quad wnd[CAP];
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int i = 0; i < CAP; ++i) {
        const bool held = in && i == nw - 1;                             // frame N - 1 of a push step: in `fresh`
        tp_quad word = 0;
        if (i < nw && !held) word = tp_load4<FMT>(ring, (long)((lo + i) & (TP_SLOTS - 1)) * hw + p, hw - p, a.vec);
        wnd[i] = held ? fresh : word;
      }
      tp_quad cur = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int i = 0; i < CAP; ++i) cur = i == t - lo ? wnd[i] : cur;
      const tp_quad res = tp_filter4<CAP>(wnd, cur, nw, a, first, second);
      tp_store4<FMT>(out, p, hw - p, res, a.vec);
    }
  }
  if (cnt) {
    cnt[tid] = first;
    cnt[TP_THREADS + tid] = second;
  }
}

// workgroup gx of grid (ceil(h w / TP_TILE)), after wg_temporal_push_begin.  in: the new frame, or null for a flush step; a.T and
// a.chunk are not read; a.vec: h w is a multiple of TP_PER and in, out and the ring stand on a multiple of TP_PER elements.  LDS:
// cnt 2 TP_THREADS words and part 32, read with statistics alone.  stats (may be null): the four words begin zeroed
template <int FMT, int CAP, class G>
CODON_FL_HD void wg_temporal_push(G wg, long gx, const void* in, const TpArgs& a, void* ring, const unsigned* state, void* out,
                                  unsigned* stats, unsigned* cnt, unsigned* part) {
  const int N = (int)state[TP_PUSHED], F = (int)state[TP_FLUSHED];
  const int t = in ? N - 1 - a.ahead : (N > a.ahead ? N - a.ahead : 0) + F - 1;
  WG_EACH(wg, tid) tp_push_step<FMT, CAP>(tid, gx, N, t, in, a, ring, out, stats ? cnt : nullptr);
  if (stats) {
    wg.sync();
    WG_EACH(wg, tid) cl_sum32(tid, cnt, part);
    wg.sync();
    WG_EACH(wg, tid) cl_sum_add(wg, tid, TP_STATS, part, stats);
  }
}

}  // namespace codon
