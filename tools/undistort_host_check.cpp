// Host-side check of the undistortion of colour images: the launch plan, the host's tile table and the
// workgroup body of csrc/undistort_tile.h -- the very text the device kernel of csrc/undistort.hip calls -- compiled for the host
// and run workgroup by workgroup over exactly-sized heap buffers (the LDS arrays too: the weights and the 48 x 24 window), so that
// the address and undefined-behaviour sanitizers see every access.  Every case runs with the threads of a workgroup forwards and
// backwards, and the two outputs must agree.  The images lie `skew` bytes into their buffers: no alignment is promised for them.
// No GPU, no HIP, nothing loaded into Python.
// `python tools/host_check.py undistort` builds this, runs it over the GPU test's cases and compares what it writes with
// tests/undistort_ref.py, bit for bit.
//
//   undistort_host_check <channels 1|3> B hs ws ho wo skew in.bin map.bin weights.bin out.bin tiles.bin counts.bin
//     in.bin: (B, hs, ws, channels) u8; map.bin: (ho, wo, 2) int32; weights.bin: (32, 4) int16
//     ->  out.bin: (B, ho, wo, channels) u8; tiles.bin: (ty, tx, 4) int32; counts.bin: 4 uint32
#include "host_check.h"

#include "../codon_amd/csrc/undistort_tile.h"

using namespace codon;

// undistort(): the one launch
template <int C>
static void launch(WgHost wg, int B, const unsigned char* in, int hs, int ws, int ho, int wo, const int* map, const int* tiles,
                   const short* weights, unsigned char* out) {
  const UdPlan p = ud_plan(ho, wo);
  for (long b = 0; b < B; ++b)
    for (int ty = 0; ty < p.ty; ++ty)
      for (int tx = 0; tx < p.tx; ++tx) {
        short* lk = hc_alloc<short>(sizeof(short) * UD_WEIGHTS, 0xCD);
        unsigned* win = hc_alloc<unsigned>(sizeof(unsigned) * UD_WIN, 0xCD);
        wg_undistort_tile<C>(wg, tx, ty, b, in, hs, ws, ho, wo, map, tiles, weights, out, lk, win);
        free(lk), free(win);
      }
}

template <int C>
static int run(int B, int hs, int ws, int ho, int wo, int skew, char** path) {
  const size_t in_bytes = (size_t)B * hs * ws * C, out_bytes = (size_t)B * ho * wo * C, map_bytes = sizeof(int) * 2 * ho * wo;
  const UdPlan p = ud_plan(ho, wo);
  const size_t tiles_bytes = sizeof(int) * 4 * p.tx * p.ty;
  unsigned char* in = hc_read<unsigned char>(path[0], in_bytes, skew);
  int* map = hc_read<int>(path[1], map_bytes, 0, hc_aligned(map_bytes));
  short* weights = hc_read<short>(path[2], sizeof(short) * UD_WEIGHTS);
  int* tiles = (int*)memset(hc_aligned(tiles_bytes), 0xEE, tiles_bytes);
  unsigned* counts = hc_alloc<unsigned>(sizeof(unsigned) * UD_COUNTS, 0xEE);
  if (ud_tiles(hs, ws, ho, wo, map, tiles, counts) >= 0) hc_die("a map entry outside the source image");
  unsigned char* out[2];
  for (int rev = 0; rev < 2; ++rev) {
    out[rev] = hc_alloc<unsigned char>(skew + out_bytes, 0xEE);
    launch<C>(WgHost{UD_THREADS, rev != 0}, B, in + skew, hs, ws, ho, wo, map, tiles, weights, out[rev] + skew);
  }
  hc_same(out[0], out[1], skew + out_bytes, "the output depends on the order of the threads within a phase");
  hc_write(path[3], out[0] + skew, out_bytes);
  hc_write(path[4], tiles, tiles_bytes);
  hc_write(path[5], counts, sizeof(unsigned) * UD_COUNTS);
  free(in), free(map), free(weights), free(tiles), free(counts), free(out[0]), free(out[1]);
  return 0;
}

int main(int argc, char** argv) {
  hc_name = "undistort_host_check";
  if (argc != 14)
    hc_die("usage: undistort_host_check <channels 1|3> B hs ws ho wo skew in.bin map.bin weights.bin out.bin tiles.bin counts.bin");
  const int C = atoi(argv[1]), B = atoi(argv[2]), hs = atoi(argv[3]), ws = atoi(argv[4]), ho = atoi(argv[5]), wo = atoi(argv[6]);
  const int skew = atoi(argv[7]);
  if (B < 1 || hs < 1 || hs > UD_MAX_SIDE || ws < 1 || ws > UD_MAX_SIDE || ho < 1 || ho > UD_MAX_SIDE || wo < 1 || wo > UD_MAX_SIDE ||
      skew < 0 || skew > 15)
    return 2;
  if (C == 1) return run<1>(B, hs, ws, ho, wo, skew, argv + 8);
  if (C == 3) return run<3>(B, hs, ws, ho, wo, skew, argv + 8);
  return 2;
}
