// Host-side check of the sensor model's kernel: the per-pixel body of csrc/sensor_pixel.h with the generator of
// csrc/sensor_rng.h -- the very text the device kernel of csrc/sensor.hip calls -- compiled for the host and driven sample by
// sample, pixel by pixel over exactly-sized heap buffers, so that the address and undefined-behaviour sanitizers see every
// access.  No GPU, no HIP, nothing loaded into Python.  `python tools/host_check.py sensor` builds this (with
// -ffp-contract=off), runs it over the GPU tests' shapes and compares what it writes with tests/sensor_ref.py, byte for byte.
//
//   sensor_host_check DIR      reads DIR/cases.bin, DIR/gauss.bin (65 536 fp32), DIR/lut<levels>.bin (levels + 1 fp32);
//                              writes DIR/out.bin, the output maps of the cases one after the other
// cases.bin: per case a 64-byte record (the struct below) followed by its input map, batch * size * size fp32.
#include <cstdint>

#include "host_check.h"

#include "../codon_amd/csrc/sensor_pixel.h"

using namespace codon;

struct CaseRecord {
  int32_t batch, size, masked, levels;
  uint32_t k0, k1, step, first;
  float sigma, quad, edge_thr;
  uint32_t reserved;
  uint64_t t_drop, t_edge;
};
static_assert(sizeof(CaseRecord) == 64, "cases.bin's record is 64 bytes");

int main(int argc, char** argv) {
  hc_name = "sensor_host_check";
  if (argc != 2) hc_die("usage: sensor_host_check DIR");
  const std::string dir = std::string(argv[1]) + "/";
  float* gauss = hc_read<float>(dir + "gauss.bin", 65536 * sizeof(float));
  FILE* in = fopen((dir + "cases.bin").c_str(), "rb");
  FILE* out = fopen((dir + "out.bin").c_str(), "wb");
  if (!in || !out) hc_die("cannot open cases.bin / out.bin");
  CaseRecord c;
  int cases = 0;
  while (fread(&c, sizeof(c), 1, in) == 1) {
    if (c.batch < 1 || c.batch > 64 || c.size < 4 || c.size > 512 || c.levels < 1 || c.levels > 65535) hc_die("bad case record");
    const size_t pp = (size_t)c.size * c.size, n = (size_t)c.batch * pp;
    float* lr = hc_alloc<float>(n * sizeof(float), 0);
    float* res = hc_alloc<float>(n * sizeof(float), 0xEE);          // a pixel no thread writes stays this
    if (fread(lr, sizeof(float), n, in) != n) hc_die("short case");
    float* lut = hc_read<float>(dir + "lut" + std::to_string(c.levels) + ".bin", ((size_t)c.levels + 1) * sizeof(float));
    SensorArgs a;
    a.p = c.size; a.masked = c.masked; a.levels = c.levels;
    a.k0 = c.k0; a.k1 = c.k1; a.step = c.step; a.first = c.first;
    a.sigma = c.sigma; a.quad = c.quad; a.edge_thr = c.edge_thr;
    a.t_drop = c.t_drop; a.t_edge = c.t_edge;
    // the launch of lr_sensor_kernel: grid (ceil(p*p / 256), B), thread idx of block-row b owns pixel idx of sample b
    for (int b = 0; b < c.batch; ++b)
      for (int idx = 0; idx < (int)pp; ++idx) {
        const int y = idx / c.size;
        res[(size_t)b * pp + idx] = sensor_pixel(a, lr + (size_t)b * pp, gauss, lut, b, y, idx - y * c.size);
      }
    if (fwrite(res, sizeof(float), n, out) != n) hc_die("cannot write out.bin");
    free(lr);
    free(res);
    free(lut);
    ++cases;
  }
  if (!feof(in) || fclose(out) != 0) hc_die("cases.bin ends inside a record");
  fclose(in);
  free(gauss);
  printf("%d cases\n", cases);
  return 0;
}
