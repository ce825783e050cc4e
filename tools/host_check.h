// What every host-side sanitizer check (tools/*_host_check.cpp, built and run by tools/host_check.py) needs: files
// read and written exactly, and buffers of exactly the bytes asked for, so that one element past either end is a sanitizer
// report.  A program sets hc_name first thing in main.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

static const char* hc_name = "host_check";

[[noreturn]] static void hc_die(const std::string& what) {
  fprintf(stderr, "%s: %s\n", hc_name, what.c_str());
  exit(2);
}

// exactly `bytes` bytes with every byte `pattern`: 0xCD for an LDS array (what a phase reads without an earlier phase having
// written it shows as this), 0xEE for an output (an element no thread writes stays this)
template <typename T = void>
static T* hc_alloc(size_t bytes, int pattern) {
  void* p = malloc(bytes);
  if (!p) hc_die("out of memory");
  return (T*)memset(p, pattern, bytes);
}

// 16-byte aligned, as a device allocation is at least
static char* hc_aligned(size_t bytes) {
  void* p = nullptr;
  if (posix_memalign(&p, 16, bytes) != 0) hc_die("out of memory");
  return (char*)p;
}

// the file must hold exactly `bytes` bytes; they go `lead` bytes into a buffer of exactly lead + bytes
template <typename T = void>
static T* hc_read(const std::string& path, size_t bytes, size_t lead = 0, char* into = nullptr) {
  char* p = into ? into : hc_alloc<char>(lead + bytes, 0);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f || fread(p + lead, 1, bytes, f) != bytes || fgetc(f) != EOF)
    hc_die(path + " does not hold exactly " + std::to_string(bytes) + " bytes");
  fclose(f);
  return (T*)p;
}

static void hc_write(const std::string& path, const void* p, size_t bytes) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, 1, bytes, f) != bytes || fclose(f) != 0) hc_die("cannot write " + path);
}

// two runs of one case that must agree (the two thread orders of the host group; in place and into another buffer)
static void hc_same(const void* a, const void* b, size_t bytes, const char* what) {
  if (memcmp(a, b, bytes) != 0) {
    fprintf(stderr, "%s: %s\n", hc_name, what);
    exit(3);
  }
}
