// option_probe.cpp -- TEST-ONLY: a stand-alone walk of plan states through the C ABI (include/fourier.h and nothing else), linked by
// tests/test_option_emu.py against the AddressSanitizer build of the emulation library (tests/emu/build_emu.py, FOURIER_EMU_ASAN=1) with
// -fsanitize=address and run as a child process.  An undersized scratch, unlike a null one, corrupts a neighbouring buffer silently; here
// every buffer -- the plan's, and the input and output, which are exactly as long as the call says -- has the sanitizer's red zones.
//
// usage: option_probe <state list>.  One state a line:
//   <length> <f32|f64> <batch> <reserve 0|1> <kind 0..3> <transform code> <input file> <output file> [key=value ...]
// A fresh plan gets the options in the order given; reserve 1 calls fourier_hip_reserve_* out of place and in place; kind 0 = plain,
// 1 = plain in place, 2 = profiled, 3 = profiled in place.  The input file holds batch * length complex values, the output file gets
// as many.  Exit status 0 where every state ran and every call returned FOURIER_HIP_OK; the test compares the outputs' bits.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "fourier.h"

using namespace fourier::c;

template <typename Handle> struct Abi {
  Handle* (*create)(size_t);
  void (*destroy)(Handle*);
  int (*set_option)(Handle*, const char*, long long);
  int (*reserve)(const Handle*, size_t, int);
  int (*transform)(const Handle*, const void*, void*, size_t, int, void*);
  int (*profile)(const Handle*, const void*, void*, size_t, int, void*, int, float*, int*);
};

static int fail(int line, const std::string& what) {
  fprintf(stderr, "option_probe: state %d: %s\n", line, what.c_str());
  return 1;
}

template <typename Handle> static int run_state(const Abi<Handle>& abi, int line, size_t n, size_t elem, std::istringstream& in) {
  size_t batch = 0;
  int reserve = 0, kind = 0, code = 0;
  std::string in_path, out_path, setting;
  if (!(in >> batch >> reserve >> kind >> code >> in_path >> out_path) || batch == 0 || kind < 0 || kind > 3) return fail(line, "malformed");
  Handle* h = abi.create(n);
  if (!h) return fail(line, "create failed");
  while (in >> setting) {
    const size_t eq = setting.find('=');
    if (eq == std::string::npos) return fail(line, "malformed option " + setting);
    if (abi.set_option(h, setting.substr(0, eq).c_str(), atoll(setting.c_str() + eq + 1)) != 0) return fail(line, "refused " + setting);
  }
  if (reserve && (abi.reserve(h, batch, 0) != 0 || abi.reserve(h, batch, 1) != 0)) return fail(line, "reserve failed");
  const size_t bytes = batch * n * elem;
  char* x = (char*)malloc(bytes);
  char* y = (char*)malloc(bytes);
  FILE* f = fopen(in_path.c_str(), "rb");
  if (!x || !y || !f || fread(x, 1, bytes, f) != bytes) return fail(line, "cannot read " + in_path);
  fclose(f);
  const bool in_place = (kind & 1) != 0, profiled = (kind & 2) != 0;
  if (in_place) memcpy(y, x, bytes);
  else memset(y, 0xff, bytes);
  const void* src = in_place ? y : x;
  float ms[16];
  int launches[16];
  const int st = profiled ? abi.profile(h, src, y, batch, code, nullptr, 16, ms, launches) : abi.transform(h, src, y, batch, code, nullptr);
  if (st != 0) return fail(line, "the call returned " + std::to_string(st));
  f = fopen(out_path.c_str(), "wb");
  if (!f || fwrite(y, 1, bytes, f) != bytes || fclose(f) != 0) return fail(line, "cannot write " + out_path);
  free(x);
  free(y);
  abi.destroy(h);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) return fail(0, "usage: option_probe <state list>");
  FILE* list = fopen(argv[1], "r");
  if (!list) return fail(0, "cannot open the state list");
  const Abi<fourier_fft_float> f32{fourier_create_float, fourier_destroy_float, fourier_hip_set_option_float, fourier_hip_reserve_float,
                                   fourier_hip_transform_batch_float, fourier_hip_profile_float};
  const Abi<fourier_fft_double> f64{fourier_create_double, fourier_destroy_double, fourier_hip_set_option_double, fourier_hip_reserve_double,
                                    fourier_hip_transform_batch_double, fourier_hip_profile_double};
  char buf[4096];
  int line = 0, ran = 0;
  while (fgets(buf, sizeof buf, list)) {
    ++line;
    std::istringstream in(buf);
    size_t n = 0;
    std::string real;
    if (!(in >> n >> real)) continue;  // an empty line
    const int bad = real == "f32" ? run_state(f32, line, n, 2 * sizeof(float), in) : real == "f64" ? run_state(f64, line, n, 2 * sizeof(double), in)
                                                                                                    : fail(line, "unknown precision " + real);
    if (bad) return bad;
    ++ran;
  }
  fclose(list);
  printf("option_probe: %d states\n", ran);
  return 0;
}
