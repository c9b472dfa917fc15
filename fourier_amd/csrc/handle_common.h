// handle_common.h -- the host toolkit every handle class shares (Plan, AxisRoute, RealPlan, RealNdPlan, ConvPlan): device guard,
// argument checks, the transform codes and their scale, chunk and grid sizes, the real transforms' twiddle table, and the error model
// of the C ABI.  Host code only: plan.h includes it, no kernel translation unit does.
#pragma once
#include <cstdlib>
#include <utility>

#include "engine_common.h"

namespace fourier_hip {

// makes `dev` the current device for a scope
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
    else prev = -1;
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// x / d = (umulhi(x, m) + x) >> l for every 32-bit x, d >= 1: what a sweep kernel divides by
static inline void divider(uint32_t d, uint32_t& m, uint32_t& l) {
  l = 0;
  while ((1ull << l) < d) ++l;
  m = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << l) - d)) / d + 1);
}

// The buffers of a device call: both given, both aligned to `align` bytes, and the in_bytes at `in` apart from the out_bytes at `out`
// -- except that in == out is an in-place call where the handle allows one (an empty call has no bytes to overlap)
static inline void check_buffers(const void* in, const void* out, size_t in_bytes, size_t out_bytes, size_t align, bool in_place_allowed) {
  if (!in || !out) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "null buffer");
  const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
  if (a % align || b % align) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "misaligned buffer");
  if (a == b ? !in_place_allowed : (a < b + out_bytes && b < a + in_bytes))
    throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "input and output overlap");
}

// fft.rs:20-25 is_forward; the other three codes are the inverses
static inline bool is_forward(int code) {
  return code == ::fourier::c::FOURIER_TRANSFORM_FFT || code == ::fourier::c::FOURIER_TRANSFORM_SQRT_SCALED_FFT;
}
static inline bool is_inverse(int code) {
  return code == ::fourier::c::FOURIER_TRANSFORM_IFFT || code == ::fourier::c::FOURIER_TRANSFORM_UNSCALED_IFFT ||
         code == ::fourier::c::FOURIER_TRANSFORM_SQRT_SCALED_IFFT;
}
// the code's scale over n points, computed in T (autosort/mod.rs:381-385) and widened for the argument block
template <typename T> static double code_scale(int code, T n) {
  if (code == ::fourier::c::FOURIER_TRANSFORM_IFFT) return (double)((T)1 / n);
  if (code == ::fourier::c::FOURIER_TRANSFORM_SQRT_SCALED_FFT || code == ::fourier::c::FOURIER_TRANSFORM_SQRT_SCALED_IFFT)
    return (double)((T)1 / std::sqrt((T)n));
  return 1.0;
}

// rows per chunk of a call of `batch` rows of `per` bytes such that a chunk stays within `cap` bytes (never less than one row)
static inline size_t chunk_rows(size_t batch, size_t cap, size_t per) { return std::max<size_t>(1, std::min<size_t>(batch, cap / per)); }
// f(b0, nb) for every chunk of the `batch` rows of a call, in order: nb = `chunk` rows from row b0 on, fewer in the last one
template <typename F> static inline void for_chunks(size_t batch, size_t chunk, F&& f) {
  for (size_t b0 = 0; b0 < batch; b0 += chunk) f(b0, std::min(chunk, batch - b0));
}
// a scratch bound: `dflt`, or what the development switch `name` says (experiments library and emulator build only, read at create)
static inline size_t scratch_bound(const char* name, size_t dflt) {
  const char* e = dev_env(name);
  return e ? (size_t)std::strtoull(e, nullptr, 10) : dflt;
}
// a launch bound: `dflt` (what the kernels' 32-bit indices and 31-bit byte offsets allow), or what the development switch `name`
// says where that is smaller and not 0 (FOURIER_LAUNCH_BYTES, FOURIER_LAUNCH_ITEMS; visible and read as scratch_bound's are)
static inline size_t launch_bound(const char* name, size_t dflt) {
  const char* e = dev_env(name);
  const size_t v = e ? (size_t)std::strtoull(e, nullptr, 10) : dflt;
  return v == 0 ? dflt : std::min(v, dflt);
}

// workgroups of 256 threads for a grid-stride sweep over `elems` elements
static inline unsigned elementwise_grid(size_t elems) {
  return (unsigned)std::min<size_t>(std::max<size_t>((elems + 255) / 256, 1), 256 * 32);
}

// W_n^j, j <= n/4, of the even-length real transforms' untangle sweeps: f64 trigonometry, cast (twiddle.rs:7-19)
template <typename T> static std::vector<cpx<T>> real_untangle_twiddles(size_t n) {
  std::vector<cpx<T>> tw(n / 4 + 1);
  for (size_t j = 0; j < tw.size(); ++j) { double re, im; unit_root(j, n, re, im); tw[j] = {(T)re, (T)im}; }
  return tw;
}

// what the C ABI reads of every handle: the status of the last call and the route description
class HandleBase {
 public:
  HandleBase() = default;
  HandleBase(const HandleBase&) = delete;
  HandleBase& operator=(const HandleBase&) = delete;
  const char* describe() const { return desc_.c_str(); }
  int last_status() const { return status_; }
  void set_status(int s) const { status_ = s; }

 protected:
  std::string desc_;

 private:
  mutable int status_ = 0;
};

// the error model of every handle: NULL from a create that throws, status of the last call, nothing unwinds into C
// (fourier-ffi/src/lib.rs:18-19)
template <typename H, typename... A> static H* create_handle(A... args) {
  try {
    return new H(args...);
  } catch (...) {
    return nullptr;
  }
}
template <typename H, typename F> static int guarded_handle(const H* p, F&& f) {
  if (!p) return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
  p->set_status(::fourier::c::FOURIER_HIP_OK);  // last_status = status of the LAST call on this handle
  try {
    f();
    return ::fourier::c::FOURIER_HIP_OK;
  } catch (const EngineError& e) {
    p->set_status(e.status);
    if (getenv("FOURIER_HIP_VERBOSE")) fprintf(stderr, "libfourier: %s\n", e.what());
    return e.status;
  } catch (const std::bad_alloc&) {
    p->set_status(::fourier::c::FOURIER_HIP_OUT_OF_MEMORY);
    return ::fourier::c::FOURIER_HIP_OUT_OF_MEMORY;
  } catch (...) {
    p->set_status(::fourier::c::FOURIER_HIP_RUNTIME_ERROR);
    return ::fourier::c::FOURIER_HIP_RUNTIME_ERROR;
  }
}

}  // namespace fourier_hip
