// kernels_hilbert.cpp -- instantiates the analytic-signal kernels (kernels_hilbert.h): the one-launch kernel on the shapes of the
// two-level plans of 2^11 ... 2^15 (f64: ... 2^14), analytic and envelope, and the two sweeps of the composed route.
// Compiled once per precision: -DFOURIER_TU_REAL=float / double (fourier_amd/build.py).
#include "engine_common.h"
#include "kernels_hilbert.h"

namespace fourier_hip {

typedef FOURIER_TU_REAL TUReal;

// the launch shape and the LDS bytes are the two-level plan's of the same length (kernels_onelaunch.cpp)
template <typename T, int L1, int L2> static bool hilbert_small_info(int k, bool envelope, KernelInfo& info) {
  int l1 = 0, l2 = 0;
  if (!get_twolevel_kernel(Real<T>{}, k, info, l1, l2) || l1 != L1 || l2 != L2) return false;
  info.fn = envelope ? &hilbert_small_kernel<T, L1, L2, true> : &hilbert_small_kernel<T, L1, L2, false>;
  return true;
}
bool get_hilbert_small_kernel(Real<TUReal>, int k, bool envelope, KernelInfo& info) {
  typedef TUReal T;
  switch (k) {
    case 11: return hilbert_small_info<T, 64, 32>(k, envelope, info);
    case 12: return hilbert_small_info<T, 64, 64>(k, envelope, info);
    case 13: return hilbert_small_info<T, 128, 64>(k, envelope, info);
    case 14: return hilbert_small_info<T, 128, 128>(k, envelope, info);
    case 15:
      if constexpr (sizeof(T) == 4) return hilbert_small_info<T, 256, 128>(k, envelope, info);
      return false;
    default: return false;
  }
}

HilbertKernel get_hilbert_kernel(Real<TUReal>, int which) {
  typedef TUReal T;
  switch (which) {
    case HILBERT_EXPAND: return &hilbert_expand_kernel<T>;
    case HILBERT_ABS: return &hilbert_abs_kernel<T>;
    default: return nullptr;
  }
}

}  // namespace fourier_hip
