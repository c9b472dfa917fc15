// kernels_czt.cpp -- instantiates the chirp-z kernels (kernels_czt.h): the one-launch kernel on the shapes of the two-level plans of
// 2^11 ... 2^15 (f64: ... 2^14), complex and real input rows, and the two end sweeps of the composed route.
// Compiled once per precision: -DFOURIER_TU_REAL=float / double (fourier_amd/build.py).
#include "engine_common.h"
#include "kernels_czt.h"

namespace fourier_hip {

typedef FOURIER_TU_REAL TUReal;

// the launch shape and the LDS bytes are the two-level plan's of the same length (kernels_onelaunch.cpp)
template <typename T, int L1, int L2> static bool czt_small_info(int k, bool real_input, KernelInfo& info) {
  int l1 = 0, l2 = 0;
  if (!get_twolevel_kernel(Real<T>{}, k, info, l1, l2) || l1 != L1 || l2 != L2) return false;
  info.fn = real_input ? &czt_small_kernel<T, L1, L2, true> : &czt_small_kernel<T, L1, L2, false>;
  return true;
}
bool get_czt_small_kernel(Real<TUReal>, int k, bool real_input, KernelInfo& info) {
  typedef TUReal T;
  switch (k) {
    case 11: return czt_small_info<T, 64, 32>(k, real_input, info);
    case 12: return czt_small_info<T, 64, 64>(k, real_input, info);
    case 13: return czt_small_info<T, 128, 64>(k, real_input, info);
    case 14: return czt_small_info<T, 128, 128>(k, real_input, info);
    case 15:
      if constexpr (sizeof(T) == 4) return czt_small_info<T, 256, 128>(k, real_input, info);
      return false;
    default: return false;
  }
}

CztKernel get_czt_kernel(Real<TUReal>, int which) {
  typedef TUReal T;
  switch (which) {
    case CZT_IN: return &czt_in_kernel<T>;
    case CZT_OUT: return &czt_out_kernel<T>;
    default: return nullptr;
  }
}

}  // namespace fourier_hip
