// kernels_delay.cpp -- instantiates the delay kernels (kernels_delay.h): the one-launch kernel on the shapes of the two-level plans of
// 2^11 ... 2^15 (f64: ... 2^14), and the composed routes' sweep on half and on whole spectra.
// Compiled once per precision: -DFOURIER_TU_REAL=float / double (fourier_amd/build.py).
#include "engine_common.h"
#include "kernels_delay.h"

namespace fourier_hip {

typedef FOURIER_TU_REAL TUReal;

// An instance is in the table only if it spills no more than hilbert_small_kernel<T, L1, L2, true> of the same shape (gfx950,
// -Rpass-analysis=kernel-resource-usage; the table of DESIGN.md section 4, "Fractional delay").
bool get_delay_small_kernel(Real<TUReal>, int k, KernelInfo& info) {
  typedef TUReal T;
  switch (k) {
    case 11: return delay_small_info<T, 64, 32>(k, info);
    case 12: return delay_small_info<T, 64, 64>(k, info);
    case 13: return delay_small_info<T, 128, 64>(k, info);
    case 14: return delay_small_info<T, 128, 128>(k, info);
    case 15:
      if constexpr (sizeof(T) == 4) return delay_small_info<T, 256, 128>(k, info);
      return false;
    default: return false;
  }
}

DelayKernel get_delay_kernel(Real<TUReal>, bool real_data) {
  typedef TUReal T;
  return real_data ? &delay_mul_kernel<T, true> : &delay_mul_kernel<T, false>;
}

}  // namespace fourier_hip
