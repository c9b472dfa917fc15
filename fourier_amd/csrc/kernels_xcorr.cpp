// kernels_xcorr.cpp -- instantiates the cross-correlation kernels (kernels_xcorr.h): the one-launch kernel's instances without scratch
// memory (f64, no weighting, 2^11 ... 2^14), and the sweeps of the composed routes on real and complex values.
// Compiled once per precision: -DFOURIER_TU_REAL=float / double (fourier_amd/build.py).
#include "engine_common.h"
#include "kernels_xcorr.h"

namespace fourier_hip {

typedef FOURIER_TU_REAL TUReal;

// Only an instance WITHOUT scratch memory is in the one-launch table (gfx950, -Rpass-analysis=kernel-resource-usage under the
// 128-VGPR bound of the launch bounds; the table of DESIGN.md section 4): f64 without weighting.  The f32 instances sit on the 12 - 20
// bytes a lane that the shared core spills in every f32 kernel built on it; f64 PHAT has 20 - 24.  Those are instantiated in the
// experiments library only (get_xcorr_spilling_kernel, kernels_experiments.cpp): the product holds no code for them.
bool get_xcorr_small_kernel(Real<TUReal>, int k, bool phat, KernelInfo& info) {
  typedef TUReal T;
  if constexpr (sizeof(T) == 8) {
    if (!phat) return xcorr_small_by_length<T, false>(k, info);
  }
  return false;
}

XcorrKernel get_xcorr_kernel(Real<TUReal>, int which, bool real_data, bool phat) {
  typedef TUReal T;
  switch (which) {
    case XCORR_PAD: return real_data ? &xcorr_pad_kernel<T, true> : &xcorr_pad_kernel<T, false>;
    case XCORR_MUL: return phat ? &xcorr_mul_kernel<T, true> : &xcorr_mul_kernel<T, false>;
    case XCORR_WINDOW: return real_data ? &xcorr_window_kernel<T, true> : &xcorr_window_kernel<T, false>;
    default: return nullptr;
  }
}

}  // namespace fourier_hip
