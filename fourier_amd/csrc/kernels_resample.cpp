// kernels_resample.cpp -- instantiates the sweeps of the resampling handle (kernels_resample.h): the spectrum remap and the fused
// untangle of the real even / even route.  Compiled once per precision: -DFOURIER_TU_REAL=float / double (fourier_amd/build.py).
#include "engine_common.h"
#include "kernels_resample.h"

namespace fourier_hip {

typedef FOURIER_TU_REAL TUReal;

ResampleKernel get_resample_kernel(Real<TUReal>, int which) {
  typedef TUReal T;
  switch (which) {
    case RESAMPLE_REMAP: return &resample_remap_kernel<T>;
    case RESAMPLE_UNTANGLE: return &resample_untangle_kernel<T>;
    default: return nullptr;
  }
}

}  // namespace fourier_hip
