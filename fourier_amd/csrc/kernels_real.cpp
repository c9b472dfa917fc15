// kernels_real.cpp -- instantiates the real-input transform kernels (kernels_real.h).
// Compiled once per precision: -DFOURIER_TU_REAL=float / double (fourier_amd/build.py).
#include "engine_common.h"
#include "kernels_real.h"

namespace fourier_hip {

typedef FOURIER_TU_REAL TUReal;

RealKernel get_real_kernel(Real<TUReal>, int which) {
  typedef TUReal T;
  switch (which) {
    case REAL_POST: return &real_post_kernel<T>;
    case REAL_PRE: return &real_pre_kernel<T>;
    case REAL_WIDEN: return &real_widen_kernel<T>;
    case REAL_NARROW: return &real_narrow_kernel<T>;
    case REAL_EXTEND: return &real_extend_kernel<T>;
    case REAL_PART: return &real_part_kernel<T>;
    case REAL_ND_POST: return &realnd_post_kernel<T>;
    case REAL_ND_PRE: return &realnd_pre_kernel<T>;
    default: return nullptr;
  }
}

}  // namespace fourier_hip
