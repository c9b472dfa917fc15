// kernels_r2r.cpp -- instantiates the DCT / DST sweeps (kernels_r2r.h).
// Compiled once per precision: -DFOURIER_TU_REAL=float / double (fourier_amd/build.py).
#include "engine_common.h"
#include "kernels_r2r.h"

namespace fourier_hip {

typedef FOURIER_TU_REAL TUReal;

R2RKernel get_r2r_kernel(Real<TUReal>, int which) {
  typedef TUReal T;
  switch (which) {
    case R2R_PACK: return &r2r_pack_kernel<T>;
    case R2R_POST: return &r2r_post_kernel<T>;
    case R2R_PRE: return &r2r_pre_kernel<T>;
    case R2R_UNPACK: return &r2r_unpack_kernel<T>;
    case R2R_ODD_WIDEN: return &r2r_odd_widen_kernel<T>;
    case R2R_ODD_POST: return &r2r_odd_post_kernel<T>;
    case R2R_ODD_PRE: return &r2r_odd_pre_kernel<T>;
    case R2R_ODD_PART: return &r2r_odd_part_kernel<T>;
    default: return nullptr;
  }
}

}  // namespace fourier_hip
