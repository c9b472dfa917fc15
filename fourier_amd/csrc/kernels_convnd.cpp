// kernels_convnd.cpp -- instantiates the sweeps of the N-D convolution handle (kernels_convnd.h).
// Compiled once per precision: -DFOURIER_TU_REAL=float / double (fourier_amd/build.py).
#include "engine_common.h"
#include "kernels_convnd.h"

namespace fourier_hip {

typedef FOURIER_TU_REAL TUReal;

ConvNdKernel get_convnd_kernel(Real<TUReal>, int which) {
  typedef TUReal T;
  switch (which) {
    case CONVND_MID: return &realnd_conv_mid_kernel<T>;
    case CONVND_PAD: return &convnd_pad_kernel<T>;
    case CONVND_CROP: return &convnd_crop_kernel<T>;
    case CONVND_MUL: return &convnd_mul_kernel<T>;
    default: return nullptr;
  }
}

}  // namespace fourier_hip
