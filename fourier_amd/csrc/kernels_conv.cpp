// kernels_conv.cpp -- instantiates the sweeps of the convolution handle (kernels_conv.h).
// Compiled once per precision: -DFOURIER_TU_REAL=float / double (fourier_amd/build.py).
#include "engine_common.h"
#include "kernels_conv.h"

namespace fourier_hip {

typedef FOURIER_TU_REAL TUReal;

ConvKernel get_conv_sweep_kernel(Real<TUReal>, int which) {
  typedef TUReal T;
  switch (which) {
    case CONV_MUL: return &conv_mul_kernel<T>;
    case CONV_REAL_MID: return &real_conv_mid_kernel<T>;
    case CONV_FINISH: return &conv_finish_kernel<T>;
    case CONV_PAD: return &conv_pad_kernel<T>;
    case CONV_LCOPY: return &lconv_copy_kernel<T>;
    case CONV_LTAPS: return &lconv_taps_kernel<T>;
    default: return nullptr;
  }
}

}  // namespace fourier_hip
