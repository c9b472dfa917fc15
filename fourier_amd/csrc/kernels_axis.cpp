// kernels_axis.cpp -- instantiates the kernels of the transforms along a strided axis (kernels_axis.h).
// Compiled once per precision: -DFOURIER_TU_REAL=float / double (fourier_amd/build.py).
#include "engine_common.h"
#include "kernels_axis.h"

namespace fourier_hip {

typedef FOURIER_TU_REAL TUReal;

AxisKernel get_axis_kernel(Real<TUReal>, int n) {
  typedef TUReal T;
  switch (n) {
    case 0: return &axis_transpose_kernel<T>;
#define FOURIER_AXIS_LANE(N) case N: return &axis_lane_kernel<T, N>;
    FOURIER_AXIS_LANE(1) FOURIER_AXIS_LANE(2) FOURIER_AXIS_LANE(3) FOURIER_AXIS_LANE(4) FOURIER_AXIS_LANE(5) FOURIER_AXIS_LANE(6)
    FOURIER_AXIS_LANE(7) FOURIER_AXIS_LANE(8) FOURIER_AXIS_LANE(9) FOURIER_AXIS_LANE(10) FOURIER_AXIS_LANE(11) FOURIER_AXIS_LANE(12)
    FOURIER_AXIS_LANE(13) FOURIER_AXIS_LANE(14) FOURIER_AXIS_LANE(15) FOURIER_AXIS_LANE(16) FOURIER_AXIS_LANE(17) FOURIER_AXIS_LANE(18)
    FOURIER_AXIS_LANE(19) FOURIER_AXIS_LANE(20) FOURIER_AXIS_LANE(21) FOURIER_AXIS_LANE(22) FOURIER_AXIS_LANE(23) FOURIER_AXIS_LANE(24)
    FOURIER_AXIS_LANE(25) FOURIER_AXIS_LANE(26) FOURIER_AXIS_LANE(27) FOURIER_AXIS_LANE(28) FOURIER_AXIS_LANE(29) FOURIER_AXIS_LANE(30)
    FOURIER_AXIS_LANE(31) FOURIER_AXIS_LANE(32)
#undef FOURIER_AXIS_LANE
    default: return nullptr;
  }
}

}  // namespace fourier_hip
