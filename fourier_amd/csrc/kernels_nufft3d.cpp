// kernels_nufft3d.cpp -- instantiates the 3-D non-uniform FFT kernels (kernels_nufft3d.h): the spreading gather for every item block
// 1 ... NUFFT_RB (the tails are instances of their own; the kernel width is a launch argument), the interpolation for every kernel
// width of the precision (f32 2 ... 8, f64 2 ... 16) and every item block, the two sweeps and the set-up kernel of the tabulated
// weights.  Compiled once per precision: -DFOURIER_TU_REAL=float / double (fourier_amd/build.py).
#include "engine_common.h"
#include "kernels_nufft3d.h"

namespace fourier_hip {

typedef FOURIER_TU_REAL TUReal;

namespace {

constexpr int MAX_W = sizeof(TUReal) == 4 ? NUFFT_MAX_W_F32 : NUFFT_MAX_W_F64;

template <int W> Nufft3dKernel interp_of(int rb) {
  typedef TUReal T;
  static_assert(NUFFT_RB == 4, "one case per item block");
  switch (rb) {
    case 1: return &nufft3d_interp_kernel<T, W, 1>;
    case 2: return &nufft3d_interp_kernel<T, W, 2>;
    case 3: return &nufft3d_interp_kernel<T, W, 3>;
    case 4: return &nufft3d_interp_kernel<T, W, 4>;
    default: return nullptr;
  }
}

// interp_of<W>(rb) for the compile-time width equal to w
template <int W> Nufft3dKernel by_width(int w, int rb) {
  if constexpr (W > MAX_W) {
    return nullptr;
  } else {
    if (w == W) return interp_of<W>(rb);
    return by_width<W + 1>(w, rb);
  }
}

}  // namespace

Nufft3dKernel get_nufft3d_spread_kernel(Real<TUReal>, int rb) {
  typedef TUReal T;
  switch (rb) {
    case 1: return &nufft3d_spread_kernel<T, 1>;
    case 2: return &nufft3d_spread_kernel<T, 2>;
    case 3: return &nufft3d_spread_kernel<T, 3>;
    case 4: return &nufft3d_spread_kernel<T, 4>;
    default: return nullptr;
  }
}
Nufft3dKernel get_nufft3d_interp_kernel(Real<TUReal>, int w, int rb) { return w < NUFFT_MIN_W ? nullptr : by_width<NUFFT_MIN_W>(w, rb); }

Nufft3dKernel get_nufft3d_sweep_kernel(Real<TUReal>, int which) {
  typedef TUReal T;
  return which == NUFFT_DECONV ? &nufft3d_deconv_kernel<T> : which == NUFFT_AMPLIFY ? &nufft3d_amplify_kernel<T> : nullptr;
}

Nufft3dKernel get_nufft3d_table_kernel(Real<TUReal>) { return &nufft3d_table_kernel<TUReal>; }

}  // namespace fourier_hip
