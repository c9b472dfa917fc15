// kernels_nufft.cpp -- instantiates the non-uniform FFT kernels (kernels_nufft.h): the spreading gather and the interpolation for
// every kernel width of the precision (f32 2 ... 8, f64 2 ... 16) and every row block 1 ... NUFFT_RB (the tails are instances of
// their own), the two sweeps and the set-up kernel of the tabulated weights.
// Compiled once per precision: -DFOURIER_TU_REAL=float / double (fourier_amd/build.py).
#include "engine_common.h"
#include "kernels_nufft.h"

namespace fourier_hip {

typedef FOURIER_TU_REAL TUReal;

namespace {

constexpr int MAX_W = sizeof(TUReal) == 4 ? NUFFT_MAX_W_F32 : NUFFT_MAX_W_F64;

template <int W> NufftKernel spread_of(int rb) {
  typedef TUReal T;
  static_assert(NUFFT_RB == 4, "one case per row block");
  switch (rb) {
    case 1: return &nufft_spread_kernel<T, W, 1>;
    case 2: return &nufft_spread_kernel<T, W, 2>;
    case 3: return &nufft_spread_kernel<T, W, 3>;
    case 4: return &nufft_spread_kernel<T, W, 4>;
    default: return nullptr;
  }
}
template <int W> NufftKernel interp_of(int rb) {
  typedef TUReal T;
  switch (rb) {
    case 1: return &nufft_interp_kernel<T, W, 1>;
    case 2: return &nufft_interp_kernel<T, W, 2>;
    case 3: return &nufft_interp_kernel<T, W, 3>;
    case 4: return &nufft_interp_kernel<T, W, 4>;
    default: return nullptr;
  }
}

// f(width) for the compile-time width equal to w
template <int W, bool SPREAD> NufftKernel by_width(int w, int rb) {
  if constexpr (W > MAX_W) {
    return nullptr;
  } else {
    if (w == W) return SPREAD ? spread_of<W>(rb) : interp_of<W>(rb);
    return by_width<W + 1, SPREAD>(w, rb);
  }
}

}  // namespace

NufftKernel get_nufft_spread_kernel(Real<TUReal>, int w, int rb) { return w < NUFFT_MIN_W ? nullptr : by_width<NUFFT_MIN_W, true>(w, rb); }
NufftKernel get_nufft_interp_kernel(Real<TUReal>, int w, int rb) { return w < NUFFT_MIN_W ? nullptr : by_width<NUFFT_MIN_W, false>(w, rb); }

NufftKernel get_nufft_sweep_kernel(Real<TUReal>, int which) {
  typedef TUReal T;
  return which == NUFFT_DECONV ? &nufft_deconv_kernel<T> : which == NUFFT_AMPLIFY ? &nufft_amplify_kernel<T> : nullptr;
}

NufftKernel get_nufft_table_kernel(Real<TUReal>) { return &nufft_table_kernel<TUReal>; }

}  // namespace fourier_hip
