// kernels_stft.cpp -- instantiates the short-time Fourier transform kernels (kernels_stft.h): the frame gather and the overlap-add of the
// composed routes, and the fused one-launch frame route on the whole-row kernels' tile shapes (kernels_pass.cpp's MODE_ROWS table).
// Compiled once per precision: -DFOURIER_TU_REAL=float / double (fourier_amd/build.py).
#include "engine_common.h"
#include "kernels_stft.h"
#include "tile_shapes.h"

namespace fourier_hip {

typedef FOURIER_TU_REAL TUReal;

StftKernel get_stft_kernel(Real<TUReal>, int which) {
  typedef TUReal T;
  switch (which) {
    case STFT_FRAME: return &stft_frame_kernel<T>;
    case STFT_OLA: return &istft_ola_kernel<T>;
    default: return nullptr;
  }
}

template <typename T, int L, int CG> static StftRowsKernel make_stft_rows() {
  using C = TileCfg<T, L, CG>;
  StftRowsKernel k;
  k.fn = &stft_rows_kernel<T, L, CG>;
  k.L = L; k.CG = CG; k.NT = C::NT; k.COLS = C::COLS;
  k.smem = StftRowsCfg<T, L, CG>::SMEM;
  return k;
}

// h = L: the tile width of the whole-row kernel of that length (get_kernel, MODE_ROWS); f64 h = 1024 is a one-launch 32 x 32 plan and
// has no row kernel
StftRowsKernel get_stft_rows_kernel(Real<TUReal>, int L) {
  typedef TUReal T;
  switch (L) {
    case 64: return make_stft_rows<T, 64, 16>();
    case 128: return make_stft_rows<T, 128, FOURIER_CG_128_ROWS>();
    case 256: return make_stft_rows<T, 256, 16>();
    case 512: return make_stft_rows<T, 512, FOURIER_CG_512>();
    case 1024:
      if constexpr (sizeof(T) == 4) return make_stft_rows<T, 1024, 4>();
      return StftRowsKernel();
    default: return StftRowsKernel();
  }
}

}  // namespace fourier_hip
