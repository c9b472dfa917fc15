// kernels_spectrogram.cpp -- instantiates the spectrogram and Welch kernels (kernels_spectrogram.h): the sweeps of the composed routes and
// the final reduction, and the fused one-launch frame route, three epilogues each, on the whole-row kernels' tile shapes
// (kernels_pass.cpp's MODE_ROWS table; the same lengths as kernels_stft.cpp).
// Compiled once per precision: -DFOURIER_TU_REAL=float / double (fourier_amd/build.py).
#include "engine_common.h"
#include "kernels_spectrogram.h"
#include "tile_shapes.h"

namespace fourier_hip {

typedef FOURIER_TU_REAL TUReal;

SpectrogramKernel get_spectrogram_kernel(Real<TUReal>, int which) {
  typedef TUReal T;
  switch (which) {
    case SPECTROGRAM_POWER_SWEEP: return &spectrogram_power_kernel<T>;
    case WELCH_COLSUM: return &welch_colsum_kernel<T>;
    case WELCH_REDUCE: return &welch_reduce_kernel<T>;
    default: return nullptr;
  }
}

template <typename T, int L, int CG> static SpectrogramRowsKernel make_spectrogram_rows() {
  using C = TileCfg<T, L, CG>;
  SpectrogramRowsKernel k;
  k.fn[SPEC_MAGNITUDE] = &spectrogram_rows_kernel<T, L, CG, SPEC_MAGNITUDE>;
  k.fn[SPEC_POWER] = &spectrogram_rows_kernel<T, L, CG, SPEC_POWER>;
  k.fn[SPEC_PARTIAL] = &spectrogram_rows_kernel<T, L, CG, SPEC_PARTIAL>;
  k.L = L; k.CG = CG; k.NT = C::NT; k.COLS = C::COLS;
  k.smem = StftRowsCfg<T, L, CG>::SMEM;
  return k;
}

// h = L: the tile width of the whole-row kernel of that length (get_kernel, MODE_ROWS); f64 h = 1024 is a one-launch 32 x 32 plan and
// has no row kernel
SpectrogramRowsKernel get_spectrogram_rows_kernel(Real<TUReal>, int L) {
  typedef TUReal T;
  switch (L) {
    case 64: return make_spectrogram_rows<T, 64, 16>();
    case 128: return make_spectrogram_rows<T, 128, FOURIER_CG_128_ROWS>();
    case 256: return make_spectrogram_rows<T, 256, 16>();
    case 512: return make_spectrogram_rows<T, 512, FOURIER_CG_512>();
    case 1024:
      if constexpr (sizeof(T) == 4) return make_spectrogram_rows<T, 1024, 4>();
      return SpectrogramRowsKernel();
    default: return SpectrogramRowsKernel();
  }
}

}  // namespace fourier_hip
