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
  SpectrogramRowsKernel k = frame_rows_shape<SpectrogramRowsKernel, T, L, CG>();
  k.fn[SPEC_MAGNITUDE] = &spectrogram_rows_kernel<T, L, CG, SPEC_MAGNITUDE>;
  k.fn[SPEC_POWER] = &spectrogram_rows_kernel<T, L, CG, SPEC_POWER>;
  k.fn[SPEC_PARTIAL] = &spectrogram_rows_kernel<T, L, CG, SPEC_PARTIAL>;
  return k;
}

SpectrogramRowsKernel get_spectrogram_rows_kernel(Real<TUReal>, int L) { FOURIER_FRAME_ROWS_TABLE(TUReal, L, make_spectrogram_rows) }

}  // namespace fourier_hip
