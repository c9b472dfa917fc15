// kernels_bandspec.cpp -- instantiates the band-energy spectrogram kernels (kernels_bandspec.h): the band sweep of the composed route and
// the fused one-launch frame route, one kernel per power, on the whole-row kernels' tile shapes (kernels_pass.cpp's MODE_ROWS table; the
// same lengths as kernels_stft.cpp).  A translation unit of its own: the spectrogram's kernels are compiled as they were.
// Compiled once per precision: -DFOURIER_TU_REAL=float / double (fourier_amd/build.py).
#include "engine_common.h"
#include "kernels_bandspec.h"
#include "tile_shapes.h"

namespace fourier_hip {

typedef FOURIER_TU_REAL TUReal;

BandSpecKernel get_bandspec_kernel(Real<TUReal>) { return &bandspec_sweep_kernel<TUReal>; }

template <typename T, int L, int CG> static BandSpecRowsKernel make_bandspec_rows() {
  BandSpecRowsKernel k = frame_rows_shape<BandSpecRowsKernel, T, L, CG>();
  k.fn[SPEC_MAGNITUDE] = &bandspec_rows_kernel<T, L, CG, SPEC_MAGNITUDE>;
  k.fn[SPEC_POWER] = &bandspec_rows_kernel<T, L, CG, SPEC_POWER>;
  return k;
}

BandSpecRowsKernel get_bandspec_rows_kernel(Real<TUReal>, int L) { FOURIER_FRAME_ROWS_TABLE(TUReal, L, make_bandspec_rows) }

}  // namespace fourier_hip
