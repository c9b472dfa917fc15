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
  StftRowsKernel k = frame_rows_shape<StftRowsKernel, T, L, CG>();
  k.fn[0] = &stft_rows_kernel<T, L, CG>;
  return k;
}

StftRowsKernel get_stft_rows_kernel(Real<TUReal>, int L) { FOURIER_FRAME_ROWS_TABLE(TUReal, L, make_stft_rows) }

}  // namespace fourier_hip
