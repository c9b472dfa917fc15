// kernels_csd.cpp -- instantiates the cross-spectral density and coherence kernels (kernels_csd.h): the column-sum sweep of the composed
// route, the final reduction, and the fused one-launch frame route on the whole-row kernels' tile shapes (kernels_pass.cpp's MODE_ROWS
// table; the same lengths as kernels_stft.cpp).
// Compiled once per precision: -DFOURIER_TU_REAL=float / double (fourier_amd/build.py).
#include "engine_common.h"
#include "kernels_csd.h"
#include "tile_shapes.h"

namespace fourier_hip {

typedef FOURIER_TU_REAL TUReal;

CsdKernel get_csd_kernel(Real<TUReal>, int which) {
  typedef TUReal T;
  switch (which) {
    case CSD_COLSUM: return &csd_colsum_kernel<T>;
    case CSD_REDUCE: return &csd_reduce_kernel<T>;
    default: return nullptr;
  }
}

template <typename T, int L, int CG> static CsdRowsKernel make_csd_rows() {
  CsdRowsKernel k = frame_rows_shape<CsdRowsKernel, T, L, CG>();
  k.fn[0] = &csd_rows_kernel<T, L, CG>;
  return k;
}

CsdRowsKernel get_csd_rows_kernel(Real<TUReal>, int L) { FOURIER_FRAME_ROWS_TABLE(TUReal, L, make_csd_rows) }

}  // namespace fourier_hip
