// kernels_mdct.cpp -- instantiates the modified discrete cosine transform kernels (kernels_mdct.h): the sweeps of the composed and
// full-length routes, and the fused one-launch frame route on the whole-row kernels' tile shapes (kernels_pass.cpp's MODE_ROWS table).
// Compiled once per precision: -DFOURIER_TU_REAL=float / double (fourier_amd/build.py).
#include "engine_common.h"
#include "kernels_mdct.h"
#include "tile_shapes.h"

namespace fourier_hip {

typedef FOURIER_TU_REAL TUReal;

MdctKernel get_mdct_kernel(Real<TUReal>, int which) {
  typedef TUReal T;
  switch (which) {
    case MDCT_FOLD: return &mdct_fold_kernel<T>;
    case MDCT_POST: return &mdct_post_kernel<T>;
    case MDCT_ODD_PRE: return &mdct_odd_pre_kernel<T>;
    case MDCT_ODD_POST: return &mdct_odd_post_kernel<T>;
    case IMDCT_PRE: return &imdct_pre_kernel<T>;
    case IMDCT_ODD_PRE: return &imdct_odd_pre_kernel<T>;
    case IMDCT_OLA: return &imdct_ola_kernel<T>;
    case IMDCT_ODD_OLA: return &imdct_odd_ola_kernel<T>;
    default: return nullptr;
  }
}

template <typename T, int L, int CG> static MdctRowsKernel make_mdct_rows() {
  MdctRowsKernel k = frame_rows_shape<MdctRowsKernel, T, L, CG>();
  k.fn[0] = &mdct_rows_kernel<T, L, CG>;
  return k;
}

MdctRowsKernel get_mdct_rows_kernel(Real<TUReal>, int L) { FOURIER_FRAME_ROWS_TABLE(TUReal, L, make_mdct_rows) }

}  // namespace fourier_hip
