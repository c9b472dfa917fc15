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
  using C = TileCfg<T, L, CG>;
  MdctRowsKernel k;
  k.fn = &mdct_rows_kernel<T, L, CG>;
  k.L = L; k.CG = CG; k.NT = C::NT; k.COLS = C::COLS;
  k.smem = MdctRowsCfg<T, L, CG>::SMEM;
  return k;
}

// h = L: the tile width of the whole-row kernel of that length (get_kernel, MODE_ROWS); f64 h = 1024 is a one-launch 32 x 32 plan and
// has no row kernel
MdctRowsKernel get_mdct_rows_kernel(Real<TUReal>, int L) {
  typedef TUReal T;
  switch (L) {
    case 64: return make_mdct_rows<T, 64, 16>();
    case 128: return make_mdct_rows<T, 128, FOURIER_CG_128_ROWS>();
    case 256: return make_mdct_rows<T, 256, 16>();
    case 512: return make_mdct_rows<T, 512, FOURIER_CG_512>();
    case 1024:
      if constexpr (sizeof(T) == 4) return make_mdct_rows<T, 1024, 4>();
      return MdctRowsKernel();
    default: return MdctRowsKernel();
  }
}

}  // namespace fourier_hip
