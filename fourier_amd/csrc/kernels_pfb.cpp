// kernels_pfb.cpp -- instantiates the polyphase filter bank kernels (kernels_pfb.h): the fold sweep of the composed route, and the fused
// one-launch frame routes for complex and real rows on the whole-row kernels' tile shapes (kernels_pass.cpp's MODE_ROWS table); the synthesis
// bank's overlap-add gather.
// Compiled once per precision: -DFOURIER_TU_REAL=float / double (fourier_amd/build.py).
#include "engine_common.h"
#include "kernels_pfb.h"
#include "tile_shapes.h"

namespace fourier_hip {

typedef FOURIER_TU_REAL TUReal;

PfbKernel get_pfb_kernel(Real<TUReal>) { return &pfb_fold_kernel<TUReal>; }
IpfbKernel get_ipfb_kernel(Real<TUReal>) { return &ipfb_gather_kernel<TUReal>; }

template <typename T, int L, int CG> static PfbRowsKernel make_pfb_rows() {
  PfbRowsKernel k = frame_rows_shape<PfbRowsKernel, T, L, CG>();
  k.fn[0] = &pfb_rows_kernel<T, L, CG>;
  k.fn[1] = &pfb_real_rows_kernel<T, L, CG>;
  return k;
}

PfbRowsKernel get_pfb_rows_kernel(Real<TUReal>, int L) { FOURIER_FRAME_ROWS_TABLE(TUReal, L, make_pfb_rows) }

}  // namespace fourier_hip
