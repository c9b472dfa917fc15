// kernels_cepstrum.cpp -- instantiates the cepstrum kernels (kernels_cepstrum.h): the one-launch kernel on the shapes of the two-level
// plans of 2^11 ... 2^15 (f64: ... 2^14) in both modes, and the composed route's three sweeps.
// Compiled once per precision: -DFOURIER_TU_REAL=float / double (fourier_amd/build.py).
#include "engine_common.h"
#include "kernels_cepstrum.h"

namespace fourier_hip {

typedef FOURIER_TU_REAL TUReal;

// An instance is in the table only if it spills no more than hilbert_small_kernel<T, L1, L2, true> of the same shape (gfx950,
// -Rpass-analysis=kernel-resource-usage; the table of DESIGN.md section 4, "Cepstrum and minimum phase").  That leaves out the f32
// minimum-phase kernels of 2^13 (16 against 12 bytes a lane) and 2^15 (20 against 16): they exist in the experiments library only
// (get_cepstrum_spilling_kernel, kernels_experiments.cpp), and the product holds no code for them.
template <typename T> static bool cepstrum_minphase_product(int k, KernelInfo& info) {  // (a template: the branch not taken is not instantiated)
  if constexpr (sizeof(T) == 4) {
    switch (k) {
      case 11: return cepstrum_small_info<T, 64, 32, true>(k, info);
      case 12: return cepstrum_small_info<T, 64, 64, true>(k, info);
      case 14: return cepstrum_small_info<T, 128, 128, true>(k, info);
      default: return false;
    }
  } else {
    return cepstrum_small_by_length<T, true>(k, info);
  }
}

bool get_cepstrum_small_kernel(Real<TUReal>, int k, bool minphase, KernelInfo& info) {
  return minphase ? cepstrum_minphase_product<TUReal>(k, info) : cepstrum_small_by_length<TUReal, false>(k, info);
}

CepstrumKernel get_cepstrum_kernel(Real<TUReal>, int which) {
  typedef TUReal T;
  switch (which) {
    case CEPSTRUM_LOG: return &cepstrum_log_kernel<T>;
    case CEPSTRUM_FOLD: return &cepstrum_fold_kernel<T>;
    case CEPSTRUM_EXP: return &cepstrum_exp_kernel<T>;
    default: return nullptr;
  }
}

}  // namespace fourier_hip
