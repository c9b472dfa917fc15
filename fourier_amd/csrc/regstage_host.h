// regstage_host.h -- host side of the instantiation units of the register-stage kernels (kernels_chirpz.cpp, kernels_regfft.cpp): the
// ChirpzKernel record (engine_common.h) of a kernel, filled from its configuration struct C (kernels_chirpz.h, kernels_regfft.h).
#pragma once
#include "engine_common.h"

namespace fourier_hip {

// R3 == 0, two stages: a workgroup is one wave of C::TPW transforms; three stages: C::NT threads, C::NV transforms
template <typename C, uint32_t R1, uint32_t R2, uint32_t R3> static ChirpzKernel regstage_kernel_record(ChirpzKernelFn fn, bool split = false, bool fact = false) {
  ChirpzKernel k;
  k.fn = fn; k.m = C::M; k.r1 = R1; k.r2 = R2; k.r3 = R3; k.smem = C::SMEM; k.split = split; k.fact = fact;
  if constexpr (R3 == 0) { k.tpw = C::TPW; } else { k.tpw = C::NV; k.threads = C::NT; }
  return k;
}

}  // namespace fourier_hip
