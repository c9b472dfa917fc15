// kernels_frames.h -- what the fused one-launch frame kernels share: stft_rows_kernel (kernels_stft.h), spectrogram_rows_kernel
// (kernels_spectrogram.h) and mdct_rows_kernel (kernels_mdct.h).  Each of them takes COLS consecutive frames of the flat frame index into
// the register tile of a whole-row kernel (tile_core in MODE_ROWS, kernels_pass.h), runs the row core and leaves through LDS half a tile
// at a time.
//   FrameRowsCfg          the staging area of a tile shape, frame_rows_shape its launch shape for the host
//   frame_of              the flat frame index -> (row, frame in the row), for the sweeps and the rows kernels alike
// The gather, the untangle and the half-tile staging loop stay spelled out in the three kernels: composed of shared __forceinline__
// pieces with functors for the frame locator and the epilogue, the compiler allocated registers and spills differently at most shapes
// (DESIGN.md section 4 holds the tables those kernels are kept to).
#pragma once
#include "kernels_pass.h"
#include "kernels_real.h"

FOURIER_KERNELS_BEGIN

template <typename T, int L, int CG> struct FrameRowsCfg {
  using C = TileCfg<T, L, CG>;
  static constexpr int HALF = C::COLS / 2;   // frames staged at a time: v = 0 / v = 1 (f32), cg below / above CG / 2 (f64)
  static constexpr int LP = C::STAGE_LP;     // the staged frames' pitch in complex values: L of them (n = 2L reals) and the pad
  static constexpr size_t STAGE_BYTES = (size_t)HALF * LP * sizeof(cpx<T>);
  static constexpr size_t SMEM = C::EXCH_BYTES > STAGE_BYTES ? C::EXCH_BYTES : STAGE_BYTES;
};
// host: the launch shape of a rows kernel on that tile, into a descriptor K (FrameRowsKernel, engine_common.h)
template <typename K, typename T, int L, int CG> K frame_rows_shape() {
  K k;
  k.L = L; k.CG = CG; k.NT = TileCfg<T, L, CG>::NT; k.COLS = TileCfg<T, L, CG>::COLS;
  k.smem = FrameRowsCfg<T, L, CG>::SMEM;
  return k;
}

// item i of a launch (StftArgs, MdctArgs): frame x = a.first + i of the flat frame index row * frames + f
template <typename Args> __device__ __forceinline__ void frame_of(const Args& a, uint32_t i, uint32_t& row, uint32_t& f) {
  const uint32_t x = a.first + i;
  row = real_div(x, a.fr_m, a.fr_l);
  f = x - row * a.frames;
}

FOURIER_KERNELS_END
