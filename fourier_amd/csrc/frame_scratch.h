// frame_scratch.h -- the composed walk the handles on top of the STFT share (SpectrogramPlan, BandSpecPlan): a chunk of the flat frame
// index is gathered, padded and windowed by stft_frame_kernel into a handle-owned scratch, RealPlan::run_forward transforms it into a
// second region of the same scratch, and the handle's own sweep reads the spectra from there.  A frame takes n_fft reals + bins complex
// values; a chunk holds at most `cap` bytes of them, never less than one frame, and at most one launch's frames.
#pragma once
#include "stft_plan.h"

namespace fourier_hip {

template <typename T> struct FrameScratch {
  static constexpr size_t ELEM = sizeof(cpx<T>);
  mutable DevBuf buf;
  size_t cap = REAL_SCRATCH_BYTES;
  size_t items = StftPlan<T>::LAUNCH_ITEMS;  // frames of one launch (the owner sets it with cap)

  // frames per chunk for `total` frames; sizes the scratch and RealPlan's buffers
  size_t prepare(const StftPlan<T>& stft, size_t total) const {
    const size_t frame = stft.bins() * ELEM + stft.n_fft() * sizeof(T);
    const size_t chunk = std::min(chunk_rows(total, cap, frame), items);
    buf.ensure(chunk * frame);
    stft.real().reserve(chunk);
    return chunk;
  }
  // the scratch of a chunk: the transformed frames first (aligned as complex values), the windowed frames behind them
  cpx<T>* spectra() const { return (cpx<T>*)buf.p; }
  T* gathered(const StftPlan<T>& stft, size_t chunk) const { return (T*)((cpx<T>*)buf.p + chunk * stft.bins()); }
  // frames g0 ... g0 + ng - 1 of the flat frame index counted from the row at `in`: gathered, windowed, transformed into spectra();
  // `block` is StftPlan::frame_args of the call
  void transform_chunk(const StftPlan<T>& stft, const StftArgs& block, const T* in, size_t length, size_t fr, size_t g0, size_t ng,
                       size_t chunk, int code, hipStream_t stream) const {
    StftArgs f = block;
    frame_launch_at(f, in, length, fr, g0, ng);
    f.out = gathered(stft, chunk);
    FOURIER_LAUNCH(get_stft_kernel(Real<T>{}, STFT_FRAME), ng, 256, 0, stream, f);
    stft.real().run_forward(gathered(stft, chunk), spectra(), ng, code, stream);
  }
};

}  // namespace fourier_hip
