// spectrogram_plan.h -- the plan behind a spectrogram handle (fourier_hip_spectrogram_*, include/fourier.h): |X|^p of the STFT's frames
// X[b, f, k] (frame-major reals, batch x frames x bins), and the Welch average scale * c_k / frames * sum_f |X[b, f, k]|^2 (batch x bins),
// without the complex frames reaching the caller.  It owns a StftPlan<T> and takes from it the framing, the window table and the real
// plan; the STFT's own routes are not touched.  Routes, the same choice for both entry points:
//   "spectrogram fused rows" / "welch fused rows"  wherever stft_rows_kernel exists: spectrogram_rows_kernel (kernels_spectrogram.h) in
//                      one launch.  The spectrogram needs no scratch.  Welch is tiled per row, ceil(frames / COLS) workgroups a row,
//                      each leaving one row of `bins` partial sums; welch_reduce_kernel sums a row's tiles in ascending order.
//   "spectrogram composed" / "welch composed"      every n_fft: per chunk of the flat frame index stft_frame_kernel gathers, pads and
//                      windows into the scratch, RealPlan::run_forward transforms into a second region of it, then
//                      spectrogram_power_kernel writes |.|^p to the output, or welch_colsum_kernel adds the chunk's |.|^2 to the slots
//                      (WELCH_TILE frames of one row each) it meets, and welch_reduce_kernel finishes.  Chunks may end inside a row.
// The default is the composed route until the fused one is measured (the constructor); option "fusion" = 1 takes the fused route
// wherever it exists, 0 the composed one.
// Scratch: the frames of a chunk take n_fft reals + bins complex each, at most the bound of FOURIER_REAL_SCRATCH_BYTES and never less than
// one frame; the partials are a buffer of their own under the same bound, never less than one row's, the rows walked in groups that fit.
// No atomics: the order of every sum is fixed by (route, shape, chunking), so equal calls give bit-equal results.
#pragma once
#include "frame_scratch.h"

namespace fourier_hip {

template <typename T> class SpectrogramPlan : public HandleBase {
 public:
  static constexpr size_t ELEM = sizeof(cpx<T>);
  static constexpr size_t LAUNCH_ITEMS = StftPlan<T>::LAUNCH_ITEMS;  // frames of one launch: 32-bit frame arithmetic in the kernels
  static constexpr size_t WELCH_TILE = 32;                           // composed Welch: frames of one row per slot of partials

  SpectrogramPlan(size_t n_fft, size_t hop, size_t win_length, int pad_mode, int device) {
    stft_.reset(new StftPlan<T>(n_fft, hop, win_length, pad_mode, device));
    device_ = stft_->real().inner().device();
    DeviceGuard g(device_);
    scratch_cap_ = frames_.cap = scratch_bound("FOURIER_REAL_SCRATCH_BYTES", REAL_SCRATCH_BYTES);
    launch_items_ = frames_.items = launch_bound("FOURIER_LAUNCH_ITEMS", LAUNCH_ITEMS);
    // Where the fused route is the default: nowhere yet.  The project's rule is that a default follows a measurement (the STFT's fused
    // route became one after tools/stft_bench.py), and tools/spectrogram_bench.py has not run on an MI355X -- DESIGN.md section 4, "Power
    // spectrogram and Welch average".  Option "fusion" = 1 selects the fused kernels wherever they exist.
    // FOURIER_SPECTROGRAM_FUSION = 0 / 1 is the development switch of the experiments library and the emulator build.
    fusion_.init(stft_->enable_spectrogram(), "FOURIER_SPECTROGRAM_FUSION", false);
    refresh_desc();
  }

  size_t n_fft() const { return stft_->n_fft(); }
  size_t hop() const { return stft_->hop(); }
  size_t win_length() const { return stft_->win_length(); }
  size_t bins() const { return stft_->bins(); }
  size_t frames(size_t length) const { return stft_->frames(length); }

  int set_option(const std::string& key, long long v) {
    if (!fusion_.set(key, v)) return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    refresh_desc();
    return ::fourier::c::FOURIER_HIP_OK;
  }

  // the STFT handle's set-up call: win_length reals T on the device, or nullptr for all ones; waits for `stream`
  void set_window(const void* d_window, hipStream_t stream) { stft_->set_window(d_window, stream); }

  // later forward and welch calls of at most `batch` rows of `length` reals never allocate (on the route selected now)
  void reserve(size_t length, size_t batch) const {
    const size_t fr = frames(length);
    if (fr == 0) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "invalid length");
    if (batch == 0) return;
    DeviceGuard g(device_);
    if (!fusion_.on) (void)prepare_frames(batch * fr);
    (void)prepare_partials(fr, batch);
  }

  void forward(const void* d_in, void* d_out, size_t length, size_t batch, int power, bool normalized, hipStream_t stream) const {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    if (power != ::fourier::c::FOURIER_SPECTROGRAM_MAGNITUDE && power != ::fourier::c::FOURIER_SPECTROGRAM_POWER)
      throw EngineError(INVALID, "power must be 1 (magnitude) or 2 (power)");
    const size_t fr = frames(length), bins = this->bins();
    if (fr == 0) throw EngineError(INVALID, "invalid length");
    check_buffers(d_in, d_out, batch * length * sizeof(T), batch * fr * bins * sizeof(T), sizeof(T), false);
    if (batch == 0) return;
    DeviceGuard g(device_);
    const size_t total = batch * fr;
    const T* in = (const T*)d_in;
    T* out = (T*)d_out;
    SpectrogramArgs a{};
    a.f = fusion_.on ? stft_->fused_args(length, fr, normalized) : stft_->frame_args(length, fr);
    a.bins = (uint32_t)bins;
    a.power = (uint32_t)power;
    if (fusion_.on) {
      for_chunks(total, launch_items_, [&](size_t g0, size_t ng) {
        stft_->fused_launch_at(a.f, in, length, fr, g0, ng);
        a.f.out = out + g0 * bins;
        stft_->real().inner().exec_frames(a, stream, power);
      });
      return;
    }
    const size_t chunk = prepare_frames(total);
    const int code = normalized ? ::fourier::c::FOURIER_TRANSFORM_SQRT_SCALED_FFT : ::fourier::c::FOURIER_TRANSFORM_FFT;
    for_chunks(total, chunk, [&](size_t g0, size_t ng) {
      transform_chunk(a, in, length, fr, g0, ng, chunk, code, stream);
      a.f.in = frames_.spectra();
      a.f.out = out + g0 * bins;
      a.count = ng * bins;
      FOURIER_LAUNCH(get_spectrogram_kernel(Real<T>{}, SPECTROGRAM_POWER_SWEEP), elementwise_grid(a.count), 256, 0, stream, a);
    });
  }

  void welch(const void* d_in, void* d_out, size_t length, size_t batch, bool fold, double scale, hipStream_t stream) const {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    const size_t fr = frames(length), bins = this->bins();
    if (fr == 0) throw EngineError(INVALID, "invalid length");
    check_buffers(d_in, d_out, batch * length * sizeof(T), batch * bins * sizeof(T), sizeof(T), false);
    if (batch == 0) return;
    DeviceGuard g(device_);
    const T* in = (const T*)d_in;
    T* out = (T*)d_out;
    const size_t tiles = tiles_of(fr);
    const size_t rows_per = prepare_partials(fr, batch);
    SpectrogramArgs a{};
    a.f = fusion_.on ? stft_->fused_args(length, fr, false) : stft_->frame_args(length, fr);
    a.bins = (uint32_t)bins;
    a.part = part_.p;
    a.tiles = (uint32_t)tiles;
    divider(a.tiles, a.tl_m, a.tl_l);
    a.tile_frames = (uint32_t)WELCH_TILE;
    a.fold = fold ? 1 : 0;
    a.scale = scale / (double)fr;
    const size_t chunk = fusion_.on ? 0 : prepare_frames(std::min(batch, rows_per) * fr);
    for_chunks(batch, rows_per, [&](size_t b0, size_t nb) {
      if (fusion_.on) {
        stft_->fused_launch_at(a.f, in + b0 * length, length, fr, 0, 0);  // (tiled per row: the kernel reads neither first nor total)
        stft_->real().inner().exec_frames(a, stream, SPEC_PARTIAL, nb * tiles);
      } else {
        for_chunks(nb * fr, chunk, [&](size_t g0, size_t ng) {
          transform_chunk(a, in + b0 * length, length, fr, g0, ng, chunk, ::fourier::c::FOURIER_TRANSFORM_FFT, stream);
          const size_t g_last = g0 + ng - 1, r0 = g0 / fr, r1 = g_last / fr;
          a.f.in = frames_.spectra();
          a.g0 = g0; a.g1 = g0 + ng;
          a.slot0 = r0 * tiles + (g0 - r0 * fr) / WELCH_TILE;
          a.count = (r1 * tiles + (g_last - r1 * fr) / WELCH_TILE - a.slot0 + 1) * bins;
          FOURIER_LAUNCH(get_spectrogram_kernel(Real<T>{}, WELCH_COLSUM), elementwise_grid(a.count), 256, 0, stream, a);
        });
      }
      a.f.out = out + b0 * bins;
      a.count = nb * bins;
      FOURIER_LAUNCH(get_spectrogram_kernel(Real<T>{}, WELCH_REDUCE), elementwise_grid(a.count), 256, 0, stream, a);
    });
  }

 private:
  void refresh_desc() {
    desc_ = std::string(fusion_.on ? "spectrogram fused rows, welch fused rows: " : "spectrogram composed, welch composed: ") + stft_->real().describe();
  }
  // partial slots per row: the fused kernel's tiles of COLS frames, the composed route's runs of WELCH_TILE frames
  size_t tiles_of(size_t fr) const {
    const size_t per = fusion_.on ? (size_t)stft_->real().inner().template frame_cols<SpectrogramArgs>() : WELCH_TILE;
    return (fr + per - 1) / per;
  }
  // rows per group of a Welch call: their partials fit the bound (never less than one row's) and one launch's 32-bit indices
  size_t prepare_partials(size_t fr, size_t batch) const {
    const size_t tiles = tiles_of(fr), row = tiles * bins() * sizeof(T);
    const size_t rows_per = std::min(chunk_rows(batch, scratch_cap_, row), std::max<size_t>(1, launch_items_ / std::max(fr, tiles * WELCH_TILE)));
    part_.ensure(rows_per * row);
    return rows_per;
  }
  // frames per chunk of the composed routes; sizes the scratch (bins complex + n_fft reals per frame) and RealPlan's buffers
  size_t prepare_frames(size_t total) const { return frames_.prepare(*stft_, total); }
  // frames g0 ... g0 + ng - 1 of the flat frame index counted from the row at `in`: gathered, windowed, transformed into frames_.spectra()
  void transform_chunk(SpectrogramArgs& a, const T* in, size_t length, size_t fr, size_t g0, size_t ng, size_t chunk, int code,
                       hipStream_t stream) const {
    frames_.transform_chunk(*stft_, a.f, in, length, fr, g0, ng, chunk, code, stream);
  }

  std::unique_ptr<StftPlan<T>> stft_;
  int device_ = 0;
  FusionSwitch fusion_;
  FrameScratch<T> frames_;  // the composed routes' scratch (frame_scratch.h)
  mutable DevBuf part_;
  size_t scratch_cap_ = REAL_SCRATCH_BYTES;
  size_t launch_items_ = LAUNCH_ITEMS;  // frames of one launch (development switch FOURIER_LAUNCH_ITEMS)
};

}  // namespace fourier_hip
