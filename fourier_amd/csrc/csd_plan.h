// csd_plan.h -- the plan behind a cross-spectrum handle (fourier_hip_csd_*, include/fourier.h): of the STFT's frames X[b, f, k] of row b of
// x and Y[b, f, k] of row b of y, the cross-spectral density scale * c_k / frames * sum_f conj(X) Y (batch x bins complex values) and the
// coherence |sum_f conj(X) Y|^2 / (sum_f |X|^2 sum_f |Y|^2) (batch x bins reals) -- scipy.signal.csd / coherence without detrending --
// without a frame reaching the caller.  It owns a StftPlan<T> and takes from it the framing, the window table and the real plan, as
// SpectrogramPlan does; the STFT's own routes are not touched.  Routes, the same choice for both entry points:
//   "csd fused rows" / "coherence fused rows"  wherever stft_rows_kernel exists: csd_rows_kernel (kernels_csd.h) in one launch, tiled per
//                      row, ceil(frames / (COLS / 2)) workgroups a row, each leaving four rows of `bins` partial sums (|X|^2, |Y|^2, Re
//                      and Im of conj(X) Y); csd_reduce_kernel sums a row's tiles in ascending order and writes either result.
//   "csd composed" / "coherence composed"      every n_fft: per chunk of the flat frame index stft_frame_kernel gathers, pads and windows
//                      the chunk's x frames and y frames into the scratch, ONE RealPlan::run_forward transforms both into a second region
//                      of it, csd_colsum_kernel adds the chunk's four products to the slots (WELCH_TILE frames of one row each) it
//                      meets, and csd_reduce_kernel finishes.  Chunks may end inside a row.
// The default route follows the measurement at the constructor; option "fusion" = 1 takes the fused route wherever it exists, 0 the
// composed one.
// Scratch: a frame pair of a chunk takes 2 x (n_fft reals + bins complex), at most the bound of FOURIER_REAL_SCRATCH_BYTES and never less
// than one pair; the partials are a buffer of their own under the same bound, never less than one row's, the rows walked in groups that
// fit.  No atomics: the order of every sum is fixed by (route, shape, scratch bound) -- ascending frames inside a tile, then ascending
// tiles -- so equal calls give bit-equal results.
#pragma once
#include "stft_plan.h"

namespace fourier_hip {

template <typename T> class CsdPlan : public HandleBase {
 public:
  static constexpr size_t ELEM = sizeof(cpx<T>);
  static constexpr size_t LAUNCH_ITEMS = StftPlan<T>::LAUNCH_ITEMS;  // frames of one launch: 32-bit frame arithmetic in the kernels
  static constexpr size_t WELCH_TILE = 32;                           // composed route: frames of one row per slot of partials

  CsdPlan(size_t n_fft, size_t hop, size_t win_length, int pad_mode, int device) {
    stft_.reset(new StftPlan<T>(n_fft, hop, win_length, pad_mode, device));
    device_ = stft_->real().inner().device();
    DeviceGuard g(device_);
    scratch_cap_ = scratch_bound("FOURIER_REAL_SCRATCH_BYTES", REAL_SCRATCH_BYTES);
    launch_items_ = launch_bound("FOURIER_LAUNCH_ITEMS", LAUNCH_ITEMS);
    // Where the fused route is the default: nowhere yet.  The project's rule is that a default follows a measurement: the fused route
    // has to beat the composed one on every shape of tools/csd_bench.py by more than the spread between repetitions of one arm
    // ("Cross-spectral density and coherence").  Option "fusion" = 1 selects the fused kernel wherever it exists.
    // FOURIER_CSD_FUSION = 0 / 1 is the development switch of the experiments library and the emulator build.
    fusion_.init(stft_->enable_csd(), "FOURIER_CSD_FUSION", false);
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

  // later csd and coherence calls of at most `batch` rows of `length` reals never allocate (on the route selected now)
  void reserve(size_t length, size_t batch) const {
    const size_t fr = frames(length);
    if (fr == 0) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "invalid length");
    if (batch == 0) return;
    DeviceGuard g(device_);
    const size_t rows_per = prepare_partials(fr, batch);
    if (!fusion_.on) (void)prepare_frames(std::min(batch, rows_per) * fr);
  }

  void csd(const void* d_x, const void* d_y, void* d_out, size_t length, size_t batch, bool fold, double scale, hipStream_t stream) const {
    run(d_x, d_y, d_out, length, batch, false, fold, scale, stream);
  }
  void coherence(const void* d_x, const void* d_y, void* d_out, size_t length, size_t batch, hipStream_t stream) const {
    run(d_x, d_y, d_out, length, batch, true, false, 1.0, stream);
  }

 private:
  void run(const void* d_x, const void* d_y, void* d_out, size_t length, size_t batch, bool coherence, bool fold, double scale,
           hipStream_t stream) const {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    const size_t fr = frames(length), bins = this->bins();
    if (fr == 0) throw EngineError(INVALID, "invalid length");
    const size_t out_elem = coherence ? sizeof(T) : ELEM;
    // x and y may be one buffer; the output lies apart from both
    check_buffers(d_x, d_out, batch * length * sizeof(T), batch * bins * out_elem, sizeof(T), false);
    check_buffers(d_y, d_out, batch * length * sizeof(T), batch * bins * out_elem, sizeof(T), false);
    if ((uintptr_t)d_out % out_elem) throw EngineError(INVALID, "misaligned buffer");
    if (batch == 0) return;
    DeviceGuard g(device_);
    const T* x = (const T*)d_x;
    const T* y = (const T*)d_y;
    const size_t tiles = tiles_of(fr);
    const size_t rows_per = prepare_partials(fr, batch);
    CsdArgs a{};
    a.f = fusion_.on ? stft_->fused_args(length, fr, false) : stft_->frame_args(length, fr);
    a.bins = (uint32_t)bins;
    a.part = part_.p;
    a.tiles = (uint32_t)tiles;
    divider(a.tiles, a.tl_m, a.tl_l);
    a.tile_frames = (uint32_t)WELCH_TILE;
    a.fold = fold ? 1 : 0;
    a.coherence = coherence ? 1 : 0;
    a.scale = scale / (double)fr;
    const size_t chunk = fusion_.on ? 0 : prepare_frames(std::min(batch, rows_per) * fr);
    for_chunks(batch, rows_per, [&](size_t b0, size_t nb) {
      if (fusion_.on) {
        stft_->fused_launch_at(a.f, x + b0 * length, length, fr, 0, 0);  // (tiled per row: the kernel reads neither first nor total)
        a.in2 = y + b0 * length;
        a.f.pairs = a.f.pairs && (uintptr_t)a.in2 % (2 * sizeof(T)) == 0;
        stft_->real().inner().exec_frames(a, stream, 0, nb * tiles);
      } else {
        for_chunks(nb * fr, chunk, [&](size_t g0, size_t ng) {
          gather_chunk(a.f, x + b0 * length, length, fr, g0, ng, gathered(chunk), stream);
          gather_chunk(a.f, y + b0 * length, length, fr, g0, ng, gathered(chunk) + ng * n_fft(), stream);
          stft_->real().run_forward(gathered(chunk), spectra(), 2 * ng, ::fourier::c::FOURIER_TRANSFORM_FFT, stream);
          const size_t g_last = g0 + ng - 1, r0 = g0 / fr, r1 = g_last / fr;
          a.f.in = spectra();
          a.ystride = ng * bins;
          a.g0 = g0; a.g1 = g0 + ng;
          a.slot0 = r0 * tiles + (g0 - r0 * fr) / WELCH_TILE;
          a.count = (r1 * tiles + (g_last - r1 * fr) / WELCH_TILE - a.slot0 + 1) * bins;
          FOURIER_LAUNCH(get_csd_kernel(Real<T>{}, CSD_COLSUM), elementwise_grid(a.count), 256, 0, stream, a);
        });
      }
      a.f.out = coherence ? (void*)((T*)d_out + b0 * bins) : (void*)((cpx<T>*)d_out + b0 * bins);
      a.count = nb * bins;
      FOURIER_LAUNCH(get_csd_kernel(Real<T>{}, CSD_REDUCE), elementwise_grid(a.count), 256, 0, stream, a);
    });
  }

  void refresh_desc() {
    desc_ = std::string(fusion_.on ? "csd fused rows, coherence fused rows: " : "csd composed, coherence composed: ") + stft_->real().describe();
  }
  // partial slots per row: the fused kernel's tiles of COLS / 2 frame pairs, the composed route's runs of WELCH_TILE frames
  size_t tiles_of(size_t fr) const {
    const size_t per = fusion_.on ? (size_t)stft_->real().inner().template frame_cols<CsdArgs>() / 2 : WELCH_TILE;
    return (fr + per - 1) / per;
  }
  // rows per group of a call: their partials (four planes a slot) fit the bound (never less than one row's) and one launch's 32-bit indices
  size_t prepare_partials(size_t fr, size_t batch) const {
    const size_t tiles = tiles_of(fr), row = tiles * CSD_PLANES * bins() * sizeof(T);
    const size_t rows_per = std::min(chunk_rows(batch, scratch_cap_, row), std::max<size_t>(1, launch_items_ / std::max(fr, tiles * WELCH_TILE)));
    part_.ensure(rows_per * row);
    return rows_per;
  }
  // frame pairs per chunk of the composed route; sizes the scratch (2 x (bins complex + n_fft reals) per pair) and RealPlan's buffers
  size_t prepare_frames(size_t total) const {
    const size_t pair = 2 * (bins() * ELEM + n_fft() * sizeof(T));
    const size_t chunk = std::min(chunk_rows(total, scratch_cap_, pair), std::max<size_t>(1, launch_items_ / 2));
    scratch_.ensure(chunk * pair);
    stft_->real().reserve(2 * chunk);
    return chunk;
  }
  // the scratch of a chunk of ng pairs: the transformed frames first (X of the ng frames, then Y of them; aligned as complex values),
  // the windowed frames behind the room of a full chunk of them, in the same order
  cpx<T>* spectra() const { return (cpx<T>*)scratch_.p; }
  T* gathered(size_t chunk) const { return (T*)((cpx<T>*)scratch_.p + 2 * chunk * bins()); }
  // frames g0 ... g0 + ng - 1 of the flat frame index counted from the row at `in`: gathered and windowed into rows of n_fft reals at `to`
  void gather_chunk(const StftArgs& block, const T* in, size_t length, size_t fr, size_t g0, size_t ng, T* to, hipStream_t stream) const {
    StftArgs f = block;
    frame_launch_at(f, in, length, fr, g0, ng);
    f.out = to;
    FOURIER_LAUNCH(get_stft_kernel(Real<T>{}, STFT_FRAME), ng, 256, 0, stream, f);
  }

  std::unique_ptr<StftPlan<T>> stft_;
  int device_ = 0;
  FusionSwitch fusion_;
  mutable DevBuf scratch_, part_;
  size_t scratch_cap_ = REAL_SCRATCH_BYTES;
  size_t launch_items_ = LAUNCH_ITEMS;  // frames of one launch (development switch FOURIER_LAUNCH_ITEMS)
};

}  // namespace fourier_hip
