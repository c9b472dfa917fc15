// stft_plan.h -- the plan behind a short-time Fourier transform handle (fourier_hip_stft_*, include/fourier.h): torch.stft / torch.istft
// with onesided = True on batches of real rows, frame-major output (frame f of row b at complex offset (b * frames + f) * bins), built
// on RealPlan<T>.  Frames of n_fft samples every `hop` samples; the window of win_length reals sits centred in the frame; the centred
// modes pad p = n_fft / 2 samples by reflection or with zeros, by index arithmetic at the load.  Routes:
//   "stft composed"    every n_fft: stft_frame_kernel gathers, pads and windows the frames of a chunk of the flat frame index into the
//                      scratch (rows of n_fft reals), RealPlan::run_forward takes them straight into the caller's output.
//   "stft fused rows"  n_fft = 2h with a whole-row h-point kernel: stft_rows_kernel in one launch, no scratch (kernels_stft.h).  The
//                      default where the measurements at the constructor say so; option "fusion" = 0 forces the composed route, 1 takes the
//                      fused one wherever its kernel exists.
//   inverse            "istft composed" only: RealPlan::run_inverse (unscaled) takes the frames of a chunk into the scratch,
//                      istft_ola_kernel gathers the overlap-add, times the reciprocal envelope 1 / sum_f w^2.  The envelope depends on
//                      the window, hop, frames and length only: f64 on the host, cached per (frames, length); a minimum below 1e-11
//                      over the kept samples refuses the call (torch's NOLA check).  Chunks are whole rows where a row's frames fit
//                      the scratch bound, else ranges of output samples of one row; frames two neighbouring ranges both need are
//                      transformed twice.  A range needs every frame that covers one sample, so the scratch never holds fewer than
//                      ceil(n_fft / hop) frames.
#pragma once
#include <map>

#include "frame_plan_common.h"
#include "real_plan.h"

namespace fourier_hip {

template <typename T> class StftPlan : public HandleBase {
 public:
  static constexpr size_t ELEM = sizeof(cpx<T>);
  static constexpr size_t LAUNCH_ITEMS = (size_t)1 << 30;  // frames of one launch: 32-bit frame arithmetic in the kernels
  static constexpr double NOLA_MIN = 1e-11;                // torch.istft's threshold on the window envelope
  static constexpr size_t ENVELOPES = 16;                  // cached reciprocal envelopes, one per (frames, length)

  StftPlan(size_t n_fft, size_t hop, size_t win_length, int pad_mode, int device) : n_(n_fft), hop_(hop), wl_(win_length), mode_(pad_mode) {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    if (n_fft == 0 || hop == 0 || win_length == 0 || win_length > n_fft) throw EngineError(INVALID, "n_fft, hop >= 1 and 1 <= win_length <= n_fft");
    if (pad_mode != ::fourier::c::FOURIER_STFT_PAD_NONE && pad_mode != ::fourier::c::FOURIER_STFT_PAD_REFLECT &&
        pad_mode != ::fourier::c::FOURIER_STFT_PAD_ZERO)
      throw EngineError(INVALID, "unknown pad mode");
    if (n_fft > 0x7fffffffull || hop > 0x7fffffffull) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "n_fft or hop above 2^31");
    pad_ = mode_ == ::fourier::c::FOURIER_STFT_PAD_NONE ? 0 : n_ / 2;
    bins_ = n_ / 2 + 1;
    real_.reset(new RealPlan<T>(n_, device));
    device_ = real_->inner().device();
    DeviceGuard g(device_);
    scratch_cap_ = scratch_bound("FOURIER_REAL_SCRATCH_BYTES", REAL_SCRATCH_BYTES);
    launch_items_ = launch_bound("FOURIER_LAUNCH_ITEMS", LAUNCH_ITEMS);
    load_window(std::vector<T>(wl_, (T)1));
    // Where the fused route is the default: wherever its kernel exists.  Every (precision, n_fft) measured 0.31 - 0.42 of the composed
    // route's time at hop = n_fft / 4 and n_fft / 2, against a spread of 1 - 4 % ("Short-time Fourier transform";
    // profiles/stft/stft_bench.jsonl).  FOURIER_STFT_FUSION = 0 / 1 is the development switch of the experiments library and the emulator build.
    fusion_.init(real_->template enable_frames<StftArgs>(), "FOURIER_STFT_FUSION", true);
    refresh_desc();
  }

  size_t n_fft() const { return n_; }
  size_t hop() const { return hop_; }
  size_t win_length() const { return wl_; }
  size_t bins() const { return bins_; }

  // what the spectrogram handle (spectrogram_plan.h) builds its routes from: the framing, the window table and the real plan
  size_t pad() const { return pad_; }
  const void* window() const { return win_.p; }
  const RealPlan<T>& real() const { return *real_; }
  bool enable_spectrogram() { return real_->template enable_frames<SpectrogramArgs>(); }
  bool enable_csd() { return real_->template enable_frames<CsdArgs>(); }  // ... and the cross-spectrum handle (csd_plan.h)
  bool enable_bandspec() { return real_->template enable_frames<BandSpecArgs>(); }  // ... and the band-spectrogram handle (bandspec_plan.h)
  // the argument block of a forward launch, all but in, out, first, total (and the fused route's tw, scale, pairs)
  StftArgs frame_args(size_t length, size_t fr) const {
    StftArgs a{};
    a.win = win_.p;
    a.length = length; a.frames = (uint32_t)fr;
    divider(a.frames, a.fr_m, a.fr_l);
    a.n_fft = (uint32_t)n_; a.hop = (uint32_t)hop_; a.pad = (uint32_t)pad_; a.mode = (uint32_t)mode_;
    a.scale = 1.0;
    return a;
  }
  // ... of a fused launch (stft_rows_kernel, spectrogram_rows_kernel): with the untangle's table and the scale of the bins
  StftArgs fused_args(size_t length, size_t fr, bool normalized) const {
    StftArgs a = frame_args(length, fr);
    a.tw = real_->twiddles();
    a.scale = normalized ? code_scale<T>(::fourier::c::FOURIER_TRANSFORM_SQRT_SCALED_FFT, (T)n_) : 1.0;
    return a;
  }
  // ... and its row base: the fused load takes two reals per access where every interior frame starts on an even element of a
  // 2 * sizeof(T)-aligned row
  void fused_launch_at(StftArgs& a, const T* in, size_t length, size_t fr, size_t g0, size_t ng) const {
    frame_launch_at(a, in, length, fr, g0, ng);
    a.pairs = hop_ % 2 == 0 && pad_ % 2 == 0 && length % 2 == 0 && (uintptr_t)a.in % (2 * sizeof(T)) == 0;
  }
  // frames of a row of `length` reals; 0 where the length is invalid
  size_t frames(size_t length) const {
    size_t f = 0;
    if (mode_ == ::fourier::c::FOURIER_STFT_PAD_NONE) { if (length >= n_) f = 1 + (length - n_) / hop_; }
    else if (length >= 1 && (mode_ != ::fourier::c::FOURIER_STFT_PAD_REFLECT || length > pad_)) f = 1 + (length + 2 * pad_ - n_) / hop_;  // even n_fft: 1 + length / hop
    return f <= 0x7fffffffull ? f : 0;
  }

  int set_option(const std::string& key, long long v) {
    if (!fusion_.set(key, v)) return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    refresh_desc();
    return ::fourier::c::FOURIER_HIP_OK;
  }

  // win_length reals T on the device, or nullptr for all ones.  A set-up call: it waits for `stream` (the tables are replaced in place
  // and the host keeps a copy for the inverse's envelope).
  void set_window(const void* d_window, hipStream_t stream) {
    if (d_window && (uintptr_t)d_window % sizeof(T)) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "misaligned window");
    DeviceGuard g(device_);
    std::vector<T> w(wl_, (T)1);
    if (d_window) HIP_CHECK(hipMemcpyAsync(w.data(), d_window, wl_ * sizeof(T), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    load_window(w);
  }

  // later forward calls of at most `batch` rows of `length` reals, and inverse calls to that length from frames(length) frames, never allocate
  void reserve(size_t length, size_t batch) const {
    const size_t fr = frames(length);
    if (fr == 0) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "invalid length");
    if (batch == 0) return;
    DeviceGuard g(device_);
    if (!fusion_.on) (void)prepare_forward(batch * fr);
    (void)prepare_inverse(inverse_chunks(fr, batch).frames());
    const size_t full = hop_ * (fr - 1) + n_ - 2 * pad_;
    if (length <= full) {
      try { (void)envelope(fr, length); } catch (const EngineError& e) { if (e.status != ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT) throw; }  // (a window without an inverse)
    }
  }

  void forward(const void* d_in, void* d_out, size_t length, size_t batch, bool normalized, hipStream_t stream) const {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    const size_t fr = frames(length);
    if (fr == 0) throw EngineError(INVALID, "invalid length");
    check_buffers(d_in, d_out, batch * length * sizeof(T), batch * fr * bins_ * ELEM, sizeof(T), false);
    if ((uintptr_t)d_out % ELEM) throw EngineError(INVALID, "misaligned buffer");
    if (batch == 0) return;
    DeviceGuard g(device_);
    const size_t total = batch * fr;
    const T* in = (const T*)d_in;
    cpx<T>* out = (cpx<T>*)d_out;
    if (fusion_.on) {
      StftArgs a = fused_args(length, fr, normalized);
      for_chunks(total, launch_items_, [&](size_t g0, size_t ng) {
        fused_launch_at(a, in, length, fr, g0, ng);
        a.out = out + g0 * bins_;
        real_->inner().exec_frames(a, stream);
      });
      return;
    }
    StftArgs a = frame_args(length, fr);
    const size_t chunk = prepare_forward(total);
    const int code = normalized ? ::fourier::c::FOURIER_TRANSFORM_SQRT_SCALED_FFT : ::fourier::c::FOURIER_TRANSFORM_FFT;
    for_chunks(total, chunk, [&](size_t g0, size_t ng) {
      frame_launch_at(a, in, length, fr, g0, ng);
      a.out = scratch_.p;
      FOURIER_LAUNCH(get_stft_kernel(Real<T>{}, STFT_FRAME), ng, 256, 0, stream, a);
      real_->run_forward(scratch_.p, out + g0 * bins_, ng, code, stream);
    });
  }

  void inverse(const void* d_in, void* d_out, size_t fr, size_t length, size_t batch, bool normalized, hipStream_t stream) const {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    if (fr == 0 || fr > 0x7fffffffull) throw EngineError(INVALID, "invalid frame count");
    const size_t full = hop_ * (fr - 1) + n_;
    if (length == 0 || full < 2 * pad_ + length) throw EngineError(INVALID, "invalid length");
    check_buffers(d_in, d_out, batch * fr * bins_ * ELEM, batch * length * sizeof(T), sizeof(T), false);
    if ((uintptr_t)d_in % ELEM) throw EngineError(INVALID, "misaligned buffer");
    DeviceGuard g(device_);
    const void* env = envelope(fr, length);  // the NOLA refusal comes before the empty batch: it is a property of the handle and the sizes
    if (batch == 0) return;
    const cpx<T>* in = (const cpx<T>*)d_in;
    T* out = (T*)d_out;
    const FrameInverseChunks chunks = inverse_chunks(fr, batch);
    (void)prepare_inverse(chunks.frames());
    StftArgs a{};
    a.win = win_.p; a.env = env;
    a.length = length; a.frames = (uint32_t)fr;
    a.n_fft = (uint32_t)n_; a.hop = (uint32_t)hop_; a.pad = (uint32_t)pad_; a.mode = (uint32_t)mode_;
    a.scale = (normalized ? std::sqrt((double)n_) : 1.0) / (double)n_;  // the inner inverse runs unscaled
    a.in = scratch_.p;
    const int code = ::fourier::c::FOURIER_TRANSFORM_UNSCALED_IFFT;
    frame_inverse_walk(overlap(), chunks, fr, batch, length, [&](size_t b0, size_t nb, size_t t0, size_t span, size_t f_lo, size_t nfr) {
      real_->run_inverse(in + (b0 * fr + f_lo) * bins_, scratch_.p, nb == 1 ? nfr : nb * fr, code, stream);
      a.out = out + b0 * length;
      a.t0 = t0; a.span = span; a.rows = nb; a.f_lo = f_lo; a.nfr = nfr;
      a.total = nb * span;
      FOURIER_LAUNCH(get_stft_kernel(Real<T>{}, STFT_OLA), elementwise_grid(a.total), 256, 0, stream, a);
    });
  }

 private:
  void refresh_desc() {
    desc_ = std::string(fusion_.on ? "stft fused rows" : "stft composed") + ", istft composed: " + real_->describe();
  }
  // the window centred in the frame, (n_fft - win_length) / 2 zeros in front: the device table in T, the host copy in f64
  void load_window(const std::vector<T>& w) {
    std::vector<T> full(n_, (T)0);
    const size_t left = (n_ - wl_) / 2;
    for (size_t i = 0; i < wl_; ++i) full[left + i] = w[i];
    win_.upload(full);
    win_host_.assign(full.begin(), full.end());
    env_.clear();
  }
  // frames per chunk of the composed forward route; sizes the scratch and RealPlan's buffers
  size_t prepare_forward(size_t total) const {
    const size_t chunk = std::min(chunk_rows(total, scratch_cap_, n_ * sizeof(T)), launch_items_);
    scratch_.ensure(chunk * n_ * sizeof(T));
    real_->reserve(chunk);
    return chunk;
  }
  size_t prepare_inverse(size_t frames_in_scratch) const {
    scratch_.ensure(frames_in_scratch * n_ * sizeof(T));
    real_->reserve(frames_in_scratch);
    return frames_in_scratch;
  }
  // the inverse's framing and its chunks under the scratch bound (reserve() and inverse() size from the same function)
  FrameOverlap overlap() const { return {n_, hop_, pad_}; }
  FrameInverseChunks inverse_chunks(size_t fr, size_t batch) const {
    return frame_inverse_chunks(overlap(), fr, batch, scratch_cap_ / (n_ * sizeof(T)));
  }
  // 1 / sum_f w[t + p - f hop]^2, t < length, on the device; built on first use of (frames, length)
  const void* envelope(size_t fr, size_t length) const {
    const auto key = std::make_pair(fr, length);
    auto it = env_.find(key);
    if (it != env_.end()) return it->second->p;
    std::vector<T> rec(length);
    double lowest = INFINITY;
    for (size_t t = 0; t < length; ++t) {
      const size_t u = t + pad_;
      const size_t f_hi = std::min(fr - 1, u / hop_), f_lo = u >= n_ ? (u - n_) / hop_ + 1 : 0;
      double e = 0;
      for (size_t f = f_lo; f <= f_hi && f_lo <= f_hi; ++f) { const double w = win_host_[u - f * hop_]; e += w * w; }
      lowest = std::min(lowest, std::fabs(e));
      rec[t] = (T)(1.0 / e);
    }
    if (!(lowest >= NOLA_MIN)) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "window overlap-add envelope below 1e-11 (NOLA)");
    if (env_.size() >= ENVELOPES) env_.clear();  // (hipFree waits for the device: nothing in flight reads a freed table)
    std::unique_ptr<DevBuf> buf(new DevBuf());
    buf->upload(rec);
    return env_.emplace(key, std::move(buf)).first->second->p;
  }

  size_t n_, hop_, wl_;
  int mode_;
  size_t pad_ = 0, bins_ = 0;
  int device_ = 0;
  std::unique_ptr<RealPlan<T>> real_;
  FusionSwitch fusion_;
  DevBuf win_;
  std::vector<double> win_host_;
  mutable std::map<std::pair<size_t, size_t>, std::unique_ptr<DevBuf>> env_;
  mutable DevBuf scratch_;
  size_t scratch_cap_ = REAL_SCRATCH_BYTES;
  size_t launch_items_ = LAUNCH_ITEMS;  // frames of one launch (development switch FOURIER_LAUNCH_ITEMS)
};

}  // namespace fourier_hip
