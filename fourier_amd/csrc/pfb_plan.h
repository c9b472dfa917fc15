// pfb_plan.h -- the plan behind a polyphase filter bank handle (fourier_hip_pfb_*, include/fourier.h): the weighted-overlap-add
// channelizer on batches of complex or real rows.  P = channels, T = taps, D = hop, a prototype filter h of P * T reals:
//   frames(length) = 1 + (length - P T) / D  for length >= P T, else 0
//   u[f, n] = sum_{t < T} h[t P + n] x[f D + t P + n],  n < P        (the taps summed in the order t = 0, 1, ...)
//   X[f, k] = sum_{n < P} u[f, n] exp(-2 pi i k n / P)
// frame-major output (frame f of row b at complex offset (b * frames + f) * bins), bins = P for complex rows, P / 2 + 1 for real ones.
// No padding, no per-frame phase rotation for D != P (a frame's time origin is its first sample, as in the STFT handle), no scale: the
// prototype filter carries the gain.  Built on a Plan<T>(P) (complex rows) or a RealPlan<T>(P) (real rows).  Routes:
//   "pfb composed"    every P: pfb_fold_kernel folds the frames of a chunk of the flat frame index into the scratch (rows of P values of
//                     the input's kind), the inner plan takes them straight into the caller's output.
//   "pfb fused rows"  the inner plan is one whole-row pass with a kernel on its tile shape (complex rows: P points; real rows: P = 2h,
//                     h points): pfb_rows_kernel / pfb_real_rows_kernel in one launch, no scratch (kernels_pfb.h).  The default where
//                     the measurements at the constructor say so; option "fusion" = 0 forces the composed route, 1 takes the fused
//                     one wherever its kernel exists.
#pragma once
#include "frame_plan_common.h"
#include "real_plan.h"

namespace fourier_hip {

template <typename T> class PfbPlan : public HandleBase {
 public:
  static constexpr size_t ELEM = sizeof(cpx<T>);
  static constexpr size_t LAUNCH_ITEMS = (size_t)1 << 30;  // frames of one launch: 32-bit frame arithmetic in the kernels

  PfbPlan(size_t channels, size_t taps, size_t hop, int real_input, int device) : p_(channels), taps_(taps), hop_(hop), real_in_(real_input != 0) {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    if (channels == 0 || taps == 0 || hop == 0) throw EngineError(INVALID, "channels, taps, hop >= 1");
    if (real_input != 0 && real_input != 1) throw EngineError(INVALID, "real_input is 0 or 1");
    if (taps > 0x7fffffffull / channels || hop > 0x7fffffffull) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "channels * taps or hop above 2^31");
    span_ = p_ * taps_;
    bins_ = real_in_ ? p_ / 2 + 1 : p_;
    vs_ = real_in_ ? sizeof(T) : ELEM;
    if (real_in_) {
      real_.reset(new RealPlan<T>(p_, device));
      device_ = real_->inner().device();
    } else {
      plan_.reset(new Plan<T>(p_, device));
      device_ = plan_->device();
    }
    DeviceGuard g(device_);
    scratch_cap_ = scratch_bound("FOURIER_REAL_SCRATCH_BYTES", REAL_SCRATCH_BYTES);
    launch_items_ = launch_bound("FOURIER_LAUNCH_ITEMS", LAUNCH_ITEMS);
    filt_.upload(std::vector<T>(span_, (T)1));
    // Where the fused route is the default: wherever its kernel exists.  Every measured shape of every (precision, input kind) -- P 256
    // and 1024, T 4 and 8, D = P and 3 P / 4, 64 rows of 2^20 values -- took 0.46 - 0.67 of the composed route's time (f64 complex rows,
    // P = 256 only: 0.74 - 0.88), the gap beyond the larger max - min of the two arms on all 28 lines ("Polyphase
    // filter bank"; profiles/pfb/pfb_bench.jsonl).  FOURIER_PFB_FUSION = 0 / 1 is the development switch of the experiments library
    // and the emulator build.
    const bool have = real_in_ ? real_->template enable_frames<PfbArgs>() : plan_->template enable_frames<PfbArgs>();
    fusion_.init(have, "FOURIER_PFB_FUSION", true);
    refresh_desc();
  }

  size_t channels() const { return p_; }
  size_t taps() const { return taps_; }
  size_t hop() const { return hop_; }
  size_t bins() const { return bins_; }
  // frames of a row of `length` values; 0 where the length is invalid
  size_t frames(size_t length) const {
    const size_t f = length >= span_ ? 1 + (length - span_) / hop_ : 0;
    return f <= 0x7fffffffull ? f : 0;
  }

  int set_option(const std::string& key, long long v) {
    if (!fusion_.set(key, v)) return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    refresh_desc();
    return ::fourier::c::FOURIER_HIP_OK;
  }

  // channels * taps reals T on the device, or nullptr for all ones.  A set-up call: it waits for `stream` (the table is replaced in place).
  void set_filter(const void* d_filter, hipStream_t stream) {
    if (d_filter && (uintptr_t)d_filter % sizeof(T)) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "misaligned filter");
    DeviceGuard g(device_);
    std::vector<T> h(span_, (T)1);
    if (d_filter) HIP_CHECK(hipMemcpyAsync(h.data(), d_filter, span_ * sizeof(T), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    filt_.upload(h);
  }

  // later forward calls of at most `batch` rows of `length` values never allocate
  void reserve(size_t length, size_t batch) const {
    const size_t fr = frames(length);
    if (fr == 0) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "invalid length");
    if (batch == 0) return;
    DeviceGuard g(device_);
    if (!fusion_.on) (void)prepare(batch * fr);
  }

  void forward(const void* d_in, void* d_out, size_t length, size_t batch, hipStream_t stream) const {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    const size_t fr = frames(length);
    if (fr == 0) throw EngineError(INVALID, "invalid length");
    check_buffers(d_in, d_out, batch * length * vs_, batch * fr * bins_ * ELEM, vs_, false);
    if ((uintptr_t)d_out % ELEM) throw EngineError(INVALID, "misaligned buffer");
    if (batch == 0) return;
    DeviceGuard g(device_);
    const size_t total = batch * fr;
    cpx<T>* out = (cpx<T>*)d_out;
    PfbArgs a{};
    a.filt = filt_.p;
    a.length = length; a.frames = (uint32_t)fr;
    divider(a.frames, a.fr_m, a.fr_l);
    a.channels = (uint32_t)p_; a.taps = (uint32_t)taps_; a.hop = (uint32_t)hop_;
    a.real = real_in_;
    if (fusion_.on) {
      const Plan<T>& inner = real_in_ ? real_->inner() : *plan_;
      if (real_in_) a.tw = real_->twiddles();
      for_chunks(total, launch_items_, [&](size_t g0, size_t ng) {
        launch_at(a, d_in, length, fr, g0, ng);
        // the real rows' load takes two reals per access where every frame starts on an even element of a 2 * sizeof(T)-aligned row
        a.pairs = real_in_ && hop_ % 2 == 0 && length % 2 == 0 && (uintptr_t)a.in % (2 * sizeof(T)) == 0;
        a.out = out + g0 * bins_;
        inner.exec_frames(a, stream, real_in_ ? 1 : 0);
      });
      return;
    }
    const size_t chunk = prepare(total);
    for_chunks(total, chunk, [&](size_t g0, size_t ng) {
      launch_at(a, d_in, length, fr, g0, ng);
      a.out = scratch_.p;
      FOURIER_LAUNCH(get_pfb_kernel(Real<T>{}), ng, 256, 0, stream, a);
      if (real_in_) real_->run_forward(scratch_.p, out + g0 * bins_, ng, ::fourier::c::FOURIER_TRANSFORM_FFT, stream);
      else plan_->exec(scratch_.p, out + g0 * bins_, ng, ::fourier::c::FOURIER_TRANSFORM_FFT, stream);
    });
  }

 private:
  void refresh_desc() {
    desc_ = std::string(fusion_.on ? "pfb fused rows: " : "pfb composed: ") + (real_in_ ? real_->describe() : plan_->describe());
  }
  // the row base of a launch over the flat frame index, by the input's kind
  void launch_at(PfbArgs& a, const void* d_in, size_t length, size_t fr, size_t g0, size_t ng) const {
    if (real_in_) frame_launch_at(a, (const T*)d_in, length, fr, g0, ng);
    else frame_launch_at(a, (const cpx<T>*)d_in, length, fr, g0, ng);
  }
  // frames per chunk of the composed route; sizes the scratch and the inner plan's buffers
  size_t prepare(size_t total) const {
    const size_t chunk = std::min(chunk_rows(total, scratch_cap_, p_ * vs_), launch_items_);
    scratch_.ensure(chunk * p_ * vs_);
    if (real_in_) real_->reserve(chunk);
    else plan_->reserve_for(chunk, false);
    return chunk;
  }

  size_t p_, taps_, hop_;
  bool real_in_;
  size_t span_ = 0, bins_ = 0, vs_ = 0;
  int device_ = 0;
  std::unique_ptr<Plan<T>> plan_;      // complex rows: the P-point plan
  std::unique_ptr<RealPlan<T>> real_;  // real rows: the real-input plan of P points
  FusionSwitch fusion_;
  DevBuf filt_;
  mutable DevBuf scratch_;
  size_t scratch_cap_ = REAL_SCRATCH_BYTES;
  size_t launch_items_ = LAUNCH_ITEMS;  // frames of one launch (development switch FOURIER_LAUNCH_ITEMS)
};

}  // namespace fourier_hip
