// ipfb_plan.h -- the plan behind a polyphase synthesis filter bank handle (fourier_hip_ipfb_*, include/fourier.h): the weighted
// overlap-add that mirrors the channelizer (pfb_plan.h) on batches of frames.  P = channels, T = taps, D = hop, a synthesis filter g of
// P * T reals; the input is batch x frames x bins complex values, frame-major, what PfbPlan::forward writes (bins = P for complex output
// rows, P / 2 + 1 for real ones):
//   full(frames) = (frames - 1) D + P T
//   v[f, n] = 1/P sum_k Y[f, k] exp(+2 pi i k n / P),  n < P       (real rows: the half spectrum's inverse, numpy's irfft(Y, n = P))
//   y[t]    = sum over the frames f with 0 <= t - f D < P T, in ascending f, of g[t - f D] v[f, (t - f D) mod P],   t < length <= full
// A sample no frame covers (D > P T) is 0.  No envelope division, no NOLA check, no per-frame phase rotation: reconstruction is a
// property of the pair (h, g) (include/fourier.h has the identity).  Built on a Plan<T>(P) (complex rows) or a RealPlan<T>(P) (real rows).
// One route, "ipfb composed": the inner inverse, unscaled, takes the frames of a chunk from the caller's input into the scratch (rows of
// P values of the output's kind), ipfb_gather_kernel (kernels_pfb.h) gathers the chunk's samples with the 1/P folded in.  Chunks are
// whole rows where a row's frames fit the scratch bound, else ranges of output samples of one row (frame_plan_common.h); the gather sums
// in ascending f whatever the chunking, so a bounded handle's output is bit-equal to an unbounded one's.
#pragma once
#include "frame_plan_common.h"
#include "real_plan.h"

namespace fourier_hip {

template <typename T> class IpfbPlan : public HandleBase {
 public:
  static constexpr size_t ELEM = sizeof(cpx<T>);
  static constexpr size_t LAUNCH_ITEMS = (size_t)1 << 30;  // samples of a row, and lanes, of one gather launch: 32-bit arithmetic in the kernel

  IpfbPlan(size_t channels, size_t taps, size_t hop, int real_output, int device) : p_(channels), taps_(taps), hop_(hop), real_out_(real_output != 0) {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    if (channels == 0 || taps == 0 || hop == 0) throw EngineError(INVALID, "channels, taps, hop >= 1");
    if (real_output != 0 && real_output != 1) throw EngineError(INVALID, "real_output is 0 or 1");
    if (taps > 0x7fffffffull / channels || hop > 0x7fffffffull) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "channels * taps or hop above 2^31");
    span_ = p_ * taps_;
    bins_ = real_out_ ? p_ / 2 + 1 : p_;
    vs_ = real_out_ ? sizeof(T) : ELEM;
    if (real_out_) {
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
    desc_ = std::string("ipfb composed: ") + (real_out_ ? real_->describe() : plan_->describe());
  }

  size_t channels() const { return p_; }
  size_t taps() const { return taps_; }
  size_t hop() const { return hop_; }
  size_t bins() const { return bins_; }
  // full(frames) = (frames - 1) D + P T; 0 where the frame count is invalid.  (Frames, hop and P T are all below 2^31: the result is
  // below 2^63, it always fits.)
  size_t length(size_t fr) const { return fr == 0 || fr > 0x7fffffffull ? 0 : (fr - 1) * hop_ + span_; }

  // channels * taps reals T on the device, or nullptr for all ones.  A set-up call: it waits for `stream` (the table is replaced in place).
  void set_filter(const void* d_filter, hipStream_t stream) {
    if (d_filter && (uintptr_t)d_filter % sizeof(T)) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "misaligned filter");
    DeviceGuard g(device_);
    std::vector<T> f(span_, (T)1);
    if (d_filter) HIP_CHECK(hipMemcpyAsync(f.data(), d_filter, span_ * sizeof(T), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    filt_.upload(f);
  }

  // later inverse calls from at most `fr` frames and `batch` rows never allocate.  What a call holds in the scratch does not grow with
  // its frame count (whole rows: floor(fit / fr') * fr' frames, more for some fr' < fr), so the reservation is the most any such call
  // can hold: all its frames, batch * fr, where they fit the bound, else the bound -- or cover() frames where that is more.
  void reserve(size_t fr, size_t batch) const {
    if (length(fr) == 0) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "invalid frame count");
    if (batch == 0) return;
    DeviceGuard g(device_);
    const size_t all = batch > SIZE_MAX / fr ? SIZE_MAX : batch * fr;
    prepare(std::min(all, std::max(fit(), overlap().cover())));
  }

  void inverse(const void* d_in, void* d_out, size_t fr, size_t length_out, size_t batch, hipStream_t stream) const {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    const size_t full = length(fr);
    if (full == 0) throw EngineError(INVALID, "invalid frame count");
    if (length_out == 0 || length_out > full) throw EngineError(INVALID, "invalid length");
    check_buffers(d_in, d_out, batch * fr * bins_ * ELEM, batch * length_out * vs_, vs_, false);
    if ((uintptr_t)d_in % ELEM) throw EngineError(INVALID, "misaligned buffer");
    if (batch == 0) return;
    DeviceGuard g(device_);
    const cpx<T>* in = (const cpx<T>*)d_in;
    const FrameInverseChunks chunks = inverse_chunks(fr, batch);
    prepare(chunks.frames());
    IpfbArgs a{};
    a.in = scratch_.p; a.filt = filt_.p;
    a.length = length_out;
    a.channels = (uint32_t)p_; a.span_pt = (uint32_t)span_; a.hop = (uint32_t)hop_; a.hop_mod = (uint32_t)(hop_ % p_);
    divider(a.hop, a.hop_m, a.hop_l);
    divider(a.channels, a.ch_m, a.ch_l);
    a.real = real_out_;
    a.scale = (double)((T)1 / (T)p_);  // the inner inverse runs unscaled
    const int code = ::fourier::c::FOURIER_TRANSFORM_UNSCALED_IFFT;
    frame_inverse_walk(overlap(), chunks, fr, batch, length_out, [&](size_t b0, size_t nb, size_t t0, size_t span, size_t f_lo, size_t nfr) {
      const size_t count = nb == 1 ? nfr : nb * fr;
      if (real_out_) real_->run_inverse(in + (b0 * fr + f_lo) * bins_, scratch_.p, count, code, stream);
      else plan_->exec(in + (b0 * fr + f_lo) * bins_, scratch_.p, count, code, stream);
      a.nfr = nfr;
      gather(a, (char*)d_out + b0 * length_out * vs_, nb, t0, span, f_lo, nfr, stream);
    });
  }

 private:
  // the gather launches of a chunk: samples t0 ... t0 + span - 1 of nb rows from the frames f_lo ... f_lo + nfr - 1 in the scratch, in
  // pieces of at most LAUNCH_ITEMS samples of a row and LAUNCH_ITEMS lanes
  void gather(IpfbArgs& a, char* out, size_t nb, size_t t0, size_t span, size_t f_lo, size_t nfr, hipStream_t stream) const {
    for_chunks(span, launch_items_, [&](size_t s0, size_t ns) {
      const size_t t = t0 + s0;
      // fb: the first frame that does not end before t, among those in the scratch
      const size_t fb = std::min(std::max(f_lo, t >= span_ ? (t - span_) / hop_ + 1 : 0), f_lo + nfr - 1);
      a.t0 = t;
      a.e0 = (long long)t - (long long)(fb * hop_);
      a.q0 = (uint32_t)(fb - f_lo);
      a.kcount = (uint32_t)(nfr - (fb - f_lo));
      a.span = (uint32_t)ns;
      for_chunks(nb, std::max<size_t>(1, launch_items_ / ns), [&](size_t r0, size_t nr) {
        a.in = (const char*)scratch_.p + r0 * nfr * p_ * vs_;
        a.out = out + r0 * a.length * vs_;
        // two reals per store where every row of the launch starts its range on a 2 * sizeof(T)-aligned address
        a.pairs = real_out_ && ((uintptr_t)a.out + t * sizeof(T)) % (2 * sizeof(T)) == 0 && (nr == 1 || a.length % 2 == 0);
        a.items = (uint32_t)(a.pairs ? (ns + 1) / 2 : ns);
        divider(a.items, a.it_m, a.it_l);
        a.total = (uint32_t)(nr * a.items);
        FOURIER_LAUNCH(get_ipfb_kernel(Real<T>{}), (a.total + 255) / 256, 256, 0, stream, a);
      });
    });
  }
  // sizes the scratch and the inner plan's buffers for that many frames
  void prepare(size_t frames_in_scratch) const {
    scratch_.ensure(frames_in_scratch * p_ * vs_);
    if (real_out_) real_->reserve(frames_in_scratch);
    else plan_->reserve_for(frames_in_scratch, false);
  }
  // the framing and its chunks under the scratch bound (reserve() bounds what inverse() sizes from the same figures); a frame occupies
  // P values of the scratch
  FrameOverlap overlap() const { return {span_, hop_, 0}; }
  size_t fit() const { return scratch_cap_ / (p_ * vs_); }  // frames the bound holds
  FrameInverseChunks inverse_chunks(size_t fr, size_t batch) const { return frame_inverse_chunks(overlap(), fr, batch, fit()); }

  size_t p_, taps_, hop_;
  bool real_out_;
  size_t span_ = 0, bins_ = 0, vs_ = 0;
  int device_ = 0;
  std::unique_ptr<Plan<T>> plan_;      // complex rows: the P-point plan
  std::unique_ptr<RealPlan<T>> real_;  // real rows: the real-input plan of P points
  DevBuf filt_;
  mutable DevBuf scratch_;
  size_t scratch_cap_ = REAL_SCRATCH_BYTES;
  size_t launch_items_ = LAUNCH_ITEMS;  // samples of a row, and lanes, of one launch (development switch FOURIER_LAUNCH_ITEMS)
};

}  // namespace fourier_hip
