// delay_plan.h -- the plan behind a delay handle (fourier_hip_delay_*, include/fourier.h): batched rows of n values, zero-extended to a
// transform length L >= n, are delayed by d[r] samples each (any finite real, one per input row, on the device), optionally weighted
// by w[r], and summed over groups of C consecutive rows (C = `channels`; C = 1: the plain fractional delay):
//   Y[g, k] = sum_{c < C, ascending} w[gC + c] X[gC + c, k] m(k, d[gC + c]),   out[g, t] = ifft(Y[g])[t],  t < n,
//   m(k, d) = exp(-2 pi i k' d / L),  k' = k below L/2 and k - L above;  m(L/2, d) = cos(pi d)  (even L).
// A positive d delays (out[t] = x[t - d]), circularly over L.  Real rows give real output, complex rows complex output.  The channel
// sum happens on the spectra: a group costs C forward transforms and ONE inverse.  Built on a complex Plan<T>(L) and a RealPlan<T>(L)
// that run unchanged.  Routes, chosen at create:
//   "delay one-launch"  real rows, C = 1, L a one-launch two-level length with a kernel (2^11 ... 2^15, f64 ... 2^14;
//                       kernels_delay.cpp): load, FFT, the phase, inverse FFT, store of the first n in ONE launch on register-resident
//                       data (delay_small_kernel, Plan::exec_delay); no scratch; in place allowed
//   "delay composed"    any L, any C.  Real rows: each row padded to L (xcorr_pad_kernel; skipped where n == L and the rows are
//                       aligned for the transform), RealPlan forward -> half spectra of L/2 + 1 values, delay_mul_kernel -> Y / L, one
//                       row a group, RealPlan unscaled inverse -> the caller's output where n == L and it is aligned for that, else
//                       scratch and xcorr_window_kernel.  Complex rows: the same with Plan<T>(L) on whole spectra, the inverse in place.
// Option "fusion" = 1 (the default, by the measurements at the constructor) selects the one-launch route where it exists, 0 the
// composed route.  The
// batch is walked in chunks of WHOLE groups so that the plan-owned scratch stays bounded (never less than one group); no atomics: the
// result is the same on repetition and under any scratch bound (up to the inner transforms' own dependence on a row's position in its
// launch: at f32 their last bits differ between even and odd rows, DESIGN.md section 4, "Cross-correlation").
#pragma once
#include "plan.h"
#include "real_plan.h"

namespace fourier_hip {

// The scratch bound of a DelayPlan is RealPlan's (REAL_SCRATCH_BYTES).  The experiments library and the emulator build read
// FOURIER_DELAY_SCRATCH_BYTES at create instead (the chunk-walk test).
template <typename T> class DelayPlan : public HandleBase {
 public:
  static constexpr size_t ELEM = sizeof(cpx<T>);
  enum Route { ONE_LAUNCH, COMPOSED };

  DelayPlan(size_t n, size_t length, size_t channels, int real_data, int device)
      : n_(n), l_(length), c_(channels), real_(real_data != 0) {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    if (n == 0 || n > length) throw EngineError(INVALID, "1 <= size <= length");
    if (channels == 0) throw EngineError(INVALID, "channels >= 1");
    if (real_data != 0 && real_data != 1) throw EngineError(INVALID, "real_data is 0 or 1");
    if (length * ELEM > REAL_LAUNCH_BYTES) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "delays above 2^31 bytes per row");
    // one launch of the sweep reads whole groups through one descriptor
    if (channels > REAL_LAUNCH_BYTES / (length * ELEM)) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "groups above 2^31 bytes of spectra");
    h_ = l_ / 2;
    if (real_) {
      rplan_.reset(new RealPlan<T>(l_, device));
      device_ = rplan_->inner().device();
      // the complex plan serves real rows only as the one-launch route's tables: built where that route can exist
      if (c_ == 1 && is_pow2(l_) && l_ >= 2048 && l_ <= 32768) {
        plan_.reset(new Plan<T>(l_, device));
        DeviceGuard g(device_);
        has_fused_ = plan_->enable_delay();
        if (!has_fused_) plan_.reset();
      }
    } else {
      plan_.reset(new Plan<T>(l_, device));
      device_ = plan_->device();
    }
    scratch_cap_ = scratch_bound("FOURIER_DELAY_SCRATCH_BYTES", REAL_SCRATCH_BYTES);
    launch_bytes_ = launch_bound("FOURIER_LAUNCH_BYTES", REAL_LAUNCH_BYTES);
    launch_items_ = launch_bound("FOURIER_LAUNCH_ITEMS", (size_t)1 << 30);
    // Where the one-launch route is the default: wherever it exists.  Every shape measured -- f32 L = 2^11, 2^13, 2^15 and f64 L = 2^11,
    // 2^13, 2^14, n = L / 2, 512 MiB of input -- took 0.26 - 0.42 of the composed route's time, the gap beyond the larger max - min of
    // the two arms on all 6 lines ("Fractional delay"; profiles/delay/delay_bench.jsonl).
    set_fusion(true);
  }

  size_t size() const { return n_; }
  size_t length() const { return l_; }
  size_t channels() const { return c_; }
  int device() const { return device_; }

  int set_option(const std::string& key, long long v) {
    if (key == "fusion" && (v == 0 || v == 1)) { set_fusion(v == 1); return ::fourier::c::FOURIER_HIP_OK; }
    return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
  }

  // groups per chunk for a call of `batch` input rows; sizes the scratch and the plans' buffers for it
  size_t prepare(size_t batch) const {
    if (batch == 0) return 0;
    if (route_ == ONE_LAUNCH) return batch;  // no scratch, no plan buffers
    const size_t chunk = chunk_rows((batch + c_ - 1) / c_, scratch_cap_, group_bytes());
    DeviceGuard g(device_);
    scratch_.ensure(chunk * group_bytes());
    if (real_) {
      rplan_->reserve(chunk * c_);
    } else {
      plan_->reserve_for(chunk * c_, true);
      plan_->reserve_for(chunk * c_, false);
    }
    return chunk;
  }
  void reserve(size_t batch) const { (void)prepare(batch); }

  // `batch` rows of n values at d_in, `batch` delays at d_delays and (unless null) `batch` weights at d_weights -> batch / C rows of n
  // values at d_out, which may be d_in when C == 1
  void apply(const void* d_in, const void* d_delays, const void* d_weights, void* d_out, size_t batch, hipStream_t stream) const {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    const size_t vs = real_ ? sizeof(T) : ELEM;
    if (batch % c_) throw EngineError(INVALID, "batch is not a multiple of channels");
    check_buffers(d_in, d_out, batch * n_ * vs, batch / c_ * n_ * vs, vs, c_ == 1);
    if (!d_delays) throw EngineError(INVALID, "null buffer");
    if ((uintptr_t)d_delays % sizeof(T) || (uintptr_t)d_weights % sizeof(T)) throw EngineError(INVALID, "misaligned buffer");
    if (batch == 0) return;
    DeviceGuard g(device_);
    const size_t chunk = prepare(batch);
    const char* in = (const char*)d_in;
    const T* dl = (const T*)d_delays;
    const T* wt = (const T*)d_weights;
    char* out = (char*)d_out;
    if (route_ == ONE_LAUNCH) {  // one workgroup a row: launches of less than 2^31 workgroups
      for_chunks(batch, launch_items_, [&](size_t c0, size_t nb) {
        plan_->exec_delay(in + c0 * n_ * vs, dl + c0, wt ? wt + c0 : nullptr, out + c0 * n_ * vs, nb, n_, stream);
      });
      return;
    }
    const int FWD = ::fourier::c::FOURIER_TRANSFORM_FFT, INV = ::fourier::c::FOURIER_TRANSFORM_UNSCALED_IFFT;
    const size_t spec = real_ ? h_ + 1 : l_;  // spectrum values a row
    // a chunk's scratch: the spectra of its rows, the sums of its groups (C > 1; the sweep runs in place where C == 1), then (real
    // rows) the padded rows and the inverse's whole rows
    cpx<T>* sx = (cpx<T>*)scratch_.p;
    cpx<T>* sy = c_ > 1 ? sx + chunk * c_ * spec : sx;
    T* pad = (T*)(sx + chunk * (c_ + (c_ > 1 ? 1 : 0)) * spec);
    T* rr = pad + chunk * c_ * l_;
    for_chunks(batch / c_, chunk, [&](size_t g0, size_t ng) {
      const size_t r0 = g0 * c_, nb = ng * c_;
      const char* src = in + r0 * n_ * vs;
      char* oc = out + g0 * n_ * vs;
      const T* wc = wt ? wt + r0 : nullptr;
      if (real_) {
        // the transforms read their rows as complex values: the caller's rows only where they need no padding and are aligned for that
        if (n_ != l_ || (uintptr_t)src % ELEM) { window_sweep(XCORR_PAD, src, pad, nb, true, stream); src = (const char*)pad; }
        rplan_->run_forward(src, sx, nb, FWD, stream);
        mul_sweep(sx, dl + r0, wc, sy, ng, stream);
        const bool direct = n_ == l_ && (uintptr_t)oc % ELEM == 0;
        rplan_->run_inverse(sy, direct ? (void*)oc : (void*)rr, ng, INV, stream);
        if (!direct) window_sweep(XCORR_WINDOW, rr, oc, ng, true, stream);
      } else {
        if (n_ != l_) { window_sweep(XCORR_PAD, src, sx, nb, false, stream); src = (const char*)sx; }
        plan_->exec(src, sx, nb, FWD, stream);
        cpx<T>* y = n_ == l_ ? (cpx<T>*)oc : sy;
        mul_sweep(sx, dl + r0, wc, y, ng, stream);
        plan_->exec(y, y, ng, INV, stream);
        if (n_ != l_) window_sweep(XCORR_WINDOW, y, oc, ng, false, stream);
      }
    });
  }

 private:
  void set_fusion(bool on) {
    route_ = on && has_fused_ ? ONE_LAUNCH : COMPOSED;
    if (route_ == ONE_LAUNCH) desc_ = std::string("delay one-launch: ") + plan_->describe();
    else if (!real_) desc_ = std::string("delay composed: ") + plan_->describe() + " (complex rows: no one-launch kernel)";
    else desc_ = std::string("delay composed: ") + rplan_->describe() +
                 (has_fused_ ? "" : c_ > 1 ? " (delay-and-sum: no one-launch kernel)" : " (no one-launch kernel for this length)");
  }
  // scratch bytes per group of a chunk on the composed routes
  size_t group_bytes() const {
    const size_t spec = real_ ? h_ + 1 : l_;
    return (c_ + (c_ > 1 ? 1 : 0)) * spec * ELEM + (real_ ? (c_ + 1) * l_ * sizeof(T) : 0);
  }

  // delay_mul_kernel over ng groups, in launches of whole groups of at most REAL_LAUNCH_BYTES of spectra (never less than one group)
  void mul_sweep(const cpx<T>* in, const T* delays, const T* weights, cpx<T>* out, size_t ng, hipStream_t stream) const {
    const size_t spec = real_ ? h_ + 1 : l_;
    const size_t irow = c_ * spec * ELEM, orow = spec * ELEM;
    const size_t per = std::max<size_t>(1, launch_bytes_ / irow);
    for (size_t g0 = 0; g0 < ng; g0 += per) {
      const size_t groups = std::min(per, ng - g0);
      DelayArgs a{};
      a.in = (const char*)in + g0 * irow;
      a.out = (char*)out + g0 * orow;
      a.delays = delays + g0 * c_;
      a.weights = weights ? weights + g0 * c_ : nullptr;
      a.l = (uint32_t)l_; a.spec = (uint32_t)spec; a.channels = (uint32_t)c_;
      a.total = (uint32_t)(groups * spec);
      divider(a.spec, a.div_m, a.div_l);
      divider(a.l, a.len_m, a.len_l);
      a.in_bytes = (uint32_t)(groups * irow);
      a.out_bytes = (uint32_t)(groups * orow);
      a.scale = code_scale<T>(::fourier::c::FOURIER_TRANSFORM_IFFT, (T)l_);  // the inverse's 1/L, folded into the multiplier
      FOURIER_LAUNCH(get_delay_kernel(Real<T>{}, real_), (a.total + 255) / 256, 256, 0, stream, a);
    }
  }

  // xcorr_pad_kernel (rows of n values -> rows of L, zeros from n on) or xcorr_window_kernel (rows of L -> their first n values) over
  // nb rows, in launches of at most REAL_LAUNCH_BYTES per side
  void window_sweep(int which, const void* in, void* out, size_t nb, bool real_values, hipStream_t stream) const {
    const size_t vs = real_values ? sizeof(T) : ELEM;
    const size_t ivals = which == XCORR_PAD ? n_ : l_, ovals = which == XCORR_PAD ? l_ : n_;
    const size_t irow = ivals * vs, orow = ovals * vs;
    const size_t rows_per = std::max<size_t>(1, launch_bytes_ / std::max(irow, orow));
    for (size_t r0 = 0; r0 < nb; r0 += rows_per) {
      const size_t rows = std::min(rows_per, nb - r0);
      XcorrArgs a{};
      a.in = (const char*)in + r0 * irow;
      a.out = (char*)out + r0 * orow;
      a.n = (uint32_t)n_; a.l = (uint32_t)l_;
      a.lags = (uint32_t)n_; a.first = 0;
      a.total = (uint32_t)(rows * ovals);
      divider((uint32_t)ovals, a.div_m, a.div_l);
      a.in_bytes = (uint32_t)(rows * irow);
      a.out_bytes = (uint32_t)(rows * orow);
      a.real = real_values;
      a.scale = 1.0;
      FOURIER_LAUNCH(get_xcorr_kernel(Real<T>{}, which, real_values, false), (a.total + 255) / 256, 256, 0, stream, a);
    }
  }

  size_t n_, l_, c_, h_ = 0;
  bool real_;
  int device_ = 0;
  std::unique_ptr<Plan<T>> plan_;       // complex rows: both transforms; real rows: the one-launch route's tables, absent where it has none
  std::unique_ptr<RealPlan<T>> rplan_;  // real rows, composed route: both transforms
  bool has_fused_ = false;
  Route route_ = COMPOSED;
  mutable DevBuf scratch_;
  size_t scratch_cap_ = REAL_SCRATCH_BYTES;
  size_t launch_bytes_ = REAL_LAUNCH_BYTES;  // of either side of one sweep launch (development switch FOURIER_LAUNCH_BYTES)
  size_t launch_items_ = (size_t)1 << 30;  // rows of the one-launch route of one launch (development switch FOURIER_LAUNCH_ITEMS)
};

}  // namespace fourier_hip
