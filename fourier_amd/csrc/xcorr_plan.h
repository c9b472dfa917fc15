// xcorr_plan.h -- the plan behind a cross-correlation handle (fourier_hip_xcorr_*, include/fourier.h): of batched rows x[b], y[b] of n
// values, zero-extended to a transform length L >= n,
//   G = conj(fft(x~)) fft(y~) psi,  r[b, l] = ifft(G)[l] = sum_t conj(x~[b, t]) y~[b, (t + l) mod L]  (psi = 1),
//   out[b, j] = r[b, (lag_first + j) mod L],  j < lags,
// psi = 1 or (option "weighting" = FOURIER_XCORR_WEIGHT_PHAT) 1 / (|X| |Y|): the generalized cross-correlation with phase transform.
// Real rows give real output, complex rows complex output.  Built on a complex Plan<T>(L) and a RealPlan<T>(L) that run unchanged.
// Routes, chosen at create:
//   "xcorr one-launch"  real rows, L a one-launch two-level length (2^11 ... 2^15, f64 ... 2^14), where the kernel of that precision
//                       and weighting runs without scratch memory (f64 without weighting; kernels_xcorr.cpp): both rows as ONE
//                       complex row, balanced by powers of two, FFT, the mirror exchange that separates X and Y, the weighted
//                       product, inverse FFT, store of the window in ONE launch on register-resident data (xcorr_small_kernel,
//                       Plan::exec_xcorr); no scratch
//   "xcorr composed"    any L.  Real rows: each row padded to L (xcorr_pad_kernel; skipped where n == L and the rows are aligned
//                       for the transform), RealPlan forward of each -> two half spectra of L/2 + 1 values, xcorr_mul_kernel ->
//                       G / L in place of Y's, RealPlan unscaled inverse -> the caller's output where the window is the whole row
//                       (lag_first == 0, lags == L) and the output is aligned for it, else scratch and xcorr_window_kernel.  The two
//                       rows are transformed APART, so that power-of-two scaling of either row is exact.  Complex rows: the same
//                       with Plan<T>(L) on whole spectra, the inverse in place.  Complex rows have no one-launch route.
// d_x == d_y (the autocorrelation) transforms the row once on the composed routes.
// Option "fusion" = 1 (the default, by the measurements at the constructor) selects the one-launch route where it exists, 0 the
// composed route.  The batch is walked in chunks so that the plan-owned scratch stays bounded; no atomics: the result is the same on
// repetition and under any scratch bound (up to the inner transforms' own dependence on a row's position in its launch: at f32 their
// last bits differ between even and odd rows, so a bound of an odd number of rows moves last bits).
#pragma once
#include "plan.h"
#include "real_plan.h"

namespace fourier_hip {

// The scratch bound of an XcorrPlan is RealPlan's (REAL_SCRATCH_BYTES).  The experiments library and the emulator build read
// FOURIER_XCORR_SCRATCH_BYTES at create instead (the chunk-walk test).
template <typename T> class XcorrPlan : public HandleBase {
 public:
  static constexpr size_t ELEM = sizeof(cpx<T>);
  enum Route { ONE_LAUNCH, COMPOSED };

  XcorrPlan(size_t n, size_t length, long long lag_first, size_t lags, int real_data, int device)
      : n_(n), l_(length), lags_(lags), real_(real_data != 0) {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    if (n == 0 || n > length) throw EngineError(INVALID, "1 <= size <= length");
    if (lags == 0 || lags > length) throw EngineError(INVALID, "1 <= lags <= length");
    if (real_data != 0 && real_data != 1) throw EngineError(INVALID, "real_data is 0 or 1");
    if (lag_first <= -(long long)length || lag_first >= (long long)length) throw EngineError(INVALID, "|lag_first| < length");
    if (length * ELEM > REAL_LAUNCH_BYTES) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "correlations above 2^31 bytes per row");
    first_ = (size_t)(lag_first < 0 ? lag_first + (long long)length : lag_first);
    h_ = l_ / 2;
    if (real_) {
      rplan_.reset(new RealPlan<T>(l_, device));
      device_ = rplan_->inner().device();
      // the complex plan serves real rows only as the one-launch route's tables: built where that route can exist
      if (is_pow2(l_) && l_ >= 2048 && l_ <= 32768) {
        plan_.reset(new Plan<T>(l_, device));
        DeviceGuard g(device_);
        has_fused_ = plan_->enable_xcorr();
        if (!has_fused_) plan_.reset();
      }
    } else {
      plan_.reset(new Plan<T>(l_, device));
      device_ = plan_->device();
    }
    scratch_cap_ = scratch_bound("FOURIER_XCORR_SCRATCH_BYTES", REAL_SCRATCH_BYTES);
    launch_bytes_ = launch_bound("FOURIER_LAUNCH_BYTES", REAL_LAUNCH_BYTES);
    launch_items_ = launch_bound("FOURIER_LAUNCH_ITEMS", (size_t)1 << 30);
    // Where the one-launch route is the default: wherever it exists.  Every shape measured -- f64, L = 2^11, 2^13, 2^14, n = L / 2, the
    // full linear window, 512 MiB of input -- took 0.23 - 0.37 of the composed route's time, the gap beyond the larger max - min of the
    // two arms on all 3 lines ("Cross-correlation"; profiles/xcorr/xcorr_bench.jsonl).
    set_fusion(true);
  }

  size_t size() const { return n_; }
  size_t length() const { return l_; }
  size_t lags() const { return lags_; }
  int device() const { return device_; }

  int set_option(const std::string& key, long long v) {
    if (key == "fusion" && (v == 0 || v == 1)) { set_fusion(v == 1); return ::fourier::c::FOURIER_HIP_OK; }
    if (key == "weighting" && (v == ::fourier::c::FOURIER_XCORR_WEIGHT_NONE || v == ::fourier::c::FOURIER_XCORR_WEIGHT_PHAT)) {
      phat_ = v == ::fourier::c::FOURIER_XCORR_WEIGHT_PHAT;
      set_fusion(fusion_);  // (a weighting may have no one-launch kernel)
      return ::fourier::c::FOURIER_HIP_OK;
    }
    return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
  }

  // rows per chunk for a call of `batch` rows; sizes the scratch and the plans' buffers for it
  size_t prepare(size_t batch) const {
    if (batch == 0) return 0;
    if (route_ == ONE_LAUNCH) return batch;  // no scratch, no plan buffers
    const size_t chunk = chunk_rows(batch, scratch_cap_, row_bytes());
    DeviceGuard g(device_);
    scratch_.ensure(chunk * row_bytes());
    if (real_) {
      rplan_->reserve(chunk);
    } else {
      plan_->reserve_for(chunk, true);
      plan_->reserve_for(chunk, false);
    }
    return chunk;
  }
  void reserve(size_t batch) const { (void)prepare(batch); }

  // `batch` rows of n values at d_x and at d_y (which may be the same) -> `batch` rows of `lags` values at d_out, apart from both
  void correlate(const void* d_x, const void* d_y, void* d_out, size_t batch, hipStream_t stream) const {
    const size_t vs = real_ ? sizeof(T) : ELEM;
    check_buffers(d_x, d_out, batch * n_ * vs, batch * lags_ * vs, vs, false);
    check_buffers(d_y, d_out, batch * n_ * vs, batch * lags_ * vs, vs, false);
    if (batch == 0) return;
    DeviceGuard g(device_);
    const size_t chunk = prepare(batch);
    const char* x = (const char*)d_x;
    const char* y = (const char*)d_y;
    char* out = (char*)d_out;
    if (route_ == ONE_LAUNCH) {  // one workgroup a row pair: launches of less than 2^31 workgroups
      for_chunks(batch, launch_items_, [&](size_t c0, size_t nb) {
        plan_->exec_xcorr(x + c0 * n_ * vs, y + c0 * n_ * vs, out + c0 * lags_ * vs, nb, n_, first_, lags_, phat_, stream);
      });
      return;
    }
    const int FWD = ::fourier::c::FOURIER_TRANSFORM_FFT, INV = ::fourier::c::FOURIER_TRANSFORM_UNSCALED_IFFT;
    const bool same = d_x == d_y;
    const bool whole = first_ == 0 && lags_ == l_;
    const size_t spec = real_ ? h_ + 1 : l_;  // spectrum values a row
    // a chunk's scratch: the two spectra, then (real rows) the two padded rows and the inverse's whole row
    cpx<T>* sx = (cpx<T>*)scratch_.p;
    cpx<T>* sy = sx + chunk * spec;
    T* px = (T*)(sy + chunk * spec);
    T* py = px + chunk * l_;
    T* rr = py + chunk * l_;
    for_chunks(batch, chunk, [&](size_t c0, size_t nb) {
      const char* xc = x + c0 * n_ * vs;
      const char* yc = y + c0 * n_ * vs;
      char* oc = out + c0 * lags_ * vs;
      if (real_) {
        // the transforms read their rows as complex values: the caller's rows only where they need no padding and are aligned for that
        const auto spectrum = [&](const char* src, T* pad, cpx<T>* s) {
          if (n_ != l_ || (uintptr_t)src % ELEM) { sweep(XCORR_PAD, src, nullptr, pad, nb, true, stream); src = (const char*)pad; }
          rplan_->run_forward(src, s, nb, FWD, stream);
        };
        spectrum(xc, px, sx);
        if (!same) spectrum(yc, py, sy);
        sweep(XCORR_MUL, sx, same ? sx : sy, sy, nb, true, stream);
        const bool direct = whole && (uintptr_t)oc % ELEM == 0;
        rplan_->run_inverse(sy, direct ? (void*)oc : (void*)rr, nb, INV, stream);
        if (!direct) sweep(XCORR_WINDOW, rr, nullptr, oc, nb, true, stream);
      } else {
        const auto spectrum = [&](const char* src, cpx<T>* s) {
          if (n_ != l_) { sweep(XCORR_PAD, src, nullptr, s, nb, false, stream); src = (const char*)s; }
          plan_->exec(src, s, nb, FWD, stream);
        };
        spectrum(xc, sx);
        if (!same) spectrum(yc, sy);
        cpx<T>* g = whole ? (cpx<T>*)oc : sy;
        sweep(XCORR_MUL, sx, same ? sx : sy, g, nb, false, stream);
        plan_->exec(g, g, nb, INV, stream);
        if (!whole) sweep(XCORR_WINDOW, g, nullptr, oc, nb, false, stream);
      }
    });
  }

 private:
  void set_fusion(bool on) {
    fusion_ = on;
    const bool has = (has_fused_ >> (phat_ ? 1 : 0)) & 1;
    route_ = on && has ? ONE_LAUNCH : COMPOSED;
    if (route_ == ONE_LAUNCH) desc_ = std::string("xcorr one-launch: ") + plan_->describe();
    else if (real_) desc_ = std::string("xcorr composed: ") + rplan_->describe() + (has ? "" : " (no one-launch kernel for this length and weighting)");
    else desc_ = std::string("xcorr composed: ") + plan_->describe() + " (complex rows: no one-launch kernel)";
  }
  // scratch bytes per row pair of a chunk on the composed routes
  size_t row_bytes() const { return real_ ? 2 * (h_ + 1) * ELEM + 3 * l_ * sizeof(T) : 2 * l_ * ELEM; }

  // one sweep of kernels_xcorr.h over nb rows, in launches of at most REAL_LAUNCH_BYTES per side
  void sweep(int which, const void* in, const void* in2, void* out, size_t nb, bool real_values, hipStream_t stream) const {
    const size_t vs = which == XCORR_MUL ? ELEM : real_values ? sizeof(T) : ELEM;
    const size_t spec = real_values ? h_ + 1 : l_;
    const size_t ivals = which == XCORR_PAD ? n_ : which == XCORR_MUL ? spec : l_;
    const size_t ovals = which == XCORR_PAD ? l_ : which == XCORR_MUL ? spec : lags_;
    const size_t irow = ivals * vs, orow = ovals * vs;
    const size_t rows_per = std::max<size_t>(1, launch_bytes_ / std::max(irow, orow));
    for (size_t r0 = 0; r0 < nb; r0 += rows_per) {
      const size_t rows = std::min(rows_per, nb - r0);
      XcorrArgs a{};
      a.in = (const char*)in + r0 * irow;
      a.in2 = in2 ? (const char*)in2 + r0 * irow : nullptr;
      a.out = (char*)out + r0 * orow;
      a.n = (uint32_t)n_; a.l = (uint32_t)l_;
      a.lags = (uint32_t)lags_; a.first = (uint32_t)first_;
      a.total = (uint32_t)(rows * ovals);
      divider((uint32_t)ovals, a.div_m, a.div_l);
      a.in_bytes = (uint32_t)(rows * irow);
      a.out_bytes = (uint32_t)(rows * orow);
      a.real = real_values; a.phat = phat_;
      a.scale = code_scale<T>(::fourier::c::FOURIER_TRANSFORM_IFFT, (T)l_);  // the inverse's 1/L, folded into the product
      FOURIER_LAUNCH(get_xcorr_kernel(Real<T>{}, which, real_values, phat_), (a.total + 255) / 256, 256, 0, stream, a);
    }
  }

  size_t n_, l_, lags_, first_ = 0, h_ = 0;
  bool real_;
  bool phat_ = false;
  int device_ = 0;
  std::unique_ptr<Plan<T>> plan_;       // complex rows: both transforms; real rows: the one-launch route's tables, absent where it has none
  std::unique_ptr<RealPlan<T>> rplan_;  // real rows, composed route: both transforms
  int has_fused_ = 0;                   // the weightings with a one-launch kernel: bit 0 none, bit 1 PHAT
  bool fusion_ = false;
  Route route_ = COMPOSED;
  mutable DevBuf scratch_;
  size_t scratch_cap_ = REAL_SCRATCH_BYTES;
  size_t launch_bytes_ = REAL_LAUNCH_BYTES;  // of either side of one sweep launch (development switch FOURIER_LAUNCH_BYTES)
  size_t launch_items_ = (size_t)1 << 30;  // rows of the one-launch route of one launch (development switch FOURIER_LAUNCH_ITEMS)
};

}  // namespace fourier_hip
