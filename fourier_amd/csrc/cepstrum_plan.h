// cepstrum_plan.h -- the plan behind a cepstrum handle (fourier_hip_cepstrum_*, include/fourier.h): batched rows of n reals,
// zero-extended to a transform length L >= n; with X = fft(x, L) and the per-call reals log_mult != 0 and log_floor >= 0 (log_mult
// finite and not 0 AFTER rounding to T, a positive log_floor a normal number of T after rounding: anything else is an invalid
// argument; every such floor is honoured, also where its square leaves T)
//   g[k] = log_mult ln(max(|X[k]|, log_floor)), formed as 0.5 log_mult ln(max(re^2 + im^2, log_floor^2)) with the accurate logarithm
//   mode CEPSTRUM (0):       c = ifft(g), real and even;  out = c[0 .. m),  m <= L
//   mode MINIMUM_PHASE (1):  chat[0] = c[0], chat[q] = 2 c[q] for 0 < q < L/2 (odd L: q <= (L - 1) / 2), chat[L/2] = c[L/2] (even L),
//                            0 above;  C = fft(chat),  E[k] = exp(Re C[k]) (cos Im C[k], sin Im C[k]),  h = Re ifft(E);  out = h[0 .. m)
// log_mult = 0.5 in mode 1 is scipy.signal.minimum_phase(method="homomorphic", half=True).  Two deviations from scipy 1.15.3: the
// floor is the caller's log_floor applied with max (scipy adds 1e-7 x the smallest positive |X|, a reduction over the data), and at
// even L quefrency L/2 keeps weight 1 (Oppenheim and Schafer eq. 13.42b; scipy's window leaves it at 0).
// Built on a RealPlan<T>(L) that runs unchanged, and on a complex Plan<T>(L) that lends its tables.  Routes, chosen at create:
//   "cepstrum one-launch"  L a one-launch two-level length with a kernel of the mode (2^11 ... 2^15, f64 ... 2^14;
//                          kernels_cepstrum.cpp): the whole chain -- two transforms, or four -- in ONE launch on register-resident
//                          data (cepstrum_small_kernel, Plan::exec_cepstrum); no scratch; in place allowed where m == n
//   "cepstrum composed"    any L that RealPlan accepts: each row padded to L (xcorr_pad_kernel; skipped where n == L and the rows are
//                          aligned for the transform), RealPlan forward -> half spectra, cepstrum_log_kernel in place with 1/L folded
//                          in, RealPlan unscaled inverse.  CEPSTRUM ends here: into the caller's output where m == L and it is aligned
//                          for that, else into scratch and through xcorr_window_kernel.  MINIMUM_PHASE goes on: cepstrum_fold_kernel
//                          in place, RealPlan forward, cepstrum_exp_kernel in place with 1/L folded in, RealPlan unscaled inverse,
//                          and the direct write or xcorr_window_kernel as before.
// Option "fusion" = 1 (the default, by the measurements at the constructor) selects the one-launch route where it exists, 0 the
// composed route.
// The batch is walked in chunks of WHOLE rows so that the plan-owned scratch stays bounded (never less than one row); no atomics: the
// result is the same on repetition and under any scratch bound (up to the inner transforms' own dependence on a row's position in its
// launch: at f32 their last bits differ between even and odd rows, DESIGN.md section 4, "Cross-correlation").
#pragma once
#include <cmath>
#include <limits>

#include "plan.h"
#include "real_plan.h"

namespace fourier_hip {

// The scratch bound of a CepstrumPlan is RealPlan's (REAL_SCRATCH_BYTES).  The experiments library and the emulator build read
// FOURIER_CEPSTRUM_SCRATCH_BYTES at create instead (the chunk-walk test).
template <typename T> class CepstrumPlan : public HandleBase {
 public:
  static constexpr size_t ELEM = sizeof(cpx<T>);
  enum Route { ONE_LAUNCH, COMPOSED };
  enum Mode { CEPSTRUM = 0, MINIMUM_PHASE = 1 };

  CepstrumPlan(size_t n, size_t length, size_t outputs, int mode, int device) : n_(n), l_(length), m_(outputs), mode_(mode) {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    if (n == 0) throw EngineError(INVALID, "size >= 1");
    if (n > length) throw EngineError(INVALID, "size <= length");
    if (outputs == 0) throw EngineError(INVALID, "outputs >= 1");
    if (outputs > length) throw EngineError(INVALID, "outputs <= length");
    if (mode != CEPSTRUM && mode != MINIMUM_PHASE) throw EngineError(INVALID, "mode is 0 (cepstrum) or 1 (minimum phase)");
    if (length * ELEM > REAL_LAUNCH_BYTES) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "cepstra above 2^31 bytes per row");
    h_ = l_ / 2;
    rplan_.reset(new RealPlan<T>(l_, device));
    device_ = rplan_->inner().device();
    // the complex plan serves only as the one-launch route's tables: built where that route can exist
    if (is_pow2(l_) && l_ >= 2048 && l_ <= 32768) {
      plan_.reset(new Plan<T>(l_, device));
      DeviceGuard g(device_);
      has_fused_ = plan_->enable_cepstrum(mode_);
      if (!has_fused_) plan_.reset();
    }
    scratch_cap_ = scratch_bound("FOURIER_CEPSTRUM_SCRATCH_BYTES", REAL_SCRATCH_BYTES);
    launch_bytes_ = launch_bound("FOURIER_LAUNCH_BYTES", REAL_LAUNCH_BYTES);
    launch_items_ = launch_bound("FOURIER_LAUNCH_ITEMS", (size_t)1 << 30);
    // Where the one-launch route is the default: wherever it exists, in both modes.  Every shape measured -- f32 L = 2^11, 2^13, 2^15
    // and f64 L = 2^11, 2^13, 2^14, n = L / 2, m = n, 512 MiB of input -- at which the product holds the kernel took 0.26 - 0.53
    // (cepstrum, 6 shapes) and 0.29 - 0.51 (minimum phase, 4 shapes: f32 2^13 and 2^15 have no kernel) of the composed route's time,
    // the gap beyond the larger max - min of the two arms on all 10 lines ("Cepstrum and minimum phase";
    // profiles/cepstrum/cepstrum_bench.jsonl).
    set_fusion(true);
  }

  size_t size() const { return n_; }
  size_t length() const { return l_; }
  size_t outputs() const { return m_; }
  int mode() const { return mode_; }
  int device() const { return device_; }

  int set_option(const std::string& key, long long v) {
    if (key == "fusion" && (v == 0 || v == 1)) { set_fusion(v == 1); return ::fourier::c::FOURIER_HIP_OK; }
    return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
  }

  // rows per chunk for a call of `batch` rows; sizes the scratch and the real plan's buffers for it
  size_t prepare(size_t batch) const {
    if (batch == 0) return 0;
    if (route_ == ONE_LAUNCH) return batch;  // no scratch, no plan buffers
    const size_t chunk = chunk_rows(batch, scratch_cap_, row_bytes());
    DeviceGuard g(device_);
    scratch_.ensure(chunk * row_bytes());
    rplan_->reserve(chunk);
    return chunk;
  }
  void reserve(size_t batch) const { (void)prepare(batch); }

  // `batch` rows of n reals at d_in -> `batch` rows of m reals at d_out, which may be d_in where m == n
  void apply(const void* d_in, void* d_out, size_t batch, double log_mult, double log_floor, hipStream_t stream) const {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    if (!std::isfinite(log_mult) || log_mult == 0) throw EngineError(INVALID, "log_mult is finite and not 0");
    if (!std::isfinite(log_floor) || log_floor < 0) throw EngineError(INVALID, "log_floor is finite and not negative");
    // in T too: the kernels work with the rounded values, and a floor that rounds to 0 would silently mean "no floor"
    const T lm = (T)log_mult, fl = (T)log_floor;
    if (!std::isfinite(lm) || lm == (T)0) throw EngineError(INVALID, "log_mult is finite and not 0 in the handle's precision");
    if (log_floor > 0 && !std::isnormal(fl)) throw EngineError(INVALID, "a positive log_floor is a normal number of the handle's precision");
    check_buffers(d_in, d_out, batch * n_ * sizeof(T), batch * m_ * sizeof(T), sizeof(T), m_ == n_);
    if (batch == 0) return;
    DeviceGuard g(device_);
    const size_t chunk = prepare(batch);
    const T* in = (const T*)d_in;
    T* out = (T*)d_out;
    // Every normal floor is honoured whatever its square does in T: where fl * fl is no normal number the kernels get it clamped
    // and take the value of a bin below it from here, rounded to T once (CepstrumFloor, kernel_args.h); where it is one, their
    // arithmetic is what it always was
    const T sq = fl * fl;  // computed in T
    CepstrumFloor floor{(double)sq, 0.0, 0u};
    if (fl > (T)0 && !std::isnormal(sq)) {
      floor.floor2 = (double)std::max(sq, std::numeric_limits<T>::min());
      floor.ln_floor = std::log((double)fl);
      floor.given = 1u;
    }
    if (route_ == ONE_LAUNCH) {  // one workgroup a row: launches of less than 2^31 workgroups
      for_chunks(batch, launch_items_, [&](size_t c0, size_t nb) {
        plan_->exec_cepstrum(in + c0 * n_, out + c0 * m_, nb, n_, m_, mode_, (double)lm, floor, stream);
      });
      return;
    }
    const int FWD = ::fourier::c::FOURIER_TRANSFORM_FFT, INV = ::fourier::c::FOURIER_TRANSFORM_UNSCALED_IFFT;
    const size_t spec = h_ + 1;  // half-spectrum values a row
    const double inv_l = code_scale<T>(::fourier::c::FOURIER_TRANSFORM_IFFT, (T)l_);  // the inverse's 1/L, folded into the sweeps
    // a chunk's scratch: the half spectra of its rows, the padded rows, the inverses' whole rows
    cpx<T>* sx = (cpx<T>*)scratch_.p;
    T* pad = (T*)(sx + chunk * spec);
    T* rr = pad + chunk * l_;
    for_chunks(batch, chunk, [&](size_t r0, size_t nb) {
      const T* src = in + r0 * n_;
      T* oc = out + r0 * m_;
      // the transforms read their rows as complex values: the caller's rows only where they need no padding and are aligned for that
      if (n_ != l_ || (uintptr_t)src % ELEM) { window_sweep(XCORR_PAD, src, pad, nb, stream); src = pad; }
      const bool direct = m_ == l_ && (uintptr_t)oc % ELEM == 0;
      rplan_->run_forward(src, sx, nb, FWD, stream);
      sweep(CEPSTRUM_LOG, sx, nb, spec * ELEM, (double)lm, floor, inv_l, stream);
      const bool last = mode_ == CEPSTRUM;
      rplan_->run_inverse(sx, last && direct ? (void*)oc : (void*)rr, nb, INV, stream);
      if (!last) {
        sweep(CEPSTRUM_FOLD, rr, nb, l_ * sizeof(T), 0.0, CepstrumFloor{}, 1.0, stream);
        rplan_->run_forward(rr, sx, nb, FWD, stream);
        sweep(CEPSTRUM_EXP, sx, nb, spec * ELEM, 0.0, CepstrumFloor{}, inv_l, stream);
        rplan_->run_inverse(sx, direct ? (void*)oc : (void*)rr, nb, INV, stream);
      }
      if (!direct) window_sweep(XCORR_WINDOW, rr, oc, nb, stream);
    });
  }

 private:
  void set_fusion(bool on) {
    route_ = on && has_fused_ ? ONE_LAUNCH : COMPOSED;
    const char* what = mode_ == CEPSTRUM ? "real cepstrum" : "minimum phase";
    if (route_ == ONE_LAUNCH) desc_ = std::string("cepstrum one-launch (") + what + "): " + plan_->describe();
    else desc_ = std::string("cepstrum composed (") + what + "): " + rplan_->describe() + (has_fused_ ? "" : " (no one-launch kernel for this length and mode)");
  }
  // scratch bytes per row of a chunk on the composed route
  size_t row_bytes() const { return (h_ + 1) * ELEM + 2 * l_ * sizeof(T); }

  // one of the three in-place sweeps over nb rows of `row` bytes, in launches of whole rows of at most REAL_LAUNCH_BYTES (never less
  // than one row)
  void sweep(int which, void* data, size_t nb, size_t row, double log_mult, const CepstrumFloor& floor, double scale, hipStream_t stream) const {
    const size_t vs = which == CEPSTRUM_FOLD ? sizeof(T) : ELEM;
    const size_t per = std::max<size_t>(1, launch_bytes_ / row);
    for (size_t r0 = 0; r0 < nb; r0 += per) {
      const size_t rows = std::min(per, nb - r0);
      CepstrumArgs a{};
      a.data = (char*)data + r0 * row;
      a.l = (uint32_t)l_;
      a.total = (uint32_t)(rows * (row / vs));
      divider(a.l, a.div_m, a.div_l);
      a.bytes = (uint32_t)(rows * row);
      a.log_mult = log_mult; a.floor2 = floor.floor2; a.g_floor = log_mult * floor.ln_floor / (double)l_; a.floor_given = floor.given; a.scale = scale;
      FOURIER_LAUNCH(get_cepstrum_kernel(Real<T>{}, which), (a.total + 255) / 256, 256, 0, stream, a);
    }
  }

  // xcorr_pad_kernel (rows of n reals -> rows of L, zeros from n on) or xcorr_window_kernel (rows of L -> their first m reals) over
  // nb rows, in launches of at most REAL_LAUNCH_BYTES per side
  void window_sweep(int which, const void* in, void* out, size_t nb, hipStream_t stream) const {
    const size_t vs = sizeof(T);
    const size_t ivals = which == XCORR_PAD ? n_ : l_, ovals = which == XCORR_PAD ? l_ : m_;
    const size_t irow = ivals * vs, orow = ovals * vs;
    const size_t rows_per = std::max<size_t>(1, launch_bytes_ / std::max(irow, orow));
    for (size_t r0 = 0; r0 < nb; r0 += rows_per) {
      const size_t rows = std::min(rows_per, nb - r0);
      XcorrArgs a{};
      a.in = (const char*)in + r0 * irow;
      a.out = (char*)out + r0 * orow;
      a.n = (uint32_t)n_; a.l = (uint32_t)l_;
      a.lags = (uint32_t)m_; a.first = 0;
      a.total = (uint32_t)(rows * ovals);
      divider((uint32_t)ovals, a.div_m, a.div_l);
      a.in_bytes = (uint32_t)(rows * irow);
      a.out_bytes = (uint32_t)(rows * orow);
      a.real = true;
      a.scale = 1.0;
      FOURIER_LAUNCH(get_xcorr_kernel(Real<T>{}, which, true, false), (a.total + 255) / 256, 256, 0, stream, a);
    }
  }

  size_t n_, l_, m_, h_ = 0;
  int mode_;
  int device_ = 0;
  std::unique_ptr<Plan<T>> plan_;       // the one-launch route's tables, absent where it has no kernel
  std::unique_ptr<RealPlan<T>> rplan_;  // the composed route: all transforms
  bool has_fused_ = false;
  Route route_ = COMPOSED;
  mutable DevBuf scratch_;
  size_t scratch_cap_ = REAL_SCRATCH_BYTES;
  size_t launch_bytes_ = REAL_LAUNCH_BYTES;  // of either side of one sweep launch (development switch FOURIER_LAUNCH_BYTES)
  size_t launch_items_ = (size_t)1 << 30;  // rows of the one-launch route of one launch (development switch FOURIER_LAUNCH_ITEMS)
};

}  // namespace fourier_hip
