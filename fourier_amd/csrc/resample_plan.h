// resample_plan.h -- the plan behind a resampling handle (fourier_hip_resample_*, include/fourier.h): batched rows of N = n_in values
// -> rows of M = n_out values through the spectrum, scipy.signal.resample(x, M, axis=-1, window=W) with W an array of N reals in FFT
// order or absent.  K = min(N, M); the definition, with the rule of an even K's bin K/2, is the header's.  Built on two complex
// Plan<T>s or two RealPlan<T>s that run unchanged.  Routes, chosen at create:
//   "resample complex"              complex rows, any N and M: Plan(N) forward -> scratch (rows of N), resample_remap_kernel -> the
//                                   caller's output (rows of M; window, Nyquist rule and 1/N folded in), Plan(M) unscaled inverse in
//                                   place there
//   "resample real composed"        real rows, any N and M: RealPlan(N) forward -> scratch (rows of N/2 + 1), the remap in its
//                                   half-spectrum form -> a second scratch (rows of M/2 + 1), RealPlan(M) unscaled inverse -> the output
//   "resample real fused untangle"  real rows, N and M both even: RealPlan(N)'s inner N/2-point FFT on the reals taken as complex
//                                   values -> scratch, ONE launch of resample_untangle_kernel (post-untangle, remap and pre-untangle)
//                                   -> a second scratch, RealPlan(M)'s inner unscaled inverse -> the output
// Option "fusion" = 1 (the default, by the measurements at the constructor) selects the fused untangle route where it exists, 0 the
// composed route; on the other routes the option is accepted and changes nothing.  The sweeps are
// kernels_resample.h.  The batch is walked in chunks so that the plan-owned scratch stays bounded; one chunk size serves reserve and
// the run.  No atomics: the result is the same under any scratch bound and on repetition.
#pragma once
#include "plan.h"
#include "real_plan.h"

namespace fourier_hip {

// The scratch bound of a ResamplePlan is RealPlan's (REAL_SCRATCH_BYTES).  The experiments library and the emulator build read
// FOURIER_RESAMPLE_SCRATCH_BYTES at create instead (the chunk-walk test).
template <typename T> class ResamplePlan : public HandleBase {
 public:
  static constexpr size_t ELEM = sizeof(cpx<T>);
  enum Route { COMPLEX, REAL_COMPOSED, REAL_FUSED };

  ResamplePlan(size_t n_in, size_t n_out, int real_input, int device) : n_(n_in), m_(n_out), real_(real_input != 0) {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, UNSUPPORTED = ::fourier::c::FOURIER_HIP_UNSUPPORTED;
    if (n_in == 0 || n_out == 0) throw EngineError(INVALID, "size 0 is invalid");
    if (real_input != 0 && real_input != 1) throw EngineError(INVALID, "real_input is 0 or 1");
    if (std::max(n_, m_) > REAL_LAUNCH_BYTES / ELEM) throw EngineError(UNSUPPORTED, "rows above 2^31 bytes of spectrum");
    if (real_) {
      rin_.reset(new RealPlan<T>(n_, device));
      rout_.reset(new RealPlan<T>(m_, device));
      device_ = rin_->inner().device();
      has_fused_ = rin_->even() && rout_->even();
    } else {
      pin_.reset(new Plan<T>(n_, device));
      pout_.reset(new Plan<T>(m_, device));
      device_ = pin_->device();
    }
    scratch_cap_ = scratch_bound("FOURIER_RESAMPLE_SCRATCH_BYTES", REAL_SCRATCH_BYTES);
    launch_bytes_ = launch_bound("FOURIER_LAUNCH_BYTES", REAL_LAUNCH_BYTES);
    // Where the fused untangle route is the default: wherever it exists.  Every real even / even shape measured -- 64 rows of 2^20 ->
    // 2^19 and 2^20 -> 2^21, 1024 rows of 48000 -> 44100 and 44100 -> 48000, f32 and f64 -- took 0.79 - 0.84 of the composed route's
    // time, the gap beyond the larger max - min of the two arms on all 8 lines ("Fourier-domain resampling";
    // profiles/resample/resample_bench.jsonl).
    set_fusion(true);
  }

  size_t size_in() const { return n_; }
  size_t size_out() const { return m_; }
  bool real_input() const { return real_; }
  int device() const { return device_; }

  int set_option(const std::string& key, long long v) {
    if (key == "fusion" && (v == 0 || v == 1)) { set_fusion(v == 1); return ::fourier::c::FOURIER_HIP_OK; }
    return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
  }

  // n_in reals T on the device, FFT order, or nullptr for no window.  A set-up call: it waits for `stream` (the handle keeps a copy of
  // its own, replaced in place).  Real rows keep the folded window Wr[0] = W[0], Wr[k] = (W[k] + W[N-k]) / 2, k <= N/2.
  void set_window(const void* d_window, hipStream_t stream) {
    if (d_window && (uintptr_t)d_window % sizeof(T)) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "misaligned window");
    DeviceGuard g(device_);
    if (!d_window) {
      HIP_CHECK(hipStreamSynchronize(stream));
      has_win_ = false;
      return;
    }
    std::vector<T> w(n_);
    HIP_CHECK(hipMemcpyAsync(w.data(), d_window, n_ * sizeof(T), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    if (real_) {
      std::vector<T> f(n_ / 2 + 1);
      f[0] = w[0];
      for (size_t k = 1; k < f.size(); ++k) f[k] = (w[k] + w[n_ - k]) * (T)0.5;
      win_.upload(f);
    } else {
      win_.upload(w);
    }
    has_win_ = true;
  }

  // rows per chunk for a call of `batch` rows; sizes the scratch and the plans' buffers for it
  size_t prepare(size_t batch) const {
    if (batch == 0) return 0;
    const size_t chunk = chunk_rows(batch, scratch_cap_, row_bytes());
    DeviceGuard g(device_);
    scratch_.ensure(chunk * row_bytes());
    switch (route_) {
      case COMPLEX: pin_->reserve_for(chunk, false); pout_->reserve_for(chunk, true); break;
      case REAL_COMPOSED: rin_->reserve(chunk); rout_->reserve(chunk); break;
      case REAL_FUSED: rin_->inner().reserve_for(chunk, false); rout_->inner().reserve_for(chunk, false); break;
    }
    return chunk;
  }
  void reserve(size_t batch) const { (void)prepare(batch); }

  // `batch` rows of N values at d_in -> `batch` rows of M values at d_out, apart from the input
  void forward(const void* d_in, void* d_out, size_t batch, hipStream_t stream) const {
    const size_t vs = real_ ? sizeof(T) : ELEM;
    check_buffers(d_in, d_out, batch * n_ * vs, batch * m_ * vs, vs, false);
    if (batch == 0) return;
    DeviceGuard g(device_);
    const size_t chunk = prepare(batch);
    const int FWD = ::fourier::c::FOURIER_TRANSFORM_FFT, INV = ::fourier::c::FOURIER_TRANSFORM_UNSCALED_IFFT;
    const char* in = (const char*)d_in;
    char* out = (char*)d_out;
    cpx<T>* a = (cpx<T>*)scratch_.p;  // the spectra of a chunk, or the forward inner transform's output
    for_chunks(batch, chunk, [&](size_t c0, size_t nb) {
      const void* src = in + c0 * n_ * vs;
      void* dst = out + c0 * m_ * vs;
      switch (route_) {
        case COMPLEX:
          pin_->exec(src, a, nb, FWD, stream);
          sweep(RESAMPLE_REMAP, a, dst, nb, stream);
          pout_->exec(dst, dst, nb, INV, stream);
          break;
        case REAL_COMPOSED: {
          cpx<T>* b = a + chunk * (n_ / 2 + 1);
          rin_->run_forward(src, a, nb, FWD, stream);
          sweep(RESAMPLE_REMAP, a, b, nb, stream);
          rout_->run_inverse(b, dst, nb, INV, stream);
          break;
        }
        case REAL_FUSED: {
          cpx<T>* b = a + chunk * (n_ / 2);
          rin_->inner().exec(src, a, nb, FWD, stream);
          sweep(RESAMPLE_UNTANGLE, a, b, nb, stream);
          rout_->inner().exec(b, dst, nb, INV, stream);
          break;
        }
      }
    });
  }

 private:
  void set_fusion(bool on) {
    route_ = !real_ ? COMPLEX : (on && has_fused_) ? REAL_FUSED : REAL_COMPOSED;
    switch (route_) {
      case COMPLEX: desc_ = std::string("resample complex: ") + pin_->describe() + "; inverse: " + pout_->describe(); break;
      case REAL_COMPOSED: desc_ = std::string("resample real composed: ") + rin_->describe() + "; inverse: " + rout_->describe(); break;
      case REAL_FUSED:
        desc_ = std::string("resample real fused untangle: ") + rin_->inner().describe() + "; inverse: " + rout_->inner().describe();
        break;
    }
  }
  // scratch bytes per row of a chunk: the spectrum of a complex row; the two half spectra of a real row (one size for both real
  // routes: the fused one's two inner rows are an element shorter each)
  size_t row_bytes() const { return real_ ? (n_ / 2 + 1 + m_ / 2 + 1) * ELEM : n_ * ELEM; }

  // resample_remap_kernel or resample_untangle_kernel over nb rows, in launches of at most REAL_LAUNCH_BYTES per side
  void sweep(int which, const void* in, void* out, size_t nb, hipStream_t stream) const {
    const bool fused = which == RESAMPLE_UNTANGLE;
    const size_t ivals = fused ? n_ / 2 : real_ ? n_ / 2 + 1 : n_, ovals = fused ? m_ / 2 : real_ ? m_ / 2 + 1 : m_;
    const size_t irow = ivals * ELEM, orow = ovals * ELEM;
    const size_t rows_per = std::max<size_t>(1, launch_bytes_ / std::max(irow, orow));
    const size_t k = std::min(n_, m_);
    const size_t lanes = fused ? ovals / 2 + 1 : ovals;  // per row
    for (size_t r0 = 0; r0 < nb; r0 += rows_per) {
      const size_t rows = std::min(rows_per, nb - r0);
      ResampleArgs a{};
      a.in = (const char*)in + r0 * irow;
      a.out = (char*)out + r0 * orow;
      a.win = has_win_ ? win_.p : nullptr;
      if (fused) { a.tw_in = rin_->twiddles(); a.tw_out = rout_->twiddles(); }
      a.n = (uint32_t)n_; a.m = (uint32_t)m_;
      a.irow = (uint32_t)ivals; a.orow = (uint32_t)ovals;
      a.kh = (uint32_t)(k / 2);
      a.even = k % 2 == 0;
      a.mode = m_ == n_ ? RESAMPLE_SAME : m_ < n_ ? RESAMPLE_DOWN : RESAMPLE_UP;
      a.half = real_;
      a.pairs = (uint32_t)lanes;
      a.total = (uint32_t)(rows * lanes);
      divider((uint32_t)lanes, a.div_m, a.div_l);
      a.in_bytes = (uint32_t)(rows * irow);
      a.out_bytes = (uint32_t)(rows * orow);
      a.nyq = a.mode == RESAMPLE_SAME ? 1.0 : a.mode == RESAMPLE_DOWN ? 2.0 : 0.5;
      a.scale = code_scale<T>(::fourier::c::FOURIER_TRANSFORM_IFFT, (T)n_);  // M/N times the inverse's 1/M
      FOURIER_LAUNCH(get_resample_kernel(Real<T>{}, which), (a.total + 255) / 256, 256, 0, stream, a);
    }
  }

  size_t n_, m_;
  bool real_;
  int device_ = 0;
  std::unique_ptr<Plan<T>> pin_, pout_;       // complex rows: the N-point forward plan, the M-point inverse
  std::unique_ptr<RealPlan<T>> rin_, rout_;   // real rows: the same pair
  bool has_fused_ = false;
  Route route_ = COMPLEX;
  DevBuf win_;
  bool has_win_ = false;
  mutable DevBuf scratch_;
  size_t scratch_cap_ = REAL_SCRATCH_BYTES;
  size_t launch_bytes_ = REAL_LAUNCH_BYTES;  // of either side of one sweep launch (development switch FOURIER_LAUNCH_BYTES)
};

}  // namespace fourier_hip
