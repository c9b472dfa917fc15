// hilbert_plan.h -- the plan behind an analytic-signal handle (fourier_hip_hilbert_*, include/fourier.h): of batched rows of N reals x
// the analytic signal
//   z = ifft(fft(x) (.) m),  m[k] = 1 for k = 0 and (N even) k = N/2, 2 for 0 < k < N/2, 0 above        (scipy.signal.hilbert),
// N complex values per row with Re z = x, or its magnitude |z|, the envelope, N reals per row.  Built on a RealPlan<T>(N) and a complex
// Plan<T>(N) that run unchanged.  Routes, chosen at create:
//   "hilbert one-launch"  a one-launch two-level plan (2^11 ... 2^15, f64 ... 2^14): load the reals, FFT, multiplier from the bin index,
//                         inverse FFT, store z or |z| in ONE launch on register-resident data (hilbert_small_kernel,
//                         Plan::exec_hilbert); no scratch
//   "hilbert composed"    any N: RealPlan forward -> half-spectrum scratch (N/2 + 1 values a row), hilbert_expand_kernel -> the row's N
//                         values X[k] m[k] / N straight into the caller's output, the plan's unscaled inverse in place there.  The
//                         envelope expands into a second scratch array of N complex values a row, runs the inverse there, and
//                         hilbert_abs_kernel writes |z|
// Option "fusion" = 1 selects the one-launch route where the length has one, 0 (the default: no measured comparison of the two routes
// exists) the composed route.  The sweeps are kernels_hilbert.h.  The batch is walked in chunks so that the
// plan-owned scratch stays bounded; one chunk size serves both entry points, so that reserve covers both.
#pragma once
#include "plan.h"
#include "real_plan.h"

namespace fourier_hip {

// The scratch bound of a HilbertPlan is RealPlan's (REAL_SCRATCH_BYTES).  The experiments library and the emulator build read
// FOURIER_HILBERT_SCRATCH_BYTES at create instead (the chunk-walk test).
template <typename T> class HilbertPlan : public HandleBase {
 public:
  static constexpr size_t ELEM = sizeof(cpx<T>);
  enum Route { ONE_LAUNCH, COMPOSED };

  HilbertPlan(size_t n, int device) : n_(n), h_(n / 2) {
    if (n == 0) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "size 0 is invalid");
    if (n * ELEM > REAL_LAUNCH_BYTES) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "analytic signals above 2^31 bytes per row");
    rplan_.reset(new RealPlan<T>(n, device));
    plan_.reset(new Plan<T>(n, device));
    device_ = plan_->device();
    {
      DeviceGuard g(device_);
      has_fused_ = plan_->enable_hilbert();
    }
    scratch_cap_ = scratch_bound("FOURIER_HILBERT_SCRATCH_BYTES", REAL_SCRATCH_BYTES);
    launch_bytes_ = launch_bound("FOURIER_LAUNCH_BYTES", REAL_LAUNCH_BYTES);
    launch_items_ = launch_bound("FOURIER_LAUNCH_ITEMS", (size_t)1 << 30);
    set_fusion(false);
  }

  size_t size() const { return n_; }
  int device() const { return device_; }

  int set_option(const std::string& key, long long v) {
    if (key == "fusion" && (v == 0 || v == 1)) { set_fusion(v == 1); return ::fourier::c::FOURIER_HIP_OK; }
    return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
  }

  // rows per chunk for a call of `batch` rows; sizes the scratch and the plans' buffers for it
  size_t prepare(size_t batch) const {
    if (batch == 0) return 0;
    if (route_ == ONE_LAUNCH) return batch;  // no scratch, no plan buffers
    const size_t per = row_bytes();
    const size_t chunk = chunk_rows(batch, scratch_cap_, per);
    DeviceGuard g(device_);
    scratch_.ensure(chunk * per);
    rplan_->reserve(chunk);
    plan_->reserve_for(chunk, true);
    return chunk;
  }
  void reserve(size_t batch) const { (void)prepare(batch); }

  // z: `batch` rows of N complex values at d_out, apart from the input
  void analytic(const void* d_in, void* d_out, size_t batch, hipStream_t stream) const {
    check_buffers(d_in, d_out, batch * n_ * sizeof(T), batch * n_ * ELEM, sizeof(T), false);
    if ((uintptr_t)d_out % ELEM) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "misaligned buffer");
    run(d_in, d_out, batch, false, stream);
  }
  // |z|: `batch` rows of N reals at d_out, which may be d_in
  void envelope(const void* d_in, void* d_out, size_t batch, hipStream_t stream) const {
    check_buffers(d_in, d_out, batch * n_ * sizeof(T), batch * n_ * sizeof(T), sizeof(T), true);
    run(d_in, d_out, batch, true, stream);
  }

 private:
  void run(const void* d_in, void* d_out, size_t batch, bool envelope, hipStream_t stream) const {
    if (batch == 0) return;
    DeviceGuard g(device_);
    const size_t chunk = prepare(batch);
    const T* in = (const T*)d_in;
    if (route_ == ONE_LAUNCH) {  // one workgroup a row: launches of less than 2^31 workgroups
      const size_t orow = n_ * (envelope ? sizeof(T) : ELEM);
      for_chunks(batch, launch_items_, [&](size_t c0, size_t nb) {
        plan_->exec_hilbert(in + c0 * n_, (char*)d_out + c0 * orow, nb, envelope, stream);
      });
      return;
    }
    cpx<T>* half = (cpx<T>*)scratch_.p;          // the half spectra of a chunk
    cpx<T>* work = half + chunk * (h_ + 1);      // envelope: the analytic signal of a chunk
    for_chunks(batch, chunk, [&](size_t c0, size_t nb) {
      rplan_->run_forward(in + c0 * n_, half, nb, ::fourier::c::FOURIER_TRANSFORM_FFT, stream);
      cpx<T>* z = envelope ? work : (cpx<T>*)d_out + c0 * n_;
      sweep(HILBERT_EXPAND, half, z, nb, stream);
      plan_->exec(z, z, nb, ::fourier::c::FOURIER_TRANSFORM_UNSCALED_IFFT, stream);
      if (envelope) sweep(HILBERT_ABS, work, (T*)d_out + c0 * n_, nb, stream);
    });
  }

  void set_fusion(bool on) {
    route_ = on && has_fused_ ? ONE_LAUNCH : COMPOSED;
    if (route_ == ONE_LAUNCH) desc_ = std::string("hilbert one-launch: ") + plan_->describe();
    else desc_ = std::string("hilbert composed: ") + rplan_->describe() + "; inverse: " + plan_->describe();
  }
  // scratch bytes per row of a chunk on the composed route: the half spectrum and the envelope's analytic signal
  size_t row_bytes() const { return (h_ + 1 + n_) * ELEM; }

  // hilbert_expand_kernel (rows of N/2 + 1 -> rows of N) or hilbert_abs_kernel (rows of N complex values -> rows of N reals) over nb
  // rows, in launches of at most REAL_LAUNCH_BYTES of the complex side
  void sweep(int which, const void* in, void* out, size_t nb, hipStream_t stream) const {
    const size_t rows_per = std::max<size_t>(1, launch_bytes_ / (n_ * ELEM));
    const bool expand = which == HILBERT_EXPAND;
    const size_t irow = (expand ? h_ + 1 : n_) * ELEM, orow = n_ * (expand ? ELEM : sizeof(T));
    for (size_t r0 = 0; r0 < nb; r0 += rows_per) {
      const size_t rows = std::min(rows_per, nb - r0);
      HilbertArgs a{};
      a.in = (const char*)in + r0 * irow;
      a.out = (char*)out + r0 * orow;
      a.n = (uint32_t)n_;
      a.h = (uint32_t)h_;
      a.total = (uint32_t)(rows * n_);
      divider(a.n, a.div_m, a.div_l);
      a.in_bytes = (uint32_t)(rows * irow);
      a.out_bytes = (uint32_t)(rows * orow);
      a.scale = code_scale<T>(::fourier::c::FOURIER_TRANSFORM_IFFT, (T)n_);  // the inverse's 1/N, folded into the multiplier
      FOURIER_LAUNCH(get_hilbert_kernel(Real<T>{}, which), (a.total + 255) / 256, 256, 0, stream, a);
    }
  }

  size_t n_, h_;
  int device_ = 0;
  std::unique_ptr<RealPlan<T>> rplan_;  // the forward transform of the composed route
  std::unique_ptr<Plan<T>> plan_;       // its inverse; the one-launch route runs on this plan's tables
  bool has_fused_ = false;
  Route route_ = COMPOSED;
  mutable DevBuf scratch_;
  size_t scratch_cap_ = REAL_SCRATCH_BYTES;
  size_t launch_bytes_ = REAL_LAUNCH_BYTES;  // of either side of one sweep launch (development switch FOURIER_LAUNCH_BYTES)
  size_t launch_items_ = (size_t)1 << 30;  // rows of the one-launch route of one launch (development switch FOURIER_LAUNCH_ITEMS)
};

}  // namespace fourier_hip
