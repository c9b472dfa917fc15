// conv_plan.h -- the plan behind a convolution handle (fourier_hip_conv_*, include/fourier.h): batched circular convolution or
// correlation of rows of N elements with a prepared bank of F filters, row b with filter b mod F,
//   y[b] = ifft(fft(x[b]) * H[b mod F]),  H[f] = fft(h[f], N) / N  (conjugated for a correlation),
// built on a complex Plan<T> (complex data) or a RealPlan<T> (real data) that run unchanged.  Routes, chosen at create:
//   complex  "conv one-launch"        a one-launch two-level plan (2^11 ... 2^15, f64 ... 2^14): load, FFT, product, inverse FFT, store in ONE
//                                     launch on register-resident data (conv_small_kernel, Plan::exec_conv); no scratch
//            "conv fused passes"      a power-of-two plan of two or more tile passes: forward passes 0 ... np-2, fft_conv_kernel with
//                                     the bank (last forward pass, product, first inverse pass), inverse passes 1 ... np-1
//                                     (Plan::exec_conv); the spectrum never reaches HBM
//            "conv composed"          any N: plan forward -> scratch, conv_mul_kernel in place, plan unscaled inverse -> out
//   real     "conv real fused untangle"  even N: inner N/2-point plan forward -> scratch, ONE real_conv_mid_kernel sweep (untangle,
//                                     product with the half spectrum, retangle) in place, inner plan unscaled inverse -> out
//            "conv real composed"     odd N: RealPlan forward -> half-spectrum scratch, conv_mul_kernel, RealPlan unscaled inverse
// Option "fusion" = 0 selects the composed route of the kind.  The sweeps are kernels_conv.h.  The batch is walked in chunks so
// that the plan-owned scratch stays bounded; the filter of a row counts over the whole call.
#pragma once
#include "plan.h"
#include "real_plan.h"

namespace fourier_hip {

// The scratch bound of a ConvPlan is RealPlan's (REAL_SCRATCH_BYTES): rows per chunk such that the scratch stays at most this many
// bytes, never less than one row.  The experiments library and the emulator build read FOURIER_CONV_SCRATCH_BYTES at create instead
// (the chunk-walk test).
template <typename T> class ConvPlan : public HandleBase {
 public:
  static constexpr size_t ELEM = sizeof(cpx<T>);
  enum Route { ONE_LAUNCH, FUSED_PASSES, COMPOSED, REAL_FUSED, REAL_COMPOSED };

  ConvPlan(size_t n, bool real_data, int device) : n_(n), h_(n / 2), real_(real_data) {
    if (n == 0) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "size 0 is invalid");
    if (real_) {
      rplan_.reset(new RealPlan<T>(n, device));
      device_ = rplan_->inner().device();
      blen_ = h_ + 1;
    } else {
      if (n * ELEM > REAL_LAUNCH_BYTES) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "convolutions above 2^31 bytes per row");
      plan_.reset(new Plan<T>(n, device));
      device_ = plan_->device();
      blen_ = n;
      DeviceGuard g(device_);
      fused_route_ = plan_->enable_conv_bank();
    }
    scratch_cap_ = scratch_bound("FOURIER_CONV_SCRATCH_BYTES", REAL_SCRATCH_BYTES);
    launch_bytes_ = launch_bound("FOURIER_LAUNCH_BYTES", REAL_LAUNCH_BYTES);
    set_fusion(true);
  }

  size_t size() const { return n_; }
  size_t filters() const { return filters_; }
  int device() const { return device_; }

  int set_option(const std::string& key, long long v) {
    if (key == "fusion" && (v == 0 || v == 1)) { set_fusion(v == 1); return ::fourier::c::FOURIER_HIP_OK; }
    return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
  }

  // rows per chunk for a call of `batch` rows; sizes the scratch and the inner plan's buffers for it
  size_t prepare(size_t batch) const {
    if (batch == 0) return 0;
    if (route_ == ONE_LAUNCH) return batch;  // no scratch, no plan buffers
    const size_t per = row_bytes();
    const size_t chunk = chunk_rows(batch, scratch_cap_, per);
    DeviceGuard g(device_);
    scratch_.ensure(chunk * per);
    if (route_ == REAL_COMPOSED) rplan_->reserve(chunk);
    else if (route_ == REAL_FUSED) rplan_->inner().reserve_for(chunk, false);
    else if (route_ == COMPOSED) plan_->reserve_for(chunk, false);
    return chunk;
  }
  void reserve(size_t batch) const { (void)prepare(batch); }

  // `filters` rows of `taps` values (complex handle: complex, real handle: real) at d_taps -> the bank, on `stream`
  void set_filters(const void* d_taps, size_t taps, size_t filters, bool correlate, hipStream_t stream) {
    if (!d_taps) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "null taps");
    if ((uintptr_t)d_taps % (real_ ? sizeof(T) : ELEM)) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "misaligned taps");
    if (taps == 0 || taps > n_ || filters == 0) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "taps outside 1 ... N, or no filters");
    if (filters > 0x7fffffffull) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "more than 2^31 filters");
    DeviceGuard g(device_);
    bank_.ensure(filters * blen_ * ELEM);
    // the zero-extended taps of a chunk of filters in the scratch (a row of N values fits a scratch row on every route), the plan's
    // own forward transform in T into the bank, then 1/N and the conjugate in place
    const size_t words = real_ ? 1 : 2;
    const size_t per = real_ ? (h_ + 1) * ELEM : n_ * ELEM;  // (N reals fit N/2 + 1 complex)
    const size_t chunk = chunk_rows(filters, scratch_cap_, per);
    scratch_.ensure(chunk * per);
    if (real_) rplan_->reserve(chunk);  // (RealPlan's own scratch: rows of the filter transforms, kept)
    else plan_->reserve_for(chunk, false);
    cpx<T>* bank = (cpx<T>*)bank_.p;
    for_chunks(filters, chunk, [&](size_t f0, size_t nf) {
      ConvArgs a{};
      a.in = (const T*)d_taps + f0 * taps * words;
      a.out = scratch_.p;
      a.n = n_ * words; a.taps = taps * words; a.rows = nf;
      FOURIER_LAUNCH(get_conv_sweep_kernel(Real<T>{}, CONV_PAD), elementwise_grid(nf * n_ * words), 256, 0, stream, a);
      if (real_) rplan_->run_forward(scratch_.p, bank + f0 * blen_, nf, ::fourier::c::FOURIER_TRANSFORM_FFT, stream);
      else plan_->exec(scratch_.p, bank + f0 * blen_, nf, ::fourier::c::FOURIER_TRANSFORM_FFT, stream);
    });
    ConvArgs a{};
    a.out = bank;
    a.count = filters * blen_;
    a.scale = code_scale<T>(::fourier::c::FOURIER_TRANSFORM_IFFT, (T)n_);  // the inverse's 1/N, folded into the bank
    a.conj = correlate;
    FOURIER_LAUNCH(get_conv_sweep_kernel(Real<T>{}, CONV_FINISH), elementwise_grid(a.count), 256, 0, stream, a);
    filters_ = filters;
  }

  // first: the index the call's first row counts its filter from (the linear-convolution handle walks its own chunks)
  void apply(const void* d_in, void* d_out, size_t batch, hipStream_t stream, size_t first = 0) const {
    const size_t row = n_ * (real_ ? sizeof(T) : ELEM);
    check_buffers(d_in, d_out, batch * row, batch * row, ELEM, true);
    if (filters_ == 0) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "no filters set");
    if (batch == 0) return;
    DeviceGuard g(device_);
    const size_t chunk = prepare(batch);
    const char* in = (const char*)d_in;
    char* out = (char*)d_out;
    cpx<T>* work = (cpx<T>*)scratch_.p;
    const cpx<T>* bank = (const cpx<T>*)bank_.p;
    const int FWD = ::fourier::c::FOURIER_TRANSFORM_FFT, INV = ::fourier::c::FOURIER_TRANSFORM_UNSCALED_IFFT;
    for_chunks(batch, chunk, [&](size_t c0, size_t nb) {
      const void* src = in + c0 * row;
      void* dst = out + c0 * row;
      const size_t b0 = first + c0;
      switch (route_) {
        case ONE_LAUNCH:
          plan_->exec_conv(src, dst, nb, bank, filters_, b0, nullptr, nullptr, stream);
          break;
        case FUSED_PASSES:
          plan_->exec_conv(src, dst, nb, bank, filters_, b0, work, work + chunk * n_, stream);
          break;
        case COMPOSED:
          plan_->exec(src, work, nb, FWD, stream);
          sweep(CONV_MUL, work, nb, n_, b0, stream);
          plan_->exec(work, dst, nb, INV, stream);
          break;
        case REAL_FUSED:
          rplan_->inner().exec(src, work, nb, FWD, stream);
          sweep(CONV_REAL_MID, work, nb, h_, b0, stream);
          rplan_->inner().exec(work, dst, nb, INV, stream);
          break;
        case REAL_COMPOSED:
          rplan_->run_forward(src, work, nb, FWD, stream);
          sweep(CONV_MUL, work, nb, h_ + 1, b0, stream);
          rplan_->run_inverse(work, dst, nb, INV, stream);
          break;
      }
    });
  }

 private:
  void set_fusion(bool on) {
    if (real_) route_ = (on && rplan_->even()) ? REAL_FUSED : REAL_COMPOSED;
    else route_ = !on ? COMPOSED : fused_route_ == Plan<T>::CONV_ONE_LAUNCH ? ONE_LAUNCH : fused_route_ == Plan<T>::CONV_PASSES ? FUSED_PASSES : COMPOSED;
    switch (route_) {
      case ONE_LAUNCH: desc_ = std::string("conv one-launch: ") + plan_->describe(); break;
      case FUSED_PASSES: desc_ = std::string("conv fused passes: ") + plan_->describe(); break;
      case COMPOSED: desc_ = std::string("conv composed: ") + plan_->describe(); break;
      case REAL_FUSED: desc_ = std::string("conv real fused untangle: ") + rplan_->inner().describe(); break;
      case REAL_COMPOSED: desc_ = std::string("conv real composed: ") + rplan_->describe(); break;
    }
  }
  // scratch bytes per row of a chunk on the current route: the two work arrays of the fused passes, the spectrum of the composed route,
  // the inner plan's output (real, fused) or the half spectrum (real, composed; one size for both real routes)
  size_t row_bytes() const { return real_ ? (h_ + 1) * ELEM : (route_ == FUSED_PASSES ? 2 : 1) * n_ * ELEM; }

  // conv_mul_kernel (len values per row) or real_conv_mid_kernel (rows of len = h) over nb rows of the scratch, in launches of at
  // most REAL_LAUNCH_BYTES; b0: the first row's index in the call
  void sweep(int which, cpx<T>* z, size_t nb, size_t len, size_t b0, hipStream_t stream) const {
    const size_t rows_per = std::max<size_t>(1, launch_bytes_ / (len * ELEM));
    const uint32_t lanes = which == CONV_REAL_MID ? (uint32_t)(len / 2 + 1) : (uint32_t)len;
    for (size_t r0 = 0; r0 < nb; r0 += rows_per) {
      const size_t rows = std::min(rows_per, nb - r0);
      ConvArgs a{};
      a.in = a.out = z + r0 * len;
      a.tw = which == CONV_REAL_MID ? rplan_->twiddles() : nullptr;
      a.bank = bank_.p;
      a.h = (uint32_t)h_;
      a.len = lanes;
      a.total = (uint32_t)(rows * lanes);
      divider(lanes, a.div_m, a.div_l);
      a.filters = (uint32_t)filters_;
      a.first = (uint32_t)((b0 + r0) % filters_);
      divider(a.filters, a.f_m, a.f_l);
      a.bytes = (uint32_t)(rows * len * ELEM);
      FOURIER_LAUNCH(get_conv_sweep_kernel(Real<T>{}, which), (a.total + 255) / 256, 256, 0, stream, a);
    }
  }

  size_t n_, h_;
  bool real_;
  int device_ = 0;
  std::unique_ptr<Plan<T>> plan_;       // complex data
  std::unique_ptr<RealPlan<T>> rplan_;  // real data: set_filters and the composed route; its inner plan and twiddles run the fused route
  int fused_route_ = 0;                 // Plan::CONV_NONE ...: what "fusion" = 1 runs on complex data
  Route route_ = COMPOSED;
  size_t blen_ = 0;                     // complex values per filter of the bank: N, real data N/2 + 1
  size_t filters_ = 0;
  DevBuf bank_;
  mutable DevBuf scratch_;
  size_t scratch_cap_ = REAL_SCRATCH_BYTES;
  size_t launch_bytes_ = REAL_LAUNCH_BYTES;  // of either side of one sweep launch (development switch FOURIER_LAUNCH_BYTES)
};

}  // namespace fourier_hip
