// real_plan.h -- the plan behind a real-input handle (fourier_hip_real_*, include/fourier.h): batched real-to-half-spectrum and
// half-spectrum-to-real transforms, numpy's rfft / irfft layout, built on an inner complex Plan<T> that runs unchanged.
//
//   even N = 2h  forward: the reals as h complex values -> inner h-point FFT -> scratch -> real_post_kernel -> X (rows of h + 1)
//                inverse: X -> real_pre_kernel (scale folded in) -> scratch -> inner h-point UNSCALED_IFFT -> the reals (h complex)
//   odd N        forward: widen -> scratch -> inner N-point transform in place (the code's scale) -> narrow -> X
//                inverse: Hermitian extension -> scratch -> inner N-point inverse in place -> real parts
// The even path's untangle sweeps are kernels_real.h.  The batch is walked in chunks so that the plan-owned scratch stays bounded.
#pragma once
#include "plan.h"

namespace fourier_hip {

// Scratch bound of a RealPlan: rows of the inner transform per chunk such that the scratch stays at most this many bytes (never
// less than one row).  f32 N = 2^20 x 4096, r2c / c2r ms per call (profiles/real_fft/real_fft_bench.jsonl, alternating arms): 256 MiB
// 19.83 / 19.94, 1 GiB 17.99 / 18.03, the whole batch (16 GiB of scratch) 17.01 / 17.46.  The whole batch is 3 - 5 % faster (fewer
// chunk tails of the inner plan) but holds 16 GiB of device memory the caller does not get back; 1 GiB keeps the scratch a small
// fraction of the HBM at 0.78 x the complex transform ("Real-input transforms").  The experiments library and
// the emulator build read FOURIER_REAL_SCRATCH_BYTES at create instead (the A/B and the chunk-walk test).
constexpr size_t REAL_SCRATCH_BYTES = (size_t)1 << 30;
// Bytes of either side of one untangle launch: the sweeps address with 31-bit byte offsets (one launch covers a whole chunk of the
// default scratch bound; a row may take at most half of it, RealPlan's constructor)
constexpr size_t REAL_LAUNCH_BYTES = ((size_t)1 << 31) - 1;

template <typename T> class RealPlan : public HandleBase {
 public:
  static constexpr size_t ELEM = sizeof(cpx<T>);

  RealPlan(size_t n, int device) : n_(n), h_(n / 2), even_(n % 2 == 0) {
    if (n == 0) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "size 0 is invalid");
    if ((h_ + 1) * ELEM > REAL_LAUNCH_BYTES / 2) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "real transforms above 2^30 bytes of half spectrum");
    inner_.reset(new Plan<T>(even_ ? h_ : n_, device));
    DeviceGuard g(inner_->device());
    if (even_) tw_.upload(real_untangle_twiddles<T>(n_));
    scratch_cap_ = scratch_bound("FOURIER_REAL_SCRATCH_BYTES", REAL_SCRATCH_BYTES);
    launch_bytes_ = launch_bound("FOURIER_LAUNCH_BYTES", REAL_LAUNCH_BYTES);
    desc_ = std::string(even_ ? "real half-length: " : "real full-length: ") + inner_->describe();
  }

  size_t size() const { return n_; }
  // the pieces the convolution handle's fused untangle route runs by itself (conv_plan.h): the inner plan, W_N^j (even N)
  bool even() const { return even_; }
  const Plan<T>& inner() const { return *inner_; }
  const void* twiddles() const { return tw_.p; }
  // the fused frame route of the STFT / spectrogram / filter bank handle (Args = StftArgs / SpectrogramArgs / PfbArgs; stft_plan.h,
  // spectrogram_plan.h, pfb_plan.h): even N
  // whose inner plan is one whole-row pass with a kernel for it
  template <typename Args> bool enable_frames() { return even_ && inner_->template enable_frames<Args>(); }

  // rows per chunk for a call of `batch` rows; sizes the scratch and the inner plan's buffers for it (reserve: ahead of time, so
  // that later calls of at most `batch` rows never allocate)
  size_t prepare(size_t batch) const {
    if (batch == 0) return 0;
    const size_t per = (even_ ? h_ : n_) * ELEM;
    const size_t chunk = chunk_rows(batch, scratch_cap_, per);
    DeviceGuard g(inner_->device());
    scratch_.ensure(chunk * per);
    inner_->reserve_for(chunk, !even_);
    return chunk;
  }
  void reserve(size_t batch) const { (void)prepare(batch); }

  void forward(const void* d_in, void* d_out, size_t batch, int code, hipStream_t stream) const {
    check_buffers(d_in, d_out, batch * n_ * sizeof(T), batch * (h_ + 1) * ELEM, ELEM, false);
    if (!is_forward(code)) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "not a forward transform code");
    run_forward(d_in, d_out, batch, code, stream);
  }
  // forward / inverse after the argument checks (RealNdPlan's composed route runs rows of odd N whose reals start on any T)
  void run_forward(const void* d_in, void* d_out, size_t batch, int code, hipStream_t stream) const {
    if (batch == 0) return;
    DeviceGuard g(inner_->device());
    const size_t chunk = prepare(batch);
    const double scale = code_scale<T>(code, (T)n_);
    const T* in = (const T*)d_in;
    cpx<T>* out = (cpx<T>*)d_out;
    cpx<T>* work = (cpx<T>*)scratch_.p;
    for_chunks(batch, chunk, [&](size_t b0, size_t nb) {
      if (even_) {
        inner_->exec(in + b0 * n_, work, nb, ::fourier::c::FOURIER_TRANSFORM_FFT, stream);
        sweep(REAL_POST, work, out + b0 * (h_ + 1), nb, scale, stream);
      } else {
        odd_sweep(REAL_WIDEN, in + b0 * n_, work, nb, stream);
        inner_->exec(work, work, nb, code, stream);
        odd_sweep(REAL_NARROW, work, out + b0 * (h_ + 1), nb, stream);
      }
    });
  }

  void inverse(const void* d_in, void* d_out, size_t batch, int code, hipStream_t stream) const {
    check_buffers(d_in, d_out, batch * (h_ + 1) * ELEM, batch * n_ * sizeof(T), ELEM, false);
    if (!is_inverse(code)) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "not an inverse transform code");
    run_inverse(d_in, d_out, batch, code, stream);
  }
  void run_inverse(const void* d_in, void* d_out, size_t batch, int code, hipStream_t stream) const {
    if (batch == 0) return;
    DeviceGuard g(inner_->device());
    const size_t chunk = prepare(batch);
    // the code's scale over N: the inner h-point IFFT runs unscaled and returns h (x[2m] + i x[2m+1]) times what the sweep wrote,
    // and the sweep's S +- iT carry a factor 2
    const double fac = code_scale<T>(code, (T)n_);
    const cpx<T>* in = (const cpx<T>*)d_in;
    T* out = (T*)d_out;
    cpx<T>* work = (cpx<T>*)scratch_.p;
    for_chunks(batch, chunk, [&](size_t b0, size_t nb) {
      if (even_) {
        sweep(REAL_PRE, in + b0 * (h_ + 1), work, nb, fac, stream);
        inner_->exec(work, out + b0 * n_, nb, ::fourier::c::FOURIER_TRANSFORM_UNSCALED_IFFT, stream);
      } else {
        odd_sweep(REAL_EXTEND, in + b0 * (h_ + 1), work, nb, stream);
        inner_->exec(work, work, nb, code, stream);
        odd_sweep(REAL_PART, work, out + b0 * n_, nb, stream);
      }
    });
  }

 private:
  // the untangle sweep over nb rows, in launches of at most REAL_LAUNCH_BYTES per side
  void sweep(int which, const cpx<T>* in, cpx<T>* out, size_t nb, double scale, hipStream_t stream) const {
    const size_t zrow = h_ * ELEM, xrow = (h_ + 1) * ELEM;
    const size_t rows_per = std::max<size_t>(1, launch_bytes_ / xrow);
    const uint32_t pairs = (uint32_t)(h_ / 2 + 1);
    for (size_t r0 = 0; r0 < nb; r0 += rows_per) {
      const size_t rows = std::min(rows_per, nb - r0);
      RealArgs a{};
      const bool post = which == REAL_POST;
      a.in = post ? (const void*)(in + r0 * h_) : (const void*)(in + r0 * (h_ + 1));
      a.out = post ? (void*)(out + r0 * (h_ + 1)) : (void*)(out + r0 * h_);
      a.tw = tw_.p;
      a.h = (uint32_t)h_;
      a.pairs = pairs;
      a.total = (uint32_t)(rows * pairs);
      divider(pairs, a.div_m, a.div_l);
      a.in_bytes = (uint32_t)(rows * (post ? zrow : xrow));
      a.out_bytes = (uint32_t)(rows * (post ? xrow : zrow));
      a.scale = scale;
      FOURIER_LAUNCH(get_real_kernel(Real<T>{}, which), (a.total + 255) / 256, 256, 0, stream, a);
    }
  }
  void odd_sweep(int which, const void* in, void* out, size_t nb, hipStream_t stream) const {
    RealArgs a{};
    a.in = in;
    a.out = out;
    a.n = n_;
    a.rows = nb;
    FOURIER_LAUNCH(get_real_kernel(Real<T>{}, which), elementwise_grid(nb * n_), 256, 0, stream, a);
  }

  size_t n_, h_;
  bool even_;
  std::unique_ptr<Plan<T>> inner_;
  DevBuf tw_;
  mutable DevBuf scratch_;
  size_t scratch_cap_ = REAL_SCRATCH_BYTES;
  size_t launch_bytes_ = REAL_LAUNCH_BYTES;  // of either side of one untangle launch (development switch FOURIER_LAUNCH_BYTES)
};

}  // namespace fourier_hip
