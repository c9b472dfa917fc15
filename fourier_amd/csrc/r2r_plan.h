// r2r_plan.h -- the plan behind a real-to-real handle (fourier_hip_r2r_*, include/fourier.h): batched DCT-II / DCT-III / DST-II /
// DST-III, scipy's definitions and norms, rows of N reals in and out, built on an inner complex Plan<T> that runs unchanged.
//
//   even N = 2h  type II:  x -> r2r_pack_kernel -> scratch A -> inner h-point FFT -> scratch B -> r2r_post_kernel -> X
//                type III: X -> r2r_pre_kernel (norm folded in) -> scratch A -> inner h-point UNSCALED_IFFT -> scratch B ->
//                          r2r_unpack_kernel -> x
//   odd N        type II:  widen with the permutation -> scratch -> inner N-point FFT in place -> post -> X
//                type III: pre (all N values, Hermitian by construction) -> scratch -> inner N-point UNSCALED_IFFT in place -> real parts
// The sweeps are kernels_r2r.h.  One handle serves the four kinds and the three norms: the tables are the same.  The batch is walked in
// chunks so that the plan-owned scratch (both halves together) stays bounded; a chunk is read completely into the scratch before any
// of its rows is written, so d_in == d_out is allowed.
#pragma once
#include "real_plan.h"

namespace fourier_hip {

template <typename T> class R2RPlan : public HandleBase {
 public:
  static constexpr size_t ELEM = sizeof(cpx<T>);

  R2RPlan(size_t n, int device) : n_(n), h_(n / 2), even_(n % 2 == 0) {
    if (n == 0) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "size 0 is invalid");
    if ((h_ + 1) * ELEM > REAL_LAUNCH_BYTES / 2) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "real-to-real transforms above 2^30 bytes per row");
    inner_.reset(new Plan<T>(even_ ? h_ : n_, device));
    DeviceGuard g(inner_->device());
    if (even_) tw_.upload(real_untangle_twiddles<T>(n_));
    std::vector<cpx<T>> ct(even_ ? h_ + 1 : n_);  // c_j = exp(-i pi j / 2N) = W_4N^j
    for (size_t j = 0; j < ct.size(); ++j) ct[j] = root<T>(j, 4 * (uint64_t)n_);
    ct_.upload(ct);
    scratch_cap_ = scratch_bound("FOURIER_REAL_SCRATCH_BYTES", REAL_SCRATCH_BYTES);
    launch_bytes_ = launch_bound("FOURIER_LAUNCH_BYTES", REAL_LAUNCH_BYTES);
    desc_ = std::string(even_ ? "r2r half-length: " : "r2r full-length: ") + inner_->describe();
  }

  size_t size() const { return n_; }

  // rows per chunk for a call of `batch` rows; sizes the scratch and the inner plan's buffers for it (reserve: ahead of time, so
  // that later calls of at most `batch` rows never allocate)
  size_t prepare(size_t batch) const {
    if (batch == 0) return 0;
    const size_t per = even_ ? 2 * h_ * ELEM : n_ * ELEM;  // even N: the inner plan runs from one half of the scratch into the other
    const size_t chunk = chunk_rows(batch, scratch_cap_, per);
    DeviceGuard g(inner_->device());
    scratch_.ensure(chunk * per);
    inner_->reserve_for(chunk, !even_);
    return chunk;
  }
  void reserve(size_t batch) const { (void)prepare(batch); }

  void transform(const void* d_in, void* d_out, size_t batch, int kind, int norm, hipStream_t stream) const {
    check_buffers(d_in, d_out, batch * n_ * sizeof(T), batch * n_ * sizeof(T), ELEM, true);
    if (kind < ::fourier::c::FOURIER_R2R_DCT2 || kind > ::fourier::c::FOURIER_R2R_DST3)
      throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "unknown real-to-real kind");
    if (norm < ::fourier::c::FOURIER_R2R_NORM_BACKWARD || norm > ::fourier::c::FOURIER_R2R_NORM_FORWARD)
      throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "unknown real-to-real norm");
    if (batch == 0) return;
    DeviceGuard g(inner_->device());
    const size_t chunk = prepare(batch);
    const bool type3 = kind == ::fourier::c::FOURIER_R2R_DCT3 || kind == ::fourier::c::FOURIER_R2R_DST3;
    const int sine = kind == ::fourier::c::FOURIER_R2R_DST2 || kind == ::fourier::c::FOURIER_R2R_DST3;
    const bool ortho = norm == ::fourier::c::FOURIER_R2R_NORM_ORTHO;
    // scipy: backward 1, forward 1 / 2N, ortho 1 / sqrt(2N) with element 0 of the transform side (cosine index) times 1 / sqrt 2
    // (type II, an output) or sqrt 2 (type III, an input); f64 on the host, cast by the sweep
    const double two_n = 2.0 * (double)n_;
    const double scale = ortho ? 1.0 / std::sqrt(two_n) : norm == ::fourier::c::FOURIER_R2R_NORM_FORWARD ? 1.0 / two_n : 1.0;
    const double edge = !ortho ? 1.0 : type3 ? std::sqrt(2.0) : std::sqrt(0.5);
    const T* in = (const T*)d_in;
    T* out = (T*)d_out;
    cpx<T>* wa = (cpx<T>*)scratch_.p;
    for_chunks(batch, chunk, [&](size_t b0, size_t nb) {
      const T* x = in + b0 * n_;
      T* y = out + b0 * n_;
      if (even_) {
        cpx<T>* wb = wa + chunk * h_;
        sweep(type3 ? R2R_PRE : R2R_PACK, x, wa, nb, sine, scale, edge, stream);
        inner_->exec(wa, wb, nb, type3 ? ::fourier::c::FOURIER_TRANSFORM_UNSCALED_IFFT : ::fourier::c::FOURIER_TRANSFORM_FFT, stream);
        sweep(type3 ? R2R_UNPACK : R2R_POST, wb, y, nb, sine, scale, edge, stream);
      } else {
        odd_sweep(type3 ? R2R_ODD_PRE : R2R_ODD_WIDEN, x, wa, nb, sine, scale, edge, stream);
        inner_->exec(wa, wa, nb, type3 ? ::fourier::c::FOURIER_TRANSFORM_UNSCALED_IFFT : ::fourier::c::FOURIER_TRANSFORM_FFT, stream);
        odd_sweep(type3 ? R2R_ODD_PART : R2R_ODD_POST, wa, y, nb, sine, scale, edge, stream);
      }
    });
  }

 private:
  // one even-N sweep over nb rows, in launches of at most REAL_LAUNCH_BYTES per side (a row of N reals and a row of h complex
  // values have the same size)
  void sweep(int which, const void* in, void* out, size_t nb, int sine, double scale, double edge, hipStream_t stream) const {
    const size_t row = h_ * ELEM;
    const size_t rows_per = std::max<size_t>(1, launch_bytes_ / row);
    const uint32_t lanes = (uint32_t)((which == R2R_PACK || which == R2R_UNPACK) ? (h_ + 1) / 2 : h_ / 2 + 1);
    for (size_t r0 = 0; r0 < nb; r0 += rows_per) {
      const size_t rows = std::min(rows_per, nb - r0);
      R2RArgs a{};
      a.in = (const char*)in + r0 * row;
      a.out = (char*)out + r0 * row;
      a.tw = tw_.p;
      a.ct = ct_.p;
      a.h = (uint32_t)h_;
      a.lanes = lanes;
      a.total = (uint32_t)(rows * lanes);
      divider(lanes, a.div_m, a.div_l);
      a.in_bytes = a.out_bytes = (uint32_t)(rows * row);
      a.sine = sine;
      a.scale = scale;
      a.edge = edge;
      FOURIER_LAUNCH(get_r2r_kernel(Real<T>{}, which), (a.total + 255) / 256, 256, 0, stream, a);
    }
  }
  void odd_sweep(int which, const void* in, void* out, size_t nb, int sine, double scale, double edge, hipStream_t stream) const {
    R2RArgs a{};
    a.in = in;
    a.out = out;
    a.ct = ct_.p;
    a.n = n_;
    a.rows = nb;
    a.sine = sine;
    a.scale = scale;
    a.edge = edge;
    FOURIER_LAUNCH(get_r2r_kernel(Real<T>{}, which), elementwise_grid(nb * n_), 256, 0, stream, a);
  }

  size_t n_, h_;
  bool even_;
  std::unique_ptr<Plan<T>> inner_;
  DevBuf tw_, ct_;
  mutable DevBuf scratch_;
  size_t scratch_cap_ = REAL_SCRATCH_BYTES;
  size_t launch_bytes_ = REAL_LAUNCH_BYTES;  // of either side of one sweep launch (development switch FOURIER_LAUNCH_BYTES)
};

}  // namespace fourier_hip
