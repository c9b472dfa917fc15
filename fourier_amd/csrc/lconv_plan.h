// lconv_plan.h -- the plan behind a linear-convolution handle (fourier_hip_lconv_*, include/fourier.h): batched linear convolution or
// correlation of rows of Lx values with a prepared bank of F filters of K taps, row b with filter b mod F,
//   full[b] = x[b] * h[b mod F]  (numpy.convolve, Lx + K - 1 values),  y[b] = full[b][off : off + Lout],
//   FULL: off = 0, Lout = Lx + K - 1;  SAME: off = (K - 1) / 2, Lout = Lx;  VALID: off = K - 1, Lout = Lx - K + 1.
// A correlation stores conj(h[K-1-i]) in place of h[i] when the filters are set; apply does not know about it.  Routes, chosen at create:
//   "lconv overlap-save"  a one-launch two-level plan of N = 2^11 ... 2^15 (f64 ... 2^14) points on overlapping blocks of every row
//                         (lconv_small_kernel, Plan::exec_lconv): step S = floor((N - (K - 1)) / A) * A with A the values of one
//                         128-byte line of complex data, block j loaded from j * S - (N - S) with zeros outside the row, its first
//                         N - S outputs dropped, the others stored at j * S - off where that lies in the output row.  One launch, no
//                         scratch.  Real rows: two blocks of a row as the real and the imaginary part of one complex block (the taps
//                         are real, so ifft(fft(a + i b) H) = a (*) h + i (b (*) h)); the bank is the full spectrum in both kinds.
//   "lconv padded"        filters too long for a block, or option "overlap_save" = 0: rows zero-padded into the scratch (lconv_copy_kernel),
//                         the circular handle of M = the smallest power of two >= Lx + K - 1 in place there (ConvPlan), a crop sweep
//                         to the output; the batch is walked in chunks under ConvPlan's scratch bound.
// Block rule: f32 first tries the smallest N <= 2^13 with N >= 8 (K - 1) and N < Lx + K - 1 (a row of more than one block); then, and in
// f64 at once, the smallest N with N >= 4 (K - 1); where there is none the largest N if N >= 2 (K - 1); else the padded route.  Option
// "block" = 11 ... 15 forces 2^v (0: the rule again).  A change of route or block drops the bank: set the filters again.
#pragma once
#include "conv_plan.h"

namespace fourier_hip {

template <typename T> class LinearConvPlan : public HandleBase {
 public:
  static constexpr size_t ELEM = sizeof(cpx<T>);
  static constexpr size_t LINE = 128 / ELEM;  // A: complex values of one 128-byte line
  static constexpr int K_MIN = 11, K_MAX = sizeof(T) == 4 ? 15 : 14;  // the shapes of lconv_small_kernel
  static constexpr size_t ROW_BYTES_MAX = (size_t)1 << 31;            // the kernel's descriptors and 32-bit byte offsets
  enum Route { OVERLAP_SAVE, PADDED };

  LinearConvPlan(size_t lx, size_t taps, int mode, bool real_data, int device) : lx_(lx), k_(taps), mode_(mode), real_(real_data), device_arg_(device) {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    if (lx == 0 || taps == 0) throw EngineError(INVALID, "length 0 or no taps");
    if (mode != ::fourier::c::FOURIER_LCONV_FULL && mode != ::fourier::c::FOURIER_LCONV_SAME && mode != ::fourier::c::FOURIER_LCONV_VALID)
      throw EngineError(INVALID, "unknown mode");
    if (mode == ::fourier::c::FOURIER_LCONV_VALID && taps > lx) throw EngineError(INVALID, "valid mode needs taps <= length");
    if (taps > ROW_BYTES_MAX || lx > ROW_BYTES_MAX) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "rows above 2^31 bytes");
    off_ = mode == ::fourier::c::FOURIER_LCONV_FULL ? 0 : mode == ::fourier::c::FOURIER_LCONV_SAME ? (taps - 1) / 2 : taps - 1;
    lout_ = mode == ::fourier::c::FOURIER_LCONV_FULL ? lx + taps - 1 : mode == ::fourier::c::FOURIER_LCONV_SAME ? lx : lx - taps + 1;
    val_ = real_ ? sizeof(T) : ELEM;
    if (lx * val_ > ROW_BYTES_MAX || lout_ * val_ > ROW_BYTES_MAX) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "rows above 2^31 bytes");
    scratch_cap_ = scratch_bound("FOURIER_CONV_SCRATCH_BYTES", REAL_SCRATCH_BYTES);
    launch_items_ = launch_bound("FOURIER_LAUNCH_ITEMS", LAUNCH_WORKGROUPS);
    select(0, true);
  }

  size_t length() const { return lx_; }
  size_t taps() const { return k_; }
  size_t out_length() const { return lout_; }
  size_t filters() const { return filters_; }

  int set_option(const std::string& key, long long v) {
    if (key == "block" && (v == 0 || (v >= K_MIN && v <= 15))) { select((int)v, overlap_save_); return ::fourier::c::FOURIER_HIP_OK; }
    if (key == "overlap_save" && (v == 0 || v == 1)) { select(block_opt_, v == 1); return ::fourier::c::FOURIER_HIP_OK; }
    return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
  }

  // rows per chunk of the padded route for a call of `batch` rows; sizes the scratch and the inner handle for it
  size_t prepare(size_t batch) const {
    if (batch == 0) return 0;
    if (route_ == OVERLAP_SAVE) return batch;  // no scratch
    const size_t per = m_ * val_;
    const size_t chunk = chunk_rows(batch, scratch_cap_, per);
    DeviceGuard g(device_);
    scratch_.ensure(chunk * per);
    inner_->reserve(chunk);
    return chunk;
  }
  void reserve(size_t batch) const { (void)prepare(batch); }

  // `filters` rows of K values of the handle's kind at d_taps -> the bank, on `stream`
  void set_filters(const void* d_taps, size_t filters, bool correlate, hipStream_t stream) {
    if (!d_taps) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "null taps");
    if ((uintptr_t)d_taps % val_) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "misaligned taps");
    if (filters == 0) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "no filters");
    if (filters > 0x7fffffffull) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "more than 2^31 filters");
    DeviceGuard g(device_);
    filters_ = 0;
    if (route_ == PADDED) {
      // the inner handle takes the taps as they are; a correlation hands it conj(h[K-1-i]), prepared in a buffer of its own
      const void* src = d_taps;
      if (correlate) {
        taps_.ensure(filters * k_ * val_);
        prepare_taps(d_taps, taps_.p, 0, filters, k_, true, false, stream);
        src = taps_.p;
      }
      inner_->set_filters(src, k_, filters, false, stream);
    } else {
      // the taps of a chunk of filters, zero-extended to N complex values, in the scratch; the block plan's own forward transform into the
      // bank; then the inverse's 1/N in place
      bank_.ensure(filters * n_ * ELEM);
      const size_t per = n_ * ELEM;
      const size_t chunk = chunk_rows(filters, scratch_cap_, per);
      scratch_.ensure(chunk * per);
      plan_->reserve_for(chunk, false);
      cpx<T>* bank = (cpx<T>*)bank_.p;
      for_chunks(filters, chunk, [&](size_t f0, size_t nf) {
        prepare_taps(d_taps, scratch_.p, f0, nf, n_, correlate, real_, stream);
        plan_->exec(scratch_.p, bank + f0 * n_, nf, ::fourier::c::FOURIER_TRANSFORM_FFT, stream);
      });
      ConvArgs a{};
      a.out = bank;
      a.count = filters * n_;
      a.scale = code_scale<T>(::fourier::c::FOURIER_TRANSFORM_IFFT, (T)n_);
      FOURIER_LAUNCH(get_conv_sweep_kernel(Real<T>{}, CONV_FINISH), elementwise_grid(a.count), 256, 0, stream, a);
    }
    filters_ = filters;
  }

  void apply(const void* d_in, void* d_out, size_t batch, hipStream_t stream) const {
    check_buffers(d_in, d_out, batch * lx_ * val_, batch * lout_ * val_, val_, false);
    if (filters_ == 0) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "no filters set");
    if (batch == 0) return;
    DeviceGuard g(device_);
    const char* in = (const char*)d_in;
    char* out = (char*)d_out;
    if (route_ == OVERLAP_SAVE) {
      const size_t rows_per = std::max<size_t>(1, launch_items_ / geo_.wpr);
      for_chunks(batch, rows_per, [&](size_t b0, size_t nb) {
        plan_->exec_lconv(in + b0 * lx_ * val_, out + b0 * lout_ * val_, nb, bank_.p, filters_, b0, real_, geo_, stream);
      });
      return;
    }
    const size_t chunk = prepare(batch);
    const size_t words = real_ ? 1 : 2;
    for_chunks(batch, chunk, [&](size_t b0, size_t nb) {
      copy_rows(in + b0 * lx_ * val_, scratch_.p, nb, lx_ * words, m_ * words, 0, stream);
      inner_->apply(scratch_.p, scratch_.p, nb, stream, b0);
      copy_rows(scratch_.p, out + b0 * lout_ * val_, nb, m_ * words, lout_ * words, off_ * words, stream);
    });
  }

 private:
  static constexpr size_t LAUNCH_WORKGROUPS = (size_t)1 << 30;

  // block = 0: the rule; 11 ... 15: that block.  Builds what the new route needs first, then commits: a throw leaves the handle as it was.
  void select(int block, bool overlap_save) {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    int k = 0;
    if (block) {
      if (block > K_MAX) throw EngineError(INVALID, "no block of that size in this precision");
      if (((size_t)1 << block) < k_ - 1 + LINE) throw EngineError(INVALID, "block too short for the taps");
      k = block;
    } else {
      // f32, measured: up to 2^13 a block of 8 (K - 1) beats one of 4 (K - 1) (fewer contaminated outputs per block at the same cost
      // per point) where the row is longer than that block; longer blocks cost more per point, and f64 shows no such gain
      if (sizeof(T) == 4)
        for (int v = K_MIN; v <= 13 && !k; ++v)
          if (((size_t)1 << v) >= 8 * (k_ - 1) && lx_ + k_ - 1 > ((size_t)1 << v)) k = v;
      for (int v = K_MIN; v <= K_MAX && !k; ++v)
        if (((size_t)1 << v) >= 4 * (k_ - 1)) k = v;
      if (!k && ((size_t)1 << K_MAX) >= 2 * (k_ - 1)) k = K_MAX;
    }
    if (!overlap_save) k = 0;
    std::unique_ptr<Plan<T>> plan;
    if (k && !(plan_ && n_ == ((size_t)1 << k))) {
      plan.reset(new Plan<T>((size_t)1 << k, device_arg_));
      if (!plan->enable_lconv(real_)) {
        if (block) throw EngineError(INVALID, "no overlap-save kernel for that block");
        plan.reset();
        k = 0;
      }
    }
    if (!k && !inner_) {
      size_t m = 1;
      while (m < lx_ + k_ - 1) m <<= 1;
      inner_.reset(new ConvPlan<T>(m, real_, device_arg_));
      m_ = m;
    }
    const bool same = have_route_ && (k ? (route_ == OVERLAP_SAVE && n_ == ((size_t)1 << k)) : route_ == PADDED);
    block_opt_ = block;
    overlap_save_ = overlap_save;
    if (same) return;
    filters_ = 0;
    have_route_ = true;
    if (k) {
      if (plan) plan_ = std::move(plan);
      route_ = OVERLAP_SAVE;
      n_ = (size_t)1 << k;
      device_ = plan_->device();
      const size_t s = (n_ - (k_ - 1)) / LINE * LINE, nb = (lx_ + k_ - 1 + s - 1) / s;
      geo_.lx = (uint32_t)lx_; geo_.lout = (uint32_t)lout_; geo_.step = (uint32_t)s; geo_.off = (uint32_t)off_;
      geo_.nb = (uint32_t)nb; geo_.wpr = (uint32_t)(real_ ? (nb + 1) / 2 : nb);
      divider(geo_.wpr, geo_.div_m, geo_.div_l);
      desc_ = "lconv overlap-save: block " + std::to_string(n_) + " step " + std::to_string(s) + " blocks " + std::to_string(nb) +
              (real_ ? " real pairs, " : ", ") + plan_->describe();
    } else {
      route_ = PADDED;
      device_ = inner_->device();
      desc_ = "lconv padded: M=" + std::to_string(m_) + ", " + inner_->describe();
    }
  }

  // lconv_taps_kernel: filters f0 ... f0 + nf - 1 of the caller's taps -> rows of `n` values at dst
  void prepare_taps(const void* d_taps, void* dst, size_t f0, size_t nf, size_t n, bool reverse_conj, bool widen, hipStream_t stream) const {
    ConvArgs a{};
    a.in = (const char*)d_taps + f0 * k_ * val_;
    a.out = dst;
    a.n = n; a.taps = k_; a.rows = nf;
    a.conj = reverse_conj; a.widen = widen; a.real = real_;
    FOURIER_LAUNCH(get_conv_sweep_kernel(Real<T>{}, CONV_LTAPS), elementwise_grid(nf * n), 256, 0, stream, a);
  }
  // lconv_copy_kernel: word skip + k of every input row (w_in words) -> word k of the output row (w_out words), zero beyond the input row
  void copy_rows(const void* src, void* dst, size_t rows, size_t w_in, size_t w_out, size_t skip, hipStream_t stream) const {
    const size_t segs = (w_out + LCONV_SEG - 1) / LCONV_SEG;
    const size_t rows_per = std::max<size_t>(1, launch_items_ / segs);
    for_chunks(rows, rows_per, [&](size_t r0, size_t nr) {
      ConvArgs a{};
      a.in = (const T*)src + r0 * w_in;
      a.out = (T*)dst + r0 * w_out;
      a.n = w_out; a.taps = w_in; a.rows = nr; a.skip = skip;
      a.len = (uint32_t)segs;
      divider(a.len, a.div_m, a.div_l);
      FOURIER_LAUNCH(get_conv_sweep_kernel(Real<T>{}, CONV_LCOPY), nr * segs, 256, 0, stream, a);
    });
  }

  size_t lx_, k_;
  int mode_;
  bool real_;
  int device_arg_, device_ = 0;
  size_t off_ = 0, lout_ = 0, val_ = 0;  // val_: bytes of one value of the handle's kind
  int block_opt_ = 0;
  bool overlap_save_ = true, have_route_ = false;
  Route route_ = PADDED;
  size_t n_ = 0, m_ = 0;                 // block length (overlap-save), padded length (padded)
  LconvGeom geo_;
  std::unique_ptr<Plan<T>> plan_;        // the block plan: transforms the filters, runs the blocks
  std::unique_ptr<ConvPlan<T>> inner_;   // the circular handle of the padded route
  size_t filters_ = 0;
  DevBuf bank_, taps_;
  mutable DevBuf scratch_;
  size_t scratch_cap_ = REAL_SCRATCH_BYTES;
  size_t launch_items_ = LAUNCH_WORKGROUPS;  // workgroups of one launch (development switch FOURIER_LAUNCH_ITEMS)
};

}  // namespace fourier_hip
