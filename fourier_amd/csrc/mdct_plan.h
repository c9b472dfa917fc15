// mdct_plan.h -- the plan behind a modified discrete cosine transform handle (fourier_hip_mdct_*, include/fourier.h): batches of real
// rows <-> frames of n coefficients, frame-major (frame f of row b at element offset (b * frames + f) * n), a frame of 2n windowed
// samples every n samples, zero padding by index arithmetic at the load (`center`), built on an inner complex Plan<T> that runs
// unchanged.  The algebra is in kernels_mdct.h.  Routes:
//   "mdct composed"     even n = 2h: mdct_fold_kernel folds, windows and pre-twiddles the frames of a chunk of the flat frame index into
//                       one half of the scratch, the h-point plan takes them into the other half, mdct_post_kernel writes the caller's
//                       output.
//   "mdct fused rows"   n = 2h with a whole-row h-point kernel: mdct_rows_kernel in one launch, no scratch.  The default only where
//                       the constructor records a faster measurement (nowhere yet); option "fusion" = 0 forces the composed route, 1 takes
//                       the fused one wherever its kernel exists.
//   "mdct full-length"  odd n, the correctness path: the 2n-point plan in place on the windowed frame times exp(-i pi m / 2n).
//   inverse             "imdct composed" (even n) / "imdct full-length" (odd n): a pre sweep, the inner plan, and the overlap-add as a
//                       gather over the at most two frames that cover a sample.  Chunks are whole rows where a row's frames fit the
//                       scratch bound, else ranges of output samples of one row; the frame two neighbouring ranges both need is
//                       transformed twice.  A range needs both frames that cover a sample, so the scratch never holds fewer than two.
#pragma once
#include "frame_plan_common.h"
#include "real_plan.h"

namespace fourier_hip {

template <typename T> class MdctPlan : public HandleBase {
 public:
  static constexpr size_t ELEM = sizeof(cpx<T>);
  static constexpr size_t LAUNCH_ITEMS = (size_t)1 << 30;  // frames of one launch: 32-bit frame arithmetic in the kernels

  MdctPlan(size_t n, int center, int device) : n_(n), h_(n / 2), even_(n % 2 == 0), pad_(center ? n : 0) {
    if (n == 0) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "n >= 1");
    if (n > 0x1fffffffull) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "n above 2^29");
    inner_.reset(new Plan<T>(even_ ? h_ : 2 * n_, device));
    device_ = inner_->device();
    DeviceGuard g(device_);
    scratch_cap_ = scratch_bound("FOURIER_REAL_SCRATCH_BYTES", REAL_SCRATCH_BYTES);
    launch_items_ = launch_bound("FOURIER_LAUNCH_ITEMS", LAUNCH_ITEMS);
    // host f64, cast.  Even n: A[j] = exp(-i pi (4j + 1) / 4n) = W_8n^(4j+1), B[j] = exp(-i pi j / n) = W_2n^j, j < h;
    // odd n: D[m] = exp(-i pi m / 2n) = W_4n^m, m < 2n, C[k] = exp(-i pi (n + 1)(2k + 1) / 4n) = W_8n^((n+1)(2k+1)), k < n
    const uint64_t n64 = n_;
    std::vector<cpx<T>> ta(even_ ? h_ : 2 * n_), tb(even_ ? h_ : n_);
    for (uint64_t j = 0; j < ta.size(); ++j) ta[j] = even_ ? root<T>(4 * j + 1, 8 * n64) : root<T>(j, 4 * n64);
    for (uint64_t j = 0; j < tb.size(); ++j) tb[j] = even_ ? root<T>(j, 2 * n64) : root<T>((n64 + 1) * (2 * j + 1) % (8 * n64), 8 * n64);
    twa_.upload(ta);
    twb_.upload(tb);
    load_window(nullptr);
    // Where the fused route is the default.  The rule: only for a (precision, n) where it measured faster than the composed route by
    // more than the composed arm's spread (tools/mdct_bench.py).  No such measurement exists yet ("Modified discrete
    // cosine transform"), so the composed route is the default everywhere and option "fusion" = 1 takes the fused one.
    // FOURIER_MDCT_FUSION = 0 / 1 is the development switch of the experiments library and the emulator build.
    fusion_.init(even_ && inner_->template enable_frames<MdctArgs>(), "FOURIER_MDCT_FUSION", false);
    refresh_desc();
  }

  size_t size() const { return n_; }

  // frames of a row of `length` reals; 0 where the length is invalid
  size_t frames(size_t length) const {
    size_t f = 0;
    if (pad_) { if (length >= 1) f = (length + n_ - 1) / n_ + 1; }
    else if (length >= 2 * n_) f = length / n_ - 1;
    return f <= 0x7fffffffull ? f : 0;
  }

  int set_option(const std::string& key, long long v) {
    if (!fusion_.set(key, v)) return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    refresh_desc();
    return ::fourier::c::FOURIER_HIP_OK;
  }

  // 2n reals T on the device, or nullptr for the sine window.  A set-up call: it waits for `stream` (the table is replaced in place).
  void set_window(const void* d_window, hipStream_t stream) {
    if (d_window && (uintptr_t)d_window % sizeof(T)) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "misaligned window");
    DeviceGuard g(device_);
    std::vector<T> w(2 * n_);
    if (d_window) HIP_CHECK(hipMemcpyAsync(w.data(), d_window, w.size() * sizeof(T), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    load_window(d_window ? &w : nullptr);
  }

  // later forward calls of at most `batch` rows of `length` reals, and inverse calls to that length from frames(length) frames, never allocate
  void reserve(size_t length, size_t batch) const {
    const size_t fr = frames(length);
    if (fr == 0) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "invalid length");
    if (batch == 0) return;
    DeviceGuard g(device_);
    if (!fusion_.on) (void)prepare_forward(batch * fr);
    prepare(inverse_chunks(fr, batch).frames());
  }

  void forward(const void* d_in, void* d_out, size_t length, size_t batch, bool normalized, hipStream_t stream) const {
    const size_t fr = frames(length);
    if (fr == 0) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "invalid length");
    check_buffers(d_in, d_out, batch * length * sizeof(T), batch * fr * n_ * sizeof(T), sizeof(T), false);
    if (batch == 0) return;
    DeviceGuard g(device_);
    const size_t total = batch * fr;
    const T* in = (const T*)d_in;
    T* out = (T*)d_out;
    MdctArgs a = base_args(length, fr);
    divider(a.frames, a.fr_m, a.fr_l);
    a.scale = normalized ? std::sqrt(2.0 / (double)n_) : 1.0;
    if (fusion_.on) {
      a.pairs = (uintptr_t)out % ELEM == 0;
      for_chunks(total, launch_items_, [&](size_t g0, size_t ng) {
        frame_launch_at(a, in, length, fr, g0, ng);
        a.out = out + g0 * n_;
        inner_->exec_frames(a, stream);
      });
      return;
    }
    const size_t chunk = prepare_forward(total);
    cpx<T>* wa = (cpx<T>*)scratch_.p;
    const int code = ::fourier::c::FOURIER_TRANSFORM_FFT;
    for_chunks(total, chunk, [&](size_t g0, size_t ng) {
      frame_launch_at(a, in, length, fr, g0, ng);
      a.out = wa;
      if (even_) {
        cpx<T>* wb = wa + chunk * h_;
        sweep(MDCT_FOLD, a, ng, stream);
        inner_->exec(wa, wb, ng, code, stream);
        a.in = wb;
      } else {
        sweep(MDCT_ODD_PRE, a, ng, stream);
        inner_->exec(wa, wa, ng, code, stream);
        a.in = wa;
      }
      a.out = out + g0 * n_;
      sweep(even_ ? MDCT_POST : MDCT_ODD_POST, a, ng, stream);
    });
  }

  void inverse(const void* d_in, void* d_out, size_t fr, size_t length, size_t batch, bool normalized, hipStream_t stream) const {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    if (fr == 0 || fr > 0x7fffffffull) throw EngineError(INVALID, "invalid frame count");
    if (length == 0 || length > (pad_ ? fr - 1 : fr + 1) * n_) throw EngineError(INVALID, "invalid length");
    check_buffers(d_in, d_out, batch * fr * n_ * sizeof(T), batch * length * sizeof(T), sizeof(T), false);
    if (batch == 0) return;
    DeviceGuard g(device_);
    const T* in = (const T*)d_in;
    T* out = (T*)d_out;
    const FrameInverseChunks chunks = inverse_chunks(fr, batch);
    const size_t cap_frames = chunks.frames();
    prepare(cap_frames);
    cpx<T>* wa = (cpx<T>*)scratch_.p;
    cpx<T>* wb = even_ ? wa + cap_frames * h_ : wa;
    MdctArgs a = base_args(length, fr);
    const double scale = normalized ? std::sqrt(2.0 / (double)n_) : 2.0 / (double)n_;
    const int code = ::fourier::c::FOURIER_TRANSFORM_FFT;
    frame_inverse_walk(overlap(), chunks, fr, batch, length, [&](size_t b0, size_t nb, size_t t0, size_t span, size_t f_lo, size_t nfr) {
      const size_t count = nb == 1 ? nfr : nb * fr;
      a.in = in + (b0 * fr + f_lo) * n_;
      a.out = wa;
      a.total = count;
      sweep(even_ ? IMDCT_PRE : IMDCT_ODD_PRE, a, count, stream);
      inner_->exec(wa, wb, count, code, stream);
      a.in = wb;
      a.out = out + b0 * length;
      a.t0 = t0; a.span = span; a.rows = nb; a.f_lo = f_lo; a.nfr = nfr;
      a.total = nb * span;
      a.scale = scale;
      FOURIER_LAUNCH(get_mdct_kernel(Real<T>{}, even_ ? IMDCT_OLA : IMDCT_ODD_OLA), elementwise_grid(a.total), 256, 0, stream, a);
    });
  }

 private:
  void refresh_desc() {
    desc_ = std::string(!even_ ? "mdct full-length, imdct full-length: " : fusion_.on ? "mdct fused rows, imdct composed: " : "mdct composed, imdct composed: ") +
            inner_->describe();
  }
  MdctArgs base_args(size_t length, size_t fr) const {
    MdctArgs a{};
    a.win = win_.p; a.twa = twa_.p; a.twb = twb_.p;
    a.length = length; a.frames = (uint32_t)fr;
    a.n = (uint32_t)n_; a.pad = (uint32_t)pad_;
    a.scale = 1.0;
    return a;
  }
  // one frame per workgroup
  void sweep(int which, const MdctArgs& a, size_t count, hipStream_t stream) const {
    FOURIER_LAUNCH(get_mdct_kernel(Real<T>{}, which), count, 256, 0, stream, a);
  }
  // the window table: `w`, or the sine window sin(pi (m + 1/2) / 2n) in f64, cast
  void load_window(const std::vector<T>* w) {
    std::vector<T> sine;
    if (!w) {
      sine.resize(2 * n_);
      for (size_t m = 0; m < 2 * n_; ++m) sine[m] = (T)std::sin(M_PI * ((double)m + 0.5) / (2.0 * (double)n_));
      w = &sine;
    }
    win_.upload(*w);
  }
  // bytes of the scratch per frame: even n two halves of h complex values, odd n 2n complex values transformed in place
  size_t frame_bytes() const { return even_ ? 2 * h_ * ELEM : 2 * n_ * ELEM; }
  void prepare(size_t frames_in_scratch) const {
    scratch_.ensure(std::max<size_t>(frames_in_scratch * frame_bytes(), ELEM));
    inner_->reserve_for(frames_in_scratch, !even_);
  }
  // frames per chunk of the composed forward routes
  size_t prepare_forward(size_t total) const {
    const size_t chunk = std::min(chunk_rows(total, scratch_cap_, frame_bytes()), launch_items_);
    prepare(chunk);
    return chunk;
  }
  // the inverse's framing -- 2n samples a frame, two frames cover a sample -- and its chunks under the scratch bound (reserve() and
  // inverse() size from the same function)
  FrameOverlap overlap() const { return {2 * n_, n_, pad_}; }
  FrameInverseChunks inverse_chunks(size_t fr, size_t batch) const {
    return frame_inverse_chunks(overlap(), fr, batch, std::min(scratch_cap_ / frame_bytes(), launch_items_));
  }

  size_t n_, h_;
  bool even_;
  size_t pad_;
  int device_ = 0;
  std::unique_ptr<Plan<T>> inner_;
  FusionSwitch fusion_;
  DevBuf win_, twa_, twb_;
  mutable DevBuf scratch_;
  size_t scratch_cap_ = REAL_SCRATCH_BYTES;
  size_t launch_items_ = LAUNCH_ITEMS;  // frames of one launch (development switch FOURIER_LAUNCH_ITEMS)
};

}  // namespace fourier_hip
