// czt_plan.h -- the plan behind a chirp-z handle (fourier_hip_czt_*, include/fourier.h): of batched rows of n values x (complex, or
// reals) the m values
//   X[k] = sum_{j<n} x[j] a^-j w^(j k),  k < m,   w = w_abs exp(2 pi i w_turns),  a = a_abs exp(2 pi i a_turns)   (scipy.signal.czt),
// n samples in, m points out, on any arc or spiral of the z-plane.  Bluestein's identity j k = (j^2 + k^2 - (k - j)^2) / 2 gives
//   X[k] = B[k] sum_j (x[j] A[j]) v[k - j],
// a linear convolution carried by a circular one of L >= n + m - 1 points, L a power of two.  Host tables, evaluated in f64 and cast:
//   c(q)  = w_abs^(q/2) exp(2 pi i frac(w_turns q / 2)),  q = j^2
//   A[j]  = a_abs^-j exp(-2 pi i frac(a_turns j)) c(j^2),  j < n        B[k] = c(k^2),  k < m
//   v[i]  = 1 / c(i^2),  i = -(n-1) ... m-1, stored at i mod L          H = FFT_L(v) / L  (host_fft of plan.h)
// Every phase is reduced to one turn before the trigonometry, with the rounding error of the f64 product recovered by an fma (the
// exact-exponent chirp of Plan::build_chirp_tables reduces an integer; here the parameters are doubles), and every magnitude is
// exp(log(.) * .), with the logarithms of A's two factors added first.  Built on a complex Plan<T>(L) that runs unchanged.  Routes,
// chosen at create:
//   "czt one-launch"  L = max(2048, next_pow2(n + m - 1)) <= 2^15 (f64: 2^14): load n, (.) A, FFT, (.) H, inverse FFT, (.) B, store m in
//                     ONE launch on register-resident data (czt_small_kernel, Plan::exec_czt); no scratch
//   "czt composed"    any n, m with n + m - 1 <= 2^26, L = next_pow2(n + m - 1): czt_in_kernel -> rows of L in the scratch, the
//                     convolution with the one-table bank H in place there -- Plan::exec_conv where the plan has a route (one-launch or
//                     fused passes), else exec forward, conv_mul_kernel, exec unscaled inverse --, czt_out_kernel -> the caller's output
// Option "fusion" = 1 selects the one-launch route where the lengths have one, 0 the composed route.  The default is 1 where both
// routes run the same L, next_pow2(n + m - 1) >= 2048: there the one-launch route took 0.45 - 0.55 of the composed route's time at
// every measured L (profiles/czt/).  Below, the composed route convolves fewer than 2048 points, nothing is
// measured, and the default is 0.  The kernels are kernels_czt.h.  The batch is walked in chunks so that the plan-owned scratch
// stays bounded.
#pragma once
#include <cmath>

#include "plan.h"
#include "real_plan.h"

namespace fourier_hip {

// frac(t * q) for an integer or half-integer q below 2^52: the rounded product's fraction is exact, the product's rounding error is
// what the fma recovers.  The result may leave [0, 1) by that error.
static inline double czt_frac(double t, double q) {
  const double p = t * q, e = std::fma(t, q, -p);
  return (p - std::floor(p)) + e;
}
// c(q)^sign for q = i^2, times exp(extra_log + 2 pi i extra_turns)
static inline void czt_chirp(double lw, double w_turns, uint64_t i, double sign, double extra_log, double extra_turns, double& re, double& im) {
  const double half = 0.5 * ((double)i * (double)i);  // exact: i < 2^26
  const double mag = std::exp(sign * lw * half + extra_log);
  const double ang = 2.0 * M_PI * (sign * czt_frac(w_turns, half) + extra_turns);
  re = mag * std::cos(ang); im = mag * std::sin(ang);
}
// what a table entry must be after the cast to T: finite and (a chirp value) not zero
template <typename T> static bool czt_carried(const std::vector<cpx<T>>& t, bool zero_allowed = false) {
  for (const cpx<T>& z : t)
    if (!std::isfinite(z.re) || !std::isfinite(z.im) || (!zero_allowed && z.re == (T)0 && z.im == (T)0)) return false;
  return true;
}

// The scratch bound of a CztPlan is RealPlan's (REAL_SCRATCH_BYTES).  The experiments library and the emulator build read
// FOURIER_CZT_SCRATCH_BYTES at create instead (the chunk-walk test).
template <typename T> class CztPlan : public HandleBase {
 public:
  static constexpr size_t ELEM = sizeof(cpx<T>);
  static constexpr size_t MAX_ONE_LAUNCH = sizeof(T) == 4 ? (size_t)1 << 15 : (size_t)1 << 14;
  enum Route { ONE_LAUNCH, COMPOSED };

  CztPlan(size_t n, size_t m, double w_abs, double w_turns, double a_abs, double a_turns, bool real_input, int device)
      : n_(n), m_(m), real_(real_input), w_abs_(w_abs), w_turns_(w_turns) {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, UNSUPPORTED = ::fourier::c::FOURIER_HIP_UNSUPPORTED;
    if (n == 0 || m == 0) throw EngineError(INVALID, "n and m must be at least 1");
    if (!std::isfinite(w_abs) || !std::isfinite(w_turns) || !std::isfinite(a_abs) || !std::isfinite(a_turns))
      throw EngineError(INVALID, "a chirp-z parameter is not finite");
    if (!(w_abs > 0) || !(a_abs > 0)) throw EngineError(INVALID, "w_abs and a_abs must be positive");
    if (n > ((size_t)1 << 26) || m > ((size_t)1 << 26) || n + m - 1 > ((size_t)1 << 26))
      throw EngineError(UNSUPPORTED, "chirp-z transforms with n + m - 1 above 2^26 are not supported");
    const size_t lc = (size_t)1 << ilog2(n + m - 1), l1 = std::max<size_t>(2048, lc);
    // A and B, shared by both routes
    const double lw = std::log(w_abs), la = std::log(a_abs);
    std::vector<cpx<T>> A(n), B(m);
    for (size_t j = 0; j < n; ++j) {
      double re, im;
      czt_chirp(lw, w_turns, j, 1.0, -(double)j * la, -czt_frac(a_turns, (double)j), re, im);
      A[j] = {(T)re, (T)im};
    }
    for (size_t k = 0; k < m; ++k) {
      double re, im;
      czt_chirp(lw, w_turns, k, 1.0, 0.0, 0.0, re, im);
      B[k] = {(T)re, (T)im};
    }
    if (!czt_carried(A) || !czt_carried(B)) throw EngineError(UNSUPPORTED, "the spiral's chirp tables leave the range of the precision");
    comp_.reset(new Side(*this, lc, device));
    device_ = comp_->plan->device();
    DeviceGuard g(device_);
    atab_.upload(A);
    btab_.upload(B);
    conv_route_ = comp_->plan->enable_conv_bank();
    if (l1 <= MAX_ONE_LAUNCH) {
      if (l1 != lc) own_one_.reset(new Side(*this, l1, device_));
      Side* s = own_one_ ? own_one_.get() : comp_.get();
      if (s->plan->enable_czt(real_)) one_ = s;
    }
    scratch_cap_ = scratch_bound("FOURIER_CZT_SCRATCH_BYTES", REAL_SCRATCH_BYTES);
    launch_bytes_ = launch_bound("FOURIER_LAUNCH_BYTES", REAL_LAUNCH_BYTES);
    launch_items_ = launch_bound("FOURIER_LAUNCH_ITEMS", (size_t)1 << 30);
    set_fusion(one_ && !own_one_);  // the measured default: one launch where both routes run the same L
  }

  size_t size() const { return n_; }
  size_t points() const { return m_; }
  int device() const { return device_; }

  int set_option(const std::string& key, long long v) {
    if (key == "fusion" && (v == 0 || v == 1)) { set_fusion(v == 1); return ::fourier::c::FOURIER_HIP_OK; }
    return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
  }

  // rows per chunk for a call of `batch` rows; sizes the scratch and the plan's buffers for it
  size_t prepare(size_t batch) const {
    if (batch == 0) return 0;
    if (route_ == ONE_LAUNCH) return batch;  // no scratch, no plan buffers
    const size_t chunk = chunk_rows(batch, scratch_cap_, row_bytes());
    DeviceGuard g(device_);
    scratch_.ensure(chunk * row_bytes());
    if (conv_route_ == Plan<T>::CONV_NONE) comp_->plan->reserve_for(chunk, true);
    return chunk;
  }
  void reserve(size_t batch) const { (void)prepare(batch); }

  // `batch` rows of n values at d_in -> `batch` rows of m complex values at d_out, apart from the input
  void transform(const void* d_in, void* d_out, size_t batch, hipStream_t stream) const {
    const size_t vs = real_ ? sizeof(T) : ELEM;
    check_buffers(d_in, d_out, batch * n_ * vs, batch * m_ * ELEM, vs, false);
    if ((uintptr_t)d_out % ELEM) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "misaligned buffer");
    if (batch == 0) return;
    DeviceGuard g(device_);
    const size_t chunk = prepare(batch);
    const char* in = (const char*)d_in;
    cpx<T>* out = (cpx<T>*)d_out;
    if (route_ == ONE_LAUNCH) {  // one workgroup a row: launches of less than 2^31 workgroups
      for_chunks(batch, launch_items_, [&](size_t c0, size_t nb) {
        one_->plan->exec_czt(in + c0 * n_ * vs, out + c0 * m_, nb, n_, m_, atab_.p, btab_.p, one_->htab.p, real_, stream);
      });
      return;
    }
    const size_t L = comp_->L;
    const Plan<T>& plan = *comp_->plan;
    cpx<T>* work = (cpx<T>*)scratch_.p;  // rows of L of a chunk; behind them the two work arrays of the fused passes
    for_chunks(batch, chunk, [&](size_t c0, size_t nb) {
      sweep(CZT_IN, in + c0 * n_ * vs, work, nb, stream);
      if (conv_route_ != Plan<T>::CONV_NONE) {
        plan.exec_conv(work, work, nb, comp_->htab.p, 1, 0, work + chunk * L, work + 2 * chunk * L, stream);
      } else {
        plan.exec(work, work, nb, ::fourier::c::FOURIER_TRANSFORM_FFT, stream);
        multiply(work, nb, stream);
        plan.exec(work, work, nb, ::fourier::c::FOURIER_TRANSFORM_UNSCALED_IFFT, stream);
      }
      sweep(CZT_OUT, work, out + c0 * m_, nb, stream);
    });
  }

 private:
  // a plan of L points and the table H = FFT_L(v) / L on its device
  struct Side {
    size_t L;
    std::unique_ptr<Plan<T>> plan;
    DevBuf htab;
    Side(const CztPlan& c, size_t l, int device) : L(l) {
      std::vector<double> vr(L, 0.0), vi(L, 0.0);
      const double lw = std::log(c.w_abs_);
      for (size_t i = 0; i < c.m_; ++i) czt_chirp(lw, c.w_turns_, i, -1.0, 0.0, 0.0, vr[i], vi[i]);
      for (size_t i = 1; i < c.n_; ++i) czt_chirp(lw, c.w_turns_, i, -1.0, 0.0, 0.0, vr[L - i], vi[L - i]);
      // v itself must be carried by T where it is defined; a ZERO of its spectrum is no loss (w = 1 gives v = 1 on its support, and a
      // full-length support makes H a single impulse), so H is only required to be finite
      for (size_t i = 0; i < L; ++i) {
        const bool defined = i < c.m_ || i > L - c.n_;
        const cpx<T> z = {(T)vr[i], (T)vi[i]};
        if (defined && (!std::isfinite(z.re) || !std::isfinite(z.im) || (z.re == (T)0 && z.im == (T)0)))
          throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "the spiral's chirp tables leave the range of the precision");
      }
      host_fft(vr, vi);
      std::vector<cpx<T>> H(L);
      const double inv = 1.0 / (double)L;
      for (size_t k = 0; k < L; ++k) H[k] = {(T)(vr[k] * inv), (T)(vi[k] * inv)};
      if (!czt_carried(H, true)) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "the spiral's convolution table leaves the range of the precision");
      plan.reset(new Plan<T>(L, device));
      DeviceGuard g(plan->device());
      htab.upload(H);
    }
  };

  void set_fusion(bool on) {
    route_ = on && one_ ? ONE_LAUNCH : COMPOSED;
    if (route_ == ONE_LAUNCH) { desc_ = std::string("czt one-launch: ") + one_->plan->describe(); return; }
    const char* conv = conv_route_ == Plan<T>::CONV_ONE_LAUNCH ? "conv one-launch" : conv_route_ == Plan<T>::CONV_PASSES ? "conv fused passes" : "forward, product, inverse";
    desc_ = std::string("czt composed: ") + conv + ": " + comp_->plan->describe();
  }
  // scratch bytes per row of a chunk on the composed route: the work row, and the two work arrays of the fused passes
  size_t row_bytes() const { return (conv_route_ == Plan<T>::CONV_PASSES ? 3 : 1) * comp_->L * ELEM; }

  // czt_in_kernel (user rows of n -> work rows of L) or czt_out_kernel (work rows of L -> user rows of m) over nb rows, in launches of
  // at most REAL_LAUNCH_BYTES of the work array
  void sweep(int which, const void* in, void* out, size_t nb, hipStream_t stream) const {
    const size_t L = comp_->L, vs = real_ ? sizeof(T) : ELEM;
    const size_t rows_per = std::max<size_t>(1, launch_bytes_ / (L * ELEM));
    const bool first = which == CZT_IN;
    const size_t irow = first ? n_ * vs : L * ELEM, orow = first ? L * ELEM : m_ * ELEM;
    for (size_t r0 = 0; r0 < nb; r0 += rows_per) {
      const size_t rows = std::min(rows_per, nb - r0);
      CztArgs a{};
      a.in = (const char*)in + r0 * irow;
      a.out = (char*)out + r0 * orow;
      a.tab = first ? atab_.p : btab_.p;
      a.n = (uint32_t)n_; a.m = (uint32_t)m_;
      a.l_shift = (uint32_t)ilog2(L);
      a.total = (uint32_t)(rows * (first ? L : m_));
      divider(a.m, a.div_m, a.div_l);
      a.in_bytes = (uint32_t)(rows * irow);
      a.out_bytes = (uint32_t)(rows * orow);
      a.real = real_;
      FOURIER_LAUNCH(get_czt_kernel(Real<T>{}, which), (a.total + 255) / 256, 256, 0, stream, a);
    }
  }
  // work rows (.) H in place: conv_mul_kernel (kernels_conv.h) with a bank of one table
  void multiply(cpx<T>* z, size_t nb, hipStream_t stream) const {
    const size_t L = comp_->L;
    const size_t rows_per = std::max<size_t>(1, launch_bytes_ / (L * ELEM));
    for (size_t r0 = 0; r0 < nb; r0 += rows_per) {
      const size_t rows = std::min(rows_per, nb - r0);
      ConvArgs a{};
      a.in = a.out = z + r0 * L;
      a.bank = comp_->htab.p;
      a.len = (uint32_t)L;
      a.total = (uint32_t)(rows * L);
      divider(a.len, a.div_m, a.div_l);
      a.filters = 1;
      a.first = 0;
      divider(a.filters, a.f_m, a.f_l);
      a.bytes = (uint32_t)(rows * L * ELEM);
      FOURIER_LAUNCH(get_conv_sweep_kernel(Real<T>{}, CONV_MUL), (a.total + 255) / 256, 256, 0, stream, a);
    }
  }

  size_t n_, m_;
  bool real_;
  double w_abs_, w_turns_;
  int device_ = 0;
  std::unique_ptr<Side> comp_;     // the composed route: L = next_pow2(n + m - 1)
  std::unique_ptr<Side> own_one_;  // the one-launch route where its L = 2048 is above the composed route's
  Side* one_ = nullptr;            // the side the one-launch route runs on: comp_, own_one_, or none
  int conv_route_ = 0;             // Plan::CONV_NONE ...: how the composed route convolves
  DevBuf atab_, btab_;
  Route route_ = COMPOSED;
  mutable DevBuf scratch_;
  size_t scratch_cap_ = REAL_SCRATCH_BYTES;
  size_t launch_bytes_ = REAL_LAUNCH_BYTES;  // of either side of one sweep launch (development switch FOURIER_LAUNCH_BYTES)
  size_t launch_items_ = (size_t)1 << 30;  // rows of the one-launch route of one launch (development switch FOURIER_LAUNCH_ITEMS)
};

}  // namespace fourier_hip
