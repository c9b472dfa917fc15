// nufft_plan.h -- the plan behind a non-uniform FFT handle (fourier_hip_nufft_*, include/fourier.h): FINUFFT's 1-D type 1 and type 2
// with the points shared by the rows of a batch.  For n modes k = -floor(n/2) .. ceil(n/2) - 1 and m points x_j (any finite reals,
// taken modulo 2 pi), s = +1 or -1:
//   to_modes  (type 1)  f[b, k] = sum_j c[b, j] exp(i s k x_j)      batch rows of m -> batch rows of n
//   to_points (type 2)  c[b, j] = sum_k f[b, k] exp(i s k x_j)      batch rows of n -> batch rows of m
// no scale factor; to_points with s is the exact adjoint of to_modes with -s.  order 0 stores k ascending, order 1 in FFT order.
// The algorithm: the "exponential of semicircle" kernel phi(z) = exp(beta (sqrt(1 - z^2) - 1)), beta = 2.30 w, of width
// w = ceil(log10(1 / eps)) + 1 clamped to 2 .. 8 (f32) or 2 .. 16 (f64), on a fine grid of l cells, l the smallest 2^a 3^b 5^c >=
// max(2 n, 2 w); point x has the grid coordinate xg = (x mod 2 pi) l / (2 pi), first cell i0 = ceil(xg - w/2) and touches the cells
// i0 .. i0 + w - 1 modulo l with weight phi(2 (i - xg) / w).  phihat(k) = integral over |t| <= w/2 of phi(2 t / w) cos(2 pi k t / l).
//   to_modes:  nufft_spread_kernel (a gather, no atomics) -> Plan<T>(l) in place (FFT for s = -1, UNSCALED_IFFT for s = +1) ->
//              nufft_deconv_kernel picks the n modes and multiplies by 1 / phihat
//   to_points: nufft_amplify_kernel writes f / phihat into a zeroed grid row -> Plan<T>(l) in place -> nufft_interp_kernel
// Option "table": 0 = "nufft evaluated", the weights come from the accurate exp and sqrt in the two hot kernels; 1 = "nufft tabulated",
// a set-up kernel writes the m x w weights once and the hot kernels read them.  The default follows the rule at the constructor.
// The grid rows live in a plan-owned scratch bounded by REAL_SCRATCH_BYTES (never less than one row); the batch is walked with the
// shared chunk walk.  No atomics and a summation order fixed by the points: equal calls give bit-equal results, under any launch split
// and any scratch bound (up to the inner transforms' own dependence on a row's position in its launch).
#pragma once
#include <numeric>

#include "plan.h"
#include "real_plan.h"

namespace fourier_hip {

// 1 / phihat(|k|) for |k| <= n / 2 of the kernel of width w on a grid of l cells, cast to T (NufftPlan, and per axis Nufft2dPlan).
// With t = (w/2) sin(theta) the integrand is entire in theta,
//   phihat(k) = w * integral over [0, pi/2] of exp(beta (cos(theta) - 1)) cos(a sin(theta)) cos(theta),  a = pi k w / l,
// so Gauss-Legendre converges geometrically: q = 32 + floor(beta + pi w / 4) nodes (the integrand's widest oscillation over the
// interval is (beta + a) pi / 2 radians, a <= pi w / 4).  Nodes, weights and the integrand are formed in long double: in f64 the
// rounding of a node alone, times the integrand's logarithmic slope of up to beta + a = 50, costs 5e-15 of phihat at w = 16; in
// long double the rule agrees with itself on 200 nodes within 1e-15 at every width (tests/nufft_truth.py holds the same rule).
template <typename T> static std::vector<T> nufft_inverse_phihat(size_t n, int w, size_t l) {
  typedef long double R;
  const R pi = std::acos((R)-1), beta = (R)2.30 * (R)w;
  const int q = 32 + (int)(2.30 * (double)w + M_PI * (double)w / 4.0);
  std::vector<R> st(q), g(q);  // sin(theta_i), and the k-independent factor with the quadrature weight and the interval
  for (int i = 0; i < q; ++i) {  // Newton's iteration on P_q from the Chebyshev guess
    R x = std::cos(pi * ((R)i + (R)0.75) / ((R)q + (R)0.5)), dp = 1;
    for (int it = 0; it < 100; ++it) {
      R p0 = 1, p1 = x;
      for (int j = 2; j <= q; ++j) { const R p2 = ((2 * j - 1) * x * p1 - (j - 1) * p0) / j; p0 = p1; p1 = p2; }
      dp = q * (x * p1 - p0) / (x * x - 1);
      const R dx = p1 / dp;
      x -= dx;
      if (std::fabs(dx) < (R)1e-19) break;
    }
    R p0 = 1, p1 = x;
    for (int j = 2; j <= q; ++j) { const R p2 = ((2 * j - 1) * x * p1 - (j - 1) * p0) / j; p0 = p1; p1 = p2; }
    dp = q * (x * p1 - p0) / (x * x - 1);
    const R weight = 2 / ((1 - x * x) * dp * dp), theta = pi / 4 * (x + 1);
    st[i] = std::sin(theta);
    g[i] = pi / 4 * weight * std::exp(beta * (std::cos(theta) - 1)) * std::cos(theta) * (R)w;
  }
  std::vector<T> inv(n / 2 + 1);
  for (size_t k = 0; k < inv.size(); ++k) {
    const R a = pi * (R)k * (R)w / (R)l;
    R s = 0;
    for (int i = 0; i < q; ++i) s += g[i] * std::cos(a * st[i]);
    inv[k] = (T)(double)(1 / s);
  }
  return inv;
}

// The scratch bound of a NufftPlan is RealPlan's (REAL_SCRATCH_BYTES).  The experiments library and the emulator build read
// FOURIER_NUFFT_SCRATCH_BYTES at create instead (the chunk-walk test).
template <typename T> class NufftPlan : public HandleBase {
 public:
  static constexpr size_t ELEM = sizeof(cpx<T>);
  static constexpr size_t MAX_ROW_BYTES = (size_t)1 << 30;  // of a row of strengths or modes
  static constexpr size_t MAX_POINTS = 0x7fffffffu;
  static constexpr int MAX_W = sizeof(T) == 4 ? NUFFT_MAX_W_F32 : NUFFT_MAX_W_F64;

  NufftPlan(size_t n_modes, double eps, int device) : n_(n_modes) {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    if (n_modes == 0) throw EngineError(INVALID, "n_modes >= 1");
    if (!(eps > 0) || !std::isfinite(eps)) throw EngineError(INVALID, "eps must be finite and > 0");
    if (n_modes > MAX_ROW_BYTES / ELEM) throw EngineError(INVALID, "rows above 2^30 bytes");
    w_ = width_for(eps);
    l_ = grid_length(n_, (size_t)w_);
    if (l_ * ELEM > REAL_LAUNCH_BYTES) throw EngineError(INVALID, "fine grids above 2^31 bytes per row");
    plan_.reset(new Plan<T>(l_, device));
    device_ = plan_->device();
    DeviceGuard g(device_);
    scratch_cap_ = scratch_bound("FOURIER_NUFFT_SCRATCH_BYTES", REAL_SCRATCH_BYTES);
    launch_bytes_ = launch_bound("FOURIER_LAUNCH_BYTES", REAL_LAUNCH_BYTES);
    launch_items_ = launch_bound("FOURIER_LAUNCH_ITEMS", (size_t)1 << 30);
    inv_phihat_.upload(nufft_inverse_phihat<T>(n_, w_, l_));
    // Which route is the default: the project's rule is that the tabulated route becomes the default only if it beats the evaluated one
    // at every measured shape of both types beyond the larger max - min of the two arms.  It did so at none of the ten lines of the
    // committed run (0.98 - 1.11 of the evaluated route's time; tools/nufft_bench.py, profiles/nufft/nufft_bench.jsonl, DESIGN.md
    // section 4, "Non-uniform FFT"), so the evaluated route is.
    table_ = TABLE_BY_DEFAULT;
    refresh_desc();
  }

  size_t modes() const { return n_; }
  size_t points() const { return m_; }
  size_t grid() const { return l_; }
  int width() const { return w_; }
  int device() const { return device_; }

  // ceil(log10(1 / eps)) + 1, clamped to the widths with a kernel
  static int width_for(double eps) {
    const double w = std::ceil(std::log10(1.0 / eps)) + 1.0;
    return w < (double)NUFFT_MIN_W ? NUFFT_MIN_W : w > (double)MAX_W ? MAX_W : (int)w;
  }
  // the smallest 2^a 3^b 5^c >= max(2 n, 2 w): a length the inner plan runs natively
  static size_t grid_length(size_t n, size_t w) {
    const size_t need = std::max(2 * n, 2 * w);
    size_t best = 0;
    for (size_t p5 = 1; best == 0 || p5 < best; p5 *= 5) {
      for (size_t p3 = p5; best == 0 || p3 < best; p3 *= 3) {
        size_t v = p3;
        while (v < need) v *= 2;
        if (best == 0 || v < best) best = v;
      }
    }
    return best;
  }

  int set_option(const std::string& key, long long v) {
    if (key != "table" || (v != 0 && v != 1)) return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    const bool on = v == 1;
    if (on && !table_ && have_points_ && m_ > 0) {  // a set-up call: the table of the points in use, on the null stream
      DeviceGuard g(device_);
      DevBuf tab;
      build_table(tab, d_.p, m_, nullptr);
      swap_buf(wtab_, tab);
    }
    table_ = on;
    refresh_desc();
    return ::fourier::c::FOURIER_HIP_OK;
  }

  // m points as f64 on the HOST.  A set-up call: it waits for `stream` before the points in use are replaced and again after the
  // upload.  The new tables go into buffers of their own and replace the old ones only when all of them are complete: a call that
  // fails -- a point that is NaN or infinite, or an allocation or copy that fails -- leaves the points as they were.
  void set_points(const double* h_points, size_t m, hipStream_t stream) {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    if (m > MAX_POINTS) throw EngineError(INVALID, "more than 2^31 - 1 points");
    if (m > MAX_ROW_BYTES / ELEM) throw EngineError(INVALID, "rows above 2^30 bytes");
    if (m && !h_points) throw EngineError(INVALID, "null points");
    if ((uintptr_t)h_points % sizeof(double)) throw EngineError(INVALID, "misaligned points");
    for (size_t j = 0; j < m; ++j)
      if (!std::isfinite(h_points[j])) throw EngineError(INVALID, "a point is NaN or infinite");
    const double two_pi = 2.0 * M_PI, dl = (double)l_, half_w = 0.5 * (double)w_;
    std::vector<double> xg(m);
    for (size_t j = 0; j < m; ++j) {
      double x = h_points[j] - two_pi * std::floor(h_points[j] / two_pi);
      if (x < 0) x = 0;
      double g = x * (dl / two_pi);
      if (g >= dl) g -= dl;
      if (g < 0) g = 0;
      xg[j] = g;
    }
    std::vector<uint32_t> perm(m);
    std::iota(perm.begin(), perm.end(), 0u);
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return xg[a] < xg[b]; });
    std::vector<int32_t> i0(m);
    std::vector<T> d(m);
    const size_t ne = l_ + 2 * (size_t)w_ + 1;  // e in [-w, l + w]
    std::vector<uint32_t> first(ne);
    size_t e = 0;
    for (size_t p = 0; p < m; ++p) {
      const double g = xg[perm[p]];
      const double c = std::ceil(g - half_w);
      i0[p] = (int32_t)c;
      d[p] = (T)(c - g);  // formed in f64: the accuracy at f32 does not fall with l
      // first[e + w] = p for every e up to this point's i0 that no earlier point reached
      const size_t upto = (size_t)((int64_t)i0[p] + w_);
      for (; e <= upto; ++e) first[e] = (uint32_t)p;
    }
    for (; e < ne; ++e) first[e] = (uint32_t)m;
    DeviceGuard guard(device_);
    HIP_CHECK(hipStreamSynchronize(stream));
    DevBuf ni0, nd, nperm, nfirst, ntab;
    ni0.upload(i0);
    nd.upload(d);
    nperm.upload(perm);
    nfirst.upload(first);
    if (table_ && m > 0) build_table(ntab, nd.p, m, stream);
    HIP_CHECK(hipStreamSynchronize(stream));
    swap_buf(i0_, ni0);
    swap_buf(d_, nd);
    swap_buf(perm_, nperm);
    swap_buf(first_, nfirst);
    swap_buf(wtab_, ntab);  // (an empty one where the evaluated route is selected: set_option builds it when asked)
    m_ = m;
    have_points_ = true;
  }

  // rows per chunk for a call of `batch` rows; sizes the scratch and the inner plan's buffers for it
  size_t prepare(size_t batch) const {
    if (batch == 0) return 0;
    const size_t chunk = chunk_rows(batch, scratch_cap_, l_ * ELEM);
    DeviceGuard g(device_);
    scratch_.ensure(chunk * l_ * ELEM);
    plan_->reserve_for(chunk, true);
    return chunk;
  }
  void reserve(size_t batch) const { (void)prepare(batch); }

  // type 1: `batch` rows of m strengths at d_in -> `batch` rows of n modes at d_out
  void to_modes(const void* d_in, void* d_out, size_t batch, int sign, int order, hipStream_t stream) const {
    check_call(d_in, d_out, batch, m_, n_, sign, order);
    if (batch == 0) return;
    DeviceGuard g(device_);
    if (m_ == 0) {  // an empty sum
      HIP_CHECK(hipMemsetAsync(d_out, 0, batch * n_ * ELEM, stream));
      return;
    }
    const size_t chunk = prepare(batch);
    const cpx<T>* in = (const cpx<T>*)d_in;
    cpx<T>* out = (cpx<T>*)d_out;
    cpx<T>* grid = (cpx<T>*)scratch_.p;
    for_chunks(batch, chunk, [&](size_t b0, size_t nb) {
      hot_sweep(true, in + b0 * m_, grid, nb, stream);
      plan_->exec(grid, grid, nb, code_of(sign), stream);
      mode_sweep(NUFFT_DECONV, grid, out + b0 * n_, nb, order, stream);
    });
  }

  // type 2: `batch` rows of n modes at d_in -> `batch` rows of m values at d_out
  void to_points(const void* d_in, void* d_out, size_t batch, int sign, int order, hipStream_t stream) const {
    check_call(d_in, d_out, batch, n_, m_, sign, order);
    if (batch == 0 || m_ == 0) return;
    DeviceGuard g(device_);
    const size_t chunk = prepare(batch);
    const cpx<T>* in = (const cpx<T>*)d_in;
    cpx<T>* out = (cpx<T>*)d_out;
    cpx<T>* grid = (cpx<T>*)scratch_.p;
    for_chunks(batch, chunk, [&](size_t b0, size_t nb) {
      mode_sweep(NUFFT_AMPLIFY, in + b0 * n_, grid, nb, order, stream);
      plan_->exec(grid, grid, nb, code_of(sign), stream);
      hot_sweep(false, grid, out + b0 * m_, nb, stream);
    });
  }

 private:
  // The measured default (the constructor's comment).
  static constexpr bool TABLE_BY_DEFAULT = false;

  static int code_of(int sign) { return sign < 0 ? ::fourier::c::FOURIER_TRANSFORM_FFT : ::fourier::c::FOURIER_TRANSFORM_UNSCALED_IFFT; }

  void refresh_desc() {
    desc_ = std::string(table_ ? "nufft tabulated: " : "nufft evaluated: ") + "w " + std::to_string(w_) + ", L " + std::to_string(l_) + ", " +
            plan_->describe();
  }

  void check_call(const void* d_in, void* d_out, size_t batch, size_t ivals, size_t ovals, int sign, int order) const {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    if (sign != 1 && sign != -1) throw EngineError(INVALID, "sign is +1 or -1");
    if (order != 0 && order != 1) throw EngineError(INVALID, "order is 0 or 1");
    if (!have_points_) throw EngineError(INVALID, "no points: call set_points first");
    if (batch > ((size_t)1 << 62) / (std::max(ivals, ovals) * ELEM + 1)) throw EngineError(INVALID, "batch too large");
    check_buffers(d_in, d_out, batch * ivals * ELEM, batch * ovals * ELEM, ELEM, false);
  }

  NufftArgs base_args() const {
    NufftArgs a{};
    a.i0 = (const int32_t*)i0_.p; a.d = d_.p; a.perm = (const uint32_t*)perm_.p; a.first = (const uint32_t*)first_.p;
    a.wtab = table_ ? wtab_.p : nullptr;
    a.inv_phihat = inv_phihat_.p;
    a.l = (uint32_t)l_; a.m = (uint32_t)m_; a.n = (uint32_t)n_; a.w = (uint32_t)w_;
    a.beta = 2.30 * (double)w_;
    return a;
  }

  static void swap_buf(DevBuf& a, DevBuf& b) { std::swap(a.p, b.p); std::swap(a.bytes, b.bytes); }

  // the [w][m] weights of m sorted points with the offsets d (nufft_table_kernel) into `tab`, enqueued on `stream`; waits for it
  void build_table(DevBuf& tab, const void* d, size_t m, hipStream_t stream) const {
    tab.ensure((size_t)w_ * m * sizeof(T));
    NufftArgs a{};
    a.d = d; a.out = tab.p;
    a.m = a.total = (uint32_t)m; a.w = (uint32_t)w_;
    a.beta = 2.30 * (double)w_;
    FOURIER_LAUNCH(get_nufft_table_kernel(Real<T>{}), elementwise_grid(m), 256, 0, stream, a);
    HIP_CHECK(hipStreamSynchronize(stream));
  }

  // nufft_spread_kernel (strengths -> grid rows) or nufft_interp_kernel (grid rows -> values) over nb rows: whole blocks of NUFFT_RB
  // rows in launches of at most FOURIER_LAUNCH_ITEMS lanes (never less than one block), then the tail's own instance
  void hot_sweep(bool spread, const cpx<T>* in, cpx<T>* out, size_t nb, hipStream_t stream) const {
    const size_t lanes = spread ? l_ : m_, irow = spread ? m_ : l_, orow = spread ? l_ : m_;
    const size_t per = (lanes + 255) / 256;
    const size_t blocks_per = std::max<size_t>(1, launch_items_ / lanes);
    NufftArgs a = base_args();
    a.per = (uint32_t)per;
    divider(a.per, a.per_m, a.per_l);
    for (size_t r = 0; r < nb;) {
      const size_t left = nb - r;
      const int rb = left >= (size_t)NUFFT_RB ? NUFFT_RB : (int)left;
      const size_t blocks = rb == NUFFT_RB ? std::min(left / NUFFT_RB, blocks_per) : 1;
      a.in = in + r * irow;
      a.out = out + r * orow;
      a.blocks = (uint32_t)blocks;
      const NufftKernel k = spread ? get_nufft_spread_kernel(Real<T>{}, w_, rb) : get_nufft_interp_kernel(Real<T>{}, w_, rb);
      if (!k) throw EngineError(::fourier::c::FOURIER_HIP_RUNTIME_ERROR, "no nufft kernel for this width");
      FOURIER_LAUNCH(k, blocks * per, 256, 0, stream, a);
      r += blocks * (size_t)rb;
    }
  }

  // nufft_deconv_kernel (grid rows -> rows of n modes) or nufft_amplify_kernel (rows of n modes -> grid rows) over nb rows, in
  // launches of at most REAL_LAUNCH_BYTES per side and FOURIER_LAUNCH_ITEMS values (never less than one row)
  void mode_sweep(int which, const cpx<T>* in, cpx<T>* out, size_t nb, int order, hipStream_t stream) const {
    const size_t ivals = which == NUFFT_DECONV ? l_ : n_, ovals = which == NUFFT_DECONV ? n_ : l_;
    const size_t rows_per = std::max<size_t>(1, std::min(launch_bytes_ / (l_ * ELEM), launch_items_ / ovals));
    NufftArgs a = base_args();
    a.order = (uint32_t)order;
    divider((uint32_t)ovals, a.div_m, a.div_l);
    for (size_t r0 = 0; r0 < nb; r0 += rows_per) {
      const size_t rows = std::min(rows_per, nb - r0);
      a.in = in + r0 * ivals;
      a.out = out + r0 * ovals;
      a.total = (uint32_t)(rows * ovals);
      a.in_bytes = (uint32_t)(rows * ivals * ELEM);
      a.out_bytes = (uint32_t)(rows * ovals * ELEM);
      FOURIER_LAUNCH(get_nufft_sweep_kernel(Real<T>{}, which), (a.total + 255) / 256, 256, 0, stream, a);
    }
  }

  size_t n_, l_ = 0, m_ = 0;
  int w_ = 0;
  int device_ = 0;
  std::unique_ptr<Plan<T>> plan_;  // the l-point transform of the fine grid, in place on the scratch
  bool table_ = false;
  bool have_points_ = false;
  DevBuf inv_phihat_, i0_, d_, perm_, first_, wtab_;
  mutable DevBuf scratch_;
  size_t scratch_cap_ = REAL_SCRATCH_BYTES;
  size_t launch_bytes_ = REAL_LAUNCH_BYTES;  // of either side of one sweep launch (development switch FOURIER_LAUNCH_BYTES)
  size_t launch_items_ = (size_t)1 << 30;    // lanes of one launch (development switch FOURIER_LAUNCH_ITEMS)
};

}  // namespace fourier_hip
