// nufft3d_plan.h -- the plan behind a 3-D non-uniform FFT handle (fourier_hip_nufft3d_*, include/fourier.h): FINUFFT's 3-D type 1 and
// type 2 in C order with the points shared by the items of a batch.  For n1 x n2 x n3 modes, k_d = -floor(n_d/2) .. ceil(n_d/2) - 1,
// and m points (x1_j, x2_j, x3_j) (any finite reals, taken modulo 2 pi per coordinate; coordinate d pairs with axis d, axis 3 is
// contiguous), s = +1 or -1:
//   to_modes  (type 1)  f[b, k1, k2, k3] = sum_j c[b, j] exp(i s (k1 x1_j + k2 x2_j + k3 x3_j))          rows of m -> items of n1 x n2 x n3
//   to_points (type 2)  c[b, j] = sum_{k1,k2,k3} f[b, k1, k2, k3] exp(i s (k1 x1_j + k2 x2_j + k3 x3_j))  the reverse
// no scale factor; to_points with s is the exact adjoint of to_modes with -s.  order 0 stores all three axes ascending, order 1 all
// three in FFT order.  The algorithm is Nufft2dPlan's (nufft2d_plan.h) with one more axis: the same kernel phi, one width w for all
// three axes, l_d the smallest 2^a 3^b 5^c >= max(2 n_d, 2 w), the weight of a point on cell (i1, i2, i3) the product of its three
// 1-D weights, the deconvolution factor kept as three 1-D tables from NufftPlan's quadrature (nufft_inverse_phihat).
//   to_modes:  nufft3d_spread_kernel (a gather, no atomics) onto items of l1 x l2 x l3 -> the l3-point row plan on nb l1 l2 rows in
//              place -> the l2-point plan's axis route with outer = nb l1, inner = l3 in place -> the l1-point plan's axis route with
//              outer = nb, inner = l2 l3 in place (FFT for s = -1, UNSCALED_IFFT for s = +1) -> nufft3d_deconv_kernel picks the
//              n1 x n2 x n3 modes and multiplies by 1 / phihat
//   to_points: nufft3d_amplify_kernel writes f / phihat into a zeroed grid item -> the three transforms -> nufft3d_interp_kernel
// Option "table": 0 = "nufft3d evaluated", the weights come from the accurate exp and sqrt in the two hot kernels; 1 = "nufft3d
// tabulated", a set-up kernel writes the 3 x w x m weights once and the hot kernels read them.  The default follows the rule at the
// constructor.
// Besides seven arrays of m values, set_points keeps first[]: l1 l2 (l3 + 2w + 1) uint32, about half of one f32 grid item and a
// quarter of an f64 one (kernels_nufft3d.h).
// The grid items live in a plan-owned scratch bounded by REAL_SCRATCH_BYTES (never less than one item); the batch is walked with the
// shared chunk walk.  No atomics and a summation order fixed by the points: equal calls give bit-equal results, under any launch split
// and any scratch bound (up to the inner transforms' own dependence on a row's position in its launch).
#pragma once
#include <numeric>

#include "axis_plan.h"
#include "nufft_plan.h"

namespace fourier_hip {

// The scratch bound of a Nufft3dPlan is RealPlan's (REAL_SCRATCH_BYTES).  The experiments library and the emulator build read
// FOURIER_NUFFT3D_SCRATCH_BYTES at create instead (the chunk-walk test).
template <typename T> class Nufft3dPlan : public HandleBase {
 public:
  static constexpr size_t ELEM = sizeof(cpx<T>);
  static constexpr size_t MAX_ITEM_BYTES = (size_t)1 << 30;  // of a row of strengths or an item of modes
  static constexpr size_t MAX_POINTS = 0x7fffffffu;

  Nufft3dPlan(size_t n1, size_t n2, size_t n3, double eps, int device) : n1_(n1), n2_(n2), n3_(n3) {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    if (n1 == 0 || n2 == 0 || n3 == 0) throw EngineError(INVALID, "n1, n2, n3 >= 1");
    if (!(eps > 0) || !std::isfinite(eps)) throw EngineError(INVALID, "eps must be finite and > 0");
    const size_t cap = MAX_ITEM_BYTES / ELEM;  // each factor <= cap < 2^27: no product of two overflows
    if (n1 > cap || n2 > cap || n3 > cap || n1 * n2 > cap || n1 * n2 * n3 > cap) throw EngineError(INVALID, "items above 2^30 bytes");
    w_ = NufftPlan<T>::width_for(eps);
    l1_ = NufftPlan<T>::grid_length(n1_, (size_t)w_);
    l2_ = NufftPlan<T>::grid_length(n2_, (size_t)w_);
    l3_ = NufftPlan<T>::grid_length(n3_, (size_t)w_);
    const size_t lcap = REAL_LAUNCH_BYTES / ELEM;
    if (l1_ > lcap || l2_ > lcap || l3_ > lcap || l1_ * l2_ > lcap || l1_ * l2_ * l3_ > lcap)
      throw EngineError(INVALID, "fine grids above 2^31 bytes per item");
    cells_ = l1_ * l2_ * l3_;
    rows_.reset(new Plan<T>(l3_, device));
    device_ = rows_->device();
    axis2_.reset(new Plan<T>(l2_, device_));  // one plan per axis even where two lengths are equal: a route caches its reservation per plan
    axis1_.reset(new Plan<T>(l1_, device_));
    DeviceGuard g(device_);
    scratch_cap_ = scratch_bound("FOURIER_NUFFT3D_SCRATCH_BYTES", REAL_SCRATCH_BYTES);
    launch_bytes_ = launch_bound("FOURIER_LAUNCH_BYTES", REAL_LAUNCH_BYTES);
    launch_items_ = launch_bound("FOURIER_LAUNCH_ITEMS", (size_t)1 << 30);
    inv1_.upload(nufft_inverse_phihat<T>(n1_, w_, l1_));
    inv2_.upload(nufft_inverse_phihat<T>(n2_, w_, l2_));
    inv3_.upload(nufft_inverse_phihat<T>(n3_, w_, l3_));
    // Which route is the default: the project's rule is that the tabulated route becomes the default only if it beats the evaluated one
    // at every measured shape of both types beyond the larger max - min of the two arms.  In the committed run it did so at all six
    // type-1 lines (0.56 - 0.85 of the evaluated route's time) and at one of the six type-2 lines (0.92 at 32^3 modes, f32; 0.98 -
    // 1.03 at the other five, inside the spreads; tools/nufft3d_bench.py, profiles/nufft3d/nufft3d_bench.jsonl, DESIGN.md section 4,
    // "Non-uniform FFT, 3-D"), so the evaluated route is.  Where type 1 dominates a caller's time, "table" = 1 is worth setting.
    table_ = false;
    refresh_desc();
  }

  size_t modes1() const { return n1_; }
  size_t modes2() const { return n2_; }
  size_t modes3() const { return n3_; }
  size_t points() const { return m_; }
  int device() const { return device_; }

  int set_option(const std::string& key, long long v) {
    if (key != "table" || (v != 0 && v != 1)) return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    const bool on = v == 1;
    if (on && !table_ && have_points_ && m_ > 0) {  // a set-up call: the table of the points in use, on the null stream
      DeviceGuard g(device_);
      DevBuf tab;
      build_table(tab, d1_.p, d2_.p, d3_.p, m_, nullptr);
      swap_buf(wtab_, tab);
    }
    table_ = on;
    refresh_desc();
    return ::fourier::c::FOURIER_HIP_OK;
  }

  // m points as three arrays of f64 on the HOST.  A set-up call with Nufft2dPlan::set_points' semantics: it waits for `stream` before
  // the points in use are replaced and again after the upload; the new tables go into buffers of their own and replace the old ones
  // only when all of them are complete, so a call that fails leaves the points as they were.
  void set_points(const double* h_x1, const double* h_x2, const double* h_x3, size_t m, hipStream_t stream) {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    if (m > MAX_POINTS) throw EngineError(INVALID, "more than 2^31 - 1 points");
    if (m > MAX_ITEM_BYTES / ELEM) throw EngineError(INVALID, "rows above 2^30 bytes");
    if (m && (!h_x1 || !h_x2 || !h_x3)) throw EngineError(INVALID, "null points");
    if ((uintptr_t)h_x1 % sizeof(double) || (uintptr_t)h_x2 % sizeof(double) || (uintptr_t)h_x3 % sizeof(double))
      throw EngineError(INVALID, "misaligned points");
    for (size_t j = 0; j < m; ++j)
      if (!std::isfinite(h_x1[j]) || !std::isfinite(h_x2[j]) || !std::isfinite(h_x3[j])) throw EngineError(INVALID, "a point is NaN or infinite");
    const double half_w = 0.5 * (double)w_;
    // per point and axis: the folded grid coordinate g, the first cell ceil(g - w/2) and the offset, formed in f64 as in 1-D
    std::vector<double> g3(m);
    std::vector<uint32_t> bucket(m);  // r1 l2 + r2 < l1 l2 <= 2^28
    std::vector<int32_t> c3(m);
    std::vector<T> o1(m), o2(m), o3(m);
    for (size_t j = 0; j < m; ++j) {
      const double g1 = fold(h_x1[j], l1_), c1 = std::ceil(g1 - half_w);
      const double g2 = fold(h_x2[j], l2_), c2 = std::ceil(g2 - half_w);
      const uint32_t r1 = (uint32_t)(c1 < 0 ? c1 + (double)l1_ : c1), r2 = (uint32_t)(c2 < 0 ? c2 + (double)l2_ : c2);
      bucket[j] = r1 * (uint32_t)l2_ + r2;
      o1[j] = (T)(c1 - g1);
      o2[j] = (T)(c2 - g2);
      g3[j] = fold(h_x3[j], l3_);
      const double c = std::ceil(g3[j] - half_w);
      c3[j] = (int32_t)c;
      o3[j] = (T)(c - g3[j]);
    }
    // buckets by (r1, r2), each sorted by g3; stable, so that points equal in all three keep the caller's order
    std::vector<uint32_t> perm(m);
    std::iota(perm.begin(), perm.end(), 0u);
    std::stable_sort(perm.begin(), perm.end(),
                     [&](uint32_t a, uint32_t b) { return bucket[a] != bucket[b] ? bucket[a] < bucket[b] : g3[a] < g3[b]; });
    std::vector<uint32_t> sb(m), sr1(m), sr2(m);
    std::vector<int32_t> si03(m);
    std::vector<T> sd1(m), sd2(m), sd3(m);
    for (size_t p = 0; p < m; ++p) {
      const uint32_t j = perm[p];
      sb[p] = bucket[j]; sr1[p] = bucket[j] / (uint32_t)l2_; sr2[p] = bucket[j] % (uint32_t)l2_;
      si03[p] = c3[j]; sd1[p] = o1[j]; sd2[p] = o2[j]; sd3[p] = o3[j];
    }
    const size_t ne3 = l3_ + 2 * (size_t)w_ + 1;  // e in [-w, l3 + w]
    const size_t nbuckets = l1_ * l2_;
    std::vector<uint32_t> first(nbuckets * ne3);
    size_t p = 0;
    for (size_t r = 0; r < nbuckets; ++r) {
      uint32_t* row = first.data() + r * ne3;
      size_t e = 0;
      for (; p < m && sb[p] == r; ++p) {
        // row[e + w] = p for every e up to this point's i0_3 that no earlier point of the bucket reached
        const size_t upto = (size_t)((int64_t)si03[p] + w_);
        for (; e <= upto; ++e) row[e] = (uint32_t)p;
      }
      for (; e < ne3; ++e) row[e] = (uint32_t)p;  // the bucket's end (its start where it is empty)
    }
    DeviceGuard guard(device_);
    HIP_CHECK(hipStreamSynchronize(stream));
    DevBuf nr1, nr2, ni03, nd1, nd2, nd3, nperm, nfirst, ntab;
    nr1.upload(sr1);
    nr2.upload(sr2);
    ni03.upload(si03);
    nd1.upload(sd1);
    nd2.upload(sd2);
    nd3.upload(sd3);
    nperm.upload(perm);
    nfirst.upload(first);
    if (table_ && m > 0) build_table(ntab, nd1.p, nd2.p, nd3.p, m, stream);
    HIP_CHECK(hipStreamSynchronize(stream));
    swap_buf(r1_, nr1);
    swap_buf(r2_, nr2);
    swap_buf(i03_, ni03);
    swap_buf(d1_, nd1);
    swap_buf(d2_, nd2);
    swap_buf(d3_, nd3);
    swap_buf(perm_, nperm);
    swap_buf(first_, nfirst);
    swap_buf(wtab_, ntab);  // (an empty one where the evaluated route is selected: set_option builds it when asked)
    m_ = m;
    have_points_ = true;
  }

  // items per chunk for a call of `batch` items; sizes the scratch, the row plan's buffers and the two axis routes for it
  size_t prepare(size_t batch) const {
    if (batch == 0) return 0;
    const size_t chunk = chunk_rows(batch, scratch_cap_, cells_ * ELEM);
    DeviceGuard g(device_);
    scratch_.ensure(chunk * cells_ * ELEM);
    rows_->reserve_for(chunk * l1_ * l2_, true);
    AxisRoute<T>::of(*axis2_).reserve(chunk * l1_, l3_);
    AxisRoute<T>::of(*axis1_).reserve(chunk, l2_ * l3_);
    return chunk;
  }
  void reserve(size_t batch) const { (void)prepare(batch); }

  // type 1: `batch` rows of m strengths at d_in -> `batch` items of n1 x n2 x n3 modes at d_out
  void to_modes(const void* d_in, void* d_out, size_t batch, int sign, int order, hipStream_t stream) const {
    const size_t modes = n1_ * n2_ * n3_;
    check_call(d_in, d_out, batch, m_, modes, sign, order);
    if (batch == 0) return;
    DeviceGuard g(device_);
    if (m_ == 0) {  // an empty sum
      HIP_CHECK(hipMemsetAsync(d_out, 0, batch * modes * ELEM, stream));
      return;
    }
    const size_t chunk = prepare(batch);
    const cpx<T>* in = (const cpx<T>*)d_in;
    cpx<T>* out = (cpx<T>*)d_out;
    cpx<T>* grid = (cpx<T>*)scratch_.p;
    for_chunks(batch, chunk, [&](size_t b0, size_t nb) {
      hot_sweep(true, in + b0 * m_, grid, nb, stream);
      transform(grid, nb, sign, stream);
      mode_sweep(NUFFT_DECONV, grid, out + b0 * modes, nb, order, stream);
    });
  }

  // type 2: `batch` items of n1 x n2 x n3 modes at d_in -> `batch` rows of m values at d_out
  void to_points(const void* d_in, void* d_out, size_t batch, int sign, int order, hipStream_t stream) const {
    const size_t modes = n1_ * n2_ * n3_;
    check_call(d_in, d_out, batch, modes, m_, sign, order);
    if (batch == 0 || m_ == 0) return;
    DeviceGuard g(device_);
    const size_t chunk = prepare(batch);
    const cpx<T>* in = (const cpx<T>*)d_in;
    cpx<T>* out = (cpx<T>*)d_out;
    cpx<T>* grid = (cpx<T>*)scratch_.p;
    for_chunks(batch, chunk, [&](size_t b0, size_t nb) {
      mode_sweep(NUFFT_AMPLIFY, in + b0 * modes, grid, nb, order, stream);
      transform(grid, nb, sign, stream);
      hot_sweep(false, grid, out + b0 * m_, nb, stream);
    });
  }

 private:
  // x modulo 2 pi as a grid coordinate in [0, l): NufftPlan::set_points' fold
  static double fold(double v, size_t l) {
    const double two_pi = 2.0 * M_PI, dl = (double)l;
    double x = v - two_pi * std::floor(v / two_pi);
    if (x < 0) x = 0;
    double g = x * (dl / two_pi);
    if (g >= dl) g -= dl;
    if (g < 0) g = 0;
    return g;
  }

  // the transform of nb grid items in place: the rows of l3, then axis 2, then axis 1
  void transform(cpx<T>* grid, size_t nb, int sign, hipStream_t stream) const {
    const int code = sign < 0 ? ::fourier::c::FOURIER_TRANSFORM_FFT : ::fourier::c::FOURIER_TRANSFORM_UNSCALED_IFFT;
    rows_->exec(grid, grid, nb * l1_ * l2_, code, stream);
    AxisRoute<T>::of(*axis2_).transform(grid, grid, nb * l1_, l3_, code, stream);
    AxisRoute<T>::of(*axis1_).transform(grid, grid, nb, l2_ * l3_, code, stream);
  }

  void refresh_desc() {
    desc_ = std::string(table_ ? "nufft3d tabulated: " : "nufft3d evaluated: ") + "w " + std::to_string(w_) + ", L " + std::to_string(l1_) + " x " +
            std::to_string(l2_) + " x " + std::to_string(l3_) + ", rows " + rows_->describe() + ", axis 2 " +
            AxisRoute<T>::of(*axis2_).describe(l3_) + ", axis 1 " + AxisRoute<T>::of(*axis1_).describe(l2_ * l3_);
  }

  void check_call(const void* d_in, void* d_out, size_t batch, size_t ivals, size_t ovals, int sign, int order) const {
    const int INVALID = ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
    if (sign != 1 && sign != -1) throw EngineError(INVALID, "sign is +1 or -1");
    if (order != 0 && order != 1) throw EngineError(INVALID, "order is 0 or 1");
    if (!have_points_) throw EngineError(INVALID, "no points: call set_points first");
    if (batch > ((size_t)1 << 62) / (std::max(ivals, ovals) * ELEM + 1)) throw EngineError(INVALID, "batch too large");
    check_buffers(d_in, d_out, batch * ivals * ELEM, batch * ovals * ELEM, ELEM, false);
  }

  Nufft3dArgs base_args() const {
    Nufft3dArgs a{};
    a.r1 = (const uint32_t*)r1_.p; a.r2 = (const uint32_t*)r2_.p; a.i03 = (const int32_t*)i03_.p;
    a.d1 = d1_.p; a.d2 = d2_.p; a.d3 = d3_.p;
    a.perm = (const uint32_t*)perm_.p; a.first = (const uint32_t*)first_.p;
    a.wtab = table_ ? wtab_.p : nullptr;
    a.inv1 = inv1_.p; a.inv2 = inv2_.p; a.inv3 = inv3_.p;
    a.l1 = (uint32_t)l1_; a.l2 = (uint32_t)l2_; a.l3 = (uint32_t)l3_; a.m = (uint32_t)m_;
    a.n1 = (uint32_t)n1_; a.n2 = (uint32_t)n2_; a.n3 = (uint32_t)n3_; a.w = (uint32_t)w_;
    a.ne3 = (uint32_t)(l3_ + 2 * (size_t)w_ + 1);
    a.cells = (uint32_t)cells_;
    a.beta = 2.30 * (double)w_;
    return a;
  }

  static void swap_buf(DevBuf& a, DevBuf& b) { std::swap(a.p, b.p); std::swap(a.bytes, b.bytes); }

  // the [3][w][m] weights of m sorted points with the offsets d1, d2, d3 (nufft3d_table_kernel) into `tab`, enqueued on `stream`; waits
  void build_table(DevBuf& tab, const void* d1, const void* d2, const void* d3, size_t m, hipStream_t stream) const {
    tab.ensure(3 * (size_t)w_ * m * sizeof(T));
    Nufft3dArgs a{};
    a.d1 = d1; a.d2 = d2; a.d3 = d3; a.out = tab.p;
    a.m = a.total = (uint32_t)m; a.w = (uint32_t)w_;
    a.beta = 2.30 * (double)w_;
    FOURIER_LAUNCH(get_nufft3d_table_kernel(Real<T>{}), elementwise_grid(m), 256, 0, stream, a);
    HIP_CHECK(hipStreamSynchronize(stream));
  }

  // nufft3d_spread_kernel (strengths -> grid items) or nufft3d_interp_kernel (grid items -> values) over nb items: whole blocks of
  // NUFFT_RB items in launches of at most FOURIER_LAUNCH_ITEMS lanes (never less than one block), then the tail's own instance
  void hot_sweep(bool spread, const cpx<T>* in, cpx<T>* out, size_t nb, hipStream_t stream) const {
    const size_t lanes = spread ? cells_ : m_, ivals = spread ? m_ : cells_, ovals = spread ? cells_ : m_;
    const size_t per = (lanes + 255) / 256;
    const size_t blocks_per = std::max<size_t>(1, launch_items_ / lanes);
    Nufft3dArgs a = base_args();
    a.per = (uint32_t)per;
    divider(a.per, a.per_m, a.per_l);
    divider(a.l3, a.l3_m, a.l3_l);
    divider(a.l2, a.l2_m, a.l2_l);
    for (size_t r = 0; r < nb;) {
      const size_t left = nb - r;
      const int rb = left >= (size_t)NUFFT_RB ? NUFFT_RB : (int)left;
      const size_t blocks = rb == NUFFT_RB ? std::min(left / NUFFT_RB, blocks_per) : 1;
      a.in = in + r * ivals;
      a.out = out + r * ovals;
      a.blocks = (uint32_t)blocks;
      const Nufft3dKernel k = spread ? get_nufft3d_spread_kernel(Real<T>{}, rb) : get_nufft3d_interp_kernel(Real<T>{}, w_, rb);
      if (!k) throw EngineError(::fourier::c::FOURIER_HIP_RUNTIME_ERROR, "no nufft3d kernel for this width");
      FOURIER_LAUNCH(k, blocks * per, 256, 0, stream, a);
      r += blocks * (size_t)rb;
    }
  }

  // nufft3d_deconv_kernel (grid items -> items of n1 x n2 x n3 modes) or nufft3d_amplify_kernel (the reverse) over nb items, in
  // launches of at most REAL_LAUNCH_BYTES per side and FOURIER_LAUNCH_ITEMS values (never less than one item)
  void mode_sweep(int which, const cpx<T>* in, cpx<T>* out, size_t nb, int order, hipStream_t stream) const {
    const size_t modes = n1_ * n2_ * n3_;
    const size_t ivals = which == NUFFT_DECONV ? cells_ : modes, ovals = which == NUFFT_DECONV ? modes : cells_;
    const size_t items_per = std::max<size_t>(1, std::min(launch_bytes_ / (cells_ * ELEM), launch_items_ / ovals));
    Nufft3dArgs a = base_args();
    a.order = (uint32_t)order;
    divider((uint32_t)ovals, a.item_m, a.item_l);
    divider(which == NUFFT_DECONV ? a.n3 : a.l3, a.row_m, a.row_l);
    divider(which == NUFFT_DECONV ? a.n2 : a.l2, a.mid_m, a.mid_l);
    for (size_t r0 = 0; r0 < nb; r0 += items_per) {
      const size_t items = std::min(items_per, nb - r0);
      a.in = in + r0 * ivals;
      a.out = out + r0 * ovals;
      a.total = (uint32_t)(items * ovals);
      a.in_bytes = (uint32_t)(items * ivals * ELEM);
      a.out_bytes = (uint32_t)(items * ovals * ELEM);
      FOURIER_LAUNCH(get_nufft3d_sweep_kernel(Real<T>{}, which), (a.total + 255) / 256, 256, 0, stream, a);
    }
  }

  size_t n1_, n2_, n3_, l1_ = 0, l2_ = 0, l3_ = 0, cells_ = 0, m_ = 0;
  int w_ = 0;
  int device_ = 0;
  std::unique_ptr<Plan<T>> rows_;   // the l3-point transform of the grid's rows, in place on the scratch
  std::unique_ptr<Plan<T>> axis2_;  // the l2-point plan whose axis route (axis_plan.h) transforms axis 2 in place
  std::unique_ptr<Plan<T>> axis1_;  // the l1-point plan whose axis route transforms axis 1 in place
  bool table_ = false;
  bool have_points_ = false;
  DevBuf inv1_, inv2_, inv3_, r1_, r2_, i03_, d1_, d2_, d3_, perm_, first_, wtab_;
  mutable DevBuf scratch_;
  size_t scratch_cap_ = REAL_SCRATCH_BYTES;
  size_t launch_bytes_ = REAL_LAUNCH_BYTES;  // of either side of one sweep launch (development switch FOURIER_LAUNCH_BYTES)
  size_t launch_items_ = (size_t)1 << 30;    // lanes of one launch (development switch FOURIER_LAUNCH_ITEMS)
};

}  // namespace fourier_hip
