// realnd_plan.h -- the plan behind a real-input N-D handle (fourier_hip_realnd_*, include/fourier.h): batched real-input transforms
// over the trailing `rank` (1 ... 4) dimensions of contiguous items [n_1, ..., n_{r-1}, W], numpy's rfftn / irfftn layout (the last
// axis is the real one and has W/2 + 1 complex values in the result).  Built on complex Plan<T>s that run unchanged, one per distinct
// length, through their axis routes (axis_plan.h).  Every item has R = n_1 x ... x n_{r-1} rows.
//
//   packed (even W = 2h)  forward: the reals as h complex values -> the h-point plan on the rows -> scratch -> one axis FFT in place
//                                  per leading dimension -> realnd_post_kernel (the untangle with mirror rows) -> X
//                         inverse: X -> realnd_pre_kernel (the projection of columns 0 and h, the scale folded in) -> scratch -> the
//                                  axis UNSCALED_IFFTs in place -> the h-point rows UNSCALED_IFFT from the scratch into the reals
//   composed (odd W)      forward: RealPlan(W) along the rows into X, the axis transforms in place over X with inner = (h+1) x trailing
//                         inverse: the axis inverses out of place from X into the scratch, RealPlan(W)'s inverse into the reals
//                                  (numpy's procedure; the rows' irfft drops Im of bins 0 and h after the leading inverses)
//   rank 1                a RealPlan(W): the same kernels and bits as fourier_hip_real_*
// The sweeps are kernels_real.h.  Items are walked in chunks of whole items that fit the scratch bound (never less than one item).
#pragma once
#include "real_plan.h"
#include "axis_plan.h"

namespace fourier_hip {

// The scratch bound is REAL_SCRATCH_BYTES; the experiments library and the emulator build read FOURIER_REALND_SCRATCH_BYTES at create
// instead (the chunk-walk tests)
constexpr int REALND_MAX_RANK = 4;

template <typename T> class RealNdPlan : public HandleBase {
 public:
  static constexpr size_t ELEM = sizeof(cpx<T>);

  RealNdPlan(int rank, const size_t* shape, int device) {
    if (!shape) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "null shape");
    if (rank < 1 || rank > REALND_MAX_RANK) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "rank outside 1 ... 4");
    shape_.assign(shape, shape + rank);
    double total = 1;
    for (size_t n : shape_) {
      if (n == 0) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "size 0 is invalid");
      total *= (double)n;
    }
    w_ = shape_.back();
    h_ = w_ / 2;
    rows_ = 1;
    for (int d = 0; d + 1 < rank; ++d) rows_ *= shape_[d];
    if ((double)rows_ * (double)(w_ / 2 + 1) * ELEM >= 9.2e18 || total * sizeof(T) >= 9.2e18 || rows_ >= ((size_t)1 << 32))
      throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "item too large");
    if (rank == 1) {
      rows1d_.reset(new RealPlan<T>(w_, device));
      desc_ = std::string("realnd rank 1: ") + rows1d_->describe();
      return;
    }
    packed_ = w_ % 2 == 0;
    if (packed_ && (h_ + 1) * ELEM > REAL_LAUNCH_BYTES / 2)
      throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "real transforms above 2^30 bytes of half spectrum");
    if (packed_ && (double)rows_ * (double)((h_ + 1) / 2 + 255) / 256 >= 2147483647.0)
      throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "too many rows per item");
    if (packed_) row_ = plan_of(h_, device);
    else rows1d_.reset(new RealPlan<T>(w_, device));
    for (int d = 0; d + 1 < rank; ++d) axis_.push_back(shape_[d] == 1 ? nullptr : plan_of(shape_[d], device));
    if (packed_) device_ = row_->device();
    else if (device >= 0) device_ = device;
    else if (hipGetDevice(&device_) != hipSuccess) device_ = 0;
    DeviceGuard g(device_);
    if (packed_) tw_.upload(real_untangle_twiddles<T>(w_));
    scratch_cap_ = scratch_bound("FOURIER_REALND_SCRATCH_BYTES", REAL_SCRATCH_BYTES);
    desc_ = std::string(packed_ ? "realnd packed: rows " : "realnd composed: rows ") + (packed_ ? row_->describe() : rows1d_->describe());
    const size_t cols = packed_ ? h_ : h_ + 1;
    for (size_t d = 0; d < axis_.size(); ++d) {
      desc_ += "; axis " + std::to_string(d) + " (" + std::to_string(shape_[d]) + "): ";
      desc_ += axis_[d] ? AxisRoute<T>::of(*axis_[d]).describe(inner(d, cols)) : std::string("identity");
    }
  }

  int rank() const { return (int)shape_.size(); }

  // items per chunk for a call of `batch` items; sizes the scratch, the row plan's and the axis routes' buffers for it (reserve:
  // ahead of time, so that later calls of at most `batch` items never allocate)
  size_t prepare(size_t batch) const {
    if (batch == 0) return 0;
    if (rank() == 1) { rows1d_->reserve(batch); return batch; }
    DeviceGuard g(device_);
    const size_t cols = packed_ ? h_ : h_ + 1, per = rows_ * cols * ELEM;
    const size_t chunk = chunk_rows(batch, scratch_cap_, per);
    scratch_.ensure(chunk * per);
    if (packed_) {
      row_->reserve_for(chunk * rows_, false);
    } else {
      rows1d_->reserve(chunk * rows_);
    }
    reserve_axes(chunk, cols);
    return chunk;
  }
  void reserve(size_t batch) const { (void)prepare(batch); }

  void forward(const void* d_in, void* d_out, size_t batch, int code, hipStream_t stream) const {
    check_buffers(d_in, d_out, batch * rows_ * w_ * sizeof(T), batch * rows_ * (h_ + 1) * ELEM, ELEM, false);
    if (!is_forward(code)) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "not a forward transform code");
    if (rank() == 1) return rows1d_->run_forward(d_in, d_out, batch, code, stream);
    if (batch == 0) return;
    DeviceGuard g(device_);
    const size_t chunk = prepare(batch);
    const T* in = (const T*)d_in;
    cpx<T>* out = (cpx<T>*)d_out;
    cpx<T>* work = (cpx<T>*)scratch_.p;
    const size_t xi = rows_ * (h_ + 1);
    for_chunks(batch, chunk, [&](size_t b0, size_t nb) {
      if (packed_) {
        row_->exec(in + b0 * rows_ * w_, work, nb * rows_, ::fourier::c::FOURIER_TRANSFORM_FFT, stream);
        axes(work, work, nb, h_, ::fourier::c::FOURIER_TRANSFORM_FFT, stream);
        sweep(REAL_ND_POST, work, out + b0 * xi, nb, item_scale(code), stream);
      } else {
        rows1d_->run_forward(in + b0 * rows_ * w_, out + b0 * xi, nb * rows_, code, stream);
        axes(out + b0 * xi, out + b0 * xi, nb, h_ + 1, code, stream);
      }
    });
  }

  void inverse(const void* d_in, void* d_out, size_t batch, int code, hipStream_t stream) const {
    check_buffers(d_in, d_out, batch * rows_ * (h_ + 1) * ELEM, batch * rows_ * w_ * sizeof(T), ELEM, false);
    if (!is_inverse(code)) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "not an inverse transform code");
    if (rank() == 1) return rows1d_->run_inverse(d_in, d_out, batch, code, stream);
    if (batch == 0) return;
    DeviceGuard g(device_);
    const size_t chunk = prepare(batch);
    const cpx<T>* in = (const cpx<T>*)d_in;
    T* out = (T*)d_out;
    cpx<T>* work = (cpx<T>*)scratch_.p;
    const size_t xi = rows_ * (h_ + 1);
    for_chunks(batch, chunk, [&](size_t b0, size_t nb) {
      if (packed_) {
        // the code's scale over P = W x R: the unscaled inverses of Z return P/2 times what the sweep wrote, and the sweep's S +- iT
        // carry a factor 2 (RealPlan::run_inverse with N = P)
        sweep(REAL_ND_PRE, in + b0 * xi, work, nb, item_scale(code), stream);
        axes(work, work, nb, h_, ::fourier::c::FOURIER_TRANSFORM_UNSCALED_IFFT, stream);
        row_->exec(work, out + b0 * rows_ * w_, nb * rows_, ::fourier::c::FOURIER_TRANSFORM_UNSCALED_IFFT, stream);
      } else {
        axes(in + b0 * xi, work, nb, h_ + 1, code, stream);
        rows1d_->run_inverse(work, out + b0 * rows_ * w_, nb * rows_, code, stream);
      }
    });
  }

  // ---- the stages of the packed route, for a handle that runs them around a sweep of its own on its own scratch (ConvNdPlan,
  // convnd_plan.h); rank >= 2
  bool packed() const { return packed_; }
  int device() const { return device_; }
  size_t rows() const { return rows_; }    // R = n_1 x ... x n_{r-1}
  size_t width() const { return w_; }      // W
  const std::vector<size_t>& shape() const { return shape_; }
  const Plan<T>& row_plan() const { return *row_; }  // the h-point plan of the rows (packed)
  // the axis routes' buffers for chunks of `chunk` items of rows x cols
  void reserve_axes(size_t chunk, size_t cols) const {
    for (size_t d = 0; d < axis_.size(); ++d)
      if (axis_[d]) AxisRoute<T>::of(*axis_[d]).reserve(outer(d, chunk), inner(d, cols));
  }
  // one axis transform per leading dimension over nb items of rows x cols, in place
  void axes_in_place(cpx<T>* z, size_t nb, size_t cols, int code, hipStream_t stream) const { axes(z, z, nb, cols, code, stream); }
  // the row indexing of an N-D sweep (realnd_rows, kernels_real.h) and the untangle twiddles; returns the workgroup size
  uint32_t sweep_geometry(RealArgs& a) const {
    const uint32_t lanes = (uint32_t)((h_ + 1) / 2);
    uint32_t threads = 64;
    while (threads < lanes && threads < REAL_THREADS_H) threads *= 2;
    const uint32_t segs = (lanes + threads - 1) / threads;
    a.tw = tw_.p;
    a.h = (uint32_t)h_;
    a.nd_rows = (uint32_t)rows_;
    a.lanes = lanes;
    a.segs = segs;
    const size_t lead = shape_.size() - 1;  // 1 ... 3 leading sizes, right-aligned into nd[0 .. 2]
    for (int i = 0; i < 3; ++i) a.nd[i] = 1;
    for (size_t d = 0; d < lead; ++d) a.nd[3 - lead + d] = (uint32_t)shape_[d];
    divider(segs, a.seg_m, a.seg_l);
    divider((uint32_t)rows_, a.row_m, a.row_l);
    divider(a.nd[2], a.c_m, a.c_l);
    divider(a.nd[1], a.b_m, a.b_l);
    return threads;
  }

 private:
  // one complex plan per distinct length
  const Plan<T>* plan_of(size_t n, int device) {
    for (auto& p : plans_)
      if (p->size() == n) return p.get();
    plans_.emplace_back(new Plan<T>(n, device));
    return plans_.back().get();
  }

  // the leading dimension d of `nb` items of rows x cols: [outer][n_d][inner]
  size_t outer(size_t d, size_t nb) const {
    size_t o = nb;
    for (size_t e = 0; e < d; ++e) o *= shape_[e];
    return o;
  }
  size_t inner(size_t d, size_t cols) const {
    size_t c = cols;
    for (size_t e = d + 1; e + 1 < shape_.size(); ++e) c *= shape_[e];
    return c;
  }

  // one axis transform per leading dimension: the first from `in` to `out`, the others in place in `out`
  void axes(const cpx<T>* in, cpx<T>* out, size_t nb, size_t cols, int code, hipStream_t stream) const {
    const cpx<T>* src = in;
    for (size_t d = 0; d < axis_.size(); ++d) {
      if (!axis_[d]) continue;  // a 1-point transform is the identity under every code
      AxisRoute<T>::of(*axis_[d]).transform(src, out, outer(d, nb), inner(d, cols), code, stream);
      src = out;
    }
    if (src != out) HIP_CHECK(hipMemcpyAsync(out, in, nb * rows_ * cols * ELEM, hipMemcpyDeviceToDevice, stream));
  }

  // the code's scale over the product P of the transformed lengths
  double item_scale(int code) const { return code_scale<T>(code, (T)((double)rows_ * (double)w_)); }

  // the N-D sweep over nb items: one workgroup per row and segment of lanes, launches of whole items with fewer than 2^31 workgroups
  void sweep(int which, const cpx<T>* in, cpx<T>* out, size_t nb, double scale, hipStream_t stream) const {
    RealArgs a{};
    const uint32_t threads = sweep_geometry(a), segs = a.segs;
    a.scale = scale;
    const bool post = which == REAL_ND_POST;
    const size_t zi = rows_ * h_, xi = rows_ * (h_ + 1);
    const size_t per = std::max<size_t>(1, (size_t)0x7fffffff / ((size_t)rows_ * segs));
    for (size_t b0 = 0; b0 < nb; b0 += per) {
      const size_t n = std::min(per, nb - b0);
      a.in = post ? (const void*)(in + b0 * zi) : (const void*)(in + b0 * xi);
      a.out = post ? (void*)(out + b0 * xi) : (void*)(out + b0 * zi);
      FOURIER_LAUNCH(get_real_kernel(Real<T>{}, which), (uint64_t)n * rows_ * segs, threads, 0, stream, a);
    }
  }

  static constexpr uint32_t REAL_THREADS_H = 256;  // REAL_THREADS of kernels_real.h
  std::vector<size_t> shape_;
  size_t w_ = 0, h_ = 0, rows_ = 1;
  bool packed_ = false;
  int device_ = 0;
  std::vector<std::unique_ptr<Plan<T>>> plans_;
  const Plan<T>* row_ = nullptr;
  std::vector<const Plan<T>*> axis_;  // per leading dimension; null: length 1
  std::unique_ptr<RealPlan<T>> rows1d_;
  DevBuf tw_;
  mutable DevBuf scratch_;
  size_t scratch_cap_ = REAL_SCRATCH_BYTES;
};

}  // namespace fourier_hip
