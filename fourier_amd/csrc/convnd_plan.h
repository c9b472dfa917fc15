// convnd_plan.h -- the plan behind an N-D convolution handle (fourier_hip_convnd_*, include/fourier.h): batched circular convolution
// or correlation of real items over their trailing `rank` (2 ... 4) dimensions with a prepared bank of F filters.  With the transform
// shape S = [n_1, ..., n_{r-1}, W] and P = prod S, item b is zero-extended from in_shape <= S at the high end of every dimension,
// convolved circularly over S with filter (filter_first + b) mod F, and the window [out_first, out_first + out_shape) is stored:
//   y = irfftn(rfftn(x, S) * H[f], S),  H[f] = rfftn(h[f] zero-extended to S) / P  (conjugated for a correlation).
// Built on a RealNdPlan<T> of shape S (realnd_plan.h) that runs unchanged: it transforms the filters, runs the composed route, and lends
// the stages of its packed route (the row plan, the axis routes, the untangle twiddles, the mirror-row indexing) to the fused one.
// Routes, chosen at create and by option "fusion":
//   "convnd fused untangle"  even W = 2h: [pad sweep -> scratch] -> the h-point row plan forward (from the input, or in place after a
//                            pad) -> the axis FFTs in place -> ONE realnd_conv_mid_kernel launch in place (untangle, product, retangle)
//                            -> the axis unscaled inverses in place -> the row plan's unscaled inverse (to the output; in place with
//                            a crop sweep behind it under any other window).  The half spectrum never reaches memory.
//   "convnd composed"        odd W, or "fusion" = 0: [pad] -> RealNdPlan forward -> half-spectrum scratch -> the product sweep
//                            (conv_mul_kernel; convnd_mul_kernel where an item is beyond its 32-bit index) -> RealNdPlan unscaled
//                            inverse -> [crop].
// The sweeps are kernels_convnd.h.  Items are walked in chunks of whole items that fit the scratch bound (never less than one item);
// the filter of an item counts over the whole call.
#pragma once
#include "realnd_plan.h"

namespace fourier_hip {

// The scratch bound is REAL_SCRATCH_BYTES; the experiments library and the emulator build read FOURIER_CONVND_SCRATCH_BYTES at create
// instead (the chunk-walk tests), and FOURIER_LAUNCH_ITEMS for the workgroups of one launch of the new sweeps.
template <typename T> class ConvNdPlan : public HandleBase {
 public:
  static constexpr size_t ELEM = sizeof(cpx<T>);
  static constexpr size_t LAUNCH_WORKGROUPS = 0x7fffffff;

  ConvNdPlan(int rank, const size_t* shape, int device) {
    if (!shape) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "null shape");
    if (rank < 2 || rank > REALND_MAX_RANK)  // rank 1 is fourier_hip_conv_*
      throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "rank outside 2 ... 4");
    nd_.reset(new RealNdPlan<T>(rank, shape, device));  // size 0 and the item bounds: RealNdPlan's
    shape_ = nd_->shape();
    rows_ = nd_->rows();
    w_ = nd_->width();
    h_ = w_ / 2;
    device_ = nd_->device();
    if ((double)rows_ * (double)((w_ + LCONV_SEG - 1) / LCONV_SEG) >= 2147483647.0 || (double)rows_ * (double)(h_ / 256 + 1) >= 2147483647.0)
      throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "too many rows per item");
    in_shape_ = out_shape_ = shape_;
    out_first_.assign(shape_.size(), 0);
    scratch_cap_ = scratch_bound("FOURIER_CONVND_SCRATCH_BYTES", REAL_SCRATCH_BYTES);
    launch_items_ = launch_bound("FOURIER_LAUNCH_ITEMS", LAUNCH_WORKGROUPS);
    set_fusion(true);
  }

  int rank() const { return (int)shape_.size(); }
  const std::vector<size_t>& shape() const { return shape_; }
  size_t filters() const { return filters_; }

  int set_option(const std::string& key, long long v) {
    if (key == "fusion" && (v == 0 || v == 1)) { set_fusion(v == 1); return ::fourier::c::FOURIER_HIP_OK; }
    return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
  }

  // host state: the extent of the caller's items and the stored window of the result; may be called between applies
  void set_window(const size_t* in_shape, const size_t* out_first, const size_t* out_shape) {
    if (!in_shape || !out_first || !out_shape) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "null window");
    for (size_t d = 0; d < shape_.size(); ++d)
      if (in_shape[d] == 0 || in_shape[d] > shape_[d] || out_shape[d] == 0 || out_shape[d] > shape_[d] || out_first[d] > shape_[d] - out_shape[d])
        throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "window outside the transform shape");
    in_shape_.assign(in_shape, in_shape + shape_.size());
    out_first_.assign(out_first, out_first + shape_.size());
    out_shape_.assign(out_shape, out_shape + shape_.size());
  }

  // items per chunk for a call of `batch` items; sizes the scratch, the row plan's and the axis routes' buffers for it
  size_t prepare(size_t batch) const {
    if (batch == 0) return 0;
    DeviceGuard g(device_);
    const size_t chunk = chunk_rows(batch, scratch_cap_, item_bytes());
    scratch_.ensure(chunk * item_bytes());
    if (fused_) {
      nd_->row_plan().reserve_for(chunk * rows_, false);
      nd_->row_plan().reserve_for(chunk * rows_, true);
      nd_->reserve_axes(chunk, h_);
    } else {
      nd_->reserve(chunk);
    }
    return chunk;
  }
  void reserve(size_t batch) const { (void)prepare(batch); }

  // `filters` contiguous blocks of taps_shape <= S reals at d_taps -> the bank of half spectra [rows][h + 1], on `stream`
  void set_filters(const void* d_taps, const size_t* taps_shape, size_t filters, bool correlate, hipStream_t stream) {
    if (!d_taps || !taps_shape) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "null taps");
    if ((uintptr_t)d_taps % sizeof(T)) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "misaligned taps");
    for (size_t d = 0; d < shape_.size(); ++d)
      if (taps_shape[d] == 0 || taps_shape[d] > shape_[d]) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "taps outside 1 ... S");
    if (filters == 0) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "no filters");
    if (filters > 0x7fffffffull) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "more than 2^31 filters");
    const size_t xi = rows_ * (h_ + 1);
    if ((double)filters * (double)xi * ELEM >= 9.2e18) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "bank too large");
    DeviceGuard g(device_);
    bank_.ensure(filters * xi * ELEM);
    // the zero-extended taps of a chunk of filters in the scratch (an item of P reals fits a scratch item on either route), the handle's
    // own forward transform in T into the bank, then 1/P and the conjugate in place
    const std::vector<size_t> taps(taps_shape, taps_shape + shape_.size()), zero(shape_.size(), 0);
    const size_t chunk = chunk_rows(filters, scratch_cap_, item_bytes());
    scratch_.ensure(chunk * item_bytes());
    nd_->reserve(chunk);
    cpx<T>* bank = (cpx<T>*)bank_.p;
    for_chunks(filters, chunk, [&](size_t f0, size_t nf) {
      window_copy(CONVND_PAD, (const T*)d_taps + f0 * count(taps), taps, (T*)scratch_.p, shape_, zero, nf, stream);
      nd_->forward(scratch_.p, bank + f0 * xi, nf, ::fourier::c::FOURIER_TRANSFORM_FFT, stream);
    });
    ConvArgs a{};
    a.out = bank;
    a.count = filters * xi;
    a.scale = code_scale<T>(::fourier::c::FOURIER_TRANSFORM_IFFT, (T)((double)rows_ * (double)w_));  // the inverse's 1/P, folded into the bank
    a.conj = correlate;
    FOURIER_LAUNCH(get_conv_sweep_kernel(Real<T>{}, CONV_FINISH), elementwise_grid(a.count), 256, 0, stream, a);
    filters_ = filters;
  }

  // `batch` items of in_shape reals at d_in -> `batch` items of out_shape reals at d_out, item b with filter (first + b) mod F
  void apply(const void* d_in, void* d_out, size_t batch, size_t first, hipStream_t stream) const {
    const size_t in_item = count(in_shape_), out_item = count(out_shape_), full = rows_ * w_;
    const bool whole_in = in_shape_ == shape_, whole_out = out_shape_ == shape_;
    if ((double)batch * (double)full * sizeof(T) >= 9.2e18) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "call too large");
    check_buffers(d_in, d_out, batch * in_item * sizeof(T), batch * out_item * sizeof(T), ELEM, whole_in && whole_out);
    if (filters_ == 0) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "no filters set");
    if (batch == 0) return;
    DeviceGuard g(device_);
    const size_t chunk = prepare(batch);
    // the transforms read and write whole items of P reals as pairs: an odd P goes through the scratch like a window
    const bool pad = !whole_in || (!fused_ && full % 2), crop = !whole_out || (!fused_ && full % 2);
    const T* in = (const T*)d_in;
    T* out = (T*)d_out;
    const std::vector<size_t> zero(shape_.size(), 0);
    const int FWD = ::fourier::c::FOURIER_TRANSFORM_FFT, INV = ::fourier::c::FOURIER_TRANSFORM_UNSCALED_IFFT;
    const size_t xi = rows_ * (h_ + 1);
    for_chunks(batch, chunk, [&](size_t c0, size_t nb) {
      const size_t b0 = first + c0;
      if (fused_) {
        cpx<T>* z = (cpx<T>*)scratch_.p;  // nb items of rows x h
        if (pad) window_copy(CONVND_PAD, in + c0 * in_item, in_shape_, (T*)z, shape_, zero, nb, stream);
        nd_->row_plan().exec(pad ? (const void*)z : (const void*)(in + c0 * full), z, nb * rows_, FWD, stream);
        nd_->axes_in_place(z, nb, h_, FWD, stream);
        mid_sweep(z, nb, b0, stream);
        nd_->axes_in_place(z, nb, h_, INV, stream);
        nd_->row_plan().exec(z, crop ? (void*)z : (void*)(out + c0 * full), nb * rows_, INV, stream);
        if (crop) window_copy(CONVND_CROP, (const T*)z, shape_, out + c0 * out_item, out_shape_, out_first_, nb, stream);
      } else {
        cpx<T>* x = (cpx<T>*)scratch_.p;  // nb half spectra of rows x (h + 1), then nb items of reals for the windows
        T* y = (T*)(x + chunk * xi);
        if (pad) window_copy(CONVND_PAD, in + c0 * in_item, in_shape_, y, shape_, zero, nb, stream);
        nd_->forward(pad ? (const void*)y : (const void*)(in + c0 * full), x, nb, FWD, stream);
        mul_sweep(x, nb, b0, stream);
        nd_->inverse(x, crop ? (void*)y : (void*)(out + c0 * full), nb, INV, stream);
        if (crop) window_copy(CONVND_CROP, y, shape_, out + c0 * out_item, out_shape_, out_first_, nb, stream);
      }
    });
  }

 private:
  static size_t count(const std::vector<size_t>& s) {
    size_t c = 1;
    for (size_t n : s) c *= n;
    return c;
  }
  void set_fusion(bool on) {
    fused_ = on && nd_->packed();
    desc_ = std::string(fused_ ? "convnd fused untangle: " : "convnd composed: ") + nd_->describe();
  }
  // scratch bytes per item of a chunk: the packed rows of the fused route (a half spectrum's size keeps one size for set_filters); the
  // half spectrum and the reals of a windowed item on the composed route
  size_t item_bytes() const { return (fused_ ? 1 : 2) * rows_ * (h_ + 1) * ELEM; }

  // convnd_pad_kernel / convnd_crop_kernel: nb items of `sshape` at src -> nb items of `dshape` at dst, destination element i from source
  // element i + off (pad: zero where that is outside the source item), in launches of whole items of at most launch_items_ workgroups
  void window_copy(int which, const T* src, const std::vector<size_t>& sshape, T* dst, const std::vector<size_t>& dshape,
                   const std::vector<size_t>& off, size_t nb, hipStream_t stream) const {
    ConvNdArgs a{};
    const size_t lead = shape_.size() - 1;  // 1 ... 3 leading sizes, right-aligned
    for (int i = 0; i < 3; ++i) { a.dl[i] = a.sl[i] = 1; a.off[i] = 0; }
    for (size_t d = 0; d < lead; ++d) {
      a.dl[3 - lead + d] = (uint32_t)dshape[d];
      a.sl[3 - lead + d] = (uint32_t)sshape[d];
      a.off[3 - lead + d] = (uint32_t)off[d];
    }
    a.dw = dshape[lead]; a.sw = sshape[lead]; a.offw = off[lead];
    a.dlines = a.dl[0] * a.dl[1] * a.dl[2];
    a.slines = a.sl[0] * a.sl[1] * a.sl[2];
    a.segs = (uint32_t)((a.dw + LCONV_SEG - 1) / LCONV_SEG);
    divider(a.segs, a.seg_m, a.seg_l);
    divider(a.dlines, a.line_m, a.line_l);
    divider(a.dl[2], a.c_m, a.c_l);
    divider(a.dl[1], a.b_m, a.b_l);
    const size_t per = std::max<size_t>(1, launch_items_ / ((size_t)a.dlines * a.segs));
    for_chunks(nb, per, [&](size_t b0, size_t n) {
      a.src = src + b0 * a.slines * a.sw;
      a.dst = dst + b0 * a.dlines * a.dw;
      FOURIER_LAUNCH(get_convnd_kernel(Real<T>{}, which), (uint64_t)n * a.dlines * a.segs, 256, 0, stream, a);
    });
  }

  // realnd_conv_mid_kernel over nb items of the scratch; b0: the first item's filter count
  void mid_sweep(cpx<T>* z, size_t nb, size_t b0, hipStream_t stream) const {
    ConvNdArgs a{};
    const uint32_t threads = nd_->sweep_geometry(a.r);
    set_bank(a);
    const size_t per = std::max<size_t>(1, launch_items_ / ((size_t)rows_ * a.r.segs));
    for_chunks(nb, per, [&](size_t i0, size_t n) {
      a.r.in = a.r.out = z + i0 * rows_ * h_;
      a.first = (uint32_t)((b0 + i0) % filters_);
      FOURIER_LAUNCH(get_convnd_kernel(Real<T>{}, CONVND_MID), (uint64_t)n * rows_ * a.r.segs, threads, 0, stream, a);
    });
  }

  // the composed route's product over nb half spectra: conv_mul_kernel on items as its rows where an item fits its 32-bit flat index
  // and the launch bound, else convnd_mul_kernel
  void mul_sweep(cpx<T>* x, size_t nb, size_t b0, hipStream_t stream) const {
    const size_t xi = rows_ * (h_ + 1);
    if (xi * ELEM <= REAL_LAUNCH_BYTES && (xi + 255) / 256 <= launch_items_) {
      const size_t per = std::max<size_t>(1, std::min(REAL_LAUNCH_BYTES / (xi * ELEM), launch_items_ / ((xi + 255) / 256)));
      for_chunks(nb, per, [&](size_t i0, size_t n) {
        ConvArgs a{};
        a.in = a.out = x + i0 * xi;
        a.bank = bank_.p;
        a.len = (uint32_t)xi;
        a.total = (uint32_t)(n * xi);
        divider(a.len, a.div_m, a.div_l);
        a.filters = (uint32_t)filters_;
        a.first = (uint32_t)((b0 + i0) % filters_);
        divider(a.filters, a.f_m, a.f_l);
        a.bytes = (uint32_t)(n * xi * ELEM);
        FOURIER_LAUNCH(get_conv_sweep_kernel(Real<T>{}, CONV_MUL), (a.total + 255) / 256, 256, 0, stream, a);
      });
      return;
    }
    ConvNdArgs a{};
    set_bank(a);
    a.dlines = (uint32_t)rows_;
    a.dw = h_ + 1;
    a.segs = (uint32_t)((h_ + 1 + 255) / 256);
    divider(a.segs, a.seg_m, a.seg_l);
    divider(a.dlines, a.line_m, a.line_l);
    const size_t per = std::max<size_t>(1, launch_items_ / ((size_t)rows_ * a.segs));
    for_chunks(nb, per, [&](size_t i0, size_t n) {
      a.dst = x + i0 * xi;
      a.first = (uint32_t)((b0 + i0) % filters_);
      FOURIER_LAUNCH(get_convnd_kernel(Real<T>{}, CONVND_MUL), (uint64_t)n * rows_ * a.segs, 256, 0, stream, a);
    });
  }
  void set_bank(ConvNdArgs& a) const {
    a.bank = bank_.p;
    a.filters = (uint32_t)filters_;
    divider(a.filters, a.f_m, a.f_l);
  }

  std::unique_ptr<RealNdPlan<T>> nd_;  // shape S: set_filters, the composed route; its stages run the fused route
  std::vector<size_t> shape_, in_shape_, out_first_, out_shape_;
  size_t rows_ = 1, w_ = 0, h_ = 0;
  int device_ = 0;
  bool fused_ = false;
  size_t filters_ = 0;
  DevBuf bank_;  // F half spectra of rows x (h + 1), 1/P and the conjugate folded in
  mutable DevBuf scratch_;
  size_t scratch_cap_ = REAL_SCRATCH_BYTES;
  size_t launch_items_ = LAUNCH_WORKGROUPS;  // workgroups of one launch of the new sweeps (development switch FOURIER_LAUNCH_ITEMS)
};

}  // namespace fourier_hip
