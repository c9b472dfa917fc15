// axis_plan.h -- transforms along a strided axis (fourier_hip_transform_axis_*, include/fourier.h): a plan of length N transforms
// the middle axis of an [outer][N][inner] array of interleaved complex T, element (o, j, c) at (o*N + j)*inner + c, into the same
// layout.  The route is chosen from N and inner alone:
//
//   rows         inner == 1                                   Plan::exec, unchanged (the same kernels, the same bits)
//   lane         N <= 32                                      axis_lane_kernel<T, N>: one HBM round trip
//   column tile  N = 2^k in 64 ... 2048, inner = 2^m >= the   the last pass of every two-pass power-of-two plan, fft_pass_kernel<T,
//                kernel's COLS, (N/16) * inner * sizeof(cpx)  N, CG, MODE_LAST>, IS a length-N transform down the columns of an
//                <= 2^31 (its 32-bit lane offsets)            N x s block: launched with s = inner, one HBM round trip
//   transpose    everything else                              axis_transpose_kernel<T> into plan-owned scratch (contiguous rows),
//                                                             Plan::exec in place there, the transpose back: 2 + the plan's own
//
// The transpose route walks the call in chunks of whole outer blocks that fit the scratch bound; a block larger than the bound is
// walked by column ranges (and, where a column range spans more than AXIS_LAUNCH_BYTES of the user array, by row bands per launch).
#pragma once
#include "plan.h"

namespace fourier_hip {

// Scratch bound of the transpose route, the size of REAL_SCRATCH_BYTES (real_plan.h).  The experiments library and the emulator build read
// FOURIER_AXIS_SCRATCH_BYTES at create instead (the chunk-walk tests); FOURIER_AXIS_ROUTE=transpose sends every call with
// inner > 1 through the transpose route (the A/B of the bench tool, the route-agreement tests).
constexpr size_t AXIS_SCRATCH_BYTES = (size_t)1 << 30;
// Bytes of either side of one transpose launch: the kernel addresses with 31-bit byte offsets
constexpr size_t AXIS_LAUNCH_BYTES = ((size_t)1 << 31) - 1;

template <typename T> class AxisRoute {
 public:
  static constexpr size_t ELEM = sizeof(cpx<T>);
  enum Route { ROWS, LANE, COLUMN, TRANSPOSE };

  // the plan's route object, built on its first axis call
  static AxisRoute& of(const Plan<T>& p) {
    if (!p.axis_) p.axis_.reset(new AxisRoute(p));
    return *p.axis_;
  }

  Route route(size_t inner) const {
    if (inner == 1) return ROWS;
    if (p_.axis_force_transpose_) return TRANSPOSE;
    if (n_ <= 32) return LANE;
    if (col_.fn && is_pow2(inner) && inner >= (size_t)col_.COLS && (double)(n_ / 16) * (double)inner * ELEM <= 2147483648.0) return COLUMN;
    return TRANSPOSE;
  }

  const char* describe(size_t inner) const {
    switch (route(inner)) {
      case ROWS: return p_.describe();
      case LANE: return lane_desc_.c_str();
      case COLUMN: return col_desc_.c_str();
      default: return tr_desc_.c_str();
    }
  }

  void reserve(size_t outer, size_t inner) const {
    if (outer == 0 || inner == 0) return;
    DeviceGuard g(p_.device());
    switch (route(inner)) {
      case ROWS: p_.reserve_for(outer, false); p_.reserve_for(outer, true); return;
      case TRANSPOSE: (void)prepare(outer, inner); return;
      default: return;
    }
  }

  void transform(const void* d_in, void* d_out, size_t outer, size_t inner, int code, hipStream_t stream) const {
    if (code < 0 || code > 4) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "unknown transform code");
    const double total = (double)outer * (double)inner * (double)n_;
    if (total * ELEM >= 9.2e18) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "array too large");
    const size_t bytes = outer * inner * n_ * ELEM;
    check_buffers(d_in, d_out, bytes, bytes, ELEM, true);
    if (outer == 0 || inner == 0) return;
    DeviceGuard g(p_.device());
    const bool inverse = !is_forward(code);
    const double scale = code_scale<T>(code, (T)n_);
    const cpx<T>* in = (const cpx<T>*)d_in;
    cpx<T>* out = (cpx<T>*)d_out;
    switch (route(inner)) {
      case ROWS: p_.exec(d_in, d_out, outer, code, stream); return;
      case LANE: run_lane(in, out, outer, inner, inverse, scale, stream); return;
      case COLUMN: run_column(in, out, outer, inner, inverse, scale, stream); return;
      default: run_transpose(in, out, outer, inner, code, stream); return;
    }
  }

 private:
  explicit AxisRoute(const Plan<T>& p) : p_(p), n_(p.size()) {
    cap_ = std::min(p.axis_scratch_bytes_ ? p.axis_scratch_bytes_ : AXIS_SCRATCH_BYTES, AXIS_LAUNCH_BYTES);
    DeviceGuard g(p.device());
    if (is_pow2(n_) && n_ >= 64 && n_ <= 2048) {
      col_ = get_kernel(Real<T>{}, (int)n_, MODE_LAST, IO_PLAIN);
      if (col_.split) col_ = KernelInfo();  // (experiments: the half-tile form of 2048 takes other arguments; transpose route then)
    }
    if (col_.fn) {
      raise_smem_limit((const void*)col_.fn, col_.smem);
      make_stage_tables<T>((int)n_, st_);
    }
    lane_desc_ = "axis lane: " + std::to_string(n_);
    col_desc_ = "axis column tile: L=" + std::to_string(n_);
    tr_desc_ = std::string("axis transpose: ") + p.describe();
  }

  // ---- lane: launches over whole outer blocks and column ranges such that a launch has fewer than 2^31 lanes
  void run_lane(const cpx<T>* in, cpx<T>* out, size_t outer, size_t inner, bool inverse, double scale, hipStream_t stream) const {
    if (n_ == 1 && in == out) return;  // the 1-point transform is the identity (every scale of N = 1 is 1)
    const size_t LANES = (size_t)1 << 30;
    const size_t w = std::min(inner, LANES), per = std::max<size_t>(1, LANES / w);
    const AxisKernel fn = get_axis_kernel(Real<T>{}, (int)n_);
    for (size_t o0 = 0; o0 < outer; o0 += per) {
      const size_t nb = std::min(per, outer - o0);
      for (size_t c0 = 0; c0 < inner; c0 += w) {
        const size_t cw = std::min(w, inner - c0);
        AxisArgs a{};
        a.in = in + o0 * n_ * inner + c0;
        a.out = out + o0 * n_ * inner + c0;
        a.block = n_ * inner;
        a.inner = inner;
        a.cols = (uint32_t)cw;
        a.total = (uint32_t)(nb * cw);
        divider((uint32_t)cw, a.div_m, a.div_l);
        a.swap = inverse;
        a.scale = scale;
        FOURIER_LAUNCH(fn, (a.total + AXIS_THREADS_H - 1) / AXIS_THREADS_H, AXIS_THREADS_H, 0, stream, a);
      }
    }
  }

  // ---- column tile: the MODE_LAST pass of length N over N x inner blocks, set up as Pow2Engine::launch_pass sets up a last pass
  void run_column(const cpx<T>* in, cpx<T>* out, size_t outer, size_t inner, bool inverse, double scale, hipStream_t stream) const {
    const uint64_t tiles = inner / (uint64_t)col_.COLS;
    const size_t per = std::max<size_t>(1, (size_t)(0x7fffffffull / tiles));  // workgroups of a launch below 2^31
    for (size_t o0 = 0; o0 < outer; o0 += per) {
      const size_t nb = std::min(per, outer - o0);
      PassArgs a;
      std::memset(&a, 0, sizeof(a));
      a.in = in + o0 * n_ * inner;
      a.out = out + o0 * n_ * inner;
      a.tw1 = st_.tw1.p; a.tw2 = st_.tw2.p;
      a.n = n_ * inner; a.cn = inner; a.s = inner; a.s_shift = (uint32_t)ilog2(inner);
      a.tiles = tiles;
      a.nxcd = 8;  // every XCD walks a contiguous range of tiles (the plan default, xcd_remap mode 0)
      a.swap_in = inverse; a.swap_out = inverse;  // the only pass: leading and trailing swap
      a.scale = scale;
      FOURIER_LAUNCH(col_.fn, (uint64_t)nb * tiles, col_.NT, col_.smem, stream, a);
    }
  }

  // ---- transpose: chunk walk through the scratch
  struct Chunk { size_t blocks, cols; };  // whole outer blocks per chunk, or (blocks == 0) columns per chunk of one block
  Chunk prepare(size_t outer, size_t inner) const {
    const size_t blk = n_ * inner * ELEM;
    Chunk c{0, 0};
    if (blk <= cap_) c.blocks = chunk_rows(outer, cap_, blk);
    else c.cols = std::max<size_t>(1, cap_ / (n_ * ELEM));
    const size_t rows = c.blocks ? c.blocks * inner : c.cols;
    scratch_.ensure(rows * n_ * ELEM);
    p_.reserve_for(rows, true);
    return c;
  }

  // blocks x (rows x cols, leading dimension ld_in, block stride bs_in) -> blocks x (cols x rows, ld_out, bs_out)
  void transpose(const cpx<T>* src, cpx<T>* dst, size_t blocks, size_t rows, size_t cols, size_t ld_in, size_t ld_out, size_t bs_in,
                 size_t bs_out, hipStream_t stream) const {
    AxisArgs a{};
    a.in = src; a.out = dst;
    a.rows = (uint32_t)rows; a.cols = (uint32_t)cols;
    a.tiles_r = (uint32_t)((rows + 31) / 32); a.tiles_c = (uint32_t)((cols + 31) / 32);
    a.blocks = (uint32_t)blocks;
    a.ld_in = (uint32_t)ld_in; a.ld_out = (uint32_t)ld_out;
    a.bs_in = bs_in; a.bs_out = bs_out;
    a.in_bytes = (uint32_t)(((blocks - 1) * bs_in + (rows - 1) * ld_in + cols) * ELEM);
    a.out_bytes = (uint32_t)(((blocks - 1) * bs_out + (cols - 1) * ld_out + rows) * ELEM);
    const uint64_t grid = (uint64_t)blocks * a.tiles_r * a.tiles_c;
    FOURIER_LAUNCH(get_axis_kernel(Real<T>{}, 0), grid, AXIS_THREADS_H, 32 * 33 * ELEM, stream, a);
  }

  void run_transpose(const cpx<T>* in, cpx<T>* out, size_t outer, size_t inner, int code, hipStream_t stream) const {
    const Chunk ch = prepare(outer, inner);
    cpx<T>* work = (cpx<T>*)scratch_.p;
    const size_t blk = n_ * inner;
    if (ch.blocks) {  // whole outer blocks: [nb][N][inner] -> [nb * inner][N] -> transform -> back
      for (size_t o0 = 0; o0 < outer; o0 += ch.blocks) {
        const size_t nb = std::min(ch.blocks, outer - o0);
        transpose(in + o0 * blk, work, nb, n_, inner, inner, n_, blk, blk, stream);
        p_.exec(work, work, nb * inner, code, stream);
        transpose(work, out + o0 * blk, nb, inner, n_, n_, inner, blk, blk, stream);
      }
      return;
    }
    // one block is larger than the scratch: column ranges of cw columns, in row bands whose user-side span fits one launch
    for (size_t o = 0; o < outer; ++o) {
      for (size_t c0 = 0; c0 < inner; c0 += ch.cols) {
        const size_t cw = std::min(ch.cols, inner - c0);
        const size_t band = std::min(n_, (AXIS_LAUNCH_BYTES / ELEM - cw) / inner + 1);
        for (size_t r0 = 0; r0 < n_; r0 += band)
          transpose(in + o * blk + r0 * inner + c0, work + r0, 1, std::min(band, n_ - r0), cw, inner, n_, 0, 0, stream);
        p_.exec(work, work, cw, code, stream);
        for (size_t r0 = 0; r0 < n_; r0 += band)
          transpose(work + r0, out + o * blk + r0 * inner + c0, 1, cw, std::min(band, n_ - r0), n_, inner, 0, 0, stream);
      }
    }
  }

  static constexpr unsigned AXIS_THREADS_H = 256;  // AXIS_THREADS of kernels_axis.h
  const Plan<T>& p_;
  size_t n_;
  size_t cap_;
  KernelInfo col_;
  StageTables<T> st_;
  mutable DevBuf scratch_;
  std::string lane_desc_, col_desc_, tr_desc_;
};

}  // namespace fourier_hip
