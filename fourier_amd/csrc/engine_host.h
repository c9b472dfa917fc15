// engine_host.h -- the host code the engines share (engine_pow2.h, engine_mixed.h, engine_tiled.h, engine_generic.h): one builder per
// twiddle-table layout and one launch sequence.  Host code only: the engine headers include it, no kernel translation unit does.
#pragma once
#include "engine_common.h"

namespace fourier_hip {

// W_size^e: f64 trigonometry, cast (twiddle.rs:7-19)
template <typename T> static inline cpx<T> root(uint64_t e, uint64_t size) {
  double re, im;
  unit_root(e, size, re, im);
  return {(T)re, (T)im};
}

// W_size^e as a two-level table, W^e = lo[e & mask] * hi[e >> lo_bits]: uploads both halves and returns lo_bits
template <typename T> static uint32_t upload_two_level(uint64_t size, DevBuf& lo_buf, DevBuf& hi_buf) {
  const int lb = (ilog2(size) + 1) / 2;
  std::vector<cpx<T>> lo((size_t)1 << lb), hi((size_t)(size >> lb) + 1);  // +1: size need not be a power of two
  for (size_t e = 0; e < lo.size(); ++e) lo[e] = root<T>(e, size);
  for (size_t h = 0; h < hi.size(); ++h) hi[h] = root<T>((uint64_t)h << lb, size);
  lo_buf.upload(lo);
  hi_buf.upload(hi);
  return (uint32_t)lb;
}

// W_size^{row * col} as [row < rows][col < cols]: the twiddle between two register stages (size = L = r1 x r2, [k1 < r1][j2 < r2]) and the
// full inter-pass table of a one-launch plan (size = N = rows x cols)
template <typename T> static std::vector<cpx<T>> product_table(uint64_t size, uint64_t rows, uint64_t cols) {
  std::vector<cpx<T>> tw((size_t)(rows * cols));
  for (uint64_t r = 0; r < rows; ++r)
    for (uint64_t c = 0; c < cols; ++c) tw[(size_t)(r * cols + c)] = root<T>(r * c, size);
  return tw;
}

// twiddle.rs:7-19 verbatim: theta = (index*2) as f64 * PI / size as f64; (cos, -sin) cast to T.
// cos and sin stay two separate libm calls, as in Rust (a merged sincos() differs in the last bit).
__attribute__((noinline)) static double libm_cos(double t) { return std::cos(t); }
__attribute__((noinline)) static double libm_sin(double t) { return std::sin(t); }
template <typename T> static cpx<T> ref_twiddle(size_t index, size_t size) {
  const double theta = (double)(index * 2) * M_PI / (double)size;
  return {(T)libm_cos(theta), (T)(-libm_sin(theta))};
}
// the reference's tables of a plan of length n on the radix sequence `radices` (mod.rs:24-46); twiddle(index, size): ref_twiddle<T>, or
// the tile passes' own expression (engine_tiled.h)
template <typename T, typename F> static std::vector<cpx<T>> ref_schedule_table(size_t n, const std::vector<uint32_t>& radices, F twiddle) {
  std::vector<cpx<T>> tw;
  size_t cur = n;
  for (const size_t R : radices) {
    const size_t m = cur / R;
    for (size_t i = 0; i < m; ++i) {
      tw.push_back({(T)1, (T)0});
      for (size_t j = 1; j < R; ++j) tw.push_back(twiddle(i * j, cur));
    }
    cur /= R;
  }
  return tw;
}

// the tile order of a pass as the plan encodes it: XCDs | block -> tile mode << 8 | tiles per band << 12 | transforms per group << 20 |
// transform-fastest << 30 (Plan::set_option "xcd_swizzle", "tile_walk")
static inline void set_tile_order(PassArgs& a, unsigned nxcd) {
  a.nxcd = nxcd & 0xff;
  a.xcd_interleave = (nxcd >> 8) & 7;
  a.walk_band = (nxcd >> 12) & 0xff; a.walk_group = (nxcd >> 20) & 0x3ff; a.walk_tf = nxcd >> 30;
}

static inline void check_grid(uint64_t grid) {
  if (grid > 0x7fffffffull) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "grid too large; lower chunk_bytes");
}
// One kernel launch, timed in `slot` where a profiler is given.  rtc.fn set: the kernel is a module function compiled at run time
// (rtc.cpp) and `fn` is not used.
template <typename K, typename A>
static inline void launch(Profiler* prof, int slot, K fn, uint64_t grid, unsigned threads, size_t smem, hipStream_t stream, const A& args,
                          RtcKernel rtc = RtcKernel()) {
  check_grid(grid);
  PROF_BEGIN(prof, slot);
#ifndef FOURIER_EMU
  if (rtc.fn) {
    void* params[] = {(void*)&args};
    HIP_CHECK(hipModuleLaunchKernel((hipFunction_t)rtc.fn, (unsigned)grid, 1, 1, threads, 1, 1, (unsigned)smem, stream, params, nullptr));
  } else
#endif
  {
    (void)rtc;
    FOURIER_LAUNCH(fn, grid, threads, smem, stream, args);
  }
  PROF_END(prof);
}

}  // namespace fourier_hip
