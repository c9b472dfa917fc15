// frame_plan_common.h -- the host pieces the frame handles share (StftPlan, MdctPlan, SpectrogramPlan): the switch between a composed and
// a fused forward route, the row base of a launch over the flat frame index, and the chunk walk of an overlap-add inverse.
#pragma once
#include "handle_common.h"

namespace fourier_hip {

// The choice between the composed route and the fused one-launch route of a frame handle.  `have`: the fused kernel exists for this plan;
// `on`: it is the route of the next call.
struct FusionSwitch {
  bool have = false, on = false;
  // at create: on where the kernel exists and the development switch `env_name` (experiments library and emulator build) says so, or,
  // without it, where the handle's measurements made it the default
  void init(bool have_kernel, const char* env_name, bool measured_default) {
    const char* e = dev_env(env_name);
    have = have_kernel;
    on = have && (e ? atoi(e) != 0 : measured_default);
  }
  // option "fusion" = 0: the composed route, 1: the fused one wherever its kernel exists; false: not this option or not such a value
  bool set(const std::string& key, long long v) {
    if (key != "fusion" || (v != 0 && v != 1)) return false;
    on = v == 1 && have;
    return true;
  }
};

// A forward launch over frames g0 ... g0 + ng - 1 of the flat frame index of rows of `length` reals at `in`, `fr` frames a row: the
// block's row base, the first frame within that row, the count (StftArgs, MdctArgs)
template <typename Block, typename T> static inline void frame_launch_at(Block& a, const T* in, size_t length, size_t fr, size_t g0, size_t ng) {
  const size_t row0 = g0 / fr;
  a.in = in + row0 * length;
  a.first = (uint32_t)(g0 - row0 * fr);
  a.total = ng;
}

// The framing an overlap-add inverse walks: a frame covers `span` samples of the padded row, frame f starts at f * hop, the row at `pad`.
struct FrameOverlap {
  size_t span, hop, pad;
  size_t cover() const { return (span + hop - 1) / hop; }  // the most frames that cover one sample
};
// The chunks of an inverse call of `batch` rows of `fr` frames under a scratch of `fit` frames: rows_per whole rows where a row's frames
// fit, else ranges of output samples of one row over nfr frames.  A range needs every frame that covers one sample, so the scratch
// never holds fewer than cover() frames, whatever the bound says.
struct FrameInverseChunks {
  size_t rows_per, nfr;
  size_t frames() const { return rows_per * nfr; }  // what the scratch holds
};
static inline FrameInverseChunks frame_inverse_chunks(const FrameOverlap& o, size_t fr, size_t batch, size_t fit) {
  if (fit >= fr) return {std::min(batch, fit / fr), fr};
  return {1, std::min(fr, std::max(fit, o.cover()))};
}
// ola(b0, nb, t0, span, f_lo, nfr) for every chunk in order: nb rows from b0 on, their samples t0 ... t0 + span - 1 from the frames
// f_lo ... f_lo + nfr - 1 of each.  Ranges start at the first frame that covers their first sample; the frames two neighbouring ranges
// both need are transformed twice.
template <typename Ola>
static inline void frame_inverse_walk(const FrameOverlap& o, const FrameInverseChunks& c, size_t fr, size_t batch, size_t length, Ola&& ola) {
  if (c.nfr == fr) {  // whole rows
    for_chunks(batch, c.rows_per, [&](size_t b0, size_t nb) { ola(b0, nb, 0, length, 0, fr); });
    return;
  }
  for (size_t b = 0; b < batch; ++b)
    for (size_t t0 = 0; t0 < length;) {
      const size_t u0 = t0 + o.pad;
      const size_t f_lo = std::min(u0 >= o.span ? (u0 - o.span) / o.hop + 1 : 0, fr - 1);
      const size_t nfr = std::min(c.nfr, fr - f_lo);
      const size_t t1 = f_lo + nfr >= fr ? length : std::min(length, (f_lo + nfr) * o.hop - o.pad);
      ola(b, 1, t0, t1 - t0, f_lo, nfr);
      t0 = t1;
    }
}

}  // namespace fourier_hip
