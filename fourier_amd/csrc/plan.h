// plan.h -- the plan behind a handle: create_fft_f32/f64 (fourier/src/lib.rs:31-60) one level up -- Stockham where the length
// factors, else Bluestein (bluesteins.rs) -- with chunking, plan-owned buffers, the host-buffer paths and the error model.
#pragma once
#include "engine_pow2.h"
#include "engine_mixed.h"
#include "engine_generic.h"
#include "engine_tiled.h"
#include "handle_common.h"

namespace fourier_hip {

// ---------------------------------------------------------------------------------------------
// host f64 radix-2 FFT, used only at plan time for the Bluestein w table (bluesteins.rs:46-47)
static inline void host_fft(std::vector<double>& re, std::vector<double>& im) {
  const size_t m = re.size();
  for (size_t i = 1, j = 0; i < m; ++i) {
    size_t bit = m >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) { std::swap(re[i], re[j]); std::swap(im[i], im[j]); }
  }
  std::vector<double> wr(m / 2 ? m / 2 : 1), wi(m / 2 ? m / 2 : 1);
  for (size_t k = 0; k < m / 2; ++k) unit_root(k, m, wr[k], wi[k]);
  for (size_t len = 2; len <= m; len <<= 1) {
    const size_t half = len / 2, step = m / len;
    for (size_t i = 0; i < m; i += len)
      for (size_t k = 0; k < half; ++k) {
        const double ur = wr[k * step], ui = wi[k * step];
        const double xr = re[i + k + half] * ur - im[i + k + half] * ui;
        const double xi = re[i + k + half] * ui + im[i + k + half] * ur;
        re[i + k + half] = re[i + k] - xr; im[i + k + half] = im[i + k] - xi;
        re[i + k] += xr; im[i + k] += xi;
      }
  }
}

// ... and for any length whose prime factors are small (Bluestein on a smooth M): one Stockham pass per prime factor,
// out[j + s*(p*i + k)] = W_cur^{i*k} sum_r W_p^{r*k} in[j + s*(i + (cur/p)*r)]   (mod.rs:203-284 with plain O(p^2) butterflies)
static inline void host_fft_any(std::vector<double>& re, std::vector<double>& im) {
  const size_t m = re.size();
  if (is_pow2(m)) { host_fft(re, im); return; }
  std::vector<double> ore(m), oim(m);
  size_t cur = m, s = 1;
  while (cur > 1) {
    size_t p = 2;
    while (cur % p) ++p;
    if (p > 16) throw EngineError(::fourier::c::FOURIER_HIP_RUNTIME_ERROR, "host_fft_any: a prime factor above 16");  // (tile lengths: up to 7)
    const size_t mm = cur / p;
    std::vector<double> wr(p * p), wi(p * p);
    for (size_t e = 0; e < p * p; ++e) unit_root(e % p, p, wr[e], wi[e]);  // W_p^{r*k} at [r * p + k] via (r*k) % p below
    for (size_t i = 0; i < mm; ++i) {
      std::vector<double> tr(p), ti(p);
      for (size_t k = 0; k < p; ++k) unit_root(i * k, cur, tr[k], ti[k]);
      for (size_t j = 0; j < s; ++j) {
        double xr[16], xi[16];
        for (size_t r = 0; r < p; ++r) { xr[r] = re[j + s * (i + mm * r)]; xi[r] = im[j + s * (i + mm * r)]; }
        for (size_t k = 0; k < p; ++k) {
          double yr = 0, yi = 0;
          for (size_t r = 0; r < p; ++r) {
            const size_t e = (r * k) % p;
            yr += xr[r] * wr[e] - xi[r] * wi[e]; yi += xr[r] * wi[e] + xi[r] * wr[e];
          }
          ore[j + s * (p * i + k)] = yr * tr[k] - yi * ti[k]; oim[j + s * (p * i + k)] = yr * ti[k] + yi * tr[k];
        }
      }
    }
    re.swap(ore); im.swap(oim);
    s *= p; cur = mm;
  }
}

template <typename T> class AxisRoute;  // transforms along a strided axis (axis_plan.h), built on first use

// ---------------------------------------------------------------------------------------------
template <typename T> class Plan : public HandleBase {
  friend class AxisRoute<T>;

 public:
  static constexpr size_t ELEM = sizeof(cpx<T>);

  Plan(size_t n, int device) : n_(n) {
    if (n == 0) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "size 0 is invalid");
    int count = 0;
    HIP_CHECK(hipGetDeviceCount(&count));
    if (count <= 0) throw EngineError(::fourier::c::FOURIER_HIP_RUNTIME_ERROR, "no HIP device");
    if (device < 0) HIP_CHECK(hipGetDevice(&device));
    if (device >= count) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "bad device index");
    device_ = device;
    DeviceGuard g(device_);
    // the axis transforms' development switches (experiments library and emulator build only; axis_plan.h)
    axis_scratch_bytes_ = scratch_bound("FOURIER_AXIS_SCRATCH_BYTES", 0);
    if (const char* e = dev_env("FOURIER_AXIS_ROUTE")) axis_force_transpose_ = std::string(e) == "transpose";
    if (is_pow2(n)) {
      eng_.reset(new Pow2Engine<T>(n, false, true));
      // f32 2^20 = 1024 x 1024 (BASELINE configs[1]): every XCD walks its range of transforms in bands of eight adjacent tiles
      // (1 KiB of every row of eight transforms in flight per XCD instead of whole 8 KiB rows of one) -- 23.07 against 23.50 ms and
      // 23.05 against 23.70 ms per 4096 transforms on two boxes, bit-identical (profiles/r05_s2_*, r05_s3_c2_tile_walk_ab.jsonl);
      // f64, the L = 2048 plans and the Bluestein inner passes lose 0 - 8 % with it (r05_s3_*, r05_s4_*) and keep the tile order
      if (sizeof(T) == 4 && n == ((size_t)1 << 20) && !dev_env("FOURIER_NO_BAND_WALK")) nxcd_ = 8u | (4u << 8) | (8u << 12);
    } else if (tiled_before_pow2_tiles(n)) {
      // 2^a * 3^b with a >= 12 as TWO mixed-length tile passes instead of power-of-two tiles + odd passes (three or four round
      // trips).  Round 6, register tiles: 512 x 384 +25 %, 512 x 432 +26 ... 41 %, 576 x 576 +34 ... 50 %; 768 x 576 level, 768 x 768 -3 ... 5 %,
      // 1024 x 768 / 864 f32 -13 ... 17 % (profiles/r06_s40_long_tiles_ab.jsonl; the LDS tile passes of round 4 paid up to 384 x 384 only)
      tiled_.reset(new TiledMixedEngine<T>(n));
    } else if (Pow2Engine<T>::handles_mixed(n)) {
      // big-radix passes over the 2^a part (a >= 12), then a radix-3^b pass: three HBM round trips at full tile
      // efficiency beat the one-workgroup-per-CU LDS kernel where both apply (3*2^12 f32: 23 % vs 14 %)
      eng_.reset(new Pow2Engine<T>(n));
    } else if (regfft_route(n)) {
      // a length with factors 5 ... 13 that regfft_shapes.h lists in this precision: ONE launch with the transform on two or three register
      // stages (kernels_regfft.h) instead of the LDS mixed-radix kernel's round trip per small radix, two tile passes or Bluestein -- each
      // length at least 1.04 x faster than the route below it had (profiles/r06_s49 ... s51_regfft_*_ab.jsonl)
      regf_.reset(new BluRegEngine<T>(n, (uint32_t)n, true));
    } else if (MixedEngine<T>::handles(n) && try_mixed(n)) {
      // a length on the runtime-parameterised kernel takes its own kernel where the code-object cache has it (policy 2: compiles it)
      if (specialise_policy() >= 1) (void)mix_->specialise(nullptr, specialise_policy() >= 2);
      // ... and a 2^a 3^b length the register-stage kernel listed for it on request, where the library-wide default says so
      if (register_stages_default() == 1 && BluRegEngine<T>::has_direct_on_request(n)) {
        regf_.reset(new BluRegEngine<T>(n, (uint32_t)n, true, 100));
        regf_on_request_ = true;
      }
    } else if (TiledMixedEngine<T>::handles(n)) {
      tiled_.reset(new TiledMixedEngine<T>(n));  // two or three HBM round trips on column tiles of mixed length
    } else if (GenericEngine<T>::handles(n)) {
      gen_.reset(new GenericEngine<T>(n));       // what is left of 2^a*3^b, a < 12: one round trip per radix
    } else if (TiledMixedEngine<T>::handles_smooth(n) && !(n <= MixedEngine<T>::MAX_N && specialise_policy() >= 1 && specialised_route(n, specialise_policy() >= 2, nullptr))) {
      // factors 5 / 7 beyond the ahead-of-time LDS kernels: tile passes instead of Bluestein (round 5) -- unless the length fits a compute
      // unit's LDS and its own one-launch kernel is in the code-object cache (one HBM round trip instead of two)
      tiled_.reset(new TiledMixedEngine<T>(n));
    } else if (specialise_policy() >= 1 && specialised_route(n, specialise_policy() >= 2, nullptr)) {
      // prime factors up to 13 without an ahead-of-time route: the kernels of an earlier "specialise" from the on-disk cache
    } else {
      init_bluestein();
      apply_bluestein_options();
    }
    refresh_desc();
  }
  // A length the default routes send to Bluestein although its prime factors stop at 13: its own LDS kernel (<= MAX_N points) or
  // two / three column-tile passes, specialised at run time (rtc.cpp).  allow_compile = false: only where every kernel it needs is
  // in the code-object cache.  true: mix_ / tiled_ is set.
  bool specialised_route(size_t n, bool allow_compile, std::string* why) {
    std::string local;
    std::string& w = why ? *why : local;
    if (is_pow2(n) || n < 2) { w = "a power of two"; return false; }
    std::vector<uint32_t> radices;
    if (n <= MixedEngine<T>::MAX_N) {
      if (!MixedEngine<T>::factor(n, radices)) { w = "a prime factor above 13"; return false; }
      if (!allow_compile && !MixedEngine<T>::specialised_kernel_cached(n)) { w = "not in the code-object cache"; return false; }
      std::unique_ptr<MixedEngine<T>> m;
      try { m.reset(new MixedEngine<T>(n, true)); }
      catch (const EngineError& e) {
        if (e.status == ::fourier::c::FOURIER_HIP_OUT_OF_MEMORY) throw;  // as try_mixed: out of memory is not "take the next route"
        (void)hipGetLastError(); w = e.what(); return false;
      }
      if (m->specialise(&w, allow_compile) != ::fourier::c::FOURIER_HIP_OK) return false;
      mix_ = std::move(m);
      return true;
    }
    if (n <= TiledMixedEngine<T>::MAX_N && !TiledMixedEngine<T>::factorise(n, true).empty()) {
      if (!allow_compile && !TiledMixedEngine<T>::specialised_kernels_cached(n)) { w = "not in the code-object cache"; return false; }
      try { tiled_.reset(new TiledMixedEngine<T>(n, true, allow_compile)); }
      catch (const EngineError& e) {
        tiled_.reset();
        if (e.status == ::fourier::c::FOURIER_HIP_OUT_OF_MEMORY) throw;
        (void)hipGetLastError(); w = e.what(); return false;
      }
      return true;
    }
    w = "not a length whose prime factors stop at 13 with a kernel to specialise";
    return false;
  }
  // 2^a 3^b keep the LDS kernels on the reference's own schedule (bit-identical to the CPU restatement)
  static bool regfft_route(size_t n) {
    size_t p = n;
    while (p % 2 == 0) p /= 2;
    while (p % 3 == 0) p /= 3;
    return p != 1 && BluRegEngine<T>::has_direct(n);
  }
  static bool tiled_before_pow2_tiles(size_t n) {
    if (!Pow2Engine<T>::handles_mixed(n) || dev_env("FOURIER_POW2_TILES_FIRST") || !TiledMixedEngine<T>::handles(n, true)) return false;
    const std::vector<uint32_t> f = TiledMixedEngine<T>::factorise(n);
    return f.size() == 2 && f[0] <= 576 && f[1] <= 576;
  }
  // the longest LDS plans ask for the whole 160 KiB of a CU: where the runtime refuses, the next route takes the length
  bool try_mixed(size_t n) {
    try { mix_.reset(new MixedEngine<T>(n)); return true; }
    catch (const EngineError& e) {
      if (e.status == ::fourier::c::FOURIER_HIP_OUT_OF_MEMORY) throw;
      (void)hipGetLastError();
      mix_.reset();
      return false;
    }
  }
  void refresh_desc() {
    if (regf_) desc_ = "stockham " + regf_->describe();
    else if (mix_) desc_ = "stockham mixed-radix " + mix_->describe();
    else if (tiled_) desc_ = "stockham mixed tiles " + tiled_->describe();
    else if (gen_) desc_ = "stockham global-pass " + gen_->describe();
    else if (blur_) desc_ = "bluestein M=" + std::to_string(m_) + " " + blur_->describe();
    else if (blut_) desc_ = "bluestein M=" + std::to_string(m_) + " inner " + blut_->describe();
    else if (blu_) {
      // "fused": the whole chirp-z in one launch; "separate" (chirp sweeps: blu_pre, blu_post) / "no-conv": a plan that has the fused form /
      // the conv kernel with it switched off
      const bool off = (small_ok_ && !small_fused_) || (fuse_ok_ && !fused_);
      desc_ = "bluestein M=" + std::to_string(m_) + " inner " + eng_->describe() +
              (small_fused_ ? " fused" : off ? " separate" : (conv_ok_ && !conv_) ? " no-conv" : "");
    }
    else desc_ = "stockham " + eng_->describe();
    desc_ += sizeof(T) == 4 ? " f32" : " f64";
  }

  ~Plan() {
    if (legacy_stream_) {
      DeviceGuard g(device_);
      (void)hipStreamDestroy(legacy_stream_);
    }
  }

  size_t size() const { return n_; }
  int device() const { return device_; }

  // kernel "slots" in launch order, as reported by profile(): names for bench.py / rocprof matching
  std::string slot_names() const {
    std::string d;
    auto passes = [&](const char* tag, size_t count) {  // "tag0,tag1,..." appended to d
      for (size_t p = 0; p < count; ++p) d += std::string(d.empty() ? "" : ",") + tag + std::to_string(p);
    };
    if (regf_) return "registers_one_launch";
    if (mix_) return "mixed_radix";
    if (tiled_) { passes("pass", tiled_->num_passes()); return d; }
    if (gen_) { passes("pass", gen_->num_passes()); return d; }
    if (blur_) return "bluestein_one_launch";
    if (blut_) return "chirp_in_pass,conv_pass,chirp_out_pass";
    if (!blu_) { passes("pass", eng_->hbm_round_trips()); return d; }
    if (small_fused_) return "bluestein_one_launch";
    d = "blu_pre"; passes("fwd_pass", eng_->num_passes()); passes("inv_pass", eng_->num_passes()); d += ",blu_post";  // blu_pre/post stay empty when fused
    if (fused_ && conv_) {  // the last forward pass and the first inverse pass are one launch (inv_pass0 stays empty)
      const std::string from = "fwd_pass" + std::to_string(eng_->num_passes() - 1);
      d.replace(d.find(from), from.size(), "conv_pass");
    }
    return d;
  }

  double model_bytes() const {
    if (mix_ || regf_) return 2.0 * n_ * ELEM;
    if (tiled_) return 2.0 * n_ * ELEM * tiled_->num_passes();
    if (gen_) return 2.0 * n_ * ELEM * gen_->num_passes();
    if (!blu_) return 2.0 * n_ * ELEM * eng_->hbm_round_trips();
    // unfused: pre (n + table read, m write) + 2 inner FFTs + w table + post (n + table read, n write);
    // fused: the first / last inner pass read / write the n-point user array instead of an m-point sweep
    if (blut_) return (double)ELEM * (5.0 * m_ + 4.0 * n_);  // (n + n, m) + (m + m, m) + (m + n, n)
    if (small_fused_ || blur_) return (double)ELEM * 2.0 * n_;  // tables stay L2-resident
    const double chirp_reads = (chirp_compute_ ? 1.0 : 2.0) * n_;  // the n-entry chirp table: the chirp-out pass reads it, the chirp-in pass only without bluestein_chirp_compute
    if (fused_ && conv_) return (double)ELEM * (2.0 * m_ * (2.0 * eng_->num_passes() - 1.0) - 2.0 * (m_ - n_) + m_ + chirp_reads);
    // without the conv kernel the product with w is a sweep of its own over the M-point spectrum: 2 m on top of the w table
    if (fused_) return (double)ELEM * (2.0 * 2.0 * m_ * eng_->num_passes() - 2.0 * (m_ - n_) + 2.0 * m_ + m_ + chirp_reads);
    return (double)ELEM * ((2.0 * n_ + m_) + 2.0 * 2.0 * m_ * eng_->num_passes() + 2.0 * m_ + m_ + 3.0 * n_);
  }

  int set_option(const std::string& key, long long v) {
    DeviceGuard g(device_);  // bluestein_fusion may allocate tables: they must land on the plan's device
    if (key == "chunk_bytes" && v >= 0) { chunk_bytes_ = (size_t)v; return 0; }
    if (key == "scratch" && (v == 0 || v == 1)) { force_scratch_ = (v == 1); return 0; }
    if (key == "xcd_swizzle" && v >= 0 && v <= 4) { nxcd_ = v == 0 ? 1 : (8 | ((unsigned)(v - 1) << 8)); return 0; }
    // the general band walk of the tile passes (xcd_remap mode 4): v = tiles per band | transforms per group << 8 (0 = the XCD's
    // whole range) | transform-fastest << 19; v = 0 restores the default order
    if (key == "tile_walk_last" && v >= 0 && v < (1 << 21)) {  // the same encoding, for the last pass of a plain multi-pass plan alone (0 = as the others)
      const unsigned band = (unsigned)v & 0xff, group = ((unsigned)v >> 8) & 0x3ff, tf = ((unsigned)v >> 19) & 3;
      nxcd_last_ = band == 0 ? 0u : (8u | (4u << 8) | (band << 12) | (group << 20) | (tf << 30));
      return 0;
    }
    if (key == "tile_walk" && v >= 0 && v < (1 << 21)) {
      const unsigned band = (unsigned)v & 0xff, group = ((unsigned)v >> 8) & 0x3ff, tf = ((unsigned)v >> 19) & 3;  // bit 20: strided bands (A/B)
      nxcd_ = band == 0 ? 8u : (8u | (4u << 8) | (band << 12) | (group << 20) | (tf << 30));
      return 0;
    }
    // Bluestein's M: 1 (default) = the smallest product of two tile lengths where that saves a quarter of the power-of-two work array,
    // 0 = always the reference's next power of two (bluesteins.rs:110).  Rebuilds the plan's tables now; not while a transform is in flight.
    if (key == "bluestein_smooth_m" && v >= 0 && v <= 2) {  // (2: wherever a product of two tile lengths exists -- for measurements)
      if (!blu_) return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
      want_smooth_m_ = (int)v;
      apply_bluestein_options();
      return 0;
    }
    // The five Bluestein options only record the caller's request; apply_bluestein_options() derives what the plan runs from the requests
    // last set, whatever their order (include/fourier.h states the precedence).  "bluestein_fusion" = 0: the tile route has no unfused form
    // (ignored there), nor has the register route: the unfused sweeps run on the reference's power-of-two M, and 1 brings the route back.
    if (key == "bluestein_fusion" && (v == 0 || v == 1)) { want_fusion_ = (v == 1); if (blu_) apply_bluestein_options(); return 0; }
    if (key == "bluestein_conv" && (v == 0 || v == 1)) { want_conv_ = (v == 1); if (blu_) apply_bluestein_options(); return 0; }
    // (the computed chirp is built on exact exponents: under "bluestein_reference_chirp" it would disagree with the chirp-out table and w by the
    // reference's own angle error -- the request stands for when that option is switched off again, the pass keeps reading the table)
    if (key == "bluestein_chirp_compute" && (v == 0 || v == 1)) { want_chirp_compute_ = (int)v; if (blu_) apply_bluestein_options(); return 0; }
    if (key == "host_chunk_bytes" && v > 0) { host_chunk_bytes_ = (size_t)v; return 0; }
    // the two passes of a two-pass power-of-two plan software-pipelined over two internal streams with the intermediate in a small
    // ring (Pow2Engine::run_pipelined): v = transforms per chunk | ring slots << 16 | one-stream control << 24; 0 = off
    if (key == "stream_pipeline" && v >= 0 && v < (1 << 25)) {
      if (v != 0 && (blu_ || !eng_ || !eng_->can_pipeline())) return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
      pipe_chunk_ = (size_t)(v & 0xffff); pipe_slots_ = (size_t)((v >> 16) & 0xff); pipe_one_stream_ = ((v >> 24) & 1) != 0;
      if (pipe_chunk_ && pipe_slots_ < 2) pipe_slots_ = 2;
      return 0;
    }
    // the reference's unreduced chirp angle (build_chirp_tables): rebuilds the x and w tables now; the chirp-in pass then READS the
    // table (its computed chirp is built on exact exponents).  Not while a transform is in flight on this handle.
    if (key == "bluestein_reference_chirp" && (v == 0 || v == 1)) {
      if (!blu_) return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
      want_reference_chirp_ = (v == 1);
      apply_bluestein_options();
      return 0;
    }
    // "register_stages" = 1: a 2^a 3^b length that runs the LDS kernel on the reference's own schedule (bit-identical to the CPU restatement)
    // takes the register-stage kernel regfft_shapes.h lists for it instead (kernels_regfft.h: within the tolerance, not the bits; 1.04 ... 1.6 x);
    // 0 brings the default back.  UNSUPPORTED where no such kernel is listed; OK unchanged on a plan that runs register stages by default.
    if (key == "register_stages" && (v == 0 || v == 1)) {
      if (v == 1) {
        if (regf_) return ::fourier::c::FOURIER_HIP_OK;
        if (!mix_ || !BluRegEngine<T>::has_direct_on_request(n_)) return ::fourier::c::FOURIER_HIP_UNSUPPORTED;
        try { regf_.reset(new BluRegEngine<T>(n_, (uint32_t)n_, true, 100)); } catch (const EngineError& e) { return e.status; }
        regf_on_request_ = true;
      } else if (regf_on_request_) {
        regf_.reset();
        regf_on_request_ = false;
      }
      refresh_desc();
      return ::fourier::c::FOURIER_HIP_OK;
    }
    // "specialise" = 1: compile this length's own LDS mixed-radix kernel with hipRTC (about a second, now) and run it from the
    // next call on -- for a length whose prime factors stop at 13, that fits a compute unit's LDS and has no ahead-of-time
    // per-length kernel (it runs the runtime-parameterised kernel, or Bluestein beyond that kernel's reach).  A plan that
    // already runs a per-length kernel returns OK unchanged; UNSUPPORTED where hipRTC is not available or the length is not of
    // that family: the plan keeps its route.
    if (key == "specialise" && v == 1) {
      std::string why;
      auto report = [&](int st) {
        if (st != ::fourier::c::FOURIER_HIP_OK && getenv("FOURIER_HIP_VERBOSE")) fprintf(stderr, "libfourier: specialise(%zu): %s\n", n_, why.c_str());
        return st;
      };
      if (regf_) return ::fourier::c::FOURIER_HIP_OK;  // already on a kernel of its own
      if (mix_) { const int st = mix_->specialise(&why); refresh_desc(); return report(st); }
      if (blu_) {  // exec() takes the new route from here on; the Bluestein tables stay allocated but unused
        if (specialised_route(n_, true, &why)) { refresh_desc(); return ::fourier::c::FOURIER_HIP_OK; }
        return report(::fourier::c::FOURIER_HIP_UNSUPPORTED);
      }
      if (tiled_) {
        // ahead-of-time tile passes: where the length fits a compute unit's LDS its own one-launch kernel replaces them (one HBM round trip
        // instead of two); otherwise there is nothing to specialise and the plan stays as it is (OK)
        if (n_ <= MixedEngine<T>::MAX_N && !tiled_->specialised()) {
          std::unique_ptr<TiledMixedEngine<T>> keep = std::move(tiled_);
          if (specialised_route(n_, true, &why) && mix_) { refresh_desc(); return ::fourier::c::FOURIER_HIP_OK; }
          tiled_ = std::move(keep);
          mix_.reset();
          return report(::fourier::c::FOURIER_HIP_UNSUPPORTED);
        }
        return ::fourier::c::FOURIER_HIP_OK;
      }
      why = "not a length whose prime factors stop at 13 with a kernel to specialise";
      return report(::fourier::c::FOURIER_HIP_UNSUPPORTED);
    }
    // LAST pass as persistent workgroups that prefetch their next tile (fft_last_prefetch_kernel; experiments library only,
    // measured slower): 1 where the kernel exists, INVALID_ARGUMENT where it does not
    if (key == "last_pass_prefetch" && (v == 0 || v == 1) && eng_) {
      if (v == 1 && !eng_->has_prefetch_last() && !(eng_inv_ && eng_inv_->has_prefetch_last())) return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
      eng_->set_prefetch_last(v == 1);
      if (eng_inv_) eng_inv_->set_prefetch_last(v == 1);
      return 0;
    }
    // the passes as their load / store skeleton (experiments library only; timing tool of bench.py's streaming ceiling, wrong results)
    if (key == "skeleton" && (v == 0 || v == 1) && eng_ && !blu_) {
      if (v == 1 && !eng_->has_skeleton()) return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
      eng_->set_skeleton(v == 1);
      return 0;
    }
    // both passes in one launch with the intermediate in the XCD's L2 (2^16..2^18 f32, 2^15..2^17 f64); 0 where unavailable
    if (key == "l2_fused" && (v == 0 || v == 1)) {
      if (blu_ || !eng_ || (v == 1 && !eng_->has_l2fused())) return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
      eng_->set_l2fused(v == 1);
      refresh_desc();
      return 0;
    }
    if (key == "l2_fused_depth" && !blu_ && eng_ && eng_->set_l2fused_depth((unsigned)v)) return 0;
    if (key == "l2_fused_grid" && !blu_ && eng_ && eng_->has_l2fused() && v > 0) { eng_->set_l2fused_grid((unsigned)v); return 0; }
    return ::fourier::c::FOURIER_HIP_INVALID_ARGUMENT;
  }

  // Chunk size for a call of `batch` transforms and the plan-owned device buffers it needs (scratch of the in-place /
  // three-pass plans, the Bluestein work array).  exec() calls this on every call -- it allocates only when the batch
  // is larger than anything seen before -- and fourier_hip_reserve_* calls it ahead of time, so that a later
  // transform_batch of at most that batch never allocates (hipMalloc / hipFree synchronise the device) and can be
  // captured into a HIP graph.  Returns the number of transforms per chunk.
  // `profiled`: the call is a profiled one (exec()'s prof), which a pipelined plan runs on the ordinary route when it is out of place.
  size_t prepare(size_t batch, bool in_place, bool profiled = false) const {
    if (mix_ || regf_ || batch == 0) return batch;
    if (tiled_) {  // one scratch of a chunk for in-place calls and three-pass plans
      size_t chunk = first_chunk(batch, n_, 8.0);
      if (tiled_->needs_scratch(in_place) || force_scratch_) reserve(chunk, [&](size_t c) { scratch_.ensure(c * n_ * ELEM); });
      return chunk;
    }
    if (gen_) {  // two scratch halves of one chunk each
      size_t chunk = first_chunk(batch, n_, 256.0);
      reserve(chunk, [&](size_t c) { scratch_.ensure(2 * c * n_ * ELEM); });
      return chunk;
    }
    size_t chunk = first_chunk(batch, blu_ ? m_ : n_, 16.0);
    if (!blu_) {
      // (only where exec() pipelines: every other call takes the ordinary route below and needs its scratch, within "chunk_bytes")
      if (pipelines(in_place, profiled)) { eng_->reserve_pipeline(std::min(pipe_chunk_, batch), pipe_slots_); return batch; }
      if (eng_->l2fused_enabled()) { eng_->reserve_l2fused(chunk); return chunk; }
      if (needs_plan_scratch(in_place)) reserve(chunk, [&](size_t c) { scratch_.ensure(c * n_ * ELEM); });
      return chunk;
    }
    if (small_fused_ || blur_) return batch;  // whole chirp-z in one launch: no work array
    reserve(chunk, [&](size_t c) {
      work_.ensure(c * m_ * ELEM);
      if (blut_ || eng_->needs_scratch(true) || fused_) scratch_.ensure(c * m_ * ELEM);
    });
    return chunk;
  }
  // the chunk a call starts from: `batch` transforms of `points` elements within option "chunk_bytes", halved until a launch of one
  // workgroup per `per_group` elements keeps its grid below 2^31 workgroups
  size_t first_chunk(size_t batch, size_t points, double per_group) const {
    size_t chunk = chunk_bytes_ ? chunk_rows(batch, chunk_bytes_, points * ELEM) : batch;
    while (chunk > 1 && (double)chunk * (double)points / per_group > 2.0e9) chunk = (chunk + 1) / 2;
    return chunk;
  }
  // The plan's scratch (and the Bluestein work array) hold one chunk.  If the device cannot give that much -- an
  // in-place call on a batch that fills most of the HBM -- fall back to smaller chunks instead of failing: chunks
  // run back to back on the stream and the results are the same.
  template <typename F> static void reserve(size_t& chunk, F&& alloc) {
    for (;;) {
      try { alloc(chunk); return; }
      catch (const EngineError& e) {
        if (e.status != ::fourier::c::FOURIER_HIP_OUT_OF_MEMORY || chunk <= 1) throw;
        (void)hipGetLastError();  // the allocation failure is handled here
        chunk = (chunk + 1) / 2;
      }
    }
  }
  void reserve_for(size_t batch, bool in_place) const {
    DeviceGuard g(device_);
    (void)prepare(batch, in_place);
    if (pipe_chunk_ && !in_place) (void)prepare(batch, in_place, true);  // ... and the profiled call of a pipelined plan, which does not pipeline
  }
  // a plan with option "stream_pipeline" pipelines every call but the profiled out-of-place one, which times the kernels one by one on
  // the caller's stream; prepare() and exec() both decide here
  bool pipelines(bool in_place, bool profiled) const { return pipe_chunk_ != 0 && (!profiled || in_place); }
  // whether the ordinary route of a plain power-of-two plan sends a pass through the plan's scratch: prepare() sizes it, exec() checks it
  bool needs_plan_scratch(bool in_place) const {
    return !eng_->l2fused_enabled() && (eng_->needs_scratch(in_place) || (force_scratch_ && eng_->num_passes() >= 2));
  }

  // Batched transform on device memory (the operator behind Fft::transform / transform_in_place).
  void exec(const void* d_in, void* d_out, size_t batch, int code, hipStream_t stream, Profiler* prof = nullptr) const {
    if (!d_in || !d_out) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "null buffer");
    if (code < 0 || code > 4) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "unknown transform code");
    if (batch == 0) return;
    DeviceGuard g(device_);
    const bool inverse = !is_forward(code);
    const double scale = code_scale<T>(code, (T)n_);
    const cpx<T>* in = (const cpx<T>*)d_in;
    cpx<T>* out = (cpx<T>*)d_out;
    const bool in_place = (d_in == d_out);
    if (regf_) {  // the whole transform in registers: one launch, in place allowed (a workgroup reads its transforms first)
      regf_->run(in, out, batch, nullptr, nullptr, inverse, scale, stream, prof);
      return;
    }
    if (mix_) {  // every pass stays in LDS: one launch, in place allowed (a workgroup reads its transforms first)
      const bool scaled = code == ::fourier::c::FOURIER_TRANSFORM_IFFT || code == ::fourier::c::FOURIER_TRANSFORM_SQRT_SCALED_FFT ||
                          code == ::fourier::c::FOURIER_TRANSFORM_SQRT_SCALED_IFFT;  // mod.rs:381-385
      mix_->run(in, out, batch, !inverse, scaled,
                scale, stream, prof);
      return;
    }
    const size_t chunk = prepare(batch, in_place, prof != nullptr);

    cpx<T>* const scratch = (cpx<T>*)scratch_.p;
    if (tiled_) {
      for_chunks(batch, chunk, [&](size_t b0, size_t nb) { tiled_->run(in + b0 * n_, out + b0 * n_, scratch, nb, inverse, scale, stream, prof); });
      return;
    }
    if (gen_) {
      for_chunks(batch, chunk, [&](size_t b0, size_t nb) { gen_->run(in + b0 * n_, out + b0 * n_, scratch, nb, inverse, scale, stream, prof); });
      return;
    }
    if (!blu_) {
      if (pipelines(in_place, prof != nullptr)) {
        eng_->run_pipelined(in, out, batch, pipe_chunk_, pipe_slots_, inverse, scale, stream, nxcd_, nxcd_last_, pipe_one_stream_);
        return;
      }
      if (!scratch && needs_plan_scratch(in_place))  // prepare() sized it; never a pass through a null pointer
        throw EngineError(::fourier::c::FOURIER_HIP_RUNTIME_ERROR, "the plan's scratch buffer is missing");
      for_chunks(batch, chunk, [&](size_t b0, size_t nb) {
        eng_->run(in + b0 * n_, out + b0 * n_, scratch, nb, inverse, scale, nullptr, force_scratch_, stream, prof, 0, nxcd_, BluIO(), nxcd_last_);
      });
      return;
    }
    // Bluestein (bluesteins.rs:215-259): work = x.in (zero padded) ; FFT_M ; .w ; IFFT_M ; out = work.x.scale
    if (small_fused_) {  // M <= 2^15: the whole chirp-z in one launch, no work array
      eng_->run_bluestein_small(in, out, batch, xtab_.p, wtab_.p, n_, inverse, scale, stream, prof, nxcd_);
      return;
    }
    if (blur_) {  // a short transform on a smooth M = R1 x R2: one launch, both transforms in registers (kernels_chirpz.h)
      blur_->run(in, out, batch, xtab_.p, wtab_.p, inverse, scale, stream, prof);
      return;
    }
    cpx<T>* work = (cpx<T>*)work_.p;
    if (blut_) {  // smooth M: three sweeps on register tiles (kernels_regtile.h)
      for_chunks(batch, chunk, [&](size_t b0, size_t nb) {
        blut_->run(in + b0 * n_, out + b0 * n_, work, scratch, nb, xtab_.p, wtab_.p, inverse, scale, stream, prof);
      });
      return;
    }
    const int np = (int)eng_->num_passes();
    for_chunks(batch, chunk, [&](size_t b0, size_t nb) {
      const cpx<T>* x = in + b0 * n_;
      cpx<T>* y = out + b0 * n_;
      if (fused_ && conv_) {
        // three sweeps instead of four: first forward pass (chirp-in fused), the conv kernel (last forward pass,
        // (.) w, first inverse pass), last inverse pass (chirp-out fused); intermediates ping-pong work/scratch
        three_sweeps(x, y, nb, work, scratch, blu_in(inverse), blu_out(inverse), wtab_.p, 0, 0, nxcd_, nxcd_, scale, stream, prof);
      } else if (fused_) {
        // chirp multiply + zero pad fused into the forward inner FFT's first pass, chirp * scale fused into
        // the inverse inner FFT's last pass: no separate sweeps over the M-point work array
        eng_->run(x, work, scratch, nb, false, 1.0, (const cpx<T>*)wtab_.p, false, stream, prof, 1, nxcd_, blu_in(inverse));
        eng_->run(work, y, scratch, nb, true, scale, nullptr, false, stream, prof, 1 + np, nxcd_, blu_out(inverse));
      } else {
        BluArgs pre{x, work, xtab_.p, (uint64_t)n_, (uint64_t)m_, (uint64_t)nb, inverse, 1.0};
        launch(prof, 0, get_blu_kernel(Real<T>{}, 0), elementwise_grid(nb * m_), 256, 0, stream, pre);
        eng_->run(work, work, scratch, nb, false, 1.0, (const cpx<T>*)wtab_.p, false, stream, prof, 1, nxcd_);
        eng_->run(work, work, scratch, nb, true, 1.0, nullptr, false, stream, prof, 1 + np, nxcd_);
        BluArgs post{work, y, xtab_.p, (uint64_t)n_, (uint64_t)m_, (uint64_t)nb, inverse, scale};
        launch(prof, 1 + 2 * np, get_blu_kernel(Real<T>{}, 1), elementwise_grid(nb * n_), 256, 0, stream, post);
      }
    });
  }

  // ---- the hook of the convolution handle (ConvPlan, conv_plan.h); exec() is not affected.  enable_conv_bank sets up and returns the
  // route this plan has for a convolution with a filter bank: CONV_NONE; CONV_ONE_LAUNCH (a one-launch two-level plan, 2^11 ... 2^15: load,
  // FFT, product, inverse FFT, store in conv_small_kernel); CONV_PASSES (a power-of-two plan of two or more tile passes whose mirror image
  // exists: forward passes 0 ... np-2, fft_conv_kernel with the bank -- last forward pass, the product with the row's filter, first inverse
  // pass --, inverse passes 1 ... np-1: the Bluestein sequence below without the chirp I/O).  exec_conv runs `batch` rows; d_in may be
  // d_out; CONV_PASSES needs two caller-owned work arrays of batch * n elements each.  bank: `filters` tables of n entries in spectrum
  // order (the inverse's 1/n folded in), row b of the call uses table (first + b) mod filters.  The caller bounds `batch` (ConvPlan's
  // scratch): the option "chunk_bytes" of exec() does not apply here.
  enum { CONV_NONE = 0, CONV_ONE_LAUNCH = 1, CONV_PASSES = 2 };
  int enable_conv_bank() {
    if (conv_route_ != CONV_NONE || blu_ || !eng_) return conv_route_;
    DeviceGuard g(device_);
    if (eng_->enable_conv_small()) return conv_route_ = CONV_ONE_LAUNCH;
    if (!eng_->can_conv()) return CONV_NONE;
    const size_t np = eng_->num_passes();
    std::unique_ptr<Pow2Engine<T>> inv;
    if (!eng_->palindromic()) {
      inv.reset(new Pow2Engine<T>(n_, true));
      if (inv->num_passes() != np) return CONV_NONE;
      for (size_t p = 0; p < np; ++p)
        if (inv->pass_len(p) != eng_->pass_len(np - 1 - p)) return CONV_NONE;  // (a plan that is not built from the default lengths)
    }
    eng_->enable_conv_bank();
    if (!eng_->has_conv_bank()) return CONV_NONE;
    eng_inv_ = std::move(inv);
    return conv_route_ = CONV_PASSES;
  }
  bool exec_conv(const void* d_in, void* d_out, size_t batch, const void* bank, size_t filters, size_t first, void* work_a, void* work_b,
                 hipStream_t stream) const {
    if (conv_route_ == CONV_NONE) return false;
    if (batch == 0) return true;
    DeviceGuard g(device_);
    if (conv_route_ == CONV_ONE_LAUNCH) {
      eng_->run_conv_small((const cpx<T>*)d_in, (cpx<T>*)d_out, batch, bank, (uint32_t)filters, (uint32_t)(first % filters), stream, nxcd_);
      return true;
    }
    // (the conv kernel in the tile order every Bluestein plan runs it in, 8 XCDs and launch_conv's slicing -- not this plan's nxcd_, which at
    // f32 2^20 is the band walk of the plain passes, an order the conv kernel has never been measured or tested in)
    three_sweeps((const cpx<T>*)d_in, (cpx<T>*)d_out, batch, (cpx<T>*)work_a, (cpx<T>*)work_b, BluIO(), BluIO(), bank, (uint32_t)filters,
                 (uint32_t)(first % filters), 8, nxcd_last_ ? nxcd_last_ : nxcd_, 1.0, stream, nullptr);
    return true;
  }

  // ---- the hook of the linear-convolution handle (LinearConvPlan, lconv_plan.h); exec() is not affected.  A one-launch two-level plan
  // (2^11 ... 2^15, f64 ... 2^14) runs the overlap-save blocks of `rows` rows in one launch of lconv_small_kernel; the bank is laid out as
  // exec_conv's, row b of the call uses table (first + b) mod filters.  The caller keeps rows * g.wpr below 2^31.
  bool enable_lconv(bool real_data) {
    if (blu_ || !eng_) return false;
    DeviceGuard g(device_);
    return eng_->enable_lconv_small(real_data);
  }
  void exec_lconv(const void* d_in, void* d_out, size_t rows, const void* bank, size_t filters, size_t first, bool real_data,
                  const LconvGeom& geo, hipStream_t stream) const {
    DeviceGuard g(device_);
    eng_->run_lconv_small(d_in, d_out, rows, bank, (uint32_t)filters, (uint32_t)(first % filters), real_data, geo, stream, nxcd_);
  }

  // ---- the hook of the analytic-signal handle (HilbertPlan, hilbert_plan.h); exec() is not affected.  A one-launch two-level plan
  // (2^11 ... 2^15, f64 ... 2^14) runs `batch` rows of n reals in one launch of hilbert_small_kernel: rows of n complex values out, or
  // (envelope) rows of n reals, which may be the input.  The caller keeps `batch` below 2^31.
  bool enable_hilbert() {
    if (blu_ || !eng_) return false;
    DeviceGuard g(device_);
    return eng_->enable_hilbert_small();
  }
  void exec_hilbert(const void* d_in, void* d_out, size_t batch, bool envelope, hipStream_t stream) const {
    DeviceGuard g(device_);
    eng_->run_hilbert_small(d_in, d_out, batch, envelope, stream, nxcd_);
  }

  // ---- the hook of the cross-correlation handle (XcorrPlan, xcorr_plan.h); exec() is not affected.  A one-launch two-level plan of L
  // points (2^11 ... 2^15, f64 ... 2^14) runs `batch` pairs of rows of n <= L reals in one launch of xcorr_small_kernel: rows of `lags`
  // reals out, apart from both inputs; `first` is lag_first mod L.  The caller keeps `batch` below 2^31.  enable_xcorr returns the
  // weightings that have a kernel: bit 0 none, bit 1 PHAT.
  int enable_xcorr() {
    if (blu_ || !eng_) return 0;
    DeviceGuard g(device_);
    return eng_->enable_xcorr_small();
  }
  void exec_xcorr(const void* d_x, const void* d_y, void* d_out, size_t batch, size_t n, size_t first, size_t lags, bool phat,
                  hipStream_t stream) const {
    DeviceGuard g(device_);
    eng_->run_xcorr_small(d_x, d_y, d_out, batch, (uint32_t)n, (uint32_t)first, (uint32_t)lags, phat, stream, nxcd_);
  }

  // ---- the hook of the delay handle (DelayPlan, delay_plan.h); exec() is not affected.  A one-launch two-level plan of L points
  // (2^11 ... 2^15, f64 ... 2^14) runs `batch` rows of n <= L reals in one launch of delay_small_kernel: row b delayed by d_delays[b]
  // samples, circularly over L, and scaled by d_weights[b] (null: 1); rows of n reals out, d_out == d_in allowed.  The caller keeps
  // `batch` below 2^31.
  bool enable_delay() {
    if (blu_ || !eng_) return false;
    DeviceGuard g(device_);
    return eng_->enable_delay_small();
  }
  void exec_delay(const void* d_in, const void* d_delays, const void* d_weights, void* d_out, size_t batch, size_t n,
                  hipStream_t stream) const {
    DeviceGuard g(device_);
    eng_->run_delay_small(d_in, d_delays, d_weights, d_out, batch, (uint32_t)n, stream, nxcd_);
  }

  // ---- the hook of the cepstrum handle (CepstrumPlan, cepstrum_plan.h); exec() is not affected.  A one-launch two-level plan of L
  // points (2^11 ... 2^15, f64 ... 2^14) runs `batch` rows of n <= L reals in one launch of cepstrum_small_kernel: mode 0 the real
  // cepstrum, mode 1 the minimum-phase row; rows of m <= L reals out, d_out == d_in allowed where m == n.  fl: CepstrumFloor, kernel_args.h.
  // The caller keeps `batch` below 2^31.
  bool enable_cepstrum(int mode) {
    if (blu_ || !eng_) return false;
    DeviceGuard g(device_);
    return eng_->enable_cepstrum_small(mode);
  }
  void exec_cepstrum(const void* d_in, void* d_out, size_t batch, size_t n, size_t m, int mode, double log_mult, const CepstrumFloor& fl,
                     hipStream_t stream) const {
    DeviceGuard g(device_);
    eng_->run_cepstrum_small(d_in, d_out, batch, (uint32_t)n, (uint32_t)m, mode, log_mult, fl, stream, nxcd_);
  }

  // ---- the hook of the chirp-z handle (CztPlan, czt_plan.h); exec() is not affected.  A one-launch two-level plan of L points
  // (2^11 ... 2^15, f64 ... 2^14) runs `batch` rows of n values (complex, or reals) in one launch of czt_small_kernel: rows of m complex
  // values out, apart from the input, n + m - 1 <= L.  The tables are the caller's: A (n entries), B (m entries), H (L entries, spectrum
  // order, 1 / L folded in).  The caller keeps `batch` below 2^31.
  bool enable_czt(bool real_input) {
    if (blu_ || !eng_) return false;
    DeviceGuard g(device_);
    return eng_->enable_czt_small(real_input);
  }
  void exec_czt(const void* d_in, void* d_out, size_t batch, size_t n, size_t m, const void* atab, const void* btab, const void* htab,
                bool real_input, hipStream_t stream) const {
    DeviceGuard g(device_);
    eng_->run_czt_small(d_in, d_out, batch, (uint32_t)n, (uint32_t)m, atab, btab, htab, real_input, stream, nxcd_);
  }

  // ---- the hooks of the frame handles (StftPlan, MdctPlan, SpectrogramPlan, CsdPlan, PfbPlan), selected by the kernels' argument block
  // (StftArgs, MdctArgs, SpectrogramArgs, CsdArgs, PfbArgs); exec() is not affected.  A plan of h points that is one whole-row pass runs the
  // frames of n = 2h samples (PfbArgs: of P = 2h real or P = h complex channels, fn[1] / fn[0]) in one launch of the family's rows kernel
  // (kernels_frames.h): fn[which] on `groups` workgroups of frame_cols() frames, 0: those that cover the `total` frames of the block.
  template <typename Args> bool enable_frames() {
    if (blu_ || !eng_) return false;
    DeviceGuard g(device_);
    return eng_->template enable_frame_rows<Args>();
  }
  template <typename Args> int frame_cols() const { return eng_->template frame_rows_cols<Args>(); }
  template <typename Args> void exec_frames(const Args& a, hipStream_t stream, int which = 0, uint64_t groups = 0) const {
    DeviceGuard g(device_);
    eng_->run_frame_rows(a, which, groups, stream);
  }

  // Wait for everything queued on `stream` of the plan's device (the blocking half of a stream-ordered batched call).
  void synchronize(hipStream_t stream) const {
    DeviceGuard g(device_);
    HIP_CHECK(hipStreamSynchronize(stream));
  }

  // Legacy host-buffer path (fourier-ffi/src/lib.rs:31-59): H2D, one transform, D2H, synchronous.
  void exec_host(const void* h_in, void* h_out, int code) const {
    if (!h_in || !h_out) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "null buffer");
    if (code < 0 || code > 4) return;  // unknown code: silent no-op (lib.rs:10)
    DeviceGuard g(device_);
    const size_t bytes = n_ * ELEM;
    pinned_.ensure(bytes);
    // the plan's own non-blocking stream: a legacy call never serialises against the NULL stream or any other
    // stream of the process (a relinked, threaded C/C++ program keeps its concurrency; one thread per handle)
    if (!legacy_stream_) HIP_CHECK(hipStreamCreateWithFlags(&legacy_stream_, hipStreamNonBlocking));
    const hipStream_t st = legacy_stream_;
    {
      const CopyJob in_job{pinned_.h, h_in, bytes};
      parallel_copy(&in_job, 1);  // one thread below 4 MiB, a few above (a 2^20-point transform is 8-16 MiB)
    }
    if (bytes <= ZERO_COPY_MAX) {
      // small transforms are latency-bound: the kernels read and write the mapped host buffer directly over
      // PCIe (every plan reads its input once and writes its output once) -- one launch chain, one sync
      exec(pinned_.d, pinned_.d, 1, code, st);
    } else {
      hostio_.ensure(bytes);
      HIP_CHECK(hipMemcpyAsync(hostio_.p, pinned_.h, bytes, hipMemcpyHostToDevice, st));
      exec(hostio_.p, hostio_.p, 1, code, st);
      HIP_CHECK(hipMemcpyAsync(pinned_.h, hostio_.p, bytes, hipMemcpyDeviceToHost, st));
    }
    // (polling hipStreamQuery before this blocking wait was measured: 27.0-27.4 vs 26.7 us per N = 4096 call -- the runtime's
    // own wait already spins; profiles/r03_s19_c1_spin_poll_ab.jsonl)
    HIP_CHECK(hipStreamSynchronize(st));
    const CopyJob out_job{h_out, pinned_.h, bytes};
    parallel_copy(&out_job, 1);
  }
  static constexpr size_t ZERO_COPY_MAX = 256 * 1024;

  // Batched transform on HOST memory (extension; the reference's callers hold host slices, fft.rs:48-61): `batch`
  // contiguous transforms are streamed through the device in chunks.  NSLOTS slots of pinned staging + device buffer;
  // the H2D copy of chunk i+1, the kernels of chunk i and the D2H copy of chunk i-1 run on three streams, and
  // the calling thread (helped by a few copy threads) moves pageable user memory in and out of the staging
  // buffers meanwhile.  Synchronous: returns when `h_out` is complete.  h_in == h_out is allowed.
  void exec_host_batch(const void* h_in, void* h_out, size_t batch, int code) const {
    if (!h_in || !h_out) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "null buffer");
    if (code < 0 || code > 4) throw EngineError(::fourier::c::FOURIER_HIP_INVALID_ARGUMENT, "unknown transform code");
    if (batch == 0) return;
    DeviceGuard g(device_);
    const size_t per = n_ * ELEM;
    const size_t chunk = chunk_rows(batch, host_chunk_bytes_, per);
    const size_t nchunks = (batch + chunk - 1) / chunk;
    pipe_.ensure(chunk * per);
    const char* src = (const char*)h_in;
    char* dst = (char*)h_out;
    auto chunk_bytes = [&](size_t i) { return std::min(chunk, batch - i * chunk) * per; };
    for (size_t i = 0; i < nchunks + NSLOTS; ++i) {
      const int s = (int)(i % NSLOTS);
      CopyJob jobs[2];
      int njobs = 0;
      if (i >= NSLOTS) {  // chunk i-NSLOTS used this slot: its result is in the staging buffer once its D2H has finished
        HIP_CHECK(hipEventSynchronize(pipe_.d2h_done[s]));
        jobs[njobs++] = {dst + (i - NSLOTS) * chunk * per, pipe_.pin_out[s].h, chunk_bytes(i - NSLOTS)};
      }
      if (i < nchunks) jobs[njobs++] = {pipe_.pin_in[s].h, src + i * chunk * per, chunk_bytes(i)};
      parallel_copy(jobs, njobs);  // result of chunk i-NSLOTS out of, input of chunk i into the staging buffers, together
      if (i < nchunks) {
        const size_t bytes = chunk_bytes(i);
        HIP_CHECK(hipMemcpyAsync(pipe_.dev[s].p, pipe_.pin_in[s].h, bytes, hipMemcpyHostToDevice, pipe_.s_h2d));
        HIP_CHECK(hipEventRecord(pipe_.h2d_done[s], pipe_.s_h2d));
        HIP_CHECK(hipStreamWaitEvent(pipe_.s_comp, pipe_.h2d_done[s], 0));
        exec(pipe_.dev[s].p, pipe_.dev[s].p, bytes / per, code, pipe_.s_comp);
        HIP_CHECK(hipEventRecord(pipe_.comp_done[s], pipe_.s_comp));
        HIP_CHECK(hipStreamWaitEvent(pipe_.s_d2h, pipe_.comp_done[s], 0));
        HIP_CHECK(hipMemcpyAsync(pipe_.pin_out[s].h, pipe_.dev[s].p, bytes, hipMemcpyDeviceToHost, pipe_.s_d2h));
        HIP_CHECK(hipEventRecord(pipe_.d2h_done[s], pipe_.s_d2h));
      }
    }
  }
  static constexpr size_t HOST_CHUNK_BYTES = (size_t)32 << 20;
  static constexpr size_t NSLOTS = 4;  // chunks in flight: copy-in, H2D, kernels, D2H + copy-out each take about one chunk time

 private:
  using BluIO = typename Pow2Engine<T>::BluIO;
  // the chirp I/O of a fused Bluestein plan's first forward pass (x . chirp, zero padded) and last inverse pass (. chirp . scale)
  BluIO blu_in(bool inverse) const {
    BluIO b;
    b.io = IO_BLU_IN; b.xtab = xtab_.p; b.n = n_; b.swap = inverse;
    if (chirp_compute_) { b.p_tab = chirp_p_.p; b.u_tab = chirp_u_.p; b.tn_lo = tn_lo_.p; b.tn_hi = tn_hi_.p; b.tn_bits = tn_bits_; }
    return b;
  }
  BluIO blu_out(bool inverse) const {
    BluIO b;
    b.io = IO_BLU_OUT; b.xtab = xtab_.p; b.n = n_; b.swap = inverse;
    return b;
  }
  // A forward transform, a product with a table in spectrum order and an inverse transform in three sweeps of memory: forward passes
  // 0 ... np-2 (the first reads `in` through `first`), launch_conv (last forward pass, (.) table, first inverse pass), inverse passes
  // 1 ... np-1 (the last writes `out` through `last`, times `scale`, in the tile order nxcd_last); intermediates ping-pong buf_a / buf_b.
  // filters != 0: `table` is a bank, row b multiplies by table (first_row + b) mod filters.  Timed in slots 1 + p, np, 1 + np + p.
  void three_sweeps(const cpx<T>* in, cpx<T>* out, size_t nb, cpx<T>* buf_a, cpx<T>* buf_b, const BluIO& first, const BluIO& last,
                    const void* table, uint32_t filters, uint32_t first_row, unsigned nxcd_conv, unsigned nxcd_last, double scale,
                    hipStream_t stream, Profiler* prof) const {
    const int np = (int)eng_->num_passes();
    const Pow2Engine<T>& inv = eng_inv_ ? *eng_inv_ : *eng_;
    cpx<T>* bufs[2] = {buf_a, buf_b};
    const cpx<T>* src = in;
    int cur = 0;
    for (int p = 0; p + 1 < np; ++p) {
      eng_->launch_pass((size_t)p, src, bufs[cur], nb, false, 1.0, stream, prof, 1 + p, nxcd_, p == 0 ? first : BluIO());
      src = bufs[cur]; cur ^= 1;
    }
    eng_->launch_conv(src, bufs[cur], nb, table, stream, prof, np, nxcd_conv, filters, first_row);
    src = bufs[cur]; cur ^= 1;
    for (int p = 1; p < np; ++p) {
      const bool end = (p + 1 == np);
      cpx<T>* dst = end ? out : bufs[cur];
      inv.launch_pass((size_t)p, src, dst, nb, true, end ? scale : 1.0, stream, prof, 1 + np + p, end ? nxcd_last : nxcd_, end ? last : BluIO());
      src = dst; cur ^= 1;
    }
  }
  // What a Bluestein plan runs, derived from the caller's requests (want_*) alone -- after init_bluestein(), after every rebuild and after
  // every Bluestein setter, so that the order of the setters and the values set before do not matter:
  //   "bluestein_smooth_m" chooses M and the route; "bluestein_fusion" = 0 takes a register-route plan to the reference's power-of-two M
  //   (the rule of mode 0) and a power-of-two inner plan to the separate sweeps, and is ignored on the three-sweep tile route; the conv
  //   kernel needs the fused end passes; "bluestein_reference_chirp" = 1 overrides "bluestein_chirp_compute" while it is set.
  // Rebuilds the route and the tables only where they change (not while a transform is in flight on this handle).
  void apply_bluestein_options() {
    const int mode = (!want_fusion_ && register_route_m(want_smooth_m_) != 0) ? 0 : want_smooth_m_;
    if (mode != smooth_m_mode_) {
      HIP_CHECK(hipDeviceSynchronize());
      smooth_m_mode_ = mode;
      blur_.reset(); blut_.reset(); eng_.reset(); eng_inv_.reset();
      init_bluestein();
    }
    if (tables_reference_ != want_reference_chirp_) {
      HIP_CHECK(hipDeviceSynchronize());  // the tables are replaced in place
      build_chirp_tables(want_reference_chirp_);
    }
    fused_ = want_fusion_ && fuse_ok_;
    small_fused_ = want_fusion_ && small_ok_;
    conv_ = want_conv_ && conv_ok_;
    chirp_compute_ = !want_reference_chirp_ && chirp_ok_ && (want_chirp_compute_ < 0 ? chirp_default_ : want_chirp_compute_ == 1);
    refresh_desc();
  }
  // the M of the one-launch register route (kernels_chirpz.h) where rule `mode` of "bluestein_smooth_m" takes it for this length, else 0
  uint32_t register_route_m(int mode) const {
    if (mode == 0 || dev_env("FOURIER_NO_SMOOTH_M")) return 0;
    size_t m2 = 1;
    while (m2 < 2 * n_ - 1) m2 <<= 1;
    const uint32_t mr = BluRegEngine<T>::choose_m(n_);
    // Three stages (M = R1 x R2 x R3, 1296 ... 3072 and 8820 / 9261): where M is at least 1.25 x shorter -- f32 1.13 ... 1.6 x, f64 1.05 ... 1.55 x
    // the power-of-two one-launch kernels of M = 2048, 4096, 16384 (profiles/r06_s46_chirpz_reg3_ab.jsonl)
    const bool pays = mr > 1152 ? 5 * (uint64_t)mr <= 4 * (uint64_t)m2
                                : (sizeof(T) == 8 || mr <= 64 || (mr <= 800 && 11 * (uint64_t)mr <= 10 * (uint64_t)m2) || 17 * (uint64_t)mr <= 10 * (uint64_t)m2);
    return (mr != 0 && (mode == 2 || pays)) ? mr : 0;
  }
  // builds the route of rule smooth_m_mode_ in its fused form, with the chirp tables of the angle the caller wants (once: a rebuild under
  // "bluestein_reference_chirp" does not build the exact tables first); what the route CAN do goes to
  // fuse_ok_, small_ok_, conv_ok_, chirp_ok_ and chirp_default_, and apply_bluestein_options() decides what it does
  void init_bluestein() {
    blu_ = true;
    if (n_ > ((size_t)1 << 26)) throw EngineError(::fourier::c::FOURIER_HIP_UNSUPPORTED, "Bluestein sizes above 2^26 are not supported");
    m_ = 1;
    while (m_ < 2 * n_ - 1) m_ <<= 1;  // bluesteins.rs:110
    if (2 * n_ > m_) throw EngineError(::fourier::c::FOURIER_HIP_RUNTIME_ERROR, "Bluestein: M < 2N");  // the fused end passes rely on it
    fuse_ok_ = small_ok_ = conv_ok_ = chirp_ok_ = chirp_default_ = false;
    // M need only reach 2N - 1 (bluesteins.rs:110 rounds up to a power of two: up to 4N).  Beyond the one-launch kernels (M <= 2^15, f64 2^14)
    // the work array is swept three times: a product of two register-tile lengths instead, where the power-of-two array is at least 1.6 x
    // longer -- f32 +3 ... 43 %, f64 +20 ... 51 % there -- and in f64 from 1.44 x on while the conv kernel stays within 336 points (+5 ... 11 %;
    // beyond: -8 %).  Below that the power-of-two tiles' higher rate wins (f32 1.49 x: -7 ... -2 %; 1.35 x: -5 ... -1 %; f64 1.35 x: 0 ... +3 %;
    // profiles/r06_s35_smooth_m_late_loads_*.jsonl)
    // A short transform (M up to 1024 points, f32 1152): the whole chirp-z in one launch on M = R1 x R2 with both transforms in registers
    // (kernels_chirpz.h).  f64: wherever such an M exists -- 1.15 ... 2.05 x the power-of-two one-launch kernels, 1.2 - 1.3 x at the SAME M (64, 256,
    // 1024).  f32 (two transforms per lane, packed arithmetic): where M is at least 1.1 x shorter (1.1 ... 1.55 x up to M = 784; 480 against 512
    // and the stages of 30 and 32 points against 1024: 0.88 ... 0.99), up to M = 64 regardless (1.2 x at 64 against 64), 1152 against 2048
    // (1.37 x) -- profiles/r06_s45_chirpz_reg_ab.jsonl
    if (const uint32_t mr = register_route_m(smooth_m_mode_)) {
      m_ = mr;
      blur_.reset(new BluRegEngine<T>(n_, mr));
      build_chirp_tables(want_reference_chirp_);
      return;
    }
    if (smooth_m_mode_ != 0 && !dev_env("FOURIER_NO_SMOOTH_M") && m_ > ((size_t)1 << (sizeof(T) == 4 ? 15 : 14))) {
      uint32_t l1 = 0, l2 = 0;
      const uint64_t ms = BluTiledEngine<T>::choose_m(n_, l1, l2);
      const bool pays = smooth_m_mode_ == 2 || 8 * ms <= 5 * (uint64_t)m_ || (sizeof(T) == 8 && 36 * ms <= 25 * (uint64_t)m_ && l2 <= 336);
      if (ms != 0 && pays) {
        m_ = ms;
        blut_.reset(new BluTiledEngine<T>(n_, l1, l2));
        build_chirp_tables(want_reference_chirp_);
        return;
      }
    }
    // forward inner plan: the larger pass first (2048 x 1024 at M = 2^21), so the conv kernel runs at the SHORTER length
    // and the end passes at the longer one.  FOURIER_BLU_SHORT_FIRST=1 (experiment) swaps the roles: 1024 x 2048 forward,
    // end passes of length 1024, conv kernel at 2048.
    const bool short_first = dev_env("FOURIER_BLU_SHORT_FIRST") != nullptr;
    eng_.reset(new Pow2Engine<T>(m_, short_first));
    eng_->enable_bluestein_fusion();
    fuse_ok_ = eng_->can_fuse_bluestein();
    small_ok_ = eng_->enable_bluestein_small();
    if (fuse_ok_ && eng_->can_conv()) {
      // the inverse inner FFT must begin with the pass length the forward one ends with: the same plan when the
      // lengths read the same in both directions, otherwise its mirror image
      eng_->enable_conv();
      if (!eng_->palindromic()) {
        eng_inv_.reset(new Pow2Engine<T>(m_, !short_first));
        eng_inv_->enable_bluestein_fusion();
      }
      conv_ok_ = true;
    }
    build_chirp_tables(want_reference_chirp_);
    const uint64_t two_n = 2 * (uint64_t)n_;
    if (fuse_ok_ && !small_ok_) {
      // Tables for the chirp-in pass that computes the chirp instead of reading x (a quarter of that pass's traffic):
      // index k = row*cn + b  =>  x[k] = W_2n^{(row*cn)^2} * W_2n^{b^2} * W_n^{cn*row*b}; exact exponents, f64 trig, cast.
      const uint64_t cn = eng_->first_cn(), rows = (uint64_t)eng_->first_len() / 2;
      std::vector<cpx<T>> pt(rows), ut(cn);
      for (uint64_t r = 0; r < rows; ++r) {
        const unsigned __int128 k = (unsigned __int128)r * cn;
        pt[r] = root<T>((uint64_t)((k * k) % two_n), two_n);
      }
      for (uint64_t b = 0; b < cn; ++b) ut[b] = root<T>((uint64_t)(((unsigned __int128)b * b) % two_n), two_n);
      chirp_p_.upload(pt);
      chirp_u_.upload(ut);
      tn_bits_ = upload_two_level<T>(n_, tn_lo_, tn_hi_);  // W_n^e
      // Default: only where it pays.  Measured (profiles/r03_s7_chirp_compute_ab.jsonl): C4 (N = 999983, first pass of length
      // 2048 on 8-column tiles) 2.76-2.85 vs 2.92-3.08 ms per 512, f64 2.61 vs 2.88; N = 40000 / 65537 (the 0.3-0.5 MB table
      // is L2-resident anyway) and N = 2200000 (first pass of length 256: 32-column tiles, eight times the per-tile table
      // work) are 5-17 % SLOWER.  So: a long first pass and a table beyond an XCD's L2.
      chirp_ok_ = true;
      chirp_default_ = eng_->first_len() >= 1024 && n_ * ELEM >= ((size_t)4 << 20);
    }
  }
  // The chirp x[k] = exp(-i*pi*k^2/n) (bluesteins.rs:51-61) and w = FFT_M(conj chirp, mirrored) (bluesteins.rs:18-48), evaluated in f64 on
  // the host and cast (twiddle.rs:7-19 style), the inner IFFT's 1/M (bluesteins.rs:239 -> mod.rs:383) folded into w.
  // reference_angle = false (default): the angle is reduced exactly, k^2 mod 2n, before the trigonometry -- the reference leaves it
  // unreduced (bluesteins.rs:10,31,57: theta = k^2 * pi / n in f64, up to pi * n radians), which costs it about n * 1e-16 of
  // absolute angle error (2e-10 at n = 10^6: invisible in f32, the whole error budget in f64).  true (plan option
  // "bluestein_reference_chirp"): the reference's own expression, for a caller who wants the reference's f64 RESULTS rather than the
  // exact DFT: the engine then agrees with the CPU restatement to f64 rounding instead of to 1e-9 (tests: test_bluestein_reference_chirp).
  void build_chirp_tables(bool reference_angle) {
    std::vector<double> cr(n_), ci(n_);
    const uint64_t two_n = 2 * (uint64_t)n_;
    for (size_t k = 0; k < n_; ++k) {
      double ang;
      if (reference_angle) {
        const double index = (double)k * (double)k;  // (i as f64).powi(2), bluesteins.rs:31,57
        ang = index * M_PI / (double)n_;             // bluesteins.rs:10
      } else {
        const uint64_t r = (uint64_t)(((unsigned __int128)k * k) % two_n);
        ang = M_PI * (double)r / (double)n_;
      }
      cr[k] = std::cos(ang); ci[k] = -std::sin(ang);
    }
    std::vector<cpx<T>> x(n_);
    for (size_t k = 0; k < n_; ++k) x[k] = {(T)cr[k], (T)ci[k]};  // x_fwd, bluesteins.rs:51-61
    xtab_.upload(x);
    std::vector<double> wr(m_, 0.0), wi(m_, 0.0);
    for (size_t k = 0; k < n_; ++k) {
      wr[k] = cr[k]; wi[k] = -ci[k];
      if (k) { wr[m_ - k] = cr[k]; wi[m_ - k] = -ci[k]; }
    }
    host_fft_any(wr, wi);
    std::vector<cpx<T>> w(m_);
    const double inv_m = 1.0 / (double)m_;
    for (size_t k = 0; k < m_; ++k) w[k] = {(T)(wr[k] * inv_m), (T)(wi[k] * inv_m)};
    wtab_.upload(w);
    tables_reference_ = reference_angle;
  }

  // pageable <-> pinned copies of a chunk, split over a few threads (one core moves ~10 GB/s, PCIe wants 50+ each way)
  struct CopyJob { void* dst; const void* src; size_t bytes; };
  static void parallel_copy(const CopyJob* jobs, int njobs) {
    std::vector<std::thread> th;
    for (int j = 0; j < njobs; ++j) {
      const CopyJob job = jobs[j];
      const size_t nt = std::max<size_t>(1, std::min<size_t>(COPY_THREADS, job.bytes / ((size_t)2 << 20)));
      // ceil(bytes / nt) rounded up to a page: nt * piece >= bytes for every byte count (floor division dropped
      // the last r < nt bytes of jobs of the form nt*4096*k + r)
      const size_t piece = (((job.bytes + nt - 1) / nt) + 4095) & ~(size_t)4095;
      for (size_t t = 0; t < nt; ++t) {
        const size_t off = t * piece;
        if (off >= job.bytes) break;
        const size_t len = std::min(piece, job.bytes - off);
        if (nt == 1 && njobs == 1) { std::memcpy(job.dst, job.src, len); return; }
        th.emplace_back([=] { std::memcpy((char*)job.dst + off, (const char*)job.src + off, len); });
      }
    }
    for (auto& t : th) t.join();
  }
  static constexpr size_t COPY_THREADS = 12;
  struct HostPipe {  // exec_host_batch: NSLOTS slots, three streams
    static constexpr int NS = 4;
    PinnedBuf pin_in[NS], pin_out[NS];
    DevBuf dev[NS];
    hipStream_t s_h2d = nullptr, s_comp = nullptr, s_d2h = nullptr;
    hipEvent_t h2d_done[NS] = {}, comp_done[NS] = {}, d2h_done[NS] = {};
    void ensure(size_t bytes) {
      if (!s_h2d) {
        HIP_CHECK(hipStreamCreateWithFlags(&s_h2d, hipStreamNonBlocking));
        HIP_CHECK(hipStreamCreateWithFlags(&s_comp, hipStreamNonBlocking));
        HIP_CHECK(hipStreamCreateWithFlags(&s_d2h, hipStreamNonBlocking));
        for (int s = 0; s < NS; ++s) {
          HIP_CHECK(hipEventCreateWithFlags(&h2d_done[s], hipEventDisableTiming));
          HIP_CHECK(hipEventCreateWithFlags(&comp_done[s], hipEventDisableTiming));
          HIP_CHECK(hipEventCreateWithFlags(&d2h_done[s], hipEventDisableTiming));
        }
      }
      for (int s = 0; s < NS; ++s) { pin_in[s].ensure(bytes); pin_out[s].ensure(bytes); dev[s].ensure(bytes); }
    }
    ~HostPipe() {
      for (int s = 0; s < NS; ++s)
        for (hipEvent_t e : {h2d_done[s], comp_done[s], d2h_done[s]})
          if (e) (void)hipEventDestroy(e);
      for (hipStream_t st : {s_h2d, s_comp, s_d2h})
        if (st) (void)hipStreamDestroy(st);
    }
  };
  static_assert(NSLOTS == HostPipe::NS, "slot count");
  mutable HostPipe pipe_;

  size_t n_, m_ = 0;
  int device_ = 0;
  bool blu_ = false;
  std::unique_ptr<Pow2Engine<T>> eng_, eng_inv_;  // eng_inv_: mirrored inverse plan of a conv-fused Bluestein, or of the convolution handle's fused passes (enable_conv_bank)
  std::unique_ptr<BluTiledEngine<T>> blut_;       // Bluestein on a smooth M (then eng_ is empty)
  std::unique_ptr<BluRegEngine<T>> blur_;         // ... of a short transform: one launch, transforms in registers (then eng_ is empty)
  std::unique_ptr<BluRegEngine<T>> regf_;         // a length with factors 5 ... 13 as a direct transform on the same register stages
  bool regf_on_request_ = false;                  // ... of a 2^a 3^b length, by plan option "register_stages" (mix_ stays allocated)
  // the caller's requests, as the Bluestein options were last set (apply_bluestein_options derives everything else from them)
  int want_smooth_m_ = 1;                         // option "bluestein_smooth_m"
  bool want_fusion_ = true, want_conv_ = true;    // options "bluestein_fusion", "bluestein_conv"
  int want_chirp_compute_ = -1;                   // option "bluestein_chirp_compute"; -1: never set, the plan's own default (chirp_default_)
  bool want_reference_chirp_ = false;             // option "bluestein_reference_chirp"
  int smooth_m_mode_ = 1;                         // the rule the route was built under (init_bluestein): the request, or 0 for an unfused register-route plan
  std::unique_ptr<MixedEngine<T>> mix_;
  std::unique_ptr<TiledMixedEngine<T>> tiled_;  // 2^a*3^b, a < 12, beyond the LDS kernels: column tiles of mixed length
  std::unique_ptr<GenericEngine<T>> gen_;  // ... and what has no tile factorisation: one global pass per radix
  DevBuf xtab_, wtab_;
  DevBuf chirp_p_, chirp_u_, tn_lo_, tn_hi_;  // chirp-in pass computing the chirp (init_bluestein)
  uint32_t tn_bits_ = 0;
  bool tables_reference_ = false;  // the x and w tables hold the reference's unreduced chirp angle (build_chirp_tables)
  bool chirp_ok_ = false, chirp_default_ = false;  // the route has the chirp-in pass that computes the chirp; ... and runs it by default
  bool chirp_compute_ = false;  // effective: the chirp-in pass computes the chirp
  mutable DevBuf scratch_, work_, hostio_;
  mutable PinnedBuf pinned_;
  mutable hipStream_t legacy_stream_ = nullptr;  // legacy host-buffer calls (exec_host)
  size_t chunk_bytes_ = 0;
  size_t host_chunk_bytes_ = HOST_CHUNK_BYTES;  // exec_host_batch: bytes of one streamed chunk
  bool force_scratch_ = false;
  size_t pipe_chunk_ = 0, pipe_slots_ = 0;  // option "stream_pipeline"
  bool pipe_one_stream_ = false;
  // effective flags (apply_bluestein_options) and what the route can do (init_bluestein: *_ok_)
  bool fused_ = false, fuse_ok_ = false;  // Bluestein: chirp steps fused into the inner passes
  bool small_fused_ = false, small_ok_ = false;  // Bluestein with M <= 2^15: everything in one launch
  bool conv_ = false, conv_ok_ = false;  // Bluestein: forward LAST + (.)w + inverse FIRST in one launch (runs where fused_ too)
  int conv_route_ = 0;  // enable_conv_bank: the convolution handle's route on this plan (CONV_NONE ...)
  unsigned nxcd_ = 8, nxcd_last_ = 0;
  mutable std::shared_ptr<AxisRoute<T>> axis_;  // (shared_ptr: AxisRoute<T> is incomplete here)
  size_t axis_scratch_bytes_ = 0;               // 0: AXIS_SCRATCH_BYTES
  bool axis_force_transpose_ = false;
};

}  // namespace fourier_hip
