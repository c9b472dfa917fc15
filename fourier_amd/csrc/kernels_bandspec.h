// kernels_bandspec.h -- device code of the band-energy spectrogram (BandSpecPlan, bandspec_plan.h): Y[j] = sum_k W[j, k] |X[k]|^p of the
// STFT's frames X (kernels_stft.h) for a sparse-row bank W (BandSpecArgs, kernel_args.h), optionally log_mult * ln(max(Y, log_floor)),
// without |X|^p reaching memory on the fused route.
//   bandspec_sweep_kernel  composed route: one lane per (frame, band) over the chunk's transformed frames in the scratch; |Z|^p is formed
//                          on the fly, the band summed in ascending k in one accumulator, the log applied, the caller's output written.
//   bandspec_rows_kernel   fused route for n_fft = 2h with a whole-row h-point kernel, on the flat frame index: spectrogram_rows_kernel's
//                          gather, window, row core and LDS-staged untangle restated (that kernel's generated code stays what it was), its
//                          Welch epilogue's LDS layout of the tile's |X|^p -- frame c at c * PS, PS = h + 1 odd, bin h from the th == 0
//                          lane, dead frames zero -- and then a band epilogue: work item i = c + COLS * j (frame c fastest: the lanes of a
//                          wave walk the odd pitch on distinct banks, and the weight of a step is one address per band) sums its band into
//                          a register; after a barrier the results go to LDS as the output lays them out, c * bands + j -- they fit the
//                          area the powers held because bands <= bins = PS -- and leave as ONE contiguous run of live frames * bands
//                          reals, a lane per element, cut at f.total.
// No atomics, no sum across frames: a result depends on its frame and the bank alone.
#pragma once
#include "kernels_spectrogram.h"

FOURIER_KERNELS_BEGIN

__device__ __forceinline__ float band_ln(float x) { return logf(x); }
__device__ __forceinline__ double band_ln(double x) { return log(x); }
// log_mult == 0: linear; else log_mult * ln(max(y, log_floor)) with the library logarithm
template <typename T> __device__ __forceinline__ T band_finish(T y, T log_mult, T log_floor) {
  if (log_mult == (T)0) return y;
  return log_mult * band_ln(y > log_floor ? y : log_floor);
}

template <typename T>
__global__ void __launch_bounds__(STFT_THREADS) bandspec_sweep_kernel(BandSpecArgs a) {
  const cpx<T>* z = (const cpx<T>*)a.f.in;
  T* out = (T*)a.f.out;
  const uint32_t* lo = (const uint32_t*)a.lo;
  const uint32_t* off = (const uint32_t*)a.off;
  const T* w = (const T*)a.w;
  const T lm = (T)a.log_mult, lf = (T)a.log_floor;
  for (uint64_t i = (uint64_t)blockIdx.x * STFT_THREADS + threadIdx.x; i < a.count; i += (uint64_t)gridDim.x * STFT_THREADS) {
    const uint64_t fr = i / a.bands;
    const uint32_t j = (uint32_t)(i - fr * a.bands);
    const uint32_t o0 = off[j], cnt = off[j + 1] - o0;
    const cpx<T>* p = z + fr * a.bins + lo[j];
    const T* wp = w + o0;
    T acc = 0;
    for (uint32_t k = 0; k < cnt; ++k) {
      const cpx<T> v = p[k];
      acc += wp[k] * spec_value(v.re, v.im, a.power);
    }
    out[i] = band_finish(acc, lm, lf);
  }
}

// ---- the fused route.  The occupancy request and the staging area are stft_rows_kernel's (FrameRowsCfg).
template <typename T, int L, int CG, int OUT>
__global__ void __launch_bounds__((L / 16) * CG, 4) bandspec_rows_kernel(BandSpecArgs a) {
  using C = TileCfg<T, L, CG>;
  using S = FrameRowsCfg<T, L, CG>;
  constexpr int VEC = C::VEC, Q = C::Q, COLS = C::COLS, HALF = S::HALF, LP = S::LP, NT = C::NT;
  constexpr int PS = L + 1;  // the reals of one frame's powers in LDS: an odd row pitch, neighbouring frames on neighbouring banks
  constexpr int ITEMS = (COLS * PS + NT - 1) / NT;  // (frame, band) items of a lane at bands = bins, the most the route takes
  static_assert(OUT == SPEC_MAGNITUDE || OUT == SPEC_POWER, "band rows kernel: |X| or |X|^2");
  static_assert(Q > 1 && COLS % 2 == 0 && (COLS & (COLS - 1)) == 0, "band rows kernel: L >= 32, a power-of-two number of frames per tile");
  // LDS budget: the tile's powers, COLS rows of PS reals, and later its results, COLS rows of bands <= PS reals, in the staging area
  static_assert((size_t)COLS * PS * sizeof(T) <= S::SMEM, "the powers and the band sums of a tile fit the staging area");
  FOURIER_DYN_SMEM(smem);
  const int tid = (int)threadIdx.x;
  int th = tid % Q, cg = tid / Q;
  // every XCD walks one contiguous range of the flat frame index: the frames that share samples meet in one L2
  const uint32_t blk = real_xcd_block(blockIdx.x, gridDim.x);
  const uint64_t g0 = (uint64_t)blk * COLS;
  const T* __restrict__ in = (const T*)a.f.in;
  const cpx<T>* __restrict__ win = (const cpx<T>*)a.f.win + th;  // (w[2m], w[2m+1]) as the complex value m
  const int64_t length = (int64_t)a.f.length;

  // ---- load: register r <- complex value m = th + Q*r of frame cg*VEC + v of the tile
  cpx<T> x[VEC][16];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    const uint64_t g = g0 + (uint64_t)(cg * VEC + v);
    if (g >= a.f.total) {  // a dead frame: zeros, so its powers are zero
#pragma unroll
      for (int r = 0; r < 16; ++r) x[v][r] = cpx<T>{0, 0};
      continue;
    }
    uint32_t row, f;
    frame_of(a.f, (uint32_t)g, row, f);
    const T* src = in + (uint64_t)row * a.f.length;
    const int64_t t0 = (int64_t)f * a.f.hop - (int64_t)a.f.pad;
    if (t0 >= 0 && t0 + (int64_t)a.f.n_fft <= length) {
      // an interior frame: no padding index.  Two reals per access where every frame starts on an aligned pair, single reals otherwise
      const T* p = src + t0 + 2 * th;
      if (a.f.pairs) {
#pragma unroll
        for (int r = 0; r < 16; ++r) x[v][r] = *(const cpx<T>*)(p + 2 * Q * r);
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) x[v][r] = cpx<T>{p[2 * Q * r], p[2 * Q * r + 1]};
      }
    } else {
      // an edge frame: the mirrored or zeroed index per element
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t t = t0 + 2 * (th + Q * r);
        x[v][r] = cpx<T>{stft_sample(src, t, length, a.f.mode), stft_sample(src, t + 1, length, a.f.mode)};
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const cpx<T> w = win[Q * r];  // plain loads: the table is shared by every frame and stays in the L2
      x[v][r] = cpx<T>{x[v][r].re * w.re, x[v][r].im * w.im};
    }
  }

  // ---- Z = FFT_h: register r holds Z[k], k = th + Q*r, of frame cg*VEC + v
  tile_core<T, L, CG, MODE_ROWS>(x, th, cg, tid, smem, (const cpx<T>*)a.f.tw1, (const cpx<T>*)a.f.tw2);

  // ---- untangle through LDS, half a tile at a time, as stft_rows_kernel: X[k] = s/2 (E + W_N^k O); |X[k]|^p stays in x[v][r].re and
  // bin h's in xh[v]
  cpx<T>* stage = (cpx<T>*)smem;
  const cpx<T>* tw = (const cpx<T>*)a.f.tw;
  const T s = (T)a.f.scale * (T)0.5;
  T xh[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) xh[v] = 0;
  __syncthreads();  // the last exchange's readers are done with the buffer
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const int col = VEC == 2 ? v * CG + cg : cg;  // position in the staging order: each half one run of HALF frames
      if (col / HALF == hf) {
        cpx<T>* p = stage + (col % HALF) * LP + th;
#pragma unroll
        for (int r = 0; r < 16; ++r) p[Q * r] = x[v][r];
      }
    }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const int col = VEC == 2 ? v * CG + cg : cg;
      if (col / HALF == hf) {
        const cpx<T>* z = stage + (col % HALF) * LP;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int k = th + Q * r;
          const cpx<T> A = x[v][r], P = z[k == 0 ? 0 : L - k];
          const cpx<T> t1 = tw[k <= L / 2 ? k : L - k];
          const cpx<T> w = k <= L / 2 ? t1 : cpx<T>{-t1.re, t1.im};
          const cpx<T> e = {A.re + P.re, A.im - P.im};
          const cpx<T> o = {A.im + P.im, P.re - A.re};
          const cpx<T> t = cmul(w, o);
          const T edge = (T)a.f.scale * (A.re - A.im);  // bin h, real
          x[v][r].re = spec_value(s * (e.re + t.re), s * (e.im + t.im), (uint32_t)OUT);
          if (k == 0) xh[v] = OUT == SPEC_MAGNITUDE ? (edge < 0 ? -edge : edge) : edge * edge;
        }
      }
    }
    __syncthreads();
  }

  // ---- the tile's powers to LDS, frame c = cg*VEC + v at c * PS
  T* pw = (T*)smem;
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    T* p = pw + (cg * VEC + v) * PS + th;
#pragma unroll
    for (int r = 0; r < 16; ++r) p[Q * r] = x[v][r].re;
    if (th == 0) p[L] = xh[v];
  }
  __syncthreads();

  // ---- the band sums: item i = c + COLS * j, frame c fastest, in registers until every lane has read the powers
  const uint32_t* __restrict__ lo = (const uint32_t*)a.lo;
  const uint32_t* __restrict__ off = (const uint32_t*)a.off;
  const T* __restrict__ wt = (const T*)a.w;  // plain loads: the bank is a few KB and stays in the L2
  const T lm = (T)a.log_mult, lf = (T)a.log_floor;
  const uint32_t nb = a.bands, items = (uint32_t)COLS * nb;  // nb <= PS (the plan takes this route for bands <= bins only)
  T y[ITEMS];
#pragma unroll
  for (int n = 0; n < ITEMS; ++n) {
    const uint32_t i = (uint32_t)(tid + n * NT);
    T acc = 0;
    if (i < items) {
      const uint32_t c = i % COLS, j = i / COLS;
      const uint32_t o0 = off[j], cnt = off[j + 1] - o0;
      const T* pp = pw + c * PS + lo[j];  // lo[j] + cnt <= bins = PS: inside frame c's row
      const T* wp = wt + o0;
      for (uint32_t k = 0; k < cnt; ++k) acc += wp[k] * pp[k];
      acc = band_finish(acc, lm, lf);
    }
    y[n] = acc;
  }
  __syncthreads();  // the powers are read: their area takes the results, laid out as the output, frame c's bands at c * nb
#pragma unroll
  for (int n = 0; n < ITEMS; ++n) {
    const uint32_t i = (uint32_t)(tid + n * NT);
    if (i < items) pw[(i % COLS) * nb + i / COLS] = y[n];
  }
  __syncthreads();
  // ---- one contiguous run of the tile's live frames x bands reals: a lane per element, rows only element-aligned, so no wider stores
  const uint64_t left = g0 < a.f.total ? a.f.total - g0 : 0;
  const uint32_t run = (left < (uint64_t)COLS ? (uint32_t)left : (uint32_t)COLS) * nb;
  T* __restrict__ dst = (T*)a.f.out + g0 * (uint64_t)nb;
  for (uint32_t i = (uint32_t)tid; i < run; i += NT) dst[i] = pw[i];
}

FOURIER_KERNELS_END
