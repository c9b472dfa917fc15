// kernels_spectrogram.h -- device code of the power spectrogram and the Welch average (SpectrogramPlan, spectrogram_plan.h): |X|^p of
// the STFT's frames X (kernels_stft.h) without the complex frames ever reaching memory, and the mean of |X|^2 over a row's frames.
//   spectrogram_rows_kernel  fused route for n_fft = 2h with a whole-row h-point kernel: stft_rows_kernel's gather, window, row core and
//                            LDS-staged untangle restated (that kernel's generated code stays what it was), with another epilogue.
//                            OUT = SPEC_POWER / SPEC_MAGNITUDE: the lane that holds bin k stores one real at out + g * (h + 1) + k, bin h
//                            from the k = 0 lane -- half the bytes of the complex store.  OUT = SPEC_PARTIAL (Welch): the launch is tiled
//                            per row, `tiles` = ceil(frames / COLS) workgroups a row, the columns past the row's last frame load as zero
//                            and so add exactly 0; the |X|^2 of the tile go to LDS (COLS rows of h + 1 reals, inside the staging area the
//                            untangle used) and one lane per bin sums them in ascending frame order into one row of h + 1 partials.
//   welch_reduce_kernel      out[b, k] = scale * c_k * sum_t partial[b][t][k] in ascending t, one lane per (b, k); the final sweep of
//                            both Welch routes (a.scale already holds the 1 / frames).
//   spectrogram_power_kernel composed route: |Z|^p over the chunk's transformed frames in the scratch, into the caller's output.
//   welch_colsum_kernel      composed route: one lane per (slot, k) of the slots -- runs of `tile_frames` frames of one row -- a chunk
//                            of the flat frame index meets, the |Z|^2 of the slot's frames inside the chunk summed in ascending order.
//                            The chunk that holds a slot's first frame writes the slot, a later chunk adds to what is there: launches
//                            of one stream run in order, so the sum's order is fixed by the chunking.  No atomics anywhere.
#pragma once
#include "kernels_stft.h"

FOURIER_KERNELS_BEGIN

__device__ __forceinline__ float spec_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double spec_sqrt(double x) { return sqrt(x); }
template <typename T> __device__ __forceinline__ T spec_value(T re, T im, uint32_t power) {
  const T p = re * re + im * im;
  return power == SPEC_MAGNITUDE ? spec_sqrt(p) : p;
}

template <typename T>
__global__ void __launch_bounds__(STFT_THREADS) spectrogram_power_kernel(SpectrogramArgs a) {
  const cpx<T>* z = (const cpx<T>*)a.f.in;
  T* out = (T*)a.f.out;
  for (uint64_t i = (uint64_t)blockIdx.x * STFT_THREADS + threadIdx.x; i < a.count; i += (uint64_t)gridDim.x * STFT_THREADS) {
    const cpx<T> v = z[i];
    out[i] = spec_value(v.re, v.im, a.power);
  }
}

template <typename T>
__global__ void __launch_bounds__(STFT_THREADS) welch_colsum_kernel(SpectrogramArgs a) {
  const cpx<T>* z = (const cpx<T>*)a.f.in;
  T* part = (T*)a.part;
  const uint64_t fr = a.f.frames, tf = a.tile_frames;
  for (uint64_t i = (uint64_t)blockIdx.x * STFT_THREADS + threadIdx.x; i < a.count; i += (uint64_t)gridDim.x * STFT_THREADS) {
    const uint64_t sl = i / a.bins, k = i - sl * a.bins;
    const uint64_t vt = a.slot0 + sl, r = vt / a.tiles, t = vt - r * a.tiles;
    const uint64_t s0 = r * fr + t * tf, s1 = r * fr + ((t + 1) * tf < fr ? (t + 1) * tf : fr);
    const uint64_t lo = s0 > a.g0 ? s0 : a.g0, hi = s1 < a.g1 ? s1 : a.g1;
    T acc = 0;
    for (uint64_t g = lo; g < hi; ++g) {
      const cpx<T> v = z[(g - a.g0) * a.bins + k];
      acc += v.re * v.re + v.im * v.im;
    }
    T* p = part + vt * a.bins + k;
    *p = s0 >= a.g0 ? acc : *p + acc;
  }
}

template <typename T>
__global__ void __launch_bounds__(STFT_THREADS) welch_reduce_kernel(SpectrogramArgs a) {
  const T* part = (const T*)a.part;
  T* out = (T*)a.f.out;
  for (uint64_t i = (uint64_t)blockIdx.x * STFT_THREADS + threadIdx.x; i < a.count; i += (uint64_t)gridDim.x * STFT_THREADS) {
    const uint64_t b = i / a.bins, k = i - b * a.bins;
    const T* p = part + b * a.tiles * (uint64_t)a.bins + k;
    T acc = 0;
    for (uint32_t t = 0; t < a.tiles; ++t) acc += p[(uint64_t)t * a.bins];
    const T c = a.fold && k > 0 && 2 * k < a.f.n_fft ? (T)2 : (T)1;
    out[i] = (T)a.scale * c * acc;
  }
}

// ---- the fused route.  The occupancy request and the staging area are stft_rows_kernel's (FrameRowsCfg).
template <typename T, int L, int CG, int OUT>
__global__ void __launch_bounds__((L / 16) * CG, 4) spectrogram_rows_kernel(SpectrogramArgs a) {
  using C = TileCfg<T, L, CG>;
  using S = FrameRowsCfg<T, L, CG>;
  constexpr int VEC = C::VEC, Q = C::Q, COLS = C::COLS, HALF = S::HALF, LP = S::LP, NT = C::NT;
  constexpr int PS = L + 1;  // the reals of one frame's powers in LDS: an odd row pitch, neighbouring frames on neighbouring banks
  static_assert(Q > 1 && COLS % 2 == 0, "spectrogram rows kernel: L >= 32, an even number of frames per tile");
  static_assert((size_t)COLS * PS * sizeof(T) <= S::SMEM, "the powers of a tile fit the staging area");
  FOURIER_DYN_SMEM(smem);
  const int tid = (int)threadIdx.x;
  int th = tid % Q, cg = tid / Q;
  // every XCD walks one contiguous range of the flat frame index (PARTIAL: of the tiles of consecutive rows): the frames that share
  // samples meet in one L2
  const uint32_t blk = real_xcd_block(blockIdx.x, gridDim.x);
  const uint64_t g0 = (uint64_t)blk * COLS;
  const uint32_t prow = OUT == SPEC_PARTIAL ? real_div(blk, a.tl_m, a.tl_l) : 0, ptile = blk - prow * a.tiles;
  const T* __restrict__ in = (const T*)a.f.in;
  const cpx<T>* __restrict__ win = (const cpx<T>*)a.f.win + th;  // (w[2m], w[2m+1]) as the complex value m
  const int64_t length = (int64_t)a.f.length;

  // ---- load: register r <- complex value m = th + Q*r of frame cg*VEC + v of the tile
  cpx<T> x[VEC][16];
  bool live[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    uint32_t row, f;
    if (OUT == SPEC_PARTIAL) {
      row = prow;
      f = ptile * COLS + (uint32_t)(cg * VEC + v);
      live[v] = f < a.f.frames;
    } else {
      const uint64_t g = g0 + (uint64_t)(cg * VEC + v);
      live[v] = g < a.f.total;
      frame_of(a.f, (uint32_t)g, row, f);
    }
    if (!live[v]) {
#pragma unroll
      for (int r = 0; r < 16; ++r) x[v][r] = cpx<T>{0, 0};
      continue;
    }
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

  // ---- untangle through LDS, half a tile at a time, as stft_rows_kernel: X[k] = s/2 (E + W_N^k O); what leaves is |X[k]|^p.
  // POWER / MAGNITUDE store it; PARTIAL keeps |X[k]|^2 in x[v][r].re and bin h's in xh[v] for the sum below.
  cpx<T>* stage = (cpx<T>*)smem;
  const cpx<T>* tw = (const cpx<T>*)a.f.tw;
  T* __restrict__ out = (T*)a.f.out;
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
      if (col / HALF == hf && (OUT == SPEC_PARTIAL || live[v])) {
        const cpx<T>* z = stage + (col % HALF) * LP;
        T* dst = out + (g0 + (uint64_t)(cg * VEC + v)) * (uint64_t)(L + 1);
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
          if (OUT == SPEC_PARTIAL) {
            x[v][r].re = spec_value(s * (e.re + t.re), s * (e.im + t.im), SPEC_POWER);
            if (k == 0) xh[v] = edge * edge;
          } else {
            // runs of Q reals per store instruction; rows of h + 1 reals are only element-aligned, so no streaming hint (as the STFT's)
            dst[k] = spec_value(s * (e.re + t.re), s * (e.im + t.im), (uint32_t)OUT);
            if (k == 0) dst[L] = OUT == SPEC_MAGNITUDE ? (edge < 0 ? -edge : edge) : edge * edge;
          }
        }
      }
    }
    if (hf == 0 || OUT == SPEC_PARTIAL) __syncthreads();
  }

  if (OUT == SPEC_PARTIAL) {
    // ---- the tile's powers to LDS, frame c = cg*VEC + v at c * PS; then one lane per bin sums the COLS frames in ascending order
    T* pw = (T*)smem;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      T* p = pw + (cg * VEC + v) * PS + th;
#pragma unroll
      for (int r = 0; r < 16; ++r) p[Q * r] = x[v][r].re;
      if (th == 0) p[L] = xh[v];
    }
    __syncthreads();
    T* dst = (T*)a.part + (uint64_t)blk * (uint64_t)(L + 1);
    for (int k = tid; k < L + 1; k += NT) {
      T acc = 0;
#pragma unroll
      for (int c = 0; c < COLS; ++c) acc += pw[c * PS + k];
      dst[k] = acc;
    }
  }
}

FOURIER_KERNELS_END
