// kernels_csd.h -- device code of the cross-spectral density and the coherence (CsdPlan, csd_plan.h): of the STFT's frames X of a row of
// x and Y of the same row of y (kernels_stft.h), the sums over a row's frames of |X|^2, |Y|^2 and conj(X) Y, without a frame reaching
// memory.  Four planes of h + 1 (bins) reals per slot of partials: CSD_PXX, CSD_PYY, CSD_RE, CSD_IM (kernel_args.h).
//   csd_rows_kernel    fused route for n_fft = 2h with a whole-row h-point kernel: spectrogram_rows_kernel's gather, window, row core and
//                      LDS-staged untangle restated (that kernel's generated code stays what it was) on a tile that carries COLS / 2
//                      frame PAIRS: the columns staged in the first half are the x frames of pairs 0 ... HALF - 1, those of the second
//                      half the y frames of the same pairs.  f32 (VEC = 2): X[k] and Y[k] of a pair sit in one lane (v = 0, v = 1); f64
//                      (VEC = 1): in the lanes cg and cg + CG / 2, and the y half passes its untangled bins through the staging area.
//                      The launch is tiled per row, `tiles` = ceil(frames / HALF) workgroups a row; pairs past the row's last frame load
//                      as zero and so add exactly 0.  The tile's sums go through LDS in two rounds of two planes (|X|^2 and |Y|^2, then
//                      Re and Im of conj(X) Y; COLS rows of h + 1 reals each, inside the staging area the untangle used), one lane per
//                      bin sums the HALF pairs in ascending order into four rows of h + 1 partials.
//   csd_colsum_kernel  composed route: one lane per (slot, k) of the slots -- runs of `tile_frames` frames of one row -- a chunk of the
//                      flat frame index meets, the four products of the slot's frames inside the chunk summed in ascending order.  The
//                      chunk that holds a slot's first frame writes the slot, a later chunk adds to what is there (welch_colsum_kernel's
//                      rule): launches of one stream run in order, so the sum's order is fixed by the chunking.
//   csd_reduce_kernel  the final sweep of both routes: a row's slots summed in ascending order, one lane per (b, k); the cross spectrum
//                      scale * c_k * (Re, Im) (a.scale already holds the 1 / frames) or the coherence (Re^2 + Im^2) / (Pxx Pyy) as
//                      (Re / Pxx)(Re / Pyy) + (Im / Pxx)(Im / Pyy), plain IEEE divisions: no product of two sums is formed.
// No atomics anywhere.
#pragma once
#include "kernels_stft.h"

FOURIER_KERNELS_BEGIN

template <typename T>
__global__ void __launch_bounds__(STFT_THREADS) csd_colsum_kernel(CsdArgs a) {
  const cpx<T>* zx = (const cpx<T>*)a.f.in;
  const cpx<T>* zy = zx + a.ystride;
  T* part = (T*)a.part;
  const uint64_t fr = a.f.frames, tf = a.tile_frames;
  for (uint64_t i = (uint64_t)blockIdx.x * STFT_THREADS + threadIdx.x; i < a.count; i += (uint64_t)gridDim.x * STFT_THREADS) {
    const uint64_t sl = i / a.bins, k = i - sl * a.bins;
    const uint64_t vt = a.slot0 + sl, r = vt / a.tiles, t = vt - r * a.tiles;
    const uint64_t s0 = r * fr + t * tf, s1 = r * fr + ((t + 1) * tf < fr ? (t + 1) * tf : fr);
    const uint64_t lo = s0 > a.g0 ? s0 : a.g0, hi = s1 < a.g1 ? s1 : a.g1;
    T pxx = 0, pyy = 0, re = 0, im = 0;
    for (uint64_t g = lo; g < hi; ++g) {
      const cpx<T> x = zx[(g - a.g0) * a.bins + k], y = zy[(g - a.g0) * a.bins + k];
      pxx += x.re * x.re + x.im * x.im;
      pyy += y.re * y.re + y.im * y.im;
      re += x.re * y.re + x.im * y.im;
      im += x.re * y.im - x.im * y.re;
    }
    T* p = part + vt * CSD_PLANES * a.bins + k;
    const bool first = s0 >= a.g0;
    p[CSD_PXX * (uint64_t)a.bins] = first ? pxx : p[CSD_PXX * (uint64_t)a.bins] + pxx;
    p[CSD_PYY * (uint64_t)a.bins] = first ? pyy : p[CSD_PYY * (uint64_t)a.bins] + pyy;
    p[CSD_RE * (uint64_t)a.bins] = first ? re : p[CSD_RE * (uint64_t)a.bins] + re;
    p[CSD_IM * (uint64_t)a.bins] = first ? im : p[CSD_IM * (uint64_t)a.bins] + im;
  }
}

template <typename T>
__global__ void __launch_bounds__(STFT_THREADS) csd_reduce_kernel(CsdArgs a) {
  const T* part = (const T*)a.part;
  const uint64_t bins = a.bins, slot = CSD_PLANES * bins;
  for (uint64_t i = (uint64_t)blockIdx.x * STFT_THREADS + threadIdx.x; i < a.count; i += (uint64_t)gridDim.x * STFT_THREADS) {
    const uint64_t b = i / bins, k = i - b * bins;
    const T* p = part + b * a.tiles * slot + k;
    T re = 0, im = 0;
    for (uint32_t t = 0; t < a.tiles; ++t) {
      re += p[t * slot + CSD_RE * bins];
      im += p[t * slot + CSD_IM * bins];
    }
    if (a.coherence) {
      T pxx = 0, pyy = 0;
      for (uint32_t t = 0; t < a.tiles; ++t) {
        pxx += p[t * slot + CSD_PXX * bins];
        pyy += p[t * slot + CSD_PYY * bins];
      }
      // quotients first: neither Re^2 + Im^2 nor Pxx Pyy is formed at full magnitude.  |Re|, |Im| <= sqrt(Pxx Pyy), so every quotient is
      // at most sqrt(Pyy / Pxx) or its inverse; a power-of-two scaling of x and y moves the quotients by exact powers of two that cancel
      const T rx = re / pxx, ry = re / pyy, ix = im / pxx, iy = im / pyy;
      ((T*)a.f.out)[i] = rx * ry + ix * iy;
    } else {
      const T c = (T)a.scale * (a.fold && k > 0 && 2 * k < a.f.n_fft ? (T)2 : (T)1);
      ((cpx<T>*)a.f.out)[i] = cpx<T>{c * re, c * im};
    }
  }
}

// ---- the fused route.  The occupancy request and the staging area are stft_rows_kernel's (FrameRowsCfg).
template <typename T, int L, int CG>
__global__ void __launch_bounds__((L / 16) * CG, 4) csd_rows_kernel(CsdArgs a) {
  using C = TileCfg<T, L, CG>;
  using S = FrameRowsCfg<T, L, CG>;
  constexpr int VEC = C::VEC, Q = C::Q, COLS = C::COLS, HALF = S::HALF, LP = S::LP, NT = C::NT;
  constexpr int PS = L + 1;  // the reals of one frame's plane in LDS: an odd row pitch, neighbouring frames on neighbouring banks
  static_assert(Q > 1 && COLS % 2 == 0, "csd rows kernel: L >= 32, an even number of columns per tile");
  static_assert((size_t)COLS * PS * sizeof(T) <= S::SMEM, "two planes of a tile fit the staging area");
  static_assert(L + 1 <= LP, "a staged frame holds its h + 1 untangled bins");
  FOURIER_DYN_SMEM(smem);
  const int tid = (int)threadIdx.x;
  int th = tid % Q, cg = tid / Q;
  // every XCD walks the tiles of consecutive rows: the frames that share samples meet in one L2
  const uint32_t blk = real_xcd_block(blockIdx.x, gridDim.x);
  const uint32_t prow = real_div(blk, a.tl_m, a.tl_l), ptile = blk - prow * a.tiles;
  const cpx<T>* __restrict__ win = (const cpx<T>*)a.f.win + th;  // (w[2m], w[2m+1]) as the complex value m
  const int64_t length = (int64_t)a.f.length;

  // ---- load: register r <- complex value m = th + Q*r of column `col` of the staging order: the x frame (col < HALF) or the y frame of
  // pair col % HALF, frame ptile * HALF + col % HALF of the row
  cpx<T> x[VEC][16];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    const int col = VEC == 2 ? v * CG + cg : cg;
    const uint32_t f = ptile * HALF + (uint32_t)(col % HALF);
    if (f >= a.f.frames) {
#pragma unroll
      for (int r = 0; r < 16; ++r) x[v][r] = cpx<T>{0, 0};
      continue;
    }
    const T* src = (col < HALF ? (const T*)a.f.in : (const T*)a.in2) + (uint64_t)prow * a.f.length;
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

  // ---- Z = FFT_h: register r holds Z[k], k = th + Q*r, of the column
  tile_core<T, L, CG, MODE_ROWS>(x, th, cg, tid, smem, (const cpx<T>*)a.f.tw1, (const cpx<T>*)a.f.tw2);

  // ---- untangle through LDS, half a tile at a time, as stft_rows_kernel: X[k] = 1/2 (E + W_N^k O).  The bins stay in x[v][r], the
  // real bin h in xh[v] (its value in the k = 0 lane)
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
      const int col = VEC == 2 ? v * CG + cg : cg;
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
          if (k == 0) xh[v] = (T)a.f.scale * (A.re - A.im);  // bin h, real
          x[v][r] = cpx<T>{s * (e.re + t.re), s * (e.im + t.im)};
        }
      }
    }
    __syncthreads();
  }

  T* pw = (T*)smem;
  T* dst = (T*)a.part + (uint64_t)blk * (uint64_t)(CSD_PLANES * (L + 1));
  // ---- round 0: |X|^2 of pair c at row c, |Y|^2 of it at row HALF + c -- the staging order; one lane per bin sums each plane's HALF
  // rows in ascending order
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    const int col = VEC == 2 ? v * CG + cg : cg;
    T* p = pw + col * PS + th;
#pragma unroll
    for (int r = 0; r < 16; ++r) p[Q * r] = x[v][r].re * x[v][r].re + x[v][r].im * x[v][r].im;
    if (th == 0) p[L] = xh[v] * xh[v];
  }
  __syncthreads();
  for (int k = tid; k < L + 1; k += NT) {
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
      T acc = 0;
#pragma unroll
      for (int c = 0; c < HALF; ++c) acc += pw[(pl * HALF + c) * PS + k];
      dst[(CSD_PXX + pl) * (L + 1) + k] = acc;
    }
  }
  __syncthreads();

  // ---- conj(X) Y into the lane that holds X.  f64: the y half passes its bins through the staging area first
  if (VEC == 2) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const cpx<T> X = x[0][r], Y = x[VEC - 1][r];
      x[0][r] = cpx<T>{X.re * Y.re + X.im * Y.im, X.re * Y.im - X.im * Y.re};
    }
    xh[0] = xh[0] * xh[VEC - 1];
  } else {
    if (cg >= HALF) {
      cpx<T>* p = stage + (cg - HALF) * LP + th;
#pragma unroll
      for (int r = 0; r < 16; ++r) p[Q * r] = x[0][r];
      if (th == 0) p[L] = cpx<T>{xh[0], 0};
    }
    __syncthreads();
    if (cg < HALF) {
      const cpx<T>* p = stage + cg * LP + th;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const cpx<T> X = x[0][r], Y = p[Q * r];
        x[0][r] = cpx<T>{X.re * Y.re + X.im * Y.im, X.re * Y.im - X.im * Y.re};
      }
      if (th == 0) xh[0] = xh[0] * p[L].re;
    }
    __syncthreads();
  }

  // ---- round 1: Re of pair c at row c, Im of it at row HALF + c (bin h is real: Im = 0)
  if (VEC == 2 || cg < HALF) {
    T* p = pw + cg * PS + th;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      p[Q * r] = x[0][r].re;
      p[HALF * PS + Q * r] = x[0][r].im;
    }
    if (th == 0) {
      p[L] = xh[0];
      p[HALF * PS + L] = 0;
    }
  }
  __syncthreads();
  for (int k = tid; k < L + 1; k += NT) {
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
      T acc = 0;
#pragma unroll
      for (int c = 0; c < HALF; ++c) acc += pw[(pl * HALF + c) * PS + k];
      dst[(CSD_RE + pl) * (L + 1) + k] = acc;
    }
  }
}

FOURIER_KERNELS_END
