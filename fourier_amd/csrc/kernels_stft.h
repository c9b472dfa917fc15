// kernels_stft.h -- device code of the short-time Fourier transform (StftPlan, stft_plan.h).
//
// Frame f of a signal row holds xpad[f * hop - pad + n] * win[n], n < n_fft, where xpad is the row with `pad` samples of reflect or
// zero padding on each side -- computed by index arithmetic at the load, there is no padded copy (stft_sample).
//   stft_frame_kernel   composed forward route: gathers, pads and windows the frames of a chunk into rows of n_fft reals, which
//                       RealPlan transforms straight into the caller's frame-major output.
//   istft_ola_kernel    inverse: the overlap-add as a gather over the inverse-transformed frames, one lane per output sample, no
//                       atomics; window and reciprocal envelope are tables.
//   stft_rows_kernel    fused forward route for n_fft = 2h with a whole-row h-point kernel (tile_core in MODE_ROWS, kernels_pass.h): a
//                       workgroup takes COLS consecutive frames of the flat frame index, fills its register tile with the windowed
//                       samples (x[2m], x[2m+1]) as the complex value m, runs the row core, stages Z in LDS half a tile at a time and
//                       untangles on the way out: the lane that stores bin k reads Z[h - k] from LDS (real_post_kernel's formula,
//                       kernels_real.h).  One launch, no scratch: a frame's samples are read hop-strided from the rows (the overlap of
//                       neighbouring frames comes from the L2: consecutive frames stay on one XCD), the h + 1 bins are written once.
#pragma once
#include "kernels_frames.h"

FOURIER_KERNELS_BEGIN

constexpr int STFT_THREADS = 256;

// sample t of the padded row: inside the row as it is, outside mirrored (reflect) or zero
template <typename T> __device__ __forceinline__ T stft_sample(const T* row, int64_t t, int64_t length, uint32_t mode) {
  if (t < 0 || t >= length) {
    if (mode != STFT_PAD_REFLECT) return (T)0;
    t = t < 0 ? -t : 2 * (length - 1) - t;
    if (t < 0 || t >= length) return (T)0;  // (the plan admits length > pad only: one mirror always lands inside)
  }
  return row[t];
}

// item i = blockIdx.x of the launch: one frame per workgroup, its n_fft samples strided over the lanes
template <typename T>
__global__ void __launch_bounds__(STFT_THREADS) stft_frame_kernel(StftArgs a) {
  const uint32_t i = blockIdx.x;
  uint32_t row, f;
  frame_of(a, i, row, f);
  const T* src = (const T*)a.in + (uint64_t)row * a.length;
  const T* win = (const T*)a.win;
  T* dst = (T*)a.out + (uint64_t)i * a.n_fft;
  const int64_t t0 = (int64_t)f * a.hop - (int64_t)a.pad, length = (int64_t)a.length;
  for (uint32_t n = threadIdx.x; n < a.n_fft; n += STFT_THREADS) dst[n] = win[n] * stft_sample(src, t0 + n, length, a.mode);
}

template <typename T>
__global__ void __launch_bounds__(STFT_THREADS) istft_ola_kernel(StftArgs a) {
  const T* fr = (const T*)a.in;
  const T* win = (const T*)a.win;
  const T* env = (const T*)a.env;
  T* out = (T*)a.out;
  const T scale = (T)a.scale;
  for (uint64_t i = (uint64_t)blockIdx.x * STFT_THREADS + threadIdx.x; i < a.total; i += (uint64_t)gridDim.x * STFT_THREADS) {
    const uint64_t r = i / a.span, t = a.t0 + (i - r * a.span), u = t + a.pad;
    const uint64_t f_hi = u / a.hop < (uint64_t)a.frames - 1 ? u / a.hop : (uint64_t)a.frames - 1;
    const uint64_t f_lo = u >= a.n_fft ? (u - a.n_fft) / a.hop + 1 : 0;
    T acc = 0;
    for (uint64_t f = f_lo; f <= f_hi; ++f) {
      const uint64_t n = u - f * a.hop;
      acc += win[n] * fr[(r * a.nfr + (f - a.f_lo)) * a.n_fft + n];
    }
    out[r * a.length + t] = acc * env[t] * scale;
  }
}

// ---- the fused forward route
// Four waves per SIMD asked for outright: the gather's address arithmetic on top of the row core otherwise takes a few registers more than
// 128 at f32 h = 512 and f64 h = 64, 256, 512, and with them a wave of the occupancy the row kernels of the same length have; the price
// is 2 ... 16 spilled registers at those four shapes ("Short-time Fourier transform").
template <typename T, int L, int CG>
__global__ void __launch_bounds__((L / 16) * CG, 4) stft_rows_kernel(StftArgs a) {
  using C = TileCfg<T, L, CG>;
  using S = FrameRowsCfg<T, L, CG>;
  constexpr int VEC = C::VEC, Q = C::Q, COLS = C::COLS, HALF = S::HALF, LP = S::LP;
  static_assert(Q > 1 && COLS % 2 == 0, "stft rows kernel: L >= 32, an even number of frames per tile");
  FOURIER_DYN_SMEM(smem);
  const int tid = (int)threadIdx.x;
  int th = tid % Q, cg = tid / Q;
  // every XCD walks one contiguous range of the flat frame index: the frames that share samples meet in one L2
  const uint32_t blk = real_xcd_block(blockIdx.x, gridDim.x);
  const uint64_t g0 = (uint64_t)blk * COLS;
  const T* __restrict__ in = (const T*)a.in;
  const cpx<T>* __restrict__ win = (const cpx<T>*)a.win + th;  // (w[2m], w[2m+1]) as the complex value m
  const int64_t length = (int64_t)a.length;

  // ---- load: register r <- complex value m = th + Q*r of frame cg*VEC + v
  cpx<T> x[VEC][16];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    const uint64_t g = g0 + (uint64_t)(cg * VEC + v);
    if (g >= a.total) {
#pragma unroll
      for (int r = 0; r < 16; ++r) x[v][r] = cpx<T>{0, 0};
      continue;
    }
    uint32_t row, f;
    frame_of(a, (uint32_t)g, row, f);
    const T* src = in + (uint64_t)row * a.length;
    const int64_t t0 = (int64_t)f * a.hop - (int64_t)a.pad;
    if (t0 >= 0 && t0 + (int64_t)a.n_fft <= length) {
      // an interior frame: no padding index.  Two reals per access where every frame starts on an aligned pair, single reals otherwise
      const T* p = src + t0 + 2 * th;
      if (a.pairs) {
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
        x[v][r] = cpx<T>{stft_sample(src, t, length, a.mode), stft_sample(src, t + 1, length, a.mode)};
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const cpx<T> w = win[Q * r];  // plain loads: the table is shared by every frame and stays in the L2
      x[v][r] = cpx<T>{x[v][r].re * w.re, x[v][r].im * w.im};
    }
  }

  // ---- Z = FFT_h: register r holds Z[k], k = th + Q*r, of frame cg*VEC + v
  tile_core<T, L, CG, MODE_ROWS>(x, th, cg, tid, smem, (const cpx<T>*)a.tw1, (const cpx<T>*)a.tw2);

  // ---- untangle through LDS, half a tile at a time: X[k] = s/2 (E + W_N^k O), E = Z[k] + conj Z[h-k], O = -i (Z[k] - conj Z[h-k]);
  // bins 0 and h both come from Z[0].  W_N^k for k > h/2 is -conj W_N^{h-k}: the table stops at N/4.
  cpx<T>* stage = (cpx<T>*)smem;
  const cpx<T>* tw = (const cpx<T>*)a.tw;
  cpx<T>* __restrict__ out = (cpx<T>*)a.out;
  const T s = (T)a.scale * (T)0.5;
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
      const uint64_t g = g0 + (uint64_t)(cg * VEC + v);
      if (col / HALF == hf && g < a.total) {
        const cpx<T>* z = stage + (col % HALF) * LP;
        cpx<T>* dst = out + g * (uint64_t)(L + 1);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int k = th + Q * r;
          const cpx<T> A = x[v][r], P = z[k == 0 ? 0 : L - k];
          const cpx<T> t1 = tw[k <= L / 2 ? k : L - k];
          const cpx<T> w = k <= L / 2 ? t1 : cpx<T>{-t1.re, t1.im};
          const cpx<T> e = {A.re + P.re, A.im - P.im};
          const cpx<T> o = {A.im + P.im, P.re - A.re};
          const cpx<T> t = cmul(w, o);
          // no streaming hint: rows of h + 1 values are only element-aligned, the L2 merges the line halves of neighbouring frames
          store_elem<T, false>(dst + k, cpx<T>{s * (e.re + t.re), s * (e.im + t.im)});
          if (k == 0) store_elem<T, false>(dst + L, cpx<T>{(T)a.scale * (A.re - A.im), (T)0});
        }
      }
    }
    if (hf == 0) __syncthreads();
  }
}

FOURIER_KERNELS_END
