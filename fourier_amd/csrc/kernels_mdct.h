// kernels_mdct.h -- device code of the modified discrete cosine transform (MdctPlan, mdct_plan.h).
//
// Frame f of a signal row holds xw[m] = win[m] * xpad[f * n - pad + m], m < 2n, where xpad is the row with zeros on both sides --
// computed by index arithmetic at the load, there is no padded copy (mdct_sample).  Even n = 2h: the frame folds to n reals
//   u[i] = -xw[3h - 1 - i] - xw[3h + i]  (i < h),   u[i] = xw[i - h] - xw[3h - 1 - i]  (i >= h),
// the MDCT is the DCT-IV of u, and that is an h-point complex FFT between two twiddles:
//   z[j] = (u[2j] + i u[n - 1 - 2j]) A[j],  Z = FFT_h z,  t = Z[j] B[j],  X[2j] = Re t,  X[n - 1 - 2j] = -Im t,
// A[j] = exp(-i pi (4j + 1) / 4n), B[j] = exp(-i pi j / n).  The DCT-IV is its own inverse up to scale, so the inverse runs the same
// three steps on X and unfolds: Y[m] = v[m + h] (m < h), -v[3h - 1 - m] (h <= m < 3h), -v[m - 3h] (m >= 3h), v = DCT-IV(X).
//   mdct_fold_kernel / mdct_post_kernel     composed forward route around the inner h-point plan
//   imdct_pre_kernel / imdct_ola_kernel     composed inverse: the overlap-add is a gather, one lane per output sample, over the at most
//                                           two frames that cover it (post-twiddle, unfold, window, sum, scale); no atomics
//   mdct_odd_* / imdct_odd_*                odd n: the 2n-point complex plan on xw[m] D[m], X[k] = Re(C[k] Z[k]), D[m] = exp(-i pi m / 2n),
//                                           C[k] = exp(-i pi (n + 1)(2k + 1) / 4n); the inverse is Y[m] = Re(D[m] FFT_2n(X C, n zeros)[m])
//   mdct_rows_kernel    fused forward route for n = 2h with a whole-row h-point kernel (tile_core in MODE_ROWS, kernels_pass.h): a
//                       workgroup takes COLS consecutive frames of the flat frame index; a lane forms its z[j] from the four samples and
//                       four window values it needs, the row core runs, the post-twiddled outputs go through LDS (even coefficients
//                       ascending, odd ones descending) so that every store instruction writes one contiguous run of the frame.
#pragma once
#include "kernels_frames.h"

FOURIER_KERNELS_BEGIN

constexpr int MDCT_THREADS = 256;

// windowed sample m of the frame that starts at padded-row index t0: zero outside the row
template <typename T> __device__ __forceinline__ T mdct_sample(const T* row, const T* win, int64_t t0, uint32_t m, int64_t length) {
  const int64_t t = t0 + (int64_t)m;
  return t >= 0 && t < length ? win[m] * row[t] : (T)0;
}

// z[j] before the pre-twiddle, h = n / 2 (any parity of h); EDGE: the frame reaches outside the row
template <typename T, bool EDGE>
__device__ __forceinline__ cpx<T> mdct_fold(const T* row, const T* win, int64_t t0, int64_t length, uint32_t h, uint32_t j) {
  uint32_t i0, i1, i2, i3;
  const bool lo = 2 * j < h;
  if (lo) { i0 = 3 * h - 1 - 2 * j; i1 = 3 * h + 2 * j; i2 = h - 1 - 2 * j; i3 = h + 2 * j; }
  else { i0 = 2 * j - h; i1 = 3 * h - 1 - 2 * j; i2 = h + 2 * j; i3 = 5 * h - 1 - 2 * j; }
  T s0, s1, s2, s3;
  if (EDGE) {
    s0 = mdct_sample(row, win, t0, i0, length); s1 = mdct_sample(row, win, t0, i1, length);
    s2 = mdct_sample(row, win, t0, i2, length); s3 = mdct_sample(row, win, t0, i3, length);
  } else {
    const T* p = row + t0;
    s0 = win[i0] * p[i0]; s1 = win[i1] * p[i1]; s2 = win[i2] * p[i2]; s3 = win[i3] * p[i3];
  }
  return lo ? cpx<T>{-s0 - s1, s2 - s3} : cpx<T>{s0 - s1, -s2 - s3};
}

// the frame of item i = blockIdx.x: its row and its first index in the padded row
template <typename T> __device__ __forceinline__ const T* mdct_frame(const MdctArgs& a, uint32_t i, int64_t& t0) {
  uint32_t row, f;
  frame_of(a, i, row, f);
  t0 = (int64_t)f * a.n - (int64_t)a.pad;
  return (const T*)a.in + (uint64_t)row * a.length;
}

// ---- even n: one frame per workgroup, its h complex values strided over the lanes
template <typename T>
__global__ void __launch_bounds__(MDCT_THREADS) mdct_fold_kernel(MdctArgs a) {
  const uint32_t i = blockIdx.x, h = a.n / 2;
  int64_t t0;
  const T* src = mdct_frame<T>(a, i, t0);
  const T* win = (const T*)a.win;
  const cpx<T>* A = (const cpx<T>*)a.twa;
  cpx<T>* dst = (cpx<T>*)a.out + (uint64_t)i * h;
  const int64_t length = (int64_t)a.length;
  if (t0 >= 0 && t0 + 2 * (int64_t)a.n <= length)
    for (uint32_t j = threadIdx.x; j < h; j += MDCT_THREADS) dst[j] = cmul(mdct_fold<T, false>(src, win, t0, length, h, j), A[j]);
  else
    for (uint32_t j = threadIdx.x; j < h; j += MDCT_THREADS) dst[j] = cmul(mdct_fold<T, true>(src, win, t0, length, h, j), A[j]);
}

// lane j writes the neighbours X[2j] = Re t_j and X[2j + 1] = X[n - 1 - 2 (h - 1 - j)] = -Im t_{h-1-j}
template <typename T>
__global__ void __launch_bounds__(MDCT_THREADS) mdct_post_kernel(MdctArgs a) {
  const uint32_t i = blockIdx.x, h = a.n / 2;
  const cpx<T>* Z = (const cpx<T>*)a.in + (uint64_t)i * h;
  const cpx<T>* B = (const cpx<T>*)a.twb;
  T* dst = (T*)a.out + (uint64_t)i * a.n;
  const T s = (T)a.scale;
  for (uint32_t j = threadIdx.x; j < h; j += MDCT_THREADS) {
    const cpx<T> t = cmul(Z[j], B[j]), m = cmul(Z[h - 1 - j], B[h - 1 - j]);
    dst[2 * j] = s * t.re;
    dst[2 * j + 1] = -s * m.im;
  }
}

template <typename T>
__global__ void __launch_bounds__(MDCT_THREADS) imdct_pre_kernel(MdctArgs a) {
  const uint32_t i = blockIdx.x, h = a.n / 2;
  const T* X = (const T*)a.in + (uint64_t)i * a.n;
  const cpx<T>* A = (const cpx<T>*)a.twa;
  cpx<T>* dst = (cpx<T>*)a.out + (uint64_t)i * h;
  for (uint32_t j = threadIdx.x; j < h; j += MDCT_THREADS) dst[j] = cmul(cpx<T>{X[2 * j], X[a.n - 1 - 2 * j]}, A[j]);
}

template <typename T>
__global__ void __launch_bounds__(MDCT_THREADS) imdct_ola_kernel(MdctArgs a) {
  const cpx<T>* fr = (const cpx<T>*)a.in;
  const T* win = (const T*)a.win;
  const cpx<T>* B = (const cpx<T>*)a.twb;
  T* out = (T*)a.out;
  const T scale = (T)a.scale;
  const uint64_t n = a.n, h = n / 2;
  for (uint64_t i = (uint64_t)blockIdx.x * MDCT_THREADS + threadIdx.x; i < a.total; i += (uint64_t)gridDim.x * MDCT_THREADS) {
    const uint64_t r = i / a.span, t = a.t0 + (i - r * a.span), u = t + a.pad, q = u / n;
    const uint64_t f_hi = q < (uint64_t)a.frames - 1 ? q : (uint64_t)a.frames - 1;
    const uint64_t f_lo = q >= 2 ? q - 1 : 0;
    T acc = 0;
    for (uint64_t f = f_lo; f <= f_hi; ++f) {
      const uint64_t m = u - f * n;  // < 2n
      const uint64_t e = m < h ? m + h : m < 3 * h ? 3 * h - 1 - m : m - 3 * h;  // Y[m] = +- v[e]
      const uint64_t j = e % 2 == 0 ? e / 2 : (n - 1 - e) / 2;
      const cpx<T> tv = cmul(fr[(r * a.nfr + (f - a.f_lo)) * h + j], B[j]);
      const T v = e % 2 == 0 ? tv.re : -tv.im;
      acc += win[m] * (m < h ? v : -v);
    }
    out[r * a.length + t] = acc * scale;
  }
}

// ---- odd n: frames of 2n complex values
template <typename T>
__global__ void __launch_bounds__(MDCT_THREADS) mdct_odd_pre_kernel(MdctArgs a) {
  const uint32_t i = blockIdx.x;
  int64_t t0;
  const T* src = mdct_frame<T>(a, i, t0);
  const T* win = (const T*)a.win;
  const cpx<T>* D = (const cpx<T>*)a.twa;
  cpx<T>* dst = (cpx<T>*)a.out + (uint64_t)i * 2 * a.n;
  for (uint32_t m = threadIdx.x; m < 2 * a.n; m += MDCT_THREADS) {
    const T s = mdct_sample(src, win, t0, m, (int64_t)a.length);
    dst[m] = cpx<T>{s * D[m].re, s * D[m].im};
  }
}

template <typename T>
__global__ void __launch_bounds__(MDCT_THREADS) mdct_odd_post_kernel(MdctArgs a) {
  const uint32_t i = blockIdx.x;
  const cpx<T>* Z = (const cpx<T>*)a.in + (uint64_t)i * 2 * a.n;
  const cpx<T>* C = (const cpx<T>*)a.twb;
  T* dst = (T*)a.out + (uint64_t)i * a.n;
  const T s = (T)a.scale;
  for (uint32_t k = threadIdx.x; k < a.n; k += MDCT_THREADS) dst[k] = s * cmul(C[k], Z[k]).re;
}

template <typename T>
__global__ void __launch_bounds__(MDCT_THREADS) imdct_odd_pre_kernel(MdctArgs a) {
  const uint32_t i = blockIdx.x;
  const T* X = (const T*)a.in + (uint64_t)i * a.n;
  const cpx<T>* C = (const cpx<T>*)a.twb;
  cpx<T>* dst = (cpx<T>*)a.out + (uint64_t)i * 2 * a.n;
  for (uint32_t k = threadIdx.x; k < 2 * a.n; k += MDCT_THREADS)
    dst[k] = k < a.n ? cpx<T>{X[k] * C[k].re, X[k] * C[k].im} : cpx<T>{0, 0};
}

template <typename T>
__global__ void __launch_bounds__(MDCT_THREADS) imdct_odd_ola_kernel(MdctArgs a) {
  const cpx<T>* fr = (const cpx<T>*)a.in;
  const T* win = (const T*)a.win;
  const cpx<T>* D = (const cpx<T>*)a.twa;
  T* out = (T*)a.out;
  const T scale = (T)a.scale;
  const uint64_t n = a.n;
  for (uint64_t i = (uint64_t)blockIdx.x * MDCT_THREADS + threadIdx.x; i < a.total; i += (uint64_t)gridDim.x * MDCT_THREADS) {
    const uint64_t r = i / a.span, t = a.t0 + (i - r * a.span), u = t + a.pad, q = u / n;
    const uint64_t f_hi = q < (uint64_t)a.frames - 1 ? q : (uint64_t)a.frames - 1;
    const uint64_t f_lo = q >= 2 ? q - 1 : 0;
    T acc = 0;
    for (uint64_t f = f_lo; f <= f_hi; ++f) {
      const uint64_t m = u - f * n;
      acc += win[m] * cmul(fr[(r * a.nfr + (f - a.f_lo)) * 2 * n + m], D[m]).re;
    }
    out[r * a.length + t] = acc * scale;
  }
}

// ---- the fused forward route.  The staging area and the frame locator are the frame family's (kernels_frames.h); the half-tile staging
// loop stays spelled out here: routed through a shared skeleton with put / get functors, the kernel's spills moved at every shape.
// Four waves per SIMD asked for outright, as stft_rows_kernel does and for its reason: the fold's address arithmetic sits on top of the row
// core ("Modified discrete cosine transform", lists the registers and spills of every instantiation).
template <typename T, int L, int CG>
__global__ void __launch_bounds__((L / 16) * CG, 4) mdct_rows_kernel(MdctArgs a) {
  using C = TileCfg<T, L, CG>;
  constexpr int VEC = C::VEC, Q = C::Q, COLS = C::COLS, HALF = FrameRowsCfg<T, L, CG>::HALF, LP = FrameRowsCfg<T, L, CG>::LP;
  static_assert(Q > 1 && COLS % 2 == 0, "mdct rows kernel: L >= 32, an even number of frames per tile");
  FOURIER_DYN_SMEM(smem);
  const int tid = (int)threadIdx.x;
  int th = tid % Q, cg = tid / Q;
  // every XCD walks one contiguous range of the flat frame index: the two frames that read a sample meet in one L2
  const uint64_t g0 = (uint64_t)real_xcd_block(blockIdx.x, gridDim.x) * COLS;
  const T* __restrict__ in = (const T*)a.in;
  const T* __restrict__ win = (const T*)a.win;
  const cpx<T>* __restrict__ A = (const cpx<T>*)a.twa + th;
  const int64_t length = (int64_t)a.length;

  // ---- load: register r <- z[j], j = th + Q*r, of frame cg*VEC + v.  Registers r < 8 hold j < L / 2, the others j >= L / 2: per
  // register a lane reads two ascending and two descending runs of every second sample, and the two halves of the registers take the
  // two parities of every quarter of the frame, so each line is fetched once per frame.
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
    const int64_t t0 = (int64_t)f * (2 * L) - (int64_t)a.pad;
    if (t0 >= 0 && t0 + 4 * L <= length) {
#pragma unroll
      for (int r = 0; r < 16; ++r) x[v][r] = mdct_fold<T, false>(src, win, t0, length, (uint32_t)L, (uint32_t)(th + Q * r));
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) x[v][r] = mdct_fold<T, true>(src, win, t0, length, (uint32_t)L, (uint32_t)(th + Q * r));
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) x[v][r] = cmul(x[v][r], A[Q * r]);  // plain loads: the tables are shared by every frame and stay in the L2
  }

  // ---- Z = FFT_h: register r holds Z[k], k = th + Q*r, of frame cg*VEC + v
  tile_core<T, L, CG, MODE_ROWS>(x, th, cg, tid, smem, (const cpx<T>*)a.tw1, (const cpx<T>*)a.tw2);

  // ---- t = Z[k] B[k]; X[2k] = s Re t ascending, X[n - 1 - 2k] = -s Im t descending, through LDS as the frame's n reals, half a tile at
  // a time; the lanes of a frame then store its reals as L pairs in order
  T* stage = (T*)smem;
  const cpx<T>* __restrict__ B = (const cpx<T>*)a.twb + th;
  T* __restrict__ out = (T*)a.out;
  const T s = (T)a.scale;
#pragma unroll
  for (int v = 0; v < VEC; ++v)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const cpx<T> t = cmul(x[v][r], B[Q * r]);
      x[v][r] = cpx<T>{s * t.re, -s * t.im};
    }
  __syncthreads();  // the last exchange's readers are done with the buffer
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const int col = VEC == 2 ? v * CG + cg : cg;  // position in the staging order: each half one run of HALF frames
      if (col / HALF == hf) {
        T* p = stage + (col % HALF) * (2 * LP);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int k = th + Q * r;
          p[2 * k] = x[v][r].re;
          p[2 * L - 1 - 2 * k] = x[v][r].im;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const int col = VEC == 2 ? v * CG + cg : cg;
      const uint64_t g = g0 + (uint64_t)(cg * VEC + v);
      if (col / HALF == hf && g < a.total) {
        const cpx<T>* z = (const cpx<T>*)(stage + (col % HALF) * (2 * LP)) + th;
        T* dst = out + g * (uint64_t)(2 * L) + 2 * th;
        if (a.pairs) {
#pragma unroll
          for (int r = 0; r < 16; ++r) store_elem<T, false>((cpx<T>*)(dst + 2 * Q * r), z[Q * r]);
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const cpx<T> y = z[Q * r];
            dst[2 * Q * r] = y.re;
            dst[2 * Q * r + 1] = y.im;
          }
        }
      }
    }
    if (hf == 0) __syncthreads();
  }
}

FOURIER_KERNELS_END
