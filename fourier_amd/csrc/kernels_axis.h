// kernels_axis.h -- device code of the transforms along a strided axis (AxisRoute, axis_plan.h): a length-N transform down the
// middle axis of an [outer][N][inner] array, element (o, j, c) at (o*N + j)*inner + c.
//
// axis_lane_kernel<T, N> (N <= 32): one lane owns one column (o, c) and holds its N elements in registers.  Adjacent lanes are adjacent
// columns, so every load and store instruction of a wave covers 64 consecutive elements of one row j; no LDS, no shuffles.  The DFT
// is dft_any (kernels_regtile.h) for the lengths whose prime factors stop at 13 and a direct transform with compile-time roots for
// the primes 17 ... 31.  Inverse = swap . DFT . swap, the scale on the store, as every final pass does.
//
// axis_transpose_kernel<T>: 32 x 32 tiles of a row-major matrix into its transpose, through LDS.  A tile row is 256 bytes (f32) /
// 512 bytes (f64) on both global sides: whole 128-byte segments.  The LDS tile has a leading dimension of 33 elements: under the
// bank model of MI355X_MICROARCH.md (and the emulator's) the row-wise writes and the column-wise reads are both conflict-free
// (f32 read: lane tx at dword 66 tx mod 64 = 2 tx; f64 read: 132 tx mod 64 = 4 tx over each 16-lane group).  Buffer descriptors
// with 32-bit byte offsets (the plan bounds a launch's range on either side), streaming hints, ragged edges masked on the global
// side only (every lane does its LDS accesses).
#pragma once
#include "kernels_real.h"
#include "kernels_regtile.h"

FOURIER_KERNELS_BEGIN

constexpr int AXIS_THREADS = 256;
constexpr int AXIS_TILE = 32, AXIS_LD = 33;  // transpose tile side, LDS leading dimension (elements)

template <typename T> __device__ __forceinline__ cpx<T> axis_load(const cpx<T>* p) {
#ifndef FOURIER_EMU
  typedef T v2 __attribute__((ext_vector_type(2)));
  const v2 v = __builtin_nontemporal_load((const v2*)p);
  return {v.x, v.y};
#else
  return *p;
#endif
}

// forward DFT of a prime R in registers: X[k], X[R-k] = x0 + sum_q a_q cos(2 pi qk / R) -/+ i sum_q d_q sin(2 pi qk / R),
// a_q = x_q + x_{R-q}, d_q = x_q - x_{R-q} (the form of dft_prime, kernels_mixed.h, on root_tab's compile-time roots)
template <typename T, int R> __device__ __forceinline__ void axis_dft_prime(cpx<T>* x) {
  constexpr RootTab<R> tab = root_tab<R>();
  constexpr int H = (R - 1) / 2;
  cpx<T> a[H], d[H];
  cpx<T> y0 = x[0];
#pragma unroll
  for (int q = 1; q <= H; ++q) {
    a[q - 1] = {x[q].re + x[R - q].re, x[q].im + x[R - q].im};
    d[q - 1] = {x[q].re - x[R - q].re, x[q].im - x[R - q].im};
    y0 = {y0.re + a[q - 1].re, y0.im + a[q - 1].im};
  }
  const cpx<T> x0 = x[0];
#pragma unroll
  for (int k = 1; k <= H; ++k) {
    cpx<T> m = x0, n = {(T)0, (T)0};
#pragma unroll
    for (int q = 1; q <= H; ++q) {
      const T c = (T)tab.c[(k * q) % R], s = (T)tab.s[(k * q) % R];
      m = {m.re + c * a[q - 1].re, m.im + c * a[q - 1].im};
      n = {n.re + s * d[q - 1].re, n.im + s * d[q - 1].im};
    }
    x[k] = {m.re + n.im, m.im - n.re};  // m - i n
    x[R - k] = {m.re - n.im, m.im + n.re};
  }
  x[0] = y0;
}

template <typename T, int N> __device__ __forceinline__ void axis_dft(cpx<T>* x) {
  if constexpr (N == 17 || N == 19 || N == 23 || N == 29 || N == 31) axis_dft_prime<T, N>(x);
  else dft_any<T, N>(x);
}

template <typename T, int N>
__global__ void __launch_bounds__(AXIS_THREADS) axis_lane_kernel(AxisArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * AXIS_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t o = real_div(idx, a.div_m, a.div_l);
  const uint64_t off = (uint64_t)o * a.block + (idx - o * a.cols);
  const cpx<T>* in = (const cpx<T>*)a.in + off;
  cpx<T>* out = (cpx<T>*)a.out + off;
  cpx<T> x[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const cpx<T> v = axis_load(in + (uint64_t)j * a.inner);
    x[j] = a.swap ? cpx<T>{v.im, v.re} : v;
  }
  axis_dft<T, N>(x);
  const T s = (T)a.scale;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    cpx<T> y = x[k];
    if (a.swap) y = {y.im, y.re};
    store_elem<T, true>(out + (uint64_t)k * a.inner, cpx<T>{y.re * s, y.im * s});
  }
}

// block b of the launch: source rows x cols at in + b * bs_in (leading dimension ld_in) -> cols x rows at out + b * bs_out
template <typename T>
__global__ void __launch_bounds__(AXIS_THREADS) axis_transpose_kernel(AxisArgs a) {
  FOURIER_DYN_SMEM(smem);
  constexpr uint32_t E = sizeof(cpx<T>);
  const uint32_t blk = real_xcd_block(blockIdx.x, gridDim.x);
  const uint32_t per = a.tiles_r * a.tiles_c, b = blk / per, rem = blk - b * per, tr = rem / a.tiles_c, tc = rem - tr * a.tiles_c;
  const uint32_t tx = threadIdx.x % AXIS_TILE, ty = threadIdx.x / AXIS_TILE;
  constexpr uint32_t STEP = AXIS_THREADS / AXIS_TILE;
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  cpx<T>* tile = (cpx<T>*)smem;
  cpx<T> v[AXIS_TILE / STEP];
  {
    const uint32_t c = tc * AXIS_TILE + tx;
    const uint64_t base = (uint64_t)b * a.bs_in + c;
#pragma unroll
    for (uint32_t i = 0; i < AXIS_TILE / STEP; ++i) {
      const uint32_t r = tr * AXIS_TILE + ty + STEP * i;
      v[i] = (r < a.rows && c < a.cols) ? real_load<T>(rin, (uint32_t)((base + (uint64_t)r * a.ld_in) * E)) : cpx<T>{(T)0, (T)0};
    }
  }
#pragma unroll
  for (uint32_t i = 0; i < AXIS_TILE / STEP; ++i) {
    cpx<T>* p = tile + (ty + STEP * i) * AXIS_LD + tx;
    LDS_NOTE(p, E, true, 400);
    *p = v[i];
  }
  __syncthreads();
  const uint32_t r = tr * AXIS_TILE + tx;  // source row = output column
  const uint64_t base = (uint64_t)b * a.bs_out + r;
#pragma unroll
  for (uint32_t i = 0; i < AXIS_TILE / STEP; ++i) {
    const cpx<T>* p = tile + tx * AXIS_LD + ty + STEP * i;
    LDS_NOTE(p, E, false, 401);
    const cpx<T> w = *p;
    const uint32_t c = tc * AXIS_TILE + ty + STEP * i;  // source column = output row
    if (r < a.rows && c < a.cols) buf_store_elem<T, BUF_NT>(rout, (uint32_t)((base + (uint64_t)c * a.ld_out) * E), w);
  }
}

FOURIER_KERNELS_END
