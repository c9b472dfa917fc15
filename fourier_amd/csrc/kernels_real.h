// kernels_real.h -- device code of the real-input transforms (RealPlan, real_plan.h).
//
// Even N = 2h: the N reals of a row are read as h complex values z[m] = x[2m] + i x[2m+1], the inner h-point plan transforms
// them, and one linear sweep untangles the half spectrum:
//   X[k]     = s/2 * (E + W_N^k O),  X[h - k] = s/2 * conj(E - W_N^k O),  E = Z[k] + conj(Z[h-k]),  O = -i (Z[k] - conj(Z[h-k]))
// (Z[h] = Z[0]; k = 0 gives X[0] = s (Re Z0 + Im Z0), X[h] = s (Re Z0 - Im Z0); k = h / 2, h even, is its own partner).  The
// inverse runs the same algebra backwards, Z[k] = f (S + iT), Z[h-k] = f (conj S + i conj T), S = X[k] + conj(X[h-k]),
// T = W_N^-k (X[k] - conj(X[h-k])), and the inner plan's unscaled IFFT of Z is f h (x[2m] + i x[2m+1]).
//
// real_post_kernel / real_pre_kernel are pure streaming sweeps, written like the pass kernels:
//   * one lane per pair (j, h - j): the partner run h - j descends, so a wave still touches one contiguous run of each side;
//   * one element per access (8 bytes f32, 16 bytes f64), through buffer descriptors with non-temporal hints; elements rather
//     than two-element units because the half-spectrum rows have the odd stride h + 1, whose rows start on any 8-byte boundary
//     in f32 -- with element accesses every row is aligned alike and no lane needs a branch on the row's alignment;
//   * the flat index rows x pairs is split with a multiply-high (no 64-bit division per lane), workgroups are remapped so that
//     each XCD (blockIdx % 8) walks one contiguous range of the index, that is of whole rows;
//   * the twiddle table W_N^j (j <= N/4) is read with plain loads: it is shared by every row and stays in the L2.
// The odd-N kernels (widen, narrow, Hermitian extend, real part) belong to the correctness path and are plain grid-stride loops.
#pragma once
#include "kernels_common.h"

FOURIER_KERNELS_BEGIN

constexpr int REAL_THREADS = 256;

// workgroup blk of nwg -> index such that XCD x = blk % 8 owns the x-th contiguous eighth of the grid
__device__ __forceinline__ uint32_t real_xcd_block(uint32_t blk, uint32_t nwg) {
  const uint32_t xcd = blk % 8u, slot = blk / 8u, q = nwg / 8u, r = nwg % 8u;
  return (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + slot;
}
__device__ __forceinline__ uint32_t real_div(uint32_t x, uint32_t m, uint32_t l) {
  const uint32_t hi = (uint32_t)(((uint64_t)x * m) >> 32);
  return (uint32_t)(((uint64_t)hi + x) >> l);
}
template <typename T> __device__ __forceinline__ cpx<T> real_load(BufRsrc r, uint32_t voff) {
  cpx<T> y;
  if constexpr (sizeof(T) == 4) {
    const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, 0, BUF_NT);
    __builtin_memcpy(&y, &v, 8);
  } else {
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, 0, BUF_NT);
    __builtin_memcpy(&y, &v, 16);
  }
  return y;
}

// scratch Z (rows of h) -> half spectrum X (rows of h + 1)
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) real_post_kernel(RealArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t row = real_div(idx, a.div_m, a.div_l), j = idx - row * a.pairs, h = a.h;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  const uint32_t zrow = row * h, xrow = zrow + row;  // row * (h + 1)
  const cpx<T> A = real_load<T>(rin, (zrow + j) * E);
  const cpx<T> P = real_load<T>(rin, (zrow + (j == 0 ? 0 : h - j)) * E);
  const cpx<T> w = ((const cpx<T>*)a.tw)[j];
  const cpx<T> e = {A.re + P.re, A.im - P.im};
  const cpx<T> o = {A.im + P.im, P.re - A.re};  // -i (A - conj P)
  const cpx<T> t = cmul(w, o);
  const T s = (T)a.scale * (T)0.5;
  buf_store_elem<T, BUF_NT>(rout, (xrow + j) * E, cpx<T>{s * (e.re + t.re), s * (e.im + t.im)});
  if (h - j != j) buf_store_elem<T, BUF_NT>(rout, (xrow + h - j) * E, cpx<T>{s * (e.re - t.re), s * (t.im - e.im)});
}

// half spectrum X (rows of h + 1) -> scratch Z (rows of h); the imaginary parts of X[0] and X[h] are ignored
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) real_pre_kernel(RealArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t row = real_div(idx, a.div_m, a.div_l), j = idx - row * a.pairs, h = a.h;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  const uint32_t zrow = row * h, xrow = zrow + row;
  cpx<T> A = real_load<T>(rin, (xrow + j) * E);
  cpx<T> P = real_load<T>(rin, (xrow + h - j) * E);
  if (j == 0) { A.im = 0; P.im = 0; }
  const cpx<T> w = ((const cpx<T>*)a.tw)[j];
  const cpx<T> sm = {A.re + P.re, A.im - P.im};                        // S = A + conj P
  const cpx<T> d = {A.re - P.re, A.im + P.im};                         // A - conj P
  const cpx<T> t = {w.re * d.re + w.im * d.im, w.re * d.im - w.im * d.re};  // T = conj(w) d
  const T f = (T)a.scale;
  buf_store_elem<T, BUF_NT>(rout, (zrow + j) * E, cpx<T>{f * (sm.re - t.im), f * (sm.im + t.re)});
  if (j != 0 && h - j != j) buf_store_elem<T, BUF_NT>(rout, (zrow + h - j) * E, cpx<T>{f * (sm.re + t.im), f * (t.re - sm.im)});
}

// ---- odd N: the full-length complex transform on a widened copy
// x (rows of n reals) -> work (rows of n complex, imaginary parts 0)
template <typename T>
__global__ void __launch_bounds__(256) real_widen_kernel(RealArgs a) {
  const T* x = (const T*)a.in;
  cpx<T>* w = (cpx<T>*)a.out;
  const uint64_t total = a.rows * a.n;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) w[i] = {x[i], (T)0};
}
// work (rows of n) -> X (rows of n / 2 + 1): the first n / 2 + 1 values of every row
template <typename T>
__global__ void __launch_bounds__(256) real_narrow_kernel(RealArgs a) {
  const cpx<T>* w = (const cpx<T>*)a.in;
  cpx<T>* X = (cpx<T>*)a.out;
  const uint64_t hp = a.n / 2 + 1, total = a.rows * hp;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    const uint64_t b = i / hp, k = i - b * hp;
    X[i] = w[b * a.n + k];
  }
}
// X (rows of n / 2 + 1) -> work (rows of n): the Hermitian extension, Im X[0] ignored
template <typename T>
__global__ void __launch_bounds__(256) real_extend_kernel(RealArgs a) {
  const cpx<T>* X = (const cpx<T>*)a.in;
  cpx<T>* w = (cpx<T>*)a.out;
  const uint64_t hp = a.n / 2 + 1, total = a.rows * a.n;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    const uint64_t b = i / a.n, k = i - b * a.n;
    cpx<T> y;
    if (k == 0) y = {X[b * hp].re, (T)0};
    else if (k < hp) y = X[b * hp + k];
    else { const cpx<T> v = X[b * hp + (a.n - k)]; y = {v.re, -v.im}; }
    w[i] = y;
  }
}
// work (rows of n complex) -> x (rows of n reals)
template <typename T>
__global__ void __launch_bounds__(256) real_part_kernel(RealArgs a) {
  const cpx<T>* w = (const cpx<T>*)a.in;
  T* x = (T*)a.out;
  const uint64_t total = a.rows * a.n;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) x[i] = w[i].re;
}

FOURIER_KERNELS_END
