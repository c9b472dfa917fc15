// kernels_r2r.h -- device code of the real-to-real transforms (R2RPlan, r2r_plan.h): DCT-II / DCT-III / DST-II / DST-III, scipy's
// definitions, rows of N reals in and out.
//
// DCT-II of x is a real N-point FFT of the permuted row v (v[j] = x[2j], v[N-1-j] = x[2j+1]) followed by one twiddle:
//   X[k] = 2 Re(c_k V[k]),  X[N-k] = -2 Im(c_k V[k]),  c_k = exp(-i pi k / 2N),  V = FFT_N(v)
// and DCT-III runs it backwards: V[k] = conj(c_k) (X[k] - i X[N-k]) / 2 (X[N] := 0), v = 2 UIFFT_N(V).  For even N = 2h the real FFT
// is the half-length complex one of kernels_real.h, z[m] = v[2m] + i v[2m+1], so that
//   r2r_pack_kernel    x -> z: lane m < h / 2 reads the four consecutive reals x[4m .. 4m+3] and writes z[m] = (x[4m], x[4m+2]),
//                      z[h-1-m] = (x[4m+3], x[4m+1]); the middle lane of an odd h has x[4m], x[4m+1] -> z[m] only
//   r2r_post_kernel    Z -> X: real_post_kernel's lane per pair (j, h - j) and its algebra for V[j], V[h-j], then c_j, c_{h-j} and the
//                      four reals X[j], X[N-j], X[h-j], X[h+j] (j = 0: X[0], X[h]; 2j = h: X[j], X[N-j])
//   r2r_pre_kernel     X -> Z: the four reals -> V[j], V[h-j] -> real_pre_kernel's algebra (the inner plan's UNSCALED_IFFT follows)
//   r2r_unpack_kernel  z -> x: the pack's inverse
// The norm's factor and the orthogonalised form's edge term (on the transform side's element 0) are folded into post and pre.
// A DST is the same four sweeps with a uniform flag: DST-II(x)[k] = DCT-II((-1)^n x[n])[N-1-k], DST-III(X)[n] = (-1)^n
// DCT-III(X reversed)[n] -- a sign on the odd-indexed reals in pack / unpack, a reversed index in post / pre.
//
// The sweeps are written like kernels_real.h's: buffer descriptors with non-temporal hints, the flat index rows x lanes split by a
// multiply-high, real_xcd_block so that each XCD walks whole rows, 32-bit byte offsets, the tables (W_N^j and c_j, shared by every
// row) read with plain loads.  pack / unpack move 16-byte units (f64: two of them) that need dword alignment only, so rows that
// start on any 8-byte boundary (f32, N % 4 == 2) take the same path as every other row.  post / pre move single reals: a wave stores
// (loads) four runs of reals, two ascending and two descending, 256 bytes each in f32.  Pairing neighbouring lanes' reals into 8-byte
// accesses would need a cross-lane exchange and a second case per run (the descending runs pair at odd indices); element accesses
// keep every row and every lane alike.
// The odd-N kernels belong to the correctness path (the N-point complex plan on a widened copy) and are plain grid-stride loops.
#pragma once
#include "kernels_real.h"

FOURIER_KERNELS_BEGIN

// four consecutive reals (f32: one 16-byte unit, f64: two) and single reals through a descriptor, bounds-checked like the units
template <typename T> __device__ __forceinline__ void r2r_load4(BufRsrc r, uint32_t voff, T* v) {
  if constexpr (sizeof(T) == 4) {
    const auto u = __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, 0, BUF_NT);
    __builtin_memcpy(v, &u, 16);
  } else {
    const auto u0 = __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, 0, BUF_NT);
    const auto u1 = __builtin_amdgcn_raw_buffer_load_b128(r, (int)(voff + 16u), 0, BUF_NT);
    __builtin_memcpy(v, &u0, 16);
    __builtin_memcpy(v + 2, &u1, 16);
  }
}
template <typename T> __device__ __forceinline__ void r2r_store2(BufRsrc r, uint32_t voff, T a, T b) {
  buf_store_elem<T, BUF_NT>(r, voff, cpx<T>{a, b});
}
template <typename T> __device__ __forceinline__ void r2r_store4(BufRsrc r, uint32_t voff, const T* v) {
  if constexpr (sizeof(T) == 4) {
    decltype(__builtin_amdgcn_raw_buffer_load_b128(r, 0, 0, 0)) u;
    __builtin_memcpy(&u, v, 16);
    __builtin_amdgcn_raw_buffer_store_b128(u, r, (int)voff, 0, BUF_NT);
  } else {
    r2r_store2<T>(r, voff, v[0], v[1]);
    r2r_store2<T>(r, voff + 16u, v[2], v[3]);
  }
}
template <typename T> __device__ __forceinline__ T r2r_load_real(BufRsrc r, uint32_t voff) {
  T y;
#ifdef FOURIER_EMU
  y = 0;
  if ((uint64_t)voff + sizeof(T) <= r.num_records) __builtin_memcpy(&y, r.base + voff, sizeof(T));
#else
  if constexpr (sizeof(T) == 4) {
    const auto v = __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, 0, BUF_NT);
    __builtin_memcpy(&y, &v, 4);
  } else {
    const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, 0, BUF_NT);
    __builtin_memcpy(&y, &v, 8);
  }
#endif
  return y;
}
template <typename T> __device__ __forceinline__ void r2r_store_real(BufRsrc r, uint32_t voff, T y) {
#ifdef FOURIER_EMU
  if ((uint64_t)voff + sizeof(T) <= r.num_records) __builtin_memcpy(r.base + voff, &y, sizeof(T));
#else
  if constexpr (sizeof(T) == 4) {
    decltype(__builtin_amdgcn_raw_buffer_load_b32(r, 0, 0, 0)) v;
    __builtin_memcpy(&v, &y, 4);
    __builtin_amdgcn_raw_buffer_store_b32(v, r, (int)voff, 0, BUF_NT);
  } else {
    decltype(__builtin_amdgcn_raw_buffer_load_b64(r, 0, 0, 0)) v;
    __builtin_memcpy(&v, &y, 8);
    __builtin_amdgcn_raw_buffer_store_b64(v, r, (int)voff, 0, BUF_NT);
  }
#endif
}

// byte offset of element i of the cosine transform: element i (DCT) or N-1-i (DST) of the row of reals that starts at xrow
template <typename T> __device__ __forceinline__ uint32_t r2r_at(uint32_t xrow, uint32_t i, uint32_t last, int sine) {
  return (xrow + (sine ? last - i : i)) * (uint32_t)sizeof(T);
}

// x (rows of N = 2h reals) -> z (rows of h complex values)
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) r2r_pack_kernel(R2RArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t row = real_div(idx, a.div_m, a.div_l), m = idx - row * a.lanes, h = a.h;
  constexpr uint32_t E = sizeof(cpx<T>), R = sizeof(T);
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  const uint32_t zrow = row * h;
  T v[4];
  r2r_load4<T>(rin, (2u * zrow + 4u * m) * R, v);  // the middle lane of an odd h reads two reals of the next row (or zeros) and drops them
  if (a.sine) { v[1] = -v[1]; v[3] = -v[3]; }
  if (2u * m + 1u == h) {
    buf_store_elem<T, BUF_NT>(rout, (zrow + m) * E, cpx<T>{v[0], v[1]});
  } else {
    buf_store_elem<T, BUF_NT>(rout, (zrow + m) * E, cpx<T>{v[0], v[2]});
    buf_store_elem<T, BUF_NT>(rout, (zrow + h - 1u - m) * E, cpx<T>{v[3], v[1]});
  }
}

// z (rows of h complex values) -> x (rows of N = 2h reals)
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) r2r_unpack_kernel(R2RArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t row = real_div(idx, a.div_m, a.div_l), m = idx - row * a.lanes, h = a.h;
  constexpr uint32_t E = sizeof(cpx<T>), R = sizeof(T);
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  const uint32_t zrow = row * h, xoff = (2u * zrow + 4u * m) * R;
  const T sg = a.sine ? (T)-1 : (T)1;
  const cpx<T> A = real_load<T>(rin, (zrow + m) * E);
  if (2u * m + 1u == h) {
    r2r_store2<T>(rout, xoff, A.re, sg * A.im);
  } else {
    const cpx<T> B = real_load<T>(rin, (zrow + h - 1u - m) * E);
    const T v[4] = {A.re, sg * B.im, A.im, sg * B.re};
    r2r_store4<T>(rout, xoff, v);
  }
}

// scratch Z (rows of h) -> X (rows of N reals)
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) r2r_post_kernel(R2RArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t row = real_div(idx, a.div_m, a.div_l), j = idx - row * a.lanes, h = a.h, n = 2u * h;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  const uint32_t zrow = row * h, xrow = 2u * zrow;
  const cpx<T> A = real_load<T>(rin, (zrow + j) * E);
  const cpx<T> P = real_load<T>(rin, (zrow + (j == 0 ? 0 : h - j)) * E);
  const cpx<T> w = ((const cpx<T>*)a.tw)[j];
  const cpx<T> cj = ((const cpx<T>*)a.ct)[j], ch = ((const cpx<T>*)a.ct)[h - j];
  const cpx<T> e = {A.re + P.re, A.im - P.im};
  const cpx<T> o = {A.im + P.im, P.re - A.re};  // -i (A - conj P)
  const cpx<T> t = cmul(w, o);
  const cpx<T> vj = {e.re + t.re, e.im + t.im}, vh = {e.re - t.re, t.im - e.im};  // 2 V[j], 2 V[h-j]
  const cpx<T> pj = cmul(cj, vj), ph = cmul(ch, vh);
  const T s = (T)a.scale;
  const uint32_t last = n - 1u;
  r2r_store_real<T>(rout, r2r_at<T>(xrow, j, last, a.sine), j == 0 ? s * (T)a.edge * pj.re : s * pj.re);
  if (j != 0) r2r_store_real<T>(rout, r2r_at<T>(xrow, n - j, last, a.sine), -s * pj.im);
  if (h - j != j) {
    r2r_store_real<T>(rout, r2r_at<T>(xrow, h - j, last, a.sine), s * ph.re);
    if (j != 0) r2r_store_real<T>(rout, r2r_at<T>(xrow, h + j, last, a.sine), -s * ph.im);
  }
}

// X (rows of N reals) -> scratch Z (rows of h)
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) r2r_pre_kernel(R2RArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t row = real_div(idx, a.div_m, a.div_l), j = idx - row * a.lanes, h = a.h, n = 2u * h;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  const uint32_t zrow = row * h, xrow = 2u * zrow;
  const uint32_t last = n - 1u;
  T x0 = r2r_load_real<T>(rin, r2r_at<T>(xrow, j, last, a.sine));
  const T x1 = j != 0 ? r2r_load_real<T>(rin, r2r_at<T>(xrow, n - j, last, a.sine)) : (T)0;  // X[N] := 0
  const T x2 = r2r_load_real<T>(rin, r2r_at<T>(xrow, h - j, last, a.sine));
  const T x3 = r2r_load_real<T>(rin, r2r_at<T>(xrow, h + j, last, a.sine));
  if (j == 0) x0 *= (T)a.edge;
  const cpx<T> w = ((const cpx<T>*)a.tw)[j];
  const cpx<T> cj = ((const cpx<T>*)a.ct)[j], ch = ((const cpx<T>*)a.ct)[h - j];
  // 2 V[k] = conj(c_k) (X[k] - i X[N-k])
  cpx<T> A = {cj.re * x0 - cj.im * x1, -cj.re * x1 - cj.im * x0};
  cpx<T> P = {ch.re * x2 - ch.im * x3, -ch.re * x3 - ch.im * x2};
  if (j == 0) { A.im = 0; P.im = 0; }  // V[0] and V[h] are real
  const cpx<T> sm = {A.re + P.re, A.im - P.im};                        // S = A + conj P
  const cpx<T> d = {A.re - P.re, A.im + P.im};                         // A - conj P
  const cpx<T> t = {w.re * d.re + w.im * d.im, w.re * d.im - w.im * d.re};  // T = conj(w) d
  const T f = (T)a.scale;
  buf_store_elem<T, BUF_NT>(rout, (zrow + j) * E, cpx<T>{f * (sm.re - t.im), f * (sm.im + t.re)});
  if (j != 0 && h - j != j) buf_store_elem<T, BUF_NT>(rout, (zrow + h - j) * E, cpx<T>{f * (sm.re + t.im), f * (t.re - sm.im)});
}

// ---- odd N: the full-length complex transform on a widened, permuted copy
// position i of v holds x[2i] (i < (n + 1) / 2) or x[2 (n - 1 - i) + 1]
__device__ __forceinline__ uint64_t r2r_source(uint64_t i, uint64_t n) { return i < (n + 1) / 2 ? 2 * i : 2 * (n - 1 - i) + 1; }

// x (rows of n reals) -> work (rows of n complex, imaginary parts 0)
template <typename T>
__global__ void __launch_bounds__(256) r2r_odd_widen_kernel(R2RArgs a) {
  const T* x = (const T*)a.in;
  cpx<T>* w = (cpx<T>*)a.out;
  const uint64_t total = a.rows * a.n;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    const uint64_t b = i / a.n, src = r2r_source(i - b * a.n, a.n);
    const T v = x[b * a.n + src];
    w[i] = {(a.sine && (src & 1)) ? -v : v, (T)0};
  }
}
// work V (rows of n) -> X (rows of n reals): X[k] = 2 Re(c_k V[k])
template <typename T>
__global__ void __launch_bounds__(256) r2r_odd_post_kernel(R2RArgs a) {
  const cpx<T>* w = (const cpx<T>*)a.in;
  T* X = (T*)a.out;
  const uint64_t total = a.rows * a.n;
  const T s = (T)2 * (T)a.scale;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    const uint64_t b = i / a.n, k = i - b * a.n;
    const cpx<T> v = w[i], c = ((const cpx<T>*)a.ct)[k];
    const T y = s * (c.re * v.re - c.im * v.im);
    X[b * a.n + (a.sine ? a.n - 1 - k : k)] = k == 0 ? (T)a.edge * y : y;
  }
}
// X (rows of n reals) -> work (rows of n): V[k] = f conj(c_k) (X[k] - i X[n-k]), X[n] := 0 (Hermitian by construction)
template <typename T>
__global__ void __launch_bounds__(256) r2r_odd_pre_kernel(R2RArgs a) {
  const T* X = (const T*)a.in;
  cpx<T>* w = (cpx<T>*)a.out;
  const uint64_t total = a.rows * a.n;
  const T f = (T)a.scale;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    const uint64_t b = i / a.n, k = i - b * a.n, last = a.n - 1;
    const T* row = X + b * a.n;
    const T x0 = k == 0 ? (T)a.edge * row[a.sine ? last : 0] : row[a.sine ? last - k : k];
    const T x1 = k == 0 ? (T)0 : row[a.sine ? last - (a.n - k) : a.n - k];
    const cpx<T> c = ((const cpx<T>*)a.ct)[k];
    w[i] = {f * (c.re * x0 - c.im * x1), f * (-c.re * x1 - c.im * x0)};
  }
}
// work (rows of n complex) -> x (rows of n reals): the real parts, unpermuted
template <typename T>
__global__ void __launch_bounds__(256) r2r_odd_part_kernel(R2RArgs a) {
  const cpx<T>* w = (const cpx<T>*)a.in;
  T* x = (T*)a.out;
  const uint64_t total = a.rows * a.n;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    const uint64_t b = i / a.n, src = r2r_source(i - b * a.n, a.n);
    const T v = w[i].re;
    x[b * a.n + src] = (a.sine && (src & 1)) ? -v : v;
  }
}

FOURIER_KERNELS_END
