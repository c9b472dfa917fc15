// kernels_resample.h -- device code of the resampling handle (ResamplePlan, resample_plan.h): rows of n values -> rows of m values
// through the spectrum (scipy.signal.resample; the definition is include/fourier.h's).  K = min(n, m), kh = K / 2.
//
// resample_remap_kernel: the spectrum of a row, n values (complex rows) or n / 2 + 1 (half spectra of real rows), -> the spectrum the
// inverse transform takes, m or m / 2 + 1 values, with the window, the rule of the bin kh and 1 / n folded in.  One lane per output
// bin; a lane loads the one input bin it copies (two where m < n folds X[kh] + X[n - kh]) and none where it writes a zero.
//
// resample_untangle_kernel (real rows, n = 2 hn and m = 2 hm both even): ONE sweep between the two inner transforms in place of three
// -- real_post_kernel (kernels_real.h), the remap above, real_pre_kernel with RealPlan::run_inverse's factor and m / n.  Z is the
// hn-point transform of the reals taken as complex values.  One lane per output pair (j, hm - j), j <= hm / 2, computes the two
// half-spectrum bins the pair needs,
//   X[k] = (E + W_n^k O) / 2,  E = Z[k] + conj Z[hn - k],  O = -i (Z[k] - conj Z[hn - k])    (indices mod hn),
// for k = j and k = hm - j, so it reads at most the four values Z[j], Z[hn - j], Z[hm - j], Z[hn - hm + j] -- two where n == m, and
// none for a bin above kh, which is a constant zero and is never loaded.  Y[k] = X[k] win[k] (times nyq at k = kh), and the lane writes
//   Zo[j] = f (S + iT),  Zo[hm - j] = f (conj S + i conj T),  S = Y[j] + conj Y[hm - j],  T = W_m^-j (Y[j] - conj Y[hm - j]),  f = 1 / n,
// the imaginary parts of Y[0] and Y[hm] dropped, whose unscaled hm-point inverse is the m reals of irfft_m(Y) m / n.  The twiddles are
// the two RealPlans' tables W^j, j <= quarter length: a forward bin k above hn / 2 takes W_n^k = -conj(W_n^(hn - k)).
//
// Byte model per f32 row at n = m (a model, not a measurement): the two inner transforms move 8 n bytes each and this sweep 4 n in and
// 4 n out -- 24 n; the composed route's three sweeps move 8 n each -- 40 n; a caller's rfft, slice, scale, irfft about 56 n.
//
// Both sweeps are written like real_post_kernel and hilbert_expand_kernel: one element per access through buffer descriptors with
// non-temporal hints on the streamed sides, plain loads for the twiddle and window tables (shared by every row, they stay in the L2),
// the flat index split by multiply-high, XCD-contiguous workgroups.
#pragma once
#include "kernels_real.h"

FOURIER_KERNELS_BEGIN

template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) resample_remap_kernel(ResampleArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t row = real_div(idx, a.div_m, a.div_l), k = idx - row * a.orow, kh = a.kh;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  const T* win = (const T*)a.win;
  const uint32_t base = row * a.irow;
  const T s = (T)a.scale;
  const bool nyquist = a.even != 0 && k == kh;
  cpx<T> y = {(T)0, (T)0};
  if (a.half) {
    if (k <= kh) {  // 2 k < K, or the bin kh of an even K
      const cpx<T> X = real_load<T>(rin, (base + k) * E);
      T g = win ? win[k] * s : s;
      if (nyquist) g *= (T)a.nyq;
      y = {X.re * g, X.im * g};
    }
  } else {
    const uint32_t d = a.m - k;  // the bin's negative frequency is -d
    uint32_t src = 0xffffffffu;
    T g = s;
    if (nyquist) {
      src = kh;
      if (a.mode == RESAMPLE_UP) g *= (T)0.5;
    } else if (k <= kh) {
      src = k;
    } else if (a.even != 0 && d == kh) {
      if (a.mode == RESAMPLE_UP) { src = kh; g *= (T)0.5; }  // (m < n and m == n: the bin m - kh is the bin kh)
    } else if (d <= kh) {
      src = a.n - d;
    }
    if (src != 0xffffffffu) {
      const cpx<T> X = real_load<T>(rin, (base + src) * E);
      const T g1 = win ? win[src] * g : g;
      y = {X.re * g1, X.im * g1};
      if (nyquist && a.mode == RESAMPLE_DOWN) {  // Y[kh] = X[kh] + X[n - kh]
        const uint32_t s2 = a.n - kh;
        const cpx<T> X2 = real_load<T>(rin, (base + s2) * E);
        const T g2 = win ? win[s2] * g : g;
        y = {y.re + X2.re * g2, y.im + X2.im * g2};
      }
    }
  }
  buf_store_elem<T, BUF_NT>(rout, idx * E, y);
}

// W_n^k, k <= hn, from the table of j <= hn / 2
template <typename T> __device__ __forceinline__ cpx<T> resample_twiddle(const cpx<T>* tw, uint32_t hn, uint32_t k) {
  if (k <= hn / 2) return tw[k];
  const cpx<T> t = tw[hn - k];
  return {-t.re, t.im};
}
// 2 X[k] c from A = Z[k mod hn], P = Z[(hn - k) mod hn], w = W_n^k
template <typename T> __device__ __forceinline__ cpx<T> resample_bin(cpx<T> A, cpx<T> P, cpx<T> w, T c) {
  const cpx<T> e = {A.re + P.re, A.im - P.im};
  const cpx<T> o = {A.im + P.im, P.re - A.re};  // -i (A - conj P)
  const cpx<T> t = cmul(w, o);
  return {c * (e.re + t.re), c * (e.im + t.im)};
}

template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) resample_untangle_kernel(ResampleArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t row = real_div(idx, a.div_m, a.div_l), j = idx - row * a.pairs;
  const uint32_t hn = a.irow, hm = a.orow, kh = a.kh, jb = hm - j;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  const T* win = (const T*)a.win;
  const cpx<T>* twi = (const cpx<T>*)a.tw_in;
  const uint32_t zin = row * hn, zout = row * hm;
  const T c = (T)a.scale * (T)0.5;  // f and the untangle's 1 / 2
  cpx<T> A = {(T)0, (T)0}, P = {(T)0, (T)0};  // Y[j], Y[hm - j]
  cpx<T> za = {(T)0, (T)0}, zp = {(T)0, (T)0};
  if (j <= kh) {
    za = real_load<T>(rin, (zin + (j == hn ? 0 : j)) * E);
    zp = real_load<T>(rin, (zin + (j == 0 ? 0 : hn - j)) * E);
    T g = win ? win[j] * c : c;
    if (j == kh) g *= (T)a.nyq;
    A = resample_bin(za, zp, resample_twiddle(twi, hn, j), g);
  }
  if (jb <= kh) {
    cpx<T> zb = zp, zq = za;  // n == m: Z[hm - j] and Z[hn - hm + j] are the two values above
    if (hn != hm) {
      zb = real_load<T>(rin, (zin + (jb == hn ? 0 : jb)) * E);
      zq = real_load<T>(rin, (zin + hn - jb) * E);
    }
    T g = win ? win[jb] * c : c;
    if (jb == kh) g *= (T)a.nyq;
    P = resample_bin(zb, zq, resample_twiddle(twi, hn, jb), g);
  }
  if (j == 0) { A.im = 0; P.im = 0; }
  const cpx<T> w = ((const cpx<T>*)a.tw_out)[j];
  const cpx<T> sm = {A.re + P.re, A.im - P.im};                        // S = A + conj P
  const cpx<T> d = {A.re - P.re, A.im + P.im};                         // A - conj P
  const cpx<T> t = {w.re * d.re + w.im * d.im, w.re * d.im - w.im * d.re};  // T = conj(w) d
  buf_store_elem<T, BUF_NT>(rout, (zout + j) * E, cpx<T>{sm.re - t.im, sm.im + t.re});
  if (j != 0 && jb != j) buf_store_elem<T, BUF_NT>(rout, (zout + jb) * E, cpx<T>{sm.re + t.im, t.re - sm.im});
}

FOURIER_KERNELS_END
