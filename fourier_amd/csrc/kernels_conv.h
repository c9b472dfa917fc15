// kernels_conv.h -- device code of the convolution handles' sweeps (ConvPlan, conv_plan.h; LinearConvPlan, lconv_plan.h).
//
// conv_mul_kernel: the pointwise product of a batch of spectra with a filter bank, Z[b][k] *= H[(first + b) mod F][k], in place.
// real_conv_mid_kernel: the middle of a real-data convolution of even length N = 2h, between the inner h-point plan's forward
// transform Z and its unscaled inverse.  One lane per mirrored pair (j, h - j) untangles the half spectrum as real_post_kernel does,
//   X[j] = (E + W_N^j O) / 2,  X[h - j] = conj(E - W_N^j O) / 2,  E = Z[j] + conj Z[h-j],  O = -i (Z[j] - conj Z[h-j]),
// multiplies by H[f][j] and H[f][h - j], and retangles as real_pre_kernel does,
//   Z'[j] = S + iT,  Z'[h - j] = conj S + i conj T,  S = Y[j] + conj Y[h-j],  T = W_N^-j (Y[j] - conj Y[h-j]),
// storing to the two places it read: one read and one write of h complex values per row instead of the three sweeps (untangle,
// multiply, retangle) and their half-spectrum intermediates.  In place is safe because a lane owns both elements it writes.
// j = 0 carries X[0] and X[h], both real: they are multiplied by the real parts of H[0] and H[h] (numpy's irfft drops the
// imaginary parts of those two bins); j = h / 2 (h even) is its own partner.
//
// Both are written like the real sweeps (kernels_real.h): one element per access through buffer descriptors with non-temporal
// hints on the data, the flat index rows x lanes split by multiply-high, workgroups remapped so that every XCD walks one contiguous
// range.  The bank and the twiddles are read with plain loads: with one filter they are shared by every row and stay in the L2.
// A row's filter is (first + row) mod F, by the same multiply-high divider.
#pragma once
#include "kernels_real.h"

FOURIER_KERNELS_BEGIN

template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) conv_mul_kernel(ConvArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t row = real_div(idx, a.div_m, a.div_l), k = idx - row * a.len;
  const uint32_t fr = a.first + row, f = fr - real_div(fr, a.f_m, a.f_l) * a.filters;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc rz = make_rsrc(a.out, a.bytes);
  const cpx<T> z = real_load<T>(rz, idx * E);
  const cpx<T> w = ((const cpx<T>*)a.bank)[(uint64_t)f * a.len + k];
  buf_store_elem<T, BUF_NT>(rz, idx * E, cmul(z, w));
}

template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) real_conv_mid_kernel(ConvArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t row = real_div(idx, a.div_m, a.div_l), j = idx - row * a.len, h = a.h;
  const uint32_t fr = a.first + row, f = fr - real_div(fr, a.f_m, a.f_l) * a.filters;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc rz = make_rsrc(a.out, a.bytes);
  const uint32_t zrow = row * h, jp = j == 0 ? 0 : h - j;
  const cpx<T> A = real_load<T>(rz, (zrow + j) * E);
  const cpx<T> P = real_load<T>(rz, (zrow + jp) * E);
  const cpx<T> w = ((const cpx<T>*)a.tw)[j];
  const cpx<T>* H = (const cpx<T>*)a.bank + (uint64_t)f * (h + 1);
  const cpx<T> ha = H[j], hp = H[h - j];
  // untangle (real_post_kernel, scale 1)
  const cpx<T> e = {A.re + P.re, A.im - P.im};
  const cpx<T> o = {A.im + P.im, P.re - A.re};  // -i (A - conj P)
  const cpx<T> t = cmul(w, o);
  const cpx<T> xa = {(T)0.5 * (e.re + t.re), (T)0.5 * (e.im + t.im)};  // X[j]
  const cpx<T> xp = {(T)0.5 * (e.re - t.re), (T)0.5 * (t.im - e.im)};  // X[h - j]
  // multiply; bins 0 and h are real
  cpx<T> ya = cmul(xa, ha), yp = cmul(xp, hp);
  if (j == 0) { ya = {xa.re * ha.re, (T)0}; yp = {xp.re * hp.re, (T)0}; }
  // retangle (real_pre_kernel, scale 1)
  const cpx<T> sm = {ya.re + yp.re, ya.im - yp.im};                        // S = Y[j] + conj Y[h-j]
  const cpx<T> d = {ya.re - yp.re, ya.im + yp.im};                         // Y[j] - conj Y[h-j]
  const cpx<T> u = {w.re * d.re + w.im * d.im, w.re * d.im - w.im * d.re};  // T = conj(w) d
  buf_store_elem<T, BUF_NT>(rz, (zrow + j) * E, cpx<T>{sm.re - u.im, sm.im + u.re});
  if (j != 0 && h - j != j) buf_store_elem<T, BUF_NT>(rz, (zrow + h - j) * E, cpx<T>{sm.re + u.im, u.re - sm.im});
}

// ---- set_filters: small kernels off the hot path, plain grid-stride loops
// the transformed taps -> the bank: the inverse's 1/N folded in, conjugated for a correlation
template <typename T>
__global__ void __launch_bounds__(256) conv_finish_kernel(ConvArgs a) {
  cpx<T>* H = (cpx<T>*)a.out;
  const T s = (T)a.scale;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < a.count; i += (uint64_t)gridDim.x * 256) {
    const cpx<T> v = H[i];
    H[i] = {s * v.re, a.conj ? -(s * v.im) : s * v.im};
  }
}
// taps (rows of a.taps words) -> rows of a.n words, zero-extended
template <typename T>
__global__ void __launch_bounds__(256) conv_pad_kernel(ConvArgs a) {
  const T* x = (const T*)a.in;
  T* y = (T*)a.out;
  const uint64_t total = a.rows * a.n;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    const uint64_t r = i / a.n, k = i - r * a.n;
    y[i] = k < a.taps ? x[r * a.taps + k] : (T)0;
  }
}

// ---- the linear-convolution handle (LinearConvPlan, lconv_plan.h)
// The pad and the crop sweep of its padded route: word k of output row r = word skip + k of input row r, zero beyond the input row.
// One workgroup per LCONV_SEG words of an output row (flat index rows x segments, split by multiply-high, XCD-contiguous like the
// other sweeps); a lane walks its segment with stride 256, so a wave moves whole lines.  Rows are addressed with 64-bit indices: their
// lengths are not multiples of anything and a launch is bounded by its grid only.
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) lconv_copy_kernel(ConvArgs a) {
  const uint32_t blk = real_xcd_block(blockIdx.x, gridDim.x);
  const uint32_t row = real_div(blk, a.div_m, a.div_l), seg = blk - row * a.len;
  const T* x = (const T*)a.in + (uint64_t)row * a.taps;
  T* y = (T*)a.out + (uint64_t)row * a.n;
  const uint64_t k0 = (uint64_t)seg * LCONV_SEG + threadIdx.x;
#pragma unroll
  for (uint32_t u = 0; u < LCONV_SEG / REAL_THREADS; ++u) {
    const uint64_t k = k0 + u * REAL_THREADS;
    if (k < a.n) y[k] = a.skip + k < a.taps ? x[a.skip + k] : (T)0;
  }
}
// set_filters: filters of a.taps values -> rows of a.n values, zero-extended; a correlation (conj != 0) takes conj(h[K-1-k]) for h[k]
template <typename T>
__global__ void __launch_bounds__(256) lconv_taps_kernel(ConvArgs a) {
  const uint64_t total = a.rows * a.n;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    const uint64_t r = i / a.n, k = i - r * a.n;
    cpx<T> v = {(T)0, (T)0};
    if (k < a.taps) {
      const uint64_t src = r * a.taps + (a.conj ? a.taps - 1 - k : k);
      if (a.real) v.re = ((const T*)a.in)[src];
      else v = ((const cpx<T>*)a.in)[src];
      if (a.conj) v.im = -v.im;
    }
    if (a.real && !a.widen) ((T*)a.out)[i] = v.re;
    else ((cpx<T>*)a.out)[i] = v;
  }
}

FOURIER_KERNELS_END
