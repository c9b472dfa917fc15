// kernels_convnd.h -- device code of the N-D convolution handle (ConvNdPlan, convnd_plan.h).
//
// realnd_conv_mid_kernel: the middle of a real-data convolution over the trailing dimensions [n_1, ..., n_{r-1}, W], W = 2h, between the
// forward transforms of the packed rows Z (the h-point row plan, then the axis transforms) and their unscaled inverses.  It is the
// N-D form of real_conv_mid_kernel (kernels_conv.h) on the workgroups and rows of realnd_post_kernel (kernels_real.h): one workgroup
// per row r and segment of lanes, r' the mirror row, workgroups of r > r' return; one lane per k <= h / 2
//   1. loads Z[r, k], Z[r, h - k], Z[r', k], Z[r', h - k] and untangles them as realnd_post_kernel does with scale 1 into the four
//      half-spectrum values X[r, k], X[r', h - k], X[r', k], X[r, h - k];
//   2. multiplies them by H[r, k], H[r', h - k], H[r', k], H[r, h - k] of the item's filter (first + item) mod F;
//   3. retangles as realnd_pre_kernel does with scale 1, that kernel's projection of columns 0 and h included, and stores to the four
//      places it read.
// One read and one write of the packed rows replace the untangle sweep, the product sweep, the retangle sweep and their half-spectrum
// intermediates.  In place is safe because a lane owns all four elements; the lane of k = 0 also takes k = h / 2 (h even), whose two
// elements are nobody else's.  On a self-mirrored row (r == r') the pairing is the 1-D one, and its columns 0 and h, the bins that
// are their own mirror, are real: they are multiplied by the real part of H (numpy's irfftn drops the imaginary parts there).
// Row bases are 64-bit and workgroup-uniform, offsets within a row 32-bit.  The data goes through buffer descriptors with non-temporal
// hints like the other sweeps; the bank and the twiddles are read with plain loads: with one filter the bank is shared by every item.
//
// convnd_pad_kernel / convnd_crop_kernel: the window copies around the transforms, written like lconv_copy_kernel (kernels_conv.h): one
// workgroup per LCONV_SEG words of a destination line, a lane walks its segment with stride 256 so that a wave moves whole lines,
// 64-bit line addresses.  The pad sweep zero-fills what lies outside the source item.
#pragma once
#include "kernels_conv.h"

FOURIER_KERNELS_BEGIN

template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) realnd_conv_mid_kernel(ConvNdArgs a) {
  uint32_t seg;
  RealNdRows rw;
  if (!realnd_rows(a.r, seg, rw)) return;
  const uint32_t j0 = seg * blockDim.x + threadIdx.x, h = a.r.h;
  if (j0 >= a.r.lanes) return;
  constexpr uint32_t E = sizeof(cpx<T>);
  const bool self = rw.r == rw.m;
  // the item of this row (rows of a launch are counted from its base and stay below 2^31), its filter, the rows within the item
  const uint32_t item = real_div((uint32_t)rw.r, a.r.row_m, a.r.row_l);
  const uint32_t fr = a.first + item, f = fr - real_div(fr, a.f_m, a.f_l) * a.filters;
  const uint64_t base = (uint64_t)item * a.r.nd_rows;
  const cpx<T>* H = (const cpx<T>*)a.bank + (uint64_t)f * a.r.nd_rows * (h + 1);
  const cpx<T>* hr = H + (rw.r - base) * (h + 1);
  const cpx<T>* hm = H + (rw.m - base) * (h + 1);
  cpx<T>* z = (cpx<T>*)a.r.out;
  const BufRsrc zr = make_rsrc(z + rw.r * h, h * E), zm = make_rsrc(z + rw.m * h, h * E);
  for (uint32_t pass = 0; pass < 2; ++pass) {
    const uint32_t j = pass == 0 ? j0 : h / 2;  // pass 1: the lane of k = 0 also takes k = h / 2 (h even)
    if (pass == 1 && !(j0 == 0 && h % 2 == 0 && h >= 2)) break;
    const uint32_t jm = j == 0 ? 0 : h - j;
    const bool mid = 2 * j == h;
    const cpx<T> w = ((const cpx<T>*)a.r.tw)[j];
    // 1. untangle (realnd_post_kernel, scale 1): (r, k) from Z[r, k], Z[r', h - k]; (r', k) from Z[r', k], Z[r, h - k]
    const cpx<T> A = real_load<T>(zr, j * E), P = real_load<T>(zm, jm * E);
    cpx<T> C = A, D = P;
    if (!self) { C = real_load<T>(zm, j * E); D = real_load<T>(zr, jm * E); }
    cpx<T> xa, xp, xc, xd;  // X[r, k], X[r', h - k], X[r', k], X[r, h - k]
    {
      const cpx<T> e = {A.re + P.re, A.im - P.im};
      const cpx<T> o = {A.im + P.im, P.re - A.re};  // -i (A - conj P)
      const cpx<T> t = cmul(w, o);
      xa = {(T)0.5 * (e.re + t.re), (T)0.5 * (e.im + t.im)};
      xp = {(T)0.5 * (e.re - t.re), (T)0.5 * (t.im - e.im)};
    }
    {
      const cpx<T> e = {C.re + D.re, C.im - D.im};
      const cpx<T> o = {C.im + D.im, D.re - C.re};
      const cpx<T> t = cmul(w, o);
      xc = {(T)0.5 * (e.re + t.re), (T)0.5 * (e.im + t.im)};
      xd = {(T)0.5 * (e.re - t.re), (T)0.5 * (t.im - e.im)};
    }
    // 2. the product with the item's filter; the bins that are their own mirror are real
    const cpx<T> ha = hr[j], hp = hm[h - j], hc = hm[j], hd = hr[h - j];
    cpx<T> ya = cmul(xa, ha), yp = cmul(xp, hp), yc = cmul(xc, hc), yd = cmul(xd, hd);
    if (self && j == 0) { ya = {xa.re * ha.re, (T)0}; yp = {xp.re * hp.re, (T)0}; yc = ya; yd = yp; }
    if (mid) { yp = yc; yd = ya; }  // column h / 2: (r', h - k) is (r', k), (r, h - k) is (r, k)
    // 3. retangle (realnd_pre_kernel, scale 1); first its projection of columns 0 and h over the leading axes
    if (j == 0) {
      const cpx<T> a0 = {(ya.re + yc.re) * (T)0.5, (ya.im - yc.im) * (T)0.5}, ah = {(yd.re + yp.re) * (T)0.5, (yd.im - yp.im) * (T)0.5};
      ya = a0; yc = {a0.re, -a0.im};
      yd = ah; yp = {ah.re, -ah.im};
    }
    const bool two = j != 0 && !mid;  // (r', h - k) and (r, h - k) are other elements
    {
      const cpx<T> sm = {ya.re + yp.re, ya.im - yp.im};
      const cpx<T> d = {ya.re - yp.re, ya.im + yp.im};
      const cpx<T> t = {w.re * d.re + w.im * d.im, w.re * d.im - w.im * d.re};
      buf_store_elem<T, BUF_NT>(zr, j * E, cpx<T>{sm.re - t.im, sm.im + t.re});
      if (two) buf_store_elem<T, BUF_NT>(zm, (h - j) * E, cpx<T>{sm.re + t.im, t.re - sm.im});
    }
    if (!self) {
      const cpx<T> sm = {yc.re + yd.re, yc.im - yd.im};
      const cpx<T> d = {yc.re - yd.re, yc.im + yd.im};
      const cpx<T> t = {w.re * d.re + w.im * d.im, w.re * d.im - w.im * d.re};
      buf_store_elem<T, BUF_NT>(zm, j * E, cpx<T>{sm.re - t.im, sm.im + t.re});
      if (two) buf_store_elem<T, BUF_NT>(zr, (h - j) * E, cpx<T>{sm.re + t.im, t.re - sm.im});
    }
  }
}

// The product sweep of the composed route where conv_mul_kernel's 32-bit flat index cannot hold an item: X[b][r][k] *= H[f][r][k] in
// place on half spectra (items of rows x (h + 1)), one workgroup per row and segment of REAL_THREADS columns, 64-bit row bases.
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) convnd_mul_kernel(ConvNdArgs a) {
  const uint32_t blk = real_xcd_block(blockIdx.x, gridDim.x);
  const uint32_t row = real_div(blk, a.seg_m, a.seg_l), seg = blk - row * a.segs;
  const uint32_t item = real_div(row, a.line_m, a.line_l), r = row - item * a.dlines;
  const uint32_t fr = a.first + item, f = fr - real_div(fr, a.f_m, a.f_l) * a.filters;
  const uint32_t k = seg * REAL_THREADS + threadIdx.x, cols = (uint32_t)a.dw;
  if (k >= cols) return;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc rz = make_rsrc((cpx<T>*)a.dst + (uint64_t)row * cols, cols * E);
  const cpx<T> w = ((const cpx<T>*)a.bank)[((uint64_t)f * a.dlines + r) * cols + k];
  buf_store_elem<T, BUF_NT>(rz, k * E, cmul(real_load<T>(rz, k * E), w));
}

// the window copy of both sweeps; ZERO: the source window may end before the destination line does, or miss it (the pad sweep)
template <typename T, bool ZERO>
__device__ __forceinline__ void convnd_window_copy(const ConvNdArgs& a) {
  const uint32_t blk = real_xcd_block(blockIdx.x, gridDim.x);
  const uint32_t line = real_div(blk, a.seg_m, a.seg_l), seg = blk - line * a.segs;
  const uint32_t item = real_div(line, a.line_m, a.line_l), l = line - item * a.dlines;
  const uint32_t q = real_div(l, a.c_m, a.c_l), ic = l - q * a.dl[2];
  const uint32_t ia = real_div(q, a.b_m, a.b_l), ib = q - ia * a.dl[1];
  const uint32_t sa = ia + a.off[0], sb = ib + a.off[1], sc = ic + a.off[2];
  const bool inside = !ZERO || (sa < a.sl[0] && sb < a.sl[1] && sc < a.sl[2]);
  const uint64_t sline = (uint64_t)item * a.slines + ((uint64_t)sa * a.sl[1] + sb) * a.sl[2] + sc;
  const T* x = (const T*)a.src + (inside ? sline : 0) * a.sw + a.offw;
  T* y = (T*)a.dst + (uint64_t)line * a.dw;
  const uint64_t avail = !inside ? 0 : ZERO ? a.sw - a.offw : a.dw;  // words of the source line from offw on
  const uint64_t k0 = (uint64_t)seg * LCONV_SEG + threadIdx.x;
#pragma unroll
  for (uint32_t u = 0; u < LCONV_SEG / REAL_THREADS; ++u) {
    const uint64_t k = k0 + u * REAL_THREADS;
    if (k < a.dw) y[k] = k < avail ? x[k] : (T)0;
  }
}

// the caller's items of in_shape -> the scratch's items of the transform shape, zero-extended at the high end of every dimension
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) convnd_pad_kernel(ConvNdArgs a) {
  convnd_window_copy<T, true>(a);
}
// the window [out_first, out_first + out_shape) of the scratch's items -> the caller's items of out_shape
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) convnd_crop_kernel(ConvNdArgs a) {
  convnd_window_copy<T, false>(a);
}

FOURIER_KERNELS_END
