// kernels_nufft2d.h -- device code of the 2-D non-uniform FFT handle (Nufft2dPlan, nufft2d_plan.h): types 1 and 2 with m points
// (x1, x2) shared by the items of a batch, on a fine grid of l1 x l2 cells (C order, axis 2 contiguous) and the 1-D handle's kernel phi
// of width w per axis (kernels_nufft.h): the weight of a point on cell (i1, i2) is the product of its two 1-D weights.
// The host (Nufft2dPlan::set_points) forms per point and axis the first cell i0 = ceil(g - w/2) and the offset d = i0 - g, buckets the
// points by r1 = i0_1 mod l1 and sorts each bucket by g_2 (stable), and uploads per SORTED point p r1[p], i02[p], d1[p], d2[p] and the
// caller's index perm[p].  first[r][e + w], e in [-w, l2 + w], is the global sorted index of the first point of bucket r with
// i0_2 >= e: l1 (l2 + 2w + 1) uint32, about a quarter of one f32 grid item (an eighth of an f64 one).
//
// nufft2d_spread_kernel<T, RB> (type 1, step 1) is a GATHER: one lane owns one cell (i1, i2) for RB consecutive items.  The points
// that reach row i1 through axis-1 tap t have r1 = (i1 - t) mod l1; l1 >= 2w makes these w buckets distinct, and the lane visits them
// for t = 0 .. w - 1.  Inside a bucket the points that reach column i2 are three contiguous runs of the bucket, exactly the three
// images i2 - l2, i2, i2 + l2 of nufft_spread_kernel, walked in ascending sorted index.  The lane forms phi_1(d1, t) * phi_2(d2, i2 -
// i0_2) once per point and adds weight * c[item, perm[p]] into one accumulator per item.  No atomics, no LDS, one store a cell: the
// sum's order depends on the points alone, so it is bit-equal on repetition, under any launch split and for any batch.  The width
// is a launch argument, not a template parameter: nothing in the kernel is sized by it (4 instances a precision, one per item block).
// nufft2d_interp_kernel<T, W, RB> (type 2, step 3): one lane owns one sorted point for RB items, holds its W axis-2 weights, forms
// the axis-1 weight inside the outer tap loop (holding both vectors spills at the wide f64 widths), reads its W x W cells with the
// wrap in both axes in ascending taps (axis 1 outer) and stores c[item, perm[p]].  4 (W - 1 widths) instances a precision: 28 / 60.
// Weights: evaluated in the kernel with the accurate exp and sqrt (a.wtab == null), or read from the [2][w][m] table a set-up kernel
// wrote with the same function (nufft2d_table_kernel).
// nufft2d_deconv_kernel / nufft2d_amplify_kernel are the 1-D sweeps over two axes: deconv picks the n1 x n2 modes out of a transformed
// grid item and multiplies by 1 / (phihat_1(|k1|) phihat_2(|k2|)), two 1-D tables; amplify writes f / phihat into a grid item and zeros
// into the rest of it.  Both map the mode index of either axis (order 0: ascending from -floor(n/2); order 1: FFT order) to cell k,
// or l + k for k < 0 (nufft_mode).
#pragma once
#include "kernels_nufft.h"

FOURIER_KERNELS_BEGIN

// the weight of tap t of axis `axis` of sorted point p
template <typename T> __device__ __forceinline__ T nufft2d_tap(const Nufft2dArgs& a, uint32_t p, uint32_t axis, uint32_t t, T inv_half_w, T beta) {
  if (a.wtab) return ((const T*)a.wtab)[((size_t)axis * a.w + t) * a.m + p];
  return nufft_weight<T>(((const T*)(axis ? a.d2 : a.d1))[p], t, inv_half_w, beta);
}

// the item block of this workgroup and its position among the workgroups of that block (XCD-contiguous: real_xcd_block's rule)
__device__ __forceinline__ void nufft2d_block(const Nufft2dArgs& a, uint32_t& ib, uint32_t& seg) {
  const uint32_t blk = real_xcd_block(blockIdx.x, gridDim.x);
  ib = real_div(blk, a.per_m, a.per_l);
  seg = blk - ib * a.per;
}

template <typename T, int RB>
__global__ void __launch_bounds__(REAL_THREADS) nufft2d_spread_kernel(Nufft2dArgs a) {
  uint32_t ib, seg;
  nufft2d_block(a, ib, seg);
  const uint32_t c = seg * REAL_THREADS + threadIdx.x, L1 = a.l1, L2 = a.l2, M = a.m, W = a.w, cells = a.cells;
  if (c >= cells) return;
  const uint32_t i1 = real_div(c, a.l2_m, a.l2_l), i2 = c - i1 * L2;
  constexpr uint32_t E = sizeof(cpx<T>);
  const T inv_half_w = (T)2 / (T)W, beta = (T)a.beta;
  const char* in = (const char*)a.in + (size_t)ib * RB * M * E;
  char* out = (char*)a.out + (size_t)ib * RB * cells * E;
  BufRsrc rin[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) rin[r] = make_rsrc(in + (size_t)r * M * E, M * E);
  cpx<T> acc[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) acc[r] = {(T)0, (T)0};
  const int64_t top = (int64_t)L2 + 2 * (int64_t)W;  // the last index of a row of first[]
  uint32_t bucket = i1;                              // (i1 - t) mod l1
  for (uint32_t t = 0; t < W; ++t) {
    const uint32_t* first = a.first + (size_t)bucket * a.ne2;
    // the images of column i2 in ascending sorted index within the bucket, as in nufft_spread_kernel
#pragma unroll
    for (int img = 0; img < 3; ++img) {
      const int64_t col = (int64_t)i2 + (int64_t)(img - 1) * (int64_t)L2;  // the column as the points see it
      int64_t elo = col + 1, ehi = col + 1 + W;                            // indices into first[]: e = col - W + 1 and col + 1
      elo = elo < 0 ? 0 : elo > top ? top : elo;
      ehi = ehi < 0 ? 0 : ehi > top ? top : ehi;
      if (img != 1 && elo == ehi) continue;
      const uint32_t p0 = first[elo], p1 = first[ehi];
      for (uint32_t p = p0; p < p1; ++p) {
        const uint32_t t2 = (uint32_t)(col - (int64_t)a.i02[p]);  // in [0, W)
        const T wt = nufft2d_tap<T>(a, p, 0, t, inv_half_w, beta) * nufft2d_tap<T>(a, p, 1, t2, inv_half_w, beta);
        const uint32_t src = a.perm[p] * E;
#pragma unroll
        for (int r = 0; r < RB; ++r) {
          const cpx<T> v = buf_load_elem<T>(rin[r], src);
          acc[r].re += wt * v.re;
          acc[r].im += wt * v.im;
        }
      }
    }
    bucket = bucket == 0 ? L1 - 1u : bucket - 1u;
  }
#pragma unroll
  for (int r = 0; r < RB; ++r) buf_store_elem<T, BUF_NT>(make_rsrc(out + (size_t)r * cells * E, cells * E), c * E, acc[r]);
}

template <typename T, int W, int RB>
__global__ void __launch_bounds__(REAL_THREADS) nufft2d_interp_kernel(Nufft2dArgs a) {
  uint32_t ib, seg;
  nufft2d_block(a, ib, seg);
  const uint32_t p = seg * REAL_THREADS + threadIdx.x, L1 = a.l1, L2 = a.l2, M = a.m, cells = a.cells;
  if (p >= M) return;
  constexpr uint32_t E = sizeof(cpx<T>);
  const T inv_half_w = (T)2 / (T)W, beta = (T)a.beta;
  const char* in = (const char*)a.in + (size_t)ib * RB * cells * E;
  char* out = (char*)a.out + (size_t)ib * RB * M * E;
  T w2[W];
#pragma unroll
  for (int t = 0; t < W; ++t) w2[t] = nufft2d_tap<T>(a, p, 1, (uint32_t)t, inv_half_w, beta);
  BufRsrc rin[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) rin[r] = make_rsrc(in + (size_t)r * cells * E, cells * E);
  cpx<T> acc[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) acc[r] = {(T)0, (T)0};
  const int32_t i02 = a.i02[p];  // in [-W, l2)
  const uint32_t col0 = i02 < 0 ? (uint32_t)(i02 + (int32_t)L2) : (uint32_t)i02;
  uint32_t row = a.r1[p];
#pragma unroll 1
  for (uint32_t t1 = 0; t1 < (uint32_t)W; ++t1) {
    const T w1 = nufft2d_tap<T>(a, p, 0, t1, inv_half_w, beta);
    const uint32_t base = row * L2;
    uint32_t col = col0;
#pragma unroll
    for (int t2 = 0; t2 < W; ++t2) {
      const T wt = w1 * w2[t2];
      const uint32_t off = (base + col) * E;
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const cpx<T> v = buf_load_elem<T>(rin[r], off);
        acc[r].re += wt * v.re;
        acc[r].im += wt * v.im;
      }
      col = col + 1u == L2 ? 0u : col + 1u;
    }
    row = row + 1u == L1 ? 0u : row + 1u;
  }
  const uint32_t dst = a.perm[p] * E;
#pragma unroll
  for (int r = 0; r < RB; ++r) buf_store_elem<T>(make_rsrc(out + (size_t)r * M * E, M * E), dst, acc[r]);
}

// the [2][w][m] table of the tabulated route: one lane per sorted point
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) nufft2d_table_kernel(Nufft2dArgs a) {
  const T inv_half_w = (T)2 / (T)a.w, beta = (T)a.beta;
  for (size_t p = (size_t)blockIdx.x * REAL_THREADS + threadIdx.x; p < a.m; p += (size_t)gridDim.x * REAL_THREADS) {
    const T d1 = ((const T*)a.d1)[p], d2 = ((const T*)a.d2)[p];
    for (uint32_t t = 0; t < a.w; ++t) {
      ((T*)a.out)[(size_t)t * a.m + p] = nufft_weight<T>(d1, t, inv_half_w, beta);
      ((T*)a.out)[((size_t)a.w + t) * a.m + p] = nufft_weight<T>(d2, t, inv_half_w, beta);
    }
  }
}

// transformed grid items of l1 x l2 -> items of n1 x n2 modes: out[item, j1, j2] = grid[item, cell(k1), cell(k2)] / (phihat_1 phihat_2)
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) nufft2d_deconv_kernel(Nufft2dArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t item = real_div(idx, a.item_m, a.item_l), rem = idx - item * (a.n1 * a.n2);
  const uint32_t j1 = real_div(rem, a.row_m, a.row_l), j2 = rem - j1 * a.n2;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  uint32_t mag1, mag2;
  bool neg1, neg2;
  nufft_mode(j1, a.n1, a.order, mag1, neg1);
  nufft_mode(j2, a.n2, a.order, mag2, neg2);
  const uint32_t cell1 = neg1 ? a.l1 - mag1 : mag1, cell2 = neg2 ? a.l2 - mag2 : mag2;
  const T s = ((const T*)a.inv1)[mag1] * ((const T*)a.inv2)[mag2];
  const cpx<T> v = real_load<T>(rin, (item * a.cells + cell1 * a.l2 + cell2) * E);
  buf_store_elem<T, BUF_NT>(rout, idx * E, cpx<T>{v.re * s, v.im * s});
}

// the position of the mode that cell g of an axis of l cells holds (n modes on that axis), and |k|; false where the cell holds none
__device__ __forceinline__ bool nufft2d_cell_mode(uint32_t g, uint32_t l, uint32_t n, uint32_t order, uint32_t& j, uint32_t& mag) {
  const uint32_t lo = n / 2u, hi = n - lo;
  const bool pos = g < hi, neg = g >= l - lo;  // l >= 2 n: never both
  if (!pos && !neg) return false;
  mag = pos ? g : l - g;
  if (order == 0) j = pos ? lo + mag : lo - mag;
  else j = pos ? mag : n - mag;
  return true;
}

// items of n1 x n2 modes -> grid items of l1 x l2: grid[item, cell(k1), cell(k2)] = f[item, j(k1), j(k2)] / phihat, zeros elsewhere
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) nufft2d_amplify_kernel(Nufft2dArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t item = real_div(idx, a.item_m, a.item_l), rem = idx - item * a.cells;
  const uint32_t g1 = real_div(rem, a.row_m, a.row_l), g2 = rem - g1 * a.l2;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  cpx<T> y = {(T)0, (T)0};
  uint32_t j1, j2, mag1, mag2;
  if (nufft2d_cell_mode(g1, a.l1, a.n1, a.order, j1, mag1) && nufft2d_cell_mode(g2, a.l2, a.n2, a.order, j2, mag2)) {
    const T s = ((const T*)a.inv1)[mag1] * ((const T*)a.inv2)[mag2];
    const cpx<T> v = real_load<T>(rin, (item * (a.n1 * a.n2) + j1 * a.n2 + j2) * E);
    y = {v.re * s, v.im * s};
  }
  buf_store_elem<T, BUF_NT>(rout, idx * E, y);
}

FOURIER_KERNELS_END
