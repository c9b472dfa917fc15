// kernels_nufft3d.h -- device code of the 3-D non-uniform FFT handle (Nufft3dPlan, nufft3d_plan.h): types 1 and 2 with m points
// (x1, x2, x3) shared by the items of a batch, on a fine grid of l1 x l2 x l3 cells (C order, axis 3 contiguous) and the 1-D handle's
// kernel phi of width w per axis (kernels_nufft.h): the weight of a point on cell (i1, i2, i3) is the product of its three 1-D weights,
// formed as (phi_1 phi_2) phi_3 in both hot kernels.
// The host (Nufft3dPlan::set_points) forms per point and axis the first cell i0 = ceil(g - w/2) and the offset d = i0 - g, buckets the
// points by the pair (r1, r2) = (i0_1 mod l1, i0_2 mod l2), bucket index r1 l2 + r2, sorts each bucket by g_3 (stable), and uploads per
// SORTED point p r1[p], r2[p], i03[p], d1[p], d2[p], d3[p] and the caller's index perm[p].  first[bucket][e + w], e in [-w, l3 + w],
// is the global sorted index of the first point of the bucket with i0_3 >= e: l1 l2 (l3 + 2w + 1) uint32, about half of one f32 grid
// item (a quarter of an f64 one).
//
// nufft3d_spread_kernel<T, RB> (type 1, step 1) is a GATHER: one lane owns one cell (i1, i2, i3) for RB consecutive items.  The
// points that reach plane i1 through axis-1 tap t1 and row i2 through axis-2 tap t2 lie in bucket ((i1 - t1) mod l1, (i2 - t2) mod l2);
// l_d >= 2w makes these w x w buckets distinct, and the lane visits them in ascending t1, then ascending t2.  Inside a bucket the
// points that reach column i3 are three contiguous runs of the bucket, the three images i3 - l3, i3, i3 + l3 of nufft_spread_kernel,
// walked in ascending sorted index; an empty outer image is skipped before any load.  The lane forms phi_1(d1, t1) phi_2(d2, t2)
// phi_3(d3, i3 - i0_3) once per point and adds weight * c[item, perm[p]] into one accumulator per item.  No atomics, no LDS, one store
// a cell: the sum's order depends on the points alone, so it is bit-equal on repetition, under any launch split and for any batch.
// The width is a launch argument, not a template parameter: nothing in the kernel is sized by it (4 instances a precision).
// nufft3d_interp_kernel<T, W, RB> (type 2, step 3): one lane owns one sorted point for RB items, holds its W axis-3 weights, forms the
// axis-1 and axis-2 weights inside the two outer tap loops, which are not unrolled (holding all three vectors spills at the wide f64
// widths), reads its W^3 cells with the wrap on all three axes in ascending taps (axis 1 outermost) and stores c[item, perm[p]].
// 4 (W - 1 widths) instances a precision: 28 / 60.
// Weights: evaluated in the kernel with the accurate exp and sqrt (a.wtab == null), or read from the [3][w][m] table a set-up kernel
// wrote with the same function (nufft3d_table_kernel).
// nufft3d_deconv_kernel / nufft3d_amplify_kernel are the 2-D sweeps over three axes: deconv picks the n1 x n2 x n3 modes out of a
// transformed grid item and multiplies by 1 / (phihat_1(|k1|) phihat_2(|k2|) phihat_3(|k3|)), three 1-D tables; amplify writes
// f / phihat into a grid item and zeros into the rest of it.  Both map the mode index of an axis (order 0: ascending from
// -floor(n/2); order 1: FFT order) to cell k, or l + k for k < 0 (nufft_mode).
#pragma once
#include "kernels_nufft.h"

FOURIER_KERNELS_BEGIN

// the weight of tap t of axis `axis` (0, 1, 2) of sorted point p
template <typename T> __device__ __forceinline__ T nufft3d_tap(const Nufft3dArgs& a, uint32_t p, uint32_t axis, uint32_t t, T inv_half_w, T beta) {
  if (a.wtab) return ((const T*)a.wtab)[((size_t)axis * a.w + t) * a.m + p];
  return nufft_weight<T>(((const T*)(axis == 0 ? a.d1 : axis == 1 ? a.d2 : a.d3))[p], t, inv_half_w, beta);
}

// the item block of this workgroup and its position among the workgroups of that block (XCD-contiguous: real_xcd_block's rule)
__device__ __forceinline__ void nufft3d_block(const Nufft3dArgs& a, uint32_t& ib, uint32_t& seg) {
  const uint32_t blk = real_xcd_block(blockIdx.x, gridDim.x);
  ib = real_div(blk, a.per_m, a.per_l);
  seg = blk - ib * a.per;
}

template <typename T, int RB>
__global__ void __launch_bounds__(REAL_THREADS) nufft3d_spread_kernel(Nufft3dArgs a) {
  uint32_t ib, seg;
  nufft3d_block(a, ib, seg);
  const uint32_t c = seg * REAL_THREADS + threadIdx.x, L1 = a.l1, L2 = a.l2, L3 = a.l3, M = a.m, W = a.w, cells = a.cells;
  if (c >= cells) return;
  const uint32_t q = real_div(c, a.l3_m, a.l3_l), i3 = c - q * L3;
  const uint32_t i1 = real_div(q, a.l2_m, a.l2_l), i2 = q - i1 * L2;
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
  // the three images of column i3 as index pairs into a row of first[] (e = col - W + 1 and col + 1, clamped): the same in every bucket
  const int32_t top = (int32_t)L3 + 2 * (int32_t)W;  // the last index of a row of first[]
  uint32_t elo[3], ehi[3];
#pragma unroll
  for (int img = 0; img < 3; ++img) {
    const int32_t col = (int32_t)i3 + (img - 1) * (int32_t)L3;  // the column as the points see it
    const int32_t lo = col + 1, hi = col + 1 + (int32_t)W;
    elo[img] = (uint32_t)(lo < 0 ? 0 : lo > top ? top : lo);
    ehi[img] = (uint32_t)(hi < 0 ? 0 : hi > top ? top : hi);
  }
  uint32_t b1 = i1;  // (i1 - t1) mod l1
  for (uint32_t t1 = 0; t1 < W; ++t1) {
    uint32_t b2 = i2;  // (i2 - t2) mod l2
    for (uint32_t t2 = 0; t2 < W; ++t2) {
      const uint32_t* first = a.first + ((size_t)b1 * L2 + b2) * a.ne3;
#pragma unroll
      for (int img = 0; img < 3; ++img) {
        if (img != 1 && elo[img] == ehi[img]) continue;
        const int32_t col = (int32_t)i3 + (img - 1) * (int32_t)L3;
        const uint32_t p0 = first[elo[img]], p1 = first[ehi[img]];
        for (uint32_t p = p0; p < p1; ++p) {
          const uint32_t t3 = (uint32_t)(col - a.i03[p]);  // in [0, W)
          const T wt = nufft3d_tap<T>(a, p, 0, t1, inv_half_w, beta) * nufft3d_tap<T>(a, p, 1, t2, inv_half_w, beta) *
                       nufft3d_tap<T>(a, p, 2, t3, inv_half_w, beta);
          const uint32_t src = a.perm[p] * E;
#pragma unroll
          for (int r = 0; r < RB; ++r) {
            const cpx<T> v = buf_load_elem<T>(rin[r], src);
            acc[r].re += wt * v.re;
            acc[r].im += wt * v.im;
          }
        }
      }
      b2 = b2 == 0 ? L2 - 1u : b2 - 1u;
    }
    b1 = b1 == 0 ? L1 - 1u : b1 - 1u;
  }
#pragma unroll
  for (int r = 0; r < RB; ++r) buf_store_elem<T, BUF_NT>(make_rsrc(out + (size_t)r * cells * E, cells * E), c * E, acc[r]);
}

template <typename T, int W, int RB>
__global__ void __launch_bounds__(REAL_THREADS) nufft3d_interp_kernel(Nufft3dArgs a) {
  uint32_t ib, seg;
  nufft3d_block(a, ib, seg);
  const uint32_t p = seg * REAL_THREADS + threadIdx.x, L1 = a.l1, L2 = a.l2, L3 = a.l3, M = a.m, cells = a.cells;
  if (p >= M) return;
  constexpr uint32_t E = sizeof(cpx<T>);
  const T inv_half_w = (T)2 / (T)W, beta = (T)a.beta;
  const char* in = (const char*)a.in + (size_t)ib * RB * cells * E;
  char* out = (char*)a.out + (size_t)ib * RB * M * E;
  T w3[W];
#pragma unroll
  for (int t = 0; t < W; ++t) w3[t] = nufft3d_tap<T>(a, p, 2, (uint32_t)t, inv_half_w, beta);
  BufRsrc rin[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) rin[r] = make_rsrc(in + (size_t)r * cells * E, cells * E);
  cpx<T> acc[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) acc[r] = {(T)0, (T)0};
  const int32_t i03 = a.i03[p];  // in [-W, l3)
  const uint32_t col0 = i03 < 0 ? (uint32_t)(i03 + (int32_t)L3) : (uint32_t)i03;
  const uint32_t row0 = a.r2[p];
  uint32_t plane = a.r1[p];
#pragma unroll 1
  for (uint32_t t1 = 0; t1 < (uint32_t)W; ++t1) {
    const T w1 = nufft3d_tap<T>(a, p, 0, t1, inv_half_w, beta);
    uint32_t row = row0;
#pragma unroll 1
    for (uint32_t t2 = 0; t2 < (uint32_t)W; ++t2) {
      const T w12 = w1 * nufft3d_tap<T>(a, p, 1, t2, inv_half_w, beta);
      const uint32_t base = (plane * L2 + row) * L3;
      uint32_t col = col0;
#pragma unroll
      for (int t3 = 0; t3 < W; ++t3) {
        const T wt = w12 * w3[t3];
        const uint32_t off = (base + col) * E;
#pragma unroll
        for (int r = 0; r < RB; ++r) {
          const cpx<T> v = buf_load_elem<T>(rin[r], off);
          acc[r].re += wt * v.re;
          acc[r].im += wt * v.im;
        }
        col = col + 1u == L3 ? 0u : col + 1u;
      }
      row = row + 1u == L2 ? 0u : row + 1u;
    }
    plane = plane + 1u == L1 ? 0u : plane + 1u;
  }
  const uint32_t dst = a.perm[p] * E;
#pragma unroll
  for (int r = 0; r < RB; ++r) buf_store_elem<T>(make_rsrc(out + (size_t)r * M * E, M * E), dst, acc[r]);
}

// the [3][w][m] table of the tabulated route: one lane per sorted point
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) nufft3d_table_kernel(Nufft3dArgs a) {
  const T inv_half_w = (T)2 / (T)a.w, beta = (T)a.beta;
  for (size_t p = (size_t)blockIdx.x * REAL_THREADS + threadIdx.x; p < a.m; p += (size_t)gridDim.x * REAL_THREADS) {
    const T d1 = ((const T*)a.d1)[p], d2 = ((const T*)a.d2)[p], d3 = ((const T*)a.d3)[p];
    for (uint32_t t = 0; t < a.w; ++t) {
      ((T*)a.out)[(size_t)t * a.m + p] = nufft_weight<T>(d1, t, inv_half_w, beta);
      ((T*)a.out)[((size_t)a.w + t) * a.m + p] = nufft_weight<T>(d2, t, inv_half_w, beta);
      ((T*)a.out)[((size_t)2 * a.w + t) * a.m + p] = nufft_weight<T>(d3, t, inv_half_w, beta);
    }
  }
}

// transformed grid items of l1 x l2 x l3 -> items of n1 x n2 x n3 modes:
// out[item, j1, j2, j3] = grid[item, cell(k1), cell(k2), cell(k3)] / (phihat_1 phihat_2 phihat_3)
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) nufft3d_deconv_kernel(Nufft3dArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t item = real_div(idx, a.item_m, a.item_l), rem = idx - item * (a.n1 * a.n2 * a.n3);
  const uint32_t q = real_div(rem, a.row_m, a.row_l), j3 = rem - q * a.n3;
  const uint32_t j1 = real_div(q, a.mid_m, a.mid_l), j2 = q - j1 * a.n2;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  uint32_t mag1, mag2, mag3;
  bool neg1, neg2, neg3;
  nufft_mode(j1, a.n1, a.order, mag1, neg1);
  nufft_mode(j2, a.n2, a.order, mag2, neg2);
  nufft_mode(j3, a.n3, a.order, mag3, neg3);
  const uint32_t cell1 = neg1 ? a.l1 - mag1 : mag1, cell2 = neg2 ? a.l2 - mag2 : mag2, cell3 = neg3 ? a.l3 - mag3 : mag3;
  const T s = ((const T*)a.inv1)[mag1] * ((const T*)a.inv2)[mag2] * ((const T*)a.inv3)[mag3];
  const cpx<T> v = real_load<T>(rin, (item * a.cells + (cell1 * a.l2 + cell2) * a.l3 + cell3) * E);
  buf_store_elem<T, BUF_NT>(rout, idx * E, cpx<T>{v.re * s, v.im * s});
}

// the position of the mode that cell g of an axis of l cells holds (n modes on that axis), and |k|; false where the cell holds none
__device__ __forceinline__ bool nufft3d_cell_mode(uint32_t g, uint32_t l, uint32_t n, uint32_t order, uint32_t& j, uint32_t& mag) {
  const uint32_t lo = n / 2u, hi = n - lo;
  const bool pos = g < hi, neg = g >= l - lo;  // l >= 2 n: never both
  if (!pos && !neg) return false;
  mag = pos ? g : l - g;
  if (order == 0) j = pos ? lo + mag : lo - mag;
  else j = pos ? mag : n - mag;
  return true;
}

// items of n1 x n2 x n3 modes -> grid items of l1 x l2 x l3: grid[item, cell(k1), cell(k2), cell(k3)] = f[item, j(k1), j(k2), j(k3)] /
// phihat, zeros elsewhere
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) nufft3d_amplify_kernel(Nufft3dArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t item = real_div(idx, a.item_m, a.item_l), rem = idx - item * a.cells;
  const uint32_t q = real_div(rem, a.row_m, a.row_l), g3 = rem - q * a.l3;
  const uint32_t g1 = real_div(q, a.mid_m, a.mid_l), g2 = q - g1 * a.l2;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  cpx<T> y = {(T)0, (T)0};
  uint32_t j1, j2, j3, mag1, mag2, mag3;
  if (nufft3d_cell_mode(g1, a.l1, a.n1, a.order, j1, mag1) && nufft3d_cell_mode(g2, a.l2, a.n2, a.order, j2, mag2) &&
      nufft3d_cell_mode(g3, a.l3, a.n3, a.order, j3, mag3)) {
    const T s = ((const T*)a.inv1)[mag1] * ((const T*)a.inv2)[mag2] * ((const T*)a.inv3)[mag3];
    const cpx<T> v = real_load<T>(rin, (item * (a.n1 * a.n2 * a.n3) + (j1 * a.n2 + j2) * a.n3 + j3) * E);
    y = {v.re * s, v.im * s};
  }
  buf_store_elem<T, BUF_NT>(rout, idx * E, y);
}

FOURIER_KERNELS_END
