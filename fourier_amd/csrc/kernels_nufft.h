// kernels_nufft.h -- device code of the non-uniform FFT handle (NufftPlan, nufft_plan.h): 1-D types 1 and 2 with m points shared by the
// rows of a batch, on a fine grid of l cells and the "exponential of semicircle" kernel of width w,
//   phi(z) = exp(beta (sqrt(1 - z^2) - 1)) on |z| <= 1,  beta = 2.30 w.
// The host (NufftPlan::set_points) sorts the points by their grid coordinate xg and uploads per SORTED point p its first cell
// i0[p] = ceil(xg - w/2), the offset d[p] = i0 - xg in [-w/2, -w/2 + 1) and the caller's index perm[p]; point p touches the cells
// i0 .. i0 + w - 1 modulo l, tap t with weight phi(2 (d + t) / w).  first[e + w], e in [-w, l + w], counts the sorted points with i0 < e.
//
// nufft_spread_kernel<T, W, RB> (type 1, step 1) is a GATHER: one lane owns one cell i for RB consecutive rows.  The points whose
// footprint covers i have i0 in [i - W + 1, i], a contiguous run first[i - W + 1] .. first[i + 1] of the sorted list; the footprints
// that wrap reach i as cell i - l (footprints that begin below 0: the lowest sorted indices) or as cell i + l (footprints that end at or
// above l: the highest), two more runs, empty for all but the W cells at either end.  The lane walks the three runs in ascending
// sorted index, forms the weight once per point and adds weight * c[row, perm[p]] into one accumulator per row.  No atomics, no
// LDS, one store a cell: the sum's order depends on the points alone, so it is bit-equal on repetition, under any launch split and
// for any batch.  Points with equal xg keep the caller's order (a stable sort).
// nufft_interp_kernel<T, W, RB> (type 2, step 3): one lane owns one sorted point for RB rows, forms its W weights once, reads its W
// cells with the wrap in ascending tap and stores c[row, perm[p]].
// Weights: evaluated in the kernel with the accurate exp and sqrt (a.wtab == null), or read from the table a set-up kernel wrote
// with the same function (nufft_table_kernel; [w][m], so that the interpolation's lanes read runs).
// nufft_deconv_kernel / nufft_amplify_kernel are sweeps written like delay_mul_kernel: buffer descriptors with non-temporal hints,
// the flat index split by multiply-high, XCD-contiguous workgroups.  deconv picks the n modes out of a transformed grid row and
// multiplies by 1 / phihat(|k|); amplify writes f / phihat into a grid row and zeros into the rest of it.  Both map the mode index k
// (order 0: ascending from -floor(n/2); order 1: FFT order) to cell k, or l + k for k < 0.
#pragma once
#include "kernels_real.h"

FOURIER_KERNELS_BEGIN

__device__ __forceinline__ float nufft_exp(float x) { return expf(x); }
__device__ __forceinline__ double nufft_exp(double x) { return exp(x); }
__device__ __forceinline__ float nufft_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double nufft_sqrt(double x) { return sqrt(x); }

// phi(2 (d + t) / W): the weight of tap t of a point with offset d
template <typename T> __device__ __forceinline__ T nufft_weight(T d, uint32_t t, T inv_half_w, T beta) {
  const T z = (d + (T)t) * inv_half_w;
  const T q = (T)1 - z * z;
  return nufft_exp(beta * (nufft_sqrt(q > (T)0 ? q : (T)0) - (T)1));
}
template <typename T> __device__ __forceinline__ T nufft_tap(const NufftArgs& a, uint32_t p, uint32_t t, T inv_half_w, T beta) {
  if (a.wtab) return ((const T*)a.wtab)[(size_t)t * a.m + p];
  return nufft_weight<T>(((const T*)a.d)[p], t, inv_half_w, beta);
}

// the row block of this workgroup and its position among the workgroups of that block (XCD-contiguous: real_xcd_block's rule)
__device__ __forceinline__ void nufft_block(const NufftArgs& a, uint32_t& rb, uint32_t& seg) {
  const uint32_t blk = real_xcd_block(blockIdx.x, gridDim.x);
  rb = real_div(blk, a.per_m, a.per_l);
  seg = blk - rb * a.per;
}

template <typename T, int W, int RB>
__global__ void __launch_bounds__(REAL_THREADS) nufft_spread_kernel(NufftArgs a) {
  uint32_t rb, seg;
  nufft_block(a, rb, seg);
  const uint32_t i = seg * REAL_THREADS + threadIdx.x, L = a.l, M = a.m;
  if (i >= L) return;
  constexpr uint32_t E = sizeof(cpx<T>);
  const T inv_half_w = (T)2 / (T)W, beta = (T)a.beta;
  const char* in = (const char*)a.in + (size_t)rb * RB * M * E;
  char* out = (char*)a.out + (size_t)rb * RB * L * E;
  BufRsrc rin[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) rin[r] = make_rsrc(in + (size_t)r * M * E, M * E);
  cpx<T> acc[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) acc[r] = {(T)0, (T)0};
  // the images of cell i in ascending sorted index: i - l (reached by footprints that begin below 0), i, i + l (... that end at or
  // above l); first[] is indexed by e + W and clamped to its range, where the two outer runs are empty
  const uint32_t top = L + 2u * W;  // the table's last index
#pragma unroll
  for (int img = 0; img < 3; ++img) {
    const int64_t c = (int64_t)i + (int64_t)(img - 1) * (int64_t)L;  // the cell as the points see it
    int64_t elo = c - W + 1 + W, ehi = c + 1 + W;                    // indices into first[]
    elo = elo < 0 ? 0 : elo > (int64_t)top ? (int64_t)top : elo;
    ehi = ehi < 0 ? 0 : ehi > (int64_t)top ? (int64_t)top : ehi;
    if (img != 1 && elo == ehi) continue;
    const uint32_t p0 = a.first[elo], p1 = a.first[ehi];
    for (uint32_t p = p0; p < p1; ++p) {
      const uint32_t t = (uint32_t)(c - (int64_t)a.i0[p]);  // in [0, W)
      const T wt = nufft_tap<T>(a, p, t, inv_half_w, beta);
      const uint32_t src = a.perm[p] * E;
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const cpx<T> v = buf_load_elem<T>(rin[r], src);
        acc[r].re += wt * v.re;
        acc[r].im += wt * v.im;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RB; ++r) buf_store_elem<T, BUF_NT>(make_rsrc(out + (size_t)r * L * E, L * E), i * E, acc[r]);
}

template <typename T, int W, int RB>
__global__ void __launch_bounds__(REAL_THREADS) nufft_interp_kernel(NufftArgs a) {
  uint32_t rb, seg;
  nufft_block(a, rb, seg);
  const uint32_t p = seg * REAL_THREADS + threadIdx.x, L = a.l, M = a.m;
  if (p >= M) return;
  constexpr uint32_t E = sizeof(cpx<T>);
  const T inv_half_w = (T)2 / (T)W, beta = (T)a.beta;
  const char* in = (const char*)a.in + (size_t)rb * RB * L * E;
  char* out = (char*)a.out + (size_t)rb * RB * M * E;
  T wt[W];
#pragma unroll
  for (int t = 0; t < W; ++t) wt[t] = nufft_tap<T>(a, p, (uint32_t)t, inv_half_w, beta);
  // the first cell modulo l: i0 is in [-W, l]
  const int32_t i0 = a.i0[p];
  uint32_t cell = i0 < 0 ? (uint32_t)(i0 + (int32_t)L) : (uint32_t)i0 >= L ? (uint32_t)i0 - L : (uint32_t)i0;
  uint32_t off[W];
#pragma unroll
  for (int t = 0; t < W; ++t) {
    off[t] = cell * E;
    cell = cell + 1u == L ? 0u : cell + 1u;
  }
  const uint32_t dst = a.perm[p] * E;
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    const BufRsrc rin = make_rsrc(in + (size_t)r * L * E, L * E);
    cpx<T> acc = {(T)0, (T)0};
#pragma unroll
    for (int t = 0; t < W; ++t) {
      const cpx<T> v = buf_load_elem<T>(rin, off[t]);
      acc.re += wt[t] * v.re;
      acc.im += wt[t] * v.im;
    }
    buf_store_elem<T>(make_rsrc(out + (size_t)r * M * E, M * E), dst, acc);
  }
}

// the [w][m] table of the tabulated route: one lane per sorted point
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) nufft_table_kernel(NufftArgs a) {
  const T inv_half_w = (T)2 / (T)a.w, beta = (T)a.beta;
  for (size_t p = (size_t)blockIdx.x * REAL_THREADS + threadIdx.x; p < a.m; p += (size_t)gridDim.x * REAL_THREADS) {
    const T d = ((const T*)a.d)[p];
    for (uint32_t t = 0; t < a.w; ++t) ((T*)a.out)[(size_t)t * a.m + p] = nufft_weight<T>(d, t, inv_half_w, beta);
  }
}

// the signed mode index k of position j of a row of n modes, as |k| and its sign
__device__ __forceinline__ void nufft_mode(uint32_t j, uint32_t n, uint32_t order, uint32_t& mag, bool& neg) {
  const uint32_t lo = n / 2u, hi = n - lo;  // floor(n/2) negative modes, ceil(n/2) from 0 on
  if (order == 0) { neg = j < lo; mag = neg ? lo - j : j - lo; }
  else { neg = j >= hi; mag = neg ? n - j : j; }
}

// transformed grid rows of l -> rows of n modes: out[row, j] = grid[row, cell(k_j)] / phihat(|k_j|)
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) nufft_deconv_kernel(NufftArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t row = real_div(idx, a.div_m, a.div_l), j = idx - row * a.n;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  uint32_t mag;
  bool neg;
  nufft_mode(j, a.n, a.order, mag, neg);
  const uint32_t cell = neg ? a.l - mag : mag;
  const T s = ((const T*)a.inv_phihat)[mag];
  const cpx<T> v = real_load<T>(rin, (row * a.l + cell) * E);
  buf_store_elem<T, BUF_NT>(rout, idx * E, cpx<T>{v.re * s, v.im * s});
}

// rows of n modes -> grid rows of l: grid[row, cell(k)] = f[row, j(k)] / phihat(|k|), zeros elsewhere
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) nufft_amplify_kernel(NufftArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t row = real_div(idx, a.div_m, a.div_l), g = idx - row * a.l, n = a.n;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  const uint32_t lo = n / 2u, hi = n - lo;
  cpx<T> y = {(T)0, (T)0};
  const bool pos = g < hi, neg = g >= a.l - lo;  // l >= 2 n: never both
  if (pos || neg) {
    const uint32_t mag = pos ? g : a.l - g;
    uint32_t j;
    if (a.order == 0) j = pos ? lo + mag : lo - mag;
    else j = pos ? mag : n - mag;
    const T s = ((const T*)a.inv_phihat)[mag];
    const cpx<T> v = real_load<T>(rin, (row * n + j) * E);
    y = {v.re * s, v.im * s};
  }
  buf_store_elem<T, BUF_NT>(rout, idx * E, y);
}

FOURIER_KERNELS_END
