// kernels_czt.h -- device code of the chirp-z handle (CztPlan, czt_plan.h): of rows of n values x, the m values
//   X[k] = sum_j x[j] a^-j w^(j k) = B[k] sum_j (x[j] A[j]) v[k - j],   A[j] = a^-j w^(j^2/2),  B[k] = w^(k^2/2),  v[i] = w^(-i^2/2),
// Bluestein's identity j k = (j^2 + k^2 - (k - j)^2) / 2 with a free output count and a free contour: a linear convolution of n with
// n + m - 1 values, carried by a circular one of L >= n + m - 1 points whose table H = FFT_L(v) / L the host prepares (czt_plan.h).
//
// czt_small_kernel: the whole chain in ONE launch for L = L1 x L2 = 2^11 ... 2^15 (f64: ... 2^14), a sibling of bluestein_small_kernel
// (kernels_onelaunch.h) with these differences.  The input row has n values and the output row m, independent of each other, each behind
// its own descriptor: everything at or beyond n loads as zero, nothing at or beyond m is stored.  n may reach L - m + 1 and m may reach
// L - n + 1, so ALL 16 register rows are live on both sides (the Bluestein kernel's 2n <= M makes rows 8 .. 15 constant zeros).  The two
// chirps are separate tables, A of n entries and B of m entries, read through descriptors of their own (zero beyond the end: a padding
// position is 0 * 0, never 0 * garbage).  REAL: the input rows are reals, loaded with the imaginary registers zero; an f32 lane's two
// adjacent reals move as one 8-byte access where n is even and the input is 8-byte aligned (then every row is, and a pair lies inside
// or outside its row as one).  User rows of odd length are only 8-byte aligned in f32, which the 16-byte buffer accesses tolerate; the
// hardware's dword-wise range check cuts the ragged last unit of a row.  H carries the inverse's 1 / L; there is no scale.
//
// The two end sweeps of the composed route are written like conv_mul_kernel (kernels_conv.h): one element per access through buffer
// descriptors with non-temporal hints on the data, XCD-contiguous workgroups; the chirps are read with plain loads (shared by every row).
// czt_in_kernel: rows of n -> rows of L, x[j] A[j] and zeros from n on.  czt_out_kernel: the first m of L, times B[k].
#pragma once
#include "kernels_onelaunch.h"
#include "kernels_real.h"

FOURIER_KERNELS_BEGIN

template <typename T, int L1, int L2, bool REAL>
__global__ void __launch_bounds__(FOURIER_TWOLEVEL_NT(T, L1, L2), FOURIER_BLU_SMALL_MIN_WAVES(FOURIER_TWOLEVEL_NT(T, L1, L2)))
    czt_small_kernel(PassArgs a) {
  constexpr int VEC = 16 / (2 * (int)sizeof(T));
  constexpr int CG1 = L2 / VEC, CG2 = L1 / VEC, Q1 = L1 / 16, Q2 = L2 / 16, N = L1 * L2;
  FOURIER_DYN_SMEM(smem);
  const int tid = (int)threadIdx.x;
  const uint64_t blk = onelaunch_block(a);
  constexpr uint32_t RS = (uint32_t)sizeof(T), CS = (uint32_t)sizeof(cpx<T>);
  constexpr uint32_t VS = REAL ? RS : CS;  // bytes of one value of an input row
  const uint32_t n = a.cz_n, m = a.cz_m;
  const BufRsrc ri = make_rsrc((const char*)a.in + blk * n * VS, n * VS);
  const BufRsrc ro = make_rsrc((cpx<T>*)a.out + blk * m, m * CS);
  const BufRsrc ra = make_rsrc(a.cz_a, n * CS), rb = make_rsrc(a.cz_b, m * CS);
  constexpr uint32_t ROW = (uint32_t)(Q1 * L2);  // register r holds index (th + Q1*r)*L2 + cg*VEC + v
  cpx<T> x[VEC][16];
  {
    const int th = tid / CG1, cg = tid % CG1;
    const uint32_t e0 = (uint32_t)(th * L2 + cg * VEC);
    if constexpr (REAL) {
      const bool pairs = VEC == 2 && (n & 1u) == 0 && ((uint64_t)a.in & 7u) == 0;  // wave-uniform, the same in every workgroup
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const uint32_t off = (e0 + (uint32_t)r * ROW) * RS;
        if constexpr (VEC == 2) {
          if (pairs) {
            const cpx<T> p = buf_load_pair<T, BUF_NT>(ri, off);
            x[0][r] = {p.re, (T)0};
            x[1][r] = {p.im, (T)0};
            continue;
          }
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) x[v][r] = {buf_load_real<T, BUF_NT>(ri, off + (uint32_t)v * RS), (T)0};
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const Unit16<T> u = buf_load_unit<T, BUF_NT>(ri, (e0 + (uint32_t)r * ROW) * CS);
#pragma unroll
        for (int v = 0; v < VEC; ++v) x[v][r] = {u.a[2 * v], u.a[2 * v + 1]};
      }
    }
    // (.) A: zero from n on, like the data
    const uint32_t aoff = e0 * CS;
    units_batched<T, 8>([&](int r) { return buf_load_unit<T>(ra, aoff + (uint32_t)r * ROW * CS); },
                        [&](int r, const Unit16<T>& c) {
#pragma unroll
                          for (int v = 0; v < VEC; ++v) x[v][r] = cmul(cpx<T>{c.a[2 * v], c.a[2 * v + 1]}, x[v][r]);
                        });
  }
  twolevel_core<T, L1, L2>(x, tid, smem, (const cpx<T>*)a.tw1, (const cpx<T>*)a.tw2, (const cpx<T>*)a.tw_lo, 0);
  {  // register r holds X[k1 + L1*k2], k2 = th2 + Q2*r, k1 = cg2*VEC + v: (.) H, then the inverse's leading swap (conv_small_kernel)
    int tb = tid;
    FOURIER_LAUNDER(tb);
    const BufRsrc rw = make_rsrc(a.mul, (uint32_t)(N * sizeof(cpx<T>)));
    const uint32_t woff = (uint32_t)(((tb / CG2) * L1 + (tb % CG2) * VEC) * sizeof(cpx<T>));
    onelaunch_times_table_swap<T, L1, Q2>(x, rw, woff);
  }
  __syncthreads();
  {
    int t2 = tid;
    FOURIER_LAUNDER(t2);  // the inverse's lane mappings are derived here, not carried through the forward transform
    twolevel_core<T, L2, L1>(x, t2, smem, (const cpx<T>*)a.tw2, (const cpx<T>*)a.tw1, (const cpx<T>*)a.tw_hi, 32);
  }
  // back in the input's layout: the trailing swap, (.) B, streaming stores of the first m
  {
    int tb = tid;
    FOURIER_LAUNDER(tb);
    const uint32_t soff = (uint32_t)(((tb / CG1) * L2 + (tb % CG1) * VEC) * sizeof(cpx<T>));
    units_batched<T, 8>([&](int r) { return buf_load_unit<T>(rb, soff + (uint32_t)r * ROW * CS); },
                        [&](int r, const Unit16<T>& c) {
                          Unit16<T> u;
#pragma unroll
                          for (int v = 0; v < VEC; ++v) {
                            const cpx<T> y = cmul(cpx<T>{x[v][r].im, x[v][r].re}, cpx<T>{c.a[2 * v], c.a[2 * v + 1]});
                            u.a[2 * v] = y.re; u.a[2 * v + 1] = y.im;
                          }
                          buf_store_unit<T, BUF_NT>(ro, soff + (uint32_t)r * ROW * CS, u);
                        });
  }
}

// rows of n values (complex, or reals) -> rows of L = 2^l_shift complex values x[j] A[j], zeros from n on; one lane per output
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) czt_in_kernel(CztArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t row = idx >> a.l_shift, j = idx - (row << a.l_shift);
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  cpx<T> y = {(T)0, (T)0};
  if (j < a.n) {
    cpx<T> x;
    if (a.real) x = {buf_load_real<T, BUF_NT>(rin, (row * a.n + j) * (uint32_t)sizeof(T)), (T)0};
    else x = real_load<T>(rin, (row * a.n + j) * E);
    y = cmul(((const cpx<T>*)a.tab)[j], x);
  }
  buf_store_elem<T, BUF_NT>(rout, idx * E, y);
}

// rows of L complex values y -> rows of m complex values y[k] B[k]; one lane per output
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) czt_out_kernel(CztArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t row = real_div(idx, a.div_m, a.div_l), k = idx - row * a.m;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  const cpx<T> y = real_load<T>(rin, ((row << a.l_shift) + k) * E);
  buf_store_elem<T, BUF_NT>(rout, idx * E, cmul(y, ((const cpx<T>*)a.tab)[k]));
}

FOURIER_KERNELS_END
