// kernels_hilbert.h -- device code of the analytic-signal handle (HilbertPlan, hilbert_plan.h): of rows of N reals x the analytic
// signal z = ifft(fft(x) (.) m), m[k] = 1 for k = 0 and (N even) k = N/2, 2 for 0 < k < N/2, 0 above, so that Re z = x
// (scipy.signal.hilbert), or its magnitude |z|, the envelope.
//
// hilbert_small_kernel: the whole chain in ONE launch for N = L1 x L2 = 2^11 ... 2^15 (f64: ... 2^14), conv_small_kernel
// (kernels_onelaunch.h) with three differences.  It loads REAL rows with the imaginary registers zero; the product with a table
// becomes the multiplier m[k] / N computed from the bin index, with no memory access; and it stores either z (16-byte units of complex
// values, as conv_small_kernel) or |z| (reals).  One workgroup reads its whole row before it stores any of it, so the envelope may
// be written onto its input.
//
// The two sweeps of the composed route are written like conv_mul_kernel (kernels_conv.h): one element per access through buffer
// descriptors with non-temporal hints, the flat index rows x N split by multiply-high, XCD-contiguous workgroups.
// hilbert_expand_kernel: half spectrum X (rows of h + 1, RealPlan's output) -> rows of N complex values X[k] m[k] / N, zeros above.
// hilbert_abs_kernel: rows of N complex values z -> rows of N reals |z|.
#pragma once
#include "kernels_onelaunch.h"
#include "kernels_real.h"

FOURIER_KERNELS_BEGIN

__device__ __forceinline__ float hilbert_abs(float re, float im) { return sqrtf(re * re + im * im); }
__device__ __forceinline__ double hilbert_abs(double re, double im) { return sqrt(re * re + im * im); }

template <typename T, int L1, int L2, bool ENVELOPE>
__global__ void __launch_bounds__(FOURIER_TWOLEVEL_NT(T, L1, L2), FOURIER_BLU_SMALL_MIN_WAVES(FOURIER_TWOLEVEL_NT(T, L1, L2)))
    hilbert_small_kernel(PassArgs a) {
  constexpr int VEC = 16 / (2 * (int)sizeof(T));
  constexpr int CG1 = L2 / VEC, CG2 = L1 / VEC, Q1 = L1 / 16, Q2 = L2 / 16, N = L1 * L2;
  FOURIER_DYN_SMEM(smem);
  const int tid = (int)threadIdx.x;
  const uint64_t blk = onelaunch_block(a);
  constexpr uint32_t RS = (uint32_t)sizeof(T), CS = (uint32_t)sizeof(cpx<T>);
  constexpr uint32_t OS = ENVELOPE ? RS : CS;  // bytes of one value of an output row
  const BufRsrc ri = make_rsrc((const T*)a.in + blk * N, (uint32_t)N * RS);
  const BufRsrc ro = make_rsrc((char*)a.out + blk * N * OS, (uint32_t)N * OS);
  constexpr uint32_t ROW = (uint32_t)(Q1 * L2);  // register r holds index (th + Q1*r)*L2 + cg*VEC + v
  cpx<T> x[VEC][16];
  {
    const int th = tid / CG1, cg = tid % CG1;
    const uint32_t e0 = (uint32_t)(th * L2 + cg * VEC);
    // f32: a lane's two adjacent reals lie on an 8-byte boundary of their row (rows are whole multiples of 8 bytes): one 8-byte access
    // where the input itself is 8-byte aligned (wave-uniform; lconv_small_kernel's `pairs`)
    const bool pairs = VEC == 2 && ((uint64_t)a.in & 7u) == 0;
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
  }
  twolevel_core<T, L1, L2>(x, tid, smem, (const cpx<T>*)a.tw1, (const cpx<T>*)a.tw2, (const cpx<T>*)a.tw_lo, 0);
  {  // register r holds X[k], k = k1 + L1*k2, k2 = th2 + Q2*r, k1 = cg2*VEC + v (conv_small_kernel): (.) m[k] / N, then the inverse's
    // leading swap.  th2 < Q2 and N / 2 = L1 * 8 Q2, so k < N/2 exactly in the registers r < 8: they take 2 / N, the registers above are
    // constant zeros (the first radix-16 stage of the inverse folds), and the bins 0 and N/2, which take 1 / N, are v = 0 of the
    // registers 0 and 8 of lane 0.
    int tb = tid;
    FOURIER_LAUNDER(tb);
    constexpr T S1 = (T)1 / (T)N, S2 = (T)2 / (T)N;
    const bool lane0 = tb == 0;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const T s = (v == 0 && r == 0 && lane0) ? S1 : S2;
        x[v][r] = {x[v][r].im * s, x[v][r].re * s};
      }
      x[v][8] = (v == 0 && lane0) ? cpx<T>{x[v][8].im * S1, x[v][8].re * S1} : cpx<T>{(T)0, (T)0};
#pragma unroll
      for (int r = 9; r < 16; ++r) x[v][r] = cpx<T>{(T)0, (T)0};
    }
  }
  __syncthreads();
  {
    int t2 = tid;
    FOURIER_LAUNDER(t2);  // the inverse's lane mappings are derived here, not carried through the forward transform
    twolevel_core<T, L2, L1>(x, t2, smem, (const cpx<T>*)a.tw2, (const cpx<T>*)a.tw1, (const cpx<T>*)a.tw_hi, 32);
  }
  // back in the input's layout; the trailing swap: z = (x.im, x.re); streaming stores
  {
    int tb = tid;
    FOURIER_LAUNDER(tb);
    const uint32_t e0 = (uint32_t)((tb / CG1) * L2 + (tb % CG1) * VEC);
    if constexpr (ENVELOPE) {
      // the magnitudes first, pinned in registers: the stores below exist twice (wave-uniform branch), and square roots that sink into
      // both copies spill under the 128-VGPR budget
      T m[VEC][16];
#pragma unroll
      for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          m[v][r] = hilbert_abs(x[v][r].re, x[v][r].im);
          FOURIER_LAUNDER(m[v][r]);
        }
      const bool pairs = VEC == 2 && ((uint64_t)a.out & 7u) == 0;  // (as the load)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const uint32_t off = (e0 + (uint32_t)r * ROW) * RS;
        if constexpr (VEC == 2) {
          if (pairs) {
            buf_store_elem<T, BUF_NT>(ro, off, cpx<T>{m[0][r], m[1][r]});
            continue;
          }
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) buf_store_real<T, BUF_NT>(ro, off + (uint32_t)v * RS, m[v][r]);
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        Unit16<T> u;
#pragma unroll
        for (int v = 0; v < VEC; ++v) { u.a[2 * v] = x[v][r].im; u.a[2 * v + 1] = x[v][r].re; }
        buf_store_unit<T, BUF_NT>(ro, (e0 + (uint32_t)r * ROW) * CS, u);
      }
    }
  }
}

// half spectrum X (rows of h + 1 complex values) -> rows of n complex values X[k] m[k] * scale, zeros above n / 2; one lane per output
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) hilbert_expand_kernel(HilbertArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t row = real_div(idx, a.div_m, a.div_l), k = idx - row * a.n;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  cpx<T> y = {(T)0, (T)0};
  if (k <= a.h) {  // (odd n: h = (n - 1) / 2, every bin but 0 is doubled)
    const cpx<T> X = real_load<T>(rin, (row * (a.h + 1) + k) * E);
    const T s = (k == 0 || 2 * k == a.n) ? (T)a.scale : (T)2 * (T)a.scale;
    y = {X.re * s, X.im * s};
  }
  buf_store_elem<T, BUF_NT>(rout, idx * E, y);
}

// `total` complex values z -> reals |z|
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) hilbert_abs_kernel(HilbertArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  const cpx<T> z = real_load<T>(rin, idx * (uint32_t)sizeof(cpx<T>));
  buf_store_real<T, BUF_NT>(rout, idx * (uint32_t)sizeof(T), hilbert_abs(z.re, z.im));
}

FOURIER_KERNELS_END
