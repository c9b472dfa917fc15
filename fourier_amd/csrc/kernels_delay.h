// kernels_delay.h -- device code of the delay handle (DelayPlan, delay_plan.h): rows of n values, zero-extended to L, are delayed by a
// per-row number of samples d (any finite real, read from device memory), optionally weighted and summed over groups of C channels:
//   Y[g, k] = sum_c w[gC + c] X[gC + c, k] m(k, d[gC + c]),  m(k, d) = exp(-2 pi i k' d / L),  k' = k below L/2, k - L above,
//   m(L/2, d) = cos(pi d) (even L),  out[g] = ifft(Y[g])[0 .. n).
//
// The phase (delay_split, delay_phase): d is reduced modulo L by fmod (exact) and split into rint and a remainder of at most 1/2
// (both exact); the integer part's exponent (k d_int) mod L is formed in integer arithmetic, the fraction adds k' d_frac / L, at
// most a quarter turn, and ONE accurate sincospi of the sum in turns follows: the phase error does not grow with |d| or with k.
// The delay never enters an address: a NaN or an infinity gives NaN multipliers, so the rows of its group are NaN and nothing else is
// touched.
//
// delay_small_kernel: the whole chain for REAL rows, C = 1, in ONE launch for L = L1 x L2 = 2^11 ... 2^15 (f64: ... 2^14), on
// hilbert_small_kernel's skeleton (kernels_hilbert.h).  After the forward core register r of lane (th2, cg2) holds bin
// k = k0 + (L/16) r, k0 = cg2 VEC + v + L1 th2 < L/16: the bins below L/2 are the registers r < 8, the Nyquist bin is v = 0, r = 8 of
// lane 0.  So m(k, d) = m(k0, d) t[r], t[r] = exp(-2 pi i r d / 16) for r < 8 and exp(-2 pi i (r - 16) d / 16) for r >= 8 (k' = k - L
// there): VEC accurate sincospi a lane for m(k0, d), and the 16 factors t[r] w / L, the same for the whole row, computed once per
// workgroup by 16 lanes with the same split (integer exponent (r d_int) mod 16, fraction at most half a turn) into the head of the
// core's LDS area between the two transforms.  One workgroup reads its whole row before it stores any of it: in place is allowed.
//
// delay_mul_kernel, the composed routes' one new sweep, is written like xcorr_mul_kernel / hilbert_expand_kernel: buffer descriptors
// with non-temporal hints, the flat index split by multiply-high, XCD-contiguous workgroups; one lane per output bin, which walks its
// group's C rows in ascending order: no atomics, bit-equal on repetition.
#pragma once
#include "kernels_hilbert.h"

FOURIER_KERNELS_BEGIN

// sin(pi x), cos(pi x), accurate (not the fast hardware sine)
__device__ __forceinline__ void delay_sincospi(float x, float& s, float& c) {
#ifdef FOURIER_EMU
  const double p = 3.14159265358979323846 * (double)x;
  s = (float)std::sin(p); c = (float)std::cos(p);
#else
  sincospif(x, &s, &c);
#endif
}
__device__ __forceinline__ void delay_sincospi(double x, double& s, double& c) {
#ifdef FOURIER_EMU
  const long double p = 3.14159265358979323846264338327950288L * (long double)x;
  s = (double)std::sin(p); c = (double)std::cos(p);
#else
  sincospi(x, &s, &c);
#endif
}

// d mod L as an integer in [0, L] and a remainder of at most 1/2, both exact; a delay that is not finite gives 0 and a NaN
template <typename T> __device__ __forceinline__ uint32_t delay_split(T d, uint32_t L, T& frac) {
  const T r = fmod(d, (T)L);  // exact; |r| < L
  const T q = rint(r);
  frac = r - q;               // exact
  int32_t di = q == q ? (int32_t)q : 0;
  if (di < 0) di += (int32_t)L;
  return (uint32_t)di;
}

// exp(-2 pi i (e + kp frac) / L) for an integer exponent e < L (reduced to [-L/2, L/2) first) and |kp frac| <= L / 4
template <typename T> __device__ __forceinline__ cpx<T> delay_phase(uint32_t e, T kp, T frac, uint32_t L) {
  const int32_t es = 2u * e >= L ? (int32_t)e - (int32_t)L : (int32_t)e;
  const T sum = kp * frac + (T)es;
  T s, c;
  delay_sincospi((T)-2 * sum / (T)L, s, c);
  return cpx<T>{c, s};
}

template <typename T> __device__ __forceinline__ cpx<T> delay_cmul(cpx<T> a, cpx<T> b) {
  return cpx<T>{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}

template <typename T, int L1, int L2>
__global__ void __launch_bounds__(FOURIER_TWOLEVEL_NT(T, L1, L2), FOURIER_BLU_SMALL_MIN_WAVES(FOURIER_TWOLEVEL_NT(T, L1, L2)))
    delay_small_kernel(PassArgs a) {
  constexpr int VEC = 16 / (2 * (int)sizeof(T));
  constexpr int CG1 = L2 / VEC, CG2 = L1 / VEC, Q1 = L1 / 16, Q2 = L2 / 16, N = L1 * L2;
  static_assert(L2 % 16 == 0 && (size_t)16 * sizeof(cpx<T>) <= TwolevelTr<T, L1, L2>::BYTES, "the row's 16 factors fit the core's area");
  FOURIER_DYN_SMEM(smem);
  const int tid = (int)threadIdx.x;
  const uint64_t blk = onelaunch_block(a);
  constexpr uint32_t RS = (uint32_t)sizeof(T);
  const uint32_t n = a.dl_n;
  const BufRsrc ri = make_rsrc((const T*)a.in + blk * n, n * RS);  // positions n ... N - 1 load as zeros
  const BufRsrc ro = make_rsrc((T*)a.out + blk * n, n * RS);       // ... and are not stored
  constexpr uint32_t ROW = (uint32_t)(Q1 * L2);  // register r holds index (th + Q1*r)*L2 + cg*VEC + v
  cpx<T> x[VEC][16];
  {
    const int th = tid / CG1, cg = tid % CG1;
    const uint32_t e0 = (uint32_t)(th * L2 + cg * VEC);
    // f32: a lane's two adjacent reals in one 8-byte access where the input is 8-byte aligned and the rows are whole multiples of 8
    // bytes (wave-uniform; hilbert_small_kernel's `pairs`); n is even then, so a pair lies wholly below n or wholly above
    const bool pairs = VEC == 2 && ((uint64_t)a.in & 7u) == 0 && (n & 1u) == 0;
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
  {  // (.) m(k, d) w / N, then the inverse's leading swap
    int tb = tid;
    FOURIER_LAUNDER(tb);
    const int th2 = tb / CG2, cg2 = tb % CG2;
    T frac;
    const uint32_t di = delay_split<T>(((const T*)a.dl_delays)[blk], (uint32_t)N, frac);
    cpx<T>* fac = (cpx<T>*)smem;
    __syncthreads();  // the reads of the core's last exchange are done
    if (tb < 16) {
      const T w = a.dl_weights ? ((const T*)a.dl_weights)[blk] : (T)1;
      const T ws = w * ((T)1 / (T)N);
      const cpx<T> t = delay_phase<T>(((uint32_t)tb * di) & 15u, (T)(tb < 8 ? tb : tb - 16), frac, 16u);
      fac[tb] = cpx<T>{t.re * ws, t.im * ws};
    }
    cpx<T> m0[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const uint32_t k0 = (uint32_t)(cg2 * VEC + v + L1 * th2);  // < N / 16
      m0[v] = delay_phase<T>((k0 * di) & (uint32_t)(N - 1), (T)k0, frac, (uint32_t)N);
    }
    __syncthreads();
    const bool lane0 = tb == 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const cpx<T> t = fac[r];
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        cpx<T> m = delay_cmul<T>(m0[v], t);
        if (r == 8 && v == 0 && lane0) m.im = (T)0;  // the Nyquist bin: cos(pi d)
        const cpx<T> y = delay_cmul<T>(x[v][r], m);
        x[v][r] = {y.im, y.re};
      }
    }
  }
  __syncthreads();
  {
    int t2 = tid;
    FOURIER_LAUNDER(t2);  // the inverse's lane mappings are derived here, not carried through the forward transform
    twolevel_core<T, L2, L1>(x, t2, smem, (const cpx<T>*)a.tw2, (const cpx<T>*)a.tw1, (const cpx<T>*)a.tw_hi, 32);
  }
  // back in the input's layout; the trailing swap: the real part is x.im; streaming stores of the first n
  {
    int tb = tid;
    FOURIER_LAUNDER(tb);
    const uint32_t e0 = (uint32_t)((tb / CG1) * L2 + (tb % CG1) * VEC);
    const bool pairs = VEC == 2 && ((uint64_t)a.out & 7u) == 0 && (n & 1u) == 0;  // (as the load)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const uint32_t off = (e0 + (uint32_t)r * ROW) * RS;
      if constexpr (VEC == 2) {
        if (pairs) {
          buf_store_elem<T, BUF_NT>(ro, off, cpx<T>{x[0][r].im, x[1][r].im});
          continue;
        }
      }
#pragma unroll
      for (int v = 0; v < VEC; ++v) buf_store_real<T, BUF_NT>(ro, off + (uint32_t)v * RS, x[v][r].im);
    }
  }
}

// groups of `channels` spectra -> one row a group: sum_c w[c] X[c][k] m(k, d[c]) * scale, ascending c; one lane per output bin
template <typename T, bool REAL_DATA>
__global__ void __launch_bounds__(REAL_THREADS) delay_mul_kernel(DelayArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t g = real_div(idx, a.div_m, a.div_l), k = idx - g * a.spec, L = a.l;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  const bool below = REAL_DATA || 2u * k < L;  // (half spectra end at L/2)
  const T kp = below ? (T)k : -(T)(L - k);
  const bool nyquist = 2u * k == L;
  const bool narrow = L <= 65536u;  // k d_int fits 32 bits
  const T scale = (T)a.scale;
  cpx<T> acc = {(T)0, (T)0};
  uint32_t row = g * a.channels;  // of this launch
  for (uint32_t c = 0; c < a.channels; ++c, ++row) {
    T frac;
    const uint32_t di = delay_split<T>(((const T*)a.delays)[row], L, frac);
    const T w = a.weights ? ((const T*)a.weights)[row] * scale : scale;
    uint32_t e;
    if (narrow) {
      const uint32_t p = k * di;
      e = p - real_div(p, a.len_m, a.len_l) * L;
    } else {
      e = (uint32_t)(((uint64_t)k * di) % L);
    }
    cpx<T> m = delay_phase<T>(e, kp, frac, L);
    if (nyquist) m.im = (T)0;
    const cpx<T> X = real_load<T>(rin, (row * a.spec + k) * E);
    const cpx<T> y = delay_cmul<T>(X, m);
    acc.re += y.re * w;
    acc.im += y.im * w;
  }
  buf_store_elem<T, BUF_NT>(rout, idx * E, acc);
}

FOURIER_KERNELS_END

namespace fourier_hip {

// delay_small_kernel<T, L1, L2> with the launch shape and the LDS bytes of the two-level plan of the same length
// (kernels_onelaunch.cpp)
template <typename T, int L1, int L2> static bool delay_small_info(int k, KernelInfo& info) {
  int l1 = 0, l2 = 0;
  if (!get_twolevel_kernel(Real<T>{}, k, info, l1, l2) || l1 != L1 || l2 != L2) return false;
  info.fn = &delay_small_kernel<T, L1, L2>;
  return true;
}

}  // namespace fourier_hip
