// kernels_cepstrum.h -- device code of the cepstrum handle (CepstrumPlan, cepstrum_plan.h): rows of n reals, zero-extended to L,
// X = fft(x, L), g[k] = log_mult ln(max(|X[k]|, log_floor)), formed as 0.5 log_mult ln(max(re^2 + im^2, log_floor^2)) with the accurate
// logarithm;
//   CEPSTRUM       c = ifft(g) (real and even), out = c[0 .. m)
//   MINIMUM_PHASE  chat[0] = c[0], chat[q] = 2 c[q] for 0 < q < L/2, chat[L/2] = c[L/2] (even L), 0 above;  C = fft(chat),
//                  E[k] = exp(Re C[k]) (cos Im C[k], sin Im C[k]),  h = Re ifft(E),  out = h[0 .. m)
// (scipy.signal.minimum_phase(method="homomorphic") with the caller's floor and, at even L, weight 1 at quefrency L/2).
// The floor is applied as `p < f ? f : p`: a NaN bin stays NaN.  log_floor == 0 on a bin that is exactly 0 gives -inf: that row's
// output is not finite, and nothing else is touched -- no value of a row enters an address.  A positive floor whose square is no
// normal number of T arrives clamped, with the value of a bin below it from the host (cepstrum_g): below sqrt(min normal) every bin whose
// re^2 + im^2 is less than the smallest normal number -- a zero row, a bin that flushed to zero -- gives log_mult ln(log_floor); above
// sqrt(max) every bin whose re^2 + im^2 is finite does.
//
// cepstrum_small_kernel: the whole chain in ONE launch for L = L1 x L2 = 2^11 ... 2^15 (f64: ... 2^14) on delay_small_kernel's
// skeleton (kernels_delay.h): its load (n reals, zeros above, the f32 `pairs` rule), forward core, every register -> {g / N, 0} with
// the inverse's leading swap, inverse core; CEPSTRUM stores the first m real parts.  MINIMUM_PHASE goes on with the row in registers:
// back in the input's layout register r of lane (th, cg) holds index (th + Q1 r) L2 + cg VEC + v and N / 2 = 8 Q1 L2, so the fold is
// weight 2 for r < 8 but 1 for index 0 (r = 0, v = 0 of lane 0), 1 for r = 8, v = 0 of lane 0 and 0 for the rest; forward core again;
// E / N with the phase through ONE accurate sincospi of Im C / pi (no large-argument reduction: the rounding of that product is of the
// order of the error Im C already carries) and the accurate exponential; inverse core; store of the first m real parts.  Four cores,
// no table beyond the two-level plan's, no scratch buffer.  One workgroup reads its whole row before it stores any of it: in place
// is allowed where m == n.
//
// The composed route's three sweeps are written like delay_mul_kernel: buffer descriptors with non-temporal hints, one lane per
// value, XCD-contiguous workgroups, the flat index split by multiply-high where a row position is needed; all three run in place.
//   cepstrum_log_kernel   half spectra: X -> {g * scale, 0}
//   cepstrum_fold_kernel  rows of L reals: c -> chat
//   cepstrum_exp_kernel   half spectra: C -> E * scale
#pragma once
#include "kernels_delay.h"

FOURIER_KERNELS_BEGIN

// the accurate library functions, never the fast hardware ones
__device__ __forceinline__ float cepstrum_ln(float x) { return logf(x); }
__device__ __forceinline__ double cepstrum_ln(double x) { return log(x); }
__device__ __forceinline__ float cepstrum_exp(float x) { return expf(x); }
__device__ __forceinline__ double cepstrum_exp(double x) { return exp(x); }

// half * ln(max(re^2 + im^2, floor2)), half = 0.5 log_mult (times the inverse's 1 / L).  given: floor2 is log_floor^2 clamped to
// [min normal, +inf] and a bin below it takes g_floor, its finished value from the host (CepstrumFloor, kernel_args.h); the
// arithmetic of a bin at or above the floor, and of every bin where the square itself is a normal number, is unchanged
template <typename T> __device__ __forceinline__ T cepstrum_g(cpx<T> X, T half, T floor2, T g_floor, bool given) {
  const T p = X.re * X.re + X.im * X.im;
  const bool under = p < floor2;
  const T g = half * cepstrum_ln(under ? floor2 : p);
  return under && given ? g_floor : g;
}

// exp(re) (cos im, sin im) * scale
template <typename T> __device__ __forceinline__ cpx<T> cepstrum_e(cpx<T> C, T scale) {
  T s, c;
  delay_sincospi(C.im * (T)0.31830988618379067153776752674503, s, c);
  const T e = cepstrum_exp(C.re) * scale;
  return cpx<T>{e * c, e * s};
}

template <typename T, int L1, int L2, bool MINPHASE>
__global__ void __launch_bounds__(FOURIER_TWOLEVEL_NT(T, L1, L2), FOURIER_BLU_SMALL_MIN_WAVES(FOURIER_TWOLEVEL_NT(T, L1, L2)))
    cepstrum_small_kernel(PassArgs a) {
  constexpr int VEC = 16 / (2 * (int)sizeof(T));
  constexpr int CG1 = L2 / VEC, Q1 = L1 / 16, N = L1 * L2;
  FOURIER_DYN_SMEM(smem);
  const int tid = (int)threadIdx.x;
  const uint64_t blk = onelaunch_block(a);
  constexpr uint32_t RS = (uint32_t)sizeof(T);
  const uint32_t n = a.cp_n, m = a.cp_m;
  const BufRsrc ri = make_rsrc((const T*)a.in + blk * n, n * RS);  // positions n ... N - 1 load as zeros
  const BufRsrc ro = make_rsrc((T*)a.out + blk * m, m * RS);       // positions m ... N - 1 are not stored
  constexpr uint32_t ROW = (uint32_t)(Q1 * L2);  // register r holds index (th + Q1*r)*L2 + cg*VEC + v
  cpx<T> x[VEC][16];
  {
    const int th = tid / CG1, cg = tid % CG1;
    const uint32_t e0 = (uint32_t)(th * L2 + cg * VEC);
    // f32: a lane's two adjacent reals in one 8-byte access where the input is 8-byte aligned and the rows are whole multiples of 8
    // bytes (wave-uniform; delay_small_kernel's `pairs`); n is even then, so a pair lies wholly below n or wholly above
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
  {  // X -> {g / N, 0}, then the inverse's leading swap
    const T half = (T)a.cp_log_mult * ((T)0.5 / (T)N), floor2 = (T)a.cp_floor2, g_floor = (T)a.cp_g_floor;
    const bool given = a.cp_floor_given != 0;
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
      for (int v = 0; v < VEC; ++v) x[v][r] = {(T)0, cepstrum_g<T>(x[v][r], half, floor2, g_floor, given)};
  }
  __syncthreads();
  {
    int t2 = tid;
    FOURIER_LAUNDER(t2);  // the inverse's lane mappings are derived here, not carried through the forward transform
    twolevel_core<T, L2, L1>(x, t2, smem, (const cpx<T>*)a.tw2, (const cpx<T>*)a.tw1, (const cpx<T>*)a.tw_hi, 32);
  }
  if constexpr (MINPHASE) {
    {  // back in the input's layout, the trailing swap: c is x.im.  The fold; the next transform's rows are real
      int tb = tid;
      FOURIER_LAUNDER(tb);
      const bool lane0 = tb == 0;
      // an opaque zero: with literal zeros the compiler specialises this core apart from the fourth, and every f32 instance spills
      // 4 - 12 bytes a lane more
      T zero = (T)0;
      FOURIER_LAUNDER(zero);
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const T c = x[v][r].im;
          x[v][r] = {(v == 0 && r == 0 && lane0) ? c : c + c, zero};
        }
        x[v][8] = {(v == 0 && lane0) ? x[v][8].im : zero, zero};
#pragma unroll
        for (int r = 9; r < 16; ++r) x[v][r] = cpx<T>{zero, zero};
      }
    }
    __syncthreads();
    {
      int t3 = tid;
      FOURIER_LAUNDER(t3);
      twolevel_core<T, L1, L2>(x, t3, smem, (const cpx<T>*)a.tw1, (const cpx<T>*)a.tw2, (const cpx<T>*)a.tw_lo, 64);
    }
    {  // C -> E / N, then the inverse's leading swap
      constexpr T S = (T)1 / (T)N;
#pragma unroll
      for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const cpx<T> e = cepstrum_e<T>(x[v][r], S);
          x[v][r] = {e.im, e.re};
        }
    }
    __syncthreads();
    {
      int t4 = tid;
      FOURIER_LAUNDER(t4);
      twolevel_core<T, L2, L1>(x, t4, smem, (const cpx<T>*)a.tw2, (const cpx<T>*)a.tw1, (const cpx<T>*)a.tw_hi, 96);
    }
  }
  // back in the input's layout; the trailing swap: the real part is x.im; streaming stores of the first m
  {
    int tb = tid;
    FOURIER_LAUNDER(tb);
    const uint32_t e0 = (uint32_t)((tb / CG1) * L2 + (tb % CG1) * VEC);
    const bool pairs = VEC == 2 && ((uint64_t)a.out & 7u) == 0 && (m & 1u) == 0;  // (as the load)
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

// `total` half-spectrum values in place: X -> {0.5 log_mult ln(max(|X|^2, floor2)) * scale, 0}
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) cepstrum_log_kernel(CepstrumArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc r = make_rsrc(a.data, a.bytes);
  const cpx<T> X = real_load<T>(r, idx * E);
  const T half = (T)a.log_mult * (T)0.5 * (T)a.scale;
  buf_store_elem<T, BUF_NT>(r, idx * E, cpx<T>{cepstrum_g<T>(X, half, (T)a.floor2, (T)a.g_floor, a.floor_given != 0), (T)0});
}

// rows of l reals in place: c -> chat
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) cepstrum_fold_kernel(CepstrumArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t row = real_div(idx, a.div_m, a.div_l), q = idx - row * a.l;
  if (q == 0 || 2u * q == a.l) return;  // weight 1
  constexpr uint32_t RS = sizeof(T);
  const BufRsrc r = make_rsrc(a.data, a.bytes);
  T y = (T)0;
  if (2u * q < a.l) {
    const T c = buf_load_real<T, BUF_NT>(r, idx * RS);
    y = c + c;
  }
  buf_store_real<T, BUF_NT>(r, idx * RS, y);
}

// `total` half-spectrum values in place: C -> exp(Re C) (cos Im C, sin Im C) * scale
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) cepstrum_exp_kernel(CepstrumArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc r = make_rsrc(a.data, a.bytes);
  buf_store_elem<T, BUF_NT>(r, idx * E, cepstrum_e<T>(real_load<T>(r, idx * E), (T)a.scale));
}

FOURIER_KERNELS_END

namespace fourier_hip {

// cepstrum_small_kernel<T, L1, L2, MINPHASE> with the launch shape and the LDS bytes of the two-level plan of the same length
// (kernels_onelaunch.cpp)
template <typename T, int L1, int L2, bool MINPHASE> static bool cepstrum_small_info(int k, KernelInfo& info) {
  int l1 = 0, l2 = 0;
  if (!get_twolevel_kernel(Real<T>{}, k, info, l1, l2) || l1 != L1 || l2 != L2) return false;
  info.fn = &cepstrum_small_kernel<T, L1, L2, MINPHASE>;
  return true;
}
// every instance, for the translation units that hold them all (kernels_experiments.cpp) or pick from them (kernels_cepstrum.cpp)
template <typename T, bool MINPHASE> static bool cepstrum_small_by_length(int k, KernelInfo& info) {
  switch (k) {
    case 11: return cepstrum_small_info<T, 64, 32, MINPHASE>(k, info);
    case 12: return cepstrum_small_info<T, 64, 64, MINPHASE>(k, info);
    case 13: return cepstrum_small_info<T, 128, 64, MINPHASE>(k, info);
    case 14: return cepstrum_small_info<T, 128, 128, MINPHASE>(k, info);
    case 15:
      if constexpr (sizeof(T) == 4) return cepstrum_small_info<T, 256, 128, MINPHASE>(k, info);
      return false;
    default: return false;
  }
}

}  // namespace fourier_hip
