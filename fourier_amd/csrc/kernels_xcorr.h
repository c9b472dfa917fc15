// kernels_xcorr.h -- device code of the cross-correlation handle (XcorrPlan, xcorr_plan.h): of rows x and y of n values, zero-extended
// to L, r = ifft(conj(fft(x)) fft(y) psi), psi = 1 or the phase transform 1 / (|X| |Y|) (GCC-PHAT), and a window of its lags.
//
// xcorr_small_kernel: the whole chain for two REAL rows in ONE launch for L = L1 x L2 = 2^11 ... 2^15 (f64: ... 2^14), on
// hilbert_small_kernel's skeleton (kernels_hilbert.h).  It loads x as the real and y as the imaginary registers, so that ONE forward
// transform serves both: Z = X + i Y, and with Z[k] = a + ib and the partner Z[(L - k) mod L] = c + id
//   X = ((a + c) + i (b - d)) / 2,  Y = ((b + d) + i (c - a)) / 2,  conj(X) Y = (ad + bc) / 2 + i (c^2 + d^2 - a^2 - b^2) / 4.
// After the forward core register r of lane (th2, cg2) holds k = k1 + L1 k2, k1 = cg2 VEC + v, k2 = th2 + Q2 r; the partner, k1' =
// (L1 - k1) mod L1 and k2' = L2 - 1 - k2 (k1 = 0: (L2 - k2) mod L2), sits in another lane: the MIRROR EXCHANGE stages the row in the LDS
// area of the inter-pass transpose (TwolevelTr<T, L1, L2>::BYTES: one plane of a row on every one-launch shape, so the exchange runs
// once for the real and once for the imaginary parts, the partner's real parts kept in registers between the two) and every lane reads
// its partners.
// The image: value (slot v, k1 group g, k2) at v CG2 (L2 + 1) + g (L2 + 1) + k2, one value per access.  A wave's lanes walk g first,
// stride L2 + 1 values, an odd number of banks (f64: of bank pairs), in the write and, descending, in the mirrored read: conflict-free
// but for the lane that holds k1 = 0, whose partner row is one further (2-way at most; the figures are in DESIGN.md section 4).
// G is Hermitian, so the inverse's result is real: only that part is stored, lag t at output position (t - lag_first) mod L where
// that lies inside the window.  One workgroup reads both whole rows before it stores anything.
//
// The packed transform rounds x and y against each other, so the kernel BALANCES the two rows first: a workgroup reduction finds each
// row's peak, each row is scaled by the power of two that brings its peak into [1, 2), and the product of the two powers goes back
// onto the unweighted result at the store (PHAT needs none); a pair with an all-zero row stores exact zeros.  Powers of two are exact:
// scaling either input by one leaves every bit of the transform chain as it was.  What the packing cannot give is PHAT's exact 0 in a
// SINGLE bin where one spectrum vanishes and the other does not: X[k] is a difference of two roundings there, and the bin keeps a unit
// phasor.  The sum of the two exponents and the empty-row flag wait in 16 bytes of LDS behind the core's area, not in registers.
//
// The sweeps of the composed routes are written like hilbert_expand_kernel: one element per access through buffer descriptors with
// non-temporal hints, the flat index split by multiply-high, XCD-contiguous workgroups.  REAL: the values are reals, else complex.
#pragma once
#include "kernels_hilbert.h"

FOURIER_KERNELS_BEGIN

// conj(X / |X|) (Y / |Y|): the two unit phasors are formed apart, quotients first (as the coherence); 0 where a magnitude is 0
template <typename T> __device__ __forceinline__ cpx<T> xcorr_phat(cpx<T> X, cpx<T> Y) {
  const T mx = hilbert_abs(X.re, X.im), my = hilbert_abs(Y.re, Y.im);
  if (mx == (T)0 || my == (T)0) return cpx<T>{(T)0, (T)0};
  const cpx<T> u = {X.re / mx, X.im / mx}, w = {Y.re / my, Y.im / my};
  return cpx<T>{u.re * w.re + u.im * w.im, u.re * w.im - u.im * w.re};
}

// LDS bytes of the two-level core of an L1 x L2 plan (make_twolevel_info, kernels_onelaunch.cpp); the kernel asks for 16 more
template <typename T, int L1, int L2> constexpr size_t xcorr_core_bytes() {
  constexpr int VEC = 16 / (2 * (int)sizeof(T));
  constexpr size_t a = TileCfg<T, L1, L2 / VEC>::EXCH_BYTES, b = TileCfg<T, L2, L1 / VEC>::EXCH_BYTES;
  constexpr size_t c = TwolevelTr<T, L1, L2>::BYTES, d = TwolevelTr<T, L2, L1>::BYTES;
  return (a > b ? a : b) > (c > d ? c : d) ? (a > b ? a : b) : (c > d ? c : d);
}

// floor(log2(peak)) of a row's peak magnitude; 0 for an empty row and for a peak that is not finite
template <typename T> __device__ __forceinline__ int xcorr_exponent(T peak) {
  if (!(peak > (T)0) || !(peak <= std::numeric_limits<T>::max())) return 0;
  int e = 0;
  (void)frexp(peak, &e);
  return e - 1;
}

// xcorr_phat for spectra of any amplitude (the composed route, whose rows are not balanced): each value is first scaled by the power
// of two that brings its larger component into [1, 2), so that re^2 + im^2 neither overflows nor vanishes wherever X and Y are
// normal numbers.  A power of two changes no bit of the square root or of the quotients while nothing leaves the normal range: the
// result is the unscaled one's bit for bit wherever that one was right.  A zero component stays zero, a zero value gives 0, and a
// component that is not finite leaves the value as it is (xcorr_exponent returns 0).
template <typename T> __device__ __forceinline__ cpx<T> xcorr_unit_scale(cpx<T> X) {
  const T ar = X.re < (T)0 ? -X.re : X.re, ai = X.im < (T)0 ? -X.im : X.im;
  const int e = xcorr_exponent(ar > ai ? ar : ai);
  return cpx<T>{(T)ldexp(X.re, -e), (T)ldexp(X.im, -e)};
}
template <typename T> __device__ __forceinline__ cpx<T> xcorr_phat_any(cpx<T> X, cpx<T> Y) {
  return xcorr_phat<T>(xcorr_unit_scale<T>(X), xcorr_unit_scale<T>(Y));
}

// G[k] / N from Z[k] = (a, b) and Z[(N - k) mod N] = (c, d), with the inverse's leading swap re <-> im
template <typename T, bool PHAT, int N> __device__ __forceinline__ cpx<T> xcorr_untangle_swapped(T a, T b, T c, T d) {
  if constexpr (PHAT) {
    // (the halves of X and Y are powers of two and cancel in the phasors)
    const cpx<T> g = xcorr_phat<T>(cpx<T>{a + c, b - d}, cpx<T>{b + d, c - a});
    constexpr T S = (T)1 / (T)N;
    return cpx<T>{g.im * S, g.re * S};
  } else {
    constexpr T S2 = (T)0.5 / (T)N, S4 = (T)0.25 / (T)N;
    return cpx<T>{(c * c + d * d - a * a - b * b) * S4, (a * d + b * c) * S2};
  }
}

template <typename T, int L1, int L2, bool PHAT>
__global__ void __launch_bounds__(FOURIER_TWOLEVEL_NT(T, L1, L2), FOURIER_BLU_SMALL_MIN_WAVES(FOURIER_TWOLEVEL_NT(T, L1, L2)))
    xcorr_small_kernel(PassArgs a) {
  constexpr int VEC = 16 / (2 * (int)sizeof(T));
  constexpr int CG1 = L2 / VEC, CG2 = L1 / VEC, Q1 = L1 / 16, Q2 = L2 / 16, N = L1 * L2;
  FOURIER_DYN_SMEM(smem);
  const int tid = (int)threadIdx.x;
  const uint64_t blk = onelaunch_block(a);
  constexpr uint32_t RS = (uint32_t)sizeof(T);
  const uint32_t n = a.xc_n, lags = a.xc_lags;
  const BufRsrc rx = make_rsrc((const T*)a.in + blk * n, n * RS);  // positions n ... N - 1 load as zeros
  const BufRsrc ry = make_rsrc((const T*)a.xc_in2 + blk * n, n * RS);
  const BufRsrc ro = make_rsrc((T*)a.out + blk * lags, lags * RS);
  constexpr uint32_t ROW = (uint32_t)(Q1 * L2);  // register r holds index (th + Q1*r)*L2 + cg*VEC + v
  cpx<T> x[VEC][16];
  {
    const int th = tid / CG1, cg = tid % CG1;
    const uint32_t e0 = (uint32_t)(th * L2 + cg * VEC);
    // f32: a lane's two adjacent reals in one 8-byte access where both inputs are 8-byte aligned and the rows are whole multiples of
    // 8 bytes (wave-uniform; hilbert_small_kernel's `pairs`); n is even then, so a pair lies wholly below n or wholly above
    const bool pairs = VEC == 2 && (((uint64_t)a.in | (uint64_t)a.xc_in2) & 7u) == 0 && (n & 1u) == 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const uint32_t off = (e0 + (uint32_t)r * ROW) * RS;
      if constexpr (VEC == 2) {
        if (pairs) {
          const cpx<T> p = buf_load_pair<T, BUF_NT>(rx, off), q = buf_load_pair<T, BUF_NT>(ry, off);
          x[0][r] = {p.re, q.re};
          x[1][r] = {p.im, q.im};
          continue;
        }
      }
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        x[v][r] = {buf_load_real<T, BUF_NT>(rx, off + (uint32_t)v * RS), buf_load_real<T, BUF_NT>(ry, off + (uint32_t)v * RS)};
    }
  }
  {  // balance the rows: the peaks of x and of y over the workgroup (lane, 32 lanes, all), each row times 2^-floor(log2(peak))
    constexpr int NT = FOURIER_TWOLEVEL_NT(T, L1, L2);
    static_assert(NT >= 32 && (size_t)(2 * NT + 64) * sizeof(T) <= xcorr_core_bytes<T, L1, L2>(), "the reduction fits the core's area");
    T px = (T)0, py = (T)0;
#pragma unroll
    for (int v = 0; v < VEC; ++v)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const T ax = x[v][r].re < (T)0 ? -x[v][r].re : x[v][r].re, ay = x[v][r].im < (T)0 ? -x[v][r].im : x[v][r].im;
        px = ax > px ? ax : px;
        py = ay > py ? ay : py;
      }
    T* red = (T*)smem;
    red[2 * tid] = px;
    red[2 * tid + 1] = py;
    __syncthreads();
    if (tid < 32) {
      for (int j = tid + 32; j < NT; j += 32) {
        px = red[2 * j] > px ? red[2 * j] : px;
        py = red[2 * j + 1] > py ? red[2 * j + 1] : py;
      }
      red[2 * NT + 2 * tid] = px;
      red[2 * NT + 2 * tid + 1] = py;
    }
    __syncthreads();
    px = py = (T)0;
    for (int j = 0; j < 32; ++j) {
      px = red[2 * NT + 2 * j] > px ? red[2 * NT + 2 * j] : px;
      py = red[2 * NT + 2 * j + 1] > py ? red[2 * NT + 2 * j + 1] : py;
    }
    const int ex = xcorr_exponent(px), ey = xcorr_exponent(py);
    if (tid == 0) {
      int* keep = (int*)(smem + xcorr_core_bytes<T, L1, L2>());
      keep[0] = ex + ey;
      keep[1] = px == (T)0 || py == (T)0;  // an all-zero row: the result is exactly zero (the packed spectra would leave rounding noise)
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v)
#pragma unroll
      for (int r = 0; r < 16; ++r) x[v][r] = {ldexp(x[v][r].re, -ex), ldexp(x[v][r].im, -ey)};
    __syncthreads();  // the reduction's reads are done before the core writes the area
  }
  twolevel_core<T, L1, L2>(x, tid, smem, (const cpx<T>*)a.tw1, (const cpx<T>*)a.tw2, (const cpx<T>*)a.tw_lo, 0);
  {  // the mirror exchange and the weighted product, then the inverse's leading swap
    int tb = tid;
    FOURIER_LAUNDER(tb);
    const int th2 = tb / CG2, cg2 = tb % CG2;
    // every one-launch shape exchanges one plane at a time: the transpose's area holds the real OR the imaginary parts of a row
    static_assert(TwolevelTr<T, L1, L2>::SPLIT && (size_t)VEC * CG2 * (L2 + 1) * sizeof(T) <= TwolevelTr<T, L1, L2>::BYTES, "one plane fits");
    constexpr int LD = L2 + 1, SLOT = CG2 * LD;  // values per k1 group (odd), values per slot v
    T* img = (T*)smem;
    T c[VEC][16];  // the partners' real parts, kept between the two planes
    __syncthreads();  // the reads of the core's last exchange are done
#pragma unroll
    for (int plane = 0; plane < 2; ++plane) {
      if (plane == 1) __syncthreads();
#pragma unroll
      for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          T* p = img + v * SLOT + cg2 * LD + th2 + Q2 * r;
          LDS_NOTE(p, sizeof(T), true, 66 + plane);
          *p = plane ? x[v][r].im : x[v][r].re;
        }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const int k1 = cg2 * VEC + v, k1p = (L1 - k1) & (L1 - 1);
          const int k2 = th2 + Q2 * r, k2p = k1 == 0 ? ((L2 - k2) & (L2 - 1)) : L2 - 1 - k2;
          const T* p = img + (k1p % VEC) * SLOT + (k1p / VEC) * LD + k2p;
          LDS_NOTE(p, sizeof(T), false, 68 + plane);
          if (plane == 0) c[v][r] = *p;
          else x[v][r] = xcorr_untangle_swapped<T, PHAT, N>(x[v][r].re, x[v][r].im, c[v][r], *p);
        }
    }
  }
  __syncthreads();
  {
    int t2 = tid;
    FOURIER_LAUNDER(t2);  // the inverse's lane mappings are derived here, not carried through the forward transform
    twolevel_core<T, L2, L1>(x, t2, smem, (const cpx<T>*)a.tw2, (const cpx<T>*)a.tw1, (const cpx<T>*)a.tw_hi, 32);
  }
  // back in the input's layout; the trailing swap: r[t] = x.im (the result is real); streaming stores of the window
  {
    int tb = tid;
    FOURIER_LAUNDER(tb);
    const uint32_t e0 = (uint32_t)((tb / CG1) * L2 + (tb % CG1) * VEC);
    const uint32_t shift = (uint32_t)N - a.xc_first;  // position of lag t: (t - first) mod N
    {  // the two balancing powers back onto the unweighted result; exact zeros where a row was empty.  The peak's comparisons are
       // false for a NaN, so a row of nothing but NaN and zeros counts as empty too: v - v is +0 for every finite v and keeps that
       // row's result NaN, as the composed route does
      const int* keep = (const int*)(smem + xcorr_core_bytes<T, L1, L2>());
      const int e = PHAT ? 0 : keep[0];
      const bool empty = keep[1] != 0;
#pragma unroll
      for (int v = 0; v < VEC; ++v)
#pragma unroll
        for (int r = 0; r < 16; ++r) x[v][r].im = empty ? x[v][r].im - x[v][r].im : ldexp(x[v][r].im, e);
    }
    // f32: an even shift keeps a lane's two lags adjacent and on an even position; rows of an even number of lags at an 8-byte
    // aligned base make that one 8-byte store that lies wholly inside the window or wholly outside (wave-uniform)
    const bool pairs = VEC == 2 && ((uint64_t)a.out & 7u) == 0 && ((lags | a.xc_first) & 1u) == 0;
    constexpr uint32_t REJECT = 0xfffffff0u;  // beyond every descriptor range: the store is dropped
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const uint32_t j = (e0 + (uint32_t)r * ROW + shift) & (uint32_t)(N - 1);
      if constexpr (VEC == 2) {
        if (pairs) {
          buf_store_elem<T, BUF_NT>(ro, j < lags ? j * RS : REJECT, cpx<T>{x[0][r].im, x[1][r].im});
          continue;
        }
      }
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const uint32_t jv = (j + (uint32_t)v) & (uint32_t)(N - 1);
        buf_store_real<T, BUF_NT>(ro, jv < lags ? jv * RS : REJECT, x[v][r].im);
      }
    }
  }
}

// one value of a sweep: a real or a complex value at index i of the range behind r
template <typename T, bool REAL> struct XcorrValue {
  typedef typename std::conditional<REAL, T, cpx<T>>::type V;
  static constexpr uint32_t BYTES = (uint32_t)sizeof(V);
  static __device__ __forceinline__ V zero() {
    if constexpr (REAL) return (T)0; else return cpx<T>{(T)0, (T)0};
  }
  static __device__ __forceinline__ V load(BufRsrc r, uint32_t i) {
    if constexpr (REAL) return buf_load_real<T, BUF_NT>(r, i * BYTES); else return real_load<T>(r, i * BYTES);
  }
  static __device__ __forceinline__ void store(BufRsrc r, uint32_t i, V y) {
    if constexpr (REAL) buf_store_real<T, BUF_NT>(r, i * BYTES, y); else buf_store_elem<T, BUF_NT>(r, i * BYTES, y);
  }
};

// rows of n values -> rows of l values, zeros from n on; one lane per output value
template <typename T, bool REAL>
__global__ void __launch_bounds__(REAL_THREADS) xcorr_pad_kernel(XcorrArgs a) {
  typedef XcorrValue<T, REAL> V;
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t row = real_div(idx, a.div_m, a.div_l), t = idx - row * a.l;
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  typename V::V y = V::zero();
  if (t < a.n) y = V::load(rin, row * a.n + t);
  V::store(rout, idx, y);
}

// `total` spectrum values: conj(X) Y psi * scale; out may be Y
template <typename T, bool PHAT>
__global__ void __launch_bounds__(REAL_THREADS) xcorr_mul_kernel(XcorrArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc rx = make_rsrc(a.in, a.in_bytes), ry = make_rsrc(a.in2, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  const cpx<T> X = real_load<T>(rx, idx * E), Y = real_load<T>(ry, idx * E);
  cpx<T> g;
  if constexpr (PHAT) g = xcorr_phat_any<T>(X, Y);
  else g = cpx<T>{X.re * Y.re + X.im * Y.im, X.re * Y.im - X.im * Y.re};
  const T s = (T)a.scale;
  buf_store_elem<T, BUF_NT>(rout, idx * E, cpx<T>{g.re * s, g.im * s});
}

// rows of l values r -> rows of `lags` values r[(first + j) mod l]; one lane per output value
template <typename T, bool REAL>
__global__ void __launch_bounds__(REAL_THREADS) xcorr_window_kernel(XcorrArgs a) {
  typedef XcorrValue<T, REAL> V;
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t row = real_div(idx, a.div_m, a.div_l), j = idx - row * a.lags;
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  uint32_t t = a.first + j;  // first < l, j < lags <= l
  if (t >= a.l) t -= a.l;
  V::store(rout, idx, V::load(rin, row * a.l + t));
}

FOURIER_KERNELS_END

namespace fourier_hip {

// xcorr_small_kernel<T, L1, L2, PHAT> with the launch shape of the two-level plan of the same length (kernels_onelaunch.cpp) and its
// LDS bytes + 16; for the translation units that instantiate it (kernels_xcorr.cpp, kernels_experiments.cpp)
template <typename T, int L1, int L2, bool PHAT> static bool xcorr_small_info(int k, KernelInfo& info) {
  int l1 = 0, l2 = 0;
  if (!get_twolevel_kernel(Real<T>{}, k, info, l1, l2) || l1 != L1 || l2 != L2) return false;
  if (info.smem != xcorr_core_bytes<T, L1, L2>()) return false;
  info.smem += 16;  // where the balancing exponent waits
  info.fn = &xcorr_small_kernel<T, L1, L2, PHAT>;
  return true;
}
template <typename T, bool PHAT> static bool xcorr_small_by_length(int k, KernelInfo& info) {
  switch (k) {
    case 11: return xcorr_small_info<T, 64, 32, PHAT>(k, info);
    case 12: return xcorr_small_info<T, 64, 64, PHAT>(k, info);
    case 13: return xcorr_small_info<T, 128, 64, PHAT>(k, info);
    case 14: return xcorr_small_info<T, 128, 128, PHAT>(k, info);
    case 15:
      if constexpr (sizeof(T) == 4) return xcorr_small_info<T, 256, 128, PHAT>(k, info);
      return false;
    default: return false;
  }
}

}  // namespace fourier_hip
