// kernels_regstage.h -- the pieces the register-stage kernels are built from (kernels_chirpz.h: chirpz_reg_kernel, chirpz_reg3_kernel;
// kernels_regfft.h: regfft_kernel, regfft3_kernel): the lane value types, the launch-bound rule, the LDS put / get / exchange and the batched table
// product.  Every piece is force-inlined into the kernel that names it; the kernels keep their lane mappings, tables and access-site numbers.
// The stage loads and stores through the buffer descriptors, three of chirpz_reg3_kernel's LDS writers and regfft_kernel's reader stay written
// out in the kernels: hipcc orders the operands of the butterflies' multiply-adds by the shape of the address and swap expressions around them,
// and a shared form of those changed which product of a complex multiply is fused -- the rounding -- or commuted adds.  Which call sites are
// neutral was found by comparing device assembly per kernel, not derived: a site that is neutral alone may not be with its neighbours.
#pragma once
#include "kernels_regtile.h"

namespace fourier_hip {

// two f32 values, one per transform of the lane: arithmetic on both at once
typedef float v2f_t __attribute__((vector_size(8)));
struct Pk2 {
  v2f_t v;
  Pk2() = default;
  __device__ __forceinline__ explicit Pk2(double s) : v{(float)s, (float)s} {}
  __device__ __forceinline__ Pk2(v2f_t w) : v(w) {}
};
__device__ __forceinline__ Pk2 operator+(Pk2 a, Pk2 b) { return Pk2(a.v + b.v); }
__device__ __forceinline__ Pk2 operator-(Pk2 a, Pk2 b) { return Pk2(a.v - b.v); }
__device__ __forceinline__ Pk2 operator*(Pk2 a, Pk2 b) { return Pk2(a.v * b.v); }
__device__ __forceinline__ Pk2 operator-(Pk2 a) { return Pk2(-a.v); }
__device__ __forceinline__ Pk2 operator*(Pk2 a, float s) { return Pk2(a.v * v2f_t{s, s}); }
// lane value type P over memory type T: T itself (one transform per lane) or Pk2 over float (two)
template <typename P, typename T> struct LaneVal {
  static constexpr uint32_t NV = 1;
  static __device__ __forceinline__ P make(const T* s) { return s[0]; }
  static __device__ __forceinline__ T get(P p, uint32_t) { return p; }
};
template <> struct LaneVal<Pk2, float> {
  static constexpr uint32_t NV = 2;
  static __device__ __forceinline__ Pk2 make(const float* s) { return Pk2(v2f_t{s[0], s[1]}); }
  static __device__ __forceinline__ float get(Pk2 p, uint32_t v) { return p.v[v]; }
};
// a lane value times a table entry (one per lane, shared by the lane's transforms)
template <typename P, typename T> __device__ __forceinline__ cpx<P> cmul_tab(cpx<P> a, cpx<T> w) {
  return {a.re * w.re - a.im * w.im, a.re * w.im + a.im * w.re};
}
template <bool B, typename X, typename Y> struct ChirpzSelect { typedef X type; };
template <typename X, typename Y> struct ChirpzSelect<false, X, Y> { typedef Y type; };

// the lane values of a kernel over T: f32 runs TWO transforms per lane on packed arithmetic unless PAIR = false (kernels_chirpz.h, kernels_regfft.h)
template <typename T, bool PAIR = true> struct RegStageLane {
  static constexpr bool VEC2 = sizeof(T) == 4 && PAIR;
  using P = typename ChirpzSelect<VEC2, Pk2, T>::type;
  static constexpr uint32_t NV = VEC2 ? 2u : 1u;
};
// waves per SIMD the register allocation aims at: what the LDS lets a compute unit hold (160 KiB, four SIMDs; workgroups of `waves` waves and
// `smem` bytes), at least one, at most `cap`
constexpr uint32_t regstage_min_waves(size_t smem, uint32_t waves, uint32_t cap) {
  const uint32_t w = (uint32_t)((160u * 1024u) / smem) * waves / 4u;
  return w < 1u ? 1u : (w < cap ? w : cap);
}
constexpr uint32_t chirpz3_pitch_runs(uint32_t lanes, uint32_t run) {  // >= lanes, = run (mod 16)
  uint32_t p = lanes;
  while (p % 16u != run % 16u) ++p;
  return p;
}

// LDS put / get: the lane's R values at element idx(i) of the buffer; `site` names the access in the emulator's LDS trace.  WHOLE complex
// values, or their real / imaginary parts alone in a buffer of P (the imaginary plane repeats the real plane's addresses and is not traced).
enum { LDS_WHOLE = 0, LDS_RE = 1, LDS_IM = 2 };
template <uint32_t R, int PART = LDS_WHOLE, typename P, typename IDX>
__device__ __forceinline__ void regstage_put(void* buf, const cpx<P>* v, IDX idx, int site) {
#pragma unroll
  for (uint32_t i = 0; i < R; ++i) {
    if constexpr (PART == LDS_WHOLE) {
      cpx<P>* p = (cpx<P>*)buf + idx(i);
      LDS_NOTE(p, (uint32_t)sizeof(cpx<P>), true, site);
      *p = v[i];
    } else {
      P* p = (P*)buf + idx(i);
      if constexpr (PART == LDS_RE) { LDS_NOTE(p, (uint32_t)sizeof(P), true, site); }
      *p = PART == LDS_RE ? v[i].re : v[i].im;
    }
  }
  (void)site;
}
template <uint32_t R, int PART = LDS_WHOLE, typename P, typename IDX>
__device__ __forceinline__ void regstage_get(const void* buf, cpx<P>* v, IDX idx, int site) {
#pragma unroll
  for (uint32_t i = 0; i < R; ++i) {
    if constexpr (PART == LDS_WHOLE) {
      const cpx<P>* p = (const cpx<P>*)buf + idx(i);
      LDS_NOTE(p, (uint32_t)sizeof(cpx<P>), false, site);
      v[i] = *p;
    } else {
      const P* p = (const P*)buf + idx(i);
      if constexpr (PART == LDS_RE) { LDS_NOTE(p, (uint32_t)sizeof(P), false, site); }
      (PART == LDS_RE ? v[i].re : v[i].im) = *p;
    }
  }
  (void)site;
}
// one exchange: the writer lanes put their RW values at widx(i) (site), barrier, the reader lanes take their RR values from ridx(i) (site + 1).
// SPLIT: the real parts, then the imaginary parts, through a buffer of half the size (two more barriers)
template <bool SPLIT, uint32_t RW, uint32_t RR, typename P, typename WI, typename RI>
__device__ __forceinline__ void regstage_exchange(void* buf, bool writer, bool reader, const cpx<P>* w, cpx<P>* r, WI widx, RI ridx, int site) {
  if constexpr (!SPLIT) {
    if (writer) regstage_put<RW>(buf, w, widx, site);
    __syncthreads();
    if (reader) regstage_get<RR>(buf, r, ridx, site + 1);
  } else {
    if (writer) regstage_put<RW, LDS_RE>(buf, w, widx, site);
    __syncthreads();
    if (reader) regstage_get<RR, LDS_RE>(buf, r, ridx, site + 1);
    __syncthreads();
    if (writer) regstage_put<RW, LDS_IM>(buf, w, widx, site);
    __syncthreads();
    if (reader) regstage_get<RR, LDS_IM>(buf, r, ridx, site + 1);
  }
}

// y[r] *= tab[r * stride] for first <= r < R (swap: re <-> im afterwards), the loads in batches of TB, each issued one batch ahead of its use
template <typename P, typename T, uint32_t R, uint32_t TB> __device__ __forceinline__ void chirpz_table_product(cpx<P>* y, const cpx<T>* tab, uint32_t stride, bool swap) {
  constexpr uint32_t NB = (R + TB - 1) / TB;
  cpx<T> t[2][TB];
#pragma unroll
  for (uint32_t i = 0; i < TB; ++i)
    if (i < R) t[0][i] = tab[i * stride];
#pragma unroll
  for (uint32_t b = 0; b < NB; ++b) {
    if (b + 1 < NB) {
#pragma unroll
      for (uint32_t i = 0; i < TB; ++i)
        if ((b + 1) * TB + i < R) t[(b + 1) & 1u][i] = tab[((b + 1) * TB + i) * stride];
    }
    FOURIER_SCHED_FENCE();
#pragma unroll
    for (uint32_t i = 0; i < TB; ++i)
      if (b * TB + i < R) {
        const cpx<P> z = cmul_tab(y[b * TB + i], t[b & 1u][i]);
        y[b * TB + i] = swap ? cpx<P>{z.im, z.re} : z;
      }
    FOURIER_SCHED_FENCE();
  }
}

}  // namespace fourier_hip
