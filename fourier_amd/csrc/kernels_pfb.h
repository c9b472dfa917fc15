// kernels_pfb.h -- device code of the polyphase filter bank channelizer (PfbPlan, pfb_plan.h).
//
// Frame f of a signal row folds P * T values under the prototype filter h onto P points,
//   u[f, n] = sum_{t < T} h[t P + n] x[f D + t P + n],  n < P,  the taps summed in the order t = 0, 1, ...,
// and X[f, :] is the P-point DFT of u[f, :] (the half spectrum for real rows).  There is no padding: every frame lies inside its row.
//   pfb_fold_kernel       composed route: folds the frames of a chunk into rows of P values (reals, or complex values) in the scratch,
//                         which the inner plan transforms straight into the caller's frame-major output.
//   pfb_rows_kernel       fused route for complex rows, P = L with a whole-row L-point kernel (tile_core in MODE_ROWS, kernels_pass.h): a
//                         workgroup takes COLS consecutive frames of the flat frame index; register r of a frame accumulates the fold of
//                         value m = th + Q*r over a run-time tap loop, the row core runs, whole rows of P bins are stored as
//                         fft_pass_kernel's ROWS store does.
//   pfb_real_rows_kernel  fused route for real rows, P = 2L: the complex value m is (x[2m], x[2m+1]) under the coefficient pair
//                         (h[2m], h[2m+1]), as stft_rows_kernel packs its window; after the row core it untangles through LDS half a tile at
//                         a time (real_post_kernel's formula, kernels_real.h; stft_rows_kernel's epilogue with scale = 1).
//   ipfb_gather_kernel    the synthesis bank (IpfbPlan, ipfb_plan.h): the weighted overlap-add of the inverse-transformed frames of a
//                         chunk as a gather, y[t] = 1/P sum_f g[t - f D] v[f, (t - f D) mod P] in ascending f, one lane per output
//                         sample (or pair of reals), no atomics; as istft_ola_kernel lives beside the STFT's forward kernels.
// The fused routes take one launch, no scratch: the T-fold re-read of every sample comes from the L2 (consecutive frames stay on one XCD), the filter table
// is shared by every frame and stays there too; the bins are written once.  The accumulators are the register tile itself, so the tap
// loop costs address registers only.  The gather and the epilogue stay spelled out, as kernels_frames.h says of the siblings.
#pragma once
#include "kernels_frames.h"

FOURIER_KERNELS_BEGIN

constexpr int PFB_THREADS = 256;

// item i = blockIdx.x of the launch: one frame per workgroup, its P folded values strided over the lanes
template <typename T>
__global__ void __launch_bounds__(PFB_THREADS) pfb_fold_kernel(PfbArgs a) {
  const uint32_t i = blockIdx.x;
  uint32_t row, f;
  frame_of(a, i, row, f);
  const T* filt = (const T*)a.filt;
  const uint64_t t0 = (uint64_t)row * a.length + (uint64_t)f * a.hop, P = a.channels;
  if (a.real) {
    const T* src = (const T*)a.in + t0;
    T* dst = (T*)a.out + (uint64_t)i * P;
    for (uint32_t n = threadIdx.x; n < a.channels; n += PFB_THREADS) {
      T acc = filt[n] * src[n];
      for (uint64_t t = 1; t < a.taps; ++t) acc += filt[t * P + n] * src[t * P + n];
      dst[n] = acc;
    }
  } else {
    const cpx<T>* src = (const cpx<T>*)a.in + t0;
    cpx<T>* dst = (cpx<T>*)a.out + (uint64_t)i * P;
    for (uint32_t n = threadIdx.x; n < a.channels; n += PFB_THREADS) {
      cpx<T> acc = {filt[n] * src[n].re, filt[n] * src[n].im};
      for (uint64_t t = 1; t < a.taps; ++t) {
        const T w = filt[t * P + n];
        const cpx<T> s = src[t * P + n];
        acc.re += w * s.re; acc.im += w * s.im;
      }
      dst[n] = acc;
    }
  }
}

// ---- the synthesis bank's overlap-add (IpfbPlan, ipfb_plan.h; the argument block's comment in kernel_args.h has the geometry)
// One value of the output's kind times a filter coefficient, and the running sum: the same two expressions for every sample, whichever
// store width its lane has, so that a sample's bits do not depend on the launch it falls into.
template <typename T> __device__ __forceinline__ T ipfb_mul(T g, T v) { return g * v; }
template <typename T> __device__ __forceinline__ cpx<T> ipfb_mul(T g, cpx<T> v) { return cpx<T>{g * v.re, g * v.im}; }
template <typename T> __device__ __forceinline__ T ipfb_acc(T acc, T g, T v) { return acc + g * v; }
template <typename T> __device__ __forceinline__ cpx<T> ipfb_acc(cpx<T> acc, T g, cpx<T> v) { return cpx<T>{acc.re + g * v.re, acc.im + g * v.im}; }
template <typename T> __device__ __forceinline__ T ipfb_scaled(T acc, T s) { return acc * s; }
template <typename T> __device__ __forceinline__ cpx<T> ipfb_scaled(cpx<T> acc, T s) { return cpx<T>{acc.re * s, acc.im * s}; }

// the sample u values behind the start of frame fb: `fr` points at that frame of the sample's row.  Three multiply-high divisions in
// front of the frame loop (the last and the first covering frame, the first index within a frame), none inside: m moves by D per frame,
// n = m mod P by D mod P with a conditional add.  Ascending frames, starting from the first term.
template <typename T, typename V> __device__ __forceinline__ V ipfb_sample(const IpfbArgs& a, const V* __restrict__ fr, const T* __restrict__ filt, int64_t u) {
  V zero{};
  if (u < 0 || a.kcount == 0) return zero;  // inside a gap in front of frame fb: no frame covers it
  const uint32_t x = (uint32_t)u, P = a.channels, D = a.hop, dm = a.hop_mod;
  uint32_t k_hi = real_div(x, a.hop_m, a.hop_l);
  const uint32_t k_lo = x >= a.span_pt ? real_div(x - a.span_pt, a.hop_m, a.hop_l) + 1u : 0u;
  if (k_hi > a.kcount - 1u) k_hi = a.kcount - 1u;
  if (k_lo > k_hi) return zero;  // a gap behind frame k_lo - 1, or behind the last frame
  uint32_t m = x - k_lo * D;     // < P T
  uint32_t n = m - real_div(m, a.ch_m, a.ch_l) * P;
  const V* p = fr + (uint64_t)k_lo * P;
  V acc = ipfb_mul(filt[m], p[n]);
  for (uint32_t k = k_lo; k < k_hi; ++k) {
    m -= D;
    n = n >= dm ? n - dm : n + (P - dm);
    p += P;
    acc = ipfb_acc(acc, filt[m], p[n]);
  }
  return ipfb_scaled(acc, (T)a.scale);
}

// One lane per output sample of the launch's range, consecutive lanes consecutive samples: g[m] and the frames' values are read in runs
// (up to the wrap at P), every sample of the range is written once, zeros included, nothing else.  With `pairs` a lane owns two
// neighbouring reals and stores them together; the last lane of an odd range stores one.
template <typename T>
__global__ void __launch_bounds__(PFB_THREADS) ipfb_gather_kernel(IpfbArgs a) {
  const uint32_t idx = blockIdx.x * (uint32_t)PFB_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t row = real_div(idx, a.it_m, a.it_l), j = idx - row * a.items;
  const T* __restrict__ filt = (const T*)a.filt;
  const uint64_t fr0 = ((uint64_t)row * a.nfr + a.q0) * a.channels, o0 = (uint64_t)row * a.length + a.t0;
  if (!a.real) {
    const cpx<T>* fr = (const cpx<T>*)a.in + fr0;
    ((cpx<T>*)a.out)[o0 + j] = ipfb_sample<T, cpx<T>>(a, fr, filt, a.e0 + (int64_t)j);
    return;
  }
  const T* fr = (const T*)a.in + fr0;
  T* out = (T*)a.out + o0;
  if (!a.pairs) {
    out[j] = ipfb_sample<T, T>(a, fr, filt, a.e0 + (int64_t)j);
    return;
  }
  const uint32_t i = 2u * j;
  const T y0 = ipfb_sample<T, T>(a, fr, filt, a.e0 + (int64_t)i);
  if (i + 1u < a.span) {
    const T y1 = ipfb_sample<T, T>(a, fr, filt, a.e0 + (int64_t)i + 1);
    *(cpx<T>*)(out + i) = cpx<T>{y0, y1};
  } else {
    out[i] = y0;
  }
}

// ---- the fused routes
// The launch bounds are the row kernels' own (fft_pass_kernel): the tap loop adds the frames' pointers and a counter to the row core's
// registers, nothing that lives across it ("Polyphase filter bank", has every instance's resources).
template <typename T, int L, int CG>
__global__ void __launch_bounds__((L / 16) * CG, FOURIER_MIN_WAVES((L / 16) * CG)) pfb_rows_kernel(PfbArgs a) {
  using C = TileCfg<T, L, CG>;
  constexpr int VEC = C::VEC, Q = C::Q, COLS = C::COLS;
  static_assert(Q > 1, "pfb rows kernel: L >= 32");
  FOURIER_DYN_SMEM(smem);
  const int tid = (int)threadIdx.x;
  int th = tid % Q, cg = tid / Q;
  // every XCD walks one contiguous range of the flat frame index: the frames that share samples meet in one L2
  const uint32_t blk = real_xcd_block(blockIdx.x, gridDim.x);
  const uint64_t g0 = (uint64_t)blk * COLS;
  const cpx<T>* __restrict__ in = (const cpx<T>*)a.in;
  const T* __restrict__ filt = (const T*)a.filt + th;

  // ---- fold: register r <- sum_t h[t L + m] x[f D + t L + m], m = th + Q*r, of frame cg*VEC + v
  cpx<T> x[VEC][16];
  const cpx<T>* src[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    const uint64_t g = g0 + (uint64_t)(cg * VEC + v);
#pragma unroll
    for (int r = 0; r < 16; ++r) x[v][r] = cpx<T>{0, 0};
    src[v] = nullptr;
    if (g < a.total) {
      uint32_t row, f;
      frame_of(a, (uint32_t)g, row, f);
      src[v] = in + (uint64_t)row * a.length + (uint64_t)f * a.hop + th;
    }
  }
  for (uint32_t t = 0; t < a.taps; ++t) {
    T w[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) w[r] = filt[Q * r];  // plain loads: the table is shared by every frame and stays in the L2
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      if (src[v]) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const cpx<T> s = src[v][Q * r];
          x[v][r].re += w[r] * s.re; x[v][r].im += w[r] * s.im;
        }
        src[v] += L;
      }
    }
    filt += L;
  }

  // ---- X = FFT_P: register r holds X[k], k = th + Q*r, of frame cg*VEC + v
  tile_core<T, L, CG, MODE_ROWS>(x, th, cg, tid, smem, (const cpx<T>*)a.tw1, (const cpx<T>*)a.tw2);

  cpx<T>* __restrict__ out = (cpx<T>*)a.out;
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    const uint64_t g = g0 + (uint64_t)(cg * VEC + v);
    if (g >= a.total) continue;
    cpx<T>* p = out + g * L + th;
#pragma unroll
    for (int r = 0; r < 16; ++r) store_elem<T, PassPolicy<L, MODE_ROWS, CG>::ST == POL_NT>(p + Q * r, x[v][r]);
  }
}

// Four waves per SIMD asked for outright, as stft_rows_kernel does and for its reason: the untangle's addresses on top of the row core.
template <typename T, int L, int CG>
__global__ void __launch_bounds__((L / 16) * CG, 4) pfb_real_rows_kernel(PfbArgs a) {
  using C = TileCfg<T, L, CG>;
  using S = FrameRowsCfg<T, L, CG>;
  constexpr int VEC = C::VEC, Q = C::Q, COLS = C::COLS, HALF = S::HALF, LP = S::LP;
  static_assert(Q > 1 && COLS % 2 == 0, "pfb real rows kernel: L >= 32, an even number of frames per tile");
  FOURIER_DYN_SMEM(smem);
  const int tid = (int)threadIdx.x;
  int th = tid % Q, cg = tid / Q;
  const uint32_t blk = real_xcd_block(blockIdx.x, gridDim.x);
  const uint64_t g0 = (uint64_t)blk * COLS;
  const T* __restrict__ in = (const T*)a.in;
  const cpx<T>* __restrict__ filt = (const cpx<T>*)a.filt + th;  // (h[2m], h[2m+1]) as the complex value m; P = 2L is even: every tap's are aligned

  // ---- fold: register r <- sum_t (h[t P + 2m] x[f D + t P + 2m], h[t P + 2m + 1] x[f D + t P + 2m + 1]), m = th + Q*r, of frame cg*VEC + v
  cpx<T> x[VEC][16];
  const T* src[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    const uint64_t g = g0 + (uint64_t)(cg * VEC + v);
#pragma unroll
    for (int r = 0; r < 16; ++r) x[v][r] = cpx<T>{0, 0};
    src[v] = nullptr;
    if (g < a.total) {
      uint32_t row, f;
      frame_of(a, (uint32_t)g, row, f);
      src[v] = in + (uint64_t)row * a.length + (uint64_t)f * a.hop + 2 * th;
    }
  }
  // registers in groups of G: a tap's coefficient pairs and samples of one group are live together, not all sixteen (which, on top of
  // the tile, is past the 128 registers of four waves per SIMD)
  constexpr int G = sizeof(T) == 4 ? 8 : 4;
  for (uint32_t t = 0; t < a.taps; ++t) {
#pragma unroll
    for (int r0 = 0; r0 < 16; r0 += G) {
      cpx<T> w[G];
#pragma unroll
      for (int q = 0; q < G; ++q) w[q] = filt[Q * (r0 + q)];  // plain loads: the table is shared by every frame and stays in the L2
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        if (!src[v]) continue;
        const T* p = src[v] + 2 * Q * r0;
        // two reals per access where every frame starts on an aligned pair, single reals otherwise
        if (a.pairs) {
#pragma unroll
          for (int q = 0; q < G; ++q) {
            const cpx<T> s = *(const cpx<T>*)(p + 2 * Q * q);
            x[v][r0 + q].re += w[q].re * s.re; x[v][r0 + q].im += w[q].im * s.im;
          }
        } else {
#pragma unroll
          for (int q = 0; q < G; ++q) {
            x[v][r0 + q].re += w[q].re * p[2 * Q * q]; x[v][r0 + q].im += w[q].im * p[2 * Q * q + 1];
          }
        }
      }
      FOURIER_SCHED_FENCE();
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v)
      if (src[v]) src[v] += 2 * L;
    filt += L;
  }

  // ---- Z = FFT_h: register r holds Z[k], k = th + Q*r, of frame cg*VEC + v
  tile_core<T, L, CG, MODE_ROWS>(x, th, cg, tid, smem, (const cpx<T>*)a.tw1, (const cpx<T>*)a.tw2);

  // ---- untangle through LDS, half a tile at a time: X[k] = 1/2 (E + W_P^k O), E = Z[k] + conj Z[h-k], O = -i (Z[k] - conj Z[h-k]);
  // bins 0 and h both come from Z[0].  W_P^k for k > h/2 is -conj W_P^{h-k}: the table stops at P/4.
  cpx<T>* stage = (cpx<T>*)smem;
  const cpx<T>* tw = (const cpx<T>*)a.tw;
  cpx<T>* __restrict__ out = (cpx<T>*)a.out;
  const T s = (T)0.5;
  __syncthreads();  // the last exchange's readers are done with the buffer
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const int col = VEC == 2 ? v * CG + cg : cg;  // position in the staging order: each half one run of HALF frames
      if (col / HALF == hf) {
        cpx<T>* p = stage + (col % HALF) * LP + th;
#pragma unroll
        for (int r = 0; r < 16; ++r) p[Q * r] = x[v][r];
      }
    }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const int col = VEC == 2 ? v * CG + cg : cg;
      const uint64_t g = g0 + (uint64_t)(cg * VEC + v);
      if (col / HALF == hf && g < a.total) {
        const cpx<T>* z = stage + (col % HALF) * LP;
        cpx<T>* dst = out + g * (uint64_t)(L + 1);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int k = th + Q * r;
          const cpx<T> A = x[v][r], P = z[k == 0 ? 0 : L - k];
          const cpx<T> t1 = tw[k <= L / 2 ? k : L - k];
          const cpx<T> w = k <= L / 2 ? t1 : cpx<T>{-t1.re, t1.im};
          const cpx<T> e = {A.re + P.re, A.im - P.im};
          const cpx<T> o = {A.im + P.im, P.re - A.re};
          const cpx<T> t = cmul(w, o);
          // no streaming hint: rows of h + 1 values are only element-aligned, the L2 merges the line halves of neighbouring frames
          store_elem<T, false>(dst + k, cpx<T>{s * (e.re + t.re), s * (e.im + t.im)});
          if (k == 0) store_elem<T, false>(dst + L, cpx<T>{A.re - A.im, (T)0});
        }
      }
    }
    if (hf == 0) __syncthreads();
  }
}

FOURIER_KERNELS_END
