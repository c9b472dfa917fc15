// kernels_real.h -- device code of the real-input transforms (RealPlan, real_plan.h).
//
// Even N = 2h: the N reals of a row are read as h complex values z[m] = x[2m] + i x[2m+1], the inner h-point plan transforms
// them, and one linear sweep untangles the half spectrum:
//   X[k]     = s/2 * (E + W_N^k O),  X[h - k] = s/2 * conj(E - W_N^k O),  E = Z[k] + conj(Z[h-k]),  O = -i (Z[k] - conj(Z[h-k]))
// (Z[h] = Z[0]; k = 0 gives X[0] = s (Re Z0 + Im Z0), X[h] = s (Re Z0 - Im Z0); k = h / 2, h even, is its own partner).  The
// inverse runs the same algebra backwards, Z[k] = f (S + iT), Z[h-k] = f (conj S + i conj T), S = X[k] + conj(X[h-k]),
// T = W_N^-k (X[k] - conj(X[h-k])), and the inner plan's unscaled IFFT of Z is f h (x[2m] + i x[2m+1]).
//
// real_post_kernel / real_pre_kernel are pure streaming sweeps, written like the pass kernels:
//   * one lane per pair (j, h - j): the partner run h - j descends, so a wave still touches one contiguous run of each side;
//   * one element per access (8 bytes f32, 16 bytes f64), through buffer descriptors with non-temporal hints; elements rather
//     than two-element units because the half-spectrum rows have the odd stride h + 1, whose rows start on any 8-byte boundary
//     in f32 -- with element accesses every row is aligned alike and no lane needs a branch on the row's alignment;
//   * the flat index rows x pairs is split with a multiply-high (no 64-bit division per lane), workgroups are remapped so that
//     each XCD (blockIdx % 8) walks one contiguous range of the index, that is of whole rows;
//   * the twiddle table W_N^j (j <= N/4) is read with plain loads: it is shared by every row and stays in the L2.
// The odd-N kernels (widen, narrow, Hermitian extend, real part) belong to the correctness path and are plain grid-stride loops.
#pragma once
#include "kernels_common.h"

FOURIER_KERNELS_BEGIN

constexpr int REAL_THREADS = 256;

// workgroup blk of nwg -> index such that XCD x = blk % 8 owns the x-th contiguous eighth of the grid
__device__ __forceinline__ uint32_t real_xcd_block(uint32_t blk, uint32_t nwg) {
  const uint32_t xcd = blk % 8u, slot = blk / 8u, q = nwg / 8u, r = nwg % 8u;
  return (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + slot;
}
__device__ __forceinline__ uint32_t real_div(uint32_t x, uint32_t m, uint32_t l) {
  const uint32_t hi = (uint32_t)(((uint64_t)x * m) >> 32);
  return (uint32_t)(((uint64_t)hi + x) >> l);
}
template <typename T> __device__ __forceinline__ cpx<T> real_load(BufRsrc r, uint32_t voff) {
  cpx<T> y;
  if constexpr (sizeof(T) == 4) {
    const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, 0, BUF_NT);
    __builtin_memcpy(&y, &v, 8);
  } else {
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, 0, BUF_NT);
    __builtin_memcpy(&y, &v, 16);
  }
  return y;
}

// scratch Z (rows of h) -> half spectrum X (rows of h + 1)
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) real_post_kernel(RealArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t row = real_div(idx, a.div_m, a.div_l), j = idx - row * a.pairs, h = a.h;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  const uint32_t zrow = row * h, xrow = zrow + row;  // row * (h + 1)
  const cpx<T> A = real_load<T>(rin, (zrow + j) * E);
  const cpx<T> P = real_load<T>(rin, (zrow + (j == 0 ? 0 : h - j)) * E);
  const cpx<T> w = ((const cpx<T>*)a.tw)[j];
  const cpx<T> e = {A.re + P.re, A.im - P.im};
  const cpx<T> o = {A.im + P.im, P.re - A.re};  // -i (A - conj P)
  const cpx<T> t = cmul(w, o);
  const T s = (T)a.scale * (T)0.5;
  buf_store_elem<T, BUF_NT>(rout, (xrow + j) * E, cpx<T>{s * (e.re + t.re), s * (e.im + t.im)});
  if (h - j != j) buf_store_elem<T, BUF_NT>(rout, (xrow + h - j) * E, cpx<T>{s * (e.re - t.re), s * (t.im - e.im)});
}

// half spectrum X (rows of h + 1) -> scratch Z (rows of h); the imaginary parts of X[0] and X[h] are ignored
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) real_pre_kernel(RealArgs a) {
  const uint32_t idx = real_xcd_block(blockIdx.x, gridDim.x) * REAL_THREADS + threadIdx.x;
  if (idx >= a.total) return;
  const uint32_t row = real_div(idx, a.div_m, a.div_l), j = idx - row * a.pairs, h = a.h;
  constexpr uint32_t E = sizeof(cpx<T>);
  const BufRsrc rin = make_rsrc(a.in, a.in_bytes), rout = make_rsrc(a.out, a.out_bytes);
  const uint32_t zrow = row * h, xrow = zrow + row;
  cpx<T> A = real_load<T>(rin, (xrow + j) * E);
  cpx<T> P = real_load<T>(rin, (xrow + h - j) * E);
  if (j == 0) { A.im = 0; P.im = 0; }
  const cpx<T> w = ((const cpx<T>*)a.tw)[j];
  const cpx<T> sm = {A.re + P.re, A.im - P.im};                        // S = A + conj P
  const cpx<T> d = {A.re - P.re, A.im + P.im};                         // A - conj P
  const cpx<T> t = {w.re * d.re + w.im * d.im, w.re * d.im - w.im * d.re};  // T = conj(w) d
  const T f = (T)a.scale;
  buf_store_elem<T, BUF_NT>(rout, (zrow + j) * E, cpx<T>{f * (sm.re - t.im), f * (sm.im + t.re)});
  if (j != 0 && h - j != j) buf_store_elem<T, BUF_NT>(rout, (zrow + h - j) * E, cpx<T>{f * (sm.re + t.im), f * (t.re - sm.im)});
}

// ---- N-D, even last length W = 2h (RealNdPlan, realnd_plan.h): the rows are the h-point rows of an item's complex r-D transform
// Z = FFT_r(z), z[.., m] = x[.., 2m] + i x[.., 2m+1]; r' is the mirror row of r (every leading index negated mod its length).  With
// A = Z[r, k], P = conj Z[r', (h - k) mod h], E = (A + P) / 2, O = -i (A - P) / 2:
//   X[r, k] = s (E + W_W^k O),  X[r', h - k] = s conj(E - W_W^k O)
// One lane per k <= h / 2 of a row pair r < r' handles the four outputs (r, k), (r', h - k), (r', k), (r, h - k) from the four
// inputs Z[r, k], Z[r, h - k], Z[r', k], Z[r', h - k], so the table W_W^j (j <= W/4) suffices; the lane of k = 0 also takes k = h / 2
// (h even), which has two outputs only.  A self-mirrored row (r == r') is the 1-D pairing.  Workgroups of rows r > r' return at once:
// their outputs are their mirror's.  The row bases are workgroup-uniform and 64-bit (an item may be larger than 2^31 bytes), the
// offsets within a row 32-bit (rows are bounded as RealPlan's).  Element accesses and non-temporal hints as the 1-D sweeps.
struct RealNdRows { uint64_t r, m; };  // a row and its mirror, counted from the launch base
__device__ __forceinline__ bool realnd_rows(const RealArgs& a, uint32_t& seg, RealNdRows& rows) {
  const uint32_t blk = real_xcd_block(blockIdx.x, gridDim.x);
  const uint32_t row = real_div(blk, a.seg_m, a.seg_l);
  seg = blk - row * a.segs;
  const uint32_t item = real_div(row, a.row_m, a.row_l), r = row - item * a.nd_rows;
  const uint32_t q = real_div(r, a.c_m, a.c_l), ic = r - q * a.nd[2];
  const uint32_t ia = real_div(q, a.b_m, a.b_l), ib = q - ia * a.nd[1];
  const uint32_t ma = ia ? a.nd[0] - ia : 0, mb = ib ? a.nd[1] - ib : 0, mc = ic ? a.nd[2] - ic : 0;
  const uint32_t rm = (ma * a.nd[1] + mb) * a.nd[2] + mc;
  const uint64_t base = (uint64_t)item * a.nd_rows;
  rows = {base + r, base + rm};
  return r <= rm;
}

// scratch Z (items of rows x h) -> half spectrum X (items of rows x (h + 1))
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) realnd_post_kernel(RealArgs a) {
  uint32_t seg;
  RealNdRows rw;
  if (!realnd_rows(a, seg, rw)) return;
  const uint32_t j0 = seg * blockDim.x + threadIdx.x, h = a.h;
  if (j0 >= a.lanes) return;
  constexpr uint32_t E = sizeof(cpx<T>);
  const bool self = rw.r == rw.m;
  const cpx<T>* zin = (const cpx<T>*)a.in;
  cpx<T>* xout = (cpx<T>*)a.out;
  const BufRsrc zr = make_rsrc(zin + rw.r * h, h * E), zm = make_rsrc(zin + rw.m * h, h * E);
  const BufRsrc xr = make_rsrc(xout + rw.r * (h + 1), (h + 1) * E), xm = make_rsrc(xout + rw.m * (h + 1), (h + 1) * E);
  const T s = (T)a.scale * (T)0.5;
  for (uint32_t pass = 0; pass < 2; ++pass) {
    const uint32_t j = pass == 0 ? j0 : h / 2;  // pass 1: the lane of k = 0 also takes k = h / 2 (h even)
    if (pass == 1 && !(j0 == 0 && h % 2 == 0 && h >= 2)) break;
    const uint32_t jm = j == 0 ? 0 : h - j;
    const cpx<T> w = ((const cpx<T>*)a.tw)[j];
    const cpx<T> A = real_load<T>(zr, j * E), P = real_load<T>(zm, jm * E);  // (r, k): Z[r, k], Z[r', h - k]
    const bool mid = 2 * j == h;
    {
      const cpx<T> e = {A.re + P.re, A.im - P.im};
      const cpx<T> o = {A.im + P.im, P.re - A.re};  // -i (A - conj P)
      const cpx<T> t = cmul(w, o);
      buf_store_elem<T, BUF_NT>(xr, j * E, cpx<T>{s * (e.re + t.re), s * (e.im + t.im)});
      if (!mid) buf_store_elem<T, BUF_NT>(xm, (h - j) * E, cpx<T>{s * (e.re - t.re), s * (t.im - e.im)});
    }
    if (!self) {
      const cpx<T> C = real_load<T>(zm, j * E), D = real_load<T>(zr, jm * E);  // (r', k): Z[r', k], Z[r, h - k]
      const cpx<T> e = {C.re + D.re, C.im - D.im};
      const cpx<T> o = {C.im + D.im, D.re - C.re};
      const cpx<T> t = cmul(w, o);
      buf_store_elem<T, BUF_NT>(xm, j * E, cpx<T>{s * (e.re + t.re), s * (e.im + t.im)});
      if (!mid) buf_store_elem<T, BUF_NT>(xr, (h - j) * E, cpx<T>{s * (e.re - t.re), s * (t.im - e.im)});
    }
  }
}

// half spectrum X (items of rows x (h + 1)) -> scratch Z (items of rows x h), the scale folded in:
//   Z[r, k] = f (S + iT),  Z[r', h - k] = f (conj S + i conj T),  S = X[r, k] + conj X[r', h - k],  T = W_W^-k (X[r, k] - conj X[r', h - k])
// Columns 0 and h are first projected over the leading axes, X~[r, 0] = (X[r, 0] + conj X[r', 0]) / 2 (the same for column h): numpy's
// irfftn runs the leading inverses first and its last-axis irfft drops the imaginary parts of bins 0 and h, which is this projection
// (rank 1: "ignore Im X[0], Im X[h]").  So the lane of k = 0 reads X[r, 0], X[r, h], X[r', 0], X[r', h] and writes Z[r, 0], Z[r', 0].
template <typename T>
__global__ void __launch_bounds__(REAL_THREADS) realnd_pre_kernel(RealArgs a) {
  uint32_t seg;
  RealNdRows rw;
  if (!realnd_rows(a, seg, rw)) return;
  const uint32_t j0 = seg * blockDim.x + threadIdx.x, h = a.h;
  if (j0 >= a.lanes) return;
  constexpr uint32_t E = sizeof(cpx<T>);
  const bool self = rw.r == rw.m;
  const cpx<T>* xin = (const cpx<T>*)a.in;
  cpx<T>* zout = (cpx<T>*)a.out;
  const BufRsrc xr = make_rsrc(xin + rw.r * (h + 1), (h + 1) * E), xm = make_rsrc(xin + rw.m * (h + 1), (h + 1) * E);
  const BufRsrc zr = make_rsrc(zout + rw.r * h, h * E), zm = make_rsrc(zout + rw.m * h, h * E);
  const T f = (T)a.scale;
  for (uint32_t pass = 0; pass < 2; ++pass) {
    const uint32_t j = pass == 0 ? j0 : h / 2;
    if (pass == 1 && !(j0 == 0 && h % 2 == 0 && h >= 2)) break;
    const cpx<T> w = ((const cpx<T>*)a.tw)[j];
    cpx<T> A = real_load<T>(xr, j * E), P = real_load<T>(xm, (h - j) * E);  // X[r, k], X[r', h - k]
    cpx<T> C = A, D = P;                                                       // X[r', k], X[r, h - k]
    if (!self) { C = real_load<T>(xm, j * E); D = real_load<T>(xr, (h - j) * E); }
    if (j == 0) {  // the projection of columns 0 and h: A, C from X[r, 0], X[r', 0]; P, D from X[r', h], X[r, h]
      const cpx<T> a0 = {(A.re + C.re) * (T)0.5, (A.im - C.im) * (T)0.5}, ah = {(D.re + P.re) * (T)0.5, (D.im - P.im) * (T)0.5};
      A = a0; C = {a0.re, -a0.im};
      D = ah; P = {ah.re, -ah.im};
    }
    const bool two = j != 0 && 2 * j != h;  // (r', h - k) and (r, h - k) are other outputs
    {
      const cpx<T> sm = {A.re + P.re, A.im - P.im};
      const cpx<T> d = {A.re - P.re, A.im + P.im};
      const cpx<T> t = {w.re * d.re + w.im * d.im, w.re * d.im - w.im * d.re};
      buf_store_elem<T, BUF_NT>(zr, j * E, cpx<T>{f * (sm.re - t.im), f * (sm.im + t.re)});
      if (two) buf_store_elem<T, BUF_NT>(zm, (h - j) * E, cpx<T>{f * (sm.re + t.im), f * (t.re - sm.im)});
    }
    if (!self) {
      const cpx<T> sm = {C.re + D.re, C.im - D.im};
      const cpx<T> d = {C.re - D.re, C.im + D.im};
      const cpx<T> t = {w.re * d.re + w.im * d.im, w.re * d.im - w.im * d.re};
      buf_store_elem<T, BUF_NT>(zm, j * E, cpx<T>{f * (sm.re - t.im), f * (sm.im + t.re)});
      if (two) buf_store_elem<T, BUF_NT>(zr, (h - j) * E, cpx<T>{f * (sm.re + t.im), f * (t.re - sm.im)});
    }
  }
}

// ---- odd N: the full-length complex transform on a widened copy
// x (rows of n reals) -> work (rows of n complex, imaginary parts 0)
template <typename T>
__global__ void __launch_bounds__(256) real_widen_kernel(RealArgs a) {
  const T* x = (const T*)a.in;
  cpx<T>* w = (cpx<T>*)a.out;
  const uint64_t total = a.rows * a.n;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) w[i] = {x[i], (T)0};
}
// work (rows of n) -> X (rows of n / 2 + 1): the first n / 2 + 1 values of every row
template <typename T>
__global__ void __launch_bounds__(256) real_narrow_kernel(RealArgs a) {
  const cpx<T>* w = (const cpx<T>*)a.in;
  cpx<T>* X = (cpx<T>*)a.out;
  const uint64_t hp = a.n / 2 + 1, total = a.rows * hp;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    const uint64_t b = i / hp, k = i - b * hp;
    X[i] = w[b * a.n + k];
  }
}
// X (rows of n / 2 + 1) -> work (rows of n): the Hermitian extension, Im X[0] ignored
template <typename T>
__global__ void __launch_bounds__(256) real_extend_kernel(RealArgs a) {
  const cpx<T>* X = (const cpx<T>*)a.in;
  cpx<T>* w = (cpx<T>*)a.out;
  const uint64_t hp = a.n / 2 + 1, total = a.rows * a.n;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    const uint64_t b = i / a.n, k = i - b * a.n;
    cpx<T> y;
    if (k == 0) y = {X[b * hp].re, (T)0};
    else if (k < hp) y = X[b * hp + k];
    else { const cpx<T> v = X[b * hp + (a.n - k)]; y = {v.re, -v.im}; }
    w[i] = y;
  }
}
// work (rows of n complex) -> x (rows of n reals)
template <typename T>
__global__ void __launch_bounds__(256) real_part_kernel(RealArgs a) {
  const cpx<T>* w = (const cpx<T>*)a.in;
  T* x = (T*)a.out;
  const uint64_t total = a.rows * a.n;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) x[i] = w[i].re;
}

FOURIER_KERNELS_END
