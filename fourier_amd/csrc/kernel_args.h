// kernel_args.h -- argument blocks of the kernels (passed by value) and the enums that name their modes: what the host
// translation unit needs to know about a kernel family without seeing its device code.
#pragma once
#ifdef __HIPCC_RTC__  // hipRTC (rtc.cpp): no system headers; its built-in runtime header is already in
typedef unsigned char uint8_t; typedef unsigned int uint32_t; typedef unsigned long long uint64_t; typedef int int32_t;
#else
#include <stdint.h>
#endif

namespace fourier_hip {

template <typename T> struct cpx { T re, im; };

enum { MODE_FIRST = 0, MODE_MID = 1, MODE_LAST = 2, MODE_ROWS = 3 };
// Bluestein fusion (bluesteins.rs:229-258): IO_BLU_IN = the first pass of the forward inner FFT reads the
// USER array (length blu_n, zero padded to n) times the chirp x; IO_BLU_OUT = the last pass of the inverse
// inner FFT writes the first blu_n points times the chirp (and the user scaling) into the USER array.
enum { IO_PLAIN = 0, IO_BLU_IN = 1, IO_BLU_OUT = 2 };


// Kernel argument block (passed by value).
struct PassArgs {
  const void* in;
  void* out;
  const void* tw1;    // [Q][16]  W_L^{th*k}            (stage-1 twiddles)
  const void* tw2;    // [R3][16] W_Q^{i*k}             (stage-2 twiddles, only when R3 > 1)
  const void* tw_lo;  // W_size^{e},          e < 2^lo_bits     } two-level table of the
  const void* tw_hi;  // W_size^{h<<lo_bits}, h < size>>lo_bits } inter-pass twiddle W_size^{i*k}
  const void* tw_half;  // split tiles: W_2L^{n}, n < L (the radix-2 decimation-in-frequency twiddle in front of a length-L tile)
  const void* mul;    // Bluestein kernels (conv / one-launch): the transformed chirp w, indexed like the M-point spectrum
  uint64_t n;         // elements per transform (batch stride)
  uint64_t cn;        // columns of this pass = n / L
  uint64_t s;         // Stockham stride = product of the previous passes' lengths (a power of two for the tile passes)
  uint32_t s_shift;   // log2(s)
  uint64_t tiles;     // column tiles per transform = cn / COLS
  uint64_t total_cols;  // ROWS mode: number of transforms in this launch
  uint32_t lo_bits;
  uint32_t nxcd;      // >1: remap blockIdx so that each XCD (blockIdx % nxcd) walks a contiguous tile range
  uint32_t xcd_interleave;  // block -> tile mapping mode, see xcd_remap()
  uint32_t walk_band, walk_group, walk_tf;  // mode 4: tiles per band, transforms per group (0 = the XCD's whole range), transform-fastest
  const void* blu_x;  // Bluestein chirp table x[0..blu_n) (IO_BLU_IN / IO_BLU_OUT)
  // chirp-in pass WITHOUT the n-entry chirp table (a quarter of that pass's HBM-side traffic when read, PMC round 3):
  // index k = row*cn + b, so x[k] = W_2n^{k^2} = blu_p[row] * blu_u[b] * W_n^{cn*row*b}; the cross term splits like the
  // pass's own inter-pass twiddle into a per-thread factor and a per-tile LDS table, both from a two-level table of n-th
  // roots with EXACT integer exponents (f64 products below 2^53).  blu_p == nullptr selects the table read.
  const void* blu_p;     // [L/2]  W_2n^{(row*cn)^2 mod 2n}
  const void* blu_u;     // [cn]   W_2n^{b^2 mod 2n}
  const void* tn_lo;     // W_n^{e},            e < 2^tn_bits      } two-level table of n-th roots
  const void* tn_hi;     // W_n^{h << tn_bits}, h <= n >> tn_bits  }
  uint32_t tn_bits;
  uint32_t blu_cn_mod;   // cn mod n
  uint32_t blu_cnq_mod;  // (cn * Q) mod n
  double blu_nd, blu_inv_nd;  // n and 1/n as doubles
  uint64_t blu_n;     // user transform length (batch stride of the user-side buffer)
  int blu_swap;       // user-level inverse: swap re/im of the user data
  int swap_in, swap_out;
  double scale;       // applied on the final store (LAST / ROWS)
  // fft_conv_kernel with a filter bank (ConvPlan, conv_plan.h): transform b of this launch multiplies by the table at
  // mul + ((bank_first + b) mod bank_filters) * n; the Bluestein instantiations read neither field
  uint32_t bank_filters;
  uint32_t bank_first;  // (the first row of the launch) mod bank_filters
  // lconv_small_kernel (LinearConvPlan, lconv_plan.h): overlap-save blocks of rows of lc_lx values in, lc_lout values out.  Block j of a
  // row holds input positions j * lc_step - (N - lc_step) + i, i < N, and stores its elements i >= N - lc_step to output position
  // j * lc_step + i - (N - lc_step) - lc_off.  Workgroup w of the launch: row w / lc_wpr, block (complex data) or pair of blocks
  // (real data) w % lc_wpr.
  uint32_t lc_lx, lc_lout, lc_step, lc_off;
  uint32_t lc_nb;           // blocks per row
  uint32_t lc_wpr;          // workgroups per row: lc_nb, real data (lc_nb + 1) / 2
  uint32_t lc_m, lc_l;      // w / lc_wpr = (umulhi(w, lc_m) + w) >> lc_l
  // czt_small_kernel (CztPlan, czt_plan.h): rows of cz_n values in (complex, or reals), rows of cz_m complex values out; the input is
  // multiplied by cz_a (cz_n entries), the result by cz_b (cz_m entries); `mul` is the one table H of n entries
  const void* cz_a;
  const void* cz_b;
  uint32_t cz_n, cz_m;
  // xcorr_small_kernel (XcorrPlan, xcorr_plan.h): rows of xc_n reals at `in` (x) and at xc_in2 (y), rows of xc_lags reals out: lag
  // t of the n-point circular correlation goes to output position (t - xc_first) mod n where that is below xc_lags
  const void* xc_in2;
  uint32_t xc_n, xc_first, xc_lags;  // xc_first = lag_first mod n
  // delay_small_kernel (DelayPlan, delay_plan.h): rows of dl_n reals in and out; row b of the launch is delayed by dl_delays[b]
  // samples and scaled by dl_weights[b] (null: 1), both reals T on the device
  const void* dl_delays;
  const void* dl_weights;
  uint32_t dl_n;
  // cepstrum_small_kernel (CepstrumPlan, cepstrum_plan.h): rows of cp_n reals in, rows of cp_m reals out;
  // g = 0.5 cp_log_mult ln(max(|X|^2, cp_floor2)), cp_floor2 = log_floor^2 computed in T.  Where that square is no normal number
  // of T, cp_floor_given is 1, cp_floor2 is the square clamped to [min normal, +inf] and a bin below it takes the finished value
  // cp_g_floor = cp_log_mult ln(log_floor) / N, computed in double on the host
  uint32_t cp_n, cp_m;
  uint32_t cp_floor_given;
  double cp_log_mult, cp_floor2, cp_g_floor;
};


// ---- lane-per-transform kernels (kernels_small.h)
struct TinyArgs {
  const void* in; void* out;
  uint64_t batch; int n; int swap_in, swap_out; double scale;
};


// ---- LDS mixed-radix kernels (kernels_mixed.h)
struct MixArgs {
  const void* in; void* out; const void* tw;  // tw: forward table, Sum(size_cur) entries
  uint64_t batch;
  uint32_t n, group;      // transform length, transforms per workgroup
  uint32_t npass;         // passes, and the radix of each (mix_next_radix)
  uint8_t radix[20];
  int forward, scaled;
  double scale, w3re, w3im, w8re, w8im;  // compute_twiddle(1,3,true), compute_twiddle(1,8,true) as T values
};


// ---- odd-radix passes, global-memory passes, unfused Bluestein sweeps (kernels_misc.h)
struct OddArgs {
  const void* in; void* out;
  uint64_t n, s, batch;       // transform length, Stockham stride of this pass, transforms
  uint64_t m;                 // size_cur / R: 1 for the last pass (stride = n / R), > 1 for a twiddled middle pass
  const void* tw;             // middle passes: W_size_cur^{e}, e < size_cur (size_cur = R * m)
  int swap_out;
  double scale;
  double wr[27], wi[27];      // W_R^e = exp(-2*pi*i*e/R), e < R (f64 on the host, cast on use)
};


struct GenArgs {
  const void* in; void* out;
  const void* tw_lo;          // W_size^{e}, e < 2^lo_bits          } two-level table of the pass twiddle W_size^{i*k}, as in the
  const void* tw_hi;          // W_size^{h << lo_bits}               } tile passes (null when m == 1: the last pass has no twiddle,
  uint32_t lo_bits;           //                                       mod.rs:238)
  uint64_t n;                 // transform length (batch stride)
  uint32_t s, m;              // stride, butterflies per stride group; s * m = n / R
  uint32_t blocks_per;        // workgroups per transform
  int swap_in, swap_out, final_pass;
  double scale;
  double wr[27], wi[27];      // W_R^e for the radix-3^b butterflies
};

struct BluArgs {
  const void* in; void* out; const void* xtab;
  uint64_t n, m, batch; int swap; double scale;
};

// ---- big-radix passes of mixed length on column tiles (kernels_tiled.h)
struct TiledArgs {
  const void* in; void* out;
  const void* tw;             // tables of the in-tile length-L transform, the reference's per-pass layout (mod.rs:24-46)
  const void* tw_lo;          // two-level table of the inter-pass twiddle W_size^{i*k} (null in the last pass)
  const void* tw_hi;
  uint32_t lo_bits;
  uint64_t n, s, m;           // transform length (batch stride); Stockham stride; size / L (1 in the last pass)
  uint64_t tiles_per_row;     // ceil(columns / COLS): columns = m in the first pass (s == 1), s afterwards
  int swap_in, swap_out;
  uint32_t xcd_chunk;         // workgroup -> tile order (xcd_chunked, kernels_common.h): 0 = identity
  double scale;               // applied by the last pass
  double w3re, w3im, w8re, w8im;  // compute_twiddle(1, 3, true), compute_twiddle(1, 8, true) as T values (butterfly.rs:12,50)
  // Bluestein on smooth M (kernels_regtile.h): chirp table x (blu_n entries), w = FFT_M(conj chirp) / M (n entries), user length,
  // user-level inverse (swap at the user array)
  const void* blu_x; const void* blu_w;
  uint64_t blu_n;
  int blu_swap;
};

// ---- whole chirp-z of a short transform in one launch on a smooth M = R1 x R2, both transforms in registers (kernels_chirpz.h)
struct ChirpzArgs {
  const void* in; void* out;
  const void* chirp;          // x[0 .. n): exp(-i pi k^2 / n) (bluesteins.rs:51-61)
  const void* w;              // FFT_M(conj chirp, mirrored) / M (bluesteins.rs:18-48), M entries
  const void* tw;             // [j2 < R2][k1 < R1]: W_M^{j2 * k1}
  uint64_t n, batch;          // user transform length (batch stride), transforms
  int swap;                   // user-level inverse: swap re / im of the user data
  double scale;
};

// ---- real-input transforms (kernels_real.h)
// real_post_kernel / real_pre_kernel: one lane per mirrored pair (j, h - j) of a row, j <= h / 2, over a flat index of
// rows x pairs; byte offsets are 32-bit (the plan launches at most REAL_LAUNCH_BYTES of either side per launch).  The odd-N sweeps
// (plain grid-stride loops between user rows and the complex N-point work array) read in, out, n and rows only.
// realnd_post_kernel / realnd_pre_kernel (the N-D sweeps of RealNdPlan, realnd_plan.h): one workgroup per row r of an item and
// segment of its `lanes` lanes; workgroup index = row * segs + segment, row = item * rows + r, r = (i_a * n_b + i_b) * n_c + i_c
// over the leading sizes nd[0 .. 2] (unused ones 1).  Row bases are 64-bit, offsets within a row 32-bit.
enum { REAL_POST = 0, REAL_PRE = 1, REAL_WIDEN = 2, REAL_NARROW = 3, REAL_EXTEND = 4, REAL_PART = 5, REAL_ND_POST = 6, REAL_ND_PRE = 7 };
struct RealArgs {
  const void* in; void* out;
  const void* tw;             // W_N^j, j <= h / 2 (f64 on the host, cast)
  uint32_t h;                 // N / 2: complex points of the inner transform
  uint32_t pairs;             // h / 2 + 1 lanes per row
  uint32_t total;             // rows * pairs
  uint32_t div_m, div_l;      // idx / pairs = (umulhi(idx, div_m) + idx) >> div_l
  uint32_t in_bytes, out_bytes;  // descriptor ranges of this launch
  double scale;               // forward: the code's scale; inverse: the code's scale / N (the inner IFFT runs unscaled)
  uint64_t n, rows;           // odd N: real length, rows in this launch
  uint32_t nd_rows, lanes;    // N-D: rows per item (product of the leading sizes), lanes per row (h / 2 rounded up)
  uint32_t segs;              // N-D: workgroups per row
  uint32_t nd[3];             // N-D: leading sizes n_a, n_b, n_c (unused ones 1)
  uint32_t seg_m, seg_l, row_m, row_l, c_m, c_l, b_m, b_l;  // N-D: multiply-high dividers by segs, nd_rows, nd[2], nd[1]
};

// ---- real-to-real transforms, DCT / DST of types II and III (kernels_r2r.h; R2RPlan, r2r_plan.h)
// Even N = 2h: r2r_pack_kernel / r2r_unpack_kernel run one lane per four consecutive reals of a row (`lanes` = (h + 1) / 2; the
// middle lane of an odd h has two), r2r_post_kernel / r2r_pre_kernel one lane per mirrored pair (j, h - j), j <= h / 2 (`lanes` =
// h / 2 + 1), all over a flat index of rows x lanes; byte offsets are 32-bit as the real sweeps' (rows of N reals and rows of h
// complex values have the same size, so one launch covers the same rows of both sides).  The odd-N sweeps (plain grid-stride loops
// between user rows and the complex N-point work array) read in, out, ct, n, rows, sine, scale and edge only.
enum { R2R_PACK = 0, R2R_POST = 1, R2R_PRE = 2, R2R_UNPACK = 3, R2R_ODD_WIDEN = 4, R2R_ODD_POST = 5, R2R_ODD_PRE = 6, R2R_ODD_PART = 7 };
struct R2RArgs {
  const void* in; void* out;
  const void* tw;             // W_N^j, j <= h / 2 (f64 on the host, cast)
  const void* ct;             // c_j = exp(-i pi j / 2N), j <= h (odd N: j < N)
  uint32_t h;                 // N / 2: complex points of the inner transform
  uint32_t lanes;             // lanes per row
  uint32_t total;             // rows * lanes
  uint32_t div_m, div_l;      // idx / lanes = (umulhi(idx, div_m) + idx) >> div_l
  uint32_t in_bytes, out_bytes;  // descriptor ranges of this launch
  int sine;                   // DST: the odd-indexed reals of the time side change sign, the index of the transform side is reversed
  double scale;               // the norm's factor (post: times 2 Re / -2 Im; pre: on V)
  double edge;                // factor on the transform side's element 0 (cosine index): 1, or the orthogonalised form's 1/sqrt 2, sqrt 2
  uint64_t n, rows;           // odd N: real length, rows in this launch
};

// ---- short-time Fourier transform (kernels_stft.h; StftPlan, stft_plan.h)
// A launch covers `total` items counted from a row base: `in` (forward) or `out` (inverse) points at the first sample of signal row 0
// of the launch.  Forward (stft_frame_kernel, stft_rows_kernel): item i is frame x = first + i of the flat frame index row * frames + f,
// row = x / frames by multiply-high (first < frames, x < 2^32); its sample n is xpad[f * hop - pad + n], the padding by index arithmetic
// (mode = FOURIER_STFT_PAD_*), times win[n]; the frame kernel writes rows of n_fft reals at out + i * n_fft, the fused kernel the h + 1
// bins at out + i * (h + 1).  Inverse (istft_ola_kernel): one lane per output sample of `rows` rows, sample t = t0 + i of `span` samples
// per row; frames f_lo ... f_lo + nfr - 1 of every row lie in `in` as rows of n_fft reals (row r at (r * nfr + f - f_lo) * n_fft), and
//   y[t] = scale * env[t] * sum_f win[t + pad - f hop] * frame_f[t + pad - f hop]   over the frames that cover t.
enum { STFT_FRAME = 0, STFT_OLA = 1 };
enum { STFT_PAD_NONE = 0, STFT_PAD_REFLECT = 1, STFT_PAD_ZERO = 2 };  // FOURIER_STFT_PAD_* (include/fourier.h)
struct StftArgs {
  const void* in; void* out;
  const void* win;            // the window, zero-extended to n_fft reals
  const void* env;            // inverse: 1 / sum_f win^2, `length` reals
  const void* tw;             // fused: W_N^j, j <= N / 4 (real_untangle_twiddles)
  const void* tw1; const void* tw2;  // fused: the row core's stage tables
  uint64_t length;            // reals per signal row
  uint64_t total;             // forward: frames of this launch; inverse: rows * span
  uint32_t frames;            // frames per signal row
  uint32_t first;             // forward: frame index (within row 0 of the launch) of item 0
  uint32_t fr_m, fr_l;        // x / frames = (umulhi(x, fr_m) + x) >> fr_l
  uint32_t n_fft, hop, pad, mode;
  int pairs;                  // fused: every interior frame starts on an even element of a 2 * sizeof(T)-aligned row
  uint64_t t0, span, rows;    // inverse: first sample of the range, samples per row in it, rows
  uint64_t f_lo, nfr;         // inverse: first frame in the scratch, frames per row there
  double scale;
};

// ---- power spectrogram and Welch average (kernels_spectrogram.h; SpectrogramPlan, spectrogram_plan.h)
// `f` is the STFT's argument block: the frame geometry, the window, the tables, and f.in / f.out of the launch.  The fused kernel reads
// it as stft_rows_kernel does and writes reals: OUT = SPEC_POWER / SPEC_MAGNITUDE the h + 1 values of item i at f.out + i * (h + 1);
// OUT = SPEC_PARTIAL one row of h + 1 partial sums per workgroup at part + blk * (h + 1), workgroup blk = row * tiles + tile over the
// frames tile * COLS ... of that row (f.in at the first sample of row 0 of the launch).  The sweeps: spectrogram_power_kernel |z|^power
// over `count` complex values f.in -> reals f.out; welch_colsum_kernel one lane per (slot, bin) of `count` / bins slots from slot0 on,
// slot v = row * tiles + t the frames t * tile_frames ... of a row, over the flat frames g0 ... g1 - 1 whose transforms lie at f.in
// (frame g at (g - g0) * bins); welch_reduce_kernel `count` = rows * bins lanes, f.out[b, k] = scale * c_k * sum_t part[b][t][k].
enum { SPEC_MAGNITUDE = 1, SPEC_POWER = 2, SPEC_PARTIAL = 3 };  // 1, 2: FOURIER_SPECTROGRAM_MAGNITUDE / _POWER (include/fourier.h)
enum { SPECTROGRAM_POWER_SWEEP = 0, WELCH_COLSUM = 1, WELCH_REDUCE = 2 };
struct SpectrogramArgs {
  StftArgs f;
  void* part;                 // Welch: the partial sums, rows x tiles x bins reals
  uint32_t tiles;             // Welch: slots per row
  uint32_t tl_m, tl_l;        // fused: blk / tiles = (umulhi(blk, tl_m) + blk) >> tl_l
  uint32_t bins;
  uint32_t tile_frames;       // composed Welch: frames per slot
  uint32_t power;             // spectrogram_power_kernel: SPEC_MAGNITUDE / SPEC_POWER
  int fold;                   // reduce: c_k = 2 for the bins with a mirror, 0 < 2k < n_fft
  uint64_t slot0, g0, g1;     // composed Welch: first slot of the launch, the chunk's flat frame range (from row 0 of the group)
  uint64_t count;             // sweeps: lanes
  double scale;               // reduce: the caller's scale over frames
};

// ---- cross-spectral density and coherence (kernels_csd.h; CsdPlan, csd_plan.h)
// `f` is the STFT's argument block with f.in at the first sample of x's row 0 of the launch; `in2` is the same row of y.  The partial
// sums are four planes of `bins` reals per (row, slot): |X|^2, |Y|^2, Re and Im of conj(X) Y, slot v = row * tiles + t at
// part + v * 4 * bins.  csd_rows_kernel: workgroup blk = row * tiles + tile over the frame pairs tile * COLS / 2 ... of that row.
// csd_colsum_kernel: one lane per (slot, bin) of `count` / bins slots from slot0 on, slot v the frames t * tile_frames ... of a row, over
// the flat frames g0 ... g1 - 1 whose transforms lie at f.in: X of frame g at (g - g0) * bins, Y of it `ystride` complex values behind.
// csd_reduce_kernel: `count` = rows * bins lanes, the slots of a row summed in ascending order; coherence == 0 writes the complex
// f.out[b, k] = scale * c_k * (Re, Im), else the real |(Re, Im)|^2 / (sum |X|^2 * sum |Y|^2).
enum { CSD_COLSUM = 0, CSD_REDUCE = 1 };
enum { CSD_PXX = 0, CSD_PYY = 1, CSD_RE = 2, CSD_IM = 3, CSD_PLANES = 4 };
struct CsdArgs {
  StftArgs f;
  const void* in2;            // y: the rows of the second signal, laid out as f.in
  void* part;                 // the partial sums, rows x tiles x 4 x bins reals
  uint32_t tiles;             // slots per row
  uint32_t tl_m, tl_l;        // fused: blk / tiles = (umulhi(blk, tl_m) + blk) >> tl_l
  uint32_t bins;
  uint32_t tile_frames;       // composed: frames per slot
  int fold;                   // reduce: c_k = 2 for the bins with a mirror, 0 < 2k < n_fft
  int coherence;              // reduce: the coherence instead of the cross spectrum
  uint64_t slot0, g0, g1;     // composed: first slot of the launch, the chunk's flat frame range (from row 0 of the group)
  uint64_t ystride;           // composed: complex values between X and Y of a frame in the scratch
  uint64_t count;             // sweeps: lanes
  double scale;               // reduce: the caller's scale over frames
};

// ---- band-energy (mel) spectrogram (kernels_bandspec.h; BandSpecPlan, bandspec_plan.h)
// `f` is the STFT's argument block.  The bank is a sparse-row matrix of `bands` x `bins` reals: row j has its support at the columns
// lo[j] ... lo[j] + (off[j + 1] - off[j]) - 1 and its weights, zeros inside the support included, at w + off[j].  Item i of a launch
// writes `bands` reals at f.out + i * bands: y_j = sum_k w_j[k] |X[k]|^power in ascending k in one accumulator, then, log_mult != 0,
// log_mult * ln(max(y_j, log_floor)).  bandspec_rows_kernel reads f as stft_rows_kernel does; bandspec_sweep_kernel has one lane per
// (frame, band) of `count` = frames * bands over the transformed frames at f.in (frame i at i * bins complex values).
struct BandSpecArgs {
  StftArgs f;
  const void* lo;             // uint32_t[bands]: first column of a row's support
  const void* off;            // uint32_t[bands + 1]: start of a row's weights in w
  const void* w;              // the packed weights, reals T
  uint32_t bins, bands;
  uint32_t power;             // sweep: SPEC_MAGNITUDE / SPEC_POWER
  uint64_t count;             // sweep: lanes
  double log_mult, log_floor;
};

// ---- modified discrete cosine transform (kernels_mdct.h; MdctPlan, mdct_plan.h)
// A frame is 2n samples, the hop n; frame f of a row covers xpad[f n - pad ... f n - pad + 2n), zero outside the row.  The flat frame
// index, `first`, `total` and the multiply-high division are StftArgs'.  Even n = 2h: a frame is h complex values in the scratch
// (z before the inner plan, Z behind it); odd n: 2n complex values.  Forward sweeps and the fused kernel write frame i of the launch at
// out + i * n reals.  Inverse: the pre sweeps read frame i at in + i * n reals; imdct_ola_kernel has one lane per output sample of
// `rows` rows, sample t = t0 + i of `span` samples per row, over frames f_lo ... f_lo + nfr - 1 of every row in the scratch.
enum { MDCT_FOLD = 0, MDCT_POST = 1, MDCT_ODD_PRE = 2, MDCT_ODD_POST = 3, IMDCT_PRE = 4, IMDCT_ODD_PRE = 5, IMDCT_OLA = 6, IMDCT_ODD_OLA = 7 };
struct MdctArgs {
  const void* in; void* out;
  const void* win;            // the window, 2n reals
  const void* twa;            // even n: exp(-i pi (4j + 1) / 4n), j < h; odd n: exp(-i pi m / 2n), m < 2n
  const void* twb;            // even n: exp(-i pi j / n), j < h; odd n: exp(-i pi (n + 1)(2k + 1) / 4n), k < n
  const void* tw1; const void* tw2;  // fused: the row core's stage tables
  uint64_t length;            // reals per signal row
  uint64_t total;             // forward, inverse pre sweeps: frames of this launch; overlap-add: rows * span
  uint32_t frames;            // frames per signal row
  uint32_t first;             // forward: frame index (within row 0 of the launch) of item 0
  uint32_t fr_m, fr_l;        // x / frames = (umulhi(x, fr_m) + x) >> fr_l
  uint32_t n, pad;
  int pairs;                  // fused: every output frame starts on a 2 * sizeof(T)-aligned address
  uint64_t t0, span, rows;    // overlap-add: first sample of the range, samples per row in it, rows
  uint64_t f_lo, nfr;         // overlap-add: first frame in the scratch, frames per row there
  double scale;
};

// ---- convolution with a filter bank (kernels_conv.h; ConvPlan, conv_plan.h)
// conv_mul_kernel: Z[b][k] *= H[(first + b) mod filters][k] over a flat index of rows x len, one lane per element.
// real_conv_mid_kernel: one lane per mirrored pair (j, h - j) of a row of the inner plan's output, as the real sweeps (`len` = h / 2 + 1
// lanes per row); untangle, multiply by the half spectrum H (rows of h + 1), retangle, in place.  Byte offsets into the data are
// 32-bit (at most REAL_LAUNCH_BYTES per launch), the bank is addressed with 64-bit indices.
// conv_finish_kernel: bank[i] = scale * bank[i] (conjugated where conj != 0), i < count.  conv_pad_kernel: `rows` rows of `taps`
// words T -> rows of `n` words, zero-extended (a complex value is two words).
// The linear-convolution handle (LinearConvPlan, lconv_plan.h) adds two more.  lconv_copy_kernel, the pad and the crop sweep of its
// padded route: output row r, word k < n, is input word skip + k of input row r (rows of `taps` words) where that lies inside the
// row, else zero; one workgroup per LCONV_SEG words of an output row, `len` segments per row, over a flat index of rows x len.
// lconv_taps_kernel (set_filters): `rows` filters of `taps` values of the handle's kind -> rows of `n` values, zero-extended, in
// reverse order and conjugated where conj != 0 (a correlation), real values widened to complex ones where widen != 0.
enum { CONV_MUL = 0, CONV_REAL_MID = 1, CONV_FINISH = 2, CONV_PAD = 3, CONV_LCOPY = 4, CONV_LTAPS = 5 };
constexpr uint32_t LCONV_SEG = 2048;
struct ConvArgs {
  const void* in; void* out;  // the sweeps run in place: in == out
  const void* tw;             // real mid sweep: W_N^j, j <= h / 2
  const void* bank;           // H: `filters` rows of `len` (mul) or h + 1 (real mid) complex values
  uint32_t h;                 // real mid sweep: N / 2
  uint32_t len;               // lanes per row: complex values per row (mul), h / 2 + 1 pairs (real mid)
  uint32_t total;             // rows * len
  uint32_t div_m, div_l;      // idx / len = (umulhi(idx, div_m) + idx) >> div_l
  uint32_t filters, first;    // row b of this launch uses filter (first + b) mod filters, first < filters
  uint32_t f_m, f_l;          // the same divider for `filters`
  uint32_t bytes;             // descriptor range of this launch
  uint64_t n, taps, rows;     // pad: words per output row, words per input row, rows
  uint64_t count;             // finish: complex values
  int conj;
  double scale;
  uint64_t skip;              // lconv copy: words of an input row in front of the first one copied
  int widen, real;            // lconv taps: real taps -> complex rows; the values are reals (else complex)
};

// ---- N-D convolution with a filter bank (kernels_convnd.h; ConvNdPlan, convnd_plan.h)
// realnd_conv_mid_kernel: the middle of the packed route, in place on Z (items of rows x h): the workgroups and rows of the N-D real
// sweeps (`r`: in == out == Z, tw, h, lanes, segs, nd and the dividers as realnd_post_kernel reads them; scale unused), the bank H of
// `filters` half spectra of rows x (h + 1), item b of this launch with filter (first + b) mod filters.  Row bases are 64-bit, offsets
// within a row 32-bit.
// convnd_pad_kernel / convnd_crop_kernel: window copies between items of lines of words T.  Destination line (i_a, i_b, i_c) of an
// item of dl[0] x dl[1] x dl[2] lines of dw words (unused leading sizes 1), word k, is word offw + k of line (i_a + off[0], i_b +
// off[1], i_c + off[2]) of the source item of sl[0] x sl[1] x sl[2] lines of sw words; the pad sweep stores zero where that lies
// outside the source item, the crop sweep's windows lie inside it.  One workgroup per LCONV_SEG words of a destination line over a flat
// index of lines x segs; line addresses are 64-bit.
// convnd_mul_kernel (the composed route's product where an item is beyond conv_mul_kernel's 32-bit index): dst[b][r][k] *=
// bank[(first + b) mod filters][r][k] over items of dlines rows of dw complex values, one workgroup per row and segment of 256 columns.
enum { CONVND_MID = 0, CONVND_PAD = 1, CONVND_CROP = 2, CONVND_MUL = 3 };
struct ConvNdArgs {
  RealArgs r;                 // mid
  const void* bank;
  uint32_t filters, first;    // first < filters
  uint32_t f_m, f_l;          // the divider for `filters`
  const void* src; void* dst; // window copies
  uint32_t dl[3], sl[3], off[3];
  uint32_t dlines, slines;    // lines per destination and per source item
  uint32_t segs;              // workgroups per destination line
  uint32_t seg_m, seg_l, line_m, line_l, c_m, c_l, b_m, b_l;  // dividers by segs, dlines, dl[2], dl[1]
  uint64_t dw, sw, offw;
};

// ---- analytic signal and envelope (kernels_hilbert.h; HilbertPlan, hilbert_plan.h): the sweeps of the composed route, one lane per
// element over a flat index of rows x n; byte offsets are 32-bit (at most REAL_LAUNCH_BYTES of the complex side per launch).
// hilbert_expand_kernel: rows of h + 1 complex values X (a half spectrum) -> rows of n complex values X[k] m[k] * scale, m = 1 for
// k = 0 and 2k = n, 2 for the other k <= h, 0 above.  hilbert_abs_kernel: `total` complex values z -> `total` reals |z|.
enum { HILBERT_EXPAND = 0, HILBERT_ABS = 1 };
struct HilbertArgs {
  const void* in; void* out;
  uint32_t n, h;              // values per row, n / 2
  uint32_t total;             // rows * n
  uint32_t div_m, div_l;      // idx / n = (umulhi(idx, div_m) + idx) >> div_l
  uint32_t in_bytes, out_bytes;  // descriptor ranges of this launch
  double scale;               // the inverse's 1 / n, computed in T
};

// ---- chirp-z transform (kernels_czt.h; CztPlan, czt_plan.h): the end sweeps of the composed route, one lane per element of the
// output side over a flat index; byte offsets are 32-bit (at most REAL_LAUNCH_BYTES of the work array per launch).
// czt_in_kernel: rows of n values x (complex, or reals where `real`) -> rows of L = 2^l_shift complex values x[j] A[j], zeros from n on.
// czt_out_kernel: rows of L complex values y -> rows of m complex values y[k] B[k].
enum { CZT_IN = 0, CZT_OUT = 1 };
struct CztArgs {
  const void* in; void* out;
  const void* tab;            // A (n entries) or B (m entries)
  uint32_t n, m;              // values per user row: in, out
  uint32_t l_shift;           // log2 of the work row
  uint32_t total;             // rows * L (in) or rows * m (out)
  uint32_t div_m, div_l;      // out: idx / m = (umulhi(idx, div_m) + idx) >> div_l
  uint32_t in_bytes, out_bytes;  // descriptor ranges of this launch
  int real;                   // in: the user rows are reals
};

// ---- polyphase filter bank (kernels_pfb.h; PfbPlan, pfb_plan.h)
// A frame is channels * taps values of a row (complex values, or reals where `real`), frame f of a row starts at value f * hop; there is
// no padding, every frame lies inside its row.  The flat frame index, `first`, `total` and the multiply-high division are StftArgs'.
// pfb_fold_kernel writes the `channels` folded values u[n] = sum_t filt[t * channels + n] x[f hop + t channels + n] of frame i of the
// launch at out + i * channels (values of the input's kind); the fused kernels write frame i's bins at out + i * bins complex values.
struct PfbArgs {
  const void* in; void* out;
  const void* filt;           // the prototype filter, channels * taps reals
  const void* tw;             // fused, real rows: W_P^j, j <= P / 4 (real_untangle_twiddles)
  const void* tw1; const void* tw2;  // fused: the row core's stage tables
  uint64_t length;            // values per signal row
  uint64_t total;             // frames of this launch
  uint32_t frames;            // frames per signal row
  uint32_t first;             // frame index (within row 0 of the launch) of item 0
  uint32_t fr_m, fr_l;        // x / frames = (umulhi(x, fr_m) + x) >> fr_l
  uint32_t channels, taps, hop;
  int real;                   // fold sweep: the rows are reals
  int pairs;                  // fused, real rows: every frame starts on an even element of a 2 * sizeof(T)-aligned row
};

// ---- polyphase synthesis filter bank (kernels_pfb.h; IpfbPlan, ipfb_plan.h)
// ipfb_gather_kernel: the weighted overlap-add as a gather.  Frames q < nfr of each of the launch's rows lie in `in` as rows of `channels`
// values of the output's kind (complex values, or reals where `real`), frame q of row r at (r * nfr + q) * channels.  The launch writes
// samples t0 ... t0 + span - 1 of every row (row r at out + r * length), one lane per sample, or per pair of samples where `pairs`:
// `items` lanes a row, lane index = r * items + j by multiply-high.  Everything inside a row is 32-bit and relative to frame fb, the first
// frame of the row that does not end before t0: sample t0 + i lies u = e0 + i values behind the start of frame fb (e0 = t0 - fb * hop,
// negative inside a gap between frames), frame fb + k covers it where 0 <= u - k * hop < span_pt, and
//   y[t0 + i] = scale * sum over those k < kcount, ascending, of filt[u - k hop] * frame_{q0 + k}[(u - k hop) mod channels],
// 0 where there is none.  The plan keeps span <= 2^30, so u < 2^32.
struct IpfbArgs {
  const void* in; void* out;
  const void* filt;           // the synthesis filter, channels * taps reals
  uint64_t length;            // values per output row
  uint64_t t0;                // first sample of the launch within a row
  uint64_t nfr;               // frames per row in `in`
  long long e0;               // t0 - fb * hop (signed; spelled without a stdint name: the run-time compiler has no int64_t)
  uint32_t span;              // samples per row in this launch
  uint32_t items;             // lanes per row: span, with `pairs` (span + 1) / 2
  uint32_t total;             // rows * items
  uint32_t it_m, it_l;        // idx / items = (umulhi(idx, it_m) + idx) >> it_l
  uint32_t q0;                // the frame fb's index within `in`
  uint32_t kcount;            // frames of `in` from fb on: nfr - q0
  uint32_t channels, span_pt, hop;  // P, P * T, D
  uint32_t hop_mod;           // D mod P: what the index within a frame moves by per frame
  uint32_t hop_m, hop_l;      // the same divider for hop
  uint32_t ch_m, ch_l;        // ... and for channels
  int real;                   // the rows are reals
  int pairs;                  // real rows: every row of the launch starts on a 2 * sizeof(T)-aligned address, two reals per store
  double scale;               // 1 / channels (the inner inverse runs unscaled), applied to the finished sum
};

// ---- Fourier-domain resampling (kernels_resample.h; ResamplePlan, resample_plan.h): rows of n values -> rows of m values, K = min(n, m),
// kh = K / 2.  Byte offsets are 32-bit (at most REAL_LAUNCH_BYTES of either side per launch); `win` is NULL for no window.
// resample_remap_kernel: one lane per output bin over a flat index of rows x orow.  Complex rows (half = 0): spectra of n values ->
// spectra of m values, Y[f mod m] = X[f mod n] win[f mod n] * scale for 2 |f| < K and the rule of include/fourier.h for an even K's bin
// kh, zeros elsewhere.  Half spectra (half = 1): rows of n / 2 + 1 -> rows of m / 2 + 1, Y[k] = X[k] win[k] * scale for 2 k < K,
// Y[kh] = X[kh] win[kh] * scale * nyq for an even K, zeros above; win is the folded window of n / 2 + 1 reals.
// resample_untangle_kernel (n = 2 hn, m = 2 hm): the hn values Z of the forward inner transform of a row -> the hm values the inverse
// inner transform takes, one lane per pair (j, hm - j), j <= hm / 2: `pairs` lanes a row.
enum { RESAMPLE_REMAP = 0, RESAMPLE_UNTANGLE = 1 };
enum { RESAMPLE_SAME = 0, RESAMPLE_DOWN = 1, RESAMPLE_UP = 2 };  // m == n, m < n, n < m
struct ResampleArgs {
  const void* in; void* out;
  const void* win;            // remap, complex rows: n reals; remap, half spectra, and untangle: n / 2 + 1 reals (folded); or NULL
  const void* tw_in;          // untangle: W_n^j, j <= n / 4 (real_untangle_twiddles)
  const void* tw_out;         // untangle: W_m^j, j <= m / 4
  uint32_t n, m;              // values per row of the signal: in, out
  uint32_t irow, orow;        // remap: values per row of the two spectra; untangle: hn, hm
  uint32_t kh;                // K / 2
  uint32_t even;              // K is even: the bin kh takes the Nyquist rule
  uint32_t mode;              // RESAMPLE_SAME / DOWN / UP
  uint32_t half;              // remap: the rows are half spectra
  uint32_t pairs;             // untangle: hm / 2 + 1
  uint32_t total;             // remap: rows * orow; untangle: rows * pairs
  uint32_t div_m, div_l;      // idx / orow (remap) or idx / pairs (untangle) = (umulhi(idx, div_m) + idx) >> div_l
  uint32_t in_bytes, out_bytes;  // descriptor ranges of this launch
  double nyq;                 // half spectra and untangle: the factor of the bin kh -- 1, 2 (m < n) or 1/2 (n < m)
  double scale;               // 1 / n, computed in T: m / n times the inverse's 1 / m
};

// ---- pairwise cross-correlation (kernels_xcorr.h; XcorrPlan, xcorr_plan.h): the sweeps of the composed routes, one lane per element of
// the output side over a flat index; byte offsets are 32-bit (at most REAL_LAUNCH_BYTES of either side per launch).  The values are
// reals where `real`, else complex values.
// xcorr_pad_kernel: rows of n values -> rows of l values, zeros from n on.
// xcorr_mul_kernel: `total` spectrum values X (in) and Y (in2) -> conj(X) Y * scale, or (phat) conj(X / |X|) (Y / |Y|) * scale with
// |.| = sqrt(re^2 + im^2), 0 where either magnitude is 0; out may be in2.
// xcorr_window_kernel: rows of l values r -> rows of `lags` values r[(first + j) mod l].
enum { XCORR_PAD = 0, XCORR_MUL = 1, XCORR_WINDOW = 2 };
struct XcorrArgs {
  const void* in; const void* in2; void* out;
  uint32_t n, l;              // values per row: the signal, the transform
  uint32_t lags, first;       // window: values per output row, lag_first mod l
  uint32_t total;             // pad: rows * l; mul: values; window: rows * lags
  uint32_t div_m, div_l;      // idx / l (pad) or idx / lags (window) = (umulhi(idx, div_m) + idx) >> div_l
  uint32_t in_bytes, out_bytes;  // descriptor ranges of this launch
  int real, phat;
  double scale;               // mul: the inverse's 1 / l, computed in T
};

// ---- fractional delay and delay-and-sum (kernels_delay.h; DelayPlan, delay_plan.h): the composed routes' one sweep, one lane per
// output bin over a flat index; byte offsets are 32-bit (at most REAL_LAUNCH_BYTES of either side per launch).
// delay_mul_kernel: groups of `channels` consecutive spectra of `spec` bins (the half spectrum l / 2 + 1 of real rows, or all l bins) ->
// one row of `spec` bins a group, sum_c w[c] X[c][k] m(k, d[c]) * scale in ascending c; the delays and weights (null: 1) are reals T,
// one per input row, and never enter an address.
struct DelayArgs {
  const void* in; void* out;
  const void* delays; const void* weights;  // of the launch's first input row on
  uint32_t l, spec;           // the transform length; bins per row
  uint32_t channels;          // input rows per output row
  uint32_t total;             // output rows * spec
  uint32_t div_m, div_l;      // idx / spec = (umulhi(idx, div_m) + idx) >> div_l
  uint32_t len_m, len_l;      // the same for x / l, used where l <= 65536 (the exponent k * d_int fits 32 bits)
  uint32_t in_bytes, out_bytes;  // descriptor ranges of this launch
  double scale;               // the inverse's 1 / l, computed in T
};

// ---- cepstrum and minimum phase (kernels_cepstrum.h; CepstrumPlan, cepstrum_plan.h): the composed route's three sweeps, all in place,
// one lane per value over a flat index; byte offsets are 32-bit (at most REAL_LAUNCH_BYTES per launch).
// cepstrum_log_kernel: `total` half-spectrum values X -> {0.5 log_mult ln(max(|X|^2, floor2)) * scale, 0}; floor_given = 1: a value
// below floor2 takes the finished value g_floor (CepstrumFloor below).
// cepstrum_fold_kernel: rows of l reals c -> chat: weight 1 at 0 and (even l) at l / 2, 2 below l / 2, 0 above.
// cepstrum_exp_kernel: `total` half-spectrum values C -> exp(Re C) (cos Im C, sin Im C) * scale.
enum { CEPSTRUM_LOG = 0, CEPSTRUM_FOLD = 1, CEPSTRUM_EXP = 2 };
// The floor of one call as the logarithm kernels of both routes take it.  log_floor == 0, or log_floor^2 a normal number of T:
// floor2 is that square computed in T and given is 0 -- ln(floor2) is taken on the device.  Otherwise (the square underflows or
// overflows T) floor2 is the square clamped to [min normal, +inf], ln_floor = ln(log_floor) computed in double, given is 1; a launch
// hands its kernel log_mult ln_floor / L, the value of a bin below the floor, rounded to T once.
struct CepstrumFloor {
  double floor2, ln_floor;
  uint32_t given;
};
struct CepstrumArgs {
  void* data;
  uint32_t l;                 // fold: values per row
  uint32_t total;             // values of this launch
  uint32_t div_m, div_l;      // fold: idx / l = (umulhi(idx, div_m) + idx) >> div_l
  uint32_t bytes;             // descriptor range of this launch
  uint32_t floor_given;       // log: 1 where floor2 is the clamped square and g_floor the value of a bin below it
  double log_mult, floor2;    // log: log_floor^2, computed in T
  double g_floor;             // log: log_mult ln(log_floor) / l from the host, read where floor_given
  double scale;               // log, exp: the inverse's 1 / l, computed in T
};

// ---- non-uniform FFT, 1-D, types 1 and 2 (kernels_nufft.h; NufftPlan, nufft_plan.h): m points shared by the rows of a batch, sorted by
// their fine-grid coordinate; fine-grid rows of l cells, rows of m strengths, rows of n modes, all complex T.
// nufft_spread_kernel / nufft_interp_kernel: one lane per (row block, cell) / (row block, sorted point); `blocks` row blocks of RB rows
// from the launch's first row on, `per` workgroups a row block.  Every row has a buffer descriptor of its own (row bytes <= 2^31 - 1).
// nufft_deconv_kernel / nufft_amplify_kernel: one lane per output value over a flat index; byte offsets are 32-bit (at most
// REAL_LAUNCH_BYTES of either side per launch).  nufft_table_kernel: one lane per point, w weights each.
enum { NUFFT_DECONV = 0, NUFFT_AMPLIFY = 1 };
constexpr int NUFFT_RB = 4;                      // rows a lane of the two hot kernels serves ("Non-uniform FFT")
constexpr int NUFFT_MIN_W = 2, NUFFT_MAX_W_F32 = 8, NUFFT_MAX_W_F64 = 16;  // the kernel widths with an instance
struct NufftArgs {
  const void* in; void* out;  // spread: strengths -> grid; interp: grid -> strengths; deconv: grid -> modes; amplify: modes -> grid
  const int32_t* i0;          // [m] first cell of sorted point p (may lie outside [0, l): the footprint wraps)
  const void* d;              // [m] reals T: i0 - xg, in [-w/2, -w/2 + 1)
  const uint32_t* perm;       // [m] the caller's index of sorted point p
  const uint32_t* first;      // [l + 2w + 1]: first[e + w] = sorted points with i0 < e, e in [-w, l + w]
  const void* wtab;           // tabulated route: [w][m] reals T, weight of tap t of sorted point p at t * m + p; null: evaluated
  const void* inv_phihat;     // [n / 2 + 1] reals T: 1 / phihat(|k|)
  uint32_t l, m, n, w;
  uint32_t blocks, per;       // spread, interp: row blocks of this launch; workgroups a row block
  uint32_t per_m, per_l;      // blk / per = (umulhi(blk, per_m) + blk) >> per_l
  uint32_t total;             // deconv, amplify: values of this launch; table: m
  uint32_t div_m, div_l;      // deconv: idx / n; amplify: idx / l
  uint32_t in_bytes, out_bytes;  // deconv, amplify: descriptor ranges of this launch
  uint32_t order;             // 0: k ascending from -floor(n/2); 1: FFT order
  double beta;                // 2.30 w
};

// ---- non-uniform FFT, 2-D, types 1 and 2 (kernels_nufft2d.h; Nufft2dPlan, nufft2d_plan.h): m points shared by the items of a batch,
// bucketed by the wrapped first cell of axis 1 and sorted by the axis-2 grid coordinate within a bucket; fine-grid items of l1 x l2
// cells, rows of m strengths, items of n1 x n2 modes, all complex T, the last axis contiguous.
// nufft2d_spread_kernel / nufft2d_interp_kernel: one lane per (item block, cell) / (item block, sorted point); `blocks` item blocks of
// RB items from the launch's first item on, `per` workgroups an item block.  Every item has a buffer descriptor of its own (item bytes
// <= 2^31 - 1).  nufft2d_deconv_kernel / nufft2d_amplify_kernel: one lane per output value over a flat index; byte offsets are 32-bit
// (at most REAL_LAUNCH_BYTES of either side per launch).  nufft2d_table_kernel: one lane per point, 2 w weights each.
// The row block NUFFT_RB, the widths NUFFT_MIN_W .. NUFFT_MAX_W_* and NUFFT_DECONV / NUFFT_AMPLIFY are the 1-D handle's.
struct Nufft2dArgs {
  const void* in; void* out;  // spread: strengths -> grid; interp: grid -> strengths; deconv: grid -> modes; amplify: modes -> grid
  const uint32_t* r1;         // [m] first cell of axis 1 of sorted point p, modulo l1: its bucket
  const int32_t* i02;         // [m] first cell of axis 2 (may lie outside [0, l2): the footprint wraps)
  const void* d1;             // [m] reals T: i0_1 - g_1, in [-w/2, -w/2 + 1)
  const void* d2;             // [m] reals T: i0_2 - g_2
  const uint32_t* perm;       // [m] the caller's index of sorted point p
  const uint32_t* first;      // [l1][ne2]: first[r][e + w] = sorted index of the first point of bucket r with i0_2 >= e, e in [-w, l2 + w]
  const void* wtab;           // tabulated route: [2][w][m] reals T, weight of tap t of axis d of sorted point p at (d w + t) m + p; null: evaluated
  const void* inv1;           // [n1 / 2 + 1] reals T: 1 / phihat_1(|k1|)
  const void* inv2;           // [n2 / 2 + 1] reals T: 1 / phihat_2(|k2|)
  uint32_t l1, l2, m, n1, n2, w;
  uint32_t ne2;               // l2 + 2 w + 1: the row length of first[]
  uint32_t cells;             // l1 l2
  uint32_t blocks, per;       // spread, interp: item blocks of this launch; workgroups an item block
  uint32_t per_m, per_l;      // blk / per = (umulhi(blk, per_m) + blk) >> per_l
  uint32_t l2_m, l2_l;        // spread: cell / l2
  uint32_t total;             // deconv, amplify: values of this launch; table: m
  uint32_t item_m, item_l;    // deconv: idx / (n1 n2); amplify: idx / (l1 l2)
  uint32_t row_m, row_l;      // deconv: rem / n2; amplify: rem / l2
  uint32_t in_bytes, out_bytes;  // deconv, amplify: descriptor ranges of this launch
  uint32_t order;             // 0: both axes ascending from -floor(n/2); 1: both in FFT order
  double beta;                // 2.30 w
};

// ---- non-uniform FFT, 3-D, types 1 and 2 (kernels_nufft3d.h; Nufft3dPlan, nufft3d_plan.h): m points shared by the items of a batch,
// bucketed by the pair of wrapped first cells of axes 1 and 2 and sorted by the axis-3 grid coordinate within a bucket; fine-grid items
// of l1 x l2 x l3 cells, rows of m strengths, items of n1 x n2 x n3 modes, all complex T, the last axis contiguous.
// nufft3d_spread_kernel / nufft3d_interp_kernel: one lane per (item block, cell) / (item block, sorted point); `blocks` item blocks of
// RB items from the launch's first item on, `per` workgroups an item block.  Every item has a buffer descriptor of its own (item bytes
// <= 2^31 - 1).  nufft3d_deconv_kernel / nufft3d_amplify_kernel: one lane per output value over a flat index; byte offsets are 32-bit
// (at most REAL_LAUNCH_BYTES of either side per launch).  nufft3d_table_kernel: one lane per point, 3 w weights each.
// The item block NUFFT_RB, the widths NUFFT_MIN_W .. NUFFT_MAX_W_* and NUFFT_DECONV / NUFFT_AMPLIFY are the 1-D handle's.
struct Nufft3dArgs {
  const void* in; void* out;  // spread: strengths -> grid; interp: grid -> strengths; deconv: grid -> modes; amplify: modes -> grid
  const uint32_t* r1;         // [m] first cell of axis 1 of sorted point p, modulo l1
  const uint32_t* r2;         // [m] first cell of axis 2, modulo l2: the point's bucket is r1 l2 + r2
  const int32_t* i03;         // [m] first cell of axis 3 (may lie outside [0, l3): the footprint wraps)
  const void* d1;             // [m] reals T: i0_1 - g_1, in [-w/2, -w/2 + 1)
  const void* d2;             // [m] reals T: i0_2 - g_2
  const void* d3;             // [m] reals T: i0_3 - g_3
  const uint32_t* perm;       // [m] the caller's index of sorted point p
  const uint32_t* first;      // [l1 l2][ne3]: first[b][e + w] = sorted index of the first point of bucket b with i0_3 >= e, e in [-w, l3 + w]
  const void* wtab;           // tabulated route: [3][w][m] reals T, weight of tap t of axis d of sorted point p at (d w + t) m + p; null: evaluated
  const void* inv1;           // [n1 / 2 + 1] reals T: 1 / phihat_1(|k1|)
  const void* inv2;           // [n2 / 2 + 1] reals T: 1 / phihat_2(|k2|)
  const void* inv3;           // [n3 / 2 + 1] reals T: 1 / phihat_3(|k3|)
  uint32_t l1, l2, l3, m, n1, n2, n3, w;
  uint32_t ne3;               // l3 + 2 w + 1: the row length of first[]
  uint32_t cells;             // l1 l2 l3
  uint32_t blocks, per;       // spread, interp: item blocks of this launch; workgroups an item block
  uint32_t per_m, per_l;      // blk / per = (umulhi(blk, per_m) + blk) >> per_l
  uint32_t l3_m, l3_l;        // spread: cell / l3
  uint32_t l2_m, l2_l;        // spread: (cell / l3) / l2
  uint32_t total;             // deconv, amplify: values of this launch; table: m
  uint32_t item_m, item_l;    // deconv: idx / (n1 n2 n3); amplify: idx / (l1 l2 l3)
  uint32_t row_m, row_l;      // deconv: rem / n3; amplify: rem / l3
  uint32_t mid_m, mid_l;      // deconv: (rem / n3) / n2; amplify: (rem / l3) / l2
  uint32_t in_bytes, out_bytes;  // deconv, amplify: descriptor ranges of this launch
  uint32_t order;             // 0: all three axes ascending from -floor(n/2); 1: all in FFT order
  double beta;                // 2.30 w
};

// ---- transforms along a strided axis (kernels_axis.h): element (o, j, c) of an [outer][N][inner] array at (o*N + j)*inner + c
// axis_lane_kernel: one lane per column (o, c) of this launch's outer blocks and column range (`cols` columns from the launch's
// base); flat index idx < total = blocks * cols, o = idx / cols by multiply-high.  axis_transpose_kernel: `blocks` source matrices of rows x cols
// (leading dimension ld_in, block stride bs_in) -> their transposes (leading dimension ld_out, block stride bs_out), 32 x 32
// tiles; byte offsets are 32-bit (the plan launches at most AXIS_LAUNCH_BYTES of either side per launch).
struct AxisArgs {
  const void* in; void* out;
  uint64_t block;             // lane: N * inner, elements between outer blocks
  uint64_t inner;             // lane: elements between the rows j of a column
  uint32_t cols, total;       // lane: columns per block, blocks * cols lanes; transpose: source columns
  uint32_t div_m, div_l;      // lane: idx / cols = (umulhi(idx, div_m) + idx) >> div_l
  uint32_t rows, tiles_r, tiles_c, blocks;  // transpose: source rows; 32-row / 32-column tiles per block; blocks
  uint32_t ld_in, ld_out;     // transpose: leading dimensions (elements)
  uint64_t bs_in, bs_out;     // transpose: block strides (elements)
  uint32_t in_bytes, out_bytes;  // transpose: descriptor ranges of this launch
  int swap;                   // lane: inverse = swap . DFT . swap
  double scale;               // lane: applied on the store
};

// ---- XCD-fused one-launch plan (kernels_experiments.h)
struct FusedArgs {
  PassArgs a, b;       // pass A / pass B arguments; a.in, a.out, b.in, b.out are set per item
  const void* in;      // user input  (batch stride a.n)
  void* out;           // user output (may equal in: a transform is read completely before any of it is written)
  void* window;        // [16 XCC ids][depth][n] intermediates
  uint32_t* ctrl;      // control block, zeroed before every launch (layout below)
  uint32_t batch, depth, tiles_a, tiles_b, spin_limit;
};
// ctrl: [0] next global transform, [1] abort flag; queue of XCC id x at FUSED_CTRL_HDR + x * fused_ctrl_stride(batch):
//       [0] next item, [16 + j] map[j] (0 = unclaimed, 0xffffffff = batch exhausted, else transform + 1),
//       [16 + cap + j] done_a[j], [16 + 2*cap + j] done_b[j], cap = batch + 2
enum { FUSED_CTRL_HDR = 16, FUSED_XCC_IDS = 16 };
constexpr uint64_t fused_ctrl_stride(uint64_t batch) { return 16 + 3 * (batch + 2); }
constexpr uint64_t fused_ctrl_words(uint64_t batch) { return FUSED_CTRL_HDR + FUSED_XCC_IDS * fused_ctrl_stride(batch); }


}  // namespace fourier_hip
