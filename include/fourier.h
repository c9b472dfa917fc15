/* fourier.h -- C ABI of the MI355X-native FFT engine (libfourier.so).
 *
 * Part 1 is byte-compatible with the reference's C header, calebzulawski/fourier
 * `fourier-ffi/include/fourier.h:30-58` (implementation `fourier-ffi/src/lib.rs:14-106`): same
 * symbol names, argument meaning, transform codes and error behaviour, so existing C/C++ users and
 * the reference's own `Fft` trait (fourier-algorithms/src/fft.rs:40-82, through the Rust shim shown
 * in INTEGRATION.md) relink against this library unchanged.  The 8 legacy entry points take HOST
 * buffers of exactly `size` elements (no length argument, as in the reference) and are synchronous.
 *
 * Part 2 is the new surface the reversed boundary needs: batched execution
 * on device-resident interleaved buffers, stream-ordered, plus status queries.  The reference has
 * no batch API (fft.rs:48-61 is one slice per call); batching is what the GPU path is measured on.
 *
 * Handles are Send, not Sync -- like the reference's plans (RefCell scratch,
 * fourier-algorithms/src/autosort/mod.rs:54): one thread / one stream at a time per handle.
 */
#ifndef FOURIER_H_
#define FOURIER_H_

#ifdef __cplusplus
#include <complex>
#include <cstddef>
#include <memory>
#define FOURIER_COMPLEX_FLOAT_TYPE ::std::complex<float>
#define FOURIER_COMPLEX_DOUBLE_TYPE ::std::complex<double>
#define FOURIER_SIZE_TYPE ::std::size_t
#define FOURIER_STRUCT
namespace fourier {
namespace c {
extern "C" {
#else
#include <stddef.h>
#define FOURIER_COMPLEX_FLOAT_TYPE float _Complex
#define FOURIER_COMPLEX_DOUBLE_TYPE double _Complex
#define FOURIER_SIZE_TYPE size_t
#define FOURIER_STRUCT struct
#endif

/* ---------------- Part 1: legacy ABI (replaces fourier-ffi/include/fourier.h:30-58) ---------- */

/* Transform codes: fourier.h:30-36, fourier-ffi/src/lib.rs:3-12, fourier-algorithms/src/fft.rs:4-16 */
enum {
  FOURIER_TRANSFORM_FFT = 0,              /* forward, unscaled                */
  FOURIER_TRANSFORM_IFFT = 1,             /* inverse, scaled by 1/N           */
  FOURIER_TRANSFORM_UNSCALED_IFFT = 2,    /* inverse, unscaled                */
  FOURIER_TRANSFORM_SQRT_SCALED_FFT = 3,  /* forward, scaled by 1/sqrt(N)     */
  FOURIER_TRANSFORM_SQRT_SCALED_IFFT = 4, /* inverse, scaled by 1/sqrt(N)     */
};

struct fourier_fft_float;
struct fourier_fft_double;

/* replaces fourier.h:41-42 / lib.rs:15-20,62-67.  NULL on failure (the reference returns NULL when
 * plan creation panics, lib.rs:18-19).  size == 0 returns NULL (the reference hangs). */
struct fourier_fft_float *fourier_create_float(FOURIER_SIZE_TYPE);
struct fourier_fft_double *fourier_create_double(FOURIER_SIZE_TYPE);

/* replaces fourier.h:44-45 / lib.rs:22-29,69-76.  NULL is a no-op. */
void fourier_destroy_float(FOURIER_STRUCT fourier_fft_float *);
void fourier_destroy_double(FOURIER_STRUCT fourier_fft_double *);

/* replaces fourier.h:47-51 / lib.rs:31-43,78-90.  Host buffer of `size` elements, in place.
 * Unknown transform code: silent no-op, buffer untouched (lib.rs:10). */
void fourier_transform_in_place_float(const FOURIER_STRUCT fourier_fft_float *,
                                      FOURIER_COMPLEX_FLOAT_TYPE *, int);
void fourier_transform_in_place_double(
    const FOURIER_STRUCT fourier_fft_double *, FOURIER_COMPLEX_DOUBLE_TYPE *,
    int);

/* replaces fourier.h:53-58 / lib.rs:45-59,92-106.  Host buffers, out of place (in == out allowed). */
void fourier_transform_float(const FOURIER_STRUCT fourier_fft_float *,
                             const FOURIER_COMPLEX_FLOAT_TYPE *,
                             FOURIER_COMPLEX_FLOAT_TYPE *, int);
void fourier_transform_double(const FOURIER_STRUCT fourier_fft_double *,
                              const FOURIER_COMPLEX_DOUBLE_TYPE *,
                              FOURIER_COMPLEX_DOUBLE_TYPE *, int);

/* ---------------- Part 2: device-resident batched extension (new surface) -------------------- */

/* Status codes returned by the fourier_hip_* calls and by fourier_hip_last_status_*. */
enum {
  FOURIER_HIP_OK = 0,
  FOURIER_HIP_INVALID_ARGUMENT = 1, /* NULL handle/pointer, unknown transform code, bad option   */
  FOURIER_HIP_OUT_OF_MEMORY = 2,    /* device allocation failed                                  */
  FOURIER_HIP_RUNTIME_ERROR = 3,    /* a HIP call or kernel launch failed                        */
  FOURIER_HIP_UNSUPPORTED = 4,      /* size outside the engine's range                           */
};

/* Amplitude.  No entry point has an absolute constant in its arithmetic; the dynamic range of each follows from the number format T
 * (FLT_MAX = 2^128 (1 - 2^-24), DBL_MAX = 2^1024 (1 - 2^-53)) and is pinned by tests/amplitude_cases.py:
 *   linear entry points  (the transforms of every handle, convolution in the signal and in the filter, STFT / MDCT / filter banks /
 *                        resampling / chirp-z / analytic signal and their inverses): f(2^k x) = 2^k f(x) BIT FOR BIT while every input,
 *                        intermediate and output stays a normal number of T -- a power of two changes exponents only.  So do
 *                        fourier_hip_xcorr_* without weighting in x and in y (bilinear: both scaled, 2^2k; x by 2^k and y by 2^-k, no bit
 *                        changes), fourier_hip_delay_* in the rows and in the weights (never the delays), fourier_hip_convnd_* in the
 *                        items and in the taps, fourier_hip_nufft_* in the strengths (type 1) and the modes (type 2) (never the points).
 *   power and Welch      (fourier_hip_spectrogram_* at power 2 and welch, fourier_hip_csd_csd_*, the band sums of fourier_hip_bandspec_*):
 *                        scale by exactly 2^2k under the same condition; |X|^2 = re^2 + im^2 and every sum of it (over frames, over the
 *                        bins of a band) must be representable: |X| < sqrt(FLT_MAX) ~ 2^64 (f64: sqrt(DBL_MAX) ~ 2^512).
 *   magnitude, envelope  (spectrogram and band spectrogram at power 1, fourier_hip_hilbert_envelope_*) are sqrt(re^2 + im^2), NOT a hypot: the
 *                        result is representable for every finite X, but re^2 + im^2 must be: finite and exactly scaling for
 *                        |X| < sqrt(FLT_MAX) ~ 2^64 (f64 2^512), inf beyond although |X| itself is far from FLT_MAX; and re^2 and im^2 must
 *                        stay normal, |re|, |im| >= 2^-63 (f64 2^-511) where not 0, below which the result loses bits and then flushes to 0.
 *                        The tests pin finite and exactly scaled results with the largest magnitude in [2^61, 2^62) (f64 [2^509, 2^510)).
 *   coherence            is invariant under a power-of-two scaling of x or of y (degree 0) up to the overflow of the partial sums
 *                        themselves: sum_f |X[b, f, k]|^2 and sum_f |Y[b, f, k]|^2 must be finite (the cross sums are bounded by them:
 *                        Cauchy-Schwarz).  |X[b, f, k]| <= max |x| * sum_j |w_j|, so frames * (max |x| * sum |w|)^2 < FLT_MAX is
 *                        sufficient: with a Hann window of 2048 samples and 1000 frames, max |x| < 5.7e14 in f32 -- neither their
 *                        product nor the square of a cross sum is formed (see fourier_hip_csd_coherence_*).
 *   GCC-PHAT             (fourier_hip_xcorr_* under weighting 1) is degree 0 in x and in y: bit-identical under a power-of-two scaling
 *                        of either input for EVERY input whose values are normal numbers of T, on every route -- each spectrum value
 *                        is brought to a larger component in [1, 2) by a power of two before its magnitude is formed (the one-launch
 *                        route scales whole rows instead), so re^2 + im^2 cannot leave the format.  The tests pin it with x 2^k against
 *                        y 2^-k at k = +-100 (f64 +-900) and with the largest spectrum value in [2^61, 2^62) (f64 [2^509, 2^510)).
 *   cepstrum             (fourier_hip_cepstrum_*) has NO exact scaling, a logarithm lies between input and output: scaling x by 2^k
 *                        moves c[0] by k log_mult ln 2 and h by 2^(k log_mult) within the family's error bound, for
 *                        sqrt(min normal) < |X| < sqrt(max) (re^2 + im^2 is formed in T).  Its floor is honoured for every normal
 *                        log_floor, whatever log_floor^2 does in T.
 * Subnormal values may be flushed to zero by the device; nothing above holds where one appears. */

/* Create a plan on a specific device (-1 = current device).  Same plan factory as `create_fft_f32/f64`
 * (fourier/src/lib.rs:31-60): Stockham autosort for 2^a * 3^b as in the reference (`Autosort::new`, autosort/mod.rs:104-134),
 * Bluestein chirp-z (fourier-algorithms/src/bluesteins.rs) otherwise -- with one extension: SOME lengths that the reference
 * sends to Bluestein run as direct Stockham passes here (closer to the exact DFT than the chirp-z route, within the same
 * tolerance).  The routes, in the order they are tried (fourier_amd/csrc/plan.h, Plan::Plan), with the string
 * `fourier_hip_describe_*` returns for each (followed by " f32" / " f64"):
 *   powers of two                                   "stockham <L1>[x<L2>[x<L3>]]", "stockham <L1>x<L2> one-launch", "stockham tiny(<n>)":
 *                                                   big-radix Stockham passes, one, two or three HBM round trips
 *   2^a * 3^b, a >= 12, N = L1 x L2 with both tile  "stockham mixed tiles <L1>x<L2>": two column-tile passes of mixed length
 *     lengths <= 576 (12288 ... 331776)
 *   2^a * 3^b, a >= 12, every other length          "stockham <L1>x...x<27|9|3>": the power-of-two passes over 2^a, then radix-27 / 9 / 3 passes
 *   a length of 14 ... 20480 points with a factor   "stockham registers <R1>x<R2>[x<R3>] one-launch" (round 6): the whole transform in one launch on two or
 *     5 ... 13 that fourier_amd/csrc/regfft_shapes.h  three register-resident stages of at most 40 points -- 736 lengths in f32, 763 in f64 (to 20475 points:
 *     lists in the precision                          above 10240 f32 one transform per workgroup, f64 split planes), each one at least 1.04 x faster
 *                                                   than the route below it had (5005: f32 0.24 -> 0.49 of the HBM peak, f64 0.14 (Bluestein)
 *                                                   -> 0.50; 1001: 0.42 -> 0.60, 0.27 -> 0.69; f32 15625: 0.33 -> 0.42)
 *   2^a * 3^b * 5^c * 7^d * 11^e * 13^f that fit    "stockham mixed-radix <r1>.<r2>...." (+ " specialised" for a kernel compiled at run time):
 *     one compute unit's LDS (<= 20480 points in    every 2^a * 3^b; every such length with factors 5 (and the instantiated ones with a
 *     f32, 10240 in f64) AND have a kernel          factor 7) has a per-length kernel; any other length of this family up to 8192 points runs
 *                                                   the runtime-parameterised kernel (f64 with a factor 11 or 13: up to 2048 points)
 *   2^a * 3^b, a < 12, beyond the LDS limit, with   "stockham mixed tiles <L1>x<L2>[x<L3>]": two or three column-tile passes of mixed length
 *     N = L1 x L2 (x L3), every L in 64 ... 1024
 *   2^a * 3^b, a < 12, without such a factorisation "stockham global-pass <r1>.<r2>....": one Stockham pass per radix in global memory (since round 6,
 *                                                   tile lengths up to 1024, no accepted length is left without one: the fallback)
 *   2^a * 3^b * 5^c * 7^d with c + d >= 1 beyond    "stockham mixed tiles <L1>x<L2>[x<L3>]" (round 5; 10^5 = 400x250, 44100 = 210x210,
 *     the LDS kernels, N = L1 x L2 (x L3), every      10^6 = 1000x1000 in f32, 100x100x100 in f64; 390625 = 625x625, 500000 = 800x625): column-tile passes whose
 *     L in 64 ... 1024 (28 lengths above 512,         lengths have prime factors up to 7
 *     f32: 33)
 *   prime factors up to 13, no route above, and     "stockham mixed-radix ... specialised" / "stockham mixed tiles ... specialised": kernels
 *     its run-time kernels in the code-object cache   compiled by an earlier "specialise" (below) -- see fourier_hip_set_default_option
 *   every other length                              "bluestein M=<M> inner <power-of-two plan>[ fused]": chirp-z over a power-of-two transform
 *                                                   (bluesteins.rs:110), or -- round 6, where that work array is at least 1.6 x (f64: 1.44 x) longer and is
 *                                                   swept three times (M > 2^15, f64 2^14) -- "bluestein M=<L1*L2> inner mixed tiles
 *                                                   <L1>x<L2>": the same chirp-z over a product of two tile lengths >= 2N - 1
 *                                                   -- or, for a short length (2N - 1 <= 1024; f32 where that saves a tenth of the power of two),
 *                                                   "bluestein M=<R1*R2> registers <R1>x<R2> one-launch": the whole chirp-z in one launch
 *                                                   over M = R1 x R2 >= 2N - 1 with both M-point transforms in registers; up to 2N - 1 = 9261
 *                                                   "... registers <R1>x<R2>x<R3> one-launch" where such an M (1296 ... 3072, 8820, 9261) is
 *                                                   at least 1.25 x shorter than the power of two
 *                                                   (plan option "bluestein_smooth_m" = 0 brings the power of two back)
 * Rely on `fourier_hip_describe_*`, not on this list, where the accuracy class (direct versus chirp-z) matters.  NULL on failure. */
struct fourier_fft_float *fourier_hip_create_float(FOURIER_SIZE_TYPE size, int device);
struct fourier_fft_double *fourier_hip_create_double(FOURIER_SIZE_TYPE size, int device);

/* `Fft::size()` (fft.rs:45). 0 for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_size_float(const FOURIER_STRUCT fourier_fft_float *);
FOURIER_SIZE_TYPE fourier_hip_size_double(const FOURIER_STRUCT fourier_fft_double *);

/* Batched `Fft::transform` on DEVICE memory: `batch` contiguous transforms, transform b at element
 * offset b*size, interleaved complex.  d_in == d_out selects in-place (`transform_in_place`).
 * Enqueued on `stream` (a hipStream_t, NULL = default stream); the kernels are only enqueued, the call
 * does not wait for them.  Plans that need a plan-owned device buffer (in-place calls of the two-pass
 * plans, three-pass plans, the Bluestein work array) allocate it on the first call whose batch is larger
 * than any before -- hipMalloc / hipFree synchronise the device -- unless fourier_hip_reserve_* was
 * called for at least that batch first; after a reserve the call never allocates and can be captured
 * into a HIP graph.  Partial overlap of d_in and d_out is not allowed. */
int fourier_hip_transform_batch_float(const FOURIER_STRUCT fourier_fft_float *, const void *d_in,
                                      void *d_out, FOURIER_SIZE_TYPE batch, int transform,
                                      void *stream);
int fourier_hip_transform_batch_double(const FOURIER_STRUCT fourier_fft_double *, const void *d_in,
                                       void *d_out, FOURIER_SIZE_TYPE batch, int transform,
                                       void *stream);

/* Pre-size the plan-owned device buffers (scratch / Bluestein work array) for calls of up to `batch`
 * transforms, in place (in_place != 0) or out of place.  May synchronise the device; a later
 * fourier_hip_transform_batch_* with batch <= `batch` and the same placement does not allocate. */
int fourier_hip_reserve_float(const FOURIER_STRUCT fourier_fft_float *, FOURIER_SIZE_TYPE batch, int in_place);
int fourier_hip_reserve_double(const FOURIER_STRUCT fourier_fft_double *, FOURIER_SIZE_TYPE batch, int in_place);

/* Device index the plan lives on (its tables, scratch and kernels); -1 for a NULL handle.  Buffers
 * passed to fourier_hip_transform_batch_* must be resident on (or mapped into) that device. */
int fourier_hip_device_float(const FOURIER_STRUCT fourier_fft_float *);
int fourier_hip_device_double(const FOURIER_STRUCT fourier_fft_double *);

/* Blocks until everything queued on `stream` (a hipStream_t, NULL = the NULL stream) of the plan's device has
 * finished -- the wait that follows a stream-ordered fourier_hip_transform_batch_* for a caller that does not own a
 * HIP runtime of its own (the Rust shim, a ctypes binding). */
int fourier_hip_synchronize_float(const FOURIER_STRUCT fourier_fft_float *, void *stream);
int fourier_hip_synchronize_double(const FOURIER_STRUCT fourier_fft_double *, void *stream);

/* Batched `Fft::transform` on HOST memory -- what a caller of the reference holds (one slice per transform,
 * fourier-algorithms/src/fft.rs:48-61), `batch` of them contiguously.  The transforms are streamed through the
 * device in chunks (pinned staging; the host-to-device copy of one chunk, the kernels of the previous one and the
 * device-to-host copy of the one before overlap), so the rate is PCIe's, not one call's latency.  Synchronous:
 * `out` is complete on return.  in == out selects in-place; partial overlap is not allowed. */
int fourier_hip_transform_batch_host_float(const FOURIER_STRUCT fourier_fft_float *,
                                           const FOURIER_COMPLEX_FLOAT_TYPE *in, FOURIER_COMPLEX_FLOAT_TYPE *out,
                                           FOURIER_SIZE_TYPE batch, int transform);
int fourier_hip_transform_batch_host_double(const FOURIER_STRUCT fourier_fft_double *,
                                            const FOURIER_COMPLEX_DOUBLE_TYPE *in, FOURIER_COMPLEX_DOUBLE_TYPE *out,
                                            FOURIER_SIZE_TYPE batch, int transform);

/* Status of the LAST call that can fail made on this handle, and the text of a status.  The entry points that do
 * work -- the four legacy `void` transforms of Part 1, fourier_hip_transform_batch[_host]_*, _reserve_*,
 * _synchronize_*, _profile_* -- reset it to FOURIER_HIP_OK on entry and record their own failure, if any: a
 * successful call after a failed one reads FOURIER_HIP_OK again, and the legacy `void` entry points report through
 * this query only.  The pure queries (_size_*, _device_*, _describe_*, _model_bytes_*, _slot_names_*, _last_status_*
 * itself) and _set_option_* (which returns its own status) leave it untouched. */
int fourier_hip_last_status_float(const FOURIER_STRUCT fourier_fft_float *);
int fourier_hip_last_status_double(const FOURIER_STRUCT fourier_fft_double *);
const char *fourier_hip_status_string(int status);

/* Tunables (return FOURIER_HIP_OK or FOURIER_HIP_INVALID_ARGUMENT; "specialise" and "register_stages" also FOURIER_HIP_UNSUPPORTED).  A handle is Send, not
 * Sync, as in the reference (RefCell scratch, autosort/mod.rs:54): fourier_hip_set_option_* must not run concurrently with a
 * transform or another call on the SAME handle ("specialise" swaps the engine the plan executes with).
 *
 * THE RULE: what a plan runs is a function of the option values LAST SET on it, not of the order in which they were set or of values
 * set before them.  A plan on which every option was set to some value runs the same kernels on the same tables, describes itself
 * the same way and gives the same bits as a fresh plan on which those values were set once, in any order (tests/option_cases.py).
 * Where options meet, the precedence among the five "bluestein_*" options is:
 *   1. "bluestein_smooth_m" chooses M and with it the route (register stages in one launch, three sweeps on tiles, a power-of-two inner plan).
 *   2. "bluestein_fusion" = 0 takes a plan on a power-of-two inner plan, and a plan on the register route, to the separate sweeps
 *      (blu_pre, the inner passes, blu_post) on the reference's power-of-two M; describe() then says "separate", never "fused".  It is accepted and
 *      ignored on the three-sweep tile route, which has no unfused form.  1 brings back what "bluestein_smooth_m" chooses.
 *   3. "bluestein_conv" needs "bluestein_fusion": it is ignored on an unfused plan, on the one-launch routes and on the tile route.
 *      describe() ends in "no-conv" for a fused plan that has the conv kernel switched off.
 *   4. "bluestein_reference_chirp" = 1 overrides "bluestein_chirp_compute" while it is set; set back to 0, the value last set for
 *      "bluestein_chirp_compute" (or, never set, the plan's default) holds again.  "bluestein_chirp_compute" acts on a fused power-of-two
 *      inner plan of two or more passes only and is ignored elsewhere.
 * "scratch", "chunk_bytes", "stream_pipeline", "tile_walk" and "tile_walk_last" never change a bit of the result, in any combination;
 * after fourier_hip_reserve_* no call of at most that batch allocates under any of them, profiled calls included.
 *   "chunk_bytes"  bytes of one batch chunk pushed through all passes before the next chunk starts
 *                  (keeps the inter-pass intermediate inside the 256 MiB Infinity Cache); 0 = whole batch
 *   "scratch"      1 = always route the intermediate through the plan's reused scratch buffer,
 *                  0 = use the output buffer as intermediate when out of place (default)
 *   "xcd_swizzle"  1 (default) = XCD-aware workgroup->tile mapping (each XCD owns a contiguous run of transforms),
 *                  2 = XCDs interleaved over adjacent transforms, 3 = each XCD owns an eighth of every transform's
 *                  tiles, 4 = contiguous transforms per XCD walked band-major (the others measured slower or equal,
 *                  4 is "tile_walk" with bands of an eighth of a row), 0 = plain blockIdx order
 *   "bluestein_fusion" 1 (default where the inner FFT has >= 2 passes) = chirp steps fused into the inner passes
 *   "host_chunk_bytes" bytes of one chunk of fourier_hip_transform_batch_host_* (default 32 MiB, four in flight)
 *   "bluestein_conv"   1 (default with bluestein_fusion) = the forward inner FFT's last pass, the multiply by the
 *                  transformed chirp and the inverse inner FFT's first pass run as one launch
 *   "bluestein_smooth_m" 1 (default) = a Bluestein plan whose power-of-two work array would be swept three times takes M = L1 x L2, a
 *                  product of two tile lengths (64 ... 512, prime factors up to 7; the smallest that reaches 2N - 1, or one up to 4 % longer
 *                  whose lengths split more evenly into register stages), where that is at least 1.6 x shorter (f64: 1.44 x while the middle sweep's
 *                  tile stays within 336 points) (N = 16411: M = 32928 =
 *                  196 x 168 instead of 65536, f32 +39 %, f64 +53 %; N = 10007 f64: 20160 instead of 32768, +31 %); 0 = always the
 *                  reference's next power of two (bluesteins.rs:110); 2 = wherever such a product exists (measurements).  Rebuilds the plan's tables when the value changes (not while a
 *                  transform is in flight on the handle); INVALID_ARGUMENT on a plan that is not Bluestein.  Same tolerance class.
 *   "bluestein_chirp_compute" 1 = the fused chirp-in pass computes exp(-i*pi*k^2/N) (row table x column table x an
 *                  exact-exponent cross term) instead of reading the N-entry chirp table, a quarter of that pass's
 *                  memory traffic; default 1 where it was measured faster (first pass of length >= 1024 and a table
 *                  of >= 4 MiB, e.g. N = 999983), else 0.  Same tolerance class, not the same bits.
 *   "bluestein_reference_chirp" 1 = build the chirp tables from the reference's own expression, theta = k^2 * pi / N evaluated UNREDUCED in
 *                  f64 (bluesteins.rs:10,31,57), instead of from k^2 mod 2N reduced exactly: for a caller who wants the reference's f64
 *                  results rather than the exact DFT.  The reference's form costs it N * 1e-16 of angle -- 1.7e-10 of the result at
 *                  N = 999983 --; with the option the engine agrees with the reference's arithmetic to f64 rounding (1e-15), without it with
 *                  the exact DFT to 1e-15 (profiles/r05_s18_reference_chirp.jsonl).  Rebuilds two tables on the host, synchronises the device;
 *                  the chirp-in pass then reads its table ("bluestein_chirp_compute" off).  Default 0.  INVALID_ARGUMENT on a non-Bluestein plan.
 *   "specialise"   1 = compile this length's own LDS mixed-radix kernel with hipRTC, now (about a second, once per length,
 *                  device and process), and run it from the next call on.  For a length whose prime factors stop at 13, that
 *                  fits a compute unit's LDS and has no ahead-of-time per-length kernel -- by default it runs the
 *                  runtime-parameterised kernel (24-36 % of the HBM peak where per-length kernels reach 45-60 %) or, beyond
 *                  that kernel's reach, Bluestein.  OK and unchanged for a plan that already runs a per-length kernel;
 *                  FOURIER_HIP_UNSUPPORTED -- the plan keeps its route -- for any other length, where libhiprtc is not
 *                  installed, or where the compilation fails.  Beyond the LDS limit (up to 2^26 points) the option replaces a
 *                  Bluestein plan by two or three column-tile passes whose lengths (64 ... 1024 points) have prime factors up to 13
 *                  (143000 = 440 x 325, 5^8 = 625 x 625), compiled the same way, where such a factorisation exists.  Compiled code objects are kept in an
 *                  on-disk cache (below), so a length costs its second once per machine.  Compilation never happens implicitly unless
 *                  the library-wide default "specialise_at_create" is raised to 2 (fourier_hip_set_default_option).  Same tolerance
 *                  class as the default route, not the same bits.
 *   "tile_walk"    order in which an XCD walks the column tiles of its transforms: tiles per band | transforms per group << 8 | 1 << 19
 *                  for transform-fastest | 1 << 20 for strided bands (every (tiles / band)-th tile instead of adjacent ones; measured slower);
 *                  0 = tile-major (the default except f32 N = 2^20, which walks bands of eight tiles).  "tile_walk_last": the same encoding
 *                  for the LAST pass of a plain multi-pass plan alone (0 = as the other passes)
 *   "stream_pipeline" chunk | slots << 16 (| 1 << 24: both passes on ONE internal stream, a control): the two passes of a two-pass
 *                  power-of-two plan chunk by chunk over two internal streams, ordered by events only -- pass 0 of chunk k+1 beside pass 1 of
 *                  chunk k -- with the intermediate in a plan-owned ring of `slots` (>= 2) chunks of `chunk` transforms.  The same kernels on the same
 *                  data: the same bits.  Measured on MI355X: level with the two whole-batch launches for chunks of 128+ transforms, slower
 *                  below (launch and event latency); what it buys is MEMORY -- an in-place call then needs the ring (two chunks) instead of a
 *                  scratch of the whole batch.  The call stays stream-ordered on the caller's stream (forked into and joined from the internal
 *                  streams; capturable after fourier_hip_reserve_*).  0 = off (default).  INVALID_ARGUMENT on any other plan.
 *   "register_stages" 1 = a 2^a * 3^b length that runs the LDS kernel on the reference's own schedule (bit-identical to the reference's CPU
 *                  arithmetic as restated in oracle/) takes the register-stage kernel that fourier_amd/csrc/regfft_shapes.h lists for it ON REQUEST
 *                  instead ("stockham registers <R1>x<R2>[x<R3>] one-launch": the same values within rounding, not the same bits; 24 lengths in
 *                  f32, 34 in f64, each 1.04 ... 1.44 x faster -- 4608 f32 0.46 -> 0.56 of the HBM peak, 13122 f32 0.32 -> 0.41, 2592 f64 0.57 -> 0.72);
 *                  0 = back to the default.  FOURIER_HIP_UNSUPPORTED where no such kernel is listed (the plan is unchanged); OK and
 *                  unchanged on a plan that runs register stages by default.
 *   "l2_fused"     (lib/libfourier_experiments.so only; INVALID_ARGUMENT in the product library; so is
 *                  "last_pass_prefetch", the persistent prefetching last pass of DESIGN.md section 4) 1 = run both
 *                  passes of a two-pass plan in ONE launch with the intermediate parked in the XCD's L2 (persistent
 *                  workgroups, per-XCD work queues; f32 2^16..2^18, f64 2^15..2^17 only).  Same results bit for
 *                  bit; measured 30-45 % slower than the two-launch plan on MI355X.  Calls
 *                  under this option are synchronous: the kernel's bounded waits report a time-out through a flag
 *                  that is read back before the call returns (FOURIER_HIP_RUNTIME_ERROR).  "l2_fused_depth" (1..8
 *                  windows per XCD) and "l2_fused_grid" (persistent workgroups) tune it. */
int fourier_hip_set_option_float(FOURIER_STRUCT fourier_fft_float *, const char *key, long long value);
int fourier_hip_set_option_double(FOURIER_STRUCT fourier_fft_double *, const char *key, long long value);

/* Library-wide defaults for plans created AFTERWARDS (any thread; plans that exist keep what they have).  The keys:
 *   "specialise_at_create"  what `create` does for a length whose prime factors stop at 13 and that has no ahead-of-time route
 *                  (it would run the runtime-parameterised LDS kernel or Bluestein):
 *                    0  nothing: run-time kernels only through fourier_hip_set_option_*(h, "specialise", 1)
 *                    1  (default) load its specialised kernels where the on-disk code-object cache holds ALL of them (a few
 *                       milliseconds; nothing is ever compiled implicitly) -- a length specialised once is fast in every later process
 *                    2  ... and compile what the cache lacks (hipRTC, about a second per new length and machine, inside `create`)
 *                  so that a drop-in caller of fourier_create_float / create_fft_f32 reaches the specialised kernels with one call at
 *                  start-up, or with NO code change through the environment variable FOURIER_HIP_SPECIALISE=0|1|2 (read once, before the
 *                  first plan; the function overrides it).
 *   "register_stages_at_create"  0 (default) / 1: a 2^a * 3^b length with a register-stage kernel listed on request (plan option
 *                  "register_stages" above) takes it at create -- faster by 1.04 ... 1.44 x, the reference's values within rounding instead of
 *                  its bits; environment variable FOURIER_HIP_REGISTER_STAGES=1 (read once, before the first plan; the function overrides it).
 * Environment the library reads, all of it: FOURIER_HIP_VERBOSE (error text on stderr), FOURIER_HIP_SPECIALISE, FOURIER_HIP_REGISTER_STAGES (above) and the
 * location of the code-object cache: $FOURIER_HIP_CACHE_DIR, else $XDG_CACHE_HOME/fourier-hip, else $HOME/.cache/fourier-hip (an EMPTY
 * FOURIER_HIP_CACHE_DIR switches the disk cache off).  Cache files are keyed by device architecture, precision, kernel kind, length
 * and a hash of the embedded kernel sources, the compile options and the HIP runtime's version: a library or ROCm update never loads a stale
 * kernel.  A cache entry is executed on the device, so it is trusted only if its directory belongs to the calling user and nobody else may write it,
 * the entry itself is a regular file of that user that nobody else may write, opened without following a symbolic link, and it names the very
 * key (precision, kind, length, LDS bytes) and payload length it is read for; anything else of the user's under that name is discarded, anything of
 * another user's is ignored (files are created 0600, the directory 0700).  `fourier_warm_cache` (packaging/warm_cache.c, CMake target `warm_cache`)
 * and `python -m fourier_amd.warm_cache` fill the cache at install time: see INTEGRATION.md section 1.
 * Returns FOURIER_HIP_OK or FOURIER_HIP_INVALID_ARGUMENT (unknown key / value); _get_ returns the value or -1. */
int fourier_hip_set_default_option(const char *key, long long value);
long long fourier_hip_get_default_option(const char *key);

/* Human-readable plan description ("stockham 1024x1024 ..."), valid until the handle is destroyed. */
const char *fourier_hip_describe_float(const FOURIER_STRUCT fourier_fft_float *);
const char *fourier_hip_describe_double(const FOURIER_STRUCT fourier_fft_double *);

/* HBM bytes this plan reads+writes per transform across all its kernels (design traffic model). */
double fourier_hip_model_bytes_float(const FOURIER_STRUCT fourier_fft_float *);
double fourier_hip_model_bytes_double(const FOURIER_STRUCT fourier_fft_double *);

/* Measurement hook: runs ONE batched transform exactly like fourier_hip_transform_batch_*, with a
 * HIP event pair around every kernel launch on `stream`, waits for it, and returns per kernel slot
 * (launch order; names from fourier_hip_slot_names_*) the summed duration in ms and launch count. */
int fourier_hip_profile_float(const FOURIER_STRUCT fourier_fft_float *, const void *d_in, void *d_out,
                              FOURIER_SIZE_TYPE batch, int transform, void *stream, int nslots,
                              float *ms_sum, int *launches);
int fourier_hip_profile_double(const FOURIER_STRUCT fourier_fft_double *, const void *d_in, void *d_out,
                               FOURIER_SIZE_TYPE batch, int transform, void *stream, int nslots,
                               float *ms_sum, int *launches);
/* Comma-separated kernel slot names ("pass0,pass1" / "blu_pre,fwd_pass0,...,blu_post"). */
const char *fourier_hip_slot_names_float(const FOURIER_STRUCT fourier_fft_float *);
const char *fourier_hip_slot_names_double(const FOURIER_STRUCT fourier_fft_double *);

/* ---------------- real-input transforms (extension; the reference has none) ------------------------
 * Batched real-to-half-spectrum and half-spectrum-to-real transforms of length N >= 1 on DEVICE memory, numpy's rfft / irfft
 * layout:
 *   forward  d_in:  `batch` rows of N reals T, row b at element offset b*N;
 *            d_out: `batch` rows of N/2+1 interleaved complex T (row stride N/2+1, integer division).
 *            FOURIER_TRANSFORM_FFT: rfft(x); FOURIER_TRANSFORM_SQRT_SCALED_FFT: rfft(x) / sqrt(N).
 *   inverse  d_in:  N/2+1 complex values per row; d_out: N reals per row.
 *            FOURIER_TRANSFORM_IFFT: irfft(X, n=N); FOURIER_TRANSFORM_UNSCALED_IFFT: N * irfft; FOURIER_TRANSFORM_SQRT_SCALED_IFFT:
 *            sqrt(N) * irfft.  The imaginary parts of X[0] and, for even N, X[N/2] are ignored.  d_in is NOT modified (unlike
 *            cuFFT's c2r).
 * A code of the other direction, d_in == d_out or any overlap of the two ranges, a NULL pointer or a pointer not aligned to
 * 2*sizeof(T) give FOURIER_HIP_INVALID_ARGUMENT.  batch == 0 is a successful no-op.  Stream-ordered on `stream` like
 * fourier_hip_transform_batch_*.  Even N runs an inner N/2-point complex plan plus one untangle sweep (about 3/4 of the bytes
 * of the complex N-point transform); odd N runs the N-point complex plan on a widened copy (a correctness path).  The plan
 * owns a scratch of at most 1 GiB (never less than one row) and walks larger batches in chunks of it; the first call with a
 * batch larger than any before allocates it unless fourier_hip_real_reserve_* was called for at least that batch.
 * fourier_hip_real_describe_* returns "real half-length: <inner plan's describe>" (even N) or "real full-length: <inner plan's
 * describe>" (odd N).  Handles are Send, not Sync, like the complex ones; status of the last call: fourier_hip_real_last_status_*. */
struct fourier_real_fft_float;
struct fourier_real_fft_double;

/* NULL on failure (size 0 included). */
struct fourier_real_fft_float *fourier_hip_real_create_float(FOURIER_SIZE_TYPE size, int device);
struct fourier_real_fft_double *fourier_hip_real_create_double(FOURIER_SIZE_TYPE size, int device);
/* NULL is a no-op. */
void fourier_hip_real_destroy_float(FOURIER_STRUCT fourier_real_fft_float *);
void fourier_hip_real_destroy_double(FOURIER_STRUCT fourier_real_fft_double *);
/* N; 0 for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_real_size_float(const FOURIER_STRUCT fourier_real_fft_float *);
FOURIER_SIZE_TYPE fourier_hip_real_size_double(const FOURIER_STRUCT fourier_real_fft_double *);
int fourier_hip_real_forward_batch_float(const FOURIER_STRUCT fourier_real_fft_float *, const void *d_in, void *d_out,
                                         FOURIER_SIZE_TYPE batch, int transform, void *stream);
int fourier_hip_real_forward_batch_double(const FOURIER_STRUCT fourier_real_fft_double *, const void *d_in, void *d_out,
                                          FOURIER_SIZE_TYPE batch, int transform, void *stream);
int fourier_hip_real_inverse_batch_float(const FOURIER_STRUCT fourier_real_fft_float *, const void *d_in, void *d_out,
                                         FOURIER_SIZE_TYPE batch, int transform, void *stream);
int fourier_hip_real_inverse_batch_double(const FOURIER_STRUCT fourier_real_fft_double *, const void *d_in, void *d_out,
                                          FOURIER_SIZE_TYPE batch, int transform, void *stream);
/* Pre-size the scratch and the inner plan's buffers: afterwards calls of at most `batch` rows never allocate. */
int fourier_hip_real_reserve_float(const FOURIER_STRUCT fourier_real_fft_float *, FOURIER_SIZE_TYPE batch);
int fourier_hip_real_reserve_double(const FOURIER_STRUCT fourier_real_fft_double *, FOURIER_SIZE_TYPE batch);
const char *fourier_hip_real_describe_float(const FOURIER_STRUCT fourier_real_fft_float *);
const char *fourier_hip_real_describe_double(const FOURIER_STRUCT fourier_real_fft_double *);
int fourier_hip_real_last_status_float(const FOURIER_STRUCT fourier_real_fft_float *);
int fourier_hip_real_last_status_double(const FOURIER_STRUCT fourier_real_fft_double *);

/* ---------------- real-input N-D transforms (extension; the reference has none) ------------------------
 * Batched real-input transforms over the trailing `rank` (1 ... 4) dimensions, numpy's rfftn / irfftn layout, on DEVICE memory.
 * A handle is made for the shape [n_1, ..., n_rank] of one item; the last dimension W is the real one:
 *   forward  d_in:  `batch` contiguous items of n_1 x ... x n_{rank-1} x W reals T;
 *            d_out: `batch` contiguous items of n_1 x ... x n_{rank-1} x (W/2+1) interleaved complex T.
 *            FOURIER_TRANSFORM_FFT: rfftn(x); FOURIER_TRANSFORM_SQRT_SCALED_FFT: rfftn(x) / sqrt(P), P = n_1 x ... x W.
 *   inverse  d_in:  items of the half-spectrum shape; d_out: items of reals.
 *            FOURIER_TRANSFORM_IFFT: irfftn(X, s=shape); FOURIER_TRANSFORM_UNSCALED_IFFT: P * irfftn; FOURIER_TRANSFORM_SQRT_SCALED_IFFT:
 *            sqrt(P) * irfftn.  Input that is not Hermitian in columns 0 and W/2 gives numpy's result (the leading inverses run
 *            first, the last axis drops the imaginary parts of its bins 0 and W/2).  d_in is NOT modified.
 * The argument checks and error codes are those of fourier_hip_real_*: a code of the other direction, d_in == d_out or any overlap,
 * a NULL pointer or a pointer not aligned to 2*sizeof(T) give FOURIER_HIP_INVALID_ARGUMENT; batch == 0 is a successful no-op;
 * stream-ordered on `stream`.  Rank 1 runs a real-input plan of length W (the same kernels and bits as fourier_hip_real_*).  Even
 * W (rank >= 2) runs the "packed" route: the W/2-point complex plan on the rows, one axis transform per leading dimension
 * (fourier_hip_transform_axis_*'s routes), one untangle sweep; odd W runs the "composed" route, real rows then the axis transforms
 * (a correctness path).  The plan owns a scratch of at most 1 GiB (never less than one item) and walks larger batches in chunks of
 * whole items; after fourier_hip_realnd_reserve_* for `batch` items, calls of at most `batch` items never allocate.
 * fourier_hip_realnd_describe_* names the route ("realnd packed: ...", "realnd composed: ...", "realnd rank 1: ..."), the row
 * plan and the axis route of each leading dimension.  Handles are Send, not Sync; status of the last call:
 * fourier_hip_realnd_last_status_*. */
struct fourier_realnd_fft_float;
struct fourier_realnd_fft_double;

/* NULL on failure: rank outside 1 ... 4, a NULL shape or a size 0. */
struct fourier_realnd_fft_float *fourier_hip_realnd_create_float(int rank, const FOURIER_SIZE_TYPE *shape, int device);
struct fourier_realnd_fft_double *fourier_hip_realnd_create_double(int rank, const FOURIER_SIZE_TYPE *shape, int device);
/* NULL is a no-op. */
void fourier_hip_realnd_destroy_float(FOURIER_STRUCT fourier_realnd_fft_float *);
void fourier_hip_realnd_destroy_double(FOURIER_STRUCT fourier_realnd_fft_double *);
/* rank; 0 for a NULL handle. */
int fourier_hip_realnd_rank_float(const FOURIER_STRUCT fourier_realnd_fft_float *);
int fourier_hip_realnd_rank_double(const FOURIER_STRUCT fourier_realnd_fft_double *);
int fourier_hip_realnd_forward_batch_float(const FOURIER_STRUCT fourier_realnd_fft_float *, const void *d_in, void *d_out,
                                           FOURIER_SIZE_TYPE batch, int transform, void *stream);
int fourier_hip_realnd_forward_batch_double(const FOURIER_STRUCT fourier_realnd_fft_double *, const void *d_in, void *d_out,
                                            FOURIER_SIZE_TYPE batch, int transform, void *stream);
int fourier_hip_realnd_inverse_batch_float(const FOURIER_STRUCT fourier_realnd_fft_float *, const void *d_in, void *d_out,
                                           FOURIER_SIZE_TYPE batch, int transform, void *stream);
int fourier_hip_realnd_inverse_batch_double(const FOURIER_STRUCT fourier_realnd_fft_double *, const void *d_in, void *d_out,
                                            FOURIER_SIZE_TYPE batch, int transform, void *stream);
/* Pre-size every plan-owned buffer: afterwards calls of at most `batch` items never allocate. */
int fourier_hip_realnd_reserve_float(const FOURIER_STRUCT fourier_realnd_fft_float *, FOURIER_SIZE_TYPE batch);
int fourier_hip_realnd_reserve_double(const FOURIER_STRUCT fourier_realnd_fft_double *, FOURIER_SIZE_TYPE batch);
const char *fourier_hip_realnd_describe_float(const FOURIER_STRUCT fourier_realnd_fft_float *);
const char *fourier_hip_realnd_describe_double(const FOURIER_STRUCT fourier_realnd_fft_double *);
int fourier_hip_realnd_last_status_float(const FOURIER_STRUCT fourier_realnd_fft_float *);
int fourier_hip_realnd_last_status_double(const FOURIER_STRUCT fourier_realnd_fft_double *);

/* ---------------- transforms along a strided axis (extension; the reference has none) ------------------
 * A complex plan of length N transforms along the middle axis of an [outer][N][inner] array of interleaved complex T on DEVICE
 * memory: element (o, j, c) at element offset (o*N + j)*inner + c, the result in the same layout.  inner == 1 is
 * fourier_hip_transform_batch_* with batch = outer (the same kernels, the same bits).  The five transform codes keep their meaning
 * and scaling (an inverse is swap . DFT . swap, the scale computed in T).  d_in == d_out is in place; a partial overlap, a NULL
 * pointer, a pointer not aligned to 2*sizeof(T) or an unknown code give FOURIER_HIP_INVALID_ARGUMENT (and set the handle's last
 * status).  outer * inner == 0 is a successful no-op.  Stream-ordered on `stream` like the batched call.
 * The route depends on N and inner only (fourier_hip_describe_axis_* names it):
 *   inner == 1                                       the plan's own route ("<the plan's describe>")
 *   N <= 32                                          one lane per column, one HBM round trip ("axis lane: N")
 *   N = 2^k in 64 ... 2048, inner a power of two     the last pass of the power-of-two plans down the columns, one round trip
 *     >= the pass's tile width (f32: 32 columns up   ("axis column tile: L=N"); also (N/16) * inner * 2*sizeof(T) <= 2^31
 *     to N = 256, 16 above; f64: half that)
 *   anything else                                    a tiled transpose into plan-owned scratch (at most 1 GiB, walked in chunks),
 *                                                    the plan's transform there, the transpose back ("axis transpose: <describe>")
 * The first call with a larger outer x inner than any before may allocate the scratch unless fourier_hip_reserve_axis_* was called
 * for at least that outer x inner. */
int fourier_hip_transform_axis_float(const FOURIER_STRUCT fourier_fft_float *, const void *d_in, void *d_out,
                                     FOURIER_SIZE_TYPE outer, FOURIER_SIZE_TYPE inner, int transform, void *stream);
int fourier_hip_transform_axis_double(const FOURIER_STRUCT fourier_fft_double *, const void *d_in, void *d_out,
                                      FOURIER_SIZE_TYPE outer, FOURIER_SIZE_TYPE inner, int transform, void *stream);
/* Afterwards, axis calls of at most this outer x inner (with the same inner's route) never allocate. */
int fourier_hip_reserve_axis_float(const FOURIER_STRUCT fourier_fft_float *, FOURIER_SIZE_TYPE outer, FOURIER_SIZE_TYPE inner);
int fourier_hip_reserve_axis_double(const FOURIER_STRUCT fourier_fft_double *, FOURIER_SIZE_TYPE outer, FOURIER_SIZE_TYPE inner);
/* The route an axis call with this `inner` takes (see above); inner == 1 returns fourier_hip_describe_*.  "" for a NULL handle. */
const char *fourier_hip_describe_axis_float(const FOURIER_STRUCT fourier_fft_float *, FOURIER_SIZE_TYPE inner);
const char *fourier_hip_describe_axis_double(const FOURIER_STRUCT fourier_fft_double *, FOURIER_SIZE_TYPE inner);

/* ---------------- convolution with a prepared filter bank (extension; the reference has none) ----------
 * A handle is made for a length N >= 1, a kind of data (real_data == 0: rows of N interleaved complex T, else rows of N reals T) and
 * a device.  It holds a bank of F >= 1 filters, given in the time domain as `filters` contiguous rows of `taps` values of the
 * handle's kind (1 <= taps <= N, zero-extended to N) and transformed once by fourier_hip_conv_set_filters_*.
 * fourier_hip_conv_apply_* then maps `batch` contiguous rows at d_in to `batch` rows at d_out on DEVICE memory, row b with filter
 * b mod F (b counted over the whole call):
 *   convolution (circular, length N)   y[b] = ifft(fft(x[b]) * fft(h[b mod F], N))
 *   correlation (correlate != 0)       y[b] = ifft(fft(x[b]) * conj(fft(h[b mod F], N))),  y[b][n] = sum_m x[b][(n+m) mod N] conj(h[m])
 * scaled as numpy's ifft / irfft (the 1/N lives in the stored spectra).  Real data: real taps, real rows in and out; the half
 * spectrum never leaves the library.  A linear ("full", "same", "valid") convolution is fourier_hip_lconv_* below.
 * d_in == d_out is in place and allowed; any other overlap, a NULL pointer, a pointer not aligned to 2*sizeof(T) (also for real
 * rows; taps: one value of their kind), taps == 0, taps > N, filters == 0, or apply before any filters were set give
 * FOURIER_HIP_INVALID_ARGUMENT.  batch == 0 is a successful no-op.  Both calls are stream-ordered on `stream` like
 * fourier_hip_transform_batch_*: set_filters reads the taps and enqueues the filter transforms there; it may allocate (and so
 * synchronise) when the bank grows.  It may be called again to replace the bank, not while a call on the handle is in flight.
 * Routes, chosen at create (fourier_hip_conv_describe_* names the route and the plan under it):
 *   complex, N = 2^k on two or more tile passes   "conv fused passes: ..."  forward passes but the last, ONE launch for the last
 *     (2^16 and up; f64 2^15 and up)                forward pass, the product and the first inverse pass, the remaining inverse
 *                                                   passes: with two passes 3 round trips of HBM per row instead of 5
 *   complex, N = 2^11 ... 2^15 (f64: ... 2^14),   "conv one-launch: ..."    ONE launch: load, two-level FFT, product, two-level inverse, store on
 *     the one-launch two-level plans                register-resident data: 1 round trip of HBM per row instead of 3; no scratch
 *   complex, any other N                          "conv composed: ..."      forward transform into scratch, one product sweep in
 *                                                   place, unscaled inverse transform
 *   real, even N                                  "conv real fused untangle: ..."  the N/2-point plan forward into scratch, ONE sweep
 *                                                   (untangle, product with the half spectrum, retangle) in place, the N/2-point
 *                                                   plan's unscaled inverse
 *   real, odd N                                   "conv real composed: ..." rfft into scratch, product sweep, unscaled irfft
 * Option "fusion" (fourier_hip_conv_set_option_*): 1 (default) as above, 0 = the composed route of the handle's kind.
 * Bytes per row, algorithmic, the bank not counted (with one filter it stays in the L2; with many every row reads one more
 * spectrum): complex two-pass fused 6 N E against 10 N E composed (E = 2*sizeof(T)); real fused 5 (N/2) E against 7 (N/2) E.
 * Device memory the handle owns: the bank, F x N complex (real data: F x (N/2+1)), the plans' own tables and buffers, and a scratch
 * of at most 1 GiB (never less than one row); larger batches are walked in chunks of it.  A real-data handle sits on a whole
 * real-input plan (fourier_hip_real_*), which transforms the filters and runs the composed route, and so also keeps that plan's own
 * scratch, sized by the largest number of filters set so far (at most 1 GiB more).  After fourier_hip_conv_reserve_* for `batch`
 * rows, apply calls of at most `batch` rows on the route of that moment never allocate; after a change of "fusion" call reserve
 * again.  The taps are read with plain loads and need the alignment of one value of their kind only.  Handles are Send, not Sync; the status of the last call that
 * did work (set_filters, apply, reserve) is fourier_hip_conv_last_status_*. */
struct fourier_conv_float;
struct fourier_conv_double;

/* NULL on failure (size 0 included). */
struct fourier_conv_float *fourier_hip_conv_create_float(FOURIER_SIZE_TYPE size, int real_data, int device);
struct fourier_conv_double *fourier_hip_conv_create_double(FOURIER_SIZE_TYPE size, int real_data, int device);
/* NULL is a no-op. */
void fourier_hip_conv_destroy_float(FOURIER_STRUCT fourier_conv_float *);
void fourier_hip_conv_destroy_double(FOURIER_STRUCT fourier_conv_double *);
/* N; 0 for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_conv_size_float(const FOURIER_STRUCT fourier_conv_float *);
FOURIER_SIZE_TYPE fourier_hip_conv_size_double(const FOURIER_STRUCT fourier_conv_double *);
/* F; 0 before set_filters and for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_conv_filters_float(const FOURIER_STRUCT fourier_conv_float *);
FOURIER_SIZE_TYPE fourier_hip_conv_filters_double(const FOURIER_STRUCT fourier_conv_double *);
int fourier_hip_conv_set_filters_float(FOURIER_STRUCT fourier_conv_float *, const void *d_taps, FOURIER_SIZE_TYPE taps,
                                       FOURIER_SIZE_TYPE filters, int correlate, void *stream);
int fourier_hip_conv_set_filters_double(FOURIER_STRUCT fourier_conv_double *, const void *d_taps, FOURIER_SIZE_TYPE taps,
                                        FOURIER_SIZE_TYPE filters, int correlate, void *stream);
int fourier_hip_conv_apply_float(const FOURIER_STRUCT fourier_conv_float *, const void *d_in, void *d_out,
                                 FOURIER_SIZE_TYPE batch, void *stream);
int fourier_hip_conv_apply_double(const FOURIER_STRUCT fourier_conv_double *, const void *d_in, void *d_out,
                                  FOURIER_SIZE_TYPE batch, void *stream);
/* Pre-size the scratch and the plans' buffers: afterwards apply calls of at most `batch` rows never allocate. */
int fourier_hip_conv_reserve_float(const FOURIER_STRUCT fourier_conv_float *, FOURIER_SIZE_TYPE batch);
int fourier_hip_conv_reserve_double(const FOURIER_STRUCT fourier_conv_double *, FOURIER_SIZE_TYPE batch);
/* "fusion": 1 (default) / 0 = the composed route.  FOURIER_HIP_INVALID_ARGUMENT for anything else. */
int fourier_hip_conv_set_option_float(FOURIER_STRUCT fourier_conv_float *, const char *key, long long value);
int fourier_hip_conv_set_option_double(FOURIER_STRUCT fourier_conv_double *, const char *key, long long value);
/* "" for a NULL handle. */
const char *fourier_hip_conv_describe_float(const FOURIER_STRUCT fourier_conv_float *);
const char *fourier_hip_conv_describe_double(const FOURIER_STRUCT fourier_conv_double *);
int fourier_hip_conv_last_status_float(const FOURIER_STRUCT fourier_conv_float *);
int fourier_hip_conv_last_status_double(const FOURIER_STRUCT fourier_conv_double *);

/* ---------------- N-D convolution with a prepared filter bank (extension; the reference has none) ----------
 * A handle is made for a transform shape S = [n_1, ..., n_{r-1}, W] of rank r = 2, 3 or 4 (every length >= 1; P = prod S) and a
 * device.  It serves REAL data over the trailing r dimensions of contiguous items; rank 1 is fourier_hip_conv_* (real_data != 0) and
 * is refused here (FOURIER_HIP_UNSUPPORTED: create returns NULL), as is a rank above 4.  The item bounds are fourier_hip_realnd_*'s.
 * The handle holds a bank of F >= 1 filters, given in the time domain as `filters` contiguous blocks of taps_shape <= S reals (every
 * length >= 1) and transformed once by fourier_hip_convnd_set_filters_* with the handle's own forward transform in T.
 * fourier_hip_convnd_apply_batch_* maps `batch` contiguous items of in_shape reals at d_in to `batch` items of out_shape reals at
 * d_out on DEVICE memory.  Item b
 *   is zero-extended from in_shape <= S to S at the high end of every dimension,
 *   is convolved circularly over S with filter f = (filter_first + b) mod F (b counted over the whole call),
 *       y = irfftn(rfftn(x, S) * H[f], S),   H[f] = rfftn(h[f] zero-extended to S) / P   (conj H[f] where correlate != 0:
 *       y[n] = sum_m x[(n + m) mod S] h[m], the circular correlation),
 *   and the window [out_first, out_first + out_shape) of y is stored; out_first + out_shape <= S in every dimension, the window never
 *   wraps.
 * fourier_hip_convnd_set_window_* sets in_shape, out_first and out_shape (arrays of r lengths; host state, no device work; the
 * default is S, 0, S) and may be called between applies.  With in_shape = a, taps k, S >= a + k - 1, out_first = 0 / (k - 1) / 2 /
 * k - 1 and out_shape = a + k - 1 / a / a - k + 1 the items are scipy.signal.convolve's "full" / "same" / "valid".
 * The bins that are their own mirror (columns 0 and W/2 of the rows that are their own mirror row) are real and are multiplied by
 * the real part of H, as numpy's irfftn drops their imaginary parts.  No atomics: a repetition is bit-equal, and scaling the input by
 * a power of two scales the output exactly.
 * d_in == d_out is in place and allowed when in_shape == out_shape == S; any other overlap, a NULL pointer, a pointer not aligned to
 * 2*sizeof(T) (taps: sizeof(T)), a length of 0 or above S in taps_shape, in_shape or out_shape, a window beyond S, filters == 0, or
 * apply before any filters were set give FOURIER_HIP_INVALID_ARGUMENT.  batch == 0 is a successful no-op.  set_filters and apply are
 * stream-ordered on `stream` like fourier_hip_transform_batch_*; set_filters may allocate (and so synchronise) when the bank grows,
 * and may be called again to replace the bank, not while a call on the handle is in flight.
 * Routes, chosen at create (fourier_hip_convnd_describe_* names the route and the plans under it):
 *   even W   "convnd fused untangle: ..."  [a pad sweep into the scratch where in_shape != S,] the W/2-point row plan forward on the
 *                                          packed reals, the leading axes' transforms in place, ONE sweep in place (untangle with the
 *                                          mirror rows, product with the half spectrum, retangle), the axes' unscaled inverses, the
 *                                          row plan's unscaled inverse [and a crop sweep under any window but the whole of S].
 *                                          The half spectrum never reaches memory.
 *   odd W    "convnd composed: ..."        [pad,] rfftn into a half-spectrum scratch, one product sweep in place, unscaled irfftn
 *                                          [, crop]
 * Option "fusion" (fourier_hip_convnd_set_option_*): 1 = as above, 0 = the composed route for every W.  The default is the value
 * that measured faster (README.md, "N-D convolution").
 * Bytes per item of N = P reals of f32, algorithmic, the bank not counted: fused 40 N (rows 8 N + 8 N, axes 8 N + 8 N, the sweep
 * 8 N) against 56 N composed (rfftn 24 N, product 8 N, irfftn 24 N); a window adds its copy.
 * Device memory the handle owns: the bank, F x P/W x (W/2 + 1) complex, the plans' own tables and buffers, and a scratch of at most
 * 1 GiB (never less than one item); larger batches are walked in chunks of whole items.  The handle sits on a whole real-input N-D
 * plan (fourier_hip_realnd_*), which transforms the filters and runs the composed route, and so also keeps that plan's own scratch.
 * After fourier_hip_convnd_reserve_* for `batch` items, apply calls of at most `batch` items on the route of that moment never
 * allocate; after a change of "fusion" call reserve again.  Handles are Send, not Sync; the status of the last call that did work
 * (set_filters, set_window, apply_batch, reserve) is fourier_hip_convnd_last_status_*. */
struct fourier_convnd_float;
struct fourier_convnd_double;

/* NULL on failure (rank outside 2 ... 4, a NULL shape or a length of 0 included). */
struct fourier_convnd_float *fourier_hip_convnd_create_float(int rank, const FOURIER_SIZE_TYPE *shape, int device);
struct fourier_convnd_double *fourier_hip_convnd_create_double(int rank, const FOURIER_SIZE_TYPE *shape, int device);
/* NULL is a no-op. */
void fourier_hip_convnd_destroy_float(FOURIER_STRUCT fourier_convnd_float *);
void fourier_hip_convnd_destroy_double(FOURIER_STRUCT fourier_convnd_double *);
/* r; 0 for a NULL handle. */
int fourier_hip_convnd_rank_float(const FOURIER_STRUCT fourier_convnd_float *);
int fourier_hip_convnd_rank_double(const FOURIER_STRUCT fourier_convnd_double *);
/* S into out[0 .. r-1]; FOURIER_HIP_INVALID_ARGUMENT for a NULL handle or a NULL out. */
int fourier_hip_convnd_shape_float(const FOURIER_STRUCT fourier_convnd_float *, FOURIER_SIZE_TYPE *out);
int fourier_hip_convnd_shape_double(const FOURIER_STRUCT fourier_convnd_double *, FOURIER_SIZE_TYPE *out);
/* F; 0 before set_filters and for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_convnd_filters_float(const FOURIER_STRUCT fourier_convnd_float *);
FOURIER_SIZE_TYPE fourier_hip_convnd_filters_double(const FOURIER_STRUCT fourier_convnd_double *);
int fourier_hip_convnd_set_filters_float(FOURIER_STRUCT fourier_convnd_float *, const void *d_taps, const FOURIER_SIZE_TYPE *taps_shape,
                                         FOURIER_SIZE_TYPE filters, int correlate, void *stream);
int fourier_hip_convnd_set_filters_double(FOURIER_STRUCT fourier_convnd_double *, const void *d_taps, const FOURIER_SIZE_TYPE *taps_shape,
                                          FOURIER_SIZE_TYPE filters, int correlate, void *stream);
int fourier_hip_convnd_set_window_float(FOURIER_STRUCT fourier_convnd_float *, const FOURIER_SIZE_TYPE *in_shape,
                                        const FOURIER_SIZE_TYPE *out_first, const FOURIER_SIZE_TYPE *out_shape);
int fourier_hip_convnd_set_window_double(FOURIER_STRUCT fourier_convnd_double *, const FOURIER_SIZE_TYPE *in_shape,
                                         const FOURIER_SIZE_TYPE *out_first, const FOURIER_SIZE_TYPE *out_shape);
int fourier_hip_convnd_apply_batch_float(const FOURIER_STRUCT fourier_convnd_float *, const void *d_in, void *d_out,
                                         FOURIER_SIZE_TYPE batch, FOURIER_SIZE_TYPE filter_first, void *stream);
int fourier_hip_convnd_apply_batch_double(const FOURIER_STRUCT fourier_convnd_double *, const void *d_in, void *d_out,
                                          FOURIER_SIZE_TYPE batch, FOURIER_SIZE_TYPE filter_first, void *stream);
/* Pre-size the scratch and the plans' buffers: afterwards apply calls of at most `batch` items never allocate. */
int fourier_hip_convnd_reserve_float(const FOURIER_STRUCT fourier_convnd_float *, FOURIER_SIZE_TYPE batch);
int fourier_hip_convnd_reserve_double(const FOURIER_STRUCT fourier_convnd_double *, FOURIER_SIZE_TYPE batch);
/* "fusion": 1 / 0 = the composed route.  FOURIER_HIP_INVALID_ARGUMENT for anything else. */
int fourier_hip_convnd_set_option_float(FOURIER_STRUCT fourier_convnd_float *, const char *key, long long value);
int fourier_hip_convnd_set_option_double(FOURIER_STRUCT fourier_convnd_double *, const char *key, long long value);
/* "" for a NULL handle. */
const char *fourier_hip_convnd_describe_float(const FOURIER_STRUCT fourier_convnd_float *);
const char *fourier_hip_convnd_describe_double(const FOURIER_STRUCT fourier_convnd_double *);
int fourier_hip_convnd_last_status_float(const FOURIER_STRUCT fourier_convnd_float *);
int fourier_hip_convnd_last_status_double(const FOURIER_STRUCT fourier_convnd_double *);

/* ---------------- linear convolution with a prepared filter bank by overlap-save (extension; the reference has none) ----------
 * A handle is made for a row length Lx >= 1, a tap count K >= 1, a mode, a kind of data (real_data == 0: rows of interleaved complex
 * T with complex taps, else rows of reals T with real taps) and a device.  It holds a bank of F >= 1 filters of K taps, given in the
 * time domain as `filters` contiguous rows of K values of the handle's kind and transformed once by fourier_hip_lconv_set_filters_*.
 * fourier_hip_lconv_apply_* maps `batch` contiguous rows of Lx values at d_in to `batch` contiguous rows of Lout values at d_out on
 * DEVICE memory, row b with filter b mod F (b counted over the whole call):
 *   full[b] = x[b] * h[b mod F]          the linear convolution of Lx + K - 1 values, numpy.convolve(x, h)
 *   y[b]    = full[b][off : off + Lout]  FOURIER_LCONV_FULL   off = 0,          Lout = Lx + K - 1
 *                                        FOURIER_LCONV_SAME   off = (K - 1) / 2, Lout = Lx          (integer division)
 *                                        FOURIER_LCONV_VALID  off = K - 1,      Lout = Lx - K + 1  (needs K <= Lx)
 * the lengths of scipy.signal.fftconvolve for K <= Lx.  With correlate != 0 set_filters stores conj(h[K-1-i]) in place of h[i], and
 * the rows are numpy.correlate(x, h, mode); apply does not know about it.
 * d_in and d_out may not overlap at all (d_in == d_out included: the blocks of a row overlap and the row strides differ); an overlap,
 * a NULL pointer, a pointer not aligned to one value of the handle's kind, filters == 0 or apply before any filters were set give
 * FOURIER_HIP_INVALID_ARGUMENT; create returns NULL for Lx == 0, K == 0, an unknown mode, FOURIER_LCONV_VALID with K > Lx, and for rows
 * of more than 2^31 bytes on either side.  batch == 0 is a successful no-op.  Calls are stream-ordered on `stream` like
 * fourier_hip_conv_*.
 * Routes, chosen at create and named by fourier_hip_lconv_describe_*:
 *   "lconv overlap-save: block N step S blocks nb[ real pairs], <block plan>"   ONE launch per apply, no scratch.  Every row is cut
 *     into nb = ceil((Lx + K - 1) / S) overlapping blocks of N = 2^11 ... 2^15 (f64: ... 2^14) values, S = floor((N - (K - 1)) / A) * A
 *     with A = 128 / (2 sizeof(T)) values (one 128-byte line of complex data).  One workgroup loads block j from position j*S - (N - S)
 *     of its row (zeros outside the row), transforms it on register-resident data, multiplies by the filter's N-point spectrum,
 *     transforms back, drops the first N - S values and stores the others at j*S - off where that lies in the output row.  Real rows:
 *     one workgroup takes blocks 2j and 2j + 1 as the real and the imaginary part of one complex block (the taps are real); float
 *     rows of even Lx, Lout and off at 8-byte aligned pointers move two reals per access, all others one.  The
 *     bank is F x N complex values in both kinds.  Bytes per row, algorithmic: (Lx + Lout) values; the N - S values neighbouring
 *     blocks share are read twice, the second time from the L2.
 *   "lconv padded: M=..., <circular handle>"   filters too long for a block, or option "overlap_save" = 0: the rows zero-padded into
 *     the handle's scratch, the circular handle (fourier_hip_conv_*) of M = the smallest power of two >= Lx + K - 1 in place there,
 *     a crop sweep to the output: the circular handle's bytes per row of M values plus (Lx + M) and (M + Lout) values for the two
 *     sweeps.  The batch is walked in chunks of a scratch of at most 1 GiB (never less than one row); fourier_hip_lconv_reserve_*
 *     for `batch` rows makes later apply calls of at most `batch` rows allocation-free (the overlap-save route has nothing to size).
 * Block rule: float handles first take the smallest N = 2^11 ... 2^13 with N >= 8 (K - 1) where the row has more than one such block
 * (N < Lx + K - 1; measured faster than the next rule's block there); then, and double handles at once, the smallest N = 2^11 ...
 * with N >= 4 (K - 1); where there is none, the largest N if N >= 2 (K - 1); else the padded route.  Options (fourier_hip_lconv_set_option_*): "block" = 11 ... 15 forces N = 2^value (FOURIER_HIP_INVALID_ARGUMENT where the
 * precision has no such block or N < K - 1 + A), 0 = the rule; "overlap_save" = 0 selects the padded route, 1 (default) the rule.
 * An option that changes the route or the block drops the bank: set the filters again.  Handles are Send, not Sync; the status of the
 * last call that did work (set_filters, apply, reserve) is fourier_hip_lconv_last_status_*. */
enum fourier_lconv_mode {
  FOURIER_LCONV_FULL = 0,
  FOURIER_LCONV_SAME = 1,
  FOURIER_LCONV_VALID = 2,
};
struct fourier_lconv_float;
struct fourier_lconv_double;

/* NULL on failure. */
struct fourier_lconv_float *fourier_hip_lconv_create_float(FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE taps, int mode, int real_data,
                                                           int device);
struct fourier_lconv_double *fourier_hip_lconv_create_double(FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE taps, int mode, int real_data,
                                                             int device);
/* NULL is a no-op. */
void fourier_hip_lconv_destroy_float(FOURIER_STRUCT fourier_lconv_float *);
void fourier_hip_lconv_destroy_double(FOURIER_STRUCT fourier_lconv_double *);
/* Lx, K, Lout, F (0 before set_filters); 0 for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_lconv_length_float(const FOURIER_STRUCT fourier_lconv_float *);
FOURIER_SIZE_TYPE fourier_hip_lconv_length_double(const FOURIER_STRUCT fourier_lconv_double *);
FOURIER_SIZE_TYPE fourier_hip_lconv_taps_float(const FOURIER_STRUCT fourier_lconv_float *);
FOURIER_SIZE_TYPE fourier_hip_lconv_taps_double(const FOURIER_STRUCT fourier_lconv_double *);
FOURIER_SIZE_TYPE fourier_hip_lconv_out_length_float(const FOURIER_STRUCT fourier_lconv_float *);
FOURIER_SIZE_TYPE fourier_hip_lconv_out_length_double(const FOURIER_STRUCT fourier_lconv_double *);
FOURIER_SIZE_TYPE fourier_hip_lconv_filters_float(const FOURIER_STRUCT fourier_lconv_float *);
FOURIER_SIZE_TYPE fourier_hip_lconv_filters_double(const FOURIER_STRUCT fourier_lconv_double *);
/* `filters` rows of K values of the handle's kind at d_taps -> the bank. */
int fourier_hip_lconv_set_filters_float(FOURIER_STRUCT fourier_lconv_float *, const void *d_taps, FOURIER_SIZE_TYPE filters,
                                        int correlate, void *stream);
int fourier_hip_lconv_set_filters_double(FOURIER_STRUCT fourier_lconv_double *, const void *d_taps, FOURIER_SIZE_TYPE filters,
                                        int correlate, void *stream);
int fourier_hip_lconv_apply_float(const FOURIER_STRUCT fourier_lconv_float *, const void *d_in, void *d_out,
                                  FOURIER_SIZE_TYPE batch, void *stream);
int fourier_hip_lconv_apply_double(const FOURIER_STRUCT fourier_lconv_double *, const void *d_in, void *d_out,
                                  FOURIER_SIZE_TYPE batch, void *stream);
int fourier_hip_lconv_reserve_float(const FOURIER_STRUCT fourier_lconv_float *, FOURIER_SIZE_TYPE batch);
int fourier_hip_lconv_reserve_double(const FOURIER_STRUCT fourier_lconv_double *, FOURIER_SIZE_TYPE batch);
int fourier_hip_lconv_set_option_float(FOURIER_STRUCT fourier_lconv_float *, const char *key, long long value);
int fourier_hip_lconv_set_option_double(FOURIER_STRUCT fourier_lconv_double *, const char *key, long long value);
/* "" for a NULL handle. */
const char *fourier_hip_lconv_describe_float(const FOURIER_STRUCT fourier_lconv_float *);
const char *fourier_hip_lconv_describe_double(const FOURIER_STRUCT fourier_lconv_double *);
int fourier_hip_lconv_last_status_float(const FOURIER_STRUCT fourier_lconv_float *);
int fourier_hip_lconv_last_status_double(const FOURIER_STRUCT fourier_lconv_double *);

/* ---------------- real-to-real transforms: DCT and DST of types II and III (extension; the reference has none) ----------
 * Batched discrete cosine / sine transforms of length N >= 1 on DEVICE memory, scipy.fft's dct / dst definitions (FFTW's REDFT10,
 * REDFT01, RODFT10, RODFT01): `batch` rows of N reals T in, row b at element offset b*N, `batch` rows of N reals out.
 *   FOURIER_R2R_DCT2  X[k] = 2 sum_n x[n] cos(pi k (2n+1) / 2N)
 *   FOURIER_R2R_DCT3  x[n] = X[0] + 2 sum_{k>=1} X[k] cos(pi k (2n+1) / 2N)         (DCT3(DCT2(x)) = 2N x)
 *   FOURIER_R2R_DST2  X[k] = 2 sum_n x[n] sin(pi (k+1) (2n+1) / 2N)
 *   FOURIER_R2R_DST3  x[n] = (-1)^n X[N-1] + 2 sum_{k<N-1} X[k] sin(pi (k+1) (2n+1) / 2N)   (DST3(DST2(x)) = 2N x)
 * times the norm's factor: FOURIER_R2R_NORM_BACKWARD 1, FOURIER_R2R_NORM_FORWARD 1/2N, FOURIER_R2R_NORM_ORTHO 1/sqrt(2N) in scipy's
 * orthogonalised form (DCT2's X[0] and DST2's X[N-1] times 1/sqrt 2, DCT3's input X[0] and DST3's input X[N-1] times sqrt 2), whose
 * matrices are orthogonal.  The inverse of a type-II transform is the type-III one with BACKWARD and FORWARD exchanged (scipy's idct /
 * idst), and the other way round.  One handle serves every kind and norm.
 * d_in == d_out is in place and allowed; any other overlap, a NULL pointer, a pointer not aligned to 2*sizeof(T), a kind or norm
 * outside the enums give FOURIER_HIP_INVALID_ARGUMENT.  batch == 0 is a successful no-op.  Stream-ordered on `stream` like
 * fourier_hip_transform_batch_*.  Even N runs an inner N/2-point complex plan between two linear sweeps (pack and post, or pre and
 * unpack), each one read and one write of the rows; odd N runs the N-point complex plan on a widened copy (a correctness path).  The
 * plan owns a scratch of at most 1 GiB (never less than one row) and walks larger batches in chunks of it; the first call with a
 * batch larger than any before allocates it unless fourier_hip_r2r_reserve_* was called for at least that batch.
 * fourier_hip_r2r_describe_* returns "r2r half-length: <inner plan's describe>" (even N) or "r2r full-length: <inner plan's
 * describe>" (odd N).  Handles are Send, not Sync, like the complex ones; status of the last call: fourier_hip_r2r_last_status_*. */
enum {
  FOURIER_R2R_DCT2 = 0,
  FOURIER_R2R_DCT3 = 1,
  FOURIER_R2R_DST2 = 2,
  FOURIER_R2R_DST3 = 3,
};
enum {
  FOURIER_R2R_NORM_BACKWARD = 0,
  FOURIER_R2R_NORM_ORTHO = 1,
  FOURIER_R2R_NORM_FORWARD = 2,
};
struct fourier_r2r_float;
struct fourier_r2r_double;

/* NULL on failure (size 0 included). */
struct fourier_r2r_float *fourier_hip_r2r_create_float(FOURIER_SIZE_TYPE size, int device);
struct fourier_r2r_double *fourier_hip_r2r_create_double(FOURIER_SIZE_TYPE size, int device);
/* NULL is a no-op. */
void fourier_hip_r2r_destroy_float(FOURIER_STRUCT fourier_r2r_float *);
void fourier_hip_r2r_destroy_double(FOURIER_STRUCT fourier_r2r_double *);
/* N; 0 for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_r2r_size_float(const FOURIER_STRUCT fourier_r2r_float *);
FOURIER_SIZE_TYPE fourier_hip_r2r_size_double(const FOURIER_STRUCT fourier_r2r_double *);
int fourier_hip_r2r_transform_batch_float(const FOURIER_STRUCT fourier_r2r_float *, const void *d_in, void *d_out,
                                          FOURIER_SIZE_TYPE batch, int kind, int norm, void *stream);
int fourier_hip_r2r_transform_batch_double(const FOURIER_STRUCT fourier_r2r_double *, const void *d_in, void *d_out,
                                           FOURIER_SIZE_TYPE batch, int kind, int norm, void *stream);
/* Pre-size the scratch and the inner plan's buffers: afterwards calls of at most `batch` rows never allocate. */
int fourier_hip_r2r_reserve_float(const FOURIER_STRUCT fourier_r2r_float *, FOURIER_SIZE_TYPE batch);
int fourier_hip_r2r_reserve_double(const FOURIER_STRUCT fourier_r2r_double *, FOURIER_SIZE_TYPE batch);
const char *fourier_hip_r2r_describe_float(const FOURIER_STRUCT fourier_r2r_float *);
const char *fourier_hip_r2r_describe_double(const FOURIER_STRUCT fourier_r2r_double *);
int fourier_hip_r2r_last_status_float(const FOURIER_STRUCT fourier_r2r_float *);
int fourier_hip_r2r_last_status_double(const FOURIER_STRUCT fourier_r2r_double *);

/* ---------------- short-time Fourier transform and its inverse (extension; the reference has none) ----------
 * torch.stft / torch.istft with onesided = True, return_complex = True, on DEVICE memory.  A handle is made for n_fft >= 1, hop >= 1,
 * win_length in 1 ... n_fft and a pad mode: FOURIER_STFT_PAD_NONE (torch's center = False), FOURIER_STFT_PAD_REFLECT or
 * FOURIER_STFT_PAD_ZERO (center = True with p = n_fft / 2 samples, integer division, of padding on each side; p' = p below, 0 without
 * padding).  The padding is index arithmetic at the load (reflect: t < 0 -> -t, t >= length -> 2 (length - 1) - t); no padded copy exists.
 * Window: fourier_hip_stft_set_window_* takes win_length reals T on the device, centred in the frame ((n_fft - win_length) / 2 zeros
 * in front); NULL restores the default of all ones (torch's window = None).  A set-up call: it waits for `stream`.
 * Frames of a row of `length` reals (fourier_hip_stft_frames_*; 0 where the length is invalid): PAD_NONE 1 + (length - n_fft) / hop
 * for length >= n_fft; otherwise 1 + (length + 2 p - n_fft) / hop as torch, which is 1 + length / hop for even n_fft, where PAD_REFLECT
 * needs length > p.  bins = n_fft / 2 + 1.
 * Forward: `batch` contiguous rows of `length` reals in; batch x frames x bins interleaved complex out, FRAME-MAJOR: frame f of row b at
 * complex offset (b * frames + f) * bins (torch's (bins, frames) is the transposed view of a row's block),
 *   X[b, f, k] = sum_n w[n] xpad[b, f hop + n] exp(-2 pi i k n / n_fft),   times n_fft^-1/2 where normalized != 0.
 * Inverse: batch x frames x bins in, `batch` rows of `length` reals out, 1 <= length <= hop (frames - 1) + n_fft - 2 p',
 *   y[t] = (sum_f w[t + p' - f hop] frame_f[t + p' - f hop]) / (sum_f w[t + p' - f hop]^2),   frame_f = irfft(X[b, f], n_fft),
 * times n_fft^1/2 where normalized != 0.  Where the envelope sum_f w^2 falls below 1e-11 on a kept sample (torch's NOLA check) the call
 * returns FOURIER_HIP_INVALID_ARGUMENT.  The envelope is computed on the host in f64 on first use of a (frames, length) and cached.
 * The overlap-add is a gather, one lane per output sample: no atomics, deterministic.
 * A NULL handle or pointer, reals not aligned to sizeof(T) or complex values not aligned to 2 * sizeof(T), any overlap of d_in and d_out
 * or an invalid length give FOURIER_HIP_INVALID_ARGUMENT; batch == 0 is a successful no-op.  Stream-ordered on `stream` like
 * fourier_hip_transform_batch_*.  Routes (fourier_hip_stft_describe_*: "<forward route>, istft composed: <the real plan's describe>"):
 *   "stft composed"    any n_fft: a gather sweep windows the frames of a chunk into a handle-owned scratch (at most 1 GiB, never less
 *                      than one frame), the real-input plan transforms them into the output.
 *   "stft fused rows"  n_fft = 2h whose h-point plan is one whole-row kernel (n_fft 128 ... 1024, f32 also 2048): gather, window,
 *                      transform and untangle in ONE launch, no scratch.  Option "fusion" = 0 forces the composed route, 1 takes the
 *                      fused one wherever it exists.
 * The inverse runs the real-input plan's inverse into the scratch and the overlap-add sweep, in chunks of whole rows, or of ranges of
 * one row's samples where a row's frames exceed the bound.  fourier_hip_stft_reserve_*(h, length, batch) sizes everything forward calls
 * of at most `batch` rows of `length` reals, and inverse calls to that length from frames(length) frames, need: they then never
 * allocate.  Handles are Send, not Sync, like the complex ones; status of the last call: fourier_hip_stft_last_status_*. */
enum {
  FOURIER_STFT_PAD_NONE = 0,
  FOURIER_STFT_PAD_REFLECT = 1,
  FOURIER_STFT_PAD_ZERO = 2,
};
struct fourier_stft_float;
struct fourier_stft_double;

/* NULL on failure (parameters outside the ranges above included). */
struct fourier_stft_float *fourier_hip_stft_create_float(FOURIER_SIZE_TYPE n_fft, FOURIER_SIZE_TYPE hop, FOURIER_SIZE_TYPE win_length,
                                                         int pad_mode, int device);
struct fourier_stft_double *fourier_hip_stft_create_double(FOURIER_SIZE_TYPE n_fft, FOURIER_SIZE_TYPE hop, FOURIER_SIZE_TYPE win_length,
                                                           int pad_mode, int device);
/* NULL is a no-op. */
void fourier_hip_stft_destroy_float(FOURIER_STRUCT fourier_stft_float *);
void fourier_hip_stft_destroy_double(FOURIER_STRUCT fourier_stft_double *);
/* 0 for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_stft_n_fft_float(const FOURIER_STRUCT fourier_stft_float *);
FOURIER_SIZE_TYPE fourier_hip_stft_n_fft_double(const FOURIER_STRUCT fourier_stft_double *);
FOURIER_SIZE_TYPE fourier_hip_stft_hop_float(const FOURIER_STRUCT fourier_stft_float *);
FOURIER_SIZE_TYPE fourier_hip_stft_hop_double(const FOURIER_STRUCT fourier_stft_double *);
FOURIER_SIZE_TYPE fourier_hip_stft_win_length_float(const FOURIER_STRUCT fourier_stft_float *);
FOURIER_SIZE_TYPE fourier_hip_stft_win_length_double(const FOURIER_STRUCT fourier_stft_double *);
FOURIER_SIZE_TYPE fourier_hip_stft_bins_float(const FOURIER_STRUCT fourier_stft_float *);
FOURIER_SIZE_TYPE fourier_hip_stft_bins_double(const FOURIER_STRUCT fourier_stft_double *);
/* frames of a row of `length` reals; 0 for an invalid length or a NULL handle */
FOURIER_SIZE_TYPE fourier_hip_stft_frames_float(const FOURIER_STRUCT fourier_stft_float *, FOURIER_SIZE_TYPE length);
FOURIER_SIZE_TYPE fourier_hip_stft_frames_double(const FOURIER_STRUCT fourier_stft_double *, FOURIER_SIZE_TYPE length);
int fourier_hip_stft_set_window_float(FOURIER_STRUCT fourier_stft_float *, const void *d_window, void *stream);
int fourier_hip_stft_set_window_double(FOURIER_STRUCT fourier_stft_double *, const void *d_window, void *stream);
int fourier_hip_stft_forward_float(const FOURIER_STRUCT fourier_stft_float *, const void *d_in, void *d_out, FOURIER_SIZE_TYPE length,
                                   FOURIER_SIZE_TYPE batch, int normalized, void *stream);
int fourier_hip_stft_forward_double(const FOURIER_STRUCT fourier_stft_double *, const void *d_in, void *d_out, FOURIER_SIZE_TYPE length,
                                    FOURIER_SIZE_TYPE batch, int normalized, void *stream);
int fourier_hip_stft_inverse_float(const FOURIER_STRUCT fourier_stft_float *, const void *d_in, void *d_out, FOURIER_SIZE_TYPE frames,
                                   FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch, int normalized, void *stream);
int fourier_hip_stft_inverse_double(const FOURIER_STRUCT fourier_stft_double *, const void *d_in, void *d_out, FOURIER_SIZE_TYPE frames,
                                    FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch, int normalized, void *stream);
int fourier_hip_stft_reserve_float(const FOURIER_STRUCT fourier_stft_float *, FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch);
int fourier_hip_stft_reserve_double(const FOURIER_STRUCT fourier_stft_double *, FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch);
/* "fusion": 0 = the composed forward route, 1 = the fused one wherever it exists.  Anything else: FOURIER_HIP_INVALID_ARGUMENT. */
int fourier_hip_stft_set_option_float(FOURIER_STRUCT fourier_stft_float *, const char *key, long long value);
int fourier_hip_stft_set_option_double(FOURIER_STRUCT fourier_stft_double *, const char *key, long long value);
/* "" for a NULL handle. */
const char *fourier_hip_stft_describe_float(const FOURIER_STRUCT fourier_stft_float *);
const char *fourier_hip_stft_describe_double(const FOURIER_STRUCT fourier_stft_double *);
int fourier_hip_stft_last_status_float(const FOURIER_STRUCT fourier_stft_float *);
int fourier_hip_stft_last_status_double(const FOURIER_STRUCT fourier_stft_double *);

/* ---------------- modified discrete cosine transform and its inverse (extension; the reference has none) ----------
 * The lapped transform of AAC, Vorbis and Opus, on DEVICE memory.  A handle is made for n >= 1 coefficients per frame and a `center`
 * flag; a frame is 2n samples and the hop is n.
 * Window: fourier_hip_mdct_set_window_* takes 2n reals T on the device; NULL restores the default, the sine window
 * w[m] = sin(pi (m + 1/2) / 2n), computed on the host in f64 and cast.  A set-up call: it waits for `stream`.
 * Padding: with center != 0 the row is treated as if n zeros stood in front of it and zeros behind it (xpad; p = n below, 0 without) --
 * index arithmetic at the load, no padded copy exists.  Frames of a row of `length` reals (fourier_hip_mdct_frames_*; 0 where the
 * length is invalid): with center ceil(length / n) + 1 for length >= 1; without, length / n - 1 (integer division) for length >= 2n,
 * and the samples behind the last whole frame are ignored.
 * Forward: `batch` contiguous rows of `length` reals in; batch x frames x n reals out, FRAME-MAJOR: frame f of row b at element offset
 * (b * frames + f) * n,
 *   X[b, f, k] = sum_{m=0}^{2n-1} w[m] xpad[b, f n + m] cos(pi/n (m + 1/2 + n/2)(k + 1/2)),  k = 0 ... n-1,
 * times sqrt(2/n) where normalized != 0 (the orthogonal TDAC scaling).
 * Inverse: batch x frames x n reals in, `batch` rows of `length` reals out, 1 <= length <= (frames - 1) n with center and
 * 1 <= length <= (frames + 1) n without,
 *   y[b, t] = (2/n) sum_f w[t + p - f n] Y_f[t + p - f n],   Y_f[m] = sum_k X[b, f, k] cos(pi/n (m + 1/2 + n/2)(k + 1/2)),
 * over the at most two frames that cover t; sqrt(2/n) instead of 2/n where normalized != 0.  No envelope division is done:
 * reconstruction is exact on samples covered by two frames exactly when the window satisfies Princen-Bradley,
 * w[m]^2 + w[m + n]^2 = 1 with w[m] = w[2n - 1 - m]; the sine default does.  With center == 0 the first and the last n samples are
 * covered by one frame only and carry uncancelled time-domain aliasing.  The overlap-add is a gather, one lane per output sample:
 * no atomics, deterministic.
 * A NULL handle or pointer, reals not aligned to sizeof(T), any overlap of d_in and d_out or an invalid length give
 * FOURIER_HIP_INVALID_ARGUMENT; batch == 0 is a successful no-op.  Stream-ordered on `stream` like fourier_hip_transform_batch_*.
 * Routes (fourier_hip_mdct_describe_*: "<forward route>, <inverse route>: <the inner plan's describe>"):
 *   "mdct composed"     even n = 2h: a fold sweep (window, fold to n reals, pre-twiddle) into a handle-owned scratch (at most 1 GiB,
 *                       never less than one frame forward and two frames inverse), the h-point complex plan, a post-twiddle sweep
 *                       into the output.
 *   "mdct fused rows"   n = 2h whose h-point plan is one whole-row kernel (n 128 ... 1024, f32 also 2048): fold, transform and
 *                       post-twiddle in ONE launch, no scratch.  Option "fusion" = 0 forces the composed route, 1 takes the fused one
 *                       wherever it exists.
 *   "mdct full-length"  odd n, the correctness path: the 2n-point complex plan on w[m] x[m] exp(-i pi m / 2n).
 * The inverse ("imdct composed" for even n, "imdct full-length" for odd n) is a pre sweep, the inner plan and the overlap-add sweep,
 * in chunks of whole rows, or of ranges of one row's samples where a row's frames exceed the bound; there is no fused inverse.
 * fourier_hip_mdct_reserve_*(h, length, batch) sizes everything forward calls of at most `batch` rows of `length` reals, and inverse
 * calls to that length from frames(length) frames, need: they then never allocate.  Handles are Send, not Sync, like the complex
 * ones; status of the last call: fourier_hip_mdct_last_status_*. */
struct fourier_mdct_float;
struct fourier_mdct_double;

/* NULL on failure (n == 0 included). */
struct fourier_mdct_float *fourier_hip_mdct_create_float(FOURIER_SIZE_TYPE n, int center, int device);
struct fourier_mdct_double *fourier_hip_mdct_create_double(FOURIER_SIZE_TYPE n, int center, int device);
/* NULL is a no-op. */
void fourier_hip_mdct_destroy_float(FOURIER_STRUCT fourier_mdct_float *);
void fourier_hip_mdct_destroy_double(FOURIER_STRUCT fourier_mdct_double *);
/* n; 0 for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_mdct_size_float(const FOURIER_STRUCT fourier_mdct_float *);
FOURIER_SIZE_TYPE fourier_hip_mdct_size_double(const FOURIER_STRUCT fourier_mdct_double *);
/* frames of a row of `length` reals; 0 for an invalid length or a NULL handle */
FOURIER_SIZE_TYPE fourier_hip_mdct_frames_float(const FOURIER_STRUCT fourier_mdct_float *, FOURIER_SIZE_TYPE length);
FOURIER_SIZE_TYPE fourier_hip_mdct_frames_double(const FOURIER_STRUCT fourier_mdct_double *, FOURIER_SIZE_TYPE length);
int fourier_hip_mdct_set_window_float(FOURIER_STRUCT fourier_mdct_float *, const void *d_window, void *stream);
int fourier_hip_mdct_set_window_double(FOURIER_STRUCT fourier_mdct_double *, const void *d_window, void *stream);
int fourier_hip_mdct_forward_float(const FOURIER_STRUCT fourier_mdct_float *, const void *d_in, void *d_out, FOURIER_SIZE_TYPE length,
                                   FOURIER_SIZE_TYPE batch, int normalized, void *stream);
int fourier_hip_mdct_forward_double(const FOURIER_STRUCT fourier_mdct_double *, const void *d_in, void *d_out, FOURIER_SIZE_TYPE length,
                                    FOURIER_SIZE_TYPE batch, int normalized, void *stream);
int fourier_hip_mdct_inverse_float(const FOURIER_STRUCT fourier_mdct_float *, const void *d_in, void *d_out, FOURIER_SIZE_TYPE frames,
                                   FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch, int normalized, void *stream);
int fourier_hip_mdct_inverse_double(const FOURIER_STRUCT fourier_mdct_double *, const void *d_in, void *d_out, FOURIER_SIZE_TYPE frames,
                                    FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch, int normalized, void *stream);
int fourier_hip_mdct_reserve_float(const FOURIER_STRUCT fourier_mdct_float *, FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch);
int fourier_hip_mdct_reserve_double(const FOURIER_STRUCT fourier_mdct_double *, FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch);
/* "fusion": 0 = the composed forward route, 1 = the fused one wherever it exists.  Anything else: FOURIER_HIP_INVALID_ARGUMENT. */
int fourier_hip_mdct_set_option_float(FOURIER_STRUCT fourier_mdct_float *, const char *key, long long value);
int fourier_hip_mdct_set_option_double(FOURIER_STRUCT fourier_mdct_double *, const char *key, long long value);
/* "" for a NULL handle. */
const char *fourier_hip_mdct_describe_float(const FOURIER_STRUCT fourier_mdct_float *);
const char *fourier_hip_mdct_describe_double(const FOURIER_STRUCT fourier_mdct_double *);
int fourier_hip_mdct_last_status_float(const FOURIER_STRUCT fourier_mdct_float *);
int fourier_hip_mdct_last_status_double(const FOURIER_STRUCT fourier_mdct_double *);

/* ---------------- power spectrogram and Welch power spectral density (extension; the reference has none) ----------
 * |X|^p of the short-time Fourier transform's frames, and the mean of |X|^2 over a row's frames, on DEVICE memory, without the complex
 * frames being written anywhere the caller sees.  A handle is made with the STFT handle's parameters (n_fft, hop, win_length, pad mode
 * FOURIER_STFT_PAD_*): the framing, the centring of the window, fourier_hip_spectrogram_frames_* and fourier_hip_spectrogram_set_window_*
 * (win_length reals T on the device, NULL: all ones; a set-up call that waits for `stream`) are exactly those of fourier_hip_stft_*, and
 * X[b, f, k] below is exactly what fourier_hip_stft_forward_* produces for the same arguments.  bins = n_fft / 2 + 1.
 * fourier_hip_spectrogram_forward_*: `batch` contiguous rows of `length` reals in; batch x frames x bins REALS out, FRAME-MAJOR (frame f of
 * row b at element offset (b * frames + f) * bins),
 *   out[b, f, k] = |X[b, f, k]|^power,   power = FOURIER_SPECTROGRAM_MAGNITUDE (1) or FOURIER_SPECTROGRAM_POWER (2),
 * X times n_fft^-1/2 where normalized != 0.  Any other power gives FOURIER_HIP_INVALID_ARGUMENT.
 * fourier_hip_spectrogram_welch_*: the same rows in; batch x bins reals out,
 *   out[b, k] = scale * c_k / frames * sum_f |X[b, f, k]|^2   with the unnormalized X,
 * c_k = 2 where onesided_fold != 0 and bin k has a mirror (0 < k < n_fft / 2, and also k = (n_fft - 1) / 2 for odd n_fft), else 1.
 * Welch's method with the mean over the frames: scipy.signal.welch(detrend = False, average = "mean") with PAD_NONE,
 * hop = nperseg - noverlap, scale = 1 / (fs sum w^2) for a density and 1 / (sum w)^2 for a spectrum.  There is NO detrending: scipy's
 * default removes each segment's mean first, this does not.
 * Determinism: no atomics.  Every sum over frames runs in an order fixed by the route, the shape and the scratch bound, so two calls
 * with equal arguments on one handle give bit-equal results.
 * A NULL handle or pointer, reals not aligned to sizeof(T), any overlap of d_in and d_out or an invalid length give
 * FOURIER_HIP_INVALID_ARGUMENT; batch == 0 is a successful no-op.  Stream-ordered on `stream` like fourier_hip_transform_batch_*.
 * Routes (fourier_hip_spectrogram_describe_*: "spectrogram <route>, welch <route>: <the real plan's describe>"):
 *   "fused rows"  n_fft = 2h whose h-point plan is one whole-row kernel (n_fft 128 ... 1024, f32 also 2048), wherever "stft fused rows"
 *                 exists: gather, window, transform, untangle and |.|^p in ONE launch, no scratch.  Welch: one workgroup per tile of
 *                 frames of one row sums its frames' powers in ascending order into a row of partials in a handle-owned buffer, a
 *                 second sweep sums a row's tiles in ascending order.
 *   "composed"    any n_fft: per chunk of the flat frame index a gather sweep, the real-input plan into a handle-owned scratch (at
 *                 most 1 GiB, never less than one frame), then a sweep that writes |.|^p or adds the chunk's powers to the partials.
 * Option "fusion" = 1 takes the fused routes wherever they exist, 0 the composed ones (the default: the fused kernels have not been
 * measured on the device yet).  The partials stay within
 * the scratch bound too (never less than one row's): more rows are walked in groups.  fourier_hip_spectrogram_reserve_*(h, length, batch)
 * sizes everything both entry points need for at most `batch` rows of `length` reals on the route selected at that time: they then
 * never allocate.  Handles are Send, not Sync, like the complex ones; status of the last call: fourier_hip_spectrogram_last_status_*. */
enum {
  FOURIER_SPECTROGRAM_MAGNITUDE = 1,
  FOURIER_SPECTROGRAM_POWER = 2,
};
struct fourier_spectrogram_float;
struct fourier_spectrogram_double;

/* NULL on failure (parameters outside the STFT handle's ranges included). */
struct fourier_spectrogram_float *fourier_hip_spectrogram_create_float(FOURIER_SIZE_TYPE n_fft, FOURIER_SIZE_TYPE hop,
                                                                       FOURIER_SIZE_TYPE win_length, int pad_mode, int device);
struct fourier_spectrogram_double *fourier_hip_spectrogram_create_double(FOURIER_SIZE_TYPE n_fft, FOURIER_SIZE_TYPE hop,
                                                                         FOURIER_SIZE_TYPE win_length, int pad_mode, int device);
/* NULL is a no-op. */
void fourier_hip_spectrogram_destroy_float(FOURIER_STRUCT fourier_spectrogram_float *);
void fourier_hip_spectrogram_destroy_double(FOURIER_STRUCT fourier_spectrogram_double *);
/* 0 for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_spectrogram_n_fft_float(const FOURIER_STRUCT fourier_spectrogram_float *);
FOURIER_SIZE_TYPE fourier_hip_spectrogram_n_fft_double(const FOURIER_STRUCT fourier_spectrogram_double *);
FOURIER_SIZE_TYPE fourier_hip_spectrogram_hop_float(const FOURIER_STRUCT fourier_spectrogram_float *);
FOURIER_SIZE_TYPE fourier_hip_spectrogram_hop_double(const FOURIER_STRUCT fourier_spectrogram_double *);
FOURIER_SIZE_TYPE fourier_hip_spectrogram_win_length_float(const FOURIER_STRUCT fourier_spectrogram_float *);
FOURIER_SIZE_TYPE fourier_hip_spectrogram_win_length_double(const FOURIER_STRUCT fourier_spectrogram_double *);
FOURIER_SIZE_TYPE fourier_hip_spectrogram_bins_float(const FOURIER_STRUCT fourier_spectrogram_float *);
FOURIER_SIZE_TYPE fourier_hip_spectrogram_bins_double(const FOURIER_STRUCT fourier_spectrogram_double *);
/* frames of a row of `length` reals; 0 for an invalid length or a NULL handle */
FOURIER_SIZE_TYPE fourier_hip_spectrogram_frames_float(const FOURIER_STRUCT fourier_spectrogram_float *, FOURIER_SIZE_TYPE length);
FOURIER_SIZE_TYPE fourier_hip_spectrogram_frames_double(const FOURIER_STRUCT fourier_spectrogram_double *, FOURIER_SIZE_TYPE length);
int fourier_hip_spectrogram_set_window_float(FOURIER_STRUCT fourier_spectrogram_float *, const void *d_window, void *stream);
int fourier_hip_spectrogram_set_window_double(FOURIER_STRUCT fourier_spectrogram_double *, const void *d_window, void *stream);
int fourier_hip_spectrogram_forward_float(const FOURIER_STRUCT fourier_spectrogram_float *, const void *d_in, void *d_out,
                                          FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch, int power, int normalized, void *stream);
int fourier_hip_spectrogram_forward_double(const FOURIER_STRUCT fourier_spectrogram_double *, const void *d_in, void *d_out,
                                           FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch, int power, int normalized, void *stream);
int fourier_hip_spectrogram_welch_float(const FOURIER_STRUCT fourier_spectrogram_float *, const void *d_in, void *d_out,
                                        FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch, int onesided_fold, double scale, void *stream);
int fourier_hip_spectrogram_welch_double(const FOURIER_STRUCT fourier_spectrogram_double *, const void *d_in, void *d_out,
                                         FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch, int onesided_fold, double scale, void *stream);
int fourier_hip_spectrogram_reserve_float(const FOURIER_STRUCT fourier_spectrogram_float *, FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch);
int fourier_hip_spectrogram_reserve_double(const FOURIER_STRUCT fourier_spectrogram_double *, FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch);
/* "fusion": 0 = the composed routes, 1 = the fused ones wherever they exist.  Anything else: FOURIER_HIP_INVALID_ARGUMENT. */
int fourier_hip_spectrogram_set_option_float(FOURIER_STRUCT fourier_spectrogram_float *, const char *key, long long value);
int fourier_hip_spectrogram_set_option_double(FOURIER_STRUCT fourier_spectrogram_double *, const char *key, long long value);
/* "" for a NULL handle. */
const char *fourier_hip_spectrogram_describe_float(const FOURIER_STRUCT fourier_spectrogram_float *);
const char *fourier_hip_spectrogram_describe_double(const FOURIER_STRUCT fourier_spectrogram_double *);
int fourier_hip_spectrogram_last_status_float(const FOURIER_STRUCT fourier_spectrogram_float *);
int fourier_hip_spectrogram_last_status_double(const FOURIER_STRUCT fourier_spectrogram_double *);

/* ---------------- cross-spectral density and coherence (extension; the reference has none) ----------
 * Of two signals x and y on DEVICE memory, the averaged cross spectrum of their short-time Fourier transforms' frames and the
 * magnitude-squared coherence, without a frame being written anywhere the caller sees.  A handle is made with the STFT handle's parameters
 * (n_fft, hop, win_length, pad mode FOURIER_STFT_PAD_*): the framing, the centring of the window, fourier_hip_csd_frames_* and
 * fourier_hip_csd_set_window_* (win_length reals T on the device, NULL: all ones; a set-up call that waits for `stream`) are exactly those
 * of fourier_hip_stft_*, and X[b, f, k] and Y[b, f, k] below are exactly what fourier_hip_stft_forward_* (unnormalized) produces for row b of
 * x and of y.  bins = n_fft / 2 + 1.  d_x and d_y are each `batch` contiguous rows of `length` reals; they may be the same buffer.
 * fourier_hip_csd_csd_*: batch x bins interleaved COMPLEX values out,
 *   out[b, k] = scale * c_k / frames * sum_f conj(X[b, f, k]) * Y[b, f, k],
 * c_k = 2 where onesided_fold != 0 and bin k has a mirror (0 < k < n_fft / 2, and also k = (n_fft - 1) / 2 for odd n_fft), else 1: the fold
 * factor of fourier_hip_spectrogram_welch_*.  scipy.signal.csd(detrend = False, average = "mean") with PAD_NONE, hop = nperseg - noverlap,
 * scale = 1 / (fs sum w^2) for a density and 1 / (sum w)^2 for a spectrum.
 * fourier_hip_csd_coherence_*: batch x bins REALS out,
 *   out[b, k] = |sum_f conj(X) Y|^2 / (sum_f |X|^2 * sum_f |Y|^2)
 * (scale and fold cancel): scipy.signal.coherence(detrend = False).  Computed quotients first, with S = sum_f conj(X) Y, Pxx and Pyy as
 * (Re S / Pxx) (Re S / Pyy) + (Im S / Pxx) (Im S / Pyy) in plain IEEE divisions, so that neither |S|^2 nor Pxx Pyy is formed: the result is
 * finite and scale-invariant wherever the sums themselves are finite ("Amplitude" above).  A bin whose denominator is 0 gives what the
 * divisions give.  There is NO detrending: scipy's default removes each segment's mean first, this does not.
 * Determinism: no atomics.  Every sum over frames runs in an order fixed by the route, the shape and the scratch bound -- ascending
 * frames inside a tile, then ascending tiles -- so two calls with equal arguments on one handle give bit-equal results.
 * A NULL handle or pointer, reals not aligned to sizeof(T), a cross spectrum not aligned to 2 sizeof(T), any overlap of d_out with d_x or
 * d_y, or an invalid length give FOURIER_HIP_INVALID_ARGUMENT; batch == 0 is a successful no-op.  Stream-ordered on `stream` like
 * fourier_hip_transform_batch_*.
 * Routes (fourier_hip_csd_describe_*: "csd <route>, coherence <route>: <the real plan's describe>"):
 *   "fused rows"  n_fft = 2h whose h-point plan is one whole-row kernel (n_fft 128 ... 1024, f32 also 2048), wherever "stft fused rows"
 *                 exists: gather, window, transform and untangle of the frames of BOTH signals and their products in ONE launch.  One
 *                 workgroup per tile of frame pairs of one row sums |X|^2, |Y|^2 and conj(X) Y in ascending frame order into four rows
 *                 of partials in a handle-owned buffer; a second sweep sums a row's tiles in ascending order and writes the result.
 *   "composed"    any n_fft: per chunk of the flat frame index a gather sweep per signal and one run of the real-input plan over both
 *                 into a handle-owned scratch (2 x (n_fft reals + bins complex) per frame pair, at most 1 GiB, never less than one pair),
 *                 then a sweep that adds the chunk's products to the partials, and the same final sweep.
 * Option "fusion" = 1 takes the fused route wherever it exists, 0 the composed one (the default: DESIGN.md section 4, "Cross-spectral
 * density and coherence", has the measurement the default follows).  The partials stay within the scratch bound too (never less than one
 * row's): more rows are walked in groups.  fourier_hip_csd_reserve_*(h, length, batch) sizes everything both entry points need for at
 * most `batch` rows of `length` reals on the route selected at that time: they then never allocate.  Handles are Send, not Sync, like
 * the complex ones; status of the last call: fourier_hip_csd_last_status_*. */
struct fourier_csd_float;
struct fourier_csd_double;

/* NULL on failure (parameters outside the STFT handle's ranges included). */
struct fourier_csd_float *fourier_hip_csd_create_float(FOURIER_SIZE_TYPE n_fft, FOURIER_SIZE_TYPE hop, FOURIER_SIZE_TYPE win_length,
                                                       int pad_mode, int device);
struct fourier_csd_double *fourier_hip_csd_create_double(FOURIER_SIZE_TYPE n_fft, FOURIER_SIZE_TYPE hop, FOURIER_SIZE_TYPE win_length,
                                                         int pad_mode, int device);
/* NULL is a no-op. */
void fourier_hip_csd_destroy_float(FOURIER_STRUCT fourier_csd_float *);
void fourier_hip_csd_destroy_double(FOURIER_STRUCT fourier_csd_double *);
/* 0 for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_csd_n_fft_float(const FOURIER_STRUCT fourier_csd_float *);
FOURIER_SIZE_TYPE fourier_hip_csd_n_fft_double(const FOURIER_STRUCT fourier_csd_double *);
FOURIER_SIZE_TYPE fourier_hip_csd_hop_float(const FOURIER_STRUCT fourier_csd_float *);
FOURIER_SIZE_TYPE fourier_hip_csd_hop_double(const FOURIER_STRUCT fourier_csd_double *);
FOURIER_SIZE_TYPE fourier_hip_csd_win_length_float(const FOURIER_STRUCT fourier_csd_float *);
FOURIER_SIZE_TYPE fourier_hip_csd_win_length_double(const FOURIER_STRUCT fourier_csd_double *);
FOURIER_SIZE_TYPE fourier_hip_csd_bins_float(const FOURIER_STRUCT fourier_csd_float *);
FOURIER_SIZE_TYPE fourier_hip_csd_bins_double(const FOURIER_STRUCT fourier_csd_double *);
/* frames of a row of `length` reals; 0 for an invalid length or a NULL handle */
FOURIER_SIZE_TYPE fourier_hip_csd_frames_float(const FOURIER_STRUCT fourier_csd_float *, FOURIER_SIZE_TYPE length);
FOURIER_SIZE_TYPE fourier_hip_csd_frames_double(const FOURIER_STRUCT fourier_csd_double *, FOURIER_SIZE_TYPE length);
int fourier_hip_csd_set_window_float(FOURIER_STRUCT fourier_csd_float *, const void *d_window, void *stream);
int fourier_hip_csd_set_window_double(FOURIER_STRUCT fourier_csd_double *, const void *d_window, void *stream);
int fourier_hip_csd_csd_float(const FOURIER_STRUCT fourier_csd_float *, const void *d_x, const void *d_y, void *d_out,
                              FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch, int onesided_fold, double scale, void *stream);
int fourier_hip_csd_csd_double(const FOURIER_STRUCT fourier_csd_double *, const void *d_x, const void *d_y, void *d_out,
                               FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch, int onesided_fold, double scale, void *stream);
int fourier_hip_csd_coherence_float(const FOURIER_STRUCT fourier_csd_float *, const void *d_x, const void *d_y, void *d_out,
                                    FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch, void *stream);
int fourier_hip_csd_coherence_double(const FOURIER_STRUCT fourier_csd_double *, const void *d_x, const void *d_y, void *d_out,
                                     FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch, void *stream);
int fourier_hip_csd_reserve_float(const FOURIER_STRUCT fourier_csd_float *, FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch);
int fourier_hip_csd_reserve_double(const FOURIER_STRUCT fourier_csd_double *, FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch);
/* "fusion": 0 = the composed route, 1 = the fused one wherever it exists.  Anything else: FOURIER_HIP_INVALID_ARGUMENT. */
int fourier_hip_csd_set_option_float(FOURIER_STRUCT fourier_csd_float *, const char *key, long long value);
int fourier_hip_csd_set_option_double(FOURIER_STRUCT fourier_csd_double *, const char *key, long long value);
/* "" for a NULL handle. */
const char *fourier_hip_csd_describe_float(const FOURIER_STRUCT fourier_csd_float *);
const char *fourier_hip_csd_describe_double(const FOURIER_STRUCT fourier_csd_double *);
int fourier_hip_csd_last_status_float(const FOURIER_STRUCT fourier_csd_float *);
int fourier_hip_csd_last_status_double(const FOURIER_STRUCT fourier_csd_double *);

/* ---------------- band-energy (mel) spectrogram (extension; the reference has none) ----------
 * Of `batch` rows of `length` reals T on DEVICE memory, the energies of every STFT frame in `bands` bands: with X[b, f, k] exactly what
 * fourier_hip_stft_forward_* produces (framing, window, padding and `normalized` as fourier_hip_spectrogram_*), S = |X|^p, p = 1
 * (FOURIER_SPECTROGRAM_MAGNITUDE) or 2 (FOURIER_SPECTROGRAM_POWER), and a real matrix W of bands x bins,
 *   Y[b, f, j] = sum_k W[j, k] * S[b, f, k],   and with log_mult != 0   Y <- log_mult * ln(max(Y, log_floor)),
 * frame-major batch x frames x bands REALS out; S never reaches memory the caller sees.  bins = n_fft / 2 + 1, 1 <= bands <= 65535.
 * torchaudio's MelSpectrogram is W = melscale_fbanks(...)^T; any sparse-row matrix works, negative weights included.
 * The sum over k runs in ascending k over the row's support [lo_j, hi_j) -- first non-zero column to last non-zero column + 1, zeros
 * inside kept -- in ONE accumulator of type T; an all-zero row gives 0 (log_mult * ln(log_floor) under the log).  The logarithm is the
 * library's logf / log.  log_mult == 0 means linear and log_floor is ignored; otherwise log_floor must be finite and > 0 (in T too).
 * fourier_hip_bandspec_set_bands_*: h_matrix points to bands x bins reals T, row-major, on the HOST.  A set-up call like
 * fourier_hip_bandspec_set_window_*: the supports are found and packed, uploaded, and the call waits for `stream`.  A NaN or infinite
 * weight gives FOURIER_HIP_INVALID_ARGUMENT and keeps the bank that was there.  A later call replaces the bank; forward before any
 * set_bands gives FOURIER_HIP_INVALID_ARGUMENT.
 * Determinism: no atomics, and no sum crosses a frame: two calls with equal arguments give bit-equal results on a route, whatever the
 * scratch bound.
 * A NULL handle or pointer, reals not aligned to sizeof(T), any overlap of d_out with d_in, an invalid length or power give
 * FOURIER_HIP_INVALID_ARGUMENT; batch == 0 is a successful no-op.  Stream-ordered on `stream` like fourier_hip_transform_batch_*.
 * Routes (fourier_hip_bandspec_describe_*: "bandspec <route>: <the real plan's describe>"):
 *   "fused rows"  n_fft = 2h whose h-point plan is one whole-row kernel (n_fft 128 ... 1024, f32 also 2048) and bands <= bins: gather,
 *                 window, transform, untangle, |.|^p, the band sums and the log in ONE launch; the |X|^p of a tile of frames live in
 *                 LDS only.  No scratch.
 *   "composed"    any n_fft and any bands: per chunk of the flat frame index the spectrogram's gather sweep and the real-input plan
 *                 into a handle-owned scratch (n_fft reals + bins complex per frame, at most 1 GiB, never less than one frame), then a
 *                 sweep with one lane per (frame, band).
 * Option "fusion" = 1 takes the fused route wherever it exists (the default: it measured 0.18 - 0.20 of the composed route's time,
 * DESIGN.md section 4, "Band-energy (mel) spectrogram"), 0 the composed one.  fourier_hip_bandspec_reserve_*(h, length, batch) sizes what forward needs
 * for at most `batch` rows of `length` reals on the route selected at that time: it then never allocates (the bank's buffers belong
 * to set_bands).  Handles are Send, not Sync, like the complex ones; status of the last call: fourier_hip_bandspec_last_status_*. */
struct fourier_bandspec_float;
struct fourier_bandspec_double;

/* NULL on failure (parameters outside the STFT handle's ranges, bands == 0 or bands > 65535 included). */
struct fourier_bandspec_float *fourier_hip_bandspec_create_float(FOURIER_SIZE_TYPE n_fft, FOURIER_SIZE_TYPE hop, FOURIER_SIZE_TYPE win_length,
                                                                 int pad_mode, FOURIER_SIZE_TYPE bands, int device);
struct fourier_bandspec_double *fourier_hip_bandspec_create_double(FOURIER_SIZE_TYPE n_fft, FOURIER_SIZE_TYPE hop, FOURIER_SIZE_TYPE win_length,
                                                                   int pad_mode, FOURIER_SIZE_TYPE bands, int device);
/* NULL is a no-op. */
void fourier_hip_bandspec_destroy_float(FOURIER_STRUCT fourier_bandspec_float *);
void fourier_hip_bandspec_destroy_double(FOURIER_STRUCT fourier_bandspec_double *);
/* 0 for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_bandspec_n_fft_float(const FOURIER_STRUCT fourier_bandspec_float *);
FOURIER_SIZE_TYPE fourier_hip_bandspec_n_fft_double(const FOURIER_STRUCT fourier_bandspec_double *);
FOURIER_SIZE_TYPE fourier_hip_bandspec_hop_float(const FOURIER_STRUCT fourier_bandspec_float *);
FOURIER_SIZE_TYPE fourier_hip_bandspec_hop_double(const FOURIER_STRUCT fourier_bandspec_double *);
FOURIER_SIZE_TYPE fourier_hip_bandspec_win_length_float(const FOURIER_STRUCT fourier_bandspec_float *);
FOURIER_SIZE_TYPE fourier_hip_bandspec_win_length_double(const FOURIER_STRUCT fourier_bandspec_double *);
FOURIER_SIZE_TYPE fourier_hip_bandspec_bins_float(const FOURIER_STRUCT fourier_bandspec_float *);
FOURIER_SIZE_TYPE fourier_hip_bandspec_bins_double(const FOURIER_STRUCT fourier_bandspec_double *);
FOURIER_SIZE_TYPE fourier_hip_bandspec_bands_float(const FOURIER_STRUCT fourier_bandspec_float *);
FOURIER_SIZE_TYPE fourier_hip_bandspec_bands_double(const FOURIER_STRUCT fourier_bandspec_double *);
/* frames of a row of `length` reals; 0 for an invalid length or a NULL handle */
FOURIER_SIZE_TYPE fourier_hip_bandspec_frames_float(const FOURIER_STRUCT fourier_bandspec_float *, FOURIER_SIZE_TYPE length);
FOURIER_SIZE_TYPE fourier_hip_bandspec_frames_double(const FOURIER_STRUCT fourier_bandspec_double *, FOURIER_SIZE_TYPE length);
int fourier_hip_bandspec_set_window_float(FOURIER_STRUCT fourier_bandspec_float *, const void *d_window, void *stream);
int fourier_hip_bandspec_set_window_double(FOURIER_STRUCT fourier_bandspec_double *, const void *d_window, void *stream);
/* h_matrix: bands x bins reals on the HOST */
int fourier_hip_bandspec_set_bands_float(FOURIER_STRUCT fourier_bandspec_float *, const void *h_matrix, void *stream);
int fourier_hip_bandspec_set_bands_double(FOURIER_STRUCT fourier_bandspec_double *, const void *h_matrix, void *stream);
int fourier_hip_bandspec_forward_float(const FOURIER_STRUCT fourier_bandspec_float *, const void *d_in, void *d_out, FOURIER_SIZE_TYPE length,
                                       FOURIER_SIZE_TYPE batch, int power, int normalized, double log_mult, double log_floor, void *stream);
int fourier_hip_bandspec_forward_double(const FOURIER_STRUCT fourier_bandspec_double *, const void *d_in, void *d_out, FOURIER_SIZE_TYPE length,
                                        FOURIER_SIZE_TYPE batch, int power, int normalized, double log_mult, double log_floor, void *stream);
int fourier_hip_bandspec_reserve_float(const FOURIER_STRUCT fourier_bandspec_float *, FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch);
int fourier_hip_bandspec_reserve_double(const FOURIER_STRUCT fourier_bandspec_double *, FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch);
/* "fusion": 0 = the composed route, 1 = the fused one wherever it exists.  Anything else: FOURIER_HIP_INVALID_ARGUMENT. */
int fourier_hip_bandspec_set_option_float(FOURIER_STRUCT fourier_bandspec_float *, const char *key, long long value);
int fourier_hip_bandspec_set_option_double(FOURIER_STRUCT fourier_bandspec_double *, const char *key, long long value);
/* "" for a NULL handle. */
const char *fourier_hip_bandspec_describe_float(const FOURIER_STRUCT fourier_bandspec_float *);
const char *fourier_hip_bandspec_describe_double(const FOURIER_STRUCT fourier_bandspec_double *);
int fourier_hip_bandspec_last_status_float(const FOURIER_STRUCT fourier_bandspec_float *);
int fourier_hip_bandspec_last_status_double(const FOURIER_STRUCT fourier_bandspec_double *);

/* ---------------- analytic signal and envelope of real rows (extension; the reference has none) ----------
 * Of `batch` rows of N >= 1 reals T on DEVICE memory, row b at element offset b*N, with X = fft(x) and
 *   m[k] = 1 for k = 0 and (N even) k = N/2,  2 for 0 < k < N/2 (odd N: k <= (N-1)/2),  0 above,
 * fourier_hip_hilbert_analytic_*: z = ifft(X (.) m), `batch` rows of N interleaved COMPLEX values out, Re z = x: scipy.signal.hilbert
 * along the last axis;
 * fourier_hip_hilbert_envelope_*: |z|, `batch` rows of N REALS out.  This is abs(scipy.signal.hilbert(x)); it is NOT
 * scipy.signal.envelope.
 * A NULL pointer, an input not aligned to sizeof(T), an analytic output not aligned to one complex value (2*sizeof(T)), an envelope
 * output not aligned to sizeof(T) give FOURIER_HIP_INVALID_ARGUMENT.  analytic: ANY overlap of input and output is
 * FOURIER_HIP_INVALID_ARGUMENT (the output is twice the input's size: rows do not line up).  envelope: d_out == d_in is in place and
 * allowed, any other overlap is not.  batch == 0 is a successful no-op.  A row above 2^31 - 1 bytes of complex values cannot be
 * carried by one launch: create fails (as fourier_hip_conv_create_*).  Stream-ordered on `stream` like fourier_hip_transform_batch_*.
 * Routes (fourier_hip_hilbert_describe_* begins with the route's name):
 *   "hilbert one-launch"  N = 2^11 ... 2^15 (double: ... 2^14): load, FFT, multiplier computed from the bin index, inverse FFT, store
 *                         z or |z| in ONE launch on register-resident data; no scratch.
 *   "hilbert composed"    every N: real forward transform -> half spectrum (N/2 + 1 values a row) in the plan's scratch, one sweep that
 *                         writes X[k] m[k] / N, zeros above, into the caller's output, the unscaled inverse in place there.  The
 *                         envelope runs the sweep and the inverse in a second scratch array of N complex values a row, and a second
 *                         sweep writes |z|.
 * Option "fusion" (fourier_hip_hilbert_set_option_*): 1 = the one-launch route where the length has one, 0 = the composed route, the
 * DEFAULT (the two routes have not been measured against each other).  The plan owns a scratch of at most 1 GiB (never less than one
 * row) and walks larger batches in chunks of it; the first call with a batch larger than any before allocates it unless
 * fourier_hip_hilbert_reserve_* was called for at least that batch (one size covers both entry points).  A NULL handle gives
 * FOURIER_HIP_INVALID_ARGUMENT, 0 from fourier_hip_hilbert_size_* and "" from fourier_hip_hilbert_describe_*.  Handles are Send, not
 * Sync, like the complex ones; status of the last call: fourier_hip_hilbert_last_status_*. */
struct fourier_hilbert_float;
struct fourier_hilbert_double;

/* NULL on failure (size 0 included). */
struct fourier_hilbert_float *fourier_hip_hilbert_create_float(FOURIER_SIZE_TYPE size, int device);
struct fourier_hilbert_double *fourier_hip_hilbert_create_double(FOURIER_SIZE_TYPE size, int device);
/* NULL is a no-op. */
void fourier_hip_hilbert_destroy_float(FOURIER_STRUCT fourier_hilbert_float *);
void fourier_hip_hilbert_destroy_double(FOURIER_STRUCT fourier_hilbert_double *);
/* 0 for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_hilbert_size_float(const FOURIER_STRUCT fourier_hilbert_float *);
FOURIER_SIZE_TYPE fourier_hip_hilbert_size_double(const FOURIER_STRUCT fourier_hilbert_double *);
int fourier_hip_hilbert_analytic_float(const FOURIER_STRUCT fourier_hilbert_float *, const void *d_in, void *d_out,
                                       FOURIER_SIZE_TYPE batch, void *stream);
int fourier_hip_hilbert_analytic_double(const FOURIER_STRUCT fourier_hilbert_double *, const void *d_in, void *d_out,
                                        FOURIER_SIZE_TYPE batch, void *stream);
int fourier_hip_hilbert_envelope_float(const FOURIER_STRUCT fourier_hilbert_float *, const void *d_in, void *d_out,
                                       FOURIER_SIZE_TYPE batch, void *stream);
int fourier_hip_hilbert_envelope_double(const FOURIER_STRUCT fourier_hilbert_double *, const void *d_in, void *d_out,
                                        FOURIER_SIZE_TYPE batch, void *stream);
int fourier_hip_hilbert_reserve_float(const FOURIER_STRUCT fourier_hilbert_float *, FOURIER_SIZE_TYPE batch);
int fourier_hip_hilbert_reserve_double(const FOURIER_STRUCT fourier_hilbert_double *, FOURIER_SIZE_TYPE batch);
/* "fusion": 0 = the composed route, 1 = the one-launch route where it exists.  Anything else: FOURIER_HIP_INVALID_ARGUMENT. */
int fourier_hip_hilbert_set_option_float(FOURIER_STRUCT fourier_hilbert_float *, const char *key, long long value);
int fourier_hip_hilbert_set_option_double(FOURIER_STRUCT fourier_hilbert_double *, const char *key, long long value);
/* "" for a NULL handle. */
const char *fourier_hip_hilbert_describe_float(const FOURIER_STRUCT fourier_hilbert_float *);
const char *fourier_hip_hilbert_describe_double(const FOURIER_STRUCT fourier_hilbert_double *);
int fourier_hip_hilbert_last_status_float(const FOURIER_STRUCT fourier_hilbert_float *);
int fourier_hip_hilbert_last_status_double(const FOURIER_STRUCT fourier_hilbert_double *);

/* ---------------- chirp-z transform and zoom FFT (extension; the reference has only the DFT special case) ----------
 * Of `batch` rows of n >= 1 values on DEVICE memory, row b at element offset b*n -- interleaved COMPLEX values, or REALS T where the
 * handle was created with real_input = 1 --, with w = w_abs exp(2 pi i w_turns) and a = a_abs exp(2 pi i a_turns):
 *   X[b][k] = sum_{j=0}^{n-1} x[b][j] a^(-j) w^(j k),   k = 0 .. m-1,
 * `batch` rows of m interleaved complex values out, row b at element offset b*m: scipy.signal.czt(x, m, w, a) along the last axis.
 * The four parameters are doubles in polar form, the angles in TURNS, fixed at create: a zoom FFT of m points from f1 to f2 at sample
 * rate fs passes w_turns = -(f2 - f1) / (fs m), a_turns = f1 / fs, w_abs = a_abs = 1; the DFT of n points is m = n, w_turns = -1/n.
 * Algorithm: Bluestein's identity j k = (j^2 + k^2 - (k - j)^2) / 2, a circular convolution of L >= n + m - 1 points, L a power of
 * two.  Host tables, evaluated in double and cast to T, every phase reduced to one turn first, every magnitude as exp(log(.) * .):
 *   c(q) = w_abs^(q/2) exp(2 pi i frac(w_turns q / 2));  A[j] = a_abs^-j exp(-2 pi i frac(a_turns j)) c(j^2), j < n;  B[k] = c(k^2), k < m;
 *   v[i] = 1 / c(i^2), i = -(n-1) .. m-1, stored at i mod L;  H = FFT_L(v) / L;   X = B (.) ifft_L(fft_L(x (.) A, zero-padded) (.) H)[0..m).
 * create gives NULL for n == 0, m == 0, a parameter that is not finite, w_abs <= 0 or a_abs <= 0 (invalid), for n + m - 1 > 2^26, and
 * for a spiral so tight that an entry of A, B or H is not finite or is zero after the cast to T (unsupported).  On a spiral the error
 * of the result grows with R, the largest over the smallest magnitude among A and B; R = 1 on the unit circle.
 * A NULL pointer, an input not aligned to one input value (complex rows: 2*sizeof(T), real rows: sizeof(T)), an output not aligned
 * to 2*sizeof(T), or ANY overlap of input and output give FOURIER_HIP_INVALID_ARGUMENT.  batch == 0 is a successful no-op.
 * Stream-ordered on `stream` like fourier_hip_transform_batch_*.
 * Routes (fourier_hip_czt_describe_* begins with the route's name):
 *   "czt one-launch"  L = max(2048, next_pow2(n + m - 1)) <= 2^15 (double: 2^14): load n, (.) A, FFT, (.) H, inverse FFT, (.) B, store m
 *                     in ONE launch on register-resident data; no scratch.
 *   "czt composed"    every n, m, L = next_pow2(n + m - 1): one sweep x (.) A -> rows of L in the plan's scratch, the convolution with H
 *                     in place there (the convolution handle's one-launch or fused-pass route where the L-point plan has one, else
 *                     forward transform, product, inverse), one sweep (.) B -> the first m of each row into the caller's output.
 * Option "fusion" (fourier_hip_czt_set_option_*): 1 = the one-launch route where the lengths have one, 0 = the composed route.  The
 * DEFAULT is 1 where next_pow2(n + m - 1) >= 2048, so that both routes run the same L (there the one-launch route was measured at about
 * half the composed route's time), and 0 below, where the composed route convolves fewer points and nothing is measured.  The plan owns a scratch of at most 1 GiB (never less than one
 * row) and walks larger batches in chunks of it; the first call with a batch larger than any before allocates it unless
 * fourier_hip_czt_reserve_* was called for at least that batch.  A NULL handle gives FOURIER_HIP_INVALID_ARGUMENT, 0 from
 * fourier_hip_czt_size_* / _points_* and "" from fourier_hip_czt_describe_*.  Handles are Send, not Sync, like the complex ones;
 * status of the last call: fourier_hip_czt_last_status_*. */
struct fourier_czt_float;
struct fourier_czt_double;

/* NULL on failure. */
struct fourier_czt_float *fourier_hip_czt_create_float(FOURIER_SIZE_TYPE n, FOURIER_SIZE_TYPE m, double w_abs, double w_turns,
                                                       double a_abs, double a_turns, int real_input, int device);
struct fourier_czt_double *fourier_hip_czt_create_double(FOURIER_SIZE_TYPE n, FOURIER_SIZE_TYPE m, double w_abs, double w_turns,
                                                         double a_abs, double a_turns, int real_input, int device);
/* NULL is a no-op. */
void fourier_hip_czt_destroy_float(FOURIER_STRUCT fourier_czt_float *);
void fourier_hip_czt_destroy_double(FOURIER_STRUCT fourier_czt_double *);
/* n, the values of an input row; 0 for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_czt_size_float(const FOURIER_STRUCT fourier_czt_float *);
FOURIER_SIZE_TYPE fourier_hip_czt_size_double(const FOURIER_STRUCT fourier_czt_double *);
/* m, the values of an output row; 0 for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_czt_points_float(const FOURIER_STRUCT fourier_czt_float *);
FOURIER_SIZE_TYPE fourier_hip_czt_points_double(const FOURIER_STRUCT fourier_czt_double *);
int fourier_hip_czt_transform_float(const FOURIER_STRUCT fourier_czt_float *, const void *d_in, void *d_out,
                                    FOURIER_SIZE_TYPE batch, void *stream);
int fourier_hip_czt_transform_double(const FOURIER_STRUCT fourier_czt_double *, const void *d_in, void *d_out,
                                     FOURIER_SIZE_TYPE batch, void *stream);
int fourier_hip_czt_reserve_float(const FOURIER_STRUCT fourier_czt_float *, FOURIER_SIZE_TYPE batch);
int fourier_hip_czt_reserve_double(const FOURIER_STRUCT fourier_czt_double *, FOURIER_SIZE_TYPE batch);
/* "fusion": 0 = the composed route, 1 = the one-launch route where it exists.  Anything else: FOURIER_HIP_INVALID_ARGUMENT. */
int fourier_hip_czt_set_option_float(FOURIER_STRUCT fourier_czt_float *, const char *key, long long value);
int fourier_hip_czt_set_option_double(FOURIER_STRUCT fourier_czt_double *, const char *key, long long value);
/* "" for a NULL handle. */
const char *fourier_hip_czt_describe_float(const FOURIER_STRUCT fourier_czt_float *);
const char *fourier_hip_czt_describe_double(const FOURIER_STRUCT fourier_czt_double *);
int fourier_hip_czt_last_status_float(const FOURIER_STRUCT fourier_czt_float *);
int fourier_hip_czt_last_status_double(const FOURIER_STRUCT fourier_czt_double *);

/* ---------------- polyphase filter bank channelizer (extension; the reference has none) ----------
 * The weighted-overlap-add analysis bank on DEVICE memory: P = channels >= 1, T = taps >= 1, D = hop >= 1 (D = P critically sampled,
 * D < P oversampled, D > P leaves gaps) and a prototype filter h of P * T reals of the handle's precision.  Of `batch` contiguous rows of
 * `length` values -- interleaved COMPLEX values, or REALS where the handle was created with real_input = 1 --
 *   frames(length) = 1 + (length - P T) / D   for length >= P T, else 0 (an invalid length; fourier_hip_pfb_frames_*),
 *   u[b, f, n] = sum_{t < T} h[t P + n] x[b, f D + t P + n],   n < P,   the taps summed in the order t = 0, 1, ...,
 *   X[b, f, k] = sum_{n < P} u[b, f, n] exp(-2 pi i k n / P),
 * batch x frames x bins interleaved complex values out, FRAME-MAJOR like every frame handle: frame f of row b at complex offset
 * (b * frames + f) * bins; bins = P for complex rows, P / 2 + 1 (onesided) for real rows.  There is no padding.  There is NO per-frame
 * phase rotation for D != P: a frame's time origin is its first sample, as in the STFT handle; a caller who wants the bins referred to
 * the row's origin multiplies bin k of frame f by exp(-2 pi i k f D / P).  There is no `normalized` flag: the prototype filter carries
 * the gain.  The synthesis bank that takes these frames back to rows is the fourier_hip_ipfb_* family below.
 * Filter: fourier_hip_pfb_set_filter_* takes P * T reals T on the device; NULL restores the default of all ones.  A set-up call: it
 * waits for `stream`.
 * create gives NULL for channels, taps or hop of 0 or a real_input flag outside {0, 1} (invalid), and for P * T or D above 2^31 - 1
 * (unsupported).  Frames per row stay below 2^31.
 * A NULL handle or pointer, reals not aligned to sizeof(T) or complex values -- a complex input included -- not aligned to 2 * sizeof(T),
 * any overlap of d_in and d_out or an invalid length give FOURIER_HIP_INVALID_ARGUMENT; batch == 0 is a successful no-op.
 * Stream-ordered on `stream` like fourier_hip_transform_batch_*.  Routes (fourier_hip_pfb_describe_*: "<route>: <the inner plan's describe>"):
 *   "pfb composed"    every P: a fold sweep writes u of a chunk of frames into a handle-owned scratch (at most 1 GiB, never less than one
 *                     frame), the inner plan -- the complex plan of P points, or the real-input plan of P points -- transforms them
 *                     into the output.
 *   "pfb fused rows"  the inner transform is one whole-row kernel (complex rows: P 64 ... 512, f32 also 1024; real rows: P 128 ... 1024,
 *                     f32 also 2048): fold, transform and (real rows) untangle in ONE launch, no scratch.  Option "fusion" = 0 forces
 *                     the composed route, 1 takes the fused one wherever it exists.  The DEFAULT is 1: the fused route was measured
 *                     at 0.46 - 0.88 of the composed route's time at every shape tried.
 * fourier_hip_pfb_reserve_*(h, length, batch) sizes everything forward calls of at most `batch` rows of `length` values need: they then
 * never allocate.  NULL-handle calls return 0 from the getters, "" from describe and FOURIER_HIP_INVALID_ARGUMENT from the rest.
 * Handles are Send, not Sync, like the complex ones; status of the last call: fourier_hip_pfb_last_status_*. */
struct fourier_pfb_float;
struct fourier_pfb_double;

/* NULL on failure (parameters outside the ranges above included). */
struct fourier_pfb_float *fourier_hip_pfb_create_float(FOURIER_SIZE_TYPE channels, FOURIER_SIZE_TYPE taps, FOURIER_SIZE_TYPE hop,
                                                       int real_input, int device);
struct fourier_pfb_double *fourier_hip_pfb_create_double(FOURIER_SIZE_TYPE channels, FOURIER_SIZE_TYPE taps, FOURIER_SIZE_TYPE hop,
                                                         int real_input, int device);
/* NULL is a no-op. */
void fourier_hip_pfb_destroy_float(FOURIER_STRUCT fourier_pfb_float *);
void fourier_hip_pfb_destroy_double(FOURIER_STRUCT fourier_pfb_double *);
/* 0 for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_pfb_channels_float(const FOURIER_STRUCT fourier_pfb_float *);
FOURIER_SIZE_TYPE fourier_hip_pfb_channels_double(const FOURIER_STRUCT fourier_pfb_double *);
FOURIER_SIZE_TYPE fourier_hip_pfb_taps_float(const FOURIER_STRUCT fourier_pfb_float *);
FOURIER_SIZE_TYPE fourier_hip_pfb_taps_double(const FOURIER_STRUCT fourier_pfb_double *);
FOURIER_SIZE_TYPE fourier_hip_pfb_hop_float(const FOURIER_STRUCT fourier_pfb_float *);
FOURIER_SIZE_TYPE fourier_hip_pfb_hop_double(const FOURIER_STRUCT fourier_pfb_double *);
FOURIER_SIZE_TYPE fourier_hip_pfb_bins_float(const FOURIER_STRUCT fourier_pfb_float *);
FOURIER_SIZE_TYPE fourier_hip_pfb_bins_double(const FOURIER_STRUCT fourier_pfb_double *);
/* frames of a row of `length` values; 0 for an invalid length or a NULL handle */
FOURIER_SIZE_TYPE fourier_hip_pfb_frames_float(const FOURIER_STRUCT fourier_pfb_float *, FOURIER_SIZE_TYPE length);
FOURIER_SIZE_TYPE fourier_hip_pfb_frames_double(const FOURIER_STRUCT fourier_pfb_double *, FOURIER_SIZE_TYPE length);
int fourier_hip_pfb_set_filter_float(FOURIER_STRUCT fourier_pfb_float *, const void *d_filter, void *stream);
int fourier_hip_pfb_set_filter_double(FOURIER_STRUCT fourier_pfb_double *, const void *d_filter, void *stream);
int fourier_hip_pfb_forward_float(const FOURIER_STRUCT fourier_pfb_float *, const void *d_in, void *d_out, FOURIER_SIZE_TYPE length,
                                  FOURIER_SIZE_TYPE batch, void *stream);
int fourier_hip_pfb_forward_double(const FOURIER_STRUCT fourier_pfb_double *, const void *d_in, void *d_out, FOURIER_SIZE_TYPE length,
                                   FOURIER_SIZE_TYPE batch, void *stream);
int fourier_hip_pfb_reserve_float(const FOURIER_STRUCT fourier_pfb_float *, FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch);
int fourier_hip_pfb_reserve_double(const FOURIER_STRUCT fourier_pfb_double *, FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch);
/* "fusion": 0 = the composed route, 1 = the fused one wherever it exists.  Anything else: FOURIER_HIP_INVALID_ARGUMENT. */
int fourier_hip_pfb_set_option_float(FOURIER_STRUCT fourier_pfb_float *, const char *key, long long value);
int fourier_hip_pfb_set_option_double(FOURIER_STRUCT fourier_pfb_double *, const char *key, long long value);
/* "" for a NULL handle. */
const char *fourier_hip_pfb_describe_float(const FOURIER_STRUCT fourier_pfb_float *);
const char *fourier_hip_pfb_describe_double(const FOURIER_STRUCT fourier_pfb_double *);
int fourier_hip_pfb_last_status_float(const FOURIER_STRUCT fourier_pfb_float *);
int fourier_hip_pfb_last_status_double(const FOURIER_STRUCT fourier_pfb_double *);

/* ---------------- polyphase synthesis filter bank (extension; the reference has none) ----------
 * The weighted-overlap-add synthesis bank on DEVICE memory, the mirror of the channelizer above with its parameterisation: P = channels,
 * T = taps, D = hop and a synthesis filter g of P * T reals of the handle's precision.  Of batch x frames x bins interleaved complex
 * values, FRAME-MAJOR, exactly what fourier_hip_pfb_forward_* writes (bins = P for complex output rows, P / 2 + 1 for REAL output rows,
 * real_output = 1),
 *   full(frames)  = (frames - 1) D + P T                                       (fourier_hip_ipfb_length_*),
 *   v[b, f, n]    = (1/P) sum_k Y[b, f, k] exp(+2 pi i k n / P),  n < P        (real rows: numpy's irfft(Y, n = P): the imaginary parts
 *                                                                               of bin 0 and, for even P, of bin P / 2 are ignored),
 *   y[b, t]       = sum over the frames f with 0 <= t - f D < P T, in ASCENDING f, of  g[t - f D] * v[b, f, (t - f D) mod P],  t < length,
 * `batch` contiguous rows of `length` values out, 1 <= length <= full(frames).  The sum starts from its first term; a sample that no
 * frame covers (D > P T) is written as 0.  No atomics: repeated calls give the same bits.  There is no envelope division and no NOLA
 * check, and no per-frame phase rotation (the mirror of the analysis convention): reconstruction is a property of the pair (h, g).
 * For frames made by the analysis handle with filter h, in the interior where every covering frame exists,
 *   y[t] = sum_{|s| < T} c_s(t mod D) x[t + s P],     c_s(r) = sum_j g[r + j D] h[r + j D + s P]   (both indices inside [0, P T)),
 * so the pair reconstructs perfectly with zero delay iff c_0 == 1 and c_s == 0 for s != 0 -- for instance T = 1, D = P / 2,
 * h = g = the periodic sqrt-Hann window, or D = P, h = g = ones on the first P coefficients and zeros after.
 * Filter: fourier_hip_ipfb_set_filter_* takes P * T reals T on the device; NULL restores the default of all ones.  A set-up call: it
 * waits for `stream`.
 * create gives NULL for channels, taps or hop of 0 or a real_output flag outside {0, 1} (invalid), and for P * T or D above 2^31 - 1
 * (unsupported).  Frames per row stay below 2^31.
 * A NULL handle or pointer, frames = 0 or >= 2^31, length = 0 or > full(frames), d_in not aligned to 2 * sizeof(T), d_out not aligned
 * to its element (sizeof(T) for real rows, 2 * sizeof(T) for complex rows) or any overlap of d_in and d_out give
 * FOURIER_HIP_INVALID_ARGUMENT; batch == 0 is a successful no-op.  The input is not modified.
 * Stream-ordered on `stream` like fourier_hip_transform_batch_*.  One route (fourier_hip_ipfb_describe_*: "ipfb composed: <the inner
 * plan's describe>"): the inner plan -- the complex plan of P points, or the real-input plan of P points -- takes a chunk of frames,
 * unscaled, into a handle-owned scratch of rows of P values (at most 1 GiB, never fewer frames than cover one sample, ceil(P T / D)),
 * one gather launch writes the chunk's samples with the 1/P folded in.  The output does not depend on the chunking.
 * fourier_hip_ipfb_reserve_*(h, frames, batch) sizes everything inverse calls from at most `frames` frames and `batch` rows need: they
 * then never allocate.  NULL-handle calls return 0 from the getters, "" from describe and FOURIER_HIP_INVALID_ARGUMENT from the rest.
 * Handles are Send, not Sync, like the complex ones; status of the last call: fourier_hip_ipfb_last_status_*. */
struct fourier_ipfb_float;
struct fourier_ipfb_double;

/* NULL on failure (parameters outside the ranges above included). */
struct fourier_ipfb_float *fourier_hip_ipfb_create_float(FOURIER_SIZE_TYPE channels, FOURIER_SIZE_TYPE taps, FOURIER_SIZE_TYPE hop,
                                                         int real_output, int device);
struct fourier_ipfb_double *fourier_hip_ipfb_create_double(FOURIER_SIZE_TYPE channels, FOURIER_SIZE_TYPE taps, FOURIER_SIZE_TYPE hop,
                                                           int real_output, int device);
/* NULL is a no-op. */
void fourier_hip_ipfb_destroy_float(FOURIER_STRUCT fourier_ipfb_float *);
void fourier_hip_ipfb_destroy_double(FOURIER_STRUCT fourier_ipfb_double *);
/* 0 for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_ipfb_channels_float(const FOURIER_STRUCT fourier_ipfb_float *);
FOURIER_SIZE_TYPE fourier_hip_ipfb_channels_double(const FOURIER_STRUCT fourier_ipfb_double *);
FOURIER_SIZE_TYPE fourier_hip_ipfb_taps_float(const FOURIER_STRUCT fourier_ipfb_float *);
FOURIER_SIZE_TYPE fourier_hip_ipfb_taps_double(const FOURIER_STRUCT fourier_ipfb_double *);
FOURIER_SIZE_TYPE fourier_hip_ipfb_hop_float(const FOURIER_STRUCT fourier_ipfb_float *);
FOURIER_SIZE_TYPE fourier_hip_ipfb_hop_double(const FOURIER_STRUCT fourier_ipfb_double *);
FOURIER_SIZE_TYPE fourier_hip_ipfb_bins_float(const FOURIER_STRUCT fourier_ipfb_float *);
FOURIER_SIZE_TYPE fourier_hip_ipfb_bins_double(const FOURIER_STRUCT fourier_ipfb_double *);
/* full(frames), the longest row `frames` frames give; 0 for frames = 0 or >= 2^31 or a NULL handle */
FOURIER_SIZE_TYPE fourier_hip_ipfb_length_float(const FOURIER_STRUCT fourier_ipfb_float *, FOURIER_SIZE_TYPE frames);
FOURIER_SIZE_TYPE fourier_hip_ipfb_length_double(const FOURIER_STRUCT fourier_ipfb_double *, FOURIER_SIZE_TYPE frames);
int fourier_hip_ipfb_set_filter_float(FOURIER_STRUCT fourier_ipfb_float *, const void *d_filter, void *stream);
int fourier_hip_ipfb_set_filter_double(FOURIER_STRUCT fourier_ipfb_double *, const void *d_filter, void *stream);
int fourier_hip_ipfb_inverse_float(const FOURIER_STRUCT fourier_ipfb_float *, const void *d_in, void *d_out, FOURIER_SIZE_TYPE frames,
                                   FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch, void *stream);
int fourier_hip_ipfb_inverse_double(const FOURIER_STRUCT fourier_ipfb_double *, const void *d_in, void *d_out, FOURIER_SIZE_TYPE frames,
                                    FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE batch, void *stream);
int fourier_hip_ipfb_reserve_float(const FOURIER_STRUCT fourier_ipfb_float *, FOURIER_SIZE_TYPE frames, FOURIER_SIZE_TYPE batch);
int fourier_hip_ipfb_reserve_double(const FOURIER_STRUCT fourier_ipfb_double *, FOURIER_SIZE_TYPE frames, FOURIER_SIZE_TYPE batch);
/* "" for a NULL handle. */
const char *fourier_hip_ipfb_describe_float(const FOURIER_STRUCT fourier_ipfb_float *);
const char *fourier_hip_ipfb_describe_double(const FOURIER_STRUCT fourier_ipfb_double *);
int fourier_hip_ipfb_last_status_float(const FOURIER_STRUCT fourier_ipfb_float *);
int fourier_hip_ipfb_last_status_double(const FOURIER_STRUCT fourier_ipfb_double *);

/* ---------------- Fourier-domain resampling (extension; the reference has none) ----------------
 * `batch` contiguous rows of N = n_in values x on DEVICE memory -> `batch` contiguous rows of M = n_out values y: the row's spectrum
 * cut or zero-padded to M bins and transformed back.  K = min(N, M).  W is an optional window of N reals in FFT order (DC first);
 * absent (the default) means all ones.
 * Complex rows (real_input = 0, interleaved complex values):
 *   X = fft_N(x) * W, Y = M zeros;  Y[f mod M] = X[f mod N] for every signed frequency f with 2 |f| < K;  for an even K, h = K / 2:
 *   M < N: Y[h] = X[h] + X[N-h];   N < M: Y[h] = Y[M-h] = X[h] / 2;   N == M: Y[h] = X[h];   y = ifft_M(Y) * M / N.
 * Real rows (real_input = 1):
 *   X = rfft_N(x) * Wr, Wr[0] = W[0], Wr[k] = (W[k] + W[N-k]) / 2;  Y = M / 2 + 1 zeros;  Y[k] = X[k] for 2 k < K;  for an even K,
 *   Y[K/2] = X[K/2] * c with c = 2 for M < N, 1/2 for N < M, 1 for N == M;  y = irfft_M(Y) * M / N (the imaginary parts of bin 0 and of
 *   an even M's bin M / 2 are dropped, as irfft does).
 * This is scipy.signal.resample(x, M, axis=-1, window=W) with W given as an array, with ONE exception: for complex rows with
 * M == 2 < N scipy 1.15 does not add X[N-1] into Y[1] (a slice expression in its source is empty there); the rule above does, so that
 * complex rows whose imaginary part is zero agree with real rows.  scipy's `t`, domain='freq' and window names or callables have no
 * counterpart here.
 * Window: fourier_hip_resample_set_window_*(h, d_window, stream) takes n_in reals T on the device; NULL clears the window.  The handle
 * keeps a copy of its own (real rows: the folded Wr).  A set-up call: it waits for `stream`.
 * Routes (fourier_hip_resample_describe_*), chosen at create:
 *   "resample complex: ..."              complex rows: the N-point plan into a handle-owned scratch, one remap sweep into the output
 *                                        with the window, the rule of the bin K/2 and 1/N folded in, the M-point unscaled inverse in place
 *   "resample real composed: ..."        real rows: the real-input plan of N points, the remap sweep on half spectra, the real-input
 *                                        plan of M points
 *   "resample real fused untangle: ..."  real rows, N and M both even: the N/2-point inner plan, ONE sweep that does the work of the
 *                                        forward untangle, the remap and the inverse untangle, the M/2-point inner plan
 * Option "fusion" (fourier_hip_resample_set_option_*): 1 (the default: it measured faster at every shape) selects
 * the fused untangle route where it exists, 0 the composed one; on the other routes it is accepted and changes nothing.  Any other
 * key or value: FOURIER_HIP_INVALID_ARGUMENT.
 * create gives NULL for a length of 0 or a real_input flag outside {0, 1} (invalid) and for lengths beyond what the inner plans or
 * one sweep launch serve (2^31 - 1 bytes of a row's spectrum: unsupported).
 * A NULL handle or pointer, a buffer not aligned to its element (sizeof(T) for real rows, which may start on any T; 2 * sizeof(T) for
 * complex rows), or any overlap of d_in and d_out (in place included) give FOURIER_HIP_INVALID_ARGUMENT; batch == 0 is a successful
 * no-op.  The input is not modified.  Stream-ordered on `stream` like fourier_hip_transform_batch_*.  The batch is walked in chunks
 * of a handle-owned scratch of at most 1 GiB (never less than one row); there are no atomics, so the result does not depend on the
 * chunking and repeated calls give the same bits.  fourier_hip_resample_reserve_*(h, batch) sizes everything calls of at most `batch`
 * rows need on the current route: they then never allocate.  NULL-handle calls return 0 from the getters, "" from describe and
 * FOURIER_HIP_INVALID_ARGUMENT from the rest.  Handles are Send, not Sync, like the complex ones; status of the last call:
 * fourier_hip_resample_last_status_*. */
struct fourier_resample_float;
struct fourier_resample_double;

/* NULL on failure (parameters outside the ranges above included). */
struct fourier_resample_float *fourier_hip_resample_create_float(FOURIER_SIZE_TYPE n_in, FOURIER_SIZE_TYPE n_out, int real_input,
                                                                 int device);
struct fourier_resample_double *fourier_hip_resample_create_double(FOURIER_SIZE_TYPE n_in, FOURIER_SIZE_TYPE n_out, int real_input,
                                                                   int device);
/* NULL is a no-op. */
void fourier_hip_resample_destroy_float(FOURIER_STRUCT fourier_resample_float *);
void fourier_hip_resample_destroy_double(FOURIER_STRUCT fourier_resample_double *);
/* 0 for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_resample_size_in_float(const FOURIER_STRUCT fourier_resample_float *);
FOURIER_SIZE_TYPE fourier_hip_resample_size_in_double(const FOURIER_STRUCT fourier_resample_double *);
FOURIER_SIZE_TYPE fourier_hip_resample_size_out_float(const FOURIER_STRUCT fourier_resample_float *);
FOURIER_SIZE_TYPE fourier_hip_resample_size_out_double(const FOURIER_STRUCT fourier_resample_double *);
int fourier_hip_resample_real_input_float(const FOURIER_STRUCT fourier_resample_float *);
int fourier_hip_resample_real_input_double(const FOURIER_STRUCT fourier_resample_double *);
int fourier_hip_resample_forward_float(const FOURIER_STRUCT fourier_resample_float *, const void *d_in, void *d_out,
                                       FOURIER_SIZE_TYPE batch, void *stream);
int fourier_hip_resample_forward_double(const FOURIER_STRUCT fourier_resample_double *, const void *d_in, void *d_out,
                                        FOURIER_SIZE_TYPE batch, void *stream);
int fourier_hip_resample_set_window_float(FOURIER_STRUCT fourier_resample_float *, const void *d_window, void *stream);
int fourier_hip_resample_set_window_double(FOURIER_STRUCT fourier_resample_double *, const void *d_window, void *stream);
int fourier_hip_resample_reserve_float(const FOURIER_STRUCT fourier_resample_float *, FOURIER_SIZE_TYPE batch);
int fourier_hip_resample_reserve_double(const FOURIER_STRUCT fourier_resample_double *, FOURIER_SIZE_TYPE batch);
int fourier_hip_resample_set_option_float(FOURIER_STRUCT fourier_resample_float *, const char *key, long long value);
int fourier_hip_resample_set_option_double(FOURIER_STRUCT fourier_resample_double *, const char *key, long long value);
/* "" for a NULL handle. */
const char *fourier_hip_resample_describe_float(const FOURIER_STRUCT fourier_resample_float *);
const char *fourier_hip_resample_describe_double(const FOURIER_STRUCT fourier_resample_double *);
int fourier_hip_resample_last_status_float(const FOURIER_STRUCT fourier_resample_float *);
int fourier_hip_resample_last_status_double(const FOURIER_STRUCT fourier_resample_double *);

/* ---------------- pairwise cross-correlation and GCC-PHAT (extension; the reference has none) ----------
 * Of `batch` rows x[b] and `batch` rows y[b] of n = `size` values on DEVICE memory, row b at element offset b*n -- REALS T where the
 * handle was created with real_data = 1, interleaved COMPLEX values with real_data = 0 --, zero-extended to the transform length
 * L = `length` >= n, with X = fft(x~, L), Y = fft(y~, L) and G[k] = conj(X[k]) Y[k]:
 *   r[b][l] = ifft(G psi)[l] = sum_t conj(x~[b][t]) y~[b][(t + l) mod L]      (psi = 1),
 *   out[b][j] = r[b][(lag_first + j) mod L],   j = 0 .. lags-1,
 * `batch` rows of `lags` values out, reals for real rows and complex values for complex rows.  1 <= n <= L, 1 <= lags <= L and
 * |lag_first| < L (signed), else create fails.  L == n, lag_first = 0, lags = L is the circular correlation; L >= 2n - 1,
 * lag_first = -(n - 1), lags = 2n - 1 is numpy.correlate(y, x, "full") and scipy.signal.correlate(y, x, "full") -- mind the argument
 * order, it is the cross spectrum's conj(X) Y convention: a peak at lag l > 0 means that y lags x by l samples.
 * Option "weighting": FOURIER_XCORR_WEIGHT_NONE (0, the default): psi = 1.  FOURIER_XCORR_WEIGHT_PHAT (1): the generalized
 * cross-correlation with phase transform, G psi = conj(X / |X|) (Y / |Y|): the two unit phasors are formed separately, quotients first,
 * |.| = sqrt(re^2 + im^2) (the magnitude convention above, not a hypot), and the bin is exactly 0 where |X[k]| or |Y[k]| is 0: an
 * all-zero row gives an all-zero row, never a NaN.  There is no epsilon.  The 1/L of the inverse is folded into the product.
 * d_x == d_y is allowed: the autocorrelation.  The output may not overlap either input.  A NULL pointer, a real buffer not aligned to
 * sizeof(T) or a complex one not aligned to 2*sizeof(T), an overlap of the output with an input give FOURIER_HIP_INVALID_ARGUMENT.
 * batch == 0 is a successful no-op.  L * 2 * sizeof(T) > 2^31 - 1: create fails (as fourier_hip_hilbert_create_*).  Stream-ordered on
 * `stream` like fourier_hip_transform_batch_*.
 * Routes (fourier_hip_xcorr_describe_* begins with the route's name):
 *   "xcorr one-launch"  REAL rows, L = 2^11 ... 2^15 (double: ... 2^14), any n <= L and any window, where the kernel of that precision
 *                       and weighting runs without scratch memory -- double without weighting; elsewhere the handle stays on the
 *                       composed route and its description says so.  The two rows are scaled by powers of two to peaks in [1, 2),
 *                       x becomes the real and y the imaginary part of ONE complex row, then FFT, an exchange that separates X and Y,
 *                       the weighted product, inverse FFT and the store of the window in ONE launch on register-resident data; no
 *                       scratch.  Under PHAT a SINGLE bin where one spectrum is exactly 0 and the other is not keeps a unit phasor
 *                       there (X[k] is a difference of two roundings on this route); an all-zero row still gives an all-zero row.
 *   "xcorr composed"    every L.  The two rows are padded and transformed APART (real rows: to half spectra of L/2 + 1 values), one
 *                       sweep forms G psi / L, the unscaled inverse follows -- straight into the caller's output where the window is
 *                       the whole row (lag_first == 0, lags == L) --, and a last sweep stores the window.  Complex rows have no
 *                       one-launch route.
 * On every route power-of-two scaling of either input scales the unweighted output exactly while nothing over- or underflows, and
 * leaves the PHAT output bit-identical for every input whose values are normal numbers of T: the composed route brings every
 * spectrum value X[k], Y[k] to a larger component in [1, 2) by a power of two before it forms |X[k]|, |Y[k]| and the quotients, which
 * changes no bit of them while re^2 + im^2 is normal and keeps them right where it would have left the format ("Amplitude" above).
 * Option "fusion" (fourier_hip_xcorr_set_option_*): 1 = the one-launch route where it exists, the DEFAULT (it took 0.23 - 0.37 of the
 * composed route's time at every measured shape), 0 = the composed route.  The plan owns a scratch of at most
 * 1 GiB (never less than one row pair) and walks larger batches in chunks of it; the first call with a batch larger than any before
 * allocates it unless fourier_hip_xcorr_reserve_* was called for at least that batch.  No atomics: the result is the same on
 * repetition.  A NULL handle gives FOURIER_HIP_INVALID_ARGUMENT, 0 from fourier_hip_xcorr_size_* / _length_* / _lags_* and "" from
 * fourier_hip_xcorr_describe_*.  Handles are Send, not Sync, like the complex ones; status of the last call:
 * fourier_hip_xcorr_last_status_*. */
enum {
  FOURIER_XCORR_WEIGHT_NONE = 0,
  FOURIER_XCORR_WEIGHT_PHAT = 1
};
struct fourier_xcorr_float;
struct fourier_xcorr_double;

/* NULL on failure (a parameter outside the ranges above included). */
struct fourier_xcorr_float *fourier_hip_xcorr_create_float(FOURIER_SIZE_TYPE size, FOURIER_SIZE_TYPE length, long long lag_first,
                                                           FOURIER_SIZE_TYPE lags, int real_data, int device);
struct fourier_xcorr_double *fourier_hip_xcorr_create_double(FOURIER_SIZE_TYPE size, FOURIER_SIZE_TYPE length, long long lag_first,
                                                             FOURIER_SIZE_TYPE lags, int real_data, int device);
/* NULL is a no-op. */
void fourier_hip_xcorr_destroy_float(FOURIER_STRUCT fourier_xcorr_float *);
void fourier_hip_xcorr_destroy_double(FOURIER_STRUCT fourier_xcorr_double *);
/* n, L and the number of lags; 0 for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_xcorr_size_float(const FOURIER_STRUCT fourier_xcorr_float *);
FOURIER_SIZE_TYPE fourier_hip_xcorr_size_double(const FOURIER_STRUCT fourier_xcorr_double *);
FOURIER_SIZE_TYPE fourier_hip_xcorr_length_float(const FOURIER_STRUCT fourier_xcorr_float *);
FOURIER_SIZE_TYPE fourier_hip_xcorr_length_double(const FOURIER_STRUCT fourier_xcorr_double *);
FOURIER_SIZE_TYPE fourier_hip_xcorr_lags_float(const FOURIER_STRUCT fourier_xcorr_float *);
FOURIER_SIZE_TYPE fourier_hip_xcorr_lags_double(const FOURIER_STRUCT fourier_xcorr_double *);
int fourier_hip_xcorr_correlate_float(const FOURIER_STRUCT fourier_xcorr_float *, const void *d_x, const void *d_y, void *d_out,
                                      FOURIER_SIZE_TYPE batch, void *stream);
int fourier_hip_xcorr_correlate_double(const FOURIER_STRUCT fourier_xcorr_double *, const void *d_x, const void *d_y, void *d_out,
                                       FOURIER_SIZE_TYPE batch, void *stream);
int fourier_hip_xcorr_reserve_float(const FOURIER_STRUCT fourier_xcorr_float *, FOURIER_SIZE_TYPE batch);
int fourier_hip_xcorr_reserve_double(const FOURIER_STRUCT fourier_xcorr_double *, FOURIER_SIZE_TYPE batch);
/* "fusion": 0 / 1; "weighting": FOURIER_XCORR_WEIGHT_NONE / _PHAT.  Anything else: FOURIER_HIP_INVALID_ARGUMENT. */
int fourier_hip_xcorr_set_option_float(FOURIER_STRUCT fourier_xcorr_float *, const char *key, long long value);
int fourier_hip_xcorr_set_option_double(FOURIER_STRUCT fourier_xcorr_double *, const char *key, long long value);
/* "" for a NULL handle. */
const char *fourier_hip_xcorr_describe_float(const FOURIER_STRUCT fourier_xcorr_float *);
const char *fourier_hip_xcorr_describe_double(const FOURIER_STRUCT fourier_xcorr_double *);
int fourier_hip_xcorr_last_status_float(const FOURIER_STRUCT fourier_xcorr_float *);
int fourier_hip_xcorr_last_status_double(const FOURIER_STRUCT fourier_xcorr_double *);

/* ---------------- fractional delay and delay-and-sum (extension; the reference has none) ----------
 * `batch` rows x[r] of n = `size` values on DEVICE memory, row r at element offset r*n -- REALS T where the handle was created with
 * real_data = 1, interleaved COMPLEX values with real_data = 0 --, zero-extended to the transform length L = `length` >= n, are
 * delayed by d[r] samples each, optionally weighted by w[r], and summed over groups of C = `channels` consecutive rows (C = 1: the
 * plain fractional delay).  With X = fft(x~, L):
 *   Y[g][k] = sum_{c < C, ascending c} w[gC+c] X[gC+c][k] m(k, d[gC+c]),    out[g][t] = ifft(Y[g])[t],  t = 0 .. n-1,
 *   m(k, d) = exp(-2 pi i k' d / L),  k' = k for k < L/2 and k - L for k > L/2;   m(L/2, d) = cos(pi d)  (even L, real and complex rows),
 * batch / C rows of n values out, reals for real rows and complex values for complex rows.  A POSITIVE d delays: out[t] = x[t - d]; to
 * align a channel that arrived late by tau pass -tau.  The shift is circular over L; with L >= n + ceil(max |d|) it is the linear
 * delay with zeros shifting in, and L == n is the circular shift (an integer d: numpy.roll).
 * d_delays and d_weights hold one value of the handle's real type T per INPUT row, on the device: the delays in samples, the weights
 * reals.  d_weights == NULL means every weight is 1 (a plain sum, not a mean).  Nothing about them crosses to the host: the argmax of
 * a GCC-PHAT can feed d_delays directly, and a captured graph may be replayed after they were overwritten.  Any finite T is a valid
 * delay; the phase error does not grow with |d| or with k: d is reduced modulo L by fmod and split into rint and a remainder (all
 * exact), (k d_int) mod L is formed in integer arithmetic, the fraction adds at most a quarter turn, and one accurate sincospi of the
 * sum follows.  A delay never enters an address: a delay or weight that is not finite makes the output rows of its group not finite
 * and touches nothing else; it is not an error.
 * 1 <= n <= L, C >= 1 and real_data 0 / 1, else create fails; so it does for L * 2 * sizeof(T) > 2^31 - 1 (as
 * fourier_hip_hilbert_create_*) and for C * L * 2 * sizeof(T) > 2^31 - 1.  batch % C != 0, a NULL d_in / d_delays / d_out, a real
 * buffer (d_delays and d_weights included) not aligned to sizeof(T) or a complex one not aligned to 2*sizeof(T), a partial overlap of
 * input and output, and ANY overlap of them when C > 1 give FOURIER_HIP_INVALID_ARGUMENT.  d_out == d_in is allowed when C == 1.
 * batch == 0 is a successful no-op.  Stream-ordered on `stream` like fourier_hip_transform_batch_*.
 * Routes (fourier_hip_delay_describe_* begins with the route's name):
 *   "delay one-launch"  REAL rows, C == 1, L = 2^11 ... 2^15 (double: ... 2^14), any n <= L: load, FFT, the phase (from the bin index, no
 *                       table), inverse FFT and the store of the first n values in ONE launch on register-resident data; no scratch.
 *   "delay composed"    every L, real and complex rows, every C: the rows are padded to L and transformed (real rows: to half spectra of
 *                       L/2 + 1 values), ONE sweep forms Y / L for each group, ONE unscaled inverse a group follows -- straight into the
 *                       caller's output where n == L --, and a last sweep stores the first n values.  A group of C channels costs C
 *                       forward transforms and one inverse.
 * On every route scaling the input, or every weight, by a power of two scales the output exactly while nothing over- or underflows.
 * Option "fusion" (fourier_hip_delay_set_option_*): 1 = the one-launch route where it exists, the DEFAULT (it took 0.26 - 0.42 of the
 * composed route's time at every measured shape, DESIGN.md section 4, "Fractional delay"), 0 = the composed route.  The plan owns a scratch of at most 1 GiB (never less than one group) and walks larger
 * batches in chunks of whole groups; the first call with a batch larger than any before allocates it unless
 * fourier_hip_delay_reserve_* was called for at least that batch.  No atomics: the result is the same on repetition.  A NULL handle
 * gives FOURIER_HIP_INVALID_ARGUMENT, 0 from fourier_hip_delay_size_* / _length_* / _channels_* and "" from
 * fourier_hip_delay_describe_*.  Handles are Send, not Sync, like the complex ones; status of the last call:
 * fourier_hip_delay_last_status_*. */
struct fourier_delay_float;
struct fourier_delay_double;

/* NULL on failure (a parameter outside the ranges above included). */
struct fourier_delay_float *fourier_hip_delay_create_float(FOURIER_SIZE_TYPE size, FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE channels,
                                                           int real_data, int device);
struct fourier_delay_double *fourier_hip_delay_create_double(FOURIER_SIZE_TYPE size, FOURIER_SIZE_TYPE length, FOURIER_SIZE_TYPE channels,
                                                             int real_data, int device);
/* NULL is a no-op. */
void fourier_hip_delay_destroy_float(FOURIER_STRUCT fourier_delay_float *);
void fourier_hip_delay_destroy_double(FOURIER_STRUCT fourier_delay_double *);
/* n, L and C; 0 for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_delay_size_float(const FOURIER_STRUCT fourier_delay_float *);
FOURIER_SIZE_TYPE fourier_hip_delay_size_double(const FOURIER_STRUCT fourier_delay_double *);
FOURIER_SIZE_TYPE fourier_hip_delay_length_float(const FOURIER_STRUCT fourier_delay_float *);
FOURIER_SIZE_TYPE fourier_hip_delay_length_double(const FOURIER_STRUCT fourier_delay_double *);
FOURIER_SIZE_TYPE fourier_hip_delay_channels_float(const FOURIER_STRUCT fourier_delay_float *);
FOURIER_SIZE_TYPE fourier_hip_delay_channels_double(const FOURIER_STRUCT fourier_delay_double *);
/* `batch` input rows, `batch` delays, `batch` weights or NULL -> batch / C output rows. */
int fourier_hip_delay_apply_float(const FOURIER_STRUCT fourier_delay_float *, const void *d_in, const void *d_delays,
                                  const void *d_weights, void *d_out, FOURIER_SIZE_TYPE batch, void *stream);
int fourier_hip_delay_apply_double(const FOURIER_STRUCT fourier_delay_double *, const void *d_in, const void *d_delays,
                                   const void *d_weights, void *d_out, FOURIER_SIZE_TYPE batch, void *stream);
int fourier_hip_delay_reserve_float(const FOURIER_STRUCT fourier_delay_float *, FOURIER_SIZE_TYPE batch);
int fourier_hip_delay_reserve_double(const FOURIER_STRUCT fourier_delay_double *, FOURIER_SIZE_TYPE batch);
/* "fusion": 0 / 1.  Anything else: FOURIER_HIP_INVALID_ARGUMENT. */
int fourier_hip_delay_set_option_float(FOURIER_STRUCT fourier_delay_float *, const char *key, long long value);
int fourier_hip_delay_set_option_double(FOURIER_STRUCT fourier_delay_double *, const char *key, long long value);
/* "" for a NULL handle. */
const char *fourier_hip_delay_describe_float(const FOURIER_STRUCT fourier_delay_float *);
const char *fourier_hip_delay_describe_double(const FOURIER_STRUCT fourier_delay_double *);
int fourier_hip_delay_last_status_float(const FOURIER_STRUCT fourier_delay_float *);
int fourier_hip_delay_last_status_double(const FOURIER_STRUCT fourier_delay_double *);

/* ---------------- real cepstrum and minimum-phase reconstruction (extension; the reference has none) ----------
 * `batch` rows x[r] of n = `size` REALS T on DEVICE memory, row r at element offset r*n, zero-extended to the transform length
 * L = `length` >= n.  With X = fft(x~, L) and the per-call reals log_mult != 0 and log_floor >= 0:
 *   g[k] = log_mult ln(max(|X[k]|, log_floor)),
 * formed as 0.5 log_mult ln(max(re^2 + im^2, log_floor^2)) with the accurate logarithm, never the fast hardware one.
 *   mode 0, CEPSTRUM:       c = ifft(g), which is real and even;  out[r][q] = c[q], q = 0 .. m-1, m = `outputs` <= L
 *                           (log_mult = 1: the real cepstrum irfft(log|rfft(x)|)).
 *   mode 1, MINIMUM_PHASE:  the fold chat[0] = c[0]; chat[q] = 2 c[q] for 0 < q < L/2 (odd L: q <= (L-1)/2); chat[L/2] = c[L/2]
 *                           (even L); chat[q] = 0 above.  C = fft(chat), E[k] = exp(Re C[k]) (cos Im C[k], sin Im C[k]),
 *                           h = Re ifft(E);  out[r][t] = h[t], t = 0 .. m-1.  log_mult = 1 is
 *                           scipy.signal.minimum_phase(x, method="homomorphic", n_fft=L, half=False), log_mult = 0.5 its half=True.
 * Two deviations from scipy 1.15.3.  The FLOOR: scipy adds 1e-7 x the smallest positive |X| to |X|, a reduction over the data; here
 * the floor is the caller's log_floor, applied with max.  The FOLD AT EVEN L: scipy's window leaves quefrency L/2 at weight 0; here
 * it keeps weight 1 (Oppenheim and Schafer, eq. 13.42b).  On firwin(101, 0.3) at L = 2048 and 8192 the two definitions agree to
 * 2.3e-7 and 1.8e-7 relative in f64.
 * log_floor == 0 on a bin that is exactly 0 gives -inf there: that row's output is not finite, nothing else is touched, and it is
 * not an error.  No value of a row enters an address.  A NaN in a row makes that row's output NaN.
 * Amplitude range: re^2 + im^2 must neither overflow nor flush to zero in T, so sqrt(min normal) < |X[k]| < sqrt(max):
 * 1.1e-19 .. 1.8e19 in float, 1.5e-154 .. 1.3e154 in double (a bin below the range counts as 0: the floor, or -inf).  The FLOOR is
 * not bound by that range: every log_floor > 0 that is a normal number of T is honoured, whatever log_floor^2 does in T.  A bin whose
 * re^2 + im^2 is below log_floor^2 gives log_mult ln(log_floor) -- below sqrt(min normal) that is every bin whose re^2 + im^2 is
 * less than the smallest normal number, a zero row and a bin that flushed to zero included; above sqrt(max) it is every bin whose
 * re^2 + im^2 is finite.  Where log_floor^2 is a normal number of T the arithmetic is ln(max(re^2 + im^2, log_floor^2)) as written
 * above.  (In mode 1 a floored row gives h[0] = log_floor^log_mult, which must itself fit T: exp(Re C) / L is formed in T.)  Scaling x by
 * 2^j moves c[0] by j log_mult ln 2 and h by 2^(j log_mult): bit-exact power-of-two scaling is NOT claimed for this family.
 * The phase of E goes through one accurate sincospi of Im C / pi, the exponential is the accurate one.
 * n == 0, n > L, m == 0, m > L, a mode other than 0 / 1 make create fail; so does L * 2 * sizeof(T) > 2^31 - 1 (as
 * fourier_hip_hilbert_create_*).  log_mult == 0, a log_mult or log_floor that is not finite, log_floor < 0 -- and, AFTER ROUNDING TO T,
 * a log_mult that is 0 or not finite (float: 1e-50, 1e60) or a log_floor > 0 that is 0, subnormal or inf (float: 1e-200, 1e-40, 1e39)
 * --, a NULL buffer, a buffer not aligned to sizeof(T), and an overlap of input and output other than d_out == d_in with m == n give
 * FOURIER_HIP_INVALID_ARGUMENT and write nothing.  log_floor == 0 keeps meaning "no floor".
 * batch == 0 is a successful no-op.  Stream-ordered on `stream` like fourier_hip_transform_batch_*.
 * Routes (fourier_hip_cepstrum_describe_* begins with the route's name):
 *   "cepstrum one-launch"  L = 2^11 ... 2^15 (double: ... 2^14) where the library holds a kernel of the mode: load, FFT, logarithm,
 *                          inverse FFT -- and for mode 1 the fold, FFT, complex exponential and inverse FFT -- and the store of the
 *                          first m values in ONE launch on register-resident data; no scratch.
 *   "cepstrum composed"    every L (odd and Bluestein lengths included): the rows are padded to L, transformed to half spectra, ONE
 *                          sweep forms g / L in place, an unscaled inverse follows; mode 1 goes on with a fold sweep, a forward
 *                          transform, a sweep that forms E / L and an unscaled inverse; the last inverse writes straight into the
 *                          caller's output where m == L, else a last sweep stores the first m values.
 * Option "fusion" (fourier_hip_cepstrum_set_option_*): 1 = the one-launch route where it exists, the DEFAULT (it took 0.26 - 0.53 of
 * the composed route's time at every measured shape, DESIGN.md section 4, "Cepstrum and minimum phase"), 0 = the composed route.
 * The plan owns a scratch of at most 1 GiB (never less than one row)
 * and walks larger batches in chunks of whole rows; the first call with a batch larger than any before allocates it unless
 * fourier_hip_cepstrum_reserve_* was called for at least that batch.  No atomics: the result is the same on repetition.  A NULL
 * handle gives FOURIER_HIP_INVALID_ARGUMENT, 0 from fourier_hip_cepstrum_size_* / _length_* / _outputs_*, -1 from
 * fourier_hip_cepstrum_mode_* and "" from fourier_hip_cepstrum_describe_*.  Handles are Send, not Sync, like the complex ones; status
 * of the last call: fourier_hip_cepstrum_last_status_*. */
struct fourier_cepstrum_float;
struct fourier_cepstrum_double;

#define FOURIER_CEPSTRUM_MODE_CEPSTRUM 0
#define FOURIER_CEPSTRUM_MODE_MINIMUM_PHASE 1

/* NULL on failure (a parameter outside the ranges above included). */
struct fourier_cepstrum_float *fourier_hip_cepstrum_create_float(FOURIER_SIZE_TYPE size, FOURIER_SIZE_TYPE length,
                                                                 FOURIER_SIZE_TYPE outputs, int mode, int device);
struct fourier_cepstrum_double *fourier_hip_cepstrum_create_double(FOURIER_SIZE_TYPE size, FOURIER_SIZE_TYPE length,
                                                                   FOURIER_SIZE_TYPE outputs, int mode, int device);
/* NULL is a no-op. */
void fourier_hip_cepstrum_destroy_float(FOURIER_STRUCT fourier_cepstrum_float *);
void fourier_hip_cepstrum_destroy_double(FOURIER_STRUCT fourier_cepstrum_double *);
/* n, L and m; 0 for a NULL handle.  The mode; -1 for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_cepstrum_size_float(const FOURIER_STRUCT fourier_cepstrum_float *);
FOURIER_SIZE_TYPE fourier_hip_cepstrum_size_double(const FOURIER_STRUCT fourier_cepstrum_double *);
FOURIER_SIZE_TYPE fourier_hip_cepstrum_length_float(const FOURIER_STRUCT fourier_cepstrum_float *);
FOURIER_SIZE_TYPE fourier_hip_cepstrum_length_double(const FOURIER_STRUCT fourier_cepstrum_double *);
FOURIER_SIZE_TYPE fourier_hip_cepstrum_outputs_float(const FOURIER_STRUCT fourier_cepstrum_float *);
FOURIER_SIZE_TYPE fourier_hip_cepstrum_outputs_double(const FOURIER_STRUCT fourier_cepstrum_double *);
int fourier_hip_cepstrum_mode_float(const FOURIER_STRUCT fourier_cepstrum_float *);
int fourier_hip_cepstrum_mode_double(const FOURIER_STRUCT fourier_cepstrum_double *);
/* `batch` rows of n reals -> `batch` rows of m reals. */
int fourier_hip_cepstrum_apply_float(const FOURIER_STRUCT fourier_cepstrum_float *, const void *d_in, void *d_out,
                                     FOURIER_SIZE_TYPE batch, double log_mult, double log_floor, void *stream);
int fourier_hip_cepstrum_apply_double(const FOURIER_STRUCT fourier_cepstrum_double *, const void *d_in, void *d_out,
                                      FOURIER_SIZE_TYPE batch, double log_mult, double log_floor, void *stream);
int fourier_hip_cepstrum_reserve_float(const FOURIER_STRUCT fourier_cepstrum_float *, FOURIER_SIZE_TYPE batch);
int fourier_hip_cepstrum_reserve_double(const FOURIER_STRUCT fourier_cepstrum_double *, FOURIER_SIZE_TYPE batch);
/* "fusion": 0 / 1.  Anything else: FOURIER_HIP_INVALID_ARGUMENT. */
int fourier_hip_cepstrum_set_option_float(FOURIER_STRUCT fourier_cepstrum_float *, const char *key, long long value);
int fourier_hip_cepstrum_set_option_double(FOURIER_STRUCT fourier_cepstrum_double *, const char *key, long long value);
/* "" for a NULL handle. */
const char *fourier_hip_cepstrum_describe_float(const FOURIER_STRUCT fourier_cepstrum_float *);
const char *fourier_hip_cepstrum_describe_double(const FOURIER_STRUCT fourier_cepstrum_double *);
int fourier_hip_cepstrum_last_status_float(const FOURIER_STRUCT fourier_cepstrum_float *);
int fourier_hip_cepstrum_last_status_double(const FOURIER_STRUCT fourier_cepstrum_double *);

/* ---------------- non-uniform FFT, 1-D, types 1 and 2 (extension; the reference has none) ----------
 * FINUFFT's 1-D type 1 and type 2 with the points shared by the rows of a batch.  A handle is created for n_modes = N >= 1 and a
 * requested accuracy eps; fourier_hip_nufft_set_points_* gives it M >= 0 points x_j, any finite reals, taken modulo 2 pi.  The mode
 * index k runs over -floor(N/2) .. ceil(N/2) - 1.  With s = `sign`, +1 or -1 per call:
 *   to_modes  (type 1)   f[b][k] = sum_j c[b][j] exp(i s k x_j)     `batch` rows of M complex T in, `batch` rows of N complex T out
 *   to_points (type 2)   c[b][j] = sum_k f[b][k] exp(i s k x_j)     `batch` rows of N complex T in, `batch` rows of M complex T out
 * on DEVICE memory, interleaved complex values, row b at element offset b*M or b*N.  `order` 0 stores the modes with k ascending as
 * above, 1 in FFT order (k = 0 .. ceil(N/2) - 1, -floor(N/2) .. -1).  There is no scale factor; to_points with sign s is the exact
 * adjoint of to_modes with sign -s.
 * The algorithm is fixed: the "exponential of semicircle" kernel phi(z) = exp(beta (sqrt(1 - z^2) - 1)) on |z| <= 1, beta = 2.30 w, of
 * width w = ceil(log10(1 / eps)) + 1 clamped to 2 .. 8 (float) or 2 .. 16 (double), on a fine grid whose length L is the smallest
 * 2^a 3^b 5^c >= max(2 N, 2 w); a point with grid coordinate xg = (x mod 2 pi) L / (2 pi) touches the cells ceil(xg - w/2) + 0 .. w - 1
 * modulo L with weight phi(2 (i - xg) / w); the deconvolution factor 1 / phihat(k), phihat(k) the integral over |t| <= w/2 of
 * phi(2 t / w) cos(2 pi k t / L), is computed on the host in double by a quadrature good to 1e-15.  to_modes spreads onto the grid (a
 * gather over the sorted points: no atomics), runs the L-point plan (FFT for s = -1, UNSCALED_IFFT for s = +1), picks the N modes
 * and multiplies by 1 / phihat; to_points writes f / phihat into a zeroed grid, runs the plan and interpolates at the points.  The
 * relative L2 error of a call against the direct sum is about 10^(1 - w), plus the rounding of T.
 * fourier_hip_nufft_set_points_*: h_points points to m doubles on the HOST, for both precisions (the fold modulo 2 pi needs them).  A
 * set-up call like fourier_hip_bandspec_set_bands_*: it waits for `stream`, sorts the points by grid coordinate (stable: equal points
 * keep the caller's order), uploads the tables and waits again.  Calling it again replaces the points; m == 0 is valid (to_modes then
 * writes zeros, to_points writes nothing).  A NaN or infinite point, m > 2^31 - 1, m * 2 * sizeof(T) > 2^30, a NULL pointer with m > 0
 * or one not aligned to 8 bytes give FOURIER_HIP_INVALID_ARGUMENT and leave the points as they were; so does an allocation or copy
 * that fails (the new tables replace the old ones only when all of them are complete).
 * A transform call before any set_points, sign other than +1 / -1, order other than 0 / 1, a NULL or misaligned (2*sizeof(T)) buffer
 * and ANY overlap of input and output give FOURIER_HIP_INVALID_ARGUMENT and write nothing.  batch == 0 is a successful no-op.
 * n_modes == 0, eps <= 0 or not finite, or a row above 2^30 bytes: create fails.  Stream-ordered on `stream` like
 * fourier_hip_transform_batch_*.
 * Option "table" (fourier_hip_nufft_set_option_*): 0 = "nufft evaluated", the weights are evaluated in the two hot kernels with the
 * accurate exp and sqrt; 1 = "nufft tabulated", a set-up kernel writes the M x w weights once (at set_points, or at set_option on the
 * null stream when points are set) and the hot kernels read them.  The two routes agree to rounding.  The default is 0: the
 * tabulated route beat the evaluated one at none of the measured shapes ("Non-uniform FFT").  fourier_hip_nufft_describe_* begins "nufft evaluated: " or
 * "nufft tabulated: ", then "w <w>, L <L>, " and the inner plan's description.
 * The plan owns a scratch of fine-grid rows of at most 1 GiB (never less than one row) and walks larger batches in chunks; the first
 * call with a batch larger than any before allocates it unless fourier_hip_nufft_reserve_* was called for at least that batch.  No
 * atomics and a summation order fixed by the points: the result is the same on repetition.  A NULL handle gives
 * FOURIER_HIP_INVALID_ARGUMENT, 0 from fourier_hip_nufft_modes_* / _points_* and "" from fourier_hip_nufft_describe_*.  Handles are
 * Send, not Sync, like the complex ones; status of the last call: fourier_hip_nufft_last_status_*. */
struct fourier_nufft_float;
struct fourier_nufft_double;

/* NULL on failure (a parameter outside the ranges above included). */
struct fourier_nufft_float *fourier_hip_nufft_create_float(FOURIER_SIZE_TYPE n_modes, double eps, int device);
struct fourier_nufft_double *fourier_hip_nufft_create_double(FOURIER_SIZE_TYPE n_modes, double eps, int device);
/* NULL is a no-op. */
void fourier_hip_nufft_destroy_float(FOURIER_STRUCT fourier_nufft_float *);
void fourier_hip_nufft_destroy_double(FOURIER_STRUCT fourier_nufft_double *);
/* N, and the M of the last set_points (0 before any); 0 for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_nufft_modes_float(const FOURIER_STRUCT fourier_nufft_float *);
FOURIER_SIZE_TYPE fourier_hip_nufft_modes_double(const FOURIER_STRUCT fourier_nufft_double *);
FOURIER_SIZE_TYPE fourier_hip_nufft_points_float(const FOURIER_STRUCT fourier_nufft_float *);
FOURIER_SIZE_TYPE fourier_hip_nufft_points_double(const FOURIER_STRUCT fourier_nufft_double *);
/* m doubles on the host, for both precisions. */
int fourier_hip_nufft_set_points_float(FOURIER_STRUCT fourier_nufft_float *, const double *h_points, FOURIER_SIZE_TYPE m, void *stream);
int fourier_hip_nufft_set_points_double(FOURIER_STRUCT fourier_nufft_double *, const double *h_points, FOURIER_SIZE_TYPE m, void *stream);
int fourier_hip_nufft_to_modes_batch_float(const FOURIER_STRUCT fourier_nufft_float *, const void *d_in, void *d_out,
                                           FOURIER_SIZE_TYPE batch, int sign, int order, void *stream);
int fourier_hip_nufft_to_modes_batch_double(const FOURIER_STRUCT fourier_nufft_double *, const void *d_in, void *d_out,
                                            FOURIER_SIZE_TYPE batch, int sign, int order, void *stream);
int fourier_hip_nufft_to_points_batch_float(const FOURIER_STRUCT fourier_nufft_float *, const void *d_in, void *d_out,
                                            FOURIER_SIZE_TYPE batch, int sign, int order, void *stream);
int fourier_hip_nufft_to_points_batch_double(const FOURIER_STRUCT fourier_nufft_double *, const void *d_in, void *d_out,
                                             FOURIER_SIZE_TYPE batch, int sign, int order, void *stream);
int fourier_hip_nufft_reserve_float(const FOURIER_STRUCT fourier_nufft_float *, FOURIER_SIZE_TYPE batch);
int fourier_hip_nufft_reserve_double(const FOURIER_STRUCT fourier_nufft_double *, FOURIER_SIZE_TYPE batch);
/* "table": 0 / 1.  Anything else: FOURIER_HIP_INVALID_ARGUMENT. */
int fourier_hip_nufft_set_option_float(FOURIER_STRUCT fourier_nufft_float *, const char *key, long long value);
int fourier_hip_nufft_set_option_double(FOURIER_STRUCT fourier_nufft_double *, const char *key, long long value);
/* "" for a NULL handle. */
const char *fourier_hip_nufft_describe_float(const FOURIER_STRUCT fourier_nufft_float *);
const char *fourier_hip_nufft_describe_double(const FOURIER_STRUCT fourier_nufft_double *);
int fourier_hip_nufft_last_status_float(const FOURIER_STRUCT fourier_nufft_float *);
int fourier_hip_nufft_last_status_double(const FOURIER_STRUCT fourier_nufft_double *);

/* ---------------- non-uniform FFT, 2-D, types 1 and 2 (extension; the reference has none) ----------
 * FINUFFT's 2-D type 1 and type 2 in C order with the points shared by the items of a batch.  A handle is created for n1 x n2 modes
 * (each >= 1) and a requested accuracy eps; fourier_hip_nufft2d_set_points_* gives it M >= 0 points (x1_j, x2_j), any finite reals,
 * taken modulo 2 pi per coordinate.  Coordinate d pairs with axis d of the mode array; k_d runs over -floor(n_d/2) .. ceil(n_d/2) - 1.
 * With s = `sign`, +1 or -1 per call:
 *   to_modes  (type 1)   f[b][k1][k2] = sum_j c[b][j] exp(i s (k1 x1_j + k2 x2_j))        `batch` rows of M in, `batch` items of n1 x n2 out
 *   to_points (type 2)   c[b][j] = sum_{k1,k2} f[b][k1][k2] exp(i s (k1 x1_j + k2 x2_j))  `batch` items of n1 x n2 in, `batch` rows of M out
 * on DEVICE memory, interleaved complex T, the last mode axis contiguous, item b at element offset b*M or b*n1*n2.  `order` 0 stores
 * both axes with k ascending, 1 both in FFT order (numpy's ifftshift over both axes of order 0).  There is no scale factor; to_points
 * with sign s is the exact adjoint of to_modes with sign -s.
 * The algorithm is fourier_hip_nufft_*'s per axis: the same kernel phi with beta = 2.30 w, the same w = ceil(log10(1 / eps)) + 1 clamped
 * to 2 .. 8 (float) or 2 .. 16 (double), one w for both axes; L_d is the smallest 2^a 3^b 5^c >= max(2 n_d, 2 w); a point's weight on
 * cell (i1, i2) is the product of its two 1-D weights, and the deconvolution factor is 1 / (phihat_1(|k1|) phihat_2(|k2|)), two 1-D
 * tables from the same quadrature.  to_modes spreads onto grid items of L1 x L2 (a gather over the points, bucketed by their first
 * axis-1 cell and sorted by their axis-2 coordinate: no atomics), transforms the rows of L2 and then axis 1 in place (FFT for s = -1,
 * UNSCALED_IFFT for s = +1), picks the n1 x n2 modes and multiplies by 1 / phihat; to_points writes f / phihat into a zeroed grid,
 * transforms and interpolates at the points.  The relative L2 error of a call against the direct sum is about 2 x 10^(1 - w), plus
 * the rounding of T.
 * fourier_hip_nufft2d_set_points_*: h_x1 and h_x2 each point to m doubles on the HOST, for both precisions.  A set-up call like
 * fourier_hip_nufft_set_points_*: it waits for `stream`, sorts (stable: equal points keep the caller's order), uploads the tables and
 * waits again.  Calling it again replaces the points; m == 0 is valid (to_modes then writes zeros, to_points writes nothing).  A NaN
 * or infinite coordinate in either array, m > 2^31 - 1, m * 2 * sizeof(T) > 2^30, a NULL pointer with m > 0 or one not aligned to 8
 * bytes give FOURIER_HIP_INVALID_ARGUMENT and leave the points as they were; so does an allocation or copy that fails (the new tables
 * replace the old ones only when all of them are complete).
 * A transform call before any set_points, sign other than +1 / -1, order other than 0 / 1, a NULL or misaligned (2*sizeof(T)) buffer
 * and ANY overlap of input and output give FOURIER_HIP_INVALID_ARGUMENT and write nothing.  batch == 0 is a successful no-op.
 * n1 == 0 or n2 == 0, eps <= 0 or not finite, n1 * n2 items above 2^30 bytes or a grid item above 2^31 bytes: create fails.
 * Stream-ordered on `stream` like fourier_hip_transform_batch_*.
 * Option "table" (fourier_hip_nufft2d_set_option_*): 0 = "nufft2d evaluated", the weights are evaluated in the two hot kernels with
 * the accurate exp and sqrt; 1 = "nufft2d tabulated", a set-up kernel writes the 2 x w x M weights once (at set_points, or at set_option
 * on the null stream when points are set) and the hot kernels read them.  The two routes agree to rounding.  The default is 0: the
 * tabulated route beat the evaluated one at one of the ten measured lines only ("Non-uniform FFT, 2-D").  fourier_hip_nufft2d_describe_* begins "nufft2d evaluated: " or "nufft2d
 * tabulated: ", then "w <w>, L <L1> x <L2>, " and the descriptions of the row plan and of the axis-1 route.
 * The plan owns a scratch of fine-grid items of at most 1 GiB (never less than one item) and walks larger batches in chunks; the first
 * call with a batch larger than any before allocates it unless fourier_hip_nufft2d_reserve_* was called for at least that batch.  No
 * atomics and a summation order fixed by the points: the result is the same on repetition.  A NULL handle gives
 * FOURIER_HIP_INVALID_ARGUMENT, 0 from fourier_hip_nufft2d_modes1_* / _modes2_* / _points_* and "" from fourier_hip_nufft2d_describe_*.
 * Handles are Send, not Sync, like the complex ones; status of the last call: fourier_hip_nufft2d_last_status_*. */
struct fourier_nufft2d_float;
struct fourier_nufft2d_double;

/* NULL on failure (a parameter outside the ranges above included). */
struct fourier_nufft2d_float *fourier_hip_nufft2d_create_float(FOURIER_SIZE_TYPE n1, FOURIER_SIZE_TYPE n2, double eps, int device);
struct fourier_nufft2d_double *fourier_hip_nufft2d_create_double(FOURIER_SIZE_TYPE n1, FOURIER_SIZE_TYPE n2, double eps, int device);
/* NULL is a no-op. */
void fourier_hip_nufft2d_destroy_float(FOURIER_STRUCT fourier_nufft2d_float *);
void fourier_hip_nufft2d_destroy_double(FOURIER_STRUCT fourier_nufft2d_double *);
/* n1, n2, and the M of the last set_points (0 before any); 0 for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_nufft2d_modes1_float(const FOURIER_STRUCT fourier_nufft2d_float *);
FOURIER_SIZE_TYPE fourier_hip_nufft2d_modes1_double(const FOURIER_STRUCT fourier_nufft2d_double *);
FOURIER_SIZE_TYPE fourier_hip_nufft2d_modes2_float(const FOURIER_STRUCT fourier_nufft2d_float *);
FOURIER_SIZE_TYPE fourier_hip_nufft2d_modes2_double(const FOURIER_STRUCT fourier_nufft2d_double *);
FOURIER_SIZE_TYPE fourier_hip_nufft2d_points_float(const FOURIER_STRUCT fourier_nufft2d_float *);
FOURIER_SIZE_TYPE fourier_hip_nufft2d_points_double(const FOURIER_STRUCT fourier_nufft2d_double *);
/* two arrays of m doubles on the host, for both precisions. */
int fourier_hip_nufft2d_set_points_float(FOURIER_STRUCT fourier_nufft2d_float *, const double *h_x1, const double *h_x2,
                                         FOURIER_SIZE_TYPE m, void *stream);
int fourier_hip_nufft2d_set_points_double(FOURIER_STRUCT fourier_nufft2d_double *, const double *h_x1, const double *h_x2,
                                          FOURIER_SIZE_TYPE m, void *stream);
int fourier_hip_nufft2d_to_modes_batch_float(const FOURIER_STRUCT fourier_nufft2d_float *, const void *d_in, void *d_out,
                                             FOURIER_SIZE_TYPE batch, int sign, int order, void *stream);
int fourier_hip_nufft2d_to_modes_batch_double(const FOURIER_STRUCT fourier_nufft2d_double *, const void *d_in, void *d_out,
                                              FOURIER_SIZE_TYPE batch, int sign, int order, void *stream);
int fourier_hip_nufft2d_to_points_batch_float(const FOURIER_STRUCT fourier_nufft2d_float *, const void *d_in, void *d_out,
                                              FOURIER_SIZE_TYPE batch, int sign, int order, void *stream);
int fourier_hip_nufft2d_to_points_batch_double(const FOURIER_STRUCT fourier_nufft2d_double *, const void *d_in, void *d_out,
                                               FOURIER_SIZE_TYPE batch, int sign, int order, void *stream);
int fourier_hip_nufft2d_reserve_float(const FOURIER_STRUCT fourier_nufft2d_float *, FOURIER_SIZE_TYPE batch);
int fourier_hip_nufft2d_reserve_double(const FOURIER_STRUCT fourier_nufft2d_double *, FOURIER_SIZE_TYPE batch);
/* "table": 0 / 1.  Anything else: FOURIER_HIP_INVALID_ARGUMENT. */
int fourier_hip_nufft2d_set_option_float(FOURIER_STRUCT fourier_nufft2d_float *, const char *key, long long value);
int fourier_hip_nufft2d_set_option_double(FOURIER_STRUCT fourier_nufft2d_double *, const char *key, long long value);
/* "" for a NULL handle. */
const char *fourier_hip_nufft2d_describe_float(const FOURIER_STRUCT fourier_nufft2d_float *);
const char *fourier_hip_nufft2d_describe_double(const FOURIER_STRUCT fourier_nufft2d_double *);
int fourier_hip_nufft2d_last_status_float(const FOURIER_STRUCT fourier_nufft2d_float *);
int fourier_hip_nufft2d_last_status_double(const FOURIER_STRUCT fourier_nufft2d_double *);

/* ---------------- non-uniform FFT, 3-D, types 1 and 2 (extension; the reference has none) ----------
 * FINUFFT's 3-D type 1 and type 2 in C order with the points shared by the items of a batch.  A handle is created for n1 x n2 x n3
 * modes (each >= 1) and a requested accuracy eps; fourier_hip_nufft3d_set_points_* gives it M >= 0 points (x1_j, x2_j, x3_j), any
 * finite reals, taken modulo 2 pi per coordinate.  Coordinate d pairs with axis d of the mode array; k_d runs over
 * -floor(n_d/2) .. ceil(n_d/2) - 1.  With s = `sign`, +1 or -1 per call:
 *   to_modes  (type 1)   f[b][k1][k2][k3] = sum_j c[b][j] exp(i s (k1 x1_j + k2 x2_j + k3 x3_j))            rows of M in, items of n1 x n2 x n3 out
 *   to_points (type 2)   c[b][j] = sum_{k1,k2,k3} f[b][k1][k2][k3] exp(i s (k1 x1_j + k2 x2_j + k3 x3_j))   items of n1 x n2 x n3 in, rows of M out
 * on DEVICE memory, interleaved complex T, the last mode axis contiguous, item b at element offset b*M or b*n1*n2*n3.  `order` 0
 * stores all three axes with k ascending, 1 all three in FFT order (numpy's ifftshift over the three axes of order 0).  There is no
 * scale factor; to_points with sign s is the exact adjoint of to_modes with sign -s.
 * The algorithm is fourier_hip_nufft2d_*'s with one more axis: the same kernel phi with beta = 2.30 w, the same
 * w = ceil(log10(1 / eps)) + 1 clamped to 2 .. 8 (float) or 2 .. 16 (double), one w for all three axes; L_d is the smallest
 * 2^a 3^b 5^c >= max(2 n_d, 2 w); a point's weight on cell (i1, i2, i3) is the product of its three 1-D weights, and the
 * deconvolution factor is the product of three 1-D tables from the same quadrature.  to_modes spreads onto grid items of
 * L1 x L2 x L3 (a gather over the points, bucketed by their first cells of axes 1 and 2 and sorted by their axis-3 coordinate: no
 * atomics), transforms the rows of L3, then axis 2, then axis 1 in place (FFT for s = -1, UNSCALED_IFFT for s = +1), picks the
 * n1 x n2 x n3 modes and multiplies by 1 / phihat; to_points writes f / phihat into a zeroed grid, transforms and interpolates at
 * the points.  The relative L2 error of a call against the direct sum is about 3 x 10^(1 - w), plus the rounding of T.
 * fourier_hip_nufft3d_set_points_*: h_x1, h_x2 and h_x3 each point to m doubles on the HOST, for both precisions.  A set-up call like
 * fourier_hip_nufft2d_set_points_*: it waits for `stream`, sorts (stable: equal points keep the caller's order), uploads the tables
 * and waits again.  Besides seven arrays of m values the tables hold L1 L2 (L3 + 2w + 1) 32-bit indices, about half of one float grid
 * item and a quarter of a double one.  Calling it again replaces the points; m == 0 is valid (to_modes then writes zeros, to_points
 * writes nothing).  A NaN or infinite coordinate in any array, m > 2^31 - 1, m * 2 * sizeof(T) > 2^30, a NULL pointer with m > 0 or
 * one not aligned to 8 bytes give FOURIER_HIP_INVALID_ARGUMENT and leave the points as they were; so does an allocation or copy that
 * fails (the new tables replace the old ones only when all of them are complete).
 * A transform call before any set_points, sign other than +1 / -1, order other than 0 / 1, a NULL or misaligned (2*sizeof(T)) buffer
 * and ANY overlap of input and output give FOURIER_HIP_INVALID_ARGUMENT and write nothing.  batch == 0 is a successful no-op.
 * An n_d of 0, eps <= 0 or not finite, items of n1 * n2 * n3 modes above 2^30 bytes or a grid item above 2^31 bytes: create fails.
 * Stream-ordered on `stream` like fourier_hip_transform_batch_*.
 * Option "table" (fourier_hip_nufft3d_set_option_*): 0 = "nufft3d evaluated", the weights are evaluated in the two hot kernels with
 * the accurate exp and sqrt; 1 = "nufft3d tabulated", a set-up kernel writes the 3 x w x M weights once (at set_points, or at set_option
 * on the null stream when points are set) and the hot kernels read them.  The two routes agree to rounding.  The default is 0
 * ("Non-uniform FFT, 3-D").  fourier_hip_nufft3d_describe_* begins "nufft3d evaluated: " or "nufft3d
 * tabulated: ", then "w <w>, L <L1> x <L2> x <L3>, " and the descriptions of the row plan and of the axis-2 and axis-1 routes.
 * The plan owns a scratch of fine-grid items of at most 1 GiB (never less than one item) and walks larger batches in chunks; the first
 * call with a batch larger than any before allocates it unless fourier_hip_nufft3d_reserve_* was called for at least that batch.  No
 * atomics and a summation order fixed by the points: the result is the same on repetition.  A NULL handle gives
 * FOURIER_HIP_INVALID_ARGUMENT, 0 from fourier_hip_nufft3d_modes1_* / _modes2_* / _modes3_* / _points_* and "" from
 * fourier_hip_nufft3d_describe_*.  Handles are Send, not Sync, like the complex ones; status of the last call:
 * fourier_hip_nufft3d_last_status_*. */
struct fourier_nufft3d_float;
struct fourier_nufft3d_double;

/* NULL on failure (a parameter outside the ranges above included). */
struct fourier_nufft3d_float *fourier_hip_nufft3d_create_float(FOURIER_SIZE_TYPE n1, FOURIER_SIZE_TYPE n2, FOURIER_SIZE_TYPE n3,
                                                               double eps, int device);
struct fourier_nufft3d_double *fourier_hip_nufft3d_create_double(FOURIER_SIZE_TYPE n1, FOURIER_SIZE_TYPE n2, FOURIER_SIZE_TYPE n3,
                                                                 double eps, int device);
/* NULL is a no-op. */
void fourier_hip_nufft3d_destroy_float(FOURIER_STRUCT fourier_nufft3d_float *);
void fourier_hip_nufft3d_destroy_double(FOURIER_STRUCT fourier_nufft3d_double *);
/* n1, n2, n3, and the M of the last set_points (0 before any); 0 for a NULL handle. */
FOURIER_SIZE_TYPE fourier_hip_nufft3d_modes1_float(const FOURIER_STRUCT fourier_nufft3d_float *);
FOURIER_SIZE_TYPE fourier_hip_nufft3d_modes1_double(const FOURIER_STRUCT fourier_nufft3d_double *);
FOURIER_SIZE_TYPE fourier_hip_nufft3d_modes2_float(const FOURIER_STRUCT fourier_nufft3d_float *);
FOURIER_SIZE_TYPE fourier_hip_nufft3d_modes2_double(const FOURIER_STRUCT fourier_nufft3d_double *);
FOURIER_SIZE_TYPE fourier_hip_nufft3d_modes3_float(const FOURIER_STRUCT fourier_nufft3d_float *);
FOURIER_SIZE_TYPE fourier_hip_nufft3d_modes3_double(const FOURIER_STRUCT fourier_nufft3d_double *);
FOURIER_SIZE_TYPE fourier_hip_nufft3d_points_float(const FOURIER_STRUCT fourier_nufft3d_float *);
FOURIER_SIZE_TYPE fourier_hip_nufft3d_points_double(const FOURIER_STRUCT fourier_nufft3d_double *);
/* three arrays of m doubles on the host, for both precisions. */
int fourier_hip_nufft3d_set_points_float(FOURIER_STRUCT fourier_nufft3d_float *, const double *h_x1, const double *h_x2,
                                         const double *h_x3, FOURIER_SIZE_TYPE m, void *stream);
int fourier_hip_nufft3d_set_points_double(FOURIER_STRUCT fourier_nufft3d_double *, const double *h_x1, const double *h_x2,
                                          const double *h_x3, FOURIER_SIZE_TYPE m, void *stream);
int fourier_hip_nufft3d_to_modes_batch_float(const FOURIER_STRUCT fourier_nufft3d_float *, const void *d_in, void *d_out,
                                             FOURIER_SIZE_TYPE batch, int sign, int order, void *stream);
int fourier_hip_nufft3d_to_modes_batch_double(const FOURIER_STRUCT fourier_nufft3d_double *, const void *d_in, void *d_out,
                                              FOURIER_SIZE_TYPE batch, int sign, int order, void *stream);
int fourier_hip_nufft3d_to_points_batch_float(const FOURIER_STRUCT fourier_nufft3d_float *, const void *d_in, void *d_out,
                                              FOURIER_SIZE_TYPE batch, int sign, int order, void *stream);
int fourier_hip_nufft3d_to_points_batch_double(const FOURIER_STRUCT fourier_nufft3d_double *, const void *d_in, void *d_out,
                                               FOURIER_SIZE_TYPE batch, int sign, int order, void *stream);
int fourier_hip_nufft3d_reserve_float(const FOURIER_STRUCT fourier_nufft3d_float *, FOURIER_SIZE_TYPE batch);
int fourier_hip_nufft3d_reserve_double(const FOURIER_STRUCT fourier_nufft3d_double *, FOURIER_SIZE_TYPE batch);
/* "table": 0 / 1.  Anything else: FOURIER_HIP_INVALID_ARGUMENT. */
int fourier_hip_nufft3d_set_option_float(FOURIER_STRUCT fourier_nufft3d_float *, const char *key, long long value);
int fourier_hip_nufft3d_set_option_double(FOURIER_STRUCT fourier_nufft3d_double *, const char *key, long long value);
/* "" for a NULL handle. */
const char *fourier_hip_nufft3d_describe_float(const FOURIER_STRUCT fourier_nufft3d_float *);
const char *fourier_hip_nufft3d_describe_double(const FOURIER_STRUCT fourier_nufft3d_double *);
int fourier_hip_nufft3d_last_status_float(const FOURIER_STRUCT fourier_nufft3d_float *);
int fourier_hip_nufft3d_last_status_double(const FOURIER_STRUCT fourier_nufft3d_double *);

#ifdef __cplusplus
} /* extern "C" */
} /* namespace c */

/* Header-only C++ RAII wrapper, same shape as the reference's (fourier.h:64-128). */
enum class transform {
  fft = ::fourier::c::FOURIER_TRANSFORM_FFT,
  ifft = ::fourier::c::FOURIER_TRANSFORM_IFFT,
  unscaled_ifft = ::fourier::c::FOURIER_TRANSFORM_UNSCALED_IFFT,
  sqrt_scaled_fft = ::fourier::c::FOURIER_TRANSFORM_SQRT_SCALED_FFT,
  sqrt_scaled_ifft = ::fourier::c::FOURIER_TRANSFORM_SQRT_SCALED_IFFT,
};

template <typename T> struct fft;

#define FOURIER_DEFINE_CXX_WRAPPER(T, SUFFIX)                                                      \
  template <> struct fft<T> {                                                                      \
    explicit fft(std::size_t size)                                                                 \
        : impl(::fourier::c::fourier_create_##SUFFIX(size), ::fourier::c::fourier_destroy_##SUFFIX) {} \
    fft() = delete;                                                                                \
    fft(const fft &) = delete;                                                                     \
    fft(fft &&) = default;                                                                         \
    fft &operator=(const fft &) = delete;                                                          \
    fft &operator=(fft &&) = default;                                                              \
    ~fft() = default;                                                                              \
    void transform_in_place(::std::complex<T> *x, transform t) const {                             \
      ::fourier::c::fourier_transform_in_place_##SUFFIX(impl.get(), x, static_cast<int>(t));       \
    }                                                                                              \
    void transform(const ::std::complex<T> *in, ::std::complex<T> *out, transform t) const {       \
      ::fourier::c::fourier_transform_##SUFFIX(impl.get(), in, out, static_cast<int>(t));          \
    }                                                                                              \
    /* device-resident batched execution (extension) */                                           \
    int transform_batch_device(const void *d_in, void *d_out, std::size_t batch,               \
                               ::fourier::transform t,                                            \
                               void *stream = nullptr) const {                                     \
      return ::fourier::c::fourier_hip_transform_batch_##SUFFIX(impl.get(), d_in, d_out, batch,    \
                                                                static_cast<int>(t), stream);      \
    }                                                                                              \
    /* transform along the middle axis of an [outer][size][inner] array on device memory (extension) */ \
    int transform_axis_device(const void *d_in, void *d_out, std::size_t outer, std::size_t inner, \
                              ::fourier::transform t, void *stream = nullptr) const {              \
      return ::fourier::c::fourier_hip_transform_axis_##SUFFIX(impl.get(), d_in, d_out, outer, inner, \
                                                               static_cast<int>(t), stream);       \
    }                                                                                              \
    /* many transforms in host memory, streamed through the device (extension) */                 \
    int transform_batch_host(const ::std::complex<T> *in, ::std::complex<T> *out, std::size_t batch, \
                             ::fourier::transform t) const {                                       \
      return ::fourier::c::fourier_hip_transform_batch_host_##SUFFIX(impl.get(), in, out, batch,   \
                                                                     static_cast<int>(t));         \
    }                                                                                              \
    explicit operator bool() const { return static_cast<bool>(impl); }                             \
                                                                                                   \
  private:                                                                                         \
    ::std::unique_ptr<::fourier::c::fourier_fft_##SUFFIX, void (*)(::fourier::c::fourier_fft_##SUFFIX *)> impl; \
  };
FOURIER_DEFINE_CXX_WRAPPER(float, float)
FOURIER_DEFINE_CXX_WRAPPER(double, double)
#undef FOURIER_DEFINE_CXX_WRAPPER

/* real-input transforms on device memory (extension): fourier::real_fft<float> / <double> */
template <typename T> struct real_fft;

#define FOURIER_DEFINE_CXX_REAL_WRAPPER(T, SUFFIX)                                                 \
  template <> struct real_fft<T> {                                                                 \
    explicit real_fft(std::size_t size, int device = -1)                                           \
        : impl(::fourier::c::fourier_hip_real_create_##SUFFIX(size, device),                       \
               ::fourier::c::fourier_hip_real_destroy_##SUFFIX) {}                                 \
    real_fft() = delete;                                                                           \
    real_fft(const real_fft &) = delete;                                                           \
    real_fft(real_fft &&) = default;                                                               \
    real_fft &operator=(const real_fft &) = delete;                                                \
    real_fft &operator=(real_fft &&) = default;                                                    \
    ~real_fft() = default;                                                                         \
    std::size_t size() const { return ::fourier::c::fourier_hip_real_size_##SUFFIX(impl.get()); }  \
    /* N reals per row -> N/2+1 complex per row */                                                 \
    int forward_batch_device(const void *d_in, void *d_out, std::size_t batch,                     \
                             ::fourier::transform t = ::fourier::transform::fft,                   \
                             void *stream = nullptr) const {                                       \
      return ::fourier::c::fourier_hip_real_forward_batch_##SUFFIX(impl.get(), d_in, d_out, batch, \
                                                                   static_cast<int>(t), stream);   \
    }                                                                                              \
    /* N/2+1 complex per row -> N reals per row */                                                 \
    int inverse_batch_device(const void *d_in, void *d_out, std::size_t batch,                     \
                             ::fourier::transform t = ::fourier::transform::ifft,                  \
                             void *stream = nullptr) const {                                       \
      return ::fourier::c::fourier_hip_real_inverse_batch_##SUFFIX(impl.get(), d_in, d_out, batch, \
                                                                   static_cast<int>(t), stream);   \
    }                                                                                              \
    int reserve(std::size_t batch) const {                                                         \
      return ::fourier::c::fourier_hip_real_reserve_##SUFFIX(impl.get(), batch);                   \
    }                                                                                              \
    explicit operator bool() const { return static_cast<bool>(impl); }                             \
                                                                                                   \
  private:                                                                                         \
    ::std::unique_ptr<::fourier::c::fourier_real_fft_##SUFFIX,                                     \
                      void (*)(::fourier::c::fourier_real_fft_##SUFFIX *)> impl;                   \
  };
FOURIER_DEFINE_CXX_REAL_WRAPPER(float, float)
FOURIER_DEFINE_CXX_REAL_WRAPPER(double, double)
#undef FOURIER_DEFINE_CXX_REAL_WRAPPER

/* DCT / DST of types II and III on device memory (extension): fourier::r2r<float> / <double> */
enum class r2r_kind {
  dct2 = ::fourier::c::FOURIER_R2R_DCT2,
  dct3 = ::fourier::c::FOURIER_R2R_DCT3,
  dst2 = ::fourier::c::FOURIER_R2R_DST2,
  dst3 = ::fourier::c::FOURIER_R2R_DST3,
};
enum class r2r_norm {
  backward = ::fourier::c::FOURIER_R2R_NORM_BACKWARD,
  ortho = ::fourier::c::FOURIER_R2R_NORM_ORTHO,
  forward = ::fourier::c::FOURIER_R2R_NORM_FORWARD,
};
template <typename T> struct r2r;

#define FOURIER_DEFINE_CXX_R2R_WRAPPER(T, SUFFIX)                                                  \
  template <> struct r2r<T> {                                                                      \
    explicit r2r(std::size_t size, int device = -1)                                                \
        : impl(::fourier::c::fourier_hip_r2r_create_##SUFFIX(size, device),                        \
               ::fourier::c::fourier_hip_r2r_destroy_##SUFFIX) {}                                  \
    r2r() = delete;                                                                                \
    r2r(const r2r &) = delete;                                                                     \
    r2r(r2r &&) = default;                                                                         \
    r2r &operator=(const r2r &) = delete;                                                          \
    r2r &operator=(r2r &&) = default;                                                              \
    ~r2r() = default;                                                                              \
    std::size_t size() const { return ::fourier::c::fourier_hip_r2r_size_##SUFFIX(impl.get()); }   \
    /* N reals per row -> N reals per row; d_out may be d_in */                                    \
    int transform_batch_device(const void *d_in, void *d_out, std::size_t batch, r2r_kind kind,    \
                               r2r_norm norm = r2r_norm::backward, void *stream = nullptr) const { \
      return ::fourier::c::fourier_hip_r2r_transform_batch_##SUFFIX(                               \
          impl.get(), d_in, d_out, batch, static_cast<int>(kind), static_cast<int>(norm), stream); \
    }                                                                                              \
    int reserve(std::size_t batch) const {                                                         \
      return ::fourier::c::fourier_hip_r2r_reserve_##SUFFIX(impl.get(), batch);                    \
    }                                                                                              \
    const char *describe() const { return ::fourier::c::fourier_hip_r2r_describe_##SUFFIX(impl.get()); } \
    int last_status() const { return ::fourier::c::fourier_hip_r2r_last_status_##SUFFIX(impl.get()); } \
    explicit operator bool() const { return static_cast<bool>(impl); }                             \
                                                                                                   \
  private:                                                                                         \
    ::std::unique_ptr<::fourier::c::fourier_r2r_##SUFFIX,                                          \
                      void (*)(::fourier::c::fourier_r2r_##SUFFIX *)> impl;                        \
  };
FOURIER_DEFINE_CXX_R2R_WRAPPER(float, float)
FOURIER_DEFINE_CXX_R2R_WRAPPER(double, double)
#undef FOURIER_DEFINE_CXX_R2R_WRAPPER

/* short-time Fourier transform on device memory (extension): fourier::stft<float> / <double> */
enum class stft_pad {
  none = ::fourier::c::FOURIER_STFT_PAD_NONE,
  reflect = ::fourier::c::FOURIER_STFT_PAD_REFLECT,
  zero = ::fourier::c::FOURIER_STFT_PAD_ZERO,
};
template <typename T> struct stft;

#define FOURIER_DEFINE_CXX_STFT_WRAPPER(T, SUFFIX)                                                 \
  template <> struct stft<T> {                                                                     \
    stft(std::size_t n_fft, std::size_t hop, std::size_t win_length, stft_pad pad = stft_pad::reflect, int device = -1) \
        : impl(::fourier::c::fourier_hip_stft_create_##SUFFIX(n_fft, hop, win_length, static_cast<int>(pad), device), \
               ::fourier::c::fourier_hip_stft_destroy_##SUFFIX) {}                                 \
    stft() = delete;                                                                               \
    stft(const stft &) = delete;                                                                   \
    stft(stft &&) = default;                                                                       \
    stft &operator=(const stft &) = delete;                                                        \
    stft &operator=(stft &&) = default;                                                            \
    ~stft() = default;                                                                             \
    std::size_t n_fft() const { return ::fourier::c::fourier_hip_stft_n_fft_##SUFFIX(impl.get()); } \
    std::size_t hop() const { return ::fourier::c::fourier_hip_stft_hop_##SUFFIX(impl.get()); }    \
    std::size_t win_length() const { return ::fourier::c::fourier_hip_stft_win_length_##SUFFIX(impl.get()); } \
    std::size_t bins() const { return ::fourier::c::fourier_hip_stft_bins_##SUFFIX(impl.get()); }  \
    std::size_t frames(std::size_t length) const {                                                 \
      return ::fourier::c::fourier_hip_stft_frames_##SUFFIX(impl.get(), length);                   \
    }                                                                                              \
    /* win_length reals on the device; nullptr: all ones */                                        \
    int set_window(const void *d_window, void *stream = nullptr) {                                 \
      return ::fourier::c::fourier_hip_stft_set_window_##SUFFIX(impl.get(), d_window, stream);     \
    }                                                                                              \
    /* batch rows of `length` reals -> batch x frames x bins complex, frame-major */               \
    int forward_device(const void *d_in, void *d_out, std::size_t length, std::size_t batch,       \
                       bool normalized = false, void *stream = nullptr) const {                    \
      return ::fourier::c::fourier_hip_stft_forward_##SUFFIX(impl.get(), d_in, d_out, length, batch, \
                                                             normalized ? 1 : 0, stream);          \
    }                                                                                              \
    /* batch x frames x bins complex -> batch rows of `length` reals */                            \
    int inverse_device(const void *d_in, void *d_out, std::size_t frames, std::size_t length,      \
                       std::size_t batch, bool normalized = false, void *stream = nullptr) const { \
      return ::fourier::c::fourier_hip_stft_inverse_##SUFFIX(impl.get(), d_in, d_out, frames, length, \
                                                             batch, normalized ? 1 : 0, stream);   \
    }                                                                                              \
    int reserve(std::size_t length, std::size_t batch) const {                                     \
      return ::fourier::c::fourier_hip_stft_reserve_##SUFFIX(impl.get(), length, batch);           \
    }                                                                                              \
    int set_option(const char *key, long long value) {                                             \
      return ::fourier::c::fourier_hip_stft_set_option_##SUFFIX(impl.get(), key, value);           \
    }                                                                                              \
    const char *describe() const { return ::fourier::c::fourier_hip_stft_describe_##SUFFIX(impl.get()); } \
    int last_status() const { return ::fourier::c::fourier_hip_stft_last_status_##SUFFIX(impl.get()); } \
    explicit operator bool() const { return static_cast<bool>(impl); }                             \
                                                                                                   \
  private:                                                                                         \
    ::std::unique_ptr<::fourier::c::fourier_stft_##SUFFIX,                                         \
                      void (*)(::fourier::c::fourier_stft_##SUFFIX *)> impl;                       \
  };
FOURIER_DEFINE_CXX_STFT_WRAPPER(float, float)
FOURIER_DEFINE_CXX_STFT_WRAPPER(double, double)
#undef FOURIER_DEFINE_CXX_STFT_WRAPPER

/* modified discrete cosine transform on device memory (extension): fourier::mdct<float> / <double> */
template <typename T> struct mdct;

#define FOURIER_DEFINE_CXX_MDCT_WRAPPER(T, SUFFIX)                                                 \
  template <> struct mdct<T> {                                                                     \
    explicit mdct(std::size_t n, bool center = true, int device = -1)                              \
        : impl(::fourier::c::fourier_hip_mdct_create_##SUFFIX(n, center ? 1 : 0, device),          \
               ::fourier::c::fourier_hip_mdct_destroy_##SUFFIX) {}                                 \
    mdct() = delete;                                                                               \
    mdct(const mdct &) = delete;                                                                   \
    mdct(mdct &&) = default;                                                                       \
    mdct &operator=(const mdct &) = delete;                                                        \
    mdct &operator=(mdct &&) = default;                                                            \
    ~mdct() = default;                                                                             \
    std::size_t size() const { return ::fourier::c::fourier_hip_mdct_size_##SUFFIX(impl.get()); }  \
    std::size_t frames(std::size_t length) const {                                                 \
      return ::fourier::c::fourier_hip_mdct_frames_##SUFFIX(impl.get(), length);                   \
    }                                                                                              \
    /* 2n reals on the device; nullptr: the sine window */                                         \
    int set_window(const void *d_window, void *stream = nullptr) {                                 \
      return ::fourier::c::fourier_hip_mdct_set_window_##SUFFIX(impl.get(), d_window, stream);     \
    }                                                                                              \
    /* batch rows of `length` reals -> batch x frames x n reals, frame-major */                    \
    int forward_device(const void *d_in, void *d_out, std::size_t length, std::size_t batch,       \
                       bool normalized = false, void *stream = nullptr) const {                    \
      return ::fourier::c::fourier_hip_mdct_forward_##SUFFIX(impl.get(), d_in, d_out, length, batch, \
                                                             normalized ? 1 : 0, stream);          \
    }                                                                                              \
    /* batch x frames x n reals -> batch rows of `length` reals */                                 \
    int inverse_device(const void *d_in, void *d_out, std::size_t frames, std::size_t length,      \
                       std::size_t batch, bool normalized = false, void *stream = nullptr) const { \
      return ::fourier::c::fourier_hip_mdct_inverse_##SUFFIX(impl.get(), d_in, d_out, frames, length, \
                                                             batch, normalized ? 1 : 0, stream);   \
    }                                                                                              \
    int reserve(std::size_t length, std::size_t batch) const {                                     \
      return ::fourier::c::fourier_hip_mdct_reserve_##SUFFIX(impl.get(), length, batch);           \
    }                                                                                              \
    int set_option(const char *key, long long value) {                                             \
      return ::fourier::c::fourier_hip_mdct_set_option_##SUFFIX(impl.get(), key, value);           \
    }                                                                                              \
    const char *describe() const { return ::fourier::c::fourier_hip_mdct_describe_##SUFFIX(impl.get()); } \
    int last_status() const { return ::fourier::c::fourier_hip_mdct_last_status_##SUFFIX(impl.get()); } \
    explicit operator bool() const { return static_cast<bool>(impl); }                             \
                                                                                                   \
  private:                                                                                         \
    ::std::unique_ptr<::fourier::c::fourier_mdct_##SUFFIX,                                         \
                      void (*)(::fourier::c::fourier_mdct_##SUFFIX *)> impl;                       \
  };
FOURIER_DEFINE_CXX_MDCT_WRAPPER(float, float)
FOURIER_DEFINE_CXX_MDCT_WRAPPER(double, double)
#undef FOURIER_DEFINE_CXX_MDCT_WRAPPER

/* power spectrogram and Welch average on device memory (extension): fourier::spectrogram<float> / <double>; the pad modes are stft_pad */
template <typename T> struct spectrogram;

#define FOURIER_DEFINE_CXX_SPECTROGRAM_WRAPPER(T, SUFFIX)                                          \
  template <> struct spectrogram<T> {                                                              \
    spectrogram(std::size_t n_fft, std::size_t hop, std::size_t win_length, stft_pad pad = stft_pad::reflect, int device = -1) \
        : impl(::fourier::c::fourier_hip_spectrogram_create_##SUFFIX(n_fft, hop, win_length, static_cast<int>(pad), device), \
               ::fourier::c::fourier_hip_spectrogram_destroy_##SUFFIX) {}                          \
    spectrogram() = delete;                                                                        \
    spectrogram(const spectrogram &) = delete;                                                     \
    spectrogram(spectrogram &&) = default;                                                         \
    spectrogram &operator=(const spectrogram &) = delete;                                          \
    spectrogram &operator=(spectrogram &&) = default;                                              \
    ~spectrogram() = default;                                                                      \
    std::size_t n_fft() const { return ::fourier::c::fourier_hip_spectrogram_n_fft_##SUFFIX(impl.get()); } \
    std::size_t hop() const { return ::fourier::c::fourier_hip_spectrogram_hop_##SUFFIX(impl.get()); } \
    std::size_t win_length() const { return ::fourier::c::fourier_hip_spectrogram_win_length_##SUFFIX(impl.get()); } \
    std::size_t bins() const { return ::fourier::c::fourier_hip_spectrogram_bins_##SUFFIX(impl.get()); } \
    std::size_t frames(std::size_t length) const {                                                 \
      return ::fourier::c::fourier_hip_spectrogram_frames_##SUFFIX(impl.get(), length);            \
    }                                                                                              \
    /* win_length reals on the device; nullptr: all ones */                                        \
    int set_window(const void *d_window, void *stream = nullptr) {                                 \
      return ::fourier::c::fourier_hip_spectrogram_set_window_##SUFFIX(impl.get(), d_window, stream); \
    }                                                                                              \
    /* batch rows of `length` reals -> batch x frames x bins reals |X|^power, frame-major */       \
    int forward_device(const void *d_in, void *d_out, std::size_t length, std::size_t batch,       \
                       int power = ::fourier::c::FOURIER_SPECTROGRAM_POWER, bool normalized = false, \
                       void *stream = nullptr) const {                                             \
      return ::fourier::c::fourier_hip_spectrogram_forward_##SUFFIX(impl.get(), d_in, d_out, length, batch, \
                                                                    power, normalized ? 1 : 0, stream); \
    }                                                                                              \
    /* batch rows of `length` reals -> batch x bins reals scale c_k / frames sum_f |X|^2 (no detrending) */ \
    int welch_device(const void *d_in, void *d_out, std::size_t length, std::size_t batch,         \
                     bool onesided_fold = true, double scale = 1.0, void *stream = nullptr) const { \
      return ::fourier::c::fourier_hip_spectrogram_welch_##SUFFIX(impl.get(), d_in, d_out, length, batch, \
                                                                  onesided_fold ? 1 : 0, scale, stream); \
    }                                                                                              \
    int reserve(std::size_t length, std::size_t batch) const {                                     \
      return ::fourier::c::fourier_hip_spectrogram_reserve_##SUFFIX(impl.get(), length, batch);    \
    }                                                                                              \
    int set_option(const char *key, long long value) {                                             \
      return ::fourier::c::fourier_hip_spectrogram_set_option_##SUFFIX(impl.get(), key, value);    \
    }                                                                                              \
    const char *describe() const { return ::fourier::c::fourier_hip_spectrogram_describe_##SUFFIX(impl.get()); } \
    int last_status() const { return ::fourier::c::fourier_hip_spectrogram_last_status_##SUFFIX(impl.get()); } \
    explicit operator bool() const { return static_cast<bool>(impl); }                             \
                                                                                                   \
  private:                                                                                         \
    ::std::unique_ptr<::fourier::c::fourier_spectrogram_##SUFFIX,                                  \
                      void (*)(::fourier::c::fourier_spectrogram_##SUFFIX *)> impl;                \
  };
FOURIER_DEFINE_CXX_SPECTROGRAM_WRAPPER(float, float)
FOURIER_DEFINE_CXX_SPECTROGRAM_WRAPPER(double, double)
#undef FOURIER_DEFINE_CXX_SPECTROGRAM_WRAPPER

/* cross-spectral density and coherence of two signals on device memory (extension): fourier::csd<float> / <double>; the pad modes are stft_pad */
template <typename T> struct csd;

#define FOURIER_DEFINE_CXX_CSD_WRAPPER(T, SUFFIX)                                                  \
  template <> struct csd<T> {                                                                      \
    csd(std::size_t n_fft, std::size_t hop, std::size_t win_length, stft_pad pad = stft_pad::reflect, int device = -1) \
        : impl(::fourier::c::fourier_hip_csd_create_##SUFFIX(n_fft, hop, win_length, static_cast<int>(pad), device), \
               ::fourier::c::fourier_hip_csd_destroy_##SUFFIX) {}                                  \
    csd() = delete;                                                                                \
    csd(const csd &) = delete;                                                                     \
    csd(csd &&) = default;                                                                         \
    csd &operator=(const csd &) = delete;                                                          \
    csd &operator=(csd &&) = default;                                                              \
    ~csd() = default;                                                                              \
    std::size_t n_fft() const { return ::fourier::c::fourier_hip_csd_n_fft_##SUFFIX(impl.get()); } \
    std::size_t hop() const { return ::fourier::c::fourier_hip_csd_hop_##SUFFIX(impl.get()); }     \
    std::size_t win_length() const { return ::fourier::c::fourier_hip_csd_win_length_##SUFFIX(impl.get()); } \
    std::size_t bins() const { return ::fourier::c::fourier_hip_csd_bins_##SUFFIX(impl.get()); }   \
    std::size_t frames(std::size_t length) const {                                                 \
      return ::fourier::c::fourier_hip_csd_frames_##SUFFIX(impl.get(), length);                    \
    }                                                                                              \
    /* win_length reals on the device; nullptr: all ones */                                        \
    int set_window(const void *d_window, void *stream = nullptr) {                                 \
      return ::fourier::c::fourier_hip_csd_set_window_##SUFFIX(impl.get(), d_window, stream);      \
    }                                                                                              \
    /* batch rows of `length` reals each -> batch x bins complex scale c_k / frames sum_f conj(X) Y (no detrending) */ \
    int csd_device(const void *d_x, const void *d_y, void *d_out, std::size_t length, std::size_t batch, \
                   bool onesided_fold = true, double scale = 1.0, void *stream = nullptr) const {  \
      return ::fourier::c::fourier_hip_csd_csd_##SUFFIX(impl.get(), d_x, d_y, d_out, length, batch, \
                                                        onesided_fold ? 1 : 0, scale, stream);     \
    }                                                                                              \
    /* ... -> batch x bins reals |sum_f conj(X) Y|^2 / (sum_f |X|^2 sum_f |Y|^2) */                \
    int coherence_device(const void *d_x, const void *d_y, void *d_out, std::size_t length, std::size_t batch, \
                         void *stream = nullptr) const {                                           \
      return ::fourier::c::fourier_hip_csd_coherence_##SUFFIX(impl.get(), d_x, d_y, d_out, length, batch, stream); \
    }                                                                                              \
    int reserve(std::size_t length, std::size_t batch) const {                                     \
      return ::fourier::c::fourier_hip_csd_reserve_##SUFFIX(impl.get(), length, batch);            \
    }                                                                                              \
    int set_option(const char *key, long long value) {                                             \
      return ::fourier::c::fourier_hip_csd_set_option_##SUFFIX(impl.get(), key, value);            \
    }                                                                                              \
    const char *describe() const { return ::fourier::c::fourier_hip_csd_describe_##SUFFIX(impl.get()); } \
    int last_status() const { return ::fourier::c::fourier_hip_csd_last_status_##SUFFIX(impl.get()); } \
    explicit operator bool() const { return static_cast<bool>(impl); }                             \
                                                                                                   \
  private:                                                                                         \
    ::std::unique_ptr<::fourier::c::fourier_csd_##SUFFIX,                                          \
                      void (*)(::fourier::c::fourier_csd_##SUFFIX *)> impl;                        \
  };
FOURIER_DEFINE_CXX_CSD_WRAPPER(float, float)
FOURIER_DEFINE_CXX_CSD_WRAPPER(double, double)
#undef FOURIER_DEFINE_CXX_CSD_WRAPPER

/* band-energy (mel) spectrogram on device memory (extension): fourier::bandspec<float> / <double>; the pad modes are stft_pad, the powers spectrogram_power's values */
template <typename T> struct bandspec;

#define FOURIER_DEFINE_CXX_BANDSPEC_WRAPPER(T, SUFFIX)                                             \
  template <> struct bandspec<T> {                                                                 \
    bandspec(std::size_t n_fft, std::size_t hop, std::size_t win_length, std::size_t bands, stft_pad pad = stft_pad::reflect, \
             int device = -1)                                                                      \
        : impl(::fourier::c::fourier_hip_bandspec_create_##SUFFIX(n_fft, hop, win_length, static_cast<int>(pad), bands, device), \
               ::fourier::c::fourier_hip_bandspec_destroy_##SUFFIX) {}                             \
    bandspec() = delete;                                                                           \
    bandspec(const bandspec &) = delete;                                                           \
    bandspec(bandspec &&) = default;                                                               \
    bandspec &operator=(const bandspec &) = delete;                                                \
    bandspec &operator=(bandspec &&) = default;                                                    \
    ~bandspec() = default;                                                                         \
    std::size_t n_fft() const { return ::fourier::c::fourier_hip_bandspec_n_fft_##SUFFIX(impl.get()); } \
    std::size_t hop() const { return ::fourier::c::fourier_hip_bandspec_hop_##SUFFIX(impl.get()); } \
    std::size_t win_length() const { return ::fourier::c::fourier_hip_bandspec_win_length_##SUFFIX(impl.get()); } \
    std::size_t bins() const { return ::fourier::c::fourier_hip_bandspec_bins_##SUFFIX(impl.get()); } \
    std::size_t bands() const { return ::fourier::c::fourier_hip_bandspec_bands_##SUFFIX(impl.get()); } \
    std::size_t frames(std::size_t length) const {                                                 \
      return ::fourier::c::fourier_hip_bandspec_frames_##SUFFIX(impl.get(), length);               \
    }                                                                                              \
    /* win_length reals on the device; nullptr: all ones */                                        \
    int set_window(const void *d_window, void *stream = nullptr) {                                 \
      return ::fourier::c::fourier_hip_bandspec_set_window_##SUFFIX(impl.get(), d_window, stream); \
    }                                                                                              \
    /* bands x bins reals on the HOST, row-major */                                                \
    int set_bands(const T *h_matrix, void *stream = nullptr) {                                     \
      return ::fourier::c::fourier_hip_bandspec_set_bands_##SUFFIX(impl.get(), h_matrix, stream);  \
    }                                                                                              \
    /* batch rows of `length` reals -> batch x frames x bands reals; power: 1 = |X|, 2 = |X|^2; log_mult != 0: log_mult ln(max(., log_floor)) */ \
    int forward_device(const void *d_in, void *d_out, std::size_t length, std::size_t batch, int power = 2, \
                       bool normalized = false, double log_mult = 0.0, double log_floor = 0.0, void *stream = nullptr) const { \
      return ::fourier::c::fourier_hip_bandspec_forward_##SUFFIX(impl.get(), d_in, d_out, length, batch, power, \
                                                                 normalized ? 1 : 0, log_mult, log_floor, stream); \
    }                                                                                              \
    int reserve(std::size_t length, std::size_t batch) const {                                     \
      return ::fourier::c::fourier_hip_bandspec_reserve_##SUFFIX(impl.get(), length, batch);       \
    }                                                                                              \
    int set_option(const char *key, long long value) {                                             \
      return ::fourier::c::fourier_hip_bandspec_set_option_##SUFFIX(impl.get(), key, value);       \
    }                                                                                              \
    const char *describe() const { return ::fourier::c::fourier_hip_bandspec_describe_##SUFFIX(impl.get()); } \
    int last_status() const { return ::fourier::c::fourier_hip_bandspec_last_status_##SUFFIX(impl.get()); } \
    explicit operator bool() const { return static_cast<bool>(impl); }                             \
                                                                                                   \
  private:                                                                                         \
    ::std::unique_ptr<::fourier::c::fourier_bandspec_##SUFFIX,                                     \
                      void (*)(::fourier::c::fourier_bandspec_##SUFFIX *)> impl;                   \
  };
FOURIER_DEFINE_CXX_BANDSPEC_WRAPPER(float, float)
FOURIER_DEFINE_CXX_BANDSPEC_WRAPPER(double, double)
#undef FOURIER_DEFINE_CXX_BANDSPEC_WRAPPER

/* analytic signal and envelope of real rows on device memory (extension): fourier::hilbert<float> / <double> */
template <typename T> struct hilbert;

#define FOURIER_DEFINE_CXX_HILBERT_WRAPPER(T, SUFFIX)                                              \
  template <> struct hilbert<T> {                                                                  \
    explicit hilbert(std::size_t size, int device = -1)                                            \
        : impl(::fourier::c::fourier_hip_hilbert_create_##SUFFIX(size, device),                    \
               ::fourier::c::fourier_hip_hilbert_destroy_##SUFFIX) {}                              \
    hilbert() = delete;                                                                            \
    hilbert(const hilbert &) = delete;                                                             \
    hilbert(hilbert &&) = default;                                                                 \
    hilbert &operator=(const hilbert &) = delete;                                                  \
    hilbert &operator=(hilbert &&) = default;                                                      \
    ~hilbert() = default;                                                                          \
    std::size_t size() const { return ::fourier::c::fourier_hip_hilbert_size_##SUFFIX(impl.get()); }\
    /* `batch` rows of N reals -> rows of N complex values z (no overlap) */                       \
    int analytic_device(const void *d_in, void *d_out, std::size_t batch, void *stream = nullptr) const {\
      return ::fourier::c::fourier_hip_hilbert_analytic_##SUFFIX(impl.get(), d_in, d_out, batch, stream);\
    }                                                                                              \
    /* ... -> rows of N reals |z| (d_out may be d_in) */                                           \
    int envelope_device(const void *d_in, void *d_out, std::size_t batch, void *stream = nullptr) const {\
      return ::fourier::c::fourier_hip_hilbert_envelope_##SUFFIX(impl.get(), d_in, d_out, batch, stream);\
    }                                                                                              \
    int reserve(std::size_t batch) const {                                                         \
      return ::fourier::c::fourier_hip_hilbert_reserve_##SUFFIX(impl.get(), batch);                \
    }                                                                                              \
    int set_option(const char *key, long long value) {                                             \
      return ::fourier::c::fourier_hip_hilbert_set_option_##SUFFIX(impl.get(), key, value);        \
    }                                                                                              \
    const char *describe() const { return ::fourier::c::fourier_hip_hilbert_describe_##SUFFIX(impl.get()); }\
    int last_status() const { return ::fourier::c::fourier_hip_hilbert_last_status_##SUFFIX(impl.get()); }\
    explicit operator bool() const { return static_cast<bool>(impl); }                             \
                                                                                                   \
  private:                                                                                         \
    ::std::unique_ptr<::fourier::c::fourier_hilbert_##SUFFIX,                                      \
                      void (*)(::fourier::c::fourier_hilbert_##SUFFIX *)> impl;                    \
  };
FOURIER_DEFINE_CXX_HILBERT_WRAPPER(float, float)
FOURIER_DEFINE_CXX_HILBERT_WRAPPER(double, double)
#undef FOURIER_DEFINE_CXX_HILBERT_WRAPPER

/* pairwise cross-correlation and GCC-PHAT on device memory (extension): fourier::xcorr<float> / <double> */
template <typename T> struct xcorr;

#define FOURIER_DEFINE_CXX_XCORR_WRAPPER(T, SUFFIX)                                                \
  template <> struct xcorr<T> {                                                                    \
    xcorr(std::size_t size, std::size_t length, long long lag_first, std::size_t lags,             \
          bool real_data = true, int device = -1)                                                  \
        : impl(::fourier::c::fourier_hip_xcorr_create_##SUFFIX(size, length, lag_first, lags,      \
                                                               real_data ? 1 : 0, device),        \
               ::fourier::c::fourier_hip_xcorr_destroy_##SUFFIX) {}                                \
    xcorr() = delete;                                                                              \
    xcorr(const xcorr &) = delete;                                                                 \
    xcorr(xcorr &&) = default;                                                                     \
    xcorr &operator=(const xcorr &) = delete;                                                      \
    xcorr &operator=(xcorr &&) = default;                                                          \
    ~xcorr() = default;                                                                            \
    std::size_t size() const { return ::fourier::c::fourier_hip_xcorr_size_##SUFFIX(impl.get()); } \
    std::size_t length() const { return ::fourier::c::fourier_hip_xcorr_length_##SUFFIX(impl.get()); }\
    std::size_t lags() const { return ::fourier::c::fourier_hip_xcorr_lags_##SUFFIX(impl.get()); } \
    /* `batch` rows of n values at d_x and d_y (which may be the same) -> rows of lags values (no overlap) */\
    int correlate_device(const void *d_x, const void *d_y, void *d_out, std::size_t batch,         \
                         void *stream = nullptr) const {                                           \
      return ::fourier::c::fourier_hip_xcorr_correlate_##SUFFIX(impl.get(), d_x, d_y, d_out, batch, stream);\
    }                                                                                              \
    int reserve(std::size_t batch) const {                                                         \
      return ::fourier::c::fourier_hip_xcorr_reserve_##SUFFIX(impl.get(), batch);                  \
    }                                                                                              \
    int set_option(const char *key, long long value) {                                             \
      return ::fourier::c::fourier_hip_xcorr_set_option_##SUFFIX(impl.get(), key, value);          \
    }                                                                                              \
    const char *describe() const { return ::fourier::c::fourier_hip_xcorr_describe_##SUFFIX(impl.get()); }\
    int last_status() const { return ::fourier::c::fourier_hip_xcorr_last_status_##SUFFIX(impl.get()); }\
    explicit operator bool() const { return static_cast<bool>(impl); }                             \
                                                                                                   \
  private:                                                                                         \
    ::std::unique_ptr<::fourier::c::fourier_xcorr_##SUFFIX,                                        \
                      void (*)(::fourier::c::fourier_xcorr_##SUFFIX *)> impl;                      \
  };
FOURIER_DEFINE_CXX_XCORR_WRAPPER(float, float)
FOURIER_DEFINE_CXX_XCORR_WRAPPER(double, double)
#undef FOURIER_DEFINE_CXX_XCORR_WRAPPER

/* fractional delay and delay-and-sum on device memory (extension): fourier::delay<float> / <double> */
template <typename T> struct delay;

#define FOURIER_DEFINE_CXX_DELAY_WRAPPER(T, SUFFIX)                                                \
  template <> struct delay<T> {                                                                    \
    delay(std::size_t size, std::size_t length, std::size_t channels = 1, bool real_data = true,   \
          int device = -1)                                                                         \
        : impl(::fourier::c::fourier_hip_delay_create_##SUFFIX(size, length, channels,             \
                                                               real_data ? 1 : 0, device),        \
               ::fourier::c::fourier_hip_delay_destroy_##SUFFIX) {}                                \
    delay() = delete;                                                                              \
    delay(const delay &) = delete;                                                                 \
    delay(delay &&) = default;                                                                     \
    delay &operator=(const delay &) = delete;                                                      \
    delay &operator=(delay &&) = default;                                                          \
    ~delay() = default;                                                                            \
    std::size_t size() const { return ::fourier::c::fourier_hip_delay_size_##SUFFIX(impl.get()); } \
    std::size_t length() const { return ::fourier::c::fourier_hip_delay_length_##SUFFIX(impl.get()); }\
    std::size_t channels() const { return ::fourier::c::fourier_hip_delay_channels_##SUFFIX(impl.get()); }\
    /* `batch` rows of n values, `batch` delays, `batch` weights or nullptr -> batch / channels rows */\
    int apply_device(const void *d_in, const void *d_delays, const void *d_weights, void *d_out,   \
                     std::size_t batch, void *stream = nullptr) const {                            \
      return ::fourier::c::fourier_hip_delay_apply_##SUFFIX(impl.get(), d_in, d_delays, d_weights, d_out, batch, stream);\
    }                                                                                              \
    int reserve(std::size_t batch) const {                                                         \
      return ::fourier::c::fourier_hip_delay_reserve_##SUFFIX(impl.get(), batch);                  \
    }                                                                                              \
    int set_option(const char *key, long long value) {                                             \
      return ::fourier::c::fourier_hip_delay_set_option_##SUFFIX(impl.get(), key, value);          \
    }                                                                                              \
    const char *describe() const { return ::fourier::c::fourier_hip_delay_describe_##SUFFIX(impl.get()); }\
    int last_status() const { return ::fourier::c::fourier_hip_delay_last_status_##SUFFIX(impl.get()); }\
    explicit operator bool() const { return static_cast<bool>(impl); }                             \
                                                                                                   \
  private:                                                                                         \
    ::std::unique_ptr<::fourier::c::fourier_delay_##SUFFIX,                                        \
                      void (*)(::fourier::c::fourier_delay_##SUFFIX *)> impl;                      \
  };
FOURIER_DEFINE_CXX_DELAY_WRAPPER(float, float)
FOURIER_DEFINE_CXX_DELAY_WRAPPER(double, double)
#undef FOURIER_DEFINE_CXX_DELAY_WRAPPER

/* real cepstrum (mode 0) and minimum-phase reconstruction (mode 1) on device memory (extension): fourier::cepstrum<float> / <double> */
template <typename T> struct cepstrum;

#define FOURIER_DEFINE_CXX_CEPSTRUM_WRAPPER(T, SUFFIX)                                             \
  template <> struct cepstrum<T> {                                                                 \
    cepstrum(std::size_t size, std::size_t length, std::size_t outputs, int mode = 0,              \
             int device = -1)                                                                      \
        : impl(::fourier::c::fourier_hip_cepstrum_create_##SUFFIX(size, length, outputs, mode, device),\
               ::fourier::c::fourier_hip_cepstrum_destroy_##SUFFIX) {}                             \
    cepstrum() = delete;                                                                           \
    cepstrum(const cepstrum &) = delete;                                                           \
    cepstrum(cepstrum &&) = default;                                                               \
    cepstrum &operator=(const cepstrum &) = delete;                                                \
    cepstrum &operator=(cepstrum &&) = default;                                                    \
    ~cepstrum() = default;                                                                         \
    std::size_t size() const { return ::fourier::c::fourier_hip_cepstrum_size_##SUFFIX(impl.get()); }\
    std::size_t length() const { return ::fourier::c::fourier_hip_cepstrum_length_##SUFFIX(impl.get()); }\
    std::size_t outputs() const { return ::fourier::c::fourier_hip_cepstrum_outputs_##SUFFIX(impl.get()); }\
    int mode() const { return ::fourier::c::fourier_hip_cepstrum_mode_##SUFFIX(impl.get()); }      \
    /* `batch` rows of size() reals -> `batch` rows of outputs() reals */                          \
    int apply_device(const void *d_in, void *d_out, std::size_t batch, double log_mult = 1.0,      \
                     double log_floor = 0.0, void *stream = nullptr) const {                       \
      return ::fourier::c::fourier_hip_cepstrum_apply_##SUFFIX(impl.get(), d_in, d_out, batch, log_mult, log_floor, stream);\
    }                                                                                              \
    int reserve(std::size_t batch) const {                                                         \
      return ::fourier::c::fourier_hip_cepstrum_reserve_##SUFFIX(impl.get(), batch);               \
    }                                                                                              \
    int set_option(const char *key, long long value) {                                             \
      return ::fourier::c::fourier_hip_cepstrum_set_option_##SUFFIX(impl.get(), key, value);       \
    }                                                                                              \
    const char *describe() const { return ::fourier::c::fourier_hip_cepstrum_describe_##SUFFIX(impl.get()); }\
    int last_status() const { return ::fourier::c::fourier_hip_cepstrum_last_status_##SUFFIX(impl.get()); }\
    explicit operator bool() const { return static_cast<bool>(impl); }                             \
                                                                                                   \
  private:                                                                                         \
    ::std::unique_ptr<::fourier::c::fourier_cepstrum_##SUFFIX,                                     \
                      void (*)(::fourier::c::fourier_cepstrum_##SUFFIX *)> impl;                   \
  };
FOURIER_DEFINE_CXX_CEPSTRUM_WRAPPER(float, float)
FOURIER_DEFINE_CXX_CEPSTRUM_WRAPPER(double, double)
#undef FOURIER_DEFINE_CXX_CEPSTRUM_WRAPPER

/* non-uniform FFT, 1-D types 1 and 2, on device memory (extension): fourier::nufft<float> / <double> */
template <typename T> struct nufft;

#define FOURIER_DEFINE_CXX_NUFFT_WRAPPER(T, SUFFIX)                                                \
  template <> struct nufft<T> {                                                                    \
    nufft(std::size_t n_modes, double eps = 1e-6, int device = -1)                                 \
        : impl(::fourier::c::fourier_hip_nufft_create_##SUFFIX(n_modes, eps, device),              \
               ::fourier::c::fourier_hip_nufft_destroy_##SUFFIX) {}                                \
    nufft() = delete;                                                                              \
    nufft(const nufft &) = delete;                                                                 \
    nufft(nufft &&) = default;                                                                     \
    nufft &operator=(const nufft &) = delete;                                                      \
    nufft &operator=(nufft &&) = default;                                                          \
    ~nufft() = default;                                                                            \
    std::size_t modes() const { return ::fourier::c::fourier_hip_nufft_modes_##SUFFIX(impl.get()); }\
    std::size_t points() const { return ::fourier::c::fourier_hip_nufft_points_##SUFFIX(impl.get()); }\
    /* m doubles on the HOST; a set-up call that waits for `stream` */                             \
    int set_points(const double *h_points, std::size_t m, void *stream = nullptr) {                \
      return ::fourier::c::fourier_hip_nufft_set_points_##SUFFIX(impl.get(), h_points, m, stream); \
    }                                                                                              \
    /* type 1: `batch` rows of points() strengths -> `batch` rows of modes() */                    \
    int to_modes_device(const void *d_in, void *d_out, std::size_t batch, int sign = -1,           \
                        int order = 0, void *stream = nullptr) const {                             \
      return ::fourier::c::fourier_hip_nufft_to_modes_batch_##SUFFIX(impl.get(), d_in, d_out, batch, sign, order, stream);\
    }                                                                                              \
    /* type 2: `batch` rows of modes() -> `batch` rows of points() values */                       \
    int to_points_device(const void *d_in, void *d_out, std::size_t batch, int sign = 1,           \
                         int order = 0, void *stream = nullptr) const {                            \
      return ::fourier::c::fourier_hip_nufft_to_points_batch_##SUFFIX(impl.get(), d_in, d_out, batch, sign, order, stream);\
    }                                                                                              \
    int reserve(std::size_t batch) const {                                                         \
      return ::fourier::c::fourier_hip_nufft_reserve_##SUFFIX(impl.get(), batch);                  \
    }                                                                                              \
    int set_option(const char *key, long long value) {                                             \
      return ::fourier::c::fourier_hip_nufft_set_option_##SUFFIX(impl.get(), key, value);          \
    }                                                                                              \
    const char *describe() const { return ::fourier::c::fourier_hip_nufft_describe_##SUFFIX(impl.get()); }\
    int last_status() const { return ::fourier::c::fourier_hip_nufft_last_status_##SUFFIX(impl.get()); }\
    explicit operator bool() const { return static_cast<bool>(impl); }                             \
                                                                                                   \
  private:                                                                                         \
    ::std::unique_ptr<::fourier::c::fourier_nufft_##SUFFIX,                                        \
                      void (*)(::fourier::c::fourier_nufft_##SUFFIX *)> impl;                      \
  };
FOURIER_DEFINE_CXX_NUFFT_WRAPPER(float, float)
FOURIER_DEFINE_CXX_NUFFT_WRAPPER(double, double)
#undef FOURIER_DEFINE_CXX_NUFFT_WRAPPER

/* non-uniform FFT, 2-D types 1 and 2, on device memory (extension): fourier::nufft2d<float> / <double> */
template <typename T> struct nufft2d;

#define FOURIER_DEFINE_CXX_NUFFT2D_WRAPPER(T, SUFFIX)                                              \
  template <> struct nufft2d<T> {                                                                  \
    nufft2d(std::size_t n1, std::size_t n2, double eps = 1e-6, int device = -1)                    \
        : impl(::fourier::c::fourier_hip_nufft2d_create_##SUFFIX(n1, n2, eps, device),             \
               ::fourier::c::fourier_hip_nufft2d_destroy_##SUFFIX) {}                              \
    nufft2d() = delete;                                                                            \
    nufft2d(const nufft2d &) = delete;                                                             \
    nufft2d(nufft2d &&) = default;                                                                 \
    nufft2d &operator=(const nufft2d &) = delete;                                                  \
    nufft2d &operator=(nufft2d &&) = default;                                                      \
    ~nufft2d() = default;                                                                          \
    std::size_t modes1() const { return ::fourier::c::fourier_hip_nufft2d_modes1_##SUFFIX(impl.get()); }\
    std::size_t modes2() const { return ::fourier::c::fourier_hip_nufft2d_modes2_##SUFFIX(impl.get()); }\
    std::size_t points() const { return ::fourier::c::fourier_hip_nufft2d_points_##SUFFIX(impl.get()); }\
    /* two arrays of m doubles on the HOST; a set-up call that waits for `stream` */               \
    int set_points(const double *h_x1, const double *h_x2, std::size_t m, void *stream = nullptr) {\
      return ::fourier::c::fourier_hip_nufft2d_set_points_##SUFFIX(impl.get(), h_x1, h_x2, m, stream);\
    }                                                                                              \
    /* type 1: `batch` rows of points() strengths -> `batch` items of modes1() x modes2() */       \
    int to_modes_device(const void *d_in, void *d_out, std::size_t batch, int sign = -1,           \
                        int order = 0, void *stream = nullptr) const {                             \
      return ::fourier::c::fourier_hip_nufft2d_to_modes_batch_##SUFFIX(impl.get(), d_in, d_out, batch, sign, order, stream);\
    }                                                                                              \
    /* type 2: `batch` items of modes1() x modes2() -> `batch` rows of points() values */          \
    int to_points_device(const void *d_in, void *d_out, std::size_t batch, int sign = 1,           \
                         int order = 0, void *stream = nullptr) const {                            \
      return ::fourier::c::fourier_hip_nufft2d_to_points_batch_##SUFFIX(impl.get(), d_in, d_out, batch, sign, order, stream);\
    }                                                                                              \
    int reserve(std::size_t batch) const {                                                         \
      return ::fourier::c::fourier_hip_nufft2d_reserve_##SUFFIX(impl.get(), batch);                \
    }                                                                                              \
    int set_option(const char *key, long long value) {                                             \
      return ::fourier::c::fourier_hip_nufft2d_set_option_##SUFFIX(impl.get(), key, value);        \
    }                                                                                              \
    const char *describe() const { return ::fourier::c::fourier_hip_nufft2d_describe_##SUFFIX(impl.get()); }\
    int last_status() const { return ::fourier::c::fourier_hip_nufft2d_last_status_##SUFFIX(impl.get()); }\
    explicit operator bool() const { return static_cast<bool>(impl); }                             \
                                                                                                   \
  private:                                                                                         \
    ::std::unique_ptr<::fourier::c::fourier_nufft2d_##SUFFIX,                                      \
                      void (*)(::fourier::c::fourier_nufft2d_##SUFFIX *)> impl;                    \
  };
FOURIER_DEFINE_CXX_NUFFT2D_WRAPPER(float, float)
FOURIER_DEFINE_CXX_NUFFT2D_WRAPPER(double, double)
#undef FOURIER_DEFINE_CXX_NUFFT2D_WRAPPER

/* non-uniform FFT, 3-D types 1 and 2, on device memory (extension): fourier::nufft3d<float> / <double> */
template <typename T> struct nufft3d;

#define FOURIER_DEFINE_CXX_NUFFT3D_WRAPPER(T, SUFFIX)                                              \
  template <> struct nufft3d<T> {                                                                  \
    nufft3d(std::size_t n1, std::size_t n2, std::size_t n3, double eps = 1e-6, int device = -1)    \
        : impl(::fourier::c::fourier_hip_nufft3d_create_##SUFFIX(n1, n2, n3, eps, device),         \
               ::fourier::c::fourier_hip_nufft3d_destroy_##SUFFIX) {}                              \
    nufft3d() = delete;                                                                            \
    nufft3d(const nufft3d &) = delete;                                                             \
    nufft3d(nufft3d &&) = default;                                                                 \
    nufft3d &operator=(const nufft3d &) = delete;                                                  \
    nufft3d &operator=(nufft3d &&) = default;                                                      \
    ~nufft3d() = default;                                                                          \
    std::size_t modes1() const { return ::fourier::c::fourier_hip_nufft3d_modes1_##SUFFIX(impl.get()); }\
    std::size_t modes2() const { return ::fourier::c::fourier_hip_nufft3d_modes2_##SUFFIX(impl.get()); }\
    std::size_t modes3() const { return ::fourier::c::fourier_hip_nufft3d_modes3_##SUFFIX(impl.get()); }\
    std::size_t points() const { return ::fourier::c::fourier_hip_nufft3d_points_##SUFFIX(impl.get()); }\
    /* three arrays of m doubles on the HOST; a set-up call that waits for `stream` */             \
    int set_points(const double *h_x1, const double *h_x2, const double *h_x3, std::size_t m,      \
                   void *stream = nullptr) {                                                       \
      return ::fourier::c::fourier_hip_nufft3d_set_points_##SUFFIX(impl.get(), h_x1, h_x2, h_x3, m, stream);\
    }                                                                                              \
    /* type 1: `batch` rows of points() strengths -> `batch` items of modes1() x modes2() x modes3() */\
    int to_modes_device(const void *d_in, void *d_out, std::size_t batch, int sign = -1,           \
                        int order = 0, void *stream = nullptr) const {                             \
      return ::fourier::c::fourier_hip_nufft3d_to_modes_batch_##SUFFIX(impl.get(), d_in, d_out, batch, sign, order, stream);\
    }                                                                                              \
    /* type 2: `batch` items of modes1() x modes2() x modes3() -> `batch` rows of points() values */\
    int to_points_device(const void *d_in, void *d_out, std::size_t batch, int sign = 1,           \
                         int order = 0, void *stream = nullptr) const {                            \
      return ::fourier::c::fourier_hip_nufft3d_to_points_batch_##SUFFIX(impl.get(), d_in, d_out, batch, sign, order, stream);\
    }                                                                                              \
    int reserve(std::size_t batch) const {                                                         \
      return ::fourier::c::fourier_hip_nufft3d_reserve_##SUFFIX(impl.get(), batch);                \
    }                                                                                              \
    int set_option(const char *key, long long value) {                                             \
      return ::fourier::c::fourier_hip_nufft3d_set_option_##SUFFIX(impl.get(), key, value);        \
    }                                                                                              \
    const char *describe() const { return ::fourier::c::fourier_hip_nufft3d_describe_##SUFFIX(impl.get()); }\
    int last_status() const { return ::fourier::c::fourier_hip_nufft3d_last_status_##SUFFIX(impl.get()); }\
    explicit operator bool() const { return static_cast<bool>(impl); }                             \
                                                                                                   \
  private:                                                                                         \
    ::std::unique_ptr<::fourier::c::fourier_nufft3d_##SUFFIX,                                      \
                      void (*)(::fourier::c::fourier_nufft3d_##SUFFIX *)> impl;                    \
  };
FOURIER_DEFINE_CXX_NUFFT3D_WRAPPER(float, float)
FOURIER_DEFINE_CXX_NUFFT3D_WRAPPER(double, double)
#undef FOURIER_DEFINE_CXX_NUFFT3D_WRAPPER

/* chirp-z transform on device memory (extension): fourier::czt<float> / <double> */
template <typename T> struct czt;

#define FOURIER_DEFINE_CXX_CZT_WRAPPER(T, SUFFIX)                                                  \
  template <> struct czt<T> {                                                                      \
    /* w = w_abs exp(2 pi i w_turns), a = a_abs exp(2 pi i a_turns) */                             \
    czt(std::size_t n, std::size_t m, double w_abs, double w_turns, double a_abs = 1.0,            \
        double a_turns = 0.0, bool real_input = false, int device = -1)                            \
        : impl(::fourier::c::fourier_hip_czt_create_##SUFFIX(n, m, w_abs, w_turns, a_abs, a_turns, \
                                                             real_input ? 1 : 0, device),         \
               ::fourier::c::fourier_hip_czt_destroy_##SUFFIX) {}                                  \
    czt() = delete;                                                                                \
    czt(const czt &) = delete;                                                                     \
    czt(czt &&) = default;                                                                         \
    czt &operator=(const czt &) = delete;                                                          \
    czt &operator=(czt &&) = default;                                                              \
    ~czt() = default;                                                                              \
    std::size_t size() const { return ::fourier::c::fourier_hip_czt_size_##SUFFIX(impl.get()); }   \
    std::size_t points() const { return ::fourier::c::fourier_hip_czt_points_##SUFFIX(impl.get()); }\
    /* `batch` rows of n values -> rows of m complex values (no overlap) */                        \
    int transform_device(const void *d_in, void *d_out, std::size_t batch, void *stream = nullptr) const {\
      return ::fourier::c::fourier_hip_czt_transform_##SUFFIX(impl.get(), d_in, d_out, batch, stream);\
    }                                                                                              \
    int reserve(std::size_t batch) const {                                                         \
      return ::fourier::c::fourier_hip_czt_reserve_##SUFFIX(impl.get(), batch);                    \
    }                                                                                              \
    int set_option(const char *key, long long value) {                                             \
      return ::fourier::c::fourier_hip_czt_set_option_##SUFFIX(impl.get(), key, value);            \
    }                                                                                              \
    const char *describe() const { return ::fourier::c::fourier_hip_czt_describe_##SUFFIX(impl.get()); }\
    int last_status() const { return ::fourier::c::fourier_hip_czt_last_status_##SUFFIX(impl.get()); }\
    explicit operator bool() const { return static_cast<bool>(impl); }                             \
                                                                                                   \
  private:                                                                                         \
    ::std::unique_ptr<::fourier::c::fourier_czt_##SUFFIX,                                          \
                      void (*)(::fourier::c::fourier_czt_##SUFFIX *)> impl;                        \
  };
FOURIER_DEFINE_CXX_CZT_WRAPPER(float, float)
FOURIER_DEFINE_CXX_CZT_WRAPPER(double, double)
#undef FOURIER_DEFINE_CXX_CZT_WRAPPER

/* polyphase filter bank channelizer on device memory (extension): fourier::pfb<float> / <double> */
template <typename T> struct pfb;

#define FOURIER_DEFINE_CXX_PFB_WRAPPER(T, SUFFIX)                                                  \
  template <> struct pfb<T> {                                                                      \
    /* hop = 0: critically sampled, hop = channels */                                              \
    pfb(std::size_t channels, std::size_t taps, std::size_t hop = 0, bool real_input = false,      \
        int device = -1)                                                                           \
        : impl(::fourier::c::fourier_hip_pfb_create_##SUFFIX(channels, taps, hop ? hop : channels, \
                                                             real_input ? 1 : 0, device),          \
               ::fourier::c::fourier_hip_pfb_destroy_##SUFFIX) {}                                  \
    pfb() = delete;                                                                                \
    pfb(const pfb &) = delete;                                                                     \
    pfb(pfb &&) = default;                                                                         \
    pfb &operator=(const pfb &) = delete;                                                          \
    pfb &operator=(pfb &&) = default;                                                              \
    ~pfb() = default;                                                                              \
    std::size_t channels() const { return ::fourier::c::fourier_hip_pfb_channels_##SUFFIX(impl.get()); } \
    std::size_t taps() const { return ::fourier::c::fourier_hip_pfb_taps_##SUFFIX(impl.get()); }   \
    std::size_t hop() const { return ::fourier::c::fourier_hip_pfb_hop_##SUFFIX(impl.get()); }     \
    std::size_t bins() const { return ::fourier::c::fourier_hip_pfb_bins_##SUFFIX(impl.get()); }   \
    std::size_t frames(std::size_t length) const {                                                 \
      return ::fourier::c::fourier_hip_pfb_frames_##SUFFIX(impl.get(), length);                    \
    }                                                                                              \
    /* channels * taps reals on the device, nullptr: all ones; waits for `stream` */               \
    int set_filter(const void *d_filter, void *stream = nullptr) {                                 \
      return ::fourier::c::fourier_hip_pfb_set_filter_##SUFFIX(impl.get(), d_filter, stream);      \
    }                                                                                              \
    /* `batch` rows of `length` values -> batch x frames x bins complex values (no overlap) */     \
    int forward_device(const void *d_in, void *d_out, std::size_t length, std::size_t batch,       \
                       void *stream = nullptr) const {                                             \
      return ::fourier::c::fourier_hip_pfb_forward_##SUFFIX(impl.get(), d_in, d_out, length, batch, \
                                                            stream);                               \
    }                                                                                              \
    int reserve(std::size_t length, std::size_t batch) const {                                     \
      return ::fourier::c::fourier_hip_pfb_reserve_##SUFFIX(impl.get(), length, batch);            \
    }                                                                                              \
    int set_option(const char *key, long long value) {                                             \
      return ::fourier::c::fourier_hip_pfb_set_option_##SUFFIX(impl.get(), key, value);            \
    }                                                                                              \
    const char *describe() const { return ::fourier::c::fourier_hip_pfb_describe_##SUFFIX(impl.get()); } \
    int last_status() const { return ::fourier::c::fourier_hip_pfb_last_status_##SUFFIX(impl.get()); } \
    explicit operator bool() const { return static_cast<bool>(impl); }                             \
                                                                                                   \
  private:                                                                                         \
    ::std::unique_ptr<::fourier::c::fourier_pfb_##SUFFIX,                                          \
                      void (*)(::fourier::c::fourier_pfb_##SUFFIX *)> impl;                        \
  };
FOURIER_DEFINE_CXX_PFB_WRAPPER(float, float)
FOURIER_DEFINE_CXX_PFB_WRAPPER(double, double)
#undef FOURIER_DEFINE_CXX_PFB_WRAPPER

/* polyphase synthesis filter bank on device memory (extension): fourier::ipfb<float> / <double> */
template <typename T> struct ipfb;

#define FOURIER_DEFINE_CXX_IPFB_WRAPPER(T, SUFFIX)                                                 \
  template <> struct ipfb<T> {                                                                     \
    /* hop = 0: critically sampled, hop = channels */                                              \
    ipfb(std::size_t channels, std::size_t taps, std::size_t hop = 0, bool real_output = false,    \
         int device = -1)                                                                          \
        : impl(::fourier::c::fourier_hip_ipfb_create_##SUFFIX(channels, taps, hop ? hop : channels, \
                                                              real_output ? 1 : 0, device),        \
               ::fourier::c::fourier_hip_ipfb_destroy_##SUFFIX) {}                                 \
    ipfb() = delete;                                                                               \
    ipfb(const ipfb &) = delete;                                                                   \
    ipfb(ipfb &&) = default;                                                                       \
    ipfb &operator=(const ipfb &) = delete;                                                        \
    ipfb &operator=(ipfb &&) = default;                                                            \
    ~ipfb() = default;                                                                             \
    std::size_t channels() const { return ::fourier::c::fourier_hip_ipfb_channels_##SUFFIX(impl.get()); } \
    std::size_t taps() const { return ::fourier::c::fourier_hip_ipfb_taps_##SUFFIX(impl.get()); }  \
    std::size_t hop() const { return ::fourier::c::fourier_hip_ipfb_hop_##SUFFIX(impl.get()); }    \
    std::size_t bins() const { return ::fourier::c::fourier_hip_ipfb_bins_##SUFFIX(impl.get()); }  \
    /* (frames - 1) * hop + channels * taps */                                                     \
    std::size_t length(std::size_t frames) const {                                                 \
      return ::fourier::c::fourier_hip_ipfb_length_##SUFFIX(impl.get(), frames);                   \
    }                                                                                              \
    /* channels * taps reals on the device, nullptr: all ones; waits for `stream` */               \
    int set_filter(const void *d_filter, void *stream = nullptr) {                                 \
      return ::fourier::c::fourier_hip_ipfb_set_filter_##SUFFIX(impl.get(), d_filter, stream);     \
    }                                                                                              \
    /* batch x frames x bins complex values -> `batch` rows of `length` values (no overlap) */     \
    int inverse_device(const void *d_in, void *d_out, std::size_t frames, std::size_t length,      \
                       std::size_t batch, void *stream = nullptr) const {                          \
      return ::fourier::c::fourier_hip_ipfb_inverse_##SUFFIX(impl.get(), d_in, d_out, frames, length, \
                                                             batch, stream);                       \
    }                                                                                              \
    int reserve(std::size_t frames, std::size_t batch) const {                                     \
      return ::fourier::c::fourier_hip_ipfb_reserve_##SUFFIX(impl.get(), frames, batch);           \
    }                                                                                              \
    const char *describe() const { return ::fourier::c::fourier_hip_ipfb_describe_##SUFFIX(impl.get()); } \
    int last_status() const { return ::fourier::c::fourier_hip_ipfb_last_status_##SUFFIX(impl.get()); } \
    explicit operator bool() const { return static_cast<bool>(impl); }                             \
                                                                                                   \
  private:                                                                                         \
    ::std::unique_ptr<::fourier::c::fourier_ipfb_##SUFFIX,                                         \
                      void (*)(::fourier::c::fourier_ipfb_##SUFFIX *)> impl;                       \
  };
FOURIER_DEFINE_CXX_IPFB_WRAPPER(float, float)
FOURIER_DEFINE_CXX_IPFB_WRAPPER(double, double)
#undef FOURIER_DEFINE_CXX_IPFB_WRAPPER

/* convolution with a prepared filter bank on device memory (extension): fourier::conv<float> / <double> */
template <typename T> struct conv;

#define FOURIER_DEFINE_CXX_CONV_WRAPPER(T, SUFFIX)                                                  \
  template <> struct conv<T> {                                                                      \
    explicit conv(std::size_t size, bool real_data = false, int device = -1)                        \
        : impl(::fourier::c::fourier_hip_conv_create_##SUFFIX(size, real_data ? 1 : 0, device),     \
               ::fourier::c::fourier_hip_conv_destroy_##SUFFIX) {}                                  \
    conv() = delete;                                                                                \
    conv(const conv &) = delete;                                                                    \
    conv(conv &&) = default;                                                                        \
    conv &operator=(const conv &) = delete;                                                         \
    conv &operator=(conv &&) = default;                                                             \
    ~conv() = default;                                                                              \
    std::size_t size() const { return ::fourier::c::fourier_hip_conv_size_##SUFFIX(impl.get()); }   \
    std::size_t filters() const { return ::fourier::c::fourier_hip_conv_filters_##SUFFIX(impl.get()); } \
    /* `filters` rows of `taps` values of the handle's kind -> the bank */                          \
    int set_filters_device(const void *d_taps, std::size_t taps, std::size_t filters = 1,           \
                           bool correlate = false, void *stream = nullptr) {                        \
      return ::fourier::c::fourier_hip_conv_set_filters_##SUFFIX(impl.get(), d_taps, taps, filters, \
                                                                 correlate ? 1 : 0, stream);        \
    }                                                                                               \
    /* `batch` rows of N values -> `batch` rows of N values, row b with filter b mod F */           \
    int apply_device(const void *d_in, void *d_out, std::size_t batch, void *stream = nullptr) const { \
      return ::fourier::c::fourier_hip_conv_apply_##SUFFIX(impl.get(), d_in, d_out, batch, stream); \
    }                                                                                               \
    int reserve(std::size_t batch) const {                                                          \
      return ::fourier::c::fourier_hip_conv_reserve_##SUFFIX(impl.get(), batch);                    \
    }                                                                                               \
    int set_option(const char *key, long long value) {                                              \
      return ::fourier::c::fourier_hip_conv_set_option_##SUFFIX(impl.get(), key, value);            \
    }                                                                                               \
    const char *describe() const { return ::fourier::c::fourier_hip_conv_describe_##SUFFIX(impl.get()); } \
    int last_status() const { return ::fourier::c::fourier_hip_conv_last_status_##SUFFIX(impl.get()); } \
    explicit operator bool() const { return static_cast<bool>(impl); }                              \
                                                                                                    \
  private:                                                                                          \
    ::std::unique_ptr<::fourier::c::fourier_conv_##SUFFIX,                                          \
                      void (*)(::fourier::c::fourier_conv_##SUFFIX *)> impl;                        \
  };
FOURIER_DEFINE_CXX_CONV_WRAPPER(float, float)
FOURIER_DEFINE_CXX_CONV_WRAPPER(double, double)
#undef FOURIER_DEFINE_CXX_CONV_WRAPPER

/* N-D convolution of real items with a prepared filter bank on device memory (extension): fourier::convnd<float> / <double> */
template <typename T> struct convnd;

#define FOURIER_DEFINE_CXX_CONVND_WRAPPER(T, SUFFIX)                                                \
  template <> struct convnd<T> {                                                                    \
    convnd(int rank, const std::size_t *shape, int device = -1)                                     \
        : impl(::fourier::c::fourier_hip_convnd_create_##SUFFIX(rank, shape, device),               \
               ::fourier::c::fourier_hip_convnd_destroy_##SUFFIX) {}                                \
    convnd() = delete;                                                                              \
    convnd(const convnd &) = delete;                                                                \
    convnd(convnd &&) = default;                                                                    \
    convnd &operator=(const convnd &) = delete;                                                     \
    convnd &operator=(convnd &&) = default;                                                         \
    ~convnd() = default;                                                                            \
    int rank() const { return ::fourier::c::fourier_hip_convnd_rank_##SUFFIX(impl.get()); }         \
    /* S into out[0 .. rank-1] */                                                                   \
    int shape(std::size_t *out) const { return ::fourier::c::fourier_hip_convnd_shape_##SUFFIX(impl.get(), out); } \
    std::size_t filters() const { return ::fourier::c::fourier_hip_convnd_filters_##SUFFIX(impl.get()); } \
    /* `filters` blocks of taps_shape reals -> the bank */                                          \
    int set_filters_device(const void *d_taps, const std::size_t *taps_shape, std::size_t filters = 1, \
                           bool correlate = false, void *stream = nullptr) {                        \
      return ::fourier::c::fourier_hip_convnd_set_filters_##SUFFIX(impl.get(), d_taps, taps_shape, filters, \
                                                                   correlate ? 1 : 0, stream);      \
    }                                                                                               \
    /* the extent of the items read and the window of the result stored (default: S, 0, S) */       \
    int set_window(const std::size_t *in_shape, const std::size_t *out_first, const std::size_t *out_shape) { \
      return ::fourier::c::fourier_hip_convnd_set_window_##SUFFIX(impl.get(), in_shape, out_first, out_shape); \
    }                                                                                               \
    /* `batch` items of in_shape reals -> `batch` items of out_shape reals, item b with filter (filter_first + b) mod F */ \
    int apply_device(const void *d_in, void *d_out, std::size_t batch, std::size_t filter_first = 0, \
                     void *stream = nullptr) const {                                                \
      return ::fourier::c::fourier_hip_convnd_apply_batch_##SUFFIX(impl.get(), d_in, d_out, batch, filter_first, stream); \
    }                                                                                               \
    int reserve(std::size_t batch) const {                                                          \
      return ::fourier::c::fourier_hip_convnd_reserve_##SUFFIX(impl.get(), batch);                  \
    }                                                                                               \
    int set_option(const char *key, long long value) {                                              \
      return ::fourier::c::fourier_hip_convnd_set_option_##SUFFIX(impl.get(), key, value);          \
    }                                                                                               \
    const char *describe() const { return ::fourier::c::fourier_hip_convnd_describe_##SUFFIX(impl.get()); } \
    int last_status() const { return ::fourier::c::fourier_hip_convnd_last_status_##SUFFIX(impl.get()); } \
    explicit operator bool() const { return static_cast<bool>(impl); }                              \
                                                                                                    \
  private:                                                                                          \
    ::std::unique_ptr<::fourier::c::fourier_convnd_##SUFFIX,                                        \
                      void (*)(::fourier::c::fourier_convnd_##SUFFIX *)> impl;                      \
  };
FOURIER_DEFINE_CXX_CONVND_WRAPPER(float, float)
FOURIER_DEFINE_CXX_CONVND_WRAPPER(double, double)
#undef FOURIER_DEFINE_CXX_CONVND_WRAPPER

/* linear convolution with a prepared filter bank on device memory (extension): fourier::lconv<float> / <double> */
template <typename T> struct lconv;

#define FOURIER_DEFINE_CXX_LCONV_WRAPPER(T, SUFFIX)                                                 \
  template <> struct lconv<T> {                                                                     \
    lconv(std::size_t length, std::size_t taps, int mode = ::fourier::c::FOURIER_LCONV_FULL,        \
          bool real_data = false, int device = -1)                                                  \
        : impl(::fourier::c::fourier_hip_lconv_create_##SUFFIX(length, taps, mode, real_data ? 1 : 0, device), \
               ::fourier::c::fourier_hip_lconv_destroy_##SUFFIX) {}                                 \
    lconv() = delete;                                                                               \
    lconv(const lconv &) = delete;                                                                  \
    lconv(lconv &&) = default;                                                                      \
    lconv &operator=(const lconv &) = delete;                                                       \
    lconv &operator=(lconv &&) = default;                                                           \
    ~lconv() = default;                                                                             \
    std::size_t length() const { return ::fourier::c::fourier_hip_lconv_length_##SUFFIX(impl.get()); } \
    std::size_t taps() const { return ::fourier::c::fourier_hip_lconv_taps_##SUFFIX(impl.get()); }  \
    std::size_t out_length() const { return ::fourier::c::fourier_hip_lconv_out_length_##SUFFIX(impl.get()); } \
    std::size_t filters() const { return ::fourier::c::fourier_hip_lconv_filters_##SUFFIX(impl.get()); } \
    /* `filters` rows of taps() values of the handle's kind -> the bank */                          \
    int set_filters_device(const void *d_taps, std::size_t filters = 1, bool correlate = false,     \
                           void *stream = nullptr) {                                                \
      return ::fourier::c::fourier_hip_lconv_set_filters_##SUFFIX(impl.get(), d_taps, filters,      \
                                                                  correlate ? 1 : 0, stream);       \
    }                                                                                               \
    /* `batch` rows of length() values -> `batch` rows of out_length() values, row b with filter b mod F */ \
    int apply_device(const void *d_in, void *d_out, std::size_t batch, void *stream = nullptr) const { \
      return ::fourier::c::fourier_hip_lconv_apply_##SUFFIX(impl.get(), d_in, d_out, batch, stream); \
    }                                                                                               \
    int reserve(std::size_t batch) const {                                                          \
      return ::fourier::c::fourier_hip_lconv_reserve_##SUFFIX(impl.get(), batch);                   \
    }                                                                                               \
    int set_option(const char *key, long long value) {                                              \
      return ::fourier::c::fourier_hip_lconv_set_option_##SUFFIX(impl.get(), key, value);           \
    }                                                                                               \
    const char *describe() const { return ::fourier::c::fourier_hip_lconv_describe_##SUFFIX(impl.get()); } \
    int last_status() const { return ::fourier::c::fourier_hip_lconv_last_status_##SUFFIX(impl.get()); } \
    explicit operator bool() const { return static_cast<bool>(impl); }                              \
                                                                                                    \
  private:                                                                                          \
    ::std::unique_ptr<::fourier::c::fourier_lconv_##SUFFIX,                                         \
                      void (*)(::fourier::c::fourier_lconv_##SUFFIX *)> impl;                       \
  };
FOURIER_DEFINE_CXX_LCONV_WRAPPER(float, float)
FOURIER_DEFINE_CXX_LCONV_WRAPPER(double, double)
#undef FOURIER_DEFINE_CXX_LCONV_WRAPPER

/* real-input N-D transforms on device memory (extension): fourier::real_fft_nd<float> / <double> */
template <typename T> struct real_fft_nd;

#define FOURIER_DEFINE_CXX_REALND_WRAPPER(T, SUFFIX)                                                 \
  template <> struct real_fft_nd<T> {                                                                \
    real_fft_nd(int rank, const std::size_t *shape, int device = -1)                                 \
        : impl(::fourier::c::fourier_hip_realnd_create_##SUFFIX(rank, shape, device),                \
               ::fourier::c::fourier_hip_realnd_destroy_##SUFFIX) {}                                 \
    real_fft_nd() = delete;                                                                          \
    real_fft_nd(const real_fft_nd &) = delete;                                                       \
    real_fft_nd(real_fft_nd &&) = default;                                                           \
    real_fft_nd &operator=(const real_fft_nd &) = delete;                                            \
    real_fft_nd &operator=(real_fft_nd &&) = default;                                                \
    ~real_fft_nd() = default;                                                                        \
    int rank() const { return ::fourier::c::fourier_hip_realnd_rank_##SUFFIX(impl.get()); }         \
    /* items of reals -> items of the half-spectrum shape */                                         \
    int forward_batch_device(const void *d_in, void *d_out, std::size_t batch,                       \
                             ::fourier::transform t = ::fourier::transform::fft,                     \
                             void *stream = nullptr) const {                                         \
      return ::fourier::c::fourier_hip_realnd_forward_batch_##SUFFIX(impl.get(), d_in, d_out, batch, \
                                                                     static_cast<int>(t), stream);   \
    }                                                                                                \
    /* items of the half-spectrum shape -> items of reals */                                         \
    int inverse_batch_device(const void *d_in, void *d_out, std::size_t batch,                       \
                             ::fourier::transform t = ::fourier::transform::ifft,                    \
                             void *stream = nullptr) const {                                         \
      return ::fourier::c::fourier_hip_realnd_inverse_batch_##SUFFIX(impl.get(), d_in, d_out, batch, \
                                                                     static_cast<int>(t), stream);   \
    }                                                                                                \
    int reserve(std::size_t batch) const {                                                           \
      return ::fourier::c::fourier_hip_realnd_reserve_##SUFFIX(impl.get(), batch);                   \
    }                                                                                                \
    const char *describe() const { return ::fourier::c::fourier_hip_realnd_describe_##SUFFIX(impl.get()); } \
    explicit operator bool() const { return static_cast<bool>(impl); }                               \
                                                                                                     \
  private:                                                                                           \
    ::std::unique_ptr<::fourier::c::fourier_realnd_fft_##SUFFIX,                                     \
                      void (*)(::fourier::c::fourier_realnd_fft_##SUFFIX *)> impl;                   \
  };
FOURIER_DEFINE_CXX_REALND_WRAPPER(float, float)
FOURIER_DEFINE_CXX_REALND_WRAPPER(double, double)
#undef FOURIER_DEFINE_CXX_REALND_WRAPPER

} /* namespace fourier */
#endif

#endif /* FOURIER_H_ */
