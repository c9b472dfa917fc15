"""The chunk and row-group walks of the spectrogram / Welch handle and of the cross-spectrum handle under a small scratch bound: the
cases and their assertions, stated once and run twice -- on the CPU emulation (tests/test_spectrogram_emu.py, tests/test_csd_emu.py)
and on the MI355X through the experiments library (tests/test_gpu_chunks.py).  The two callers hand in an adapter (`api`) that creates
handles under a bound, uploads numpy arrays, runs an entry point into an output between guard elements, checks the guards and returns
the result as a numpy array; everything else -- shapes, bounds, the walk a bound gives, tolerances -- is here.

How a call is cut is restated from the plans (spectrogram_plan.h, csd_plan.h, handle_common.h's chunk_rows) so that every case can
assert that it really walks more than one chunk or group, and where the cut falls:
  scratch bytes per frame         bins * ELEM + n_fft * sizeof(T)  (the transformed frame, complex, and the windowed frame, real);
                                  the cross spectrum holds a frame of x and one of y: twice that per frame pair
  partials of one row             tiles * bins * sizeof(T), times CSD_PLANES for the cross spectrum; tiles = ceil(frames / 32) on the
                                  composed route (WELCH_TILE), ceil(frames / frames-per-workgroup) on the fused one
  rows per group                  max(1, min(batch, bound // partials of one row)); the partials buffer is reused by every group
  frames (pairs) per chunk        max(1, min(frames of a group, bound // bytes per frame)), ranges of the flat frame index of the group
forward() has no partials: chunks of the flat frame index of the whole call.

Comparisons.  Against the f64 truth: the tolerances of tests/test_gpu_spectrogram.py and tests/test_gpu_csd.py.  Against a handle of
the same library created without the bound, on the same buffers: bit for bit wherever the walk sums in the unbounded order -- forward()
always (it has no sum), Welch / CSD / coherence wherever no chunk ends inside a slot of partials, and on the fused route always (a
workgroup's tile never spans two groups).  Where a chunk does end inside a slot, the slot's frames are summed in another association:
  Welch   both orders add at most WELCH_TILE = 32 non-negative terms one after another, so each is within 31 eps / 2 of the exact sum S
          of its element and they differ by at most 31 eps S.  S is what the truth holds, so ||got - unbounded||_2 <= 32 eps ||truth||_2.
          (The two roundings behind the slots -- the sum over a row's slots and the scale -- can each move by eps / 2 on either side, so
          the worst case of a single element is 33 eps S; the L2 norm over the bins of a call sits far below it, and the figure is printed.)
  CSD     the terms are not of one sign; sum_f |conj(X) Y| <= sqrt(sum |X|^2 sum |Y|^2) (Cauchy-Schwarz) takes the place of S:
          ||got - unbounded||_2 <= 32 eps ||sqrt(Pxx Pyy)||_2 with Pxx, Pyy the truth's csd(x, x), csd(y, y) under the same fold and scale.
Both are conditions derived from the arithmetic, not measurements.  Every figure is printed with its bound before it is asserted."""
import numpy as np

import csd_truth
import spectrogram_truth
from helpers import rel_l2

REAL = "FOURIER_REAL_SCRATCH_BYTES"
WELCH_TILE = 32
CSD_PLANES = 4
N_FFTS = (64, 250, 63)  # the packed even case; h = 125 odd; odd: the inner plan takes n_fft complex values a row
ALIGNED = (64, (32, 64, 96))                 # frames a row, frames (pairs) in the scratch: every chunk ends on a slot boundary
RAGGED = (35, (1, 2, 3, 7, 20, 35, 40))      # two slots a row, the last partly used: chunks end inside slots, inside rows
FUSED_TILE = {"f32": 64, "f64": 32}          # frames per workgroup of the fused kernels at n_fft = 256; frame pairs: half as many
WORST = {}                                   # (family, real) -> the largest figure / bound seen in this process


def np_real(real):
    return np.float32 if real == "f32" else np.float64


def real_bytes(real):
    return 4 if real == "f32" else 8


def eps(real):
    return float(np.finfo(np_real(real)).eps)


def bins(n_fft):
    return n_fft // 2 + 1


def frame_bytes(real, n_fft, pair=False):
    """scratch bytes per frame of the composed route (per frame pair: the cross spectrum)"""
    per = bins(n_fft) * 2 * real_bytes(real) + n_fft * real_bytes(real)
    return 2 * per if pair else per


def partial_row_bytes(real, n_fft, tiles, pair=False):
    return tiles * bins(n_fft) * real_bytes(real) * (CSD_PLANES if pair else 1)


def length_for(frames, n_fft, hop, pad_mode, extra):
    """a row length that gives `frames` frames, `extra` samples beyond the last frame's start rule"""
    return (frames - 1) * hop + extra + (n_fft if pad_mode == "none" else 0)


def chunk_rows(batch, cap, per):
    return max(1, min(batch, cap // per))


def chunks_of(total, chunk):
    return [(g0, min(chunk, total - g0)) for g0 in range(0, total, chunk)]


def forward_walk(batch, fr, bound, real, n_fft):
    """the chunks (g0, ng) of SpectrogramPlan::forward on the composed route"""
    return chunks_of(batch * fr, chunk_rows(batch * fr, bound, frame_bytes(real, n_fft)))


def sum_walk(batch, fr, bound, real, n_fft, pair=False, tile=WELCH_TILE, fused=False):
    """the row groups [(b0, nb, chunks)] of a Welch / CSD / coherence call; chunks: (g0, ng) of the group's flat frame index on the
    composed route, none on the fused one"""
    tiles = -(-fr // tile)
    rows_per = chunk_rows(batch, bound, partial_row_bytes(real, n_fft, tiles, pair))
    chunk = chunk_rows(min(batch, rows_per) * fr, bound, frame_bytes(real, n_fft, pair))
    return [(b0, nb, [] if fused else chunks_of(nb * fr, chunk)) for b0, nb in chunks_of(batch, rows_per)]


def launches(groups):
    """column-sum launches of a walk, or its groups where it has none"""
    return sum(max(1, len(chunks)) for _, _, chunks in groups)


def split_slots(groups, fr):
    """chunk boundaries that fall inside a slot of partials: the chunk behind each adds to what the one before it wrote"""
    return sum(1 for _, _, chunks in groups for g0, _ in chunks if (g0 % fr) % WELCH_TILE != 0)


def base_tol(describe, real):
    """tests/test_gpu_real.py's tol(): one transform of the inner plan"""
    blu = "bluestein" in describe
    return (4e-6 if blu else 2e-6) if real == "f32" else (1e-11 if blu else 1e-13)


def spectrogram_tol(describe, real):
    """tests/test_gpu_spectrogram.py's tol()"""
    return 2 * 2 * base_tol(describe, real)


def csd_base(describe, real):
    """tests/test_gpu_csd.py's base()"""
    blu = "bluestein" in describe
    return (4e-6 if blu else 2e-6) if real == "f32" else (2e-13 if blu else 1e-13)


def figure(family, real, what, value, bound):
    """print, record, assert"""
    print(f"chunks {family} {real} {what}: figure {value:.3g} bound {bound:.3g} ratio {value / bound:.3g}")
    WORST[family, real] = max(WORST.get((family, real), 0.0), value / bound)
    assert value <= bound, (family, real, what, value, bound)


def print_worst():
    for key, v in sorted(WORST.items()):
        print(f"chunk walks worst figure / bound {key}: {v:.3g}")


def l2(a):
    return float(np.linalg.norm(np.asarray(a, np.complex128)))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def window(rng, real, n):
    return np.ascontiguousarray((0.5 + rng.random(n)).astype(np_real(real)))


class HostApi:
    """the adapter of the CPU emulation build: `fa` is fourier_amd bound to it, the buffers are host memory"""
    GUARD = 64
    SENTINEL = 77.0

    def __init__(self, fa, monkeypatch):
        self.fa, self.monkeypatch = fa, monkeypatch

    def _create(self, cls, real, n_fft, hop, pad_mode, w, bound, fusion):
        if bound is not None:
            self.monkeypatch.setenv(REAL, str(bound))  # read at create only
        try:
            plan = cls(n_fft, real, hop, None, pad_mode != "none", "reflect")
        finally:
            if bound is not None:
                self.monkeypatch.delenv(REAL)
        plan.set_option("fusion", fusion)
        plan.set_window_ptr(w.ctypes.data)
        return plan

    def spectrogram(self, real, n_fft, hop, pad_mode, w, bound, fusion=0):
        return self._create(self.fa.Spectrogram, real, n_fft, hop, pad_mode, w, bound, fusion)

    def cross_spectrum(self, real, n_fft, hop, pad_mode, w, bound, fusion=0):
        return self._create(self.fa.CrossSpectrum, real, n_fft, hop, pad_mode, w, bound, fusion)

    def put(self, a):
        return a

    def _run(self, call, shape, dtype):
        count = int(np.prod(shape))
        buf = np.full(count + 2 * self.GUARD, self.SENTINEL, dtype)
        out = buf[self.GUARD:self.GUARD + count]
        out[:] = np.nan
        call(out.ctypes.data)
        assert np.all(buf[:self.GUARD] == self.SENTINEL) and np.all(buf[-self.GUARD:] == self.SENTINEL), "a guard element was written"
        return out.reshape(shape).copy()

    def forward(self, plan, x, batch, length, power, normalized):
        return self._run(lambda out: plan.forward_ptr(x.ctypes.data, out, length, batch, power, normalized),
                         (batch, plan.frames(length), plan.bins()), x.dtype)

    def welch(self, plan, x, batch, length, fold, scale):
        return self._run(lambda out: plan.welch_ptr(x.ctypes.data, out, length, batch, fold, scale), (batch, plan.bins()), x.dtype)

    def csd(self, plan, x, y, batch, length, fold, scale):
        return self._run(lambda out: plan.csd_ptr(x.ctypes.data, y.ctypes.data, out, length, batch, fold, scale), (batch, plan.bins()),
                         np.complex64 if x.dtype == np.float32 else np.complex128)

    def coherence(self, plan, x, y, batch, length):
        return self._run(lambda out: plan.coherence_ptr(x.ctypes.data, y.ctypes.data, out, length, batch), (batch, plan.bins()), x.dtype)


# ---- the chunk walks of the composed routes
def spectrogram_chunks(api, real, n_fft):
    """SpectrogramPlan::forward and ::welch, "fusion" = 0, batch 3, hop n_fft / 4, with and without padding.  Per frame the scratch holds
    bins complex + n_fft reals; one row of partials is tiles * bins reals, less than one frame's scratch, so the smallest bounds also
    cut the batch into row groups.  n_fft = 63: the inner RealPlan takes 63 complex values a row against the 63.5 a frame has here, so
    under every bound of this test it holds as many rows as the chunk has frames."""
    rng = np.random.default_rng(101 + n_fft)
    hop, batch, per = n_fft // 4, 3, frame_bytes(real, n_fft)
    w = window(rng, real, n_fft)
    for fr, bounds in (ALIGNED, RAGGED):
        for pad_mode in ("reflect", "none"):
            length = length_for(fr, n_fft, hop, pad_mode, 3)
            xh = np.ascontiguousarray(rng.standard_normal((batch, length)).astype(np_real(real)))
            x = api.put(xh)
            ref = api.spectrogram(real, n_fft, hop, pad_mode, w, None)
            d = ref.describe()
            assert d.startswith("spectrogram composed, welch composed: real "), d
            assert ref.frames(length) == spectrogram_truth.frames(length, n_fft, hop, pad_mode) == fr
            t = spectrogram_tol(d, real)
            tag = f"n_fft={n_fft} {pad_mode} frames={fr}"
            want, full = {}, {}
            for power, normalized in ((2, False), (1, True)):
                want[power] = spectrogram_truth.spectrogram(xh, n_fft, hop, n_fft, w, pad_mode, power, normalized)
                full[power] = api.forward(ref, x, batch, length, power, normalized)
                figure("spectrogram", real, f"{tag} unbounded power={power} [{d}]", rel_l2(full[power], want[power]), t)
            want_w = spectrogram_truth.welch(xh, n_fft, hop, n_fft, w, pad_mode, True, 0.37)
            full_w = api.welch(ref, x, batch, length, True, 0.37)
            figure("welch", real, f"{tag} unbounded", rel_l2(full_w, want_w), t)
            for k in bounds:
                small = api.spectrogram(real, n_fft, hop, pad_mode, w, k * per)
                assert small.describe() == d
                fwd, groups = forward_walk(batch, fr, k * per, real, n_fft), sum_walk(batch, fr, k * per, real, n_fft)
                split = split_slots(groups, fr)
                assert len(fwd) > 1 and launches(groups) > 1, (k, fwd, groups)
                assert fwd[0][1] == k and max(ng for _, _, c in groups for _, ng in c) == k  # k frames in the scratch, as the case says
                if fr == ALIGNED[0]:
                    assert split == 0 and len(groups) == 1
                    assert k != 96 or fwd[1][0] % fr == 32  # a chunk that begins inside a row, on its second slot
                else:
                    assert (split > 0) == (k != 35), (k, split)
                for power, normalized in ((2, False), (1, True)):
                    got = api.forward(small, x, batch, length, power, normalized)
                    figure("spectrogram", real, f"{tag} k={k} power={power}", rel_l2(got, want[power]), t)
                    assert same_bits(got, full[power]), ("forward", real, n_fft, pad_mode, fr, k, power)
                got = api.welch(small, x, batch, length, True, 0.37)
                figure("welch", real, f"{tag} k={k}", rel_l2(got, want_w), t)
                assert same_bits(api.welch(small, x, batch, length, True, 0.37), got), ("welch repeated", real, n_fft, pad_mode, fr, k)
                if split == 0:
                    assert same_bits(got, full_w), ("welch", real, n_fft, pad_mode, fr, k)
                else:
                    figure("welch reassociated", real, f"{tag} k={k} split slots={split}", l2(got.astype(np.float64) - full_w),
                           32 * eps(real) * l2(want_w))


def csd_chunks(api, real, n_fft):
    """CsdPlan::csd and ::coherence, "fusion" = 0, batch 3, hop n_fft / 4, with and without padding.  Per frame PAIR the scratch holds
    2 x (bins complex + n_fft reals): the y frames are gathered behind the ng x frames of the chunk, at n_fft = 63 and an odd ng on an
    address that is only element-aligned, and transformed with them in one call of 2 ng rows.  One row of partials is
    tiles * CSD_PLANES * bins reals, about one frame pair's scratch, so a bound of k pairs holds k - 1 rows of partials: the batch is
    cut into row groups up to k = 3."""
    rng = np.random.default_rng(202 + n_fft)
    hop, batch, per = n_fft // 4, 3, frame_bytes(real, n_fft, True)
    w = window(rng, real, n_fft)
    for fr, bounds in (ALIGNED, RAGGED):
        for pad_mode in ("reflect", "none"):
            length = length_for(fr, n_fft, hop, pad_mode, 3)
            xh, yh = csd_truth.pair(rng, batch, length, np_real(real))
            x, y = api.put(xh), api.put(yh)
            ref = api.cross_spectrum(real, n_fft, hop, pad_mode, w, None)
            d = ref.describe()
            assert d.startswith("csd composed, coherence composed: real "), d
            assert ref.frames(length) == csd_truth.frames(length, n_fft, hop, pad_mode) == fr
            tp, tc = 4 * csd_base(d, real), 12 * csd_base(d, real)
            tag = f"n_fft={n_fft} {pad_mode} frames={fr}"
            want_p = csd_truth.csd(xh, yh, n_fft, hop, n_fft, w, pad_mode, True, 0.37)
            want_c = csd_truth.coherence(xh, yh, n_fft, hop, n_fft, w, pad_mode)
            pxx = csd_truth.csd(xh, xh, n_fft, hop, n_fft, w, pad_mode, True, 0.37).real
            pyy = csd_truth.csd(yh, yh, n_fft, hop, n_fft, w, pad_mode, True, 0.37).real
            full_p, full_c = api.csd(ref, x, y, batch, length, True, 0.37), api.coherence(ref, x, y, batch, length)
            figure("csd", real, f"{tag} unbounded [{d}]", rel_l2(full_p, want_p), tp)
            figure("coherence", real, f"{tag} unbounded", rel_l2(full_c, want_c), tc)
            for k in bounds:
                small = api.cross_spectrum(real, n_fft, hop, pad_mode, w, k * per)
                assert small.describe() == d
                groups = sum_walk(batch, fr, k * per, real, n_fft, True)
                split = split_slots(groups, fr)
                assert launches(groups) > 1 and max(ng for _, _, c in groups for _, ng in c) == k, (k, groups)
                if fr == ALIGNED[0]:
                    assert split == 0 and len(groups) == 1
                    assert k != 96 or groups[0][2][1][0] % fr == 32  # a chunk that begins inside a row, on its second slot
                else:
                    assert (split > 0) == (k != 35), (k, split)
                    assert (len(groups) > 1) == (k <= 3), (k, groups)
                got_p, got_c = api.csd(small, x, y, batch, length, True, 0.37), api.coherence(small, x, y, batch, length)
                figure("csd", real, f"{tag} k={k}", rel_l2(got_p, want_p), tp)
                figure("coherence", real, f"{tag} k={k}", rel_l2(got_c, want_c), tc)
                assert same_bits(api.csd(small, x, y, batch, length, True, 0.37), got_p), ("csd repeated", real, n_fft, pad_mode, fr, k)
                assert same_bits(api.coherence(small, x, y, batch, length), got_c), ("coherence repeated", real, n_fft, pad_mode, fr, k)
                if split == 0:
                    assert same_bits(got_p, full_p) and same_bits(got_c, full_c), ("csd", real, n_fft, pad_mode, fr, k)
                else:
                    figure("csd reassociated", real, f"{tag} k={k} split slots={split}", l2(got_p.astype(np.complex128) - full_p),
                           32 * eps(real) * l2(np.sqrt(pxx * pyy)))


# ---- the row groups
def group_bounds(real, n_fft, tiles, pair):
    """a bound below a frame and below a row of partials, and one of exactly two rows of partials"""
    return (8, 2 * partial_row_bytes(real, n_fft, tiles, pair))


def group_shapes(n_fft, hop, fr):
    """one odd and one even row length of `fr` frames, reflect padding"""
    lengths = [length_for(fr, n_fft, hop, "reflect", extra) for extra in (2, 3)]
    assert sorted(v % 2 for v in lengths) == [0, 1]
    return lengths


def check_groups(groups, bound, batch):
    if bound == 8:
        assert [nb for _, nb, _ in groups] == [1] * batch and all(ng == 1 for _, _, c in groups for _, ng in c), groups
    else:
        assert [nb for _, nb, _ in groups] == [2, 2, 1], groups


def welch_groups(api, real, n_fft, fused):
    """Batch 5 walked in groups of one row (a bound of 8 bytes) and of 2, 2 and 1 rows (a bound of exactly two rows of partials), every
    group through the same partials buffer, an odd and an even row length.  With the odd length every second row starts on an odd
    element.  Fused route (n_fft = 256): bit-equal to the unbounded fused handle, a tile never spans two groups; its loads take pairs
    of reals only where the row length is even, and then every group's base is even too.  Composed route: 35 frames a row, under
    either bound one frame per chunk; the truth's tolerance, and the bound on a re-associated sum against the unbounded handle."""
    rng = np.random.default_rng(303 + n_fft)
    hop, batch = n_fft // 4, 5
    tile = FUSED_TILE[real] if fused else WELCH_TILE
    fr = tile + 3
    tiles = -(-fr // tile)
    w = window(rng, real, n_fft)
    route = "fused rows" if fused else "composed"
    for length in group_shapes(n_fft, hop, fr):
        xh = np.ascontiguousarray(rng.standard_normal((batch, length)).astype(np_real(real)))
        x = api.put(xh)
        ref = api.spectrogram(real, n_fft, hop, "reflect", w, None, fusion=int(fused))
        d = ref.describe()
        assert d.startswith(f"spectrogram {route}, welch {route}: real "), d
        assert ref.frames(length) == fr
        t = spectrogram_tol(d, real)
        want = spectrogram_truth.welch(xh, n_fft, hop, n_fft, w, "reflect", True, 0.37)
        full = api.welch(ref, x, batch, length, True, 0.37)
        figure("welch", real, f"groups n_fft={n_fft} length={length} {route} unbounded", rel_l2(full, want), t)
        for bound in group_bounds(real, n_fft, tiles, False):
            small = api.spectrogram(real, n_fft, hop, "reflect", w, bound, fusion=int(fused))
            assert small.describe() == d
            groups = sum_walk(batch, fr, bound, real, n_fft, False, tile, fused)
            check_groups(groups, bound, batch)
            got = api.welch(small, x, batch, length, True, 0.37)
            figure("welch", real, f"groups n_fft={n_fft} length={length} {route} bound={bound}", rel_l2(got, want), t)
            assert same_bits(api.welch(small, x, batch, length, True, 0.37), got), ("repeated", real, n_fft, length, bound)
            if fused:
                assert same_bits(got, full), ("welch groups", real, n_fft, length, bound)
            else:
                figure("welch reassociated", real, f"groups n_fft={n_fft} length={length} bound={bound}",
                       l2(got.astype(np.float64) - full), 32 * eps(real) * l2(want))


def csd_groups(api, real, n_fft, fused):
    """welch_groups for the cross spectrum and the coherence: the fused route takes its base from x and from y again for every
    group.  Composed route: one frame pair per chunk under 8 bytes, two under two rows of partials."""
    rng = np.random.default_rng(404 + n_fft)
    hop, batch = n_fft // 4, 5
    tile = FUSED_TILE[real] // 2 if fused else WELCH_TILE
    fr = tile + 3
    tiles = -(-fr // tile)
    w = window(rng, real, n_fft)
    route = "fused rows" if fused else "composed"
    for length in group_shapes(n_fft, hop, fr):
        xh, yh = csd_truth.pair(rng, batch, length, np_real(real))
        x, y = api.put(xh), api.put(yh)
        ref = api.cross_spectrum(real, n_fft, hop, "reflect", w, None, fusion=int(fused))
        d = ref.describe()
        assert d.startswith(f"csd {route}, coherence {route}: real "), d
        assert ref.frames(length) == fr
        tp, tc = 4 * csd_base(d, real), 12 * csd_base(d, real)
        want_p = csd_truth.csd(xh, yh, n_fft, hop, n_fft, w, "reflect", True, 0.37)
        want_c = csd_truth.coherence(xh, yh, n_fft, hop, n_fft, w, "reflect")
        pxx = csd_truth.csd(xh, xh, n_fft, hop, n_fft, w, "reflect", True, 0.37).real
        pyy = csd_truth.csd(yh, yh, n_fft, hop, n_fft, w, "reflect", True, 0.37).real
        full_p, full_c = api.csd(ref, x, y, batch, length, True, 0.37), api.coherence(ref, x, y, batch, length)
        figure("csd", real, f"groups n_fft={n_fft} length={length} {route} unbounded", rel_l2(full_p, want_p), tp)
        figure("coherence", real, f"groups n_fft={n_fft} length={length} {route} unbounded", rel_l2(full_c, want_c), tc)
        for bound in group_bounds(real, n_fft, tiles, True):
            small = api.cross_spectrum(real, n_fft, hop, "reflect", w, bound, fusion=int(fused))
            assert small.describe() == d
            groups = sum_walk(batch, fr, bound, real, n_fft, True, tile, fused)
            check_groups(groups, bound, batch)
            got_p, got_c = api.csd(small, x, y, batch, length, True, 0.37), api.coherence(small, x, y, batch, length)
            figure("csd", real, f"groups n_fft={n_fft} length={length} {route} bound={bound}", rel_l2(got_p, want_p), tp)
            figure("coherence", real, f"groups n_fft={n_fft} length={length} {route} bound={bound}", rel_l2(got_c, want_c), tc)
            assert same_bits(api.csd(small, x, y, batch, length, True, 0.37), got_p), ("repeated", real, n_fft, length, bound)
            if fused:
                assert same_bits(got_p, full_p) and same_bits(got_c, full_c), ("csd groups", real, n_fft, length, bound)
            else:
                figure("csd reassociated", real, f"groups n_fft={n_fft} length={length} bound={bound}",
                       l2(got_p.astype(np.complex128) - full_p), 32 * eps(real) * l2(np.sqrt(pxx * pyy)))
