"""States with a known answer for the adaptive selection (csrc/pt_adaptive.hip: classify, decide, scan, scatter) and finalize
kernels, shared by tests/test_adaptive_exact_host.py (the NumPy model gives exactly these answers) and
tests/test_adaptive_exact_gpu.py (so do the kernels, through pt_debug_adaptive_select / pt_debug_adaptive_finalize).

Records are built by hand, so the expected decision follows from the construction and not from running the model:
  * rule cases: one pixel per case, radius 0; the colour variance is the largest float <= the header's threshold T (converged)
    or the next float above it (not converged), T written out here in Python doubles, left to right as include/ptcore.h states it;
  * dilation cases: one unconverged pixel, the expected set is the clipped window's rectangle;
  * compaction cases: the set is given (mode 1) or made by the records (mode 0, radius 0); the list is its indices in order.
"""
import numpy as np

from adaptive_model import BLOCK, REC_M2, REC_N_COLOR, REC_N_HIT, REC_WORDS

F32 = np.float32
SCAN_THREADS = 1024  # PT_ADAPTIVE_SCAN_THREADS (csrc/pt_adaptive.hip)
HUGE = F32(2.0 ** 100)  # a variance no threshold of these cases reaches (a power of two: HUGE * (n - 1) is exact)


def bits(x):
    return np.asarray(x, F32).view(np.uint32)


def blocks_of(pixels):
    return (pixels + BLOCK - 1) // BLOCK


def per_of(pixels):
    """Blocks per lane of the scan's one workgroup."""
    return (blocks_of(pixels) + SCAN_THREADS - 1) // SCAN_THREADS


def lum_of(c):
    """The reference's luminance of a float colour: double through the literals, left to right, rounded to float."""
    c0, c1, c2 = (float(F32(x)) for x in c)
    return F32(0.2126 * c0 + 0.7152 * c1 + 0.0722 * c2)


def threshold(tol, n, lum, floor):
    """The header's right-hand side in double, left to right: ((tol * tol) * n) * (m * m), m = lum > floor ? lum : floor."""
    tol, lum, floor = float(F32(tol)), float(F32(lum)), float(F32(floor))
    m = lum if lum > floor else floor
    return ((tol * tol) * float(n)) * (m * m)


def floats_around(t):
    """(the largest float32 <= t, the next float32 above it) of a finite positive double t."""
    lo = F32(t)
    if float(lo) > t:
        lo = np.nextafter(lo, F32(-np.inf))
    hi = np.nextafter(lo, F32(np.inf))
    assert float(lo) <= t < float(hi)
    return lo, hi


def m2_for(v, n):
    """A float M2 with float32(M2 / (float)(n - 1)) == v (welford_variance), by search around v * (n - 1); None if there is none."""
    v, d = F32(v), F32(n - 1)
    with np.errstate(all="ignore"):
        c = F32(v * d)
        cands = [c]
        up = down = c
        for _ in range(8):
            up, down = np.nextafter(up, F32(np.inf)), np.nextafter(down, F32(-np.inf))
            cands += [up, down]
        for m2 in cands:
            if bits(F32(m2 / d)) == bits(v):
                return F32(m2)
    return None


def variances_around(t, n):
    """((v_lo, M2), (v_hi, M2)): the largest variance <= t and the smallest variance > t that a record at count n can hold at all,
    that is among the floats float32(M2 / (float)(n - 1)) of a float M2.  Where n - 1 is a power of two, and wherever the search
    finds them, these are floats_around(t); at other counts the division skips some floats (steps of up to 1.45 ulp at n - 1 =
    11) and the pair is then the tightest one that exists: no record holds a variance between the two."""
    d = F32(n - 1)
    c = F32(F32(t) * d)
    cands = [c]
    up = down = c
    for _ in range(8):
        up, down = np.nextafter(up, F32(np.inf)), np.nextafter(down, F32(-np.inf))
        cands += [up, down]
    pairs = sorted((float(F32(m2 / d)), F32(m2)) for m2 in cands)
    lo = max((p for p in pairs if p[0] <= t), key=lambda p: p[0])
    hi = min((p for p in pairs if p[0] > t), key=lambda p: p[0])
    assert pairs[0][0] < lo[0] and hi[0] < pairs[-1][0]  # (the search window reaches beyond both)
    f_lo, f_hi = floats_around(t)
    assert 0 <= (int(bits(f_lo)) - int(bits(F32(lo[0])))) <= 1 and 0 <= (int(bits(F32(hi[0]))) - int(bits(f_hi))) <= 1
    return (F32(lo[0]), lo[1]), (F32(hi[0]), hi[1])


def empty_record(pixels):
    return np.zeros((REC_WORDS, pixels), np.uint32)


def put_pixel(rec, p, colour, n, var=None, m2=None, n0=None, n1=None):
    """Pixel p: colour sums = colour * n (asserted exact, and to divide back exactly), both counts n unless given, the colour's
    M2 such that the variance at n0 is `var` (or the M2 given)."""
    n0 = n if n0 is None else n0
    n1 = n if n1 is None else n1
    for k in range(3):
        c = F32(colour[k])
        with np.errstate(all="ignore"):
            s = F32(c * F32(n))
            back = F32(s / F32(n))
        if np.isfinite(c):
            assert float(s) == float(c) * n and back == c, (colour, n)
        rec[k, p] = bits(s)
    rec[9, p] = bits(F32(n))  # (depth sum: something hit)
    rec[REC_N_COLOR, p], rec[REC_N_HIT, p] = n0, n1
    if m2 is None:
        m2 = F32(0) if var is None or n0 < 2 else m2_for(var, n0)
        assert m2 is not None, ("no M2 for variance", var, n0)
    rec[REC_M2, p] = bits(m2)


class Call:
    """One call of the selection: inputs, and the set the call must decide (by construction)."""

    def __init__(self, name, rec, width, n, n_end, mode, peek, tol, floor, min_samples, radius, mask, expect, counts=None,
                 lst=None, words=None, labels=None):
        tp = rec.shape[1]
        self.name, self.rec, self.width, self.n, self.n_end, self.mode, self.peek = name, rec, width, n, n_end, mode, peek
        self.tol, self.floor, self.min_samples, self.radius = F32(tol), F32(floor), min_samples, radius
        self.mask = np.asarray(mask, np.uint8).reshape(-1)
        self.expect = np.asarray(expect, bool).reshape(-1)
        # what a caller could hold before the call: distinct counts, a list of marked slots, two marked words
        self.counts = (1000 + np.arange(tp, dtype=np.uint32) % 7) if counts is None else np.asarray(counts, np.uint32)
        self.lst = (0xDEAD0000 + np.arange(tp, dtype=np.uint32) % 0xFFFF) if lst is None else np.asarray(lst, np.uint32)
        self.words = np.array([0xAAAA, 77], np.uint32) if words is None else np.asarray(words, np.uint32)
        self.labels = labels or {}
        assert self.mask.size == tp == self.expect.size

    def args(self):
        return (self.rec, self.width, self.n, self.n_end, self.mode, self.peek, self.tol, self.floor, self.min_samples, self.radius,
                self.mask, self.counts, self.lst, self.words)

    def __repr__(self):
        return self.name


def check_call(call, got, what):
    """Everything a call must leave behind, from the expected set alone.  got = (mask, counts, list, words, prefix).  Returns the
    number of values compared."""
    mask, counts, lst, words, prefix = (np.asarray(a) for a in got[:5])
    e = call.expect
    tp = e.size
    idx = np.flatnonzero(e).astype(np.uint32)
    tag = f"{what}: {call.name}"
    wrong = np.flatnonzero(((mask & 1) != 0) != e) if not call.peek else np.array([], int)
    assert wrong.size == 0, (tag, "set differs at", wrong[:5], [call.labels.get(int(p)) for p in wrong[:5]])
    assert words[0] == idx.size, (tag, "words[0]", int(words[0]), idx.size)
    per_block = np.add.reduceat(e.astype(np.uint64), np.arange(0, tp, BLOCK))
    want_prefix = (np.cumsum(per_block) - per_block).astype(np.uint32)
    assert np.array_equal(prefix, want_prefix), (tag, "block prefix", np.flatnonzero(prefix != want_prefix)[:5])
    if call.peek:
        keep0 = call.mask & 1 if call.mode != 2 else np.ones(tp, np.uint8)
        assert np.array_equal(mask & 1, keep0), (tag, "peek changed mask bit 0")
        assert np.array_equal(counts, call.counts), (tag, "peek changed the counts")
        assert np.array_equal(lst, call.lst), (tag, "peek changed the list")
        assert words[1] == call.words[1], (tag, "peek changed words[1]")
    else:
        assert np.array_equal(mask, e.astype(np.uint8)), (tag, "mask bytes are not 0 / 1", np.unique(mask))
        assert np.array_equal(lst[:idx.size], idx), (tag, "list", np.flatnonzero(lst[:idx.size] != idx)[:5])
        assert np.array_equal(lst[idx.size:], call.lst[idx.size:]), (tag, "the list was written beyond its length")
        assert np.array_equal(counts, np.where(e, np.uint32(call.n_end), call.counts)), (tag, "counts")
        assert words[1] == (call.n_end if idx.size else call.words[1]), (tag, "words[1]", int(words[1]))
    return 3 * tp + prefix.size + 2


# ---- rule cases ------------------------------------------------------------------------------------------------------------------

def _floor_variants(lum):
    """(name, floor): the luminance sets T; the floor sets T; the luminance one float above the floor; one float below it."""
    lum = F32(lum)
    return [("lum sets T", F32(lum / F32(4))), ("floor sets T", F32(lum * F32(4))),
            ("lum one float above the floor", np.nextafter(lum, F32(0))), ("lum one float below the floor", np.nextafter(lum, F32(np.inf)))]


# grey colours whose luminance is the grey itself, dyadic tolerances, n - 1 a power of two: every operation of T is exact in double
# and M2 = v * (n - 1) is exact in float
EXACT_SETTINGS = [(g, tol, n) for g, tol in ((0.5, 0.25), (0.125, 0.5), (1.0, 0.0625), (2.0, 0.125)) for n in (2, 3, 5, 9, 17)]
GENERAL_SETTINGS = [((0.25, 0.5, 1.0), 0.1, n) for n in (4, 7, 12)]


def rule_threshold_calls(colour, tol, n, exact):
    """Four calls (one per floor variant) of two pixels each: the variance at and just above the threshold."""
    colour = (colour,) * 3 if np.isscalar(colour) else colour
    lum = lum_of(colour)
    calls = []
    for fname, floor in _floor_variants(lum):
        t = threshold(tol, n, lum, floor)
        (lo, m2_lo), (hi, m2_hi) = variances_around(t, n)
        if exact:
            assert (lo, hi) == floats_around(t)
        rec = empty_record(4)
        labels = {}
        for p, (v, m2, conv) in enumerate(((lo, m2_lo, True), (hi, m2_hi, False), (F32(0), F32(0), True), (HUGE, m2_for(HUGE, n), False))):
            assert m2 is not None and bits(F32(m2 / F32(n - 1))) == bits(v), ("no M2 for", v, n)
            assert (float(v) <= t) == conv
            if exact:
                assert float(m2) == float(v) * (n - 1)
            put_pixel(rec, p, colour, n, m2=m2)
            labels[p] = f"variance {v!r} against T = {t!r}: converged = {conv}"
        if exact:
            assert float(lo) == t or "one float" in fname  # (T is a float itself where a power of two sets it)
        name = f"colour {colour[0]}.. tol {tol} n {n}, {fname}"
        calls.append(Call(name, rec, 4, n, n + 1, 0, False, tol, floor, 2, 0, np.ones(4, np.uint8), [False, True, False, True], labels=labels))
    return calls


def rule_other_calls():
    """Counts, degenerate values and scratch bits: one pixel per statement, radius 0."""
    calls = []
    grey = (0.5, 0.5, 0.5)
    nan, inf = F32(np.nan), F32(np.inf)

    def build(name, n, tol, floor, min_samples, pixels):
        """pixels: (label, put_pixel keywords, incoming mask byte, stays active)"""
        rec = empty_record(len(pixels))
        for p, (_, kw, _, _) in enumerate(pixels):
            put_pixel(rec, p, kw.pop("colour", grey), n, **kw)
        return Call(name, rec, len(pixels), n, n + 3, 0, False, tol, floor, min_samples, 0, [m for _, _, m, _ in pixels],
                    [a for _, _, _, a in pixels], labels={p: lab for p, (lab, _, _, _) in enumerate(pixels)})

    n = 8
    calls.append(build("counts", n, 0.5, 0.05, 2, [
        ("n0 = n - 1, variance 0: never converged", dict(n0=n - 1), 1, True),
        ("n0 = n, variance 0: converged", dict(), 1, False),
        ("n1 = 0, n0 = n, huge variance: converged", dict(n1=0, var=HUGE), 1, False),
        ("n1 = 0, n0 = n - 1, NaN colour: converged", dict(n1=0, n0=n - 1, colour=(nan, nan, nan), m2=nan), 1, False),
        ("n1 = 1, n0 = n, huge variance: not converged", dict(n1=1, var=HUGE), 1, True),
        ("n0 = n + 1, variance 0: not converged", dict(n0=n + 1), 1, True)]))
    same = [("variance 0", dict(), 1, None), ("n1 = 0", dict(n1=0), 1, None), ("huge variance", dict(var=HUGE), 1, None),
            ("inactive", dict(), 0, None)]
    calls.append(build("n = min_samples - 1: nobody stops", n, 0.5, 0.05, n + 1, [(a, dict(b), c, c == 1) for a, b, c, _ in same]))
    calls.append(build("n = min_samples: the rule applies", n, 0.5, 0.05, n, [(a, dict(b), c, c == 1 and "huge" in a) for a, b, c, _ in same]))
    calls.append(build("tolerance 0", n, 0.0, 0.05, 2, [
        ("variance 0: converged (0 <= 0)", dict(), 1, False),
        ("the smallest positive variance: not converged", dict(m2=F32(1e-30)), 1, True),
        ("infinite luminance: 0 * inf is NaN, not converged", dict(colour=(inf, inf, inf)), 1, True)]))
    # tol 0.5, n 8, m = 0.5: T = 0.25 * 8 * 0.25 = 0.5; with the floor 2: T = 0.25 * 8 * 4 = 8
    lo, hi = floats_around(threshold(0.5, n, 0.5, 0.05))
    flo, fhi = floats_around(threshold(0.5, n, 0.0, 2.0))
    assert (float(lo), float(flo)) == (0.5, 8.0)
    calls.append(build("degenerate values", n, 0.5, 2.0, 2, [
        ("variance NaN: not converged", dict(m2=nan), 1, True),
        ("variance +Inf: not converged", dict(m2=inf), 1, True),
        ("variance -Inf: converged", dict(m2=-inf), 1, False),
        ("luminance NaN takes the floor: variance at T(floor) converged", dict(colour=(nan, nan, nan), var=flo), 1, False),
        ("luminance NaN takes the floor: one float above T(floor) not", dict(colour=(nan, nan, nan), var=fhi), 1, True),
        ("one NaN channel is a NaN luminance", dict(colour=(0.5, nan, 0.5), var=flo), 1, False),
        ("luminance +Inf: converged", dict(colour=(inf, inf, inf), var=HUGE), 1, False),
        ("luminance -Inf takes the floor", dict(colour=(-inf, -inf, -inf), var=fhi), 1, True),
        ("negative luminance takes the floor", dict(colour=(-64.0, -64.0, -64.0), var=flo), 1, False)]))
    # the scratch bits a peek (bits 1 and 2) or anything else leaves in the incoming mask must not matter; inactive stays inactive
    px = []
    for byte in (1, 3, 5, 7, 0xFF, 0, 2, 4, 6, 0xFE):
        act = byte & 1
        px.append((f"mask byte {byte:#x}, variance at T", dict(var=lo), byte, False))
        px.append((f"mask byte {byte:#x}, variance above T", dict(var=hi), byte, bool(act)))
    calls.append(build("scratch bits", n, 0.5, 0.05, 2, px))
    return calls


# ---- dilation cases ----------------------------------------------------------------------------------------------------------------

DILATION_TILES = [(37, 29), (1, 257), (257, 1)]  # (width, rows)


def _positions(width, rows):
    ys = sorted({0, rows // 2, rows - 1})
    xs = sorted({0, width // 2, width - 1})
    return [(y, x) for y in ys for x in xs]  # corners, edge middles and the middle (fewer where a side is 1)


def _uniform_record(pixels, n, unconverged):
    """Every pixel grey 0.5 with both counts n; variance huge where `unconverged`, else 0."""
    rec = empty_record(pixels)
    rec[0:3] = bits(F32(0.5) * F32(n))
    rec[9] = bits(F32(n))
    rec[REC_N_COLOR] = rec[REC_N_HIT] = n
    rec[REC_M2] = np.where(unconverged, bits(HUGE), np.uint32(0))
    return rec


def dilation_calls(width, rows, radius):
    """One unconverged pixel per call; the rest converged.  Expected set: the window's rectangle clipped to the tile (its area is
    asserted), without the pixel that came in inactive."""
    n, tp = 4, width * rows
    calls = []
    for (y, x) in _positions(width, rows):
        r0, r1, c0, c1 = max(0, y - radius), min(rows - 1, y + radius), max(0, x - radius), min(width - 1, x + radius)
        area = (r1 - r0 + 1) * (c1 - c0 + 1)
        for hole in (False, True):
            unconv = np.zeros((rows, width), bool)
            unconv[y, x] = True
            mask = np.ones((rows, width), np.uint8)
            expect = np.zeros((rows, width), bool)
            expect[r0:r1 + 1, c0:c1 + 1] = True
            assert expect.sum() == area
            if hole:  # an inactive pixel inside the window (unconverged by its record, too): it stays inactive and keeps nobody
                if area == 1:
                    continue
                hy, hx = (r0 if r0 != y else r1), (c0 if c0 != x else c1)
                assert (hy, hx) != (y, x)
                mask[hy, hx] = 6  # (inactive, scratch bits set)
                unconv[hy, hx] = True
                expect[hy, hx] = False
                area -= 1
            assert expect.sum() == area
            name = f"{width}x{rows} radius {radius} at ({y},{x}){' with an inactive pixel' if hole else ''}: {area} active"
            calls.append(Call(name, _uniform_record(tp, n, unconv.reshape(-1)), width, n, n + 2, 0, False, 0.5, 0.05, 2, radius, mask, expect))
    return calls


def inactive_never_unconverged_call():
    """An inactive pixel whose record is far from converged, active converged pixels all round it, radius 1: everybody stops."""
    w, rows, n = 5, 5, 4
    unconv = np.zeros((rows, w), bool)
    unconv[2, 2] = True
    mask = np.ones((rows, w), np.uint8)
    mask[2, 2] = 0
    return Call("inactive pixel with a huge variance keeps nobody", _uniform_record(w * rows, n, unconv.reshape(-1)), w, n, n + 1, 0, False, 0.5,
                0.05, 2, 1, mask, np.zeros(w * rows, bool))


# ---- compaction cases --------------------------------------------------------------------------------------------------------------

# (width, rows, blocks, per): the table the scan's paths were chosen from; the host test asserts blocks and per
COMPACTION_TILES = [(1, 1, 1, 1), (1, 255, 1, 1), (1, 256, 1, 1), (1, 257, 2, 1), (37, 29, 5, 1), (131, 127, 65, 1),
                    (512, 512, 1024, 1), (513, 512, 1026, 2), (1024, 513, 2052, 3)]
LARGE = 262144  # from here on: a handful of masks


def compaction_sets(pixels):
    """{name: set} for a tile of `pixels`; every kind below LARGE, a handful from there on."""
    t = np.arange(pixels)
    rng = np.random.default_rng(pixels)
    waves = np.arange(0, pixels, 64)
    per64 = np.zeros(pixels, bool)
    per64[np.minimum(waves + (waves // 64 * 7) % 64, pixels - 1)] = True  # one pixel per 64 at a moving lane
    tail0 = (pixels - 1) // BLOCK * BLOCK
    sets = {
        "empty": np.zeros(pixels, bool),
        "only the last pixel": t == pixels - 1,
        "one per 64 at a moving lane": per64,
        "blocks alternating full and empty": (t // BLOCK) % 2 == 0,
        "random 50%": rng.uniform(size=pixels) < 0.5,
    }
    if pixels < LARGE:
        sets.update({
            "full": np.ones(pixels, bool),
            "only pixel 0": t == 0,
            "blocks alternating empty and full": (t // BLOCK) % 2 == 1,
            "random 1%": rng.uniform(size=pixels) < 0.01,
            "random 99%": rng.uniform(size=pixels) < 0.99,
            "only the ragged tail": t >= tail0,
        })
    return sets


def compaction_call(width, rows, name, want, mode, peek=False):
    """mode 1: the set is the incoming mask (its other bits set at random: scratch).  mode 0: every pixel comes in active and the
    records make exactly `want` unconverged, radius 0."""
    tp = width * rows
    n = 4
    if mode == 1:
        rec = empty_record(tp)
        junk = (np.random.default_rng(7).integers(0, 128, tp, dtype=np.uint8) << 1).astype(np.uint8)
        mask = junk | want.astype(np.uint8)
    else:
        rec = _uniform_record(tp, n, want)
        mask = np.ones(tp, np.uint8)
    return Call(f"{width}x{rows} mode {mode}{' peek' if peek else ''}: {name}", rec, width, n, n + 4, mode, peek, 0.5, 0.05, 2, 0, mask, want)


# ---- the chained sequence ----------------------------------------------------------------------------------------------------------

def chain_steps(width=131, rows=127, radius=1):
    """mode 2, then mode 0, then a peek, then mode 0 with a shrinking set: (name, record, n, n_end, mode, peek, expected set); the
    state (mask, counts, list, words) of each call is the one the call before left.  Unconverged pixels sit on a coarse lattice, so
    the windows of radius 1 do not touch and the expected set is the union of their clipped rectangles."""
    tp = width * rows
    yy, xx = np.mgrid[0:rows, 0:width]

    def windows(centres):
        out = np.zeros((rows, width), bool)
        for y, x in np.argwhere(centres):
            out[max(0, y - radius):y + radius + 1, max(0, x - radius):x + radius + 1] = True
        return out.reshape(-1)

    first = (yy % 5 == 0) & (xx % 7 == 0)
    second = first & (yy % 10 == 0)  # a subset: the set shrinks
    steps = [("first pass: every pixel", empty_record(tp), 0, 4, 2, False, np.ones(tp, bool)),
             ("rule at 4 samples", _uniform_record(tp, 4, first.reshape(-1)), 4, 8, 0, False, windows(first)),
             ("peek at 8 samples", _uniform_record(tp, 8, second.reshape(-1)), 8, 9, 0, True, windows(second)),
             ("rule at 8 samples", _uniform_record(tp, 8, second.reshape(-1)), 8, 12, 0, False, windows(second))]
    assert windows(first).sum() == sum(min(3, 1 + min(y, 1) + min(rows - 1 - y, 1)) * min(3, 1 + min(x, 1) + min(width - 1 - x, 1))
                                       for y, x in np.argwhere(first))
    return steps


# ---- finalize cases ----------------------------------------------------------------------------------------------------------------

FINALIZE_TILES = [257, 1073]


def finalize_case(pixels):
    """(record, counts): sums, means and M2 are random finite float32 bit patterns (both signs, denormals included), counts mixed
    from {1, 2, 3, 4, 7, 16, 1000}; n1 < count on some pixels, n0 < 2 on some."""
    rng = np.random.default_rng(pixels)
    rec = rng.integers(0, 2**32, (REC_WORDS, pixels), dtype=np.uint64).astype(np.uint32)
    expo = (rec >> 23) & 0xFF
    rec = np.where(expo == 0xFF, rec & np.uint32(0x807FFFFF), rec).astype(np.uint32)  # Inf / NaN patterns become denormals
    rec[0:10, ::9] &= np.uint32(0x807FFFFF)  # and a good share of denormal sums besides
    counts = rng.choice(np.array([1, 2, 3, 4, 7, 16, 1000], np.uint32), pixels)
    n0, n1 = counts.copy(), counts.copy()
    n1[::3] = counts[::3] // 2          # some first hits missed (0 where the count is 1)
    n0[1::5] = rng.integers(0, 2, n0[1::5].size)  # n0 < 2: the colour's variance is 0
    n0[2::7] = np.maximum(counts[2::7], 1) - 1
    rec[REC_N_COLOR], rec[REC_N_HIT] = n0, n1
    assert np.isfinite(rec[0:10].view(F32)).all() and (n1 < counts).any() and (n0 < 2).any() and (n1 < 2).any()
    f = rec[0:10].view(F32)
    assert (f < 0).any() and (f > 0).any() and ((np.abs(f) < np.finfo(F32).tiny) & (f != 0)).any()
    return rec, counts
