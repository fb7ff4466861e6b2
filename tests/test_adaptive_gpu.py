"""Adaptive sampling of progressive sessions (pt_progressive_set_adaptive; pt_adaptive.hip and pixel_kernel's ADAPTIVE builds).
Contract (include/ptcore.h, EXACTNESS.md A.20): after every pass, each pixel p with count n_p >= 2 is bit for bit pixel p of the
first Render() of a fresh renderer at n_p spp -- oracle.render(..., n_p, frame=0) at that pixel -- and the active sets are those
of the rule, restated in NumPy (tests/adaptive_model.py) from the oracle frames and the record's two counts."""
import os
import subprocess

import numpy as np
import pytest

from adaptive_model import next_active
from conftest import ROOT
from test_denoiser_gpu import _read_exr
from test_parity_gpu import assert_bit_exact

pytestmark = pytest.mark.gpu

EINVAL = -1
_oracle_cache = {}


def ref_frame(oracle, w, h, n, spheres, basis, mb, rng, row_begin, row_end, key):
    k = (key, w, h, n, mb, rng, row_begin, row_end)
    if k not in _oracle_cache:
        _oracle_cache[k] = oracle.render(w, h, n, spheres=spheres, basis=basis, max_bounces=mb, rng_mode=rng, row_begin=row_begin,
                                         row_end=row_end, frame=0, native=True)
    return _oracle_cache[k]


def download_frame(d_out, rows, w, planar):
    if planar:
        return np.ascontiguousarray(d_out.download(np.float32, (14, rows, w)).transpose(1, 2, 0))
    return d_out.download(np.float32, (rows, w, 14))


def check_pixels_at_counts(img, counts, ref_at, what):
    """Every pixel with count >= 2 equals the oracle frame at its own count."""
    for c in np.unique(counts):
        if c < 2:
            continue
        m = counts == c
        assert_bit_exact(img[m][:, None, :], ref_at(int(c))[m][:, None, :], f"{what}: the {m.sum()} pixels at {c} samples")


def tolerance_for(oracle_frame, n, floor, q):
    """A tolerance that stops about a fraction q of the pixels at n samples (so that others stop in later passes)."""
    f = oracle_frame.astype(np.float64)
    lum = 0.2126 * f[..., 0] + 0.7152 * f[..., 1] + 0.0722 * f[..., 2]
    rse = np.sqrt(f[..., 10] / n) / np.maximum(lum, floor)
    return float(np.quantile(rse, q))


class Session:
    """A renderer + session + scene + output buffer on `lib` (product or lab library), and the oracle at any count."""

    def __init__(self, lib, oracle, w, h, spheres, mb, rng, key, variant=None, renderer_spp=8, **ropts):
        self.lib, self.oracle, self.w, self.h, self.spheres, self.mb, self.rng, self.key = lib, oracle, w, h, spheres, mb, rng, key
        self.basis = lib.camera_basis(width=w, height=h)
        self.r = lib.Renderer(w, h, renderer_spp, max_bounces=mb, rng_mode=rng, variant=variant, **ropts)
        self.planar = ropts.get("layout", 0) == lib.LAYOUT_PLANAR
        self.s = lib.Progressive(self.r)
        self.d_scene, self.ns = lib.upload_scene(spheres)
        self.rows = self.r.rows
        self.d_out = lib.DeviceBuffer(self.rows * w * 56)

    def ref(self, n):
        return ref_frame(self.oracle, self.w, self.h, n, self.spheres, self.basis, self.mb, self.rng, self.r.row_begin, self.r.row_end,
                         self.key)

    def render(self, spp):
        return self.s.render(spp, self.d_out.ptr, self.d_scene.ptr, self.ns, self.basis)

    def frame(self):
        return download_frame(self.d_out, self.rows, self.w, self.planar)

    def counts(self):
        return self.s.counts().cpu().numpy().reshape(self.rows, self.w)

    def close(self):
        self.s.destroy()
        self.r.destroy()
        self.d_out.free()
        self.d_scene.free()


def run_adaptive(lab, oracle, w, h, spheres, passes, mb, rng, key, q=0.75, floor=0.05, min_samples=4, radius=1, variant=None,
                 forced=None, **ropts):
    """Adaptive passes against the oracle and the NumPy model after every pass.  forced: {pass index: mask} (lab setter).
    Returns (final counts, variants that ran)."""
    se = Session(lab, oracle, w, h, spheres, mb, rng, key, variant=variant, **ropts)
    try:
        # (the tolerance that stops a fraction q at the middle pass's count: earlier passes stop fewer, later ones more)
        mid = max(min_samples, int(np.cumsum(passes)[len(passes) // 2]))
        tol = tolerance_for(se.ref(mid), mid, floor, q) if q is not None else 0.0
        se.s.set_adaptive(tol, floor=floor, min_samples=min_samples, radius=radius)
        active = np.ones((se.rows, w), bool)
        model_counts = np.zeros((se.rows, w), np.int64)
        ran = set()
        n = 0
        for k, p in enumerate(passes):
            if k > 0:
                rec = se.s.record()
                n0, n1 = rec[10].reshape(se.rows, w), rec[11].reshape(se.rows, w)
                assert (n0[active] <= n).all() and (n1[active] <= n).all()
                if forced is not None and k in forced:
                    want = forced[k]
                    se.s.set_active(want)
                    active = active & want
                else:
                    active = next_active(active, se.ref(n), n0, n1, n, np.float32(tol), np.float32(floor), min_samples, radius)
                assert se.s.active() == active.sum(), f"pass {k}: active() vs the model"
            ran.add(se.s.variant(se.ns))
            se.render(p)
            n += p
            model_counts[active] = n
            counts = se.counts()
            assert np.array_equal(counts, model_counts), f"{key}: pass {k}, counts differ from the model at {np.argwhere(counts != model_counts)[:3]}"
            assert se.s.samples() == counts.max()
            check_pixels_at_counts(se.frame(), counts, se.ref, f"{key} pass {k} rng {rng} bounces {mb} variant {variant}")
        return model_counts, ran
    finally:
        se.close()


@pytest.mark.parametrize("rng", [0, 1], ids=["xorwow", "philox"])
@pytest.mark.parametrize("mb", [5, 8, 3])
@pytest.mark.parametrize("w, h", [(96, 64), (64, 64)], ids=["96x64", "64x64"])
def test_cornell_per_pixel_against_oracle_and_model(lab, oracle, gpu, rng, mb, w, h):
    """The REFB = 5 / 8 and the generic resume builds over the active list: pixels stop in several different passes."""
    counts, ran = run_adaptive(lab, oracle, w, h, lab.scene_cornell(), [4, 4, 4, 4, 4], mb, rng, "cornell")
    assert ran == {6}
    assert len(np.unique(counts)) >= 3, f"stops at {np.unique(counts)}: the tolerance should stagger them"


@pytest.mark.parametrize("radius", [0, 1, 2])
def test_decision_model_for_each_radius(lab, oracle, gpu, radius):
    run_adaptive(lab, oracle, 96, 64, lab.scene_cornell(), [4, 2, 2, 3, 3], 5, 0, "cornell", q=0.5, radius=radius, min_samples=4)


def test_scan_past_one_wave_in_a_session(lab, oracle, gpu):
    """131 x 127 = 16637 pixels = 65 blocks of 256: the scan's second wave on the product's own one-allocation state, and a real
    pass over the list it made (tests/test_adaptive_exact_gpu.py holds the list itself, up to 2052 blocks)."""
    counts, _ = run_adaptive(lab, oracle, 131, 127, lab.scene_cornell(), [4, 4, 4], 5, 0, "cornell", radius=2)
    assert len(np.unique(counts)) >= 2


@pytest.mark.parametrize("rng", [0, 1], ids=["xorwow", "philox"])
def test_every_variant_explicitly_and_automatically(lab, oracle, gpu, rng):
    """Random closed scenes of 40 and 300 spheres, 64 x 48: variants 6, 10, 13, 14 and the automatic choice."""
    ran = set()
    for n, explicit in ((40, [6, 10, None]), (300, [13, 14, None])):
        spheres = lab.scene_random(n, 7, True)
        for v in explicit:
            _, got = run_adaptive(lab, oracle, 64, 48, spheres, [4, 4, 4], 5, rng, ("random", n), q=0.4, variant=v)
            if v is not None:
                assert got == {v}
            ran |= got
    assert {6, 10, 13, 14} <= ran


@pytest.mark.parametrize("rng", [0, 1], ids=["xorwow", "philox"])
def test_row_tile_and_planar_layout(lab, oracle, gpu, rng):
    run_adaptive(lab, oracle, 96, 64, lab.scene_cornell(), [4, 3, 5], 5, rng, "cornell", row_begin=17, row_end=50)
    run_adaptive(lab, oracle, 96, 64, lab.scene_cornell(), [4, 3, 5], 5, rng, "cornell", layout=lab.LAYOUT_PLANAR)
    run_adaptive(lab, oracle, 96, 64, lab.scene_cornell(), [4, 3, 5], 5, rng, "cornell", layout=lab.LAYOUT_PLANAR, row_begin=5,
                 row_end=40)


def _forced_masks(rows, w):
    t = rows * w
    flat = lambda idx: np.isin(np.arange(t), idx).reshape(rows, w)  # noqa: E731
    rng = np.random.default_rng(11)
    isolated = flat(rng.choice(t, size=t // 40, replace=False))
    waves = np.arange(0, t, 64)
    per_wave = flat(np.minimum(waves + (waves // 64 * 7) % 64, t - 1))  # one pixel in every 64 consecutive ones, a different lane each
    ends = flat(np.concatenate([np.arange(w - 1, t, w), np.arange(0, t, w), [t - 1]]))
    all_but_one = ~flat([t // 2 + 3])
    return {"isolated": isolated, "one per wave": per_wave, "row ends and the last pixel": ends, "all but one": all_but_one}


@pytest.mark.parametrize("rng", [0, 1], ids=["xorwow", "philox"])
def test_forced_masks(lab, oracle, gpu, rng):
    w, h = 96, 64
    for name, mask in _forced_masks(h, w).items():
        shrink = mask.copy()
        shrink[np.argwhere(mask)[::3][:, 0], np.argwhere(mask)[::3][:, 1]] = False  # a subset for the third pass
        counts, _ = run_adaptive(lab, oracle, w, h, lab.scene_cornell(), [4, 3, 5], 5, rng, "cornell", q=None,
                                 forced={1: mask, 2: shrink})
        assert (counts[shrink] == 12).all() and (counts[mask & ~shrink] == 7).all() and (counts[~mask] == 4).all(), name


@pytest.mark.parametrize("rng", [0, 1], ids=["xorwow", "philox"])
def test_checkerboard_on_a_thousand_spheres(lab, oracle, gpu, rng):
    """Variant 13 (automatic) with scattered waves: the primary lists' wave cone widens or falls back; both stay exact."""
    w, h = 64, 48
    yy, xx = np.mgrid[0:h, 0:w]
    board = (yy + xx) % 2 == 0
    stripes = board & (xx % 8 < 4)
    for walls in (True, False):
        counts, ran = run_adaptive(lab, oracle, w, h, lab.scene_random(1000, 5, walls), [4, 4, 4], 5, rng, ("random", 1000, walls),
                                   q=None, forced={1: board, 2: stripes})
        assert ran <= {13, 14} and (counts[stripes] == 12).all()


def test_forced_set_may_only_shrink_and_needs_a_first_pass(lab, gpu):
    se = Session(lab, None, 32, 16, lab.scene_cornell(), 5, 0, "x")
    try:
        se.s.set_adaptive(0.1)
        with pytest.raises(lab.PtError) as e:
            se.s.set_active(np.ones((16, 32), bool))
        assert e.value.code == EINVAL and "first pass" in str(e.value)
        se.render(4)
        m = np.zeros((16, 32), bool)
        m[3, 4] = True
        se.s.set_active(m)
        se.render(2)
        with pytest.raises(lab.PtError) as e:
            se.s.set_active(np.ones((16, 32), bool))
        assert e.value.code == EINVAL and "shrink" in str(e.value)
        assert se.s.active() == 1
    finally:
        se.close()


@pytest.mark.parametrize("rng", [0, 1], ids=["xorwow", "philox"])
def test_identity_when_nothing_converges(pt, gpu, rng):
    """min_samples beyond the total: never evaluated, so the frames are a plain session's, byte for byte, and counts uniform."""
    w, h = 96, 64
    basis = pt.camera_basis(width=w, height=h)
    d_scene, ns = pt.upload_scene(pt.scene_cornell())
    r = pt.Renderer(w, h, 8, rng_mode=rng)
    a, b = pt.Progressive(r), pt.Progressive(r)
    b.set_adaptive(0.0, min_samples=1000)
    d_a, d_b = pt.DeviceBuffer(w * h * 56), pt.DeviceBuffer(w * h * 56)
    n = 0
    for p in (3, 2, 4):
        a.render(p, d_a.ptr, d_scene.ptr, ns, basis)
        b.render(p, d_b.ptr, d_scene.ptr, ns, basis)
        n += p
        assert d_a.download(np.uint8, (w * h * 56,)).tobytes() == d_b.download(np.uint8, (w * h * 56,)).tobytes()
        assert (b.counts().cpu().numpy() == n).all() and b.samples() == n and b.active() == w * h
    for x in (a, b):
        x.destroy()
    r.destroy()
    for d in (d_a, d_b, d_scene):
        d.free()


@pytest.mark.parametrize("rng", [0, 1], ids=["xorwow", "philox"])
def test_everything_converges_at_min_samples(pt, oracle, gpu, rng):
    """An enormous tolerance in the closed Cornell box: every pixel stops at min_samples; later passes change nothing."""
    w, h, mb = 96, 64, 5
    se = Session(pt, oracle, w, h, pt.scene_cornell(), mb, rng, "cornell")
    try:
        se.s.set_adaptive(1e30, min_samples=6)
        se.render(3)
        se.render(3)
        assert se.s.active() == 0
        first = se.d_out.download(np.uint8, (w * h * 56,)).tobytes()
        assert_bit_exact(se.frame(), se.ref(6), "all stopped at 6")
        for _ in range(2):
            se.render(5)
            assert se.d_out.download(np.uint8, (w * h * 56,)).tobytes() == first
            assert se.s.active() == 0 and se.s.samples() == 6
            assert (se.counts() == 6).all()
        # reset: every pixel active again, the options kept
        se.s.reset()
        assert se.s.samples() == 0 and se.s.active() == w * h
        se.render(2)
        assert se.s.active() == w * h  # (2 < min_samples)
        se.render(4)
        assert se.s.active() == 0 and se.s.samples() == 6
    finally:
        se.close()


def test_headline_size_rows_against_oracle(pt, oracle, gpu):
    """1024^2 headline scene, passes of 16: sampled rows against the oracle at each pixel's count."""
    w = h = 1024
    se = Session(pt, oracle, w, h, pt.scene_cornell(), 5, 0, "headline")
    try:
        # the tolerance from a plain 16-spp frame (the session's first pass): about a third of the pixels stop at 16
        plain = pt.Progressive(se.r)
        plain.render(16, se.d_out.ptr, se.d_scene.ptr, se.ns, se.basis)
        plain.destroy()
        se.s.set_adaptive(tolerance_for(se.frame(), 16, pt.ADAPTIVE_FLOOR, 0.3), min_samples=16)
        for _ in range(3):
            se.render(16)
        counts, img = se.counts(), se.frame()
        assert len(np.unique(counts)) >= 2
        for row in (0, 401, 777, 1023):
            for c in np.unique(counts[row]):
                ref = oracle.render(w, h, int(c), spheres=pt.scene_cornell(), basis=se.basis, row_begin=row, row_end=row + 1, frame=0,
                                    native=True)[0]
                m = counts[row] == c
                assert_bit_exact(img[row][m][:, None, :], ref[m][:, None, :], f"headline row {row} at {c} samples")
    finally:
        se.close()


def test_refusals(pt, gpu):
    import ctypes

    se = Session(pt, None, 32, 16, pt.scene_cornell(), 5, 0, "x")
    try:
        for kw in ({"tolerance": -0.1}, {"tolerance": float("nan")}, {"tolerance": 0.1, "floor": 0.0}, {"tolerance": 0.1, "floor": -1.0},
                   {"tolerance": 0.1, "min_samples": 1}, {"tolerance": 0.1, "radius": 5}, {"tolerance": 0.1, "radius": -1}):
            with pytest.raises(pt.PtError) as e:
                se.s.set_adaptive(**kw)
            assert e.value.code == EINVAL, kw
        se.s.set_adaptive(0.1)
        assert se.s.active() == 32 * 16
        assert (se.counts() == 0).all()
        se.render(4)
        with pytest.raises(pt.PtError) as e:
            se.s.set_adaptive(0.2)
        assert e.value.code == EINVAL and "0 samples" in str(e.value)
        with pytest.raises(pt.PtError) as e:
            se.s.set_adaptive(None)
        assert e.value.code == EINVAL
        assert pt.lib.pt_progressive_counts(se.s.handle, None, None) == EINVAL
        assert pt.lib.pt_progressive_active(se.s.handle, None) == EINVAL
        assert (se.counts() == 4).all() and se.s.active() <= 32 * 16
        # reset: set_adaptive is allowed again, and None turns it off
        se.s.reset()
        se.s.set_adaptive(None)
        se.render(3)
        assert (se.counts() == 3).all() and se.s.active() == 32 * 16
        n = ctypes.c_int64(0)
        assert pt.lib.pt_progressive_active(se.s.handle, ctypes.byref(n)) == 0 and n.value == 32 * 16
    finally:
        se.close()


def test_refine_stops_when_nothing_is_active(pt, oracle, gpu):
    se = Session(pt, oracle, 64, 32, pt.scene_cornell(), 5, 0, "cornell")
    try:
        se.s.set_adaptive(1e30, min_samples=8)
        seen = []
        passes = se.s.refine(1000, 4, se.d_out.ptr, se.d_scene.ptr, se.ns, se.basis, on_pass=lambda s, k, ms: seen.append(k))
        assert passes == 2 and seen == [0, 1] and se.s.samples() == 8
        se.s.reset()
        se.s.set_adaptive(0.0, min_samples=1000)
        assert se.s.refine(10, 4, se.d_out.ptr, se.d_scene.ptr, se.ns, se.basis) == 2 and se.s.samples() == 8  # (the budget)
    finally:
        se.close()


@pytest.mark.parametrize("rng", ["xorwow", "philox"])
def test_cli_adaptive_equals_python(pt, gpu, tmp_path, rng):
    """pathtrace --size 64 -s 4 --progressive 5 --adaptive T --adaptive-min 4 --adaptive-radius 0: the EXR holds the frame the
    same options give through Python, and the pass lines report the active fraction and the mean spp."""
    w = 64
    tol = 0.35
    out = str(tmp_path / f"ad_{rng}")
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    run = subprocess.run([exe, "--size", str(w), "--rng", rng, "-s", "4", "--progressive", "5", "--adaptive", str(tol), "--adaptive-min",
                          "4", "--adaptive-radius", "0", "-o", out, "--nobitmap"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert "Pass 1: active 100%" in run.stdout and "mean 4 spp" in run.stdout
    got = _read_exr(out + ".exr", w, w)
    se = Session(pt, None, w, w, pt.scene_cornell(), 5, 0 if rng == "xorwow" else 1, "x")
    try:
        se.s.set_adaptive(tol, floor=pt.ADAPTIVE_FLOOR, min_samples=4, radius=0)
        se.s.refine(20, 4, se.d_out.ptr, se.d_scene.ptr, se.ns, se.basis)
        assert_bit_exact(got, se.frame(), "CLI vs Python")
    finally:
        se.close()
