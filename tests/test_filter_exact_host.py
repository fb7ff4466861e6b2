"""CPU side of the filter's exact cases (tests/filter_exact_cases.py): the NumPy model in pieces (filter_model.setup / iterate)
against integer expectations worked without it, the preconditions that make those cases exact and biting, the two rounding
mutants of the set-up, and the refactored model against the function it replaced."""
import numpy as np
import pytest

import filter_exact_cases as fx
import filter_model as fm
from filter_exact_cases import bits

KINDS = [(kind, size) for kind in fx.STOPS for size in fx.SIZES]
IDS = [f"{kind}-{w}x{h}" for kind, (w, h) in KINDS]


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def model_step(c, step, dtype, **sigmas):
    """One unfused iteration of the model on a case's frame: (ill', var') in `dtype`."""
    ill, var, dz, _ = fm.setup(c["frame"], samples=fx.N, dtype=dtype)
    return fm.iterate(ill, var, c["frame"], dz, step, **{**c["sigmas"], **sigmas})


# ---- the refactored model against the one it replaced -----------------------------------------------------------------

def _old_filter_model(frame, samples=None, counts=None, iterations=5, sigma_l=4.0, sigma_n=0.35, sigma_a=0.1, sigma_z=1.0,
                      dtype=np.float64, steps=None):
    """tests/filter_model.py's filter_model as it stood before it was split into setup() and iterate(), kept word for word."""
    T = np.dtype(dtype).type
    _lum = fm._lum
    f = np.asarray(frame, dtype=np.float32).astype(T)
    H, W = f.shape[:2]
    if steps is None:
        steps = [1 << i for i in range(iterations)]
    with np.errstate(over="ignore", under="ignore"):
        colour, nrm, alb, z, cvar = f[..., 0:3], f[..., 3:6], f[..., 6:9], f[..., 9], f[..., 10]
        a = T(fm.EPS32) + alb
        ill = colour / a
        n = (np.asarray(counts).astype(T) if counts is not None else np.full((H, W), T(samples), dtype=T))
        la = _lum(T, a)
        li = _lum(T, ill)
        var = np.where(n >= T(2), cvar / np.maximum(n, T(1)) / (la * la), li * li).astype(T)
        ys, xs = np.arange(H), np.arange(W)
        yu, yd, xl, xr = np.clip(ys - 1, 0, H - 1), np.clip(ys + 1, 0, H - 1), np.clip(xs - 1, 0, W - 1), np.clip(xs + 1, 0, W - 1)
        dz = T(0.5) * np.maximum(np.abs(z[:, xr] - z[:, xl]), np.abs(z[yd, :] - z[yu, :]))
        sn2, sa2 = T(sigma_n) * T(sigma_n), T(sigma_a) * T(sigma_a)
        zc = T(1e-3) * np.abs(z) + T(1e-20)
        for s in steps:
            k3 = (T(0.25), T(0.5), T(0.25))
            g = np.zeros((H, W), dtype=T)
            for r, yy in enumerate((yu, ys, yd)):
                g = g + k3[r] * (k3[0] * var[yy][:, xl] + k3[1] * var[yy][:, xs] + k3[2] * var[yy][:, xr])
            sd = np.sqrt(np.maximum(g, T(0)))
            L = _lum(T, ill)
            den_l = T(sigma_l) * sd + T(0.01) * np.abs(L) + T(1e-4)
            sw = np.zeros((H, W), dtype=T)
            si = np.zeros((H, W, 3), dtype=T)
            sv = np.zeros((H, W), dtype=T)
            for j in range(-2, 3):
                qy = ys + s * j
                vy = (qy >= 0) & (qy < H)
                qyc = np.clip(qy, 0, H - 1)
                for i in range(-2, 3):
                    qx = xs + s * i
                    vx = (qx >= 0) & (qx < W)
                    qxc = np.clip(qx, 0, W - 1)
                    valid = vy[:, None] & vx[None, :]
                    take = lambda m: m[qyc][:, qxc]
                    h = T(fm.KERNEL[i + 2]) * T(fm.KERNEL[j + 2])
                    d = T(s) * np.sqrt(T(i * i + j * j))
                    dn, da = take(nrm) - nrm, take(alb) - alb
                    e = (dn * dn).sum(-1) / sn2 + (da * da).sum(-1) / sa2
                    e = e + np.abs(take(z) - z) / (T(sigma_z) * dz * d + zc)
                    e = e + np.abs(take(L) - L) / den_l
                    w = np.where(valid, h * np.exp(-e), T(0)).astype(T)
                    sw = sw + w
                    si = si + w[..., None] * take(ill)
                    sv = sv + w * w * take(var)
            ill = si / sw[..., None]
            var = sv / (sw * sw)
        out = ill * a
    return out


def test_the_model_in_pieces_gives_the_bits_of_the_model_it_replaced():
    """Every finite input and every set of sigmas the suite uses: the golden frames and crops at the defaults, the CLI test's
    options, a count image with the n < 2 rule, single steps with all four sigmas at 1e30, and one stop closed."""
    runs = []
    for k in range(3):
        for shape in ("29x37", "5x64", "64x3", "1x1"):
            frame, spp = fx.crop(k, shape)
            runs.append((frame, dict(samples=spp)))
    frame, spp = fx.crop(1, "64x64")
    runs.append((frame, dict(samples=spp, iterations=2, sigma_l=8.0, sigma_n=0.5, sigma_a=0.2, sigma_z=2.0)))
    frame, _ = fx.crop(1, "29x37")
    runs.append((frame, dict(counts=np.random.default_rng(7).integers(1, 41, frame.shape[:2]).astype(np.uint32))))
    runs.append((frame, dict(samples=4, iterations=8)))
    for step in fx.STEPS:
        runs.append((fx.case("open", 37, 29)["frame"], dict(samples=fx.N, steps=[step], **fx.OPEN)))
    for kind in fx.STOPS:
        c = fx.case(kind, 37, 29)
        runs.append((c["frame"], dict(samples=fx.N, steps=[1, 2], **c["sigmas"])))
    for frame, args in runs:
        for dtype, view in ((np.float32, bits), (np.float64, bits64)):
            new, old = fm.filter_model(frame, dtype=dtype, **args), _old_filter_model(frame, dtype=dtype, **args)
            assert np.isfinite(old).all()
            assert np.array_equal(view(new), view(old)), (args, dtype)


# ---- the set-up ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["open", "chain"] + list(fx.STOPS))
def test_built_frames_set_up_to_their_integers(kind):
    for w, h in fx.SIZES:
        c = fx.case(kind, w, h)
        for dtype in (np.float32, np.float64):
            ill, var, dz, a = fm.setup(c["frame"], samples=fx.N, dtype=dtype)
            assert ill.dtype == var.dtype == dz.dtype == np.dtype(dtype)
            assert np.array_equal(ill, c["ill"]) and np.array_equal(var, c["var"]), (kind, w, h, dtype)
            assert np.array_equal(a, np.repeat(c["a"][..., None], 3, axis=-1))
        if kind == "depth":
            edge = dz > 0
            assert edge.any() and (dz[edge] >= 32).all()  # beside an edge dz is 32 or 64: sigma_z = 2^-30 cuts there too


def _var_mutants(frame, samples, counts):
    """Two rounding-level changes of the float32 set-up's variance: ch10 / (n la^2) instead of ch10 / n / la^2, and lum(a)
    formed in double."""
    T = np.float32
    f = np.asarray(frame, dtype=T)
    h, w = f.shape[:2]
    with np.errstate(all="ignore"):
        a = T(fm.EPS32) + f[..., 6:9]
        n = counts.astype(T) if counts is not None else np.full((h, w), T(samples), dtype=T)
        la, li = fm._lum(T, a), fm._lum(T, f[..., 0:3] / a)
        la64 = fm._lum(np.float64, a.astype(np.float64)).astype(T)
        one = np.where(n >= 2, f[..., 10] / (np.maximum(n, T(1)) * (la * la)), li * li).astype(T)
        two = np.where(n >= 2, f[..., 10] / np.maximum(n, T(1)) / (la64 * la64), li * li).astype(T)
    return one, two


def test_the_set_up_inputs_bite_on_rounding_mutants():
    """The inputs the GPU test holds the set-up on change at least one bit of var under each of the two mutants (a kernel that
    contracted, reassociated or approximated there would be seen), and the count image reaches both branches of the rule."""
    changed = np.zeros(2, np.int64)
    total = 0
    for name, frame, samples, counts in fx.setup_inputs():
        var = fm.setup(frame, samples=samples, counts=counts, dtype=np.float32)[1]
        assert var.dtype == np.float32 and np.isfinite(var).all(), name
        for m, mutant in enumerate(_var_mutants(frame, samples, counts)):
            changed[m] += int((bits(mutant) != bits(var)).sum())
        total += var.size
    print(f"SETUP MUTANTS: n x la^2 changes {changed[0]} of {total} values of var, lum(a) in double {changed[1]}")
    assert (changed > 0).all()
    _, frame, _, counts = fx.setup_inputs()[-1]
    var32 = fm.setup(frame, counts=counts, dtype=np.float32)[1]
    li = fm._lum(np.float32, fm.setup(frame, counts=counts, dtype=np.float32)[0])
    low = counts < 2
    assert low.any() and np.array_equal(bits(var32[low]), bits((li * li)[low]))
    assert np.float32(counts.max()) == np.float32(2.0 ** 32)  # 2^32 - 1 rounds up in float32, as the kernel's conversion does


# ---- one stop at a time ---------------------------------------------------------------------------------------------------

def _refused_floor(kind, c, step):
    """The smallest exponent the closed stop gives a refused tap inside the frame, by the definition, in float64."""
    f = c["frame"].astype(np.float64)
    ill, var, dz, _ = fm.setup(c["frame"], samples=fx.N)
    h, w = c["cls"].shape
    sig = {k: float(np.float32(v)) for k, v in c["sigmas"].items()}
    lum = fm._lum(np.float64, ill)
    sd_max = np.sqrt(var.max())  # (the blur is a mean: at most the largest variance)
    floor = np.inf
    for j in range(-2, 3):
        for i in range(-2, 3):
            y0, y1, x0, x1 = max(0, -j * step), min(h, h - j * step), max(0, -i * step), min(w, w - i * step)
            if y0 >= y1 or x0 >= x1:
                continue
            p = (slice(y0, y1), slice(x0, x1))
            q = (slice(y0 + j * step, y1 + j * step), slice(x0 + i * step, x1 + i * step))
            other = c["cls"][q] != c["cls"][p]
            if not other.any():
                continue
            if kind == "normal":
                e = ((f[q][..., 3:6] - f[p][..., 3:6]) ** 2).sum(-1) / sig["sigma_n"] ** 2
            elif kind == "albedo":
                e = ((f[q][..., 6:9] - f[p][..., 6:9]) ** 2).sum(-1) / sig["sigma_a"] ** 2
            elif kind == "depth":
                d = step * np.sqrt(float(i * i + j * j))
                e = np.abs(f[q][..., 9] - f[p][..., 9]) / (sig["sigma_z"] * dz[p] * d + 1e-3 * np.abs(f[p][..., 9]) + 1e-20)
            else:
                e = np.abs(lum[q] - lum[p]) / (sig["sigma_l"] * sd_max + 0.01 * np.abs(lum[p]) + 1e-4)
            floor = min(floor, float(e[other].min()))
    return floor


@pytest.mark.parametrize("kind,size", KINDS, ids=IDS)
def test_one_closed_stop_is_the_exact_mean_over_the_class(kind, size):
    """Both precisions of the model give, to the bit, the integer expectation over "in the frame and of the pixel's class" at
    every step, for ill' and var'.  Preconditions: a refused tap's exponent is above the stop's floor (STOPS); at steps 1 and 2
    at least half the pixels have an admitted and a refused off-centre tap inside the frame; the result differs from the
    all-open result."""
    w, h = size
    c = fx.case(kind, w, h)
    for step in fx.STEPS:
        ill, var, admitted, refused = fx.expected_step(c, step)
        for dtype in (np.float32, np.float64):
            m_ill, m_var = model_step(c, step, dtype)
            assert np.array_equal(bits(m_ill.astype(np.float32)), bits(ill)), (step, dtype)
            assert np.array_equal(bits(m_var.astype(np.float32)), bits(var)), (step, dtype)
        if not refused.any():
            continue  # (33 x 9 at step 16: the few taps inside the frame may all be of the pixel's class)
        floor = _refused_floor(kind, c, step)
        assert floor > fx.STOPS[kind][2], (step, floor)
        both = float(((admitted > 0) & (refused > 0)).mean())
        open_ill, open_var, _, _ = fx.expected_step(dict(c, cls=np.zeros_like(c["cls"])), step)
        differs = float(((bits(open_ill) != bits(ill)).any(-1) | (bits(open_var) != bits(var))).mean())
        print(f"SHARES {kind} {w}x{h} step {step}: admitted and refused {both:.3f}, differs from all-open {differs:.3f}, "
              f"refused exponent >= {floor:.4g}")
        assert differs > 0
        if step <= 2:
            assert both >= 0.5 and differs >= 0.5, (step, both, differs)


@pytest.mark.parametrize("kind,sigma", [("normal", "sigma_n"), ("albedo", "sigma_a")])
def test_a_sigma_whose_inverse_square_overflows_is_the_same_hard_stop(kind, sigma):
    """sigma 1e-20 (float32: the inverse square is beyond the largest float) and 1e-30 (float32: the square underflows to 0):
    both precisions give the bits of the hard-switch sigma, all finite."""
    c = fx.case(kind, 37, 29)
    for step in (1, 2, 16):
        ill, var, _, _ = fx.expected_step(c, step)
        for tiny in (1e-20, 1e-30):
            for dtype in (np.float32, np.float64):
                m_ill, m_var = model_step(c, step, dtype, **{sigma: tiny})
                assert np.isfinite(m_ill).all() and np.isfinite(m_var).all()
                assert np.array_equal(bits(m_ill.astype(np.float32)), bits(ill)) and np.array_equal(bits(m_var.astype(np.float32)), bits(var))


# ---- the variance and chains of steps -------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", fx.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_open_stops_give_the_exact_variance_and_exact_chains(size):
    """All stops open: var' after one iteration at each step, borders included, and the state after the chains 1, 2 and 1, 2, 4
    where every tap of every iteration was inside the frame, are the integer expectation in both precisions."""
    w, h = size
    c = fx.case("open", w, h)
    for step in fx.STEPS:
        ill, var, _, _ = fx.expected_step(c, step)
        for dtype in (np.float32, np.float64):
            m_ill, m_var = model_step(c, step, dtype)
            assert np.array_equal(bits(m_ill.astype(np.float32)), bits(ill)) and np.array_equal(bits(m_var.astype(np.float32)), bits(var))
        assert len(np.unique(var)) > 16
    c = fx.case("chain", w, h)
    for steps in ((1, 2), (1, 2, 4)):
        ill, var, margin = fx.expected_chain(c, steps)
        inner = (slice(margin, h - margin), slice(margin, w - margin))
        count = ill[inner][..., 0].size
        print(f"CHAIN {w}x{h} steps {steps}: {count} pixels {margin} from every border, var exact: {var is not None}")
        assert (count > 0) == (min(w, h) > 2 * margin)
        if steps == (1, 2):
            assert var is not None
            assert count > 0 or (w, h) == (33, 9)
        for dtype in (np.float32, np.float64):
            m_ill, m_var, dz, _ = fm.setup(c["frame"], samples=fx.N, dtype=dtype)
            for s in steps:
                m_ill, m_var = fm.iterate(m_ill, m_var, c["frame"], dz, s, **fx.OPEN)
            assert np.array_equal(bits(m_ill.astype(np.float32)[inner]), bits(ill[inner]))
            if var is not None:
                assert np.array_equal(bits(m_var.astype(np.float32)[inner]), bits(var[inner]))


# ---- non-finite frames and the lab export -----------------------------------------------------------------------------------

def test_a_poisoned_edge_pixel_reaches_only_its_own_taps_in_the_model():
    """One iteration at step 2 with NaN colour at (y, 0): pixel (y, 1) has no tap there and stays finite; (y, 2) has one."""
    frame, spp = fx.poisoned("left", "nan")
    y, _ = fx.POISON_AT["left"]
    for dtype in (np.float32, np.float64):
        out = fm.filter_model(frame, samples=spp, steps=[2], dtype=dtype)
        assert np.isfinite(out[y, 1]).all() and np.isnan(out[y, 2]).all() and np.isnan(out[y, 0]).all()
        assert np.isfinite(out[:, 1]).all()


def test_the_state_export_is_the_lab_librarys_alone(pt, lab):
    import os

    from conftest import ROOT
    assert "pt_debug_filter_state(" in open(os.path.join(ROOT, "include", "ptcore_lab.h")).read()
    assert "pt_debug_filter_state" in lab.LAB_ABI and hasattr(lab.lib, "pt_debug_filter_state")
    assert not hasattr(pt.lib, "pt_debug_filter_state")
    assert "pt_debug_filter_state" not in open(os.path.join(ROOT, "include", "ptcore.h")).read()
