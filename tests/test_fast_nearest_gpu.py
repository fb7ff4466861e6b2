"""The fast mode's nearest<> (csrc/pt_fast.hip) on lists of rays, through the lab library's pt_debug_fast_nearest: what no
frame shows per ray.  Only bounce 4 of the 9-sphere, 5-bounce build uses nearest<NS, LAST = true> (the key alone decides hit or
miss and the index), only primary rays at spp >= 8 reach the masked ctz loop of the specialised build, and a frame at 1 spp
states the first hit only.

The rays have the shape of every secondary ray: 65 536 + 37 origins (a ragged last workgroup) that are model hit points of the
primary-ray cases moved 0.05 along the normal, with random unit directions in the hemisphere of that normal
(fast_model.secondary_rays: why the hemisphere).  Each answer is held to the float64 model of tests/fast_model.py restricted to
the masked spheres: with last = 0 the strong and weak checks of tests/test_fast_rays_gpu.py and at most 2 % undecided rays;
with last = 1 hit or miss and the index equal the model's on decided rays and possible ones elsewhere, the low ib bits of t
are clear, and t is otherwise not compared.  The same list with directions anywhere on the sphere runs without a cap (half of
it heads back into the surface 0.05 away: the shortest hits there are).  A zero-root list -- origins exactly on a sphere, any
direction -- goes through both values of last."""
import numpy as np
import pytest

import fast_model as fm

pytestmark = pytest.mark.gpu

N_RAYS = 65536 + 37
CAP = 0.02


@pytest.fixture(scope="module")
def all_cases(pt):
    return fm.cases(pt)


@pytest.fixture(scope="module")
def ray_lists(all_cases):
    """{(case name, hemisphere): (o, d)}: made once, shared, never changed."""
    made = {}

    def get(name, hemisphere=True):
        if (name, hemisphere) not in made:
            o, d = fm.secondary_rays(all_cases[name], N_RAYS, seed=20 + len(made), hemisphere=hemisphere)
            o.setflags(write=False)
            d.setflags(write=False)
            made[(name, hemisphere)] = (o, d)
        return made[(name, hemisphere)]

    return get


def _probe_and_hold(lab, spheres, o, d, family, specialised, last, mask=0xFFFFFFFF, cap=CAP, tag=""):
    n = len(spheres)
    t, idx = lab.fast_nearest(spheres, np.concatenate([o, d], axis=1), specialised=specialised, last=last, mask=mask)
    ib = fm.index_bits(n)
    active = [bool((mask >> i) & 1) for i in range(n)] if specialised else None
    v = fm.check_ray_list(o, d, spheres, ib, idx, t, active=active, t_exact=not last)
    print(f"{tag}: undecided {100 * v.stats['undecided']:.2f} % (cap {cap}), worst |t - t_model| / tol {v.stats['worst_t_ratio']:.3f}, "
          f"{(idx < 0).sum()} of {len(idx)} rays miss")
    fm.record("nearest:" + family, v.stats)
    assert v, str(v)
    assert cap is None or v.stats["undecided"] <= cap
    if last and ib:  # the ranked key with its index bits cleared
        assert not (t.view(np.uint32)[idx >= 0] & np.uint32((1 << ib) - 1)).any()
    return v, idx, t


@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("mask", [0x1FF, 0x13F, 0x080, 0], ids=["full", "no_small_spheres", "one_sphere", "none"])
def test_specialised_nearest_on_secondary_rays(lab, gpu, all_cases, ray_lists, mask, last):
    case = all_cases["cornell_64x64_b5"]
    o, d = ray_lists(case.name)
    v, idx, _ = _probe_and_hold(lab, case.spheres, o, d, "specialised", True, last, mask, tag=f"cornell <9> mask {mask:#x} last {last}")
    assert set(np.unique(idx)) <= {-1} | {i for i in range(9) if (mask >> i) & 1}
    if mask == 0:
        assert (idx == -1).all()
    if mask == 0x1FF:
        assert (idx >= 0).all()  # a closed scene


@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 9, 33, 64, 65])
def test_generic_nearest_on_secondary_rays(lab, gpu, pt, all_cases, ray_lists, n, last):
    if n <= 2:    # the first spheres of the zero-root scene, origins from its two-sphere frame
        spheres, source = fm.unique_materials(fm.zero_root_scene(pt, n)), "zero_root_generic_n2"
    elif n == 9:
        spheres, source = all_cases["cornell_64x64_b8"].spheres, "cornell_64x64_b8"
    else:
        spheres, source = all_cases[f"random_n{n}_closed"].spheres, f"random_n{n}_closed"
    assert len(spheres) == n
    o, d = ray_lists(source)
    _probe_and_hold(lab, spheres, o, d, "generic", False, last, tag=f"generic n {n} last {last}")


@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("build", ["specialised", "generic_n65"])
def test_nearest_on_directions_anywhere(lab, gpu, all_cases, ray_lists, build, last):
    """Directions over the whole sphere: half head back into the surface 0.05 behind the origin.  No cap (the model alone leaves
    a tenth of these undecided), every check."""
    case = all_cases["cornell_64x64_b5" if build == "specialised" else "random_n65_closed"]
    o, d = ray_lists(case.name, hemisphere=False)
    _probe_and_hold(lab, case.spheres, o, d, "anywhere", build == "specialised", last, 0x1FF, cap=None, tag=f"{build} anywhere last {last}")


@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("build", ["specialised", "specialised_masked", "generic_n2", "generic_n70"])
def test_zero_root_ray_list(lab, gpu, pt, all_cases, build, last):
    """Origins exactly on a sphere (c == 0 whatever the direction: small integers, and the left wall's 1e5), directions anywhere.
    Inward rays (h < 0) are sure hits of that sphere's far side unless something is nearer; outward ones leave that sphere a
    maybe, so only the weak check speaks there -- and nothing is ever returned at t = 0."""
    count = 4096 + 37
    d = fm.random_directions(count, seed=3)
    if build.startswith("specialised"):
        spheres, eye, under = all_cases["zero_root_cornell"].spheres, fm.LEFT_WALL_EYE, 0
        mask = 0x1FF if build == "specialised" else 0x13F
    else:
        spheres, eye, under, mask = fm.unique_materials(fm.zero_root_scene(pt, int(build.split("_n")[1]))), (16.0, 0.0, 0.0), 0, 0xFFFFFFFF
    o = np.broadcast_to(np.asarray(eye, dtype=np.float32), d.shape).copy()
    v, idx, t = _probe_and_hold(lab, spheres, o, d, "zero_root", build.startswith("specialised"), last, mask, cap=None, tag=f"zero root {build} last {last}")
    g, _, r2 = fm.geometry(spheres)
    h = (d.astype(np.float64) * (o - g[under]).astype(np.float64)).sum(-1)
    inward = h < 0
    assert 0.3 < inward.mean() < 0.7
    assert v.decided[inward].mean() > 0.9 and (idx[inward] >= 0).all(), f"{(idx[inward] < 0).sum()} inward rays escape"
    assert (idx[~inward] != under).all()
    if not last:
        assert (t[idx >= 0] > 0).all()
