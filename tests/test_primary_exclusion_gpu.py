"""The device's own primary-ray exclusions against their NumPy models, bit for bit: each lane's primary_candidates word
(csrc/pt_footprint.h; lab.primary_masks) equals tests/footprint_model.py, the five directions it used equal the primary-ray
formula of tests/numpy_restatement.py, and each lane's primary list (csrc/pt_primlist.h; lab.primary_lists) equals
tests/primlist_model.py on all six words.  The models are proved sound against the reference's intersection on the CPU
(tests/test_primary_exclusion_host.py), so equality here is what makes the kernels' exclusions sound -- a compiler, constant
or lane-cooperation error inside either function (the ballot compaction, the shift register, the link encoding, the wave cone
from readlane) changes a word.  The pictures of tests/test_footprint_gpu.py would not notice most of them.

Both dumps put their outputs between 64 guard words on either side and read the sphere buffer back (the bindings raise if
either changed)."""
import numpy as np
import pytest

import footprint_model as fm
import primlist_cases as pc
import primlist_model as pm
from footprint_cases import BASE_SEEDS, EXTRA_SEEDS, case
from numpy_restatement import _primary
from test_primary_exclusion_host import ARMS_FLOOR, coarse_cases, list_arms

pytestmark = pytest.mark.gpu
f32 = np.float32


def assert_masks_equal(lab, name, sc, eye, basis, w, h, rb, re_):
    got = lab.primary_masks(sc, eye, basis, w, h, rb, re_)
    m = fm.primary_candidates(sc, eye, basis, w, h, rb, re_)
    bad = np.nonzero(got != m["word"])[0]
    for tp in bad[:8]:
        print(f"{name}: pixel {tp} (row {rb + tp // w}, col {tp % w}): device {got[tp]:#x}, model {m['word'][tp]:#x}, model's drops "
              f"A {m['A'][tp]:#x} B {m['B'][tp]:#x} C_out {m['C_out'][tp]:#x} C_wall {m['C_wall'][tp]:#x}, coarse {bool(m['keep_all_coarse'][tp])}")
    assert bad.size == 0, (name, int(bad.size))
    return m


@pytest.mark.parametrize("seed", BASE_SEEDS + EXTRA_SEEDS)
def test_masks_equal_the_model_on_the_cases(lab, gpu, seed):
    sc, eye, basis, size, rb, re_, _ = case(lab, seed)  # the case's own size (a 128-row tile at 1024)
    m = assert_masks_equal(lab, f"case {seed}", sc, eye, basis, size, size, rb, re_)
    assert not m["keep_all_coarse"].all(), seed  # the analysis ran


def test_masks_equal_the_model_at_the_edges(lab, gpu):
    sc, eye, basis, _, _, _, _ = case(lab, 3, 256)
    two = np.concatenate([sc, sc])
    two["pos"][9:] += f32(3.0)
    for n in (1, 2, 16, 17):  # the n > 16 || n < 2 shortcut and both sides of it
        m = assert_masks_equal(lab, f"n = {n}", two[:n], eye, basis, 256, 256, 100, 140)
        assert m["keep_all_n"] == (n in (1, 17))
    for size in (64, 320, 500):  # coarse: all kept; 320 and 500: the division path (256, 512, 1024 multiply by the reciprocal)
        sc, eye, basis, _, rb, re_, _ = case(lab, 5, size)
        m = assert_masks_equal(lab, f"{size} px", sc, eye, basis, size, size, rb, re_)
        assert m["keep_all_coarse"].all() == (size == 64)
    sc, eye, basis, _, _, _, _ = case(lab, 0, 256)
    nan_basis = basis.copy()
    nan_basis[4] = np.nan
    m = assert_masks_equal(lab, "NaN basis", sc, eye, nan_basis, 256, 256, 0, 64)
    assert m["keep_all_coarse"].all() and (m["word"] == 0x1FF).all()
    flat = np.tile(basis[:3], 4)  # all four corners equal: dev = 0, every direction the same
    assert_masks_equal(lab, "degenerate basis", sc, eye, flat, 256, 256, 0, 64)


@pytest.mark.parametrize("size", [64, 256, 320, 500, 512, 1024])
def test_directions_are_the_primary_ray_formula(lab, gpu, size):
    sc, eye, basis, _, _, _, _ = case(lab, 1, size)
    rb, re_ = (0, size) if size <= 512 else (700, 828)
    _, dirs = lab.primary_masks(sc, eye, basis, size, size, rb, re_, dirs=True)
    shape = (size, size)
    jit = {-0.5: np.zeros(shape, dtype=f32), 0.0: np.full(shape, f32(0.5)), 0.5: np.ones(shape, dtype=f32)}  # x + (j * 1 - 0.5)
    for k, (dx, dy) in enumerate([(0.0, 0.0), (-0.5, -0.5), (0.5, -0.5), (-0.5, 0.5), (0.5, 0.5)]):
        _, d = _primary(size, size, basis, eye, (jit[dx], jit[dy]))
        want = np.stack([c[rb:re_].reshape(-1) for c in d], axis=-1)
        assert np.array_equal(dirs[:, k].view(np.uint32), want.view(np.uint32)), (size, k)


def device_and_model(lab, sc, eye, basis, w, h, rb, re_, threads):
    """The device's lists and the model's.  r_small, r_big and prim_base are the header words of the very grid the dump staged:
    the builder sums log2(radius) with float atomics, so the last bits of its reference radius -- and with them r_small and r_big --
    may differ between two builds of one scene, and a second build (lab.grid_image) need not classify as this one did.
    lab.grid_image of the same scene, eye and `threads` must agree on everything that does not hang on that sum's rounding."""
    g = lab.grid_image(sc, eye=eye, threads=threads)
    hdr, lists = lab.primary_lists(sc, eye, basis, w, h, rb, re_, threads=threads)
    assert g["valid"] == 1 and hdr[0] == 1
    r_small, r_big = (float(x) for x in hdr[16:18].view(f32))
    assert np.allclose([r_small, r_big], [g["r_small"], g["r_big"]], rtol=1e-5) and int(hdr[18]) == g["prim_base"] == g["max_entries"]
    g["prim_base"] = int(hdr[18])
    m = pm.build_primary_lists(sc, eye, basis, w, h, rb, re_, threads, r_small, r_big, g["prim_base"])
    return lists, m, g


def assert_lists_equal(name, lists, m, prim_base, threads):
    assert lists.shape == m["words"].shape, name
    bad = np.nonzero((lists != m["words"]).any(axis=1))[0]
    for lane in bad[:8]:
        print(f"{name}: lane {lane}: device {[hex(int(x)) for x in lists[lane]]}, model {[hex(int(x)) for x in m['words'][lane]]}, why {m['why'][lane]}")
    assert bad.size == 0, (name, int(bad.size))
    # the entry format, decoded from its description (csrc/pt_grid.h): a valid list names exactly the spheres the lane's cone keeps
    for lane in np.nonzero(lists[:, 0] == 1)[0][::7]:
        got = pm.decode(lists[lane, 2:])
        assert sorted(got) == np.nonzero(m["members"][lane])[0].tolist() and len(got) == lists[lane, 1], (name, lane)
        if lists[lane, 1] > 3:
            assert (int(lists[lane, 2]) >> 16) & 0x1FFF == prim_base + 2 * (lane % threads) + 1, (name, lane)


@pytest.fixture(scope="module")
def device_results():
    return []


@pytest.mark.parametrize("threads", [512, 1024])
def test_lists_equal_the_model(lab, gpu, threads, device_results):
    cases = pc.random_cases(lab) + coarse_cases(lab)
    sc = lab.scene_random(1200, seed=9, with_walls=True)
    eye, basis = pc.camera(lab, sc, 0, 1200, 320, 320)
    cases.append(("random1200_walls_cam0_w320", sc, eye, basis, 320, 320, 158, 162))
    for name, sc, eye, basis, w, h, rb, re_ in cases:
        lists, m, g = device_and_model(lab, sc, eye, basis, w, h, rb, re_, threads)
        assert_lists_equal(f"{name} threads {threads}", lists, m, g["prim_base"], threads)
        device_results.append((lists, m))


@pytest.mark.parametrize("threads", [512, 1024])
def test_lists_equal_the_model_on_the_fallbacks(lab, gpu, threads, device_results):
    for name, sc, eye, basis, w, h, rb, re_, (kind, where) in pc.fallback_cases(lab):
        lists, m, g = device_and_model(lab, sc, eye, basis, w, h, rb, re_, threads)
        assert_lists_equal(f"{name} threads {threads}", lists, m, g["prim_base"], threads)
        device_results.append((lists, m))
        if kind == "pixel":
            assert lists[where, 0] == 0 and lists[where - 8, 0] == 1 and lists[where + 8, 0] == 1, name
        elif kind == "wave":
            assert (lists[64 * where:64 * where + 64, 0] == 0).all() and lists[64 * (where - 1):64 * where, 0].sum() >= 48, name
        else:
            assert (lists[:, 0] == 0).sum() == (m["why"] != pm.VALID).sum() and (m["why"] == pm.WAVE_WIDE).sum() == 3 * 64, name


def test_list_arms_on_the_device(lab, gpu, device_results):
    """Every arm of build_primary_list occurred at least ARMS_FLOOR times in what the device returned (the two tests above)"""
    if not device_results:
        pytest.fail("the list tests of this module did not run before this one")
    arms = list_arms(device_results)
    print(arms)
    assert min(arms.values()) >= ARMS_FLOOR, arms


def test_dumps_are_deterministic_and_an_invalid_grid_is_reported(lab, gpu):
    sc, eye, basis, size, rb, re_, _ = case(lab, 4)
    a = lab.primary_masks(sc, eye, basis, size, size, rb, re_, dirs=True)
    b = lab.primary_masks(sc, eye, basis, size, size, rb, re_, dirs=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    name, sc, eye, basis, w, h, rb, re_ = pc.random_cases(lab, counts=(300,))[3]
    for threads in (512, 1024):
        (h0, l0), (h1, l1) = (lab.primary_lists(sc, eye, basis, w, h, rb, re_, threads=threads) for _ in range(2))
        assert h0[0] == h1[0] == 1 and l0.tobytes() == l1.tobytes(), threads  # (the header's radii: see device_and_model)
    # more spheres than the grid takes: the header says invalid, nothing is launched, the output keeps its fill
    big = lab.scene_random(2100, seed=1, with_walls=False)
    hdr, lists = lab.primary_lists(big, eye, basis, w, h, rb, re_, threads=512)
    assert hdr[0] == 0 and lists is None
