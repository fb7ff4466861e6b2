"""The pixel-footprint exclusion of the bounce-0 screen (csrc/pt_footprint.h; reference-configuration builds of variants 6 and 8,
spp >= 8): the Cornell box with perturbed spheres and cameras placed where the exclusion's criteria are closest to their limits --
the eye next to a sphere (c near 0), hugging a wall or in a corner (grazing walls), spheres poking through walls, nested and
duplicated spheres, a scaled scene, a non-power-of-two image -- at resolutions where the exclusion is active, whole frames (or a
128-row tile of the larger ones) against the oracle bit for bit.  tools/footprint_soak.py is the long form of this test
(profiles/r02/footprint_soak_600.json), including two deliberately unsound mutants that it catches.

Pictures at 8-16 samples have little power against a wrong exclusion (a footprint radius three times too small changes no pixel
of 14 of these 16 cases).  The masks themselves are held elsewhere: tests/footprint_cases.py has the cases,
tests/footprint_model.py defines primary_candidates in NumPy float32, tests/test_primary_exclusion_host.py proves that model sound
against the reference's intersection on dense direction lattices, and tests/test_primary_exclusion_gpu.py requires the device's
per-pixel words to equal the model bit for bit."""
import numpy as np
import pytest

from footprint_cases import case as _case
from test_parity_gpu import assert_bit_exact

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", range(16))
def test_footprint_exclusion_changes_no_pixel(pt, oracle, gpu, seed):
    sc, eye, basis, size, rb, re_, spp = _case(pt, seed)
    mode = seed % 2
    ref = oracle.render(size, size, spp, spheres=sc, basis=basis, eye=eye, rng_mode=mode, row_begin=rb, row_end=re_)
    for v in (6, 8, None):
        img, _ = pt.render_frame(size, size, spp, spheres=sc, basis=basis, eye=eye, rng_mode=mode, variant=v, row_begin=rb, row_end=re_)
        assert_bit_exact(img, ref, f"footprint case {seed} ({size}px, {spp} spp, rng {mode}) variant {v}")
