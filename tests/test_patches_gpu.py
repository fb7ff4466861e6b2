"""GPU tests of the training-patch stage (pt_patches_*, csrc/pt_patches.hip): bit parity with the float32 NumPy model
(tests/patches_model.py) of the gathered inputs and targets, the eight sums and the three doubles, at sizes that reach every path
of the kernels (ragged rows, a patch as high as the frame, one pixel, the whole frame, several staging runs and score workgroups),
for three target strides and output bases of every 16-byte misalignment; the network's own pre-processing; independence of order
and of batching; untouched inputs and guard bands; divisors that follow the frame; refusals that launch nothing; and
training_patches on a rendered pair."""
import ctypes
import random

import numpy as np
import pytest

import denoise_restatement as dr
import patches_model as pm
import patches_refusal_cases as prc

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 64  # floats on either side of each output


def _same_values(got, want, what):
    for k in pm.SUMS + ("values",):
        assert got[k] == want[k], f"{what}: {k} {got[k]} on the device, {want[k]} in the model"
    for k in pm.DOUBLES:
        assert pm.double_bits(got[k]) == pm.double_bits(want[k]), f"{what}: {k} {got[k]!r} on the device, {want[k]!r} in the model"


def _same_tensor(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float32, what
    bad = np.argwhere(pm.bits(got) != pm.bits(want))
    assert len(bad) == 0, (f"{what}: {len(bad)} values differ, first [k][c][j][i] = {bad[0].tolist()}: "
                           f"{got[tuple(bad[0])]!r} on the device, {want[tuple(bad[0])]!r} in the model")


def _fields(res):
    return tuple(res[k] for k in pm.SUMS + ("values",)) + tuple(pm.double_bits(res[k]) for k in pm.DOUBLES)


class Rig:
    """A session with its frame pair on the device and two guarded outputs whose bases lie `shift` floats past a 16-byte
    boundary."""

    def __init__(self, pt, frame, gt, p, k, shift=0):
        self.pt, self.p, self.k, self.shift = pt, p, k, shift
        self.frame, self.gt = np.ascontiguousarray(frame, dtype=F), np.ascontiguousarray(gt, dtype=F)
        h, w = self.frame.shape[:2]
        self.ps = pt.Patches(w, h, p, max_patches=k)
        self.d_train, self.d_gt = pt.DeviceBuffer(self.frame.nbytes).upload(self.frame), pt.DeviceBuffer(self.gt.nbytes).upload(self.gt)
        self.sizes = (k * 14 * p * p, k * 3 * p * p)
        self.d_out = [pt.DeviceBuffer((s + 2 * GUARD + 4) * 4) for s in self.sizes]

    def prepare(self):
        self.ps.run_prepare(self.d_train.ptr)

    def score(self, corners):
        self.ps.score(self.d_train.ptr, corners)
        return self.ps.results(len(corners))

    def gather(self, corners, targets=True):
        """-> (inputs, targets or None); asserts that everything outside the n patches kept its bytes."""
        pt, p, n = self.pt, self.p, len(corners)
        for d, s in zip(self.d_out, self.sizes):
            pt.check(pt.lib.pt_memset(d.ptr, 0x5C, (s + 2 * GUARD + 4) * 4))
        first = (GUARD + self.shift) * 4
        self.ps.gather(self.d_train.ptr, corners, self.d_out[0].ptr + first, d_gt=self.d_gt.ptr if targets else None,
                       d_targets=self.d_out[1].ptr + first if targets else None, gt_pixel_stride=self.gt.shape[2])
        out = []
        for d, s, c, wanted in zip(self.d_out, self.sizes, (14, 3), (True, targets)):
            raw = d.download(np.uint32, (s + 2 * GUARD + 4,))
            used = n * c * p * p if wanted else 0
            lo = GUARD + self.shift
            assert (raw[:lo] == 0x5C5C5C5C).all() and (raw[lo + used:] == 0x5C5C5C5C).all(), "written outside the patches"
            out.append(raw[lo:lo + used].view(np.float32).reshape(n, c, p, p) if wanted else None)
        return out

    def inputs_untouched(self):
        return (self.d_train.download(F, self.frame.shape).tobytes() == self.frame.tobytes()
                and self.d_gt.download(F, self.gt.shape).tobytes() == self.gt.tobytes())

    def close(self):
        self.ps.destroy()
        for d in [self.d_train, self.d_gt] + self.d_out:
            d.free()


def _check_against_the_model(rig, corners, what):
    want_in, want_t = pm.gather(rig.frame, rig.gt, corners, rig.p)
    want = pm.scores(rig.frame, corners, rig.p)
    got = rig.score(corners)
    for k, (g, w) in enumerate(zip(got, want)):
        _same_values(g, w, f"{what}, patch {k} at {corners[k]}")
    got_in, got_t = rig.gather(corners)
    _same_tensor(got_in, want_in, f"{what}, inputs")
    _same_tensor(got_t, want_t, f"{what}, targets")


# ---- (a) bit parity with the model ---------------------------------------------------------------------------------------

CASES = [(size, stride, shift) for size, stride, shift in zip(pm.SIZES, (3, 14, 64, 14, 3, 64), (0, 3, 0, 2, 0, 1))]
CASES += [((37, 29, 5), 64, 1), ((37, 29, 5), 14, 0), ((37, 29, 8), 3, 0), ((96, 80, 64), 3, 0), ((300, 9, 9), 14, 2), ((131, 131, 131), 3, 3)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-P{c[0][2]}-stride{c[1]}-shift{c[2]}")
def test_random_hdr_pairs_equal_the_model(pt, gpu, case):
    """Lognormal frames with NaN, +-inf, negatives, exactly 1.0, 65504 and more planted in colour, normal, albedo and the target,
    and a NaN among the features: n = K = 10 corners (the extremes, odd offsets, a duplicate, overlapping neighbours), then n = 1."""
    (w, h, p), stride, shift = case
    frame, gt = pm.frame_pair(w, h, seed=w * 7 + h + p, gt_stride=stride, nan_features=True)
    corners = pm.corner_list(w, h, p)
    rig = Rig(pt, frame, gt, p, len(corners), shift)
    try:
        rig.prepare()
        what = f"{w}x{h} P={p} stride {stride} shift {shift}"
        _check_against_the_model(rig, corners, what)
        _check_against_the_model(rig, corners[1:2], what + ", n = 1")
        assert rig.inputs_untouched(), "an input was written"
        assert rig.ps.memory()["workspace"] > 0
    finally:
        rig.close()


# ---- (b) the network's pre-processing ---------------------------------------------------------------------------------------

def test_inputs_are_the_networks_preprocessing_cropped(pt, gpu):
    """denoise_restatement.preprocess of the whole frame, cropped: also when every maximum of channels 9-13 sits in a pixel that
    no patch holds."""
    w, h, p = 37, 29, 8
    frame, gt = pm.frame_pair(w, h, seed=77)
    frame[h - 1, w - 1, 9:14] = (900.0, 70.0, 50.0, 30.0, 10.0)
    assert all(frame[..., k].max() == frame[h - 1, w - 1, k] for k in range(9, 14))
    corners = [(0, 0), (5, 3), (20, 10), (w - p - 1, h - p - 1)]
    with np.errstate(all="ignore"):
        want = dr.preprocess(frame)
    rig = Rig(pt, frame, gt, p, len(corners))
    try:
        rig.prepare()
        got, _ = rig.gather(corners, targets=False)
        for k, (x, y) in enumerate(corners):
            _same_tensor(got[k], np.ascontiguousarray(want[y:y + p, x:x + p].transpose(2, 0, 1)), f"patch {k}")
    finally:
        rig.close()


# ---- (c) order and batching -------------------------------------------------------------------------------------------------

def test_reversed_corners_give_reversed_results_and_a_batch_equals_its_singles(pt, gpu):
    w, h, p = 64, 48, 12
    frame, gt = pm.frame_pair(w, h, seed=5, gt_stride=14)
    corners = pm.corner_list(w, h, p)
    rig = Rig(pt, frame, gt, p, len(corners))
    try:
        rig.prepare()
        res, (tin, tt) = rig.score(corners), rig.gather(corners)
        back = corners[::-1]
        res_b, (tin_b, tt_b) = rig.score(back), rig.gather(back)
        assert [_fields(r) for r in res_b] == [_fields(r) for r in res][::-1]
        assert tin_b.tobytes() == tin[::-1].tobytes() and tt_b.tobytes() == tt[::-1].tobytes()
        for k, c in enumerate(corners):
            one = rig.score([c])
            assert _fields(one[0]) == _fields(res[k]), f"patch {k} alone"
            a, b = rig.gather([c])
            assert a.tobytes() == tin[k:k + 1].tobytes() and b.tobytes() == tt[k:k + 1].tobytes(), f"patch {k} alone"
        assert len({_fields(r) for r in res}) > 5  # (the patches do differ)
    finally:
        rig.close()


# ---- (d) state --------------------------------------------------------------------------------------------------------------

def test_divisors_follow_the_frame_and_results_survive_a_gather(pt, gpu):
    w, h, p = 37, 29, 8
    one, gt = pm.frame_pair(w, h, seed=31)
    two, _ = pm.frame_pair(w, h, seed=32)
    two[..., 9:14] *= F(3.0)
    corners = pm.corner_list(w, h, p)[:4]
    rig = Rig(pt, one, gt, p, len(corners))
    try:
        rig.prepare()
        res = rig.score(corners)
        got, _ = rig.gather(corners[:2])
        _same_tensor(got, pm.gather(one, gt, corners[:2], p)[0], "first frame")
        assert [_fields(r) for r in rig.ps.results(len(corners))] == [_fields(r) for r in res], "a gather changed the results"
        assert pt.lib.pt_patches_result(rig.ps.handle, len(corners), ctypes.byref(pt.PatchesValues())) == prc.PT_EINVAL
        # a second frame in the same buffer: without a new prepare the old divisors divide it, with one its own
        rig.d_train.upload(two)
        rig.frame = two
        stale, _ = rig.gather(corners[:2])
        fresh_want = pm.gather(two, gt, corners[:2], p)[0]
        assert np.array_equal(pm.bits(stale[:, :9]), pm.bits(fresh_want[:, :9]))
        with np.errstate(all="ignore"):
            old_div = two.transpose(2, 0, 1)[9:14] / pm.divisors(one)[:, None, None]
        x, y = corners[1]
        assert np.array_equal(pm.bits(stale[1, 9:14]), pm.bits(old_div[:, y:y + p, x:x + p]))
        rig.prepare()
        fresh, _ = rig.gather(corners[:2])
        _same_tensor(fresh, fresh_want, "second frame")
        assert not np.array_equal(pm.bits(fresh[:, 9:14]), pm.bits(stale[:, 9:14]))
    finally:
        rig.close()


# ---- (e) refusals -----------------------------------------------------------------------------------------------------------

def test_live_refusals_launch_nothing(pt, gpu):
    """Every refusal of a live 8 x 8 session (tests/patches_refusal_cases.py): PT_EINVAL naming the argument, and after each one
    the outputs still hold their bytes, the records of the score before are what they were, and a valid score and gather give
    the model's bits."""
    w, h, p, k = prc.W, prc.H, prc.P, prc.K
    frame, gt = pm.frame_pair(w, h, seed=9, gt_stride=64)
    corners = [(0, 0), (4, 4)]
    want = pm.scores(frame, corners, p)
    want_in, want_t = pm.gather(frame, gt, corners, p)
    nin, nt = k * 14 * p * p * 4, k * 3 * p * p * 4
    ps = pt.Patches(w, h, p, max_patches=k)
    d_train, d_gt = pt.DeviceBuffer(frame.nbytes).upload(frame), pt.DeviceBuffer(gt.nbytes).upload(gt)
    d_in, d_t = pt.DeviceBuffer(nin), pt.DeviceBuffer(nt)
    try:
        values = pt.PatchesValues()
        assert pt.lib.pt_patches_result(ps.handle, 0, ctypes.byref(values)) == prc.PT_EINVAL  # nothing has been scored yet
        assert "patch_index" in pt.lib.pt_last_error().decode()
        pt.check(pt.lib.pt_memset(d_in.ptr, 0x11, nin))
        cases = prc.unprepared_cases(pt, ps.handle, d_train.ptr, d_gt.ptr, d_in.ptr, d_t.ptr)
        assert prc.play(pt, cases) == 4
        pt.check(pt.lib.pt_device_synchronize())
        assert (d_in.download(np.uint8, (nin,)) == 0x11).all(), "a call before prepare wrote the inputs"
        ps.run_prepare(d_train.ptr)
        ps.score(d_train.ptr, corners)
        cases = [c for c in prc.live_cases(pt, ps.handle, d_train.ptr, d_gt.ptr, d_in.ptr, d_t.ptr)]
        played = 0
        for case in cases:
            if case[1] is None:
                continue
            pt.check(pt.lib.pt_memset(d_in.ptr, 0x11, nin))
            pt.check(pt.lib.pt_memset(d_t.ptr, 0x11, nt))
            played += prc.play(pt, [case])
            pt.check(pt.lib.pt_device_synchronize())
            assert (d_in.download(np.uint8, (nin,)) == 0x11).all() and (d_t.download(np.uint8, (nt,)) == 0x11).all(), (case[0], "wrote")
            for g, wv in zip(ps.results(k), want):
                _same_values(g, wv, f"after {case[0]}, the records")
            ps.score(d_train.ptr, corners)
            for g, wv in zip(ps.results(k), want):
                _same_values(g, wv, f"after {case[0]}, a new score")
            ps.gather(d_train.ptr, corners, d_in.ptr, d_gt=d_gt.ptr, d_targets=d_t.ptr, gt_pixel_stride=64)
            _same_tensor(d_in.download(F, want_in.shape), want_in, f"after {case[0]}, inputs")
            _same_tensor(d_t.download(F, want_t.shape), want_t, f"after {case[0]}, targets")
        assert played >= 40
    finally:
        ps.destroy()
        for d in (d_train, d_gt, d_in, d_t):
            d.free()


# ---- (f) end to end ---------------------------------------------------------------------------------------------------------

def test_training_patches_on_a_rendered_pair(pt, gpu):
    """64 x 64 Cornell at 4 spp and 256 spp, 4 patches of 16 x 16 chosen among 16 with a seeded generator."""
    w = h = 64
    p, n = 16, 4
    basis = pt.camera_basis(width=w, height=h)
    noisy, _ = pt.render_frame(w, h, 4, basis=basis)
    clean, _ = pt.render_frame(w, h, 256, basis=basis)
    inputs, targets, corners, scores = pt.training_patches(noisy, clean, patch_size=p, num_patches=n, rng=random.Random(11))
    assert inputs.shape == (n, 14, p, p) and targets.shape == (n, 3, p, p) and inputs.dtype == targets.dtype == np.float32
    assert corners.shape == (n, 2) and corners.dtype == np.int32 and scores.shape == (n,) and scores.dtype == np.float64
    assert (corners >= 0).all() and (corners <= w - p - 1).all()  # the reference's range stops one short of the last corner
    rng = random.Random(11)
    drawn = [(rng.randint(0, w - p - 1), rng.randint(0, h - p - 1)) for _ in range(4 * n)]
    chosen = [tuple(int(v) for v in c) for c in corners]
    assert all(c in drawn for c in chosen)
    want_in, want_t = pm.gather(noisy, clean, chosen, p)
    _same_tensor(inputs, want_in, "inputs")
    _same_tensor(targets, want_t, "targets")
    want = pm.scores(noisy, chosen, p)
    assert [pm.double_bits(s) for s in scores] == [pm.double_bits(r["score"]) for r in want] and (scores > 0).all()
    again = pt.training_patches(noisy, clean, patch_size=p, num_patches=n, rng=random.Random(11))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (inputs, targets, corners, scores)))
    cmp_ = pt.Compare(p, p)
    try:
        for k, (x, y) in enumerate(chosen):
            res = pt.compare_frames(np.ascontiguousarray(targets[k].transpose(1, 2, 0)), clean[y:y + p, x:x + p], compare=cmp_)
            assert res["sum_mse"] == 0 and res["mse"] == 0.0, f"patch {k}"
    finally:
        cmp_.destroy()
