"""Groups of more than one frame through the denoiser's kernels, bit for bit against the float64 reference of each frame
(csrc/pt_denoise.hip: frame_of, the per-row window base iyb[i], the frame's slice of the coarse map in upsample(), the head's
f * frame_stride + pixel * ld0 store, blockIdx.y of the two pre-processing kernels, batch_plan()).  The batch tests of
tests/test_denoiser_frames_gpu.py compare the kernel with itself; here every convolution of a case runs ALONE on a group
through the lab hooks (set_activation / run_conv / activation with frames=g), on small-integer inputs that make every
accumulation exact, every frame's inputs different, so at no size is anything tolerated.

The cases and the reason for every convolution are tests/denoise_group_cases.py; tests/test_denoiser_groups_host.py shows on
the CPU that the reasons hold on the plan model and that the exactness preconditions hold on the reference.  Each case first
holds the library's conv_plan(g) to the model, field by field.  DENOISER.md, "Tests"; profiles/denoise_groups/README.md."""
import time

import numpy as np
import pytest

import denoise_exact_model as EM
import denoise_group_cases as GC
import denoise_plan_model as P
import denoise_restatement as R
from test_denoiser_frames_gpu import make_frames, singles
from test_denoiser_gpu import bits

pytestmark = pytest.mark.gpu

PT_EINVAL = -1
SENTINEL = np.float32(-1234.5)
PARAMS = GC.params()
IDS = [f"{p}-{w}x{h}-g{g}" for p, w, h, g, _, _ in PARAMS]
CONV_KEYS = ("in", "out0", "out1", "res", "up", "ks", "stride", "N", "epi")


@pytest.fixture(scope="module")
def dw(pt):
    from cuda_pathtrace_amd import denoise_weights

    return denoise_weights


def _assert_plan_is_the_model(dn, precision, w, h, g):
    """The library's layer table, convolution table and conv_plan of 1 and g frames equal the model's, field by field."""
    acts, _ = P.layers(w, h)
    assert dn.layers() == acts
    convs = dn.convs()
    for frames in (1, g):
        model = P.plan(w, h, precision, frames)
        got = dn.conv_plan(frames)
        assert len(got) == len(model) == len(convs) == 26
        for (name, info), m, p in zip(convs, model, got):
            assert name == m["name"]
            assert {k: info[k] for k in CONV_KEYS} == {k: m[k] for k in CONV_KEYS}, name
            assert {k: p[k] for k in P.PLAN_FIELDS} == {k: m[k] for k in P.PLAN_FIELDS}, (name, frames, p, m)
    ws, part = P.workspace_elements(w, h, g, precision)
    mem = dn.memory()
    assert (mem["workspace"], mem["partials"]) == (ws * mem["element"], part * 4), (mem["workspace"], mem["partials"], ws, part)


def _mismatch(what, got, ref):
    """'' or the count of differing values and the first few as (frame, y, x, channel, got, want)."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.argwhere(bits(got) != bits(ref))
    if len(bad) == 0:
        return ""
    return (f"{what}: {len(bad)} of {got.size} differ, first (frame, y, x, channel, got, want) "
            + "; ".join(f"({', '.join(map(str, b.tolist()))}, {got[tuple(b)]!r}, {ref[tuple(b)]!r})" for b in bad[:4]))


def _run_head(lab, dn, ci, g, w, h, ld, gap):
    """The head of a group into a buffer of frames `gap` floats apart beyond their pixels, full of a sentinel: ([g][h][w][3],
    whether everything but channels 0..2 of the pixels kept the sentinel)."""
    fs = w * h * ld + gap
    buf = lab.DeviceBuffer(g * fs * 4).upload(np.full(g * fs, SENTINEL, np.float32))
    try:
        dn.run_conv(ci, buf.ptr, frames=g, ld=ld, frame_stride=fs)
        out = buf.download(np.float32, (g, fs))
    finally:
        buf.free()
    px = out[:, :w * h * ld].reshape(g, h, w, ld)
    kept = bool(np.all(bits(px[..., 3:]) == bits(SENTINEL))) and bool(np.all(bits(out[:, w * h * ld:]) == bits(SENTINEL)))
    return np.ascontiguousarray(px[..., :3]), kept


@pytest.mark.parametrize("precision,w,h,g,names,reasons", PARAMS, ids=IDS)
def test_every_convolution_of_a_group_is_exact(lab, gpu, dw, precision, w, h, g, names, reasons, capsys):
    """Each listed convolution of the plan of a group of g frames of width x height, alone, every frame on its own random
    integer activations, residuals, coarse maps and albedos: every stored value of every frame equals the float64 reference of
    that frame bit for bit.  The head runs into a gapped buffer (ld = 3, and ld = 14 too where the case is the wide head's):
    the gaps and channels 3.. keep their sentinel."""
    t0 = time.perf_counter()
    half = precision == "half"
    sdi, blob = GC.integer_weights(dw, precision)
    assert GC.failed_reasons(w, h, precision, g, names, reasons) == []
    rs = np.random.default_rng(GC.seed_of(w, h, g))
    dn = lab.Denoiser(w, h, blob, max_frames=g, precision=precision)
    compared, errors, seen = 0, [], []
    try:
        assert dn.precision == precision
        _assert_plan_is_the_model(dn, precision, w, h, g)
        for ci, c in GC.rows_of(w, h, precision, g, names):
            d = GC.conv_inputs(rs, c, g, w, h, half)
            dn.set_activation(c["in"], d["x"], frames=g)
            if d["res"] is not None:
                dn.set_activation(c["res"], d["res"], frames=g)
            if d["up"] is not None:
                dn.set_activation(c["up"], d["up"], frames=g)
            if d["x0"] is not None:
                dn.set_activation(0, d["x0"], frames=g)
            refs = GC.conv_reference(dw, sdi, c, d, half)
            what = (f"{precision} {w}x{h} group {g} {c['name']} (tile {c['bm']}x{c['bn']}, {c['splits']} slices of "
                    f"{c['chunks_per_split']} of {c['nchunks']} chunks)")
            if c["epi"] == P.EPI_RGB:
                wide_head = names is not None and (c["bm"], c["bn"]) == (256, 32)
                got = []
                for ld, gap in ((3, 5), (14, 9)) if wide_head else ((3, 5),):
                    out, kept = _run_head(lab, dn, ci, g, w, h, ld, gap)
                    assert kept, f"{what}, ld {ld}: the head wrote outside channels 0..2 of its pixels"
                    got.append(out)
                refs = refs * len(got)
            else:
                dn.run_conv(ci, frames=g)
                got = [dn.activation(o, frames=g) for o in (c["out0"], c["out1"]) if o >= 0]
            assert len(got) == len(refs), c["name"]
            for k, (a, ref) in enumerate(zip(got, refs)):
                compared += a.size
                msg = _mismatch(f"{what}, output {k}", a, ref)
                if msg:
                    errors.append(msg)
            seen.append(((c["bm"], c["bn"]), c["splits"]))
    finally:
        dn.destroy()
    with capsys.disabled():
        print(f"\n{precision} {w}x{h} group {g}: {len(seen)} convolutions, {compared} values compared, {len(errors)} outputs differ; "
              f"tiles {sorted({t for t, _ in seen})}, slices {sorted({s for _, s in seen})}; {time.perf_counter() - t0:.2f} s")
    assert not errors, "\n".join(errors[:6])


def _planted_frames(w, h, g):
    """[g][h][w][14] frames of values in (0.05, 1), and in each frame the maximum of every channel 9..13 planted at the first
    pixel, the last pixel or a pixel of a later block (rotating over frames and channels), of a size that differs per frame
    and channel: a frame divided by a neighbour's maxima differs in every pixel."""
    px = w * h
    rs = np.random.default_rng(77 * w + g)
    frames = rs.uniform(0.05, 1.0, (g, px, 14)).astype(np.float32)
    spots = (0, px - 1, 256 * ((px // 256 + 1) // 2) + 77)
    assert spots[2] >= 256 and spots[2] < px - 1
    planted = np.empty((g, 5), np.float32)
    for f in range(g):
        for k in range(5):
            planted[f, k] = np.float32(3.0 + 7.0 * f + 0.37 * k)
            frames[f, spots[(f + k) % 3], 9 + k] = planted[f, k]
    return frames.reshape(g, h, w, 14), planted


@pytest.mark.parametrize("precision", P.PRECISIONS)
@pytest.mark.parametrize("w,h", GC.PRE_CASES, ids=[f"{w}x{h}" for w, h in GC.PRE_CASES])
def test_preprocessing_of_a_group_is_exact(lab, gpu, dw, precision, w, h):
    """launch_pre alone (run_pre) on groups of 3 and 61 frames, packed and gapped, in place and not: x0 of every frame (read
    through the group accessor) and, in place, channels 9..13 equal the NumPy restatement of that frame, divisor
    float32(0.00316 + float64(max)) of the frame's OWN maxima; everything else, the gaps included, is untouched."""
    half = precision == "half"
    px = w * h
    gmax = max(GC.PRE_GROUPS)
    dn = lab.Denoiser(w, h, GC.integer_weights(dw, precision)[1], max_frames=gmax, precision=precision)
    try:
        for g in GC.PRE_GROUPS:
            frames, planted = _planted_frames(w, h, g)
            ref = np.stack([R.preprocess(f) for f in frames])
            for f in range(g):
                for k in range(5):
                    assert ref[f, ..., 9 + k].max() == planted[f, k] / np.float32(0.00316 + float(planted[f, k]))
            x0_ref = np.zeros((g, h, w, 16), np.float32)
            x0_ref[..., :14] = EM.to_stored(ref, half)
            for gap in (0, 37):
                fs = px * 14 + gap
                host = np.full((g, fs), SENTINEL, np.float32)
                host[:, :px * 14] = frames.reshape(g, -1)
                for inplace in (True, False):
                    what = f"{precision} {w}x{h} group {g}, frame stride {fs}, {'in place' if inplace else 'out of place'}"
                    dn.set_activation(0, np.full((g, h, w, 16), 7.0, np.float32), frames=g)
                    d = lab.DeviceBuffer(host.nbytes).upload(host)
                    try:
                        dn.run_pre(d.ptr, g, fs, inplace)
                        after = d.download(np.float32, (g, fs))
                    finally:
                        d.free()
                    msg = _mismatch(what + ": x0", dn.activation(0, frames=g), x0_ref)
                    assert not msg, msg
                    want = frames.copy()
                    if inplace:
                        want[..., 9:14] = ref[..., 9:14]
                    msg = _mismatch(what + ": frames", after[:, :px * 14].reshape(g, h, w, 14), want)
                    assert not msg, msg
                    assert np.all(bits(after[:, px * 14:]) == bits(SENTINEL)), what + ": a gap was written"
    finally:
        dn.destroy()


@pytest.fixture(scope="module")
def real_frames(pt, gpu):
    """The frames of the end-to-end test, made once for both precisions and dropped with the module."""
    w, h, n = GC.END_TO_END
    return make_frames(pt, w, h, n)


@pytest.mark.parametrize("precision", P.PRECISIONS)
def test_a_batch_through_the_wide_tiles_equals_single_enqueues(pt, gpu, real_frames, precision):
    """The product library with real weights, 816 frames of 37 x 29 in ONE group (its plan runs 256x32, 128x64 and 128x128,
    split and unsplit): enqueue_frames equals the loop of single enqueues bit for bit, in place and out of place.  The only
    check here that sees a changed K slicing -- integer sums are exact in any order."""
    from cuda_pathtrace_amd import denoise_weights

    w, h, n = GC.END_TO_END
    tiles = {(c["bm"], c["bn"]) for c in P.plan(w, h, precision, n)}
    assert tiles >= GC.WIDE, tiles
    sd = denoise_weights.random_state_dict(seed=5)
    frames = real_frames
    one = pt.Denoiser(w, h, sd, precision=precision)
    dn = pt.Denoiser(w, h, sd, max_frames=n, precision=precision)
    try:
        want = singles(pt, one, frames, False)
        got = pt.denoise_frames(frames, None, denoiser=dn)
        msg = _mismatch(f"{precision} {w}x{h} n={n} in place", got, want)
        assert not msg, msg
        want_f, want_rgb = singles(pt, one, frames, True)
        got_f, got_rgb = pt.denoise_frames(frames, None, out_of_place=True, denoiser=dn)
        msg = _mismatch(f"{precision} {w}x{h} n={n} out of place", got_rgb, want_rgb)
        assert not msg, msg
        assert np.array_equal(bits(got_f), bits(frames)) and np.array_equal(bits(want_f), bits(frames)), "frames touched out of place"
        assert float(np.ptp(got_rgb)) > 0.0 and np.isfinite(got).all()
    finally:
        one.destroy()
        dn.destroy()


def test_the_group_hooks_refuse_bad_arguments_and_launch_nothing(lab, gpu, dw):
    """frames < 1, frames > max_frames, a head without an output buffer, a head frame_stride < width x height x ld: PT_EINVAL,
    last_enqueue() and every buffer as they were, and a valid call works afterwards."""
    w, h, g = 7, 5, 3
    px = w * h
    sdi, blob = GC.integer_weights(dw, "float32")
    dn = lab.Denoiser(w, h, blob, max_frames=g)
    frames = np.random.default_rng(5).uniform(0.05, 1.0, (g, h, w, 14)).astype(np.float32)
    d = lab.DeviceBuffer(frames.nbytes).upload(frames)
    out = lab.DeviceBuffer(g * px * 14 * 4).upload(np.full(g * px * 14, SENTINEL, np.float32))
    try:
        dn.enqueue_frames(d.ptr, g)
        lab.check(lab.lib.pt_device_synchronize())
        last = dn.last_enqueue()
        assert last[0] == 1 and last[1] > 26
        d.upload(frames)
        nl = len(dn.layers())
        before = [dn.activation(i, frames=g) for i in range(nl)]
        head = len(dn.convs()) - 1
        x = np.ones((g,) + dn.layers()[1][1], np.float32)
        calls = [
            (lambda: dn.run_conv(0, frames=0), "frames"),
            (lambda: dn.run_conv(0, frames=-2), "frames"),
            (lambda: dn.run_conv(0, frames=g + 1), "frames"),
            (lambda: dn.run_conv(head, None, frames=g), "output buffer"),
            (lambda: dn.run_conv(head, out.ptr, frames=g, ld=3, frame_stride=px * 3 - 1), "frame_stride"),
            (lambda: dn.run_conv(head, out.ptr, frames=g, ld=14, frame_stride=px * 14 - 1), "frame_stride"),
            (lambda: dn.set_activation(1, x[:1][:0], frames=0), "frames"),
            (lambda: dn.set_activation(1, np.concatenate([x, x[:1]]), frames=g + 1), "frames"),
            (lambda: dn.activation(1, frames=g + 1), "frames"),
            (lambda: dn.activation(1, frames=0), "frames"),
            (lambda: dn.run_pre(d.ptr, 0), "frames"),
            (lambda: dn.run_pre(d.ptr, g + 1), "frames"),
            (lambda: dn.run_pre(d.ptr, g, px * 14 - 1), "frame_stride"),
            (lambda: dn.run_pre(None, g), "null"),
        ]
        for call, word in calls:
            with pytest.raises(lab.PtError) as e:
                call()
            assert e.value.code == PT_EINVAL and word in str(e.value), (word, str(e.value))
            assert dn.last_enqueue() == last, word
        after = [dn.activation(i, frames=g) for i in range(nl)]
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(before, after)), "a refused call touched the workspace"
        assert np.all(bits(out.download(np.float32, (g * px * 14,))) == bits(SENTINEL)), "a refused call touched the output"
        assert np.array_equal(bits(d.download(np.float32, frames.shape)), bits(frames)), "a refused call touched the frames"
        dn.run_pre(d.ptr, g)
        dn.run_conv(head, out.ptr, frames=g, ld=14)
        assert dn.last_enqueue() == last  # the hooks are not enqueues
        rgb = out.download(np.float32, (g, h, w, 14))
        assert np.all((rgb[..., :3] >= 0.0) & (rgb[..., :3] <= 1.0)) and np.all(bits(rgb[..., 3:]) == bits(SENTINEL))
        assert not np.array_equal(bits(d.download(np.float32, frames.shape)[..., 9:14]), bits(frames[..., 9:14]))
    finally:
        d.free()
        out.free()
        dn.destroy()
