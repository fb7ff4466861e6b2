"""pt_renderer_enqueue_frames: a batch of frames with known cameras in ONE launch (the reference's frame loop, src/main.cu:146-177,
for a scripted fly-through).  Contract: exactly the frames -- and the persisted XORWOW state afterwards (src/pathtrace.cu:212,256)
-- that the same sequence of single Render() calls produces; every frame against the frame-by-frame CPU oracle, bit for bit.

Only variant 6 has a frames kernel, and on a chip of 256 CUs the automatic policy gives tiles this small to variant 8 (which the
call then renders as the loop of single enqueues).  So the tests of the batch KERNEL ask for variant 6 and check that it ran: under
the lab library by the exact count of frames-kernel launches (Renderer.batch_launches), under the product library -- the same
sources, no diagnostics -- by the variant kernel_info reports.  The two tests that keep the automatic policy document that
fall-back."""
import numpy as np
import pytest

from test_parity_gpu import assert_bit_exact

pytestmark = pytest.mark.gpu

RNGS = pytest.mark.parametrize("rng", [0, 1], ids=["xorwow", "philox"])
SENTINEL = np.uint32(0x7FC0BEEF)  # a NaN no kernel writes: what the gaps between strided frames must still hold afterwards


def poses(pt, n, size):
    """A short fly-through: the default camera drifting and turning a little every frame."""
    bases, eyes = [], []
    for k in range(n):
        eye = (50.0 + 0.7 * k, 52.0 - 0.3 * k, 295.6 - 1.1 * k)
        bases.append(pt.camera_basis(eye, yaw=-90.0 + 0.9 * k, pitch=-0.4 * k, width=size[0], height=size[1]))
        eyes.append(eye)
    return np.asarray(bases, dtype=np.float32), np.asarray(eyes, dtype=np.float32)


# ---- the frame-by-frame oracle, computed once per configuration and shared (read-only) -------------------------------------
_REFERENCE = {}


def reference(pt, oracle, size, spp, rng, mb, n, rows=None, first_frame=0, persist=True):
    """What n single Render() calls with the cameras of poses() produce on a fresh renderer whose frame counter stands at
    first_frame: (bases, eyes, frames, states), frames[f] the oracle's frame f, states[k] the XORWOW state after k frames (None
    for the counter-based generator, and for a renderer that does not persist its state: every frame then starts from the
    seeded stream)."""
    key = (size, spp, rng, mb, n, rows, first_frame, persist)
    if key not in _REFERENCE:
        w, h = size
        rb, re_ = rows if rows else (0, h)
        bases, eyes = poses(pt, n, size)
        carried = rng == 0 and persist
        st = oracle.setup_random(w, h, row_begin=rb, row_end=re_) if carried else None
        frames, states = [], [st.copy() if carried else None]
        for f in range(n):
            frames.append(oracle.render(w, h, spp, spheres=pt.scene_cornell(), basis=bases[f], eye=eyes[f], max_bounces=mb, rng_mode=rng,
                                        row_begin=rb, row_end=re_, rng_state=st, frame=first_frame + f))
            states.append(st.copy() if carried else None)
        for a in [bases, eyes] + frames + [s for s in states if s is not None]:
            a.setflags(write=False)
        _REFERENCE[key] = (bases, eyes, tuple(frames), tuple(states))
    return _REFERENCE[key]


def batch_views(pt, lab):
    """(module, tag) of the two libraries that compile the frames kernel from the same source."""
    return ((lab, "lab"), (pt, "product"))


def variant6(mod, size, spp, rng, mb, **kw):
    """A renderer forced to variant 6 -- the one with a frames kernel; kernel_info must agree (both libraries export it)."""
    r = mod.Renderer(size[0], size[1], spp, max_bounces=mb, rng_mode=rng, variant=6, **kw)
    assert r.kernel_info(9)["variant"] == 6
    return r


def expect_launches(mod, r, want, what):
    """The exact number of frames-kernel launches so far; only the lab library can tell."""
    if mod.IS_LAB:
        assert r.batch_launches() == want, f"{what}: {r.batch_launches()} launches of the frames kernel, expected {want}"


class Strided:
    """n frames of `per` floats each, `stride` floats apart in one device buffer pre-filled with SENTINEL."""

    def __init__(self, mod, n, per, stride):
        self.n, self.per, self.stride = n, per, stride
        self.buf = mod.DeviceBuffer(n * stride * 4).upload(np.full(n * stride, SENTINEL, dtype=np.uint32))
        self.ptr = self.buf.ptr

    def download(self, shape):
        """(frames [n] + shape, gaps [n][stride - per] as uint32)"""
        raw = self.buf.download(np.float32, (self.n, self.stride))
        return np.ascontiguousarray(raw[:, :self.per]).reshape((self.n,) + shape), np.ascontiguousarray(raw[:, self.per:]).view(np.uint32)


# ---- the batch kernel itself (variant 6 forced, the launch counted) -----------------------------------------------------------
N_MAX = 35  # 32 + 3: two launches


@pytest.mark.parametrize("n,launches", [(2, 1), (3, 1), (33, 1), (35, 2)])
@pytest.mark.parametrize("mb", [5, 8])
@RNGS
@pytest.mark.parametrize("spp", [4, 1])
@pytest.mark.parametrize("size", [(72, 40), (64, 32)], ids=["72x40", "64x32"])
def test_batch_kernel_frame_counts(pt, lab, oracle, gpu, size, spp, rng, mb, n, launches):
    """72x40 = 11.25 workgroups (the last partly empty, waves straddling rows, not a power of two) and 64x32 (the power-of-two
    image path); 4 spp and 1 spp (the primary ray without jitter); 5 bounces (the build with the wall screen) and 8.  2, 3 and
    35 frames (32 + 3) are one, one and two launches; 33 is one launch and a single enqueue for the frame left over.  Every
    frame, the generator state afterwards and the single frame that follows are those of the frame-by-frame oracle."""
    w, h = size
    bases, eyes, frames, states = reference(pt, oracle, size, spp, rng, mb, N_MAX + 1)
    for mod, tag in batch_views(pt, lab):
        what = f"{tag} {w}x{h} spp {spp} rng {rng} bounces {mb} n {n}"
        r = variant6(mod, size, spp, rng, mb)
        d_scene, ns = mod.upload_scene(pt.scene_cornell())
        d_out = mod.DeviceBuffer(n * w * h * 56)
        r.enqueue_frames(d_out.ptr, w * h * 14, d_scene.ptr, ns, bases[:n], eyes[:n])
        assert r.check(wait=True) == 0
        expect_launches(mod, r, launches, what)
        got = d_out.download(np.float32, (n, h, w, 14))
        for f in range(n):
            assert_bit_exact(got[f], frames[f], f"{what}: batched frame {f}")
        if rng == 0:
            assert np.array_equal(r.get_rng_state(), states[n]), f"{what}: generator state after the batch"
        # the renderer goes on from there with single frames (frame counter and generator state are where n Render() calls leave them)
        one = mod.DeviceBuffer(w * h * 56)
        r.render(one.ptr, d_scene.ptr, ns, bases[n], eyes[n])
        assert_bit_exact(one.download(np.float32, (h, w, 14)), frames[n], f"{what}: single frame after the batch")
        expect_launches(mod, r, launches, what + " (after the single frame)")
        r.destroy()


@pytest.mark.parametrize("mb", [5, 8])
@RNGS
def test_batch_kernel_strides_and_gaps(pt, lab, oracle, gpu, rng, mb):
    """Frames 37 floats and display vertices 11 floats further apart than they are long (so only frames 0 and 4 of the five are
    16-byte aligned: the waves of the others take the plain stores), fused display pack: frames and vertices bit-exact, every
    float between them untouched."""
    size, spp, n = (72, 40), 4, 5
    w, h = size
    tile = w * h * 14
    bases, eyes, frames, _ = reference(pt, oracle, size, spp, rng, mb, N_MAX + 1)
    for mod, tag in batch_views(pt, lab):
        what = f"{tag} rng {rng} bounces {mb}"
        r = variant6(mod, size, spp, rng, mb)
        d_scene, ns = mod.upload_scene(pt.scene_cornell())
        out = Strided(mod, n, tile, tile + 37)
        vtx = Strided(mod, n, tile * 3 // 14, tile * 3 // 14 + 11)
        r.enqueue_frames(out.ptr, out.stride, d_scene.ptr, ns, bases[:n], eyes[:n], d_vertices=vtx.ptr, vtx_stride_floats=vtx.stride)
        assert r.check(wait=True) == 0
        expect_launches(mod, r, 1, what)
        got, gaps = out.download((h, w, 14))
        got_v, gaps_v = vtx.download((h, w, 3))
        for f in range(n):
            assert_bit_exact(got[f], frames[f], f"{what}: strided frame {f}")
            assert np.array_equal(got_v[f].view(np.uint32), oracle.display_pack(frames[f]).view(np.uint32)), f"{what}: display vertices of frame {f}"
        assert (gaps == SENTINEL).all(), f"{what}: the gaps between the frames were written"
        assert (gaps_v == SENTINEL).all(), f"{what}: the gaps between the display vertices were written"
        r.destroy()


@RNGS
def test_batch_kernel_on_a_ragged_row_tile(pt, lab, oracle, gpu, rng):
    """A rank's tile (rows 37..101 of a 200-wide image: waves straddle rows, the last workgroup is partly empty): 6 frames, one launch."""
    size, spp, n, rows = (200, 120), 4, 6, (37, 101)
    w, nr = size[0], rows[1] - rows[0]
    bases, eyes, frames, states = reference(pt, oracle, size, spp, rng, 8, n, rows=rows)
    for mod, tag in batch_views(pt, lab):
        r = variant6(mod, size, spp, rng, 8, row_begin=rows[0], row_end=rows[1])
        d_scene, ns = mod.upload_scene(pt.scene_cornell())
        d_out = mod.DeviceBuffer(n * nr * w * 56)
        r.enqueue_frames(d_out.ptr, nr * w * 14, d_scene.ptr, ns, bases, eyes)
        assert r.check(wait=True) == 0
        expect_launches(mod, r, 1, f"{tag} tile rng {rng}")
        got = d_out.download(np.float32, (n, nr, w, 14))
        for f in range(n):
            assert_bit_exact(got[f], frames[f], f"{tag} rng {rng}: tile frame {f}")
        if rng == 0:
            assert np.array_equal(r.get_rng_state(), states[n])
        r.destroy()


@pytest.mark.parametrize("mb", [5, 8])
@RNGS
def test_batch_kernel_continues_from_the_frame_counter_and_the_last_batch(pt, lab, oracle, gpu, rng, mb):
    """After set_frame(k) the counter-based generator's batch is keyed from k, and a second batch on the same renderer goes on
    from where the first ended (frame counter k + 3; XORWOW: the state the first batch left)."""
    size, spp, k, n1, n2 = (72, 40), 4, 1000, 3, 4
    w, h = size
    bases, eyes, frames, states = reference(pt, oracle, size, spp, rng, mb, n1 + n2, first_frame=k)
    for mod, tag in batch_views(pt, lab):
        what = f"{tag} rng {rng} bounces {mb}"
        r = variant6(mod, size, spp, rng, mb)
        r.set_frame(k)
        d_scene, ns = mod.upload_scene(pt.scene_cornell())
        d_out = mod.DeviceBuffer((n1 + n2) * w * h * 56)
        r.enqueue_frames(d_out.ptr, w * h * 14, d_scene.ptr, ns, bases[:n1], eyes[:n1])
        assert r.check(wait=True) == 0
        expect_launches(mod, r, 1, what)
        if rng == 0:
            assert np.array_equal(r.get_rng_state(), states[n1]), f"{what}: state between the batches"
        r.enqueue_frames(d_out.ptr + n1 * w * h * 56, w * h * 14, d_scene.ptr, ns, bases[n1:], eyes[n1:])
        assert r.check(wait=True) == 0
        expect_launches(mod, r, 2, what)
        got = d_out.download(np.float32, (n1 + n2, h, w, 14))
        for f in range(n1 + n2):
            assert_bit_exact(got[f], frames[f], f"{what}: frame {k} + {f}")
        if rng == 0:
            assert np.array_equal(r.get_rng_state(), states[n1 + n2])
        r.destroy()
    if rng == 1:  # (the key really depends on the counter: the same cameras from frame 0 are other frames)
        assert not np.array_equal(frames[0], reference(pt, oracle, size, spp, rng, mb, N_MAX + 1)[2][0])


@RNGS
def test_batch_without_persisted_state_starts_every_frame_from_the_seed(pt, lab, oracle, gpu, rng):
    """persist_rng = 0.  XORWOW: every single enqueue starts from the seeded stream (xorwow_init(id + seed)), a frames kernel
    that keeps the generator in its registers would let frames 1 .. n-1 draw a continuing stream -- so this renderer gets the
    loop of single enqueues (0 launches of the frames kernel).  The counter-based generator's key depends only on the frame
    counter: it stays batched (1 launch)."""
    size, spp, mb, n = (72, 40), 4, 8, 5
    w, h = size
    bases, eyes, frames, _ = reference(pt, oracle, size, spp, rng, mb, n, persist=False)
    assert not any(np.array_equal(frames[0], f) for f in frames[1:])  # (the cameras move)
    for mod, tag in batch_views(pt, lab):
        r = variant6(mod, size, spp, rng, mb, persist_rng=False)
        d_scene, ns = mod.upload_scene(pt.scene_cornell())
        d_out = mod.DeviceBuffer(n * w * h * 56)
        r.enqueue_frames(d_out.ptr, w * h * 14, d_scene.ptr, ns, bases, eyes)
        assert r.check(wait=True) == 0
        got = d_out.download(np.float32, (n, h, w, 14))
        launches = r.batch_launches() if mod.IS_LAB else None
        r.destroy()
        wrong = [f for f in range(n) if not np.array_equal(got[f].view(np.uint32), frames[f].view(np.uint32))]
        print(f"{tag} rng {rng} persist_rng 0: frames-kernel launches {launches}, frames that differ from the oracle {wrong}")
        assert not wrong, f"{tag} rng {rng}: frames {wrong} of {n} differ from the frames of single enqueues (launches of the frames kernel: {launches})"
        if mod.IS_LAB:
            assert launches == (0 if rng == 0 else 1)


@pytest.mark.parametrize("mb", [5, 8])
@RNGS
def test_batch_kernel_equals_the_loop_of_single_enqueues(pt, lab, gpu, rng, mb):
    """The sentence of include/ptcore.h without the oracle: one renderer batched (35 frames, two launches, display vertices
    fused) and a twin fed 35 single enqueues leave the same bytes and the same generator state."""
    size, spp, n = (72, 40), 4, N_MAX
    w, h = size
    bases, eyes = poses(pt, n, size)
    for mod, tag in batch_views(pt, lab):
        what = f"{tag} rng {rng} bounces {mb}"
        a, b = variant6(mod, size, spp, rng, mb), variant6(mod, size, spp, rng, mb)
        d_scene, ns = mod.upload_scene(pt.scene_cornell())
        out_a, out_b = mod.DeviceBuffer(n * w * h * 56), mod.DeviceBuffer(n * w * h * 56)
        vtx_a, vtx_b = mod.DeviceBuffer(n * w * h * 12), mod.DeviceBuffer(n * w * h * 12)
        a.enqueue_frames(out_a.ptr, w * h * 14, d_scene.ptr, ns, bases, eyes, d_vertices=vtx_a.ptr, vtx_stride_floats=w * h * 3)
        for f in range(n):
            b.set_display(vtx_b.ptr + f * w * h * 12)
            b.enqueue(out_b.ptr + f * w * h * 56, d_scene.ptr, ns, bases[f], eyes[f])
        assert a.check(wait=True) == 0 and b.check(wait=True) == 0
        expect_launches(mod, a, 2, what)
        expect_launches(mod, b, 0, what + " (the twin)")
        assert np.array_equal(out_a.download(np.uint32, (n, h, w, 14)), out_b.download(np.uint32, (n, h, w, 14))), f"{what}: frames"
        assert np.array_equal(vtx_a.download(np.uint32, (n, h, w, 3)), vtx_b.download(np.uint32, (n, h, w, 3))), f"{what}: display vertices"
        if rng == 0:
            assert np.array_equal(a.get_rng_state(), b.get_rng_state()), f"{what}: generator state"
        a.destroy()
        b.destroy()


# ---- the call under the automatic policy, and where it is the loop of single enqueues ----------------------------------------
def fallback_count(mod, r):
    """Under the automatic policy nothing is assumed about the choice -- but where it is variant 8 (every chip of 256 CUs), which
    has no frames kernel, the call must have been the loop of single enqueues."""
    if mod.IS_LAB and r.kernel_info(9)["variant"] == 8:
        assert r.batch_launches() == 0


@RNGS
@pytest.mark.parametrize("mb", [8, 5])
def test_frame_batch_under_the_automatic_policy_equals_frame_by_frame_oracle(pt, lab, oracle, gpu, rng, mb):
    """The interactive shape (config 5's kernel, smaller image), 35 frames, display vertices fused, the kernel left to the policy:
    on a full MI355X that is variant 8 for so small a tile, i.e. the loop of single enqueues."""
    w, h, spp, n = 256, 128, 4, 35
    scene = pt.scene_cornell()
    bases, eyes = poses(pt, n, (w, h))
    st = oracle.setup_random(w, h) if rng == 0 else None
    refs = [oracle.render(w, h, spp, spheres=scene, basis=bases[f], eye=eyes[f], max_bounces=mb, rng_mode=rng, rng_state=st, frame=f) for f in range(n)]
    st_n = st.copy() if rng == 0 else None
    ref_next = oracle.render(w, h, spp, spheres=scene, basis=bases[0], eye=eyes[0], max_bounces=mb, rng_mode=rng, rng_state=st, frame=n)
    for mod in (pt, lab):
        r = mod.Renderer(w, h, spp, max_bounces=mb, rng_mode=rng)
        d_scene, ns = mod.upload_scene(scene)
        d_out = mod.DeviceBuffer(n * w * h * 56)
        d_vtx = mod.DeviceBuffer(n * w * h * 12)
        r.enqueue_frames(d_out.ptr, w * h * 14, d_scene.ptr, ns, bases, eyes, d_vertices=d_vtx.ptr, vtx_stride_floats=w * h * 3)
        assert r.check(wait=True) == 0
        fallback_count(mod, r)
        got = d_out.download(np.float32, (n, h, w, 14))
        vtx = d_vtx.download(np.float32, (n, h, w, 3))
        for f in range(n):
            assert_bit_exact(got[f], refs[f], f"batched frame {f} rng {rng} bounces {mb}")
            assert np.array_equal(vtx[f].view(np.uint32), oracle.display_pack(refs[f]).view(np.uint32)), f"display vertices of frame {f}"
        if rng == 0:
            assert np.array_equal(r.get_rng_state(), st_n)
        # the renderer goes on from there with single frames (frame counter and generator state are where 35 Render() calls leave them)
        one = mod.DeviceBuffer(w * h * 56)
        r.render(one.ptr, d_scene.ptr, ns, bases[0], eyes[0])
        assert_bit_exact(one.download(np.float32, (h, w, 14)), ref_next, "single frame after the batch")
        r.destroy()


def test_frame_batch_under_the_automatic_policy_on_a_ragged_row_tile(pt, lab, oracle, gpu):
    """A rank's tile (rows 37..101 of a 200-wide image: waves straddle rows, the last workgroup is partly empty), xorwow."""
    w, h, spp, n, rb, re_ = 200, 120, 4, 6, 37, 101
    bases, eyes, frames, states = reference(pt, oracle, (w, h), spp, 0, 8, n, rows=(rb, re_))
    for mod in (pt, lab):
        r = mod.Renderer(w, h, spp, max_bounces=8, row_begin=rb, row_end=re_)
        d_scene, ns = mod.upload_scene(pt.scene_cornell())
        tile = (re_ - rb) * w
        d_out = mod.DeviceBuffer(n * tile * 56)
        r.enqueue_frames(d_out.ptr, tile * 14, d_scene.ptr, ns, bases, eyes)
        assert r.check(wait=True) == 0
        fallback_count(mod, r)
        got = d_out.download(np.float32, (n, re_ - rb, w, 14))
        for f in range(n):
            assert_bit_exact(got[f], frames[f], f"tile frame {f}")
        assert np.array_equal(r.get_rng_state(), states[n])
        r.destroy()


def test_frame_batch_falls_back_to_single_frames_elsewhere(pt, oracle, gpu):
    """No frames kernel for other scenes / kernels, and frames that share a buffer cannot be in flight together: the call is then the
    loop of single enqueues it stands for -- same results."""
    w, h, spp, n = 96, 64, 3, 4
    bases, eyes = poses(pt, n, (w, h))
    rs = np.random.default_rng(3)
    scene = pt.scene_random(40, seed=9, with_walls=True)  # variant 10's territory
    r = pt.Renderer(w, h, spp)
    d_scene, ns = pt.upload_scene(scene)
    d_out = pt.DeviceBuffer(n * w * h * 56)
    r.enqueue_frames(d_out.ptr, w * h * 14, d_scene.ptr, ns, bases, eyes)
    assert r.check(wait=True) == 0
    got = d_out.download(np.float32, (n, h, w, 14))
    st = oracle.setup_random(w, h)
    for f in range(n):
        ref = oracle.render(w, h, spp, spheres=scene, basis=bases[f], eye=eyes[f], rng_state=st)
        assert_bit_exact(got[f], ref, f"40-sphere scene frame {f}")
    r.destroy()
    # the reference's scene, every frame into the SAME buffer (stride 0): rendered one by one, the last frame stays
    scene = pt.scene_cornell()
    r = pt.Renderer(w, h, spp, max_bounces=8)
    d_scene, ns = pt.upload_scene(scene)
    r.enqueue_frames(d_out.ptr, 0, d_scene.ptr, ns, bases, eyes)
    assert r.check(wait=True) == 0
    st = oracle.setup_random(w, h)
    for f in range(n):
        ref = oracle.render(w, h, spp, spheres=scene, basis=bases[f], eye=eyes[f], max_bounces=8, rng_state=st)
    assert_bit_exact(d_out.download(np.float32, (n, h, w, 14))[0], ref, "stride 0: the last frame")
    assert np.array_equal(r.get_rng_state(), st)
    r.destroy()
    with pytest.raises(pt.PtError):
        r2 = pt.Renderer(w, h, spp)
        try:
            pt.check(pt.lib.pt_renderer_enqueue_frames(r2.handle, 2, d_out.ptr, w * h * 14, None, 0, d_scene.ptr, ns, None, None, None))
        finally:
            r2.destroy()


def test_cli_fly_through_in_batches_writes_the_same_file(pt, gpu, tmp_path):
    """pathtrace --poses FILE --batch (Renderer::RenderFrames): the saved last frame is byte for byte the file the frame-by-frame
    fly-through writes (which tests/test_parity_gpu.py holds against the oracle)."""
    import os
    import subprocess

    from conftest import ROOT

    rs = np.random.default_rng(2)
    pf = tmp_path / "poses.txt"
    pf.write_text("".join("%g %g %g %g %g\n" % (50 + rs.uniform(-5, 5), 52 + rs.uniform(-5, 5), 295.6 - 3 * k, -90 + rs.uniform(-4, 4), rs.uniform(-3, 3))
                          for k in range(37)))
    exe = os.path.join(ROOT, "cuda-pathtrace_amd", "pathtrace")
    # -s 4: the policy's own choice for a 96^2 tile (variant 8 on a full MI355X: --batch is then the loop); -s 3: below four
    # samples the policy keeps variant 6, so --batch really goes out as launches of the frames kernel
    r = pt.Renderer(96, 96, 3, max_bounces=8)
    assert r.kernel_info(9)["variant"] == 6
    r.destroy()
    for spp in ("4", "3"):
        files = []
        for extra, tag in (([], "loop"), (["--batch"], "batch")):
            out = str(tmp_path / (tag + spp))
            res = subprocess.run([exe, "--size", "96", "-s", spp, "--max-bounces", "8", "--poses", str(pf), "--nobitmap", "-o", out] + extra,
                                 capture_output=True, text=True, timeout=120)
            assert res.returncode == 0, res.stderr
            assert ("Fly-through in batches: 37 frames" in res.stdout) == bool(extra)
            files.append(open(out + ".exr", "rb").read())
        assert files[0] == files[1] and len(files[0]) > 96 * 96 * 56, f"-s {spp}"
