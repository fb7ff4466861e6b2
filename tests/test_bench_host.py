"""bench.py's host-side pieces that need no GPU: the configuration table and the CPU-baseline leg (the oracle timed on a
bounded sample of the same workload) for the smallest configuration, whose whole frame is less CPU work than the budget."""
import sys

from conftest import ROOT

sys.path.insert(0, ROOT)


def test_configs_name_baseline_json_entries():
    import bench

    assert set(bench.CONFIGS) == {"cfg2", "cfg3", "cfg4", "cfg4open", "cfg5"}
    assert bench.CONFIGS["cfg2"]["spp"] == 1024 and bench.CONFIGS["cfg5"]["max_bounces"] == 8
    for key, c in bench.CONFIGS.items():
        assert "BASELINE.json configs[" in c["name"], key


def test_cpu_baseline_of_a_frame_smaller_than_the_budget(pt, oracle):
    import bench

    cfg = dict(bench.CONFIGS["cfg5"], width=64, height=64)  # the same shape, smaller: the band must stay inside the frame
    spheres, label = bench.scene_of(pt, cfg)
    out = bench.cpu_baseline(oracle, cfg, spheres, pt.camera_basis(width=64, height=64), 0)
    assert out["kind"] == "port" and out["value"] > 0 and out["cores"] >= 1
    assert "rows 0..63 of the 64x64 frame" in out["sample"] and "rendered" in out["sample"]
    spheres4, label4 = bench.scene_of(pt, bench.CONFIGS["cfg4open"])
    assert len(spheres4) == 1000 and "without walls" in label4


def test_dump_outputs_whole_frame_and_seeded_sample(tmp_path):
    """--dump-outputs: a frame that fits in 64 MB is written whole; a larger one as the same seeded pixel sample in every run."""
    import os

    import numpy as np

    import bench

    small = np.arange(8 * 8 * 14, dtype=np.float32).reshape(8, 8, 14)
    bench.dump_outputs(str(tmp_path / "small"), small)
    assert os.listdir(tmp_path / "small") == ["frame.npy"]
    got = np.load(tmp_path / "small" / "frame.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small)

    h, w = 2048, 1024  # 2^21 pixels x 14 floats = 117 MB, over the limit
    big = np.random.default_rng(5).random((h, w, 14), dtype=np.float32)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), big)
        assert sorted(os.listdir(tmp_path / run)) == ["frame_sample.npy", "frame_sample_index.npy"]
        assert sum(os.path.getsize(tmp_path / run / f) for f in os.listdir(tmp_path / run)) <= bench.DUMP_LIMIT_BYTES
    idx = np.load(tmp_path / "a" / "frame_sample_index.npy")
    val = np.load(tmp_path / "a" / "frame_sample.npy")
    assert idx.dtype == np.float64 and val.dtype == np.float32 and val.shape == (bench.DUMP_SAMPLE_PIXELS, 14)
    assert np.array_equal(idx, np.load(tmp_path / "b" / "frame_sample_index.npy"))
    assert np.array_equal(val, big.reshape(h * w, 14)[idx.astype(np.int64)])
