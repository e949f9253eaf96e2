"""bench.py's launch contract (the launch checks need no GPU: they happen before torch or the library is touched) and its
--dump-outputs."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra, timeout=120):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)


def test_world_size_mismatch_is_an_error():
    # under a launcher with another world size the run would measure something else than it reports
    r = _run(["--gpus", "8", "--steps", "1", "--warmup", "0"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "does not match WORLD_SIZE" in (r.stderr + r.stdout)
    r = _run(["--gpus", "1", "--steps", "1", "--warmup", "0"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "does not match WORLD_SIZE" in (r.stderr + r.stdout)


def test_single_gpu_run_without_gpu_fails_loudly():
    # no CPU fallback: on a box without an MI355X the bench refuses instead of timing something else
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    r = _run(["--steps", "1", "--warmup", "0"], {})
    assert r.returncode != 0 and "no CPU path" in (r.stderr + r.stdout)


def test_dump_arguments_are_checked_before_any_work():
    r = _run(["--gpus", "2", "--dump-outputs", "unused"], {})
    assert r.returncode != 0 and "single GPU only" in r.stderr
    r = _run(["--steps", "0"], {})
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr


def test_dump_sample_is_bounded_and_fixed_by_the_shape():
    import numpy as np
    import bench
    small = np.arange(1000, dtype=np.float32).reshape(10, 25, 4)
    got, rec = bench.bounded(small, 4000)
    assert got is small and rec == {"shape": [10, 25, 4], "dtype": "float32", "sample_of": None}
    # over its budget an image is dumped as whole pixels: ascending, distinct, one of every group of `every`, from every
    # column phase, and the same ones whatever the values (the positions below are pinned: they must not move with numpy)
    a = np.arange(240_000, dtype=np.float32).reshape(300, 200, 4)
    got, rec = bench.bounded(a, 100_000)
    assert got.dtype == np.float32 and got.shape == (6000, 4) and got.nbytes <= 100_000
    assert rec == {"shape": [6000, 4], "dtype": "float32",
                   "sample_of": {"shape": [300, 200, 4], "one_row_of_every": 10, "rows": "bench.sample_rows(60000, 6250)[0]"}}
    rows, every = bench.sample_rows(60_000, 6250)
    assert every == 10 and np.array_equal(rows // 10, np.arange(6000)) and np.array_equal(got, a.reshape(-1, 4)[rows])
    assert rows[:8].tolist() == [0, 19, 23, 33, 46, 50, 60, 74] and len(set((rows % 200 % 16).tolist())) == 16
    b = np.random.default_rng(5).random((300, 200, 4), dtype=np.float32)
    assert np.array_equal(bench.bounded(b, 100_000)[0], b.reshape(-1, 4)[rows])
    # a 1-D array (depthIndex) is sampled by element; a row count that `every` does not divide ends inside the array
    d = np.arange(1001, dtype=np.float64)
    got, rec = bench.bounded(d, 8 * 250)
    assert got.shape == (201,) and rec["sample_of"]["one_row_of_every"] == 5 and got[-1] == 1000 and np.all(np.diff(got) > 0)
    assert sum(bench.DUMP_MAX_BYTES.values()) + 1024 <= 64_000_000


@pytest.mark.gpu
def test_dump_outputs_is_the_last_timed_step_and_repeats(tmp_path):
    # C2 (300 k splats, 1080p), W + K = 2 + 5 steps: the last timed step is pose 6.  Twice on the default three contexts
    # (pose 6 is on context 0; a dump taken too late, or a step too few, finds pose 3 there), and once on one context, which
    # every step renders over: a step too many leaves pose 7 there, a step too few pose 5.
    import json
    import numpy as np
    import gsplat_hip as gh
    cfg = gh.synth.CONFIGS["C2"]
    dumps = {}
    for name, extra in (("a", []), ("b", []), ("one", ["--frames-in-flight", "1"])):
        d = tmp_path / name
        r = _run(["--gpus", "1", "--steps", "5", "--warmup", "2", "--config", "C2", "--timed-only", "--dump-outputs", str(d)] + extra,
                 {}, timeout=900)   # (a whole bench process: torch's first import alone can take a minute)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == 5 and line["warmup"] == 2 and line["dropped_frames"] == 0
        assert line["dumped_outputs"] == {
            "image.npy": {"shape": [cfg["height"], cfg["width"], 4], "dtype": "float32", "sample_of": None},
            "depth_index.npy": {"shape": [cfg["n"]], "dtype": "float64", "sample_of": None}}
        assert sum(p.stat().st_size for p in d.iterdir()) <= 64_000_000
        dumps[name] = {p.name: np.load(p) for p in d.iterdir()}
        for f, rec in line["dumped_outputs"].items():
            assert list(dumps[name][f].shape) == rec["shape"] and str(dumps[name][f].dtype) == rec["dtype"]
    a, b, one = dumps["a"], dumps["b"], dumps["one"]
    assert np.array_equal(a["image.npy"], b["image.npy"]) and np.array_equal(a["depth_index.npy"], b["depth_index.npy"])
    scene = gh.Scene()
    scene.setData(gh.synth.config_rows("C2"))
    rr = gh.HIPRenderer(cfg["width"], cfg["height"], throughput=True)
    index = {}
    for k in (5, 6, 7):
        rr.render(scene, gh.orbit_camera(k, 120, cfg["width"], cfg["height"], cfg["fx"]))
        index[k] = rr.lastDepthIndex()
        if k == 6:
            image = rr.readPixelsFloat()
    rr.dispose()
    assert not np.array_equal(index[5], index[6]) and not np.array_equal(index[7], index[6])   # (its neighbours are other frames)
    for got in (a, one):
        assert np.array_equal(got["depth_index.npy"], index[6])
        assert float(np.abs(got["image.npy"] - image).max()) <= 2e-6
