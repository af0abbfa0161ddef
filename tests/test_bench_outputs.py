"""bench.py's plain run and --dump-outputs: the line a plain run prints, and the arrays it writes for an output-for-output
comparison of two builds (float32 .npy files, at most 64 MB, a fixed seeded sample beyond that)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("detection_boxes", "detection_scores", "detection_classes", "detection_indices", "num_valid",
         "decoded_boxes", "decoded_classes", "decoded_scores")


def _bench_module():
    spec = importlib.util.spec_from_file_location("y3_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _fake_step(B=3, N=50, M=6, seed=0):
    import torch
    rng = np.random.default_rng(seed)
    bboxes = rng.random((B, N, 4), dtype=np.float32)
    cls = rng.integers(0, 80, (B, N)).astype(np.int64)
    scores = rng.random((B, N), dtype=np.float32)
    nv = np.array([M, 2, 0][:B], np.int32)
    sel = np.stack([rng.permutation(N)[:M] for _ in range(B)]).astype(np.int32)
    packed = np.zeros((B, M, 7), np.int32)
    for b in range(B):
        for k in range(nv[b]):
            i = sel[b, k]
            packed[b, k, :4] = bboxes[b, i].view(np.int32)
            packed[b, k, 4] = scores[b, i:i + 1].view(np.int32)[0]
            packed[b, k, 5], packed[b, k, 6] = cls[b, i], i
    t = torch.from_numpy
    return (t(packed), t(nv)), (t(bboxes), t(cls), t(scores))


def test_outputs_of_step_unpacks_the_packed_rows():
    bench = _bench_module()
    gathered, decoded = _fake_step()
    got = bench.outputs_of_step(gathered, decoded)
    assert set(got) == set(NAMES)
    bboxes, cls, scores = (t.numpy() for t in decoded)
    nv = got["num_valid"]
    for b in range(len(nv)):
        idx = got["detection_indices"][b, :nv[b]]
        np.testing.assert_array_equal(got["detection_boxes"][b, :nv[b]], bboxes[b, idx])
        np.testing.assert_array_equal(got["detection_scores"][b, :nv[b]], scores[b, idx])
        np.testing.assert_array_equal(got["detection_classes"][b, :nv[b]], cls[b, idx])
        assert (got["detection_boxes"][b, nv[b]:] == 0).all()


def test_write_outputs_float32_and_seeded_sample_within_budget(tmp_path):
    bench = _bench_module()
    gathered, decoded = _fake_step()
    arrays = bench.outputs_of_step(gathered, decoded)
    full = bench.write_outputs(str(tmp_path / "a"), arrays)
    for k in NAMES:
        a = np.load(tmp_path / "a" / f"{k}.npy")
        assert a.dtype == np.float32 and a.shape == arrays[k].shape
        np.testing.assert_array_equal(a, arrays[k].astype(np.float32))
        assert full[k].shape == arrays[k].shape
    # over the budget: every array keeps the same seeded rows, the same from call to call
    big = {"x": np.arange(1000 * 64, dtype=np.float32).reshape(1000, 64), "y": np.arange(1000, dtype=np.int64)}
    budget = 64 * 1024
    s1 = bench.write_outputs(str(tmp_path / "b"), big, budget=budget)
    s2 = bench.write_outputs(str(tmp_path / "c"), big, budget=budget)
    assert sum(os.path.getsize(tmp_path / "b" / f"{k}.npy") for k in big) <= budget
    assert 0 < len(s1["y"]) < 1000 and np.array_equal(s1["x"][:, 0] / 64, s1["y"])
    for k in big:
        np.testing.assert_array_equal(np.load(tmp_path / "b" / f"{k}.npy"), np.load(tmp_path / "c" / f"{k}.npy"))


@pytest.mark.gpu
def test_bench_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """A plain run: no gate, no extra measurements, --steps timed steps, the headline fields, and the last step's outputs."""
    out = tmp_path / "dump"
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "4", "--image-size", "96",
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False and d["dtype"] == "f32"
    assert d["unit"] == "images/s" and d["higher_is_better"] is True and d["metric"].startswith("images/sec at 96x96 batch=4")
    assert d["ms_per_step"] > 0 and abs(d["value"] - 4 * 1e3 / d["ms_per_step"]) <= 0.01 * d["value"]
    assert d["parity_checked"] == 0 and "cpu_baseline" not in d and not [k for k in d if k.startswith("alt_")]
    got = {k: np.load(out / f"{k}.npy") for k in NAMES}
    assert all(a.dtype == np.float32 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["num_valid"].shape == (4,) and got["detection_boxes"].shape == (4, 100, 4)
    n = 3 * (3 * 3 + 6 * 6 + 12 * 12)
    assert got["decoded_boxes"].shape == (4, n, 4) and got["decoded_scores"].shape == (4, n)
    for b in range(4):
        nv = int(got["num_valid"][b])
        idx = got["detection_indices"][b, :nv].astype(np.int64)
        np.testing.assert_array_equal(got["detection_boxes"][b, :nv], got["decoded_boxes"][b, idx])
        np.testing.assert_array_equal(got["detection_scores"][b, :nv], got["decoded_scores"][b, idx])
    assert abs(float(got["num_valid"].mean()) - d["config"]["mean_num_valid"]) <= 0.01
