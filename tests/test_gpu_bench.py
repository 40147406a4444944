"""-m gpu: a plain `bench.py` run on a small configuration -- exactly --steps timed steps, the result line's headline fields, and
--dump-outputs: what the last timed step computed, the same bits from run to run (the inputs are seeded)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C1", "--steps", "3", "--warmup", "2",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_run_and_its_outputs(tmp_path):
    res = _plain_run(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in res, k
    assert res["full"] is False and res["steps"] == 3 and res["warmup"] == 2 and len(res["ms_per_step_regions"]) == 1
    assert res["unit"] == "Msplats/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
    assert res["ms_per_step"] > 0 and res["value"] > 0 and res["config"]["sort_mode"] == "visible_in_flight"
    assert abs(res["value"] - 100_000 / (res["ms_per_step"] * 1e-3) / 1e6) <= 0.01 * res["value"]
    names = sorted(f[:-4] for f in os.listdir(tmp_path / "a"))
    assert names == ["frame_stats", "framebuffer", "order", "resolved", "visible_order"], names
    a = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in names}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(os.path.getsize(tmp_path / "a" / f"{k}.npy") for k in names) <= 64_000_000
    assert a["framebuffer"].shape == a["resolved"].shape == (360, 640, 4)
    assert np.array_equal(np.sort(a["order"]), np.arange(100_000))                      # 100 k splats: the whole order buffer, a permutation
    assert a["frame_stats"][0] == res["config"]["tile_pairs_P"] and a["frame_stats"][1] == res["config"]["visible_splats"]
    v = a["visible_order"]
    assert 0 < len(v) <= 100_000 and len(np.unique(v)) == len(v) and v.min() >= 0 and v.max() < 100_000 and np.array_equal(v, np.floor(v))
    assert a["resolved"][..., :3].max() > 0
    b = _plain_run(tmp_path / "b")
    for k in names:
        assert np.array_equal(a[k], np.load(tmp_path / "b" / f"{k}.npy")), k
