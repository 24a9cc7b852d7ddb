"""bench.py's command line: a plain run prints the headline figure only, ``--full`` adds the
per-kernel / roofline figures, and ``--dump-outputs`` writes the last timed step's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "frame_roofline", "kernel_ms_per_step", "cpu_baseline")


def run_bench(*args):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", *args],
                       cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines   # one JSON result line
    return json.loads(lines[0])


def test_dump_outputs_writes_float_arrays(tmp_path):
    import bench
    last = {"matches0": torch.tensor([[3, -1, 0]]), "mscores0": torch.tensor([[0.5, 0.0, 0.25]]),
            "cmd": torch.tensor([[1, 0, 1]], dtype=torch.uint8),
            "pose": torch.eye(3, 4, dtype=torch.float64)[None]}
    rows = torch.arange(40, dtype=torch.float64).reshape(2, 20)
    out = tmp_path / "nested" / "out"
    bench.dump_outputs(str(out), last, rows)
    assert sorted(os.listdir(out)) == ["cmd.npy", "matches0.npy", "mscores0.npy", "pose.npy",
                                       "result_rows.npy"]
    want = {"matches0": np.float64, "cmd": np.float64, "pose": np.float64,
            "mscores0": np.float32, "result_rows": np.float64}
    for name, dt in want.items():
        a = np.load(out / (name + ".npy"))
        src = rows if name == "result_rows" else last[name]
        assert a.dtype == dt and np.array_equal(a, src.numpy())
    with pytest.raises(AssertionError):   # the size limit holds over all arrays together
        bench.dump_outputs(str(out), {"big": torch.zeros(bench.DUMP_LIMIT_BYTES // 4 - 10)}, rows)


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_step(device, tmp_path):
    d = run_bench("--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path / "o"))
    assert d["steps"] == 7 and d["warmup"] == 2 and d["full"] is False
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "fp32"
    assert d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 1e-3   # one frame per step
    assert d["pose"]["frames"] == 7 and d["pose"]["status_ok"] == 1.0
    assert not any(k in d for k in FULL_ONLY)
    a = {f[:-4]: np.load(tmp_path / "o" / f) for f in os.listdir(tmp_path / "o")}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    n1, n3 = d["config"]["n1"], d["config"]["n3"]
    assert a["matches0"].shape == (1, n1) and a["matches1"].shape == (1, n3)
    assert a["mscores0"].shape == (1, n1) and a["pose"].shape == (1, 3, 4)
    # the last step's frame is one of the gathered result rows: its pose, errors, inliers
    rows = a["result_rows"]
    hit = np.flatnonzero((rows[:, :12] == a["pose"].reshape(1, 12)).all(1))
    assert len(hit) == 1
    row = rows[hit[0]]
    assert row[12] == a["R_err"][0] and row[13] == a["t_err"][0]
    assert row[17] == a["n_inliers"][0] == a["inlier_mask"].sum() and row[18] == a["status"][0] == 0
    # ... and its correspondences are the matcher outputs dumped beside it
    m0 = a["matches0"][0]
    assert a["n_correspondences"][0] == (m0 > -1).sum() > 20
    assert np.array_equal(a["matches1"][0][m0[m0 > -1].astype(int)], np.flatnonzero(m0 > -1))
    assert (a["mscores0"][0][m0 > -1] > 0).all()


@pytest.mark.gpu
def test_full_run_adds_kernel_and_roofline_figures(device):
    d = run_bench("--steps", "7", "--warmup", "2", "--full", "--no-cpu-baseline")
    assert d["steps"] == 7 and d["full"] is True and d["ms_per_step"] > 0
    assert d["roofline"]["launches_timed"] > 0 and 0 < d["roofline"]["frac"] < 1
    assert d["roofline"]["kernel"] in d["kernel_ms_per_step"]
    assert 0 < d["frame_roofline"]["frac"] < 1
    assert "cpu_baseline" not in d
