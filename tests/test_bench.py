"""bench.py's own contract: what --dump-outputs writes (CPU, on hand-made frames) and what a plain run does (GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fake_frame(B, H, W):
    g = torch.Generator().manual_seed(7)
    full = torch.rand((B, H, W, 5), generator=g)
    return {"rgb": full[..., :3], "depth": full[..., 3], "acc": full[..., 4]}      # views, as dist.TileShardedRenderer returns them


def test_dump_outputs_whole_frame(tmp_path):
    frame = fake_frame(1, 6, 9)
    bench.dump_outputs(frame, str(tmp_path / "out"))
    assert sorted(os.listdir(tmp_path / "out")) == ["acc.npy", "depth.npy", "rgb.npy"]
    for k, v in frame.items():
        a = np.load(tmp_path / "out" / f"{k}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, v.numpy())


def test_dump_outputs_seeded_sample_above_the_limit(tmp_path):
    frame = fake_frame(2, 20, 30)                                    # 1200 pixels x 5 floats = 24 000 B
    limit = 6000
    bench.dump_outputs(frame, str(tmp_path / "a"), limit=limit)
    bench.dump_outputs(frame, str(tmp_path / "b"), limit=limit)
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in frame}
    assert sum(a.nbytes for a in got.values()) <= limit
    assert got["rgb"].shape == (300, 3) and got["depth"].shape == (300, 1) and got["acc"].shape == (300, 1)
    for k in frame:                                                  # the same sample from run to run
        assert np.array_equal(got[k], np.load(tmp_path / "b" / f"{k}.npy"))
    # one pixel sample shared by all arrays: rgb, depth and acc of a row come from the same pixel
    flat = torch.cat([frame["rgb"], frame["depth"][..., None], frame["acc"][..., None]], -1).reshape(-1, 5).numpy()
    rows = np.concatenate([got["rgb"], got["depth"], got["acc"]], -1)
    idx = [int(np.flatnonzero((flat == r).all(-1))[0]) for r in rows]
    assert idx == sorted(set(idx))


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    """A plain run: the headline line with `steps` timed steps, no --full legs, and the last step's frame on disk."""
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d
    assert d["steps"] == 2 and d["higher_is_better"] is True and d["unit"] == "ray-samples/s"
    assert abs(d["value"] - 640000 * 192 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert not {"configs", "cpu_baseline", "psnr_vs_oracle_db", "strong", "in_process"} & set(d)
    shapes = {"rgb": (1, 800, 800, 3), "depth": (1, 800, 800), "acc": (1, 800, 800)}
    for k, shape in shapes.items():
        a = np.load(out_dir / f"{k}.npy")
        assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all()
