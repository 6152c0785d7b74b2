"""bench.py's plain run, --full and --dump-outputs: the dump helper on the CPU, one tiny plain
run and one tiny --full run on the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("preprocess_ms", "kernels_ms", "pairs", "entries", "roofline", "hbm", "cpu_baseline")


def test_dump_outputs_whole_arrays(tmp_path):
    g = torch.Generator().manual_seed(1)
    arrays = {"out": torch.randn(37, 3, generator=g), "dmeans": torch.randn(11, 2, generator=g).double(),
              "half": torch.randn(5, generator=g).half(), "absent": None}
    bench.dump_outputs(str(tmp_path / "d"), arrays, torch)
    assert sorted(os.listdir(tmp_path / "d")) == ["dmeans.npy", "half.npy", "out.npy"]
    out = np.load(tmp_path / "d" / "out.npy")
    assert out.dtype == np.float32 and np.array_equal(out, arrays["out"].numpy())
    dm = np.load(tmp_path / "d" / "dmeans.npy")
    assert dm.dtype == np.float64 and np.array_equal(dm, arrays["dmeans"].numpy())
    assert np.load(tmp_path / "d" / "half.npy").dtype == np.float32


def test_dump_outputs_samples_rows_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 200_000)
    a = torch.arange(30000, dtype=torch.float32).reshape(30000, 1).repeat(1, 3)  # 360000 bytes
    b = torch.arange(20001, dtype=torch.float32)                                 # 80004 bytes
    small = torch.arange(7, dtype=torch.float32)                                 # kept whole
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), {"a": a, "b": b, "small": small}, torch)
    size = sum(os.path.getsize(tmp_path / "x" / f) for f in os.listdir(tmp_path / "x"))
    assert 150_000 < size <= 200_000
    assert np.array_equal(np.load(tmp_path / "x" / "small.npy"), small.numpy())
    for name, src in (("a", a), ("b", b)):
        x, y = np.load(tmp_path / "x" / f"{name}.npy"), np.load(tmp_path / "y" / f"{name}.npy")
        assert np.array_equal(x, y)  # the same rows from run to run
        rows = x.reshape(x.shape[0], -1)[:, 0].astype(np.int64)
        assert 0 < len(rows) < src.shape[0] and np.all(np.diff(rows) > 0)  # whole rows, ascending, distinct
        assert np.array_equal(x, src.numpy()[rows])


def _run_bench(*argv):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *argv], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


SMALL = ("--gpus", "1", "--P", "2000", "--N", "8000", "--settle-ms", "0")


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_what_the_step_returned(dgs, tmp_path):
    from diff_gaussian_sampling import synthetic as syn
    out_dir = tmp_path / "dump"
    res = _run_bench(*SMALL, "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir))
    assert all(k in res for k in CORE) and not any(k in res for k in FULL_ONLY)
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0
    assert res["unit"] == "points/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
    assert abs(res["value"] - 8000 / (res["ms_per_step"] * 1e-3)) <= 1e-9 * res["value"]
    # the same seeded inputs through the package: the forward is deterministic; the gradients are
    # float sums in no fixed order, each run within rtol 1e-5 + 1e-6 max|ref| of the exact sum
    # (tests/helpers.py), so two runs within twice that of each other
    dev = torch.device("cuda:0")
    m, v, cv, c = (t.to(dev) for t in syn.gaussians(2000, 2, 1, seed=0))
    s = syn.samples(8000, 2, seed=4).to(dev)
    dL = syn.grad_out(8000, 1, 1, seed=5).to(dev)
    for t in (m, v, c):
        t.requires_grad_(True)
    R, gb, sb, rg, srg, _ = dgs._C.preprocess_gaussians(m.detach(), v.detach(), cv, c.detach(), s, False)
    out = dgs.sample_gaussians(m, v, c, s, R, gb, sb, rg, srg, False)
    out.backward(dL.reshape(out.shape))
    assert sorted(os.listdir(out_dir)) == ["dconics.npy", "dmeans.npy", "dvalues.npy", "out.npy"]
    got = np.load(out_dir / "out.npy")
    assert got.dtype == np.float32 and np.array_equal(got, out.detach().cpu().numpy())
    for name, t in (("dmeans", m), ("dvalues", v), ("dconics", c)):
        g, ref = np.load(out_dir / f"{name}.npy"), t.grad.cpu().numpy()
        assert g.dtype == np.float32 and g.shape == ref.shape
        assert np.all(np.abs(g - ref) <= 2 * (1e-5 * np.abs(ref) + 1e-6 * np.abs(ref).max())), name


@pytest.mark.gpu
def test_full_run_keeps_every_figure(dgs):
    res = _run_bench(*SMALL, "--steps", "4", "--warmup", "1", "--full", "--cpu-samples", "64",
                     "--cpu-oracle-samples", "64", "--pre-reps", "2")
    assert all(k in res for k in CORE + FULL_ONLY)
    assert res["steps"] == 4 and res["kernels_ms"]["forward_render"] > 0 and res["kernels_ms"]["backward_render"] > 0
    assert res["pairs"]["W_live"] > 0 and res["roofline"]["frac"] > 0
    assert res["cpu_baseline"]["value"] > 0 and res["cpu_baseline_oracle"]["value"] > 0
    assert res["preprocess_resampled_ms"] > 0 and res["preprocess_alternating_ms"] > 0
