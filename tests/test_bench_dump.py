"""bench.py --dump-outputs (CPU): an output within the size budget is written whole, a larger one
as a fixed, seeded sample of its elements -- the same elements in every run, so two builds' files
compare element for element -- always flat float32, and all files of a run stay within the budget."""
import importlib.util
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("ceres_bench", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_sample_index_is_fixed_and_in_range(bench):
    assert bench.dump_sample_index(1000, 1000) is None and bench.dump_sample_index(7, 1000) is None
    a, b = bench.dump_sample_index(10_001, 500), bench.dump_sample_index(10_001, 500)
    assert a.dtype == np.int64 and a.shape == (500,) and np.array_equal(a, b)
    assert a.min() >= 0 and a.max() < 10_001 and np.all(np.diff(a) >= 0)
    assert len(np.unique(a)) > 400                                   # spread over the array, not one spot
    assert not np.array_equal(a, bench.dump_sample_index(10_002, 500))


def test_dump_writes_float32_whole_or_sampled(bench, tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 2 * 600)      # 600 elements per output (two outputs)
    rgb = (torch.arange(2 * 5 * 9, dtype=torch.int64) % 256).to(torch.uint8).view(2, 5, 9)
    px = torch.linspace(-1.0, 1.0, 5000, dtype=torch.float32)
    wrote = bench.dump_outputs(str(tmp_path / "o"), {"rgb8": rgb, "pixels": px})
    assert wrote == {"rgb8.npy": 90, "pixels.npy": 600}
    got_rgb, got_px = np.load(tmp_path / "o" / "rgb8.npy"), np.load(tmp_path / "o" / "pixels.npy")
    assert got_rgb.dtype == np.float32 and np.array_equal(got_rgb, rgb.numpy().reshape(-1).astype(np.float32))
    assert got_px.dtype == np.float32 and np.array_equal(got_px, px.numpy()[bench.dump_sample_index(5000, 600)])
    assert sum(os.path.getsize(tmp_path / "o" / f) for f in wrote) <= 4 * 2 * 600 + 2 * 128   # + .npy headers
    # a second run writes the same bytes; a rank > 0 names its files after itself and skips absent outputs
    again = bench.dump_outputs(str(tmp_path / "p"), {"rgb8": rgb, "pixels": px})
    assert again == wrote and (tmp_path / "p" / "pixels.npy").read_bytes() == (tmp_path / "o" / "pixels.npy").read_bytes()
    assert bench.dump_outputs(str(tmp_path / "q"), {"rgb8": None, "pixels": px}, rank=1, world=2) == {"pixels_rank1.npy": 300}


def test_default_budget_is_below_64_mb(bench):
    assert bench.DUMP_BUDGET_BYTES + 16 * 128 <= 64_000_000


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_reference_frames(tmp_path):
    """A plain run (no --full) on a small step -- C1, two frames, three timed steps: the line holds
    the headline fields and none of the blocks that take runs of their own, `value` is the counted
    rays of the timed steps over their time, and --dump-outputs holds the last step's frames: every
    RGB8 frame the reference's PPM body of the C1 view, the float frames equal to each other."""
    import json
    import subprocess
    import sys
    from conftest import load_golden
    meta, _, ppm = load_golden("bunny_640")
    W, H, F, K = 640, 480, 2, 3
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--config", "bunny_640",
                        "--steps", str(K), "--warmup", "1", "--frames-per-gpu", str(F), "--prime-s", "0",
                        "--dump-outputs", str(tmp_path / "d")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == K and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    for k in ("roofline", "roofline_step", "roofline_solo", "cpu_baseline", "parity"):
        assert line[k] is None, k
    assert "orbit" not in line and "orbit_value" not in line and "partition_alt" not in line
    assert line["config"]["rays_per_step"] == F * meta["ref"]["rays"]
    assert abs(line["value"] - F * meta["ref"]["rays"] / (line["ms_per_step"] * 1e3)) <= 1e-3 * line["value"]
    assert line["native"]["built_from_this_tree"] is True
    assert sorted(os.listdir(tmp_path / "d")) == ["pixels.npy", "rgb8.npy"]
    rgb, px = np.load(tmp_path / "d" / "rgb8.npy"), np.load(tmp_path / "d" / "pixels.npy")
    body = np.frombuffer(ppm["ref"][len(b"P6 %d %d 255\n" % (W, H)):], np.uint8).astype(np.float32)
    assert rgb.dtype == np.float32 and rgb.shape == (F * 3 * W * H,)
    assert all(np.array_equal(rgb[f * body.size:(f + 1) * body.size], body) for f in range(F))
    assert px.dtype == np.float32 and px.shape == (F * 3 * W * H,) and np.isfinite(px).all()
    assert np.array_equal(px[:3 * W * H].view(np.uint32), px[3 * W * H:].view(np.uint32)) and px.max() > 0
