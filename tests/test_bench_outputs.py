"""bench.py's plain run and `--dump-outputs DIR`: what the last timed step computed, written as .npy files (a fixed,
seeded sample of the filtered rows, their pixel indices, per-label sums over all rows), bounded in size, the same from
run to run; a plain run prints the headline line only (the extras are behind `--full`)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
NAMES = ("filter_out_rows.npy", "filter_out_pixels.npy", "filter_out_label_sums.npy")


def _bench():
    """bench.py as a module, without leaving its import-time environment default behind in this test process."""
    key = "HSA_ENABLE_IPC_MODE_LEGACY"
    before = os.environ.get(key)
    import bench

    if before is None:
        os.environ.pop(key, None)
    return bench


def _load(d, prefix=""):
    return [np.load(os.path.join(d, prefix + n)) for n in NAMES]


def test_dump_is_a_fixed_sample_of_the_output(tmp_path):
    bench = _bench()

    n, L = 40000, 8
    out = torch.rand((n, L), generator=torch.Generator().manual_seed(5))
    bench.dump_outputs(torch, str(tmp_path / "a"), out, 0, 0, 1)
    bench.dump_outputs(torch, str(tmp_path / "b"), out, 0, 0, 1)
    rows, pix, sums = _load(tmp_path / "a")
    for x, y in zip(_load(tmp_path / "a"), _load(tmp_path / "b")):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert rows.dtype == np.float32 and pix.dtype == np.float64 and sums.dtype == np.float64
    assert rows.shape == (bench.DUMP_ROWS, L) and pix.shape == (bench.DUMP_ROWS,) and sums.shape == (L,)
    idx = pix.astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    assert np.array_equal(rows, out.numpy()[idx])
    assert np.allclose(sums, out.double().sum(0).numpy(), rtol=1e-12, atol=0)


def test_dump_of_a_rank_names_its_files_and_offsets_its_pixels(tmp_path):
    bench = _bench()

    out = torch.arange(300 * 4, dtype=torch.float32).reshape(300, 4)
    bench.dump_outputs(torch, str(tmp_path), out, 1000, 1, 2)
    rows, pix, _ = _load(tmp_path, "rank1_")
    assert rows.shape == (300, 4) and np.array_equal(pix, np.arange(1000, 1300, dtype=np.float64))
    assert np.array_equal(rows, out.numpy())


def test_dump_stays_under_64_mb_on_every_workload():
    bench = _bench()

    for H, W, L, _ in bench.WORKLOADS.values():
        k = min(H * W, bench.DUMP_ROWS)
        assert 4 * k * L + 8 * k + 8 * L <= 64 << 20


def test_steps_must_be_positive():
    p = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--steps" in p.stderr


@pytest.mark.gpu
def test_plain_run_dumps_what_its_timed_steps_computed(tmp_path):
    """A plain run at the Tsukuba size: headline keys only, the dump equals the filter of the same seeded inputs."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--workload", "c1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0 and line["full"] is False
    assert line["unit"] == "Mpixel-labels/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    for k in ("roofline", "cpu_baseline", "mean_field_iteration", "regimes", "c1_small_image", "check"):
        assert k not in line, k
    assert sum(os.path.getsize(os.path.join(tmp_path, n)) for n in os.listdir(tmp_path)) <= 64 << 20
    rows, pix, sums = _load(tmp_path)

    import phl

    bench = _bench()

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dev = torch.device("cuda", 0)
    H, W, L, _ = bench.WORKLOADS["c1"]
    ref = torch.from_numpy(bench.synthetic_features(H, W).reshape(-1, 5)).to(dev)
    src = bench.synthetic_values(torch, H, W, L, 0, dev)
    lat = phl.Lattice(ref, reference_table=True)
    assert lat.M == line["config"]["M"]
    want = lat.filter(src)
    lat.close()
    w = want[torch.from_numpy(pix.astype(np.int64)).to(dev)].cpu().numpy()
    assert rows.shape == (min(H * W, bench.DUMP_ROWS), L)
    assert float(np.abs(rows - w).max()) <= 1e-5 * float(np.abs(w).max())
    wsum = torch.sum(want, dim=0, dtype=torch.float64).cpu().numpy()
    assert np.allclose(sums, wsum, rtol=1e-5, atol=0)
