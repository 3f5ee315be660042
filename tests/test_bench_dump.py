"""bench.py --dump-outputs: what the last timed step computed, written as float32 / float64 .npy files under the 64 MB cap,
identical from run to run with the same arguments, and equal to the CPU oracle's sequence on the same seeded frames; a
plain run's line leaves everything beyond the headline to --full.
The CPU tests drive bench.py's main() on the emulated device (tests/bench_dryrun.py); the GPU test runs bench.py itself."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = ["--frames", "3", "--height", "96", "--width", "128", "--steps", "2", "--warmup", "1"]
SMALL = [*SIZE, "--no-cpu-baseline", "--no-configs", "--no-parity", "--sustained-steps", "0"]


def _run(script, args, out_dir, timeout):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), *args, "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=dict(env, OMP_NUM_THREADS="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(out_dir):
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir)) if f.endswith(".npy")}
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values()), {k: a.dtype for k, a in arrays.items()}
    return arrays


def _check_against_oracle(arrays, frames_host):
    from oracle import pylinac_oracle as o

    ref_out, ref_prof, ref_rec = o.epid_pipeline(frames_host)
    n = frames_host.shape[0]
    assert arrays["record"].shape == (n, 9) and arrays["profile"].shape == ref_prof.shape
    idx = arrays["frames_index"].astype(int)
    assert np.array_equal(arrays["frames"], ref_out[idx].astype(np.float32))
    assert np.array_equal(arrays["profile"], ref_prof)
    assert np.array_equal(arrays["record"][:, :3], ref_rec[:, :3])
    assert np.allclose(arrays["record"], ref_rec, rtol=1e-12, atol=0, equal_nan=True)
    assert np.array_equal(arrays["threshold"], ref_rec[:, 0]) and np.array_equal(arrays["fwxm"], arrays["record"][:, 1:], equal_nan=True)
    assert np.array_equal(arrays["status"], np.zeros(n))


def test_bench_dump_outputs_dry_run(tmp_path):
    """Two emulated runs with the same arguments dump the same arrays, and they are the oracle's results on the bench's
    seeded frames (seed 1000 + i); the line reports the --steps it timed."""
    from pylinac_amd.synthetic import epid_open_field_frames

    lines = [_run("tests/bench_dryrun.py", SMALL, tmp_path / d, timeout=900) for d in ("a", "b")]
    assert all(ln["steps"] == 2 and ln["ms_per_step"] > 0 for ln in lines)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
    assert set(lines[0]["dumped_outputs"]["arrays"]) == set(a)
    _check_against_oracle(a, epid_open_field_frames(3, 96, 128, seed0=1000).numpy())


def test_plain_run_leaves_extras_to_full(tmp_path):
    """Without --full the line carries the headline and its roofline only: no sustained steps, parity sample, other
    configurations or CPU baselines.  --full adds the parts it is not told to drop, and the dumped step is the same."""
    plain = _run("tests/bench_dryrun.py", SIZE, tmp_path / "a", timeout=900)
    assert plain["steps"] == 2 and plain["ms_per_step"] > 0 and "roofline" in plain
    assert not {"sustained", "parity_sample", "configs", "cpu_baseline"} & plain.keys(), plain.keys()
    full = _run("tests/bench_dryrun.py", [*SIZE, "--full", "--no-configs", "--no-cpu-baseline", "--sustained-steps", "2"],
                tmp_path / "b", timeout=900)
    assert full["sustained"]["steps"] == 2 and full["parity_sample"]["ok"] is True
    assert "configs" not in full and "cpu_baseline" not in full
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def test_dump_outputs_samples_large_outputs(tmp_path):
    """Outputs past the cap: a fixed seeded sample of whole frames (indices in frames_index.npy), total under 64 MB."""
    import bench
    from pylinac_amd.pipeline import EpidResult

    n, h, w = 40, 512, 512                       # 40 MB of frames as float32: more than the frame share of the cap
    g = torch.Generator().manual_seed(5)
    frames = torch.randint(0, 65536, (n, h, w), generator=g, dtype=torch.int32).to(torch.uint16)
    fwxm = torch.rand((n, 8), generator=g, dtype=torch.float64)
    res = EpidResult(frames, torch.rand((n, w), generator=g, dtype=torch.float64), torch.arange(n, dtype=torch.int32),
                     fwxm, torch.zeros(n, dtype=torch.int32))
    shapes = bench.dump_outputs(str(tmp_path / "a"), res, res.record())
    bench.dump_outputs(str(tmp_path / "b"), res, res.record())
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert all(np.array_equal(a[k], b[k]) for k in a) and {k: list(v.shape) for k, v in a.items()} == shapes
    idx = a["frames_index"].astype(int)
    assert 1 <= len(idx) < n and np.all(np.diff(idx) > 0)
    assert np.array_equal(a["frames"], frames.numpy()[idx].astype(np.float32))
    assert np.array_equal(a["record"], res.record().numpy()) and np.array_equal(a["profile"], res.profile.numpy())


@pytest.mark.gpu
def test_bench_dump_outputs_gpu(dev, tmp_path):
    """bench.py on the device: two runs dump the same arrays, equal to the oracle's results on the same seeded frames."""
    from pylinac_amd.synthetic import epid_open_field_frames

    args = ["--gpus", "1", "--frames", "8", "--height", "256", "--width", "256", "--steps", "3", "--warmup", "1",
            "--no-cpu-baseline", "--no-configs", "--no-parity", "--sustained-steps", "0"]
    lines = [_run("bench.py", args, tmp_path / d, timeout=600) for d in ("a", "b")]
    assert all(ln["steps"] == 3 and ln["ms_per_step"] > 0 for ln in lines)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
    _check_against_oracle(a, epid_open_field_frames(8, 256, 256, seed0=1000, device=dev).cpu().numpy())
