"""`bench.py --gpus N` starts its N ranks itself (bench.py: launch_ranks) when
no launcher set WORLD_SIZE: child processes with RANK / LOCAL_RANK /
WORLD_SIZE / MASTER_* set, rendezvous on 127.0.0.1, the first failing rank
ends the others and gives the job its exit code.  The rank bodies here are the
hidden `--launch-probe` mode (a gloo all-reduce, no device), so the launcher
is checked on CPU; the GPU test checks that more ranks than visible GPUs is
refused promptly before any rank starts."""
import json
import os
import subprocess
import sys
import time

import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def _bench(args, timeout=120, env=None):
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=timeout, env=e)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_launcher_starts_n_ranks(n):
    r = _bench(["--gpus", str(n), "--launch-probe"])
    assert r.returncode == 0, r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == n
    assert line["rank_sum"] == n * (n + 1) // 2  # every rank joined the all-reduce
    assert line["master"] == "127.0.0.1"


def test_launcher_failing_rank_ends_the_job():
    """Rank 1 exits 7 while ranks 0 and 2 would sleep for minutes: the job
    must end with 7 within the launcher's grace period, not wait for them."""
    t0 = time.monotonic()
    r = _bench(["--gpus", "3", "--launch-probe", "--launch-probe-fail", "1"], timeout=90)
    assert r.returncode == 7, (r.returncode, r.stderr)
    assert time.monotonic() - t0 < 60
    assert "rank 1 of 3 exited with 7" in r.stderr


def test_gpus_mismatch_with_launcher_refused():
    r = _bench(["--gpus", "2", "--launch-probe"], env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2 and "--gpus 2" in r.stderr


def test_gpus_zero_refused():
    r = _bench(["--gpus", "0"])
    assert r.returncode == 2


def _visible_devices():
    import torch

    return torch.cuda.device_count()


def test_more_ranks_than_devices_refused_on_cpu():
    n = max(2, _visible_devices() + 1)
    t0 = time.monotonic()
    r = _bench(["--gpus", str(n), "--no-cpu"], timeout=120)
    assert r.returncode == 3, (r.returncode, r.stderr[-2000:])
    assert "visible GPUs" in r.stderr
    assert time.monotonic() - t0 < 100


@pytest.mark.gpu
def test_bench_gpus_more_than_visible_fails_fast():
    """on a 1-GPU box `bench.py --gpus 2` exits non-zero
    within a bound (no rank is started, no device is initialised)."""
    n = max(2, _visible_devices() + 1)
    t0 = time.monotonic()
    r = _bench(["--gpus", str(n), "--no-cpu", "--steps", "1", "--warmup", "0"], timeout=120)
    assert r.returncode != 0
    assert "visible GPUs" in r.stderr
    assert time.monotonic() - t0 < 100


def test_bench_options_listed():
    r = _bench(["--help"])
    assert r.returncode == 0
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_timed_frame(tmp_path):
    """A plain run (no --full) on a small frame: --steps sets the timed steps,
    the line holds ms_per_step and none of the --full legs, and --dump-outputs
    leaves the last timed frame — byte for byte the host-buffer render of the
    same scene and flags — as DIR/rgb8.npy, float32, height x width x 3."""
    import numpy as np

    from conftest import load_package

    flags = "-w 96 -r 3 -O r -A 2"
    out = tmp_path / "dump"
    r = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--flags", flags, "--dump-outputs", str(out)],
               timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["frame_check"]["bad_frames"] == 0
    for leg in ("cpu_baseline", "cpu_baseline_O0", "parity", "frame_latency_ms", "gather_check"):
        assert line[leg] is None
    assert sorted(os.listdir(out)) == ["rgb8.npy"]
    got = np.load(out / "rgb8.npy")
    pkg = load_package()
    opts = pkg.RenderOptions.from_cli(flags.split())
    host = pkg.HostScene(os.path.join(ROOT, "scenes", "trimesh2.ray"))
    ref = pkg.DeviceScene(host, 0).render(opts, want_f64=False)["rgb8"]
    assert got.dtype == np.float32 and got.shape == (host.height_for(96), 96, 3)
    assert np.array_equal(got, ref.reshape(got.shape).astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 4])
def test_bench_ranks_rehearsal_on_one_gpu(n):
    """The N-rank bench path end to end on the one-GPU box: `bench.py --gpus 2`
    with RTX_BENCH_REHEARSAL=1 starts two ranks on device 0 (gloo instead of
    RCCL, which cannot hold two ranks on one device), each renders its tile
    shard, rank 0 gathers them and prints one line with n_gpus 2 and the
    slowest rank's time; the line says it is a rehearsal."""
    t0 = time.monotonic()
    r = _bench(["--gpus", str(n), "--full", "--no-cpu", "--steps", "2", "--warmup", "1"], timeout=240,
               env={"RTX_BENCH_REHEARSAL": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["n_gpus"] == n and line["steps"] == 2
    assert line["frame_check"]["bad_frames"] == 0
    assert line["gather_check"]["rgb8_mismatch_pixels"] == 0
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert "REHEARSAL" in line["config"]["parallelism"]
    assert time.monotonic() - t0 < 240
