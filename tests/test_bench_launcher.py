"""CPU: ``bench.py --gpus N`` launches N ranks (BASELINE metric "1/2/4/8 MI355X").

* ``launch_plan``: --gpus -> the torch.distributed.run command, WORLD_SIZE cross-check, the
  refusal to measure fewer devices than asked;
* end to end: ``bench.py --gpus 2 --plumbing-check`` started without a launcher re-runs itself
  under torch.distributed.run and each rank sees RANK / LOCAL_RANK / WORLD_SIZE (gloo, no GPU);
* ``bench.py --gpus 2`` on a box with fewer GPUs exits non-zero instead of measuring one;
* ``--dump-outputs`` / ``--full``: what a dump holds, and (GPU) that a plain run prints the
  headline fields alone.
"""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _env():
    e = {k: v for k, v in os.environ.items()
         if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    e["OMP_NUM_THREADS"] = "1"
    return e


def test_launch_plan_single_gpu_runs_in_process():
    assert bench.launch_plan(1, {}, 0, []) is None
    assert bench.launch_plan(1, {"WORLD_SIZE": "1"}, 1, []) is None


def test_launch_plan_builds_torchrun_command():
    cmd = bench.launch_plan(8, {}, 8, ["--gpus", "8", "--steps", "3"], port=29511)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in cmd and "--nnodes=1" in cmd
    assert "--master-addr=127.0.0.1" in cmd and "--master-port=29511" in cmd
    i = cmd.index(os.path.abspath(bench.__file__))
    assert cmd[i + 1:] == ["--gpus", "8", "--steps", "3"]


def test_launch_plan_under_launcher_checks_world_size():
    assert bench.launch_plan(4, {"WORLD_SIZE": "4"}, 8, []) is None
    with pytest.raises(bench.LaunchError):
        bench.launch_plan(8, {"WORLD_SIZE": "1"}, 8, [])


def test_launch_plan_refuses_missing_devices():
    with pytest.raises(bench.LaunchError, match="only 1 GPU"):
        bench.launch_plan(2, {}, 1, [])
    with pytest.raises(bench.LaunchError):
        bench.launch_plan(0, {}, 8, [])


def test_bench_gpus2_spawns_two_ranks():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2",
                        "--plumbing-check"], cwd=ROOT, env=_env(), capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, r.stdout          # rank 0 only
    d = json.loads(line[0])
    assert d["n_gpus"] == 2 and d["parallelism"] == "dp2"
    assert sorted(d["ranks"]) == [0, 1] and sorted(d["local_ranks"]) == [0, 1]
    assert d["world_sizes"] == [2, 2]


def test_bench_gpus1_plumbing_unchanged():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--plumbing-check"],
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["n_gpus"] == 1 and d["ranks"] == [0]


def test_bench_refuses_more_gpus_than_visible():
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("this box has >= 2 GPUs")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"],
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=240)
    assert r.returncode == 2
    assert "GPU(s) visible" in r.stderr


@pytest.mark.gpu
def test_bench_two_rank_path_rehearsed_on_one_gpu():
    """GPU: the N > 1 bench path end to end -- torch.distributed.run, two ranks, the bucketed
    gradient all-reduce, barriers, max-over-ranks timing and the rank-0 line -- with both ranks
    on GPU 0 over gloo (FS2_BENCH_REHEARSE=1; RCCL needs one GPU per rank).  Not a
    measurement: the line says so."""
    e = _env()
    e["FS2_BENCH_REHEARSE"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={bench._free_port()}",
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--no-cpu-baseline", "--no-extractor", "--no-fp32-leg", "--no-config2-leg"]
    r = subprocess.run(cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, r.stdout          # rank 0 only
    d = json.loads(line[0])
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 64
    assert d["config"]["parallelism"] == "dp2" and "rehearsal" in d
    assert d["value"] > 0 and d["build"]["library_source_hash"] == d["build"]["tree_source_hash"]


def test_dump_outputs_writes_float32_arrays_at_fixed_positions(tmp_path, monkeypatch):
    """--dump-outputs: loss and params as float32 .npy; a flat buffer longer than DUMP_SAMPLE is
    sampled at positions that depend on its length alone, a shorter one is written whole."""
    import types
    import numpy as np
    import torch
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    loss = torch.arange(7, dtype=torch.bfloat16)
    got = {}
    for d, n in (("a", 4099), ("b", 4099), ("small", 1000)):
        m = types.SimpleNamespace(_flat=torch.arange(n, dtype=torch.float32))
        bench.dump_outputs(str(tmp_path / d), loss, m)
        assert sorted(os.listdir(tmp_path / d)) == ["loss.npy", "params.npy"]
        got[d] = {k: np.load(tmp_path / d / f"{k}.npy") for k in ("loss", "params")}
        assert all(v.dtype == np.float32 for v in got[d].values())
        assert np.array_equal(got[d]["loss"], np.arange(7, dtype=np.float32))
    p = got["a"]["params"]                                             # values = positions
    assert p.shape == (1000,) and np.all(np.diff(p) >= 0) and p[0] >= 0 and p[-1] < 4099
    assert len(np.unique(p)) > 800                                     # spread over the buffer
    assert np.array_equal(p, got["b"]["params"])
    assert np.array_equal(got["small"]["params"], np.arange(1000, dtype=np.float32))


FULL_ONLY = ("roofline", "roofline_conv1_wgrad", "kernel_ms", "host_enqueue_ms_per_step",
             "with_intensity_extractor", "fp32", "config2_b16_single_speaker_bf16", "cpu_baseline")


def test_full_is_off_by_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    assert bench.parse(["--full"]).full is True


@pytest.mark.gpu
def test_bench_plain_run_reports_the_headline_alone_and_dumps_outputs(tmp_path):
    """GPU: ``bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`` times K steps, prints the
    headline fields without any --full measurement, and writes the last step's arrays."""
    import numpy as np
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        "2", "--warmup", "1", "--batch", "2", "--dump-outputs", str(tmp_path)],
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, r.stdout
    d = json.loads(line[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "mel-frames/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["metric"].startswith("train mel-frames/sec")
    frames = d["config"]["valid_mel_frames_per_step"]
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(frames / (d["ms_per_step"] * 1e-3))
    assert not [k for k in FULL_ONLY if k in d]
    assert sorted(os.listdir(tmp_path)) == ["loss.npy", "params.npy"]
    out = {k: np.load(tmp_path / f"{k}.npy") for k in ("loss", "params")}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in out.values())
    assert out["loss"].ndim == 1 and out["loss"][0] == pytest.approx(d["loss_total_last"])
    assert out["params"].shape == (bench.DUMP_SAMPLE,)
    assert np.count_nonzero(out["params"]) > bench.DUMP_SAMPLE // 2
    assert sum(v.nbytes for v in out.values()) <= 64 << 20
