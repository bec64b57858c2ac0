"""GPU: the N-rank code path of bench.py on ONE device (LCR_BENCH_SINGLE_DEVICE=1, gloo: RCCL refuses two ranks on one GPU): rank
processes started by bench.py itself, bound to their core ranges, rendezvous on 127.0.0.1, all-gather of the descriptors inside the
timed region, one JSON line from rank 0 with n_gpus = 2.  (the reference's multi-process entry is
utils/engine/base_tester.py:88.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_ranks_on_one_device():
    env = dict(os.environ, LCR_BENCH_SINGLE_DEVICE="1", LCR_BENCH_RANK_TIMEOUT="600")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--repeats", "2",
                        "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout                      # only rank 0 writes to stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 3 and line["repeats"] == 2 and line["scaling"] == "weak"
    assert line["value"] > 0 and line["ms_per_step_min"] <= line["ms_per_step"] <= line["ms_per_step_max"]
    assert "gloo" in line["config"]["parallelism"]


def test_one_rank_rccl_group_runs_the_n_rank_path():
    """LCR_BENCH_FORCE_DIST=1: a one-rank RCCL communicator, and with it everything an N-rank run does around the pipeline — barriers,
    `all_gather_into_tensor` issued on the encoder's external HIP stream inside the timed region, the max-over-ranks all-reduce of the block
    times, every secondary block — against real RCCL on this single-GPU box (two ranks on one device are refused by RCCL)."""
    env = dict(os.environ, LCR_BENCH_FORCE_DIST="1", MASTER_PORT="29631")
    env.pop("LCR_BENCH_SINGLE_DEVICE", None)
    env.pop("LCR_BENCH_BACKEND", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "1", "--repeats", "2", "--full",
                        "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["forced_one_rank_process_group"] == "nccl" and line["n_gpus"] == 1 and line["value"] > 0
    assert "nccl" in line["config"]["parallelism"]
    blocks = ["with_h2d", "descriptor_only_7_searches"]
    # the A/B block times the form the headline does NOT use (default headline: split-bf16 K-deep GEMMs)
    blocks.append("split_bf16_gemm_ab" if os.environ.get("LCR_GEMM_SPLIT", "1") in ("", "0") else "true_fp32_gemm_ab")
    assert ("bf16 x 3 split" in line["dtype"]) == (os.environ.get("LCR_GEMM_SPLIT", "1") not in ("", "0"))
    for k in blocks:
        assert line[k]["value"] > 0
    assert line["with_h2d"]["descriptors_max_abs_diff_vs_resident"] == 0.0


def test_plain_run_times_exactly_the_steps_and_dumps_the_descriptors(tmp_path):
    """A plain run (no --full) times one block of exactly --steps steps, carries the headline keys only, and --dump-outputs writes
    the last timed step's descriptors: float32 [8, 256], unit rows, the same values (1e-5) on a second run with the same arguments."""
    env = dict(os.environ)
    for k in ("LCR_BENCH_SINGLE_DEVICE", "LCR_BENCH_BACKEND", "LCR_BENCH_FORCE_DIST"):
        env.pop(k, None)
    dumps = []
    for run in range(2):
        out = tmp_path / ("run%d" % run)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                            "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in line, k
        assert line["steps"] == 5 and line["warmup"] == 2 and line["repeats"] == 1 and line["full"] is False
        assert line["value"] > 0 and abs(line["value"] - 8 * 1e3 / line["ms_per_step"]) <= 1e-3 * line["value"]
        for k in ("roofline", "cpu_baseline", "with_h2d", "pairs", "retrieval", "sequence", "descriptor_only_7_searches"):
            assert k not in line, k
        files = sorted(p.name for p in out.iterdir())
        assert files == ["descriptors.npy"], files
        d = np.load(out / "descriptors.npy")
        assert d.dtype == np.float32 and d.shape == (8, 256)
        assert np.isfinite(d).all() and np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-3)
        dumps.append(d)
    assert np.allclose(dumps[0], dumps[1], rtol=0, atol=1e-5)      # identical inputs from run to run
