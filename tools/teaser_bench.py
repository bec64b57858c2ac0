#!/usr/bin/env python
"""TEASER-style registration (csrc/teaser.hip) on planted pairs; one JSON line per measurement, appended to --out when given.

    python tools/teaser_bench.py [--sizes 256,1024,4096] [--outliers 0.5,0.9] [--problems 1,16] [--steps 5] [--warmup 2]
                                 [--cpu-max 1024] [--eval-pairs 8] [--eval-n 1024] [--out profiles/FILE.jsonl]

Three measurements (device-synchronised wall clock around whole native calls, after warm-up):
  call   time per call of the default operator (kcore selection, the reference's parameters) at every (correspondences, outlier share,
         problems per call), with the pose error against the planted motion, and the fp64 NumPy restatement of
         tests/teaser_restatement.py on the same host for one problem (sizes up to --cpu-max: it holds N x N x 3 doubles);
  pass   time per GNC pass: `none` selection (every pair of the N rows is a measurement) with cost_threshold 0, so that exactly
         max_iterations passes run; (t(40) - t(10)) / 30 is one sweep + step.  Against it the work a pass must do: N (N - 1) / 2
         measurements x 75 fp64 operations (6 subtractions, two residuals of 23, 2 for the cost, 3 + 18 for H; the weights' compares, and
         the square root and division of the middle band, not counted) and N x 24 bytes of points per workgroup, N / 2 workgroups, all
         from L2.  The share of a default call spent in the GNC launches is (t(default) - t(max_iterations 1)) / t(default): in kcore
         mode on clean inliers the loop stops at iteration 0 and the remaining launches exit at once;
  eval   tools/registration_eval.py --method teaser against --method ransac (the reference's 0.3 m / 4 points / 50 000 iterations) on the
         same planted pair files: recall and seconds."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

FLOPS_PER_MEASUREMENT = 75


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", default="256,1024,4096")
    p.add_argument("--outliers", default="0.5,0.9")
    p.add_argument("--problems", default="1,16")
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--cpu-max", type=int, default=1024)
    p.add_argument("--eval-pairs", type=int, default=8)
    p.add_argument("--eval-n", type=int, default=1024)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    import teaser_restatement as tr
    from lcrnet_amd import functional as F
    from lcrnet_amd import io_formats as io

    dev = torch.device("cuda:0")
    sizes = [int(x) for x in args.sizes.split(",")]
    shares = [float(x) for x in args.outliers.split(",")]
    counts = [int(x) for x in args.problems.split(",")]
    date = time.strftime("%Y-%m-%d")

    def batch(n, share, S):
        n_out = int(round(n * share))
        probs = [tr.planted(n - n_out, n_out, 100 + i) for i in range(S)]
        src = torch.from_numpy(np.concatenate([q[0] for q in probs])).to(dev)
        ref = torch.from_numpy(np.concatenate([q[1] for q in probs])).to(dev)
        return probs, src, ref, torch.arange(0, S + 1, dtype=torch.int32, device=dev) * n

    for n in sizes:
        for share in shares:
            cpu_ms = None
            if n <= args.cpu_max:
                q = tr.planted(n - int(round(n * share)), int(round(n * share)), 100)
                t0 = time.perf_counter()
                tr.teaser(q[0], q[1])
                cpu_ms = (time.perf_counter() - t0) * 1e3
            for S in counts:
                probs, src, ref, start = batch(n, share, S)
                t = timed(lambda: F.teaser_registration(src, ref, start), args.steps, args.warmup)
                t1 = timed(lambda: F.teaser_registration(src, ref, start, max_iterations=1), args.steps, args.warmup)
                T, valid, nsel, rot, tc = F.teaser_registration(src, ref, start)
                T = T.cpu().numpy().astype(np.float64)
                err_R = max(np.abs(T[i, :3, :3] - q[2][:3, :3]).max() for i, q in enumerate(probs))
                err_t = max(np.abs(T[i, :3, 3] - q[2][:3, 3]).max() for i, q in enumerate(probs))
                emit({"measurement": "call", "date": date, "correspondences": n, "outlier_share": share, "problems": S,
                      "ms_per_call": t * 1e3, "ms_per_problem": t * 1e3 / S, "ms_per_call_max_iterations_1": t1 * 1e3,
                      "gnc_launch_share": max(0.0, (t - t1) / t), "valid": int(valid.sum()), "mean_selected": float(nsel.float().mean()),
                      "max_abs_rotation_error": err_R, "max_abs_translation_error_m": err_t,
                      "numpy_restatement_ms_per_problem": cpu_ms}, args.out)
        for S in counts:
            probs, src, ref, start = batch(n, 0.5, S)
            run = lambda it: F.teaser_registration(src, ref, start, inlier_selection="none", max_iterations=it, cost_threshold=0.0)
            ta, tb = timed(lambda: run(10), args.steps, args.warmup), timed(lambda: run(40), args.steps, args.warmup)
            per_pass = (tb - ta) / 30
            meas = n * (n - 1) // 2
            emit({"measurement": "pass", "date": date, "correspondences": n, "problems": S, "us_per_pass": per_pass * 1e6,
                  "measurements_per_problem": meas, "fp64_ops_per_pass": FLOPS_PER_MEASUREMENT * meas * S,
                  "fp64_gflops": FLOPS_PER_MEASUREMENT * meas * S / per_pass / 1e9,
                  "l2_bytes_per_pass": 24 * n * (n // 2) * S, "l2_gbytes_per_s": 24 * n * (n // 2) * S / per_pass / 1e9,
                  "ms_per_call_10_passes": ta * 1e3, "ms_per_call_40_passes": tb * 1e3}, args.out)

    if args.eval_pairs > 0:
        import registration_eval as reval
        with tempfile.TemporaryDirectory() as d:
            n, n_out = args.eval_n, int(round(args.eval_n * 0.9))
            for i in range(args.eval_pairs):
                src, ref, Tp, _ = tr.planted(n - n_out, n_out, 500 + i)
                pos, anc = torch.from_numpy(ref), torch.from_numpy(src)
                io.save_registration(d, 0, 100 + i, 200 + i, dict(
                    pos_points_f=pos, anc_points_f=anc, pos_points_c=pos, anc_points_c=anc, pos_corr_points=pos, anc_corr_points=anc,
                    pos_node_corr_indices=torch.zeros((0, 2), dtype=torch.int64), anc_node_corr_indices=torch.zeros((0, 2), dtype=torch.int64),
                    corr_scores=torch.ones(n), estimated_transform=torch.eye(4), pos_feature_global=torch.zeros(1, 256),
                    anc_feature_global=torch.zeros(1, 256)), Tp)
            for method in ("teaser", "ransac"):
                reval.main([d, "--method", method])                       # warm-up (library load, allocator)
                r = reval.main([d, "--method", method])
                emit({"measurement": "eval", "date": date, "method": method, "pairs": r["pairs"], "correspondences": n, "outlier_share": 0.9,
                      "RR": r["registration"]["RR"], "RRE": r["registration"]["RRE"], "RTE": r["registration"]["RTE"],
                      "seconds": r["seconds"], "detail": r.get(method)}, args.out)


if __name__ == "__main__":
    main()
