#!/usr/bin/env python
"""Correspondence RANSAC throughput (csrc/ransac.hip) at the reference's settings; one JSON line.

    python tools/ransac_bench.py [--pairs 16] [--n 4096] [--iterations 50000] [--steps 10] [--warmup 3] [--cpu-iterations 1000]

Times (device-synchronised wall clock around whole native calls, after warm-up) the batched form (all pairs in one call) and one pair per
call, and reports ms per pair, hypothesis-correspondence evaluations per second and the share of the VALU-issue bound.  The bound:
256 CUs x 4 SIMD-32 x 32 lanes x 2.4 GHz = 7.9e13 lane-instructions/s, divided by the scoring loop's vector instructions per evaluation, which are
counted in the compiled ISA of k_ransac_score (device assembly from hipcc; the unrolled main loop's v_* instructions over its
v_cmp_* count, one compare per evaluation).  The whole call (hypotheses + scoring + selection) is timed, so the share is a lower bound
for the scoring kernel's own.  CPU baseline: the fp64 NumPy restatement of tests/ransac_restatement.py (Open3D is not available), one
pair, extrapolated linearly from --cpu-iterations hypotheses — labelled as such."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LANE_INSTR_PER_S = 256 * 4 * 32 * 2.4e9


def valu_per_eval():
    """(vector instructions per evaluation, evaluations per loop trip) of k_ransac_score's main loop, from the compiled ISA."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "lcr-net_amd", "csrc", "ransac.hip")
    sys.path.insert(0, os.path.join(ROOT, "lcr-net_amd", "csrc"))
    import build as B
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "ransac.s")
        subprocess.run([hipcc] + B.FLAGS + ["--cuda-device-only", "-S", src, "-o", out], check=True, capture_output=True)
        asm = open(out).read()
    body = asm[re.search(r"^_ZN3lcr14k_ransac_score\w*:", asm, re.M).start():]
    body = body[:body.index(".Lfunc_end")]
    lines = [l.split(";")[0].strip() for l in body.splitlines()]
    best = None
    for i, l in enumerate(lines):                                  # loops: a label and a later branch back to it
        m = re.match(r"^(\.LBB\w+):$", l)
        if not m:
            continue
        for j in range(i + 1, len(lines)):
            if lines[j].startswith("s_cbranch") and lines[j].endswith(m.group(1)):
                ins = [x.split()[0] for x in lines[i + 1:j] if x and not x.startswith(".")]
                cmp_ = sum(1 for x in ins if x.startswith("v_cmp"))
                if cmp_ and any(x.startswith("ds_read") for x in ins) and not any(x.startswith("s_barrier") for x in ins):
                    nv = sum(1 for x in ins if x.startswith("v_"))
                    if best is None or cmp_ > best[1]:
                        best = (nv, cmp_)
                break
    if best is None:
        raise RuntimeError("no scoring loop found in the ISA of k_ransac_score")
    return best[0] / best[1], best[1]


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--pairs", type=int, default=16)
    p.add_argument("--n", type=int, default=4096)
    p.add_argument("--iterations", type=int, default=50000)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--cpu-iterations", type=int, default=1000)
    args = p.parse_args()
    import ransac_restatement as rr
    from lcrnet_amd import functional as F

    dev = torch.device("cuda:0")
    pairs = [rr.planted_pair(args.n, 0.7, 0.02, seed=1000 + i) for i in range(args.pairs)]
    src = torch.from_numpy(np.concatenate([q[0] for q in pairs])).to(dev)
    ref = torch.from_numpy(np.concatenate([q[1] for q in pairs])).to(dev)
    start = torch.arange(0, args.pairs + 1, dtype=torch.int32, device=dev) * args.n
    singles = [(src[i * args.n:(i + 1) * args.n], ref[i * args.n:(i + 1) * args.n]) for i in range(args.pairs)]
    one = torch.tensor([0, args.n], dtype=torch.int32, device=dev)
    run_batched = lambda: F.ransac_correspondences(src, ref, start, 0.3, 4, args.iterations)
    run_single = lambda: [F.ransac_correspondences(s, r, one, 0.3, 4, args.iterations) for s, r in singles]
    t_b = timed(run_batched, args.steps, args.warmup)
    t_s = timed(run_single, max(1, args.steps // 2), 1)
    T, inl, _, _ = run_batched()
    ok = sum(1 for i, q in enumerate(pairs) if np.abs(T[i].cpu().numpy().astype(np.float64) - q[2]).max() < 0.05)

    evals = args.pairs * args.n * args.iterations
    try:
        vpe, per_trip = valu_per_eval()
    except Exception as e:                                          # no compiler where the bench runs: report without the bound
        print("ISA count unavailable: %s" % e, file=sys.stderr)
        vpe, per_trip = None, None
    bound_s = evals * vpe / LANE_INSTR_PER_S if vpe else None

    h = max(1, min(args.cpu_iterations, args.iterations))
    t0 = time.perf_counter()
    rr.ransac(pairs[0][0], pairs[0][1], 0.3, 4, h)
    cpu_ms = (time.perf_counter() - t0) * 1e3 * args.iterations / h

    out = {"workload": "ransac %d pairs x %d correspondences x %d iterations (0.3 m, 4 points)" % (args.pairs, args.n, args.iterations),
           "batched_ms_per_pair": t_b * 1e3 / args.pairs, "batched_ms_per_call": t_b * 1e3,
           "single_ms_per_pair": t_s * 1e3 / args.pairs,
           "batched_evals_per_s": evals / t_b, "single_evals_per_s": evals / t_s,
           "valu_per_eval_isa": vpe, "evals_per_loop_trip_isa": per_trip,
           "valu_bound_ms_per_pair": bound_s * 1e3 / args.pairs if bound_s else None,
           "batched_share_of_valu_bound": bound_s / t_b if bound_s else None,
           "single_share_of_valu_bound": bound_s / t_s if bound_s else None,
           "cpu_baseline": {"what": "fp64 NumPy restatement (tests/ransac_restatement.py), one process, Open3D absent; extrapolated from %d "
                                    "iterations" % h, "ms_per_pair": cpu_ms},
           "planted_pairs_recovered": ok, "pairs": args.pairs, "steps": args.steps, "warmup": args.warmup}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
