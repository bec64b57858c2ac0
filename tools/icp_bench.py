#!/usr/bin/env python
"""Point-to-point ICP throughput (csrc/icp.hip) on raw scans; one JSON line.

    python tools/icp_bench.py [--pairs 16] [--steps 5] [--warmup 2] [--gt-iterations 5000] [--trips 40] [--cpu]

Workload: S pairs; each target is a synthetic raw scan (lcrnet_amd.synthetic, ~120 k rays), each source a random 70 % of the target's rows
moved by a planted motion (3 deg, 0.6 m) with 1 cm noise; ICP starts 1 deg / 0.25 m off the motion, r = 0.5 m.  Timed (device-synchronised
wall clock around whole native calls, after warm-up) at Open3D's default criteria (30 iterations, 1e-6 / 1e-6) and at the ground-truth
setting of the reference's pair generators (max_iteration 5000).  Per-trip cost: calls forced to run exactly --trips iterations (relative
criteria 0: never converged, check_every 0) minus a call of 0 iterations, over --trips; that is kernel A + kernel B + two launches per trip.
Kernel A's bound: per query the candidates of its 3x3x3 cells (counted on the host with cell = r, the grid's smallest cell) times the VALU
instructions per candidate of k_icp_match's candidate loop (counted in the compiled ISA), at 256 CUs x 4 SIMD x 32 lanes x 2.4 GHz.
For the choice of one thread per query, the same queries also go through lcr_radius_query_ordered(limit = 1) (one wavefront per query).
--cpu adds the restatement's time (tests/icp_restatement.py: fp64 NumPy + the C++ oracle's radius search, one process; Open3D is not
available) for one pair at the default criteria, labelled as the CPU baseline."""
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
R = 0.5


def valu_per_candidate():
    """vector instructions per candidate (per unrolled candidate) of k_icp_match's candidate loop, from the compiled ISA"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "lcr-net_amd", "csrc", "icp.hip")
    sys.path.insert(0, os.path.join(ROOT, "lcr-net_amd", "csrc"))
    import build as B
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "icp.s")
        subprocess.run([hipcc] + B.FLAGS + ["--cuda-device-only", "-S", src, "-o", out], check=True, capture_output=True)
        asm = open(out).read()
    body = asm[re.search(r"^_ZN3lcr11k_icp_match\w*:", asm, re.M).start():]
    body = body[:body.index(".Lfunc_end")]
    lines = [l.split(";")[0].strip() for l in body.splitlines()]
    best = None                                                    # the innermost (shortest) loop with candidate loads and key compares
    for i, l in enumerate(lines):
        m = re.match(r"^(\.LBB\w+):$", l)
        if not m:
            continue
        for j in range(i + 1, len(lines)):
            if lines[j].startswith("s_cbranch") and lines[j].endswith(m.group(1)):
                ins = [x.split()[0] for x in lines[i + 1:j] if x and not x.startswith(".")]
                loads = sum(1 for x in ins if x.startswith("global_load_dwordx4"))
                keys = sum(1 for x in ins if x.startswith("v_cmp_lt_u64") or x.startswith("v_cmp_gt_u64"))
                if loads and keys == loads and (best is None or len(ins) < best[0]):
                    best = (len(ins), sum(1 for x in ins if x.startswith("v_")) / loads, loads)
                break
    if best is None:
        raise RuntimeError("no candidate loop found in the ISA of k_icp_match")
    return best[1], best[2]


def candidates_per_query(q, tgt, cell):
    """mean number of target rows in the 3x3x3 cells around each query (cells of edge `cell` anchored at the target's minimum)"""
    org = tgt.min(axis=0).astype(np.float64)
    ct = np.floor((tgt - org) / cell).astype(np.int64)
    key = lambda c: (c[:, 0] * 1_000_003 + c[:, 1]) * 1_000_033 + c[:, 2]
    uniq, cnt = np.unique(key(ct), return_counts=True)
    cq = np.floor((q.astype(np.float64) - org) / cell).astype(np.int64)
    tot = np.zeros(len(q), np.int64)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                k = key(cq + np.array([dx, dy, dz]))
                pos = np.clip(np.searchsorted(uniq, k), 0, len(uniq) - 1)
                tot += np.where(uniq[pos] == k, cnt[pos], 0)
    return float(tot.mean())


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps, out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--pairs", type=int, default=16)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--gt-iterations", type=int, default=5000)
    p.add_argument("--trips", type=int, default=40)
    p.add_argument("--cpu", action="store_true")
    args = p.parse_args()
    import icp_restatement as ir
    import lcrnet_amd.synthetic as synthetic
    from lcrnet_amd import evaluation as ev
    from lcrnet_amd import functional as F
    from lcrnet_amd.modules.ops.radius_search import SupportGrid

    dev = torch.device("cuda:0")
    tgts, srcs, motions, inits = [], [], [], []
    for i in range(args.pairs):
        tgt = synthetic.synthetic_scan(100 + i)
        motion = ir.rigid([0.05 * i, 0.1, 1.0], 3.0, [0.6, -0.2, 0.05])
        tgts.append(tgt)
        srcs.append(ir.planted_scan_pair(tgt, motion, seed=i))
        motions.append(motion)
        inits.append(motion @ np.linalg.inv(ir.rigid([0, 0, 1], 1.0, [0.2, -0.15, 0.05])))
    src = torch.from_numpy(np.concatenate(srcs)).to(dev)
    tgt = torch.from_numpy(np.concatenate(tgts)).to(dev)
    sl, tl = [len(x) for x in srcs], [len(x) for x in tgts]
    init = torch.from_numpy(np.stack(inits)).to(dev)
    call = lambda **kw: F.icp_point_to_point(src, sl, tgt, tl, init, R, **kw)

    t_def, o_def = timed(lambda: call(max_iteration=30), args.steps, args.warmup)
    t_gt, o_gt = timed(lambda: call(max_iteration=args.gt_iterations), args.steps, args.warmup)
    it_def, it_gt = o_def["iterations"].cpu().numpy(), o_gt["iterations"].cpu().numpy()
    t_forced, _ = timed(lambda: call(max_iteration=args.trips, relative_fitness=0.0, relative_rmse=0.0, check_every=0), args.steps, args.warmup)
    t_zero, _ = timed(lambda: call(max_iteration=0, check_every=0), args.steps, args.warmup)
    per_trip = (t_forced - t_zero) / args.trips
    nq = int(sum(sl))
    T_gt = o_gt["T"].cpu().numpy()
    err = [ev.compute_registration_error(m, T_gt[i])[:2] for i, m in enumerate(motions)]

    # the same queries through the wave-cooperative nearest-neighbour search (lcr_radius_query_ordered, limit = 1)
    q = torch.from_numpy(np.concatenate([ir.transform_f32(s, T_gt[i]) for i, s in enumerate(srcs)])).to(dev)
    grid = SupportGrid(tgt, torch.tensor(tl, dtype=torch.int64, device=dev), R)
    ql = torch.tensor(sl, dtype=torch.int64, device=dev)
    t_wave, _ = timed(lambda: grid.query(q, ql, 1), args.steps, args.warmup)

    cand = float(np.average([candidates_per_query(ir.transform_f32(s, T_gt[i]), tgts[i], R) for i, s in enumerate(srcs)], weights=sl))
    try:
        vpc, unroll = valu_per_candidate()
    except Exception as e:                                          # no compiler where the bench runs: report without the bound
        print("ISA count unavailable: %s" % e, file=sys.stderr)
        vpc, unroll = None, None
    bound_us = cand * vpc / LANE_INSTR_PER_S * 1e6 if vpc else None   # per query-iteration, whole chip

    out = {"workload": "icp %d pairs of synthetic raw scans (%d source / %d target rows in all), r = %.1f m" % (args.pairs, nq, int(sum(tl)), R),
           "default": {"max_iteration": 30, "ms_per_call": t_def * 1e3, "iterations_max": int(it_def.max()), "iterations_mean": float(it_def.mean()),
                       "ms_per_iteration": t_def * 1e3 / (int(it_def.max()) + 1)},
           "gt_setting": {"max_iteration": args.gt_iterations, "ms_per_call": t_gt * 1e3, "iterations_max": int(it_gt.max()),
                          "iterations_mean": float(it_gt.mean()), "ms_per_iteration": t_gt * 1e3 / (int(it_gt.max()) + 1),
                          "rre_deg_max": float(max(e[0] for e in err)), "rte_m_max": float(max(e[1] for e in err))},
           "trip_ms_all_pairs_live": per_trip * 1e3, "trip_us_per_query": per_trip * 1e6 / nq,
           "wave_per_query_nn_ms_same_queries": t_wave * 1e3,
           "candidates_per_query_est": cand, "valu_per_candidate_isa": vpc, "candidate_unroll_isa": unroll,
           "kernel_a_valu_bound_us_per_query": bound_us, "kernel_a_valu_bound_ms_per_trip": bound_us * nq / 1e3 if bound_us else None,
           "trip_share_of_bound": (bound_us * nq / 1e6) / per_trip if bound_us else None,
           "pairs": args.pairs, "steps": args.steps, "warmup": args.warmup}
    if args.cpu:
        t0 = time.perf_counter()
        r = ir.icp(srcs[0], tgts[0], R, inits[0], max_iteration=30)
        out["cpu_baseline"] = {"what": "fp64 NumPy restatement + C++ oracle radius search (tests/icp_restatement.py), one pair, one process; "
                                       "Open3D absent", "ms_per_pair": (time.perf_counter() - t0) * 1e3, "iterations": r["iterations"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
