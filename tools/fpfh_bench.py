#!/usr/bin/env python
"""FPFH descriptor time (csrc/fpfh.hip, lcr_fpfh) at demo-scan size; one JSON line.

    python tools/fpfh_bench.py [--steps 10] [--warmup 3] [--radius 1.5] [--normal-radius 0.9] [--normal-max-nn 30] [--no-cpu]

Workload: the six committed demo scans (tests/golden/scans, voxelised at 0.3 m, ~17 k rows each) with normals from lcr_estimate_normals.
Timed (device-synchronised wall clock around whole native calls, after warm-up, workspace allocation by torch's caching allocator
included): one scan per call at max_nn 100 and 32 (mean over the six scans), and one call on 16 clouds (the six scans and rigidly turned
copies of them) at both settings.  Next to each: the same neighbour table from the radius search alone (support grid + ordered query with
limit = max_nn: the part lcr_fpfh reuses), so the remainder is what k_spfh and k_fpfh cost, and the share of rows whose ball holds more
than 512 rows (those take the search's storage-free exact path).  The CPU baseline is the fp64 NumPy restatement (tests/fpfh_restatement.py,
with the C++ oracle's radius search; one process; Open3D is not available) on the first scan, margins included."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SCANS = ["000026", "000560", "000958", "003528", "003854", "004481"]


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
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--radius", type=float, default=1.5)
    p.add_argument("--normal-radius", type=float, default=0.9)
    p.add_argument("--normal-max-nn", type=int, default=30)
    p.add_argument("--no-cpu", action="store_true")
    args = p.parse_args()
    import fpfh_restatement as fr
    from lcrnet_amd import functional as F
    from lcrnet_amd.modules.ops.radius_search import SupportGrid

    dev = torch.device("cuda:0")
    scans = [np.load(os.path.join(ROOT, "tests", "golden", "scans", s + ".npy")).astype(np.float32) for s in SCANS]
    clouds = list(scans)
    for i in range(10):                                                # 16 clouds: turned copies of the scans
        clouds.append((scans[i % 6].astype(np.float64) @ fr.rotation([0.1 * i, 0.2, 1.0], 20.0 + 15.0 * i).T).astype(np.float32))

    def prepare(cs):
        pts = torch.from_numpy(np.concatenate(cs)).to(dev)
        ln = [len(c) for c in cs]
        nrm = F.estimate_normals(pts, ln, args.normal_radius, args.normal_max_nn)["normals"]
        return pts, nrm, ln

    def search_only(pts, ln, max_nn):
        lens = torch.tensor(ln, dtype=torch.int64, device=dev)
        return SupportGrid(pts, lens, args.radius).query(pts, lens, max_nn)

    singles = [prepare([c]) for c in scans]
    batch = prepare(clouds)
    t_nrm, _ = timed(lambda: F.estimate_normals(singles[0][0], singles[0][2], args.normal_radius, args.normal_max_nn), args.steps, args.warmup)
    out = {"workload": "FPFH on the six demo scans (%d rows on average), radius %.2f m; normals r = %.2f m, max_nn %d" % (
        int(np.mean([len(c) for c in scans])), args.radius, args.normal_radius, args.normal_max_nn),
        "normals_ms_per_scan": t_nrm * 1e3, "steps": args.steps, "warmup": args.warmup}
    lens0 = torch.tensor(singles[0][2], dtype=torch.int64, device=dev)
    full = SupportGrid(singles[0][0], lens0, args.radius).query(singles[0][0], lens0, 0, want_counts=True)[1].cpu().numpy()
    out["in_radius_rows_first_scan"] = {"mean": float(full.mean()), "max": int(full.max()), "share_over_512": float((full > 512).mean())}
    for max_nn in (100, 32):
        ts, tq, m = [], [], []
        for pts, nrm, ln in singles:
            t, o = timed(lambda: F.fpfh(pts, nrm, ln, args.radius, max_nn, want_count=True), args.steps, args.warmup)
            ts.append(t)
            m.append(float(o["count"].float().mean()))
            tq.append(timed(lambda: search_only(pts, ln, max_nn), args.steps, args.warmup)[0])
        tb, ob = timed(lambda: F.fpfh(batch[0], batch[1], batch[2], args.radius, max_nn, want_count=True), args.steps, args.warmup)
        tbq, _ = timed(lambda: search_only(batch[0], batch[2], max_nn), args.steps, args.warmup)
        pairs = float(ob["count"].sum())
        out["max_nn_%d" % max_nn] = {
            "ms_per_scan": float(np.mean(ts)) * 1e3, "ms_per_scan_min": float(np.min(ts)) * 1e3, "ms_per_scan_max": float(np.max(ts)) * 1e3,
            "search_only_ms_per_scan": float(np.mean(tq)) * 1e3, "neighbours_per_row": float(np.mean(m)),
            "batch16": {"rows": int(sum(batch[2])), "ms_per_call": tb * 1e3, "ms_per_scan": tb * 1e3 / 16, "search_only_ms_per_call": tbq * 1e3,
                        "pair_features": pairs, "ns_per_pair_feature_all_in": tb * 1e9 / pairs}}
    if not args.no_cpu:
        pts, nrm, _ = singles[0]
        P, Nn = pts.cpu().numpy(), nrm.cpu().numpy()
        cpu = {}
        for max_nn in (100, 32):
            t0 = time.perf_counter()
            fr.fpfh(P, Nn, args.radius, max_nn)
            cpu["max_nn_%d_ms_per_scan" % max_nn] = (time.perf_counter() - t0) * 1e3
        cpu["what"] = "fp64 NumPy restatement + C++ oracle radius search (tests/fpfh_restatement.py), one scan, one process, margins included; Open3D absent"
        out["cpu_baseline"] = cpu
    print(json.dumps(out))


if __name__ == "__main__":
    main()
