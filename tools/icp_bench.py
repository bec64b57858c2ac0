#!/usr/bin/env python
"""Point-to-point ICP throughput (csrc/icp.hip) on raw scans; one JSON line.

    python tools/icp_bench.py [--pairs 16] [--steps 5] [--warmup 2] [--gt-iterations 5000] [--trips 40] [--cpu]
                              [--estimation point_to_point|point_to_plane|both|generalized] [--normals]

Workload: S pairs; each target is a synthetic raw scan (lcrnet_amd.synthetic, ~120 k rays), each source a random 70 % of the target's rows
moved by a planted motion (3 deg, 0.6 m) with 1 cm noise; ICP starts 1 deg / 0.25 m off the motion, r = 0.5 m.  Timed (device-synchronised
wall clock around whole native calls, after warm-up) at Open3D's default criteria (30 iterations, 1e-6 / 1e-6) and at the ground-truth
setting of the reference's pair generators (max_iteration 5000).  Per-trip cost: calls forced to run exactly --trips iterations (relative
criteria 0: never converged, check_every 0) minus a call of 0 iterations, over --trips; that is kernel A + kernel B + two launches per trip.
Kernel A's bound: per query the candidates of its 3x3x3 cells (counted on the host with cell = r, the grid's smallest cell) times the VALU
instructions per candidate of k_icp_match's candidate loop (counted in the compiled ISA), at 256 CUs x 4 SIMD x 32 lanes x 2.4 GHz.
For the choice of one thread per query, the same queries also go through lcr_radius_query_ordered(limit = 1) (one wavefront per query).
--cpu adds the restatement's time (tests/icp_restatement.py: fp64 NumPy + the C++ oracle's radius search, one process; Open3D is not
available) for one pair at the default criteria, labelled as the CPU baseline.
--estimation point_to_plane / both adds an `estimators` block: at Open3D's default criteria, ms per call, mean iterations and the pose error
against the plant, per estimator (both: point-to-point and point-to-plane calls alternated, --steps each), and the per-trip cost of
point-to-plane.  Target normals come from lcr_estimate_normals on the raw targets (r = 0.5 m, max_nn 30).  Either estimator's kernel-A bound
uses the VALU count of its own candidate loop (k_icp_match, k_icp_match_plane).
--estimation generalized runs all three estimators alternated in the same way: the `estimators` block gains a `generalized` entry
(lcr_icp_generalized at epsilon 1e-3, with the per-trip cost and the VALU bound of k_icp_match_gicp) and every entry carries
ms_per_iteration (ms per call over the longest pair's iterations + 1).  Source normals (lcr_estimate_normals on the raw sources, the same
radius) are computed outside the timed calls and reported on their own as source_normals_ms_per_call.  With --cpu the generalized
restatement (tests/gicp_restatement.py, normals from the GPU) is timed for one pair.
--normals (implied by --estimation other than point_to_point) adds a `normals` block: lcr_estimate_normals per call on the 16 raw targets
(r = 0.5 m) and on the same scans voxelised at 0.3 m (r = 0.9 m), max_nn 30, the candidates per query (host count, cell = r) and the
share of rows whose ball holds max_nn rows or more (those take the radix select); with --cpu also the normals restatement's time for one
raw scan (tests/normals_restatement.py)."""
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
NORMAL_R, NORMAL_MAX_NN = 0.5, 30          # normals of the raw targets (point-to-plane, and the raw half of the normals block)
VOXEL, VOXEL_NORMAL_R = 0.3, 0.9           # the voxelised half of the normals block
GICP_EPS = 1e-3                            # Open3D's default epsilon of TransformationEstimationForGeneralizedICP


def kernel_asm(src_name, kernel):
    """the compiled ISA lines of one kernel of csrc/<src_name>"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "lcr-net_amd", "csrc", src_name)
    sys.path.insert(0, os.path.join(ROOT, "lcr-net_amd", "csrc"))
    import build as B
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([hipcc] + B.FLAGS + ["--cuda-device-only", "-S", src, "-o", out], check=True, capture_output=True)
        asm = open(out).read()
    body = asm[re.search(r"^_ZN3lcr%d%sE\w*:" % (len(kernel), kernel), asm, re.M).start():]
    body = body[:body.index(".Lfunc_end")]
    return [l.split(";")[0].strip() for l in body.splitlines()]


def loops(lines):
    """instruction mnemonics of every loop closed by a backward branch to its own label, in an ISA listing"""
    out = []
    for i, l in enumerate(lines):
        m = re.match(r"^(\.LBB\w+):$", l)
        if not m:
            continue
        for j in range(i + 1, len(lines)):
            if lines[j].startswith("s_cbranch") and lines[j].endswith(m.group(1)):
                out.append([x.split()[0] for x in lines[i + 1:j] if x and not x.startswith(".")])
                break
    return out


def valu_per_candidate(kernel="k_icp_match"):
    """vector instructions per candidate (per unrolled candidate) of an ICP match kernel's candidate loop, from the compiled ISA"""
    lines = kernel_asm("icp.hip", kernel)
    best = None                                                    # the innermost (shortest) loop with candidate loads and key compares
    for ins in loops(lines):
        loads = sum(1 for x in ins if x.startswith("global_load_dwordx4"))
        keys = sum(1 for x in ins if x.startswith("v_cmp_lt_u64") or x.startswith("v_cmp_gt_u64"))
        if loads and keys == loads and (best is None or len(ins) < best[0]):
            best = (len(ins), sum(1 for x in ins if x.startswith("v_")) / loads, loads)
    if best is None:
        raise RuntimeError("no candidate loop found in the ISA of %s" % kernel)
    return best[1], best[2]


def candidates_per_query(q, tgt, cell, per_query=False):
    """mean number of target rows in the 3x3x3 cells around each query (cells of edge `cell` anchored at the target's minimum); with
    per_query the counts themselves"""
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
    return tot if per_query else float(tot.mean())


def normals_block(args, tgts, tgt, tl, dev):
    """lcr_estimate_normals per call on the raw targets and on them voxelised"""
    from lcrnet_amd import functional as F
    from lcrnet_amd.data import voxelize_raw_scans
    vox, _, vl = voxelize_raw_scans(tgt, torch.tensor(tl, dtype=torch.int64, device=dev), VOXEL)
    vox_np = vox.cpu().numpy()
    voff = np.concatenate([[0], np.cumsum(vl)])
    out = {}
    for name, pts, lens, clouds, r in (("raw", tgt, tl, tgts, NORMAL_R),
                                       ("voxel_%.1f" % VOXEL, vox, vl, [vox_np[voff[i]:voff[i + 1]] for i in range(len(vl))], VOXEL_NORMAL_R)):
        t, o = timed(lambda: F.estimate_normals(pts, lens, r, NORMAL_MAX_NN, want_count=True), args.steps, args.warmup)
        cnt = o["count"].cpu().numpy()
        out[name] = {"rows": int(sum(lens)), "radius": r, "max_nn": NORMAL_MAX_NN, "ms_per_call": t * 1e3,
                     "share_rows_at_max_nn": float((cnt == NORMAL_MAX_NN).mean()),
                     "degenerate_share": float((o["normals"] == 0).all(1).float().mean()),
                     "candidates_per_query_est": float(np.mean(np.concatenate([candidates_per_query(c, c, r, per_query=True) for c in clouds])))}
    return out

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
    p.add_argument("--estimation", choices=["point_to_point", "point_to_plane", "both", "generalized"], default="point_to_point")
    p.add_argument("--normals", action="store_true")
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
    if args.estimation != "point_to_point" or args.normals:
        out["normals"] = normals_block(args, tgts, tgt, tl, dev)
    if args.estimation != "point_to_point":
        nrm = F.estimate_normals(tgt, tl, NORMAL_R, NORMAL_MAX_NN)["normals"]
        plane = lambda **kw: F.icp_point_to_plane(src, sl, tgt, tl, nrm, init, R, **kw)
        runs = {"point_to_point": lambda: call(max_iteration=30), "point_to_plane": lambda: plane(max_iteration=30)}
        if args.estimation == "point_to_plane":
            del runs["point_to_point"]
        if args.estimation == "generalized":
            t_sn, o_sn = timed(lambda: F.estimate_normals(src, sl, NORMAL_R, NORMAL_MAX_NN), args.steps, args.warmup)
            src_nrm = o_sn["normals"]
            gicp = lambda **kw: F.icp_generalized(src, sl, src_nrm, tgt, tl, nrm, init, R, GICP_EPS, **kw)
            runs["generalized"] = lambda: gicp(max_iteration=30)
        for _ in range(args.warmup):
            for fn in runs.values():
                fn()
        times = {k: [] for k in runs}
        res = {}
        for _ in range(args.steps):                                # alternated call by call
            for k, fn in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res[k] = fn()
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
        est = {}
        for k in runs:
            it = res[k]["iterations"].cpu().numpy()
            T = res[k]["T"].cpu().numpy()
            e = [ev.compute_registration_error(m, T[i])[:2] for i, m in enumerate(motions)]
            est[k] = {"ms_per_call_mean": float(np.mean(times[k])) * 1e3, "ms_per_call_min": float(np.min(times[k])) * 1e3,
                      "ms_per_iteration": float(np.mean(times[k])) * 1e3 / (int(it.max()) + 1),
                      "iterations_mean": float(it.mean()), "iterations_max": int(it.max()),
                      "rre_deg_max": float(max(x[0] for x in e)), "rte_m_max": float(max(x[1] for x in e)),
                      "rre_deg_mean": float(np.mean([x[0] for x in e])), "rte_m_mean": float(np.mean([x[1] for x in e]))}
        t_pf, _ = timed(lambda: plane(max_iteration=args.trips, relative_fitness=0.0, relative_rmse=0.0, check_every=0), args.steps, args.warmup)
        t_p0, _ = timed(lambda: plane(max_iteration=0, check_every=0), args.steps, args.warmup)
        est["point_to_plane"]["trip_ms_all_pairs_live"] = (t_pf - t_p0) / args.trips * 1e3
        try:
            vpp, _ = valu_per_candidate("k_icp_match_plane")
        except Exception as e:                                      # no compiler where the bench runs
            print("ISA count unavailable: %s" % e, file=sys.stderr)
            vpp = None
        est["point_to_plane"]["valu_per_candidate_isa"] = vpp
        est["point_to_plane"]["kernel_a_valu_bound_ms_per_trip"] = cand * vpp / LANE_INSTR_PER_S * nq * 1e3 if vpp else None
        if args.estimation == "generalized":
            t_gf, _ = timed(lambda: gicp(max_iteration=args.trips, relative_fitness=0.0, relative_rmse=0.0, check_every=0), args.steps, args.warmup)
            t_g0, _ = timed(lambda: gicp(max_iteration=0, check_every=0), args.steps, args.warmup)
            g = est["generalized"]
            g["epsilon"] = GICP_EPS
            g["source_normals_ms_per_call"] = t_sn * 1e3
            g["trip_ms_all_pairs_live"] = (t_gf - t_g0) / args.trips * 1e3
            g["trip_ratio_to_point_to_plane"] = g["trip_ms_all_pairs_live"] / est["point_to_plane"]["trip_ms_all_pairs_live"]
            try:
                vpg, _ = valu_per_candidate("k_icp_match_gicp")
            except Exception as e:                                  # no compiler where the bench runs
                print("ISA count unavailable: %s" % e, file=sys.stderr)
                vpg = None
            g["valu_per_candidate_isa"] = vpg
            g["kernel_a_valu_bound_ms_per_trip"] = cand * vpg / LANE_INSTR_PER_S * nq * 1e3 if vpg else None
        est["normals"] = {"radius": NORMAL_R, "max_nn": NORMAL_MAX_NN}
        out["estimators"] = est
    if args.cpu:
        t0 = time.perf_counter()
        r = ir.icp(srcs[0], tgts[0], R, inits[0], max_iteration=30)
        out["cpu_baseline"] = {"what": "fp64 NumPy restatement + C++ oracle radius search (tests/icp_restatement.py), one pair, one process; "
                                       "Open3D absent", "ms_per_pair": (time.perf_counter() - t0) * 1e3, "iterations": r["iterations"]}
        if "estimators" in out:
            import icp_plane_restatement as ipr
            n0 = nrm[:tl[0]].cpu().numpy()
            t0 = time.perf_counter()
            r = ipr.icp(srcs[0], tgts[0], n0, R, inits[0], max_iteration=30)
            out["cpu_baseline"]["point_to_plane_ms_per_pair"] = (time.perf_counter() - t0) * 1e3
            out["cpu_baseline"]["point_to_plane_iterations"] = r["iterations"]
            if args.estimation == "generalized":
                import gicp_restatement as gr
                s0 = src_nrm[:sl[0]].cpu().numpy()
                t0 = time.perf_counter()
                r = gr.icp(srcs[0], s0, tgts[0], n0, R, inits[0], eps=GICP_EPS, max_iteration=30)
                out["cpu_baseline"]["generalized_ms_per_pair"] = (time.perf_counter() - t0) * 1e3
                out["cpu_baseline"]["generalized_iterations"] = r["iterations"]
        if "normals" in out:
            import normals_restatement as nr
            t0 = time.perf_counter()
            nr.estimate_normals(tgts[0], NORMAL_R, NORMAL_MAX_NN)
            out["cpu_baseline"]["normals_ms_per_raw_scan"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
