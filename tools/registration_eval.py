#!/usr/bin/env python
"""Registration evaluation over saved pair files: the counterpart of experiments/registration/eval.py.

    python tools/registration_eval.py FEATURES_DIR [--method lgr|ransac|svd|teaser|ransac_featurematch|fpfh_ransac] [--num_corr K] [--seed S]
                                      [--pairs-per-call P] [--distance-threshold 0.3] [--ransac-n 4] [--num-iterations 50000]
                                      [--write-back] [--mutual-filter] [--edge-similarity 0.9]
                                      [--refine icp|icp_plane|gicp [--icp-distance 0.5] [--icp-iterations 30]
                                                                   [--normal-radius 1.0] [--normal-max-nn 30] [--gicp-epsilon 1e-3]]
                                      [--fpfh-radius 2.5] [--fpfh-max-nn 100]
                                      [--noise-bound 0.01] [--inlier-selection kcore|none]

Reads every `{seq}_{anc}_{pos}.npz` of FEATURES_DIR (what io_formats.save_registration / demo.py write; both the pos_/anc_ and the
ref_/src_ key families of eval.py:96-110 are accepted), keeps the top --num_corr correspondences by corr_scores (:114-118), and
registers the anchor onto the positive:
  lgr     the stored `estimated_transform` (falls back to `estimated_transform_lgr`, :171-175);
  ransac  the deterministic GPU RANSAC of lcrnet_amd.registration with src = anchor, ref = positive and the reference's settings
          (config_reg.py:69-73: 0.3 m, 4 points, 50 000 iterations); --pairs-per-call pairs go into one native call;
          --write-back stores `estimated_transform_ransac` in the file as :184-185 do;
  svd     weighted Procrustes over all correspondences with corr_scores as weights (:186-193), one batched native call per group;
  teaser  eval.py:197-218 (TEASER++ with GNC-TLS rotation, noise_bound 0.01, cbar2 1, gnc factor 1.4, 100 iterations, cost threshold
          1e-12) as the GPU operator of lcrnet_amd.registration.teaser_batched states it: consistency graph, k-core selection
          (--inlier-selection none: every correspondence), GNC-TLS rotation, voted translation; --noise-bound sets the bound, pair files
          are grouped per native call as for ransac.  At most 4096 correspondences per pair enter (the best by corr_scores when a file
          holds more or --num_corr asks for more).  The JSON line carries the parameters, the number of invalid pairs (identity
          returned) and the mean number of selected correspondences;
  ransac_featurematch
          eval.py's fourth choice (utils/utils/open3d.py:109-142): every point of `anc_points_f` is matched to its exact nearest
          neighbour among `pos_feats_f` in feature space (--mutual-filter keeps only matches that point back), and the RANSAC runs on
          those correspondences with Open3D's edge-length checker (--edge-similarity, 0.9) and its distance checker at
          --distance-threshold (lcrnet_amd.registration.ransac_from_feats_batched).  Needs `pos_feats_f` / `anc_feats_f` in the pair
          files (io_formats.save_registration(..., with_feats=True)); a file without them ends the run with a non-zero exit.
  fpfh_ransac
          the learning-free baseline: normals of `anc_points_f` / `pos_points_f` (--normal-radius, --normal-max-nn, oriented toward each
          cloud's origin) -> FPFH descriptors (--fpfh-radius, --fpfh-max-nn) -> the feature-matching RANSAC above, all on the GPU
          (lcrnet_amd.registration.fpfh_ransac_batched).  Needs only `pos_points_f` / `anc_points_f` (and `transform`) in the pair
          files; where a file has no correspondences the Fine Matching line averages over the files that have.
--refine icp (opt-in) then refines every estimate by point-to-point ICP of the dense anchor cloud (`anc_points_f`) onto the positive's
(`pos_points_f`), Open3D's criteria with --icp-distance / --icp-iterations, batched on the GPU (lcrnet_amd.registration.icp_batched).
--refine icp_plane does the same with point-to-plane ICP, on normals of `pos_points_f` computed on the GPU (radius --normal-radius,
at most --normal-max-nn neighbours; lcrnet_amd.registration.estimate_normals_batched).  --refine gicp runs generalized (plane-to-plane)
ICP on normals of both `anc_points_f` and `pos_points_f` (the same radius and neighbour limit) with --gicp-epsilon (1e-3, Open3D's
default; lcrnet_amd.registration.gicp_batched).
Prints the reference's Fine Matching line (FMR / IR at acceptance_radius 0.6 with inlier_ratio_threshold 0.05, IR@0.3, IR@0.1,
num_Corr; config_reg.py:64-65) and Registration line (RR, RRE, RTE, Rx, Ry, Rz: evaluation.registration_summary), then one JSON line.
When at least one pair file carries non-empty `gt_node_corr_indices` (modules.registration.get_node_correspondences_batched stores
them before io_formats.save_registration), the reference's Coarse Matching line (NUM, PIR, RECALL, HIT_RATIO, PMR>0: eval.py:117-133,
249-255, over all pairs) comes first and its values go into the JSON line as "coarse_matching"; without labels the output is as before.
Like eval.py:92-94 the pair seq 8, anchor 15, positive 58 is skipped."""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lcrnet_amd import evaluation as ev  # noqa: E402
from lcrnet_amd import io_formats as io  # noqa: E402


def parse_name(path):
    seq, anc, pos = os.path.splitext(os.path.basename(path))[0].split("_")
    try:
        seq = int(seq)
    except ValueError:
        pass
    return seq, int(anc), int(pos)


def load_pair(path, num_corr, need_corr=True):
    d = io.load_registration(path)
    if not need_corr and not ("corr_scores" in d and ("pos_corr_points" in d or "ref_corr_points" in d)):
        return d, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0,), np.float32)
    if "pos_corr_points" in d:
        pos, anc = d["pos_corr_points"], d["anc_corr_points"]
    else:
        pos, anc = d["ref_corr_points"], d["src_corr_points"]
    scores = d["corr_scores"]
    if num_corr is not None and scores.shape[0] > num_corr:
        sel = np.argsort(-scores)[:num_corr]
        pos, anc, scores = pos[sel], anc[sel], scores[sel]
    return d, np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(anc, np.float32), np.ascontiguousarray(scores, np.float32)


def stacked(items, device):
    """[(src, ref, w)] -> device tensors stacked pair-major and the int32 [S+1] row offsets."""
    import torch
    lens = [len(s) for s, _, _ in items]
    start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cat = lambda k: torch.from_numpy(np.concatenate([it[k] for it in items]) if items else np.zeros((0, 3), np.float32)).to(device)
    return cat(0).reshape(-1, 3), cat(1).reshape(-1, 3), cat(2).reshape(-1), torch.from_numpy(start).to(device)


def estimate_group(method, items, args, device):
    """Transforms (S,4,4) float64 for a group of pairs in one native call."""
    import torch
    src, ref, w, start = stacked(items, device)
    if method == "ransac":
        from lcrnet_amd.registration import ransac_batched
        T, _, _ = ransac_batched(src, ref, start, args.distance_threshold, args.ransac_n, args.num_iterations, args.seed)
    else:
        from lcrnet_amd import functional as F
        T = F.procrustes(src, ref, w, start)
    torch.cuda.synchronize(device)
    return T.cpu().numpy().astype(np.float64)


def estimate_teaser(items, args, device):
    """TEASER-style registration for a group of pairs in one native call: (transforms (S,4,4) float64, valid [S], n_selected [S])."""
    import torch
    from lcrnet_amd.registration import teaser_batched
    src, ref, _, start = stacked(items, device)
    r = teaser_batched(src, ref, start, noise_bound=args.noise_bound, inlier_selection=args.inlier_selection,
                       max_rows=max([len(s) for s, _, _ in items] + [0]))
    torch.cuda.synchronize(device)
    return r["T"].cpu().numpy().astype(np.float64), r["valid"].cpu().numpy(), r["n_selected"].cpu().numpy()


def estimate_featurematch(group, args, device):
    """Feature-matching RANSAC for a group of pairs in one native call sequence: (transforms (S,4,4) float64, num_corr [S],
    reject codes uint8 [S, iterations])."""
    import torch
    from lcrnet_amd.registration import ransac_from_feats_batched
    pts = lambda k: [np.ascontiguousarray(d[k], np.float32).reshape(-1, 3) for _, d, _, _, _ in group]
    fts = lambda k: [np.ascontiguousarray(d[k], np.float32).reshape(len(d[k]), -1) for _, d, _, _, _ in group]
    cat = lambda xs: torch.from_numpy(np.concatenate(xs)).to(device)
    sp, rp, sf, rf = pts("anc_points_f"), pts("pos_points_f"), fts("anc_feats_f"), fts("pos_feats_f")
    r = ransac_from_feats_batched(cat(sp), cat(rp), cat(sf), cat(rf), [len(x) for x in sp], [len(x) for x in rp], args.distance_threshold,
                                  args.ransac_n, args.num_iterations, args.seed, mutual_filter=args.mutual_filter,
                                  edge_similarity=args.edge_similarity, want_reject=True)
    torch.cuda.synchronize(device)
    return (r["T"].cpu().numpy().astype(np.float64), r["num_corr"].cpu().numpy(),
            r["reject_all"].cpu().numpy().reshape(len(group), args.num_iterations))


def estimate_fpfh(group, args, device):
    """normals -> FPFH -> feature-matching RANSAC for a group of pairs: (transforms (S,4,4) float64, num_corr [S])."""
    import torch
    from lcrnet_amd.registration import fpfh_ransac_batched
    pts = lambda k: [np.ascontiguousarray(d[k], np.float32).reshape(-1, 3) for _, d, _, _, _ in group]
    cat = lambda xs: torch.from_numpy(np.concatenate(xs)).to(device)
    sp, rp = pts("anc_points_f"), pts("pos_points_f")
    r = fpfh_ransac_batched(cat(sp), [len(x) for x in sp], cat(rp), [len(x) for x in rp], args.normal_radius, args.normal_max_nn,
                            args.fpfh_radius, args.fpfh_max_nn, distance_threshold=args.distance_threshold, ransac_n=args.ransac_n,
                            num_iterations=args.num_iterations, seed=args.seed, mutual_filter=args.mutual_filter,
                            edge_similarity=args.edge_similarity)
    torch.cuda.synchronize(device)
    return r["T"].cpu().numpy().astype(np.float64), r["num_corr"].cpu().numpy()


def refine_icp(pairs, est, args, device):
    """The estimates (anchor onto positive) refined by ICP of each pair's anc_points_f onto its pos_points_f; float64 (4,4) each.
    --refine icp_plane: point-to-plane, on normals of pos_points_f estimated on the GPU first.  --refine gicp: generalized ICP, on normals
    of both clouds."""
    import torch
    from lcrnet_amd.registration import estimate_normals_batched, gicp_batched, icp_batched
    out = []
    for g in range(0, len(pairs), args.pairs_per_call):
        group = pairs[g:g + args.pairs_per_call]
        srcs = [np.ascontiguousarray(d["anc_points_f"], np.float32).reshape(-1, 3) for _, d, _, _, _ in group]
        tgts = [np.ascontiguousarray(d["pos_points_f"], np.float32).reshape(-1, 3) for _, d, _, _, _ in group]
        cat = lambda xs: torch.from_numpy(np.concatenate(xs)).to(device)
        init = torch.from_numpy(np.stack([np.asarray(T, np.float64) for T in est[g:g + args.pairs_per_call]])).to(device)
        tgt, tl = cat(tgts), [len(x) for x in tgts]
        if args.refine == "icp_plane":
            nrm = estimate_normals_batched(tgt, tl, args.normal_radius, args.normal_max_nn)["normals"]
            r = icp_batched(cat(srcs), [len(x) for x in srcs], tgt, tl, init, args.icp_distance, args.icp_iterations,
                            estimation_method="point_to_plane", tgt_normals=nrm)
        elif args.refine == "gicp":
            src, sl = cat(srcs), [len(x) for x in srcs]
            nrm = estimate_normals_batched(tgt, tl, args.normal_radius, args.normal_max_nn)["normals"]
            src_nrm = estimate_normals_batched(src, sl, args.normal_radius, args.normal_max_nn)["normals"]
            r = gicp_batched(src, sl, src_nrm, tgt, tl, nrm, init, args.icp_distance, args.gicp_epsilon, args.icp_iterations)
        else:
            r = icp_batched(cat(srcs), [len(x) for x in srcs], tgt, tl, init, args.icp_distance, args.icp_iterations)
        out += list(r["T"].cpu().numpy())
    return out


def coarse_block(dicts):
    """The coarse-matching block (eval.py:117-133, 249-255) over the loaded pair files, or None when none of them carries labels."""
    labelled = [d for d in dicts if "gt_node_corr_indices" in d and np.asarray(d["gt_node_corr_indices"]).shape[0] > 0]
    if not labelled:
        return None
    nums, ms = [], []
    for d in dicts:
        fam = "pos" if "pos_node_corr_indices" in d else "ref"
        side = {"pos": "anc", "ref": "src"}[fam]
        gt = d["gt_node_corr_indices"] if "gt_node_corr_indices" in d else np.zeros((0, 2), np.int64)
        ms.append(ev.coarse_matching_metrics(d[fam + "_points_c"], d[side + "_points_c"], d[fam + "_node_corr_indices"],
                                             d[side + "_node_corr_indices"], gt))
        nums.append(np.asarray(d[fam + "_node_corr_indices"]).shape[0])
    return ev.coarse_matching_summary(nums, ms)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("features_dir")
    p.add_argument("--method", choices=["lgr", "ransac", "svd", "teaser", "ransac_featurematch", "fpfh_ransac"], default="lgr")
    p.add_argument("--num_corr", type=int, default=None)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--pairs-per-call", type=int, default=16)
    p.add_argument("--distance-threshold", type=float, default=0.3)
    p.add_argument("--ransac-n", type=int, default=4)
    p.add_argument("--num-iterations", type=int, default=50000)
    p.add_argument("--write-back", action="store_true", help="store estimated_transform_ransac in each file (eval.py:184-185)")
    p.add_argument("--mutual-filter", action="store_true", help="ransac_featurematch: keep only mutual nearest neighbours")
    p.add_argument("--edge-similarity", type=float, default=0.9, help="ransac_featurematch: edge-length checker (<= 0: off)")
    p.add_argument("--refine", choices=["icp", "icp_plane", "gicp"], default=None,
                   help="refine each estimate by point-to-point (icp), point-to-plane (icp_plane) or generalized (gicp) ICP of the dense clouds")
    p.add_argument("--icp-distance", type=float, default=0.5)
    p.add_argument("--icp-iterations", type=int, default=30)
    p.add_argument("--gicp-epsilon", type=float, default=1e-3, help="--refine gicp: covariance along a normal (1 across it)")
    p.add_argument("--normal-radius", type=float, default=1.0, help="--refine icp_plane / gicp / fpfh_ransac: normal search radius")
    p.add_argument("--normal-max-nn", type=int, default=30, help="--refine icp_plane / gicp / fpfh_ransac: neighbours per normal at most")
    p.add_argument("--fpfh-radius", type=float, default=2.5, help="fpfh_ransac: FPFH search radius")
    p.add_argument("--fpfh-max-nn", type=int, default=100, help="fpfh_ransac: neighbours per FPFH row at most")
    p.add_argument("--noise-bound", type=float, default=0.01, help="teaser: noise bound in metres (eval.py:201)")
    p.add_argument("--inlier-selection", choices=["kcore", "none"], default="kcore", help="teaser: rows that enter the GNC-TLS fit")
    args = p.parse_args(argv)
    if args.pairs_per_call < 1:
        p.error("--pairs-per-call must be >= 1")

    files = sorted(glob.glob(os.path.join(args.features_dir, "*.npz")))
    pairs = []
    for f in files:
        seq, anc, pos = parse_name(f)
        if seq == 8 and anc == 15 and pos == 58:          # eval.py:92-94 ("delete bad data")
            continue
        num_corr = args.num_corr
        if args.method == "teaser":
            from lcrnet_amd.functional import TEASER_MAX_ROWS
            num_corr = TEASER_MAX_ROWS if num_corr is None else min(num_corr, TEASER_MAX_ROWS)
        d, pos_pts, anc_pts, scores = load_pair(f, num_corr, need_corr=args.method != "fpfh_ransac")
        if args.method == "fpfh_ransac":
            missing = [k for k in ("pos_points_f", "anc_points_f", "transform") if k not in d]
            if missing:
                sys.exit("registration_eval: --method fpfh_ransac needs %s in %s" % (", ".join(missing), f))
        if args.method == "ransac_featurematch":
            missing = [k for k in io.REGISTRATION_FEAT_KEYS + ("pos_points_f", "anc_points_f") if k not in d]
            if missing:
                sys.exit("registration_eval: --method ransac_featurematch needs %s in %s; write the pair files with "
                         "io_formats.save_registration(..., with_feats=True)" % (", ".join(missing), f))
        pairs.append((f, d, pos_pts, anc_pts, scores))

    t0 = time.perf_counter()
    if args.method == "lgr":
        est = [d["estimated_transform"] for _, d, _, _, _ in pairs]         # as stored (f32), like eval.py:171-175
    else:
        import torch
        device = torch.device("cuda", torch.cuda.current_device())
        est, fm_corr, fm_reject, tz_valid, tz_selected = [], [], [], [], []
        for g in range(0, len(pairs), args.pairs_per_call):
            group = pairs[g:g + args.pairs_per_call]
            if args.method == "ransac_featurematch":
                T, nc, rej = estimate_featurematch(group, args, device)
                est += list(T)
                fm_corr += list(nc)
                fm_reject.append(rej)
            elif args.method == "fpfh_ransac":
                T, nc = estimate_fpfh(group, args, device)
                est += list(T)
                fm_corr += list(nc)
            elif args.method == "teaser":
                T, ok, nsel = estimate_teaser([(a, b, s) for _, _, b, a, s in group], args, device)
                est += list(T)
                tz_valid += list(ok)
                tz_selected += list(nsel)
            else:
                est += list(estimate_group(args.method, [(a, b, s) for _, _, b, a, s in group], args, device))
    scored = est                                          # --write-back stores the method's own estimate, refined or not
    if args.refine:
        import torch
        scored = refine_icp(pairs, est, args, torch.device("cuda", torch.cuda.current_device()))
    seconds = time.perf_counter() - t0

    if args.method == "ransac" and args.write_back:
        for (f, d, _, _, _), T in zip(pairs, est):
            modified = dict(d)
            modified["estimated_transform_ransac"] = T
            np.savez(f, **modified)

    fine = [ev.fine_matching_metrics(b, a, d["transform"]) for _, d, b, a, _ in pairs if args.method != "fpfh_ransac" or len(b)]
    fm = {k: float(np.mean([x[k] for x in fine])) if fine else float("nan") for k in ("FMR", "IR", "IR@0.3", "IR@0.1", "num_corr")}
    reg = ev.registration_summary([d["transform"] for _, d, _, _, _ in pairs], scored)
    print("Pairs: %d" % len(files))
    coarse = coarse_block([d for _, d, _, _, _ in pairs])
    if coarse is not None:
        print("  Coarse Matching, NUM: {:.3f}, PIR: {:.3f}, RECALL: {:.3f}, HIT_RATIO: {:.3f}, PMR>0: {:.3f}".format(
            coarse["NUM"], coarse["PIR"], coarse["RECALL"], coarse["HIT_RATIO"], coarse["PMR>0"]))
    print("  Fine Matching, FMR: {:.4f}, IR: {:.3f}, IR@0.3: {:.3f}, IR@0.1: {:.3f}, num_Corr: {:.3f}".format(
        fm["FMR"], fm["IR"], fm["IR@0.3"], fm["IR@0.1"], fm["num_corr"]))
    print("  Registration, RR: {:.4f}, RRE: {:.3f}, RTE: {:.3f}, Rx: {:.3f}, Ry: {:.3f}, Rz: {:.3f}".format(
        reg["RR"], reg["RRE"], reg["RTE"], reg["Rx"], reg["Ry"], reg["Rz"]))
    out = {"method": args.method, "pairs": reg["pairs"], "accepted": reg["accepted"], "fine_matching": fm,
           "registration": {k: reg[k] for k in ("RR", "RRE", "RTE", "Rx", "Ry", "Rz")}, "seconds": seconds,
           "num_corr": args.num_corr, "seed": args.seed, "pairs_per_call": args.pairs_per_call}
    if coarse is not None:
        out["coarse_matching"] = coarse
    if args.method == "ransac":
        out["ransac"] = {"distance_threshold": args.distance_threshold, "ransac_n": args.ransac_n, "num_iterations": args.num_iterations}
    if args.method == "teaser":
        from lcrnet_amd import registration as reg_mod
        out["teaser"] = {"noise_bound": args.noise_bound, "cbar2": reg_mod.REF_TEASER_CBAR2, "gnc_factor": reg_mod.REF_TEASER_GNC_FACTOR,
                         "max_iterations": reg_mod.REF_TEASER_MAX_ITERATIONS, "cost_threshold": reg_mod.REF_TEASER_COST_THRESHOLD,
                         "inlier_selection": args.inlier_selection, "invalid": int(sum(1 for v in tz_valid if not v)),
                         "n_selected": float(np.mean(tz_selected)) if tz_selected else float("nan")}
    if args.method == "ransac_featurematch":
        rej = np.concatenate(fm_reject) if fm_reject else np.zeros((0, args.num_iterations), np.uint8)
        share = lambda code: float((rej == code).mean()) if rej.size else float("nan")
        out["ransac_featurematch"] = {"distance_threshold": args.distance_threshold, "ransac_n": args.ransac_n,
                                      "num_iterations": args.num_iterations, "mutual_filter": args.mutual_filter,
                                      "edge_similarity": args.edge_similarity,
                                      "num_corr": float(np.mean(fm_corr)) if fm_corr else float("nan"),
                                      "rejected": {"degenerate": share(1), "edge_length": share(2), "distance": share(3)}}
    if args.method == "fpfh_ransac":
        out["fpfh_ransac"] = {"normal_radius": args.normal_radius, "normal_max_nn": args.normal_max_nn, "fpfh_radius": args.fpfh_radius,
                              "fpfh_max_nn": args.fpfh_max_nn, "distance_threshold": args.distance_threshold, "ransac_n": args.ransac_n,
                              "num_iterations": args.num_iterations, "mutual_filter": args.mutual_filter,
                              "edge_similarity": args.edge_similarity, "num_corr": float(np.mean(fm_corr)) if fm_corr else float("nan")}
    if args.refine:
        out["refine"] = {"method": args.refine, "max_correspondence_distance": args.icp_distance, "max_iteration": args.icp_iterations}
        if args.refine in ("icp_plane", "gicp"):
            out["refine"].update(normal_radius=args.normal_radius, normal_max_nn=args.normal_max_nn)
        if args.refine == "gicp":
            out["refine"]["epsilon"] = args.gicp_epsilon
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
