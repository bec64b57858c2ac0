#!/usr/bin/env python
"""Loop ground truth of a sequence from its scans and poses (lcrnet_amd.loop_gt; csrc/scan_overlap.hip): the range-image overlap labels
that evaluation.compute_topN / compute_PR_overlap consume and the distance-based loop pairs that the registration half reads; one JSON line.

    python tools/loop_gt_run.py --poses poses/00.txt --calib sequences/00/calib.txt --scans sequences/00/velodyne [--out DIR]
    python tools/loop_gt_run.py --synthetic 64 [--pairs 256]

Real sequence: pose lines are KITTI's (12 numbers, a 3x4 in the CAMERA frame); with --calib the file's `Tr` (velodyne to camera) turns
them into sensor poses T = inv(Tr) P Tr, without it they are taken as sensor poses.  Scans are `.bin` (velodyne rows) or `.npy` files in
name order, one per pose.  Writes `loop_gt_overlap{thres}.npz` (object array, entry i = the frames overlapping frame i by more than thres;
loop_detection_run.py --gt-labels reads it) and `loop_pairs_distance{dis}.npz` (io_formats.load_loop_pairs reads it).

--synthetic N: N frames of lcrnet_amd.synthetic scans (about 120 k points each) on a planted trajectory with a revisit; times ONE native
call of --pairs pairs at 64 x 900 (pairs per second, projected points per second) and the NumPy restatement on the same pairs beside it."""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses")
    ap.add_argument("--calib")
    ap.add_argument("--scans")
    ap.add_argument("--synthetic", type=int, default=0, help="number of synthetic frames (timing mode)")
    ap.add_argument("--pairs", type=int, default=256, help="pairs of the timed call (synthetic mode)")
    ap.add_argument("--restated-pairs", type=int, default=16, help="pairs the NumPy restatement is timed on (synthetic mode)")
    ap.add_argument("--out", default=".")
    ap.add_argument("--seq", type=int, default=0)
    ap.add_argument("--thres", type=float, default=0.3)
    ap.add_argument("--denom", choices=["current", "min"], default="current")
    ap.add_argument("--exclude", type=int, default=100, help="frames before i that are not candidates (the retrieval's exclusion window)")
    ap.add_argument("--H", type=int, default=64)
    ap.add_argument("--W", type=int, default=900)
    ap.add_argument("--fov-up", type=float, default=3.0)
    ap.add_argument("--fov-down", type=float, default=-25.0)
    ap.add_argument("--max-range", type=float, default=50.0)
    ap.add_argument("--eps", type=float, default=1.0)
    ap.add_argument("--loop-dis", type=float, default=4.0)
    ap.add_argument("--loop-start", type=int, default=100)
    ap.add_argument("--loop-gap", type=int, default=50)
    return ap.parse_args(argv)


def load_poses(path, calib=None):
    """KITTI pose lines -> f64 [F,4,4]; with a calib file's Tr: inv(Tr) P Tr"""
    rows = np.loadtxt(path, dtype=np.float64, ndmin=2)
    if rows.shape[1] != 12:
        raise SystemExit("%s: expected 12 numbers per pose line, got %d" % (path, rows.shape[1]))
    poses = np.tile(np.eye(4), (len(rows), 1, 1))
    poses[:, :3, :4] = rows.reshape(-1, 3, 4)
    if calib:
        Tr = None
        with open(calib) as f:
            for line in f:
                if line.startswith("Tr"):
                    Tr = np.eye(4)
                    Tr[:3, :4] = np.array(line.split(":", 1)[1].split(), dtype=np.float64).reshape(3, 4)
        if Tr is None:
            raise SystemExit("%s: no Tr line" % calib)
        poses = np.linalg.inv(Tr) @ poses @ Tr
    return poses


def run_sequence(args):
    from lcrnet_amd import io_formats, loop_gt
    poses = load_poses(args.poses, args.calib)
    files = sorted(glob.glob(os.path.join(args.scans, "*.bin")) + glob.glob(os.path.join(args.scans, "*.npy")))
    if len(files) != len(poses):
        raise SystemExit("%d scans in %s for %d poses" % (len(files), args.scans, len(poses)))
    proj = dict(H=args.H, W=args.W, fov_up=args.fov_up, fov_down=args.fov_down, max_range=args.max_range)
    clouds = [np.ascontiguousarray(io_formats.load_scan_rows(f, pin=False).numpy()[:, :3]) for f in files]
    pairs = loop_gt.candidate_pairs(poses, exclude=args.exclude, max_range=args.max_range)
    t0 = time.perf_counter()
    overlap, counts = loop_gt.scan_overlaps(np.concatenate(clouds), [len(c) for c in clouds], poses, pairs, denom=args.denom, eps=args.eps, **proj)
    t_ov = time.perf_counter() - t0
    labels = loop_gt.loop_labels_from_overlap(len(poses), pairs, overlap, args.thres)
    data = loop_gt.loop_pairs_by_distance(poses, dis=args.loop_dis, start=args.loop_start, gap=args.loop_gap, seq=args.seq)
    os.makedirs(args.out, exist_ok=True)
    f_lab = os.path.join(args.out, "loop_gt_overlap%g.npz" % args.thres)
    f_pairs = os.path.join(args.out, "loop_pairs_distance%g.npz" % args.loop_dis)
    loop_gt.save_loop_labels(f_lab, labels)
    loop_gt.save_loop_pairs(f_pairs, data)
    out = {"metric": "loop ground truth of a sequence", "frames": len(poses), "pairs": int(len(pairs)), "overlap_s": round(t_ov, 3),
           "pairs_per_s": round(len(pairs) / t_ov, 1) if t_ov > 0 else None, "labelled_frames": int(sum(len(l) > 0 for l in labels)),
           "labels": int(sum(len(l) for l in labels)), "thres": args.thres, "denom": args.denom, "projection": dict(proj, eps=args.eps),
           "loop_pair_frames": len(data), "loop_pairs": int(sum(len(d["pos_idx"]) for d in data)), "labels_file": f_lab, "loop_pairs_file": f_pairs}
    print(json.dumps(out), flush=True)
    return out


def run_synthetic(args):
    import torch
    import lcrnet_amd.synthetic as synthetic
    from lcrnet_amd import functional as F
    from lcrnet_amd import loop_gt
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import scan_overlap_restatement as R
    n = args.synthetic
    proj = dict(H=args.H, W=args.W, fov_up=args.fov_up, fov_down=args.fov_down, max_range=args.max_range)
    # a drive out and back: the second half revisits the first half's places, half a metre aside
    half = (n + 1) // 2
    poses = [R.pose(2.0 * k, 0.0, 3.0 * np.sin(k)) for k in range(half)] + [R.pose(2.0 * (n - 1 - k), 0.5, 180.0 + 3.0 * np.cos(k)) for k in range(half, n)]
    poses = np.stack(poses)
    base = [synthetic.synthetic_scan(2000 + u) for u in range(min(n, 4))]
    clouds = [base[k % len(base)] for k in range(n)]
    rng = np.random.default_rng(0)
    pairs = np.stack([rng.integers(0, n, args.pairs), rng.integers(0, n, args.pairs)], axis=1)
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {"metric": "range-image scan overlap, one call", "frames": n, "pairs": int(args.pairs), "image": [args.H, args.W],
           "points_per_scan": int(np.mean([len(c) for c in clouds]))}
    chunk = F.SCAN_OVERLAP_MAX_CLOUDS
    frames = np.arange(min(n, chunk))
    pts = torch.from_numpy(np.concatenate([clouds[f] for f in frames])).to(dev)
    ln = [len(clouds[f]) for f in frames]
    pr = torch.from_numpy((pairs % len(frames)).astype(np.int32)).to(dev)
    rel = torch.from_numpy(loop_gt.relative_transforms(poses, pairs % len(frames))).to(dev)
    images, valid = F.range_images(pts, ln, **proj)

    def timed(fn, steps=5):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(steps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    t_img = timed(lambda: F.range_images(pts, ln, **proj))
    t_ov = timed(lambda: F.scan_overlap(pts, ln, images, valid, pr, rel, eps=args.eps, **proj))
    counts, status = F.scan_overlap(pts, ln, images, valid, pr, rel, eps=args.eps, **proj)
    counts = counts.cpu().numpy()
    assert int(status.cpu()[0]) == 0
    projected = int(sum(ln[j] for j in (pairs[:, 1] % len(frames))))
    out.update(range_images_ms=round(t_img * 1e3, 3), scan_overlap_ms=round(t_ov * 1e3, 3), pairs_per_s=round(args.pairs / t_ov, 1),
               points_per_s=round(projected / t_ov, 1), mean_overlap=round(float(loop_gt.overlap_from_counts(counts).mean()), 4))
    k = min(args.restated_pairs, args.pairs)
    if k > 0:
        sub = pairs[:k] % len(frames)
        cl = [clouds[f] for f in frames]
        imgs = R.range_images(cl, **proj)
        t0 = time.perf_counter()
        w = R.scan_overlap(cl, sub, loop_gt.relative_transforms(poses, sub), images=imgs, eps=args.eps, **proj)
        t_np = (time.perf_counter() - t0) / k
        safe = w["margin"] >= R.MARGIN
        out.update(numpy_ms_per_pair=round(t_np * 1e3, 3), numpy_pairs_per_s=round(1.0 / t_np, 2), restated_pairs=int(k),
                   restated_pairs_equal=bool(np.array_equal(w["counts"][safe], counts[:k][safe])), restated_pairs_with_margin=int(safe.sum()))
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    args = parse(argv)
    if args.synthetic > 0:
        return run_synthetic(args)
    if not (args.poses and args.scans):
        raise SystemExit("give --poses FILE --scans DIR [--calib FILE], or --synthetic N")
    return run_sequence(args)


if __name__ == "__main__":
    main()
