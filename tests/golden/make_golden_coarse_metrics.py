"""Golden vectors for the coarse-matching metrics from the IMPORTED reference (build container only).

    python tests/golden/make_golden_coarse_metrics.py

Runs, unmodified, utils/utils/registration.py: evaluate_sparse_correspondences (:319-347) on seeded index lists, and restates the
meter of experiments/registration/eval.py:129-133, 249-255 (means of num / precision / recall / hit_ratio / float(precision > 0)) over
them.  Cases: random predictions with a planted share of hits, an empty prediction, an empty ground truth, duplicate predicted rows.
For compute_overlap (:196-202) the reference's get_nearest_neighbor passes n_jobs to cKDTree.query, which the installed scipy rejects,
so that function cannot be called as it is: the overlap entries are computed here with cKDTree.query WITHOUT that argument and the
reference's remaining two lines (apply_transform is imported).  Output: tests/golden/coarse_metrics_golden.npz, a few KB.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
REF = "/root/reference"


def make_cases(seed=0):
    rng = np.random.default_rng(seed)
    cases = []
    for c in range(8):
        M, N = int(rng.integers(5, 40)), int(rng.integers(5, 40))
        n_gt, n_pred = int(rng.integers(1, 60)), int(rng.integers(1, 50))
        gt = np.stack([rng.integers(0, M, n_gt), rng.integers(0, N, n_gt)], 1)
        take = gt[rng.integers(0, n_gt, n_pred // 2)]                      # planted hits
        rnd = np.stack([rng.integers(0, M, n_pred - len(take)), rng.integers(0, N, n_pred - len(take))], 1)
        pred = np.concatenate([take, rnd])
        if c == 1:
            pred = np.zeros((0, 2), np.int64)                              # empty prediction
        if c == 2:
            gt = np.zeros((0, 2), np.int64)                                # empty ground truth
        if c == 3:
            pred = np.concatenate([pred, pred[:5], pred[:5]])              # duplicate predicted rows
        if c == 4:
            pred = rnd                                                     # (almost surely) no hit: PMR>0 = 0 for this pair
        cases.append((M, N, gt.astype(np.int64), pred.astype(np.int64)))
    return cases


def main():
    import make_golden_model as mgm
    mgm.install_stubs()
    sys.path.insert(0, REF)
    from scipy.spatial import cKDTree
    from utils.utils.registration import apply_transform, evaluate_sparse_correspondences
    out = {}
    cases = make_cases()
    rows = []
    for c, (M, N, gt, pred) in enumerate(cases):
        r = evaluate_sparse_correspondences(np.zeros((M, 3)), np.zeros((N, 3)), pred[:, 0], pred[:, 1], gt)
        out["c%d_shape" % c] = np.array([M, N], np.int64)
        out["c%d_gt" % c] = gt
        out["c%d_pred" % c] = pred
        rows.append([len(pred), r["precision"], r["recall"], r["hit_ratio"], float(r["precision"] > 0)])
    rows = np.array(rows, np.float64)
    out["per_pair"] = rows                                                 # num, precision, recall, hit_ratio, PMR>0
    out["summary"] = rows.mean(0)                                          # eval.py:249-255: the meter's means
    rng = np.random.default_rng(1)
    for c in range(3):
        radius = [0.6, 0.3, 0.1][c]
        ref = rng.uniform(-20, 20, (int(rng.integers(30, 60)), 3)).astype(np.float32)
        src = ref[rng.integers(0, len(ref), int(rng.integers(30, 60)))]
        src = (src + rng.normal(scale=0.6 * radius, size=src.shape)).astype(np.float32)
        T = np.eye(4)
        a = rng.uniform(0, np.pi)
        T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
        T[:3, 3] = rng.uniform(-3, 3, 3)
        src_in = ((src.astype(np.float64) - T[:3, 3]) @ T[:3, :3]).astype(np.float32)          # T maps src_in back onto src
        moved = apply_transform(src_in, T)
        dist, _ = cKDTree(moved).query(ref, k=1)                           # get_nearest_neighbor without n_jobs
        out["ov%d_ref" % c], out["ov%d_src" % c], out["ov%d_T" % c] = ref, src_in, T
        out["ov%d_radius" % c] = np.float64(radius)
        out["ov%d_overlap" % c] = np.float64(np.mean(dist < radius))
        out["ov%d_margin" % c] = np.float64(np.mean(np.abs(dist - radius) < 1e-4))             # share of ref points within 1e-4 of the radius
    path = os.path.join(HERE, "coarse_metrics_golden.npz")
    np.savez_compressed(path, **out)
    print("cases", len(cases), "summary", out["summary"], "overlaps", [float(out["ov%d_overlap" % c]) for c in range(3)],
          "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
