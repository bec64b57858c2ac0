"""GPU: the deterministic correspondence RANSAC (csrc/ransac.hip, lcr_ransac_correspondences) against the fp64 restatement of
tests/ransac_restatement.py — per hypothesis, on planted motion, on the reference's own correspondences at the reference's settings
(0.3 m / 4 points / 50 000 iterations), batch against single calls, degenerate pairs inside a batch, and tools/registration_eval.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ransac_restatement as rr
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

BORDER = 1e-5        # m: rows whose fp64 distance lies this close to the threshold may be decided either way by the fp32 score


def run(pairs, thr, k, iters, seed=0, details=False):
    from lcrnet_amd import functional as F
    lens = [len(s) for s, _ in pairs]
    start = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32).cuda()
    cat = lambda j: torch.from_numpy(np.concatenate([p[j] for p in pairs]).reshape(-1, 3).astype(np.float32)).cuda()
    out = F.ransac_correspondences(cat(0), cat(1), start, thr, k, iters, seed, want_details=details)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def borderline(src, ref, R, t, thr):
    """per hypothesis: number of rows whose fp64 distance is within BORDER of thr"""
    src, ref = src.astype(np.float64), ref.astype(np.float64)
    out = np.zeros(len(R), np.int64)
    for a in range(0, len(R), 256):
        d = np.linalg.norm(np.matmul(src[None], np.transpose(R[a:a + 256], (0, 2, 1))) + t[a:a + 256, None] - ref[None], axis=2)
        out[a:a + 256] = (np.abs(d - thr) < BORDER).sum(axis=1)
    return out


def golden_pair(name):
    g = np.load(os.path.join(GOLDEN, name))
    return g["anc_corr_points"], g["pos_corr_points"], g


def test_per_hypothesis_parity_with_the_restatement():
    from lcrnet_amd import functional as F
    p5 = rr.planted_pair(5, 0.0, 0.01, seed=4)[:2]
    s1, r1, _, _ = rr.planted_pair(1000, 0.5, 0.05, seed=5)
    s3, r3, _ = golden_pair("pose_e2e_rot3_golden.npz")
    pairs = [p5, (s1, r1), (s3, r3)]
    thr, k, iters, seed = 0.3, 4, 2000, 77
    T, inl, rmse, best, T_all, counts, sse = run(pairs, thr, k, iters, seed, details=True)
    for s, (src, ref) in enumerate(pairs):
        assert np.array_equal(F.ransac_sample_host(seed, 0, iters, k, len(src)), rr.sample(seed, np.arange(iters), k, len(src)))
        want = rr.ransac(src, ref, thr, k, iters, seed)
        sl = slice(s * iters, (s + 1) * iters)
        c, e, Ta = counts[sl], sse[sl], T_all[sl]
        valid = c >= 0
        assert np.array_equal(valid, want["valid"]), s
        if s == 0:
            assert 0 < valid.sum() < iters                    # 5 rows drawn 4 times: two distinct rows (collinear) happen
        assert np.abs(Ta[valid, :3, :3] - want["R"][valid]).max() < 1e-5
        assert np.abs(Ta[valid, :3, 3] - want["t"][valid]).max() < 1e-5 * max(1.0, np.abs(want["t"]).max())
        assert np.array_equal(Ta[~valid], np.broadcast_to(np.eye(4, dtype=np.float32), Ta[~valid].shape))
        bl = borderline(src, ref, want["R"], want["t"], thr)
        dc = np.abs(c - want["counts"])
        assert (dc[valid] <= bl[valid]).all(), (s, int(dc.max()))
        assert np.allclose(e[valid], want["sse"][valid], rtol=1e-3, atol=thr * thr * bl[valid] + 1e-4)
        b, wb = int(best[s]), want["best_h"]
        assert b == wb or abs(int(want["counts"][b]) - int(want["counts"][wb])) <= bl[b] + bl[wb], (s, b, wb)
        assert int(inl[s]) == int(c[b]) and np.array_equal(T[s], Ta[b])
        assert rmse[s] == pytest.approx(np.sqrt(np.float64(e[b]) / c[b]), rel=1e-6)
        # the winner is the best of the device's own scores in the stated total order
        order = np.lexsort((np.arange(iters), e, -c))
        assert order[0] == b


def test_planted_motion_is_recovered():
    from lcrnet_amd import evaluation as ev
    src, ref, Tp, _ = rr.planted_pair(4000, 0.7, 0.02, seed=21)
    T, inl, rmse, best = run([(src, ref)], 0.3, 4, 50000)
    rre, rte = ev.compute_registration_error(Tp, T[0].astype(np.float64))[:2]
    print("planted: RRE %.4f deg RTE %.4f m, %d inliers, rmse %.4f" % (rre, rte, inl[0], rmse[0]))
    assert rre < 0.5 and rte < 0.1
    d = np.linalg.norm(src.astype(np.float64) @ Tp[:3, :3].T + Tp[:3, 3] - ref, axis=1)
    # rows whose distance under the planted motion and under the estimate fall on different sides of 0.3 m: both lie near it
    de = np.linalg.norm(src.astype(np.float64) @ T[0, :3, :3].T.astype(np.float64) + T[0, :3, 3] - ref, axis=1)
    assert abs(int(inl[0]) - int((d < 0.3).sum())) <= int(((d < 0.3) != (de < 0.3)).sum())
    assert abs(int(inl[0]) - int((d < 0.3).sum())) <= 5


def test_reference_correspondences_at_the_reference_settings():
    """rot3 (3 deg about z + (1.6, -0.9, 0.12) m planted; the reference's correspondences of a seeded-weight model): eval.py accepts it
    (RRE < 5 deg, RTE < 2 m), and the tighter bounds come from the fp64 restatement with the same seed: RRE 0.014 deg, RTE 0.0026 m,
    754 inliers (hypothesis 47406) -> RRE < 0.1 deg (fp32 rotation entries put a floor of ~0.03 deg under the acos form), RTE < 0.01 m,
    754 +- 3 inliers.
    The demo pair (scans 003854 / 000958 through the same seeded-weight model; its correspondences are mostly noise) is NOT registered
    by a 4-point RANSAC at these settings: the reference's own LGR pose has only 18 inliers at 0.3 m among 4 060 correspondences, so a
    hypothesis drawn from 4 of them turns up with probability (18 / 4060)^4 * 50 000 ~ 2e-5.  The restatement's best hypothesis
    (9092) has 9 inliers and lies 6.2 deg / 10.8 m from the LGR pose.  Here the device must reproduce that winner, and LGR's pose must score
    more inliers under the same rule than any hypothesis RANSAC drew (the scoring is not what fails)."""
    from lcrnet_amd import evaluation as ev
    s, r, g = golden_pair("pose_e2e_rot3_golden.npz")
    s2, r2, g2 = golden_pair("pose_golden.npz")
    T, inl, rmse, best = run([(s, r), (s2, r2)], 0.3, 4, 50000)
    gt = np.linalg.inv(g["planted_transform"])                  # planted: positive -> anchor; RANSAC maps anchor (src) onto positive
    rre, rte = ev.compute_registration_error(gt, T[0].astype(np.float64))[:2]
    print("rot3: RRE %.4f deg RTE %.4f m, %d inliers (h %d)" % (rre, rte, inl[0], best[0]))
    assert rre < 5 and rte < 2
    assert rre < 0.1 and rte < 0.01 and abs(int(inl[0]) - 754) <= 3
    lgr = g2["estimated_transform"].astype(np.float64)
    d_lgr = np.linalg.norm(s2.astype(np.float64) @ lgr[:3, :3].T + lgr[:3, 3] - r2, axis=1)
    rre2, rte2 = ev.compute_registration_error(lgr, T[1].astype(np.float64))[:2]
    print("demo pair: %d inliers (h %d), LGR pose %d inliers; RANSAC vs LGR %.2f deg / %.2f m" % (inl[1], best[1], (d_lgr < 0.3).sum(), rre2, rte2))
    assert int(best[1]) == 9092 and int(inl[1]) == 9
    assert int((d_lgr < 0.3).sum()) >= 2 * int(inl[1])


def test_batch_equals_single_calls_bitwise():
    pairs = []
    for i in range(16):
        n = [4096, 1000, 7, 333, 2048][i % 5] + i
        src, ref, _, _ = rr.planted_pair(n, 0.3 + 0.04 * i, 0.03, seed=100 + i)
        pairs.append((src, ref))
    a = run(pairs, 0.3, 4, 3000, seed=5, details=True)
    b = run(pairs, 0.3, 4, 3000, seed=5, details=True)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    for i, p in enumerate(pairs):
        one = run([p], 0.3, 4, 3000, seed=5)
        for x, y in zip(one, a[:4]):
            assert np.array_equal(x[0:1].view(np.uint8), y[i:i + 1].view(np.uint8)), i
    assert (a[1] > 0).all()


def test_degenerate_pairs_inside_a_batch():
    k = np.arange(60, dtype=np.float32)[:, None]
    line = (k * np.array([1, 2, -1], np.float32), k * np.array([2, -1, 0.5], np.float32) + np.float32(3))   # exactly collinear in fp32
    good1 = rr.planted_pair(800, 0.4, 0.02, seed=1)[:2]
    good2 = rr.planted_pair(1200, 0.5, 0.02, seed=2)[:2]
    few = (good1[0][:3], good1[1][:3])
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    same = (np.full((50, 3), 2.5, np.float32), np.full((50, 3), -1.0, np.float32))
    pairs = [good1, few, empty, same, line, good2]
    T, inl, rmse, best = run(pairs, 0.3, 4, 2000, seed=9)
    for i in (1, 2, 3, 4):
        assert np.array_equal(T[i], np.eye(4, dtype=np.float32)) and inl[i] == 0 and rmse[i] == 0 and best[i] == -1, i
    for i, p in ((0, good1), (5, good2)):
        one = run([p], 0.3, 4, 2000, seed=9)
        assert np.array_equal(one[0][0], T[i]) and one[1][0] == inl[i] and one[3][0] == best[i] and inl[i] > 300


def test_registration_with_ransac_from_correspondences_api():
    from lcrnet_amd import evaluation as ev
    from lcrnet_amd.registration import registration_with_ransac_from_correspondences as reg
    src, ref, Tp, _ = rr.planted_pair(1500, 0.5, 0.02, seed=8)
    T = reg(src, ref, distance_threshold=0.3, ransac_n=4, num_iterations=5000)
    assert T.dtype == np.float64 and T.shape == (4, 4)
    assert ev.compute_registration_error(Tp, T)[0] < 0.5
    perm = np.random.default_rng(0).permutation(len(src))
    corr = np.stack([perm, perm], axis=1)                         # [K,2] (src index, ref index) on shuffled clouds
    T2 = reg(torch.from_numpy(src[np.argsort(perm)]).cuda(), ref[np.argsort(perm)], corr, 0.3, 4, 5000)
    assert ev.compute_registration_error(Tp, T2)[0] < 0.5


def test_registration_eval_ransac_and_svd_end_to_end(tmp_path):
    paths = rr.save_golden_pair_files(str(tmp_path), os.path.join(GOLDEN, "pose_e2e_rot3_golden.npz"), copies=3)

    def ev_tool(*extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "registration_eval.py"), str(tmp_path)] + list(extra),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return json.loads(r.stdout.strip().splitlines()[-1])

    got = ev_tool("--method", "ransac", "--pairs-per-call", "2", "--write-back")
    assert got["pairs"] == 3 and got["registration"]["RR"] == 1.0 and got["registration"]["RRE"] < 0.1 and got["registration"]["RTE"] < 0.01
    for p in paths:
        assert np.load(p)["estimated_transform_ransac"].shape == (4, 4)
    # svd = corr_scores-weighted Procrustes over every correspondence.  With the seeded-weight model's scores 81 % of the weight sits on
    # outliers and the fit lands 4.4 deg / 5.6 m off (fp64 restatement below): eval.py rejects it, RR = 0.
    svd = ev_tool("--method", "svd")
    g = np.load(os.path.join(GOLDEN, "pose_e2e_rot3_golden.npz"))
    s, r, w = (g[k].astype(np.float64) for k in ("anc_corr_points", "pos_corr_points", "corr_scores"))
    w = w / (w.sum() + 1e-5)
    cs, cr = w @ s, w @ r
    U, _, Vt = np.linalg.svd(((s - cs) * w[:, None]).T @ (r - cr))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    Tw = np.eye(4)
    Tw[:3, :3], Tw[:3, 3] = R, cr - R @ cs
    from lcrnet_amd import evaluation as ev
    rre, rte = ev.compute_registration_error(g["transform_gt"], Tw)[:2]
    assert svd["pairs"] == 3 and svd["registration"]["RR"] == float(rre < 5 and rte < 2) == 0.0
    top = ev_tool("--method", "ransac", "--num_corr", "2000", "--seed", "3")
    assert top["fine_matching"]["num_corr"] == 2000 and top["pairs"] == 3
