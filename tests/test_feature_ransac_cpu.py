"""CPU: the NumPy restatement of feature-matching RANSAC (tests/feature_ransac_restatement.py) against float64 brute force and hand-made
cases, the planted pairs the GPU tests run on, and the public signature of registration_with_ransac_from_feats."""
import inspect

import numpy as np
import pytest

import feature_ransac_restatement as fr

BORDER = 1e-5        # m, as tests/test_ransac_gpu.py: a sampled row this close to checker_distance may be decided either way in fp32


def unit_rows(rng, n, C):
    x = rng.normal(size=(n, C))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("C", [1, 3, 32, 33])
def test_restatement_nn_equals_float64_brute_force(C):
    rng = np.random.default_rng(C)
    q, d = unit_rows(rng, 300, C), unit_rows(rng, 257, C)
    nn, d2 = fr.feature_nn(q, d, chunk=64)
    best, m, second = fr.feature_nn_f64(q, d)
    clear = second - m > 1e-5 * np.maximum(m, 1e-30)
    assert clear.mean() > 0.9 or C == 1
    assert np.array_equal(nn[clear], best[clear])
    assert np.allclose(d2, ((q.astype(np.float64) - d[nn]) ** 2).sum(axis=1), rtol=1e-5, atol=1e-12)
    assert nn.dtype == np.int32 and d2.dtype == np.float32


def test_restatement_nn_ties_nan_and_empty():
    rng = np.random.default_rng(0)
    d = unit_rows(rng, 50, 8)
    d[31] = d[7]                                      # exact duplicate: the tie goes to row 7
    d[40] = d[12]
    q = np.concatenate([d[7:8], d[12:13], unit_rows(rng, 20, 8)])
    nn, d2 = fr.feature_nn(q, d)
    assert nn[0] == 7 and nn[1] == 12 and d2[0] == 0 and not np.isin(nn, [31, 40]).any()
    # NaN distances never win; a row whose every distance is NaN, and every row of an empty database, gets -1 / NaN
    d_nan = d.copy()
    d_nan[7, 3] = np.nan
    nn2, _ = fr.feature_nn(q, d_nan)
    assert nn2[0] == 31
    q_nan = q.copy()
    q_nan[5, 0] = np.nan
    nn3, d23 = fr.feature_nn(q_nan, d)
    assert nn3[5] == -1 and np.isnan(d23[5]) and np.array_equal(np.delete(nn3, 5), np.delete(nn, 5))
    nn4, d24 = fr.feature_nn(q, np.zeros((0, 8), np.float32))
    assert (nn4 == -1).all() and np.isnan(d24).all()
    assert d24.view(np.uint32)[0] == 0x7FC00000


def test_checker_unit_cases():
    rng = np.random.default_rng(1)
    s = rng.uniform(-10, 10, size=(1, 3, 3)).astype(np.float32)
    shrunk = (s * np.float32(0.85)).astype(np.float32)
    assert not fr.edge_check(s, shrunk, 0.9)[0] and fr.edge_check(s, shrunk, 0.8)[0]
    assert not fr.edge_check(shrunk, s, 0.9)[0]                       # the check is symmetric
    ang = 0.7
    Rz = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    moved = (s.astype(np.float64) @ Rz.T + np.array([1.0, -2.0, 0.5])).astype(np.float32)
    assert fr.edge_check(s, moved, 0.9)[0]                            # congruent
    assert fr.edge_check(s, shrunk, 0.0)[0]                           # <= 0: off
    # exactly ls2 == k2 * lr2 passes: k = 0.5 (k2 = 0.25 exact), ref edges of length 4, src edges of length 2, all exact in float32
    r = np.array([[[0, 0, 0], [4, 0, 0], [0, 4, 0]]], np.float32)
    assert fr.edge_check(r * np.float32(0.5), r, 0.5)[0]
    assert not fr.edge_check(r * np.float32(0.5), r, np.nextafter(np.float32(0.5), np.float32(1)))[0]
    # distance checker: one sampled row 0.4 m off under the hypothesis fails at 0.3 and passes at 0.5
    R, t = np.eye(3)[None], np.zeros((1, 3))
    off = s.copy()
    off[0, 1, 0] += np.float32(0.4)
    ok3, dist = fr.distance_check(s, off, R, t, 0.3)
    ok5, _ = fr.distance_check(s, off, R, t, 0.5)
    assert not ok3[0] and ok5[0] and abs(dist[0, 1] - 0.4) < 1e-5 and fr.distance_check(s, off, R, t, 0.0)[0][0]


def test_mutual_filter_and_its_fallback():
    nn_sr = np.array([2, 0, 1, 1, -1, 3], np.int32)
    nn_rs = np.array([1, 2, 0, 4], np.int32)
    rows, used = fr.correspondences(nn_sr, None, n_ref=4, min_rows=3)
    assert not used and rows.tolist() == [[0, 2], [1, 0], [2, 1], [3, 1], [5, 3]]
    rows, used = fr.correspondences(nn_sr, nn_rs, n_ref=4, min_rows=3)
    assert used and rows.tolist() == [[0, 2], [1, 0], [2, 1]]                     # exactly min_rows mutual rows: the filter holds
    rows, used = fr.correspondences(nn_sr, nn_rs, n_ref=4, min_rows=4)
    assert not used and rows.tolist() == [[0, 2], [1, 0], [2, 1], [3, 1], [5, 3]]   # one short: back to the unfiltered set
    rows, used = fr.correspondences(np.zeros(0, np.int32), np.zeros(0, np.int32), n_ref=0, min_rows=3)
    assert rows.shape == (0, 2) and not used


def pose_error(Tp, T):
    dR = Tp[:3, :3].T @ T[:3, :3]
    return np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))), np.linalg.norm(Tp[:3, 3] - T[:3, 3])


@pytest.mark.parametrize("k", range(len(fr.PLANTED)))
def test_planted_feature_pairs_are_fit_for_the_gpu_tests(k):
    """The restatement alone on the pairs the GPU tests use (0.3 m, 4 000 iterations, seed 3, edge check 0.9, distance check 0.3 m):
      pair 0 (n 2000, overlap 0.35, feat_noise 0.15, seed 11, ransac_n 3): inlier share of the 2 000 feature correspondences 0.209
        (0.351 of the 1 029 mutual ones); winner h 2780 with 419 inliers, 0.022 deg / 0.013 m from the planted pose; rejected: 0.08 %
        degenerate, 98.35 % edge, 0.33 % distance, 1.25 % reach scoring;
      pair 1 (n 1500, overlap 0.4, feat_noise 0.15, seed 12, ransac_n 4): inlier share 0.252 (0.398 mutual); winner h 3348 with 378
        inliers, 0.027 deg / 0.010 m; 99.38 % edge, 0.10 % distance, 0.53 % reach scoring.
    No sampled row lies within 1e-5 m of the distance checker's threshold in either, so no hypothesis' reject code is exempt."""
    cfg = dict(fr.PLANTED[k])
    rn = cfg.pop("ransac_n")
    sp, rp, sf, rf, T, match = fr.planted_feature_pair(**cfg)
    assert np.allclose(np.linalg.norm(sf, axis=1), 1, atol=1e-5) and np.allclose(np.linalg.norm(rf, axis=1), 1, atol=1e-5)
    for mutual in (False, True):
        out = fr.feature_ransac(sp, rp, sf, rf, fr.PLANTED_THR, rn, fr.PLANTED_ITERS, fr.PLANTED_SEED, mutual_filter=mutual)
        c = out["corr"]
        d = np.linalg.norm(sp[c[:, 0]].astype(np.float64) @ T[:3, :3].T + T[:3, 3] - rp[c[:, 1]], axis=1)
        share = float((d < fr.PLANTED_THR).mean())
        rre, rte = pose_error(T, out["T"])
        exempt = int((np.abs(out["sample_dist"] - fr.PLANTED_THR) < BORDER).any(axis=1).sum())
        print("pair %d mutual %d: %d corr, inlier share %.3f, winner %d with %d inliers, %.4f deg / %.4f m, reject shares %s, exempt %d" % (
            k, mutual, len(c), share, out["best_h"], out["inliers"], rre, rte,
            (np.bincount(out["reject"], minlength=4) / fr.PLANTED_ITERS).round(4).tolist(), exempt))
        assert 0.05 <= share <= 0.40
        assert rre < 0.5 and rte < 0.1
        assert exempt <= 0.01 * fr.PLANTED_ITERS
        assert out["mutual_used"] == mutual and (len(c) == len(sp)) == (not mutual)
        assert 0 < (out["reject"] == fr.REJECT_VALID).sum() < fr.PLANTED_ITERS and (out["reject"] == fr.REJECT_EDGE).any() \
            and (out["reject"] == fr.REJECT_DISTANCE).any()


def test_registration_with_ransac_from_feats_has_the_reference_signature():
    from lcrnet_amd import registration
    sig = inspect.signature(registration.registration_with_ransac_from_feats)
    names = list(sig.parameters)
    assert names[:8] == ["src_points", "ref_points", "src_feats", "ref_feats", "distance_threshold", "ransac_n", "num_iterations",
                         "val_iterations"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["distance_threshold"], d["ransac_n"], d["num_iterations"], d["val_iterations"]) == (0.05, 3, 50000, 1000)
    assert d["mutual_filter"] is False and d["seed"] == 0
    b = inspect.signature(registration.ransac_from_feats_batched).parameters
    assert list(b)[:9] == ["src_points", "ref_points", "src_feats", "ref_feats", "src_len", "ref_len", "distance_threshold", "ransac_n",
                           "num_iterations"]
    assert b["mutual_filter"].default is False and b["edge_similarity"].default == 0.9 and b["seed"].default == 0


def test_new_entries_validate_their_arguments():
    """The C ABI refuses what lies outside the stated domains (no GPU needed: the checks run before any launch)."""
    import ctypes
    from lcrnet_amd import _lib
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.lcr_feature_nn_ws_bytes(1, 100, 100, ctypes.byref(n)) == 0 and n.value > 0
    assert L.lcr_feature_nn_ws_bytes(0, 100, 100, ctypes.byref(n)) != 0
    assert L.lcr_feature_nn_ws_bytes(65536, 100, 100, ctypes.byref(n)) != 0
    small, big = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.lcr_feature_nn_ws_bytes(1, 12000, 12000, ctypes.byref(small)) == 0
    assert small.value < 12000 * 12000                     # never an nq x nd matrix
    one = ctypes.c_void_p(256)                             # a non-null placeholder: the domain check comes first
    assert L.lcr_feature_nn(one, one, one, one, 1, 0, 10, 10, one, one, one, 1 << 30, None) != 0        # C < 1
    assert L.lcr_feature_nn(one, one, one, one, 1, 1025, 10, 10, one, one, one, 1 << 30, None) != 0     # C > 1024
    assert L.lcr_feature_nn(one, one, one, one, 1, 32, 10, 10, one, one, one, 16, None) != 0            # workspace too small
    assert L.lcr_ransac_ex_ws_bytes(2, 1000, 500, ctypes.byref(big)) == 0 and L.lcr_ransac_ws_bytes(2, 1000, ctypes.byref(small)) == 0
    assert big.value > small.value
    assert L.lcr_ransac_ex_ws_bytes(2, 1000, -1, ctypes.byref(big)) != 0
    args = lambda edge, dist: (one, one, one, 1, None, None, None, 0, 0.3, 3, 100, 0, edge, dist, one, one, one, None, None, None, None, None,
                               one, 1 << 30, None)
    assert L.lcr_ransac_correspondences_ex(*args(float("nan"), 0.0)) != 0
    assert L.lcr_ransac_correspondences_ex(*args(0.9, float("inf"))) != 0
    assert L.lcr_feature_correspondences_ws_bytes(0, ctypes.byref(n)) != 0
    assert L.lcr_feature_correspondences(one, one, None, one, 1, -1, one, one, None, one, 1 << 20, None) != 0
