"""CPU: FPFH without a GPU — the fp64 restatement (tests/fpfh_restatement.py) on a hand-computed case, its invariants, the condition the
GPU tests rely on (almost every row of their inputs is safe), and the host-side domain checks of lcr_fpfh_ws_bytes / lcr_fpfh (refused
before anything is launched)."""
import ctypes
import os

import numpy as np

import fpfh_restatement as fr
import normals_restatement as nr
from conftest import GOLDEN

EARG, ESPACE = -1, -2


def hist(**bins):
    h = np.zeros(33)
    for k, v in bins.items():
        h[int(k[1:])] = v
    return h


def test_hand_computed_three_points():
    # p0 at the origin, p1 one metre along x, p2 half a metre along y; n0 = n1 = z, n2 tilted toward p0 -> p2 by (0, 0.6, 0.8).
    # (p0, p1): n . dp = 0 on both sides, v = dp x n1 = -y, w = x, f = (atan2(0, 1), 0, 0) = 0: bins (5, 5, 5).
    # (p0, p2): a1 = 0, a2 = 0.6: swap, f2 = -0.6, v = -x, w = (0, -0.8, 0.6), f1 = 0, f0 = atan2(0.6, 0.8) = 0.6435:
    #           scaled (6.63, 5.5, 2.2): bins (6, 5, 2).  (p2, p0): a1 = -0.6, a2 = 0: no swap, the same v, w: bins (6, 5, 2).
    # p1 - p2 is 1.118 m apart: outside the radius of 1.1.
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 0.5, 0]], np.float32)
    nrm = np.array([[0, 0, 1], [0, 0, 1], [0, 0.6, 0.8]], np.float32)
    o = fr.fpfh(pts, nrm, 1.1, 10)
    assert o["count"].tolist() == [2, 1, 1]
    assert np.array_equal(o["spfh"][0], hist(b5=50, b6=50, b16=100, b24=50, b27=50))
    assert np.array_equal(o["spfh"][1], hist(b5=100, b16=100, b27=100))
    assert np.array_equal(o["spfh"][2], hist(b6=100, b16=100, b24=100))
    # row 0: acc = spfh(1) / 1 + spfh(2) / 0.25 -> block 0 (100, 400) * 100 / 500 = (20, 80), plus its own (50, 50)
    assert np.allclose(o["features"][0], hist(b5=70, b6=130, b16=200, b24=130, b27=70), rtol=0, atol=1e-12)
    # rows 1 and 2: one neighbour, so the weight cancels: spfh(0) scaled to 100 per block, plus their own
    assert np.allclose(o["features"][1], hist(b5=150, b6=50, b16=200, b24=50, b27=150), rtol=0, atol=1e-12)
    assert np.allclose(o["features"][2], hist(b5=50, b6=150, b16=200, b24=150, b27=50), rtol=0, atol=1e-12)
    assert o["safe_fpfh"].all() and o["margin"].min() > 0.1


def test_blocks_sum_to_200_and_isolated_rows_are_zero():
    pts = np.concatenate([fr.scene_cloud(3)[::3], [[100.0, 100.0, 100.0]]]).astype(np.float32)
    nrm = nr.estimate_normals(pts, 0.6, 30)["normals"].astype(np.float32)
    o = fr.fpfh(pts, nrm, 0.6, 32)
    n = len(pts)
    has = ((o["idx"] < n) & (o["d2"] != 0)).any(axis=1)
    assert has.sum() > 0.9 * n and not has[-1] and o["count"][-1] == 0
    blocks = o["features"].reshape(n, 3, 11).sum(axis=2)
    assert np.abs(blocks[has] - 200.0).max() < 1e-9
    assert np.abs(o["spfh"].reshape(n, 3, 11).sum(axis=2)[o["count"] > 0] - 100.0).max() < 1e-9
    assert not o["features"][o["count"] == 0].any() and not o["spfh"][o["count"] == 0].any()
    assert (o["votes"].reshape(n, 3, 11).sum(axis=2) == o["count"][:, None]).all()


def test_coincident_points_and_zero_normals_vote_bin_5():
    mid = hist(b5=100, b16=100, b27=100)
    dup = np.tile(np.array([[1.0, 2.0, 3.0]], np.float32), (6, 1))
    z = np.array([[0.0, 0.0, 1.0]], np.float32)
    o = fr.fpfh(dup, np.tile(z, (6, 1)), 0.5, 10)
    assert (o["count"] == 5).all() and np.array_equal(o["spfh"], np.tile(mid, (6, 1)))
    assert np.array_equal(o["features"], o["spfh"])                       # every neighbour has d2 == 0: nothing is added
    assert o["safe_fpfh"].all()
    # more coincident rows than max_nn: a late row is not in its own list, nothing is removed, m = max_nn
    many = fr.fpfh(np.tile(dup[:1], (8, 1)), np.tile(z, (8, 1)), 0.5, 4)
    assert many["count"].tolist() == [3, 3, 3, 3, 4, 4, 4, 4]
    rng = np.random.default_rng(2)
    pts = rng.uniform(-1, 1, (200, 3)).astype(np.float32)
    o = fr.fpfh(pts, np.zeros_like(pts), 0.6, 32)                         # zero normals: a1 = a2 = 0, v = dp x 0 = 0
    assert (o["count"] > 0).all() and np.array_equal(o["spfh"], np.tile(mid, (200, 1)))


def test_quarter_turn_and_exact_shift_leave_safe_rows_unchanged():
    # a motion that fp32 carries exactly: coordinates on a 2^-8 grid, a quarter turn about z ((x, y, z) -> (-y, x, z): d2 keeps its bits
    # because the first sum commutes) and a shift on the same grid.  Neighbourhoods are then identical and only fp64 rounding differs.
    pts = (np.round(fr.scene_cloud(5).astype(np.float64) * 256) / 256).astype(np.float32)
    nrm = nr.estimate_normals(pts, 0.6, 30)["normals"].astype(np.float32)
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    moved = (pts.astype(np.float64) @ R.T + np.array([3.0, -2.0, 0.5])).astype(np.float32)
    assert np.array_equal(moved.astype(np.float64), pts.astype(np.float64) @ R.T + np.array([3.0, -2.0, 0.5]))
    a = fr.fpfh(pts, nrm, 0.6, 32)
    b = fr.fpfh(moved, (nrm.astype(np.float64) @ R.T).astype(np.float32), 0.6, 32)
    assert np.array_equal(a["idx"], b["idx"]) and np.array_equal(a["d2"], b["d2"])
    safe = a["safe_fpfh"] & b["safe_fpfh"]
    assert safe.mean() > 0.99
    assert np.array_equal(a["votes"][a["safe_spfh"] & b["safe_spfh"]], b["votes"][a["safe_spfh"] & b["safe_spfh"]])
    assert np.abs(a["features"][safe] - b["features"][safe]).max() <= 1e-9


def gpu_test_inputs():
    """(name, points, normals by the restatement, radius, max_nn) of the inputs of tests/test_fpfh_gpu.py"""
    for name in ("000026", "003528"):
        crop = fr.nearest_rows(np.load(os.path.join(GOLDEN, "scans", name + ".npy")))
        nrm = nr.estimate_normals(crop, 0.9, 30)["normals"].astype(np.float32)
        for radius, max_nn in ((1.5, 100), (1.5, 32)):
            yield name, crop, nrm, radius, max_nn
    scene = fr.scene_cloud()
    yield "scene", scene, nr.estimate_normals(scene, 0.6, 30)["normals"].astype(np.float32), 0.6, 32


def test_gpu_test_inputs_are_almost_entirely_safe():
    seen = set()
    for name, pts, nrm, radius, max_nn in gpu_test_inputs():
        o = fr.fpfh(pts, nrm, radius, max_nn)
        unsafe = 1.0 - o["safe_fpfh"].mean()
        loose = 1.0 - (o["margin"] >= 1e-6).mean()
        print("%s r=%g max_nn=%d: unsafe for FPFH %.4f, rows with margin < 1e-6 %.4f, m max %d" % (name, radius, max_nn, unsafe, loose,
                                                                                                  o["count"].max()))
        assert unsafe <= 0.01, (name, radius, max_nn, unsafe)
        seen.add((name, o["count"].max() > 64, (o["count"] == max_nn - 1).mean() > 0.5))
    assert ("000026", True, False) in seen or ("003528", True, False) in seen     # the radius-limited path with more than 64 neighbours
    assert ("000026", False, True) in seen and ("003528", False, True) in seen    # the cap path


def test_ws_bytes_and_domain_checks_return_earg():
    from lcrnet_amd import _lib
    L = _lib.lib()
    nb = ctypes.c_size_t(0)
    assert L.lcr_fpfh_ws_bytes(16, 16 * 20000, 100, ctypes.byref(nb)) == 0
    grid = ctypes.c_size_t(0)
    assert L.lcr_support_grid_ws_bytes(16 * 20000, 16, ctypes.byref(grid)) == 0
    assert nb.value >= grid.value + 16 * 20000 * (100 * 4 + 33 * 8)
    for args in ((0, 10, 30), (65, 10, 30), (1, -1, 30), (1, 2**31, 30), (1, 10, 1), (1, 10, 129)):
        assert L.lcr_fpfh_ws_bytes(*args, ctypes.byref(nb)) == EARG, args
        assert b"lcr_fpfh_ws_bytes" in L.lcr_last_error()
    assert L.lcr_fpfh_ws_bytes(1, 10, 30, None) == EARG


def test_fpfh_domain_checks_return_earg():
    from lcrnet_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(256)                                        # never dereferenced: the checks come first

    def call(B=1, lens=(10,), r=0.5, nn=30, pts=fake, nrm=fake, out=fake, ws=fake, ws_bytes=1 << 40):
        ln = np.asarray(list(lens) + [0] * 64, np.int64)
        return L.lcr_fpfh(pts, nrm, ln.ctypes.data, B, r, nn, out, None, None, ws, ws_bytes, None)

    for kw in (dict(B=0), dict(B=65), dict(r=0.0), dict(r=-1.0), dict(r=float("nan")), dict(r=float("inf")), dict(r=1e20), dict(nn=1),
               dict(nn=129), dict(lens=(-1,)), dict(lens=(2**31,)), dict(B=2, lens=(2**31 - 1, 1)), dict(pts=None), dict(nrm=None),
               dict(out=None), dict(ws=None)):
        assert call(**kw) == EARG, kw
        assert b"lcr_fpfh" in L.lcr_last_error()
    assert call(ws_bytes=16) == ESPACE
